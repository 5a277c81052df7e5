"""Every linear op reaches the same native entries, in the same order and with the same
arguments, as the revision ``linear_trace_golden.json`` was recorded in (``linear_trace.py``:
CPU tensors, the native layer stubbed out). No GPU."""
import json

import pytest

import linear_trace as T
from distributed_llm_inferencing_amd.ops import _native as N
from distributed_llm_inferencing_amd.ops import gemm as G

GOLDEN = json.loads(T.GOLDEN.read_text())
ENTRIES = ("dli_gemm", "dli_gemv_fp8", "dli_gemm_fp8_stream", "dli_gemm_grouped_list",
           "dli_gemm_grouped_gather", "dli_gemv_fused", "dli_gemv_fused_fp8")
SPLITS = {name: 11 for name in ("dli_gemm", "dli_gemv_fp8", "dli_gemm_fp8_stream")}  # arg index


def _native(case):
    return [e for e in case["trace"] if e[0] in N._SIGS]


def test_case_table_and_golden_agree():
    assert sorted(GOLDEN) == sorted(T.CASES)


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_trace_equals_golden(name):
    got, want = T.run_case(name), GOLDEN[name]
    if "raises" in want:
        assert got.get("raises") == want["raises"]
        assert _native(got) == []
    assert got == want


def test_error_cases_launch_nothing():
    errors = {k: v for k, v in GOLDEN.items() if "raises" in v}
    assert {k for k in errors if "stream-tile-on-bf16" in k} and len(errors) >= 4
    for k, v in errors.items():
        assert v["raises"] == "ValueError" and _native(v) == [], k


def test_golden_reaches_every_entry():
    seen = {e[0] for c in GOLDEN.values() for e in c["trace"]}
    assert set(ENTRIES) <= seen
    assert "bf16()" in seen and any(c["workspace"] for c in GOLDEN.values())


def _stream_fallbacks(prefix):
    """(forced splits, launched splits) of the cases under ``prefix`` whose forced stream tile
    ended on ``dli_gemm``."""
    out = []
    for k, c in GOLDEN.items():
        if k.startswith(prefix) and c["plan"] and c["plan"][0] in G.FP8_STREAM_TILES:
            out += [(c["plan"][1], e[1 + SPLITS[e[0]]]) for e in c["trace"] if e[0] == "dli_gemm"]
    return out


def test_golden_holds_both_fallback_rules():
    """A plain call falls back to the heuristic plan (its own split count); a slab call keeps
    the split count its consumer was sized for, also where the heuristic would split less."""
    plain, slab = _stream_fallbacks("gemm_native/"), _stream_fallbacks("slab_gemm/")
    assert any(forced != ran for forced, ran in plain)
    assert slab and all(forced == ran for forced, ran in slab)
    kept = GOLDEN["slab_gemm/fp8/M65/t70s4"]
    (gemm,) = [e for e in kept["trace"] if e[0] == "dli_gemm"]
    assert gemm[1 + SPLITS["dli_gemm"]] == 4 != G._heuristic(65, T.N0, T.K0, "splitk").splits


def test_golden_holds_both_slab_formats():
    fmts = {e[9] for c in GOLDEN.values() for e in c["trace"] if e[0] == "dli_splitk_add_rmsnorm"}
    assert fmts == {0, 1}
    rets = {c["trace"][-1][1] for k, c in GOLDEN.items()
            if k.startswith("slab_gemm/") and "raises" not in c}
    assert rets == {0, 1}
    assert any(e[0] == "dli_splitk_add_rmsnorm_route" for c in GOLDEN.values() for e in c["trace"])
