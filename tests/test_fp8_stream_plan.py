"""The FP8 stream tiles in the planner, without a GPU: they are no heuristic plan and no
``dli_gemm`` tile, they enter the autotuner's list exactly for an ``ops.Fp8Weight`` at
``GEMV_MAX_M`` < M <= ``FP8_STREAM_MAX_M``, every split obeys the slice rule, and
``Fp8Weight.stream_ok`` refuses what the kernel cannot take."""
import pytest
import torch

from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.ops import gemm as G
from distributed_llm_inferencing_amd.ops import reference as R

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
EPIS = ("none", "f32", "silu_mul", "bias_gelu", "bias", "splitk", "res")
# the tiles tile_ok answered True for before the stream tiles existed (silu_mul, res; every
# other epilogue: all but the SiLU-only GEMV tiles 29 / 58 / 59)
SILU_OK = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 20, 21, 22, 25, 26, 28,
           29, 31, 33, 34, 41, 45, 55, 58, 59, 61]
RES_OK = [30, 32, 56, 57]


def fp8_weight(N, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(N, K, generator=g).to(F8)
    s = torch.exp2(torch.rand(N // 16, -(-K // 128), generator=g) * 8 - 10).float()
    return ops.Fp8Weight(q, s)


def stream(plans):
    return [p for p in plans if p.tile in G.FP8_STREAM_TILES]


def test_stream_tiles_are_a_table_of_their_own():
    assert G.FP8_STREAM_MAX_M == 64 and len(G.FP8_STREAM_TILES) >= 2
    assert min(G.FP8_STREAM_TILES) >= 70
    assert len(set(G.FP8_STREAM_TILES.values())) == len(G.FP8_STREAM_TILES)   # distinct heights
    for t in G.FP8_STREAM_TILES:
        assert t not in G.TILE_TABLE and t not in G.TILES and t not in G.GEMV_TILES
        assert t not in G.SLAB16_TILES and t not in G.GEMV_RES_TILES
    assert "stream" not in G.EPI and len(G.EPI) == 7


def test_tile_ok_is_unchanged_for_every_pinned_tile():
    tiles = sorted(set(G.TILES) | set(G.GEMV_TILES))
    plain = [t for t in tiles if t not in (29, 58, 59)]
    for epi in EPIS + ("slab16",):
        want = SILU_OK if epi == "silu_mul" else RES_OK if epi == "res" else plain
        assert [t for t in tiles if G.tile_ok(t, epi)] == want, epi


def test_heuristic_never_returns_a_stream_tile():
    for M in (1, 4, 5, 8, 16, 17, 32, 48, 64, 65, 128, 512, 513, 2048):
        for N in (96, 512, 4096, 6144, 28672):
            for K in (512, 1024, 1040, 4096, 14336):
                for epi in EPIS:
                    assert G._heuristic(M, N, K, epi).tile not in G.FP8_STREAM_TILES


@pytest.mark.parametrize("epi", ["none", "f32", "silu_mul", "bias", "splitk"])
def test_autotune_list_has_stream_tiles_exactly_for_fp8_at_mid_m(epi):
    N, K = 6144, 4096
    for M in (5, 8, 16, 17, 32, 48, 64):
        plans = G.autotune_plans(M, N, K, epi, "fp8")
        assert {p.tile for p in stream(plans)} == set(G.FP8_STREAM_TILES), M
        # the default candidates are all still there, in their order, in front
        base = G.candidate_plans(M, N, K, epi)
        assert plans[:len(base)] == base and stream(base) == []
        assert not stream(G.autotune_plans(M, N, K, epi, None))          # a bf16 weight
    for M in (1, 4, 65, 128, 512):
        assert not stream(G.autotune_plans(M, N, K, epi, "fp8")), M
    # a candidates= callable (prefill) replaces the list: no stream tiles are appended
    for M in (8, 64):
        assert G.autotune_plans(M, N, K, epi, "fp8", G.prefill_candidates) == \
            G.prefill_candidates(M, N, K, epi)
    # wdt() is what autotune() passes
    assert G.wdt(fp8_weight(16, 128)) == "fp8" and G.wdt(torch.zeros(16, 128, dtype=BF)) is None


def test_no_stream_plans_for_the_epilogues_the_kernel_has_not():
    for epi in ("res", "bias_gelu", "slab16"):
        assert not stream(G.autotune_plans(8, 4096, 4096, epi, "fp8"))
    assert not stream(G.autotune_plans(8, 4112, 4096, "silu_mul", "fp8"))   # N % 32


def test_every_split_obeys_the_slice_rule():
    seen = set()
    for K in (512, 1024, 1040, 1152, 4096, 14336, 1032):
        for p in stream(G.autotune_plans(8, 4096, K, "splitk", "fp8")):
            assert p.splits in (1, 2, 4, 8) and K % 16 == 0 and K % p.splits == 0
            assert p.splits == 1 or (K // p.splits) % 128 == 0, (K, p)
            seen.add((K, p.splits))
    assert {(4096, 1), (4096, 2), (4096, 4), (4096, 8), (14336, 8), (1040, 1), (1152, 1),
            (512, 4)} <= seen
    assert not {(1040, 2), (1152, 2), (1152, 4), (512, 8), (1032, 1)} & seen


def test_stream_ok_truth_table():
    tiles = sorted(G.FP8_STREAM_TILES)
    w = fp8_weight(96, 1024)
    for t in tiles:
        for splits in (1, 2, 4, 8):
            assert w.stream_ok(5, G.GemmPlan("dli", t, splits))
            assert w.stream_ok(64, G.GemmPlan("dli", t, splits))
        assert not w.stream_ok(4, G.GemmPlan("dli", t, 1))
        assert not w.stream_ok(65, G.GemmPlan("dli", t, 1))
        assert not w.stream_ok(8, G.GemmPlan("dli", t, 16))          # 64-wide slices
        assert not fp8_weight(96, 1032).stream_ok(8, G.GemmPlan("dli", t, 1))   # K % 16
        assert fp8_weight(96, 1040).stream_ok(8, G.GemmPlan("dli", t, 1))
        assert not fp8_weight(96, 1040).stream_ok(8, G.GemmPlan("dli", t, 2))
        assert fp8_weight(96, 1152).stream_ok(8, G.GemmPlan("dli", t, 1))
        assert not fp8_weight(96, 1152).stream_ok(8, G.GemmPlan("dli", t, 2))   # 576-wide slices
    for t in (0, 30, 56):                                            # not a stream tile
        assert not w.stream_ok(8, G.GemmPlan("dli", t, 1))
    # the GEMV predicate does not take the stream tiles either
    assert not w.gemv_ok(4, G.GemmPlan("dli", tiles[0], 1))


def test_linear_on_a_cpu_tensor_is_the_reference_path():
    torch.manual_seed(0)
    w = fp8_weight(96, 1040, seed=3)
    wf = R.dequantize_weight(w.q, w.scale, torch.float32)
    for M in (4, 8, 64):
        x = (torch.randn(M, 1040) * 0.5).to(BF)
        assert torch.equal(ops.linear(x, w), R.linear(x, wf))
        assert torch.equal(ops.linear(x, w, epi="f32"), R.linear(x, wf, out_dtype=torch.float32))
        assert torch.equal(ops.linear(x, w, epi="silu_mul"), R.silu_mul(R.linear(x, wf)))
