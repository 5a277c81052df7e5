"""The W4 stream tiles (74 / 75) in the planner and the kernel choice, without a GPU: they enter
the autotuner's list exactly for an ``ops.W4Weight`` at ``GEMV_MAX_M`` < M <= ``W4_STREAM_MAX_M``,
every split is whole 128-column groups, and ``_pick_kernel`` runs them on a ``W4Weight`` only."""
import pytest
import torch

from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.ops import gemm as G
from distributed_llm_inferencing_amd.ops import reference as R

BF = torch.bfloat16
TILES = (74, 75)
plan = lambda tile, splits=1: G.GemmPlan("dli", tile, splits)  # noqa: E731


def w4_weight(N, K):
    return ops.W4Weight(*R.pack_w4(torch.zeros(N, K, dtype=torch.uint8),
                                   torch.ones(N, K // 128, dtype=torch.float16),
                                   torch.zeros(N, K // 128, dtype=torch.uint8)))


def test_plans_ranges_and_slice_rule():
    assert G.W4_STREAM_TILES == {74: 64, 75: 128} and G.W4_STREAM_MAX_M == 64
    for t in TILES:
        assert t not in G.TILE_TABLE and t not in G.GEMV_TILES and t not in G.SLAB16_TILES
        assert t not in G.FP8_STREAM_TILES and t not in G.FP8_TILE_TABLE
    for M in (1, 4, 65, 512):
        assert G.w4_stream_plans(M, 4096, 4096, "none") == []
    for epi in ("res", "bias_gelu", "slab16"):
        assert G.w4_stream_plans(8, 4096, 4096, epi) == []
    assert G.w4_stream_plans(8, 4112, 4096, "silu_mul") == []           # N % 32
    want = {384: (1,), 640: (1,), 1024: (1, 2, 4, 8), 1152: (1,), 14336: (1, 2, 4, 8), 512: (1, 2, 4)}
    for K, splits in want.items():
        for M in (5, 64):
            got = G.w4_stream_plans(M, 4096, K, "splitk")
            assert got == [plan(t, s) for t in TILES for s in splits], (K, M)
    for M, N, K in ((1, 96, 512), (8, 6144, 4096), (2048, 4096, 4096)):
        for epi in ("none", "silu_mul", "splitk", "res"):
            assert G._heuristic(M, N, K, epi).tile not in TILES


@pytest.mark.parametrize("epi", ["none", "f32", "silu_mul", "bias", "splitk"])
def test_autotune_list_has_the_tiles_exactly_for_w4_at_mid_m(epi):
    N, K = 6144, 4096
    for M in (1, 4, 5, 16, 64, 65, 512):
        tiles = {p.tile for p in G.autotune_plans(M, N, K, epi, "w4")}
        assert tiles & set(TILES) == (set(TILES) if 4 < M <= 64 else set()), M
        assert not tiles & (set(G.FP8_STREAM_TILES) | set(G.FP8_TILE_TABLE))
        for wd in (None, "fp8"):
            assert not {p.tile for p in G.autotune_plans(M, N, K, epi, wd)} & set(TILES)
        base = G.candidate_plans(M, N, K, epi)
        assert G.autotune_plans(M, N, K, epi, "w4")[:len(base)] == base


@pytest.mark.parametrize("tile", TILES)
def test_pick_kernel(tile):
    w = w4_weight(64, 1024)
    x = lambda M: torch.zeros(M, 1024, dtype=BF)  # noqa: E731
    for M in (5, 64):
        for splits, epi in ((1, "none"), (2, "splitk"), (1, "silu_mul")):
            p = plan(tile, splits)
            assert w.mfma_ok(M, p)
            assert ops._pick_kernel(x(M), w, p, epi) == ("w4_stream", p, w)
    assert not w.mfma_ok(8, plan(tile, 16)) and not w.mfma_ok(8, plan(0)) \
        and not w.gemv_ok(4, plan(tile))
    # what the kernel cannot take runs a bf16-family plan on the dequantised weight
    deq = w.dequantize(BF)
    for M, kw in ((4, {}), (65, {}), (8, {"groups": 2})):
        kind, run, ww = ops._pick_kernel(x(M), w, plan(tile, 2), "splitk", **kw)
        assert kind == "gemm" and torch.equal(ww, deq) and run.tile in G.TILES | G.GEMV_TILES
    kind, run, _ = ops._pick_kernel(x(65), w, plan(tile, 4), "splitk", keep_splits=True)
    assert kind == "gemm" and run.tile in G.TILES and run.splits == 4
    odd = torch.zeros(8, 1025, dtype=BF)[:, :1024]                  # rows not 16-B aligned
    assert ops._pick_kernel(odd, w, plan(tile), "none")[0] == "gemm"
    # a non-stream tile on the same weight at the same rows keeps the dequantise path
    assert ops._pick_kernel(x(8), w, plan(0), "none")[0] == "gemm"
    for other in (torch.zeros(64, 1024, dtype=BF),
                  ops.Fp8Weight(torch.zeros(64, 1024).to(torch.float8_e4m3fn), torch.ones(4, 8))):
        with pytest.raises(ValueError, match=str(tile)):
            ops._pick_kernel(x(8), other, plan(tile), "none")
