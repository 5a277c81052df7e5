"""The FP8 LDS tiles (``G.FP8_TILE_TABLE``, ``dli_gemm_fp8_tiles``) in the planner, without a GPU."""
import pytest
import torch

from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.ops import gemm as G


def fp8_weight(N, K):
    return ops.Fp8Weight(torch.zeros(N, K).to(torch.float8_e4m3fn), torch.ones(N // 16, -(-K // 128)))


def tiled(plans):
    return [p for p in plans if p.tile in G.FP8_TILE_TABLE]


def test_the_tiles_are_a_table_of_their_own():
    assert G.FP8_TILE_TABLE == {72: (128, 128), 73: (128, 256)}
    assert G.FP8_TILE_MAX_M == 512 and G.FP8_STREAM_MAX_M == 64
    for table in (G.TILE_TABLE, G.TILES, G.GEMV_TILES, G.FP8_STREAM_TILES, G.SLAB16_TILES):
        assert not set(G.FP8_TILE_TABLE) & set(table)


@pytest.mark.parametrize("epi", ["none", "f32", "silu_mul", "bias", "splitk"])
def test_autotune_list_has_the_tiles_exactly_for_fp8_past_64_rows(epi):
    N, K = 6144, 4096
    for M in (65, 128, 512):
        plans = G.autotune_plans(M, N, K, epi, "fp8")
        assert {p.tile for p in tiled(plans)} == set(G.FP8_TILE_TABLE), M
        base = G.candidate_plans(M, N, K, epi)
        assert plans[:len(base)] == base and tiled(base) == []
        assert not tiled(G.autotune_plans(M, N, K, epi, None))           # a bf16 weight
    for M in (4, 64, 513):
        assert not tiled(G.autotune_plans(M, N, K, epi, "fp8")), M
    assert not tiled(G.autotune_plans(128, N, 1040, epi, "fp8"))          # K % 128
    for other in ("res", "bias_gelu", "slab16"):
        assert not tiled(G.autotune_plans(128, N, K, other, "fp8"))


def test_every_split_obeys_the_128_rule_and_the_grid_cap():
    seen = set()
    for K in (256, 512, 1024, 1152, 4096, 14336):
        for p in tiled(G.autotune_plans(128, 4096, K, "splitk", "fp8")):
            assert p.splits in (1, 2, 4, 8) and K % p.splits == 0
            assert (K // p.splits) % 128 == 0, (K, p)
            seen.add((K, p.splits))
    assert {(256, 2), (512, 4), (1024, 8), (1152, 1), (4096, 8), (14336, 8)} <= seen
    assert not {(256, 4), (512, 8), (1152, 2), (1152, 4)} & seen
    # 4 x 224 tiles of 128 x 128: split 8 would be 7168 workgroups, past 4 x the CUs
    big = tiled(G.autotune_plans(512, 28672, 4096, "none", "fp8"))
    assert G.GemmPlan("dli", 72, 1) in big and G.GemmPlan("dli", 72, 8) not in big
    assert not tiled(G.autotune_plans(128, 4112, 4096, "silu_mul", "fp8"))   # N % 32


def test_tiles_ok_truth_table():
    w = fp8_weight(96, 1024)
    for t in G.FP8_TILE_TABLE:
        for splits in (1, 2, 4, 8):
            assert w.tiles_ok(65, G.GemmPlan("dli", t, splits))
            assert w.tiles_ok(512, G.GemmPlan("dli", t, splits))
        assert not w.tiles_ok(64, G.GemmPlan("dli", t, 1))
        assert not w.tiles_ok(513, G.GemmPlan("dli", t, 1))
        assert not w.tiles_ok(128, G.GemmPlan("dli", t, 16))             # 64-wide slices
        assert not fp8_weight(96, 1040).tiles_ok(128, G.GemmPlan("dli", t, 1))   # K % 128
        assert fp8_weight(96, 1152).tiles_ok(128, G.GemmPlan("dli", t, 1))
        assert not fp8_weight(96, 1152).tiles_ok(128, G.GemmPlan("dli", t, 2))   # 576-wide slices
        assert not w.stream_ok(65, G.GemmPlan("dli", t, 1))
    for t in (2, 30, 70, 71):                                            # not one of the tiles
        assert not w.tiles_ok(128, G.GemmPlan("dli", t, 1))
