"""The views derived from ops.gemm.TILE_TABLE equal the literals they replaced."""
from distributed_llm_inferencing_amd.ops import gemm as G

TILES = {0: (64, 64), 1: (64, 128), 2: (128, 128), 3: (128, 256), 4: (256, 128),
         5: (64, 64), 6: (64, 128), 7: (128, 128), 8: (128, 256), 9: (256, 128),
         10: (192, 128), 11: (192, 128), 12: (160, 128),
         13: (256, 256), 14: (256, 128), 15: (128, 256), 16: (256, 128), 17: (128, 256),
         18: (128, 96), 19: (128, 96), 20: (128, 64), 21: (128, 64),
         22: (256, 256),
         23: (128, 192), 24: (128, 192), 25: (256, 192),
         26: (256, 224),
         28: (256, 128),
         60: (128, 192), 61: (128, 256),
         34: (256, 256), 41: (256, 256), 45: (256, 256),
         55: (256, 256)}
TILE_WAVES = {13: (2, 4), 14: (4, 2), 15: (2, 4), 16: (4, 2), 17: (2, 4),
              22: (2, 4), 23: (2, 4), 24: (2, 4), 25: (4, 2),
              26: (4, 2), 28: (4, 2), 60: (2, 4), 61: (2, 4)}
SLAB16_TILES = frozenset(list(range(0, 22)) + [22, 23, 24, 25, 26, 28, 60, 61])
GATHER_TILES = frozenset(list(range(0, 22)) + [23, 24, 25, 60, 61])

# tile_ok(tile, epi) is True exactly for these tiles (MFMA tiles and GEMV tiles together)
_PLAIN = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23,
          24, 25, 26, 28, 30, 31, 32, 33, 34, 41, 45, 55, 56, 57, 60, 61]
TILE_OK = {"none": _PLAIN, "f32": _PLAIN, "bias_gelu": _PLAIN, "bias": _PLAIN,
           "splitk": _PLAIN, "slab16": _PLAIN,
           "silu_mul": [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 20, 21, 22,
                        25, 26, 28, 29, 31, 33, 34, 41, 45, 55, 58, 59, 61],
           "res": [30, 32, 56, 57]}


def test_derived_views_equal_the_literals():
    assert G.TILES == TILES
    assert list(G.TILES) == list(TILES)          # the autotuner walks the tiles in this order
    assert G.TILE_WAVES == TILE_WAVES
    assert G.SLAB16_TILES == SLAB16_TILES
    assert G.GATHER_TILES == GATHER_TILES


def test_tile_ok_over_every_tile_and_epilogue():
    assert set(TILE_OK) == set(G.EPI) | {"res"}
    tiles = sorted(set(G.TILES) | set(G.GEMV_TILES))
    for epi, ok in TILE_OK.items():
        assert [t for t in tiles if G.tile_ok(t, epi)] == ok, epi
