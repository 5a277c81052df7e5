"""Exact integer witnesses for the bf16 GEMM, GEMV and grouped kernels (CPU side: builders,
float64 expectations, the case lists of tests/test_kernels_gemm_witness_gpu.py and a numpy
model of a tiled split-K GEMM whose mutations tests/test_gemm_witness.py runs).

The inputs are small integers stored as bf16, so every product and every partial sum is an
integer below 2^24: the fp32 accumulators hold the exact result whatever the MFMA order, the
split count or the slab format, and the check is equality with a float64 matmul, not a
tolerance.

* narrow: x, w in {-1, +1}. Every product is odd, so one dropped or doubled term moves the sum
  by an odd integer. |sum| <= CAP (255: exact in bf16) and every split-K slice <= SLICE_CAP
  (2048: exact in fp16 after the slab's 1/16) are asserted on the reference before a launch;
  the seed is the first for which they hold, the data are never clamped.
* wide: x, w in {+-1, +-3}: fp32 outputs and slabs, and bf16 outputs against the
  round-to-nearest-even image of sums beyond 256 (csrc/kernels/common.h f2bf).
* SiLU*up: a gate row has one nonzero weight, a power of two, in a column where every x row is
  1, so the gate is 32, 64 or 128, where x / (1 + exp(-x)) == x in fp32: the output is
  bf16(gate * up) exactly.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np
import torch

from distributed_llm_inferencing_amd.ops import gemm as G

BF = torch.bfloat16
CAP = 255
NARROW_CAP = CAP - 40           # what the seed search asks of x @ w.T: room for a bias / residual
SLICE_CAP = 2048
BK = 64
GATES = (32.0, 64.0, 128.0)
SENTINEL = -7.0


# ----------------------------------------------------------------------------- data sets
def _ints(shape, values, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), shape, generator=g)].to(BF)


def _seed(kind: str, M: int, N: int, K: int, seed: int) -> int:
    return (sum(map(ord, kind)) * 1000003 + M * 7919 + N * 104729 + K * 31 + seed * 15485863) % (
        2 ** 31 - 1)


@functools.lru_cache(maxsize=None)
def wide(M: int, N: int, K: int, seed: int = 0):
    """(x [M, K], w [N, K]) in {+-1, +-3}, independent per element."""
    s = _seed("wide", M, N, K, seed)
    return _ints((M, K), (-3.0, -1.0, 1.0, 3.0), s), _ints((N, K), (-3.0, -1.0, 1.0, 3.0), s + 1)


def matmul64(x, w):
    """x @ w.T in float64 on the CPU (exact for these integers)."""
    return x.double() @ w.double().t()


def slices64(x, w, splits: int):
    """The expectation of each split-K slab: x[:, ks] @ w[:, ks].T for the slice ks of each
    split, in slab order."""
    K = x.shape[1]
    ksl = K // splits
    assert ksl * splits == K and ksl % 8 == 0
    return [matmul64(x[:, s * ksl:(s + 1) * ksl], w[:, s * ksl:(s + 1) * ksl])
            for s in range(splits)]


def caps_hold(x, w, splits=(1,), bias=None, cap=CAP) -> bool:
    y = matmul64(x, w)
    if bias is not None:
        y = y + bias.double()
    if y.abs().max().item() > cap:
        return False
    return all(p.abs().max().item() <= SLICE_CAP for s in splits if s > 1
               for p in slices64(x, w, s))


def assert_caps(x, w, splits=(1,), bias=None, cap=CAP):
    """The narrow set's conditions, asserted on the reference before any launch."""
    y = matmul64(x, w)
    if bias is not None:
        y = y + bias.double()
    top = y.abs().max().item()
    assert top <= cap, f"|want| {top} > {cap}: not exact in bf16"
    for s in splits:
        if s > 1:
            part = max(p.abs().max().item() for p in slices64(x, w, s))
            assert part <= SLICE_CAP, f"|slice| {part} > {SLICE_CAP} at splits {s}"
    return y


@functools.lru_cache(maxsize=None)
def narrow(M: int, N: int, K: int, splits: tuple = (1,), cap: int = CAP):
    """(x, w) in {-1, +1} from the first seed whose sums meet the caps (never clamped)."""
    for seed in range(16):
        s = _seed("narrow", M, N, K, seed)
        x, w = _ints((M, K), (-1.0, 1.0), s), _ints((N, K), (-1.0, 1.0), s + 1)
        if cap is None or caps_hold(x, w, splits, cap=cap):
            return x, w
    raise AssertionError(f"no seed in 0..15 keeps narrow data within the caps at {(M, N, K)}")


def int_bias(N: int, seed: int = 0, span: int = 8):
    """Integer bias in [-span, span] as bf16."""
    g = torch.Generator().manual_seed(_seed("bias", 0, N, 0, seed))
    return torch.randint(-span, span + 1, (N,), generator=g).to(BF)


def int_residual(M: int, N: int, seed: int = 0, span: int = 40):
    g = torch.Generator().manual_seed(_seed("res", M, N, 0, seed))
    return torch.randint(-span, span + 1, (M, N), generator=g).to(BF)


def to_bf16(y64):
    """The round-to-nearest-even bf16 image of float64 integers below 2^24."""
    assert y64.abs().max().item() < 2 ** 24
    return y64.float().to(BF)


def expect_res(y64, r0):
    """The residual epilogue: bf16(r0 + bf16(y)) (the GEMM result is rounded before the add)."""
    return (r0.double() + to_bf16(y64).double()).float().to(BF)


# ----------------------------------------------------------------------------- SiLU*up
def silu_cols(K: int):
    """The gate columns: one in the first, one in a middle and one in the last K-tile."""
    return (3, (K // 128) * 64 + 5, K - 2)


def gate_value(pair: int, expert: int = 0) -> float:
    return GATES[(pair + expert) % 3]


def assert_silu_identity():
    """fp32 x / (1 + exp(-x)) == x at the gate values; so is the float64 SiLU rounded to fp32."""
    g = torch.tensor(GATES, dtype=torch.float32)
    assert torch.equal(g / (1.0 + torch.exp(-g)), g)
    g64 = g.double()
    s64 = g64 / (1.0 + torch.exp(-g64))
    assert torch.equal(s64.float(), g) and (s64 - g64).abs().max().item() < 1e-11
    assert torch.equal(torch.nn.functional.silu(g), g)


@functools.lru_cache(maxsize=None)
def silu_data(M: int, N: int, K: int, expert: int = 0, cap: int = CAP, seed: int = 0):
    """(x, w) of the exact SiLU*up witness: w is the 16-row interleaved gate/up weight [N, K]
    (N % 32 == 0): gate row j of pair p is zero but for gate_value(p) at column
    silu_cols(K)[(p // 3 + j) % 3], the up rows are dense narrow data; x is narrow with 1 in
    the gate columns. With ``cap`` the up sums stay within it."""
    assert N % 32 == 0 and K >= 64
    cols = silu_cols(K)
    for s in range(16):
        sd = _seed("silu", M, N, K, seed + 16 * expert + 1000 * s)
        x, w = _ints((M, K), (-1.0, 1.0), sd), _ints((N, K), (-1.0, 1.0), sd + 1)
        x[:, list(cols)] = 1.0
        wv = w.view(N // 32, 2, 16, K)
        wv[:, 0] = 0.0
        for p in range(N // 32):
            for j in range(16):
                wv[p, 0, j, cols[(p // 3 + j) % 3]] = gate_value(p, expert)
        if cap is None or matmul64(x, w).view(M, N // 32, 2, 16)[:, :, 1].abs().max() <= cap:
            return x, w
    raise AssertionError(f"no seed keeps the up sums within {cap} at {(M, N, K)}")


def expect_silu(y64):
    """bf16(gate * up) of y = x @ w.T over the 16-row interleaved layout, [M, N / 2]; asserts
    that every gate is one of GATES (where SiLU is the identity in fp32)."""
    M, N = y64.shape
    v = y64.view(M, N // 32, 2, 16)
    g, u = v[:, :, 0], v[:, :, 1]
    assert set(g.unique().tolist()) <= set(GATES)
    return to_bf16((g * u).reshape(M, N // 2))


# ----------------------------------------------------------------------------- grouped rows
def group_sizes(bm: int):
    """Empty groups, one row, a tile less one, a whole tile, a tile plus one, two tiles plus."""
    return [0, 1, bm - 1, bm, bm + 1, 0, 2 * bm + 5]


def offsets(sizes):
    return [0] + list(itertools.accumulate(sizes))


def expect_grouped(x, w, sizes, arow=None):
    """Rows [off[g], off[g+1]) of x (read through ``arow`` when given) meet w[g]: float64
    [rows, N]."""
    off = offsets(sizes)
    src = x if arow is None else x[arow.long()]
    return torch.cat([matmul64(src[off[g]:off[g + 1]], w[g]) for g in range(len(sizes))])


@functools.lru_cache(maxsize=None)
def grouped_data(bm: int, N: int, K: int, silu: bool):
    """(x [rows, K], w [E, N, K], sizes) with per-expert independent weights: a row that met
    another expert's weight gives another integer."""
    sizes = group_sizes(bm)
    rows, E = sum(sizes), len(sizes)
    if silu:
        ws = [silu_data(rows, N, K, expert=e, cap=None)[1] for e in range(E)]
        x = silu_data(rows, N, K, expert=0, cap=None)[0]
    else:
        x = narrow(rows, N, K, cap=None)[0]
        ws = [_ints((N, K), (-1.0, 1.0), _seed("expert", e, N, K, 0)) for e in range(E)]
    return x, torch.stack(ws), sizes


def gather_rows(rows: int, T: int, seed: int = 0):
    """A non-identity row map with repeats: int32 [rows] into T source rows."""
    g = torch.Generator().manual_seed(_seed("arow", rows, T, 0, seed))
    a = torch.randint(0, T, (rows,), generator=g, dtype=torch.int32)
    assert len(a.unique()) < rows and not torch.equal(a, torch.arange(rows, dtype=torch.int32))
    return a


# ----------------------------------------------------------------------------- comparison
def assert_exact(got, want, label=""):
    """got == want element for element; a failure reports the mismatch count, the first 16
    rows and columns, and the differences got - want (for integer data their sign and size say
    how many terms went wrong)."""
    assert got.shape == want.shape, f"{label}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    assert got.dtype == want.dtype, f"{label}: dtype {got.dtype} != {want.dtype}"
    if want.device != got.device:
        want = want.to(got.device)
    if torch.equal(got, want):
        return
    g, w = got.double().cpu(), want.double().cpu()
    bad = ~((g == w) | (g.isnan() & w.isnan()))
    idx = bad.nonzero()
    if idx.numel() == 0:
        return
    if g.dim() == 1:
        g, w, idx = g[None], w[None], torch.cat([torch.zeros_like(idx), idx], 1)
    rows, cols = idx[:, -2].unique()[:16].tolist(), idx[:, -1].unique()[:16].tolist()
    first = [(tuple(i.tolist()), g[tuple(i)].item(), w[tuple(i)].item(),
              g[tuple(i)].item() - w[tuple(i)].item()) for i in idx[:16]]
    raise AssertionError(
        f"{label}: {idx.shape[0]} of {bad.numel()} elements differ; rows {rows} cols {cols}; "
        "(index, got, want, got - want): " + "; ".join(
            f"{i} {a:g} {b:g} {d:+g}" for i, a, b, d in first))


# ----------------------------------------------------------------------------- case lists
# The tile ids the GPU module launches, as literals: tests/test_gemm_witness.py compares them
# with ops.gemm's tables, so a tile cannot be added there without a witness here.
MFMA_TILES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22,
              23, 24, 25, 26, 28, 34, 41, 45, 55, 60, 61)
GEMV_TILE_IDS = (29, 30, 31, 32, 33, 56, 57, 58, 59)
M_SIZES = (1, 300)
N_SIZES = (520, 516, 515)          # 16-B wide stores + an odd block, 8-B quads, per column
K_UNSPLIT = (64, 128, 192, 320, 384, 1216)
K_SPLIT = (512, 1536)
SPLITS = (2, 4, 8)
K_TILE55 = (128, 384, 1280)
TILE55_BIG = (300, 40968, 384)     # 2 x 161 = 322 tiles on at most 256 workgroups
REPEAT_FAMILIES = ("8p", "4w", "4wp")
STAGGERED = (60, 61)
GROUPED_K = (192, 448)
GROUPED_K_SPLIT = 384              # splits = 2 needs whole K-tiles per slice (K % 128 == 0)
GEMV_M = (1, 2, 3, 4)
GEMV_N = (40, 100)
GEMV_N_SILU = 96
GEMV_K = {t: (72, 520, 1024, 1096, 2120) for t in (29, 30, 31, 32, 33)}
GEMV_K.update({t: (64, 576, 1024, 2112, 4672) for t in (56, 57, 58, 59)})
GEMV_SPLITS = (2, 4)
GEMV_K_SPLIT = 1536
NARROW_MAX_K = 1536                # beyond it narrow sums leave the cap: fp32 / RNE images


def repeats(tile: int) -> int:
    """Launches per case: a schedule race shows as an intermittent tile."""
    return 3 if (G.TILE_TABLE[tile].family in REPEAT_FAMILIES or tile in STAGGERED) else 1


def silu_n(tile: int) -> int:
    """Weight rows of the SiLU*up cases: 544 (N % 32 == 0, two whole column tiles and a
    partial one at every width), 576 for the 256x256 8-phase tile, which takes N % 64 == 0."""
    return 576 if tile == 22 else 544


def splits_ok(tile: int) -> bool:
    return G.TILE_TABLE[tile].family != "4wp"


def groups_ok(tile: int) -> bool:
    return G.TILE_TABLE[tile].family != "4wp"


def mfma_cases(tile: int):
    """(M, N, K, splits, epi, data) of every exact case of one MFMA tile; epi "none" / "bias"
    with data "wide" is compared with the round-to-nearest-even image."""
    fam = G.TILE_TABLE[tile].family
    assert fam in ("tiles", "8p", "4w", "4wp"), f"no witness rules for family {fam}"
    ks = [(K, 1) for K in (K_TILE55 if fam == "4wp" else K_UNSPLIT)]
    if splits_ok(tile):
        ks += [(K, s) for K in K_SPLIT for s in SPLITS]
    out = []
    for (K, s), M in itertools.product(ks, M_SIZES):
        for N in N_SIZES:
            out += [(M, N, K, s, "f32", "wide"), (M, N, K, s, "none", "narrow"),
                    (M, N, K, s, "none", "wide"), (M, N, K, s, "bias", "narrow"),
                    (M, N, K, s, "bias", "wide")]
        if G.tile_ok(tile, "silu_mul"):
            out.append((M, silu_n(tile), K, s, "silu_mul", "silu"))
    return out


def gemv_cases(tile: int):
    """(M, N, K, splits, epi, data) of every exact case of one GEMV tile. At K beyond
    NARROW_MAX_K the narrow sums leave the cap, so the plain tiles run the fp32 epilogue there
    and the SiLU*up / residual epilogues are compared with their round-to-nearest-even images
    (exact for any integer sum below 2^24)."""
    assert tile in G.GEMV_TILES
    ms = (1,) if tile in G.GEMV_M1_ONLY else GEMV_M
    ks = [(K, 1) for K in GEMV_K[tile]] + [(GEMV_K_SPLIT, s) for s in GEMV_SPLITS]
    out = []
    for (K, s), M in itertools.product(ks, ms):
        if G.tile_ok(tile, "silu_mul"):
            out.append((M, GEMV_N_SILU, K, s, "silu_mul", "silu"))
        if G.tile_ok(tile, "none"):
            for N in GEMV_N:
                out.append((M, N, K, s, "f32", "wide"))
                if K <= NARROW_MAX_K:
                    out += [(M, N, K, s, "none", "narrow"), (M, N, K, s, "bias", "narrow")]
                out.append((M, N, K, s, "none", "wide"))
        if G.tile_ok(tile, "res") and s == 1:
            out += [(M, N, K, 1, "res", "narrow") for N in GEMV_N]
    return out


def case_tiles():
    """{tile id: number of exact cases} over both tables."""
    out = {t: len(mfma_cases(t)) for t in G.TILE_TABLE}
    out.update({t: len(gemv_cases(t)) for t in G.GEMV_TILES})
    return out


@functools.lru_cache(maxsize=None)
def case_data(M: int, N: int, K: int, splits: int, epi: str, data: str):
    """(x, w, bias / residual or None, want in the output dtype) of one case, caps asserted."""
    extra = None
    if data == "silu":
        cap = CAP if K <= NARROW_MAX_K else None
        x, w = silu_data(M, N, K, cap=cap)
        return x, w, None, expect_silu(matmul64(x, w))
    if data == "wide":
        x, w = wide(M, N, K)
    else:
        # the seed is chosen with room for the integer bias (8) or residual (40); beyond
        # NARROW_MAX_K ("res" alone) the result is compared with its RNE image
        x, w = narrow(M, N, K, (splits,), NARROW_CAP if K <= NARROW_MAX_K else None)
    if epi == "bias":
        extra = int_bias(N)
    if data == "narrow" and K <= NARROW_MAX_K:
        y = assert_caps(x, w, (splits,), extra, CAP)
    else:
        y = matmul64(x, w) if extra is None else matmul64(x, w) + extra.double()
    if epi == "res":
        extra = int_residual(M, N)
        want = expect_res(y, extra)
        if K <= NARROW_MAX_K:
            assert (extra.double() + y).abs().max().item() <= CAP
    elif epi == "f32":
        want = y.float()
    else:
        want = to_bf16(y)
        if data == "narrow":
            assert torch.equal(want.double(), y)         # nothing was rounded
    return x, w, extra, want


# ----------------------------------------------------------------------------- numpy model
def np_bf16(a, truncate: bool = False):
    """float -> bf16 -> float32 by bit arithmetic: round to nearest even, or truncation."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    if not truncate:
        u = u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))
    return (u & np.uint32(0xFFFF0000)).view(np.float32)


MUTATIONS = {
    1: "last K-tile of a slice dropped",
    2: "one 8-element chunk of one row in one K-tile dropped",
    3: "one 16-row block of a K-tile read from the K-tile `stages` earlier",
    4: "a K-tile counted in two slices",
    40: "a K-tile counted in no slice",
    5: "two slabs swapped",
    6: "last row of a partial row tile dropped",
    7: "last partial column quad skipped",
    8: "a 16x16 block transposed",
    9: "fp16 slab scale missing",
    90: "fp16 slab scale applied twice",
    10: "gate block paired with the neighbouring pair's up block",
    11: "row tile straddling a group end uses the previous group's weight",
    12: "gather reads x[p] instead of x[arow[p]]",
    13: "the two 8-column runs of a wide store swapped",
    14: "conversion truncates to bf16",
    15: "values rounded to bf16 before the bias add",
    16: "one k term of one row dropped",
}


def model_gemm(x, w, bm: int, bn: int, *, splits: int = 1, stages: int = 2, epi: str = "f32",
               bias=None, slab=None, sizes=None, arow=None, mut: int = 0):
    """A tiled, K-tiled, split-K GEMM in numpy with the structure of the kernels: row tiles (per
    group in grouped mode) x column tiles x K slices x 64-wide K-tiles, float64 accumulators,
    then the slab store (``slab`` 0: fp32, 1: fp16 x 1/16; returns [splits, rows, N]) or the
    epilogue (f32 / none / bias / silu_mul) into a SENTINEL-filled output. ``mut`` (a key of
    MUTATIONS) breaks one thing, in the last tile that has it."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    K = x.shape[1]
    N = w.shape[-2]
    nk = K // BK
    assert nk * BK == K and nk % splits == 0
    per = nk // splits
    src = np.arange(x.shape[0]) if arow is None else np.asarray(arow, dtype=np.int64)
    if mut == 12:
        src = np.arange(len(src)) % x.shape[0]
    rows = len(src)
    # row tiles: (global rows, weight matrix)
    tiles_m = []
    if sizes is None:
        tiles_m = [(np.arange(r, min(r + bm, rows)), w) for r in range(0, rows, bm)]
    elif mut == 11:
        grp = np.repeat(np.arange(len(sizes)), sizes)
        tiles_m = [(np.arange(r, min(r + bm, rows)), w[grp[r]]) for r in range(0, rows, bm)]
    else:
        off = offsets(sizes)
        for g in range(len(sizes)):
            tiles_m += [(np.arange(r, min(r + bm, off[g + 1])), w[g])
                        for r in range(off[g], off[g + 1], bm)]
    # K-tiles of each slice
    ranges = [list(range(s * per, (s + 1) * per)) for s in range(splits)]
    if mut == 4 and splits > 1:
        ranges[0].append(ranges[1][0])
    if mut == 40 and splits > 1:
        ranges[1] = ranges[1][1:]
    slabs = np.zeros((splits, rows, N))
    last_m = len(tiles_m) - 1
    for ti, (R, wg) in enumerate(tiles_m):
        for n0 in range(0, N, bn):
            n1 = min(n0 + bn, N)
            hit = ti == last_m and n1 == N               # the mutated tile
            for s, kts in enumerate(ranges):
                if mut == 1 and hit and s == splits - 1:
                    kts = kts[:-1]
                for t in kts:
                    xa = x[src[R], t * BK:(t + 1) * BK].copy()
                    if mut == 2 and hit and t == kts[len(kts) // 2]:
                        xa[len(R) // 2, 8:16] = 0.0
                    if mut == 16 and hit and t == kts[0]:
                        xa[0, 0] = 0.0
                    if mut == 3 and hit and t == kts[-1] and t >= stages:
                        blk = slice(0, min(16, len(R)))
                        xa[blk] = x[src[R[blk]], (t - stages) * BK:(t - stages + 1) * BK]
                    slabs[s][R[:, None], np.arange(n0, n1)[None]] += xa @ wg[n0:n1,
                                                                           t * BK:(t + 1) * BK].T
    if mut == 5 and splits > 1:
        slabs[[0, 1]] = slabs[[1, 0]]
    if slab is not None:
        if slab == 0:
            return slabs.astype(np.float32)
        scale = {9: 1.0, 90: 1.0 / 256}.get(mut, 1.0 / 16)
        return (slabs * scale).astype(np.float16)
    acc = slabs.sum(0)
    if epi == "silu_mul":
        v = acc.reshape(rows, N // 32, 2, 16)
        g, u = v[:, :, 0].astype(np.float32), v[:, :, 1].astype(np.float32).copy()
        if mut == 10:
            last = N // 32 - 1
            u[:, [last - 1, last]] = u[:, [last, last - 1]]
        with np.errstate(over="ignore"):
            val = np_bf16((g / (np.float32(1) + np.exp(-g))) * u).reshape(rows, N // 2)
        return val
    if epi == "f32":
        val = acc.astype(np.float32)
    elif epi == "bias":
        b = np.asarray(bias, dtype=np.float32)[None]
        a32 = np_bf16(acc) if mut == 15 else acc.astype(np.float32)
        val = np_bf16(a32 + b, truncate=mut == 14)
    else:
        val = np_bf16(acc, truncate=mut == 14)
    out = np.full((rows, N), SENTINEL, dtype=np.float32)
    out[:] = val
    R = tiles_m[last_m][0]
    if mut == 6:
        out[R[-1]] = SENTINEL
    if mut == 7:
        out[:, (N - 1) // 4 * 4:] = SENTINEL
    if mut == 8:
        r0, c0 = rows - 16, (N - 16) // 4 * 4
        if r0 >= 0 and c0 >= 0:                          # (a matrix under 16 rows has none)
            out[r0:r0 + 16, c0:c0 + 16] = val[r0:r0 + 16, c0:c0 + 16].T
    if mut == 13:
        c0 = (N - 32) // 32 * 32
        r = R[:16]
        out[r, c0 + 8:c0 + 16], out[r, c0 + 16:c0 + 24] = (val[r, c0 + 16:c0 + 24],
                                                           val[r, c0 + 8:c0 + 16])
    return out
