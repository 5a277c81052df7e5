"""The staggered two-group tiles (60 = tile 23's 128x192, 61 = tile 17's 128x256: waves 4-7
one segment behind waves 0-3, gemm_tiles.hip STAG) against their lockstep twins, bit for bit,
and the 16-B epilogue stores of the 2-byte outputs (gemm_common.h widen_pair) against the
8-B stores of the same build.

Where a case cannot run as first written the nearest runnable one is used:
* the SiLU*up epilogue needs N % 32 == 0 (whole gate/up pairs; dli_gemm refuses other N), so
  its N is rounded up to a multiple of 32, and tile 60 (48-column waves) has no SiLU pairing;
* the SiLU*up epilogue keeps its 8-B stores (pairing two gate/up results into one 16-B store
  measured slower on the gate/up GEMM, profiles/r7/README.md), and its output, N / 2 = a
  multiple of 16 columns, would be wide at every N: the test pins that the output depends on
  neither the row stride nor N;
* the fused add+RMSNorm reduce needs N % 8 == 0, so at the narrow width the fp16 slab image
  itself is compared (and at both widths with fp16(fp32 partial / 16), the fp32 partials
  being written by 16-B fp32 stores that no change here touches).
"""
import itertools

import pytest
import torch

from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.ops import gemm as G
from distributed_llm_inferencing_amd.ops import reference as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TWIN = {60: 23, 61: 17}


def rnd(*shape, dev, scale=1.0, dtype=BF):
    return (torch.randn(*shape, device=dev) * scale).to(dtype)


def close(a, b, rtol, atol):
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    tol = atol + rtol * b.abs().max().item()
    assert err <= tol, f"max err {err} > tol {tol}"


def test_new_tiles_registered():
    for t, twin in TWIN.items():
        assert G.TILES[t] == G.TILES[twin] and G.TILE_WAVES[t] == G.TILE_WAVES[twin]
        assert t in G.SLAB16_TILES and t in G.GATHER_TILES
        assert any(p.tile == t for p in G.candidate_plans(512, 4096, 4096, "splitk"))


@pytest.mark.parametrize("tile", sorted(TWIN))
@pytest.mark.parametrize("M", [100, 128, 300])
def test_twin_equality(gpu, tile, M):
    """1-7 K-steps (the ring's prologue and tail), partial row / column tiles, every epilogue:
    the same bits as the lockstep twin, and the fp32 reference within 1e-2 for the plain and
    fp32 outputs."""
    torch.manual_seed(70 + tile)
    bn = G.TILES[tile][1]
    for K in (64, 128, 192, 256, 320, 448):
        x = rnd(M, K, dev=gpu)
        for N in (bn, 200, 3 * bn + 8):
            Nw = -(-N // 32) * 32
            w = rnd(Nw, K, dev=gpu, scale=0.05)
            bias = rnd(Nw, dev=gpu)
            ref = R.linear(x, w[:N], out_dtype=torch.float32)
            for epi in ("none", "f32", "silu_mul", "bias_gelu"):
                if not G.tile_ok(tile, epi):
                    continue
                n = Nw if epi == "silu_mul" else N
                b = bias[:n] if epi == "bias_gelu" else None
                out = ops._gemm_native(x, w[:n], epi, bias=b, plan=G.GemmPlan("dli", tile, 1))
                twin = ops._gemm_native(x, w[:n], epi, bias=b,
                                        plan=G.GemmPlan("dli", TWIN[tile], 1))
                assert torch.equal(out, twin), (tile, M, N, K, epi)
                if epi in ("none", "f32"):
                    close(out, ref, rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize("tile", sorted(TWIN))
@pytest.mark.parametrize("splits", [2, 4])
def test_split_k_equals_twin(gpu, tile, splits):
    """K = 512 in 2 / 4 slices: fp16 slabs into the fused add+RMSNorm reduce, and fp32 slabs +
    splitk_reduce_kernel through the plain epilogue."""
    torch.manual_seed(80 + tile)
    M, N, K = 300, 3 * G.TILES[tile][1] + 8, 512
    x, w = rnd(M, K, dev=gpu), rnd(N, K, dev=gpu, scale=0.05)
    r0, nw = rnd(M, N, dev=gpu), (1.0 + 0.1 * rnd(N, dev=gpu)).to(BF)
    outs = {}
    for t in (tile, TWIN[tile]):
        p = G.GemmPlan("dli", t, splits)
        r = r0.clone()
        o = ops.linear_add_rmsnorm(x, w, r, nw, 1e-5, plan=p)
        outs[t] = (o, r, ops._gemm_native(x, w, "none", plan=p))
    for a, b in zip(outs[tile], outs[TWIN[tile]]):
        assert torch.equal(a, b)
    close(outs[tile][2], R.linear(x, w, out_dtype=torch.float32), rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize("tile", sorted(TWIN))
def test_grouped_equals_twin(gpu, tile):
    """Grouped (MoE) mode with an empty group and a partial last tile, plain and SiLU*up,
    unsplit and split; the SiLU*up GEMM that reads its rows through a permutation."""
    torch.manual_seed(90 + tile)
    sizes = [37, 0, 170, 5]
    E, N, K = len(sizes), 512, 448
    rows = sum(sizes)
    x = rnd(rows, K, dev=gpu)
    w = rnd(E, N, K, dev=gpu, scale=0.05)
    off = torch.tensor([0] + list(itertools.accumulate(sizes)), dtype=torch.int32, device=gpu)
    for epi in ("none", "silu_mul"):
        if not G.tile_ok(tile, epi):
            continue
        for splits in (1, 7):
            out, twin = (ops._gemm_native(x, w, epi, plan=G.GemmPlan("dli", t, splits), groups=E,
                                          group_off=off, rows_per_group=rows)
                         for t in (tile, TWIN[tile]))
            assert torch.equal(out, twin), (tile, epi, splits)
    if not G.tile_ok(tile, "silu_mul"):
        return
    T = 150
    xs = rnd(T, K, dev=gpu)
    src = torch.randint(0, T, (rows,), dtype=torch.int32, device=gpu)
    got = []
    for t in (tile, TWIN[tile]):
        out = torch.full((rows, N // 2), float("nan"), dtype=BF, device=gpu)
        ops._native_call("dli_gemm_grouped_gather", ops._p(xs), xs.stride(0), ops._p(w),
                         w.stride(-2), ops._p(out), out.stride(0), rows, N, K, t, ops._p(src),
                         ops._p(off), E, ops._st())
        got.append(out)
    assert torch.equal(got[0], got[1])
    ref = ops._gemm_native(xs[src.long()].contiguous(), w, "silu_mul",
                           plan=G.GemmPlan("dli", TWIN[tile], 1), groups=E, group_off=off,
                           rows_per_group=rows)
    assert torch.equal(got[0], ref)


@pytest.mark.parametrize("tile", sorted(TWIN))
@pytest.mark.parametrize("splits", [1, 7])
def test_race_screen(gpu, tile, splits):
    """A new barrier structure: one unsplit and one split launch (K = 448: 7 K-steps, or 7
    one-step slices) repeated 20 times in-process must give the same bits every time."""
    torch.manual_seed(100 + tile)
    M, N, K = 300, 3 * G.TILES[tile][1] + 8, 448
    x, w = rnd(M, K, dev=gpu), rnd(N, K, dev=gpu, scale=0.05)
    p = G.GemmPlan("dli", tile, splits)
    first = ops._gemm_native(x, w, "none", plan=p).clone()
    for _ in range(19):
        assert torch.equal(ops._gemm_native(x, w, "none", plan=p), first)


WIDE_TILES = [17, 23, 22, 26, 28, 60, 61]


@pytest.mark.parametrize("tile", WIDE_TILES)
def test_wide_store_plain(gpu, tile):
    """N = 208 (16-B stores) against N = 204 (N % 8 = 4: the 8-B stores) of the same weight:
    the common columns carry the same bits."""
    torch.manual_seed(110)
    M, K = 300, 256
    x, w = rnd(M, K, dev=gpu), rnd(208, K, dev=gpu, scale=0.05)
    p = G.GemmPlan("dli", tile, 1)
    wide = ops._gemm_native(x, w, "none", plan=p)
    narrow = ops._gemm_native(x, w[:204], "none", plan=p)
    assert torch.equal(wide[:, :204], narrow)
    close(wide, R.linear(x, w, out_dtype=torch.float32), rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize("tile", [t for t in WIDE_TILES if G.tile_ok(t, "silu_mul")])
def test_wide_store_silu(gpu, tile):
    """SiLU*up output 224 columns wide (N = 448: the 256x256 8-phase tile takes N % 64 == 0
    only) against the same GEMM written into a view with a 228-column row stride (no 16-B
    row alignment) and against N = 384 (whole gate/up pairs) of the same weight."""
    torch.manual_seed(111)
    M, K = 300, 256
    x, w = rnd(M, K, dev=gpu), rnd(448, K, dev=gpu, scale=0.05)
    p = G.GemmPlan("dli", tile, 1)
    wide = ops._gemm_native(x, w, "silu_mul", plan=p)
    buf = torch.zeros(M, 228, dtype=BF, device=gpu)
    narrow = ops._gemm_native(x, w, "silu_mul", out=buf[:, :224], plan=p)
    assert torch.equal(wide, narrow)
    assert not buf[:, 224:].any()
    less = ops._gemm_native(x, w[:384], "silu_mul", plan=p)
    assert torch.equal(wide[:, :192], less)
    close(wide, R.silu_mul(R.linear(x, w).float().to(BF)), rtol=2e-2, atol=2e-2)


def _slab_image(x, w, p):
    """(fp16 slab image the slab16 epilogue stores, fp16(fp32 partial / 16) of the same plan)."""
    M, N = x.shape[0], w.shape[0]
    ws = G.workspace(x.device, p.splits * M * N * 4)
    assert ops._slab_gemm(x, w, p, ws) == 1
    img = ws[:p.splits * M * N * 2].view(torch.float16).clone()
    ops._gemm_native(x, w, "none", plan=p)            # leaves its fp32 partials in ws
    part = ws[:p.splits * M * N * 4].view(torch.float32).clone()
    return img, (part * 0.0625).to(torch.float16)


@pytest.mark.parametrize("tile", WIDE_TILES + [5])
@pytest.mark.parametrize("splits", [2, 4])
def test_wide_store_slab16(gpu, tile, splits):
    """fp16 slabs through linear_add_rmsnorm at N = 512 (16-B stores): the forced tile against
    tile 5 under the same split count (same slab order, same sums), bit for bit; and the slab
    image at N = 512 and at N = 508 (8-B stores) against fp16(fp32 partial / 16)."""
    torch.manual_seed(112)
    M, K = 300, 512
    x, w = rnd(M, K, dev=gpu), rnd(512, K, dev=gpu, scale=0.05)
    r0, nw = rnd(M, 512, dev=gpu), (1.0 + 0.1 * rnd(512, dev=gpu)).to(BF)
    outs = []
    for t in (tile, 5):
        r = r0.clone()
        outs.append((ops.linear_add_rmsnorm(x, w, r, nw, 1e-5, plan=G.GemmPlan("dli", t, splits)),
                     r))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for n in (512, 508):
        img, want = _slab_image(x, w[:n], G.GemmPlan("dli", tile, splits))
        assert torch.equal(img.view(torch.int16), want.view(torch.int16)), n
