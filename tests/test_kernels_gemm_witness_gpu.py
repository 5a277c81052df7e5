"""Every bf16 GEMM tile, GEMV tile and grouped form against the exact integer witnesses of
tests/gemm_witness.py: small integers in bf16, so the fp32 accumulators hold the exact sum
whatever the MFMA order, split count or slab format, and every comparison is equality with a
float64 matmul computed on the CPU. A failure names the tile, shape, split count and epilogue,
the rows and columns that differ and by how many products.

Every launch goes through ops._gemm_native, ops._slab_gemm, ops.linear_add_rmsnorm (without a
norm weight) and ops.linear_residual under a forced plan; the grouped gather form, which
ops.moe_mlp reaches through ops._launch_gemm, is launched through it here too.

Where a case cannot run as the kernels stand the nearest runnable one is used:
* the 256x256 8-phase tile takes SiLU*up at N % 64 == 0 only: its SiLU cases use N = 576;
* split-K needs whole K-tiles per slice, so the grouped splits = 2 cases run at K = 384 beside
  the unsplit K = 192 and 448;
* the RMSNorm prologue and bias + GELU are not exactly predictable and keep their tolerance
  tests; the FP8 streams have witnesses of their own.

(The file name sorts this module among the kernel tests on purpose, as
test_kernels_attention_witness_gpu.py explains.)"""
import pytest
import torch

import gemm_witness as W
from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.ops import gemm as G

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
_UP = {}


def up(t, gpu):
    """The device copy of a cached CPU tensor (one upload per tensor)."""
    if t is None:
        return None
    hit = _UP.get(id(t))
    if hit is None or hit[0] is not t:
        hit = _UP[id(t)] = (t, t.to(gpu))
    return hit[1]


class Failures:
    """Collects every failing case of a test, so that one run shows the pattern."""

    def __init__(self):
        self.msgs = []

    def check(self, got, want, label):
        try:
            W.assert_exact(got, want, label)
        except AssertionError as e:
            self.msgs.append(str(e))

    def done(self):
        assert not self.msgs, f"{len(self.msgs)} cases fail:\n" + "\n".join(self.msgs[:24])


def launch(gpu, tile, case, out=None):
    """(result, expectation) of one case of W.mfma_cases / W.gemv_cases on the device."""
    M, N, K, splits, epi, data = case
    x, w, extra, want = (up(t, gpu) for t in W.case_data(*case))
    p = G.GemmPlan("dli", tile, splits)
    if epi == "res":
        r = extra.clone()
        ops.linear_residual(x, w, r, plan=p)
        return r, want
    return ops._gemm_native(x, w, epi, bias=extra, out=out, plan=p), want


@pytest.mark.parametrize("tile", W.MFMA_TILES)
def test_mfma_tile(gpu, tile):
    """Item 1 and 2: every epilogue at M = 1 / 300 x N = 520 / 516 / 515 (544 / 576 for
    SiLU*up) x 1-19 K-tiles unsplit and split-K 2 / 4 / 8 at K = 512 / 1536; tile 55 unsplit
    at even K-tile counts only (other calls are refused on the host)."""
    f = Failures()
    for case in W.mfma_cases(tile):
        for rep in range(W.repeats(tile)):
            got, want = launch(gpu, tile, case)
            f.check(got, want, f"tile {tile} {case} run {rep}")
    if not W.splits_ok(tile):
        x, w, _, _ = (up(t, gpu) for t in W.case_data(300, 520, 512, 1, "f32", "wide"))
        with pytest.raises(RuntimeError):
            ops._gemm_native(x, w, "f32", plan=G.GemmPlan("dli", tile, 2))
        x, w, _, _ = (up(t, gpu) for t in W.case_data(300, 520, 192, 1, "f32", "wide"))
        with pytest.raises(RuntimeError):
            ops._gemm_native(x, w, "f32", plan=G.GemmPlan("dli", tile, 1))
    f.done()


@pytest.mark.parametrize("tile", W.MFMA_TILES)
def test_mfma_tile_writes_only_its_view(gpu, tile):
    """One case per epilogue into a column view of a wider sentinel-filled buffer at a 16-B
    aligned offset (ldc != N, the vector stores kept): exact inside, untouched outside."""
    f = Failures()
    K = 384
    for epi, data, N in (("f32", "wide", 520), ("none", "narrow", 520), ("bias", "wide", 520),
                         ("silu_mul", "silu", W.silu_n(tile))):
        if not G.tile_ok(tile, epi):
            continue
        case = (300, N, K, 1, epi, data)
        n_out = N // 2 if epi == "silu_mul" else N
        big = torch.full((300, n_out + 16), W.SENTINEL, device=gpu,
                         dtype=torch.float32 if epi == "f32" else BF)
        _, want = launch(gpu, tile, case, out=big[:, 8:8 + n_out])
        full = torch.full_like(big, W.SENTINEL)
        full[:, 8:8 + n_out] = want
        f.check(big, full, f"tile {tile} {case} in a view at column 8")
        # the same case with x and w read as 16-B aligned column views of wider buffers
        # (lda, ldw != K) whose other columns hold 5: a row stride taken for K reads them
        x, w, extra, _ = (up(t, gpu) for t in W.case_data(*case))
        xb = torch.full((300, K + 24), 5.0, dtype=BF, device=gpu)
        wb = torch.full((N, K + 16), 5.0, dtype=BF, device=gpu)
        xb[:, 16:16 + K], wb[:, 8:8 + K] = x, w
        got = ops._gemm_native(xb[:, 16:16 + K], wb[:, 8:8 + K], epi, bias=extra,
                               plan=G.GemmPlan("dli", tile, 1))
        f.check(got, want, f"tile {tile} {case} from strided x and w")
    f.done()


def test_persistent_tile_walks_two_tiles(gpu):
    """Tile 55 with more tiles (2 x 161) than workgroups: a workgroup walks two tiles and
    stages the next tile's first K-tiles inside the current one."""
    M, N, K = W.TILE55_BIG
    f = Failures()
    for case in ((M, N, K, 1, "f32", "wide"), (M, N, K, 1, "none", "narrow")):
        for rep in range(W.repeats(55)):
            got, want = launch(gpu, 55, case)
            f.check(got, want, f"tile 55 {case} run {rep}")
    f.done()


def _check_slabs(f, gpu, tile, splits, M, N, K, fmt_want):
    """ops._slab_gemm into the caller's buffer, every slab against its own slice's expectation
    (fp32 slabs as they are, fp16 slabs as image x 16 at the same element index), narrow and
    wide data; then, where N % 8 == 0, the fused add-only consumer on the narrow data:
    residual == bf16(r0 + bf16(y))."""
    p = G.GemmPlan("dli", tile, splits)
    sets = [("narrow", W.narrow(M, N, K, (splits,), W.NARROW_CAP)), ("wide", W.wide(M, N, K))]
    for name, (x, w) in sets:
        if name == "narrow":
            W.assert_caps(x, w, (splits,))
        parts = torch.stack(W.slices64(x, w, splits)).float()
        assert parts.abs().max().item() <= W.SLICE_CAP             # exact in fp16 after 1/16
        ws = torch.full((splits * M * N * 4,), 0xFF, dtype=torch.uint8, device=gpu)
        for rep in range(W.repeats(tile) if tile in G.TILE_TABLE else 1):
            fmt = ops._slab_gemm(up(x, gpu), up(w, gpu), p, ws)
            assert fmt == fmt_want
            if fmt == 1:
                img = ws.view(torch.float16)[:splits * M * N].float() * 16.0
            else:
                img = ws.view(torch.float32)
            f.check(img.view(splits, M, N), parts,
                    f"tile {tile} slabs (format {fmt}) {name} {(M, N, K)} splits {splits} "
                    f"run {rep}")
    if N % 8 == 0:
        x, w = sets[0][1]
        r0 = W.int_residual(M, N)
        r = up(r0, gpu).clone()
        assert ops.linear_add_rmsnorm(up(x, gpu), up(w, gpu), r, None, 0.0, plan=p) is None
        f.check(r, W.expect_res(W.matmul64(x, w), r0),
                f"tile {tile} add-only consumer {(M, N, K)} splits {splits}")


@pytest.mark.parametrize("s16", [True, False], ids=["slab16", "slab32"])
@pytest.mark.parametrize("tile", [t for t in W.MFMA_TILES if W.splits_ok(t)])
def test_slabs_slice_by_slice(gpu, monkeypatch, tile, s16):
    """Item 3: split-K 2 / 4 / 8 at K = 512 / 1536, each slab against its own slice (the sum
    would hide a K-tile credited to the wrong slab), with the fp16 slab format on and off."""
    monkeypatch.setattr(G, "SLAB16", s16)
    f = Failures()
    fmt_want = 1 if (s16 and tile in G.SLAB16_TILES) else 0
    for K in W.K_SPLIT:
        for splits in W.SPLITS:
            for M in W.M_SIZES:
                for N in (520, 515):
                    _check_slabs(f, gpu, tile, splits, M, N, K, fmt_want)
    f.done()


@pytest.mark.parametrize("tile", [t for t in W.GEMV_TILE_IDS if G.tile_ok(t, "none")])
def test_gemv_slabs_slice_by_slice(gpu, tile):
    """The same for the weight-streaming tiles (fp32 slabs): split-K 2 / 4 at K = 1536."""
    f = Failures()
    for splits in W.GEMV_SPLITS:
        for M in ((1,) if tile in G.GEMV_M1_ONLY else W.GEMV_M):
            for N in W.GEMV_N:
                _check_slabs(f, gpu, tile, splits, M, N, W.GEMV_K_SPLIT, 0)
    f.done()


@pytest.mark.parametrize("tile", W.GEMV_TILE_IDS)
def test_gemv_tile(gpu, tile):
    """Item 4: the weight-streaming tiles at M = 1..4, partial row blocks, K around the
    512-element lane step and the tile's steps per iteration, split-K 2 / 4, and the
    residual epilogue through ops.linear_residual."""
    f = Failures()
    for case in W.gemv_cases(tile):
        got, want = launch(gpu, tile, case)
        f.check(got, want, f"gemv tile {tile} {case}")
    f.done()


def _grouped_launches(gpu, tile, epi, K, splits):
    """[(label, result, expectation)] of one grouped configuration: the dense grid, the tile
    list form and, for unsplit SiLU*up, the gather form of both."""
    bm = G.TILES[tile][0]
    N = W.silu_n(tile)
    silu = epi == "silu_mul"
    x, w, sizes = W.grouped_data(bm, N, K, silu)
    rows, E = sum(sizes), len(sizes)
    y = W.expect_grouped(x, w, sizes)
    if not silu:
        assert y.abs().max().item() <= W.CAP
    want = W.expect_silu(y) if silu else W.to_bf16(y)
    off = torch.tensor(W.offsets(sizes), dtype=torch.int32, device=gpu)
    p = G.GemmPlan("dli", tile, splits)
    xd, wd = up(x, gpu), up(w, gpu)
    what = f"tile {tile} grouped {epi} K {K} splits {splits}"
    out = [(what + " dense", ops._gemm_native(xd, wd, epi, plan=p, groups=E, group_off=off,
                                              rows_per_group=rows), want)]
    tl = G.host_tile_list(sizes, bm, gpu) if tile in G.LIST_TILES else None
    if tl is not None:
        out.append((what + " list", ops._gemm_native(xd, wd, epi, plan=p, groups=E, group_off=off,
                                                     rows_per_group=rows, tile_list=tl), want))
    if silu and splits == 1 and tile in G.GATHER_TILES:
        T = 150
        arow = W.gather_rows(rows, T)
        xs = xd[:T].contiguous()
        gwant = W.expect_silu(W.expect_grouped(x[:T], w, sizes, arow))
        for name, lst in (("gather", None), ("gather list", tl)):
            if name == "gather list" and tl is None:
                continue
            got = torch.full((rows, N // 2), float("nan"), dtype=BF, device=gpu)
            ops._launch_gemm("gemm", xs, wd, p, G.EPI[epi], got, got.stride(0), rows, N, K,
                             group_off=off, groups=E, tile_list=lst, arow=arow.to(gpu))
            out.append((f"{what} {name}", got, gwant))
    return out


@pytest.mark.parametrize("tile", [t for t in W.MFMA_TILES if W.groups_ok(t)])
def test_grouped_tile(gpu, tile):
    """Item 5: per-expert weights with independent signs over groups of 0, 1, bm - 1, bm,
    bm + 1, 0 and 2 bm + 5 rows: dense grid, tile list and gather forms, plain and SiLU*up."""
    f = Failures()
    for epi in ("none", "silu_mul"):
        if not G.tile_ok(tile, epi):
            continue
        for K, splits in [(k, 1) for k in W.GROUPED_K] + [(W.GROUPED_K_SPLIT, 2)]:
            for rep in range(W.repeats(tile)):
                for label, got, want in _grouped_launches(gpu, tile, epi, K, splits):
                    f.check(got, want, f"{label} run {rep}")
    f.done()
