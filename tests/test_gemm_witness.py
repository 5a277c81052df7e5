"""The exact GEMM witnesses on the CPU (tests/gemm_witness.py): the builders meet their caps
at every shape the GPU module launches, the expectations equal ops.reference on the same
integers, the case lists cover ops.gemm's tile tables, and every mutation of the numpy model
of a tiled split-K GEMM fails at least one witness. MOTIVE records which of those mutations
the tolerance check of the random-data tests lets through."""
import numpy as np
import pytest
import torch

import gemm_witness as W
from distributed_llm_inferencing_amd.ops import gemm as G
from distributed_llm_inferencing_amd.ops import reference as R

BF = torch.bfloat16


def test_case_lists_cover_the_tile_tables():
    assert sorted(W.MFMA_TILES) == sorted(G.TILE_TABLE)
    assert sorted(W.GEMV_TILE_IDS) == sorted(G.GEMV_TILES)
    counts = W.case_tiles()
    assert set(counts) == set(G.TILE_TABLE) | set(G.GEMV_TILES)
    assert all(n > 0 for n in counts.values()), counts
    # every epilogue a tile has is among its exact cases
    for t in G.TILE_TABLE:
        epis = {c[4] for c in W.mfma_cases(t)}
        assert {"f32", "none", "bias"} <= epis and ("silu_mul" in epis) == G.tile_ok(t, "silu_mul")
    for t in G.GEMV_TILES:
        epis = {c[4] for c in W.gemv_cases(t)}
        for e in ("none", "silu_mul", "res"):
            assert (e in epis) == G.tile_ok(t, e), (t, e)


def test_builders_meet_their_caps_at_every_gpu_shape():
    """case_data asserts the caps itself; here every distinct case of every tile is built."""
    cases = set()
    for t in G.TILE_TABLE:
        cases.update(W.mfma_cases(t))
    for t in G.GEMV_TILES:
        cases.update(W.gemv_cases(t))
    seen = set()
    for c in sorted(cases):
        x, w, extra, want = W.case_data(*c)
        M, N, K, splits, epi, data = c
        vals = {"wide": {-3.0, -1.0, 1.0, 3.0}, "narrow": {-1.0, 1.0}}.get(data)
        if vals and (id(x), id(w)) not in seen:
            seen.add((id(x), id(w)))
            assert set(x.float().unique().tolist()) <= vals
            assert set(w.float().unique().tolist()) <= vals
        assert want.shape == (M, N // 2 if epi == "silu_mul" else N)
        assert want.dtype == (torch.float32 if epi == "f32" else BF)
    # the slab and add-only cases of the GPU module
    slabs = [(m, n, k, s) for m in W.M_SIZES for n in (520, 515) for k in W.K_SPLIT
             for s in W.SPLITS]
    slabs += [(m, n, W.GEMV_K_SPLIT, s) for m in W.GEMV_M for n in W.GEMV_N for s in W.GEMV_SPLITS]
    for M, N, K, s in slabs:
        x, w = W.narrow(M, N, K, (s,), W.NARROW_CAP)
        W.assert_caps(x, w, (s,), cap=W.NARROW_CAP)
        assert max(p.abs().max().item() for p in W.slices64(*W.wide(M, N, K), s)) <= W.SLICE_CAP
    # the grouped cases: every tile height, plain sums within the cap
    for bm in sorted({t.bm for t in G.TILE_TABLE.values()}):
        for K in W.GROUPED_K + (W.GROUPED_K_SPLIT,):
            x, w, sizes = W.grouped_data(bm, 544, K, False)
            assert x.shape[0] == sum(sizes) == 5 * bm + 6
            assert W.expect_grouped(x, w, sizes).abs().max().item() <= W.CAP


def test_expectations_equal_the_reference_ops():
    W.assert_silu_identity()
    x, w = W.wide(300, 515, 384)
    y = W.matmul64(x, w)
    assert torch.equal(y, R.linear(x, w, out_dtype=torch.float64))
    assert torch.equal(sum(W.slices64(x, w, 2)), y)
    b = W.int_bias(515)
    assert torch.equal(W.to_bf16(y + b.double()), R.linear(x, w, b))
    xs, ws = W.silu_data(300, 544, 384)
    ys = W.matmul64(xs, ws)
    assert torch.equal(W.expect_silu(ys), R.silu_mul(ys.float()).to(BF))
    assert torch.equal(W.expect_silu(ys).double(), R.silu_mul(ys))      # float64 SiLU, rounded
    # neighbouring gate blocks differ, and the gate columns span the K range
    g = ys.view(300, 17, 2, 16)[0, :, 0, 0]
    assert all(g[p] != g[p + 1] for p in range(16))
    assert W.silu_cols(384)[0] < 64 <= W.silu_cols(384)[1] < 320 <= W.silu_cols(384)[2]
    xg, wg, sizes = W.grouped_data(64, 544, 192, False)
    yg = W.expect_grouped(xg, wg, sizes)
    off = W.offsets(sizes)
    for e in range(len(sizes)):
        assert torch.equal(yg[off[e]:off[e + 1]],
                           R.linear(xg[off[e]:off[e + 1]], wg[e], out_dtype=torch.float64))


# ------------------------------------------------------------------ mutations of the model
def _f(t):
    return t.float().numpy()


def _witnesses():
    """[(label, run(mut) -> (got, want))]: the model under a 64x64 tile at shapes of the GPU
    module, against the expectations the GPU module uses."""
    out = []

    def add(label, case, bm=64, bn=64, slab=None, stages=2):
        M, N, K, splits, epi, data = case

        def run(mut):
            x, w, extra, want = W.case_data(*case)
            if slab is not None:
                got = W.model_gemm(_f(x), _f(w), bm, bn, splits=splits, stages=stages, slab=slab,
                                   mut=mut)
                parts = torch.stack(W.slices64(x, w, splits))
                want = parts.float() if slab == 0 else (parts / 16).to(torch.float16)
                return torch.from_numpy(got), want
            got = W.model_gemm(_f(x), _f(w), bm, bn, splits=splits, stages=stages, epi=epi,
                               bias=None if extra is None else _f(extra), mut=mut)
            return torch.from_numpy(got), want.float()
        out.append((label, run))

    add("f32 wide", (300, 515, 384, 1, "f32", "wide"))
    add("none narrow", (300, 520, 320, 1, "none", "narrow"), stages=3)
    add("none wide (RNE)", (300, 516, 1216, 1, "none", "wide"))
    add("bias narrow", (300, 520, 192, 1, "bias", "narrow"))
    # (K even: a sum of wide products is even, so it is exact in bf16 below 512 and only an
    # odd bias makes ties below that; rounding before the add shows from |sum| >= 512)
    add("bias wide (RNE)", (300, 520, 1216, 1, "bias", "wide"))
    add("silu", (300, 544, 384, 1, "silu_mul", "silu"))
    add("split f32", (300, 515, 512, 2, "f32", "wide"))
    add("slab fp32", (300, 515, 512, 4, "f32", "wide"), slab=0)
    add("slab fp16", (300, 520, 1536, 8, "none", "narrow"), slab=1)

    def grouped(silu, gather):
        def run(mut):
            x, w, sizes = W.grouped_data(64, 544, 192, silu)
            arow = None
            if gather:
                arow = W.gather_rows(sum(sizes), 150)
                x = x[:150]
            y = W.expect_grouped(x, w, sizes, arow)
            want = W.expect_silu(y) if silu else W.to_bf16(y)
            got = W.model_gemm(_f(x), _f(w), 64, 64, epi="silu_mul" if silu else "none",
                               sizes=sizes, arow=None if arow is None else arow.numpy(), mut=mut)
            return torch.from_numpy(got), want.float()
        return run
    out.append(("grouped none", grouped(False, False)))
    out.append(("grouped silu gather", grouped(True, True)))
    return out


def _fails(run, mut):
    got, want = run(mut)
    try:
        W.assert_exact(got, want, "model")
    except AssertionError:
        return True
    return False


def test_model_passes_every_witness_unmutated():
    for label, run in _witnesses():
        got, want = run(0)
        W.assert_exact(got, want, label)


@pytest.mark.parametrize("mut", sorted(W.MUTATIONS))
def test_every_mutation_fails_a_witness(mut):
    caught = [label for label, run in _witnesses() if _fails(run, mut)]
    assert caught, f"mutation {mut} ({W.MUTATIONS[mut]}) passes every witness"


def test_assert_exact_reports_rows_columns_and_differences():
    want = torch.zeros(4, 8)
    got = want.clone()
    got[2, 5] = -3.0
    with pytest.raises(AssertionError, match=r"1 of 32 .*rows \[2\] cols \[5\].*-3 0 -3"):
        W.assert_exact(got, want, "probe")


# ------------------------------------------------------------------ the motive table
def _close(a, b, rtol=1e-2, atol=1e-2):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.abs(a - b).max() <= atol + rtol * np.abs(b).max())


def _present_check_passes(mut: int) -> bool:
    """Whether the mutated model passes close(rtol=1e-2, atol=1e-2) against the fp32 reference
    on x ~ N(0, 1), w ~ 0.05 N(0, 1) (bf16) at K = 4096, under the epilogue the mutation
    lives in; slabs are checked as the present tests check them, through their sum."""
    g = torch.Generator().manual_seed(4096 + mut)
    M, N, K, bm, bn = 300, 544, 4096, 256, 256
    sizes = arow = None
    epi, splits, slab = "none", 1, None
    if mut in (4, 40, 5):
        splits = 2
    if mut in (9, 90, 5):
        splits, slab = 2, (1 if mut != 5 else 0)
    if mut == 10:
        epi = "silu_mul"
    if mut == 15:
        epi = "bias"
    x = torch.randn(M, K, generator=g).to(BF)
    w = (0.05 * torch.randn(N, K, generator=g)).to(BF)
    bias = torch.randn(N, generator=g).to(BF)
    if mut in (11, 12):
        sizes = [0, 37, 170, 93]
        w = (0.05 * torch.randn(len(sizes), N, K, generator=g)).to(BF)
        if mut == 12:
            arow = W.gather_rows(M, 150).numpy()
    src = x if arow is None else x[torch.from_numpy(arow).long()]
    if sizes is None:
        ref = R.linear(src, w, out_dtype=torch.float32)
    else:
        off = W.offsets(sizes)
        ref = torch.cat([R.linear(src[off[e]:off[e + 1]], w[e], out_dtype=torch.float32)
                         for e in range(len(sizes))])
    if epi == "bias":
        ref = ref + bias.float()
    if epi == "silu_mul":
        ref = R.silu_mul(ref.to(BF)).float()
    got = W.model_gemm(_f(x), _f(w), bm, bn, splits=splits, stages=2, epi=epi, bias=_f(bias),
                       slab=slab, sizes=sizes, arow=arow, mut=mut)
    if slab is not None:
        got = got.astype(np.float64).sum(0) * (16.0 if slab == 1 else 1.0)
    return _close(got, ref.numpy())


# mutation -> passes the present tolerance check (True: the random-data tests cannot see it)
MOTIVE = {1: False, 2: False, 3: False, 4: False, 40: False, 5: True, 6: False, 7: False,
          8: False, 9: False, 90: False, 10: False, 11: False, 12: False, 13: False, 14: True,
          15: True, 16: True}


def test_motive_table():
    measured = {m: _present_check_passes(m) for m in sorted(W.MUTATIONS)}
    print("motive table:", measured)
    assert _present_check_passes(0)
    assert measured == MOTIVE
