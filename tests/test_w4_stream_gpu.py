"""The W4 MFMA weight stream (``dli_gemm_w4_stream``, tiles 74 / 75) at 4 < M <= 64 against
``x.double() @ w.dequantize(torch.float64).T``: an exact integer witness, every epilogue and the
slab forms, no dequantise pass under a stream plan, and an engine with stream plans pinned."""
import pytest
import torch

from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.models.weights import quantize_params, random_init, \
    stage_param_shapes
from distributed_llm_inferencing_amd.ops import gemm as G
from distributed_llm_inferencing_amd.ops import reference as R
from test_w4_weights_gpu import BF, CFG, IDS, _run, close, plan, rnd, w4_weight

pytestmark = pytest.mark.gpu
TILES = sorted(G.W4_STREAM_TILES)


@pytest.fixture
def bf16_calls(monkeypatch):
    """The calls of ``ops.W4Weight.bf16`` (the dequantise pass) during the test."""
    calls = []
    real = ops.W4Weight.bf16
    monkeypatch.setattr(ops.W4Weight, "bf16", lambda self: (calls.append(1), real(self))[1])
    return calls


_witness = {}


def witness(M, K, N=80):
    """tests/test_w4_weights_gpu.py::test_exact_witness's operands: integers everywhere and
    scales in {1/2, 1, 2}. (W4Weight on the CPU, x, the fp64 product), checked to be fp32."""
    if (M, K) not in _witness:
        n, k, grp = torch.arange(N)[:, None], torch.arange(K)[None, :], torch.arange(K // 128)
        q = ((k + 3 * (k // 8) + 5 * n) % 16).to(torch.uint8)
        z = ((5 * n + 3 * grp) % 16).to(torch.uint8)
        s = torch.exp2(((n + grp) % 3 - 1).float()).to(torch.float16)
        w = ops.W4Weight(*R.pack_w4(q, s, z))
        x = ((torch.arange(M)[:, None] * 7 + k * 5 + k // 8) % 9 - 4).to(BF)
        want = x.double() @ w.dequantize(torch.float64).t()
        assert torch.equal(want, want.float().double()) and want.abs().max() > 0
        _witness[(M, K)] = (w, x, want)
    return _witness[(M, K)]


@pytest.mark.parametrize("K", [384, 640, 1152])
@pytest.mark.parametrize("M", [5, 16, 17, 33, 64])
@pytest.mark.parametrize("tile", TILES)
def test_exact_witness(gpu, tile, M, K):
    """Every partial sum is below 2^24 in steps of 1/2 (a block's 128 + q sum stays below
    143 * 4 * 128), so the fp32 result equals the fp64 reference or an index is wrong: the
    nibble order, the group, the zero point, the xsum row, the K pairing, a ring stage past the
    slice's end (K = 384: 3 blocks, fewer than either ring; K = 640: 5)."""
    w, x, want = witness(M, K)
    w, x = w.to(gpu), x.to(gpu)
    for splits in (1, 2):
        p = plan(tile, splits)
        if not G.tile_slices_ok(K, splits):       # 192- / 320- / 576-wide slices: refused
            assert not w.mfma_ok(M, p) and ops._pick_kernel(x, w, p, "f32")[0] == "gemm"
            continue
        assert ops._pick_kernel(x, w, p, "f32")[0] == "w4_stream"
        y = ops._gemm_native(x, w, "f32", plan=p)
        assert y.dtype == torch.float32 and torch.equal(y.cpu().double(), want), splits


def test_exact_witness_in_two_slices(gpu):
    """K = 1280 = 2 x 5 blocks: each slice shorter than tile 74's ring, one trip and a tail of
    tile 75's."""
    w, x, want = witness(33, 1280)
    for tile in TILES:
        y = ops._gemm_native(x.to(gpu), w.to(gpu), "f32", plan=plan(tile, 2))
        assert torch.equal(y.cpu().double(), want), tile


@pytest.mark.parametrize("M", [5, 48])
@pytest.mark.parametrize("tile", TILES)
def test_epilogues_and_slabs(gpu, tile, M):
    torch.manual_seed(3)
    N = 96
    # K = 640 takes one slice only (320 is no whole group); K = 768 in two: the reduce kernel's
    # epilogues, then the slabs alone under the add + RMSNorm
    assert not G.tile_slices_ok(640, 2)
    for K, splits in ((640, 1), (768, 2)):
        p = plan(tile, splits)
        w, wf = w4_weight(N, K, gpu, seed=K)
        x, b = rnd(M, K, dev=gpu), rnd(N, dev=gpu)
        y = x.double() @ wf.t()
        assert w.mfma_ok(M, p)
        for epi, ref in (("none", y), ("bias", y + b.double()),
                         ("silu_mul", R.silu_mul(y.to(BF)))):
            out = ops._gemm_native(x, w, epi, bias=b if epi == "bias" else None, plan=p)
            assert out.dtype == BF and out.shape == ref.shape
            close(out, ref)
    r0, nw = rnd(M, N, dev=gpu), rnd(N, dev=gpu)
    ref_out, ref_res = R.fused_add_rmsnorm(y.to(BF), r0, nw, 1e-5)
    res = r0.clone()
    close(ops.linear_add_rmsnorm(x, w, res, nw, 1e-5, plan=p), ref_out)
    close(res, ref_res)


@pytest.mark.parametrize("tile", TILES)
def test_no_dequantise_pass_under_a_stream_plan(gpu, tile, bf16_calls):
    torch.manual_seed(8)
    w, wf = w4_weight(96, 1024, gpu, seed=4)
    r0, nw = rnd(65, 96, dev=gpu), rnd(96, dev=gpu)
    for M, calls in ((5, 0), (64, 0), (65, 1)):
        x = rnd(M, 1024, dev=gpu)
        y = x.double() @ wf.t()
        for splits in (1, 2):
            n0 = len(bf16_calls)
            close(ops._gemm_native(x, w, "none", plan=plan(tile, splits)), y)
            assert len(bf16_calls) - n0 == calls, (M, splits)
        n0 = len(bf16_calls)
        res = r0[:M].clone()
        ops.linear_add_rmsnorm(x, w, res, nw, 1e-5, plan=plan(tile, 2))
        close(res, R.fused_add_rmsnorm(y.to(BF), r0[:M], nw, 1e-5)[1], rtol=1e-2)
        assert len(bf16_calls) - n0 == calls, M


@pytest.mark.parametrize("tile", TILES)
def test_engine_at_batch_8_under_stream_plans(gpu, tile, monkeypatch, request):
    """tests/test_w4_weights_gpu.py's engine at batch 8 with the layer's four projections pinned
    on the stream tile, eager and graph-captured, against the CPU reference run: that test's
    logit bound and near-tie rule."""
    monkeypatch.setenv("DLI_GEMM_AUTOTUNE", "0")
    G.clear_plans()
    request.addfinalizer(G.clear_plans)
    D, F = CFG.hidden_size, CFG.intermediate_size
    qkv = (CFG.num_heads + 2 * CFG.num_kv_heads) * CFG.head_dim
    for N, K, epi, splits in ((qkv, D, "splitk", 2), (D, CFG.num_heads * CFG.head_dim, "splitk", 1),
                              (D, CFG.num_heads * CFG.head_dim, "none", 1),
                              (2 * F, D, "silu_mul", 1), (D, F, "splitk", 2)):
        assert G.tile_slices_ok(K, splits)
        G.set_plan(8, N, K, epi, plan(tile, splits), wd="w4")
    shapes = stage_param_shapes(CFG, 0, CFG.num_layers, True, True)
    params = quantize_params(CFG, random_init(shapes, "cpu", BF, seed=11, std=0.05), "w4")
    prompts = [IDS[i:i + 4 + i] for i in range(8)]
    t_ref, l_ref = _run("cpu", params, prompts, monkeypatch, False)
    picked = []
    real = ops._pick_kernel
    monkeypatch.setattr(ops, "_pick_kernel",
                        lambda *a, **k: (picked.append(real(*a, **k)), picked[-1])[1])
    t_gpu, l_gpu = _run("cuda", params, prompts, monkeypatch, False)
    assert sum(k == "w4_stream" for k, _, _ in picked) >= 4 * 3 * CFG.num_layers   # >= 3 steps
    assert _run("cuda", params, prompts, monkeypatch, True)[0] == t_gpu
    assert len(l_ref) == len(l_gpu) >= 6 and all(len(t) == 6 for t in t_gpu)
    for i, (a, b) in enumerate(zip(l_gpu, l_ref)):
        err = (a - b).abs().max().item()
        assert err < 0.05 * b.abs().max().item() + 0.02, (i, err)
        if [t[:i + 1] for t in t_gpu] != [t[:i + 1] for t in t_ref]:
            break                      # a near tie flipped a token: later steps see other inputs
    else:
        assert t_gpu == t_ref
