"""The FP8 MFMA weight stream (``dli_gemm_fp8_stream``, tiles ``G.FP8_STREAM_TILES``) at
4 < M <= 64: two exact witnesses (the scale index, the pairing of weight and activation
fragments along K), every epilogue and split-K consumer against the fp32 reference
``R.linear(x, R.dequantize_weight(q, s, torch.float32))``, no dequantise pass under a stream
plan, the fallbacks of what the kernel refuses, and a model / engine with stream plans pinned."""
import pytest
import torch

from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.engine import SamplingParams
from distributed_llm_inferencing_amd.engine.llm_engine import LLMEngine
from distributed_llm_inferencing_amd.models import get_config
from distributed_llm_inferencing_amd.models.model import TransformerLM
from distributed_llm_inferencing_amd.models.weights import quantize_params, random_init, \
    stage_param_shapes
from distributed_llm_inferencing_amd.ops import gemm as G
from distributed_llm_inferencing_amd.ops import reference as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F8 = torch.float8_e4m3fn
TILES = sorted(G.FP8_STREAM_TILES)


def close(a, b, rtol=2e-2, atol=2e-2):
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    tol = atol + rtol * b.abs().max().item()
    assert err <= tol, f"max err {err} > tol {tol}"


def rnd(*shape, dev, scale=1.0):
    return (torch.randn(*shape, device=dev) * scale).to(BF)


def fp8_weight(N, K, dev, lo=-10, hi=-2, seed=0):
    """Weights ~N(0, 1) in fp8 units, scales 2^lo..2^hi varying per group and block.
    Returns (ops.Fp8Weight on ``dev``, its fp32 reconstruction there)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(N, K, generator=g).to(F8)
    kb = -(-K // 128)
    s = torch.exp2(torch.rand(N // 16, kb, generator=g) * (hi - lo) + lo).float()
    w = ops.Fp8Weight(q.to(dev), s.to(dev))
    return w, R.dequantize_weight(w.q, w.scale, torch.float32)


def plan(tile, splits=1):
    return G.GemmPlan("dli", tile, splits)


@pytest.fixture
def bf16_calls(monkeypatch):
    """The calls of ``ops.Fp8Weight.bf16`` (the dequantise pass) during the test."""
    calls = []
    real = ops.Fp8Weight.bf16
    monkeypatch.setattr(ops.Fp8Weight, "bf16", lambda self: (calls.append(1), real(self))[1])
    return calls


@pytest.fixture
def clean_plans():
    G.clear_plans()
    yield
    G.clear_plans()


# ----------------------------------------------------------------------------- witnesses
WN, WK = 80, 1040          # tails in both directions for 64 / 128 rows a workgroup, 9 blocks


def witness_scales():
    """(2 i + 1) * 2^-(i % 7): 45 distinct scales, exact wherever they multiply a small value."""
    kb = -(-WK // 128)
    i = torch.arange((WN // 16) * kb, dtype=torch.float32)
    s = ((2 * i + 1) * torch.exp2(-(i % 7))).view(WN // 16, kb)
    assert s.unique().numel() == s.numel() == 45 and 2 * i.max() + 1 < 256
    return s


@pytest.mark.parametrize("M", [5, 16, 17, 64])
def test_scale_index_witness(gpu, M):
    """Every weight byte is fp8 1.0, x is one-hot at column k with its own value per row:
    y[m, n] = x[m, k] * s[n // 16, k // 128] exactly. A wrong block, row group or row is a
    mismatch, not a tolerance question."""
    s = witness_scales()
    w = ops.Fp8Weight(torch.ones(WN, WK).to(F8).to(gpu), s.to(gpu))
    xv = ((torch.arange(M, dtype=torch.float32) + 1) / 8).to(BF)       # (m + 1) / 8: exact
    assert torch.equal(xv.float(), (torch.arange(M, dtype=torch.float32) + 1) / 8)
    for k in (0, 15, 16, 63, 64, 127, 128, 1023, 1024, WK - 17, WK - 1):
        x = torch.zeros(M, WK, dtype=BF)
        x[:, k] = xv
        want = xv.float()[:, None] * s[:, k // 128].repeat_interleave(16)[None, :]
        xg = x.to(gpu)
        for tile in TILES:
            y = ops._gemm_native(xg, w, "f32", plan=plan(tile))
            assert y.dtype == torch.float32 and y.shape == (M, WN)
            assert torch.equal(y.cpu(), want), (k, tile)


def pairing_case(M):
    """One fp8 1.0 per weight row, at k_n = (37 n + 11) % K; x multiples of 1/8 in [-2, 2]."""
    s = witness_scales()
    n = torch.arange(WN)
    kn = (37 * n + 11) % WK
    q = torch.zeros(WN, WK)
    q[n, kn] = 1.0
    k = torch.arange(WK)[None, :]
    m = torch.arange(M)[:, None]
    x = ((((7 * k + 3 * m) % 31) - 15).float() / 8).to(BF)
    want = x.float()[:, kn] * s[n // 16, kn // 128][None, :]
    return q.to(F8), s, x, want


@pytest.mark.parametrize("M", [5, 33, 64])
def test_k_pairing_witness(gpu, M):
    """A weight fragment that met the x fragment of other K indices would pick another x
    value: y[m, n] = x[m, k_n] * s[n // 16, k_n // 128] exactly. The expectation is checked
    against the fp32 reference on the CPU first."""
    q, s, x, want = pairing_case(M)
    assert torch.equal(want, R.linear(x, R.dequantize_weight(q, s, torch.float32),
                                      out_dtype=torch.float32))
    assert want.abs().max() > 0 and x.float().unique().numel() == 31
    w = ops.Fp8Weight(q.to(gpu), s.to(gpu))
    xg = x.to(gpu)
    for tile in TILES:
        y = ops._gemm_native(xg, w, "f32", plan=plan(tile))
        assert torch.equal(y.cpu(), want), tile


# ----------------------------------------------------------------------------- epilogues
_refs = {}


def epi_case(gpu, M, K):
    """Operands and the fp32 product, computed once per (M, K) and shared by the epilogues."""
    if (M, K) not in _refs:
        torch.manual_seed(3)
        w, wf = fp8_weight(96, K, gpu, seed=K)
        x, b = rnd(M, K, dev=gpu), rnd(96, dev=gpu)
        _refs[(M, K)] = (w, x, b, R.linear(x, wf, out_dtype=torch.float32))
    return _refs[(M, K)]


# K = 1040: 9 scale blocks, the last 16 wide; the rings hold 4 (tile 70) / 2 (tile 71) blocks,
# so both loops already run past the pre-issued blocks. K = 2192: 18 blocks, five / nine trips
@pytest.mark.parametrize("K", [1040, 2192])
@pytest.mark.parametrize("M", [5, 16, 17, 48, 64])
@pytest.mark.parametrize("epi", ["none", "f32", "bias", "silu_mul"])
def test_epilogues(gpu, M, epi, K):
    w, x, b, y = epi_case(gpu, M, K)
    ref = (R.silu_mul(y.to(BF)) if epi == "silu_mul" else y + b.float() if epi == "bias" else y)
    for tile in TILES:
        out = ops._gemm_native(x, w, epi, bias=b if epi == "bias" else None, plan=plan(tile))
        assert out.dtype == (torch.float32 if epi == "f32" else BF)
        assert out.shape == (M, 48 if epi == "silu_mul" else 96)
        close(out, ref)


# ----------------------------------------------------------------------------- split-K
HQ, HKV, HD = 2, 1, 64


def qkv_case(gpu, M, K=1024, seed=4):
    torch.manual_seed(8)
    N = (HQ + 2 * HKV) * HD
    w, wf = fp8_weight(N, K, gpu, seed=seed)
    x = rnd(M, K, dev=gpu)
    return w, x, R.linear(x, wf, out_dtype=torch.float32)


def check_add_rmsnorm(gpu, x, w, y, p):
    M, N = y.shape
    r0, nw = rnd(M, N, dev=gpu), rnd(N, dev=gpu)
    ref_out, ref_res = R.fused_add_rmsnorm(y.to(BF), r0, nw, 1e-5)
    res = r0.clone()
    out = ops.linear_add_rmsnorm(x, w, res, nw, 1e-5, plan=p)
    close(out, ref_out, atol=3e-2)
    close(res, ref_res, rtol=1e-2)


def check_rope_cache(gpu, x, w, y, p):
    M = y.shape[0]
    pos = torch.arange(M, dtype=torch.int32, device=gpu)
    slots = torch.arange(M, dtype=torch.int32, device=gpu)
    kc = torch.zeros(-(-M // 16), HKV, 16, HD, dtype=BF, device=gpu)
    vc = torch.zeros_like(kc)
    cs = R.rope_cos_sin(128, HD, 10000.0, device=gpu)
    ref = y.to(BF)
    kc1, vc1 = kc.clone(), vc.clone()
    R.rope_and_cache(ref, pos, slots, cs, kc1, vc1, HQ, HKV, HD)
    got = ops.linear_rope_cache(x, w, pos, slots, cs, kc, vc, HQ, HKV, HD, plan=p)
    close(got, ref)
    close(kc, kc1)
    close(vc, vc1)


@pytest.mark.parametrize("M", [5, 64])
@pytest.mark.parametrize("splits", [2, 4])
def test_split_k(gpu, M, splits):
    """K = 1024 in slices of 512 / 256: the fp32 slabs summed, reduced by the add + RMSNorm and
    the RoPE + cache kernels (slab format 0), and by the reduce kernel into C (bf16 and
    SiLU*up)."""
    w, x, y = qkv_case(gpu, M)
    N = y.shape[1]
    for tile in TILES:
        p = plan(tile, splits)
        assert w.stream_ok(M, p)
        ws = G.workspace(x.device, splits * M * N * 4)
        assert ops._slab_gemm(x, w, p, ws) == 0
        close(ws[:splits * M * N * 4].view(torch.float32).view(splits, M, N).sum(0), y)
        check_add_rmsnorm(gpu, x, w, y, p)
        check_rope_cache(gpu, x, w, y, p)
        close(ops._gemm_native(x, w, "none", plan=p), y)
        close(ops._gemm_native(x, w, "silu_mul", plan=p), R.silu_mul(y.to(BF)))


# ----------------------------------------------------------------------------- no dequantise
@pytest.mark.parametrize("M", [5, 64])
def test_no_dequantise_pass_under_a_stream_plan(gpu, M, bf16_calls, clean_plans):
    w, x, y = qkv_case(gpu, M)
    for tile in TILES:
        for splits in (1, 2):
            p = plan(tile, splits)
            close(ops._gemm_native(x, w, "none", plan=p), y)
            check_add_rmsnorm(gpu, x, w, y, p)
            check_rope_cache(gpu, x, w, y, p)
    assert bf16_calls == []
    # no forced plan, nothing cached for the shape: the heuristic plan, which dequantises
    for epi in ("none", "splitk"):
        G._plan_cache.pop(G._key(M, y.shape[1], x.shape[1], epi, "fp8"), None)
    close(ops.linear(x, w), y)
    assert len(bf16_calls) == 1
    check_add_rmsnorm(gpu, x, w, y, None)
    assert len(bf16_calls) == 2
    check_rope_cache(gpu, x, w, y, None)
    assert len(bf16_calls) == 3


# ----------------------------------------------------------------------------- refusals
def check_falls_back(gpu, M, K, splits, bf16_calls):
    w, x, y = qkv_case(gpu, M, K, seed=5)
    base = ops.linear(x, w.bf16())                # the heuristic plan on the dequantised image
    n0 = len(bf16_calls)
    assert n0 == 1
    for tile in TILES:
        p = plan(tile, splits)
        assert not w.stream_ok(M, p)
        out = ops._gemm_native(x, w, "none", plan=p)
        close(out, base)
        close(out, y)
    assert len(bf16_calls) == n0 + len(TILES)


@pytest.mark.parametrize("M", [4, 65])
def test_m_outside_the_range_falls_back(gpu, M, bf16_calls, clean_plans):
    check_falls_back(gpu, M, 1024, 1, bf16_calls)
    # the slab form too: a cached split plan that meets a neighbouring M
    w, x, y = qkv_case(gpu, M)
    for tile in TILES:
        n0 = len(bf16_calls)
        check_add_rmsnorm(gpu, x, w, y, plan(tile, 2))
        assert len(bf16_calls) == n0 + 1


def test_k_not_a_multiple_of_16_falls_back(gpu, bf16_calls, clean_plans):
    """K = 1032 at M = 3: the bf16 MFMA tiles take K in multiples of 64 only, so the rows that
    have a dequantise path at this K are the GEMV's (M <= 4); the K predicate alone at M = 8 is
    in test_fp8_stream_plan.py's truth table."""
    check_falls_back(gpu, 3, 1032, 1, bf16_calls)
    w, _ = fp8_weight(96, 1032, gpu)
    assert not any(w.stream_ok(8, plan(t)) for t in TILES)


def test_slices_that_split_a_scale_block_fall_back(gpu, bf16_calls, clean_plans):
    """K = 1152 in two slices of 576: the second would start inside a 128-column block."""
    check_falls_back(gpu, 5, 1152, 2, bf16_calls)
    w, x, y = qkv_case(gpu, 5, 1152, seed=5)
    for tile in TILES:                            # unsplit, the same K streams
        n0 = len(bf16_calls)
        close(ops._gemm_native(x, w, "none", plan=plan(tile)), y)
        assert len(bf16_calls) == n0


def test_a_bf16_weight_with_a_stream_tile_is_an_error(gpu):
    x, w = rnd(8, 1024, dev=gpu), rnd(96, 1024, dev=gpu)
    res, nw = rnd(8, 96, dev=gpu), rnd(96, dev=gpu)
    for tile in TILES:
        with pytest.raises(ValueError, match=str(tile)):
            ops._gemm_native(x, w, "none", plan=plan(tile))
        with pytest.raises(ValueError, match=str(tile)):
            ops.linear_add_rmsnorm(x, w, res, nw, 1e-5, plan=plan(tile, 2))


# ----------------------------------------------------------------------------- model, engine
CFG = get_config("llama-tiny128", 2)
IDS = [5, 17, 99, 3, 250, 7, 8, 1000, 42, 11, 600, 3, 3, 9]
BATCH = 8


@pytest.fixture(scope="module")
def fp8_params():
    shapes = stage_param_shapes(CFG, 0, CFG.num_layers, True, True)
    return quantize_params(CFG, random_init(shapes, "cpu", BF, seed=11, std=0.05))


@pytest.fixture
def stream_plans(request, monkeypatch):
    """A stream plan pinned for the layer's four projections at the decode batch: QKV split 2
    (the fused RoPE + attention consumer), O unsplit, gate/up with SiLU*up, down split 4."""
    monkeypatch.setenv("DLI_GEMM_AUTOTUNE", "0")
    G.clear_plans()
    request.addfinalizer(G.clear_plans)

    def pin(tile):
        D, F = CFG.hidden_size, CFG.intermediate_size
        qkv = (CFG.num_heads + 2 * CFG.num_kv_heads) * CFG.head_dim
        G.set_plan(BATCH, qkv, D, "splitk", plan(tile, 2), wd="fp8")
        G.set_plan(BATCH, D, CFG.num_heads * CFG.head_dim, "splitk", plan(tile, 1), wd="fp8")
        G.set_plan(BATCH, D, CFG.num_heads * CFG.head_dim, "none", plan(tile, 1), wd="fp8")
        G.set_plan(BATCH, 2 * F, D, "silu_mul", plan(tile, 1), wd="fp8")
        G.set_plan(BATCH, D, F, "splitk", plan(tile, 4), wd="fp8")
    return pin


def _decode_spy(monkeypatch, bf16_calls):
    """bf16() calls made inside each decode step of BATCH rows."""
    per_step = []
    real = TransformerLM.forward_layers

    def spy(self, x, b, kv_caches):
        n0 = len(bf16_calls)
        out = real(self, x, b, kv_caches)
        if not b.is_prefill and x.is_cuda and x.shape[0] == BATCH:
            per_step.append(len(bf16_calls) - n0)
        return out
    monkeypatch.setattr(TransformerLM, "forward_layers", spy)
    return per_step


def _step_logits(device, params, prompts, steps, monkeypatch, **kw):
    logits = []
    real = TransformerLM.sample

    def spy(self, lg, b, generator=None):
        logits.append(lg.float().cpu())
        return real(self, lg, b, generator=generator)
    monkeypatch.setattr(TransformerLM, "sample", spy)
    eng = LLMEngine(CFG, device=device, params=params, max_batch=8, max_model_len=64,
                    num_blocks=64, use_graphs=False, lookahead=False, **kw)
    sp = SamplingParams(max_new_tokens=steps, temperature=0.0, ignore_eos=True)
    toks = [o.output_ids for o in eng.generate(prompts, sp)]
    monkeypatch.setattr(TransformerLM, "sample", real)
    return eng, toks, logits


@pytest.mark.parametrize("tile", TILES)
def test_model_logits_under_stream_plans(gpu, fp8_params, tile, stream_plans, bf16_calls,
                                         monkeypatch):
    """Prefill, then decode at batch 8 with every projection on the stream tile: every step's
    logits against a CPU engine holding the fp32 reconstruction of the same weights, and no
    dequantise pass inside the decode steps."""
    stream_plans(tile)
    per_step = _decode_spy(monkeypatch, bf16_calls)
    prompts = [IDS[i:i + 4 + i] for i in range(BATCH)]
    deq = {}
    for k, v in fp8_params.items():
        if k.endswith("_scale"):
            continue
        deq[k] = (R.dequantize_weight(v, fp8_params[k + "_scale"], torch.float32)
                  if v.dtype == F8 else v)
    _, t_ref, l_ref = _step_logits("cpu", deq, prompts, 4, monkeypatch)
    eng, t_gpu, l_gpu = _step_logits("cuda", fp8_params, prompts, 4, monkeypatch)
    assert eng.stats()["weight_dtype"] == "fp8"
    assert len(l_ref) == len(l_gpu) >= 4
    for i, (a, b) in enumerate(zip(l_gpu, l_ref)):
        assert a.shape == b.shape
        err = (a - b).abs().max().item()
        assert err < 0.05 * b.abs().max().item() + 0.02, (i, err)
        if [t[:i + 1] for t in t_gpu] != [t[:i + 1] for t in t_ref]:
            break                      # a near tie flipped a token: later steps see other inputs
    assert len(per_step) >= 3 and not any(per_step), per_step


@pytest.mark.parametrize("tile", TILES)
def test_graph_decode_equals_eager_under_stream_plans(gpu, fp8_params, tile, stream_plans,
                                                      bf16_calls, monkeypatch):
    stream_plans(tile)
    per_step = _decode_spy(monkeypatch, bf16_calls)
    prompts = [IDS[i:i + 4 + i] for i in range(BATCH)]
    sp = SamplingParams(max_new_tokens=12, temperature=0.0, ignore_eos=True)
    outs = []
    for graphs in (False, True):
        eng = LLMEngine(CFG, device="cuda", params=fp8_params, max_batch=8, max_model_len=64,
                        num_blocks=64, use_graphs=graphs)
        assert eng.weight_dtype == "fp8"
        outs.append([o.output_ids for o in eng.generate(prompts, sp)])
    assert outs[0] == outs[1] and all(len(t) == 12 for t in outs[0])
    assert len(per_step) >= 11 and not any(per_step), per_step
