"""FP8 block-scaled weights on the GPU: the dequantise kernel (byte for byte), the M <= 4
weight stream (an exact scale-index witness, then every epilogue against the fp32 reference
``R.linear(x, R.dequantize_weight(q, s, torch.float32))``), the dequantise-then-GEMM path of
every other shape, and a model / engine on FP8 weights."""
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


# ----------------------------------------------------------------------------- dequantise
@pytest.mark.parametrize("N,K", [(48, 384), (160, 128), (32, 144), (32, 136), (16, 1032)])
def test_dequant_kernel_is_the_reference_byte_for_byte(gpu, N, K):
    """K = 136 and 1032 are no multiples of 16: the one-element-per-thread kernel."""
    g = torch.Generator().manual_seed(N + K)
    b = (torch.arange(N * K, dtype=torch.int32) * 7 + 3) % 256     # every byte value
    b[(b & 0x7F) == 0x7F] -= 1                                       # NaN -> +-448
    q = b.to(torch.uint8).view(N, K).view(F8)
    assert {0x00, 0x80, 0x01, 0x07, 0x7E, 0xFE} <= set(b.tolist())  # +-0, subnormals, +-448
    s = torch.exp2(torch.rand(N // 16, -(-K // 128), generator=g) * 14 - 12).float()
    ref = R.dequantize_weight(q, s, BF)
    got = ops.Fp8Weight(q.to(gpu), s.to(gpu)).bf16()
    assert got.dtype == BF and got.shape == (N, K)
    assert torch.equal(got.cpu().view(torch.int16), ref.view(torch.int16))


# ----------------------------------------------------------------------------- witness
def _f32_tiles(M):
    return [t for t in G.GEMV_TILES if G.tile_ok(t, "f32") and not (t in G.GEMV_M1_ONLY and M > 1)]


@pytest.mark.parametrize("M", [1, 4])
def test_scale_index_witness(gpu, M):
    """Every weight byte is fp8 1.0 and every scale a distinct odd integer times a power of
    two; x is one-hot at column k. y[m, n] = x[m, k] * s[n // 16, k // 128] exactly: a wrong
    block or row-group index is a mismatch, not a tolerance question."""
    N, K = 80, 1040
    kb = -(-K // 128)
    i = torch.arange((N // 16) * kb, dtype=torch.float32)
    s = ((2 * i + 1) * torch.exp2(-(i % 7))).view(N // 16, kb)
    assert s.unique().numel() == s.numel()
    q = torch.ones(N, K).to(F8)
    w = ops.Fp8Weight(q.to(gpu), s.to(gpu))
    xv = torch.tensor([1.0, 1.5, -2.0, 0.75][:M], dtype=BF)
    tiles = _f32_tiles(M)
    assert {30, 31, 56, 57} <= set(tiles)
    for k in (0, 15, 16, 127, 128, 1023, 1024, K - 17, K - 1):
        x = torch.zeros(M, K, dtype=BF)
        x[:, k] = xv
        want = xv.float()[:, None] * s[:, k // 128].repeat_interleave(16)[None, :]
        xg = x.to(gpu)
        for tile in tiles:
            y = ops._gemm_native(xg, w, "f32", plan=G.GemmPlan("dli", tile, 1))
            assert y.dtype == torch.float32
            assert torch.equal(y.cpu(), want), (k, tile)


# ----------------------------------------------------------------------------- GEMV
def _shapes(tile, silu):
    """(N, K) for a tile: one full step plus a masked tail at its depth."""
    if tile in (56, 57, 58, 59):
        return 96, 9232
    return (96 if silu else 80), 1040


@pytest.mark.parametrize("M", [1, 2, 3, 4])
@pytest.mark.parametrize("epi", ["none", "f32", "bias", "silu_mul"])
def test_gemv_epilogues(gpu, M, epi):
    torch.manual_seed(3)
    ran = 0
    refs = {}
    for tile in G.GEMV_TILES:
        if not G.tile_ok(tile, epi) or (tile in G.GEMV_M1_ONLY and M > 1):
            continue
        N, K = _shapes(tile, epi == "silu_mul")
        if (N, K) not in refs:
            w, wf = fp8_weight(N, K, gpu, seed=K)
            x, b = rnd(M, K, dev=gpu), rnd(N, dev=gpu)
            y = R.linear(x, wf, out_dtype=torch.float32)
            ref = (R.silu_mul(y.to(BF)) if epi == "silu_mul"
                   else y + b.float() if epi == "bias" else y)
            refs[(N, K)] = (w, x, b, ref)
        w, x, b, ref = refs[(N, K)]
        out = ops._gemm_native(x, w, epi, bias=b if epi == "bias" else None,
                               plan=G.GemmPlan("dli", tile, 1))
        assert out.dtype == (torch.float32 if epi == "f32" else BF)
        close(out, ref)
        ran += 1
    assert ran >= 2


@pytest.mark.parametrize("M", [1, 2, 3, 4])
@pytest.mark.parametrize("splits", [2, 4])
def test_gemv_split_k_slabs(gpu, M, splits):
    """K slices that start inside a 128-column block (1088 / 4 = 272): the sum of the fp32
    slabs, and the reduce kernel's bf16 / SiLU*up output."""
    torch.manual_seed(4)
    N, K = 96, 1088
    w, wf = fp8_weight(N, K, gpu, seed=1)
    x = rnd(M, K, dev=gpu)
    y = R.linear(x, wf, out_dtype=torch.float32)
    for tile in (30, 56, 57):
        p = G.GemmPlan("dli", tile, splits)
        assert w.gemv_ok(M, p)
        ws = G.workspace(x.device, splits * M * N * 4)
        assert ops._slab_gemm(x, w, p, ws) == 0
        close(ws[:splits * M * N * 4].view(torch.float32).view(splits, M, N).sum(0), y)
        close(ops._gemm_native(x, w, "none", plan=p), y)
    for tile in (29, 31, 58, 59):
        close(ops._gemm_native(x, w, "silu_mul", plan=G.GemmPlan("dli", tile, splits)),
              R.silu_mul(y.to(BF)))


@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_gemv_residual_epilogue(gpu, M):
    torch.manual_seed(5)
    for tile in G.GEMV_RES_TILES:
        if tile in G.GEMV_M1_ONLY and M > 1:
            continue
        N, K = _shapes(tile, False)
        w, wf = fp8_weight(N, K, gpu, seed=2)
        x, r0 = rnd(M, K, dev=gpu), rnd(M, N, dev=gpu)
        ref = (r0.float() + R.linear(x, wf, out_dtype=torch.float32).to(BF).float()).to(BF)
        res = r0.clone()
        ops.linear_residual(x, w, res, plan=G.GemmPlan("dli", tile, 1))
        close(res, ref, rtol=1e-2, atol=2e-2)


@pytest.mark.parametrize("M", [1, 4])          # the runtime-branch and the template prologue
@pytest.mark.parametrize("epi", ["none", "silu_mul", "splitk"])
def test_gemv_norm_prologue(gpu, M, epi):
    torch.manual_seed(6)
    ran = 0
    for tile in G.GEMV_PRO_TILES[epi]:
        if tile in G.GEMV_PRO_M1_ONLY and M > 1:
            continue
        N, K = (96, 1088) if epi == "splitk" else (_shapes(tile, epi == "silu_mul")[0], 1040)
        w, wf = fp8_weight(N, K, gpu, seed=3)
        r, nw = rnd(M, K, dev=gpu), rnd(K, dev=gpu)
        h = ops.NormedRows(r, nw, 1e-5)
        y = R.linear(R.rmsnorm(r, nw, 1e-5), wf, out_dtype=torch.float32)
        if epi == "splitk":
            ws = torch.empty(2 * M * N, dtype=torch.float32, device=gpu)
            assert ops._gemv_prologue(h, w, "splitk", G.GemmPlan("dli", tile, 2), None, N, ws=ws)
            close(ws.view(2, M, N).sum(0), y)
        else:
            out = ops.linear_normed(h, w, epi, G.GemmPlan("dli", tile, 1))
            close(out, R.silu_mul(y.to(BF)) if epi == "silu_mul" else y)
        ran += 1
    assert ran


@pytest.mark.parametrize("M", [1, 4])
@pytest.mark.parametrize("epi", ["none", "silu_mul"])
def test_gemv_norm_prologue_past_the_first_steps(gpu, M, epi):
    """K = 4112 = 257 chunks: after the prologue's pre-issued steps (128 chunks at 2 steps in
    flight, 256 at 4) the full-iteration loop and the masked one-chunk tail run too, as at the
    production K = 4096; K > 4096 also takes the 4-vector norm prologue."""
    torch.manual_seed(7)
    N, K = 96, 4112
    w, wf = fp8_weight(N, K, gpu, seed=6)
    r, nw = rnd(M, K, dev=gpu), rnd(K, dev=gpu)
    h = ops.NormedRows(r, nw, 1e-5)
    y = R.linear(R.rmsnorm(r, nw, 1e-5), wf, out_dtype=torch.float32)
    ref = R.silu_mul(y.to(BF)) if epi == "silu_mul" else y
    ran = 0
    for tile in G.GEMV_PRO_TILES[epi]:
        if tile in G.GEMV_PRO_M1_ONLY and M > 1:
            continue
        p = G.GemmPlan("dli", tile, 1)
        assert w.gemv_ok(M, p)
        close(ops.linear_normed(h, w, epi, p), ref)
        ran += 1
    assert ran >= 3


# ----------------------------------------------------------------------------- fallback
@pytest.mark.parametrize("M", [5, 64])
def test_other_batches_dequantise_then_gemm(gpu, M, monkeypatch):
    torch.manual_seed(8)
    calls = []
    real = ops.Fp8Weight.bf16
    monkeypatch.setattr(ops.Fp8Weight, "bf16", lambda self: (calls.append(1), real(self))[1])
    hq, hkv, hd = 2, 1, 64
    N, K = (hq + 2 * hkv) * hd, 1024
    w, wf = fp8_weight(N, K, gpu, seed=4)
    x = rnd(M, K, dev=gpu)
    y = R.linear(x, wf, out_dtype=torch.float32)
    close(ops.linear(x, w), y)
    r0, nw = rnd(M, N, dev=gpu), rnd(N, dev=gpu)
    ref_out, ref_res = R.fused_add_rmsnorm(y.to(BF), r0, nw, 1e-5)
    res = r0.clone()
    out = ops.linear_add_rmsnorm(x, w, res, nw, 1e-5)
    close(out, ref_out, atol=3e-2)
    close(res, ref_res, rtol=1e-2)
    pos = torch.arange(M, dtype=torch.int32, device=gpu)
    slots = torch.arange(M, dtype=torch.int32, device=gpu)
    kc = torch.zeros(-(-M // 16), hkv, 16, hd, dtype=BF, device=gpu)
    vc = torch.zeros_like(kc)
    cs = R.rope_cos_sin(128, hd, 10000.0, device=gpu)
    ref = y.to(BF)
    kc1, vc1 = kc.clone(), vc.clone()
    R.rope_and_cache(ref, pos, slots, cs, kc1, vc1, hq, hkv, hd)
    got = ops.linear_rope_cache(x, w, pos, slots, cs, kc, vc, hq, hkv, hd)
    close(got, ref)
    close(kc, kc1)
    close(vc, vc1)
    assert len(calls) >= 3


def test_k_not_a_multiple_of_16_takes_the_dequant_path(gpu, monkeypatch):
    torch.manual_seed(9)
    calls = []
    real = ops.Fp8Weight.bf16
    monkeypatch.setattr(ops.Fp8Weight, "bf16", lambda self: (calls.append(1), real(self))[1])
    N, K = 96, 1032
    w, wf = fp8_weight(N, K, gpu, seed=5)
    x = rnd(1, K, dev=gpu)
    p = G.plan(1, N, K, "none", G.wdt(w))
    assert p.tile in G.GEMV_TILES and not w.gemv_ok(1, p)
    close(ops.linear(x, w), R.linear(x, wf, out_dtype=torch.float32))
    assert calls


# ----------------------------------------------------------------------------- model, engine
CFG = get_config("llama-tiny128", 2)
IDS = [5, 17, 99, 3, 250, 7, 8, 1000, 42, 11, 600, 3, 3, 9]


@pytest.fixture(scope="module")
def fp8_params():
    shapes = stage_param_shapes(CFG, 0, CFG.num_layers, True, True)
    return quantize_params(CFG, random_init(shapes, "cpu", BF, seed=11, std=0.05))


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


@pytest.mark.parametrize("batch", [1, 3, 8])
def test_model_logits_against_the_dequantised_reference(gpu, fp8_params, batch, monkeypatch):
    """Prefill, then decode at batch 1 (the deferred-norm FP8 GEMV chain), 3 (FP8 GEMVs with
    the split-K reduces) and 8 (dequantise, then the bf16 GEMMs): every step's logits against
    a CPU engine holding the fp32 reconstruction of the same weights."""
    monkeypatch.setenv("DLI_GEMM_AUTOTUNE", "0")
    G.clear_plans()
    prompts = [IDS[i:i + 4 + i] for i in range(batch)]
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


@pytest.mark.parametrize("batch,kv", [(1, "bf16"), (8, "bf16"), (1, "fp8")])
def test_graph_decode_equals_eager(gpu, fp8_params, batch, kv, monkeypatch):
    monkeypatch.setenv("DLI_GEMM_AUTOTUNE", "0")
    G.clear_plans()
    prompts = [IDS[i:i + 4 + i] for i in range(batch)]
    sp = SamplingParams(max_new_tokens=12, temperature=0.0, ignore_eos=True)
    outs = []
    for graphs in (False, True):
        eng = LLMEngine(CFG, device="cuda", params=fp8_params, max_batch=8, max_model_len=64,
                        num_blocks=64, use_graphs=graphs, kv_dtype=kv)
        assert eng.weight_dtype == "fp8"
        outs.append([o.output_ids for o in eng.generate(prompts, sp)])
    assert outs[0] == outs[1] and all(len(t) == 12 for t in outs[0])
