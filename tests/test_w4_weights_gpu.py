"""4-bit group-scaled weights on the GPU: the dequantise kernel, the M <= 4 weight stream (exact
integer witness, then every epilogue against the fp64 product of the dequantised weight), the
dequantise-then-GEMM path and an engine on 4-bit weights."""
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
CH = G.W4_CHUNK
plan = lambda tile, splits=1: G.GemmPlan("dli", tile, splits)  # noqa: E731


def close(a, b, rtol=2e-2, atol=2e-2):          # tests/test_fp8_weights_gpu.py's tolerance
    err = (a.float() - b.float()).abs().max().item()
    assert err <= atol + rtol * b.float().abs().max().item(), err


def rnd(*shape, dev):
    return torch.randn(*shape, device=dev).to(BF)


def w4_weight(N, K, dev, seed=0):
    """Random nibbles and zero points, scales 2^-8..2^-4: (ops.W4Weight, its fp64 value)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    z = torch.randint(0, 16, (N, K // 128), generator=g, dtype=torch.uint8)
    s = torch.exp2(torch.rand(N, K // 128, generator=g) * 4 - 8).to(torch.float16)
    w = ops.W4Weight(*R.pack_w4(q, s, z)).to(dev)
    return w, w.dequantize(torch.float64)


@pytest.mark.parametrize("N", [16, 48])
@pytest.mark.parametrize("K", [128, 384])
def test_dequant_kernel_is_the_reference_byte_for_byte(gpu, N, K):
    w, _ = w4_weight(N, K, "cpu", seed=N + K)
    got = w.to(gpu).bf16()
    assert got.dtype == BF and got.shape == (N, K)
    assert torch.equal(got.cpu().view(torch.int16), w.dequantize(BF).view(torch.int16))


def unroll(tile, M):
    """K-steps in flight per lane (gemv.h dispatch_gemv)."""
    if tile in (29, 57, 59):
        return (8 if tile > 29 else 4) if M == 1 else (4 if tile > 29 else 2)
    return {30: 2, 31: 2, 32: 4, 33: 4, 56: 8, 58: 8}[tile]


@pytest.mark.parametrize("tile,M,splits", [
    (t, M, sp) for t in G.GEMV_TILES for M in (1, 2, 3, 4) for sp in (1, 2)
    if not (t in G.GEMV_M1_ONLY and M > 1) and (G.tile_ok(t, "f32") or sp == 2)])
def test_exact_witness(gpu, tile, M, splits):
    """Integers everywhere and power-of-two scales, so every sum is exact in fp32 (below 2^23
    in steps of 1/2): the result equals the fp64 reference or an index is wrong. Tiles without
    an fp32 epilogue (SiLU*up only) are read through their fp32 split-K slabs."""
    f32 = G.tile_ok(tile, "f32")
    N = 48 if f32 else 64
    full = unroll(tile, M) * 64 * CH
    for K in (384, (full + 384) * splits, full * splits):   # tail only; full + tail; full
        n, k, grp = torch.arange(N)[:, None], torch.arange(K)[None, :], torch.arange(K // 128)
        q = ((k + 3 * (k // 8) + 5 * n) % 16).to(torch.uint8)
        z = ((5 * n + 3 * grp) % 16).to(torch.uint8)
        s = torch.exp2(((n + grp) % 3 - 1).float()).to(torch.float16)
        w = ops.W4Weight(*R.pack_w4(q, s, z)).to(gpu)
        x = ((torch.arange(M)[:, None] * 7 + k * 5 + k // 8) % 9 - 4).to(BF)
        want = x.double() @ w.dequantize(torch.float64).cpu().t()
        assert ops._pick_kernel(x.to(gpu), w, plan(tile, splits), "f32")[0] == "gemv_w4"
        y = ops._gemm_native(x.to(gpu), w, "f32" if f32 else "silu_mul", plan=plan(tile, splits))
        if not f32:
            ws = G.workspace(gpu, splits * M * N * 4)
            y = ws[:splits * M * N * 4].view(torch.float32).view(splits, M, N).sum(0)
        assert torch.equal(y.cpu().double(), want), K


def _shape(tile, silu):
    """(N, K): a full iteration of the 2-step / 8-step tiles plus a masked tail."""
    return (96 if silu else 80), (8 * 64 * CH + 384 if tile >= 56 else 2 * 64 * CH + 384)


@pytest.mark.parametrize("M", [1, 2, 3, 4])
@pytest.mark.parametrize("epi", ["none", "bias", "silu_mul"])
def test_gemv_epilogues_and_split_k(gpu, M, epi):
    torch.manual_seed(3)
    ran = 0
    for tile in G.GEMV_TILES:
        if not G.tile_ok(tile, epi) or (tile in G.GEMV_M1_ONLY and M > 1):
            continue
        N, K = _shape(tile, epi == "silu_mul")
        w, wf = w4_weight(N, K, gpu, seed=K)
        x, b = rnd(M, K, dev=gpu), rnd(N, dev=gpu)
        y = x.double() @ wf.t()
        ref = R.silu_mul(y.to(BF)) if epi == "silu_mul" else y + b.double() if epi == "bias" else y
        for splits in (1, 2):
            out = ops._gemm_native(x, w, epi, bias=b if epi == "bias" else None,
                                   plan=plan(tile, splits))
            assert out.dtype == BF
            close(out, ref)
            ran += 1
    assert ran >= 4


@pytest.mark.parametrize("M", [1, 4])
def test_fused_entry_and_fused_consumers(gpu, M):
    """The residual epilogue, split-K slabs reduced by the add + RMSNorm kernel, and the norm
    prologue (bf16, SiLU*up and fp32 slabs)."""
    torch.manual_seed(5)
    for tile in G.GEMV_RES_TILES:
        if tile in G.GEMV_M1_ONLY and M > 1:
            continue
        N, K = _shape(tile, False)
        w, wf = w4_weight(N, K, gpu, seed=K)
        x, r0, nw = rnd(M, K, dev=gpu), rnd(M, N, dev=gpu), rnd(N, dev=gpu)
        y = (x.double() @ wf.t()).to(BF)
        res = r0.clone()
        ops.linear_residual(x, w, res, plan=plan(tile))
        close(res, (r0.float() + y.float()).to(BF), rtol=1e-2)
        ref_out, ref_res = R.fused_add_rmsnorm(y, r0, nw, 1e-5)
        res = r0.clone()
        close(ops.linear_add_rmsnorm(x, w, res, nw, 1e-5, plan=plan(tile, 2)), ref_out, atol=3e-2)
        close(res, ref_res, rtol=1e-2)
    for epi in ("none", "silu_mul", "splitk"):
        for tile in G.GEMV_PRO_TILES[epi]:
            if tile in G.GEMV_PRO_M1_ONLY and M > 1:
                continue
            N, K = _shape(tile, epi == "silu_mul")
            K = min(K, 8192 - 7 * 128)               # the prologue holds K <= 8192 in LDS
            w, wf = w4_weight(N, K, gpu, seed=K)
            r, nw = rnd(M, K, dev=gpu), rnd(K, dev=gpu)
            h = ops.NormedRows(r, nw, 1e-5)
            y = R.rmsnorm(r, nw, 1e-5).double() @ wf.t()
            if epi == "splitk":
                ws = torch.empty(2 * M * N, dtype=torch.float32, device=gpu)
                assert ops._gemv_prologue(h, w, "splitk", plan(tile, 2), None, N, ws=ws)
                close(ws.view(2, M, N).sum(0), y)
            else:
                close(ops.linear_normed(h, w, epi, plan(tile)),
                      R.silu_mul(y.to(BF)) if epi == "silu_mul" else y)


def test_m8_is_the_bf16_gemm_on_the_dequantised_weight(gpu):
    torch.manual_seed(8)
    w, _ = w4_weight(256, 1024, gpu, seed=4)
    x = rnd(8, 1024, dev=gpu)
    want = ops.linear(x, w.dequantize(BF).contiguous())
    assert torch.equal(ops.linear(x, w).view(torch.int16), want.view(torch.int16))


CFG = get_config("llama-tiny128", 2)
IDS = [5, 17, 99, 3, 250, 7, 8, 1000, 42, 11, 600, 3, 3, 9]


def _run(device, params, prompts, monkeypatch, graphs):
    logits = []
    real = TransformerLM.sample

    def spy(self, lg, b, generator=None):
        logits.append(lg.float().cpu())
        return real(self, lg, b, generator=generator)
    if not graphs:                     # (no host copy inside a graph capture)
        monkeypatch.setattr(TransformerLM, "sample", spy)
    eng = LLMEngine(CFG, device=device, params=params, max_batch=8, max_model_len=64,
                    num_blocks=64, use_graphs=graphs, lookahead=False)
    assert eng.stats()["weight_dtype"] == "w4"
    sp = SamplingParams(max_new_tokens=6, temperature=0.0, ignore_eos=True)
    toks = [o.output_ids for o in eng.generate(prompts, sp)]
    monkeypatch.setattr(TransformerLM, "sample", real)
    return toks, logits


@pytest.mark.parametrize("batch", [1, 3, 8])
def test_engine_against_the_cpu_reference(gpu, batch, monkeypatch):
    """Batch 1 (the deferred-norm W4 GEMV chain), 3 (W4 GEMVs with split-K reduces) and 8
    (dequantise, then the bf16 GEMMs), eager and graph-captured, against the CPU reference run
    of the same quantised parameters: greedy tokens equal up to a near tie (the logits agree
    until the first flipped token, as tests/test_fp8_weights_gpu.py has it)."""
    monkeypatch.setenv("DLI_GEMM_AUTOTUNE", "0")
    G.clear_plans()
    shapes = stage_param_shapes(CFG, 0, CFG.num_layers, True, True)
    params = quantize_params(CFG, random_init(shapes, "cpu", BF, seed=11, std=0.05), "w4")
    prompts = [IDS[i:i + 4 + i] for i in range(batch)]
    t_ref, l_ref = _run("cpu", params, prompts, monkeypatch, False)
    t_gpu, l_gpu = _run("cuda", params, prompts, monkeypatch, False)
    assert _run("cuda", params, prompts, monkeypatch, True)[0] == t_gpu
    assert len(l_ref) == len(l_gpu) >= 6 and all(len(t) == 6 for t in t_gpu)
    for i, (a, b) in enumerate(zip(l_gpu, l_ref)):
        err = (a - b).abs().max().item()
        assert err < 0.05 * b.abs().max().item() + 0.02, (i, err)
        if [t[:i + 1] for t in t_gpu] != [t[:i + 1] for t in t_ref]:
            break                      # a near tie flipped a token: later steps see other inputs
    else:
        assert t_gpu == t_ref
