"""The FP8 LDS tiles 72 / 73 (``dli_gemm_fp8_tiles``) at 64 < M <= 512 against the fp32 reference
``R.linear(x, R.dequantize_weight(q, s, torch.float32), out_dtype=torch.float32)``.

Two cases the tiles' specification lists cannot exist. SiLU*up at N = 272: a gate/up weight has
N % 32 == 0 and the launcher must refuse the call; that refusal is asserted. The fall-back at
K = 1040 and M = 128: no bf16 tile takes K % 64 at M > 4, so that K has no dequantise path
either; K = 1088 (a multiple of 64, not of 128) stands in for it."""
import pytest
import torch

from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.ops import gemm as G
from distributed_llm_inferencing_amd.ops import reference as R
from distributed_llm_inferencing_amd.engine import SamplingParams
from distributed_llm_inferencing_amd.engine.llm_engine import LLMEngine
from distributed_llm_inferencing_amd.models.model import TransformerLM
from test_fp8_stream_gpu import (BF, CFG, F8, IDS, bf16_calls, clean_plans, close,  # noqa: F401
                                 fp8_params, fp8_weight, plan, rnd)

pytestmark = pytest.mark.gpu
TILES = sorted(G.FP8_TILE_TABLE)
WN, WK = 272, 1152         # 17 scale groups: a 16-row tail past both BN; 9 blocks: the rings wrap
ONE_HOT = (0, 15, 16, 63, 64, 127, 128, 1023, 1024, 1151)


def ref(x, q, s):
    return R.linear(x, R.dequantize_weight(q, s, torch.float32), out_dtype=torch.float32)


def witness_scales(K):
    """(2 i + 1) * 2^-(i % 7): distinct, exact wherever they multiply a multiple of 1/8 < 32."""
    i = torch.arange((WN // 16) * (K // 128), dtype=torch.float32)
    return ((2 * i + 1) * torch.exp2(-(i % 7))).view(WN // 16, K // 128)


@pytest.mark.parametrize("K,splits", [(WK, 1), (1024, 4)])
@pytest.mark.parametrize("M", [65, 128, 129])
@pytest.mark.parametrize("tile", TILES)
def test_scale_index_witness(gpu, tile, M, K, splits):
    """Weights all fp8 1.0, x one-hot at column k: y[m, n] = x[m, k] * s[n // 16, k // 128]
    exactly (under split-K the other slices add zeros)."""
    q, s = torch.ones(WN, K).to(F8), witness_scales(K)
    assert s.unique().numel() == s.numel()
    w = ops.Fp8Weight(q.to(gpu), s.to(gpu))
    xv = ((torch.arange(M, dtype=torch.float32) + 1) / 8).to(BF)
    for k in (k for k in ONE_HOT if k < K):
        x = torch.zeros(M, K, dtype=BF)
        x[:, k] = xv
        want = xv.float()[:, None] * s[:, k // 128].repeat_interleave(16)[None, :]
        if M == 65:
            assert torch.equal(want, ref(x, q, s))
        y = ops._gemm_native(x.to(gpu), w, "f32", plan=plan(tile, splits))
        assert torch.equal(y.cpu(), want), k


@pytest.mark.parametrize("M", [65, 128, 129])
@pytest.mark.parametrize("tile", TILES)
def test_k_pairing_witness(gpu, tile, M):
    """One fp8 1.0 per weight row, at k_n: y[m, n] = x[m, k_n] * s[n // 16, k_n // 128] exactly."""
    s, n = witness_scales(WK), torch.arange(WN)
    kn = (37 * n + 11) % WK
    q = torch.zeros(WN, WK)
    q[n, kn] = 1.0
    x = ((((7 * torch.arange(WK)[None, :] + 3 * torch.arange(M)[:, None]) % 31) - 15).float()
         / 8).to(BF)
    want = x.float()[:, kn] * s[n // 16, kn // 128][None, :]
    assert torch.equal(want, ref(x, q.to(F8), s)) and want.abs().max() > 0
    y = ops._gemm_native(x.to(gpu), ops.Fp8Weight(q.to(F8).to(gpu), s.to(gpu)), "f32",
                         plan=plan(tile))
    assert torch.equal(y.cpu(), want)


_cases = {}


def case(gpu, M, N, K):                  # operands and their fp32 product, once per shape
    if (M, N, K) not in _cases:
        torch.manual_seed(3)
        w, wf = fp8_weight(N, K, gpu, seed=N + K)
        x = rnd(M, K, dev=gpu)
        _cases[(M, N, K)] = (w, x, rnd(N, dev=gpu), R.linear(x, wf, out_dtype=torch.float32))
    return _cases[(M, N, K)]


# K = 256: two blocks, shorter than the 3-stage ring's prologue
@pytest.mark.parametrize("N,K", [(96, 1152), (272, 256)])
@pytest.mark.parametrize("M", [65, 128, 200])
@pytest.mark.parametrize("epi", ["none", "f32", "bias", "silu_mul"])
@pytest.mark.parametrize("tile", TILES)
def test_epilogues(gpu, tile, epi, M, N, K):
    w, x, b, y = case(gpu, M, N, K)
    if epi == "silu_mul" and N % 32:
        with pytest.raises(RuntimeError, match="dli_gemm_fp8_tiles"):
            ops._gemm_native(x, w, epi, plan=plan(tile))
        return
    want = R.silu_mul(y.to(BF)) if epi == "silu_mul" else y + b.float() if epi == "bias" else y
    out = ops._gemm_native(x, w, epi, bias=b if epi == "bias" else None, plan=plan(tile))
    assert out.dtype == (torch.float32 if epi == "f32" else BF)
    assert out.shape == (M, N // 2 if epi == "silu_mul" else N)
    close(out, want)


@pytest.mark.parametrize("M", [65, 129])
@pytest.mark.parametrize("splits", [2, 4, 8])
@pytest.mark.parametrize("tile", TILES)
def test_split_k(gpu, tile, splits, M, bf16_calls):
    """K = 1024 in slices of 512 / 256 / 128: reduced into C, and fp32 slabs for a fused consumer."""
    w, x, _, y = case(gpu, M, WN, 1024)
    close(ops._gemm_native(x, w, "none", plan=plan(tile, splits)), y)
    r0, nw = rnd(M, WN, dev=gpu), rnd(WN, dev=gpu)
    ref_out, ref_res = R.fused_add_rmsnorm(y.to(BF), r0, nw, 1e-5)
    res = r0.clone()
    close(ops.linear_add_rmsnorm(x, w, res, nw, 1e-5, plan=plan(tile, splits)), ref_out)
    close(res, ref_res)
    assert bf16_calls == []


@pytest.mark.parametrize("tile", TILES)
def test_routing(gpu, tile, bf16_calls, clean_plans):
    w, x, _, y = case(gpu, 128, WN, 1024)
    G.set_plan(128, WN, 1024, "none", plan(tile), wd="fp8")
    close(ops.linear(x, w), y)
    assert bf16_calls == []                       # the pinned tile: no dequantise pass
    w, x, _, y = case(gpu, 128, WN, 1088)         # K % 128: the dequantise path, once a call
    assert not w.tiles_ok(128, plan(tile))
    close(ops._gemm_native(x, w, "none", plan=plan(tile)), y)
    assert len(bf16_calls) == 1
    with pytest.raises(ValueError, match=str(tile)):
        ops._gemm_native(x, rnd(WN, 1088, dev=gpu), "none", plan=plan(tile))


@pytest.mark.parametrize("tile", TILES)
def test_model_decode_step_of_80_rows(gpu, tile, fp8_params, bf16_calls, clean_plans,
                                      monkeypatch):
    """Decode steps of 80 rows, the four projections on the tile: logits against a CPU engine on
    the fp32 reconstruction of the weights, and no dequantise pass in the layers."""
    monkeypatch.setenv("DLI_GEMM_AUTOTUNE", "0")
    B, D, F = 80, CFG.hidden_size, CFG.intermediate_size
    qkv = (CFG.num_heads + 2 * CFG.num_kv_heads) * CFG.head_dim
    for n, k, epi, splits in ((qkv, D, "splitk", 2), (D, D, "splitk", 1), (D, D, "none", 1),
                              (2 * F, D, "silu_mul", 1), (D, F, "splitk", 4)):
        G.set_plan(B, n, k, epi, plan(tile, splits), wd="fp8")
    real, real_sample = TransformerLM.forward_layers, TransformerLM.sample
    per_step, logits, toks = [], {}, {}

    def spy(self, x, b, kv_caches):
        n0 = len(bf16_calls)
        out = real(self, x, b, kv_caches)
        if not b.is_prefill and x.is_cuda and x.shape[0] == B:
            per_step.append(len(bf16_calls) - n0)
        return out

    def sample_spy(self, lg, b, generator=None):
        logits.setdefault(lg.device.type, []).append(lg.float().cpu())
        return real_sample(self, lg, b, generator=generator)
    monkeypatch.setattr(TransformerLM, "forward_layers", spy)
    monkeypatch.setattr(TransformerLM, "sample", sample_spy)
    prompts = [IDS[i % 8:i % 8 + 4 + i % 5] + [i + 1] for i in range(B)]
    deq = {k: R.dequantize_weight(v, fp8_params[k + "_scale"], torch.float32) if v.dtype == F8
           else v for k, v in fp8_params.items() if not k.endswith("_scale")}
    sp = SamplingParams(max_new_tokens=3, temperature=0.0, ignore_eos=True)
    for dev, params in (("cpu", deq), ("cuda", fp8_params)):
        eng = LLMEngine(CFG, device=dev, params=params, max_batch=B, max_model_len=64,
                        num_blocks=4 * B + 8, use_graphs=False, lookahead=False)
        toks[dev] = [o.output_ids for o in eng.generate(prompts, sp)]
    assert len(logits["cpu"]) == len(logits["cuda"]) >= 3
    for i, (a, b) in enumerate(zip(logits["cuda"], logits["cpu"])):
        err = (a - b).abs().max().item()
        assert a.shape == b.shape and err < 0.05 * b.abs().max().item() + 0.02, (i, err)
        if [t[:i + 1] for t in toks["cuda"]] != [t[:i + 1] for t in toks["cpu"]]:
            break                      # a near tie flipped a token: later steps see other inputs
    assert len(per_step) >= 2 and not any(per_step), per_step
