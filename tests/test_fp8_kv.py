"""FP8 (OCP e4m3fn) paged KV cache, CPU tier: the cache object and its sizing, the one
definition of the quantisation (``ops/reference.py`` ``quantize_kv``), the ops layer's checks,
and engines on the reference ops. ``three_step_logits`` (prefill -> paged chunk -> decode,
hand-built steps) is shared with the GPU tier (test_fp8_kv_gpu.py)."""
import numpy as np
import pytest
import torch

from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.engine import SamplingParams
from distributed_llm_inferencing_amd.engine.batch import DECODE, PREFILL, StepMeta, to_device
from distributed_llm_inferencing_amd.engine.kv_cache import (KVCache, auto_num_blocks,
                                                             blocks_for_budget, bytes_per_block)
from distributed_llm_inferencing_amd.engine.llm_engine import LLMEngine
from distributed_llm_inferencing_amd.models import TransformerLM, get_config
from distributed_llm_inferencing_amd.ops import reference as R

F8 = torch.float8_e4m3fn
MODELS = ["llama-tiny", "mistral-tiny128", "qwen3-tiny"]

# Max |logit difference| FP8 cache vs bf16 cache over the three steps of three_step_logits,
# measured on the CPU (reference ops, bf16 model, seed 0, scales 1): the paged chunk and the
# decode step read the cache, the plain prefill does not (difference exactly 0). The asserted
# bound is twice the measured value; a wrong scale or a missing clamp is off by far more.
MEASURED_FP8_VS_BF16 = {"llama-tiny": 0.0153, "mistral-tiny128": 0.0274, "qwen3-tiny": 0.0281}


# ------------------------------------------------------------------------------ cache object
def test_kvcache_fp8_holds_e4m3_bytes_of_the_same_shape():
    cfg = get_config("llama-tiny")
    a = KVCache(cfg, 2, 8, 16, "cpu")
    b = KVCache(cfg, 2, 8, 16, "cpu", kv_dtype="fp8", k_scale=0.5, v_scale=2.0)
    assert a.kv_dtype == "bf16" and a.k.dtype == torch.bfloat16
    assert b.kv_dtype == "fp8" and b.k.dtype == F8 and b.v.dtype == F8
    assert b.k.shape == a.k.shape and b.v.shape == a.v.shape
    assert 2 * b.nbytes == a.nbytes and b.capacity_tokens == a.capacity_tokens
    assert int(b.k.view(torch.uint8).max()) == 0                   # zero bytes = 0.0
    layers = b.layers()
    assert len(layers) == 2 and layers[0][0].dtype == F8
    assert (layers.k_scale, layers.v_scale) == (0.5, 2.0)
    assert (a.layers().k_scale, a.layers().v_scale) == (1.0, 1.0)


def test_pool_sizing_takes_the_element_size():
    cfg = get_config("llama-tiny")
    assert bytes_per_block(cfg, 4, 16, 1) * 2 == bytes_per_block(cfg, 4, 16)
    budget = 1000 * bytes_per_block(cfg, 4, 16) + 7
    assert blocks_for_budget(cfg, 4, 16, budget) == 1000
    assert blocks_for_budget(cfg, 4, 16, budget, dtype_bytes=1) == 2000
    n2 = auto_num_blocks(cfg, 64, 16, "cpu", cap_tokens=1 << 30)
    n1 = auto_num_blocks(cfg, 64, 16, "cpu", cap_tokens=1 << 30, dtype_bytes=1)
    assert n1 == 2 * n2


def test_kvcache_rejects_unknown_dtype_and_bad_scales():
    cfg = get_config("llama-tiny")
    with pytest.raises(ValueError):
        KVCache(cfg, 1, 4, 16, "cpu", kv_dtype="int8")
    with pytest.raises(ValueError):
        KVCache(cfg, 1, 4, 16, "cpu", kv_dtype="fp8", k_scale=0.0)
    with pytest.raises(ValueError):
        KVCache(cfg, 1, 4, 16, "cpu", kv_dtype="bf16", v_scale=2.0)


def test_engine_kv_dtype_argument_and_environment(monkeypatch):
    monkeypatch.delenv("KV_CACHE_DTYPE", raising=False)
    kw = dict(device="cpu", max_batch=4, max_model_len=64, num_blocks=16)
    eng = LLMEngine("llama-tiny", kv_dtype="fp8", **kw)
    assert eng.kv.k.dtype == F8 and eng.memory_report()["kv_cache_dtype"] == "fp8"
    out = eng.generate([[3, 4, 5, 6]], SamplingParams(max_length=12, do_sample=False,
                                                     ignore_eos=True))
    assert len(out[0].output_ids) == 8
    assert LLMEngine("llama-tiny", **kw).memory_report()["kv_cache_dtype"] == "bf16"
    monkeypatch.setenv("KV_CACHE_DTYPE", "fp8")
    assert LLMEngine("llama-tiny", **kw).kv.k.dtype == F8
    assert LLMEngine("llama-tiny", kv_dtype="bf16", **kw).kv.k.dtype == torch.bfloat16
    monkeypatch.setenv("KV_CACHE_DTYPE", "fp4")
    with pytest.raises(ValueError):
        LLMEngine("llama-tiny", **kw)
    with pytest.raises(ValueError):
        LLMEngine("llama-tiny", kv_dtype="e5m2", **kw)


def test_settings_and_worker_state_carry_the_dtype(monkeypatch, tmp_path):
    from distributed_llm_inferencing_amd.config import get_settings
    from distributed_llm_inferencing_amd.worker.server import WorkerState
    monkeypatch.setenv("MODEL_CACHE_DIR", str(tmp_path / "cache"))    # WorkerState creates it
    monkeypatch.delenv("KV_CACHE_DTYPE", raising=False)
    s = get_settings()
    assert s.kv_cache_dtype == "bf16"
    assert WorkerState(s, "cpu").engine_kwargs["kv_dtype"] == "bf16"
    monkeypatch.setenv("KV_CACHE_DTYPE", "fp8")
    s = get_settings()
    assert s.kv_cache_dtype == "fp8"
    assert WorkerState(s, "cpu").engine_kwargs["kv_dtype"] == "fp8"
    assert WorkerState(s, "cpu", {"kv_dtype": "bf16"}).engine_kwargs["kv_dtype"] == "bf16"
    monkeypatch.setenv("KV_CACHE_DTYPE", "fp16")
    with pytest.raises(ValueError):
        get_settings()


def test_cli_node_commands_pass_kv_dtype():
    from distributed_llm_inferencing_amd.cli import node_commands
    cmd, _ = node_commands(1, kv_dtype="fp8")[0]
    assert cmd[cmd.index("--kv-dtype") + 1] == "fp8"
    assert "--kv-dtype" not in node_commands(1)[0][0]


# ------------------------------------------------------------------------------ quantize_kv
def test_quantize_kv_saturates_never_nan():
    x = torch.tensor([449.0, 1e4, -1e4, 460.0, 500.0, 448.0, -448.0, float("inf")])
    q = R.quantize_kv(x).float()
    assert not q.isnan().any()
    assert q.tolist() == [448.0, 448.0, -448.0, 448.0, 448.0, 448.0, -448.0, 448.0]
    assert torch.tensor(500.0).to(F8).float().isnan()        # what the clamp is for
    assert R.quantize_kv(torch.tensor([1e4, -1e4]), 8.0).float().tolist() == [448.0, -448.0]
    assert R.quantize_kv(torch.tensor([1e4]), 32.0).float().tolist() == [320.0]


def test_quantize_kv_subnormal_rounding():
    """e4m3 subnormals are multiples of 2^-9: ties go to the even multiple."""
    u = 2.0 ** -9
    x = torch.tensor([u, u / 2, 1.5 * u, 2.5 * u, 0.75 * u, 0.49 * u, 7 * u, 7.5 * u, -u / 2])
    want = [u, 0.0, 2 * u, 2 * u, u, 0.0, 7 * u, 8 * u, -0.0]
    q = R.quantize_kv(x)
    assert q.float().tolist() == want
    assert q.view(torch.uint8).tolist() == [1, 0, 2, 2, 1, 0, 7, 8, 0x80]


@pytest.mark.parametrize("scale", [0.5, 2.0])
def test_quantize_kv_scale_round_trips_representable_values(scale):
    codes = torch.arange(256, dtype=torch.uint8)
    codes = codes[(codes & 0x7F) != 0x7F]                       # every finite e4m3fn value
    x = codes.view(F8).float()
    q = R.quantize_kv(x * scale, scale)
    assert torch.equal(q.view(torch.uint8), codes)
    assert torch.equal(R.dequantize_kv(q, scale), x * scale)
    assert R.inv_scale(scale) == 1.0 / scale


def test_write_and_gather_apply_the_scales():
    torch.manual_seed(0)
    hkv, hd, bs = 2, 16, 4
    k = (torch.randn(6, hkv, hd) * 3).bfloat16()
    v = (torch.randn(6, hkv, hd) * 300).bfloat16()             # some |v| / 0.5 > 448: clamped
    kc = torch.zeros(5, hkv, bs, hd, dtype=F8)
    vc = torch.zeros(5, hkv, bs, hd, dtype=F8)
    slots = torch.tensor([4, 5, -1, 17, 18, 19], dtype=torch.int32)
    R.write_kv(k, v, slots, kc, vc, k_scale=2.0, v_scale=0.5)
    table = torch.tensor([1, 4, 0], dtype=torch.int32)          # slots 4.. = block 1, 16.. = 4
    kk, vv = R.gather_kv(kc, vc, table, 8, k_scale=2.0, v_scale=0.5)
    assert torch.equal(kk[0], R.quantize_kv(k[0], 2.0).float() * 2.0)
    assert torch.equal(vv[1], R.quantize_kv(v[1], 0.5).float() * 0.5)
    assert torch.equal(kk[5], R.quantize_kv(k[3], 2.0).float() * 2.0)
    assert vv.abs().max() <= 224.0 and (v.float().abs() > 224).any()
    assert int(kc[0].view(torch.uint8).max()) == 0 and int(kc[1, :, 2:].view(torch.uint8).max()) == 0


# ------------------------------------------------------------------------------ ops validation
def _ops_args(kdt, vdt=None):
    hq, hkv, hd, bs = 4, 2, 16, 4
    qkv = torch.randn(3, (hq + 2 * hkv) * hd).bfloat16()
    kc = torch.zeros(4, hkv, bs, hd, dtype=kdt)
    vc = torch.zeros(4, hkv, bs, hd, dtype=vdt or kdt)
    pos = torch.arange(3, dtype=torch.int32)
    slots = torch.tensor([0, 1, 2], dtype=torch.int32)
    cs = R.rope_cos_sin(16, hd, 10000.0)
    return qkv, kc, vc, pos, slots, cs, (hq, hkv, hd)


def _every_op(kdt, vdt=None, **scales):
    qkv, kc, vc, pos, slots, cs, (hq, hkv, hd) = _ops_args(kdt, vdt)
    tables = torch.zeros(3, 1, dtype=torch.int32)
    ctx = torch.tensor([1, 2, 3], dtype=torch.int32)
    cu = torch.tensor([0, 3], dtype=torch.int32)
    w = torch.randn((hq + 2 * hkv) * hd, 8).bfloat16()
    x = torch.randn(3, 8).bfloat16()
    return [
        lambda: ops.rope_and_cache(qkv, pos, slots, cs, kc, vc, hq, hkv, hd, **scales),
        lambda: ops.linear_rope_cache(x, w, pos, slots, cs, kc, vc, hq, hkv, hd, **scales),
        lambda: ops.decode_attention(qkv, kc, vc, tables, ctx, 3, hq, hkv, hd, 0.25, **scales),
        lambda: ops.prefill_attention_paged(qkv, cu, 3, ctx[2:], tables[:1], kc, vc, hq, hkv,
                                            hd, 0.25, **scales),
    ]


@pytest.mark.parametrize("case", [
    dict(kdt=torch.uint8), dict(kdt=torch.int8), dict(kdt=torch.float8_e5m2),
    dict(kdt=F8, vdt=torch.bfloat16), dict(kdt=torch.bfloat16, vdt=F8),
    dict(kdt=F8, k_scale=0.0), dict(kdt=F8, v_scale=-1.0), dict(kdt=F8, k_scale=float("nan")),
    dict(kdt=torch.bfloat16, k_scale=0.5), dict(kdt=torch.bfloat16, v_scale=2.0)])
def test_ops_reject_bad_cache_dtype_or_scale(case):
    for call in _every_op(**case):
        with pytest.raises(ValueError):
            call()


def test_ops_accept_fp8_and_bf16_caches():
    for call in _every_op(F8, k_scale=0.5, v_scale=2.0) + _every_op(torch.bfloat16):
        call()
    assert ops.kv_cache_is_fp8(torch.zeros(1, dtype=F8), torch.zeros(1, dtype=F8))
    with pytest.raises(ValueError):           # what the HIP kernels read: bf16 or e4m3fn only
        ops.kv_cache_is_fp8(torch.zeros(1), torch.zeros(1), native=True)
    assert not ops.kv_cache_is_fp8(torch.zeros(1), torch.zeros(1), native=False)


def test_linear_rope_attention_declines_an_fp8_cache():
    """CPU tensors never take the fused kernel; the FP8 rule itself is exercised on the GPU."""
    qkv, kc, vc, pos, slots, cs, (hq, hkv, hd) = _ops_args(F8)
    assert ops.linear_rope_attention(qkv, qkv, pos, slots, cs, kc, vc, None, None, 1, hq, hkv,
                                     hd, 0.25) is None


# ------------------------------------------------------------------------------ model, engine
IDS = [(7 * i * i + 3 * i + 11) % 250 + 2 for i in range(40)]


def _meta(kind, ids, pos0, slots, ctx, tables):
    n = len(ids)
    return StepMeta(kind=kind, seq_ids=[0], input_ids=np.array(ids, np.int32),
                    positions=np.arange(pos0, pos0 + n, dtype=np.int32),
                    slot_mapping=np.array(slots, np.int32), seq_lens=np.array([n], np.int32),
                    context_lens=np.array([ctx], np.int32), block_tables=tables,
                    temperature=np.zeros(1, np.float32), top_k=np.ones(1, np.int32),
                    top_p=np.ones(1, np.float32), seeds=np.zeros(1, np.int64))


def three_step_logits(name, device, kv_dtype, k_scale=1.0, v_scale=1.0, seed=0):
    """Last-token fp32 logits of: a 20-token prefill that writes the cache (plain attention
    over the qkv rows), a 12-token chunk over the paged cache (context 32), one decode step
    (context 33). Blocks are scattered; block size 16."""
    cfg = get_config(name)
    m = TransformerLM.random(cfg, device="cpu", dtype=torch.bfloat16, seed=seed).to(device)
    kv = KVCache(cfg, cfg.num_layers, 8, 16, device, torch.bfloat16, kv_dtype=kv_dtype,
                 k_scale=k_scale, v_scale=v_scale)
    layers = kv.layers()
    blocks = [5, 2, 6]
    slot = lambda t: blocks[t // 16] * 16 + t % 16              # noqa: E731
    tables = np.array([blocks], np.int32)
    steps = [_meta(PREFILL, IDS[:20], 0, [slot(t) for t in range(20)], 20,
                   np.zeros((1, 0), np.int32)),
             _meta(PREFILL, IDS[20:32], 20, [slot(t) for t in range(20, 32)], 32, tables),
             _meta(DECODE, IDS[32:33], 32, [slot(32)], 33, tables)]
    out = []
    for meta in steps:
        _, lg = m.forward(to_device(meta, device), layers, return_logits=True)
        out.append(lg[0].float().cpu())
    return out


_bf16_logits = {}


def bf16_three_step_logits(name):
    if name not in _bf16_logits:
        _bf16_logits[name] = three_step_logits(name, "cpu", "bf16")
    return _bf16_logits[name]


@pytest.mark.parametrize("name", MODELS)
def test_fp8_logits_stay_close_to_bf16_cache(name):
    ref = bf16_three_step_logits(name)
    got = three_step_logits(name, "cpu", "fp8")
    errs = [(a - b).abs().max().item() for a, b in zip(got, ref)]
    print(f"{name}: max |fp8 - bf16| per step {errs}, max |logit| "
          f"{max(r.abs().max().item() for r in ref):.3f}")
    assert errs[0] == 0.0                  # the plain prefill reads no cache
    assert max(errs[1:]) > 0.0             # the cache really is quantised
    assert max(errs) <= 2 * MEASURED_FP8_VS_BF16[name], errs


@pytest.mark.parametrize("name", MODELS[:1])
def test_fp8_logits_with_scales(name):
    """Power-of-two scales move no FP8 rounding point while nothing clamps or goes subnormal:
    logits equal those of scales (1, 1) up to the softmax scale's own rounding."""
    base = three_step_logits(name, "cpu", "fp8")
    got = three_step_logits(name, "cpu", "fp8", k_scale=0.5, v_scale=2.0)
    for a, b in zip(got, base):
        assert (a - b).abs().max().item() <= 2e-2


@pytest.mark.parametrize("name", MODELS)
def test_fp8_engine_generates_with_chunks_mixed_steps_and_preemption(name, monkeypatch):
    monkeypatch.delenv("KV_CACHE_DTYPE", raising=False)
    sp = SamplingParams(max_length=70, do_sample=False, ignore_eos=True)
    prompts = [list(range(20 + i, 20 + i + 40)) for i in range(5)]
    eng = LLMEngine(name, device="cpu", max_batch=8, max_model_len=128, max_prefill_tokens=24,
                    num_blocks=20, kv_dtype="fp8", mixed_steps=True)       # 320 tokens of KV
    n_pre = [0]
    orig = eng.scheduler._preempt

    def counted(mb):
        n_pre[0] += 1
        return orig(mb)
    eng.scheduler._preempt = counted
    rids = [eng.add_request(p, sp) for p in prompts[:2]]
    for _ in range(4):
        eng.step()
    rids += [eng.add_request(p, sp) for p in prompts[2:]]
    outs = {}
    while eng.has_work():
        for o in eng.step():
            outs[o.request_id] = o
    for o in eng.step():
        outs[o.request_id] = o
    assert all(len(outs[r].all_ids) == 70 for r in rids)
    vocab = get_config(name).vocab_size
    assert all(0 <= t < vocab for r in rids for t in outs[r].output_ids)
    assert eng.stats.prefill_steps > 5 and eng.stats.mixed_steps > 0 and n_pre[0] > 0
    assert eng.kv.k.dtype == F8 and int(eng.kv.k.view(torch.uint8).max()) > 0
