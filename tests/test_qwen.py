"""Qwen3 (per-head q/k RMSNorm before RoPE) and Qwen2 / 2.5 (QKV bias) on the CPU path: the
reference ``rope_and_cache`` against a brute-force fp64 computation, the config / HF import,
the weight shapes, and the model and engine against HF transformers' eager
``Qwen3ForCausalLM`` / ``Qwen2ForCausalLM`` in fp32."""
import dataclasses
import json
import math

import pytest
import torch

from distributed_llm_inferencing_amd.engine import SamplingParams
from distributed_llm_inferencing_amd.engine.llm_engine import LLMEngine
from distributed_llm_inferencing_amd.models import ModelConfig, get_config
from distributed_llm_inferencing_amd.models import weights as W
from distributed_llm_inferencing_amd.models.hf import config_from_hf, load_hf_dir
from distributed_llm_inferencing_amd.models.weights import from_hf_state_dict
from distributed_llm_inferencing_amd.ops import reference as R

from hf_helpers import our_last_logits

PROMPT60 = [(7 * i + 3) % 1024 for i in range(60)]


# ------------------------------------------------------------------------------ reference op
def _brute(qkv, pos, slots, cs, hq, hkv, hd, bs, nblk, bias, qk_norm):
    """fp64, element by element: bias, per-head RMSNorm of q and k, rotate-half RoPE, and the
    cache rows of the tokens whose slot is not -1."""
    T = qkv.shape[0]
    half = hd // 2
    x = qkv.double().clone()
    if bias is not None:
        x = x + bias.double()
    out = x.clone()
    kc = torch.zeros(nblk, hkv, bs, hd, dtype=torch.float64)
    vc = torch.zeros(nblk, hkv, bs, hd, dtype=torch.float64)
    for t in range(T):
        for h in range(hq + 2 * hkv):
            v = x[t, h * hd:(h + 1) * hd].clone()
            if h < hq + hkv:
                if qk_norm is not None:
                    w = (qk_norm[0] if h < hq else qk_norm[1]).double()
                    v = v / math.sqrt(float((v * v).sum()) / hd + qk_norm[2]) * w
                r = torch.empty_like(v)
                for d in range(half):
                    co, si = float(cs[pos[t], d]), float(cs[pos[t], half + d])
                    r[d] = v[d] * co - v[half + d] * si
                    r[half + d] = v[half + d] * co + v[d] * si
                v = r
            out[t, h * hd:(h + 1) * hd] = v
            s = int(slots[t])
            if s >= 0 and h >= hq:
                dst = kc if h < hq + hkv else vc
                dst[s // bs, (h - hq) % hkv, s % bs] = v
    return out, kc, vc


@pytest.mark.parametrize("mode", ["norm", "bias", "both"])
@pytest.mark.parametrize("hq,hkv,hd", [(4, 2, 64), (3, 1, 128)])
def test_reference_rope_and_cache_bias_and_qk_norm(hq, hkv, hd, mode):
    g = torch.Generator().manual_seed(hd + len(mode))
    T, bs, nblk = 5, 4, 3
    n = (hq + 2 * hkv) * hd
    qkv = torch.randn(T, n, generator=g)
    pos = torch.tensor([0, 3, 17, 4, 9], dtype=torch.int32)
    slots = torch.tensor([5, 0, -1, 11, 6], dtype=torch.int32)
    cs = R.rope_cos_sin(32, hd, 10000.0)
    bias = torch.randn(n, generator=g) if mode != "norm" else None
    qkn = ((1 + 0.5 * torch.randn(hd, generator=g), 1 + 0.5 * torch.randn(hd, generator=g), 1e-6)
           if mode != "bias" else None)
    ref, kc_r, vc_r = _brute(qkv, pos, slots, cs, hq, hkv, hd, bs, nblk, bias, qkn)
    kc, vc = torch.zeros(nblk, hkv, bs, hd), torch.zeros(nblk, hkv, bs, hd)
    mine = qkv.clone()
    q, k, v = R.rope_and_cache(mine, pos, slots, cs, kc, vc, hq, hkv, hd, bias=bias, qk_norm=qkn)
    assert torch.allclose(mine.double(), ref, atol=1e-5, rtol=1e-5)
    assert torch.allclose(kc.double(), kc_r, atol=1e-5, rtol=1e-5)
    assert torch.allclose(vc.double(), vc_r, atol=1e-5, rtol=1e-5)
    assert q.data_ptr() == mine.data_ptr() and k.shape == (T, hkv, hd)     # views, in place
    # the token with slot -1 wrote nothing: 4 rows per cache and head
    assert int((kc.abs().sum(-1) > 0).sum()) == 4 * hkv


def test_reference_rope_and_cache_none_is_unchanged():
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(3, 8 * 64, generator=g).to(torch.bfloat16)
    pos = torch.tensor([0, 1, 2], dtype=torch.int32)
    slots = torch.tensor([0, 1, 2], dtype=torch.int32)
    cs = R.rope_cos_sin(8, 64, 10000.0)
    a, b = qkv.clone(), qkv.clone()
    ka, va, kb, vb = (torch.zeros(1, 2, 4, 64, dtype=torch.bfloat16) for _ in range(4))
    R.rope_and_cache(a, pos, slots, cs, ka, va, 4, 2, 64)
    R.rope_and_cache(b, pos, slots, cs, kb, vb, 4, 2, 64, bias=None, qk_norm=None)
    assert torch.equal(a, b) and torch.equal(ka, kb) and torch.equal(va, vb)


# ------------------------------------------------------------------------------ config / import
QWEN3_JSON = {
    "model_type": "qwen3", "hidden_size": 1024, "num_attention_heads": 16,
    "num_key_value_heads": 8, "head_dim": 128, "num_hidden_layers": 28,
    "intermediate_size": 3072, "vocab_size": 151936, "max_position_embeddings": 40960,
    "rope_theta": 1000000, "rms_norm_eps": 1e-6, "attention_bias": False,
    "tie_word_embeddings": True, "sliding_window": None, "use_sliding_window": False,
    "max_window_layers": 28, "bos_token_id": 151643, "eos_token_id": 151645}

QWEN2_JSON = {
    "model_type": "qwen2", "hidden_size": 3584, "num_attention_heads": 28,
    "num_key_value_heads": 4, "num_hidden_layers": 28, "intermediate_size": 18944,
    "vocab_size": 152064, "max_position_embeddings": 131072, "rope_theta": 1000000.0,
    "rms_norm_eps": 1e-6, "tie_word_embeddings": False, "sliding_window": 131072,
    "use_sliding_window": False, "max_window_layers": 28, "bos_token_id": 151643,
    "eos_token_id": 151643}


def test_config_from_hf_qwen3_and_qwen2():
    c = config_from_hf(QWEN3_JSON, "q3")
    assert c.arch == "llama" and c.qk_norm and not c.qkv_bias and c.tie_embeddings
    assert (c.head_dim, c.q_size, c.hidden_size, c.qkv_size) == (128, 2048, 1024, 4096)
    assert (c.norm_eps, c.rope_theta, c.eos_token_id) == (1e-6, 1e6, 151645)
    assert config_from_hf(dict(QWEN3_JSON, attention_bias=True), "q3").qkv_bias
    c2 = config_from_hf(QWEN2_JSON, "q2")
    assert c2.qkv_bias and not c2.qk_norm and c2.head_dim == 128 and c2.q_size == 3584
    assert dataclasses.replace(c2, name="qwen2.5-7b") == get_config("qwen2.5-7b")
    for mt in ("llama", "mistral"):
        c = config_from_hf(dict(QWEN2_JSON, model_type=mt, sliding_window=None), "x")
        assert not c.qk_norm and not c.qkv_bias
    with pytest.raises(ValueError, match="qwen2, qwen3"):
        config_from_hf({"model_type": "phi3"}, "x")


@pytest.mark.parametrize("opt_in", [False, True])
def test_config_from_hf_qwen_window_value_is_not_a_window(opt_in):
    """Both families ship a sliding_window value with use_sliding_window false: no window, and
    the context is not capped at it either."""
    for base in (QWEN3_JSON, QWEN2_JSON):
        c = config_from_hf(dict(base, sliding_window=4096), "q", sliding_window=opt_in)
        assert (c.sliding_window, c.max_position) == (0, base["max_position_embeddings"])
        with pytest.raises(ValueError, match="use_sliding_window"):
            config_from_hf(dict(base, sliding_window=4096, use_sliding_window=True), "q",
                           sliding_window=opt_in)


def test_config_fields_round_trip_and_registry():
    c = config_from_hf(dict(QWEN3_JSON, attention_bias=True), "q3")
    d = json.loads(json.dumps(c.to_dict()))
    assert d["qk_norm"] is True and d["qkv_bias"] is True
    assert ModelConfig.from_dict(d) == c
    d.pop("qk_norm"), d.pop("qkv_bias")      # a shard directory written before the fields
    old = ModelConfig.from_dict(d)
    assert not old.qk_norm and not old.qkv_bias
    q3 = get_config("Qwen/Qwen3-8B")
    assert (q3.name, q3.qk_norm, q3.qkv_bias) == ("qwen3-8b", True, False)
    assert (q3.hidden_size, q3.num_layers, q3.num_heads, q3.num_kv_heads, q3.head_dim,
            q3.intermediate_size, q3.vocab_size, q3.max_position, q3.rope_theta, q3.norm_eps,
            q3.bos_token_id, q3.eos_token_id) == (4096, 36, 32, 8, 128, 12288, 151936, 40960,
                                                  1e6, 1e-6, 151643, 151645)
    for alias in ("Qwen/Qwen2.5-7B", "Qwen/Qwen2.5-7B-Instruct"):
        assert get_config(alias).name == "qwen2.5-7b" and get_config(alias).qkv_bias
    assert get_config("qwen3-tiny") == dataclasses.replace(get_config("llama-tiny"),
                                                           name="qwen3-tiny", qk_norm=True)
    assert get_config("qwen2-tiny128") == dataclasses.replace(
        get_config("llama-tiny128"), name="qwen2-tiny128", qkv_bias=True)
    t = get_config("qwen3-tiny128")
    assert (t.hidden_size, t.q_size, t.head_dim, t.tie_embeddings, t.qk_norm) == (
        256, 512, 128, True, True)
    assert not get_config("llama3-8b").qk_norm and not get_config("llama3-8b").qkv_bias


# ------------------------------------------------------------------------------ weights
@pytest.mark.parametrize("name", ["qwen3-tiny128", "qwen2-tiny128", "qwen3-8b", "qwen2.5-7b"])
def test_param_shapes_and_counts(name):
    cfg = get_config(name)
    ls = W.layer_param_shapes(cfg, 1)
    assert ("layers.1.q_norm" in ls) == cfg.qk_norm == ("layers.1.k_norm" in ls)
    assert ("layers.1.bqkv" in ls) == cfg.qkv_bias
    if cfg.qk_norm:
        assert ls["layers.1.q_norm"] == ls["layers.1.k_norm"] == (cfg.head_dim,)
    if cfg.qkv_bias:
        assert ls["layers.1.bqkv"] == (cfg.qkv_size,)
    assert ls["layers.1.wo"] == (cfg.hidden_size, cfg.q_size)
    assert cfg.layer_param_count() == sum(math.prod(s) for s in ls.values())
    base = dataclasses.replace(cfg, qk_norm=False, qkv_bias=False)
    assert cfg.layer_param_count() > base.layer_param_count()


def test_stage_param_shapes_two_stage_split():
    for name, new in (("qwen3-tiny128", ("q_norm", "k_norm")), ("qwen2-tiny128", ("bqkv",))):
        cfg = get_config(name)
        s0 = W.stage_param_shapes(cfg, 0, 2, True, False)
        s1 = W.stage_param_shapes(cfg, 2, 4, False, True)
        for i in range(4):
            for t in new:
                k = f"layers.{i}.{t}"
                assert (k in s0) == (i < 2) and (k in s1) == (i >= 2), k
        assert not any(k.endswith(("q_norm", "k_norm", "bqkv")) for k in
                       W.stage_param_shapes(get_config("llama-tiny128"), 0, 4, True, True))
        p = W.random_init(s0, "cpu", torch.float32, seed=1)
        for t in new:                              # norms start at 1, the bias at 0
            want = 0.0 if t == "bqkv" else 1.0
            assert torch.all(p[f"layers.0.{t}"] == want)


def test_tensor_parallel_slices_bias_with_the_heads():
    from distributed_llm_inferencing_amd.parallel.tensor import shard_param
    cfg = get_config("qwen2-tiny128")                        # 4 q heads, 2 kv heads, hd 128
    hd = cfg.head_dim
    b = torch.arange(cfg.qkv_size, dtype=torch.float32)
    w = b[:, None].repeat(1, 2)
    for rank in range(2):
        sb = shard_param("layers.0.bqkv", b, cfg, rank, 2)
        sw = shard_param("layers.0.wqkv", w, cfg, rank, 2)
        assert sb.shape == (cfg.qkv_size // 2,) and torch.equal(sb, sw[:, 0])
        assert sb[0] == rank * 2 * hd and sb[2 * hd] == (4 + rank) * hd
    n = torch.ones(hd)
    q3 = get_config("qwen3-tiny128")
    assert shard_param("layers.0.q_norm", n, q3, 1, 2) is n              # replicated


# ------------------------------------------------------------------------------ HF parity
def hf_qwen(cfg, seed=0):
    """The eager HF twin (fp32) of a Qwen tiny config: random weights, q/k norm weights that are
    not all ones and biases that are not zero."""
    import transformers as tf
    torch.manual_seed(seed)
    kw = dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size,
              intermediate_size=cfg.intermediate_size, num_hidden_layers=cfg.num_layers,
              num_attention_heads=cfg.num_heads, num_key_value_heads=cfg.num_kv_heads,
              rope_theta=cfg.rope_theta, rms_norm_eps=cfg.norm_eps,
              max_position_embeddings=cfg.max_position, bos_token_id=cfg.bos_token_id,
              eos_token_id=cfg.eos_token_id, tie_word_embeddings=cfg.tie_embeddings,
              use_sliding_window=False, attn_implementation="eager")
    if cfg.qk_norm:
        hm = tf.Qwen3ForCausalLM(tf.Qwen3Config(head_dim=cfg.head_dim,
                                                attention_bias=cfg.qkv_bias, **kw))
    else:
        assert cfg.head_dim * cfg.num_heads == cfg.hidden_size
        hm = tf.Qwen2ForCausalLM(tf.Qwen2Config(**kw))
    hm = hm.float().eval()
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for n, p in hm.named_parameters():
            if n.endswith(("q_norm.weight", "k_norm.weight")):
                p.copy_(1 + 0.3 * torch.randn(p.shape, generator=g))
            elif n.endswith(("q_proj.bias", "k_proj.bias", "v_proj.bias")):
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
    return hm


TWINS = ["qwen3-tiny128", "qwen3-tiny", "qwen2-tiny128"]


@pytest.fixture(scope="module", params=TWINS)
def twin(request):
    cfg = get_config(request.param)
    hm = hf_qwen(cfg)
    return cfg, hm, from_hf_state_dict(cfg, hm.state_dict(), dtype=torch.float32)


def test_twin_exercises_the_new_tensors(twin):
    cfg, hm, params = twin
    assert hm.config._attn_implementation == "eager"
    if cfg.qk_norm:
        assert type(hm).__name__ == "Qwen3ForCausalLM"
        assert not torch.allclose(params["layers.0.q_norm"], torch.ones(cfg.head_dim))
        assert not torch.equal(params["layers.0.q_norm"], params["layers.0.k_norm"])
    if cfg.qkv_bias:
        assert type(hm).__name__ == "Qwen2ForCausalLM"
        assert params["layers.1.bqkv"].shape == (cfg.qkv_size,)
        assert params["layers.1.bqkv"].abs().min() > 0
    assert set(params) == set(W.stage_param_shapes(cfg, 0, cfg.num_layers, True, True))


def test_logits_match_hf(twin):
    cfg, hm, params = twin
    with torch.no_grad():
        ref = hm(torch.tensor([PROMPT60])).logits[0, -1]
    ours = our_last_logits(cfg, params, PROMPT60)
    assert torch.allclose(ours, ref, atol=2e-4, rtol=1e-3), (ours - ref).abs().max()
    # the new tensors matter: the same weights as a plain Llama layer are off
    plain = our_last_logits(dataclasses.replace(cfg, qk_norm=False, qkv_bias=False), params,
                            PROMPT60)
    assert not torch.allclose(plain, ref, atol=2e-4, rtol=1e-3)


@pytest.mark.parametrize("chunk", [16384, 4])
def test_greedy_generation_matches_hf(twin, chunk):
    """Greedy decode token for token with HF ``generate``, with whole-prompt prefill and with
    4-token prefill chunks (paged prefill over the cache the earlier chunks wrote)."""
    cfg, hm, params = twin
    eng = LLMEngine(cfg, device="cpu", dtype=torch.float32, params=params, max_batch=4,
                    max_model_len=64, num_blocks=16, block_size=16, max_prefill_tokens=chunk)
    prompts = [PROMPT60[:6], PROMPT60[10:30], PROMPT60[21:34]]
    outs = eng.generate(prompts, SamplingParams(max_length=40, do_sample=False, ignore_eos=True))
    for p, o in zip(prompts, outs):
        with torch.no_grad():
            ref = hm.generate(torch.tensor([p]), max_length=40, do_sample=False,
                              eos_token_id=None, pad_token_id=0)[0].tolist()
        assert o.all_ids == ref, (len(p), o.all_ids, ref)


def test_load_hf_dir_round_trip(twin, tmp_path):
    cfg, hm, _ = twin
    hm.save_pretrained(str(tmp_path / "ck"), safe_serialization=True)
    c2, params = load_hf_dir(tmp_path / "ck", dtype=torch.float32, name=cfg.name)
    assert c2 == cfg
    with torch.no_grad():
        ref = hm(torch.tensor([PROMPT60])).logits[0, -1]
    ours = our_last_logits(c2, params, PROMPT60)
    assert torch.allclose(ours, ref, atol=2e-4, rtol=1e-3), (ours - ref).abs().max()
