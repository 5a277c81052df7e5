"""Sliding-window attention (Mistral family) on the CPU path: the reference ops against a
brute-force softmax over the explicitly listed visible keys, the config / HF import, and the
model and engine against HF transformers' eager ``MistralForCausalLM`` in fp32.

The rule (``transformers.masking_utils.sliding_window_overlay``): the query at position q
sees key j iff q - W < j <= q, i.e. W keys including its own."""
import dataclasses
import json
import math

import pytest
import torch

from distributed_llm_inferencing_amd.engine import SamplingParams
from distributed_llm_inferencing_amd.engine.llm_engine import LLMEngine
from distributed_llm_inferencing_amd.models import ModelConfig, get_config
from distributed_llm_inferencing_amd.models.hf import config_from_hf, load_hf_dir
from distributed_llm_inferencing_amd.models.weights import from_hf_state_dict
from distributed_llm_inferencing_amd.ops import reference as R

from hf_helpers import our_last_logits

HQ, HKV, HD, BS = 4, 2, 16, 4
SCALE = 1 / math.sqrt(HD)
PROMPT60 = [(7 * i + 3) % 1024 for i in range(60)]


def _visible(qpos, window):
    lo = 0 if window <= 0 else max(0, qpos - window + 1)
    return list(range(lo, qpos + 1))


def _brute(q, k, v, qpos, window):
    """One query [Hq, hd] at position ``qpos`` over the keys k/v [n, Hkv, hd] it may see."""
    idx = _visible(qpos, window)
    rep = q.shape[0] // k.shape[1]
    out = torch.empty(q.shape, dtype=torch.float32)
    for h in range(q.shape[0]):
        kk, vv = k[idx, h // rep].float(), v[idx, h // rep].float()
        p = torch.softmax((kk @ q[h].float()) * SCALE, 0)
        out[h] = p @ vv
    return out


def _paged(ctxs, seed=0):
    """A scattered paged cache holding random K/V of the sequences; returns the caches, the
    block tables and the contiguous per-sequence K/V."""
    g = torch.Generator().manual_seed(seed)
    nblk = sum(-(-c // BS) for c in ctxs) + 2
    kc = torch.zeros(nblk, HKV, BS, HD)
    vc = torch.zeros(nblk, HKV, BS, HD)
    perm = torch.randperm(nblk, generator=g).tolist()
    maxb = max(-(-c // BS) for c in ctxs)
    tables, ks, vs, o = [], [], [], 0
    for c in ctxs:
        nb = -(-c // BS)
        blocks = perm[o:o + nb]
        o += nb
        tables.append(blocks + [0] * (maxb - nb))
        k, v = torch.randn(c, HKV, HD, generator=g), torch.randn(c, HKV, HD, generator=g)
        slots = torch.tensor([blocks[t // BS] * BS + t % BS for t in range(c)], dtype=torch.int32)
        R.write_kv(k, v, slots, kc, vc)
        ks.append(k)
        vs.append(v)
    return kc, vc, torch.tensor(tables, dtype=torch.int32), ks, vs


@pytest.mark.parametrize("window", [1, 3, 4, 5, 9, 40])
def test_reference_decode_window_matches_brute_force(window):
    ctxs = [1, 3, 4, 5, 9, 10, 23]
    kc, vc, tables, ks, vs = _paged(ctxs)
    q = torch.randn(len(ctxs), HQ, HD, generator=torch.Generator().manual_seed(1))
    out = R.decode_attention(q, kc, vc, tables, torch.tensor(ctxs, dtype=torch.int32), SCALE,
                             window=window)
    for b, c in enumerate(ctxs):
        assert _visible(c - 1, window) == list(range(max(0, c - window), c))
        ref = _brute(q[b], ks[b], vs[b], c - 1, window)
        assert torch.allclose(out[b], ref, atol=1e-5, rtol=1e-5), (b, c)


@pytest.mark.parametrize("window", [1, 3, 8, 40])
def test_reference_prefill_window_matches_brute_force(window):
    lens = [1, 5, 8, 9, 21]
    g = torch.Generator().manual_seed(2)
    T = sum(lens)
    q = torch.randn(T, HQ, HD, generator=g)
    k, v = torch.randn(T, HKV, HD, generator=g), torch.randn(T, HKV, HD, generator=g)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)
    out = R.prefill_attention(q, k, v, cu, SCALE, window=window)
    o = 0
    for n in lens:
        for t in range(n):
            ref = _brute(q[o + t], k[o:o + n], v[o:o + n], t, window)
            assert torch.allclose(out[o + t], ref, atol=1e-5, rtol=1e-5), (n, t)
        o += n


@pytest.mark.parametrize("window", [1, 4, 7, 40])
def test_reference_paged_chunk_window_matches_brute_force(window):
    chunks = [(23, 5), (9, 9), (10, 1), (17, 12)]           # (context, chunk length)
    ctxs = [c for c, _ in chunks]
    lens = [n for _, n in chunks]
    kc, vc, tables, ks, vs = _paged(ctxs, seed=3)
    T = sum(lens)
    q = torch.randn(T, HQ, HD, generator=torch.Generator().manual_seed(4))
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)
    out = R.prefill_attention_paged(q, kc, vc, cu, torch.tensor(ctxs, dtype=torch.int32), tables,
                                    SCALE, window=window)
    o = 0
    for i, (c, n) in enumerate(chunks):
        for t in range(n):
            ref = _brute(q[o + t], ks[i], vs[i], c - n + t, window)
            assert torch.allclose(out[o + t], ref, atol=1e-5, rtol=1e-5), (c, n, t)
        o += n


def test_reference_window_off_or_wide_equals_full_attention():
    """window = 0 and any window >= the context leave the results exactly as they were."""
    ctxs = [1, 6, 23]
    kc, vc, tables, ks, vs = _paged(ctxs, seed=5)
    g = torch.Generator().manual_seed(6)
    cl = torch.tensor(ctxs, dtype=torch.int32)
    q = torch.randn(len(ctxs), HQ, HD, generator=g)
    full = R.decode_attention(q, kc, vc, tables, cl, SCALE)
    for w in (0, 23, 24, 1000):
        assert torch.equal(R.decode_attention(q, kc, vc, tables, cl, SCALE, window=w), full)
    lens = [4, 23]
    T = sum(lens)
    qp = torch.randn(T, HQ, HD, generator=g)
    k, v = torch.randn(T, HKV, HD, generator=g), torch.randn(T, HKV, HD, generator=g)
    cu = torch.tensor([0, 4, 27], dtype=torch.int32)
    full = R.prefill_attention(qp, k, v, cu, SCALE)
    for w in (0, 23, 1000):
        assert torch.equal(R.prefill_attention(qp, k, v, cu, SCALE, window=w), full)
    assert not torch.equal(R.prefill_attention(qp, k, v, cu, SCALE, window=22), full)
    qc = torch.randn(5 + 3, HQ, HD, generator=g)
    cu2 = torch.tensor([0, 5, 8], dtype=torch.int32)
    c2, t2 = torch.tensor([6, 23], dtype=torch.int32), tables[1:]
    full = R.prefill_attention_paged(qc, kc, vc, cu2, c2, t2, SCALE)
    for w in (0, 23, 1000):
        assert torch.equal(R.prefill_attention_paged(qc, kc, vc, cu2, c2, t2, SCALE, window=w),
                           full)


# ------------------------------------------------------------------------------ config / import
MISTRAL_7B_JSON = {
    "model_type": "mistral", "hidden_size": 4096, "num_attention_heads": 32,
    "num_key_value_heads": 8, "num_hidden_layers": 32, "intermediate_size": 14336,
    "vocab_size": 32000, "max_position_embeddings": 32768, "rope_theta": 10000.0,
    "rms_norm_eps": 1e-5, "sliding_window": 4096, "bos_token_id": 1, "eos_token_id": 2}


def test_config_from_hf_window_opt_in():
    c = config_from_hf(MISTRAL_7B_JSON, "m", sliding_window=True)
    assert (c.max_position, c.sliding_window) == (32768, 4096)
    capped = config_from_hf(MISTRAL_7B_JSON, "m")               # unchanged: cap, no window
    assert (capped.max_position, capped.sliding_window) == (4096, 0)
    for sw in (None, 32768, 40000):                             # null / never reached: full
        c = config_from_hf(dict(MISTRAL_7B_JSON, sliding_window=sw), "m", sliding_window=True)
        assert (c.max_position, c.sliding_window) == (32768, 0)
        c = config_from_hf(dict(MISTRAL_7B_JSON, sliding_window=sw), "m")
        assert (c.max_position, c.sliding_window) == (32768, 0)


def test_config_field_round_trip_and_registry():
    c = config_from_hf(MISTRAL_7B_JSON, "m", sliding_window=True)
    d = json.loads(json.dumps(c.to_dict()))
    assert d["sliding_window"] == 4096
    assert ModelConfig.from_dict(d) == c
    d.pop("sliding_window")                  # a shard directory written before the field
    assert ModelConfig.from_dict(d).sliding_window == 0
    m7 = get_config("mistralai/Mistral-7B-v0.1")
    assert m7.name == "mistral-7b"
    assert dataclasses.replace(c, name=m7.name) == m7
    for twin, base in (("mistral-tiny128", "llama-tiny128"), ("mistral-tiny", "llama-tiny")):
        assert get_config(twin) == dataclasses.replace(get_config(base), name=twin,
                                                       sliding_window=24)
    assert get_config("llama3-8b").sliding_window == 0


# ------------------------------------------------------------------------------ HF parity
def hf_mistral(cfg, seed=0):
    """The eager HF twin of a windowed config (random weights, fp32)."""
    import transformers as tf
    torch.manual_seed(seed)
    c = tf.MistralConfig(
        vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size,
        intermediate_size=cfg.intermediate_size, num_hidden_layers=cfg.num_layers,
        num_attention_heads=cfg.num_heads, num_key_value_heads=cfg.num_kv_heads,
        head_dim=cfg.head_dim, rope_theta=cfg.rope_theta, rms_norm_eps=cfg.norm_eps,
        max_position_embeddings=cfg.max_position, bos_token_id=cfg.bos_token_id,
        eos_token_id=cfg.eos_token_id, tie_word_embeddings=False,
        sliding_window=cfg.sliding_window, attn_implementation="eager")
    return tf.MistralForCausalLM(c).float().eval()


@pytest.fixture(scope="module")
def twin():
    cfg = get_config("mistral-tiny128")
    hm = hf_mistral(cfg)
    return cfg, hm, from_hf_state_dict(cfg, hm.state_dict(), dtype=torch.float32)


def test_windowed_logits_match_hf(twin):
    cfg, hm, params = twin
    assert hm.config.sliding_window == 24 and hm.config._attn_implementation == "eager"
    with torch.no_grad():
        ref = hm(torch.tensor([PROMPT60])).logits[0, -1]
    ours = our_last_logits(cfg, params, PROMPT60)
    assert torch.allclose(ours, ref, atol=2e-4, rtol=1e-3), (ours - ref).abs().max()
    # the window matters at this length: the same weights under full attention are off
    full = our_last_logits(dataclasses.replace(cfg, sliding_window=0), params, PROMPT60)
    assert not torch.allclose(full, ref, atol=2e-4, rtol=1e-3)


@pytest.mark.parametrize("chunk", [16384, 4])
def test_windowed_greedy_generation_matches_hf(twin, chunk):
    """Greedy decode crosses the window (length 70 > 24) token for token with HF ``generate``;
    with 4-token prefill chunks the first chunks of the 30-token prompt lie wholly outside
    the last chunk's window."""
    cfg, hm, params = twin
    eng = LLMEngine(cfg, device="cpu", dtype=torch.float32, params=params, max_batch=4,
                    max_model_len=128, num_blocks=32, block_size=16, max_prefill_tokens=chunk)
    prompts = [PROMPT60[:6], PROMPT60[10:30], PROMPT60[20:50]]
    outs = eng.generate(prompts, SamplingParams(max_length=70, do_sample=False, ignore_eos=True))
    for p, o in zip(prompts, outs):
        with torch.no_grad():
            ref = hm.generate(torch.tensor([p]), max_length=70, do_sample=False,
                              eos_token_id=None, pad_token_id=0)[0].tolist()
        assert o.all_ids == ref, (len(p), o.all_ids, ref)


def test_load_hf_dir_keeps_the_window(twin, tmp_path):
    cfg, hm, _ = twin
    hm.save_pretrained(str(tmp_path / "ck"), safe_serialization=True)
    c2, params = load_hf_dir(tmp_path / "ck", dtype=torch.float32)
    assert (c2.sliding_window, c2.max_position) == (24, cfg.max_position)
    with torch.no_grad():
        ref = hm(torch.tensor([PROMPT60])).logits[0, -1]
    ours = our_last_logits(c2, params, PROMPT60)
    assert torch.allclose(ours, ref, atol=2e-4, rtol=1e-3), (ours - ref).abs().max()
