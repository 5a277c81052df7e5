"""Qwen3-MoE (Qwen3 layers, 128 routed experts of their own width, top-8, optional
renormalisation of the routing weights) on the CPU path: the registry, the HF config import
and what it refuses, the routing reference against transformers' router, both expert weight
layouts, and the model, the engine and expert parallelism against HF transformers' eager
``Qwen3MoeForCausalLM`` in fp32."""
import dataclasses
import json
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from distributed_llm_inferencing_amd.engine import SamplingParams
from distributed_llm_inferencing_amd.engine.llm_engine import LLMEngine
from distributed_llm_inferencing_amd.models import ModelConfig, get_config
from distributed_llm_inferencing_amd.models import weights as W
from distributed_llm_inferencing_amd.models.hf import config_from_hf, load_hf_dir
from distributed_llm_inferencing_amd.models.weights import from_hf_state_dict
from distributed_llm_inferencing_amd.ops import reference as R

from hf_helpers import our_last_logits

PROMPT14 = [(7 * i + 3) % 1024 for i in range(14)]
TWINS = ["qwen3-moe-tiny", "qwen3-moe-tiny128"]


def hf_config(cfg, **over):
    import transformers as tf
    kw = dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size,
              intermediate_size=4 * cfg.hidden_size, moe_intermediate_size=cfg.intermediate_size,
              num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.num_heads,
              num_key_value_heads=cfg.num_kv_heads, head_dim=cfg.head_dim,
              num_experts=cfg.num_experts, num_experts_per_tok=cfg.top_k_experts,
              norm_topk_prob=cfg.norm_topk_prob, rope_theta=cfg.rope_theta,
              rms_norm_eps=cfg.norm_eps, max_position_embeddings=cfg.max_position,
              bos_token_id=cfg.bos_token_id, eos_token_id=cfg.eos_token_id,
              tie_word_embeddings=cfg.tie_embeddings, attention_bias=cfg.qkv_bias,
              use_sliding_window=False, attn_implementation="eager")
    kw.update(over)
    return tf.Qwen3MoeConfig(**kw)


def hf_qwen3_moe(cfg, seed=0):
    """The eager HF twin (fp32) of a Qwen3-MoE tiny config: transformers' own random weights
    (router and fused expert tensors included, std 0.02) and q/k norm weights that are not all
    ones."""
    import transformers as tf
    torch.manual_seed(seed)
    hm = tf.Qwen3MoeForCausalLM(hf_config(cfg)).float().eval()
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for n, p in hm.named_parameters():
            if n.endswith(("q_norm.weight", "k_norm.weight")):
                p.copy_(1 + 0.3 * torch.randn(p.shape, generator=g))
    return hm


@pytest.fixture(scope="module", params=TWINS)
def twin(request):
    cfg = get_config(request.param)
    hm = hf_qwen3_moe(cfg)
    return cfg, hm, from_hf_state_dict(cfg, hm.state_dict(), dtype=torch.float32)


# ------------------------------------------------------------------------------ registry
def test_registry_qwen3_30b_a3b():
    c = get_config("qwen3-30b-a3b")
    for alias in ("Qwen/Qwen3-30B-A3B", "qwen3_30b_a3b"):
        assert get_config(alias) == c
    assert (c.hidden_size, c.num_layers, c.num_heads, c.num_kv_heads, c.head_dim,
            c.intermediate_size, c.num_experts, c.top_k_experts, c.vocab_size, c.max_position,
            c.rope_theta, c.norm_eps, c.bos_token_id, c.eos_token_id) == (
                2048, 48, 32, 4, 128, 768, 128, 8, 151936, 40960, 1e6, 1e-6, 151643, 151645)
    assert c.qk_norm and c.norm_topk_prob and not c.tie_embeddings and not c.qkv_bias
    # 48 x (128 x 3 x 2048 x 768 + attention) + 2 x 151936 x 2048 ~ 30.5e9
    assert 30.0e9 < c.param_count() < 31.0e9
    t = get_config("qwen3-moe-tiny")
    assert t == dataclasses.replace(get_config("qwen3-tiny"), name="qwen3-moe-tiny",
                                    num_experts=128, top_k_experts=8, intermediate_size=64)
    t128 = get_config("qwen3-moe-tiny128")
    assert t128 == dataclasses.replace(get_config("qwen3-tiny128"), name="qwen3-moe-tiny128",
                                       num_experts=16, top_k_experts=4, intermediate_size=128,
                                       norm_topk_prob=False)
    assert t128.tie_embeddings and t128.q_size != t128.hidden_size


def test_norm_topk_prob_round_trips_and_defaults_true():
    c = get_config("qwen3-moe-tiny128")
    d = json.loads(json.dumps(c.to_dict()))
    assert d["norm_topk_prob"] is False and ModelConfig.from_dict(d) == c
    d.pop("norm_topk_prob")                    # a shard directory written before the field
    assert ModelConfig.from_dict(d).norm_topk_prob is True
    assert get_config("mixtral-8x7b").norm_topk_prob is True


# ------------------------------------------------------------------------------ config import
@pytest.mark.parametrize("name", TWINS)
def test_config_from_hf_qwen3_moe(name):
    cfg = get_config(name)
    d = hf_config(cfg).to_dict()
    assert d["model_type"] == "qwen3_moe"
    assert config_from_hf(d, cfg.name) == cfg
    # the hub's config.json spells the expert count num_experts
    hub = {k: v for k, v in d.items() if k != "num_local_experts"}
    hub["num_experts"] = cfg.num_experts
    assert config_from_hf(hub, cfg.name) == cfg
    hub.pop("norm_topk_prob")                  # Qwen3MoeConfig's default
    assert config_from_hf(hub, cfg.name).norm_topk_prob is False
    assert config_from_hf(dict(hub, norm_topk_prob=True), cfg.name).norm_topk_prob is True
    assert config_from_hf(dict(d, attention_bias=True), cfg.name).qkv_bias


@pytest.mark.parametrize("field,value", [("mlp_only_layers", [1]), ("decoder_sparse_step", 2),
                                         ("shared_expert_intermediate_size", 512),
                                         ("use_sliding_window", True)])
def test_config_from_hf_qwen3_moe_refuses(field, value):
    d = hf_config(get_config("qwen3-moe-tiny")).to_dict()
    with pytest.raises(ValueError, match=field):
        config_from_hf(dict(d, **{field: value}), "x")


def test_unsupported_type_message_lists_qwen3_moe():
    with pytest.raises(ValueError, match="qwen3_moe"):
        config_from_hf({"model_type": "qwen2_moe"}, "x")


# ------------------------------------------------------------------------------ routing
@pytest.mark.parametrize("E,k", [(128, 8), (16, 4)])
def test_router_topk_unnormalised_matches_transformers(E, k):
    from transformers.models.qwen3_moe.modeling_qwen3_moe import Qwen3MoeTopKRouter
    logits = 2 * torch.randn(9, E, generator=torch.Generator().manual_seed(E))
    for norm in (False, True):
        r = Qwen3MoeTopKRouter(hf_config(get_config("qwen3-moe-tiny"), hidden_size=E,
                                         num_experts=E, num_experts_per_tok=k,
                                         norm_topk_prob=norm))
        with torch.no_grad():
            r.weight.copy_(torch.eye(E))               # router logits = the input rows
            _, hw, hi = r(logits)
        w, ids = R.router_topk(logits, k, norm_topk=norm)
        assert torch.equal(ids.long(), hi) and w.dtype == torch.float32
        assert torch.allclose(w, hw, atol=1e-7, rtol=1e-6)
        if norm:
            assert torch.allclose(w.sum(-1), torch.ones(9), atol=1e-6)
        else:
            assert torch.equal(w, logits.softmax(-1).gather(1, hi)) and bool((w.sum(-1) < 1).all())
    dw, di = R.router_topk(logits, k)                  # the default renormalises, as before
    nw, ni = R.router_topk(logits, k, norm_topk=True)
    assert torch.equal(dw, nw) and torch.equal(di, ni)


# ------------------------------------------------------------------------------ weights
def per_expert_state_dict(hm):
    """The checkpoint layout of the released Qwen3-MoE files: one gate / up / down matrix per
    expert under ``mlp.experts.{e}.`` instead of the fused tensors."""
    sd = {}
    for k, v in hm.state_dict().items():
        if k.endswith("experts.gate_up_proj"):
            f = v.shape[1] // 2
            for e in range(v.shape[0]):
                sd[k.replace("gate_up_proj", f"{e}.gate_proj.weight")] = v[e, :f].clone()
                sd[k.replace("gate_up_proj", f"{e}.up_proj.weight")] = v[e, f:].clone()
        elif k.endswith("experts.down_proj"):
            for e in range(v.shape[0]):
                sd[k.replace("down_proj", f"{e}.down_proj.weight")] = v[e].clone()
        else:
            sd[k] = v
    return sd


def test_both_expert_layouts_convert_alike(twin):
    cfg, hm, params = twin
    assert type(hm).__name__ == "Qwen3MoeForCausalLM"
    assert hm.config._attn_implementation == "eager"
    assert any(k.endswith("mlp.experts.gate_up_proj") for k in hm.state_dict())
    sd = per_expert_state_dict(hm)
    assert f"model.layers.1.mlp.experts.{cfg.num_experts - 1}.up_proj.weight" in sd
    assert not any(k.endswith("gate_up_proj") for k in sd)
    split = from_hf_state_dict(cfg, sd, dtype=torch.float32)
    assert set(split) == set(params) == set(
        W.stage_param_shapes(cfg, 0, cfg.num_layers, True, True))
    for k in params:
        assert torch.equal(split[k], params[k]), k
    f = cfg.intermediate_size
    assert params["layers.0.w_gu"].shape == (cfg.num_experts, 2 * f, cfg.hidden_size)
    assert params["layers.0.router"].shape == (cfg.num_experts, cfg.hidden_size)
    assert params["layers.0.w_gu"].abs().max() > 0 and params["layers.0.router"].abs().max() > 0


# ------------------------------------------------------------------------------ HF parity
def test_logits_match_hf_fp32_and_bf16(twin):
    cfg, hm, params = twin
    with torch.no_grad():
        ref = hm(torch.tensor([PROMPT14])).logits[0, -1]
    ours = our_last_logits(cfg, params, PROMPT14)
    assert (ours - ref).abs().max() <= 1e-4, (ours - ref).abs().max()
    # the routing weights' normalisation matters: the other setting is off
    flipped = our_last_logits(dataclasses.replace(cfg, norm_topk_prob=not cfg.norm_topk_prob),
                              params, PROMPT14)
    assert (flipped - ref).abs().max() > 1e-3
    bf = our_last_logits(cfg, {k: v.to(torch.bfloat16) for k, v in params.items()}, PROMPT14)
    err = (bf.float() - ref).abs().max()
    assert err <= 0.05 * ref.abs().max() + 0.02, (err, ref.abs().max())


def test_saved_checkpoint_loads_and_generates_like_hf(twin, tmp_path):
    cfg, hm, _ = twin
    hm.save_pretrained(str(tmp_path / "ck"), safe_serialization=True)
    c2, params = load_hf_dir(tmp_path / "ck", dtype=torch.float32, name=cfg.name)
    assert c2 == cfg
    eng = LLMEngine(c2, device="cpu", dtype=torch.float32, params=params, max_batch=4,
                    max_model_len=64, num_blocks=16, block_size=16)
    prompts = [PROMPT14[:6], PROMPT14]
    outs = eng.generate(prompts, SamplingParams(max_new_tokens=16, do_sample=False,
                                                ignore_eos=True))
    for p, o in zip(prompts, outs):
        with torch.no_grad():
            ref = hm.generate(torch.tensor([p]), max_new_tokens=16, do_sample=False,
                              eos_token_id=None, pad_token_id=0)[0].tolist()
        assert len(o.all_ids) == len(p) + 16 and o.all_ids == ref, (len(p), o.all_ids, ref)


# ------------------------------------------------------------------------------ expert parallel
PROMPTS = [[5, 6, 7, 8], [9, 10, 11], [1, 2, 3, 4, 5, 6, 7], [100, 200], [7] * 9, [3, 4], [8] * 3]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _ep_worker(rank, world, port, q, model):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    import torch.distributed as dist
    from distributed_llm_inferencing_amd.parallel.expert import ExpertParallelEngine
    eng = ExpertParallelEngine(model, "cpu", max_batch=8, max_model_len=64, num_blocks=64,
                               dtype=torch.float32)
    mine = PROMPTS[rank::world] if rank == 0 else PROMPTS[rank::world][:1]
    sp = SamplingParams(max_length=18, do_sample=False, ignore_eos=True)
    out = [o.all_ids for o in eng.generate(mine, sp)]
    q.put((rank, mine, out, eng.moe.norm_topk))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_expert_parallel_gloo_matches_dense(world):
    """128 experts over 2 / 4 gloo ranks (64 / 32 each, a token's 8 picks spread over all of
    them) == one fp32 engine with every expert, token for token."""
    model = "qwen3-moe-tiny"
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ep_worker, args=(r, world, port, q, model))
             for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    eng = LLMEngine(model, device="cpu", dtype=torch.float32, max_batch=8, max_model_len=64,
                    num_blocks=64)
    sp = SamplingParams(max_length=18, do_sample=False, ignore_eos=True)
    for rank, mine, out, norm in res:
        assert norm is True
        assert out == [o.all_ids for o in eng.generate(mine, sp)], rank
