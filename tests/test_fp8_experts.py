"""FP8 block-scaled expert weights off the GPU: the per-expert quantiser and its stacked scale
layout, the import of per-expert HF FP8 checkpoints (the ``Qwen/Qwen3-30B-A3B-FP8`` layout),
the refusals that remain, expert slicing, the planner's grouped FP8 keys, HF parity of the
quantised tiny MoE models and two expert-parallel gloo ranks."""
import json
import os

import pytest
import torch
import torch.multiprocessing as mp

from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.engine import SamplingParams
from distributed_llm_inferencing_amd.engine.llm_engine import LLMEngine
from distributed_llm_inferencing_amd.models import get_config
from distributed_llm_inferencing_amd.models import weights as W
from distributed_llm_inferencing_amd.models.hf import config_from_hf, load_hf_dir
from distributed_llm_inferencing_amd.models.model import TransformerLM
from distributed_llm_inferencing_amd.ops import gemm as G
from distributed_llm_inferencing_amd.ops import reference as R

from hf_helpers import hf_model, our_last_logits
from test_fp8_weights import QCFG, block_dequant
from test_qwen3_moe import PROMPTS, _free_port, hf_config, hf_qwen3_moe, per_expert_state_dict

F8 = torch.float8_e4m3fn
IDS = [5, 17, 3, 99, 42, 7, 250]
ATTN = ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight",
        "self_attn.o_proj.weight")
EXPERT = ("gate_proj.weight", "up_proj.weight", "down_proj.weight")


def _is_expert_key(k):
    return ".experts." in k and k.endswith(EXPERT)


def fp8_state_dict(hm, skip=lambda k: False):
    """The per-expert FP8 checkpoint of the HF model ``hm`` (F8_E4M3 ``weight`` + F32
    ``weight_scale_inv`` per attention projection and per expert matrix; the router stays as
    it is), and ``hm`` itself loaded with the dequantised weights."""
    sd = {k: v.detach().clone() for k, v in per_expert_state_dict(hm).items()}
    deq = {}
    for k in [k for k in sd if (k.endswith(ATTN) or _is_expert_key(k)) and not skip(k)]:
        q, s = R.quantize_weight(sd[k])
        deq[k] = block_dequant(q, s)
        sd[k], sd[k + "_scale_inv"] = q, s
    with torch.no_grad():
        for name, p in hm.named_parameters():
            if name in deq:
                p.copy_(deq[name])
            elif name.endswith("experts.gate_up_proj"):
                f = p.shape[1] // 2
                for e in range(p.shape[0]):
                    g = name.replace("gate_up_proj", f"{e}.gate_proj.weight")
                    u = name.replace("gate_up_proj", f"{e}.up_proj.weight")
                    if g in deq:
                        p[e, :f].copy_(deq[g])
                    if u in deq:
                        p[e, f:].copy_(deq[u])
            elif name.endswith("experts.down_proj"):
                for e in range(p.shape[0]):
                    d = name.replace("down_proj", f"{e}.down_proj.weight")
                    if d in deq:
                        p[e].copy_(deq[d])
    return sd, deq


def _hf_twin(name):
    cfg = get_config(name)
    if name.startswith("qwen3"):
        return cfg, hf_qwen3_moe(cfg)
    torch.manual_seed(0)
    return cfg, hf_model(cfg)


@pytest.fixture(scope="module", params=["qwen3-moe-tiny", "mixtral-tiny"])
def fp8_twin(request):
    """(config, the HF model holding the dequantised weights, the FP8 state dict, the
    dequantised tensors by HF name, our fp32 params before quantisation, our FP8 params)."""
    cfg, hm = _hf_twin(request.param)
    plain = W.from_hf_state_dict(cfg, hm.state_dict(), dtype=torch.float32)
    sd, deq = fp8_state_dict(hm)
    return cfg, hm, sd, deq, plain, W.from_hf_state_dict(cfg, sd, dtype=torch.float32)


# ----------------------------------------------------------------------------- config
def test_config_from_hf_accepts_fp8_experts():
    cfg = get_config("qwen3-moe-tiny")
    d = hf_config(cfg).to_dict()
    assert d["model_type"] == "qwen3_moe"
    assert config_from_hf(dict(d, quantization_config=QCFG), cfg.name) == cfg
    assert config_from_hf(dict(d, quantization_config=QCFG), cfg.name).is_moe
    # what stays refused: other schemes, gpt2
    with pytest.raises(ValueError, match="weight_block_size"):
        config_from_hf(dict(d, quantization_config=dict(QCFG, weight_block_size=[64, 64])), "x")
    W.check_fp8_model(cfg)
    with pytest.raises(ValueError, match="gpt2"):
        W.check_fp8_model(get_config("gpt2-tiny"))


# ----------------------------------------------------------------------------- import
def test_per_expert_fp8_state_dict_converts(fp8_twin):
    cfg, hm, sd, deq, plain, params = fp8_twin
    E, f, d = cfg.num_experts, cfg.intermediate_size, cfg.hidden_size
    moe = "mlp." if "model.layers.0.mlp.gate.weight" in sd else "block_sparse_moe."
    for i in range(cfg.num_layers):
        p = f"layers.{i}."
        assert params[p + "w_gu"].dtype == F8 and params[p + "w_gu"].shape == (E, 2 * f, d)
        assert params[p + "w_down"].dtype == F8 and params[p + "w_down"].shape == (E, d, f)
        assert params[p + "w_gu_scale"].shape == (E, 2 * f // 16, -(-d // 128))
        assert params[p + "w_down_scale"].shape == (E, d // 16, -(-f // 128))
        assert params[p + "w_gu_scale"].dtype == params[p + "w_down_scale"].dtype == torch.float32
        assert params[p + "router"].dtype == torch.float32 and p + "router_scale" not in params
        assert params[p + "wqkv"].dtype == F8 and params[p + "wo"].dtype == F8
        gu = ops.Fp8Experts(params[p + "w_gu"], params[p + "w_gu_scale"])
        dn = ops.Fp8Experts(params[p + "w_down"], params[p + "w_down_scale"])
        assert gu.dim() == 3 and gu.shape == (E, 2 * f, d) and gu.numel() == E * 2 * f * d
        assert gu.device == params[p + "w_gu"].device
        ex = f"model.layers.{i}.{moe}experts."
        want_gu = torch.stack([R.interleave_gate_up(deq[f"{ex}{e}.gate_proj.weight"],
                                                    deq[f"{ex}{e}.up_proj.weight"])
                               for e in range(E)])
        want_dn = torch.stack([deq[f"{ex}{e}.down_proj.weight"] for e in range(E)])
        assert torch.equal(gu.dequantize(), want_gu)
        assert torch.equal(dn.dequantize(), want_dn)
        assert torch.equal(gu.bf16(), want_gu.to(torch.bfloat16))
        assert torch.equal(R.dequantize_experts(gu.q, gu.scale)[E - 1],
                           R.dequantize_weight(gu.q[E - 1], gu.scale[E - 1]))
    # quantising the converted bf16/fp32 model takes the same unfused tensors: the same bytes
    qp = W.quantize_params(cfg, plain)
    assert set(qp) == set(params)
    for k in params:
        a, b = qp[k], params[k]
        assert a.dtype == b.dtype and torch.equal(W._u8(a), W._u8(b)), k


def test_partly_quantised_experts_are_refused_by_name():
    cfg, hm = _hf_twin("mixtral-tiny")
    one = "model.layers.1.mlp.experts.2.down_proj.weight"
    sd, _ = fp8_state_dict(hm, skip=lambda k: k == one)
    if one not in sd:
        one = one.replace("mlp.", "block_sparse_moe.")
    assert one in sd and one + "_scale_inv" not in sd
    with pytest.raises(ValueError, match=r"layers\.1\..*experts\.2\.down_proj"):
        W.from_hf_state_dict(cfg, sd, dtype=torch.float32)
    # gate with a scale, up without: the pair cannot fuse
    up = one.replace("2.down_proj", "0.up_proj")
    cfg, hm = _hf_twin("mixtral-tiny")
    sd, _ = fp8_state_dict(hm, skip=lambda k: k == up)
    with pytest.raises(ValueError, match=r"experts\.0\.up_proj"):
        W.from_hf_state_dict(cfg, sd, dtype=torch.float32)
    # every down projection plain, every gate / up FP8
    cfg, hm = _hf_twin("mixtral-tiny")
    sd, _ = fp8_state_dict(hm, skip=lambda k: k.endswith("down_proj.weight"))
    with pytest.raises(ValueError, match=r"experts\.0\.down_proj"):
        W.from_hf_state_dict(cfg, sd, dtype=torch.float32)


def test_fused_fp8_expert_layout_is_refused_by_name():
    cfg, hm = _hf_twin("mixtral-tiny")
    sd = {k: v.detach().clone() for k, v in hm.state_dict().items()}
    fused = [k for k in sd if k.endswith("experts.gate_up_proj")]
    assert fused, "this transformers stores the experts fused"
    k = fused[0]
    sd[k + "_scale_inv"] = torch.ones(sd[k].shape[0], -(-sd[k].shape[1] // 128),
                                      -(-sd[k].shape[2] // 128))
    with pytest.raises(ValueError, match=r"experts\.gate_up_proj_scale_inv"):
        W.from_hf_state_dict(cfg, sd, dtype=torch.float32)


def test_rows_not_a_multiple_of_16_are_refused():
    cfg = get_config("mixtral-tiny")
    shapes = {"layers.0.w_gu": (2, 64, 120), "layers.0.w_down": (2, 120, 32)}
    params = W.random_init(shapes, "cpu", torch.float32)
    with pytest.raises(ValueError, match=r"layers\.0\.w_down\[0\].*multiple of 16"):
        W.quantize_params(cfg, params)
    with pytest.raises(ValueError, match="Fp8Experts"):
        ops.Fp8Experts(torch.zeros(2, 16, 128).to(F8), torch.ones(16, 1))
    with pytest.raises(ValueError, match="3-D"):
        ops.Fp8Experts(torch.zeros(16, 128).to(F8), torch.ones(1, 1))


# ----------------------------------------------------------------------------- slicing
@pytest.mark.parametrize("name", ["qwen3-moe-tiny", "mixtral-tiny"])
def test_slice_experts_and_scratch(name):
    cfg = get_config(name)
    shapes = W.stage_param_shapes(cfg, 0, 1, True, True)
    params = W.random_init(shapes, "cpu", torch.float32, seed=3, std=0.05)
    qp = W.quantize_params(cfg, params)
    E = cfg.num_experts
    er = (E // 4, E // 2)
    cut = {k: W.slice_experts(k, v, er) for k, v in params.items()}
    assert cut["layers.0.w_gu"].shape[0] == er[1] - er[0]
    qcut = W.quantize_params(cfg, cut)
    for leaf in ("w_gu", "w_gu_scale", "w_down", "w_down_scale"):
        k = "layers.0." + leaf
        got = W.slice_experts(k, qp[k], er)
        assert got.shape[0] == er[1] - er[0]
        assert torch.equal(W._u8(got), W._u8(qcut[k])), k
    assert torch.equal(W.slice_experts("layers.0.wqkv_scale", qp["layers.0.wqkv_scale"], er),
                       qp["layers.0.wqkv_scale"])
    # the bf16 scratch holds the larger stack whole (the dequantise path rewrites all of it)
    stack = max(qp["layers.0.w_gu"].numel(), qp["layers.0.w_down"].numel())
    assert W.fp8_scratch_bytes(cfg) >= 2 * stack
    assert W.fp8_scratch_bytes(cfg, experts=er[1] - er[0]) >= 2 * stack * (er[1] - er[0]) // E
    assert W.fp8_scratch_bytes(get_config("llama-tiny")) == W.fp8_scratch_bytes(
        get_config("llama-tiny"), experts=3)


# ----------------------------------------------------------------------------- model, engine
def test_quantised_model_matches_hf_on_the_dequantised_weights(fp8_twin):
    cfg, hm, sd, deq, plain, params = fp8_twin
    with torch.no_grad():
        ref = hm(torch.tensor([IDS])).logits[0, -1]
    ours = our_last_logits(cfg, params, IDS)
    assert torch.allclose(ours, ref, atol=2e-4, rtol=1e-3), (ours - ref).abs().max()
    # the engine switch on the unquantised weights arrives at the same model (Qwen3-MoE; a
    # Mixtral engine takes the quantised parameters, the switch stays refused for it)
    kw = (dict(params=dict(plain), weight_dtype="fp8") if cfg.qk_norm
          else dict(params=W.quantize_params(cfg, plain)))
    eng = LLMEngine(cfg, device="cpu", dtype=torch.float32, max_batch=4, max_model_len=64,
                    num_blocks=32, **kw)
    assert eng.stats()["weight_dtype"] == "fp8" and eng.weight_dtype == "fp8"
    assert isinstance(eng.model.layers[0]["w_gu"], ops.Fp8Experts)
    assert isinstance(eng.model.layers[0]["wqkv"], ops.Fp8Weight)
    out = eng.generate([IDS], SamplingParams(max_length=20, do_sample=False, ignore_eos=True))
    with torch.no_grad():
        want = hm.generate(torch.tensor([IDS]), max_length=20, do_sample=False,
                           eos_token_id=None, pad_token_id=0)[0].tolist()
    assert IDS + out[0].output_ids == want
    with pytest.raises(ValueError, match="bf16"):
        LLMEngine(cfg, device="cpu", params=params, weight_dtype="bf16", max_batch=4,
                  max_model_len=64, num_blocks=32)


def write_fp8_moe_dir(d):
    """A directory in the released per-expert FP8 layout (config.json with the
    quantization_config, one safetensors file) of the qwen3-moe-tiny twin; returns (config,
    the HF model holding the dequantised weights)."""
    from safetensors.torch import save_file
    cfg, hm = _hf_twin("qwen3-moe-tiny")
    sd, _ = fp8_state_dict(hm)
    d.mkdir(parents=True)
    save_file({k: v.contiguous() for k, v in sd.items()}, str(d / "model.safetensors"),
              metadata={"format": "pt"})
    c = json.loads(hm.config.to_json_string())
    c["quantization_config"] = dict(QCFG, modules_to_not_convert=["lm_head", "mlp.gate"])
    (d / "config.json").write_text(json.dumps(c))
    return cfg, hm


def test_fp8_moe_checkpoint_directory_loads_and_generates(tmp_path):
    cfg, hm = write_fp8_moe_dir(tmp_path / "ck")
    c2, params = load_hf_dir(tmp_path / "ck", dtype=torch.float32, name=cfg.name)
    assert c2 == cfg and params["layers.0.w_gu"].dtype == F8
    eng = LLMEngine(c2, device="cpu", params=params, dtype=torch.float32, max_batch=4,
                    max_model_len=64, num_blocks=32)
    assert eng.stats()["weight_dtype"] == "fp8"
    out = eng.generate([IDS], SamplingParams(max_length=16, do_sample=False, ignore_eos=True))
    with torch.no_grad():
        want = hm.generate(torch.tensor([IDS]), max_length=16, do_sample=False,
                           eos_token_id=None, pad_token_id=0)[0].tolist()
    assert IDS + out[0].output_ids == want


def test_load_model_serves_an_fp8_moe_checkpoint(tmp_path):
    """The worker's /load_model finds the directory in its model cache, loads the FP8 experts
    as they are and /inference generates what an engine on the same tensors generates."""
    from distributed_llm_inferencing_amd.worker.server import create_worker_app
    from test_pipeline_serving import SMALL, _settings
    s = _settings(tmp_path)
    name = "qwen3-moe-tiny"
    cfg, _ = write_fp8_moe_dir(tmp_path / "cache" / name)
    app = create_worker_app(s, device="cpu", engine_kwargs=SMALL)
    c = app.test_client()
    r = c.post("/load_model", json={"model_name": name})
    assert r.status_code == 200, r.get_json()
    st = app.extensions["dli_worker"]
    assert st.weights_source[name] == "cache"
    body = {"model_name": name, "prompt": "abc", "max_length": 16, "temperature": 0}
    got = c.post("/inference", json=body).get_json()["result"]
    c2, params = load_hf_dir(tmp_path / "cache" / name, dtype=torch.float32, name=name)
    ref = LLMEngine(c2, device="cpu", params=params, dtype=torch.float32, **SMALL)
    assert ref.weight_dtype == "fp8"
    want = ref.generate(["abc"], SamplingParams(max_length=16, temperature=0))[0]
    assert got == want.resolve_text()
    m = c.get("/metrics")
    assert m.status_code == 200 and "fp8" in m.get_data(as_text=True)


def test_cpu_moe_mlp_runs_on_the_dequantised_stack():
    torch.manual_seed(0)
    E, F, D, T, k = 4, 32, 128, 6, 2
    cfg = get_config("mixtral-tiny")
    qp = W.quantize_params(cfg, {"layers.0.w_gu": torch.randn(E, 2 * F, D) * 0.1,
                                 "layers.0.w_down": torch.randn(E, D, F) * 0.1})
    w_gu = ops.Fp8Experts(qp["layers.0.w_gu"], qp["layers.0.w_gu_scale"])
    w_dn = ops.Fp8Experts(qp["layers.0.w_down"], qp["layers.0.w_down_scale"])
    x = torch.randn(T, D)
    tw, ti = R.router_topk(torch.randn(T, E), k)
    got = ops.moe_mlp(x, w_gu, w_dn, tw, ti)
    want = R.moe_mlp(x, w_gu.dequantize(), w_dn.dequantize(), tw, ti)
    assert torch.equal(got, want) and want.abs().max() > 0
    # an expert_range shard: experts 1..2 of the stack
    half = ops.moe_mlp(x, ops.Fp8Experts(w_gu.q[1:3], w_gu.scale[1:3]),
                       ops.Fp8Experts(w_dn.q[1:3], w_dn.scale[1:3]), tw, ti, expert_offset=1)
    want = R.moe_mlp(x, w_gu.dequantize()[1:3], w_dn.dequantize()[1:3], tw, ti, 1)
    assert torch.equal(half, want)


# ----------------------------------------------------------------------------- planner
def test_fp8_grouped_bm():
    # 1.25 x mean rows per expert, in the smallest of 16 / 32 / 48 / 64 that holds it
    assert G.fp8_grouped_bm(8 * 8, 128) == 16          # Qwen3-MoE batch 8: 0.5 rows
    assert G.fp8_grouped_bm(64 * 8, 128) == 16         # batch 64: 4 rows
    assert G.fp8_grouped_bm(512 * 8, 128) == 48        # batch 512: 32 rows -> 40
    assert G.fp8_grouped_bm(64 * 2, 8) == 32           # Mixtral batch 64: 16 rows -> 20
    assert G.fp8_grouped_bm(512 * 2, 8) == 64          # 128 rows: capped
    assert G.fp8_grouped_bm(0, 8) == 16 and G.fp8_grouped_bm(5, 0) == 16
    for rows, groups, want in ((128, 10, 16), (129, 10, 32), (256, 10, 32), (257, 10, 48),
                               (384, 10, 48), (385, 10, 64)):
        assert G.fp8_grouped_bm(rows, groups) == want, (rows, groups)


def test_grouped_plan_keys_are_separate_per_weight_dtype():
    saved = dict(G._grouped_cache)
    try:
        G._grouped_cache.clear()
        shape = (64, 512, 256, "silu_mul", 4)
        bf = G.grouped_plan(*shape)
        assert bf.tile in G.TILES and bf.tile not in G.FP8_STREAM_TILES
        # untuned: the stream for an FP8 stack, never for a bf16 one
        assert G.grouped_plan(*shape, wd="fp8") == G.GemmPlan("dli", 70, 1)
        G._grouped_cache[G._grouped_key(*shape, wd="fp8")] = G.GemmPlan("dli", 71, 1)
        assert G.grouped_plan(*shape, wd="fp8").tile == 71
        assert G.grouped_plan(*shape) == bf
        assert G._grouped_key(*shape) == (64, 512, 256, "silu_mul", 4)
        assert G._grouped_key(*shape, wd="fp8") != G._grouped_key(*shape)
        G._grouped_cache[G._grouped_key(*shape)] = G.GemmPlan("dli", 2, 1)
        assert G.grouped_plan(*shape).tile == 2 and G.grouped_plan(*shape, wd="fp8").tile == 71
        for rows in (1, 8, 64, 512, 4096):
            for groups in (4, 8, 128):
                G._grouped_cache.clear()
                assert G.grouped_plan(rows, 512, 256, "none", groups).tile in G.TILES
    finally:
        G._grouped_cache.clear()
        G._grouped_cache.update(saved)


def test_stream_ok_truth_table():
    w = ops.Fp8Experts(torch.zeros(4, 32, 256).to(F8), torch.ones(4, 2, 2))
    p70, p71 = G.GemmPlan("dli", 70, 1), G.GemmPlan("dli", 71, 1)
    assert w.stream_ok(64, 4, p70) and w.stream_ok(1, 4, p71) and w.stream_ok(4096, 4, p70)
    assert not w.stream_ok(64, 4, G.GemmPlan("dli", 70, 2))       # no split-K
    assert not w.stream_ok(64, 4, G.GemmPlan("dli", 1, 1))        # a bf16 tile
    assert not w.stream_ok(0, 4, p70)
    assert not w.stream_ok(64, 3, p70)                            # another stack
    odd = ops.Fp8Experts(torch.zeros(4, 32, 72).to(F8), torch.ones(4, 2, 1))
    assert not odd.stream_ok(64, 4, p70)                          # K % 16
    assert G.wdt(w) == "fp8" and G.wdt(torch.zeros(4, 32, 256)) is None
    # a bf16 stack with a stream plan pinned by hand is an error, not a wrong kernel
    saved = dict(G._grouped_cache)
    try:
        G._grouped_cache[G._grouped_key(8, 32, 256, "none", 4)] = p70
        with pytest.raises(ValueError, match="70"):
            ops._expert_plan(torch.zeros(4, 32, 256), 8, 8, 32, 256, "none", 4, 16, True)
    finally:
        G._grouped_cache.clear()
        G._grouped_cache.update(saved)


# ----------------------------------------------------------------------------- expert parallel
def _ep_worker(rank, world, port, q, model):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    import torch.distributed as dist
    from distributed_llm_inferencing_amd.parallel.expert import ExpertParallelEngine
    eng = ExpertParallelEngine(model, "cpu", max_batch=8, max_model_len=64, num_blocks=64,
                               dtype=torch.float32, weight_dtype="fp8")
    lp = eng.engine.model.layers[0]
    mine = PROMPTS[rank::world] if rank == 0 else PROMPTS[rank::world][:1]
    sp = SamplingParams(max_length=18, do_sample=False, ignore_eos=True)
    out = [o.all_ids for o in eng.generate(mine, sp)]
    q.put((rank, mine, out, type(lp["w_gu"]).__name__, tuple(lp["w_gu"].shape),
           eng.engine.stats()["weight_dtype"]))
    dist.barrier()
    dist.destroy_process_group()


def test_expert_parallel_gloo_fp8_matches_one_engine():
    """128 FP8 experts over 2 gloo ranks (64 each, quantised after slicing) == one fp32 engine
    that quantised every expert, token for token."""
    model, world = "qwen3-moe-tiny", 2
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
                    num_blocks=64, weight_dtype="fp8")
    sp = SamplingParams(max_length=18, do_sample=False, ignore_eos=True)
    cfg = get_config(model)
    for rank, mine, out, kind, shape, wdt in res:
        assert kind == "Fp8Experts" and wdt == "fp8"
        assert shape == (cfg.num_experts // world, 2 * cfg.intermediate_size, cfg.hidden_size)
        ref = [o.all_ids for o in eng.generate(mine, sp)]
        assert out == ref, (rank, out, ref)
    assert isinstance(eng.model, TransformerLM) and eng.model.weight_dtype == "fp8"
