"""4-bit group-scaled (AWQ) weights off the GPU: the packing and its one definition, the import
of an AutoAWQ GEMM-packed checkpoint, every refusal, and the kernel choice."""
import json

import pytest
import torch

from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.engine import SamplingParams
from distributed_llm_inferencing_amd.engine.llm_engine import LLMEngine
from distributed_llm_inferencing_amd.models import get_config
from distributed_llm_inferencing_amd.models import weights as W
from distributed_llm_inferencing_amd.models.hf import config_from_hf, load_hf_dir
from distributed_llm_inferencing_amd.ops import gemm as G
from distributed_llm_inferencing_amd.ops import reference as R

IDS = [5, 17, 3, 99, 42, 7, 250]
KW = dict(device="cpu", max_batch=4, max_model_len=64, num_blocks=32)
QCFG = {"quant_method": "awq", "bits": 4, "group_size": 128, "zero_point": True,
        "version": "GEMM"}
LLAMA_HF = {"model_type": "llama", "hidden_size": 256, "num_attention_heads": 4,
            "num_key_value_heads": 2, "num_hidden_layers": 2, "intermediate_size": 512,
            "vocab_size": 512, "max_position_embeddings": 128}


def rand_qsz(n, k, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 16, (n, k), generator=g, dtype=torch.uint8)
    z = torch.randint(0, 16, (n, k // 128), generator=g, dtype=torch.uint8)
    s = (torch.rand(n, k // 128, generator=g) * 0.02 + 0.001).to(torch.float16)
    return q, s, z


def fp64(q, s, z):
    return (q.double() - z.double().repeat_interleave(128, 1)) * s.double().repeat_interleave(128, 1)


def test_pack_round_trip_and_the_formula():
    q, s, z = rand_qsz(48, 384, 0)
    qp, sz = R.pack_w4(q, s, z)
    assert qp.dtype == torch.uint8 and qp.shape == (48, 192) and sz.dtype == torch.int32
    assert all(torch.equal(a, b) for a, b in zip(R.unpack_w4(qp, sz), (q, s, z)))
    # the word the kernels read: nibble i of word w is element 8 w + [0, 2, 4, 6, 1, 3, 5, 7][i]
    word = int(qp.view(torch.int32)[5, 7]) & 0xFFFFFFFF
    assert [(word >> 4 * i) & 15 for i in range(8)] == \
        [int(q[5, 56 + e]) for e in (0, 2, 4, 6, 1, 3, 5, 7)]
    assert int(sz[5, 1]) == (int(s[5, 1].view(torch.int16)) & 0xFFFF) | int(z[5, 1]) << 16
    ref = fp64(q, s, z)
    assert torch.equal(R.dequantize_weight_w4(qp, sz).double(), ref.float().double())
    assert torch.equal(R.dequantize_weight_w4(qp, sz, torch.bfloat16), ref.to(torch.bfloat16))
    # the quantiser: q and z each round by half a step, so w comes back within one step; a
    # constant group (row 3) stays finite
    w = torch.randn(16, 256) * 0.05
    w[3] = 0.25
    qq, ss, zz = R.quantize_weight_w4(w)
    back = fp64(qq, ss, zz)
    assert torch.isfinite(back).all() and ss.min() > 0
    ok = (back - w).abs() <= ss.double().repeat_interleave(128, 1) * 1.001
    assert ok[:3].all() and ok[4:].all()
    with pytest.raises(ValueError, match="layers.0.wo.*multiple"):
        R.quantize_weight_w4(torch.zeros(16, 192), "layers.0.wo")


# ----------------------------------------------------------------------------- AWQ import
def awq_pack(intw):
    """AutoAWQ's WQLinear_GEMM packing of [rows, N] integers along N, as its source has it."""
    order_map = [0, 2, 4, 6, 1, 3, 5, 7]
    out = torch.zeros(intw.shape[0], intw.shape[1] // 8, dtype=torch.int32)
    for col in range(intw.shape[1] // 8):
        for i in range(8):
            out[:, col] |= intw[:, col * 8 + order_map[i]].to(torch.int32) << (i * 4)
    return out


PROJ = {"self_attn.q_proj": (256, 256), "self_attn.k_proj": (128, 256),
        "self_attn.v_proj": (128, 256), "self_attn.o_proj": (256, 256),
        "mlp.gate_proj": (512, 256), "mlp.up_proj": (512, 256), "mlp.down_proj": (256, 512)}


@pytest.fixture(scope="module")
def awq_dir(tmp_path_factory):
    """A tiny llama AWQ directory and the integers it was packed from: {module: (q, s, z)}.
    Layer 1's o_proj stays fp16 (modules_to_not_convert)."""
    from safetensors.torch import save_file
    d = tmp_path_factory.mktemp("awq")
    g = torch.Generator().manual_seed(1)
    sd = {"model.embed_tokens.weight": torch.randn(512, 256, generator=g).half() * 0.05,
          "lm_head.weight": torch.randn(512, 256, generator=g).half() * 0.05,
          "model.norm.weight": torch.ones(256).half()}
    known = {}
    for i in range(2):
        h = f"model.layers.{i}."
        sd[h + "input_layernorm.weight"] = torch.ones(256).half()
        sd[h + "post_attention_layernorm.weight"] = torch.ones(256).half()
        for j, (name, (n, k)) in enumerate(PROJ.items()):
            if (i, name) == (1, "self_attn.o_proj"):
                sd[h + name + ".weight"] = torch.randn(n, k, generator=g).half() * 0.05
                continue
            q, s, z = rand_qsz(n, k, 10 * i + j)
            known[h + name] = (q, s, z)
            sd[h + name + ".qweight"] = awq_pack(q.t())
            sd[h + name + ".qzeros"] = awq_pack(z.t())
            sd[h + name + ".scales"] = s.t().contiguous()
    save_file(sd, str(d / "model.safetensors"), metadata={"format": "pt"})
    qc = dict(QCFG, modules_to_not_convert=["model.layers.1.self_attn.o_proj"])
    (d / "config.json").write_text(json.dumps(dict(LLAMA_HF, quantization_config=qc)))
    return d, known


def test_load_awq_checkpoint(awq_dir):
    d, known = awq_dir
    assert _awq(version="gemm")(d).hidden_size == 256          # (the fixture's is "GEMM")
    cfg, params = load_hf_dir(d)
    deq = {}
    for i in range(2):
        h, p = f"model.layers.{i}.", f"layers.{i}."
        ref = {n: fp64(*known[h + n]).float() for n in PROJ if h + n in known}
        want = {"wqkv": torch.cat([ref["self_attn." + n + "_proj"] for n in "qkv"]),
                "w_gu": R.interleave_gate_up(ref["mlp.gate_proj"], ref["mlp.up_proj"]),
                "w_down": ref["mlp.down_proj"]}
        if i == 0:
            want["wo"] = ref["self_attn.o_proj"]
        for leaf, w in want.items():
            got = ops.W4Weight(params[p + leaf], params[p + leaf + "_sz"])
            assert torch.equal(got.dequantize(), w), (i, leaf)
            deq[p + leaf] = w
    assert params["layers.1.wo"].dtype == torch.bfloat16 and "layers.1.wo_sz" not in params
    assert params["embed"].dtype == torch.bfloat16
    eng = LLMEngine(cfg, params=params, **KW)
    assert eng.stats()["weight_dtype"] == eng.memory_report()["weight_dtype"] == "w4"
    assert isinstance(eng.model.layers[0]["w_gu"], ops.W4Weight)
    ref = LLMEngine(cfg, params={k: deq.get(k, v) for k, v in params.items()
                                 if not k.endswith("_sz")}, **KW)
    sp = SamplingParams(max_new_tokens=10, temperature=0.0, ignore_eos=True)
    toks = [[o.output_ids for o in e.generate([IDS, IDS[:3]], sp)] for e in (eng, ref)]
    assert ref.weight_dtype == "bf16" and toks[0] == toks[1] and len(toks[0][0]) == 10


def test_w4_switch_quantises_a_bf16_model(monkeypatch):
    monkeypatch.setenv("WEIGHT_DTYPE", "w4")
    eng = LLMEngine("llama-tiny", seed=3, **KW)
    p = eng.model.params
    assert eng.stats()["weight_dtype"] == "w4" and p["embed"].dtype == torch.bfloat16
    assert p["layers.0.wqkv"].dtype == torch.uint8 and p["layers.0.wqkv_sz"].dtype == torch.int32
    base = W.random_init(W.stage_param_shapes(eng.cfg, 0, 1, True, True), "cpu", seed=3)
    want = W.quantize_params(eng.cfg, base, "w4")
    assert torch.equal(want["layers.0.w_gu"], p["layers.0.w_gu"])
    assert torch.equal(want["layers.0.w_gu_sz"], p["layers.0.w_gu_sz"])


# ----------------------------------------------------------------------------- refusals
def _awq(**patch):
    return lambda d: config_from_hf(dict(LLAMA_HF, quantization_config=dict(QCFG, **patch)), "x")


def _shard(d):
    from distributed_llm_inferencing_amd.shard.writer import main
    main(["--model_name", "acme/l", "--num_shards", "2", "--output_dir", str(d / "out"),
          "--from-hf", str(d)])


def _tp(d):
    from distributed_llm_inferencing_amd.parallel.tensor import TensorParallelEngine
    TensorParallelEngine("llama-tiny", "cpu", weight_dtype="w4")


@pytest.mark.parametrize("call,match", [
    (_awq(bits=8), "bits"), (_awq(group_size=64), "group_size"), (_awq(version="gemv"), "version"),
    (_awq(zero_point=False), "zero_point"), (_awq(quant_method="gptq"), "quant_method"),
    (lambda d: config_from_hf({"model_type": "gpt2", "n_embd": 64, "n_layer": 1, "n_head": 2,
                               "vocab_size": 100, "quantization_config": QCFG}, "x"), "gpt2"),
    (lambda d: config_from_hf(dict(LLAMA_HF, model_type="mixtral", num_local_experts=4,
                                   quantization_config=QCFG), "x"), "mixtral"),
    (lambda d: config_from_hf(dict(LLAMA_HF, model_type="qwen3_moe", num_experts=4,
                                   moe_intermediate_size=64, quantization_config=QCFG), "x"),
     "qwen3_moe"),
    (lambda d: LLMEngine(*load_hf_dir(d)[:1], params=load_hf_dir(d)[1], weight_dtype="bf16",
                         **KW), "bf16"),
    (_shard, "AWQ"), (_tp, "w4"),
    (lambda d: LLMEngine("mixtral-tiny", weight_dtype="w4", **KW), "num_experts"),
    (lambda d: LLMEngine("gpt2-tiny", weight_dtype="w4", **KW), "gpt2")])
def test_refusals(awq_dir, monkeypatch, call, match):
    monkeypatch.delenv("WEIGHT_DTYPE", raising=False)
    with pytest.raises(ValueError, match=match):
        call(awq_dir[0])


# ----------------------------------------------------------------------------- kernel choice
def test_pick_kernel():
    w = ops.W4Weight(*R.pack_w4(*rand_qsz(64, 1024, 2)))
    assert G.wdt(w) == "w4" and tuple(w.shape) == (64, 1024) and w.dim() == 2
    assert not hasattr(w, "stream_ok") and not hasattr(w, "tiles_ok")
    gv, mfma, stream = G.GemmPlan("dli", 30, 2), G.GemmPlan("dli", 0, 1), G.GemmPlan("dli", 70, 1)
    for M in (1, 4):
        kind, p, ww = ops._pick_kernel(torch.zeros(M, 1024, dtype=torch.bfloat16), w, gv, "none")
        assert (kind, p, ww) == ("gemv_w4", gv, w)
    for M, p in ((5, gv), (8, gv), (2, mfma), (8, stream), (100, G.GemmPlan("dli", 72, 1))):
        kind, run, ww = ops._pick_kernel(torch.zeros(M, 1024, dtype=torch.bfloat16), w, p, "none")
        assert kind == "gemm" and torch.equal(ww, w.dequantize(torch.bfloat16))
        assert run.tile not in G.FP8_STREAM_TILES and run.tile not in G.FP8_TILE_TABLE
    # a slice that is no whole chunk, and what the autotuner offers
    assert not w.gemv_ok(1, G.GemmPlan("dli", 30, 128)) and w.gemv_ok(4, G.GemmPlan("dli", 56, 8))
    tiles = {p.tile for M in (1, 4, 8, 100) for p in G.autotune_plans(M, 64, 1024, "none", "w4")}
    assert tiles & set(G.GEMV_TILES) and not tiles & (set(G.FP8_STREAM_TILES) | set(G.FP8_TILE_TABLE))
