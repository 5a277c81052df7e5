"""FP8 block-scaled weights off the GPU: the quantiser and its scale layout, the import of HF
FP8 checkpoints (``float8_e4m3fn`` tensors + ``weight_scale_inv`` in 128 x 128 blocks), every
refusal, and the engine switch (``weight_dtype`` / ``WEIGHT_DTYPE``)."""
import json
from dataclasses import replace

import pytest
import torch

from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.engine import SamplingParams
from distributed_llm_inferencing_amd.engine.llm_engine import LLMEngine
from distributed_llm_inferencing_amd.models import get_config
from distributed_llm_inferencing_amd.models import weights as W
from distributed_llm_inferencing_amd.models.hf import config_from_hf, load_hf_dir
from distributed_llm_inferencing_amd.ops import reference as R

from hf_helpers import hf_model, our_last_logits

F8 = torch.float8_e4m3fn
IDS = [5, 17, 3, 99, 42, 7, 250]


def block_dequant(q, s_blocks):
    """HF's own reconstruction: W = q * weight_scale_inv over 128 x 128 blocks."""
    n, k = q.shape
    se = s_blocks.repeat_interleave(128, 0)[:n].repeat_interleave(128, 1)[:, :k]
    return q.float() * se


# ----------------------------------------------------------------------------- quantiser
def test_quantize_weight_scales_and_round_trip():
    torch.manual_seed(0)
    w = torch.randn(200, 300) * 0.05                # ceil blocks on both axes
    w[128:, 256:] = 0                               # a zero block
    w[3, 5] = 7.0                                   # one block's amax
    q, s = R.quantize_weight(w)
    assert q.dtype == F8 and q.shape == w.shape and s.shape == (2, 3) and s.dtype == torch.float32
    for i in range(2):
        for j in range(3):
            blk = w[128 * i:128 * (i + 1), 128 * j:128 * (j + 1)]
            want = blk.abs().max() / 448 if blk.abs().max() > 0 else torch.tensor(1.0)
            assert s[i, j] == want.float(), (i, j)
    assert s[0, 0] == torch.tensor(7.0) / 448 and s[1, 2] == 1.0
    assert torch.all(q[128:, 256:].float() == 0)
    back = block_dequant(q, s)
    # e4m3 keeps 3 mantissa bits: half an ulp is 2^-4 of the value; subnormals of a block
    # step by s * 2^-9
    err = (back - w).abs()
    bound = w.abs() * 2.0 ** -4 + s.repeat_interleave(128, 0)[:200].repeat_interleave(
        128, 1)[:, :300] * 2.0 ** -10
    assert torch.all(err <= bound * 1.0001)
    # the in-memory layout reconstructs the same values
    w2 = torch.randn(208, 300) * 0.05
    q2, s2 = R.quantize_weight(w2)
    g2 = R.group_scales(R.row_scales(s2, 208))
    assert g2.shape == (13, 3)
    assert torch.equal(R.dequantize_weight(q2, g2, torch.float32), block_dequant(q2, s2))
    assert torch.equal(R.dequantize_weight(q2, g2, torch.bfloat16),
                       block_dequant(q2, s2).to(torch.bfloat16))


def test_quantize_weight_block_extremes_and_clamp():
    """A block's amax maps to +-448 and nothing comes out inf or nan. The clamp is what keeps
    it so where w / s rounds past 448 in fp32: with s = amax / 448 rounded down, amax / s can
    exceed 448, and beyond 464 torch's own cast gives nan. Every fp32 amax over a range of
    exponents, negative and positive, must come out as exactly +-448."""
    w = torch.zeros(16, 128)
    w[0, 0], w[1, 1], w[2, 2] = 3.0, -3.0, 1e-30
    q, s = R.quantize_weight(w)
    f = q.float()
    assert torch.isfinite(f).all() and f[0, 0] == 448 and f[1, 1] == -448 and f[2, 2] == 0
    g = torch.Generator().manual_seed(5)
    amax = torch.exp2(torch.rand(64, generator=g) * 60 - 30) * (1 + torch.rand(64, generator=g))
    big = torch.zeros(64 * 128, 128)
    big[::128, 0] = amax                        # one block per amax
    big[1::128, 1] = -amax
    qb, sb = R.quantize_weight(big)
    fb = qb.float()
    assert torch.isfinite(fb).all()
    assert torch.all(fb[::128, 0] == 448) and torch.all(fb[1::128, 1] == -448)
    assert torch.equal(sb[:, 0], amax / 448)
    with pytest.raises(ValueError, match="multiple of 16"):
        R.group_scales(torch.ones(24, 1))
    with pytest.raises(ValueError, match="scales"):
        R.dequantize_weight(q, torch.ones(2, 1), torch.float32)


def test_fused_scales_follow_the_weight_rows():
    """wqkv (K rows starting mid-block) and the interleaved w_gu: the [N/16, KB] scales are the
    checkpoint's block scales, expanded per row, pushed through the rows' own permutation."""
    torch.manual_seed(1)
    cfg = replace(get_config("llama-tiny"), hidden_size=192, num_heads=3, num_kv_heads=1,
                  head_dim=48, intermediate_size=208, num_layers=1)
    shapes = W.stage_param_shapes(cfg, 0, 1, True, True)
    params = W.random_init(shapes, "cpu", torch.float32, seed=2, std=0.05)
    qp = W.quantize_params(cfg, params)
    assert qp["embed"].dtype == torch.float32 and "embed_scale" not in qp
    parts = [params["layers.0.wqkv"][a:b] for a, b in ((0, 144), (144, 192), (192, 240))]
    qs = [R.quantize_weight(p) for p in parts]
    rows = torch.cat([R.row_scales(s, p.shape[0]) for (_, s), p in zip(qs, parts)])
    assert torch.equal(qp["layers.0.wqkv_scale"], rows[::16])
    assert qp["layers.0.wqkv_scale"].shape == (15, 2)
    assert torch.equal(qp["layers.0.wqkv"].view(torch.uint8),
                       torch.cat([q.view(torch.uint8) for q, _ in qs]))
    # K's first rows (fused rows 144..) carry K's block (0, .) scale, not Q's block (1, .)
    assert torch.equal(qp["layers.0.wqkv_scale"][9], qs[1][1][0])
    g, u = R.split_gate_up(params["layers.0.w_gu"].t())
    (qg, sg), (qu, su) = R.quantize_weight(g.t()), R.quantize_weight(u.t())
    rows = R.interleave_gate_up(R.row_scales(sg, 208), R.row_scales(su, 208))
    assert torch.equal(qp["layers.0.w_gu_scale"], rows[::16])
    assert torch.equal(qp["layers.0.w_gu"].view(torch.uint8),
                       R.interleave_gate_up(qg.view(torch.uint8), qu.view(torch.uint8)))
    back = R.dequantize_weight(qp["layers.0.w_gu"], qp["layers.0.w_gu_scale"])
    assert torch.equal(back, R.interleave_gate_up(block_dequant(qg, sg), block_dequant(qu, su)))


# ----------------------------------------------------------------------------- HF import
QCFG = {"quant_method": "fp8", "fmt": "e4m3", "weight_block_size": [128, 128],
        "activation_scheme": "dynamic"}
PROJ = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
        "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def write_fp8_checkpoint(hm, path, skip=()):
    """Quantise the projections of the HF model ``hm`` in place (it then holds the dequantised
    fp32 weights) and write them the way the FP8 checkpoints ship: F8_E4M3 ``weight`` +
    F32 ``weight_scale_inv``; modules in ``skip`` stay as they are."""
    from safetensors.torch import save_file
    sd = {k: v.detach().clone().contiguous() for k, v in hm.state_dict().items()}
    with torch.no_grad():
        for name, mod in hm.named_modules():
            if not name.endswith(PROJ) or name.endswith(tuple(skip)):
                continue
            q, s = R.quantize_weight(mod.weight)
            mod.weight.copy_(block_dequant(q, s))
            sd[name + ".weight"] = q
            sd[name + ".weight_scale_inv"] = s
    path.mkdir(parents=True, exist_ok=True)
    save_file(sd, str(path / "model.safetensors"), metadata={"format": "pt"})
    c = json.loads(hm.config.to_json_string())
    c["quantization_config"] = dict(QCFG, **({"modules_to_not_convert": list(skip)} if skip
                                             else {}))
    (path / "config.json").write_text(json.dumps(c))


# hidden 192 and intermediate 208: no multiple of 128 (ceil blocks); 3 x 48 query rows: the K
# rows of wqkv start at row 144, inside the second 128-row block
TWIN = dict(hidden_size=192, num_heads=3, num_kv_heads=1, head_dim=48, intermediate_size=208,
            num_layers=2)


def _twin(kind):
    if kind == "llama":
        cfg = replace(get_config("llama-tiny"), **TWIN)
        torch.manual_seed(0)
        return cfg, hf_model(cfg)
    from test_qwen import hf_qwen
    cfg = replace(get_config("qwen3-tiny"), **TWIN)
    return cfg, hf_qwen(cfg)


def _hf_greedy(m, ids, max_length):
    with torch.no_grad():
        out = m.generate(torch.tensor([ids]), max_length=max_length, do_sample=False,
                         pad_token_id=0)
    return out[0].tolist()


@pytest.mark.parametrize("kind,skip", [("llama", ()), ("qwen3", ()),
                                       ("llama", ("self_attn.o_proj",))])
def test_load_hf_fp8_checkpoint(tmp_path, kind, skip):
    cfg, hm = _twin(kind)
    write_fp8_checkpoint(hm, tmp_path / "ck", skip)
    c2, params = load_hf_dir(tmp_path / "ck", dtype=torch.float32)
    assert (c2.hidden_size, c2.head_dim, c2.qk_norm) == (192, 48, kind == "qwen3")
    for i in range(2):
        for leaf in ("wqkv", "w_gu", "w_down"):
            assert params[f"layers.{i}.{leaf}"].dtype == F8
            assert params[f"layers.{i}.{leaf}_scale"].dtype == torch.float32
        assert params[f"layers.{i}.wqkv_scale"].shape == (15, 2)
        assert params[f"layers.{i}.w_down_scale"].shape == (12, 2)
        assert (params[f"layers.{i}.wo"].dtype == F8) == (not skip)
        assert (f"layers.{i}.wo_scale" in params) == (not skip)
    assert params["embed"].dtype == torch.float32 and params["lm_head"].dtype == torch.float32
    with torch.no_grad():
        ref = hm(torch.tensor([IDS])).logits[0, -1]
    ours = our_last_logits(c2, params, IDS)
    assert torch.allclose(ours, ref, atol=2e-4, rtol=1e-3), (ours - ref).abs().max()
    eng = LLMEngine(c2, device="cpu", params=params, dtype=torch.float32, max_batch=4,
                    max_model_len=64, num_blocks=32)
    assert eng.stats()["weight_dtype"] == "fp8"
    out = eng.generate([IDS], SamplingParams(max_length=20, do_sample=False, ignore_eos=True))
    assert IDS + out[0].output_ids == _hf_greedy(hm, IDS, 20)
    # an FP8 checkpoint sets the dtype by itself; a contradictory explicit bf16 is an error
    with pytest.raises(ValueError, match="bf16"):
        LLMEngine(c2, device="cpu", params=params, weight_dtype="bf16", max_batch=4,
                  max_model_len=64, num_blocks=32)


# ----------------------------------------------------------------------------- refusals
LLAMA_HF = {"model_type": "llama", "hidden_size": 256, "num_attention_heads": 4,
            "num_key_value_heads": 2, "num_hidden_layers": 2, "intermediate_size": 512,
            "vocab_size": 1024}


@pytest.mark.parametrize("patch,field", [
    ({"quant_method": "gptq"}, "quant_method"),
    ({"quant_method": "fbgemm_fp8"}, "quant_method"),
    ({"weight_block_size": [64, 64]}, "weight_block_size"),
    ({"weight_block_size": None}, "weight_block_size"),
    ({"activation_scheme": "static"}, "activation_scheme"),
    ({"fmt": "e5m2"}, "fmt")])
def test_config_from_hf_refuses_other_quantisation(patch, field):
    with pytest.raises(ValueError, match=field):
        config_from_hf(dict(LLAMA_HF, quantization_config=dict(QCFG, **patch)), "x")


def test_config_from_hf_accepts_the_fp8_block():
    q = dict(QCFG)
    del q["activation_scheme"], q["fmt"]
    for qc in (QCFG, q):
        c = config_from_hf(dict(LLAMA_HF, quantization_config=qc), "x")
        assert c.hidden_size == 256 and not c.is_moe


def test_config_from_hf_refuses_fp8_moe_and_gpt2():
    moe = dict(LLAMA_HF, model_type="mixtral", num_local_experts=4, quantization_config=QCFG)
    with pytest.raises(ValueError, match="num_experts"):
        config_from_hf(moe, "x")
    gpt2 = {"model_type": "gpt2", "n_embd": 64, "n_layer": 1, "n_head": 2, "vocab_size": 100,
            "quantization_config": QCFG}
    with pytest.raises(ValueError, match="gpt2"):
        config_from_hf(gpt2, "x")


def test_rows_not_a_multiple_of_16_are_refused_by_name():
    cfg = replace(get_config("llama-tiny"), hidden_size=128, num_heads=1, num_kv_heads=1,
                  head_dim=24, intermediate_size=64, num_layers=1)
    params = W.random_init(W.stage_param_shapes(cfg, 0, 1, True, True), "cpu", torch.float32)
    with pytest.raises(ValueError, match=r"layers\.0\.wqkv\[q\].*multiple of 16"):
        W.quantize_params(cfg, params)


KW = dict(device="cpu", max_batch=4, max_model_len=64, num_blocks=32)


def test_engine_refusals(monkeypatch):
    monkeypatch.delenv("WEIGHT_DTYPE", raising=False)
    with pytest.raises(ValueError, match="int4"):
        LLMEngine("llama-tiny", weight_dtype="int4", **KW)
    monkeypatch.setenv("WEIGHT_DTYPE", "fp4")
    with pytest.raises(ValueError, match="fp4"):
        LLMEngine("llama-tiny", **KW)
    monkeypatch.delenv("WEIGHT_DTYPE")
    with pytest.raises(ValueError, match="num_experts"):
        LLMEngine("mixtral-tiny", weight_dtype="fp8", **KW)
    with pytest.raises(ValueError, match="gpt2"):
        LLMEngine("gpt2-tiny", weight_dtype="fp8", **KW)


def test_shard_model_from_hf_refuses_fp8(tmp_path):
    from distributed_llm_inferencing_amd.shard.writer import main as shard_main
    cfg, hm = _twin("llama")
    write_fp8_checkpoint(hm, tmp_path / "hf")
    with pytest.raises(ValueError, match="FP8"):
        shard_main(["--model_name", "acme/llama8", "--num_shards", "2", "--output_dir",
                    str(tmp_path / "out"), "--from-hf", str(tmp_path / "hf")])


def test_tensor_parallel_refuses_fp8(monkeypatch):
    from distributed_llm_inferencing_amd.parallel.tensor import TensorParallelEngine, shard_param
    monkeypatch.delenv("WEIGHT_DTYPE", raising=False)
    with pytest.raises(ValueError, match="FP8"):
        TensorParallelEngine("llama-tiny", "cpu", weight_dtype="fp8")
    monkeypatch.setenv("WEIGHT_DTYPE", "fp8")
    with pytest.raises(ValueError, match="FP8"):
        TensorParallelEngine("llama-tiny", "cpu")
    cfg = get_config("llama-tiny")
    with pytest.raises(ValueError, match=r"layers\.0\.wo"):
        shard_param("layers.0.wo", torch.zeros(256, 256).to(F8), cfg, 0, 2)


def test_fp8_weight_object():
    q, s = R.quantize_weight(torch.randn(32, 200))
    w = ops.Fp8Weight(q, R.group_scales(R.row_scales(s, 32)))
    assert tuple(w.shape) == (32, 200) and w.dim() == 2 and w.device.type == "cpu"
    assert w.numel() == 6400 and w.element_size() == 1
    with pytest.raises(ValueError, match="scale"):
        ops.Fp8Weight(q, s)
    with pytest.raises(ValueError, match="float8"):
        ops.Fp8Weight(q.float(), s)
    x = torch.randn(3, 200).to(torch.bfloat16)
    assert torch.equal(ops.linear(x, w), R.linear(x, w.dequantize(torch.float32)))


# ----------------------------------------------------------------------------- engine
def _tokens(eng):
    sp = SamplingParams(max_new_tokens=10, temperature=0.0, ignore_eos=True)
    return [o.output_ids for o in eng.generate([IDS, IDS[:3]], sp)]


def test_engine_weight_dtype_argument_and_environment(monkeypatch):
    monkeypatch.delenv("WEIGHT_DTYPE", raising=False)
    base = LLMEngine("llama-tiny", seed=3, **KW)
    assert base.stats()["weight_dtype"] == "bf16" and base.memory_report()["weight_dtype"] == "bf16"
    eng = LLMEngine("llama-tiny", seed=3, weight_dtype="fp8", **KW)
    assert eng.stats()["weight_dtype"] == "fp8" and eng.memory_report()["weight_dtype"] == "fp8"
    assert eng.stats.snapshot()["weight_dtype"] == "fp8"
    p = eng.model.params
    assert p["layers.0.wqkv"].dtype == F8 and p["layers.0.wqkv_scale"].dtype == torch.float32
    assert p["embed"].dtype == torch.bfloat16 and p["layers.0.attn_norm"].dtype == torch.bfloat16
    assert isinstance(eng.model.layers[0]["w_gu"], ops.Fp8Weight)
    assert eng.model.param_bytes() < 0.75 * base.model.param_bytes()
    # the reference: the same engine on the fp32 reconstruction of the weights (R.linear)
    deq = {}
    for k, v in p.items():
        if not k.endswith("_scale"):
            deq[k] = R.dequantize_weight(v, p[k + "_scale"], torch.float32) if v.dtype == F8 else v
    ref = LLMEngine("llama-tiny", params=deq, **KW)
    assert ref.stats()["weight_dtype"] == "bf16"
    want = _tokens(ref)
    assert _tokens(eng) == want
    monkeypatch.setenv("WEIGHT_DTYPE", "fp8")
    env = LLMEngine("llama-tiny", seed=3, **KW)
    assert env.stats()["weight_dtype"] == "fp8" and _tokens(env) == want
    assert LLMEngine("llama-tiny", seed=3, weight_dtype="bf16", **KW).weight_dtype == "bf16"


def test_worker_settings_and_cli_pass_weight_dtype(monkeypatch):
    from distributed_llm_inferencing_amd.cli import node_commands
    from distributed_llm_inferencing_amd.config import Settings
    from distributed_llm_inferencing_amd.worker.server import WorkerState
    monkeypatch.delenv("WEIGHT_DTYPE", raising=False)
    assert WorkerState(Settings.from_env(), "cpu").engine_kwargs["weight_dtype"] is None
    monkeypatch.setenv("WEIGHT_DTYPE", "fp8")
    assert WorkerState(Settings.from_env(), "cpu").engine_kwargs["weight_dtype"] == "fp8"
    monkeypatch.setenv("WEIGHT_DTYPE", "int8")
    with pytest.raises(ValueError, match="WEIGHT_DTYPE"):
        Settings.from_env()
    monkeypatch.delenv("WEIGHT_DTYPE")
    cmd, _ = node_commands(1, weight_dtype="fp8")[0]
    assert cmd[cmd.index("--weight-dtype") + 1] == "fp8"
    assert "--weight-dtype" not in node_commands(1)[0][0]
