"""4-bit expert stacks (``ops.W4Experts``) without a GPU: the class, ``quantize_params`` of a
stack, the model's pairing, ``slice_experts``, the ``weight_dtype`` switch and the plan route."""
import pytest
import torch

from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.engine.llm_engine import LLMEngine
from distributed_llm_inferencing_amd.models import get_config
from distributed_llm_inferencing_amd.models import weights as W
from distributed_llm_inferencing_amd.ops import gemm as G
from distributed_llm_inferencing_amd.ops import reference as R

BF = torch.bfloat16
KW = dict(device="cpu", max_batch=2, max_model_len=32, num_blocks=16, use_graphs=False)
plan = lambda tile, splits=1: G.GemmPlan("dli", tile, splits)  # noqa: E731


def zeros(E=4, n=32, K=256):
    return torch.zeros(E, n, K // 2, dtype=torch.uint8), torch.zeros(E, n, K // 128,
                                                                      dtype=torch.int32)


@pytest.mark.parametrize("q,sz,match", [
    (zeros()[0][0], zeros()[1], "3-D uint8"), (zeros()[0].int(), zeros()[1], "3-D uint8"),
    (zeros(K=192)[0], zeros()[1], "multiple of 128"), (zeros()[0], zeros()[1][:, :, :1], "sz"),
    (zeros()[0], zeros()[1][:3], "sz"), (zeros()[0], zeros()[1].float(), "sz")])
def test_shape_errors(q, sz, match):
    with pytest.raises(ValueError, match=match):
        ops.W4Experts(q, sz)


def test_quantize_params_round_trip_pairing_and_slices():
    cfg = get_config("qwen3-moe-tiny128", 1)
    base = W.random_init(W.stage_param_shapes(cfg, 0, 1, True, True), "cpu", BF, seed=3, std=0.05)
    p = W.quantize_params(cfg, base, "w4")
    E, D, F = cfg.num_experts, cfg.hidden_size, cfg.intermediate_size
    assert p["layers.0.router"].dtype == BF and W.params_weight_dtype(p) == "w4"
    for name, shape in (("layers.0.w_gu", (E, 2 * F, D)), ("layers.0.w_down", (E, D, F))):
        q, sz = p[name], p[name + "_sz"]
        assert q.dtype == torch.uint8 and q.shape == shape[:2] + (shape[2] // 2,)
        assert sz.dtype == torch.int32 and sz.shape == shape[:2] + (shape[2] // 128,)
        w = ops.W4Experts(q, sz)
        assert tuple(w.shape) == shape and w.dim() == 3 and G.wdt(w) == "w4"
        assert w.numel() == base[name].numel() and w.clone().to("cpu").act_dtype == BF
        for e in (0, E - 1):                   # every expert by itself, within one scale step
            one = ops.W4Weight(q[e], sz[e])
            assert torch.equal(w.dequantize()[e], one.dequantize())
            step = R.unpack_w4(q[e], sz[e])[1].float().repeat_interleave(128, 1)
            assert bool(((one.dequantize() - base[name][e].float()).abs() <= step).all())
        assert torch.equal(w.bf16(), w.dequantize(BF))
        # slice_experts cuts the sz words with the nibbles
        assert W._is_expert_tensor(name + "_sz")
        assert torch.equal(W.slice_experts(name + "_sz", sz, (4, 12)), sz[4:12])
        assert torch.equal(W.slice_experts(name, q, (4, 12)), q[4:12])
    lm = LLMEngine(cfg, params=p, **KW).model
    lp = lm._layer_params(0)
    assert isinstance(lp["w_gu"], ops.W4Experts) and isinstance(lp["w_down"], ops.W4Experts)
    assert isinstance(lp["wqkv"], ops.W4Weight) and "w_gu_sz" not in lp


def test_weight_dtype_switch():
    eng = LLMEngine("qwen3-moe-tiny128", weight_dtype="w4", **KW)
    assert eng.stats()["weight_dtype"] == "w4"
    assert isinstance(eng.model.layers[0]["w_down"], ops.W4Experts)
    with pytest.raises(ValueError, match=r"w_down\[0\].*multiple"):       # F = 64
        LLMEngine("qwen3-moe-tiny", weight_dtype="w4", **KW)


def test_plan_route():
    saved = dict(G._grouped_cache)
    G._grouped_cache.clear()
    try:
        w, x = ops.W4Experts(*zeros()), torch.zeros(4, 32, 256, dtype=BF)
        args = (8, 8, 32, 256, "silu_mul", 4, 16)
        assert G.grouped_plan(8, 32, 256, "silu_mul", 4, "w4") == plan(G.W4_GROUPED_DEFAULT_TILE)
        assert ops._expert_plan(w, *args, True) == (plan(74), True)
        # the form or the shape does not allow it: the bf16 plan, never a stream tile
        for ww, ok in ((w, False), (ops.W4Experts(*zeros(n=48)), True)):
            p, st = ops._expert_plan(ww, 8, 8, ww.shape[1], 256, "silu_mul", 4, 16, ok)
            assert not st and p == G.grouped_plan(8, ww.shape[1], 256, "silu_mul", 4)
        assert w.stream_ok(8, 4, plan(75)) and not w.stream_ok(8, 4, plan(74, 2))
        assert not w.stream_ok(8, 4, plan(70)) and not w.stream_ok(8, 3, plan(74))
        # a stream tile on a stack of another class names the tile and the class
        for wd, tile, stack, match in (("w4", 70, w, "tile 70.*W4Experts"),
                                       (None, 74, x, "tile 74.*W4Experts.*bfloat16"),
                                       (None, 70, x, "tile 70.*Fp8Experts.*bfloat16")):
            G._grouped_cache[G._grouped_key(8, 32, 256, "silu_mul", 4, wd)] = plan(tile)
            with pytest.raises(ValueError, match=match):
                ops._expert_plan(stack, *args, True)
    finally:
        G._grouped_cache.clear()
        G._grouped_cache.update(saved)
