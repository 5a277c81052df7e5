"""Weight naming, random init, HF-layout conversion and per-stage selection.

Our in-memory layout (all [out, in] row-major like torch Linear, bf16):

llama / mixtral (per layer ``layers.{i}.``):
    attn_norm [D], wqkv [(Hq+2Hkv)*hd, D], wo [D, Hq*hd], mlp_norm [D],
    (qk_norm, Qwen3) q_norm [hd], k_norm [hd]; (qkv_bias, Qwen2) bqkv [(Hq+2Hkv)*hd]
    dense: w_gu [2F, D] (16-row gate/up interleave, see ops/reference.py), w_down [D, F]
    FP8 weights (llama family): wqkv / wo / w_gu / w_down may be float8_e4m3fn,
    each with a fp32 ``<name>_scale`` [N/16, ceil(K/128)] beside it (ops/reference.py
    ``dequantize_weight``); ``TransformerLM`` pairs the two into an ``ops.Fp8Weight``
    moe:   router [E, D], w_gu [E, 2F, D], w_down [E, D, F]
    FP8 expert stacks: w_gu / w_down float8_e4m3fn with ``<name>_scale`` [E, N/16, ceil(K/128)]
    (every expert quantised by itself), paired into an ``ops.Fp8Experts``; the router is bf16
gpt2 (per layer): ln1_w, ln1_b, wqkv [3D, D], bqkv [3D], wo [D, D], bo [D], ln2_w, ln2_b,
    w_fc [F, D], b_fc [F], w_proj [D, F], b_proj [D]
globals: embed [V, D], (gpt2) pos_embed [P, D], final_norm [D], (gpt2) final_norm_b [D],
    lm_head [V, D] (absent when tied to embed)

Random init mirrors HF ``_init_weights`` (normal(0, 0.02), norms = 1, biases = 0) and is
generated directly on the target device, per stage, so a 70B stage never materialises the
full model anywhere.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional

import torch

from .configs import ModelConfig
from ..ops import reference as R
from ..ops.reference import interleave_gate_up

INIT_STD = 0.02


def layer_param_shapes(cfg: ModelConfig, i: int) -> Dict[str, tuple]:
    d, f, hd = cfg.hidden_size, cfg.intermediate_size, cfg.head_dim
    p = f"layers.{i}."
    if cfg.arch == "gpt2":
        return {p + "ln1_w": (d,), p + "ln1_b": (d,), p + "wqkv": (3 * d, d), p + "bqkv": (3 * d,),
                p + "wo": (d, d), p + "bo": (d,), p + "ln2_w": (d,), p + "ln2_b": (d,),
                p + "w_fc": (f, d), p + "b_fc": (f,), p + "w_proj": (d, f), p + "b_proj": (d,)}
    s = {p + "attn_norm": (d,), p + "wqkv": (cfg.qkv_size, d), p + "wo": (d, cfg.q_size),
         p + "mlp_norm": (d,)}
    if cfg.qk_norm:
        s.update({p + "q_norm": (hd,), p + "k_norm": (hd,)})
    if cfg.qkv_bias:
        s[p + "bqkv"] = (cfg.qkv_size,)
    if cfg.is_moe:
        e = cfg.num_experts
        s.update({p + "router": (e, d), p + "w_gu": (e, 2 * f, d), p + "w_down": (e, d, f)})
    else:
        s.update({p + "w_gu": (2 * f, d), p + "w_down": (d, f)})
    return s


def global_param_shapes(cfg: ModelConfig, first: bool, last: bool) -> Dict[str, tuple]:
    d, v = cfg.hidden_size, cfg.vocab_size
    s: Dict[str, tuple] = {}
    if first or (last and cfg.tie_embeddings):
        s["embed"] = (v, d)
    if first and cfg.arch == "gpt2":
        s["pos_embed"] = (cfg.max_position, d)
    if last:
        s["final_norm"] = (d,)
        if cfg.arch == "gpt2":
            s["final_norm_b"] = (d,)
        if not cfg.tie_embeddings:
            s["lm_head"] = (v, d)
    return s


def stage_param_shapes(cfg: ModelConfig, layer_start: int, layer_end: int, first: bool,
                       last: bool, expert_range: Optional[tuple] = None) -> Dict[str, tuple]:
    s = global_param_shapes(cfg, first, last)
    for i in range(layer_start, layer_end):
        ls = layer_param_shapes(cfg, i)
        if expert_range is not None and cfg.is_moe:
            e0, e1 = expert_range
            for k in list(ls):
                if k.endswith(".w_gu") or k.endswith(".w_down"):
                    ls[k] = (e1 - e0,) + tuple(ls[k][1:])
        s.update(ls)
    return s


def _is_norm_weight(name: str) -> bool:
    return name.endswith(("attn_norm", "mlp_norm", "final_norm", "ln1_w", "ln2_w", ".q_norm",
                          ".k_norm"))


def _is_bias(name: str) -> bool:
    return name.endswith(("ln1_b", "ln2_b", "bqkv", "bo", "b_fc", "b_proj", "final_norm_b"))


def random_init(shapes: Dict[str, tuple], device, dtype=torch.bfloat16, seed: int = 0,
                std: float = INIT_STD) -> Dict[str, torch.Tensor]:
    """Deterministic per-tensor init: each tensor's values depend only on (seed, name), so a
    pipeline stage generates exactly the slice the full model would hold."""
    out = {}
    dev = torch.device(device)
    for name in sorted(shapes):
        shape = shapes[name]
        if _is_norm_weight(name):
            out[name] = torch.ones(shape, dtype=dtype, device=dev)
        elif _is_bias(name):
            out[name] = torch.zeros(shape, dtype=dtype, device=dev)
        else:
            g = torch.Generator(device=dev)
            g.manual_seed((seed * 1_000_003 + _name_hash(name)) & 0x7FFF_FFFF_FFFF)
            t = torch.empty(shape, dtype=dtype, device=dev)
            t.normal_(0.0, std, generator=g)
            out[name] = t
    return out


def _is_expert_tensor(name: str) -> bool:
    """An expert stack or the FP8 scales that go with it."""
    return name.endswith((".w_gu", ".w_down", ".w_gu_scale", ".w_down_scale"))


def slice_experts(name: str, t: torch.Tensor, expert_range: Optional[tuple]) -> torch.Tensor:
    if expert_range is None or not _is_expert_tensor(name):
        return t
    if t.dim() != 3:
        return t
    if expert_range[0] == 0 and expert_range[1] == t.shape[0]:
        return t
    # a copy: a leading-dim slice is already contiguous, so .contiguous() would return a
    # view that keeps every expert's storage alive (each EP rank held all 8 experts)
    return t[expert_range[0]:expert_range[1]].clone()


def _name_hash(name: str) -> int:
    h = 1469598103934665603
    for ch in name.encode():
        h ^= ch
        h = (h * 1099511628211) & 0xFFFF_FFFF_FFFF_FFFF
    return h


def nbytes(params: Dict[str, torch.Tensor]) -> int:
    return sum(t.numel() * t.element_size() for t in params.values())


# ----------------------------------------------------------------------------- FP8 weights
WEIGHT_DTYPES = ("bf16", "fp8")
FP8_PROJECTIONS = ("wqkv", "wo", "w_gu", "w_down")


def resolve_weight_dtype(weight_dtype: Optional[str] = None) -> Optional[str]:
    """``"bf16"`` | ``"fp8"`` from the argument or, without one, the environment variable
    ``WEIGHT_DTYPE``; None when neither names one (the weights stay as they come). Anything
    else is an error."""
    import os
    v = os.environ.get("WEIGHT_DTYPE", "") if weight_dtype is None else weight_dtype
    v = str(v).strip().lower()
    if not v:
        return None
    if v not in WEIGHT_DTYPES:
        raise ValueError(f"weight_dtype {v!r}: expected one of {WEIGHT_DTYPES}")
    return v


def is_fp8(params: Dict[str, torch.Tensor]) -> bool:
    return any(t.dtype == R.FP8_W for t in params.values())


def fp8_scratch_bytes(cfg: ModelConfig, experts: Optional[int] = None) -> int:
    """Bytes of the bf16 scratch a model with FP8 projections reserves: its largest one; for
    a MoE model the largest expert stack (``experts``: the local experts of an expert-parallel
    rank, default all), which the dequantise path rewrites whole."""
    d, f = cfg.hidden_size, cfg.intermediate_size
    mlp = 2 * f * d * ((cfg.num_experts if experts is None else experts) if cfg.is_moe else 1)
    return 2 * max(cfg.qkv_size * d, d * cfg.q_size, mlp)


def check_fp8_model(cfg: ModelConfig) -> None:
    """FP8 weights exist for the llama-family layers, dense and MoE."""
    if cfg.arch == "gpt2":
        raise ValueError(f"{cfg.name}: weight_dtype fp8 is not available for gpt2 (arch) models")


def apply_weight_dtype(model, want: Optional[str]) -> None:
    """Bring a ``TransformerLM`` to the asked weight dtype (``resolve_weight_dtype``): "fp8"
    quantises a bf16 model's projections (refused for gpt2, and among the MoE models for all
    but Qwen3-MoE: a Mixtral holds FP8 experts only where its parameters come quantised,
    ``quantize_params``); an FP8 checkpoint sets the dtype by itself, and an explicit "bf16"
    for one is an error, not a silent dequantise."""
    have = model.weight_dtype
    if want == "fp8":
        check_fp8_model(model.cfg)
        cfg = model.cfg
        if cfg.is_moe and not cfg.qk_norm and have != "fp8":
            raise ValueError(f"{cfg.name}: weight_dtype fp8 with num_experts={cfg.num_experts}: "
                             "the switch quantises the experts of Qwen3-MoE models only")
        if have != "fp8":
            model.quantize_fp8()
    elif want == "bf16" and have == "fp8":
        raise ValueError(f"{model.cfg.name}: weight_dtype bf16 was asked for, but the loaded "
                         "weights are FP8 (float8_e4m3fn projections with scales); they are "
                         "not dequantised silently")


def _u8(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.uint8) if t.dtype == R.FP8_W else t


def _fuse(parts, names, fuse):
    """``parts``: [(q [n, K] e4m3fn, block scales [ceil(n/128), KB])] of the unfused tensors
    ``names``; ``fuse``: what turns their rows into the fused weight's (``torch.cat`` /
    ``interleave_gate_up``). The scales take the same path row by row. Returns (q, scale in
    the [N/16, KB] layout)."""
    for (q, _), name in zip(parts, names):
        if q.shape[0] % R.W_SCALE_ROWS:
            raise ValueError(f"{name}: {q.shape[0]} rows, not a multiple of "
                             f"{R.W_SCALE_ROWS}: its FP8 block scales cannot follow the rows "
                             "into the fused weight")
    q = fuse([_u8(q) for q, _ in parts]).contiguous().view(R.FP8_W)
    rows = fuse([R.row_scales(s.to(q.device), pq.shape[0]) for pq, s in parts])
    return q, R.group_scales(rows)


def _stack_fp8(qs):
    return torch.stack([_u8(q) for q in qs]).view(R.FP8_W)


def _cat(ts):
    return torch.cat(ts, 0) if len(ts) > 1 else ts[0]


def _interleave(ts):
    return interleave_gate_up(ts[0], ts[1])


def _quantize_proj(w: torch.Tensor, leaf: str, name: str):
    """(q, scale [N/16, KB]) of one 2-D ``w_gu`` (gate and up quantised apart, per 128 x 128
    block of the unfused tensors) or any other projection."""
    if leaf == "w_gu":
        g, u = R.split_gate_up(w.t())            # rows are the interleaved axis
        parts = [R.quantize_weight(g.t()), R.quantize_weight(u.t())]
        return _fuse(parts, [name + "[gate]", name + "[up]"], _interleave)
    return _fuse([R.quantize_weight(w)], [name], _cat)


def quantize_params(cfg: ModelConfig, params: Dict[str, torch.Tensor],
                    inplace: bool = False) -> Dict[str, torch.Tensor]:
    """The four projections of every llama-family layer in ``params`` as FP8 block-scaled
    weights (``reference.quantize_weight`` of each unfused tensor: q / k / v, o, gate / up,
    down; of a MoE layer every expert's gate / up / down, the router stays bf16); everything
    else as it is. Returns a new dict, or with ``inplace`` ``params`` itself,
    each bf16 tensor replaced as soon as it is quantised (a caller that holds no other
    reference then never has the bf16 and the FP8 model in memory together)."""
    check_fp8_model(cfg)
    out = params if inplace else dict(params)
    hq, hkv, hd = cfg.num_heads, cfg.num_kv_heads, cfg.head_dim
    for name in [k for k in params if k.rsplit(".", 1)[-1] in FP8_PROJECTIONS]:
        w = params[name]
        if w.dtype == R.FP8_W:
            continue
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "wqkv":
            cuts = [("q", 0, hq * hd), ("k", hq * hd, (hq + hkv) * hd),
                    ("v", (hq + hkv) * hd, (hq + 2 * hkv) * hd)]
            parts = [R.quantize_weight(w[a:b]) for _, a, b in cuts]
            q, s = _fuse(parts, [f"{name}[{n}]" for n, _, _ in cuts], _cat)
        elif w.dim() == 3:                       # an expert stack: every expert by itself
            qs = [_quantize_proj(w[e], leaf, f"{name}[{e}]") for e in range(w.shape[0])]
            q, s = _stack_fp8([a for a, _ in qs]), torch.stack([b for _, b in qs])
            del qs
        elif leaf == "w_gu":
            q, s = _quantize_proj(w, leaf, name)
        else:
            parts = [R.quantize_weight(w)]
            q, s = _fuse(parts, [name], _cat)
        out[name], out[name + "_scale"] = q, s
        del w
    return out


# ----------------------------------------------------------------------------- HF conversion
def _hf_proj(sd, keys, name: str, fuse, cv):
    """One (possibly fused) projection from the HF tensors ``keys``: {name: bf16 weight}, or,
    when the checkpoint holds ``<key>_scale_inv`` for them (an FP8 block-quantised module;
    modules it left unconverted have none), {name: e4m3fn weight, name_scale: fp32 scales}."""
    has = [k + "_scale_inv" in sd for k in keys]
    if not any(has):
        return {name: cv(fuse([sd[k] for k in keys]))}
    if not all(has):
        raise ValueError(f"{name}: {[k for k, h in zip(keys, has) if not h]} lack "
                         "weight_scale_inv while the tensors fused with them have one")
    parts = []
    for k in keys:
        q, s = sd[k], sd[k + "_scale_inv"]
        if q.dtype != R.FP8_W:
            raise ValueError(f"{k}: has a weight_scale_inv but dtype {q.dtype}, expected "
                             "float8_e4m3fn")
        want = (-(-q.shape[0] // R.W_BLOCK), -(-q.shape[1] // R.W_BLOCK))
        if tuple(s.shape) != want:
            raise ValueError(f"{k}_scale_inv: shape {tuple(s.shape)}, expected {want} "
                             "(128 x 128 blocks)")
        parts.append((q.detach(), s.detach().float()))
    q, s = _fuse(parts, keys, fuse)
    return {name: q, name + "_scale": s}


def from_hf_state_dict(cfg: ModelConfig, sd: Dict[str, torch.Tensor],
                       layers: Optional[Iterable[int]] = None, first: bool = True,
                       last: bool = True, dtype=torch.bfloat16) -> Dict[str, torch.Tensor]:
    """Convert a HF LlamaForCausalLM / MixtralForCausalLM / GPT2LMHeadModel state dict."""
    layers = range(cfg.num_layers) if layers is None else layers
    out: Dict[str, torch.Tensor] = {}
    cv = lambda t: t.detach().to(dtype).contiguous()  # noqa: E731
    if cfg.arch == "gpt2":
        pre = "transformer."
        if first or (last and cfg.tie_embeddings):
            out["embed"] = cv(sd[pre + "wte.weight"])
        if first:
            out["pos_embed"] = cv(sd[pre + "wpe.weight"])
        if last:
            out["final_norm"] = cv(sd[pre + "ln_f.weight"])
            out["final_norm_b"] = cv(sd[pre + "ln_f.bias"])
        for i in layers:
            h = f"{pre}h.{i}."
            p = f"layers.{i}."
            # HF GPT-2 Conv1D stores [in, out]; ours is [out, in]
            out[p + "ln1_w"] = cv(sd[h + "ln_1.weight"]); out[p + "ln1_b"] = cv(sd[h + "ln_1.bias"])
            out[p + "wqkv"] = cv(sd[h + "attn.c_attn.weight"].t()); out[p + "bqkv"] = cv(sd[h + "attn.c_attn.bias"])
            out[p + "wo"] = cv(sd[h + "attn.c_proj.weight"].t()); out[p + "bo"] = cv(sd[h + "attn.c_proj.bias"])
            out[p + "ln2_w"] = cv(sd[h + "ln_2.weight"]); out[p + "ln2_b"] = cv(sd[h + "ln_2.bias"])
            out[p + "w_fc"] = cv(sd[h + "mlp.c_fc.weight"].t()); out[p + "b_fc"] = cv(sd[h + "mlp.c_fc.bias"])
            out[p + "w_proj"] = cv(sd[h + "mlp.c_proj.weight"].t()); out[p + "b_proj"] = cv(sd[h + "mlp.c_proj.bias"])
        return out
    if first:
        out["embed"] = cv(sd["model.embed_tokens.weight"])
    if last:
        out["final_norm"] = cv(sd["model.norm.weight"])
        if cfg.tie_embeddings:
            out["embed"] = cv(sd["model.embed_tokens.weight"])
        else:
            out["lm_head"] = cv(sd["lm_head.weight"])
    for i in layers:
        h = f"model.layers.{i}."
        p = f"layers.{i}."
        out[p + "attn_norm"] = cv(sd[h + "input_layernorm.weight"])
        out[p + "mlp_norm"] = cv(sd[h + "post_attention_layernorm.weight"])
        out.update(_hf_proj(sd, [h + f"self_attn.{n}_proj.weight" for n in "qkv"],
                            p + "wqkv", _cat, cv))
        out.update(_hf_proj(sd, [h + "self_attn.o_proj.weight"], p + "wo", _cat, cv))
        if cfg.qk_norm:                          # Qwen3: per-head q/k RMSNorm weights [hd]
            out[p + "q_norm"] = cv(sd[h + "self_attn.q_norm.weight"])
            out[p + "k_norm"] = cv(sd[h + "self_attn.k_norm.weight"])
        if cfg.qkv_bias:                         # Qwen2: biases of q/k/v, in wqkv's row order
            out[p + "bqkv"] = cv(torch.cat([sd[h + "self_attn.q_proj.bias"],
                                            sd[h + "self_attn.k_proj.bias"],
                                            sd[h + "self_attn.v_proj.bias"]], 0))
        if cfg.is_moe:
            moe = h + "block_sparse_moe."
            if moe + "gate.weight" not in sd:
                moe = h + "mlp."
            out[p + "router"] = cv(sd[moe + "gate.weight"])
            gus, downs = [], []
            if moe + "experts.gate_up_proj" in sd:
                for t in ("gate_up_proj", "down_proj"):
                    for suf in ("_scale_inv", ".weight_scale_inv"):
                        if moe + "experts." + t + suf in sd:
                            raise ValueError(
                                f"{moe}experts.{t}{suf}: the fused expert layout with FP8 "
                                "block scales is not supported (FP8 experts are read from the "
                                "per-expert experts.{e}.{gate,up,down}_proj tensors)")
                # fused expert tensors (transformers >= 5 MixtralExperts):
                # gate_up_proj [E, 2F, D] (gate rows then up rows), down_proj [E, D, F]
                gu = sd[moe + "experts.gate_up_proj"]
                dn = sd[moe + "experts.down_proj"]
                f = cfg.intermediate_size
                gus = [interleave_gate_up(gu[e, :f], gu[e, f:]) for e in range(cfg.num_experts)]
                downs = [dn[e] for e in range(cfg.num_experts)]
            else:
                for e in range(cfg.num_experts):
                    ex = f"{moe}experts.{e}."
                    if ex + "w1.weight" in sd:   # original Mixtral naming (w1 gate, w3 up, w2 down)
                        kg, ku, kd = ex + "w1.weight", ex + "w3.weight", ex + "w2.weight"
                    else:
                        kg, ku, kd = (ex + "gate_proj.weight", ex + "up_proj.weight",
                                      ex + "down_proj.weight")
                    # _hf_proj's rule per expert: FP8 iff its weight_scale_inv is there
                    gus.append(_hf_proj(sd, [kg, ku], "gu", _interleave, lambda t: t.detach()))
                    downs.append(_hf_proj(sd, [kd], "dn", _cat, lambda t: t.detach()))
                for stack, leaf in ((gus, "gu"), (downs, "dn")):
                    quant = [leaf + "_scale" in d for d in stack]
                    if any(quant) and not all(quant):
                        e = quant.index(False)
                        part = "gate_proj" if leaf == "gu" else "down_proj"
                        raise ValueError(
                            f"{moe}experts.{e}.{part}.weight: no weight_scale_inv, while other "
                            f"experts of layer {i} are FP8: a layer's experts must be quantised "
                            "all or none")
                if "gu_scale" in gus[0]:
                    out[p + "w_gu_scale"] = torch.stack([d["gu_scale"] for d in gus])
                    gus = [_u8(d["gu"]) for d in gus]
                else:
                    gus = [d["gu"] for d in gus]
                if "dn_scale" in downs[0]:
                    out[p + "w_down_scale"] = torch.stack([d["dn_scale"] for d in downs])
                    downs = [_u8(d["dn"]) for d in downs]
                else:
                    downs = [d["dn"] for d in downs]
            if (p + "w_gu_scale" in out) != (p + "w_down_scale" in out):
                bf = "down_proj" if p + "w_gu_scale" in out else "gate_proj"
                raise ValueError(
                    f"{moe}experts.0.{bf}.weight: no weight_scale_inv, while the layer's other "
                    "expert projections are FP8: a layer's experts must be quantised all or "
                    "none")
            fp8cv = lambda t: t.contiguous().view(R.FP8_W)  # noqa: E731
            out[p + "w_gu"] = (fp8cv if p + "w_gu_scale" in out else cv)(torch.stack(gus))
            out[p + "w_down"] = (fp8cv if p + "w_down_scale" in out else cv)(torch.stack(downs))
        else:
            out.update(_hf_proj(sd, [h + "mlp.gate_proj.weight", h + "mlp.up_proj.weight"],
                                p + "w_gu", _interleave, cv))
            out.update(_hf_proj(sd, [h + "mlp.down_proj.weight"], p + "w_down", _cat, cv))
    return out
