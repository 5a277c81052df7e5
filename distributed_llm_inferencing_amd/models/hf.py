"""HF checkpoint import: ``save_pretrained`` directories (and hub-cache snapshots) of
LlamaForCausalLM / MistralForCausalLM / MixtralForCausalLM / Qwen2ForCausalLM /
Qwen3ForCausalLM / Qwen3MoeForCausalLM / GPT2LMHeadModel.

The reference loads checkpoints with ``AutoModelForCausalLM.from_pretrained(model_name,
cache_dir=MODEL_CACHE_DIR)`` (``worker/app.py:117-124``) and its sharder shards a loaded HF
model (``master/dashboard/management/commands/shard_model.py:37,55-96``). Here a checkpoint
directory is read without transformers at run time:

* ``config.json`` -> ``ModelConfig`` (``config_from_hf``);
* ``model.safetensors`` or ``model.safetensors.index.json`` + its shard files, read tensor by
  tensor through the C++ safetensors loader (mmap, no pickle) as ``from_hf_state_dict`` asks
  for them, so host memory holds the converted stage, not the checkpoint twice;
* ``layers`` / ``first`` / ``last`` select one pipeline stage's tensors (``shard-model
  --from-hf``, or a worker loading only its stage).

Directory forms accepted by ``find_hf_dir``: the directory itself, ``<root>/<name with / ->
_>/``, and the HF hub cache layout ``<root>/models--<org>--<name>/snapshots/<rev>/``.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Dict, Iterable, Iterator, Optional, Tuple

import torch

from .configs import ModelConfig
from .weights import from_hf_state_dict


def is_hf_dir(d) -> bool:
    d = Path(d)
    cj = d / "config.json"
    if not cj.exists():
        return False
    try:
        c = json.loads(cj.read_text())
    except (OSError, ValueError):
        return False
    return "model_type" in c and ((d / "model.safetensors").exists()
                                  or (d / "model.safetensors.index.json").exists())


def find_hf_dir(root: str, name: str) -> Optional[Path]:
    """The HF checkpoint directory of ``name`` under ``root`` (see module docstring)."""
    r = Path(root)
    cands = [r / name.replace("/", "_"), r / name]
    hub = r / ("models--" + name.replace("/", "--"))
    snaps = hub / "snapshots"
    if snaps.is_dir():
        ref = hub / "refs" / "main"
        if ref.exists():
            cands.append(snaps / ref.read_text().strip())
        cands += sorted(snaps.iterdir(), key=lambda p: p.stat().st_mtime, reverse=True)
    for c in cands:
        if c.is_dir() and is_hf_dir(c):
            return c
    return None


def hf_weight_dtype(c: dict) -> str:
    """``fp8`` for a checkpoint whose ``quantization_config`` is the one block this engine
    reads — ``quant_method`` "fp8", e4m3 where a format is stated, ``weight_block_size``
    [128, 128], ``activation_scheme`` "dynamic" or absent (activations are never quantised
    here, so the scheme changes nothing) — ``bf16`` without the block, and an error naming
    the field for anything else."""
    qc = c.get("quantization_config")
    if not qc:
        return "bf16"
    if qc.get("quant_method") != "fp8":
        raise ValueError(f"quantization_config.quant_method={qc.get('quant_method')!r}: only "
                         "'fp8' (128 x 128 block-scaled e4m3 weights) is supported")
    fmt = qc.get("fmt", qc.get("format"))
    if fmt is not None and "e4m3" not in str(fmt).lower():
        raise ValueError(f"quantization_config.fmt={fmt!r}: only e4m3 is supported")
    bs = qc.get("weight_block_size")
    if bs is None or list(bs) != [128, 128]:
        raise ValueError(f"quantization_config.weight_block_size={bs!r}: only [128, 128] is "
                         "supported")
    act = qc.get("activation_scheme")
    if act not in (None, "dynamic"):
        raise ValueError(f"quantization_config.activation_scheme={act!r}: only 'dynamic' "
                         "(activations stay bf16 here) is supported")
    return "fp8"


def config_from_hf(c: dict, name: Optional[str] = None,
                   sliding_window: bool = False) -> ModelConfig:
    """Map a HF ``config.json`` (llama / mistral / mixtral / qwen2 / qwen3 / qwen3_moe / gpt2
    model types; qwen3 and qwen3_moe set ``qk_norm``, qwen2 — and a qwen3 / qwen3_moe with
    ``attention_bias`` — ``qkv_bias``). qwen3_moe: every layer sparse, no shared expert; the
    expert width is ``moe_intermediate_size`` and an absent ``norm_topk_prob`` means false.
    ``sliding_window``: the caller runs the model through ``TransformerLM``, whose attention
    honours ``ModelConfig.sliding_window``: a checkpoint's window (smaller than its
    ``max_position_embeddings``) is kept and the context is the model's own. Without it the
    result describes a full-attention model, so the context is capped at the window."""
    mt = c.get("model_type", "")
    name = name or c.get("_name_or_path") or mt
    fp8 = hf_weight_dtype(c) == "fp8"
    if fp8 and mt == "gpt2":
        raise ValueError("quantization_config (fp8) with model_type gpt2: FP8 weights exist "
                         "for the llama family only")
    if mt == "gpt2":
        d = int(c["n_embd"])
        return ModelConfig(
            name=name, arch="gpt2", hidden_size=d, num_layers=int(c["n_layer"]),
            num_heads=int(c["n_head"]), num_kv_heads=int(c["n_head"]),
            head_dim=d // int(c["n_head"]), intermediate_size=int(c.get("n_inner") or 4 * d),
            vocab_size=int(c["vocab_size"]), max_position=int(c.get("n_positions", 1024)),
            rope_theta=0.0, norm_eps=float(c.get("layer_norm_epsilon", 1e-5)),
            tie_embeddings=True, bos_token_id=int(c.get("bos_token_id", 50256)),
            eos_token_id=_eos(c, 50256))
    if mt not in ("llama", "mistral", "mixtral", "qwen2", "qwen3", "qwen3_moe"):
        raise ValueError(f"unsupported HF model_type '{mt}' "
                         "(llama, mistral, mixtral, qwen2, qwen3, qwen3_moe, gpt2)")
    qwen = mt in ("qwen2", "qwen3", "qwen3_moe")
    if qwen and c.get("use_sliding_window"):
        raise ValueError(
            f"{mt} checkpoint with use_sliding_window=true: it windows only some of its layers "
            "(max_window_layers / layer_types), and this engine applies one window to every "
            "layer")
    experts, inter, norm_topk = 0, c.get("intermediate_size"), True
    if mt == "mixtral":
        experts = int(c.get("num_local_experts", 0))
    elif mt == "qwen3_moe":
        # this engine runs one kind of layer: every layer sparse, routed experts only
        if c.get("mlp_only_layers"):
            raise ValueError(f"qwen3_moe checkpoint with mlp_only_layers={c['mlp_only_layers']}: "
                             "dense and sparse layers cannot be mixed")
        if int(c.get("decoder_sparse_step", 1)) != 1:
            raise ValueError(f"qwen3_moe checkpoint with decoder_sparse_step="
                             f"{c['decoder_sparse_step']}: every layer must be sparse (1)")
        for f in ("shared_expert_intermediate_size", "num_shared_experts"):
            if c.get(f):
                raise ValueError(f"qwen3_moe checkpoint with {f}={c[f]}: shared experts "
                                 "(Qwen2-MoE) are not supported")
        experts = int(c.get("num_experts") or c.get("num_local_experts") or 0)
        if experts <= 0:
            raise ValueError("qwen3_moe checkpoint without num_experts")
        inter = c["moe_intermediate_size"]
        norm_topk = bool(c.get("norm_topk_prob", False))
    if fp8 and mt == "mixtral":
        raise ValueError(f"quantization_config (fp8) with model_type mixtral (num_experts="
                         f"{experts}): FP8 expert checkpoints are read in the per-expert "
                         "qwen3_moe layout only; no block-scaled Mixtral export is known")
    d, nh = int(c["hidden_size"]), int(c["num_attention_heads"])
    rope = c.get("rope_theta")
    params = c.get("rope_parameters") or {}
    if rope is None:
        rope = params.get("rope_theta", 10000.0)
    # rope scaling (Llama-3.1 / 3.2 "llama3", "linear"): absorbed into the cos/sin table;
    # transformers 5 keeps it in rope_parameters, older configs in rope_scaling
    sc = dict(c.get("rope_scaling") or {})
    if not sc and params.get("rope_type", "default") not in ("default", None):
        sc = {k: v for k, v in params.items() if k != "rope_theta"}
    if sc:
        from ..ops.reference import rope_scaled_inv_freq
        import torch as _t
        rope_scaled_inv_freq(_t.ones(2, dtype=_t.float64), sc)     # refuse unknown types now
    max_pos = int(c.get("max_position_embeddings", 8192))
    # sliding-window attention (Mistral). A null window, or one the context never outgrows,
    # is full attention. A caller that does not opt in gets a full-attention config: full
    # attention equals the windowed one while a sequence fits the window, so the context is
    # capped there instead of silently diverging past it
    # Qwen configs carry a sliding_window value next to use_sliding_window=false: not a window
    sw = None if qwen else c.get("sliding_window")
    window = 0
    if sw and int(sw) < max_pos:
        if sliding_window:
            window = int(sw)
        else:
            import logging
            logging.getLogger(__name__).warning(
                "sliding_window=%s < max_position_embeddings=%s: context capped at the window "
                "(this caller did not ask for sliding-window attention; pass "
                "sliding_window=True to config_from_hf to serve the full context)", sw, max_pos)
            max_pos = int(sw)
    return ModelConfig(
        name=name, arch="llama", hidden_size=d, num_layers=int(c["num_hidden_layers"]),
        num_heads=nh, num_kv_heads=int(c.get("num_key_value_heads") or nh),
        head_dim=int(c.get("head_dim") or d // nh),
        intermediate_size=int(inter), vocab_size=int(c["vocab_size"]),
        max_position=max_pos, rope_theta=float(rope),
        rope_scaling=tuple(sorted((str(k), v) for k, v in sc.items()
                                  if isinstance(v, (int, float, str)))),
        norm_eps=float(c.get("rms_norm_eps", 1e-5)),
        num_experts=experts,
        top_k_experts=int(c.get("num_experts_per_tok", 2)),
        tie_embeddings=bool(c.get("tie_word_embeddings", False)),
        bos_token_id=int(c.get("bos_token_id") or 1), eos_token_id=_eos(c, 2),
        sliding_window=window, qk_norm=mt in ("qwen3", "qwen3_moe"),
        qkv_bias=mt == "qwen2" or (mt in ("qwen3", "qwen3_moe")
                                   and bool(c.get("attention_bias", False))),
        norm_topk_prob=norm_topk)


def _eos(c: dict, default: int) -> int:
    e = c.get("eos_token_id", default)
    if isinstance(e, list):
        e = e[0] if e else default
    return int(default if e is None else e)


class LazyStateDict:
    """Mapping over every tensor of a (possibly multi-file) safetensors checkpoint; a tensor
    is read from disk (C++ loader, to host memory) when it is first asked for."""

    def __init__(self, d: Path):
        from ..runtime import SafetensorsFile
        self.dir = Path(d)
        idx = self.dir / "model.safetensors.index.json"
        if idx.exists():
            wm = json.loads(idx.read_text())["weight_map"]
            files = sorted(set(wm.values()))
        else:
            files = ["model.safetensors"]
            wm = None
        self._files = {f: SafetensorsFile(str(self.dir / f)) for f in files}
        self._where: Dict[str, str] = {}
        for f, st in self._files.items():
            for k in st.keys():
                self._where[k] = f
        if wm is not None:
            missing = [k for k in wm if k not in self._where]
            if missing:
                raise ValueError(f"{idx}: {len(missing)} indexed tensors missing, e.g. "
                                 f"{missing[0]}")

    def __contains__(self, k) -> bool:
        return k in self._where

    def __getitem__(self, k) -> torch.Tensor:
        f = self._where[k]
        return self._files[f].load([k])[k]

    def keys(self) -> Iterator[str]:
        return iter(self._where)

    def close(self) -> None:
        for st in self._files.values():
            st.close()


def load_hf_dir(d, device="cpu", dtype=torch.bfloat16, name: Optional[str] = None,
                layers: Optional[Iterable[int]] = None, first: bool = True,
                last: bool = True) -> Tuple[ModelConfig, Dict[str, torch.Tensor]]:
    """(config, our parameter dict on ``device``) from a HF checkpoint directory; with
    ``layers`` / ``first`` / ``last`` only that pipeline stage's tensors."""
    d = Path(d)
    cfg = config_from_hf(json.loads((d / "config.json").read_text()), name,
                         sliding_window=True)
    sd = LazyStateDict(d)
    try:
        params = from_hf_state_dict(cfg, sd, layers=layers, first=first, last=last, dtype=dtype)
    finally:
        sd.close()
    dev = torch.device(device)
    if dev.type != "cpu":
        params = {k: v.to(dev, non_blocking=True) for k, v in params.items()}
        torch.cuda.synchronize(dev)
    return cfg, params
