"""Paged KV cache storage for one pipeline stage (its layers only).

Two tensors per stage (one allocation each, sized from free HBM):
    K: [L_stage, num_blocks, Hkv, block_size, hd]
    V: [L_stage, num_blocks, Hkv, block_size, hd]   (token-major like K, see ops/reference.py)
Elements are the model's dtype (bf16) or, with ``kv_dtype="fp8"``, one OCP ``float8_e4m3fn``
byte each with a per-cache scale for K and for V (half the bytes per token).
Zero-initialised once so rows past a sequence's context are always finite (the decode
kernel reads whole 32-token tiles and multiplies the masked ones by 0).
"""
from __future__ import annotations

import os
from typing import List, Optional, Tuple

import torch

from ..models.configs import ModelConfig


KV_DTYPES = ("bf16", "fp8")


def resolve_kv_dtype(kv_dtype: Optional[str] = None) -> str:
    """``"bf16"`` or ``"fp8"``: the argument, or when it is None the environment variable
    ``KV_CACHE_DTYPE`` (default bf16). Anything else is an error."""
    v = os.environ.get("KV_CACHE_DTYPE", "") or "bf16" if kv_dtype is None else kv_dtype
    v = str(v).strip().lower()
    if v not in KV_DTYPES:
        raise ValueError(f"unknown kv cache dtype {v!r} (one of {', '.join(KV_DTYPES)})")
    return v


def kv_element_bytes(kv_dtype: Optional[str] = "bf16") -> int:
    """Bytes per cache element that the pool is sized with: 1 for fp8, 2 for bf16."""
    return 1 if resolve_kv_dtype(kv_dtype) == "fp8" else 2


def bytes_per_block(cfg: ModelConfig, num_layers: int, block_size: int, dtype_bytes: int = 2):
    return 2 * num_layers * cfg.num_kv_heads * cfg.head_dim * block_size * dtype_bytes


def blocks_for_budget(cfg: ModelConfig, num_layers: int, block_size: int, budget_bytes: int,
                      dtype_bytes: int = 2):
    return max(1, int(budget_bytes // max(1, bytes_per_block(cfg, num_layers, block_size,
                                                             dtype_bytes))))


def auto_num_blocks(cfg: ModelConfig, num_layers: int, block_size: int, device,
                    fraction: float = 0.85, reserve_bytes: Optional[int] = None,
                    cap_tokens: int = 0, pending_bytes: int = 0, dtype_bytes: int = 2) -> int:
    """Blocks that fit in ``fraction`` of the HBM still free (weights already resident)
    minus a reserve for activations, GEMM workspaces and graph pools: the KV pool is sized
    for the 288 GB of an MI355X (Llama-3-8B: ~1.7M tokens of context on one GPU), not for
    max_batch x max_model_len. ``cap_tokens`` / ``DLI_KV_MAX_TOKENS`` cap it (0 = no cap).
    ``pending_bytes``: weights that will land on this device after the pool is sized (a
    pipeline stage sizes its pool before it loads its layers; ranks sharing one device pass
    every rank's). Ranks sharing one device (``DLI_SAME_DEVICE=1`` rehearsals) split the rest
    by ``LOCAL_WORLD_SIZE``. ``dtype_bytes``: bytes per cache element (1 for an FP8 cache: the
    same budget holds twice the blocks)."""
    dev = torch.device(device)
    env_cap = int(os.environ.get("DLI_KV_MAX_TOKENS", "0") or 0)
    cap_tokens = env_cap or cap_tokens
    if dev.type == "cuda":
        free, total = torch.cuda.mem_get_info(dev)
        free = max(0, free - int(pending_bytes))
        if reserve_bytes is None:
            reserve_bytes = max(8 << 30, int(0.03 * total))
        if os.environ.get("DLI_SAME_DEVICE", "0") == "1":
            ranks = os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE"))
            if ranks is None:
                # a worker that joined a ring by init_method (no launcher environment)
                import torch.distributed as dist
                ranks = dist.get_world_size() if dist.is_initialized() else 1
            fraction /= max(1, int(ranks))
        budget = max(0, int(free * fraction) - reserve_bytes)
    else:
        budget = 256 << 20                  # CPU (tests / the gpt2 plumbing config)
        cap_tokens = cap_tokens or (1 << 16)
    n = blocks_for_budget(cfg, max(1, num_layers), block_size, budget, dtype_bytes)
    if cap_tokens:
        n = min(n, -(-cap_tokens // block_size))
    return max(n, 16)


class KVLayers(list):
    """The per-layer (k, v) pairs of a cache, with the cache's scales (``k_scale``,
    ``v_scale``): what a model's forward takes as ``kv_caches``."""

    def __init__(self, pairs, k_scale: float = 1.0, v_scale: float = 1.0):
        super().__init__(pairs)
        self.k_scale, self.v_scale = float(k_scale), float(v_scale)


class KVCache:
    """``kv_dtype`` "bf16": elements of ``dtype`` (the model's). "fp8": one OCP
    ``float8_e4m3fn`` byte per element, value = byte * scale with one fp32 scale per cache
    (``k_scale``, ``v_scale``; see ops/reference.py ``quantize_kv``). A zero byte is 0.0, so
    the zero-initialised pool holds finite rows either way."""

    def __init__(self, cfg: ModelConfig, num_layers: int, num_blocks: int, block_size: int,
                 device, dtype=torch.bfloat16, kv_dtype: str = "bf16", k_scale: float = 1.0,
                 v_scale: float = 1.0):
        self.cfg = cfg
        self.num_layers = num_layers
        self.num_blocks = num_blocks
        self.block_size = block_size
        self.kv_dtype = resolve_kv_dtype(kv_dtype)
        if not (k_scale > 0 and v_scale > 0):
            raise ValueError(f"kv cache scales must be > 0, got {k_scale}, {v_scale}")
        if self.kv_dtype != "fp8" and (k_scale != 1.0 or v_scale != 1.0):
            raise ValueError("k_scale / v_scale other than 1 need kv_dtype='fp8'")
        self.k_scale, self.v_scale = float(k_scale), float(v_scale)
        if self.kv_dtype == "fp8":
            dtype = torch.float8_e4m3fn
        hkv, hd = cfg.num_kv_heads, cfg.head_dim
        self.k = torch.zeros(num_layers, num_blocks, hkv, block_size, hd, dtype=dtype, device=device)
        self.v = torch.zeros(num_layers, num_blocks, hkv, block_size, hd, dtype=dtype, device=device)

    def layers(self) -> KVLayers:
        return KVLayers([(self.k[i], self.v[i]) for i in range(self.num_layers)],
                        self.k_scale, self.v_scale)

    @property
    def nbytes(self) -> int:
        return 2 * self.k.numel() * self.k.element_size()

    @property
    def capacity_tokens(self) -> int:
        return self.num_blocks * self.block_size
