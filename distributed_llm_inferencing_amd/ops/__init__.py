"""Op API used by the models. CUDA(HIP) tensors -> gfx950 kernels; CPU tensors -> PyTorch
reference (``ops/reference.py``). There is no silent fallback on a GPU: if the kernel
library is missing, the first GPU op raises (``_native.require_native``).

All functions take/return torch tensors and launch on torch's current stream.
"""
from __future__ import annotations

import math
import time
from typing import Optional

import torch

from . import _native as N
from . import gemm as G
from . import reference as R

_native_call = N.call
_p = N.ptr
# rows per expert from which eager (prefill) MoE GEMMs take the grouped 256x256 tile
_MOE_PREFILL_ROWS = 1024


def _use_native(t: torch.Tensor) -> bool:
    """GPU tensors always run the HIP kernels (no switch reroutes them to torch ops)."""
    return t.is_cuda


def _st():
    return N.stream_ptr()


# ----------------------------------------------------------------------------- norms
def rmsnorm(x, w, eps, residual_copy: Optional[torch.Tensor] = None):
    """out = rmsnorm(x)*w; if residual_copy is given it receives a copy of x."""
    if not _use_native(x):
        if residual_copy is not None:
            residual_copy.copy_(x)
        return R.rmsnorm(x, w, eps)
    out = torch.empty_like(x)
    rows, dim = x.shape
    _native_call("dli_rmsnorm", _p(out), _p(residual_copy), _p(x), _p(w), rows, dim, eps, _st())
    return out


def add_rmsnorm(x, residual, w, eps):
    """residual += x (in place); returns rmsnorm(residual)*w. ``x`` may be a ``MoEPending``
    (a MoE layer's output not yet combined): the combine, the add and the norm then run as
    one kernel."""
    if isinstance(x, MoEPending):
        return x.add_rmsnorm(residual, w, eps)
    if not _use_native(x):
        out, r = R.fused_add_rmsnorm(x, residual, w, eps)
        residual.copy_(r)
        return out
    out = torch.empty_like(x)
    rows, dim = x.shape
    _native_call("dli_fused_add_rmsnorm", _p(out), _p(residual), _p(x), _p(w), rows, dim, eps,
                 _st())
    return out


def layernorm(x, w, b, eps, residual_copy: Optional[torch.Tensor] = None):
    if not _use_native(x):
        if residual_copy is not None:
            residual_copy.copy_(x)
        return R.layernorm(x, w, b, eps)
    out = torch.empty_like(x)
    rows, dim = x.shape
    _native_call("dli_layernorm", _p(out), _p(residual_copy), _p(x), _p(w), _p(b), rows, dim,
                 eps, _st())
    return out


def add_layernorm(x, residual, w, b, eps):
    if not _use_native(x):
        out, r = R.fused_add_layernorm(x, residual, w, b, eps)
        residual.copy_(r)
        return out
    out = torch.empty_like(x)
    rows, dim = x.shape
    _native_call("dli_fused_add_layernorm", _p(out), _p(residual), _p(x), _p(w), _p(b), rows,
                 dim, eps, _st())
    return out


class MoEPending:
    """A decode MoE layer's output before its combine: the grouped down projection's fp16
    split-K slabs, the routing weights and the row of each (token, pick). ``add_rmsnorm``
    (the next layer's input norm, via ``ops.add_rmsnorm``) combines, adds into the residual
    and normalises in one kernel (``dli_moe_combine_add_rmsnorm``); ``materialize()`` runs
    the plain combine for any other consumer. The slab workspace must not be reused before
    the consumer has run (the next GEMM to use it is the next layer's)."""

    def __init__(self, ws, splits: int, rows: int, topk_w, pos, shape, dtype, device):
        self.ws, self.splits, self.rows = ws, splits, rows
        self.topk_w, self.pos = topk_w, pos
        self.shape, self.dtype, self.device = shape, dtype, device

    def materialize(self) -> torch.Tensor:
        T, D = self.shape
        out = torch.empty(T, D, dtype=self.dtype, device=self.device)
        k = self.topk_w.shape[1]
        _native_call("dli_moe_combine_slabs", _p(out), _p(self.ws), self.splits, self.rows,
                     _p(self.topk_w), _p(self.pos), T, k, D, _st())
        return out

    def add_rmsnorm(self, residual, w, eps):
        """w None: the residual add only (a stage's last layer); returns None then."""
        T, D = self.shape
        if D not in (4096, 2048) or not residual.is_contiguous():
            m = self.materialize()
            if w is None:
                residual.add_(m)
                return None
            return add_rmsnorm(m, residual, w, eps)
        out = torch.empty(T, D, dtype=self.dtype, device=self.device) if w is not None else None
        k = self.topk_w.shape[1]
        _native_call("dli_moe_combine_add_rmsnorm", _p(out), _p(residual), _p(self.ws),
                     self.splits, self.rows, _p(self.topk_w), _p(self.pos), T, k, D, _p(w),
                     float(eps), _st())
        return out


class NormedRows:
    """rmsnorm(residual) * w, not yet computed: batch-1 decode (models/model.py) hands this to
    the consuming GEMV, whose prologue normalises the rows into LDS (``dli_gemv_fused``), so
    the O / down projections add straight into the residual (``linear_residual``) and no
    reduce + norm kernel runs between them. Consumers without such a prologue call
    ``materialize()``. The residual must not change before the consumer has run."""
    __slots__ = ("residual", "w", "eps")

    def __init__(self, residual: torch.Tensor, w: torch.Tensor, eps: float):
        self.residual, self.w, self.eps = residual, w, eps

    @property
    def shape(self):
        return self.residual.shape

    @property
    def device(self):
        return self.residual.device

    @property
    def dtype(self):
        return self.residual.dtype

    def materialize(self) -> torch.Tensor:
        return rmsnorm(self.residual, self.w, self.eps)


# ----------------------------------------------------------------------------- FP8 weights
_fp8_scratch: dict = {}


def reserve_fp8_scratch(device, numel: int) -> None:
    """Make the per-device bf16 scratch of ``Fp8Weight.bf16()`` hold ``numel`` elements (the
    largest quantised projection of a model, reserved when the model is built: the KV pool
    is sized after it and no allocation happens inside a graph capture). Not ``G.workspace``:
    a GEMM's split-K slabs live there during the same call."""
    device = torch.device(device)
    if device.type != "cuda" or numel <= 0:
        return
    key = (device.type, device.index if device.index is not None
           else torch.cuda.current_device())
    buf = _fp8_scratch.get(key)
    if buf is not None and buf.numel() >= numel:
        return
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("the FP8 weight scratch cannot grow inside a graph capture "
                           "(ops.reserve_fp8_scratch was not called for this weight)")
    with G._ws_lock:                     # growth, as G.workspace
        buf = _fp8_scratch.get(key)
        if buf is not None and buf.numel() >= numel:
            return
        if buf is not None:
            G._retired.append(buf)       # a captured graph may still write it (ops.gemm)
        _fp8_scratch[key] = torch.empty(numel, dtype=torch.bfloat16, device=device)


class Fp8Weight:
    """A weight-only quantised projection: ``q`` [N, K] ``float8_e4m3fn`` and fp32 ``scale``
    [N / 16, ceil(K / 128)], W[n, k] = float(q[n, k]) * scale[n // 16, k // 128]
    (``reference.dequantize_weight``). Looks like its [N, K] tensor to the planner (``shape``,
    ``dim()``, ``device``); the linear ops stream it through the FP8 GEMV kernels at
    M <= ``G.GEMV_MAX_M``, through the FP8 MFMA stream tiles up to ``G.FP8_STREAM_MAX_M`` rows
    where the autotuner pinned one (``stream_ok``), and run every other shape on its bf16
    image (``bf16()``)."""
    __slots__ = ("q", "scale")
    act_dtype = torch.bfloat16           # what the activations it meets are

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        if q.dtype != R.FP8_W or q.dim() != 2:
            raise ValueError(f"Fp8Weight: q must be a 2-D float8_e4m3fn tensor, got {q.dtype} "
                             f"{tuple(q.shape)}")
        n, k = q.shape
        if n % R.W_SCALE_ROWS:
            raise ValueError(f"Fp8Weight: {n} rows, not a multiple of {R.W_SCALE_ROWS}")
        want = (n // R.W_SCALE_ROWS, -(-k // R.W_BLOCK))
        if scale.dtype != torch.float32 or tuple(scale.shape) != want:
            raise ValueError(f"Fp8Weight: scale must be fp32 {want} for a weight {(n, k)}, got "
                             f"{scale.dtype} {tuple(scale.shape)}")
        if scale.device != q.device:
            raise ValueError("Fp8Weight: q and scale on different devices")
        self.q, self.scale = q.contiguous(), scale.contiguous()

    @property
    def shape(self):
        return self.q.shape

    @property
    def device(self):
        return self.q.device

    @property
    def dtype(self):
        return self.q.dtype

    def dim(self) -> int:
        return 2

    def numel(self) -> int:
        return self.q.numel()

    def element_size(self) -> int:
        return 1

    def clone(self) -> "Fp8Weight":
        return Fp8Weight(self.q.clone(), self.scale.clone())

    def to(self, device) -> "Fp8Weight":
        return Fp8Weight(self.q.to(device), self.scale.to(device))

    def dequantize(self, dtype=torch.float32) -> torch.Tensor:
        return R.dequantize_weight(self.q, self.scale, dtype)

    def bf16(self) -> torch.Tensor:
        """The bf16 weight ``reference.dequantize_weight(q, scale, torch.bfloat16)``: on the
        GPU a view of the per-device scratch filled by ``dli_dequant_fp8_block`` on the
        current stream, valid until the next ``bf16()`` there (the stream orders the reuse:
        the GEMM that reads it is enqueued before the next fill). Like ``G.workspace``, the
        scratch assumes that one host thread at a time issues a device's ops on one stream:
        two threads interleaving fill A, fill B, GEMM A would hand GEMM A the weight of B."""
        if not self.q.is_cuda:
            return self.dequantize(torch.bfloat16)
        n, k = self.q.shape
        reserve_fp8_scratch(self.q.device, n * k)
        out = _fp8_scratch[(self.q.device.type, self.q.device.index)][:n * k].view(n, k)
        _native_call("dli_dequant_fp8_block", _p(self.q), _p(self.scale), _p(out), n, k, _st())
        return out

    def gemv_ok(self, M: int, p: G.GemmPlan) -> bool:
        """Whether the FP8 weight stream takes this call: a GEMV tile, and K and every K slice
        in whole 16-element chunks."""
        K = self.q.shape[1]
        return (M <= G.GEMV_MAX_M and p.tile in G.GEMV_TILES and K % 16 == 0
                and K % p.splits == 0 and (K // p.splits) % 16 == 0)

    def stream_ok(self, M: int, p: G.GemmPlan) -> bool:
        """Whether the FP8 MFMA weight stream (``dli_gemm_fp8_stream``) takes this call: one
        of its tiles, ``G.GEMV_MAX_M`` < M <= ``G.FP8_STREAM_MAX_M``, K in whole 16-element
        chunks and, with split-K, every slice a multiple of 128 (``G.stream_slices_ok``)."""
        return (p.tile in G.FP8_STREAM_TILES and G.GEMV_MAX_M < M <= G.FP8_STREAM_MAX_M
                and G.stream_slices_ok(self.q.shape[1], p.splits))


class Fp8Experts:
    """A stack of weight-only quantised expert projections: ``q`` [E, N, K] ``float8_e4m3fn``
    and fp32 ``scale`` [E, N / 16, ceil(K / 128)], every expert an ``Fp8Weight`` of its own:
    W[e, n, k] = float(q[e, n, k]) * scale[e, n // 16, k // 128]
    (``reference.dequantize_experts``). Looks like its [E, N, K] tensor to ``moe_mlp`` and the
    planner; a decode step streams it through the grouped FP8 MFMA stream
    (``dli_gemm_fp8_stream_grouped``) where ``stream_ok`` holds, and every other call runs the
    bf16 grouped GEMMs on its bf16 image (``bf16()``, the whole stack in one pass)."""
    __slots__ = ("q", "scale")
    act_dtype = torch.bfloat16

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        if q.dtype != R.FP8_W or q.dim() != 3:
            raise ValueError(f"Fp8Experts: q must be a 3-D float8_e4m3fn tensor, got {q.dtype} "
                             f"{tuple(q.shape)}")
        e, n, k = q.shape
        if n % R.W_SCALE_ROWS:
            raise ValueError(f"Fp8Experts: {n} rows, not a multiple of {R.W_SCALE_ROWS}")
        want = (e, n // R.W_SCALE_ROWS, -(-k // R.W_BLOCK))
        if scale.dtype != torch.float32 or tuple(scale.shape) != want:
            raise ValueError(f"Fp8Experts: scale must be fp32 {want} for a stack {(e, n, k)}, "
                             f"got {scale.dtype} {tuple(scale.shape)}")
        if scale.device != q.device:
            raise ValueError("Fp8Experts: q and scale on different devices")
        self.q, self.scale = q.contiguous(), scale.contiguous()

    @property
    def shape(self):
        return self.q.shape

    @property
    def device(self):
        return self.q.device

    @property
    def dtype(self):
        return self.q.dtype

    def dim(self) -> int:
        return 3

    def numel(self) -> int:
        return self.q.numel()

    def element_size(self) -> int:
        return 1

    def clone(self) -> "Fp8Experts":
        return Fp8Experts(self.q.clone(), self.scale.clone())

    def to(self, device) -> "Fp8Experts":
        return Fp8Experts(self.q.to(device), self.scale.to(device))

    def dequantize(self, dtype=torch.float32) -> torch.Tensor:
        return R.dequantize_experts(self.q, self.scale, dtype)

    def bf16(self) -> torch.Tensor:
        """The bf16 stack [E, N, K]: on the GPU a view of the per-device scratch of
        ``Fp8Weight.bf16`` (same validity rule), filled by one ``dli_dequant_fp8_block`` call
        on the [E * N, K] view (N is a multiple of 16, so no scale group straddles two
        experts)."""
        if not self.q.is_cuda:
            return self.dequantize(torch.bfloat16)
        e, n, k = self.q.shape
        reserve_fp8_scratch(self.q.device, e * n * k)
        out = _fp8_scratch[(self.q.device.type, self.q.device.index)][:e * n * k].view(e, n, k)
        _native_call("dli_dequant_fp8_block", _p(self.q), _p(self.scale), _p(out), e * n, k,
                     _st())
        return out

    def stream_ok(self, rows: int, groups: int, p: G.GemmPlan) -> bool:
        """Whether the grouped FP8 stream takes ``rows`` permuted rows over ``groups`` experts
        under ``p``: one of its tiles, unsplit, K in whole 16-element chunks, and a tile list
        (``G.max_items`` at ``G.fp8_grouped_bm``) that fits one grid dimension."""
        return (p.tile in G.FP8_STREAM_TILES and p.splits == 1 and rows > 0
                and groups == self.q.shape[0] and G.stream_slices_ok(self.q.shape[2], 1)
                and G.max_items(rows, groups, G.fp8_grouped_bm(rows, groups)) <= 65535)


def _dense(w):
    """The tensor the bf16 kernels (or, off the GPU, the reference ops) read for ``w``."""
    if isinstance(w, (Fp8Weight, Fp8Experts)):
        return w.bf16() if w.q.is_cuda else w.dequantize(torch.float32)
    return w


def _inner_contig(w) -> bool:
    return isinstance(w, Fp8Weight) or w.stride(-1) == 1


def _stream_plan(x, w, p: G.GemmPlan, form_ok: bool = True) -> bool:
    """Whether ``p`` runs this call on the FP8 MFMA weight stream (``_pick_kernel``'s first
    question; never ``w.bf16()``). A stream tile forced on a plain tensor is an error; an
    ``Fp8Weight`` call the kernel cannot take (``stream_ok``, rows not 16-B aligned,
    ``form_ok`` False: a grouped call or an epilogue it has not) is False."""
    if p.tile not in G.FP8_STREAM_TILES:
        return False
    if not isinstance(w, Fp8Weight):
        raise ValueError(f"GEMM tile {p.tile} streams FP8 block-scaled weights "
                         f"(ops.Fp8Weight) only, got a {w.dtype} tensor")
    return (form_ok and w.stream_ok(x.shape[0], p) and x.stride(0) % 8 == 0
            and x.data_ptr() % 16 == 0)


def _pick_kernel(x, w, p: G.GemmPlan, epi: str, groups: Optional[int] = None,
                 keep_splits: bool = False):
    """The one choice of a GEMM's native family: (kind, plan, weight) with kind "stream"
    (``w`` an ``Fp8Weight`` on the MFMA weight stream), "gemv_fp8" (on the FP8 GEMV stream) or
    "gemm" (``w`` a plain tensor: the bf16 image of an ``Fp8Weight`` neither stream takes,
    dequantised here, once). A stream plan the call cannot take (a cached plan met another M,
    an odd K, a grouped call) gives way to a plan of the bf16 families, so its tile id never
    reaches ``dli_gemm``: the heuristic plan; with ``keep_splits`` (slabs a fused consumer was
    sized for) the heuristic's tile at ``p``'s split count; ``grouped_tile`` for a grouped
    call (``groups`` given)."""
    fp8 = isinstance(w, Fp8Weight)
    if not fp8 and p.tile not in G.FP8_STREAM_TILES:
        return "gemm", p, w
    M, K = x.shape
    fp8_form = groups is None and epi in G.FP8_STREAM_EPIS
    if _stream_plan(x, w, p, fp8_form):
        return "stream", p, w
    if p.tile in G.FP8_STREAM_TILES:
        if groups is not None:
            p = G.GemmPlan("dli", G.grouped_tile(M, groups), 1)
        elif keep_splits:
            p = G.GemmPlan("dli", G._heuristic(M, w.shape[-2], K, "splitk").tile, p.splits)
        else:
            p = G._heuristic(M, w.shape[-2], K, epi)
    elif fp8_form and w.gemv_ok(M, p):
        return "gemv_fp8", p, w
    return "gemm", p, w.bf16()


def _launch_gemm(kind: str, x, w, p: G.GemmPlan, code: int, C, ldc: int, rows: int, Nn: int,
                 K: int, bias=None, ws=None, group_off=None, groups: int = 1, tile_list=None,
                 arow=None):
    """Marshal one GEMM of ``_pick_kernel``'s ``kind``: C [rows, Nn] (None: slabs only, into
    ``ws``) = epilogue ``code`` of x @ w.T. For "gemm", ``tile_list`` (list, max items) selects
    the compact grouped grid and ``arow`` the row permutation x is read through."""
    # the optional operands are None more often than not: no ``_p`` call for those
    pC = None if C is None else _p(C)
    pbias = None if bias is None else _p(bias)
    poff = None if group_off is None else _p(group_off)
    if kind != "gemm":
        _native_call("dli_gemm_fp8_stream" if kind == "stream" else "dli_gemv_fp8", _p(x),
                     x.stride(0), _p(w.q), _p(w.scale), w.scale.stride(0), K, pC, ldc, rows, Nn,
                     K, code, p.tile, p.splits, pbias, _p(ws), _st())
    elif tile_list is not None:
        _native_call("dli_gemm_grouped_list", _p(x), x.stride(0), _p(w), w.stride(-2), pC, ldc,
                     rows, Nn, K, code, p.tile, p.splits, _p(arow), _p(ws), poff, groups,
                     _p(tile_list[0]), tile_list[1], _st())
    elif arow is not None:               # unsplit SiLU*up only (G.GATHER_TILES)
        _native_call("dli_gemm_grouped_gather", _p(x), x.stride(0), _p(w), w.stride(-2), pC, ldc,
                     rows, Nn, K, p.tile, _p(arow), poff, groups, _st())
    else:
        _native_call("dli_gemm", _p(x), x.stride(0), _p(w), w.stride(-2), pC, ldc, rows, Nn, K,
                     code, p.tile, p.splits, pbias, _p(ws), poff, groups, _st())


def _launch_gemv_fused(rows, norm_w, eps: float, w, C, ldc: int, code: int, tile: int,
                       splits: int, ws):
    """Marshal the fused GEMV of either weight format: C = epilogue ``code`` of
    (rmsnorm(rows) * norm_w, or ``rows`` as they are when ``norm_w`` is None) @ w.T."""
    M, K = rows.shape
    fp8 = isinstance(w, Fp8Weight)
    wargs = (_p(w.q), _p(w.scale), w.scale.stride(0), K) if fp8 else (_p(w), w.stride(-2))
    _native_call("dli_gemv_fused_fp8" if fp8 else "dli_gemv_fused", _p(rows), rows.stride(0),
                 _p(norm_w), eps, *wargs, _p(C), ldc, M, w.shape[0], K, code, tile, splits,
                 _p(ws), _st())


def _out_width(n: int, epi: str) -> int:
    """Columns of epi(x @ w.T) for an ``n``-row w: SiLU*up halves the interleaved gate/up rows."""
    return n // 2 if epi == "silu_mul" else n


def deferred_norm_ok(x: torch.Tensor) -> bool:
    """Whether a decode step of ``x.shape[0]`` rows runs the reduce-free GEMV chain."""
    M, K = x.shape
    return (G.DEFER_NORM and _use_native(x) and M <= G.GEMV_MAX_M and K % 8 == 0
            and K <= 8192 and x.is_contiguous())


def _gemv_prologue(x: NormedRows, w, epi: str, plan: Optional[G.GemmPlan], C, ldc, ws=None):
    """Run the GEMV with the deferred norm in its prologue; False if the plan has no such
    variant (the caller materialises the norm)."""
    M, K = x.shape
    p = plan or G.plan(M, w.shape[0], K, epi, G.wdt(w))
    tiles = G.GEMV_PRO_TILES.get(epi, ())
    if p.tile not in tiles or (p.tile in G.GEMV_PRO_M1_ONLY and M > 1) or M > G.GEMV_MAX_M:
        return False
    if isinstance(w, Fp8Weight) and not w.gemv_ok(M, p):
        return False
    r = x.residual
    if ws is None and p.splits > 1:      # split K into C: slabs + the reduce kernel
        ws = G.workspace(r.device, p.splits * M * w.shape[0] * 4)
    _launch_gemv_fused(r, x.w, x.eps, w, C, ldc, G.EPI["silu_mul"] if epi == "silu_mul" else 0,
                       p.tile, p.splits, ws)
    return True


def linear_normed(x: NormedRows, w, epi: str, plan: G.GemmPlan):
    """epi(rmsnorm(x) @ w.T) under a forced plan (the autotuner's timing of a prologue GEMV;
    plans without a prologue variant materialise the norm first, as ``linear`` does)."""
    y = torch.empty(x.shape[0], _out_width(w.shape[-2], epi), dtype=x.dtype, device=x.device)
    if plan.splits > 1 and epi == "splitk":
        return _gemm_native(x.materialize(), w, "none", plan=plan)
    if _gemv_prologue(x, w, epi, plan, y, y.stride(0)):
        return y
    return _gemm_native(x.materialize(), w, epi, plan=plan, out=y)


def linear_residual(x, w, residual, plan: Optional[G.GemmPlan] = None):
    """residual += x @ w.T (bf16-rounded, in place) — the O / down projection of a batch-1
    decode layer as ONE kernel: full K per workgroup, the add in its epilogue (no split-K
    slabs, no reduce kernel). Other shapes take ``linear_add_rmsnorm`` without a norm."""
    M, K = x.shape
    p = plan or G.plan(M, w.shape[0], K, "res", G.wdt(w))
    if (not _use_native(x) or p.tile not in G.GEMV_RES_TILES or M > G.GEMV_MAX_M
            or not residual.is_contiguous() or x.stride(-1) != 1 or not _inner_contig(w)
            or (isinstance(w, Fp8Weight) and not w.gemv_ok(M, p))):
        linear_add_rmsnorm(x, w, residual, None, 0.0)
        return
    _launch_gemv_fused(x, None, 0.0, w, residual, residual.stride(0), G.EPI_RES, p.tile, 1,
                       None)


# ----------------------------------------------------------------------------- embedding
def embedding(ids, table, pos_table=None, positions=None):
    if not _use_native(table):
        return R.embedding(ids, table, pos_table, positions)
    T = ids.shape[0]
    out = torch.empty(T, table.shape[1], dtype=table.dtype, device=table.device)
    _native_call("dli_embedding", _p(out), _p(ids), _p(table), _p(pos_table), _p(positions), T,
                 table.shape[1], _st())
    return out


# ----------------------------------------------------------------------------- GEMM
def _gemm_native(x, w, epi: str, bias=None, out=None, plan: Optional[G.GemmPlan] = None,
                 groups: int = 1, group_off=None, rows_per_group: Optional[int] = None,
                 tile_list=None):
    """``tile_list`` = (list, max items) of a grouped call: the compact grid over the align
    step's list for the plan's tile height (``dli_gemm_grouped_list``); ``rows_per_group`` is
    then the total permuted rows."""
    M, K = x.shape
    Nn = w.shape[-2]
    grouped = group_off is not None
    if plan is None:
        plan = (G.grouped_plan(M, Nn, K, epi, groups) if grouped
                else G.plan(M, Nn, K, epi, G.wdt(w)))
    kind, plan, w = _pick_kernel(x, w, plan, epi, groups if grouped else None)
    if out is None:
        dt = torch.float32 if epi == "f32" else x.dtype
        out = torch.empty(M, _out_width(Nn, epi), dtype=dt, device=x.device)
    ws = G.workspace(x.device, plan.splits * M * Nn * 4) if plan.splits > 1 else None
    _launch_gemm(kind, x, w, plan, G.EPI[epi], out, out.stride(0),
                 rows_per_group if grouped else M, Nn, K, bias, ws, group_off, groups, tile_list)
    return out


def linear(x, w, bias=None, epi: str = "none", out=None):
    """y = epi(x @ w.T (+bias)). epi in {none, f32, silu_mul, bias_gelu, bias}.
    silu_mul expects the 16-row interleaved gate/up weight and returns width N/2."""
    if bias is not None and epi == "none":
        epi = "bias"
    if isinstance(x, NormedRows):
        if (bias is None and epi in ("none", "silu_mul") and _use_native(x.residual)
                and x.residual.is_contiguous()):
            y = out if out is not None else torch.empty(x.shape[0], _out_width(w.shape[-2], epi),
                                                        dtype=x.dtype, device=x.device)
            if _gemv_prologue(x, w, epi, None, y, y.stride(0)):
                return y
        x = x.materialize()
    if not _use_native(x):
        w = _dense(w)
        if epi == "silu_mul":
            y = R.silu_mul(R.linear(x, w))
        elif epi == "f32":
            y = R.linear(x, w, out_dtype=torch.float32)
        elif epi == "bias_gelu":
            y = R.gelu_tanh(R.linear(x, w, bias))
        else:
            y = R.linear(x, w, bias)
        if out is not None:
            out.copy_(y)
            return out
        return y
    if x.stride(-1) != 1 or not _inner_contig(w):
        raise ValueError("linear: inner dims must be contiguous")
    return _gemm_native(x, w, epi, bias=bias, out=out)


def _splitk_plan(x, w):
    """A split-K plan for a GEMM whose partial sums feed a fused reduce, or None."""
    if not _use_native(x) or x.stride(-1) != 1 or not (isinstance(w, Fp8Weight)
                                                       or w.stride(-1) == 1):
        return None
    M, K = x.shape
    p = G.plan(M, w.shape[0], K, "splitk", G.wdt(w))
    return p if p.splits > 1 else None


def _split_slabs(x, w, plan: Optional[G.GemmPlan] = None, ws=None):
    """The GEMM of a fused split-K consumer: (plan, workspace, slab format) with x @ w.T as
    the plan's split-K partial slabs in the workspace (no output tensor: the consumer reduces
    them), or None where the plan (``plan`` if forced, else the "splitk" plan of the shape)
    does not split. The format the consumer must read: 1 = fp16 x 1/16 (the MFMA families'
    EPI "slab16" store, half the bytes), 0 = fp32 (the GEMV and FP8 stream tiles, the 4-wave
    family). ``x`` may be a ``NormedRows``: the GEMV with the norm in its prologue where the
    plan has one, else the materialised norm. ``ws``: the caller's own slab buffer."""
    normed = isinstance(x, NormedRows)
    rows = x.residual if normed else x
    p = _splitk_plan(rows, w) if plan is None else plan
    if p is None or (p.splits == 1 and ws is None):
        return None
    M, K = rows.shape
    Nn = w.shape[0]
    if ws is None:
        ws = G.workspace(rows.device, p.splits * M * Nn * 4)
    if normed:
        if _gemv_prologue(x, w, "splitk", p, None, Nn, ws=ws):
            return p, ws, 0
        x = x.materialize()
    kind, run, w = _pick_kernel(x, w, p, "splitk", None, True)     # (keeps p's split count)
    fmt = 1 if (G.SLAB16 and run.tile in G.SLAB16_TILES and run.splits in (2, 4, 8)) else 0
    _launch_gemm(kind, x, w, run, G.EPI["slab16"] if fmt else 0, None, Nn, M, Nn, K, None, ws)
    return p, ws, fmt


def _slab_gemm(x, w, p: G.GemmPlan, ws) -> int:
    """x @ w.T as ``p.splits`` split-K partial slabs in ``ws``; returns their format
    (``_split_slabs``)."""
    return _split_slabs(x, w, p, ws)[2]


def linear_add_rmsnorm(x, w, residual, norm_w, eps, plan: Optional[G.GemmPlan] = None,
                       route=None):
    """residual += x @ w.T (bf16-rounded, in place); returns rmsnorm(residual) * norm_w
    (None when norm_w is None). Split-K GEMMs reduce their partial slabs inside the norm
    kernel (fused_reduce.hip), so the bf16 GEMM output is never materialised.
    ``plan`` forces the GEMM plan (the autotuner times every candidate with its consumer).
    ``route`` = (router weight [E, N], k[, norm_topk = True]): also the MoE gate of the output
    rows — returns (out, topk_w, topk_ids); with fp16 slabs, N = 4096, E <= 8 and renormalised
    weights inside the same reduce kernel (``dli_splitk_add_rmsnorm_route``), else by
    ``moe_router``."""
    slabs = _split_slabs(x, w, plan)
    if slabs is None:
        y = linear(x, w) if plan is None else _gemm_native(x, w, "none", plan=plan)
        if norm_w is None:
            residual.add_(y)             # bf16 add computes in fp32 and rounds once
            out = None
        else:
            out = add_rmsnorm(y, residual, norm_w, eps)
    else:
        p, ws, fmt = slabs
        M, Nn = residual.shape
        out = torch.empty_like(residual) if norm_w is not None else None
        if (route is not None and fmt == 1 and norm_w is not None and Nn == 4096
                and route[0].shape[0] <= 8 and (len(route) < 3 or route[2])
                and route[0].is_contiguous() and residual.is_contiguous()
                and route[0].data_ptr() % 16 == 0):
            wr, k = route[:2]
            tw = torch.empty(M, k, dtype=torch.float32, device=x.device)
            ti = torch.empty(M, k, dtype=torch.int32, device=x.device)
            _native_call("dli_splitk_add_rmsnorm_route", _p(out), _p(residual), _p(ws),
                         p.splits, M, Nn, _p(norm_w), eps, _p(wr), wr.shape[0], k, _p(tw),
                         _p(ti), _st())
            return out, tw, ti
        _native_call("dli_splitk_add_rmsnorm", _p(out), _p(residual), _p(ws), p.splits, M, Nn,
                     _p(norm_w), eps, fmt, _st())
    if route is None:
        return out
    return (out,) + tuple(moe_router(out, route[0], route[1], route[2] if len(route) > 2
                                     else True))


def _qkv_extras(bias, qk_norm, n: int, hd: int):
    """The optional inputs of the RoPE kernels, checked: ``bias`` [n] (Qwen2's QKV bias) and
    ``qk_norm`` = (q_w [hd], k_w [hd], eps) (Qwen3's per-head RMSNorm of q and k before the
    rotation). Returns (bias, q_w, k_w, eps) with None for what is absent."""
    if bias is None and qk_norm is None:
        return None, None, None, 0.0
    q_w = k_w = None
    eps = 0.0
    if qk_norm is not None:
        q_w, k_w, eps = qk_norm
        if q_w.numel() != hd or k_w.numel() != hd:
            raise ValueError(f"qk_norm weights must have head_dim = {hd} elements")
    ts = [t for t in (bias, q_w, k_w) if t is not None]
    if bias is not None and bias.numel() != n:
        raise ValueError(f"qkv bias must have {n} elements, got {bias.numel()}")
    if any(t.dtype != torch.bfloat16 or not t.is_contiguous() or t.data_ptr() % 16
           for t in ts):
        raise ValueError("qkv bias / qk_norm weights must be contiguous 16-B aligned bf16")
    return bias, q_w, k_w, float(eps)


_CPU_KV_DTYPES = (torch.bfloat16, torch.float16, torch.float32, R.FP8_KV)


def kv_cache_is_fp8(k_cache, v_cache, k_scale: float = 1.0, v_scale: float = 1.0,
                    native: bool = True) -> bool:
    """Checks a paged cache pair and its scales before any kernel sees them; True for an FP8
    (``float8_e4m3fn``) cache. The HIP kernels read bf16 or e4m3fn and nothing else (a
    one-byte buffer handed to the bf16 kernels would be read as 2-byte elements, past its
    end); the reference ops also take fp16 / fp32 caches. K and V share one dtype, scales
    are > 0, and only an FP8 cache has scales other than 1."""
    if not (k_scale > 0 and v_scale > 0):       # (NaN fails too)
        raise ValueError(f"kv cache scales must be > 0, got {k_scale}, {v_scale}")
    if k_cache is None or v_cache is None:
        return False
    if k_cache.dtype != v_cache.dtype:
        raise ValueError(f"k_cache is {k_cache.dtype} but v_cache is {v_cache.dtype}")
    dt = k_cache.dtype
    if dt not in ((torch.bfloat16, R.FP8_KV) if native else _CPU_KV_DTYPES):
        raise ValueError(f"unsupported kv cache dtype {dt} (bfloat16 or float8_e4m3fn)")
    fp8 = dt == R.FP8_KV
    if not fp8 and (k_scale != 1.0 or v_scale != 1.0):
        raise ValueError("k_scale / v_scale other than 1 need a float8_e4m3fn kv cache")
    return fp8


def _kv_inv_scales(fp8: bool, k_scale: float, v_scale: float):
    """The cache writers' (kv_fp8, 1 / k_scale, 1 / v_scale) arguments."""
    if not fp8:
        return 0, 1.0, 1.0
    return 1, R.inv_scale(k_scale), R.inv_scale(v_scale)


def linear_rope_cache(x, w, positions, slot_mapping, cos_sin, k_cache, v_cache, hq, hkv, hd,
                      use_rope: bool = True, plan: Optional[G.GemmPlan] = None, bias=None,
                      qk_norm=None, k_scale: float = 1.0, v_scale: float = 1.0):
    """qkv = x @ w.T with RoPE applied in place to q,k and k,v written to the paged cache
    (``k_scale`` / ``v_scale``: the scales of an FP8 cache, see ``rope_and_cache``).
    ``plan`` forces the GEMM plan (the autotuner times QKV candidates with this consumer).
    ``bias`` / ``qk_norm``: see ``rope_and_cache``; with split-K slabs the bias is added to
    their fp32 sum, before the one rounding that stands for the GEMM output."""
    xr = x.residual if isinstance(x, NormedRows) else x
    fp8 = kv_cache_is_fp8(k_cache, v_cache, k_scale, v_scale, native=_use_native(xr))
    if isinstance(x, NormedRows):
        x = x.materialize()
    slabs = _split_slabs(x, w, plan)
    if slabs is None:
        if plan is None:
            qkv = linear(x, w, bias)
        else:
            qkv = _gemm_native(x, w, "none" if bias is None else "bias", bias=bias, plan=plan)
        rope_and_cache(qkv, positions, slot_mapping, cos_sin, k_cache, v_cache, hq, hkv, hd,
                       use_rope, qk_norm=qk_norm, k_scale=k_scale, v_scale=v_scale)
        return qkv
    p, ws, fmt = slabs
    M, Nn = x.shape[0], w.shape[0]
    qkv = torch.empty(M, Nn, dtype=x.dtype, device=x.device)
    bs = k_cache.shape[2] if k_cache is not None else 16
    bias, q_w, k_w, eps = _qkv_extras(bias, qk_norm, Nn, hd)
    _native_call("dli_splitk_rope_cache", _p(qkv), _p(ws), p.splits, M, Nn, _p(positions),
                 _p(slot_mapping), _p(cos_sin), _p(k_cache), _p(v_cache), hq, hkv, hd, bs,
                 int(use_rope), fmt, _p(bias), _p(q_w), _p(k_w), eps,
                 *_kv_inv_scales(fp8, k_scale, v_scale), _st())
    return qkv


def linear_rope_attention(x, w, positions, slot_mapping, cos_sin, k_cache, v_cache,
                          block_tables, context_lens, max_context: int, hq, hkv, hd, scale,
                          window: int = 0, bias=None, qk_norm=None):
    """Decode step, one fused pass after the QKV GEMM: the split-K slabs (or, for an unsplit
    plan, the bf16 QKV rows) are reduced, q and k rotated, k/v written to the paged cache and
    attention computed by ONE kernel per layer (``dli_decode_attention_fused``) instead of
    ``linear_rope_cache`` + ``decode_attention``. Returns the attention output [B, hq*hd], or
    None where the fused kernel does not apply (the caller then runs the two-kernel path):
    split counts other than 2 / 4, KV-split attention (long contexts at small batch), the
    pipelined long-context kernel, head dim != 128. ``window`` > 0: sliding-window attention;
    the choice between the kernels follows the span a sequence can attend over,
    min(max_context, window). ``bias`` / ``qk_norm`` (Qwen2 / Qwen3, see ``rope_and_cache``)
    are applied by the same kernel's prologue. An FP8 cache has no fused kernel: None."""
    xr = x.residual if isinstance(x, NormedRows) else x
    if hd != 128 or k_cache is None or not _use_native(xr):
        return None
    if kv_cache_is_fp8(k_cache, v_cache):
        return None
    p = _splitk_plan(xr, w)
    if p is not None and p.splits not in (2, 4):
        return None
    B, K = x.shape
    span = decode_span(max_context, window)
    if decode_num_splits(B, hkv, span) != 1:
        return None
    if N.require_native().dli_decode_uses_pipe(hd, span, 1):
        return None                       # dli_decode_attention picks the pipelined kernel
    Nn = w.shape[0]
    if p is None:                         # unsplit plan: the prologue reads the bf16 rows
        src, splits, fmt = linear(x, w, bias), 0, 0
        bias = None                       # applied by the GEMM's epilogue
    else:           # x a NormedRows: _split_slabs tries the prologue GEMV, then the norm
        (_, src, fmt), splits = _split_slabs(x, w, p), p.splits
    out = torch.empty(B, hq * hd, dtype=x.dtype, device=x.device)
    bias, q_w, k_w, eps = _qkv_extras(bias, qk_norm, Nn, hd)
    _native_call("dli_decode_attention_fused", _p(out), _p(src), splits, _p(positions),
                 _p(slot_mapping), _p(cos_sin), _p(k_cache), _p(v_cache), _p(block_tables),
                 block_tables.stride(0), _p(context_lens), B, hq, hkv, hd, k_cache.shape[2],
                 scale, fmt, max(int(window), 0), _p(bias), _p(q_w), _p(k_w), eps, _st())
    return out


def feed_ids(ids, src, feed):
    """In place: ids[i] = feed[src[i]] where src[i] >= 0 (int32 tensors; lookahead input ids
    taken from the in-flight step's sampled tokens)."""
    if not _use_native(ids):
        take = feed.index_select(0, src.clamp(min=0).long()).to(ids.dtype)
        ids.copy_(torch.where(src >= 0, take, ids))
        return ids
    if ids.dtype != torch.int32 or src.dtype != torch.int32 or feed.dtype != torch.int32:
        raise ValueError("feed_ids: int32 tensors expected")
    _native_call("dli_feed_ids", _p(ids), _p(src), _p(feed), ids.shape[0], feed.shape[0], _st())
    return ids


_sinks: dict = {}


def prefetch(t: torch.Tensor, max_wgs: int = 256, nbytes: Optional[int] = None) -> None:
    """Read ``t`` (its first ``nbytes``) on the current stream and discard it: the weight
    lands in the Infinity Cache for the GEMM that streams it next (see
    ``TransformerLM._llama_layers``). No-op off the GPU."""
    if not _use_native(t):
        return
    sink = _sinks.get(t.device)
    if sink is None:
        sink = _sinks[t.device] = torch.empty(256, dtype=torch.int32, device=t.device)
    n = t.numel() * t.element_size() if nbytes is None else int(nbytes)
    _native_call("dli_prefetch", _p(t), n, int(max_wgs), _p(sink), _st())


def silu_mul(gu):
    if not _use_native(gu):
        return R.silu_mul(gu)
    T, F2 = gu.shape
    out = torch.empty(T, F2 // 2, dtype=gu.dtype, device=gu.device)
    _native_call("dli_silu_mul", _p(out), _p(gu), T, F2 // 2, _st())
    return out


def bias_act_(x, bias, act: str = "none"):
    if not _use_native(x):
        y = x.float() + (bias.float() if bias is not None else 0)
        if act == "gelu":
            y = torch.nn.functional.gelu(y, approximate="tanh")
        x.copy_(y.to(x.dtype))
        return x
    T, Nn = x.shape
    _native_call("dli_bias_act", _p(x), _p(bias), T, Nn, 1 if act == "gelu" else 0, _st())
    return x


# ----------------------------------------------------------------------------- RoPE / KV cache
def rope_and_cache(qkv, positions, slot_mapping, cos_sin, k_cache, v_cache, hq, hkv, hd,
                   use_rope: bool = True, bias=None, qk_norm=None, k_scale: float = 1.0,
                   v_scale: float = 1.0):
    """In-place RoPE on q,k inside qkv + paged cache write. Returns views (q, k, v).
    ``bias`` [(hq+2hkv)*hd]: added to the rows first (Qwen2's QKV bias; rows that come from
    ``linear(x, w, bias)`` already hold it). ``qk_norm`` = (q_w [hd], k_w [hd], eps): every q
    and k head is RMS-normalised over its hd dims before the rotation (Qwen3); v is not.
    Each step rounds to bf16: bias, norm, rotation. A ``float8_e4m3fn`` cache receives
    ``reference.quantize_kv`` of the k / v values stored in the rows, under the per-cache
    scales ``k_scale`` / ``v_scale`` (stored = fp8(clamp(x / scale, +-448)))."""
    fp8 = kv_cache_is_fp8(k_cache, v_cache, k_scale, v_scale, native=_use_native(qkv))
    if not _use_native(qkv):
        return R.rope_and_cache(qkv, positions, slot_mapping, cos_sin, k_cache, v_cache, hq, hkv,
                                hd, use_rope, bias=bias, qk_norm=qk_norm, k_scale=k_scale,
                                v_scale=v_scale)
    T = qkv.shape[0]
    bs = k_cache.shape[2] if k_cache is not None else 16
    bias, q_w, k_w, eps = _qkv_extras(bias, qk_norm, (hq + 2 * hkv) * hd, hd)
    _native_call("dli_rope_cache", _p(qkv), qkv.stride(0), _p(positions), _p(slot_mapping),
                 _p(cos_sin), _p(k_cache), _p(v_cache), T, hq, hkv, hd, bs, int(use_rope),
                 _p(bias), _p(q_w), _p(k_w), eps, *_kv_inv_scales(fp8, k_scale, v_scale), _st())
    return R.split_qkv(qkv, hq, hkv, hd)


# ----------------------------------------------------------------------------- attention
def prefill_attention(qkv, cu_seqlens, max_seqlen: int, hq, hkv, hd, scale, out=None,
                      window: int = 0):
    """Causal varlen attention over the packed prompt tokens in ``qkv``; returns [T, Hq*hd].
    ``window`` > 0: sliding-window attention (the query at position p sees the keys
    p - window < j <= p); 0 = full attention."""
    window = max(int(window), 0)
    T = qkv.shape[0]
    if not _use_native(qkv):
        q, k, v = R.split_qkv(qkv, hq, hkv, hd)
        o = R.prefill_attention(q, k, v, cu_seqlens, scale, window).reshape(T, hq * hd)
        if out is not None:
            out.copy_(o)
            return out
        return o
    if out is None:
        out = torch.empty(T, hq * hd, dtype=qkv.dtype, device=qkv.device)
    nseq = cu_seqlens.shape[0] - 1
    _native_call("dli_prefill_attention", _p(out), out.stride(0), _p(qkv), qkv.stride(0),
                 _p(cu_seqlens), nseq, max_seqlen, hq, hkv, hd, scale, window, _st())
    return out


def decode_pipelined(v: int) -> int:
    """Select the pipelined (1), one-tile-per-round (0) or automatic (2, the default: pipelined
    for KV splits of >= 768 tokens) decode attention kernel for head_dim 128. Returns the
    previous setting (tests force either kernel with it)."""
    return int(N.require_native().dli_decode_set_pipe(int(v)))


def decode_form(v: int) -> int:
    """Force the unsplit decode attention's form: 1 = a wave per (sequence, kv head), 4 = a
    workgroup per item, 0 = automatic (workgroup per item for <= 256 items). Returns the
    previous setting (tests force either form with it)."""
    return int(N.require_native().dli_decode_set_form(int(v)))


def prefill_long_min_len(n: int = 0) -> int:
    """Shortest max_seqlen routed to the 256-row (32x32x16) prefill attention kernel; n > 0
    sets it. Returns the previous value (A/B runs and tests force either kernel with it)."""
    return int(N.require_native().dli_prefill_set_min_len(int(n)))


def prefill_set_pack(on: bool) -> bool:
    """Head packing of the short-prompt prefill attention kernel (2 / 4 query heads of a GQA
    group per workgroup when every prompt of the batch is <= 32 / 16 tokens); returns the
    previous setting (A/B switch, on by default)."""
    return bool(N.require_native().dli_prefill_set_pack(1 if on else 0))


def prefill_attention_paged(qkv, cu_seqlens, max_seqlen: int, context_lens, block_tables,
                            k_cache, v_cache, hq, hkv, hd, scale, out=None, window: int = 0,
                            k_scale: float = 1.0, v_scale: float = 1.0):
    """Chunked prefill attention: each sequence's chunk of queries (packed rows of ``qkv``)
    attends over all ``context_lens[i]`` keys of the sequence in the paged cache — earlier
    chunks plus this one (already written by ``rope_and_cache``); [T, Hq*hd]. ``window`` > 0:
    each query sees the last ``window`` keys up to its own position. ``k_scale`` /
    ``v_scale``: the scales of an FP8 cache (every chunk length then takes the 64-row kernel)."""
    window = max(int(window), 0)
    T = qkv.shape[0]
    fp8 = kv_cache_is_fp8(k_cache, v_cache, k_scale, v_scale, native=_use_native(qkv))
    if not _use_native(qkv):
        q = qkv[:, : hq * hd].reshape(T, hq, hd)
        o = R.prefill_attention_paged(q, k_cache, v_cache, cu_seqlens, context_lens,
                                      block_tables, scale, window, k_scale,
                                      v_scale).reshape(T, hq * hd)
        if out is not None:
            out.copy_(o)
            return out
        return o
    if out is None:
        out = torch.empty(T, hq * hd, dtype=qkv.dtype, device=qkv.device)
    nseq = cu_seqlens.shape[0] - 1
    _native_call("dli_prefill_attention_paged", _p(out), out.stride(0), _p(qkv), qkv.stride(0),
                 _p(cu_seqlens), _p(context_lens), _p(k_cache), _p(v_cache), _p(block_tables),
                 block_tables.stride(0), nseq, max_seqlen, hq, hkv, hd, k_cache.shape[2], scale,
                 window, int(fp8), float(k_scale), float(v_scale), _st())
    return out


def decode_span(max_context: int, window: int = 0) -> int:
    """The most keys a decode query attends over: the context, or the sliding window."""
    return min(max_context, window) if window > 0 else max_context


def decode_num_splits(B: int, hkv: int, max_context: int) -> int:
    """KV splits so that the B*Hkv*splits work items (one wave each) fill the chip's ~2048
    resident waves for long contexts, keeping >= 128 tokens per split. With a sliding window
    pass the span (``decode_span``): the splits divide the window, not the context."""
    items = B * hkv
    splits = 1
    # tiny batches (batch-1 latency): >= 512 tokens per split, so graphs captured for a
    # 512-token table take the single-pass kernel with the fused QKV reduce / RoPE / cache
    # prologue (the 4-split form cost rope + attention + merge = 23 us per layer at B = 1,
    # profiles/r3/prof_b1_summary.txt)
    min_tok = 512 if B <= 4 else 128
    while items * splits < 2048 and max_context // (splits * 2) >= min_tok and splits < 64:
        splits *= 2
    return splits


def decode_attention(qkv, k_cache, v_cache, block_tables, context_lens, max_context: int,
                     hq, hkv, hd, scale, out=None, num_splits: Optional[int] = None,
                     window: int = 0, k_scale: float = 1.0, v_scale: float = 1.0):
    """One query per row of ``qkv`` (rows = sequences) against its paged KV; [B, Hq*hd].
    ``window`` > 0: sliding-window attention, sequence b attends over the keys
    [max(0, context_lens[b] - window), context_lens[b]). ``k_scale`` / ``v_scale``: the
    scales of an FP8 cache (the wave-per-item kernel of attention_decode_fp8.hip)."""
    B = qkv.shape[0]
    window = max(int(window), 0)
    fp8 = kv_cache_is_fp8(k_cache, v_cache, k_scale, v_scale, native=_use_native(qkv))
    if not _use_native(qkv):
        q = qkv[:, : hq * hd].reshape(B, hq, hd)
        o = R.decode_attention(q, k_cache, v_cache, block_tables, context_lens,
                               scale, window, k_scale, v_scale).reshape(B, hq * hd)
        if out is not None:
            out.copy_(o)
            return out
        return o
    if out is None:
        out = torch.empty(B, hq * hd, dtype=qkv.dtype, device=qkv.device)
    if num_splits is None:
        num_splits = decode_num_splits(B, hkv, decode_span(max_context, window))
    ws = None
    if num_splits > 1:
        ws = G.workspace(qkv.device, int(N.require_native().dli_decode_attention_workspace_bytes(
            B, hq, hd, num_splits)))
    _native_call("dli_decode_attention", _p(out), _p(qkv), qkv.stride(0), _p(k_cache),
                 _p(v_cache), _p(block_tables), block_tables.stride(0), _p(context_lens), B, hq,
                 hkv, hd, k_cache.shape[2], scale, max_context, num_splits, _p(ws), window,
                 int(fp8), float(k_scale), float(v_scale), _st())
    return out


# ----------------------------------------------------------------------------- sampling
_sample_wss: dict = {}


def _sample_ws(device, B: int, V: int):
    """Zero-initialised scratch of the two-phase small-batch sampler (sampling.hip
    sample_chunk_kernel: B <= 8 rows split over up to 64 workgroups each), or None. One buffer
    per device, sized for the largest batch; the kernels leave its overflow flags zero."""
    lib = N.require_native()
    if int(lib.dli_sample_workspace_bytes(B, V)) == 0:
        return None
    key = (device.type, device.index)
    ws = _sample_wss.get(key)
    nbytes = int(lib.dli_sample_workspace_bytes(B, V))
    if ws is None or ws.numel() < nbytes:
        # sized for the largest two-phase batch (the library's split limit; 8 by default)
        maxb = int(lib.dli_sample_set_split_max_b(0))
        nbytes = max(nbytes, int(lib.dli_sample_workspace_bytes(maxb, V)))
        if ws is not None:
            G._retired.append(ws)        # a captured graph may still hold it (ops.gemm)
        ws = _sample_wss[key] = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    return ws


# LM-head output dtype: fp32 (the head GEMM accumulates in fp32 and stores it). bf16 logits
# were measured without a gain at batch 512 (profiles/r5/s05/ab.jsonl: the head GEMM is
# MFMA-bound at the same 407 us either way) and make a request's draws depend on which GEMM
# plan (batch size) rounded its logits, which breaks batch-invariant seeded sampling.
HEAD_EPI = "f32"


def sample(logits, temperature, top_k, top_p, seeds, generator=None, ids=None):
    """logits fp32 or bf16 [B, V] -> int32 tokens [B] (every comparison on the exact fp32
    value of each logit). temperature<=0 -> greedy. With ``ids``
    [B, V] the row holds candidates (vocab-parallel LM head) in ascending token-id order,
    and the sampled column is mapped to its token id (ties then break by token id exactly
    as over the full vocabulary)."""
    if not _use_native(logits):
        return R.sample(logits, temperature, top_k, top_p, generator=generator, seeds=seeds,
                        ids=ids)
    B, V = logits.shape
    out = torch.empty(B, dtype=torch.int32, device=logits.device)
    if logits.dtype not in (torch.float32, torch.bfloat16):
        logits = logits.float()
    fn = "dli_sample_bf16" if logits.dtype == torch.bfloat16 else "dli_sample"
    _native_call(fn, _p(out), _p(logits), logits.stride(0), B, V, _p(temperature),
                 _p(top_k), _p(top_p), _p(seeds), _p(_sample_ws(logits.device, B, V)), _st())
    if ids is not None:
        out = ids.gather(1, out.long().unsqueeze(1)).squeeze(1).to(torch.int32)
    return out


def head_candidates(h, w_slice, offset: int, c: int):
    """Vocab-parallel LM head slice on this rank: logits (``HEAD_EPI``: the model dtype, as
    the single-stage head) for token ids ``[offset, offset + V_r)`` and the top-``c`` per
    row (ties broken by the lower token id), returned in ascending token-id order (values
    fp32 [S, c], ids int32 [S, c]). The union over ranks contains every token a top-k <= c
    sampler can pick."""
    lg = linear(h, w_slice, epi=HEAD_EPI)
    S, V = lg.shape
    c = min(c, V)
    if not _use_native(h):
        # stable descending sort: equal logits keep ascending token-id order
        v, i = torch.sort(lg.float(), dim=-1, descending=True, stable=True)
        v, i = v[:, :c], (i[:, :c] + offset).to(torch.int32)
        i, perm = torch.sort(i, dim=-1)
        return v.gather(1, perm), i
    v = torch.empty(S, c, dtype=torch.float32, device=h.device)
    i = torch.empty(S, c, dtype=torch.int32, device=h.device)
    # HIP top-c per row, written in ascending id order (sampling.hip topk_rows_kernel)
    fn = "dli_topk_rows_bf16" if lg.dtype == torch.bfloat16 else "dli_topk_rows"
    _native_call(fn, _p(v), _p(i), _p(lg), lg.stride(0), S, V, c, int(offset), _st())
    return v, i


# ----------------------------------------------------------------------------- MoE
def moe_route(router_logits, k: int, norm_topk: bool = True):
    """softmax -> top-``k`` (lowest index on ties) -> weights p / sum(all), divided by the sum
    of the picks when ``norm_topk``; up to 256 experts, k <= 8 past 64 (``moe_route_kernel``)."""
    if not _use_native(router_logits):
        return R.router_topk(router_logits, k, norm_topk)
    T, E = router_logits.shape
    w = torch.empty(T, k, dtype=torch.float32, device=router_logits.device)
    ids = torch.empty(T, k, dtype=torch.int32, device=router_logits.device)
    _native_call("dli_moe_route", _p(w), _p(ids), _p(router_logits), T, E, k, int(norm_topk),
                 _st())
    return w, ids


def moe_router(h, w_router, k: int, norm_topk: bool = True):
    """The MoE gate: logits = h @ w_router.T (bf16, as a GEMM would write them), softmax,
    top-``k``, renormalised when ``norm_topk``. On the GPU with <= 8 experts and renormalised
    weights one kernel does all of it (``moe_router_kernel``, a workgroup per token); else the
    GEMM then ``moe_route``."""
    T, D = h.shape
    E = w_router.shape[0]
    if (_use_native(h) and E <= 8 and norm_topk and D % 8 == 0 and h.stride(-1) == 1
            and h.stride(0) % 8 == 0 and w_router.is_contiguous()
            and h.data_ptr() % 16 == 0 and w_router.data_ptr() % 16 == 0):
        w = torch.empty(T, k, dtype=torch.float32, device=h.device)
        ids = torch.empty(T, k, dtype=torch.int32, device=h.device)
        _native_call("dli_moe_router", _p(w), _p(ids), _p(h), h.stride(0), _p(w_router), T, E,
                     D, k, _st())
        return w, ids
    return moe_route(linear(h, w_router), k, norm_topk)


def moe_mlp(x, w_gu, w_down, topk_w, topk_ids, expert_offset: int = 0,
            plan_rows: Optional[int] = None, defer_combine: bool = False):
    """Experts [expert_offset, expert_offset+E_local) of one MoE layer; returns the weighted
    sum over the token's selected local experts (zeros for tokens routed elsewhere).
    ``plan_rows``: the routed rows these experts typically receive, when ``x`` is a region
    sized for the worst case (the expert-parallel receive region: every peer's bucket at
    min(k, E/N) rows per token). The grouped-GEMM plan is looked up for it — the autotuned
    key — instead of for the capacity, whose 4-8x larger row count mapped to 256-row tiles
    (1 workgroup per CU) that streamed the experts at ~2 TB/s.
    With more than ``G.LIST_MIN_GROUPS`` local experts (Qwen3-MoE) the grouped GEMMs of the
    generic tile family run on the compact grid over the align step's tile list
    (``G.list_plan``), whose size does not grow as rows x experts."""
    if not _use_native(x):
        return R.moe_mlp(x, _dense(w_gu), _dense(w_down), topk_w, topk_ids, expert_offset)
    T, D = x.shape
    k = topk_ids.shape[1]
    E_local, F2, _ = w_gu.shape
    n = T * k
    dev = x.device
    offsets = torch.empty(E_local + 1, dtype=torch.int32, device=dev)
    pos = torch.empty(n, dtype=torch.int32, device=dev)
    src = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    prefill = (n >= _MOE_PREFILL_ROWS * E_local
               and not torch.cuda.is_current_stream_capturing())
    rows = plan_rows if plan_rows is not None else n
    # FP8 expert stacks (Fp8Experts): a decode step streams them (dli_gemm_fp8_stream_grouped)
    # where the plan is a stream tile the call can take; else the bf16 plan below runs on the
    # stack's bf16 image, dequantised right before its GEMM (one scratch for both stacks)
    sbm = G.fp8_grouped_bm(rows, E_local)
    p_gu, st_gu = _expert_plan(w_gu, rows, n, F2, D, "silu_mul", E_local, sbm,
                               not prefill and _rows_aligned(x) and x.is_contiguous())
    p_dn, st_dn = _expert_plan(w_down, rows, n, D, F2 // 2, "none", E_local, sbm, not prefill)
    # one tile list per row-tile height that the two projections run on the compact grid
    lists = {}
    if not prefill and n > 0:
        for p, st in ((p_gu, st_gu), (p_dn, st_dn)):
            bm = sbm if st else G.TILES[p.tile][0]
            if (st or G.list_plan(p, E_local)) and bm not in lists:
                cap = G.max_items(n, E_local, bm)
                lists[bm] = (torch.empty(1 + cap, 2, dtype=torch.int32, device=dev), cap)
    if lists:
        a, b = (list(lists.items()) + [(0, (None, 0))])[:2]      # (bm, (list, max items))
        _native_call("dli_moe_align_tiles", _p(offsets), _p(pos), _p(src), _p(topk_ids), n, k,
                     expert_offset, E_local, _p(a[1][0]), a[0], a[1][1], _p(b[1][0]), b[0],
                     b[1][1], _st())
    else:
        _native_call("dli_moe_align", _p(offsets), _p(pos), _p(src), _p(topk_ids), n, k,
                     expert_offset, E_local, _st())
    tl_gu = tl_dn = None
    if not st_gu and G.list_plan(p_gu, E_local):
        tl_gu = lists.get(G.TILES[p_gu.tile][0])
    if not st_dn and G.list_plan(p_dn, E_local):
        tl_dn = lists.get(G.TILES[p_dn.tile][0])
    act = torch.empty(max(n, 1), F2 // 2, dtype=x.dtype, device=dev)
    if prefill:
        # prefill-sized expert GEMMs (thousands of rows per expert) are compute-bound: a
        # grouped 256x256 kernel (G.MOE_PREFILL_TILE: the two-barrier 4-wave tile, grid.z =
        # expert) with the fused SiLU*up epilogue. The largest expert's row count bounds the
        # grid (one host read of the offsets per MoE layer, eager prefill only) instead of n,
        # which would launch ~8x more (empty) row tiles per expert.
        xp = torch.empty(max(n, 1), D, dtype=x.dtype, device=dev)
        _native_call("dli_moe_gather", _p(xp), _p(x), _p(src), n, D, _p(offsets[E_local:]),
                     _st())
        offs = offsets.tolist()
        rows_max = max(b - a for a, b in zip(offs[:-1], offs[1:]))
        y = torch.empty(max(n, 1), D, dtype=x.dtype, device=dev)
        if rows_max > 0:
            p8 = G.GemmPlan("dli", G.MOE_PREFILL_TILE, 1)
            _gemm_native(xp, _stack(w_gu), "silu_mul", out=act, groups=E_local,
                         group_off=offsets, rows_per_group=rows_max, plan=p8)
            _gemm_native(act, _stack(w_down), "none", out=y, groups=E_local, group_off=offsets,
                         rows_per_group=rows_max, plan=p8)
        out = torch.empty_like(x)
        _native_call("dli_moe_combine", _p(out), _p(y), _p(topk_w), _p(pos), T, k, D, _st())
        return out
    if st_gu:                            # token rows read through the permutation, as below
        grouped_fp8_stream(x, w_gu, p_gu, "silu_mul", act, offsets, n, sbm, lists[sbm], src)
    elif p_gu.splits == 1 and p_gu.tile in G.GATHER_TILES and x.is_contiguous():
        w_gu = _stack(w_gu)
        # the gate/up GEMM reads the token rows in place through the permutation (no gathered
        # copy of them: dli_gemm_grouped_gather, the generic tile family)
        # (on the compact grid: dli_gemm_grouped_list with the same row permutation)
        _launch_gemm("gemm", x, w_gu, p_gu, G.EPI["silu_mul"], act, act.stride(0), n, F2, D,
                     group_off=offsets, groups=E_local, tile_list=tl_gu, arow=src)
    else:
        # permuted rows: at most n (all local); rows past offsets[E_local] are never touched
        xp = torch.empty(max(n, 1), D, dtype=x.dtype, device=dev)
        xc = x if x.is_contiguous() else x.contiguous()      # (the gather reads D-strided rows)
        _native_call("dli_moe_gather", _p(xp), _p(xc), _p(src), n, D, _p(offsets[E_local:]),
                     _st())
        _gemm_native(xp, _stack(w_gu), "silu_mul", out=act, groups=E_local, group_off=offsets,
                     rows_per_group=n, plan=p_gu, tile_list=tl_gu)
    if st_dn:
        y = torch.empty(max(n, 1), D, dtype=x.dtype, device=dev)
        grouped_fp8_stream(act, w_down, p_dn, "none", y, offsets, n, sbm, lists[sbm])
        out = torch.empty_like(x)
        _native_call("dli_moe_combine", _p(out), _p(y), _p(topk_w), _p(pos), T, k, D, _st())
        return out
    w_down = _stack(w_down)
    if moe_slab_plan(p_dn):
        if defer_combine:
            # the down projection's slabs; the combine runs with the next layer's add + norm
            ws = _moe_down_slabs(act, w_down, offsets, n, p_dn, tl_dn)
            return MoEPending(ws, p_dn.splits, n, topk_w, pos, (T, D), x.dtype, dev)
        out = torch.empty_like(x)
        moe_down_combine(act, w_down, offsets, n, p_dn, topk_w, pos, out, tile_list=tl_dn)
        return out
    y = torch.empty(max(n, 1), D, dtype=x.dtype, device=dev)
    _gemm_native(act, w_down, "none", out=y, groups=E_local, group_off=offsets,
                 rows_per_group=n, plan=p_dn, tile_list=tl_dn)
    out = torch.empty_like(x)
    _native_call("dli_moe_combine", _p(out), _p(y), _p(topk_w), _p(pos), T, k, D, _st())
    return out


def _stack(w):
    """The [E, N, K] tensor the bf16 grouped GEMMs read for an expert stack."""
    return w.bf16() if isinstance(w, Fp8Experts) else w


def _rows_aligned(x) -> bool:
    return x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0 and x.stride(-1) == 1


def _expert_plan(w, rows: int, n: int, Nn: int, K: int, epi: str, groups: int, bm: int,
                 form_ok: bool):
    """(plan, streams) of one expert projection of ``moe_mlp``: a bf16 stack's grouped plan as
    ever; an ``Fp8Experts`` stack's plan under the FP8 key, which streams when it is a stream
    tile that takes the call (``stream_ok``, ``form_ok``: a decode step with aligned rows)
    and else gives way to a bf16-family plan of the dequantise path, so a stream tile id
    never reaches ``dli_gemm``."""
    if not isinstance(w, Fp8Experts):
        p = G.grouped_plan(rows, Nn, K, epi, groups)
        if p.tile in G.FP8_STREAM_TILES:
            raise ValueError(f"GEMM tile {p.tile} streams FP8 block-scaled weights "
                             f"(ops.Fp8Experts) only, got a {w.dtype} stack")
        return p, False
    p = G.grouped_plan(rows, Nn, K, epi, groups, "fp8")
    if p.tile not in G.FP8_STREAM_TILES:
        return p, False
    if (form_ok and n > 0 and w.stream_ok(n, groups, p)
            and G.max_items(n, groups, bm) <= 65535):
        return p, True
    return G.grouped_plan(rows, Nn, K, epi, groups), False


def grouped_fp8_stream(x, w: "Fp8Experts", p: G.GemmPlan, epi: str, out, offsets, n: int,
                       bm: int, tile_list, arow=None):
    """out[r] = epi(x[arow[r] or r] @ W[e(r)].T) for the ``n`` permuted rows whose experts
    ``offsets`` delimits, on the grouped FP8 MFMA stream: ``tile_list`` = (list, max items)
    of the align step for ``bm``-row items. Rows past ``offsets[-1]`` are not written."""
    E, Nn, K = w.shape
    _native_call("dli_gemm_fp8_stream_grouped", _p(x), x.stride(0), _p(w.q), _p(w.scale),
                 w.scale.stride(1), K, _p(out), out.stride(0), n, Nn, K, G.EPI[epi], p.tile,
                 p.splits, bm, _p(arow), _p(offsets), E, _p(tile_list[0]), tile_list[1], _st())
    return out


def moe_slab_plan(p: Optional[G.GemmPlan]) -> bool:
    """Whether a grouped down-projection plan runs as fp16 split-K slabs reduced inside the
    combine (``moe_down_combine``) instead of GEMM -> fp32 slab reduce -> bf16 y -> combine."""
    return (p is not None and G.SLAB16 and p.splits in (2, 4, 8)
            and p.tile in G.SLAB16_TILES)


def _moe_down_slabs(act, w_down, offsets, n: int, p: G.GemmPlan, tile_list=None):
    """Grouped down projection of the ``n`` permuted rows ``act`` as ``p.splits`` fp16 split-K
    slabs (EPI "slab16") in the workspace, which is returned; ``tile_list``: on the compact
    grid (``_gemm_native``)."""
    E_local, D, F = w_down.shape
    ws = G.workspace(act.device, p.splits * max(n, 1) * D * 2)
    _launch_gemm("gemm", act, w_down, p, G.EPI["slab16"], None, D, n, D, F, ws=ws,
                 group_off=offsets, groups=E_local, tile_list=tile_list)
    return ws


def moe_down_combine(act, w_down, offsets, n: int, p: G.GemmPlan, topk_w, pos, out,
                     tile_list=None):
    """Grouped down projection of the ``n`` permuted rows ``act`` as fp16 split-K slabs
    (``_moe_down_slabs``), reduced by the combine itself: out[t] = sum_j topk_w[t, j] *
    bf16(sum_s slab_s[pos[t * k + j]]) (csrc/kernels/moe.hip moe_combine_slabs_kernel)."""
    D = w_down.shape[1]
    ws = _moe_down_slabs(act, w_down, offsets, n, p, tile_list)
    T, k = topk_w.shape                  # pos: [T * k] rows (flat, as moe_align writes it)
    _native_call("dli_moe_combine_slabs", _p(out), _p(ws), p.splits, n, _p(topk_w), _p(pos),
                 T, k, D, _st())
    return out


def ep_pack(x, topk_ids, e_per: int, base, send_rows: int, counts: bool = False):
    """Expert-parallel dispatch: (token, pick) rows into per-destination-rank buckets
    starting at ``base[dest]`` (int32 [N] on the device). Returns (send_x [send_rows, D],
    send_e int32 [send_rows] global expert id or -1, pos int32 [T, k] row of each pick)
    and, with ``counts``, the rows per destination (int32 [N] on the device)."""
    T, D = x.shape
    k = topk_ids.shape[1]
    dev = x.device
    send_x = torch.empty(max(send_rows, 1), D, dtype=x.dtype, device=dev)[:send_rows]
    send_e = torch.full((send_rows,), -1, dtype=torch.int32, device=dev)
    pos = torch.empty(T, k, dtype=torch.int32, device=dev)
    if not _use_native(x):
        # deterministic reference: slots in (token, pick) order
        fill = [0] * base.shape[0]
        bl = base.tolist()
        ids = topk_ids.tolist()
        for t in range(T):
            for j in range(k):
                d = ids[t][j] // e_per
                p = bl[d] + fill[d]
                fill[d] += 1
                pos[t, j] = p
                send_e[p] = ids[t][j]
                send_x[p] = x[t]
        if counts:
            return send_x, send_e, pos, torch.tensor(fill, dtype=torch.int32)
        return send_x, send_e, pos
    fill = torch.zeros(base.shape[0], dtype=torch.int32, device=dev)
    if T > 0:
        _native_call("dli_ep_pack", _p(send_x), _p(send_e), _p(pos), _p(fill), _p(base), _p(x),
                     _p(topk_ids), T, k, D, e_per, _st())
    if counts:
        return send_x, send_e, pos, fill
    return send_x, send_e, pos


def moe_combine(y, topk_w, pos):
    """out[t] = sum_j topk_w[t, j] * y[pos[t, j]] (fp32 sum in j order, bf16 out); pos < 0
    rows contribute nothing."""
    T, k = pos.shape
    D = y.shape[1]
    if not _use_native(y):
        out = torch.zeros(T, D, dtype=torch.float32, device=y.device)
        for j in range(k):
            pj = pos[:, j].long()
            ok = pj >= 0
            out[ok] += topk_w[ok, j:j + 1].float() * y[pj[ok]].float()
        return out.to(y.dtype)
    out = torch.empty(T, D, dtype=y.dtype, device=y.device)
    _native_call("dli_moe_combine", _p(out), _p(y), _p(topk_w), _p(pos), T, k, D, _st())
    return out


# ----------------------------------------------------------------------------- misc
def native_library_path():
    return N.loaded_path()


def benchmark(fn, iters: int = 20, warmup: int = 3, graph: bool = False) -> float:
    """Median milliseconds of fn() on the current stream (GPU) or wall clock (CPU).
    ``graph=True`` captures fn() in a HIP graph and times replays: the GPU time of a
    launch-bound sequence as a decode graph runs it. Timed eagerly, a batch-1 GEMM (~15 us)
    plus its consumer kernel cost less GPU time than the host spends launching them, so the
    autotuner compared host launch overheads and picked plans at random (two runs of the
    same bench took different decode paths)."""
    for _ in range(warmup):
        fn()
    if graph and torch.cuda.is_available():
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        g.replay()
        torch.cuda.synchronize()
        times = []
        for _ in range(iters):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            g.replay()
            e.record()
            e.synchronize()
            times.append(s.elapsed_time(e))
        del g
        times.sort()
        return times[len(times) // 2]
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        times = []
        for _ in range(iters):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            times.append(s.elapsed_time(e))
    else:
        times = []
        for _ in range(iters):
            t0 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return times[len(times) // 2]
