"""Launch traces of the linear ops: which native entries a call reaches, in which order and
with which arguments, recorded on CPU tensors with the native layer stubbed out. The Python
side of a linear op decides the kernel, the plan fallback, the workspace size and every
marshalled argument; none of that needs a device to be observed.

The recorder replaces a few seams of ``ops`` (``_native_call``, ``_use_native``, ``_st``,
``_p``, ``Fp8Weight.bf16``), ``G.workspace``, ``N.require_native`` and
``torch.cuda.is_current_stream_capturing``; nothing else, so this file runs unchanged against
any revision that keeps those names. ``_p`` is replaced only to keep every tensor whose address
was taken alive until the case ends: a freed temporary's address could be handed out again and
two buffers would share a label.

An event is ``[name, arg, ...]``. Arguments are normalised with ``N._SIGS[name]``: a pointer
becomes ``"<label>+<byte offset>"`` of the case's tensor it points into, ``"ws+.."`` for the
workspace, ``"new<i>+.."`` for a buffer first seen in this case (numbered by first appearance)
or None; every other argument is recorded as is. ``["bf16()"]`` (a dequantise pass: a launch)
and a final ``["return", value]`` are events too. The byte counts asked of ``G.workspace`` are
kept beside the trace, in order: a request is no launch, and where it falls between two
launches is not behaviour.

    python tests/linear_trace.py --record tests/linear_trace_golden.json
    python tests/linear_trace.py --time        # host cost of a call, see ``host_cost``

The golden file is recorded in a checkout of the revision a change is compared against, never
in the tree under test.
"""
from __future__ import annotations

import argparse
import contextlib
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path
from typing import Optional

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from distributed_llm_inferencing_amd import ops  # noqa: E402
from distributed_llm_inferencing_amd.ops import _native as N  # noqa: E402
from distributed_llm_inferencing_amd.ops import gemm as G  # noqa: E402
from distributed_llm_inferencing_amd.ops import reference as R  # noqa: E402

GOLDEN = Path(__file__).with_name("linear_trace_golden.json")
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
K0, N0 = 1024, 256
HQ, HKV, HD = 4, 2, 128
NQKV = (HQ + 2 * HKV) * HD


class _Lib:
    @staticmethod
    def dli_decode_uses_pipe(*a):
        return 0


class Recorder:
    """One case's tensors and events. ``t`` makes a labelled tensor; ``patched()`` installs
    the stubs."""

    def __init__(self, record: bool = True):
        self.record = record
        self.events, self.ws_bytes, self.keep = [], [], []
        self.bufs = {}                   # storage address -> (label, bytes)
        self.new = 0
        self.ws = None

    # ---- tensors
    def know(self, label: Optional[str], t: torch.Tensor) -> torch.Tensor:
        s = t.untyped_storage()
        self.bufs[s.data_ptr()] = (label, s.nbytes())
        self.keep.append(t)
        return t

    def t(self, label: str, *shape, dtype=BF16) -> torch.Tensor:
        return self.know(label, torch.zeros(*shape).to(dtype))

    def fp8w(self, n: int = N0, k: int = K0) -> "ops.Fp8Weight":
        return ops.Fp8Weight(self.t("w.q", n, k, dtype=R.FP8_W),
                             self.know("w.scale", torch.ones(n // 16, -(-k // 128))))

    def label(self, ptr):
        if not ptr:
            return ptr                   # None, or the stub stream 0
        for base, (label, nbytes) in self.bufs.items():
            if base <= ptr < base + max(nbytes, 1):
                if label is None:        # a buffer the op made: numbered where it first shows
                    label = f"new{self.new}"
                    self.new += 1
                    self.bufs[base] = (label, nbytes)
                return f"{label}+{ptr - base}"
        raise AssertionError(f"pointer {ptr:#x} of no tensor the recorder has seen")

    def value(self, v):
        """A return value as data."""
        if isinstance(v, torch.Tensor):
            self._p(v)                   # a tensor the op made: a new buffer, or a view
            return {"ptr": self.label(v.data_ptr()), "shape": list(v.shape),
                    "dtype": str(v.dtype)}
        if isinstance(v, ops.MoEPending):
            return {"pending": [self.value(v.ws)["ptr"], v.splits, v.rows, list(v.shape)]}
        if isinstance(v, (tuple, list)):
            return [self.value(x) for x in v]
        assert v is None or isinstance(v, (bool, int, float)), type(v)
        return v

    # ---- the stubs
    def _p(self, t):
        if t is None:
            return None
        base = t.untyped_storage().data_ptr()
        if base not in self.bufs:
            self.know(None, t)
        return t.data_ptr()

    def _call(self, name, *args):
        sig = N._SIGS[name]
        assert len(args) == len(sig), (name, len(args), len(sig))
        self.events.append([name] + [self.label(a) if ty is ctypes.c_void_p else a
                                     for a, ty in zip(args, sig)])

    def _workspace(self, device, nbytes):
        if self.record:
            self.ws_bytes.append(int(nbytes))
        if self.ws is None or self.ws.numel() < nbytes:
            self.ws = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8)
            if self.record:
                self.know("ws", self.ws)
        return self.ws

    @contextlib.contextmanager
    def patched(self):
        orig_bf16 = ops.Fp8Weight.bf16
        rec = self

        def bf16(self):
            if rec.record:
                rec.events.append(["bf16()"])
            return orig_bf16(self)

        seams = [(ops, "_use_native", lambda t: True), (ops, "_st", lambda: 0),
                 (G, "workspace", self._workspace), (N, "require_native", lambda: _Lib),
                 (torch.cuda, "is_current_stream_capturing", lambda: False),
                 (ops.Fp8Weight, "bf16", bf16)]
        if self.record:
            seams += [(ops, "_native_call", self._call), (ops, "_p", self._p)]
        else:
            seams += [(ops, "_native_call", lambda name, *a: None)]
        old = [(o, n, getattr(o, n)) for o, n, _ in seams]
        saved = [(c, c.copy()) for c in (G._plan_cache, G._grouped_cache, G._tuned)]
        for c, _ in saved:
            c.clear()
        try:
            for o, n, f in seams:
                setattr(o, n, f)
            yield self
        finally:
            for o, n, f in old:
                setattr(o, n, f)
            for c, was in saved:
                c.clear()
                c.update(was)


# --------------------------------------------------------------------------------- cases
def P(tile: int, splits: int) -> G.GemmPlan:
    return G.GemmPlan("dli", tile, splits)


def _w(r: Recorder, kind: str, n: int = N0):
    """kind: "bf16", "fp8", or "fp8odd" (K = 1032: no 16-element chunks per K slice)."""
    if kind == "bf16":
        return r.t("w", n, K0)
    return r.fp8w(n, 1032 if kind == "fp8odd" else K0)


def _x(r: Recorder, M: int, w, label: str = "x"):
    return r.t(label, M, w.shape[-1])


def _normed(r: Recorder, M: int, w):
    return ops.NormedRows(_x(r, M, w, "h"), r.t("h.w", w.shape[-1]), 1e-5)


def _set(w, M, epi, plan, n=None):
    G.set_plan(M, n or w.shape[0], w.shape[-1], epi, plan, G.wdt(w))


CASES = {}          # name -> (forced plan or None, fn(recorder) -> return value)


def case(name, plan=None):
    def add(fn):
        assert name not in CASES, name
        CASES[name] = (plan, fn)
        return fn
    return add


def _linear_cases():
    for M in (1, 3, 4, 5, 8, 64, 65, 300):
        for kind in ("bf16", "fp8") + (("fp8odd",) if M in (1, 8) else ()):
            @case(f"linear/heuristic/{kind}/M{M}")
            def _(r, M=M, kind=kind):
                w = _w(r, kind)
                return ops.linear(_x(r, M, w), w)
    for kind, M in (("bf16", 8), ("fp8", 1)):
        for epi in ("none", "f32", "silu_mul", "bias_gelu", "bias"):
            @case(f"linear/epi/{kind}/M{M}/{epi}")
            def _(r, M=M, kind=kind, epi=epi):
                w = _w(r, kind)
                bias = r.t("bias", N0) if epi.startswith("bias") else None
                return ops.linear(_x(r, M, w), w, bias, "none" if epi == "bias" else epi)
    for epi in ("none", "silu_mul"):
        @case(f"linear/out/{epi}")
        def _(r, epi=epi):
            w = _w(r, "bf16")
            out = r.t("out", 8, N0 // 2 if epi == "silu_mul" else N0)
            return ops.linear(_x(r, 8, w), w, epi=epi, out=out)

    # NormedRows: a prologue tile (the heuristic's at M <= 4), split and unsplit, a tile
    # without a prologue, more rows than the GEMV takes, an FP8 weight the stream refuses
    for kind, epi, M, plan in (("bf16", "none", 1, None), ("bf16", "none", 4, None),
                               ("fp8", "silu_mul", 1, None), ("fp8", "none", 3, None),
                               ("bf16", "none", 1, P(30, 2)), ("fp8", "none", 1, P(56, 2)),
                               ("bf16", "none", 1, P(0, 1)), ("bf16", "silu_mul", 1, P(0, 2)),
                               ("bf16", "none", 2, P(32, 1)), ("bf16", "none", 5, None),
                               ("fp8odd", "none", 1, None), ("bf16", "bias_gelu", 1, None)):
        tag = "heur" if plan is None else f"t{plan.tile}s{plan.splits}"

        @case(f"linear/normed/{kind}/{epi}/M{M}/{tag}", plan)
        def _(r, kind=kind, epi=epi, M=M, plan=plan):
            w = _w(r, kind)
            if plan is not None:
                _set(w, M, epi, plan)
            bias = r.t("bias", N0) if epi == "bias_gelu" else None
            return ops.linear(_normed(r, M, w), w, bias, epi)

    @case("linear/normed/out")
    def _(r):
        w = _w(r, "bf16")
        return ops.linear(_normed(r, 1, w), w, out=r.t("out", 1, N0))

    for name, mk in (("x", lambda r, w: (r.t("x", 8, 2 * K0)[:, ::2], w)),
                     ("w", lambda r, w: (_x(r, 8, w), r.t("w2", N0, 2 * K0)[:, ::2]))):
        @case(f"linear/error/inner-stride-{name}")
        def _(r, mk=mk):
            x, w = mk(r, _w(r, "bf16"))
            return ops.linear(x, w)


def _gemm_native_cases():
    table = []
    for plan in (P(30, 1), P(30, 2), P(56, 1), P(56, 2)):
        table += [("fp8", 1, "none", plan), ("fp8", 4, "none", plan), ("bf16", 1, "none", plan)]
    table += [("fp8", 5, "none", P(30, 2)), ("fp8odd", 1, "none", P(30, 1)),
              ("fp8", 1, "silu_mul", P(29, 1)), ("fp8", 1, "silu_mul", P(29, 2)),
              ("bf16", 3, "silu_mul", P(29, 1)), ("fp8", 1, "bias_gelu", P(30, 1))]
    for plan in (P(0, 1), P(0, 2), P(45, 2)):
        table += [("bf16", 8, "none", plan), ("fp8", 300, "none", plan)]
    for plan in (P(70, 1), P(70, 2), P(71, 1), P(71, 2)):
        table += [("fp8", 5, "none", plan), ("fp8", 64, "none", plan)]
    table += [("fp8", 8, epi, P(70, 2)) for epi in ("f32", "silu_mul", "bias", "splitk")]
    # stream plans the call cannot take: the heuristic plan on the bf16 image
    table += [("fp8", 4, "none", P(70, 1)), ("fp8", 65, "none", P(70, 1)),
              ("fp8", 65, "none", P(71, 4)), ("fp8", 8, "bias_gelu", P(70, 1)),
              ("fp8odd", 8, "none", P(71, 1))]
    for kind, M, epi, plan in table:
        @case(f"gemm_native/{kind}/M{M}/{epi}/t{plan.tile}s{plan.splits}", plan)
        def _(r, kind=kind, M=M, epi=epi, plan=plan):
            w = _w(r, kind)
            bias = r.t("bias", N0) if epi.startswith("bias") else None
            return ops._gemm_native(_x(r, M, w), w, epi, bias=bias, plan=plan)

    @case("gemm_native/fp8/stream-fallback/row-stride", P(71, 2))
    def _(r):
        w = _w(r, "fp8")
        return ops._gemm_native(r.t("x", 8, K0 + 4)[:, :K0], w, "none", plan=P(71, 2))

    @case("gemm_native/fp8/stream-fallback/grouped", P(70, 1))
    def _(r):
        w = _w(r, "fp8")
        return ops._gemm_native(_x(r, 8, w), w, "none", plan=P(70, 1), groups=1,
                                group_off=r.t("off", 2, dtype=I32), rows_per_group=8)

    @case("gemm_native/error/stream-tile-on-bf16", P(70, 1))
    def _(r):
        w = _w(r, "bf16")
        return ops._gemm_native(_x(r, 8, w), w, "none", plan=P(70, 1))

    @case("slab_gemm/error/stream-tile-on-bf16", P(71, 2))
    def _(r):
        w = _w(r, "bf16")
        return ops._slab_gemm(_x(r, 8, w), w, P(71, 2), r.t("slabs", 2 * 8 * N0, dtype=F32))

    # grouped: the dense grid (heuristic and forced plan, an epilogue, an out=) and the list
    for tag, epi, plan, tl in (("dense-heur", "none", None, False),
                               ("dense", "silu_mul", P(2, 1), False),
                               ("dense-split", "none", P(1, 2), False),
                               ("list", "silu_mul", P(1, 1), True),
                               ("list-split", "none", P(1, 2), True)):
        @case(f"gemm_native/grouped/{tag}", plan)
        def _(r, epi=epi, plan=plan, tl=tl):
            E, rows = 4, 32
            w = r.t("w", E, N0, K0)
            out = r.t("out", rows, N0 // 2 if epi == "silu_mul" else N0)
            cap = G.max_items(rows, E, 64)
            tile_list = (r.t("list", 1 + cap, 2, dtype=I32), cap) if tl else None
            return ops._gemm_native(r.t("x", rows, K0), w, epi, out=out, plan=plan, groups=E,
                                    group_off=r.t("off", E + 1, dtype=I32), rows_per_group=rows,
                                    tile_list=tile_list)


def _slab_cases():
    for kind, M, plan in (("bf16", 8, P(0, 2)), ("bf16", 8, P(0, 4)), ("bf16", 8, P(0, 3)),
                          ("bf16", 300, P(45, 2)), ("bf16", 1, P(30, 2)),
                          ("fp8", 1, P(30, 2)), ("fp8", 4, P(56, 2)), ("fp8", 5, P(30, 2)),
                          ("fp8", 8, P(0, 2)), ("fp8odd", 1, P(30, 2)),
                          ("fp8", 8, P(70, 2)), ("fp8", 64, P(71, 4)),
                          # stream plans the call cannot take: the consumer's split count stays
                          ("fp8", 65, P(70, 4)), ("fp8", 4, P(71, 2)), ("fp8odd", 8, P(70, 2))):
        @case(f"slab_gemm/{kind}/M{M}/t{plan.tile}s{plan.splits}", plan)
        def _(r, kind=kind, M=M, plan=plan):
            w = _w(r, kind)
            return ops._slab_gemm(_x(r, M, w), w, plan,
                                  r.t("slabs", plan.splits * M * N0, dtype=F32))

    @case("slab_gemm/fp8/stream-fallback/row-stride", P(70, 2))
    def _(r):
        w = _w(r, "fp8")
        return ops._slab_gemm(r.t("x", 8, K0 + 4)[:, :K0], w, P(70, 2),
                              r.t("slabs", 2 * 8 * N0, dtype=F32))


def _fused_gemv_cases():
    for kind, epi, M, plan in (("bf16", "none", 1, P(30, 1)), ("bf16", "splitk", 1, P(30, 2)),
                               ("bf16", "none", 1, P(0, 1)), ("fp8", "silu_mul", 1, P(29, 1)),
                               ("fp8", "none", 2, P(56, 2)), ("fp8", "splitk", 1, P(0, 2)),
                               ("fp8odd", "none", 1, P(30, 1)), ("bf16", "none", 5, P(30, 1))):
        @case(f"linear_normed/{kind}/{epi}/M{M}/t{plan.tile}s{plan.splits}", plan)
        def _(r, kind=kind, epi=epi, M=M, plan=plan):
            w = _w(r, kind)
            return ops.linear_normed(_normed(r, M, w), w, epi, plan)

    @case("gemv_prologue/ws-given", P(30, 2))
    def _(r):
        w = _w(r, "fp8")
        return ops._gemv_prologue(_normed(r, 1, w), w, "splitk", P(30, 2), None, N0,
                                  ws=r.t("slabs", 2 * N0, dtype=F32))

    def residual_case(name, kind="bf16", M=1, plan=None, res=None, x=None, w=None):
        @case(f"linear_residual/{name}", plan)
        def _(r):
            wt = w(r) if w else _w(r, kind)
            xt = x(r) if x else _x(r, M, wt)
            rt = res(r) if res else r.t("res", M, N0)
            return ops.linear_residual(xt, wt, rt, plan)

    residual_case("taken/bf16")
    residual_case("taken/bf16/M4/t30", M=4, plan=P(30, 1))
    residual_case("taken/fp8", kind="fp8")
    residual_case("refused/tile", plan=P(0, 1))
    residual_case("refused/M5", M=5)
    residual_case("refused/fp8odd", kind="fp8odd")
    residual_case("refused/residual-stride", res=lambda r: r.t("res", 1, 2 * N0)[:, ::2])
    residual_case("refused/x-stride", x=lambda r: r.t("x", 1, 2 * K0)[:, ::2])
    residual_case("refused/w-stride", w=lambda r: r.t("w", N0, 2 * K0)[:, ::2])


def _add_rmsnorm_cases():
    for kind, M, plan in (("bf16", 8, None), ("bf16", 8, P(0, 2)), ("bf16", 8, P(0, 1)),
                          ("bf16", 8, P(45, 2)), ("bf16", 1, None), ("fp8", 1, None),
                          ("fp8", 8, None), ("fp8", 8, P(70, 2)), ("fp8", 8, P(71, 1)),
                          ("fp8", 65, P(70, 4)), ("fp8odd", 1, None)):
        for norm in (True, False) if kind == "bf16" and M == 8 else (True,):
            tag = "heur" if plan is None else f"t{plan.tile}s{plan.splits}"

            @case(f"linear_add_rmsnorm/{kind}/M{M}/{tag}/{'norm' if norm else 'add'}", plan)
            def _(r, kind=kind, M=M, plan=plan, norm=norm):
                w = _w(r, kind)
                return ops.linear_add_rmsnorm(_x(r, M, w), w, r.t("res", M, N0),
                                              r.t("norm_w", N0) if norm else None, 1e-6, plan)

    # route: (n, experts, plan, norm_w, route tail); the fast path needs N = 4096, <= 8
    # experts, renormalised weights, a norm and split slabs; fp16 slabs for the fused gate
    for tag, n, E, plan, norm, tail in (("fmt1", 4096, 8, None, True, ()),
                                        ("fmt1-forced", 4096, 4, P(0, 4), True, (True,)),
                                        ("fmt0", 4096, 8, P(45, 2), True, ()),
                                        ("no/experts", 4096, 16, None, True, ()),
                                        ("no/width", N0, 8, None, True, ()),
                                        ("no/norm_topk", 4096, 8, P(0, 2), True, (False,)),
                                        ("no/unsplit", 4096, 8, P(0, 1), True, ())):
        @case(f"linear_add_rmsnorm/route/{tag}", plan)
        def _(r, n=n, E=E, plan=plan, norm=norm, tail=tail):
            w = r.t("w", n, K0)
            route = (r.t("router", E, n), 2) + tail
            return ops.linear_add_rmsnorm(r.t("x", 8, K0), w, r.t("res", 8, n),
                                          r.t("norm_w", n) if norm else None, 1e-6, plan,
                                          route=route)


def _qkv_inputs(r: Recorder, M: int, fp8_cache: bool = False):
    kv = R.FP8_KV if fp8_cache else BF16
    return dict(positions=r.t("positions", M, dtype=I32), slot_mapping=r.t("slots", M, dtype=I32),
                cos_sin=r.t("cos_sin", 64, HD, dtype=F32),
                k_cache=r.t("k_cache", 4, HKV, 16, HD, dtype=kv),
                v_cache=r.t("v_cache", 4, HKV, 16, HD, dtype=kv))


def _qkv_cases():
    def extras(r, bias, qk):
        return dict(bias=r.t("bias", NQKV) if bias else None,
                    qk_norm=(r.t("q_w", HD), r.t("k_w", HD), 1e-6) if qk else None)

    for tag, kind, M, plan, bias, qk, fp8c, normed in (
            ("plain", "bf16", 8, None, False, False, False, False),
            ("bias", "bf16", 8, None, True, False, False, False),
            ("qk_norm", "bf16", 8, None, False, True, False, False),
            ("fp8-cache", "bf16", 8, None, True, True, True, False),
            ("unsplit", "bf16", 8, P(0, 1), False, False, False, False),
            ("unsplit-bias", "bf16", 8, P(0, 1), True, True, False, False),
            ("split-forced", "bf16", 8, P(0, 4), True, False, False, False),
            ("normed", "bf16", 1, None, False, False, False, True),
            ("fp8w-gemv", "fp8", 1, None, False, False, False, False),
            ("fp8w-stream", "fp8", 8, P(70, 2), True, False, True, False),
            ("fp8w-fallback", "fp8", 65, P(71, 4), False, False, False, False)):
        @case(f"linear_rope_cache/{tag}", plan)
        def _(r, kind=kind, M=M, plan=plan, bias=bias, qk=qk, fp8c=fp8c, normed=normed):
            w = _w(r, kind, NQKV)
            x = _normed(r, M, w) if normed else _x(r, M, w)
            q = _qkv_inputs(r, M, fp8c)
            scales = dict(k_scale=0.5, v_scale=2.0) if fp8c else {}
            return ops.linear_rope_cache(x, w, q["positions"], q["slot_mapping"], q["cos_sin"],
                                         q["k_cache"], q["v_cache"], HQ, HKV, HD, plan=plan,
                                         **extras(r, bias, qk), **scales)

    # linear_rope_attention reads its plan from the cache ("splitk" key)
    for tag, kind, B, plan, normed, kw in (
            ("s2", "bf16", 8, P(0, 2), False, {}),
            ("s4", "bf16", 8, P(0, 4), False, dict(bias=True, qk=True, window=32)),
            ("s8-none", "bf16", 8, P(0, 8), False, {}),
            ("heuristic", "bf16", 3, None, False, {}),
            ("unsplit", "bf16", 8, P(0, 1), False, dict(bias=True)),
            ("unsplit-normed", "bf16", 1, P(30, 1), True, {}),
            ("normed-prologue", "bf16", 1, P(30, 2), True, dict(qk=True)),
            ("normed-prologue-fp8w", "fp8", 1, P(56, 4), True, {}),
            ("normed-no-prologue", "bf16", 1, P(0, 2), True, {}),
            ("normed-fp8odd", "fp8odd", 1, P(30, 2), True, {}),
            ("fp8w-stream", "fp8", 8, P(70, 2), False, {}),
            ("fp8w-fallback", "fp8", 65, P(70, 4), False, {}),
            ("none/head-dim", "bf16", 8, P(0, 2), False, dict(hd=64)),
            ("none/fp8-cache", "bf16", 8, P(0, 2), False, dict(fp8c=True)),
            ("none/kv-splits", "bf16", 1, P(0, 2), False, dict(max_context=4096))):
        @case(f"linear_rope_attention/{tag}", plan)
        def _(r, kind=kind, B=B, plan=plan, normed=normed, kw=kw):
            w = _w(r, kind, NQKV)
            if plan is not None:
                _set(w, B, "splitk", plan)
            x = _normed(r, B, w) if normed else _x(r, B, w)
            q = _qkv_inputs(r, B, kw.get("fp8c", False))
            return ops.linear_rope_attention(
                x, w, q["positions"], q["slot_mapping"], q["cos_sin"], q["k_cache"],
                q["v_cache"], r.t("block_tables", B, 4, dtype=I32),
                r.t("context_lens", B, dtype=I32), kw.get("max_context", 64), HQ, HKV,
                kw.get("hd", HD), 0.125, window=kw.get("window", 0),
                **extras(r, kw.get("bias"), kw.get("qk")))


def _moe_cases():
    D, F, T, k = K0, 128, 8, 2

    for tag, plan, tl in (("dense", P(1, 2), False), ("list", P(2, 4), True)):
        def down(r, plan=plan, tl=tl):
            E, n = 4, T * k
            cap = G.max_items(n, E, 64)
            return dict(act=r.t("act", n, F), w_down=r.t("w_down", E, D, F),
                        offsets=r.t("off", E + 1, dtype=I32), n=n, p=plan,
                        tile_list=(r.t("list", 1 + cap, 2, dtype=I32), cap) if tl else None)

        @case(f"moe_down_slabs/{tag}", plan)
        def _(r, down=down):
            return ops._moe_down_slabs(**down(r))

        @case(f"moe_down_combine/{tag}", plan)
        def _(r, down=down):
            a = down(r)
            return ops.moe_down_combine(a["act"], a["w_down"], a["offsets"], a["n"], a["p"],
                                        r.t("topk_w", T, k, dtype=F32),
                                        r.t("pos", T * k, dtype=I32), r.t("out", T, D),
                                        tile_list=a["tile_list"])

    # moe_mlp: 4 experts keep the dense grid (the row-gathering gate/up GEMM), 16 take the
    # tile list; a split down plan on an fp16-slab tile reduces inside the combine (or is left
    # pending); a gate/up tile outside the gathering family runs on a gathered copy
    for tag, E, p_gu, p_dn, defer in (("E4", 4, None, None, False),
                                      ("E16", 16, None, None, False),
                                      ("E4-slabs", 4, None, P(1, 2), False),
                                      ("E16-slabs-pending", 16, None, P(1, 2), True),
                                      ("E4-copy", 4, P(45, 1), None, False),
                                      ("E16-copy-split", 16, P(1, 2), P(45, 2), False)):
        @case(f"moe_mlp/{tag}")
        def _(r, E=E, p_gu=p_gu, p_dn=p_dn, defer=defer):
            if p_gu is not None:
                G._grouped_cache[(T * k, 2 * F, D, "silu_mul", E)] = p_gu
            if p_dn is not None:
                G._grouped_cache[(T * k, D, F, "none", E)] = p_dn
            return ops.moe_mlp(r.t("x", T, D), r.t("w_gu", E, 2 * F, D), r.t("w_down", E, D, F),
                               r.t("topk_w", T, k, dtype=F32), r.t("topk_ids", T, k, dtype=I32),
                               defer_combine=defer)


for _make in (_linear_cases, _gemm_native_cases, _slab_cases, _fused_gemv_cases,
              _add_rmsnorm_cases, _qkv_cases, _moe_cases):
    _make()


def run_case(name: str) -> dict:
    """{"plan": [tile, splits] or None, "trace": events, "workspace": byte counts}, with
    "raises": the exception's type name where the case ends in one."""
    plan, fn = CASES[name]
    out = {"plan": [plan.tile, plan.splits] if plan is not None else None}
    with Recorder().patched() as r:
        try:
            ret = fn(r)
        except (ValueError, RuntimeError) as e:
            out["raises"] = type(e).__name__
        else:
            r.events.append(["return", r.value(ret)])
        out["trace"], out["workspace"] = r.events, r.ws_bytes
    return json.loads(json.dumps(out))          # tuples as lists, as the golden file holds them


def record_all() -> dict:
    return {name: run_case(name) for name in CASES}


# ----------------------------------------------------------------------------- host cost
def host_cost(calls: int = 20000, repeats: int = 5) -> dict:
    """Seconds per ``calls`` calls of ``ops.linear`` (bf16, M = 8) and of
    ``ops.linear_add_rmsnorm`` (a split plan), native calls stubbed to nothing: what eager
    prefill and graph capture pay in Python for one linear op."""
    out = {}
    with Recorder(record=False).patched() as r:
        w = _w(r, "bf16")
        x, res, nw = _x(r, 8, w), r.t("res", 8, N0), r.t("norm_w", N0)
        assert G.plan(8, N0, K0, "splitk").splits > 1
        for name, fn in (("linear", lambda: ops.linear(x, w)),
                         ("linear_add_rmsnorm",
                          lambda: ops.linear_add_rmsnorm(x, w, res, nw, 1e-6))):
            fn()
            times = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                times.append(time.perf_counter() - t0)
            out[name] = {"runs_s": [round(t, 4) for t in times],
                         "median_s": round(statistics.median(times), 4),
                         "spread_s": round(max(times) - min(times), 4)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--record", type=Path, nargs="?", const=GOLDEN, help="write the traces")
    ap.add_argument("--time", action="store_true", help="print the host cost of a call")
    a = ap.parse_args()
    if a.record:
        traces = record_all()
        a.record.write_text("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}"
                                               for k, v in traces.items()) + "\n}\n")
        print(f"{len(traces)} cases -> {a.record}")
    if a.time:
        print(json.dumps(host_cost()))


if __name__ == "__main__":
    main()
