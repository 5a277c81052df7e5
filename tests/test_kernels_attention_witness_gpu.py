"""Every attention entry point and kernel form against the closed-form witnesses of
tests/attention_witness.py: a needle per query head (is this key read, from the right block,
by the right head?) and a count of the visible keys (is every key counted exactly once?), with
finite poison in every slot a kernel may touch but must not use. The expected values are
closed forms, so no reference runs on the device. A failure names the entry point, form, split
count, window, sequence, head and target position.

(The file name sorts this module among the kernel tests on purpose: a GPU module that sorts
before test_bench_contract.py initialises the GPU in a single-process run of the suite ahead of
test_spawn_failure_ends_the_job, whose launcher refuses a parent that has done so.)"""
import math

import pytest
import torch

import attention_witness as W
from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.ops import gemm as G
from distributed_llm_inferencing_amd.ops import reference as R

pytestmark = pytest.mark.gpu
FORMS = [(1, 0), (0, 4), (0, 1)]      # (pipelined, form): pipelined, workgroup / wave per item


class Failures:
    """Collects every failing configuration of a test, so that one run shows the pattern."""

    def __init__(self):
        self.msgs = []

    def check(self, out, sc, what):
        try:
            W.check(out, sc, what)
        except AssertionError as e:
            self.msgs.append(str(e))

    def done(self):
        assert not self.msgs, f"{len(self.msgs)} configurations fail:\n" + "\n".join(self.msgs[:40])


def _decode(sc, qkv, cache, hkv, window, splits, scales=(1.0, 1.0), max_context=None):
    k, v, tables, ctx = cache
    _, hq, hd = sc.q.shape
    return ops.decode_attention(qkv, k, v, tables, ctx, max_context or max(sc.ctxs), hq, hkv, hd,
                                1 / math.sqrt(hd), num_splits=splits, window=window,
                                k_scale=scales[0], v_scale=scales[1])


def _decode_scenes(hq, hkv, hd, bs, window, ctxs=W.DECODE_CTXS):
    return W.decode_scenes(ctxs, hq, hkv, hd, bs, window, seed=window + 1)


def _groups(gpu, needles, count, hkv, scales=None):
    """(scenes, their qkv on the device, the device cache they share)."""
    out = [(needles, [W.device_qkv(s, hkv, gpu) for s in needles],
            W.device_cache(needles[0], gpu, scales))]
    if count is not None:
        out.append(([count], [W.device_qkv(count, hkv, gpu)], W.device_cache(count, gpu, scales)))
    return out


@pytest.mark.parametrize("window", W.DECODE_WINDOWS)
@pytest.mark.parametrize("hq,hkv,hd,bs", W.DECODE_SHAPES)
def test_decode_bf16(gpu, hq, hkv, hd, bs, window):
    f = Failures()
    groups = _groups(gpu, *_decode_scenes(hq, hkv, hd, bs, window), hkv)
    for pipe, form in FORMS:
        old, old_form = ops.decode_pipelined(pipe), ops.decode_form(form)
        try:
            for splits in W.DECODE_SPLITS:
                for scenes, qkvs, cache in groups:
                    for sc, qkv in zip(scenes, qkvs):
                        f.check(_decode(sc, qkv, cache, hkv, window, splits), sc,
                                f"decode_attention bf16 pipe {pipe} form {form} splits {splits} "
                                f"window {window}")
        finally:
            ops.decode_pipelined(old)
            ops.decode_form(old_form)
    f.done()


@pytest.mark.parametrize("scales", W.FP8_SCALES)
@pytest.mark.parametrize("window", W.DECODE_WINDOWS)
@pytest.mark.parametrize("hq,hkv,hd,bs", W.DECODE_SHAPES)
def test_decode_fp8(gpu, hq, hkv, hd, bs, window, scales):
    f = Failures()
    for scenes, qkvs, cache in _groups(gpu, *_decode_scenes(hq, hkv, hd, bs, window), hkv, scales):
        for splits in W.DECODE_SPLITS:
            for sc, qkv in zip(scenes, qkvs):
                f.check(_decode(sc, qkv, cache, hkv, window, splits, scales), sc,
                        f"decode_attention fp8 scales {scales} splits {splits} window {window}")
    f.done()


def test_decode_32k(gpu):
    """Needle only (the count witness is blind at 32768 keys): 0, 32767 and both sides of every
    tile and KV-block boundary, the split boundaries of the three split counts and the
    multiples of 1024 among them, with a 77-token sequence in the same batch."""
    hq, hkv, hd, bs = 32, 8, 128, 16
    ctxs, split_counts = [32768, 77], [None, 8, 32]
    scenes = W.decode_needle(ctxs, hq, hkv, hd, bs, 0, 1 / math.sqrt(hd), seed=5)
    cache = W.device_cache(scenes[0], gpu)
    qkvs = [W.device_qkv(s, hkv, gpu) for s in scenes]
    f = Failures()
    for pipe in (1, 0):
        old = ops.decode_pipelined(pipe)
        try:
            for splits in split_counts:
                for sc, qkv in zip(scenes, qkvs):
                    f.check(_decode(sc, qkv, cache, hkv, 0, splits), sc,
                            f"decode_attention bf16 32k pipe {pipe} splits {splits}")
        finally:
            ops.decode_pipelined(old)
    f.done()


@pytest.mark.parametrize("window", [0, 48])
@pytest.mark.parametrize("form", [1, 4])
@pytest.mark.parametrize("splits", [1, 2, 4])
@pytest.mark.parametrize("hq,hkv", [(32, 8), (8, 1)])
def test_fused_decode_count(gpu, request, hq, hkv, splits, form, window):
    """``linear_rope_attention`` with x = 0: every projected row is 0, RoPE of 0 is 0 and the
    new token's K / V rows are written as 0, so with the count cache the output is n_d / n with
    position L - 1 in n but not in n_d. The slot of L - 1 holds poison beforehand; every other
    cache byte, poison included, must come back untouched."""
    old_form = ops.decode_form(form)
    request.addfinalizer(lambda: ops.decode_form(old_form))
    hd, bs, lens = 128, 16, W.FUSED_LENS
    B, K, N = len(lens), 1024, (hq + 2 * hkv) * hd
    sc = W.decode_count(lens, hq, hkv, hd, bs, window, seed=11, new_token=True)
    kc, vc, tables, ctx = W.device_cache(sc, gpu)
    last = [blocks[(L - 1) // bs] * bs + (L - 1) % bs for L, blocks in zip(lens, sc.lay.blocks)]
    slots = torch.tensor(last, device=gpu, dtype=torch.int32)
    pos = torch.tensor(lens, device=gpu, dtype=torch.int32) - 1
    cs = R.rope_cos_sin(2048, hd, 500000.0, device=gpu)
    torch.manual_seed(3)
    x = torch.zeros(B, K, device=gpu, dtype=torch.bfloat16)
    w = (torch.randn(N, K, device=gpu) * 0.05).to(torch.bfloat16)
    k0, v0 = kc.clone(), vc.clone()
    G.set_plan(B, N, K, "splitk", G.GemmPlan("dli", 0, splits))
    try:
        out = ops.linear_rope_attention(x, w, pos, slots, cs, kc, vc, tables, ctx, max(lens),
                                        hq, hkv, hd, 1 / math.sqrt(hd), window=window)
    finally:
        G.clear_plans()
    assert out is not None
    W.check(out, sc, f"linear_rope_attention form {form} qkv splits {splits} window {window}")
    for c0 in (k0, v0):                      # the rows the kernel had to write: zeros
        c0[slots.long() // bs, :, slots.long() % bs, :] = 0
    assert torch.equal(kc, k0) and torch.equal(vc, v0), "cache bytes outside the new slots changed"


def _prefill(gpu, f, lens, hq, hkv, hd, window, what):
    scale = 1 / math.sqrt(hd)
    for kind in ("needle", "count"):
        if kind == "count" and not W.count_ok(max(lens), window, hd):
            continue
        sc = W.prefill_scene(kind, lens, hq, hkv, hd, window, scale)
        out = ops.prefill_attention(W.device_qkv(sc, hkv, gpu), W.cu_seqlens(sc, gpu), max(lens),
                                    hq, hkv, hd, scale, window=window)
        f.check(out, sc, f"prefill_attention {what} lens {lens} window {window}")


@pytest.mark.parametrize("window", W.PREFILL_WINDOWS)
@pytest.mark.parametrize("hq,hkv,hd", W.PREFILL_SHAPES)
def test_prefill_short(gpu, hq, hkv, hd, window):
    """The 64-row kernel, head-packed (2 / 4 heads per workgroup at <= 32 / 16 tokens) and not."""
    f = Failures()
    for pack in (True, False):
        old = ops.prefill_set_pack(pack)
        try:
            for lens in W.PREFILL_SHORT:
                _prefill(gpu, f, lens, hq, hkv, hd, window, f"pack {pack}")
        finally:
            ops.prefill_set_pack(old)
    f.done()


@pytest.mark.parametrize("window", W.PREFILL_WINDOWS)
@pytest.mark.parametrize("hq,hkv,hd", W.PREFILL_SHAPES)
def test_prefill_long(gpu, hq, hkv, hd, window):
    """The 256-row kernel (head dim 128, min_len 1) and the 64-row kernel (min_len 1 << 30)."""
    f = Failures()
    for thr in (1, 1 << 30) if hd == 128 else (1 << 30,):
        old = ops.prefill_long_min_len(thr)
        try:
            for lens in W.PREFILL_LONG:
                _prefill(gpu, f, lens, hq, hkv, hd, window, f"min_len {thr}")
        finally:
            ops.prefill_long_min_len(old)
    f.done()


@pytest.mark.parametrize("scales", [None] + W.FP8_SCALES)
@pytest.mark.parametrize("window", W.PAGED_WINDOWS)
@pytest.mark.parametrize("hq,hkv,hd,bs", W.DECODE_SHAPES)
def test_prefill_paged(gpu, hq, hkv, hd, bs, window, scales):
    """Chunked prefill over a scattered paged cache: bf16 through both kernels (head dim 128),
    FP8 (one kernel) under both scale pairs."""
    f = Failures()
    scale = 1 / math.sqrt(hd)
    ks, vs = scales or (1.0, 1.0)
    for kind in ("needle", "count"):
        chunks = [c for c in W.PAGED_CHUNKS
                  if kind == "needle" or W.count_ok(c[0], window, hd)]
        sc = W.paged_prefill_scene(kind, chunks, hq, hkv, hd, bs, window, scale, seed=9)
        k, v, tables, ctx = W.device_cache(sc, gpu, scales)
        qkv, cu = W.device_qkv(sc, hkv, gpu), W.cu_seqlens(sc, gpu)
        for thr in (1, 1 << 30) if (hd == 128 and scales is None) else (1 << 30,):
            old = ops.prefill_long_min_len(thr)
            try:
                out = ops.prefill_attention_paged(qkv, cu, max(n for _, n in chunks), ctx, tables,
                                                  k, v, hq, hkv, hd, scale, window=window,
                                                  k_scale=ks, v_scale=vs)
            finally:
                ops.prefill_long_min_len(old)
            f.check(out, sc, f"prefill_attention_paged {'fp8 ' + str(scales) if scales else 'bf16'}"
                             f" min_len {thr} window {window}")
    f.done()


@pytest.mark.parametrize("window", [0, 40])
def test_witnesses_reject_wrong_launches(gpu, window):
    """The comparison itself has teeth on the device: the same kernels, handed a context one
    key short or long, a table with one block swapped for the pad block, or the query heads
    of each GQA group rolled by one, fail a witness (all of it in bounds: every table row
    ends in a pad entry)."""
    hq, hkv, hd, bs = 32, 8, 128, 16
    ctxs = [1, 33, 100, 1025]
    needles, count = _decode_scenes(hq, hkv, hd, bs, window, ctxs)
    needles = needles[:2]
    wrong = {"context - 1": [], "context + 1": [], "pad block": [], "heads rolled": []}
    for scenes, qkvs, (k, v, tables, ctx) in _groups(gpu, needles, count, hkv):
        pad_tables = tables.clone()
        for b, L in enumerate(ctxs):
            pad_tables[b, (L - 1) // bs] = scenes[0].lay.pad
        for sc, qkv in zip(scenes, qkvs):
            rolled = qkv.clone()
            rolled[:, :hq * hd] = qkv[:, :hq * hd].reshape(-1, hkv, hq // hkv, hd).roll(
                1, 2).reshape(-1, hq * hd)
            for name, cache, x in (("context - 1", (k, v, tables, ctx - 1), qkv),
                                   ("context + 1", (k, v, tables, ctx + 1), qkv),
                                   ("pad block", (k, v, pad_tables, ctx), qkv),
                                   ("heads rolled", (k, v, tables, ctx), rolled)):
                out = _decode(sc, x, cache, hkv, window, None, max_context=max(ctxs) + 1)
                wrong[name].append(bool(W.violations(out, sc).any()))
    for name, caught in wrong.items():
        assert any(caught), f"{name}: no witness fails on the device (window {window})"
