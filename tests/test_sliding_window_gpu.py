"""Sliding-window attention on the GPU: every decode kernel form, the fused decode kernel and
both prefill kernels against the fp32 reference ops (``ops/reference.py``, themselves checked
against a brute-force softmax in test_sliding_window.py), then the model and the engine in
bf16 against the eager HF fp32 twin. The window starts are chosen to fall inside 32-token
tiles, inside KV blocks and past the first 64-block table window."""
import math

import numpy as np
import pytest
import torch

from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.engine import SamplingParams
from distributed_llm_inferencing_amd.engine.llm_engine import LLMEngine
from distributed_llm_inferencing_amd.models import get_config
from distributed_llm_inferencing_amd.models.weights import from_hf_state_dict
from distributed_llm_inferencing_amd.ops import gemm as G
from distributed_llm_inferencing_amd.ops import reference as R

from hf_helpers import our_last_logits
from test_sliding_window import PROMPT60, hf_mistral

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FORMS = ((1, 0), (0, 4), (0, 1))     # (pipelined, wave per item / workgroup per item)


def rnd(*shape, dev, scale=1.0, dtype=BF):
    return (torch.randn(*shape, device=dev) * scale).to(dtype)


def close(a, b, rtol=2e-2, atol=2e-2):
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    tol = atol + rtol * b.abs().max().item()
    assert err <= tol, f"max err {err} > tol {tol}"


def _cache(gpu, ctxs, hkv, hd, bs, seed):
    """Random K/V in a scattered paged cache for sequences of ``ctxs`` tokens."""
    torch.manual_seed(seed)
    nblk = sum(-(-c // bs) for c in ctxs) + 4
    kc = rnd(nblk, hkv, bs, hd, dev=gpu)
    vc = rnd(nblk, hkv, bs, hd, dev=gpu)
    perm = torch.randperm(nblk - 4, device=gpu).to(torch.int32)
    maxb = -(-max(ctxs) // bs)
    tables, o = [], 0
    for c in ctxs:
        nb = -(-c // bs)
        tables.append(torch.cat([perm[o:o + nb], torch.zeros(maxb - nb, dtype=torch.int32,
                                                               device=gpu)]))
        o += nb
    return kc, vc, torch.stack(tables)


def _decode_case(gpu, lens, windows, hq, hkv, hd, bs, seed):
    kc, vc, tables = _cache(gpu, lens, hkv, hd, bs, seed)
    B = len(lens)
    qkv = rnd(B, (hq + 2 * hkv) * hd, dev=gpu)
    ctx = torch.tensor(lens, device=gpu, dtype=torch.int32)
    scale = 1 / math.sqrt(hd)
    q = qkv[:, : hq * hd].reshape(B, hq, hd)
    refs = {w: R.decode_attention(q, kc, vc, tables, ctx, scale, window=w).reshape(B, -1)
            for w in windows}

    def run(window, splits):
        return ops.decode_attention(qkv, kc, vc, tables, ctx, max(lens), hq, hkv, hd, scale,
                                    num_splits=splits, window=window)
    for pipe, wpi in FORMS:
        old, old_form = ops.decode_pipelined(pipe), ops.decode_form(wpi)
        try:
            for splits in (1, 2, 4):
                for w in windows:
                    out = run(w, splits)
                    try:
                        close(out, refs[w])
                    except AssertionError as e:
                        raise AssertionError(f"pipe {pipe} wpi {wpi} splits {splits} "
                                             f"window {w}: {e}") from None
                # a window no sequence outgrows takes the full-attention path bit for bit
                full = run(0, splits)
                assert torch.equal(run(max(lens), splits), full)
                assert torch.equal(run(max(lens) + 7, splits), full)
        finally:
            ops.decode_pipelined(old)
            ops.decode_form(old_form)


SHAPES = [(32, 8, 128, 16), (12, 12, 64, 32), (8, 1, 128, 16)]


@pytest.mark.parametrize("hq,hkv,hd,bs", SHAPES)
def test_decode_window_every_form(gpu, hq, hkv, hd, bs):
    """Windows larger than, equal to and one less than a context, and starts that straddle
    tiles (32) and blocks, in the pipelined, wave-per-item and workgroup-per-item kernels
    with 1 / 2 / 4 KV splits (some splits of the short sequences are empty)."""
    _decode_case(gpu, [1, 31, 32, 33, 49, 100, 130], [1, 5, 31, 32, 33, 48, 100], hq, hkv, hd,
                 bs, seed=31)


@pytest.mark.parametrize("hq,hkv,hd,bs", [s for s in SHAPES if s[3] == 16])
def test_decode_window_block_table_windows(gpu, hq, hkv, hd, bs):
    """Contexts of more than 64 blocks: window 40 starts past the first 64-block table
    window, window 1050 makes the span cross a table-window refresh."""
    _decode_case(gpu, [1100, 1030], [40, 1050], hq, hkv, hd, bs, seed=32)


@pytest.mark.parametrize("wpi", [1, 4])
@pytest.mark.parametrize("splits", [1, 2, 4])
def test_fused_rope_attention_window(gpu, request, splits, wpi):
    """The fused QKV-reduce + RoPE + cache-write + attention kernel with a window: the cache
    bytes of the unfused path, its output, and the fp32 chain."""
    old_form = ops.decode_form(wpi)
    request.addfinalizer(lambda: ops.decode_form(old_form))
    hq, hkv, hd, bs, W = 32, 8, 128, 16, 48
    lens = [1, 5, 33, 100, 200, 17, 130]
    B = len(lens)
    torch.manual_seed(33)
    nblk = sum(-(-n // bs) for n in lens) + 8
    kc = rnd(nblk, hkv, bs, hd, dev=gpu)
    vc = rnd(nblk, hkv, bs, hd, dev=gpu)
    perm = torch.randperm(nblk).tolist()
    maxb = max(-(-n // bs) for n in lens)
    tables, slots, o = [], [], 0
    for n in lens:
        nb = -(-n // bs)
        blocks = perm[o:o + nb]
        o += nb
        tables.append(blocks + [0] * (maxb - nb))
        slots.append(blocks[(n - 1) // bs] * bs + (n - 1) % bs)
    tables = torch.tensor(tables, device=gpu, dtype=torch.int32)
    slots = torch.tensor(slots, device=gpu, dtype=torch.int32)
    ctx = torch.tensor(lens, device=gpu, dtype=torch.int32)
    pos = ctx - 1
    cs = R.rope_cos_sin(2048, hd, 500000.0, device=gpu)
    K = 1024
    N = (hq + 2 * hkv) * hd
    x, w = rnd(B, K, dev=gpu), rnd(N, K, dev=gpu, scale=0.05)
    scale = 1 / math.sqrt(hd)
    G.set_plan(B, N, K, "splitk", G.GemmPlan("dli", 0, splits))
    try:
        kc1, vc1 = kc.clone(), vc.clone()
        qkv = ops.linear_rope_cache(x, w, pos, slots, cs, kc1, vc1, hq, hkv, hd)
        ref2 = ops.decode_attention(qkv, kc1, vc1, tables, ctx, max(lens), hq, hkv, hd, scale,
                                    window=W)
        kc2, vc2 = kc.clone(), vc.clone()
        out = ops.linear_rope_attention(x, w, pos, slots, cs, kc2, vc2, tables, ctx,
                                        max(lens), hq, hkv, hd, scale, window=W)
        kc4, vc4 = kc.clone(), vc.clone()
        full = ops.linear_rope_attention(x, w, pos, slots, cs, kc4, vc4, tables, ctx,
                                         max(lens), hq, hkv, hd, scale)
        wide = ops.linear_rope_attention(x, w, pos, slots, cs, kc4, vc4, tables, ctx,
                                         max(lens), hq, hkv, hd, scale, window=max(lens))
    finally:
        G.clear_plans()
    assert out is not None and full is not None
    torch.cuda.synchronize()
    assert torch.equal(kc2, kc1) and torch.equal(vc2, vc1)
    assert torch.equal(wide, full)
    close(out, ref2, rtol=1e-2, atol=1e-2)
    qkv_r = R.linear(x, w)
    kc3, vc3 = kc.clone(), vc.clone()
    R.rope_and_cache(qkv_r, pos, slots, cs, kc3, vc3, hq, hkv, hd)
    q = qkv_r[:, : hq * hd].reshape(B, hq, hd)
    ref = R.decode_attention(q, kc3, vc3, tables, ctx, scale, window=W).reshape(B, -1)
    close(out, ref)
    assert not torch.allclose(out.float(), full.float(), atol=2e-2)     # the window matters


# ------------------------------------------------------------------------------ prefill
def _prefill_case(gpu, lens, windows, hq, hkv, hd, thresholds, seed):
    torch.manual_seed(seed)
    T = sum(lens)
    qkv = rnd(T, (hq + 2 * hkv) * hd, dev=gpu)
    cu = torch.tensor([0] + list(np.cumsum(lens)), device=gpu, dtype=torch.int32)
    scale = 1 / math.sqrt(hd)
    q, k, v = R.split_qkv(qkv, hq, hkv, hd)
    for thr in thresholds:
        old = ops.prefill_long_min_len(thr)
        try:
            full = ops.prefill_attention(qkv, cu, max(lens), hq, hkv, hd, scale)
            assert torch.equal(ops.prefill_attention(qkv, cu, max(lens), hq, hkv, hd, scale,
                                                     window=max(lens)), full)
            for w in windows:
                out = ops.prefill_attention(qkv, cu, max(lens), hq, hkv, hd, scale, window=w)
                ref = R.prefill_attention(q, k, v, cu, scale, window=w).reshape(T, -1)
                try:
                    close(out, ref)
                except AssertionError as e:
                    raise AssertionError(f"thr {thr} window {w}: {e}") from None
        finally:
            ops.prefill_long_min_len(old)


@pytest.mark.parametrize("hq,hkv,hd", [(32, 8, 128), (12, 12, 64)])
def test_prefill_window(gpu, hq, hkv, hd):
    """Windows around the 64-key tile and the 16-row wave: the 64-row kernel, and at head dim
    128 (max length 300 >= 256) the 256-row kernel too."""
    _prefill_case(gpu, [1, 17, 64, 65, 130, 300], [1, 16, 63, 64, 65, 100], hq, hkv, hd,
                  thresholds=(1 << 30, 256) if hd == 128 else (1 << 30,), seed=34)


@pytest.mark.parametrize("lens,hq,hkv,hd", [([16, 3, 9], 32, 8, 128), ([7, 32, 20], 32, 8, 128),
                                             ([7, 32, 20], 12, 6, 64)])
def test_prefill_window_short_prompts_packed(gpu, lens, hq, hkv, hd):
    """Prompts <= 16 / 32 tokens (4 / 2 query heads packed per workgroup) with window 8."""
    torch.manual_seed(35)
    T = sum(lens)
    qkv = rnd(T, (hq + 2 * hkv) * hd, dev=gpu)
    cu = torch.tensor([0] + list(np.cumsum(lens)), device=gpu, dtype=torch.int32)
    scale = 1 / math.sqrt(hd)
    old = ops.prefill_set_pack(True)
    try:
        packed = ops.prefill_attention(qkv, cu, max(lens), hq, hkv, hd, scale, window=8)
        ops.prefill_set_pack(False)
        plain = ops.prefill_attention(qkv, cu, max(lens), hq, hkv, hd, scale, window=8)
    finally:
        ops.prefill_set_pack(old)
    assert torch.equal(packed, plain)
    q, k, v = R.split_qkv(qkv, hq, hkv, hd)
    close(packed, R.prefill_attention(q, k, v, cu, scale, window=8).reshape(T, -1))


def test_prefill_window_long_kernel(gpu):
    """The 256-row kernel: its three-stage ring starts at the first tile a row block can see
    (windows of one tile, between tiles, and longer than a row block)."""
    _prefill_case(gpu, [293, 700], [64, 100, 257], 8, 2, 128, thresholds=(1,), seed=36)


def _chunks(sizes):
    """(context, chunk length) of every chunk of a prompt prefilled in chunks of ``sizes``."""
    out, ctx = [], 0
    for n in sizes:
        ctx += n
        out.append((ctx, n))
    return out


@pytest.mark.parametrize("hq,hkv,hd,bs,chunks,thresholds", [
    (32, 8, 128, 16, _chunks([40, 40, 40]), (256,)),
    (12, 12, 64, 32, _chunks([40, 40, 40]), (256,)),
    (32, 8, 128, 16, _chunks([100, 7, 300]), (256, 1 << 30)),     # 256-row and 64-row kernel
    (12, 12, 64, 32, _chunks([100, 7, 300]), (256,)),
    (8, 2, 128, 16, [(700, 300)], (256,))])                       # 256-row kernel, context 700
def test_prefill_window_paged_chunks(gpu, hq, hkv, hd, bs, chunks, thresholds):
    """Chunked prefill over the paged cache: earlier chunks lie partly or wholly below the
    window of a later chunk's rows."""
    ctxs = [c for c, _ in chunks]
    lens = [n for _, n in chunks]
    kc, vc, tables = _cache(gpu, ctxs, hkv, hd, bs, seed=37)
    T = sum(lens)
    qkv = rnd(T, (hq + 2 * hkv) * hd, dev=gpu)
    cu = torch.tensor([0] + list(np.cumsum(lens)), device=gpu, dtype=torch.int32)
    ctx = torch.tensor(ctxs, device=gpu, dtype=torch.int32)
    scale = 1 / math.sqrt(hd)
    q = qkv[:, : hq * hd].reshape(T, hq, hd)
    for thr in thresholds:
        old = ops.prefill_long_min_len(thr)
        try:
            full = ops.prefill_attention_paged(qkv, cu, max(lens), ctx, tables, kc, vc, hq, hkv,
                                               hd, scale)
            assert torch.equal(ops.prefill_attention_paged(qkv, cu, max(lens), ctx, tables, kc,
                                                           vc, hq, hkv, hd, scale,
                                                           window=max(ctxs)), full)
            for w in (50, 64):
                out = ops.prefill_attention_paged(qkv, cu, max(lens), ctx, tables, kc, vc, hq,
                                                  hkv, hd, scale, window=w)
                ref = R.prefill_attention_paged(q, kc, vc, cu, ctx, tables, scale,
                                                window=w).reshape(T, -1)
                try:
                    close(out, ref)
                except AssertionError as e:
                    raise AssertionError(f"thr {thr} window {w}: {e}") from None
        finally:
            ops.prefill_long_min_len(old)


# ------------------------------------------------------------------------------ model, engine
@pytest.mark.parametrize("name", ["mistral-tiny128", "mistral-tiny"])
def test_gpu_windowed_logits_close_to_hf_fp32(gpu, name):
    cfg = get_config(name)
    hm = hf_mistral(cfg)
    with torch.no_grad():
        ref = hm(torch.tensor([PROMPT60])).logits[0, -1]
    params = from_hf_state_dict(cfg, hm.state_dict(), dtype=torch.bfloat16)
    params = {k: v.to(gpu) for k, v in params.items()}
    ours = our_last_logits(cfg, params, PROMPT60, device=gpu).cpu()
    err = (ours - ref).abs().max().item()
    assert err < 0.05 * ref.abs().max().item() + 0.02, err
    assert ours.argmax() == ref.argmax() or (ref.topk(2).values.diff().abs() < 0.05).item()


@pytest.mark.parametrize("name", ["mistral-tiny128", "mistral-tiny"])
def test_windowed_graph_decode_equals_eager(gpu, name, monkeypatch):
    """Generation runs past the window (40 > 24); the captured graphs carry the window as a
    launch scalar."""
    monkeypatch.setenv("DLI_GEMM_AUTOTUNE", "0")      # same GEMM plans on both sides
    prompts = [PROMPT60[:5], PROMPT60[:9], PROMPT60[3:14], PROMPT60[:2], PROMPT60[10:40]]
    sp = SamplingParams(max_length=40, temperature=0.8, top_k=50, top_p=0.95, seed=123,
                        ignore_eos=True)
    outs = []
    for graphs in (False, True):
        eng = LLMEngine(name, device="cuda", max_batch=8, max_model_len=128, num_blocks=64,
                        use_graphs=graphs, seed=3)
        outs.append([o.output_ids for o in eng.generate(prompts, sp)])
    assert outs[0] == outs[1]


# (model seed, prompt offsets into PROMPT60) chosen on the CPU in fp32: along each 20-token
# prompt's greedy continuation to length 36 the top-two logits of the HF twin are never
# closer than 0.057 (mistral-tiny128) / 0.134 (mistral-tiny), several times the near-tie
# bound below (~0.03), so the reference alone decides every token of these prompts
GREEDY_CASES = {"mistral-tiny128": (10, (15, 24, 39)), "mistral-tiny": (19, (15, 33))}


@pytest.mark.parametrize("name", ["mistral-tiny128", "mistral-tiny"])
def test_windowed_greedy_tokens_match_hf_fp32(gpu, name):
    """bf16 engine on the GPU (paged prefill, graph decode past the window) against HF fp32
    ``generate``: a prompt may differ only from a step where the reference's top-two logits
    are a near tie, and at most one prompt may differ."""
    seed, offs = GREEDY_CASES[name]
    cfg = get_config(name)
    hm = hf_mistral(cfg, seed=seed)
    params = from_hf_state_dict(cfg, hm.state_dict(), dtype=torch.bfloat16)
    eng = LLMEngine(cfg, device="cuda", params=params, max_batch=4, max_model_len=128,
                    num_blocks=32)
    prompts = [PROMPT60[o:o + 20] for o in offs]
    outs = eng.generate(prompts, SamplingParams(max_length=36, do_sample=False, ignore_eos=True))
    differ = 0
    for p, o in zip(prompts, outs):
        with torch.no_grad():
            ref = hm.generate(torch.tensor([p]), max_length=36, do_sample=False,
                              eos_token_id=None, pad_token_id=0)[0].tolist()
        assert len(o.all_ids) == len(ref) == 36
        if o.all_ids == ref:
            continue
        differ += 1
        n = next(i for i, (a, b) in enumerate(zip(o.all_ids, ref)) if a != b)
        with torch.no_grad():
            top = hm(torch.tensor([ref[:n]])).logits[0, -1].topk(2).values
        assert (top[0] - top[1]).item() < 0.01 * top[0].abs().item() + 0.01, (n, top)
    assert differ <= 1, differ
