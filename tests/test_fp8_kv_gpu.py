"""FP8 (OCP e4m3fn) paged KV cache on the GPU: the cache writers byte for byte against
``reference.quantize_kv``, the FP8 decode and chunked-prefill attention kernels against the
reference ops on the same cache bytes (only the bf16 rounding of P and O separates them), then
the model against the CPU reference and the engine's graph decode against its eager decode."""
import math

import numpy as np
import pytest
import torch

from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.engine import SamplingParams
from distributed_llm_inferencing_amd.engine.llm_engine import LLMEngine
from distributed_llm_inferencing_amd.ops import gemm as G
from distributed_llm_inferencing_amd.ops import reference as R

from test_fp8_kv import three_step_logits

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F8 = torch.float8_e4m3fn
U8 = torch.uint8


def rnd(*shape, dev, scale=1.0, dtype=BF):
    return (torch.randn(*shape, device=dev) * scale).to(dtype)


def close(a, b, rtol=2e-2, atol=2e-2):
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    tol = atol + rtol * b.abs().max().item()
    assert err <= tol, f"max err {err} > tol {tol}"


# ------------------------------------------------------------------------------ writers
LENS = [5, 17, 1]
BS = 16
WRITER_SHAPES = [(32, 8, 128), (12, 12, 64), (4, 2, 64)]


def _writer_meta(gpu):
    """Positions and scattered slots of three sequences of LENS tokens; one slot is -1."""
    pos = torch.cat([torch.arange(n) for n in LENS]).to(torch.int32)
    blocks = [[6], [3, 1], [4]]
    slots = [blocks[i][t // BS] * BS + t % BS for i, n in enumerate(LENS) for t in range(n)]
    slots[9] = -1
    return pos.to(gpu), torch.tensor(slots, dtype=torch.int32, device=gpu), 8


def _spread_v(v, big=400.0, small=0.004, tiny=0.0007):
    """Columns (or weight rows) of V scaled so that its values cover the whole finite range:
    beyond +-448 (clamped), the e4m3 subnormals (2^-9 .. 2^-6) and below half the smallest
    subnormal (+-0)."""
    v[..., 0::7] *= big
    v[..., 1::7] *= small
    v[..., 2::7] *= tiny
    return v


def _extras(mode, hq, hkv, hd, gpu):
    bias = qkn = None
    if mode in ("bias", "both"):
        bias = rnd((hq + 2 * hkv) * hd, dev=gpu, scale=0.5)
    if mode in ("norm", "both"):
        qkn = (rnd(hd, dev=gpu, scale=0.3) + 1, rnd(hd, dev=gpu, scale=0.3) + 1, 1e-6)
    return bias, qkn


def _check_cache_bytes(qkv, slots, kc, vc, nblk, hq, hkv, hd, ks, vs):
    """Every written row = quantize_kv of the K / V columns the call left in qkv (reference on
    the CPU); every other row still zero."""
    torch.cuda.synchronize()
    _, k, v = R.split_qkv(qkv.cpu(), hq, hkv, hd)
    kc_r = torch.zeros(nblk, hkv, BS, hd, dtype=F8)
    vc_r = torch.zeros(nblk, hkv, BS, hd, dtype=F8)
    R.write_kv(k, v, slots.cpu(), kc_r, vc_r, ks, vs)
    assert torch.equal(kc.cpu().view(U8), kc_r.view(U8))
    got, want = vc.cpu().view(U8), vc_r.view(U8)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()[0].tolist()
        b, h, o, d = bad
        t = int((slots.cpu() == b * BS + o).nonzero()[0])
        raise AssertionError(f"v byte {bad}: got {int(got[b, h, o, d]):#x} want "
                             f"{int(want[b, h, o, d]):#x} for x = {float(v[t, h, d])!r}")
    # the range really is covered
    codes = want[want != 0] & 0x7F
    assert (codes == 0x7E).any() and (codes < 8).any() and (want == 0x80).any()


@pytest.mark.parametrize("scales", [(1.0, 1.0), (0.5, 0.5)])
@pytest.mark.parametrize("mode", ["plain", "bias", "norm"])
@pytest.mark.parametrize("hq,hkv,hd", WRITER_SHAPES)
def test_rope_and_cache_writes_exact_fp8(gpu, hq, hkv, hd, mode, scales):
    torch.manual_seed(50)
    pos, slots, nblk = _writer_meta(gpu)
    T = sum(LENS)
    qkv = rnd(T, (hq + 2 * hkv) * hd, dev=gpu)
    _spread_v(qkv[:, (hq + hkv) * hd:])
    cs = R.rope_cos_sin(64, hd, 10000.0, device=gpu)
    kc = torch.zeros(nblk, hkv, BS, hd, dtype=F8, device=gpu)
    vc = torch.zeros_like(kc)
    bias, qkn = _extras(mode, hq, hkv, hd, gpu)
    if bias is not None:
        bias[(hq + hkv) * hd:] = 0                    # keep V's spread of magnitudes
    ops.rope_and_cache(qkv, pos, slots, cs, kc, vc, hq, hkv, hd, bias=bias, qk_norm=qkn,
                       k_scale=scales[0], v_scale=scales[1])
    _check_cache_bytes(qkv, slots, kc, vc, nblk, hq, hkv, hd, *scales)


@pytest.mark.parametrize("scales", [(1.0, 1.0), (0.5, 0.5)])
@pytest.mark.parametrize("mode", ["plain", "both"])
@pytest.mark.parametrize("splits,f16", [(2, False), (2, True), (4, False), (4, True)])
@pytest.mark.parametrize("hq,hkv,hd", WRITER_SHAPES)
def test_linear_rope_cache_splitk_writes_exact_fp8(gpu, monkeypatch, hq, hkv, hd, splits, f16,
                                                   mode, scales):
    """The slab consumers (fp32 and fp16 slabs, 2 and 4 of them), plain and with bias + norm."""
    torch.manual_seed(51)
    assert 0 in G.SLAB16_TILES
    monkeypatch.setattr(G, "SLAB16", f16)
    pos, slots, nblk = _writer_meta(gpu)
    T, K = sum(LENS), 1024
    n = (hq + 2 * hkv) * hd
    x, w = rnd(T, K, dev=gpu), rnd(n, K, dev=gpu, scale=0.03)
    _spread_v(w[(hq + hkv) * hd:].t())                # whole weight rows = columns of V
    cs = R.rope_cos_sin(64, hd, 10000.0, device=gpu)
    kc = torch.zeros(nblk, hkv, BS, hd, dtype=F8, device=gpu)
    vc = torch.zeros_like(kc)
    bias, qkn = _extras(mode, hq, hkv, hd, gpu)
    if bias is not None:
        bias[(hq + hkv) * hd:] = 0
    qkv = ops.linear_rope_cache(x, w, pos, slots, cs, kc, vc, hq, hkv, hd,
                                plan=G.GemmPlan("dli", 0, splits), bias=bias, qk_norm=qkn,
                                k_scale=scales[0], v_scale=scales[1])
    _check_cache_bytes(qkv, slots, kc, vc, nblk, hq, hkv, hd, *scales)


# ------------------------------------------------------------------------------ attention
def _fill(gpu, ctxs, hkv, hd, bs, ks, vs, seed):
    """An FP8 cache filled through the FP8 writer with random K / V for sequences of ``ctxs``
    tokens in scattered blocks; returns (k_cache, v_cache, tables) on the GPU."""
    torch.manual_seed(seed)
    nblk = sum(-(-c // bs) for c in ctxs) + 4
    perm = torch.randperm(nblk - 4).tolist()
    maxb = -(-max(ctxs) // bs)
    tables, slots, o = [], [], 0
    for c in ctxs:
        nb = -(-c // bs)
        blocks = perm[o:o + nb]
        o += nb
        tables.append(blocks + [0] * (maxb - nb))
        slots += [blocks[t // bs] * bs + t % bs for t in range(c)]
    T = sum(ctxs)
    kv = rnd(T, 2 * hkv * hd, dev=gpu)
    kv[:, hkv * hd:] *= 2.0
    kc = torch.zeros(nblk, hkv, bs, hd, dtype=F8, device=gpu)
    vc = torch.zeros_like(kc)
    ops.rope_and_cache(kv, torch.zeros(T, dtype=torch.int32, device=gpu),
                       torch.tensor(slots, dtype=torch.int32, device=gpu), None, kc, vc, 0, hkv,
                       hd, use_rope=False, k_scale=ks, v_scale=vs)
    torch.cuda.synchronize()
    return kc, vc, torch.tensor(tables, dtype=torch.int32, device=gpu)


SCALES = [(1.0, 1.0), (0.5, 2.0)]


@pytest.mark.parametrize("lens", [[1, 2, 3], [100, 31, 64, 17], [700, 1025]])
@pytest.mark.parametrize("hq,hkv,hd,bs", [(32, 8, 128, 16), (12, 12, 64, 32), (8, 1, 128, 16)])
def test_decode_attention_fp8(gpu, hq, hkv, hd, bs, lens):
    """1 / 2 / 4 KV splits, full attention and window 50, scales (1, 1) and (0.5, 2); 1025
    tokens at 16 per block cross the 64-block table window."""
    B = len(lens)
    scale = 1 / math.sqrt(hd)
    for ks, vs in SCALES:
        kc, vc, tables = _fill(gpu, lens, hkv, hd, bs, ks, vs, seed=60)
        qkv = rnd(B, (hq + 2 * hkv) * hd, dev=gpu)
        ctx = torch.tensor(lens, device=gpu, dtype=torch.int32)
        q = qkv[:, : hq * hd].reshape(B, hq, hd).cpu()
        for window in (0, 50):
            ref = R.decode_attention(q, kc.cpu(), vc.cpu(), tables.cpu(), ctx.cpu(), scale,
                                     window, ks, vs).reshape(B, -1)
            for splits in (1, 2, 4):
                out = ops.decode_attention(qkv, kc, vc, tables, ctx, max(lens), hq, hkv, hd,
                                           scale, num_splits=splits, window=window, k_scale=ks,
                                           v_scale=vs)
                try:
                    close(out.cpu(), ref)
                except AssertionError as e:
                    raise AssertionError(f"scales {ks, vs} window {window} splits {splits}: "
                                         f"{e}") from None


@pytest.mark.parametrize("hq,hkv,hd,bs,chunks,scales", [
    (32, 8, 128, 16, [(100, 37), (2053, 512), (16, 16), (1, 1)], (1.0, 1.0)),
    (12, 12, 64, 32, [(70, 70), (300, 64), (129, 1)], (0.5, 2.0)),
    (32, 8, 128, 16, [(100, 17), (33, 32), (5, 5)], (0.5, 2.0))])     # short chunks: packed heads
def test_prefill_attention_paged_fp8(gpu, hq, hkv, hd, bs, chunks, scales):
    """(context, chunk length) pairs over scattered block tables, full attention and window 50.
    Every chunk length takes the 64-row kernel, whatever the long-kernel threshold says."""
    ks, vs = scales
    ctxs = [c for c, _ in chunks]
    lens = [n for _, n in chunks]
    kc, vc, tables = _fill(gpu, ctxs, hkv, hd, bs, ks, vs, seed=61)
    T = sum(lens)
    qkv = rnd(T, (hq + 2 * hkv) * hd, dev=gpu)
    cu = torch.tensor([0] + list(np.cumsum(lens)), device=gpu, dtype=torch.int32)
    ctx = torch.tensor(ctxs, device=gpu, dtype=torch.int32)
    scale = 1 / math.sqrt(hd)
    q = qkv[:, : hq * hd].reshape(T, hq, hd).cpu()
    for window in (0, 50):
        ref = R.prefill_attention_paged(q, kc.cpu(), vc.cpu(), cu.cpu(), ctx.cpu(), tables.cpu(),
                                        scale, window, ks, vs).reshape(T, -1)
        outs = []
        for thr in (256, 1 << 30):
            old = ops.prefill_long_min_len(thr)
            try:
                outs.append(ops.prefill_attention_paged(qkv, cu, max(lens), ctx, tables, kc, vc,
                                                        hq, hkv, hd, scale, window=window,
                                                        k_scale=ks, v_scale=vs))
            finally:
                ops.prefill_long_min_len(old)
        assert torch.equal(outs[0], outs[1])
        try:
            close(outs[0].cpu(), ref)
        except AssertionError as e:
            raise AssertionError(f"window {window}: {e}") from None


def test_gpu_ops_validate_the_cache_before_any_kernel(gpu):
    hq, hkv, hd, bs = 8, 2, 128, 16
    qkv = rnd(2, (hq + 2 * hkv) * hd, dev=gpu)
    tables = torch.zeros(2, 1, dtype=torch.int32, device=gpu)
    ctx = torch.ones(2, dtype=torch.int32, device=gpu)
    for dt in (U8, torch.float16, torch.float32, torch.float8_e5m2):
        kc = torch.zeros(2, hkv, bs, hd, device=gpu).to(dt)
        with pytest.raises(ValueError):
            ops.decode_attention(qkv, kc, kc, tables, ctx, 1, hq, hkv, hd, 0.1)
    k8 = torch.zeros(2, hkv, bs, hd, dtype=F8, device=gpu)
    kb = torch.zeros(2, hkv, bs, hd, dtype=BF, device=gpu)
    with pytest.raises(ValueError):
        ops.decode_attention(qkv, k8, kb, tables, ctx, 1, hq, hkv, hd, 0.1)
    with pytest.raises(ValueError):
        ops.decode_attention(qkv, kb, kb, tables, ctx, 1, hq, hkv, hd, 0.1, k_scale=2.0)
    # no fused QKV + attention kernel for an FP8 cache: the caller takes the two-kernel path
    pos = torch.zeros(2, dtype=torch.int32, device=gpu)
    cs = R.rope_cos_sin(16, hd, 10000.0, device=gpu)
    w = rnd((hq + 2 * hkv) * hd, 256, dev=gpu, scale=0.05)
    x = rnd(2, 256, dev=gpu)
    assert ops.linear_rope_attention(x, w, pos, pos, cs, k8, k8.clone(), tables, ctx, 1, hq, hkv,
                                     hd, 0.1) is None
    assert ops.linear_rope_attention(x, w, pos, pos, cs, kb, kb.clone(), tables, ctx, 1, hq, hkv,
                                     hd, 0.1) is not None


# ------------------------------------------------------------------------------ model, engine
_cpu_logits = {}


@pytest.mark.parametrize("name", ["llama-tiny", "qwen3-tiny"])
def test_gpu_fp8_logits_close_to_cpu_reference(gpu, name):
    """prefill -> paged chunk -> decode, both sides with FP8 caches. A last-bit difference in
    a rotated bf16 K can move an FP8 code by one step, so the bound is the model-level one of
    test_gpu_windowed_logits_close_to_hf_fp32, not the kernels'."""
    if name not in _cpu_logits:
        _cpu_logits[name] = three_step_logits(name, "cpu", "fp8", 0.5, 2.0)
    got = three_step_logits(name, gpu, "fp8", 0.5, 2.0)
    for step, (a, ref) in enumerate(zip(got, _cpu_logits[name])):
        err = (a - ref).abs().max().item()
        print(f"{name} step {step}: max |gpu - cpu| {err:.5f}, max |ref| "
              f"{ref.abs().max().item():.3f}")
        assert err < 0.05 * ref.abs().max().item() + 0.02, (step, err)


@pytest.mark.parametrize("name", ["llama-tiny", "mistral-tiny128"])
def test_fp8_graph_decode_equals_eager(gpu, name, monkeypatch):
    """The captured graphs carry the cache scales as launch scalars, like the window."""
    monkeypatch.setenv("DLI_GEMM_AUTOTUNE", "0")      # same GEMM plans on both sides
    base = [(5 * i * i + 3 * i + 7) % 250 + 2 for i in range(60)]
    prompts = [base[:5], base[:9], base[3:14], base[:2], base[10:40]]
    sp = SamplingParams(max_length=40, temperature=0.8, top_k=50, top_p=0.95, seed=123,
                        ignore_eos=True)
    outs = []
    for graphs in (False, True):
        eng = LLMEngine(name, device="cuda", max_batch=8, max_model_len=128, num_blocks=64,
                        use_graphs=graphs, seed=3, kv_dtype="fp8", k_scale=0.5, v_scale=2.0)
        assert eng.kv.k.dtype == F8
        outs.append([o.output_ids for o in eng.generate(prompts, sp)])
        assert int(eng.kv.k.view(U8).max()) > 0
    assert outs[0] == outs[1]


# ------------------------------------------------------------------------------ the kv_fp8 flag
def entry_args(dev, kv_dtype):
    """Valid arguments of the four entry points that take (kv_fp8, scale, scale), by name,
    without that tail and the stream: one sequence of 5 tokens, 8 / 2 heads of 128, 2 slabs."""
    hq, hkv, hd, bs, T = 8, 2, 128, 16, 5
    n = (hq + 2 * hkv) * hd
    qkv, ws = rnd(T, n, dev=dev), torch.zeros(2, T, n, device=dev)
    out = torch.empty(T, hq * hd, dtype=BF, device=dev)
    kc, vc = (torch.zeros(2, hkv, bs, hd, dtype=BF, device=dev).to(kv_dtype) for _ in range(2))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)   # noqa: E731
    pos, slots, cs = i32(list(range(T))), i32(list(range(T))), R.rope_cos_sin(16, hd, 1e4, dev)
    tables, ctx, cu = i32([[1, 0]]), i32([T]), i32([0, T])
    p = ops._p
    keep = (qkv, ws, out, kc, vc, pos, slots, cs, tables, ctx, cu)
    return keep, {
        "dli_rope_cache": (p(qkv), n, p(pos), p(slots), p(cs), p(kc), p(vc), T, hq, hkv, hd, bs,
                           1, None, None, None, 0.0),
        "dli_splitk_rope_cache": (p(qkv), p(ws), 2, T, n, p(pos), p(slots), p(cs), p(kc), p(vc),
                                  hq, hkv, hd, bs, 1, 0, None, None, None, 0.0),
        "dli_decode_attention": (p(out), p(qkv), n, p(kc), p(vc), p(tables), 2, p(ctx), 1, hq,
                                 hkv, hd, bs, hd ** -0.5, T, 1, None, 0),
        "dli_prefill_attention_paged": (p(out), hq * hd, p(qkv), n, p(cu), p(ctx), p(kc), p(vc),
                                        p(tables), 2, 1, T, hq, hkv, hd, bs, hd ** -0.5, 0),
    }


def test_bf16_cache_with_a_scale_is_refused(gpu):
    """kv_fp8 = 0 with k_scale = 2: every entry point that takes the flag returns
    hipErrorInvalidValue before any launch (``kv_cache_is_fp8`` keeps the ops from asking)."""
    keep, calls = entry_args(gpu, BF)
    for name, args in calls.items():
        with pytest.raises(RuntimeError, match=f"{name} failed with hipError 1$"):
            ops._native_call(name, *args, 0, 2.0, 1.0, ops._st())
    torch.cuda.synchronize()


@pytest.mark.parametrize("kv_dtype", [BF, F8])
def test_slab_writer_refuses_zero_splits(gpu, kv_dtype):
    """splits = 0 is refused for either cache dtype, rows and caches untouched."""
    keep, calls = entry_args(gpu, kv_dtype)
    qkv, kc = keep[0], keep[3]
    qkv0 = qkv.clone()
    args = list(calls["dli_splitk_rope_cache"])
    args[2] = 0
    with pytest.raises(RuntimeError, match="dli_splitk_rope_cache failed with hipError 1$"):
        ops._native_call("dli_splitk_rope_cache", *args, int(kv_dtype == F8), 1.0, 1.0, ops._st())
    torch.cuda.synchronize()
    assert torch.equal(qkv, qkv0) and int(kc.view(U8).max()) == 0
