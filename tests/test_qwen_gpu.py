"""Qwen3 QK-norm and Qwen2 QKV bias on the GPU: the three RoPE kernels (``rope_and_cache``,
the split-K slab consumer of ``linear_rope_cache`` and the fused decode kernel of
``linear_rope_attention``) against the fp32 reference chain (``ops/reference.py``, itself
checked against a brute-force fp64 computation in test_qwen.py), then the bf16 model and the
engine against the eager HF fp32 twins."""
import math

import pytest
import torch

from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.engine import SamplingParams
from distributed_llm_inferencing_amd.engine.llm_engine import LLMEngine
from distributed_llm_inferencing_amd.models import get_config
from distributed_llm_inferencing_amd.models.weights import from_hf_state_dict
from distributed_llm_inferencing_amd.ops import _native as N
from distributed_llm_inferencing_amd.ops import gemm as G
from distributed_llm_inferencing_amd.ops import reference as R

from hf_helpers import our_last_logits
from test_qwen import PROMPT60, hf_qwen
from test_sliding_window_gpu import close, rnd

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
MODES = ["norm", "bias", "both"]
EPS = 1e-6


def extras(mode, hq, hkv, hd, dev):
    """(bias, qk_norm) of a mode, bf16 on ``dev``: norm weights around 1, a bias of the size
    of the activations."""
    bias = rnd((hq + 2 * hkv) * hd, dev=dev, scale=0.5) if mode != "norm" else None
    qkn = None
    if mode != "bias":
        qkn = ((1 + 0.3 * torch.randn(hd, device=dev)).to(BF),
               (1 + 0.3 * torch.randn(hd, device=dev)).to(BF), EPS)
    return bias, qkn


def f32(qkn):
    return None if qkn is None else (qkn[0].float(), qkn[1].float(), qkn[2])


def ulps(a, b):
    """Largest distance between two bf16 tensors in units of the last place."""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs().max().item()


# ------------------------------------------------------------------------------ rope_and_cache
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hq,hkv,hd", [(32, 8, 128), (4, 2, 64), (7, 1, 128)])
def test_rope_and_cache_extras(gpu, hq, hkv, hd, mode):
    """7 rows of a strided QKV buffer, one of them without a cache slot; head counts that
    fill whole waves, a fraction of one, and (9 heads of 8 lanes) straddle them."""
    check_rope_and_cache_extras(gpu, hq, hkv, hd, mode, use_rope=True)


def check_rope_and_cache_extras(gpu, hq, hkv, hd, mode, use_rope):
    torch.manual_seed(41)
    T, bs, nblk = 7, 16, 3
    n = (hq + 2 * hkv) * hd
    buf = rnd(T, n + 64, dev=gpu)
    qkv = buf[:, :n]
    assert qkv.stride(0) == n + 64
    pos = torch.tensor([0, 3, 17, 4, 9, 100, 31], device=gpu, dtype=torch.int32)
    slots = torch.tensor([5, 0, -1, 11, 6, 33, 47], device=gpu, dtype=torch.int32)
    cs = R.rope_cos_sin(128, hd, 1e6, device=gpu)
    kc, vc = rnd(nblk, hkv, bs, hd, dev=gpu), rnd(nblk, hkv, bs, hd, dev=gpu)
    bias, qkn = extras(mode, hq, hkv, hd, gpu)
    ref, kc_r, vc_r = qkv.float().clone(), kc.float(), vc.float()
    R.rope_and_cache(ref, pos, slots, cs, kc_r, vc_r, hq, hkv, hd, use_rope,
                     bias=None if bias is None else bias.float(), qk_norm=f32(qkn))
    pad = buf[:, n:].clone()
    q, k, v = ops.rope_and_cache(qkv, pos, slots, cs, kc, vc, hq, hkv, hd, use_rope, bias=bias,
                                 qk_norm=qkn)
    torch.cuda.synchronize()
    close(qkv, ref)
    close(kc, kc_r)
    close(vc, vc_r)
    assert torch.equal(buf[:, n:], pad)                       # nothing past the rows
    assert q.shape == (T, hq, hd) and q.data_ptr() == qkv.data_ptr()
    unwritten = torch.ones(nblk * bs, dtype=torch.bool, device=gpu)
    unwritten[slots[slots >= 0].long()] = False
    m = unwritten.view(nblk, 1, bs, 1).expand_as(kc)
    assert torch.equal(kc[m].float(), kc_r[m]) and torch.equal(vc[m].float(), vc_r[m])


def test_rope_and_cache_extras_without_rope(gpu):
    """``use_rope=False`` with a bias and QK-norm weights: the rows are biased and normalised
    in place and k, v go to the cache unrotated."""
    check_rope_and_cache_extras(gpu, 4, 2, 64, "both", use_rope=False)


# ------------------------------------------------------------------------------ linear_rope_cache
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("splits,f16", [(1, False), (2, False), (2, True), (3, False),
                                        (4, False), (4, True), (8, False), (8, True)])
def test_linear_rope_cache_extras(gpu, monkeypatch, splits, f16, mode):
    """The slab consumer under forced plans: 2 / 4 / 8 slabs in fp32 and in fp16, 3 fp32 slabs
    (the runtime-split loop, on a K that splits into 3 multiples of 64), and the unsplit plan
    (bias in the GEMM epilogue, norm in ``rope_and_cache``)."""
    torch.manual_seed(42)
    hq, hkv, hd, bs, nblk = 32, 8, 128, 16, 4
    M, K = 7, 1536 if splits == 3 else 1024
    n = (hq + 2 * hkv) * hd
    assert 0 in G.SLAB16_TILES
    monkeypatch.setattr(G, "SLAB16", f16)
    x, w = rnd(M, K, dev=gpu), rnd(n, K, dev=gpu, scale=0.05)
    pos = torch.tensor([0, 3, 17, 4, 9, 100, 31], device=gpu, dtype=torch.int32)
    slots = torch.tensor([5, 0, -1, 11, 6, 33, 63], device=gpu, dtype=torch.int32)
    cs = R.rope_cos_sin(128, hd, 1e6, device=gpu)
    kc, vc = rnd(nblk, hkv, bs, hd, dev=gpu), rnd(nblk, hkv, bs, hd, dev=gpu)
    bias, qkn = extras(mode, hq, hkv, hd, gpu)
    ref = R.linear(x.float(), w.float(), None if bias is None else bias.float())
    kc_r, vc_r = kc.float(), vc.float()
    R.rope_and_cache(ref, pos, slots, cs, kc_r, vc_r, hq, hkv, hd, qk_norm=f32(qkn))
    qkv = ops.linear_rope_cache(x, w, pos, slots, cs, kc, vc, hq, hkv, hd,
                                plan=G.GemmPlan("dli", 0, splits), bias=bias, qk_norm=qkn)
    torch.cuda.synchronize()
    close(qkv, ref)
    close(kc, kc_r)
    close(vc, vc_r)


# ------------------------------------------------------------------------------ fused decode kernel
HQ, HKV, HD, BS, WIN = 32, 8, 128, 16, 48
LENS = [1, 5, 33, 100, 200, 17, 130]
K_IN = 1024


@pytest.fixture(scope="module")
def fused_case(gpu):
    """Inputs shared by the fused-kernel cases, and the fp32 chain per (mode, window),
    computed once."""
    torch.manual_seed(43)
    B = len(LENS)
    nblk = sum(-(-n // BS) for n in LENS) + 8
    kc, vc = rnd(nblk, HKV, BS, HD, dev=gpu), rnd(nblk, HKV, BS, HD, dev=gpu)
    perm = torch.randperm(nblk).tolist()
    maxb = max(-(-n // BS) for n in LENS)
    tables, slots, o = [], [], 0
    for n in LENS:
        nb = -(-n // BS)
        blocks = perm[o:o + nb]
        o += nb
        tables.append(blocks + [0] * (maxb - nb))
        slots.append(blocks[(n - 1) // BS] * BS + (n - 1) % BS)
    c = dict(kc=kc, vc=vc, nblk=nblk, B=B,
             tables=torch.tensor(tables, device=gpu, dtype=torch.int32),
             slots=torch.tensor(slots, device=gpu, dtype=torch.int32),
             ctx=torch.tensor(LENS, device=gpu, dtype=torch.int32),
             cs=R.rope_cos_sin(2048, HD, 1e6, device=gpu),
             x=rnd(B, K_IN, dev=gpu), w=rnd((HQ + 2 * HKV) * HD, K_IN, dev=gpu, scale=0.05),
             scale=1 / math.sqrt(HD), ext={m: extras(m, HQ, HKV, HD, gpu) for m in MODES},
             refs={})
    c["pos"] = c["ctx"] - 1
    written = torch.zeros(nblk * BS, dtype=torch.bool, device=gpu)
    written[c["slots"].long()] = True
    c["written"] = written.view(nblk, 1, BS, 1).expand_as(kc)

    def ref(mode, window):
        if (mode, window) not in c["refs"]:
            bias, qkn = c["ext"][mode]
            qkv = R.linear(c["x"].float(), c["w"].float(),
                           None if bias is None else bias.float())
            kc_r, vc_r = kc.float(), vc.float()
            R.rope_and_cache(qkv, c["pos"], c["slots"], c["cs"], kc_r, vc_r, HQ, HKV, HD,
                             qk_norm=f32(qkn))
            q = qkv[:, : HQ * HD].reshape(B, HQ, HD)
            c["refs"][mode, window] = R.decode_attention(
                q, kc_r, vc_r, c["tables"], c["ctx"], c["scale"], window=window).reshape(B, -1)
        return c["refs"][mode, window]
    c["ref"] = ref
    return c


@pytest.mark.parametrize("window", [0, WIN])
@pytest.mark.parametrize("splits", [0, 2, 4])
@pytest.mark.parametrize("wpi", [1, 4])
def test_fused_rope_attention_extras(gpu, request, monkeypatch, fused_case, wpi, splits, window):
    """The fused slab-reduce + bias + QK-norm + RoPE + cache-write + attention kernel, a wave
    and a workgroup per item, from the bf16 rows and from 2 / 4 slabs in both slab formats:
    its output against the fp32 chain, the cache rows it wrote against the unfused kernels
    (one bf16 ulp: the two sum a head's squares in a different lane order) and every other
    cache row against its bytes before the call."""
    c = fused_case
    old_form = ops.decode_form(wpi)
    request.addfinalizer(lambda: ops.decode_form(old_form))
    B, N_ = c["B"], (HQ + 2 * HKV) * HD
    args = (c["x"], c["w"], c["pos"], c["slots"], c["cs"])
    for f16 in ((False, True) if splits else (False,)):
        monkeypatch.setattr(G, "SLAB16", f16)
        G.set_plan(B, N_, K_IN, "splitk", G.GemmPlan("dli", 0, max(splits, 1)))
        try:
            for mode in MODES:
                bias, qkn = c["ext"][mode]
                kc1, vc1 = c["kc"].clone(), c["vc"].clone()
                ops.linear_rope_cache(*args, kc1, vc1, HQ, HKV, HD, bias=bias, qk_norm=qkn)
                kc2, vc2 = c["kc"].clone(), c["vc"].clone()
                out = ops.linear_rope_attention(*args, kc2, vc2, c["tables"], c["ctx"],
                                                max(LENS), HQ, HKV, HD, c["scale"],
                                                window=window, bias=bias, qk_norm=qkn)
                assert out is not None, (mode, f16)
                torch.cuda.synchronize()
                tag = f"mode {mode} fp16 slabs {f16}"
                try:
                    close(out, c["ref"](mode, window))
                except AssertionError as e:
                    raise AssertionError(f"{tag}: {e}") from None
                w_ = c["written"]
                assert ulps(kc2[w_], kc1[w_]) <= 1, tag
                assert ulps(vc2[w_], vc1[w_]) <= 1, tag
                assert torch.equal(kc2[~w_], c["kc"][~w_]), tag
                assert torch.equal(vc2[~w_], c["vc"][~w_]), tag
                assert not torch.equal(kc2[w_], c["kc"][w_])            # the rows were written
        finally:
            G.clear_plans()


# ------------------------------------------------------------------------------ null extras
def test_null_extras_change_nothing(gpu, fused_case):
    """bias=None, qk_norm=None: the three ops give the bits of the calls that do not pass
    them, and the entry point called directly with null pointers gives them too."""
    c = fused_case
    B, N_ = c["B"], (HQ + 2 * HKV) * HD
    torch.manual_seed(44)
    qkv0 = rnd(B, N_, dev=gpu)
    res = []
    for kw in ({}, dict(bias=None, qk_norm=None)):
        qkv, kc, vc = qkv0.clone(), c["kc"].clone(), c["vc"].clone()
        ops.rope_and_cache(qkv, c["pos"], c["slots"], c["cs"], kc, vc, HQ, HKV, HD, **kw)
        res.append((qkv, kc, vc))
    qkv, kc, vc = qkv0.clone(), c["kc"].clone(), c["vc"].clone()
    N.call("dli_rope_cache", qkv.data_ptr(), qkv.stride(0), c["pos"].data_ptr(),
           c["slots"].data_ptr(), c["cs"].data_ptr(), kc.data_ptr(), vc.data_ptr(), B, HQ, HKV,
           HD, BS, 1, None, None, None, 0.0, 0, 1.0, 1.0, N.stream_ptr())
    res.append((qkv, kc, vc))
    torch.cuda.synchronize()
    for other in res[1:]:
        assert all(torch.equal(a, b) for a, b in zip(res[0], other))
    args = (c["x"], c["w"], c["pos"], c["slots"], c["cs"])
    for splits in (1, 2):
        G.set_plan(B, N_, K_IN, "splitk", G.GemmPlan("dli", 0, splits))
        try:
            res = []
            for kw in ({}, dict(bias=None, qk_norm=None)):
                kc, vc = c["kc"].clone(), c["vc"].clone()
                qkv = ops.linear_rope_cache(*args, kc, vc, HQ, HKV, HD, **kw)
                kc2, vc2 = c["kc"].clone(), c["vc"].clone()
                out = ops.linear_rope_attention(*args, kc2, vc2, c["tables"], c["ctx"],
                                                max(LENS), HQ, HKV, HD, c["scale"], **kw)
                assert out is not None
                res.append((qkv, kc, vc, out, kc2, vc2))
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(*res))
        finally:
            G.clear_plans()


# ------------------------------------------------------------------------------ model, engine
@pytest.mark.parametrize("name", ["qwen3-tiny128", "qwen2-tiny128"])
def test_gpu_logits_close_to_hf_fp32(gpu, name):
    cfg = get_config(name)
    hm = hf_qwen(cfg)
    with torch.no_grad():
        ref = hm(torch.tensor([PROMPT60])).logits[0, -1]
    params = from_hf_state_dict(cfg, hm.state_dict(), dtype=torch.bfloat16)
    params = {k: v.to(gpu) for k, v in params.items()}
    ours = our_last_logits(cfg, params, PROMPT60, device=gpu).cpu()
    err = (ours - ref).abs().max().item()
    assert err < 0.05 * ref.abs().max().item() + 0.02, err
    assert ours.argmax() == ref.argmax() or (ref.topk(2).values.diff().abs() < 0.05).item()


# (model seed, prompt offsets into PROMPT60) chosen on the CPU in fp32: along each 16-token
# prompt's greedy continuation of 24 tokens the top-two logits of the HF twin are never closer
# than 0.197 (qwen3-tiny128) / 0.42 (qwen2-tiny128), several times the near-tie bound below
# (~0.03), so the reference alone decides every token of these prompts
GREEDY_CASES = {"qwen3-tiny128": (19, (27, 24, 0, 36)), "qwen2-tiny128": (5, (3, 0, 36, 33))}


@pytest.mark.parametrize("name", ["qwen3-tiny128", "qwen2-tiny128"])
def test_engine_greedy_tokens_match_hf_fp32(gpu, name):
    """4 prompts x 24 new tokens through the bf16 engine on the GPU against HF fp32
    ``generate``. Two requests decode (graph replays) before the other two arrive, so their
    prefill runs as a mixed prefill + decode step (the two-kernel path on the decode rows)
    and the rest as captured decode graphs (the fused kernel). A prompt may differ only from
    a step where the reference's top-two logits are a near tie, and at most one may differ."""
    seed, offs = GREEDY_CASES[name]
    cfg = get_config(name)
    hm = hf_qwen(cfg, seed=seed)
    params = from_hf_state_dict(cfg, hm.state_dict(), dtype=torch.bfloat16)
    eng = LLMEngine(cfg, device="cuda", params=params, max_batch=4, max_model_len=128,
                    num_blocks=32)
    assert eng.runner.use_graphs and eng.mixed_steps
    prompts = [PROMPT60[o:o + 16] for o in offs]
    sp = SamplingParams(max_new_tokens=24, do_sample=False, ignore_eos=True)
    rids = [eng.add_request(p, sp) for p in prompts[:2]]
    done = {}
    for _ in range(4):
        done.update({o.request_id: o for o in eng.step()})
    rids += [eng.add_request(p, sp) for p in prompts[2:]]
    while eng.has_work():
        done.update({o.request_id: o for o in eng.step()})
    assert eng.stats.mixed_steps >= 1 and eng.stats.decode_steps >= 20, eng.stats
    assert eng.runner.graphs, "no decode graph was captured"
    differ = 0
    for p, rid in zip(prompts, rids):
        got = list(p) + list(done[rid].output_ids)
        with torch.no_grad():
            ref = hm.generate(torch.tensor([p]), max_length=40, do_sample=False,
                              eos_token_id=None, pad_token_id=0)[0].tolist()
        assert len(got) == len(ref) == 40
        if got == ref:
            continue
        differ += 1
        n = next(i for i, (a, b) in enumerate(zip(got, ref)) if a != b)
        with torch.no_grad():
            top = hm(torch.tensor([ref[:n]])).logits[0, -1].topk(2).values
        assert (top[0] - top[1]).item() < 0.01 * top[0].abs().item() + 0.01, (n, top)
    assert differ <= 1, differ
