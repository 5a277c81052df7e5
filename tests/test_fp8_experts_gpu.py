"""The grouped FP8 MFMA weight stream (``dli_gemm_fp8_stream_grouped``) and FP8 expert stacks
(``ops.Fp8Experts``) on the GPU: exact witnesses of the scale, expert and K indexing on the
compact tile-list grid, the rows it must leave alone, its epilogues, ``ops.moe_mlp`` under
stream plans and on the dequantise path, what the entry refuses, a quantised Qwen3-MoE model
and the grouped autotune.

The issue's fallback case F = 72 (a down projection with K % 16 != 0) cannot be built: the
16-row gate/up interleave takes F in multiples of 16, and the bf16 grouped GEMMs of the
dequantise path take K in multiples of 64 only. The K rule is covered by ``stream_ok``'s truth
table (tests/test_fp8_experts.py) and by the entry's refusal below."""
import itertools

import pytest
import torch

from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.engine import SamplingParams
from distributed_llm_inferencing_amd.engine.llm_engine import LLMEngine
from distributed_llm_inferencing_amd.models import get_config
from distributed_llm_inferencing_amd.models.model import TransformerLM
from distributed_llm_inferencing_amd.models.weights import quantize_params, random_init, \
    stage_param_shapes
from distributed_llm_inferencing_amd.ops import gemm as G
from distributed_llm_inferencing_amd.ops import reference as R

from test_fp8_stream_gpu import close as _close, rnd

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F8 = torch.float8_e4m3fn
TILES = sorted(G.FP8_STREAM_TILES)
SENT = 777.0


def close(a, b, **kw):
    """``test_fp8_stream_gpu.close`` (rtol = atol = 2e-2 of the reference's max), the figure
    printed before it is asserted."""
    err = (a.float() - b.float()).abs().max().item()
    print(f"max err {err:.4g} of max {b.float().abs().max().item():.4g} on {a.device}")
    _close(a, b, **kw)


def plan(tile, splits=1):
    return G.GemmPlan("dli", tile, splits)


@pytest.fixture
def bf16_calls(monkeypatch):
    """The calls of ``ops.Fp8Experts.bf16`` (the dequantise pass of a stack) during the test."""
    calls = []
    real = ops.Fp8Experts.bf16
    monkeypatch.setattr(ops.Fp8Experts, "bf16", lambda self: (calls.append(1), real(self))[1])
    return calls


@pytest.fixture
def clean_plans():
    saved = dict(G._grouped_cache)
    G._grouped_cache.clear()
    yield
    G._grouped_cache.clear()
    G._grouped_cache.update(saved)


# ----------------------------------------------------------------------------- witnesses
# 80 rows: tails for 64 / 128 weight rows a workgroup; 1040: 9 scale blocks, the last 16 wide.
# Rows per expert: none, one, two 16-row blocks with a tail, one full 64-row item, two with a tail
WE, WN, WK = 5, 80, 1040
COUNTS = [0, 1, 17, 64, 70]
ROWS = sum(COUNTS)                       # 152 routed rows
PAD = 5                                  # rows of the buffers past the routed total
TOKENS = 100                             # the permutation reads 100 tokens: some feed two experts
OFF = [0] + list(itertools.accumulate(COUNTS))
EXPERT_OF = torch.tensor([e for e, c in enumerate(COUNTS) for _ in range(c)])


def witness_scales():
    """(2 i + 1) * 2^-(i % 7) over the 225 (expert, group, block) triples: all distinct, nine
    significant bits at most."""
    kb = -(-WK // 128)
    i = torch.arange(WE * (WN // 16) * kb, dtype=torch.float32)
    s = ((2 * i + 1) * torch.exp2(-(i % 7))).view(WE, WN // 16, kb)
    assert s.numel() == 225 and s.unique().numel() == 225 and 2 * i.max() + 1 < 512
    return s


def arow_of(mode):
    """None (rows in place) or the token behind each permuted row."""
    if mode == "identity":
        return None
    a = (7 * torch.arange(ROWS + PAD) + 3) % TOKENS
    a[ROWS:] = -12345                    # never read: rows past the routed total
    tok = a[:ROWS]
    two = [t for t in tok.unique().tolist()
           if EXPERT_OF[tok == t].unique().numel() > 1]
    assert two, "one token feeds two experts"
    return a.to(torch.int32)


def x_rows(mode):
    return ROWS + PAD if mode == "identity" else TOKENS


def run_stream(gpu, x, w, epi, tile, bm, arow, tl=None, counts=COUNTS, out=None):
    n = sum(counts) + PAD
    off = torch.tensor([0] + list(itertools.accumulate(counts)), dtype=torch.int32, device=gpu)
    if tl is None:
        tl = G.host_tile_list(counts, bm, gpu)
    Nn = w.shape[1]
    if out is None:
        out = torch.full((n, Nn // 2 if epi == "silu_mul" else Nn), SENT,
                         dtype=torch.float32 if epi == "f32" else BF, device=gpu)
    a = None if arow is None else arow.to(gpu)
    ops.grouped_fp8_stream(x, w, plan(tile), epi, out, off, sum(counts), bm, tl, a)
    return out


@pytest.mark.parametrize("mode", ["identity", "permuted"])
@pytest.mark.parametrize("bm", [16, 32, 64])
def test_scale_and_expert_index_witness(gpu, bm, mode):
    """Every weight byte is fp8 1.0, x is one-hot at column k with (m + 1) / 8 in row m:
    y[p, n] = x[arow[p], k] * s[e(p), n // 16, k // 128] exactly. Another expert's weights or
    scales, another block, group or row is a mismatch, not a tolerance question; rows past the
    routed total keep the sentinel."""
    s = witness_scales()
    w = ops.Fp8Experts(torch.ones(WE, WN, WK).to(F8).to(gpu), s.to(gpu))
    arow = arow_of(mode)
    M = x_rows(mode)
    xv = ((torch.arange(M, dtype=torch.float32) + 1) / 8).to(BF)
    assert torch.equal(xv.float(), (torch.arange(M, dtype=torch.float32) + 1) / 8)
    src = torch.arange(ROWS) if arow is None else arow[:ROWS].long()
    for k in (0, 15, 16, 63, 64, 127, 128, 1023, 1024, WK - 17, WK - 1):
        x = torch.zeros(M, WK, dtype=BF)
        x[:, k] = xv
        sk = s[EXPERT_OF, :, k // 128].repeat_interleave(16, dim=1)          # [ROWS, WN]
        want = xv.float()[src][:, None] * sk
        # 9 significant bits times 8 (7 for the 100 tokens): exact in fp32
        assert torch.equal(want.double(), xv.double()[src][:, None] * sk.double())
        xg = x.to(gpu)
        for tile in TILES:
            y = run_stream(gpu, xg, w, "f32", tile, bm, arow)
            if k == WK - 1:
                print(f"tile {tile} bm {bm} {mode}: sum {y[:ROWS].double().sum().item():.6f} "
                      f"want {want.double().sum().item():.6f} on {y.device}")
            assert torch.equal(y[:ROWS].cpu(), want), (k, tile)
            assert bool((y[ROWS:] == SENT).all()), (k, tile)


def pairing_case(mode):
    """One fp8 1.0 per weight row, at k = (37 n + 11 + 101 e) % K; x multiples of 1/8 in
    [-2, 2] (the dense witness's pattern)."""
    s = witness_scales()
    n = torch.arange(WN)
    q = torch.zeros(WE, WN, WK)
    kn = torch.stack([(37 * n + 11 + 101 * e) % WK for e in range(WE)])     # [E, N]
    for e in range(WE):
        q[e, n, kn[e]] = 1.0
    M = x_rows(mode)
    k = torch.arange(WK)[None, :]
    m = torch.arange(M)[:, None]
    x = ((((7 * k + 3 * m) % 31) - 15).float() / 8).to(BF)
    return q.to(F8), s, x, kn


@pytest.mark.parametrize("mode", ["identity", "permuted"])
@pytest.mark.parametrize("bm", [16, 32, 64])
def test_k_pairing_witness(gpu, bm, mode):
    """A weight fragment that met the x fragment of other K indices, or of another item's
    rows, would pick another x value. The expectation is the fp32 reference's, on the CPU."""
    q, s, x, kn = pairing_case(mode)
    arow = arow_of(mode)
    src = torch.arange(ROWS) if arow is None else arow[:ROWS].long()
    wf = R.dequantize_experts(q, s, torch.float32)
    want = torch.cat([R.linear(x[src[OFF[e]:OFF[e + 1]]], wf[e], out_dtype=torch.float32)
                      for e in range(WE)])
    ke = kn[EXPERT_OF]                                                       # [ROWS, N]
    xk = x.float()[src][:, None, :].expand(-1, WN, -1).gather(2, ke[:, :, None])[:, :, 0]
    sk = s[EXPERT_OF].repeat_interleave(16, dim=1).gather(2, (ke // 128)[:, :, None])[:, :, 0]
    direct = xk * sk
    assert torch.equal(want, direct) and want.abs().max() > 0
    w = ops.Fp8Experts(q.to(gpu), s.to(gpu))
    xg = x.to(gpu)
    for tile in TILES:
        y = run_stream(gpu, xg, w, "f32", tile, bm, arow)
        assert torch.equal(y[:ROWS].cpu(), want), tile
        assert bool((y[ROWS:] == SENT).all()), tile


@pytest.mark.parametrize("tile", TILES)
def test_untouched_rows(gpu, tile):
    """A list of one item writes that item's rows of its expert and nothing else: not the
    rows of the next expert that follow them within the item's height, not the pairs that
    stand in the list past its count."""
    s = witness_scales()
    w = ops.Fp8Experts(torch.ones(WE, WN, WK).to(F8).to(gpu), s.to(gpu))
    x = torch.zeros(ROWS + PAD, WK, dtype=BF)
    x[:, 130] = 1.0
    xg = x.to(gpu)
    for bm, (e, r0) in ((16, (2, 16)), (32, (2, 0)), (64, (4, 64)), (16, (1, 0))):
        full, cap = G.host_tile_list(COUNTS, bm, gpu)
        assert [e, r0] in full[1:1 + int(full[0, 0])].tolist()
        one = full.clone()                                   # every pair stays in the list ...
        one[0, 0] = 1                                        # ... but the count says one
        one[1, 0], one[1, 1] = e, r0
        y = run_stream(gpu, xg, w, "f32", tile, bm, None, tl=(one, cap))
        lo = OFF[e] + r0
        hi = min(lo + bm, OFF[e + 1])
        assert hi > lo
        want = s[e, :, 1].repeat_interleave(16)[None, :].expand(hi - lo, -1)
        assert torch.equal(y[lo:hi].cpu(), want), (bm, e)
        assert bool((y[:lo] == SENT).all()) and bool((y[hi:] == SENT).all()), (bm, e)
        # a list written for another item height is not run at all
        other = one.clone()
        other[0, 1] = 48
        y = run_stream(gpu, xg, w, "f32", tile, bm, None, tl=(other, cap))
        assert bool((y == SENT).all()), bm
        none = full.clone()
        none[0, 0] = 0
        y = run_stream(gpu, xg, w, "f32", tile, bm, None, tl=(none, cap))
        assert bool((y == SENT).all()), bm


# ----------------------------------------------------------------------------- epilogues
_refs = {}


def experts_fp8(E, N, K, dev, lo=-10, hi=-2, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(E, N, K, generator=g).to(F8)
    s = torch.exp2(torch.rand(E, N // 16, -(-K // 128), generator=g) * (hi - lo) + lo).float()
    w = ops.Fp8Experts(q.to(dev), s.to(dev))
    return w, w.dequantize(torch.float32)


def epi_case(gpu, K):
    """Operands and the fp32 product through the permutation, once per K."""
    if K not in _refs:
        torch.manual_seed(3)
        w, wf = experts_fp8(WE, 96, K, gpu, seed=K)
        x = rnd(TOKENS, K, dev=gpu)
        arow = arow_of("permuted")
        src = arow[:ROWS].long().to(gpu)
        y = torch.cat([R.linear(x[src[OFF[e]:OFF[e + 1]]], wf[e], out_dtype=torch.float32)
                       for e in range(WE)])
        _refs[K] = (w, x, arow, y)
    return _refs[K]


# K = 2192: 18 blocks, so both rings (4 / 2 blocks) go round several times
@pytest.mark.parametrize("K", [1040, 2192])
@pytest.mark.parametrize("bm", [16, 32, 48, 64])
@pytest.mark.parametrize("epi", ["none", "silu_mul"])
def test_epilogues(gpu, epi, bm, K):
    w, x, arow, y = epi_case(gpu, K)
    ref = R.silu_mul(y.to(BF)) if epi == "silu_mul" else y
    for tile in TILES:
        out = run_stream(gpu, x, w, epi, tile, bm, arow)
        assert out.dtype == BF and out.shape == (ROWS + PAD, 48 if epi == "silu_mul" else 96)
        close(out[:ROWS], ref)
        assert bool((out[ROWS:] == SENT).all())


# ----------------------------------------------------------------------------- refusals
def test_entry_refuses_what_the_kernel_cannot_take(gpu):
    w, _ = experts_fp8(WE, 96, 1040, gpu)
    x = rnd(ROWS + PAD, 1040, dev=gpu)
    out = torch.zeros(ROWS + PAD, 96, dtype=BF, device=gpu)
    off = torch.tensor(OFF, dtype=torch.int32, device=gpu)
    tl, cap = G.host_tile_list(COUNTS, 16, gpu)

    def call(n=ROWS, K=1040, splits=1, bm=16, poff=off, max_items=cap, tile=70, epi="none"):
        ops._native_call("dli_gemm_fp8_stream_grouped", ops._p(x), x.stride(0), ops._p(w.q),
                         ops._p(w.scale), w.scale.stride(1), 1040, ops._p(out), out.stride(0),
                         n, 96, K, G.EPI[epi], tile, splits, bm,
                         None, None if poff is None else ops._p(poff), WE, ops._p(tl), max_items,
                         ops._st())
    call()                                                # the call itself is fine
    name = "dli_gemm_fp8_stream_grouped"
    with pytest.raises(RuntimeError, match=name):         # the bound on the item count
        call(max_items=-(-ROWS // 16) + WE - 1)
    with pytest.raises(RuntimeError, match=name):
        call(poff=None)
    with pytest.raises(RuntimeError, match=name):
        call(splits=2)
    with pytest.raises(RuntimeError, match=name):         # K in whole 16-byte chunks
        call(K=1032)
    with pytest.raises(RuntimeError, match=name):
        call(bm=24)
    with pytest.raises(RuntimeError, match=name):
        call(tile=1)
    with pytest.raises(RuntimeError, match=name):         # no bias epilogue in the grouped form
        call(epi="bias")
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- moe_mlp
SHAPES = {"qwen": dict(E=128, k=8, D=256, F=64), "mixtral": dict(E=4, k=2, D=256, F=256)}
_moe = {}


def moe_case(gpu, kind, T):
    """Stacks, tokens, a routing and the fp32 reference layer, once per (kind, T)."""
    if (kind, T) not in _moe:
        sh = SHAPES[kind]
        E, k, D, F = sh["E"], sh["k"], sh["D"], sh["F"]
        if kind not in _moe:
            _moe[kind] = (experts_fp8(E, 2 * F, D, gpu, lo=-8, hi=-5, seed=1),
                          experts_fp8(E, D, F, gpu, lo=-8, hi=-5, seed=2))
        (wgu, gf), (wd, df) = _moe[kind]
        torch.manual_seed(T)
        x = rnd(T, D, dev=gpu)
        tw, ti = R.router_topk(torch.randn(T, E, device=gpu), k)
        ref = R.moe_mlp(x.float(), gf, df, tw, ti)
        _moe[kind, T] = (wgu, wd, gf, df, x, tw, ti, ref)
    return _moe[kind, T]


def pin(kind, n, p_gu, p_dn):
    sh = SHAPES[kind]
    E, D, F = sh["E"], sh["D"], sh["F"]
    G._grouped_cache[G._grouped_key(n, 2 * F, D, "silu_mul", E, "fp8")] = p_gu
    G._grouped_cache[G._grouped_key(n, D, F, "none", E, "fp8")] = p_dn


@pytest.mark.parametrize("kind,T", [("qwen", 1), ("qwen", 37), ("qwen", 300), ("mixtral", 5),
                                    ("mixtral", 129)])
def test_moe_mlp_streams_and_dequantises(gpu, kind, T, bf16_calls, clean_plans):
    wgu, wd, gf, df, x, tw, ti, ref = moe_case(gpu, kind, T)
    sh = SHAPES[kind]
    n = T * sh["k"]
    assert G.wdt(wgu) == "fp8" and ref.abs().max() > 0
    # untuned: the stream, tile 70
    close(ops.moe_mlp(x, wgu, wd, tw, ti), ref)
    for tile in TILES:
        pin(kind, n, plan(tile), plan(tile))
        close(ops.moe_mlp(x, wgu, wd, tw, ti), ref)
        out = ops.moe_mlp(x, wgu, wd, tw, ti, defer_combine=True)
        assert isinstance(out, torch.Tensor)             # no slab plan: the plain tensor
        close(out, ref)
    assert bf16_calls == []
    # a bf16-family plan pinned under the FP8 key: the dequantise path, one pass per stack
    bf = plan(G.grouped_tile(n, sh["E"]))
    pin(kind, n, bf, bf)
    close(ops.moe_mlp(x, wgu, wd, tw, ti), ref)
    assert len(bf16_calls) == 2
    # gate/up streamed, down dequantised, and the reverse
    pin(kind, n, plan(70), bf)
    close(ops.moe_mlp(x, wgu, wd, tw, ti), ref)
    pin(kind, n, bf, plan(71))
    close(ops.moe_mlp(x, wgu, wd, tw, ti), ref)
    assert len(bf16_calls) == 4
    # the bf16 keys were never touched
    assert all(len(key) == 6 for key in G._grouped_cache)


@pytest.mark.parametrize("kind,T", [("qwen", 37), ("mixtral", 129)])
def test_moe_mlp_expert_range_shard(gpu, kind, T, bf16_calls, clean_plans):
    wgu, wd, gf, df, x, tw, ti, ref = moe_case(gpu, kind, T)
    E = SHAPES[kind]["E"]
    e0, e1 = E // 4, E // 4 + E // 2
    sgu = ops.Fp8Experts(wgu.q[e0:e1].clone(), wgu.scale[e0:e1].clone())
    sdn = ops.Fp8Experts(wd.q[e0:e1].clone(), wd.scale[e0:e1].clone())
    want = R.moe_mlp(x.float(), gf[e0:e1], df[e0:e1], tw, ti, e0)
    assert want.abs().max() > 0
    close(ops.moe_mlp(x, sgu, sdn, tw, ti, e0), want)
    # plan_rows: the rows these experts typically get, the buffer sized for more
    close(ops.moe_mlp(x, sgu, sdn, tw, ti, e0, plan_rows=max(1, T * SHAPES[kind]["k"] // 2)),
          want)
    assert bf16_calls == []


def test_fallbacks_take_the_dequantise_path(gpu, bf16_calls, clean_plans):
    wgu, wd, gf, df, x, tw, ti, ref = moe_case(gpu, "mixtral", 129)
    n = 129 * 2
    # a non-contiguous x: the gate/up projection gathers and dequantises, the down streams
    wide = torch.zeros(129, 2 * 256, dtype=BF, device=gpu)
    xs = wide[:, ::2]
    xs.copy_(x)
    assert not xs.is_contiguous()
    close(ops.moe_mlp(xs, wgu, wd, tw, ti), ref)
    assert len(bf16_calls) == 1
    # a pinned stream plan with splits = 2: no split-K in the grouped stream
    pin("mixtral", n, plan(70, 2), plan(71, 2))
    close(ops.moe_mlp(x, wgu, wd, tw, ti), ref)
    assert len(bf16_calls) == 3
    # a pinned split plan of the bf16 family (the fp16-slab combine): on the bf16 image
    pin("mixtral", n, plan(1), plan(1, 2))
    close(ops.moe_mlp(x, wgu, wd, tw, ti), ref)
    assert len(bf16_calls) == 5
    # K the stream cannot take: never eligible
    odd = ops.Fp8Experts(torch.zeros(4, 32, 72).to(F8).to(gpu), torch.ones(4, 2, 1, device=gpu))
    assert not any(odd.stream_ok(n, 4, plan(t)) for t in TILES)


def test_prefill_sized_call_dequantises(gpu, bf16_calls, clean_plans):
    """4096 routed rows over 4 experts: the eager prefill branch, on the bf16 image."""
    wgu, wd, gf, df, x, tw, ti, ref = moe_case(gpu, "mixtral", 2048)
    close(ops.moe_mlp(x, wgu, wd, tw, ti), ref)
    assert len(bf16_calls) >= 1


# ----------------------------------------------------------------------------- model, engine
CFG = get_config("qwen3-moe-tiny", 2)
IDS = [5, 17, 99, 3, 250, 7, 8, 1000, 42, 11, 600, 3, 3, 9]
BATCH = 8


@pytest.fixture(scope="module")
def fp8_params():
    shapes = stage_param_shapes(CFG, 0, CFG.num_layers, True, True)
    return quantize_params(CFG, random_init(shapes, "cpu", BF, seed=11, std=0.05))


def _decode_spy(monkeypatch, bf16_calls):
    per_step = []
    real = TransformerLM.forward_layers

    def spy(self, x, b, kv_caches):
        n0 = len(bf16_calls)
        out = real(self, x, b, kv_caches)
        if not b.is_prefill and x.is_cuda and x.shape[0] == BATCH:
            per_step.append(len(bf16_calls) - n0)
        return out
    monkeypatch.setattr(TransformerLM, "forward_layers", spy)
    return per_step


def _step_logits(device, params, prompts, steps, monkeypatch, **kw):
    logits = []
    real = TransformerLM.sample

    def spy(self, lg, b, generator=None):
        logits.append(lg.float().cpu())
        return real(self, lg, b, generator=generator)
    monkeypatch.setattr(TransformerLM, "sample", spy)
    eng = LLMEngine(CFG, device=device, params=params, max_batch=8, max_model_len=64,
                    num_blocks=64, use_graphs=False, lookahead=False, **kw)
    sp = SamplingParams(max_new_tokens=steps, temperature=0.0, ignore_eos=True)
    toks = [o.output_ids for o in eng.generate(prompts, sp)]
    monkeypatch.setattr(TransformerLM, "sample", real)
    return eng, toks, logits


def test_model_logits_with_streamed_experts(gpu, fp8_params, bf16_calls, clean_plans,
                                            monkeypatch):
    """Prefill, then decode at batch 8 with the experts on the stream (the untuned plan):
    every step's logits against a CPU engine holding the fp32 reconstruction of the same
    weights, and no dequantise pass of a stack inside the decode steps."""
    monkeypatch.setenv("DLI_GEMM_AUTOTUNE", "0")
    G.clear_plans()
    per_step = _decode_spy(monkeypatch, bf16_calls)
    prompts = [IDS[i:i + 4 + i] for i in range(BATCH)]
    deq = {}
    for k, v in fp8_params.items():
        if k.endswith("_scale"):
            continue
        if v.dtype == F8:
            s = fp8_params[k + "_scale"]
            v = (R.dequantize_experts if v.dim() == 3 else R.dequantize_weight)(
                v, s, torch.float32)
        deq[k] = v
    _, t_ref, l_ref = _step_logits("cpu", deq, prompts, 4, monkeypatch)
    eng, t_gpu, l_gpu = _step_logits("cuda", fp8_params, prompts, 4, monkeypatch)
    assert eng.stats()["weight_dtype"] == "fp8"
    assert eng.memory_report()["weight_dtype"] == "fp8"
    assert isinstance(eng.model.layers[0]["w_gu"], ops.Fp8Experts)
    assert len(l_ref) == len(l_gpu) >= 4
    for i, (a, b) in enumerate(zip(l_gpu, l_ref)):
        assert a.shape == b.shape
        err = (a - b).abs().max().item()
        assert err < 0.05 * b.abs().max().item() + 0.02, (i, err)
        if [t[:i + 1] for t in t_gpu] != [t[:i + 1] for t in t_ref]:
            break                      # a near tie flipped a token: later steps see other inputs
    assert len(per_step) >= 3 and not any(per_step), per_step
    G.clear_plans()


def test_graph_decode_equals_eager_with_streamed_experts(gpu, fp8_params, bf16_calls,
                                                         clean_plans, monkeypatch):
    monkeypatch.setenv("DLI_GEMM_AUTOTUNE", "0")
    G.clear_plans()
    per_step = _decode_spy(monkeypatch, bf16_calls)
    prompts = [IDS[i:i + 4 + i] for i in range(BATCH)]
    sp = SamplingParams(max_new_tokens=12, temperature=0.0, ignore_eos=True)
    outs = []
    for graphs in (False, True):
        eng = LLMEngine(CFG, device="cuda", params=fp8_params, max_batch=8, max_model_len=64,
                        num_blocks=64, use_graphs=graphs)
        assert eng.weight_dtype == "fp8"
        outs.append([o.output_ids for o in eng.generate(prompts, sp)])
    assert outs[0] == outs[1] and all(len(t) == 12 for t in outs[0])
    assert len(per_step) >= 11 and not any(per_step), per_step
    G.clear_plans()


# ----------------------------------------------------------------------------- autotune
def test_autotune_grouped_pins_under_the_fp8_key(gpu, clean_plans):
    (wgu, _), (wd, _) = (experts_fp8(4, 512, 256, gpu, seed=5), experts_fp8(4, 256, 256, gpu,
                                                                          seed=6))
    rows = 64
    for w, epi in ((wgu, "silu_mul"), (wd, "none")):
        E, N, K = w.shape
        best = G.autotune_grouped(rows, w, epi, iters=2)
        assert best is not None and isinstance(best[0], G.GemmPlan) and best[1] > 0
        assert G._grouped_cache[G._grouped_key(rows, N, K, epi, E, "fp8")] == best[0]
        assert G._grouped_key(rows, N, K, epi, E) not in G._grouped_cache
        assert G.grouped_plan(rows, N, K, epi, E, "fp8") == best[0]
        assert G.grouped_plan(rows, N, K, epi, E).tile not in G.FP8_STREAM_TILES
        assert G.autotune_grouped(rows, w, epi) == best[0]          # cached: not timed again
