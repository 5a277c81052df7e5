"""The attention witnesses (tests/attention_witness.py) on the CPU, where the ``ops`` entry
points run ``ops/reference.py``: the unmutated reference reproduces the closed forms, and
every listed mutation of it - the off-by-one, wrong-tile, wrong-block and wrong-head errors an
attention kernel can make - fails at least one witness assertion. The last test records which
of those mutations the random-data comparison of test_kernels_gpu.py accepts."""
import math

import pytest
import torch

import attention_witness as W
from distributed_llm_inferencing_amd import ops
from distributed_llm_inferencing_amd.ops import reference as R

CPU = torch.device("cpu")


# ----------------------------------------------------------------------------- runners
def run_decode(sc, hkv, window, cache=None, scales=None):
    k, v, tables, ctx = cache or W.device_cache(sc, CPU, scales)
    _, hq, hd = sc.q.shape
    ks, vs = scales or (1.0, 1.0)
    return ops.decode_attention(W.device_qkv(sc, hkv, CPU), k, v, tables, ctx, max(sc.ctxs), hq,
                                hkv, hd, 1 / math.sqrt(hd), window=window, k_scale=ks, v_scale=vs)


def run_prefill(sc, hkv, window):
    _, hq, hd = sc.q.shape
    n = int(torch.bincount(sc.seq).max())
    return ops.prefill_attention(W.device_qkv(sc, hkv, CPU), W.cu_seqlens(sc, CPU), n, hq, hkv,
                                 hd, 1 / math.sqrt(hd), window=window)


def run_paged(sc, hkv, window, scales=None):
    k, v, tables, ctx = W.device_cache(sc, CPU, scales)
    _, hq, hd = sc.q.shape
    n = int(torch.bincount(sc.seq).max())
    ks, vs = scales or (1.0, 1.0)
    return ops.prefill_attention_paged(W.device_qkv(sc, hkv, CPU), W.cu_seqlens(sc, CPU), n, ctx,
                                       tables, k, v, hq, hkv, hd, 1 / math.sqrt(hd),
                                       window=window, k_scale=ks, v_scale=vs)


def decode_scenes(hq, hkv, hd, bs, window, ctxs=W.DECODE_CTXS):
    """The scenes of the GPU test, the count scene (where a sequence fits one) first."""
    needles, count = W.decode_scenes(ctxs, hq, hkv, hd, bs, window, seed=window + 1)
    return ([count] if count is not None else []) + needles


# ----------------------------------------------------------------------------- 1. clean
def test_helper_invariants():
    for hkv, hd in ((8, 128), (12, 64), (1, 128)):
        v = W.v_table(torch.arange(1023), hkv, hd).permute(1, 0, 2).reshape(-1, hd)
        assert len(torch.unique(v, dim=0)) == len(v)              # rows distinct, heads too
        assert float(v.abs().max()) <= 2 and torch.equal(v * 8, (v * 8).round())
        assert torch.equal(v.to(torch.bfloat16).float(), v)
        assert torch.equal(R.dequantize_kv(R.quantize_kv(v, 0.5), 0.5), v)
    c = W.code(torch.arange(1 << 16), 64)
    assert len(torch.unique(c, dim=0)) == 1 << 16
    assert W.split_tokens(2100, 4) == 544 and W.split_tokens(1, 4) == 32
    with pytest.raises(AssertionError, match="count witness"):
        W.decode_count([2100], 32, 8, 128, 16, 0, seed=0)
    lay = W.make_layout([1, 100, 33], 16, seed=3)
    used = {b for blocks in lay.blocks for b in blocks}
    assert lay.pad not in used and not used & set(lay.free)
    assert all(int(row[-1]) == lay.pad for row in lay.tables)


@pytest.mark.parametrize("window", W.DECODE_WINDOWS)
@pytest.mark.parametrize("hq,hkv,hd,bs", W.DECODE_SHAPES)
def test_reference_decode_clean(hq, hkv, hd, bs, window):
    scenes = decode_scenes(hq, hkv, hd, bs, window)
    assert scenes[0].kind == "count" and 1023 in scenes[0].ctxs       # whatever 2100 does
    for scales in [None] + W.FP8_SCALES:
        caches = {}
        for sc in scenes:
            cache = caches.setdefault(id(sc.k), W.device_cache(sc, CPU, scales))
            W.check(run_decode(sc, hkv, window, cache, scales), sc,
                    f"reference decode scales {scales} window {window}")


@pytest.mark.parametrize("window", W.DECODE_WINDOWS)
@pytest.mark.parametrize("hq,hkv,hd,bs", W.DECODE_SHAPES)
def test_decode_targets_cover_every_boundary(hq, hkv, hd, bs, window):
    """Every sequence has a head on its first and last visible key and on both sides of every
    tile, KV-block, 64-block table window and KV-split boundary of every split count the GPU
    test launches (as the launcher places them: lo + k * split_tokens)."""
    ctxs = W.DECODE_CTXS
    needles, _ = W.decode_scenes(ctxs, hq, hkv, hd, bs, window, seed=window + 1)
    got = torch.cat([sc.targets for sc in needles], 1)
    for b, L in enumerate(ctxs):
        lo = max(0, L - window) if window > 0 else 0
        bnd = set(range(lo + 32, L, 32)) | set(range(lo // bs * bs + bs, L, bs))
        bnd |= set(range(lo // bs * bs + 64 * bs, L, 64 * bs))
        for st in W.decode_steps(ops, len(ctxs), hkv, ctxs, window):
            bnd |= set(range(lo + st, L, st))
        need = {lo, L - 1} | bnd | {x - 1 for x in bnd}
        have = set(got[b].tolist())
        assert need <= have and min(have) >= lo and max(have) < L, (L, sorted(need - have))


def test_reference_decode_32k_clean():
    hq, hkv, hd, bs = 32, 8, 128, 16
    ctxs = [32768, 77]
    steps = W.decode_steps(ops, 2, hkv, ctxs, 0, [None, 8, 32])
    scenes = W.decode_needle(ctxs, hq, hkv, hd, bs, 0, 1 / math.sqrt(hd), 5)
    tg = set(torch.cat([s.targets[0] for s in scenes]).tolist())
    need = {0, 32767} | {m - j for m in range(1024, 32768, 1024) for j in (0, 1)}
    need |= {k * s - j for s in steps for k in range(1, 32768 // s + 1) for j in (0, 1)
             if k * s < 32768}
    assert need <= tg
    cache = W.device_cache(scenes[0], CPU)
    W.check(run_decode(scenes[0], hkv, 0, cache), scenes[0], "reference decode 32k")


@pytest.mark.parametrize("window", W.PREFILL_WINDOWS)
@pytest.mark.parametrize("hq,hkv,hd", W.PREFILL_SHAPES)
def test_reference_prefill_clean(hq, hkv, hd, window):
    for lens in W.PREFILL_SHORT + W.PREFILL_LONG:
        for kind in ("needle", "count"):
            if kind == "count" and not W.count_ok(max(lens), window, hd):
                continue
            sc = W.prefill_scene(kind, lens, hq, hkv, hd, window, 1 / math.sqrt(hd))
            W.check(run_prefill(sc, hkv, window), sc, f"reference prefill {lens} window {window}")


@pytest.mark.parametrize("scales", [None] + W.FP8_SCALES)
@pytest.mark.parametrize("window", W.PAGED_WINDOWS)
@pytest.mark.parametrize("hq,hkv,hd,bs", W.DECODE_SHAPES[:2])
def test_reference_paged_prefill_clean(hq, hkv, hd, bs, window, scales):
    for kind in ("needle", "count"):
        chunks = [c for c in W.PAGED_CHUNKS
                  if kind == "needle" or W.count_ok(c[0], window, hd)]
        sc = W.paged_prefill_scene(kind, chunks, hq, hkv, hd, bs, window, 1 / math.sqrt(hd), 9)
        W.check(run_paged(sc, hkv, window, scales), sc,
                f"reference paged prefill window {window} scales {scales}")


def test_prefill_needle_has_causal_and_window_decoys():
    """The construction the prefill needle relies on: rows exist whose target's code also
    sits at i + 1 (behind the causal mask) and just below the window."""
    hq, hkv, hd, window = 32, 8, 128, 64
    n = 300
    lab = W._labels(torch.arange(n), hkv, 0)
    t = W.prefill_targets(torch.arange(n), window, hq, hkv, 0, n)
    kvh = torch.arange(hq) // (hq // hkv)
    i = torch.arange(n).view(-1, 1)
    nxt = (i + 1).clamp(max=n - 1)
    causal = (lab[nxt, kvh] == lab[t, kvh]) & (i + 1 < n)
    below = (i - window).clamp(min=0)
    win = (lab[below, kvh] == lab[t, kvh]) & (i - window >= 0)
    assert int(causal.any(1).sum()) > n // 4 and int(win.any(1).sum()) > n // 8


# ----------------------------------------------------------------------------- 2. mutations
def _per_seq(q, kc, vc, tables, ctx, scale, window, ks, vs, fn):
    """decode, one sequence at a time, through ``fn(b, L)`` -> (gather_kv wrapper, L')."""
    out = torch.empty_like(q)
    orig = R.gather_kv
    for b, L in enumerate(ctx.tolist()):
        wrap, L2 = fn(b, L, orig)
        R.gather_kv = wrap
        try:
            out[b:b + 1] = DEC(q[b:b + 1], kc, vc, tables[b:b + 1],
                               torch.tensor([L2], dtype=ctx.dtype), scale, window, ks, vs)
        finally:
            R.gather_kv = orig
    return out


DEC, PRE, PAG = R.decode_attention, R.prefill_attention, R.prefill_attention_paged


def _tile(L):
    return (L - 1) // 2 // 32 * 32        # a whole tile inside [0, L - 1) for L >= 65


def dec_ctx(d):
    return lambda q, kc, vc, bt, ctx, s, w=0, ks=1.0, vs=1.0: DEC(q, kc, vc, bt, ctx + d, s, w, ks, vs)


def dec_win(d):
    return lambda q, kc, vc, bt, ctx, s, w=0, ks=1.0, vs=1.0: DEC(
        q, kc, vc, bt, ctx, s, w + d if w > 0 else 0, ks, vs)


def dec_tile_dropped(q, kc, vc, bt, ctx, s, w=0, ks=1.0, vs=1.0):
    def fn(b, L, orig):
        if L < 65 or w > 0:
            return orig, L
        t0 = _tile(L)

        def g(kc, vc, row, n, ks=1.0, vs=1.0):
            kk, vv = orig(kc, vc, row, n + 32, ks, vs)
            keep = torch.cat([torch.arange(t0), torch.arange(t0 + 32, n + 32)])
            return kk[keep], vv[keep]
        return g, L - 32
    return _per_seq(q, kc, vc, bt, ctx, s, w, ks, vs, fn)


def dec_tile_twice(q, kc, vc, bt, ctx, s, w=0, ks=1.0, vs=1.0):
    def fn(b, L, orig):
        if L < 65 or w > 0:
            return orig, L
        t0 = _tile(L)

        def g(kc, vc, row, n, ks=1.0, vs=1.0):
            kk, vv = orig(kc, vc, row, n - 32, ks, vs)
            idx = torch.cat([torch.arange(t0 + 32), torch.arange(t0, n - 32)])
            return kk[idx], vv[idx]
        return g, L + 32
    return _per_seq(q, kc, vc, bt, ctx, s, w, ks, vs, fn)


def _visible_block(L, w, bs):
    """A KV block that holds visible keys of a sequence of L tokens (the last but one if any)."""
    return max(0, (L - 1) // bs - 1)


def dec_block_pad(q, kc, vc, bt, ctx, s, w=0, ks=1.0, vs=1.0):
    bt = bt.clone()
    pad = int(bt[ctx.argmin(), -1])               # every row's last entry is the pad block
    for b, L in enumerate(ctx.tolist()):
        bt[b, _visible_block(L, w, kc.shape[2])] = pad
    return DEC(q, kc, vc, bt, ctx, s, w, ks, vs)


def dec_block_other_seq(q, kc, vc, bt, ctx, s, w=0, ks=1.0, vs=1.0):
    src = bt.clone()
    bt = bt.clone()
    B = len(ctx)
    for b, L in enumerate(ctx.tolist()):
        j = _visible_block(L, w, kc.shape[2])
        o = (b + 1) % B
        bt[b, j] = src[o, min(j, (int(ctx[o]) - 1) // kc.shape[2])]
    return DEC(q, kc, vc, bt, ctx, s, w, ks, vs)


def dec_q_rolled(q, kc, vc, bt, ctx, s, w=0, ks=1.0, vs=1.0):
    B, hq, hd = q.shape
    hkv = kc.shape[1]
    return DEC(q.reshape(B, hkv, hq // hkv, hd).roll(1, 2).reshape(B, hq, hd), kc, vc, bt, ctx,
               s, w, ks, vs)


def dec_kv_next_head(q, kc, vc, bt, ctx, s, w=0, ks=1.0, vs=1.0):
    return DEC(q, kc.roll(-1, 1), vc.roll(-1, 1), bt, ctx, s, w, ks, vs)


DECODE_MUTATIONS = {
    "context - 1": (dec_ctx(-1), {}),
    "context + 1": (dec_ctx(1), {}),
    "window - 1": (dec_win(-1), {"windows": [33, 40, 1050]}),
    "window + 1": (dec_win(1), {"windows": [32, 40, 1050]}),
    "tile dropped": (dec_tile_dropped, {"windows": [0]}),
    "tile twice": (dec_tile_twice, {"windows": [0]}),
    "block -> pad block": (dec_block_pad, {}),
    "block -> another sequence's": (dec_block_other_seq, {}),
    "query heads rolled in GQA group": (dec_q_rolled, {"shapes": [(32, 8, 128, 16), (8, 1, 128, 16)]}),
    "kv head h reads h + 1": (dec_kv_next_head, {"shapes": [(32, 8, 128, 16), (12, 12, 64, 32)]}),
}


@pytest.mark.parametrize("name", list(DECODE_MUTATIONS))
def test_decode_mutation_is_caught(monkeypatch, name):
    fn, opt = DECODE_MUTATIONS[name]
    monkeypatch.setattr(R, "decode_attention", fn)
    for hq, hkv, hd, bs in opt.get("shapes", W.DECODE_SHAPES):
        for window in opt.get("windows", [0, 40]):
            # the scenes of the GPU test; the first that fails settles it
            caught = any(bool(W.violations(run_decode(sc, hkv, window), sc).any())
                         for sc in decode_scenes(hq, hkv, hd, bs, window))
            assert caught, f"{name}: no witness fails at {(hq, hkv, hd, bs)} window {window}"


def _shift_rows(q, cu, d):
    """Rows moved by d inside each sequence (the rows that fall off keep their own q)."""
    out = q.clone()
    for s, e in zip(cu[:-1].tolist(), cu[1:].tolist()):
        if e - s > abs(d):
            out[s:e] = q[s:e].roll(d, 0)
    return out


def pre_causal(d):
    """Row i sees the keys up to i + d: row i's query run at row i + d, its window widened or
    narrowed by d so that its lower bound stays (rows without a row i + d stay as they are)."""
    def f(q, k, v, cu, s, w=0):
        base = PRE(q, k, v, cu, s, w)
        if w > 0 and w + d <= 0:
            return base
        sh = PRE(_shift_rows(q, cu, d), k, v, cu, s, w + d if w > 0 else 0)
        out = base.clone()
        for a, e in zip(cu[:-1].tolist(), cu[1:].tolist()):
            if e - a > abs(d):
                moved = sh[a:e].roll(-d, 0)
                keep = slice(a, e - d) if d > 0 else slice(a - d, e)
                out[keep] = moved[keep.start - a:keep.stop - a]
        return out
    return f


def pre_win(d):
    return lambda q, k, v, cu, s, w=0: PRE(q, k, v, cu, s, w + d if w > 0 else 0)


def pre_kv_next_head(q, k, v, cu, s, w=0):
    return PRE(q, k.roll(-1, 1), v.roll(-1, 1), cu, s, w)


PREFILL_MUTATIONS = {
    "causal bound + 1": (pre_causal(1), [0, 64]),
    "causal bound - 1": (pre_causal(-1), [0, 64]),
    "window - 1": (pre_win(-1), [63, 64, 65]),
    "window + 1": (pre_win(1), [63, 64, 65]),
    "kv head h reads h + 1": (pre_kv_next_head, [0]),
}


@pytest.mark.parametrize("name", list(PREFILL_MUTATIONS))
def test_prefill_mutation_is_caught(monkeypatch, name):
    fn, windows = PREFILL_MUTATIONS[name]
    monkeypatch.setattr(R, "prefill_attention", fn)
    for hq, hkv, hd in W.PREFILL_SHAPES:
        for window in windows:
            # (a window mutation changes nothing in prompts shorter than the window)
            for lens in ([[300, 65]] if name.startswith("window") else [[1, 7, 33, 64], [300, 65]]):
                caught = []
                for kind in ("needle", "count"):
                    sc = W.prefill_scene(kind, lens, hq, hkv, hd, window, 1 / math.sqrt(hd))
                    caught.append(bool(W.violations(run_prefill(sc, hkv, window), sc).any()))
                assert any(caught), f"{name}: no witness fails at {lens} window {window}"
                if lens[0] == 300 and name[:6] in ("causal", "window"):
                    assert caught[0], f"{name}: the needle's decoys miss it at {lens}, {window}"


def pag_offset(d):
    return lambda q, kc, vc, cu, ctx, bt, s, w=0, ks=1.0, vs=1.0: PAG(
        q, kc, vc, cu, ctx + d, bt, s, w, ks, vs)


def pag_win(d):
    return lambda q, kc, vc, cu, ctx, bt, s, w=0, ks=1.0, vs=1.0: PAG(
        q, kc, vc, cu, ctx, bt, s, w + d if w > 0 else 0, ks, vs)


def pag_block_pad(q, kc, vc, cu, ctx, bt, s, w=0, ks=1.0, vs=1.0):
    bt = bt.clone()
    pad = int(bt[ctx.argmin(), -1])
    for b, L in enumerate(ctx.tolist()):
        bt[b, (L - 1) // kc.shape[2]] = pad
    return PAG(q, kc, vc, cu, ctx, bt, s, w, ks, vs)


def pag_block_other_seq(q, kc, vc, cu, ctx, bt, s, w=0, ks=1.0, vs=1.0):
    src, bt = bt.clone(), bt.clone()
    for b, L in enumerate(ctx.tolist()):
        bt[b, (L - 1) // kc.shape[2]] = src[(b + 1) % len(ctx), 0]
    return PAG(q, kc, vc, cu, ctx, bt, s, w, ks, vs)


PAGED_MUTATIONS = {
    "chunk offset + 1": (pag_offset(1), [0, 48]),
    "chunk offset - 1": (pag_offset(-1), [0, 48]),
    "window - 1": (pag_win(-1), [48]),
    "window + 1": (pag_win(1), [48]),
    "block -> pad block": (pag_block_pad, [0, 48]),
    "block -> another sequence's": (pag_block_other_seq, [0, 48]),
}
MUT_CHUNKS = [(100, 37), (16, 16), (129, 1), (33, 32), (300, 9)]


@pytest.mark.parametrize("name", list(PAGED_MUTATIONS))
def test_paged_prefill_mutation_is_caught(monkeypatch, name):
    fn, windows = PAGED_MUTATIONS[name]
    monkeypatch.setattr(R, "prefill_attention_paged", fn)
    for hq, hkv, hd, bs in W.DECODE_SHAPES[:2]:
        for window in windows:
            caught = []
            for kind in ("needle", "count"):
                sc = W.paged_prefill_scene(kind, MUT_CHUNKS, hq, hkv, hd, bs, window,
                                           1 / math.sqrt(hd), 9)
                caught.append(bool(W.violations(run_paged(sc, hkv, window), sc).any()))
            assert any(caught), f"{name}: no witness fails at {(hq, hkv, hd, bs)} window {window}"


# ----------------------------------------------------------------------------- 3. the record
def test_random_data_accepts_off_by_one(capsys):
    """Why the witnesses exist: on the Gaussian inputs of test_kernels_gpu.py, ``close()``
    accepts a decode reference that drops the last key or reads one key too many at 1025
    keys (and prints what else it accepts at 700 and 1025)."""
    from test_kernels_gpu import _paged_setup, close
    hq, hkv, hd, bs = 32, 8, 128, 16
    lens = [700, 1025]
    nblk = sum(-(-n // bs) for n in lens) + 8
    qkv_all, pos, slots, kc, vc, tables = _paged_setup(CPU, lens, hq, hkv, hd, bs, nblk)
    cs = R.rope_cos_sin(2048, hd, 10000.0)
    R.rope_and_cache(qkv_all, pos, slots, cs, kc, vc, hq, hkv, hd)
    # the slots past each context and the unused blocks hold what a cache in service holds
    # there: other tokens' rows (zeros would make "one key too many" a no-op for V)
    used = torch.zeros(nblk * bs, dtype=torch.bool)
    used[slots.long()] = True
    free = (~used).view(nblk, 1, bs, 1).expand_as(kc)
    kc[free] = torch.randn(int(free.sum())).to(kc.dtype)
    vc[free] = torch.randn(int(free.sum())).to(vc.dtype)
    q = torch.randn(len(lens), hq, hd).to(torch.bfloat16)
    scale = 1 / math.sqrt(hd)
    accepted = {}
    for b, L in enumerate(lens):
        one = lambda fn: fn(q[b:b + 1], kc, vc, tables[b:b + 1],
                            torch.tensor([L], dtype=torch.int32), scale)
        ref = one(DEC)
        for name in ("context - 1", "context + 1", "tile dropped", "tile twice",
                     "block -> pad block", "kv head h reads h + 1"):
            try:
                close(one(DECODE_MUTATIONS[name][0]), ref)
                accepted[(L, name)] = True
            except AssertionError:
                accepted[(L, name)] = False
    with capsys.disabled():
        for (L, name), ok in accepted.items():
            print(f"\nrandom data, context {L}: close() {'ACCEPTS' if ok else 'rejects'} {name}",
                  end="")
        print()
    assert accepted[(1025, "context - 1")] and accepted[(1025, "context + 1")]
