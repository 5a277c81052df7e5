"""Structured attention inputs ("witnesses") whose exact output is known in closed form, so
that every key position is observable on its own (random Q/K/V hide a wrong key behind a
tolerance that does not shrink with the context, see docs/DESIGN.md).

* needle: every key row carries a +-C code of its position (16 bits, each repeated hd/16
  times); a query that is the code of t* scores ``gap`` natural-log units above every other
  visible key, the softmax is one-hot and the output is ``V[t*]``, a table of values exact in
  bf16 and e4m3. Every query head of every row has its own target.
* count: q = 0, so every visible key has p = 1 exactly, and V[t, d] = [t mod hd == d]: the
  output is n_d / n. Decisive only while hd / n is well above the tolerance: spans <= 16 hd.
* poison: every cache slot a kernel could touch but must not use (past the context, below the
  window, blocks in no table, the pad block of unused table entries) holds finite V = +-64 and,
  in the needle witness, a K that is the code of one of the batch's targets. Finite, because
  the kernels multiply p = 0 by the V rows of masked slots and the cache is zero-initialised:
  NaN there would assert a contract the project does not make.

Everything is built on the CPU in fp32 (all values are exact in bf16 and e4m3) and moved by
the caller. Nothing here indexes outside a cache: unused table entries point at a pad block.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import torch

C = 6.0            # |K|, |Q| of a code element: exact in bf16 and e4m3 (also halved/doubled)
POISON = 64.0      # |V| of a slot that must not be used
BITS = 16
REL = 2.0 ** -7    # P -> bf16 (2^-9), out -> bf16 (2^-9), exp2 and 1/l in fp32: < 2^-8, doubled
COUNT_SPAN = 16    # the count witness needs spans of <= COUNT_SPAN * hd keys


def code(t: torch.Tensor, hd: int) -> torch.Tensor:
    """[..., hd] fp32: bit j of t as -C / +C in dims [j hd/16, (j+1) hd/16)."""
    assert hd % BITS == 0
    t = torch.as_tensor(t, dtype=torch.long)
    assert int(t.max()) < (1 << BITS) and int(t.min()) >= 0
    bits = (t.unsqueeze(-1) >> torch.arange(BITS)) & 1
    return ((bits * 2 - 1).float() * C).repeat_interleave(hd // BITS, dim=-1)


def gap(hd: int, scale: float) -> float:
    """Score of the target above any key whose code differs in >= 1 bit, natural-log units."""
    return C * C * scale * 2 * (hd // BITS)


def v_table(t: torch.Tensor, hkv: int, hd: int) -> torch.Tensor:
    """[n, hkv, hd] fp32, multiples of 1/8 in [-2, 2]. Even dims run mod 33 and odd dims mod 31,
    so two rows of a kv head agree only 1023 positions apart, and the slope over d is the kv
    head's own (3 + kvh), so rows of different kv heads never agree."""
    assert hkv + 3 < 31
    t = torch.as_tensor(t, dtype=torch.long).view(-1, 1, 1)
    k = torch.arange(hkv).view(1, -1, 1)
    d = torch.arange(hd).view(1, 1, -1)
    x = 5 * t + (3 + k) * d
    return torch.where(d % 2 == 0, (x % 33 - 16) / 8.0, (x % 31 - 15) / 8.0).float()


def v_count(t: torch.Tensor, hkv: int, hd: int) -> torch.Tensor:
    t = torch.as_tensor(t, dtype=torch.long).view(-1, 1, 1)
    return (t % hd == torch.arange(hd).view(1, 1, -1)).float().expand(-1, hkv, -1).clone()


def v_poison(n: int, hkv: int, hd: int) -> torch.Tensor:
    sign = 1.0 - 2.0 * (torch.arange(hd) % 2).float()
    return (sign * POISON).expand(n, hkv, hd).clone()


def win_lo(pos, window: int):
    """First key the query at ``pos`` sees (window 0 = full attention)."""
    if window <= 0:
        return pos * 0
    return (pos - window + 1).clamp(min=0) if torch.is_tensor(pos) else max(0, pos - window + 1)


# ----------------------------------------------------------------------------- paged layout
@dataclass
class Layout:
    """Scattered block ids for sequences of ``ctxs`` tokens. Every table row ends in at least
    one unused entry; all unused entries name the pad block, and ``free`` blocks are in no
    table. Every id is < nblk."""
    bs: int
    nblk: int
    pad: int
    free: List[int]
    blocks: List[List[int]]
    tables: torch.Tensor      # int32 [B, width]


def make_layout(ctxs: Sequence[int], bs: int, seed: int, spare: int = 2) -> Layout:
    g = torch.Generator().manual_seed(seed)
    nb = [-(-c // bs) for c in ctxs]
    nblk = sum(nb) + 1 + spare
    perm = torch.randperm(nblk, generator=g).tolist()
    pad, free, o = perm[0], perm[1:1 + spare], 1 + spare
    width = max(nb) + 1
    blocks, rows = [], []
    for n in nb:
        blocks.append(perm[o:o + n])
        rows.append(perm[o:o + n] + [pad] * (width - n))
        o += n
    tables = torch.tensor(rows, dtype=torch.int32)
    assert 0 <= int(tables.min()) and int(tables.max()) < nblk
    return Layout(bs, nblk, pad, free, blocks, tables)


def fill_cache(lay: Layout, hkv: int, hd: int, seq_k, seq_v, decoy: Optional[torch.Tensor]):
    """Caches [nblk, hkv, bs, hd] fp32 from per-sequence rows [nb * bs, hkv, hd] (the caller
    has poisoned the slots past the context). Blocks of no sequence: V poison, K the ``decoy``
    codes [n, hd] in turn (zeros if None)."""
    bs = lay.bs
    n = lay.nblk * bs
    if decoy is None:
        k = torch.zeros(n, hkv, hd)
    else:
        idx = (torch.arange(n).view(-1, 1) * hkv + torch.arange(hkv).view(1, -1)) % len(decoy)
        k = decoy[idx]
    v = v_poison(n, hkv, hd)
    k = k.view(lay.nblk, bs, hkv, hd).permute(0, 2, 1, 3).contiguous()
    v = v.view(lay.nblk, bs, hkv, hd).permute(0, 2, 1, 3).contiguous()
    for blocks, sk, sv in zip(lay.blocks, seq_k, seq_v):
        b = torch.tensor(blocks, dtype=torch.long)
        k[b] = sk.view(len(blocks), bs, hkv, hd).permute(0, 2, 1, 3)
        v[b] = sv.view(len(blocks), bs, hkv, hd).permute(0, 2, 1, 3)
    return k, v


# ----------------------------------------------------------------------------- scenes
@dataclass
class Scene:
    """One witness input. ``q`` [N, hq, hd] fp32 (N = query rows: sequences for decode, packed
    tokens for prefill) with ``expected`` / ``tol`` of the same shape; ``seq`` / ``pos`` [N] name
    the sequence and position of each row, ``targets`` [N, hq] the needle positions (None for
    count). Paged scenes carry ``k`` / ``v`` caches, ``lay`` and ``ctxs``; contiguous prefill
    scenes carry ``k_rows`` / ``v_rows`` [N, hkv, hd]."""
    kind: str
    q: torch.Tensor
    expected: torch.Tensor
    tol: torch.Tensor
    seq: torch.Tensor
    pos: torch.Tensor
    targets: Optional[torch.Tensor] = None
    k: Optional[torch.Tensor] = None
    v: Optional[torch.Tensor] = None
    lay: Optional[Layout] = None
    ctxs: List[int] = field(default_factory=list)
    k_rows: Optional[torch.Tensor] = None
    v_rows: Optional[torch.Tensor] = None

    def qkv(self, hkv: int) -> torch.Tensor:
        """[N, (hq + 2 hkv) hd] fp32. Contiguous prefill: the scene's K / V rows; paged ops
        never read the k / v columns, which are poison."""
        n, hq, hd = self.q.shape
        if self.k_rows is not None:
            kr, vr = self.k_rows, self.v_rows
        else:
            kr = self.q[:, :1].expand(n, hkv, hd)
            vr = v_poison(n, hkv, hd)
        return torch.cat([self.q.reshape(n, -1), kr.reshape(n, -1), vr.reshape(n, -1)], 1)


def needle_tol(expected, n_keys, hd: int, scale: float):
    """|out - V[t*]| <= 2^-7 |V[t*]| + n exp(-gap) max|V| (the softmax mass off the target)."""
    leak = n_keys.float() * math.exp(-gap(hd, scale)) * 2.0
    return REL * expected.abs() + leak.view(-1, 1, 1)


def count_expected(lo, hi, hd: int, drop=None):
    """(expected, tol) [N, 1, hd] of the count witness over the keys [lo, hi] (inclusive, [N]):
    n_d / n; ``drop`` [N]: a position inside the span whose V row is zero (the fused decode
    kernel's new token) - counted in n, not in n_d. Relative 2^-7 on non-zero elements,
    absolute 2^-7 / n on zeros."""
    n = hi - lo + 1
    assert int(n.min()) >= 1 and int(n.max()) <= COUNT_SPAN * hd, \
        f"count witness: spans of {int(n.min())}..{int(n.max())} keys, need 1..{COUNT_SPAN * hd}"
    d = torch.arange(hd).view(1, -1)
    cnt = lambda x: (x.view(-1, 1) - d) // hd + 1           # keys p <= x with p mod hd == d
    nd = cnt(hi) - cnt(lo - 1)
    if drop is not None:
        nd = nd - (drop.view(-1, 1) % hd == d).long()
    exp = nd.float() / n.view(-1, 1).float()
    tol = torch.where(nd > 0, REL * exp, REL / n.view(-1, 1).float())
    return exp.unsqueeze(1), tol.unsqueeze(1)


# ----------------------------------------------------------------------------- decode
def split_tokens(span: int, splits: int, tile: int = 32) -> int:
    """Tokens per KV split as the decode launchers compute it."""
    per = -(-span // splits)
    return max(tile, -(-per // tile) * tile)


def decode_boundaries(L: int, lo: int, bs: int) -> List[int]:
    """Every position in (lo, L) where a decode kernel can change what it reads: the 32-key
    tile starts lo + 32 j (KV-split starts, the workgroup form's wave slices and the
    block-table window refreshes are among them: all are whole tiles from lo) and the KV-block
    starts (multiples of the block size)."""
    return sorted(set(range(lo + 32, L, 32)) | set(range(lo // bs * bs + bs, L, bs)))


def decode_targets(L: int, lo: int, bs: int, n: int, g) -> List[int]:
    """The needle targets of a sequence that sees [lo, L): lo, L - 1 and both sides of every
    ``decode_boundaries`` position, each once; seeded random positions fill the last round of
    n heads."""
    out = [lo, L - 1]
    for b in decode_boundaries(L, lo, bs):
        out += [b - 1, b]
    out = list(dict.fromkeys(out))
    while len(out) % n:
        out.append(lo + int(torch.randint(0, L - lo, (1,), generator=g)))
    return out


def _decode_rows(ctxs, lay, window):
    seqs = []
    for L, blocks in zip(ctxs, lay.blocks):
        lo = max(0, L - window) if window > 0 else 0
        pos = torch.arange(len(blocks) * lay.bs)
        seqs.append((L, lo, pos, (pos >= lo) & (pos < L)))
    return seqs


def decode_needle(ctxs, hq, hkv, hd, bs, window, scale, seed) -> List[Scene]:
    """Needle scenes over ONE cache: as many rounds of queries as it takes to give every
    target of ``decode_targets`` a head (the scenes share k / v / lay). Slots below the window
    and past the context hold poison V and the code of a target of that (sequence, kv group)."""
    g = torch.Generator().manual_seed(seed)
    lay = make_layout(ctxs, bs, seed)
    G = hq // hkv
    rows = _decode_rows(ctxs, lay, window)
    tg = [decode_targets(L, lo, bs, hq, g) for L, lo, _, _ in rows]
    rounds = max(len(t) for t in tg) // hq
    tg = torch.tensor([[t[i % len(t)] for i in range(rounds * hq)] for t in tg])  # [B, R*hq]
    seq_k, seq_v = [], []
    for b, (L, lo, pos, vis) in enumerate(rows):
        k = code(pos, hd).unsqueeze(1).repeat(1, hkv, 1)
        v = v_table(pos, hkv, hd)
        # decoy of slot p, kv head kvh: the target of a head of that group, in turn
        dec = tg[b][(pos.view(-1, 1) % (rounds * G)) // G * hq
                    + torch.arange(hkv).view(1, -1) * G + pos.view(-1, 1) % G]
        k[~vis] = code(dec, hd)[~vis]
        v[~vis] = v_poison(int((~vis).sum()), hkv, hd)
        seq_k.append(k)
        seq_v.append(v)
    kc, vc = fill_cache(lay, hkv, hd, seq_k, seq_v, code(tg.reshape(-1), hd))
    n_keys = torch.tensor([L - lo for L, lo, _, _ in rows])
    kvh = torch.arange(hq) // G
    scenes = []
    for r in range(rounds):
        t = tg[:, r * hq:(r + 1) * hq]
        exp = v_table(t.reshape(-1), hkv, hd).view(len(ctxs), hq, hkv, hd)[:, torch.arange(hq), kvh]
        scenes.append(Scene("needle", code(t, hd), exp, needle_tol(exp, n_keys, hd, scale),
                            torch.arange(len(ctxs)), torch.tensor(ctxs) - 1, t, kc, vc, lay,
                            list(ctxs)))
    return scenes


def decode_count(ctxs, hq, hkv, hd, bs, window, seed, new_token: bool = False) -> Scene:
    """Count scene. ``new_token``: the slot of position L - 1 holds poison for a kernel that
    writes that token's (zero) K / V row itself before it attends (the fused decode kernel)."""
    lay = make_layout(ctxs, bs, seed)
    seq_k, seq_v = [], []
    for L, lo, pos, vis in _decode_rows(ctxs, lay, window):
        if new_token:
            vis = vis & (pos != L - 1)
        v = v_count(pos, hkv, hd)
        v[~vis] = v_poison(int((~vis).sum()), hkv, hd)
        seq_k.append(code(pos, hd).unsqueeze(1).repeat(1, hkv, 1))
        seq_v.append(v)
    kc, vc = fill_cache(lay, hkv, hd, seq_k, seq_v, None)
    hi = torch.tensor(ctxs) - 1
    lo = torch.tensor([max(0, L - window) if window > 0 else 0 for L in ctxs])
    exp, tol = count_expected(lo, hi, hd, hi if new_token else None)
    B = len(ctxs)
    return Scene("count", torch.zeros(B, hq, hd), exp.expand(B, hq, hd), tol.expand(B, hq, hd),
                 torch.arange(B), hi, None, kc, vc, lay, list(ctxs))


def count_ok(max_keys: int, window: int, hd: int) -> bool:
    """Whether the count witness applies to queries that see up to ``max_keys`` keys."""
    return (min(max_keys, window) if window > 0 else max_keys) <= COUNT_SPAN * hd


def decode_scenes(ctxs, hq, hkv, hd, bs, window, seed):
    """(needle rounds over all of ``ctxs``, count scene or None): the count scene holds the
    sequences of the batch whose visible span meets its condition."""
    needles = decode_needle(ctxs, hq, hkv, hd, bs, window, 1 / math.sqrt(hd), seed)
    fit = [L for L in ctxs if count_ok(L, window, hd)]
    return needles, decode_count(fit, hq, hkv, hd, bs, window, seed + 1) if fit else None


# ----------------------------------------------------------------------------- prefill
def _pair_phase(kvh, seq: int):
    return 1 + (kvh + seq) % 2


def _labels(pos, hkv: int, seq: int):
    """[n, hkv] labels of the key codes. Keys (a, a + 1) with a mod 4 == phase(kv head,
    sequence) share the label a: to the query whose target is one of them the other is a decoy
    with the very same score. A row whose last visible key is such an ``a`` has its decoy at
    i + 1, behind the causal mask; a row whose first visible key is an ``a + 1`` has it at
    lo - 1, just below its window. Rows that see both keys of a pair target neither."""
    p = pos.view(-1, 1)
    ph = _pair_phase(torch.arange(hkv).view(1, -1), seq)
    second = (p >= 1) & ((p - 1) % 4 == ph)
    return torch.where(second, p - 1, p.expand(-1, hkv))


def prefill_targets(qpos, window: int, hq: int, hkv: int, seq: int, ctx: int):
    """[n, hq] targets for the queries at ``qpos`` of a ``ctx``-token sequence: in turn
    (by row + head) the row itself, its lower bound, the multiple of 64 at or below it and one
    less; the first of them (then i - 1, i - 2, i - 3) that is visible and whose label no other
    visible key shares."""
    assert window != 2, "window 2: a row's two visible keys can be one decoy pair"
    i = qpos.view(-1, 1, 1)
    lo = win_lo(i, window)
    h = torch.arange(hq).view(1, -1, 1)
    m64 = i // 64 * 64
    cyc = torch.cat([i, lo, m64, m64 - 1], -1).expand(-1, hq, -1)               # [n, hq, 4]
    rot = (torch.arange(4).view(1, 1, -1) + i + h) % 4
    cand = torch.cat([cyc.gather(-1, rot), (i - 1).expand(-1, hq, -1),
                      (i - 2).expand(-1, hq, -1), (i - 3).expand(-1, hq, -1)], -1)
    ph = _pair_phase(h // (hq // hkv), seq)
    first = (cand % 4 == ph) & (cand + 1 < ctx)
    second = (cand >= 1) & ((cand - 1) % 4 == ph)
    ok = (cand >= lo) & (cand <= i) & ~(first & (cand + 1 <= i)) & ~(second & (cand - 1 >= lo))
    assert bool(ok.any(-1).all()), "a row has no unambiguous target"
    return cand.gather(-1, ok.int().argmax(-1, keepdim=True)).squeeze(-1)


def _prefill_seq(kind, qpos, ctx, hq, hkv, hd, window, scale, seq):
    """K / V rows [ctx, hkv, hd] of one sequence and q / expected / tol / targets of its
    queries at ``qpos`` (contiguous prefill: qpos = arange(ctx))."""
    pos = torch.arange(ctx)
    lo = win_lo(qpos, window)
    if kind == "count":
        exp, tol = count_expected(lo, qpos, hd)
        n = len(qpos)
        return (code(pos, hd).unsqueeze(1).repeat(1, hkv, 1), v_count(pos, hkv, hd),
                torch.zeros(n, hq, hd), exp.expand(n, hq, hd), tol.expand(n, hq, hd), None)
    lab = _labels(pos, hkv, seq)
    t = prefill_targets(qpos, window, hq, hkv, seq, ctx)
    kvh = (torch.arange(hq) // (hq // hkv)).view(1, -1).expand_as(t)
    q = code(lab[t, kvh], hd)
    exp = v_table(pos, hkv, hd)[t, kvh]
    return (code(lab, hd), v_table(pos, hkv, hd), q, exp,
            needle_tol(exp, qpos - lo + 1, hd, scale), t)


def prefill_scene(kind, lens, hq, hkv, hd, window, scale) -> Scene:
    """Contiguous causal prefill over prompts of ``lens`` tokens."""
    parts = [_prefill_seq(kind, torch.arange(n), n, hq, hkv, hd, window, scale, s)
             for s, n in enumerate(lens)]
    cat = lambda j: torch.cat([p[j] for p in parts])
    seq = torch.cat([torch.full((n,), s) for s, n in enumerate(lens)])
    pos = torch.cat([torch.arange(n) for n in lens])
    return Scene(kind, cat(2), cat(3), cat(4), seq, pos, None if kind == "count" else cat(5),
                 k_rows=cat(0), v_rows=cat(1))


def paged_prefill_scene(kind, chunks, hq, hkv, hd, bs, window, scale, seed) -> Scene:
    """Chunked prefill: ``chunks`` = (ctx, len) per sequence, the queries at [ctx - len, ctx)
    over the ctx cached keys. Slots no row sees - past the context, and below the window of
    the chunk's first row - hold poison V and, for the needle, the code of a target of the
    chunk's last / first row."""
    ctxs = [c for c, _ in chunks]
    lay = make_layout(ctxs, bs, seed)
    G = hq // hkv
    parts, seq_k, seq_v, decoy = [], [], [], []
    for s, ((ctx, n), blocks) in enumerate(zip(chunks, lay.blocks)):
        p = _prefill_seq(kind, torch.arange(ctx - n, ctx), ctx, hq, hkv, hd, window, scale, s)
        parts.append(p)
        tail = len(blocks) * bs - ctx
        below = int(win_lo(ctx - n, window))          # keys [0, below) are seen by no row

        def codes(row, slots):                        # that row's query codes over the slots
            if kind == "count":
                return torch.zeros(len(slots), hkv, hd)
            return p[2][row].view(hkv, G, hd)[:, slots % G].permute(1, 0, 2)
        k, v = p[0].clone(), p[1].clone()
        k[:below] = codes(0, torch.arange(below))
        v[:below] = v_poison(below, hkv, hd)
        if kind == "needle":
            decoy += [p[2][0], p[2][-1]]
        seq_k.append(torch.cat([k, codes(-1, torch.arange(tail))]))
        seq_v.append(torch.cat([v, v_poison(tail, hkv, hd)]))
    kc, vc = fill_cache(lay, hkv, hd, seq_k, seq_v, torch.cat(decoy) if decoy else None)
    cat = lambda j: torch.cat([p[j] for p in parts])
    seq = torch.cat([torch.full((n,), s) for s, (_, n) in enumerate(chunks)])
    pos = torch.cat([torch.arange(c - n, c) for c, n in chunks])
    return Scene(kind, cat(2), cat(3), cat(4), seq, pos, None if kind == "count" else cat(5),
                 kc, vc, lay, ctxs)


# ----------------------------------------------------------------------------- the assertion
def violations(out, sc: Scene):
    """Boolean [N, hq, hd]: elements of ``out`` outside the scene's tolerance (or not finite)."""
    o = out.detach().float().cpu().reshape(sc.expected.shape)
    return ~((o - sc.expected).abs() <= sc.tol)


def check(out, sc: Scene, what: str) -> None:
    """Assert ``out`` ([N, hq * hd] or [N, hq, hd]) equals the scene's closed form; the message
    names ``what`` (entry point, form, splits, window), the sequence, head, position, target."""
    bad = violations(out, sc)
    if not bool(bad.any()):
        return
    o = out.detach().float().cpu().reshape(sc.expected.shape)
    excess = ((o - sc.expected).abs() - sc.tol).nan_to_num(nan=float("inf")) * bad
    n, h, d = [int(x) for x in torch.unravel_index(excess.argmax(), excess.shape)]
    tgt = "" if sc.targets is None else f" target {int(sc.targets[n, h])}"
    raise AssertionError(
        f"{what} [{sc.kind}]: {int(bad.any(-1).sum())} (row, head) pairs wrong; worst: sequence "
        f"{int(sc.seq[n])} position {int(sc.pos[n])} head {h}{tgt} dim {d}: got {float(o[n, h, d])!r}"
        f", expected {float(sc.expected[n, h, d])!r} +- {float(sc.tol[n, h, d]):.3g}")


# ----------------------------------------------------------------------------- shared cases
DECODE_SHAPES = [(32, 8, 128, 16), (12, 12, 64, 32), (8, 1, 128, 16)]      # hq, hkv, hd, bs
DECODE_CTXS = [1, 31, 32, 33, 100, 1023, 1024, 1025, 2100]
DECODE_WINDOWS = [0, 1, 32, 33, 40, 1050]
DECODE_SPLITS = [1, 2, 4, None]
FP8_SCALES = [(1.0, 1.0), (0.5, 0.5)]
FUSED_LENS = [1, 5, 33, 100, 200, 17, 130]
PREFILL_SHAPES = [(32, 8, 128), (12, 12, 64)]                              # hq, hkv, hd
PREFILL_SHORT = [[1, 7, 33, 64], [16, 3], [32] * 5]
PREFILL_LONG = [[300, 65], [1000, 400, 5, 700]]
PREFILL_WINDOWS = [0, 1, 63, 64, 65, 200]
PAGED_CHUNKS = [(100, 37), (2053, 512), (16, 16), (1, 1), (129, 1), (33, 32), (300, 9)]
PAGED_WINDOWS = [0, 48]


def decode_steps(ops, B, hkv, ctxs, window, splits=DECODE_SPLITS):
    """The split_tokens of every split count a test launches (None = the default heuristic)."""
    span = ops.decode_span(max(ctxs), window)
    ns = {s if s is not None else ops.decode_num_splits(B, hkv, span) for s in splits}
    return sorted({split_tokens(span, s) for s in ns if s > 1})


def device_cache(sc: Scene, device, scales=None):
    """(k_cache, v_cache, block_tables, context_lens) of a paged scene on ``device``: bf16, or
    with ``scales`` = (k_scale, v_scale) FP8 through ``reference.quantize_kv``."""
    from distributed_llm_inferencing_amd.ops import reference as R
    if scales is None:
        k, v = sc.k.to(torch.bfloat16), sc.v.to(torch.bfloat16)
    else:
        k, v = R.quantize_kv(sc.k, scales[0]), R.quantize_kv(sc.v, scales[1])
        assert torch.equal(R.dequantize_kv(k, scales[0]), sc.k), "witness values exact in e4m3"
    return (k.to(device), v.to(device), sc.lay.tables.to(device),
            torch.tensor(sc.ctxs, dtype=torch.int32, device=device))


def device_qkv(sc: Scene, hkv: int, device):
    return sc.qkv(hkv).to(device, torch.bfloat16)


def cu_seqlens(sc: Scene, device):
    n = torch.bincount(sc.seq)
    return torch.cat([torch.zeros(1, dtype=torch.long), n.cumsum(0)]).to(device, torch.int32)
