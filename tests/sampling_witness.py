"""Witnesses for the on-device sampler (csrc/kernels/sampling.hip): inputs for which exactly
one token is correct, and the CPU arithmetic that says which.

The sampler's randomness is a pure function, Philox4x32-10 of (row seed, fixed counter), so
the CPU computes the very 24-bit uniform the kernel will use and picks seeds that land the
draw where a bug would show. Nothing here imports the native library.

* ``philox4x32_10`` / ``draw_u24`` / ``gumbel_u24``: the kernel's random words.
* ``reference_nucleus`` / ``expected_token`` / ``gumbel_reference``: float64 on the exact fp32
  (or upcast bf16) logit values.
* ``DELTA`` = 2^-12 bounds what the kernel's fp32 arithmetic can move a CDF boundary (2048
  non-negative fp32 terms: 2^-13 relative; a few ulp on an ``exp`` argument of magnitude <= 64:
  2^-17). It is never a tolerance on an answer: it chooses inputs. Every witness draws with a
  seed whose ``u * cdf[c-1]`` lies at least DELTA (relative) inside its token's interval and
  cuts with a ``top_p`` at least DELTA away from every CDF boundary, so one token is correct.
  Two kinds of row are exempt because their fp32 sums are exact (equal maxima, weight 1 each):
  the 3000-tie row and the cut that lands exactly on a boundary. At ``top_p = 1`` the cut keeps
  everything in exact arithmetic; fp32 may drop a tail lighter than 2^-13 of the mass, which
  the seed's margin covers.
* ``model_token`` / ``model_gumbel``: the kernel's steps in fp32 numpy with mutation switches
  (tests/test_sampling_witness.py proves that each mutation changes a witness token).
* ``*_cases()``: the witness sets shared by the CPU proof and the GPU module.
"""
import functools
from dataclasses import dataclass

import numpy as np
import torch

MASK = np.uint64(0xFFFFFFFF)
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
CAP = 2048                      # SMP_CAP: most survivors of the top-k stage
CAPC = 64                       # SMP_CAPC: candidate slots per chunk, largest two-phase top-k
CHUNK_MAX = 4096                # SMP_CHUNK_MAX
DELTA = 2.0 ** -12
GUMBEL_LEAD = 2.0 ** -10        # smallest float64 lead of a flat row's winner (see flat cases)
DRAW_CTR = (0x0FFFFFFF, 1, 0xA5A5A5A5, 7)
GUMBEL_CTR = (0, 0x5A5A5A5A, 0)  # (y, z, w); x = token >> 2
BG = -30.0                      # background logit of the planted rows
LADDER_STEP = 0.25              # ladder values -j/4: exact in bf16 up to j = 64
F32 = np.float32


# ------------------------------------------------------------------------------- Philox
def philox4x32_10(key_lo, key_hi, ctr):
    """Philox4x32-10, vectorised (numpy broadcasting over keys and counters). ``ctr`` is four
    words (x, y, z, w); returns the four output words as uint32 arrays."""
    k0 = np.asarray(key_lo, dtype=np.uint64) & MASK
    k1 = np.asarray(key_hi, dtype=np.uint64) & MASK
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in ctr)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, \
            (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return tuple(np.asarray(c).astype(np.uint32) for c in (c0, c1, c2, c3))


def seed_key(seed, ignore_high=False):
    """(low, high) 32-bit words of int64 seeds taken as unsigned."""
    s = np.asarray(seed, dtype=np.int64).view(np.uint64)
    hi = s >> np.uint64(32)
    return s & MASK, (hi * np.uint64(0) if ignore_high else hi)


def draw_u24(seed, word=0, ignore_high=False):
    """The 24-bit integer behind the inverse-CDF uniform of each seed."""
    lo, hi = seed_key(seed, ignore_high)
    return philox4x32_10(lo, hi, DRAW_CTR)[word] >> np.uint32(8)


def gumbel_u24(seed, V, counter_is_token=False, word_shift=0, one_word=False):
    """The 24-bit integers behind the Gumbel uniforms of tokens 0..V-1 for one seed. The
    switches are the mutations of the model: counter ``i`` instead of ``i >> 2``, word
    ``(i + word_shift) & 3``, and word x for all four tokens of a counter."""
    lo, hi = seed_key(np.int64(seed))
    i = np.arange(V, dtype=np.int64)
    ctr = i if counter_is_token else i >> 2
    uniq, inv = np.unique(ctr, return_inverse=True)
    y, z, w = GUMBEL_CTR
    words = np.stack(philox4x32_10(lo, hi, (uniq, y, z, w)), axis=1)        # [n, 4]
    sel = np.zeros(V, dtype=np.int64) if one_word else (i + word_shift) & 3
    return words[inv, sel] >> np.uint32(8)


def u_exact(u24):
    """The uniform as the contract states it: (u24 + 0.5) / 2^24, in float64."""
    return (np.asarray(u24, dtype=np.float64) + 0.5) / 16777216.0


def u_fp32(u24):
    """The uniform as fp32 computes it: u24 + 0.5 rounds to even from 2^23 up, and the
    largest value is held strictly below 1 (sampling.hip u01)."""
    u = (np.asarray(u24).astype(F32) + F32(0.5)) * F32(1.0 / 16777216.0)
    return np.minimum(u, F32(1.0 - 2.0 ** -24))


SEED_POOL_BITS = 20


@functools.lru_cache(maxsize=None)
def seed_pool():
    """2^20 full-range int64 seeds (high word non-zero, sign bit set in half) with their
    draw uniforms."""
    rng = np.random.default_rng(20240611)
    seeds = rng.integers(-2 ** 63, 2 ** 63 - 1, size=1 << SEED_POOL_BITS, dtype=np.int64)
    seeds = seeds[(seeds.view(np.uint64) >> np.uint64(32)) != 0]
    return seeds, u_exact(draw_u24(seeds))


# --------------------------------------------------------------------------- the reference
@dataclass
class Nucleus:
    ids: np.ndarray            # the m survivors of the top-k stage, (value desc, id asc)
    cdf: np.ndarray            # float64 cumulative weights over ids
    c: int                     # tokens kept by top-p
    slack: float               # distance of P*Z to the nearest CDF boundary, over Z


_order_cache = {}


def _order(row, desc_ids=False, cache=True):
    """Token ids by (value descending, id ascending) (or id descending: a mutation)."""
    key = (id(row), desc_ids)
    hit = _order_cache.get(key)
    if hit is None or hit[0] is not row:
        ids = np.arange(row.size)
        hit = (row, np.lexsort((-ids if desc_ids else ids, -row.astype(np.float64))))
        if cache:
            _order_cache[key] = hit
    return hit[1]


def keff_of(K, V):
    return min(CAP if (K <= 0 or K > CAP) else K, V)


def _survivors(row, K, order, keep_ties=True):
    """How many entries of ``order`` survive top-k: ties with the Keff-th value are kept, as
    HF does; past 2048 the lowest-id ties are (``order`` already lists them first)."""
    keff = keff_of(K, row.size)
    if not keep_ties:
        return keff
    kth = row[order[keff - 1]]
    m = int(np.searchsorted(-row[order].astype(np.float64), -np.float64(kth), side="right"))
    return min(m, CAP)


def reference_nucleus(row, T, K, P):
    """float64 nucleus of one fp32 row (bf16 logits: pass the upcast values)."""
    assert row.dtype == F32 and row.ndim == 1
    order = _order(row)
    m = _survivors(row, K, order)
    ids = order[:m]
    x = row[ids].astype(np.float64)
    cdf = np.cumsum(np.exp((x - x[0]) / np.float64(F32(T))))
    Z, lim = cdf[-1], np.float64(F32(P)) * cdf[-1]
    hit = np.nonzero(cdf[:m - 1] >= lim)[0]
    c = 1 + (int(hit[0]) if hit.size else m - 1)
    slack = float(np.min(np.abs(cdf[:m - 1] - lim)) / Z) if m > 1 else 1.0
    return Nucleus(ids, cdf, c, slack)


def token_of_u(nuc, u):
    """(index into nuc.ids, margin) of the draw for uniforms ``u`` (array or scalar)."""
    zk = nuc.cdf[nuc.c - 1]
    t = np.asarray(u, dtype=np.float64) * zk
    edges = nuc.cdf[:nuc.c - 1]
    j = np.searchsorted(edges, t, side="right")              # first j with cdf[j] > t
    if edges.size == 0:
        return j, np.ones_like(t)
    lo = np.where(j > 0, t - edges[np.maximum(j - 1, 0)], np.inf)
    hi = np.where(j < edges.size, edges[np.minimum(j, edges.size - 1)] - t, np.inf)
    return j, np.minimum(np.minimum(lo, hi) / zk, 1.0)


def expected_token(row, T, K, P, seed):
    """(token, margin) of one seeded draw. ``T <= 0`` or ``K == 1``: greedy, lowest id on
    ties, margin 1."""
    if T <= 0 or K == 1:
        return int(np.argmax(row)), 1.0
    nuc = reference_nucleus(row, T, K, P)
    j, margin = token_of_u(nuc, u_exact(draw_u24(np.int64(seed))))
    return int(nuc.ids[int(j)]), float(margin)


def midpoint_p(row, T, K, c):
    """The ``top_p`` (as fp32) in the middle of the interval that keeps exactly ``c`` tokens;
    raises unless its slack is at least DELTA."""
    nuc = reference_nucleus(row, T, K, 1.0)
    m = nuc.ids.size
    assert 1 <= c <= m, (c, m)
    lo = nuc.cdf[c - 2] if c >= 2 else 0.0
    hi = nuc.cdf[c - 1] if c < m else nuc.cdf[-1]
    P = float(F32((lo + hi) / 2 / nuc.cdf[-1]))
    got = reference_nucleus(row, T, K, P)
    if got.c != c or got.slack < DELTA:
        raise ValueError(f"no top_p with slack >= 2^-12 keeps {c} of {m} tokens")
    return P


# --------------------------------------------------------------------------- seed pickers
@functools.lru_cache(maxsize=None)
def _pool_by_u():
    seeds, u = seed_pool()
    o = np.argsort(u, kind="stable")
    return seeds[o], u[o]


def pick_seeds(nuc, target, count=1):
    """``count`` pool seeds whose draw lands at least DELTA inside a target interval of u:
    'first' (token 0), 'last' (the last nucleus token) or an int ``j`` (the interior of token
    j), spread evenly over the part of the interval that qualifies. Raises when the pool has
    fewer: no case shrinks silently."""
    seeds, u = _pool_by_u()
    j = {"first": 0, "last": nuc.c - 1}.get(target, target)
    zk = nuc.cdf[nuc.c - 1]
    lo = nuc.cdf[j - 1] / zk + DELTA if j > 0 else 0.0
    hi = nuc.cdf[j] / zk - DELTA if j < nuc.c - 1 else 1.0
    a, b = int(np.searchsorted(u, lo, side="left")), int(np.searchsorted(u, hi, side="right"))
    if b - a < count:
        raise ValueError(f"{max(b - a, 0)} seeds of the pool land in token {target!r} of "
                         f"{nuc.c} with margin 2^-12; {count} wanted")
    picks = [int(seeds[a + int((k + 0.5) * (b - a) / count)]) for k in range(count)]
    for s in picks:                                  # the picker's promise, checked
        jj, margin = token_of_u(nuc, u_exact(draw_u24(np.int64(s))))
        assert int(jj) == j and margin >= DELTA
    return picks


# --------------------------------------------------------------------------- Gumbel-max
def gumbel_reference(row, T, seed):
    """(token, lead): float64 Gumbel-max winner (lowest id on exact ties) and its lead over
    the best other token."""
    u = u_exact(gumbel_u24(seed, row.size))
    s = row.astype(np.float64) / np.float64(F32(T)) - np.log(-np.log(u))
    w = int(np.argmax(s))
    lead = float(s[w] - np.max(np.delete(s, w))) if row.size > 1 else np.inf
    return w, lead


def model_gumbel(row, T, seed, mut=None):
    """The kernel's Gumbel-max pass in fp32 numpy (numpy's log, not the device's)."""
    u24 = gumbel_u24(seed, row.size, counter_is_token=mut == "gumbel_counter_i",
                     word_shift=1 if mut == "gumbel_word_plus_1" else 0,
                     one_word=mut == "gumbel_one_word_for_four")
    g = -np.log(-np.log(u_fp32(u24)))
    invT = F32(1.0) if mut == "gumbel_no_inv_t" else F32(1.0) / F32(T)
    return int(np.argmax(row * invT + g.astype(F32)))


# ------------------------------------------------------------------------ the fp32 model
MUTATIONS = ("nucleus_short", "nucleus_long", "cut_gt", "topk_ties_dropped", "tie_order_desc",
             "u_word_y", "u_scaled_by_z", "high_seed_ignored", "gumbel_counter_i",
             "gumbel_word_plus_1", "gumbel_no_inv_t", "chunk_last_skipped",
             "overflow_keeps_highest")


def chunk_layout(B, V):
    """(chunks per row, chunk length) of the two-phase launch of a batch, or None when the
    batch samples in one phase (launch_sample)."""
    if B > 8:
        return None
    P = 1
    while P < 64 and (B * P < 256 or (V + P - 1) // P > CHUNK_MAX):
        P <<= 1
    L = (((V + P - 1) // P) + 3) & ~3
    return (P, L) if L <= CHUNK_MAX else None


def model_token(row, T, K, P, seed, mut=None, batch=1):
    """The kernel's contract, step by step in fp32 numpy, for seeds (array or scalar)."""
    seed = np.asarray(seed, dtype=np.int64)
    if T <= 0 or K == 1:
        return np.full(seed.shape, int(np.argmax(row)))
    cache = True
    if mut == "chunk_last_skipped" and 1 <= K <= CAPC and chunk_layout(batch, row.size):
        Pc, L = chunk_layout(batch, row.size)
        row, cache = row.copy(), False
        ends = np.minimum(np.arange(1, Pc + 1) * L, row.size) - 1
        row[ends[np.arange(Pc) * L < row.size]] = -np.inf
    order = _order(row, desc_ids=mut == "tie_order_desc", cache=cache)
    keff = keff_of(K, row.size)
    kth = row[order[keff - 1]]
    m_all = int(np.searchsorted(-row[order].astype(np.float64), -np.float64(kth), side="right"))
    m = keff if mut == "topk_ties_dropped" else min(m_all, CAP)
    ids = order[:m]
    if mut == "overflow_keeps_highest" and m_all > CAP:
        above = int(np.searchsorted(-row[order].astype(np.float64), -np.float64(kth)))
        ids = np.concatenate([order[:above], order[m_all - (CAP - above):m_all]])
    x = row[ids]
    w = np.exp((x - x[0]) * (F32(1.0) / F32(T)), dtype=F32)
    cdf = np.cumsum(w, dtype=F32)
    lim = F32(P) * cdf[-1]
    hit = np.nonzero((cdf[:m - 1] > lim) if mut == "cut_gt" else (cdf[:m - 1] >= lim))[0]
    c = 1 + (int(hit[0]) if hit.size else m - 1)
    c = max(1, c - 1) if mut == "nucleus_short" else min(m, c + 1) if mut == "nucleus_long" else c
    u = u_fp32(draw_u24(seed, word=1 if mut == "u_word_y" else 0,
                        ignore_high=mut == "high_seed_ignored"))
    t = u * (cdf[-1] if mut == "u_scaled_by_z" else cdf[c - 1])
    j = np.minimum(np.searchsorted(cdf[:c - 1], t, side="right"), c - 1)
    return ids[j]


# ------------------------------------------------------------------------------ the cases
@dataclass
class Case:
    name: str
    row: np.ndarray            # fp32 values (bf16 cases: exactly representable in bf16)
    dtype: str                 # 'f32' | 'bf16'
    T: float
    K: int
    P: float
    seed: int
    token: int
    gumbel: bool = False


def bf16_round(row):
    return torch.from_numpy(row).to(torch.bfloat16).float().numpy()


def _nucleus_cases(name, row, dtype, T, K, P, targets, per=1):
    nuc = reference_nucleus(row, T, K, P)
    if P < 1.0 and nuc.slack < DELTA:
        raise ValueError(f"{name}: top_p {P} has slack {nuc.slack:.3g} < 2^-12")
    out = []
    for tg in targets:
        for s in pick_seeds(nuc, tg, per):
            j = {"first": 0, "last": nuc.c - 1}.get(tg, tg)
            out.append(Case(f"{name} T{T} K{K} P{P:.6g} c{nuc.c} draw {tg}", row, dtype, T, K, P,
                            s, int(nuc.ids[j])))
    return out


def ladder_row(V, positions):
    """Background -30 with the ladder 0, -1/4, -2/4, ... planted at ``positions`` (rank j of
    the ladder at positions[j])."""
    row = np.full(V, BG, dtype=F32)
    row[np.asarray(positions)] = -LADDER_STEP * np.arange(len(positions), dtype=F32)
    return row


def chunk_boundary_positions(V, limit=64):
    """Both sides of the first, middle and last chunk boundary of every power-of-two chunk
    count <= 64 whose chunk length is <= 4096, plus the row's first and last element."""
    pos = [0, V - 1]
    for p in (1, 2, 4, 8, 16, 32, 64):
        L = (((V + p - 1) // p) + 3) & ~3
        if L > CHUNK_MAX:
            continue
        last = (V - 1) // L
        for c in sorted({1, p // 2, last}):
            if 1 <= c and c * L < V:
                pos += [c * L - 1, c * L]
    pos = list(dict.fromkeys(pos))
    rng = np.random.default_rng(V)
    rng.shuffle(pos)                                  # value order is not id order
    return pos[:limit]


def slice_positions(V, t, count, width):
    """``count`` ids of thread t's slice of the vectorised row scan ((id // width) % 512 == t;
    width 4 for fp32, 8 for bf16), one per trip of the scan, lanes varied."""
    pos = [width * (t + 512 * r) + r % width for r in range(count)]
    assert pos[-1] < V
    return pos


LADDER_TS = (0.25, 0.8, 1.0, 1.7)


def _ladder_set(name, V, positions, dtype, K=None, Ts=LADDER_TS, all_tokens=True):
    """One ladder through its draws: at P = 1 the first token, the last and every token of
    probability >= 2^-8; with the top_p that keeps c in {1, 2, n-1, n} the first and last."""
    n = len(positions)
    row = ladder_row(V, positions)
    K = n if K is None else K
    out = []
    for T in Ts:
        nuc = reference_nucleus(row, T, K, 1.0)
        p = np.diff(nuc.cdf, prepend=0.0) / nuc.cdf[-1]
        heavy = [j for j in range(n) if p[j] >= 2.0 ** -8]
        targets = ["first", "last"] if p[nuc.c - 1] >= 2 * DELTA else ["first"]
        if all_tokens:
            targets += [j for j in heavy if 0 < j < nuc.c - 1]
        if K > 0:                                     # K <= 0 with P = 1 is the Gumbel path
            out += _nucleus_cases(name, row, dtype, T, K, 1.0, targets)
        for c in sorted({1, 2, n - 1, n}):
            if not 1 <= c <= n:
                continue
            try:
                P = midpoint_p(row, T, K, c)
            except ValueError:
                continue                  # this T leaves token c too light to cut at; the
                # other temperatures cut there (test_sampling_witness counts the cuts)
            out += _nucleus_cases(name, row, dtype, T, K, P, ["first", "last"])
    return out


@functools.lru_cache(maxsize=None)
def ladder_cases():
    out = []
    for dtype, width in (("f32", 4), ("bf16", 8)):
        # chunk boundaries: every chunk count a batch can get
        for V in (1000, 128256):
            pos = chunk_boundary_positions(V)
            out += _ladder_set(f"ladder chunk-edges V{V}", V, pos, dtype)
            # K = 0: the whole-row paths see the same ladder
            out += _ladder_set(f"ladder chunk-edges K0 V{V}", V, pos, dtype, K=0, Ts=(0.8,),
                               all_tokens=False)
        for n in (2, 5):
            out += _ladder_set(f"ladder ends n{n}", 4097, [4096, 0, 2048, 1, 4095][:n], dtype)
        # n = 64: both sides of the first 32 boundaries of the 36-element chunks of V = 2049
        pos = [c * 36 - e for c in range(1, 33) for e in (1, 0)]
        np.random.default_rng(64).shuffle(pos)
        out += _ladder_set("ladder n64", 2049, pos, dtype)
        # 7, 8 and 9 of the top-12 in one thread's slice of the vectorised scan: with 7 the
        # register top-8 proves itself complete, from 8 on it cannot and the radix select runs
        V = 40960
        for own in (7, 8, 9):
            pos = slice_positions(V, 37, own, width) + [5, 20001, 30002, 40959, 12288][:12 - own]
            out += _ladder_set(f"ladder slice t37 x{own}", V, pos, dtype, Ts=(0.8, 1.7))
        # tau0 comes from the first quarter of the row: all large values outside it / inside it
        V = 50257
        rng = np.random.default_rng(7)
        late = (V // 4 + 16 + rng.choice(V - V // 4 - 16, 16, replace=False)).tolist()
        early = rng.choice(V // 4 - 16, 16, replace=False).tolist()
        out += _ladder_set("ladder late", V, late, dtype, Ts=(0.8, 1.7))
        out += _ladder_set("ladder early", V, early, dtype, Ts=(0.8, 1.7))
    return out


VOCABS = (1, 3, 64, 511, 513, 1000, 2049, 4097, 50257, 151936, 262144, 262145)


@functools.lru_cache(maxsize=None)
def vocab_cases():
    """Three sampled rows per vocabulary size and dtype, and one greedy row with tied maxima
    (the lowest id wins; one of the maxima is the row's last element)."""
    out = []
    for dtype in ("f32", "bf16"):
        for V in VOCABS:
            pos = list(dict.fromkeys([V - 1, 0, V // 2, V // 3, (2 * V) // 3, 1]))[:min(V, 6)]
            row = ladder_row(V, pos)
            n, T, K = len(pos), 0.8, 5
            kept = min(n, K)
            name = f"vocab V{V}"
            out += _nucleus_cases(name, row, dtype, T, K, 1.0, ["first", "last"] if kept > 1
                                  else ["first"])
            if kept > 2:
                out += _nucleus_cases(name, row, dtype, T, K, midpoint_p(row, T, K, kept - 1),
                                      [kept - 2])
            else:
                out += _nucleus_cases(name, row, dtype, T, K, 1.0, ["first"])
            g = np.full(V, BG, dtype=F32)
            g[[V - 1, V // 2]] = 1.0
            out.append(Case(f"vocab V{V} greedy", g, dtype, 0.0, 1, 1.0, 5, int(np.argmax(g))))
            out.append(Case(f"vocab V{V} greedy by top_k 1", g, dtype, 0.8, 1, 0.5, 5,
                            int(np.argmax(g))))
    return out


TOPKS = (2, 5, 50, 64, 65, 256, 257)
TOPKS_WIDE = (2048, 3000, 0)        # 0 with top_p < 1


def slope_row(V, step, head, seed):
    """Distinct values -rank*step at shuffled positions; ``head`` adds four heavy tokens."""
    rank = np.random.default_rng(seed).permutation(V)
    row = (-step * rank).astype(F32)
    if head:
        for j in range(4):
            row[rank == j] = 8.0 - 0.5 * j
    return row


@functools.lru_cache(maxsize=None)
def topk_cases():
    """V = 4097 (two-phase chunks of 68 elements). K <= 257: a gentle slope, so that token K
    is nearly as likely as token 1 and token K+1 would be too; the last-token seed sees the
    top-k boundary to one token. K in {2048, 3000, 0}: no token of a 2048-token nucleus can be
    more likely than 2^-11 = 2 DELTA unless a few are heavy, so these rows have a four-token
    head over a slope that stays heavy past rank 3000 (weights e^-1 at rank 2048): 2048
    survivors against 3000 moves the head's boundaries by 6 % of the mass. They see the clamp
    and the full-row fallback of the two-phase launch, not one token more or less."""
    out, V = [], 4097
    for dtype in ("f32", "bf16"):
        gentle = slope_row(V, 1.0 / 256, False, 11)
        wide = slope_row(V, 1.0 / 2048, True, 12)
        if dtype == "bf16":
            gentle, wide = bf16_round(gentle), bf16_round(wide)
        for K in TOPKS:
            nuc = reference_nucleus(gentle, 1.0, K, 1.0)
            out += _nucleus_cases("topk slope", gentle, dtype, 1.0, K, 1.0,
                                  ["first", "last", nuc.c // 2])
        for K in TOPKS_WIDE:
            P = 1.0 if K else midpoint_p(wide, 1.0, K, 3)
            out += _nucleus_cases("topk head+slope", wide, dtype, 1.0, K, P,
                                  ["first", 1, 2] + ([3] if K else []))
    return out


TIE_V, TIE_K = 128256, 10


def tie_row(t):
    """Ranks 1..K-1 a ladder, ranks K..K+t equal (the K-th value and t ties). t = 1: two ties
    far apart; t = 70: 71 ties inside one chunk of either two-phase layout (more than the 64
    candidate slots: the chunk raises the row's overflow flag); t = 600: every seventh id,
    more than the fast path's 512 slots."""
    ids = {1: [9000, 100000], 70: list(range(8100, 8171)),
           600: list(range(20000, 20000 + 7 * 601, 7))}[t]
    row = ladder_row(TIE_V, [70000, 3, 128255, 64000, 2004, 4007, 4008, 2003, 99999])
    row[ids] = -2.5
    return row, ids


def many_maxima_row():
    """3000 equal maxima among 4097: the 2048 lowest-id ties survive with weight 1 each."""
    ids = np.sort(np.random.default_rng(5).choice(4097, 3000, replace=False))
    row = np.full(4097, BG, dtype=F32)
    row[ids] = 2.0
    return row, ids


@functools.lru_cache(maxsize=None)
def tie_cases():
    out = []
    for dtype in ("f32", "bf16"):
        for t in (1, 70, 600):
            row, ids = tie_row(t)
            nuc = reference_nucleus(row, 1.0, TIE_K, 1.0)
            assert nuc.c == TIE_K + t and nuc.ids[-1] == ids[-1]
            # the last-token seed returns the highest-id tie; interior ties in id order
            out += _nucleus_cases(f"ties t{t}", row, dtype, 1.0, TIE_K, 1.0,
                                  ["first", "last", TIE_K - 1, TIE_K + t // 2])
            # the largest uniform of the pool: still the highest-id tie, no token beyond it
            out.append(Case(f"ties t{t} largest u", row, dtype, 1.0, TIE_K, 1.0,
                            int(_pool_by_u()[0][-1]), int(ids[-1])))
        # 3000 equal maxima, K = 0, P = 0.9: sums exact in fp32, c = 1844 in closed form
        row, ids = many_maxima_row()
        nuc = reference_nucleus(row, 1.0, 0, 0.9)
        seeds, u = seed_pool()
        frac = np.modf(u * nuc.c)[0]
        ok = np.nonzero((frac >= 0.1) & (frac <= 0.9))[0]
        for i in list(ok[:6]) + [ok[np.argmax(u[ok])], ok[np.argmin(u[ok])]]:
            out.append(Case("ties 3000 maxima", row, dtype, 1.0, 0, 0.9, int(seeds[i]),
                            int(ids[int(u[i] * nuc.c)])))
        # a cut that lands exactly on a boundary: four equal maxima, P = 0.5 keeps two (HF
        # removes the ascending cumulative mass <= 1 - P); weights 1, sums exact
        row = np.full(513, BG, dtype=F32)
        row[[500, 7, 300, 64]] = 1.0
        for lo, hi, tok in ((0.05, 0.3, 7), (0.7, 0.95, 64)):
            i = int(np.nonzero((u >= lo) & (u <= hi))[0][0])
            out.append(Case("ties exact cut", row, dtype, 1.0, 4, 0.5, int(seeds[i]), tok))
    return out


RANDOM_V = 128256


@functools.lru_cache(maxsize=None)
def random_cases(count=20):
    base = (np.random.default_rng(3).standard_normal(RANDOM_V) * 3).astype(F32)
    out = []
    for dtype in ("f32", "bf16"):
        row = bf16_round(base) if dtype == "bf16" else base
        for T, K, c in ((0.8, 50, None), (0.25, 2048, 0)):
            nuc = reference_nucleus(row, T, K, 1.0)
            if c is None:
                # the cut nearest 0.95 whose slack is DELTA
                want = int(np.searchsorted(nuc.cdf, 0.95 * nuc.cdf[-1])) + 1
                for c in range(want, 1, -1):
                    try:
                        P = midpoint_p(row, T, K, c)
                        break
                    except ValueError:
                        continue
                else:
                    raise ValueError("no cut of the random row has slack 2^-12")
            else:
                P = 1.0
            nuc = reference_nucleus(row, T, K, P)
            seeds, u = seed_pool()
            j, margin = token_of_u(nuc, u[:4096])
            ok = np.nonzero(margin >= DELTA)[0]
            if ok.size < count:
                raise ValueError("too few seeds with margin 2^-12 on the random row")
            for i in ok[:count]:
                out.append(Case(f"random T{T} K{K} P{P:.6g}", row, dtype, T, K, P, int(seeds[i]),
                                int(nuc.ids[j[i]])))
    return out


GUMBEL_VS = (1, 3, 5, 511, 2049, 50257, 128256)


def _seq_seeds(start):
    seeds, _ = seed_pool()
    return seeds[start:]


@functools.lru_cache(maxsize=None)
def gumbel_flat_cases():
    """All logits one constant: the token is the id of the largest Gumbel uniform. Seeds whose
    float64 winner leads by 2^-10: fp32 rounds u24 + 0.5 to even from 2^23 up, so two
    uniforms one apart can collapse, and a lead in the score survives any monotone log.
    At V = 128256 one seed's two largest uniforms are equal: the lower id wins."""
    out = []
    for dtype in ("f32", "bf16"):
        for V in GUMBEL_VS:
            for ci, const in enumerate((0.0, 1.5)):
                row = np.full(V, const, dtype=F32)
                for ti, T in enumerate((0.5, 1.3)):
                    for s in _seq_seeds(100 * ci + 10 * ti):
                        tok, lead = gumbel_reference(row, T, s)
                        if lead >= GUMBEL_LEAD:
                            assert tok == int(np.argmax(gumbel_u24(s, V)))
                            out.append(Case(f"gumbel flat {const} V{V}", row, dtype, T, 0, 1.0,
                                            int(s), tok, True))
                            break
        s, tok = gumbel_tie_seed()
        out.append(Case("gumbel flat tie of the two largest", np.zeros(128256, dtype=F32), dtype,
                        1.3, 0, 1.0, s, tok, True))
    return out


@functools.lru_cache(maxsize=None)
def gumbel_tie_seed(V=128256, batch=32, limit=4096):
    """A seed whose two largest Gumbel uniforms over V tokens are equal (about one in 200)."""
    seeds = _seq_seeds(0)
    i = np.arange(V, dtype=np.int64)
    y, z, w = GUMBEL_CTR
    for b in range(0, limit, batch):
        lo, hi = seed_key(seeds[b:b + batch])
        words = np.stack(philox4x32_10(lo[:, None], hi[:, None], ((i[::4] >> 2)[None], y, z, w)),
                         axis=2).reshape(batch, -1)[:, :V] >> np.uint32(8)
        top = np.partition(words, V - 2, axis=1)[:, V - 2:]
        for r in np.nonzero(top[:, 0] == top[:, 1])[0]:
            return int(seeds[b + r]), int(np.argmax(words[r]))
    raise ValueError("no seed with tied largest uniforms")


def step_row(V, kind, delta=2.0):
    row = np.zeros(V, dtype=F32)
    ids = {"last37": np.arange(V - 37, V), "mod4": np.arange(3, V, 4),
           "one": np.array([V // 3])}[kind]
    row[ids] = delta
    return row


@functools.lru_cache(maxsize=None)
def gumbel_step_cases(per=8):
    """Logits 0 except a set at +2, T = 0.5. Seeds whose float64 winner leads by 0.25 (no
    plausible error of the device's fast log flips it); for half of them the winner changes
    when 1/T is dropped."""
    out = []
    for dtype in ("f32", "bf16"):
        for V, kind in ((50257, "last37"), (2049, "mod4"), (511, "one")):
            row = step_row(V, kind)
            need = {True: per // 2, False: per - per // 2}
            for s in _seq_seeds(1000):
                tok, lead = gumbel_reference(row, 0.5, s)
                if lead < 0.25:
                    continue
                flips = model_gumbel(row, 0.5, s, "gumbel_no_inv_t") != tok
                if need[flips]:
                    need[flips] -= 1
                    out.append(Case(f"gumbel step {kind} V{V}" + (" 1/T decides" if flips else ""),
                                    row, dtype, 0.5, 0, 1.0, int(s), tok, True))
                if not any(need.values()):
                    break
            else:
                raise ValueError("too few step-row seeds")
    return out


# Seeds with u24 = 0xffffff at one token of a 64-token row: (u24 + 0.5) / 2^24 rounds to 1.0 in
# fp32, and -log(-log(1)) is +inf. The token is at -30 among zeros: it must not win.
GUMBEL_TOP_SEEDS = (
    (2945977501869445036, 0), (318595042952628885, 4), (6959919387218972865, 8),
    (-4525230790288236565, 9), (-605342332899123875, 31), (999893694039577824, 32),
    (4726336293156452325, 33), (2746579985640447545, 33), (-1074412546654309172, 38),
    (2652320785186633795, 42), (6365820823252139940, 45), (-1148071821738823977, 51),
    (-5740469939265490305, 51), (4381674027693174566, 54), (-7646471755233201860, 62))


def gumbel_top_word_cases():
    out = []
    for s, tok in GUMBEL_TOP_SEEDS:
        row = np.zeros(64, dtype=F32)
        row[tok] = BG
        win, lead = gumbel_reference(row, 1.0, s)
        if lead < 0.25:                    # the other 63 tokens must not be a close call
            continue
        for dtype in ("f32", "bf16"):
            out.append(Case(f"gumbel largest uniform at -30 token {tok}", row, dtype, 1.0, 0, 1.0,
                            s, win, True))
    if len(out) < 12:
        raise ValueError("too few seeds whose largest uniform falls on the -30 token")
    return out


def expected(case):
    """The float64 reference's token for a case (what Case.token was built from)."""
    if case.gumbel:
        return gumbel_reference(case.row, case.T, case.seed)[0]
    return expected_token(case.row, case.T, case.K, case.P, case.seed)[0]


def model(case, mut=None, batch=1):
    if case.gumbel:
        return model_gumbel(case.row, case.T, case.seed, mut)
    return int(model_token(case.row, case.T, case.K, case.P, case.seed, mut, batch))
