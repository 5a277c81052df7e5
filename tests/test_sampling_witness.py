"""The sampler witnesses (tests/sampling_witness.py) proved on the CPU: the Philox port
reproduces the Random123 known answers, the float64 nucleus agrees with the HF-semantics
reference ``R.topk_topp_filter``, the fp32 model of the kernel's contract returns every
witness's token, and each listed mutation of that model changes at least one token of the
witness set the GPU module runs for that path. The last tests record which mutations the
frequency checks of test_kernels_gpu.py accept."""
import numpy as np
import pytest
import torch

import sampling_witness as W
from distributed_llm_inferencing_amd.ops import reference as R

F32 = np.float32


def test_philox_known_answers():
    assert [int(w) for w in W.philox4x32_10(0, 0, (0, 0, 0, 0))] == \
        [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = 0xFFFFFFFF
    assert [int(w) for w in W.philox4x32_10(ones, ones, (ones,) * 4)] == \
        [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    # vectorised over seeds: the key is (low, high) of the int64 taken as unsigned
    seeds = np.array([-1, 0, -2 ** 63, 0x123456789], dtype=np.int64)
    lo, hi = W.seed_key(seeds)
    assert lo.tolist() == [ones, 0, 0, 0x23456789] and hi.tolist() == [ones, 0, 0x80000000, 1]
    assert int(W.philox4x32_10(lo, hi, (ones,) * 4)[0][0]) == 0x408F276D


def test_uniform_pool():
    seeds, u = W.seed_pool()
    assert seeds.size > 0.99 * 2 ** 20
    assert abs(u.mean() - 0.5) < 0.002
    assert (seeds < 0).mean() > 0.4 and ((seeds.view(np.uint64) >> np.uint64(32)) != 0).all()
    assert 0 < u.min() and u.max() < 1
    # word x of the fixed draw counter, shifted right by 8
    lo, hi = W.seed_key(seeds[:4])
    assert (W.draw_u24(seeds[:4]) == W.philox4x32_10(lo, hi, (0x0FFFFFFF, 1, 0xA5A5A5A5, 7))[0]
            >> np.uint32(8)).all()


def test_gumbel_words_follow_the_counter_layout():
    s = int(W.seed_pool()[0][3])
    lo, hi = W.seed_key(np.int64(s))
    u = W.gumbel_u24(s, 11)
    for i in range(11):
        assert int(u[i]) == int(W.philox4x32_10(lo, hi, (i >> 2, 0, 0x5A5A5A5A, 0))[i & 3]) >> 8


def test_fp32_uniform_stays_below_one():
    """u24 + 0.5 needs 25 bits from 2^23 up: fp32 rounds it to even, and 0xffffff + 0.5 to
    2^24, a uniform of exactly 1 whose Gumbel noise -log(-log(1)) is +inf. The kernel holds the
    uniform at 1 - 2^-24; the seeds of W.GUMBEL_TOP_SEEDS draw that word for a -30 token."""
    top = F32(0xFFFFFF)
    assert (top + F32(0.5)) * F32(2.0 ** -24) == F32(1.0)
    assert W.u_fp32(np.uint32(0xFFFFFF)) == F32(1.0 - 2.0 ** -24)
    assert W.u_fp32(np.uint32(0xFFFFFD)) == W.u_fp32(np.uint32(0xFFFFFE))   # collapse to even
    cases = W.gumbel_top_word_cases()
    assert len(cases) >= 12
    for c in cases:
        tok = int(np.argmin(c.row))
        assert int(W.gumbel_u24(c.seed, 64)[tok]) == 0xFFFFFF == int(W.gumbel_u24(c.seed, 64).max())
        assert c.row[tok] == W.BG and c.token != tok
        assert W.gumbel_reference(c.row, c.T, c.seed)[1] >= 0.25   # not a close call
        assert W.model(c) == c.token


def test_reference_support_is_the_hf_support():
    """A cut falls within DELTA of a CDF boundary with probability about 2 DELTA / (mass of
    the tokens at the cut), so the rows cut where tokens still weigh a few percent (top_p <=
    0.8): a cut at 0.95 of 50 tokens, where they weigh 0.5 %, excludes one row in ten."""
    rng = np.random.default_rng(0)
    tried = excluded = 0
    for V, K, P in [(1000, 50, 0.7), (50257, 20, 0.8), (4097, 64, 0.6), (513, 5, 0.5),
                    (2049, 257, 0.5), (300, 3000, 0.7), (4097, 0, 0.6)]:
        for _ in range(40):
            row = (rng.standard_normal(V) * 3).astype(F32)
            tried += 1
            nuc = W.reference_nucleus(row, 0.8, K, P)
            if nuc.slack < W.DELTA:
                excluded += 1
                continue
            t = torch.from_numpy(row)[None]
            filt = R.topk_topp_filter(t, torch.tensor([0.8]), torch.tensor([K]),
                                      torch.tensor([P]))[0]
            assert set(nuc.ids[:nuc.c].tolist()) == \
                set(torch.isfinite(filt).nonzero().squeeze(-1).tolist()), (V, K, P)
    assert excluded < 0.05 * tried, (excluded, tried)


def test_closed_forms_of_the_tie_rows():
    row, ids = W.many_maxima_row()
    nuc = W.reference_nucleus(row, 1.0, 0, 0.9)
    assert nuc.ids.tolist() == ids[:2048].tolist()                 # the lowest-id ties
    assert nuc.c == int(np.ceil(float(F32(0.9)) * 2048)) == 1844
    row = np.full(513, W.BG, dtype=F32)
    row[[500, 7, 300, 64]] = 1.0
    nuc = W.reference_nucleus(row, 1.0, 4, 0.5)
    assert nuc.ids.tolist() == [7, 64, 300, 500] and nuc.c == 2    # HF keeps two of four


SETS = {
    "ladder": W.ladder_cases, "vocab": W.vocab_cases, "topk": W.topk_cases,
    "ties": W.tie_cases, "random": W.random_cases, "gumbel_flat": W.gumbel_flat_cases,
    "gumbel_step": W.gumbel_step_cases, "gumbel_top": W.gumbel_top_word_cases,
}


@pytest.mark.parametrize("name", list(SETS))
def test_model_returns_every_witness_token(name):
    """The cases are consistent (the float64 token is the recorded one) and the unmutated fp32
    model of the kernel's contract returns it, as a one- and a two-phase batch."""
    cases = SETS[name]()
    assert cases
    bad = [c.name for c in cases if W.model(c) != c.token or W.model(c, batch=9) != c.token]
    assert not bad, bad[:10]
    for c in cases[::7]:
        assert W.expected(c) == c.token, c.name
        if not c.gumbel and c.T > 0 and c.K != 1:
            assert W.expected_token(c.row, c.T, c.K, c.P, c.seed)[1] >= W.DELTA or \
                c.name.startswith(("ties 3000", "ties exact"))


def test_ladder_set_covers_what_it_promises():
    cases = W.ladder_cases()
    cuts = {(c.name.split(" T")[0], int(c.name.split(" draw")[0].rsplit(" c", 1)[1]))
            for c in cases}
    for dtype in ("f32", "bf16"):
        for V in (1000, 128256):
            n = len(W.chunk_boundary_positions(V))
            for c in (1, 2, n - 1, n):
                assert (f"ladder chunk-edges V{V}", c) in cuts
    assert {c.T for c in cases} == set(W.LADDER_TS)
    # both sides of a boundary of every chunk count that fits are planted
    for V in (1000, 128256):
        pos = set(W.chunk_boundary_positions(V))
        assert {0, V - 1} <= pos
        for p in (1, 2, 4, 8, 16, 32, 64):
            L = (((V + p - 1) // p) + 3) & ~3
            if L <= W.CHUNK_MAX and p > 1:
                assert any(e % L == L - 1 and e + 1 in pos for e in pos), (V, p)
    assert W.chunk_layout(8, 262144) == (64, 4096) and W.chunk_layout(1, 262145) is None
    assert W.chunk_layout(8, 128256) == (32, 4008) and W.chunk_layout(9, 1000) is None


MUTATION_SETS = {
    "nucleus_short": ["ladder"], "nucleus_long": ["ladder"], "cut_gt": ["ties"],
    "topk_ties_dropped": ["ties"], "tie_order_desc": ["ties"], "u_word_y": ["ladder", "random"],
    "u_scaled_by_z": ["ladder"], "high_seed_ignored": ["ladder", "random"],
    "gumbel_counter_i": ["gumbel_flat"], "gumbel_word_plus_1": ["gumbel_flat"],
    "gumbel_no_inv_t": ["gumbel_step"], "chunk_last_skipped": ["ladder"],
    "overflow_keeps_highest": ["ties"],
}


@pytest.mark.parametrize("mut", W.MUTATIONS)
def test_every_mutation_changes_a_witness_token(mut):
    assert set(MUTATION_SETS) == set(W.MUTATIONS)
    for name in MUTATION_SETS[mut]:
        cases = SETS[name]()
        if mut == "chunk_last_skipped":      # only rows with a planted chunk edge can see it
            cases = [c for c in cases if "chunk-edges" in c.name and c.K > 0]
        changed = sum(W.model(c, mut, batch=8) != c.token or W.model(c, mut, batch=1) != c.token
                      for c in cases)
        assert changed >= 1, (mut, name)


def _frequencies(tokens, V):
    return np.bincount(tokens, minlength=V) / tokens.size


OLD_ACCEPTS = ("u_word_y", "high_seed_ignored")


def test_what_the_old_distribution_check_accepts():
    """test_sampling_distribution_matches_reference's assertions (V = 64, 20000 rows, support
    and 0.02 on frequencies) evaluated on the model. They hold for the contract and for every
    error that keeps the distribution but gives a seed another token: the wrong Philox word,
    or a seed whose high word is ignored (the check's own seeds never set it, so two requests
    whose seeds differ only there would sample alike unnoticed). A nucleus one token short
    is seen at this shape only because the row's last nucleus token weighs 4 % (the error is
    that weight); a cut that drops a token under 2 % passes."""
    torch.manual_seed(6)
    V, B, T, K, P = 64, 20000, 0.8, 10, 0.9
    row = (torch.randn(V) * 2)
    seeds = np.arange(B, dtype=np.int64) * 104729 + 11
    p_ref = R.topk_topp_filter(row[None], torch.tensor([T]), torch.tensor([K]),
                               torch.tensor([P])).softmax(-1)[0].numpy()
    err = {}
    for mut in (None, "nucleus_short") + OLD_ACCEPTS:
        freq = _frequencies(W.model_token(row.numpy(), T, K, P, seeds, mut), V)
        assert (freq[p_ref == 0] == 0).all()
        err[mut] = float(np.abs(freq - p_ref).max())
    print("largest frequency error:", err)
    last = float(p_ref[p_ref > 0].min())
    assert err[None] < 0.02 and all(err[m] < 0.02 for m in ("u_word_y", "high_seed_ignored"))
    assert abs(err["nucleus_short"] - last) < 0.005 and last > 0.02


def test_what_the_old_gumbel_check_accepts():
    """test_sampling_pure_temperature_gumbel's assertion (V = 32, 20000 rows, 0.02 on
    frequencies) evaluated on the model: it holds for the contract and for a wrong counter or
    word layout, which only permute the stream. One Philox word shared by the four tokens of
    a counter is a distribution error (the largest logit of each four always wins, error
    0.14) and is rejected."""
    torch.manual_seed(7)
    V, B, T = 32, 20000, 1.3
    row = torch.randn(V)
    p = (row / T).softmax(-1).numpy()
    err = {}
    for mut in (None, "gumbel_counter_i", "gumbel_word_plus_1", "gumbel_one_word_for_four"):
        tok = np.array([W.model_gumbel(row.numpy(), T, s, mut) for s in range(B)])
        err[mut] = float(np.abs(_frequencies(tok, V) - p).max())
    print("largest frequency error:", err)
    assert max(err[None], err["gumbel_counter_i"], err["gumbel_word_plus_1"]) < 0.02
    assert err["gumbel_one_word_for_four"] > 0.02
