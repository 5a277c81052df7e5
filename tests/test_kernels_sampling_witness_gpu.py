"""The sampler (csrc/kernels/sampling.hip) against the witnesses of tests/sampling_witness.py:
every case has exactly one correct token, computed on the CPU in float64 from the Philox word
the kernel will draw (tests/test_sampling_witness.py proves that each plausible error of the
kernel changes one of these tokens). Nothing is compared within a tolerance.

Every case runs through ``ops.sample`` in batches of 8 (two phases where the parameters
allow), of 9 (one phase) and alone, and through ``dli_sample`` with a null workspace (the
one-phase form of a small batch), as fp32 logits and as bf16 logits (the reference is given
the upcast values). Which witness sees which path of the kernel:

  greedy                       vocab cases "greedy" (T = 0 and top_k = 1, tied maxima)
  Gumbel-max                   gumbel flat / step / largest-uniform cases, batch invariance
  register top-8 fast path     ladders (K <= 256; slice x7 keeps it), vocab, topk K <= 256,
                               and every two-phase case (the candidate list goes through it)
  radix-select fallback        ladder slice x8 and x9, topk K in {257, 2048, 3000, 0},
                               random rows at K = 2048
  more than 512 ties           ties t600
  more than 2048 ties          ties 3000 maxima (and the bf16 topk rows, whose values tie)
  chunk overflow               ties t70 and t600 as batches of <= 8; flags zero afterwards
  K > 64 under two phases      topk K in {65, 256, 257, 2048, 3000, 0} in batches of 8
  chunk edges of two phases    ladder chunk-edges (V = 1000: 64 chunks of 16; V = 128256: 64
                               chunks of 2004 and 32 of 4008), vocab 262144 (chunks of 4096)
                               and 262145 (one phase)

(The file name sorts this module after test_bench_contract.py on purpose: a GPU module that
sorts before it initialises the GPU in a single-process run of the suite ahead of
test_spawn_failure_ends_the_job, whose launcher refuses a parent that has done so.)"""
import collections

import numpy as np
import pytest
import torch

import sampling_witness as W
from distributed_llm_inferencing_amd import ops

pytestmark = pytest.mark.gpu
TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16}


def _device_rows(cases, gpu):
    rows = torch.from_numpy(np.stack([c.row for c in cases]))
    dev = rows.to(TORCH_DTYPE[cases[0].dtype])
    assert torch.equal(dev.float(), rows)             # the reference saw the device's values
    return dev.to(gpu)


def _params(cases, gpu):
    return (torch.tensor([c.T for c in cases], dtype=torch.float32, device=gpu),
            torch.tensor([c.K for c in cases], dtype=torch.int32, device=gpu),
            torch.tensor([c.P for c in cases], dtype=torch.float32, device=gpu),
            torch.tensor([c.seed for c in cases], dtype=torch.int64, device=gpu))


def _one_phase(logits, temp, topk, topp, seeds):
    """dli_sample with a null workspace: one workgroup per row whatever the batch."""
    lib = ops.N.require_native()
    out = torch.empty(logits.shape[0], dtype=torch.int32, device=logits.device)
    fn = lib.dli_sample_bf16 if logits.dtype == torch.bfloat16 else lib.dli_sample
    assert fn(ops._p(out), ops._p(logits), logits.stride(0), logits.shape[0], logits.shape[1],
              ops._p(temp), ops._p(topk), ops._p(topp), ops._p(seeds), ops._p(None), ops._st()) == 0
    return out


def run_cases(cases, gpu):
    """Every case at every batch form; returns the failures as text."""
    groups = collections.defaultdict(list)
    for c in cases:
        groups[(c.row.size, c.dtype)].append(c)
    bad = []
    for (V, dtype), cs in groups.items():
        logits = _device_rows(cs, gpu)
        par = _params(cs, gpu)
        want = torch.tensor([c.token for c in cs], dtype=torch.int32)
        n = len(cs)
        runs = [(f"ops.sample B={min(n, lo + b) - lo}", lo, min(n, lo + b), ops.sample)
                for b in (8, 9) for lo in range(0, n, b)]
        runs += [("ops.sample B=1", i, i + 1, ops.sample) for i in range(min(n, 3))]
        runs += [("one-phase dli_sample", lo, min(n, lo + 8), _one_phase)
                 for lo in range(0, n, 8)]
        got = [(what, lo, fn(logits[lo:hi], *(p[lo:hi] for p in par))) for what, lo, hi, fn in runs]
        torch.cuda.synchronize()
        for what, lo, tok in got:
            tok = tok.cpu()
            for r in (tok != want[lo:lo + tok.numel()]).nonzero().squeeze(-1).tolist():
                c = cs[lo + r]
                bad.append(f"{c.name} {dtype} V{V} seed {c.seed} [{what}, row {r}]: "
                           f"token {int(tok[r])}, reference {c.token}")
    return bad


def check(cases, gpu):
    assert cases
    bad = run_cases(cases, gpu)
    assert not bad, f"{len(bad)} draws differ from the float64 reference:\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_inverse_cdf_ladders(gpu, dtype):
    check([c for c in W.ladder_cases() if c.dtype == dtype], gpu)


def test_vocabulary_sizes_and_greedy(gpu):
    assert {c.row.size for c in W.vocab_cases()} == set(W.VOCABS)
    check(W.vocab_cases(), gpu)


def test_top_k_settings(gpu):
    assert {c.K for c in W.topk_cases()} == set(W.TOPKS + W.TOPKS_WIDE)
    check(W.topk_cases(), gpu)


def test_ties(gpu):
    """Ties with the K-th value are kept in id order (the last-token seed returns the highest
    id of the ties), more than 2048 keep the lowest ids, a cut exactly on a boundary follows
    HF, and the chunk overflow flags raised on the way are zero again afterwards."""
    check(W.tie_cases(), gpu)
    for V in (W.TIE_V, 4097, 513):
        ws = ops._sample_ws(gpu, 8, V)
        assert ws is not None and int(ws[:32].view(torch.int32).abs().sum()) == 0


def test_random_rows(gpu):
    check(W.random_cases(), gpu)


def test_gumbel_flat_rows(gpu):
    assert {c.row.size for c in W.gumbel_flat_cases()} == set(W.GUMBEL_VS)
    check(W.gumbel_flat_cases(), gpu)


def test_gumbel_step_rows(gpu):
    check(W.gumbel_step_cases(), gpu)


def test_gumbel_largest_uniform_is_finite_noise(gpu):
    """Seeds whose Philox word is 0xffffff for a token at -30 among zeros: (u24 + 0.5) / 2^24
    rounds to 1 in fp32, and -log(-log 1) = +inf would let that token win."""
    check(W.gumbel_top_word_cases(), gpu)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_batch_invariance(gpu, dtype):
    """The same (row, parameters, seed) gives the reference's token alone, as row 7 of 8, as
    row 8 of 9 and as row 300 of 512, among random rows with other parameters and seeds."""
    rnd = [c for c in W.random_cases() if c.dtype == dtype]
    flat = [c for c in W.gumbel_flat_cases() if c.dtype == dtype and c.row.size == W.RANDOM_V]
    picks = [rnd[0], rnd[-1], flat[0]]
    assert {c.K for c in picks} == {50, 2048, 0}
    V = W.RANDOM_V
    torch.manual_seed(17)
    filler = (torch.randn(512, V, device=gpu) * 3).to(TORCH_DTYPE[dtype])
    bad = []
    for B, r in ((1, 0), (8, 7), (9, 8), (512, 300)):
        for c in picks:
            logits = filler[:B].clone()
            logits[r] = _device_rows([c], gpu)[0]
            temp = torch.full((B,), 0.9, device=gpu)
            topk = torch.full((B,), 40, dtype=torch.int32, device=gpu)
            topp = torch.full((B,), 0.95, device=gpu)
            seeds = torch.arange(B, dtype=torch.int64, device=gpu) * 7919 - 5
            temp[r], topk[r], topp[r], seeds[r] = c.T, c.K, c.P, c.seed
            tok = int(ops.sample(logits, temp, topk, topp, seeds)[r])
            if tok != c.token:
                bad.append(f"{c.name} {dtype} as row {r} of {B}: token {tok}, reference {c.token}")
    assert not bad, "\n".join(bad)
