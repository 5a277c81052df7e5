#!/usr/bin/env python3
"""SHA-256 of the output bytes of the QKV post-processing, split-K reduce and decode attention
ops on seeded inputs, one JSON line per case, to compare two builds bit for bit (run it in
each tree on the same GPU, then diff the two files). The hashing and the roll-up are
scripts/gemm_digest.py's; the "tile" key of a line holds the op's name here.

Cases, at the sizes of the tests (tests/test_qwen_gpu.py, test_kernels_gpu.py):
  rope_and_cache        (32,8,128) (4,2,64) (7,1,128) heads, strided rows, a -1 slot, extras
                        none / norm / bias / both, rope on and off
  linear_rope_cache     1 / 2 / 3 / 4 / 8 splits, fp32 and fp16 slabs, the four extras modes
  linear_add_rmsnorm    N 512 / 2000 / 4096 / 8192, 2 / 3 / 4 / 8 splits, both slab formats,
                        with and without a norm weight; the fused gate (N 4096, E 8, k 2)
  moe_combine_slabs, moe_combine_add_rmsnorm    2 / 4 / 8 slabs
  decode_attention      pipelined, workgroup and wave forms, 1 / 2 / 4 KV splits, head dim 128
                        and 64, window 0 and 48, short contexts and two past a 64-block window
  linear_rope_attention decode_form 1 and 4, unsplit / 2 / 4 slabs, both formats, the four
                        extras modes, window 0 and 48

``--batch B`` runs the same cases at B rows / sequences (contexts of 33 to 100 tokens, 32 B
rows for rope_and_cache) instead of the tests' 7: a changed rounding that moves one element in
a million, such as the other fused form of a rotation, shows only at the size of a decode
batch (B = 512: bench.py's).

    python scripts/attn_digest.py --out attn_digest.jsonl [--rollup per_op.jsonl] [--batch 512]
    python scripts/attn_digest.py --from attn_digest.jsonl --rollup per_op.jsonl   # no GPU
"""
import argparse
import hashlib
import json
import math
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from gemm_digest import rnd, rollup, sha  # noqa: E402

from distributed_llm_inferencing_amd import ops  # noqa: E402
from distributed_llm_inferencing_amd.ops import gemm as G  # noqa: E402
from distributed_llm_inferencing_amd.ops import reference as R  # noqa: E402

MODES = ("none", "norm", "bias", "both")
K_IN = 1536                      # splits into 2, 3, 4 and 8 multiples of 64
BS = 16
LENS_SHORT = [1, 5, 33, 100, 200, 17, 130]
LENS_LONG = [700, 1025]          # 1025 tokens = 65 blocks: past one 64-block table window
WIN = 48
BATCH = 0                        # --batch: rows / sequences per case instead of the tests' 7


def tokens(gen, T, nblk):
    """(positions, slots) of T rows: the tests' literals, or with --batch positions below 128
    and distinct slots of an nblk-block cache, the third row without one."""
    if not BATCH:
        return i32([0, 3, 17, 4, 9, 100, 31]), i32([5, 0, -1, 11, 6, 33, 47])
    slots = torch.randperm(nblk * BS, generator=gen)[:T].to(torch.int32)
    slots[2] = -1
    return torch.randint(0, 128, (T,), generator=gen).to(torch.int32).cuda(), slots.cuda()


def short_lens(gen):
    return torch.randint(33, 101, (BATCH,), generator=gen).tolist() if BATCH else LENS_SHORT


def shas(*ts) -> str:
    return hashlib.sha256("".join(sha(t) for t in ts).encode()).hexdigest()


def i32(v):
    return torch.tensor(v, dtype=torch.int32).cuda()


def extras(gen, mode, hq, hkv, hd):
    bias = rnd(gen, (hq + 2 * hkv) * hd, scale=0.5) if mode in ("bias", "both") else None
    qkn = None
    if mode in ("norm", "both"):
        w = [(1 + 0.3 * torch.randn(hd, generator=gen)).to(torch.bfloat16).cuda() for _ in "qk"]
        qkn = (w[0], w[1], 1e-6)
    return bias, qkn


def paged(gen, lens, hkv, hd):
    """Cache, block tables (a permutation of the blocks) and the last token's slot per row."""
    nblk = sum(-(-n // BS) for n in lens) + 8
    kc, vc = rnd(gen, nblk, hkv, BS, hd), rnd(gen, nblk, hkv, BS, hd)
    perm = torch.randperm(nblk, generator=gen).tolist()
    maxb = max(-(-n // BS) for n in lens)
    tables, slots, o = [], [], 0
    for n in lens:
        nb = -(-n // BS)
        blocks = perm[o:o + nb]
        o += nb
        tables.append(blocks + [0] * (maxb - nb))
        slots.append(blocks[(n - 1) // BS] * BS + (n - 1) % BS)
    return kc, vc, i32(tables), i32(slots), i32(lens)


def rope_and_cache_cases():
    gen = torch.Generator().manual_seed(41)
    T = 32 * BATCH or 7
    nblk = -(-T // BS) + 2
    pos, slots = tokens(gen, T, nblk)
    for hq, hkv, hd in ((32, 8, 128), (4, 2, 64), (7, 1, 128)):
        n = (hq + 2 * hkv) * hd
        buf0 = rnd(gen, T, n + 64)
        kc0, vc0 = rnd(gen, nblk, hkv, BS, hd), rnd(gen, nblk, hkv, BS, hd)
        cs = R.rope_cos_sin(128, hd, 1e6, device="cuda")
        for mode in MODES:
            bias, qkn = extras(gen, mode, hq, hkv, hd)
            for rope in (True, False):
                def run(buf0=buf0, kc0=kc0, vc0=vc0, cs=cs, bias=bias, qkn=qkn, rope=rope,
                        hq=hq, hkv=hkv, hd=hd, n=n):
                    buf, kc, vc = buf0.clone(), kc0.clone(), vc0.clone()
                    ops.rope_and_cache(buf[:, :n], pos, slots, cs, kc, vc, hq, hkv, hd,
                                       use_rope=rope, bias=bias, qk_norm=qkn)
                    return shas(buf, kc, vc)
                yield f"heads {hq},{hkv},{hd} {mode} rope={int(rope)}", run


def linear_rope_cache_cases():
    gen = torch.Generator().manual_seed(42)
    hq, hkv, hd, M = 32, 8, 128, BATCH or 7
    nblk = -(-M // BS) + 3
    n = (hq + 2 * hkv) * hd
    x, w = rnd(gen, M, K_IN), rnd(gen, n, K_IN, scale=0.05)
    pos, slots = tokens(gen, M, nblk)
    cs = R.rope_cos_sin(128, hd, 1e6, device="cuda")
    kc0, vc0 = rnd(gen, nblk, hkv, BS, hd), rnd(gen, nblk, hkv, BS, hd)
    for mode in MODES:
        bias, qkn = extras(gen, mode, hq, hkv, hd)
        for splits in (1, 2, 3, 4, 8):
            for f16 in (False, True):
                def run(bias=bias, qkn=qkn, splits=splits, f16=f16):
                    G.SLAB16 = f16
                    kc, vc = kc0.clone(), vc0.clone()
                    qkv = ops.linear_rope_cache(x, w, pos, slots, cs, kc, vc, hq, hkv, hd,
                                                plan=G.GemmPlan("dli", 0, splits), bias=bias,
                                                qk_norm=qkn)
                    return shas(qkv, kc, vc)
                yield f"{mode} s{splits} fp16={int(f16)}", run


def linear_add_rmsnorm_cases():
    gen = torch.Generator().manual_seed(43)
    M = BATCH or 7
    x = rnd(gen, M, K_IN)
    for N in (512, 2000, 4096, 8192):
        w, res0, nw = rnd(gen, N, K_IN, scale=0.05), rnd(gen, M, N), rnd(gen, N)
        for splits in (2, 3, 4, 8):
            for f16 in (False, True):
                for norm in (True, False):
                    def run(w=w, res0=res0, nw=nw if norm else None, splits=splits, f16=f16):
                        G.SLAB16 = f16
                        res = res0.clone()
                        out = ops.linear_add_rmsnorm(x, w, res, nw, 1e-5,
                                                     plan=G.GemmPlan("dli", 0, splits))
                        return shas(res) if out is None else shas(res, out)
                    yield f"N={N} s{splits} fp16={int(f16)} norm={int(norm)}", run
    N, E, k = 4096, 8, 2
    w, res0, nw, wr = rnd(gen, N, K_IN, scale=0.05), rnd(gen, M, N), rnd(gen, N), rnd(gen, E, N)
    for splits in (2, 4, 8):
        for f16 in (False, True):
            def gate(splits=splits, f16=f16):
                G.SLAB16 = f16
                res = res0.clone()
                out, tw, ti = ops.linear_add_rmsnorm(x, w, res, nw, 1e-5,
                                                     plan=G.GemmPlan("dli", 0, splits),
                                                     route=(wr, k))
                return shas(res, out, tw, ti)
            yield f"gate N={N} E={E} k={k} s{splits} fp16={int(f16)}", gate


def moe_combine_cases():
    """The two slab combines (``ops.MoEPending``) on fp16 slabs of their own (partials of the
    size a down projection leaves): T tokens x 2 picks over T k + 2 permuted rows, two picks
    dropped."""
    gen = torch.Generator().manual_seed(44)
    T, k, dim = BATCH or 9, 2, 4096
    rows = T * k + 2
    pos = torch.randperm(rows, generator=gen)[:T * k].to(torch.int32).view(T, k)
    pos[2, 1] = pos[7, 0] = -1
    pos = pos.cuda()
    tw = torch.rand(T, k, generator=gen).cuda()
    res0, nw = rnd(gen, T, dim), rnd(gen, dim)
    for S in (2, 4, 8):
        ws = (torch.randn(S, rows, dim, generator=gen) * 0.03).to(torch.float16).cuda()
        pend = ops.MoEPending(ws, S, rows, tw, pos, (T, dim), torch.bfloat16, ws.device)
        yield "moe_combine_slabs", f"s{S}", lambda pend=pend: shas(pend.materialize())
        for norm in (True, False):
            def addn(pend=pend, nwp=nw if norm else None):
                res = res0.clone()
                out = pend.add_rmsnorm(res, nwp, 1e-5)
                return shas(res) if out is None else shas(res, out)
            yield "moe_combine_add_rmsnorm", f"s{S} norm={int(norm)}", addn


def decode_attention_cases():
    gen = torch.Generator().manual_seed(45)
    hq, hkv = 32, 8
    for hd in (128, 64):
        for lens in ((short_lens(gen),) if BATCH else (LENS_SHORT, LENS_LONG)):
            kc, vc, tables, _, ctx = paged(gen, lens, hkv, hd)
            qkv = rnd(gen, len(lens), (hq + 2 * hkv) * hd)
            for form, pipe, wpi in (("pipe", 1, 0), ("wg", 0, 4), ("wave", 0, 1)):
                for splits in (1, 2, 4):
                    for window in (0, WIN):
                        def run(kc=kc, vc=vc, tables=tables, ctx=ctx, qkv=qkv, lens=lens,
                                hd=hd, pipe=pipe, wpi=wpi, splits=splits, window=window):
                            old_p, old_f = ops.decode_pipelined(pipe), ops.decode_form(wpi)
                            try:
                                return shas(ops.decode_attention(
                                    qkv, kc, vc, tables, ctx, max(lens), hq, hkv, hd,
                                    1 / math.sqrt(hd), num_splits=splits, window=window))
                            finally:
                                ops.decode_pipelined(old_p)
                                ops.decode_form(old_f)
                        yield f"hd{hd} lens{len(lens)} {form} s{splits} w{window}", run


def linear_rope_attention_cases():
    gen = torch.Generator().manual_seed(46)
    hq, hkv, hd = 32, 8, 128
    lens = short_lens(gen)
    n, B = (hq + 2 * hkv) * hd, len(lens)
    kc0, vc0, tables, slots, ctx = paged(gen, lens, hkv, hd)
    pos = ctx - 1
    cs = R.rope_cos_sin(2048, hd, 1e6, device="cuda")
    x, w = rnd(gen, B, K_IN), rnd(gen, n, K_IN, scale=0.05)
    for mode in MODES:
        bias, qkn = extras(gen, mode, hq, hkv, hd)
        for wpi in (1, 4):
            for splits, f16 in ((0, False), (2, False), (2, True), (4, False), (4, True)):
                for window in (0, WIN):
                    def run(bias=bias, qkn=qkn, wpi=wpi, splits=splits, f16=f16, window=window):
                        G.SLAB16 = f16
                        G.set_plan(B, n, K_IN, "splitk", G.GemmPlan("dli", 0, max(splits, 1)))
                        old = ops.decode_form(wpi)
                        try:
                            kc, vc = kc0.clone(), vc0.clone()
                            out = ops.linear_rope_attention(
                                x, w, pos, slots, cs, kc, vc, tables, ctx, max(lens), hq,
                                hkv, hd, 1 / math.sqrt(hd), window=window, bias=bias,
                                qk_norm=qkn)
                            assert out is not None, "the fused kernel was not taken"
                            return shas(out, kc, vc)
                        finally:
                            ops.decode_form(old)
                            G.clear_plans()
                    yield f"{mode} form{wpi} s{splits} fp16={int(f16)} w{window}", run


def all_cases():
    for op, gen in (("rope_and_cache", rope_and_cache_cases),
                    ("linear_rope_cache", linear_rope_cache_cases),
                    ("linear_add_rmsnorm", linear_add_rmsnorm_cases)):
        for name, run in gen():
            yield op, name, run
    yield from moe_combine_cases()
    for op, gen in (("decode_attention", decode_attention_cases),
                    ("linear_rope_attention", linear_rope_attention_cases)):
        for name, run in gen():
            yield op, name, run


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", type=Path, help="one line per case")
    ap.add_argument("--rollup", type=Path, help="one line per op")
    ap.add_argument("--from", dest="src", type=Path, help="roll up this case file, run nothing")
    ap.add_argument("--batch", type=int, default=0,
                    help="rows / sequences per case (512: a decode batch); default: the tests' 7")
    a = ap.parse_args()
    global BATCH
    BATCH = max(a.batch, 0)
    if a.src:
        a.rollup.write_text("\n".join(rollup(a.src.read_text().splitlines())) + "\n")
        return
    slab16 = G.SLAB16
    lines = []
    try:
        for op, name, run in all_cases():
            try:
                digest = run()
            except RuntimeError as e:
                # a launcher refusing the case (hipErrorInvalidValue, before any launch) is
                # part of the record; anything else, a fault above all, ends the run
                if not str(e).endswith("failed with hipError 1"):
                    raise
                digest = "refused"
            lines.append(json.dumps({"tile": op, "case": name, "sha256": digest}))
    finally:
        G.SLAB16 = slab16
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text("\n".join(lines) + "\n")
    if a.rollup:
        a.rollup.write_text("\n".join(rollup(lines)) + "\n")
    print(f"{len(lines)} cases -> {a.out or a.rollup}")


if __name__ == "__main__":
    main()
