#!/usr/bin/env python3
"""SHA-256 of everything the QKV-to-attention ops write on seeded inputs (every output and every
touched cache), one JSON line per case, to compare two builds bit for bit: run it in each tree,
then diff the two files. Beside scripts/attn_digest.py (the tests' shapes, bf16 caches, the
split-K reduces and MoE combines too) this one walks what the native entry points dispatch on:
both cache dtypes (an FP8 cache with scales other than 1) and the prefill kernels as well, at
shapes just large enough to cross every boundary: B = 3, 8 query / 2 kv heads, block size 16,
contexts 1 / 31 / 33 / 70 (one tile, a tile edge, two and three tiles; a block edge), K = 256.
Only the public ``ops`` functions and their test switches are used, so the same file runs in
any tree that has them.

    python scripts/attn_abi_digest.py --out attn_abi_digest.jsonl
"""
import argparse
import hashlib
import itertools
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from distributed_llm_inferencing_amd import ops  # noqa: E402
from distributed_llm_inferencing_amd.ops import gemm as G  # noqa: E402
from distributed_llm_inferencing_amd.ops import reference as R  # noqa: E402

BF = torch.bfloat16
HQ, HKV, BS, K_IN, WIN = 8, 2, 16, 256, 40
CTXS = ((1, 31, 70), (33, 70, 31))
B = 3
KV = {"bf16": (1.0, 1.0), "fp8": (0.5, 2.0)}          # cache dtype -> (k_scale, v_scale)


def sha(*ts) -> str:
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in ts:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def rnd(gen, *shape, scale=1.0, dtype=BF):
    return (torch.randn(*shape, generator=gen) * scale).to(dtype).cuda()


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def caches(gen, nblk, hd, kvd):
    kc, vc = rnd(gen, nblk, HKV, BS, hd), rnd(gen, nblk, HKV, BS, hd)
    if kvd == "fp8":
        kc, vc = kc.to(R.FP8_KV), vc.to(R.FP8_KV)
    return kc, vc


def paged(gen, ctxs):
    """Shuffled block tables of the contexts, the slot of each one's last token, block count."""
    nb = [-(-c // BS) for c in ctxs]
    nblk = sum(nb) + 2
    perm = torch.randperm(nblk, generator=gen).tolist()
    tables, slots, o = [], [], 0
    for c, n in zip(ctxs, nb):
        blocks = perm[o:o + n]
        o += n
        tables.append(blocks + [0] * (max(nb) - n))
        slots.append(blocks[(c - 1) // BS] * BS + (c - 1) % BS)
    return i32(tables), i32(slots), nblk


def extras(gen, mode, hd):
    n = (HQ + 2 * HKV) * hd
    bias = rnd(gen, n, scale=0.5) if mode in ("bias", "both") else None
    qkn = None
    if mode in ("norm", "both"):
        qkn = (rnd(gen, hd, scale=0.3) + 1, rnd(gen, hd, scale=0.3) + 1, 1e-6)
    return bias, qkn


def writer_cases():
    """rope_and_cache and linear_rope_cache: plans of 1 / 2 / 4 splits in both slab formats x
    no extras / bias / QK-norm x cache dtype."""
    hd = 128
    n = (HQ + 2 * HKV) * hd
    gen = torch.Generator().manual_seed(1)
    x, w = rnd(gen, B, K_IN), rnd(gen, n, K_IN, scale=0.05)
    qkv0 = rnd(gen, B, n)
    pos = i32([0, 30, 69])
    slots = i32([5, -1, 40])
    cs = R.rope_cos_sin(128, hd, 1e6, device="cuda")
    ext = {m: extras(gen, m, hd) for m in ("none", "bias", "norm")}
    for kvd, mode in itertools.product(KV, ext):
        ks, vs = KV[kvd]
        bias, qkn = ext[mode]

        def rows(kvd=kvd, bias=bias, qkn=qkn, ks=ks, vs=vs):
            kc, vc = caches(torch.Generator().manual_seed(2), 4, hd, kvd)
            qkv = qkv0.clone()
            ops.rope_and_cache(qkv, pos, slots, cs, kc, vc, HQ, HKV, hd, bias=bias, qk_norm=qkn,
                               k_scale=ks, v_scale=vs)
            return qkv, kc, vc
        yield f"rope_and_cache {kvd} {mode}", rows
        for splits, f16 in ((1, False), (2, False), (2, True), (4, False), (4, True)):
            def slabs(kvd=kvd, bias=bias, qkn=qkn, ks=ks, vs=vs, splits=splits, f16=f16):
                kc, vc = caches(torch.Generator().manual_seed(2), 4, hd, kvd)
                old, G.SLAB16 = G.SLAB16, f16
                try:
                    qkv = ops.linear_rope_cache(x, w, pos, slots, cs, kc, vc, HQ, HKV, hd,
                                                plan=G.GemmPlan("dli", 0, splits), bias=bias,
                                                qk_norm=qkn, k_scale=ks, v_scale=vs)
                finally:
                    G.SLAB16 = old
                return qkv, kc, vc
            yield f"linear_rope_cache {kvd} {mode} s{splits} fmt{int(f16)}", slabs


def fused_cases():
    """linear_rope_attention: rows, 2 and 4 slabs in both formats x a wave / a workgroup per
    item x extras x window."""
    hd = 128
    n = (HQ + 2 * HKV) * hd
    gen = torch.Generator().manual_seed(3)
    x, w = rnd(gen, B, K_IN), rnd(gen, n, K_IN, scale=0.05)
    cs = R.rope_cos_sin(128, hd, 1e6, device="cuda")
    ext = {m: extras(gen, m, hd) for m in ("none", "bias", "both")}
    for ctxs in CTXS:
        tables, slots, nblk = paged(gen, ctxs)
        ctx = i32(ctxs)
        kc0, vc0 = caches(gen, nblk, hd, "bf16")
        for (splits, f16), form, mode, window in itertools.product(
                ((1, False), (2, False), (2, True), (4, False), (4, True)), (1, 4), ext,
                (0, WIN)):
            def run(splits=splits, f16=f16, form=form, mode=mode, window=window, tables=tables,
                    slots=slots, ctx=ctx, kc0=kc0, vc0=vc0, ctxs=ctxs):
                kc, vc = kc0.clone(), vc0.clone()
                bias, qkn = ext[mode]
                old_form, (old16, G.SLAB16) = ops.decode_form(form), (G.SLAB16, f16)
                G.set_plan(B, n, K_IN, "splitk", G.GemmPlan("dli", 0, splits))
                try:
                    out = ops.linear_rope_attention(x, w, ctx - 1, slots, cs, kc, vc, tables, ctx,
                                                    max(ctxs), HQ, HKV, hd, hd ** -0.5,
                                                    window=window, bias=bias, qk_norm=qkn)
                finally:
                    G.clear_plans()
                    G.SLAB16 = old16
                    ops.decode_form(old_form)
                assert out is not None
                return out, kc, vc
            yield (f"linear_rope_attention ctx{ctxs} s{splits} fmt{int(f16)} form{form} {mode} "
                   f"w{window}"), run


def decode_cases():
    """decode_attention: hd x KV splits x form x pipe x window x cache dtype."""
    gen = torch.Generator().manual_seed(4)
    for hd, ctxs in itertools.product((64, 128), CTXS):
        n = (HQ + 2 * HKV) * hd
        qkv = rnd(gen, B, n)
        tables, _, nblk = paged(gen, ctxs)
        ctx = i32(ctxs)
        for kvd in KV:
            kc, vc = caches(gen, nblk, hd, kvd)
            ks, vs = KV[kvd]
            for ns, form, pipe, window in itertools.product((1, 2), (1, 4), (0, 1), (0, WIN)):
                def run(hd=hd, qkv=qkv, tables=tables, ctx=ctx, kc=kc, vc=vc, ks=ks, vs=vs,
                        ns=ns, form=form, pipe=pipe, window=window, ctxs=ctxs):
                    old_form, old_pipe = ops.decode_form(form), ops.decode_pipelined(pipe)
                    try:
                        return (ops.decode_attention(qkv, kc, vc, tables, ctx, max(ctxs), HQ, HKV,
                                                     hd, hd ** -0.5, num_splits=ns, window=window,
                                                     k_scale=ks, v_scale=vs),)
                    finally:
                        ops.decode_pipelined(old_pipe)
                        ops.decode_form(old_form)
                yield (f"decode_attention hd{hd} ctx{ctxs} {kvd} splits{ns} form{form} "
                       f"pipe{pipe} w{window}"), run


def prefill_cases():
    """prefill_attention and prefill_attention_paged: batches of 5 / 33 / 70-token sequences
    (and 31, the two-head packing) x window x packing x (the 64-row kernels | the 256-row
    kernel, by a lowered threshold) x cache dtype."""
    gen = torch.Generator().manual_seed(5)
    for hd, lens in itertools.product((128, 64), ((5,), (31, 5), (5, 33), (5, 33, 70))):
        n = (HQ + 2 * HKV) * hd
        T = sum(lens)
        qkv = rnd(gen, T, n)
        cu = i32([0] + list(itertools.accumulate(lens)))
        ctxs = tuple(ln + p for ln, p in zip(lens, (0, 31, 17)))
        tables, _, nblk = paged(gen, ctxs)
        ctx = i32(ctxs)
        kv = {kvd: caches(gen, nblk, hd, kvd) for kvd in KV}
        for window, pack, long_ in itertools.product((0, WIN), (True, False), (False, True)):
            if long_ and (max(lens) != 70 or hd != 128 or not pack):
                continue                               # the 256-row kernel: once per window

            def switched(fn, pack=pack, long_=long_):
                old_pack = ops.prefill_set_pack(pack)
                old_min = ops.prefill_long_min_len(64 if long_ else 256)
                try:
                    return (fn(),)
                finally:
                    ops.prefill_long_min_len(old_min)
                    ops.prefill_set_pack(old_pack)

            def packed(sw=switched, qkv=qkv, cu=cu, lens=lens, hd=hd, window=window):
                return sw(lambda: ops.prefill_attention(qkv, cu, max(lens), HQ, HKV, hd,
                                                        hd ** -0.5, window=window))
            tag = f"hd{hd} lens{lens} w{window} pack{int(pack)} long{int(long_)}"
            yield f"prefill_attention {tag}", packed
            for kvd in KV:
                def chunk(sw=switched, qkv=qkv, cu=cu, lens=lens, hd=hd, window=window, ctx=ctx,
                          tables=tables, kv=kv, kvd=kvd):
                    return sw(lambda: ops.prefill_attention_paged(
                        qkv, cu, max(lens), ctx, tables, *kv[kvd], HQ, HKV, hd, hd ** -0.5,
                        window=window, k_scale=KV[kvd][0], v_scale=KV[kvd][1]))
                yield f"prefill_attention_paged {kvd} {tag}", chunk


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", type=Path, required=True, help="one line per case")
    a = ap.parse_args()
    lines = []
    for name, run in itertools.chain(writer_cases(), fused_cases(), decode_cases(),
                                     prefill_cases()):
        try:
            digest = sha(*run())
        except RuntimeError as e:
            # a launcher refusing the case (hipErrorInvalidValue, before any launch) is part of
            # the record; anything else, a fault above all, ends the run
            if not str(e).endswith("failed with hipError 1"):
                raise
            digest = "refused"
        lines.append(json.dumps({"case": name, "sha256": digest}))
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text("\n".join(lines) + "\n")
    print(f"{len(lines)} cases, {sum('refused' in x for x in lines)} refused -> {a.out}")


if __name__ == "__main__":
    main()
