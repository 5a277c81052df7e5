#!/usr/bin/env python3
"""Decode attention (B sequences, one query each) and prefill attention (one prompt) timed
from graph replays, for the package under --root. --window needs a build that has it."""
import argparse
import json
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--root", required=True)
ap.add_argument("--tag", required=True)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--ctx", default="4096,16384")
ap.add_argument("--window", type=int, default=0)
ap.add_argument("--prefill", type=int, default=16384)
ap.add_argument("--reps", type=int, default=9)
a = ap.parse_args()
sys.path.insert(0, a.root)
from distributed_llm_inferencing_amd import ops  # noqa: E402

assert ops.__file__.startswith(a.root), ops.__file__
dev = torch.device("cuda")
hq, hkv, hd, bs = 32, 8, 128, 16
N = (hq + 2 * hkv) * hd
scale = hd ** -0.5
kw = {"window": a.window} if a.window else {}
R = 16
B = a.batch
for ctx in [int(c) for c in a.ctx.split(",")]:
    torch.manual_seed(0)
    nblk_seq = -(-ctx // bs)
    nblk = B * nblk_seq + 8
    kc = torch.empty(nblk, hkv, bs, hd, device=dev, dtype=torch.bfloat16).normal_(0, 0.5)
    vc = torch.empty(nblk, hkv, bs, hd, device=dev, dtype=torch.bfloat16).normal_(0, 0.5)
    perm = torch.randperm(nblk - 8, device=dev).to(torch.int32)
    bt = perm[:B * nblk_seq].view(B, nblk_seq).contiguous()
    cl = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    qkv = (torch.randn(B, N, device=dev) * 0.5).to(torch.bfloat16)
    out = torch.empty(B, hq * hd, dtype=torch.bfloat16, device=dev)

    def attn():
        ops.decode_attention(qkv, kc, vc, bt, cl, ctx, hq, hkv, hd, scale, out=out, **kw)

    row = {"tag": a.tag, "op": "decode", "batch": B, "ctx": ctx, "window": a.window}
    for name, mode in (("plain", 0), ("pipe", 1), ("auto", 2)):
        old = ops.decode_pipelined(mode)

        def rep():
            for _ in range(R):
                attn()
        try:
            row[name + "_us"] = round(ops.benchmark(rep, iters=a.reps, warmup=1, graph=True) / R * 1e3, 2)
        finally:
            ops.decode_pipelined(old)
    row["checksum"] = round(out.float().abs().sum().item(), 3)
    print(json.dumps(row), flush=True)
    del kc, vc
if a.prefill:
    torch.manual_seed(1)
    T = a.prefill
    qkv = (torch.randn(T, N, device=dev) * 0.5).to(torch.bfloat16)
    cu = torch.tensor([0, T], device=dev, dtype=torch.int32)
    out = torch.empty(T, hq * hd, dtype=torch.bfloat16, device=dev)

    def pf():
        ops.prefill_attention(qkv, cu, T, hq, hkv, hd, scale, out=out, **kw)
    ms = ops.benchmark(pf, iters=a.reps, warmup=2, graph=True)
    print(json.dumps({"tag": a.tag, "op": "prefill", "tokens": T, "window": a.window,
                      "ms": round(ms, 4), "checksum": round(out.float().abs().sum().item(), 2)}),
          flush=True)
