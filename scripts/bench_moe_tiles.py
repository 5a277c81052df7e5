#!/usr/bin/env python3
"""Every grouped-GEMM candidate plan for the Mixtral 8x7B MoE projections at one decode
batch, timed as ``ops.gemm.autotune_grouped`` times them (seeded multinomial routing of
``rows = batch * top_k`` permuted rows over the experts; the expert weights together exceed
the Infinity Cache, so each call streams them from HBM). Prints one JSON line per plan,
sorted by time, with the achieved weight-streaming bandwidth.

    python scripts/bench_moe_tiles.py [--batch 512] [--which down,gate_up]
    python scripts/bench_moe_tiles.py --batch 16384 --tiles 22,45   # prefill-sized experts

With ``--tiles`` only those tiles run, and the grid is bounded by the largest expert's rows
(the eager prefill path of ``ops.moe_mlp``) instead of all rows.

    python scripts/bench_moe_tiles.py --weight-dtype fp8 --model qwen3-30b-a3b --batch 64

FP8 expert stacks (``ops.Fp8Experts``, random bytes and scales): the grouped FP8 stream tiles
70 / 71 at ``G.fp8_grouped_bm``, the dequantise pass + the fastest bf16 plan (the pass in the
timing), and that bf16 plan alone on the bf16 image (what bf16 weights cost). One JSON line
each, with the time and the FP8 weight bytes per second.
"""
import argparse
import itertools
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


MODELS = {"mixtral-8x7b": (8, 4096, 14336, 2), "qwen3-30b-a3b": (128, 2048, 768, 8)}


def fp8_probe(a, ops, G, dev):
    E, D, F, topk = MODELS[a.model]
    rows = a.batch * topk
    counts = np.random.default_rng(1234).multinomial(rows, [1.0 / E] * E).tolist()
    off = torch.tensor([0] + list(itertools.accumulate(counts)), dtype=torch.int32, device=dev)
    bm = G.fp8_grouped_bm(rows, E)
    for which in a.which.split(","):
        N, K, epi = (D, F, "none") if which == "down" else (2 * F, D, "silu_mul")
        q = torch.empty(E, N, K, dtype=torch.float8_e4m3fn, device=dev)
        for e in range(E):                       # (an expert at a time: no fp32 stack)
            q[e] = torch.randn(N, K, device=dev).to(torch.float8_e4m3fn)
        s = torch.exp2(torch.rand(E, N // 16, -(-K // 128), device=dev) * 4 - 10)
        w = ops.Fp8Experts(q, s)
        x = (torch.randn(rows, K, device=dev) * 0.5).to(torch.bfloat16)
        y = torch.empty(rows, N // 2 if epi == "silu_mul" else N, dtype=torch.bfloat16,
                        device=dev)
        base = {"model": a.model, "which": which, "batch": a.batch, "rows": rows, "E": E,
                "N": N, "K": K}

        def report(kind, ms, **kw):
            print(json.dumps(dict(base, kind=kind, us=round(ms * 1e3, 1),
                                  fp8_TBps=round(w.numel() / (ms * 1e-3) / 1e12, 2), **kw)),
                  flush=True)
        tl = G.host_tile_list(counts, bm, dev)
        for tile in sorted(G.FP8_STREAM_TILES):
            p = G.GemmPlan("dli", tile, 1)
            ms = ops.benchmark(lambda: ops.grouped_fp8_stream(x, w, p, epi, y, off, rows, bm, tl),
                               iters=a.iters, warmup=1)
            report("stream", ms, tile=tile, bm=bm)
        image = w.bf16()
        lists, timed = {}, []
        for tile in sorted(G.TILES):
            if G.TILES[tile][0] > 2 * max(64, rows // E + 32) or not G.tile_ok(tile, epi):
                continue
            p = G.GemmPlan("dli", tile, 1)
            t = None
            if G.list_plan(p, E):
                t = lists.setdefault(G.TILES[tile][0],
                                     G.host_tile_list(counts, G.TILES[tile][0], dev))

            def run(wb=None, p=p, t=t):
                ops._gemm_native(x, image if wb is None else wb(), epi, plan=p, groups=E,
                                 group_off=off, rows_per_group=rows, tile_list=t)
            try:
                timed.append((ops.benchmark(run, iters=a.iters, warmup=1), tile, run))
            except Exception:  # noqa: BLE001
                continue
        ms, tile, run = min(timed, key=lambda r: r[0])
        report("bf16_weights", ms, tile=tile, bm_bn=G.TILES[tile])
        report("dequantise+bf16", ops.benchmark(lambda: run(w.bf16), iters=a.iters, warmup=1),
               tile=tile, bm_bn=G.TILES[tile])
        report("dequantise_pass", ops.benchmark(w.bf16, iters=a.iters, warmup=1))
        del w, q, image


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weight-dtype", default="bf16", choices=["bf16", "fp8"])
    ap.add_argument("--model", default="mixtral-8x7b", choices=sorted(MODELS))
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--which", default="down,gate_up")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--tiles", default="")
    a = ap.parse_args()
    only = [int(t) for t in a.tiles.split(",") if t]
    from distributed_llm_inferencing_amd import ops
    from distributed_llm_inferencing_amd.ops import gemm as G
    dev = torch.device("cuda")
    if a.weight_dtype == "fp8":
        return fp8_probe(a, ops, G, dev)
    E, D, F = 8, 4096, 14336
    rows = a.batch * 2
    counts = np.random.default_rng(1234).multinomial(rows, [1.0 / E] * E).tolist()
    off = torch.tensor([0] + list(itertools.accumulate(counts)), dtype=torch.int32, device=dev)
    for which in a.which.split(","):
        N, K, epi = (D, F, "none") if which == "down" else (2 * F, D, "silu_mul")
        w = (torch.randn(E, N, K, device=dev) * 0.02).to(torch.bfloat16)
        x = (torch.randn(rows, K, device=dev) * 0.5).to(torch.bfloat16)
        out = []
        rpg = max(counts) if only else rows
        ones = torch.ones(rows, 1, dtype=torch.float32, device=dev)
        ident = torch.arange(rows, dtype=torch.int32, device=dev).view(-1, 1)
        comb = torch.empty(rows, N, dtype=torch.bfloat16, device=dev)
        for tile in (only or sorted(G.TILES)):
            if not only and (G.TILES[tile][0] > 2 * max(64, rows // E + 32)
                             or not G.tile_ok(tile, epi)):
                continue
            for splits in (1, 2, 4):
                if splits > 1 and not (K % (64 * splits) == 0 and K // splits >= 2048):
                    continue
                p = G.GemmPlan("dli", tile, splits)
                # split down plans on the fp16-slab tiles: the fused slab combine as the
                # model runs it (ops.moe_down_combine; one pick per row, weight 1)
                fused = which == "down" and ops.moe_slab_plan(p) and not only

                def run(p=p, fused=fused):
                    if fused:
                        ops.moe_down_combine(x, w, off, rows, p, ones, ident, comb)
                    else:
                        ops._gemm_native(x, w, epi, plan=p, groups=E, group_off=off,
                                         rows_per_group=rpg)
                try:
                    ms = ops.benchmark(run, iters=a.iters, warmup=1)
                except Exception as e:  # noqa: BLE001
                    out.append({"which": which, "tile": tile, "splits": splits,
                                "error": str(e)[:60]})
                    continue
                out.append({"which": which, "rows": rows, "tile": tile,
                            "bm_bn": G.TILES.get(tile), "splits": splits, "fused": fused,
                            "us": round(ms * 1e3, 1),
                            "tflops": round(2.0 * rows * N * K / (ms * 1e-3) / 1e12, 1),
                            "weight_TBps": round(w.numel() * 2 / (ms * 1e-3) / 1e12, 2)})
        for r in sorted(out, key=lambda r: r.get("us", 1e9)):
            print(json.dumps(r), flush=True)
        del w


if __name__ == "__main__":
    main()
