#!/usr/bin/env python3
"""The M <= 4 weight stream with bf16 and FP8 block-scaled weights, per Llama-3-8B projection:
every GEMV plan (tile x split-K) of each (projection, M, weight dtype) timed as a graph replay
over cold weights (a different weight copy per call, together larger than the Infinity Cache,
as bench_decode_tiles.py does), the fastest reported. One JSON line per (projection, M, dtype):
microseconds and weight GB/s (the weight's bytes, scales included, over the time).

    python scripts/fp8_weight_probe.py [--m 1,2,3,4] [--shapes qkv,o,gate_up,down]

Epilogues are the batch-1 chain's: QKV bf16 rows, O and down adding into the residual
(``ops.linear_residual``), gate/up with SiLU*up.
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

SHAPES = {"qkv": (6144, 4096, "none"), "o": (4096, 4096, "res"),
          "gate_up": (28672, 4096, "silu_mul"), "down": (4096, 14336, "res")}


def plans(G, M, N, K, epi):
    if epi == "res":
        return G.candidate_plans(M, N, K, "res")
    return [p for p in G.candidate_plans(M, N, K, epi) if p.tile in G.GEMV_TILES]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", default="1,2,3,4")
    ap.add_argument("--shapes", default="qkv,o,gate_up,down")
    ap.add_argument("--iters", type=int, default=6)
    a = ap.parse_args()
    from distributed_llm_inferencing_amd import ops
    from distributed_llm_inferencing_amd.ops import gemm as G
    from distributed_llm_inferencing_amd.ops import reference as R
    dev = torch.device("cuda")
    for name in a.shapes.split(","):
        N, K, epi = SHAPES[name]
        wb = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
        q, s = R.quantize_weight(wb)
        w8 = ops.Fp8Weight(q, R.group_scales(R.row_scales(s, N)))
        for dt, w0, nbytes in (("bf16", wb, N * K * 2),
                               ("fp8", w8, N * K + w8.scale.numel() * 4)):
            n_copies = max(2, min(16, -(-(1 << 30) // nbytes)))
            ws_ = [w0] + [w0.clone() for _ in range(n_copies - 1)]
            for M in [int(m) for m in a.m.split(",")]:
                x = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16)
                res = torch.zeros(M, N, dtype=torch.bfloat16, device=dev)
                best = None
                for p in plans(G, M, N, K, epi):
                    def run(p=p):
                        for w in ws_:
                            if epi == "res":
                                ops.linear_residual(x, w, res, plan=p)
                            else:
                                ops._gemm_native(x, w, epi, plan=p)
                    try:
                        ms = ops.benchmark(run, iters=a.iters, warmup=1, graph=True) / len(ws_)
                    except RuntimeError as e:     # the launcher refused the plan (hipError)
                        print(f"# skipped {name} M={M} {dt} {p}: {e}", file=sys.stderr)
                        continue
                    if best is None or ms < best[0]:
                        best = (ms, p)
                if best is None:
                    continue
                ms, p = best
                print(json.dumps({"shape": name, "N": N, "K": K, "epi": epi, "M": M,
                                  "weights": dt, "tile": p.tile, "splits": p.splits,
                                  "us": round(ms * 1e3, 2),
                                  "weight_gbs": round(nbytes / (ms * 1e-3) / 1e9, 1),
                                  "copies": n_copies}), flush=True)
            del ws_
        del wb, w8


if __name__ == "__main__":
    main()
