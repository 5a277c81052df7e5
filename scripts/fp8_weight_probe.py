#!/usr/bin/env python3
"""The weight stream with bf16 and FP8 block-scaled weights, per Llama-3-8B projection, timed as
graph replays over cold weights (a different weight copy per call, together larger than the
Infinity Cache, as bench_decode_tiles.py does). Microseconds and weight GB/s (the weight's
bytes, scales included, over the time), one JSON line each.

    python scripts/fp8_weight_probe.py [--m 1,2,3,4,8,16,32,64] [--shapes qkv,o,gate_up,down]

M <= 4: every GEMV plan (tile x split-K) of each (projection, M, weight dtype), the fastest
reported. Epilogues are the batch-1 chain's: QKV bf16 rows, O and down adding into the residual
(``ops.linear_residual``), gate/up with SiLU*up.

4 < M <= 64: per (projection, M) one line for EVERY FP8 stream plan (``path`` "fp8_stream":
the MFMA weight-stream tiles, split plans with their reduce kernel), one for the fastest plan
of the dequantise + bf16-GEMM path on the same FP8 weight ("fp8_dequant": the dequantise
kernel's time and its bytes are in it; the rate still counts the FP8 bytes) and one for the
fastest plan of the bf16-weight GEMM ("bf16"). Epilogues: bf16 rows, gate/up with SiLU*up.
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


def timed(ops, run, iters, n):
    try:
        return ops.benchmark(run, iters=iters, warmup=1, graph=True) / n
    except RuntimeError as e:                 # the launcher refused the plan (hipError)
        print(f"# skipped: {e}", file=sys.stderr)
        return None


def line(name, N, K, epi, M, path, p, ms, nbytes, copies):
    print(json.dumps({"shape": name, "N": N, "K": K, "epi": epi, "M": M, "weights": path,
                      "tile": p.tile, "splits": p.splits, "us": round(ms * 1e3, 2),
                      "weight_gbs": round(nbytes / (ms * 1e-3) / 1e9, 1), "copies": copies}),
          flush=True)


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
    ms_ = [int(m) for m in a.m.split(",")]
    if any(m < 1 or m > G.FP8_STREAM_MAX_M for m in ms_):
        ap.error(f"--m takes values in 1..{G.FP8_STREAM_MAX_M}")
    for name in a.shapes.split(","):
        N, K, epi = SHAPES[name]
        wb = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
        q, s = R.quantize_weight(wb)
        w8 = ops.Fp8Weight(q, R.group_scales(R.row_scales(s, N)))
        for dt, w0, nbytes in (("bf16", wb, N * K * 2),
                               ("fp8", w8, N * K + w8.scale.numel() * 4)):
            n_copies = max(2, min(16, -(-(1 << 30) // nbytes)))
            ws_ = [w0] + [w0.clone() for _ in range(n_copies - 1)]
            for M in ms_:
                x = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16)
                if M > G.GEMV_MAX_M:
                    mid_batch(ops, G, name, N, K, "silu_mul" if epi == "silu_mul" else "none", M,
                              dt, ws_, x, nbytes, a.iters)
                    continue
                res = torch.zeros(M, N, dtype=torch.bfloat16, device=dev)
                best = None
                for p in plans(G, M, N, K, epi):
                    def run(p=p):
                        for w in ws_:
                            if epi == "res":
                                ops.linear_residual(x, w, res, plan=p)
                            else:
                                ops._gemm_native(x, w, epi, plan=p)
                    ms = timed(ops, run, a.iters, len(ws_))
                    if ms is not None and (best is None or ms < best[0]):
                        best = (ms, p)
                if best is not None:
                    line(name, N, K, epi, M, dt, best[1], best[0], nbytes, n_copies)
            del ws_
        del wb, w8


def mid_batch(ops, G, name, N, K, epi, M, dt, ws_, x, nbytes, iters):
    """4 < M <= 64 on one weight dtype: see the module docstring."""
    def time_plan(p):
        def run():
            for w in ws_:
                ops._gemm_native(x, w, epi, plan=p)
        return timed(ops, run, iters, len(ws_))
    if dt == "fp8":
        for p in G.fp8_stream_plans(M, N, K, epi):
            ms = time_plan(p)
            if ms is not None:
                line(name, N, K, epi, M, "fp8_stream", p, ms, nbytes, len(ws_))
    best = None
    for p in G.candidate_plans(M, N, K, epi):
        ms = time_plan(p)
        if ms is not None and (best is None or ms < best[0]):
            best = (ms, p)
    if best is not None:
        line(name, N, K, epi, M, "fp8_dequant" if dt == "fp8" else "bf16", best[1], best[0],
             nbytes, len(ws_))


if __name__ == "__main__":
    main()
