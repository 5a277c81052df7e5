#!/usr/bin/env python3
"""SHA-256 of the output bytes of every bf16 GEMM tile on seeded inputs, one JSON line per case,
to compare two builds bit for bit (run it in each tree, then diff the two files).

Covers every id in TILES: each epilogue tile_ok allows, plain with split-K 1 / 2 / 4 where
legal and grouped (MoE mode, an empty group and a partial last tile), the fp16 slab image of
the SLAB16_TILES, the row-gathering SiLU*up GEMM of the GATHER_TILES, and the persistent tile
55 unsplit on an even K-tile count only. Shapes as tests/test_gemm_stagger_gpu.py: M = 300,
N = 3 BN + 8 rounded up to the epilogue's multiple, K = 512 and 448 (partial row and column
tiles, an odd block, an unaligned tail).

    python scripts/gemm_digest.py --out gemm_digest.jsonl [--rollup per_tile.jsonl]
    python scripts/gemm_digest.py --from gemm_digest.jsonl --rollup per_tile.jsonl   # no GPU

``--rollup`` condenses the case lines to one line per tile (the SHA-256 of that tile's case
lines): the form small enough to keep in the repository.
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

M = 300
EPIS = ("none", "f32", "silu_mul", "bias_gelu", "bias")
GROUP_SIZES = [37, 0, 170, 5]


def sha(t: torch.Tensor) -> str:
    torch.cuda.synchronize()
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def rnd(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(torch.bfloat16).cuda()


def n_for(tile: int, epi: str) -> int:
    n = 3 * G.TILES[tile][1] + 8
    mult = (64 if tile == 22 else 32) if epi == "silu_mul" else 1
    return -(-n // mult) * mult


def cases(tile: int):
    """(case name, thunk returning the tensor to hash) of one tile."""
    gen = torch.Generator().manual_seed(1000 + tile)
    dev = torch.device("cuda")
    rows = sum(GROUP_SIZES)
    off = torch.tensor([0] + list(itertools.accumulate(GROUP_SIZES)), dtype=torch.int32,
                       device=dev)
    E = len(GROUP_SIZES)
    for K in (512, 448):
        if tile == 55 and K % 128:
            continue                                 # the persistent tile: even K-tile counts
        x = rnd(gen, M, K)
        xg = rnd(gen, rows, K)
        for epi in EPIS:
            if not G.tile_ok(tile, epi):
                continue
            N = n_for(tile, epi)
            w = rnd(gen, N, K, scale=0.05)
            wg = rnd(gen, E, N, K, scale=0.05)
            bias = rnd(gen, N) if epi in ("bias", "bias_gelu") else None
            for splits in (1, 2, 4):
                if K % (64 * splits) or (tile == 55 and splits > 1):
                    continue
                p = G.GemmPlan("dli", tile, splits)
                yield (f"plain K={K} N={N} {epi} s{splits}",
                       lambda p=p, w=w, b=bias, e=epi: ops._gemm_native(x, w, e, bias=b, plan=p))
                if tile != 55 and epi in ("none", "silu_mul") and splits < 4:
                    yield (f"grouped K={K} N={N} {epi} s{splits}",
                           lambda p=p, w=wg, e=epi: ops._gemm_native(
                               xg, w, e, plan=p, groups=E, group_off=off, rows_per_group=rows))
        if tile in G.SLAB16_TILES and K == 512:
            N = n_for(tile, "none")
            w = rnd(gen, N, K, scale=0.05)
            for splits in (2, 4):
                def slab(splits=splits, w=w, N=N):
                    ws = G.workspace(dev, splits * M * N * 4)
                    ws.zero_()
                    assert ops._slab_gemm(x, w, G.GemmPlan("dli", tile, splits), ws) == 1
                    return ws[:splits * M * N * 2].clone()
                yield f"slab16 K={K} N={N} s{splits}", slab
        if tile in G.GATHER_TILES and G.tile_ok(tile, "silu_mul"):
            N, T = n_for(tile, "silu_mul"), 150
            xs = rnd(gen, T, K)
            wg = rnd(gen, E, N, K, scale=0.05)
            src = torch.randint(0, T, (rows,), generator=gen).to(torch.int32).cuda()

            def gather(xs=xs, wg=wg, src=src, N=N, K=K):
                out = torch.full((rows, N // 2), float("nan"), dtype=torch.bfloat16, device=dev)
                ops._native_call("dli_gemm_grouped_gather", ops._p(xs), xs.stride(0), ops._p(wg),
                                 wg.stride(-2), ops._p(out), out.stride(0), rows, N, K, tile,
                                 ops._p(src), ops._p(off), E, ops._st())
                return out
            yield f"gather K={K} N={N}", gather


def rollup(lines):
    """One line per tile: how many cases, how many refused, SHA-256 over its case lines."""
    per = {}
    for ln in lines:
        per.setdefault(json.loads(ln)["tile"], []).append(ln)
    return [json.dumps({"tile": t, "cases": len(v), "refused": sum('"refused"' in x for x in v),
                        "sha256": hashlib.sha256("\n".join(v).encode()).hexdigest()})
            for t, v in sorted(per.items())]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", type=Path, help="one line per case")
    ap.add_argument("--rollup", type=Path, help="one line per tile")
    ap.add_argument("--from", dest="src", type=Path, help="roll up this case file, run nothing")
    a = ap.parse_args()
    if a.src:
        a.rollup.write_text("\n".join(rollup(a.src.read_text().splitlines())) + "\n")
        return
    lines = []
    for tile in sorted(G.TILES):
        for name, run in cases(tile):
            try:
                out = run()
            except RuntimeError as e:
                # a launcher refusing the case (hipErrorInvalidValue, before any launch) is
                # part of the record; anything else, a fault above all, ends the run
                if not str(e).endswith("failed with hipError 1"):
                    raise
                out = None
            digest = sha(out) if out is not None else "refused"
            lines.append(json.dumps({"tile": tile, "case": name, "sha256": digest}))
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text("\n".join(lines) + "\n")
    if a.rollup:
        a.rollup.write_text("\n".join(rollup(lines)) + "\n")
    print(f"{len(lines)} cases -> {a.out or a.rollup}")


if __name__ == "__main__":
    main()
