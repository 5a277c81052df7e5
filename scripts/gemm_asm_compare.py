#!/usr/bin/env python3
"""Compare the generated device code of kernel files between two source trees.

Compiles the bf16 GEMM families (gemm_tiles.hip, gemm8p.hip, gemm4w.hip, gemm4wp.hip: the
default) or the ``--files`` of csrc/kernels named, in each tree, with build.py's kernel flags
plus ``--cuda-device-only -S`` (no GPU needed, about a minute per file). It splits the
assembly per kernel, strips comments / directives / metadata, maps kernel names whose
template parameters changed (``--map``), and reports per kernel ``identical`` or ``differs``
with the resource figures of both sides (VGPRs, AGPRs, SGPRs, scratch, LDS, instruction
count). It compares text and counts lines; it does not look at which instructions appear.

    python scripts/gemm_asm_compare.py BASE_TREE NEW_TREE [--md OUT.md] [--work DIR]
        [--map 'REGEX=REPLACEMENT' ...]      # applied to BASE's demangled kernel names; the
                                             # GEMM files' renames are built in
        [--files rope_cache.hip,...]         # any .hip files of csrc/kernels instead
        [--diff N]                           # N unified-diff lines per differing kernel

Exit status 1 if a kernel is missing on either side or a resource figure differs.
"""
import argparse
import concurrent.futures as cf
import difflib
import hashlib
import re
import shutil
import subprocess
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from distributed_llm_inferencing_amd.build import KERNEL_FLAGS, _hipcc  # noqa: E402

FILES = ("gemm_tiles.hip", "gemm8p.hip", "gemm4w.hip", "gemm4wp.hip")
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size",
          ".group_segment_fixed_size")
# the parent's VAR bit masks -> the named template parameters that replaced them
DEFAULT_MAPS = (r"gemm4w_kernel<(\d+), 8>=gemm4w_kernel<\1, false, false>",
                r"gemm4w_kernel<(\d+), 40>=gemm4w_kernel<\1, true, false>",
                r"gemm4w_kernel<(\d+), 4104>=gemm4w_kernel<\1, false, true>",
                r"gemm8p_kernel<(\d+), 776>=gemm8p_kernel<\1>")


def compile_asm(tree: Path, name: str, work: Path) -> Path:
    kdir = tree / "csrc" / "kernels"
    src = kdir / name
    h = hashlib.sha1(" ".join(KERNEL_FLAGS).encode())
    for p in [src, *sorted(kdir.glob("*.h"))]:
        h.update(p.read_bytes())
    out = work / f"{h.hexdigest()[:16]}_{src.stem}.s"
    if not out.exists():
        work.mkdir(parents=True, exist_ok=True)
        tmp = out.with_suffix(".tmp")
        subprocess.run([_hipcc(), *KERNEL_FLAGS, "-I", str(kdir), "--cuda-device-only", "-S",
                        str(src), "-o", str(tmp)], check=True, capture_output=True)
        tmp.rename(out)
    return out


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if filt is None:
        raise RuntimeError("no C++ demangler (llvm-cxxfilt / c++filt) on PATH")
    r = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True,
                       check=True)
    return dict(zip(names, r.stdout.splitlines()))


def parse(asm: Path) -> dict:
    """{demangled kernel name: (body lines, {field: value})} of one assembly file."""
    lines = asm.read_text().splitlines()
    meta, cur = {}, None
    for ln in lines:                                  # the amdhsa.kernels metadata records:
        m = re.match(r"  (- | {2})(\.[a-z_]+):\s*(\S+)$", ln)   # "  - .key: v" opens one,
        if not m:                                     # "    .key: v" belongs to it; the
            continue                                  # argument lists are indented deeper
        if m.group(1) == "- ":
            cur = {}
        if cur is not None:
            cur[m.group(2)] = m.group(3)
            if m.group(2) == ".name":
                meta[m.group(3)] = cur
    bodies, name, body = {}, None, []
    for ln in lines:
        m = re.match(r"(_Z\w+):\s*(;.*)?$", ln)
        if m and m.group(1) in meta:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        s = ln.split(";", 1)[0].strip()
        if s.startswith(".Lfunc_end"):
            bodies[name], name = body, None
            continue
        if not s or (s.startswith(".") and not s.endswith(":")):
            continue                                  # blank, comment or directive
        s = re.sub(r"\.LBB\d+_", ".LBB_", s).replace(name, "<self>")
        body.append(s)
    dm = demangle(sorted(bodies))
    out = {}
    for mangled, body in bodies.items():
        fields = {f: int(meta[mangled].get(f, "0")) for f in FIELDS}
        fields["instructions"] = sum(1 for s in body if not s.endswith(":"))
        out[kernel_name(dm[mangled])] = (body, fields)
    return out


def kernel_name(demangled: str) -> str:
    """``void f<2, (E)1>(int*)`` -> ``f<2, (E)1>``: cut at the argument list, which opens
    outside the template brackets (an enum argument has parentheses of its own)."""
    s, depth = re.sub(r"^void ", "", demangled), 0
    for i, ch in enumerate(s):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return s[:i]
    return s


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("base", type=Path)
    ap.add_argument("new", type=Path)
    ap.add_argument("--work", type=Path, default=Path("build") / "asm_compare")
    ap.add_argument("--md", type=Path, help="also write the table as markdown")
    ap.add_argument("--map", action="append", default=[])
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--files", default=",".join(FILES),
                    help="comma-separated .hip files of csrc/kernels")
    ap.add_argument("--diff", type=int, default=0, metavar="N",
                    help="print the first N unified-diff lines of each differing kernel")
    a = ap.parse_args()
    files = [f for f in a.files.split(",") if f]
    # the built-in renames belong to the GEMM families
    builtin = DEFAULT_MAPS if set(files) & set(FILES) else ()
    maps = [m.split("=", 1) for m in (*builtin, *a.map)]
    for f in files:
        for tree in (a.base, a.new):
            if not f.endswith(".hip") or not (tree / "csrc" / "kernels" / f).is_file():
                ap.error(f"--files: no {f} in {tree / 'csrc' / 'kernels'}")
    with cf.ThreadPoolExecutor(max_workers=a.j) as ex:
        futs = {(side, f): ex.submit(compile_asm, tree, f, a.work)
                for side, tree in (("base", a.base), ("new", a.new)) for f in files}
        asm = {k: v.result() for k, v in futs.items()}
    rows, bad, diffs = [], 0, []
    for f in files:
        base = {}
        for k, v in parse(asm[("base", f)]).items():
            for pat, rep in maps:
                k = re.sub(pat, rep, k)
            base[k] = v
        new = parse(asm[("new", f)])
        for k in sorted(set(base) | set(new)):
            if k not in base or k not in new:
                rows.append((f, k, "only in " + ("new" if k in new else "base"), "", ""))
                bad += 1
                continue
            (bb, bf), (nb, nf) = base[k], new[k]
            same = bb == nb
            if not same and a.diff:
                diffs += [f"--- {k}"] + list(difflib.unified_diff(bb, nb, lineterm="", n=2))[:a.diff]
            res_same = all(bf[x] == nf[x] for x in FIELDS)
            bad += not res_same
            fmt = lambda d: " / ".join(str(d[x]) for x in (*FIELDS, "instructions"))  # noqa: E731
            rows.append((f, k, "identical" if same else "differs", fmt(bf),
                         "=" if bf == nf else fmt(nf)))
    head = ("file", "kernel", "code", "base: vgpr / agpr / sgpr / scratch / LDS / instr", "new")
    table = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    table += ["| " + " | ".join(f"`{c}`" if i == 1 else c for i, c in enumerate(r)) + " |"
              for r in rows]
    n_same = sum(r[2] == "identical" for r in rows)
    table.append("")
    table.append(f"{len(rows)} kernels: {n_same} identical, {len(rows) - n_same} not; "
                 f"{bad} with a missing side or differing resources")
    print("\n".join(table + diffs))
    if a.md:
        a.md.write_text("\n".join(table) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
