#!/usr/bin/env python3
"""Two source trees' device code side by side: resource rows and instruction streams, kernel by kernel.

usage: tools/codegen_diff.py PARENT_TREE NEW_TREE [FILE.hip ...]      (default: ftk_kernels.hip)

Each file is compiled for gfx950 with the Makefile's flags (-S --cuda-device-only -Rpass-analysis=kernel-resource-usage).
Rows: VGPRs / SGPRs / scratch bytes per lane / LDS bytes per block / occupancy.  Instruction streams: the assembly of
each function with labels, comments and directives dropped.  Compiler outputs only: no GPU is involved."""
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-result", "--cuda-device-only", "-S",
         "-Rpass-analysis=kernel-resource-usage"]
KEYS = ["VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"]


def compile_tree(tree, src):
    """-> ({symbol: row string}, {symbol: [instruction, ...]}) of one file of one tree"""
    csrc = os.path.join(tree, "finaletoolkit_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, f"-I{tree}/include", f"-I{csrc}", os.path.join(csrc, src), "-o", out],
                           capture_output=True, text=True)
        if r.returncode:
            sys.exit(r.stderr)
        asm = open(out).read().splitlines()
    rows, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (.*) \[-Rpass", line)
        if not m:
            continue
        k, _, v = m.group(1).strip().partition(":")
        if k == "Function Name":
            cur = rows.setdefault(v.strip(), {})
        elif cur is not None:
            cur[k.strip()] = v.strip()
    rows = {s: "/".join(d.get(k, "?") for k in KEYS) for s, d in rows.items()}
    streams, name = {}, None
    for line in asm:
        m = re.match(r"(\w+):", line)
        if m and not line.startswith(".L"):
            name = m.group(1)
            streams[name] = []
        elif line.startswith(".Lfunc_end"):
            name = None
        elif name and line.startswith("\t") and not line.lstrip().startswith((".", ";")):
            ins = re.sub(r"\s+", " ", line.split(";")[0].strip())
            streams[name].append(re.sub(r"\.LBB\d+_\d+", ".LBB", ins))
    return rows, {s: v for s, v in streams.items() if v}


def main():
    parent, new = sys.argv[1], sys.argv[2]
    files = sys.argv[3:] or ["ftk_kernels.hip"]
    same, differ, only, table = 0, [], [], []
    for src in files:
        (r0, s0), (r1, s1) = compile_tree(parent, src), compile_tree(new, src)
        syms = sorted(set(s0) | set(s1))
        names = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.splitlines()
        for sym, name in zip(syms, names):
            if sym not in s0 or sym not in s1:
                only.append(f"{src}  {name}\n    only in the {'new tree' if sym in s1 else 'parent'}")
                continue
            row = r0.get(sym, "-") if r0.get(sym) == r1.get(sym) else f"{r0.get(sym, '-')} -> {r1.get(sym, '-')}"
            if sym in r0 or sym in r1:
                table.append(f"{src}  {name}  {row}")
            if s0[sym] == s1[sym] and r0.get(sym) == r1.get(sym):
                same += 1
            else:
                kind = "same instructions in another order or with other registers" if sorted(
                    re.sub(r"\b[svav]\d+\b|[svav]\[\d+:\d+\]", "r", i) for i in s0[sym]) == sorted(
                    re.sub(r"\b[svav]\d+\b|[svav]\[\d+:\d+\]", "r", i) for i in s1[sym]) else "other instructions"
                differ.append(f"{src}  {name}\n    differs ({len(s0[sym])} -> {len(s1[sym])} instructions, {kind}); rows {row}")
    print(f"Summary: {same + len(differ)} kernels and device functions in both trees; {same} identical; {len(differ)} differ; "
          f"{len(only)} in one tree only.")
    print("\n== Kernels and device functions in one tree only ==\n")
    print("\n\n".join(only) if only else "none")
    print("\n== Kernels whose instruction stream or row differs ==\n")
    print("\n\n".join(differ) if differ else "none")
    print("\n== Resource rows, every kernel ==\n")
    print("\n".join(table))


if __name__ == "__main__":
    main()
