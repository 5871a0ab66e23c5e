#!/usr/bin/env python3
"""profiles/<round>_pmc_hbm.txt (tools/prof_summary.py pmc) -> profiles/wps_traffic.json: the HBM bytes per launch of the
step's dominant kernel, as MI355X_MICROARCH.md prescribes for gfx950 ((2 * FETCH_SIZE + WRITE_SIZE) * 1024 from two
separate --pmc passes).  bench.py reads the file for `roofline.traffic`.
usage: tools/traffic_json.py profiles/r3_a_pmc_hbm.txt [kernel=feat_then_wps_kernel] > profiles/wps_traffic.json"""
import json
import re
import sys

path = sys.argv[1]
kernel = sys.argv[2] if len(sys.argv) > 2 else "feat_then_wps_kernel"
per_step = int(sys.argv[3]) if len(sys.argv) > 3 else 24  # launches of the kernel in one step (one per contig)
build = sys.argv[4] if len(sys.argv) > 4 else "build not recorded"  # e.g. "r5_c, git 1a2b3c4"
vals, calls = {}, {}
for line in open(path):  # (fixed-width rows of tools/prof_summary.py: 70 characters of kernel name, then four fields)
    name, f = line[:70].rstrip(), line[70:].split()
    # the step's launch is the tabix-fetch variant <CHK, HIST, DF, BAM = false, [PACKED,] NT = true>: the FOURTH template
    # argument is false; the BAM-mode variant in the same file comes from tools/kernel_rows.py
    args = re.findall(r"true|false", name[len(kernel):]) if name.startswith(kernel + "<") else []
    if len(f) == 4 and len(args) >= 5 and args[3] == "false" and args[-1] == "true" and f[0] in ("FETCH_SIZE", "WRITE_SIZE"):
        vals[f[0]] = float(f[2])
        calls[f[0]] = int(f[1])
fetch, write = vals["FETCH_SIZE"], vals["WRITE_SIZE"]
per_launch = int((2 * fetch + write) * 1024)
print(json.dumps({
    "kernel": kernel, "source": path, "build": build, "workload": "whole-genome b37 30x, %d launches per step" % per_step,
    "dispatches_profiled": calls["FETCH_SIZE"],
    "fetch_size_kib_per_launch": round(fetch, 3), "write_size_kib_per_launch": round(write, 3),
    "hbm_bytes_per_launch": per_launch, "hbm_bytes_per_step": per_launch * per_step,
    "formula": "(2*FETCH_SIZE + WRITE_SIZE)*1024 (gfx950 FETCH_SIZE correction); separate --pmc passes",
    "note": "bench.py divides hbm_bytes_per_step by the launches of its own step"}, indent=1))
