"""Time and size of the fragment export (``utils.frag_export`` / ``ftk_frags_write``) against the two host yardsticks.

    python tools/export_bench.py [OUT_DIR] [--whitelist KIND] [--blacklist KIND] [--reps N]

Input: four synthetic contigs (chr19-22 sizes at 30x) as a fragment file; the export keeps ``mapq >= 30`` and
``120 <= length <= 180``.  Three repetitions after one warm-up of
  device   rows formatted and deflated on the GPU (per contig: HIP-event times of the format, deflate + CRC and
           compaction kernels, wall clock of the copy and the write)
  split    FTK_EXPORT_DEFLATE=host's path: formatter on the GPU, ``ftk_bgzf_write`` at level 1 on the host threads
  host     ``bgzf.write_frag_gz_contigs`` on the same kept columns (format + deflate on the host threads, level 1)
Writes ``export_times.txt`` and ``export_ratio.txt`` (device / host compressed size) into OUT_DIR (default
``profiles``); the BAM fixture's export is the second row of the ratio file.

With ``--whitelist`` / ``--blacklist`` (a BED file, or one of the synthetic kinds ``encode`` - about 900 regions of
0.2-5 kb over the four contigs -, ``dense`` - 10^5 intervals per contig covering about half of it -, ``global`` - a
period small enough that a tile of 1024 rows touches more intervals than the mask kernel stages in LDS) the device
leg alone is run, with the region masks in the keep rule (``ftk_frags_write_masked``), N repetitions (default 5) after
the warm-up, and ``filter_times_<tag>.txt`` is written instead: per contig the format stage (``stage_ms[0]``: mask
kernel + formatter) of every repetition.  Without them the tool behaves as before."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from finaletoolkit_amd import bgzf, source, synth, utils, writers  # noqa: E402

SCALE = (("chr19", 59_128_983), ("chr20", 63_025_520), ("chr21", 48_129_895), ("chr22", 51_304_566))
Q, LO, HI = 30, 120, 180


TIMES_HEAD = """\
# tools/export_bench.py on one MI355X: chr19-22 sizes at 30x, export of mapq >= 30, 120 <= length <= 180; three repetitions after a warm-up.
# device = ftk_frags_write (format, deflate + CRC, scan + compaction by HIP events; copy and write by wall clock).
# split  = FTK_EXPORT_DEFLATE=host's path: rows formatted on the GPU, ftk_bgzf_write (level 1, host threads) - in these rows the
#          'deflate+CRC' column is the text's device -> host copy and 'write' holds the host deflate and the file write.
# host   = bgzf.write_frag_gz_contigs on the kept host columns (the only way to write such a file before).
"""
RATIO_HEAD = ("# compressed size, device (ftk_fragtext.hip) / host (ftk_bgzf_write level 1), same text, same 0xFF00-byte blocks; "
              "tools/export_bench.py\n")


def synthetic_mask(kind, lds_intervals):
    """{contig: (starts, ends)} of one of the synthetic mask kinds."""
    out = {}
    for k, (n, size) in enumerate(SCALE):
        if kind == "encode":
            s, e = synth.synth_blacklist(size, 700 + k, 225)
        elif kind == "dense":
            period = size // 100_000
            s = np.arange(0, size - period, period, dtype=np.int64)
            e = s + period // 2
        elif kind == "global":  # a tile of 1024 rows spans about 10 kb at 30x: 4 intervals of the budget per kb
            period = max(10_000 // (4 * lds_intervals), 2)
            s = np.arange(0, size - period, period, dtype=np.int64)
            e = s + max(period // 2, 1)
        else:
            raise SystemExit(f"unknown mask kind {kind!r}")
        out[n] = utils.merge_intervals(s, e)
    return out


def masked_main(out_dir, whitelist, blacklist, reps):
    from finaletoolkit_amd.engine import RegionMask
    os.makedirs(out_dir, exist_ok=True)
    work = os.path.join(out_dir, "export_bench_work")
    os.makedirs(work, exist_ok=True)
    src = os.path.join(work, "in.frag.gz")
    bgzf.write_frag_gz_contigs(src, ((n, *synth.synth_contig(size, depth=30.0, seed=300 + k)) for k, (n, size) in enumerate(SCALE)),
                               level=1)
    eng = source.get_engine()
    feed = source.open_source(src)
    keys = {n: feed.require(n) for n, _ in SCALE}
    lds = eng.mask_lds_intervals()

    def load(spec):
        if spec is None or spec == "none":
            return None
        return utils.read_region_mask(spec) if os.path.exists(spec) else synthetic_mask(spec, lds)
    wl, bl = load(whitelist), load(blacklist)
    none = (np.zeros(0, np.int32), np.zeros(0, np.int32))
    tag = f"wl-{os.path.basename(whitelist or 'none')}_bl-{os.path.basename(blacklist or 'none')}"
    path = os.path.join(work, "masked.frag.gz")
    stage = {n: [] for n, _ in SCALE}
    lines = [f"# tools/export_bench.py --whitelist {whitelist} --blacklist {blacklist}: chr19-22 sizes at 30x, mapq >= {Q}, "
             f"{LO} <= length <= {HI}; {reps} repetitions after a warm-up; format = stage_ms[0] (mask kernel + formatter)"]
    for rep in range(reps + 1):
        for i, (n, _) in enumerate(SCALE):
            mask = None
            if wl is not None or bl is not None:
                mask = RegionMask(None if wl is None else wl.get(n, none), None if bl is None else bl.get(n), "midpoint")
            r = eng.write_contig(keys[n], n, path, Q, LO, HI, "frag", append=i > 0, write_eof=i == len(SCALE) - 1, mask=mask)
            if rep:
                stage[n].append((r["stage_ms"][0], r["rows"]))
    for n, _ in SCALE:
        iv = tuple(0 if m is None else len(m.get(n, none)[0]) for m in (wl, bl))
        us = [f"{ms * 1e3:.0f}" for ms, _ in stage[n]]
        lines.append(f"{n}: rows in {eng.info(keys[n])[0]}, kept {stage[n][0][1]}, intervals wl {iv[0]} bl {iv[1]}; format us: "
                     + " ".join(us) + f"  (min {min(ms for ms, _ in stage[n]) * 1e3:.0f}, max {max(ms for ms, _ in stage[n]) * 1e3:.0f})")
    with open(os.path.join(out_dir, f"filter_times_{tag}.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    for f in os.listdir(work):
        os.remove(os.path.join(work, f))
    os.rmdir(work)


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir", nargs="?", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--whitelist", default=None)
    ap.add_argument("--blacklist", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    out_dir = args.out_dir
    if args.whitelist is not None or args.blacklist is not None:
        return masked_main(out_dir, args.whitelist, args.blacklist, args.reps)
    os.makedirs(out_dir, exist_ok=True)
    work = os.path.join(out_dir, "export_bench_work")
    os.makedirs(work, exist_ok=True)
    src = os.path.join(work, "in.frag.gz")
    cols = {n: synth.synth_contig(size, depth=30.0, seed=300 + k) for k, (n, size) in enumerate(SCALE)}
    bgzf.write_frag_gz_contigs(src, ((n, *cols[n]) for n, _ in SCALE), level=1)
    kept = {}
    for n, _ in SCALE:
        s, e, q, st = cols[n]
        k = (q >= Q) & (e - s >= LO) & (e - s <= HI)
        kept[n] = (s[k], e[k], q[k], st[k])
    eng = source.get_engine()
    feed = source.open_source(src)
    keys = {n: feed.require(n) for n, _ in SCALE}
    lines, sizes = [], {}
    for mode, on_host in (("device", False), ("split", True)):
        path = os.path.join(work, mode + ".frag.gz")
        for rep in range(4):
            t0 = time.perf_counter()
            per = []
            for i, (n, _) in enumerate(SCALE):
                t1 = time.perf_counter()
                r = eng.write_contig(keys[n], n, path, Q, LO, HI, "frag", append=i > 0, write_eof=i == len(SCALE) - 1,
                                     deflate_on_host=on_host)
                per.append((n, r, time.perf_counter() - t1))
            wall = time.perf_counter() - t0
            if rep == 0:
                continue  # warm-up
            text = sum(r["text_bytes"] for _, r, _ in per)
            lines.append(f"{mode} rep {rep}: wall {wall * 1e3:.1f} ms, text {text / 1e9:.3f} GB = {text / wall / 1e9:.2f} GB/s in, "
                         f"{os.path.getsize(path) / wall / 1e9:.2f} GB/s out")
            for n, r, w in per:
                f, d, c, cp, wr = r["stage_ms"]
                gbs = r["text_bytes"] / 1e6 / d if d > 0 else 0.0
                lines.append(f"    {n}: rows {r['rows']} text {r['text_bytes']} B -> {r['end_off'] - r['first_off']} B; wall {w * 1e3:.1f} ms; "
                             f"format {f * 1e3:.0f} us, deflate+CRC {d * 1e3:.0f} us ({gbs:.1f} GB/s in), compact {c * 1e3:.0f} us, "
                             f"D2H {cp:.2f} ms, write {wr:.2f} ms")
        sizes[mode] = os.path.getsize(path)
    path = os.path.join(work, "host.frag.gz")
    for rep in range(4):
        t0 = time.perf_counter()
        bgzf.write_frag_gz_contigs(path, ((n, *kept[n]) for n, _ in SCALE), level=1, with_index=False)
        wall = time.perf_counter() - t0
        if rep:
            lines.append(f"host rep {rep}: wall {wall * 1e3:.1f} ms (format + deflate level 1 on the host threads)")
    sizes["host"] = os.path.getsize(path)
    ratio = [f"scale file (chr19-22 at 30x, q>=30, 120<=len<=180): device {sizes['device']} B, host level 1 {sizes['host']} B, "
             f"ratio {sizes['device'] / sizes['host']:.4f}"]
    bam = os.path.join(ROOT, "tests", "data", "12.3444.b37.bam")
    dev = os.path.join(work, "fixture.frag.gz")
    utils.frag_export(bam, dev, quality_threshold=0)
    text = __import__("gzip").open(dev, "rb").read()
    offs = writers.bgzf_write(os.path.join(work, "fixture_host.gz"), text, 1)
    ratio.append(f"fixture export (12.3444.b37.bam, q>=0): device {os.path.getsize(dev)} B, host level 1 {int(offs[-1]) + 28} B, "
                 f"ratio {os.path.getsize(dev) / (int(offs[-1]) + 28):.4f}")
    with open(os.path.join(out_dir, "export_times.txt"), "w") as fh:
        fh.write(TIMES_HEAD + "\n".join(lines) + "\n")
    with open(os.path.join(out_dir, "export_ratio.txt"), "w") as fh:
        fh.write(RATIO_HEAD + "\n".join(ratio) + "\n")
    print("\n".join(lines + ratio))
    for f in os.listdir(work):
        os.remove(os.path.join(work, f))
    os.rmdir(work)


if __name__ == "__main__":
    main()
