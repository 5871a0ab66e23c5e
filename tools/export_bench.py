"""Time and size of the fragment export (``utils.frag_export`` / ``ftk_frags_write``) against the two host yardsticks.

    python tools/export_bench.py [OUT_DIR]

Input: four synthetic contigs (chr19-22 sizes at 30x) as a fragment file; the export keeps ``mapq >= 30`` and
``120 <= length <= 180``.  Three repetitions after one warm-up of
  device   rows formatted and deflated on the GPU (per contig: HIP-event times of the format, deflate + CRC and
           compaction kernels, wall clock of the copy and the write)
  split    FTK_EXPORT_DEFLATE=host's path: formatter on the GPU, ``ftk_bgzf_write`` at level 1 on the host threads
  host     ``bgzf.write_frag_gz_contigs`` on the same kept columns (format + deflate on the host threads, level 1)
Writes ``export_times.txt`` and ``export_ratio.txt`` (device / host compressed size) into OUT_DIR (default
``profiles``); the BAM fixture's export is the second row of the ratio file."""
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


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
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
