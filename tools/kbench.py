#!/usr/bin/env python3
"""Kernel micro-bench on one synthetic contig (GPU box): times ftk_wps / window features with
HIP events, interleaved repetitions.  usage: tools/kbench.py [contig_len] [reps]
KBENCH=depth: the depth track (per base and run-length encoded) beside the cleavage profile of the same contig.
KBENCH=gcbias: the observed and the expected length x GC table (lengths 100-220) against a synthetic 2bit image.
KBENCH=gcweights: the GC weight column (lengths 100-220) and its sums per window beside ftk_window_counts on the same windows.
KBENCH=siteprofile: the midpoint profile of 10 000 sites (H = 990, b = 15) beside ftk_weighted_window_sums over the same sites x bins windows.
KBENCH=vplot: the length x offset map of the same sites (lengths 100-399 in 60 rows of 5) beside 60 calls of ftk_site_profile, one per row.
KBENCH=siteends: the U / D end profiles and per-site OCF window sums of the same sites beside ftk_site_profile, both LDS arrangements
of the widest weighted profile, and the route there was before (the columns to host memory + the rule in numpy).
KBENCH=spectrum: the WPS periodogram of 2 000 regions x 10 000 bases at periods 120-280 - the transform alone, the fused call, and
the route there was before (ftk_wps_intervals to host memory + a numpy matrix product on the host threads).
KBENCH=peaks: nucleosome calls on the same regions - the two peak passes alone on a resident adjusted track, ftk_wps_adjust on the
same runs, the fused call, and the route there was before (scores and adjusted track carried through host memory).
KBENCH=prefends: preferred ends of the whole contig at h = 500 and h = 2048, combined and split, beside ftk_depth_runs and
ftk_cleavage of the same region (the same tile skeleton), with the call's byte floor.
KBENCH=hotspots: IFS hotspots of the whole contig at the defaults (20-base step, 200-base windows, 5 kb / 10 kb backgrounds,
alpha = 1e-5) - the whole call, the totals reduction, the per-window track into device arrays - beside preferred ends combined
at h = 500 on the same contig, with the call's byte floor.
KBENCH=endcontext: the end-context table at W = 32 with the default length classes against the 2bit image of KBENCH=gcbias, in both
LDS arrangements (lanes are offsets / lanes are fragments), beside ftk_frag_gc_table on the same contig and image and beside the
route there was before: 64 calls of ftk_motif_counts, one per offset; and the background, ftk_ref_context of the whole image.
KBENCH=cofrag: the co-fragmentation map of the contig's first 2490 bins of 100 kb over lengths 0-1000 (run it on the chr1-sized
contig: `tools/kbench.py 249250621`) - ftk_hist_ks alone on resident histogram rows in both arrangements of the pair kernel
(a thread per pair / a workgroup per 64 x 64 tile), ftk_cofrag end to end, the histogram launch alone, and the numpy
restatement on this host at N = 500 (KBENCH_COFRAG_CPU=0 leaves it out)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from finaletoolkit_amd import synth  # noqa: E402
from finaletoolkit_amd.engine import Engine  # noqa: E402

size = int(sys.argv[1]) if len(sys.argv) > 1 else synth.B37_SIZES["2"]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dev = torch.device("cuda", 0)
eng = Engine(0)
_stream = torch.cuda.Stream()  # one explicit stream for torch ops and ftk launches (handle 0 = "own stream")
torch.cuda.set_stream(_stream)
eng.set_stream(_stream.cuda_stream)
DEPTH = float(os.environ.get("KBENCH_DEPTH", "30"))
BAM = os.environ.get("KBENCH_BAM", "0") != "0"   # read1 columns beside the fragments: the BAM fetch rule (io/alignment.py:245)
n = synth.n_fragments(size, DEPTH)
s, e, q, st = bench.gen_contig_device(torch, dev, size, n, 1)
torch.cuda.synchronize()
eng.load_contig_device("c", s, e, q, st, n)
FRAG_BYTES = 10
if BAM:
    e = torch.maximum(e, s + 50)
    eng.load_contig_device("c", s, e, q, st, n)
    r1s = torch.where(st == 1, s, e - 50).to(torch.int32).contiguous()
    r1e = (r1s + 50).contiguous()
    torch.cuda.synchronize()
    eng.set_read1("c", r1s, r1e, n)
    FRAG_BYTES = 18  # +8 B per fragment for the read1 columns
    print(f"BAM contig: {n} fragments at {DEPTH}x, read1 columns resident; is_bam={eng.is_bam('c')}", flush=True)
ws, we = synth.tiling_windows(size, 100_000)
d_ws, d_we = torch.from_numpy(ws).to(dev), torch.from_numpy(we).to(dev)
out = torch.empty(size, dtype=torch.int64, device=dev)
cov = torch.zeros(len(ws), dtype=torch.int64, device=dev)
hist = torch.zeros((len(ws), 1001), dtype=torch.int32, device=dev)
over = torch.zeros(len(ws), dtype=torch.int64, device=dev)


flush_buf = torch.empty(160_000_000, dtype=torch.int32, device=dev)  # 640 MB > Infinity Cache


def timeit(fn, name, nbytes, cold=False):
    fn()
    torch.cuda.synchronize()
    ts = []
    if cold == "chain":  # 10 launches back to back between two events: no idle gap in which host preparation would count
        for _ in range(reps):
            flush_buf[:16_000_000].sum()  # keeps the GPU busy while the first launch is being prepared
            eng.event_record(0)
            for _ in range(10):
                fn()
            eng.event_record(1)
            ts.append(eng.event_elapsed_ms(0, 1) / 10)
        ts = np.array(ts)
        print(f"{name:28s} median {np.median(ts)*1e3:9.1f} us  min {ts.min()*1e3:9.1f} us   "
              f"{nbytes/np.median(ts)/1e6:8.1f} GB/s (median)  {nbytes/ts.min()/1e6:8.1f} GB/s (best)", flush=True)
        return
    for _ in range(reps):
        if cold == "read":
            flush_buf.sum()      # evict with clean lines
        elif cold:
            flush_buf.fill_(1)  # evict the contig from the 256 MiB Infinity Cache (dirty lines)
        eng.event_record(0)
        fn()
        eng.event_record(1)
        ts.append(eng.event_elapsed_ms(0, 1))
    ts = np.array(ts)
    print(f"{name:28s} median {np.median(ts)*1e3:9.1f} us  min {ts.min()*1e3:9.1f} us   "
          f"{nbytes/np.median(ts)/1e6:8.1f} GB/s (median)  {nbytes/ts.min()/1e6:8.1f} GB/s (best)", flush=True)


which = os.environ.get("KBENCH", "wps,cov,hist").split(",")
if "cal" in which:
    src = torch.ones(size, dtype=torch.int64, device=dev)
    timeit(lambda: out.fill_(7), "torch fill int64", 8 * size)
    timeit(lambda: out.copy_(src), "torch copy int64 (r+w)", 16 * size)
    del src
if "wps" in which:
    timeit(lambda: eng.wps("c", 0, size, size, 120, 120, 180, 30, out=out), "wps W=120 120-180", FRAG_BYTES * n + 8 * size)
if "merged" in which:
    # the step's launch: feature blocks (coverage + 1001-bin histogram + DELFI with blacklist and gaps) first, WPS tiles behind
    bl_s, bl_e = bench.synth_blacklist(size, 5, 160)
    sh = torch.zeros(len(ws), dtype=torch.int64, device=dev)
    lg = torch.zeros(len(ws), dtype=torch.int64, device=dev)
    gp = bench.synth_gaps(size)
    f = lambda: eng.window_features_wps("c", ws, we, out, 0, size, size, coverage=cov, hist=hist, hist_bins=(0, 1001),
                                        overflow=over, delfi_q=30, bl_start=bl_s, bl_end=bl_e, gaps=gp, short=sh, long=lg)
    nb = 2 * FRAG_BYTES * n + 8 * size + len(ws) * (1001 * 4 + 32)
    timeit(f, "features + WPS, one launch", nb)
    timeit(f, "features + WPS x10 chained", nb, cold="chain")
if "rd" in which:
    big = torch.ones(60_000_000, dtype=torch.int32, device=dev)  # 240 MB
    timeit(lambda: big.sum(), "torch sum 240MB warm", 240e6)
    timeit(lambda: big.sum(), "torch sum 240MB COLD", 240e6, cold=True)
    timeit(lambda: flush_buf.sum(), "torch sum 640MB (always cold)", 640e6)
    del big
if "cov" in which:
    timeit(lambda: eng.window_counts("c", d_ws, d_we, 30, out=cov), "window_counts 100kb", 10 * n)
    timeit(lambda: eng.window_counts("c", d_ws, d_we, 30, out=cov), "window_counts 100kb COLD", 10 * n, cold=True)
    timeit(lambda: eng.window_counts("c", d_ws, d_we, 30, out=cov), "window_counts COLD(read-flush)", 10 * n, cold="read")
if "hist" in which:
    import ctypes as C
    from finaletoolkit_amd import _lib as L
    flt = L.make_filter(30, None, None, "midpoint")
    timeit(lambda: eng._check(eng.lib.ftk_fraglen_hist(eng.ctx, eng.contig_id("c"), L.ptr(d_ws), L.ptr(d_we), len(ws),
                                                       C.byref(flt), 0, 1001, L.ptr(hist), L.ptr(over))),
           "fraglen_hist 100kb x1001", 10 * n)
    timeit(lambda: eng._check(eng.lib.ftk_fraglen_hist(eng.ctx, eng.contig_id("c"), L.ptr(d_ws), L.ptr(d_we), len(ws),
                                                       C.byref(flt), 0, 1001, L.ptr(hist), L.ptr(over))),
           "fraglen_hist COLD", 10 * n, cold=True)
if "feat" in which:
    import ctypes as C
    from finaletoolkit_amd import _lib as L
    flt = L.make_filter(30, None, None, "midpoint", L.FETCH_BAM_READ1 if BAM else L.FETCH_TABIX)
    sh = torch.zeros(len(ws), dtype=torch.int64, device=dev)
    lg = torch.zeros(len(ws), dtype=torch.int64, device=dev)
    bl_s, bl_e = bench.synth_blacklist(size, 5, 160)
    g = L.make_gaps(bench.synth_gaps(size))

    def fused(cov_on=True, hist_on=True, delfi_on=True):
        eng._check(eng.lib.ftk_window_features(
            eng.ctx, eng.contig_id("c"), L.ptr(ws), L.ptr(we), len(ws), C.byref(flt), L.ptr(cov) if cov_on else None,
            0, 1001, L.ptr(hist) if hist_on else None, L.ptr(over) if hist_on else None, 30, L.ptr(bl_s), L.ptr(bl_e),
            len(bl_s), C.byref(g), L.ptr(sh) if delfi_on else None, L.ptr(lg) if delfi_on else None))
    for name, kw in [("cov", dict(hist_on=False, delfi_on=False)), ("cov+hist", dict(delfi_on=False)),
                     ("delfi", dict(cov_on=False, hist_on=False)), ("cov+hist+delfi", {})]:
        timeit(lambda: fused(**kw), "fused " + name + " x10 chained", FRAG_BYTES * n, cold="chain")
        timeit(lambda: fused(**kw), "fused " + name + " COLD(read)", FRAG_BYTES * n, cold="read")
        timeit(lambda: fused(**kw), "fused " + name + " COLD(dirty)", FRAG_BYTES * n, cold=True)
if "cleave" in which:
    # whole-contig cleavage profile into a device buffer (float64 per base, like WPS's int64)
    import ctypes as C
    from finaletoolkit_amd import _lib as L
    cl = torch.empty(size, dtype=torch.float64, device=dev)
    s0 = np.array([0], np.int64); s1 = np.array([size], np.int64); so = np.array([0], np.int64)
    f = lambda: eng._check(eng.lib.ftk_cleavage_intervals(eng.ctx, eng.contig_id("c"), L.ptr(s0), L.ptr(s1), 1, L.ptr(so),
                                                          L.LEN_OPEN, L.LEN_OPEN, 20, L.ptr(cl)))
    timeit(f, "cleavage whole contig", 10 * n + 8 * size)
if "depth" in which:
    # Depth track of the whole contig: per base into a device buffer (the launch alone), and as runs (the whole call: two
    # tile passes, the scan between them, the 8-byte run count read back and the three run columns copied to the host).
    # Algorithmic bytes: 9 B (start, end, mapq) per candidate of every tile - the fragments the position index hands the
    # tile, counted here from the sorted starts - plus 4 B per base, or 12 B per run.
    import ctypes as C
    from finaletoolkit_amd import _lib as L
    lmax = eng.info("c")[1]
    hs = s.cpu().numpy().astype(np.int64)
    t0 = np.arange(0, size, 4096, dtype=np.int64)
    t1 = np.minimum(t0 + 4096, size)
    lo = np.searchsorted(hs, (np.maximum(t0 - lmax, 0) >> 9) << 9, side="left")
    hi = np.searchsorted(hs, ((t1 >> 9) + 1) << 9, side="left")
    cand = int((hi - lo).sum())
    dp = torch.empty(size, dtype=torch.int32, device=dev)
    cl = torch.empty(size, dtype=torch.float64, device=dev)
    runs = {}

    def run_form(include_zero):
        runs[include_zero] = len(eng.depth_runs("c", 0, size, 30, None, None, include_zero)[0])
    run_form(False)
    run_form(True)
    print(f"depth: {n} fragments, {len(t0)} tiles, {cand} candidates ({cand / n:.2f} per fragment), runs {runs[False]} "
          f"(with zero runs {runs[True]})", flush=True)
    for _ in range(2):  # twice, interleaved with the comparison: the spread between the two passes is the noise
        timeit(lambda: eng.depth("c", 0, size, 30, out=dp), "depth per base", 9 * cand + 4 * size)
        timeit(lambda: run_form(False), "depth runs (whole call)", 2 * 9 * cand + 12 * runs[False])
        timeit(lambda: run_form(True), "depth runs, include_zero", 2 * 9 * cand + 12 * runs[True])
        timeit(lambda: eng.cleavage("c", 0, size, None, None, 30, out=cl), "cleavage (comparison)", 10 * cand + 8 * size)
    print("depth checksum", int(dp.sum(dtype=torch.int64).item()), "max", int(dp.max().item()))
if "gcbias" in which:
    # Length x GC tables, lengths 100-220, against a random 2bit image of the contig with one N block: the whole calls
    # (table zeroed, kernel, 214 KB table copied to the host).  Byte floors: observed = 9 B of columns (start, end, mapq)
    # per fragment + the image once; expected = the image once (at any stride: every base is part of some window).
    rng = np.random.default_rng(7)
    packed = rng.integers(0, 256, (size + 3) // 4, dtype=np.uint8)
    ridb = eng.ref_upload(("kb", "gcbias2bit"), packed, 1)
    eng.ref_set_layout(ridb, size, 0, 0, [10_000_000], [10_050_000])
    img = (size + 3) // 4
    obs, skipped = eng.frag_gc_table("c", ridb, 100, 220, 30)
    print(f"gcbias: {n} fragments, {int(obs.sum())} counted, {skipped} skipped, image {img} B", flush=True)
    for _ in range(2):  # twice: the spread between the two passes is the noise
        timeit(lambda: eng.frag_gc_table("c", ridb, 100, 220, 30), "observed table 100-220", 9 * n + img)
        timeit(lambda: eng.ref_gc_table(ridb, 0, size, 100, 220, 1), "expected table, stride 1", img)
        timeit(lambda: eng.ref_gc_table(ridb, 0, size, 100, 220, 16), "expected table, stride 16", img)
    exp = eng.ref_gc_table(ridb, 0, size, 100, 220, 16)
    print("gcbias checksum", int(obs.sum()), int(exp.sum()), "(share of the byte floor = GB/s above / the HBM rate)")
if "gcweights" in which:
    # GC weights, lengths 100-220, against the 2bit image of KBENCH=gcbias: the weights call (table packed and uploaded,
    # kernel, the 8-byte count read back), then the weighted sums and, on the same windows in the same run, the window
    # counts that are their yardstick - over the 100 kb tiling and over one whole-contig window, outputs on the device.
    # Byte floors: weights = 9 B read (start, end, mapq) + 4 B written per fragment + the image once; sums = 13 B (start,
    # end, mapq, weight) per candidate - the fragments the position index hands each window, counted here from the
    # sorted starts; counts = 9 B per candidate.
    rng = np.random.default_rng(7)
    packed = rng.integers(0, 256, (size + 3) // 4, dtype=np.uint8)
    ridw = eng.ref_upload(("kb", "gcbias2bit"), packed, 1)
    eng.ref_set_layout(ridw, size, 0, 0, [10_000_000], [10_050_000])
    img = (size + 3) // 4
    table = rng.integers(1, 1 << 20, (121, 221), dtype=np.int64).astype(np.uint32)
    lmax = eng.info("c")[1]
    hs = s.cpu().numpy().astype(np.int64)
    lo = np.searchsorted(hs, (np.maximum(ws.astype(np.int64) - lmax, 0) >> 9) << 9, side="left")
    hi = np.searchsorted(hs, ((we.astype(np.int64) >> 9) + 1) << 9, side="left")
    cand = int((hi - lo).sum())
    one_lo, one_hi = np.array([0], np.int32), np.array([size], np.int32)
    import ctypes as C
    from finaletoolkit_amd import _lib as L
    flt = L.make_filter(30, None, None, "midpoint")
    d_sum = torch.zeros(len(ws), dtype=torch.int64, device=dev)
    d_cnt = torch.zeros(len(ws), dtype=torch.int64, device=dev)

    def sums(a, b):
        eng._check(eng.lib.ftk_weighted_window_sums(eng.ctx, eng.contig_id("c"), L.ptr(a), L.ptr(b), len(a), C.byref(flt),
                                                    L.ptr(d_sum), L.ptr(d_cnt)))
    n_zero = eng.set_gc_weights("c", ridw, 100, 220, table, 30)
    print(f"gcweights: {n} fragments, {n_zero} of weight 0, {len(ws)} windows with {cand} candidates ({cand / n:.2f} per "
          f"fragment), image {img} B", flush=True)
    for _ in range(2):  # twice: the spread between the two passes is the noise
        timeit(lambda: eng.set_gc_weights("c", ridw, 100, 220, table, 30), "gc weights 100-220", 13 * n + img)
        timeit(lambda: sums(ws, we), "weighted sums 100kb", 13 * cand)
        timeit(lambda: eng.window_counts("c", ws, we, 30, out=cov), "window_counts 100kb", 9 * cand)
        timeit(lambda: sums(one_lo, one_hi), "weighted sums one window", 13 * n)
        timeit(lambda: eng.window_counts("c", one_lo, one_hi, 30, out=cov[:1]), "window_counts one window", 9 * n)
    sums(ws, we)
    print("gcweights checksum", int(d_sum.sum().item()), int(d_cnt.sum().item()), "counts", int(eng.window_counts("c", ws, we, 30).sum()))
if "siteprofile" in which:
    # Site profile: 10 000 random sites, H = 990, b = 15 (132 bins), one group, unweighted and weighted, outputs on the
    # device - the whole call (sites sorted and cut into runs on the host, three small uploads, the kernel, one wait).
    # Beside it the only route there was before: ftk_weighted_window_sums over the same n_sites x n_bins windows, whose
    # per-window sums, added up over the sites, are the same profile (the checksum line).  Byte floors: 9 B (start, end,
    # mapq) per candidate - the fragments the position index hands each site, counted here from the sorted starts -
    # and 13 B with the weight; the windows route reads 13 B per candidate of every one of its windows.  The sites reach
    # a few tens of MB of the columns, so repeated calls find them in the Infinity Cache: the COLD lines evict first.
    import ctypes as C
    from finaletoolkit_amd import _lib as L
    rng = np.random.default_rng(11)
    H, B, NS = 990, 15, 10_000
    nb = 2 * H // B
    centres = rng.integers(H, size - H, NS).astype(np.int32)
    eng.set_weights("c", rng.integers(1, 1 << 20, n, dtype=np.int64).astype(np.uint32))
    lmax = eng.info("c")[1]
    hs = s.cpu().numpy().astype(np.int64)
    c64 = centres.astype(np.int64)
    cand = int((np.searchsorted(hs, ((c64 + H >> 9) + 1) << 9, side="left")
                - np.searchsorted(hs, (np.maximum(c64 - H - lmax, 0) >> 9) << 9, side="left")).sum())
    w_lo = (c64[:, None] - H + B * np.arange(nb)[None, :]).reshape(-1)
    w_cand = int((np.searchsorted(hs, ((w_lo + B >> 9) + 1) << 9, side="left")
                  - np.searchsorted(hs, (np.maximum(w_lo - lmax, 0) >> 9) << 9, side="left")).sum())
    w_lo32, w_hi32 = w_lo.astype(np.int32), (w_lo + B).astype(np.int32)
    d_psum = torch.zeros(nb, dtype=torch.int64, device=dev)
    d_pcnt = torch.zeros(nb, dtype=torch.int64, device=dev)
    d_wsum = torch.zeros(NS * nb, dtype=torch.int64, device=dev)
    d_wcnt = torch.zeros(NS * nb, dtype=torch.int64, device=dev)
    flt = L.make_filter(30, None, None, "midpoint")

    def profile(weighted):
        eng._check(eng.lib.ftk_site_profile(eng.ctx, eng.contig_id("c"), L.ptr(centres), None, None, NS, 1, H, B, 30, -1, -1,
                                            int(weighted), L.ptr(d_psum), L.ptr(d_pcnt)))

    def windows():
        eng._check(eng.lib.ftk_weighted_window_sums(eng.ctx, eng.contig_id("c"), L.ptr(w_lo32), L.ptr(w_hi32), NS * nb, C.byref(flt),
                                                    L.ptr(d_wsum), L.ptr(d_wcnt)))
    print(f"siteprofile: {n} fragments, {NS} sites x {nb} bins, {cand} candidates ({cand / NS:.0f} per site); the windows route: "
          f"{NS * nb} windows, {w_cand} candidates", flush=True)
    for _ in range(2):  # twice: the spread between the two passes is the noise
        timeit(lambda: profile(False), "site profile, unweighted", 9 * cand)
        timeit(lambda: profile(True), "site profile, weighted", 13 * cand)
        timeit(lambda: windows(), "weighted sums, sites x bins", 13 * w_cand)
        timeit(lambda: profile(False), "site profile, unweighted COLD", 9 * cand, cold="read")
        timeit(lambda: profile(True), "site profile, weighted COLD", 13 * cand, cold="read")
        timeit(lambda: windows(), "weighted sums, s x b COLD", 13 * w_cand, cold="read")
    profile(True)
    windows()
    torch.cuda.synchronize()
    route = d_wsum.view(NS, nb).sum(0)
    print("siteprofile checksum", int(d_psum.sum().item()), int(route.sum().item()), "bins equal", bool(torch.equal(d_psum, route)),
          "midpoints", int(d_pcnt.sum().item()))
if "vplot" in which:
    # V-plot: the siteprofile mode's contig and sites (KBENCH_VPLOT_SITES of them, 10 000 by default; KBENCH_VPLOT_ROWS=0
    # leaves the rows route out, for experiments with many sites), H = 990, b = 15
    # (132 bins), lengths 100-399 in 5-bp rows (60 rows), one group, unweighted and weighted, outputs on the device - the
    # whole call.  Beside it the only route there was before: one ftk_site_profile call per row with that row's min_len /
    # max_len, 60 calls, each sorting and uploading the sites again and reading every candidate again.  Byte floors: 9 B
    # (13 B weighted) per candidate of ONE pass over the sites - the fragments the position index hands each site with
    # the call's longest passing length; the matrix reads them once per tile of rows, the rows route once per row.
    import ctypes as C
    from finaletoolkit_amd import _lib as L
    rng = np.random.default_rng(11)
    H, B, NS = 990, 15, int(os.environ.get("KBENCH_VPLOT_SITES", "10000"))
    LO, HI, LB = 100, 399, 5
    nb, nr = 2 * H // B, (HI - LO + 1) // LB
    centres = rng.integers(H, size - H, NS).astype(np.int32)
    eng.set_weights("c", rng.integers(1, 1 << 20, n, dtype=np.int64).astype(np.uint32))
    lmax = min(eng.info("c")[1], HI)
    hs = s.cpu().numpy().astype(np.int64)
    c64 = centres.astype(np.int64)
    cand = int((np.searchsorted(hs, ((c64 + H >> 9) + 1) << 9, side="left")
                - np.searchsorted(hs, (np.maximum(c64 - H - lmax, 0) >> 9) << 9, side="left")).sum())
    d_vsum = torch.zeros(nr * nb, dtype=torch.int64, device=dev)
    d_vcnt = torch.zeros(nr * nb, dtype=torch.int64, device=dev)
    d_rsum = torch.zeros(nr * nb, dtype=torch.int64, device=dev)
    d_rcnt = torch.zeros(nr * nb, dtype=torch.int64, device=dev)
    cid = eng.contig_id("c")
    ROWS = os.environ.get("KBENCH_VPLOT_ROWS", "1") != "0"

    def vplot(weighted):
        eng._check(eng.lib.ftk_site_vplot(eng.ctx, cid, L.ptr(centres), None, None, NS, 1, H, B, LO, HI, LB, 30, int(weighted),
                                          L.ptr(d_vsum), L.ptr(d_vcnt)))

    def rows(weighted):
        for r in range(nr):
            eng._check(eng.lib.ftk_site_profile(eng.ctx, cid, L.ptr(centres), None, None, NS, 1, H, B, 30, LO + r * LB, LO + (r + 1) * LB - 1,
                                                int(weighted), d_rsum.data_ptr() + r * nb * 8, d_rcnt.data_ptr() + r * nb * 8))
    print(f"vplot: {n} fragments, {NS} sites x {nr} rows x {nb} bins, {cand} candidates per pass ({cand / NS:.0f} per site); "
          f"the rows route: {nr} calls of ftk_site_profile", flush=True)
    for _ in range(2):  # twice: the spread between the two passes is the noise
        timeit(lambda: vplot(False), "vplot, unweighted", 9 * cand)
        timeit(lambda: vplot(True), "vplot, weighted", 13 * cand)
        timeit(lambda: vplot(False), "vplot, unweighted COLD", 9 * cand, cold="read")
        timeit(lambda: vplot(True), "vplot, weighted COLD", 13 * cand, cold="read")
        if ROWS:
            timeit(lambda: rows(False), "60 profiles, unweighted", 9 * cand)
            timeit(lambda: rows(True), "60 profiles, weighted", 13 * cand)
            timeit(lambda: rows(False), "60 profiles, unw. COLD", 9 * cand, cold="read")
            timeit(lambda: rows(True), "60 profiles, weighted COLD", 13 * cand, cold="read")
    for weighted in (False, True) if ROWS else ():
        vplot(weighted)
        rows(weighted)
        torch.cuda.synchronize()
        print("vplot checksum", "weighted" if weighted else "unweighted", int(d_vsum.sum().item()), int(d_rsum.sum().item()),
              "stacked profiles equal the matrix", bool(torch.equal(d_vsum, d_rsum) and torch.equal(d_vcnt, d_rcnt)),
              "midpoints", int(d_vcnt.sum().item()))
if "siteends" in which:
    # Site ends: the siteprofile mode's contig and sites (10 000 random sites, H = 990, b = 15, one group), the whole
    # call with outputs on the device: unweighted and weighted, with and without the per-site window sums (peak 60, flank
    # 10), beside ftk_site_profile over the same sites - the same candidates, half the LDS atomics.  Then the widest
    # weighted profile (H = 2048, b = 1: 4096 bins x 2 tracks x 12 B = 96 KiB of LDS) in both arrangements: one
    # workgroup per run (FTK_SITE_ENDS_SPLIT=0), and one per (run, track) (=1), which reads the candidates twice.  Last, by
    # the wall clock, the only route there was before: the three columns to host memory and the rule in numpy, site by
    # site (KBENCH_SITEENDS_HOST=0 leaves it out).  Byte floors as in the siteprofile mode: 9 B (13 B weighted) per
    # candidate.
    import time
    from finaletoolkit_amd import _lib as L
    rng = np.random.default_rng(11)
    H, B, NS, PEAK, FLANK = 990, 15, 10_000, 60, 10
    nb = 2 * H // B
    centres = rng.integers(H, size - H, NS).astype(np.int32)
    flips = rng.integers(0, 2, NS).astype(np.uint8)
    eng.set_weights("c", rng.integers(1, 1 << 20, n, dtype=np.int64).astype(np.uint32))
    lmax = eng.info("c")[1]
    hs = s.cpu().numpy().astype(np.int64)
    c64 = centres.astype(np.int64)

    def candidates(h):
        return int((np.searchsorted(hs, ((c64 + h >> 9) + 1) << 9, side="left")
                    - np.searchsorted(hs, (np.maximum(c64 - h - lmax, 0) >> 9) << 9, side="left")).sum())
    cand = candidates(H)
    d_esum = torch.zeros(2 * 4096, dtype=torch.int64, device=dev)
    d_ecnt = torch.zeros(2 * 4096, dtype=torch.int64, device=dev)
    d_ssum = torch.zeros(NS * 4, dtype=torch.int64, device=dev)
    d_scnt = torch.zeros(NS * 4, dtype=torch.int64, device=dev)
    d_psum = torch.zeros(nb, dtype=torch.int64, device=dev)
    d_pcnt = torch.zeros(nb, dtype=torch.int64, device=dev)
    cid = eng.contig_id("c")

    def ends(weighted, per_site, h=H, b=B):
        eng._check(eng.lib.ftk_site_ends(eng.ctx, cid, L.ptr(centres), L.ptr(flips), None, NS, 1, h, b, 30, -1, -1, int(weighted), PEAK,
                                         FLANK, L.ptr(d_esum), L.ptr(d_ecnt), L.ptr(d_ssum) if per_site else None,
                                         L.ptr(d_scnt) if per_site else None))

    def profile(weighted):
        eng._check(eng.lib.ftk_site_profile(eng.ctx, cid, L.ptr(centres), L.ptr(flips), None, NS, 1, H, B, 30, -1, -1, int(weighted),
                                            L.ptr(d_psum), L.ptr(d_pcnt)))
    print(f"siteends: {n} fragments, {NS} sites x 2 tracks x {nb} bins, {cand} candidates ({cand / NS:.0f} per site)", flush=True)
    for _ in range(2):  # twice: the spread between the two passes is the noise
        for weighted, nbytes in ((False, 9), (True, 13)):
            tag = "weighted" if weighted else "unweighted"
            timeit(lambda: ends(weighted, False), f"site ends, {tag}", nbytes * cand)
            timeit(lambda: ends(weighted, True), f"site ends + sites, {tag}", nbytes * cand)
            timeit(lambda: profile(weighted), f"site profile, {tag}", nbytes * cand)
        for weighted, nbytes in ((False, 9), (True, 13)):
            tag = "weigh." if weighted else "unw."
            timeit(lambda: ends(weighted, False), f"site ends, {tag} COLD", nbytes * cand, cold="read")
            timeit(lambda: ends(weighted, True), f"site ends + sites, {tag} COLD", nbytes * cand, cold="read")
            timeit(lambda: profile(weighted), f"site profile, {tag} COLD", nbytes * cand, cold="read")
    wide = candidates(2048)
    print(f"siteends: 4096 bins, weighted, {wide} candidates per pass", flush=True)
    for _ in range(2):
        for split in ("0", "1"):
            os.environ["FTK_SITE_ENDS_SPLIT"] = split
            tag = "2 x 48 KiB" if split == "1" else "1 x 96 KiB"
            timeit(lambda: ends(True, True, 2048, 1), f"4096 bins {tag}", 13 * wide)
            timeit(lambda: ends(True, True, 2048, 1), f"4096 bins {tag} COLD", 13 * wide, cold="read")
    del os.environ["FTK_SITE_ENDS_SPLIT"]
    for weighted in (False, True):
        ends(weighted, True)
        torch.cuda.synchronize()
        ocf = (d_ssum.view(NS, 4) * torch.tensor([-1, 1, 1, -1], device=dev)).sum()
        print("siteends checksum", "weighted" if weighted else "unweighted", int(d_esum[:2 * nb].sum().item()), "ends",
              int(d_ecnt[:2 * nb].sum().item()),
              "window ends", int(d_scnt.sum().item()), "ocf units", int(ocf.item()))
    if os.environ.get("KBENCH_SITEENDS_HOST", "1") != "0":
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            fs, fe, fq = (x.cpu().numpy() for x in (s, e, q))  # the columns to host memory
            fs, fe = fs[:n].astype(np.int64), fe[:n].astype(np.int64)
            keep = (fq[:n] >= 30) & (fe > fs)
            counts, windows = np.zeros(2 * nb, np.int64), np.zeros((NS, 4), np.int64)
            for kind, x in enumerate((np.sort(fs[keep]), np.sort(fe[keep] - 1))):
                lo_i, hi_i = np.searchsorted(x, c64 - H), np.searchsorted(x, c64 + H)
                for c, f, lo, hi in zip(c64.tolist(), flips.tolist(), lo_i.tolist(), hi_i.tolist()):
                    k = (x[lo:hi] - c + H) // B
                    counts += np.bincount((1 - kind) * nb + nb - 1 - k if f else kind * nb + k, minlength=2 * nb)
                for side, mid in enumerate((c64 - PEAK, c64 + PEAK)):
                    windows[:, 2 * side + kind] = np.searchsorted(x, mid + FLANK, "right") - np.searchsorted(x, mid - FLANK, "left")
            ts.append(time.perf_counter() - t0)
        ends(False, True)
        torch.cuda.synchronize()
        print(f"host route (columns to host + numpy), unweighted: median {np.median(ts) * 1e3:.1f} ms  min {min(ts) * 1e3:.1f} ms; "
              f"equal to the call: {bool(np.array_equal(counts, d_ecnt[:2 * nb].cpu().numpy()))} "
              f"{bool(np.array_equal(windows, d_scnt.view(NS, 4).cpu().numpy()))}", flush=True)
if "spectrum" in which:
    # WPS periodogram: KBENCH_SPECTRUM_REGIONS regions (2 000) of 10 000 bases spread over the contig, periods 120-280.
    # Three times, wall clock around the whole call (the host route has no device events to offer): (a) the transform
    # alone - scores already on the device, (re, im) left there; (b) the fused call, results in host memory; (c) today's
    # route - ftk_wps_intervals to host memory, then mean, bell and x @ [cos | sin] in numpy on the host's BLAS threads.
    # Roofs of the DIRECT form for the same (sample, period) pairs: 2 float64 FMAs per pair at 39.3e12 FMA/s (78.6 TFLOP/s),
    # one 16-byte twiddle per pair out of LDS at 150 TB/s.  The kernel folds instead (one add and 8 bytes per pair).
    import time
    from finaletoolkit_amd import _lib as L
    rng = np.random.default_rng(193)
    NR, NB = int(os.environ.get("KBENCH_SPECTRUM_REGIONS", "2000")), 10_000
    periods = np.arange(120, 281, dtype=np.int32)
    r_start = np.sort(rng.integers(0, size - NB, NR)).astype(np.int64)
    r_stop = r_start + NB
    pairs = NR * NB * len(periods)
    scores, offs = eng.wps_intervals("c", r_start, r_stop, size)
    d_scores = torch.from_numpy(np.asarray(scores)).to(dev)
    d_spec = torch.zeros((NR, len(periods), 2), dtype=torch.float64, device=dev)
    d_ssw = torch.zeros(NR, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    def transform():
        eng.track_spectrum(d_scores, offs, periods, out=d_spec, ssw_out=d_ssw)

    def fused():
        return eng.wps_spectrum("c", r_start, r_stop, size, periods)

    nn = np.arange(NB)
    bell = np.ones(NB)
    M = int(np.floor(0.1 * NB))
    bell[:M] = 0.5 * (1.0 - np.cos(np.pi * (2.0 * nn[:M] + 1.0) / (2.0 * M)))
    bell[NB - M:] = bell[:M][::-1]
    ang = 2 * np.pi * (nn[:, None] % periods[None, :]) / periods[None, :]
    twiddle = np.concatenate([np.cos(ang), -np.sin(ang)], axis=1)  # built once, outside the timed part

    def host_route():
        sc, _ = eng.wps_intervals("c", r_start, r_stop, size)
        x = np.asarray(sc).reshape(NR, NB).astype(np.float64)
        x -= x.mean(axis=1, keepdims=True)
        x *= bell
        both = x @ twiddle
        return both[:, :len(periods)] + 1j * both[:, len(periods):]

    def wall(fn, name):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(max(reps // 4, 3)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ts = np.array(ts)
        print(f"{name:34s} median {np.median(ts) * 1e3:9.3f} ms  min {ts.min() * 1e3:9.3f} ms", flush=True)
        return float(np.median(ts))

    print(f"spectrum: {n} fragments, {NR} regions x {NB} bases x {len(periods)} periods = {pairs:.3g} (sample, period) pairs", flush=True)
    for _ in range(2):  # twice: the spread between the two passes is the noise
        t_tr = wall(transform, "spectrum, transform alone")
        t_fu = wall(fused, "spectrum, fused call")
        t_ho = wall(host_route, "wps_intervals + numpy on the host")
        timeit(transform, "transform alone (device events)", 8 * NR * NB * (2 + len(periods) / 4))
        print(f"  fused call vs the host route: {t_ho / t_fu:.1f} x;  transform: {pairs / t_tr / 1e12:.2f}e12 pairs/s = "
              f"{2 * pairs / 39.3e12 / t_tr:.1%} of the direct form's FMA roof, {16 * pairs / 150e12 / t_tr:.1%} of its LDS-lookup roof", flush=True)
    got, _ = fused()
    want = host_route()
    torch.cuda.synchronize()
    scale = float(np.abs(want).max())
    print("spectrum checksum: fused vs host route, largest difference over the largest value",
          float(np.abs(got - want).max()) / scale, "fused == transform bits",
          bool(np.array_equal(got.view(np.float64).reshape(NR, len(periods), 2), d_spec.cpu().numpy())))
if "peaks" in which:
    # Nucleosome calls: the spectrum mode's regions (KBENCH_PEAKS_REGIONS x KBENCH_PEAKS_BASES, 2 000 x 10 000), median window
    # 1000, savgol(21, 2), the default rule.  Four times, wall clock around the whole call: (a) the two peak passes alone on
    # an adjusted track that is on the device (the calls come home: some tens of bytes each); (b) ftk_wps_adjust on the
    # same runs, device to device; (c) the fused call; (d) the route there was before - ftk_wps_intervals to host memory,
    # float64 on the host, ftk_wps_adjust host to host, ftk_track_peaks from the host.  The passes' floor: the track is
    # read about twice (mark, then the regions), 8 bytes a base, at the HBM rate.
    import time
    rng = np.random.default_rng(193)
    NR, NB = int(os.environ.get("KBENCH_PEAKS_REGIONS", "2000")), int(os.environ.get("KBENCH_PEAKS_BASES", "10000"))
    W, SW = 1000, 21
    r_start = np.sort(rng.integers(0, size - NB, NR)).astype(np.int64)
    r_stop = r_start + NB
    scores, offs = eng.wps_intervals("c", r_start, r_stop, size)
    raw = np.asarray(scores, np.float64)
    adj_offs = offs - np.arange(NR + 1) * W
    n_adj = int(adj_offs[-1])
    d_raw = torch.from_numpy(raw).to(dev)
    d_adj = torch.zeros(n_adj, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    def adjust():
        eng.wps_adjust(d_raw.data_ptr(), offs, W, savgol_window_size=SW, out=d_adj.data_ptr())

    def passes():
        return eng.track_peaks(d_adj, adj_offs, skip=SW // 2)

    def fused():
        return eng.wps_peaks("c", r_start, r_stop, size, median_window_size=W, savgol_window_size=SW)

    def two_step():
        sc, o = eng.wps_intervals("c", r_start, r_stop, size)
        return eng.track_peaks(eng.wps_adjust(np.asarray(sc, np.float64), o, W, savgol_window_size=SW), adj_offs, skip=SW // 2)

    def wall(fn, name):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(max(reps // 4, 3)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ts = np.array(ts)
        print(f"{name:34s} median {np.median(ts) * 1e3:9.3f} ms  min {ts.min() * 1e3:9.3f} ms", flush=True)
        return float(np.median(ts))

    adjust()
    torch.cuda.synchronize()
    print(f"peaks: {n} fragments, {NR} regions x {NB} bases, {n_adj} adjusted scores", flush=True)
    for _ in range(2):  # twice: the spread between the two passes is the noise
        t_pk = wall(passes, "peaks, the two passes alone")
        t_ad = wall(adjust, "ftk_wps_adjust, device to device")
        t_fu = wall(fused, "peaks, fused call")
        t_2s = wall(two_step, "intervals + adjust + peaks by host")
        floor = 2 * 8 * n_adj / (bench.HBM_PEAK_GBS * 1e9)
        print(f"  passes: {floor / t_pk:.1%} of their HBM floor ({floor * 1e3:.3f} ms), {t_pk / t_ad:.2f} x ftk_wps_adjust;  "
              f"two-step route / fused call: {t_2s / t_fu:.2f} x", flush=True)
    (c_f, s_f), (c_2, s_2), (c_p, s_p) = fused(), two_step(), passes()
    for c in (c_2, c_p):  # a track's positions count from its run's start: to the contig, as the fused call's do
        for name in ("start", "stop", "summit"):
            c[name] += r_start[c["run"]] + W // 2
    print("peaks checksum: calls", len(c_f), "counters", s_f.sum(axis=0).tolist(), "fused == two-step bits",
          bool(c_f.tobytes() == c_2.tobytes() and np.array_equal(s_f, s_2)), "fused == passes bits",
          bool(c_f.tobytes() == c_p.tobytes() and np.array_equal(s_f, s_p)))
if "prefends" in which:
    # Preferred ends of the whole contig as one interval: the whole call (per batch of tiles the count pass, the scan, one
    # read-back, the write pass, the calls copied to host blocks) at h = 500 and h = 2048 in both modes, beside
    # ftk_depth_runs (whole call) and ftk_cleavage (launch into a device buffer) of the same region.  Byte floor: the
    # columns of every candidate of a 4 096-base tile (counted from the sorted starts as in the depth mode; 6 B with the
    # packed column, else 9 B) times (tile + 2 h) / tile for the halo, read by both passes, plus 32 B per call written.
    import time

    from finaletoolkit_amd import _lib as L
    from finaletoolkit_amd.utils import preferred_end_thresholds
    TILE = L.PREFENDS_TILE
    lmax = eng.info("c")[1]
    hs = s.cpu().numpy().astype(np.int64)
    t0 = np.arange(0, size, TILE, dtype=np.int64)
    t1 = np.minimum(t0 + TILE, size)
    cand = int((np.searchsorted(hs, ((t1 >> 9) + 1) << 9, side="left")
                - np.searchsorted(hs, (np.maximum(t0 - lmax, 0) >> 9) << 9, side="left")).sum())
    col_bytes = 6 if eng.frags_packed("c") else 9
    thr = preferred_end_thresholds(0.01)
    cl = torch.empty(size, dtype=torch.float64, device=dev)
    got = {}

    def call(h, mode):
        got[h, mode] = eng.preferred_ends("c", [0], [size], size, half=h, mode=mode, thresholds=thr)

    def wall(fn, name):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(max(reps // 4, 3)):
            a = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - a)
        ts = np.array(ts)
        print(f"{name:34s} median {np.median(ts) * 1e3:9.3f} ms  min {ts.min() * 1e3:9.3f} ms", flush=True)
        return float(np.median(ts))

    print(f"prefends: {n} fragments, {len(t0)} tiles, {cand} candidates ({cand / n:.2f} per fragment), {col_bytes} B per candidate",
          flush=True)
    for _ in range(2):  # twice: the spread between the two passes is the noise
        t_runs = wall(lambda: eng.depth_runs("c", 0, size, 30), "depth runs (whole call)")
        t_cl = wall(lambda: eng.cleavage("c", 0, size, None, None, 30, out=cl), "cleavage (launch)")
        for h in (500, 2048):
            for mode in ("combined", "split"):
                t = wall(lambda: call(h, mode), f"preferred ends h={h} {mode}")
                halo = (TILE + 2 * h) / TILE
                floor = (2 * col_bytes * cand * halo + 32 * len(got[h, mode][0])) / (bench.HBM_PEAK_GBS * 1e9)
                print(f"  {len(got[h, mode][0])} calls; {t / t_runs:.2f} x depth runs, {t / t_cl:.2f} x cleavage; halo factor x 2 = "
                      f"{2 * halo:.2f}; {floor / t:.1%} of the byte floor ({floor * 1e3:.3f} ms)", flush=True)
    print("prefends checksum:", {f"{h}/{mode}": (len(c), st.sum(axis=0).tolist()) for (h, mode), (c, st) in sorted(got.items())})
if "hotspots" in which:
    # IFS hotspots of the whole contig as one interval: the whole call (per batch of tiles the count pass, the scan, one
    # read-back, the write pass, the called windows copied to host blocks, the merge on the host) at the defaults, the totals
    # reduction that gives mean_length and global_mean, and the per-window track into device arrays; beside them preferred
    # ends combined at h = 500, the nearest kernel with the same candidate traffic.  Byte floor, computed as for prefends:
    # the columns of every candidate of a tile of 4 096 windows (81 920 bases; counted from the sorted starts) times
    # (tile + 2 (h2 + m)) / tile for the halo, read by both passes, plus 44 B per called window written.
    import time

    from finaletoolkit_amd import _lib as L
    from finaletoolkit_amd.utils import ifs_thresholds, preferred_end_thresholds
    STEP, M, H1, H2 = 20, 10, 125, 250
    TILE = L.HOTSPOTS_TILE * STEP
    lmax = eng.info("c")[1]
    hs = s.cpu().numpy().astype(np.int64)
    t0 = np.arange(0, size, TILE, dtype=np.int64)
    t1 = np.minimum(t0 + TILE, size)
    cand = int((np.searchsorted(hs, ((t1 >> 9) + 1) << 9, side="left")
                - np.searchsorted(hs, (np.maximum(t0 - lmax, 0) >> 9) << 9, side="left")).sum())
    col_bytes = 6 if eng.frags_packed("c") else 9
    thr = ifs_thresholds(1e-5)
    pthr = preferred_end_thresholds(0.01)
    N, S = eng.ifs_totals("c", size)
    Lm = max((2 * S + N) // (2 * N), 1)
    gm = (N * Lm + S) * M * 1024 // (-(-size // STEP) * Lm)
    got = {}

    def call():
        got["hot"] = eng.ifs_hotspots("c", [0], [size], size, step=STEP, m=M, mean_length=Lm, h1=H1, h2=H2, thresholds=thr,
                                      global_mean=gm)

    def wall(fn, name):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(max(reps // 4, 3)):
            a = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - a)
        ts = np.array(ts)
        print(f"{name:34s} median {np.median(ts) * 1e3:9.3f} ms  min {ts.min() * 1e3:9.3f} ms", flush=True)
        return float(np.median(ts))

    print(f"hotspots: {n} fragments, L = {Lm}, global mean {gm / 1024:.3f}, {len(t0)} tiles, {cand} candidates ({cand / n:.2f} per "
          f"fragment), {col_bytes} B per candidate", flush=True)
    for _ in range(2):  # twice: the spread between the two passes is the noise
        t_pe = wall(lambda: eng.preferred_ends("c", [0], [size], size, half=500, mode="combined", thresholds=pthr),
                    "preferred ends h=500 combined")
        t_tot = wall(lambda: eng.ifs_totals("c", size), "IFS totals")
        t_trk = wall(lambda: eng.ifs_track("c", [0], [size], size, step=STEP, m=M, mean_length=Lm, device=True), "IFS track (device arrays)")
        t = wall(call, "IFS hotspots (whole call)")
        win, hot, stats = got["hot"]
        halo = (L.HOTSPOTS_TILE + 2 * (H2 + M)) / L.HOTSPOTS_TILE
        floor = (2 * col_bytes * cand * halo + 44 * len(win)) / (bench.HBM_PEAK_GBS * 1e9)
        print(f"  {len(win)} called windows, {len(hot)} hotspots; {t / t_pe:.2f} x preferred ends; halo factor x 2 = {2 * halo:.2f}; "
              f"{floor / t:.1%} of the byte floor ({floor * 1e3:.3f} ms); totals {t_tot * 1e3:.3f} ms, track {t_trk * 1e3:.3f} ms",
              flush=True)
    print("hotspots checksum:", len(got["hot"][0]), len(got["hot"][1]), got["hot"][2].tolist())
if "gc" in which:
    rng = np.random.default_rng(6)
    packed = rng.integers(0, 256, (size + 3) // 4, dtype=np.uint8)
    rid = eng.ref_upload(("kb", "gc2bit"), packed, 1)
    glo, ghi = synth.tiling_windows(size, 100_000)
    d_lo = torch.from_numpy(glo.astype(np.int64)).to(dev); d_hi = torch.from_numpy(ghi.astype(np.int64)).to(dev)
    d_gc = torch.zeros(len(glo), dtype=torch.int64, device=dev)
    import ctypes as C
    from finaletoolkit_amd import _lib as L
    f = lambda: eng._check(eng.lib.ftk_ref_gc_counts(eng.ctx, rid, L.ptr(d_lo), L.ptr(d_hi), len(glo), L.ptr(d_gc)))
    timeit(f, "GC count 100 kb bins (2bit)", size // 4)
if "small" in which:
    # window sizes from 500 bp to 100 kb over the same contig: which launch shape the host picks matters here
    for wlen in (500, 2_000, 10_000, 20_000, 100_000):
        sws, swe = synth.tiling_windows(size, wlen)
        timeit(lambda: eng.window_counts("c", sws, swe, 30), f"window_counts {wlen} bp x{len(sws)}", 10 * n)
if "motif" in which:
    # 1 Mb windows (end_motifs' tiling), random 2bit / FASTA-text images of the contig
    mws, mwe = synth.tiling_windows(size, 1_000_000)
    rng = np.random.default_rng(5)
    packed = rng.integers(0, 256, (size + 3) // 4, dtype=np.uint8)
    rid2 = eng.ref_upload(("kb", "2bit"), packed, 1)
    eng.ref_set_layout(rid2, size, 0, 0, [10_000], [20_000])
    text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size + size // 60 + 1)].copy()
    text[60::61] = 10
    ridf = eng.ref_upload(("kb", "fa"), text, 0)
    eng.ref_set_layout(ridf, size, 60, 61)
    for rid, tag in ((rid2, "2bit"), (ridf, "fasta")):
        for k in (4, 6):
            f = lambda: eng.motif_counts("c", rid, mws, mwe, k, 0, -k, True, False, 0, False, 30)
            timeit(f, f"end motifs k={k} {tag}", 10 * n)
    c, nf, er = eng.motif_counts("c", rid2, mws, mwe, 4, 0, -4, True, False, 0, False, 30)
    print("motif total", int(c.sum()), "fragments", int(nf.sum()))
print("wps checksum", int(out[:5_000_000].sum().item()), "cov", int(cov.sum().item()))
if "endcontext" in which:
    # End context at W = 32, classes (1, 150, 221, 1001), against the 2bit image of KBENCH=gcbias: the whole call (table zeroed,
    # kernel, 77 KB copied to the host).  The work is LDS updates, not bytes: 2 kinds x 2 W offsets per kept fragment, one
    # returnless 32-bit LDS add each.  The estimate it is held against: a 64-lane LDS add takes 4 LDS cycles of a CU (the rate
    # of a 32-bit LDS write), so 16 updates per clock and CU at 2.4 GHz.  The byte figure printed is the columns + the image.
    rng = np.random.default_rng(7)
    packed = rng.integers(0, 256, (size + 3) // 4, dtype=np.uint8)
    ride = eng.ref_upload(("kb", "gcbias2bit"), packed, 1)
    eng.ref_set_layout(ride, size, 0, 0, [10_000_000], [10_050_000])
    img = (size + 3) // 4
    W, EDGES = 32, (1, 150, 221, 1001)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    lds_rate = 16 * n_cu * 2.4e9

    def context(arrange):
        os.environ["FTK_CONTEXT_ARRANGE"] = arrange
        return eng.end_context("c", ride, W, EDGES, 30, "ends")

    def motif_route():
        for o in range(-W, W):
            eng.motif_counts("c", ride, [0], [size], 2, o, -o - 2, True, False, 0, False, 30)

    tables = {a: context(a) for a in ("0", "1")}
    assert np.array_equal(tables["0"][0], tables["1"][0]) and np.array_equal(tables["0"][1], tables["1"][1])
    table, kept = tables["0"]
    updates = 2 * 2 * W * int(kept.sum())
    print(f"endcontext: {n} fragments, {int(kept.sum())} kept, {updates} LDS updates, image {img} B, {n_cu} CUs: "
          f"{updates / lds_rate * 1e6:.1f} us at the estimated LDS rate", flush=True)
    for _ in range(2):  # twice: the spread between the two passes is the noise
        timeit(lambda: context("0"), "end context, lanes=offsets", 9 * n + img)
        timeit(lambda: context("1"), "end context, lanes=frags", 9 * n + img)
        timeit(lambda: eng.frag_gc_table("c", ride, 100, 220, 30), "observed GC table 100-220", 9 * n + img)
        timeit(motif_route, "64 x motif_counts (k=2)", 64 * 9 * n)
        timeit(lambda: eng.ref_context(ride, 0, size), "ref context (background)", img)
    del os.environ["FTK_CONTEXT_ARRANGE"]
    print("endcontext checksum", int(table.sum()), int(table[..., 20:].sum()), int(eng.ref_context(ride, 0, size).sum()),
          "(share of the LDS estimate = the us above / the measured us)")
if "motiflen" in which:
    # Motif x length at k = 4 over the lengths 1 .. 1000, against the 2bit image of KBENCH=gcbias / endcontext: the whole call
    # (table zeroed, both passes, 4 MB copied to the host).  The bytes it is held against: the (start, end, mapq) columns once
    # for the row pass and once per POPULATED band of the table pass (an empty band returns before it reads a column), and
    # two 32-byte sectors of the image per kept fragment (one per end).
    rng = np.random.default_rng(7)
    packed = rng.integers(0, 256, (size + 3) // 4, dtype=np.uint8)
    ridm = eng.ref_upload(("kb", "gcbias2bit"), packed, 1)
    eng.ref_set_layout(ridm, size, 0, 0, [10_000_000], [10_050_000])
    K, LO, HI = 4, 1, 1000
    table, kept = eng.motif_length_table("c", ridm, K, 0, LO, HI, 1, 30)

    def call_bytes(k):
        band = eng.motif_length_lds_rows(k)
        populated = sum(1 for r0 in range(0, len(kept), band) if kept[r0:r0 + band].any())
        return band, populated, 9 * n * (1 + populated) + 64 * int(kept.sum())

    band, populated, nbytes = call_bytes(K)
    print(f"motiflen: {n} fragments, {int(kept.sum())} kept, k = {K}, rows {LO} .. {HI}, bands of {band} rows: {populated} of "
          f"{-(-len(kept) // band)} populated, {nbytes} algorithmic bytes", flush=True)
    for _ in range(2):  # twice: the spread between the two passes is the noise
        timeit(lambda: eng.motif_length_table("c", ridm, K, 0, LO, HI, 1, 30), "motif x length k=4 1-1000", nbytes)
        timeit(lambda: eng.motif_length_table("c", ridm, 2, -1, LO, HI, 1, 30), "motif x length k=2 breakpoint", call_bytes(2)[2])
    assert np.array_equal(table.sum(axis=-1), np.stack([kept, kept]))
    print("motiflen checksum", int(table.sum()), int(table[..., -1].sum()), int((table[0] * np.arange(4 ** K + 1)).sum()),
          int((table[1] * np.arange(4 ** K + 1)).sum()))
if "cofrag" in which:
    # Co-fragmentation: N = 2490 bins of 100 kb (chr1 at that bin size), lengths 0 .. 1000.  The work is pair steps, not bytes:
    # N (N + 1) / 2 pairs x n_bins lengths, each two 32 x 32 -> 64 multiplies, a 64-bit subtraction, an absolute value, a compare
    # and three selects (13 vector instructions in the tiled kernel's inner loop, docs/experiments.md).  Outputs stay on the
    # device except in the "host outputs" row, which adds the 74 MB of K and `at` on their way home.
    import ctypes as C
    import time
    from finaletoolkit_amd import _lib as L
    N, NB = min(2490, len(ws)), 1001
    c_ws, c_we = np.ascontiguousarray(ws[:N]), np.ascontiguousarray(we[:N])
    flt = L.make_filter(30, None, None, "midpoint")
    d_hist = torch.zeros((N, NB), dtype=torch.int32, device=dev)
    d_over = torch.zeros(N, dtype=torch.int64, device=dev)
    d_k = torch.zeros((N, N), dtype=torch.int64, device=dev)
    d_at = torch.zeros((N, N), dtype=torch.int32, device=dev)
    d_n = torch.zeros(N, dtype=torch.int64, device=dev)

    def hist_only():
        eng._check(eng.lib.ftk_fraglen_hist(eng.ctx, eng.contig_id("c"), L.ptr(c_ws), L.ptr(c_we), N, C.byref(flt), 0, NB, L.ptr(d_hist),
                                            L.ptr(d_over)))

    def ks(arrange, at=True):
        os.environ["FTK_COFRAG_ARRANGE"] = arrange
        eng._check(eng.lib.ftk_hist_ks(eng.ctx, L.ptr(d_hist), N, NB, L.ptr(d_k), L.ptr(d_at) if at else None, L.ptr(d_n)))

    def whole(arrange):
        os.environ["FTK_COFRAG_ARRANGE"] = arrange
        eng._check(eng.lib.ftk_cofrag(eng.ctx, eng.contig_id("c"), L.ptr(c_ws), L.ptr(c_we), N, C.byref(flt), 0, NB, L.ptr(d_k), L.ptr(d_at),
                                      L.ptr(d_n), L.ptr(d_over)))

    hist_only()
    got = {}
    for a in ("0", "1"):
        ks(a)
        torch.cuda.synchronize()
        got[a] = (d_k.cpu().numpy().copy(), d_at.cpu().numpy().copy(), d_n.cpu().numpy().copy())
    assert all(np.array_equal(x, y) for x, y in zip(got["0"], got["1"]))
    whole("1")
    torch.cuda.synchronize()
    assert np.array_equal(d_k.cpu().numpy(), got["1"][0]) and np.array_equal(d_at.cpu().numpy(), got["1"][1])
    steps = N * (N + 1) // 2 * NB
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"cofrag: {N} bins x {NB} lengths, {steps} pair steps, {int(got['1'][2].sum())} fragments in range, {n_cu} CUs", flush=True)
    nbytes = N * NB * 4 + N * N * 12
    for _ in range(2):  # twice: the spread between the two passes is the noise
        timeit(hist_only, "fraglen_hist 2490 x 1001", 10 * n)
        timeit(lambda: ks("0"), "hist_ks, thread per pair", nbytes)
        timeit(lambda: ks("1"), "hist_ks, 64 x 64 tiles", nbytes)
        timeit(lambda: ks("1", at=False), "hist_ks, tiles, no at", nbytes - N * N * 4)
        timeit(lambda: whole("0"), "cofrag, thread per pair", 10 * n + nbytes)
        timeit(lambda: whole("1"), "cofrag, 64 x 64 tiles", 10 * n + nbytes)
    os.environ["FTK_COFRAG_ARRANGE"] = "1"
    h_hist = d_hist.cpu().numpy().view(np.uint32)
    timeit(lambda: eng.hist_ks(h_hist), "hist_ks, host in and out", nbytes)
    del os.environ["FTK_COFRAG_ARRANGE"]
    if os.environ.get("KBENCH_COFRAG_CPU", "1") != "0":
        from tests import cofrag_helpers
        sub = h_hist[:500]
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            ck = cofrag_helpers.ks_matrix(sub)
            ts.append(time.perf_counter() - t0)
        assert np.array_equal(ck[0], got["1"][0][:500, :500]) and np.array_equal(ck[1], got["1"][1][:500, :500])
        print(f"numpy restatement on this host, N = 500 x {NB}: best of 3 {min(ts):.3f} s; SCALED by (N / 500)^2 to N = {N}: "
              f"{min(ts) * (N / 500) ** 2:.1f} s", flush=True)
    print("cofrag checksum", int(got["1"][0].sum() % (1 << 61)), int(got["1"][1].sum()), int(got["1"][2].sum()))
