"""CPU: the pieces of the IFS hotspot feature that need no GPU - the threshold table, the numpy restatement of the rule
(``tests/hotspots_helpers.py``) on cases worked by hand, the command line's parser, the writers byte for byte, the argument
checks of ``utils.frag_hotspots``, and the build's file lists."""
import gzip
import inspect
import math
import os
import re

import numpy as np
import pytest

from tests.hotspots_helpers import (HOTSPOT_DTYPE, WINDOW_DTYPE, backgrounds, bin_tracks, flat_table, global_mean_ref,
                                    ifs_hotspots_ref, ifs_track_ref, interval_windows, merge_ref, totals_ref, window_sums)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def poisson_cdf(q, mean):
    """P(X <= q | Poisson(mean)) by the sum itself."""
    return math.exp(-mean) * sum(mean ** k / math.factorial(k) for k in range(q + 1))


# ---- the table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [1e-5, 0.01, 1e-12])
def test_threshold_table(alpha):
    from scipy.special import gammaincc
    from finaletoolkit_amd import utils
    thr = utils.ifs_thresholds(alpha, 256)
    assert thr.dtype == np.uint64 and thr.shape == (256,) and int(thr.max()) < 1 << 32
    assert np.all(np.diff(thr.astype(np.int64)) > 0)  # a larger IFS needs a larger mean to be low
    q = np.arange(256, dtype=np.float64)
    assert np.all(gammaincc(q + 1, thr / 1024.0) <= alpha)            # each entry satisfies the condition ...
    assert np.all(gammaincc(q + 1, (thr - np.uint64(1)) / 1024.0) > alpha)   # ... and the integer below it does not
    assert abs(int(thr[0]) / 1024.0 + math.log(alpha)) <= 1 / 1024.0  # P(X <= 0) = exp(-mean)
    for k in (0, 1, 5, 40):  # the sum itself agrees on either side of an entry
        assert poisson_cdf(k, int(thr[k]) / 1024.0) <= alpha * (1 + 1e-9) and poisson_cdf(k, (int(thr[k]) - 1) / 1024.0) > alpha * (1 - 1e-9)


def test_threshold_table_arguments():
    from finaletoolkit_amd import utils
    assert np.array_equal(utils.ifs_thresholds(), utils.ifs_thresholds(1e-5, 256))
    assert len(utils.ifs_thresholds(0.5, 1)) == 1 and len(utils.ifs_thresholds(1e-3, 4096)) == 4096
    assert np.array_equal(utils.ifs_thresholds(1e-3, 4096)[:100], utils.ifs_thresholds(1e-3, 100))
    for bad in (0.0, 1.0, -0.1, 2.0):
        with pytest.raises(ValueError, match="alpha"):
            utils.ifs_thresholds(bad)
    for bad in (0, -1, 4097):
        with pytest.raises(ValueError, match="invalid n"):
            utils.ifs_thresholds(1e-5, bad)
    sig = inspect.signature(utils.ifs_thresholds)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [("alpha", 1e-5), ("n", 256)]


# ---- the restatement on cases worked by hand ------------------------------------------------------------------------------
def test_restatement_bins_and_windows():
    # chrom_size 95, step 10: ten bins, the last of five bases.  Midpoints: (0 + 9) >> 1 = 4 (bin 0), (10 + 31) >> 1 = 20
    # (bin 2), (88 + 100) >> 1 = 94 (bin 9, the last base), (90 + 100) >> 1 = 95 (outside), (-7 + 6) >> 1 = -1 (outside),
    # one of mapq 29, one without a base
    s = np.array([0, 10, 88, 90, -7, 40, 50])
    e = np.array([9, 31, 100, 100, 6, 60, 50])
    q = np.array([60, 60, 30, 60, 60, 29, 60])
    assert totals_ref(s, e, q, 95) == (3, 9 + 21 + 12)
    c, i = bin_tracks(s, e, q, 95, 10, L=100)
    assert c.tolist() == [1, 0, 1, 0, 0, 0, 0, 0, 0, 1] and i.tolist() == [109, 0, 121, 0, 0, 0, 0, 0, 0, 112]
    assert window_sums(c, 3).tolist() == [2, 1, 1, 0, 0, 0, 0, 1] and window_sums(c, 10).tolist() == [3] and len(window_sums(c, 11)) == 0
    B, nb = backgrounds(i, 3, 2)  # window k: bins [k - 2, k + 4] clipped to [0, 9]
    assert nb.tolist() == [5, 6, 7, 7, 7, 7, 6, 5] and B.tolist() == [230, 230, 230, 121, 121, 112, 112, 112]
    # length bounds
    assert bin_tracks(s, e, q, 95, 10, 100, min_len=10, max_len=12)[0].tolist() == [0] * 9 + [1]
    # the windows of an interval: a <= k s and the span's end <= b; the last window's span is clipped to the contig
    assert interval_windows(0, 95, 95, 10, 3) == (0, 7) and interval_windows(0, 94, 95, 10, 3) == (0, 6)
    assert interval_windows(1, 90, 95, 10, 3) == (1, 6) and interval_windows(10, 40, 95, 10, 3) == (1, 1)
    assert interval_windows(11, 40, 95, 10, 3)[1] < interval_windows(11, 40, 95, 10, 3)[0]
    assert interval_windows(0, 95, 95, 10, 10) == (0, 0) and interval_windows(0, 95, 95, 10, 11) == (0, -1)
    n, I, offs = ifs_track_ref(s, e, q, [0, 10, 50], [95, 40, 50], 95, step=10, m=3, mean_length=100)
    assert offs.tolist() == [0, 8, 9, 9] and n.tolist() == [2, 1, 1, 0, 0, 0, 0, 1, 1] and I[:2].tolist() == [230, 121] and I[8] == 121
    assert global_mean_ref(3, 42, 100, 3, 95, 10) == (342 * 3 * 1024) // 1000


def test_restatement_decision_on_equality():
    # step 1, m = 1, L = 10: one fragment of length 10 per midpoint, i = 20 per fragment, q = 2 per fragment
    mids = [50, 50, 50, 53]
    s = np.array(mids) - 5
    e, q = s + 10, np.full(4, 60)
    # window 50: n = 3, I = 60, q = 6.  h = 3: bins 47 .. 53, B = 80, n_b = 7.  B m 1024 >= t n_b L <=> 81920 >= 70 t <=> t <= 1170
    for t, called in ((1170, True), (1171, False)):
        thr = np.zeros(8, np.uint64)
        thr[6] = t
        w, h, st = ifs_hotspots_ref(s, e, q, [0], [100], 100, step=1, m=1, mean_length=10, h1=3, h2=0, thresholds=thr, join=1)
        assert st.tolist() == [[100, 100, int(called), int(called), 0, int(called)]]
        if called:
            assert w.tolist() == [(0, 50, 3, 60, 80, 7, 0, 0)] and h.tolist() == [(0, 50, 51, 1, 50, 60, 3, 80, 7)]
    thr = np.zeros(8, np.uint64)
    thr[6] = 1170
    kw = dict(step=1, m=1, mean_length=10, h1=3, thresholds=thr, join=1)
    # the second background, h = 4: bins 46 .. 54, the same B, n_b = 9: 81920 >= 90 t fails at 1170 and holds at 910
    assert ifs_hotspots_ref(s, e, q, [0], [100], 100, h2=4, **kw)[2][0, 2] == 0
    thr[6] = 910
    assert ifs_hotspots_ref(s, e, q, [0], [100], 100, h2=4, **kw)[0].tolist() == [(0, 50, 3, 60, 80, 7, 80, 9)]
    # global_mean: t <= global_mean, and 0 switches it off
    assert ifs_hotspots_ref(s, e, q, [0], [100], 100, h2=0, global_mean=910, **kw)[2][0, 2] == 1
    assert ifs_hotspots_ref(s, e, q, [0], [100], 100, h2=0, global_mean=909, **kw)[2][0, 2] == 0
    # min_count: n = 3 is tested at 3 and not at 4; windows without a fragment are tested at 0 alone
    assert ifs_hotspots_ref(s, e, q, [0], [100], 100, h2=0, min_count=3, **kw)[2].tolist() == [[100, 1, 1, 1, 0, 1]]
    assert ifs_hotspots_ref(s, e, q, [0], [100], 100, h2=0, min_count=4, **kw)[2].tolist() == [[100, 0, 0, 0, 0, 0]]
    # q == n_thr - 1 reads the last entry, q == n_thr reads nothing
    assert ifs_hotspots_ref(s, e, q, [0], [100], 100, h2=0, **dict(kw, thresholds=np.array([0] * 6 + [910], np.uint64)))[2][0, 2] == 1
    assert ifs_hotspots_ref(s, e, q, [0], [100], 100, h2=0, min_count=1, **dict(kw, thresholds=np.full(6, 1, np.uint64)))[0]["pos"].tolist() == [53]
    # a background clipped at the contig's first bin: midpoint 1, h = 3: bins 0 .. 4, n_b = 5
    w, _, _ = ifs_hotspots_ref(np.array([-4]), np.array([6]), np.array([60]), [0], [100], 100, h2=0, min_count=1,
                               **dict(kw, thresholds=flat_table(1)))
    assert w.tolist() == [(0, 1, 1, 20, 20, 5, 0, 0)]


def test_restatement_merge():
    def windows(ks, ifs, step=20):
        w = np.zeros(len(ks), WINDOW_DTYPE)
        w["pos"], w["ifs"], w["count"], w["bg1"], w["nb1"] = np.array(ks) * step, ifs, np.array(ifs) // 100, 7, 9
        return w
    # gaps of exactly join and join + 1; equal minima take the leftmost; a short hotspot is dropped
    hot, kept, dropped, bases = merge_ref(windows([3, 5, 7, 10, 11, 30], [500, 300, 300, 900, 100, 50]), 4, 1000, 20, 10, join=2, min_windows=2)
    assert hot.tolist() == [(4, 60, 340, 3, 100, 300, 3, 7, 9), (4, 200, 420, 2, 220, 100, 1, 7, 9)]
    assert (kept, dropped) == (2, 1) and bases == 280 + 80  # [60, 340) and [200, 420) overlap on [200, 340)
    hot, kept, dropped, bases = merge_ref(windows([3, 5, 7, 10, 11, 48], [5] * 6), 0, 1000, 20, 10, join=3, min_windows=1)
    assert hot[["start", "stop", "n_windows", "summit"]].tolist() == [(60, 420, 5, 60), (960, 1000, 1, 960)]  # the last span is clipped
    assert (kept, dropped, bases) == (2, 0, 360 + 40)
    assert merge_ref(windows([], []), 0, 1000, 20, 10, 1, 1)[1:] == (0, 0, 0)
    # hotspots never join across runs: two overlapping intervals over the same called windows
    s = np.repeat(np.array([40, 41]), 3) - 5
    w, h, st = ifs_hotspots_ref(s, s + 10, np.full(6, 60), [0, 30], [100, 60], 100, step=1, m=1, mean_length=10, h1=3, h2=0,
                                thresholds=flat_table(1, 16), join=1, min_count=1)
    assert h.tolist() == [(0, 40, 42, 2, 40, 60, 3, 120, 7), (1, 40, 42, 2, 40, 60, 3, 120, 7)]
    assert st.tolist() == [[100, 2, 2, 1, 0, 2], [30, 2, 2, 1, 0, 2]]


# ---- the product's Python face --------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_engine_use(tmp_path, monkeypatch):
    from finaletoolkit_amd import utils

    def no_engine(*a, **k):
        raise AssertionError("the engine was asked for")
    monkeypatch.setattr(utils, "get_engine", no_engine)
    bam = str(tmp_path / "absent.bam")  # it does not exist: nothing may open it
    cases = [
        (dict(output_file=str(tmp_path / "out.tsv")), "output_file"),
        (dict(windows_file=str(tmp_path / "out.bed.bz2")), "windows_file"),
        (dict(summary_file=str(tmp_path / "out.bed")), "summary_file"),
        (dict(step=0), "step"),
        (dict(step=65536, window=65536), "step"),
        (dict(window=210), "window"),
        (dict(window=0), "window"),
        (dict(step=1, window=65), "window"),
        (dict(background=(39, 10000)), "background"),
        (dict(background=(10000, 5000)), "background"),
        (dict(background=(5000, 10000, 20000)), "background"),
        (dict(background=(5000, 2 * 20 * 1015)), "background"),
        (dict(alpha=0.0), "alpha"),
        (dict(alpha=1.0), "alpha"),
        (dict(mean_length=0), "mean_length"),
        (dict(mean_length=65536), "mean_length"),
        (dict(min_count=-1), "min_count"),
        (dict(join=0), "join"),
        (dict(join=1025), "join"),
        (dict(min_windows=0), "min_windows"),
        (dict(min_length=-1), "min_length"),
        (dict(max_length=-1), "max_length"),
        (dict(min_length=200, max_length=100), "min_length"),
    ]
    for kwargs, word in cases:
        with pytest.raises(ValueError, match=word):
            utils.frag_hotspots(bam, **kwargs)
    with pytest.raises(ValueError, match="chrom_sizes"):  # a fragment file carries no lengths
        utils.frag_hotspots(str(tmp_path / "absent.frag.gz"))
    sizes = tmp_path / "c.sizes"
    sizes.write_text("chr2\t1000\n")
    bed = tmp_path / "iv.bed"
    bed.write_text("chr1\t0\t5000\tg\n")
    with pytest.raises(ValueError, match="chrom_sizes"):  # the interval's contig is not in the sizes file
        utils.frag_hotspots(str(tmp_path / "absent.frag.gz"), str(bed), chrom_sizes=str(sizes))
    # the defaults and the limits themselves pass: (m, h1, h2)
    check = utils._check_hotspots_args
    assert check(bam, None, "o.bed.gz", "w.bed", "s.tsv.gz", 20, 200, (5000, 10000), 1e-5, None, 0, None, 1, None, None) == (10, 125, 250)
    assert check(bam, None, None, None, None, 20, 200, (5000, 2 * 20 * 1014), 0.5, 65535, 0, 1024, 1, 0, 0) == (10, 125, 1014)
    assert check(bam, None, None, None, None, 1, 64, (2,), 0.5, 1, 7, 1, 9, None, None) == (64, 1, 0)
    assert check(bam, None, None, None, None, 65535, 65535, 131070, 0.5, 1, 7, 1, 9, None, None) == (1, 1, 0)


def test_signature_and_command_line():
    from finaletoolkit_amd import _lib as L
    from finaletoolkit_amd import utils
    from finaletoolkit_amd.engine import Engine
    from finaletoolkit_amd.hotspots import build_parser
    sig = inspect.signature(utils.frag_hotspots)
    assert list(sig.parameters) == ["input_file", "interval_file", "chrom_sizes", "output_file", "windows_file", "summary_file", "step",
                                    "window", "background", "alpha", "mean_length", "use_global", "min_count", "join", "min_windows",
                                    "min_length", "max_length", "quality_threshold", "workers", "verbose"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(interval_file=None, chrom_sizes=None, output_file=None, windows_file=None, summary_file=None, step=20,
                            window=200, background=(5000, 10000), alpha=1e-5, mean_length=None, use_global=True, min_count=0, join=None,
                            min_windows=1, min_length=None, max_length=None, quality_threshold=30, workers=None, verbose=False)
    ap = build_parser()
    args = vars(ap.parse_args(["in.bam", "out.bed"]))
    assert set(args) == set(sig.parameters)
    assert {k: args[k] for k in defaults if k != "output_file"} == {k: v for k, v in defaults.items() if k != "output_file"}
    full = vars(ap.parse_args(["in.frag.gz", "out.bed.gz", "--intervals", "genes.bed", "--windows", "w.bed", "--summary", "s.tsv",
                               "--chrom-sizes", "c.sizes", "--step", "10", "--window", "100", "--background", "2000", "4000", "--alpha",
                               "0.001", "--mean-length", "170", "--no-global", "--min-count", "3", "--join", "12", "--min-windows", "2",
                               "--min-length", "35", "--max-length", "80", "-q", "20", "-w", "3", "-v"]))
    assert full == dict(input_file="in.frag.gz", output_file="out.bed.gz", interval_file="genes.bed", windows_file="w.bed",
                        summary_file="s.tsv", chrom_sizes="c.sizes", step=10, window=100, background=[2000, 4000], alpha=0.001,
                        mean_length=170, use_global=False, min_count=3, join=12, min_windows=2, min_length=35, max_length=80,
                        quality_threshold=20, workers=3, verbose=True)
    with pytest.raises(SystemExit):
        ap.parse_args(["in.bam", "out.bed", "--background", "2000"])
    assert utils.IfsHotspots._fields == ("intervals", "hotspots", "windows", "stats", "mean_length", "global_mean", "step", "window_bins")
    assert utils.HOTSPOT_DTYPE.names == ("interval",) + HOTSPOT_DTYPE.names[1:]
    assert utils.IFS_WINDOW_DTYPE.names == ("interval", "start", "stop", "count", "ifs", "bg1", "nb1", "bg2", "nb2")
    call = inspect.signature(Engine.ifs_hotspots)
    assert list(call.parameters) == ["self", "name", "starts", "stops", "chrom_size", "step", "m", "mean_length", "h1", "h2", "min_count",
                                     "thresholds", "global_mean", "join", "min_windows", "min_length", "max_length", "quality_threshold"]
    assert [p.default for p in list(call.parameters.values())[5:]] == [20, 10, 167, 125, 250, 0, None, 0, None, 1, None, None, 30]
    assert list(inspect.signature(Engine.ifs_track).parameters)[:8] == ["self", "name", "starts", "stops", "chrom_size", "step", "m", "mean_length"]
    for mine, theirs in ((Engine.IFS_WINDOW_DTYPE, WINDOW_DTYPE), (Engine.HOTSPOT_DTYPE, HOTSPOT_DTYPE)):
        assert mine.names == theirs.names and [mine[f] for f in mine.names] == [theirs[f] for f in theirs.names]
    assert (L.IFS_MAX_WINDOW_BINS, L.IFS_MAX_REACH, L.IFS_MAX_THR, L.IFS_MAX_JOIN) == (64, 1024, 4096, 1024)
    assert L.HOTSPOTS_TILE > 0 and L.HOTSPOTS_BATCH_TILES > 0
    # the windows of an interval, as the engine lays its track out
    k_lo, n = Engine.ifs_window_ranges([0, 0, 1, 10, 11, 50], [95, 94, 90, 40, 40, 50], 95, 10, 3)
    assert k_lo.tolist() == [0, 0, 1, 1, 2, 5] and n.tolist() == [8, 7, 6, 1, 0, 0]
    assert Engine.ifs_window_ranges([0], [95], 95, 10, 11)[1].tolist() == [0] and Engine.ifs_window_ranges([0], [0], 0, 10, 1)[1].tolist() == [0]


def hand_made():
    from finaletoolkit_amd import utils
    hot = np.array([(0, 1000, 1400, 11, 1100, 334, 1, 501000, 260), (2, 0, 200, 1, 0, 0, 0, 100, 135)], utils.HOTSPOT_DTYPE)
    win = np.array([(0, 1000, 1200, 2, 700, 501000, 260, 990000, 510), (2, 0, 200, 0, 0, 100, 135, 0, 0)], utils.IFS_WINDOW_DTYPE)
    stats = np.array([[246, 246, 11, 1, 0, 400], [0, 0, 0, 0, 0, 0], [141, 141, 1, 1, 2, 200]], np.int64)
    return utils.IfsHotspots([("chr1", 100, 5100, "GENE1"), ("chr1", 7, 150, "tiny"), ("chr2", 0, 3000, ".")], hot, win, stats,
                             np.array([167, 167, 100]), np.array([73261, 73261, 0]), 20, 10)


@pytest.mark.parametrize("gz", [False, True])
def test_writer_text(tmp_path, gz):
    from finaletoolkit_amd import utils, writers
    res = hand_made()
    bed, wbed, tsv = (str(tmp_path / (name + ".gz" * gz)) for name in ("hot.bed", "win.bed", "summary.tsv"))
    writers.write_hotspot_rows(bed, res)
    writers.write_hotspot_windows(wbed, res)
    writers.write_hotspot_summary(tsv, res)

    def read(path):
        return gzip.open(path, "rt").read() if gz else open(path).read()
    # 334 / 167 = 2; expected = 501000 * 10 / (260 * 167) = 115.385; P(X <= 2 | 115.385) = 5.14...e-47.
    # 0 / 100 = 0; expected = 100 * 10 / (135 * 100) = 0.0740741; P(X <= 0) = exp(-0.0740741): -log10 = 0.0321700.
    # 700 / 167 = 4.19162: q = 4.
    e1 = 501000 * 10 / (260 * 167)
    p1, p1w, p2 = (format(-math.log10(x) + 0.0, ".6g") for x in (poisson_cdf(2, e1), poisson_cdf(4, e1), math.exp(-1000 / 13500)))
    assert (format(e1, ".6g"), p2) == ("115.385", "0.03217") and p1.startswith("46.") and p1w.startswith("43.")
    assert read(bed) == (f"chr1\t1000\t1400\tGENE1\t11\t1100\t2\t1\t115.385\t{p1}\n"
                         "chr2\t0\t200\t.\t1\t0\t0\t0\t0.0740741\t0.03217\n")
    assert read(wbed) == (f"chr1\t1000\t1200\tGENE1\t2\t4.19162\t115.385\t{p1w}\n"
                          "chr2\t0\t200\t.\t0\t0\t0.0740741\t0.03217\n")
    assert read(tsv) == ("contig\tstart\tstop\tname\tmean_length\tglobal_mean\twindows\ttested\tcalled\thotspots\tdropped\tbases\n"
                         "chr1\t100\t5100\tGENE1\t167\t71.5439\t246\t246\t11\t1\t0\t400\n"
                         "chr1\t7\t150\ttiny\t167\t71.5439\t0\t0\t0\t0\t0\t0\n"
                         "chr2\t0\t3000\t.\t100\tnan\t141\t141\t1\t1\t2\t200\n")
    assert format(73261 / 1024, ".6g") == "71.5439"
    none = utils.IfsHotspots([("chr1", 0, 10, "g")], np.zeros(0, utils.HOTSPOT_DTYPE), np.zeros(0, utils.IFS_WINDOW_DTYPE),
                             np.zeros((1, 6), np.int64), np.array([1]), np.array([0]), 20, 10)
    writers.write_hotspot_rows(bed, none)  # nothing called: two empty files, and a summary of one row
    writers.write_hotspot_windows(wbed, none)
    writers.write_hotspot_summary(tsv, none)
    assert read(bed) == "" and read(wbed) == "" and read(tsv).splitlines()[1:] == ["chr1\t0\t10\tg\t1\tnan\t0\t0\t0\t0\t0\t0"]
    for fn, bad in ((writers.write_hotspot_rows, "hot.tsv"), (writers.write_hotspot_windows, "win.tsv"), (writers.write_hotspot_summary, "s.bed")):
        with pytest.raises(ValueError, match="suffix"):
            fn(str(tmp_path / bad), res)


def test_null_ctx_is_invalid_and_hands_out_nothing():
    import ctypes as C
    from finaletoolkit_amd import _lib as L
    lib = L.load()
    for name in ("ftk_ifs_hotspots", "ftk_ifs_track", "ftk_ifs_totals"):
        assert name in L.EXPORTS and hasattr(lib, name)
    iv = np.array([0, 8], np.int64)
    thr = flat_table(1)
    stats = np.full(6, 7, np.int64)
    ptrs = [C.c_void_p(1) for _ in range(17)]
    nw, nh = C.c_int64(7), C.c_int64(7)
    outs = [C.byref(p) for p in ptrs[:8]] + [C.byref(nw)] + [C.byref(p) for p in ptrs[8:]] + [C.byref(nh), L.ptr(stats)]
    assert lib.ftk_ifs_hotspots(None, 0, L.ptr(iv[:1]), L.ptr(iv[1:]), 1, 1000, 20, 10, 167, 125, 250, 0, L.ptr(thr), len(thr), 0, 20, 1,
                                -1, -1, 30, *outs) == L.FTK_ERR_INVALID
    assert lib.ftk_last_error(None)
    assert np.all(stats == 7) and nw.value == 7 and nh.value == 7 and all(p.value == 1 for p in ptrs)
    n = np.full(4, 7, np.int32)
    assert lib.ftk_ifs_track(None, 0, L.ptr(iv[:1]), L.ptr(iv[1:]), 1, L.ptr(iv[:1]), 1000, 20, 10, 167, -1, -1, 30, L.ptr(n),
                             L.ptr(stats)) == L.FTK_ERR_INVALID
    assert lib.ftk_ifs_totals(None, 0, 1000, -1, -1, 30, C.byref(nw), C.byref(nh)) == L.FTK_ERR_INVALID
    assert np.all(n == 7) and np.all(stats == 7) and nw.value == 7


def test_symbols_are_declared_and_the_files_are_built():
    text = open(os.path.join(ROOT, "include", "ftk.h")).read()
    m = re.search(r"^int ftk_ifs_hotspots\(([^;]*)\);", text, re.M)
    assert m, "ftk_ifs_hotspots is not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    kinds, names = [" ".join(a.split()[:-1]) for a in args], [a.split()[-1] for a in args]
    assert names[:20] == ["ctx", "contig_id", "iv_start", "iv_stop", "n_iv", "chrom_size", "step", "m", "mean_len", "h1", "h2", "min_count",
                          "thr", "n_thr", "global_mean", "join", "min_windows", "min_len", "max_len", "mapq_min"]
    assert names[20:] == ["w_run", "w_pos", "w_count", "w_ifs", "w_bg1", "w_nb1", "w_bg2", "w_nb2", "n_windows", "h_run", "h_start", "h_stop",
                          "h_n_windows", "h_summit", "h_ifs", "h_count", "h_bg1", "h_nb1", "n_hotspots", "stats"]
    assert kinds[20:] == ["int32_t**", "int64_t**", "int32_t**", "int64_t**", "int64_t**", "int32_t**", "int64_t**", "int32_t**", "int64_t*",
                          "int32_t**", "int64_t**", "int64_t**", "int32_t**", "int64_t**", "int64_t**", "int32_t**", "int64_t**", "int32_t**",
                          "int64_t*", "int64_t*"]
    assert re.search(r"^int ftk_ifs_track\(", text, re.M) and re.search(r"^int ftk_ifs_totals\(", text, re.M)
    assert "---- IFS hotspots" in text and "FTK_IFS_MAX_REACH 1024" in text and "B_h m 2^10 >= t n_b_h L" in text
    makefile = open(os.path.join(ROOT, "finaletoolkit_amd", "csrc", "Makefile")).read()
    assert "ftk_hotspots.hip" in makefile.split("SRC :=")[1].splitlines()[0]  # (resource-usage walks the .hip files of SRC)
    api = open(os.path.join(ROOT, "finaletoolkit_amd", "csrc", "ftk_api.hip")).read()
    assert '#include "ftk_api_hotspots.inc"' in api
    for name in ("ftk_hotspots.hip", "ftk_hotspots.h", "ftk_api_hotspots.inc"):
        assert os.path.exists(os.path.join(ROOT, "finaletoolkit_amd", "csrc", name))


def test_flat_names_resolve():
    import finaletoolkit_amd as f
    from finaletoolkit_amd import utils
    assert f.frag_hotspots is utils.frag_hotspots and f.IfsHotspots is utils.IfsHotspots and f.ifs_thresholds is utils.ifs_thresholds
    names = {"frag_hotspots", "IfsHotspots", "ifs_thresholds"}
    assert names <= set(dir(f)) and names <= set(utils.__all__) and names <= set(f._FLAT_BY_MODULE["utils"])
    eng = __import__("finaletoolkit_amd.engine", fromlist=["Engine"]).Engine
    assert hasattr(eng, "ifs_hotspots") and hasattr(eng, "ifs_track") and hasattr(eng, "ifs_totals")
