"""CPU: the host side of the nucleosome calls - the argument errors ``frag_wps_peaks`` raises before it touches the engine,
the text of ``writers.write_wps_peaks_rows`` / ``write_wps_peaks_summary``, the command line's arguments, the flat names,
the C symbols, and the numpy restatement of the rule on examples worked by hand.  The kernels are held against the
restatement in ``tests/test_gpu_wps_peaks.py``."""
import gzip
import inspect
import os
import re

import numpy as np
import pytest

from tests.peaks_helpers import peaks_ref, peaks_ref_runs, regions_of, windows_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_argument_errors_come_before_any_engine_use(tmp_path, monkeypatch):
    from finaletoolkit_amd import utils

    def no_engine(*a, **k):
        raise AssertionError("the engine was asked for")
    monkeypatch.setattr(utils, "get_engine", no_engine)
    bam = str(tmp_path / "absent.bam")  # it does not exist: nothing may open it
    cases = [
        (dict(output_file=str(tmp_path / "out.tsv")), "output_file"),
        (dict(output_file=str(tmp_path / "out.bed.bz2")), "output_file"),
        (dict(summary_file=str(tmp_path / "out.bed")), "summary_file"),
        (dict(median_window_size=999), "median_window_size"),
        (dict(median_window_size=0), "median_window_size"),
        (dict(median_window_size=2050), "median_window_size"),
        (dict(savgol_window_size=20), "savgol_window_size"),
        (dict(savgol_window_size=1), "savgol_window_size"),
        (dict(savgol_window_size=5, savgol_poly_deg=5), "savgol_poly_deg"),
        (dict(max_gap=-1), "max_gap"),
        (dict(max_gap=64), "max_gap"),
        (dict(min_region=0), "region"),
        (dict(min_region=151), "region"),
        (dict(short_max=451), "region"),
        (dict(max_region=1025), "region"),
        (dict(chunk_size=0), "chunk_size"),
    ]
    for kwargs, word in cases:
        with pytest.raises(ValueError, match=word):
            utils.frag_wps_peaks(bam, **kwargs)
    with pytest.raises(ValueError, match="chrom_sizes"):  # a fragment file carries no lengths
        utils.frag_wps_peaks(str(tmp_path / "absent.frag.gz"))
    sizes = tmp_path / "c.sizes"
    sizes.write_text("chr2\t1000\n")
    bed = tmp_path / "iv.bed"
    bed.write_text("chr1\t0\t5000\tg\n")
    with pytest.raises(ValueError, match="chrom_sizes"):  # the interval's contig is not in the sizes file
        utils.frag_wps_peaks(str(tmp_path / "absent.frag.gz"), str(bed), chrom_sizes=str(sizes))
    # the limits themselves pass, and go on to the files (no Savitzky-Golay: its window is not looked at)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="median_window_size"):
        utils.frag_wps_peaks(bam, median_window_size=3)
    utils._check_wps_peaks_args(bam, None, "o.bed.gz", "s.tsv.gz", 2048, 20, 9, False, 63, 1, 1, 1024, 1)
    utils._check_wps_peaks_args(bam, None, None, None, 2, 3, 2, True, 0, 1024, 1024, 1024, 1 << 40)


def test_signature_and_command_line():
    from finaletoolkit_amd import utils
    from finaletoolkit_amd.engine import Engine
    from finaletoolkit_amd.peaks import build_parser
    sig = inspect.signature(utils.frag_wps_peaks)
    assert list(sig.parameters) == ["input_file", "interval_file", "chrom_sizes", "output_file", "summary_file", "window_size",
                                    "min_length", "max_length", "quality_threshold", "median_window_size", "savgol_window_size",
                                    "savgol_poly_deg", "savgol", "max_gap", "min_region", "short_max", "max_region", "chunk_size",
                                    "workers", "verbose"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(interval_file=None, chrom_sizes=None, output_file=None, summary_file=None, window_size=120, min_length=120,
                            max_length=180, quality_threshold=30, median_window_size=1000, savgol_window_size=21, savgol_poly_deg=2,
                            savgol=True, max_gap=5, min_region=50, short_max=150, max_region=450, chunk_size=1 << 20, workers=None,
                            verbose=False)
    ap = build_parser()
    args = vars(ap.parse_args(["in.bam", "out.bed"]))
    assert set(args) == set(sig.parameters)
    assert {k: args[k] for k in defaults if k != "output_file"} == {k: v for k, v in defaults.items() if k != "output_file"}
    full = vars(ap.parse_args(["in.frag.gz", "out.bed.gz", "--intervals", "genes.bed", "--summary", "s.tsv", "--chrom-sizes", "c.sizes",
                               "--window-size", "60", "--min-length", "35", "--max-length", "80", "-q", "20", "--median-window-size",
                               "500", "--savgol-window-size", "11", "--savgol-poly-deg", "3", "--no-savgol", "--max-gap", "3",
                               "--min-region", "40", "--short-max", "140", "--max-region", "400", "--chunk-size", "65536", "-w", "3",
                               "-v"]))
    assert full == dict(input_file="in.frag.gz", output_file="out.bed.gz", interval_file="genes.bed", summary_file="s.tsv",
                        chrom_sizes="c.sizes", window_size=60, min_length=35, max_length=80, quality_threshold=20,
                        median_window_size=500, savgol_window_size=11, savgol_poly_deg=3, savgol=False, max_gap=3, min_region=40,
                        short_max=140, max_region=400, chunk_size=65536, workers=3, verbose=True)
    assert utils.WpsPeaks._fields == ("intervals", "calls", "stats", "callable", "median_spacing")
    assert utils.WPS_PEAK_DTYPE.names == ("interval", "start", "stop", "summit", "height", "area")
    track = inspect.signature(Engine.track_peaks)
    assert list(track.parameters) == ["self", "scores", "offsets", "skip", "max_gap", "min_region", "short_max", "max_region"]
    assert [p.default for p in list(track.parameters.values())[3:]] == [0, 5, 50, 150, 450]
    fused = inspect.signature(Engine.wps_peaks)
    assert list(fused.parameters) == ["self", "name", "starts", "stops", "chrom_size", "window_size", "min_length", "max_length",
                                      "quality_threshold", "median_window_size", "savgol_window_size", "savgol_poly_deg", "savgol",
                                      "max_gap", "min_region", "short_max", "max_region", "batch_bases"]
    assert [p.default for p in list(fused.parameters.values())[5:]] == [120, 120, 180, 30, 1000, 21, 2, True, 5, 50, 150, 450, None]
    assert Engine.PEAK_DTYPE.names == ("run", "start", "stop", "summit", "height", "area")


def hand_made():
    from finaletoolkit_amd import utils
    calls = np.array([(0, 1100, 1240, 1171, 12.5, 1234.5678), (0, 1290, 1431, 1300, 1 / 3, 2.0e-7), (2, 50, 51, 50, 1e10, 1e10)],
                     utils.WPS_PEAK_DTYPE)
    stats = np.array([[9, 2, 4, 1, 0, 2], [0, 0, 0, 0, 0, 0], [3, 0, 1, 0, 1, 1]], np.int64)
    return utils.WpsPeaks([("chr1", 100, 5100, "GENE1"), ("chr1", 7, 900, "tiny"), ("chr2", 0, 3000, ".")], calls, stats,
                          np.array([3980, 0, 1980], np.int64), np.array([190.0, np.nan, np.nan]))


@pytest.mark.parametrize("gz", [False, True])
def test_writer_text(tmp_path, gz):
    from finaletoolkit_amd import utils, writers
    res = hand_made()
    bed, tsv = str(tmp_path / ("calls.bed" + ".gz" * gz)), str(tmp_path / ("summary.tsv" + ".gz" * gz))
    writers.write_wps_peaks_rows(bed, res)
    writers.write_wps_peaks_summary(tsv, res)

    def read(path):
        return gzip.open(path, "rt").read() if gz else open(path).read()
    assert read(bed) == ("chr1\t1100\t1240\tGENE1\t1170\t1171\t12.5\t1234.57\n"
                         "chr1\t1290\t1431\tGENE1\t1360\t1300\t0.333333\t2e-07\n"
                         "chr2\t50\t51\t.\t50\t50\t1e+10\t1e+10\n")
    assert read(tsv) == ("contig\tstart\tstop\tname\tcallable\tregions\topen\tshort\tlong\tflat\tcalls\tmedian_spacing\n"
                         "chr1\t100\t5100\tGENE1\t3980\t9\t2\t4\t1\t0\t2\t190\n"
                         "chr1\t7\t900\ttiny\t0\t0\t0\t0\t0\t0\t0\tnan\n"
                         "chr2\t0\t3000\t.\t1980\t3\t0\t1\t0\t1\t1\tnan\n")
    none = utils.WpsPeaks([("chr1", 0, 10, "g")], np.zeros(0, utils.WPS_PEAK_DTYPE), np.zeros((1, 6), np.int64), np.zeros(1, np.int64),
                          np.array([np.nan]))
    writers.write_wps_peaks_rows(bed, none)  # zero calls: an empty file, and a summary of one row
    writers.write_wps_peaks_summary(tsv, none)
    assert read(bed) == "" and read(tsv).splitlines()[1:] == ["chr1\t0\t10\tg\t0\t0\t0\t0\t0\t0\t0\tnan"]
    with pytest.raises(ValueError, match="suffix"):
        writers.write_wps_peaks_rows(str(tmp_path / "calls.tsv"), res)
    with pytest.raises(ValueError, match="suffix"):
        writers.write_wps_peaks_summary(str(tmp_path / "summary.bed"), res)


def test_median_spacing_is_between_call_centres():
    from finaletoolkit_amd import utils
    starts, stops = np.array([100, 290, 480, 700]), np.array([201, 390, 581, 800])  # centres 150, 340, 530, 750
    assert utils._median_spacing(starts, stops) == 190.0
    assert np.isnan(utils._median_spacing(starts[:1], stops[:1])) and np.isnan(utils._median_spacing(starts[:0], stops[:0]))
    assert utils._median_spacing(starts[2:], stops[2:]) == 220.0


def test_null_ctx_is_invalid_and_hands_out_nothing():
    import ctypes as C
    from finaletoolkit_amd import _lib as L
    lib = L.load()
    for sym in ("ftk_track_peaks", "ftk_wps_peaks", "ftk_buffer_free"):
        assert sym in L.EXPORTS and hasattr(lib, sym)
    scores, offs = np.arange(8, dtype=np.float64), np.array([0, 8], np.int64)
    stats = np.full(6, 7, np.int64)
    ptrs = [C.c_void_p(1) for _ in range(6)]
    n = C.c_int64(7)
    outs = [C.byref(p) for p in ptrs] + [C.byref(n), L.ptr(stats)]
    assert lib.ftk_track_peaks(None, L.ptr(scores), L.ptr(offs), 1, 0, 5, 50, 150, 450, *outs) == L.FTK_ERR_INVALID
    assert lib.ftk_last_error(None)
    assert lib.ftk_wps_peaks(None, 0, L.ptr(offs[:1]), L.ptr(offs[1:]), 1, 1000, 120, 120, 180, 30, 1000, 0, None, None, 5, 50, 150,
                             450, 0, *outs) == L.FTK_ERR_INVALID
    assert np.all(stats == 7) and n.value == 7 and all(p.value == 1 for p in ptrs)
    assert (L.PEAKS_MAX_GAP, L.PEAKS_MAX_REGION) == (63, 1024) and L.PEAKS_TILE > 0


def test_symbols_are_declared_in_the_header():
    text = open(os.path.join(ROOT, "include", "ftk.h")).read()

    def declared(name):
        m = re.search(r"^int %s\(([^;]*)\);" % name, text, re.M)
        assert m, name + " is not declared"
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
        return [" ".join(a.split()[:-1]) for a in args], [a.split()[-1] for a in args]
    outs = ["int32_t**", "int64_t**", "int64_t**", "int64_t**", "double**", "double**", "int64_t*", "int64_t*"]
    out_names = ["run", "start", "stop", "summit", "height", "area", "n_calls", "stats"]
    kinds, names = declared("ftk_track_peaks")
    assert kinds == ["ftk_ctx*", "const double*", "const int64_t*", "int64_t", "int64_t", "int32_t", "int32_t", "int32_t", "int32_t"] + outs
    assert names == ["ctx", "scores", "offsets", "n_runs", "skip", "max_gap", "min_region", "short_max", "max_region"] + out_names
    kinds, names = declared("ftk_wps_peaks")
    assert kinds == ["ftk_ctx*", "int", "const int64_t*", "const int64_t*", "int64_t", "int64_t", "int32_t", "int32_t", "int32_t", "int32_t",
                     "int32_t", "int32_t", "const double*", "const double*", "int32_t", "int32_t", "int32_t", "int32_t", "int64_t"] + outs
    assert names == ["ctx", "contig_id", "iv_start", "iv_stop", "n_iv", "chrom_size", "window_size", "min_len", "max_len", "mapq_min",
                     "median_window", "savgol_window", "savgol_coef", "savgol_edge", "max_gap", "min_region", "short_max", "max_region",
                     "batch_bases"] + out_names
    assert "---- peaks" in text and "FTK_PEAKS_MAX_REGION 1024" in text and "the leftmost of equals" in text
    makefile = open(os.path.join(ROOT, "finaletoolkit_amd", "csrc", "Makefile")).read()
    assert "ftk_peaks.hip" in makefile
    api = open(os.path.join(ROOT, "finaletoolkit_amd", "csrc", "ftk_api.hip")).read()
    assert '#include "ftk_api_peaks.inc"' in api


def test_flat_names_resolve():
    import finaletoolkit_amd as f
    from finaletoolkit_amd import utils
    assert f.frag_wps_peaks is utils.frag_wps_peaks and f.WpsPeaks is utils.WpsPeaks
    names = {"frag_wps_peaks", "WpsPeaks"}
    assert names <= set(dir(f)) and names <= set(utils.__all__) and names <= set(f._FLAT_BY_MODULE["utils"])
    eng = __import__("finaletoolkit_amd.engine", fromlist=["Engine"]).Engine
    assert hasattr(eng, "track_peaks") and hasattr(eng, "wps_peaks")


def test_restatement_on_examples_worked_by_hand():
    #                0   1   2  3  4  5   6  7  8   9  10  11
    a = np.array([-1, -1, -1, 1, 3, 2, -1, 4, 1, -1, -1, -1], np.float64)
    # positives at 3 4 5 7 8; one position (6) between 5 and 7
    assert regions_of(a, 0, 12, 1) == [(3, 9)] and regions_of(a, 0, 12, 0) == [(3, 6), (7, 9)]
    assert regions_of(a, 4, 8, 1) == [(4, 8)] and regions_of(a, 8, 8, 1) == [] and regions_of(a, 9, 3, 1) == []
    # region [3, 9): values 1 3 2 -1 4 1, sorted -1 1 1 2 3 4, median (1 + 2) / 2 = 1.5; windows above it: [4, 6) and [7, 8)
    assert windows_of(a[3:9], 1.5) == [(1, 3), (4, 5)]
    kw = dict(max_gap=1, min_region=2, max_region=12)
    # L = 6 > short_max = 5: every window of 2 .. 5 positions - [4, 6): summit 4, height 3, area 3 + 2
    calls, stats = peaks_ref(a, short_max=5, **kw)
    assert calls == [(4, 6, 4, 3.0, 5.0)] and stats.tolist() == [1, 0, 0, 0, 0, 1]
    # L = 6 <= short_max = 6: the window of largest area, 5 against 4
    calls, stats = peaks_ref(a, short_max=6, **kw)
    assert calls == [(4, 6, 4, 3.0, 5.0)] and stats.tolist() == [1, 0, 0, 0, 0, 1]
    b = a.copy()
    b[7] = 6  # now 5 against 6: the one-position window wins, whatever its length; sorted -1 1 1 2 3 6: the median stays
    assert peaks_ref(b, short_max=6, **kw)[0] == [(7, 8, 7, 6.0, 6.0)]
    assert peaks_ref(b, short_max=5, **kw)[0] == [(4, 6, 4, 3.0, 5.0)]
    b[7] = 5  # equal areas: the leftmost
    assert peaks_ref(b, short_max=6, **kw)[0] == [(4, 6, 4, 3.0, 5.0)]
    # no window of 3 .. 5 positions: no call, and the region is not flat
    calls, stats = peaks_ref(a, max_gap=1, min_region=3, short_max=5, max_region=12)
    assert calls == [] and stats.tolist() == [1, 0, 0, 0, 0, 0]
    # the classes: short, long, open at either end (distance max_gap is open, max_gap + 1 is closed), flat
    assert peaks_ref(a, max_gap=1, min_region=7, short_max=7, max_region=12)[1].tolist() == [1, 0, 1, 0, 0, 0]
    assert peaks_ref(a, max_gap=1, min_region=2, short_max=5, max_region=5)[1].tolist() == [1, 0, 0, 1, 0, 0]
    assert peaks_ref(a, skip=2, short_max=5, **kw)[1].tolist() == [1, 1, 0, 0, 0, 0]  # r0 - lo = 1, hi - r1 = 1
    assert peaks_ref(a, skip=1, short_max=5, **kw)[1].tolist() == [1, 0, 0, 0, 0, 1]  # 2 and 2
    assert peaks_ref(a[1:], short_max=5, **kw)[1].tolist() == [1, 0, 0, 0, 0, 1]      # r0 - lo = 2
    assert peaks_ref(a[2:], short_max=5, **kw)[1].tolist() == [1, 1, 0, 0, 0, 0]      # r0 - lo = 1
    assert peaks_ref(a[:-2], short_max=5, **kw)[1].tolist() == [1, 1, 0, 0, 0, 0]     # hi - r1 = 1
    # max_gap = 0 splits it: [3, 6) median 2, window [4, 5); [7, 9) median 2.5, window [7, 8)
    calls, stats = peaks_ref(a, max_gap=0, min_region=2, short_max=5, max_region=12)
    assert calls == [(4, 5, 4, 3.0, 3.0), (7, 8, 7, 4.0, 4.0)] and stats.tolist() == [2, 0, 0, 0, 0, 2]
    flat = np.array([-1, -1, 2, 2, 2, -1, -1], np.float64)
    calls, stats = peaks_ref(flat, max_gap=0, min_region=1, short_max=5, max_region=5)
    assert calls == [] and stats.tolist() == [1, 0, 0, 0, 1, 0]
    # odd L with the median among the values: 1 3 2 -> median 2, one window [1, 2)
    odd = np.array([-1, -1, 1, 3, 2, -1, -1], np.float64)
    assert peaks_ref(odd, max_gap=0, min_region=1, short_max=5, max_region=5)[0] == [(3, 4, 3, 3.0, 3.0)]
    big = np.array([-1.0, -1.0, 1e16, 1.0, 1.0, -5.0, 0.5, 1.0, 1.0, 1e16, -1.0, -1.0])
    calls, _ = peaks_ref(big, max_gap=1, min_region=2, short_max=4, max_region=12)  # region [2, 10), median 1: windows [2, 3), [9, 10)
    assert calls == []
    calls, _ = peaks_ref(big, max_gap=1, min_region=1, short_max=4, max_region=12)
    assert calls == [(2, 3, 2, 1e16, 1e16), (9, 10, 9, 1e16, 1e16)]
    order = np.array([-1.0, -1.0, 1e16, 1.0, 1.0, -1.0, -1.0, 1.0, 1.0, 1e16, -1.0, -1.0])
    calls, _ = peaks_ref(order, max_gap=0, min_region=1, short_max=3, max_region=3)  # two regions, median 1 each: one window each
    assert calls == [(2, 3, 2, 1e16, 1e16), (9, 10, 9, 1e16, 1e16)]
    # the area is added to 0 left to right: 1e16 + 1 + 1 loses both ones, 1 + 1 + 1e16 keeps them
    low2 = np.array([-9.0, -9.0, 1e16, 1.0, 1.0, 0.25, 0.25, 0.25, -9.0, -9.0, 0.25, 0.25, 0.25, 1.0, 1.0, 1e16, -9.0, -9.0])
    calls, _ = peaks_ref(low2, max_gap=0, min_region=1, short_max=6, max_region=6)  # medians (0.25 + 1) / 2: windows of three
    assert [c[:3] for c in calls] == [(2, 5, 2), (13, 16, 15)]
    assert calls[0][4] == 1e16 and calls[1][4] == 1e16 + 2.0 and calls[0][4] != calls[1][4]
    # runs side by side: the run number leads, positions count from the run's start
    scores = np.concatenate([a, np.zeros(0), a[1:]])
    got, stats = peaks_ref_runs(scores, [0, 12, 12, 23], max_gap=1, min_region=2, short_max=5, max_region=12)
    assert got.tolist() == [(0, 4, 6, 4, 3.0, 5.0), (2, 3, 5, 3, 3.0, 5.0)] and stats[:, 5].tolist() == [1, 0, 1]
