"""CPU: the host side of the preferred ends - the numpy restatement of the rule on examples worked by hand, the Poisson
threshold table, the argument errors ``frag_preferred_ends`` raises before it touches the engine, the command line's
arguments, the text of both writers, the flat names and the C symbol.  The kernels are held against the restatement in
``tests/test_gpu_preferred_ends.py``."""
import gzip
import inspect
import math
import os
import re

import numpy as np
import pytest

from tests.prefends_helpers import (CALL_DTYPE, end_tracks, flat_table, preferred_ends_ref, track_calls, window_totals)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_on_examples_worked_by_hand():
    # a contig of 10 bases.  (0, 3) twice: U on 0, D on 2.  (4, 5), one base long: both ends on 4.  (7, 12) reaches beyond
    # the contig: U on 7, its D end (base 11) does not exist.  (9, 10): both ends on 9.  (5, 5) and (6, 4) are no fragments,
    # (1, 2) has mapq 10.
    start = np.array([0, 0, 1, 4, 5, 6, 7, 9])
    end = np.array([3, 3, 2, 5, 5, 4, 12, 10])
    mapq = np.array([60, 60, 10, 60, 60, 60, 60, 30])
    u, d = end_tracks(start, end, mapq, 10)
    assert u.tolist() == [2, 0, 0, 0, 1, 0, 0, 1, 0, 1] and d.tolist() == [0, 0, 2, 0, 1, 0, 0, 0, 0, 1]
    e = u + d  # 2 0 2 0 2 0 0 1 0 2: the fragment of length 1 gives e = 2 on base 4
    total, n_w = window_totals(e, 2)
    # n_w is clipped at both contig ends: base 0 sees [0, 2], base 1 [0, 3], base 8 [6, 9], base 9 [7, 9]
    assert n_w.tolist() == [3, 4, 5, 5, 5, 5, 5, 5, 4, 3]
    assert total.tolist() == [4, 4, 6, 4, 4, 3, 3, 3, 3, 3]
    # thr[k] = 1 << 20: called iff T <= n_w.  base 0: 4 > 3.  base 2: 6 > 5.  base 4: 4 <= 5.  base 9: 3 <= 3, equality calls.
    tested, called, _, _ = track_calls(e, 2, 2, flat_table(1))
    assert np.flatnonzero(tested).tolist() == [0, 2, 4, 9] and np.flatnonzero(called).tolist() == [4, 9]
    # one unit less on the right-hand side and base 9 is out: 3 * 2^20 > (2^20 - 1) * 3
    lower = flat_table(1)
    lower[1:] -= np.uint64(1)
    assert np.flatnonzero(track_calls(e, 2, 2, lower)[1]).tolist() == [4]
    # min_count = 1 also tests base 7 (e = 1): 3 <= 5
    assert np.flatnonzero(track_calls(e, 2, 1, flat_table(1))[1]).tolist() == [4, 7, 9]
    # the clamp: with three entries e = 2 reads thr[2]; with two entries it reads thr[1], as e = 1 does
    assert np.flatnonzero(track_calls(e, 2, 1, np.array([0, 0, 1 << 20], np.uint64))[1]).tolist() == [4, 9]
    assert np.flatnonzero(track_calls(e, 2, 1, np.array([0, 1 << 20, 0], np.uint64))[1]).tolist() == [7]
    assert np.flatnonzero(track_calls(e, 2, 1, np.array([0, 1 << 20], np.uint64))[1]).tolist() == [4, 7, 9]
    many = np.array([0, 9, 0], np.int64)  # e = 9 >= n_thr = 4: the last entry, T = 9 <= 3 * 3
    assert track_calls(many, 1, 1, np.array([0, 0, 0, 3 << 20], np.uint64))[1].tolist() == [False, True, False]
    assert not track_calls(many, 1, 1, np.array([0, 3 << 20, 3 << 20, 0], np.uint64))[1].any()  # an entry of 0: never
    # the whole call, combined: runs [0, 10), [4, 5), the empty [3, 3) and [9, 10); records ordered by (run, pos, kind)
    calls, stats = preferred_ends_ref(start, end, mapq, [0, 4, 3, 9], [10, 5, 3, 10], 10, half=2, thresholds=flat_table(1))
    assert calls.dtype == CALL_DTYPE
    assert calls.tolist() == [(0, 4, 2, 2, 4, 5), (0, 9, 2, 2, 3, 3), (1, 4, 2, 2, 4, 5), (3, 9, 2, 2, 3, 3)]
    assert stats.tolist() == [[5, 4, 4, 0, 2, 0], [1, 1, 1, 0, 1, 0], [0, 0, 0, 0, 0, 0], [1, 1, 1, 0, 1, 0]]
    # split, min_count 1: U track 2 0 0 0 1 0 0 1 0 1, D track 0 0 2 0 1 0 0 0 0 1, each against its own total.
    # U totals: base 0: 2 of 3, base 4: 1 of 5, base 7: 2 of 5, base 9: 2 of 3.  D totals: base 2: 3 of 5, base 4: 3 of 5, base 9: 1 of 3.
    calls, stats = preferred_ends_ref(start, end, mapq, [0], [10], 10, half=2, mode="split", min_count=1, thresholds=flat_table(1))
    assert calls.tolist() == [(0, 0, 0, 2, 2, 3), (0, 2, 1, 2, 3, 5), (0, 4, 0, 1, 1, 5), (0, 4, 1, 1, 3, 5), (0, 7, 0, 1, 2, 5),
                              (0, 9, 0, 1, 2, 3), (0, 9, 1, 1, 1, 3)]
    assert stats.tolist() == [[5, 4, 4, 3, 4, 3]]
    # filters: lengths 3 3 1 1 5 1 (of the kept) - min_length 2 leaves (0, 3) twice and (7, 12)
    u, d = end_tracks(start, end, mapq, 10, min_len=2, max_len=5)
    assert u.tolist() == [2, 0, 0, 0, 0, 0, 0, 1, 0, 0] and d.tolist() == [0, 0, 2, 0, 0, 0, 0, 0, 0, 0]
    assert end_tracks(start, end, mapq, 10, max_len=4)[0].tolist() == [2, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    assert end_tracks(start, end, mapq, 10, mapq_min=31)[0].tolist() == [2, 0, 0, 0, 1, 0, 0, 1, 0, 0]
    assert end_tracks(start, end, mapq, 10, mapq_min=10)[0].tolist() == [2, 1, 0, 0, 1, 0, 0, 1, 0, 1]


def test_threshold_table():
    from scipy.special import gammainc
    from finaletoolkit_amd import utils
    for alpha, n in ((0.01, 256), (0.001, 64), (0.05, 2)):
        thr = utils.preferred_end_thresholds(alpha, n)
        assert thr.dtype == np.uint64 and thr.shape == (n,) and thr[0] == 0
        assert np.all(np.diff(thr.astype(np.int64)) > 0) and int(thr[-1]) < 1 << 40
        assert abs(int(thr[1]) / 2 ** 20 + math.log(1 - alpha)) < 1e-6  # P(X >= 1) = 1 - exp(-m)
        k = np.arange(1, n, dtype=np.float64)
        q = thr[1:].astype(np.float64)
        assert np.all(gammainc(k, q / 2 ** 20) < alpha)
        assert np.all(alpha <= gammainc(k, (q + 2) / 2 ** 20))  # (one unit of slack covers float64 at the boundary)
    assert np.array_equal(utils.preferred_end_thresholds(), utils.preferred_end_thresholds(0.01, 256))
    for bad in (dict(alpha=0.0), dict(alpha=1.0), dict(alpha=-0.1), dict(n=1), dict(n=4097)):
        with pytest.raises(ValueError):
            utils.preferred_end_thresholds(**bad)


@pytest.mark.parametrize("alpha", [0.01, 0.001])
def test_threshold_table_at_40_digits(alpha):
    mp = pytest.importorskip("mpmath")
    from finaletoolkit_amd import utils
    thr = utils.preferred_end_thresholds(alpha, 256)
    with mp.workdps(40):
        level, unit = mp.mpf(alpha), mp.mpf(2) ** 20

        def tail(k, q):  # P(X >= k | Poisson(q / 2^20))
            return mp.gammainc(k, 0, mp.mpf(q) / unit, regularized=True)
        for k in range(1, 256):
            q = int(thr[k])
            assert tail(k, q) < level <= tail(k, q + 1), k


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
        (dict(half_window=0), "half_window"),
        (dict(half_window=2049), "half_window"),
        (dict(alpha=0.0), "alpha"),
        (dict(alpha=1.0), "alpha"),
        (dict(min_count=0), "min_count"),
        (dict(min_length=-1), "min_length"),
        (dict(max_length=-1), "max_length"),
        (dict(min_length=200, max_length=100), "min_length"),
        (dict(chunk_size=0), "chunk_size"),
    ]
    for kwargs, word in cases:
        with pytest.raises(ValueError, match=word):
            utils.frag_preferred_ends(bam, **kwargs)
    with pytest.raises(ValueError, match="chrom_sizes"):  # a fragment file carries no lengths
        utils.frag_preferred_ends(str(tmp_path / "absent.frag.gz"))
    sizes = tmp_path / "c.sizes"
    sizes.write_text("chr2\t1000\n")
    bed = tmp_path / "iv.bed"
    bed.write_text("chr1\t0\t5000\tg\n")
    with pytest.raises(ValueError, match="chrom_sizes"):  # the interval's contig is not in the sizes file
        utils.frag_preferred_ends(str(tmp_path / "absent.frag.gz"), str(bed), chrom_sizes=str(sizes))
    # the limits themselves pass
    utils._check_preferred_ends_args(bam, None, "o.bed.gz", "s.tsv.gz", 2048, 0.5, 1, 0, 0, 1)
    utils._check_preferred_ends_args(bam, None, None, None, 1, 1e-9, 100, None, None, 1 << 40)


def test_signature_and_command_line():
    from finaletoolkit_amd import utils
    from finaletoolkit_amd.engine import Engine
    from finaletoolkit_amd.prefends import build_parser
    sig = inspect.signature(utils.frag_preferred_ends)
    assert list(sig.parameters) == ["input_file", "interval_file", "chrom_sizes", "output_file", "summary_file", "half_window", "alpha",
                                    "min_count", "split", "min_length", "max_length", "quality_threshold", "chunk_size", "workers",
                                    "verbose"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(interval_file=None, chrom_sizes=None, output_file=None, summary_file=None, half_window=500, alpha=0.01,
                            min_count=2, split=False, min_length=None, max_length=None, quality_threshold=30, chunk_size=1 << 22,
                            workers=None, verbose=False)
    ap = build_parser()
    args = vars(ap.parse_args(["in.bam", "out.bed"]))
    assert set(args) == set(sig.parameters)
    assert {k: args[k] for k in defaults if k != "output_file"} == {k: v for k, v in defaults.items() if k != "output_file"}
    full = vars(ap.parse_args(["in.frag.gz", "out.bed.gz", "--intervals", "genes.bed", "--summary", "s.tsv", "--chrom-sizes", "c.sizes",
                               "--half-window", "250", "--alpha", "0.001", "--min-count", "3", "--split", "--min-length", "35",
                               "--max-length", "80", "-q", "20", "--chunk-size", "65536", "-w", "3", "-v"]))
    assert full == dict(input_file="in.frag.gz", output_file="out.bed.gz", interval_file="genes.bed", summary_file="s.tsv",
                        chrom_sizes="c.sizes", half_window=250, alpha=0.001, min_count=3, split=True, min_length=35, max_length=80,
                        quality_threshold=20, chunk_size=65536, workers=3, verbose=True)
    assert utils.PreferredEnds._fields == ("intervals", "calls", "stats", "share")
    assert utils.PREFERRED_END_DTYPE.names == ("interval", "pos", "kind", "count", "total", "n_w")
    call = inspect.signature(Engine.preferred_ends)
    assert list(call.parameters) == ["self", "name", "starts", "stops", "chrom_size", "half", "mode", "min_count", "thresholds",
                                     "min_length", "max_length", "quality_threshold"]
    assert [p.default for p in list(call.parameters.values())[5:]] == [500, "combined", 2, None, None, None, 30]
    assert Engine.PREFERRED_END_DTYPE.names == CALL_DTYPE.names
    assert [Engine.PREFERRED_END_DTYPE[f] for f in CALL_DTYPE.names] == [CALL_DTYPE[f] for f in CALL_DTYPE.names]
    thr = inspect.signature(utils.preferred_end_thresholds)
    assert [(k, v.default) for k, v in thr.parameters.items()] == [("alpha", 0.01), ("n", 256)]


def hand_made():
    from finaletoolkit_amd import utils
    calls = np.array([(0, 100, 2, 3, 10, 1001), (0, 101, 0, 2, 1, 5), (2, 0, 1, 70000, 70001, 3)], utils.PREFERRED_END_DTYPE)
    stats = np.array([[9, 2, 4, 1, 3, 2], [0, 0, 0, 0, 0, 0], [3, 70000, 1, 0, 1, 1]], np.int64)
    return utils.PreferredEnds([("chr1", 100, 5100, "GENE1"), ("chr1", 7, 900, "tiny"), ("chr2", 0, 3000, ".")], calls, stats,
                               np.array([0.25, np.nan, 1 / 3]))


@pytest.mark.parametrize("gz", [False, True])
def test_writer_text(tmp_path, gz):
    from finaletoolkit_amd import utils, writers
    res = hand_made()
    bed, tsv = str(tmp_path / ("calls.bed" + ".gz" * gz)), str(tmp_path / ("summary.tsv" + ".gz" * gz))
    writers.write_preferred_end_rows(bed, res)
    writers.write_preferred_end_summary(tsv, res)

    def read(path):
        return gzip.open(path, "rt").read() if gz else open(path).read()
    # 10 / 1001 = 0.00999001, P(X >= 3) = 1.6492e-07.  1 / 5 = 0.2, P(X >= 2) = 1 - 1.2 exp(-0.2) = 0.0175231, -log10: 1.75639.
    # 70001 / 3: P(X >= 70000) underflows to 0, written as inf.
    assert read(bed) == ("chr1\t100\t101\tGENE1\tB\t3\t10\t0.00999001\t6.78271\n"
                         "chr1\t101\t102\tGENE1\tU\t2\t1\t0.2\t1.75639\n"
                         "chr2\t0\t1\t.\tD\t70000\t70001\t23333.7\tinf\n")
    assert format(-math.log10(1 - 1.2 * math.exp(-0.2)), ".6g") == "1.75639"
    assert read(tsv) == ("contig\tstart\tstop\tname\tu_ends\td_ends\ttested_a\ttested_b\tcalls_a\tcalls_b\tshare\n"
                         "chr1\t100\t5100\tGENE1\t9\t2\t4\t1\t3\t2\t0.25\n"
                         "chr1\t7\t900\ttiny\t0\t0\t0\t0\t0\t0\tnan\n"
                         "chr2\t0\t3000\t.\t3\t70000\t1\t0\t1\t1\t0.333333\n")
    none = utils.PreferredEnds([("chr1", 0, 10, "g")], np.zeros(0, utils.PREFERRED_END_DTYPE), np.zeros((1, 6), np.int64),
                               np.array([np.nan]))
    writers.write_preferred_end_rows(bed, none)  # zero calls: an empty file, and a summary of one row
    writers.write_preferred_end_summary(tsv, none)
    assert read(bed) == "" and read(tsv).splitlines()[1:] == ["chr1\t0\t10\tg\t0\t0\t0\t0\t0\t0\tnan"]
    with pytest.raises(ValueError, match="suffix"):
        writers.write_preferred_end_rows(str(tmp_path / "calls.tsv"), res)
    with pytest.raises(ValueError, match="suffix"):
        writers.write_preferred_end_summary(str(tmp_path / "summary.bed"), res)


def test_null_ctx_is_invalid_and_hands_out_nothing():
    import ctypes as C
    from finaletoolkit_amd import _lib as L
    lib = L.load()
    assert "ftk_preferred_ends" in L.EXPORTS and hasattr(lib, "ftk_preferred_ends")
    iv = np.array([0, 8], np.int64)
    thr = flat_table(1)
    stats = np.full(6, 7, np.int64)
    ptrs = [C.c_void_p(1) for _ in range(6)]
    n = C.c_int64(7)
    outs = [C.byref(p) for p in ptrs] + [C.byref(n), L.ptr(stats)]
    assert lib.ftk_preferred_ends(None, 0, L.ptr(iv[:1]), L.ptr(iv[1:]), 1, 1000, 500, 0, 2, L.ptr(thr), len(thr), -1, -1, 30,
                                  *outs) == L.FTK_ERR_INVALID
    assert lib.ftk_last_error(None)
    assert np.all(stats == 7) and n.value == 7 and all(p.value == 1 for p in ptrs)
    assert (L.PREFENDS_MAX_HALF, L.PREFENDS_MAX_THR) == (2048, 4096) and L.PREFENDS_TILE > 0


def test_symbol_is_declared_in_the_header():
    text = open(os.path.join(ROOT, "include", "ftk.h")).read()
    m = re.search(r"^int ftk_preferred_ends\(([^;]*)\);", text, re.M)
    assert m, "ftk_preferred_ends is not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    kinds, names = [" ".join(a.split()[:-1]) for a in args], [a.split()[-1] for a in args]
    assert kinds == ["ftk_ctx*", "int", "const int64_t*", "const int64_t*", "int64_t", "int64_t", "int32_t", "int32_t", "int32_t",
                     "const uint64_t*", "int32_t", "int32_t", "int32_t", "int32_t", "int32_t**", "int64_t**", "int32_t**", "int32_t**",
                     "int64_t**", "int32_t**", "int64_t*", "int64_t*"]
    assert names == ["ctx", "contig_id", "iv_start", "iv_stop", "n_iv", "chrom_size", "half", "mode", "min_count", "thr", "n_thr",
                     "min_len", "max_len", "mapq_min", "run", "pos", "kind", "count", "total", "n_w", "n_calls", "stats"]
    assert "---- preferred ends" in text and "FTK_PREFENDS_MAX_HALF 2048" in text and "thr[min(e(b), n_thr - 1)]" in text
    makefile = open(os.path.join(ROOT, "finaletoolkit_amd", "csrc", "Makefile")).read()
    assert "ftk_prefends.hip" in makefile
    api = open(os.path.join(ROOT, "finaletoolkit_amd", "csrc", "ftk_api.hip")).read()
    assert '#include "ftk_api_prefends.inc"' in api


def test_flat_names_resolve():
    import finaletoolkit_amd as f
    from finaletoolkit_amd import utils
    assert f.frag_preferred_ends is utils.frag_preferred_ends and f.PreferredEnds is utils.PreferredEnds
    assert f.preferred_end_thresholds is utils.preferred_end_thresholds
    names = {"frag_preferred_ends", "PreferredEnds", "preferred_end_thresholds"}
    assert names <= set(dir(f)) and names <= set(utils.__all__) and names <= set(f._FLAT_BY_MODULE["utils"])
    eng = __import__("finaletoolkit_amd.engine", fromlist=["Engine"]).Engine
    assert hasattr(eng, "preferred_ends")
