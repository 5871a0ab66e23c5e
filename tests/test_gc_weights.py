"""CPU: the host side of the GC weights - ``gc_weights`` known answers, the ``read_gc_bias_table`` round trip,
``frag_gc_coverage``'s signature and the argument errors it raises before any file is opened, the command line of
``python -m finaletoolkit_amd.gccov``, the flat names and the four C symbols.  The kernels are held against a numpy
restatement in ``tests/test_gpu_gc_weights.py``."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ftk_frags_set_weights", "ftk_frags_weights", "ftk_frags_set_gc_weights", "ftk_weighted_window_sums")
FLAT = ("frag_gc_coverage", "gc_weights", "read_gc_bias_table")


def test_gc_weights_known_answers():
    from finaletoolkit_amd import utils
    from finaletoolkit_amd import _lib as L
    assert L.WEIGHT_ONE == 65536
    b = np.array([[1.0, 0.5, 3.0], [np.nan, 0.049, 0.05]])
    w = utils.gc_weights(b)
    assert w.dtype == np.uint32 and w.shape == b.shape
    assert w.tolist() == [[65536, 131072, 21845], [0, 0, 1310720]]  # 0.05 is kept: floor(65536 / 0.05 + 0.5)
    assert utils.gc_weights(b, min_bias=0.5).tolist() == [[65536, 131072, 21845], [0, 0, 0]]
    assert utils.gc_weights(b, min_bias=0.51).tolist() == [[65536, 0, 21845], [0, 0, 0]]
    assert utils.gc_weights(np.array([np.inf, 2.0 ** -15, 1e300]), min_bias=2.0 ** -15).tolist() == [0, 2 ** 31, 0]
    obs = np.array([[1, 2, 0], [0, 3, 4]], np.int64)
    exp = np.array([[2, 0, 0], [1, 1, 6]], np.int64)
    res = utils.GCBias(2, 3, obs, exp, utils.gc_bias_ratio(obs, exp), 10, 0, ())
    assert np.array_equal(utils.gc_weights(res), utils.gc_weights(res.bias))  # a GCBias or its table
    assert utils.gc_weights(res).tolist() == [[131072, 0, 0], [0, 21845, 98304]]
    for bad in (2.0 ** -16, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="min_bias"):
            utils.gc_weights(b, min_bias=bad)


def table_with_odd_cells():
    from finaletoolkit_amd import utils
    obs = np.zeros((3, 8), np.int64)
    exp = np.zeros((3, 8), np.int64)
    bias = np.full((3, 8), np.nan)
    cells = {(0, 0): (1, 2, 0.1), (0, 5): (3, 0, float("nan")), (1, 1): (2 ** 40, 7, 5e-324), (1, 6): (0, 9, 0.0),
             (2, 7): (5, 2 ** 41, 1.7976931348623157e308), (2, 3): (4, 4, 1 / 3)}
    for (r, g), (o, e, b) in cells.items():
        obs[r, g], exp[r, g], bias[r, g] = o, e, b
    return utils.GCBias(5, 7, obs, exp, bias, int(obs.sum()), 3, ("chrUn",))


@pytest.mark.parametrize("suffix", [".tsv", ".tsv.gz"])
def test_read_gc_bias_table_round_trip(tmp_path, suffix):
    from finaletoolkit_amd import utils, writers
    res = table_with_odd_cells()
    out = str(tmp_path / ("bias" + suffix))
    writers.write_gc_bias_table(out, res.min_length, res.observed, res.expected, res.bias)
    back = utils.read_gc_bias_table(out, 5, 7)
    assert isinstance(back, utils.GCBias) and (back.min_length, back.max_length) == (5, 7)
    assert back.observed.dtype == np.int64 and back.expected.dtype == np.int64 and back.bias.dtype == np.float64
    assert np.array_equal(back.observed, res.observed) and np.array_equal(back.expected, res.expected)
    assert np.array_equal(back.bias, res.bias, equal_nan=True)  # tiny and huge biases included: exact
    assert back.bias[1, 1] == 5e-324 and back.bias[2, 7] == 1.7976931348623157e308 and np.isnan(back.bias[0, 5])
    assert (back.n_fragments, back.n_skipped, back.skipped_contigs) == (int(res.observed.sum()), 0, ())
    assert np.isnan(back.bias[0, 1]) and back.observed[0, 1] == 0 and back.expected[0, 1] == 0  # an absent cell
    assert np.array_equal(utils.gc_weights(back), utils.gc_weights(res))
    # the same file read for other lengths: a row outside them
    for lo, hi in ((6, 7), (5, 6), (1, 4)):
        with pytest.raises(ValueError, match="outside"):
            utils.read_gc_bias_table(out, lo, hi)
    wider = utils.read_gc_bias_table(out, 4, 9)
    assert wider.observed.shape == (6, 10) and np.array_equal(wider.observed[1:4, :8], res.observed)


@pytest.mark.parametrize("min_bias", [0.05, 0.2, 2.0 ** -15])
def test_weight_table_of_a_bias_and_of_its_file(tmp_path, min_bias):
    """``utils._weight_table``: a ``GCBias`` comes back as ``gc_weights`` of it, the path of its TSV gives the same array,
    and ``min_bias`` is checked with ``gc_weights``' words.  (``bias=None`` runs ``frag_gc_bias``: the GPU tests.)"""
    from finaletoolkit_amd import utils, writers
    res = table_with_odd_cells()
    want = utils.gc_weights(res, min_bias)
    args = (5, 7, 30, 1, min_bias, None, False)
    got = utils._weight_table("no input is read", "nor a reference", res, *args)
    assert got.dtype == np.uint32 and np.array_equal(got, want) and want.any()
    out = str(tmp_path / "bias.tsv")
    writers.write_gc_bias_table(out, res.min_length, res.observed, res.expected, res.bias)
    assert np.array_equal(utils._weight_table("no input is read", "nor a reference", out, *args), want)
    for bias in (res, out):
        with pytest.raises(ValueError) as e:
            utils._weight_table("no input is read", "nor a reference", bias, 5, 7, 30, 1, 2.0 ** -16, None, False)
        assert str(e.value) == "invalid min_bias (1.52587890625e-05): at least 2**-15"


def test_signature():
    from finaletoolkit_amd import utils
    sig = inspect.signature(utils.frag_gc_coverage)
    assert list(sig.parameters) == ["input_file", "reference_file", "interval_file", "output_file", "bias", "min_length",
                                    "max_length", "quality_threshold", "intersect_policy", "min_bias", "stride", "workers",
                                    "verbose"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert all(d[k] is inspect.Parameter.empty for k in ("input_file", "reference_file", "interval_file"))
    assert d["output_file"] is None and d["bias"] is None and d["workers"] is None
    assert (d["min_length"], d["max_length"], d["quality_threshold"], d["intersect_policy"], d["min_bias"], d["stride"],
            d["verbose"]) == (100, 220, 30, "midpoint", 0.05, 1, False)
    assert utils.GCCoverage._fields == ("intervals", "count", "corrected", "n_weighted", "n_zero", "skipped_contigs")
    assert list(inspect.signature(utils.gc_weights).parameters) == ["bias", "min_bias"]
    assert list(inspect.signature(utils.read_gc_bias_table).parameters) == ["path", "min_length", "max_length"]


def other_lengths():
    from finaletoolkit_amd import utils
    z = np.zeros((3, 8), np.int64)
    return utils.GCBias(5, 7, z, z, np.full((3, 8), np.nan), 0, 0, ())


@pytest.mark.parametrize("kwargs, match", [
    (dict(output_file="out.bedgraph"), "suffix"),
    (dict(output_file="out.tsv"), "suffix"),
    (dict(output_file="out.gz"), "suffix"),
    (dict(output_file="-"), "suffix"),
    (dict(min_length=0), "length"),
    (dict(min_length=150, max_length=149), "length"),
    (dict(max_length=1001), "length"),
    (dict(intersect_policy="start"), "policy"),
    (dict(intersect_policy=None), "policy"),
    (dict(stride=0), "stride"),
    (dict(min_bias=2.0 ** -16), "min_bias"),
    (dict(bias="other"), "lengths"),
    (dict(bias="other", min_length=5, max_length=8), "lengths"),
    (dict(bias="other", min_length=4, max_length=7), "lengths"),
])
def test_bad_arguments_raise_before_any_file_is_opened(tmp_path, kwargs, match):
    from finaletoolkit_amd import utils
    missing = [str(tmp_path / name) for name in ("no_such_input.frag.gz", "no_such_reference.2bit", "no_such_intervals.bed")]
    if kwargs.get("output_file") not in (None, "-"):
        kwargs = dict(kwargs, output_file=str(tmp_path / kwargs["output_file"]))
    if kwargs.get("bias") == "other":
        kwargs = dict(kwargs, bias=other_lengths())
    with pytest.raises(ValueError, match=match):
        utils.frag_gc_coverage(*missing, **kwargs)
    assert os.listdir(tmp_path) == []


def test_parser_maps_flags_onto_the_arguments():
    from finaletoolkit_amd import utils
    from finaletoolkit_amd.gccov import build_parser
    sig = inspect.signature(utils.frag_gc_coverage)
    ap = build_parser()
    flags = [a.dest for a in ap._actions if a.dest != "help"]
    assert sorted(flags) == sorted(sig.parameters)  # every flag an argument and every argument a flag
    d = {k: v.default for k, v in sig.parameters.items()}
    got = vars(ap.parse_args(["in.bam", "ref.2bit", "bins.bed", "out.bed"]))
    assert got == dict(d, input_file="in.bam", reference_file="ref.2bit", interval_file="bins.bed", output_file="out.bed")
    got = vars(ap.parse_args(["in.frag.gz", "hg38.fa", "bins.bed", "out.bed.gz", "--bias", "b.tsv.gz", "-q", "5", "--min-length",
                              "120", "--max-length", "180", "--policy", "any", "--min-bias", "0.1", "--stride", "16", "-w", "3",
                              "-v"]))
    assert got == dict(input_file="in.frag.gz", reference_file="hg38.fa", interval_file="bins.bed", output_file="out.bed.gz",
                       bias="b.tsv.gz", quality_threshold=5, min_length=120, max_length=180, intersect_policy="any",
                       min_bias=0.1, stride=16, workers=3, verbose=True)
    with pytest.raises(SystemExit):
        ap.parse_args(["in", "ref", "bins"])
    with pytest.raises(SystemExit):
        ap.parse_args(["in", "ref", "bins", "out.bed", "--policy", "start"])
    r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.gccov", "--help"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "--bias" in r.stdout and "--min-bias" in r.stdout and "INTERVALS" in r.stdout


def test_flat_names():
    import finaletoolkit_amd
    from finaletoolkit_amd import utils
    for name in FLAT:
        assert getattr(finaletoolkit_amd, name) is getattr(utils, name)
        assert name in dir(finaletoolkit_amd) and name in utils.__all__


def test_symbols_exported_and_declared():
    from finaletoolkit_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "ftk.h")).read()
    for name in SYMBOLS:
        assert name in L.EXPORTS
        assert re.search(r"^int %s\(ftk_ctx\*" % name, header, re.M), name
    assert re.search(r"^#define FTK_WEIGHT_ONE 65536u$", header, re.M)
    lib = L.load()
    for name in SYMBOLS:
        assert getattr(lib, name).argtypes


def test_coverage_rows_text(tmp_path):
    import gzip
    from finaletoolkit_amd import writers
    intervals = [("chr1", 0, 100, "a"), ("chrUn", 5, 6, "."), ("chr1", 50, 60, "b")]
    count = np.array([3, 7, 0], np.int64)
    corrected = np.array([196609 / 65536, np.nan, 0.0])
    want = "chr1\t0\t100\ta\t3\t3.000015\nchrUn\t5\t6\t.\t7\tnan\nchr1\t50\t60\tb\t0\t0.000000\n"
    for suffix in (".bed", ".bed.gz"):
        out = str(tmp_path / ("cov" + suffix))
        writers.write_gc_coverage_rows(out, intervals, count, corrected)
        raw = open(out, "rb").read()
        assert (raw[:2] == b"\x1f\x8b") == suffix.endswith(".gz")
        assert (gzip.open(out, "rt").read() if suffix.endswith(".gz") else raw.decode()) == want
    with pytest.raises(ValueError, match="suffix"):
        writers.write_gc_coverage_rows(str(tmp_path / "cov.bedgraph"), intervals, count, corrected)
