"""CPU: the host side of ``frag_gc_bias`` - its signature and the argument errors it raises before any file is opened,
the command line of ``python -m finaletoolkit_amd.gcbias``, the flat name, the three C symbols, the bias formula and
the TSV rows.  The kernels are held against a numpy restatement in ``tests/test_gpu_frag_gc_bias.py``."""
import gzip
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ftk_frag_gc", "ftk_frag_gc_table", "ftk_ref_gc_table")


def test_signature():
    from finaletoolkit_amd import utils
    sig = inspect.signature(utils.frag_gc_bias)
    assert list(sig.parameters) == ["input_file", "reference_file", "output_file", "contig", "min_length", "max_length",
                                    "quality_threshold", "stride", "expected", "workers", "verbose"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["input_file"] is inspect.Parameter.empty and d["reference_file"] is inspect.Parameter.empty
    assert d["output_file"] is None and d["contig"] is None and d["expected"] is None and d["workers"] is None
    assert (d["min_length"], d["max_length"], d["quality_threshold"], d["stride"], d["verbose"]) == (100, 220, 30, 1, False)
    assert utils.GCBias._fields == ("min_length", "max_length", "observed", "expected", "bias", "n_fragments", "n_skipped",
                                    "skipped_contigs")


@pytest.mark.parametrize("kwargs, match", [
    (dict(min_length=0), "length"),
    (dict(min_length=-5), "length"),
    (dict(min_length=150, max_length=149), "length"),
    (dict(max_length=1001), "length"),
    (dict(min_length=1001, max_length=1001), "length"),
    (dict(stride=0), "stride"),
    (dict(stride=-3), "stride"),
    (dict(expected=np.zeros((121, 220), np.int64)), "shape"),
    (dict(expected=np.zeros((120, 221), np.int64)), "shape"),
    (dict(expected=np.zeros(121 * 221, np.int64)), "shape"),
    (dict(min_length=1, max_length=3, expected=np.zeros((121, 221), np.int64)), "shape"),
    (dict(output_file="out.tsv.bgz"), "suffix"),
    (dict(output_file="out.txt"), "suffix"),
    (dict(output_file="out.gz"), "suffix"),
    (dict(output_file="-"), "suffix"),
])
def test_bad_arguments_raise_before_any_file_is_opened(tmp_path, kwargs, match):
    from finaletoolkit_amd import utils
    missing_in = str(tmp_path / "no_such_input.frag.gz")  # (opening either would be a different error)
    missing_ref = str(tmp_path / "no_such_reference.2bit")
    if kwargs.get("output_file") not in (None, "-"):
        kwargs = dict(kwargs, output_file=str(tmp_path / kwargs["output_file"]))
    with pytest.raises(ValueError, match=match):
        utils.frag_gc_bias(missing_in, missing_ref, **kwargs)
    assert os.listdir(tmp_path) == []


def test_parser_maps_flags_onto_the_arguments():
    from finaletoolkit_amd import utils
    from finaletoolkit_amd.gcbias import build_parser
    sig = inspect.signature(utils.frag_gc_bias)
    ap = build_parser()
    flags = [a.dest for a in ap._actions if a.dest != "help"]
    assert sorted(flags) == sorted(set(sig.parameters) - {"expected"})  # every flag an argument; `expected` is an array
    d = {k: v.default for k, v in sig.parameters.items() if k in flags}
    got = vars(ap.parse_args(["in.bam", "ref.2bit", "out.tsv"]))
    assert got == dict(d, input_file="in.bam", reference_file="ref.2bit", output_file="out.tsv")
    got = vars(ap.parse_args(["in.frag.gz", "hg38.fa", "out.tsv.gz", "-c", "chr7", "-q", "5", "--min-length", "120",
                              "--max-length", "180", "--stride", "16", "-w", "3", "-v"]))
    assert got == dict(input_file="in.frag.gz", reference_file="hg38.fa", output_file="out.tsv.gz", contig="chr7",
                       quality_threshold=5, min_length=120, max_length=180, stride=16, workers=3, verbose=True)
    got = vars(ap.parse_args(["a", "b", "c", "--contig", "12", "--min-mapq", "0", "--workers", "8", "--verbose"]))
    assert (got["contig"], got["quality_threshold"], got["workers"], got["verbose"], got["stride"]) == ("12", 0, 8, True, 1)
    with pytest.raises(SystemExit):
        ap.parse_args(["in", "ref"])
    r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.gcbias", "--help"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "--stride" in r.stdout and "--max-length" in r.stdout and "REF" in r.stdout


def test_flat_name():
    import finaletoolkit_amd
    from finaletoolkit_amd import utils
    assert finaletoolkit_amd.frag_gc_bias is utils.frag_gc_bias
    assert "frag_gc_bias" in dir(finaletoolkit_amd)
    code = ("import finaletoolkit_amd as f\n"
            "f.install_alias()\n"
            "import finaletoolkit\n"
            "from finaletoolkit_amd import utils\n"
            "assert 'frag_gc_bias' in dir(f) and f.frag_gc_bias is utils.frag_gc_bias\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_symbols_exported_and_declared():
    from finaletoolkit_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "ftk.h")).read()
    for name in SYMBOLS:
        assert name in L.EXPORTS
        assert re.search(r"^int %s\(ftk_ctx\*" % name, header, re.M), name
    assert re.search(r"^#define FTK_GC_MAX_LEN 1000$", header, re.M) and L.GC_MAX_LEN == 1000
    lib = L.load()
    for name in SYMBOLS:
        assert getattr(lib, name).argtypes


def test_bias_formula():
    from finaletoolkit_amd.utils import gc_bias_ratio
    obs = np.array([[1, 2, 0], [0, 3, 4]], np.int64)
    exp = np.array([[2, 0, 0], [1, 1, 6]], np.int64)
    b = gc_bias_ratio(obs, exp)
    assert b.dtype == np.float64 and b.shape == (2, 3)
    want = {(0, 0): (1 / 10) / (2 / 10), (1, 0): 0.0, (1, 1): (3 / 10) / (1 / 10), (1, 2): (4 / 10) / (6 / 10)}
    for (r, g), v in want.items():
        assert b[r, g] == v
    assert math.isnan(b[0, 1]) and math.isnan(b[0, 2])  # expected == 0: observed or not
    assert np.isnan(gc_bias_ratio(np.zeros((2, 3), np.int64), exp)).all()
    assert np.isnan(gc_bias_ratio(obs, np.zeros((2, 3), np.int64))).all()
    with pytest.raises(ValueError, match="shape"):
        gc_bias_ratio(obs, exp[:1])


def hand_made():
    from finaletoolkit_amd import utils
    obs = np.array([[1, 2, 0, 0, 0, 0, 0], [0, 3, 4, 0, 0, 0, 0]], np.int64)
    exp = np.array([[2, 0, 0, 0, 0, 7, 0], [1, 1, 6, 0, 0, 0, 0]], np.int64)
    return utils.GCBias(5, 6, obs, exp, utils.gc_bias_ratio(obs, exp), 10, 2, ("chrUn",))


def test_tsv_text_rows():
    from finaletoolkit_amd import writers
    res = hand_made()
    lines = writers.gc_bias_text(res.min_length, res.observed, res.expected, res.bias).splitlines()
    assert lines[0] == "length\tgc\tobserved\texpected\tbias"
    assert [ln.split("\t")[:4] for ln in lines[1:]] == [["5", "0", "1", "2"], ["5", "1", "2", "0"], ["5", "5", "0", "7"],
                                                       ["6", "0", "0", "1"], ["6", "1", "3", "1"], ["6", "2", "4", "6"]]
    bias = [ln.split("\t")[4] for ln in lines[1:]]
    assert bias[1] == "nan" and bias[2] == "0.0" and bias[3] == "0.0"
    for text, (r, g) in zip(bias, ((0, 0), (0, 1), (0, 5), (1, 0), (1, 1), (1, 2))):
        if text != "nan":
            assert text == repr(float(res.bias[r, g])) and float(text) == res.bias[r, g]  # round trip
    with pytest.raises(ValueError, match="shape"):
        writers.gc_bias_text(5, res.observed, res.expected[:1], res.bias)


@pytest.mark.parametrize("suffix", [".tsv", ".tsv.gz"])
def test_tsv_round_trip(tmp_path, suffix):
    from finaletoolkit_amd import writers
    res = hand_made()
    out = str(tmp_path / ("bias" + suffix))
    writers.write_gc_bias_table(out, res.min_length, res.observed, res.expected, res.bias)
    raw = open(out, "rb").read()
    assert (raw[:2] == b"\x1f\x8b") == suffix.endswith(".gz")
    text = gzip.open(out, "rt").read() if suffix.endswith(".gz") else raw.decode()
    assert text == writers.gc_bias_text(res.min_length, res.observed, res.expected, res.bias)
    obs = np.zeros_like(res.observed)
    exp = np.zeros_like(res.expected)
    for ln in text.splitlines()[1:]:
        length, g, o, e, b = ln.split("\t")
        r = int(length) - res.min_length
        obs[r, int(g)], exp[r, int(g)] = int(o), int(e)
        assert int(o) > 0 or int(e) > 0
        assert (b == "nan") == bool(np.isnan(res.bias[r, int(g)])) and (b == "nan" or float(b) == res.bias[r, int(g)])
    assert np.array_equal(obs, res.observed) and np.array_equal(exp, res.expected)
    with pytest.raises(ValueError, match="suffix"):
        writers.write_gc_bias_table(str(tmp_path / "bias.txt"), res.min_length, res.observed, res.expected, res.bias)
