"""CPU: the host side of the V-plot - the argument errors ``frag_vplot`` raises before it touches the engine, the text
of ``writers.write_vplot_rows``, the command line's arguments, the flat names and the C symbol.  The kernel is held
against a numpy restatement in ``tests/test_gpu_vplot.py``."""
import gzip
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_argument_errors_come_before_any_engine_use(tmp_path, monkeypatch):
    from finaletoolkit_amd import utils

    def no_engine(*a, **k):
        raise AssertionError("the engine was asked for")
    monkeypatch.setattr(utils, "get_engine", no_engine)
    files = (str(tmp_path / "absent.frag.gz"), str(tmp_path / "absent.bed"))  # neither exists: nothing may open them
    ref = str(tmp_path / "absent.2bit")
    cases = [
        (dict(output_file=str(tmp_path / "out.bed")), "suffix"),
        (dict(output_file=str(tmp_path / "out.tsv.bz2")), "suffix"),
        (dict(half_width=1000, bin_size=3), "bin_size"),
        (dict(half_width=1000, bin_size=0), "bin_size"),
        (dict(half_width=0), "half_width"),
        (dict(half_width=(1 << 20) + 1, bin_size=1 << 21), "half_width"),
        (dict(half_width=2049, bin_size=1), "4096"),
        (dict(bias=str(tmp_path / "bias.tsv")), "reference_file"),
        (dict(min_length=200, max_length=100), "min_length"),
        (dict(reference_file=ref, min_length=200, max_length=100), "min_length"),
        (dict(min_length=None), "min_length"),
        (dict(max_length=None), "max_length"),
        (dict(min_length=-5, max_length=294), "min_length"),
        (dict(min_length=65_436, max_length=65_536, length_bin=101), "max_length"),
        (dict(length_bin=7), "length_bin"),                  # 300 lengths
        (dict(length_bin=0), "length_bin"),
        (dict(length_bin=-5), "length_bin"),
        (dict(min_length=0, max_length=4096, length_bin=1), "4096"),   # 4097 rows
        (dict(reference_file=ref, min_bias=0.0), "min_bias"),
        (dict(reference_file=ref, stride=0), "stride"),
    ]
    for kwargs, word in cases:
        with pytest.raises(ValueError, match=word):
            utils.frag_vplot(*files, **kwargs)
    other = utils.GCBias(100, 219, np.zeros((120, 220), np.int64), np.zeros((120, 220), np.int64), np.full((120, 220), np.nan), 0, 0, ())
    with pytest.raises(ValueError, match="lengths"):
        utils.frag_vplot(*files, reference_file=ref, bias=other, min_length=100, max_length=199)
    # a site beyond the coordinate bound, and more cells than one call may have: refused once the site file is read,
    # before the input is walked
    far = tmp_path / "far.bed"
    far.write_text("chr1\t100\t200\nchr1\t2147483000\t2147483600\tfar\n")
    with pytest.raises(ValueError, match="centre"):
        utils.frag_vplot(files[0], str(far))
    named = tmp_path / "named.bed"
    named.write_text("".join(f"chr1\t{100 * i}\t{100 * i + 10}\tn{i}\n" for i in range(17)))
    big = dict(half_width=2048, bin_size=1, min_length=0, max_length=4095, length_bin=1)  # 2^24 cells per group
    with pytest.raises(ValueError, match="cells"):
        utils.frag_vplot(files[0], str(named), by_name=True, **big)
    # arguments that pass go on to the files
    with pytest.raises(OSError):
        utils.frag_vplot(*files, half_width=2048, bin_size=1)


def test_signature_and_command_line():
    from finaletoolkit_amd import utils
    from finaletoolkit_amd.vplot import build_parser
    sig = inspect.signature(utils.frag_vplot)
    assert list(sig.parameters) == ["input_file", "site_file", "output_file", "reference_file", "bias", "half_width", "bin_size",
                                    "min_length", "max_length", "length_bin", "quality_threshold", "by_name", "normalize",
                                    "min_bias", "stride", "workers", "verbose"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(output_file=None, reference_file=None, bias=None, half_width=500, bin_size=5, min_length=50,
                            max_length=349, length_bin=5, quality_threshold=30, by_name=False, normalize=False, min_bias=0.05,
                            stride=1, workers=None, verbose=False)
    ap = build_parser()
    args = vars(ap.parse_args(["in.bam", "sites.bed", "out.tsv"]))
    assert set(args) == set(sig.parameters)
    assert {k: args[k] for k in defaults if k != "output_file"} == {k: v for k, v in defaults.items() if k != "output_file"}
    full = vars(ap.parse_args(["in.bam", "sites.bed", "out.tsv.gz", "--reference", "g.2bit", "--bias", "b.tsv", "--half-width", "990",
                               "--bin-size", "15", "--min-length", "100", "--max-length", "399", "--length-bin", "10", "-q", "20",
                               "--by-name", "--normalize", "--min-bias", "0.1", "--stride", "7", "-w", "3", "-v"]))
    assert full == dict(input_file="in.bam", site_file="sites.bed", output_file="out.tsv.gz", reference_file="g.2bit", bias="b.tsv",
                        half_width=990, bin_size=15, min_length=100, max_length=399, length_bin=10, quality_threshold=20,
                        by_name=True, normalize=True, min_bias=0.1, stride=7, workers=3, verbose=True)
    assert utils.VPlot._fields == ("groups", "n_sites", "offsets", "lengths", "count", "corrected", "skipped_contigs")
    eng = inspect.signature(__import__("finaletoolkit_amd.engine", fromlist=["Engine"]).Engine.site_vplot)
    assert list(eng.parameters) == ["self", "name", "centres", "flip", "groups", "n_groups", "half_width", "bin_size", "len_lo",
                                    "len_hi", "len_bin", "mapq_min", "weighted"]
    assert [p.default for p in list(eng.parameters.values())[3:]] == [None, None, 1, 500, 5, 50, 349, 5, 30, False]


@pytest.mark.parametrize("suffix", [".tsv", ".tsv.gz"])
def test_writer_text(tmp_path, suffix):
    from finaletoolkit_amd import utils, writers
    vp = utils.VPlot(("CTCF", "GATA1"), np.array([3, 0], np.int64), np.array([-2, 0], np.int64), np.array([100, 150], np.int64),
                     np.array([[[1, 0], [2 ** 40, 7]], [[0, 0], [0, 0]]], np.int64),
                     np.array([[[1.25, 0.0], [1099511627776.0000004, 1 / 3]], [[0.0, 0.0], [0.0, 0.0]]]), ("chrUn",))
    out = str(tmp_path / ("vplot" + suffix))
    writers.write_vplot_rows(out, vp)
    text = gzip.open(out, "rt").read() if suffix.endswith(".gz") else open(out).read()
    assert text == ("#group\tn_sites\tlength\toffset\tcount\tcorrected\n"
                    "CTCF\t3\t100\t-2\t1\t1.250000\n"
                    "CTCF\t3\t100\t0\t0\t0.000000\n"
                    "CTCF\t3\t150\t-2\t1099511627776\t1099511627776.000000\n"
                    "CTCF\t3\t150\t0\t7\t0.333333\n"
                    "GATA1\t0\t100\t-2\t0\t0.000000\n"
                    "GATA1\t0\t100\t0\t0\t0.000000\n"
                    "GATA1\t0\t150\t-2\t0\t0.000000\n"
                    "GATA1\t0\t150\t0\t0\t0.000000\n")
    with pytest.raises(ValueError, match="suffix"):
        writers.write_vplot_rows(str(tmp_path / "vplot.bed"), vp)


def test_null_ctx_is_invalid_and_writes_nothing():
    from finaletoolkit_amd import _lib as L
    lib = L.load()
    assert "ftk_site_vplot" in L.EXPORTS and hasattr(lib, "ftk_site_vplot")
    centre = np.array([100], np.int32)
    sums, counts = np.full(4, 7, np.int64), np.full(4, 7, np.int64)
    rc = lib.ftk_site_vplot(None, 0, L.ptr(centre), None, None, 1, 1, 1, 1, 100, 101, 1, 0, 0, L.ptr(sums), L.ptr(counts))
    assert rc == L.FTK_ERR_INVALID
    assert lib.ftk_last_error(None)
    assert np.all(sums == 7) and np.all(counts == 7)


def test_symbol_is_declared_in_the_header():
    text = open(os.path.join(ROOT, "include", "ftk.h")).read()
    m = re.search(r"^int ftk_site_vplot\(([^;]*)\);", text, re.M)
    assert m, "ftk_site_vplot is not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    kinds = [" ".join(a.split()[:-1]) for a in args.split(",")]
    names = [a.split()[-1] for a in args.split(",")]
    assert kinds == ["ftk_ctx*", "int", "const int32_t*", "const uint8_t*", "const int32_t*", "int64_t", "int32_t", "int32_t",
                     "int32_t", "int32_t", "int32_t", "int32_t", "int32_t", "int", "int64_t*", "int64_t*"]
    assert names == ["ctx", "contig_id", "centre", "flip", "group", "n_sites", "n_groups", "half_width", "bin_size", "len_lo",
                     "len_hi", "len_bin", "mapq_min", "use_weights", "sum_out", "count_out"]
    makefile = open(os.path.join(ROOT, "finaletoolkit_amd", "csrc", "Makefile")).read()
    assert "ftk_vplot.hip" in makefile


def test_flat_names_resolve():
    import finaletoolkit_amd as f
    from finaletoolkit_amd import utils
    assert f.frag_vplot is utils.frag_vplot and f.VPlot is utils.VPlot
    assert {"frag_vplot", "VPlot"} <= set(dir(f)) and {"frag_vplot", "VPlot"} <= set(utils.__all__)
    assert hasattr(__import__("finaletoolkit_amd.engine", fromlist=["Engine"]).Engine, "site_vplot")
