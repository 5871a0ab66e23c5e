"""CPU: the host side of the site-ends feature - the argument errors ``frag_ocf`` raises before it touches the engine or a
file, the text of the three writers, the command line's arguments, the flat names and the C symbol - and the numpy
restatement of the rule on a contig small enough to count by hand.  The kernel is held against that restatement in
``tests/test_gpu_site_ends.py``."""
import gzip
import inspect
import os
import re
import sys

import numpy as np
import pytest

from tests.site_ends_helpers import SIGN, restated_site_ends

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 65536


def test_restatement_by_hand():
    # five fragments around a site on 100: U ends on 90, 96, 100, 104, 30; D ends on 99, 103, 100, 109, 39 (mapq 10: out)
    cols = (np.array([90, 96, 100, 104, 30]), np.array([100, 104, 101, 110, 40]), np.array([60, 60, 60, 60, 10]))
    w = np.array([1, 2, 4, 8, 16]) * ONE
    sums, counts, ssum, scnt = restated_site_ends(cols, w, [100, 100], [0, 1], [0, 1], 2, 10, 5, peak=4, flank=1)
    # d of U: -10, -4, 0, 4; of D: -1, 3, 0, 9.  Bins of 5 over [-10, 10): U -> 0, 1, 2, 2; D -> 1, 2, 2, 3
    assert counts[0].tolist() == [[1, 1, 2, 0], [0, 1, 2, 1]]
    assert (sums[0] // ONE).tolist() == [[1, 2, 12, 0], [0, 1, 6, 8]]
    # the flipped copy: bins reversed and the tracks swapped
    assert counts[1].tolist() == [[1, 2, 1, 0], [0, 2, 1, 1]]
    assert np.array_equal(sums[1], sums[0][::-1, ::-1])
    # windows [-5, -3] and [3, 5], in genome orientation for both sites: U -4 | no D || U 4 | D 3
    assert scnt.tolist() == [[1, 0, 1, 1]] * 2 and (ssum // ONE).tolist() == [[2, 0, 8, 2]] * 2
    assert ((scnt * SIGN).sum(axis=1)).tolist() == [-1, -1]
    # a length-1 fragment counts once in each track, in the same bin; the length bounds are closed; no base, no end
    one = (np.array([7, 7]), np.array([8, 7]), np.array([60, 60]))
    counts = restated_site_ends(one, None, [7], None, None, 1, 2, 1)[1]
    assert counts[0].tolist() == [[0, 0, 1, 0], [0, 0, 1, 0]]
    assert restated_site_ends(cols, None, [100], None, None, 1, 10, 20, 0, 2, 9)[1][0].tolist() == [[2], [2]]  # lengths 8 and 6
    assert restated_site_ends(cols, None, [100], None, None, 1, 10, 20, 0, 7, 9)[1][0].tolist() == [[1], [1]]  # length 8 alone


def test_argument_errors_come_before_any_engine_use(tmp_path, monkeypatch):
    from finaletoolkit_amd import utils

    def no_engine(*a, **k):
        raise AssertionError("the engine was asked for")
    monkeypatch.setattr(utils, "get_engine", no_engine)
    files = (str(tmp_path / "absent.frag.gz"), str(tmp_path / "absent.bed"))  # neither exists: nothing may open them
    ref = str(tmp_path / "absent.2bit")
    cases = [
        (dict(output_file=str(tmp_path / "out.bed")), "output_file"),
        (dict(profile_file=str(tmp_path / "out.tsv.bz2")), "profile_file"),
        (dict(site_output_file=str(tmp_path / "out.txt")), "site_output_file"),
        (dict(half_width=1000, bin_size=3), "bin_size"),
        (dict(half_width=1000, bin_size=0), "bin_size"),
        (dict(half_width=0), "half_width"),
        (dict(half_width=(1 << 20) + 1, bin_size=1 << 21), "half_width"),
        (dict(half_width=2049, bin_size=1), "4096"),
        (dict(peak=0, flank=0), "peak"),
        (dict(peak=None), "peak"),
        (dict(peak=10, flank=10), "flank"),
        (dict(peak=10, flank=-1), "flank"),
        (dict(half_width=70, bin_size=1, peak=60, flank=10), "half_width"),
        (dict(bias=str(tmp_path / "bias.tsv")), "reference_file"),
        (dict(min_length=200, max_length=100), "min_length"),
        (dict(reference_file=ref, min_length=200, max_length=100), "min_length"),
        (dict(reference_file=ref, min_bias=0.0), "min_bias"),
        (dict(reference_file=ref, stride=0), "stride"),
    ]
    for kwargs, word in cases:
        with pytest.raises(ValueError, match=word):
            utils.frag_ocf(*files, **kwargs)
    other = utils.GCBias(100, 219, np.zeros((120, 220), np.int64), np.zeros((120, 220), np.int64), np.full((120, 220), np.nan), 0, 0, ())
    with pytest.raises(ValueError, match="lengths"):
        utils.frag_ocf(*files, reference_file=ref, bias=other, min_length=100, max_length=199)
    # a site beyond the coordinate bound, and more cells than one call may have: refused once the site file is read,
    # before the input is walked
    far = tmp_path / "far.bed"
    far.write_text("chr1\t100\t200\nchr1\t2147483000\t2147483600\tfar\n")
    with pytest.raises(ValueError, match="centre"):
        utils.frag_ocf(files[0], str(far))
    named = tmp_path / "named.bed"
    named.write_text("".join(f"chr1\t{100 * i}\t{100 * i + 10}\tn{i}\n" for i in range((1 << 15) + 1)))
    with pytest.raises(ValueError, match="cells"):
        utils.frag_ocf(files[0], str(named), by_name=True, half_width=2048, bin_size=1)  # 2^13 cells per group
    # arguments that pass go on to the files: the windows just inside their bounds
    with pytest.raises(OSError):
        utils.frag_ocf(*files, half_width=71, bin_size=1, peak=60, flank=10)
    with pytest.raises(OSError):
        utils.frag_ocf(*files, half_width=2048, bin_size=1, peak=1, flank=0)


def test_signature_and_command_line():
    from finaletoolkit_amd import utils
    from finaletoolkit_amd.ocf import build_parser
    sig = inspect.signature(utils.frag_ocf)
    assert list(sig.parameters) == ["input_file", "site_file", "output_file", "profile_file", "site_output_file", "reference_file",
                                    "bias", "half_width", "bin_size", "peak", "flank", "min_length", "max_length",
                                    "quality_threshold", "by_name", "normalize", "min_bias", "stride", "workers", "verbose"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(output_file=None, profile_file=None, site_output_file=None, reference_file=None, bias=None,
                            half_width=1000, bin_size=1, peak=60, flank=10, min_length=50, max_length=350, quality_threshold=30,
                            by_name=False, normalize=False, min_bias=0.05, stride=1, workers=None, verbose=False)
    ap = build_parser()
    args = vars(ap.parse_args(["in.bam", "sites.bed", "out.tsv"]))
    assert set(args) == set(sig.parameters)
    assert {k: args[k] for k in defaults if k != "output_file"} == {k: v for k, v in defaults.items() if k != "output_file"}
    full = vars(ap.parse_args(["in.bam", "sites.bed", "out.tsv.gz", "--profile", "p.tsv", "--per-site", "s.tsv.gz", "--reference",
                               "g.2bit", "--bias", "b.tsv", "--half-width", "990", "--bin-size", "15", "--peak", "70", "--flank", "5",
                               "--min-length", "100", "--max-length", "399", "-q", "20", "--by-name", "--normalize", "--min-bias",
                               "0.1", "--stride", "7", "-w", "3", "-v"]))
    assert full == dict(input_file="in.bam", site_file="sites.bed", output_file="out.tsv.gz", profile_file="p.tsv",
                        site_output_file="s.tsv.gz", reference_file="g.2bit", bias="b.tsv", half_width=990, bin_size=15, peak=70,
                        flank=5, min_length=100, max_length=399, quality_threshold=20, by_name=True, normalize=True, min_bias=0.1,
                        stride=7, workers=3, verbose=True)
    assert utils.OCF._fields == ("groups", "n_sites", "offsets", "up_count", "down_count", "up_corrected", "down_corrected",
                                 "windows_count", "ocf_count", "ocf", "site_ocf", "skipped_contigs")
    eng = inspect.signature(__import__("finaletoolkit_amd.engine", fromlist=["Engine"]).Engine.site_ends)
    assert list(eng.parameters) == ["self", "name", "centres", "flip", "groups", "n_groups", "half_width", "bin_size",
                                    "quality_threshold", "min_length", "max_length", "weighted", "peak", "flank"]
    assert [p.default for p in list(eng.parameters.values())[3:]] == [None, None, 1, 1000, 1, 30, None, None, False, None, 10]


def canned():
    from finaletoolkit_amd import utils
    return utils.OCF(("CTCF", "GATA1"), np.array([3, 0], np.int64), np.array([-2, 0], np.int64),
                     np.array([[1, 0], [0, 0]], np.int64), np.array([[2 ** 40, 7], [0, 0]], np.int64),
                     np.array([[1.25, 0.0], [0.0, 0.0]]), np.array([[1099511627776.0000004, 1 / 3], [0.0, 0.0]]),
                     np.array([[5, 9, 2 ** 40, 1], [0, 0, 0, 0]], np.int64), np.array([2 ** 40 + 3, 0], np.int64),
                     np.array([-2 / 3, 0.0]), np.array([1.5, np.nan, -2 / 3]), ("chrUn",))


def read(path):
    return gzip.open(path, "rt").read() if path.endswith(".gz") else open(path).read()


@pytest.mark.parametrize("suffix", [".tsv", ".tsv.gz"])
def test_writer_text(tmp_path, suffix):
    from finaletoolkit_amd import writers
    ocf = canned()
    out = str(tmp_path / ("ocf" + suffix))
    writers.write_ocf_rows(out, ocf)
    assert read(out) == ("#group\tn_sites\tleft_up\tleft_down\tright_up\tright_down\tocf_count\tocf\n"
                         "CTCF\t3\t5\t9\t1099511627776\t1\t1099511627779\t-0.666667\n"
                         "GATA1\t0\t0\t0\t0\t0\t0\t0.000000\n")
    out = str(tmp_path / ("ends" + suffix))
    writers.write_end_profile_rows(out, ocf)
    assert read(out) == ("#group\tn_sites\toffset\tup_count\tdown_count\tup_corrected\tdown_corrected\n"
                         "CTCF\t3\t-2\t1\t1099511627776\t1.250000\t1099511627776.000000\n"
                         "CTCF\t3\t0\t0\t7\t0.000000\t0.333333\n"
                         "GATA1\t0\t-2\t0\t0\t0.000000\t0.000000\n"
                         "GATA1\t0\t0\t0\t0\t0.000000\t0.000000\n")
    out = str(tmp_path / ("sites" + suffix))
    sites = [("chr1", 100, "CTCF", "+"), ("chrUn", 5, "CTCF", "-"), ("chr2", 7, ".", "-")]
    writers.write_site_ocf_rows(out, sites, np.array([[1, 2, 3, 4], [0, 0, 0, 0], [2 ** 40, 0, 0, 9]], np.int64), ocf.site_ocf)
    assert read(out) == ("#contig\tcentre\tname\tstrand\tleft_up\tleft_down\tright_up\tright_down\tocf\n"
                         "chr1\t100\tCTCF\t+\t1\t2\t3\t4\t1.500000\n"
                         "chr2\t7\t.\t-\t1099511627776\t0\t0\t9\t-0.666667\n")  # the site of the skipped contig is left out
    for write, args in ((writers.write_ocf_rows, (ocf,)), (writers.write_end_profile_rows, (ocf,)),
                        (writers.write_site_ocf_rows, (sites, np.zeros((3, 4), np.int64), ocf.site_ocf))):
        with pytest.raises(ValueError, match="suffix"):
            write(str(tmp_path / "ocf.bed"), *args)


def test_null_ctx_is_invalid_and_writes_nothing():
    from finaletoolkit_amd import _lib as L
    lib = L.load()
    assert "ftk_site_ends" in L.EXPORTS and hasattr(lib, "ftk_site_ends")
    centre = np.array([100], np.int32)
    outs = [np.full(4, 7, np.int64) for _ in range(4)]
    rc = lib.ftk_site_ends(None, 0, L.ptr(centre), None, None, 1, 1, 1, 1, 0, -1, -1, 0, 0, 0, *(L.ptr(o) for o in outs))
    assert rc == L.FTK_ERR_INVALID
    assert lib.ftk_last_error(None)
    assert all(np.all(o == 7) for o in outs)


def test_symbol_is_declared_in_the_header_and_bound_with_its_arity():
    from finaletoolkit_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "ftk.h")).read()
    m = re.search(r"^int ftk_site_ends\(([^;]*)\);", text, re.M)
    assert m, "ftk_site_ends is not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    kinds = [" ".join(a.split()[:-1]) for a in args.split(",")]
    names = [a.split()[-1] for a in args.split(",")]
    assert kinds == ["ftk_ctx*", "int", "const int32_t*", "const uint8_t*", "const int32_t*", "int64_t", "int32_t", "int32_t",
                     "int32_t", "int32_t", "int32_t", "int32_t", "int", "int32_t", "int32_t", "int64_t*", "int64_t*", "int64_t*",
                     "int64_t*"]
    assert names == ["ctx", "contig_id", "centre", "flip", "group", "n_sites", "n_groups", "half_width", "bin_size", "mapq_min",
                     "min_len", "max_len", "use_weights", "peak", "flank", "sum_out", "count_out", "site_sum_out", "site_count_out"]
    assert len(L.load().ftk_site_ends.argtypes) == len(names)
    makefile = open(os.path.join(ROOT, "finaletoolkit_amd", "csrc", "Makefile")).read()
    assert "ftk_siteends.hip" in makefile


def test_flat_names_resolve():
    import finaletoolkit_amd as f
    from finaletoolkit_amd import utils
    assert f.frag_ocf is utils.frag_ocf and f.OCF is utils.OCF
    assert {"frag_ocf", "OCF"} <= set(dir(f)) and {"frag_ocf", "OCF"} <= set(utils.__all__)
    assert hasattr(__import__("finaletoolkit_amd.engine", fromlist=["Engine"]).Engine, "site_ends")
    f.install_alias("finaletoolkit", force=True)
    try:
        import finaletoolkit
        import finaletoolkit.utils as U
        assert U.frag_ocf is utils.frag_ocf and U.OCF is utils.OCF and finaletoolkit.frag_ocf is utils.frag_ocf
    finally:
        for k in [k for k in sys.modules if k == "finaletoolkit" or k.startswith("finaletoolkit.")]:
            del sys.modules[k]
