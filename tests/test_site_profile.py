"""CPU: the host side of the site profile - ``read_sites``, the argument errors ``frag_site_profile`` raises before it
touches the engine, the text of ``writers.write_site_profile_rows``, the command line's arguments, the flat names and
the C symbol.  The kernel is held against a numpy restatement in ``tests/test_gpu_site_profile.py``."""
import gzip
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BED = ("# a comment\n"
       "track name=sites\n"
       "browser position chr1:1-100\n"
       "\n"
       "chr1\t100\n"                                  # a short row
       "chr1\t100\t200\n"                             # no name, no strand
       "chr1\t100\t201\tCTCF\n"                       # an odd length: (100 + 201) // 2 = 150
       "chr2\t7\t8\tCTCF\t0\t-\n"
       "chr2\t0\t1\tGATA1\t0\t+\n"
       "chrX\t10\t20\t.\t0\t.\n"                      # a strand column that is neither: +
       "chrX\t999999999\t1000000000\tfar\t5\t-\textra\n")
SITES = [("chr1", 150, ".", "+"), ("chr1", 150, "CTCF", "+"), ("chr2", 7, "CTCF", "-"), ("chr2", 0, "GATA1", "+"),
         ("chrX", 15, ".", "+"), ("chrX", 999999999, "far", "-")]


def test_read_sites(tmp_path):
    from finaletoolkit_amd import utils
    plain, zipped = tmp_path / "sites.bed", tmp_path / "sites.bed.gz"
    plain.write_text(BED)
    with gzip.open(zipped, "wt") as fh:
        fh.write(BED)
    assert utils.read_sites(str(plain)) == SITES
    assert utils.read_sites(plain) == SITES            # a path object
    assert utils.read_sites(str(zipped)) == SITES      # .bed.gz reads like .bed
    assert [(c, (a + b) // 2, n) for c, a, b, n in utils.get_intervals(str(plain))] == [s[:3] for s in SITES]
    empty = tmp_path / "none.bed"
    empty.write_text("# nothing\n")
    assert utils.read_sites(str(empty)) == []


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
        (dict(half_width=4098, bin_size=2), "4096"),
        (dict(bias=str(tmp_path / "bias.tsv")), "reference_file"),
        (dict(min_length=200, max_length=100), "min_length"),
        (dict(reference_file=ref, min_length=200, max_length=100), "min_length"),
        (dict(reference_file=ref, min_bias=0.0), "min_bias"),
        (dict(reference_file=ref, stride=0), "stride"),
    ]
    for kwargs, word in cases:
        with pytest.raises(ValueError, match=word):
            utils.frag_site_profile(*files, **kwargs)
    other = utils.GCBias(100, 219, np.zeros((120, 220), np.int64), np.zeros((120, 220), np.int64), np.full((120, 220), np.nan), 0, 0, ())
    with pytest.raises(ValueError, match="lengths"):
        utils.frag_site_profile(*files, reference_file=ref, bias=other)
    # a site beyond the coordinate bound: refused before the input is walked, also where the bias would be measured first
    far = tmp_path / "far.bed"
    far.write_text("chr1\t100\t200\nchr1\t2147483000\t2147483600\tfar\n")
    for kwargs in ({}, dict(reference_file=ref)):
        with pytest.raises(ValueError, match="centre"):
            utils.frag_site_profile(files[0], str(far), **kwargs)
    # arguments that pass go on to the files
    with pytest.raises(OSError):
        utils.frag_site_profile(*files, half_width=2048, bin_size=1)


def test_signature_and_command_line():
    from finaletoolkit_amd import utils
    from finaletoolkit_amd.siteprofile import build_parser
    sig = inspect.signature(utils.frag_site_profile)
    assert list(sig.parameters) == ["input_file", "site_file", "output_file", "reference_file", "bias", "half_width", "bin_size",
                                    "min_length", "max_length", "quality_threshold", "by_name", "normalize", "min_bias",
                                    "stride", "workers", "verbose"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(output_file=None, reference_file=None, bias=None, half_width=1000, bin_size=1, min_length=100,
                            max_length=220, quality_threshold=30, by_name=False, normalize=False, min_bias=0.05, stride=1,
                            workers=None, verbose=False)
    ap = build_parser()
    args = vars(ap.parse_args(["in.bam", "sites.bed", "out.tsv"]))
    assert set(args) == set(sig.parameters)
    assert {k: args[k] for k in defaults if k != "output_file"} == {k: v for k, v in defaults.items() if k != "output_file"}
    full = vars(ap.parse_args(["in.bam", "sites.bed", "out.tsv.gz", "--reference", "g.2bit", "--bias", "b.tsv", "--half-width", "990",
                               "--bin-size", "15", "--min-length", "120", "--max-length", "180", "-q", "20", "--by-name",
                               "--normalize", "--min-bias", "0.1", "--stride", "7", "-w", "3", "-v"]))
    assert full == dict(input_file="in.bam", site_file="sites.bed", output_file="out.tsv.gz", reference_file="g.2bit", bias="b.tsv",
                        half_width=990, bin_size=15, min_length=120, max_length=180, quality_threshold=20, by_name=True,
                        normalize=True, min_bias=0.1, stride=7, workers=3, verbose=True)
    assert utils.SiteProfile._fields == ("groups", "n_sites", "offsets", "count", "corrected", "skipped_contigs")


@pytest.mark.parametrize("suffix", [".tsv", ".tsv.gz"])
def test_writer_text(tmp_path, suffix):
    from finaletoolkit_amd import utils, writers
    prof = utils.SiteProfile(("CTCF", "GATA1"), np.array([3, 0], np.int64), np.array([-4, -2, 0, 2], np.int64),
                             np.array([[1, 0, 2 ** 40, 7], [0, 0, 0, 0]], np.int64),
                             np.array([[1.25, 0.0, 1099511627776.0000004, 1 / 3], [0.0, 0.0, 0.0, 0.0]]), ("chrUn",))
    out = str(tmp_path / ("prof" + suffix))
    writers.write_site_profile_rows(out, prof)
    text = gzip.open(out, "rt").read() if suffix.endswith(".gz") else open(out).read()
    assert text == ("#group\tn_sites\toffset\tcount\tcorrected\n"
                    "CTCF\t3\t-4\t1\t1.250000\n"
                    "CTCF\t3\t-2\t0\t0.000000\n"
                    "CTCF\t3\t0\t1099511627776\t1099511627776.000000\n"
                    "CTCF\t3\t2\t7\t0.333333\n"
                    "GATA1\t0\t-4\t0\t0.000000\n"
                    "GATA1\t0\t-2\t0\t0.000000\n"
                    "GATA1\t0\t0\t0\t0.000000\n"
                    "GATA1\t0\t2\t0\t0.000000\n")
    with pytest.raises(ValueError, match="suffix"):
        writers.write_site_profile_rows(str(tmp_path / "prof.bed"), prof)


def test_null_ctx_is_invalid_and_writes_nothing():
    from finaletoolkit_amd import _lib as L
    lib = L.load()
    assert "ftk_site_profile" in L.EXPORTS and hasattr(lib, "ftk_site_profile")
    centre = np.array([100], np.int32)
    sums, counts = np.full(2, 7, np.int64), np.full(2, 7, np.int64)
    rc = lib.ftk_site_profile(None, 0, L.ptr(centre), None, None, 1, 1, 1, 1, 0, -1, -1, 0, L.ptr(sums), L.ptr(counts))
    assert rc == L.FTK_ERR_INVALID
    assert lib.ftk_last_error(None)
    assert np.all(sums == 7) and np.all(counts == 7)


def test_symbol_is_declared_in_the_header():
    text = open(os.path.join(ROOT, "include", "ftk.h")).read()
    m = re.search(r"^int ftk_site_profile\(([^;]*)\);", text, re.M)
    assert m, "ftk_site_profile is not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    kinds = [" ".join(a.split()[:-1]) for a in args.split(",")]
    assert kinds == ["ftk_ctx*", "int", "const int32_t*", "const uint8_t*", "const int32_t*", "int64_t", "int32_t", "int32_t",
                     "int32_t", "int32_t", "int32_t", "int32_t", "int", "int64_t*", "int64_t*"]
    makefile = open(os.path.join(ROOT, "finaletoolkit_amd", "csrc", "Makefile")).read()
    assert "ftk_siteprofile.hip" in makefile


def test_flat_names_resolve():
    import finaletoolkit_amd as f
    from finaletoolkit_amd import utils
    assert f.frag_site_profile is utils.frag_site_profile and f.read_sites is utils.read_sites
    assert {"frag_site_profile", "read_sites"} <= set(dir(f)) and {"frag_site_profile", "read_sites"} <= set(utils.__all__)
    assert hasattr(__import__("finaletoolkit_amd.engine", fromlist=["Engine"]).Engine, "site_profile")
