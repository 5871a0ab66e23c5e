"""CPU: the host side of the WPS periodogram - the argument errors ``frag_wps_spectrum`` raises before it touches the
engine, the text of ``writers.write_wps_spectrum_rows``, the command line's arguments, the flat names, the C symbols, and
the numpy restatement of the rule against a plain complex product.  The kernels are held against the restatement in
``tests/test_gpu_wps_spectrum.py``."""
import gzip
import inspect
import os
import re

import numpy as np
import pytest

from tests.spectrum_helpers import component_tolerance, spectrum_ref, spectrum_ref_runs, taper_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_argument_errors_come_before_any_engine_use(tmp_path, monkeypatch):
    from finaletoolkit_amd import utils

    def no_engine(*a, **k):
        raise AssertionError("the engine was asked for")
    monkeypatch.setattr(utils, "get_engine", no_engine)
    bam = (str(tmp_path / "absent.bam"), str(tmp_path / "absent.bed"))  # neither exists: nothing may open them
    cases = [
        (dict(output_file=str(tmp_path / "out.bed")), "suffix"),
        (dict(output_file=str(tmp_path / "out.tsv.bz2")), "suffix"),
        (dict(min_period=200, max_period=150, band=(160, 170)), "min_period"),
        (dict(min_period=1, max_period=100, band=(50, 60)), "range"),
        (dict(min_period=4000, max_period=4097, band=(4000, 4001)), "range"),
        (dict(min_period=2, max_period=1026, band=(100, 200)), "1024"),
        (dict(band=(100, 130)), "band"),
        (dict(band=(193, 281)), "band"),
        (dict(band=(199, 193)), "band"),
        (dict(band=193), "band"),
        (dict(taper=-0.01), "taper"),
        (dict(taper=0.51), "taper"),
        (dict(taper=float("nan")), "taper"),
    ]
    for kwargs, word in cases:
        with pytest.raises(ValueError, match=word):
            utils.frag_wps_spectrum(*bam, **kwargs)
    with pytest.raises(ValueError, match="chrom_sizes"):  # a fragment file carries no lengths
        utils.frag_wps_spectrum(str(tmp_path / "absent.frag.gz"), bam[1])
    # an interval too long for one run: refused once the interval file is read, before the input is walked
    long_bed = tmp_path / "long.bed"
    long_bed.write_text(f"chr1\t0\t{(1 << 22) + 1}\tlong\n")
    with pytest.raises(ValueError, match="bases"):
        utils.frag_wps_spectrum(bam[0], str(long_bed))
    sizes = tmp_path / "c.sizes"
    sizes.write_text("chr2\t1000\n")
    short_bed = tmp_path / "short.bed"
    short_bed.write_text("chr1\t0\t100\tg\n")
    with pytest.raises(ValueError, match="chrom_sizes"):
        utils.frag_wps_spectrum(str(tmp_path / "absent.frag.gz"), str(short_bed), chrom_sizes=str(sizes))
    # arguments that pass go on to the files
    with pytest.raises(OSError):
        utils.frag_wps_spectrum(*bam)


def test_signature_and_command_line():
    from finaletoolkit_amd import utils
    from finaletoolkit_amd.engine import Engine
    from finaletoolkit_amd.spectrum import build_parser
    sig = inspect.signature(utils.frag_wps_spectrum)
    assert list(sig.parameters) == ["input_file", "interval_file", "chrom_sizes", "output_file", "min_period", "max_period", "band",
                                    "window_size", "min_length", "max_length", "quality_threshold", "taper", "workers", "verbose"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(chrom_sizes=None, output_file=None, min_period=120, max_period=280, band=(193, 199), window_size=120,
                            min_length=120, max_length=180, quality_threshold=30, taper=0.1, workers=None, verbose=False)
    ap = build_parser()
    args = vars(ap.parse_args(["in.bam", "genes.bed", "out.tsv"]))
    assert set(args) == set(sig.parameters)
    assert {k: args[k] for k in defaults if k != "output_file"} == {k: v for k, v in defaults.items() if k != "output_file"}
    full = vars(ap.parse_args(["in.frag.gz", "genes.bed", "out.tsv.gz", "--chrom-sizes", "c.sizes", "--min-period", "100",
                               "--max-period", "300", "--band", "180", "210", "--window-size", "60", "--min-length", "35",
                               "--max-length", "80", "-q", "20", "--taper", "0.25", "-w", "3", "-v"]))
    full["band"] = tuple(full["band"])
    assert full == dict(input_file="in.frag.gz", interval_file="genes.bed", output_file="out.tsv.gz", chrom_sizes="c.sizes",
                        min_period=100, max_period=300, band=(180, 210), window_size=60, min_length=35, max_length=80,
                        quality_threshold=20, taper=0.25, workers=3, verbose=True)
    assert utils.WpsSpectrum._fields == ("intervals", "periods", "power", "band_mean", "n_bases")
    track = inspect.signature(Engine.track_spectrum)
    assert list(track.parameters)[:6] == ["self", "scores", "offsets", "periods", "taper", "detrend"]
    assert (track.parameters["taper"].default, track.parameters["detrend"].default) == (0.1, True)
    fused = inspect.signature(Engine.wps_spectrum)
    assert list(fused.parameters)[:13] == ["self", "name", "starts", "stops", "chrom_size", "periods", "window_size", "min_length",
                                           "max_length", "quality_threshold", "taper", "detrend", "batch_bases"]
    assert [p.default for p in list(fused.parameters.values())[6:13]] == [120, 120, 180, 30, 0.1, True, None]


@pytest.mark.parametrize("suffix", [".tsv", ".tsv.gz"])
def test_writer_text(tmp_path, suffix):
    from finaletoolkit_amd import utils, writers
    res = utils.WpsSpectrum([("chr1", 100, 1100, "GENE1"), ("chr2", 5, 5, ".")], np.array([192, 193, 194], np.int64),
                            np.array([[1.25, 1234567.891, 1 / 3], [np.nan, np.nan, np.nan]]), np.array([2.0e-7, np.nan]),
                            np.array([1000, 0], np.int64))
    out = str(tmp_path / ("spectrum" + suffix))
    writers.write_wps_spectrum_rows(out, res)
    text = gzip.open(out, "rt").read() if suffix.endswith(".gz") else open(out).read()
    assert text == ("contig\tstart\tstop\tname\tn_bases\tband_mean\tp192\tp193\tp194\n"
                    "chr1\t100\t1100\tGENE1\t1000\t2e-07\t1.25\t1.23457e+06\t0.333333\n"
                    "chr2\t5\t5\t.\t0\tnan\tnan\tnan\tnan\n")
    with pytest.raises(ValueError, match="suffix"):
        writers.write_wps_spectrum_rows(str(tmp_path / "spectrum.bed"), res)


def test_null_ctx_is_invalid_and_writes_nothing():
    from finaletoolkit_amd import _lib as L
    lib = L.load()
    for sym in ("ftk_track_spectrum", "ftk_wps_spectrum"):
        assert sym in L.EXPORTS and hasattr(lib, sym)
    scores, offs, per = np.arange(8, dtype=np.int64), np.array([0, 8], np.int64), np.array([2, 3], np.int32)
    out, ssw = np.full(4, 7.0), np.full(1, 7.0)
    rc = lib.ftk_track_spectrum(None, L.ptr(scores), L.ptr(offs), 1, L.ptr(per), 2, 0.1, 1, L.ptr(out), L.ptr(ssw))
    assert rc == L.FTK_ERR_INVALID and lib.ftk_last_error(None)
    rc = lib.ftk_wps_spectrum(None, 0, L.ptr(offs[:1]), L.ptr(offs[1:]), 1, 1000, 120, 120, 180, 30, L.ptr(per), 2, 0.1, 1, 0,
                              L.ptr(out), L.ptr(ssw))
    assert rc == L.FTK_ERR_INVALID
    assert np.all(out == 7.0) and np.all(ssw == 7.0)
    assert L.SPECTRUM_TILE is None or L.SPECTRUM_TILE > 0


def test_symbols_are_declared_in_the_header():
    text = open(os.path.join(ROOT, "include", "ftk.h")).read()

    def declared(name):
        m = re.search(r"^int %s\(([^;]*)\);" % name, text, re.M)
        assert m, name + " is not declared"
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
        return [" ".join(a.split()[:-1]) for a in args], [a.split()[-1] for a in args]
    kinds, names = declared("ftk_track_spectrum")
    assert kinds == ["ftk_ctx*", "const int64_t*", "const int64_t*", "int64_t", "const int32_t*", "int32_t", "double", "int",
                     "double*", "double*"]
    assert names == ["ctx", "scores", "offsets", "n_iv", "periods", "n_per", "taper", "detrend", "out", "ssw_out"]
    kinds, names = declared("ftk_wps_spectrum")
    assert kinds == ["ftk_ctx*", "int", "const int64_t*", "const int64_t*", "int64_t", "int64_t", "int32_t", "int32_t", "int32_t",
                     "int32_t", "const int32_t*", "int32_t", "double", "int", "int64_t", "double*", "double*"]
    assert names == ["ctx", "contig_id", "iv_start", "iv_stop", "n_iv", "chrom_size", "window_size", "min_len", "max_len",
                     "mapq_min", "periods", "n_per", "taper", "detrend", "batch_bases", "out", "ssw_out"]
    assert "n mod p" in text and "floor(a * N)" in text  # the rule is stated with the declarations
    makefile = open(os.path.join(ROOT, "finaletoolkit_amd", "csrc", "Makefile")).read()
    assert "ftk_spectrum.hip" in makefile


def test_flat_names_resolve():
    import finaletoolkit_amd as f
    from finaletoolkit_amd import utils
    assert f.frag_wps_spectrum is utils.frag_wps_spectrum and f.WpsSpectrum is utils.WpsSpectrum
    names = {"frag_wps_spectrum", "WpsSpectrum"}
    assert names <= set(dir(f)) and names <= set(utils.__all__) and names <= set(f._FLAT_BY_MODULE["utils"])
    eng = __import__("finaletoolkit_amd.engine", fromlist=["Engine"]).Engine
    assert hasattr(eng, "track_spectrum") and hasattr(eng, "wps_spectrum")


def test_restatement_against_a_plain_complex_product():
    """At small N the angle from n and the angle from n mod p agree to rounding: the restatement equals x @ exp(-2j pi n /
    p) within its own tolerance, the taper is symmetric with M = floor(a N) bell samples a side, and an empty run is 0."""
    rng = np.random.default_rng(7)
    periods = np.array([2, 3, 5, 7, 64, 120, 193], np.int64)
    for N in (1, 2, 9, 10, 64, 200):
        for taper in (0.0, 0.1, 0.5):
            for detrend in (False, True):
                v = rng.integers(-300, 61, N)
                w = taper_weights(N, taper)
                M = int(np.floor(taper * N))
                assert np.array_equal(w, w[::-1]) and np.all(w[M:N - M] == 1.0) and np.all(w[:M] < 1.0) and np.all(w > 0.0)
                x = (v - (v.sum() / N if detrend else 0.0)) * w
                n = np.arange(N)
                plain = np.array([np.sum(x * np.exp(-2j * np.pi * n / p)) for p in periods])
                got, ssw = spectrum_ref(v, periods, taper, detrend)
                tol = component_tolerance(v, periods)
                assert np.all(np.abs(got.real - plain.real) <= tol) and np.all(np.abs(got.imag - plain.imag) <= tol)
                assert ssw == pytest.approx(np.sum(w ** 2), rel=1e-15)
    w = taper_weights(10, 0.1)  # one bell sample a side: sin^2(pi / 4)
    assert w[0] == pytest.approx(0.5) and w[-1] == w[0] and np.all(w[1:-1] == 1.0)
    zero, ssw = spectrum_ref(np.zeros(0, np.int64), periods)
    assert np.all(zero == 0) and ssw == 0.0
    scores = rng.integers(-300, 61, 30)
    spec, ssws = spectrum_ref_runs(scores, [0, 10, 10, 30], periods[:3], 0.1, True)
    assert spec.shape == (3, 3) and np.all(spec[1] == 0) and ssws[1] == 0.0
    assert np.array_equal(spec[2], spectrum_ref(scores[10:], periods[:3], 0.1, True)[0])
