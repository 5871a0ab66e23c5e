"""GPU: the periodogram kernels (``Engine.track_spectrum``, ``Engine.wps_spectrum``, ``utils.frag_wps_spectrum``) against
the numpy restatement of the rule in ``tests/spectrum_helpers.py``, within the tolerance derived there: ``2^-49 (N + p)
(sum |v| + 1)`` per component, ``2^-49 N`` relative for ``ssw``.  Exact cases, bit-for-bit reproducibility, the fused call
against the two-step route, the C ABI's refusals and the product path."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import write_synthetic_bam
from tests.spectrum_helpers import (U49, assert_spectrum_close, component_tolerance, spectrum_ref, spectrum_ref_runs,
                                    ssw_tolerance)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERIODS = np.array([2, 3, 64, 120, 193, 280, 777, 4095, 4096], np.int32)
BIG = 2 ** 31 - 1


def tile_length():
    from finaletoolkit_amd import _lib as L
    return L.SPECTRUM_TILE or 4096  # the kernels cut a run into no tiles: the sizes of a 4096-sample one


def pack(runs):
    """(scores, offsets) of runs laid end to end."""
    offs = np.zeros(len(runs) + 1, np.int64)
    np.cumsum([len(r) for r in runs], out=offs[1:])
    return (np.concatenate(runs) if runs else np.zeros(0, np.int64)).astype(np.int64), offs


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. the rule against the restatement ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rule_runs():
    rng = np.random.default_rng(20261019)
    T = tile_length()
    runs = [rng.integers(-300, 61, N) for N in (1, 2, 63, 64, 65, 255, 256, 257, 777, T - 1, T, T + 1, 3 * T + 5)]
    runs += [rng.choice([-BIG, BIG], N) for N in (1, 2, 63, 64, 65)]           # the widest values a run may hold
    runs += [np.full(N, BIG, np.int64) for N in (2, 65)]                        # and the largest sum of them
    return runs


@pytest.mark.parametrize("detrend", [False, True])
@pytest.mark.parametrize("taper", [0.0, 0.1, 0.5])
def test_rule_against_the_restatement(engine, rule_runs, taper, detrend):
    scores, offs = pack(rule_runs)
    spec, ssw = engine.track_spectrum(scores, offs, PERIODS, taper, detrend)
    assert spec.shape == (len(rule_runs), len(PERIODS)) and spec.dtype == np.complex128 and ssw.dtype == np.float64
    worst = 0.0
    for i, v in enumerate(rule_runs):
        worst = max(worst, assert_spectrum_close(spec[i], ssw[i], v, PERIODS, taper, detrend, what=i))
    print(f"taper {taper} detrend {detrend}: worst component error {worst:.3g} of the bound")
    assert any(int(np.floor(taper * len(v))) == 0 for v in rule_runs)  # the M = 0 case is among them


# ---- 2. exact results -----------------------------------------------------------------------------------------------------
def test_constant_and_zero_runs_are_exactly_zero(engine):
    runs = [np.full(N, c, np.int64) for N in (1, 64, 777, 4097) for c in (-300, 7, BIG)]
    scores, offs = pack(runs)
    for taper in (0.0, 0.1, 0.5):
        spec, _ = engine.track_spectrum(scores, offs, PERIODS, taper, True)
        assert np.all(spec.real == 0.0) and np.all(spec.imag == 0.0)
    zeros, zoffs = pack([np.zeros(N, np.int64) for N in (1, 65, 4096)])
    for detrend in (False, True):
        spec, ssw = engine.track_spectrum(zeros, zoffs, PERIODS, 0.1, detrend)
        assert np.all(spec.real == 0.0) and np.all(spec.imag == 0.0) and np.all(ssw > 0)


def test_impulses_pin_the_sign_and_the_index(engine):
    N = 9000
    for p in (2, 3, 64, 193, 777, 4096):
        places = [0, p - 1, p, N - 1]
        runs = []
        for n0 in places:
            v = np.zeros(N, np.int64)
            v[n0] = 1
            runs.append(v)
        scores, offs = pack(runs)
        spec, ssw = engine.track_spectrum(scores, offs, [p], 0.0, False)
        assert np.all(ssw == float(N))
        for n0, got in zip(places, spec[:, 0]):
            want = np.exp(-2j * np.pi * (n0 % p) / p)  # re = cos, im = -sin of the angle of n0 mod p
            assert abs(got.real - want.real) <= 2.0 ** -50 and abs(got.imag - want.imag) <= 2.0 ** -50, (p, n0, got, want)
        assert spec[1, 0].imag > 0 or p == 2  # n0 = p - 1: the angle is just below 2 pi, so -sin is positive


def test_a_cosine_of_period_190_peaks_at_190(engine):
    n = np.arange(1900)
    v = np.rint(100 * np.cos(2 * np.pi * n / 190)).astype(np.int64)
    periods = np.arange(120, 281)
    spec, ssw = engine.track_spectrum(v, [0, len(v)], periods)
    power = (spec.real ** 2 + spec.imag ** 2)[0] / ssw[0]
    assert periods[int(np.argmax(power))] == 190


# ---- 3. reproducibility ---------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_call(engine, rule_runs):
    import torch
    rng = np.random.default_rng(5)
    runs = [rule_runs[k] for k in (3, 8, 10, 12, 15)]
    with_empty = [runs[0], np.zeros(0, np.int64), runs[1], runs[2], np.zeros(0, np.int64), np.zeros(0, np.int64), runs[3], runs[4]]
    scores, offs = pack(with_empty)
    wide = np.arange(120, 281, dtype=np.int32)
    spec, ssw = engine.track_spectrum(scores, offs, wide)
    again, ssw2 = engine.track_spectrum(scores, offs, wide)
    assert same_bits(spec, again) and same_bits(ssw, ssw2)                      # call to call
    empty = [i for i, r in enumerate(with_empty) if len(r) == 0]
    assert np.all(spec[empty] == 0) and np.all(ssw[empty] == 0)                 # empty runs: zeros, and nothing disturbed
    alone, ssw_alone = engine.track_spectrum(*pack(runs), wide)
    full = [i for i, r in enumerate(with_empty) if len(r)]
    assert same_bits(spec[full], alone) and same_bits(ssw[full], ssw_alone)
    order = rng.permutation(len(with_empty))                                    # permuted runs: permuted rows
    perm, ssw_perm = engine.track_spectrum(*pack([with_empty[i] for i in order]), wide)
    assert same_bits(perm, spec[order]) and same_bits(ssw_perm, ssw[order])
    col = list(wide).index(193)                                                 # one period, whatever else is asked
    one, _ = engine.track_spectrum(scores, offs, [193])
    many = np.concatenate([np.arange(2, 1025), [4096]]).astype(np.int32)
    assert len(many) == 1024
    big, _ = engine.track_spectrum(scores, offs, many)
    assert same_bits(one[:, 0], spec[:, col]) and same_bits(big[:, list(many).index(193)], spec[:, col])
    rev, _ = engine.track_spectrum(scores, offs, wide[::-1].copy())
    assert same_bits(rev[:, ::-1], spec)
    d_scores = torch.from_numpy(scores).cuda()                                  # device pointers: the host call's bits
    d_out = torch.full((len(with_empty), len(wide), 2), 7.0, dtype=torch.float64, device="cuda")
    d_ssw = torch.full((len(with_empty),), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()  # (the fills run on torch's stream, the call on the engine's)
    got, got_ssw = engine.track_spectrum(d_scores, offs, wide, out=d_out, ssw_out=d_ssw)
    assert got is d_out and got_ssw is d_ssw
    torch.cuda.synchronize()
    assert same_bits(d_out.cpu().numpy().view(np.complex128)[..., 0], spec) and same_bits(d_ssw.cpu().numpy(), ssw)
    part, _ = engine.track_spectrum(scores, offs[2:5], wide)                     # offsets that do not start at 0
    assert same_bits(part, spec[2:4])
    host_only, no_ssw = np.zeros((len(with_empty), len(wide)), np.complex128), None
    rc = engine.lib.ftk_track_spectrum(engine.ctx, d_scores.data_ptr(), offs.ctypes.data, len(with_empty), wide.ctypes.data, len(wide),
                                       0.1, 1, host_only.ctypes.data, no_ssw)  # ssw_out may be NULL
    assert rc == 0 and same_bits(host_only, spec)


# ---- 4. the fused call ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def contigs(engine):
    from finaletoolkit_amd import synth
    size = 60_000
    s, e, q, st = synth.synth_contig(size, depth=30.0, seed=11)
    keep = (s < 20_000) | (s > 26_000)  # a stretch without fragments
    s, e, q, st = s[keep], e[keep], q[keep], st[keep]
    r1s = np.where(st != 0, s, np.maximum(e - 50, s)).astype(np.int32)
    r1e = np.where(st != 0, np.minimum(s + 50, e), e).astype(np.int32)
    engine.load_contig("sp:plain", s, e, q, st)
    engine.load_contig("sp:bam", s, e, q, st, r1s, r1e)
    yield size
    engine.release("sp:plain")
    engine.release("sp:bam")


@pytest.mark.parametrize("key", ["sp:plain", "sp:bam"])
def test_fused_call_equals_scores_then_transform(engine, contigs, key):
    size = contigs
    starts = np.array([30_000, 0, 31_000, 52_000, 21_000, 5_000, 5_000, 40_000, 12_000, 59_000, 100], np.int64)
    stops = np.array([34_000, 2_500, 36_500, 52_001, 25_000, 5_000, 4_000, 45_000, 12_900, 60_000, 8_293], np.int64)
    lens = np.maximum(stops - starts, 0)
    periods = np.arange(120, 281, dtype=np.int32)
    some_empty = False
    for kw in (dict(), dict(quality_threshold=61), dict(min_length=160, max_length=170, quality_threshold=30, window_size=60),
               dict(taper=0.0, detrend=False)):
        wps_kw = {k: v for k, v in kw.items() if k not in ("taper", "detrend")}
        tr_kw = {k: v for k, v in kw.items() if k in ("taper", "detrend")}
        scores, offs = engine.wps_intervals(key, starts, stops, size, **wps_kw)
        want, want_ssw = engine.track_spectrum(scores, offs, periods, **tr_kw)
        for batch in (None, 1_000, int(lens.max()) - 1, int(lens.sum()) // 2, int(lens.sum())):
            got, got_ssw = engine.wps_spectrum(key, starts, stops, size, periods, batch_bases=batch, **kw)
            assert same_bits(got, want) and same_bits(got_ssw, want_ssw), (kw, batch)
        assert np.all(want[lens == 0] == 0) and np.all(want_ssw[lens == 0] == 0)  # the degenerate intervals
        hollow = [i for i in range(len(starts)) if lens[i] and not np.any(scores[offs[i]:offs[i + 1]])]
        some_empty |= 0 < len(hollow)
        assert np.all(want[hollow] == 0)
        if not kw:  # and the two-step route is the restatement of the scores
            assert np.any(scores) and 4 in hollow
            for i in (0, 1, 10):
                assert_spectrum_close(want[i], want_ssw[i], scores[offs[i]:offs[i + 1]], periods, 0.1, True, what=i)
    assert some_empty


# ---- 5. the C ABI ---------------------------------------------------------------------------------------------------------
def test_argument_errors(engine, contigs):
    import torch
    from finaletoolkit_amd import _lib as L
    lib, ctx, P = engine.lib, engine.ctx, L.ptr
    INV = L.FTK_ERR_INVALID
    scores = np.arange(-50, 50, dtype=np.int64)
    offs = np.array([0, 40, 40, 100], np.int64)
    per = np.array([2, 193, 4096], np.int32)
    out, ssw = np.full(3 * 3 * 2, 7.0), np.full(3, 7.0)
    d_offs, d_per = torch.from_numpy(offs).cuda(), torch.from_numpy(per).cuda()

    def track(ctx_=ctx, scores_=scores, offs_=offs, n=3, per_=per, n_per=3, taper=0.1, detrend=1, out_=out, ssw_=ssw):
        return lib.ftk_track_spectrum(ctx_, P(scores_), P(offs_), n, P(per_), n_per, taper, detrend, P(out_), P(ssw_))

    def failed(rc, word=None, code=INV):
        assert rc == code, (rc, code)
        message = lib.ftk_last_error(ctx)
        assert message and (word is None or word in message), message

    assert track(ctx_=None) == INV
    for name in ("scores_", "offs_", "per_", "out_"):
        failed(track(**{name: None}), b"NULL")
    failed(track(offs_=d_offs), b"host")
    failed(track(per_=d_per), b"host")
    failed(track(offs_=np.array([0, 40, 39, 100], np.int64)), b"decrease")
    failed(track(offs_=np.array([-1, 40, 40, 100], np.int64)), b"negative")
    failed(track(offs_=np.array([0, (1 << 22) + 1], np.int64), n=1), b"longer")
    failed(track(n=-1), b"n_iv")
    for n_per in (-1, 1025):
        failed(track(n_per=n_per), b"n_per")
    for bad in (1, 0, -193, 4097):
        failed(track(per_=np.array([2, bad, 4096], np.int32)), b"period")
    for taper in (-0.01, 0.51, float("nan")):
        failed(track(taper=taper), b"taper")
    assert np.all(out == 7.0) and np.all(ssw == 7.0)  # nothing was written by any of them
    # a score out of range is found on the device and reported after the call
    for wide in (1 << 31, -(1 << 31), 1 << 40):
        v = scores.copy()
        v[77] = wide
        failed(track(scores_=v), b"2^31")
    assert track() == L.FTK_OK and not np.any(out == 7.0)
    for i, want in enumerate(spectrum_ref_runs(scores, offs, per)[1]):
        assert abs(ssw[i] - want) <= ssw_tolerance(int(offs[i + 1] - offs[i]), want)
    # valid empty requests write nothing
    out[:], ssw[:] = 7.0, 7.0
    assert track(n=0) == L.FTK_OK and track(n_per=0) == L.FTK_OK and track(n=0, offs_=None, scores_=None, out_=None) == L.FTK_OK
    assert np.all(out == 7.0) and np.all(ssw == 7.0)
    assert track(n=1, offs_=np.array([5, 5], np.int64)) == L.FTK_OK and np.all(out[:6] == 0.0) and ssw[0] == 0.0  # an empty run
    out[:], ssw[:] = 7.0, 7.0

    cid = engine.contig_id("sp:plain")
    s, e = np.array([100, 5_000, 9_000], np.int64), np.array([2_100, 5_000, 9_500], np.int64)
    d_s = torch.from_numpy(s).cuda()

    def fused(ctx_=ctx, cid_=cid, s_=s, e_=e, n=3, size=60_000, W=120, lo=120, hi=180, q=30, per_=per, n_per=3, taper=0.1, detrend=1,
              batch=0, out_=out, ssw_=ssw):
        return lib.ftk_wps_spectrum(ctx_, cid_, P(s_), P(e_), n, size, W, lo, hi, q, P(per_), n_per, taper, detrend, batch, P(out_), P(ssw_))

    assert fused(ctx_=None) == INV
    for name in ("s_", "e_", "per_", "out_"):
        failed(fused(**{name: None}), b"NULL")
    failed(fused(s_=d_s), b"host")
    failed(fused(per_=d_per), b"host")
    failed(fused(batch=-1), b"batch_bases")
    for n_per in (-1, 1025):
        failed(fused(n_per=n_per), b"n_per")
    failed(fused(per_=np.array([2, 1, 4096], np.int32)), b"period")
    failed(fused(taper=0.6), b"taper")
    failed(fused(n=-1), b"n_iv")
    failed(fused(s_=np.array([100, 5_000, 0], np.int64), e_=np.array([2_100, 5_000, (1 << 22) + 1], np.int64)), b"longer")
    failed(fused(s_=np.array([-(1 << 30) - 1, 5_000, 9_000], np.int64)), b"interval")     # the validity of ftk_wps_intervals
    failed(fused(e_=np.array([2_100, 5_000, (1 << 31) + 1], np.int64)), b"interval")
    failed(fused(W=0), b"window_size")
    failed(fused(size=-1), b"chrom_size")
    failed(fused(cid_=987_654), None, L.FTK_ERR_NO_CONTIG)
    assert np.all(out == 7.0) and np.all(ssw == 7.0)
    assert fused(n=0) == L.FTK_OK and fused(n_per=0) == L.FTK_OK and np.all(out == 7.0)
    assert fused(ssw_=None) == L.FTK_OK and not np.any(out == 7.0) and np.all(ssw == 7.0)
    assert np.all(out.reshape(3, 3, 2)[1] == 0.0)  # the degenerate interval


# ---- 6. the product path --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def product(engine, tmp_path_factory):
    from finaletoolkit_amd import utils
    d = tmp_path_factory.mktemp("spectrum")
    rng = np.random.default_rng(193)
    sizes = [("sA", 40_000), ("sB", 30_000)]
    frags = {}
    for name, n in sizes:
        a = np.sort(rng.integers(0, n - 300, 5000))
        ln = rng.integers(100, 230, 5000)
        frags[name] = (a, a + ln, rng.choice([0, 10, 29, 30, 42, 60], 5000), rng.integers(0, 2, 5000))
    bam = str(d / "in.bam")
    write_synthetic_bam(bam, sizes, frags)
    frag = str(d / "in.frag.gz")
    utils.frag_export(bam, frag, quality_threshold=0)
    chrom_sizes = str(d / "g.chrom.sizes")
    with open(chrom_sizes, "w") as fh:
        fh.write("".join(f"{c}\t{n}\n" for c, n in sizes))
    rows = []
    for k in range(20):
        c, n = sizes[int(rng.integers(0, 2))]
        length = int(rng.integers(500, 5001))
        a = int(rng.integers(0, n - length))
        rows.append((c, a, a + length, f"gene{k}"))
    rows[3] = ("sA", 0, 3_000, "first")            # touches the contig's start
    rows[7] = ("sB", 30_000 - 777, 30_000, "last")  # and its end
    rows[11] = ("sA", 9_000, 9_000, "empty")       # no base
    bed = str(d / "genes.bed")
    with open(bed, "w") as fh:
        fh.write("# genes\n" + "".join(f"{c}\t{a}\t{b}\t{nm}\t0\t{'+-'[i % 2]}\n" for i, (c, a, b, nm) in enumerate(rows)))
    return dict(dir=d, bam=bam, frag=frag, chrom_sizes=chrom_sizes, bed=bed, rows=rows, sizes=dict(sizes))


def test_frag_wps_spectrum_end_to_end(engine, product, tmp_path):
    import warnings
    from finaletoolkit_amd import frag, utils
    p = product
    lo, hi, band = 150, 230, (193, 199)
    kw = dict(min_period=lo, max_period=hi, band=band)
    periods = np.arange(lo, hi + 1)
    out_frag, out_bam = str(tmp_path / "frag.tsv"), str(tmp_path / "bam.tsv.gz")
    res = utils.frag_wps_spectrum(p["frag"], p["bed"], p["chrom_sizes"], out_frag, **kw)
    res_bam = utils.frag_wps_spectrum(p["bam"], p["bed"], None, out_bam, **kw)
    assert res.intervals == p["rows"] == res_bam.intervals and np.array_equal(res.periods, periods)
    assert res.power.shape == (20, len(periods)) and res.power.dtype == np.float64 and res.n_bases.dtype == np.int64
    assert res.n_bases.tolist() == [b - a for _, a, b, _ in p["rows"]]
    assert same_bits(res.power, res_bam.power) and same_bits(res.band_mean, res_bam.band_mean)
    in_band = (periods >= band[0]) & (periods <= band[1])
    eps = 2.0 ** -52
    for i, (c, a, b, _) in enumerate(p["rows"]):
        if b == a:
            assert np.all(np.isnan(res.power[i])) and np.isnan(res.band_mean[i])
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            v = np.asarray(frag.wps(p["frag"], c, a, b, p["sizes"][c])["wps"], dtype=np.int64)
        assert len(v) == b - a and np.any(v)
        want, ssw = spectrum_ref(v, periods, 0.1, True)
        # power = (re^2 + im^2) / ssw with |d re|, |d im| <= t and |d ssw| <= r ssw, and a few roundings of its own
        t, r = component_tolerance(v, periods), U49 * len(v)
        power = (want.real ** 2 + want.imag ** 2) / ssw
        tol = (2 * (np.abs(want.real) + np.abs(want.imag)) * t + 2 * t * t) / ssw * (1 + 2 * r) + power * (2 * r + 8 * eps)
        assert np.all(np.abs(res.power[i] - power) <= tol), (i, float(np.max(np.abs(res.power[i] - power) / tol)))
        assert abs(res.band_mean[i] - power[in_band].mean()) <= tol[in_band].mean() + 8 * eps * power[in_band].mean()
        assert res.band_mean[i] == pytest.approx(res.power[i][in_band].mean(), rel=1e-15)
    # the files: one header, one row per interval in file order, six significant digits
    text = open(out_frag).read()
    assert gzip.open(out_bam, "rt").read() == text  # both inputs give the same file
    lines = text.splitlines()
    assert lines[0].split("\t") == ["contig", "start", "stop", "name", "n_bases", "band_mean"] + [f"p{q}" for q in periods]
    assert len(lines) == 21
    for i, line in enumerate(lines[1:]):
        f = line.split("\t")
        c, a, b, nm = p["rows"][i]
        assert f[:5] == [c, str(a), str(b), nm, str(b - a)]
        assert f[5:] == [("nan" if x != x else format(x, ".6g")) for x in [res.band_mean[i]] + res.power[i].tolist()]
        back = np.array([float(x) for x in f[5:]])
        assert np.allclose(back, np.concatenate([[res.band_mean[i]], res.power[i]]), rtol=5e-6, atol=0, equal_nan=True)
    # the command line in a child process, from either input
    for tag, args in (("frag", [p["frag"], p["bed"], None, "--chrom-sizes", p["chrom_sizes"]]), ("bam", [p["bam"], p["bed"], None])):
        cli = str(tmp_path / f"cli_{tag}.tsv")
        args[2] = cli
        r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.spectrum", *args, "--min-period", str(lo), "--max-period", str(hi),
                            "--band", "193", "199"], cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert open(cli).read() == text
    # an interval on a contig the input lacks, and one the chrom.sizes file lacks
    other = tmp_path / "other.bed"
    other.write_text("sA\t100\t900\tg\nsZ\t100\t900\th\n")
    with pytest.raises(ValueError, match="sZ"):
        utils.frag_wps_spectrum(p["bam"], str(other), **kw)
    with pytest.raises(ValueError, match="chrom_sizes"):
        utils.frag_wps_spectrum(p["frag"], str(other), p["chrom_sizes"], **kw)
