"""
GPU: both sides of every data-dependent path switch of the kernels, against the oracle.

Each kernel family picks its code path from the data: the length histogram from the bin count (per-wave LDS
histograms up to 2048 bins, one block-wide histogram up to 32768), the histogram median from the value range of a
tile (128 bins, 256 bins, the sort kernel), cleavage from the candidates of a tile (16-bit packed counters below
32768, two 32-bit half-tiles above), the device text rows from what a 4 KB block holds (line ends, names, runs,
digits).  Every test here puts data exactly on a threshold and just past it, shows from the data which side each
case is on, and compares exactly with the reference (stdev at rel=1e-12 as elsewhere).
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from finaletoolkit_amd import bgzf, synth
from finaletoolkit_amd._lib import FtkError
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------- length histograms
HIST_LEN = 2_000_000
LEN_LO = 30        # synth_contig clips lengths to [30, 1000]: the first bin is never empty
# lengths that land in the last bin / the overflow bin of 2048, 2049 and 32768 bins from LEN_LO, and long fragments of
# 40-70 kb (three 32768-bin chunks of the product's length range)
LONG_LENGTHS = [LEN_LO + 2047, LEN_LO + 2048, LEN_LO + 2049, LEN_LO + 32767, LEN_LO + 32768, 40_000, 55_000, 70_000, 12, 0]


def _with_long_fragments(size, depth, seed, lengths, copies):
    s, e, q, st = synth.synth_contig(size, depth=depth, seed=seed)
    rng = np.random.default_rng(seed + 1)
    ls = np.repeat(np.array(lengths, np.int64), copies)
    a = rng.integers(0, size - max(lengths) - 1, len(ls))
    s = np.concatenate([s.astype(np.int64), a])
    e = np.concatenate([e.astype(np.int64), a + ls])
    q = np.concatenate([q, np.where(rng.random(len(ls)) < 0.8, 60, 10).astype(np.uint8)])
    st = np.concatenate([st, rng.integers(0, 2, len(ls)).astype(np.uint8)])
    o = np.lexsort((e, s))
    return s[o].astype(np.int32), e[o].astype(np.int32), q[o], st[o]


@pytest.fixture(scope="module")
def hdata(engine):
    s, e, q, st = _with_long_fragments(HIST_LEN, 8.0, 501, LONG_LENGTHS, 40)
    rl = np.minimum(e - s, 100)
    r1s = np.where(st == 1, s, e - rl).astype(np.int32)
    # (read1 of the long fragments over their midpoints: with read1 at an end, the read1 fetch rule hands a 30 kb
    # fragment only to windows that its midpoint misses, and no window would count it)
    mid = (s.astype(np.int64) + e) // 2
    r1s = np.where(e - s > 2000, mid - 50, r1s).astype(np.int32)
    r1e = (r1s + rl).astype(np.int32)
    engine.load_contig("peA", s, e, q, st)
    engine.load_contig("peBAM", s, e, q, st, r1s, r1e)
    frs = {"peA": O.Frags(s, e, q, st), "peBAM": O.Frags(s, e, q, st, r1s, r1e)}
    ss, se, sq, sst = _with_long_fragments(HIST_LEN, 8.0, 502, [L for L in LONG_LENGTHS if L <= LEN_LO + 2049], 40)
    engine.load_contig("peS", ss, se, sq, sst)
    frs["peS"] = O.Frags(ss, se, sq, sst)
    yield dict(s=s, e=e, q=q, st=st, frs=frs)
    for k in frs:
        engine.release(k)


def _block_tiling():
    ws, we = synth.tiling_windows(HIST_LEN, 5_000)  # 400 windows of one length: the block-per-window path
    return ws, we


def _planned_windows():
    rng = np.random.default_rng(77)
    ws = rng.integers(0, HIST_LEN - 300_000, 60)
    we = ws + np.where(np.arange(60) % 3 == 0, rng.integers(50_000, 250_000, 60), rng.integers(1, 400, 60))
    return ws.astype(np.int32), we.astype(np.int32)


@pytest.mark.parametrize("kind,n_bins", [(k, b) for k in ("peA", "peBAM") for b in (2048, 2049, 32768)] +
                         [("peS", 2048), ("peS", 2049)])
def test_length_histogram_at_the_bin_limits(engine, hdata, kind, n_bins):
    """2048 bins: per-wave LDS histograms (feat_small_kernel) beside feat_large_kernel; 2049: block histograms only;
    32768: the block-wide LDS histogram of 131 KB.  peS has no fragment longer than 2.1 kb, so the planner hands its
    small windows to the wave-per-window kernel (at most 2048 bins); on peA the 70 kb fragments put more than 1024
    candidates under every window.  On a planned window set and on a tiling that takes the
    block-per-window path, with fragments in the first, the last and the overflow bin; fraglen_stats from the same
    rows against the reference's formulas."""
    fr = hdata["frs"][kind]
    tiles = _block_tiling()
    plan = _planned_windows()
    ln = (tiles[1] - tiles[0]).astype(np.int64)
    assert len(tiles[0]) >= 256 and ln.max() * len(ln) <= 8 * ln.sum()  # the block path's shape (>= one window per CU)
    pl = (plan[1] - plan[0]).astype(np.int64)
    assert len(plan[0]) < 256 and pl.max() > 100 * pl.min()              # the planner's (fewer windows than CUs)
    for name, (ws, we) in (("block", tiles), ("planned", plan)):
        want_h, want_o = O.c_fraglen_hist(fr, ws, we, LEN_LO, n_bins, mapq_min=30)
        assert want_h[:, 0].sum() > 0 and want_h[:, -1].sum() > 0 and want_o.sum() > 0, (name, n_bins)
        got_h, got_o = engine.fraglen_hist(kind, ws, we, LEN_LO, n_bins, 30)
        assert np.array_equal(got_h, want_h) and np.array_equal(got_o, want_o), (name, n_bins)
        r = engine.window_features(kind, ws, we, 30, hist=(LEN_LO, n_bins), delfi=dict(quality_threshold=30))
        assert np.array_equal(r["hist"], want_h) and np.array_equal(r["overflow"], want_o), (name, n_bins)
        assert np.array_equal(r["coverage"], O.c_window_counts(fr, ws, we, mapq_min=30)), (name, n_bins)
        sh, lg, _ = O.c_delfi_counts(fr, ws, we, 30)
        assert np.array_equal(r["short"], sh) and np.array_equal(r["long"], lg), (name, n_bins)
        # a request the FAST block kernels do not serve (length bounds): the general kernels at the same limit
        r = engine.window_features(kind, ws, we, 30, min_length=20, max_length=60_000, hist=(LEN_LO, n_bins))
        bh, bo = O.c_fraglen_hist(fr, ws, we, LEN_LO, n_bins, mapq_min=30, min_len=20, max_len=60_000)
        assert np.array_equal(r["hist"], bh) and np.array_equal(r["overflow"], bo), (name, n_bins)
        # statistics from the histogram rows (the overflow is not part of them)
        stats = engine.fraglen_stats(kind, ws, we, LEN_LO, n_bins, 150, 30)
        for k in range(len(ws)):
            nz = np.nonzero(want_h[k])[0]
            if len(nz) == 0:
                assert stats[k, 5] == 0, (name, k)
                continue
            w = O.py_frag_length_stats({int(b) + LEN_LO: int(want_h[k, b]) for b in nz}, 150)
            assert stats[k, 0] == w[0] and stats[k, 1] == w[1], (name, k)  # mean: one division of exact sums
            assert stats[k, 2] == pytest.approx(w[2], rel=1e-12, abs=1e-12), (name, k)
            assert (stats[k, 3], stats[k, 4], stats[k, 5]) == (w[3], w[4], w[5]), (name, k)
            assert stats[k, 6] == round(w[6] * w[5]), (name, k)


@pytest.mark.parametrize("kind", ["peA", "peBAM"])
def test_merged_feature_and_wps_launch_at_32768_bins(engine, hdata, kind):
    """all_features_wps: the merged feat_then_wps_kernel (feature blocks, then WPS tiles in one grid) with the 131 KB
    histogram, against the oracle's histograms, counts, DELFI rows and WPS."""
    fr = hdata["frs"][kind]
    ws, we = _block_tiling()
    f, w = engine.all_features_wps(kind, ws, we, HIST_LEN, 30, hist_bins=(LEN_LO, 32768), delfi_q=30)
    want_h, want_o = O.c_fraglen_hist(fr, ws, we, LEN_LO, 32768, mapq_min=30)
    assert want_h[:, -1].sum() > 0 and want_o.sum() > 0
    assert np.array_equal(f["hist"], want_h) and np.array_equal(f["overflow"], want_o)
    assert np.array_equal(f["coverage"], O.c_window_counts(fr, ws, we, mapq_min=30))
    sh, lg, _ = O.c_delfi_counts(fr, ws, we, 30)
    assert np.array_equal(f["short"], sh) and np.array_equal(f["long"], lg)
    _same_wps(engine, kind, fr, w, HIST_LEN)


def _same_wps(engine, kind, fr, w, size):
    """Whole-contig scores: against the oracle on stretches at both ends and in the middle (the oracle takes minutes
    for the whole contig), and against the separate ftk_wps call everywhere."""
    for a in (0, 4093, size // 2 - 3, size - 6000):
        assert np.array_equal(w[a:a + 6000], O.c_wps(fr, a, a + 6000, size)), a
    assert np.array_equal(w, engine.wps(kind, 0, size, size))


def test_tiled_wps_and_features_stop_at_8192_bins(engine):
    """ftk_wps_window_features (one pass over a regular tiling) takes at most 8192 bins: exact at 8192 with fragments
    in the last and the overflow bin, refused at 8193."""
    size = 1_000_000
    s, e, q, st = _with_long_fragments(size, 10.0, 611, [LEN_LO + 8191, LEN_LO + 8192, 9_000], 30)
    engine.load_contig("pw", s, e, q, st)
    fr = O.Frags(s, e, q, st)
    try:
        win = 20_000
        assert win >= 4096 + int((e - s).max())
        n_win = size // win
        ws = (np.arange(n_win) * win).astype(np.int32)
        we = (ws + win).astype(np.int32)
        cov, over = np.zeros(n_win, np.int64), np.zeros(n_win, np.int64)
        hist = np.zeros((n_win, 8192), np.uint32)
        got = engine.wps_window_features("pw", size, 0, win, n_win, coverage=cov, hist=hist, hist_bins=(LEN_LO, 8192),
                                         overflow=over)
        want_h, want_o = O.c_fraglen_hist(fr, ws, we, LEN_LO, 8192, mapq_min=30)
        assert want_h[:, 0].sum() > 0 and want_h[:, -1].sum() > 0 and want_o.sum() > 0
        assert np.array_equal(hist, want_h) and np.array_equal(over, want_o)
        assert np.array_equal(cov, O.c_window_counts(fr, ws, we, mapq_min=30))
        _same_wps(engine, "pw", fr, got, size)
        with pytest.raises(FtkError):
            engine.wps_window_features("pw", size, 0, win, n_win, coverage=cov, hist=np.zeros((n_win, 8193), np.uint32),
                                       hist_bins=(LEN_LO, 8193), overflow=over)
    finally:
        engine.release("pw")


def test_more_than_32768_bins_is_refused(engine, hdata):
    ws, we = _block_tiling()
    with pytest.raises(FtkError):
        engine.fraglen_hist("peA", ws, we, 0, 32769, 30)
    with pytest.raises(FtkError):
        engine.window_features("peA", ws, we, 30, hist=(0, 32769))
    with pytest.raises(FtkError):
        engine.fraglen_stats("peA", ws, we, 0, 32769, 150, 30)
    with pytest.raises(FtkError):
        engine.all_features_wps("peA", ws, we, HIST_LEN, 30, hist_bins=(0, 32769))


def test_length_ranges_split_into_32768_bin_chunks(hdata, tmp_path):
    """frag_length_bins / frag_length_intervals on a contig whose longest fragment is 70 kb: the product cuts the
    length range [0, 70 000] into three 32768-bin calls (and the planner's longest fragment is 70 kb)."""
    from finaletoolkit_amd import frag
    from finaletoolkit_amd.frag import _frag_length as FL
    s, e, q, st = hdata["s"], hdata["e"], hdata["q"], hdata["st"]
    fr = hdata["frs"]["peA"]
    lmax = int((e - s).max())
    assert lmax == 70_000 and -(-(lmax + 1) // FL._MAX_BINS) == 3
    p = str(tmp_path / "long.frag.gz")
    bgzf.write_frag_gz(p, [("long", s, e, q, st)], level=1)
    h, o = O.c_fraglen_hist(fr, [O.OPEN_LO], [O.OPEN_HI], 0, lmax + 1, mapq_min=30)
    assert o.sum() == 0
    nz = np.nonzero(h[0])[0]
    bins, counts = frag.frag_length_bins(p, contig="long")
    assert np.array_equal(np.asarray(bins), np.arange(nz[0], nz[-1] + 1))
    assert np.array_equal(np.asarray(counts), h[0, nz[0]:nz[-1] + 1])
    ivs = [(0, HIST_LEN), (100_000, 400_000), (1_000_000, 1_000_050), (1_500_000, 1_999_999), (10, 20)]
    bed = tmp_path / "iv.bed"
    bed.write_text("".join(f"long\t{a}\t{b}\tiv{k}\n" for k, (a, b) in enumerate(ivs)))
    got = frag.frag_length_intervals(p, str(bed))
    assert len(got) == len(ivs)
    ws = np.array([a for a, _ in ivs], np.int32)
    we = np.array([b for _, b in ivs], np.int32)
    hh, _ = O.c_fraglen_hist(fr, ws, we, 0, lmax + 1, mapq_min=30)
    n_long = 0
    for k, g in enumerate(got):
        nzk = np.nonzero(hh[k])[0]
        if len(nzk) == 0:
            assert (g.count, g.mean, g.median) == (-1, -1, -1), k
            continue
        n_long += int(nzk[-1] >= FL._MAX_BINS)
        w = O.py_frag_length_stats({int(b): int(hh[k, b]) for b in nzk}, 150)
        assert g.mean == pytest.approx(w[0], rel=1e-9, abs=1e-9) and g.median == w[1], k
        assert g.stdev == pytest.approx(w[2], rel=1e-12, abs=1e-12), k
        assert (g.minimum, g.maximum, g.count) == (w[3], w[4], w[5]), k
        assert g.frac_short_reads == pytest.approx(w[6], rel=1e-12), k
    assert n_long >= 2  # intervals holding fragments of the second and third chunk


# ---------------------------------------------------------------------------------------------- histogram median
def _median_pass(run, W):
    """Which kernel answers the run's median (the rule of adjust_median_hist_tile, tile by tile over 4096 outputs):
    128 / 256 bins, or 0 for the sort kernel; the largest request of the run's tiles wins."""
    need = 128
    n_out = len(run) - W
    for o0 in range(0, n_out, 4096):
        v = run[o0:o0 + min(4096, n_out - o0) + W - 1]
        ok = bool(np.all(v == np.rint(v)) and np.all(np.abs(v) < 1e9) and np.all(np.abs(v - v[0]) < 30000)
                  and not np.any((v == 0) & np.signbit(v)))
        rng = v.max() - v.min()
        if ok and rng < 128:
            continue
        need = 256 if (ok and rng < 256 and need != 0) else 0
        if need == 0:
            return 0
    return need


def _median_runs(W, seed):
    """Runs on both sides of every switch of the histogram median; returns [(label, values, expected pass)]."""
    rng = np.random.default_rng(seed)
    runs = []

    def ints(n, lo, span):
        v = lo + rng.integers(0, span + 1, n).astype(np.float64)
        v[rng.integers(0, n)] = lo
        v[rng.integers(0, n)] = lo + span  # the range is exactly `span`
        return v

    n = W + 700
    runs += [("range127", ints(n, -40, 127), 128), ("range128", ints(n, 17, 128), 256),
             ("range255", ints(n, -100, 255), 256), ("range256", ints(n, 3, 256), 0)]
    runs += [("near+1e9", ints(n, 1e9 - 101, 100), 128), ("near-1e9", ints(n, -(1e9 - 1), 100), 128)]
    v = ints(n, 1e9 - 101, 100)
    v[n // 2] = 1e9
    runs.append(("at+1e9", v, 0))
    v = ints(n, -(1e9 - 1), 100)
    v[n // 3] = -1e9
    runs.append(("at-1e9", v, 0))
    for off, label in ((29_999, "offset29999"), (30_000, "offset30000")):
        v = ints(n, 50, 60)
        v[n // 2] = 50 + off  # (v0 = 50 or near it: the offset from the tile's first value)
        v[0] = 50
        runs.append((label, v, 0))
    # one interval, tiles asking for different passes (the larger mark must win, whichever tile marks last)
    m = W + 4096 + 900
    v = ints(m, 0, 200)                     # tile 1: 256 bins
    v[4096 + W + 100] = 0.5                 # tile 2: the sort
    runs.append(("tile256_tile_sort", v, 0))
    v = ints(m, 0, 60)
    v[10] = 0.5                             # tile 1: the sort
    v[4096 + W:] = ints(m - 4096 - W, 0, 200)  # tile 2: 256 bins
    runs.append(("tile_sort_tile256", v, 0))
    v = ints(m, 5, 60)
    v[4096 + W:] = ints(m - 4096 - W, 5, 200)  # tile 1: 128 bins, tile 2: 256
    runs.append(("tile128_tile256", v, 256))
    # -0.0 in a tile that only the 256-bin pass could otherwise take, and in a 128-bin tile
    v = ints(n, -100, 180)
    v[n // 2] = -0.0
    runs.append(("neg_zero_wide", v, 0))
    v = ints(n, -20, 40)
    v[n // 4] = -0.0
    runs.append(("neg_zero_narrow", v, 0))
    # output counts: 1..63 (lanes without outputs), one whole tile and one output past it
    for k in (1, 2, 31, 63, 4096, 4097):
        runs.append((f"n_out{k}", ints(W + k, 100, 90), 128))
    return runs


@pytest.mark.parametrize("W", [2, 1000, 2048])
def test_histogram_median_on_both_sides_of_every_switch(engine, W, tmp_path):
    """adjust_median_hist_kernel<128> / <256> and adjust_median_kernel (the sort) on runs exactly at and just past each
    switch, all in one call (so the passes mark intervals of one another's launches): against py_adjust_run with and
    without edge subtraction, and bit for bit against the sort kernel alone (FTK_ADJUST_HIST=0, a child process)."""
    runs = _median_runs(W, 900 + W)
    for label, v, want_pass in runs:
        assert _median_pass(v, W) == want_pass, (label, W)
    assert {p for _, _, p in runs} == {128, 256, 0}
    raw = np.concatenate([v for _, v, _ in runs])
    offs = np.zeros(len(runs) + 1, np.int64)
    np.cumsum([len(v) for _, v, _ in runs], out=offs[1:])
    edge = [min(500, len(v)) for _, v, _ in runs]
    sub = np.array([np.mean([np.mean(v[:e]), np.mean(v[-e:])]) for (_, v, _), e in zip(runs, edge)])
    results = {}
    for with_sub in (False, True):
        got = engine.wps_adjust(raw, offs, W, edge_sub=sub if with_sub else None, savgol=False)
        results[with_sub] = got
        for i, (label, v, _) in enumerate(runs):
            want = O.py_adjust_run(v, W, edge_size=edge[i] if with_sub else None, savgol=False)
            seg = got[offs[i] - i * W:offs[i + 1] - (i + 1) * W]
            assert seg.shape == want.shape and np.array_equal(seg, want), (label, W, with_sub)
    np.save(tmp_path / "raw.npy", raw)
    np.save(tmp_path / "offs.npy", offs)
    np.save(tmp_path / "sub.npy", sub)
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "from finaletoolkit_amd.engine import Engine\n"
            "d = %r\n"
            "raw, offs, sub = (np.load(d + '/' + k + '.npy') for k in ('raw', 'offs', 'sub'))\n"
            "with Engine(0) as eng:\n"
            "    np.save(d + '/sort0.npy', eng.wps_adjust(raw, offs, %d, savgol=False))\n"
            "    np.save(d + '/sort1.npy', eng.wps_adjust(raw, offs, %d, edge_sub=sub, savgol=False))\n") % (ROOT, str(tmp_path), W, W)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FTK_ADJUST_HIST="0"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for with_sub in (False, True):
        sort_only = np.load(tmp_path / f"sort{int(with_sub)}.npy")
        assert np.array_equal(results[with_sub].view(np.int64), sort_only.view(np.int64)), (W, with_sub)


# ---------------------------------------------------------------------------------------------- cleavage intervals
def _tile_candidates(s, t0, len_t, lmax):
    """(lower bound, upper bound) of a cleavage tile's candidate count: starts in [t0 - lmax, t0 + len_t), widened to
    the 512-base bins of the position index for the upper bound."""
    lo = np.searchsorted(s, t0 - lmax, "left")
    hi = np.searchsorted(s, t0 + len_t, "left")
    blo = np.searchsorted(s, max(t0 - lmax, 0) >> 9 << 9, "left")
    bhi = np.searchsorted(s, ((t0 + len_t) >> 9) + 1 << 9, "left")
    return int(hi - lo), int(bhi - blo)


def test_cleavage_intervals_on_both_sides_of_the_packed_counters(engine):
    """ftk_cleavage_intervals (the multi-interval form with its own tile descriptors) over a region of > 40 000
    candidates per tile (32-bit half-tiles) and one of < 30 000 (16-bit packed counters), in the same call: interval
    lengths 1, 4095, 4096, 4097 and 20 000, duplicates, overlaps, an interval at 0; against the oracle per interval
    and against the single-interval call, and with min_length > max_length."""
    rng = np.random.default_rng(88)
    deep_s = rng.integers(20_000, 32_000, 160_000)
    calm_s = rng.integers(60_000, 400_000, 60_000)
    s = np.concatenate([deep_s, calm_s])
    e = s + rng.integers(60, 400, len(s))
    o = np.argsort(s, kind="stable")
    s, e = s[o].astype(np.int32), e[o].astype(np.int32)
    q = rng.integers(0, 61, len(s)).astype(np.uint8)
    st = rng.integers(0, 2, len(s)).astype(np.uint8)
    engine.load_contig("clv", s, e, q, st)
    fr = O.Frags(s, e, q, st)
    lmax = int((e - s).max())
    try:
        deep = [(22_000, 22_001), (22_000, 26_095), (21_000, 25_096), (20_500, 24_597), (20_000, 40_000),
                (22_000, 26_095), (23_000, 27_000)]
        calm = [(0, 4096), (100_000, 100_001), (150_000, 154_095), (200_000, 204_096), (250_000, 254_097),
                (300_000, 320_000), (300_000, 320_000), (310_000, 314_097), (399_000, 402_000)]
        ivs = deep + calm
        sides = {"half": 0, "packed": 0}
        for a, b in ivs:
            for t0 in range(a, b, 4096):
                low, high = _tile_candidates(s, t0, min(4096, b - t0), lmax)
                assert low >= 40_000 or high <= 30_000, (a, b, t0, low, high)  # clearly on one side
                sides["half" if low >= 40_000 else "packed"] += 1
        assert sides["half"] >= 6 and sides["packed"] >= 12, sides
        assert {b - a for a, b in ivs} >= {1, 4095, 4096, 4097, 20_000}
        for lo, hi, mq in ((None, None, 0), (100, 300, 20), (300, 100, 0)):
            got, offs = engine.cleavage_intervals("clv", [a for a, _ in ivs], [b for _, b in ivs], lo, hi, mq)
            for i, (a, b) in enumerate(ivs):
                want = O.c_cleavage(fr, a, b, lo, hi, mq)[2]
                assert np.array_equal(got[offs[i]:offs[i + 1]], want), (a, b, lo, hi, mq)
                assert np.array_equal(engine.cleavage("clv", a, b, lo, hi, mq), want), ("single", a, b, lo, hi, mq)
            if lo is not None and lo > hi:
                assert not got.any()
            else:
                assert got[:offs[len(deep)]].any() and got[offs[len(deep)]:].any()
    finally:
        engine.release("clv")


# ---------------------------------------------------------------------------------------------- device text rows
def _text_child(tmp_path, name, text, **env):
    """Rows of the device stream == rows of the host decoder (a child process: the stream's switches are read once);
    returns (device pieces, host pieces) from the decoder's timing line."""
    from tests.test_gpu_device_parse import _child
    p = str(tmp_path / name)
    bgzf.write_bgzf(p, text.encode(), level=1)
    out = _child(p, threads=3, FTK_DECODE_TIMING="1", **env)
    m = re.search(r"(\d+) pieces parsed on the device, (\d+) by the host", out)
    assert m, out[-1500:]
    return int(m.group(1)), int(m.group(2))


def _row(name, s, e, q, st, bed6):
    f = [name, str(s), str(e), str(q), st]
    if bed6:
        f = f[:3] + ["."] + f[3:]
    return "\t".join(f) + "\n"


@pytest.mark.parametrize("bed6", [False, True])
def test_densest_plain_block_stays_on_the_device(tmp_path, bed6):
    """Minimal plain rows ("c\\t1\\t2\\t0\\t+": 10 bytes, 409 line ends per 4 KB block) are parsed on the device; a block
    of more than 512 line ends (kMaxLinesPerBlock: empty lines) sends its piece to the host."""
    rows = "".join(_row("c", 1, 2 + (i % 7 == 0), i % 10, "+-"[i & 1], bed6) for i in range(30_000))
    assert 4096 // (len(_row("c", 1, 2, 0, "+", bed6))) >= (340 if bed6 else 409)
    dev, host = _text_child(tmp_path, "dense.frag.gz", rows)
    assert dev >= 1 and host == 0, (dev, host)
    lines = rows.splitlines(keepends=True)
    blank = "\n" * 600  # 600 line ends in 600 bytes
    text = "".join(lines[:12_000]) + blank + "".join(lines[12_000:])
    dev, host = _text_child(tmp_path, "blank.frag.gz", text)
    assert host >= 1, (dev, host)


def test_first_lines_far_in_front_of_their_block(tmp_path):
    """Rows of 140-510 bytes (long contig names) with a new contig every few rows: blocks whose first line starts
    129..256 bytes in front of them (beyond the wave's 128-byte look, inside the 256-byte halo) and more than 256 bytes
    in front (read from HBM), including the contig-run test against the line before, outside the LDS copy.  Names
    longer than 47 bytes are not reported by the device for device-inflated pieces, so the pieces are inflated by the
    host threads (FTK_DEVICE_INFLATE=0) and the rows parsed on the device."""
    rng = np.random.default_rng(41)
    parts = []
    for c in range(400):
        nm = f"ctg{c:04d}_" + "x" * int(rng.integers(120, 480))
        k = int(rng.integers(1, 9))
        st = np.sort(rng.integers(0, 1_000_000, k))
        parts += [_row(nm, int(a), int(a) + int(rng.integers(30, 600)), int(rng.integers(0, 61)), "+-"[int(rng.integers(2))], False)
                  for a in st]
    text = "".join(parts)
    ends = np.cumsum([len(r) for r in parts])
    starts = ends - np.array([len(r) for r in parts])
    back = []  # for each 4 KB boundary: how far in front of it the line ending first behind it starts
    for b in range(4096, len(text), 4096):
        j = np.searchsorted(ends, b, "right")  # first line whose '\n' lies at or behind b
        back.append(b - starts[j])
    back = np.array(back)
    assert ((back > 128) & (back <= 256)).sum() >= 20 and (back > 256).sum() >= 20, back
    dev, host = _text_child(tmp_path, "longnames.frag.gz", text, FTK_DEVICE_INFLATE="0")
    assert dev >= 1 and host == 0, (dev, host)


@pytest.mark.parametrize("name_len,device", [(47, True), (48, False)])
def test_contig_name_lengths_the_device_reports(tmp_path, name_len, device):
    """Device-inflated pieces: the device hands over contig names of up to 47 bytes (kTextNameBytes - 1); a 48-byte
    name sends the piece to the host."""
    nm = ("n%d_" % name_len).ljust(name_len, "z")
    assert len(nm) == name_len
    text = "".join(_row(nm, 1000 + i, 1200 + i, 60, "+", False) for i in range(2_000))
    dev, host = _text_child(tmp_path, f"name{name_len}.frag.gz", text)
    assert (dev >= 1 and host == 0) if device else host >= 1, (dev, host)


@pytest.mark.parametrize("n_runs,host_inflate,device", [(64, False, True), (65, False, False),
                                                         (1024, True, True), (1025, True, False)])
def test_contig_runs_per_piece(tmp_path, n_runs, host_inflate, device):
    """One piece with 64 / 65 contig runs (kTextNamedRuns: device-inflated pieces) and 1024 / 1025 (kTextMaxRuns:
    pieces inflated by the host threads)."""
    text = "".join(_row(f"r{c}", 10 * k, 10 * k + 150, 30, "+", False) for c in range(n_runs) for k in range(3))
    assert len(text) < 64 << 10  # one piece
    env = dict(FTK_DEVICE_INFLATE="0") if host_inflate else {}
    dev, host = _text_child(tmp_path, f"runs{n_runs}.frag.gz", text, **env)
    assert (dev >= 1 and host == 0) if device else host >= 1, (dev, host)


_DIGIT_CASES = [  # (label, start field, end field, mapq field, parsed on the device)
    ("int32_max", "2147483000", "2147483647", "60", True),
    ("int32_max_plus_1", "2147483000", "2147483648", "60", False),
    ("ten_digits_leading_zeros", "0000000005", "0000000170", "60", True),
    ("eleven_digits", "00000000005", "170", "60", False),
    ("mapq254", "5", "170", "254", True),
    ("mapq255", "5", "170", "255", True),
    ("mapq256", "5", "170", "256", True),
]


@pytest.mark.parametrize("bed6", [False, True])
@pytest.mark.parametrize("case", _DIGIT_CASES, ids=[c[0] for c in _DIGIT_CASES])
def test_digit_fields_at_their_limits(tmp_path, case, bed6):
    """Values of 10 digits and at most 0x7fffffff, leading zeros, MAPQ 254-256 (clamped to 255): one such row among
    plain ones, in .frag.gz and BED6 layout; the device parses the piece or hands it to the host as the row demands,
    and the rows equal the host decoder's."""
    label, fs, fe, mq, device = case
    digits = [len(fs), len(fe), len(mq)]
    assert (max(digits) <= 10 and int(fe) <= 0x7fffffff) == device
    plain = [_row("chrD", 1000 + i, 1200 + i, i % 61, "+-"[i & 1], bed6) for i in range(3_000)]
    f = ["chrD", fs, fe, mq, "+"]
    if bed6:
        f = f[:3] + ["odd"] + f[3:]
    odd = "\t".join(f) + "\n"
    # (start-sorted: a small start after the first plain row, a large one at the end)
    head = _row("chrD", 0, 100, 60, "+", bed6)
    text = head + odd + "".join(plain) if int(fs) < 1000 else head + "".join(plain) + odd
    dev, host = _text_child(tmp_path, f"{label}.frag.gz", text)
    assert (dev >= 1 and host == 0) if device else host >= 1, (label, dev, host)
