"""GPU: the nucleosome-call kernels (``Engine.track_peaks``, ``Engine.wps_peaks``, ``utils.frag_wps_peaks``) against the
numpy restatement of the rule in ``tests/peaks_helpers.py``.  Every comparison is exact: equal integers, bit-equal
float64.  Constructed runs at every length and tile boundary the rule and the mark pass turn on, exact cases, order and
reproducibility, the fused call against the two-step route, the C ABI's refusals and the product path."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import write_synthetic_bam
from tests.peaks_helpers import CALLS, FLAT, LONG, OPEN, PEAK_DTYPE, REGIONS, SHORT, pack, peaks_ref, peaks_ref_runs, same_calls

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 49, 50, 51, 149, 150, 151, 449, 450, 451, 1024)


def tile_length():
    from finaletoolkit_amd import _lib as L
    return L.PEAKS_TILE


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same(got, want, what=None):
    (calls, stats), (ref_calls, ref_stats) = got, want
    assert np.array_equal(stats, ref_stats), (what, stats.sum(axis=0), ref_stats.sum(axis=0))
    assert same_calls(calls, ref_calls), (what, len(calls), len(ref_calls))


# ---- 1. the rule against the restatement ----------------------------------------------------------------------------------
def constructed_runs(max_gap, skip, seed):
    """Runs that put a region of every length in LENGTHS, gaps of max_gap and max_gap + 1, the tile boundaries of the mark
    pass and the open / closed distances from either end of the callable track in front of the kernels."""
    rng = np.random.default_rng(seed)
    T, g = tile_length(), max_gap
    far = skip + g + 4  # a distance from a run's end at which a region is closed

    def noise(n, rounded=True):
        v = rng.normal(0.0, 3.0, n)
        return np.round(v * 4) / 4 if rounded else v

    def body(L, rounded=True):  # L positive values: exactly one region of L positions
        v = np.abs(noise(L, rounded)) + 0.25
        return v

    def off(n):  # n values that are not positive (zeros among them)
        return -np.abs(noise(n))

    runs = []
    for k, L in enumerate(LENGTHS):  # one closed region per run, rounded values (ties) and unrounded
        runs.append(np.concatenate([off(far), body(L, k % 2 == 0), off(far)]))
    runs.append(np.concatenate([np.concatenate([off(g + 1), body(L, False)]) for L in LENGTHS] + [off(far)]))  # split by max_gap + 1 each
    runs[-1] = np.concatenate([off(far), runs[-1]])
    a, b = body(60), body(70, False)
    runs.append(np.concatenate([off(far), a, off(g), b, off(far)]))      # a gap of max_gap merges ...
    runs.append(np.concatenate([off(far), a, off(g + 1), b, off(far)]))  # ... one of max_gap + 1 splits
    runs.append(np.concatenate([off(far), body(20), off(g), body(30), off(g), body(25), off(g + 1), body(60), off(far)]))
    for n in (0, 1, 2 * skip, 2 * skip + 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5):
        runs.append(noise(n))
    for r0, r1 in ((T - 1, T + 60), (T, T + 60), (T - 60, T), (T - 60, T + 1), (2 * T - 1, 2 * T + 1), (T - 500, T + 500)):
        v = off(2 * T + 100)
        v[r0:r1] = body(r1 - r0)
        runs.append(v)
    v = off(2 * T + 100)  # a gap of max_gap, and one of max_gap + 1, across the tile boundary
    lo = T - (g + 1) // 2
    v[lo - 60:lo], v[lo + g:lo + g + 60] = body(60), body(60)
    runs.append(v)
    v = off(2 * T + 100)
    v[lo - 60:lo], v[lo + g + 1:lo + g + 61] = body(60), body(60)
    runs.append(v)
    for lead in (g, g + 1):  # open and closed in turn, at lo and at hi
        runs.append(np.concatenate([off(skip + lead), body(80), off(far)]))
        runs.append(np.concatenate([off(far), body(80), off(skip + lead)]))
    runs.append(np.concatenate([off(far), np.full(60, 2.0), off(far)]))  # a closed plateau: flat
    runs.append(np.concatenate([off(far), body(700), off(far)]))         # too long at any max_region <= 450
    runs.append(noise(20_000))
    smooth = np.convolve(rng.normal(0.0, 3.0, 6_000 + 48), np.ones(49) / 7.0, mode="valid")  # and noise with nucleosome-sized swells
    runs.append(smooth)
    return runs


@pytest.mark.parametrize("skip", [0, 10])
@pytest.mark.parametrize("min_region", [1, 50])
@pytest.mark.parametrize("max_gap", [0, 5, 63])
def test_rule_against_the_restatement(engine, max_gap, min_region, skip):
    runs = constructed_runs(max_gap, skip, 20261019 + max_gap)
    scores, offs = pack(runs)
    kw = dict(skip=skip, max_gap=max_gap, min_region=min_region, short_max=150, max_region=450)
    got = engine.track_peaks(scores, offs, **kw)
    want = peaks_ref_runs(scores, offs, **kw)
    assert got[0].dtype == PEAK_DTYPE and got[1].dtype == np.int64 and got[1].shape == (len(runs), 6)
    totals = want[1].sum(axis=0)
    print(f"max_gap {max_gap} min_region {min_region} skip {skip}: {len(runs)} runs, {offs[-1]} positions, counters {totals.tolist()}")
    assert_same(got, want, kw)
    for k in (REGIONS, OPEN, LONG, FLAT, CALLS) + ((SHORT,) if min_region > 1 else ()):  # (no region is shorter than 1)
        assert totals[k] > 0, k
    assert np.all(np.diff(got[0]["run"]) >= 0)
    assert np.all((np.diff(got[0]["start"]) > 0) | (np.diff(got[0]["run"]) > 0))  # ordered by (run, start)
    assert np.all(got[1][:, CALLS] <= np.diff(offs) // (min_region + 1) + 1)      # the output bound


def test_other_length_limits(engine):
    runs = constructed_runs(5, 10, 7)
    scores, offs = pack(runs)
    for kw in (dict(skip=3, max_gap=2, min_region=10, short_max=60, max_region=1024),
               dict(skip=0, max_gap=5, min_region=150, short_max=150, max_region=150),
               dict(skip=0, max_gap=1, min_region=1, short_max=1, max_region=1),
               dict(skip=10, max_gap=5, min_region=50, short_max=450, max_region=450)):
        assert_same(engine.track_peaks(scores, offs, **kw), peaks_ref_runs(scores, offs, **kw), kw)


# ---- 2. exact cases -------------------------------------------------------------------------------------------------------
def test_exact_cases(engine):
    kw = dict(skip=0, max_gap=2, min_region=3, short_max=20, max_region=40)

    def one(v, **over):
        calls, stats = engine.track_peaks(np.asarray(v, np.float64), [0, len(v)], **{**kw, **over})
        return calls.tolist(), stats[0].tolist()

    assert one(np.zeros(300)) == ([], [0] * 6) and one(-np.ones(1500)) == ([], [0] * 6)       # nothing positive: no region
    assert one(np.ones(300)) == ([], [1, 1, 0, 0, 0, 0]) and one(np.ones(2500)) == ([], [1, 1, 0, 0, 0, 0])  # one open region
    pad = [-1.0] * 5
    assert one(pad + [2.0] * 10 + pad) == ([], [1, 0, 0, 0, 1, 0])                               # a closed plateau: flat
    # two windows of equal area: the leftmost (region 1 4 1 0 1 4 1, median 1: areas 4 and 4)
    tie = pad + [1.0, 4.0, 1.0, 0.0, 1.0, 4.0, 1.0] + pad
    assert one(tie) == ([(0, 6, 7, 6, 4.0, 4.0)], [1, 0, 0, 0, 0, 1])
    tie[10] = 4.25  # ... unless the right one is larger
    assert one(tie) == ([(0, 10, 11, 10, 4.25, 4.25)], [1, 0, 0, 0, 0, 1])
    # one triangle 1 2 3 4 5 4 3 2 1: median 3, window 4 5 4 at [8, 11), summit 9, height 5, area 13
    tri = pad + [1.0, 2.0, 3.0, 4.0, 5.0, 4.0, 3.0, 2.0, 1.0] + pad
    assert one(tri) == ([(0, 8, 11, 9, 5.0, 13.0)], [1, 0, 0, 0, 0, 1])
    # two equal summits: the leftmost
    assert one(pad + [1.0, 5.0, 5.0, 1.0] + pad) == ([(0, 6, 8, 6, 5.0, 10.0)], [1, 0, 0, 0, 0, 1])
    # odd L, the median a value of the region: 1 3 2 5 4 -> 3; windows [8, 10): 5 + 4
    assert one(pad + [1.0, 3.0, 2.0, 5.0, 4.0] + pad) == ([(0, 8, 10, 8, 5.0, 9.0)], [1, 0, 0, 0, 0, 1])
    # even L, both middle values equal: 1 3 3 5 -> 3; window [8, 9)
    assert one(pad + [1.0, 3.0, 3.0, 5.0] + pad) == ([(0, 8, 9, 8, 5.0, 5.0)], [1, 0, 0, 0, 0, 1])
    # even L, the median between two values: 1 2 4 5 -> 3; window [7, 9)
    assert one(pad + [1.0, 2.0, 4.0, 5.0] + pad) == ([(0, 7, 9, 8, 5.0, 9.0)], [1, 0, 0, 0, 0, 1])
    # a long region (L = 24 > short_max 20) yields every window of 3 .. 20 positions, in order
    wave = pad + [1.0, 5.0, 6.0, 5.0, 1.0, 1.0, 7.0, 1.0, 1.0, 4.0, 4.0, 4.0, 4.0, 1.0, 1.0, 1.0, 9.0, 9.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0] + pad
    assert one(wave) == ([(0, 6, 9, 7, 6.0, 16.0), (0, 14, 18, 14, 4.0, 16.0)], [1, 0, 0, 0, 0, 2])
    # the area is added left to right: the ones behind 1e16 are lost, the ones before it are kept
    big = pad + [1e16, 1.0, 1.0, 0.25, 0.25, 0.25, -1.0, -1.0, -1.0, 0.25, 0.25, 0.25, 1.0, 1.0, 1e16] + pad
    calls, stats = one(big, max_gap=0, min_region=1, short_max=6, max_region=6)
    assert [c[1:4] for c in calls] == [(5, 8, 5), (17, 20, 19)] and [c[5] for c in calls] == [1e16, 1e16 + 2.0] and stats == [2, 0, 0, 0, 0, 2]


# ---- 3. order and reproducibility -----------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_call(engine):
    import torch
    runs = constructed_runs(5, 10, 3)
    pick = [runs[k] for k in (3, 7, 12, 16, len(runs) - 2, len(runs) - 1)]
    empty = np.zeros(0)
    spread = [pick[0], empty, pick[1], pick[2], empty, empty, pick[3], pick[4], pick[5], empty]
    full = [i for i, r in enumerate(spread) if len(r)]
    kw = dict(skip=10, max_gap=5, min_region=50, short_max=150, max_region=450)
    scores, offs = pack(spread)
    calls, stats = engine.track_peaks(scores, offs, **kw)
    assert len(calls) > 20 and np.all(stats[[1, 4, 5, 9]] == 0)
    assert np.all(np.diff(calls["run"]) >= 0) and np.all((np.diff(calls["start"]) > 0) | (np.diff(calls["run"]) > 0))
    again = engine.track_peaks(scores, offs, **kw)                                   # call to call
    assert same_calls(again[0], calls) and np.array_equal(again[1], stats)
    together = engine.track_peaks(*pack(pick), **kw)                                 # without the empty runs
    moved = together[0].copy()
    moved["run"] = np.asarray(full, np.int32)[moved["run"]]
    assert same_calls(moved, calls) and np.array_equal(together[1], stats[full])
    for k, i in enumerate(full):                                                     # each run alone
        alone = engine.track_peaks(pick[k], [0, len(pick[k])], **kw)
        want = calls[calls["run"] == i].copy()
        want["run"] = 0
        assert same_calls(alone[0], want) and np.array_equal(alone[1][0], stats[i]), i
    part = engine.track_peaks(scores, offs[2:5], **kw)                               # offsets that do not start at 0
    want = calls[(calls["run"] >= 2) & (calls["run"] < 4)].copy()
    want["run"] -= 2
    assert same_calls(part[0], want) and np.array_equal(part[1], stats[2:4])
    d_scores = torch.from_numpy(scores).cuda()                                       # a device tensor: the host call's bits
    torch.cuda.synchronize()
    dev = engine.track_peaks(d_scores, offs, **kw)
    assert same_calls(dev[0], calls) and np.array_equal(dev[1], stats)
    assert_same((calls, stats), peaks_ref_runs(scores, offs, **kw))


# ---- 4. the fused call ----------------------------------------------------------------------------------------------------
def nucleosome_fragments(size, seed, depth=30.0):
    """Fragments of 120-180 bases around centres every 190 +- 8 bases: (start, end, mapq, forward), sorted by start."""
    rng = np.random.default_rng(seed)
    centres = np.cumsum(rng.integers(182, 199, size // 190 + 2)) - 95
    centres = centres[centres < size - 100]
    n = int(depth * size / 150)
    c = centres[rng.integers(0, len(centres), n)] + rng.integers(-12, 13, n)
    ln = rng.integers(120, 181, n)
    s = np.clip(c - ln // 2, 0, size - 181)
    order = np.argsort(s, kind="stable")
    s, ln = s[order], ln[order]
    return s.astype(np.int32), (s + ln).astype(np.int32), rng.choice([30, 42, 60], n).astype(np.uint8), rng.integers(0, 2, n).astype(np.uint8)


@pytest.fixture(scope="module")
def contigs(engine):
    size = 60_000
    s, e, q, st = nucleosome_fragments(size, 11)
    keep = (s < 20_000) | (s > 23_000)  # a stretch without fragments
    s, e, q, st = s[keep], e[keep], q[keep], st[keep]
    r1s = np.where(st != 0, s, np.maximum(e - 50, s)).astype(np.int32)
    r1e = np.where(st != 0, np.minimum(s + 50, e), e).astype(np.int32)
    engine.load_contig("pk:plain", s, e, q, st)
    engine.load_contig("pk:bam", s, e, q, st, r1s, r1e)
    yield size
    engine.release("pk:plain")
    engine.release("pk:bam")


def two_step(engine, key, starts, stops, size, W=1000, sw=21, savgol=True, wps_kw={}, **rule):
    """The route there was before: scores to the host, the adjusted track to the host, then the calls."""
    need = W + max(sw if savgol else 0, 1)
    kept = [i for i in range(len(starts)) if stops[i] - starts[i] >= need]
    scores, offs = engine.wps_intervals(key, starts[kept], stops[kept], size, **wps_kw)
    adj = engine.wps_adjust(np.asarray(scores, np.float64), offs, W, savgol_window_size=sw, savgol=savgol)
    adj_offs = offs - np.arange(len(offs)) * W
    calls, kept_stats = engine.track_peaks(adj, adj_offs, skip=sw // 2 if savgol else 0, **rule)
    shift = starts[kept][calls["run"]] + W // 2
    for name in ("start", "stop", "summit"):
        calls[name] += shift
    calls["run"] = np.asarray(kept, np.int32)[calls["run"]]
    stats = np.zeros((len(starts), 6), np.int64)
    stats[kept] = kept_stats
    return (calls, stats), adj, adj_offs, kept


@pytest.mark.parametrize("key", ["pk:plain", "pk:bam"])
def test_fused_call_equals_the_two_step_route(engine, contigs, key):
    size = contigs
    starts = np.array([30_000, 0, 31_000, 52_000, 18_000, 5_000, 40_000, 12_000, 51_000, 100, 7_000], np.int64)
    stops = np.array([34_000, 2_500, 36_500, 53_020, 25_000, 5_900, 45_000, 13_500, 60_000, 8_293, 7_000], np.int64)
    rule = dict(max_gap=5, min_region=50, short_max=150, max_region=450)
    want, adj, adj_offs, kept = two_step(engine, key, starts, stops, size, **rule)
    assert 5 not in kept and 10 not in kept and 3 not in kept and 7 in kept  # 900 and 0 and 1020 bases are too short, 1500 is not
    assert want[1][:, CALLS].sum() > 100 and np.all(want[1][[3, 5, 10]] == 0)
    assert_same(want, restated(adj, adj_offs, kept, starts, len(starts), skip=10, **rule))  # and the route is the restatement's
    lens = stops - starts
    for batch in (None, 4_096, int(lens.max()), int(lens.sum())):  # 4 096: several batches, the long intervals one each
        assert_same(engine.wps_peaks(key, starts, stops, size, batch_bases=batch, **rule), want, batch)
    want, *_ = two_step(engine, key, starts, stops, size, savgol=False, **rule)
    assert want[1][:, CALLS].sum() > 20
    for batch in (None, 4_096):
        got = engine.wps_peaks(key, starts, stops, size, savgol=False, batch_bases=batch, **rule)
        assert_same(got, want, ("no savgol", batch))
    other = dict(W=500, sw=11, wps_kw=dict(window_size=60, min_length=100, max_length=200, quality_threshold=40))
    want, *_ = two_step(engine, key, starts, stops, size, max_gap=3, min_region=30, short_max=120, max_region=400, **other)
    got = engine.wps_peaks(key, starts, stops, size, median_window_size=500, savgol_window_size=11, max_gap=3, min_region=30,
                           short_max=120, max_region=400, batch_bases=10_000, **other["wps_kw"])
    assert_same(got, want, "other parameters")
    none = engine.wps_peaks(key, starts[[5, 10]], stops[[5, 10]], size)  # nothing with a callable track
    assert len(none[0]) == 0 and np.all(none[1] == 0)


def restated(adj, adj_offs, kept, starts, n_iv, W=1000, **kw):
    """The restatement on the adjusted track, moved to the contig as the fused call does."""
    calls, kept_stats = peaks_ref_runs(adj, adj_offs, **kw)
    shift = starts[kept][calls["run"]] + W // 2
    for name in ("start", "stop", "summit"):
        calls[name] += shift
    calls["run"] = np.asarray(kept, np.int32)[calls["run"]]
    stats = np.zeros((n_iv, 6), np.int64)
    stats[kept] = kept_stats
    return calls, stats


# ---- 5. the C ABI ---------------------------------------------------------------------------------------------------------
def test_argument_errors(engine, contigs):
    import torch
    from finaletoolkit_amd import _lib as L
    lib, ctx, P = engine.lib, engine.ctx, L.ptr
    INV = L.FTK_ERR_INVALID
    rng = np.random.default_rng(9)
    runs = [np.concatenate([-np.ones(12), np.abs(rng.normal(0, 3, 70)) + 0.25, -np.ones(12)]), np.zeros(0), rng.normal(0, 3, 900)]
    scores, offs = pack(runs)
    good_kw = dict(skip=2, max_gap=5, min_region=50, short_max=150, max_region=450)
    good = peaks_ref_runs(scores, offs, **good_kw)
    assert len(good[0]) >= 1
    d_offs = torch.from_numpy(offs).cuda()
    stats = np.full(18, 7, np.int64)

    def track(ctx_=ctx, scores_=scores, offs_=offs, n=3, skip=2, max_gap=5, min_region=50, short_max=150, max_region=450, stats_=stats,
              drop=None):
        ptrs = [C.c_void_p(1) for _ in range(6)]
        count = C.c_int64(7)
        outs = [C.byref(p) for p in ptrs] + [C.byref(count)]
        if drop is not None:
            outs[drop] = None
        rc = lib.ftk_track_peaks(ctx_, P(scores_), P(offs_), n, skip, max_gap, min_region, short_max, max_region, *outs, P(stats_))
        if rc != L.FTK_OK and ctx_ is not None and drop is None:  # a failing call hands out no block
            assert count.value == 0 and all(p.value is None for p in ptrs)
        for p in ptrs:
            if p.value not in (None, 1):
                lib.ftk_buffer_free(p.value)
        return rc

    def failed(rc, word=None, code=INV):
        assert rc == code, (rc, code)
        message = lib.ftk_last_error(ctx)
        assert message and (word is None or word in message), message
        assert_same(engine.track_peaks(scores, offs, **good_kw), good, word)  # the engine still answers a good call

    assert track(ctx_=None) == INV
    for name in ("scores_", "offs_", "stats_"):
        failed(track(**{name: None}), b"NULL")
    for k in range(7):
        failed(track(drop=k), b"NULL")
    failed(track(skip=-1), b"skip")
    for g in (-1, 64):
        failed(track(max_gap=g), b"max_gap")
    failed(track(min_region=0), b"region")
    failed(track(min_region=151), b"region")
    failed(track(short_max=451), b"region")
    failed(track(max_region=1025), b"region")
    failed(track(n=-1), b"n_runs")
    failed(track(offs_=d_offs), b"host")
    failed(track(offs_=np.array([0, 94, 93, 994], np.int64)), b"decrease")
    failed(track(offs_=np.array([-1, 94, 94, 994], np.int64)), b"negative")
    assert np.all(stats == 7)  # none of them wrote
    for bad in (np.nan, np.inf, -np.inf):
        for at in (3, 50, 993):  # outside the callable track, inside a region, at the very end
            v = scores.copy()
            v[at] = bad
            failed(track(scores_=v), b"finite")
    stats[:] = 7
    assert track() == L.FTK_OK and np.array_equal(stats.reshape(3, 6), good[1])
    assert track(skip=0, max_gap=63, min_region=1024, short_max=1024, max_region=1024) == L.FTK_OK  # the limits themselves
    assert track(skip=(1 << 31) - 1) == L.FTK_OK and np.all(stats == 0)  # nothing is callable
    stats[:] = 7
    assert track(n=0) == L.FTK_OK and track(n=0, scores_=None, offs_=None, stats_=None) == L.FTK_OK and np.all(stats == 7)

    cid = engine.contig_id("pk:plain")
    s, e = np.array([100, 5_000, 9_000], np.int64), np.array([4_100, 5_900, 12_500], np.int64)
    d_s = torch.from_numpy(s).cuda()
    from finaletoolkit_amd.engine import savgol_operators
    coef, edge = savgol_operators(21, 2)
    fstats = np.full(18, 7, np.int64)

    def fused(ctx_=ctx, cid_=cid, s_=s, e_=e, n=3, size=60_000, win=120, lo=120, hi=180, q=30, W=1000, sw=21, coef_=coef, edge_=edge,
              max_gap=5, min_region=50, short_max=150, max_region=450, batch=0, stats_=fstats):
        ptrs = [C.c_void_p(1) for _ in range(6)]
        count = C.c_int64(7)
        rc = lib.ftk_wps_peaks(ctx_, cid_, P(s_), P(e_), n, size, win, lo, hi, q, W, sw, P(coef_), P(edge_), max_gap, min_region, short_max,
                               max_region, batch, *[C.byref(p) for p in ptrs], C.byref(count), P(stats_))
        for p in ptrs:
            if p.value not in (None, 1):
                lib.ftk_buffer_free(p.value)
        return rc

    assert fused(ctx_=None) == INV
    for name in ("s_", "e_", "stats_", "coef_", "edge_"):
        failed(fused(**{name: None}))
    failed(fused(s_=d_s), b"host")
    failed(fused(batch=-1), b"batch_bases")
    for W in (0, 999, 2050):
        failed(fused(W=W), b"median_window")
    for sw in (-1, 20):
        failed(fused(sw=sw), b"savgol_window")
    for g in (-1, 64):
        failed(fused(max_gap=g), b"max_gap")
    failed(fused(min_region=0), b"region")
    failed(fused(short_max=451), b"region")
    failed(fused(max_region=1025), b"region")
    failed(fused(n=-1), b"n_iv")
    failed(fused(s_=np.array([-(1 << 30) - 1, 5_000, 9_000], np.int64)), b"interval")  # the validity of ftk_wps_intervals
    failed(fused(e_=np.array([4_100, 5_900, (1 << 31) + 1], np.int64)), b"interval")
    failed(fused(win=0), b"window_size")
    failed(fused(size=-1), b"chrom_size")
    failed(fused(cid_=987_654), None, L.FTK_ERR_NO_CONTIG)
    assert np.all(fstats == 7)
    assert fused(n=0) == L.FTK_OK and np.all(fstats == 7)
    assert fused() == L.FTK_OK
    want = engine.wps_peaks("pk:plain", s, e, 60_000)
    assert np.array_equal(fstats.reshape(3, 6), want[1]) and np.all(want[1][1] == 0) and want[1][0, CALLS] > 5
    assert fused(sw=0, coef_=None, edge_=None) == L.FTK_OK  # without Savitzky-Golay the arrays may be NULL


# ---- 6. the product path --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def product(engine, tmp_path_factory):
    from finaletoolkit_amd import utils
    d = tmp_path_factory.mktemp("peaks")
    sizes = [("nA", 60_000), ("nB", 9_000)]
    frags = {}
    for k, (name, n) in enumerate(sizes):
        s, e, q, st = nucleosome_fragments(n, 190 + k)
        frags[name] = (s.astype(np.int64), e.astype(np.int64), q.astype(np.int64), st.astype(np.int64))
    bam = str(d / "in.bam")
    write_synthetic_bam(bam, sizes, frags)
    frag = str(d / "in.frag.gz")
    utils.frag_export(bam, frag, quality_threshold=0)
    chrom_sizes = str(d / "g.chrom.sizes")
    with open(chrom_sizes, "w") as fh:
        fh.write("".join(f"{c}\t{n}\n" for c, n in sizes))
    rows = [("nA", 0, 6_000, "first"), ("nB", 1_000, 8_000, "b1"), ("nA", 20_000, 29_000, "long"), ("nA", 30_000, 30_900, "short"),
            ("nA", 52_500, 60_000, "last"), ("nB", 0, 9_000, "whole"), ("nA", 31_000, 32_521, "least"), ("nA", 9_000, 9_000, "empty")]
    bed = str(d / "regions.bed")
    with open(bed, "w") as fh:
        fh.write("# regions\n" + "".join(f"{c}\t{a}\t{b}\t{nm}\t0\t{'+-'[i % 2]}\n" for i, (c, a, b, nm) in enumerate(rows)))
    return dict(dir=d, bam=bam, frag=frag, chrom_sizes=chrom_sizes, bed=bed, rows=rows, sizes=dict(sizes))


def test_frag_wps_peaks_with_intervals(engine, product, tmp_path):
    import warnings
    from finaletoolkit_amd import frag, utils
    p = product
    out_frag, sum_frag = str(tmp_path / "frag.bed"), str(tmp_path / "frag.tsv")
    out_bam, sum_bam = str(tmp_path / "bam.bed.gz"), str(tmp_path / "bam.tsv.gz")
    res = utils.frag_wps_peaks(p["frag"], p["bed"], p["chrom_sizes"], out_frag, sum_frag)
    res_bam = utils.frag_wps_peaks(p["bam"], p["bed"], None, out_bam, sum_bam)
    assert res.intervals == p["rows"] == res_bam.intervals
    assert res.calls.dtype == utils.WPS_PEAK_DTYPE and res.stats.shape == (8, 6) and res.stats.dtype == np.int64
    assert res.calls.tobytes() == res_bam.calls.tobytes() and np.array_equal(res.stats, res_bam.stats)
    assert res.callable.tolist() == [4_980, 5_980, 7_980, 0, 6_480, 7_980, 501, 0]
    assert np.all(np.diff(res.calls["interval"]) >= 0)
    for i, (c, a, b, _) in enumerate(p["rows"]):  # interval by interval: the restatement on Engine.wps_adjust's track
        mine = res.calls[res.calls["interval"] == i]
        if b - a < 1_021:
            assert len(mine) == 0 and np.all(res.stats[i] == 0) and np.isnan(res.median_spacing[i])
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            v = np.asarray(frag.wps(p["frag"], c, a, b, p["sizes"][c])["wps"], dtype=np.float64)
        adj = engine.wps_adjust(v, [0, len(v)])
        calls, stats = peaks_ref(adj, skip=10)
        assert np.array_equal(res.stats[i], stats), i
        want = np.array([(i, s + a + 500, e + a + 500, t + a + 500, h, ar) for s, e, t, h, ar in calls], utils.WPS_PEAK_DTYPE)
        assert mine.tobytes() == want.tobytes(), i
        centres = mine["start"] + (mine["stop"] - mine["start"]) // 2
        spacing = float(np.median(np.diff(centres))) if len(mine) > 1 else float("nan")
        assert res.median_spacing[i] == spacing or (np.isnan(spacing) and np.isnan(res.median_spacing[i]))
        if len(mine) >= 10:  # a sanity condition on the input, not a tolerance on the kernel
            assert 185 <= spacing <= 195, (i, spacing)
    assert len(res.calls) > 150 and res.stats[:, CALLS].sum() == len(res.calls)
    # the files, read back
    text = open(out_frag).read()
    assert gzip.open(out_bam, "rt").read() == text and gzip.open(sum_bam, "rt").read() == open(sum_frag).read()
    lines = text.splitlines()
    assert len(lines) == len(res.calls)
    for line, call in zip(lines, res.calls.tolist()):
        i, a, b, summit, height, area = call
        c, _, _, nm = p["rows"][i]
        assert line.split("\t") == [c, str(a), str(b), nm, str(a + (b - a) // 2), str(summit), format(height, ".6g"), format(area, ".6g")]
    summary = open(sum_frag).read().splitlines()
    assert summary[0].split("\t") == ["contig", "start", "stop", "name", "callable", "regions", "open", "short", "long", "flat", "calls",
                                      "median_spacing"]
    assert len(summary) == 9
    for i, line in enumerate(summary[1:]):
        c, a, b, nm = p["rows"][i]
        gap = res.median_spacing[i]
        assert line.split("\t") == [c, str(a), str(b), nm, str(res.callable[i])] + [str(x) for x in res.stats[i]] + [
            "nan" if gap != gap else format(gap, ".6g")]
    # the command line in a child process, from either input
    for tag, args in (("frag", [p["frag"], None, "--chrom-sizes", p["chrom_sizes"]]), ("bam", [p["bam"], None])):
        cli, cli_sum = str(tmp_path / f"cli_{tag}.bed"), str(tmp_path / f"cli_{tag}.tsv")
        args[1] = cli
        r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.peaks", *args, "--intervals", p["bed"], "--summary", cli_sum],
                           cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert open(cli).read() == text and open(cli_sum).read() == open(sum_frag).read()
    # an interval on a contig the input lacks, and one the chrom.sizes file lacks
    other = tmp_path / "other.bed"
    other.write_text("nA\t100\t2900\tg\nnZ\t100\t2900\th\n")
    with pytest.raises(ValueError, match="nZ"):
        utils.frag_wps_peaks(p["bam"], str(other))
    with pytest.raises(ValueError, match="chrom_sizes"):
        utils.frag_wps_peaks(p["frag"], str(other), p["chrom_sizes"])


def test_whole_contigs_do_not_depend_on_the_chunks(engine, product, tmp_path):
    from finaletoolkit_amd import utils
    p = product
    out, summary = str(tmp_path / "whole.bed"), str(tmp_path / "whole.tsv")
    small = utils.frag_wps_peaks(p["frag"], None, p["chrom_sizes"], out, summary, chunk_size=4_096)
    large = utils.frag_wps_peaks(p["frag"], None, p["chrom_sizes"], chunk_size=1 << 20)
    from_bam = utils.frag_wps_peaks(p["bam"], chunk_size=10_000)
    assert small.intervals == [("nA", 0, 60_000, "."), ("nB", 0, 9_000, ".")] == large.intervals == from_bam.intervals
    assert small.calls.tobytes() == large.calls.tobytes() == from_bam.calls.tobytes() and len(small.calls) > 300
    assert small.stats[:, CALLS].tolist() == large.stats[:, CALLS].tolist() == [int(np.sum(small.calls["interval"] == i)) for i in (0, 1)]
    assert small.callable.tolist() == [58_980, 7_980]
    assert np.array_equal(small.median_spacing, large.median_spacing)
    assert np.all((small.median_spacing >= 185) & (small.median_spacing <= 195)), small.median_spacing  # (the input's own spacing)
    # one chunk is one interval: the calls of the interval mode over the whole contig
    bed = tmp_path / "whole_contigs.bed"
    bed.write_text("nA\t0\t60000\t.\nnB\t0\t9000\t.\n")
    as_intervals = utils.frag_wps_peaks(p["frag"], str(bed), p["chrom_sizes"])
    assert as_intervals.calls.tobytes() == large.calls.tobytes() and np.array_equal(as_intervals.stats, large.stats)
    lines = open(out).read().splitlines()
    assert len(lines) == len(small.calls) and all(line.split("\t")[3] == "." for line in lines)
    assert [line.split("\t")[0] for line in lines] == ["nA"] * int(small.stats[0, CALLS]) + ["nB"] * int(small.stats[1, CALLS])
    assert len(open(summary).read().splitlines()) == 3
