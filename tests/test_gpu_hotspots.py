"""GPU: the IFS hotspot kernels (csrc/ftk_hotspots.hip) and the host merge against the numpy restatement of the rule in
``tests/hotspots_helpers.py`` - equal integers, window for window, hotspot for hotspot and counter for counter - on random
fragments, on cases built by hand around the tile bounds, the contig ends and the table's edges, on the merge across tiles,
runs and batches, on both column forms, on a planted case, on the refusals of the C call, and through
``utils.frag_hotspots`` and its command line."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import write_synthetic_bam
from tests.hotspots_helpers import (CALLED, TESTED, Contig, assert_same, at, bin_tracks, columns, flat_table, global_mean_ref,
                                    ifs_hotspots_ref, planted_fragments, random_fragments, totals_ref)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REACH = 1024  # FTK_IFS_MAX_REACH


def tile():
    from finaletoolkit_amd import _lib as L
    return L.HOTSPOTS_TILE


# ---- 1. the rule on random fragments --------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [2, 30])
@pytest.mark.parametrize("s,m", [(1, 1), (20, 10), (7, 64), (1000, 3)])
def test_rule_against_the_restatement(engine, s, m, depth):
    """Every contig size x half-widths x global_mean x min_count x table.  The Poisson table is that of alpha = 0.01; the flat
    table holds the contig's own mean IFS per window, so that about half of the backgrounds lie on either side of it.  A
    combination is held not to be vacuous - a called window, and a tested window that is not called - on the contigs of a
    tile and more: with the flat table where windows pass min_count at all (min_count = 0, or six fragments to a window on
    average); with the Poisson table where the mean integer IFS of a window lies inside the table and well above its first
    entries (between 20 and 200: (20, 10) and (7, 64) at depth 30, (1000, 3) at depth 2) and the first background is wide
    enough for the table to tell a window from it (h1 = 125 and more: with h1 = 1 a window's own bins are most of its
    background).  Elsewhere the restatement says what there is to call - next to nothing - and the kernels say the same."""
    from finaletoolkit_amd import utils
    T, L = tile(), 167
    poisson = utils.ifs_thresholds(0.01, 256)
    halves = [(1, 0), (1, 3), (125, 0), (125, 250), (REACH - m, 0), (125, REACH - m)]
    per_window = depth * 7 / 8 * s * m / L  # fragments of mapq 60 with their midpoint in a window
    bins = sorted({1, m - 1, m, m + 1, 250, T - 1, T, T + 1, 3 * T + 5})
    for k, nb in enumerate(bins):
        size = nb * s - s // 3  # (not divisible by s where s > 1; nb bins all the same)
        assert -(-size // s) == nb
        rng = np.random.default_rng(100_000 * s + 1000 * m + 10 * k + depth)
        with Contig(engine, *random_fragments(rng, size, depth)) as c:
            N, S = totals_ref(*c.cols, size)
            assert engine.ifs_totals(c.name, size) == (N, S)
            gm = global_mean_ref(N, S, L, m, size, s)
            tracks = bin_tracks(*c.cols, size, s, L)
            c.track([0], [size], size, (size, "track"), step=s, m=m, mean_length=L)
            for table, thr in (("poisson", poisson), ("flat", flat_table(max(gm, 1), 4096))):
                for h1, h2 in halves:
                    for use_global in (0, gm):
                        for min_count in (0, 3):
                            what = (size, table, h1, h2, use_global, min_count)
                            win, hot, stats = c.both([0], [size], size, what, tracks, step=s, m=m, mean_length=L, h1=h1, h2=h2,
                                                     min_count=min_count, thresholds=thr, global_mean=use_global)
                            if table == "flat":
                                telling = min_count == 0 or per_window >= 6
                            else:
                                telling = 20 <= 2 * per_window <= 200 and h1 >= 125
                            if nb >= T and telling:
                                assert len(win) >= 1 and stats[0, CALLED] == len(win) and stats[0, TESTED] > len(win), what
                                assert len(hot) >= 1


# ---- 2. cases built by hand -----------------------------------------------------------------------------------------------
def test_exact_cases(engine):
    T = tile()
    size = 3 * T + 5
    # step 1, m = 1, L = 10: fragments of length 10, i = 20 each.  Three on 50 and one on 53: window 50 has n = 3, I = 60,
    # q = 6; h = 3: bins 47 .. 53, B = 80, n_b = 7: B m 1024 >= t n_b L <=> 81920 >= 70 t <=> t <= 1170
    kw = dict(step=1, m=1, mean_length=10, h1=3, h2=0, join=1)
    with Contig(engine, *columns(at([50, 50, 50, 53]))) as c:
        for t, called in ((1170, True), (1171, False)):
            thr = np.zeros(8, np.uint64)
            thr[6] = t
            win, hot, stats = c.both([0], [size], size, t, thresholds=thr, **kw)
            assert stats.tolist() == [[size, size, int(called), int(called), 0, int(called)]]
            if called:
                assert win.tolist() == [(0, 50, 3, 60, 80, 7, 0, 0)] and hot.tolist() == [(0, 50, 51, 1, 50, 60, 3, 80, 7)]
        # the second background on equality: h = 4, n_b = 9: 81920 >= 90 t <=> t <= 910; and the first alone fails it
        for t, h1, h2, called in ((910, 3, 4, True), (911, 3, 4, False), (911, 3, 0, True), (911, 4, 0, False)):
            thr = np.zeros(8, np.uint64)
            thr[6] = t
            win, _, _ = c.both([0], [size], size, (t, h1, h2), thresholds=thr, **dict(kw, h1=h1, h2=h2))
            assert win.tolist() == ([(0, 50, 3, 60, 80, 2 * h1 + 1, 80 if h2 else 0, 9 if h2 else 0)] if called else [])
        # global_mean on equality, and 0 switches it off
        thr = np.zeros(8, np.uint64)
        thr[6] = 910
        for gm, n in ((910, 1), (909, 0), (0, 1)):
            assert len(c.both([0], [size], size, gm, thresholds=thr, global_mean=gm, **kw)[0]) == n
        # min_count: n = 3 is tested at 3 and not at 4
        assert c.both([0], [size], size, thresholds=thr, min_count=3, **kw)[2].tolist() == [[size, 1, 1, 1, 0, 1]]
        assert c.both([0], [size], size, thresholds=thr, min_count=4, **kw)[2].tolist() == [[size, 0, 0, 0, 0, 0]]
        # q == n_thr - 1 reads the last entry; q == n_thr reads nothing; an entry of 0 never calls
        assert len(c.both([0], [size], size, thresholds=np.array([0] * 6 + [910], np.uint64), **kw)[0]) == 1
        win, _, stats = c.both([0], [size], size, thresholds=np.full(6, 1, np.uint64), min_count=1, **kw)
        assert win["pos"].tolist() == [53] and stats[0, 1] == 2
        win, _, stats = c.both([0], [size], size, thresholds=np.array([1, 1, 0, 1, 1, 1, 1], np.uint64), min_count=1, **kw)
        assert win["pos"].tolist() == [50] and stats[0, 1] == 2  # (q = 2 on 53 reads the 0)
        top = np.full(4096, (1 << 32) - 1, np.uint64)  # the largest table there is: nothing reaches such a mean
        assert c.both([0], [size], size, thresholds=top, **kw)[2].tolist() == [[size, size, 0, 0, 0, 0]]
    # midpoints on base 0 and 1 and on the last base, and just outside it ((0 + 1) >> 1 = 0, (0 + 2) >> 1 = 1; a contig holds no
    # negative start, so no midpoint lies in front of base 0)
    every = dict(kw, thresholds=flat_table(1, 64), min_count=1)
    with Contig(engine, *columns((0, 1), (0, 2), at([size - 1]), at([size]), (size - 4, size + 4))) as c:
        win, _, stats = c.both([0], [size], size, **every)
        # backgrounds clipped at either end of the contig: bins 0 .. 3, 0 .. 4 and size - 4 .. size - 1
        assert win.tolist() == [(0, 0, 1, 11, 23, 4, 0, 0), (0, 1, 1, 12, 23, 5, 0, 0), (0, size - 1, 1, 20, 20, 4, 0, 0)]
        assert engine.ifs_totals(c.name, size) == (3, 13) and engine.ifs_totals(c.name, size + 1) == (5, 31)
        win, _, _ = c.both([0], [size], size, **dict(every, h1=REACH - 1))
        assert win["nb1"].tolist() == [REACH, REACH + 1, REACH]
    # called windows on either side of a tile bound; a window of m bins whose bins lie in two tiles; every tile cut
    around = [T - 1, T, T + 1, 2 * T - 1, 2 * T, 3 * T, 3 * T + 4]
    with Contig(engine, *columns(at(around, copies=2))) as c:
        win, _, _ = c.both([0], [size], size, **every)
        assert win["pos"].tolist() == around and win["count"].tolist() == [2] * 7 and win["bg1"].tolist() == [120, 120, 120, 80, 80, 40, 40]
        wide = dict(every, m=4, h1=5, h2=9)  # window k: bins k .. k + 3
        win, _, _ = c.both([0, T - 3, 0], [size, T + 9, T + 1], size, **wide)
        mine = win[win["run"] == 1]
        assert mine["pos"].tolist() == [T - 3, T - 2, T - 1, T, T + 1] and mine["count"].tolist() == [4, 6, 6, 4, 2]
        assert win[win["run"] == 2]["pos"].tolist() == [T - 4, T - 3]  # (window T - 2 would end on T + 2)
        c.track([0, T - 3, 0, 7, 7], [size, T + 9, T + 1, 7, 10], size, step=1, m=4, mean_length=10)
    # mapq and length on either side of each bound
    s, e, q = columns((100, 110), (200, 211), (300, 312), (400, 411), (500, 511))
    q[:] = [30, 30, 30, 29, 31]
    with Contig(engine, s, e, q) as c:
        assert c.both([0], [size], size, min_length=11, max_length=11, quality_threshold=30, **every)[0]["pos"].tolist() == [205, 505]
        assert c.both([0], [size], size, min_length=10, max_length=12, quality_threshold=31, **every)[0]["pos"].tolist() == [505]
        assert c.both([0], [size], size, min_length=12, quality_threshold=0, **every)[0]["pos"].tolist() == [306]
        assert c.both([0], [size], size, max_length=10, quality_threshold=29, **every)[0]["pos"].tolist() == [105]
    # 70 000 copies of one fragment: counts above 65 535 are exact
    with Contig(engine, *columns(at(np.full(70_000, 300)), at([310]))) as c:
        win, _, _ = c.both([0], [size], size, **dict(every, thresholds=flat_table(1, 4096), mean_length=1, h1=20))
        assert win.tolist() == [(0, 310, 1, 11, 770_011, 41, 0, 0)]  # (q = 770 000 on 300 is beyond the table)


def test_a_long_fragment_reaches_a_later_tile_by_its_midpoint_alone(engine):
    """A fragment of 60 000 bases, admitted because max_length is open: it starts in the first tile of windows and its
    midpoint lies in the ninth (the candidates of a tile reach back by the longest admissible fragment)."""
    T = tile()
    size = 10 * T
    t0 = 8 * T
    mid = t0 + 100
    assert 0 <= mid - 30_000 < T
    every = dict(step=1, m=1, mean_length=10, h1=3, h2=0, join=1, thresholds=flat_table(1, 4096), min_count=1)
    with Contig(engine, *columns((mid - 30_000, mid + 30_000), at([500, t0 + 102, t0 + T + 7]))) as c:
        win, hot, _ = c.both([0, t0, t0 + 100], [size, t0 + T, t0 + 101], size, **dict(every, mean_length=60_000))
        assert win[win["run"] == 0]["pos"].tolist() == [500, mid, mid + 2, t0 + T + 7]
        assert win[win["run"] == 2].tolist() == [(2, mid, 1, 120_000, 180_010, 7, 0, 0)]
        win, _, stats = c.both([t0], [t0 + T], size, max_length=1_000, **every)  # filtered out: not a candidate either
        assert win["pos"].tolist() == [mid + 2] and stats[0, 1] == 1
        c.track([0, t0 + 90], [size, t0 + 110], size, step=1, m=1, mean_length=60_000)


# ---- 3. the merge ---------------------------------------------------------------------------------------------------------
def test_merge(engine):
    from finaletoolkit_amd import _lib as L
    T, BATCH = tile(), L.HOTSPOTS_BATCH_TILES
    size = 3 * T + 5
    kw = dict(step=1, m=1, mean_length=10, h1=3, h2=0, thresholds=flat_table(1, 4096), min_count=1)
    # a fragment on every base: everything is called and one hotspot spans the three tiles
    with Contig(engine, *columns((np.arange(size), np.arange(size) + 1))) as c:
        win, hot, stats = c.both([0], [size], size, join=1, **kw)
        assert len(win) == size and hot.tolist() == [(0, 0, size, size, 0, 11, 1, 44, 4)] and stats.tolist() == [[size, size, size, 1, 0, size]]
        # two overlapping intervals: a hotspot each, none across the runs
        _, hot, stats = c.both([0, T - 7], [2 * T, size], size, join=1, **kw)
        assert hot[["run", "start", "stop", "n_windows"]].tolist() == [(0, 0, 2 * T, 2 * T), (1, T - 7, size, 2 * T + 12)]
    # gaps of exactly join and join + 1, across a tile bound as well; min_windows drops the short ones; equal minima: the leftmost
    ks = [10, 11, 12, 14, 20, T - 1, T, T + 1, T + 3, T + 4, 2 * T - 1, 2 * T + 1]
    copies = [3, 2, 2, 5, 1, 4, 2, 3, 2, 9, 1, 1]
    cols = columns(*[at([k], copies=n) for k, n in zip(ks, copies)])
    with Contig(engine, *cols) as c:
        _, hot, stats = c.both([0], [size], size, join=1, **kw)
        assert hot[["start", "stop", "n_windows", "summit", "count"]].tolist() == [
            (10, 13, 3, 11, 2), (14, 15, 1, 14, 5), (20, 21, 1, 20, 1), (T - 1, T + 2, 3, T, 2), (T + 3, T + 5, 2, T + 3, 2),
            (2 * T - 1, 2 * T, 1, 2 * T - 1, 1), (2 * T + 1, 2 * T + 2, 1, 2 * T + 1, 1)]
        _, hot, stats = c.both([0], [size], size, join=2, min_windows=2, **kw)
        assert hot[["start", "stop", "n_windows", "summit", "count"]].tolist() == [
            (10, 15, 4, 11, 2), (T - 1, T + 5, 5, T, 2), (2 * T - 1, 2 * T + 2, 2, 2 * T - 1, 1)]
        assert stats.tolist() == [[size, 12, 12, 3, 1, 5 + 6 + 3]]
        _, hot, _ = c.both([0, 12, T], [size, T + 1, T + 4], size, join=2, min_windows=2, **kw)
        assert hot[["run", "start", "stop"]].tolist() == [(0, 10, 15), (0, T - 1, T + 5), (0, 2 * T - 1, 2 * T + 2), (1, 12, 15), (1, T - 1, T + 1),
                                                          (2, T, T + 4)]
        # windows of m bins: a hotspot's stop is its last window's span end, and kept hotspots that overlap are covered once
        wide = dict(kw, m=4, thresholds=flat_table(1, 4096))
        _, hot, stats = c.both([0], [30], size, join=1, **wide)
        assert hot[["start", "stop", "n_windows"]].tolist() == [(7, 18, 8), (17, 24, 4)] and stats[0, 5] == 17
    # BATCH + 5 intervals of one window are as many tiles: the calls come home in two pieces, every run by itself
    with Contig(engine, *columns(at(np.arange(2_000, 3_000 + BATCH + 2_000)))) as c:
        starts = np.arange(3_000, 3_000 + BATCH + 5, dtype=np.int64)
        win, hot, stats = c.both(starts, starts + 1, 3 * BATCH, join=5, **kw)
        assert len(win) == BATCH + 5 == len(hot) and np.all(stats == [1, 1, 1, 1, 0, 1]) and hot["run"].tolist() == list(range(BATCH + 5))


def test_a_hotspot_crosses_the_batch_boundary(engine):
    """One interval of more tiles than a batch holds (step 1, sparse fragments): the called windows on either side of the
    last tile bound of the first batch come home in two pieces and are one hotspot."""
    from finaletoolkit_amd import _lib as L
    T, BATCH = tile(), L.HOTSPOTS_BATCH_TILES
    edge = BATCH * T
    size = edge + T + 9
    kw = dict(step=1, m=1, mean_length=10, h1=3, h2=0, thresholds=flat_table(1, 64), min_count=1, join=2)
    mids = [77, edge - 5, edge - 3, edge - 1, edge, edge + 2, edge + 5, size - 1]
    with Contig(engine, *columns(at(mids, copies=2), at([edge + 2]))) as c:
        win, hot, stats = c.both([0], [size], size, **kw)
        assert win["pos"].tolist() == mids
        assert hot[["start", "stop", "n_windows", "summit", "count"]].tolist() == [
            (77, 78, 1, 77, 2), (edge - 5, edge + 3, 5, edge - 5, 2), (edge + 5, edge + 6, 1, edge + 5, 2), (size - 1, size, 1, size - 1, 2)]
        assert stats.tolist() == [[size, 8, 8, 4, 0, 11]]


# ---- 4. the columns -------------------------------------------------------------------------------------------------------
def test_packed_and_wide_columns_give_the_same_bytes(engine):
    from finaletoolkit_amd import utils
    T = tile()
    s, m = 20, 10
    size = (3 * T + 5) * s - 7
    rng = np.random.default_rng(77)
    fs, fe, fq = random_fragments(rng, size, 30)
    fq[::5] = 31  # saturated in the packed word
    thr = utils.ifs_thresholds(0.01, 256)
    starts, stops = [0, (T - 9) * s], [size, (2 * T + 9) * s]
    answers = []
    for long_one, read1 in ((False, False), (True, False), (False, True)):
        s2, e2, q2 = (np.append(fs, 700), np.append(fe, 700 + 2_047), np.append(fq, 60)) if long_one else (fs, fe, fq)
        with Contig(engine, s2, e2, q2, read1=read1) as c:
            assert engine.frags_packed(c.name) == (not long_one and not read1)
            got = [c.both(starts, stops, size, step=s, m=m, h1=h1, h2=h2, thresholds=thr, max_length=max_length, quality_threshold=cut)
                   for h1, h2 in ((125, 250), (REACH - m, 0))
                   # (a cut above 31 or an upper bound of 2047 and more keep the wide columns on a packed contig, too)
                   for max_length, cut in ((None, 30), (1_000, 31), (None, 32), (2_047, 30))]
            tracks = [c.track(starts, stops, size, step=s, m=m, max_length=max_length, quality_threshold=cut)
                      for max_length, cut in ((None, 30), (None, 32))]
            if not long_one:
                answers.append((got, tracks))
    (a_hot, a_trk), (b_hot, b_trk) = answers  # a BAM-style contig with read1 columns gives the same bytes
    for a, b in zip(a_hot, b_hot):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a[0]) > 10
    for a, b in zip(a_trk, b_trk):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 5. intervals ---------------------------------------------------------------------------------------------------------
def test_intervals(engine):
    from finaletoolkit_amd import utils
    T = tile()
    s, m = 20, 10
    size = (3 * T + 5) * s - 7
    thr = utils.ifs_thresholds(0.01, 256)
    kw = dict(step=s, m=m, thresholds=thr, join=m)
    fields = ["pos", "count", "ifs", "bg1", "nb1", "bg2", "nb2"]
    with Contig(engine, *random_fragments(np.random.default_rng(5), size, 30)) as c:
        whole, whole_hot, whole_stats = c.both([0], [size], size, **kw)
        assert len(whole) > 30 and len(whole_hot) > 5
        # unordered, overlapping, touching and empty intervals: each holds the whole contig's called windows that lie in it
        starts = np.array([2 * T * s, 0, 100, T * s - 1, 700, 700, size, 5_000, (3 * T - 10) * s, 3], np.int64)
        stops = np.array([size, T * s, 100, T * s + 1, 9_000, 9_000, size, 5_199, size, size - 1], np.int64)
        win, hot, stats = c.both(starts, stops, size, **kw)
        for r, (a, b) in enumerate(zip(starts, stops)):
            mine = win[win["run"] == r]
            want = whole[(whole["pos"] >= a) & (np.minimum(whole["pos"] + m * s, size) <= b)]
            assert mine[fields].tolist() == want[fields].tolist()
        assert np.all(stats[[2, 3, 6, 7]] == 0) and np.array_equal(stats[4], stats[5]) and stats[8, 0] == 6
        c.track(starts, stops, size, step=s, m=m)
        # two calls in a row return the same bytes
        again = engine.ifs_hotspots(c.name, starts, stops, size, **kw)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(again, (win, hot, stats)))
        none = engine.ifs_hotspots(c.name, [], [], size, thresholds=thr)
        assert len(none[0]) == 0 and len(none[1]) == 0 and none[2].shape == (0, 6)
        assert [len(x) for x in engine.ifs_track(c.name, [], [], size)] == [0, 0, 1]
    with Contig(engine, np.zeros(0), np.zeros(0), np.zeros(0)) as c:  # an empty contig, and one without a base
        win, hot, stats = c.both([0, 10], [size, 10], size, **kw)
        assert len(win) == 0 and len(hot) == 0 and stats.tolist() == [[3 * T + 5 - m + 1, 3 * T + 5 - m + 1, 0, 0, 0, 0], [0] * 6]
        win, hot, stats = c.both([0], [0], 0, **kw)
        assert len(win) == 0 and np.all(stats == 0)
        assert engine.ifs_totals(c.name, size) == (0, 0)


# ---- 6. the planted case --------------------------------------------------------------------------------------------------
def test_planted_hotspots(engine):
    from finaletoolkit_amd import utils
    size, centres, cols = planted_fragments()
    s, m, L = 20, 10, 167
    thr = utils.ifs_thresholds(1e-5, 256)
    N, S = totals_ref(*cols, size)
    kw = dict(step=s, m=m, mean_length=L, h1=125, h2=250, thresholds=thr, global_mean=global_mean_ref(N, S, L, m, size, s), join=m)
    _, hot, _ = ifs_hotspots_ref(*cols, [0], [size], size, **kw)
    planted = [h for h in hot if any(h["start"] <= c < h["stop"] for c in centres)]
    assert len(planted) == 3 and all(h["n_windows"] >= 10 for h in planted)
    others = [h for h in hot if not any(h["start"] <= c < h["stop"] for c in centres)]
    assert len(others) <= 10 and all(h["n_windows"] <= 5 for h in others)
    with Contig(engine, *cols) as c:
        assert engine.ifs_totals(c.name, size) == (N, S)
        c.both([0], [size], size, **kw)
        _, kept, stats = c.both([0], [size], size, min_windows=6, **kw)
        assert len(kept) == 3 and stats[0, 3:5].tolist() == [3, len(others)]


# ---- 7. the refusals of the C call ----------------------------------------------------------------------------------------
def test_argument_errors(engine):
    import torch
    from finaletoolkit_amd import _lib as L
    lib, ctx, P = engine.lib, engine.ctx, L.ptr
    INV = L.FTK_ERR_INVALID
    size = 5_000
    cols = random_fragments(np.random.default_rng(3), size, 30)
    s, e = np.array([0, 1_000, 4_000], np.int64), np.array([900, 1_000, 5_000], np.int64)
    thr = flat_table(1, 64)
    base = dict(step=2, m=3, mean_length=167, h1=7, h2=9, min_count=0, thresholds=thr, global_mean=0, join=3, min_windows=1)
    with Contig(engine, *cols) as c:
        cid = engine.contig_id(c.name)
        good = c.both(s, e, size, **base)
        assert len(good[0]) >= 1 and len(good[1]) >= 1
        stats = np.full(18, 7, np.int64)
        d_s, d_thr, d_stats = torch.from_numpy(s).cuda(), torch.from_numpy(thr.view(np.int64)).cuda(), torch.from_numpy(stats).cuda()

        def call(ctx_=ctx, cid_=cid, s_=s, e_=e, n=3, size_=size, step=2, m=3, mean_len=167, h1=7, h2=9, min_count=0, thr_=thr,
                 n_thr=len(thr), gm=0, join=3, min_windows=1, stats_=stats, drop=None):
            ptrs = [C.c_void_p(1) for _ in range(17)]
            nw, nh = C.c_int64(7), C.c_int64(7)
            outs = [C.byref(p) for p in ptrs[:8]] + [C.byref(nw)] + [C.byref(p) for p in ptrs[8:]] + [C.byref(nh)]
            if drop is not None:
                outs[drop] = None
            rc = lib.ftk_ifs_hotspots(ctx_, cid_, P(s_), P(e_), n, size_, step, m, mean_len, h1, h2, min_count, P(thr_), n_thr, gm, join,
                                      min_windows, -1, -1, 30, *outs, P(stats_))
            if rc != L.FTK_OK and ctx_ is not None and drop is None:  # a refused call leaves the output pointers NULL
                assert nw.value == 0 and nh.value == 0 and all(p.value is None for p in ptrs)
            for p in ptrs:
                if p.value not in (None, 1):
                    lib.ftk_buffer_free(p.value)
            return rc

        def failed(rc, word=None, code=INV):
            assert rc == code, (rc, code, word)
            message = lib.ftk_last_error(ctx)
            assert message and (word is None or word in message), message
            assert_same(engine.ifs_hotspots(c.name, s, e, size, **base), good, word)  # a good call still answers

        assert call(ctx_=None) == INV
        for name in ("s_", "e_", "thr_", "stats_"):
            failed(call(**{name: None}), b"NULL")
        for k in range(19):
            failed(call(drop=k), b"NULL")
        for name, dev in (("s_", d_s), ("e_", d_s), ("thr_", d_thr), ("stats_", d_stats)):
            failed(call(**{name: dev}), b"host")
        failed(call(n=-1), b"n_iv")
        failed(call(s_=np.array([-1, 1_000, 4_000], np.int64)), b"interval")
        failed(call(e_=np.array([900, 999, 5_000], np.int64)), b"interval")
        failed(call(e_=np.array([900, 1_000, 5_001], np.int64)), b"interval")
        for bad in (-1, 1 << 30):
            failed(call(size_=bad, n=0), b"chrom_size")
        for bad in (0, -1, 65_536):
            failed(call(step=bad), b"step")
        for bad in (0, -1, 65):
            failed(call(m=bad), b"m ")
        for bad in (0, -1, 65_536):
            failed(call(mean_len=bad), b"mean_len")
        for bad in (0, -1):
            failed(call(h1=bad), b"h1")
        for bad in (-1, 6):
            failed(call(h2=bad), b"h2")
        failed(call(h1=REACH - 2, h2=0), b"exceeds")
        failed(call(h2=REACH - 2), b"exceeds")
        failed(call(min_count=-1), b"min_count")
        for bad in (0, -1, 4_097):
            failed(call(n_thr=bad), b"n_thr")
        over = thr.copy()
        over[3] = 1 << 32
        failed(call(thr_=over), b"threshold")
        failed(call(gm=-1), b"global_mean")
        for bad in (0, -1, 1_025):
            failed(call(join=bad), b"join")
        for bad in (0, -1):
            failed(call(min_windows=bad), b"min_windows")
        failed(call(cid_=987_654), None, L.FTK_ERR_NO_CONTIG)
        assert np.all(stats == 7)  # none of them wrote a counter
        assert call(n=0) == L.FTK_OK and call(n=0, s_=None, e_=None, stats_=None) == L.FTK_OK and np.all(stats == 7)
        assert call() == L.FTK_OK and np.array_equal(stats.reshape(3, 6), good[2])
        # the limits themselves
        assert call(step=65_535, m=1, mean_len=65_535, h1=1, h2=0, join=1_024, n_thr=1) == L.FTK_OK
        assert call(m=64, h1=REACH - 64, h2=REACH - 64, join=1) == L.FTK_OK
        top = np.full(4_096, (1 << 32) - 1, np.uint64)
        assert call(thr_=top, n_thr=4_096, size_=(1 << 30) - 1, gm=(1 << 62)) == L.FTK_OK
        # the track call refuses what it has of these
        n_out, i_out, offs = np.full(10_000, 7, np.int32), np.full(10_000, 7, np.int64), np.zeros(3, np.int64)

        def track(s_=s, e_=e, n=3, o_=offs, size_=size, step=2, m=3, mean_len=167, cid_=cid):
            return lib.ftk_ifs_track(ctx, cid_, P(s_), P(e_), n, P(o_), size_, step, m, mean_len, -1, -1, 30, P(n_out), P(i_out))
        for kwargs in (dict(s_=None), dict(o_=None), dict(o_=d_s), dict(n=-1), dict(e_=np.array([900, 999, 5_000], np.int64)),
                       dict(size_=1 << 30, n=0), dict(step=0), dict(m=65), dict(mean_len=0), dict(o_=np.array([0, -1, 0], np.int64))):
            assert track(**kwargs) == INV, kwargs
        assert track(cid_=987_654) == L.FTK_ERR_NO_CONTIG
        assert np.all(n_out == 7) and np.all(i_out == 7)
        with pytest.raises(L.FtkError):
            engine.ifs_totals(c.name, 1 << 30)


# ---- 8. the product path --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def product(engine, tmp_path_factory):
    from finaletoolkit_amd import utils
    d = tmp_path_factory.mktemp("hotspots")
    sizes = [("hA", 400_000), ("hB", 30_000)]
    frags = {}
    size, _, (s, e, q) = planted_fragments()
    e = np.minimum(e, size)  # (a BAM holds no alignment beyond its contig)
    keep = e > s
    frags["hA"] = (s[keep], e[keep], q[keep], np.arange(keep.sum()) % 2)
    s, e, q = random_fragments(np.random.default_rng(41), 30_000, 30, mean=150.0)  # (a mean length of its own)
    e = np.minimum(e, 30_000)
    keep = e > s
    frags["hB"] = (s[keep].astype(np.int64), e[keep].astype(np.int64), q[keep].astype(np.int64), np.arange(keep.sum()) % 2)
    bam = str(d / "in.bam")
    decoded = write_synthetic_bam(bam, sizes, frags)
    rows = {c: tuple(np.array([r[k] for r in decoded[c]], np.int64) for k in range(3)) for c, _ in sizes}
    frag = str(d / "in.frag.gz")
    utils.frag_export(bam, frag, quality_threshold=0)
    chrom_sizes = str(d / "g.chrom.sizes")
    with open(chrom_sizes, "w") as fh:
        fh.write("".join(f"{c}\t{n}\n" for c, n in sizes))
    bed_rows = [("hA", 90_000, 110_000, "first"), ("hB", 1_000, 24_000, "b1"), ("hA", 195_007, 500_000, "beyond"), ("hA", 3_000, 3_150, "short"),
                ("hB", 0, 30_000, "whole"), ("hA", 9_000, 9_000, "empty"), ("hA", 99_000, 101_000, "overlap")]
    bed = str(d / "regions.bed")
    with open(bed, "w") as fh:
        fh.write("# regions\n" + "".join(f"{c}\t{a}\t{b}\t{nm}\t0\t{'+-'[i % 2]}\n" for i, (c, a, b, nm) in enumerate(bed_rows)))
    return dict(dir=d, bam=bam, frag=frag, chrom_sizes=chrom_sizes, bed=bed, rows=bed_rows, sizes=dict(sizes), frags=rows)


def restated(p, intervals, step=20, window=200, background=(5000, 10000), alpha=1e-5, mean_length=None, use_global=True, min_count=0,
             join=None, min_windows=1, quality_threshold=30):
    """The ``utils.IfsHotspots`` of the product over ``intervals`` (clipped to their contigs) by the restatement, on the decoded rows."""
    from finaletoolkit_amd import utils
    m = window // step
    h1, h2 = (b // (2 * step) for b in background)
    thr = utils.ifs_thresholds(alpha)
    hots, wins, stats = [], [], np.zeros((len(intervals), 6), np.int64)
    means, globs = np.zeros(len(intervals), np.int64), np.zeros(len(intervals), np.int64)
    for i, (c, a, b, _) in enumerate(intervals):
        size = p["sizes"][c]
        N, S = totals_ref(*p["frags"][c], size, quality_threshold=quality_threshold)
        L = mean_length if mean_length is not None else (min(max((2 * S + N) // (2 * N), 1), 65535) if N else 1)
        gm = global_mean_ref(N, S, L, m, size, step) if use_global else 0
        win, hot, stats[i] = ifs_hotspots_ref(*p["frags"][c], [min(a, size)], [min(b, size)], size, step=step, m=m, mean_length=L, h1=h1,
                                              h2=h2, min_count=min_count, thresholds=thr, global_mean=gm,
                                              join=m + 200 // step if join is None else join, min_windows=min_windows,
                                              quality_threshold=quality_threshold)
        means[i], globs[i] = L, gm
        hp = np.zeros(len(hot), utils.HOTSPOT_DTYPE)
        hp["interval"] = i
        for f in utils.HOTSPOT_DTYPE.names[1:]:
            hp[f] = hot[f]
        wp = np.zeros(len(win), utils.IFS_WINDOW_DTYPE)
        wp["interval"], wp["start"], wp["stop"] = i, win["pos"], np.minimum(win["pos"] + m * step, size)
        for f in utils.IFS_WINDOW_DTYPE.names[3:]:
            wp[f] = win[f]
        hots.append(hp)
        wins.append(wp)
    return utils.IfsHotspots(list(intervals), np.concatenate(hots), np.concatenate(wins), stats, means, globs, step, m)


def same_result(got, want):
    assert got.intervals == want.intervals and (got.step, got.window_bins) == (want.step, want.window_bins)
    assert got.hotspots.dtype == want.hotspots.dtype and got.hotspots.tobytes() == want.hotspots.tobytes()
    assert got.windows.dtype == want.windows.dtype and got.windows.tobytes() == want.windows.tobytes()
    for a, b in ((got.stats, want.stats), (got.mean_length, want.mean_length), (got.global_mean, want.global_mean)):
        assert a.dtype == np.int64 and np.array_equal(a, b)


def written(tmp_path, tag, res):
    """The three files of a result, written by the writers."""
    from finaletoolkit_amd import writers
    paths = [str(tmp_path / f"{tag}.bed"), str(tmp_path / f"{tag}.win.bed"), str(tmp_path / f"{tag}.tsv")]
    writers.write_hotspot_rows(paths[0], res)
    writers.write_hotspot_windows(paths[1], res)
    writers.write_hotspot_summary(paths[2], res)
    return [open(path).read() for path in paths]


def test_frag_hotspots_with_intervals(engine, product, tmp_path):
    from finaletoolkit_amd import utils
    p = product
    out = [str(tmp_path / name) for name in ("frag.bed", "frag.win.bed", "frag.tsv")]
    out_bam = [str(tmp_path / name) for name in ("bam.bed.gz", "bam.win.bed.gz", "bam.tsv.gz")]
    opts = dict(alpha=1e-3, join=10)
    res = utils.frag_hotspots(p["frag"], p["bed"], p["chrom_sizes"], *out, **opts)
    res_bam = utils.frag_hotspots(p["bam"], p["bed"], None, *out_bam, **opts)
    want = restated(p, p["rows"], **opts)
    assert want.intervals == p["rows"] and len(want.hotspots) > 5 and len(want.windows) > 40 and want.stats[[3, 5]].sum() == 0
    assert set(want.hotspots["interval"]) >= {0, 2, 6} and want.mean_length[0] != want.mean_length[1]
    same_result(res, want)
    same_result(res_bam, want)
    texts = written(tmp_path, "want", want)
    assert [open(path).read() for path in out] == texts and [gzip.open(path, "rt").read() for path in out_bam] == texts
    assert len(texts[0].splitlines()) == len(want.hotspots) and len(texts[2].splitlines()) == 8
    # the command line in a child process
    cli = [str(tmp_path / name) for name in ("cli.bed", "cli.win.bed", "cli.tsv")]
    r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.hotspots", p["frag"], cli[0], "--chrom-sizes", p["chrom_sizes"], "--intervals",
                        p["bed"], "--windows", cli[1], "--summary", cli[2], "--alpha", "1e-3", "--join", "10"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert [open(path).read() for path in cli] == texts
    # an interval on a contig the input lacks, and one the chrom.sizes file lacks
    other = tmp_path / "other.bed"
    other.write_text("hA\t100\t2900\tg\nhZ\t100\t2900\th\n")
    with pytest.raises(ValueError, match="hZ"):
        utils.frag_hotspots(p["bam"], str(other))
    with pytest.raises(ValueError, match="chrom_sizes"):
        utils.frag_hotspots(p["frag"], str(other), p["chrom_sizes"])


def test_whole_contigs(engine, product, tmp_path):
    """Without an interval file every contig is one interval, which the C call tiles: the planted sites of hA come out of the
    defaults (alpha = 1e-5, each contig's own mean length and mean IFS), and the result is the restatement's, which knows no
    tiles."""
    from finaletoolkit_amd import utils
    p = product
    whole = [("hA", 0, 400_000, "."), ("hB", 0, 30_000, ".")]
    out = [str(tmp_path / name) for name in ("whole.bed", "whole.win.bed", "whole.tsv")]
    res = utils.frag_hotspots(p["frag"], None, p["chrom_sizes"], *out, min_windows=6)
    from_bam = utils.frag_hotspots(p["bam"], min_windows=6)
    want = restated(p, whole, min_windows=6)
    same_result(res, want)
    same_result(from_bam, want)
    assert [(h["interval"], h["start"] <= c < h["stop"]) for h, c in zip(res.hotspots, (100_000, 200_000, 300_000))] == [(0, True)] * 3
    assert len(res.hotspots) == 3 and res.stats[0, 3] == 3 and res.stats[0, 4] >= 1
    texts = written(tmp_path, "want", want)
    assert [open(path).read() for path in out] == texts
    lines = texts[0].splitlines()
    assert len(lines) == 3 and all(line.split("\t")[3] == "." and float(line.split("\t")[9]) >= 5.0 for line in lines)
    # other settings: a fixed mean length, no global test, one background given as a number's pair, a mapq cut of 0
    opts = dict(mean_length=150, use_global=False, background=(4000, 4000), alpha=1e-4, step=10, window=100, min_count=1, quality_threshold=0)
    same_result(utils.frag_hotspots(p["bam"], **opts), restated(p, whole, **opts))
    # the command line writes the same files as the function
    cli = [str(tmp_path / name) for name in ("cli.bed.gz", "cli.win.bed.gz", "cli.tsv.gz")]
    r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.hotspots", p["bam"], cli[0], "--windows", cli[1], "--summary", cli[2],
                        "--min-windows", "6"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert [gzip.open(path, "rt").read() for path in cli] == texts
