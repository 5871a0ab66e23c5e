"""The IFS hotspot kernels (csrc/ftk_hotspots.hip) at their limits, against the restatement of ``tests/hotspots_helpers.py``,
equal integers throughout:

A. LDS prefix sums that pass 2^32 inside a tile while every window and background stays below it (rule 4, "nothing
   overflows"), with backgrounds above 2^31;
B. fragments just below 2^30 (the twin contigs of ``tests/test_gpu_top_coordinates.py``): small steps through a low twin,
   the whole contig as one interval of four batches, and steps up to 65535 against the restatement directly;
C. ``max(h1, h2) + m`` on either side of 512, where ``ifs_kernel<512>`` gives way to ``ifs_kernel<1024>``;
D. ``join`` = FTK_IFS_MAX_JOIN and ``q`` on either side of ``n_thr`` = FTK_IFS_MAX_THR, by hand.

What makes a case worth its run - a prefix that wraps, a clipped background among the calls, a tested window that is not
called, data in the outermost bins a tile reads - is asserted from the restatement in tests without the ``gpu`` mark."""
import functools

import numpy as np
import pytest

from finaletoolkit_amd._lib import HOTSPOTS_BATCH_TILES as BATCH
from finaletoolkit_amd._lib import HOTSPOTS_TILE as T  # windows per workgroup
from finaletoolkit_amd._lib import IFS_MAX_JOIN as MAX_JOIN
from finaletoolkit_amd._lib import IFS_MAX_REACH as REACH
from finaletoolkit_amd._lib import IFS_MAX_THR as MAX_THR
from finaletoolkit_amd._lib import FtkError
from tests.hotspots_helpers import (BASES, CALLED, KEPT, TESTED, WINDOWS, Contig, assert_same, at, backgrounds, bin_tracks,
                                    columns, flat_table, global_mean_ref, ifs_hotspots_ref, interval_windows, random_fragments,
                                    same_records, totals_ref, window_sums)
from tests.test_gpu_top_coordinates import SHIFT, SPAN, TOP, twin_columns

gpu = pytest.mark.gpu
HALO = 512  # kIfsHaloSmall of csrc/ftk_hotspots.h: the halo of the smaller instantiation
TWO32 = 1 << 32


def frozen(*cols):
    for c in cols:
        c.setflags(write=False)
    return cols


# ---- A. wrapped prefix sums -----------------------------------------------------------------------------------------------
WRAP = dict(step=4096, m=4, mean_length=167, h1=8, h2=16, min_count=1)
LONG = (1 << 30) - (1 << 20)
# how far the long fragments are moved up: not at all (ten midpoints in tile 31 of the whole-contig call, two in tile 32,
# which counts only three of them and does not wrap) and by fifty bins (six on either side of the bound between the two
# tiles, both of which wrap).  (2^19 would put all twelve into tile 32 and the last fragments' ends beyond 2^30.)
LAYOUTS = (0, 50 * 4096)


@functools.lru_cache(maxsize=None)
def wrap_columns(shift):
    """Twelve fragments of 2^30 - 2^20 bases, their midpoints 13 bins of 4096 apart; 4 000 of 10-199 bases with their
    midpoints within 3 (h2 + m) bins of those; three at the very top of the contig."""
    rng = np.random.default_rng(4096 + shift)
    ls = shift + np.arange(12, dtype=np.int64) * 13 * 4096
    lb = (ls + (LONG >> 1)) // 4096
    reach = 3 * (WRAP["h2"] + WRAP["m"])
    mid = rng.integers((lb.min() - reach) * 4096, (lb.max() + reach + 1) * 4096, 4_000)
    ln = rng.integers(10, 200, len(mid))
    s = np.concatenate([ls, mid - ln // 2, [TOP - 1, TOP - 150, TOP - 65_545]])
    e = np.concatenate([ls + LONG, mid - ln // 2 + ln, [TOP, TOP, TOP - 65_435]])
    o = np.argsort(s, kind="stable")
    return frozen(s[o], e[o], np.full(len(s), 60, np.int64))


def wrap_intervals(shift):
    """The whole contig, and three intervals that cut through the long midpoints' tiles (one on a bin's bound, one inside
    a bin, one from the middle of the midpoints to the contig's end)."""
    lb = (shift + (LONG >> 1)) // 4096
    return ([0], [TOP]), ([0, (lb + 6) * 4096 + 5, (lb + 66) * 4096], [(lb + 56) * 4096, (lb + 156) * 4096 - 1, TOP])


def tile_reads(k0, length, m, reach):
    """The bins whose counts a tile of ``length`` windows from ``k0`` holds in LDS: ``[lo, hi)``."""
    return k0 - reach, k0 + length + m - 1 + reach


@pytest.mark.parametrize("shift", LAYOUTS)
def test_wrapped_prefix_sums_from_the_data(shift):
    """Measured (layout 0 | fifty bins up): the prefixes that tiles 31 and 32 of the whole-contig call scan 2.997 and 0.749 |
    1.998 and 1.748 x 2^32, those of the cut intervals' tiles 1.499, 2.997 and 1.998 x 2^32 in both; the largest second
    background 0.749 x 2^32 and the largest window 0.250 x 2^32 in both; 224 called windows of 272 tested, 60 of them with a
    second background above 2^31."""
    s, e, q = wrap_columns(shift)
    step, m, L, h2 = WRAP["step"], WRAP["m"], WRAP["mean_length"], WRAP["h2"]
    assert len(s) == 4_015 and s.min() >= 0 and e.max() == TOP and (e - s).max() == LONG > 2_047  # (the wide columns)
    n_bins = -(-TOP // step)
    c, i = bin_tracks(s, e, q, TOP, step, L)
    assert len(i) == n_bins == 262_144
    long_bins = ((s + e) >> 1)[e - s == LONG] // step
    assert len(long_bins) == 12 and np.all(np.diff(long_bins) == 13)
    tiles = sorted(set((long_bins // T).tolist()))
    assert tiles == [31, 32]  # on either side of a tile bound
    if shift == 50 * 4096:
        assert (long_bins // T == 31).sum() == 6  # six on either side of the bound
    # the prefix a tile scans: the sum of i over the bins it counts, inside [k0 - HALO, k0 + T + HALO)
    scanned = {}
    for t in tiles:
        lo, hi = tile_reads(t * T, T, m, h2)
        assert t * T - HALO <= lo and hi <= t * T + T + HALO
        scanned[t] = int(i[lo:hi].sum())
    print("prefix / 2^32:", {t: round(v / TWO32, 3) for t, v in scanned.items()})
    if shift == 0:
        assert max(scanned.values()) >= 2 * TWO32  # tile 31 passes 2^32 twice and more
    else:
        assert min(scanned.values()) >= TWO32  # both tiles of the midpoints wrap
    # the tiles of the cut intervals start and end elsewhere: in each interval a tile wraps as well
    for a, b in zip(*wrap_intervals(shift)[1]):
        k_lo, k_hi = interval_windows(a, b, TOP, step, m)
        sums = [int(i[max(lo, 0):hi].sum()) for lo, hi in (tile_reads(k0, min(k_hi + 1 - k0, T), m, h2) for k0 in range(k_lo, k_hi + 1, T))]
        print("interval", a, b, "prefix / 2^32:", round(max(sums) / TWO32, 3))
        assert max(sums) >= TWO32, (a, b)
    I = window_sums(i, m)
    B2, _ = backgrounds(i, m, h2)
    print("largest B / 2^32:", B2.max() / TWO32, "largest I / 2^32:", I.max() / TWO32)
    assert B2.max() < TWO32 and I.max() < TWO32 and B2.max() > 0.7 * TWO32
    win, hot, stats = ifs_hotspots_ref(s, e, q, [0], [TOP], TOP, thresholds=flat_table(1, 4096), tracks=(c, i), **WRAP)
    print("called", len(win), "tested", stats[0, TESTED], "bg2 > 2^31:", (win["bg2"] > 1 << 31).sum())
    assert len(win) >= 1 and (win["bg2"] > 1 << 31).any() and stats[0, TESTED] > stats[0, CALLED] == len(win)
    assert win["pos"].max() > TOP - 5 * step and len(hot) >= 2
    N, S = totals_ref(s, e, q, TOP)
    assert N == len(s) and S > 1 << 33


@gpu
@pytest.mark.parametrize("shift", LAYOUTS)
def test_wrapped_prefix_sums(engine, shift):
    kw = dict(WRAP, thresholds=flat_table(1, 4096))
    with Contig(engine, *wrap_columns(shift)) as c:
        assert not engine.frags_packed(c.name)
        assert engine.ifs_totals(c.name, TOP) == totals_ref(*c.cols, TOP)
        tracks = bin_tracks(*c.cols, TOP, WRAP["step"], WRAP["mean_length"])
        for starts, stops in wrap_intervals(shift):
            win, _, _ = c.both(starts, stops, TOP, (shift, len(starts)), tracks, **kw)
            assert (win["bg2"] > 1 << 31).any()
            c.track(starts, stops, TOP, (shift, len(starts)), step=WRAP["step"], m=WRAP["m"], mean_length=WRAP["mean_length"])


# ---- B. coordinates next to 2^30 ------------------------------------------------------------------------------------------
ROOM = 700  # bases in front of the first fragment that the region interval takes in
SMALL = {  # step: (m, the two pairs of half-widths with their min_count)
    20: (10, ((125, 250, 1), (REACH - 10, 0, 0))),
    1: (1, ((3, 0, 0), (125, 250, 1))),
}


def small_shift(s):
    return ((SHIFT - (REACH + 64) * s) // s) * s


def small_intervals():
    """On ``top``: the region with ROOM in front, and two inner intervals that end on TOP and on TOP - 1."""
    return np.array([TOP - SPAN - ROOM, TOP - 50_000, TOP - 20_001], np.int64), np.array([TOP, TOP, TOP - 1], np.int64)


@functools.lru_cache(maxsize=None)
def small_case(s):
    """What the cases of step ``s`` share: (top columns, low columns, the low twin's shift and size, mean length, table)."""
    from finaletoolkit_amd import utils
    top = twin_columns()[:3]
    down = small_shift(s)
    low = frozen(top[0] - down, top[1] - down) + (top[2],)
    m, L = SMALL[s][0], 167
    size = TOP - down
    if s == 20:
        thr = utils.ifs_thresholds(0.01, 256)
    else:
        N, S = totals_ref(*low, size)
        thr = flat_table(max(global_mean_ref(N, S, L, m, size, s), 1), 4)
    return top, low, down, size, L, thr


@functools.lru_cache(maxsize=None)
def small_wanted(s, h1, h2, min_count):
    """The low twin's restatement over the three intervals."""
    _, low, down, size, L, thr = small_case(s)
    starts, stops = small_intervals()
    return ifs_hotspots_ref(*low, starts - down, stops - down, size, step=s, m=SMALL[s][0], mean_length=L, h1=h1, h2=h2,
                            min_count=min_count, thresholds=thr, join=SMALL[s][0])


def moved_up(res, down):
    win, hot, stats = (x.copy() for x in res)
    win["pos"] += down
    for f in ("start", "stop", "summit"):
        hot[f] += down
    return win, hot, stats


@pytest.mark.parametrize("s", sorted(SMALL))
def test_small_steps_from_the_data(s):
    """Measured (called of tested windows in the region interval): step 20, (125, 250) with min_count 1: 298 of 46 761;
    (1014, 0): 1 025 of 150 026; step 1, (3, 0): 49 275 of 3 000 700; (125, 250) with min_count 1: 7 824 of 12 227."""
    top, low, down, size, L, thr = small_case(s)
    m = SMALL[s][0]
    assert down % s == 0 and 0 < down and len(top[0]) == 30_054
    first_bin = int(((low[0] + low[1]) >> 1).min()) // s
    assert first_bin > REACH + m and low[0].min() >= 0  # no compared window's background is clipped at bin 0
    starts, stops = small_intervals()
    assert (starts - down).min() >= 0 and stops.max() == TOP
    for h1, h2, min_count in SMALL[s][1]:
        win, hot, stats = small_wanted(s, h1, h2, min_count)
        print(s, h1, h2, "called", stats[:, CALLED].tolist(), "tested", stats[:, TESTED].tolist())
        region = win[win["run"] == 0]
        full1, full2 = 2 * h1 + m, (2 * h2 + m if h2 else 0)
        near = region["pos"] + down >= TOP - (m + max(h1, h2)) * s
        assert near.any() and ((region["nb1"][near] < full1) | (region["nb2"][near] < full2)).any()  # a clipped n_b among the calls
        assert not ((region["nb1"][~near] < full1) | (region["nb2"][~near] < full2)).any()       # and none clipped at bin 0
        assert stats[0, TESTED] > stats[0, CALLED] == len(region) and len(hot) >= 1


@gpu
@pytest.mark.parametrize("s", sorted(SMALL))
def test_small_steps_next_to_the_top(engine, s):
    """The low twin against its restatement, the top twin against the low twin moved up."""
    top, low, down, size, L, thr = small_case(s)
    m = SMALL[s][0]
    starts, stops = small_intervals()
    for key, cols, dn, sz in (("low", low, down, size), ("top", top, 0, TOP)):
        with Contig(engine, *cols, name="ifs:" + key) as c:
            for h1, h2, min_count in SMALL[s][1]:
                want = small_wanted(s, h1, h2, min_count)
                got = engine.ifs_hotspots(c.name, starts - dn, stops - dn, sz, step=s, m=m, mean_length=L, h1=h1, h2=h2,
                                          min_count=min_count, thresholds=thr, join=m)
                assert_same(got, moved_up(want, down - dn), (key, s, h1, h2))
            ends = (TOP - 90_000, TOP - 3 * T * s - 7, TOP - 9)
            t_starts, t_stops = np.array(ends, np.int64) - dn, np.array([TOP, TOP - 1, TOP], np.int64) - dn
            if key == "low":
                track = c.track(t_starts, t_stops, sz, (key, s), step=s, m=m, mean_length=L)
                totals = [totals_ref(*cols, sz - d) for d in (0, 1)]
                assert totals[0][0] == totals[1][0] + 1  # (the midpoint on TOP - 1)
            else:
                n, ifs, offs = engine.ifs_track(c.name, t_starts, t_stops, sz, step=s, m=m, mean_length=L)
                assert all(np.array_equal(a, b) for a, b in zip((n, ifs, offs), track))
                dn_, di_, _ = engine.ifs_track(c.name, t_starts, t_stops, sz, step=s, m=m, mean_length=L, device=True)
                assert np.array_equal(dn_.cpu().numpy(), track[0]) and np.array_equal(di_.cpu().numpy(), track[1])
            assert [engine.ifs_totals(c.name, sz - d) for d in (0, 1)] == totals


@gpu
def test_the_whole_contig_is_one_interval(engine):
    """``[0, TOP)`` at step 20: 13 108 tiles in four batches, nearly all of them without a fragment.  The called windows and
    the hotspots are the region interval's, which the test above holds against the restatement.  (Not run at step 1:
    2^18 tiles, whose restatement-free answer says no more than this one's.)"""
    s = 20
    top, _, _, _, L, thr = small_case(s)
    m, (h1, h2, min_count) = SMALL[s][0], SMALL[s][1][0]
    n_bins = -(-TOP // s)
    assert -(-(n_bins - m + 1) // T) == 13_108 and 3 * BATCH < 13_108 <= 4 * BATCH and min_count == 1
    kw = dict(step=s, m=m, mean_length=L, h1=h1, h2=h2, min_count=min_count, thresholds=thr, join=m)
    with Contig(engine, *top) as c:
        region = engine.ifs_hotspots(c.name, [TOP - SPAN - ROOM], [TOP], TOP, **kw)
        whole = engine.ifs_hotspots(c.name, [0], [TOP], TOP, **kw)
    assert same_records(whole[0], region[0]) and same_records(whole[1], region[1]) and len(region[0]) >= 10
    assert whole[2][0, 1:].tolist() == region[2][0, 1:].tolist() and whole[2][0, WINDOWS] == n_bins - m + 1
    want = moved_up(small_wanted(s, h1, h2, min_count), small_shift(s))
    assert same_records(region[0], want[0][want[0]["run"] == 0]) and np.array_equal(region[2][0], want[2][0])


LARGE_STEPS = (1000, 65534, 65535)
LARGE_SHAPES = ((1, 1, 0), (64, 1, 0), (64, 100, 960), (1, REACH - 1, 0))  # m, h1, h2


@functools.lru_cache(maxsize=None)
def large_columns():
    """The twin columns (about 46 bins of 65535 bases) and 2 000 fragments of 50-400 bases over the whole contig."""
    rng = np.random.default_rng(65535)
    top = twin_columns()[:3]
    a = rng.integers(0, TOP - 400, 2_000)
    ln = rng.integers(50, 401, len(a))
    s, e, q = np.concatenate([top[0], a]), np.concatenate([top[1], a + ln]), np.concatenate([top[2], np.full(len(a), 60)])
    o = np.argsort(s, kind="stable")
    return frozen(s[o], e[o], q[o])


@functools.lru_cache(maxsize=None)
def large_tracks(s):
    return bin_tracks(*large_columns(), TOP, s, 167)


def large_table(s, m):
    """Flat at half the mean IFS of the bins that hold a midpoint, per window of ``m`` bins: the contig's own mean is
    next to nothing at these steps (most bins are empty), so every occupied window would pass it; this one is passed where
    the twin columns lie and missed where a lone fragment does."""
    c, i = large_tracks(s)
    return flat_table(max(int(i.sum()) * m * 1024 // (2 * int((c > 0).sum()) * 167), 1), 4096)


@pytest.mark.parametrize("s", LARGE_STEPS)
def test_large_steps_from_the_data(s):
    """Measured, called of tested windows over ``[0, TOP)`` for the four shapes: step 1000: 1 579 of 4 457, 2 415 and 2 113 of
    123 829, 1 815 of 4 457; step 65534: 45 of 1 918, 13 and 105 of 16 316, 142 of 1 918; step 65535: 46 of 1 925, 13 and 105
    of 16 316, 142 of 1 925."""
    cols = large_columns()
    c, i = large_tracks(s)
    n_bins = -(-TOP // s)
    assert len(cols[0]) == 32_054 and len(c) == n_bins and TOP % s != 0  # a short last bin
    if s >= 65534:
        assert n_bins == 16_385 and all(c[t * T:(t + 1) * T].sum() > 0 for t in range(5))  # every tile of m = 1 holds data
        assert (c > 0).sum() > 1_000 and c[-1] > 0
    for m, h1, h2 in LARGE_SHAPES:
        win, hot, stats = ifs_hotspots_ref(*cols, [0, 0], [TOP, TOP - 1], TOP, step=s, m=m, mean_length=167, h1=h1, h2=h2, min_count=1,
                                           thresholds=large_table(s, m), join=m, tracks=(c, i))
        print(s, m, h1, h2, "called", stats[:, CALLED].tolist(), "tested", stats[:, TESTED].tolist())
        assert stats[0, WINDOWS] == n_bins - m + 1 == stats[1, WINDOWS] + 1  # [0, TOP - 1) loses the last window
        assert stats[0, TESTED] > stats[0, CALLED] >= 1
        assert stats[0, CALLED] - stats[1, CALLED] == (win[win["run"] == 0]["pos"] == (n_bins - m) * s).sum()


@gpu
@pytest.mark.parametrize("s", LARGE_STEPS)
def test_large_steps_at_the_top(engine, s):
    with Contig(engine, *large_columns()) as c:
        for m, h1, h2 in LARGE_SHAPES:
            c.both([0, 0], [TOP, TOP - 1], TOP, (s, m, h1, h2), large_tracks(s), step=s, m=m, mean_length=167, h1=h1, h2=h2, min_count=1,
                   thresholds=large_table(s, m), join=m)
        for m in (1, 64):
            c.track([0, 0, TOP - 3 * s], [TOP, TOP - 1, TOP], TOP, (s, m), step=s, m=m, mean_length=167)
        assert [engine.ifs_totals(c.name, TOP - d) for d in (0, 1)] == [totals_ref(*c.cols, TOP - d) for d in (0, 1)]


# ---- C. both sides of the halo switch -------------------------------------------------------------------------------------
HALO_STEP, HALO_BINS = 7, 3 * T + 5
HALO_SIZE = HALO_BINS * HALO_STEP - HALO_STEP // 3
HALO_MS = (1, 10, 64)


def halo_halves(m):
    return ((125, HALO - m), (125, HALO + 1 - m), (HALO - m, 0), (HALO + 1 - m, 0))


def halo_outermost(m, h):
    """The outermost background bins of the last window of a tile and of the first window of the next, at both inner
    tile bounds."""
    return [b for k0 in (T, 2 * T) for b in (k0 - 1 - h, k0 - h, k0 + m - 2 + h, k0 + m - 1 + h)]


@functools.lru_cache(maxsize=None)
def halo_columns():
    """Depth 30 at random, and a fragment of 10 bases with its midpoint in each of the outermost bins."""
    s, e, q = random_fragments(np.random.default_rng(512), HALO_SIZE, 30)
    bins = sorted({b for m in HALO_MS for h1, h2 in halo_halves(m) for b in halo_outermost(m, max(h1, h2))})
    ps, pe = at(np.array(bins, np.int64) * HALO_STEP + 3)
    s, e, q = np.concatenate([s, ps]), np.concatenate([e, pe]), np.concatenate([q, np.full(len(ps), 60)])
    o = np.argsort(s, kind="stable")
    return frozen(s[o].astype(np.int64), e[o].astype(np.int64), q[o].astype(np.int64))


def halo_table(m):
    N, S = totals_ref(*halo_columns(), HALO_SIZE)
    return flat_table(max(global_mean_ref(N, S, 167, m, HALO_SIZE, HALO_STEP), 1), 4096)


def test_halo_switch_from_the_data():
    """Measured, called windows for the four pairs of half-widths (all 12 294 - m windows are tested): m = 1: 4 258, 4 256,
    6 670, 6 661; m = 10: 4 206, 4 208, 6 546, 6 568; m = 64: 4 406, 4 412, 6 323, 6 332."""
    cols = halo_columns()
    assert len(cols[0]) <= 35_000 and -(-HALO_SIZE // HALO_STEP) == HALO_BINS
    c, i = bin_tracks(*cols, HALO_SIZE, HALO_STEP, 167)
    for m in HALO_MS:
        for h1, h2 in halo_halves(m):
            h = max(h1, h2)
            assert h + m in (HALO, HALO + 1) and all(i[b] > 0 for b in halo_outermost(m, h)) and h <= REACH - m
            win, _, stats = ifs_hotspots_ref(*cols, [0], [HALO_SIZE], HALO_SIZE, step=HALO_STEP, m=m, mean_length=167, h1=h1, h2=h2,
                                             thresholds=halo_table(m), tracks=(c, i))
            print(m, h1, h2, "called", stats[0, CALLED], "tested", stats[0, TESTED])
            assert stats[0, TESTED] > stats[0, CALLED] >= 1
            # calls among the windows next to the tile bounds, whose backgrounds end in those bins
            assert np.isin(win["pos"] // HALO_STEP, [T - 1, T, 2 * T - 1, 2 * T]).any()


@gpu
@pytest.mark.parametrize("m", HALO_MS)
def test_both_sides_of_the_halo_switch(engine, m):
    with Contig(engine, *halo_columns()) as c:
        tracks = bin_tracks(*c.cols, HALO_SIZE, HALO_STEP, 167)
        for h1, h2 in halo_halves(m):
            for starts, stops in (([0], [HALO_SIZE]), ([0, (T - 9) * HALO_STEP], [(2 * T + m) * HALO_STEP, HALO_SIZE])):
                c.both(starts, stops, HALO_SIZE, (m, h1, h2), tracks, step=HALO_STEP, m=m, mean_length=167, h1=h1, h2=h2,
                       thresholds=halo_table(m))


# ---- D. the widest axes, by hand ------------------------------------------------------------------------------------------
@gpu
def test_join_at_its_limit(engine):
    """Called windows exactly FTK_IFS_MAX_JOIN and one more apart, across a tile bound."""
    size = 2 * T
    kw = dict(step=1, m=1, mean_length=10, h1=3, h2=0, thresholds=flat_table(1, 64), min_count=1)
    for gap, hotspots, bases in ((MAX_JOIN, [(T - 500, T + 525, 2)], 1025), (MAX_JOIN + 1, [(T - 500, T - 499, 1), (T + 525, T + 526, 1)], 2)):
        with Contig(engine, *columns(at([T - 500, T - 500 + gap]))) as c:
            win, hot, stats = c.both([0], [size], size, gap, join=MAX_JOIN, **kw)
            assert win["pos"].tolist() == [T - 500, T - 500 + gap] and hot[["start", "stop", "n_windows"]].tolist() == hotspots
            assert stats.tolist() == [[size, 2, 2, len(hotspots), 0, bases]] and stats[0, KEPT] == len(hotspots) and stats[0, BASES] == bases
            _, hot, _ = c.both([0], [size], size, gap, join=MAX_JOIN - 1, **kw)
            assert len(hot) == 2
            with pytest.raises(FtkError):
                engine.ifs_hotspots(c.name, [0], [size], size, join=MAX_JOIN + 1, **kw)


@gpu
def test_the_table_s_last_entry_at_its_limit(engine):
    """With L = 1 a lone fragment of l bases gives q = l + 1: 4 094 bases read thr[4095], the last entry of the largest
    table; 4 095 bases lie beyond it."""
    size = 3 * T
    kw = dict(step=1, m=1, mean_length=1, h1=3, h2=0, min_count=1, join=1)
    a, b = 3_000, 9_000  # the midpoints
    last = np.zeros(MAX_THR, np.uint64)
    last[MAX_THR - 1] = 1
    with Contig(engine, *columns((a - 2_047, a + 2_047), (b - 2_047, b + 2_048))) as c:
        assert (c.cols[1] - c.cols[0]).tolist() == [4_094, 4_095]
        n, ifs, _ = c.track([a, b], [a + 1, b + 1], size, step=1, m=1, mean_length=1)
        assert n.tolist() == [1, 1] and ifs.tolist() == [MAX_THR - 1, MAX_THR]
        win, _, stats = c.both([0], [size], size, thresholds=last, **kw)
        assert win.tolist() == [(0, a, 1, 4_095, 4_095, 7, 0, 0)] and stats.tolist() == [[size, 2, 1, 1, 0, 1]]
        # that entry alone 0, a table one entry short, and the largest value an entry takes: 4095 * 1024 < (2^32 - 1) * 7
        for thr in (1 - last, np.ones(MAX_THR - 1, np.uint64), last * np.uint64(TWO32 - 1)):
            assert c.both([0], [size], size, thresholds=thr, **kw)[2].tolist() == [[size, 2, 0, 0, 0, 0]]
        # on equality: B m 2^10 >= t n_b L  <=>  4095 * 1024 >= 7 t  <=>  t <= 599 040
        for t, called in ((599_040, 1), (599_041, 0)):
            assert c.both([0], [size], size, thresholds=last * np.uint64(t), **kw)[2][0, CALLED] == called
