"""GPU: the preferred-end kernels (csrc/ftk_prefends.hip) against the numpy restatement of the rule in
``tests/prefends_helpers.py`` - equal integers, call for call and counter for counter - on random fragments, on cases
built by hand around the tile bounds, the contig ends and the table's edges, on both column forms, on intervals cut every
way, on the refusals of the C call, and through ``utils.frag_preferred_ends`` and its command line."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import write_synthetic_bam
from tests.prefends_helpers import (CALL_DTYPE, CALLS_A, CALLS_B, TESTED_A, TESTED_B, flat_table, preferred_ends_ref,
                                    random_fragments, same_calls)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tile():
    from finaletoolkit_amd import _lib as L
    return L.PREFENDS_TILE


def assert_same(got, want, what=None):
    assert np.array_equal(got[1], want[1]), (what, got[1].tolist(), want[1].tolist())
    assert got[0].dtype == CALL_DTYPE and same_calls(got[0], want[0]), (what, len(got[0]), len(want[0]))


class Contig:
    """A contig of the engine's for the length of a ``with`` block."""

    def __init__(self, engine, start, end, mapq, read1=False, name="pe:case"):
        order = np.argsort(np.asarray(start), kind="stable")
        self.cols = tuple(np.asarray(c)[order] for c in (start, end, mapq))
        self.engine, self.name, self.read1 = engine, name, read1

    def __enter__(self):
        s, e, q = self.cols
        strand = np.zeros(len(s), np.uint8)
        if self.read1:  # forward fragments: read1 is the first 50 bases
            self.engine.load_contig(self.name, s, e, q, strand, s, np.minimum(s + 50, e))
        else:
            self.engine.load_contig(self.name, s, e, q, strand)
        return self

    def __exit__(self, *exc):
        self.engine.release(self.name)

    def both(self, starts, stops, size, what=None, **kw):
        """The engine's answer, held against the restatement's."""
        starts, stops = np.asarray(starts, np.int64), np.asarray(stops, np.int64)
        got = self.engine.preferred_ends(self.name, starts, stops, size, **kw)
        assert_same(got, preferred_ends_ref(*self.cols, starts, stops, size, **kw), what)
        return got


def points(positions, copies=1):
    """Fragments one base long: both ends of each on its position."""
    p = np.repeat(np.asarray(positions, np.int64), copies)
    return p, p + 1


def columns(*pairs):
    s = np.concatenate([np.atleast_1d(np.asarray(a, np.int64)) for a, _ in pairs])
    e = np.concatenate([np.atleast_1d(np.asarray(b, np.int64)) for _, b in pairs])
    return s, e, np.full(len(s), 60, np.int64)


# ---- 1. the rule on random fragments --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["combined", "split"])
@pytest.mark.parametrize("h", [1, 7, 500, 2048])
def test_rule_against_the_restatement(engine, h, mode):
    """Every contig size x depth x min_count, with the Poisson table of alpha = 0.01.  The case is held not to be vacuous - a
    call, and a tested position that is not called - where the windows are wide enough for the table to tell the two apart
    (h = 500 and 2048), at depth 30 with min_count up to 2 on contigs of a tile and more: there about 0.6 % of the positions
    are called and most positions with two ends are not.  (With h = 1 or 7 a position's own ends are most of its window:
    the table calls next to nothing, and the restatement says the same.)"""
    from finaletoolkit_amd import utils
    T = tile()
    thr = utils.preferred_end_thresholds(0.01)
    for k, size in enumerate([1, 2 * h, 2 * h + 1, T - 1, T, T + 1, 3 * T + 5]):
        for depth in (2, 30):
            rng = np.random.default_rng(1000 * h + 10 * k + depth)
            with Contig(engine, *random_fragments(rng, size, depth)) as c:
                for min_count in (1, 2, 3):
                    what = (size, depth, min_count)
                    calls, stats = c.both([0], [size], size, what, half=h, mode=mode, min_count=min_count, thresholds=thr)
                    if size >= T and depth == 30 and min_count <= 2 and h >= 500:
                        n_called, n_tested = stats[0, CALLS_A] + stats[0, CALLS_B], stats[0, TESTED_A] + stats[0, TESTED_B]
                        assert len(calls) >= 1 and n_called == len(calls) and n_tested > n_called, what


# ---- 2. cases built by hand -----------------------------------------------------------------------------------------------
def test_exact_cases(engine):
    T = tile()
    size, h = 3 * T + 5, 7
    one = flat_table(1)  # called iff T <= n_w
    kw = dict(half=h, thresholds=one)
    # seven fragments of one base on p (e = 14) and one U end three bases on: T = 15 = n_w, called on equality;
    # on q the same and one more U end: T = 16, tested and not called.  The lone ends have e = 1: not tested.
    p, q = 1_000, 2_000
    with Contig(engine, *columns(points([p, q], 7), (p + 3, p + 103), (q + 3, q + 103), (q + 4, q + 104))) as c:
        calls, stats = c.both([0], [size], size, **kw)
        assert calls.tolist() == [(0, p, 2, 14, 15, 15)] and stats.tolist() == [[17, 17, 2, 0, 1, 0]]
    # the same at a window clipped at base 0 (position 2: [0, 9], n_w = 10) and at the last base (size - 3: n_w = 10)
    a, z = 2, size - 3
    with Contig(engine, *columns(points([a, z], 5))) as c:
        calls, _ = c.both([0], [size], size, **kw)
        assert calls.tolist() == [(0, a, 2, 10, 10, 10), (0, z, 2, 10, 10, 10)]
    with Contig(engine, *columns(points([a, z], 5), (a + 3, a + 103), (z - 102, z - 1))) as c:  # + a U end on 5, a D end on size - 5
        calls, stats = c.both([0], [size], size, **kw)
        assert len(calls) == 0 and stats[0, TESTED_A] == 2
    # called positions on either side of a tile bound, two tiles apart as well
    around = [T - 1, T, T + 1, 2 * T - 1, 2 * T, 3 * T, 3 * T + 4]
    with Contig(engine, *columns(points(around, 2))) as c:
        calls, _ = c.both([0], [size], size, **kw)
        assert calls["pos"].tolist() == around and calls["count"].tolist() == [4] * 7
        assert calls["total"].tolist() == [12, 12, 12, 8, 8, 8, 8] and calls["n_w"].tolist() == [15] * 5 + [12, 8]
    # a window whose ends lie in two tiles: position T - 3 sees [T - 10, T + 4], a D end on its first base and a U end on its last
    with Contig(engine, *columns(points([T - 3], 2), (T - 200, T - 9), (T + 4, T + 150), (T - 211, T - 10), (T + 5, T + 160))) as c:
        calls, _ = c.both([0], [size], size, **kw)
        assert calls.tolist() == [(0, T - 3, 2, 4, 6, 15)]  # (the ends on T - 11 and T + 5 are outside)
        # ... and whichever tile the position is in, the interval starting on it or ending behind it
        calls, _ = c.both([T - 3, 0, T - 2], [T + 9, T - 2, T + 9], size, **kw)
        assert calls.tolist() == [(0, T - 3, 2, 4, 6, 15), (1, T - 3, 2, 4, 6, 15)]
    # e >= n_thr reads the last entry; an entry of 0 never calls
    with Contig(engine, *columns(points([500], 5), points([900], 1))) as c:
        last = np.array([0, 0, 0, 1 << 20], np.uint64)
        calls, _ = c.both([0], [size], size, half=h, thresholds=last)
        assert calls.tolist() == [(0, 500, 2, 10, 10, 15)]  # e = 2 on 900 reads thr[2] = 0
        calls, stats = c.both([0], [size], size, half=h, thresholds=np.array([0, 1 << 20, 1 << 20, 0], np.uint64))
        assert calls.tolist() == [(0, 900, 2, 2, 2, 15)] and stats[0, TESTED_A] == 2
        calls, stats = c.both([0], [size], size, half=h, thresholds=np.zeros(2, np.uint64), min_count=1)
        assert len(calls) == 0 and stats.tolist() == [[6, 6, 2, 0, 0, 0]]
        top = np.full(4096, (1 << 40) - 1, np.uint64)  # the largest table there is: everything tested is called
        calls, _ = c.both([0], [size], size, half=2048, thresholds=top, min_count=1)
        assert calls["pos"].tolist() == [500, 900] and calls["total"].tolist() == [12, 12] and calls["n_w"].tolist() == [2549, 2949]


def test_ends(engine):
    T = tile()
    size = 3 * T + 5
    every = dict(half=7, min_count=1, thresholds=flat_table(1 << 19), mode="split")  # every position with an end is called
    # a D end on end - 1 when end is exactly a tile's first base, and a U end on that base
    with Contig(engine, *columns((T - 50, T), (T, T + 60))) as c:
        calls, stats = c.both([0, T, 0], [T, 2 * T, size], size, **every)
        assert [r[:3] for r in calls.tolist()] == [(0, T - 50, 0), (0, T - 1, 1), (1, T, 0), (1, T + 59, 1),
                                                   (2, T - 50, 0), (2, T - 1, 1), (2, T, 0), (2, T + 59, 1)]
        assert stats[:, :2].tolist() == [[1, 1], [1, 1], [2, 2]]
    # a fragment reaching beyond the contig: its U end counts, its D end does not exist; fragments without a base are none
    with Contig(engine, *columns((size - 10, size + 50), (100, 100), (size - 1, size - 1), (200, 201), (size - 1, size))) as c:
        calls, stats = c.both([0], [size], size, **every)
        assert [r[1:3] for r in calls.tolist()] == [(200, 0), (200, 1), (size - 10, 0), (size - 1, 0), (size - 1, 1)]
        assert stats[0, :2].tolist() == [3, 2]
    # 70 000 copies of one fragment: counts above 65 535 are exact, in either mode and either halo
    with Contig(engine, *columns((np.full(70_000, 300), np.full(70_000, 467)), (310, 480))) as c:
        for h in (7, 500, 2048):
            calls, _ = c.both([0], [size], size, **dict(every, half=h))
            assert (0, 300, 0, 70_000) in [r[:4] for r in calls.tolist()] and (0, 466, 1, 70_000) in [r[:4] for r in calls.tolist()]
            calls, _ = c.both([0], [size], size, **dict(every, half=h, mode="combined"))
            assert calls["count"].max() == 70_000 and calls["total"].max() == (140_002 if h >= 179 else 70_000)
    # mapq and length on either side of each bound
    s, e, q = columns((100, 110), (200, 211), (300, 312), (400, 411), (500, 511))
    q[:] = [30, 30, 30, 29, 31]
    with Contig(engine, s, e, q) as c:
        calls, _ = c.both([0], [size], size, min_length=11, max_length=11, quality_threshold=30, **every)
        assert calls["pos"].tolist() == [200, 210, 500, 510]
        calls, _ = c.both([0], [size], size, min_length=10, max_length=12, quality_threshold=31, **every)
        assert calls["pos"].tolist() == [500, 510]
        calls, _ = c.both([0], [size], size, min_length=12, quality_threshold=0, **every)
        assert calls["pos"].tolist() == [300, 311]
        calls, _ = c.both([0], [size], size, max_length=10, quality_threshold=29, **every)
        assert calls["pos"].tolist() == [100, 109]


def test_a_long_fragment_reaches_the_tile_by_its_d_end_alone(engine):
    """A contig of 120 000 bases (the candidates of a tile reach back by the longest admissible fragment, 100 000 here)."""
    size = 120_000
    every = dict(half=500, min_count=1, thresholds=flat_table(1 << 19), mode="split")
    with Contig(engine, *columns((5, 100_005), (40_000, 40_150), (99_000, 99_170), (100_900, 101_000))) as c:
        calls, stats = c.both([100_000, 0], [100_100, size], size, **every)
        assert [r[:3] for r in calls.tolist()][0] == (0, 100_004, 1) and stats[0].tolist() == [0, 1, 0, 1, 0, 1]
        assert calls[0]["total"] == 1 and len(calls) == 1 + 8  # (the D end on 99 169 is 835 bases away)
        calls, stats = c.both([100_000], [100_100], size, max_length=1_000, **every)  # filtered out: not a candidate either
        assert len(calls) == 0 and np.all(stats == 0)
        calls, _ = c.both([100_000], [100_100], size, **dict(every, mode="combined", half=2048))
        assert calls.tolist() == [(0, 100_004, 2, 1, 5, 4097)]  # + the ends on 99 000, 99 169, 100 900 and 100 999


# ---- 3. the columns -------------------------------------------------------------------------------------------------------
def test_packed_and_wide_columns_give_the_same_calls(engine):
    from finaletoolkit_amd import utils
    T = tile()
    size = 3 * T + 5
    rng = np.random.default_rng(77)
    s, e, q = random_fragments(rng, size, 30)
    q[::5] = 31  # saturated in the packed word
    thr = utils.preferred_end_thresholds(0.01)
    starts, stops = [0, T - 9], [size, 2 * T + 9]
    answers = []
    for long_one, read1 in ((False, False), (True, False), (False, True)):
        s2, e2, q2 = (np.append(s, 700), np.append(e, 700 + 2_047), np.append(q, 60)) if long_one else (s, e, q)
        with Contig(engine, s2, e2, q2, read1=read1) as c:
            assert engine.frags_packed(c.name) == (not long_one and not read1)
            got = [c.both(starts, stops, size, half=h, mode=mode, thresholds=thr, max_length=max_length, quality_threshold=cut)
                   for h, mode in ((500, "combined"), (2048, "split"))
                   # (a cut above 31 or an upper bound of 2047 and more keep the wide columns on a packed contig, too)
                   for max_length, cut in ((None, 30), (1_000, 31), (None, 32), (2_047, 30))]
            if not long_one:
                answers.append(got)
    for a, b in zip(*answers):  # a BAM-style contig with read1 columns gives the same calls
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and len(a[0]) > 10


# ---- 4. intervals ---------------------------------------------------------------------------------------------------------
def test_intervals(engine):
    from finaletoolkit_amd import utils
    T = tile()
    size = 3 * T + 5
    rng = np.random.default_rng(5)
    thr = utils.preferred_end_thresholds(0.01)
    with Contig(engine, *random_fragments(rng, size, 30)) as c:
        for mode in ("combined", "split"):
            kw = dict(half=500, mode=mode, thresholds=thr)
            whole, whole_stats = c.both([0], [size], size, **kw)
            assert len(whole) > 30
            # unordered, overlapping, touching and empty intervals: each is the whole contig's calls filtered to it
            starts = np.array([2 * T, 0, 100, T - 1, 700, 700, size, 5_000, 3 * T], np.int64)
            stops = np.array([size, T, 100, T + 1, 9_000, 9_000, size, 5_001, 3 * T + 5], np.int64)
            calls, stats = c.both(starts, stops, size, **kw)
            for r, (a, b) in enumerate(zip(starts, stops)):
                mine, want = calls[calls["run"] == r], whole[(whole["pos"] >= a) & (whole["pos"] < b)]
                assert mine[["pos", "kind", "count", "total", "n_w"]].tolist() == want[["pos", "kind", "count", "total", "n_w"]].tolist()
            assert np.all(stats[2] == 0) and np.all(stats[6] == 0) and np.array_equal(stats[4], stats[5])
            # a contig called whole equals the concatenation of any split of it
            for cuts in ([0, 1, T - 3, T, 2 * T + 1, size - 1, size], list(range(0, size, 1_000)) + [size]):
                parts, part_stats = c.both(cuts[:-1], cuts[1:], size, **kw)
                assert parts[["pos", "kind", "count", "total", "n_w"]].tolist() == whole[["pos", "kind", "count", "total", "n_w"]].tolist()
                assert np.array_equal(part_stats.sum(axis=0), whole_stats[0])
            # two calls in a row return the same bytes
            again, again_stats = engine.preferred_ends(c.name, starts, stops, size, **kw)
            assert again.tobytes() == calls.tobytes() and again_stats.tobytes() == stats.tobytes()
        none, none_stats = engine.preferred_ends(c.name, [], [], size, thresholds=thr)
        assert len(none) == 0 and none_stats.shape == (0, 6)
    with Contig(engine, np.zeros(0), np.zeros(0), np.zeros(0)) as c:  # an empty contig, and one without a base
        calls, stats = c.both([0, 10], [size, 10], size, thresholds=thr)
        assert len(calls) == 0 and np.all(stats == 0)
        calls, stats = c.both([0], [0], 0, thresholds=thr)
        assert len(calls) == 0 and np.all(stats == 0)


def test_more_tiles_than_a_batch_and_a_growing_scratch(engine):
    """The call walks its tiles in batches of ``BATCH`` (kCallBatchTiles): ``BATCH + 5`` intervals of one base are as many
    tiles, so the calls come home in two pieces and the counters of both reach their rows.  Then a context of its own, whose
    scratch is no larger than the plan of a batch: three copies of the whole contig at depth 200 give more calls than the
    plan's block has room for, so the scratch has to grow between the passes (where an idle block of an earlier context is
    handed out, it may not have to - the answer is the same)."""
    from finaletoolkit_amd import _lib as L
    from finaletoolkit_amd.engine import Engine
    BATCH = L.PREFENDS_BATCH_TILES
    T = tile()
    size = 3 * T + 5
    every = dict(half=500, min_count=1, thresholds=flat_table(1 << 19), mode="split")
    cols = random_fragments(np.random.default_rng(8), size, 200)
    with Contig(engine, *cols) as c:
        starts = np.arange(3_000, 3_000 + BATCH + 5, dtype=np.int64)
        calls, stats = c.both(starts, starts + 1, size, **every)
        assert len(calls) > BATCH and calls["run"][0] < BATCH <= calls["run"][-1] and stats[BATCH:, :2].sum() > 0
    with Engine(0) as own:
        with Contig(own, *cols) as c:
            calls, stats = c.both([0, 0, 0], [size, size, size], size, **every)
            assert len(calls) * 32 > 1 << 20 and np.array_equal(stats[0], stats[2])


def test_a_window_crosses_the_batch_boundary(engine):
    """One interval of more tiles than a batch holds: the positions on either side of the last tile bound of the first batch
    are tested against windows that read the ends on the far side of it, and the calls come home in two pieces."""
    from finaletoolkit_amd import _lib as L
    T, BATCH = tile(), L.PREFENDS_BATCH_TILES
    edge = BATCH * T
    size = edge + T + 9
    frags = [((77, 240), 2), ((edge - 300, edge - 140), 2), ((edge - 3, edge + 160), 2), ((edge, edge + 167), 3),
             ((edge + 2, edge + 150), 1), ((size - 160, size), 2)]
    called = [77, 239, edge - 300, edge - 141, edge - 3, edge, edge + 159, edge + 166, size - 160, size - 1]
    kw = dict(half=500, thresholds=flat_table(1))
    with Contig(engine, *columns(*[(np.full(n, a), np.full(n, b)) for (a, b), n in frags])) as c:
        calls, stats = c.both([0], [size], size, mode="combined", min_count=2, **kw)
        assert calls["pos"].tolist() == called and calls["kind"].tolist() == [2] * 10
        assert calls["total"][2:8].tolist() == [16] * 6 and calls["n_w"][2:8].tolist() == [1001] * 6
        assert stats.tolist() == [[12, 12, 10, 0, 10, 0]]
        calls, stats = c.both([0], [size], size, mode="combined", min_count=3, **kw)  # the first batch brings no call home
        assert calls.tolist() == [(0, edge, 2, 3, 16, 1001), (0, edge + 166, 2, 3, 16, 1001)]
        assert stats.tolist() == [[12, 12, 2, 0, 2, 0]]
        calls, stats = c.both([0], [size], size, mode="split", min_count=2, **kw)
        assert calls["pos"].tolist() == called and calls["kind"].tolist() == [0, 1, 0, 1, 0, 0, 1, 1, 0, 1]
        assert calls["total"][2:8].tolist() == [8] * 6
        assert stats.tolist() == [[12, 12, 5, 5, 5, 5]]


# ---- 5. the refusals of the C call ----------------------------------------------------------------------------------------
def test_argument_errors(engine):
    import torch
    from finaletoolkit_amd import _lib as L
    lib, ctx, P = engine.lib, engine.ctx, L.ptr
    INV = L.FTK_ERR_INVALID
    size = 5_000
    rng = np.random.default_rng(3)
    cols = random_fragments(rng, size, 30)
    s, e = np.array([0, 1_000, 4_000], np.int64), np.array([900, 1_000, 5_000], np.int64)
    thr = flat_table(1)
    with Contig(engine, *cols) as c:
        cid = engine.contig_id(c.name)
        good = c.both(s, e, size, half=7, thresholds=thr)
        assert len(good[0]) >= 1
        stats = np.full(18, 7, np.int64)
        d_s, d_thr, d_stats = torch.from_numpy(s).cuda(), torch.from_numpy(thr.view(np.int64)).cuda(), torch.from_numpy(stats).cuda()

        def call(ctx_=ctx, cid_=cid, s_=s, e_=e, n=3, size_=size, half=7, mode=0, min_count=2, thr_=thr, n_thr=len(thr), stats_=stats,
                 drop=None):
            ptrs = [C.c_void_p(1) for _ in range(6)]
            count = C.c_int64(7)
            outs = [C.byref(p) for p in ptrs] + [C.byref(count)]
            if drop is not None:
                outs[drop] = None
            rc = lib.ftk_preferred_ends(ctx_, cid_, P(s_), P(e_), n, size_, half, mode, min_count, P(thr_), n_thr, -1, -1, 30, *outs,
                                        P(stats_))
            if rc != L.FTK_OK and ctx_ is not None and drop is None:  # a refused call leaves the output pointers NULL
                assert count.value == 0 and all(p.value is None for p in ptrs)
            for p in ptrs:
                if p.value not in (None, 1):
                    lib.ftk_buffer_free(p.value)
            return rc

        def failed(rc, word=None, code=INV):
            assert rc == code, (rc, code)
            message = lib.ftk_last_error(ctx)
            assert message and (word is None or word in message), message
            assert_same(engine.preferred_ends(c.name, s, e, size, half=7, thresholds=thr), good, word)  # a good call still answers

        assert call(ctx_=None) == INV
        for name in ("s_", "e_", "thr_", "stats_"):
            failed(call(**{name: None}), b"NULL")
        for k in range(7):
            failed(call(drop=k), b"NULL")
        for name, dev in (("s_", d_s), ("e_", d_s), ("thr_", d_thr), ("stats_", d_stats)):
            failed(call(**{name: dev}), b"host")
        failed(call(n=-1), b"n_iv")
        failed(call(s_=np.array([-1, 1_000, 4_000], np.int64)), b"interval")
        failed(call(e_=np.array([900, 999, 5_000], np.int64)), b"interval")
        failed(call(e_=np.array([900, 1_000, 5_001], np.int64)), b"interval")
        for bad in (-1, 1 << 30):
            failed(call(size_=bad), b"chrom_size")
        for bad in (0, -1, 2_049):
            failed(call(half=bad), b"half")
        for bad in (-1, 2):
            failed(call(mode=bad), b"mode")
        for bad in (0, -1):
            failed(call(min_count=bad), b"min_count")
        for bad in (1, 0, 4_097):
            failed(call(n_thr=bad), b"n_thr")
        over = thr.copy()
        over[3] = 1 << 40
        failed(call(thr_=over), b"threshold")
        failed(call(cid_=987_654), None, L.FTK_ERR_NO_CONTIG)
        assert np.all(stats == 7)  # none of them wrote a counter
        assert call(n=0) == L.FTK_OK and call(n=0, s_=None, e_=None, stats_=None) == L.FTK_OK and np.all(stats == 7)
        assert call() == L.FTK_OK and np.array_equal(stats.reshape(3, 6), good[1])
        assert call(half=2_048, mode=1, n_thr=2) == L.FTK_OK  # the limits themselves
        top = np.full(4_096, (1 << 40) - 1, np.uint64)
        assert call(thr_=top, n_thr=4_096, size_=(1 << 30) - 1) == L.FTK_OK


# ---- 6. the product path --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def product(engine, tmp_path_factory):
    from finaletoolkit_amd import utils
    T = tile()
    d = tmp_path_factory.mktemp("prefends")
    sizes = [("eA", 3 * T + 5), ("eB", 5_000)]
    frags = {}
    for k, (name, n) in enumerate(sizes):
        s, e, q = random_fragments(np.random.default_rng(40 + k), n, 30)
        e = np.minimum(e, n)  # (a BAM holds no alignment beyond its contig)
        keep = e > s
        frags[name] = (s[keep].astype(np.int64), e[keep].astype(np.int64), q[keep].astype(np.int64), np.arange(keep.sum()) % 2)
    bam = str(d / "in.bam")
    decoded = write_synthetic_bam(bam, sizes, frags)
    rows = {c: tuple(np.array([r[k] for r in decoded[c]], np.int64) for k in range(3)) for c, _ in sizes}
    frag = str(d / "in.frag.gz")
    utils.frag_export(bam, frag, quality_threshold=0)
    chrom_sizes = str(d / "g.chrom.sizes")
    with open(chrom_sizes, "w") as fh:
        fh.write("".join(f"{c}\t{n}\n" for c, n in sizes))
    bed_rows = [("eA", 0, 6_000, "first"), ("eB", 1_000, 4_000, "b1"), ("eA", 2 * T - 7, 3 * T + 905, "beyond"), ("eA", 3_000, 3_900, "short"),
                ("eB", 0, 5_000, "whole"), ("eA", 9_000, 9_000, "empty"), ("eA", 5_000, 7_000, "overlap")]
    bed = str(d / "regions.bed")
    with open(bed, "w") as fh:
        fh.write("# regions\n" + "".join(f"{c}\t{a}\t{b}\t{nm}\t0\t{'+-'[i % 2]}\n" for i, (c, a, b, nm) in enumerate(bed_rows)))
    return dict(dir=d, bam=bam, frag=frag, chrom_sizes=chrom_sizes, bed=bed, rows=bed_rows, sizes=dict(sizes), frags=rows)


def restated(p, intervals, **kw):
    """``(calls, stats)`` of the product over ``intervals`` (clipped to their contigs) by the restatement, on the decoded rows."""
    from finaletoolkit_amd import utils
    parts, stats = [], np.zeros((len(intervals), 6), np.int64)
    for i, (c, a, b, _) in enumerate(intervals):
        size = p["sizes"][c]
        calls, stats[i] = preferred_ends_ref(*p["frags"][c], [min(a, size)], [min(b, size)], size, **kw)
        part = np.zeros(len(calls), utils.PREFERRED_END_DTYPE)
        part["interval"] = i
        for f in utils.PREFERRED_END_DTYPE.names[1:]:
            part[f] = calls[f]
        parts.append(part)
    return np.concatenate(parts), stats


@pytest.mark.parametrize("split", [False, True])
def test_frag_preferred_ends_with_intervals(engine, product, tmp_path, split):
    from finaletoolkit_amd import utils
    p = product
    out_frag, sum_frag = str(tmp_path / "frag.bed"), str(tmp_path / "frag.tsv")
    out_bam, sum_bam = str(tmp_path / "bam.bed.gz"), str(tmp_path / "bam.tsv.gz")
    res = utils.frag_preferred_ends(p["frag"], p["bed"], p["chrom_sizes"], out_frag, sum_frag, split=split)
    res_bam = utils.frag_preferred_ends(p["bam"], p["bed"], None, out_bam, sum_bam, split=split)
    assert res.intervals == p["rows"] == res_bam.intervals
    assert res.calls.dtype == utils.PREFERRED_END_DTYPE and res.stats.shape == (7, 6) and res.stats.dtype == np.int64
    assert res.calls.tobytes() == res_bam.calls.tobytes() and np.array_equal(res.stats, res_bam.stats)
    want_calls, want_stats = restated(p, p["rows"], half=500, mode="split" if split else "combined", min_count=2,
                                      thresholds=utils.preferred_end_thresholds(0.01))
    assert res.calls.tobytes() == want_calls.tobytes() and np.array_equal(res.stats, want_stats) and len(res.calls) > 20
    for i in range(7):
        ends = want_stats[i, 0] + want_stats[i, 1]
        on_calls = want_calls["count"][want_calls["interval"] == i].sum()
        assert (np.isnan(res.share[i]) and ends == 0) or res.share[i] == on_calls / ends
    assert np.isnan(res.share[5]) and 0 < res.share[0] < 0.2
    # the files, read back
    text = open(out_frag).read()
    assert gzip.open(out_bam, "rt").read() == text and gzip.open(sum_bam, "rt").read() == open(sum_frag).read()
    lines = text.splitlines()
    assert len(lines) == len(res.calls)
    for line, call in zip(lines, res.calls.tolist()):
        i, pos, kind, count, total, n_w = call
        c, _, _, nm = p["rows"][i]
        assert line.split("\t")[:8] == [c, str(pos), str(pos + 1), nm, "UDB"[kind], str(count), str(total), format(total / n_w, ".6g")]
        assert float(line.split("\t")[8]) >= 2.0  # every call is significant at alpha = 0.01
    summary = open(sum_frag).read().splitlines()
    assert len(summary) == 8 and summary[1].split("\t")[:4] == ["eA", "0", "6000", "first"]
    assert [line.split("\t")[4:10] for line in summary[1:]] == [[str(x) for x in row] for row in res.stats]
    # the command line in a child process
    cli, cli_sum = str(tmp_path / "cli.bed"), str(tmp_path / "cli.tsv")
    r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.prefends", p["frag"], cli, "--chrom-sizes", p["chrom_sizes"], "--intervals",
                        p["bed"], "--summary", cli_sum] + ["--split"] * split, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(cli).read() == text and open(cli_sum).read() == open(sum_frag).read()
    if split:
        return
    # an interval on a contig the input lacks, and one the chrom.sizes file lacks
    other = tmp_path / "other.bed"
    other.write_text("eA\t100\t2900\tg\neZ\t100\t2900\th\n")
    with pytest.raises(ValueError, match="eZ"):
        utils.frag_preferred_ends(p["bam"], str(other))
    with pytest.raises(ValueError, match="chrom_sizes"):
        utils.frag_preferred_ends(p["frag"], str(other), p["chrom_sizes"])


def test_whole_contigs_do_not_depend_on_the_chunks(engine, product, tmp_path):
    from finaletoolkit_amd import utils
    p = product
    T = tile()
    out, summary = str(tmp_path / "whole.bed"), str(tmp_path / "whole.tsv")
    small = utils.frag_preferred_ends(p["frag"], None, p["chrom_sizes"], out, summary, chunk_size=T - 3, alpha=0.05, min_count=1)
    large = utils.frag_preferred_ends(p["frag"], None, p["chrom_sizes"], alpha=0.05, min_count=1)
    from_bam = utils.frag_preferred_ends(p["bam"], chunk_size=1_000, alpha=0.05, min_count=1)
    whole = [("eA", 0, 3 * T + 5, "."), ("eB", 0, 5_000, ".")]
    assert small.intervals == whole == large.intervals == from_bam.intervals
    assert small.calls.tobytes() == large.calls.tobytes() == from_bam.calls.tobytes() and len(small.calls) > 100
    assert np.array_equal(small.stats, large.stats) and np.array_equal(small.stats, from_bam.stats)
    assert np.array_equal(small.share, large.share)
    want_calls, want_stats = restated(p, whole, half=500, mode="combined", min_count=1, thresholds=utils.preferred_end_thresholds(0.05))
    assert small.calls.tobytes() == want_calls.tobytes() and np.array_equal(small.stats, want_stats)
    lines = open(out).read().splitlines()
    assert len(lines) == len(small.calls) and all(line.split("\t")[3] == "." for line in lines)
    assert [line.split("\t")[0] for line in lines] == ["eA"] * int(small.stats[0, CALLS_A]) + ["eB"] * int(small.stats[1, CALLS_A])
    assert len(open(summary).read().splitlines()) == 3
    # the command line writes the same files as the function
    cli, cli_sum = str(tmp_path / "cli.bed.gz"), str(tmp_path / "cli.tsv.gz")
    r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.prefends", p["bam"], cli, "--summary", cli_sum, "--alpha", "0.05",
                        "--min-count", "1", "--chunk-size", "777"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert gzip.open(cli, "rt").read() == open(out).read() and gzip.open(cli_sum, "rt").read() == open(summary).read()
