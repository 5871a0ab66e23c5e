"""GPU: the later kernels on fragments just below 2^30, the largest coordinate the columns admit - the site kernels, depth
and depth runs, preferred ends, weighted window sums, cleavage and the fused ``wps_peaks`` / ``wps_spectrum``.
(``test_gpu_parity.py`` holds counts, histograms, DELFI and WPS there.)  Up there the position index has 2^21 bins and a
bound may ask for a bin behind its last, the tiles of ``depth_kernel`` and ``prefends_kernel`` start next to 2^30, a
window of ``preferred_ends`` is clipped at ``chrom_size - 1``, and positions are written as int32 next to their limit.

Two twin contigs from one draw: ``top``, with its fragments in ``[TOP - 3 000 000, TOP]``, ``TOP = 2^30 - 1``, and ``low``,
the same fragments moved down by ``SHIFT`` - no multiple of 512, so the two position indexes cut the fragments
differently.  Every call has two assertions: the ``low`` result equals its restatement, which is cheap at small
coordinates, and the ``top`` result equals the ``low`` result with its positions moved by ``SHIFT``.  Where a restatement is
local to the region it is held against ``top`` directly as well.  Everything is an integer and compared exactly; the
spectrum is compared bit for bit (equal scores give equal bits: ``test_gpu_wps_spectrum.py``).

Out of scope here: the kernels that read a reference image (``frag_gc``, the GC weights, motifs) - at 2^30 they need an
image of 256 MB."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests.depth_helpers import check_invariants, kept, restated_depth, restated_runs
from tests.peaks_helpers import CALLS, peaks_ref_runs
from tests.peaks_helpers import same_calls as same_peaks
from tests.prefends_helpers import CALLS_A, CALLS_B, TESTED_A, TESTED_B, preferred_ends_ref
from tests.prefends_helpers import same_calls as same_ends
from tests.site_ends_helpers import assert_same as assert_same_ends
from tests.site_ends_helpers import restated_site_ends
from tests.site_profile_helpers import restated_profile
from tests.spectrum_helpers import assert_spectrum_close
from tests.vplot_helpers import assert_same, restated_vplot
from tests.weights_helpers import restated_sums

gpu = pytest.mark.gpu
TOP = (1 << 30) - 1
SPAN = 3_000_000
SHIFT = TOP - SPAN - 777
LOW_SIZE = TOP - SHIFT        # the chrom_size of ``low`` that clips a window where TOP clips it on ``top``
DENSE = 100_000               # the top DENSE bases hold nucleosome-like fragments at depth 30
N_COPIES = 50
COPY = (TOP - 40_000, TOP - 40_000 + 167)
SITE_SHAPES = ((990, 15), (1 << 20, 512))
FILTERS = ((0, None, None), (30, 120, 180))
assert SHIFT % 512 and LOW_SIZE == SPAN + 777 and TOP + 1 == 1 << 30


@functools.lru_cache(maxsize=None)
def twin_columns():
    """(start, end, mapq, r1_start, r1_end, is_copy, weight) of ``top``, sorted by start, read-only: 10 000 fragments of
    lengths 0-600 over the 3 Mb, 20 000 of 120-180 bases around centres every 190 +- 8 bases in the top DENSE bases, one
    fragment without a base on TOP, one ending on TOP, one on base TOP - 1 alone, and N_COPIES copies of COPY.  Read1 is
    the first or the last 60 bases (all of a shorter fragment)."""
    rng = np.random.default_rng(1 << 30)
    a = rng.integers(TOP - SPAN, TOP - 600, 10_000)
    ln = rng.integers(0, 601, len(a))
    centres = TOP - DENSE + np.cumsum(rng.integers(182, 199, DENSE // 190 + 2)) - 95
    centres = centres[centres < TOP - 100]
    c = centres[rng.integers(0, len(centres), 20_000)] + rng.integers(-12, 13, 20_000)
    dl = rng.integers(120, 181, len(c))
    s = np.concatenate([a, c - dl // 2, [TOP, TOP - 150, TOP - 1, TOP - SPAN], np.full(N_COPIES, COPY[0])]).astype(np.int64)
    e = np.concatenate([a + ln, c - dl // 2 + dl, [TOP, TOP, TOP, TOP - SPAN + 300], np.full(N_COPIES, COPY[1])]).astype(np.int64)
    e = np.minimum(e, TOP)
    q = np.concatenate([rng.integers(0, 61, len(a) + len(c)), [60, 60, 60, 60], np.full(N_COPIES, 60)])
    copy = np.concatenate([np.zeros(len(s) - N_COPIES, bool), np.ones(N_COPIES, bool)])
    fwd = rng.integers(0, 2, len(s)).astype(bool)
    fwd[copy] = False
    rl = np.minimum(60, e - s)
    r1s = np.where(fwd, s, e - rl)
    w = np.where(rng.random(len(s)) < 0.2, 0, rng.integers(1, 2 ** 32, len(s))).astype(np.uint32)
    o = np.lexsort((copy, s))  # by start, the copies behind what else starts there: one run of the column
    cols = tuple(x[o] for x in (s, e, q, r1s, r1s + rl, copy, w))
    for x in cols:
        x.setflags(write=False)
    return cols


def low_of(cols):
    """The twin: every coordinate moved down by SHIFT."""
    return tuple(x - SHIFT for x in cols[:2]) + (cols[2],) + tuple(x - SHIFT for x in cols[3:5]) + cols[5:]


def first_midpoint(cols):
    return int(((cols[0] + cols[1]) >> 1).min())


def site_centres(H):
    """``top``'s sites, each unflipped and flipped in a group of its own: the largest centre, the axis ending on TOP and one
    short of it, the contig's first midpoint in the first bin, sites in the dense stretch and on the copies."""
    cs = [TOP, TOP - H, TOP - H + 1, first_midpoint(twin_columns()) + H, TOP - 50_000, (COPY[0] + COPY[1]) >> 1, TOP - 2_000_000]
    centres = np.array(cs + cs, np.int64)
    return centres, np.array([0] * len(cs) + [1] * len(cs), np.uint8), np.arange(len(centres), dtype=np.int32)


# ---- the fixtures are what they are meant to be: from the data, without a device ---------------------------------------------
def test_the_twins_from_the_data():
    top = twin_columns()
    low = low_of(top)
    s, e, q = top[:3]
    assert len(s) == 30_000 + 4 + N_COPIES and np.all(np.diff(s) >= 0) and s.min() == TOP - SPAN and e.max() == TOP
    assert (e - s).min() == 0 and (e - s).max() == 600
    assert ((s == TOP) & (e == TOP)).sum() == 1 and ((e == TOP) & (e > s)).sum() >= 2  # no base on TOP; fragments ending on it
    assert ((s == COPY[0]) & (e == COPY[1])).sum() == N_COPIES == top[5].sum() and np.all(np.diff(np.flatnonzero(top[5])) == 1)
    assert (np.diff(s) == 0).sum() >= N_COPIES
    assert np.all((top[3] >= s) & (top[4] <= e) & ((top[4] > top[3]) == (e > s)))  # read1 inside its fragment
    # the twin: the same columns SHIFT lower, from position 777 on; the 512-bp index bins cut them differently
    for k in (0, 1, 3, 4):
        assert np.array_equal(low[k] + SHIFT, top[k]) and low[k].min() >= 777
    assert low[1].max() == LOW_SIZE == TOP - SHIFT and all(low[k] is top[k] for k in (2, 5, 6))
    assert len(np.unique((s >> 9) - (low[0] >> 9))) == 2 and (s.max() >> 9) == (1 << 21) - 1  # the last bin of a 2^21-bin index
    assert (top[6] == 0).sum() > 1000 and (top[6] > 2 ** 31).sum() > 1000


@pytest.mark.parametrize("H, b", SITE_SHAPES)
def test_site_cases_from_the_data(H, b):
    top = twin_columns()
    centres, flip, groups = site_centres(H)
    ng, half = len(centres), len(centres) // 2
    assert centres.max() == TOP and (centres - SHIFT).min() >= 0
    cnt = restated_profile(top, None, centres, flip, groups, ng, H, b, 0)[1]
    low = restated_profile(low_of(top), None, centres - SHIFT, flip, groups, ng, H, b, 0)[1]
    assert np.array_equal(cnt, low)  # translation keeps every d
    at = {int(c): i for i, c in enumerate(centres[:half].tolist())}
    assert all(cnt[i].sum() > 0 for i in range(ng))
    assert not cnt[at[TOP], H // b + 1:].any() and cnt[at[TOP], :H // b].sum() > 0  # nothing behind the centre's own bin
    # the axis [TOP - 2 H, TOP) leaves out the midpoint on TOP (of the fragment without a base); one further on,
    # [TOP - 2 H + 1, TOP + 1) holds it in its last bin
    mid = (top[0] + top[1]) >> 1
    assert (mid == TOP).sum() == 1 and cnt[at[TOP - H + 1], -1] == (mid > TOP - b).sum() >= 2
    assert cnt[at[TOP - H], -1] == ((mid >= TOP - b) & (mid < TOP)).sum() >= 1
    assert cnt[at[TOP - H + 1]].sum() - cnt[at[TOP - H]].sum() == (mid == TOP).sum() - (mid == TOP - 2 * H).sum()
    assert cnt[at[first_midpoint(top) + H], 0] >= 1 and cnt[at[(COPY[0] + COPY[1]) >> 1]].sum() >= N_COPIES
    ends = restated_site_ends(top, None, centres, flip, groups, ng, H, b, 0, peak=60, flank=10)
    d_end = (top[1] - 1)[top[1] > top[0]]  # the last base there is, TOP - 1, holds D ends: in the last bin of both axes
    assert (d_end == TOP - 1).sum() >= 2 and ends[1][at[TOP - H], 1, -1] == (d_end >= TOP - b).sum()
    assert ends[1][at[TOP - H + 1], 1, -1] == (d_end > TOP - b).sum() >= 2 and ends[3][at[TOP - 50_000]].any()


def test_window_sums_restatement_is_the_oracle_s_count():
    """``restated_sums`` with every weight one is the C oracle's ``window_counts``, under the three policies and both fetch
    modes, on both twins - the windows on TOP, behind it, open and above 2^30 among them."""
    top = twin_columns()
    unit = np.ones(len(top[0]), np.uint32)
    for cols, down in ((top, 0), (low_of(top), SHIFT)):
        starts, stops = sum_windows(down)
        ws = np.array([O.OPEN_LO if a is None else a for a in starts], np.int32)
        we = np.array([O.OPEN_HI if b is None else b for b in stops], np.int32)
        for bam in (False, True):
            fr = O.Frags(cols[0], cols[1], cols[2], None, *((cols[3], cols[4]) if bam else ()))
            for policy in ("midpoint", "any", "fetch"):
                for mapq_min, min_len, max_len in FILTERS:
                    want = O.c_window_counts(fr, ws, we, mapq_min=mapq_min, min_len=min_len, max_len=max_len, policy=policy)
                    got = restated_sums(cols[:6], unit, starts, stops, mapq_min, min_len, max_len, policy, bam)
                    assert np.array_equal(got[0], want) and np.array_equal(got[1], want), (down, bam, policy, mapq_min)
    assert want[2] > 1000 and want[0] >= 0 and want[1] == 0 and want[3] == 0


def sum_windows(down):
    """(starts, stops) with ``None`` for an open bound: the last base, the base behind it, the whole axis, one above 2^30,
    and windows inside the data; moved ``down``."""
    pairs = [(TOP - 1, TOP), (TOP, TOP + 1), (None, None), ((1 << 30) + 5, (1 << 30) + 700), (TOP - 150, TOP + 1), (None, TOP - 50_000),
             (TOP - DENSE, None), (COPY[0] - 100, COPY[0] + 40), (COPY[1] - 30, COPY[1] + 500), (TOP - SPAN, TOP - SPAN + 1),
             (TOP - 2_000_000, TOP - 1_000_000), (TOP - 70_000, TOP - 70_000)]
    return ([None if a is None else a - down for a, _ in pairs], [None if b is None else b - down for _, b in pairs])


def oracle_frags(cols, bam):
    """The oracle's view of a twin: with its read1 columns it answers with the BAM fetch rule, as a ``:bam`` contig does (a
    fragment that reaches over an interval's bound counts there only if its read1 overlaps the interval)."""
    return O.Frags(cols[0], cols[1], cols[2], None, *((cols[3], cols[4]) if bam else ()))


def dense_intervals():
    """Four intervals in the top DENSE bases: the last bases up to 2^30, one of a few tiles, one short of a callable
    track, one on odd bounds."""
    return np.array([TOP + 1 - 9_000, TOP - 60_001, TOP - 30_000, TOP - 95_123], np.int64), \
        np.array([TOP + 1, TOP - 47_000, TOP - 29_100, TOP - 90_000], np.int64)


# ---- the device ------------------------------------------------------------------------------------------------------------
KEYS = ("top", "top:bam", "low", "low:bam")


@pytest.fixture(scope="module")
def twins(engine):
    top = twin_columns()
    low = low_of(top)
    for key, c in (("top", top), ("top:bam", top), ("low", low), ("low:bam", low)):
        r1 = (c[3].astype(np.int32), c[4].astype(np.int32)) if key.endswith("bam") else ()
        engine.load_contig(key, c[0].astype(np.int32), c[1].astype(np.int32), c[2].astype(np.uint8), np.zeros(len(c[0]), np.uint8), *r1)
        engine.set_weights(key, c[6])
        assert engine.is_bam(key) == key.endswith("bam")
    assert engine.info("top")[2] == TOP and engine.info("low")[2] == LOW_SIZE  # the largest end
    yield dict(top=top, low=low)
    for key in KEYS:
        engine.release(key)


@gpu
@pytest.mark.parametrize("H, b", SITE_SHAPES)
def test_site_calls(engine, twins, H, b):
    top, low = twins["top"], twins["low"]
    centres, flip, groups = site_centres(H)
    ng = len(centres)
    rows = (100, 399, 100) if 2 * H // b == 4096 else (20, 599, 20)
    assert ng * ((rows[1] - rows[0] + 1) // rows[2]) * (2 * H // b) <= 1 << 22
    for weighted in (False, True):
        w = top[6] if weighted else None
        for mapq_min, min_len, max_len in FILTERS:
            what = (H, b, weighted, mapq_min)
            want = restated_profile(low, w, centres - SHIFT, flip, groups, ng, H, b, mapq_min, min_len, max_len)
            assert_same(engine.site_profile("low", centres - SHIFT, flip, groups, ng, H, b, mapq_min, min_len, max_len, weighted=weighted),
                        want, ("low",) + what)
            for key in ("top", "top:bam"):
                assert_same(engine.site_profile(key, centres, flip, groups, ng, H, b, mapq_min, min_len, max_len, weighted=weighted), want,
                            (key,) + what)
            assert_same(restated_profile(top, w, centres, flip, groups, ng, H, b, mapq_min, min_len, max_len), want, "the restatement on top")
            want = restated_site_ends(low, w, centres - SHIFT, flip, groups, ng, H, b, mapq_min, min_len, max_len, peak=60, flank=10)
            assert_same_ends(engine.site_ends("low", centres - SHIFT, flip, groups, ng, H, b, mapq_min, min_len, max_len, weighted=weighted,
                                              peak=60, flank=10), want, ("low",) + what)
            for key in ("top", "top:bam"):
                assert_same_ends(engine.site_ends(key, centres, flip, groups, ng, H, b, mapq_min, min_len, max_len, weighted=weighted,
                                                  peak=60, flank=10), want, (key,) + what)
        for mapq_min in (0, 30):
            want = restated_vplot(low, w, centres - SHIFT, flip, groups, ng, H, b, *rows, mapq_min)
            assert_same(engine.site_vplot("low", centres - SHIFT, flip, groups, ng, H, b, *rows, mapq_min, weighted=weighted), want, "low")
            for key in ("top", "top:bam"):
                assert_same(engine.site_vplot(key, centres, flip, groups, ng, H, b, *rows, mapq_min, weighted=weighted), want, key)
    assert want[1].sum() > 1000


@gpu
@pytest.mark.parametrize("start, stop", [(TOP - 70_000, TOP), (TOP - 3 * 4096 - 5, TOP), (TOP - 4096, TOP), (TOP - 1, TOP),
                                         (COPY[0] - 2_000, COPY[0] + 2_100), (TOP - SPAN, TOP - SPAN + 5_000)])
def test_depth_and_depth_runs(engine, twins, start, stop):
    """Regions that end on the last base a region may hold (``stop`` below 2^30), of a few tiles, of one and of one base."""
    top, low = twins["top"], twins["low"]
    for mapq_min, min_len, max_len in FILTERS:
        keep = kept(low[0], low[1], low[2], mapq_min, min_len, max_len)
        want = restated_depth(low[0], low[1], keep, start - SHIFT, stop - SHIFT)
        assert np.array_equal(restated_depth(top[0], top[1], keep, start, stop), want)  # the restatement is local: on top as well
        for key, down in (("low", SHIFT), ("top", 0), ("top:bam", 0)):
            got = engine.depth(key, start - down, stop - down, mapq_min, min_len, max_len)
            assert got.dtype == np.int32 and np.array_equal(got, want), (key, mapq_min)
            for include_zero in (False, True):
                runs = engine.depth_runs(key, start - down, stop - down, mapq_min, min_len, max_len, include_zero)
                exp = restated_runs(want, start - down, include_zero)
                assert all(a.dtype == np.int32 for a in runs)
                assert all(np.array_equal(g, x) for g, x in zip(runs, exp)), (key, mapq_min, include_zero)
                cols = low if key == "low" else top
                check_invariants(runs, start - down, stop - down, include_zero, cols[0], cols[1], keep)
    assert want.max() >= 1


@gpu
@pytest.mark.parametrize("mode", ["combined", "split"])
@pytest.mark.parametrize("half", [512, 513, 2048])
def test_preferred_ends(engine, twins, half, mode):
    """512 | 513: either side of the halo switch (kPrefHaloSmall).  ``chrom_size`` is TOP on ``top`` and TOP - SHIFT on ``low``:
    the windows of the last ``half`` positions are clipped at the same base of the data."""
    from finaletoolkit_amd import utils
    top, low = twins["top"], twins["low"]
    thr = utils.preferred_end_thresholds(0.01)
    T = 4096
    # the last 3 tiles and 5 bases, ending on the last base; across a tile bound of the first; one base; the copies
    starts = np.array([TOP - 3 * T - 5, TOP - 3 * T - 5 + T - 9, TOP - 1, COPY[0] - 3_000, TOP - 70_000], np.int64)
    stops = np.array([TOP, TOP - 3 * T - 5 + T + 9, TOP, COPY[1] + 3_000, TOP - 70_000 + 2 * T + 1], np.int64)
    assert (starts - SHIFT).min() > 2048 and stops.max() == TOP
    kw = dict(half=half, mode=mode, thresholds=thr)
    for more in (dict(), dict(min_count=1, min_length=120, max_length=180, quality_threshold=20)):
        want = preferred_ends_ref(*low[:3], starts - SHIFT, stops - SHIFT, LOW_SIZE, **kw, **more)
        got = engine.preferred_ends("low", starts - SHIFT, stops - SHIFT, LOW_SIZE, **kw, **more)
        assert np.array_equal(got[1], want[1]) and same_ends(got[0], want[0]), ("low", more)
        moved = want[0].copy()
        moved["pos"] += SHIFT
        for key in ("top", "top:bam"):
            got = engine.preferred_ends(key, starts, stops, TOP, **kw, **more)
            assert np.array_equal(got[1], want[1]) and same_ends(got[0], moved), (key, more)
        n_called, n_tested = want[1][:, [CALLS_A, CALLS_B]].sum(), want[1][:, [TESTED_A, TESTED_B]].sum()
        # calls, and tested positions that are not called (of a track of its own the widest window calls all it tests)
        assert len(want[0]) == n_called >= 10 and (n_tested > n_called or (mode, half) == ("split", 2048))
        assert (want[0]["n_w"] < 2 * half + 1).any() and moved["pos"].max() >= TOP - half  # a clipped window among the calls
    # the packed (length, mapq) column and the wide columns: an upper bound of 2047 keeps a packed contig on the wide ones
    assert engine.frags_packed("top") and not engine.frags_packed("top:bam")
    packed = engine.preferred_ends("top", starts, stops, TOP, **kw)
    wide = engine.preferred_ends("top", starts, stops, TOP, max_length=2_047, **kw)
    assert packed[0].tobytes() == wide[0].tobytes() and np.array_equal(packed[1], wide[1]) and len(packed[0]) >= 10


@gpu
@pytest.mark.parametrize("policy", ["midpoint", "any", "fetch"])
def test_weighted_window_sums(engine, twins, policy):
    top, low = twins["top"], twins["low"]
    w = top[6]
    for bam in (False, True):
        for mapq_min, min_len, max_len in FILTERS:
            starts, stops = sum_windows(SHIFT)
            want = restated_sums(low[:6], w, starts, stops, mapq_min, min_len, max_len, policy, bam)
            there = restated_sums(top[:6], w, *sum_windows(0), mapq_min, min_len, max_len, policy, bam)  # local: on top as well
            assert np.array_equal(there[0], want[0]) and np.array_equal(there[1], want[1])
            for key, down in (("low", SHIFT), ("top", 0)):
                got = engine.weighted_window_sums(key + ":bam" * bam, *sum_windows(down), mapq_min, min_len, max_len, policy)
                assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (key, bam, mapq_min)
    assert want[0][2] > 2 ** 40 and want[1][2] > 1000 and want[0][3] == 0 and want[0][1] == 0


@gpu
@pytest.mark.parametrize("bam", [False, True])
def test_cleavage(engine, twins, bam):
    top, low = twins["top"], twins["low"]
    a, b = TOP + 1 - 20_000, TOP + 1  # the last 20 000 bases below 2^30
    cuts = np.array([a, a + 4_095, a + 4_096 + 4_097, b - 1, b], np.int64)
    on_top, on_low = oracle_frags(top, bam), oracle_frags(low, bam)
    for lo, hi, mq in ((None, None, 0), (120, 180, 30), (0, 167, 20)):
        want = O.c_cleavage(on_low, a - SHIFT, b - SHIFT, lo, hi, mq)[2]
        assert np.array_equal(O.c_cleavage(on_top, a, b, lo, hi, mq)[2], want)
        # interval by interval: with read1 columns a fragment across a cut counts on the side of its read1 only
        pieces = np.concatenate([O.c_cleavage(on_low, x - SHIFT, y - SHIFT, lo, hi, mq)[2] for x, y in zip(cuts[:-1], cuts[1:])])
        assert np.array_equal(pieces, want) == (not bam)
        for key, down in (("low", SHIFT), ("top", 0)):
            key += ":bam" * bam
            assert np.array_equal(engine.cleavage(key, a - down, b - down, lo, hi, mq), want), (key, lo, hi, mq)
            got, offs = engine.cleavage_intervals(key, cuts[:-1] - down, cuts[1:] - down, lo, hi, mq)
            assert np.array_equal(got, pieces) and offs.tolist() == (cuts - a).tolist(), (key, lo, hi, mq)
    assert (want > 0).sum() > 1000 and O.c_cleavage(on_top, a, b, lo, hi, mq)[0][-2:].tolist() == [2, 0]  # depth on TOP - 1, none on TOP


def restated_peaks(engine, key, starts, stops, size, fr):
    """The calls of the restatement on ``key``'s adjusted track, moved to the contig as the fused call moves them; the
    scores are the oracle's."""
    W, sw = 1000, 21
    keep = [i for i in range(len(starts)) if stops[i] - starts[i] >= W + sw]
    scores, offs = engine.wps_intervals(key, starts[keep], stops[keep], size)
    for k, i in enumerate(keep):
        assert np.array_equal(scores[offs[k]:offs[k + 1]], O.c_wps(fr, int(starts[i]), int(stops[i]), size, 120, 120, 180, 30)), (key, i)
    adj = engine.wps_adjust(np.asarray(scores, np.float64), offs, W, savgol_window_size=sw)
    adj_offs = offs - np.arange(len(offs)) * W
    calls, kept_stats = peaks_ref_runs(adj, adj_offs, skip=sw // 2)
    shift = starts[keep][calls["run"]] + W // 2
    for name in ("start", "stop", "summit"):
        calls[name] += shift
    calls["run"] = np.asarray(keep, np.int32)[calls["run"]]
    stats = np.zeros((len(starts), 6), np.int64)
    stats[keep] = kept_stats
    return calls, stats


@gpu
@pytest.mark.parametrize("bam", [False, True])
def test_fused_wps_peaks(engine, twins, bam):
    top, low = twins["top"], twins["low"]
    on_top, on_low = "top" + ":bam" * bam, "low" + ":bam" * bam
    starts, stops = dense_intervals()
    assert stops.max() == 1 << 30 and (stops - starts).min() < 1021 <= np.sort(stops - starts)[1]
    want = restated_peaks(engine, on_low, starts - SHIFT, stops - SHIFT, (1 << 30) - SHIFT, oracle_frags(low, bam))
    there = restated_peaks(engine, on_top, starts, stops, 1 << 30, oracle_frags(top, bam))
    moved = want[0].copy()
    for name in ("start", "stop", "summit"):
        moved[name] += SHIFT
    assert same_peaks(there[0], moved) and np.array_equal(there[1], want[1])
    for batch in (None, 4_096):
        got = engine.wps_peaks(on_low, starts - SHIFT, stops - SHIFT, (1 << 30) - SHIFT, batch_bases=batch)
        assert same_peaks(got[0], want[0]) and np.array_equal(got[1], want[1]), (on_low, batch)
        got = engine.wps_peaks(on_top, starts, stops, 1 << 30, batch_bases=batch)
        assert same_peaks(got[0], moved) and np.array_equal(got[1], want[1]), (on_top, batch)
    assert (want[1][[0, 1, 3], CALLS] >= 10).all() and not want[1][2].any()  # calls in every callable interval
    # up to where the last interval's adjusted track ends: half a median window and the Savitzky-Golay skip below 2^30
    assert TOP - 1_200 < moved["stop"].max() <= (1 << 30) - 500 - 10


@gpu
@pytest.mark.parametrize("bam", [False, True])
def test_fused_wps_spectrum(engine, twins, bam):
    top, low = twins["top"], twins["low"]
    on_top, on_low = "top" + ":bam" * bam, "low" + ":bam" * bam
    starts, stops = dense_intervals()
    periods = np.arange(120, 281, dtype=np.int32)
    frs = {"top": oracle_frags(top, bam), "low": oracle_frags(low, bam)}
    for kw in (dict(), dict(taper=0.0, detrend=False, window_size=60, min_length=100, max_length=200, quality_threshold=20)):
        wps = (kw.get("window_size", 120), kw.get("min_length", 120), kw.get("max_length", 180), kw.get("quality_threshold", 30))
        want, want_ssw = engine.wps_spectrum(on_low, starts - SHIFT, stops - SHIFT, (1 << 30) - SHIFT, periods, **kw)
        for i in range(len(starts)):  # low: the restatement of the transform on the oracle's scores - which are top's scores, too
            v = O.c_wps(frs["low"], int(starts[i] - SHIFT), int(stops[i] - SHIFT), (1 << 30) - SHIFT, *wps)
            assert np.array_equal(O.c_wps(frs["top"], int(starts[i]), int(stops[i]), 1 << 30, *wps), v) and np.any(v)
            assert_spectrum_close(want[i], want_ssw[i], v, periods, kw.get("taper", 0.1), kw.get("detrend", True), what=i)
        for batch in (None, 4_096):
            got, got_ssw = engine.wps_spectrum(on_top, starts, stops, 1 << 30, periods, batch_bases=batch, **kw)
            assert got.tobytes() == want.tobytes() and got_ssw.tobytes() == want_ssw.tobytes(), (on_top, batch, kw)
    power = (want.real ** 2 + want.imag ** 2) / want_ssw[:, None]
    assert np.all(power.max(axis=1) > 0)
