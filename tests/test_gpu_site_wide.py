"""GPU: the site kernels (``site_profile_kernel``, ``site_vplot_kernel``, ``site_ends_kernel``) over the axes the C ABI
admits and the other site tests never compare - half-widths from 2049 up to ``kSiteMaxHalfWidth = 2^20``, every way of
cutting them into up to 4096 bins, the per-site OCF windows at ``peak`` of about 10^6, and V-plot length axes up to 65 535
with up to 4096 rows - against the restatements of ``tests/site_profile_helpers.py``, ``tests/vplot_helpers.py`` and
``tests/site_ends_helpers.py``, exactly equal everywhere (sums and counts are integers).

Above ``H = 2048`` the column quotient (``quot`` in ``csrc/ftk_sitescan.h``) sees ``x`` up to ``2^21 - 1``, one site's
candidates are most of the contig (so a run is one site and many workgroups flush into one group), and ``site_ends``'
96 KiB two-track layout meets its split launch.  The tests that carry no ``gpu`` mark show from the data, without a
device, that the cases are what they are meant to be.

Two things are not as one might expect them.  ``ftk_site_vplot`` refuses a ``len_bin`` that does not divide ``len_hi -
len_lo + 1`` (``test_length_bins_that_do_not_divide_are_refused``), so the long length axes end on the top of their last
whole row - ``(50, 65 521, 16)`` and ``(37, 65 520, 17)`` - and the 14 and 15 lengths up to 65 535 lie above ``len_hi``:
they are left over all the same.  And the V-plot's LDS budget is a constant of the build (``kVplotLdsBytes``, 32 KiB),
not a switch: ``test_vplot_columns_wide`` runs under it and states how its matrices tile."""
import functools

import numpy as np
import pytest

from tests.site_ends_helpers import assert_same as assert_same_ends
from tests.site_ends_helpers import restated_site_ends
from tests.site_profile_helpers import restated_profile
from tests.vplot_helpers import ONE, assert_same, restated_vplot

gpu = pytest.mark.gpu
SPAN = 4_300_000              # the contig; LAST_END is its last fragment's end
LAST_END = SPAN
C0 = 2_150_000                # the reference centre: every shape's axis around it lies inside the contig
TOP = (1 << 30) - 1
SHAPES = ((1 << 20, 512), (1 << 20, 1 << 21), (1_048_575, 615), (1_048_575, 1023), (1_001_000, 500), (1_001_000, 1001),
          (1_001_000, 1625), (2049, 2))
N_BINS = (4096, 1, 3410, 2050, 4004, 2000, 1232, 2049)
HS = tuple(sorted({H for H, _ in SHAPES}))
FILTERS = ((0, None, None), (30, 120, 180))
HAND = 150                    # length of the hand-placed fragments: it passes both filters
LM = 2_000_000                # wide:long - the midpoint of the ladder of lengths
ROW_AXIS = (1000, 500)        # (H, b) of the long length axes: 4 columns
ROW_SHAPES = ((50, 65_521, 16), (37, 65_520, 17), (0, 4095, 1), (65_436, 65_535, 100))  # (len_lo, len_hi, lb)
N_ROWS = (4092, 3852, 4096, 1)
assert all((2 * H) % b == 0 and 2 * H // b == n <= 4096 for (H, b), n in zip(SHAPES, N_BINS))
assert all((hi - lo + 1) % lb == 0 and (hi - lo + 1) // lb == n <= 4096 for (lo, hi, lb), n in zip(ROW_SHAPES, N_ROWS))
assert all(C0 - H - HAND > 0 and C0 + H + HAND < SPAN for H in HS)


def axis_ends(H):
    """The positions around C0 that are the first bin, the last bin, and out on either side of the axis of half-width H."""
    return C0 - H, C0 + H - 1, C0 - H - 1, C0 + H


def ladder_lengths(lo, hi, lb):
    """Both sides of the bounds of rows 0, 1, 2, n_rows / 2, n_rows - 1 and of the end of the last row."""
    n_rows = (hi - lo + 1) // lb
    out = []
    for r in (0, 1, 2, n_rows // 2, n_rows - 1, n_rows):
        out += [lo + r * lb - 1, lo + r * lb]
    return sorted({n for n in out if 0 <= n <= 65_535})


@functools.lru_cache(maxsize=None)
def wide_columns(long=False):
    """(start, end, mapq, r1_start, r1_end, weight) sorted by start, read-only: 48 000 random fragments of lengths
    20-600 over [0, SPAN) (40 000 put 19 on the bin seams of b = 1625, and 20 are asked for); for every half-width H of
    SHAPES, on both sides of the MAPQ cut, a fragment with its midpoint, one with its U end and one with its D end on each
    of ``axis_ends(H)`` and on ``C0 - H + 1`` (the outermost OCF window's first base); for every shape a midpoint on either
    side of the seams of bins n_bins / 3 and n_bins - 1; fragments of one base at both ends of the contig.  ``long``: also
    what the contig ``wide:long`` adds - 400 fragments of lengths 1000-65 535 around LM, a ladder of lengths on LM for
    every shape of ROW_SHAPES, and one fragment of 65 535 bases."""
    rng = np.random.default_rng(20261020)
    a = rng.integers(0, SPAN - 700, 48_000)
    ln = rng.integers(20, 601, len(a))
    s, e, q = list(a), list(a + ln), list(rng.integers(0, 61, len(a)))
    for H in HS:
        for p in axis_ends(H) + (C0 - H + 1,):
            for mq in (30, 29):
                s += [p - HAND // 2, p, p - HAND + 1]  # the midpoint, the U end, the D end on p
                e += [p + HAND // 2, p + HAND, p + 1]
                q += [mq] * 3
    for (H, b), nb in zip(SHAPES, N_BINS):
        for x in {k * b - j for k in (nb // 3, nb - 1) for j in (0, 1) if k > 0}:  # d + H on the seam below bin k
            s.append(C0 - H + x - HAND // 2)
            e.append(C0 - H + x + HAND // 2)
            q.append(60)
    s += [0, 0, LAST_END - 100, LAST_END - 1]
    e += [1, 600, LAST_END, LAST_END]
    q += [60] * 4
    if long:
        extra = np.random.default_rng(65_535)
        mids = extra.integers(LM - 3000, LM + 3000, 400)
        lens = extra.integers(1000, 65_536, 400)
        s += list(mids - lens // 2)
        e += list(mids - lens // 2 + lens)
        q += list(extra.integers(0, 61, 400))
        for lo, hi, lb in ROW_SHAPES:
            for n in ladder_lengths(lo, hi, lb):
                s.append(LM - n // 2)
                e.append(LM - n // 2 + n)
                q.append(60)
        s.append(LM + 300 - 65_535 // 2)
        e.append(LM + 300 - 65_535 // 2 + 65_535)
        q.append(60)
    s, e, q = np.array(s, np.int64), np.array(e, np.int64), np.array(q, np.int64)
    fwd = rng.integers(0, 2, len(s)).astype(bool)
    rl = np.minimum(60, e - s)
    r1s = np.where(fwd, s, e - rl)
    w = np.where(rng.random(len(s)) < 0.2, 0, rng.integers(1, 2 ** 32, len(s))).astype(np.uint32)
    o = np.argsort(s, kind="stable")
    cols = tuple(c[o] for c in (s, e, q, r1s, r1s + rl, w))
    assert s.min() == 0 and e.max() == LAST_END and (e - s).max() == (65_535 if long else 600)
    assert (w == 0).sum() > 1000 and (w > 2 ** 31).sum() > 1000
    for c in cols:
        c.setflags(write=False)
    return cols


def axis_sites(H):
    """The sites every shape is compared at, each unflipped and flipped, each a group of its own: C0; 0, 5, H - 1 and H
    (the axis hangs over the contig's start, or just does not); the last fragment's last base in the first bin, and one
    further (nothing); the largest centre."""
    cs = [C0, 0, 5, H - 1, H, LAST_END + H - 1, LAST_END + H, TOP]
    centres = np.array(cs + cs, np.int32)
    flip = np.array([0] * len(cs) + [1] * len(cs), np.uint8)
    return centres, flip, np.arange(len(centres), dtype=np.int32)


def many_sites():
    """240 sites all over the contig and past its end in two groups: at these half-widths a run is one site, so more than
    a hundred workgroups flush into each group."""
    rng = np.random.default_rng(240)
    centres = rng.integers(0, SPAN + 50_000, 240).astype(np.int32)
    return centres, rng.integers(0, 2, 240).astype(np.uint8), (np.arange(240) % 2).astype(np.int32)


def row_sites():
    """wide:long - the ladder's midpoint in the middle, on c - H, on c + H - 1 and on c + H (out), each a group of its
    own, and 30 sites around it in two groups; every third site flipped."""
    rng = np.random.default_rng(4096)
    H = ROW_AXIS[0]
    centres = np.concatenate([[LM, LM + H, LM - H + 1, LM - H], rng.integers(LM - 4000, LM + 4000, 30)]).astype(np.int32)
    flip = (np.arange(len(centres)) % 3 == 2).astype(np.uint8)
    groups = np.concatenate([np.arange(4), 4 + np.arange(30) % 2]).astype(np.int32)
    return centres, flip, groups, 6


def midpoints(cols):
    return (cols[0] + cols[1]) >> 1


# ---- the cases are what they are meant to be: from the data, without a device ------------------------------------------------
@pytest.mark.parametrize("H, b", SHAPES)
def test_profile_cases_from_the_data(H, b):
    cols = wide_columns()
    centres, flip, groups = axis_sites(H)
    ng, half, nb = len(centres), len(centres) // 2, 2 * H // b
    at = {int(c): i for i, c in enumerate(centres[:half].tolist())}
    cnt0 = restated_profile(cols, None, centres, flip, groups, ng, H, b, 0)[1]
    cnt30 = restated_profile(cols, None, centres, flip, groups, ng, H, b, 30)[1]
    both = restated_profile(cols, None, centres, flip, groups, ng, H, b, 30, 120, 180)[1]
    mid, mq = midpoints(cols), cols[2]
    first, last, below, above = axis_ends(H)
    # the hand-placed pairs: MAPQ 30 counts and MAPQ 29 does not, in the first and in the last bin, under both filters
    for k, p in ((0, first), (nb - 1, last)):
        assert cnt0[at[C0], k] > cnt30[at[C0], k] >= both[at[C0], k] >= 1
        assert ((mid == p) & (mq == 30)).sum() >= 1 and ((mid == p) & (mq == 29)).sum() >= 1
    assert (mid == below).sum() >= 2 and (mid == above).sum() >= 2  # the pairs that are out on either side
    assert cnt0[at[C0]].sum() == ((mid >= first) & (mid <= last)).sum() > H // 100
    # the axis hangs over the contig's start: nothing left of base 0, the fragment (0, 1) in the first bin once c - H <= 0
    for c in (0, 5, H - 1, H):
        assert cnt0[at[c]].sum() > 0 and not cnt0[at[c], :(H - c) // b].any()
    assert cnt0[at[H], 0] >= 1 and cnt0[at[H - 1], 0] >= 1
    # the last fragment's midpoint (its only base) in the first bin; one further nothing; nothing near 2^30
    assert cnt0[at[LAST_END + H - 1]].sum() == cnt0[at[LAST_END + H - 1], 0] == 1
    assert not cnt0[at[LAST_END + H]].any() and not cnt0[at[TOP]].any()
    assert np.array_equal(cnt0[:half], cnt0[half:, ::-1]) and (nb == 1 or not np.array_equal(cnt0[:half], cnt0[half:]))
    # the seam of every bin: passing fragments on a bin's first or last offset
    if b <= 2048:
        x = mid[(mid >= first) & (mid <= last)] - C0 + H
        assert x.min() == 0 and x.max() == 2 * H - 1
        assert (((x % b) == 0) | ((x % b) == b - 1)).sum() >= 20
    centres, flip, groups = many_sites()
    assert len(centres) >= 200 and np.bincount(groups).tolist() == [120, 120] and 0 < flip.sum() < 240
    assert (restated_profile(cols, None, centres, flip, groups, 2, H, b, 0)[1].sum(axis=1) > 100_000 * (H > 2049)).all()


@pytest.mark.parametrize("H, b", SHAPES)
def test_end_cases_from_the_data(H, b):
    cols = wide_columns()
    centres, flip, groups = axis_sites(H)
    ng, half, nb = len(centres), len(centres) // 2, 2 * H // b
    at = {int(c): i for i, c in enumerate(centres[:half].tolist())}
    want0 = restated_site_ends(cols, None, centres, flip, groups, ng, H, b, 0, peak=H - 11, flank=10)
    want30 = restated_site_ends(cols, None, centres, flip, groups, ng, H, b, 30, peak=H - 11, flank=10)
    assert H - 11 + 10 < H and not (H - 11 + 11 < H)  # the outermost window the call admits
    first, last, below, above = axis_ends(H)
    u, d_end, mq = cols[0], cols[1] - 1, cols[2]
    for track, x in ((0, u), (1, d_end)):  # a U end and a D end on c - H and on c + H - 1, on both sides of the MAPQ cut
        for k, p in ((0, first), (nb - 1, last)):
            assert want0[1][at[C0], track, k] > want30[1][at[C0], track, k] >= 1
            assert ((x == p) & (mq == 30)).sum() >= 1 and ((x == p) & (mq == 29)).sum() >= 1
            assert want30[1][half + at[C0], 1 - track, nb - 1 - k] == want30[1][at[C0], track, k]  # flipped: the other track
        assert (x == below).sum() >= 2 and (x == above).sum() >= 2
        assert want0[1][at[C0], track].sum() == ((x >= first) & (x <= last) & (cols[1] > cols[0])).sum() > H // 100
    # the OCF windows at peak = H - 11: [c - H + 1, c - H + 21] and [c + H - 21, c + H - 1] hold the hand-placed ends on
    # their outer bases, of either kind, and the MAPQ-29 twins only without the cut
    assert (want0[3][at[C0]] > want30[3][at[C0]]).all() and (want30[3][at[C0]] >= 1).all()
    assert np.array_equal(want30[3][:half], want30[3][half:])  # (genome orientation: a flipped site has the same four)
    # both ends of the contig's last base in the first bin; nothing one further, nothing near 2^30
    assert want0[1][at[LAST_END + H - 1], :, 0].tolist() == [1, 2] and want0[1][at[LAST_END + H - 1]].sum() == 3
    assert not want0[1][at[LAST_END + H]].any() and not want0[1][at[TOP]].any() and not want0[3][at[TOP]].any()
    for c in (0, 5, H - 1, H):
        assert want0[1][at[c]].sum() > 0 and not want0[1][at[c], :, :(H - c) // b].any()


def test_length_axis_cases_from_the_data():
    cols, wide = wide_columns(long=True), wide_columns()
    assert len(cols[0]) > len(wide[0]) + 400 and (cols[1] - cols[0]).max() == 65_535 and (wide[1] - wide[0]).max() == 600
    H, b = ROW_AXIS
    ln, mid = cols[1] - cols[0], midpoints(cols)
    near = (mid >= LM - H) & (mid < LM + H)
    assert ((ln == 65_535) & near).sum() >= 2  # the ladder's and the one beside it
    for (lo, hi, lb), n_rows in zip(ROW_SHAPES, N_ROWS):
        cnt = restated_vplot(cols, None, [LM], None, None, 1, H, b, lo, hi, lb, 0)[1][0]
        assert cnt.shape == (n_rows, 2 * H // b)
        on = (mid == LM) & (cols[2] == 60)
        for n in ladder_lengths(lo, hi, lb):  # the ladder is there, and each rung is in the row the rule gives it
            assert (on & (ln == n)).sum() >= 1, n
            if lo <= n <= hi:
                assert cnt[(n - lo) // lb, H // b] >= 1, n
        # the top of the last whole row is counted: without the rung of length len_hi the last row holds one less
        top = on & (ln == hi)
        rest = tuple(c[~top] for c in cols[:3])
        less = restated_vplot(rest, None, [LM], None, None, 1, H, b, lo, hi, lb, 0)[1][0]
        assert (cnt - less).sum() == (cnt - less)[n_rows - 1, H // b] == top.sum() >= 1
        # what lies above len_hi - the lengths left over, 65 535 among them - and below len_lo is not
        assert cnt.sum() == (near & (ln >= lo) & (ln <= hi)).sum()
        if hi < 65_535:
            assert (near & (ln == hi + 1)).sum() >= 1
            assert lo + (n_rows + 1) * lb - 1 > 65_535 or n_rows == 4096  # no further whole row fits below 2^16
        if lo > 0:
            assert (near & (ln == lo - 1)).sum() >= 1
    centres, flip, groups, ng = row_sites()
    cnt = restated_vplot(cols, None, centres, flip, groups, ng, H, b, 50, 65_521, 16, 0)[1]
    assert cnt[0].sum() > 0 and cnt[3].sum() > 0 and cnt[1, :, 0].sum() >= 10 and cnt[2, :, 0].sum() >= 10  # (site 2 is flipped)
    assert (cnt[:, 1000:].sum(axis=(1, 2)) > 0).all()  # every group holds fragments of more than 16 kb


# ---- the device ------------------------------------------------------------------------------------------------------------
KEYS = ("wide", "wide:bam", "wide:long")


@pytest.fixture(scope="module")
def world(engine):
    wide, long = wide_columns(), wide_columns(long=True)
    for key, c, bam in (("wide", wide, False), ("wide:bam", wide, True), ("wide:long", long, False)):
        r1 = (c[3].astype(np.int32), c[4].astype(np.int32)) if bam else ()
        engine.load_contig(key, c[0].astype(np.int32), c[1].astype(np.int32), c[2].astype(np.uint8), np.zeros(len(c[0]), np.uint8), *r1)
        engine.set_weights(key, c[5])
    assert engine.is_bam("wide:bam") and not engine.is_bam("wide")
    yield {"wide": wide, "wide:bam": wide, "wide:long": long}
    for key in KEYS:
        engine.release(key)


@gpu
@pytest.mark.parametrize("H, b", SHAPES)
def test_site_profile_wide(engine, world, H, b):
    cols = world["wide"]
    for name, (centres, flip, groups) in (("axis", axis_sites(H)), ("many", many_sites())):
        ng = int(groups.max()) + 1
        for weighted in (False, True):
            for mapq_min, min_len, max_len in FILTERS:
                want = restated_profile(cols, cols[5] if weighted else None, centres, flip, groups, ng, H, b, mapq_min, min_len, max_len)
                got = engine.site_profile("wide", centres, flip, groups, ng, H, b, mapq_min, min_len, max_len, weighted=weighted)
                assert_same(got, want, (name, H, b, weighted, mapq_min))
                assert got[0].shape == (ng, 2 * H // b)
        bam = engine.site_profile("wide:bam", centres, flip, groups, ng, H, b, mapq_min, min_len, max_len, weighted=True)
        assert_same(bam, want, (name, H, b, "read1 columns"))


@gpu
@pytest.mark.parametrize("H, b", SHAPES)
def test_site_ends_wide(engine, world, H, b):
    cols = world["wide"]
    for name, (centres, flip, groups) in (("axis", axis_sites(H)), ("many", many_sites())):
        ng = int(groups.max()) + 1
        for peak, flank in ((60, 10), (H - 11, 10), (1, 0)):
            # (the list of 240: the outermost window under the first filter only - its restatement takes half a second)
            for mapq_min, min_len, max_len in FILTERS if name == "axis" else FILTERS[:peak == H - 11]:
                want = restated_site_ends(cols, cols[5], centres, flip, groups, ng, H, b, mapq_min, min_len, max_len, peak=peak, flank=flank)
                got = engine.site_ends("wide", centres, flip, groups, ng, H, b, mapq_min, min_len, max_len, weighted=True, peak=peak,
                                       flank=flank)
                assert_same_ends(got, want, (name, H, b, peak, flank, mapq_min))
                assert got[0].shape == (ng, 2, 2 * H // b)
        plain = restated_site_ends(cols, None, centres, flip, groups, ng, H, b, 30, peak=H - 11, flank=10)
        for key in ("wide", "wide:bam"):
            assert_same_ends(engine.site_ends(key, centres, flip, groups, ng, H, b, 30, peak=H - 11, flank=10), plain, (name, key))
        assert np.array_equal(plain[0], ONE * plain[1]) and np.array_equal(plain[2], ONE * plain[3])


@gpu
@pytest.mark.parametrize("split", [None, "0", "1"])
def test_site_ends_widest_under_each_split(engine, world, split, monkeypatch):
    """4096 bins x two tracks x 12 bytes = 96 KiB of LDS at the largest half-width; the switch as in
    ``test_gpu_site_ends.py::test_widest_weighted_profile``."""
    if split is None:
        monkeypatch.delenv("FTK_SITE_ENDS_SPLIT", raising=False)
    else:
        monkeypatch.setenv("FTK_SITE_ENDS_SPLIT", split)
    cols = world["wide"]
    H, b = SHAPES[0]
    assert 2 * H // b == 4096
    for centres, flip, groups in (axis_sites(H), many_sites()):
        ng = int(groups.max()) + 1
        for mapq_min in (0, 30):
            want = restated_site_ends(cols, cols[5], centres, flip, groups, ng, H, b, mapq_min, peak=H - 11, flank=10)
            got = engine.site_ends("wide", centres, flip, groups, ng, H, b, mapq_min, weighted=True, peak=H - 11, flank=10)
            assert_same_ends(got, want, (split, ng, mapq_min))
    assert (want[1][:, :, [0, -1]] > 0).all() and want[0].max() > 2 ** 32  # both tracks' outer bins of both groups


@gpu
@pytest.mark.parametrize("weighted", [False, True])
def test_vplot_columns_wide(engine, world, weighted):
    cols = world["wide"]
    H, b = SHAPES[0]
    len_lo, len_hi, lb = 100, 399, 100
    n_rows, n_bins, cell = 3, 4096, 12 if weighted else 4
    # the tiles of rows under the build's budget (32 KiB): one row each with weights, 2 + 1 without; a budget of 64 KiB
    # or of 160 KiB would tile the weighted matrix as 1 + 1 + 1 or whole, and hold the unweighted one whole
    assert [max(budget // (cell * n_bins), 1) for budget in (32 << 10, 64 << 10, 160 << 10)] == ([1, 1, 3] if weighted else [2, 4, 10])
    w = cols[5] if weighted else None
    for name, (centres, flip, groups) in (("axis", axis_sites(H)), ("many", many_sites())):
        ng = int(groups.max()) + 1
        for mapq_min in (0, 30):
            want = restated_vplot(cols, w, centres, flip, groups, ng, H, b, len_lo, len_hi, lb, mapq_min)
            for key in ("wide", "wide:bam"):
                got = engine.site_vplot(key, centres, flip, groups, ng, H, b, len_lo, len_hi, lb, mapq_min, weighted=weighted)
                assert_same(got, want, (name, key, weighted, mapq_min))
            assert got[0].shape == (ng, n_rows, n_bins) and ng * n_rows * n_bins <= 1 << 22
        whole = engine.site_profile("wide", centres, flip, groups, ng, H, b, 30, len_lo, len_hi, weighted=weighted)
        assert_same((got[0].sum(axis=1), got[1].sum(axis=1)), whole, (name, "rows summed"))
    assert all(want[1][:, r].any() for r in range(n_rows)) and (want[1][:, :, [0, -1]].sum(axis=(0, 1)) > 0).all()


@gpu
@pytest.mark.parametrize("len_lo, len_hi, lb", ROW_SHAPES)
def test_vplot_rows_wide(engine, world, len_lo, len_hi, lb):
    cols = world["wide:long"]
    H, b = ROW_AXIS
    centres, flip, groups, ng = row_sites()
    n_rows = (len_hi - len_lo + 1) // lb
    assert ng * n_rows * (2 * H // b) <= 1 << 22
    for weighted in (False, True):
        for mapq_min in (0, 30):
            want = restated_vplot(cols, cols[5] if weighted else None, centres, flip, groups, ng, H, b, len_lo, len_hi, lb, mapq_min)
            got = engine.site_vplot("wide:long", centres, flip, groups, ng, H, b, len_lo, len_hi, lb, mapq_min, weighted=weighted)
            assert_same(got, want, (len_lo, len_hi, lb, weighted, mapq_min))
            assert got[0].shape == (ng, n_rows, 2 * H // b)
    assert want[1][:, n_rows - 1].sum() >= 1  # the last row is not empty (test_length_axis_cases_from_the_data: why)


@gpu
def test_vplot_tiles_above_the_longest_fragment_are_empty(engine, world):
    """``len_lo`` above the contig's longest fragment (600): every tile's workgroups return before they touch their
    cells, and the zeroed outputs stay as they are.  With ``len_lo`` below it and ``len_hi`` far above, only the tiles
    of the first rows do any work."""
    cols = world["wide"]
    H, b = ROW_AXIS
    centres, flip, groups = many_sites()
    for weighted in (False, True):
        for len_lo, len_hi, lb in ((601, 700, 100), (608, 65_535, 16), (65_436, 65_535, 100)):
            sums, counts = engine.site_vplot("wide", centres, flip, groups, 2, H, b, len_lo, len_hi, lb, 0, weighted=weighted)
            assert sums.shape == (2, (len_hi - len_lo + 1) // lb, 4) and not sums.any() and not counts.any()
        w = cols[5] if weighted else None
        want = restated_vplot(cols, w, centres, flip, groups, 2, H, b, 544, 65_535, 16, 0)  # 4062 rows; lengths up to 600: rows 0-3
        assert_same(engine.site_vplot("wide", centres, flip, groups, 2, H, b, 544, 65_535, 16, 0, weighted=weighted), want, weighted)
        assert want[1][:, :4].sum(axis=(0, 2)).all() and not want[1][:, 4:].any()


@gpu
def test_length_bins_that_do_not_divide_are_refused(engine, world):
    """The length axes one would write first - ``(50, 65 535, 16)``: 4092 rows and 14 lengths over; ``(37, 65 535, 17)``:
    3852 rows and 15 over - are argument errors: the ABI has no ragged last row.  ROW_SHAPES ends them on their last
    whole row's top instead."""
    from finaletoolkit_amd import _lib as L
    for len_lo, len_hi, lb in ((50, 65_535, 16), (37, 65_535, 17)):
        assert (len_hi - len_lo + 1) % lb in (14, 15)
        with pytest.raises(L.FtkError, match="len_bin"):
            engine.site_vplot("wide:long", [LM], None, None, 1, *ROW_AXIS, len_lo, len_hi, lb, 0)
