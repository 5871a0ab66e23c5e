"""Shared pieces of the V-plot tests (``tests/test_gpu_vplot.py``): the contig - the recipe of the site-profile tests'
``profile_contig`` plus a ladder of lengths on one midpoint - and the numpy restatement of ``ftk_site_vplot``'s rule.

The rule: a fragment passes with ``mapq >= mapq_min`` and ``len_lo <= L = end - start <= len_hi``; its midpoint is ``m =
(start + end) >> 1``; it contributes to site ``i`` when ``d = m - c_i`` lies in ``[-H, H)``, in row ``r = (L - len_lo) //
lb`` and column ``k = (d + H) // b`` (``n_bins - 1 - k`` for a flipped site): ``count[g_i][r][k] += 1``, ``sum[g_i][r][k]
+= w``."""
import numpy as np

from tests.gc_genome import N_DUP

ONE = 65536           # FTK_WEIGHT_ONE
CHUNK = 4096          # kChunk
U32_MAX = 2 ** 32 - 1
EVEN, ODD = (5_000, 5_100), (7_000, 7_101)  # hand-placed fragments: midpoints 5050 and 7050 (7050.5 rounded down)
GAP = (30_000, 33_000)                      # no fragment starts or ends in here
DUP = (1_000, 1_150)                        # N_DUP copies: midpoint 1075, length 150
LONG = (35_700, 36_400)                     # the contig's longest fragment (700): its start lies in the 512-bp index bin
LONG_MID = 36_050                           # before the one of its midpoint
LONG_LEN = LONG[1] - LONG[0]
LAST_END = 40_600
LADDER_MID = 20_000                         # one fragment of every length in LADDER, all with this midpoint, mapq 60
LADDER = range(90, 216)
assert N_DUP > CHUNK and (LONG[0] >> 9) < (LONG_MID >> 9)


def vplot_contig(rng):
    """(start, end, mapq, r1_start, r1_end) sorted by start: about 8 000 random fragments of lengths 20-600 outside GAP,
    the hand-placed ones on both sides of the MAPQ threshold, the ladder, LONG, and N_DUP copies of DUP."""
    a = np.concatenate([rng.integers(0, 29_000, 6000), rng.integers(33_100, 40_000, 1500)])
    ln = rng.integers(20, 601, len(a))
    outside = (a + ln <= GAP[0]) | (a >= GAP[1])
    a, ln = a[outside], ln[outside]
    lad_s = [LADDER_MID - n // 2 for n in LADDER]
    lad_e = [s + n for s, n in zip(lad_s, LADDER)]
    s = list(a) + [EVEN[0], ODD[0], EVEN[0], ODD[0], 0, 0, 39_990, LONG[0]] + lad_s + [DUP[0]] * N_DUP
    e = list(a + ln) + [EVEN[1], ODD[1], EVEN[1], ODD[1], 1, 600, LAST_END, LONG[1]] + lad_e + [DUP[1]] * N_DUP
    q = list(rng.integers(0, 61, len(a))) + [60, 60, 29, 30, 60, 60, 60, 60] + [60] * len(LADDER) + [60] * N_DUP
    s, e, q = np.array(s, np.int64), np.array(e, np.int64), np.array(q, np.int64)
    fwd = rng.integers(0, 2, len(s)).astype(bool)
    rl = np.minimum(60, e - s)
    r1s = np.where(fwd, s, e - rl)
    o = np.argsort(s, kind="stable")
    s, e, q, r1s, rl = s[o], e[o], q[o], r1s[o], rl[o]
    assert (e - s).max() == LONG_LEN and ((e - s) == LONG_LEN).sum() == 1
    assert all(((s + e) >> 1)[(e - s == n) & (q == 60)].tolist().count(LADDER_MID) >= 1 for n in LADDER)
    return s, e, q, r1s, r1s + rl


def restated_vplot(cols, w, centres, flip, groups, n_groups, H, b, len_lo, len_hi, lb, mapq_min=30):
    """(sums, counts) int64 of shape (n_groups, n_rows, n_bins): the rule of the module's docstring, site by site.
    ``w``: the weight column, or None for FTK_WEIGHT_ONE each.  (The weights are summed in two 16-bit halves, so that
    ``np.bincount``'s float64 sums stay exact: a half's sum stays below 2^16 * 2^31.)"""
    s, e, q = (np.asarray(cols[k], np.int64) for k in range(3))
    ln = e - s
    keep = (q >= mapq_min) & (ln >= len_lo) & (ln <= len_hi)
    mid, row = ((s + e) >> 1)[keep], (ln[keep] - len_lo) // lb
    wt = np.full(len(mid), ONE, np.int64) if w is None else np.asarray(w, np.int64)[keep]
    o = np.argsort(mid, kind="stable")
    mid, row, wt = mid[o], row[o], wt[o]
    assert (2 * H) % b == 0 and (len_hi - len_lo + 1) % lb == 0
    n_bins, n_rows = 2 * H // b, (len_hi - len_lo + 1) // lb
    centres = np.asarray(centres, np.int64)
    flip = np.zeros(len(centres), bool) if flip is None else np.asarray(flip).astype(bool)
    groups = np.zeros(len(centres), np.int64) if groups is None else np.asarray(groups, np.int64)
    lo_i, hi_i = np.searchsorted(mid, centres - H, "left"), np.searchsorted(mid, centres + H, "left")
    cells, weights = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for c, f, g, lo, hi in zip(centres.tolist(), flip.tolist(), groups.tolist(), lo_i.tolist(), hi_i.tolist()):
        if hi == lo:
            continue
        k = (mid[lo:hi] - c + H) // b
        if f:
            k = n_bins - 1 - k
        cells.append((g * n_rows + row[lo:hi]) * n_bins + k)
        weights.append(wt[lo:hi])
    cells, x = np.concatenate(cells), np.concatenate(weights)
    total = n_groups * n_rows * n_bins
    counts = np.bincount(cells, minlength=total)
    low = np.bincount(cells, weights=(x & 0xffff).astype(np.float64), minlength=total).astype(np.int64)
    high = np.bincount(cells, weights=(x >> 16).astype(np.float64), minlength=total).astype(np.int64)
    shape = (n_groups, n_rows, n_bins)
    return ((high << 16) + low).reshape(shape), counts.astype(np.int64).reshape(shape)


def assert_same(got, want, what):
    for k, name in ((0, "sums"), (1, "counts")):
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, (what, name, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (what, name, bad[:5].tolist(), [int(got[k][tuple(i)]) for i in bad[:5]],
                               [int(want[k][tuple(i)]) for i in bad[:5]])
