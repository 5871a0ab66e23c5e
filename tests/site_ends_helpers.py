"""Shared pieces of the site-ends tests (``tests/test_gpu_site_ends.py``): the numpy restatement of ``ftk_site_ends``'s
rule on the V-plot tests' contig (``tests.vplot_helpers.vplot_contig``, used as it is).

The rule (``include/ftk.h``): a fragment ``[start, end)`` passes with ``mapq >= mapq_min`` and ``min_len <= end - start <=
max_len`` (None: no bound) and has its U end on base ``start`` and its D end on base ``end - 1`` (a fragment without a base
has no ends).  For site ``i``, an end at ``x`` with ``d = x - c_i`` in ``[-H, H)`` falls in bin ``k = (d + H) // b`` of
track 0 (U) or 1 (D): ``count[g_i][track][k] += 1``, ``sum[g_i][track][k] += w``; a flipped site uses bin ``n_bins - 1 -
k`` and the other track.  Per site, in genome orientation: ``left_up, left_down`` = the U / D ends with ``d`` in ``[-p - w,
-p + w]``, ``right_up, right_down`` those in ``[p - w, p + w]``."""
import numpy as np

from tests.vplot_helpers import ONE

SIGN = np.array([-1, 1, 1, -1], np.int64)  # OCF = (left_down - left_up) + (right_up - right_down)


def passing(cols, mapq_min=30, min_len=None, max_len=None):
    s, e, q = (np.asarray(cols[k], np.int64) for k in range(3))
    ln = e - s
    keep = (q >= mapq_min) & (ln >= 1)
    if min_len is not None:
        keep &= ln >= min_len
    if max_len is not None:
        keep &= ln <= max_len
    return keep


def restated_site_ends(cols, w, centres, flip, groups, n_groups, H, b, mapq_min=30, min_len=None, max_len=None, peak=None, flank=10):
    """(sums, counts) int64 of shape (n_groups, 2, n_bins), site by site; with ``peak`` also (site_sums, site_counts) of
    shape (n_sites, 4) in the order of ``centres``.  ``w``: the weight column, or None for FTK_WEIGHT_ONE each.  (The
    profile's weights are summed in two 16-bit halves, so that ``np.bincount``'s float64 sums stay exact: a half's sum
    stays below 2^16 * 2^31.  The per-site sums come from int64 prefix sums: below 2^32 * 2^31.)"""
    s, e = (np.asarray(cols[k], np.int64) for k in range(2))
    keep = passing(cols, mapq_min, min_len, max_len)
    wt = np.full(int(keep.sum()), ONE, np.int64) if w is None else np.asarray(w, np.int64)[keep]
    assert (2 * H) % b == 0
    n_bins = 2 * H // b
    centres = np.asarray(centres, np.int64)
    flip = np.zeros(len(centres), bool) if flip is None else np.asarray(flip).astype(bool)
    groups = np.zeros(len(centres), np.int64) if groups is None else np.asarray(groups, np.int64)
    ends = []  # per end kind (0: U, 1: D): positions in order, their weights, and the weights' prefix sums
    for x in (s[keep], e[keep] - 1):
        o = np.argsort(x, kind="stable")
        ends.append((x[o], wt[o], np.concatenate([[0], np.cumsum(wt[o])])))
    cells, weights = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    site_sums, site_counts = np.zeros((len(centres), 4), np.int64), np.zeros((len(centres), 4), np.int64)
    for kind, (x, xw, pre) in enumerate(ends):
        lo_i, hi_i = np.searchsorted(x, centres - H, "left"), np.searchsorted(x, centres + H, "left")
        for c, f, g, lo, hi in zip(centres.tolist(), flip.tolist(), groups.tolist(), lo_i.tolist(), hi_i.tolist()):
            if hi == lo:
                continue
            k = (x[lo:hi] - c + H) // b
            track = kind
            if f:
                k, track = n_bins - 1 - k, 1 - kind
            cells.append((g * 2 + track) * n_bins + k)
            weights.append(xw[lo:hi])
        if peak is not None:  # genome orientation: no flip
            for side, mid in enumerate((centres - peak, centres + peak)):
                lo_i, hi_i = np.searchsorted(x, mid - flank, "left"), np.searchsorted(x, mid + flank, "right")  # closed on both sides
                site_counts[:, 2 * side + kind] = hi_i - lo_i
                site_sums[:, 2 * side + kind] = pre[hi_i] - pre[lo_i]
    cells, x = np.concatenate(cells), np.concatenate(weights)
    total = n_groups * 2 * n_bins
    counts = np.bincount(cells, minlength=total)
    low = np.bincount(cells, weights=(x & 0xffff).astype(np.float64), minlength=total).astype(np.int64)
    high = np.bincount(cells, weights=(x >> 16).astype(np.float64), minlength=total).astype(np.int64)
    shape = (n_groups, 2, n_bins)
    out = ((high << 16) + low).reshape(shape), counts.astype(np.int64).reshape(shape)
    return out + (site_sums, site_counts) if peak is not None else out


def assert_same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, name in enumerate(("sums", "counts", "site_sums", "site_counts")[:len(want)]):
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, (what, name, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (what, name, bad[:5].tolist(), [int(got[k][tuple(i)]) for i in bad[:5]],
                               [int(want[k][tuple(i)]) for i in bad[:5]])
