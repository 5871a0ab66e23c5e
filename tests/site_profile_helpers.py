"""Shared piece of the site-profile tests (``tests/test_gpu_site_profile.py``, ``tests/test_gpu_site_wide.py``,
``tests/test_gpu_top_coordinates.py``): the numpy restatement of ``ftk_site_profile``'s rule.

The rule: a fragment passes with ``mapq >= mapq_min`` and ``min_len <= end - start <= max_len``; its midpoint is ``m =
(start + end) >> 1``; it contributes to site ``i`` when ``d = m - c_i`` lies in ``[-H, H)``, in bin ``k = (d + H) // b``
(``n_bins - 1 - k`` for a flipped site): ``count[g_i][k] += 1``, ``sum[g_i][k] += w``."""
import numpy as np

ONE = 65536           # FTK_WEIGHT_ONE


def restated_profile(cols, w, centres, flip, groups, n_groups, H, b, mapq_min=30, min_len=None, max_len=None):
    """(sums, counts) int64 of shape (n_groups, 2 H // b): the rule of the module's docstring, site by site.  ``w``:
    the weight column, or None for FTK_WEIGHT_ONE each.  (The weights are summed in two 16-bit halves, so that
    ``np.bincount``'s float64 sums stay exact.)"""
    s, e, q = (np.asarray(cols[k], np.int64) for k in range(3))
    ln = e - s
    keep = q >= mapq_min
    if min_len is not None:
        keep &= ln >= min_len
    if max_len is not None:
        keep &= ln <= max_len
    mid = ((s + e) >> 1)[keep]
    wt = np.full(len(mid), ONE, np.int64) if w is None else np.asarray(w, np.int64)[keep]
    o = np.argsort(mid, kind="stable")
    mid, wt = mid[o], wt[o]
    assert (2 * H) % b == 0
    n_bins = 2 * H // b
    sums, counts = np.zeros((n_groups, n_bins), np.int64), np.zeros((n_groups, n_bins), np.int64)
    centres = np.asarray(centres, np.int64)
    flip = np.zeros(len(centres), bool) if flip is None else np.asarray(flip).astype(bool)
    groups = np.zeros(len(centres), np.int64) if groups is None else np.asarray(groups, np.int64)
    lo_i, hi_i = np.searchsorted(mid, centres - H, "left"), np.searchsorted(mid, centres + H, "left")
    for c, f, g, lo, hi in zip(centres.tolist(), flip.tolist(), groups.tolist(), lo_i.tolist(), hi_i.tolist()):
        if hi == lo:
            continue
        k = (mid[lo:hi] - c + H) // b
        if f:
            k = n_bins - 1 - k
        x = wt[lo:hi]
        counts[g] += np.bincount(k, minlength=n_bins)
        low = np.bincount(k, weights=(x & 0xffff).astype(np.float64), minlength=n_bins).astype(np.int64)
        high = np.bincount(k, weights=(x >> 16).astype(np.float64), minlength=n_bins).astype(np.int64)
        sums[g] += (high << 16) + low
    return sums, counts
