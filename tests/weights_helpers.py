"""Shared piece of the weighted-window-sum tests (``tests/test_gpu_gc_weights.py``,
``tests/test_gpu_top_coordinates.py``): the numpy restatement of ``ftk_weighted_window_sums``."""
import numpy as np


def restated_sums(cols, w, starts, stops, mapq_min, min_len, max_len, policy, bam):
    """(sums, n_weighted) int64 per window: the window predicate of the reference's fragment generator over the index
    query (tabix: the fragment overlaps the window; BAM: its read1 does), restated; the run of copies is one row with
    the sum of its weights.  A window whose stop lies below its start holds nothing (it has no candidate range)."""
    s, e, q, r1s, r1e, dup = cols
    first = int(np.flatnonzero(dup)[0])
    rows = np.concatenate([np.flatnonzero(~dup), [first]])
    wsum = np.concatenate([w[~dup].astype(np.int64), [w[dup].astype(np.int64).sum()]])
    wcnt = np.concatenate([(w[~dup] > 0).astype(np.int64), [int((w[dup] > 0).sum())]])
    s, e, q, r1s, r1e = s[rows], e[rows], q[rows], r1s[rows], r1e[rows]
    ln = e - s
    keep = q >= mapq_min
    if min_len is not None:
        keep &= ln >= min_len
    if max_len is not None:
        keep &= ln <= max_len
    mid = (s + e) // 2
    sums, cnt = np.zeros(len(starts), np.int64), np.zeros(len(starts), np.int64)
    for i, (a, b) in enumerate(zip(starts, stops)):
        a = -(1 << 40) if a is None else a
        b = (1 << 40) if b is None else b
        overlap = (s < b) & (e > a) & (b >= a)
        m = keep & ((r1s < b) & (r1e > a) & (b >= a) if bam else overlap)
        m &= ((mid >= a) & (mid < b)) if policy == "midpoint" else overlap
        sums[i], cnt[i] = wsum[m].sum(), wcnt[m].sum()
    return sums, cnt
