"""The preferred-end rule of ``include/ftk.h`` ("preferred ends") restated in plain numpy: ``bincount`` for the end
tracks, ``cumsum`` for the window totals, then the inequality in ``uint64``.  Everything in the rule is an integer, so
every comparison against the kernels is exact equality - there is no tolerance here."""
import numpy as np

CALL_DTYPE = np.dtype([("run", np.int32), ("pos", np.int64), ("kind", np.int32), ("count", np.int32), ("total", np.int64),
                       ("n_w", np.int32)])
U_ENDS, D_ENDS, TESTED_A, TESTED_B, CALLS_A, CALLS_B = range(6)
KIND_U, KIND_D, KIND_B = 0, 1, 2
SHIFT = np.uint64(20)


def end_tracks(start, end, mapq, chrom_size, min_len=None, max_len=None, mapq_min=30):
    """``(u, d)`` int64 of ``chrom_size`` bases: the U ends (on ``start``) and the D ends (on ``end - 1``) of the fragments
    that pass; ends outside the contig do not exist."""
    start, end, mapq = np.asarray(start, np.int64), np.asarray(end, np.int64), np.asarray(mapq, np.int64)
    length = end - start
    keep = (mapq >= mapq_min) & (length > 0)
    if min_len is not None:
        keep &= length >= min_len
    if max_len is not None:
        keep &= length <= max_len
    up, down = start[keep], end[keep] - 1
    up = up[(up >= 0) & (up < chrom_size)]
    down = down[(down >= 0) & (down < chrom_size)]
    return (np.bincount(up, minlength=chrom_size).astype(np.int64)[:chrom_size],
            np.bincount(down, minlength=chrom_size).astype(np.int64)[:chrom_size])


def window_totals(e, half):
    """``(T, n_w)`` of every base of the track ``e``: the sum over ``[max(b - half, 0), min(b + half, n - 1)]`` and the bases
    of that window."""
    n = len(e)
    prefix = np.concatenate([[0], np.cumsum(e)]).astype(np.int64)  # prefix[i] = e[0] + ... + e[i - 1]
    b = np.arange(n, dtype=np.int64)
    lo, hi = np.maximum(b - half, 0), np.minimum(b + half, n - 1)
    return prefix[hi + 1] - prefix[lo], hi - lo + 1


def track_calls(e, half, min_count, thr):
    """``(tested, called, T, n_w)`` per base of one track: ``e >= min_count``, and with it ``T * 2^20 <= thr[min(e, n_thr -
    1)] * n_w`` in unsigned 64-bit arithmetic."""
    thr = np.asarray(thr, np.uint64)
    total, n_w = window_totals(e, half)
    tested = e >= min_count
    bound = thr[np.minimum(e, len(thr) - 1)] * n_w.astype(np.uint64)
    called = tested & ((total.astype(np.uint64) << SHIFT) <= bound)
    return tested, called, total, n_w


def preferred_ends_ref(start, end, mapq, starts, stops, chrom_size, half=500, mode="combined", min_count=2, thresholds=None,
                       min_length=None, max_length=None, quality_threshold=30):
    """``(calls, stats)`` as ``Engine.preferred_ends`` returns them: a ``CALL_DTYPE`` record array ordered by ``(run, pos,
    kind)`` and the counters ``[n_intervals, 6]``."""
    u, d = end_tracks(start, end, mapq, chrom_size, min_length, max_length, quality_threshold)
    tracks = [(KIND_B, u + d)] if mode == "combined" else [(KIND_U, u), (KIND_D, d)]
    done = [(kind, e) + track_calls(e, half, min_count, thresholds) for kind, e in tracks]
    stats = np.zeros((len(starts), 6), np.int64)
    parts = []
    for r, (a, b) in enumerate(zip(starts, stops)):
        a, b = int(a), int(b)
        stats[r, U_ENDS], stats[r, D_ENDS] = u[a:b].sum(), d[a:b].sum()
        rows = []
        for slot, (kind, e, tested, called, total, n_w) in enumerate(done):
            stats[r, TESTED_A + slot] = tested[a:b].sum()
            stats[r, CALLS_A + slot] = called[a:b].sum()
            pos = np.flatnonzero(called[a:b]) + a
            part = np.zeros(len(pos), CALL_DTYPE)
            part["run"], part["pos"], part["kind"] = r, pos, kind
            part["count"], part["total"], part["n_w"] = e[pos], total[pos], n_w[pos]
            rows.append(part)
        part = np.concatenate(rows)
        parts.append(part[np.lexsort((part["kind"], part["pos"]))])
    return (np.concatenate(parts) if parts else np.zeros(0, CALL_DTYPE)), stats


def same_calls(got, want):
    """Equal integers, field by field."""
    if got.shape != want.shape:
        return False
    return all(np.array_equal(np.asarray(got[f]).astype(CALL_DTYPE[f]), want[f]) for f in CALL_DTYPE.names)


def flat_table(c, n=8):
    """``thr[k] = c << 20`` for every ``k >= 1``: a position is called iff ``T <= c * n_w``."""
    thr = np.full(n, int(c) << 20, np.uint64)
    thr[0] = 0
    return thr


def random_fragments(rng, chrom_size, depth, mean=167.0, sd=25.0):
    """Start-sorted ``(start, end, mapq)`` of about ``depth`` x coverage: lengths ~N(mean, sd), at least 1; mapq 60, one in
    eight 10; fragments may reach beyond the contig."""
    n = max(int(depth * chrom_size / mean), 1)
    start = np.sort(rng.integers(0, max(chrom_size, 1), n)).astype(np.int32)
    length = np.maximum(np.rint(rng.normal(mean, sd, n)), 1).astype(np.int32)
    mapq = np.where(rng.integers(0, 8, n) == 0, 10, 60).astype(np.uint8)
    return start, (start + length).astype(np.int32), mapq
