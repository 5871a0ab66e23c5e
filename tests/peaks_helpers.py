"""The nucleosome-call rule of ``include/ftk.h`` ("peaks") restated in plain numpy, one Python loop per region and per
window, so that a window's area is added in the rule's own order: to 0, left to right, one float64 addition per value.
Every comparison against the kernels is exact - equal integers and bit-equal float64 - so there is no tolerance here."""
import numpy as np

PEAK_DTYPE = np.dtype([("run", np.int32), ("start", np.int64), ("stop", np.int64), ("summit", np.int64),
                       ("height", np.float64), ("area", np.float64)])
REGIONS, OPEN, SHORT, LONG, FLAT, CALLS = range(6)
DEFAULTS = dict(skip=0, max_gap=5, min_region=50, short_max=150, max_region=450)


def regions_of(a, lo, hi, max_gap):
    """``[(r0, r1)]``: the regions of the track ``[lo, hi)`` of ``a`` - positive positions joined over at most ``max_gap``
    positions between neighbours."""
    pos = [int(p) for p in np.flatnonzero(np.asarray(a[lo:hi]) > 0) + lo] if hi > lo else []
    out = []
    for p in pos:
        if out and p - out[-1][1] <= max_gap:  # (out[-1][1] is one past the last positive: p - that = positions between)
            out[-1][1] = p + 1
        else:
            out.append([p, p + 1])
    return [(r0, r1) for r0, r1 in out]


def windows_of(v, m):
    """``[(w0, w1)]``: the maximal runs of ``v > m``."""
    out, w0 = [], None
    for i, x in enumerate(v):
        if x > m:
            if w0 is None:
                w0 = i
        elif w0 is not None:
            out.append((w0, i))
            w0 = None
    if w0 is not None:
        out.append((w0, len(v)))
    return out


def peaks_ref(a, skip=0, max_gap=5, min_region=50, short_max=150, max_region=450):
    """``(calls, stats)`` of one run: ``calls`` a list of ``(start, stop, summit, height, area)`` in start order, ``stats``
    the six counters."""
    a = np.asarray(a, np.float64)
    n = len(a)
    lo, hi = skip, n - skip
    stats = np.zeros(6, np.int64)
    calls = []
    for r0, r1 in regions_of(a, lo, hi, max_gap):
        stats[REGIONS] += 1
        L = r1 - r0
        if r0 - lo <= max_gap or hi - r1 <= max_gap:
            stats[OPEN] += 1
            continue
        if L < min_region:
            stats[SHORT] += 1
            continue
        if L > max_region:
            stats[LONG] += 1
            continue
        v = a[r0:r1]
        s = np.sort(v)
        m = s[L // 2] if L % 2 else (s[L // 2 - 1] + s[L // 2]) / np.float64(2)
        wins = []
        for w0, w1 in windows_of(v, m):
            area = 0.0
            for x in v[w0:w1]:
                area = area + float(x)
            k = int(np.argmax(v[w0:w1]))  # (the first of equal maxima)
            wins.append((r0 + w0, r0 + w1, r0 + w0 + k, float(v[w0 + k]), area))
        if not wins:
            stats[FLAT] += 1
            continue
        if L <= short_max:
            best = wins[0]
            for w in wins[1:]:
                if w[4] > best[4]:
                    best = w
            keep = [best]
        else:
            keep = [w for w in wins if min_region <= w[1] - w[0] <= short_max]
        calls += keep
        stats[CALLS] += len(keep)
    return calls, stats


def peaks_ref_runs(scores, offsets, **kw):
    """``(calls, stats)`` as ``Engine.track_peaks`` returns them: a ``PEAK_DTYPE`` record array ordered by ``(run, start)``
    and the counters ``[n_runs, 6]``."""
    rows, stats = [], np.zeros((len(offsets) - 1, 6), np.int64)
    for r in range(len(offsets) - 1):
        calls, stats[r] = peaks_ref(scores[offsets[r]:offsets[r + 1]], **kw)
        rows += [(r,) + c for c in calls]
    return np.array(rows, PEAK_DTYPE) if rows else np.zeros(0, PEAK_DTYPE), stats


def same_calls(got, want):
    """Equal integers and bit-equal floats, field by field."""
    if got.shape != want.shape:
        return False
    return all(np.ascontiguousarray(got[f]).astype(PEAK_DTYPE[f]).tobytes() == np.ascontiguousarray(want[f]).tobytes()
               for f in PEAK_DTYPE.names)


def pack(runs):
    """(scores, offsets) of runs laid end to end."""
    offs = np.zeros(len(runs) + 1, np.int64)
    np.cumsum([len(r) for r in runs], out=offs[1:])
    return (np.concatenate(runs) if runs else np.zeros(0)).astype(np.float64), offs
