"""The IFS hotspot rule of ``include/ftk.h`` ("IFS hotspots") restated in plain numpy: ``bincount`` for the bins' counts
and length sums, ``cumsum`` for the windows and their backgrounds, the inequalities in ``uint64``, a plain loop for the
merge.  Everything in the rule is an integer, so every comparison against the kernels is exact equality - there is no
tolerance here."""
import numpy as np

WINDOW_DTYPE = np.dtype([("run", np.int32), ("pos", np.int64), ("count", np.int32), ("ifs", np.int64), ("bg1", np.int64),
                         ("nb1", np.int32), ("bg2", np.int64), ("nb2", np.int32)])
HOTSPOT_DTYPE = np.dtype([("run", np.int32), ("start", np.int64), ("stop", np.int64), ("n_windows", np.int32),
                          ("summit", np.int64), ("ifs", np.int64), ("count", np.int32), ("bg1", np.int64), ("nb1", np.int32)])
WINDOWS, TESTED, CALLED, KEPT, DROPPED, BASES = range(6)
SHIFT = np.uint64(10)


def passing(start, end, mapq, chrom_size, min_len=None, max_len=None, mapq_min=30):
    """``(mid, length)`` of the fragments that pass and have their midpoint on the contig."""
    start, end, mapq = np.asarray(start, np.int64), np.asarray(end, np.int64), np.asarray(mapq, np.int64)
    length = end - start
    keep = (mapq >= mapq_min) & (length > 0)
    if min_len is not None:
        keep &= length >= min_len
    if max_len is not None:
        keep &= length <= max_len
    mid = (start + end) >> 1
    keep &= (mid >= 0) & (mid < chrom_size)
    return mid[keep], length[keep]


def totals_ref(start, end, mapq, chrom_size, min_length=None, max_length=None, quality_threshold=30):
    """``(N, S)``: Python integers."""
    mid, length = passing(start, end, mapq, chrom_size, min_length, max_length, quality_threshold)
    return int(len(mid)), int(length.sum())


def global_mean_ref(N, S, L, m, chrom_size, step):
    n_bins = -(-chrom_size // step)
    return (N * L + S) * m * 1024 // (n_bins * L) if n_bins else 0


def bin_tracks(start, end, mapq, chrom_size, step, L, min_len=None, max_len=None, mapq_min=30):
    """``(c, i)`` int64 per bin: the midpoints and ``c * L + l``."""
    n_bins = -(-chrom_size // step)
    mid, length = passing(start, end, mapq, chrom_size, min_len, max_len, mapq_min)
    c = np.bincount(mid // step, minlength=n_bins).astype(np.int64)[:n_bins]
    l = np.bincount(mid // step, weights=length, minlength=n_bins).astype(np.int64)[:n_bins]
    return c, c * L + l


def window_sums(x, m):
    """The sum of ``m`` consecutive entries for every window ``0 .. len(x) - m`` (none: empty)."""
    prefix = np.concatenate([[0], np.cumsum(x)]).astype(np.int64)
    n_win = max(len(x) - m + 1, 0)
    return prefix[m:m + n_win] - prefix[:n_win]


def backgrounds(i, m, h):
    """``(B, n_b)`` of every window: bins ``[max(k - h, 0), min(k + m - 1 + h, n_bins - 1)]``."""
    n_bins = len(i)
    n_win = max(n_bins - m + 1, 0)
    prefix = np.concatenate([[0], np.cumsum(i)]).astype(np.int64)
    k = np.arange(n_win, dtype=np.int64)
    lo, hi = np.maximum(k - h, 0), np.minimum(k + m - 1 + h, n_bins - 1)
    return prefix[hi + 1] - prefix[lo], hi - lo + 1


def interval_windows(a, b, chrom_size, step, m):
    """``(k_lo, k_hi)`` of interval ``[a, b)``: ``a <= k * step`` and the span's end ``<= b`` (none: ``k_hi < k_lo``)."""
    n_bins = -(-chrom_size // step)
    k_lo = -(-a // step)
    k_hi = k_lo - 1
    for k in range(min(b // step, n_bins - m), max(k_lo - 1, -1), -1):  # (at most m + 1 candidates fail)
        if min((k + m) * step, chrom_size) <= b:
            k_hi = k
            break
    return k_lo, k_hi


def ifs_track_ref(start, end, mapq, starts, stops, chrom_size, step=20, m=10, mean_length=167, min_length=None, max_length=None,
                  quality_threshold=30):
    """``(n, I, offsets)`` as ``Engine.ifs_track`` returns them."""
    c, i = bin_tracks(start, end, mapq, chrom_size, step, mean_length, min_length, max_length, quality_threshold)
    n_all, i_all = window_sums(c, m), window_sums(i, m)
    ns, is_, offs = [], [], [0]
    for a, b in zip(starts, stops):
        k_lo, k_hi = interval_windows(int(a), int(b), chrom_size, step, m)
        ns.append(n_all[k_lo:k_hi + 1])
        is_.append(i_all[k_lo:k_hi + 1])
        offs.append(offs[-1] + max(k_hi - k_lo + 1, 0))
    n = np.concatenate(ns).astype(np.int32) if ns else np.zeros(0, np.int32)
    ifs = np.concatenate(is_).astype(np.int64) if is_ else np.zeros(0, np.int64)
    return n, ifs, np.array(offs, np.int64)


def merge_ref(windows, run, chrom_size, step, m, join, min_windows):
    """Rule 6 over the called windows of one run (in position order): ``(hotspots, kept, dropped, bases)``."""
    out, dropped, bases, covered_to = [], 0, 0, 0
    rows = windows[["pos", "ifs", "count", "bg1", "nb1"]].tolist()  # (plain integers: the loop below is plain Python)
    group = []

    def close():
        nonlocal dropped, bases, covered_to
        if not group:
            return
        if len(group) < min_windows:
            dropped += 1
        else:
            best = group[0]
            for w in group[1:]:
                if w[1] < best[1]:  # the smallest I, the leftmost of equals
                    best = w
            start = group[0][0]
            stop = min((group[-1][0] // step + m) * step, chrom_size)
            out.append((run, start, stop, len(group)) + best)
            bases += stop - max(start, covered_to)
            covered_to = stop
        group.clear()
    for w in rows:
        if group and (w[0] - group[-1][0]) // step > join:
            close()
        group.append(w)
    close()
    return np.array(out, HOTSPOT_DTYPE), len(out), dropped, bases


def ifs_hotspots_ref(start, end, mapq, starts, stops, chrom_size, step=20, m=10, mean_length=167, h1=125, h2=250, min_count=0,
                     thresholds=None, global_mean=0, join=None, min_windows=1, min_length=None, max_length=None,
                     quality_threshold=30, tracks=None):
    """``(windows, hotspots, stats)`` as ``Engine.ifs_hotspots`` returns them.  ``tracks``: the ``bin_tracks`` of these very
    arguments, computed once by a caller that asks many times."""
    L = int(mean_length)
    thr = np.asarray(thresholds, np.uint64)
    if join is None:
        join = max(m + 200 // step, 1)
    c, i = tracks if tracks is not None else bin_tracks(start, end, mapq, chrom_size, step, L, min_length, max_length, quality_threshold)
    n, I = window_sums(c, m), window_sums(i, m)
    q = I // L
    tested = n >= min_count
    in_table = q < len(thr)
    t = np.where(in_table, thr[np.minimum(q, len(thr) - 1)], np.uint64(0)).astype(np.uint64)
    called = tested & in_table & (t != 0)
    if global_mean:
        called &= t <= np.uint64(global_mean)
    B1, nb1 = backgrounds(i, m, h1)
    B2, nb2 = backgrounds(i, m, h2) if h2 else (np.zeros_like(B1), np.zeros_like(nb1))
    for B, nb in ((B1, nb1), (B2, nb2))[:2 if h2 else 1]:
        called &= (B.astype(np.uint64) * np.uint64(m) << SHIFT) >= t * nb.astype(np.uint64) * np.uint64(L)
    stats = np.zeros((len(starts), 6), np.int64)
    win_parts, hot_parts = [], []
    for r, (a, b) in enumerate(zip(starts, stops)):
        k_lo, k_hi = interval_windows(int(a), int(b), chrom_size, step, m)
        if k_hi < k_lo:
            continue
        sl = slice(k_lo, k_hi + 1)
        k = np.flatnonzero(called[sl]) + k_lo
        part = np.zeros(len(k), WINDOW_DTYPE)
        part["run"], part["pos"], part["count"], part["ifs"] = r, k * step, n[k], I[k]
        part["bg1"], part["nb1"], part["bg2"], part["nb2"] = B1[k], nb1[k], B2[k], nb2[k]
        hot, kept, dropped, bases = merge_ref(part, r, chrom_size, step, m, join, min_windows)
        stats[r] = [k_hi - k_lo + 1, tested[sl].sum(), len(k), kept, dropped, bases]
        win_parts.append(part)
        hot_parts.append(hot)
    windows = np.concatenate(win_parts) if win_parts else np.zeros(0, WINDOW_DTYPE)
    hotspots = np.concatenate(hot_parts) if hot_parts else np.zeros(0, HOTSPOT_DTYPE)
    return windows, hotspots, stats


def same_records(got, want):
    """Equal integers, field by field."""
    if got.shape != want.shape or got.dtype.names != want.dtype.names:
        return False
    return all(np.array_equal(np.asarray(got[f]).astype(want.dtype[f]), want[f]) for f in want.dtype.names)


def flat_table(t, n=8):
    """``thr[q] = t`` for every ``q < n``: a tested window with ``q < n`` is called iff every background's mean IFS per
    window is at least ``t / 1024`` (and ``t <= global_mean``)."""
    return np.full(n, int(t), np.uint64)


def random_fragments(rng, chrom_size, depth, mean=167.0, sd=25.0):
    """Start-sorted ``(start, end, mapq)`` of about ``depth`` x coverage: lengths ~N(mean, sd), at least 1; mapq 60, one in
    eight 10; fragments may reach beyond the contig."""
    n = max(int(depth * chrom_size / mean), 1)
    start = np.sort(rng.integers(0, max(chrom_size, 1), n)).astype(np.int32)
    length = np.maximum(np.rint(rng.normal(mean, sd, n)), 1).astype(np.int32)
    mapq = np.where(rng.integers(0, 8, n) == 0, 10, 60).astype(np.uint8)
    return start, (start + length).astype(np.int32), mapq


def planted_fragments():
    """The planted case: 30x on 400 000 bases with nine fragments in ten removed within 300 bases of three centres."""
    chrom_size, centres = 400_000, (100_000, 200_000, 300_000)
    rng = np.random.default_rng(1)
    n = int(30 * chrom_size / 167)
    start = np.sort(rng.integers(0, chrom_size, n)).astype(np.int64)
    length = np.maximum(np.rint(rng.normal(167, 25, n)), 1).astype(np.int64)
    drop = rng.random(n) < 0.9
    mid = (start + start + length) >> 1
    near = np.zeros(n, bool)
    for c in centres:
        near |= np.abs(mid - c) <= 300
    keep = ~(near & drop)
    start, length = start[keep], length[keep]
    return chrom_size, centres, (start, start + length, np.full(len(start), 60, np.int64))


# ---- what the GPU tests share: a resident contig held against the restatement, and fragments built by hand ----------------
def assert_same(got, want, what=None):
    assert np.array_equal(got[2], want[2]), (what, got[2].tolist(), want[2].tolist())
    assert got[0].dtype == WINDOW_DTYPE and same_records(got[0], want[0]), (what, "windows", len(got[0]), len(want[0]))
    assert got[1].dtype == HOTSPOT_DTYPE and same_records(got[1], want[1]), (what, "hotspots", got[1].tolist()[:5], want[1].tolist()[:5])


class Contig:
    """A contig of the engine's for the length of a ``with`` block."""

    def __init__(self, engine, start, end, mapq, read1=False, name="ifs:case"):
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

    def both(self, starts, stops, size, what=None, tracks=None, **kw):
        """The engine's hotspots, held against the restatement's."""
        starts, stops = np.asarray(starts, np.int64), np.asarray(stops, np.int64)
        got = self.engine.ifs_hotspots(self.name, starts, stops, size, **kw)
        assert_same(got, ifs_hotspots_ref(*self.cols, starts, stops, size, tracks=tracks, **kw), what)
        return got

    def track(self, starts, stops, size, what=None, **kw):
        """The engine's per-window track, on the host and on the device, held against the restatement's."""
        starts, stops = np.asarray(starts, np.int64), np.asarray(stops, np.int64)
        n, ifs, offs = self.engine.ifs_track(self.name, starts, stops, size, **kw)
        want = ifs_track_ref(*self.cols, starts, stops, size, **kw)
        assert n.dtype == np.int32 and ifs.dtype == np.int64 and np.array_equal(offs, want[2]), (what, offs, want[2])
        assert np.array_equal(n, want[0]) and np.array_equal(ifs, want[1]), what
        dn, di, _ = self.engine.ifs_track(self.name, starts, stops, size, device=True, **kw)
        assert np.array_equal(dn.cpu().numpy(), want[0]) and np.array_equal(di.cpu().numpy(), want[1]), what
        return n, ifs, offs


def columns(*pairs):
    s = np.concatenate([np.atleast_1d(np.asarray(a, np.int64)) for a, _ in pairs])
    e = np.concatenate([np.atleast_1d(np.asarray(b, np.int64)) for _, b in pairs])
    return s, e, np.full(len(s), 60, np.int64)


def at(mids, length=10, copies=1):
    """Fragments of ``length`` (even) bases with their midpoints on ``mids``."""
    m = np.repeat(np.asarray(mids, np.int64), copies)
    return m - length // 2, m + length // 2
