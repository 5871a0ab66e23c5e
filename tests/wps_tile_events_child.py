"""
The contigs and calls of tests/test_gpu_wps_tile_events.py, and the child process that runs them on the GPU.

    python tests/wps_tile_events_child.py OUT.npz

runs every call of CALLS on every contig of CONTIGS in THIS process - whose environment decides the path: FTK_PACKED
unset reads the packed columns where the call allows it, FTK_PACKED=0 the wide ones - through ftk_window_features_wps,
ftk_wps and ftk_wps_intervals, and stores the scores in OUT.npz.  The test module imports the same definitions for its
oracle.  Not a test module itself.

The contigs are hand-made: a few thousand fragments over five tiles of 4 096 bases, placed so that the events of a
fragment in a tile's difference array (csrc/ftk_wps_events.h) meet every edge they have.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TOP = 1 << 30
T = 4096
UNBOUNDED = 1 << 28  # the largest max_len a WPS call takes: no length reaches it (such a call reads the wide columns)
# (window_size, min_len, max_len, mapq_min): even and odd W; thresholds 0, 30 and 31; a window far wider than max_len,
# where the fetch window [start - max_len, stop + max_len) - and on a BAM contig read1 - decides for fragments that
# still reach the interval, and where the first tiles of an interval are edge tiles and the next ones interior
CALLS = ((120, 100, 180, 30), (121, 100, 180, 31), (120, 0, UNBOUNDED, 0), (1000, 100, 180, 30), (1001, 0, 2046, 1))
LENS = (99, 100, 101, 110, 119, 120, 121, 122, 150, 179, 180, 181)  # min_len, max_len +- 1; W - 1, W, W + 1; below W
MAPQS = (0, 1, 29, 30, 31, 32, 60)
A, B, SIZE = 5000, 5000 + 4 * T + 2616, 40_000  # the unit: starts behind 0, a partial fifth tile, stops short of the contig


def _halves(W):
    return (W // 2, W // 2) if W & 1 else (W // 2, W // 2 - 1)  # hl, hr


def _edge_fragments(bounds, top=TOP):
    """(start, length) pairs whose events a, b, c, e land on b - 1 and b of every bound b, for every window in CALLS:
    on -1 and 0 of the tile that begins there, on T - 1 and T (or len_t - 1, len_t) of the one that ends there."""
    out = []
    for W in sorted({c[0] for c in CALLS}):
        hl, hr = _halves(W)
        for b in bounds:
            for v in (b - 1, b):
                for length in (119, 120, 121, 150, 180, W + 1 if W < 200 else 179):
                    out += [(v + hr, length), (v - hl - 1, length), (v + hr - length, length), (v - hl - 1 - length, length)]
    return [(s, n) for s, n in out if s >= 0 and s + n < top]


def _window_fragments(lo, hi):
    """fragments whose start, midpoint and end sit at lo - 1, lo, lo + 1 and hi - 1, hi, hi + 1"""
    out = []
    for x in (lo, hi):
        for d in (-1, 0, 1):
            for length in (100, 101, 150, 180):
                out += [(x + d, length), (x + d - length // 2, length), (x + d - length, length)]
    return [(s, n) for s, n in out if s >= 0]


def _finish(pairs, size, wps, intervals, bam=False, seed=1):
    pairs = sorted(set(pairs))
    start = np.array([p[0] for p in pairs], np.int64)
    length = np.array([p[1] for p in pairs], np.int64)
    order = np.argsort(start, kind="stable")
    start, length = start[order], length[order]
    i = np.arange(len(start))
    mapq = np.array(MAPQS, np.uint8)[(i * 5 + 3) % len(MAPQS)]
    end = start + length
    assert start.min() >= 0 and end.max() <= min(size, TOP - 1)
    c = dict(start=start.astype(np.int32), end=end.astype(np.int32), mapq=mapq, size=size, wps=wps, intervals=intervals,
             r1_start=None, r1_end=None)
    if bam:  # read1 is the fragment's first 50 bases (even fragments) or its last 50 (odd ones): inside its span
        first = i % 2 == 0
        c["r1_start"] = np.where(first, start, np.maximum(start, end - 50)).astype(np.int32)
        c["r1_end"] = np.where(first, np.minimum(end, start + 50), end).astype(np.int32)
    return c


def make_contig(name):
    """-> dict(start, end, mapq, size, wps=(a, b), intervals=[(a, b), ...], r1_start, r1_end)"""
    rng = np.random.default_rng(7)
    if name in ("tiles", "bam"):
        t0 = [A + k * T for k in range(5)]
        pairs = _edge_fragments([t0[0], t0[1], t0[2], B])
        # the fetch windows of the calls: [A - max_len, B + max_len) for max_len 180 and 2046
        for m in (180, 2046):
            pairs += _window_fragments(A - m, B + m)
        # tile 1: more than 1 024 candidates (the tail loop behind the four slots), every length and mapq
        pairs += [(t0[1] + 300 + 2 * i, LENS[i % len(LENS)]) for i in range(1500)]
        # a sprinkle over tiles 0 - 2 and 4, straddling the boundaries between them too; lengths up to the column's limit
        pairs += [(int(s), int(n)) for s, n in zip(rng.integers(1000, t0[3] - 2700, 900), rng.integers(90, 200, 900))]
        pairs += [(int(s), int(n)) for s, n in zip(rng.integers(t0[4] + 1012, SIZE - 2100, 500), rng.integers(90, 200, 500))]
        pairs += [(100, 2046), (t0[1] - 1000, 2046), (t0[2] - 2046, 2045), (0, 0), (0, 100), (SIZE - 100, 100)]
        # tile 3 keeps no candidate in the bounded calls: nothing starts in [t0[3] - 1 - 500 - 180 - 512, t0[4] + 500 + 512)
        pairs = [p for p in pairs if not t0[3] - 1200 <= p[0] < t0[4] + 1012]
        ivs = [(137, 5000), (5003, 5700), (A + 77, A + 2 * T + 78), (t0[4] + 1100, SIZE)]
        return _finish(pairs, SIZE, (A, B), ivs, bam=name == "bam")
    if name == "long":
        # fragments that straddle two tile boundaries (longer than a tile: the contig keeps no packed column)
        pairs = [(A + T - 500, 5000), (A - 300, 9000), (A + T - 1, T + 2), (A + 2 * T - 60, 120)]
        pairs += [(int(s), int(n)) for s, n in zip(rng.integers(3000, 20_000, 300), rng.integers(90, 200, 300))]
        return _finish(pairs, SIZE, (A, A + 3 * T + 5), [(A + 1, A + T + 3), (A + T + 9, A + 3 * T)])
    if name == "top":
        # the same edges just below 2^30: the last fragments end at 2^30 - 1, the last tile at the contig's end
        size = TOP - 1
        a = size - 2 * T - 1000
        pairs = _edge_fragments([a, a + T, a + 2 * T], top=TOP)
        pairs += [(size - n, n) for n in LENS] + [(size - n - 1, n) for n in LENS]
        pairs += [(int(s), int(n)) for s, n in zip(rng.integers(a - 3000, size - 200, 1500), rng.integers(90, 200, 1500))]
        pairs = [(s, n) for s, n in pairs if s + n <= size]
        return _finish(pairs, size, (a, size), [(a + 5, a + T + 6), (size - 3000, size)])
    raise KeyError(name)


CONTIGS = ("tiles", "bam", "long", "top")


def run_contig(eng, name, out):
    c = make_contig(name)
    eng.load_contig(name, c["start"], c["end"], c["mapq"], None, c["r1_start"], c["r1_end"])
    a, b = c["wps"]
    ws = np.array([0, c["size"] // 2], np.int32) if name != "top" else np.array([a - 5000, a + T], np.int32)
    we = np.array([c["size"] // 2, c["size"]], np.int32) if name != "top" else np.array([a + T, c["size"]], np.int32)
    for k, (W, mn, mx, q) in enumerate(CALLS):
        key = f"{name}/{k}/"
        w = np.full(b - a, -99, np.int64)
        cov = np.full(len(ws), -7, np.int64)
        eng.window_features_wps(name, ws, we, w, a, b, c["size"], 30, coverage=cov, window_size=W, wps_min_length=mn,
                                wps_max_length=mx, wps_quality=q)
        out[key + "merged"] = w
        out[key + "wps"] = np.array(eng.wps(name, a, b, c["size"], W, mn, mx, q))
        sc, _ = eng.wps_intervals(name, [i[0] for i in c["intervals"]], [i[1] for i in c["intervals"]], c["size"], W, mn, mx, q)
        out[key + "intervals"] = np.array(sc)


def main(path):
    import ctypes as C

    from finaletoolkit_amd.engine import Engine
    out = {}
    with Engine(0) as eng:
        for name in CONTIGS:
            run_contig(eng, name, out)
            present, launches = C.c_int32(-1), C.c_int64()
            eng._check(eng.lib.ftk_frags_packed(eng.ctx, eng.contig_id(name), C.byref(present), None, C.byref(launches)))
            out[f"{name}/present"] = np.array([present.value], np.int64)
            out[f"{name}/launches"] = np.array([launches.value], np.int64)  # packed launches of the process so far
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
