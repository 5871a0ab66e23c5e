"""
The contigs and calls of tests/test_gpu_delta_column.py, and the child process that runs them on the GPU.

    python tests/delta_column_child.py OUT.npz

runs every call on every contig of CONTIGS in THIS process - whose environment decides the path: FTK_PACKED unset reads
the start deltas and the packed (length, mapq) words (ContigView::ds, gbase, lq; csrc/ftk_packed.h), FTK_PACKED=0 the
wide columns - and stores every output, with the packed-launch counter's step per call, in OUT.npz.  The test module
imports the same definitions for its oracle.  Not a test module itself.

The contigs are hand-made: a few hundred to a few thousand fragments each, placed so that the decode of the delta columns
meets every edge it has (groups of 64 fragments, deltas of 255 / 256, candidate bounds anywhere in a group, the padding
group behind the last fragment, chunks of 1 024 candidates per WPS tile, 4 096 per pass of a feature block).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TOP = 1 << 30
WS = (120, 121)                 # even and odd W
WMIN, WMAX, Q = 120, 180, 30
HIST = (0, 1001)


def _columns(start):
    """end and mapq for hand-placed starts: lengths 100 .. 230 (both sides of WMIN, WMAX and DELFI's 100 / 150 / 220),
    mapqs on both sides of Q."""
    start = np.asarray(start, np.int64)
    i = np.arange(len(start))
    length = 100 + (i * 37 + 50) % 131
    mapq = np.where(i % 5 == 2, (i * 7) % 30, 60)
    return start.astype(np.int32), (start + length).astype(np.int32), mapq.astype(np.uint8)


def _steps(n, step, first=1000, gaps=()):
    """n starts `step` apart; gaps: (index, delta) pairs that replace the delta in front of fragment `index`."""
    d = np.full(n, step, np.int64)
    if n:
        d[0] = first
    for at, gap in gaps:
        d[at] = gap
    return np.cumsum(d)


def _spec(start, size, windows, wps, intervals=None):
    s, e, q = _columns(start)
    assert len(s) == 0 or int(e.max()) < min(size + 1, TOP)
    ws = np.array([w[0] for w in windows], np.int32)
    we = np.array([w[1] for w in windows], np.int32)
    return dict(start=s, end=e, mapq=q, size=size, ws=ws, we=we, wps=wps, intervals=intervals)


def make_contig(name):
    """-> dict(start, end, mapq, size, ws, we, wps=(a, b), intervals=[(a, b), ...] or None)"""
    if name.startswith("n"):
        # 1, 63, 64, 65, 200 fragments; the window and the interval reach the contig's end, so the range ends in the
        # group that holds the padding (n = 64: ends with a whole group)
        n = int(name[1:])
        size = 1000 + 7 * n + 400
        return _spec(_steps(n, 7), size, [(0, 900), (900, size)], (0, size))
    if name == "same":
        # 80 fragments with one start, indices 40 .. 119: the run straddles the boundary between groups 0 and 1
        start = np.concatenate([_steps(40, 5), np.full(80, 1000 + 39 * 5 + 3), 1000 + 39 * 5 + 3 + _steps(60, 4, first=4)])
        return _spec(start, 3000, [(0, 1200), (1200, 3000)], (0, 3000))
    if name == "gaps":
        # group 0 holds a gap of 255 (kept), group 1 one of 256 (flagged); a gap of 100 000 in front of fragment 128, a
        # group's first (not flagged); group 3 flagged again, group 4 not: flagged and unflagged groups share the first
        # wave of a feature block (fragments 0 .. 255) and a WPS tile; behind the gap a window that 20 fragments start in
        start = _steps(330, 3, gaps=[(10, 255), (84, 256), (128, 100_000), (200, 300)])
        far = int(start[128])
        size = far + 3000
        return _spec(start, size, [(0, 2400), (far - 500, far + 60), (far + 60, size)], (137, 5000),
                     intervals=[(137, 5000), (5003, 5700), (far - 4097, far + 1500)])
    if name == "top":
        # the same shapes just below 2^30: 1 000 fragments about 30 apart, a gap of 256 inside a group, one of 255
        # inside another and one of 4 000 in front of a group's first fragment
        start = _steps(1000, 29, first=TOP - 50_000, gaps=[(70, 256), (300, 255), (640, 4000)])
        size = TOP - 1
        return _spec(start, size, [(TOP - 60_000, TOP - 40_000), (TOP - 40_000, TOP - 20_000), (TOP - 20_000, size)],
                     (TOP - 50_500, TOP - 38_000), intervals=[(TOP - 30_001, TOP - 17_000), (TOP - 9_000, size)])
    if name.startswith("b"):
        # starts 8 apart: bin k of the 512-base position index begins at fragment 64 k - off, so every candidate bound of
        # a window or a tile falls on a group's first fragment (off = 0), on its last (off = 1) or in its middle (32)
        off = int(name[1:])
        start = 8 * (np.arange(1500) + off)
        return _spec(start, 13_000, [(1024, 3072), (3072, 5000), (5000, 13_000)], (1500, 9000),
                     intervals=[(137, 5000), (5003, 5700), (7001, 12_000)])
    if name == "dense":
        # 5 000 fragments in 3 750 bases: one WPS tile holds five chunks of 1 024 candidates (the last one partly filled,
        # a flagged group in the third), one feature block walks its range in two passes of 4 096, and the stand-alone
        # feature launch picks its 512-thread blocks
        start = 1000 + (np.arange(5000) * 3) // 4
        start[2100:] += 300
        return _spec(start, 8192, [(0, 8192)], (0, 8192), intervals=[(1, 4097), (4099, 6000)])
    raise KeyError(name)


CONTIGS = ("n1", "n63", "n64", "n65", "n200", "same", "gaps", "top", "b0", "b1", "b32", "dense")
BL = (np.array([1100, 2000], np.int32), np.array([1150, 2300], np.int32))
GAPS = (3000, 3100, [(0, 500)])


def run_contig(eng, name, out):
    import ctypes as C
    c = make_contig(name)
    eng.load_contig(name, c["start"], c["end"], c["mapq"])
    lib = eng.lib

    def launches():
        v = C.c_int64()
        eng._check(lib.ftk_frags_packed(eng.ctx, eng.contig_id(name), None, None, C.byref(v)))
        return int(v.value)

    present = C.c_int32(-1)
    eng._check(lib.ftk_frags_packed(eng.ctx, eng.contig_id(name), C.byref(present), None, None))
    out[f"{name}/present"] = np.array([present.value], np.int64)
    ws, we, n = c["ws"], c["we"], len(c["ws"])
    a, b = c["wps"]
    for W in WS:
        key = f"{name}/{W}/"
        steps = []
        m = dict(coverage=np.full(n, -7, np.int64), hist=np.full((n, HIST[1]), 9, np.uint32),
                 overflow=np.full(n, -7, np.int64), short=np.full(n, -7, np.int64), long=np.full(n, -7, np.int64))
        w = np.full(b - a, -99, np.int64)
        t = launches()
        eng.window_features_wps(name, ws, we, w, a, b, c["size"], Q, coverage=m["coverage"], hist=m["hist"],
                                hist_bins=HIST, overflow=m["overflow"], delfi_q=Q, bl_start=BL[0], bl_end=BL[1],
                                gaps=GAPS, short=m["short"], long=m["long"], window_size=W, wps_min_length=WMIN,
                                wps_max_length=WMAX, wps_quality=Q)
        steps.append(launches() - t)
        for k, v in m.items():
            out[f"{key}merged_{k}"] = v
        out[f"{key}merged_wps"] = w
        t = launches()
        f = eng.window_features(name, ws, we, Q, hist=HIST,
                                delfi=dict(quality_threshold=Q, bl_start=BL[0], bl_end=BL[1], gaps=GAPS))
        steps.append(launches() - t)
        for k, v in f.items():
            out[f"{key}feat_{k}"] = v
        t = launches()
        out[f"{key}wps"] = np.array(eng.wps(name, a, b, c["size"], W, WMIN, WMAX, Q))
        steps.append(launches() - t)
        if c["intervals"]:
            t = launches()
            sc, _ = eng.wps_intervals(name, [i[0] for i in c["intervals"]], [i[1] for i in c["intervals"]], c["size"], W,
                                      WMIN, WMAX, Q)
            steps.append(launches() - t)
            out[f"{key}intervals"] = np.array(sc)
        out[f"{key}steps"] = np.array(steps, np.int64)


def main(path):
    from finaletoolkit_amd.engine import Engine
    out = {}
    with Engine(0) as eng:
        for name in CONTIGS:
            run_contig(eng, name, out)
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
