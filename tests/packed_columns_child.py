"""
The contigs and calls of tests/test_gpu_packed_columns.py, and the child process that runs them on the GPU.

    python tests/packed_columns_child.py OUT.npz

runs every call of CASES on every contig of CONTIGS (plus the reload sequence) in THIS process - whose environment
decides the path: FTK_PACKED unset reads the packed (length, mapq) column where the rule allows it, FTK_PACKED=0 never
does - and stores every output, with the packed-launch counter's step per call, in OUT.npz.  The test module imports the
same definitions for its oracle.  Not a test module itself.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZE = 300_000                  # 3 windows x 100 kb
WIN = 100_000
EMPTY = (147_000, 165_000)      # no fragment starts here: the WPS tiles inside have no candidates
LEN_MAX = 2046                  # longest packable length (11 bits, 2047 = saturated)
Q_SAT = 31                      # largest exact mapq threshold (5 bits)
SPECIAL_LENS = [0, 1, 119, 120, 121, 150, 151, 220, 221, 1000, 1001, LEN_MAX]  # W - 1, W for W = 120 and 121
SPECIAL_Q = [0, 19, 20, 29, 30, Q_SAT, Q_SAT + 1, 60, 255]                    # threshold - 1, threshold; 2^B - 1, 2^B
BL_START = np.array([10_000, 99_900, 120_000, 250_000], np.int32)
BL_END = np.array([10_500, 100_200, 120_050, 251_000], np.int32)
GAPS = (130_000, 140_000, [(0, 5_000), (SIZE - 5_000, SIZE)])
A0 = 4097                       # an interval that does not start at 0 ...
B0 = A0 + 69 * 4096 + 1234      # ... of 70 tiles, the last one 1234 bases


def make_contig(kind):
    """Start-sorted columns.  'main': ~9 000 mixture fragments + every special length x special mapq three times
    (max length LEN_MAX); 'long': 'main' and ONE fragment of LEN_MAX + 1; 'other': an unrelated contig of ~14 000, dense
    enough that the stand-alone feature pass picks its 512-thread blocks (expected_candidates), where 'main' runs 256."""
    seed, n = {"main": (11, 9000), "long": (11, 9000), "other": (12, 15000)}[kind]
    rng = np.random.default_rng(seed)
    start = rng.integers(0, SIZE - 2100, n)
    u = rng.random(n)
    length = np.where(u < 0.8, rng.normal(167, 12, n), np.where(u < 0.95, rng.normal(334, 25, n), rng.uniform(30, 1000, n)))
    length = np.clip(np.rint(length), 30, 1000).astype(np.int64)
    mapq = np.where(rng.random(n) < 0.7, 60, rng.integers(0, 61, n))
    if kind != "other":
        ls, qs = np.meshgrid(SPECIAL_LENS, SPECIAL_Q)
        ls, qs = np.tile(ls.ravel(), 3), np.tile(qs.ravel(), 3)
        start = np.concatenate([start, rng.integers(0, SIZE - 2100, len(ls))])
        length = np.concatenate([length, ls])
        mapq = np.concatenate([mapq, qs])
    if kind == "long":
        start = np.concatenate([start, [50_000]])
        length = np.concatenate([length, [LEN_MAX + 1]])
        mapq = np.concatenate([mapq, [60]])
    keep = (start < EMPTY[0]) | (start >= EMPTY[1])
    start, length, mapq = start[keep], length[keep], mapq[keep]
    end = start + length
    order = np.lexsort((end, start))
    return start[order].astype(np.int32), end[order].astype(np.int32), mapq[order].astype(np.uint8)


CONTIGS = ("main", "long", "other")


def expected_candidates(start, end, lmax):
    """The library's estimate of the candidates per window (features_common: mean density x (window + longest admissible
    fragment)): 4096 or more picks feat_fast_kernel<512>, less feat_fast_kernel<256>."""
    return len(start) / float(end.max()) * (WIN + lmax)


# q: the coverage / histogram / DELFI mapq cut; hist: (len_lo, n_bins); W, wmin, wmax, wq: the WPS call; a, b: its
# interval.  feat / wps: may the feature blocks / the WPS tiles of this call read the packed column (on a contig that has
# it)?  The merged launch may when both may.
CASES = [
    dict(q=30, hist=(0, 1001), W=120, wmin=120, wmax=180, wq=30, a=A0, b=B0, feat=True, wps=True),
    dict(q=Q_SAT, hist=(1000, 1047), W=121, wmin=0, wmax=LEN_MAX, wq=Q_SAT, a=0, b=SIZE, feat=True, wps=True),  # every bound at its limit
    dict(q=20, hist=(0, 640), W=60, wmin=1, wmax=1001, wq=20, a=A0, b=B0, feat=True, wps=True),
    dict(q=Q_SAT + 1, hist=(0, 1001), W=120, wmin=120, wmax=180, wq=Q_SAT + 1, a=A0, b=B0, feat=False, wps=False),  # threshold 2^B
    dict(q=60, hist=(0, 1001), W=121, wmin=120, wmax=180, wq=255, a=0, b=SIZE, feat=False, wps=False),
    dict(q=30, hist=(1000, 1048), W=120, wmin=120, wmax=180, wq=30, a=A0, b=B0, feat=False, wps=True),  # histogram edge 2048
    dict(q=30, hist=(0, 1001), W=120, wmin=120, wmax=LEN_MAX + 1, wq=30, a=A0, b=B0, feat=True, wps=False),  # WPS max_len at saturation
    dict(q=30, hist=(0, 1001), W=121, wmin=0, wmax=5000, wq=30, a=0, b=SIZE, feat=True, wps=False),
]
# the reload sequence under ONE contig id: (contig, release before loading?)
RELOADS = [("main", False), ("other", True), ("long", False), ("other", False), ("main", True)]


def windows():
    ws = np.arange(0, SIZE, WIN, dtype=np.int32)
    return ws, np.minimum(ws + WIN, SIZE).astype(np.int32)


def run_case(eng, name, c, out, key):
    """The three entry points of one case; out[key + ...] = every result, out[key + 'steps'] = the packed-launch
    counter's step over each call (merged, features, wps)."""
    import ctypes as C
    lib = eng.lib
    ws, we = windows()
    n = len(ws)

    def launches():
        v = C.c_int64()
        eng._check(lib.ftk_frags_packed(eng.ctx, eng.contig_id(name), None, None, C.byref(v)))
        return int(v.value)

    steps = []
    lo, nb = c["hist"]
    m = dict(coverage=np.full(n, -7, np.int64), hist=np.full((n, nb), 9, np.uint32), overflow=np.full(n, -7, np.int64),
             short=np.full(n, -7, np.int64), long=np.full(n, -7, np.int64))
    w = np.full(c["b"] - c["a"], -99, np.int64)
    t = launches()
    eng.window_features_wps(name, ws, we, w, c["a"], c["b"], SIZE, c["q"], coverage=m["coverage"], hist=m["hist"],
                            hist_bins=c["hist"], overflow=m["overflow"], delfi_q=c["q"], bl_start=BL_START, bl_end=BL_END,
                            gaps=GAPS, short=m["short"], long=m["long"], window_size=c["W"], wps_min_length=c["wmin"],
                            wps_max_length=c["wmax"], wps_quality=c["wq"])
    steps.append(launches() - t)
    for k, v in m.items():
        out[f"{key}merged_{k}"] = v
    out[f"{key}merged_wps"] = w
    t = launches()
    f = eng.window_features(name, ws, we, c["q"], hist=c["hist"],
                            delfi=dict(quality_threshold=c["q"], bl_start=BL_START, bl_end=BL_END, gaps=GAPS))
    steps.append(launches() - t)
    for k, v in f.items():
        out[f"{key}feat_{k}"] = v
    t = launches()
    out[f"{key}wps"] = np.array(eng.wps(name, c["a"], c["b"], SIZE, c["W"], c["wmin"], c["wmax"], c["wq"]))
    steps.append(launches() - t)
    out[f"{key}steps"] = np.array(steps, np.int64)


def main(path):
    import ctypes as C
    from finaletoolkit_amd.engine import Engine
    out = {}
    with Engine(0) as eng:
        for name in CONTIGS:
            s, e, q = make_contig(name)
            eng.load_contig(name, s, e, q)
            present, len_max = C.c_int32(-1), C.c_int32(-1)
            eng._check(eng.lib.ftk_frags_packed(eng.ctx, eng.contig_id(name), C.byref(present), C.byref(len_max), None))
            out[f"{name}/present"] = np.array([present.value, len_max.value], np.int64)
            for i, c in enumerate(CASES):
                run_case(eng, name, c, out, f"{name}/{i}/")
        for k, (kind, release) in enumerate(RELOADS):
            if release:  # the id stays the name's: the next load puts another contig under it
                eng._check(eng.lib.ftk_frags_release(eng.ctx, eng.contig_id("re")))
            s, e, q = make_contig(kind)
            eng.load_contig("re", s, e, q)
            run_case(eng, "re", CASES[0], out, f"re/{k}/")
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
