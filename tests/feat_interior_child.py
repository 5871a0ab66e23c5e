"""
The contigs and calls of tests/test_gpu_feat_interior.py, and the child process that runs them on the GPU.

    python tests/feat_interior_child.py OUT.npz

runs every case of CASES in THIS process - whose environment decides the path: by default a FAST feature block of a
packed launch takes coverage and the DELFI counts of an eligible window from its length histogram and reads only the
packed words of the window's interior (csrc/ftk_feat_interior.h); FTK_FEAT_INTERIOR=0 keeps the per-fragment counters,
FTK_PACKED=0 the wide columns - and stores every output in OUT.npz.  The test module imports the same definitions for
its oracle.  Not a test module itself.

The contigs are hand-made, a fragment per base or so over a few thousand bases, windows of 2-4 kb: every base is some
fragment's start, so every window has fragments that start at ws, at we - lmax - 1, we - lmax and we - lmax + 1.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

Q = 30
LENS = (0, 167, 100, 150, 99, 151, 220, 221, 1, 145, 230, 166, 0, 180)  # both sides of 100 / 150 / 151 / 220; zero length
MAPQ = (60, 30, 29, 31, 0, 42, 30, 60, 37, 32)                          # at the cut, below it, at 31 and above


def _contig(starts, lens=LENS):
    s = np.asarray(starts, np.int64)
    i = np.arange(len(s))
    ln = np.asarray(lens, np.int64)[i % len(lens)]
    q = np.asarray(MAPQ, np.int64)[i % len(MAPQ)]
    return s.astype(np.int32), (s + ln).astype(np.int32), q.astype(np.uint8)


def _case(starts, windows, lens=LENS, hist=(0, 1001), bl=None, gaps=None):
    s, e, q = _contig(starts, lens)
    size = int(e.max()) + 500 if len(s) else 5000
    ws = np.array([w[0] for w in windows], np.int32)
    we = np.array([min(w[1], size) for w in windows], np.int32)
    return dict(start=s, end=e, mapq=q, size=size, ws=ws, we=we, hist=hist, bl=bl, gaps=gaps)


def _every_base(n, first=0):
    return first + np.arange(n)


# windows on and off multiples of 512, ws = 0, one shorter than lmax + 512 (no interior), the last partial one
TILING = [(0, 2048), (2048, 4096), (4096, 6144), (6144, 8192), (8192, 12000)]
OFF = [(0, 3000), (137, 2900), (511, 2560), (512, 2561), (513, 4608), (1000, 1600), (2000, 2741), (2000, 2742), (2000, 2743),
       (5000, 9100), (7000, 20000)]


def make_case(name):
    """-> dict(start, end, mapq, size, ws, we, hist=(len_lo, n_bins) or None, bl=(starts, ends) or None, gaps or None)"""
    if name == "tiling":
        return _case(_every_base(9000), TILING)
    if name == "off":
        return _case(_every_base(9000), OFF)
    if name == "zero":  # every fragment has length zero: lmax = 0
        return _case(_every_base(6000), TILING[:3] + OFF[:6], lens=(0,))
    if name == "wide":  # a delta of 300 inside group 23, inside the interior of the first window: a wide-flagged group
        s = _every_base(6000)
        s[1500:] += 300
        return _case(s, [(0, 4096), (4096, 7000)])
    if name == "mixed":
        # windows 0, 2, 4 eligible; window 1 holds a blacklist interval; window 3 lies within reach of the centromere
        return _case(_every_base(9000), TILING, bl=(np.array([2500], np.int32), np.array([2700], np.int32)),
                     gaps=(7000, 7200, [(20000, 21000)]))
    if name == "len_lo":  # bins start above 100: the launch keeps the per-fragment counters
        return _case(_every_base(6000), TILING[:3], hist=(101, 1001))
    if name == "n_bins":  # bins end below 220: the same
        return _case(_every_base(6000), TILING[:3], hist=(0, 120))
    if name == "no_hist":  # no histogram requested: the same
        return _case(_every_base(6000), TILING[:3], hist=None)
    if name == "narrow":  # the narrowest histogram that still serves the counts: bins 100 .. 220 and the overflow bin
        return _case(_every_base(6000), TILING[:3], hist=(100, 121))
    if name == "deep":
        # eight fragments per base: the interior of the first window holds 28 672, more than one round of loads of a
        # 512-thread block (24 576) or of a 256-thread block (12 288); the second window's less than one
        return _case(np.repeat(_every_base(5200), 8), [(256, 4352), (4352, 5700)])
    if name == "empty":  # windows without a fragment, between and behind windows that hold some; we < ws; we = ws
        s = np.concatenate([_every_base(3000), _every_base(3000, 9000)])
        return _case(s, [(0, 3300), (3300, 6000), (6000, 8700), (8700, 12200), (12500, 12700), (2000, 1000), (1024, 1024)])
    raise KeyError(name)


CASES = ("tiling", "off", "zero", "wide", "mixed", "len_lo", "n_bins", "no_hist", "narrow", "deep", "empty")


def run_case(eng, name, out):
    c = make_case(name)
    eng.load_contig(name, c["start"], c["end"], c["mapq"])
    ws, we, n = c["ws"], c["we"], len(c["ws"])
    bl = c["bl"] or (None, None)
    key = f"{name}/"
    m = dict(coverage=np.full(n, -7, np.int64), short=np.full(n, -7, np.int64), long=np.full(n, -7, np.int64))
    if c["hist"]:
        m.update(hist=np.full((n, c["hist"][1]), 9, np.uint32), overflow=np.full(n, -7, np.int64))
    w = np.full(c["size"], -99, np.int64)
    eng.window_features_wps(name, ws, we, w, 0, c["size"], c["size"], Q, coverage=m["coverage"], hist=m.get("hist"),
                            hist_bins=c["hist"], overflow=m.get("overflow"), delfi_q=Q, bl_start=bl[0], bl_end=bl[1],
                            gaps=c["gaps"], short=m["short"], long=m["long"])
    for k, v in m.items():
        out[f"{key}merged_{k}"] = v
    out[f"{key}merged_wps"] = w
    f = eng.window_features(name, ws, we, Q, hist=c["hist"],
                            delfi=dict(quality_threshold=Q, bl_start=bl[0], bl_end=bl[1], gaps=c["gaps"]))
    for k, v in f.items():
        out[f"{key}feat_{k}"] = v
    # coverage and histogram without DELFI: the same rule serves the launch
    f = eng.window_features(name, ws, we, Q, hist=c["hist"])
    for k, v in f.items():
        out[f"{key}cov_{k}"] = v


def main(path):
    from finaletoolkit_amd.engine import Engine
    out = {}
    with Engine(0) as eng:
        for name in CASES:
            run_case(eng, name, out)
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
