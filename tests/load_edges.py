"""Seeded worlds for what a contig load decides on the device (csrc/ftk_api.hip: upload_common, ftk_frags_set_read1):
the validation and summary of ``stats_kernel``, the 512-bp position index of ``bin_index_kernel`` and the read-1 flag of
``r1_inside_kernel``.  One offender, one long fragment or one outlier at a time, at the lane, wave, block and grid-stride
edges of the launches.  Not a test module: ``tests/test_load_edges.py`` asserts that the worlds hold every case (CPU),
``tests/test_gpu_load_edges.py`` loads them.  numpy only; expected values come from ``oracle.oracle`` or plain numpy."""
import functools

import numpy as np

from oracle import oracle as O

# The launch shapes the positions below are laid out for.  If a cap changes, the positions must follow:
# csrc/ftk_kernels.hip, launch_stats (min(1024, ..) blocks of kStatsThreads) and launch_r1_inside (min(2048, ..) of 256).
STATS_BLOCKS, STATS_THREADS = 1024, 256
R1_BLOCKS, R1_THREADS = 2048, 256
CAP_STATS = STATS_BLOCKS * STATS_THREADS      # 262 144: fragment CAP_STATS is thread 0's second grid-stride trip
CAP_R1 = R1_BLOCKS * R1_THREADS               # 524 288
N_STATS = CAP_STATS + 1_000
N_R1 = CAP_R1 + 1_000
POS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, CAP_STATS - 1, CAP_STATS, CAP_STATS + 1, N_STATS - 1)
R1_POS = (0, 63, 64, 255, 256, CAP_R1 - 1, CAP_R1, N_R1 - 1)

BIN = 512                 # kBinShift = 9
LIMIT = 1 << 30           # coordinates must satisfy 0 <= start <= end < 2^30
LQ_LEN_MAX = 2046         # kLqLenMax (csrc/ftk_packed.h): the longest fragment of a contig that keeps the packed column
TILE = 4096               # kWpsTile: the per-base passes work in tiles of this many bases
FIRST_START = 10_000
LONG = 150_000
R1_LEN = 60
R1_SHIFT = 5_000
ERR_INVALID, ERR_NO_CONTIG, ERR_UNSORTED = -1, -7, -8

SIZES = (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025) + tuple(range(CAP_STATS - 4, CAP_STATS + 5))


def background(n, seed):
    """Sorted starts from 10 000 with gaps of 15-25 and a few ties, lengths 100-200, random mapq and strand."""
    rng = np.random.default_rng(seed)
    gap = rng.integers(15, 26, n)
    gap[rng.integers(1, n, max(n // 500, 1))] = 0
    gap[0] = 0
    fs = FIRST_START + np.cumsum(gap)
    fe = fs + rng.integers(100, 201, n)
    cols = (fs.astype(np.int32), fe.astype(np.int32), rng.integers(0, 61, n).astype(np.uint8),
            rng.integers(0, 2, n).astype(np.uint8))
    for c in cols:
        c.setflags(write=False)   # shared among the tests: every variant below works on copies
    return cols


@functools.lru_cache(maxsize=None)
def stats_world():
    return background(N_STATS, 20_261_019)


@functools.lru_cache(maxsize=None)
def r1_world():
    """``(fs, fe, mq, st, r1s, r1e)``: read 1 is the first (forward) or last (reverse) 60 bases - all spans inside."""
    fs, fe, mq, st = _copy(background(N_R1, 20_261_020))
    at = np.array(R1_POS)
    fe[at] = fs[at] + 150     # inside every length rule the calls apply (WPS 120-180, DELFI 100-220), mapq above any cut
    mq[at] = 60
    for c in (fs, fe, mq, st):
        c.setflags(write=False)
    r1s = np.where(st != 0, fs, fe - R1_LEN).astype(np.int32)
    r1e = (r1s + R1_LEN).astype(np.int32)
    r1s.setflags(write=False), r1e.setflags(write=False)
    return fs, fe, mq, st, r1s, r1e


def _copy(cols):
    return tuple(c.copy() for c in cols)


# ------------------------------------------------------------------------------------------ section 1: refusals
def unsorted_at(cols, i):
    """start[i] = start[i - 1] - 1, the end moved along: thread i alone sees disorder."""
    s, e, q, st = _copy(cols)
    d = s[i] - (s[i - 1] - 1)
    s[i] -= d
    e[i] -= d
    return s, e, q, st


def negative_at(cols, i):
    s, e, q, st = _copy(cols)
    e[i] = s[i] - 1
    return s, e, q, st


def end_at(cols, i, value):
    s, e, q, st = _copy(cols)
    e[i] = value
    return s, e, q, st


def start_at(cols, i, value):
    s, e, q, st = _copy(cols)
    s[i] = value
    return s, e, q, st


def all_equal(cols):
    s, e, q, st = _copy(cols)
    ln = e - s
    s[:] = s[0]
    return s, s + ln, q, st


def ties_at(cols, positions=POS):
    """Equal starts across every pair (i - 1, i)."""
    s, e, q, st = _copy(cols)
    for i in sorted(positions):
        d = s[i] - s[i - 1]
        s[i] -= d
        e[i] -= d
    return s, e, q, st


def summary(cols):
    """What ``ftk_frags_info`` reports: (n, max length, max end); an empty contig reports zeros."""
    s, e = cols[0].astype(np.int64), cols[1].astype(np.int64)
    return (len(s), int((e - s).max()), int(e.max())) if len(s) else (0, 0, 0)


# ------------------------------------------------------------------------------------------ section 2: the summary
def sized(n):
    """The first ``n`` fragments of the stats world with the longest fragment first (301) and the highest end last
    (250), so that both extremes sit on the edge threads of the launch."""
    s, e, q, st = (c[:n].copy() for c in stats_world())
    if n:
        e[n - 1] = s[n - 1] + 250
        e[0] = s[0] + 301
    return s, e, q, st


def long_at(cols, i, length=LONG):
    s, e, q, st = _copy(cols)
    e[i] = s[i] + length
    q[i] = 60
    return s, e, q, st


def long_windows(fs):
    """The windows of the long fragment at ``fs``: two it reaches, one that begins at its end."""
    return ([fs + LONG - 1_000, fs + LONG - 1, fs + LONG], [fs + LONG - 500, fs + LONG, fs + LONG + 100])


def long_interval(fs):
    return fs + LONG - 700, fs + LONG - 400


def restated_depth(cols, start, stop, mapq_min=0):
    s, e = cols[0].astype(np.int64), cols[1].astype(np.int64)
    m = (cols[2] >= mapq_min) & (e > start) & (s < stop)
    d = np.zeros(stop - start + 1, np.int64)
    np.add.at(d, np.maximum(s[m], start) - start, 1)
    np.add.at(d, np.minimum(e[m], stop) - start, -1)
    return np.cumsum(d[:-1]).astype(np.int32)


# ------------------------------------------------------------------------------------------ section 3: the index
INDEX_BINS = (255, 256, 257)
INDEX_FILTERS = (None, 1, 50, 600)
INDEX_Q = 10


def index_max_start(n_bins):
    return {255: 254 * BIN + 511, 256: 255 * BIN, 257: 256 * BIN}[n_bins]


def occupied_bins(n_bins):
    return (0, 1, 7, 8, n_bins - 2, n_bins - 1)


@functools.lru_cache(maxsize=None)
def index_world(n_bins):
    """A few thousand fragments whose starts sit at offsets 0, 1 and 511 of six bins, long runs of empty bins between;
    the last start makes ``n_bins`` exactly 255, 256 or 257.  Lengths 1-600 and one of 5 000.  At offset 0 of bins 7, 8
    and the last two lies a reverse-strand fragment of exactly 600 bases: the fragments whose end a cleavage tile that
    begins there can only find through ``bin_idx[k]`` itself (``index_cleavage_cases``).  The 5 000 one lies at 8 * 512."""
    rng = np.random.default_rng(1_000 + n_bins)
    top = index_max_start(n_bins)
    fs, ln, st = [], [], []
    for k in occupied_bins(n_bins):
        for d in (0, 1, 511):
            p = k * BIN + d
            if p > top:
                continue
            m = 150
            fs += [p] * m
            ln += [1, 600, 50, 51] + rng.integers(1, 601, m - 4).tolist()
            s_ = rng.integers(0, 2, m).tolist()
            s_[1] = 0
            st += s_
    fs.append(8 * BIN), ln.append(5_000), st.append(0)
    fs, ln, st = np.array(fs, np.int64), np.array(ln, np.int64), np.array(st, np.uint8)
    mq = rng.integers(0, 61, len(fs)).astype(np.uint8)
    mq[ln >= 600] = 60
    o = np.argsort(fs, kind="stable")
    return (fs[o].astype(np.int32), (fs + ln)[o].astype(np.int32), mq[o], st[o])


@functools.lru_cache(maxsize=None)
def index_windows(n_bins):
    """``(ws, we)`` as lists with None for an open end: every pair of the points k * 512 + d around the occupied bins,
    beyond the last bin and before 0, and both open ends."""
    ks = set()
    for k in occupied_bins(n_bins):
        ks |= {k - 1, k, k + 1}
    ks |= {n_bins, n_bins + 1, n_bins + 5}
    pts = sorted({k * BIN + d for k in ks for d in (-1, 0, 1)})
    ws, we = [], []
    for i, a in enumerate(pts):
        for b in pts[i + 1:]:
            ws.append(a), we.append(b)
    for p in pts:
        ws.append(None), we.append(p)
        ws.append(p), we.append(None)
    ws.append(None), we.append(None)
    return ws, we


def index_select_sample(n_bins):
    """200 window numbers: every window that lies within the last two bins (their points and the first beyond), the
    open-ended ones from there, and a seeded sample of the rest."""
    ws, we = index_windows(n_bins)
    lo = (n_bins - 2) * BIN - 1
    near = [i for i, (a, b) in enumerate(zip(ws, we))
            if (a is None or lo <= a <= n_bins * BIN + 1) and (b is None or lo <= b <= n_bins * BIN + 1)]
    rng = np.random.default_rng(n_bins)
    rest = sorted(set(range(len(ws))) - set(near))
    more = rng.choice(rest, 200 - len(near), replace=False).tolist()
    return near + sorted(more)


def index_cleavage_cases(n_bins):
    """``(start, stop, max_length, fs)``: cleavage intervals whose SECOND tile begins exactly at the end of a
    reverse-strand fragment of the longest admissible length (600 under ``max_length=600``) that starts on the bin
    boundary ``fs``: the tile finds it through ``bin_idx[fs >> 9]`` alone, and other fragments cover that base, so the
    proportion there is not 0 / 0.  (The last bin qualifies only where it holds starts behind its offset 0.)"""
    ks = (7, 8, n_bins - 2) + ((n_bins - 1,) if n_bins == 255 else ())
    return [(k * BIN + 600 - TILE, k * BIN + 600 + 100, 600, k * BIN) for k in ks]


# ------------------------------------------------------------------------------------------ section 4: read 1
R1_KINDS = ("front", "behind")
R1_Q = 0
HIST = (50, 200)   # fraglen_hist: lengths 50 .. 249 hold every background fragment


def r1_outlier(i, kind):
    """The read-1 columns of ``r1_world`` with fragment ``i``'s span moved wholly in front of / behind it."""
    fs, fe, _, _, r1s, r1e = r1_world()
    r1s, r1e = r1s.copy(), r1e.copy()
    if kind == "front":
        r1s[i], r1e[i] = fs[i] - R1_SHIFT, fs[i] - R1_SHIFT + R1_LEN
    else:
        r1s[i], r1e[i] = fe[i] + R1_SHIFT - R1_LEN, fe[i] + R1_SHIFT
    return r1s, r1e


def r1_odd_spans():
    """(c): an empty span (rs == re, inside its fragment) at every second position of R1_POS, a reversed one at the
    others."""
    fs, fe, _, _, r1s, r1e = r1_world()
    r1s, r1e = r1s.copy(), r1e.copy()
    for j, i in enumerate(R1_POS):
        if j % 2 == 0:
            r1s[i] = r1e[i] = fs[i] + 30
        else:
            r1s[i], r1e[i] = fs[i] + 40, fs[i] + 20
    return r1s, r1e


def r1_interval(i):
    fs, fe = r1_world()[:2]
    return int(fs[i]) - 10, int(fe[i]) + 10


def r1_tiles(i, n_tiles):
    """``n_tiles`` windows of 200 bases, laid end to end, with fragment ``i`` inside the one in the middle (shifted down
    the contig where ``i`` is near its start or end: the fragment stays interior to one tile)."""
    fs, fe = r1_world()[:2]
    w = 200
    mid = (int(fs[i]) + int(fe[i])) // 2
    a = mid - w // 2 - (n_tiles // 2) * w
    a = max(a, mid - w // 2 - ((mid - w // 2) // w) * w)   # keep the phase, stay at or above 0
    ws = a + w * np.arange(n_tiles)
    return ws.astype(np.int32), (ws + w).astype(np.int32)


def r1_frags(r1s, r1e, lo=0, hi=None):
    fs, fe, mq, st = r1_world()[:4]
    return O.Frags(fs[lo:hi], fe[lo:hi], mq[lo:hi], st[lo:hi], r1s[lo:hi], r1e[lo:hi])


def r1_slice(i, n_tiles=320):
    """Row range of the r1 world that holds every fragment the calls around position ``i`` can touch (the oracle is
    run on this slice: a window's answer depends on no fragment further than the slack away)."""
    fs = r1_world()[0]
    ws, we = r1_tiles(i, n_tiles)
    slack = 2 * R1_SHIFT + 1_000
    return int(np.searchsorted(fs, int(ws[0]) - slack)), int(np.searchsorted(fs, int(we[-1]) + slack))


def r1_expected(r1s, r1e, i, tile_counts=(100, 320)):
    """Every oracle answer of section 4 around fragment ``i`` for the given read-1 columns, as a dict of arrays."""
    lo, hi = r1_slice(i, max(tile_counts))
    fr = r1_frags(r1s, r1e, lo, hi)
    a, b = r1_interval(i)
    out = {}
    for pol in ("midpoint", "any"):
        out["count_" + pol] = O.c_window_counts(fr, [a], [b], mapq_min=R1_Q, policy=pol)
    out["hist"], out["over"] = O.c_fraglen_hist(fr, [a], [b], HIST[0], HIST[1], mapq_min=R1_Q)
    out["short"], out["long"], _ = O.c_delfi_counts(fr, [a], [b], R1_Q)
    for k, c in zip(("sel_s", "sel_e", "sel_q", "sel_st"), O.c_frag_select(fr, a, b, mapq_min=R1_Q)):
        out[k] = c.copy()
    out["wps"] = O.c_wps(fr, a, b, chrom_size(), mapq_min=R1_Q)
    out["cleavage"] = O.c_cleavage(fr, a, b, mapq_min=R1_Q)[2]
    for n in tile_counts:
        ws, we = r1_tiles(i, n)
        out[f"tiles{n}"] = O.c_window_counts(fr, ws, we, mapq_min=R1_Q)
        out[f"tiles{n}_hist"] = O.c_fraglen_hist(fr, ws, we, HIST[0], HIST[1], mapq_min=R1_Q)[0]
        sh, lg, _ = O.c_delfi_counts(fr, ws, we, R1_Q)
        out[f"tiles{n}_short"], out[f"tiles{n}_long"] = sh, lg
    return out


@functools.lru_cache(maxsize=None)
def chrom_size():
    return int(r1_world()[1].max()) + 2 * R1_SHIFT
