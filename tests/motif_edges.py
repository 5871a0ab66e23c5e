"""A seeded world for the end-motif / breakpoint-motif pass at the places where its kernels branch: contig ends, N runs
by the dozen, read-1 spans that stick out of their fragment, windows on both sides of the per-window range-test switch,
and a contig dense enough for the 512-thread block kernels.  Not a test module: ``tests/test_motif_edges.py`` asserts
that the world holds every case (CPU), ``tests/test_gpu_motif_edges.py`` runs the kernels on it.  Every expected value
comes from ``oracle.py_region_motifs`` / ``oracle.py_fetch``; nothing here calls the library."""
import functools

import numpy as np

from oracle import oracle as O

K_REF = 4            # the k the systematic fragments and the "k apart" runs are laid out for
MAX_LEN = 40         # longest fragment of every contig here: keeps the reach r = max_len + |f_off| + |r_off| + 1 tight
Q = 30               # mapq threshold of every case
BIN = 512            # the library's start index is binned by 512 bases (window_candidates)
L_EDGE = 24_003      # % 4 == 3; at FASTA width 60 the last line holds 3 bases
L_DENSE = 4_099
STRANDS = ((True, False), (False, False), (False, True))  # (both_strands, negative_strand)

CLUSTER = (9_200, 11_200)      # >= 40 N runs inside
N_FREE = (14_000, 20_500)      # none inside
WIN_A = (11_292, 11_592)       # (ws - MAX_LEN) % 512 == 500: fragments up to 500 bases before ws - MAX_LEN are candidates
WIN_B = (8_924, 9_224)         # we % 512 == 8: fragments up to 503 bases behind we are candidates
LOWER = ((1_000, 1_300), (9_500, 9_800), (23_900, L_EDGE))


def spec_of(kind, k, both, neg):
    """What the Python layer hands to ``Engine.motif_counts`` (frag/_end_motifs.py, frag/_breakpoint_motifs.py)."""
    h = k // 2
    if kind == "end":
        return dict(fwd_offset=0, rev_offset=-k, guard=0, rev_oob_is_error=bool(both))
    return dict(fwd_offset=-h, rev_offset=-h, guard=h, rev_oob_is_error=False)


def reach_of(kind, k, max_len=MAX_LEN):
    """motif_reach's r: a fetched fragment's k-mers start inside (ws - r, we + r + k)."""
    s = spec_of(kind, k, True, False)
    return max_len + abs(s["fwd_offset"]) + abs(s["rev_offset"]) + 1


def edge_runs():
    """Sorted, disjoint, non-adjacent N runs [a, b) of contig ``edge``."""
    runs = [(3, 5)]                                                                   # near position 0, not covering it
    runs += [(400, 401), (801, 803), (1_202, 1_205), (1_603, 1_607), (2_000, 2_005)]  # lengths 1..5, all four phases
    runs += [(2_500, 2_502), (2_503, 2_506)]                                          # one base apart
    runs += [(3_000, 3_003), (3_003 + K_REF, 3_009)]                                  # exactly k apart
    runs += [(3_500, 3_502), (3_502 + K_REF - 1, 3_510)]                              # k - 1 apart
    runs += [(4_000, 4_017), (4_500, 4_564), (5_000, 5_001), (5_511, 5_514), (6_000, 6_002), (6_143, 6_146),
             (7_000, 7_005), (7_500, 7_501), (8_000, 8_004), (8_500, 8_502)]
    runs += [(9_210 + 45 * i, 9_210 + 45 * i + i % 5 + 1) for i in range(44)]          # the cluster
    runs += [(11_500, 11_501), (12_000, 12_002), (12_500, 12_503), (13_000, 13_004), (13_500, 13_505)]
    runs += [(20_600, 20_601), (21_000, 21_007), (21_503, 21_505), (22_002, 22_005), (22_501, 22_502),
             (23_001, 23_005), (23_500, 23_533)]
    runs += [(L_EDGE - 5, L_EDGE - 2)]                                                # near the end, not covering it
    return runs


def make_seq(rng, n, runs, lower):
    s = rng.choice(np.frombuffer(b"ACGT", np.uint8), n).copy()
    for a, b in runs:
        s[a:b] = ord("N")
    for a, b in lower:
        s[a:b] |= 0x20  # (N runs inside turn into 'n')
    return s.tobytes().decode()


def candidate(fs, ws, we, max_len=MAX_LEN):
    """Is a fragment starting at ``fs`` inside the candidate range the library searches for window [ws, we)
    (window_candidates: from the 512-bp bin of ws - max_len to the end of the bin of we)?  The library answers for
    these fragments only: a tabix fetch never needs more, a BAM fetch does when read 1 sticks out further."""
    fs = np.asarray(fs, np.int64)
    if we < ws or we <= 0:
        return np.zeros(fs.shape, bool)
    lo = 0 if ws - max_len <= 0 else ((ws - max_len) // BIN) * BIN
    return (fs >= lo) & (fs < (we // BIN + 1) * BIN)


class Contig:
    """One contig's fragments, start-sorted; ``r1s`` / ``r1e`` None for the tabix variant."""

    def __init__(self, seq, fs, fe, mq, st, r1s=None, r1e=None):
        o = np.argsort(fs, kind="stable")
        self.seq, self.L = seq, len(seq)
        self.fs, self.fe = fs[o].astype(np.int32), fe[o].astype(np.int32)
        self.mq, self.st = mq[o].astype(np.uint8), st[o].astype(np.uint8)
        self.r1s = None if r1s is None else r1s[o].astype(np.int32)
        self.r1e = None if r1e is None else r1e[o].astype(np.int32)

    @property
    def bam(self):
        return self.r1s is not None

    def columns(self):
        kw = dict(r1_start=self.r1s, r1_end=self.r1e) if self.bam else {}
        return (self.fs, self.fe, self.mq, self.st), kw

    def rows(self, lo=0, hi=None):
        cols = [self.fs, self.fe, self.mq, self.st] + ([self.r1s, self.r1e] if self.bam else [])
        return list(zip(*(c[lo:hi].tolist() for c in cols)))

    def rows_near(self, ws, we):
        """The rows a window can fetch, by ``searchsorted`` on the starts (a read-1 span reaches at most ``slack``
        bases beyond its fragment)."""
        slack = MAX_LEN + (int(max((self.fs - self.r1s).max(), (self.r1e - self.fe).max(), 0)) if self.bam else 0)
        lo, hi = np.searchsorted(self.fs, ws - slack), np.searchsorted(self.fs, max(we, ws) + slack + 1)
        return self.rows(lo, hi)

    def fetched(self, ws, we):
        """Mask of the fragments ``oracle.py_fetch`` yields for [ws, we) (numpy restatement, checked against it by the
        CPU test)."""
        a, b = (self.r1s, self.r1e) if self.bam else (self.fs, self.fe)
        return (a < we) & (b > ws) & (self.mq >= Q)


def inside_spans(rng, fs, fe, st):
    """Read-1 spans inside their fragment: a prefix of a forward fragment, a suffix of a reverse one."""
    ln = fe - fs
    rl = np.minimum(ln, rng.integers(1, MAX_LEN + 1, len(fs)))
    r1s = np.where(st != 0, fs, fe - rl)
    return r1s.astype(np.int64), (r1s + rl).astype(np.int64)


def build_edge(rng):
    runs = edge_runs()
    seq = make_seq(rng, L_EDGE, runs, LOWER)
    L = L_EDGE
    fs, fe, mq, st = [], [], [], []

    def add(a, b, q=None, s=None):
        if not (0 <= a < b <= a + MAX_LEN and a <= L - 1):
            return None
        i = len(fs)
        fs.append(a), fe.append(b)
        mq.append((Q - 1, Q, 60)[i % 3] if q is None else q)
        st.append((i // 3) % 2 if s is None else s)
        return i

    # systematic: every run, both edges, the forward k-mer start fs and the reverse one fe - k at edge + d, d = -8..+1
    for a, b in runs:
        for edge in (a, b):
            for d in range(-8, 2):
                p = edge + d
                ln = int(rng.integers(K_REF + 1, MAX_LEN + 1))
                add(p, p + ln)
                add(p + K_REF - ln, p + K_REF)
    n_sys = len(fs)
    # contig start and end
    for a in range(0, 9):
        for ln in range(1, 11):
            add(a, a + ln, 60)
    for a in range(0, 13):               # the lowest starts a window at ws in {r - 2, r - 1, r} can fetch
        add(a, a + MAX_LEN, 60), add(a, a + MAX_LEN - 1, 60)
    for b in range(L - 8, L + 4):
        for ln in (1, 2, 3, K_REF, 9, MAX_LEN):
            add(b - ln, b, 60)
    for a in range(L - 60, L - 40):      # the highest starts a window at we in {L - r - k, .., + 2} can fetch
        add(a, a + MAX_LEN, 60)
    # fill
    a = rng.integers(0, L - 1, 3000)
    for x, ln, q, s in zip(a.tolist(), rng.integers(1, MAX_LEN + 1, 3000).tolist(), rng.integers(0, 61, 3000).tolist(),
                           rng.integers(0, 2, 3000).tolist()):
        add(x, min(x + ln, L), q, s)
    n_plain = len(fs)
    # fragments whose read 1 will stick out into WIN_A (from before it) / WIN_B (from behind it): on N runs and clean
    far = []  # (index, +1: r1_end beyond fe / -1: r1_start before fs)
    for ra, rb in runs:
        for side, near in ((1, WIN_A[0] - 360 <= ra and rb <= WIN_A[0] - 70),
                           (-1, WIN_B[1] + 70 <= ra and rb <= WIN_B[1] + 360)):
            if not near:
                continue
            for d in range(K_REF):
                far.append((add(ra - d, ra - d + 12, 60, 1), side))                    # forward k-mer on the run
                far.append((add(ra - d - 8, ra - d + K_REF, 60, 0), side))             # reverse k-mer on the run
            for ln in (15, 20, 24):
                far.append((add(rb + 6, rb + 6 + ln, 60, ln & 1), side))               # clean: both k-mers between runs
    fs, fe = np.array(fs, np.int64), np.array(fe, np.int64)
    mq, st = np.array(mq, np.int64), np.array(st, np.int64)
    r1s, r1e = inside_spans(rng, fs, fe, st)
    in_r1s, in_r1e = r1s.copy(), r1e.copy()
    for i, side in far:
        if side > 0:   # read 1 starts at the fragment's start and runs on into WIN_A
            r1s[i], r1e[i] = fs[i], WIN_A[0] + 1 + int(rng.integers(0, 20))
        else:          # read 1 starts inside WIN_B and ends at the fragment's end
            r1s[i], r1e[i] = WIN_B[1] - 1 - int(rng.integers(0, 20)), fe[i]
    # mild stick-outs among the plain fragments, 1..30 bases on either side
    for i in rng.choice(n_plain, 400, replace=False).tolist():
        if rng.integers(0, 2):
            r1e[i] = fe[i] + int(rng.integers(1, 31))
        else:
            r1s[i] = max(fs[i] - int(rng.integers(1, 31)), 0)
    tab = Contig(seq, fs, fe, mq, st)
    inside = Contig(seq, fs, fe, mq, st, in_r1s, in_r1e)
    # A span may stick out only as far as its fragment stays a candidate of every tested window it reaches (the limit
    # of the library's BAM fetch: candidates come from the fragment starts, window_candidates).  Spans that break this
    # for some window of the `small` sets go back inside.
    wins = sorted({w for kind in ("end", "breakpoint") for k in range(1, 8) for w in small_windows(runs, L, kind, k)})
    for ws, we in wins:
        bad = (r1s < we) & (r1e > ws) & ~candidate(fs, ws, we)
        r1s[bad], r1e[bad] = in_r1s[bad], in_r1e[bad]
    bam = Contig(seq, fs, fe, mq, st, r1s, r1e)
    return dict(runs=runs, sys_mapq=mq[:n_sys].copy(), sys_strand=st[:n_sys].copy(), edge=tab, edge_bam=bam, edge_bam_inside=inside)


def build_dense(rng):
    runs = [(0, 2), (700, 701), (1_497, 1_503), (2_047, 2_050), (3_333, 3_338), (L_DENSE - 4, L_DENSE - 1)]
    seq = make_seq(rng, L_DENSE, runs, ((2_000, 2_100),))
    n = 20_000
    fs = rng.integers(0, L_DENSE - 1, n)
    fe = np.minimum(fs + rng.integers(1, MAX_LEN + 1, n), L_DENSE + 3)
    fs[:2], fe[:2] = (0, 5), (MAX_LEN, 5 + MAX_LEN)
    mq, st = rng.integers(Q - 3, Q + 4, n), rng.integers(0, 2, n)
    r1s, r1e = inside_spans(rng, fs, fe, st)
    return dict(dense_runs=runs, dense=Contig(seq, fs, fe, mq, st), dense_bam=Contig(seq, fs, fe, mq, st, r1s, r1e))


def small_windows(runs, L, kind, k, max_len=MAX_LEN):
    """The `small` window set of one case (fewer windows than compute units: the planned wave-per-window and chunked
    kernels).  The windows beside the range-test switch depend on the case's reach r."""
    r = reach_of(kind, k, max_len)
    w = []
    for a, b in (runs[1], runs[30], runs[70], runs[-1]):   # single bases at run edges (runs[70], runs[-1]: past the 64th)
        w += [(a - 1, a), (a, a + 1), (b - 1, b), (b, b + 1)]
    w += [(0, 1), (0, k), (L - 1, L), (L, L + 10), (-50, 30), (-20, -5), (L + 100, L + 200)]
    w += [(3_001, 3_001)]            # empty, on a run: the fragments across the point are fetched (fs < we, fe > ws)
    # reversed: the library answers nothing; no fragment or read 1 is long enough to satisfy fs < we and fe > ws
    w += [(6_000, 5_000)]
    w += [(0, L), (15_000, 16_000), CLUSTER, WIN_A, WIN_B]
    w += [(ws, ws + 300) for ws in (r - 2, r - 1, r)]
    w += [(we - 300, we) for we in (L - r - k, L - r - k + 1, L - r - k + 2)]
    return w


def tile_windows(L=L_EDGE, step=64):
    ws = np.arange(0, L, step)
    return list(zip(ws.tolist(), (ws + step).tolist()))


DENSE_DISTINCT = [(0, 900), (37, 987), (500, 1_500), (1_001, 1_914), (1_500, 2_487), (2_222, 3_182), (3_000, 3_999),
                  (3_149, L_DENSE)]


def dense_windows():
    """320 windows: the 8 distinct ones, 40 times over, interleaved."""
    return DENSE_DISTINCT * 40


@functools.lru_cache(maxsize=None)
def world():
    rng = np.random.default_rng(20_261_018)
    w = build_edge(rng)
    w.update(build_dense(rng))
    return w


# ------------------------------------------------------------------------------------------ expected values
def end_both_split(rows, seq, a, b, k, q):
    """Both-strands end motifs of region [a, b) from two strand-wise oracle calls, for inputs where the reference
    raises (frag/_end_motifs.py:150-166: a 3' k-mer off the contig is a RuntimeError there, and a count in the library's
    error output).  Returns ``(counts, n_raise)``.  The forward call takes every row as a forward fragment.  The
    reverse call takes the rows whose 5' k-mer lies inside the contig: in the reference a 5' k-mer off the contig is a
    ``continue`` that drops the fragment's other end as well.  ``n_raise`` counts the fetched rows of that second set
    whose 3' k-mer leaves the contig - each of them is found by asking the oracle with that row alone."""
    n = len(seq)
    fwd = O.py_region_motifs([(r[0], r[1], r[2], 1) + tuple(r[4:]) for r in rows], seq, a, b, k, "end", False, False, q)
    keep = [r for r in rows if 0 <= r[0] and r[0] + k <= n]
    rev = O.py_region_motifs(keep, seq, a, b, k, "end", False, True, q)
    n_raise = 0
    for r in keep:
        if r[1] - k < 0 or r[1] > n:
            try:
                O.py_region_motifs([r], seq, a, b, k, "end", True, False, q)
            except RuntimeError:
                n_raise += 1
    return fwd + rev, n_raise


def expected_window(ct, ws, we, kind, k, both, neg):
    """(counts, nfrag, err) of one window from the oracle."""
    rows = ct.rows_near(ws, we)
    nfrag = sum(1 for _ in O.py_fetch(rows, ws, we, Q))
    if kind == "end" and both:
        counts, err = end_both_split(rows, ct.seq, ws, we, k, Q)
    else:
        counts, err = O.py_region_motifs(rows, ct.seq, ws, we, k, kind, both, neg, Q), 0
    return counts, nfrag, err


def expected(ct, windows, kind, k, both, neg):
    """Stacked (counts [n, 4^k], nfrag [n], err [n]); equal windows are computed once."""
    memo = {}
    for w in windows:
        if w not in memo:
            memo[w] = expected_window(ct, w[0], w[1], kind, k, both, neg)
    return (np.stack([memo[w][0] for w in windows]), np.array([memo[w][1] for w in windows], np.int64),
            np.array([memo[w][2] for w in windows], np.int64))
