"""A small genome with N runs and lower-case runs, its numpy GC oracle and hand-placed fragments, for
``tests/test_gpu_gc_weights.py`` (the shapes of ``tests/test_gpu_frag_gc_bias.py``, restated here so that file stays as
it is)."""
import numpy as np

MAX_LEN = 1000  # FTK_GC_MAX_LEN
LAYOUT = {  # name: (length, N runs, lower-case runs); no length a multiple of 60 or 50
    "wA": (30_011, ((0, 137), (15_000, 15_001), (20_000, 20_250)), ((5_000, 5_600), (20_100, 20_400))),
    "wB": (23_457, ((9_000, 9_017), (23_157, 23_457)), ((1_000, 1_900),)),
    "wC": (41_003, ((12_345, 12_346), (30_000, 31_100)), ((2_000, 2_700), (40_000, 41_003))),
    "wS": (37, (), ((10, 20),)),
}
DUP_LEN = {"wA": 150, "wB": 40, "wC": 300}  # 70 000 copies of one fragment at 1000
N_DUP = 70_000


def make_contig(rng, n, n_runs, lower_runs):
    s = rng.choice(np.frombuffer(b"ACGT", np.uint8), n, p=[0.3, 0.2, 0.2, 0.3])
    for a, b in lower_runs:
        s[a:b] |= 0x20
    for a, b in n_runs:
        s[a:b] = ord("N")
    return s.tobytes().decode()


class Contig:
    def __init__(self, name, seq):
        b = np.frombuffer(seq.encode(), np.uint8)
        self.name, self.seq, self.n = name, seq, len(seq)
        self.cg = np.concatenate(([0], np.cumsum(np.isin(b, np.frombuffer(b"GCgc", np.uint8))))).astype(np.int64)
        self.cn = np.concatenate(([0], np.cumsum(~np.isin(b, np.frombuffer(b"ACGTacgt", np.uint8))))).astype(np.int64)

    def gc(self, a, b):
        """gc(a, b) per element, -1 where it is undefined."""
        a = np.asarray(a, np.int64)
        b = np.asarray(b, np.int64)
        ok = (a >= 0) & (b <= self.n) & (b > a) & (b - a <= MAX_LEN)
        ac, bc = np.clip(a, 0, self.n), np.clip(b, 0, self.n)
        ok &= (self.cn[bc] - self.cn[ac]) == 0
        return np.where(ok, self.cg[bc] - self.cg[ac], -1)

    def expected(self, len_lo, len_hi, stride=1):
        table = np.zeros((len_hi - len_lo + 1, len_hi + 1), np.int64)
        p = np.arange(0, self.n, stride, dtype=np.int64)
        for L in range(len_lo, len_hi + 1):
            q = p[p + L <= self.n]
            q = q[self.cn[q + L] - self.cn[q] == 0]
            table[L - len_lo] = np.bincount(self.cg[q + L] - self.cg[q], minlength=len_hi + 1)
        return table


def fragments_of(ct, rng, length_edges):
    """(start, end, mapq) of one contig, sorted by start: random fragments, fragments of every length of ``length_edges``
    and one beside it at the contig's ends, fragments at the N runs' edges, at every 2bit word alignment, on both sides
    of the MAPQ thresholds, and N_DUP copies of one fragment."""
    n, name = ct.n, ct.name
    s, e, q = [], [], []

    def add(a, b, mq=60):
        s.append(int(a)), e.append(int(b)), q.append(int(mq))

    if n > 1000:
        a = rng.integers(0, n - 10, 4000)
        for x, ln, mq in zip(a, rng.integers(20, 601, 4000), rng.integers(0, 61, 4000)):
            add(x, x + ln, mq)
    lengths = sorted({v + d for v in length_edges for d in (-1, 0, 1)} | {40_000})
    for ln in lengths:
        for a in (0, 1, 777, n - ln, n - ln + 1):  # (n - ln: end = chrom_len; + 1: one base beyond)
            if a >= 0 and ln >= 0:
                add(a, a + ln)
    for ln in (1, 37, 150):
        add(0, ln), add(n - ln, n), add(n - ln + 1, n + 1), add(n - 10, n - 10 + ln + 5000), add(n + 1000, n + 1000 + ln)
        add(n, n + ln), add(n - 50, n + 100)
    for k in range(16):  # every alignment of the first base inside a 2bit word
        for ln in (15, 16, 17, 31, 32, 33, 63, 64, 65):
            add(2000 + k, 2000 + k + ln) if n > 3000 else add(k, k + ln)
    for a0, a1 in LAYOUT[name][1]:
        for ln in (20, 150, 167):
            add(a0 - ln, a0), add(a0 - ln + 1, a0 + 1)
            add(a1 - 1, a1 - 1 + ln), add(a1, a1 + ln)
            add(a0 + 1, a0 + 1 + ln), add(a0 - 5, a0 - 5 + ln)
        if a1 - a0 + 60 <= MAX_LEN:
            add(a0 - 30, a1 + 30), add(a0 - 1, a1 + 1), add(a0, a1)
    for a0, a1 in LAYOUT[name][2]:
        add(a0 + 3, min(a0 + 153, a1)), add(a0 - 20, a0 + 130)
    for mq in (0, 29, 30, 31, 255):
        add(min(3000, n // 2), min(3000, n // 2) + min(167, n // 2), mq)
    if name in DUP_LEN:
        s += [1000] * N_DUP
        e += [1000 + DUP_LEN[name]] * N_DUP
        q += [60] * N_DUP
    s, e, q = np.array(s, np.int64), np.array(e, np.int64), np.array(q, np.int64)
    keep = (s >= 0) & (e < 1 << 30)
    s, e, q = s[keep], e[keep], q[keep]
    o = np.argsort(s, kind="stable")
    return s[o].astype(np.int32), e[o].astype(np.int32), q[o].astype(np.uint8)
