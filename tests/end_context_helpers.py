"""A numpy restatement of the "end context" rule of ``include/ftk.h`` (``ftk_end_context``, ``ftk_ref_context``), and a small
genome with N runs and lower-case runs plus hand-placed fragments for it (the shapes of ``tests/gc_genome.py``, restated
here so that file stays as it is).  Shared by ``tests/test_end_context.py`` and ``tests/test_gpu_end_context.py``."""
import numpy as np

MAX_HALF = 128      # FTK_CONTEXT_MAX_HALF
MAX_CLASSES = 8     # FTK_CONTEXT_MAX_CLASSES
DEFAULT_EDGES = (1, 150, 221, 1001)
ONE_CLASS = (1, 1 << 30)
EIGHT_CLASSES = (1, 20, 100, 167, 221, 1_001, 1_500, 4_000, 39_000)
EMPTY_CLASS = 6     # of EIGHT_CLASSES: no fragment has a length of [1 500, 4 000)
WIDTHS = (1, 7, 16, 32, 33, 128)
LAYOUT = {  # name: (length, N runs, lower-case runs); no length a multiple of 60 or 50
    "eA": (30_011, ((0, 137), (15_000, 15_001), (20_000, 20_250)), ((5_000, 5_600), (20_100, 20_400))),
    "eB": (23_457, ((9_000, 9_017), (23_157, 23_457)), ((1_000, 1_900),)),
    "eC": (41_003, ((12_345, 12_346), (30_000, 31_100)), ((2_000, 2_700), (40_000, 41_003))),
    "eS": (37, (), ((10, 20),)),
    "eM": (5_003, (), ((100, 200),)),  # no N: the contig of the cross-check against the motif kernel
}
DUP = {"eA": (1_000, 1_150), "eB": (4_003, 4_043), "eC": (2_222, 2_522)}  # N_DUP copies of one fragment per contig
N_DUP = 70_000

_CODE = np.full(256, 4, np.int8)
for _i, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _i
_COMP = np.array([3, 2, 1, 0, 4], np.int8)
_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def make_contig(rng, n, n_runs, lower_runs):
    s = rng.choice(np.frombuffer(b"ACGT", np.uint8), n, p=[0.3, 0.2, 0.2, 0.3])
    for a, b in lower_runs:
        s[a:b] |= 0x20
    for a, b in n_runs:
        s[a:b] = ord("N")
    return s.tobytes().decode()


def make_genome(rng):
    seqs = {name: make_contig(rng, n, n_runs, lower) for name, (n, n_runs, lower) in LAYOUT.items()}
    assert all(len(s) % 60 and len(s) % 50 for s in seqs.values())
    assert seqs["eA"].startswith("N" * 137) and seqs["eB"].endswith("N" * 300) and seqs["eC"][12_345] == "N" and len(seqs["eS"]) == 37
    assert any(ch.islower() for ch in seqs["eA"])
    return seqs


def reverse_complement(seq: str) -> str:
    """Case and N kept: the reverse-complemented contig of the symmetry test."""
    return seq.encode().translate(_RC)[::-1].decode()


class Bases:
    """``base(q)`` of a sequence string for any integer array ``q``: the code array padded with one N on either side,
    indexed at the clipped position."""
    def __init__(self, seq: str):
        self.n = len(seq)
        self.padded = np.full(self.n + 2, 4, np.int8)
        self.padded[1:-1] = _CODE[np.frombuffer(seq.encode(), np.uint8)]

    def __call__(self, q):
        return self.padded[np.clip(np.asarray(q, np.int64), -1, self.n) + 1]


class SparseBases:
    """The same for a 2bit image of ``n`` bases that is all ``T`` but for ``tail`` (a string, the last bases) and one N
    block ``[n0, n1)``, without holding ``n`` codes."""
    def __init__(self, n, tail, n_block):
        self.n, self.tail, self.n_block = n, Bases(tail), n_block

    def __call__(self, q):
        q = np.asarray(q, np.int64)
        out = np.full(q.shape, 3, np.int8)
        t0 = self.n - self.tail.n
        out = np.where(q >= t0, self.tail(q - t0), out)
        out = np.where((q >= self.n_block[0]) & (q < self.n_block[1]), 4, out)
        return np.where((q < 0) | (q >= self.n), 4, out).astype(np.int8)


def restated_end_context(bases, start, end, mapq, half_width, edges, mapq_min=30, anchor="ends"):
    """``(table, n_kept)`` of section "end context": ``bases`` is a ``Bases`` (or anything with its call)."""
    w, edges = int(half_width), np.asarray(edges, np.int64)
    s, e, q = (np.asarray(v, np.int64) for v in (start, end, mapq))
    ln = e - s
    keep = (q >= mapq_min) & (ln >= edges[0]) & (ln < edges[-1])
    # equal fragments are counted once, with their multiplicity (N_DUP copies would otherwise be most of the work)
    (s, e), mult = np.unique(np.stack([s[keep], e[keep]]), axis=1, return_counts=True)
    ln = e - s
    cls = np.searchsorted(edges, ln, side="right") - 1
    n_classes = len(edges) - 1
    table = np.zeros((n_classes, 2, 2 * w, 25), np.int64)
    half = ln >> 1 if anchor == "centre" else np.zeros_like(ln)
    assert anchor in ("ends", "centre")
    a0, a1 = s + half, e - 1 - half
    for j in range(2 * w):
        o = j - w
        np.add.at(table, (cls, 0, j, 5 * bases(a0 + o).astype(np.int64) + bases(a0 + o + 1)), mult)
        np.add.at(table, (cls, 1, j, 5 * _COMP[bases(a1 - o)].astype(np.int64) + _COMP[bases(a1 - o - 1)]), mult)
    return table, np.bincount(cls, weights=mult, minlength=n_classes).astype(np.int64)


def looped_end_context(seq, start, end, mapq, half_width, edges, mapq_min=30, anchor="ends"):
    """The same rule, one fragment and one offset at a time, straight from the string."""
    n, w = len(seq), int(half_width)

    def base(p):
        return "ACGT".find(seq[p].upper()) % 5 if 0 <= p < n else 4  # (find: -1 for anything else, and -1 % 5 == 4)

    def comp(x):
        return 3 - x if x < 4 else 4

    table = np.zeros((len(edges) - 1, 2, 2 * w, 25), np.int64)
    n_kept = np.zeros(len(edges) - 1, np.int64)
    for s, e, q in zip(start, end, mapq):
        s, e, ln = int(s), int(e), int(e) - int(s)
        if q < mapq_min or not edges[0] <= ln < edges[-1]:
            continue
        c = max(k for k in range(len(edges) - 1) if edges[k] <= ln)
        n_kept[c] += 1
        a0, a1 = (s + (ln >> 1), e - 1 - (ln >> 1)) if anchor == "centre" else (s, e - 1)
        for o in range(-w, w):
            table[c, 0, o + w, 5 * base(a0 + o) + base(a0 + o + 1)] += 1
            table[c, 1, o + w, 5 * comp(base(a1 - o)) + comp(base(a1 - o - 1))] += 1
    return table, n_kept


def restated_ref_context(bases, pos_lo, pos_hi):
    """``out25`` of ``ftk_ref_context``: positions of ``[pos_lo, pos_hi)`` inside the contig."""
    p = np.arange(max(pos_lo, 0), min(pos_hi, bases.n), dtype=np.int64)
    return np.bincount(5 * bases(p).astype(np.int64) + bases(p + 1), minlength=25).astype(np.int64)


def fragments_of(name, n, rng, edge_sets=(DEFAULT_EDGES, EIGHT_CLASSES)):
    """(start, end, mapq) of one contig, sorted by start: random fragments and the hand-placed ones the GPU tests name."""
    s, e, q = [], [], []

    def add(a, b, mq=60):
        s.append(int(a)), e.append(int(b)), q.append(int(mq))

    if n > 1000:
        a = rng.integers(0, n - 10, 4000)
        for x, ln, mq in zip(a, rng.integers(20, 601, 4000), rng.integers(0, 61, 4000)):
            add(x, x + ln, mq)
    lengths = {v + d for edges in edge_sets for v in edges for d in (-1, 0)} | {1, 2, 5, 40_000}
    lengths -= {EIGHT_CLASSES[EMPTY_CLASS], EIGHT_CLASSES[EMPTY_CLASS + 1] - 1}  # (the two that would fill the empty class)
    for ln in sorted(lengths):  # every edge and one below it: at the contig's start, inside, end = chrom_len, one beyond
        for a in (0, 1, 777 if n > 1000 else 3, n - ln, n - ln + 1):
            if a >= 0 and ln >= 1:
                add(a, a + ln)
    for ln in (1, 2, 5, 37, 150):  # L = 1, L < W; far beyond the end; s >= chrom_len
        add(0, ln), add(n - ln, n), add(n - ln + 1, n + 1), add(n - 10, n - 10 + ln + 5000), add(n + 1000, n + 1000 + ln)
        add(n, n + ln), add(n - 1, n - 1 + ln), add(n + 3, n + 3 + ln)
    base = 2000 if n > 3000 else 0
    for k in range(16):  # every alignment of s, and of e - 1, inside a 2bit word of 16 bases
        for ln in (16, 17, 31, 160, 167):
            add(base + k, base + k + ln)
    for a0, a1 in LAYOUT[name][1]:  # anchors within W of each N-run edge, and inside the runs
        for d in (-129, -128, -33, -32, -8, -1, 0, 1, 8, 32, 33, 128, 129):
            for edge in (a0, a1):
                if edge + d >= 0:
                    add(edge + d, edge + d + 167), add(max(edge + d - 167, 0), edge + d + 1)
        add((a0 + a1) // 2, (a0 + a1) // 2 + 150)
    for row in (60, 50, 300, 3000):  # windows that cross a FASTA line break of either width
        for d in (-2, -1, 0, 1):
            if row + d + 170 < n:
                add(row + d, row + d + 170), add(row + d + 7, row + d + 7 + 33)
    for mq in (0, 29, 30, 31, 255):  # both sides of the threshold
        add(min(3000, n // 2), min(3000, n // 2) + min(167, n // 2), mq)
    if name in DUP:
        s += [DUP[name][0]] * N_DUP
        e += [DUP[name][1]] * N_DUP
        q += [60] * N_DUP
    s, e, q = np.array(s, np.int64), np.array(e, np.int64), np.array(q, np.int64)
    keep = (s >= 0) & (e < 1 << 30)
    s, e, q = s[keep], e[keep], q[keep]
    o = np.argsort(s, kind="stable")
    return s[o].astype(np.int32), e[o].astype(np.int32), q[o].astype(np.uint8)
