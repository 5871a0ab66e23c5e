"""A numpy restatement of the "motif x length" rule of ``include/ftk.h`` (``ftk_motif_length_table``) over the genome, the
``Bases`` and the hand-placed fragments of ``tests/end_context_helpers.py``.  Shared by ``tests/test_motif_lengths.py`` and
``tests/test_gpu_motif_lengths.py``."""
import numpy as np

from tests import end_context_helpers as H

MAX_K = 4        # FTK_MOTIFLEN_MAX_K
MAX_ROWS = 1024  # FTK_MOTIFLEN_MAX_ROWS
KS = (1, 2, 3, 4)
_COMP = np.array([3, 2, 1, 0, 4], np.int8)


def n_rows_of(len_lo, len_hi, len_bin):
    return (int(len_hi) - int(len_lo)) // int(len_bin) + 1


def restated_motif_lengths(bases, start, end, mapq, k, shift, len_lo, len_hi, len_bin=1, mapq_min=30):
    """``(table, n_kept)`` of section "motif x length": ``bases`` is an ``H.Bases`` (or anything with its call)."""
    k, shift = int(k), int(shift)
    s, e, q = (np.asarray(v, np.int64) for v in (start, end, mapq))
    ln = e - s
    keep = (q >= mapq_min) & (ln >= len_lo) & (ln <= len_hi)
    # equal fragments are counted once, with their multiplicity (N_DUP copies would otherwise be most of the work)
    key, mult = np.unique(s[keep] * (1 << 31) + e[keep], return_counts=True)  # (0 <= e < 2^31: one word per fragment)
    s, e = key >> 31, key & ((1 << 31) - 1)
    row = (e - s - len_lo) // len_bin
    n_rows = n_rows_of(len_lo, len_hi, len_bin)
    table = np.zeros((2, n_rows, 4 ** k + 1), np.int64)
    code = np.zeros((2, len(s)), np.int64)
    undefined = np.zeros((2, len(s)), bool)
    for i in range(k):
        u = bases(s + shift + i).astype(np.int64)
        d = _COMP[bases(e - 1 - shift - i)].astype(np.int64)
        for kind, x in enumerate((u, d)):
            undefined[kind] |= x == 4
            code[kind] = 4 * code[kind] + x
    for kind in range(2):
        np.add.at(table, (kind, row, np.where(undefined[kind], 4 ** k, code[kind])), mult)
    return table, np.bincount(row, weights=mult, minlength=n_rows).astype(np.int64)


def looped_motif_lengths(seq, start, end, mapq, k, shift, len_lo, len_hi, len_bin=1, mapq_min=30):
    """The same rule, one fragment and one base at a time, straight from the string."""
    n = len(seq)

    def base(p):
        return "ACGT".find(seq[p].upper()) % 5 if 0 <= p < n else 4  # (find: -1 for anything else, and -1 % 5 == 4)

    def comp(x):
        return 3 - x if x < 4 else 4

    n_rows = n_rows_of(len_lo, len_hi, len_bin)
    table = np.zeros((2, n_rows, 4 ** k + 1), np.int64)
    n_kept = np.zeros(n_rows, np.int64)
    for s, e, q in zip(start, end, mapq):
        s, e, ln = int(s), int(e), int(e) - int(s)
        if q < mapq_min or not len_lo <= ln <= len_hi:
            continue
        r = (ln - len_lo) // len_bin
        n_kept[r] += 1
        for kind in range(2):
            xs = [base(s + shift + i) if kind == 0 else comp(base(e - 1 - shift - i)) for i in range(k)]
            col = 4 ** k if 4 in xs else sum(x * 4 ** (k - 1 - i) for i, x in enumerate(xs))
            table[kind, r, col] += 1
    return table, n_kept


def band_starts(bands, len_lo=1, n_rows=MAX_ROWS):
    """The lengths that start a band of ``band`` rows for each of ``bands`` (rows of one length from ``len_lo``)."""
    return sorted({len_lo + r for band in bands for r in range(band, n_rows, band)})


def edge_sets_for(bands, len_lo=1, len_hi=MAX_ROWS):
    """The ``edge_sets`` of ``H.fragments_of`` (which places the lengths ``v`` and ``v - 1`` of every value it is given) for
    the rows ``len_lo .. len_hi``: both sides of every band start, ``len_lo``, ``len_hi`` and ``len_hi + 1``; without the two
    lengths ``fragments_of`` never places."""
    never = {H.EIGHT_CLASSES[H.EMPTY_CLASS], H.EIGHT_CLASSES[H.EMPTY_CLASS + 1] - 1}
    values = set(band_starts(bands, len_lo, len_hi - len_lo + 1)) | {len_lo, len_hi, len_hi + 1, len_hi + 2}
    return (tuple(sorted(values - never)),) + (H.DEFAULT_EDGES, H.EIGHT_CLASSES)


def row_sums_hold(table, n_kept):
    return all(np.array_equal(table[kind].sum(axis=-1), n_kept) for kind in range(2))
