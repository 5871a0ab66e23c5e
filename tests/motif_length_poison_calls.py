"""The motif x length call's entry in the table of ``tests/scratch_poison_calls.py``: ``ftk_motif_length_table`` (with
``ftk_motif_length_lds_rows``, which places its row plans) runs that module's whole procedure - as found, then on a scratch
block filled with 0x00, 0xFF and 0x7F, and once more with device outputs - and is held to the numpy restatement of
``tests/motif_length_helpers.py``.  ``same_after_fills`` is the plain form of the same question for any one call: the
table after ``ftk_ctx_scratch_fill(0xA5)`` and after ``0x00``.

The entry is ADDED to ``scratch_poison_calls.CALLS`` when this module is imported, and ``tests/test_gpu_motif_lengths.py``
imports it.  ``tests/test_gpu_scratch_poison.py`` reads the table when pytest collects it, behind
``test_gpu_motif_lengths.py`` in the directory's order: in a run of the suite the call gets that module's parametrised test
and its last test finds every export in the table.  Run on its own, that module does not see this entry and its last test
names the two symbols; ``test_gpu_motif_lengths.py::test_poison_table_holds_the_new_call`` says so from this side.  Not a test
module itself."""
import numpy as np

from finaletoolkit_amd import _lib as L
from tests import motif_length_helpers as M
from tests import scratch_poison_calls as P

FILLS = (0xA5, 0x00)


def _plans(eng):
    """(k, shift, len_lo, len_hi, len_bin, image): k = 4 over one band + 1 rows, k = 2 on FASTA text over 1024 rows."""
    band = eng.motif_length_lds_rows(4)
    return ((4, 0, 150, 150 + band, 1, "2bit"), (2, -1, 1, 1024, 1, "fa"), (3, 1, 50, 1000, 40, "2bit"))


def run_motif_length_table(x):
    eng, outs = x.eng, {}
    for j, (k, shift, lo, hi, b, image) in enumerate(_plans(eng)):
        n_rows = M.n_rows_of(lo, hi, b)
        table, kept = x.out((2, n_rows, 4 ** k + 1), np.int64), x.out(n_rows, np.int64)
        x.refill()
        eng._check(eng.lib.ftk_motif_length_table(eng.ctx, eng.contig_id("pt"), x.W.rid[image], k, shift, lo, hi, b, 30, table.p, kept.p))
        outs[f"table{j}"], outs[f"kept{j}"] = table, kept
    return x.ret(**outs)


def check_motif_length_table(W, R, eng):
    for j, (k, shift, lo, hi, b, _) in enumerate(_plans(eng)):
        table, kept = M.restated_motif_lengths(W.bases, W.s, W.e, W.q, k, shift, lo, hi, b, 30)
        P.equal(R[f"table{j}"], table, ("table", j))
        P.equal(R[f"kept{j}"], kept, ("kept", j))
        assert kept.sum() > 5_000 and table[..., -1].any()


def same_after_fills(eng, call):
    """``call()`` -> arrays, once as found and once behind every fill of FILLS: ``[(byte, equal to the first run)]``."""
    first = [np.array(a, copy=True) for a in call()]
    out = []
    for byte in FILLS:
        assert eng.scratch_fill(byte) > 0
        again = call()
        out.append((byte, all(np.array_equal(a, b) for a, b in zip(first, again))))
    return first, out


ENTRIES = {
    "ftk_motif_length_table+ftk_motif_length_lds_rows": (run_motif_length_table, check_motif_length_table, True),
}
for _name, _entry in ENTRIES.items():
    P.CALLS.setdefault(_name, _entry)
