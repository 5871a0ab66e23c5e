"""The co-fragmentation calls' entries in the table of ``tests/scratch_poison_calls.py``: ``ftk_hist_ks`` (with
``ftk_hist_ks_shape``, which places its rows) and ``ftk_cofrag`` run that module's whole procedure - as found, then on a
scratch block filled with 0x00, 0xFF and 0x7F, and once more with device outputs - and are held to the numpy restatement
of ``tests/cofrag_helpers.py``.

The entries are ADDED to ``scratch_poison_calls.CALLS`` when this module is imported, and ``tests/test_gpu_cofrag.py``
imports it.  ``tests/test_gpu_scratch_poison.py`` reads the table when pytest collects it, behind ``test_gpu_cofrag.py`` in
the directory's order: in a run of the suite the two calls get that module's parametrised test and its last test finds
every export in the table.  Run on its own, that module does not see these entries and its last test names the three
symbols; ``test_gpu_cofrag.py::test_poison_table_holds_the_new_calls`` says so from this side.  Not a test module itself."""
import ctypes as C

import numpy as np

from finaletoolkit_amd import _lib as L
from tests import cofrag_helpers as CF
from tests import scratch_poison_calls as P

COFRAG_HIST = (60, 300)


def _ks_hist(W, eng):
    """Histogram rows around the pair tile and the LDS chunk of the tiled kernel: two tiles a side and a partial third
    chunk, one row empty."""
    t, chunk = eng.hist_ks_shape()

    def make():
        hist = CF.random_hist(np.random.default_rng(20261022), t + 5, 2 * chunk + 3)
        hist[4] = 0
        return hist
    return W.memo("ks_hist", make)


def run_hist_ks(x):
    eng = x.eng
    hist = _ks_hist(x.W, eng)
    n_rows, n_bins = hist.shape
    k, at, n = x.out((n_rows, n_rows), np.int64), x.out((n_rows, n_rows), np.int32), x.out(n_rows, np.int64)
    x.refill()
    eng._check(eng.lib.ftk_hist_ks(eng.ctx, L.ptr(hist), n_rows, n_bins, k.p, at.p, n.p))
    k2, n2 = x.out((n_rows, n_rows), np.int64), x.out(n_rows, np.int64)  # without `at`
    x.refill()
    eng._check(eng.lib.ftk_hist_ks(eng.ctx, L.ptr(hist), n_rows, n_bins, k2.p, None, n2.p))
    return x.ret(k=k, at=at, n=n, k2=k2, n2=n2)


def check_hist_ks(W, R, eng):
    wk, wat, wn = CF.ks_matrix(_ks_hist(W, eng))
    P.equal(R["k"], wk, "k")
    P.equal(R["at"], wat, "at")
    P.equal(R["n"], wn, "n")
    P.equal(R["k2"], wk, "k2")
    P.equal(R["n2"], wn, "n2")
    assert wk.any() and wat.any()


def run_cofrag(x):
    W, eng, n = x.W, x.eng, len(x.W.ws)
    k, at, cnt, over = x.out((n, n), np.int64), x.out((n, n), np.int32), x.out(n, np.int64), x.out(n, np.int64)
    f = P._flt(eng, "pt")
    x.refill()
    eng._check(eng.lib.ftk_cofrag(eng.ctx, eng.contig_id("pt"), L.ptr(W.ws), L.ptr(W.we), n, C.byref(f), *COFRAG_HIST, k.p, at.p, cnt.p, over.p))
    return x.ret(k=k, at=at, n=cnt, overflow=over)


def check_cofrag(W, R, eng):
    want_h, want_o = P.O.c_fraglen_hist(W.fr, W.ws, W.we, *COFRAG_HIST, mapq_min=30)
    wk, wat, wn = CF.ks_matrix(want_h)
    P.equal(R["k"], wk, "k")
    P.equal(R["at"], wat, "at")
    P.equal(R["n"], wn, "n")
    P.equal(R["overflow"], want_o, "overflow")
    assert wk.any() and want_o.any()


ENTRIES = {
    "ftk_hist_ks+ftk_hist_ks_shape": (run_hist_ks, check_hist_ks, True),
    "ftk_cofrag": (run_cofrag, check_cofrag, True),
}
for _name, _entry in ENTRIES.items():
    P.CALLS.setdefault(_name, _entry)
