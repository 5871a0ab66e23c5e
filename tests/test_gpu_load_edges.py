"""What a contig load decides on the device, on the worlds of ``tests/load_edges.py``: the refusals and the summary of
``stats_kernel`` with one offender / one long fragment at every lane, wave, block and grid-stride edge of its launch,
the 512-bp index of ``bin_index_kernel`` around its last bin and the 255 / 256 / 257-bin edge of its launch, the read-1
flag of ``r1_inside_kernel`` with exactly one outlier, ``Engine.set_read1`` and ``load_contig_device``.  Every
comparison is exact: against ``oracle.oracle`` or plain numpy.  ``tests/test_load_edges.py`` asserts (CPU) that the
worlds hold the cases and that each one discriminates.

``Engine.depth`` (ftk_depth) does not read the read-1 columns: in section 4 it is checked to stay the fragments' depth;
the depth that follows the BAM fetch rule is the cleavage pass's, compared through ``Engine.cleavage``."""
import ctypes as C

import numpy as np
import pytest

from finaletoolkit_amd import _lib as L
from finaletoolkit_amd._lib import FtkError
from oracle import oracle as O
from tests import load_edges as E

pytestmark = pytest.mark.gpu
PRE = "le:"


@pytest.fixture(scope="module", autouse=True)
def _release_at_teardown(engine):
    yield
    for name in [n for n in engine.contigs if n.startswith(PRE)]:
        engine.release(name)


def c_info(engine, cid):
    """``(rc, (n, max_len, max_end))`` of the C call itself."""
    n, ml, me = C.c_int64(), C.c_int32(), C.c_int32()
    rc = engine.lib.ftk_frags_info(engine.ctx, int(cid), C.byref(n), C.byref(ml), C.byref(me))
    return rc, (int(n.value), int(ml.value), int(me.value))


def c_from_host(engine, cid, cols):
    s, e, q, st = cols
    return engine.lib.ftk_frags_from_host(engine.ctx, int(cid), L.ptr(s), L.ptr(e), L.ptr(q), L.ptr(st), len(s))


def packed_present(engine, name):
    present = C.c_int32(-1)
    engine._check(engine.lib.ftk_frags_packed(engine.ctx, engine.contig_id(name), C.byref(present), None, None))
    return bool(present.value)


def assert_forgotten(engine, name):
    assert not engine.has_contig(name) and name not in engine.contigs
    with pytest.raises(KeyError):
        engine.window_counts(name, [0], [1])


GOOD = E.sized(1025)


def refusals_of(i):
    base = E.stats_world()
    return (("unsorted", E.unsorted_at(base, i), E.ERR_UNSORTED), ("negative", E.negative_at(base, i), E.ERR_INVALID),
            ("limit", E.end_at(base, i, E.LIMIT), E.ERR_INVALID))


# ------------------------------------------------------------------------------------------ section 1
@pytest.mark.parametrize("i", E.POS)
def test_one_offender_is_refused(engine, i):
    """Through the C ABI as a RELOAD of a good contig (the id must be empty afterwards: the old columns go before the
    new ones are validated, and the next good load must not inherit a flag), then through ``Engine.load_contig`` under
    a new name and as a reload (the name must be forgotten)."""
    raw, name = PRE + "raw", PRE + "bad"
    engine.load_contig(raw, *GOOD)
    cid = engine.contig_id(raw)
    for tag, cols, code in refusals_of(i):
        assert c_from_host(engine, cid, cols) == code, (tag, i)
        assert c_info(engine, cid)[0] == E.ERR_NO_CONTIG, (tag, i)
        assert c_from_host(engine, cid, GOOD) == L.FTK_OK, (tag, i)
        assert c_info(engine, cid) == (L.FTK_OK, E.summary(GOOD)), (tag, i)
        for reload in (False, True):
            if reload:
                engine.load_contig(name, *GOOD)
            used = engine.contig_id(name) if reload else None
            with pytest.raises(FtkError) as ei:
                engine.load_contig(name, *cols)
            assert ei.value.code == code, (tag, i, reload)
            assert_forgotten(engine, name)
            if reload:
                assert c_info(engine, used)[0] == E.ERR_NO_CONTIG, (tag, i)
            engine.load_contig(name, *GOOD)
            assert engine.info(name) == E.summary(GOOD), (tag, i, reload)
            assert used is None or engine.contig_id(name) > used      # a spent id is never handed out again
            engine.release(name)
    engine.release(raw)


@pytest.mark.parametrize("i", E.POS)
def test_end_just_below_the_limit_is_accepted(engine, i):
    cols = E.end_at(E.stats_world(), i, E.LIMIT - 1)
    name = PRE + "top"
    engine.load_contig(name, *cols)
    assert engine.info(name) == (E.N_STATS, E.LIMIT - 1 - int(cols[0][i]), E.LIMIT - 1)
    assert not packed_present(engine, name)
    engine.release(name)


def test_negative_start_ties_and_table_route(engine):
    base = E.stats_world()
    name = PRE + "misc"
    with pytest.raises(FtkError) as ei:
        engine.load_contig(name, *E.start_at(base, 0, -1))
    assert ei.value.code == E.ERR_INVALID
    assert_forgotten(engine, name)
    for cols in (E.all_equal(base), E.ties_at(base), base):       # ties are not disorder
        engine.load_contig(name, *cols)
        assert engine.info(name) == E.summary(cols)
        assert engine.window_counts(name, [None], [None], quality_threshold=0).tolist() == [E.N_STATS]
    engine.release(name)
    with pytest.raises(FtkError) as ei:                           # load_contig_from_table: no such table contig
        engine.load_contig_from_table(name, None, 0, False)
    assert ei.value.code == E.ERR_NO_CONTIG
    assert_forgotten(engine, name)


# ------------------------------------------------------------------------------------------ section 2
@pytest.mark.parametrize("n", E.SIZES)
def test_summary_of_every_size(engine, n):
    cols = E.sized(n)
    name = PRE + "size"
    engine.load_contig(name, *cols)
    assert engine.info(name) == E.summary(cols)
    assert engine.window_counts(name, [None], [None], quality_threshold=0).tolist() == [n]
    ln = cols[1].astype(np.int64) - cols[0]
    want = int(((cols[2] >= 30) & (ln >= 150)).sum())             # (read from the packed column where it is kept)
    assert engine.window_counts(name, [None], [None], quality_threshold=30, min_length=150).tolist() == [want]
    got = engine.frag_select(name, None, None, 0)
    assert all(np.array_equal(g, c) for g, c in zip(got, cols))
    assert packed_present(engine, name)
    engine.release(name)


@pytest.mark.parametrize("i", E.POS)
def test_one_long_fragment(engine, i):
    base = E.stats_world()
    cols = E.long_at(base, i)
    name = PRE + "long"
    engine.load_contig(name, *cols)
    assert engine.info(name) == E.summary(cols) and engine.info(name)[1] == E.LONG
    assert not packed_present(engine, name)
    fr = O.Frags(*cols)
    fs = int(cols[0][i])
    ws, we = E.long_windows(fs)
    for ml in (None, 400):
        for pol in ("any", "midpoint"):
            got = engine.window_counts(name, ws, we, quality_threshold=0, max_length=ml, intersect_policy=pol)
            want = O.c_window_counts(fr, ws, we, mapq_min=0, policy=pol, max_len=ml)
            assert np.array_equal(got, want), (i, ml, pol, got.tolist(), want.tolist())
    lo, hi = E.long_interval(fs)
    assert np.array_equal(engine.depth(name, lo, hi, quality_threshold=0), E.restated_depth(cols, lo, hi)), i
    size = fs + 2 * E.LONG
    for ml in (180, E.LONG + 10_000):
        got = engine.wps(name, lo, hi, size, max_length=ml, quality_threshold=0)
        assert np.array_equal(got, O.c_wps(fr, lo, hi, size, max_len=ml, mapq_min=0)), (i, ml)
    for length, present in ((E.LQ_LEN_MAX, True), (E.LQ_LEN_MAX + 1, False)):
        cols = E.long_at(base, i, length)
        engine.load_contig(name, *cols)
        assert engine.info(name) == E.summary(cols) and packed_present(engine, name) == present, (i, length)
    engine.release(name)


# ------------------------------------------------------------------------------------------ section 3
@pytest.mark.parametrize("n_bins", E.INDEX_BINS)
def test_position_index(engine, n_bins):
    cols = E.index_world(n_bins)
    name = PRE + "index"
    engine.load_contig(name, *cols)
    assert engine.info(name) == E.summary(cols)
    fr = O.Frags(*cols)
    ws, we = E.index_windows(n_bins)
    sample = E.index_select_sample(n_bins)
    for pol in ("midpoint", "any"):
        for ml in E.INDEX_FILTERS:
            got = engine.window_counts(name, ws, we, quality_threshold=E.INDEX_Q, max_length=ml, intersect_policy=pol)
            want = O.c_window_counts(fr, ws, we, mapq_min=E.INDEX_Q, policy=pol, max_len=ml)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (n_bins, pol, ml, [(ws[k], we[k], int(got[k]), int(want[k])) for k in bad[:5]])
            if ml in (None, 50):
                for k in sample:
                    g = engine.frag_select(name, ws[k], we[k], E.INDEX_Q, max_length=ml, intersect_policy=pol)
                    w = O.c_frag_select(fr, ws[k], we[k], mapq_min=E.INDEX_Q, policy=pol, max_len=ml)
                    assert all(np.array_equal(a, b) for a, b in zip(g, w)), (n_bins, pol, ml, ws[k], we[k])
    # a tile of the per-base passes that begins exactly where a longest fragment from a bin boundary ends: the one place
    # where bin_idx[k] must be the FIRST start >= k * 512 and not one behind it (a window's range never is: its
    # candidates satisfy start > ws - lmax strictly)
    for start, stop, ml, at in E.index_cleavage_cases(n_bins):
        got = engine.cleavage(name, start, stop, max_length=ml, quality_threshold=E.INDEX_Q)
        want = O.c_cleavage(fr, start, stop, max_len=ml, mapq_min=E.INDEX_Q)[2]
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (n_bins, start, stop, ml, at, bad[:5].tolist())
    engine.release(name)


# ------------------------------------------------------------------------------------------ section 4
R1 = PRE + "r1"


@pytest.fixture(scope="module")
def r1(engine):
    fs, fe, mq, st, r1s, r1e = E.r1_world()
    engine.load_contig(R1, fs, fe, mq, st, r1s, r1e)
    assert engine.is_bam(R1) and engine.info(R1) == E.summary((fs, fe))
    return dict(inside=(r1s, r1e), cols=(fs, fe, mq, st))


def r1_answers(engine, i, tile_counts=(100, 320)):
    """The library's side of ``load_edges.r1_expected``."""
    a, b = E.r1_interval(i)
    out = {}
    for pol in ("midpoint", "any"):
        out["count_" + pol] = engine.window_counts(R1, [a], [b], quality_threshold=E.R1_Q, intersect_policy=pol)
    out["hist"], out["over"] = engine.fraglen_hist(R1, [a], [b], E.HIST[0], E.HIST[1], quality_threshold=E.R1_Q)
    f = engine.window_features(R1, [a], [b], quality_threshold=E.R1_Q, delfi=dict(quality_threshold=E.R1_Q))
    assert np.array_equal(f["coverage"], out["count_midpoint"])
    out["short"], out["long"] = f["short"], f["long"]
    for k, c in zip(("sel_s", "sel_e", "sel_q", "sel_st"), engine.frag_select(R1, a, b, E.R1_Q)):
        out[k] = c
    out["wps"] = engine.wps(R1, a, b, E.chrom_size(), quality_threshold=E.R1_Q)
    out["cleavage"] = engine.cleavage(R1, a, b, quality_threshold=E.R1_Q)
    for n in tile_counts:
        ws, we = E.r1_tiles(i, n)
        f = engine.window_features(R1, ws, we, quality_threshold=E.R1_Q, hist=E.HIST, delfi=dict(quality_threshold=E.R1_Q))
        out[f"tiles{n}"], out[f"tiles{n}_hist"] = f["coverage"], f["hist"]
        out[f"tiles{n}_short"], out[f"tiles{n}_long"] = f["short"], f["long"]
        assert np.array_equal(engine.window_counts(R1, ws, we, quality_threshold=E.R1_Q), f["coverage"]), (i, n)
    return out


def check_r1(engine, r1, columns, i, tag):
    want = E.r1_expected(columns[0], columns[1], i)
    got = r1_answers(engine, i)
    assert set(got) == set(want)
    for key in want:
        assert np.array_equal(np.asarray(got[key]).astype(want[key].dtype), want[key]), (tag, i, key)
    a, b = E.r1_interval(i)   # ftk_depth: the fragments' depth, whatever read 1 says
    assert np.array_equal(engine.depth(R1, a, b, quality_threshold=E.R1_Q), E.restated_depth(r1["cols"], a, b)), (tag, i)


@pytest.mark.parametrize("kind", E.R1_KINDS)
@pytest.mark.parametrize("i", E.R1_POS)
def test_one_read1_outlier(engine, r1, i, kind):
    out = E.r1_outlier(i, kind)
    engine.set_read1(R1, out[0], out[1], E.N_R1)
    check_r1(engine, r1, out, i, kind)


def test_empty_and_reversed_read1_spans(engine, r1):
    odd = E.r1_odd_spans()
    engine.set_read1(R1, odd[0], odd[1], E.N_R1)
    for i in E.R1_POS:
        check_r1(engine, r1, odd, i, "odd")


def test_read1_replacement(engine, r1):
    """Every ``set_read1`` decides the flag anew: outlier, repaired, outlier, repaired."""
    i = E.CAP_R1
    out, back = E.r1_outlier(i, "front"), r1["inside"]
    for tag, columns in (("outlier", out), ("repaired", back), ("outlier again", out), ("repaired again", back)):
        engine.set_read1(R1, columns[0], columns[1], E.N_R1)
        check_r1(engine, r1, columns, i, tag)


def test_read1_device_columns_and_wrong_row_count(engine, r1):
    import torch
    i = E.CAP_R1
    out, back = E.r1_outlier(i, "behind"), r1["inside"]
    dev = [torch.from_numpy(c).to("cuda:0") for c in out]
    torch.cuda.synchronize()
    engine.set_read1(R1, dev[0], dev[1], E.N_R1)
    for t in dev:
        t.zero_()             # the load copies: the source may change afterwards
    torch.cuda.synchronize()
    check_r1(engine, r1, out, i, "device")
    with pytest.raises(FtkError) as ei:
        engine.set_read1(R1, back[0][:-1].copy(), back[1][:-1].copy(), E.N_R1 - 1)
    assert ei.value.code == E.ERR_INVALID
    check_r1(engine, r1, out, i, "after the refused columns")   # the previous columns stay in force
    engine.set_read1(R1, back[0], back[1], E.N_R1)
    check_r1(engine, r1, back, E.R1_POS[-1], "inside")


# ------------------------------------------------------------------------------------------ section 5
def test_adopted_device_columns(engine):
    import torch
    cols = E.stats_world()
    host, dev_name = PRE + "host", PRE + "dev"
    engine.load_contig(host, *cols)
    rng = np.random.default_rng(5)
    ws = rng.integers(0, int(cols[1].max()), 500).astype(np.int32)
    we = (ws + rng.integers(1, 20_000, 500)).astype(np.int32)

    def answers(name):
        return [np.array(engine.info(name))] + list(engine.frag_select(name, None, None, 0)) + \
            [engine.window_counts(name, ws, we, quality_threshold=20)]
    want = answers(host)
    assert want[-1].max() > 0 and np.array_equal(want[-1], O.c_window_counts(O.Frags(*cols), ws, we, mapq_min=20))
    t = [torch.from_numpy(c.copy()).to("cuda:0") for c in cols]
    torch.cuda.synchronize()
    engine.load_contig_device(dev_name, *t, E.N_STATS)
    assert all(np.array_equal(a, b) for a, b in zip(answers(dev_name), want))
    for x in t:
        x.fill_(7)
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(answers(dev_name), want))
    bad = E.unsorted_at(cols, E.CAP_STATS)
    with pytest.raises(FtkError) as host_err:
        engine.load_contig(host, *bad)
    t = [torch.from_numpy(c).to("cuda:0") for c in bad]
    torch.cuda.synchronize()
    with pytest.raises(FtkError) as dev_err:
        engine.load_contig_device(dev_name, *t, E.N_STATS)
    assert dev_err.value.code == host_err.value.code == E.ERR_UNSORTED
    assert_forgotten(engine, host)
    assert_forgotten(engine, dev_name)
