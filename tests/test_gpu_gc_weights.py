"""GPU: the per-fragment weight column and its sums per window (``csrc/ftk_weights.hip``) - ``Engine.set_gc_weights``,
``set_weights``, ``weights`` and ``weighted_window_sums`` against a numpy restatement written here, exactly equal
everywhere (the sums are integers): the weight column on a 2bit and a FASTA image of one genome, at the contigs' and the
N runs' edges, at every word alignment, on both sides of the LDS limit of the weight table; the sums on arbitrary
columns, tied to ``window_counts`` by unit weights, on a plain contig and on one with read1 columns, past 2^48; the
column's life cycle; the C ABI's argument errors; and ``frag_gc_coverage`` / the command line on a synthetic BAM and its
fragment file."""
import ctypes as C
import gzip
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests.gc_genome import DUP_LEN, LAYOUT, N_DUP, Contig, fragments_of, make_contig
from tests.helpers import bam_expected, read_frag_gz, write_2bit, write_fasta, write_synthetic_bam
from tests.weights_helpers import restated_sums

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 65536           # FTK_WEIGHT_ONE
CHUNK = 4096          # kChunk: candidates per block and step of the window kernel
U32_MAX = 2 ** 32 - 1
# the weight table is staged in LDS while its packed form (row L: L + 1 cells) has at most 32 768 cells
# (kGcWeightLdsCells): (1, 254) fits, (1, 255) is read from global memory, like (1, 1000)
assert 255 * 256 // 2 - 1 <= 32_768 < 256 * 257 // 2 - 1
PAIRS = ((100, 220), (167, 167), (1, 64), (1, 254), (1, 255), (1, 1000))
IMAGES = ("2bit", "fa50")


@pytest.fixture(scope="module")
def world(engine, tmp_path_factory):
    from finaletoolkit_amd.reference import ReferenceGenome
    d = tmp_path_factory.mktemp("gcweights")
    rng = np.random.default_rng(20261019)
    seqs = {name: make_contig(rng, n, n_runs, lower) for name, (n, n_runs, lower) in LAYOUT.items()}
    assert all(len(s) % 50 for s in seqs.values())
    paths = {"2bit": str(d / "g.2bit"), "fa50": str(d / "g50.fa")}
    write_2bit(paths["2bit"], seqs)
    write_fasta(paths["fa50"], seqs, width=50)
    w = dict(dir=d, seqs=seqs, paths=paths, refs={k: ReferenceGenome(p) for k, p in paths.items()},
             contigs={name: Contig(name, s) for name, s in seqs.items()}, cols={}, gc={})
    edges = sorted({v for pair in PAIRS for v in pair})
    for name, ct in w["contigs"].items():
        cols = fragments_of(ct, rng, edges)
        engine.load_contig("gw:" + name, *cols, np.zeros(len(cols[0]), np.uint8))
        w["cols"][name] = cols
        w["gc"][name] = ct.gc(cols[0], cols[1])
    yield w
    for name in w["contigs"]:
        engine.release("gw:" + name)
    for r in w["refs"].values():
        r.close()


def rid_of(engine, world, image, name):
    return world["refs"][image].device_image(engine, name, with_layout=True)


def random_table(rng, lo, hi):
    t = rng.integers(1, 2 ** 32, (hi - lo + 1, hi + 1), dtype=np.uint64).astype(np.uint32)
    t[rng.random(t.shape) < 0.1] = 0
    return t


def restated_column(world, name, table, lo, hi, mapq_min):
    s, e, q = world["cols"][name]
    ln = e.astype(np.int64) - s
    rule = (q >= mapq_min) & (ln >= lo) & (ln <= hi)
    gc = world["gc"][name]
    ok = rule & (gc >= 0)
    want = np.zeros(len(s), np.uint32)
    want[ok] = table[ln[ok] - lo, gc[ok]]
    return want, int((rule & (want == 0)).sum()), rule, gc


# ---- 1. the weight column --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("len_lo, len_hi", PAIRS)
def test_gc_weight_column_equals_the_restatement(engine, world, len_lo, len_hi):
    rng = np.random.default_rng(len_lo * 1009 + len_hi)
    table = random_table(rng, len_lo, len_hi)
    for name in LAYOUT:
        for mapq_min in (0, 30, 31):
            want, want_zero, rule, gc = restated_column(world, name, table, len_lo, len_hi, mapq_min)
            got = {}
            for image in IMAGES:
                n_zero = engine.set_gc_weights("gw:" + name, rid_of(engine, world, image, name), len_lo, len_hi, table, mapq_min)
                got[image] = engine.weights("gw:" + name)
                assert got[image].dtype == np.uint32 and got[image].shape == want.shape
                bad = np.flatnonzero(got[image] != want)
                assert len(bad) == 0, (name, image, mapq_min, bad[:5], got[image][bad[:5]], want[bad[:5]])
                assert n_zero == want_zero, (name, image, mapq_min)
            assert np.array_equal(got["2bit"], got["fa50"])
        if name != "wS" and len_hi - len_lo >= 100:  # the case bites: weights, undefined spans and zero cells are all there
            want, want_zero, rule, gc = restated_column(world, name, table, len_lo, len_hi, 30)
            assert (want > 0).sum() > 50 and (rule & (gc < 0)).sum() > 10 and (rule & (gc >= 0) & (want == 0)).sum() > 0
        if name in DUP_LEN and len_lo <= DUP_LEN[name] <= len_hi:
            assert (rule.sum()) > N_DUP


def test_second_call_replaces_the_column(engine, world):
    rng = np.random.default_rng(5)
    rid = rid_of(engine, world, "2bit", "wB")
    first, second = random_table(rng, 100, 220), random_table(rng, 1, 64)
    engine.set_gc_weights("gw:wB", rid, 100, 220, first)
    a = engine.weights("gw:wB").copy()
    engine.set_gc_weights("gw:wB", rid, 1, 64, second, 0)
    b = engine.weights("gw:wB")
    assert np.array_equal(a, restated_column(world, "wB", first, 100, 220, 30)[0])
    assert np.array_equal(b, restated_column(world, "wB", second, 1, 64, 0)[0]) and not np.array_equal(a, b)
    engine.set_weights("gw:wB", np.full(len(a), 3, np.uint32))  # and an arbitrary column replaces that one
    assert np.all(engine.weights("gw:wB") == 3)
    with pytest.raises(ValueError, match="shape"):
        engine.set_gc_weights("gw:wB", rid, 100, 220, second)


# ---- 2. the sums -----------------------------------------------------------------------------------------------------------
EVEN, ODD = (5_000, 5_100), (7_000, 7_101)  # hand-placed fragments the windows' bounds are put on
GAP = (30_000, 33_000)                      # no fragment starts or ends in here
DUP = (1_000, 1_150)                        # N_DUP copies


def sums_contig(rng):
    """(start, end, mapq, r1_start, r1_end, is_dup) sorted by start; read1 is the first or the last 60 bases."""
    a = np.concatenate([rng.integers(0, 29_000, 6000), rng.integers(33_100, 40_000, 1500)])
    ln = rng.integers(20, 601, len(a))
    outside = (a + ln <= GAP[0]) | (a >= GAP[1])
    a, ln = a[outside], ln[outside]
    s = list(a) + [EVEN[0], ODD[0], EVEN[0], ODD[0], 0, 0, 39_990]
    e = list(a + ln) + [EVEN[1], ODD[1], EVEN[1], ODD[1], 1, 600, 40_600]
    q = list(rng.integers(0, 61, len(a))) + [60, 60, 29, 30, 60, 60, 60]
    dup = [False] * len(s) + [True] * N_DUP
    s += [DUP[0]] * N_DUP
    e += [DUP[1]] * N_DUP
    q += [60] * N_DUP
    s, e, q, dup = np.array(s, np.int64), np.array(e, np.int64), np.array(q, np.int64), np.array(dup)
    fwd = rng.integers(0, 2, len(s)).astype(bool)
    fwd[dup] = False  # the copies' read1 lies at their far end
    rl = np.minimum(60, e - s)
    r1s = np.where(fwd, s, e - rl)
    o = np.argsort(s, kind="stable")
    s, e, q, r1s, rl, dup = s[o], e[o], q[o], r1s[o], rl[o], dup[o]
    assert np.all(np.diff(np.flatnonzero(dup)) == 1)  # the copies are one run of the column
    return s, e, q, r1s, r1s + rl, dup


def window_sets(n_cu):
    tiles = lambda k: (np.arange(k) * (41_000 // k + 1), np.arange(k) * (41_000 // k + 1) + 41_000 // k + 1)  # noqa: E731
    on_bounds = []
    for fs, fe in (EVEN, ODD):
        mid = (fs + fe) // 2
        for p in (fs, fs + 1, fe - 1, fe, fe + 1, mid, mid + 1, mid - 1):
            on_bounds += [(p, p + 300), (p - 300, p), (p, p + 1), (p, p)]
    sets = {
        "whole": ([None], [None]),
        "open_lo": ([None, None, None], [0, 1_075, 1 << 30]),
        "open_hi": ([0, 1_075, 41_000, 1 << 30], [None, None, None, None]),
        "one": ([3_000], [9_000]),
        "three": ([0, 10_000, 20_000], [10_000, 20_000, 41_000]),
        "below_s": tiles(4 * n_cu - 1),   # two blocks per window ...
        "above_s": tiles(4 * n_cu + 1),   # ... and one: either side of the point where S changes
        "unsorted": ([20_000, 500, 20_000, 900, 0, 20_000, 950], [41_000, 1_500, 41_000, 1_300, 41_000, 20_001, 1_010]),
        "empty": ([5_050, 5_050, 5_051, 1_075, 1_075, 9_000], [5_050, 5_051, 5_050, 1_075, 1_076, 8_000]),
        "behind": ([41_000, 1_000_000, (1 << 30) - 5, -500, -1], [41_001, 2_000_000, 1 << 30, 0, 1]),
        "on_bounds": ([a for a, _ in on_bounds], [b for _, b in on_bounds]),
        # > kChunk candidates each; the second holds no fragment; the copies overlap the third and hold the fourth's
        # midpoint rule, their read1 [1090, 1150) lies outside both
        "chunks": ([900, GAP[0] + 700, 995, 1_000], [1_300, GAP[0] + 1_500, 1_005, 1_085]),
    }
    return {k: (list(a), list(b)) for k, (a, b) in sets.items()}


FILTERS = ((0, None, None), (30, 120, 180))


@pytest.fixture(scope="module")
def sums_world(engine):
    import torch
    rng = np.random.default_rng(424242)
    w = dict(n_cu=torch.cuda.get_device_properties(0).multi_processor_count, cols={})
    for kind in ("plain", "bam"):
        cols = sums_contig(rng)
        w["cols"][kind] = cols
        r1 = (cols[3], cols[4]) if kind == "bam" else (None, None)
        engine.load_contig("gw:sums:" + kind, cols[0], cols[1], cols[2], np.zeros(len(cols[0]), np.uint8), *r1)
    w["sets"] = window_sets(w["n_cu"])
    n = len(w["cols"]["plain"][0])
    w["weights"] = {
        "random": rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32),
        "zeros20": np.where(rng.random(n) < 0.2, 0, rng.integers(1, 2 ** 20, n)).astype(np.uint32),
        "all_zero": np.zeros(n, np.uint32),
        "unit": np.full(n, ONE, np.uint32),
    }
    yield w
    for kind in ("plain", "bam"):
        engine.release("gw:sums:" + kind)


@pytest.mark.parametrize("policy", ["midpoint", "any"])
@pytest.mark.parametrize("kind", ["plain", "bam"])
def test_weighted_sums_equal_the_restatement(engine, sums_world, kind, policy):
    import torch
    key, cols = "gw:sums:" + kind, sums_world["cols"][kind]
    assert engine.is_bam(key) == (kind == "bam")
    for tag, w in list(sums_world["weights"].items()) + [("device", sums_world["weights"]["random"][::-1].copy())]:
        if tag == "device":
            dev = torch.from_numpy(w.view(np.int32)).to("cuda:0")
            engine.set_weights(key, dev)
            engine.sync()
            del dev
        else:
            engine.set_weights(key, w)
        assert np.array_equal(engine.weights(key), w)
        for mapq_min, min_len, max_len in FILTERS:
            for name, (starts, stops) in sums_world["sets"].items():
                if len(starts) > 1000 and tag not in ("random", "unit"):
                    continue
                want = restated_sums(cols, w, starts, stops, mapq_min, min_len, max_len, policy, kind == "bam")
                got = engine.weighted_window_sums(key, starts, stops, mapq_min, min_len, max_len, policy)
                assert got[0].dtype == np.int64 and got[1].dtype == np.int64
                bad = np.flatnonzero((got[0] != want[0]) | (got[1] != want[1]))
                assert len(bad) == 0, (tag, name, mapq_min, bad[:5], got[0][bad[:5]], want[0][bad[:5]], got[1][bad[:5]], want[1][bad[:5]])
                if tag == "unit":  # the predicate is window_counts'
                    counts = engine.window_counts(key, starts, stops, mapq_min, min_len, max_len, policy)
                    assert np.array_equal(got[0], ONE * counts) and np.array_equal(got[1], counts), name
                if tag == "all_zero":
                    assert not got[0].any() and not got[1].any()
    # the cases are what they are meant to be
    sets, unit = sums_world["sets"], sums_world["weights"]["unit"]
    c = lambda name: restated_sums(cols, unit, *sets[name], 0, None, None, policy, kind == "bam")[1]  # noqa: E731
    assert c("whole")[0] > N_DUP and c("chunks")[0] > CHUNK and c("chunks")[1] == 0 and not c("behind")[:3].any()
    assert len(sets["above_s"][0]) == 4 * sums_world["n_cu"] + 1 and c("above_s").sum() > N_DUP
    assert len(set(c("on_bounds").tolist())) > 3 and c("empty")[2] == 0 and c("unsorted")[0] == c("unsorted")[2] > 0
    k = 2 if policy == "any" else 3  # the window in which the copies' read1, at their far end, decides
    assert (c("chunks")[k] < 1000) == (kind == "bam") and (c("chunks")[k] > N_DUP) == (kind == "plain")


def test_sums_pass_2_to_the_48(engine, sums_world):
    key, cols = "gw:sums:plain", sums_world["cols"]["plain"]
    w = np.full(len(cols[0]), U32_MAX, np.uint32)
    engine.set_weights(key, w)
    for starts, stops in (([None], [None]), ([900, 0], [1_300, 41_000])):
        sums, cnt = engine.weighted_window_sums(key, starts, stops, 0)
        want = restated_sums(cols, w, starts, stops, 0, None, None, "midpoint", False)
        assert np.array_equal(sums, want[0]) and np.array_equal(cnt, want[1])
        assert sums[0] >= N_DUP * U32_MAX > 2 ** 48 and cnt[0] >= N_DUP


def test_empty_contig_and_no_windows(engine, sums_world):
    z = np.zeros(0, np.int32)
    engine.load_contig("gw:empty", z, z, np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    try:
        engine.set_weights("gw:empty", np.zeros(0, np.uint32))
        assert len(engine.weights("gw:empty")) == 0
        sums, cnt = engine.weighted_window_sums("gw:empty", [None, 0, 5], [None, 100, 5], 0)
        assert sums.tolist() == [0, 0, 0] and cnt.tolist() == [0, 0, 0]
        sums, cnt = engine.weighted_window_sums("gw:empty", [], [])
        assert len(sums) == 0 and len(cnt) == 0
    finally:
        engine.release("gw:empty")
    engine.set_weights("gw:sums:plain", sums_world["weights"]["unit"])
    sums, cnt = engine.weighted_window_sums("gw:sums:plain", [], [])
    assert sums.shape == (0,) and cnt.shape == (0,)
    # n_weighted_out may be NULL
    from finaletoolkit_amd import _lib as L
    ws, we, out = np.array([0], np.int32), np.array([41_000], np.int32), np.full(1, 7, np.int64)
    f = L.make_filter(0)
    assert engine.lib.ftk_weighted_window_sums(engine.ctx, engine.contig_id("gw:sums:plain"), L.ptr(ws), L.ptr(we), 1,
                                               C.byref(f), L.ptr(out), None) == L.FTK_OK
    assert out[0] == ONE * engine.window_counts("gw:sums:plain", [0], [41_000], 0)[0] > 0


# ---- 3. life cycle -----------------------------------------------------------------------------------------------------------
def test_life_cycle(engine):
    import torch
    from finaletoolkit_amd import _lib as L
    s = np.arange(0, 3000, 3, dtype=np.int32)
    cols = (s, s + 150, np.full(len(s), 60, np.uint8), np.zeros(len(s), np.uint8))
    engine.load_contig("gw:life", *cols)
    try:
        for call in (lambda: engine.weights("gw:life"), lambda: engine.weighted_window_sums("gw:life", [0], [100])):
            with pytest.raises(L.FtkError, match="weights"):
                call()
        for bad in (len(s) - 1, len(s) + 1, 0):
            with pytest.raises(L.FtkError):
                engine.set_weights("gw:life", np.ones(bad, np.uint32))
        with pytest.raises(L.FtkError, match="weights"):  # a refused column attaches nothing
            engine.weights("gw:life")
        w = (np.arange(len(s), dtype=np.uint32) * 2_654_435_761).astype(np.uint32)
        engine.set_weights("gw:life", w)
        assert np.array_equal(engine.weights("gw:life"), w)
        # readback into a device tensor with guard elements on both sides
        buf = torch.full((len(s) + 2,), -7, dtype=torch.int32, device="cuda:0")
        engine.weights("gw:life", out=buf[1:1 + len(s)])
        engine.sync()
        host = buf.cpu().numpy()
        assert np.array_equal(host[1:-1].view(np.uint32), w) and host[0] == -7 and host[-1] == -7
        # released and loaded again under the same name: the column is gone
        engine.release("gw:life")
        engine.load_contig("gw:life", *cols)
        with pytest.raises(L.FtkError, match="weights"):
            engine.weights("gw:life")
        with pytest.raises(L.FtkError, match="weights"):
            engine.weighted_window_sums("gw:life", [0], [100])
        # and loaded again over a resident contig (the same id): gone as well
        engine.set_weights("gw:life", w)
        engine.load_contig("gw:life", *cols)
        with pytest.raises(L.FtkError, match="weights"):
            engine.weights("gw:life")
    finally:
        engine.release("gw:life")


# ---- 4. the C ABI's argument errors ----------------------------------------------------------------------------------------
def test_argument_errors(engine, world):
    from finaletoolkit_amd import _lib as L
    lib, ctx = engine.lib, engine.ctx
    rid = rid_of(engine, world, "2bit", "wA")
    cid = engine.contig_id("gw:wA")
    n = len(world["cols"]["wA"][0])
    engine.set_weights("gw:wA", np.full(n, 5, np.uint32))
    table = np.full((1000, 1001), 9, np.uint32)
    w_out = np.full(n, 7, np.uint32)
    sums, cnt = np.full(4, 7, np.int64), np.full(4, 7, np.int64)
    ws, we = np.array([0, 10, 20, 30], np.int32), np.array([100, 110, 120, 130], np.int32)
    nz = C.c_int64(7)
    f = L.make_filter(30)
    INV, NOC = L.FTK_ERR_INVALID, L.FTK_ERR_NO_CONTIG

    def failed(rc, code):
        assert rc == code, (rc, code)
        assert lib.ftk_last_error(ctx)

    P = L.ptr
    assert lib.ftk_frags_set_weights(None, cid, P(w_out), n) == INV
    assert lib.ftk_frags_weights(None, cid, P(w_out)) == INV
    assert lib.ftk_frags_set_gc_weights(None, cid, rid, 100, 220, 30, P(table), C.byref(nz)) == INV
    assert lib.ftk_weighted_window_sums(None, cid, P(ws), P(we), 4, C.byref(f), P(sums), P(cnt)) == INV
    failed(lib.ftk_frags_set_weights(ctx, cid, None, n), INV)
    failed(lib.ftk_frags_weights(ctx, cid, None), INV)
    failed(lib.ftk_frags_set_gc_weights(ctx, cid, rid, 100, 220, 30, None, C.byref(nz)), INV)
    failed(lib.ftk_frags_set_gc_weights(ctx, cid, rid, 100, 220, 30, P(table), None), INV)
    failed(lib.ftk_weighted_window_sums(ctx, cid, None, P(we), 4, C.byref(f), P(sums), P(cnt)), INV)
    failed(lib.ftk_weighted_window_sums(ctx, cid, P(ws), None, 4, C.byref(f), P(sums), P(cnt)), INV)
    failed(lib.ftk_weighted_window_sums(ctx, cid, P(ws), P(we), 4, None, P(sums), P(cnt)), INV)
    failed(lib.ftk_weighted_window_sums(ctx, cid, P(ws), P(we), 4, C.byref(f), None, P(cnt)), INV)
    failed(lib.ftk_weighted_window_sums(ctx, cid, P(ws), P(we), -1, C.byref(f), P(sums), P(cnt)), INV)
    bad_policy = L.Filter(30, -1, -1, 7, 0)
    failed(lib.ftk_weighted_window_sums(ctx, cid, P(ws), P(we), 4, C.byref(bad_policy), P(sums), P(cnt)), INV)
    read1 = L.Filter(30, -1, -1, 0, L.FETCH_BAM_READ1)  # a contig without read1 columns
    failed(lib.ftk_weighted_window_sums(ctx, cid, P(ws), P(we), 4, C.byref(read1), P(sums), P(cnt)), INV)
    failed(lib.ftk_frags_set_weights(ctx, 987_654, P(w_out), n), NOC)
    failed(lib.ftk_frags_weights(ctx, 987_654, P(w_out)), NOC)
    failed(lib.ftk_frags_set_gc_weights(ctx, 987_654, rid, 100, 220, 30, P(table), C.byref(nz)), NOC)
    failed(lib.ftk_frags_set_gc_weights(ctx, cid, 987_654, 100, 220, 30, P(table), C.byref(nz)), NOC)
    failed(lib.ftk_weighted_window_sums(ctx, 987_654, P(ws), P(we), 4, C.byref(f), P(sums), P(cnt)), NOC)
    for lo, hi in ((0, 220), (221, 220), (100, 1001)):
        failed(lib.ftk_frags_set_gc_weights(ctx, cid, rid, lo, hi, 30, P(table), C.byref(nz)), INV)
    bare = engine.ref_upload(("gw-test", "bare"), np.zeros(64, np.uint8), 1)  # an image without its layout
    failed(lib.ftk_frags_set_gc_weights(ctx, cid, bare, 100, 220, 30, P(table), C.byref(nz)), INV)
    assert b"layout" in lib.ftk_last_error(ctx)
    # nothing was written by any of them, and the column attached before them is still the contig's
    assert np.all(w_out == 7) and np.all(sums == 7) and np.all(cnt == 7) and nz.value == 7
    assert np.all(engine.weights("gw:wA") == 5)


# ---- 5. the product path -----------------------------------------------------------------------------------------------------
def restated_coverage(world, frags, intervals, bias_table, lo, hi, min_bias, mapq_min=30, bam=False):
    """(count, units, n_weighted, n_zero) of the intervals from ``{contig: rows}`` (rows: start, end, mapq[, fwd, r1s, r1e])."""
    from finaletoolkit_amd import utils
    table = utils.gc_weights(bias_table, min_bias)
    count, units, nw = (np.zeros(len(intervals), np.int64) for _ in range(3))
    n_zero, done = 0, set()
    for i, (c, a, b, _) in enumerate(intervals):
        rows = frags[c]
        s, e, q = (np.asarray(rows[k], np.int64) for k in range(3))
        ln = e - s
        rule = (q >= mapq_min) & (ln >= lo) & (ln <= hi)
        w = np.zeros(len(s), np.int64)
        if c in world["contigs"]:
            gc = world["contigs"][c].gc(s, e)
            ok = rule & (gc >= 0)
            w[ok] = table[ln[ok] - lo, gc[ok]]
            if c not in done:
                n_zero += int((rule & (w == 0)).sum())
                done.add(c)
        mid = (s + e) // 2
        m = rule & (mid >= a) & (mid < b)
        if bam:
            m &= (np.asarray(rows[4], np.int64) < b) & (np.asarray(rows[5], np.int64) > a)
        count[i], units[i], nw[i] = m.sum(), w[m].sum(), (w[m] > 0).sum()
    return count, units, nw, n_zero


def same_coverage(a, b):
    return (a.intervals == b.intervals and np.array_equal(a.count, b.count) and np.array_equal(a.corrected, b.corrected, equal_nan=True)
            and np.array_equal(a.n_weighted, b.n_weighted) and a.n_zero == b.n_zero and a.skipped_contigs == b.skipped_contigs)


def test_frag_gc_coverage_end_to_end(engine, world, tmp_path):
    from finaletoolkit_amd import utils
    rng = np.random.default_rng(78)
    contigs = [("wA", LAYOUT["wA"][0]), ("wX", 9_000), ("wC", LAYOUT["wC"][0])]
    frags = {}
    for name, n in contigs:
        a = np.sort(rng.integers(0, n - 400, 1500))
        ln = rng.integers(90, 240, 1500)
        frags[name] = (a, a + ln, rng.choice([0, 10, 29, 30, 42, 60], 1500), rng.integers(0, 2, 1500))
    bam = str(tmp_path / "in.bam")
    write_synthetic_bam(bam, contigs, frags)
    frag = str(tmp_path / "in.frag.gz")
    utils.frag_export(bam, frag, quality_threshold=0)
    ref = world["paths"]["2bit"]
    # lengths up to 199: the midpoint of such a fragment lies inside its 100-base read1, so the BAM's read1 fetch rule and
    # the fragment file's overlap rule select the same fragments for every interval
    lo, hi, stride = 100, 199, 3
    rows = []
    for name, n in contigs:
        rows += [(name, a, min(a + 3_000, n), f"{name}_{a}") for a in range(0, n, 3_000)]
    rows += [("wA", 10_000, 10_001, "one_base"), ("wC", 137, 40_999, "."), ("wA", 20_100, 20_200, "in_the_n_run")]
    order = rng.permutation(len(rows))
    intervals = [rows[i] for i in order]
    bed = str(tmp_path / "bins.bed")
    with open(bed, "w") as fh:
        fh.write("# intervals\n" + "".join(f"{c}\t{a}\t{b}" + ("" if nm == "." else f"\t{nm}") + "\n" for c, a, b, nm in intervals))
    kw = dict(min_length=lo, max_length=hi, stride=stride)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        bias = utils.frag_gc_bias(frag, ref, str(tmp_path / "bias.tsv.gz"), **kw)
    results = {}
    for tag, path in (("bam", bam), ("frag", frag)):
        for how, given in (("none", None), ("table", bias), ("tsv", str(tmp_path / "bias.tsv.gz"))):
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                results[tag, how] = utils.frag_gc_coverage(path, ref, bed, bias=given, **kw)
            ours = [w for w in caught if issubclass(w.category, UserWarning) and "not in the reference" in str(w.message)]
            assert len(ours) == 1 and "wX" in str(ours[0].message), [str(w.message) for w in caught]
    res = results["frag", "none"]
    for k, other in results.items():
        assert same_coverage(res, other), k
    assert res.intervals == intervals and res.skipped_contigs == ("wX",)
    assert res.count.dtype == np.int64 and res.n_weighted.dtype == np.int64 and res.corrected.dtype == np.float64
    want_bam = bam_expected(bam)[0]
    want_frag = read_frag_gz(frag)
    for want, is_bam in ((want_frag, False), (want_bam, True)):
        count, units, nw, n_zero = restated_coverage(world, want, intervals, utils.gc_bias_ratio(bias.observed, bias.expected),
                                                     lo, hi, 0.05, bam=is_bam)
        assert np.array_equal(res.count, count) and np.array_equal(res.n_weighted, nw) and res.n_zero == n_zero
        on_ref = np.array([c != "wX" for c, _, _, _ in intervals])
        assert np.array_equal(res.corrected[on_ref], units[on_ref] / 65536.0) and np.isnan(res.corrected[~on_ref]).all()
        assert (~on_ref).sum() == 3 and res.count[~on_ref].sum() > 100 and not res.n_weighted[~on_ref].any()
    assert res.n_zero > 0 and res.n_weighted.sum() > 500
    # the bias restated from the genome: the same table
    obs = np.zeros_like(bias.observed)
    for c in ("wA", "wC"):
        s, e, q = (np.asarray(want_frag[c][k], np.int64) for k in range(3))
        keep = (q >= 30) & (e - s >= lo) & (e - s <= hi)
        gc = world["contigs"][c].gc(s[keep], e[keep])
        np.add.at(obs, ((e - s)[keep][gc >= 0] - lo, gc[gc >= 0]), 1)
    exp = sum(world["contigs"][c].expected(lo, hi, stride) for c in ("wA", "wC"))
    assert np.array_equal(bias.observed, obs) and np.array_equal(bias.expected, exp)
    # a GCBias of other lengths; an interval on a contig the input lacks
    with pytest.raises(ValueError, match="lengths"):
        utils.frag_gc_coverage(frag, ref, bed, bias=bias, min_length=lo, max_length=hi + 1)
    bed13 = str(tmp_path / "bins13.bed")
    open(bed13, "w").write("wA\t0\t100\n13\t0\t100\n")
    with pytest.raises(ValueError, match="contig not present"):
        utils.frag_gc_coverage(frag, ref, bed13, bias=bias, **kw)
    # the files, field by field, and the command line in a child process
    for suffix in (".bed", ".bed.gz"):
        out = str(tmp_path / ("fn" + suffix))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            again = utils.frag_gc_coverage(frag, ref, bed, out, bias=bias, **kw)
        assert same_coverage(again, res)
        text = gzip.open(out, "rt").read() if suffix.endswith(".gz") else open(out).read()
        lines = text.splitlines()
        assert len(lines) == len(intervals)
        for ln, (c, a, b, nm), k, x in zip(lines, intervals, res.count, res.corrected):
            f = ln.split("\t")
            assert f[:5] == [c, str(a), str(b), nm, str(int(k))]
            assert f[5] == ("nan" if c == "wX" else format(float(x), ".6f")) and len(f) == 6
        cli = str(tmp_path / ("cli" + suffix))
        r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.gccov", frag, ref, bed, cli, "--bias", str(tmp_path / "bias.tsv.gz"),
                            "--min-length", str(lo), "--max-length", str(hi), "-q", "30"], cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert "wX" in r.stderr  # the warning
        if suffix == ".bed":
            assert open(cli, "rb").read() == open(out, "rb").read()
        else:
            assert gzip.open(cli, "rb").read() == gzip.open(out, "rb").read()
