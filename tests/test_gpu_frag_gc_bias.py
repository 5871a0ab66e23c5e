"""GPU: the fragment length x GC tables (``csrc/ftk_gcbias.hip``) - ``Engine.frag_gc``, ``Engine.frag_gc_table`` and
``Engine.ref_gc_table`` against a numpy restatement written here (``cumsum`` of is-GC and is-N over the sequence string,
``np.bincount`` per length), exactly equal everywhere: on a 2bit image and two FASTA images of one genome, at the
contigs' and the N runs' edges, at every word alignment, on both sides of each kernel's LDS limit, above the 16-bit
range; the C ABI's argument errors; and ``frag_gc_bias`` / the command line on a synthetic BAM and its fragment file."""
import ctypes as C
import gzip
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests.helpers import bam_expected, read_frag_gz, write_2bit, write_fasta, write_synthetic_bam

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096           # kGcRefTile: positions per tile of the expected table
MAX_LEN = 1000        # FTK_GC_MAX_LEN
R0 = 10_007           # the ranges' start: no multiple of the tile or of a stride
STRIDES = (1, 3, 64, 1009)
assert all(R0 % k for k in (TILE, 3, 64, 1009))
# the observed table keeps its rows in LDS while they fit 32 768 packed cells (row L: L + 1 cells): (1, 254) fits
# whole, (1, 255) leaves its last row - and (1, 1000) most rows - to global atomics; the expected table cuts its rows
# into chunks of at most 28 672 packed cells: (1, 237) is one chunk, (1, 238) two, (1, 1000) nineteen
assert 255 * 256 // 2 - 1 <= 32_768 < 256 * 257 // 2 - 1 and 238 * 239 // 2 - 1 <= 28_672 < 239 * 240 // 2 - 1
FRAG_PAIRS = ((100, 220), (1, 64), (167, 167), (1, 1000), (1, 254), (1, 255))
IMAGES = ("2bit", "fa60", "fa50")


# ---- the genome ------------------------------------------------------------------------------------------------------
def make_contig(rng, n, n_runs, lower_runs):
    s = rng.choice(np.frombuffer(b"ACGT", np.uint8), n, p=[0.3, 0.2, 0.2, 0.3])
    for a, b in lower_runs:
        s[a:b] |= 0x20
    for a, b in n_runs:
        s[a:b] = ord("N")
    return s.tobytes().decode()


LAYOUT = {  # name: (length, N runs, lower-case runs); no length a multiple of 60 or 50
    "cA": (30_011, ((0, 137), (15_000, 15_001), (20_000, 20_250)), ((5_000, 5_600), (20_100, 20_400))),
    "cB": (23_457, ((9_000, 9_017), (23_157, 23_457)), ((1_000, 1_900),)),
    "cC": (41_003, ((12_345, 12_346), (30_000, 31_100)), ((2_000, 2_700), (40_000, 41_003))),
    "cS": (37, (), ((10, 20),)),
}
DUP_LEN = {"cA": 150, "cB": 40, "cC": 300}  # 70 000 copies: a cell of LDS rows, of the (1, 64) rows, of the global rows


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

    def expected(self, pos_lo, pos_hi, len_lo, len_hi, stride):
        table = np.zeros((len_hi - len_lo + 1, len_hi + 1), np.int64)
        p = np.arange(-(-pos_lo // stride) * stride, min(pos_hi, self.n), stride, dtype=np.int64)
        for L in range(len_lo, len_hi + 1):
            q = p[p + L <= self.n]
            q = q[self.cn[q + L] - self.cn[q] == 0]
            table[L - len_lo] = np.bincount(self.cg[q + L] - self.cg[q], minlength=len_hi + 1)
        return table


def fragments_of(ct, rng):
    """(start, end, mapq) of one contig: random fragments and the hand-placed ones."""
    n, name = ct.n, ct.name
    s, e, q = [], [], []

    def add(a, b, mq=60):
        s.append(int(a)), e.append(int(b)), q.append(int(mq))

    if n > 1000:
        a = rng.integers(0, n - 10, 4000)
        for x, ln, mq in zip(a, rng.integers(20, 601, 4000), rng.integers(0, 61, 4000)):
            add(x, x + ln, mq)
    lengths = sorted({lo - 1 for lo, _ in FRAG_PAIRS} | {v for pair in FRAG_PAIRS for v in pair} | {hi + 1 for _, hi in FRAG_PAIRS}
                     | {1000, 1001, 40_000})
    assert {0, 99, 100, 220, 221, 1000, 1001, 40_000} <= set(lengths)
    for ln in lengths:
        for a in (0, 1, 777, n - ln, n - ln + 1):  # (n - ln: end = chrom_len; + 1: one base beyond)
            if a >= 0:
                add(a, a + ln)
    for ln in (1, 37, 150):
        add(0, ln), add(n - ln, n), add(n - ln + 1, n + 1), add(n - 10, n - 10 + ln + 5000), add(n + 1000, n + 1000 + ln)
        add(n, n + ln), add(n - 50, n + 100)
    for k in range(4):
        for ln in (15, 16, 17, 31, 32, 33, 63, 64, 65):
            add(2000 + k, 2000 + k + ln) if n > 3000 else add(k, k + ln)
    n_runs, lower_runs = LAYOUT[name][1], LAYOUT[name][2]
    for a0, a1 in n_runs:
        for ln in (20, 150, 167):
            add(a0 - ln, a0), add(a0 - ln + 1, a0 + 1)          # last base: the base before the run / the first N
            add(a1 - 1, a1 - 1 + ln), add(a1, a1 + ln)          # first base: the last N / the base after the run
            add(a0 + 1, a0 + 1 + ln), add(a0 - 5, a0 - 5 + ln)  # from inside the run, across its first base
        if a1 - a0 + 60 <= MAX_LEN:
            add(a0 - 30, a1 + 30), add(a0 - 1, a1 + 1), add(a0, a1)
    for a0, a1 in lower_runs:
        add(a0 + 3, min(a0 + 153, a1)), add(a0, a1) if a1 - a0 <= MAX_LEN else None
        add(a0 - 20, a0 + 130)
    for mq in (0, 29, 30, 31, 255):  # both sides of the threshold
        add(min(3000, n // 2), min(3000, n // 2) + min(167, n // 2), mq)
    if name in DUP_LEN:
        s += [1000] * 70_000
        e += [1000 + DUP_LEN[name]] * 70_000
        q += [60] * 70_000
    s, e, q = np.array(s, np.int64), np.array(e, np.int64), np.array(q, np.int64)
    keep = (s >= 0) & (e < 1 << 30)  # (fragments that would start before the contig cannot be loaded)
    s, e, q = s[keep], e[keep], q[keep]
    o = np.argsort(s, kind="stable")
    return s[o].astype(np.int32), e[o].astype(np.int32), q[o].astype(np.uint8)


@pytest.fixture(scope="module")
def world(engine, tmp_path_factory):
    from finaletoolkit_amd.reference import ReferenceGenome
    d = tmp_path_factory.mktemp("gcbias")
    rng = np.random.default_rng(20261018)
    seqs = {name: make_contig(rng, n, n_runs, lower) for name, (n, n_runs, lower) in LAYOUT.items()}
    assert seqs["cA"].startswith("N" * 137 + seqs["cA"][137]) and seqs["cB"].endswith("N" * 300) and seqs["cC"][12_345] == "N"
    assert all(len(s) % 60 and len(s) % 50 for s in seqs.values())
    paths = {"2bit": str(d / "g.2bit"), "fa60": str(d / "g60.fa"), "fa50": str(d / "g50.fa")}
    write_2bit(paths["2bit"], seqs)
    write_fasta(paths["fa60"], seqs, width=60)
    write_fasta(paths["fa50"], seqs, width=50)
    w = dict(dir=d, seqs=seqs, paths=paths, refs={k: ReferenceGenome(p) for k, p in paths.items()},
             contigs={name: Contig(name, s) for name, s in seqs.items()}, cols={}, want_gc={})
    for name, ct in w["contigs"].items():
        cols = fragments_of(ct, rng)
        engine.load_contig("gc:" + name, *cols, np.zeros(len(cols[0]), np.uint8))
        w["cols"][name] = cols
        w["want_gc"][name] = ct.gc(cols[0], cols[1])  # before the MAPQ / length rule
    yield w
    for name in w["contigs"]:
        engine.release("gc:" + name)
    for r in w["refs"].values():
        r.close()


def rid_of(engine, world, image, name):
    return world["refs"][image].device_image(engine, name, with_layout=True)


def restated_frag_gc(world, name, mapq_min=30, min_len=None, max_len=None):
    s, e, q = world["cols"][name]
    ln = e.astype(np.int64) - s
    keep = q >= mapq_min
    if min_len is not None:
        keep &= ln >= min_len
    if max_len is not None:
        keep &= ln <= max_len
    return np.where(keep, world["want_gc"][name], -1).astype(np.int16), keep, ln


# ---- 1. gc per fragment ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image", IMAGES)
def test_frag_gc_equals_the_restatement(engine, world, image):
    for name in LAYOUT:
        rid = rid_of(engine, world, image, name)
        for args in ((30, None, None), (0, None, None), (30, 100, 220), (31, 1, 1000), (0, 168, 167), (0, 1001, None)):
            want, keep, ln = restated_frag_gc(world, name, *args)
            got = engine.frag_gc("gc:" + name, rid, *args)
            assert got.dtype == np.int16 and got.shape == want.shape
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, (name, args, bad[:5], world["cols"][name][0][bad[:5]], world["cols"][name][1][bad[:5]],
                                   got[bad[:5]], want[bad[:5]])
        want, keep, ln = restated_frag_gc(world, name, 30)
        if name != "cS":  # the hand-placed cases are there and do what they are for
            assert (want >= 0).sum() > 70_000 and ((want < 0) & keep & (ln <= MAX_LEN) & (ln > 0)).sum() > 20
            assert want[(ln > MAX_LEN) | (ln < 1)].max() == -1 and want[ln == MAX_LEN].max() > 0


def test_frag_gc_into_a_device_array(engine, world):
    import torch
    want, _, _ = restated_frag_gc(world, "cB", 30)
    buf = torch.full((len(want) + 2,), -7, dtype=torch.int16, device="cuda:0")
    engine.frag_gc("gc:cB", rid_of(engine, world, "2bit", "cB"), 30, out=buf[1:1 + len(want)])
    engine.sync()
    host = buf.cpu().numpy()
    assert np.array_equal(host[1:-1], want) and host[0] == -7 and host[-1] == -7


# ---- 2. the observed table -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image", IMAGES)
@pytest.mark.parametrize("len_lo, len_hi", FRAG_PAIRS)
def test_frag_gc_table_is_the_bincount(engine, world, image, len_lo, len_hi):
    for name in LAYOUT:
        rid = rid_of(engine, world, image, name)
        gc, keep, ln = restated_frag_gc(world, name, 30, len_lo, len_hi)
        want = np.zeros((len_hi - len_lo + 1, len_hi + 1), np.int64)
        ok = gc >= 0
        np.add.at(want, (ln[ok] - len_lo, gc[ok].astype(np.int64)), 1)
        table, skipped = engine.frag_gc_table("gc:" + name, rid, len_lo, len_hi, 30)
        assert table.dtype == np.int64 and table.shape == want.shape
        assert np.array_equal(table, want), (name, np.argwhere(table != want)[:5])
        assert skipped == int((keep & ~ok).sum())
        assert np.array_equal(table, np.array([np.bincount(gc[ok & (ln == L)], minlength=len_hi + 1) for L in range(len_lo, len_hi + 1)]))
        if name in DUP_LEN and len_lo <= DUP_LEN[name] <= len_hi:
            assert table[DUP_LEN[name] - len_lo].max() > 65_535
        if name != "cS" and len_hi >= 255:  # cells of both kinds of rows are in use
            assert table[:254 - len_lo + 1].any() and table[255 - len_lo:].any()


def test_tables_overwrite_what_the_caller_passed(engine, world):
    from finaletoolkit_amd import _lib as L
    rid = rid_of(engine, world, "2bit", "cA")
    cid = engine.contig_id("gc:cA")
    table = np.full((121, 221), 7, np.int64)
    skipped = C.c_int64(7)
    assert engine.lib.ftk_frag_gc_table(engine.ctx, cid, rid, 100, 220, 30, L.ptr(table), C.byref(skipped)) == L.FTK_OK
    want, want_skipped = engine.frag_gc_table("gc:cA", rid, 100, 220, 30)
    assert np.array_equal(table, want) and skipped.value == want_skipped and (table == 0).sum() > 10_000
    table[:] = 7
    assert engine.lib.ftk_ref_gc_table(engine.ctx, rid, 0, 30_011, 100, 220, 1, L.ptr(table)) == L.FTK_OK
    assert np.array_equal(table, world["contigs"]["cA"].expected(0, 30_011, 100, 220, 1))
    # an empty contig and an empty range: zeros
    engine.load_contig("gc:empty", np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    table[:] = 7
    t, sk = engine.frag_gc_table("gc:empty", rid, 100, 220, 30)
    assert not t.any() and sk == 0 and len(engine.frag_gc("gc:empty", rid)) == 0
    engine.release("gc:empty")
    for lo, hi in ((5, 5), (30_011, 40_000), (1 << 40, 1 << 41)):
        assert not engine.ref_gc_table(rid, lo, hi, 100, 220).any()


# ---- 3. the expected table -----------------------------------------------------------------------------------------------
def ranges_of(n):
    return [(0, n), (0, n + 500)] + [(R0, R0 + k) for k in (1, TILE - 1, TILE, TILE + 1, 2 * TILE, 3 * TILE + 5)]


@pytest.mark.parametrize("stride", STRIDES)
def test_ref_gc_table_ranges_and_strides(engine, world, stride):
    ct = world["contigs"]["cC"]
    rid = rid_of(engine, world, "2bit", "cC")
    for lo, hi in ranges_of(ct.n):
        want = ct.expected(lo, hi, 100, 220, stride)
        got = engine.ref_gc_table(rid, lo, hi, 100, 220, stride)
        assert got.dtype == np.int64 and np.array_equal(got, want), (lo, hi, np.argwhere(got != want)[:5])
        # row sums: the sampled positions whose window of that length lies inside the contig and holds no N
        p = np.arange(-(-lo // stride) * stride, min(hi, ct.n), stride)
        for L in (100, 167, 220):
            inside = p[p + L <= ct.n]
            assert got[L - 100].sum() == int((ct.cn[inside + L] == ct.cn[inside]).sum())
    assert engine.ref_gc_table(rid, 0, ct.n, 100, 220, stride).sum() > 0


@pytest.mark.parametrize("len_lo, len_hi", [(1, 64), (167, 167), (1, 237), (1, 238), (1, 1000)])
def test_ref_gc_table_lengths(engine, world, len_lo, len_hi):
    ct = world["contigs"]["cA"]
    rid = rid_of(engine, world, "2bit", "cA")
    for lo, hi, stride in ((0, ct.n + 500, 3), (R0, R0 + TILE + 1, 1)):
        got = engine.ref_gc_table(rid, lo, hi, len_lo, len_hi, stride)
        assert np.array_equal(got, ct.expected(lo, hi, len_lo, len_hi, stride))
        assert got[0].sum() > 0 and got[-1].sum() > 0


@pytest.mark.parametrize("name", list(LAYOUT))
def test_ref_gc_table_images_agree_and_halves_add_up(engine, world, name):
    ct = world["contigs"][name]
    m = 12_347 if ct.n > 12_347 else 17
    assert all(m % k for k in (*STRIDES[1:], TILE))
    for stride in STRIDES:
        want = ct.expected(0, ct.n, 100, 220, stride)
        for image in IMAGES:
            rid = rid_of(engine, world, image, name)
            whole = engine.ref_gc_table(rid, 0, ct.n, 100, 220, stride)
            assert np.array_equal(whole, want), (image, stride)
            halves = engine.ref_gc_table(rid, 0, m, 100, 220, stride) + engine.ref_gc_table(rid, m, ct.n, 100, 220, stride)
            assert np.array_equal(halves, whole), (image, stride)
        if name == "cS":  # shorter than every length
            assert not want.any()
    if name == "cS":
        rid = rid_of(engine, world, "fa50", name)
        got = engine.ref_gc_table(rid, 0, ct.n, 1, 37)
        assert np.array_equal(got, ct.expected(0, ct.n, 1, 37, 1)) and got[36].sum() == 1 and got[0].sum() == 37


# ---- 4. the C ABI's argument errors ------------------------------------------------------------------------------------
def test_argument_errors(engine, world):
    from finaletoolkit_amd import _lib as L
    lib, ctx = engine.lib, engine.ctx
    rid = rid_of(engine, world, "2bit", "cA")
    cid = engine.contig_id("gc:cA")
    n = len(world["cols"]["cA"][0])
    gc = np.full(n, 7, np.int16)
    table = np.full((1000, 1001), 7, np.int64)
    sk = C.c_int64(7)
    INV, NOC = L.FTK_ERR_INVALID, L.FTK_ERR_NO_CONTIG

    def failed(rc, code):
        assert rc == code, (rc, code)
        if ctx is not None:
            assert lib.ftk_last_error(ctx)

    assert lib.ftk_frag_gc(None, cid, rid, -1, -1, 30, L.ptr(gc)) == INV
    assert lib.ftk_frag_gc_table(None, cid, rid, 100, 220, 30, L.ptr(table), C.byref(sk)) == INV
    assert lib.ftk_ref_gc_table(None, rid, 0, 100, 100, 220, 1, L.ptr(table)) == INV
    failed(lib.ftk_frag_gc(ctx, cid, rid, -1, -1, 30, None), INV)
    failed(lib.ftk_frag_gc_table(ctx, cid, rid, 100, 220, 30, None, C.byref(sk)), INV)
    failed(lib.ftk_frag_gc_table(ctx, cid, rid, 100, 220, 30, L.ptr(table), None), INV)
    failed(lib.ftk_ref_gc_table(ctx, rid, 0, 100, 100, 220, 1, None), INV)
    failed(lib.ftk_frag_gc(ctx, 987_654, rid, -1, -1, 30, L.ptr(gc)), NOC)
    failed(lib.ftk_frag_gc(ctx, cid, 987_654, -1, -1, 30, L.ptr(gc)), NOC)
    failed(lib.ftk_frag_gc_table(ctx, 987_654, rid, 100, 220, 30, L.ptr(table), C.byref(sk)), NOC)
    failed(lib.ftk_frag_gc_table(ctx, cid, 987_654, 100, 220, 30, L.ptr(table), C.byref(sk)), NOC)
    failed(lib.ftk_ref_gc_table(ctx, 987_654, 0, 100, 100, 220, 1, L.ptr(table)), NOC)
    for lo, hi in ((0, 220), (-1, 220), (221, 220), (100, 1001), (1001, 1001)):
        failed(lib.ftk_frag_gc_table(ctx, cid, rid, lo, hi, 30, L.ptr(table), C.byref(sk)), INV)
        failed(lib.ftk_ref_gc_table(ctx, rid, 0, 100, lo, hi, 1, L.ptr(table)), INV)
    for stride in (0, -1):
        failed(lib.ftk_ref_gc_table(ctx, rid, 0, 100, 100, 220, stride, L.ptr(table)), INV)
    for lo, hi in ((-1, 100), (100, 99)):
        failed(lib.ftk_ref_gc_table(ctx, rid, lo, hi, 100, 220, 1, L.ptr(table)), INV)
    with pytest.raises(L.FtkError):
        engine.ref_gc_table(rid, 0, 100, 0, 0)
    with pytest.raises(L.FtkError):
        engine.frag_gc_table("gc:cA", rid, 5, 4)
    # an image without its layout
    bare = engine.ref_upload(("gc-test", "bare"), np.zeros(64, np.uint8), 1)
    failed(lib.ftk_frag_gc(ctx, cid, bare, -1, -1, 30, L.ptr(gc)), INV)
    assert b"layout" in lib.ftk_last_error(ctx)
    failed(lib.ftk_frag_gc_table(ctx, cid, bare, 100, 220, 30, L.ptr(table), C.byref(sk)), INV)
    failed(lib.ftk_ref_gc_table(ctx, bare, 0, 100, 100, 220, 1, L.ptr(table)), INV)
    assert b"layout" in lib.ftk_last_error(ctx)
    # nothing was written by any of them
    assert np.all(gc == 7) and np.all(table == 7) and sk.value == 7


# ---- 5. the product path -----------------------------------------------------------------------------------------------
def restated_result(world, frags, len_lo, len_hi, stride=1, mapq_min=30):
    """(observed, expected, n_skipped) over ``{contig: (start, end, mapq)}`` for the contigs the reference holds."""
    shape = (len_hi - len_lo + 1, len_hi + 1)
    obs, exp, skipped = np.zeros(shape, np.int64), np.zeros(shape, np.int64), 0
    for name, (s, e, q) in frags.items():
        if name not in world["contigs"]:
            continue
        ct = world["contigs"][name]
        s, e, q = np.asarray(s, np.int64), np.asarray(e, np.int64), np.asarray(q, np.int64)
        keep = (q >= mapq_min) & (e - s >= len_lo) & (e - s <= len_hi)
        gc = ct.gc(s[keep], e[keep])
        np.add.at(obs, ((e - s)[keep][gc >= 0] - len_lo, gc[gc >= 0]), 1)
        skipped += int((gc < 0).sum())
        exp += ct.expected(0, ct.n, len_lo, len_hi, stride)
    return obs, exp, skipped


def same_result(a, b):
    return (np.array_equal(a.observed, b.observed) and np.array_equal(a.expected, b.expected) and a.n_skipped == b.n_skipped
            and a.skipped_contigs == b.skipped_contigs and a.n_fragments == b.n_fragments
            and np.array_equal(a.bias, b.bias, equal_nan=True))


def test_frag_gc_bias_end_to_end(engine, world, tmp_path):
    from finaletoolkit_amd import utils
    rng = np.random.default_rng(77)
    contigs = [("cA", LAYOUT["cA"][0]), ("cX", 9_000), ("cC", LAYOUT["cC"][0])]
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
    results = {}
    for tag, path in (("bam", bam), ("frag", frag)):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            results[tag] = utils.frag_gc_bias(path, ref, stride=3)
        ours = [w for w in caught if issubclass(w.category, UserWarning) and "not in the reference" in str(w.message)]
        assert len(ours) == 1 and "cX" in str(ours[0].message)
    assert same_result(results["bam"], results["frag"])
    res = results["bam"]
    assert (res.min_length, res.max_length, res.skipped_contigs) == (100, 220, ("cX",))
    assert res.observed.dtype == np.int64 and res.expected.dtype == np.int64 and res.bias.dtype == np.float64
    want_bam = {c: (v[0], v[1], v[2]) for c, v in bam_expected(bam)[0].items()}
    want_frag = {c: (v[0], v[1], v[2]) for c, v in read_frag_gz(frag).items()}
    for want in (want_bam, want_frag):
        obs, exp, skipped = restated_result(world, want, 100, 220, 3)
        assert np.array_equal(res.observed, obs) and np.array_equal(res.expected, exp) and res.n_skipped == skipped
        assert res.n_fragments == int(obs.sum()) > 500 and skipped > 0
        assert np.array_equal(res.bias, utils.gc_bias_ratio(obs, exp), equal_nan=True)
    # expected= from the first run reproduces the result; one contig alone; a contig the input lacks
    again = utils.frag_gc_bias(frag, ref, stride=3, expected=res.expected, contig=None)
    assert same_result(again, res)
    one = utils.frag_gc_bias(frag, ref, contig="cC", min_length=150, max_length=180, quality_threshold=0, stride=64)
    obs, exp, skipped = restated_result(world, {"cC": want_frag["cC"]}, 150, 180, 64, 0)
    assert np.array_equal(one.observed, obs) and np.array_equal(one.expected, exp) and one.n_skipped == skipped
    assert one.skipped_contigs == ()
    with pytest.raises(ValueError, match="contig not present"):
        utils.frag_gc_bias(frag, ref, contig="13")
    # the command line, in a child process, and both suffixes
    for suffix in (".tsv", ".tsv.gz"):
        out = str(tmp_path / ("cli" + suffix))
        r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.gcbias", frag, ref, out, "--stride", "3", "-q", "30"],
                           cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert "cX" in r.stderr  # the warning
        text = gzip.open(out, "rt").read() if suffix.endswith(".gz") else open(out).read()
        lines = text.splitlines()
        assert lines[0] == "length\tgc\tobserved\texpected\tbias"
        obs, exp = np.zeros_like(res.observed), np.zeros_like(res.expected)
        for ln in lines[1:]:
            length, g, o, e, b = ln.split("\t")
            cell = (int(length) - 100, int(g))
            obs[cell], exp[cell] = int(o), int(e)
            assert (b == "nan") == bool(np.isnan(res.bias[cell])) and (b == "nan" or float(b) == res.bias[cell])
        assert np.array_equal(obs, res.observed) and np.array_equal(exp, res.expected)
        assert len(lines) - 1 == int(((res.observed > 0) | (res.expected > 0)).sum())
