"""GPU: the motif x length table (``csrc/ftk_motiflen.hip``) - ``Engine.motif_length_table`` against the numpy restatement
of ``tests/motif_length_helpers.py``, exactly equal everywhere (counts are integers: no tolerance anywhere): on a 2bit image
and two FASTA images of one genome, for k = 1 .. 4 and the end, breakpoint and shifted anchors, with fewer rows than one LDS
band, one band + 1 and 1024 rows of 1 and of 40 lengths, at the contigs' and the N runs' edges, at every word alignment,
above the 16-bit range and at the top coordinates; rebinning; the cross-check against ``ftk_motif_counts``; the
reverse-complement symmetry; a poisoned scratch block; device outputs and an empty contig; the C ABI's argument errors;
``frag_motif_lengths`` and its command line on a synthetic BAM and its fragment file."""
import gzip
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests import end_context_helpers as H
from tests import motif_length_helpers as M
from tests import motif_length_poison_calls as MP
from tests.helpers import bam_expected, read_frag_gz, write_2bit, write_fasta, write_synthetic_bam

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGES = ("2bit", "fa60", "fa50")


def shifts_of(k):
    """The end motifs, the breakpoint motifs (``-(k // 2)``; for odd k also Python's ``-k // 2``, one base further) and one
    base inside the fragment."""
    return sorted({0, -(k // 2), -k // 2, 1})


def row_plans(band):
    """(len_lo, len_hi, len_bin): fewer rows than one band; exactly one band + 1; 1024 rows of one length and, on the same
    data, of 40 lengths, which reach the 40 000-base fragment."""
    return ((100, 100 + min(band, 20) - 2, 1), (1, 1 + band, 1), (1, 1024, 1), (1, 40_960, 40))


@pytest.fixture(scope="module")
def world(engine, tmp_path_factory):
    from finaletoolkit_amd.reference import ReferenceGenome
    d = tmp_path_factory.mktemp("motiflen")
    rng = np.random.default_rng(20261021)
    seqs = H.make_genome(rng)
    rc = {name: H.reverse_complement(s) for name, s in seqs.items()}
    paths = {"2bit": str(d / "g.2bit"), "fa60": str(d / "g60.fa"), "fa50": str(d / "g50.fa"), "rc": str(d / "rc.2bit")}
    write_2bit(paths["2bit"], seqs)
    write_fasta(paths["fa60"], seqs, width=60)
    write_fasta(paths["fa50"], seqs, width=50)
    write_2bit(paths["rc"], rc)
    bands = {k: engine.motif_length_lds_rows(k) for k in M.KS}
    w = dict(dir=d, seqs=seqs, rc=rc, paths=paths, refs={k: ReferenceGenome(p) for k, p in paths.items()}, bands=bands,
             bases={name: H.Bases(s) for name, s in seqs.items()}, cols={}, want={})
    sets = M.edge_sets_for(bands.values())
    for name, seq in seqs.items():
        cols = H.fragments_of(name, len(seq), rng, edge_sets=sets)
        engine.load_contig("ml:" + name, *cols, np.zeros(len(cols[0]), np.uint8))
        w["cols"][name] = cols
    yield w
    for name in seqs:
        engine.release("ml:" + name)
    for r in w["refs"].values():
        r.close()


def rid_of(engine, world, image, name):
    return world["refs"][image].device_image(engine, name, with_layout=True)


def wanted(world, name, k, shift, plan, mapq_min=30):
    """The restatement, computed once per argument set and left unchanged."""
    key = (name, k, shift, tuple(plan), mapq_min)
    if key not in world["want"]:
        table, kept = M.restated_motif_lengths(world["bases"][name], *world["cols"][name], k, shift, *plan, mapq_min)
        table.setflags(write=False), kept.setflags(write=False)
        world["want"][key] = (table, kept)
    return world["want"][key]


def assert_same(got, want, what):
    table, kept = got
    assert table.dtype == np.int64 and table.shape == want[0].shape and kept.dtype == np.int64 and kept.shape == want[1].shape, what
    assert np.array_equal(kept, want[1]), (what, np.flatnonzero(kept != want[1])[:5])
    bad = np.argwhere(table != want[0])
    assert len(bad) == 0, (what, len(bad), bad[:5], table[tuple(bad[0])], want[0][tuple(bad[0])])
    assert M.row_sums_hold(table, kept), what


# ---- 1. the hand-placed fragments are there ----------------------------------------------------------------------------
def test_hand_cases_are_present(world):
    bands = world["bands"]
    assert all(1 <= bands[k] < bands[k] + 1 <= M.MAX_ROWS for k in M.KS) and len(set(bands.values())) >= 3
    for name, seq in world["seqs"].items():
        n = len(seq)
        s, e, q = (v.astype(np.int64) for v in world["cols"][name])
        ln, ok = e - s, q >= 30
        for v in M.band_starts(bands.values()) + [1 + bands[k] for k in M.KS]:  # both sides of every band edge, for every k
            assert (ln[ok] == v).any() and (ln[ok] == v - 1).any(), (name, v)
        assert (ln[ok] == 1).any() and (ln[ok] == 1024).any() and (ln[ok] == 1025).any() and (ln[ok] == 40_000).any()
        assert (s[ok] == 0).any() and (e[ok] == n).any() and (e[ok] == n + 1).any() and (s[ok] >= n).any() and (s[ok] == n).any()
        assert (ok & (ln == 1) & (s == 0)).any() and (ok & (ln == 1) & (e == n)).any()  # L = 1 < k, at either end of the contig
        assert set(s[ok] % 16) == set(range(16)) and set((e[ok] - 1) % 16) == set(range(16))  # all 16 alignments in a 2bit word
        assert {0, 29, 30, 31, 255} <= set(q.tolist())
        for a0, a1 in H.LAYOUT[name][1]:  # anchors within 4 bases of each N-run edge, and inside the runs
            for edge in (a0, a1):
                for d in (-8, -1, 0, 1, 8):
                    assert edge + d < 0 or (s[ok] == edge + d).any() and (e[ok] - 1 == edge + d).any(), (name, edge, d)
            assert ((s > a0) & (s < a1 - 1)).any() or a1 - a0 < 3
        if name in H.DUP:
            assert ((s == H.DUP[name][0]) & (e == H.DUP[name][1])).sum() >= H.N_DUP > 65_535


# ---- 2. the table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", M.KS)
@pytest.mark.parametrize("image", IMAGES)
def test_table_equals_the_restatement(engine, world, image, k):
    band = world["bands"][k]
    for name in world["seqs"]:
        rid = rid_of(engine, world, image, name)
        for shift in shifts_of(k):
            for plan in row_plans(band):
                want = wanted(world, name, k, shift, plan)
                got = engine.motif_length_table("ml:" + name, rid, k, shift, *plan, 30)
                assert_same(got, want, (image, k, shift, plan, name))
                table, kept = got
                # the cases are there and do what they are for: both kinds, undefined readings, both sides of a band edge
                assert kept.sum() > 0
                if plan[0] == 1:
                    assert table[0, :, :-1].any() and table[1, :, :-1].any() and kept.sum() > 20
                    assert table[0, :, -1].any() and table[1, :, -1].any(), name
                    assert plan[2] != 1 or (kept[band - 1] > 0 and kept[band] > 0 and kept[0] > 0 and kept[-1] > 0)
                if plan[2] == 40:
                    assert kept[(40_000 - 1) // 40] > 0 and len(kept) == M.MAX_ROWS
                if name in H.DUP and plan[0] <= H.DUP[name][1] - H.DUP[name][0] <= plan[1]:
                    assert table.max() > 65_535  # N_DUP copies of one fragment: a cell above the 16-bit range


@pytest.mark.parametrize("mapq_min", [0, 29, 30, 31, 255, 256])
def test_mapq_threshold(engine, world, mapq_min):
    s, e, q = world["cols"]["eB"]
    plan = (1, 1000, 1)
    got = engine.motif_length_table("ml:eB", rid_of(engine, world, "fa60", "eB"), 3, 0, *plan, mapq_min)
    assert_same(got, wanted(world, "eB", 3, 0, plan, mapq_min), mapq_min)
    ln = e.astype(np.int64) - s
    assert got[1].sum() == int(((q >= mapq_min) & (ln >= 1) & (ln <= 1000)).sum())
    assert (mapq_min == 256) == (got[1].sum() == 0)


# ---- 3. rebinning ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, b", [(4, 8), (2, 25), (1, 3)])
def test_rows_of_b_lengths_are_b_rows_summed(engine, world, k, b):
    lo, n_wide = 10, 1000 // b
    hi = lo + n_wide * b - 1  # whole rows of b lengths, at most 1000 rows of one
    for name in ("eA", "eS"):
        rid = rid_of(engine, world, "2bit", name)
        fine, fine_kept = engine.motif_length_table("ml:" + name, rid, k, 0, lo, hi, 1, 30)
        wide, wide_kept = engine.motif_length_table("ml:" + name, rid, k, 0, lo, hi, b, 30)
        assert fine.shape == (2, n_wide * b, 4 ** k + 1) and wide.shape == (2, n_wide, 4 ** k + 1) and wide_kept.sum() > 20
        assert np.array_equal(fine.reshape(2, n_wide, b, -1).sum(axis=2), wide)
        assert np.array_equal(fine_kept.reshape(n_wide, b).sum(axis=1), wide_kept)


# ---- 4. the cross-check against the motif kernel, 5. symmetry ----------------------------------------------------------
@pytest.mark.parametrize("image", IMAGES)
def test_pooled_rows_equal_the_motif_kernel(engine, world, image):
    """ftk_motif_counts adds, per fragment, the forward k-mer ref[start + fwd_offset, +k) and the reverse complement of
    ref[stop + rev_offset, +k): with fwd_offset = shift and rev_offset = -k - shift, the two readings of this table."""
    n = len(world["seqs"]["eM"])
    rng = np.random.default_rng(31)
    s = np.sort(rng.integers(8, n - 8 - 300, 3000))
    e = s + rng.integers(1, 300, 3000)
    q = rng.choice([0, 29, 30, 60], 3000)
    assert s.min() >= 8 and e.max() <= n - 8 and "N" not in world["seqs"]["eM"]
    engine.load_contig("ml:motif", s, e, q, np.ones(3000, np.uint8))
    try:
        rid = rid_of(engine, world, image, "eM")
        for k in M.KS:
            for shift in (0, -(k // 2)):
                table, kept = engine.motif_length_table("ml:motif", rid, k, shift, 1, 1000, 1, 30)
                want = engine.motif_counts("ml:motif", rid, [0], [n], k, shift, -k - shift, True, False, 0, False, 30)[0]
                assert np.array_equal(table[0].sum(axis=0)[:4 ** k] + table[1].sum(axis=0)[:4 ** k], want[0].astype(np.int64)), (k, shift)
                assert kept.sum() == int((q >= 30).sum()) and not table[..., -1].any() and want.sum() == 2 * kept.sum()
    finally:
        engine.release("ml:motif")


@pytest.mark.parametrize("k", M.KS)
def test_reverse_complement_swaps_the_kinds(engine, world, k):
    for name in ("eA", "eB", "eS"):
        n = len(world["seqs"][name])
        s, e, q = (v.astype(np.int64) for v in world["cols"][name])
        inside = e <= n  # (n - e would be negative)
        rs, re_, rq = n - e[inside], n - s[inside], q[inside]
        o = np.argsort(rs, kind="stable")
        engine.load_contig("ml:fwd", s[inside], e[inside], q[inside], np.zeros(int(inside.sum()), np.uint8))
        engine.load_contig("ml:rev", rs[o], re_[o], rq[o], np.zeros(len(o), np.uint8))
        try:
            for shift in shifts_of(k):
                fwd, kept = engine.motif_length_table("ml:fwd", rid_of(engine, world, "2bit", name), k, shift, 1, 1024, 1, 30)
                rev, rkept = engine.motif_length_table("ml:rev", rid_of(engine, world, "rc", name), k, shift, 1, 1024, 1, 30)
                assert np.array_equal(kept, rkept) and kept.sum() > 20 and (fwd[..., -1].any() or name == "eS")  # (eS has no N)
                assert np.array_equal(rev[::-1], fwd), (name, shift, np.argwhere(rev[::-1] != fwd)[:5])
                assert not np.array_equal(fwd[0], fwd[1])  # (the swap is not trivially true)
        finally:
            engine.release("ml:fwd"), engine.release("ml:rev")


# ---- 6. a poisoned scratch block ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", M.KS)
def test_same_table_on_a_poisoned_scratch(engine, world, k):
    band = world["bands"][k]
    for image, name in (("2bit", "eA"), ("fa50", "eC")):
        rid = rid_of(engine, world, image, name)
        for plan in row_plans(band)[1:]:
            first, runs = MP.same_after_fills(engine, lambda: engine.motif_length_table("ml:" + name, rid, k, 0, *plan, 30))
            assert [byte for byte, _ in runs] == [0xA5, 0x00] and all(same for _, same in runs), (image, name, plan, runs)
            assert_same(first, wanted(world, name, k, 0, plan), (image, name, plan))


def test_poison_table_holds_the_new_call():
    """The entry ``tests/motif_length_poison_calls.py`` adds to the table ``tests/test_gpu_scratch_poison.py`` runs."""
    from finaletoolkit_amd import _lib as L
    from tests import scratch_poison_calls as P
    for name, entry in MP.ENTRIES.items():
        assert P.CALLS[name] is entry and set(name.split("+")) <= set(L.EXPORTS)
    assert {sym for name in MP.ENTRIES for sym in name.split("+")} == {"ftk_motif_length_table", "ftk_motif_length_lds_rows"}


# ---- 7. the caller's arrays, an empty contig ---------------------------------------------------------------------------
def test_outputs_into_the_callers_arrays(engine, world):
    import torch
    from finaletoolkit_amd import _lib as L
    rid = rid_of(engine, world, "2bit", "eA")
    cid = engine.contig_id("ml:eA")
    plan = (1, 1024, 1)
    want, want_kept = wanted(world, "eA", 4, 0, plan)
    cells, n_rows = want.size, len(want_kept)
    # device tensors with guard elements on either side
    buf = torch.full((cells + 2,), -7, dtype=torch.int64, device="cuda:0")
    kbuf = torch.full((n_rows + 2,), -7, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert engine.lib.ftk_motif_length_table(engine.ctx, cid, rid, 4, 0, *plan, 30, L.ptr(buf[1:1 + cells]), L.ptr(kbuf[1:1 + n_rows])) == L.FTK_OK
    engine.sync()
    host, khost = buf.cpu().numpy(), kbuf.cpu().numpy()
    assert np.array_equal(host[1:-1].reshape(want.shape), want) and host[0] == -7 and host[-1] == -7
    assert np.array_equal(khost[1:-1], want_kept) and khost[0] == -7 and khost[-1] == -7
    # host tables pre-filled with 7 are fully overwritten
    table, kept = np.full(want.shape, 7, np.int64), np.full(n_rows, 7, np.int64)
    assert engine.lib.ftk_motif_length_table(engine.ctx, cid, rid, 4, 0, *plan, 30, L.ptr(table), L.ptr(kept)) == L.FTK_OK
    assert np.array_equal(table, want) and np.array_equal(kept, want_kept) and (table == 0).sum() > 1000 and (kept == 0).any()
    # an empty contig: zeros
    engine.load_contig("ml:empty", np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    try:
        table[:], kept[:] = 7, 7
        ecid = engine.contig_id("ml:empty")
        assert engine.lib.ftk_motif_length_table(engine.ctx, ecid, rid, 4, 0, *plan, 30, L.ptr(table), L.ptr(kept)) == L.FTK_OK
        assert not table.any() and not kept.any()
        t, kk = engine.motif_length_table("ml:empty", rid, 2, -1, 1, 40_960, 40, 0)
        assert t.shape == (2, 1024, 17) and not t.any() and not kk.any()
    finally:
        engine.release("ml:empty")


# ---- 8. the C ABI's argument errors ------------------------------------------------------------------------------------
def test_argument_errors(engine, world):
    from finaletoolkit_amd import _lib as L
    lib, ctx = engine.lib, engine.ctx
    rid = rid_of(engine, world, "2bit", "eA")
    cid = engine.contig_id("ml:eA")
    table = np.full(2 * 1024 * 257, 7, np.int64)
    kept = np.full(1024, 7, np.int64)
    INV, NOC = L.FTK_ERR_INVALID, L.FTK_ERR_NO_CONTIG

    def call(cid_=cid, rid_=rid, k=4, shift=0, lo=1, hi=1000, b=1, out=table, n_kept=kept, ctx_=ctx):
        return lib.ftk_motif_length_table(ctx_, cid_, rid_, k, shift, lo, hi, b, 30, L.ptr(out), L.ptr(n_kept))

    def failed(rc, code):
        assert rc == code, (rc, code)
        assert lib.ftk_last_error(ctx)

    assert call() == L.FTK_OK  # the arguments the failing calls vary
    assert call(shift=4) == L.FTK_OK and call(shift=-4) == L.FTK_OK and call(lo=1 << 30, hi=1 << 30) == L.FTK_OK  # the bounds themselves
    assert call(lo=1, hi=1 << 30, b=1 << 20) == L.FTK_OK and call(lo=1, hi=1024) == L.FTK_OK and call(k=1) == L.FTK_OK
    table[:], kept[:] = 7, 7
    assert call(ctx_=None) == INV
    failed(call(out=None), INV)
    failed(call(n_kept=None), INV)
    failed(call(cid_=987_654), NOC)
    failed(call(rid_=987_654), NOC)
    for k in (0, -1, 5, 1 << 20):
        failed(call(k=k), INV)
    for shift in (5, -5, 1 << 30, -(1 << 31)):
        failed(call(shift=shift), INV)
    for lo, hi in ((0, 100), (-5, 100), (101, 100), (1, (1 << 30) + 1), ((1 << 30) + 1, (1 << 30) + 1)):
        failed(call(lo=lo, hi=hi), INV)
    for b in (0, -1, -(1 << 31)):
        failed(call(b=b), INV)
    failed(call(lo=1, hi=1025), INV)  # 1025 rows
    failed(call(lo=1, hi=1 << 30, b=(1 << 20) - 1), INV)
    failed(call(lo=100, hi=100 + 1024 * 7, b=7), INV)
    with pytest.raises(L.FtkError):
        engine.motif_length_table("ml:eA", rid, 5, 0, 1, 1000)
    with pytest.raises(L.FtkError):
        engine.motif_length_table("ml:eA", rid, 4, 0, 1, 1025)
    with pytest.raises(L.FtkError):
        engine.motif_length_table("ml:eA", rid, 4, 0, 5, 4)
    # an image without its layout
    bare = engine.ref_upload(("ml-test", "bare"), np.zeros(64, np.uint8), 1)
    failed(call(rid_=bare), INV)
    assert b"layout" in lib.ftk_last_error(ctx)
    # nothing was written by any of them
    assert np.all(table == 7) and np.all(kept == 7)


# ---- 9. the top coordinates --------------------------------------------------------------------------------------------
def test_top_coordinates(engine):
    from finaletoolkit_amd import _lib as L
    n = (1 << 30) - 1
    rng = np.random.default_rng(8)
    tail = rng.choice(np.frombuffer(b"ACGT", np.uint8), 1024).tobytes().decode()
    n_block = (n - 600, n - 550)
    image = np.zeros((n + 3) // 4, np.uint8)  # T everywhere ...
    code = np.array([2, 1, 3, 0], np.uint8)[H.Bases(tail)(np.arange(1024))]  # ... but the last kilobase (T 0, C 1, A 2, G 3)
    pos = np.arange(n - 1024, n)
    np.bitwise_or.at(image, pos >> 2, (code << (6 - 2 * (pos & 3))).astype(np.uint8))
    bases = H.SparseBases(n, tail, n_block)
    s = np.sort(np.concatenate([[0, 0, 1, 5, 1 << 29], n - rng.integers(1, 1024, 600)]))
    e = np.minimum(s + rng.integers(1, 400, len(s)), n)
    e[-40:] = n  # the last base is an end
    e[-48:-40] = n - np.arange(1, 9)  # ends within k of chrom_len
    e[:3] = (n, n - 1, n)  # L = 2^30 - 1, 2^30 - 2 and 2^30 - 2: near 2^30
    e = np.maximum(e, s + 1)
    q = np.full(len(s), 60)
    ln = e - s
    assert (e == n).sum() >= 40 and ((s < n_block[1] + 4) & (s > n_block[0] - 4)).any() and (ln >= 1).all() and ln.max() == n
    assert all((e == n - d).any() for d in range(1, 5))
    engine.load_contig("ml:top", s, e, q, np.zeros(len(s), np.uint8))
    rid = engine.ref_upload(("ml-test", "top"), image, 1)
    try:
        engine.ref_set_layout(rid, n, 0, 0, [n_block[0]], [n_block[1]])
        for k, shift in ((4, 0), (4, -2), (3, 1), (1, 0)):
            # rows of 2^20 lengths up to 2^30: L near 2^30 lands in the last of the 1024 rows
            got = engine.motif_length_table("ml:top", rid, k, shift, 1, 1 << 30, 1 << 20, 30)
            want = M.restated_motif_lengths(bases, s, e, q, k, shift, 1, 1 << 30, 1 << 20, 30)
            assert_same(got, want, (k, shift, "wide rows"))
            assert got[1][-1] == 3 and got[1][0] == len(s) - 3 and len(got[1]) == M.MAX_ROWS
            got = engine.motif_length_table("ml:top", rid, k, shift, 1, 1024, 1, 30)
            assert_same(got, M.restated_motif_lengths(bases, s, e, q, k, shift, 1, 1024, 1, 30), (k, shift, "rows of one"))
            assert got[0][..., -1].any() and got[0][..., :-1].any()
        # one base more and the coordinate bound is reached: the call refuses, and writes nothing
        engine.ref_set_layout(rid, 1 << 30, 0, 0)
        table, kept = np.full(2 * 10 * 257, 7, np.int64), np.full(10, 7, np.int64)
        cid = engine.contig_id("ml:top")
        assert engine.lib.ftk_motif_length_table(engine.ctx, cid, rid, 4, 0, 1, 10, 1, 30, L.ptr(table), L.ptr(kept)) == L.FTK_ERR_INVALID
        assert b"2^30" in engine.lib.ftk_last_error(engine.ctx)
        assert (table == 7).all() and (kept == 7).all()
    finally:
        engine.release("ml:top")


# ---- 10. the product path ----------------------------------------------------------------------------------------------
def restated_result(world, frags, k, shift, lo, hi, b, mapq_min=30):
    table = np.zeros((2, M.n_rows_of(lo, hi, b), 4 ** k + 1), np.int64)
    kept = np.zeros(table.shape[1], np.int64)
    for name, (s, e, q) in frags.items():
        if name not in world["bases"]:
            continue
        t, kk = M.restated_motif_lengths(world["bases"][name], s, e, q, k, shift, lo, hi, b, mapq_min)
        table, kept = table + t, kept + kk
    return table, kept


def same_result(a, b):
    return (np.array_equal(a.table, b.table) and np.array_equal(a.n_kept, b.n_kept)
            and (a.k, a.kind, a.min_length, a.length_bin, a.skipped_contigs) == (b.k, b.kind, b.min_length, b.length_bin, b.skipped_contigs))


def test_frag_motif_lengths_end_to_end(engine, world, tmp_path):
    from finaletoolkit_amd import utils, writers
    rng = np.random.default_rng(77)
    contigs = [("eA", H.LAYOUT["eA"][0]), ("eX", 9_000), ("eC", H.LAYOUT["eC"][0])]
    frags = {}
    for name, n in contigs:
        a = np.sort(rng.integers(0, n - 400, 1500))
        ln = rng.integers(90, 400, 1500)
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
            results[tag] = utils.frag_motif_lengths(path, ref)
        ours = [w for w in caught if issubclass(w.category, UserWarning) and "not in the reference" in str(w.message)]
        assert len(ours) == 1 and "eX" in str(ours[0].message)
    assert same_result(results["bam"], results["frag"])
    res = results["bam"]
    assert isinstance(res, utils.MotifLengths)
    assert (res.k, res.kind, res.min_length, res.length_bin, res.skipped_contigs) == (4, "end", 1, 1, ("eX",))
    assert res.table.dtype == np.int64 and res.table.shape == (2, 1000, 257) and res.n_kept.shape == (1000,)
    want_bam = {c: (v[0], v[1], v[2]) for c, v in bam_expected(bam)[0].items()}
    want_frag = {c: (v[0], v[1], v[2]) for c, v in read_frag_gz(frag).items()}
    for want in (want_bam, want_frag):
        table, kept = restated_result(world, want, 4, 0, 1, 1000, 1)
        assert np.array_equal(res.table, table) and np.array_equal(res.n_kept, kept)
        assert kept.sum() > 1000 and table[..., -1].any()
    assert M.row_sums_hold(res.table, res.n_kept)
    assert np.array_equal(res.pooled(1, 1000), res.table.sum(axis=1))  # everything: what end_motifs gives for the size selection
    assert res.frequency().shape == (2, 1000, 256) and res.mds().shape == (3, 1000) and np.nanmax(res.mds()) <= 1.0
    # one contig, breakpoint motifs, rows of 25 lengths, another reference format
    one = utils.frag_motif_lengths(frag, world["paths"]["fa50"], contig="eC", k=2, kind="breakpoint", min_length=100, max_length=349,
                                   length_bin=25, quality_threshold=0)
    table, kept = restated_result(world, {"eC": want_frag["eC"]}, 2, -1, 100, 349, 25, 0)
    assert np.array_equal(one.table, table) and np.array_equal(one.n_kept, kept) and one.table.shape == (2, 10, 17)
    assert (one.skipped_contigs, one.kind, one.k, one.min_length, one.length_bin) == ((), "breakpoint", 2, 100, 25)
    assert np.array_equal(one.pooled(100, 349), one.table.sum(axis=1)) and one.lengths().tolist() == list(range(100, 350, 25))
    with pytest.raises(ValueError, match="contig not present"):
        utils.frag_motif_lengths(frag, ref, contig="13")
    # the command line, in a child process, and both suffixes; both TSVs parse back to the table
    names = res.motifs() + ["N"]
    for suffix in (".tsv", ".tsv.gz"):
        out, summ = str(tmp_path / ("cli" + suffix)), str(tmp_path / ("cli_summary" + suffix))
        r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.motiflengths", frag, ref, out, "--summary", summ, "-q", "30", "-k", "4",
                            "--kind", "end", "--min-length", "1", "--max-length", "1000", "--length-bin", "1"],
                           cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert "eX" in r.stderr  # the warning
        text, stext = (gzip.open(p, "rt").read() if suffix.endswith(".gz") else open(p).read() for p in (out, summ))
        assert text == writers.motif_length_text(res) and stext == writers.motif_length_summary_text(res)
        lines, slines = text.splitlines(), stext.splitlines()
        assert lines[0] + "\n" == writers.MOTIF_LENGTH_HEADER and slines[0] + "\n" == writers.MOTIF_LENGTH_SUMMARY_HEADER
        count = np.zeros_like(res.table)
        for ln in lines[1:]:
            lo, hi, end, motif, c, f = ln.split("\t")
            assert lo == hi
            count[("UD".index(end), int(lo) - 1, names.index(motif))] = int(c)
        assert np.array_equal(count, res.table)
        kept, undefined = np.zeros_like(res.n_kept), np.zeros((2, 1000), np.int64)
        for ln in slines[1:]:
            lo, hi, nf, uu, ud, mu, md, mp = ln.split("\t")
            kept[int(lo) - 1], undefined[0, int(lo) - 1], undefined[1, int(lo) - 1] = int(nf), int(uu), int(ud)
            assert mp == repr(float(res.mds()[2, int(lo) - 1]))
        assert np.array_equal(kept, res.n_kept) and np.array_equal(undefined, res.table[..., -1])
    # files written by the function itself are the same bytes as the command line's
    out2, summ2 = str(tmp_path / "direct.tsv"), str(tmp_path / "direct_summary.tsv")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        utils.frag_motif_lengths(frag, ref, out2, summ2)
    assert open(out2, "rb").read() == open(str(tmp_path / "cli.tsv"), "rb").read()
    assert open(summ2, "rb").read() == open(str(tmp_path / "cli_summary.tsv"), "rb").read()
