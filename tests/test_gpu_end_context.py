"""GPU: the end-context tables (``csrc/ftk_endcontext.hip``) - ``Engine.end_context`` and ``Engine.ref_context`` against the
numpy restatement of ``tests/end_context_helpers.py``, exactly equal everywhere: on a 2bit image and two FASTA images of
one genome in both anchor modes, at every width that takes another path through a wave step, with one, three and eight
length classes and on both sides of the classes one workgroup keeps in LDS, at the contigs' and the N runs' edges, at
every word alignment, above the 16-bit range and at the top coordinates; the reverse-complement symmetry; the
cross-check against ``ftk_motif_counts``; the C ABI's argument errors; ``frag_end_context`` and its command line on a
synthetic BAM and its fragment file."""
import ctypes as C
import gzip
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests import end_context_helpers as H
from tests.helpers import bam_expected, read_frag_gz, write_2bit, write_fasta, write_synthetic_bam

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGES = ("2bit", "fa60", "fa50")
ANCHORS = ("ends", "centre")
CLASS_SETS = {"one": H.ONE_CLASS, "default": H.DEFAULT_EDGES, "eight": H.EIGHT_CLASSES}
LDS_EDGES = (1, 100, 150, 167, 200, 221, 400, 1_001, 39_000)  # the first k + 1 of them bound k populated classes
N, NOT_N = slice(20, 25), slice(0, 20)  # cells whose first base is N / is not


@pytest.fixture(scope="module")
def world(engine, tmp_path_factory):
    from finaletoolkit_amd.reference import ReferenceGenome
    d = tmp_path_factory.mktemp("endcontext")
    rng = np.random.default_rng(20261020)
    seqs = H.make_genome(rng)
    rc = {name: H.reverse_complement(s) for name, s in seqs.items()}
    paths = {"2bit": str(d / "g.2bit"), "fa60": str(d / "g60.fa"), "fa50": str(d / "g50.fa"), "rc": str(d / "rc.2bit")}
    write_2bit(paths["2bit"], seqs)
    write_fasta(paths["fa60"], seqs, width=60)
    write_fasta(paths["fa50"], seqs, width=50)
    write_2bit(paths["rc"], rc)
    w = dict(dir=d, seqs=seqs, rc=rc, paths=paths, refs={k: ReferenceGenome(p) for k, p in paths.items()},
             bases={name: H.Bases(s) for name, s in seqs.items()}, cols={}, want={})
    for name, seq in seqs.items():
        cols = H.fragments_of(name, len(seq), rng)
        engine.load_contig("ec:" + name, *cols, np.zeros(len(cols[0]), np.uint8))
        w["cols"][name] = cols
    yield w
    for name in seqs:
        engine.release("ec:" + name)
    for r in w["refs"].values():
        r.close()


def rid_of(engine, world, image, name):
    return world["refs"][image].device_image(engine, name, with_layout=True)


def wanted(world, name, half_width, edges, anchor, mapq_min=30):
    """The restatement, computed once per argument set and left unchanged."""
    key = (name, half_width, tuple(edges), anchor, mapq_min)
    if key not in world["want"]:
        table, kept = H.restated_end_context(world["bases"][name], *world["cols"][name], half_width, edges, mapq_min, anchor)
        table.setflags(write=False), kept.setflags(write=False)
        world["want"][key] = (table, kept)
    return world["want"][key]


def assert_same(got, want, what):
    table, kept = got
    assert table.dtype == np.int64 and table.shape == want[0].shape and kept.dtype == np.int64, what
    assert np.array_equal(kept, want[1]), (what, kept, want[1])
    bad = np.argwhere(table != want[0])
    assert len(bad) == 0, (what, len(bad), bad[:5], table[tuple(bad[0])], want[0][tuple(bad[0])])
    assert np.array_equal(table.sum(axis=-1), np.broadcast_to(kept[:, None, None], table.shape[:3])), what


# ---- 0. the hand-placed fragments are there ----------------------------------------------------------------------------
def test_hand_cases_are_present(world):
    for name, seq in world["seqs"].items():
        n = len(seq)
        s, e, q = (v.astype(np.int64) for v in world["cols"][name])
        ln = e - s
        assert (s == 0).any() and (e == n).any() and (e == n + 1).any() and (e > n + 4000).any() and (s >= n).any() and (s == n).any()
        assert (ln == 1).any() and ((ln > 1) & (ln < 7)).any() and (ln == 40_000).any()
        for edges in (H.DEFAULT_EDGES, H.EIGHT_CLASSES):
            for v in edges:
                skip = {H.EIGHT_CLASSES[H.EMPTY_CLASS], H.EIGHT_CLASSES[H.EMPTY_CLASS + 1] - 1}
                assert (v in skip or (ln == v).any()) and (v - 1 in skip or v == 1 or (ln == v - 1).any()), (name, v)
        assert not ((ln >= H.EIGHT_CLASSES[H.EMPTY_CLASS]) & (ln < H.EIGHT_CLASSES[H.EMPTY_CLASS + 1])).any()
        ok = q >= 30
        assert set(s[ok] % 16) == set(range(16)) and set((e[ok] - 1) % 16) == set(range(16))
        assert {0, 29, 30, 31, 255} <= set(q.tolist())
        for a0, a1 in H.LAYOUT[name][1]:  # anchors on both sides of each N-run edge, within every width, and inside the run
            for edge in (a0, a1):
                for d in (-129, -33, -1, 0, 1, 33, 129):
                    assert edge + d < 0 or (s[ok] == edge + d).any() and (e[ok] - 1 == edge + d).any(), (name, edge, d)
            assert ((s > a0) & (s < a1 - 1)).any() or a1 - a0 < 3
        if name in H.DUP:
            assert ((s == H.DUP[name][0]) & (e == H.DUP[name][1])).sum() >= H.N_DUP
        if n > 3000:  # a window of every width that crosses a line break at 60 and at 50 bases per line
            assert any((s[ok] // 60 != (s[ok] + 1) // 60).tolist()) and any((s[ok] // 50 != (s[ok] + 1) // 50).tolist())
            assert (ok & (ln >= 20)).sum() >= 1500


# ---- 1. the table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", list(CLASS_SETS))
@pytest.mark.parametrize("half_width", H.WIDTHS)
@pytest.mark.parametrize("anchor", ANCHORS)
@pytest.mark.parametrize("image", IMAGES)
def test_table_equals_the_restatement(engine, world, image, anchor, half_width, classes):
    edges = CLASS_SETS[classes]
    for name in world["seqs"]:
        want = wanted(world, name, half_width, edges, anchor)
        got = engine.end_context("ec:" + name, rid_of(engine, world, image, name), half_width, edges, 30, anchor)
        assert_same(got, want, (image, anchor, half_width, classes, name))
        table, kept = got
        # the cases are there and do what they are for: both kinds, N cells, every class but the empty one
        assert table[:, 0].any() and table[:, 1].any()
        if name != "eM" or anchor == "ends":  # (eM has no N: only the contig's ends give one)
            assert table[..., N].any() and table[..., 4::5].any(), name
        populated = np.delete(kept, H.EMPTY_CLASS) if classes == "eight" else kept
        assert (populated > 0).all() and (classes != "eight" or kept[H.EMPTY_CLASS] == 0), (name, kept)
        if classes == "eight":
            assert not table[H.EMPTY_CLASS].any()
        if name in H.DUP:
            assert table.max() > 65_535  # N_DUP copies of one fragment: a cell above the 16-bit range


@pytest.mark.parametrize("anchor", ANCHORS)
def test_classes_on_both_sides_of_the_lds_block(engine, world, anchor):
    fit = engine.end_context_lds_classes(128)
    assert 1 <= fit < fit + 1 <= H.MAX_CLASSES
    for n_classes in (fit, fit + 1):
        edges = LDS_EDGES[:n_classes + 1]
        for name in ("eA", "eC", "eS"):
            want = wanted(world, name, 128, edges, anchor)
            got = engine.end_context("ec:" + name, rid_of(engine, world, "2bit", name), 128, edges, 30, anchor)
            assert_same(got, want, (anchor, n_classes, name))
            assert (got[1] > 0).all() and all(got[0][c].any() for c in range(n_classes))
    assert engine.end_context_lds_classes(32) >= 3 and engine.end_context_lds_classes(1) == H.MAX_CLASSES


@pytest.mark.parametrize("half_width, classes", [(7, "default"), (32, "eight"), (128, "eight")])
def test_the_other_lds_arrangement_counts_the_same(engine, world, monkeypatch, half_width, classes):
    """FTK_CONTEXT_ARRANGE=0: lanes are offsets (the arrangement ``tools/kbench.py`` times beside the default)."""
    monkeypatch.setenv("FTK_CONTEXT_ARRANGE", "0")
    for image in ("2bit", "fa50"):
        for anchor in ANCHORS:
            for name in world["seqs"]:
                got = engine.end_context("ec:" + name, rid_of(engine, world, image, name), half_width, CLASS_SETS[classes], 30, anchor)
                assert_same(got, wanted(world, name, half_width, CLASS_SETS[classes], anchor), (image, anchor, name))


@pytest.mark.parametrize("mapq_min", [0, 29, 30, 31, 255, 256])
def test_mapq_threshold(engine, world, mapq_min):
    s, e, q = world["cols"]["eB"]
    want = wanted(world, "eB", 16, H.DEFAULT_EDGES, "ends", mapq_min)
    got = engine.end_context("ec:eB", rid_of(engine, world, "fa60", "eB"), 16, H.DEFAULT_EDGES, mapq_min, "ends")
    assert_same(got, want, mapq_min)
    ln = e.astype(np.int64) - s
    assert got[1].sum() == int(((q >= mapq_min) & (ln >= 1) & (ln < 1001)).sum())
    assert (mapq_min == 256) == (got[1].sum() == 0)


def test_the_37_base_contig_at_the_widest_window(engine, world):
    for image in IMAGES:
        for anchor in ANCHORS:
            got = engine.end_context("ec:eS", rid_of(engine, world, image, "eS"), 128, H.ONE_CLASS, 0, anchor)
            assert_same(got, wanted(world, "eS", 128, H.ONE_CLASS, anchor, 0), (image, anchor))
            assert got[0][..., N].sum() > got[0][..., NOT_N].sum() > 0  # most of every window lies outside the contig


# ---- 2. symmetry and the cross-check against the motif kernel ----------------------------------------------------------
@pytest.mark.parametrize("anchor", ANCHORS)
@pytest.mark.parametrize("half_width", [7, 32, 128])
def test_reverse_complement_swaps_the_kinds(engine, world, anchor, half_width):
    for name in ("eA", "eB", "eS"):
        n = len(world["seqs"][name])
        s, e, q = (v.astype(np.int64) for v in world["cols"][name])
        inside = e <= n  # (n - e would be negative)
        rs, re_, rq = n - e[inside], n - s[inside], q[inside]
        o = np.argsort(rs, kind="stable")
        engine.load_contig("ec:fwd", s[inside], e[inside], q[inside], np.zeros(int(inside.sum()), np.uint8))
        engine.load_contig("ec:rev", rs[o], re_[o], rq[o], np.zeros(len(o), np.uint8))
        try:
            fwd, kept = engine.end_context("ec:fwd", rid_of(engine, world, "2bit", name), half_width, H.DEFAULT_EDGES, 30, anchor)
            rev, rkept = engine.end_context("ec:rev", rid_of(engine, world, "rc", name), half_width, H.DEFAULT_EDGES, 30, anchor)
        finally:
            engine.release("ec:fwd"), engine.release("ec:rev")
        assert np.array_equal(kept, rkept) and kept.sum() > 20 and fwd[..., N].any()
        assert np.array_equal(rev[:, ::-1], fwd), (name, np.argwhere(rev[:, ::-1] != fwd)[:5])
        assert not np.array_equal(fwd[:, 0], fwd[:, 1])  # (the swap is not trivially true)


@pytest.mark.parametrize("image", IMAGES)
def test_dinucleotide_cells_equal_the_motif_kernel(engine, world, image):
    """ftk_motif_counts adds, per fragment, the forward k-mer ref[start + fwd_offset, +k) and the reverse complement of
    ref[stop + rev_offset, +k).  With fwd_offset = o the forward 2-mer is (base(s + o), base(s + o + 1)) = (r0(o),
    r0(o + 1)); with rev_offset = -o - 2 the reverse one is the reverse complement of (base(e - o - 2), base(e - o - 1)),
    = (comp(base(a1 - o)), comp(base(a1 - o - 1))) = (r1(o), r1(o + 1)) for a1 = e - 1.  k = 1: rev_offset = -o - 1."""
    W, n = 32, len(world["seqs"]["eM"])
    rng = np.random.default_rng(31)
    s = np.sort(rng.integers(W + 2, n - W - 2 - 300, 3000))
    e = s + rng.integers(1, 300, 3000)
    q = rng.choice([0, 29, 30, 60], 3000)
    assert s.min() >= W + 2 and e.max() <= n - W - 2 and "N" not in world["seqs"]["eM"]
    engine.load_contig("ec:motif", s, e, q, np.ones(3000, np.uint8))
    try:
        rid = rid_of(engine, world, image, "eM")
        table, kept = engine.end_context("ec:motif", rid, W, H.ONE_CLASS, 30, "ends")
        assert kept[0] == int((q >= 30).sum()) and not table[..., N].any() and not table[..., 4::5].any()
        res_shape = table.shape[:-1]
        pairs = np.ascontiguousarray(table.reshape(res_shape + (5, 5))[..., :4, :4]).reshape(res_shape + (16,))
        mono = table.reshape(res_shape + (5, 5)).sum(axis=-1)[..., :4]
        for o in (-W, -17, -2, -1, 0, 1, 15, W - 1):
            di, _, err = engine.motif_counts("ec:motif", rid, [0], [n], 2, o, -o - 2, True, False, 0, False, 30)
            assert np.array_equal(pairs[0, :, o + W].sum(axis=0), di[0].astype(np.int64)) and not err.any(), o
            assert di.sum() == 2 * kept[0]
            mo, _, _ = engine.motif_counts("ec:motif", rid, [0], [n], 1, o, -o - 1, True, False, 0, False, 30)
            assert np.array_equal(mono[0, :, o + W].sum(axis=0), mo[0].astype(np.int64)), o
    finally:
        engine.release("ec:motif")


# ---- 3. the background -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(H.LAYOUT))
def test_ref_context(engine, world, name):
    bases = world["bases"][name]
    n = bases.n
    m = 12_347 if n > 12_347 else 17
    assert m % 64 and m % 60 and m % 50 and m % 61 and m % 51
    ranges = [(0, n), (0, n + 500), (0, 1 << 40), (n - 1, n + 1), (5, 6), (1, n - 1), (m, m + 64), (m, m + 65), (63, 4_200)]
    whole = None
    for image in IMAGES:
        rid = rid_of(engine, world, image, name)
        for lo, hi in ranges:
            got = engine.ref_context(rid, lo, hi)
            assert got.dtype == np.int64 and got.shape == (25,)
            assert np.array_equal(got, H.restated_ref_context(bases, lo, hi)), (image, lo, hi)
        got = engine.ref_context(rid, 0, n)
        assert got.sum() == n and got[4::5].sum() >= 1  # one cell per position; the base behind the last one is N
        assert np.array_equal(engine.ref_context(rid, 0, m) + engine.ref_context(rid, m, n), got)
        assert whole is None or np.array_equal(whole, got)  # the three images agree
        whole = got
        for lo, hi in ((5, 5), (n, n + 1000), (n + 7, 1 << 40), (1 << 40, 1 << 41)):
            assert not engine.ref_context(rid, lo, hi).any()
    if H.LAYOUT[name][1]:
        assert whole[N].sum() == sum(b - a for a, b in H.LAYOUT[name][1])


def test_the_gc_kernels_and_the_context_kernels_read_the_same_bases(engine, tmp_path):
    """One sequence of 1 003 bases (a multiple of neither 4 nor 16) with an N run inside, N in the last three bases and a
    lower-case stretch, as 2bit, as FASTA with 60-base lines and as FASTA whose lines are 2 bytes wider than their bases:
    over every range, the 1 x 2 expected GC table (A + T positions, G + C positions) equals numpy's count of the sequence
    and the count read off ``ref_context`` by summing its cells over the second base."""
    from finaletoolkit_amd.reference import ReferenceGenome
    rng = np.random.default_rng(1003)
    b = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 1003)].copy()
    b[411:463] = ord("N")
    b[995:1003] = np.frombuffer(b"GATCANGN", np.uint8)  # (both kinds of base among the last six)
    b[590:700] |= 0x20  # lower case
    b[440:450] |= 0x20  # (n inside the N run)
    seq = b.tobytes().decode()
    assert len(seq) == 1003 and len(seq) % 4 and len(seq) % 16 and set(seq) >= set("ACGTNacgtn")
    paths = {"2bit": str(tmp_path / "r.2bit"), "fa60": str(tmp_path / "r60.fa"), "crlf": str(tmp_path / "rcrlf.fa")}
    write_2bit(paths["2bit"], {"r": seq})
    write_fasta(paths["fa60"], {"r": seq}, width=60)
    with open(paths["crlf"], "wb") as fh:
        fh.write(b">r\r\n" + b"".join(seq[i:i + 70].encode() + b"\r\n" for i in range(0, 1003, 70)))
    with open(paths["crlf"] + ".fai", "w") as fh:
        fh.write("r\t1003\t4\t70\t72\n")
    up = b & 0xDF
    at, gc = (up == ord("A")) | (up == ord("T")), (up == ord("G")) | (up == ord("C"))
    for image, path in paths.items():
        with ReferenceGenome(path) as ref:
            rid = ref.device_image(engine, "r", with_layout=True)
            for lo, hi in ((0, 1003), (1, 999), (997, 2000)):
                want = [int(at[lo:hi].sum()), int(gc[lo:hi].sum())]
                assert want[0] > 0 and want[1] > 0 and sum(want) < min(hi, 1003) - lo  # both kinds, and an N, in every range
                cells = engine.ref_context(rid, lo, hi).reshape(5, 5).sum(axis=1)
                assert [int(cells[0] + cells[3]), int(cells[1] + cells[2])] == want, (image, lo, hi, cells)
                assert engine.ref_gc_table(rid, lo, hi, 1, 1, 1)[0, :2].tolist() == want, (image, lo, hi)


# ---- 4. the top coordinates --------------------------------------------------------------------------------------------
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
    s = np.sort(np.concatenate([[0, 5, 1 << 29], n - rng.integers(1, 1024, 600)]))
    e = np.minimum(s + rng.integers(1, 400, len(s)), n)
    e[-40:] = n  # the last base is an end: the windows run across the contig's end
    q = np.full(len(s), 60)
    assert (e == n).sum() >= 40 and ((s < n_block[1] + 128) & (s > n_block[0] - 128)).any() and (e > s).all()
    engine.load_contig("ec:top", s, e, q, np.zeros(len(s), np.uint8))
    rid = engine.ref_upload(("ec-test", "top"), image, 1)
    try:
        engine.ref_set_layout(rid, n, 0, 0, [n_block[0]], [n_block[1]])
        for w in (32, 128):
            for anchor in ANCHORS:
                got = engine.end_context("ec:top", rid, w, H.DEFAULT_EDGES, 30, anchor)
                assert_same(got, H.restated_end_context(bases, s, e, q, w, H.DEFAULT_EDGES, 30, anchor), (w, anchor))
                assert got[0][..., N].any() and got[0][..., 4::5].any() and got[0][..., NOT_N].any()
        for lo, hi in ((n - 5000, n + 100), (n - 1, n), (n - 1024 - 77, n - 500), (0, 4097)):
            assert np.array_equal(engine.ref_context(rid, lo, hi), H.restated_ref_context(bases, lo, hi)), (lo, hi)
        # one base more and the coordinate bound is reached: both calls refuse, and write nothing
        engine.ref_set_layout(rid, 1 << 30, 0, 0)
        table, kept, out25 = np.full(3 * 2 * 64 * 25, 7, np.int64), np.full(3, 7, np.int64), np.full(25, 7, np.int64)
        edges = np.array(H.DEFAULT_EDGES, np.int32)
        cid = engine.contig_id("ec:top")
        assert engine.lib.ftk_end_context(engine.ctx, cid, rid, 32, L.ptr(edges), 3, 30, 0, L.ptr(table), L.ptr(kept)) == L.FTK_ERR_INVALID
        assert b"2^30" in engine.lib.ftk_last_error(engine.ctx)
        assert engine.lib.ftk_ref_context(engine.ctx, rid, 0, 100, L.ptr(out25)) == L.FTK_ERR_INVALID
        assert (table == 7).all() and (kept == 7).all() and (out25 == 7).all()
    finally:
        engine.release("ec:top")


# ---- 5. the caller's arrays ----------------------------------------------------------------------------------------------
def test_outputs_into_the_callers_arrays(engine, world):
    import torch
    from finaletoolkit_amd import _lib as L
    rid = rid_of(engine, world, "2bit", "eA")
    cid = engine.contig_id("ec:eA")
    want, want_kept = wanted(world, "eA", 32, H.DEFAULT_EDGES, "ends")
    cells = want.size
    # device tensors with guard elements on either side
    buf = torch.full((cells + 2,), -7, dtype=torch.int64, device="cuda:0")
    kbuf = torch.full((3 + 2,), -7, dtype=torch.int64, device="cuda:0")
    edges = np.array(H.DEFAULT_EDGES, np.int32)
    assert engine.lib.ftk_end_context(engine.ctx, cid, rid, 32, L.ptr(edges), 3, 30, 0, L.ptr(buf[1:1 + cells]), L.ptr(kbuf[1:4])) == L.FTK_OK
    bbuf = torch.full((25 + 2,), -7, dtype=torch.int64, device="cuda:0")
    assert engine.lib.ftk_ref_context(engine.ctx, rid, 0, 1 << 30, L.ptr(bbuf[1:26])) == L.FTK_OK
    engine.sync()
    host, khost, bhost = buf.cpu().numpy(), kbuf.cpu().numpy(), bbuf.cpu().numpy()
    assert np.array_equal(host[1:-1].reshape(want.shape), want) and host[0] == -7 and host[-1] == -7
    assert np.array_equal(khost[1:-1], want_kept) and khost[0] == -7 and khost[-1] == -7
    assert np.array_equal(bhost[1:-1], H.restated_ref_context(world["bases"]["eA"], 0, 1 << 30)) and bhost[0] == -7 and bhost[-1] == -7
    # Engine.end_context(out=...) returns what it was given
    buf.fill_(-7)
    table, kept = engine.end_context("ec:eA", rid, 32, H.DEFAULT_EDGES, 30, "ends", out=buf[1:1 + cells])
    engine.sync()
    assert table.data_ptr() == buf[1:].data_ptr() and np.array_equal(buf.cpu().numpy()[1:-1].reshape(want.shape), want)
    assert np.array_equal(kept, want_kept)
    # host tables pre-filled with 7 are fully overwritten
    table, kept, out25 = np.full(want.shape, 7, np.int64), np.full(3, 7, np.int64), np.full(25, 7, np.int64)
    assert engine.lib.ftk_end_context(engine.ctx, cid, rid, 32, L.ptr(edges), 3, 30, 0, L.ptr(table), L.ptr(kept)) == L.FTK_OK
    assert engine.lib.ftk_ref_context(engine.ctx, rid, 0, 30_011, L.ptr(out25)) == L.FTK_OK
    assert np.array_equal(table, want) and np.array_equal(kept, want_kept) and (table == 0).sum() > 1000
    assert np.array_equal(out25, H.restated_ref_context(world["bases"]["eA"], 0, 30_011))
    # an empty contig: zeros
    engine.load_contig("ec:empty", np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    table[:], kept[:] = 7, 7
    ecid = engine.contig_id("ec:empty")
    assert engine.lib.ftk_end_context(engine.ctx, ecid, rid, 32, L.ptr(edges), 3, 30, 1, L.ptr(table), L.ptr(kept)) == L.FTK_OK
    assert not table.any() and not kept.any()
    engine.release("ec:empty")


# ---- 6. the C ABI's argument errors ------------------------------------------------------------------------------------
def test_argument_errors(engine, world):
    from finaletoolkit_amd import _lib as L
    lib, ctx = engine.lib, engine.ctx
    rid = rid_of(engine, world, "2bit", "eA")
    cid = engine.contig_id("ec:eA")
    table = np.full(8 * 2 * 256 * 25, 7, np.int64)
    kept = np.full(8, 7, np.int64)
    out25 = np.full(25, 7, np.int64)
    INV, NOC = L.FTK_ERR_INVALID, L.FTK_ERR_NO_CONTIG

    def ends(cid_=cid, rid_=rid, w=32, edges=H.DEFAULT_EDGES, n_classes=None, anchor=0, out=table, n_kept=kept, ctx_=ctx, null_edges=False):
        ed = np.array(edges, np.int32)
        return lib.ftk_end_context(ctx_, cid_, rid_, w, None if null_edges else L.ptr(ed), len(edges) - 1 if n_classes is None else n_classes,
                                   30, anchor, L.ptr(out), L.ptr(n_kept))

    def failed(rc, code):
        assert rc == code, (rc, code)
        assert lib.ftk_last_error(ctx)

    assert ends() == L.FTK_OK  # the arguments the failing calls vary
    table[:], kept[:] = 7, 7
    assert ends(ctx_=None) == INV and lib.ftk_ref_context(None, rid, 0, 100, L.ptr(out25)) == INV
    failed(ends(out=None), INV)
    failed(ends(n_kept=None), INV)
    failed(ends(null_edges=True), INV)
    failed(lib.ftk_ref_context(ctx, rid, 0, 100, None), INV)
    failed(ends(cid_=987_654), NOC)
    failed(ends(rid_=987_654), NOC)
    failed(lib.ftk_ref_context(ctx, 987_654, 0, 100, L.ptr(out25)), NOC)
    for w in (0, -1, 129, 1 << 20):
        failed(ends(w=w), INV)
    nine = tuple(range(1, 11))
    failed(ends(n_classes=0), INV)
    failed(ends(n_classes=-1), INV)
    failed(ends(edges=nine), INV)  # 9 classes
    for edges in ((0, 100), (-5, 100), (100, 100), (1, 200, 150), (1, 150, 150, 300), (1, (1 << 30) + 1), (150, 100)):
        failed(ends(edges=edges), INV)
    assert ends(edges=(1, 1 << 30)) == L.FTK_OK and ends(edges=((1 << 30) - 1, 1 << 30)) == L.FTK_OK  # the bounds themselves
    table[:], kept[:] = 7, 7
    for anchor in (-1, 2, 7):
        failed(ends(anchor=anchor), INV)
    for lo, hi in ((-1, 100), (100, 99)):
        failed(lib.ftk_ref_context(ctx, rid, lo, hi, L.ptr(out25)), INV)
    with pytest.raises(L.FtkError):
        engine.end_context("ec:eA", rid, 0, H.DEFAULT_EDGES)
    with pytest.raises(L.FtkError):
        engine.end_context("ec:eA", rid, 32, (5, 4))
    with pytest.raises(ValueError):
        engine.end_context("ec:eA", rid, 32, H.DEFAULT_EDGES, anchor="middle")
    with pytest.raises(L.FtkError):
        engine.ref_context(rid, 5, 4)
    # an image without its layout
    bare = engine.ref_upload(("ec-test", "bare"), np.zeros(64, np.uint8), 1)
    failed(ends(rid_=bare), INV)
    assert b"layout" in lib.ftk_last_error(ctx)
    failed(lib.ftk_ref_context(ctx, bare, 0, 100, L.ptr(out25)), INV)
    assert b"layout" in lib.ftk_last_error(ctx)
    # nothing was written by any of them
    assert np.all(table == 7) and np.all(kept == 7) and np.all(out25 == 7)


# ---- 7. the product path -----------------------------------------------------------------------------------------------
def restated_result(world, frags, half_width, edges, anchor, mapq_min=30):
    table = np.zeros((len(edges) - 1, 2, 2 * half_width, 25), np.int64)
    kept, bg = np.zeros(len(edges) - 1, np.int64), np.zeros(25, np.int64)
    for name, (s, e, q) in frags.items():
        if name not in world["bases"]:
            continue
        t, k = H.restated_end_context(world["bases"][name], s, e, q, half_width, edges, mapq_min, anchor)
        table, kept, bg = table + t, kept + k, bg + H.restated_ref_context(world["bases"][name], 0, world["bases"][name].n)
    return table, kept, bg


def same_result(a, b):
    return (np.array_equal(a.table, b.table) and np.array_equal(a.n_kept, b.n_kept) and np.array_equal(a.background, b.background)
            and (a.half_width, a.length_edges, a.anchor, a.skipped_contigs) == (b.half_width, b.length_edges, b.anchor, b.skipped_contigs))


def test_frag_end_context_end_to_end(engine, world, tmp_path):
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
            results[tag] = utils.frag_end_context(path, ref)
        ours = [w for w in caught if issubclass(w.category, UserWarning) and "not in the reference" in str(w.message)]
        assert len(ours) == 1 and "eX" in str(ours[0].message)
    assert same_result(results["bam"], results["frag"])
    res = results["bam"]
    assert isinstance(res, utils.EndContext)
    assert (res.half_width, res.length_edges, res.anchor, res.skipped_contigs) == (32, (1, 150, 221, 1001), "ends", ("eX",))
    assert res.table.dtype == np.int64 and res.table.shape == (3, 2, 64, 25) and res.background.shape == (25,)
    want_bam = {c: (v[0], v[1], v[2]) for c, v in bam_expected(bam)[0].items()}
    want_frag = {c: (v[0], v[1], v[2]) for c, v in read_frag_gz(frag).items()}
    for want in (want_bam, want_frag):
        table, kept, bg = restated_result(world, want, 32, H.DEFAULT_EDGES, "ends")
        assert np.array_equal(res.table, table) and np.array_equal(res.n_kept, kept) and np.array_equal(res.background, bg)
        assert (kept > 100).all() and table[..., N].any()
    assert np.array_equal(res.mono.sum(axis=-1), np.broadcast_to(res.n_kept[:, None, None], (3, 2, 64)))
    assert res.enrichment(2).shape == (3, 2, 64, 16) and np.isfinite(res.enrichment(1)).all()
    # one contig, the other anchor, other classes and width, another reference format
    one = utils.frag_end_context(frag, world["paths"]["fa50"], contig="eC", quality_threshold=0, half_width=7,
                                 length_edges=(100, 167, 300), anchor="centre")
    table, kept, bg = restated_result(world, {"eC": want_frag["eC"]}, 7, (100, 167, 300), "centre", 0)
    assert np.array_equal(one.table, table) and np.array_equal(one.n_kept, kept) and np.array_equal(one.background, bg)
    assert one.skipped_contigs == () and one.anchor == "centre"
    with pytest.raises(ValueError, match="contig not present"):
        utils.frag_end_context(frag, ref, contig="13")
    # the command line, in a child process, and both suffixes
    for suffix in (".tsv", ".tsv.gz"):
        out = str(tmp_path / ("cli" + suffix))
        r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.endcontext", frag, ref, out, "-q", "30", "--half-width", "32",
                            "--length-edges", "1", "150", "221", "1001"], cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert "eX" in r.stderr  # the warning
        text = gzip.open(out, "rt").read() if suffix.endswith(".gz") else open(out).read()
        assert text == writers.end_context_text(res)
        lines = text.splitlines()
        assert lines[0] + "\n" == writers.END_CONTEXT_HEADER
        count = np.zeros((3, 2, 64, 21), np.int64)
        for ln in lines[1:]:
            lo, hi, end, o, motif, k, f, x = ln.split("\t")
            c = (1, 150, 221).index(int(lo))
            assert int(hi) == (150, 221, 1001)[c]
            count[c, "UD".index(end), int(o) + 32, writers.END_CONTEXT_MOTIFS.index(motif)] = int(k)
        assert np.array_equal(count[..., :5], res.mono) and np.array_equal(count[..., 5:], res.dinuc)
