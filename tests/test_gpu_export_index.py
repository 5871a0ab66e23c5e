"""GPU: the tabix inputs of the export (``format_pass2_kernel`` / ``format_scan_kernel`` in ``csrc/ftk_fragtext.hip``,
the virtual offsets of ``ftk_frags_write``) compared EXACTLY with a restatement written here from the SAM / tabix
text: ``runs`` (bin, begin, end) and ``linear`` of ``Engine.write_contig`` against the spec bins of the kept rows,
run-length collapsed, and the first kept row of every 16 kb window, placed with the member table parsed from the file.
Region queries (``tests/test_gpu_frag_export.py``) tolerate a linear entry that is too small and a run that is split or
merged wrongly; equality does not.

The row counts cross the scan's three levels (a thread's 4 rows, a workgroup's 1024, a scan chunk of 512 workgroups =
524288 rows); the dropped stretches empty a whole thread, workgroup and chunk.  Nothing here comes from
``finaletoolkit_amd.bgzf``'s index helpers: bins are ``spec_reg2bin`` of ``tests/test_frag_export.py``, the text is the
host formatter's (``host_rows``), the member table is ``split_members`` on the file."""
import gzip
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_frag_export as T  # noqa: E402  (spec_reg2bin)
from helpers import first_difference  # noqa: E402
import test_frag_filter as F  # noqa: E402  (the mask's restated rule)
from test_gpu_frag_export import EOF, host_rows, split_members  # noqa: E402

pytestmark = pytest.mark.gpu
B = 0xFF00
LEVELS = ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1))  # SAM spec 5.3: shift and first bin of each level


# ---- the restatement ---------------------------------------------------------------------------------------------------
def expected_loop(s, e, row_len, voff):
    """Plain loops.  ``row_len``: bytes of every kept row in file order; ``voff(t)``: text offset -> virtual offset."""
    off, bins, first = 0, [], {}
    for a, b, ln in zip(s.tolist(), e.tolist(), row_len.tolist()):
        b = max(b, a + 1)  # (a zero-length row takes the base it sits on)
        k = T.spec_reg2bin(a, b)
        if not bins or bins[-1][0] != k:
            bins.append((k, off))
        for w in range(a >> 14, ((b - 1) >> 14) + 1):
            first.setdefault(w, off)
        off += ln
    run_bin = [k for k, _ in bins]
    run_beg = [voff(t) for _, t in bins]
    run_end = run_beg[1:] + [voff(off)] if bins else []
    linear = [0] * (max(first) + 1 if first else 0)
    for w in range(len(linear) - 1, -1, -1):
        linear[w] = voff(first[w]) if w in first else linear[w + 1]
    return (np.array(run_bin, np.int32), np.array(run_beg, np.uint64), np.array(run_end, np.uint64),
            np.array(linear, np.uint64))


def expected_numpy(s, e, row_len, voff_np):
    """The same with numpy, for the large cases (held against ``expected_loop`` wherever the case is small enough)."""
    n = len(s)
    if n == 0:
        z = np.zeros(0, np.uint64)
        return np.zeros(0, np.int32), z, z, z
    s = s.astype(np.int64)
    last = np.maximum(e.astype(np.int64), s + 1) - 1
    off = np.concatenate(([0], np.cumsum(row_len)))
    bins, done = np.zeros(n, np.int64), np.zeros(n, bool)
    for shift, first_bin in LEVELS:
        m = ~done & ((s >> shift) == (last >> shift))
        bins[m] = first_bin + (s[m] >> shift)
        done |= m
    opens = np.concatenate(([True], bins[1:] != bins[:-1]))
    run_beg = voff_np(off[:-1][opens])
    run_end = np.concatenate((run_beg[1:], voff_np(off[-1:])))
    w0, w1 = s >> 14, last >> 14
    cnt = w1 - w0 + 1
    row = np.repeat(np.arange(n), cnt)
    win = np.repeat(w0, cnt) + np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    first = np.full(int(w1.max()) + 1, n, np.int64)
    np.minimum.at(first, win, row)  # the first row, in file order, whose window range holds w
    idx = np.where(first < n, np.arange(len(first)), len(first))
    nxt = np.minimum.accumulate(idx[::-1])[::-1]  # a window no row overlaps: the next window that has one
    linear = voff_np(off[first[nxt]])
    return bins[opens].astype(np.int32), run_beg, run_end, linear


def check_case(engine, path, s, e, q, st=None, name="chr1", mapq_min=0, layout="frag", mask=None, mask_keep=None, append=False,
               write_eof=False):
    """Load, write, read the file back, compare everything; returns ``(result, kept rows)``."""
    s, e, q = np.asarray(s, np.int32), np.asarray(e, np.int32), np.asarray(q, np.uint8)
    st = (np.arange(len(s)) % 3 == 0).astype(np.uint8) if st is None else np.asarray(st, np.uint8)
    assert np.all(s[1:] >= s[:-1]) and np.all(e >= s)
    before = open(path, "rb").read() if append and os.path.exists(path) else b""
    key = "idx:" + os.path.basename(path)
    engine.load_contig(key, s, e, q, st)
    try:
        res = engine.write_contig(key, name, path, quality_threshold=mapq_min, layout=layout, append=append, write_eof=write_eof,
                                  mask=mask)
    finally:
        engine.release(key)
    keep = q >= mapq_min
    if mask_keep is not None:
        keep &= mask_keep
    ks, ke = s[keep], e[keep]
    text = host_rows(name, ks, ke, q[keep], st[keep], layout)
    raw = open(path, "rb").read()
    # the file: what was there, this contig's members, the end marker if asked for
    assert res["first_off"] == len(before) and first_difference(raw[:len(before)], before) is None
    assert res["end_off"] == len(raw) - (28 if write_eof else 0) and (not write_eof or raw[-28:] == EOF)
    members = split_members(raw[res["first_off"]:res["end_off"]])
    assert res["rows"] == int(keep.sum()) and res["text_bytes"] == len(text)
    assert first_difference(gzip.decompress(raw[res["first_off"]:res["end_off"]]), text) is None
    assert [m[2] for m in members] == [min(B, len(text) - k * B) for k in range(len(members))]  # full members, then the rest
    boff = res["first_off"] + np.concatenate(([0], np.cumsum([m[3] for m in members]))).astype(np.int64)
    assert boff[-1] == res["end_off"]
    total = len(text)

    def voff(t):
        return (int(boff[t // B]) << 16 | t % B) if t < total else res["end_off"] << 16

    def voff_np(t):
        t = np.asarray(t, np.int64)
        inside = np.minimum(t, max(total - 1, 0))
        return np.where(t < total, (boff[inside // B] << 16) | (inside % B), res["end_off"] << 16).astype(np.uint64)
    nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 10)
    assert len(nl) == len(ks)
    row_len = np.diff(np.concatenate(([-1], nl)))
    want = expected_numpy(ks, ke, row_len, voff_np)
    if len(ks) <= 6000:
        loop = expected_loop(ks, ke, row_len, voff)
        assert all(np.array_equal(a, b) for a, b in zip(want, loop))
    got = (*res["runs"], res["linear"])
    for what, g, w in zip(("run bins", "run begins", "run ends", "linear index"), got, want):
        assert g.dtype == w.dtype and len(g) == len(w), (what, len(g), len(w))
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, int(bad[0]), int(g[bad[0]]), int(w[bad[0]]), len(bad))
    return res, (ks, ke)


def gen_rows(n, seed=0, origin=0, gap=60):
    """Sorted starts, lengths 1..400; the rows cross a 16 kb edge every few hundred rows."""
    rng = np.random.default_rng(seed)
    s = (origin + np.cumsum(rng.integers(0, gap, n))).astype(np.int32)
    e = (s + rng.integers(1, 401, n)).astype(np.int32)
    q = rng.integers(0, 61, n).astype(np.uint8)
    return s, e, q


# ---- row counts across the scan's levels -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 2049, 524287, 524288, 524289, 525313])
def test_row_counts_across_thread_workgroup_and_chunk(engine, tmp_path, n):
    s, e, q = gen_rows(n, seed=n)
    res, (ks, ke) = check_case(engine, str(tmp_path / "n.gz"), s, e, q)
    assert res["rows"] == n
    if n >= 1023:  # rows straddle 16 kb edges: runs change, and level-1 bins appear between the level-0 ones
        assert int(((ks >> 14) != ((ke - 1) >> 14)).sum()) >= 1 and len(res["runs"][0]) > 2 and (res["runs"][0] < 4681).any()
    if n == 2049:  # and with the MAPQ rule dropping rows all over
        res, _ = check_case(engine, str(tmp_path / "q.gz"), s, e, q, mapq_min=30)
        assert 0 < res["rows"] < n


# ---- stretches without a kept row ----------------------------------------------------------------------------------------
STRETCHES = {"thread": (13, 4, 8), "workgroup": (3000, 1024, 2048), "chunk": (1_600_000, 524288, 1048576)}


@pytest.mark.parametrize("same_bin", [True, False], ids=["same_bin", "other_bin"])
@pytest.mark.parametrize("what", sorted(STRETCHES))
def test_dropped_stretch(engine, tmp_path, what, same_bin):
    """Every row in front of the stretch lies in 16 kb window 0 (bin 4681); the rows behind it lie there too (no run may
    open: one run in all) or in window 1 (exactly one run opens: two in all)."""
    n, lo, hi = STRETCHES[what]
    rng = np.random.default_rng(lo)
    s = np.concatenate((np.sort(rng.integers(0, 5000, lo)), np.sort(rng.integers(5000, 6000, hi - lo)),
                        np.sort(rng.integers(6000, 15000, n - hi)) + (0 if same_bin else 16384))).astype(np.int32)
    e = (s + rng.integers(1, 401, n)).astype(np.int32)
    q = np.full(n, 60, np.uint8)
    q[lo:hi] = 0
    res, _ = check_case(engine, str(tmp_path / "d.gz"), s, e, q, mapq_min=30)
    assert res["rows"] == n - (hi - lo)
    assert res["runs"][0].tolist() == ([4681] if same_bin else [4681, 4682])
    assert len(res["linear"]) == (1 if same_bin else 2)


def test_dropped_first_last_all_and_all_but_one(engine, tmp_path):
    n = 2500
    s, e, _ = gen_rows(n, seed=8)
    for tag, kept in (("first", np.arange(n) != 0), ("last", np.arange(n) != n - 1), ("first4", np.arange(n) >= 4),
                      ("last_wg", np.arange(n) < 2048), ("one", np.arange(n) == 1500), ("one_first", np.arange(n) == 0),
                      ("one_last", np.arange(n) == n - 1), ("none", np.zeros(n, bool))):
        q = np.where(kept, 60, 29).astype(np.uint8)
        res, _ = check_case(engine, str(tmp_path / (tag + ".gz")), s, e, q, mapq_min=30, write_eof=True)
        assert res["rows"] == int(kept.sum()), tag
        if tag.startswith("one"):
            assert len(res["runs"][0]) == 1 and res["runs"][2][0] == res["end_off"] << 16
        if tag == "none":  # a valid file that holds the end marker alone; no run, no window
            assert len(res["runs"][0]) == 0 and len(res["linear"]) == 0 and res["text_bytes"] == 0
            assert os.path.getsize(str(tmp_path / "none.gz")) == 28 and res["first_off"] == res["end_off"] == 0


# ---- every bin level -----------------------------------------------------------------------------------------------------
def test_rows_at_the_edges_of_every_bin_level(engine, tmp_path):
    rows = [(16384, 16384), (16384 - 50, 16384), (16383, 16385), (0, 1), (5, 5)]
    for k, (shift, _) in enumerate(LEVELS):
        edge = (3 + k) << shift  # (distinct edges, none of them an edge of the next level)
        rows += [(edge - 100, edge + 100), (edge - 50, edge), (edge, edge), (edge, edge + 1), (edge - 1, edge + 1), (edge - 1, edge)]
    rows += [((1 << 29) - 10, (1 << 29) + 10), ((1 << 29) - 10, 1 << 29), (1 << 29, (1 << 29) + 1), ((1 << 30) - 2, (1 << 30) - 1)]
    rows.sort(key=lambda r: r[0])
    s, e = np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32)
    res, _ = check_case(engine, str(tmp_path / "lv.gz"), s, e, np.full(len(s), 7, np.uint8))
    got = set(res["runs"][0].tolist())
    assert 0 in got and all(any(first <= b < first + (1 << (29 - shift)) for b in got) for shift, first in LEVELS)
    assert len(res["linear"]) == 1 << 16


def test_bins_alternating_on_every_row_and_one_bin_for_all(engine, tmp_path):
    n = 2100  # crosses the workgroup boundaries at 1024 and 2048
    s = (np.arange(n) * 7).astype(np.int32)  # windows 0 (and 1 from row 2341 on: not reached)
    e = np.where(np.arange(n) % 2 == 0, s + 1, s + 20000).astype(np.int32)  # bin 4681 | a level-1 bin (the row crosses 16384)
    res, _ = check_case(engine, str(tmp_path / "alt.gz"), s, e, np.full(n, 9, np.uint8))
    assert len(res["runs"][0]) == n and res["runs"][0][:4].tolist() == [4681, 585, 4681, 585]
    s = (5 * 16384 + np.arange(n) * 7).astype(np.int32)
    res, _ = check_case(engine, str(tmp_path / "one.gz"), s, s + 100, np.full(n, 9, np.uint8))
    assert res["runs"][0].tolist() == [4681 + 5] and len(res["linear"]) == 6 and len(set(res["linear"].tolist())) == 1


# ---- long reach ----------------------------------------------------------------------------------------------------------
def test_first_row_reaches_every_window(engine, tmp_path):
    s, e, q = gen_rows(2500, seed=3, origin=1)
    s, e, q = np.concatenate(([0], s)), np.concatenate(([(1 << 30) - 1], e)), np.concatenate(([60], q))
    res, _ = check_case(engine, str(tmp_path / "reach.gz"), s, e, q)
    assert len(res["linear"]) == 1 << 16 and (res["linear"] == res["linear"][0]).all()  # no later row writes an entry


def test_row_reaching_300_windows_then_a_gap(engine, tmp_path):
    a = gen_rows(1500, seed=4)
    far = int(a[0][-1]) + 500
    long_end = far + 300 * 16384
    b = gen_rows(1200, seed=5, origin=far + 10, gap=4000)  # inside its reach, over all 300 windows
    assert far + 16384 < b[0][-1] < long_end and b[1].max() < long_end
    c = gen_rows(700, seed=6, origin=long_end + 9 * 16384)  # behind a gap of windows that no row overlaps
    s = np.concatenate((a[0], [far], b[0], c[0]))
    e = np.concatenate((a[1], [long_end], b[1], c[1]))
    q = np.concatenate((a[2], [60], b[2], c[2]))
    res, _ = check_case(engine, str(tmp_path / "gap.gz"), s, e, q)
    w0, w1, w2 = far >> 14, (long_end - 1) >> 14, int(c[0][0]) >> 14
    lin = res["linear"]
    assert w2 - w1 >= 8 and (lin[w0 + 1:w1 + 1] == lin[w0 + 1]).all() and (lin[w1 + 1:w2 + 1] == lin[w2]).all() and lin[w2] > lin[w1]


# ---- BGZF geometry ---------------------------------------------------------------------------------------------------------
def rows_of_24_bytes(n):
    """``c12<tab>7 digits<tab>7 digits<tab>1 digit<tab>strand<newline>`` = 24 bytes; 0xFF00 = 2720 rows.  Rows 0..2719
    lie in 16 kb window 61, the rest in window 62."""
    i = np.arange(n)
    s = np.where(i < 2720, 1_000_000 + i, 62 * 16384 + i).astype(np.int32)
    return s, (s + 100).astype(np.int32), np.full(n, 5, np.uint8)


@pytest.mark.parametrize("n", [2720, 5440, 5445])
def test_text_that_ends_or_turns_on_a_member_boundary(engine, tmp_path, n):
    s, e, q = rows_of_24_bytes(n)
    res, _ = check_case(engine, str(tmp_path / "g.gz"), s, e, q, name="c12")
    assert res["text_bytes"] == 24 * n and (24 * n) % B == (0 if n != 5445 else 120)
    if n > 2720:  # the second run opens on the first byte of the second member
        second = res["first_off"] + split_members(open(str(tmp_path / "g.gz"), "rb").read())[0][3]
        assert res["runs"][0].tolist() == [4681 + 61, 4681 + 62] and res["runs"][1][1] == second << 16 == res["runs"][2][0]
    assert res["runs"][2][-1] == res["end_off"] << 16


def test_a_row_straddling_the_member_boundary(engine, tmp_path):
    s, e, q = gen_rows(3000, seed=10, origin=1_000_000)
    q = (10 + q % 50).astype(np.uint8)
    assert s.max() + 400 < 10_000_000
    res, _ = check_case(engine, str(tmp_path / "s.gz"), s, e, q, name="chr12")
    assert res["text_bytes"] == 27 * 3000 and B % 27 != 0  # row 2417 holds text offset 0xFF00


@pytest.mark.parametrize("write_eof", [False, True])
def test_append_shifts_every_offset(engine, tmp_path, write_eof):
    path = str(tmp_path / "two.gz")
    s, e, q = gen_rows(4000, seed=11)
    first, _ = check_case(engine, path, s, e, q, name="chr1")
    s, e, q = gen_rows(5000, seed=12)
    res, _ = check_case(engine, path, s, e, q, name="chr2", append=True, write_eof=write_eof)
    assert res["first_off"] == first["end_off"] > 0 and int(res["linear"].min()) >> 16 >= first["end_off"]
    alone, _ = check_case(engine, str(tmp_path / "alone.gz"), s, e, q, name="chr2")
    assert np.array_equal(res["linear"], alone["linear"] + (np.uint64(res["first_off"]) << np.uint64(16)))
    assert np.array_equal(res["runs"][1], alone["runs"][1] + (np.uint64(res["first_off"]) << np.uint64(16)))


# ---- layouts and masks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["frag", "bed6", "bed3"])
def test_layouts(engine, tmp_path, layout):
    s, e, q = gen_rows(5000, seed=13, origin=99_000)  # starts pass from 5 to 6 digits
    res, _ = check_case(engine, str(tmp_path / "l.gz"), s, e, q, layout=layout, mapq_min=10)
    assert res["text_bytes"] > B  # (more than one member in every layout)


@pytest.mark.parametrize("policy", ["midpoint", "any"])
def test_region_mask(engine, tmp_path, policy):
    from finaletoolkit_amd.engine import RegionMask
    s, e, q = gen_rows(3000, seed=14)
    top = int(e.max())
    ws = np.arange(0, top, 9000, dtype=np.int32)
    wl = (ws, (ws + 6000).astype(np.int32))
    bs = np.arange(2500, top, 20_000, dtype=np.int32)
    bl = (bs, (bs + 1500).astype(np.int32))
    keep = F.restated_keep_sorted(policy, s, e, list(zip(*map(np.ndarray.tolist, wl))), list(zip(*map(np.ndarray.tolist, bl))))
    assert 500 < keep.sum() < 2500
    res, _ = check_case(engine, str(tmp_path / "m.gz"), s, e, q, mapq_min=10, mask=RegionMask(wl, bl, policy), mask_keep=keep)
    assert 0 < res["rows"] < keep.sum()
