"""GPU: region masks in the export (``mask_keep_kernel`` in ``csrc/ftk_fragtext.hip``) - ``Engine.mask_keep`` bit for
bit against the literal restatement of the two policy lines (``tests/test_frag_filter.py``) on hand-built edges and on
both sides of the kernel's LDS / global-search switch, ``format_rows(mask=...)`` against the host formatter, the C
ABI's argument errors, and ``frag_filter`` end to end against ``tests/golden/export_mask.json.gz`` with the index read
back by the tabix reader of ``tests/test_frag_export.py`` and by ``AlignmentWrapper``."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_frag_export as T  # noqa: E402  (the tabix reader and the region set)
import test_frag_filter as F  # noqa: E402  (the restatement, the golden, the synthetic recipe)

pytestmark = pytest.mark.gpu
ROOT = T.ROOT
FRAG = os.path.join(ROOT, "tests", "data", "12.3444.b37.frag.gz")
BAM = os.path.join(ROOT, "tests", "data", "12.3444.b37.bam")
LAYOUTS = ("frag", "bed6", "bed3")
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
POLICIES = ("midpoint", "any")


def region_mask(whitelist=None, blacklist=None, policy="midpoint"):
    """RegionMask from lists of (start, stop) in any order (merged the way the loader merges them) or None."""
    from finaletoolkit_amd import utils
    from finaletoolkit_amd.engine import RegionMask

    def pair(iv):
        if iv is None:
            return None
        return utils.merge_intervals([a for a, _ in iv], [b for _, b in iv])
    return RegionMask(pair(whitelist), pair(blacklist), policy)


def host_rows(name, s, e, q, st, layout):
    from finaletoolkit_amd import writers
    with writers.frag_rows(name, s, e, q, st, layout == "bed6") as rows:
        text = rows.tobytes()
    if layout == "bed3":
        text = b"".join(b"\t".join(ln.split(b"\t")[:3]) + b"\n" for ln in text.splitlines())
    return text


def numpy_keep(s, e, q, mapq_min, min_len, max_len):
    ln = e.astype(np.int64) - s
    keep = q >= mapq_min
    if min_len is not None:
        keep &= ln >= min_len
    if max_len is not None:
        keep &= ln <= max_len
    return keep


# ---- 1. edges --------------------------------------------------------------------------------------------------------
RAW = [(100, 110), (110, 120), (200, 201), (300, 400), (350, 380), (500, 600), (600, 601), (40, 41)]  # touching, nested, unsorted


def edge_rows():
    rows = set()
    for a, b in RAW:
        for mid in (a - 1, a, b - 1, b):
            for ln in (0, 1, 2, 3, 10, 11):  # zero-length, odd and even lengths
                s = mid - ln // 2
                if s >= 0:
                    rows.add((s, s + ln))  # (s + s + ln) // 2 == mid
        rows |= {(max(a - 3, 0), a), (max(a - 3, 0), a + 1), (b - 1, b + 2), (b, b + 2)}  # ends on the bounds ("any")
    rows |= {(90, 650), (0, 1000), (105, 115), (119, 121)}  # spanning several intervals, across the touching pair
    rows = sorted(rows)
    while len(rows) % 4 == 0 or len(rows) % 64 == 0:
        rows.append((rows[-1][0] + 1, rows[-1][1] + 3))
    s = np.array([r[0] for r in rows], np.int32)
    e = np.array([r[1] for r in rows], np.int32)
    return s, e


def test_mask_keep_on_hand_built_edges(engine, tmp_path):
    from finaletoolkit_amd import utils
    from finaletoolkit_amd.engine import RegionMask
    s, e = edge_rows()
    n = len(s)
    assert n % 4 and n % 64 and n > 150 and (e == s).sum() >= 8
    q = np.full(n, 60, np.uint8)
    st = (np.arange(n) % 2).astype(np.uint8)
    engine.load_contig("mask:edges", s, e, q, st)
    try:
        # touching intervals given unmerged to the loader: they stay apart (a zero-length fragment at 110 or 600 is in
        # neither of its neighbours under "any"), the nested one is merged
        bed = F.write_bed(tmp_path / "raw.bed", [("c", a, b) for a, b in RAW])
        loaded = utils.read_region_mask(bed)["c"]
        assert loaded[0].tolist() == [40, 100, 110, 200, 300, 500, 600] and loaded[1].tolist() == [41, 110, 120, 201, 400, 600, 601]
        assert (110, 110) in set(zip(s.tolist(), e.tolist())) and (600, 600) in set(zip(s.tolist(), e.tolist()))
        other = [(0, 5), (95, 100), (120, 130), (399, 500), (640, 660)]
        for policy in POLICIES:
            in_raw = F.restated_keep(policy, s, e, whitelist=RAW)
            in_other = F.restated_keep(policy, s, e, whitelist=other)
            assert 0 < in_raw.sum() < n and 0 < in_other.sum() < n
            for mask, want in ((RegionMask(loaded, None, policy), in_raw),
                               (RegionMask(None, loaded, policy), ~in_raw),
                               (region_mask(RAW, other, policy), in_raw & ~in_other),
                               (region_mask(other, RAW, policy), in_other & ~in_raw),
                               # sorted, disjoint but TOUCHING intervals straight to the library (no loader)
                               (RegionMask((np.array([100, 110, 200], np.int32), np.array([110, 120, 201], np.int32)), None, policy),
                                F.restated_keep(policy, s, e, whitelist=[(100, 110), (110, 120), (200, 201)])),
                               # an empty whitelist keeps nothing, n_wl < 0 keeps all
                               (RegionMask((np.zeros(0, np.int32), np.zeros(0, np.int32)), None, policy), np.zeros(n, bool)),
                               (RegionMask((np.zeros(0, np.int32), np.zeros(0, np.int32)), loaded, policy), np.zeros(n, bool)),
                               (RegionMask(None, None, policy), np.ones(n, bool)),
                               (RegionMask(None, (np.zeros(0, np.int32), np.zeros(0, np.int32)), policy), np.ones(n, bool))):
                got, kept = engine.mask_keep("mask:edges", mask)
                assert got.dtype == bool and np.array_equal(got, want), (policy, np.nonzero(got != want)[0][:10], s[got != want][:10], e[got != want][:10])
                assert kept == int(want.sum())
        # the two policies differ on these rows, so each test above can tell them apart
        assert not np.array_equal(F.restated_keep("midpoint", s, e, whitelist=RAW), F.restated_keep("any", s, e, whitelist=RAW))
    finally:
        engine.release("mask:edges")
    # an empty contig
    z32, z8 = np.zeros(0, np.int32), np.zeros(0, np.uint8)
    engine.load_contig("mask:empty", z32, z32, z8, z8)
    try:
        got, kept = engine.mask_keep("mask:empty", region_mask(RAW, None, "any"))
        assert len(got) == 0 and kept == 0
        assert engine.format_rows("mask:empty", "c", 0, None, None, "frag", mask=region_mask(RAW, None, "any")) == (b"", 0)
    finally:
        engine.release("mask:empty")


@pytest.mark.parametrize("n", [1, 3, 63, 65, 255, 257, 1023, 1025, 4099])
def test_mask_keep_row_counts_around_the_word_and_tile_sizes(engine, n):
    rng = np.random.default_rng(n)
    s = np.sort(rng.integers(0, 20 * n + 50, n)).astype(np.int32)
    e = (s + rng.integers(0, 40, n)).astype(np.int32)
    iv = [(int(a), int(a) + int(w)) for a, w in zip(rng.integers(0, 20 * n + 50, n // 3 + 2), rng.integers(1, 25, n // 3 + 2))]
    engine.load_contig("mask:n", s, e, np.full(n, 60, np.uint8), np.zeros(n, np.uint8))
    try:
        for policy in POLICIES:
            want = F.restated_keep(policy, s, e, whitelist=iv)
            got, kept = engine.mask_keep("mask:n", region_mask(iv, None, policy))
            assert np.array_equal(got, want) and kept == int(want.sum()), (n, policy)
            got, kept = engine.mask_keep("mask:n", region_mask(None, iv, policy))
            assert np.array_equal(got, ~want) and kept == n - int(want.sum()), (n, policy)
    finally:
        engine.release("mask:n")


# ---- 2. both sides of the LDS switch ---------------------------------------------------------------------------------
def tile_slices(s, e, starts, policy):
    """Intervals of a mask each tile of 1024 rows can touch, as the kernel counts them: from the last interval that
    starts at or before the tile's smallest search key to the last one at or before its largest."""
    key = ((s.astype(np.int64) + e) >> 1) if policy == "midpoint" else e.astype(np.int64) - 1
    out = []
    for i in range(0, len(s), 1024):
        k = key[i:i + 1024]
        lo = max(int(np.searchsorted(starts, k.min(), side="right")) - 1, 0)
        hi = int(np.searchsorted(starts, k.max(), side="right"))
        out.append(max(hi - lo, 0))
    return np.array(out)


@pytest.fixture(scope="module")
def big():
    from finaletoolkit_amd import synth
    s, e, q, st = synth.synth_contig(1_000_000, depth=30.0, seed=77)
    if len(s) % 4 == 0:
        s, e, q, st = s[:-1], e[:-1], q[:-1], st[:-1]
    assert len(s) >= 90_000 and len(s) % 4
    return s, e, q, st


def big_masks(engine, s, e):
    """sparse: a few intervals per tile.  dense: over the first 300 kb an interval period derived from the kernel's
    constant, so that every tile there can touch more than twice what a workgroup stages; sparse behind it."""
    L = engine.mask_lds_intervals()
    assert L >= 64
    sparse = [(a, a + 700) for a in range(500, 1_000_000, 3000)] + [(a + 650, a + 900) for a in range(500, 1_000_000, 9000)]
    spans = [int(e[i:i + 1024].max()) - int(s[i]) for i in range(0, len(s) - 1024, 1024)]
    period = max(min(spans) // (2 * L + 8), 2)
    width = max(period // 2, 1)
    dense = [(a, a + width) for a in range(0, 300_000, period)] + [(a, a + 700) for a in range(300_500, 1_000_000, 3000)]
    return L, sparse, dense


def test_mask_keep_on_both_sides_of_the_lds_switch(engine, big):
    from finaletoolkit_amd import utils
    s, e, q, st = big
    L, sparse, dense = big_masks(engine, s, e)
    engine.load_contig("mask:big", s, e, q, st)
    try:
        for tag, iv in (("sparse", sparse), ("dense", dense)):
            ms, _ = utils.merge_intervals([a for a, _ in iv], [b for _, b in iv])
            for policy in POLICIES:
                per_tile = tile_slices(s, e, ms, policy)
                if tag == "sparse":  # every tile's slice is staged in LDS
                    assert 1 <= per_tile.max() <= L // 4 and np.median(per_tile) >= 3, (per_tile.max(), np.median(per_tile))
                else:  # tiles on both sides in ONE launch: over the budget in the dense part, far below it behind
                    assert (per_tile > L + 8).sum() >= 20 and (per_tile < L // 4).sum() >= 20, (per_tile.max(), per_tile.min())
                want = F.restated_keep_sorted(policy, s, e, whitelist=iv)
                assert 0.02 * len(s) < want.sum() < 0.98 * len(s)
                got, kept = engine.mask_keep("mask:big", region_mask(iv, None, policy))
                assert np.array_equal(got, want) and kept == int(want.sum()), (tag, policy, np.nonzero(got != want)[0][:10])
                got, kept = engine.mask_keep("mask:big", region_mask(None, iv, policy))
                assert np.array_equal(got, ~want) and kept == len(s) - int(want.sum()), (tag, policy, np.nonzero(got == want)[0][:10])
        # one mask per path in the same launch: dense whitelist (global search), sparse blacklist (LDS)
        for policy in POLICIES:
            want = F.restated_keep_sorted(policy, s, e, whitelist=dense, blacklist=sparse)
            got, kept = engine.mask_keep("mask:big", region_mask(dense, sparse, policy))
            assert np.array_equal(got, want) and kept == int(want.sum()) and kept > 1000, policy
    finally:
        engine.release("mask:big")


# ---- 3. the formatter with a mask ------------------------------------------------------------------------------------
def test_format_rows_with_a_mask_equals_the_host_formatter(engine, big):
    s, e, q, st = big
    L, sparse, dense = big_masks(engine, s, e)
    engine.load_contig("mask:fmt", s, e, q, st)
    try:
        for mapq_min, mn, mx in ((0, None, None), (30, 120, 180)):
            rule = numpy_keep(s, e, q, mapq_min, mn, mx)
            for layout in LAYOUTS:
                plain = engine.format_rows("mask:fmt", "chr5", mapq_min, mn, mx, layout)
                assert engine.format_rows("mask:fmt", "chr5", mapq_min, mn, mx, layout, mask=None) == plain
                assert plain == (host_rows("chr5", s[rule], e[rule], q[rule], st[rule], layout), int(rule.sum()))
            for policy, wl, bl in (("midpoint", sparse, None), ("any", None, sparse), ("midpoint", dense, sparse), ("any", sparse, dense)):
                keep = rule & F.restated_keep_sorted(policy, s, e, whitelist=wl, blacklist=bl)
                assert 100 < keep.sum() < rule.sum()
                for layout in LAYOUTS:
                    got, rows = engine.format_rows("mask:fmt", "chr5", mapq_min, mn, mx, layout, mask=region_mask(wl, bl, policy))
                    assert rows == int(keep.sum()), (policy, layout)
                    assert got == host_rows("chr5", s[keep], e[keep], q[keep], st[keep], layout), (policy, layout, mapq_min)
        # a mask that keeps nothing: no text, no rows
        assert engine.format_rows("mask:fmt", "chr5", 0, None, None, "frag", mask=region_mask([], None, "any")) == (b"", 0)
    finally:
        engine.release("mask:fmt")


# ---- 4. argument errors ----------------------------------------------------------------------------------------------
def test_mask_argument_errors(engine, tmp_path):
    from finaletoolkit_amd import _lib as L
    from finaletoolkit_amd.engine import RegionMask
    s = np.array([10, 20, 30], np.int32)
    engine.load_contig("mask:err", s, s + 5, np.full(3, 60, np.uint8), np.zeros(3, np.uint8))
    lib, cid = engine.lib, engine.contig_id("mask:err")
    i32 = lambda *v: np.array(v, np.int32)  # noqa: E731
    good = (i32(5, 40), i32(12, 50))
    bad = {"unsorted": (i32(40, 5), i32(50, 12)), "overlapping": (i32(5, 10), i32(12, 50)), "start == end": (i32(5, 40), i32(5, 50)),
           "start > end": (i32(5, 40), i32(12, 39))}
    try:
        keep, kept = np.zeros(3, np.uint8), C.c_int64()
        out, n, rows = C.c_void_p(), C.c_int64(), C.c_int64()
        res = L.ExportResult()
        path = str(tmp_path / "never.frag.gz").encode()

        def all_three(mask):
            m, alive = engine._mask_struct(mask)
            rcs = (lib.ftk_frags_mask_keep(engine.ctx, cid, C.byref(m), L.ptr(keep), C.byref(kept)),
                   lib.ftk_frags_format_rows_masked(engine.ctx, cid, b"c", 0, -1, -1, 0, C.byref(out), C.byref(n), C.byref(rows), C.byref(m)),
                   lib.ftk_frags_write_masked(engine.ctx, cid, b"c", 0, -1, -1, 0, path, 0, 1, 0, C.byref(res), C.byref(m)))
            del alive
            return rcs
        for why, pair in bad.items():
            assert all_three(RegionMask(pair, None, "midpoint")) == (L.FTK_ERR_INVALID,) * 3, why
            assert all_three(RegionMask(good, pair, "any")) == (L.FTK_ERR_INVALID,) * 3, why
        for policy in (2, 7, -1):  # (2 = FTK_POLICY_FETCH: not a mask policy)
            assert all_three(RegionMask(good, None, policy)) == (L.FTK_ERR_INVALID,) * 3, policy
        assert not os.path.exists(path.decode())
        assert lib.ftk_frags_mask_keep(engine.ctx, 987654, C.byref(engine._mask_struct(RegionMask(good))[0]), L.ptr(keep),
                                       C.byref(kept)) == L.FTK_ERR_NO_CONTIG
        with pytest.raises(L.FtkError) as ei:
            engine.mask_keep("mask:err", RegionMask(bad["unsorted"], None, "midpoint"))
        assert ei.value.code == L.FTK_ERR_INVALID and "sorted" in ei.value.message
        # and the good mask passes all three: rows [10,15) [20,25) [30,35) against [5,12) [40,50)
        assert all_three(RegionMask(good, None, "any")) == (0, 0, 0)
        assert keep.tolist() == [1, 0, 0] and kept.value == 1 and rows.value == 1 and res.n_rows == 1
        lib.ftk_buffer_free(out.value)
        for p in (res.linear, res.run_bin, res.run_beg, res.run_end):
            lib.ftk_buffer_free(p)
    finally:
        engine.release("mask:err")


# ---- 5. frag_filter end to end ---------------------------------------------------------------------------------------
def check_output(path, want_text, q):
    """The file's rows, its index against a scan, and AlignmentWrapper on it."""
    from finaletoolkit_amd import source
    from finaletoolkit_amd.io import AlignmentWrapper
    raw = open(path, "rb").read()
    assert raw[-28:] == EOF
    assert gzip.decompress(raw).decode() == want_text
    rows = F.parse_rows(want_text)
    names, refs = T.read_tbi(path + ".tbi")
    assert names == list(dict.fromkeys(r[0] for r in rows))
    if not rows:
        return
    source.close_all()
    aw = AlignmentWrapper(path, quality_threshold=q)
    try:
        for c in names:
            mine = [r for r in rows if r[0] == c]
            s = np.array([r[1] for r in mine])
            e = np.array([r[2] for r in mine])
            lo, hi = int(s.min()), int(e.max())
            regs = [(lo, hi), (0, lo), (0, lo + 1), (hi - 1, hi), (hi, hi + 10), (0, 1 << 29)]
            rng = np.random.default_rng(len(mine))
            for _ in range(12):
                a = int(rng.integers(max(lo - 500, 0), hi))
                regs.append((a, a + int(rng.integers(1, 3000))))
            for a, b in regs:
                want = sorted("\t".join(map(str, r)) for r in mine if r[1] < b and r[2] > a)
                assert sorted(T.tabix_query(path, refs, c, a, b)) == want, (c, a, b)
                if b > a:
                    got = [T.fmt_row(f.contig, f.start, f.stop, f.mapq, f.is_forward) for f in aw.fetch(c, a, b)]
                    assert sorted(got) == want, (c, a, b)
    finally:
        aw.close()


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    G = F.load_golden()
    d = tmp_path_factory.mktemp("filter_golden")
    synth_path = str(d / "synth.frag.gz")
    F.write_synth(synth_path, G["synth"]["recipe"])
    inputs = {"fixture": FRAG, "synth": synth_path}
    beds = {tag: {name: F.write_bed(d / f"{tag}.{name}.bed", iv) for name, iv in G[tag]["masks"].items()} for tag in G}
    return G, inputs, beds


@pytest.mark.parametrize("tag", ["fixture", "synth"])
def test_frag_filter_reproduces_every_golden_case(golden, tmp_path, tag):
    from finaletoolkit_amd import utils
    G, inputs, beds = golden
    g = G[tag]
    q = g["quality_threshold"]
    contigs = list(dict.fromkeys(r[0] for r in F.parse_rows(g["all_rows"])))
    assert len(g["cases"]) == 18
    for k, case in enumerate(g["cases"]):
        out = str(tmp_path / f"{tag}.{k}.frag.gz")
        written = utils.frag_filter(inputs[tag], out, whitelist_file=None if case["whitelist"] is None else beds[tag][case["whitelist"]],
                                    blacklist_file=None if case["blacklist"] is None else beds[tag][case["blacklist"]],
                                    intersect_policy=case["policy"], quality_threshold=q)
        per = {c: sum(1 for r in F.parse_rows(case["rows"]) if r[0] == c) for c in contigs}
        assert written == per, (tag, k)  # every contig of the input is visited, 0 rows included
        check_output(out, case["rows"], q)
    if tag == "synth":  # the set "messy" does not name the last contig: as a whitelist it leaves that contig empty
        assert any(c["whitelist"] == "messy" and not c["rows"].count(contigs[-1] + "\t") for c in g["cases"])


def test_frag_filter_from_the_bam_fixture(golden, tmp_path):
    """The BAM holds the fragment file's 17 fragments (its MAPQ column differs: the pair's own), so a mask keeps the
    same positions: bed3 rows are the golden's first three columns, frag rows are the unmasked export's rows at those
    positions."""
    from finaletoolkit_amd import utils
    G, inputs, beds = golden
    g = G["fixture"]
    plain = str(tmp_path / "plain.frag.gz")
    written = utils.frag_export(BAM, plain, quality_threshold=0)  # (every @SQ contig of the BAM is visited)
    assert written["12"] == 17 and sum(written.values()) == 17 and len(written) == 84
    plain_lines = gzip.open(plain, "rt").read().splitlines()
    all_lines = g["all_rows"].splitlines()
    assert [ln.split("\t")[:3] for ln in plain_lines] == [ln.split("\t")[:3] for ln in all_lines]
    for k, case in enumerate(g["cases"]):
        kw = dict(whitelist_file=None if case["whitelist"] is None else beds["fixture"][case["whitelist"]],
                  blacklist_file=None if case["blacklist"] is None else beds["fixture"][case["blacklist"]],
                  intersect_policy=case["policy"], quality_threshold=0)
        kept = set(case["rows"].splitlines())
        out3 = str(tmp_path / f"bam.{k}.bed3.gz")
        written = utils.frag_filter(BAM, out3, layout="bed3", **kw)
        assert written["12"] == case["n"] and sum(written.values()) == case["n"] and len(written) == 84
        assert gzip.open(out3, "rt").read() == "".join("\t".join(ln.split("\t")[:3]) + "\n" for ln in case["rows"].splitlines())
        out5 = str(tmp_path / f"bam.{k}.frag.gz")
        assert utils.frag_filter(BAM, out5, contig="12", **kw) == {"12": case["n"]}
        want = "".join(p + "\n" for p, a in zip(plain_lines, all_lines) if a in kept)
        check_output(out5, want, 0)


def test_a_whitelist_that_holds_nothing_gives_a_valid_empty_file(golden, tmp_path):
    from finaletoolkit_amd import utils
    G, inputs, beds = golden
    bed = F.write_bed(tmp_path / "elsewhere.bed", [("chrNotInTheInput", 0, 1 << 30)])
    for tag in ("fixture", "synth"):
        contigs = list(dict.fromkeys(r[0] for r in F.parse_rows(G[tag]["all_rows"])))
        out = str(tmp_path / f"{tag}.empty.frag.gz")
        assert utils.frag_filter(inputs[tag], out, whitelist_file=bed, quality_threshold=0) == {c: 0 for c in contigs}
        assert open(out, "rb").read() == EOF and gzip.open(out, "rb").read() == b""
        assert T.read_tbi(out + ".tbi") == ([], {})
    # a whitelist whose intervals lie where no fragment is: the contig is named, nothing is in it
    far = F.write_bed(tmp_path / "far.bed", [("12", 5, 1000)])
    out = str(tmp_path / "far.frag.gz")
    assert utils.frag_filter(FRAG, out, whitelist_file=far, intersect_policy="any", quality_threshold=0) == {"12": 0}
    assert open(out, "rb").read() == EOF and T.read_tbi(out + ".tbi") == ([], {})


def test_no_masks_is_frag_export_byte_for_byte_and_the_cli_writes_the_functions_bytes(golden, tmp_path):
    from finaletoolkit_amd import utils
    G, inputs, beds = golden
    for tag, src in (("fixture", FRAG), ("bam", BAM), ("synth", inputs["synth"])):
        a, b = str(tmp_path / f"{tag}.export.frag.gz"), str(tmp_path / f"{tag}.filter.frag.gz")
        kw = dict(quality_threshold=20, min_length=100, max_length=400, layout="bed6")
        assert utils.frag_export(src, a, **kw) == utils.frag_filter(src, b, **kw)
        assert open(a, "rb").read() == open(b, "rb").read() and len(gzip.open(a, "rb").read()) > 100
        assert open(a + ".tbi", "rb").read() == open(b + ".tbi", "rb").read()
    src = inputs["synth"]
    fn, cli = str(tmp_path / "fn.frag.gz"), str(tmp_path / "cli.frag.gz")
    written = utils.frag_filter(src, fn, whitelist_file=beds["synth"]["messy"], blacklist_file=beds["synth"]["edges"],
                                intersect_policy="any", quality_threshold=10, min_length=80, max_length=500, layout="frag")
    assert sum(written.values()) > 50
    r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.filter", src, cli, "--whitelist", beds["synth"]["messy"], "--blacklist",
                        beds["synth"]["edges"], "--intersect-policy", "any", "-q", "10", "--min-length", "80", "--max-length", "500",
                        "--layout", "frag"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert open(fn, "rb").read() == open(cli, "rb").read() and open(fn + ".tbi", "rb").read() == open(cli + ".tbi", "rb").read()
    want = F.parse_rows(G["synth"]["all_rows"])  # cross-check with the restatement at another MAPQ / length cut
    lines = [ln for ln in gzip.open(src, "rt").read().splitlines()]
    keep = []
    for ln in lines:
        c, s, e, q, _ = ln.split("\t")
        s, e = int(s), int(e)
        wl = [(a, b) for cc, a, b in G["synth"]["masks"]["messy"] if cc == c]
        bl = [(a, b) for cc, a, b in G["synth"]["masks"]["edges"] if cc == c]
        if int(q) >= 10 and 80 <= e - s <= 500 and F.in_mask("any", wl, s, e) and not F.in_mask("any", bl, s, e):
            keep.append(ln)
    assert gzip.open(fn, "rt").read() == "".join(ln + "\n" for ln in keep) and len(want) > len(keep)
