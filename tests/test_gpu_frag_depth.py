"""GPU: the per-base depth track (``csrc/ftk_depth.hip``) - ``Engine.depth`` and ``Engine.depth_runs`` against a numpy
restatement in ``tests/depth_helpers.py`` (``np.add.at`` of +1 / -1 at the clipped fragment bounds, ``cumsum``, runs from
``np.flatnonzero(np.diff(depth))``), exactly equal everywhere: at the tile sizes' edges, across tiles, above the
16-bit range, over more tiles than the scan workgroup is wide; the invariants of every run table; the C ABI's
argument errors; and ``frag_depth`` / ``frag_depth_track`` / the command line on the fixture files."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from tests.depth_helpers import check_invariants, kept, restated_depth, restated_runs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAG = os.path.join(ROOT, "tests", "data", "12.3444.b37.frag.gz")
BAM = os.path.join(ROOT, "tests", "data", "12.3444.b37.bam")
TILE = 4096
LENGTHS = (1, 4095, 4096, 4097, 8192, 3 * 4096 + 5)
R0 = 10_007  # the regions' start: no multiple of 4096 or of 16
assert R0 % 16 and R0 % TILE


# ---- the yardstick ---------------------------------------------------------------------------------------------------
def load(engine, name, s, e, q=None):
    s = np.asarray(s, np.int32)
    e = np.asarray(e, np.int32)
    q = np.full(len(s), 60, np.uint8) if q is None else np.asarray(q, np.uint8)
    o = np.argsort(s, kind="stable")
    s, e, q = s[o], e[o], q[o]
    engine.load_contig(name, s, e, q, np.zeros(len(s), np.uint8))
    return s, e, q


def check_region(engine, name, cols, start, stop, mapq_min=0, min_len=None, max_len=None):
    """Per-base depth and both run tables of one region against the restatement; returns the restated depth."""
    s, e, q = cols
    keep = kept(s, e, q, mapq_min, min_len, max_len)
    want = restated_depth(s, e, keep, start, stop)
    got = engine.depth(name, start, stop, mapq_min, min_len, max_len)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want)
    for include_zero in (False, True):
        runs = engine.depth_runs(name, start, stop, mapq_min, min_len, max_len, include_zero)
        exp = restated_runs(want, start, include_zero)
        assert all(a.dtype == np.int32 for a in runs)
        for g, w in zip(runs, exp):
            assert np.array_equal(g, w)
        check_invariants(runs, start, stop, include_zero, s, e, keep)
    return want


# ---- 1. fragment sets x region lengths -------------------------------------------------------------------------------
def fragment_set(kind):
    rng = np.random.default_rng(11)
    stops = [R0 + n for n in LENGTHS]
    s, e = [], []
    if kind == "random":
        a = rng.integers(0, 40_000, 6000)
        s += a.tolist()
        e += (a + rng.integers(20, 601, 6000)).tolist()
        for k in range(1, 40):  # start before the region, end inside it
            s.append(R0 - 13 * k)
            e.append(R0 + 7 * k)
    if kind == "span":  # start before, end behind every region: each region is one run
        s += [R0 - 500, R0 - 1, 0]
        e += [stops[-1] + 700, stops[-1] + 1, stops[-1] + 4096]
    if kind == "dups":  # 70 000 copies inside one tile: depth above 65 535, candidates above 32 768
        s += [R0 + 100] * 70_000 + [R0 + 90, R0 + 250]
        e += [R0 + 300] * 70_000 + [R0 + 120, R0 + 5000]
    for k in range(4):  # touching the region from outside: they contribute nothing
        s.append(R0 - 40 - k)
        e.append(R0)
    for b in stops if kind != "span" else ():  # starting exactly at a region's stop (and inside the longer regions)
        s += [b, b]
        e += [b + 30, b + 1]
    for p in (0, R0 - 1, R0, R0 + 1, R0 + 2000, *stops, stops[-1] - 1):  # zero-length fragments
        s.append(p)
        e.append(p)
    return s, e


@pytest.fixture(scope="module")
def sets(engine):
    out = {}
    for kind in ("random", "span", "dups"):
        s, e = fragment_set(kind)
        out[kind] = load(engine, "depth:" + kind, s, e)
    yield out
    for kind in out:
        engine.release("depth:" + kind)


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("kind", ["random", "span", "dups"])
def test_depth_and_runs_equal_the_restatement(engine, sets, kind, length):
    cols = sets[kind]
    want = check_region(engine, "depth:" + kind, cols, R0, R0 + length)
    if kind == "span":
        rs, re_, rd = engine.depth_runs("depth:span", R0, R0 + length)
        assert (rs.tolist(), re_.tolist(), rd.tolist()) == ([R0], [R0 + length], [3])
    if kind == "dups" and length > 300:
        assert want.max() > 65_535
        assert int(((cols[0] < R0 + TILE) & (cols[1] >= R0)).sum()) > 32_768  # one tile's candidates
    if kind == "random":
        assert want.max() < 32_768 and (length < 4000 or len(np.unique(want)) > 10)


def test_region_from_zero_and_unaligned_device_output(engine, sets):
    """Other starts (0: no fragment in front of the region; one in the middle of the data), and outputs on the device
    at an address that is and is not a multiple of 16."""
    import torch
    cols = sets["random"]
    check_region(engine, "depth:random", cols, 0, 2 * TILE + 1)
    start, stop = 20_001, 20_001 + 2 * TILE + 7
    want = check_region(engine, "depth:random", cols, start, stop)
    buf = torch.full((len(want) + 4,), -7, dtype=torch.int32, device="cuda:0")
    for shift in (0, 1, 3):
        buf.fill_(-7)
        torch.cuda.synchronize()
        out = buf[shift:shift + len(want)]
        assert (out.data_ptr() % 16 == 0) == (shift == 0)
        engine.depth("depth:random", start, stop, 0, out=out)
        engine.sync()
        host = buf.cpu().numpy()
        assert np.array_equal(host[shift:shift + len(want)], want)
        assert np.all(host[:shift] == -7) and np.all(host[shift + len(want):] == -7)  # nothing written around it


# ---- 2. runs across tiles ------------------------------------------------------------------------------------------
def runs_of(engine, name, start, stop, include_zero):
    return [a.tolist() for a in engine.depth_runs(name, start, stop, 0, None, None, include_zero)]


@pytest.mark.parametrize("start", [0, 7])
def test_runs_across_tiles(engine, start):
    stop = start + 3 * TILE + 100
    name = "depth:hand"
    # one fragment over three tile boundaries: one run where it opens, none where it merely continues
    cols = load(engine, name, [start + 100], [start + 3 * TILE + 50])
    check_region(engine, name, cols, start, stop)
    assert runs_of(engine, name, start, stop, False) == [[start + 100], [start + 3 * TILE + 50], [1]]
    assert runs_of(engine, name, start, stop, True) == [[start, start + 100, start + 3 * TILE + 50],
                                                        [start + 100, start + 3 * TILE + 50, stop], [0, 1, 0]]
    # two fragments that abut: one run; with a one-base gap: two (three with the zero run)
    for at in (500, TILE, TILE + 1, 2 * TILE - 1):  # inside a tile, on its first base, behind it, on its last base
        cols = load(engine, name, [start + 40, start + at], [start + at, start + at + 300])
        check_region(engine, name, cols, start, stop)
        assert runs_of(engine, name, start, stop, False) == [[start + 40], [start + at + 300], [1]]
        cols = load(engine, name, [start + 40, start + at + 1], [start + at, start + at + 300])
        check_region(engine, name, cols, start, stop)
        assert runs_of(engine, name, start, stop, False) == [[start + 40, start + at + 1], [start + at, start + at + 300], [1, 1]]
        assert runs_of(engine, name, start, stop, True)[2] == [0, 1, 0, 1, 0]
    # a change of depth exactly at a tile's first base and exactly at its last base, by an end and by a start
    cols = load(engine, name, [start + 10, start + TILE + 50, start + 2 * TILE, start + 3 * TILE - 1],
                [start + TILE, start + 2 * TILE - 1, start + 2 * TILE + 9, start + 3 * TILE + 4])
    check_region(engine, name, cols, start, stop)
    assert {start + 2 * TILE, start + 3 * TILE - 1} <= set(runs_of(engine, name, start, stop, False)[0])
    zero = [a for a, d in zip(*runs_of(engine, name, start, stop, True)[::2]) if d == 0]
    assert {start + TILE, start + 2 * TILE - 1} <= set(zero)
    # a fragment that ends where another starts, on a tile's first base: the depth does not change there
    cols = load(engine, name, [start + 10, start + TILE], [start + TILE, start + TILE + 20])
    check_region(engine, name, cols, start, stop)
    assert runs_of(engine, name, start, stop, False) == [[start + 10], [start + TILE + 20], [1]]
    # the same rows seen through a region that starts and stops inside them
    check_region(engine, name, cols, start + 20, start + 2 * TILE + 2)
    check_region(engine, name, cols, start + TILE, start + 2 * TILE)
    engine.release(name)


def test_empty_contig_and_empty_region(engine, sets):
    name = "depth:empty"
    cols = load(engine, name, [], [])
    want = check_region(engine, name, cols, 0, TILE + 9)
    assert not want.any()
    assert runs_of(engine, name, 0, TILE + 9, False) == [[], [], []]
    assert runs_of(engine, name, 5, TILE + 9, True) == [[5], [TILE + 9], [0]]
    engine.release(name)
    for start in (0, R0):
        assert len(engine.depth("depth:random", start, start)) == 0
        assert runs_of(engine, "depth:random", start, start, True) == [[], [], []]


@pytest.mark.parametrize("n_frag", [2, 300])
def test_more_tiles_than_the_scan_is_wide(engine, n_frag):
    """1 025 tiles: the scan of the tiles' run counts (1 024 per trip) takes two trips; the runs stay few."""
    size = 1024 * TILE + 1
    rng = np.random.default_rng(n_frag)
    if n_frag == 2:  # one run in the first tile, one on the contig's last base: the zero run between them spans both trips
        s, e = [17, size - 1], [900, size]
    else:
        a = rng.integers(0, size - 700, n_frag - 2)
        s = a.tolist() + [1023 * TILE + 4000, size - 40]
        e = (a + rng.integers(20, 601, n_frag - 2)).tolist() + [1024 * TILE + 1, size]  # (one fragment crosses the trips' seam)
    name = "depth:sparse"
    cols = load(engine, name, s, e)
    want = check_region(engine, name, cols, 0, size)
    assert want[-1] >= 1 and len(runs_of(engine, name, 0, size, True)[0]) <= 4 * n_frag + 1
    check_region(engine, name, cols, 3, size - 1)
    engine.release(name)


# ---- 3. filters --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapq_min, min_len, max_len", [(30, None, None), (0, 150, None), (0, None, 200), (20, 120, 180),
                                                        (0, None, None), (61, None, None), (0, 0, 0), (0, 601, None)])
def test_filters(engine, mapq_min, min_len, max_len):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 30_000, 5000)
    ln = rng.integers(20, 601, 5000)
    ln[:50] = 0
    q = rng.integers(0, 61, 5000)
    name = "depth:filters"
    cols = load(engine, name, a, a + ln, q)
    want = check_region(engine, name, cols, R0, R0 + 2 * TILE + 5, mapq_min, min_len, max_len)
    n_keep = int(kept(*cols, mapq_min, min_len, max_len).sum())
    assert (n_keep == 0 or (min_len, max_len) == (0, 0)) == (not want.any())
    if mapq_min == 0 and min_len is None and max_len is None:
        assert n_keep == 5000
    elif (min_len, max_len) != (0, 0) and 0 < n_keep:
        assert n_keep < 5000
    engine.release(name)


# ---- 4. the C ABI's argument errors ------------------------------------------------------------------------------------
def test_argument_errors(engine, sets):
    from finaletoolkit_amd import _lib as L
    lib = engine.lib
    cid = engine.contig_id("depth:random")
    out = np.full(64, -1, np.int32)
    ptrs = [C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)]
    n = C.c_int64(-1)
    by = [C.byref(p) for p in ptrs]

    def depth(ctx, contig, start, stop, dst):
        return lib.ftk_depth(ctx, contig, start, stop, L.LEN_OPEN, L.LEN_OPEN, 0, dst)

    def runs(ctx, contig, start, stop, a=by[0], b=by[1], c=by[2], count=C.byref(n)):
        return lib.ftk_depth_runs(ctx, contig, start, stop, L.LEN_OPEN, L.LEN_OPEN, 0, 0, a, b, c, count)

    assert depth(None, cid, 0, 64, L.ptr(out)) == L.FTK_ERR_INVALID
    assert depth(engine.ctx, cid, 0, 64, None) == L.FTK_ERR_INVALID
    assert runs(None, cid, 0, 64) == L.FTK_ERR_INVALID
    for k in range(4):
        args = [by[0], by[1], by[2], C.byref(n)]
        args[k] = None
        assert runs(engine.ctx, cid, 0, 64, *args) == L.FTK_ERR_INVALID
    for start, stop in ((-1, 64), (64, 63), (0, 1 << 30), (0, (1 << 30) + 5), (1 << 31, 1 << 32)):
        assert depth(engine.ctx, cid, start, stop, L.ptr(out)) == L.FTK_ERR_INVALID
        assert lib.ftk_last_error(engine.ctx)
        assert runs(engine.ctx, cid, start, stop) == L.FTK_ERR_INVALID
        assert n.value == 0 and all(p.value is None for p in ptrs)
    assert depth(engine.ctx, 987_654, 0, 64, L.ptr(out)) == L.FTK_ERR_NO_CONTIG  # the code of every call for an unknown contig
    assert runs(engine.ctx, 987_654, 0, 64) == L.FTK_ERR_NO_CONTIG
    assert np.all(out == -1)
    # start == stop is valid: no values, no runs
    assert depth(engine.ctx, cid, 9, 9, L.ptr(out)) == L.FTK_OK and np.all(out == -1)
    n.value = -1
    assert runs(engine.ctx, cid, 9, 9) == L.FTK_OK and n.value == 0 and all(p.value is None for p in ptrs)
    # the largest stop there is
    assert depth(engine.ctx, cid, (1 << 30) - 65, (1 << 30) - 1, L.ptr(out)) == L.FTK_OK and not out.any()


# ---- 5. the product path -----------------------------------------------------------------------------------------------
def fixture_columns():
    rows = [ln.split("\t") for ln in gzip.open(FRAG, "rt").read().splitlines()]
    assert {r[0] for r in rows} == {"12"}
    return (np.array([int(r[1]) for r in rows], np.int32), np.array([int(r[2]) for r in rows], np.int32),
            np.array([int(r[3]) for r in rows], np.uint8))


def restated_track(contig, s, e, keep, include_zero=False, length=None):
    """The text of a contig's track over [0, length) - ``length=None``: a fragment file, which spans up to its largest
    fragment end and knows no length to give a contig without kept fragments a row.  The restatement runs over
    [lo, hi), the span of the kept fragments; the depth is 0 on every base outside it, so with ``include_zero`` the
    rows in front of and behind it are added here."""
    if not keep.any():
        return (f"{contig}\t0\t{length}\t0\n", 1) if include_zero and length else ("", 0)
    length = int(e.max()) if length is None else length
    lo, hi = int(s[keep].min()), min(int(e[keep].max()), length)
    rs, re_, rd = (a.tolist() for a in restated_runs(restated_depth(s, e, keep, lo, hi), lo, include_zero))
    if include_zero and lo > 0:
        rs, re_, rd = [0] + rs, [lo] + re_, [0] + rd
    if include_zero and hi < length:
        rs, re_, rd = rs + [hi], re_ + [length], rd + [0]
    return "".join(f"{contig}\t{a}\t{b}\t{d}\n" for a, b, d in zip(rs, re_, rd)), len(rs)


@pytest.mark.parametrize("suffix", [".bedgraph", ".bg", ".bedgraph.gz", ".bg.gz"])
@pytest.mark.parametrize("q, include_zero", [(0, False), (30, False), (30, True), (61, True)])
def test_track_of_the_fragment_file(tmp_path, suffix, q, include_zero):
    from finaletoolkit_amd import utils
    s, e, mq = fixture_columns()
    keep = kept(s, e, mq, q)
    want, n_rows = restated_track("12", s, e, keep, include_zero)
    out = str(tmp_path / ("track" + suffix))
    res = utils.frag_depth_track(FRAG, out, quality_threshold=q, include_zero=include_zero)
    raw = open(out, "rb").read()
    assert (raw[:2] == b"\x1f\x8b") == suffix.endswith(".gz")
    text = gzip.open(out, "rt").read() if suffix.endswith(".gz") else raw.decode()
    assert text == want
    depth = restated_depth(s, e, keep, int(s.min()), int(e.max()))
    assert res == dict(n_runs=n_rows, n_fragments=int(keep.sum()), bases_covered=int((depth > 0).sum()),
                       max_depth=int(depth.max()))
    if q == 61:
        assert want == "" and res["n_runs"] == 0  # nothing kept, and a fragment file knows no contig length


def test_track_options_and_command_line(tmp_path):
    from finaletoolkit_amd import depth as cli
    from finaletoolkit_amd import utils
    s, e, mq = fixture_columns()
    out = str(tmp_path / "cli.bedgraph")
    assert cli.main([FRAG, out, "-q", "0"]) == 0
    assert open(out).read() == restated_track("12", s, e, kept(s, e, mq, 0))[0]
    assert cli.main([FRAG, out, "-c", "12", "--min-length", "160", "--max-length", "170", "--include-zero", "-w", "2"]) == 0
    assert open(out).read() == restated_track("12", s, e, kept(s, e, mq, 30, 160, 170), True)[0]
    with pytest.raises(ValueError, match="contig not present"):
        utils.frag_depth_track(FRAG, out, contig="13")


def test_frag_depth_on_an_interval():
    from finaletoolkit_amd import utils
    s, e, mq = fixture_columns()
    for q, lo, hi in ((30, 34_443_000, 34_447_000), (0, 34_443_200, 34_443_201), (30, 34_444_000, 34_444_000)):
        got = utils.frag_depth(FRAG, "12", lo, hi, quality_threshold=q)
        assert got.dtype == np.int32 and np.array_equal(got, restated_depth(s, e, kept(s, e, mq, q), lo, hi))
        bam = utils.frag_depth(BAM, "12", lo, hi, quality_threshold=q)
        fa = utils.frag_array(BAM, "12", quality_threshold=q, intersect_policy="any")
        assert np.array_equal(bam, restated_depth(fa["start"], fa["stop"], np.ones(len(fa), bool), lo, hi))
    whole = utils.frag_depth(FRAG, "12", quality_threshold=0)  # stop: the largest fragment end
    assert len(whole) == int(e.max()) and np.array_equal(whole[int(s.min()):], restated_depth(s, e, kept(s, e, mq), int(s.min()), int(e.max())))
    assert not whole[:int(s.min())].any()
    with pytest.raises(ValueError):
        utils.frag_depth(FRAG, "12", 10, 5)


def test_bam_track_against_its_own_fragments(tmp_path):
    """BAM and fragment file give one track at MAPQ 0 when ``frag_array`` of the two agrees there; either way each
    track is the restatement over its own file's ``frag_array``."""
    from finaletoolkit_amd import utils
    texts, arrays = {}, {}
    for tag, path in (("bam", BAM), ("frag", FRAG)):
        out = str(tmp_path / (tag + ".bg"))
        res = utils.frag_depth_track(path, out, quality_threshold=0)
        fa = utils.frag_array(path, "12", quality_threshold=0, intersect_policy="any")
        fa = fa[np.argsort(fa["start"], kind="stable")]
        want, n_rows = restated_track("12", fa["start"], fa["stop"], np.ones(len(fa), bool))
        texts[tag] = open(out).read()
        arrays[tag] = fa
        assert texts[tag] == want and res["n_runs"] == n_rows and res["n_fragments"] == len(fa) > 0
    same = len(arrays["bam"]) == len(arrays["frag"]) and all(
        np.array_equal(np.sort(arrays["bam"][k]), np.sort(arrays["frag"][k])) for k in ("start", "stop"))
    if same:
        assert texts["bam"] == texts["frag"]
    # with include_zero every contig of the BAM header has rows, in header order; its length closes each
    from finaletoolkit_amd.source import open_source
    out = str(tmp_path / "bam_zero.bedgraph")
    res = utils.frag_depth_track(BAM, out, quality_threshold=0, include_zero=True)
    src = open_source(BAM)
    fa = arrays["bam"]
    assert len(src.contigs) == 84 and src.contigs.index("12") == 11
    want = "".join(restated_track("12", fa["start"], fa["stop"], np.ones(len(fa), bool), True, src.lengths[c])[0] if c == "12"
                   else f"{c}\t0\t{src.lengths[c]}\t0\n" for c in src.contigs)
    assert open(out).read() == want and res["n_runs"] == want.count("\n")
    one = str(tmp_path / "bam_one.bg")
    utils.frag_depth_track(BAM, one, contig="12", quality_threshold=0, include_zero=True)
    assert open(one).read() == restated_track("12", fa["start"], fa["stop"], np.ones(len(fa), bool), True, src.lengths["12"])[0]
