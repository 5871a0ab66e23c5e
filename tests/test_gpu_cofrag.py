"""GPU: the co-fragmentation calls (``csrc/ftk_cofrag.hip``) - ``Engine.hist_ks`` and ``Engine.cofrag`` against the numpy
restatement of ``tests/cofrag_helpers.py``, exactly equal, in both arrangements of the pair kernel: at every size around
the pair tile and the LDS chunk (``ftk_hist_ks_shape``), on rows that stress the rule (empty and identical rows, disjoint
supports, a maximum attained several times, a maximum in the last cell of a partial chunk that can hold one), at the 2^31 edge of the
width, with host and device outputs, on a poisoned scratch; ``ftk_cofrag`` against ``hist_ks(fraglen_hist(...))`` on a
tabix-style and a BAM-style contig; the C ABI's argument errors; ``frag_cofragmentation`` and its command line on the
repository's fragment file."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from finaletoolkit_amd import _lib as L
from tests import cofrag_helpers as H
from tests import cofrag_poison_calls as PC  # (adds the two calls to the scratch-poison table at import)
from tests.helpers import read_frag_gz

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "data")
ARRANGEMENTS = ("0", "1")


@pytest.fixture(params=ARRANGEMENTS)
def arrangement(request):
    """FTK_COFRAG_ARRANGE for the test's calls (the library reads it at every call), put back afterwards."""
    before = os.environ.get("FTK_COFRAG_ARRANGE")
    os.environ["FTK_COFRAG_ARRANGE"] = request.param
    yield request.param
    if before is None:
        del os.environ["FTK_COFRAG_ARRANGE"]
    else:
        os.environ["FTK_COFRAG_ARRANGE"] = before


@pytest.fixture(scope="module")
def shape(engine):
    t, chunk = engine.hist_ks_shape()
    assert t >= 4 and chunk >= 4
    return t, chunk


_wanted = {}


def wanted(key, make):
    """A case's histogram and its restatement, computed once and shared by the arrangements."""
    if key not in _wanted:
        hist = make()
        _wanted[key] = (hist, H.ks_matrix(hist))
    return _wanted[key]


def same(got, want):
    K, at, n = got
    wK, wat, wn = want
    assert K.dtype == np.int64 and n.dtype == np.int64
    assert np.array_equal(n, wn)
    assert np.array_equal(K, wK), np.argwhere(K != wK)[:5]
    if at is not None:
        assert at.dtype == np.int32 and np.array_equal(at, wat), np.argwhere(at != wat)[:5]


# ---- 1. sizes around the tile and the chunk -----------------------------------------------------------------------------
@pytest.mark.parametrize("bins_case", range(6))
@pytest.mark.parametrize("rows_case", range(6))
def test_sizes_around_tile_and_chunk(engine, shape, arrangement, rows_case, bins_case):
    t, chunk = shape
    n_rows = (1, 2, t - 1, t, t + 1, 2 * t + 1)[rows_case]
    n_bins = (1, 2, chunk - 1, chunk, chunk + 1, 2 * chunk + 1)[bins_case]
    hist, want = wanted(("size", n_rows, n_bins), lambda: H.random_hist(np.random.default_rng(1000 * n_rows + n_bins), n_rows, n_bins))
    got = engine.hist_ks(hist)
    same(got, want)
    K = got[0]
    assert np.array_equal(K, K.T) and not np.diag(K).any()


# ---- 2. rows that stress the rule ---------------------------------------------------------------------------------------
def stress_rows(t, chunk):
    rng = np.random.default_rng(99)
    n_rows, n_bins = t + 9, 2 * chunk + 5  # two tiles a side, a partial last chunk
    hist = H.random_hist(rng, n_rows, n_bins)
    hist[[0, 3, t, n_rows - 1]] = 0                    # empty rows among the others
    hist[5] = hist[4]                                  # identical rows, in one tile and across tiles
    hist[t + 2] = hist[4]
    hist[6] = 0                                        # disjoint supports
    hist[6, :3] = (4, 0, 9)
    hist[7] = 0
    hist[7, chunk + 1:chunk + 4] = (2, 5, 1)
    # the maximum attained at several lengths: |C(8) n(9) - C(9) n(8)| is flat over a run inside the first chunk ...
    hist[8] = 0
    hist[8, 2] = 6
    hist[9] = 0
    hist[9, chunk - 1] = 6
    # ... and over a run that starts in a later chunk and crosses into the last one
    hist[10] = 0
    hist[10, chunk + 3] = 7
    hist[11] = 0
    hist[11, n_bins - 2] = 3
    # a maximum in the last cell of the last, partial chunk that can hold one (at the very last length every difference is
    # 0): the rows differ only by their last two cells
    hist[12] = 1
    hist[13] = 1
    hist[12, n_bins - 2:] = (0, 9)
    hist[13, n_bins - 2:] = (9, 0)
    hist[t + 3] = hist[12]
    hist[t + 4] = hist[13]
    return hist


def test_rows_that_stress_the_rule(engine, shape, arrangement):
    t, chunk = shape
    hist, want = wanted(("stress",), lambda: stress_rows(t, chunk))
    wK, wat, wn = want
    n_bins = hist.shape[1]
    # what the cases are there for, on the restatement
    assert wn[0] == 0 and not wK[0].any() and not wat[0].any()
    assert wK[4, 5] == 0 and wat[4, 5] == 0 and wK[4, t + 2] == 0 and wat[5, t + 2] == 0
    assert wK[6, 7] == wn[6] * wn[7] and wat[6, 7] == 2
    assert wK[8, 9] == 36 and wat[8, 9] == 2
    assert wK[10, 11] == 21 and wat[10, 11] == chunk + 3
    assert wat[12, 13] == n_bins - 2 and wat[12, t + 4] == n_bins - 2 and wat[13, t + 3] == n_bins - 2
    same(engine.hist_ks(hist), want)


def test_maximum_in_the_last_cell(engine, shape, arrangement):
    """The latest a maximum can stand: at the last length every C(i, l) is n(i) and the difference is 0 for every pair, so
    the last cell that can hold a maximum is the one before it - here the FIRST cell of a last chunk of two lengths."""
    t, chunk = shape
    n_bins = 2 * chunk + 2

    def make():
        hist = np.ones((t + 2, n_bins), np.uint32)
        hist[0] = 0
        hist[0, n_bins - 1] = 3  # nothing before the last cell: against a flat row the gap grows up to the last cell but one
        hist[t] = hist[0]
        hist[2] = 0
        hist[2, 0] = 3           # everything in the first cell: against a flat row the gap is largest at once
        return hist
    hist, want = wanted(("last",), make)
    wK, wat, wn = want
    assert wat[0, 1] == n_bins - 2 and wat[1, t] == n_bins - 2 and wat[0, 2] == 0 and wat[2, 1] == 0 and wat.max() == n_bins - 2
    assert wK[0, 1] == 3 * (n_bins - 1) and wK[0, 2] == 9
    same(engine.hist_ks(hist), want)


# ---- 3. width -----------------------------------------------------------------------------------------------------------
def test_largest_row_sums(engine, arrangement):
    top = (1 << 31) - 1
    hist = np.zeros((3, 70), np.uint32)
    hist[0, 3] = top
    hist[1, 66] = top
    hist[2, 10:20] = top // 10
    K, at, n = engine.hist_ks(hist)
    assert K[0, 1] == top * top and K[1, 0] == top * top and at[0, 1] == 3 and n.tolist() == [top, top, top // 10 * 10]
    Kl, atl, nl = H.ks_matrix_loop(hist)
    assert K.tolist() == Kl and at.tolist() == atl and n.tolist() == nl


@pytest.mark.parametrize("device", [False, True])
def test_row_sum_of_2_31_is_refused_and_writes_nothing(engine, arrangement, device):
    import torch
    hist = H.random_hist(np.random.default_rng(5), 70, 40)
    for bad, cells in ((66, {7: (1 << 32) - 1}), (3, {0: 1 << 30, 39: 1 << 30}), (69, {5: 1 << 31})):
        h = hist.copy()
        h[bad] = 0
        for l, v in cells.items():
            h[bad, l] = v
        h[69 if bad != 69 else 68, :] = 0
        h[69 if bad != 69 else 68, 1] = (1 << 31) - 1  # the largest sum that is allowed, beside it
        if bad < 69:
            h[69, 2] = 1                                # ... and a later row over the limit: the FIRST is named
        if device:
            outs = [torch.full((70 * 70,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda"),
                    torch.full((70 * 70,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"),
                    torch.full((70,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")]
            torch.cuda.synchronize()
        else:
            outs = [np.full(70 * 70, 0x5A5A5A5A5A5A5A5A, np.int64), np.full(70 * 70, 0x5A5A5A5A, np.int32),
                    np.full(70, 0x5A5A5A5A5A5A5A5A, np.int64)]
        rc = engine.lib.ftk_hist_ks(engine.ctx, L.ptr(h), 70, 40, *[L.ptr(o) for o in outs])
        assert rc == L.FTK_ERR_INVALID
        assert f"row {bad} " in engine.lib.ftk_last_error(engine.ctx).decode()
        engine.sync()
        for o, fill in zip(outs, (0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A)):
            o = o.cpu().numpy() if device else o
            assert (o == fill).all()
    with pytest.raises(L.FtkError, match="row 69"):
        engine.hist_ks(h)


# ---- 4. outputs ---------------------------------------------------------------------------------------------------------
def test_host_and_device_outputs_and_inputs(engine, shape, arrangement):
    import torch
    t, chunk = shape
    n_rows, n_bins = t + 5, chunk + 7
    hist, want = wanted(("outputs", n_rows, n_bins), lambda: H.random_hist(np.random.default_rng(8), n_rows, n_bins))
    host = engine.hist_ks(hist)
    same(host, want)
    d_k = torch.full((n_rows, n_rows), -1, dtype=torch.int64, device="cuda")
    d_at = torch.full((n_rows, n_rows), -1, dtype=torch.int32, device="cuda")
    d_n = torch.full((n_rows,), -1, dtype=torch.int64, device="cuda")
    d_hist = torch.from_numpy(hist.view(np.int32)).cuda()
    torch.cuda.synchronize()
    assert engine.lib.ftk_hist_ks(engine.ctx, L.ptr(d_hist), n_rows, n_bins, L.ptr(d_k), L.ptr(d_at), L.ptr(d_n)) == L.FTK_OK
    engine.sync()
    assert d_k.cpu().numpy().tobytes() == host[0].tobytes() and d_at.cpu().numpy().tobytes() == host[1].tobytes()
    assert d_n.cpu().numpy().tobytes() == host[2].tobytes()
    # the engine's own forms: a device histogram, K into a tensor, no `at`
    out = torch.full((n_rows, n_rows), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    K, at, n = engine.hist_ks(d_hist.view(n_rows, n_bins), out=out, at=False)
    engine.sync()
    assert K is out and at is None and np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(n, want[2])
    K, at, n = engine.hist_ks(hist, at=False)
    assert at is None
    same((K, None, n), want)


def test_answers_do_not_depend_on_the_scratch(engine, shape, arrangement):
    t, chunk = shape
    hist, want = wanted(("poison",), lambda: H.random_hist(np.random.default_rng(9), 2 * t + 3, chunk + 3))
    same(engine.hist_ks(hist), want)
    for byte in (0xA5, 0xFF, 0x00):
        engine.scratch_fill(byte)
        same(engine.hist_ks(hist), want)


# ---- 5. ftk_cofrag ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def contigs(engine):
    rng = np.random.default_rng(77)
    n = 30_000
    s = np.sort(rng.integers(0, 1_000_000, n)).astype(np.int32)
    e = (s + rng.integers(20, 420, n)).astype(np.int32)
    q = rng.integers(0, 61, n).astype(np.uint8)
    st = rng.integers(0, 2, n).astype(np.uint8)
    r1s = np.where(st == 1, s, np.maximum(e - 60, s)).astype(np.int32)
    r1e = np.where(st == 1, np.minimum(s + 60, e), e).astype(np.int32)
    engine.load_contig("cf:tabix", s, e, q, st)
    engine.load_contig("cf:bam", s, e, q, st, r1s, r1e)
    engine.load_contig("cf:empty", np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    ws = np.arange(0, 1_000_000, 9_100, dtype=np.int64)  # 110 windows, the last one partial and two of them emptied below
    we = np.minimum(ws + 9_100, 1_000_000)
    we[7] = ws[7]
    yield dict(ws=ws, we=we)
    for name in ("cf:tabix", "cf:bam", "cf:empty"):
        engine.release(name)


@pytest.mark.parametrize("name", ["cf:tabix", "cf:bam"])
@pytest.mark.parametrize("len_lo,n_bins,min_length,max_length", [(0, 512, None, None), (100, 97, None, None), (150, 40, 120, 300)])
def test_cofrag_equals_hist_ks_of_fraglen_hist(engine, contigs, arrangement, name, len_lo, n_bins, min_length, max_length):
    ws, we = contigs["ws"], contigs["we"]
    key = ("cofrag", name, len_lo, n_bins, min_length, max_length)
    if key not in _wanted:
        hist, over = engine.fraglen_hist(name, ws, we, len_lo, n_bins, 30, min_length, max_length)
        _wanted[key] = (hist, over, H.ks_matrix(hist))
    hist, over, want = _wanted[key]
    K, at, n, overflow = engine.cofrag(name, ws, we, len_lo, n_bins, 30, min_length, max_length)
    same((K, at, n), want)
    assert np.array_equal(overflow, over) and overflow.dtype == np.int64
    assert n[7] == 0 and (np.delete(n, 7) > 0).all()
    if len_lo:
        assert over.any()  # lengths outside the range went to the overflow column and took no part
    same(engine.hist_ks(hist), want)


def test_cofrag_small_cases(engine, contigs, arrangement):
    import torch
    one = engine.cofrag("cf:tabix", [0], [500_000], 50, 300)
    hist, over = engine.fraglen_hist("cf:tabix", [0], [500_000], 50, 300)
    assert one[0].tolist() == [[0]] and one[1].tolist() == [[0]] and one[2].tolist() == [int(hist.sum())] and np.array_equal(one[3], over)
    K, at, n, over = engine.cofrag("cf:empty", contigs["ws"][:9], contigs["we"][:9], 0, 64)
    assert not K.any() and not at.any() and not n.any() and not over.any() and K.shape == (9, 9)
    K, at, n, over = engine.cofrag("cf:empty", [0], [1000], 0, 1)
    assert K.tolist() == [[0]] and n.tolist() == [0]
    # device outputs, no `at`
    ws, we = contigs["ws"], contigs["we"]
    want = engine.cofrag("cf:bam", ws, we, 60, 200)
    out = torch.full((len(ws), len(ws)), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    K, at, n, over = engine.cofrag("cf:bam", ws, we, 60, 200, out=out, at=False)
    engine.sync()
    assert at is None and np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(n, want[2]) and np.array_equal(over, want[3])
    engine.scratch_fill(0xA5)
    again = engine.cofrag("cf:bam", ws, we, 60, 200)
    assert all(np.array_equal(a, b) for a, b in zip(again, want))


def test_poison_table_holds_the_new_calls(request):
    """``tests/cofrag_poison_calls.py`` has put both calls into the table of ``tests/scratch_poison_calls.py``, and where
    this session holds ``tests/test_gpu_scratch_poison.py`` that module's parametrised test has a case for each."""
    from tests import scratch_poison_calls as P
    for name, entry in PC.ENTRIES.items():
        assert P.CALLS[name] is entry and set(name.split("+")) <= set(L.EXPORTS)
    cases = [it.name for it in request.session.items if it.nodeid.startswith("tests/test_gpu_scratch_poison.py::")]
    if cases:
        for name in PC.ENTRIES:
            assert f"test_same_answer_on_a_poisoned_scratch[{name}]" in cases, name


# ---- 6. the C ABI's argument errors -------------------------------------------------------------------------------------
def test_argument_errors(engine, contigs):
    lib, ctx = engine.lib, engine.ctx
    INV, NOC = L.FTK_ERR_INVALID, L.FTK_ERR_NO_CONTIG
    hist = np.ones((4, 8), np.uint32)
    k, at, n, over = np.full(16, 7, np.int64), np.full(16, 7, np.int32), np.full(4, 7, np.int64), np.full(4, 7, np.int64)
    ws, we = np.array([0, 100, 200, 300], np.int32), np.array([100, 200, 300, 400], np.int32)
    f = engine._filter("cf:tabix", 30, None, None, "midpoint")
    cid = engine.contig_id("cf:tabix")

    def ks(ctx_=ctx, h=hist, rows=4, bins=8, k_=k, at_=at, n_=n):
        return lib.ftk_hist_ks(ctx_, L.ptr(h), rows, bins, L.ptr(k_), L.ptr(at_), L.ptr(n_))

    def co(ctx_=ctx, cid_=cid, ws_=ws, we_=we, rows=4, f_=f, bins=8, k_=k, n_=n, over_=over):
        return lib.ftk_cofrag(ctx_, cid_, L.ptr(ws_), L.ptr(we_), rows, None if f_ is None else C.byref(f_), 0, bins, L.ptr(k_), L.ptr(at),
                              L.ptr(n_), L.ptr(over_))

    def failed(rc, code):
        assert rc == code, (rc, code)
        assert lib.ftk_last_error(ctx)

    assert ks() == L.FTK_OK and co() == L.FTK_OK and ks(at_=None) == L.FTK_OK
    k[:], at[:], n[:], over[:] = 7, 7, 7, 7
    assert ks(ctx_=None) == INV and co(ctx_=None) == INV
    for kw in (dict(h=None), dict(k_=None), dict(n_=None)):
        failed(ks(**kw), INV)
    for kw in (dict(ws_=None), dict(we_=None), dict(k_=None), dict(n_=None), dict(over_=None), dict(f_=None)):
        failed(co(**kw), INV)
    for rows in (0, -1, 4097, 1 << 40):
        failed(ks(rows=rows), INV)
        failed(co(rows=rows), INV)
    for bins in (0, -1, 4097):
        failed(ks(bins=bins), INV)
        failed(co(bins=bins), INV)
    failed(co(cid_=987_654), NOC)
    assert (k == 7).all() and (at == 7).all() and (n == 7).all() and (over == 7).all()
    t, c = C.c_int32(), C.c_int32()
    assert lib.ftk_hist_ks_shape(None, C.byref(c)) == INV and lib.ftk_hist_ks_shape(C.byref(t), None) == INV
    with pytest.raises(ValueError):
        engine.hist_ks(np.ones(5, np.uint32))
    with pytest.raises(L.FtkError):
        engine.hist_ks(np.ones((0, 5), np.uint32))
    with pytest.raises(KeyError):
        engine.cofrag("cf:nowhere", [0], [10], 0, 5)


def test_the_limits_themselves(engine, arrangement):
    """4096 lengths (one row pair) and 4096 rows (one length): the widest axes the calls take."""
    hist, want = wanted(("wide",), lambda: H.random_hist(np.random.default_rng(11), 2, 4096))
    same(engine.hist_ks(hist), want)
    hist, want = wanted(("tall",), lambda: H.random_hist(np.random.default_rng(12), 4096, 1))
    K, at, n = engine.hist_ks(hist)
    assert not K.any() and not at.any() and np.array_equal(n, want[2])  # one length: C = n, every difference is 0


# ---- 7. the product path ------------------------------------------------------------------------------------------------
def test_frag_cofragmentation_end_to_end(engine, tmp_path):
    from finaletoolkit_amd import utils, writers
    frag = os.path.join(DATA, "12.3444.b37.frag.gz")
    sizes = os.path.join(DATA, "b37.chrom.sizes")
    size12 = dict(utils.chrom_sizes_to_list(sizes))["12"]
    bin_size = 34_444_500  # four bins on contig 12; the file's fragments fall on both sides of the first bound
    opts = dict(bin_size=bin_size, contigs=["12"], chrom_sizes=sizes, min_length=100, max_length=260, quality_threshold=30, min_count=1)
    track, pairs = str(tmp_path / "track.tsv"), str(tmp_path / "pairs.tsv.gz")
    res = utils.frag_cofragmentation(frag, output_file=track, pairs_file=pairs, **opts)
    assert len(res) == 1
    r = res[0]
    starts, stops = utils.cofrag_bins(size12, bin_size)
    assert r.contig == "12" and len(starts) == 4 and np.array_equal(r.starts, starts) and np.array_equal(r.stops, stops)
    s, e, q, st = read_frag_gz(frag)["12"]
    engine.load_contig("cf:file", s, e, q, st)
    try:
        hist, over = engine.fraglen_hist("cf:file", starts, stops, 100, 161, 30, 100, 260)
    finally:
        engine.release("cf:file")
    K, at, n = H.ks_matrix(hist)
    assert np.array_equal(r.K, K) and np.array_equal(r.n, n) and np.array_equal(r.at, at + 100) and np.array_equal(r.overflow, over)
    assert n[0] > 0 and n[1] > 0 and K[0, 1] > 0 and r.valid.tolist() == [True, True, False, False]
    assert r.D[0, 1] == K[0, 1] / (n[0] * n[1]) and np.isnan(r.pc1).all()  # (two valid bins: no correlation)
    assert open(track).read() == writers.cofrag_track_text(res)
    assert gzip.open(pairs, "rt").read() == writers.cofrag_pairs_text(res)
    rows = [ln.split("\t") for ln in open(track).read().splitlines()[1:]]
    assert [int(x[1]) for x in rows] == starts.tolist() and [int(x[3]) for x in rows] == n.tolist()
    rows = [ln.split("\t") for ln in gzip.open(pairs, "rt").read().splitlines()[1:]]
    assert len(rows) == 6 and int(rows[0][5]) == K[0, 1] and float(rows[0][6]) == r.D[0, 1] and int(rows[0][7]) == r.at[0, 1]
    # the command line, in a child process
    cli_t, cli_p = str(tmp_path / "cli.tsv.gz"), str(tmp_path / "cli_pairs.tsv")
    p = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.cofrag", frag, cli_t, "--pairs", cli_p, "--bin-size", str(bin_size),
                        "--contigs", "12", "--chrom-sizes", sizes, "--min-length", "100", "--max-length", "260", "-q", "30",
                        "--min-count", "1"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert gzip.open(cli_t, "rt").read() == writers.cofrag_track_text(res) and open(cli_p).read() == writers.cofrag_pairs_text(res)
    # more than 4096 bins says so
    with pytest.raises(ValueError, match="at most 4096 bins"):
        utils.frag_cofragmentation(frag, bin_size=10_000, contigs=["12"], chrom_sizes=sizes)
