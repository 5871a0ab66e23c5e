"""GPU: the site-aggregated midpoint profile (``csrc/ftk_siteprofile.hip``) - ``Engine.site_profile`` against a numpy
restatement of its rule (``tests/site_profile_helpers.py``), exactly equal everywhere (sums and counts are integers): sites on the edges of
hand-placed midpoints, at the contig's ends, in a gap and on a run of copies longer than one chunk, every shape from
one bin to 4096, site lists in any order with repeats, empty groups, more groups than workgroups fit and groups that
several workgroups flush into; weights past 2^48; the ties to ``window_counts`` and ``weighted_window_sums``; a contig
with read1 columns; empty inputs; the C ABI's argument errors; and ``frag_site_profile`` / the command line on a
synthetic BAM and its fragment file.

The rule: a fragment passes with ``mapq >= mapq_min`` and ``min_len <= end - start <= max_len``; its midpoint is ``m =
(start + end) >> 1``; it contributes to site ``i`` when ``d = m - c_i`` lies in ``[-H, H)``, in bin ``k = (d + H) // b``
(``n_bins - 1 - k`` for a flipped site): ``count[g_i][k] += 1``, ``sum[g_i][k] += w``."""
import ctypes as C
import gzip
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests.gc_genome import LAYOUT, N_DUP, Contig, make_contig
from tests.helpers import read_frag_gz, write_2bit, write_synthetic_bam
from tests.site_profile_helpers import restated_profile

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 65536           # FTK_WEIGHT_ONE
CHUNK = 4096          # kChunk
U32_MAX = 2 ** 32 - 1
EVEN, ODD = (5_000, 5_100), (7_000, 7_101)  # hand-placed fragments: midpoints 5050 and 7050 (7050.5 rounded down)
GAP = (30_000, 33_000)                      # no fragment starts or ends in here
DUP = (1_000, 1_150)                        # N_DUP copies: midpoint 1075
LONG = (35_700, 36_400)                     # the contig's longest fragment (700): its start lies in the 512-bp index bin
LONG_MID = 36_050                           # before the one of its midpoint
LAST_END = 40_600
SHAPES = ((1, 1), (1, 2), (1000, 1), (990, 15), (300, 600), (2048, 1))
FILTERS = ((0, None, None), (30, 120, 180))
assert N_DUP > CHUNK and (LONG[0] >> 9) < (LONG_MID >> 9)


def profile_contig(rng):
    """(start, end, mapq, r1_start, r1_end) sorted by start: about 8 000 random fragments of lengths 20-600 outside GAP,
    the hand-placed ones on both sides of the MAPQ threshold, LONG, and N_DUP copies of DUP."""
    a = np.concatenate([rng.integers(0, 29_000, 6000), rng.integers(33_100, 40_000, 1500)])
    ln = rng.integers(20, 601, len(a))
    outside = (a + ln <= GAP[0]) | (a >= GAP[1])
    a, ln = a[outside], ln[outside]
    s = list(a) + [EVEN[0], ODD[0], EVEN[0], ODD[0], 0, 0, 39_990, LONG[0]] + [DUP[0]] * N_DUP
    e = list(a + ln) + [EVEN[1], ODD[1], EVEN[1], ODD[1], 1, 600, LAST_END, LONG[1]] + [DUP[1]] * N_DUP
    q = list(rng.integers(0, 61, len(a))) + [60, 60, 29, 30, 60, 60, 60, 60] + [60] * N_DUP
    s, e, q = np.array(s, np.int64), np.array(e, np.int64), np.array(q, np.int64)
    fwd = rng.integers(0, 2, len(s)).astype(bool)
    rl = np.minimum(60, e - s)
    r1s = np.where(fwd, s, e - rl)
    o = np.argsort(s, kind="stable")
    s, e, q, r1s, rl = s[o], e[o], q[o], r1s[o], rl[o]
    assert (e - s).max() == LONG[1] - LONG[0] and ((e - s) == LONG[1] - LONG[0]).sum() == 1
    return s, e, q, r1s, r1s + rl


def boundary_sites(H):
    """Centres that put a bound of [c - H, c + H) on a hand-placed midpoint, and the other edge cases; every centre
    once unflipped and once flipped.  Each site is a group of its own, so every one is compared on its own."""
    cs = []
    for mid in ((EVEN[0] + EVEN[1]) >> 1, (ODD[0] + ODD[1]) >> 1):
        cs += [mid + H, mid - H + 1, mid - H, mid + H - 1, mid + H + 1, mid]  # c - H, c + H - 1, c + H on the midpoint; beside them
    cs += [0, 1, 100_000, (1 << 30) - 1, (GAP[0] + GAP[1]) >> 1, (DUP[0] + DUP[1]) >> 1, LAST_END, LAST_END + H]
    # the longest fragment: its midpoint on c - H (counted, in the first bin), one before it (not counted), and its
    # START lmax before c - H (the first candidate the index has to hand the site; its midpoint lies below c - H)
    cs += [LONG_MID + H, LONG_MID + H + 1, LONG[1] + H]
    cs = [c for c in cs if 0 <= c < 1 << 30]
    centres = np.array(cs + cs, np.int32)
    flip = np.array([0] * len(cs) + [1] * len(cs), np.uint8)
    return centres, flip, np.arange(len(centres), dtype=np.int32)


def assert_same(got, want, what):
    for k, name in ((0, "sums"), (1, "counts")):
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, (what, name, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (what, name, bad[:5].tolist(), [int(got[k][tuple(i)]) for i in bad[:5]],
                               [int(want[k][tuple(i)]) for i in bad[:5]])


@pytest.fixture(scope="module")
def world(engine):
    import torch
    rng = np.random.default_rng(20261019)
    cols = profile_contig(rng)
    n = len(cols[0])
    mapq = cols[2].astype(np.uint8)
    zeros = np.zeros(n, np.uint8)
    s32, e32 = cols[0].astype(np.int32), cols[1].astype(np.int32)
    engine.load_contig("sp:plain", s32, e32, mapq, zeros)
    engine.load_contig("sp:bare", s32, e32, mapq, zeros)  # never gets a weight column
    engine.load_contig("sp:bam", s32, e32, mapq, zeros, cols[3].astype(np.int32), cols[4].astype(np.int32))
    is_dup = (cols[0] == DUP[0]) & (cols[1] == DUP[1])
    random = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    random[is_dup] = U32_MAX
    w = dict(cols=cols, n=n, n_cu=torch.cuda.get_device_properties(0).multi_processor_count, weights={
        "random": random,
        "zeros20": np.where(rng.random(n) < 0.2, 0, rng.integers(1, 2 ** 32, n, dtype=np.uint64)).astype(np.uint32),
        "unit": np.full(n, ONE, np.uint32),
    })
    assert is_dup.sum() == N_DUP and 7000 < n - N_DUP < 9000
    yield w
    for key in ("sp:plain", "sp:bare", "sp:bam"):
        engine.release(key)


# ---- 1. boundaries and shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H, b", SHAPES)
def test_boundaries_at_every_shape(engine, world, H, b):
    cols, w = world["cols"], world["weights"]["random"]
    engine.set_weights("sp:plain", w)
    centres, flip, groups = boundary_sites(H)
    ng = len(centres)
    long_len = LONG[1] - LONG[0]
    for mapq_min, min_len, max_len in FILTERS + ((0, None, long_len), (0, long_len, long_len)):
        want = restated_profile(cols, w, centres, flip, groups, ng, H, b, mapq_min, min_len, max_len)
        got = engine.site_profile("sp:plain", centres, flip, groups, ng, H, b, mapq_min, min_len, max_len, weighted=True)
        assert_same(got, want, (H, b, mapq_min, min_len, max_len))
        assert got[0].shape == (ng, 2 * H // b)
    # the cases are what they are meant to be (no filter): the site on the copies, the gap, the ends, the longest fragment
    _, cnt = restated_profile(cols, None, centres, flip, groups, ng, H, b, 0, None, None)
    half = ng // 2
    at = {int(c): i for i, c in enumerate(centres[:half].tolist())}
    assert cnt[at[(DUP[0] + DUP[1]) >> 1]].sum() >= N_DUP
    assert not cnt[at[(GAP[0] + GAP[1]) >> 1]].any() or H > 1400
    assert not cnt[at[100_000]].any() and not cnt[at[(1 << 30) - 1]].any()
    only_long = restated_profile(cols, None, centres, flip, groups, ng, H, b, 0, long_len, long_len)[1]
    assert only_long[at[LONG_MID + H], 0] == 1 and only_long[at[LONG_MID + H] + half, -1] == 1  # on c - H: the first bin, flipped the last
    assert not only_long[at[LONG_MID + H + 1]].any() and not only_long[at[LONG[1] + H]].any()
    for mid in ((EVEN[0] + EVEN[1]) >> 1, (ODD[0] + ODD[1]) >> 1):  # the hand-placed pair: in at c - H and c + H - 1, out at c + H
        assert cnt[at[mid + H], 0] >= 2 and cnt[at[mid - H + 1], -1] >= 2 and cnt[at[mid + H] + half, -1] >= 2
        assert cnt[at[mid - H + 1]].sum() - cnt[at[mid - H]].sum() >= 2 - cnt[at[mid - H], 0]  # one step down: the midpoint leaves
    if 2 * H // b > 1:  # a flipped site's profile is the unflipped one reversed, and differs from it
        assert np.array_equal(cnt[:half], cnt[half:, ::-1]) and not np.array_equal(cnt[:half], cnt[half:])


# ---- 2. site lists -----------------------------------------------------------------------------------------------------------
def site_lists(rng, n_cu):
    r = lambda n: rng.integers(0, 42_000, n).astype(np.int32)  # noqa: E731
    many = 4 * n_cu + 3
    lists = {
        "unsorted": (np.array([20_000, 500, 39_000, 900, 0, 20_001, 950, 5_050], np.int32), np.array([0, 1, 0, 1, 1, 0, 0, 1], np.uint8),
                     np.array([1, 0, 1, 0, 2, 1, 0, 2], np.int32), 3),
        "twice": (np.array([7_050, 1_075, 7_050, 7_050, 1_075], np.int32), np.array([0, 0, 0, 1, 0], np.uint8),
                  np.array([0, 0, 0, 0, 1], np.int32), 2),
        "overlapping": (np.arange(4_000, 9_000, 37, dtype=np.int32), None, None, 1),
        "interleaved": (r(600), rng.integers(0, 2, 600).astype(np.uint8), (np.arange(600) % 5).astype(np.int32), 5),
        "empty_group": (r(50), None, rng.choice([0, 2, 4], 50).astype(np.int32), 6),  # groups 1, 3 and 5 have no site
        "many_groups": (r(many), rng.integers(0, 2, many).astype(np.uint8), rng.permutation(many).astype(np.int32), many),
        # more than four sites per compute unit in one call: runs of several sites, and many workgroups per group
        "big_group": (r(12 * n_cu + 5), rng.integers(0, 2, 12 * n_cu + 5).astype(np.uint8),
                      (rng.random(12 * n_cu + 5) < 0.9).astype(np.int32), 2),
        "no_flip_no_groups": (r(300), None, None, 1),
    }
    return lists


@pytest.mark.parametrize("H, b", [(990, 15), (1000, 1)])
def test_site_lists(engine, world, H, b):
    rng = np.random.default_rng(H)
    cols, w = world["cols"], world["weights"]["zeros20"]
    engine.set_weights("sp:plain", w)
    lists = site_lists(rng, world["n_cu"])
    for name, (centres, flip, groups, ng) in lists.items():
        for mapq_min, min_len, max_len in FILTERS:
            want = restated_profile(cols, w, centres, flip, groups, ng, H, b, mapq_min, min_len, max_len)
            got = engine.site_profile("sp:plain", centres, flip, groups, ng, H, b, mapq_min, min_len, max_len, weighted=True)
            assert_same(got, want, (name, mapq_min))
    # the lists are what they are meant to be
    cnt = {k: restated_profile(cols, None, c, f, g, ng, H, b, 0)[1] for k, (c, f, g, ng) in lists.items()}
    assert len(lists["many_groups"][0]) > 4 * world["n_cu"] and len(lists["big_group"][0]) > 12 * world["n_cu"]
    assert np.bincount(lists["big_group"][2])[1] > 8 * world["n_cu"]
    assert cnt["empty_group"][[1, 3, 5]].sum() == 0
    assert all(cnt["empty_group"][g].any() for g in (0, 2, 4))
    one = restated_profile(cols, None, [7_050], None, None, 1, H, b, 0)[1][0]
    dup = restated_profile(cols, None, [1_075], None, None, 1, H, b, 0)[1][0]
    assert np.array_equal(cnt["twice"][0], 2 * one + one[::-1] + dup) and np.array_equal(cnt["twice"][1], dup)
    assert cnt["overlapping"].sum() > 3 * (world["n"] - N_DUP)  # every fragment near them counts for many sites
    assert (cnt["many_groups"].sum(axis=1) > 0).sum() > 0.8 * len(lists["many_groups"][0])


def test_more_runs_than_one_launch_holds(engine, world):
    """More than 2^20 runs (one group per site): the call splits its launches.  One bin, so the restatement is two
    bisections per site on the sorted midpoints and a running sum of the weights."""
    rng = np.random.default_rng(20)
    n = (1 << 20) + 37
    centres = rng.integers(2_500, 42_000, n).astype(np.int32)  # (clear of the copies: 10^6 sites on them would take seconds)
    centres[:3] = (1_075, 5_050, 36_050 + 300)
    groups = rng.permutation(n).astype(np.int32)
    flip = rng.integers(0, 2, n).astype(np.uint8)
    cols, w = world["cols"], world["weights"]["zeros20"]
    engine.set_weights("sp:plain", w)
    H = 300
    s, e, q = (np.asarray(cols[k], np.int64) for k in range(3))
    keep = (q >= 30) & (e - s >= 120) & (e - s <= 180)
    mid = ((s + e) >> 1)[keep]
    o = np.argsort(mid, kind="stable")
    mid, run = mid[o], np.concatenate([[0], np.cumsum(w.astype(np.int64)[keep][o])])
    lo, hi = np.searchsorted(mid, centres.astype(np.int64) - H, "left"), np.searchsorted(mid, centres.astype(np.int64) + H, "left")
    want_sum, want_cnt = np.zeros(n, np.int64), np.zeros(n, np.int64)
    want_sum[groups], want_cnt[groups] = run[hi] - run[lo], hi - lo
    sums, counts = engine.site_profile("sp:plain", centres, flip, groups, n, H, 2 * H, 30, 120, 180, weighted=True)
    assert sums.shape == counts.shape == (n, 1)
    assert np.array_equal(counts[:, 0], want_cnt) and np.array_equal(sums[:, 0], want_sum)
    assert want_cnt[groups[0]] >= N_DUP and (want_cnt[1 << 20:] > 0).any()  # groups of the second launch count


# ---- 3. weights --------------------------------------------------------------------------------------------------------------
def test_weights(engine, world):
    from finaletoolkit_amd import _lib as L
    cols = world["cols"]
    rng = np.random.default_rng(3)
    centres = np.concatenate([[1_075, 1_000, 5_050], rng.integers(0, 41_000, 200)]).astype(np.int32)
    flip = rng.integers(0, 2, len(centres)).astype(np.uint8)
    groups = rng.integers(0, 4, len(centres)).astype(np.int32)
    groups[:2] = 3
    H, b = 990, 15
    results = {}
    for tag, w in world["weights"].items():
        engine.set_weights("sp:plain", w)
        for mapq_min, min_len, max_len in FILTERS:
            want = restated_profile(cols, w, centres, flip, groups, 4, H, b, mapq_min, min_len, max_len)
            got = engine.site_profile("sp:plain", centres, flip, groups, 4, H, b, mapq_min, min_len, max_len, weighted=True)
            assert_same(got, want, (tag, mapq_min))
            results[tag, mapq_min] = got
            if tag == "unit":
                assert np.array_equal(got[0], ONE * got[1])
                # weighted=False: the same numbers, with the column attached and on a contig that never had one
                for key in ("sp:plain", "sp:bare"):
                    plain = engine.site_profile(key, centres, flip, groups, 4, H, b, mapq_min, min_len, max_len, weighted=False)
                    assert_same(plain, got, (key, "unweighted"))
    big = results["random", 0][0]
    assert big.max() >= N_DUP * U32_MAX > 2 ** 48 and (big > 2 ** 32).sum() > 100   # the copies' bin, and ordinary bins
    above_zero = restated_profile(cols, world["weights"]["zeros20"] != 0, centres, flip, groups, 4, H, b, 0)[0]
    assert (above_zero < results["zeros20", 0][1]).sum() > 100 and (results["zeros20", 0][0] > 0).sum() > 100  # weight-0 fragments count
    with pytest.raises(L.FtkError, match="weights"):
        engine.site_profile("sp:bare", centres, flip, groups, 4, H, b, weighted=True)


# ---- 4. ties to the pinned kernels -------------------------------------------------------------------------------------------
def test_one_bin_equals_the_window_kernels(engine, world):
    w = world["weights"]["random"]
    engine.set_weights("sp:plain", w)
    rng = np.random.default_rng(4)
    for H in (1, 300, 1000):
        centres = np.concatenate([boundary_sites(H)[0][: len(boundary_sites(H)[0]) // 2], rng.integers(H, 41_000, 100)]).astype(np.int32)
        centres = centres[(centres >= H) & (centres < (1 << 30) - H)]  # windows the window calls can hold in int32
        groups = np.arange(len(centres), dtype=np.int32)
        for mapq_min, min_len, max_len in FILTERS:
            sums, counts = engine.site_profile("sp:plain", centres, None, groups, len(centres), H, 2 * H, mapq_min, min_len, max_len,
                                               weighted=True)
            ws, we = centres.astype(np.int64) - H, centres.astype(np.int64) + H
            assert np.array_equal(counts[:, 0], engine.window_counts("sp:plain", ws, we, mapq_min, min_len, max_len, "midpoint"))
            assert np.array_equal(sums[:, 0], engine.weighted_window_sums("sp:plain", ws, we, mapq_min, min_len, max_len, "midpoint")[0])
        assert counts.sum() > 100


# ---- 5. a contig with read1 columns ------------------------------------------------------------------------------------------
def test_read1_columns_play_no_part(engine, world):
    assert engine.is_bam("sp:bam") and not engine.is_bam("sp:plain")
    w = world["weights"]["zeros20"]
    engine.set_weights("sp:plain", w)
    engine.set_weights("sp:bam", w)
    rng = np.random.default_rng(5)
    centres, flip, groups = rng.integers(0, 41_000, 400).astype(np.int32), rng.integers(0, 2, 400).astype(np.uint8), rng.integers(0, 3, 400)
    for H, b in ((990, 15), (1, 1)):
        for weighted in (False, True):
            a = engine.site_profile("sp:plain", centres, flip, groups, 3, H, b, 30, 100, 220, weighted=weighted)
            c = engine.site_profile("sp:bam", centres, flip, groups, 3, H, b, 30, 100, 220, weighted=weighted)
            assert_same(c, a, (H, b, weighted))
            assert_same(a, restated_profile(world["cols"], w if weighted else None, centres, flip, groups, 3, H, b, 30, 100, 220), (H, b))
    assert a[1].sum() > 0


# ---- 6. empty inputs ---------------------------------------------------------------------------------------------------------
def test_empty_contig_and_no_sites(engine, world):
    z = np.zeros(0, np.int32)
    engine.load_contig("sp:empty", z, z, np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    try:
        for weighted in (False, True):
            if weighted:
                engine.set_weights("sp:empty", np.zeros(0, np.uint32))
            sums, counts = engine.site_profile("sp:empty", [0, 500, (1 << 30) - 1], [0, 1, 0], [0, 2, 1], 3, 990, 15, 0, weighted=weighted)
            assert sums.shape == counts.shape == (3, 132) and not sums.any() and not counts.any()
    finally:
        engine.release("sp:empty")
    sums, counts = engine.site_profile("sp:bare", [], None, None, 2, 1000, 1)
    assert sums.shape == counts.shape == (2, 2000) and sums.dtype == counts.dtype == np.int64
    assert not sums.any() and not counts.any()
    sums, counts = engine.site_profile("sp:bare", np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.int32), 1, 300, 600)
    assert sums.shape == (1, 1) and not sums.any() and not counts.any()
    # count_out may be NULL; the outputs of a call with sites are overwritten, not added to
    from finaletoolkit_amd import _lib as L
    c = np.array([5_050], np.int32)
    out = np.full(2, 7, np.int64)
    assert engine.lib.ftk_site_profile(engine.ctx, engine.contig_id("sp:bare"), L.ptr(c), None, None, 1, 1, 1, 1, 0, -1, -1, 0,
                                       L.ptr(out), None) == L.FTK_OK
    want = restated_profile(world["cols"], None, c, None, None, 1, 1, 1, 0)[0][0]
    assert out.tolist() == want.tolist() and out[1] >= 2 * ONE


# ---- 7. the C ABI's argument errors ------------------------------------------------------------------------------------------
def test_argument_errors(engine, world):
    from finaletoolkit_amd import _lib as L
    lib, ctx, P = engine.lib, engine.ctx, L.ptr
    cid, bare = engine.contig_id("sp:plain"), engine.contig_id("sp:bare")
    engine.set_weights("sp:plain", world["weights"]["unit"])
    centre = np.array([100, 5_050, 7_050], np.int32)
    flip, group = np.array([0, 1, 0], np.uint8), np.array([0, 1, 1], np.int32)
    sums, counts = np.full(2 * 4096, 7, np.int64), np.full(2 * 4096, 7, np.int64)
    INV, NOC = L.FTK_ERR_INVALID, L.FTK_ERR_NO_CONTIG

    def call(ctx_=ctx, cid_=cid, centre_=centre, flip_=flip, group_=group, n=3, ng=2, H=1000, b=1, q=30, lo=-1, hi=-1, w=0,
             sums_=sums, counts_=counts):
        return lib.ftk_site_profile(ctx_, cid_, P(centre_), P(flip_), P(group_), n, ng, H, b, q, lo, hi, w, P(sums_), P(counts_))

    def failed(rc, code, word=None):
        assert rc == code, (rc, code)
        message = lib.ftk_last_error(ctx)
        assert message and (word is None or word in message), message

    assert call(ctx_=None) == INV
    failed(call(centre_=None), INV)
    failed(call(sums_=None), INV)
    for H in (0, -1, (1 << 20) + 1):
        failed(call(H=H, b=max(2 * H, 1)), INV, b"half_width")
    for b in (0, -15, 3, 2001):
        failed(call(b=b), INV, b"bin_size")
    failed(call(H=2049, b=1), INV, b"bins")           # 4098 bins
    failed(call(H=1 << 20, b=256), INV, b"bins")      # 8192 bins
    failed(call(ng=0), INV, b"n_groups")
    failed(call(ng=-3), INV, b"n_groups")
    failed(call(ng=(1 << 28) // 2000 + 1), INV, b"n_groups")   # n_groups * n_bins > 2^28
    failed(call(centre_=np.array([100, -1, 7_050], np.int32)), INV, b"centre")
    failed(call(centre_=np.array([100, 1 << 30, 7_050], np.int32)), INV, b"centre")
    failed(call(group_=np.array([0, 2, 1], np.int32)), INV, b"group")
    failed(call(group_=np.array([0, -1, 1], np.int32)), INV, b"group")
    failed(call(group_=None, ng=1, centre_=np.array([100, 1 << 30, 7_050], np.int32)), INV, b"centre")
    failed(call(cid_=bare, w=1), INV, b"ftk_frags_set_weights")    # the message names the weights calls
    assert b"ftk_frags_set_gc_weights" in lib.ftk_last_error(ctx)
    failed(call(n=-1), INV, b"n_sites")
    failed(call(cid_=987_654), NOC)
    failed(call(cid_=987_654, n=0), NOC)
    assert np.all(sums == 7) and np.all(counts == 7)  # nothing was written by any of them
    # and the same arguments, in range, succeed: the largest half-width, 4096 bins, n_groups * n_bins = 2^28 is not tried
    assert call(H=1 << 20, b=512) == L.FTK_OK and call(H=2048, b=1) == L.FTK_OK and call(w=1) == L.FTK_OK
    assert not np.any(sums[: 2 * 2000] == 7)


# ---- 8. the product path -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def product(engine, tmp_path_factory):
    from finaletoolkit_amd import utils
    d = tmp_path_factory.mktemp("siteprofile")
    rng = np.random.default_rng(99)
    seqs = {name: make_contig(rng, n, n_runs, lower) for name, (n, n_runs, lower) in LAYOUT.items() if name in ("wA", "wC")}
    ref = str(d / "g.2bit")
    write_2bit(ref, seqs)
    contigs = [("wA", LAYOUT["wA"][0]), ("wX", 9_000), ("wC", LAYOUT["wC"][0])]  # wX: in the input, not in the reference
    frags = {}
    for name, n in contigs:
        a = np.sort(rng.integers(0, n - 400, 2500))
        ln = rng.integers(90, 240, 2500)
        frags[name] = (a, a + ln, rng.choice([0, 10, 29, 30, 42, 60], 2500), rng.integers(0, 2, 2500))
    bam = str(d / "in.bam")
    write_synthetic_bam(bam, contigs, frags)
    frag = str(d / "in.frag.gz")
    utils.frag_export(bam, frag, quality_threshold=0)
    names = ["CTCF", "GATA1", ".", "SPI1"]
    rows = []
    for name, n in contigs + [("wZ", 50_000)]:  # wZ: in neither
        for a in rng.integers(0, n - 50, 60).tolist():
            rows.append((name, a, a + int(rng.integers(1, 40)), names[int(rng.integers(0, 4))], "-" if rng.random() < 0.4 else "+"))
    bed = str(d / "sites.bed")
    with open(bed, "w") as fh:
        fh.write("# sites\n" + "".join(f"{c}\t{a}\t{b}\t{nm}\t0\t{st}\n" for c, a, b, nm, st in rows))
    bedgz = str(d / "sites.bed.gz")
    with gzip.open(bedgz, "wt") as fh:
        fh.write(open(bed).read())
    return dict(dir=d, ref=ref, bam=bam, frag=frag, bed=bed, bedgz=bedgz, rows=rows, cols=read_frag_gz(frag),
                contigs={name: Contig(name, s) for name, s in seqs.items()})


def restated_product(p, table, lo, hi, H, b, by_name, skip, mapq_min=30):
    """(groups, n_sites, units, count) of the site file from the fragment file's rows; ``table``: the weight table, or
    None for the uncorrected profile; ``skip``: the contigs left out."""
    sites = [(c, (a + z) // 2, nm, st) for c, a, z, nm, st in p["rows"]]
    groups = list(dict.fromkeys(s[2] for s in sites)) if by_name else ["all"]
    n_bins = 2 * H // b
    units, count, n_sites = np.zeros((len(groups), n_bins), np.int64), np.zeros((len(groups), n_bins), np.int64), np.zeros(len(groups), np.int64)
    for c in dict.fromkeys(s[0] for s in sites):
        if c in skip:
            continue
        mine = [s for s in sites if s[0] == c]
        cols = p["cols"][c]
        w = None
        if table is not None:
            s, e, q = (np.asarray(cols[k], np.int64) for k in range(3))
            ln = e - s
            gc = p["contigs"][c].gc(s, e)
            ok = (q >= mapq_min) & (ln >= lo) & (ln <= hi) & (gc >= 0)
            w = np.zeros(len(s), np.int64)
            w[ok] = table[ln[ok] - lo, gc[ok]]
        g = np.array([groups.index(s[2]) if by_name else 0 for s in mine])
        got = restated_profile(cols, w, [s[1] for s in mine], [s[3] == "-" for s in mine], g, len(groups), H, b, mapq_min, lo, hi)
        units += got[0]
        count += got[1]
        n_sites += np.bincount(g, minlength=len(groups))
    return tuple(groups), n_sites, units, count


def same_profile(a, b):
    return (a.groups == b.groups and np.array_equal(a.n_sites, b.n_sites) and np.array_equal(a.offsets, b.offsets)
            and np.array_equal(a.count, b.count) and np.array_equal(a.corrected, b.corrected) and a.skipped_contigs == b.skipped_contigs)


def run_profile(*args, **kwargs):
    from finaletoolkit_amd import utils
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = utils.frag_site_profile(*args, **kwargs)
    return res, [str(w.message) for w in caught if issubclass(w.category, UserWarning) and "frag_site_profile" in str(w.message)]


def test_frag_site_profile_end_to_end(engine, product, tmp_path):
    from finaletoolkit_amd import utils
    p = product
    lo, hi, stride, H, b = 100, 199, 3, 990, 15
    kw = dict(min_length=lo, max_length=hi, half_width=H, bin_size=b)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        bias = utils.frag_gc_bias(p["frag"], p["ref"], str(tmp_path / "bias.tsv.gz"), min_length=lo, max_length=hi, stride=stride)
    table = utils.gc_weights(bias)
    # uncorrected: only wZ is skipped; corrected == count
    res, notes = run_profile(p["frag"], p["bed"], **kw)
    groups, n_sites, units, count = restated_product(p, None, lo, hi, H, b, False, {"wZ"})
    assert len(notes) == 1 and "wZ" in notes[0] and "not in the input" in notes[0]
    assert res.groups == ("all",) and res.skipped_contigs == ("wZ",) and res.n_sites.tolist() == [180] == n_sites.tolist()
    assert np.array_equal(res.count, count) and np.array_equal(res.corrected, count.astype(np.float64))
    assert res.count.dtype == np.int64 and res.n_sites.dtype == np.int64 and res.offsets.dtype == np.int64 and res.corrected.dtype == np.float64
    assert res.offsets.tolist() == list(range(-H, H, b)) and res.count.shape == (1, 2 * H // b)
    assert same_profile(run_profile(p["bam"], p["bedgz"], **kw)[0], res)
    # corrected, from the BAM and from the fragment file, the bias given three ways: wZ and wX are skipped
    results = {}
    for tag, path in (("bam", p["bam"]), ("frag", p["frag"])):
        for how, given in (("none", None), ("table", bias), ("tsv", str(tmp_path / "bias.tsv.gz"))):
            r, notes = run_profile(path, p["bed"], reference_file=p["ref"], bias=given, by_name=True, stride=stride, **kw)
            assert len(notes) == 2 and "wZ" in notes[0] and "not in the input" in notes[0], notes
            assert "wX" in notes[1] and "not in the reference" in notes[1] and "wZ" not in notes[1], notes
            results[tag, how] = r
    res = results["frag", "none"]
    for k, other in results.items():
        assert same_profile(res, other), k
    groups, n_sites, units, count = restated_product(p, table, lo, hi, H, b, True, {"wZ", "wX"})
    first = list(dict.fromkeys(r[3] for r in p["rows"]))
    assert res.groups == groups == tuple(first) and set(groups) == {"CTCF", "GATA1", ".", "SPI1"}  # first-appearance order
    assert res.skipped_contigs == ("wZ", "wX") and np.array_equal(res.n_sites, n_sites) and n_sites.sum() == 120
    assert np.array_equal(res.count, count) and np.array_equal(res.corrected, units / 65536.0)
    # the cases bite: non-empty bins, a - site whose profile differs from its unflipped one, a weight-0 fragment in a window
    assert (count > 0).sum() >= 50 and not np.array_equal(units, count * ONE)
    minus = next(r for r in p["rows"] if r[0] == "wA" and r[4] == "-")
    one = [restated_profile(p["cols"]["wA"], None, [(minus[1] + minus[2]) // 2], [f], None, 1, H, b, 30, lo, hi)[1] for f in (1, 0)]
    assert one[0].any() and not np.array_equal(one[0], one[1]) and np.array_equal(one[0], one[1][:, ::-1])
    s, e, q = (np.asarray(p["cols"]["wA"][k], np.int64) for k in range(3))
    ok = (q >= 30) & (e - s >= lo) & (e - s <= hi)
    gc = p["contigs"]["wA"].gc(s, e)
    w0 = ok & ((gc < 0) | (table[np.clip(e - s - lo, 0, hi - lo), np.clip(gc, 0, hi)] == 0))
    centres_a = np.array([(r[1] + r[2]) // 2 for r in p["rows"] if r[0] == "wA"])
    mids = (s + e) >> 1
    assert (np.abs(mids[w0][:, None] - centres_a[None, :]) < H - 1).any()  # a weight-0 fragment inside a site's window
    # normalize: every row over its mean
    norm, _ = run_profile(p["frag"], p["bed"], reference_file=p["ref"], bias=bias, by_name=True, normalize=True, **kw)
    assert np.array_equal(norm.count, res.count)
    for g in range(len(groups)):
        row = res.corrected[g]
        assert row.mean() > 0 and np.array_equal(norm.corrected[g], row / row.mean())
    # the files, field by field, and the command line in a child process
    for suffix in (".tsv", ".tsv.gz"):
        out = str(tmp_path / ("fn" + suffix))
        again, _ = run_profile(p["frag"], p["bed"], out, reference_file=p["ref"], bias=bias, by_name=True, **kw)
        assert same_profile(again, res)
        text = gzip.open(out, "rt").read() if suffix.endswith(".gz") else open(out).read()
        lines = text.splitlines()
        assert lines[0] == "#group\tn_sites\toffset\tcount\tcorrected" and len(lines) == 1 + len(groups) * (2 * H // b)
        at = 1
        for g, name in enumerate(groups):
            for k in range(2 * H // b):
                assert lines[at].split("\t") == [name, str(int(n_sites[g])), str(-H + k * b), str(int(count[g, k])),
                                                 format(units[g, k] / 65536.0, ".6f")], (g, k)
                at += 1
        cli = str(tmp_path / ("cli" + suffix))
        r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.siteprofile", p["frag"], p["bed"], cli, "--reference", p["ref"],
                            "--bias", str(tmp_path / "bias.tsv.gz"), "--half-width", str(H), "--bin-size", str(b), "--min-length", str(lo),
                            "--max-length", str(hi), "-q", "30", "--by-name"], cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert "wX" in r.stderr and "wZ" in r.stderr  # the warnings
        if suffix == ".tsv":
            assert open(cli, "rb").read() == open(out, "rb").read()
        else:
            assert gzip.open(cli, "rb").read() == gzip.open(out, "rb").read()
