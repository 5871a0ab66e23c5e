"""GPU: the V-plot (``csrc/ftk_vplot.hip``) - ``Engine.site_vplot`` against the numpy restatement of its rule in
``tests/vplot_helpers.py``, exactly equal everywhere (sums and counts are integers): the edges of both axes, matrices
that no LDS budget holds in one tile (with ragged last tiles at 64 KiB and at 160 KiB, and the longest fragment handed
over by the last tile's reach), the exact ties to the pinned ``Engine.site_profile``, site lists in any order, weights
past 2^48, empty inputs, the C ABI's argument errors, and ``frag_vplot`` / the command line on a synthetic BAM and its
fragment file."""
import gzip
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests.gc_genome import LAYOUT, N_DUP, Contig, make_contig
from tests.helpers import read_frag_gz, write_2bit, write_synthetic_bam
from tests.vplot_helpers import (DUP, EVEN, LADDER, LADDER_MID, LAST_END, LONG, LONG_LEN, LONG_MID, ODD, ONE, U32_MAX, assert_same,
                                 restated_vplot, vplot_contig)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (1, 2), (990, 15), (2048, 1))
KEYS = ("vp:plain", "vp:bare", "vp:bam")


@pytest.fixture(scope="module")
def world(engine):
    import torch
    rng = np.random.default_rng(20261019)
    cols = vplot_contig(rng)
    n = len(cols[0])
    mapq = cols[2].astype(np.uint8)
    zeros = np.zeros(n, np.uint8)
    s32, e32 = cols[0].astype(np.int32), cols[1].astype(np.int32)
    engine.load_contig("vp:plain", s32, e32, mapq, zeros)
    engine.load_contig("vp:bare", s32, e32, mapq, zeros)  # never gets a weight column
    engine.load_contig("vp:bam", s32, e32, mapq, zeros, cols[3].astype(np.int32), cols[4].astype(np.int32))
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
    for key in KEYS:
        engine.release(key)


def edge_sites(H, few):
    """Centres that put a bound of [c - H, c + H) on a hand-placed midpoint, and the other edge cases; every centre once
    unflipped and once flipped.  Each site is a group of its own, so every one is compared on its own.  ``few``: the
    ladder's sites and the contig's ends only (for the shape of 4096 bins, whose matrices are large)."""
    cs = []
    for mid in (LADDER_MID,) if few else (LADDER_MID, (EVEN[0] + EVEN[1]) >> 1, (ODD[0] + ODD[1]) >> 1):
        cs += [mid + H, mid - H + 1, mid - H, mid]  # the midpoint on c - H, on c + H - 1, on c + H (out), in the middle
    cs += [0, 100_000, (1 << 30) - 1, LAST_END + H]
    if not few:
        cs += [(DUP[0] + DUP[1]) >> 1, LONG_MID + H, LONG_MID + H + 1]
    centres = np.array(cs + cs, np.int32)
    flip = np.array([0] * len(cs) + [1] * len(cs), np.uint8)
    return centres, flip, np.arange(len(centres), dtype=np.int32)


# ---- 1. the edges of both axes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H, b", SHAPES)
def test_edges_of_both_axes(engine, world, H, b):
    cols, w = world["cols"], world["weights"]["zeros20"]
    engine.set_weights("vp:plain", w)
    few = 2 * H // b == 4096
    centres, flip, groups = edge_sites(H, few)
    ng, half = len(centres), len(centres) // 2
    at = {int(c): i for i, c in enumerate(centres[:half].tolist())}
    len_lo, len_hi = 100, 199
    assert LADDER[0] < len_lo - 1 and len_hi + 1 < LADDER[-1]
    for lb in (5, 100) if few else (1, 5, 20, 100):  # one length per row ... the whole range in one row
        for mapq_min in (0, 30):
            want = restated_vplot(cols, w, centres, flip, groups, ng, H, b, len_lo, len_hi, lb, mapq_min)
            got = engine.site_vplot("vp:plain", centres, flip, groups, ng, H, b, len_lo, len_hi, lb, mapq_min, weighted=True)
            assert_same(got, want, (H, b, lb, mapq_min))
            assert got[0].shape == (ng, 100 // lb, 2 * H // b)
        # the cases are what they are meant to be: the ladder holds one fragment of every length on LADDER_MID, so the
        # site on it sees lengths len_lo and len_hi and not len_lo - 1 and len_hi + 1, and every row boundary
        cnt = restated_vplot(cols, None, centres, flip, groups, ng, H, b, len_lo, len_hi, lb, 60)[1]
        wide = restated_vplot(cols, None, centres, flip, groups, ng, H, b, len_lo - 1, len_hi + 1, 1, 60)[1]
        on = at[LADDER_MID]
        k_mid = H // b
        assert (cnt[on, :, k_mid] >= lb).all() and (wide[on, :, k_mid] >= 1).all()     # each length of each row, both outer lengths
        assert cnt[on].sum() == wide[on, 1:-1].sum() == wide[on].sum() - wide[on, 0].sum() - wide[on, -1].sum()
        assert wide[on, 0].sum() >= 1 and wide[on, -1].sum() >= 1
        # midpoints on c - H (first column), c + H - 1 (last column) and c + H (out)
        assert (cnt[at[LADDER_MID + H], :, 0] >= lb).all() and (cnt[at[LADDER_MID - H + 1], :, -1] >= lb).all()
        assert cnt[at[LADDER_MID - H + 1]].sum() - cnt[at[LADDER_MID - H]].sum() >= 100 - cnt[at[LADDER_MID - H], :, 0].sum()
        assert not cnt[at[100_000]].any() and not cnt[at[(1 << 30) - 1]].any()
        # flipped against unflipped: the offset axis is reversed, the length axis is not, and the two differ
        assert np.array_equal(cnt[:half], cnt[half:, :, ::-1])
        if 2 * H // b > 1:
            assert not np.array_equal(cnt[:half], cnt[half:])
        if 100 // lb > 1:
            assert not np.array_equal(cnt[:half], cnt[half:, ::-1, ::-1])


# ---- 2. tiling ---------------------------------------------------------------------------------------------------------------
# (H, b, len_lo, len_hi, lb, weighted): rows x bins x cell bytes, and the tiles at a budget of 64 KiB / 160 KiB
TILINGS = (
    (2048, 1, 151, 700, 50, False),   # 11 rows x 4096 bins x 4 B = 176 KiB: tiles of 4 rows (4 + 4 + 3) / of 10 (10 + 1)
    (2048, 1, 201, 700, 100, True),   # 5 rows x 4096 bins x 12 B = 240 KiB: tiles of 1 row / of 3 (3 + 2)
    (990, 15, 50, 574, 5, True),      # 105 rows x 132 bins x 12 B: tiles of 41 rows (41 + 41 + 23) / of 103 (103 + 2)
    (990, 15, 75, 700, 1, False),     # 626 rows x 132 bins x 4 B: tiles of 124 rows (5 x 124 + 6) / of 310 (2 x 310 + 6)
)


@pytest.mark.parametrize("H, b, len_lo, len_hi, lb, weighted", TILINGS)
def test_matrices_of_several_tiles(engine, world, H, b, len_lo, len_hi, lb, weighted):
    cols, w = world["cols"], world["weights"]["zeros20"]
    engine.set_weights("vp:plain", w)
    n_rows, n_bins, cell = (len_hi - len_lo + 1) // lb, 2 * H // b, 12 if weighted else 4
    for budget in (64 << 10, 160 << 10):  # more than one tile, the last one ragged (or tiles of one row)
        tile = budget // (cell * n_bins)
        assert n_rows > tile and (n_rows % tile or tile == 1), (budget, tile)
    rng = np.random.default_rng(H + lb)
    # the longest fragment with its midpoint on c - H, and one past it; the copies; the ladder; random sites
    centres = np.concatenate([[LONG_MID + H, LONG_MID + H + 1, 1_075, LADDER_MID], rng.integers(0, 41_000, 8)]).astype(np.int32)
    flip = (np.arange(len(centres)) % 3 == 1).astype(np.uint8)
    groups = (np.arange(len(centres)) % 2).astype(np.int32)
    groups[0] = 0
    for mapq_min in (0, 30):
        want = restated_vplot(cols, w if weighted else None, centres, flip, groups, 2, H, b, len_lo, len_hi, lb, mapq_min)
        got = engine.site_vplot("vp:plain", centres, flip, groups, 2, H, b, len_lo, len_hi, lb, mapq_min, weighted=weighted)
        assert_same(got, want, (H, b, lb, mapq_min))
    for budget in (64 << 10, 160 << 10):  # every tile, at either budget, holds something
        tile = budget // (cell * n_bins)
        assert all(want[1][:, r0:r0 + tile].any() for r0 in range(0, n_rows, tile)), budget
    if len_hi != LONG_LEN:
        return
    # The longest fragment alone (one site): its midpoint lies on c - H and its length in the last row, so it counts in
    # the last row's first column - the last tile's reach has to hand it over, its start lies a whole index bin before
    # c - H.  One row outside the range it does not count.  (Both against the restatement on the contig without it.)
    one = np.array([LONG_MID + H], np.int32)
    is_long = (cols[0] == LONG[0]) & (cols[1] == LONG[1])
    assert is_long.sum() == 1
    rest = tuple(np.asarray(c)[~is_long] for c in cols[:3])
    w_use, w_rest = (w, w[~is_long]) if weighted else (None, None)
    for shift, inside in ((0, True), (lb, False)):
        lo_s, hi_s = len_lo - shift, len_hi - shift
        got = engine.site_vplot("vp:plain", one, None, None, 1, H, b, lo_s, hi_s, lb, 0, weighted=weighted)
        assert_same(got, restated_vplot(cols, w_use, one, None, None, 1, H, b, lo_s, hi_s, lb, 0), ("long", shift))
        without = restated_vplot(rest, w_rest, one, None, None, 1, H, b, lo_s, hi_s, lb, 0)
        extra = got[1] - without[1]
        assert extra.sum() == (1 if inside else 0) and extra[0, -1, 0] == (1 if inside else 0), shift


# ---- 3. ties to the pinned kernel --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["vp:plain", "vp:bam"])
def test_ties_to_site_profile(engine, world, key):
    assert engine.is_bam("vp:bam") and not engine.is_bam("vp:plain")
    engine.set_weights(key, world["weights"]["random"])
    rng = np.random.default_rng(3)
    centres = np.concatenate([[1_075, LADDER_MID, LONG_MID + 990], rng.integers(0, 41_000, 300)]).astype(np.int32)
    flip, groups = rng.integers(0, 2, len(centres)).astype(np.uint8), rng.integers(0, 3, len(centres)).astype(np.int32)
    for H, b, len_lo, len_hi, lb in ((990, 15, 100, 399, 5), (2048, 1, 201, 700, 100), (1, 1, 20, 699, 170)):
        n_rows = (len_hi - len_lo + 1) // lb
        for weighted in (False, True):
            sums, counts = engine.site_vplot(key, centres, flip, groups, 3, H, b, len_lo, len_hi, lb, 30, weighted=weighted)
            whole = engine.site_profile(key, centres, flip, groups, 3, H, b, 30, len_lo, len_hi, weighted=weighted)
            assert_same((sums.sum(axis=1), counts.sum(axis=1)), whole, (H, b, weighted, "rows summed"))
            for r in sorted({0, 1, n_rows // 2, n_rows - 1}):
                row = engine.site_profile(key, centres, flip, groups, 3, H, b, 30, len_lo + r * lb, len_lo + (r + 1) * lb - 1,
                                          weighted=weighted)
                assert_same((sums[:, r], counts[:, r]), row, (H, b, weighted, r))
            assert counts.sum() > 100
    if key == "vp:bam":  # the read1 columns play no part
        engine.set_weights("vp:plain", world["weights"]["random"])
        for weighted in (False, True):
            assert_same(engine.site_vplot("vp:bam", centres, flip, groups, 3, 990, 15, 100, 399, 5, 30, weighted=weighted),
                        engine.site_vplot("vp:plain", centres, flip, groups, 3, 990, 15, 100, 399, 5, 30, weighted=weighted), weighted)


# ---- 4. site lists -----------------------------------------------------------------------------------------------------------
def site_lists(rng, n_cu):
    r = lambda n: rng.integers(0, 42_000, n).astype(np.int32)  # noqa: E731
    many = 4 * n_cu + 3
    return {
        "unsorted": (np.array([20_000, 500, 39_000, 900, 0, 20_001, 950, 5_050], np.int32), np.array([0, 1, 0, 1, 1, 0, 0, 1], np.uint8),
                     np.array([1, 0, 1, 0, 2, 1, 0, 2], np.int32), 3),
        "twice": (np.array([7_050, 1_075, 7_050, 7_050, 1_075], np.int32), np.array([0, 0, 0, 1, 0], np.uint8),
                  np.array([0, 0, 0, 0, 1], np.int32), 2),
        "empty_group": (r(50), None, rng.choice([0, 2, 4], 50).astype(np.int32), 6),  # groups 1, 3 and 5 have no site
        "many_groups": (r(many), rng.integers(0, 2, many).astype(np.uint8), rng.permutation(many).astype(np.int32), many),
        # one group of more than twelve sites per compute unit: several runs flush into one group's matrix
        "big_group": (r(14 * n_cu + 5), rng.integers(0, 2, 14 * n_cu + 5).astype(np.uint8),
                      (rng.random(14 * n_cu + 5) < 0.95).astype(np.int32), 2),
        "no_flip_no_groups": (r(300), None, None, 1),
    }


def test_site_lists(engine, world):
    rng = np.random.default_rng(4)
    cols, w = world["cols"], world["weights"]["zeros20"]
    engine.set_weights("vp:plain", w)
    lists = site_lists(rng, world["n_cu"])
    H, b, len_lo, len_hi, lb = 990, 15, 100, 299, 40  # 5 rows x 132 bins
    cnt = {}
    for name, (centres, flip, groups, ng) in lists.items():
        want = restated_vplot(cols, w, centres, flip, groups, ng, H, b, len_lo, len_hi, lb, 30)
        got = engine.site_vplot("vp:plain", centres, flip, groups, ng, H, b, len_lo, len_hi, lb, 30, weighted=True)
        assert_same(got, want, name)
        plain = engine.site_vplot("vp:bare", centres, flip, groups, ng, H, b, len_lo, len_hi, lb, 30, weighted=False)
        assert np.array_equal(plain[1], want[1]) and np.array_equal(plain[0], ONE * want[1]), name
        cnt[name] = want[1]
    # the lists are what they are meant to be
    assert len(lists["many_groups"][0]) > 4 * world["n_cu"] and np.bincount(lists["big_group"][2])[1] > 12 * world["n_cu"]
    assert cnt["empty_group"][[1, 3, 5]].sum() == 0 and all(cnt["empty_group"][g].any() for g in (0, 2, 4))
    one = restated_vplot(cols, None, [7_050], None, None, 1, H, b, len_lo, len_hi, lb, 30)[1][0]
    dup = restated_vplot(cols, None, [1_075], None, None, 1, H, b, len_lo, len_hi, lb, 30)[1][0]
    assert np.array_equal(cnt["twice"][0], 2 * one + one[:, ::-1] + dup) and np.array_equal(cnt["twice"][1], dup)
    assert (cnt["many_groups"].sum(axis=(1, 2)) > 0).sum() > 0.8 * len(lists["many_groups"][0])


# ---- 5. weights --------------------------------------------------------------------------------------------------------------
def test_weights(engine, world):
    from finaletoolkit_amd import _lib as L
    cols = world["cols"]
    rng = np.random.default_rng(5)
    centres = np.concatenate([[1_075, 1_000, 5_050], rng.integers(0, 41_000, 200)]).astype(np.int32)
    flip = rng.integers(0, 2, len(centres)).astype(np.uint8)
    groups = rng.integers(0, 4, len(centres)).astype(np.int32)
    groups[:2] = 3
    args = (990, 15, 100, 399, 5)
    results = {}
    for tag, w in world["weights"].items():
        engine.set_weights("vp:plain", w)
        for mapq_min in (0, 30):
            want = restated_vplot(cols, w, centres, flip, groups, 4, *args, mapq_min)
            got = engine.site_vplot("vp:plain", centres, flip, groups, 4, *args, mapq_min, weighted=True)
            assert_same(got, want, (tag, mapq_min))
            results[tag, mapq_min] = got
            if tag == "unit":
                assert np.array_equal(got[0], ONE * got[1])
                for key in ("vp:plain", "vp:bare"):  # weighted=False: the same numbers, with a column attached and without one
                    assert_same(engine.site_vplot(key, centres, flip, groups, 4, *args, mapq_min, weighted=False), got, (key, "unweighted"))
    big, n_big = results["random", 0]
    assert big.max() >= N_DUP * U32_MAX > 2 ** 48 and n_big.max() >= N_DUP > 4096 and (big > 2 ** 32).sum() > 100
    above_zero = restated_vplot(cols, world["weights"]["zeros20"] != 0, centres, flip, groups, 4, *args, 0)[0]
    assert (above_zero < results["zeros20", 0][1]).sum() > 100 and (results["zeros20", 0][0] > 0).sum() > 100  # weight-0 fragments count
    with pytest.raises(L.FtkError, match="ftk_frags_set_weights"):
        engine.site_vplot("vp:bare", centres, flip, groups, 4, *args, weighted=True)


# ---- 6. empty inputs ---------------------------------------------------------------------------------------------------------
def test_empty_contig_no_sites_and_null_counts(engine, world):
    from finaletoolkit_amd import _lib as L
    z = np.zeros(0, np.int32)
    engine.load_contig("vp:empty", z, z, np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    try:
        for weighted in (False, True):
            if weighted:
                engine.set_weights("vp:empty", np.zeros(0, np.uint32))
            sums, counts = engine.site_vplot("vp:empty", [0, 500, (1 << 30) - 1], [0, 1, 0], [0, 2, 1], 3, 990, 15, 100, 399, 5, 0,
                                             weighted=weighted)
            assert sums.shape == counts.shape == (3, 60, 132) and not sums.any() and not counts.any()
    finally:
        engine.release("vp:empty")
    sums, counts = engine.site_vplot("vp:bare", [], None, None, 2, 1000, 1, 0, 9, 5)
    assert sums.shape == counts.shape == (2, 2, 2000) and sums.dtype == counts.dtype == np.int64
    assert not sums.any() and not counts.any()
    # count_out may be NULL; the outputs of a call with sites are overwritten, not added to
    c = np.array([LADDER_MID], np.int32)
    out = np.full(2 * 2, 7, np.int64)
    assert engine.lib.ftk_site_vplot(engine.ctx, engine.contig_id("vp:bare"), L.ptr(c), None, None, 1, 1, 1, 1, 100, 101, 1, 60, 0,
                                     L.ptr(out), None) == L.FTK_OK
    want = restated_vplot(world["cols"], None, c, None, None, 1, 1, 1, 100, 101, 1, 60)[0][0]
    assert out.tolist() == want.reshape(-1).tolist() and (want[:, 1] >= ONE).all()
    again = np.full(4, 7, np.int64)
    both = np.full(4, 7, np.int64)
    assert engine.lib.ftk_site_vplot(engine.ctx, engine.contig_id("vp:bare"), L.ptr(c), None, None, 1, 1, 1, 1, 100, 101, 1, 60, 0,
                                     L.ptr(again), L.ptr(both)) == L.FTK_OK
    assert again.tolist() == out.tolist() and (both * ONE).tolist() == out.tolist()


# ---- 7. the C ABI's argument errors ------------------------------------------------------------------------------------------
def test_argument_errors(engine, world):
    from finaletoolkit_amd import _lib as L
    lib, ctx, P = engine.lib, engine.ctx, L.ptr
    cid, bare = engine.contig_id("vp:plain"), engine.contig_id("vp:bare")
    engine.set_weights("vp:plain", world["weights"]["unit"])
    centre = np.array([100, 5_050, 7_050], np.int32)
    flip, group = np.array([0, 1, 0], np.uint8), np.array([0, 1, 1], np.int32)
    size = 2 * 4 * 4096
    sums, counts = np.full(size, 7, np.int64), np.full(size, 7, np.int64)
    INV, NOC = L.FTK_ERR_INVALID, L.FTK_ERR_NO_CONTIG

    def call(ctx_=ctx, cid_=cid, centre_=centre, flip_=flip, group_=group, n=3, ng=2, H=1000, b=1, lo=100, hi=199, lb=25, q=30, w=0,
             sums_=sums, counts_=counts):
        return lib.ftk_site_vplot(ctx_, cid_, P(centre_), P(flip_), P(group_), n, ng, H, b, lo, hi, lb, q, w, P(sums_), P(counts_))

    def failed(rc, code, word=None):
        assert rc == code, (rc, code)
        message = lib.ftk_last_error(ctx)
        assert message and (word is None or word in message), message

    assert call(ctx_=None) == INV
    failed(call(centre_=None), INV, b"centre")
    failed(call(sums_=None), INV, b"sum_out")
    for H in (0, -1, (1 << 20) + 1):
        failed(call(H=H, b=max(2 * H, 1)), INV, b"half_width")
    for b in (0, -15, 3, 2001):
        failed(call(b=b), INV, b"bin_size")
    failed(call(H=2049, b=1), INV, b"bins")           # 4098 bins
    failed(call(H=1 << 20, b=256), INV, b"bins")      # 8192 bins
    failed(call(lo=-1, hi=98), INV, b"len_lo")        # the order and the range of the length bounds
    failed(call(lo=200, hi=199), INV, b"len_hi")
    failed(call(lo=65_436, hi=65_536, lb=101), INV, b"len_hi")
    for lb in (0, -5, 3, 101):
        failed(call(lb=lb), INV, b"len_bin")
    failed(call(lo=0, hi=4096, lb=1), INV, b"rows")   # 4097 rows
    failed(call(lo=0, hi=65_535, lb=8), INV, b"rows")  # 8192 rows
    failed(call(ng=0), INV, b"n_groups")
    failed(call(ng=-3), INV, b"n_groups")
    failed(call(ng=(1 << 28) // 8000 + 1), INV, b"n_groups")   # n_groups * n_rows * n_bins > 2^28
    failed(call(centre_=np.array([100, -1, 7_050], np.int32)), INV, b"centre")
    failed(call(centre_=np.array([100, 1 << 30, 7_050], np.int32)), INV, b"centre")
    failed(call(group_=np.array([0, 2, 1], np.int32)), INV, b"group")
    failed(call(group_=np.array([0, -1, 1], np.int32)), INV, b"group")
    failed(call(cid_=bare, w=1), INV, b"ftk_frags_set_weights")    # the message names the weights calls
    assert b"ftk_frags_set_gc_weights" in lib.ftk_last_error(ctx)
    failed(call(n=-1), INV, b"n_sites")
    failed(call(cid_=987_654), NOC)
    failed(call(cid_=987_654, n=0), NOC)
    assert np.all(sums == 7) and np.all(counts == 7)  # nothing was written by any of them
    # and the same arguments, in range, succeed: the largest half-width, 4096 bins, the longest length, 4096 rows
    assert call(H=1 << 20, b=512) == L.FTK_OK and call(H=2048, b=1) == L.FTK_OK and call(w=1) == L.FTK_OK
    assert call(H=1, b=1, lo=65_436, hi=65_535, lb=100) == L.FTK_OK and call(H=1, b=1, lo=0, hi=4095, lb=1) == L.FTK_OK
    assert call(lo=199, hi=199, lb=1) == L.FTK_OK and call(lb=100) == L.FTK_OK
    assert not np.any(sums[: 2 * 2000] == 7)


# ---- 8. the product path -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def product(engine, tmp_path_factory):
    from finaletoolkit_amd import utils
    d = tmp_path_factory.mktemp("vplot")
    rng = np.random.default_rng(77)
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


def restated_product(p, table, lo, hi, lb, H, b, by_name, skip, mapq_min=30):
    """(groups, n_sites, units, count) of the site file from the fragment file's rows; ``table``: the weight table, or
    None for the uncorrected matrix; ``skip``: the contigs left out."""
    sites = [(c, (a + z) // 2, nm, st) for c, a, z, nm, st in p["rows"]]
    groups = list(dict.fromkeys(s[2] for s in sites)) if by_name else ["all"]
    shape = (len(groups), (hi - lo + 1) // lb, 2 * H // b)
    units, count, n_sites = np.zeros(shape, np.int64), np.zeros(shape, np.int64), np.zeros(len(groups), np.int64)
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
        got = restated_vplot(cols, w, [s[1] for s in mine], [s[3] == "-" for s in mine], g, len(groups), H, b, lo, hi, lb, mapq_min)
        units += got[0]
        count += got[1]
        n_sites += np.bincount(g, minlength=len(groups))
    return tuple(groups), n_sites, units, count


def same_vplot(a, b):
    return (a.groups == b.groups and np.array_equal(a.n_sites, b.n_sites) and np.array_equal(a.offsets, b.offsets)
            and np.array_equal(a.lengths, b.lengths) and np.array_equal(a.count, b.count) and np.array_equal(a.corrected, b.corrected)
            and a.skipped_contigs == b.skipped_contigs)


def run_vplot(*args, **kwargs):
    from finaletoolkit_amd import utils
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = utils.frag_vplot(*args, **kwargs)
    return res, [str(w.message) for w in caught if issubclass(w.category, UserWarning) and "frag_vplot" in str(w.message)]


def test_frag_vplot_end_to_end(engine, product, tmp_path):
    from finaletoolkit_amd import utils
    p = product
    lo, hi, lb, stride, H, b = 100, 199, 20, 3, 300, 50
    n_rows, n_bins = (hi - lo + 1) // lb, 2 * H // b
    kw = dict(min_length=lo, max_length=hi, length_bin=lb, half_width=H, bin_size=b)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        bias = utils.frag_gc_bias(p["frag"], p["ref"], str(tmp_path / "bias.tsv.gz"), min_length=lo, max_length=hi, stride=stride)
    table = utils.gc_weights(bias)
    # uncorrected: only wZ is skipped; corrected == count
    res, notes = run_vplot(p["frag"], p["bed"], **kw)
    groups, n_sites, units, count = restated_product(p, None, lo, hi, lb, H, b, False, {"wZ"})
    assert len(notes) == 1 and "wZ" in notes[0] and "not in the input" in notes[0]
    assert res.groups == ("all",) and res.skipped_contigs == ("wZ",) and res.n_sites.tolist() == [180] == n_sites.tolist()
    assert np.array_equal(res.count, count) and np.array_equal(res.corrected, count.astype(np.float64))
    assert res.count.dtype == np.int64 and res.n_sites.dtype == np.int64 and res.offsets.dtype == np.int64
    assert res.lengths.dtype == np.int64 and res.corrected.dtype == np.float64
    assert res.offsets.tolist() == list(range(-H, H, b)) and res.lengths.tolist() == list(range(lo, hi + 1, lb))
    assert res.count.shape == res.corrected.shape == (1, n_rows, n_bins)
    assert same_vplot(run_vplot(p["bam"], p["bedgz"], **kw)[0], res)
    # corrected, from the BAM and from the fragment file, the bias given three ways: wZ and wX are skipped
    results = {}
    for tag, path in (("bam", p["bam"]), ("frag", p["frag"])):
        for how, given in (("none", None), ("table", bias), ("tsv", str(tmp_path / "bias.tsv.gz"))):
            r, notes = run_vplot(path, p["bed"], reference_file=p["ref"], bias=given, by_name=True, stride=stride, **kw)
            assert len(notes) == 2 and "wZ" in notes[0] and "not in the input" in notes[0], notes
            assert "wX" in notes[1] and "not in the reference" in notes[1] and "wZ" not in notes[1], notes
            results[tag, how] = r
    res = results["frag", "none"]
    for k, other in results.items():
        assert same_vplot(res, other), k
    groups, n_sites, units, count = restated_product(p, table, lo, hi, lb, H, b, True, {"wZ", "wX"})
    first = list(dict.fromkeys(r[3] for r in p["rows"]))
    assert res.groups == groups == tuple(first) and set(groups) == {"CTCF", "GATA1", ".", "SPI1"}  # first-appearance order
    assert res.skipped_contigs == ("wZ", "wX") and np.array_equal(res.n_sites, n_sites) and n_sites.sum() == 120
    assert np.array_equal(res.count, count) and np.array_equal(res.corrected, units / 65536.0)
    # the cases bite: non-empty cells in every row, weights that are not all one, a - site among the sites
    assert (count.sum(axis=(0, 2)) > 0).all() and (count > 0).sum() >= 50 and not np.array_equal(units, count * ONE)
    assert any(r[4] == "-" and r[0] in ("wA", "wC") for r in p["rows"])
    # normalize: every group's matrix over its mean
    norm, _ = run_vplot(p["frag"], p["bed"], reference_file=p["ref"], bias=bias, by_name=True, normalize=True, **kw)
    assert np.array_equal(norm.count, res.count)
    for g in range(len(groups)):
        m = res.corrected[g]
        assert m.mean() > 0 and np.array_equal(norm.corrected[g], m / m.mean())
    # the files, field by field, and the command line in a child process
    for suffix in (".tsv", ".tsv.gz"):
        out = str(tmp_path / ("fn" + suffix))
        again, _ = run_vplot(p["frag"], p["bed"], out, reference_file=p["ref"], bias=bias, by_name=True, **kw)
        assert same_vplot(again, res)
        text = gzip.open(out, "rt").read() if suffix.endswith(".gz") else open(out).read()
        lines = text.splitlines()
        assert lines[0] == "#group\tn_sites\tlength\toffset\tcount\tcorrected" and len(lines) == 1 + len(groups) * n_rows * n_bins
        at = 1
        for g, name in enumerate(groups):
            for r in range(n_rows):
                for k in range(n_bins):
                    assert lines[at].split("\t") == [name, str(int(n_sites[g])), str(lo + r * lb), str(-H + k * b), str(int(count[g, r, k])),
                                                     format(units[g, r, k] / 65536.0, ".6f")], (g, r, k)
                    at += 1
        cli = str(tmp_path / ("cli" + suffix))
        r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.vplot", p["frag"], p["bed"], cli, "--reference", p["ref"],
                            "--bias", str(tmp_path / "bias.tsv.gz"), "--half-width", str(H), "--bin-size", str(b), "--min-length", str(lo),
                            "--max-length", str(hi), "--length-bin", str(lb), "-q", "30", "--by-name"], cwd=ROOT, capture_output=True,
                           text=True)
        assert r.returncode == 0, r.stderr
        assert "wX" in r.stderr and "wZ" in r.stderr  # the warnings
        if suffix == ".tsv":
            assert open(cli, "rb").read() == open(out, "rb").read()
        else:
            assert gzip.open(cli, "rb").read() == gzip.open(out, "rb").read()
