"""GPU: fragment-end profiles and OCF window sums (``csrc/ftk_siteends.hip``) - ``Engine.site_ends`` against the numpy
restatement of its rule in ``tests/site_ends_helpers.py``, exactly equal everywhere (sums and counts are integers): the
edges of the axis for either end, the widest weighted profile (both tracks in one workgroup, and one track per
workgroup), the per-site windows at each of their bounds and in the caller's order, site lists in any order, weights past
2^48, the ties to plain numpy counts, empty inputs, the C ABI's argument errors, and ``frag_ocf`` / the command line on a
synthetic BAM and its fragment file."""
import gzip
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests.gc_genome import LAYOUT, N_DUP, Contig, make_contig
from tests.helpers import read_frag_gz, write_2bit, write_synthetic_bam
from tests.site_ends_helpers import SIGN, assert_same, passing, restated_site_ends
from tests.vplot_helpers import DUP, EVEN, LAST_END, LONG, ODD, ONE, U32_MAX, vplot_contig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (1, 2), (990, 15), (2048, 1))
KEYS = ("se:plain", "se:bare", "se:bam")
U_EVEN, D_EVEN, U_ODD, D_ODD = EVEN[0], EVEN[1] - 1, ODD[0], ODD[1] - 1  # the bases the hand-placed fragments' ends are on
D_LONG = LONG[1] - 1


@pytest.fixture(scope="module")
def world(engine):
    import torch
    rng = np.random.default_rng(20261019)
    cols = vplot_contig(rng)
    n = len(cols[0])
    mapq = cols[2].astype(np.uint8)
    zeros = np.zeros(n, np.uint8)
    s32, e32 = cols[0].astype(np.int32), cols[1].astype(np.int32)
    engine.load_contig("se:plain", s32, e32, mapq, zeros)
    engine.load_contig("se:bare", s32, e32, mapq, zeros)  # never gets a weight column
    engine.load_contig("se:bam", s32, e32, mapq, zeros, cols[3].astype(np.int32), cols[4].astype(np.int32))
    is_dup = (cols[0] == DUP[0]) & (cols[1] == DUP[1])
    random = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    random[is_dup] = U32_MAX
    w = dict(cols=cols, n=n, n_cu=torch.cuda.get_device_properties(0).multi_processor_count, weights={
        "random": random,
        "zeros20": np.where(rng.random(n) < 0.2, 0, rng.integers(1, 2 ** 32, n, dtype=np.uint64)).astype(np.uint32),
        "unit": np.full(n, ONE, np.uint32),
    })
    assert is_dup.sum() == N_DUP and 7000 < n - N_DUP < 9000
    assert (LONG[0] >> 9) + 1 < (D_LONG >> 9)  # LONG starts more than a whole index bin before its D end
    yield w
    for key in KEYS:
        engine.release(key)


def without(cols, frag, w=None):
    """The contig (three columns) without every copy of the hand-placed fragment ``frag``, and ``w`` without their weights."""
    s, e = np.asarray(cols[0]), np.asarray(cols[1])
    mine = (s == frag[0]) & (e == frag[1])
    assert mine.sum() >= 1
    rest = tuple(np.asarray(c)[~mine] for c in cols[:3])
    return rest if w is None else (rest, np.asarray(w)[~mine])


# ---- 1. the edges of the axis ------------------------------------------------------------------------------------------------
def edge_sites(H):
    """Centres that put a bound of [c - H, c + H) on a hand-placed end, and the other edge cases; every centre once
    unflipped and once flipped.  Each site is a group of its own, so every one is compared on its own."""
    cs = []
    for x in (U_EVEN, D_EVEN, U_ODD, D_ODD):
        cs += [x + H, x - H + 1, x - H]  # the end on c - H, on c + H - 1, on c + H (out)
    cs += [0, (1 << 30) - 1, LAST_END + H, 100_000, D_LONG + H, D_LONG + H + 1, (DUP[0] + DUP[1]) >> 1]
    centres = np.array(cs + cs, np.int32)
    flip = np.array([0] * len(cs) + [1] * len(cs), np.uint8)
    return centres, flip, np.arange(len(centres), dtype=np.int32)


@pytest.mark.parametrize("H, b", SHAPES)
def test_edges_of_the_axis(engine, world, H, b):
    cols, w = world["cols"], world["weights"]["zeros20"]
    engine.set_weights("se:plain", w)
    centres, flip, groups = edge_sites(H)
    ng, half, nb = len(centres), len(centres) // 2, 2 * H // b
    at = {int(c): i for i, c in enumerate(centres[:half].tolist())}
    cnt = {}
    # open and closed length bounds on both sides of the hand-placed lengths (EVEN: 100, ODD: 101), MAPQ 29 | 30
    for mapq_min in (0, 30):
        for lens in ((None, None), (None, 99), (100, 100), (101, None), (100, 101), (102, 700)):
            want = restated_site_ends(cols, w, centres, flip, groups, ng, H, b, mapq_min, *lens)
            got = engine.site_ends("se:plain", centres, flip, groups, ng, H, b, mapq_min, *lens, weighted=True)
            assert_same(got, want, (H, b, mapq_min, lens))
            assert got[0].shape == (ng, 2, nb)
            cnt[mapq_min, lens] = want[1]
    # the cases are what they are meant to be.  What a hand-placed fragment adds: the restatement without it, subtracted
    all30 = cnt[30, (None, None)]
    # (of EVEN's two copies one passes MAPQ 30 - its twin has MAPQ 29 - and of ODD's both do: MAPQ 60 and 30)
    for frag, ux, dx, n in ((EVEN, U_EVEN, D_EVEN, 1), (ODD, U_ODD, D_ODD, 2)):
        extra = all30 - restated_site_ends(without(cols, frag), None, centres, flip, groups, ng, H, b, 30)[1]
        for x, track in ((ux, 0), (dx, 1)):  # on c - H the first bin, on c + H - 1 the last, on c + H out
            assert extra[at[x + H], track, 0] == n and extra[at[x + H], track].sum() == n
            assert extra[at[x - H + 1], track, -1] == n and extra[at[x - H + 1], track].sum() == n
            assert extra[at[x - H], track].sum() == 0
            # the flipped copy of the site: the other track, the bins counted from the other end
            assert extra[half + at[x + H], 1 - track, -1] == n and extra[half + at[x + H], 1 - track].sum() == n
    assert (cnt[0, (None, None)] - all30)[at[U_EVEN + H], 0, 0] >= 1 and (cnt[0, (None, None)] - all30)[at[D_EVEN + H], 1, 0] >= 1  # the MAPQ-29 twin
    lens_of = {k[1]: v for k, v in cnt.items() if k[0] == 30}
    assert np.array_equal(lens_of[None, 99] + lens_of[100, 100] + lens_of[101, None], all30)
    assert np.array_equal(lens_of[None, 99] + lens_of[100, 101] + lens_of[102, 700], all30)  # (700: the longest fragment)
    assert lens_of[100, 100][at[U_EVEN + H], 0, 0] >= 1 and lens_of[101, None][at[U_ODD + H], 0, 0] >= 1
    assert lens_of[100, 100][at[U_EVEN + H], 0, 0] < lens_of[100, 101][at[U_EVEN + H], 0, 0] + 1
    # the fragment (0, 1) of length 1: both of its ends on base 0, the same bin of both tracks
    one = all30 - restated_site_ends(without(cols, (0, 1)), None, centres, flip, groups, ng, H, b, 30)[1]
    assert one[at[0]].sum() == 2 and one[at[0], 0, H // b] == 1 and one[at[0], 1, H // b] == 1
    assert not all30[at[100_000]].any() and not all30[at[(1 << 30) - 1]].any() and not all30[at[LAST_END + H]].any()
    # flipped against unflipped: the bins reversed AND the tracks swapped - not the bins reversed alone
    assert np.array_equal(all30[:half], all30[half:, ::-1, ::-1])
    assert not np.array_equal(all30[:half], all30[half:, :, ::-1])
    # LONG alone (one site): its D end lies on c - H, so it counts in track 1, bin 0, while its start lies more than a
    # whole index bin to the left of the window; one base further it is out.  (Against the restatement without it.)
    rest, w_rest = without(cols, LONG, w)
    for c, inside in ((D_LONG + H, 1), (D_LONG + H + 1, 0)):
        got = engine.site_ends("se:plain", [c], None, None, 1, H, b, 0, weighted=True)
        assert_same(got, restated_site_ends(cols, w, [c], None, None, 1, H, b, 0), ("long", c))
        extra = got[1] - restated_site_ends(rest, w_rest, [c], None, None, 1, H, b, 0)[1]
        assert extra.sum() == inside and extra[0, 1, 0] == inside, c


# ---- 2. the largest LDS case -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [None, "0", "1"])
def test_widest_weighted_profile(engine, world, split, monkeypatch):
    """4096 bins x two tracks x 12 bytes = 96 KiB of LDS.  ``FTK_SITE_ENDS_SPLIT=0``: both tracks in one workgroup, with
    the kernel's dynamic-LDS limit raised (where the device has the room); ``=1``: one workgroup per track; unset: the
    library's own choice between the two."""
    if split is None:
        monkeypatch.delenv("FTK_SITE_ENDS_SPLIT", raising=False)
    else:
        monkeypatch.setenv("FTK_SITE_ENDS_SPLIT", split)
    cols, w = world["cols"], world["weights"]["random"]
    engine.set_weights("se:plain", w)
    H, b = 2048, 1
    rng = np.random.default_rng(2)
    # a U end and a D end in the first and in the last bin of their tracks, both as they are and flipped; random sites
    centres = np.concatenate([[U_EVEN + H, U_EVEN - H + 1, D_EVEN + H, D_EVEN - H + 1] * 2, [1_075], rng.integers(0, 41_000, 40)])
    centres = centres.astype(np.int32)
    flip = np.concatenate([[0] * 4 + [1] * 4, rng.integers(0, 2, 41)]).astype(np.uint8)
    groups = np.concatenate([[0] * 4 + [1] * 4, rng.integers(0, 2, 41)]).astype(np.int32)
    for mapq_min in (0, 30):
        want = restated_site_ends(cols, w, centres, flip, groups, 2, H, b, mapq_min, peak=60, flank=10)
        assert_same(engine.site_ends("se:plain", centres, flip, groups, 2, H, b, mapq_min, weighted=True, peak=60, flank=10), want,
                    (mapq_min, "sites"))
        assert_same(engine.site_ends("se:plain", centres, flip, groups, 2, H, b, mapq_min, weighted=True), want[:2], mapq_min)
        bare = engine.site_ends("se:bare", centres, flip, groups, 2, H, b, mapq_min, peak=2037, flank=10)
        assert np.array_equal(bare[1], want[1]) and np.array_equal(bare[0], ONE * want[1])
        assert_same(bare[2:], restated_site_ends(cols, None, centres, flip, groups, 2, H, b, mapq_min, peak=2037, flank=10)[2:], "bare")
    corners = want[1][:, :, [0, -1]]
    assert (corners > 0).all(), corners.tolist()  # first and last bin of both tracks of both groups
    assert want[0].max() >= N_DUP * U32_MAX > 2 ** 48 and want[2].max() > 2 ** 32


# ---- 3. per-site sums --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H, b, p, w", [(990, 15, 60, 10), (990, 15, 1, 0), (990, 15, 979, 10), (2, 1, 1, 0), (80, 1, 60, 10)])
def test_per_site_window_bounds(engine, world, H, b, p, w):
    cols, wt = world["cols"], world["weights"]["zeros20"]
    engine.set_weights("se:plain", wt)
    assert 0 <= w < p and p + w < H
    ds = [-p - w, -p + w, -p + w + 1, p - w - 1, p - w, p + w]  # in, in, out | out, in, in
    inside = {0: [1, 1, 0, 0, 0, 0], 2: [0, 0, 0, 0, 1, 1]}     # per column (left, right) of the end's own kind
    centres = np.array([U_EVEN - d for d in ds] + [D_ODD - d for d in ds], np.int32)
    centres = np.concatenate([centres, centres])
    flip = np.repeat([0, 1], 12).astype(np.uint8)
    groups = (np.arange(24) % 3).astype(np.int32)
    for weighted in (False, True):
        want = restated_site_ends(cols, wt if weighted else None, centres, flip, groups, 3, H, b, 30, peak=p, flank=w)
        got = engine.site_ends("se:plain", centres, flip, groups, 3, H, b, 30, weighted=weighted, peak=p, flank=w)
        assert_same(got, want, (H, b, p, w, weighted))
        assert_same(engine.site_ends("se:plain", centres, flip, groups, 3, H, b, 30, weighted=weighted), want[:2], "no per-site sums")
    # one-count differences: what EVEN's U end and ODD's D end add at each placement
    cnt = want[3]
    no_even = restated_site_ends(without(cols, EVEN), None, centres, flip, groups, 3, H, b, 30, peak=p, flank=w)[3]
    no_odd = restated_site_ends(without(cols, ODD), None, centres, flip, groups, 3, H, b, 30, peak=p, flank=w)[3]
    for col, ins in inside.items():  # (ODD has two copies that pass: MAPQ 60 and 30)
        assert (cnt - no_even)[:6, col].tolist() == ins and (cnt - no_even)[12:18, col].tolist() == ins, (col, "U")
        twice = [2 * x for x in ins]
        assert (cnt - no_odd)[6:12, col + 1].tolist() == twice and (cnt - no_odd)[18:, col + 1].tolist() == twice, (col, "D")
    # a site and its flipped copy: the same four sums (genome orientation), so the same OCF
    assert np.array_equal(got[2][:12], got[2][12:]) and np.array_equal(got[3][:12], got[3][12:])
    assert np.array_equal((got[2][:12] * SIGN).sum(axis=1), (got[2][12:] * SIGN).sum(axis=1))


def test_per_site_rows_and_profile_slices(engine, world):
    cols, wt = world["cols"], world["weights"]["random"]
    engine.set_weights("se:plain", wt)
    H, p, w = 200, 60, 10
    rng = np.random.default_rng(33)
    # rows in the caller's order: unsorted, with repeats, groups and flips mixed
    centres = np.array([20_000, 1_060, 39_000, 1_060, 0, 20_000, 5_050, 1_060, 7_100, (1 << 30) - 1, 36_000], np.int32)  # (DUP's U ends: 60 left of 1 060)
    flip = (np.arange(len(centres)) % 3 == 0).astype(np.uint8)
    groups = np.array([2, 0, 1, 1, 0, 2, 2, 0, 1, 0, 2], np.int32)
    want = restated_site_ends(cols, wt, centres, flip, groups, 3, H, 8, 30, peak=p, flank=w)
    got = engine.site_ends("se:plain", centres, flip, groups, 3, H, 8, 30, weighted=True, peak=p, flank=w)
    assert_same(got, want, "order")
    assert np.array_equal(got[3][1], got[3][3]) and np.array_equal(got[3][1], got[3][7]) and np.array_equal(got[3][0], got[3][5])
    assert len({tuple(r) for r in got[3].tolist()}) >= 6 and got[3][1].sum() > N_DUP and not got[3][9].any()
    # no site flipped, b = 1, one site per group: the four sums are slices of the group's own profile
    centres = np.concatenate([[1_075, 5_050, 7_050], rng.integers(0, 41_000, 60)]).astype(np.int32)
    ng = len(centres)
    sums, counts, ssum, scnt = engine.site_ends("se:plain", centres, None, np.arange(ng, dtype=np.int32), ng, H, 1, 30, weighted=True,
                                                peak=p, flank=w)
    left, right = slice(H - p - w, H - p + w + 1), slice(H + p - w, H + p + w + 1)
    for arr, site in ((sums, ssum), (counts, scnt)):
        sliced = np.stack([arr[:, 0, left].sum(axis=1), arr[:, 1, left].sum(axis=1), arr[:, 0, right].sum(axis=1),
                           arr[:, 1, right].sum(axis=1)], axis=1)
        assert np.array_equal(sliced, site)
    assert scnt.sum() > 200 and (scnt > 0).sum() > 100  # (the windows hold something)
    # several sites per group: the group-summed sites are the slices of the group's profile
    g3 = rng.integers(0, 3, ng).astype(np.int32)
    sums, counts, ssum, scnt = engine.site_ends("se:plain", centres, None, g3, 3, H, 1, 30, weighted=True, peak=p, flank=w)
    for arr, site in ((sums, ssum), (counts, scnt)):
        by_group = np.zeros((3, 4), np.int64)
        np.add.at(by_group, g3, site)
        sliced = np.stack([arr[:, 0, left].sum(axis=1), arr[:, 1, left].sum(axis=1), arr[:, 0, right].sum(axis=1),
                           arr[:, 1, right].sum(axis=1)], axis=1)
        assert np.array_equal(sliced, by_group)
    assert_same(engine.site_ends("se:plain", centres, None, g3, 3, H, 1, 30, weighted=True), (sums, counts), "site_sum_out NULL")


# ---- 4. site lists -----------------------------------------------------------------------------------------------------------
def site_lists(rng, n_cu):
    """The six lists of the V-plot test."""
    r = lambda n: rng.integers(0, 42_000, n).astype(np.int32)  # noqa: E731
    many = 4 * n_cu + 3
    return {
        "unsorted": (np.array([20_000, 500, 39_000, 900, 0, 20_001, 950, 5_050], np.int32), np.array([0, 1, 0, 1, 1, 0, 0, 1], np.uint8),
                     np.array([1, 0, 1, 0, 2, 1, 0, 2], np.int32), 3),
        "twice": (np.array([7_050, 1_075, 7_050, 7_050, 1_075], np.int32), np.array([0, 0, 0, 1, 0], np.uint8),
                  np.array([0, 0, 0, 0, 1], np.int32), 2),
        "empty_group": (r(50), None, rng.choice([0, 2, 4], 50).astype(np.int32), 6),  # groups 1, 3 and 5 have no site
        "many_groups": (r(many), rng.integers(0, 2, many).astype(np.uint8), rng.permutation(many).astype(np.int32), many),
        # one group of more than twelve sites per compute unit: several runs flush into one group's tracks
        "big_group": (r(14 * n_cu + 5), rng.integers(0, 2, 14 * n_cu + 5).astype(np.uint8),
                      (rng.random(14 * n_cu + 5) < 0.95).astype(np.int32), 2),
        "no_flip_no_groups": (r(300), None, None, 1),
    }


def test_site_lists(engine, world):
    rng = np.random.default_rng(4)
    cols, w = world["cols"], world["weights"]["zeros20"]
    engine.set_weights("se:plain", w)
    lists = site_lists(rng, world["n_cu"])
    H, b = 990, 15
    cnt = {}
    for name, (centres, flip, groups, ng) in lists.items():
        want = restated_site_ends(cols, w, centres, flip, groups, ng, H, b, 30, 50, 350, peak=60, flank=10)
        got = engine.site_ends("se:plain", centres, flip, groups, ng, H, b, 30, 50, 350, weighted=True, peak=60, flank=10)
        assert_same(got, want, name)
        plain = engine.site_ends("se:bare", centres, flip, groups, ng, H, b, 30, 50, 350)
        assert np.array_equal(plain[1], want[1]) and np.array_equal(plain[0], ONE * want[1]), name
        cnt[name] = want[1]
    # the lists are what they are meant to be
    assert len(lists["many_groups"][0]) > 4 * world["n_cu"] and np.bincount(lists["big_group"][2])[1] > 12 * world["n_cu"]
    assert cnt["empty_group"][[1, 3, 5]].sum() == 0 and all(cnt["empty_group"][g].any() for g in (0, 2, 4))
    one = restated_site_ends(cols, None, [7_050], None, None, 1, H, b, 30, 50, 350)[1][0]
    dup = restated_site_ends(cols, None, [1_075], None, None, 1, H, b, 30, 50, 350)[1][0]
    assert np.array_equal(cnt["twice"][0], 2 * one + one[::-1, ::-1] + dup) and np.array_equal(cnt["twice"][1], dup)
    assert (cnt["many_groups"].sum(axis=(1, 2)) > 0).sum() > 0.8 * len(lists["many_groups"][0])


def test_more_runs_than_one_split_launch_holds(engine, world, monkeypatch):
    """More than 2^19 runs (one group per site) of two workgroups each (``FTK_SITE_ENDS_SPLIT=1``): a launch takes 2^19
    runs, not the 2^20 of an unsplit one, and the call splits its launches.  One bin, so the restatement is two
    bisections per site and end on the sorted ends and a running sum of the weights - as the helper's per-site rows are."""
    monkeypatch.setenv("FTK_SITE_ENDS_SPLIT", "1")
    rng = np.random.default_rng(21)
    n = (1 << 19) + 37
    centres = rng.integers(2_500, 42_000, n).astype(np.int32)  # (clear of the copies: 10^5 sites on them would take seconds)
    centres[:3] = (1_075, U_EVEN, D_LONG)
    groups = rng.permutation(n).astype(np.int32)
    flip = rng.integers(0, 2, n).astype(np.uint8)
    cols, w = world["cols"], world["weights"]["zeros20"]
    engine.set_weights("se:plain", w)
    H, peak, flank = 300, 60, 10
    s, e = (np.asarray(cols[k], np.int64) for k in range(2))
    keep = passing(cols, 30, 120, 180)
    c = centres.astype(np.int64)
    want = [np.zeros((n, 2, 1), np.int64), np.zeros((n, 2, 1), np.int64), np.zeros((n, 4), np.int64), np.zeros((n, 4), np.int64)]
    for kind, x in enumerate((s[keep], e[keep] - 1)):  # 0: the U ends, 1: the D ends
        o = np.argsort(x, kind="stable")
        x, run = x[o], np.concatenate([[0], np.cumsum(w.astype(np.int64)[keep][o])])
        lo, hi = np.searchsorted(x, c - H, "left"), np.searchsorted(x, c + H, "left")
        track = kind ^ flip  # a flipped site's ends count in the other track (and in the same, only, bin)
        want[0][groups, track, 0], want[1][groups, track, 0] = run[hi] - run[lo], hi - lo
        for side, mid in enumerate((c - peak, c + peak)):  # genome orientation: no flip; closed on both sides
            lo, hi = np.searchsorted(x, mid - flank, "left"), np.searchsorted(x, mid + flank, "right")
            want[2][:, 2 * side + kind], want[3][:, 2 * side + kind] = run[hi] - run[lo], hi - lo
    got = engine.site_ends("se:plain", centres, flip, groups, n, H, 2 * H, 30, 120, 180, weighted=True, peak=peak, flank=flank)
    assert_same(got, tuple(want), "split launches")
    assert want[1][groups[0]].sum() >= 2 * N_DUP and (want[1][1 << 19:] > 0).any()  # groups of the second launch count
    assert (want[3][groups >= 1 << 19] > 0).any()  # and so do rows of its sites


# ---- 5. weights --------------------------------------------------------------------------------------------------------------
def test_weights(engine, world):
    from finaletoolkit_amd import _lib as L
    cols = world["cols"]
    rng = np.random.default_rng(5)
    centres = np.concatenate([[1_075, 1_000, 5_050], rng.integers(0, 41_000, 200)]).astype(np.int32)
    flip = rng.integers(0, 2, len(centres)).astype(np.uint8)
    groups = rng.integers(0, 4, len(centres)).astype(np.int32)
    groups[:2] = 3
    args = (990, 15)
    results = {}
    for tag, w in world["weights"].items():
        engine.set_weights("se:plain", w)
        for mapq_min in (0, 30):
            want = restated_site_ends(cols, w, centres, flip, groups, 4, *args, mapq_min, peak=75, flank=10)
            got = engine.site_ends("se:plain", centres, flip, groups, 4, *args, mapq_min, weighted=True, peak=75, flank=10)
            assert_same(got, want, (tag, mapq_min))
            results[tag, mapq_min] = got
            if tag == "unit":
                assert np.array_equal(got[0], ONE * got[1]) and np.array_equal(got[2], ONE * got[3])
                for key in ("se:plain", "se:bare"):  # weighted=False: the same numbers, with a column attached and without one
                    assert_same(engine.site_ends(key, centres, flip, groups, 4, *args, mapq_min, weighted=False, peak=75, flank=10), got,
                                (key, "unweighted"))
    big, n_big, site_big, site_n = results["random", 0]
    assert big.max() >= N_DUP * U32_MAX > 2 ** 48 and n_big.max() >= N_DUP > 4096 and (big > 2 ** 32).sum() > 100
    assert site_big.max() >= N_DUP * U32_MAX and site_n.max() >= N_DUP  # DUP's U ends lie 75 left of the site on 1 075
    above_zero = restated_site_ends(cols, world["weights"]["zeros20"] != 0, centres, flip, groups, 4, *args, 0)[0]
    assert (above_zero < results["zeros20", 0][1]).sum() > 100 and (results["zeros20", 0][0] > 0).sum() > 100  # weight-0 fragments count
    with pytest.raises(L.FtkError, match="ftk_frags_set_weights.*ftk_frags_set_gc_weights|ftk_frags_set_gc_weights.*ftk_frags_set_weights"):
        engine.site_ends("se:bare", centres, flip, groups, 4, *args, weighted=True)


# ---- 6. ties -----------------------------------------------------------------------------------------------------------------
def test_ties(engine, world):
    cols = world["cols"]
    assert engine.is_bam("se:bam") and not engine.is_bam("se:plain")
    rng = np.random.default_rng(6)
    centres = np.concatenate([[1_075, 5_050, 36_050], rng.integers(0, 41_000, 300)]).astype(np.int32)
    flip, groups = rng.integers(0, 2, len(centres)).astype(np.uint8), rng.integers(0, 3, len(centres)).astype(np.int32)
    for key in ("se:plain", "se:bam"):
        engine.set_weights(key, world["weights"]["random"])
    for weighted in (False, True):  # the read1 columns play no part
        assert_same(engine.site_ends("se:bam", centres, flip, groups, 3, 990, 15, 30, 50, 350, weighted=weighted, peak=60, flank=10),
                    engine.site_ends("se:plain", centres, flip, groups, 3, 990, 15, 30, 50, 350, weighted=weighted, peak=60, flank=10),
                    weighted)
    # b = 2 H: the one bin of a track is the number of passing fragments with that end inside [c - H, c + H)
    keep = passing(cols, 30, 50, 350)
    s, d_end = np.asarray(cols[0])[keep], np.asarray(cols[1])[keep] - 1
    ng = len(centres)
    for H in (1, 990, 1 << 20):
        counts = engine.site_ends("se:plain", centres, None, np.arange(ng, dtype=np.int32), ng, H, 2 * H, 30, 50, 350)[1]
        c = centres.astype(np.int64)[:, None]
        assert np.array_equal(counts[:, 0, 0], ((s[None] >= c - H) & (s[None] < c + H)).sum(axis=1))
        assert np.array_equal(counts[:, 1, 0], ((d_end[None] >= c - H) & (d_end[None] < c + H)).sum(axis=1))
        assert counts.shape == (ng, 2, 1) and counts.sum() > 0


# ---- 7. empty inputs ---------------------------------------------------------------------------------------------------------
def test_empty_contig_no_sites_and_null_outputs(engine, world):
    from finaletoolkit_amd import _lib as L
    z = np.zeros(0, np.int32)
    engine.load_contig("se:empty", z, z, np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    try:
        for weighted in (False, True):
            if weighted:
                engine.set_weights("se:empty", np.zeros(0, np.uint32))
            out = engine.site_ends("se:empty", [0, 500, (1 << 30) - 1], [0, 1, 0], [0, 2, 1], 3, 990, 15, 0, weighted=weighted, peak=60)
            assert out[0].shape == out[1].shape == (3, 2, 132) and out[2].shape == out[3].shape == (3, 4)
            assert not any(o.any() for o in out)
        # outputs prefilled with 7 are overwritten with the zeros
        c = np.array([5, 9], np.int32)
        outs = [np.full(2 * 4, 7, np.int64) for _ in range(4)]
        assert engine.lib.ftk_site_ends(engine.ctx, engine.contig_id("se:empty"), L.ptr(c), None, None, 2, 1, 2, 1, 0, -1, -1, 0, 1, 0,
                                        *(L.ptr(o) for o in outs)) == L.FTK_OK
        assert not any(o.any() for o in outs)
    finally:
        engine.release("se:empty")
    out = engine.site_ends("se:bare", [], None, None, 2, 1000, 1, peak=60)
    assert out[0].shape == out[1].shape == (2, 2, 2000) and out[2].shape == out[3].shape == (0, 4)
    assert all(o.dtype == np.int64 and not o.any() for o in out)
    # count_out and site_count_out may be NULL; the outputs of a call with sites are overwritten, not added to
    c = np.array([U_EVEN, D_ODD + 1], np.int32)
    want = restated_site_ends(world["cols"], None, c, None, None, 1, 2, 1, 60, peak=1, flank=0)
    cid = engine.contig_id("se:bare")
    sums, ssum = np.full(8, 7, np.int64), np.full(8, 7, np.int64)
    assert engine.lib.ftk_site_ends(engine.ctx, cid, L.ptr(c), None, None, 2, 1, 2, 1, 60, -1, -1, 0, 1, 0, L.ptr(sums), None, L.ptr(ssum),
                                    None) == L.FTK_OK
    assert sums.tolist() == want[0].reshape(-1).tolist() and ssum.tolist() == want[2].reshape(-1).tolist()
    assert want[0][0, 0, 2] >= ONE and want[2][1, 1] >= ONE  # EVEN's U end on the first centre, ODD's D end one left of the second
    again = [np.full(8, 7, np.int64) for _ in range(4)]
    assert engine.lib.ftk_site_ends(engine.ctx, cid, L.ptr(c), None, None, 2, 1, 2, 1, 60, -1, -1, 0, 1, 0,
                                    *(L.ptr(o) for o in again)) == L.FTK_OK
    assert again[0].tolist() == sums.tolist() and (again[1] * ONE).tolist() == sums.tolist()
    assert again[2].tolist() == ssum.tolist() and (again[3] * ONE).tolist() == ssum.tolist()
    # site_count_out without site_sum_out: ignored, with peak and flank
    only = np.full(8, 7, np.int64)
    assert engine.lib.ftk_site_ends(engine.ctx, cid, L.ptr(c), None, None, 2, 1, 2, 1, 60, -1, -1, 0, -5, 99, L.ptr(again[0]), None, None,
                                    L.ptr(only)) == L.FTK_OK
    assert again[0].tolist() == sums.tolist() and np.all(only == 7)


# ---- 8. the C ABI's argument errors ------------------------------------------------------------------------------------------
def test_argument_errors(engine, world):
    from finaletoolkit_amd import _lib as L
    lib, ctx, P = engine.lib, engine.ctx, L.ptr
    cid, bare = engine.contig_id("se:plain"), engine.contig_id("se:bare")
    engine.set_weights("se:plain", world["weights"]["unit"])
    centre = np.array([100, 5_050, 7_050], np.int32)
    flip, group = np.array([0, 1, 0], np.uint8), np.array([0, 1, 1], np.int32)
    size = 2 * 2 * 4096
    sums, counts = np.full(size, 7, np.int64), np.full(size, 7, np.int64)
    ssum, scnt = np.full(12, 7, np.int64), np.full(12, 7, np.int64)
    INV, NOC = L.FTK_ERR_INVALID, L.FTK_ERR_NO_CONTIG

    def call(ctx_=ctx, cid_=cid, centre_=centre, flip_=flip, group_=group, n=3, ng=2, H=1000, b=1, q=30, lo=-1, hi=-1, w=0, p=60, f=10,
             sums_=sums, counts_=counts, ssum_=ssum, scnt_=scnt):
        return lib.ftk_site_ends(ctx_, cid_, P(centre_), P(flip_), P(group_), n, ng, H, b, q, lo, hi, w, p, f, P(sums_), P(counts_),
                                 P(ssum_), P(scnt_))

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
    failed(call(ng=0), INV, b"n_groups")
    failed(call(ng=-3), INV, b"n_groups")
    failed(call(ng=(1 << 28) // 4000 + 1), INV, b"n_groups")   # n_groups * 2 * n_bins > 2^28
    failed(call(H=2048, ng=(1 << 15) + 1), INV, b"n_groups")
    for p, f in ((0, 0), (-1, 0), (0, -1)):
        failed(call(p=p, f=f), INV, b"peak")
    for p, f in ((60, 60), (60, 61), (60, -1), (1, 1)):
        failed(call(p=p, f=f), INV, b"flank")
    failed(call(p=990, f=10), INV, b"peak + flank")            # peak + flank == H
    failed(call(H=70, p=60, f=10), INV, b"peak + flank")
    failed(call(H=1, p=1, f=0), INV, b"peak + flank")
    failed(call(centre_=np.array([100, -1, 7_050], np.int32)), INV, b"centre")
    failed(call(centre_=np.array([100, 1 << 30, 7_050], np.int32)), INV, b"centre")
    failed(call(group_=np.array([0, 2, 1], np.int32)), INV, b"group")
    failed(call(group_=np.array([0, -1, 1], np.int32)), INV, b"group")
    failed(call(cid_=bare, w=1), INV, b"ftk_frags_set_weights")    # the message names the weights calls
    assert b"ftk_frags_set_gc_weights" in lib.ftk_last_error(ctx)
    failed(call(n=-1), INV, b"n_sites")
    import torch
    on_device = torch.tensor(centre, device="cuda")
    failed(call(centre_=on_device), INV, b"host arrays")           # the sites are host arrays
    failed(call(group_=torch.tensor(group, device="cuda")), INV, b"host arrays")
    failed(call(cid_=987_654), NOC)
    failed(call(cid_=987_654, n=0), NOC)
    assert all(np.all(o == 7) for o in (sums, counts, ssum, scnt))  # nothing was written by any of them
    # and the same arguments, in range, succeed: the largest half-width, 4096 bins, the most cells, the windows at their bounds
    assert call(H=1 << 20, b=512) == L.FTK_OK and call(H=2048, b=1) == L.FTK_OK and call(w=1) == L.FTK_OK
    assert call(p=989, f=10) == L.FTK_OK and call(H=71, p=60, f=10) == L.FTK_OK and call(H=2, p=1, f=0) == L.FTK_OK
    assert call(p=60, f=59) == L.FTK_OK and call(p=1, f=0) == L.FTK_OK
    assert not np.any(sums[: 2 * 2 * 2000] == 7) and not np.any(ssum == 7) and not np.any(scnt == 7)
    # without site_sum_out the same bad windows are accepted: peak and flank are ignored
    for p, f in ((0, 0), (-1, 0), (60, 60), (990, 10), (60, -1)):
        assert call(p=p, f=f, ssum_=None, scnt_=None) == L.FTK_OK, (p, f)
    most = np.zeros(1 << 28, np.int64)  # n_groups * 2 * n_bins == 2^28, no sites
    assert call(n=0, H=2048, ng=1 << 15, sums_=most, counts_=None, ssum_=None, scnt_=None) == L.FTK_OK


# ---- 9. the product path -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def product(engine, tmp_path_factory):
    """The synthetic two-contig BAM, its fragment file, the 2bit and the sites of the V-plot test's product path."""
    from finaletoolkit_amd import utils
    d = tmp_path_factory.mktemp("ocf")
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
    order = rng.permutation(len(rows))  # the contigs' sites interleaved: per-site results have to find their way back
    rows = [rows[i] for i in order]
    bed = str(d / "sites.bed")
    with open(bed, "w") as fh:
        fh.write("# sites\n" + "".join(f"{c}\t{a}\t{b}\t{nm}\t0\t{st}\n" for c, a, b, nm, st in rows))
    bedgz = str(d / "sites.bed.gz")
    with gzip.open(bedgz, "wt") as fh:
        fh.write(open(bed).read())
    return dict(dir=d, ref=ref, bam=bam, frag=frag, bed=bed, bedgz=bedgz, rows=rows, cols=read_frag_gz(frag),
                contigs={name: Contig(name, s) for name, s in seqs.items()})


def restated_product(p, table, lo, hi, H, b, peak, flank, by_name, skip, mapq_min=30):
    """(groups, n_sites, units, count, site_units, site_count, seen) of the site file from the fragment file's rows;
    ``table``: the weight table, or None for the uncorrected profile; ``skip``: the contigs left out."""
    sites = [(c, (a + z) // 2, nm, st) for c, a, z, nm, st in p["rows"]]
    groups = list(dict.fromkeys(s[2] for s in sites)) if by_name else ["all"]
    shape = (len(groups), 2, 2 * H // b)
    units, count, n_sites = np.zeros(shape, np.int64), np.zeros(shape, np.int64), np.zeros(len(groups), np.int64)
    site_units, site_count, seen = np.zeros((len(sites), 4), np.int64), np.zeros((len(sites), 4), np.int64), np.zeros(len(sites), bool)
    for c in dict.fromkeys(s[0] for s in sites):
        if c in skip:
            continue
        idx = [i for i, s in enumerate(sites) if s[0] == c]
        mine = [sites[i] for i in idx]
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
        got = restated_site_ends(cols, w, [s[1] for s in mine], [s[3] == "-" for s in mine], g, len(groups), H, b, mapq_min, lo, hi,
                                 peak=peak, flank=flank)
        units += got[0]
        count += got[1]
        site_units[idx], site_count[idx], seen[idx] = got[2], got[3], True
        n_sites += np.bincount(g, minlength=len(groups))
    return tuple(groups), n_sites, units, count, site_units, site_count, seen


def same_ocf(a, b):
    return (a.groups == b.groups and a.skipped_contigs == b.skipped_contigs
            and all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=(f == "site_ocf")) for f in a._fields
                    if f not in ("groups", "skipped_contigs")))


def run_ocf(*args, **kwargs):
    from finaletoolkit_amd import utils
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = utils.frag_ocf(*args, **kwargs)
    return res, [str(w.message) for w in caught if issubclass(w.category, UserWarning) and "frag_ocf" in str(w.message)]


def read_text(path):
    return gzip.open(path, "rt").read() if path.endswith(".gz") else open(path).read()


def test_frag_ocf_end_to_end(engine, product, tmp_path):
    from finaletoolkit_amd import utils
    p = product
    lo, hi, stride, H, b, peak, flank = 100, 199, 3, 300, 50, 60, 10
    n_bins = 2 * H // b
    kw = dict(min_length=lo, max_length=hi, half_width=H, bin_size=b, peak=peak, flank=flank)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        bias = utils.frag_gc_bias(p["frag"], p["ref"], str(tmp_path / "bias.tsv.gz"), min_length=lo, max_length=hi, stride=stride)
    table = utils.gc_weights(bias)
    site_contig = np.array([r[0] for r in p["rows"]])
    # uncorrected: only wZ is skipped; corrected == count, ocf == ocf_count, the sites of wZ are NaN
    res, notes = run_ocf(p["frag"], p["bed"], **kw)
    groups, n_sites, units, count, site_units, site_count, seen = restated_product(p, None, lo, hi, H, b, peak, flank, False, {"wZ"})
    assert len(notes) == 1 and "wZ" in notes[0] and "not in the input" in notes[0]
    assert res.groups == ("all",) and res.skipped_contigs == ("wZ",) and res.n_sites.tolist() == [180] == n_sites.tolist()
    assert np.array_equal(res.up_count, count[:, 0]) and np.array_equal(res.down_count, count[:, 1])
    assert np.array_equal(res.up_corrected, count[:, 0].astype(np.float64)) and np.array_equal(res.down_corrected, count[:, 1].astype(np.float64))
    assert np.array_equal(res.windows_count, site_count[seen].sum(axis=0)[None])
    assert np.array_equal(res.ocf_count, (res.windows_count * SIGN).sum(axis=1)) and np.array_equal(res.ocf, res.ocf_count.astype(np.float64))
    assert np.array_equal(np.isnan(res.site_ocf), site_contig == "wZ") and np.array_equal(~seen, site_contig == "wZ")
    assert np.array_equal(res.site_ocf[seen], (site_count[seen] * SIGN).sum(axis=1).astype(np.float64))
    for f in ("n_sites", "offsets", "up_count", "down_count", "windows_count", "ocf_count"):
        assert getattr(res, f).dtype == np.int64, f
    for f in ("up_corrected", "down_corrected", "ocf", "site_ocf"):
        assert getattr(res, f).dtype == np.float64, f
    assert res.offsets.tolist() == list(range(-H, H, b)) and res.up_count.shape == res.down_corrected.shape == (1, n_bins)
    assert res.site_ocf.shape == (len(p["rows"]),) and res.windows_count.shape == (1, 4)
    assert same_ocf(run_ocf(p["bam"], p["bedgz"], **kw)[0], res)
    # corrected, from the BAM and from the fragment file, the bias given three ways: wZ and wX are skipped
    results = {}
    for tag, path in (("bam", p["bam"]), ("frag", p["frag"])):
        for how, given in (("none", None), ("table", bias), ("tsv", str(tmp_path / "bias.tsv.gz"))):
            r, notes = run_ocf(path, p["bed"], reference_file=p["ref"], bias=given, by_name=True, stride=stride, **kw)
            assert len(notes) == 2 and "wZ" in notes[0] and "not in the input" in notes[0], notes
            assert "wX" in notes[1] and "not in the reference" in notes[1] and "wZ" not in notes[1], notes
            results[tag, how] = r
    res = results["frag", "none"]
    for k, other in results.items():
        assert same_ocf(res, other), k
    groups, n_sites, units, count, site_units, site_count, seen = restated_product(p, table, lo, hi, H, b, peak, flank, True, {"wZ", "wX"})
    first = list(dict.fromkeys(r[3] for r in p["rows"]))
    assert res.groups == groups == tuple(first) and set(groups) == {"CTCF", "GATA1", ".", "SPI1"}  # first-appearance order
    assert res.skipped_contigs == ("wZ", "wX") and np.array_equal(res.n_sites, n_sites) and n_sites.sum() == 120
    assert np.array_equal(res.up_count, count[:, 0]) and np.array_equal(res.down_count, count[:, 1])
    assert np.array_equal(res.up_corrected, units[:, 0] / 65536.0) and np.array_equal(res.down_corrected, units[:, 1] / 65536.0)
    group_of = np.array([groups.index(r[3]) for r in p["rows"]])
    windows, ocf_units = np.zeros((len(groups), 4), np.int64), np.zeros(len(groups), np.int64)
    np.add.at(windows, group_of[seen], site_count[seen])
    np.add.at(ocf_units, group_of[seen], (site_units[seen] * SIGN).sum(axis=1))
    assert np.array_equal(res.windows_count, windows) and np.array_equal(res.ocf_count, (windows * SIGN).sum(axis=1))
    assert np.array_equal(res.ocf, ocf_units / 65536.0)
    assert np.array_equal(np.isnan(res.site_ocf), np.isin(site_contig, ("wZ", "wX"))) and np.array_equal(~seen, np.isnan(res.site_ocf))
    assert np.array_equal(res.site_ocf[seen], (site_units[seen] * SIGN).sum(axis=1) / 65536.0)
    # the cases bite: ends in every bin of both tracks, weights that are not all one, a - site among the sites, windows
    # that are not empty, scores of either sign
    assert (count.sum(axis=0) > 0).all() and not np.array_equal(units, count * ONE) and (windows > 0).all()
    assert any(r[4] == "-" and r[0] in ("wA", "wC") for r in p["rows"])
    assert (res.site_ocf[seen] > 0).any() and (res.site_ocf[seen] < 0).any()
    # normalize: both corrected tracks and the score of a group over the mean of its corrected profile
    norm, _ = run_ocf(p["frag"], p["bed"], reference_file=p["ref"], bias=bias, by_name=True, normalize=True, **kw)
    assert np.array_equal(norm.up_count, res.up_count) and np.array_equal(norm.ocf_count, res.ocf_count)
    assert np.array_equal(norm.site_ocf, res.site_ocf, equal_nan=True)
    for g in range(len(groups)):
        mean = np.stack([res.up_corrected[g], res.down_corrected[g]]).mean()
        assert mean > 0 and np.array_equal(norm.up_corrected[g], res.up_corrected[g] / mean)
        assert np.array_equal(norm.down_corrected[g], res.down_corrected[g] / mean) and norm.ocf[g] == res.ocf[g] / mean
    # the three files, field by field, and the command line in a child process
    for suffix in (".tsv", ".tsv.gz"):
        out, prof, per = (str(tmp_path / (stem + suffix)) for stem in ("fn", "fn_profile", "fn_sites"))
        again, _ = run_ocf(p["frag"], p["bed"], out, prof, per, reference_file=p["ref"], bias=bias, by_name=True, **kw)
        assert same_ocf(again, res)
        lines = read_text(out).splitlines()
        assert lines[0] == "#group\tn_sites\tleft_up\tleft_down\tright_up\tright_down\tocf_count\tocf" and len(lines) == 1 + len(groups)
        for g, name in enumerate(groups):
            assert lines[1 + g].split("\t") == [name, str(int(n_sites[g]))] + [str(int(x)) for x in windows[g]] + [
                str(int((windows[g] * SIGN).sum())), format(ocf_units[g] / 65536.0, ".6f")], g
        lines = read_text(prof).splitlines()
        assert lines[0] == "#group\tn_sites\toffset\tup_count\tdown_count\tup_corrected\tdown_corrected"
        assert len(lines) == 1 + len(groups) * n_bins
        for g, name in enumerate(groups):
            for k in range(n_bins):
                assert lines[1 + g * n_bins + k].split("\t") == [
                    name, str(int(n_sites[g])), str(-H + k * b), str(int(count[g, 0, k])), str(int(count[g, 1, k])),
                    format(units[g, 0, k] / 65536.0, ".6f"), format(units[g, 1, k] / 65536.0, ".6f")], (g, k)
        lines = read_text(per).splitlines()
        assert lines[0] == "#contig\tcentre\tname\tstrand\tleft_up\tleft_down\tright_up\tright_down\tocf"
        kept = [i for i in range(len(p["rows"])) if seen[i]]
        assert len(lines) == 1 + len(kept) == 121
        for line, i in zip(lines[1:], kept):
            c, a, z, nm, st = p["rows"][i]
            assert line.split("\t") == [c, str((a + z) // 2), nm, st] + [str(int(x)) for x in site_count[i]] + [
                format((site_units[i] * SIGN).sum() / 65536.0, ".6f")], i
        cli = [str(tmp_path / (stem + suffix)) for stem in ("cli", "cli_profile", "cli_sites")]
        r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.ocf", p["frag"], p["bed"], cli[0], "--profile", cli[1], "--per-site",
                            cli[2], "--reference", p["ref"], "--bias", str(tmp_path / "bias.tsv.gz"), "--half-width", str(H),
                            "--bin-size", str(b), "--peak", str(peak), "--flank", str(flank), "--min-length", str(lo), "--max-length",
                            str(hi), "-q", "30", "--by-name"], cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert "wX" in r.stderr and "wZ" in r.stderr  # the warnings
        for mine, theirs in zip((out, prof, per), cli):
            if suffix == ".tsv":
                assert open(theirs, "rb").read() == open(mine, "rb").read()
            else:
                assert gzip.open(theirs, "rb").read() == gzip.open(mine, "rb").read()
