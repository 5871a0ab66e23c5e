"""CPU: the co-fragmentation feature's host side - the two restatements of the rule held to each other (also at the
2^31 edge), ``utils.ks_neglog10_p`` against scipy and against its own closed form, the bin tiling and its limit, the
mask, the correlation and the sign rule of ``pc1``, both writers, and the planted compartments of the issue."""
import gzip

import numpy as np
import pytest

from finaletoolkit_amd import utils, writers
from tests import cofrag_helpers as H


def parts(hist, min_count=1, distance="d", len_lo=0):
    K, at, n = H.ks_matrix(hist)
    N = len(n)
    starts = np.arange(N, dtype=np.int64) * 100
    return utils.cofrag_host_part("c", starts, starts + 100, n, np.zeros(N, np.int64), K, at, len_lo, min_count, distance)


# ---- the restatements
@pytest.mark.parametrize("n_rows,n_bins,top", [(1, 1, 40), (2, 2, 40), (7, 33, 40), (12, 65, 3), (5, 40, 1 << 20)])
def test_restatements_agree(n_rows, n_bins, top):
    hist = H.random_hist(np.random.default_rng(n_rows * 1000 + n_bins), n_rows, n_bins, top)
    hist[n_rows // 2] = 0 if n_rows > 2 else hist[n_rows // 2]
    K, at, n = H.ks_matrix(hist)
    Kl, atl, nl = H.ks_matrix_loop(hist)
    assert K.tolist() == Kl and at.tolist() == atl and n.tolist() == nl
    assert (K == K.T).all() and (at == at.T).all() and not np.diag(K).any() and not np.diag(at).any()


def test_restatements_agree_at_the_width_limit():
    top = (1 << 31) - 1
    hist = np.zeros((4, 9), np.uint32)
    hist[0, 2] = top
    hist[1, 7] = top
    hist[2] = top // 9
    hist[3, 8] = 5
    K, at, n = H.ks_matrix(hist)
    Kl, atl, nl = H.ks_matrix_loop(hist)
    assert K.tolist() == Kl and at.tolist() == atl and n.tolist() == nl
    assert K[0, 1] == top * top and at[0, 1] == 2


def test_leftmost_maximum_and_disjoint_supports():
    hist = np.zeros((2, 10), np.uint32)
    hist[0, 1] = 3
    hist[1, 6] = 5
    K, at, n = H.ks_matrix(hist)
    assert K[0, 1] == 15 and at[0, 1] == 1  # |C0 n1 - C1 n0| = 15 on lengths 1 .. 5: the first of them


# ---- the p-value
def test_ks_neglog10_p_against_scipy():
    special = pytest.importorskip("scipy.special")
    z = np.array([0.04, 0.05, 0.3, 1.0, 2.0, 5.0])
    got = 10.0 ** -utils.ks_neglog10_p(z)
    np.testing.assert_allclose(got, special.kolmogorov(z), rtol=1e-9, atol=1e-12)


def series(z):
    k = np.arange(1, 201, dtype=np.float64)
    return 2.0 * float((np.where(k % 2 == 1, 1.0, -1.0) * np.exp(-2.0 * k * k * z * z)).sum())


def test_ks_neglog10_p_closed_form_and_edges():
    for z in (1.0, 1.5, 2.0, 3.0, 5.0, 10.0, 15.0):  # the series is still a normal number up to here
        assert utils.ks_neglog10_p(z) == pytest.approx(-np.log10(series(z)), rel=1e-12)
    for z in (0.04, 0.1, 0.5, 0.999):
        assert utils.ks_neglog10_p(z) == pytest.approx(-np.log10(min(series(z), 1.0)), rel=1e-12, abs=1e-15)
    assert series(40.0) == 0.0
    big = utils.ks_neglog10_p(np.array([39.0, 40.0, 41.0]))
    assert np.isfinite(big).all() and big[0] < big[1] < big[2]
    assert big[1] == pytest.approx((2 * 1600.0 - np.log(2.0)) / np.log(10.0), rel=1e-12)
    z = np.array([[0.0, 0.0399, np.nan], [0.04, 1.0, 2.0]])
    out = utils.ks_neglog10_p(z)
    assert out.shape == z.shape and out[0, 0] == 0 and out[0, 1] == 0 and np.isnan(out[0, 2]) and (out[1] >= 0).all()
    assert np.all(np.diff(utils.ks_neglog10_p(np.linspace(0.3, 3.0, 200))) > 0)


# ---- bins
def test_bin_tiling_and_limit():
    starts, stops = utils.cofrag_bins(1050, 100)
    assert starts.tolist() == list(range(0, 1100, 100)) and stops.tolist() == list(range(100, 1100, 100)) + [1050]
    starts, stops = utils.cofrag_bins(1000, 100)
    assert len(starts) == 10 and stops[-1] == 1000
    assert len(utils.cofrag_bins(0, 100)[0]) == 0
    assert len(utils.cofrag_bins(4096 * 50, 50)[0]) == 4096
    with pytest.raises(ValueError, match="4097 bins.*at most 4096"):
        utils.cofrag_bins(4096 * 50 + 1, 50, "chrZ")
    with pytest.raises(ValueError):
        utils.cofrag_bins(100, 0)


# ---- the host arithmetic
def test_mask_by_min_count_and_float_fields():
    rng = np.random.default_rng(3)
    hist = H.random_hist(rng, 8, 30)
    hist[2] = 0
    hist[5, 3:] = 0
    hist[5, :3] = 1
    r = parts(hist, min_count=10, len_lo=50)
    K, at, n = H.ks_matrix(hist)
    assert r.valid.tolist() == (n >= 10).tolist() and not r.valid[2] and not r.valid[5]
    pair = r.valid[:, None] & r.valid[None, :]
    assert np.isnan(r.D[~pair]).all() and np.isnan(r.z[~pair]).all() and np.isnan(r.neglog10_p[~pair]).all() and np.isnan(r.corr[~pair]).all()
    i, j = 0, 7
    d = int(K[i, j]) / (int(n[i]) * int(n[j]))
    assert r.D[i, j] == pytest.approx(d, rel=1e-15)
    assert r.z[i, j] == pytest.approx(d * np.sqrt(int(n[i]) * int(n[j]) / (int(n[i]) + int(n[j]))), rel=1e-14)
    assert r.neglog10_p[i, j] == utils.ks_neglog10_p(r.z[i, j]) and (r.neglog10_p == r.neglog10_p.T)[pair].all()
    assert (r.at == at + 50).all() and r.at.dtype == np.int32 and (r.K == K).all()
    assert np.isnan(r.pc1[[2, 5]]).all() and np.isfinite(r.pc1[r.valid]).all()
    assert np.nansum(r.pc1 ** 2) == pytest.approx(1.0)
    v = np.flatnonzero(r.valid)
    np.testing.assert_allclose(r.corr[np.ix_(v, v)], np.corrcoef(r.D[np.ix_(v, v)]), rtol=0, atol=1e-15)
    # min_count never lets an empty bin through
    assert not parts(hist, min_count=0).valid[2]


def test_fewer_than_three_valid_bins():
    hist = H.random_hist(np.random.default_rng(4), 5, 20)
    hist[2:] = 0
    r = parts(hist)
    assert r.valid.sum() == 2 and np.isnan(r.corr).all() and np.isnan(r.pc1).all() and np.isfinite(r.D[:2, :2]).all()
    r = parts(np.zeros((1, 4), np.uint32))
    assert not r.valid.any() and np.isnan(r.pc1).all()


def test_pc1_sign_rule_and_distance():
    for depth in (300, 2000):
        hist = H.planted_hist(depth)
        for rows in (hist, hist[::-1].copy()):
            for distance in "dz":
                r = parts(rows, distance=distance)
                assert r.pc1[np.argmax(np.abs(r.pc1))] > 0
    with pytest.raises(ValueError):
        parts(hist, distance="x")


@pytest.mark.parametrize("distance", ["d", "z"])
@pytest.mark.parametrize("depth", [300, 2000])
def test_planted_compartments(depth, distance):
    r = parts(H.planted_hist(depth), distance=distance)
    side = r.pc1 > 0
    assert (side == (H.PLANTED_GROUPS == H.PLANTED_GROUPS[np.argmax(np.abs(r.pc1))])).all()
    print("smallest |pc1|", np.abs(r.pc1).min())
    assert np.abs(r.pc1).min() > 0.1


# ---- the writers
@pytest.mark.parametrize("suffix", [".tsv", ".tsv.gz"])
def test_writers_round_trip(tmp_path, suffix):
    hist = H.planted_hist(300)
    hist[3] = 0
    a, b = parts(hist, min_count=5, len_lo=50), parts(hist[:4], min_count=5)
    b = b._replace(contig="d", overflow=np.array([0, 2, 0, 9], np.int64))
    track, pairs = str(tmp_path / ("t" + suffix)), str(tmp_path / ("p" + suffix))
    writers.write_cofrag_track(track, [a, b])
    writers.write_cofrag_pairs(pairs, [a, b])
    opener = gzip.open if suffix.endswith(".gz") else open
    with opener(track, "rt") as fh:
        rows = [line.rstrip("\n").split("\t") for line in fh]
    assert rows[0] == "contig start stop n_frags overflow valid pc1".split()
    want = [(r, k) for r in (a, b) for k in range(len(r.n))]
    assert len(rows) == 1 + len(want)
    for row, (r, k) in zip(rows[1:], want):
        assert row[:6] == [r.contig, str(r.starts[k]), str(r.stops[k]), str(r.n[k]), str(r.overflow[k]), str(int(r.valid[k]))]
        assert float(row[6]) == r.pc1[k] or (np.isnan(float(row[6])) and np.isnan(r.pc1[k]))
    with opener(pairs, "rt") as fh:
        rows = [line.rstrip("\n").split("\t") for line in fh]
    assert rows[0] == "contig start_i start_j n_i n_j ks_num d at z neglog10_p corr".split()
    want = [(r, i, j) for r in (a, b) for i in range(len(r.n)) for j in range(i + 1, len(r.n))]
    assert len(rows) == 1 + len(want)
    for row, (r, i, j) in zip(rows[1:], want):
        assert row[:6] == [r.contig, str(r.starts[i]), str(r.starts[j]), str(r.n[i]), str(r.n[j]), str(r.K[i, j])] and int(row[7]) == r.at[i, j]
        for text, value in zip((row[6], row[8], row[9], row[10]), (r.D[i, j], r.z[i, j], r.neglog10_p[i, j], r.corr[i, j])):
            assert float(text) == value or (np.isnan(float(text)) and np.isnan(value))
    with pytest.raises(ValueError):
        writers.write_cofrag_track(str(tmp_path / "t.bed"), [a])
    with pytest.raises(ValueError):
        writers.write_cofrag_pairs(str(tmp_path / "p.txt"), [a])


def test_exported_from_the_package():
    import finaletoolkit_amd as F
    assert F.frag_cofragmentation is utils.frag_cofragmentation and F.CoFragmentation is utils.CoFragmentation
    assert F.ks_neglog10_p is utils.ks_neglog10_p
    from finaletoolkit_amd import cofrag
    args = cofrag.build_parser().parse_args(["in.frag.gz", "out.tsv", "--pairs", "p.tsv.gz", "--bin-size", "1000", "--contigs", "a", "b",
                                             "--chrom-sizes", "s", "--min-length", "10", "--max-length", "90", "-q", "5", "--min-count",
                                             "7", "--distance", "z"])
    assert vars(args) == dict(input_file="in.frag.gz", output_file="out.tsv", pairs_file="p.tsv.gz", bin_size=1000, contigs=["a", "b"],
                              chrom_sizes="s", min_length=10, max_length=90, quality_threshold=5, min_count=7, distance="z")
    for bad in (dict(distance="x"), dict(bin_size=0), dict(min_length=10, max_length=9), dict(min_length=0, max_length=4096),
                dict(output_file="o.bed"), dict(pairs_file="p.txt"), dict()):
        with pytest.raises(ValueError):
            utils.frag_cofragmentation("in.frag.gz", **bad)  # (the last: no chrom_sizes for a fragment file)
