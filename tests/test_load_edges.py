"""The worlds of ``tests/load_edges.py`` hold every case ``tests/test_gpu_load_edges.py`` relies on, and every pair of
oracle answers that is meant to tell a right load from a wrong one really differs.  CPU only."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import load_edges as E

# The caps of the two grid-stride launches, restated: csrc/ftk_kernels.hip, launch_stats (at most 1024 blocks of
# kStatsThreads = 256) and launch_r1_inside (at most 2048 blocks of 256).  The positions follow from them.
STATS_CAP = 1024 * 256
R1_CAP = 2048 * 256


def test_positions_follow_the_launch_caps():
    assert (E.CAP_STATS, E.CAP_R1) == (STATS_CAP, R1_CAP) == (262_144, 524_288)
    assert (E.N_STATS, E.N_R1) == (STATS_CAP + 1_000, R1_CAP + 1_000)
    assert set(E.POS) == {1, 63, 64, 65, 255, 256, 257, 1023, 1024, STATS_CAP - 1, STATS_CAP, STATS_CAP + 1, E.N_STATS - 1}
    assert set(E.R1_POS) == {0, 63, 64, 255, 256, R1_CAP - 1, R1_CAP, E.N_R1 - 1}
    assert set(E.SIZES) == {0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025} | set(range(262_140, 262_149))
    assert {n % 4 for n in E.SIZES} == {0, 1, 2, 3}


@pytest.mark.parametrize("cols", [E.stats_world, E.r1_world], ids=["stats", "r1"])
def test_background(cols):
    fs, fe, mq, st = (c.astype(np.int64) for c in cols()[:4])
    gap = np.diff(fs)
    assert fs[0] == E.FIRST_START and gap.min() == 0 and 0 < (gap == 0).sum() < len(fs) // 100
    assert set(gap[gap > 0].tolist()) == set(range(15, 26))
    ln = fe - fs
    assert (ln.min(), ln.max()) == (100, 200) and fe.max() < E.LIMIT // 64
    assert mq.min() == 0 and mq.max() == 60 and set(st.tolist()) == {0, 1}
    assert not cols()[0].flags.writeable


@pytest.mark.parametrize("i", E.POS)
def test_one_offender(i):
    base = E.stats_world()
    s, e = E.unsorted_at(base, i)[:2]
    assert np.flatnonzero(np.diff(s.astype(np.int64)) < 0).tolist() == [i - 1]        # thread i alone: start[i-1] > start[i]
    assert s[i] == s[i - 1] - 1 and (e - s).min() >= 100 and s.min() >= 0
    s, e = E.negative_at(base, i)[:2]
    assert np.flatnonzero(e < s).tolist() == [i] and e[i] == s[i] - 1 and np.all(np.diff(s) >= 0)
    for v, ok in ((E.LIMIT, False), (E.LIMIT - 1, True)):
        s, e = E.end_at(base, i, v)[:2]
        assert np.flatnonzero(e >= E.LIMIT).tolist() == ([] if ok else [i]) and np.all(np.diff(s) >= 0) and (e - s).min() >= 0
        if ok:   # the accepted contig's summary is this fragment's alone
            assert E.summary((s, e)) == (E.N_STATS, E.LIMIT - 1 - int(s[i]), E.LIMIT - 1)
            assert E.summary((s, e))[1:] != E.summary(base)[1:]


def test_ties_and_the_negative_start():
    base = E.stats_world()
    s, e = E.all_equal(base)[:2]
    assert np.all(s == s[0]) and np.array_equal(e - s, base[1] - base[0])
    s, e = E.ties_at(base)[:2]
    assert all(s[i] == s[i - 1] for i in E.POS) and np.all(np.diff(s) >= 0) and np.array_equal(e - s, base[1] - base[0])
    s, e = E.start_at(base, 0, -1)[:2]
    assert np.flatnonzero(s < 0).tolist() == [0] and np.all(np.diff(s) >= 0) and e[0] > s[0]


@pytest.mark.parametrize("n", E.SIZES)
def test_sized_contigs(n):
    s, e, q, st = E.sized(n)
    assert len(s) == n and np.all(np.diff(s) >= 0)
    if n >= 2:
        ln = e.astype(np.int64) - s
        assert ln.argmax() == 0 and (ln == ln.max()).sum() == 1                       # the longest: thread 0
    if n >= 64:
        assert e.argmax() == n - 1 and (e == e.max()).sum() == 1                      # the highest end: the last thread


@pytest.mark.parametrize("i", E.POS)
def test_long_fragment_discriminates(i):
    base = E.stats_world()
    cols = E.long_at(base, i)
    assert E.summary(cols)[1] == E.LONG and E.summary(base)[1] == 200 and np.array_equal(cols[0], base[0])
    fs = int(cols[0][i])
    ws, we = E.long_windows(fs)
    with_, without = O.Frags(*cols), O.Frags(*base)
    a = O.c_window_counts(with_, ws, we, mapq_min=0, policy="any")
    b = O.c_window_counts(without, ws, we, mapq_min=0, policy="any")
    assert (a - b).tolist() == [1, 1, 0]                 # reaches the first two; the third begins at its end
    a = O.c_window_counts(with_, ws, we, mapq_min=0, policy="any", max_len=400)
    assert np.array_equal(a, b)                          # capped below it: absent
    lo, hi = E.long_interval(fs)
    assert fs + E.LONG - 1_000 <= lo and hi <= fs + E.LONG and hi - lo == 300
    assert np.array_equal(E.restated_depth(cols, lo, hi) - E.restated_depth(base, lo, hi), np.ones(300, np.int32))
    size = fs + 2 * E.LONG
    w1 = O.c_wps(with_, lo, hi, size, max_len=E.LONG + 10_000, mapq_min=0)
    w0 = O.c_wps(without, lo, hi, size, max_len=E.LONG + 10_000, mapq_min=0)
    assert np.array_equal(w1 - w0, np.ones(300, np.int64))
    for length, present in ((E.LQ_LEN_MAX, True), (E.LQ_LEN_MAX + 1, False)):
        assert (E.summary(E.long_at(base, i, length))[1] <= E.LQ_LEN_MAX) == present


@pytest.mark.parametrize("n_bins", E.INDEX_BINS)
def test_index_world(n_bins):
    fs, fe, mq, st = E.index_world(n_bins)
    fs64 = fs.astype(np.int64)
    assert 2_000 <= len(fs) <= 5_000 and np.all(np.diff(fs64) >= 0)
    assert int(fs.max()) == E.index_max_start(n_bins) and (int(fs.max()) >> 9) + 1 == n_bins
    assert tuple(sorted(set((fs64 // E.BIN).tolist()))) == E.occupied_bins(n_bins)
    assert set((fs64 % E.BIN).tolist()) == {0, 1, 511}
    assert set((fs64[fs64 // E.BIN == n_bins - 2] % E.BIN).tolist()) == {0, 1, 511}
    ln = fe.astype(np.int64) - fs64
    assert ln.min() == 1 and np.sort(ln)[-2] == 600 and ln.max() == 5_000 and (ln == 5_000).sum() == 1
    ws, we = E.index_windows(n_bins)
    assert 800 <= len(ws) <= 5_000
    assert any(a is not None and a < 0 for a in ws) and any(a is not None and a >= n_bins * E.BIN for a in ws)
    assert (None, None) in set(zip(ws, we)) and all(a is None or b is None or a < b for a, b in zip(ws, we))
    sample = E.index_select_sample(n_bins)
    assert len(sample) == len(set(sample)) == 200
    fr = O.Frags(fs, fe, mq, st)
    last = fs64 // E.BIN >= n_bins - 2
    cut = O.Frags(fs[~last], fe[~last], mq[~last], st[~last])
    for pol in ("midpoint", "any"):
        for ml in E.INDEX_FILTERS:
            a = O.c_window_counts(fr, ws, we, mapq_min=E.INDEX_Q, policy=pol, max_len=ml)
            b = O.c_window_counts(cut, ws, we, mapq_min=E.INDEX_Q, policy=pol, max_len=ml)
            assert a.max() > 0 and (a != b).sum() > 100            # the last two bins matter to many windows
            assert (a[sample] != b[sample]).any()
    # the cleavage cases: the named fragment's end is the one found (or not) through bin_idx[k] alone, and it shows
    cases = E.index_cleavage_cases(n_bins)
    assert len(cases) >= 3 and {c[3] // E.BIN for c in cases} >= {7, 8, n_bins - 2}
    for start, stop, ml, at in cases:
        hit = np.flatnonzero((fs64 == at) & (ln == ml) & (st == 0) & (mq >= E.INDEX_Q))
        assert hit.size >= 1 and at % E.BIN == 0 and start >= 0 and at + ml == start + E.TILE < stop and ln[ln <= ml].max() == ml
        keep = np.ones(len(fs), bool)
        keep[hit] = False
        _, ends, prop = O.c_cleavage(fr, start, stop, max_len=ml, mapq_min=E.INDEX_Q)
        _, ends0, prop0 = O.c_cleavage(O.Frags(fs[keep], fe[keep], mq[keep], st[keep]), start, stop, max_len=ml, mapq_min=E.INDEX_Q)
        assert ends[E.TILE] - ends0[E.TILE] == hit.size and prop[E.TILE] != prop0[E.TILE]


def test_r1_world_is_all_inside():
    fs, fe, mq, st, r1s, r1e = E.r1_world()
    assert np.all((fs <= r1s) & (r1s < r1e) & (r1e <= fe)) and np.all(r1e - r1s == E.R1_LEN)
    assert np.all(np.where(st != 0, r1s == fs, r1e == fe))
    at = np.array(E.R1_POS)
    assert np.all(fe[at] - fs[at] == 150) and np.all(mq[at] == 60)
    r1s, r1e = E.r1_odd_spans()
    bad = np.flatnonzero(~((fs <= r1s) & (r1s < r1e) & (r1e <= fe)))
    assert bad.tolist() == sorted(E.R1_POS) and (r1s[at] == r1e[at]).sum() == 4 and (r1s[at] > r1e[at]).sum() == 4


@pytest.mark.parametrize("kind", E.R1_KINDS)
@pytest.mark.parametrize("i", E.R1_POS)
def test_one_read1_outlier_discriminates(i, kind):
    fs, fe, mq, st, in_s, in_e = E.r1_world()
    r1s, r1e = E.r1_outlier(i, kind)
    bad = np.flatnonzero(~((fs <= r1s) & (r1s < r1e) & (r1e <= fe)))
    assert bad.tolist() == [i] and r1s.min() >= 0
    a, b = E.r1_interval(i)
    assert a < fs[i] and fe[i] < b                                   # an interior fragment of the window
    assert r1e[i] <= a - 180 - 120 or r1s[i] >= b + 180 + 120        # beyond the WPS fetch margin too
    for n in (100, 320):
        ws, we = E.r1_tiles(i, n)
        inside = np.flatnonzero((ws <= fs[i]) & (fe[i] <= we))
        assert len(ws) == n and ws[0] >= 0 and inside.size == 1 and np.all(ws[1:] == we[:-1])
        assert np.all(we - ws == we[0] - ws[0])                      # one length: the block path from one window per CU on
    lo, hi = E.r1_slice(i)
    assert lo <= i < hi
    out, back = E.r1_expected(r1s, r1e, i), E.r1_expected(in_s, in_e, i)
    assert set(out) == set(back)
    for key in out:
        if key in ("over", "sel_q", "sel_st") or key.endswith("_short") or key.endswith("_long") or key in ("short", "long"):
            continue
        assert out[key].shape != back[key].shape or not np.array_equal(out[key], back[key]), key
    assert (out["short"] + out["long"] != back["short"] + back["long"]).all()
    for n in (100, 320):
        assert ((out[f"tiles{n}_short"] + out[f"tiles{n}_long"]) != (back[f"tiles{n}_short"] + back[f"tiles{n}_long"])).sum() == 1
        assert (out[f"tiles{n}"] != back[f"tiles{n}"]).sum() == 1
