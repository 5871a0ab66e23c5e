"""The world of ``tests/motif_edges.py`` holds every case ``tests/test_gpu_motif_edges.py`` relies on (so an edit of the
builder cannot silently lose one), and its both-strands helper agrees with ``oracle.py_region_motifs`` where that does
not raise.  CPU only; the conditions are the ones the motif kernels branch on (csrc/ftk_kernels.hip: motif_window,
motif_has_n, motif_stream's EDGE switch, the 512-thread choice of features_common)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import motif_edges as M

K = M.K_REF


@pytest.fixture(scope="module")
def W():
    return M.world()


def test_contig_edge_layout(W):
    e, runs = W["edge"], W["runs"]
    L = e.L
    assert L == 24_003 and L % 4 == 3 and L % 60 == 3 and L % 61 != 0
    b = np.frombuffer(e.seq.encode(), np.uint8)
    is_n = (b & 0xDF) == ord("N")
    d = np.diff(np.concatenate([[0], is_n.astype(np.int8), [0]]))
    found = list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))
    assert found == runs                                  # the list IS the sequence's N runs: sorted, disjoint, apart
    assert len(runs) >= 70                                # motif_window counts 64 blocks per trip: a second trip
    lens = {y - x for x, y in runs}
    assert {1, 2, 3, 4, 5} <= lens
    assert {x & 3 for x, _ in runs} == {0, 1, 2, 3}
    gaps = [runs[i + 1][0] - runs[i][1] for i in range(len(runs) - 1)]
    assert 1 in gaps and K in gaps and K - 1 in gaps
    assert 0 < runs[0][0] <= 7 and L - 7 <= runs[-1][1] < L
    assert sum(M.CLUSTER[0] <= x and y <= M.CLUSTER[1] for x, y in runs) >= 40 and M.CLUSTER[1] - M.CLUSTER[0] == 2000
    assert M.N_FREE[1] - M.N_FREE[0] >= 6000 and not is_n[M.N_FREE[0]:M.N_FREE[1]].any()
    assert ((b & 0x20) != 0).any() and (b == ord("n")).any()   # lower-case runs, one of them over N runs


def test_fragments(W):
    e, runs = W["edge"], W["runs"]
    L = e.L
    assert np.all(np.diff(e.fs) >= 0) and len(e.fs) <= 8000
    ln = e.fe.astype(np.int64) - e.fs
    assert ln.min() >= 1 and ln.max() == M.MAX_LEN and e.fs.min() == 0 and e.fs.max() <= L - 1
    have_f = set(e.fs.tolist())
    have_r = set((e.fe - K).tolist())
    for a, b in runs:  # every run, both edges, d = -8..+1: a forward k-mer start and a reverse one there
        for edge in (a, b):
            for d in range(-8, 2):
                if edge + d >= 0:
                    assert edge + d in have_f and edge + d in have_r, (a, b, d)
    assert {M.Q - 1, M.Q} <= set(W["sys_mapq"].tolist()) and set(W["sys_strand"].tolist()) == {0, 1}
    assert set(e.st.tolist()) == {0, 1}
    pairs = set(zip(e.fs.tolist(), ln.tolist()))
    assert all((a, n) in pairs for a in range(9) for n in range(1, 11))
    ends = {(int(y)) for x, y in zip(e.fs, e.fe) if x <= L - 1}
    assert set(range(L - 8, L + 4)) <= ends
    assert (e.fe < K).any() and (e.fs < K).any() and (e.fe > L).any()
    # 5' k-mer off the contig, 3' k-mer on it: the reference's `continue` drops the 3' end too (end_both_split)
    assert ((e.fs + K > L) & (e.fe <= L) & (e.fe - K >= 0) & (e.mq >= M.Q)).any()


def test_bam_variants(W):
    e, b, ins = W["edge"], W["edge_bam"], W["edge_bam_inside"]
    for c in (b, ins):
        assert all(np.array_equal(getattr(c, f), getattr(e, f)) for f in ("fs", "fe", "mq", "st")) and c.seq == e.seq
        assert np.all(c.r1s < c.r1e) and c.r1s.min() >= 0
    assert np.all((ins.r1s >= ins.fs) & (ins.r1e <= ins.fe))            # r1_inside = 1
    fwd = ins.st != 0
    assert np.all(ins.r1s[fwd] == ins.fs[fwd]) and np.all(ins.r1e[~fwd] == ins.fe[~fwd])
    out_r = b.r1e > b.fe
    out_l = b.r1s < b.fs
    assert (out_r | out_l).sum() >= 200 and (out_r | out_l).mean() < 0.2
    assert (b.r1e - b.fe).max() <= 400 and (b.fs - b.r1s).max() <= 400
    assert (b.r1e - b.fe).max() > 300 and (b.fs - b.r1s).max() > 300
    # fragments that end before WIN_A / start behind WIN_B and are fetched for it through read 1 alone
    assert (out_r & (b.fe <= M.WIN_A[0]) & b.fetched(*M.WIN_A)).sum() >= 20
    assert (out_l & (b.fs >= M.WIN_B[1]) & b.fetched(*M.WIN_B)).sum() >= 20
    d, db = W["dense"], W["dense_bam"]
    assert np.all((db.r1s >= db.fs) & (db.r1e <= db.fe)) and np.array_equal(d.fs, db.fs)


def all_small_windows(W):
    return sorted({w for kind in ("end", "breakpoint") for k in range(1, 8)
                   for w in M.small_windows(W["runs"], M.L_EDGE, kind, k)})


def test_fetched_fragments_are_candidates(W):
    """The library looks for a window's fragments among the starts from the 512-bp bin of ws - max_len to the end of the
    bin of we.  A read-1 span may stick out only as far as that: every fragment the oracle fetches for a tested
    window lies in the window's candidate range."""
    sets = {"edge": all_small_windows(W) + M.tile_windows(), "edge_bam": all_small_windows(W),
            "edge_bam_inside": all_small_windows(W) + M.tile_windows(), "dense": M.DENSE_DISTINCT,
            "dense_bam": M.DENSE_DISTINCT}
    for name, wins in sets.items():
        c = W[name]
        for ws, we in wins:
            f = c.fetched(ws, we)
            assert np.all(M.candidate(c.fs[f], ws, we)), (name, ws, we)


def test_fetched_mask_is_the_oracle_fetch(W):
    for name in ("edge", "edge_bam"):
        c = W[name]
        rows = c.rows()
        for ws, we in (M.WIN_A, M.WIN_B, (0, 1), (3_001, 3_001), (6_000, 5_000), (c.L, c.L + 10), (-50, 30)):
            got = [r[:4] for r, f in zip(rows, c.fetched(ws, we)) if f]
            assert got == list(O.py_fetch(rows, ws, we, M.Q)), (name, ws, we)
            assert got == list(O.py_fetch(c.rows_near(ws, we), ws, we, M.Q)), (name, ws, we)


def touches_n(seq_is_n_cum, p, k, L):
    """Does the k-mer [p, p + k) (inside the contig) hold an N?"""
    return seq_is_n_cum[np.clip(p + k, 0, L)] - seq_is_n_cum[np.clip(p, 0, L)] > 0


@pytest.mark.parametrize("kind", ["end", "breakpoint"])
def test_stick_outs_beyond_the_reach(W, kind):
    """motif_has_n's fallback: a k-mer at or beyond the reach (ws - r, we + r + k) of the window its fragment is
    fetched for searches every N block - with an N under it (the fallback decides the count) and without."""
    b = W["edge_bam"]
    L = b.L
    cum = np.concatenate([[0], np.cumsum((np.frombuffer(b.seq.encode(), np.uint8) & 0xDF) == ord("N"))])
    s = M.spec_of(kind, K, True, False)
    r = M.reach_of(kind, K)
    on_n = clean = 0
    for ws, we in (M.WIN_A, M.WIN_B):
        f = b.fetched(ws, we)
        pf, pr = b.fs.astype(np.int64) + s["fwd_offset"], b.fe.astype(np.int64) + s["rev_offset"]
        inside = lambda p: (p >= 0) & (p + K <= L)
        beyond = lambda p: inside(p) & ((p <= ws - r) | (p + K >= we + r + K))
        n_f, n_r = touches_n(cum, pf, K, L), touches_n(cum, pr, K, L)
        far = f & (beyond(pf) | beyond(pr))
        on_n += int((f & ((beyond(pf) & n_f) | (beyond(pr) & n_r))).sum())
        clean += int((far & ~n_f & ~n_r).sum())
    assert on_n >= 20 and clean >= 20, (on_n, clean)


@pytest.mark.parametrize("kind", ["end", "breakpoint"])
@pytest.mark.parametrize("k", range(1, 8))
def test_small_windows(W, kind, k):
    e, runs = W["edge"], W["runs"]
    L = e.L
    wins = M.small_windows(runs, L, kind, k)
    assert 30 <= len(wins) <= 48
    r = M.reach_of(kind, k)
    for w in ((0, 1), (0, k), (L - 1, L), (L, L + 10), (0, L), M.CLUSTER, M.WIN_A, M.WIN_B):
        assert w in wins
    assert any(ws < 0 < we for ws, we in wins) and any(ws == we for ws, we in wins) and any(we < ws for ws, we in wins)
    assert any(we <= 0 and ws < we for ws, we in wins) and any(ws > L + 3 for ws, we in wins)
    edges = {x for a, b in runs for x in (a, b)}
    assert sum(we - ws == 1 and (ws in edges or we in edges) for ws, we in wins) >= 12
    assert any(M.N_FREE[0] <= ws and we <= M.N_FREE[1] and we - ws >= 1000 for ws, we in wins)
    # single-base windows at runs past the 64th
    assert any(we - ws == 1 and ws >= runs[64][0] for ws, we in wins)
    # [0, L): chunked (> 1024 candidates) over two chunks (> 4096)
    assert len(e.fs) > 4096
    # both sides of the range-test switch, g_lo >= -1 and g_hi - 1 <= L with g_lo = ws - r, g_hi = we + r + k: each
    # window fetches the fragment that comes closest to the contig end its reach admits (fs = ws + 1 - max_len, and
    # fs = we - 1 with the full length) - its 5' k-mer starts within k + 2 of position 0, its 3' k-mer ends within
    # 2 k of L
    for ws in (r - 2, r - 1, r):
        assert (ws, ws + 300) in wins
        f = e.fetched(ws, ws + 300)
        assert (f & (e.fs == ws + 1 - M.MAX_LEN) & (e.fe == ws + 1)).any(), ws
        assert ws + 1 - M.MAX_LEN <= k + 2
    assert [ws - r >= -1 for ws in (r - 2, r - 1, r)] == [False, True, True]
    for we in (L - r - k, L - r - k + 1, L - r - k + 2):
        assert (we - 300, we) in wins
        f = e.fetched(we - 300, we)
        assert (f & (e.fs == we - 1) & (e.fe == we - 1 + M.MAX_LEN)).any(), we
        assert L - (we - 1 + M.MAX_LEN) <= 2 * k + r - M.MAX_LEN
    assert [we + r + k - 1 <= L for we in (L - r - k, L - r - k + 1, L - r - k + 2)] == [True, True, False]


def test_tiles_and_dense(W):
    t = M.tile_windows()
    assert len(t) == 376 and t[0] == (0, 64) and t[-1][0] < M.L_EDGE <= t[-1][1]
    d = W["dense"]
    assert d.L == 4_099 and len(d.fs) == 20_000 and (d.fe - d.fs).max() == M.MAX_LEN
    assert ((np.frombuffer(d.seq.encode(), np.uint8) & 0xDF) == ord("N")).sum() > 0
    wins = M.dense_windows()
    assert len(wins) == 320 and len(set(wins)) == 8 and wins[:8] == M.DENSE_DISTINCT and wins[8:16] == M.DENSE_DISTINCT
    lens = np.array([b - a for a, b in wins])
    assert lens.min() >= 900 and lens.max() <= 1000 and max(b for _, b in wins) == d.L
    # the library's own estimate of candidates per window (features_common): 512-thread blocks from 4096 on
    assert len(d.fs) / int(d.fe.max()) * (lens.mean() + M.MAX_LEN) >= 4096
    assert lens.max() * len(wins) <= 8 * lens.sum()          # windows_suit_block_path
    lt = np.array([b - a for a, b in t])
    assert lt.max() * len(t) <= 8 * lt.sum()
    assert len(W["edge"].fs) / int(W["edge"].fe.max()) * (64 + M.MAX_LEN) < 4096   # 256-thread blocks


def test_end_both_split_against_the_oracle(W):
    """Where ``py_region_motifs`` does not raise for both-strands end motifs, the strand-wise split gives its vector
    and counts no error; where it raises, the split counts at least one.  Windows at both contig ends included: there
    the split must drop the 3' end of a fragment whose 5' k-mer leaves the contig."""
    raised = agreed = 0
    for name in ("edge", "edge_bam"):
        c = W[name]
        L = c.L
        for k in (1, 2, K, 7):
            for ws, we in ((0, 1), (0, k), (-50, 30), (L - 1, L), (L, L + 10), (L - 300, L - 20), (L - 12, L - 9),
                           M.WIN_A, M.WIN_B, (3_001, 3_001), (2_480, 2_520)):
                rows = c.rows_near(ws, we)
                got, n_raise = M.end_both_split(rows, c.seq, ws, we, k, M.Q)
                try:
                    want = O.py_region_motifs(rows, c.seq, ws, we, k, "end", True, False, M.Q)
                except RuntimeError:
                    assert n_raise > 0, (name, k, ws, we)
                    raised += 1
                    continue
                assert n_raise == 0 and np.array_equal(got, want), (name, k, ws, we)
                agreed += 1
    assert raised >= 6 and agreed >= 30
    # [L - 1, L) fetches the fragment [L - 1, L): for k = 2 its 5' k-mer leaves the contig and its 3' k-mer [L - 2, L)
    # is clean - without the drop the split counts it
    c = W["edge"]
    a, b = c.L - 1, c.L
    rows = c.rows_near(a, b)
    assert (a, b) in {(r[0], r[1]) for r in rows} and "N" not in c.seq[c.L - 2:].upper()
    naive = O.py_region_motifs(rows, c.seq, a, b, 2, "end", False, True, M.Q) + \
        O.py_region_motifs([(r[0], r[1], r[2], 1) for r in rows], c.seq, a, b, 2, "end", False, False, M.Q)
    assert naive.sum() > M.end_both_split(rows, c.seq, a, b, 2, M.Q)[0].sum()


def test_odd_k_breakpoint_is_all_zero(W):
    """frag/_breakpoint_motifs.py never launches the kernel for an odd k: the reference's k-mer has 2 (k // 2) bases
    there and none is counted.  The GPU test therefore compares counts for even k only."""
    c = W["edge"]
    for k in (1, 3, 5, 7):
        assert not O.py_region_motifs(c.rows_near(*M.WIN_A), c.seq, *M.WIN_A, k, "breakpoint", True, False, M.Q).any()
