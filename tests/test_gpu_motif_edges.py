"""The motif pass (``ftk_motif_counts``: the general form on FASTA text, the word form on a 2bit image) on the world of
``tests/motif_edges.py``: contig ends, 79 N runs, both sides of motif_stream's per-window range-test switch, the BAM
fetch with read-1 spans that stick out of their fragment, every kernel family (wave per window, chunk walker, 256- and
512-thread block per window).  Counts, fetched fragments and the error count per window against
``oracle.py_region_motifs`` / ``oracle.py_fetch``, exactly.  ``tests/test_motif_edges.py`` asserts that the world holds
the cases named here.

Limits of the library the inputs stay inside, both asserted by the CPU test:
* a BAM fetch finds a fragment through the 512-bp index of the fragment STARTS, from the bin of ws - max_len to the
  end of the bin of we; a read-1 span that reaches a window from a fragment outside that range is not answered.  The
  spans of ``edge_bam`` stick out by up to 400 bases but never that far; the 64-base tiles run on ``edge_bam_inside``.
* an odd k never reaches the kernel for breakpoint motifs (frag/_breakpoint_motifs.py returns zeros, as the oracle
  does): counts are compared for even k, nfrag and err for every k."""
import numpy as np
import pytest

from tests import helpers as H
from tests import motif_edges as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(engine, tmp_path_factory):
    """The contigs on the device and the reference images of both sequences: FASTA at widths 60 and 61, 2bit."""
    from finaletoolkit_amd.reference import ReferenceGenome
    W = M.world()
    d = tmp_path_factory.mktemp("motif_edges")
    seqs = {"edge": W["edge"].seq, "dense": W["dense"].seq}
    H.write_fasta(d / "w60.fa", seqs, width=60)
    H.write_fasta(d / "w61.fa", seqs, width=61)
    H.write_2bit(d / "w.2bit", seqs)
    names = ("edge", "edge_bam", "edge_bam_inside", "dense", "dense_bam")
    for n in names:
        cols, kw = W[n].columns()
        engine.load_contig("me_" + n, *cols, **kw)
        assert engine.info("me_" + n)[:2] == (len(W[n].fs), M.MAX_LEN)
    refs = {p: ReferenceGenome(str(d / p)) for p in ("w60.fa", "w61.fa", "w.2bit")}
    yield W, refs
    for r in refs.values():
        r.close()
    for n in names:
        engine.release("me_" + n)


def run_case(engine, world, name, windows, kind, k, both, neg, images):
    """One case on every image against the oracle; returns the library's first (counts, nfrag, err)."""
    W, refs = world
    ct = W[name]
    want, want_n, want_err = M.expected(ct, windows, kind, k, both, neg)
    spec = M.spec_of(kind, k, both, neg)
    ws, we = np.array([w[0] for w in windows], np.int32), np.array([w[1] for w in windows], np.int32)
    first = None
    for p in images:
        rid = refs[p].device_image(engine, name.split("_")[0])   # (the engine keeps two images: uploaded as needed)
        got, nfrag, err = engine.motif_counts("me_" + name, rid, ws, we, k, both_strands=both,
                                              negative_strand=neg, quality_threshold=M.Q, bam=ct.bam, **spec)
        tag = (name, kind, k, both, neg, p)
        assert np.array_equal(nfrag, want_n), (tag, np.flatnonzero(nfrag != want_n)[:5])
        assert np.array_equal(err, want_err), (tag, np.flatnonzero(err != want_err)[:5])
        if kind == "end" or k % 2 == 0:
            bad = np.flatnonzero((got.astype(np.int64) != want).any(axis=1))
            assert bad.size == 0, (tag, [windows[i] for i in bad[:5]])
        first = first or (got, nfrag, err)
    return first, (want, want_n, want_err)


@pytest.mark.parametrize("kind", ["end", "breakpoint"])
@pytest.mark.parametrize("name", ["edge", "edge_bam"])
def test_small_window_set(engine, world, name, kind):
    """~40 windows (wave-per-window kernel up to k = 5, the chunk walker for [0, L) and for every window from k = 6 on):
    contig ends, empty / reversed / negative windows, single bases at run edges, the 44-run cluster, both sides of the
    range-test switch, and - ``edge_bam`` - the windows read-1 spans reach into from up to 400 bases away."""
    W, _ = world
    max_len = engine.info("me_" + name)[1]
    errs = 0
    for k in range(1, 8):
        windows = M.small_windows(W["runs"], M.L_EDGE, kind, k, max_len)
        assert len(windows) < _cu_count()
        for both, neg in M.STRANDS:
            _, (_, _, want_err) = run_case(engine, world, name, windows, kind, k, both, neg,
                                           ("w60.fa", "w61.fa", "w.2bit"))
            errs += int(want_err.sum())
    assert (errs > 0) == (kind == "end")   # rev_oob_is_error is exercised with a non-zero count


def _cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("kind", ["end", "breakpoint"])
@pytest.mark.parametrize("name", ["edge", "edge_bam_inside"])
def test_tiles_take_the_256_thread_block_kernels(engine, world, name, kind):
    windows = M.tile_windows()
    if len(windows) < _cu_count():
        pytest.skip(f"{len(windows)} tiles are fewer than the device's {_cu_count()} compute units: not the block path")
    for k in (1, 4, 6, 7) if kind == "breakpoint" else (1, 4, 7):
        for both, neg in M.STRANDS:
            run_case(engine, world, name, windows, kind, k, both, neg, ("w60.fa", "w.2bit"))


@pytest.mark.parametrize("kind", ["end", "breakpoint"])
@pytest.mark.parametrize("name", ["dense", "dense_bam"])
def test_dense_windows_take_the_512_thread_block_kernels(engine, world, name, kind):
    windows = M.dense_windows()
    assert len(windows) >= _cu_count()
    for k in (1, 4, 6, 7) if kind == "breakpoint" else (1, 4, 7):
        for both, neg in M.STRANDS:
            (got, nfrag, err), _ = run_case(engine, world, name, windows, kind, k, both, neg, ("w60.fa", "w.2bit"))
            for i in range(8, len(windows)):   # the 40 copies of a window give identical rows
                assert np.array_equal(got[i], got[i % 8]) and nfrag[i] == nfrag[i % 8] and err[i] == err[i % 8]


def test_ref_gc_counts_long_ranges(engine, tmp_path):
    """``ftk_ref_gc_counts`` on ranges of 17 000 - 40 000 bases: more than 4 x 16 x 64 bytes of a 2bit image, so the
    four-rows-per-trip loop of gc_count_kernel runs (the 10 kb ranges of the other tests are 2 500 bytes); every phase
    of lo & 3 and hi & 3, one range up to the image's last, partial byte, the same ranges on FASTA text."""
    from finaletoolkit_amd.reference import ReferenceGenome
    rng = np.random.default_rng(41)
    n = 90_003
    b = rng.choice(np.frombuffer(b"ACGT", np.uint8), n, p=[0.2, 0.3, 0.3, 0.2]).copy()
    b[50_000:50_300] |= 0x20
    seq = b.tobytes().decode()
    H.write_fasta(tmp_path / "g.fa", {"g": seq}, width=70)
    H.write_2bit(tmp_path / "g.2bit", {"g": seq})
    lo = [1_000 + 148 * i + i % 4 for i in range(16)]                                   # lo & 3 = i % 4
    hi = [a + 17_000 + 1_532 * i + (i // 4 - i % 4) % 4 for i, a in enumerate(lo)]      # hi & 3 = i // 4
    lo += [n - 40_000, n - 17_001, 0, 3]
    hi += [n, n, 40_000, n - 1]
    lo, hi = np.array(lo, np.int64), np.array(hi, np.int64)
    assert {(int(a) & 3, int(c) & 3) for a, c in zip(lo[:16], hi[:16])} == {(x, y) for x in range(4) for y in range(4)}
    assert (hi - lo).min() >= 17_000 and np.sort(hi - lo)[-2] == 40_000 and n % 4 == 3 and hi.max() == n
    cg = np.concatenate([[0], np.cumsum(np.isin(b, np.frombuffer(b"GCgc", np.uint8)))])
    want = cg[hi] - cg[lo]
    for path in ("g.2bit", "g.fa"):
        with ReferenceGenome(str(tmp_path / path)) as ref:
            assert np.array_equal(ref.gc_counts(engine, "g", lo, hi), want), path
