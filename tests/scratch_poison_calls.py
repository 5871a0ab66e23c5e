"""
The world, the table of calls and the procedure of tests/test_gpu_scratch_poison.py, and the child process that runs the
procedure for the block-path calls.

    python tests/scratch_poison_calls.py DIR OUT.npz

runs ``procedure`` for every call of CHILD_CALLS in THIS process - whose environment decides the path: with
FTK_FEAT_BLOCK=1 the window features take the one-block-per-window kernels and ftk_window_features_wps its merged launch -
and stores every run's outputs and the scratch sizes in OUT.npz.  Not a test module itself.

Every device-side entry point of the C ABI carves its buffers out of ONE scratch block per context that is never cleared
("What a call may assume about the scratch: nothing").  ``procedure`` runs a call as found, then on a block
filled with 0x00, 0xFF and 0x7F (``Engine.scratch_fill``): every output of every run must be the same bits.  As int32 or
int64, 0xFF.. is -1 and as a double a NaN, and it sets every flag; 0x7F.. is a large positive integer and a large finite
double.  CALLS maps each entry point to ``(run, check, device)``: ``run(x)`` makes the call in the forms that use the
most scratch - its outputs come from ``x.out``, host arrays or device tensors pre-filled with SENTINEL bytes, and it
calls ``x.refill()`` in front of EVERY library call, so that each form of an entry that makes several starts on a
freshly filled block and not on what the form before it left - and returns them; ``check(W, R, eng)`` holds the first
run to the restatement the call's own test module uses, by that module's rule; ``device``: the call takes device
outputs, and a fourth run under 0xFF hands it device tensors (the three fills themselves all run with host outputs, whose
stand-ins live in the scratch).
"""
import ctypes as C
import gzip
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))

from finaletoolkit_amd import _lib as L  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import depth_helpers as DH  # noqa: E402
from tests import end_context_helpers as EC  # noqa: E402
from tests import gc_genome as G  # noqa: E402
from tests import hotspots_helpers as HH  # noqa: E402
from tests import motif_edges as M  # noqa: E402
from tests import packed_columns_child as K  # noqa: E402
from tests import peaks_helpers as PK  # noqa: E402
from tests import prefends_helpers as PH  # noqa: E402
from tests import site_ends_helpers as SE  # noqa: E402
from tests import site_profile_helpers as SP  # noqa: E402
from tests import spectrum_helpers as SH  # noqa: E402
from tests import vplot_helpers as VP  # noqa: E402
from tests import weights_helpers as WH  # noqa: E402
from tests.helpers import write_2bit, write_fasta  # noqa: E402

FILLS = (0x00, 0xFF, 0x7F)
SENTINEL = 0xA5
SIZE = K.SIZE                       # 300 kb
TILE = 4096                         # kWpsTile, kCallTile
A0, B0 = K.A0, K.B0                 # a region that starts off a tile boundary and ends in a partial tile, across EMPTY
QUIET = (K.EMPTY[0] + 1000 + 1, K.EMPTY[1])  # no fragment starts OR ends here ('other' has no fragment over 1000 bases)
N_RUNS = ((0, 137), (150_000, 150_001), (200_000, 200_250), (SIZE - 300, SIZE))
LOWER_RUNS = ((5_000, 5_600), (200_100, 200_400))
FASTA_WIDTH = 61                    # SIZE % 61 == 2: a ragged last line
HIST = (0, 1001)
WIDE_HIST = (100, 2_500)            # more than kHistSmallMaxBins (2048) bins: the histogram rows are cleared by memsets
SMALL_MAX = 1024                    # kSmallMax: a window with more candidates goes to the chunk walker
GC_LENS = (100, 220)
PERIODS = np.arange(120, 281, 7, dtype=np.int32)  # 23 periods
# start off a tile boundary and end in a partial tile; zero-length; inside the quiet stretch; long, ending in a partial tile
IV_START = np.array([4_097, 50_000, 152_000, 200_123], np.int64)
IV_STOP = np.array([4_097 + 3 * TILE + 1_234, 50_000, 156_500, 263_000], np.int64)
FUSED_BINS = (0, 10_007, 29)        # win_start, win_len (>= tile + longest fragment), n_win of ftk_wps_window_features
MOTIF_WINDOWS = (0, 5, 20, 66, 67, 100, 130)  # of the world's windows: 7, with the empty one, the long one, a quiet one
ADJ_W = 200


class World:
    """Everything the calls read, built once from the seeds; nothing here calls the library."""

    def __init__(self, tmp):
        rng = np.random.default_rng(20261021)
        s, e, q = K.make_contig("other")
        if len(s) % 4 == 0:
            s, e, q = s[:-1], e[:-1], q[:-1]
        n = len(s)
        self.s, self.e, self.q, self.n = s, e, q, n
        self.st = rng.integers(0, 2, n).astype(np.uint8)
        # BAM-style read-1 spans: 60 bases at the fragment's own end of its strand
        self.r1s = np.where(self.st == 1, s, np.maximum(e - 60, s)).astype(np.int32)
        self.r1e = np.where(self.st == 1, np.minimum(s + 60, e), e).astype(np.int32)
        self.order = np.arange(n, dtype=np.int32)
        self.fr = O.Frags(s, e, q, self.st)
        self.frb = O.Frags(s, e, q, self.st, self.r1s, self.r1e)
        gs, ge, gq = K.make_contig("main")
        self.g = (gs, ge, gq, rng.integers(0, 2, len(gs)).astype(np.uint8))
        self.frg = O.Frags(*self.g)
        self.w = rng.integers(0, 4 * L.WEIGHT_ONE, n).astype(np.uint32)
        self.w[rng.random(n) < 0.1] = 0
        # the reference: N runs and lower-case runs, as a 2bit record and as FASTA text with a ragged last line
        self.seq = G.make_contig(rng, SIZE, N_RUNS, LOWER_RUNS)
        self.ct = G.Contig("c", self.seq)
        self.bases = EC.Bases(self.seq)
        self.paths = {"2bit": os.path.join(tmp, "poison.2bit"), "fa": os.path.join(tmp, "poison.fa")}
        write_2bit(self.paths["2bit"], {"c": self.seq})
        write_fasta(self.paths["fa"], {"c": self.seq}, width=FASTA_WIDTH)
        # 131 windows (no multiple of 4 or 64): a tiling, one of them empty, one long and over its neighbours
        ws = np.arange(131, dtype=np.int32) * 2290
        we = ws + 2290
        we[5] = ws[5]
        we[20] = ws[20] + 30_000
        self.ws, self.we = ws, we.astype(np.int32)
        self.ws2, self.we2 = K.windows()  # the second item of the batch: 3 windows of 100 kb on contig 'pg'
        # 53 sites, one of them in the quiet stretch, about half flipped, three groups
        self.centres = np.concatenate([rng.integers(2_000, SIZE - 2_000, 52), [157_000]]).astype(np.int32)
        self.flip = (rng.random(53) < 0.5).astype(np.uint8)
        self.groups = rng.integers(0, 3, 53).astype(np.int32)
        self.mask_wl = [(a, a + 2_500) for a in range(1_000, SIZE, 7_000)]
        self.mask_bl = [(a, a + 300) for a in range(2_000, SIZE, 11_000)]
        # float64 score runs for the peak calls: several tiles of 1024, partial tiles, an empty run
        runs = []
        for m in (5_000, 0, 1_500, 9_000):
            i = np.arange(m)
            runs.append(np.rint((3.0 * np.sin(2 * np.pi * i / 190.0) + rng.normal(0, 1, m)) * 8) / 8)
        self.peak_scores, self.peak_offs = PK.pack(runs)
        # median runs for all three kernels (128 bins, 256 bins, the sort) and a run without an output
        def ints(m, lo, span):
            v = lo + rng.integers(0, span + 1, m).astype(np.float64)
            v[0], v[1] = lo, lo + span
            return v
        self.adj_runs = [ints(ADJ_W + 700, -40, 100), ints(ADJ_W + 4_096 + 333, 17, 200), ints(ADJ_W + 900, 3, 1_000),
                         ints(ADJ_W, 0, 50)]
        self._memo = {}

    def memo(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    def wps(self, which="t"):
        """The oracle's WPS of every base of the contig ('t': pt / pb's fragments, 'g': pg's), asked for in pieces: its
        cost grows with the square of the interval."""
        fr = self.fr if which == "t" else self.frg
        return self.memo(("wps", which), lambda: np.concatenate(
            [O.c_wps(fr, a, min(a + 4_000, SIZE), SIZE, 120, 120, 180, 30) for a in range(0, SIZE, 4_000)]))

    def cleavage(self, a, b):
        """(of the very region: its first base is a matter of the region, not of the base alone)"""
        return self.memo(("cleavage", a, b), lambda: O.c_cleavage(self.fr, a, b, None, None, 30)[2])

    def gc(self):
        return self.memo("gc", lambda: self.ct.gc(self.s, self.e))

    def text(self):
        keep = self.q >= 30
        return self.memo("text", lambda: host_rows("chr5", self.s[keep], self.e[keep], self.q[keep], self.st[keep]))

    def bgzf(self):
        def make():
            from finaletoolkit_amd import bgzf
            path = os.path.join(os.path.dirname(self.paths["fa"]), "poison.txt.gz")
            bgzf.write_bgzf(path, self.text(), level=6)
            with open(path, "rb") as fh:
                return fh.read()
        return self.memo("bgzf", make)


def host_rows(name, s, e, q, st):
    from finaletoolkit_amd import writers
    with writers.frag_rows(name, s, e, q, st, False) as rows:
        return rows.tobytes()


def open_engine(W):
    """An Engine of its own (the block's size then depends on these calls alone) with the world resident: 'pt' (tabix
    rule, with a weight column), 'pb' (the same fragments with read-1 spans and an order column), 'pg' (another contig),
    and both reference images."""
    from finaletoolkit_amd.engine import Engine
    from finaletoolkit_amd.reference import ReferenceGenome
    eng = Engine(0)
    eng.load_contig("pt", W.s, W.e, W.q, W.st)
    eng.set_weights("pt", W.w)
    eng.load_contig("pb", W.s, W.e, W.q, W.st, W.r1s, W.r1e)
    eng._check(eng.lib.ftk_frags_set_order(eng.ctx, eng.contig_id("pb"), L.ptr(W.order), W.n))
    eng.load_contig("pg", *W.g)
    W.refs = {k: ReferenceGenome(p) for k, p in W.paths.items()}
    W.rid = {k: r.device_image(eng, "c") for k, r in W.refs.items()}
    import torch  # (its start-up belongs to the setup, not to the first call that takes a device tensor)
    torch.zeros(1, device=f"cuda:{eng.device}")
    torch.cuda.synchronize()
    return eng


# ------------------------------------------------------------------------------------------------------ outputs
class Buf:
    def __init__(self, raw, shape, dtype, nbytes):
        self.raw, self.shape, self.dtype, self.nbytes = raw, shape, np.dtype(dtype), nbytes
        # what a call takes: the typed host array, or the device tensor (passed by address)
        self.a = raw if hasattr(raw, "data_ptr") else raw[:nbytes].view(dtype).reshape(shape)
        self.p = L.ptr(raw)


class Run:
    """One run of one call: hands out its outputs - host arrays, or device tensors when ``device`` - filled with SENTINEL
    bytes, and brings them home."""

    def __init__(self, eng, W, device=False, byte=None):
        self.eng, self.W, self.device, self.byte, self.sizes = eng, W, device, byte, []

    def refill(self):
        """In front of EVERY library call of a run: the block filled again with the run's byte, so that no call of a
        run that makes several starts on what the one before it left (the first run, as found, fills nothing)."""
        if self.byte is not None:
            self.sizes.append(self.eng.scratch_fill(self.byte))

    def out(self, shape, dtype):
        shape = tuple(int(v) for v in np.atleast_1d(shape))
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if self.device:
            import torch
            raw = torch.full((max(nbytes, 8),), SENTINEL, dtype=torch.uint8, device=f"cuda:{self.eng.device}")
            torch.cuda.synchronize()  # (the fill runs on torch's stream, the call on the context's)
        else:
            raw = np.full(max(nbytes, 8), SENTINEL, np.uint8)
        return Buf(raw, shape, dtype, nbytes)

    def get(self, b):
        if isinstance(b, Buf):
            if self.device:
                self.eng.sync()
                return b.raw.cpu().numpy()[:b.nbytes].view(b.dtype).reshape(b.shape).copy()
            return b.a.copy()
        return np.ascontiguousarray(b)

    def ret(self, **outs):
        return {k: self.get(v) for k, v in outs.items()}


def same_bits(a, b):
    """Every output array equal bit for bit (floats as their integer views: NaN included)."""
    if sorted(a) != sorted(b):
        return False
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in a)


def differing(a, b):
    """``{output: cells that differ}`` of two runs (-1: a missing output, another dtype or shape)."""
    out = {}
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b or a[k].dtype != b[k].dtype or a[k].shape != b[k].shape:
            out[k] = -1
        elif a[k].tobytes() != b[k].tobytes():
            out[k] = int((a[k].view(np.uint8).reshape(a[k].size, -1) != b[k].view(np.uint8).reshape(b[k].size, -1)).any(axis=1).sum())
    return out


def fill_runs(name):
    """``[(tag, byte, device)]``: host outputs under each of FILLS - all three patterns reach the stand-ins of host
    outputs - and, for a call that takes device outputs, device tensors once more under 0xFF."""
    runs = [(hex(b), b, False) for b in FILLS]
    return runs + [("0xff device", 0xFF, True)] if CALLS[name][2] else runs


def procedure(eng, W, name):
    """``(R, S, runs, sizes)``: the call as found, then every run of ``fill_runs`` with the block filled in front of each
    library call it makes - again when a call grew the block, so that every compared run starts on a filled block of
    the final size.  ``sizes[tag]``: the block's size behind the run, -1 when one of its fills met another size than
    ``S`` or the block was still growing at the last try."""
    run = CALLS[name][0]
    R = run(Run(eng, W))
    S = eng.scratch_fill(None)
    runs, sizes = {}, {}
    for tag, byte, device in fill_runs(name):
        for _ in range(3):
            x = Run(eng, W, device, byte)
            got = run(x)
            size = eng.scratch_fill(None)
            steady = size == S and len(x.sizes) > 0 and all(s == S for s in x.sizes)
            if steady:
                break
            S = size
        runs[tag], sizes[tag] = got, size if steady else -1
    return R, S, runs, sizes


def records(x, rec, prefix):
    return {f"{prefix}{f}": np.ascontiguousarray(rec[f]) for f in rec.dtype.names}


def equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist())


# ------------------------------------------------------------------------------------------------------ window calls
def _flt(eng, name, policy="midpoint"):
    return eng._filter(name, 30, None, None, policy)


def _delfi_args(W):
    g = L.make_gaps(K.GAPS)
    return g, (30, L.ptr(K.BL_START), L.ptr(K.BL_END), len(K.BL_START), C.byref(g))


def run_window_counts(x):
    out = x.out(len(x.W.ws), np.int64)
    x.refill()
    x.eng.window_counts("pb", x.W.ws, x.W.we, 30, out=out.a)
    return x.ret(count=out)


def check_window_counts(W, R, eng):
    equal(R["count"], O.c_window_counts(W.frb, W.ws, W.we, mapq_min=30), "count")


def run_delfi_counts(x):
    W, eng, n = x.W, x.eng, len(x.W.ws)
    sh, lg, nf = (x.out(n, np.int64) for _ in range(3))
    g, tail = _delfi_args(W)
    x.refill()
    eng._check(eng.lib.ftk_delfi_counts(eng.ctx, eng.contig_id("pt"), L.ptr(W.ws), L.ptr(W.we), n, *tail, sh.p, lg.p, nf.p))
    return x.ret(short=sh, long=lg, nfrag=nf)


def _delfi_want(W, fr, ws, we, plain=False):
    return O.c_delfi_counts(fr, ws, we, 30, None if plain else K.BL_START, None if plain else K.BL_END, None if plain else K.GAPS)


def check_delfi_counts(W, R, eng):
    for k, want in zip(("short", "long", "nfrag"), _delfi_want(W, W.fr, W.ws, W.we)):
        equal(R[k], want, k)


def run_fraglen_hist(x):
    W, eng, n = x.W, x.eng, len(x.W.ws)
    hist, over = x.out((n, HIST[1]), np.uint32), x.out(n, np.int64)
    f = _flt(eng, "pt")
    x.refill()
    eng._check(eng.lib.ftk_fraglen_hist(eng.ctx, eng.contig_id("pt"), L.ptr(W.ws), L.ptr(W.we), n, C.byref(f), *HIST, hist.p, over.p))
    # more bins than the wave-per-window pass takes (kHistSmallMaxBins = 2048): the rows are cleared by two memsets
    wide, wide_over = x.out((n, WIDE_HIST[1]), np.uint32), x.out(n, np.int64)
    x.refill()
    eng._check(eng.lib.ftk_fraglen_hist(eng.ctx, eng.contig_id("pt"), L.ptr(W.ws), L.ptr(W.we), n, C.byref(f), *WIDE_HIST, wide.p, wide_over.p))
    return x.ret(hist=hist, overflow=over, wide_hist=wide, wide_overflow=wide_over)


def check_fraglen_hist(W, R, eng):
    want_h, want_o = O.c_fraglen_hist(W.fr, W.ws, W.we, *HIST, mapq_min=30)
    equal(R["hist"], want_h, "hist")
    equal(R["overflow"], want_o, "overflow")
    want_h, want_o = O.c_fraglen_hist(W.fr, W.ws, W.we, *WIDE_HIST, mapq_min=30)
    equal(R["wide_hist"], want_h, "wide_hist")
    equal(R["wide_overflow"], want_o, "wide_overflow")
    assert want_o.any() and want_h.any()  # (lengths below the first bin count as overflow)


def run_fraglen_stats(x):
    W, eng, n = x.W, x.eng, len(x.W.ws)
    out = x.out((n, 7), np.float64)
    f = _flt(eng, "pt")
    x.refill()
    eng._check(eng.lib.ftk_fraglen_stats(eng.ctx, eng.contig_id("pt"), L.ptr(W.ws), L.ptr(W.we), n, C.byref(f), *HIST, 150, out.p))
    return x.ret(stats=out)


def check_fraglen_stats(W, R, eng):
    """The rule of test_fraglen_stats_on_the_device_equal_the_reference_formulas (tests/test_gpu_parity.py)."""
    import pytest
    hist, over = O.c_fraglen_hist(W.fr, W.ws, W.we, *HIST, mapq_min=30)
    assert not over.any()
    got = R["stats"]
    for k in range(len(W.ws)):
        nz = np.nonzero(hist[k])[0]
        if len(nz) == 0:
            assert got[k, 5] == 0, k
            continue
        want = O.py_frag_length_stats({int(b) + HIST[0]: int(hist[k][b]) for b in nz}, 150)
        assert got[k, 0] == want[0] and got[k, 1] == want[1], (k, got[k], want)
        assert got[k, 2] == pytest.approx(want[2], rel=1e-12, abs=1e-12)
        assert (got[k, 3], got[k, 4], got[k, 5]) == (want[3], want[4], want[5])
        assert got[k, 6] == round(want[6] * want[5])


def _feature_outs(x, n):
    return dict(coverage=x.out(n, np.int64), hist=x.out((n, HIST[1]), np.uint32), overflow=x.out(n, np.int64),
                short=x.out(n, np.int64), long=x.out(n, np.int64))


def _check_features(W, R, fr, ws, we, rows=slice(None), plain=False, prefix=""):
    hist, over = O.c_fraglen_hist(fr, ws, we, *HIST, mapq_min=30)
    sh, lg, _ = _delfi_want(W, fr, ws, we, plain)
    want = dict(coverage=O.c_window_counts(fr, ws, we, mapq_min=30), hist=hist, overflow=over, short=sh, long=lg)
    for k, v in want.items():
        equal(R[prefix + k][rows], v, prefix + k)


def run_window_features(x):
    W, eng, n = x.W, x.eng, len(x.W.ws)
    o = _feature_outs(x, n)
    f = _flt(eng, "pt")
    g, tail = _delfi_args(W)
    x.refill()
    eng._check(eng.lib.ftk_window_features(eng.ctx, eng.contig_id("pt"), L.ptr(W.ws), L.ptr(W.we), n, C.byref(f), o["coverage"].p,
                                           *HIST, o["hist"].p, o["overflow"].p, *tail, o["short"].p, o["long"].p))
    return x.ret(**o)


def check_window_features(W, R, eng):
    _check_features(W, R, W.fr, W.ws, W.we)


def run_window_features_batch(x):
    W, eng = x.W, x.eng
    batch = eng.feature_batch([dict(name="pt", starts=W.ws, stops=W.we, bl_start=K.BL_START, bl_end=K.BL_END, gaps=K.GAPS),
                               dict(name="pg", starts=W.ws2, stops=W.we2)], 30)
    o = _feature_outs(x, batch["rows"])
    x.refill()
    eng.window_features_batch(batch, coverage=o["coverage"].a, hist=o["hist"].a, hist_bins=HIST, overflow=o["overflow"].a,
                              delfi_q=30, short=o["short"].a, long=o["long"].a)
    return x.ret(**o)


def check_window_features_batch(W, R, eng):
    n = len(W.ws)
    _check_features(W, R, W.fr, W.ws, W.we, slice(0, n))
    _check_features(W, R, W.frg, W.ws2, W.we2, slice(n, n + len(W.ws2)), plain=True)


def run_window_features_wps(x):
    W, eng, n = x.W, x.eng, len(x.W.ws)
    o = _feature_outs(x, n)
    wps = x.out(B0 - A0, np.int64)
    x.refill()
    eng.window_features_wps("pt", W.ws, W.we, wps.a, A0, B0, SIZE, 30, coverage=o["coverage"].a, hist=o["hist"].a, hist_bins=HIST,
                            overflow=o["overflow"].a, delfi_q=30, bl_start=K.BL_START, bl_end=K.BL_END, gaps=K.GAPS,
                            short=o["short"].a, long=o["long"].a)
    return x.ret(wps=wps, **o)


def check_window_features_wps(W, R, eng):
    _check_features(W, R, W.fr, W.ws, W.we)
    equal(R["wps"], W.wps()[A0:B0], "wps")


def _fused_windows():
    ws = (FUSED_BINS[0] + np.arange(FUSED_BINS[2]) * FUSED_BINS[1]).astype(np.int32)
    return ws, (ws + FUSED_BINS[1]).astype(np.int32)


def run_wps_window_features(x):
    W, eng = x.W, x.eng
    o = _feature_outs(x, FUSED_BINS[2])
    wps = x.out(SIZE, np.int64)
    x.refill()
    eng.wps_window_features("pt", SIZE, *FUSED_BINS, wps_out=wps.a, coverage=o["coverage"].a, hist=o["hist"].a, hist_bins=HIST,
                            overflow=o["overflow"].a, delfi_q=30, bl_start=K.BL_START, bl_end=K.BL_END, gaps=K.GAPS,
                            short=o["short"].a, long=o["long"].a)
    return x.ret(wps=wps, **o)


def check_wps_window_features(W, R, eng):
    _check_features(W, R, W.fr, *_fused_windows())
    equal(R["wps"], W.wps(), "wps")


# ------------------------------------------------------------------------------------------------------ selection
SELECT = (20_000, 140_000)


def run_frag_lengths(x):
    x.refill()
    return x.ret(lengths=x.eng.frag_lengths("pb", *SELECT, 30))


def check_frag_lengths(W, R, eng):
    s, e, _, _ = O.c_frag_select(W.frb, *SELECT, mapq_min=30)
    assert len(s) > 4 * 256  # more candidates than a few blocks of the count pass
    equal(R["lengths"], e - s, "lengths")


def run_frag_select(x):
    x.refill()
    s, e, q, st = x.eng.frag_select("pb", *SELECT, 30)
    return x.ret(start=s, end=e, mapq=q, strand=st)


def check_frag_select(W, R, eng):
    for k, want in zip(("start", "end", "mapq", "strand"), O.c_frag_select(W.frb, *SELECT, mapq_min=30)):
        equal(R[k], want, k)


# ------------------------------------------------------------------------------------------------------ per-base calls
def _iv_offsets(gap=0):
    lens = np.maximum(IV_STOP - IV_START, 0)
    offs = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens + gap, out=offs[1:])
    return lens, offs


def _iv_slices(track):
    return np.concatenate([track[a:b] for a, b in zip(IV_START, IV_STOP)])


def run_wps(x):
    out = x.out(B0 - A0, np.int64)
    x.refill()
    x.eng.wps("pt", A0, B0, SIZE, out=out.a)
    return x.ret(wps=out)


def check_wps(W, R, eng):
    equal(R["wps"], W.wps()[A0:B0], "wps")
    assert not R["wps"][QUIET[0] + 200 - A0:QUIET[1] - 200 - A0].any() and R["wps"].any()  # whole tiles without a candidate


def run_wps_intervals(x):
    eng = x.eng
    _, offs = _iv_offsets()
    out = x.out(int(offs[-1]), np.int64)
    x.refill()
    eng._check(eng.lib.ftk_wps_intervals(eng.ctx, eng.contig_id("pt"), L.ptr(IV_START), L.ptr(IV_STOP), len(IV_START),
                                         L.ptr(np.ascontiguousarray(offs[:-1])), SIZE, 120, 120, 180, 30, out.p))
    return x.ret(wps=out)


def check_wps_intervals(W, R, eng):
    equal(R["wps"], _iv_slices(W.wps()), "wps")


BATCH = (("pt", 4_097, 20_000), ("pg", 100_001, 130_000), ("pt", 150_000, 150_000), ("pt", 250_000, 262_144 + 5))


def run_wps_batch(x):
    lens = np.array([b - a for _, a, b in BATCH], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)])
    out = x.out(int(offs[-1]), np.int64)
    x.refill()
    x.eng.wps_batch([n for n, _, _ in BATCH], [a for _, a, _ in BATCH], [b for _, _, b in BATCH], [SIZE] * len(BATCH), offs[:-1], out.a)
    return x.ret(wps=out)


def check_wps_batch(W, R, eng):
    equal(R["wps"], np.concatenate([W.wps("t" if n == "pt" else "g")[a:b] for n, a, b in BATCH]), "wps")


def run_cleavage(x):
    out = x.out(B0 - A0, np.float64)
    x.refill()
    x.eng.cleavage("pt", A0, B0, None, None, 30, out=out.a)
    return x.ret(cleavage=out)


def check_cleavage(W, R, eng):
    equal(R["cleavage"], W.cleavage(A0, B0), "cleavage")


def run_cleavage_intervals(x):
    eng = x.eng
    _, offs = _iv_offsets()
    out = x.out(int(offs[-1]), np.float64)
    x.refill()
    eng._check(eng.lib.ftk_cleavage_intervals(eng.ctx, eng.contig_id("pt"), L.ptr(IV_START), L.ptr(IV_STOP), len(IV_START),
                                              L.ptr(np.ascontiguousarray(offs[:-1])), L.LEN_OPEN, L.LEN_OPEN, 30, out.p))
    return x.ret(cleavage=out)


def check_cleavage_intervals(W, R, eng):
    equal(R["cleavage"], np.concatenate([W.cleavage(int(a), int(b)) for a, b in zip(IV_START, IV_STOP)]), "cleavage")


def run_wps_adjust(x):
    """Two calls: the median alone over runs for all three kernels and a run without an output (which the Savitzky-Golay
    pass refuses), then the median and the Savitzky-Golay pass over the others - the form with the most buffers."""
    W, eng = x.W, x.eng
    raw, offs = PK.pack(W.adj_runs)
    n_out = int(offs[-1]) - len(W.adj_runs) * ADJ_W
    med = x.out(n_out, np.float64)
    x.refill()
    eng.wps_adjust(raw, offs, ADJ_W, savgol=False, out=med.a)
    raw3, offs3 = PK.pack(W.adj_runs[:3])
    sub = np.array([float(np.mean(v[:50])) for v in W.adj_runs[:3]])
    sg = x.out(int(offs3[-1]) - 3 * ADJ_W, np.float64)
    x.refill()
    eng.wps_adjust(raw3, offs3, ADJ_W, edge_sub=sub, out=sg.a)
    return x.ret(median=med, savgol=sg)


def check_wps_adjust(W, R, eng):
    """The median exactly, the Savitzky-Golay pass within tests/test_adjust_wps.py's TOL."""
    # integers within 30 000 of one another: a range below 128 takes the 128-bin histogram, below 256 the 256-bin one, a
    # wider one the sort (adjust_median_hist_tile)
    assert [int(np.ptp(v)) for v in W.adj_runs[:3]] == [100, 200, 1_000] and len(W.adj_runs[3]) == ADJ_W
    at = 0
    for v in W.adj_runs:
        want = O.py_adjust_run(v, ADJ_W, savgol=False)
        equal(R["median"][at:at + len(want)], want, "median")
        at += len(want)
    assert at == len(R["median"])
    at = 0
    for v in W.adj_runs[:3]:
        want = O.py_adjust_run(v - float(np.mean(v[:50])), ADJ_W)
        np.testing.assert_allclose(R["savgol"][at:at + len(want)], want, rtol=1e-9, atol=1e-9)
        at += len(want)


# ------------------------------------------------------------------------------------------------------ reference calls
GC_RANGES = (np.array([0, 100, 137, 149_990, 199_000, 250_001, SIZE - 400], np.int64),
             np.array([137, 4_196, 138, 150_011, 201_000, 250_001, SIZE], np.int64))


def run_ref_gc_counts(x):
    eng, outs = x.eng, {}
    lo, hi = GC_RANGES
    for image in ("2bit", "fa"):
        if image == "fa":  # bases -> bytes of the text
            lo, hi = ((v // FASTA_WIDTH) * (FASTA_WIDTH + 1) + v % FASTA_WIDTH for v in GC_RANGES)
        out = x.out(len(lo), np.int64)
        x.refill()
        eng._check(eng.lib.ftk_ref_gc_counts(eng.ctx, x.W.rid[image], L.ptr(np.ascontiguousarray(lo)), L.ptr(np.ascontiguousarray(hi)),
                                             len(lo), out.p))
        outs[image] = out
    return x.ret(**outs)


def check_ref_gc_counts(W, R, eng):
    want = W.ct.cg[GC_RANGES[1]] - W.ct.cg[GC_RANGES[0]]  # (an N is packed as T and is no G or C in the text either)
    equal(R["2bit"], want, "2bit")
    equal(R["fa"], want, "fa")


def run_motif_counts(x):
    W, eng, outs = x.W, x.eng, {}
    ws, we = W.ws[list(MOTIF_WINDOWS)], W.we[list(MOTIF_WINDOWS)]
    for image in ("2bit", "fa"):
        for k in (4, 6):  # the LDS histogram of up to 4^5 bins, and the wide one
            m = L.Motif(k, 0, -k, 1, 0, 0, 1)  # tests/motif_edges.py, spec_of("end", k, True, False)
            counts, nfrag, err = x.out((len(ws), 4 ** k), np.uint32), x.out(len(ws), np.int64), x.out(len(ws), np.int64)
            x.refill()
            eng._check(eng.lib.ftk_motif_counts(eng.ctx, eng.contig_id("pt"), W.rid[image], L.ptr(ws), L.ptr(we), len(ws), C.byref(m), 30,
                                                L.FETCH_TABIX, counts.p, nfrag.p, err.p))
            outs.update({f"{image}{k}_counts": counts, f"{image}{k}_nfrag": nfrag, f"{image}{k}_err": err})
    return x.ret(**outs)


def check_motif_counts(W, R, eng):
    assert M.spec_of("end", 4, True, False) == dict(fwd_offset=0, rev_offset=-4, guard=0, rev_oob_is_error=True)
    for k in (4, 6):
        counts, nfrag = [], []
        for i in MOTIF_WINDOWS:
            a, b = int(W.ws[i]), int(W.we[i])
            lo, hi = np.searchsorted(W.s, a - 1_001), np.searchsorted(W.s, max(a, b) + 1)
            rows = list(zip(W.s[lo:hi].tolist(), W.e[lo:hi].tolist(), W.q[lo:hi].tolist(), W.st[lo:hi].tolist()))
            nfrag.append(sum(1 for _ in O.py_fetch(rows, a, b, 30)))
            counts.append(O.py_region_motifs(rows, W.seq, a, b, k, "end", True, False, 30))  # (no fragment leaves the contig)
        assert nfrag[3] == 0 and max(nfrag) > 1_000  # the quiet window fetches nothing
        for image in ("2bit", "fa"):
            equal(R[f"{image}{k}_counts"], np.stack(counts), (image, k, "counts"))
            equal(R[f"{image}{k}_nfrag"], nfrag, (image, k, "nfrag"))
            assert not R[f"{image}{k}_err"].any()


# ------------------------------------------------------------------------------------------------------ depth
def run_depth(x):
    out = x.out(B0 - A0, np.int32)
    x.refill()
    x.eng.depth("pt", A0, B0, 30, out=out.a)
    return x.ret(depth=out)


def _depth_want(W):
    return W.memo("depth", lambda: DH.restated_depth(W.s, W.e, DH.kept(W.s, W.e, W.q, 30), A0, B0))


def check_depth(W, R, eng):
    equal(R["depth"], _depth_want(W), "depth")
    assert not R["depth"][QUIET[0] - A0:QUIET[1] - A0].any()


def run_depth_runs(x):
    out = {}
    for zero in (False, True):
        x.refill()
        rs, re_, rd = x.eng.depth_runs("pt", A0, B0, 30, include_zero=zero)
        out.update({f"start{int(zero)}": rs, f"end{int(zero)}": re_, f"depth{int(zero)}": rd})
    return x.ret(**out)


def check_depth_runs(W, R, eng):
    for zero in (False, True):
        want = DH.restated_runs(_depth_want(W), A0, zero)
        got = tuple(R[f"{k}{int(zero)}"] for k in ("start", "end", "depth"))
        for g, w_, k in zip(got, want, ("start", "end", "depth")):
            equal(g, w_, (k, zero))
        DH.check_invariants(got, A0, B0, zero, W.s, W.e, DH.kept(W.s, W.e, W.q, 30))


# ------------------------------------------------------------------------------------------------------ GC bias
def run_frag_gc(x):
    outs = {}
    for image in ("2bit", "fa"):
        outs[image] = x.out(x.W.n, np.int16)
        x.refill()
        x.eng.frag_gc("pt", x.W.rid[image], 30, out=outs[image].a)
    return x.ret(**outs)


def check_frag_gc(W, R, eng):
    want = np.where(W.q >= 30, W.gc(), -1).astype(np.int16)
    assert (want >= 0).sum() > 5_000 and ((want < 0) & (W.q >= 30)).sum() > 5  # spans over an N run are there
    equal(R["2bit"], want, "2bit")
    equal(R["fa"], want, "fa")


def _gc_table_shape():
    return (GC_LENS[1] - GC_LENS[0] + 1, GC_LENS[1] + 1)


def run_frag_gc_table(x):
    eng, outs = x.eng, {}
    for image in ("2bit", "fa"):
        table, skipped = x.out(_gc_table_shape(), np.int64), C.c_int64(-7)
        x.refill()
        eng._check(eng.lib.ftk_frag_gc_table(eng.ctx, eng.contig_id("pt"), x.W.rid[image], *GC_LENS, 30, table.p, C.byref(skipped)))
        outs[image], outs[image + "_skipped"] = table, np.array([skipped.value])
    return x.ret(**outs)


def check_frag_gc_table(W, R, eng):
    """The bincount of test_frag_gc_table_is_the_bincount (tests/test_gpu_frag_gc_bias.py)."""
    ln = W.e.astype(np.int64) - W.s
    keep = (W.q >= 30) & (ln >= GC_LENS[0]) & (ln <= GC_LENS[1])
    ok = keep & (W.gc() >= 0)
    want = np.zeros(_gc_table_shape(), np.int64)
    np.add.at(want, (ln[ok] - GC_LENS[0], W.gc()[ok]), 1)
    for image in ("2bit", "fa"):
        equal(R[image], want, image)
        assert R[image + "_skipped"][0] == int((keep & ~ok).sum())


def run_ref_gc_table(x):
    eng, outs = x.eng, {}
    for image in ("2bit", "fa"):
        outs[image] = x.out(_gc_table_shape(), np.int64)
        x.refill()
        eng._check(eng.lib.ftk_ref_gc_table(eng.ctx, x.W.rid[image], 0, SIZE, *GC_LENS, 1, outs[image].p))
    return x.ret(**outs)


def check_ref_gc_table(W, R, eng):
    want = W.ct.expected(*GC_LENS)
    equal(R["2bit"], want, "2bit")
    equal(R["fa"], want, "fa")


def _weight_table():
    t = np.random.default_rng(5).integers(1, 2 ** 32, _gc_table_shape(), dtype=np.uint64).astype(np.uint32)
    t[::7, ::5] = 0
    return t


def run_gc_weights(x):
    """ftk_frags_set_gc_weights, then ftk_frags_weights (the column itself is the contig's, not scratch)."""
    eng, gs = x.eng, x.W.g[0]
    x.refill()
    n_zero = eng.set_gc_weights("pg", x.W.rid["2bit"], *GC_LENS, _weight_table(), 30)
    out = x.out(len(gs), np.uint32)
    x.refill()
    eng.weights("pg", out=out.a)
    return x.ret(n_zero=np.array([n_zero]), weights=out)


def check_gc_weights(W, R, eng):
    """restated_column of tests/test_gpu_gc_weights.py."""
    s, e, q, _ = W.g
    ln = e.astype(np.int64) - s
    rule = (q >= 30) & (ln >= GC_LENS[0]) & (ln <= GC_LENS[1])
    gc = W.ct.gc(s, e)
    ok = rule & (gc >= 0)
    want = np.zeros(len(s), np.uint32)
    want[ok] = _weight_table()[ln[ok] - GC_LENS[0], gc[ok]]
    equal(R["weights"], want, "weights")
    assert R["n_zero"][0] == int((rule & (want == 0)).sum()) and (want > 0).sum() > 1_000


def run_weighted_window_sums(x):
    W, eng, n = x.W, x.eng, len(x.W.ws)
    sums, cnt = x.out(n, np.int64), x.out(n, np.int64)
    f = _flt(eng, "pt")
    x.refill()
    eng._check(eng.lib.ftk_weighted_window_sums(eng.ctx, eng.contig_id("pt"), L.ptr(W.ws), L.ptr(W.we), n, C.byref(f), sums.p, cnt.p))
    return x.ret(sums=sums, n_weighted=cnt)


def check_weighted_window_sums(W, R, eng):
    dup = np.zeros(W.n, bool)
    dup[0] = True  # (the helper wants a run of copies: a run of one)
    want = WH.restated_sums((W.s.astype(np.int64), W.e.astype(np.int64), W.q, W.s, W.e, dup), W.w, W.ws.tolist(), W.we.tolist(), 30,
                            None, None, "midpoint", False)
    equal(R["sums"], want[0], "sums")
    equal(R["n_weighted"], want[1], "n_weighted")
    assert want[0].max() > 0


# ------------------------------------------------------------------------------------------------------ site calls
SITE_H, SITE_B = 1_000, 8           # 250 bins
VPLOT = (500, 10, 50, 349, 5)       # half_width, bin_size, len_lo, len_hi, len_bin: 60 rows x 100 bins
ENDS_PEAK, ENDS_FLANK = 60, 10


def _sites(x):
    """(the leading arguments of a site call, what keeps their arrays alive)"""
    return x.eng._site_inputs(x.W.centres, x.W.flip, x.W.groups)


def run_site_profile(x):
    eng = x.eng
    shape = (3, 2 * SITE_H // SITE_B)
    sums, counts = x.out(shape, np.int64), x.out(shape, np.int64)
    sites, alive = _sites(x)
    x.refill()
    eng._check(eng.lib.ftk_site_profile(eng.ctx, eng.contig_id("pt"), *sites, 3, SITE_H, SITE_B, 30, 100, 400, 1, sums.p, counts.p))
    return x.ret(sums=sums, counts=counts)


def check_site_profile(W, R, eng):
    want = SP.restated_profile((W.s, W.e, W.q), W.w, W.centres, W.flip, W.groups, 3, SITE_H, SITE_B, 30, 100, 400)
    equal(R["sums"], want[0], "sums")
    equal(R["counts"], want[1], "counts")
    assert want[1].sum() > 1_000


def run_site_vplot(x):
    eng = x.eng
    h, b, lo, hi, lb = VPLOT
    shape = (3, (hi - lo + 1) // lb, 2 * h // b)
    sums, counts = x.out(shape, np.int64), x.out(shape, np.int64)
    sites, alive = _sites(x)
    x.refill()
    eng._check(eng.lib.ftk_site_vplot(eng.ctx, eng.contig_id("pt"), *sites, 3, h, b, lo, hi, lb, 30, 1, sums.p, counts.p))
    return x.ret(sums=sums, counts=counts)


def check_site_vplot(W, R, eng):
    VP.assert_same((R["sums"], R["counts"]), VP.restated_vplot((W.s, W.e, W.q), W.w, W.centres, W.flip, W.groups, 3, *VPLOT, 30), "vplot")


def run_site_ends(x):
    eng, n = x.eng, len(x.W.centres)
    shape = (3, 2, 2 * SITE_H // SITE_B)
    sums, counts, ss, sc = x.out(shape, np.int64), x.out(shape, np.int64), x.out((n, 4), np.int64), x.out((n, 4), np.int64)
    sites, alive = _sites(x)
    x.refill()
    eng._check(eng.lib.ftk_site_ends(eng.ctx, eng.contig_id("pt"), *sites, 3, SITE_H, SITE_B, 30, 100, 400, 1, ENDS_PEAK, ENDS_FLANK,
                                     sums.p, counts.p, ss.p, sc.p))
    return x.ret(sums=sums, counts=counts, site_sums=ss, site_counts=sc)


def check_site_ends(W, R, eng):
    want = SE.restated_site_ends((W.s, W.e, W.q), W.w, W.centres, W.flip, W.groups, 3, SITE_H, SITE_B, 30, 100, 400, ENDS_PEAK, ENDS_FLANK)
    SE.assert_same((R["sums"], R["counts"], R["site_sums"], R["site_counts"]), want, "site ends")


# ------------------------------------------------------------------------------------------------------ spectrum, peaks
def _spectrum_outs(x):
    return x.out((len(IV_START), len(PERIODS), 2), np.float64), x.out(len(IV_START), np.float64)


def _check_spectrum(W, R):
    """Every component within spectrum_helpers.component_tolerance of the float64 restatement."""
    got = R["spectrum"][..., 0] + 1j * R["spectrum"][..., 1]
    for i, (a, b) in enumerate(zip(IV_START, IV_STOP)):
        SH.assert_spectrum_close(got[i], R["ssw"][i], W.wps()[a:b], PERIODS, 0.1, True, i)


def run_track_spectrum(x):
    """Runs on both sides of the LDS limit (at most _lib.SPECTRUM_TILE samples are folded out of LDS) and an empty one."""
    _, offs = _iv_offsets()
    out, ssw = _spectrum_outs(x)
    x.refill()
    x.eng.track_spectrum(_iv_slices(x.W.wps()), offs, PERIODS, out=out.a, ssw_out=ssw.a)
    return x.ret(spectrum=out, ssw=ssw)


def check_track_spectrum(W, R, eng):
    lens = _iv_offsets()[0]
    assert lens.min() == 0 and sorted(lens)[1] < L.SPECTRUM_TILE < lens.max()
    _check_spectrum(W, R)


def run_wps_spectrum(x):
    out, ssw = _spectrum_outs(x)
    x.refill()
    x.eng.wps_spectrum("pt", IV_START, IV_STOP, SIZE, PERIODS, batch_bases=40_000, out=out.a, ssw_out=ssw.a)  # (two batches)
    return x.ret(spectrum=out, ssw=ssw)


def check_wps_spectrum(W, R, eng):
    _check_spectrum(W, R)


PEAKS = dict(skip=10, max_gap=5, min_region=50, short_max=150, max_region=450)


def run_track_peaks(x):
    eng, offs = x.eng, x.W.peak_offs
    n_runs = len(offs) - 1
    stats = x.out((n_runs, 6), np.int64)  # (host or device; the calls come home in blocks of the library's)
    x.refill()
    calls, = eng._library_records(lambda *out: eng.lib.ftk_track_peaks(
        eng.ctx, L.ptr(x.W.peak_scores), L.ptr(offs), n_runs, PEAKS["skip"], PEAKS["max_gap"], PEAKS["min_region"], PEAKS["short_max"],
        PEAKS["max_region"], *out, stats.p), eng.PEAK_DTYPE)
    return x.ret(stats=stats, **records(x, calls, "call_"))


def _calls_of(R, dtype):
    rec = np.zeros(len(R["call_" + dtype.names[0]]), dtype)
    for f in dtype.names:
        rec[f] = R["call_" + f]
    return rec


def check_track_peaks(W, R, eng):
    want, stats = PK.peaks_ref_runs(W.peak_scores, W.peak_offs, **PEAKS)
    assert len(want) > 20 and PK.same_calls(_calls_of(R, PK.PEAK_DTYPE), want)
    equal(R["stats"], stats, "stats")


def run_wps_peaks(x):
    x.refill()
    calls, stats = x.eng.wps_peaks("pt", IV_START, IV_STOP, SIZE, batch_bases=40_000)
    return x.ret(stats=stats, **records(x, calls, "call_"))


def check_wps_peaks(W, R, eng):
    """Interval by interval: the restatement on Engine.wps_adjust's track, as tests/test_gpu_wps_peaks.py holds it."""
    got = _calls_of(R, PK.PEAK_DTYPE)
    for i, (a, b) in enumerate(zip(IV_START.tolist(), IV_STOP.tolist())):
        mine = got[got["run"] == i]
        if b - a < 1_021:
            assert len(mine) == 0 and not R["stats"][i].any()
            continue
        adj = eng.wps_adjust(W.wps()[a:b].astype(np.float64), [0, b - a])
        calls, stats = PK.peaks_ref(adj, skip=10)
        equal(R["stats"][i], stats, ("stats", i))
        want = np.array([(i, s + a + 500, e + a + 500, t + a + 500, h, ar) for s, e, t, h, ar in calls], PK.PEAK_DTYPE)
        assert PK.same_calls(mine, want), i
    assert len(got) > 50


# ------------------------------------------------------------------------------------------------------ tile calls
def run_preferred_ends(x):
    x.refill()
    calls, stats = x.eng.preferred_ends("pt", IV_START, IV_STOP, SIZE, half=500, mode="split", thresholds=PH.flat_table(1))
    return x.ret(stats=stats, **records(x, calls, "call_"))


def check_preferred_ends(W, R, eng):
    want, stats = PH.preferred_ends_ref(W.s, W.e, W.q, IV_START, IV_STOP, SIZE, 500, "split", 2, PH.flat_table(1))
    assert len(want) > 20 and PH.same_calls(_calls_of(R, PH.CALL_DTYPE), want)
    equal(R["stats"], stats, "stats")


IFS_THR = HH.flat_table(1, 64)


def run_ifs_hotspots(x):
    x.refill()
    windows, hotspots, stats = x.eng.ifs_hotspots("pt", IV_START, IV_STOP, SIZE, thresholds=IFS_THR)
    return x.ret(stats=stats, **records(x, windows, "call_"), **records(x, hotspots, "hot_"))


def check_ifs_hotspots(W, R, eng):
    windows, hotspots, stats = HH.ifs_hotspots_ref(W.s, W.e, W.q, IV_START, IV_STOP, SIZE, thresholds=IFS_THR)
    got_h = np.zeros(len(R["hot_run"]), HH.HOTSPOT_DTYPE)
    for f in HH.HOTSPOT_DTYPE.names:
        got_h[f] = R["hot_" + f]
    assert len(windows) > 50 and len(hotspots) > 1
    assert HH.same_records(_calls_of(R, HH.WINDOW_DTYPE), windows) and HH.same_records(got_h, hotspots)
    equal(R["stats"], stats, "stats")


IFS_GAP = 7  # windows of the output arrays between two intervals' that no interval owns


def run_ifs_track(x):
    """Windows that no interval owns: zeros in a host array (its stand-in is cleared and copied back whole), the caller's
    own bytes in a device array - checked here, then cleared so that the runs compare."""
    from finaletoolkit_amd.engine import Engine
    eng = x.eng
    count = Engine.ifs_window_ranges(IV_START, IV_STOP, SIZE, 20, 10)[1]
    offs = np.concatenate([[0], np.cumsum(count + IFS_GAP)])
    total = int(offs[-1]) - IFS_GAP
    n_out, i_out = x.out(total, np.int32), x.out(total, np.int64)
    x.refill()
    eng._check(eng.lib.ftk_ifs_track(eng.ctx, eng.contig_id("pt"), L.ptr(IV_START), L.ptr(IV_STOP), len(IV_START),
                                     L.ptr(np.ascontiguousarray(offs[:-1])), SIZE, 20, 10, 167, L.LEN_OPEN, L.LEN_OPEN, 30, n_out.p, i_out.p))
    got = x.ret(n=n_out, ifs=i_out)
    owned = np.zeros(total, bool)
    for o, c in zip(offs[:-1], count):
        owned[o:o + c] = True
    for k, v in got.items():
        gap = v[~owned].view(np.uint8)
        assert len(gap) and np.all(gap == (SENTINEL if x.device else 0)), (k, x.device)
        v[~owned] = 0
    return got


def check_ifs_track(W, R, eng):
    n, ifs, offs = HH.ifs_track_ref(W.s, W.e, W.q, IV_START, IV_STOP, SIZE)
    at = 0
    for i in range(len(IV_START)):
        c = int(offs[i + 1] - offs[i])
        equal(R["n"][at:at + c], n[offs[i]:offs[i + 1]], ("n", i))
        equal(R["ifs"][at:at + c], ifs[offs[i]:offs[i + 1]], ("ifs", i))
        at += c + IFS_GAP
    assert n.any()


def run_ifs_totals(x):
    x.refill()
    return x.ret(totals=np.array(x.eng.ifs_totals("pt", SIZE), np.int64))


def check_ifs_totals(W, R, eng):
    equal(R["totals"], np.array(HH.totals_ref(W.s, W.e, W.q, SIZE), np.int64), "totals")


# ------------------------------------------------------------------------------------------------------ end context
def _context_sets(eng):
    """(half_width, the class sets): one class, which a workgroup keeps in LDS, and the eight of EIGHT_CLASSES at a width
    at which it cannot."""
    for half in (128, 64, 32, 16, 7):
        if 1 <= eng.end_context_lds_classes(half) < 8:
            return half, (EC.ONE_CLASS, EC.EIGHT_CLASSES)
    raise AssertionError("no half-width keeps fewer than eight classes in LDS")


def run_end_context(x):
    eng, outs = x.eng, {}
    half, sets = _context_sets(eng)
    for edges in sets:
        n_classes = len(edges) - 1
        table, kept = x.out((n_classes, 2, 2 * half, 25), np.int64), x.out(n_classes, np.int64)
        edges32 = np.ascontiguousarray(edges, dtype=np.int32)
        x.refill()
        eng._check(eng.lib.ftk_end_context(eng.ctx, eng.contig_id("pt"), x.W.rid["2bit" if n_classes > 1 else "fa"], half, L.ptr(edges32),
                                           n_classes, 30, L.CONTEXT_ANCHOR["ends"], table.p, kept.p))
        outs[f"table{len(edges) - 1}"], outs[f"kept{len(edges) - 1}"] = table, kept
    return x.ret(**outs)


def check_end_context(W, R, eng):
    half, sets = _context_sets(eng)
    for edges in sets:
        table, kept = EC.restated_end_context(W.bases, W.s, W.e, W.q, half, edges, 30)
        equal(R[f"table{len(edges) - 1}"], table, ("table", len(edges) - 1))
        equal(R[f"kept{len(edges) - 1}"], kept, ("kept", len(edges) - 1))
        assert kept.sum() > 5_000


def run_ref_context(x):
    eng, outs = x.eng, {}
    for image in ("2bit", "fa"):
        outs[image] = x.out(25, np.int64)
        x.refill()
        eng._check(eng.lib.ftk_ref_context(eng.ctx, x.W.rid[image], 1, SIZE + 5, outs[image].p))
    return x.ret(**outs)


def check_ref_context(W, R, eng):
    want = EC.restated_ref_context(W.bases, 1, SIZE + 5)
    equal(R["2bit"], want, "2bit")
    equal(R["fa"], want, "fa")


# ------------------------------------------------------------------------------------------------------ export
def _mask(W):
    from finaletoolkit_amd.engine import RegionMask

    def pair(iv):  # (sorted and disjoint as they are)
        return np.array([a for a, _ in iv], np.int32), np.array([b for _, b in iv], np.int32)
    return RegionMask(pair(W.mask_wl), pair(W.mask_bl), "midpoint")


def _mask_keep(W):
    import test_frag_filter as F
    return W.memo("mask", lambda: F.restated_keep_sorted("midpoint", W.s, W.e, whitelist=W.mask_wl, blacklist=W.mask_bl))


def _text(b):
    return np.frombuffer(b, np.uint8)


def run_format_rows(x):
    x.refill()
    text, rows = x.eng.format_rows("pt", "chr5", 30)
    return x.ret(text=_text(text), rows=np.array([rows]))


def check_format_rows(W, R, eng):
    assert R["text"].tobytes() == W.text() and R["rows"][0] == int((W.q >= 30).sum())
    assert len(W.text()) > 4 * 0xFF00  # several BGZF members' worth


def run_mask_keep(x):
    x.refill()
    keep, kept = x.eng.mask_keep("pt", _mask(x.W))
    return x.ret(keep=keep, kept=np.array([kept]))


def check_mask_keep(W, R, eng):
    want = _mask_keep(W)
    assert 0.05 * W.n < want.sum() < 0.95 * W.n
    equal(R["keep"], want, "keep")
    assert R["kept"][0] == int(want.sum())


def run_format_rows_masked(x):
    x.refill()
    text, rows = x.eng.format_rows("pt", "chr5", 30, mask=_mask(x.W))
    return x.ret(text=_text(text), rows=np.array([rows]))


def check_format_rows_masked(W, R, eng):
    keep = (W.q >= 30) & _mask_keep(W)
    assert R["text"].tobytes() == host_rows("chr5", W.s[keep], W.e[keep], W.q[keep], W.st[keep]) and R["rows"][0] == int(keep.sum())


def run_bgzf_deflate(x):
    x.refill()
    image, offs = x.eng.bgzf_deflate(x.W.text())
    return x.ret(image=_text(image), offsets=offs)


def check_bgzf_deflate(W, R, eng):
    """The round trip through zlib gives the input back, member by member."""
    import zlib
    image, offs, text = R["image"].tobytes(), R["offsets"], W.text()
    assert len(offs) == -(-len(text) // 0xFF00) + 1 and offs[0] == 0 and offs[-1] + 28 == len(image)
    back = b"".join(zlib.decompress(image[a:b], 31) for a, b in zip(offs[:-1], offs[1:]))
    assert back == text and gzip.decompress(image) == text


def run_bgzf_inflate(x):
    eng, image, cap = x.eng, _text(x.W.bgzf()), len(x.W.text()) + 64
    out, n = np.full(cap, SENTINEL, np.uint8), C.c_int64()
    x.refill()
    eng._check(eng.lib.ftk_bgzf_inflate_device(eng.ctx, L.ptr(image), len(image), L.ptr(out), cap, C.byref(n)))
    return x.ret(text=out[:n.value], tail=out[n.value:])


def check_bgzf_inflate(W, R, eng):
    assert R["text"].tobytes() == W.text() == gzip.decompress(W.bgzf()) and np.all(R["tail"] == SENTINEL)


def _written(x, tag, mask):
    path = os.path.join(os.path.dirname(x.W.paths["fa"]), f"poison.{tag}.frag.gz")
    x.refill()
    res = x.eng.write_contig("pt", "chr5", path, 30, mask=mask, write_eof=True)
    with open(path, "rb") as fh:
        data = fh.read()
    rb, rs, re_ = res["runs"]
    return x.ret(file=_text(data), linear=res["linear"], run_bin=rb, run_beg=rs, run_end=re_,
                 counts=np.array([res["rows"], res["text_bytes"], res["first_off"], res["end_off"]]))


def run_frags_write(x):
    return _written(x, "plain", None)


def check_frags_write(W, R, eng):
    assert gzip.decompress(R["file"].tobytes()) == W.text() and R["counts"][0] == int((W.q >= 30).sum())
    assert R["counts"][3] + 28 == len(R["file"]) and len(R["linear"]) > 10 and len(R["run_bin"]) > 10


def run_frags_write_masked(x):
    return _written(x, "masked", _mask(x.W))


def check_frags_write_masked(W, R, eng):
    keep = (W.q >= 30) & _mask_keep(W)
    assert gzip.decompress(R["file"].tobytes()) == host_rows("chr5", W.s[keep], W.e[keep], W.q[keep], W.st[keep])
    assert R["counts"][0] == int(keep.sum())


# name: (run, check, takes device outputs).  One entry per entry point; "a+b": the calls of one entry share a test id.
CALLS = {
    "ftk_window_counts": (run_window_counts, check_window_counts, True),
    "ftk_delfi_counts": (run_delfi_counts, check_delfi_counts, True),
    "ftk_fraglen_hist": (run_fraglen_hist, check_fraglen_hist, True),
    "ftk_fraglen_stats": (run_fraglen_stats, check_fraglen_stats, True),
    "ftk_window_features": (run_window_features, check_window_features, True),
    "ftk_window_features_batch": (run_window_features_batch, check_window_features_batch, True),
    "ftk_window_features_wps": (run_window_features_wps, check_window_features_wps, True),
    "ftk_wps_window_features": (run_wps_window_features, check_wps_window_features, True),
    "ftk_frag_lengths": (run_frag_lengths, check_frag_lengths, False),
    "ftk_frag_select": (run_frag_select, check_frag_select, False),
    "ftk_wps": (run_wps, check_wps, True),
    "ftk_wps_intervals": (run_wps_intervals, check_wps_intervals, True),
    "ftk_wps_batch": (run_wps_batch, check_wps_batch, True),
    "ftk_cleavage": (run_cleavage, check_cleavage, True),
    "ftk_cleavage_intervals": (run_cleavage_intervals, check_cleavage_intervals, True),
    "ftk_wps_adjust": (run_wps_adjust, check_wps_adjust, True),
    "ftk_ref_gc_counts": (run_ref_gc_counts, check_ref_gc_counts, True),
    "ftk_motif_counts": (run_motif_counts, check_motif_counts, True),
    "ftk_depth": (run_depth, check_depth, True),
    "ftk_depth_runs": (run_depth_runs, check_depth_runs, False),
    "ftk_frag_gc": (run_frag_gc, check_frag_gc, True),
    "ftk_frag_gc_table": (run_frag_gc_table, check_frag_gc_table, True),
    "ftk_ref_gc_table": (run_ref_gc_table, check_ref_gc_table, True),
    "ftk_frags_set_gc_weights+ftk_frags_weights": (run_gc_weights, check_gc_weights, True),
    "ftk_weighted_window_sums": (run_weighted_window_sums, check_weighted_window_sums, True),
    "ftk_site_profile": (run_site_profile, check_site_profile, True),
    "ftk_site_vplot": (run_site_vplot, check_site_vplot, True),
    "ftk_site_ends": (run_site_ends, check_site_ends, True),
    "ftk_track_spectrum": (run_track_spectrum, check_track_spectrum, True),
    "ftk_wps_spectrum": (run_wps_spectrum, check_wps_spectrum, True),
    "ftk_track_peaks": (run_track_peaks, check_track_peaks, True),
    "ftk_wps_peaks": (run_wps_peaks, check_wps_peaks, False),
    "ftk_preferred_ends": (run_preferred_ends, check_preferred_ends, False),
    "ftk_ifs_hotspots": (run_ifs_hotspots, check_ifs_hotspots, False),
    "ftk_ifs_track": (run_ifs_track, check_ifs_track, True),
    "ftk_ifs_totals": (run_ifs_totals, check_ifs_totals, False),
    "ftk_end_context": (run_end_context, check_end_context, True),
    "ftk_ref_context": (run_ref_context, check_ref_context, True),
    "ftk_frags_format_rows": (run_format_rows, check_format_rows, False),
    "ftk_frags_mask_keep": (run_mask_keep, check_mask_keep, False),
    "ftk_frags_format_rows_masked": (run_format_rows_masked, check_format_rows_masked, False),
    "ftk_bgzf_deflate_device": (run_bgzf_deflate, check_bgzf_deflate, False),
    "ftk_bgzf_inflate_device": (run_bgzf_inflate, check_bgzf_inflate, False),
    "ftk_frags_write": (run_frags_write, check_frags_write, False),
    "ftk_frags_write_masked": (run_frags_write_masked, check_frags_write_masked, False),
}
# the window features and the batch / merged calls once more in a process with FTK_FEAT_BLOCK=1
CHILD_CALLS = ("ftk_window_features", "ftk_window_features_batch", "ftk_window_features_wps", "ftk_wps_window_features")


def main(tmp, path):
    W = World(tmp)
    eng = open_engine(W)
    out = {}
    try:
        for name in CHILD_CALLS:
            R, S, runs, sizes = procedure(eng, W, name)
            out[f"{name}/S"] = np.array([S] + [sizes[tag] for tag in runs], np.int64)
            for tag, got in [("R", R)] + list(runs.items()):
                for k, v in got.items():
                    out[f"{name}/{tag}/{k}"] = v
    finally:
        eng.close()
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
