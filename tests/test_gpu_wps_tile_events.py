"""
GPU: a fragment's events in a WPS tile's difference array (csrc/ftk_wps_events.h: 32-bit tile-relative cells, one OR-ed
sign test, the fetch-window tests only in edge tiles, read1 compiled out of the packed tile) give the oracle's scores.

Every call of tests/wps_tile_events_child.py runs twice, each time in a fresh process: with the packed columns (the
default) and with FTK_PACKED=0 (the wide columns); FTK_FEAT_BLOCK=1 puts the windows of ftk_window_features_wps on the
block path, i.e. on feat_then_wps_kernel.  The two runs and the oracle must agree in every integer, through
ftk_window_features_wps, ftk_wps and ftk_wps_intervals (partial first and last tiles, intervals that begin anywhere).
The oracle is asked for each interval whole: its fetch window is part of what is checked.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import wps_tile_events_child as K
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu


def _child(tmp, tag, **env):
    path = os.path.join(tmp, tag + ".npz")
    e = {k: v for k, v in os.environ.items() if k not in ("FTK_PACKED", "FTK_FEAT_FAST", "FTK_WPS_TPB")}
    e.update(FTK_FEAT_BLOCK="1", **env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wps_tile_events_child.py"), path], env=e,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("wps_events"))
    return _child(tmp, "packed"), _child(tmp, "wide", FTK_PACKED="0")


@pytest.fixture(scope="module")
def frags():
    out = {}
    for name in K.CONTIGS:
        c = K.make_contig(name)
        out[name] = c, O.Frags(c["start"], c["end"], c["mapq"], None, c["r1_start"], c["r1_end"])
    return out


def _events(c, W, t0):
    """tile-relative cells a, b, c, e of every fragment"""
    hl, hr = K._halves(W)
    s, e = c["start"].astype(np.int64), c["end"].astype(np.int64)
    return s - hr - t0, s + hl + 1 - t0, e - hr - t0, e + hl + 1 - t0


def test_the_contigs_hold_what_the_cases_need():
    c = K.make_contig("tiles")
    s, e, q = c["start"].astype(np.int64), c["end"].astype(np.int64), c["mapq"]
    length = e - s
    assert (np.diff(s) >= 0).all() and len(s) <= 6000 and length.max() == 2046  # the packed column stays
    a0, b0 = c["wps"]
    assert a0 > 0 and b0 < c["size"] and (b0 - a0) % K.T and (b0 - a0) // K.T == 4
    for W, mn, mx, mq in K.CALLS[:2]:
        ok = (length >= mn) & (length <= mx)
        len_4 = b0 - a0 - 4 * K.T  # the partial last tile
        for t0, cells in ((a0, {-1, 0, K.T - 1, K.T}), (a0 + K.T, {-1, 0, K.T - 1, K.T}), (a0 + 4 * K.T, {len_4 - 1, len_4})):
            ev = _events(c, W, t0)
            for v in ev:  # every event on -1, 0 and on the tile's last cell and the one behind it
                assert cells <= set(v[ok].tolist()), (W, t0)
            assert ((ev[2] == ev[1]) & ok).any() and ((ev[2] == ev[1] - 1) & ok).any() and ((ev[2] == ev[1] + 1) & ok).any()
        assert set(K.LENS) <= set(length.tolist()) and {mn - 1, mn, mn + 1, mx - 1, mx, mx + 1} <= set(length.tolist())
        assert {mq - 1, mq, mq + 1} <= set(q.tolist())
    # fragments across one tile boundary; a tile with more than 1 024 candidates; one with none in the bounded calls
    t1, t3, t4 = a0 + K.T, a0 + 3 * K.T, a0 + 4 * K.T
    assert ((s < t1) & (e > t1)).any()
    assert ((s >= t1) & (s < t1 + K.T)).sum() > 1024 + 256
    assert not ((s >= t3 - 1 - 500 - 180 - 512) & (s < t4 + 500 + 512)).any()
    # the fetch window [a0 - 180, b0 + 180): midpoints, starts and ends on both sides of each bound
    mid = (s + e) >> 1
    for x in (a0 - 180, b0 + 180):
        for v in (mid, s, e):
            assert {x - 1, x, x + 1} <= set(v.tolist())
    assert not a0 % K.T == 0 and all(iv[0] % K.T for iv in c["intervals"])
    # with W = 1000 the first tile of the unit is an edge tile and the second an interior one (ftk_wps_events.h)
    hl = 500
    assert not a0 - hl - 1 - 180 > a0 - 180 and a0 + K.T - hl - 1 - 180 > a0 - 180
    b = K.make_contig("bam")
    assert np.array_equal(b["start"], c["start"]) and (b["r1_start"] >= b["start"]).all() and (b["r1_end"] <= b["end"]).all()
    lg = K.make_contig("long")
    ls, le = lg["start"].astype(np.int64), lg["end"].astype(np.int64)
    assert ((ls < lg["wps"][0] + K.T) & (le > lg["wps"][0] + 2 * K.T)).any() and (le - ls).max() > 2046
    tp = K.make_contig("top")
    assert tp["end"].max() == K.TOP - 1 == tp["size"] == tp["wps"][1] and (tp["end"] == K.TOP - 1).sum() >= len(K.LENS)


@pytest.mark.parametrize("call", range(len(K.CALLS)))
@pytest.mark.parametrize("name", K.CONTIGS)
def test_packed_equals_wide_equals_oracle(runs, frags, name, call):
    packed, wide = runs
    c, fr = frags[name]
    W, mn, mx, q = K.CALLS[call]
    key = f"{name}/{call}/"
    a, b = c["wps"]
    want = O.c_wps(fr, a, b, c["size"], W, mn, mx, q)
    want_iv = np.concatenate([O.c_wps(fr, x, y, c["size"], W, mn, mx, q) for x, y in c["intervals"]])
    assert want.any() and want_iv.any()
    for got in (wide, packed):
        assert np.array_equal(got[key + "merged"], want), (key, "merged")
        assert np.array_equal(got[key + "wps"], want), (key, "wps")
        assert np.array_equal(got[key + "intervals"], want_iv), (key, "intervals")


def test_read1_decides_on_the_bam_contig(runs):
    """The BAM contig holds the fragments of `tiles`; where the window is far wider than max_len its scores differ: read1
    decided for fragments that cross the fetch window's bounds."""
    packed, _ = runs
    k = [c[0] for c in K.CALLS].index(1000)
    assert not np.array_equal(packed[f"bam/{k}/wps"], packed[f"tiles/{k}/wps"])


def test_the_packed_path_ran(runs):
    """`tiles` and `top` hold the packed columns and every bounded call made packed launches; none under FTK_PACKED=0."""
    packed, wide = runs
    assert packed["tiles/present"].tolist() == [1] and packed["top/present"].tolist() == [1]
    assert packed["long/present"].tolist() == [0]  # a fragment longer than 2 046
    n_bounded = sum(1 for c in K.CALLS if c[2] < 2047)
    assert packed["tiles/launches"][0] >= 3 * n_bounded
    assert all(wide[f"{n}/launches"][0] == 0 for n in K.CONTIGS)
