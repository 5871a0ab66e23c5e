"""
GPU: the start column as 1-byte deltas (ContigView::ds / gbase, csrc/ftk_packed.h) changes no result.

Every call of tests/delta_column_child.py runs twice, each time in a fresh process: once with the packed path on (the
default: start deltas + packed (length, mapq) words) and once with FTK_PACKED=0 (the wide columns); FTK_FEAT_BLOCK=1 puts
the windows on the block path, i.e. on the kernels that have a packed form (feat_then_wps_kernel, feat_fast_kernel,
wps_stream_kernel).  The two runs and the oracle must agree in every integer - the reference of every expectation is the
wide path and the oracle, never the packed path - and the packed-launch counter must show that the packed path ran.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import delta_column_child as K
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu


def _child(tmp, tag, **env):
    path = os.path.join(tmp, tag + ".npz")
    e = {k: v for k, v in os.environ.items() if k not in ("FTK_PACKED", "FTK_FEAT_FAST", "FTK_WPS_TPB")}
    e.update(FTK_FEAT_BLOCK="1", **env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "delta_column_child.py"), path], env=e,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("delta"))
    return _child(tmp, "packed"), _child(tmp, "wide", FTK_PACKED="0")


def _oracle_wps(fr, a, b, size, W, step=4000):
    """The oracle's scores of [a, b), asked for in pieces: its cost grows with the square of the interval.  A piece's
    narrower fetch window [a' - max_len, b' + max_len) drops no fragment that reaches the piece: one whose midpoint lies
    outside ends at least max_len / 2 away, and max_len / 2 > W / 2."""
    assert K.WMAX > W
    return np.concatenate([O.c_wps(fr, x, min(x + step, b), size, W, K.WMIN, K.WMAX, K.Q) for x in range(a, b, step)])


@pytest.fixture(scope="module")
def want():
    """The oracle's results per (contig, W), computed once."""
    out = {}
    for name in K.CONTIGS:
        c = K.make_contig(name)
        fr = O.Frags(c["start"], c["end"], c["mapq"], np.zeros(len(c["start"]), np.uint8))
        hist, over = O.c_fraglen_hist(fr, c["ws"], c["we"], K.HIST[0], K.HIST[1], mapq_min=K.Q)
        d = O.c_delfi_counts(fr, c["ws"], c["we"], K.Q, K.BL[0], K.BL[1], K.GAPS)
        feat = dict(coverage=O.c_window_counts(fr, c["ws"], c["we"], mapq_min=K.Q), hist=hist, overflow=over, short=d[0],
                    long=d[1])
        for W in K.WS:
            w = dict(feat, wps=_oracle_wps(fr, c["wps"][0], c["wps"][1], c["size"], W))
            if c["intervals"]:
                w["intervals"] = np.concatenate([_oracle_wps(fr, a, b, c["size"], W) for a, b in c["intervals"]])
            out[name, W] = w
    return out


def _check(got, key, w):
    for k in ("coverage", "hist", "overflow", "short", "long"):
        assert np.array_equal(got[f"{key}merged_{k}"].astype(np.int64), w[k].astype(np.int64)), (key, "merged", k)
        assert np.array_equal(got[f"{key}feat_{k}"].astype(np.int64), w[k].astype(np.int64)), (key, "features", k)
    assert np.array_equal(got[f"{key}merged_wps"], w["wps"]), (key, "merged wps")
    assert np.array_equal(got[f"{key}wps"], w["wps"]), (key, "wps")
    if "intervals" in w:
        assert np.array_equal(got[f"{key}intervals"], w["intervals"]), (key, "intervals")


def test_the_contigs_hold_what_the_cases_need():
    for name, n in (("n1", 1), ("n63", 63), ("n64", 64), ("n65", 65), ("n200", 200)):
        c = K.make_contig(name)
        assert len(c["start"]) == n and c["we"][-1] == c["size"] == c["wps"][1] > c["end"].max()
    for name in K.CONTIGS:
        c = K.make_contig(name)
        s = c["start"].astype(np.int64)
        assert (np.diff(s) >= 0).all() and s.min() >= 0 and c["end"].max() < K.TOP and len(s) <= 5000
    d = np.diff(K.make_contig("same")["start"].astype(np.int64))
    run = np.flatnonzero(d == 0)
    assert len(run) >= 69 and run.min() < 63 < run.max()  # 70 or more equal starts across the boundary 63 | 64
    g = K.make_contig("gaps")
    d = np.diff(g["start"].astype(np.int64), prepend=g["start"][0])
    big = {int(i): int(d[i]) for i in np.flatnonzero(d > 200)}
    assert big == {10: 255, 84: 256, 128: 100_000, 200: 300}
    assert g["wps"][0] < g["start"][0] and g["start"][127] < g["wps"][1] and g["wps"][0] % 4096  # groups 0 and 1, one tile
    t = K.make_contig("top")
    d = np.diff(t["start"].astype(np.int64))
    assert sorted(d[d > 200].tolist()) == [255, 256, 4000] and d[639] == 4000 and t["start"].min() > K.TOP - 60_000
    for off in (0, 1, 32):  # first fragment of position-index bin k
        s = K.make_contig(f"b{off}")["start"]
        assert [int(np.searchsorted(s, 512 * k)) % 64 for k in (1, 5, 17)] == [(-off) % 64] * 3
    dn = K.make_contig("dense")
    assert len(dn["start"]) > 4096 + 256 and dn["end"].max() < 8192  # one tile: five chunks of 1 024; two feature passes
    assert {W & 1 for W in K.WS} == {0, 1}
    assert all(a % 4096 for name in ("gaps", "top", "b1", "dense") for a, _ in K.make_contig(name)["intervals"])


@pytest.mark.parametrize("W", K.WS)
@pytest.mark.parametrize("name", K.CONTIGS)
def test_packed_equals_wide_equals_oracle(runs, want, name, W):
    packed, wide = runs
    key = f"{name}/{W}/"
    n = 0
    for k in packed:
        if k.startswith(key) and not k.endswith("steps"):
            assert packed[k].dtype == wide[k].dtype and np.array_equal(packed[k], wide[k]), k
            n += 1
    assert n >= 12
    _check(wide, key, want[name, W])
    _check(packed, key, want[name, W])


@pytest.mark.parametrize("name", K.CONTIGS)
def test_the_packed_path_ran(runs, name):
    """Every contig holds the columns; each call - merged, features, WPS, intervals - made one packed launch, and none
    under FTK_PACKED=0."""
    packed, wide = runs
    assert packed[f"{name}/present"].tolist() == [1] and wide[f"{name}/present"].tolist() == [1]
    for W in K.WS:
        steps = packed[f"{name}/{W}/steps"].tolist()
        assert steps == [1] * len(steps) and len(steps) == (4 if K.make_contig(name)["intervals"] else 3)
        assert not wide[f"{name}/{W}/steps"].any()
