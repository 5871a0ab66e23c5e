"""
GPU: counts taken from the length histogram, and a window's interior read from the packed words alone
(csrc/ftk_feat_interior.h), change no result.

Every case of tests/feat_interior_child.py runs three times, each time in a fresh process: with the default path, with
FTK_FEAT_INTERIOR=0 (the per-fragment counters in every window) and with FTK_PACKED=0 (the wide columns);
FTK_FEAT_BLOCK=1 puts the windows on the block path, i.e. on feat_then_wps_kernel (ftk_window_features_wps) and
feat_fast_kernel (ftk_window_features).  The three runs and the oracle must agree in every integer; the reference of
every expectation is the oracle, never the new path.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import feat_interior_child as K
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu


def _child(tmp, tag, **env):
    path = os.path.join(tmp, tag + ".npz")
    e = {k: v for k, v in os.environ.items() if k not in ("FTK_PACKED", "FTK_FEAT_FAST", "FTK_FEAT_INTERIOR", "FTK_WPS_TPB")}
    e.update(FTK_FEAT_BLOCK="1", **env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "feat_interior_child.py"), path], env=e,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("interior"))
    return dict(interior=_child(tmp, "interior"), counters=_child(tmp, "counters", FTK_FEAT_INTERIOR="0"),
                wide=_child(tmp, "wide", FTK_PACKED="0"))


@pytest.fixture(scope="module")
def want():
    """The oracle's results per case, computed once."""
    out = {}
    for name in K.CASES:
        c = K.make_case(name)
        fr = O.Frags(c["start"], c["end"], c["mapq"], np.zeros(len(c["start"]), np.uint8))
        bl = c["bl"] or (None, None)
        d = O.c_delfi_counts(fr, c["ws"], c["we"], K.Q, bl[0], bl[1], c["gaps"])
        w = dict(coverage=O.c_window_counts(fr, c["ws"], c["we"], mapq_min=K.Q), short=d[0], long=d[1])
        if c["hist"]:
            w["hist"], w["overflow"] = O.c_fraglen_hist(fr, c["ws"], c["we"], c["hist"][0], c["hist"][1], mapq_min=K.Q)
        out[name] = w
    return out


def test_the_cases_hold_what_they_are_for():
    lmax = max(K.LENS)
    for name in K.CASES:
        c = K.make_case(name)
        s = c["start"].astype(np.int64)
        assert (np.diff(s) >= 0).all() and s.min() >= 0 and len(c["ws"]) >= 2
    c = K.make_case("off")
    s, ln = c["start"].astype(np.int64), (c["end"] - c["start"]).astype(np.int64)
    for ws, we in zip(c["ws"].tolist(), c["we"].tolist()):
        for d in (-1, 0, 1):  # fragments on both sides of the interior's upper bound
            assert (s == we - lmax + d).any() or we - lmax + d >= len(s)
    assert any(((s == ws) & (ln == 0)).any() for ws in c["ws"].tolist())  # zero-length fragments at ws
    assert {int(w) % 512 == 0 for w in c["ws"]} == {True, False} and 0 in c["ws"].tolist()
    assert any(we - ws < lmax + 512 for ws, we in zip(c["ws"].tolist(), c["we"].tolist()))
    assert c["we"][-1] == c["size"] > c["end"].max()  # the last, partial window
    z = K.make_case("zero")
    assert (z["end"] == z["start"]).all()
    wd = K.make_case("wide")
    d = np.diff(wd["start"].astype(np.int64))
    at = np.flatnonzero(d > 255) + 1
    assert at.tolist() == [1500] and 1500 % 64 and 512 < wd["start"][1500 - 64] and wd["start"][1500 + 64] < 4096 - lmax - 512
    m = K.make_case("mixed")
    assert m["bl"][0][0] > m["ws"][1] and m["bl"][1][0] < m["we"][1] and m["ws"][3] < m["gaps"][0] < m["we"][3]
    assert K.make_case("len_lo")["hist"][0] == 101 and K.make_case("n_bins")["hist"] == (0, 120) and K.make_case("no_hist")["hist"] is None
    dp = K.make_case("deep")
    inside = (dp["start"] >= 512) & (dp["start"] < 4096)
    assert inside.sum() > 24_576 and len(dp["start"]) < 50_000
    e = K.make_case("empty")
    counts = [int(((e["start"] >= a) & (e["start"] < b)).sum()) for a, b in zip(e["ws"].tolist(), e["we"].tolist())]
    assert counts[1] == 0 and counts[2] == 0 and counts[4] == 0 and counts[0] > 0 and counts[3] > 0


@pytest.mark.parametrize("name", K.CASES)
def test_every_path_equals_the_oracle(runs, want, name):
    w = want[name]
    keys = [k for k in runs["wide"] if k.startswith(name + "/")]
    assert len(keys) >= 6
    for mode, got in runs.items():
        assert sorted(k for k in got if k.startswith(name + "/")) == sorted(keys)
        for k in keys:
            call, what = k.split("/")[1].split("_", 1)
            if what == "wps":
                assert np.array_equal(got[k], runs["wide"][k]), (mode, k)
            else:
                assert np.array_equal(got[k].astype(np.int64), np.asarray(w[what]).astype(np.int64)), (mode, k)
