"""
GPU: the packed (length, mapq) column (ContigView::lq, csrc/ftk_packed.h) changes no result.

Every call of tests/packed_columns_child.py runs twice, each time in a fresh process: once with the packed path on (the
default) and once with FTK_PACKED=0; FTK_FEAT_BLOCK=1 puts the three windows on the block path, i.e. on the kernels that
have a packed form (feat_then_wps_kernel, feat_fast_kernel, wps_stream_kernel).  The two runs and the oracle must agree in
every integer, and the packed-launch counter must show that each call took the path the rule gives it.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import packed_columns_child as K
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu


def _child(tmp, tag, **env):
    path = os.path.join(tmp, tag + ".npz")
    e = {k: v for k, v in os.environ.items() if k not in ("FTK_PACKED", "FTK_FEAT_FAST", "FTK_WPS_TPB")}
    e.update(FTK_FEAT_BLOCK="1", **env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "packed_columns_child.py"), path], env=e,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("packed"))
    return _child(tmp, "packed"), _child(tmp, "wide", FTK_PACKED="0")


def _oracle_wps(fr, c, step=4000):
    """The oracle's scores of [a, b), asked for in pieces: its cost grows with the square of the interval.  A piece's
    narrower fetch window [a' - max_len, b' + max_len) drops no fragment that reaches the piece: one whose midpoint lies
    outside ends at least max_len / 2 away, and every case has max_len / 2 > W / 2."""
    assert c["wmax"] > c["W"]
    return np.concatenate([O.c_wps(fr, a, min(a + step, c["b"]), K.SIZE, c["W"], c["wmin"], c["wmax"], c["wq"])
                           for a in range(c["a"], c["b"], step)])


@pytest.fixture(scope="module")
def want():
    """The oracle's results per (contig, case), computed once."""
    ws, we = K.windows()
    out = {}
    for name in K.CONTIGS:
        s, e, q = K.make_contig(name)
        fr = O.Frags(s, e, q, np.zeros(len(s), np.uint8))
        for i, c in enumerate(K.CASES):
            hist, over = O.c_fraglen_hist(fr, ws, we, c["hist"][0], c["hist"][1], mapq_min=c["q"])
            d = O.c_delfi_counts(fr, ws, we, c["q"], K.BL_START, K.BL_END, K.GAPS)
            out[name, i] = dict(coverage=O.c_window_counts(fr, ws, we, mapq_min=c["q"]), hist=hist, overflow=over,
                                short=d[0], long=d[1],
                                wps=_oracle_wps(fr, c))
    return out


def _check_case(got, key, w):
    for k in ("coverage", "hist", "overflow", "short", "long"):
        assert np.array_equal(got[f"{key}merged_{k}"].astype(np.int64), w[k].astype(np.int64)), (key, "merged", k)
        assert np.array_equal(got[f"{key}feat_{k}"].astype(np.int64), w[k].astype(np.int64)), (key, "features", k)
    assert np.array_equal(got[f"{key}merged_wps"], w["wps"]), (key, "merged wps")
    assert np.array_equal(got[f"{key}wps"], w["wps"]), (key, "wps")


def test_the_contigs_hold_what_the_cases_need():
    s, e, q = K.make_contig("main")
    assert 2_000 <= len(s) <= 20_000 and int((e - s).max()) == K.LEN_MAX
    assert set(K.SPECIAL_LENS) <= set((e - s).tolist()) and set(K.SPECIAL_Q) <= set(q.tolist())
    s2, e2, _ = K.make_contig("long")
    assert len(s2) == len(s) + 1 and int((e2 - s2).max()) == K.LEN_MAX + 1
    assert not ((s >= K.EMPTY[0]) & (s < K.EMPTY[1])).any()
    # both block sizes of the stand-alone feature kernel: 'main' stays below the 4096 expected candidates per window at
    # which the library switches to 512-thread blocks, 'other' lies above it (the merged launch always runs 256)
    s3, e3, _ = K.make_contig("other")
    assert len(s3) <= 20_000
    assert K.expected_candidates(s, e, int((e - s).max())) < 4096 <= K.expected_candidates(s3, e3, int((e3 - s3).max()))
    n_tiles = -(-(K.B0 - K.A0) // 4096)
    assert n_tiles == 70 and (K.B0 - K.A0) % 4096 == 1234 and K.A0 > 0
    assert {c["W"] & 1 for c in K.CASES} == {0, 1}


def test_column_presence(runs):
    """'main' and 'other' hold the column (whatever FTK_PACKED says: it is a property of the resident contig); 'long',
    with ONE fragment of 2047, does not."""
    for got in runs:
        assert got["main/present"].tolist() == [1, K.LEN_MAX]
        assert got["other/present"].tolist() == [1, K.LEN_MAX]
        assert got["long/present"].tolist() == [0, K.LEN_MAX]


@pytest.mark.parametrize("case", range(len(K.CASES)))
@pytest.mark.parametrize("name", K.CONTIGS)
def test_packed_equals_wide_equals_oracle(runs, want, name, case):
    packed, wide = runs
    key = f"{name}/{case}/"
    for k in packed:
        if k.startswith(key) and not k.endswith("steps"):
            assert packed[k].dtype == wide[k].dtype and np.array_equal(packed[k], wide[k]), k
    _check_case(packed, key, want[name, case])
    _check_case(wide, key, want[name, case])


@pytest.mark.parametrize("case", range(len(K.CASES)))
def test_each_call_takes_the_path_the_rule_gives_it(runs, case):
    """Steps of the packed-launch counter over (merged, features, wps): a threshold of 2^B or more, a histogram edge or a
    length bound beyond the packable range, and a contig without the column keep the wide kernels."""
    packed, wide = runs
    c = K.CASES[case]
    expect = [int(c["feat"] and c["wps"]), int(c["feat"]), int(c["wps"])]
    assert packed[f"main/{case}/steps"].tolist() == expect
    assert packed[f"other/{case}/steps"].tolist() == expect
    assert packed[f"long/{case}/steps"].tolist() == [0, 0, 0]
    for name in K.CONTIGS:
        assert wide[f"{name}/{case}/steps"].tolist() == [0, 0, 0]


def test_reload_under_one_id_never_reads_a_stale_column(runs, want):
    """load / release / load of other contigs under the same id, with and without the column: every result is the
    loaded contig's."""
    packed, wide = runs
    for k, (kind, _) in enumerate(K.RELOADS):
        for got in runs:
            _check_case(got, f"re/{k}/", want[kind, 0])
        assert packed[f"re/{k}/steps"].tolist() == ([0, 0, 0] if kind == "long" else [1, 1, 1])
        assert wide[f"re/{k}/steps"].tolist() == [0, 0, 0]
