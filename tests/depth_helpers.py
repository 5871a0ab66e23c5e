"""Shared pieces of the depth tests (``tests/test_gpu_frag_depth.py``, ``tests/test_gpu_top_coordinates.py``): the numpy
restatement of ``ftk_depth`` and ``ftk_depth_runs`` - ``np.add.at`` of +1 / -1 at the clipped fragment bounds, ``cumsum``,
runs from ``np.flatnonzero(np.diff(depth))`` - and the invariants of every run table."""
import numpy as np


def kept(s, e, q, mapq_min=0, min_len=None, max_len=None):
    ln = e.astype(np.int64) - s
    keep = q >= mapq_min
    if min_len is not None:
        keep &= ln >= min_len
    if max_len is not None:
        keep &= ln <= max_len
    return keep


def restated_depth(s, e, keep, start, stop):
    s = s.astype(np.int64)
    e = e.astype(np.int64)
    m = keep & (e > start) & (s < stop)  # the kept fragments that overlap the region
    d = np.zeros(stop - start + 1, np.int64)
    np.add.at(d, np.maximum(s[m], start) - start, 1)
    np.add.at(d, np.minimum(e[m], stop) - start, -1)
    return np.cumsum(d[:-1]).astype(np.int32)


def restated_runs(depth, start, include_zero):
    n = len(depth)
    if n == 0:
        return (np.zeros(0, np.int32),) * 3
    cut = np.flatnonzero(np.diff(depth)) + 1
    rs = np.concatenate(([0], cut))
    re_ = np.concatenate((cut, [n]))
    rd = depth[rs]
    if not include_zero:
        rs, re_, rd = rs[rd != 0], re_[rd != 0], rd[rd != 0]
    return (rs + start).astype(np.int32), (re_ + start).astype(np.int32), rd.astype(np.int32)


def check_invariants(runs, start, stop, include_zero, s, e, keep):
    rs, re_, rd = (a.astype(np.int64) for a in runs)
    assert np.all(rs < re_) and np.all(re_[:-1] <= rs[1:])
    touch = re_[:-1] == rs[1:]
    assert np.all(rd[:-1][touch] != rd[1:][touch])
    clipped = np.clip(np.minimum(e.astype(np.int64), stop) - np.maximum(s.astype(np.int64), start), 0, None)
    assert int(((re_ - rs) * rd).sum()) == int(clipped[keep].sum())
    if include_zero:
        assert (len(rs) == 0) == (stop == start)
        if len(rs):
            assert rs[0] == start and re_[-1] == stop and np.all(touch)
    else:
        assert np.all(rd != 0)
        assert len(rs) == 0 or (rs[0] >= start and re_[-1] <= stop)
