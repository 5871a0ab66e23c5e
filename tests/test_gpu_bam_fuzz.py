"""GPU: every BAM decode route over the seeded adversarial corpus of tests/test_bam_fuzz.py, held to oracle.bam_rows
(never to the library's own host decoder): device inflate + device records at stretches of 64 B to 16 KB and pieces of
64 KB to the default, host records on device inflate, everything on the host, one contig through the BAI, regions,
the host decoder taking over from the device parser and the device path starting over - every table exact, read1
columns and file order included, and the count of dropped records exact.  Each stream runs in a child process (the
harnesses of tests/test_gpu_inflate.py) under a time limit."""
import os
import pickle
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests.test_bam_fuzz import assert_table, build_corpus
from tests.test_gpu_inflate import _BAM_MULTI_CHILD, _BAM_REGION_CHILD

pytestmark = pytest.mark.gpu

# _BAM_MULTI_CHILD's stream(), then: the whole file ("*") and the contigs named, pickled
_ROUTES_CHILD = _BAM_MULTI_CHILD[:_BAM_MULTI_CHILD.index("\nwant = _decode")] + r"""
import pickle
res = {{}}
for spec in sys.argv[3:]:
    got, order = stream(None if spec == "*" else spec)
    res[spec] = (order, skipped[-1], {{c: (v[0], v[1], ranks[c]) for c, v in got.items()}})
pickle.dump(res, open(sys.argv[2], "wb"))
print("ok device_tables", n_device[0])
"""

# _BAM_REGION_CHILD's stream(path, contig, a, b), then: the regions "contig:a:b", pickled
_REGION_CHILD = _BAM_REGION_CHILD[:_BAM_REGION_CHILD.index("\npath = sys.argv[1]")] + r"""
import pickle
res = {{}}
for spec in sys.argv[3:]:
    c, a, b = spec.split(":")
    res[spec] = stream(sys.argv[1], c, int(a), int(b))
pickle.dump(res, open(sys.argv[2], "wb"))
print("ok")
"""

TAKEOVER = "the host decoder takes over"


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return build_corpus(tmp_path_factory.mktemp("fuzzbam_gpu"))


def _run(tmp_path, child, path, specs, env, timeout=300):
    out = str(tmp_path / "out.pkl")
    r = subprocess.run([sys.executable, "-c", child.format(root=H.ROOT), path, out, *specs], capture_output=True, text=True,
                       timeout=timeout, env=dict(os.environ, FTK_DECODE_TIMING="1", **env))
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-1500:] + r.stderr[-2500:]
    with open(out, "rb") as fh:
        return pickle.load(fh), r


def _check(what, res, exp, spec):
    """The stream ``spec`` ("*" or a contig) of a routes child equal to the reference: order, tables, dropped counts."""
    want, skipped, _, per = exp
    order, sk, got = res[spec]
    names = [c for c in want if len(want[c][0])] if spec == "*" else [c for c in [spec] if len(want[c][0])]
    assert order == names, (what, spec, order)
    for c in names:
        assert_table((what, spec, c), *got[c], want[c])
    assert sk == (skipped if spec == "*" else per[spec]), (what, spec, sk)


def _report(what, r):
    # (the issue this corpus was built for asks whether adversarial aux content ever sends a piece to the host decoder)
    print(f"[bam fuzz] {what}: host decoder took over: {'yes' if TAKEOVER in r.stderr else 'no'}")


@pytest.mark.parametrize("piece,stretch", [(1 << 16, "64"), (1 << 16, "700"), (1 << 20, "16384"), (1 << 20, "700"),
                                           (None, "16384"), (None, "64")])
def test_device_records_equal_the_reference(corpus, tmp_path, piece, stretch):
    """The default route (ftk_fragstream_open_device: device inflate, bam_setup/walk/scan/emit_kernel, device sort) on
    the mixed file (whole, and chr2 through the BAI) and the 2^30 file (whole, and its big contig)."""
    env = dict(FTK_BAM_DEV_STRETCH=stretch)
    if piece:
        env["FTK_STREAM_PIECE"] = str(piece)
    for name, one in (("mixed", "chr2"), ("top", "chrBig")):
        res, r = _run(tmp_path, _ROUTES_CHILD, corpus[name][0], ["*", one], env)
        for spec in ("*", one):
            _check((name, piece, stretch), res, corpus[name][1], spec)
        assert "parsed on the device" in r.stderr, r.stderr[-1500:]
        _report(f"{name} piece {piece} stretch {stretch}", r)


@pytest.mark.parametrize("env", [dict(FTK_DEVICE_BAM_PARSE="0"), dict(FTK_DEVICE_INFLATE="0"),
                                 dict(FTK_DEVICE_BAM_PARSE="0", FTK_STREAM_PIECE=str(1 << 16))])
def test_host_record_routes_equal_the_reference(corpus, tmp_path, env):
    """Records parsed by the host threads on device-inflated pieces, and everything on the host - the fuzzed files,
    the CIGAR-less one included (its records are counted, not turned into rows)."""
    for name, one in (("mixed", "chr3"), ("top", "chrBig"), ("nocigar", "chrA")):
        res, _ = _run(tmp_path, _ROUTES_CHILD, corpus[name][0], ["*", one], env)
        for spec in ("*", one):
            _check((name, env), res, corpus[name][1], spec)


def test_nocigar_file_on_the_device(corpus, tmp_path):
    """The CIGAR-less file through the device parser: its rows, and the three records counted."""
    res, r = _run(tmp_path, _ROUTES_CHILD, corpus["nocigar"][0], ["*", "chrA"], dict(FTK_STREAM_PIECE=str(1 << 16)))
    for spec in ("*", "chrA"):
        _check("nocigar", res, corpus["nocigar"][1], spec)
    assert res["*"][1][1] == 3
    _report("nocigar", r)


def test_host_takeover_counts_every_record_once(corpus, tmp_path):
    """More contig runs in one 64 KB piece than the device summary lists: the stream starts over on the host decoder
    after big0 was handed out and mid0's first pieces were parsed, both with negative starts.  Every contig once,
    exact, and the dropped count exact: neither the contig handed out nor the one in progress is counted twice."""
    path, exp = corpus["alts"]
    res, r = _run(tmp_path, _ROUTES_CHILD, path, ["*", "big1"], dict(FTK_STREAM_PIECE=str(1 << 16)))
    assert TAKEOVER in r.stderr, r.stderr[-1500:]
    print("[bam fuzz] alts:", [ln for ln in r.stderr.splitlines() if TAKEOVER in ln][:1])
    for spec in ("*", "big1"):
        _check("alts", res, exp, spec)
    assert res["*"][1][0] == exp[3]["big0"][0] + exp[3]["mid0"][0] + exp[3]["big1"][0] >= 45


def test_device_restart_counts_every_record_once(corpus, tmp_path):
    """A doubled piece outgrows the text a piece may hold (FTK_TEST_PIECE_LIMIT): the device path starts over with
    standard pieces.  The contig of fuzzed records in front holds negative starts; their count is exact."""
    path, exp = corpus["rising"]
    ratio_first, ratio_second, size_first, size_second = corpus["rising_ratios"]
    piece, room = 1 << 20, 32 << 20  # (kRoom of the stream)
    limit = room + int(1.5 * piece * ratio_second)
    assert room + 2 * piece * ratio_first < limit and size_first > 2.5 * piece and size_second > 3 * piece
    res, r = _run(tmp_path, _ROUTES_CHILD, path, ["*"], dict(FTK_STREAM_PIECE=str(piece), FTK_TEST_PIECE_LIMIT=str(limit)))
    assert "the device path starts over with standard pieces" in r.stderr, r.stderr[-2000:]
    print("[bam fuzz] rising:", [ln for ln in r.stderr.splitlines() if "starts over" in ln][:1])
    _check("rising", res, exp, "*")
    assert res["*"][1][0] == exp[3]["first"][0] >= 30
    _report("rising", r)


def test_region_streams_hold_every_read1_that_overlaps(corpus, tmp_path):
    """ftk_fragstream_open_region: every fragment whose read1 [r1s, r1e) overlaps the region (py_fetch's rule on the
    reference's rows), none that is not a row of the contig, in fragment-start order - regions at the contig ends, in
    runs of records with aux copies of headers, and at the top of the 1.1e9 contig."""
    top = H.BAM_COORD_LIMIT
    for name, specs in (("mixed", ["chr1:0:1", "chr1:0:50000", "chr1:1999000:2001000", "chr1:3990000:4000000",
                                   "chr2:1500000:1500001", "chr3:0:500000", "alt04:0:20000", "chrEmpty:0:1000"]),
                        ("top", [f"chrBig:{top - 1000}:{top}", f"chrBig:{top - 5}:{top + 10}", "chrBig:0:10000",
                                 "chrBig:500000000:600000000"])):
        want, _, rows, _ = corpus[name][1]
        for env in (dict(), dict(FTK_STREAM_PIECE=str(1 << 17))):
            res, _ = _run(tmp_path, _REGION_CHILD, corpus[name][0], specs, env)
            for spec in specs:
                c, a, b = spec.split(":")
                a, b = int(a), int(b)
                got = res[spec]
                w = want[c]
                kept = np.stack(w[:6], 1) if len(w[0]) else np.zeros((0, 6), np.int64)
                have = {}
                for row in map(tuple, kept.tolist()):
                    have[row] = have.get(row, 0) + 1
                need = [r for r in rows[c] if r[4] < b and r[5] > a and tuple(r) in have]  # py_fetch's overlap, kept rows
                assert len(need) == sum(1 for _ in O.py_fetch([r for r in rows[c] if tuple(r) in have], a, b, 0)), spec
                gk = {}
                for row in map(tuple, got.tolist()):
                    gk[row] = gk.get(row, 0) + 1
                assert all(gk[k] <= have.get(k, 0) for k in gk), (name, spec)  # rows of the contig, none more often
                nk = {}
                for row in need:
                    nk[tuple(row)] = nk.get(tuple(row), 0) + 1
                assert all(gk.get(k, 0) >= n for k, n in nk.items()), (name, spec, len(need), len(got))
                assert np.all(np.diff(got[:, 0]) >= 0), (name, spec)


def test_python_surface_on_fuzzed_contigs(corpus):
    """AlignmentWrapper.fetch and frag_generator on three contigs = py_fetch / py_frag_generator over the reference's
    rows without the dropped ones; the UserWarning names the number dropped; the CIGAR-less file raises TypeError."""
    from finaletoolkit_amd import source
    from finaletoolkit_amd.io import AlignmentWrapper
    from finaletoolkit_amd.utils import frag_generator
    path, (want, _, rows, per) = corpus["mixed"]
    kept = {c: [r for r in rr if r[0] >= 0 and r[1] < H.BAM_COORD_LIMIT and r[5] < H.BAM_COORD_LIMIT] for c, rr in rows.items()}
    source.close_all()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        got = [(f[1], f[2], f[3], f[4]) for f in frag_generator(path, "chr1", quality_threshold=0)]
    want_rows = [(fs, fe, q, bool(st)) for fs, fe, q, st in
                 O.py_frag_generator(kept["chr1"], None, None, None, None, "midpoint", 0)]
    assert got == want_rows
    counts = [int(m.group(1)) for w in seen if issubclass(w.category, UserWarning)
              for m in [re.search(r"(\d+) read1 record\(s\)", str(w.message))] if m]
    assert counts == [per["chr1"][0]], counts
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for q in (0, 30):
            with AlignmentWrapper(path, quality_threshold=q) as aw:
                for c, a, b in (("chr1", None, None), ("chr2", 1_000_000, 1_200_000), ("chr3", 0, 700), ("alt08", None, None)):
                    got = [(f.start, f.stop, f.mapq, f.is_forward) for f in aw.fetch(c, a, b)]
                    assert got == [(fs, fe, mq, bool(st)) for fs, fe, mq, st in O.py_fetch(kept[c], a, b, q)], (c, a, b, q)
        for c, a, b in (("chr2", 0, 3_000_000), ("chr3", 100_000, 200_000)):
            got = [(f[1], f[2], f[3], f[4]) for f in frag_generator(path, c, 20, a, b, 100, 500, "any")]
            assert got == [(fs, fe, mq, bool(st)) for fs, fe, mq, st in
                           O.py_frag_generator(kept[c], a, b, 100, 500, "any", 20)], (c, a, b)
    source.close_all()
    with pytest.raises(TypeError, match="NoneType"):
        list(frag_generator(corpus["nocigar"][0], "chrA", quality_threshold=0))
    source.close_all()
