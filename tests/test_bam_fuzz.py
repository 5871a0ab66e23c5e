"""BAM input against an INDEPENDENT statement of the reference's record rule: seeded adversarial BAMs
(tests/helpers.py: every CIGAR op, every flag bit, TLEN of any sign, names of 1-254 bytes, records longer than a
16 KB stretch, aux tags that carry copies of a neighbouring record's header, negative fragment starts, empty and
all-rejected contigs, contig runs that change inside a piece, unplaced reads, a contig of 1.1e9 bases whose fragments
reach 2^30) decoded by the host decoders and compared, exactly and in order, with oracle.bam_rows - the pure-Python
parser pinned to the reference's own _fetch_sam by tests/golden/bam.json.gz.  The host decoders and the device parser
share csrc/ftk_bamrule.h; only a comparison like this one can catch a mistake in that rule.  The device routes over the
same corpus: tests/test_gpu_bam_fuzz.py."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from finaletoolkit_amd import _lib as L
from finaletoolkit_amd import bgzf
from tests import helpers as H
from tests.test_abi import _decode

# (name, length, records, negative-start fragments, kind)
MIXED = ([("chr1", 4_000_000, 45_000, 20, "fuzz"), ("chrEmpty", 1_000, 0, 0, "fuzz"), ("chrRej", 300_000, 2_000, 0, "rejected")]
         + [(f"alt{k:02d}", 20_000, 1 + k % 5, 1 if k % 4 == 0 else 0, "fuzz") for k in range(40)]
         + [("chr2", 3_000_000, 45_000, 10, "fuzz"), ("chr3", 500_000, 20_000, 0, "fuzz")])
# more contig runs in one 64 KB piece than the device parser lists (kBamMaxRuns): the device stream hands the file to
# the host decoder.  Negative starts in big0 (handed out before that), in mid0 (pieces parsed, not yet handed out)
# and in big1 (behind it).
ALTS = ([("big0", 1_500_000, 20_000, 25, "fuzz"), ("mid0", 1_000_000, 10_000, 15, "fuzz")]
        + [(f"alt{k:03d}", 20_000, 1, 0, "lite") for k in range(150)] + [("big1", 600_000, 10_000, 5, "fuzz")])


def _rising(path, tmp):
    """The layout of test_gpu_inflate.py::test_bam_whose_compression_rises_behind_its_first_piece_stays_on_the_device
    with fuzzed records (negative starts among them) in front of long constant reads: a doubled piece of the second
    contig outgrows the text a piece may hold and the device path starts over.  Returns the compression ratios of the
    two parts."""
    contigs = [("first", 3_600_000), ("second", 4_000_000)]
    a, b = str(tmp / "rising_a.bam"), str(tmp / "rising_b.bam")
    H.write_fuzz_bam(a, 71, [("first", 3_600_000, 90_000, 30, "fuzz"), ("second", 4_000_000, 0, 0, "fuzz")])
    rng = np.random.default_rng(73)
    n = 4_000_000 // 30
    s = np.sort(rng.integers(0, 4_000_000 - 2_000, n))
    H.write_synthetic_bam(b, contigs, {"second": (s, s + rng.integers(420, 900, n), rng.integers(0, 61, n),
                                                  rng.integers(0, 2, n).astype(bool))}, read_len=400, junk=False)
    ra, rb = gzip.open(a, "rb").read(), gzip.open(b, "rb").read()
    head = 12 + int.from_bytes(ra[4:8], "little") + sum(8 + len(c) + 1 for c, _ in contigs)
    assert ra[:head] == rb[:head]
    offs = bgzf.write_bgzf(path, ra + rb[head:], level=6)
    bgzf.write_index(path + ".bai", True, [("first", bgzf.virtual_offset(offs, head), bgzf.virtual_offset(offs, len(ra))),
                                           ("second", bgzf.virtual_offset(offs, len(ra)),
                                            bgzf.virtual_offset(offs, len(ra) + len(rb) - head))])
    front = os.path.getsize(a)
    return len(ra) / front, (len(rb) - head) / max(os.path.getsize(path) - front, 1), front, os.path.getsize(path) - front


def build_corpus(tmp):
    """{name: (path, helpers.bam_expected(path))} for the fuzzed files; "rising_ratios": what _rising returned."""
    files = {}
    for name, write in (("mixed", lambda p: H.write_fuzz_bam(p, 20261016, MIXED, unplaced=400)),
                        ("alts", lambda p: H.write_fuzz_bam(p, 20261017, ALTS, unplaced=20)),
                        ("top", lambda p: H.write_top_bam(p, 20261018)),
                        ("nocigar", lambda p: H.write_nocigar_bam(p, 20261019))):
        files[name] = str(tmp / f"{name}.bam")
        write(files[name])
    files["rising"] = str(tmp / "rising.bam")
    ratios = _rising(files["rising"], tmp)
    out = {k: (v, H.bam_expected(v)) for k, v in files.items()}
    out["rising_ratios"] = ratios
    return out


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return build_corpus(tmp_path_factory.mktemp("fuzzbam"))


def assert_table(what, rows, cols, rank, want):
    """One contig's table (columns in stable start order + file-order rank) equal to the reference's, exactly."""
    assert rows == len(want[0]), (what, rows, len(want[0]))
    if rows == 0:
        return
    for k, name in enumerate(("start", "end", "mapq", "strand", "r1_start", "r1_end")):
        got = np.asarray(cols[k], np.int64)
        bad = np.flatnonzero(got != want[k])
        assert bad.size == 0, (what, name, "row", int(bad[0]), "got", int(got[bad[0]]), "want", int(want[k][bad[0]]), bad.size)
    assert np.array_equal(np.asarray(rank, np.int64), want[6]), (what, "file order")


def _host_order(lib, t, i, rows):
    p = C.c_void_p()
    assert lib.ftk_fragtable_order(t, i, C.byref(p)) == 0 and (p.value or rows == 0)
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), (rows,)).copy() if rows else np.zeros(0, np.int32)


def _whole(path, contig=None, threads=3):
    """ftk_bam_decode: {contig: (rows, cols, rank)} and its skipped counts."""
    lib = L.load()
    t = C.c_void_p()
    rc = lib.ftk_bam_decode(path.encode(), None if contig is None else contig.encode(), threads, C.byref(t))
    assert rc == 0, lib.ftk_fragtable_error().decode()
    try:
        ranks = {}
        for i in range(lib.ftk_fragtable_n_contigs(t)):
            rows = lib.ftk_fragtable_contig_rows(t, i)
            ranks[lib.ftk_fragtable_contig_name(t, i).decode()] = (rows, _host_order(lib, t, i, rows))
        sk = (C.c_int64 * 2)()
        assert lib.ftk_fragtable_skipped(t, C.byref(sk)) == 0
    finally:
        lib.ftk_fragtable_free(t)
    cols = _decode(path, bam=True, contig=contig, threads=threads)
    return {c: (r, cols[c][1], rank) for c, (r, rank) in ranks.items()}, list(sk)


def _host_stream(path, contig=None, threads=3):
    """ftk_fragstream_open (the host stream): {contig: (rows, cols, rank)}, the order, its skipped counts."""
    lib = L.load()
    s = C.c_void_p()
    assert lib.ftk_fragstream_open(path.encode(), None if contig is None else contig.encode(), 1, threads, 2, C.byref(s)) == 0
    out, order = {}, []
    try:
        while True:
            t = C.c_void_p()
            assert lib.ftk_fragstream_next(s, C.byref(t)) == 0, lib.ftk_fragtable_error().decode()
            if not t.value:
                break
            rows = lib.ftk_fragtable_contig_rows(t, 0)
            name = lib.ftk_fragtable_contig_name(t, 0).decode()
            ps = [C.c_void_p() for _ in range(6)]
            assert lib.ftk_fragtable_columns(t, 0, *[C.byref(p) for p in ps]) == 0
            cols = [np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), (rows,)).copy() for p, ct in
                    zip(ps, (C.c_int32, C.c_int32, C.c_uint8, C.c_uint8, C.c_int32, C.c_int32))]
            out[name] = (rows, cols, _host_order(lib, t, 0, rows))
            order.append(name)
            lib.ftk_fragtable_free(t)
        sk = (C.c_int64 * 2)()
        assert lib.ftk_fragstream_skipped(s, C.byref(sk)) == 0
    finally:
        lib.ftk_fragstream_close(s)
    return out, order, list(sk)


def test_corpus_reaches_the_edges(corpus):
    """The files hold what they are meant to: dropped fragments, empty and all-rejected contigs, CIGAR-less reverse
    read1 records, fragments that end just below 2^30, aux copies of record headers, records beyond a 16 KB stretch."""
    want, _, _, per = corpus["mixed"][1]
    assert len(want["chrEmpty"][0]) == 0 and len(want["chrRej"][0]) == 0 and per["chr1"][0] >= 20
    assert sum(len(v[0]) for v in want.values()) > 30_000
    assert corpus["nocigar"][1][1][1] == 3 and corpus["alts"][1][3]["big0"][0] >= 25 and corpus["rising"][1][3]["first"][0] >= 30
    top = corpus["top"][1]
    assert top[3]["chrBig"][0] >= 5 + 2 * 3 + 1 + 1  # negative starts, ends at / beyond 2^30, the stray TLEN, read1_past
    assert int(top[0]["chrBig"][1].max()) == H.BAM_COORD_LIMIT - 1
    data = gzip.open(corpus["mixed"][0], "rb").read()
    assert data.count(b"XBBC") > 1000 and data.count(b"XZZ") > 1000
    assert corpus["rising_ratios"][1] > 1.6 * corpus["rising_ratios"][0]


@pytest.mark.parametrize("name", ["mixed", "alts", "top", "rising", "nocigar"])
def test_host_decoders_hold_the_reference_rows_of_fuzzed_bams(corpus, name):
    """ftk_bam_decode (1 and 4 threads) and the host stream: per contig exactly the reference's rows - start, end,
    mapq, strand, read1's [pos, bam_endpos), in stable start order with the file rank - and exactly the reference's
    count of fragments the columns cannot hold and of CIGAR-less reverse read1 records."""
    path, (want, skipped, _, _) = corpus[name]
    for threads in (1, 4):
        got, sk = _whole(path, threads=threads)
        assert sorted(got) == sorted(want)
        for c in want:
            assert_table((name, c, threads), *got[c], want[c])
        assert sk == skipped, (name, threads)
    got, order, sk = _host_stream(path)
    assert order == [c for c in want if len(want[c][0])]
    for c in order:
        assert_table((name, c, "stream"), *got[c], want[c])
    assert sk == skipped, (name, "stream")


@pytest.mark.parametrize("name,contig", [("mixed", "chr2"), ("mixed", "alt20"), ("mixed", "alt21"), ("top", "chrBig"), ("alts", "big0")])
def test_host_decoders_of_one_contig(corpus, name, contig):
    """One contig by name (whole-file decoder) and through the BAI (host stream): its rows and its own counts."""
    path, (want, _, _, per) = corpus[name]
    got, sk = _whole(path, contig)
    assert_table((name, contig), *got[contig], want[contig])
    assert sk == per[contig]
    got, order, sk = _host_stream(path, contig)
    assert order == ([contig] if len(want[contig][0]) else [])
    if order:
        assert_table((name, contig, "stream"), *got[contig], want[contig])
    assert sk == per[contig]


def test_oracle_counts_what_the_reference_raises_on(corpus):
    """bam_rows raises TypeError by default (the reference's None + tlen) and counts those records with count_nocigar."""
    from oracle import oracle as O
    path = corpus["nocigar"][0]
    with pytest.raises(TypeError):
        O.bam_rows(path)
    _, _, rows, n = O.bam_rows(path, count_nocigar=True)
    assert n == {"chrA": 3, "chrB": 0} and sum(r[4] == 60_000 and r[1] - r[0] == 250 for r in rows["chrA"]) == 1
