"""GPU: the write direction (``csrc/ftk_fragtext.hip``) - device row formatter against the host formatter, the device
BGZF deflate against zlib and against the project's own device inflate, and ``frag_export`` round trips with the index
read back by a tabix reader written from the format note (``tests/test_frag_export.py``) and by ``AlignmentWrapper``.

Compressed size: the device / host(level 1) ratios asserted in ``test_fraggz_roundtrip_at_scale`` are the ones measured
on an MI355X and recorded in ``profiles/export_ratio.txt`` (the compressor is deterministic)."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_frag_export as T  # noqa: E402  (the tabix reader and the region set)

pytestmark = pytest.mark.gpu
ROOT = T.ROOT
BAM = os.path.join(ROOT, "tests", "data", "12.3444.b37.bam")
LAYOUTS = ("frag", "bed6", "bed3")
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
# device bytes / host level-1 bytes on the file of test 6 (profiles/export_ratio.txt); 5 % of room for another seed
RATIO_SCALE = 1.036


def numpy_keep(s, e, q, mapq_min, min_len, max_len):
    ln = e.astype(np.int64) - s
    keep = q >= mapq_min
    if min_len is not None:
        keep &= ln >= min_len
    if max_len is not None:
        keep &= ln <= max_len
    return keep


def host_rows(name, s, e, q, st, layout):
    from finaletoolkit_amd import writers
    with writers.frag_rows(name, s, e, q, st, layout == "bed6") as rows:
        text = rows.tobytes()
    if layout == "bed3":  # the host formatter's first three columns
        text = b"".join(b"\t".join(ln.split(b"\t")[:3]) + b"\n" for ln in text.splitlines())
    return text


def check_format(engine, key, name, s, e, q, st, filters):
    engine.load_contig(key, s, e, q, st)
    try:
        for mapq_min, mn, mx in filters:
            keep = numpy_keep(s, e, q, mapq_min, mn, mx)
            for layout in LAYOUTS:
                got, rows = engine.format_rows(key, name, mapq_min, mn, mx, layout)
                assert rows == int(keep.sum()), (name, layout, mapq_min, mn, mx)
                assert got == host_rows(name, s[keep], e[keep], q[keep], st[keep], layout), (name, layout, mapq_min, mn, mx)
    finally:
        engine.release(key)


# ---- 3. formatter ---------------------------------------------------------------------------------------------------
def test_formatter_equals_host_formatter_on_a_synthetic_contig(engine):
    from finaletoolkit_amd import synth
    s, e, q, st = synth.synth_contig(1_000_000, depth=30.0, seed=11)
    if len(s) % 4 == 0:
        s, e, q, st = s[:-1], e[:-1], q[:-1], st[:-1]
    assert len(s) % 4 and len(s) > 90_000
    ln = (e - s).astype(np.int64)
    one = int(np.nonzero((ln == ln.max()) & (q >= 0))[0][0])
    only = [(0, int(ln[one]), None)] if (ln == ln.max()).sum() == 1 else []
    filters = [(0, None, None), (30, None, None), (30, 120, 180), (256, None, None), (0, 5, 4), (0, int(np.median(ln)), int(np.median(ln))),
               (0, int(np.median(ln)), None), (0, None, int(np.median(ln)))] + only
    for name in ("7", "12", "chr21", "chrUn_GL000220v1_alt_xyz"):
        assert len(name) in (1, 2, 5, 24)
        check_format(engine, "fmt:" + name, name, s, e, q, st, filters if name == "chr21" else filters[:3])


def test_formatter_digit_count_edges_and_empty_contig(engine):
    edges = [0, 9, 10, 99, 100, 999, 1000, 9999, 10_000, 99_999, 100_000, 999_999, 1_000_000, 9_999_999, 10_000_000,
             99_999_999, 100_000_000, 999_999_999, 1_000_000_000, (1 << 30) - 1]
    ss, ee = [], []
    for a in edges:
        for b in edges:
            if b >= a:
                ss.append(a)
                ee.append(b)
    s, e = np.array(ss, np.int32), np.array(ee, np.int32)
    mq = np.array([0, 9, 10, 99, 100, 255], np.uint8)
    q = mq[np.arange(len(s)) % 6]
    st = (np.arange(len(s)) % 3 == 0).astype(np.uint8)
    o = np.argsort(s, kind="stable")
    s, e, q, st = s[o], e[o], q[o], st[o]
    filters = [(0, None, None), (10, None, None), (100, 0, 0), (0, 1, 1), (0, 999_999_999, None), (256, None, None)]
    one = [(0, (1 << 30) - 1, None)]  # exactly one row: [0, 2^30 - 1)
    assert int(numpy_keep(s, e, q, *one[0]).sum()) == 1
    check_format(engine, "fmt:edges", "chr1", s, e, q, st, filters + one)
    z32, z8 = np.zeros(0, np.int32), np.zeros(0, np.uint8)
    check_format(engine, "fmt:empty", "chr1", z32, z32, z8, z8, [(0, None, None)])


def test_formatter_argument_errors(engine):
    from finaletoolkit_amd import _lib as L
    z32, z8 = np.zeros(1, np.int32), np.zeros(1, np.uint8)
    engine.load_contig("fmt:err", z32, z32 + 5, z8, z8)
    out, n, rows = C.c_void_p(), C.c_int64(), C.c_int64()
    lib, cid = engine.lib, engine.contig_id("fmt:err")
    assert lib.ftk_frags_format_rows(engine.ctx, cid, b"c", 0, -1, -1, 7, C.byref(out), C.byref(n), C.byref(rows)) == L.FTK_ERR_INVALID
    assert lib.ftk_frags_format_rows(engine.ctx, cid, b"", 0, -1, -1, 0, C.byref(out), C.byref(n), C.byref(rows)) == L.FTK_ERR_INVALID
    assert lib.ftk_frags_format_rows(engine.ctx, 987654, b"c", 0, -1, -1, 0, C.byref(out), C.byref(n), C.byref(rows)) == L.FTK_ERR_NO_CONTIG
    res = L.ExportResult()
    assert lib.ftk_frags_write(engine.ctx, cid, b"c", 0, -1, -1, 0, b"/nonexistent-dir/x.gz", 0, 1, 0, C.byref(res)) == L.FTK_ERR_IO
    engine.release("fmt:err")


# ---- 4. deflate -----------------------------------------------------------------------------------------------------
def split_members(image):
    pos, members = 0, []
    while pos < len(image):
        head = image[pos:pos + 18]
        assert head[:4] == b"\x1f\x8b\x08\x04" and head[10:12] == b"\x06\x00" and head[12:16] == b"BC\x02\x00"
        bsize = struct.unpack_from("<H", head, 16)[0] + 1
        assert bsize <= 65536
        crc, isize = struct.unpack_from("<II", image, pos + bsize - 8)
        members.append((image[pos + 18:pos + bsize - 8], crc, isize, bsize))
        pos += bsize
    assert pos == len(image)
    return members


def test_device_deflate_against_zlib_and_the_device_inflate(engine):
    from finaletoolkit_amd import synth
    B = 0xFF00
    s, e, q, st = synth.synth_contig(3_000_000, depth=30.0, seed=5)
    frag = host_rows("chr9", s, e, q, st, "frag")
    assert len(frag) > 10 * B + 7
    rng = np.random.default_rng(1)
    row = b"chr1\t1000000\t1000167\t60\t+\n"
    kinds = {"frag": frag, "zeros": bytes(11 * B), "row": row * (11 * B // len(row) + 1),
             "random": rng.integers(0, 256, 11 * B, dtype=np.uint8).tobytes()}
    for kind, data in kinds.items():
        for n in (0, 1, B - 1, B, B + 1, 10 * B + 7):
            text = data[:n]
            image, offs = engine.bgzf_deflate(text)
            again, _ = engine.bgzf_deflate(text)
            assert image == again, (kind, n)  # deterministic
            assert image[-28:] == EOF
            members = split_members(image[:-28])
            assert len(members) == -(-n // B) and len(offs) == len(members) + 1
            pos = 0
            for k, (payload, crc, isize, bsize) in enumerate(members):
                piece = text[k * B:(k + 1) * B]
                assert offs[k] == pos
                assert zlib.decompress(payload, -15) == piece, (kind, n, k)
                assert crc == zlib.crc32(piece) and isize == len(piece), (kind, n, k)
                pos += bsize
            assert offs[-1] == pos
            assert gzip.decompress(image) == text
            # the stored bound, derived: a member is 18 bytes of header, a stored block's 5-byte header, the data and
            # 8 bytes of trailer = data + 31 (26 leaves out the stored block's own header: one byte cannot be coded in
            # less than 3 bytes of DEFLATE by any encoder - zlib's member for it is 29 bytes too)
            assert len(image) <= n + 31 * len(members) + 28, (kind, n)
            no_eof, _ = engine.bgzf_deflate(text, write_eof=False)
            assert no_eof == image[:-28]
            out = np.zeros(max(n, 1), np.uint8)
            got = C.c_int64()
            src = np.frombuffer(image, np.uint8)
            rc = engine.lib.ftk_bgzf_inflate_device(engine.ctx, src.ctypes.data_as(C.c_void_p), len(image),
                                                    out.ctypes.data_as(C.c_void_p), n, C.byref(got))
            assert rc == 0 and got.value == n and out[:n].tobytes() == text, (kind, n)
    # a capacity that is too small: FTK_ERR_INVALID with the size needed
    src = np.frombuffer(frag[:B], np.uint8)
    small, got = np.zeros(16, np.uint8), C.c_int64()
    rc = engine.lib.ftk_bgzf_deflate_device(engine.ctx, src.ctypes.data_as(C.c_void_p), B, small.ctypes.data_as(C.c_void_p), 16,
                                            C.byref(got), None, 1)
    assert rc == -1 and got.value == len(engine.bgzf_deflate(frag[:B])[0])


# ---- 5. BAM -> frag.gz ----------------------------------------------------------------------------------------------
def expected_rows(path, contig, q):
    from finaletoolkit_amd.utils import frag_generator
    rows = list(frag_generator(path, contig, quality_threshold=q))
    return sorted(rows, key=lambda r: r[1])  # (sorted() is stable)


def check_bam_roundtrip(tmp_path, bam, contig, size, q, tag):
    from finaletoolkit_amd import source, utils
    want = expected_rows(bam, contig, q)
    assert want
    out = str(tmp_path / f"{tag}.q{q}.frag.gz")
    written = utils.frag_export(bam, out, contig=contig, quality_threshold=q)
    assert written == {contig: len(want)}
    text = "".join(T.fmt_row(*r) + "\n" for r in want)
    assert gzip.open(out, "rt").read() == text
    assert list(utils.frag_generator(out, contig, quality_threshold=0)) == want
    # the same features from the BAM and from the export.  Whole-contig calls on both sources; the tiling windows are
    # region calls, which a BAM answers by read1 overlap and a fragment file by fragment overlap,
    # so for them the BAM's side is its fragments (frag_generator's rows) held as plain columns
    eng = source.get_engine()
    kb = source.open_source(bam).require(contig)
    ke = source.open_source(out).require(contig)
    s = np.array([r[1] for r in want], np.int32)
    e = np.array([r[2] for r in want], np.int32)
    mq = np.array([r[3] for r in want], np.uint8)
    st = np.array([r[4] for r in want], np.uint8)
    eng.load_contig("rt:cols", s, e, mq, st)
    ws = np.arange(0, size, 5000, dtype=np.int32)
    we = np.minimum(ws + 5000, size).astype(np.int32)
    lo, hi = int(s.min()), int(e.max())
    for policy in ("midpoint", "any"):
        assert eng.window_counts(kb, [None], [None], q, None, None, policy)[0] == len(want)
        assert eng.window_counts(ke, [None], [None], q, None, None, policy)[0] == len(want)
        cov = eng.window_counts(ke, ws, we, q, None, None, policy)
        assert np.array_equal(cov, eng.window_counts("rt:cols", ws, we, q, None, None, policy)) and cov.sum() >= len(want) - 2
        hb, ob = eng.fraglen_hist(kb, [None], [None], 0, 1001, q, None, None, policy)
        he, oe = eng.fraglen_hist(ke, [None], [None], 0, 1001, q, None, None, policy)
        assert np.array_equal(hb, he) and np.array_equal(ob, oe) and int(he.sum() + oe.sum()) == len(want)
    a, b = max(lo - 500, 0), min(hi + 500, size)
    assert np.array_equal(eng.wps(kb, a, b, size, quality_threshold=q), eng.wps(ke, a, b, size, quality_threshold=q))
    eng.release("rt:cols")
    return out


@pytest.mark.parametrize("q", [0, 30])
def test_bam_fixture_roundtrip(tmp_path, q):
    check_bam_roundtrip(tmp_path, BAM, "12", 133_851_895, q, "fixture")


def test_synthetic_bam_roundtrip_both_strands(tmp_path):
    from finaletoolkit_amd import synth
    bam = str(tmp_path / "w.bam")
    exp = synth.write_paired_bam(bam, "w", 400_000, 60.0, 99, read_len=50)
    assert 0 < exp["st"].sum() < len(exp["st"])
    check_bam_roundtrip(tmp_path, bam, "w", 400_000, 30, "synth")


# ---- 6 - 8. frag.gz -> filtered frag.gz at scale, its index, the host-deflate switch -----------------------------------
SCALE = (("chr19", 59_128_983), ("chr20", 63_025_520), ("chr21", 48_129_895), ("chr22", 51_304_566))


@pytest.fixture(scope="module")
def scale_files(tmp_path_factory):
    from finaletoolkit_amd import bgzf, source, synth, utils
    d = tmp_path_factory.mktemp("export_scale")
    src = str(d / "in.frag.gz")
    cols = {n: synth.synth_contig(size, depth=30.0, seed=300 + k) for k, (n, size) in enumerate(SCALE)}
    bgzf.write_frag_gz_contigs(src, ((n, *cols[n]) for n, _ in SCALE), level=1)
    out = str(d / "out.frag.gz")
    written = utils.frag_export(src, out, quality_threshold=30, min_length=120, max_length=180)
    yield src, out, cols, written
    source.close_all()


def test_fraggz_roundtrip_at_scale(scale_files, tmp_path):
    from finaletoolkit_amd import source, writers
    src, out, cols, written = scale_files
    kept = {}
    for n, _ in SCALE:
        s, e, q, st = cols[n]
        k = numpy_keep(s, e, q, 30, 120, 180)
        kept[n] = (s[k], e[k], q[k], st[k])
        assert written[n] == int(k.sum()) and written[n] > 1_000_000
    assert list(written) == [n for n, _ in SCALE]
    eng = source.get_engine()
    back = source.open_source(out)
    assert back.contigs == [n for n, _ in SCALE]
    host_bytes = 0
    for n, _ in SCALE:
        s, e, q, st = kept[n]
        gs, ge, gq, gst = eng.frag_select(back.require(n), None, None, 0, None, None, "midpoint")
        assert np.array_equal(gs, s) and np.array_equal(ge, e) and np.array_equal(gq, q) and np.array_equal(gst != 0, st != 0), n
        with writers.frag_rows(n, s, e, q, st) as rows:  # the size yardstick: the same text at level 1 on the host
            assert rows.n > 1000 * 0xFF00  # (over a thousand blocks per contig, thousands per file)
            offs = writers.bgzf_write(str(tmp_path / "host.gz"), rows, 1, append=False, write_eof=False)
            host_bytes += int(offs[-1])
    ratio = (os.path.getsize(out) - 28) / host_bytes
    print(f"export size: device {os.path.getsize(out) - 28} B, host level 1 {host_bytes} B, ratio {ratio:.4f}")
    assert abs(ratio - RATIO_SCALE) <= 0.05 * RATIO_SCALE, ratio


def check_index_answers(path, cols_by_contig, sizes):
    from finaletoolkit_amd import source
    from finaletoolkit_amd.io import AlignmentWrapper
    names, refs = T.read_tbi(path + ".tbi")
    assert names == [n for n in cols_by_contig if len(cols_by_contig[n][0])]
    source.close_all()  # a cold source: the region goes through the linear index
    aw = AlignmentWrapper(path)
    try:
        for n in names:
            s, e, q, st = cols_by_contig[n]
            regs = T.region_set(np.random.default_rng(len(s)), sizes[n], n_random=40)
            for a, b in regs:
                want = T.brute(n, s, e, q, st, a, b)
                assert sorted(T.tabix_query(path, refs, n, a, b)) == sorted(want), (n, a, b)
                if b > a:
                    got = [T.fmt_row(f.contig, f.start, f.stop, f.mapq, f.is_forward) for f in aw.fetch(n, a, b)]
                    assert sorted(got) == sorted(want), (n, a, b)
    finally:
        aw.close()


def test_index_of_the_product_file(scale_files):
    src, out, cols, written = scale_files
    kept = {}
    for n, _ in SCALE:
        s, e, q, st = cols[n]
        k = numpy_keep(s, e, q, 30, 120, 180)
        kept[n] = (s[k], e[k], q[k], st[k])
    check_index_answers(out, kept, dict(SCALE))


def test_host_deflate_switch_gives_the_same_text_and_index_answers(scale_files, tmp_path):
    src, out, cols, written = scale_files
    host_out = str(tmp_path / "host.frag.gz")
    code = ("import sys; sys.path.insert(0, %r); from finaletoolkit_amd import utils; "
            "print(utils.frag_export(%r, %r, contig='chr21', quality_threshold=30, min_length=120, max_length=180))" % (ROOT, src, host_out))
    env = dict(os.environ, FTK_EXPORT_DEFLATE="host")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    dev_out = str(tmp_path / "dev.frag.gz")
    from finaletoolkit_amd import utils
    assert utils.frag_export(src, dev_out, contig="chr21", quality_threshold=30, min_length=120, max_length=180) == {"chr21": written["chr21"]}
    a, b = open(dev_out, "rb").read(), open(host_out, "rb").read()
    assert a != b and gzip.decompress(a) == gzip.decompress(b)
    s, e, q, st = cols["chr21"]
    k = numpy_keep(s, e, q, 30, 120, 180)
    kept = {"chr21": (s[k], e[k], q[k], st[k])}
    check_index_answers(host_out, kept, dict(SCALE))
    check_index_answers(dev_out, kept, dict(SCALE))
