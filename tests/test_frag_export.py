"""CPU: the surface of ``frag_export`` (names, signature, command line, argument errors that need no device) and the
full tabix writer ``bgzf.write_tabix`` held against a tabix READER written here from the format note (SAM spec 5.2 /
the tabix note): header, names, bins, chunks, linear index, ``reg2bins``, rows read at their virtual offsets."""
import gzip
import inspect
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- a tabix reader from the format note -------------------------------------------------------------------------
def read_tbi(path):
    raw = gzip.open(path, "rb").read()
    assert raw[:4] == b"TBI\1"
    n_ref, fmt, col_seq, col_beg, col_end, meta, skip, l_nm = struct.unpack_from("<8i", raw, 4)
    assert (fmt, col_seq, col_beg, col_end, meta, skip) == (0x10000, 1, 2, 3, ord("#"), 0)
    pos = 36
    names = raw[pos:pos + l_nm].split(b"\0")[:-1]
    assert len(names) == n_ref
    pos += l_nm
    refs = {}
    for name in names:
        (n_bin,) = struct.unpack_from("<i", raw, pos)
        pos += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", raw, pos)
            pos += 8
            bins[b] = [struct.unpack_from("<QQ", raw, pos + 16 * k) for k in range(n_chunk)]
            pos += 16 * n_chunk
        (n_intv,) = struct.unpack_from("<i", raw, pos)
        pos += 4
        linear = list(struct.unpack_from(f"<{n_intv}Q", raw, pos))
        pos += 8 * n_intv
        refs[name.decode()] = (bins, linear)
    assert pos == len(raw) or pos + 8 == len(raw)  # (optional n_no_coor)
    return [n.decode() for n in names], refs


def reg2bins(beg, end):
    """The tabix note's reg2bins: every bin that may hold a record overlapping [beg, end)."""
    out = [0]
    end -= 1
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += list(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


def spec_reg2bin(beg, end):
    """int reg2bin(int beg, int end) of the SAM spec, section 5.3, restated literally."""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def read_virtual(fh, v0, v1):
    """The uncompressed bytes of a BGZF file between two virtual offsets."""
    out = []
    coff, first = v0 >> 16, True
    while coff <= v1 >> 16:
        fh.seek(coff)
        head = fh.read(18)
        if len(head) < 18:
            break
        assert head[:4] == b"\x1f\x8b\x08\x04" and head[12:14] == b"BC"
        bsize = struct.unpack_from("<H", head, 16)[0] + 1
        data = zlib.decompress(fh.read(bsize - 18 - 8), -15)
        lo = (v0 & 0xFFFF) if first else 0
        hi = (v1 & 0xFFFF) if coff == v1 >> 16 else len(data)
        out.append(data[lo:hi])
        first = False
        coff += bsize
    return b"".join(out)


def tabix_query(path, refs, name, a, b):
    """Rows (as text lines) of ``name`` overlapping [a, b), found the way htslib finds them: the candidate bins'
    chunks, cut at the linear index's offset for the window of ``a``."""
    if name not in refs or b <= a:
        return []
    bins, linear = refs[name]
    w = a >> 14
    # (behind the last window a row reaches htslib takes the last entry; nothing overlaps there either way)
    min_off = linear[w] if w < len(linear) else (linear[-1] if linear else 0)
    chunks = sorted((max(v0, min_off), v1) for k in reg2bins(a, b) for v0, v1 in bins.get(k, []) if v1 > min_off)
    merged = []
    for v0, v1 in chunks:  # (htslib reads the candidate chunks in file order, overlapping ones as one)
        if merged and v0 <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], v1)
        else:
            merged.append([v0, v1])
    rows = []
    with open(path, "rb") as fh:
        for v0, v1 in merged:
            for line in read_virtual(fh, v0, v1).splitlines():
                f = line.split(b"\t")
                if int(f[1]) < b and int(f[2]) > a:
                    rows.append(line.decode())
    return rows


def region_set(rng, contig_len, n_random=150):
    """Random and boundary regions: 16 kb multiples +-1, the contig's ends, empty regions."""
    regs = []
    for _ in range(n_random):
        a = int(rng.integers(0, contig_len))
        regs.append((a, a + int(rng.integers(1, 60_000))))
    for k in (1, 2, 3, 7, 8, 9, 64, 65):
        w = k << 14
        if w < contig_len:
            regs += [(w - 1, w), (w, w + 1), (w - 1, w + 1), (w, w + (1 << 14)), (w + 1, w + (1 << 14) - 1), (w - 300, w + 300)]
    regs += [(0, 1), (0, 1 << 14), (0, contig_len), (contig_len - 1, contig_len), (contig_len - 20_000, contig_len + 50_000),
             (contig_len + 10, contig_len + 1000), (5000, 5000), (1 << 17, (1 << 17) + 5), ((1 << 20) - 3, (1 << 20) + 3)]
    return [(max(a, 0), b) for a, b in regs]


def brute(name, s, e, q, st, a, b, layout="frag"):
    keep = (s < b) & (e > a) if b > a else np.zeros(len(s), bool)
    return [fmt_row(name, s[i], e[i], q[i], st[i], layout) for i in np.nonzero(keep)[0]]


def fmt_row(name, s, e, q, st, layout="frag"):
    if layout == "bed3":
        return f"{name}\t{int(s)}\t{int(e)}"
    mid = ".\t" if layout == "bed6" else ""
    return f"{name}\t{int(s)}\t{int(e)}\t{mid}{int(q)}\t{'+' if st else '-'}"


# ---- 1. surface -----------------------------------------------------------------------------------------------------
def test_flat_name_signature_and_cli_flags():
    import finaletoolkit_amd as f
    from finaletoolkit_amd import utils
    from finaletoolkit_amd.export import build_parser
    assert f.frag_export is utils.frag_export
    sig = inspect.signature(utils.frag_export)
    assert list(sig.parameters) == ["input_file", "output_file", "contig", "quality_threshold", "min_length", "max_length",
                                    "layout", "workers", "verbose"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["contig"] is None and d["quality_threshold"] == 30 and d["min_length"] is None and d["max_length"] is None
    assert d["layout"] == "frag" and d["workers"] is None and d["verbose"] is False
    flags = [a.dest for a in build_parser()._actions if a.dest != "help"]
    assert sorted(flags) == sorted(sig.parameters)  # every flag an argument, every argument a flag
    f.install_alias("finaletoolkit", force=True)
    try:
        import finaletoolkit.utils as U
        assert U.frag_export is utils.frag_export
    finally:
        for k in [k for k in sys.modules if k == "finaletoolkit" or k.startswith("finaletoolkit.")]:
            del sys.modules[k]


def test_export_cli_help_exits_zero():
    r = subprocess.run([sys.executable, "-m", "finaletoolkit_amd.export", "--help"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "--layout" in r.stdout and "--min-length" in r.stdout


def test_bad_arguments_raise_before_any_device_use(tmp_path):
    from finaletoolkit_amd import utils
    src = os.path.join(ROOT, "tests", "data", "12.3444.b37.bam")
    with pytest.raises(ValueError, match="suffix"):
        utils.frag_export(src, str(tmp_path / "out.bed"))
    with pytest.raises(ValueError, match="suffix"):
        utils.frag_export(src, "-")
    with pytest.raises(ValueError, match="layout"):
        utils.frag_export(src, str(tmp_path / "out.frag.gz"), layout="bed12")
    same = tmp_path / "same.frag.gz"
    same.write_bytes(b"")
    with pytest.raises(ValueError, match="same"):
        utils.frag_export(str(same), str(same))
    assert not (tmp_path / "out.frag.gz").exists()


# ---- 2. the index writer ---------------------------------------------------------------------------------------------
def test_reg2bin_is_the_specs():
    from finaletoolkit_amd import bgzf
    rng = np.random.default_rng(5)
    spans = [(int(a), int(a) + 1 + int(rng.integers(0, 1 << int(rng.integers(1, 29))))) for a in rng.integers(0, 1 << 29, 10_000)]
    for shift in (14, 17, 20, 23, 26):
        for k in (1, 2, 5):
            edge = k << shift
            spans += [(edge - 1, edge), (edge - 1, edge + 1), (edge, edge + 1), (edge - 200, edge + 200), (edge - (1 << shift), edge),
                      (edge - (1 << shift), edge + 1)]
    spans += [(0, 1), (0, 1 << 29), ((1 << 29) - 1, 1 << 29), ((1 << 30) - 2, (1 << 30) - 1)]
    for a, b in spans:
        assert bgzf.reg2bin(a, b) == spec_reg2bin(a, b), (a, b)


def _numpy_index_inputs(name, s, e, q, st, offsets, first_byte):
    from finaletoolkit_amd import bgzf
    rb = bgzf.row_lengths(name, s, e, q)
    pos = first_byte + np.concatenate(([0], np.cumsum(rb)))
    bins = np.array([bgzf.reg2bin(int(a), int(b)) for a, b in zip(s, e)], np.int32)
    first = np.nonzero(np.concatenate(([True], bins[1:] != bins[:-1])))[0]
    end = np.concatenate((first[1:], [len(s)]))
    v = lambda p: bgzf.virtual_offset(offsets, int(p))  # noqa: E731
    runs = (bins[first], np.array([v(pos[i]) for i in first], np.uint64), np.array([v(pos[i]) for i in end], np.uint64))
    return dict(name=name, v_begin=v(pos[0]), v_end=v(pos[-1]), rows=len(s), linear=bgzf.linear_index(s, e, rb, offsets, first_byte),
                runs=runs), int(pos[-1])


def test_write_tabix_answers_region_queries(tmp_path):
    from finaletoolkit_amd import bgzf, synth
    contigs = []
    for k, (name, size) in enumerate((("chr7", 2_500_000), ("12", 1_200_000), ("empty", 1000))):
        s, e, q, st = synth.synth_contig(size, depth=3.0, seed=40 + k)
        if name == "12":  # long rows that straddle several windows and levels, rows at a window's edge
            extra_s = np.array([0, 16383, 16384, 100_000, 131_000, 900_000], np.int32)
            extra_e = np.array([1, 16384, 16385, 180_000, 132_000, 1_150_000], np.int32)
            s = np.concatenate((s, extra_s))
            e = np.concatenate((e, extra_e))
            q = np.concatenate((q, np.full(6, 60, np.uint8)))
            st = np.concatenate((st, np.ones(6, np.uint8)))
            o = np.argsort(s, kind="stable")
            s, e, q, st = s[o], e[o], q[o], st[o]
        if name == "empty":
            s, e, q, st = s[:0], e[:0], q[:0], st[:0]
        contigs.append((name, size, s, e, q, st))
    text = "".join(fmt_row(n, s[i], e[i], q[i], st[i]) + "\n" for n, _, s, e, q, st in contigs for i in range(len(s))).encode()
    path = str(tmp_path / "rows.frag.gz")
    offsets = bgzf.write_bgzf(path, text, level=1)
    assert len(offsets) > 12  # many blocks: chunks start and end inside blocks
    index, first = [], 0
    for n, _, s, e, q, st in contigs:
        if len(s) == 0:
            index.append(dict(name=n, v_begin=0, v_end=0, rows=0, linear=np.zeros(0, np.uint64),
                              runs=(np.zeros(0, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint64))))
            continue
        item, first = _numpy_index_inputs(n, s, e, q, st, offsets, first)
        index.append(item)
    bgzf.write_tabix(path + ".tbi", index)
    names, refs = read_tbi(path + ".tbi")
    assert names == ["chr7", "12"]  # contigs without rows are not listed
    for n, size, s, e, q, st in contigs[:2]:
        bins, linear = refs[n]
        assert bins[37450] == [(index[names.index(n)]["v_begin"], index[names.index(n)]["v_end"]), (len(s), 0)]
        assert set(bins) - {37450} == {spec_reg2bin(int(a), int(b)) for a, b in zip(s, e)}
        rng = np.random.default_rng(len(s))
        regs = region_set(rng, size)
        assert len(regs) > 150
        hits = 0
        for a, b in regs:
            got = tabix_query(path, refs, n, a, b)
            want = brute(n, s, e, q, st, a, b)
            assert sorted(got) == sorted(want), (n, a, b)
            hits += len(want)
        assert hits > 1000
    assert tabix_query(path, refs, "empty", 0, 1000) == [] and tabix_query(path, refs, "chrNone", 0, 1000) == []
