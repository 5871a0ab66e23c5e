"""CPU: zlib judges every member that ``tests/deflate_writer.py`` builds for the device inflate's tests - the named
catalogue and the token-level fuzz - before any GPU sees one: class A is accepted with the expected bytes, classes B and
C are refused; and ``tests/deflate_tokens.py`` reads back from every class A stream exactly what the writer was told
(tokens, the three code-length tables, the code-length symbol sequence), so a member is what its name says."""
import time
import zlib

import pytest

from tests import deflate_tokens as D
from tests import deflate_writer as W

T0 = time.perf_counter()
CASES = W.catalogue()
FUZZ = W.fuzz()
BUILD_SECONDS = time.perf_counter() - T0


def _raw_verdict(raw):
    """(accepted, bytes) of zlib on the raw DEFLATE stream: accepted = no error and the final block seen."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(raw) + d.flush()
    except zlib.error:
        return False, None
    return d.eof, out


def _gzip_verdict(member):
    d = zlib.decompressobj(31)
    try:
        out = d.decompress(member) + d.flush()
    except zlib.error:
        return False, None
    return d.eof and not d.unused_data, out


def _check_accepted(case):
    ok, out = _raw_verdict(case.raw)
    assert ok and out == case.data, case.name
    ok, out = _gzip_verdict(case.member())
    assert ok and out == case.data, case.name
    assert W.fits(case.raw, case.data, case.extra), case.name
    if not case.tokens_ok:
        with pytest.raises(D.InflateError):
            D.inflate(case.raw)
        return
    blocks, used = D.inflate(case.raw)
    assert used == len(case.raw) and len(blocks) == len(case.blocks), case.name
    for k, (got, told) in enumerate(zip(blocks, case.blocks)):
        assert got.btype == told["btype"] and got.final == told["final"], (case.name, k)
        assert got.tokens == told["tokens"], (case.name, k)
        if got.btype == "dynamic":
            assert got.ll_lengths == told["ll_lengths"] and got.d_lengths == told["d_lengths"], (case.name, k)
            assert got.cl_lengths == told["cl_lengths"] and got.cl_symbols == told["cl_symbols"], (case.name, k)


def test_catalogue_and_fuzz_build_in_seconds():
    assert BUILD_SECONDS < 10.0, BUILD_SECONDS
    assert len(FUZZ) == 150 and sum(len(c.data) > 40_000 for c in FUZZ) >= 5
    assert {c.cls for c in CASES} == {"A", "B", "C"}


@pytest.mark.parametrize("case", [c for c in CASES if c.cls == "A"], ids=lambda c: c.name)
def test_zlib_accepts_class_a(case):
    _check_accepted(case)


def test_zlib_accepts_every_fuzz_member():
    for case in FUZZ:
        _check_accepted(case)
    # the fuzz reaches what it is meant to reach
    dists = {t[1] for c in FUZZ for b in c.blocks for t in b["tokens"] if not isinstance(t, int)}
    assert {1, 2, 258, 1726, 1727, 2048, 2049, 32506, 32507, 32767, 32768} <= dists
    assert {b["btype"] for c in FUZZ for b in c.blocks} == {"stored", "fixed", "dynamic"}
    assert max(max(b["ll_lengths"]) for c in FUZZ for b in c.blocks if b["btype"] == "dynamic") == 15


@pytest.mark.parametrize("case", [c for c in CASES if c.cls in "BC"], ids=lambda c: c.name)
def test_zlib_refuses_classes_b_and_c(case):
    assert not _gzip_verdict(case.member())[0], case.name
    ok, out = _raw_verdict(case.raw)
    if case.raw_refused:
        assert not ok, case.name
    elif ok:  # the stream is sound: it is the trailer that does not describe it
        assert len(out) != len(case.data) or (zlib.crc32(out) & 0xFFFFFFFF) != (case.crc if case.crc is not None else zlib.crc32(case.data) & 0xFFFFFFFF)
    if case.cls == "B":  # (class C is zlib's stricter rule, which the token reader shares)
        try:
            D.inflate(case.raw)
        except D.InflateError:
            return
        assert not case.raw_refused, case.name


def _crossing(block):
    """The repeat symbols of a dynamic header that span the end of the literal / length lengths."""
    at, crossing = 0, []
    for s, extra in block.cl_symbols:
        n = 1 if s < 16 else extra + (3, 3, 11)[s - 16]
        if at < len(block.ll_lengths) < at + n:
            crossing.append(s)
        at += n
    return crossing


def test_what_the_cases_are_made_of():
    """The properties the names promise, read back from the streams."""
    by = {c.name: c for c in CASES}

    def toks(name):
        return [t for b in D.inflate(by[name].raw)[0] for t in b.tokens]

    for source in ("stored", "literals"):
        got = {t for t in toks(f"far_window_from_{source}") if not isinstance(t, int)}
        assert got >= {(n, d) for n in (3, 258) for d in (32506, 32507, 32767, 32768)}
        got = {t for t in toks(f"far_ring_from_{source}") if not isinstance(t, int)}
        assert got >= {(n, d) for n in (3, 258) for d in (1726, 1727, 2047, 2048, 2049)}
    for depth in (10, 12, 15):
        (b,) = D.inflate(by[f"deep_{depth}"].raw)[0]
        lu, du = W.used_symbols(b.tokens)
        assert len(b.tokens) >= 20_000 and all(b.ll_lengths[s] == depth for s in lu) and all(b.d_lengths[s] == depth for s in du)
    wide = 0
    for k in range(12):
        b = D.inflate(by[f"wide_tokens_{k}"].raw)[0][-1]
        for t in b.tokens:
            if not isinstance(t, int):
                ls, ds = (284 if t[0] >= 227 else D.length_symbol(t[0])[0]), D.distance_symbol(t[1])[0]
                assert b.ll_lengths[ls] == 15 and D.LEN_EXTRA[ls - 257] == 5 and b.d_lengths[ds] == 15 and D.DIST_EXTRA[ds] == 13
                wide += 1
    assert wide >= 1500
    assert len(by["one_bit_literals"].raw) < 8200 and len(by["one_bit_literals"].data) == W.BLOCK_DATA
    assert len(by["two_bit_matches_d1"].raw) < 100 and len(by["two_bit_matches_d1"].data) == W.BLOCK_DATA
    assert len(D.inflate(by["200_tiny_dynamic_blocks"].raw)[0]) == 200
    for name in ("header_16_across_hlit", "header_17_across_hlit", "header_18_across_hlit"):
        (b,) = D.inflate(by[name].raw)[0]
        assert _crossing(b) == [int(name.split("_")[1])], name
    # header repeats across HLIT under zlib's own tokens (where a block codes distance 1, no run of zeros can span it)
    for name in ("bam_runs", "rows_cuts", "bam_cuts"):
        assert sum(_crossing(b) != [] for b in D.inflate(by[name].raw)[0] if b.btype == "dynamic") >= 2, name
    for k in range(4):  # the end-of-block code ends the payload's last byte
        (b,) = D.inflate(by[f"payload_alignment_{k}"].raw)[0]
        assert b.bits == 8 * len(by[f"payload_alignment_{k}"].raw) and len(by[f"payload_alignment_{k}"].extra) == 4 + k
