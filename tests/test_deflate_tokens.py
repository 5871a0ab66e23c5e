"""CPU: ``tests/deflate_tokens.py`` (the token-level inflater the GPU compressor tests read decisions from) against
zlib's own streams at several levels and strategies, and against hand-built streams that RFC 1951 refuses."""
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_tokens as D  # noqa: E402


def inputs():
    rng = np.random.default_rng(3)
    row = "".join(f"chr7\t{1_000_000 + 37 * k}\t{1_000_167 + 37 * k}\t{(k * 7) % 61}\t{'+-'[k & 1]}\n" for k in range(900)).encode()
    skew = rng.geometric(0.08, 20_000).clip(1, 255).astype(np.uint8).tobytes()
    return {"zeros": bytes(70_000), "rows": row, "skewed": skew, "random": rng.integers(0, 256, 20_000, dtype=np.uint8).tobytes(),
            "one": b"x", "empty": b""}


INPUTS = inputs()
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "huffman_only": zlib.Z_HUFFMAN_ONLY}


@pytest.mark.parametrize("strategy", sorted(STRATEGIES))
@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_inflater_reproduces_zlib_streams(level, strategy):
    for kind, data in INPUTS.items():
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, STRATEGIES[strategy])
        raw = co.compress(data) + co.flush()
        blocks, used = D.inflate(raw)
        assert used == len(raw), (kind, level, strategy)
        assert b"".join(b.data for b in blocks) == data, (kind, level, strategy)
        assert sum(D.token_bytes(b.tokens) for b in blocks) == len(data), (kind, level, strategy)
        assert [b.final for b in blocks] == [False] * (len(blocks) - 1) + [True]
        assert sum(b.bits for b in blocks) <= 8 * len(raw) < sum(b.bits for b in blocks) + 8
        types = {b.btype for b in blocks}
        if level == 0:
            assert types == {"stored"}
        elif strategy == "fixed":
            assert types <= {"fixed", "stored"}
        for b in blocks:
            assert D.token_bytes(b.tokens) == len(b.data)
            if strategy == "huffman_only" or b.btype == "stored":
                assert all(isinstance(t, int) for t in b.tokens)
            if b.btype == "fixed":
                assert b.bits == D.fixed_cost_bits(b.tokens)
            if b.btype == "dynamic":
                assert len(b.cl_lengths) == 19 and 257 <= len(b.ll_lengths) <= 286 and 1 <= len(b.d_lengths) <= 30
                assert max(b.cl_lengths) <= 7 and max(b.ll_lengths) <= 15 and max(b.d_lengths) <= 15
                have, full = D.kraft(b.cl_lengths)
                assert have == full
                # the header's symbol sequence expands to exactly the two tables
                n = sum(1 if s < 16 else (3 + x if s < 18 else 11 + x) for s, x in b.cl_symbols)
                assert n == len(b.ll_lengths) + len(b.d_lengths)


def test_length_and_distance_symbols_are_the_rfc_tables():
    assert [D.length_symbol(n) for n in (3, 10, 11, 12, 13, 257, 258)] == [(257, 0), (264, 0), (265, 1), (265, 1), (266, 1), (284, 5), (285, 0)]
    assert [D.distance_symbol(n) for n in (1, 4, 5, 6, 7, 24577, 32768)] == [(0, 0), (3, 0), (4, 1), (4, 1), (5, 1), (29, 13), (29, 13)]
    for n in range(3, 259):
        sym, extra = D.length_symbol(n)
        assert 0 <= n - D.LEN_BASE[sym - 257] < (1 << extra) or (n == 258 and sym == 285)
    for n in range(1, 32769):
        sym, extra = D.distance_symbol(n)
        assert 0 <= n - D.DIST_BASE[sym] < (1 << extra) or extra == 0 and n == D.DIST_BASE[sym]


# ---- streams the RFC refuses -----------------------------------------------------------------------------------------
class Put:
    def __init__(self):
        self.bits = []

    def int(self, v, n):  # least significant bit first
        self.bits += [(v >> k) & 1 for k in range(n)]
        return self

    def code(self, v, n):  # a Huffman code: most significant bit first
        self.bits += [(v >> k) & 1 for k in range(n - 1, -1, -1)]
        return self

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[8 * i + k] << k for k in range(8)) for i in range(len(b) // 8))


def dynamic_head(cl):
    """BFINAL, BTYPE = 2, HLIT = 257, HDIST = 1, all 19 code-length code lengths (``cl``: by symbol)."""
    p = Put().int(1, 1).int(2, 2).int(0, 5).int(0, 5).int(15, 4)
    for s in D.CL_ORDER:
        p.int(cl.get(s, 0), 3)
    return p


def test_refuses_what_the_rfc_refuses():
    bad = {}
    bad["reserved"] = Put().int(1, 1).int(3, 2).bytes()
    bad["stored"] = Put().int(1, 1).int(0, 2).int(0, 5).int(3, 16).int(3, 16).bytes() + b"abc"
    bad["over-subscribed"] = dynamic_head({0: 1, 1: 1, 2: 1}).bytes() + bytes(40)
    bad["incomplete"] = dynamic_head({0: 1, 1: 2}).bytes() + bytes(40)
    # fixed code: literal 'a' (0x30 + 97, 8 bits), then length 3 (symbol 257: 0000001) at distance 2 (symbol 1)
    bad["distance"] = Put().int(1, 1).int(1, 2).code(0x30 + 97, 8).code(1, 7).code(1, 5).code(0, 7).bytes()
    bad["inside"] = Put().int(1, 1).int(1, 2).code(0x30 + 97, 8).bytes()
    bad["length symbol"] = Put().int(1, 1).int(1, 2).code(0xC0 + 6, 8).bytes() + bytes(4)  # symbol 286
    bad["distance symbol"] = Put().int(1, 1).int(1, 2).code(0x30 + 97, 8).code(1, 7).code(30, 5).code(0, 7).bytes()
    # code-length code {1: 1 bit, 18: 1 bit}: 257 lengths of zero and none for 256 -> no end-of-block code;
    # a repeat of 138 + 138 zeros runs past 258
    bad["end-of-block"] = dynamic_head({0: 1, 18: 1}).code(1, 1).int(127, 7).code(1, 1).int(109, 7).bytes() + bytes(4)
    bad["past"] = dynamic_head({0: 1, 18: 1}).code(1, 1).int(127, 7).code(1, 1).int(127, 7).bytes() + bytes(4)
    bad["in front of it"] = dynamic_head({0: 1, 16: 1}).code(1, 1).int(0, 2).bytes() + bytes(4)
    for what, raw in bad.items():
        with pytest.raises(D.InflateError, match=what):
            D.inflate(raw)
        with pytest.raises(zlib.error):  # (zlib agrees that each of them is no stream)
            zlib.decompress(raw, -15)
    with pytest.raises(D.InflateError, match="behind"):
        D.inflate(zlib.compress(b"abc")[2:])  # (the zlib wrapper's check value follows the final block)
    assert D.inflate(zlib.compress(b"abc")[2:], whole=False)[1] == len(zlib.compress(b"abc")) - 6


def test_accepts_the_one_distance_code_case():
    # RFC 3.2.7: "If only one distance code is used, it is encoded using one bit, not zero bits".  'a' = 1 bit, 256 and
    # 257 (length 3) = 2 bits each, and ONE distance code of 1 bit (distance 1), whose other half stays unused: "aaaa"
    p = Put().int(1, 1).int(2, 2).int(1, 5).int(0, 5).int(15, 4)  # HLIT = 258
    cl = {0: 1, 1: 2, 2: 3, 18: 3}
    for s in D.CL_ORDER:
        p.int(cl.get(s, 0), 3)
    # canonical code-length code: 0 -> 0, 1 -> 10, 2 -> 110, 18 -> 111
    p.code(7, 3).int(97 - 11, 7)  # 97 zeros
    p.code(2, 2)  # 'a': 1 bit
    p.code(7, 3).int(138 - 11, 7).code(7, 3).int(20 - 11, 7)  # 158 zeros: symbols 98..255
    p.code(6, 3).code(6, 3)  # 256, 257: 2 bits
    p.code(2, 2)  # the distance code: 1 bit, alone
    # literal/length code: 'a' -> 0, 256 -> 10, 257 -> 11; distance 0 -> 0
    p.code(0, 1).code(3, 2).code(0, 1).code(2, 2)
    raw = p.bytes()
    assert zlib.decompress(raw, -15) == b"aaaa"
    (blk,), used = D.inflate(raw)
    assert blk.btype == "dynamic" and blk.data == b"aaaa" and blk.tokens == [97, (3, 1)] and used == len(raw)
    assert blk.d_lengths == [1] and blk.cl_symbols[0] == (18, 86)
