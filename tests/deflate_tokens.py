"""A plain inflater of a raw DEFLATE stream, written from RFC 1951, that keeps what a decompressor throws away: per
block its type, the three code-length tables and the code-length symbol sequence of a dynamic header, its size in
bits, and the token list (literals and ``(length, distance)`` pairs).  Tests of a COMPRESSOR read its decisions from
these (``tests/test_gpu_deflate_choices.py``); ``tests/test_deflate_tokens.py`` holds this file against zlib's streams.

It refuses what the RFC refuses: a reserved block type, a stored block whose LEN and NLEN disagree, an over-subscribed
code, an incomplete code (except a distance code of one single 1-bit code, RFC 3.2.7, or of no code at all in a block
without matches), a repeat symbol with nothing in front of it or running past HLIT + HDIST, a missing end-of-block
code, length symbols 286 / 287, distance symbols 30 / 31, a distance that reaches in front of the output, a stream
that ends inside a block."""

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8  # RFC 3.2.6
FIXED_D = [5] * 32


class InflateError(ValueError):
    pass


class Block:
    """One DEFLATE block.  ``btype``: "stored" / "fixed" / "dynamic"; ``bits``: its size from BFINAL to its last bit
    (a stored block's padding included); ``tokens``: ints (literals) and ``(length, distance)`` pairs, the bytes of a
    stored block as literals; ``data``: the bytes the block adds.  Dynamic blocks only: ``cl_lengths`` (19, by symbol),
    ``ll_lengths`` (HLIT + 257), ``d_lengths`` (HDIST + 1), ``cl_symbols`` (the header's ``(symbol, extra value)``
    sequence)."""
    __slots__ = ("btype", "final", "bits", "tokens", "data", "cl_lengths", "ll_lengths", "d_lengths", "cl_symbols")

    def __init__(self):
        self.cl_lengths = self.ll_lengths = self.d_lengths = self.cl_symbols = None


def kraft(lengths):
    """(sum of 2^(max - l) over the coded symbols, 2^max): equal = complete, greater = over-subscribed."""
    top = max(lengths) if len(lengths) else 0
    return sum(1 << (top - l) for l in lengths if l), 1 << top


def _decoder(lengths, what, may_be_single):
    """{(length, code): symbol} of the canonical code (RFC 3.2.2), after the RFC's checks."""
    used = [l for l in lengths if l]
    if not used:
        if may_be_single:
            return {}
        raise InflateError(f"{what} code has no symbol")
    have, full = kraft(lengths)
    if have > full:
        raise InflateError(f"{what} code is over-subscribed")
    if have < full and not (may_be_single and used == [1]):
        raise InflateError(f"{what} code is incomplete")
    count = [0] * 17
    for l in used:
        count[l] += 1
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    table = {}
    for sym, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = sym
            nxt[l] += 1
    return table


class _Bits:
    def __init__(self, raw):
        self.raw, self.pos, self.n = raw, 0, 8 * len(raw)

    def take(self, k):  # k bits, least significant first (RFC 3.1.1)
        if self.pos + k > self.n:
            raise InflateError("the stream ends inside a block")
        v, raw, p = 0, self.raw, self.pos
        for i in range(k):
            v |= ((raw[(p + i) >> 3] >> ((p + i) & 7)) & 1) << i
        self.pos = p + k
        return v

    def symbol(self, table, what):  # Huffman codes arrive most significant bit first
        code, raw, p, n = 0, self.raw, self.pos, self.n
        for l in range(1, 16):
            if p >= n:
                raise InflateError("the stream ends inside a block")
            code = (code << 1) | ((raw[p >> 3] >> (p & 7)) & 1)
            p += 1
            sym = table.get((l, code))
            if sym is not None:
                self.pos = p
                return sym
        raise InflateError(f"no {what} code matches")


def _dynamic_header(bits, blk):
    hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
    if hlit > 286 or hdist > 30:
        raise InflateError("HLIT / HDIST beyond 286 / 30")
    cl = [0] * 19
    for k in range(hclen):
        cl[CL_ORDER[k]] = bits.take(3)
    cl_table = _decoder(cl, "code-length", False)
    lens, seq = [], []
    while len(lens) < hlit + hdist:
        sym = bits.symbol(cl_table, "code-length")
        if sym < 16:
            seq.append((sym, 0))
            lens.append(sym)
            continue
        if sym == 16:
            if not lens:
                raise InflateError("repeat symbol 16 with no length in front of it")
            extra = bits.take(2)
            rep, val = 3 + extra, lens[-1]
        elif sym == 17:
            extra = bits.take(3)
            rep, val = 3 + extra, 0
        else:
            extra = bits.take(7)
            rep, val = 11 + extra, 0
        seq.append((sym, extra))
        lens += [val] * rep
        if len(lens) > hlit + hdist:
            raise InflateError("a repeat runs past HLIT + HDIST")
    blk.cl_lengths, blk.cl_symbols = cl, seq
    blk.ll_lengths, blk.d_lengths = lens[:hlit], lens[hlit:]
    if not blk.ll_lengths[256]:
        raise InflateError("no end-of-block code")
    return _decoder(blk.ll_lengths, "literal/length", False), _decoder(blk.d_lengths, "distance", True)


_FIXED = None


def _fixed_tables():
    global _FIXED
    if _FIXED is None:
        _FIXED = (_decoder(FIXED_LL, "literal/length", False), _decoder(FIXED_D, "distance", False))
    return _FIXED


def inflate(raw, whole=True):
    """``(blocks, bytes consumed)`` of the raw DEFLATE stream at the front of ``raw``; ``whole``: nothing may follow
    the final block but the padding of its last byte."""
    bits, out, blocks = _Bits(raw), bytearray(), []
    while True:
        blk = Block()
        begin, at = bits.pos, len(out)
        blk.final = bool(bits.take(1))
        btype = bits.take(2)
        blk.tokens = []
        if btype == 0:
            blk.btype = "stored"
            bits.pos = (bits.pos + 7) & ~7
            n, nn = bits.take(16), bits.take(16)
            if n != nn ^ 0xFFFF:
                raise InflateError("stored block: LEN and NLEN disagree")
            p = bits.pos >> 3
            if p + n > len(raw):
                raise InflateError("the stream ends inside a block")
            out += raw[p:p + n]
            blk.tokens = list(raw[p:p + n])
            bits.pos += 8 * n
        elif btype == 3:
            raise InflateError("reserved block type 3")
        else:
            blk.btype = "fixed" if btype == 1 else "dynamic"
            ll, dd = _fixed_tables() if btype == 1 else _dynamic_header(bits, blk)
            tokens = blk.tokens
            while True:
                sym = bits.symbol(ll, "literal/length")
                if sym < 256:
                    tokens.append(sym)
                    out.append(sym)
                    continue
                if sym == 256:
                    break
                if sym > 285:
                    raise InflateError(f"length symbol {sym}")
                length = LEN_BASE[sym - 257] + bits.take(LEN_EXTRA[sym - 257])
                if not dd:
                    raise InflateError("a match in a block without distance codes")
                ds = bits.symbol(dd, "distance")
                if ds > 29:
                    raise InflateError(f"distance symbol {ds}")
                dist = DIST_BASE[ds] + bits.take(DIST_EXTRA[ds])
                if dist > len(out):
                    raise InflateError(f"distance {dist} with {len(out)} bytes of output")
                tokens.append((length, dist))
                if dist >= length:
                    out += out[len(out) - dist:len(out) - dist + length]
                else:  # the copy overlaps what it writes
                    piece = bytes(out[len(out) - dist:])
                    out += (piece * (length // dist + 1))[:length]
        blk.bits = bits.pos - begin
        blk.data = bytes(out[at:])
        blocks.append(blk)
        if blk.final:
            break
    used = (bits.pos + 7) >> 3
    if whole and used != len(raw):
        raise InflateError(f"{len(raw) - used} bytes behind the final block")
    return blocks, used


def token_bytes(tokens):
    return sum(1 if isinstance(t, int) else t[0] for t in tokens)


def length_symbol(length):
    """(symbol, extra bits) of a match length 3..258, from the table of RFC 3.2.5."""
    for k in range(28, -1, -1):  # (258 has its own symbol 285, found first; 284 stops at 257)
        if length >= LEN_BASE[k]:
            return 257 + k, LEN_EXTRA[k]
    raise ValueError(length)


def distance_symbol(dist):
    for k in range(29, -1, -1):
        if dist >= DIST_BASE[k]:
            return k, DIST_EXTRA[k]
    raise ValueError(dist)


def fixed_cost_bits(tokens):
    """Bits of ONE block that codes ``tokens`` with the fixed code (RFC 3.2.6): 3 header bits, the tokens, the
    end-of-block code."""
    bits = 3 + FIXED_LL[256]
    for t in tokens:
        if isinstance(t, int):
            bits += FIXED_LL[t]
        else:
            sym, extra = length_symbol(t[0])
            bits += FIXED_LL[sym] + extra
            bits += 5 + distance_symbol(t[1])[1]
    return bits
