"""A DEFLATE writer driven by tokens and code lengths - the counterpart of ``tests/deflate_tokens.py``, whose tables it
uses.  It writes exactly what it is told, legal or not: stored, fixed and dynamic blocks with caller-chosen literal /
length, distance and code-length code lengths, HLIT / HDIST / HCLEN fields and code-length symbol sequence; raw bits;
BGZF members with a chosen extra field and trailer.  No compressor writes most of what comes out of it, which is the
point: ``catalogue()`` and ``fuzz()`` hold the members that the device inflate (csrc/ftk_inflate.hip) is held to in
``tests/test_gpu_inflate_crafted.py``, and ``tests/test_deflate_writer.py`` has zlib judge every one of them first.

Tokens: an int is a literal, ``(length, distance)`` a match, ``(258, distance, 284)`` the same match written as length
symbol 284 with extra value 31 (RFC 1951 gives 258 its own symbol 285; 227 + 31 is legal all the same), and three escapes
for streams a decoder must refuse: ``("lsym", s)`` the bare literal / length code of symbol ``s``, ``("dsym", s)`` the
bare distance code, ``("bits", value, count)`` raw bits.

Classes of a case: "A" legal (zlib accepts, expected bytes known), "B" zlib refuses and so must every decoder, "C" an
incomplete code whose unassigned patterns never occur (zlib refuses; a decoder may also deliver the intended bytes)."""
import random
import struct
import zlib

try:
    from tests.deflate_tokens import (CL_ORDER, DIST_BASE, DIST_EXTRA, FIXED_D, FIXED_LL, LEN_BASE, LEN_EXTRA, distance_symbol,
                                      inflate, length_symbol, token_bytes)
except ImportError:  # (imported from inside tests/)
    from deflate_tokens import (CL_ORDER, DIST_BASE, DIST_EXTRA, FIXED_D, FIXED_LL, LEN_BASE, LEN_EXTRA, distance_symbol, inflate,
                                length_symbol, token_bytes)

BLOCK_DATA = 0xFF00  # bytes of data a BGZF writer puts into one block
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


# ---- codes ---------------------------------------------------------------------------------------------------------
def _rev(v, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (v & 1)
        v >>= 1
    return r


def canonical(lengths):
    """Per symbol ``(code as it goes into the stream - first bit lowest -, length)`` of the canonical code (RFC 3.2.2);
    unused symbols get ``(0, 0)``.  An over-subscribed set is numbered the same way, its codes cut to their length."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if l:
            out.append((_rev(nxt[l] & ((1 << l) - 1), l), l))
            nxt[l] += 1
        else:
            out.append((0, 0))
    return out


def balanced(m):
    """Lengths of a complete code of ``m`` >= 2 leaves, as flat as it can be."""
    k = max(1, (m - 1).bit_length())
    return [k - 1] * ((1 << k) - m) + [k] * (2 * m - (1 << k))


def random_complete(rng, m, depth):
    """Lengths of a random complete code of ``m`` >= 2 leaves whose deepest is ``depth`` bits (or m - 1 when there are too
    few leaves for that, or as many bits as ``m`` leaves need when they are too many), by Kraft splitting: a spine down to the depth, then random leaves split in two."""
    depth = min(max(depth, (m - 1).bit_length()), m - 1, 15)
    leaves = list(range(1, depth + 1)) + [depth]
    open_ = [k for k, l in enumerate(leaves) if l < depth]
    while len(leaves) < m:
        if not open_:
            raise ValueError((m, depth))
        j = rng.randrange(len(open_))
        k = open_[j]
        leaves[k] += 1
        leaves.append(leaves[k])
        if leaves[k] == depth:
            open_[j] = open_[-1]
            open_.pop()
        else:
            open_.append(len(leaves) - 1)
    rng.shuffle(leaves)
    return leaves


def spread(n, symbols, lengths):
    """``n`` code lengths with ``lengths`` on ``symbols`` and 0 elsewhere."""
    out = [0] * n
    for s, l in zip(symbols, lengths):
        out[s] = l
    return out


def random_code(rng, n, used, depth, spare=0):
    """A random complete code of at most ``depth`` bits over the ``used`` symbols of an alphabet of ``n`` and up to
    ``spare`` symbols nothing uses (at least one when a single symbol is used: one code alone is not complete)."""
    used = sorted(set(used))
    free = [s for s in range(n) if s not in set(used)]
    rng.shuffle(free)
    extra = free[:max(spare, 2 - len(used))]
    syms = used + extra
    return spread(n, syms, random_complete(rng, len(syms), depth))


def deep_code(n, used, depth):
    """Every ``used`` symbol exactly ``depth`` bits deep, the code made complete with short codes on symbols nothing uses:
    what is left of the code space, 2^depth - len(used) slots, is one code per set bit.  Where the alphabet has too few
    unused symbols for that (distances: 30 in all), the unused ones form a spine of 1, 2, 3 ... bits and the used ones a
    flat code below it: as deep as the alphabet allows."""
    used = sorted(set(used))
    left = (1 << depth) - len(used)
    assert left >= 0
    free = [s for s in range(n) if s not in set(used)]
    if bin(left).count("1") <= len(free):
        out = spread(n, used, [depth] * len(used))
        for bit in range(depth):
            if (left >> bit) & 1:
                out[free.pop()] = depth - bit  # (from the top of the alphabet: leaves HLIT / HDIST long)
        return out
    flat = balanced(len(used))
    k = min(len(free), 15 - max(flat))
    return spread(n, free[len(free) - k:] + used, list(range(1, k + 1)) + [k + l for l in flat])


def used_symbols(tokens):
    """(literal / length symbols with the end-of-block code, distance symbols) that ``tokens`` need."""
    ll, dd = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            ll.add(t)
        elif isinstance(t[0], int):
            ll.add(284 if len(t) == 3 else length_symbol(t[0])[0])
            dd.add(distance_symbol(t[1])[0])
    return ll, dd


def trim(lengths, least):
    """Without the zeros at the end, down to ``least`` entries (HLIT >= 257, HDIST >= 1)."""
    n = len(lengths)
    while n > least and lengths[n - 1] == 0:
        n -= 1
    return list(lengths[:n])


def plain_sequence(lens):
    return [(l, 0) for l in lens]


def rle_sequence(lens):
    """The code-length symbols of ``lens`` with every repeat taken greedily - over the literal / length and the distance
    lengths as ONE sequence (RFC 3.2.7 allows it; zlib codes the two apart)."""
    seq, i, n = [], 0, len(lens)
    while i < n:
        v, j = lens[i], i
        while j < n and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                seq.append((18, k - 11))
                run -= k
            if run >= 3:
                seq.append((17, run - 3))
                run = 0
            seq += [(0, 0)] * run
        else:
            seq.append((v, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                seq.append((16, k - 3))
                run -= k
            seq += [(v, 0)] * run
        i = j
    return seq


def with_run(lens, start, count, sym):
    """The plain sequence of ``lens`` with ``lens[start:start + count]`` written as ONE repeat symbol ``sym``."""
    if sym == 16:
        assert 3 <= count <= 6 and start > 0 and all(l == lens[start - 1] for l in lens[start:start + count])
        run = (16, count - 3)
    else:
        assert all(l == 0 for l in lens[start:start + count]) and (3 <= count <= 10 if sym == 17 else 11 <= count <= 138)
        run = (sym, count - (3 if sym == 17 else 11))
    return plain_sequence(lens[:start]) + [run] + plain_sequence(lens[start + count:])


def expand(tokens, out):
    """Append to bytearray ``out`` what ``tokens`` (literals and matches only) stand for."""
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            n, d = t[0], t[1]
            if d > len(out):
                raise ValueError(f"distance {d} with {len(out)} bytes")
            if d >= n:
                out += out[len(out) - d:len(out) - d + n]
            else:
                out += (bytes(out[len(out) - d:]) * (n // d + 1))[:n]
    return out


def plain(tokens):
    """Tokens as ``deflate_tokens.inflate`` reports them."""
    return [t if isinstance(t, int) else (t[0], t[1]) for t in tokens]


# ---- the writer ----------------------------------------------------------------------------------------------------
_FIXED_LL_CODES = canonical(FIXED_LL)
_FIXED_D_CODES = canonical(FIXED_D)


class DeflateWriter:
    """Bits go into an integer that is emptied into a bytearray every 64 bits.  ``data``: what the legal tokens written
    so far stand for (``history`` in front of it: bytes a match may reach that are not this stream's); ``blocks``: one
    record per block of what the writer was told, in the shape of ``deflate_tokens.Block``."""

    def __init__(self, history=b""):
        self.out, self.acc, self.n = bytearray(), 0, 0
        self.all = bytearray(history)
        self.skip = len(history)
        self.blocks = []

    @property
    def data(self):
        return bytes(self.all[self.skip:])

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def bits(self, v, k):
        self.acc |= v << self.n
        self.n += k
        if self.n >= 64:
            nb = self.n >> 3
            self.out += (self.acc & ((1 << (8 * nb)) - 1)).to_bytes(nb, "little")
            self.acc >>= 8 * nb
            self.n &= 7

    def align(self):
        self.bits(0, -self.n & 7)

    def getvalue(self):
        return bytes(self.out) + self.acc.to_bytes((self.n + 7) >> 3, "little")

    def stored(self, data, final=False, len_field=None, nlen_field=None):
        self.bits(int(final), 3)
        self.align()
        n = len(data) if len_field is None else len_field
        self.bits(n | ((n ^ 0xFFFF) if nlen_field is None else nlen_field) << 16, 32)
        nb = self.n >> 3  # (byte aligned: the bytes go straight into the array)
        self.out += self.acc.to_bytes(nb, "little") + data
        self.acc, self.n = 0, 0
        self.all += data
        self.blocks.append(dict(btype="stored", final=final, tokens=list(data)))

    def _tokens(self, tokens, llc, dc):
        bits = self.bits
        for t in tokens:
            if isinstance(t, int):
                bits(*llc[t])
            elif t[0] == "lsym":
                bits(*llc[t[1]])
            elif t[0] == "dsym":
                bits(*dc[t[1]])
            elif t[0] == "bits":
                bits(t[1], t[2])
            else:
                n, d = t[0], t[1]
                if len(t) == 3:
                    assert n == 258 and t[2] == 284
                    s, eb, ev = 284, 5, 31
                else:
                    s, eb = length_symbol(n)
                    ev = n - LEN_BASE[s - 257]
                ds, deb = distance_symbol(d)
                c, l = llc[s]
                dcode, dl = dc[ds]
                assert l and dl, ("no code for", t)
                v = c | ev << l
                l += eb
                v |= dcode << l
                l += dl
                bits(v | (d - DIST_BASE[ds]) << l, l + deb)
        expand([t for t in tokens if isinstance(t, int) or isinstance(t[0], int)], self.all)

    def fixed(self, tokens, final=False, eob=True):
        self.bits(int(final) | 2, 3)
        self._tokens(tokens, _FIXED_LL_CODES, _FIXED_D_CODES)
        if eob:
            self.bits(*_FIXED_LL_CODES[256])
        self.blocks.append(dict(btype="fixed", final=final, tokens=plain(tokens)))

    def dynamic(self, tokens, ll, dl, final=False, cl=None, hclen=None, cl_symbols=None, hlit_field=None, hdist_field=None,
                eob=True):
        """``ll`` / ``dl``: the literal / length and distance code lengths, HLIT and HDIST entries of them (the 5-bit
        fields can be forced); ``cl_symbols``: the ``(symbol, extra value)`` sequence that describes them (default:
        ``rle_sequence``); ``cl``: the 19 code-length code lengths by symbol (default: a flat complete code over the
        symbols of the sequence); ``hclen``: how many of them are written (default: up to the last non-zero)."""
        seq = rle_sequence(list(ll) + list(dl)) if cl_symbols is None else cl_symbols
        if cl is None:
            used = sorted({s for s, _ in seq})
            if len(used) < 2:
                used.append(next(s for s in (0, 1, 2) if s not in used))
            cl = spread(19, used, balanced(len(used)))
        if hclen is None:
            hclen = max([4] + [k + 1 for k in range(19) if cl[CL_ORDER[k]]])
        self.bits(int(final) | 4, 3)
        self.bits(len(ll) - 257 if hlit_field is None else hlit_field, 5)
        self.bits(len(dl) - 1 if hdist_field is None else hdist_field, 5)
        self.bits(hclen - 4, 4)
        for k in range(hclen):
            self.bits(cl[CL_ORDER[k]], 3)
        clc = canonical(cl)
        for s, extra in seq:
            assert clc[s][1], ("no code-length code for", s)
            self.bits(*clc[s])
            if s >= 16:
                self.bits(extra, (2, 3, 7)[s - 16])
        llc, dc = canonical(ll), canonical(dl)
        self._tokens(tokens, llc, dc)
        if eob:
            self.bits(*llc[256])
        self.blocks.append(dict(btype="dynamic", final=final, tokens=plain(tokens), ll_lengths=list(ll), d_lengths=list(dl),
                                cl_lengths=list(cl), cl_symbols=list(seq)))


def member(raw, data, extra=b"", crc=None, isize=None):
    """A BGZF block around the DEFLATE stream ``raw``: ``extra`` goes in front of the BC subfield; the trailer is that
    of ``data`` unless ``crc`` / ``isize`` say otherwise."""
    xlen = 6 + len(extra)
    bsize = 12 + xlen + len(raw) + 8
    if bsize > 65536:
        raise ValueError(f"{bsize} bytes do not fit a BGZF block")
    head = struct.pack("<BBBBIBBH", 31, 139, 8, 4, 0, 0, 255, xlen) + extra + struct.pack("<BBHH", 66, 67, 2, bsize - 1)
    return head + raw + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF if crc is None else crc, len(data) if isize is None else isize)


def fits(raw, data, extra=b""):
    return 12 + 6 + len(extra) + len(raw) + 8 <= 65536 and len(data) <= BLOCK_DATA


class Case:
    """``raw``: the DEFLATE stream; ``data``: the expected bytes (A), the intended bytes (C), the bytes the trailer is
    made from (B); ``blocks``: what the writer was told (A); ``raw_refused``: zlib refuses the raw stream itself (else
    it is the gzip trailer, or the missing end, that it refuses); ``tokens_ok``: ``deflate_tokens`` reads it too."""

    def __init__(self, name, cls, w, data=None, extra=b"", crc=None, isize=None, raw_refused=True, tokens_ok=True, raw=None):
        self.name, self.cls = name, cls
        self.raw = w.getvalue() if raw is None else raw
        self.data = w.data if data is None else data
        self.blocks = w.blocks if w is not None else None
        self.extra, self.crc, self.isize = extra, crc, isize
        self.raw_refused, self.tokens_ok = raw_refused, tokens_ok

    def member(self):
        return member(self.raw, self.data, self.extra, self.crc, self.isize)


# ---- data and tokens ---------------------------------------------------------------------------------------------
def noise(rng, n, lo=0, hi=256):
    return bytes(rng.randrange(lo, hi) for _ in range(n)) if hi - lo < 256 else rng.randbytes(n)


def fragment_rows(rng, n_bytes, contig="chr7"):
    """Whole fragment rows (start-sorted: contig, start, end, mapq, strand), a little more than ``n_bytes`` of them."""
    out, pos = [], 1_000_000
    size = 0
    while size < n_bytes:
        pos += rng.randrange(0, 60)
        row = f"{contig}\t{pos}\t{pos + rng.randrange(90, 420)}\t{rng.randrange(0, 61)}\t{'+-'[rng.randrange(2)]}\n"
        out.append(row)
        size += len(row)
    return "".join(out).encode()


def bam_like_records(rng, n_bytes):
    """Records shaped like a BAM's: a 36-byte binary head, a read name, a CIGAR word, packed bases, qualities."""
    out = bytearray()
    pos = 50_000
    k = 0
    while len(out) < n_bytes:
        pos += rng.randrange(0, 40)
        name = f"r{k:07d}:{rng.randrange(1000)}".encode() + b"\0"
        l_seq = 50
        body = struct.pack("<iiBBHHHiiii", 0, pos, len(name), rng.randrange(0, 61), 4681, 1, (99, 147, 83, 163)[k & 3], l_seq, 0,
                           pos + rng.randrange(100, 300), rng.randrange(-400, 400)) + name + struct.pack("<I", l_seq << 4)
        body += rng.randbytes(l_seq // 2) + bytes(rng.randrange(20, 41) for _ in range(l_seq))
        out += struct.pack("<i", len(body)) + body
        k += 1
    return bytes(out[:n_bytes])


def zlib_tokens(data, level=6):
    """zlib's own tokens for ``data``, all blocks in one list (stored blocks come back as literals)."""
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    blocks, _ = inflate(co.compress(data) + co.flush())
    return [t for b in blocks for t in b.tokens]


_FAR = (1, 2, 258, 1726, 1727, 2048, 2049) + tuple(range(32506, 32769, 37)) + (32506, 32507, 32767, 32768)


def random_tokens(rng, have, room, n_tokens, literals, p_match=0.45):
    """At most ``n_tokens`` tokens that add at most ``room`` bytes behind ``have`` bytes of output.  Distances over all
    of 1..min(32 768, bytes so far), weighted to both sides of the limits the device decoder has (its LDS ring, the reach
    of an LDS-to-LDS copy, the DEFLATE window, zlib's own 32 506) and to copies that overlap what they write; lengths
    over 3..258, weighted to the ends and to the 64 bytes of a wavefront."""
    toks, made = [], 0
    while len(toks) < n_tokens and made < room:
        if have + made == 0 or room - made < 3 or rng.random() >= p_match:
            toks.append(literals[rng.randrange(len(literals))])
            made += 1
            continue
        r = rng.random()
        n = (3, 64, 65, 257, 258)[rng.randrange(5)] if r < 0.5 else rng.randrange(3, 259)
        n = min(n, room - made)
        top = min(32768, have + made)
        r = rng.random()
        if r < 0.5:
            d = _FAR[rng.randrange(len(_FAR))]
            if d > top:
                d = rng.randrange(1, top + 1)
        elif r < 0.7:
            d = min(top, rng.randrange(1, max(2, n)))  # overlapping: distance below length
        else:
            d = rng.randrange(1, top + 1)
        toks.append((n, d))
        made += n
    return toks


def shrink_to_fit(build, n):
    """``build(n)`` -> writer; halves ``n`` until the stream fits a BGZF block, so that no member is dropped."""
    while True:
        w = build(n)
        if fits(w.getvalue(), w.data):
            return w
        assert n > 1
        n //= 2


# ---- the catalogue -----------------------------------------------------------------------------------------------
def _dyn(w, tokens, rng, depth=15, final=False, spare=2, cross=False, **kw):
    """One dynamic block with random complete codes over what ``tokens`` use.  ``cross``: where the distance lengths
    begin with a zero, HLIT is made longer than the code needs, so that one 17 / 18 run of the header spans HLIT."""
    lu, du = used_symbols(tokens)
    ll = trim(random_code(rng, 286, lu, depth, spare), 257)
    dl = trim(random_code(rng, 30, du, depth, min(spare, 30 - len(du))), 1) if du else [0]
    if cross and dl[0] == 0 and len(ll) <= 284:
        ll += [0] * rng.randrange(2, min(286 - len(ll), 12) + 1)
    w.dynamic(tokens, ll, dl, final=final, **kw)


def _far_cases(rng):
    cases = []
    base = noise(rng, 32768)
    for source in ("stored", "literals"):
        for name, pre, dists in (("window", 32768, (32506, 32507, 32767, 32768)), ("ring", 2100, (1726, 1727, 2047, 2048, 2049))):
            w = DeflateWriter()
            if source == "stored":
                w.stored(base[:pre])
            else:
                _dyn(w, list(base[:pre]), rng, 11)
            toks = []
            for d in dists:
                for n in (3, 258):
                    toks += [(n, d), rng.randrange(256)] if name == "ring" else [(n, d)]
            # (behind the first match the same distance reaches other bytes: every match is checked, not one)
            _dyn(w, toks, rng, 9, final=True)
            cases.append(Case(f"far_{name}_from_{source}", "A", w))
    return cases


def _header_cases(rng):
    cases = []
    lits = (97, 98, 99)

    def toks(lens, dists, n=300):
        return [lits[rng.randrange(3)] for _ in range(40)] + [
            lits[rng.randrange(3)] if rng.random() < 0.5 else (lens[rng.randrange(len(lens))], dists[rng.randrange(len(dists))])
            for _ in range(n)]

    # a 16 over the last two literal / length lengths and the first three distance lengths
    ll = spread(261, (97, 98, 99, 256, 257, 258, 259, 260), (2, 2, 3, 3, 4, 4, 4, 4))
    dl = [4, 4, 4, 4, 2, 2, 2]
    w = DeflateWriter()
    w.dynamic(toks((3, 4, 5, 6), (1, 2, 3, 4, 5, 7)), ll, dl, final=True, cl_symbols=with_run(ll + dl, 259, 5, 16))
    cases.append(Case("header_16_across_hlit", "A", w))
    # a 17 over the last two literal / length lengths (HLIT longer than the code needs) and the first three distance lengths
    ll = spread(265, (97, 98, 99, 256, 257, 258, 259, 260), (2, 2, 3, 3, 4, 4, 4, 4))
    dl = [0, 0, 0, 2, 2, 2, 2]
    w = DeflateWriter()
    w.dynamic(toks((3, 4, 5, 6), (4, 5, 7, 8)), ll, dl, final=True, cl_symbols=with_run(ll + dl, 263, 5, 17))
    cases.append(Case("header_17_across_hlit", "A", w))
    # an 18 of 14: eight literal / length lengths, six distance lengths
    ll = spread(276, (97, 98, 99, 256, 257, 258, 259, 260), (2, 2, 3, 3, 4, 4, 4, 4))
    dl = [0] * 6 + [2, 2, 2, 2]
    w = DeflateWriter()
    w.dynamic(toks((3, 4, 5, 6), (9, 12, 13, 17, 24, 25, 32), 400), ll, dl, final=True, cl_symbols=with_run(ll + dl, 268, 14, 18))
    cases.append(Case("header_18_across_hlit", "A", w))
    # an 18 of 138 inside the literals
    ll = spread(258, (138, 139, 200, 255, 256, 257), (2, 2, 2, 3, 4, 4))
    w = DeflateWriter()
    seq = [(18, 127)] + rle_sequence(ll[138:] + [1])
    w.dynamic([(138, 139, 200, 255)[rng.randrange(4)] for _ in range(50)] + [(3, 1), (3, 1), 138], ll, [1], final=True, cl_symbols=seq)
    assert seq[0] == (18, 127) and all(l == 0 for l in ll[:138])
    cases.append(Case("header_18_of_138", "A", w))
    # HLIT = 257 with HDIST = 1 (a one-bit distance code nothing can use: there is no length symbol)
    w = DeflateWriter()
    data = list(noise(rng, 700, 48, 58))
    w.dynamic(data, trim(random_code(rng, 257, set(data) | {256}, 7), 257), [1], final=True)
    assert len(w.blocks[0]["ll_lengths"]) == 257
    cases.append(Case("header_hlit257_hdist1", "A", w))
    # HLIT = 286 with HDIST = 30: every symbol of both alphabets coded
    w = DeflateWriter()
    t = random_tokens(rng, 0, 6000, 2500, list(range(256)))
    w.dynamic(t, random_complete(rng, 286, 13), random_complete(rng, 30, 11), final=True)
    cases.append(Case("header_hlit286_hdist30", "A", w))
    # the fewest code-length code lengths that can describe a code at all: 16 17 18 0 8 - lengths of 8 and 0 only, so
    # 256 symbols of 8 bits and no distance code.  (HCLEN = 4 itself - 16 17 18 0 - can only say "no code": class B)
    used = list(range(1, 256)) + [256]
    w = DeflateWriter()
    ll = spread(257, used, [8] * 256)
    w.dynamic(list(noise(rng, 900, 1, 256)), ll, [0], final=True, cl=spread(19, (0, 8), (1, 1)), hclen=5, cl_symbols=plain_sequence(ll + [0]))
    cases.append(Case("header_hclen5", "A", w))
    # the HCLEN field at 4: eight code-length code lengths (16 17 18 0 8 7 9 6)
    w = DeflateWriter()
    data = list(noise(rng, 900, 0, 200))
    ll = spread(260, list(range(200)) + [256, 257, 258, 259], sorted(_lengths_of(rng, 204, (6, 7, 8, 9))))
    w.dynamic(data, ll, [0], final=True, cl=spread(19, (0, 6, 7, 8, 9, 16, 17, 18), [3] * 8), hclen=8)
    cases.append(Case("header_hclen_field4", "A", w))
    # a code-length code with 7-bit lengths - on the symbols the header uses most
    w = DeflateWriter()
    t = random_tokens(rng, 0, 5000, 2000, list(noise(rng, 40)))
    lu, du = used_symbols(t)
    ll, dl = trim(random_code(rng, 286, lu, 12, 3), 257), trim(random_code(rng, 30, du, 9, 2), 1)
    seq = rle_sequence(ll + dl)
    freq = {}
    for s, _ in seq:
        freq[s] = freq.get(s, 0) + 1
    order = sorted(freq, key=lambda s: -freq[s])  # most frequent first: they get the LONG codes
    assert 3 <= len(order) <= 19
    lens = sorted(random_complete(rng, max(len(order), 8), 7), reverse=True)
    syms = order + [s for s in range(19) if s not in freq][:max(0, 8 - len(order))]
    w.dynamic(t, ll, dl, final=True, cl=spread(19, syms, lens), cl_symbols=seq)
    assert max(w.blocks[0]["cl_lengths"]) == 7
    cases.append(Case("header_cl_7_bits", "A", w))
    return cases


def _lengths_of(rng, m, allowed):
    """A complete code of ``m`` leaves whose lengths all lie in ``allowed`` (consecutive), by splitting from the flat code
    of the shortest length."""
    lo, hi = min(allowed), max(allowed)
    leaves = [lo] * (1 << lo)
    assert (1 << lo) <= m <= (1 << hi)
    while len(leaves) < m:
        k = rng.randrange(len(leaves))
        if leaves[k] < hi:
            leaves[k] += 1
            leaves.append(leaves[k])
    return leaves


def _degenerate_cases(rng):
    cases = []
    # one distance code of one bit: every match at distance 1 (HDIST = 1), or at 4 behind three unused symbols
    for name, dl, d in (("d0", [1], 1), ("d3", [0, 0, 0, 1], 4)):
        t = [120, 121, 122, 123]
        for _ in range(600):
            t += [rng.randrange(118, 126)] if rng.random() < 0.5 else [((3, 4, 17, 64, 65, 258)[rng.randrange(6)], d)]
        w = DeflateWriter()
        lu, _ = used_symbols(t)
        w.dynamic(t, trim(random_code(rng, 286, lu, 9, 2), 257), dl, final=True)
        cases.append(Case(f"one_distance_code_{name}", "A", w))
    # no distance code, literals only
    w = DeflateWriter()
    t = list(noise(rng, 3000, 65, 91))
    w.dynamic(t, trim(random_code(rng, 286, set(t) | {256}, 9, 0), 257), [0], final=True)
    cases.append(Case("no_distance_code", "A", w))
    # a literal / length code of the end-of-block code alone: an empty block, then data
    w = DeflateWriter()
    w.dynamic([], [0] * 256 + [1], [0])
    w.fixed(list(b"behind an empty block\n") * 20 + [(40, 22)], final=True)
    cases.append(Case("only_end_of_block", "A", w, tokens_ok=False))
    # two-symbol literal codes: one literal and the end-of-block code, one bit each - several blocks, other literals
    w = DeflateWriter()
    for k in range(12):
        lit = rng.randrange(256)
        w.dynamic([lit] * rng.randrange(1, 300), spread(257, (lit, 256), (1, 1)), [0], final=k == 11)
    cases.append(Case("two_symbol_codes", "A", w))
    return cases


def _depth_cases(rng):
    cases = []
    # literal / length and distance codes of lengths 1, 2, ..., 15, 15
    stairs = list(range(1, 16)) + [15]
    lsyms = rng.sample(range(256), 10) + [256, 257, 264, 270, 281, 285]
    rng.shuffle(lsyms)
    dsyms = rng.sample(range(20), 16)
    ll, dl = trim(spread(286, lsyms, stairs), 257), trim(spread(30, dsyms, stairs), 1)
    lits = [s for s in lsyms if s < 256]
    lens = [3, 10, 23, 24, 26, 131, 150, 162, 258]
    t = list(lits)
    have = len(t)
    while len(t) < 6000 and have < 50_000:
        if rng.random() < 0.6:
            t.append(lits[rng.randrange(len(lits))])
            have += 1
        else:
            ds = dsyms[rng.randrange(16)]
            d = DIST_BASE[ds] + rng.randrange(1 << DIST_EXTRA[ds])
            if d <= have:
                n = lens[rng.randrange(len(lens))]
                t.append((n, d))
                have += n
    w = DeflateWriter()
    w.dynamic(t, ll, dl, final=True)
    cases.append(Case("lengths_1_to_15", "A", w))
    # every used symbol deeper than the roots of the decoder's tables (9 / 8 bits): 10, 12 and 15 bits, 20 000 tokens
    for depth in (10, 12, 15):
        lits = rng.sample(range(256), 48)
        # (15 of the 30 distance symbols, so that the other 15 can take what is left of the code space)
        dsyms = [0, 1, 2, 3, 4, 5, 14, 15, 16, 17, 20, 21, 22, 28, 29]
        t, have = [], 0
        while len(t) < 20_000:
            room = BLOCK_DATA - have - (20_000 - len(t))  # (20 000 tokens must fit: most matches are short)
            if have == 0 or room < 3 or rng.random() < 0.88:
                t.append(lits[rng.randrange(48)])
                have += 1
                continue
            n = min(room, 3 + rng.randrange(6) if rng.random() < 0.93 else (64, 65, 257, 258, rng.randrange(3, 259))[rng.randrange(5)])
            d = have + 1
            while d > have:
                ds = dsyms[rng.randrange(15)]
                d = DIST_BASE[ds] + rng.randrange(1 << DIST_EXTRA[ds])
            t.append((n, d))
            have += n
        lu, du = used_symbols(t)
        w = DeflateWriter()
        w.dynamic(t, trim(deep_code(286, lu, depth), 257), trim(deep_code(30, du, depth), 1), final=True)
        assert len(t) >= 20_000 and fits(w.getvalue(), w.data), (depth, len(t))
        cases.append(Case(f"deep_{depth}", "A", w))
    return cases


def _wide_token_cases(rng):
    """The 48-bit token: a 15-bit length code, 5 extra bits, a 15-bit distance code, 13 extra bits, back to back and,
    with literals of 1 .. 13 and 15 bits between them, at every bit alignment."""
    cases = []
    lit_by_len = rng.sample(range(256), 15)                      # literal k has a code of k + 1 bits in the first block
    first_ll = spread(257, lit_by_len + [256], list(range(1, 16)) + [15])
    ll = spread(285, lit_by_len[:13] + [lit_by_len[14], 256, 283, 284], list(range(1, 14)) + [15, 15, 15, 15])
    dl = list(range(1, 15)) + [0] * 14 + [15, 15]                # distance symbols 28 and 29: 13 extra bits
    total = 0
    for k in range(12):
        w = DeflateWriter()
        w.stored(noise(rng, 32768 - 700 * k))
        w.dynamic(list(lit_by_len), first_ll, [0])
        t = []
        have = len(w.data)
        while have + 258 <= BLOCK_DATA:
            if rng.random() < 0.25:
                t.append((lit_by_len[:13] + [lit_by_len[14]])[rng.randrange(14)])
                have += 1
            else:
                n = 195 + rng.randrange(63) if rng.random() < 0.9 else 258
                d = rng.randrange(16385, min(have, 32768) + 1)
                t.append((n, d, 284) if n == 258 else (n, d))
                have += n
                total += 1
        w.dynamic(t, ll, dl, final=True)
        cases.append(Case(f"wide_tokens_{k}", "A", w))
    assert total >= 1500
    # the same distances behind SHORT length codes (2 bits + 5 extra): 35 bits a token, the distance code found bit by bit
    for k in range(2):
        w = DeflateWriter()
        w.stored(noise(rng, 30_000))
        t = []
        while len(w.data) + token_bytes(t) + 258 <= BLOCK_DATA:
            t.append((195 + rng.randrange(63), rng.randrange(16385, 30_001)) if rng.random() < 0.8 else lit_by_len[rng.randrange(2)])
        w.dynamic(t, spread(285, (283, 284, 256, lit_by_len[0], lit_by_len[1]), (2, 2, 2, 3, 3)), dl, final=True)
        cases.append(Case(f"short_length_wide_distance_{k}", "A", w))
    return cases


def _dense_cases(rng):
    cases = []
    # one-bit literals: a block of BLOCK_DATA bytes in 8 KB of payload
    w = DeflateWriter()
    w.dynamic([0x41] * BLOCK_DATA, spread(257, (0x41, 256), (1, 1)), [0], final=True)
    cases.append(Case("one_bit_literals", "A", w))
    w = DeflateWriter()
    w.dynamic([(0x41, 0x42)[rng.random() < 0.34] for _ in range(BLOCK_DATA)], spread(257, (0x41, 0x42, 256), (1, 2, 2)), [0], final=True)
    cases.append(Case("one_and_two_bit_literals", "A", w))
    # two-bit matches: length symbol 285 and distance symbol 0, one bit each
    n_full, rest = divmod(BLOCK_DATA - 1, 258)
    w = DeflateWriter()
    w.dynamic([0x5A] + [(258, 1)] * n_full + [(rest, 1)], spread(286, (285, 0x5A, length_symbol(rest)[0], 256), (1, 2, 3, 3)), [1], final=True)
    assert len(w.data) == BLOCK_DATA and w.bitpos < 600 + 200
    cases.append(Case("two_bit_matches_d1", "A", w))
    n_full, rest = divmod(BLOCK_DATA - 258, 258)
    w = DeflateWriter()
    w.stored(noise(rng, 258))
    w.dynamic([(258, 258)] * n_full, spread(286, (285, 256), (1, 1)), [0] * 16 + [1], final=True)
    assert len(w.data) == BLOCK_DATA - rest and rest < 258
    cases.append(Case("one_bit_codes_258_258", "A", w))
    # 258 written as symbol 284 with extra value 31, mixed with symbol 285 and with 257 (284 + 30)
    for fixed in (True, False):
        t = list(noise(rng, 300))
        for _ in range(120):
            t += [(258, rng.randrange(1, 300), 284), rng.randrange(256), (258, rng.randrange(1, 300)), (257, rng.randrange(1, 300))][:rng.randrange(1, 5)]
        w = DeflateWriter()
        if fixed:
            w.fixed(t, final=True)
        else:
            _dyn(w, t, rng, 12, final=True)
        cases.append(Case("len258_as_284_" + ("fixed" if fixed else "dynamic"), "A", w))
    return cases


def _block_mix_cases(rng):
    cases = []
    # stored blocks whose headers start at each of the 8 bit offsets: a fixed block of b nine-bit literals ends 2 + b
    # bits into a byte
    w = DeflateWriter()
    seen = set()
    for b in range(8):
        w.fixed([rng.randrange(144, 256) for _ in range(b)])
        seen.add(w.bitpos & 7)
        w.stored(noise(rng, rng.randrange(1, 90)), final=b == 7)
    assert seen == set(range(8))
    cases.append(Case("stored_at_every_bit_offset", "A", w))
    # empty stored blocks in the middle and as the final block
    w = DeflateWriter()
    w.fixed(list(b"in front of an empty stored block "))
    w.stored(b"")
    w.fixed([(30, 34), 33])
    w.stored(b"", final=True)
    cases.append(Case("empty_stored_blocks", "A", w))
    w = DeflateWriter()
    w.stored(noise(rng, BLOCK_DATA), final=True)
    cases.append(Case("stored_full_block", "A", w))
    # a Huffman block copying from a stored one, a stored one in between, a Huffman block copying across it
    w = DeflateWriter()
    w.stored(noise(rng, 3000))
    w.fixed(random_tokens(rng, 3000, 4000, 300, list(range(256)), 0.7))
    _dyn(w, random_tokens(rng, len(w.data), 4000, 300, list(range(256)), 0.7), rng, 10)
    w.stored(noise(rng, 2500))
    _dyn(w, random_tokens(rng, len(w.data), 5000, 400, list(range(256)), 0.7), rng, 15)
    w.fixed(random_tokens(rng, len(w.data), 5000, 400, list(range(256)), 0.7), final=True)
    cases.append(Case("huffman_and_stored_copy_across", "A", w))
    # 200 tiny dynamic blocks
    w = DeflateWriter()
    for k in range(200):
        _dyn(w, random_tokens(rng, len(w.data), 120, rng.randrange(1, 25), list(noise(rng, 6))), rng, rng.randrange(2, 16), final=k == 199)
    cases.append(Case("200_tiny_dynamic_blocks", "A", w))
    return cases


def _alignment_cases(rng):
    """One member behind extra subfields of 0 .. 3 bytes of content: the payload starts at each byte alignment, and its
    end-of-block code ends on the last bit of its last byte (3 + 7 header and end bits, 8-bit literals, six of 9 bits)."""
    t = list(noise(rng, 500, 0, 144)) + [rng.randrange(144, 256) for _ in range(6)] + [(20, 100), (258, 1)]
    w = DeflateWriter()
    w.fixed(t, final=True)
    assert w.bitpos % 8 == 0, w.bitpos
    return [Case(f"payload_alignment_{k}", "A", w, extra=struct.pack("<BBH", 88, 89, k) + bytes([0xEE] * k)) for k in range(4)]


def reencode(tokens, rng, mode):
    """zlib's tokens under codes no compressor chooses.  ``deep10`` / ``deep12`` / ``deep15``: one block, every used
    symbol that deep; ``runs``: blocks of ~3 000 tokens, random codes of up to 15 bits with unused symbols coded, header
    repeats taken across HLIT; ``cuts``: blocks of 1 - 400 tokens of random type - stored, fixed, dynamic."""
    w = DeflateWriter()
    if mode.startswith("deep"):
        lu, du = used_symbols(tokens)
        depth = int(mode[4:])
        w.dynamic(tokens, trim(deep_code(286, lu, depth), 257), trim(deep_code(30, du, depth), 1) if du else [0], final=True)
        return w
    i = 0
    while i < len(tokens):
        n = 3000 if mode == "runs" else rng.randrange(1, 400)
        part, i = tokens[i:i + n], i + n
        final = i >= len(tokens)
        kind = 2 if mode == "runs" else rng.randrange(3)
        if kind == 0:
            w.stored(bytes(expand(part, bytearray(w.all))[len(w.all):]), final=final)
        elif kind == 1:
            w.fixed(part, final=final)
        else:
            _dyn(w, part, rng, rng.randrange(9, 16), final=final, spare=rng.randrange(0, 12), cross=mode == "runs" or rng.random() < 0.5)
    return w


def reencoded_rows(seed=11, n_members=4):
    """``(rows text, [Case])``: ~40 000 bytes of fragment rows per member, zlib's tokens for them re-encoded in the modes
    of ``reencode`` - the members of the file-level test."""
    rng = random.Random(seed)
    text, cases = b"", []
    for k, mode in enumerate(("deep10", "runs", "cuts", "deep15", "deep12")[:n_members]):
        rows = fragment_rows(rng, 40_000)
        w = reencode(zlib_tokens(rows, (6, 9, 1, 6, 6)[k]), rng, mode)
        assert w.data == rows and fits(w.getvalue(), w.data)
        cases.append(Case(f"rows_{mode}", "A", w))
        text += rows
    return text, cases


def _reencoded_cases(rng):
    cases = reencoded_rows()[1]
    for mode in ("deep10", "deep15", "runs", "cuts"):
        data = bam_like_records(rng, 40_000)
        w = reencode(zlib_tokens(data), rng, mode)
        assert w.data == data
        cases.append(Case(f"bam_{mode}", "A", w))
    return cases


def good_neighbour():
    """``(member, data)``: BLOCK_DATA bytes of compressible text by zlib - what stands on both sides of a class B member."""
    data = fragment_rows(random.Random(5), BLOCK_DATA)[:BLOCK_DATA]
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    return member(co.compress(data) + co.flush(), data), data


def _refused_cases(rng):
    """Class B: one member per check of the decoder.  ``data`` is what the trailer is made from."""
    cases = []
    text = list(b"a member that a decoder must refuse, and nothing else: ") * 3
    n_text = len(text)

    def add(name, w, **kw):
        cases.append(Case(name, "B", w, **kw))

    ok_ll = spread(261, (97, 98, 99, 256, 257, 258, 259, 260), (2, 2, 3, 3, 4, 4, 4, 4))
    ok_dl = [2, 2, 2, 2]
    toks = [97, 98, 99, 97, (3, 1), (4, 2), 98, (5, 3), (6, 4)] * 10
    # over-subscribed codes (one symbol too many at a length that was full)
    w = DeflateWriter()
    w.dynamic(toks, spread(261, (97, 98, 99, 100, 256, 257, 258, 259, 260), (2, 2, 3, 3, 3, 4, 4, 4, 4)), ok_dl, final=True)
    add("oversubscribed_literal_code", w)
    w = DeflateWriter()
    w.dynamic(toks, ok_ll, [2, 2, 2, 2, 2], final=True)
    add("oversubscribed_distance_code", w)
    w = DeflateWriter()
    w.dynamic(toks, ok_ll, ok_dl, final=True, cl=spread(19, (0, 2, 3, 4), (1, 1, 2, 2)), cl_symbols=plain_sequence(ok_ll + ok_dl))
    add("oversubscribed_code_length_code", w)
    # symbol 16 with no length in front of it
    w = DeflateWriter()
    w.dynamic(toks, ok_ll, ok_dl, final=True, cl=spread(19, (0, 2, 3, 4, 16), (2, 2, 2, 3, 3)),
              cl_symbols=[(16, 0)] + plain_sequence(ok_ll[3:] + ok_dl))
    add("repeat_16_first", w)
    # a repeat that runs one past HLIT + HDIST
    w = DeflateWriter()
    dl0 = [2, 2, 2, 2, 0, 0, 0]
    w.dynamic(toks, ok_ll, dl0, final=True, cl_symbols=plain_sequence(ok_ll + dl0[:4]) + [(17, 1)])
    add("repeat_past_hlit_hdist", w)
    # no end-of-block code: a complete code without symbol 256 (the block ends with another symbol's code)
    w = DeflateWriter()
    w.dynamic(toks, spread(261, (97, 98, 99, 100, 257, 258, 259, 260), (2, 2, 3, 3, 4, 4, 4, 4)), ok_dl, final=True, eob=False)
    add("no_end_of_block_code", w)
    # HCLEN = 4: only 16 17 18 0 have lengths, which can say nothing but "no code"
    w = DeflateWriter()
    w.dynamic([], [0] * 257, [0], final=True, cl=spread(19, (0, 18), (1, 1)), hclen=4, eob=False)
    add("hclen_4_describes_no_code", w)
    # HLIT = 287 / 288, HDIST = 31 / 32; the longest of each uses the symbols beyond the alphabets (a length symbol 287,
    # a distance symbol 31 in a dynamic block: there is no other way to give them a code)
    for hl, hd in ((287, 4), (288, 4), (261, 31), (261, 32)):
        ll = spread(hl, (97, 98, 99, 256, 257, 258, 259, hl - 1), (2, 2, 3, 3, 4, 4, 4, 4))
        dl = spread(hd, (0, 1, 2, hd - 1), (2, 2, 2, 2))
        t = [97, 98, 99, (3, 1), (4, 2)] * 6 + ([("lsym", hl - 1), ("dsym", 0)] if hl > 286 else [("lsym", 257), ("dsym", hd - 1)])
        w = DeflateWriter()
        w.dynamic(t, ll, dl, final=True)
        add(f"hlit_{hl}" if hl > 286 else f"hdist_{hd}", w)
    # a stored block whose NLEN is not the complement of LEN (LEN itself stays inside the payload)
    w = DeflateWriter()
    w.fixed(text)
    w.stored(b"0123456789", final=True, nlen_field=(10 ^ 0xFFFF) ^ 0x0100)
    add("stored_len_nlen", w)
    # block type 3 behind a good block
    w = DeflateWriter()
    w.fixed(text)
    w.bits(1 | 3 << 1, 3)
    w.bits(0, 13)
    add("block_type_3_second", w)
    # symbols with a code in the fixed code and no meaning: lengths 286 / 287, distances 30 / 31
    for s in (286, 287):
        w = DeflateWriter()
        w.fixed(text + [("lsym", s), ("dsym", 0)], final=True)
        add(f"fixed_length_symbol_{s}", w)
    for s in (30, 31):
        w = DeflateWriter()
        w.fixed(text + [("lsym", 257), ("dsym", s)], final=True)
        add(f"fixed_distance_symbol_{s}", w)
    # the bit pattern a single one-bit distance code leaves unassigned
    w = DeflateWriter()
    w.dynamic([97, 98, 99, (3, 1), (4, 1), ("lsym", 257), ("bits", 1, 1), 97, 98], ok_ll, [1], final=True)
    add("one_distance_code_unassigned_pattern", w)
    # a match in a block without any distance code
    w = DeflateWriter()
    w.dynamic([97, 98, 99, 97, ("lsym", 257), ("bits", 0, 2), 97, 98], ok_ll, [0], final=True)
    add("match_without_distance_code", w)
    # a distance one byte in front of the member's data.  Only that check can refuse it: the match reaches the last byte
    # of the neighbour in front (far enough back that a decoder reads it from the output buffer), and the trailer is that
    # of the bytes such a decoder would deliver
    _, before = good_neighbour()
    pre = noise(rng, 3000)
    w = DeflateWriter(history=before)
    w.stored(pre)
    w.fixed([(40, 3001), 33], final=True)
    assert w.data == pre + before[-1:] + pre[:39] + b"!"
    add("distance_in_front_of_the_data", w)
    # one byte more than ISIZE - by a literal, by a match, by a stored block; one byte less; no final block
    w = DeflateWriter()
    w.fixed(text + [33], final=True)
    add("literal_beyond_isize", w, data=w.data[:-1], raw_refused=False)
    w = DeflateWriter()
    w.fixed(text + [(20, 7)], final=True)
    add("match_beyond_isize", w, data=w.data[:-1], raw_refused=False)
    w = DeflateWriter()
    w.fixed(text)
    w.stored(b"twelve bytes", final=True)
    add("stored_beyond_isize", w, data=w.data[:-1], raw_refused=False)
    w = DeflateWriter()
    w.fixed(text, final=True)
    add("final_block_short_of_isize", w, data=w.data + b"!", raw_refused=False)
    w = DeflateWriter()
    w.fixed(text)
    w.fixed([(n_text, n_text)], final=False)
    add("no_final_block", w, raw_refused=False)
    return cases


def _incomplete_cases(rng):
    """Class C: incomplete codes whose unassigned patterns the stream never uses."""
    cases = []
    toks = [97, 98, 99, 97, (3, 1), (4, 2), 98, (5, 3), (6, 4)] * 40
    ok_ll = spread(261, (97, 98, 99, 256, 257, 258, 259, 260), (2, 2, 3, 3, 4, 4, 4, 4))
    w = DeflateWriter()
    w.dynamic(toks, spread(261, (97, 98, 99, 256, 257, 258, 259, 260), (2, 2, 3, 3, 4, 4, 4, 5)), [2, 2, 2, 2], final=True)
    cases.append(Case("incomplete_literal_code", "C", w))
    w = DeflateWriter()
    w.dynamic(toks, ok_ll, [2, 2, 2, 3], final=True)
    cases.append(Case("incomplete_distance_code", "C", w))
    w = DeflateWriter()
    w.dynamic(toks, ok_ll, [2, 2, 2, 2], final=True, cl=spread(19, (0, 2, 3, 4), (2, 2, 2, 3)), cl_symbols=plain_sequence(ok_ll + [2, 2, 2, 2]))
    cases.append(Case("incomplete_code_length_code", "C", w))
    return cases


_CATALOGUE = None


def catalogue():
    """Every named case, built once from fixed seeds."""
    global _CATALOGUE
    if _CATALOGUE is None:
        rng = random.Random(20)
        cases = []
        for part in (_far_cases, _header_cases, _degenerate_cases, _depth_cases, _wide_token_cases, _dense_cases, _block_mix_cases,
                     _alignment_cases, _reencoded_cases, _refused_cases, _incomplete_cases):
            cases += part(rng)
        assert len({c.name for c in cases}) == len(cases)
        for c in cases:
            assert c.cls != "A" or fits(c.raw, c.data, c.extra), c.name
        _CATALOGUE = cases
    return _CATALOGUE


_FUZZ = None


def fuzz(n=150, seed=77):
    """``n`` class A members of random make-up: 1 - 5 blocks of random type, random complete codes of up to 15 bits,
    tokens from ``random_tokens``; most of a few KB of data, every twelfth up to BLOCK_DATA behind a stored stretch long
    enough for the far distances.  A member that does not fit a BGZF block is built again with half the tokens."""
    global _FUZZ
    if _FUZZ is not None and (n, seed) == _FUZZ[0]:
        return _FUZZ[1]
    rng = random.Random(seed)
    cases = []
    for k in range(n):
        big = k % 12 == 5
        state = rng.getstate()

        def build(n_tokens):
            rng.setstate(state)  # (the same member again, only shorter)
            w = DeflateWriter()
            room = BLOCK_DATA if big else rng.randrange(200, 9000)
            if big:
                w.stored(noise(rng, rng.randrange(30_000, 33_500)))
            literals = list(noise(rng, rng.randrange(1, 80)))
            n_blocks = rng.randrange(1, 6)
            for b in range(n_blocks):
                final = b == n_blocks - 1
                left = room - len(w.data)
                t = random_tokens(rng, len(w.data), left if final else rng.randrange(0, left + 1), n_tokens // n_blocks + 1, literals,
                                  rng.choice((0.1, 0.45, 0.9)))
                kind = rng.randrange(4)
                if kind == 0:
                    w.stored(bytes(expand(t, bytearray(w.all))[len(w.all):]), final=final)
                elif kind == 1:
                    w.fixed(t, final=final)
                else:
                    _dyn(w, t, rng, rng.randrange(2, 16), final=final, spare=rng.randrange(0, 20), cross=rng.random() < 0.5)
            return w

        w = shrink_to_fit(build, rng.randrange(1, 1200) * (3 if big else 1))
        cases.append(Case(f"fuzz_{k}", "A", w))
    _FUZZ = ((n, seed), cases)
    return cases
