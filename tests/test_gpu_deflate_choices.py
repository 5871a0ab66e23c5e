"""GPU: what the device DEFLATE compressor (``csrc/ftk_fragtext.hip``, part (c)) DECIDED, read back from its streams
with the token-level inflater of ``tests/deflate_tokens.py`` - a round trip alone cannot see a compressor that stops
finding matches at some distance, always takes the fixed code or splits its blocks at the wrong token count.

Every case runs the round trip per member (zlib's inflate, CRC, ISIZE, BSIZE, the data + 31 bound, determinism); at
most two members per case are decoded to tokens and held against DESIGN.md 3.10 and RFC 1951: matches of 4..258 bytes
at 1..32768, blocks of at most 8192 tokens (non-final ones exactly 8192), complete codes within 7 / 15 / 15 bits, a
dynamic block strictly smaller than the fixed-code cost of its tokens, a stored member only at data + 5 bytes.  No
number here is a tolerance: equalities, bounds from the format, and coverage conditions checked on the decoded stream.

``test_more_blocks_than_lanes`` is the one large case (8195 blocks, 535 MB of text: three lanes compress a second
block); its wall time on an MI355X is recorded in ``profiles/export_test_mutations.txt``."""
import os
import sys
import time
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_tokens as D  # noqa: E402
from helpers import first_difference  # noqa: E402
from test_gpu_frag_export import EOF, split_members  # noqa: E402

pytestmark = pytest.mark.gpu
B = 0xFF00
MAX_TOKENS = 8192  # "per DEFLATE block of at most 8192 tokens"


def row_text(n, seed=0):
    """``n`` bytes of fragment rows (deterministic; cut inside the last row)."""
    rng = np.random.default_rng(seed)
    k = n // 24 + 2
    s = 1_000_000 + np.cumsum(rng.integers(0, 40, k))
    ln, q, st = rng.integers(100, 220, k), rng.integers(0, 61, k), rng.integers(0, 2, k)
    return "".join(f"chr1\t{a}\t{a + b}\t{c}\t{'-+'[d]}\n" for a, b, c, d in zip(s, ln, q, st)).encode()[:n]


def de_bruijn(k, n):
    """The de Bruijn sequence B(k, n) (Lyndon words, the textbook recursion): every n-gram over k symbols once."""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq


def no_repeat_text(n):
    """``n`` <= 10000 bytes over ten symbols in which no four bytes occur twice: no LZ77 match of length >= 4 exists."""
    text = bytes(ord("0") + d for d in de_bruijn(10, 4)[:n])
    grams = {text[i:i + 4] for i in range(len(text) - 3)}
    assert len(text) == n and len(grams) == max(n - 3, 0)
    return text


def deflate_checked(engine, text, deterministic=True):
    """The existing round trip: ``(members, image, offs)`` of ``text``."""
    n = len(text)
    image, offs = engine.bgzf_deflate(text)
    if deterministic:
        assert first_difference(engine.bgzf_deflate(text)[0], image) is None
    assert image[-28:] == EOF
    members = split_members(image[:-28])
    assert len(members) == -(-n // B) and len(offs) == len(members) + 1
    pos = 0
    for k, (payload, crc, isize, bsize) in enumerate(members):
        piece = text[k * B:(k + 1) * B]
        assert offs[k] == pos, k
        assert first_difference(zlib.decompress(payload, -15), piece) is None, k
        assert crc == zlib.crc32(piece) and isize == len(piece), k
        # 18 bytes of header, 8 of trailer; a stored block (5 + data) is the most a payload may take
        assert bsize == len(payload) + 26 and len(payload) <= len(piece) + 5, k
        pos += bsize
    assert offs[-1] == pos
    assert len(image) <= n + 31 * len(members) + 28
    return members, image, offs


def decode_member(payload, piece):
    """The member's blocks, after the properties every member has."""
    blocks, used = D.inflate(payload)
    n = len(piece)
    assert used == len(payload) and first_difference(b"".join(b.data for b in blocks), piece) is None
    assert [b.final for b in blocks] == [False] * (len(blocks) - 1) + [True]
    if any(b.btype == "stored" for b in blocks):
        assert len(blocks) == 1 and len(payload) == n + 5  # exactly one stored block, LEN = the whole member
        return blocks
    for b in blocks:
        assert len(b.tokens) == MAX_TOKENS if not b.final else 0 <= len(b.tokens) <= MAX_TOKENS
        for t in b.tokens:
            if not isinstance(t, int):
                assert 4 <= t[0] <= 258 and 1 <= t[1] <= 32768, t
        if b.btype == "dynamic":
            for lens, limit in ((b.cl_lengths, 7), (b.ll_lengths, 15), (b.d_lengths, 15)):
                have, full = D.kraft(lens)
                assert have == full and max(lens) <= limit, (lens, limit)
            assert b.ll_lengths[256] > 0
            assert b.bits < D.fixed_cost_bits(b.tokens)
        else:
            assert b.bits == D.fixed_cost_bits(b.tokens)
    return blocks


def tokens_of(engine, text):
    """Token list of a text of one member that is not stored, with each token's position."""
    assert 0 < len(text) <= B
    members, _, _ = deflate_checked(engine, text)
    blocks = decode_member(members[0][0], text)
    assert blocks[0].btype != "stored"
    out, pos = [], 0
    for b in blocks:
        for t in b.tokens:
            out.append((pos, t))
            pos += 1 if isinstance(t, int) else t[0]
    return out, blocks


# ---- matches: how far, how long --------------------------------------------------------------------------------------
# R: 8 distinct non-zero bytes.  Whether the single-candidate hash table still holds R's entry when its second copy
# arrives depends on the hash function (no four bytes of R, of its borders with the zeros or of the zeros may land in
# the slot of R's first four bytes), not on the format: this seed works for the committed hash; another hash may need
# another seed - the assertions below say so when it does.
R = bytes(np.random.default_rng(7).permutation(np.arange(1, 256))[:8].astype(np.uint8))


@pytest.mark.parametrize("dist", [9, 32767, 32768, 32769, 40000])
def test_match_window_reaches_32768_and_no_further(engine, dist):
    assert len(set(R)) == 8 and 0 not in R
    text = R + bytes(dist - 8) + R
    toks, _ = tokens_of(engine, text)
    second = [(p, t) for p, t in toks if p + (1 if isinstance(t, int) else t[0]) > dist]  # tokens that reach into the second R
    if dist <= 32768:
        assert (dist, (8, dist)) in toks, second
    else:
        # no reference into the first R: every match copies from the zeros (or from the second R itself)
        for p, t in toks:
            assert isinstance(t, int) or p - t[1] >= 8, (p, t)
        assert [t for p, t in toks if p >= dist] == list(R), second


MATCH_LENGTHS = (4, 5, 10, 11, 18, 19, 34, 35, 66, 67, 130, 131, 257, 258, 259)


def test_match_lengths_at_the_length_symbols_edges(engine):
    """Runs of one byte, each of its own byte value, between stretches of bytes that occur once in the whole text: a run
    of L + 1 bytes is a literal and one match of length L at distance 1 (259: 258 and one more literal).  The lengths
    are the first and last of the extra-bit groups of RFC 3.2.5 (10 | 11, 18 | 19, ...), 257 | 258 and the cap."""
    once = np.random.default_rng(2).permutation(np.arange(0, 200)).astype(np.uint8)
    text, want = b"", []
    for k, ln in enumerate(MATCH_LENGTHS):
        text += bytes(once[12 * k:12 * k + 12])
        want += [(len(text) + 1, (min(ln, 258), 1))] + ([(len(text) + 259, 200 + k)] if ln > 258 else [])
        text += bytes([200 + k]) * (ln + 1)
    text += bytes(once[180:192])
    toks, _ = tokens_of(engine, text)
    assert [(p, t) for p, t in toks if not isinstance(t, int) or (p, t) in want] == want
    assert sorted({D.length_symbol(t[0])[0] for _, t in toks if not isinstance(t, int)}) == [258, 259, 264, 265, 268, 269, 272, 273, 276, 277,
                                                                                          280, 281, 284, 285]


def test_tails_and_tiny_inputs(engine):
    u = bytes(np.random.default_rng(4).permutation(np.arange(1, 200))[:43].astype(np.uint8))
    head, tail = u[:40], u[40:]
    for k in (0, 1, 2, 3):  # the match runs to the final byte / the text ends 1, 2, 3 bytes behind it
        toks, blocks = tokens_of(engine, head + head + tail[:k])
        assert [t for _, t in toks] == list(head) + [(40, 40)] + list(tail[:k]), k
    for n in (1, 2, 3, 4, 5):
        toks, blocks = tokens_of(engine, b"abcde"[:n])
        assert [t for _, t in toks] == list(b"abcde"[:n]) and blocks[0].btype == "fixed"
        toks, blocks = tokens_of(engine, b"a" * n)
        # four bytes are the shortest match and it needs a byte in front of it: the first match is at n = 5
        assert [t for _, t in toks] == ([97] * n if n < 5 else [97, (4, 1)])
    for n in (6, 7, 8, 9, 262, 263):  # 258 + the tail of 0..3 bytes behind it, in one run
        toks, _ = tokens_of(engine, b"a" * n)
        rest = n - 1 - min(n - 1, 258)
        assert [t for _, t in toks] == [97, (min(n - 1, 258), 1)] + ([97] * rest if rest < 4 else [(rest, 1)]), n


# ---- blocks: where they split, which code they take -------------------------------------------------------------------
def test_block_split_at_8192_tokens(engine):
    for n, want in ((MAX_TOKENS - 1, [MAX_TOKENS - 1]), (MAX_TOKENS, [MAX_TOKENS]), (MAX_TOKENS + 1, [MAX_TOKENS, 1])):
        text = no_repeat_text(n)
        toks, blocks = tokens_of(engine, text)
        assert all(isinstance(t, int) for _, t in toks)  # (no match: a token per byte)
        assert [len(b.tokens) for b in blocks] == want, n
    # and with a match as the last token of the first block: 8190 literals, a run's first byte, its first match
    text = no_repeat_text(MAX_TOKENS - 2) + b"z" * 300 + b"ABCDEFG"
    toks, blocks = tokens_of(engine, text)
    assert [len(b.tokens) for b in blocks] == [MAX_TOKENS, 8]
    assert blocks[0].tokens[-2:] == [ord("z"), (258, 1)] and blocks[1].tokens == [(41, 1)] + list(b"ABCDEFG")


def test_fixed_for_a_short_text_dynamic_for_rows(engine):
    toks, blocks = tokens_of(engine, row_text(40))
    assert [b.btype for b in blocks] == ["fixed"]  # (a dynamic header alone is 17 bits + 3 per code-length code + the lengths)
    text = row_text(B, seed=1)
    members, _, _ = deflate_checked(engine, text)
    blocks = decode_member(members[0][0], text)
    assert len(blocks) > 1 and {b.btype for b in blocks} == {"dynamic"}


def test_distance_codes_none_and_one(engine):
    text = no_repeat_text(5000)  # no match: no distance code is used
    toks, blocks = tokens_of(engine, text)
    assert [b.btype for b in blocks] == ["dynamic"] and all(isinstance(t, int) for _, t in toks)
    text = b"ab" * 30000  # every match at distance 2: one distance code is used
    toks, blocks = tokens_of(engine, text)
    assert [b.btype for b in blocks] == ["dynamic"]
    assert {t[1] for _, t in toks if not isinstance(t, int)} == {2} and sum(1 for _, t in toks if isinstance(t, int)) == 2
    assert sum(1 for l in blocks[0].d_lengths if l) <= 2


def geometric_block(n, ratio, symbols, seed):
    """``n`` bytes over ``symbols`` byte values whose frequencies fall geometrically by ``ratio``, shuffled."""
    w = ratio ** np.arange(symbols, dtype=np.float64)
    counts = np.maximum((w / w.sum() * n).astype(np.int64), 1)
    counts[0] += n - counts.sum()
    vals = np.random.default_rng(seed).permutation(256)[:symbols].astype(np.uint8)
    data = np.repeat(vals, counts)
    np.random.default_rng(seed + 1).shuffle(data)
    return data.tobytes()


def class_block(lengths, counts, seed, permute):
    """``counts[j]`` byte values that occur 2^(13 - ``lengths[j]``) times each - frequencies falling by powers of two, in
    classes of very unequal size - shuffled; at most 8191 bytes, so one DEFLATE block whose literal code has about
    ``counts[j]`` codes of ``lengths[j]`` bits."""
    rng = np.random.default_rng(seed)
    k = sum(counts)
    vals = rng.permutation(256)[:k] if permute else np.arange(k)
    freq = np.concatenate([np.full(c, 1 << (13 - ln)) for c, ln in zip(counts, lengths)])
    data = np.repeat(vals.astype(np.uint8), freq)
    rng.shuffle(data)
    assert len(data) <= 8191
    return data.tobytes()


# (lengths, counts, seed, permute) - two texts, so two decoded members.  How to find such cases again (after a change of
# ``code_lengths``, say): draw 5..8 distinct lengths from 4..12 and for each a count from {1, 2, 3, 4, 8, 16, 32, 64,
# 128}; keep the draw if the counts sum to 200..254 and the text (sum of count * 2^(13 - length)) holds 6000..8191
# bytes; draw a seed and whether the byte values are permuted; compress ``class_block`` of it and keep the case if the
# decoded header satisfies the two assertions of the test below.  About one draw in a few thousand does: its header
# holds code-length symbols in counts like 128 : 64 : 16 : 8 : 2 : 1 : 1 : 1 of 256 - Shannon lengths that fill the code
# space exactly BEFORE the rare ones are cut from 8 bits to 7.  ``tools/deflate_clamp_search.py`` runs this search.
CLAMP_CASES = (((8, 5, 6, 11, 12), (128, 3, 8, 16, 64), 814063, True),
               ((8, 11, 4, 12, 5, 7, 9, 10), (2, 16, 2, 128, 1, 64, 32, 2), 746454, False))


def test_code_length_code_is_clamped_to_7_bits(engine):
    """Literal codes of many different lengths, in classes of very unequal size, make a header whose code-length
    symbols have very unequal counts; a symbol that occurs c times among T with T / c > 128 has a Shannon length above
    7, the most the 3-bit fields of RFC 3.2.7 can say: the compressor had to cut it.  Where the cut lengths
    over-subscribe the code (their Kraft sum, computed here, exceeds 1) it also had to lengthen others, and the
    general checks of ``decode_member`` hold the result to a complete code that zlib accepts.  Both conditions are
    asserted on the decoded header, so the case cannot stop reaching that path unnoticed."""
    reached = []
    for lengths, counts, seed, permute in CLAMP_CASES:
        text = class_block(lengths, counts, seed, permute)
        assert len(set(text)) >= 200
        members, _, _ = deflate_checked(engine, text)
        (b,) = decode_member(members[0][0], text)
        assert b.btype == "dynamic"
        syms = [s for s, _ in b.cl_symbols]
        total = len(syms)
        count = {s: syms.count(s) for s in set(syms)}
        rare = [s for s, c in count.items() if total > 128 * c]
        assert rare and all(0 < b.cl_lengths[s] <= 7 for s in rare), (count, b.cl_lengths)
        # Shannon lengths ceil(log2(T / c)), cut at 7, in units of 2^-7: above 128 the code was over-subscribed
        fill = sum(1 << (7 - min(7, next(l for l in range(1, 16) if (c << l) >= total))) for c in count.values())
        reached.append((total, sorted(count.items()), fill))
        assert fill > 128, reached
    print("code-length symbol counts and the cut Shannon lengths' fill / 128:", reached)


def test_members_pass_from_compressed_to_stored(engine):
    rng = np.random.default_rng(9)
    zeros = (B, 8192, 2048, 1024, 768, 512, 384, 256, 192, 128, 64, 32, 0)
    text = b"".join(bytes(z) + rng.integers(0, 256, B - z, dtype=np.uint8).tobytes() for z in zeros)
    members, _, _ = deflate_checked(engine, text)
    stored = []
    for k, (payload, _, isize, _) in enumerate(members):
        first = payload[0] & 7  # BFINAL | BTYPE << 1 of the first block
        is_stored = (first >> 1) == 0
        assert is_stored or len(payload) <= isize + 5
        if is_stored:  # one stored block: final, LEN = ISIZE, NLEN, the data
            assert first == 1 and len(payload) == isize + 5 and payload[1:5] == bytes([isize & 255, isize >> 8, ~isize & 255, (~isize >> 8) & 255])
        stored.append(is_stored)
    assert stored[0] is False and stored[-1] is True, stored  # both occur: all zeros compress, random bytes do not
    last = stored.index(True) - 1  # the last compressed member and the first stored one, token by token
    for k in (last, last + 1):
        blocks = decode_member(members[k][0], text[k * B:(k + 1) * B])
        assert (blocks[0].btype == "stored") == stored[k]


# ---- the member table --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seven_blocks():
    rng = np.random.default_rng(12)
    kinds = [bytes(B), row_text(B, 2), rng.integers(0, 256, B, dtype=np.uint8).tobytes(), row_text(B, 3), bytes(B),
             geometric_block(B, 0.9, 100, 5), rng.integers(0, 256, B, dtype=np.uint8).tobytes()]
    return np.frombuffer(b"".join(kinds), np.uint8)


@pytest.mark.parametrize("n_blocks", [1023, 1024, 1025, 2049])
def test_member_offsets_beyond_one_scan_pass(engine, seven_blocks, n_blocks):
    """``offs`` against the BSIZE fields of the image, with member sizes that differ from neighbour to neighbour (zeros /
    rows / random by k % 7), on both sides of the 1024 entries one pass of the size scan takes; the last member is short."""
    n = (n_blocks - 1) * B + 77
    text = np.resize(seven_blocks, n).tobytes()
    members, image, offs = deflate_checked(engine, text, deterministic=n_blocks == 1025)
    assert len(members) == n_blocks
    sizes = np.array([m[3] for m in members], np.int64)
    assert np.array_equal(offs, np.concatenate(([0], np.cumsum(sizes))))  # (deflate_checked's walk, said at once)
    assert all(sizes[k] != sizes[k + 1] for k in range(6)) and len(set(sizes[:7].tolist())) >= 4
    # the image depends on the text alone: equal blocks give equal members wherever they are
    assert [k for k in range(7, n_blocks - 1) if members[k][0] != members[k % 7][0]] == []


@pytest.mark.parametrize("kinds", [1, 3])
def test_more_blocks_than_lanes(engine, kinds):
    """8195 blocks of row text: 8192 lanes compress side by side and three of them take a second block, with the hash
    table their first block left behind.  DESIGN.md 3.10: the image depends on the text alone - equal blocks give equal
    members.  ``kinds`` = 1: all blocks equal (what a lane's stale entries point at are then the same bytes);
    ``kinds`` = 3: three texts in turn, so blocks 8192, 8193, 8194 follow a DIFFERENT text on their lanes (0, 1, 2)."""
    n_blocks = 8195
    blocks = [row_text(B, seed=6 + k) for k in range(kinds)]
    text = b"".join(blocks) * (n_blocks // kinds) + b"".join(blocks)[:B * (n_blocks % kinds)]
    assert len(text) == n_blocks * B
    t0 = time.perf_counter()
    image, offs = engine.bgzf_deflate(text, write_eof=False)
    dt = time.perf_counter() - t0
    print(f"8195 blocks of {kinds} kind(s) ({len(text) / 1e6:.0f} MB of text): bgzf_deflate took {dt:.2f} s")
    del text
    assert len(offs) == n_blocks + 1 and offs[0] == 0 and offs[-1] == len(image)
    # members of one kind are equal, so the image repeats with the period of the first ``kinds`` members: one reshape
    # and compare for the whole cycles, one compare for the members behind them
    period, cycles = int(offs[kinds]), n_blocks // kinds
    raw = np.frombuffer(image, np.uint8)
    assert np.array_equal(offs[::kinds][:cycles + 1], np.arange(cycles + 1, dtype=np.int64) * period)
    table = raw[:cycles * period].reshape(cycles, period)
    differs = (table != table[0]).any(axis=1)
    assert not differs.any(), np.nonzero(differs)[0][:8] * kinds
    rest = raw[cycles * period:]
    assert np.array_equal(offs[cycles * kinds:] - cycles * period, offs[:n_blocks % kinds + 1]) and np.array_equal(rest, raw[:len(rest)])
    for k, (payload, crc, isize, bsize) in enumerate(split_members(image[:period])):
        assert bsize == offs[k + 1] - offs[k] and first_difference(zlib.decompress(payload, -15), blocks[k]) is None
        assert crc == zlib.crc32(blocks[k]) and isize == B
    decode_member(payload, blocks[-1])
