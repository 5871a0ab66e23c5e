"""GPU: the device inflate (csrc/ftk_inflate.hip) on DEFLATE that no compressor of the suite writes - the members of
``tests/deflate_writer.py`` (``tests/test_deflate_writer.py`` has zlib judge every one of them on the CPU): distances up
to 32 768, header repeats across HLIT, one or no distance code, codes deeper than the tables' roots on frequent symbols,
48-bit tokens, one-bit literals, two-bit matches, 258 as 284 + 31, stored blocks anywhere, every payload alignment,
zlib's tokens under adversarial codes, a token-level fuzz; one refusal per check of the kernel; incomplete codes.  Every
image goes through all three symbol loops (``_inflate_each`` of ``tests/test_gpu_inflate.py``)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from finaletoolkit_amd import _lib as L
from tests import deflate_writer as W
from tests.helpers import ROOT
from tests.test_gpu_inflate import _inflate, _inflate_each

pytestmark = pytest.mark.gpu

LOOPS = ("serial windows", "vector matches", "lane-parallel")
CASES = W.catalogue()
CLASS_A = [c for c in CASES if c.cls == "A"]
PER_IMAGE = 30


def _hold_members(engine, cases):
    """All three loops: FTK_OK and the expected bytes, member by member (the first that differs is named)."""
    image = b"".join(c.member() for c in cases) + W.EOF_MEMBER
    results = _inflate_each(engine, image)
    for loop, (rc, got, message) in zip(LOOPS, results):
        if rc != L.FTK_OK:
            m = re.search(rb"block (\d+)", message or b"")
            where = cases[int(m.group(1))].name if m and int(m.group(1)) < len(cases) else "?"
            raise AssertionError(f"{loop}: rc {rc} at member {where}: {message}")
        off = 0
        for c in cases:
            assert got[off:off + len(c.data)] == c.data, f"{loop}: member {c.name} ({len(c.data)} bytes) differs"
            off += len(c.data)
        assert off == len(got), loop


@pytest.mark.parametrize("part", range((len(CLASS_A) + PER_IMAGE - 1) // PER_IMAGE))
def test_class_a_catalogue(engine, part):
    """Legal streams that zlib accepts: byte-equal in every loop.  The catalogue, ``PER_IMAGE`` members to an image."""
    _hold_members(engine, CLASS_A[part * PER_IMAGE:(part + 1) * PER_IMAGE])


@pytest.mark.parametrize("case", CLASS_A, ids=lambda c: c.name)
def test_class_a_member_alone(engine, case):
    """Every catalogue member as the only block of its image (block 0, output offset 0: another alignment of its
    payload and of its output than in the images above)."""
    _hold_members(engine, [case])


def test_class_a_token_fuzz(engine):
    """150 members of random block types, random complete codes of up to 15 bits and tokens over the whole range of
    lengths and distances (``deflate_writer.fuzz``)."""
    members = W.fuzz()
    for at in range(0, len(members), 40):
        _hold_members(engine, members[at:at + 40])


# what each refusal draws: the kInflate* reason of csrc/ftk_inflate.h (1 block type, 2 stored lengths, 3 code lengths,
# 4 symbol, 5 distance, 6 overrun, 7 short).  A payload without a final block goes on into whatever follows it, so any
# check may be the one that ends it.
REASON = {
    "oversubscribed_literal_code": {3}, "oversubscribed_distance_code": {3}, "oversubscribed_code_length_code": {3},
    "repeat_16_first": {3}, "repeat_past_hlit_hdist": {3}, "no_end_of_block_code": {3}, "hclen_4_describes_no_code": {3},
    "hlit_287": {3}, "hlit_288": {3}, "hdist_31": {3}, "hdist_32": {3},
    "stored_len_nlen": {2}, "block_type_3_second": {1},
    "fixed_length_symbol_286": {4}, "fixed_length_symbol_287": {4}, "fixed_distance_symbol_30": {4}, "fixed_distance_symbol_31": {4},
    "one_distance_code_unassigned_pattern": {4}, "match_without_distance_code": {4},
    "distance_in_front_of_the_data": {5},
    "literal_beyond_isize": {6}, "match_beyond_isize": {6}, "stored_beyond_isize": {6},
    "final_block_short_of_isize": {7},
    "no_final_block": {1, 2, 3, 4, 5, 6},
}


def test_every_refusal_has_its_reason():
    assert sorted(REASON) == sorted(c.name for c in CASES if c.cls == "B")


@pytest.mark.parametrize("case", [c for c in CASES if c.cls == "B"], ids=lambda c: c.name)
def test_class_b_is_refused(engine, case):
    """Streams that zlib refuses, between two good members of 0xFF00 bytes (a stray distance or overrun stays inside the
    image's output): FTK_ERR_FORMAT in every loop, naming the bad block and the reason of ``REASON``; the good members
    alone decode."""
    good, good_data = W.good_neighbour()
    assert len(good_data) == W.BLOCK_DATA
    for loop, (rc, _, message) in zip(LOOPS, _inflate_each(engine, good + case.member() + good + W.EOF_MEMBER)):
        assert rc == L.FTK_ERR_FORMAT, (loop, rc, message)
        m = re.search(rb"\(block (\d+): reason (\d+)\)", message)
        assert m, (loop, message)  # (refused by the kernel's own check, not by the CRC pass behind it)
        print(case.name, loop, "reason", int(m.group(2)))
        assert int(m.group(1)) == 1, (loop, message)
        assert int(m.group(2)) in REASON[case.name], (loop, message)
    rc, got = _inflate(engine, good + good + W.EOF_MEMBER)
    assert rc == L.FTK_OK and got == good_data + good_data


@pytest.mark.parametrize("case", [c for c in CASES if c.cls == "C"], ids=lambda c: c.name)
def test_class_c_one_verdict(engine, case):
    """Incomplete codes whose unassigned patterns the stream never uses (zlib refuses them; ``build_table`` refuses
    over-subscription only): every loop either refuses or delivers exactly the intended bytes, and all three agree.
    Today the kernel accepts all three cases and delivers the intended bytes."""
    good, good_data = W.good_neighbour()
    results = _inflate_each(engine, good + case.member() + good + W.EOF_MEMBER)
    for loop, (rc, got, message) in zip(LOOPS, results):
        print(case.name, loop, "rc", rc, message)
        assert rc == L.FTK_ERR_FORMAT or (rc == L.FTK_OK and got == good_data + case.data + good_data), (loop, rc, message)
    assert len({rc for rc, _, _ in results}) == 1, [rc for rc, _, _ in results]


def _rows_table(text):
    cols = list(zip(*(line.split(b"\t") for line in text.splitlines())))
    return (np.array(cols[1], np.int64).astype(np.int32), np.array(cols[2], np.int64).astype(np.int32),
            np.array(cols[3], np.int64).astype(np.uint8), np.array([c == b"+" for c in cols[4]], np.uint8))


_FILE_CHILD = """
import sys
sys.path.insert(0, {root!r})
from tests.test_gpu_inflate_crafted import _stream_reencoded_rows
_stream_reencoded_rows(sys.argv[1])
print("ok")
"""


def _stream_reencoded_rows(path):
    from tests.test_gpu_device_parse import _stream_device
    text, cases = W.reencoded_rows()
    with open(path, "wb") as f:
        f.write(b"".join(c.member() for c in cases) + W.EOF_MEMBER)
    got, order, _ = _stream_device(path)
    assert order == ["chr7"], order
    want = _rows_table(text)
    assert got["chr7"][0] == len(want[0])
    for a, b in zip(got["chr7"][1], want):
        assert np.array_equal(a, b)


def test_reencoded_rows_through_the_streaming_decoder(tmp_path):
    """zlib's tokens for 160 KB of fragment rows under deep codes, cross-HLIT header runs and cuts into stored / fixed /
    dynamic blocks, as an unindexed .frag.gz: the stream's own launch of the kernel (its CRC pass, its slot ring) hands
    out the rows the file was made from - and so does the host inflate (FTK_DEVICE_INFLATE=0, a child process)."""
    _stream_reencoded_rows(str(tmp_path / "crafted.frag.gz"))
    r = subprocess.run([sys.executable, "-c", _FILE_CHILD.format(root=ROOT), str(tmp_path / "host.frag.gz")], capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, FTK_DEVICE_INFLATE="0"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-1500:] + r.stderr[-2500:]
