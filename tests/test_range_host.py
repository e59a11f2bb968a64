"""Host arithmetic of random access (no GPU): hz_seek_bytes and hz_seek_span against a seek
table built on the CPU by walking the oracle's payload of tests/golden/romeo.txt."""
import ctypes
import os

import numpy as np
import pytest

import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BLK = 2048
HZ_EINVAL = -1


@pytest.fixture(scope="module")
def romeo(built_lib):
    """(nsym, seek table as uint64[nblocks + 1], payload byte count) of romeo.txt's stream; bits count
    from the file byte that holds the first payload bit."""
    with open(os.path.join(GOLD, "romeo.txt"), "rb") as f:
        data = f.read()
    blob = oracle_lib.encode(data)
    _, ln, code, info = oracle_lib.parse_header(blob)
    payload = np.frombuffer(blob, dtype=np.uint8)[info[1]:]
    nsym = len(data) // 2
    nb = (nsym + BLK - 1) // BLK
    seek = np.zeros(nb + 1, dtype=np.uint64)
    pos = info[2]
    for b in range(nb):
        seek[b] = pos
        cnt, pos, _ = oracle_lib.walk(payload, ln, code, pos, payload.size * 8, max_count=min(BLK, nsym - b * BLK))
        assert cnt == min(BLK, nsym - b * BLK)
    seek[nb] = pos
    assert (pos + 7) // 8 == payload.size
    return nsym, seek, payload.size


def _span(lib, seek, nsym, begin, count):
    b, e = ctypes.c_uint64(123), ctypes.c_uint64(456)
    rc = lib.hz_seek_span(seek.ctypes.data_as(ctypes.c_void_p), nsym, begin, count, ctypes.byref(b), ctypes.byref(e))
    return rc, b.value, e.value


def test_seek_bytes(built_lib):
    import huffman_amd
    assert huffman_amd.seek_bytes(0) == 0
    for nsym, blocks in [(1, 1), (2047, 1), (2048, 1), (2049, 2), (5 * 2048 + 3, 6), ((1 << 33) + 1, (1 << 22) + 1)]:
        assert huffman_amd.seek_bytes(nsym) == 8 * (blocks + 1)
        # the seek table is the head of the block index
        assert huffman_amd.seek_bytes(nsym) < huffman_amd.index_bytes(nsym)


def test_margins_exported(built_lib):
    from huffman_amd import _lib
    with open(os.path.join(ROOT, "include", "huffman_amd.h")) as f:
        text = f.read()
    assert f"#define HZ_RANGE_LEAD_BYTES {_lib.HZ_RANGE_LEAD_BYTES}" in text
    assert f"#define HZ_RANGE_TAIL_BYTES {_lib.HZ_RANGE_TAIL_BYTES}" in text
    # the staging window starts 16 bytes below the 16-byte chunk of the first bit (up to 15 bytes below it)
    assert _lib.HZ_RANGE_LEAD_BYTES >= 31


def test_span_holds_the_blocks_with_margins(built_lib, romeo):
    from huffman_amd import _lib
    nsym, seek, _ = romeo
    nb = seek.size - 1
    assert nb >= 4
    lead, tail = _lib.HZ_RANGE_LEAD_BYTES, _lib.HZ_RANGE_TAIL_BYTES
    cases = [(0, nsym), (0, 1), (nsym - 1, 1), (BLK, BLK), (BLK - 1, 1), (BLK - 1, 2), (BLK, 1), (BLK + 1, 1),
             (2 * BLK - 1, BLK + 2), (3 * BLK, nsym - 3 * BLK), (7, 3 * BLK)]
    for begin, count in cases:
        b0, b1 = begin // BLK, (begin + count - 1) // BLK
        rc, bb, be = _span(built_lib, seek, nsym, begin, count)
        assert rc == 0, (begin, count)
        first, last = int(seek[b0]) // 8, (int(seek[b1 + 1]) + 7) // 8
        assert bb % 16 == 0
        assert bb == (max(first - lead, 0) // 16) * 16, (begin, count)
        assert be == last + tail, (begin, count)
        assert bb <= first and be >= last  # the blocks' own bytes are inside


def test_block_boundaries_pick_the_right_blocks(built_lib, romeo):
    nsym, seek, _ = romeo
    # on, just before and just after the boundary between blocks 1 and 2
    on = _span(built_lib, seek, nsym, 2 * BLK, 1)
    before = _span(built_lib, seek, nsym, 2 * BLK - 1, 1)
    after = _span(built_lib, seek, nsym, 2 * BLK + 1, 1)
    both = _span(built_lib, seek, nsym, 2 * BLK - 1, 2)
    assert on[0] == before[0] == after[0] == both[0] == 0
    assert on == after                      # both inside block 2
    assert before[2] < on[2] and before[1] <= on[1]   # block 1 ends where block 2 starts
    assert both[1] == before[1] and both[2] == on[2]  # blocks 1 and 2
    assert before[2] == (int(seek[2]) + 7) // 8 + 32
    assert on[2] == (int(seek[3]) + 7) // 8 + 32


def test_begin_is_clamped_at_zero(built_lib, romeo):
    nsym, seek, _ = romeo
    assert int(seek[0]) // 8 < 32
    rc, bb, _ = _span(built_lib, seek, nsym, 0, 10)
    assert rc == 0 and bb == 0


def test_empty_and_invalid_ranges(built_lib, romeo):
    nsym, seek, _ = romeo
    assert _span(built_lib, seek, nsym, 7, 0) == (0, 0, 0)
    assert _span(built_lib, seek, nsym, nsym, 0) == (0, 0, 0)
    assert _span(built_lib, seek, nsym, 0, nsym + 1)[0] == HZ_EINVAL
    assert _span(built_lib, seek, nsym, nsym, 1)[0] == HZ_EINVAL
    assert _span(built_lib, seek, nsym, nsym + 1, 0)[0] == HZ_EINVAL
    assert _span(built_lib, seek, nsym, 1, (1 << 64) - 1)[0] == HZ_EINVAL  # begin + count wraps


def test_python_wrapper(built_lib, romeo):
    import huffman_amd
    nsym, seek, pay = romeo
    assert huffman_amd.seek_span(seek, nsym, 0, nsym) == (0, pay + 32)
    with pytest.raises(huffman_amd.HZError):
        huffman_amd.seek_span(seek, nsym, 1, nsym)
