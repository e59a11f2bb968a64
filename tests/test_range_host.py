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


# ---- far tables: positions past 2^32 bits, bytes and symbols -----------------------------------------
FAR_BITS = [1 << 32, 1 << 35, 1 << 37, 1 << 48]          # u32 bit position, byte offset, word index, any file size
FAR_BLOCKS = [0, 1 << 20, 1 << 21, (1 << 22) + 1]        # first block: output byte 2 sym = 2^32, sym = 2^32, past both
FAR_NB = 9


def _far_table(T, b0):
    """A host table of a stream whose blocks [b0, b0 + 9) (the last one ragged) are the only ones written:
    synthetic block sizes of 9 000 to 40 000 bits, placed so that bit T falls inside block b0 + 4."""
    rng = np.random.default_rng(T % 1000003 + b0)
    sizes = [int(v) for v in rng.integers(9000, 40000, FAR_NB)]
    near = [0]
    for v in sizes:
        near.append(near[-1] + v)
    shift = T - (near[4] + near[5]) // 2
    nsym = BLK * b0 + (FAR_NB - 1) * BLK + 5
    seek = np.zeros(b0 + FAR_NB + 1, dtype=np.uint64)    # (untouched pages of the zeros are never mapped)
    starts = [shift + v for v in near]
    seek[b0:] = np.array(starts, dtype=np.uint64)
    assert starts[4] < T < starts[5]
    return nsym, seek, starts


def _rule(starts, k0, k1):
    """include/huffman_amd.h in plain integers: 32 bytes before the first block's start byte, rounded down
    to 16 and never below 0; 32 bytes after the last block's end byte."""
    first = starts[k0] // 8
    last = -(-starts[k1 + 1] // 8)
    begin = ((first - 32) // 16) * 16 if first > 32 else 0
    return begin, last + 32


@pytest.mark.parametrize("b0", FAR_BLOCKS, ids=lambda v: "b0_%d" % v)
@pytest.mark.parametrize("T", FAR_BITS, ids=lambda v: "T2p%d" % (v.bit_length() - 1))
def test_span_on_far_tables(built_lib, T, b0):
    nsym, seek, starts = _far_table(T, b0)
    s0 = BLK * b0
    cases = [(0, nsym - s0), (0, 1), (nsym - s0 - 1, 1), (4 * BLK, 1), (4 * BLK, BLK), (3 * BLK + 7, 2 * BLK),
             (4 * BLK - 1, 2), (5 * BLK, 3 * BLK + 5), (8 * BLK, 5)]
    for begin, count in cases:
        k0, k1 = begin // BLK, (begin + count - 1) // BLK
        rc, bb, be = _span(built_lib, seek, nsym, s0 + begin, count)
        assert rc == 0, (begin, count)
        assert (bb, be) == _rule(starts, k0, k1), (begin, count, bb, be)
    # the blocks around T hold positions below and above it
    _, bb, be = _span(built_lib, seek, nsym, s0 + 4 * BLK, 1)
    assert 8 * bb < T < 8 * be
    assert _span(built_lib, seek, nsym, s0 + 7, 0) == (0, 0, 0)
    assert _span(built_lib, seek, nsym, nsym, 1)[0] == HZ_EINVAL


def test_span_straddles_byte_2p32_and_symbol_2p32(built_lib):
    """One range whose blocks lie on both sides of payload byte 2^32 (bit 2^35), in a stream whose range
    begins at or past symbol 2^32."""
    T, b0 = 1 << 35, 1 << 21
    nsym, seek, starts = _far_table(T, b0)
    sym_begin = BLK * b0 + 3 * BLK + 100
    assert sym_begin >= 1 << 32
    rc, bb, be = _span(built_lib, seek, nsym, sym_begin, 3 * BLK)
    assert rc == 0 and bb < (1 << 32) < be
    assert (bb, be) == _rule(starts, 3, 6)
    assert starts[3] // 8 < (1 << 32) < starts[7] // 8
    # a descending far table is refused
    bad = seek.copy()
    bad[b0 + 7] = bad[b0 + 3] - np.uint64(16)   # its end byte lies below the first block's start byte
    assert _span(built_lib, bad, nsym, sym_begin, 3 * BLK)[0] == HZ_EINVAL


def test_position_limit_exported(built_lib):
    """The binding's HZ_POS_LIMIT is the header's: UINT64_MAX - 0xFFFF, written there as that expression."""
    import re
    from huffman_amd import _lib
    with open(os.path.join(ROOT, "include", "huffman_amd.h")) as f:
        text = f.read()
    m = re.search(r"#define HZ_POS_LIMIT \(UINT64_MAX - (0x[0-9A-Fa-f]+)u\)", text)
    assert m, "HZ_POS_LIMIT is not defined as UINT64_MAX - <hex>u"
    assert _lib.HZ_POS_LIMIT == (1 << 64) - 1 - int(m.group(1), 16)
