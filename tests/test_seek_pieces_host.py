"""hz_seek_pieces, the host plan of a gathered buffer (no GPU): through ctypes on seek tables made by
tests/ref_stream.py from seeded symbols and code lengths, and again through tests/pieces_probe.cpp, a
stand-alone host program built here with AddressSanitizer and UndefinedBehaviorSanitizer (host code only:
every sanitizer flag goes to the host compilation through -Xarch_host) and run as a child process.

Every property is arithmetic on the table, restated here in Python from include/huffman_amd.h
(hz_seek_span's margins, the placement rule); nothing is taken from the plan under test but the plan."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ref_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLK = 2048
HZ_EINVAL, HZ_EFORMAT = -1, -5
NBLOCKS = 300
LISTS = 24           # seeded lists of 1 .. 200 ranges


def _table(nblocks, tail, seed, start_bit=5):
    """(nsym, seek, payload_bytes): code lengths of 1 .. 24 bits on 4096 symbols, seeded uniform symbols."""
    rng = np.random.default_rng(seed)
    ln = np.zeros(65536, dtype=np.uint8)
    ln[:4096] = rng.integers(1, 25, 4096)
    nsym = (nblocks - 1) * BLK + tail
    sym = rng.integers(0, 4096, nsym).astype(np.uint16)
    pos = ref_stream.positions(sym, ln, start_bit)
    start, _, _ = ref_stream.index_arrays(pos, nsym)
    assert start.size == nblocks + 1
    return nsym, np.ascontiguousarray(start, dtype=np.uint64), (int(start[-1]) + 7) // 8


@pytest.fixture(scope="module")
def table():
    return _table(NBLOCKS, 3, 11)


def _lists(nsym):
    """Seeded lists: empties, duplicates, single symbols, block edges and long ranges among them."""
    rng = np.random.default_rng(2025)
    out = []
    for li in range(LISTS):
        n = (1, 2, 200)[li] if li < 3 else int(rng.integers(1, 201))
        rg, off = [], 0
        for _ in range(n):
            kind = int(rng.integers(0, 8))
            if kind == 0:
                b, c = int(rng.integers(0, nsym + 1)), 0
            elif kind == 1 and rg:
                b, c, _ = rg[int(rng.integers(0, len(rg)))]
            elif kind == 2:
                b = int(rng.integers(0, nsym))
                c = int(rng.integers(1, min(nsym - b, 9 * BLK) + 1))
            elif kind == 3:
                b = int(rng.integers(1, NBLOCKS)) * BLK - 1
                c = 2
            else:
                b = int(rng.integers(0, nsym))
                c = int(rng.integers(1, min(nsym - b, 600) + 1))
            rg.append((b, c, off))
            off += 2 * c
        out.append(rg)
    return out


def plan(lib, seek, nsym, pay, ranges, cap=None):
    """(rc, pieces, out, buf_bytes, seek_words) of one hz_seek_pieces call; arrays of u64 rows."""
    n = len(ranges)
    rg = np.array(ranges, dtype=np.uint64).reshape(-1, 3)
    pieces = np.full((max(n, 1), 6), 0xEE, dtype=np.uint64)
    out = np.full((max(n, 1), 4), 0xEE, dtype=np.uint64)
    np_, bb, sw = ctypes.c_uint32(77), ctypes.c_uint64(77), ctypes.c_uint64(77)
    rc = lib.hz_seek_pieces(seek.ctypes.data_as(ctypes.c_void_p), nsym, pay, rg.ctypes.data_as(ctypes.c_void_p), n,
                            pieces.ctypes.data_as(ctypes.c_void_p), ctypes.byref(np_), out.ctypes.data_as(ctypes.c_void_p),
                            ctypes.byref(bb), ctypes.byref(sw))
    return rc, pieces[:np_.value].astype(object), out[:n].astype(object), bb.value, sw.value


def span(seek, b, c, pay):
    """hz_seek_span restated: 32 bytes before the first block's start byte rounded down to 16 (or byte 0),
    32 after the last block's end byte; clamped to the payload."""
    b0, b1 = b // BLK, (b + c - 1) // BLK
    first, last = int(seek[b0]) // 8, (int(seek[b1 + 1]) + 7) // 8
    return (first - 32) // 16 * 16 if first > 32 else 0, min(last + 32, pay), b0, b1


def check_plan(seek, nsym, pay, ranges, pieces, out, buf_bytes, seek_words):
    assert len(out) == len(ranges)
    span_sum = 0
    for (b, c, o), row in zip(ranges, out):
        assert (row[0], row[1], row[2]) == (b, c, o)
        if c == 0:
            assert row[3] == 0
            continue
        lo, hi, b0, b1 = span(seek, b, c, pay)
        span_sum += hi - lo
        assert row[3] < len(pieces)
        sb, nbytes, _, fb, _, nblk = pieces[row[3]]
        assert sb <= lo and hi <= sb + nbytes, (b, c)
        assert fb <= b0 and b1 < fb + nblk, (b, c)
    used = np.zeros(seek_words, dtype=np.int64)
    buf_end = word = 0
    for k, (sb, nbytes, bufb, fb, si, nblk) in enumerate(pieces):
        assert nbytes > 0 and sb + nbytes <= pay and fb + nblk + 1 <= seek.size
        if k:
            psb, pn = pieces[k - 1][0], pieces[k - 1][1]
            assert sb > psb + pn                      # ascending, disjoint, not touching
        assert bufb % 64 == sb % 64
        assert bufb == (buf_end + 63) // 64 * 64 + sb % 64   # the placement rule; no overlap in the buffer follows
        buf_end = bufb + nbytes
        assert si == word                             # seek_index counts up in piece order
        used[si:si + nblk + 1] += 1
        word += nblk + 1
    assert word == seek_words and (used == 1).all()
    assert buf_bytes == (buf_end + 15) // 16 * 16
    piece_sum = sum(p[1] for p in pieces)
    assert piece_sum <= span_sum
    assert buf_bytes <= piece_sum + 128 * len(pieces)
    # every piece is the union of the spans that name it, no more
    for k, p in enumerate(pieces):
        mine = [span(seek, b, c, pay) for (b, c, _), row in zip(ranges, out) if c and row[3] == k]
        assert mine and p[0] == min(m[0] for m in mine) and p[0] + p[1] == max(m[1] for m in mine)
        assert p[3] == min(m[2] for m in mine) and p[3] + p[5] - 1 == max(m[3] for m in mine)


def test_random_lists(built_lib, table):
    nsym, seek, pay = table
    for ranges in _lists(nsym):
        rc, pieces, out, bb, sw = plan(built_lib, seek, nsym, pay, ranges)
        assert rc == 0
        check_plan(seek, nsym, pay, ranges, pieces, out, bb, sw)


def test_scattered_list(built_lib):
    """16 single-block ranges spaced evenly over 4096 blocks of 3000 +- 300 bits: 16 pieces, under 1 % of the
    payload. Each piece is at most a block (412 bytes), 64 bytes of margins and 15 of rounding; with the
    placement's 128 per piece that is under 10 KiB of about 1.5 MiB."""
    rng = np.random.default_rng(4096)
    bits = rng.integers(2700, 3301, 4096).astype(np.uint64)
    seek = np.concatenate([np.zeros(1, np.uint64), np.cumsum(bits, dtype=np.uint64)])
    nsym, pay = 4096 * BLK, (int(seek[-1]) + 7) // 8
    ranges = [((256 * i + 100) * BLK + 17, 1000, 2000 * i) for i in range(16)]
    rc, pieces, out, bb, sw = plan(built_lib, seek, nsym, pay, ranges)
    assert rc == 0 and len(pieces) == 16 and sw == 32
    check_plan(seek, nsym, pay, ranges, pieces, out, bb, sw)
    assert [int(r[3]) for r in out] == list(range(16))
    assert bb <= 16 * (413 + 64 + 15 + 128) and 100 * bb < pay


def test_merging(built_lib, table):
    nsym, seek, pay = table
    one = lambda ranges: plan(built_lib, seek, nsym, pay, ranges)  # noqa: E731
    # adjacent blocks: the spans overlap by their margins
    rc, pieces, out, bb, sw = one([(10 * BLK + 5, 10, 0), (11 * BLK + 5, 10, 20)])
    assert rc == 0 and len(pieces) == 1 and pieces[0][3] == 10 and pieces[0][5] == 2 and sw == 3
    assert [r[3] for r in out] == [0, 0]
    # the same block, listed later first
    rc, pieces, out, bb, sw = one([(20 * BLK + 900, 10, 0), (20 * BLK + 5, 10, 20)])
    assert rc == 0 and len(pieces) == 1 and pieces[0][5] == 1 and [r[3] for r in out] == [0, 0]
    # block 0 starts the stream
    rc, pieces, out, bb, sw = one([(150 * BLK, 1, 0), (3, 4, 2)])
    assert rc == 0 and len(pieces) == 2 and pieces[0][0] == 0 and pieces[0][2] == 0 and [r[3] for r in out] == [1, 0]
    # the last block: the span's end is clamped to the payload
    rc, pieces, out, bb, sw = one([(nsym - 1, 1, 0)])
    assert rc == 0 and len(pieces) == 1 and pieces[0][0] + pieces[0][1] == pay
    assert pieces[0][3] == NBLOCKS - 1 and pieces[0][5] == 1
    # far apart: two pieces, ascending whatever the list's order
    rc, pieces, out, bb, sw = one([(200 * BLK, 5, 0), (100 * BLK, 5, 10)])
    assert rc == 0 and len(pieces) == 2 and pieces[0][3] == 100 and [r[3] for r in out] == [1, 0]
    check_plan(seek, nsym, pay, [(200 * BLK, 5, 0), (100 * BLK, 5, 10)], pieces, out, bb, sw)


def test_refusals(built_lib, table):
    nsym, seek, pay = table
    good = (5 * BLK, 100, 0)
    assert plan(built_lib, seek, nsym, pay, [good, (nsym - 1, 2, 200)])[0] == HZ_EINVAL
    assert plan(built_lib, seek, nsym, pay, [(nsym + 1, 0, 0)])[0] == HZ_EINVAL
    desc = seek.copy()
    desc[8] = desc[6] - np.uint64(64)       # block 6 .. 7 now ends before it starts, by more than a byte
    assert plan(built_lib, desc, nsym, pay, [good, (6 * BLK, 2 * BLK, 200)])[0] == HZ_EINVAL
    assert plan(built_lib, seek, nsym, pay, [good])[0] == 0
    # a span that starts at or past the payload's end: the table is not this payload's
    lo = span(seek, 200 * BLK, 10, pay)[0]
    assert plan(built_lib, seek, nsym, lo, [good, (200 * BLK, 10, 200)])[0] == HZ_EFORMAT
    assert plan(built_lib, seek, nsym, lo + 1, [good, (200 * BLK, 10, 200)])[0] == 0
    assert plan(built_lib, seek, nsym, lo, [good, (200 * BLK, 0, 200)])[0] == 0      # an empty range has no span
    # null outputs
    rg = np.array([good], dtype=np.uint64)
    pieces, out = np.zeros((1, 6), np.uint64), np.zeros((1, 4), np.uint64)
    np_, bb, sw = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    full = [p(seek), nsym, pay, p(rg), 1, p(pieces), ctypes.byref(np_), p(out), ctypes.byref(bb), ctypes.byref(sw)]
    assert built_lib.hz_seek_pieces(*full) == 0
    for i in (3, 5, 6, 7, 8, 9):
        args = list(full)
        args[i] = None
        assert built_lib.hz_seek_pieces(*args) == HZ_EINVAL, i
    args = list(full)
    args[0] = None                           # no table, and a range that needs one
    assert built_lib.hz_seek_pieces(*args) == HZ_EINVAL


def test_no_ranges(built_lib, table):
    nsym, seek, pay = table
    rc, pieces, out, bb, sw = plan(built_lib, seek, nsym, pay, [])
    assert (rc, len(pieces), len(out), bb, sw) == (0, 0, 0, 0, 0)
    np_, bb, sw = ctypes.c_uint32(9), ctypes.c_uint64(9), ctypes.c_uint64(9)
    assert built_lib.hz_seek_pieces(None, nsym, pay, None, 0, None, ctypes.byref(np_), None, ctypes.byref(bb),
                                    ctypes.byref(sw)) == 0
    assert (np_.value, bb.value, sw.value) == (0, 0, 0)
    # only empty ranges: no piece, every range names piece 0
    rc, pieces, out, bb, sw = plan(built_lib, seek, nsym, pay, [(7, 0, 0), (nsym, 0, 0)])
    assert (rc, len(pieces), bb, sw) == (0, 0, 0, 0) and [r[3] for r in out] == [0, 0]


def test_python_form(built_lib, table):
    import huffman_amd
    nsym, seek, pay = table
    ranges = _lists(nsym)[5]
    pieces, out, bb, sw = huffman_amd.seek_pieces(seek, nsym, pay, ranges)
    rc, p2, o2, bb2, sw2 = plan(built_lib, seek, nsym, pay, ranges)
    assert (bb, sw) == (bb2, sw2) and pieces.dtype.names[0] == "stream_byte" and out.dtype.names[3] == "piece"
    assert [tuple(int(v) for v in r) for r in pieces] == [tuple(r) for r in p2]
    assert [tuple(int(v) for v in r) for r in out] == [tuple(r) for r in o2]
    assert "seek_pieces" in huffman_amd.__all__ and "decode_ranges_file" in huffman_amd.__all__


def test_probe_under_sanitizers(built_lib, table, tmp_path):
    """The same seeded lists (and the refused ones) through the stand-alone program, built with
    AddressSanitizer and UndefinedBehaviorSanitizer: the same plans, and no report."""
    from huffman_amd import build
    nsym, seek, pay = table
    lists = _lists(nsym) + [[], [(7, 0, 0)], [(5 * BLK, 100, 0), (nsym - 1, 2, 200)]]
    exe = str(tmp_path / "pieces_probe")
    csrc = os.path.join(ROOT, "huffman_amd", "csrc")
    r = subprocess.run([build.HIPCC, "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        os.path.join(ROOT, "tests", "pieces_probe.cpp"), os.path.join(csrc, "hz_seek_plan.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    words = [nsym, pay, seek.size] + [int(v) for v in seek] + [len(lists)]
    for rg in lists:
        words.append(len(rg))
        for row in rg:
            words.extend(row)
    inp = tmp_path / "lists.bin"
    inp.write_bytes(np.array(words, dtype="<u8").tobytes())
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    want = []
    for rg in lists:
        rc, pieces, out, bb, sw = plan(built_lib, seek, nsym, pay, rg)
        want.append("%d %d %d %d" % (rc, len(pieces), bb, sw))
        if rc == 0:
            want += [" ".join(str(v) for v in row) for row in pieces]
            want += [" ".join(str(v) for v in row) for row in out]
    assert r.stdout.split("\n")[:-1] == want
