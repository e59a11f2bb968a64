"""Designed PART lists for the split index-less decode (hz_indexless_scan / _refix / _decode / _seek),
over the plain host model of a stream (tests/ref_stream.py). numpy only, no device code: the expected
result of a part [pb, pe) (payload bits after the stream's start bit) is arithmetic on the model's
codeword positions m.pos, with no decoder involved:

    entry   = the first pos >= start + pb       exit  = the first pos >= start + pe
    count   = the codewords between them        first = the index of the entry's codeword

The TILING list cuts the `chains` stream of 3 * 2048 + 5 symbols (symbol 2047 forced to a longest code)
from bit 0 to its end bit so that it holds, for every codebook: 1-bit parts on and off a codeword start,
parts with no codeword start in them (one placed so that the next codeword is number 2048, a seek-table
boundary), 40 consecutive 1-bit parts, widths 1, 2, 3, 5 .. 89, 24 parts of 128 bits from a 128-aligned
bit (what huffman_amd/dist.py part_range hands out for short payloads) and the ordinary parts between.
The NON-TILING list is [0, E) for the 128 values of E just below the end bit of the stream of
40 * 2048 + 777 symbols: the last chain's width takes every residue modulo 128, whatever chain length
the library chooses. The PADDING part runs past the end bit into the payload's zero bits; the model has
no codewords there, so its reference is ref_stream.span_decode.

An ISOLATED SLICE of a part is the least byte range include/huffman_amd.h asks for (the lead-in, the part,
max_len bits after it), at least 16 bytes, lowered by up to 15 bytes so that its first byte's residue
modulo 16 -- and with it the offset between a stream bit and its bit in the 64-byte aligned view --
cycles through R16 while the pointer's residue modulo 64 cycles through R64.

tests/test_parts_cases.py asserts on the CPU that every list really holds each edge for every codebook."""
import zlib
from types import SimpleNamespace

import numpy as np

import ref_stream
from table_books import book

BLK = 2048
LEAD_BITS = 1024                 # HZ_INDEXLESS_LEAD_BITS
BOOKS = ["fib57", "hot25", "dense16", "even", "fixed16", "zipf21"]
START_BITS = [5, 45]
NSYM = 3 * BLK + 5
WAVES = 40 * BLK + 777           # test_gpu_designed_streams.WAVES
WIDTHS = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89]
ONE_BIT_RUN = 40
ALIGNED_PARTS = 24
R16 = (0, 1, 4, 7, 12, 15)       # a slice's first byte modulo 16
R64 = (0, 4, 16, 33, 60, 63)     # a slice's device pointer modulo 64
LAST_WIDTHS = 128                # the non-tiling list's parts

_models = {}


def entry_given(k):
    """Part k of a list is handed its true entry at the scan (every third part); the others walk theirs and
    are refixed where the walk did not find it."""
    return k % 3 == 2


def stream(name, start_bit, nsym=NSYM):
    """(book, model) of the `chains` stream of a codebook: longest and shortest codes alternating inside the
    8-symbol chains; symbol 2047 (where there is one) a longest code."""
    key = (name, start_bit, nsym)
    if key not in _models:
        from test_gpu_designed_streams import _lead, _stream
        bk = book(name)
        rng = np.random.default_rng(zlib.crc32(("parts-%s-%d-%d" % key).encode()))
        sym = _stream(bk, "chains", nsym, rng)
        if nsym > BLK:
            sym[BLK - 1] = int(np.argmax(bk.ln))      # a code of max_len bits
        _models[key] = (bk, ref_stream.model(sym, bk.ln, bk.code, start_bit, _lead(start_bit)))
    return _models[key]


def part_ref(m, pb, pe):
    """The model's answer for the part [pb, pe), pe at most the stream's payload bits."""
    assert 0 <= pb < pe <= m.end_bit - m.start_bit
    first = int(np.searchsorted(m.pos, np.uint64(m.start_bit + pb), "left"))
    last = int(np.searchsorted(m.pos, np.uint64(m.start_bit + pe), "left"))
    return SimpleNamespace(pb=pb, pe=pe, first=first, count=last - first, entry=int(m.pos[first]),
                           exit=int(m.pos[last]), sym=m.sym[first:last])


def tiling_cuts(bk, m):
    """The tiling list's cuts: sorted payload bits from 0 to the end bit; consecutive cuts are the parts."""
    rel = lambda i: int(m.pos[i]) - m.start_bit  # noqa: E731
    P = m.end_bit - m.start_bit
    L = int(bk.ln[m.sym[BLK - 1]])
    assert L == int(bk.ln.max()) and L >= 3
    a = rel(BLK - 1)
    groups = [[0]]
    d = rel(1000)                                    # the widths, one after another
    groups.append([d + int(w) for w in np.concatenate([[0], np.cumsum(WIDTHS)])])
    groups.append([a, a + 1, a + L - 1, a + L])      # around codeword 2047
    c = rel(m.nsym // 2)                             # 1-bit parts from a codeword start
    groups.append([c + i for i in range(ONE_BIT_RUN + 1)])
    g = (rel(4500) + 127) // 128 * 128               # part_range's 128-bit parts
    groups.append([g + 128 * i for i in range(ALIGNED_PARTS + 1)])
    groups.append([P])
    for lo, hi in zip(groups, groups[1:]):           # the groups do not reach into each other
        assert lo[-1] < hi[0], (bk.name, lo[-1], hi[0])
    return [b for grp in groups for b in grp]


def tiling_parts(bk, m):
    cuts = tiling_cuts(bk, m)
    return [part_ref(m, pb, pe) for pb, pe in zip(cuts, cuts[1:])]


def last_width_parts(m):
    """[0, E) for LAST_WIDTHS consecutive E, the largest one bit below the end bit."""
    P = m.end_bit - m.start_bit
    return [part_ref(m, 0, E) for E in range(P - LAST_WIDTHS, P)]


def padding_part(bk, m, pb):
    """[pb, 8 * payload_bytes - start_bit): into the zero bits after the end bit. (pb, pe, first, entry,
    count, exit, symbols) from the serial walk of the payload, zeros after it, from the part's true entry."""
    pe = 8 * m.payload.size - m.start_bit
    assert pe > m.end_bit - m.start_bit >= pb
    first = int(np.searchsorted(m.pos, np.uint64(m.start_bit + pb), "left"))
    entry = int(m.pos[first])
    # (the oracle's reader stops at its buffer's end: the zeros the last codeword runs into are appended)
    padded = np.concatenate([m.payload, np.zeros(16, np.uint8)])
    count, xit, sym = ref_stream.span_decode(padded, bk.ln, bk.code, entry, m.start_bit + pe)
    assert count >= m.nsym - first and np.array_equal(sym[:m.nsym - first], m.sym[first:])
    return SimpleNamespace(pb=pb, pe=pe, first=first, count=count, entry=entry, exit=xit, sym=sym)


def slice_of(m, max_len, pb, pe, k):
    """Part k's isolated slice: payload bytes [b0, b1) and the residue modulo 64 of the pointer it is
    handed over at."""
    nbytes = m.payload.size
    lo = (m.start_bit + pb - min(LEAD_BITS, pb)) // 8
    hi = min(nbytes, (m.start_bit + pe + max_len) // 8 + 1)
    if hi - lo < 16:
        hi = min(nbytes, lo + 16)
        lo = hi - 16
    b0 = lo - (lo - R16[k % len(R16)]) % 16
    if b0 < 0:                                       # the stream's first bytes: no lower byte to begin at
        b0 = lo
    assert 0 <= b0 <= lo and hi - b0 >= 16
    return b0, hi, R64[(k + k // len(R16)) % len(R64)]
