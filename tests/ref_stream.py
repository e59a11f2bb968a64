"""A plain host model of one packed stream: what hz_pack must write for given symbols under any
prefix code -- the payload bytes and the block index (include/huffman_amd.h "Block index") -- and
the serial decode of a bit span. numpy plus the CPU oracle (oracle_lib.pack_range / walk); no
device code, so the device tests compare every kernel with this file, not with each other."""
from types import SimpleNamespace

import numpy as np

import oracle_lib

BLK = 2048      # symbols per block (hz_index_stride)
CHAIN = 8       # symbols per chain
CHAINS = BLK // CHAIN


def nblocks(nsym):
    return (nsym + BLK - 1) // BLK


def index_nbytes(nsym):
    """hz_index_bytes: u64 start[nblocks + 1], u64 max_bits, u16 sub[nblocks][256]."""
    nb = nblocks(nsym)
    return 8 * (nb + 2) + 2 * CHAINS * nb if nsym else 0


def positions(sym, ln, start_bit):
    """pos[i] = the stream bit where codeword i starts; pos[nsym] = the stream's end bit."""
    sym = np.asarray(sym, dtype=np.uint16)
    bits = np.asarray(ln)[sym].astype(np.uint64)
    return np.uint64(start_bit) + np.concatenate([np.zeros(1, np.uint64), np.cumsum(bits, dtype=np.uint64)])


def payload_bytes(sym, ln, code, start_bit, lead, pos=None):
    """The stream from byte 0 of its buffer to the next 32-bit boundary after its end: the bits of
    the first word before start_bit are `lead`, right aligned; the bits after the end are zero."""
    sym = np.ascontiguousarray(sym, dtype="<u2")
    pos = positions(sym, ln, start_bit) if pos is None else pos
    end = int(pos[-1])
    nbytes = 4 * ((end + 31) // 32)
    out = oracle_lib.pack_range(sym.view(np.uint8), 0, sym.size, ln, code, start_bit, max(nbytes, 4))[:nbytes]
    w0 = 32 * (start_bit // 32)       # the lead bits sit just before start_bit, in its word
    k = start_bit - w0
    assert 0 <= lead < (1 << k) or (k == 0 and lead == 0)
    for i in range(k):
        if (lead >> (k - 1 - i)) & 1:
            p = w0 + i
            out[p >> 3] |= 0x80 >> (p & 7)
    return out


def index_arrays(pos, nsym):
    """(start[nblocks + 1], max_bits, sub[nblocks][256]) from the codeword positions."""
    nb = nblocks(nsym)
    start = np.concatenate([pos[0:nsym:BLK][:nb], pos[nsym:nsym + 1]]).astype(np.uint64)
    max_bits = int(np.diff(start).max())
    at = np.minimum(np.arange(nb, dtype=np.int64)[:, None] * BLK + CHAIN * np.arange(CHAINS, dtype=np.int64)[None, :], nsym)
    sub = (pos[at] & np.uint64(0xffff)).astype(np.uint16)   # a chain past the end: the end bit's low 16 bits
    return start, max_bits, sub


def index_bytes(pos, nsym):
    """The index serialised in hz_index_bytes' layout."""
    start, max_bits, sub = index_arrays(pos, nsym)
    out = np.concatenate([start.view(np.uint8), np.array([max_bits], np.uint64).view(np.uint8),
                          np.ascontiguousarray(sub, dtype="<u2").view(np.uint8).ravel()])
    assert out.size == index_nbytes(nsym)
    return out


def model(sym, ln, code, start_bit=0, lead=0):
    """Everything hz_pack writes for `sym` (u16) under the prefix code (ln, code)."""
    sym = np.ascontiguousarray(sym, dtype="<u2")
    assert sym.size > 0
    pos = positions(sym, ln, start_bit)
    start, max_bits, sub = index_arrays(pos, sym.size)
    return SimpleNamespace(sym=sym, nsym=sym.size, start_bit=start_bit, lead=lead, pos=pos, end_bit=int(pos[-1]),
                           payload=payload_bytes(sym, ln, code, start_bit, lead, pos), start=start,
                           max_bits=max_bits, sub=sub, index=index_bytes(pos, sym.size))


def span_decode(payload, ln, code, begin, end, max_count=1 << 62):
    """Serial decode of the codewords that START in stream bits [begin, end), entered at `begin`
    (any bit, a codeword start or not): (count, exit bit = where the next codeword starts, u16
    symbols). Bits past the payload read as zeros."""
    max_count = min(max_count, max(end - begin, 0) + 1)   # every codeword has a bit: bounds the walk past the payload
    n, xit, out = oracle_lib.walk(payload, ln, code, begin, end, max_count=max_count, decode=True)
    return n, xit, np.frombuffer(out.tobytes(), dtype="<u2").copy()
