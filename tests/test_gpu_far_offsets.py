"""Every base-offset parameter at stream positions past 2^32 bits, bytes, words and symbols.

The random-access and windowed calls take a base so that a small device buffer can stand for a piece of a
much larger stream: payload_byte_base (hz_decode_range / hz_decode_ranges), sym_base / bit_base /
stream_nsym (hz_pack_seek, hz_decode_indexless_seek, hz_indexless_seek), payload_bit_base with part_begin /
part_end (hz_indexless_scan / _refix / _decode) and the u64 out_byte of a batch range. Here three streams
of a few hundred KiB are presented as pieces of streams that pass bit 2^32 (the u32 bit position), 2^35
(the u32 byte offset), 2^37 (the u32 word index) and 2^48 (any file size), and as blocks 2^20, 2^21 and
2^22 + 1 onwards (output byte 2^32, symbol 2^32, past both). A position kept in a narrower register
anywhere on these paths changes an entry or a byte.

Expected values: every far result is the NEAR result (the same call at base 0, computed once per stream
and pinned here to the numpy model of tests/ref_stream.py) plus a constant, the input bytes, or
oracle_lib.walk on the near payload. Nothing is taken from a far call. The large buffers (a 32 MiB seek
table, a 1 GiB block index, a 4 GiB output) are allocated and touched only where a call addresses them.

Run as a script (`python tests/test_gpu_far_offsets.py wide`) it builds the far tables of a fib57 stream
whose chains are at least 131 072 bits long and prints "ok": the test starts it in a fresh process to set
HZ_CHAIN_MIN_BITS, which the library reads once, so that k_chain_seek's delta rebuild of record positions
(chain_rec_pos_wide) meets the far bases too.

Tolerance: none -- every check is bit-exact."""
import ctypes
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib  # noqa: E402
import ref_stream  # noqa: E402
from table_books import book  # noqa: E402

pytestmark = pytest.mark.gpu

BLK = 2048
GUARD = 64
ONES = (1 << 64) - 1
SENT = 0x5A5A5A5A5A5A5A5A
HZ_EINVAL = -1
START_BIT = 5
LEAD_PAD = 64            # stream bytes kept before the near payload's byte 0 in a far slice (>= 32 + 15)
PART_PAD = 256           # the same for a part's slice: HZ_INDEXLESS_LEAD_BITS = 1024 bits and a spare
T_BITS = [1 << 32, 1 << 35, 1 << 37, 1 << 48]
B0S = [1 << 20, 1 << 21, (1 << 22) + 1]
STREAMS = ["zipf", "fib57", "fixed16"]
BIT_BASES = ["T2p32", "T2p35", "T2p37", "T2p48", "odd2p37", "2p48p8"]


def _tid(T):
    return "T2p%d" % (T.bit_length() - 1)


def _bid(b0):
    return "b0_%d" % b0


@pytest.fixture(scope="module")
def codec(built_lib):
    from huffman_amd.pipeline import StreamCodec
    c = StreamCodec(0)
    c.far_tables = None     # the stream whose tables the context holds
    return c


# ---- the three streams and their near results -------------------------------------------------------
def _lead(start_bit):
    k = start_bit % 32
    return ((0x15a5f3c7 & ((1 << k) - 1)) | 1) if k else 0


def _symbols(codec, name):
    """(u16 symbols, Codebook, len[], code[]) of a stream, each under 1 MiB of input."""
    import torch
    from huffman_amd import build_codebook, codebook_arrays
    if name == "zipf":          # 70 blocks + 3 symbols from the device generator, the codebook of its own histogram
        n = 2 * (70 * BLK + 3)
        x = torch.empty(n, dtype=torch.uint8, device="cuda")
        codec.dev.generate(x.data_ptr(), n, offset=0, kind=1, alpha=1.1, seed=7)
        codec.sync()
        sym = x.cpu().numpy().view("<u2").copy()
        cb = build_codebook(np.bincount(sym, minlength=65536).astype(np.uint64))
        _, ln, code = codebook_arrays(cb)
        return sym, cb, ln, code
    if name == "fib57":         # codes of 50 to 56 bits: every whole block runs past 65 536 bits
        from test_gpu_designed_streams import _stream
        bk = book("fib57")
        sym = _stream(bk, "longest", 7 * BLK + 3, np.random.default_rng(57))
    else:                       # every code 16 bits, uniform over all 65 536 symbols: 9 blocks + 5
        bk = book("fixed16")
        sym = np.random.default_rng(3).integers(0, 65536, 9 * BLK + 5)
    return np.ascontiguousarray(sym, dtype="<u2"), bk.cb, bk.ln, bk.code


def _near(codec, name):
    """The near results, from the existing calls at base 0, each equal to the model's."""
    import torch
    from huffman_amd import index_bytes, seek_bytes
    sym, cb, ln, code = _symbols(codec, name)
    nsym = sym.size
    nb = ref_stream.nblocks(nsym)
    lead = _lead(START_BIT)
    m = ref_stream.model(sym, ln, code, START_BIT, lead)
    nbytes = m.payload.size
    assert 2 * nsym < (1 << 20) and nbytes % 4 == 0
    dev = codec.dev
    dev.upload(cb)
    codec.far_tables = name
    x = torch.from_numpy(sym.view(np.uint8).copy()).cuda()
    pay = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")
    idx = torch.full((index_bytes(nsym),), 0xA5, dtype=torch.uint8, device="cuda")
    dev.pack(x.data_ptr(), x.numel(), START_BIT, lead, pay.data_ptr(), nbytes, idx.data_ptr())
    pay2 = torch.zeros_like(pay)
    tab = torch.full((nb + 1,), SENT, dtype=torch.int64, device="cuda")
    assert seek_bytes(nsym) == 8 * (nb + 1)
    dev.pack_seek(x.data_ptr(), x.numel(), START_BIT, lead, pay2.data_ptr(), nbytes, tab.data_ptr())
    out = torch.zeros(2 * nsym + 16, dtype=torch.uint8, device="cuda")
    dev.decode(pay.data_ptr(), nbytes, nsym, idx.data_ptr(), out.data_ptr())
    codec.sync()
    index_host = idx.cpu().numpy()
    assert np.array_equal(pay[:nbytes].cpu().numpy(), m.payload), name + ": near payload differs from the model"
    assert np.array_equal(index_host, m.index), name + ": near index differs from the model"
    assert np.array_equal(tab.cpu().numpy().view(np.uint64), m.start), name + ": near table differs from the model"
    assert torch.equal(pay2, pay), name + ": hz_pack_seek's payload differs from hz_pack's"
    assert np.array_equal(out[:2 * nsym].cpu().numpy(), sym.view(np.uint8)), name + ": near decode differs from the input"
    sub = index_host[8 * (nb + 2):].view("<u2").reshape(nb, 256).copy()     # pack's sub[] rows
    blocks = np.diff(m.start.astype(np.int64))
    if name == "fib57":
        assert int(blocks[:-1].min()) >= 65536
    rng = np.random.default_rng(99)
    fp = np.concatenate([rng.integers(0, 256, LEAD_PAD, dtype=np.uint8), m.payload,
                         rng.integers(0, 256, 64, dtype=np.uint8)])
    return SimpleNamespace(name=name, cb=cb, ln=ln, code=code, sym=sym, x=x, nsym=nsym, nb=nb, lead=lead, m=m,
                           nbytes=nbytes, pay=pay, start=m.start.copy(), sub=sub, max_bits=int(m.max_bits), fp=fp)


@pytest.fixture(scope="module")
def streams(codec):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _near(codec, name)
        s = made[name]
        if codec.far_tables != name:
            codec.dev.upload(s.cb)
            codec.far_tables = name
        return s
    return get


# ---- helpers ---------------------------------------------------------------------------------------------
def _same(got, want, what=""):
    """Two u64 arrays, exactly; the first difference in the message."""
    got, want = np.asarray(got, np.uint64), np.asarray(want, np.uint64)
    assert got.size == want.size, (what, got.size, want.size)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: entry %d = %d, expected %d (%d differ)" % (what, bad[0], got[bad[0]], want[bad[0]],
                                                                          bad.size)


def _u64(t):
    return t.cpu().numpy().view(np.uint64).copy()


def _guarded(nbytes):
    import torch
    buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0
    return buf, buf[GUARD:GUARD + nbytes]


def _guards_intact(buf, nbytes):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all())


def _base_for(s, T, mod64):
    """A byte base B = mod64 (mod 64) that puts stream bit T inside the middle block of the stream: positions
    below and above T occur in one call, and a carry crosses T inside a block."""
    mb = s.nb // 2
    q = (int(s.start[mb]) + int(s.start[mb + 1])) // 2
    B = (T - q) // 8 // 64 * 64 + mod64
    assert B % 16 == 0 and int(s.start[mb]) < T - 8 * B < int(s.start[mb + 1])
    return B


def _bit_base(s, key):
    mb = s.nb // 2
    if key.startswith("T2p"):
        return (1 << int(key[3:])) - int(s.start[mb])      # the middle block starts exactly at bit T
    return {"odd2p37": (1 << 37) + 12345, "2p48p8": (1 << 48) + 8}[key]


def _put(host, head):
    """Host bytes on the device at an address = head (mod 64), random bytes around them."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(31)
    buf = torch.randint(0, 256, (host.size + 8192,), dtype=torch.uint8, device="cuda", generator=g)
    off = 4096 + (head - (buf.data_ptr() + 4096)) % 64
    buf[off:off + host.size] = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    view = buf[off:off + host.size]
    assert view.data_ptr() % 64 == head
    return view


def _far_table(s, add, b0):
    """The stream's table as a far call sees it: hz_seek_bytes(nsym_far) bytes between eight guard words,
    the sentinel everywhere but entries b0 .. b0 + nb = near + add. Returns (whole buffer, table)."""
    import torch
    from huffman_amd import seek_bytes
    words = seek_bytes(BLK * b0 + s.nsym) // 8
    assert words == b0 + s.nb + 1
    buf = torch.full((8 + words + 8,), SENT, dtype=torch.int64, device="cuda")
    tab = buf[8:8 + words]
    if add is not None:
        tab[b0:] = torch.from_numpy((s.start + np.uint64(add)).view(np.int64)).cuda()
    return buf, tab


def _table_is(buf, at, want, what=""):
    """Entries at .. at + len(want) - 1 of the table inside `buf` equal `want`; every other word of the
    buffer, its guard words included, still holds the sentinel."""
    import torch
    want = np.asarray(want, np.uint64)
    _same(_u64(buf[8 + at:8 + at + want.size]), want, what)
    touched = torch.nonzero(buf != SENT).flatten().cpu().numpy()
    keep = np.nonzero(want != np.uint64(SENT))[0] + 8 + at
    assert np.array_equal(touched, keep), (what, "words written outside the call's entries", touched[:8], keep[:2])


def _ranges(s):
    """test_gpu_range's edge set for this stream and six seeded random ranges (near symbols)."""
    from test_gpu_range import _edge_ranges
    out = _edge_ranges(s.nsym, (s.nb - 1) * BLK)
    rng = np.random.default_rng(2024 + s.nsym)
    for _ in range(6):
        begin = int(rng.integers(0, s.nsym))
        out.append((begin, int(rng.integers(1, s.nsym - begin + 1))))
    return out


def _nblk(begin, count):
    return 0 if count == 0 else (begin + count - 1) // BLK - begin // BLK + 1


def _host_table(s, B, b0):
    """The far table on the host, addressed from entry 0 (the untouched zeros are never mapped)."""
    t = np.zeros(b0 + s.nb + 1, dtype=np.uint64)
    t[b0:] = s.start + np.uint64(8 * B)
    return t


def _range_calls(codec, s, B, b0, table, full):
    """hz_decode_range over every range: the whole far payload at a pointer = 0 (mod 64) and at one
    congruent to the base modulo 64, and hz_seek_span's bytes alone at a pointer 16 bytes short of
    congruence (48 past it for a span that begins on a 64-byte boundary) -- both branches of the moved
    view's head < r, at a far base."""
    import torch
    from huffman_amd import seek_span
    s0, nsym_far = BLK * b0, BLK * b0 + s.nsym
    fbase = B - LEAD_PAD
    host = _host_table(s, B, b0)
    whole = {}
    pending = []
    branches = set()
    for i, (begin, count) in enumerate(_ranges(s)):
        if i % 3 == 2 and count:
            bb, be = seek_span(host, nsym_far, s0 + begin, count)
            be = min(be, fbase + s.fp.size)
            assert bb % 16 == 0 and fbase <= bb < be
            r = bb % 64
            pay, base = _put(s.fp[bb - fbase:be - fbase], r - 16 if r else 48), bb
        else:
            head = 0 if i % 3 == 0 else fbase % 64
            if head not in whole:
                whole[head] = _put(s.fp, head)
            pay, base = whole[head], fbase
        branches.add(pay.data_ptr() % 64 < base % 64)
        off = (0, 2, 14)[i % 3]
        buf = torch.full((GUARD + 16 + 2 * count + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        lo = GUARD + off
        codec.dev.decode_range(pay.data_ptr(), pay.numel(), table.data_ptr(), nsym_far, s0 + begin, count,
                               buf[lo:].data_ptr(), full_index=full, payload_byte_base=base)
        pending.append((begin, count, buf, lo, base))
    codec.sync()
    for begin, count, buf, lo, base in pending:
        what = (s.name, begin, count, full, base)
        assert bool((buf[:lo] == 0xA5).all()) and bool((buf[lo + 2 * count:] == 0xA5).all()), what
        assert torch.equal(buf[lo:lo + 2 * count], s.x[2 * begin:2 * (begin + count)]), what
    return branches


def _batch_call(codec, s, B, b0, table, full, head):
    """hz_decode_ranges over every range in one call into one 0xA5 buffer, compared as a whole."""
    import torch
    s0, nsym_far = BLK * b0, BLK * b0 + s.nsym
    ranges = _ranges(s)
    offs, cur = [], GUARD
    for i, (_, count) in enumerate(ranges):
        off = (cur + 15) // 16 * 16 + (0, 2, 14)[i % 3]
        offs.append(off)
        cur = off + 2 * count + GUARD
    size = cur + 16
    buf = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    exp = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    for (b, c), o in zip(ranges, offs):
        exp[o:o + 2 * c] = s.x[2 * b:2 * (b + c)]
    rg = torch.tensor([[s0 + b, c, o] for (b, c), o in zip(ranges, offs)], dtype=torch.int64, device="cuda")
    stats = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    pay = _put(s.fp, head)
    codec.decode_ranges(pay, nsym_far, table, rg, buf, stats=stats, full_index=full, payload_byte_base=B - LEAD_PAD)
    codec.sync()
    if not torch.equal(buf, exp):
        bad = int(torch.nonzero(buf != exp)[0])
        raise AssertionError("%s: first differing byte %d of %d; offsets %s" % (s.name, bad, size, offs[:12]))
    st = [int(v) for v in stats.cpu()]
    assert st[3] == 0 and st[0] == sum(_nblk(b, c) for b, c in ranges), st


# ---- 1. hz_decode_range / hz_decode_ranges from the seek table, far bits ---------------------------------
@pytest.mark.parametrize("mod64", [0, 16, 48], ids=lambda v: "Bmod64_%d" % v)
@pytest.mark.parametrize("T", T_BITS, ids=_tid)
@pytest.mark.parametrize("name", STREAMS)
def test_ranges_far_bits_seek_table(codec, streams, name, T, mod64):
    s = streams(name)
    B = _base_for(s, T, mod64)
    _, table = _far_table(s, 8 * B, 0)
    branches = _range_calls(codec, s, B, 0, table, False)
    if mod64:   # (a base on a 64-byte boundary takes the other branch only where a span begins off one)
        assert branches == {False, True}
    _batch_call(codec, s, B, 0, table, False, head=0)
    _batch_call(codec, s, B, 0, table, False, head=B % 64)


# ---- 2. the same from a full index rebased to the far position ---------------------------------------------
def _far_index(s, B, b0):
    """Pack's index rebased by the header's rule: start[] + 8 B, sub[] + 8 B mod 2^16, max_bits unchanged;
    the rows of this stream's blocks alone are written into a buffer of hz_index_bytes(nsym_far)."""
    import torch
    from huffman_amd import index_bytes
    nbf = b0 + s.nb
    total = index_bytes(BLK * b0 + s.nsym)
    assert total == 8 * (nbf + 2) + 512 * nbf
    idx = torch.empty(total // 8, dtype=torch.int64, device="cuda")
    idx[b0:nbf + 1] = torch.from_numpy((s.start + np.uint64(8 * B)).view(np.int64)).cuda()
    idx[nbf + 1] = s.max_bits
    sub = ((s.sub.astype(np.uint64) + np.uint64(8 * B)) & np.uint64(0xffff)).astype("<u2")
    w0 = nbf + 2 + 64 * b0
    idx[w0:w0 + 64 * s.nb] = torch.from_numpy(np.ascontiguousarray(sub).reshape(-1).view(np.int64)).cuda()
    return idx


@pytest.mark.parametrize("T", T_BITS, ids=_tid)
@pytest.mark.parametrize("name", STREAMS)
def test_ranges_far_bits_full_index(codec, streams, name, T):
    s = streams(name)
    B = _base_for(s, T, 16)
    idx = _far_index(s, B, 0)
    _range_calls(codec, s, B, 0, idx, True)
    _batch_call(codec, s, B, 0, idx, True, head=0)


@pytest.mark.parametrize("name", STREAMS)
def test_ranges_far_symbols_full_index(codec, streams, name):
    """Blocks 2^21 onwards (symbols from 2^32) of a 1 GiB index of which only this stream's rows exist."""
    s = streams(name)
    b0 = 1 << 21
    B = _base_for(s, 1 << 37, 48)
    idx = _far_index(s, B, b0)
    _range_calls(codec, s, B, b0, idx, True)
    _batch_call(codec, s, B, b0, idx, True, head=0)


# ---- 3. far symbols: the stream is blocks [b0, b0 + nb) of a longer one --------------------------------------
@pytest.mark.parametrize("b0", B0S, ids=_bid)
@pytest.mark.parametrize("name", STREAMS)
def test_ranges_far_symbols_seek_table(codec, streams, name, b0):
    s = streams(name)
    B = _base_for(s, T_BITS[B0S.index(b0) + 1], 16)
    buf, table = _far_table(s, 8 * B, b0)
    _range_calls(codec, s, B, b0, table, False)
    _batch_call(codec, s, B, b0, table, False, head=0)
    _table_is(buf, b0, s.start + np.uint64(8 * B), "the table a decode reads")     # and never writes


# ---- 4. hz_decode_ranges with output past byte 2^32 -----------------------------------------------------------
@pytest.mark.parametrize("name", STREAMS)
def test_ranges_far_output(codec, streams, name):
    """One output buffer of 2^32 + 2^20 bytes, never filled as a whole: a range whose bytes straddle
    out_byte = 2^32, one wholly above it and one at 0."""
    import torch
    s = streams(name)
    out = torch.empty((1 << 32) + (1 << 20), dtype=torch.uint8, device="cuda")
    rows = [(BLK - 7, 3000, (1 << 32) - 2 * 1234), (3 * BLK + 1, 2 * BLK + 50, (1 << 32) + 40 * 4096 + 2), (5, 100, 0)]
    for _, c, o in rows:
        out[max(o - GUARD, 0):o + 2 * c + GUARD] = 0xA5
    assert rows[0][2] < (1 << 32) < rows[0][2] + 2 * rows[0][1]
    rg = torch.tensor([list(r) for r in rows], dtype=torch.int64, device="cuda")
    stats = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    _, table = _far_table(s, 0, 0)
    codec.decode_ranges(s.pay[:s.nbytes], s.nsym, table, rg, out, stats=stats, full_index=False)
    codec.sync()
    for b, c, o in rows:
        assert torch.equal(out[o:o + 2 * c], s.x[2 * b:2 * (b + c)]), (name, b, c, o)
        assert bool((out[max(o - GUARD, 0):o] == 0xA5).all()) and bool((out[o + 2 * c:o + 2 * c + GUARD] == 0xA5).all())
    st = [int(v) for v in stats.cpu()]
    assert st[3] == 0 and st[0] == sum(_nblk(b, c) for b, c, _ in rows), st


# ---- 5. hz_pack_seek ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b0", B0S, ids=_bid)
@pytest.mark.parametrize("key", BIT_BASES)
@pytest.mark.parametrize("name", STREAMS)
def test_pack_seek_far(codec, streams, name, key, b0):
    """The whole stream as symbols [2048 b0, 2048 b0 + nsym) of a stream that ends with it: the touched
    entries are the near table + bit_base, every other word keeps the sentinel, d_out's bytes are the near
    call's."""
    s = streams(name)
    bit_base = _bit_base(s, key)
    buf, tab = _far_table(s, None, b0)
    obuf, out = _guarded(s.nbytes)
    codec.dev.pack_seek(s.x.data_ptr(), s.x.numel(), START_BIT, s.lead, out.data_ptr(), s.nbytes, tab.data_ptr(), None,
                        BLK * b0, bit_base, BLK * b0 + s.nsym)
    codec.sync()
    _table_is(buf, b0, s.start + np.uint64(bit_base), name)
    assert np.array_equal(out.cpu().numpy(), s.m.payload) and _guards_intact(obuf, s.nbytes)


@pytest.mark.parametrize("T", T_BITS, ids=_tid)
@pytest.mark.parametrize("name", STREAMS)
def test_pack_seek_two_calls_share_a_far_boundary(codec, streams, name, T):
    """Two adjacent calls, as the streaming archive chains them: whole blocks [0, mb) of a stream that goes on
    (stream_nsym larger than the call), then the rest with the partial word carried as lead bits and
    bit_base = 8 x the bytes emitted. The boundary entry lies past T and both calls write the same value."""
    s = streams(name)
    b0 = B0S[T_BITS.index(T) % 3]
    s0, mb = BLK * b0, s.nb // 2
    bit_base = T - int(s.start[mb - 1])
    want = s.start + np.uint64(bit_base)
    assert int(want[mb]) > T
    buf, tab = _far_table(s, None, b0)
    obuf, out = _guarded(s.nbytes + 8)
    dev = codec.dev
    dev.pack_seek(s.x.data_ptr(), 2 * mb * BLK, START_BIT, s.lead, out.data_ptr(), out.numel(), tab.data_ptr(), None,
                  s0, bit_base, s0 + s.nsym)
    codec.sync()
    _table_is(buf, b0, want[:mb + 1], name + " first call")
    first = int(_u64(tab[b0 + mb:b0 + mb + 1])[0])
    end_bit = int(s.start[mb])                        # the first call's end, counted from byte 0 of d_out
    nbyte, sbit = end_bit // 32 * 4, end_bit % 32
    lead = int.from_bytes(s.m.payload[nbyte:nbyte + 4].tobytes(), "big") >> (32 - sbit) if sbit else 0
    rest = out[nbyte:]
    dev.pack_seek(s.x[2 * mb * BLK:].data_ptr(), 2 * (s.nsym - mb * BLK), sbit, lead, rest.data_ptr(), rest.numel(),
                  tab.data_ptr(), None, s0 + mb * BLK, bit_base + 8 * nbyte, s0 + s.nsym)
    codec.sync()
    _table_is(buf, b0, want, name + " both calls")
    assert int(_u64(tab[b0 + mb:b0 + mb + 1])[0]) == first == int(want[mb])
    assert np.array_equal(out[:s.nbytes].cpu().numpy(), s.m.payload) and _guards_intact(obuf, s.nbytes + 8)


@pytest.mark.parametrize("name", STREAMS)
def test_pack_seek_start_bit_past_2p32(codec, streams, name):
    """The writer's own positions past 2^32: the stream begins at bit 2^32 + 32 005 of d_out (an empty
    512 MiB buffer of which only the stream's words are touched), so the start bits the pack stores pass
    2^32 before bit_base is added. Bytes and table equal the near call's, moved by whole words."""
    import torch
    s = streams(name)
    W = (1 << 27) + 1000                                # the near call's word 0 is word W of d_out
    b0, bit_base = 1 << 20, (1 << 37) + 12345
    out = torch.empty(4 * W + s.nbytes + GUARD, dtype=torch.uint8, device="cuda")
    out[4 * W - GUARD:] = 0xA5
    buf, tab = _far_table(s, None, b0)
    codec.dev.pack_seek(s.x.data_ptr(), s.x.numel(), 32 * W + START_BIT, s.lead, out.data_ptr(), out.numel(),
                        tab.data_ptr(), None, BLK * b0, bit_base, BLK * b0 + s.nsym)
    codec.sync()
    _table_is(buf, b0, s.start + np.uint64(32 * W + bit_base), name)
    assert np.array_equal(out[4 * W:4 * W + s.nbytes].cpu().numpy(), s.m.payload)
    assert bool((out[4 * W - GUARD:4 * W] == 0xA5).all()) and bool((out[4 * W + s.nbytes:] == 0xA5).all())


# ---- 6. hz_decode_indexless_seek ---------------------------------------------------------------------------------
@pytest.mark.parametrize("b0", B0S, ids=_bid)
@pytest.mark.parametrize("key", BIT_BASES)
@pytest.mark.parametrize("name", STREAMS)
def test_indexless_seek_window_far(codec, streams, name, key, b0):
    """The stream as a window of a longer one, with an output and table only: entries = near + bit_base; the
    decoded bytes are the input; *d_end_bit counts from byte 0 of d_payload, so it is the near end bit."""
    import torch
    s = streams(name)
    bit_base = _bit_base(s, key)
    for table_only in (False, True):
        buf, tab = _far_table(s, None, b0)
        obuf, out = _guarded(2 * s.nsym)
        end = torch.full((8,), 0xA5, dtype=torch.uint8, device="cuda")
        codec.dev.decode_indexless_seek(s.pay.data_ptr(), s.nbytes, START_BIT, s.nsym,
                                        None if table_only else out.data_ptr(), tab.data_ptr(), end.data_ptr(),
                                        sym_base=BLK * b0, bit_base=bit_base, stream_nsym=BLK * b0 + s.nsym)
        codec.sync()
        _table_is(buf, b0, s.start + np.uint64(bit_base), "%s table_only=%s" % (name, table_only))
        assert int(_u64(end)[0]) == s.m.end_bit, (table_only, int(_u64(end)[0]), s.m.end_bit)
        assert _guards_intact(obuf, 2 * s.nsym)
        if table_only:
            assert bool((out == 0xA5).all())
        else:
            assert torch.equal(out, s.x)


@pytest.mark.parametrize("name", STREAMS)
def test_indexless_seek_truncated_far(codec, streams, name):
    """The payload cut to half at a far bit_base: entries of codewords that start inside it are near +
    bit_base; every later one and the end are exactly UINT64_MAX, not UINT64_MAX + bit_base."""
    import torch
    s = streams(name)
    b0, bit_base = 1 << 21, (1 << 48) + 8
    cut = s.nbytes // 2
    inside = s.start < np.uint64(8 * cut)
    assert 2 <= int(inside.sum()) <= s.nb - 1 and not bool((s.start == np.uint64(8 * cut)).any())
    want = np.where(inside, s.start + np.uint64(bit_base), np.uint64(ONES))
    buf, tab = _far_table(s, None, b0)
    end = torch.zeros(8, dtype=torch.uint8, device="cuda")
    codec.dev.decode_indexless_seek(s.pay.data_ptr(), cut, START_BIT, s.nsym, None, tab.data_ptr(), end.data_ptr(),
                                    sym_base=BLK * b0, bit_base=bit_base, stream_nsym=BLK * b0 + s.nsym)
    codec.sync()
    _table_is(buf, b0, want, name)
    assert int(_u64(end)[0]) == ONES


def test_fixed16_seek_of_2p28_codewords(codec, streams):
    """FIXED16 positions are arithmetic, start + 16 S, and S need not be small: a table-only call for
    2^28 + 6149 codewords over the 9-block payload. The entries the payload holds are near + bit_base; the
    131 067 entries of codewords it does not hold (16 S passes 2^32 among them) are exactly UINT64_MAX."""
    import torch
    s = streams("fixed16")
    nsym = (1 << 28) + 3 * BLK + 5
    nbf = ref_stream.nblocks(nsym)
    bit_base = (1 << 37) + 12345
    buf = torch.full((8 + nbf + 1 + 8,), SENT, dtype=torch.int64, device="cuda")
    end = torch.zeros(8, dtype=torch.uint8, device="cuda")
    codec.dev.decode_indexless_seek(s.pay.data_ptr(), s.nbytes, START_BIT, nsym, None, buf[8:].data_ptr(),
                                    end.data_ptr(), sym_base=0, bit_base=bit_base, stream_nsym=nsym)
    codec.sync()
    assert int(s.start[s.nb - 1]) < 8 * s.nbytes <= int(s.start[s.nb - 1]) + 16 * BLK   # block nb - 1 starts inside
    want = np.full(nbf + 1, ONES, dtype=np.uint64)
    want[:s.nb] = s.start[:s.nb] + np.uint64(bit_base)
    _table_is(buf, 0, want, "fixed16")
    assert int(_u64(end)[0]) == ONES


# ---- 7. parts: hz_indexless_scan / _refix / _decode / _seek at a far payload_bit_base ----------------------------
@pytest.mark.parametrize("b0", B0S, ids=_bid)
@pytest.mark.parametrize("T", T_BITS, ids=_tid)
@pytest.mark.parametrize("name", STREAMS)
def test_parts_far(codec, streams, name, T, b0):
    """The payload as the slice of a stream at payload_bit_base = 8 (B - 256), in two parts whose boundary
    is stream bit T: the first from its given entry, the second from its walked one (UINT64_MAX), refixed
    when that is not the first part's exit. Each part is then refixed twice, whatever its walked entry was:
    to the start of its SECOND codeword (one codeword fewer, the same exit) and back to its true entry, so
    hz_indexless_refix does real work at every threshold for every stream, FIXED16's arithmetic one
    included. d_summary = oracle_lib.walk on the near payload + 8 B on the two bit values, after every
    scan and refix; the seek entries, the decoded bytes and *d_end_bit come from the refixed state."""
    import torch
    s = streams(name)
    dev = codec.dev
    B = _base_for(s, T, 0)
    far = 8 * B
    P = s.m.end_bit - START_BIT
    pm = T - far - START_BIT                          # the boundary, in near bits after the start bit
    assert 0 < pm < P
    host = np.concatenate([s.fp[:LEAD_PAD].repeat(PART_PAD // LEAD_PAD), s.m.payload, np.zeros(64, np.uint8)])
    pay = _put(host, 0)
    bit0 = far - 8 * PART_PAD                         # stream bit of the slice's byte 0
    buf, tab = _far_table(s, None, b0)
    summ = torch.zeros(4, dtype=torch.int64, device="cuda")

    def summary():
        codec.sync()
        return [int(v) for v in _u64(summ)[:3]]

    first, entry = 0, START_BIT
    for pb, pe, known in ((0, pm, True), (pm, P, False)):
        cnt, xit, _ = oracle_lib.walk(s.m.payload, s.ln, s.code, entry, START_BIT + pe)
        one, second, _ = oracle_lib.walk(s.m.payload, s.ln, s.code, entry, START_BIT + pe, max_count=1)
        assert one == 1 and entry < second < xit and cnt > 8
        dev.indexless_scan(pay.data_ptr(), pay.numel(), START_BIT, far + pb, far + pe,
                           far + entry if known else ONES, summ.data_ptr(), nsym=0, payload_bit_base=bit0)
        got = summary()
        if got[2] != far + entry:
            assert not known
            dev.indexless_refix(far + entry, summ.data_ptr())
            got = summary()
        want = [cnt, far + xit, far + entry]
        assert got == want, (name, pb, pe, got, want)
        dev.indexless_refix(far + second, summ.data_ptr())
        got = summary()
        assert got == [cnt - 1, far + xit, far + second], (name, pb, pe, "refixed to the second codeword", got)
        dev.indexless_refix(far + entry, summ.data_ptr())
        got = summary()
        assert got == want, (name, pb, pe, "refixed back", got, want)
        dev.indexless_seek(BLK * b0 + first, cnt, BLK * b0 + s.nsym, tab.data_ptr())
        obuf, out = _guarded(2 * cnt)
        end = torch.zeros(8, dtype=torch.uint8, device="cuda")
        dev.indexless_decode(cnt, out.data_ptr(), end.data_ptr())
        codec.sync()
        assert torch.equal(out, s.x[2 * first:2 * (first + cnt)]) and _guards_intact(obuf, 2 * cnt), (name, pb, pe)
        assert int(_u64(end)[0]) == far + xit, (name, int(_u64(end)[0]), far + xit)
        lo = -(-first // BLK)
        hi = (first + cnt) // BLK if first + cnt < s.nsym else s.nb
        _same(_u64(tab[b0 + lo:b0 + hi + 1]), s.start[lo:hi + 1] + np.uint64(far), name + " part entries")
        first += cnt
        entry = xit
    assert first == s.nsym and entry == s.m.end_bit
    assert far + START_BIT < T < far + s.m.end_bit     # the parts lie on both sides of T
    _table_is(buf, b0, s.start + np.uint64(far), name)


def test_wide_chain_blocks_far(built_lib):
    """HZ_CHAIN_MIN_BITS=131072 (test hook, read once: a fresh process): every chain of a fib57 `longest`
    stream is at least 131 072 bits long, so its first decode block spans more than 65 536 bits and
    k_chain_seek rebuilds record positions from the record deltas (its counter says for how many entries,
    as in test_gpu_seek_build.py::test_wide_chain_blocks). Table only, at every bit threshold, the two
    other bit bases and every first block: entries = the model's start[] + bit_base."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "wide"], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, HZ_CHAIN_MIN_BITS="131072"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ---- 8. bases whose positions do not fit: refused at the call ---------------------------------------------------
def test_overflowing_bases_are_refused_at_the_call(codec, streams):
    """Every base-taking call returns HZ_EINVAL, with nothing launched, when its largest position is not
    below HZ_POS_LIMIT (include/huffman_amd.h "Stream positions"): at the limit exactly, where the sum
    wraps, and where the byte base times 8 wraps. Only calls that launch nothing are sent: the refused ones,
    then three just below the limit that have nothing to do (no symbols), which return HZ_OK."""
    import torch
    from huffman_amd._lib import HZ_POS_LIMIT
    s = streams("zipf")
    lib, h = codec.dev.lib, codec.dev.h
    n = s.nbytes
    assert HZ_POS_LIMIT == (1 << 64) - (1 << 16) and HZ_POS_LIMIT % 8 == 0
    out = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    buf, tab = _far_table(s, 0, 0)
    stats = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    rg = torch.tensor([[0, 16, 0]], dtype=torch.int64, device="cuda")
    p, t, o = s.pay.data_ptr(), tab.data_ptr(), out.data_ptr()
    byte_bases = [HZ_POS_LIMIT // 8 - n, 1 << 61, (1 << 61) + 16, (1 << 64) - 16, (1 << 64) - n]
    for base in byte_bases:
        for flags in (0, 1):
            assert lib.hz_decode_range(h, p, n, base, t, s.nsym, 0, 16, o, flags) == HZ_EINVAL, base
            assert lib.hz_decode_ranges(h, p, n, base, t, s.nsym, rg.data_ptr(), 1, o, out.numel(), stats.data_ptr(),
                                        flags) == HZ_EINVAL, base
    bit_bases = [HZ_POS_LIMIT - 8 * n, (1 << 64) - 8 * n, (1 << 64) - 8, ONES]
    pout = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    for bb in bit_bases:
        assert lib.hz_pack_seek(h, s.x.data_ptr(), s.x.numel(), START_BIT, s.lead, pout.data_ptr(), n, None, 0, bb,
                                s.nsym, t) == HZ_EINVAL, bb
        for d_out in (None, o):
            assert lib.hz_decode_indexless_seek(h, p, n, START_BIT, s.nsym, d_out, None, 0, bb, s.nsym, t) == HZ_EINVAL, bb
    summ = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    for bb in (HZ_POS_LIMIT - 8 * n, (1 << 64) - 8 * n, (1 << 64) - 8):
        pbeg = (bb + 2048 - START_BIT) & ONES         # a part the slice would hold, lead-in included
        assert lib.hz_indexless_scan(h, p, n, bb, START_BIT, 0, pbeg, (pbeg + 4096) & ONES, ONES,
                                     summ.data_ptr()) == HZ_EINVAL, bb
    codec.sync()                                       # nothing was launched: no error pending, nothing written
    assert bool((out == 0xA5).all()) and bool((pout == 0xA5).all())
    assert bool((stats == -1).all()) and bool((summ == -1).all())
    _table_is(buf, 0, s.start, "the table")
    # one bit below the limit the same checks pass: the calls are refused for their positions alone
    assert lib.hz_pack_seek(h, s.x.data_ptr(), 0, START_BIT, s.lead, pout.data_ptr(), n, None, 0,
                            HZ_POS_LIMIT - 8 * n - 1, 0, t) == 0     # n / 2 == 0: nothing to launch
    assert lib.hz_decode_range(h, p, n, HZ_POS_LIMIT // 8 - n - 1, t, s.nsym, 7, 0, o, 0) == 0      # sym_count 0
    assert lib.hz_decode_indexless_seek(h, p, n, START_BIT, 0, None, None, 0, HZ_POS_LIMIT - 8 * n - 1, 0, t) == 0


def _main_wide():
    import torch
    from huffman_amd import load
    from huffman_amd.pipeline import StreamCodec
    from test_gpu_designed_streams import _stream
    assert os.environ.get("HZ_CHAIN_MIN_BITS") == "131072"
    c = StreamCodec(0)
    bk = book("fib57")
    nsym = 40 * BLK + 777
    sym = _stream(bk, "longest", nsym, np.random.default_rng(57))
    m = ref_stream.model(sym, bk.ln, bk.code, 45, _lead(45))
    assert (m.end_bit - 45) // 131072 >= 16          # at least 16 chains of that length
    nb = ref_stream.nblocks(nsym)
    s = SimpleNamespace(nsym=nsym, nb=nb, start=m.start)
    c.dev.upload(bk.cb)
    pay = torch.zeros(m.payload.size + 64, dtype=torch.uint8, device="cuda")
    pay[:m.payload.size] = torch.from_numpy(m.payload).cuda()
    mid = int(m.start[nb // 2])
    cases = [(0, 0)] + [(T - mid, b0) for T, b0 in zip(T_BITS, [0] + B0S)] + \
            [((1 << 37) + 12345, B0S[0]), ((1 << 48) + 8, B0S[1])]
    for bit_base, b0 in cases:                        # (0, 0) first: the near call equals the model
        buf, tab = _far_table(s, None, b0)
        end = torch.zeros(8, dtype=torch.uint8, device="cuda")
        c.dev.decode_indexless_seek(pay.data_ptr(), m.payload.size, 45, nsym, None, tab.data_ptr(), end.data_ptr(),
                                    sym_base=BLK * b0, bit_base=bit_base, stream_nsym=BLK * b0 + nsym)
        c.sync()
        _table_is(buf, b0, m.start + np.uint64(bit_base), "wide bit_base=%d b0=%d" % (bit_base, b0))
        assert int(_u64(end)[0]) == m.end_bit
        st = (ctypes.c_uint64 * 4)()
        assert load().hz_debug_seek_stats(c.dev.h, st) == 0
        assert int(st[2]) >= 10, list(st)            # entries found through the delta rebuild


if __name__ == "__main__":
    assert sys.argv[1:] == ["wide"], sys.argv
    _main_wide()
    print("ok")
