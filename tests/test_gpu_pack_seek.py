"""hz_pack_seek: the seek table as a by-product of the pack (include/huffman_amd.h "the seek table from
the writer"). Every table is compared with the plain host model (tests/ref_stream.py) and with the first
words of the block index hz_pack writes for the same arguments; every payload with hz_pack's; the table
sits between guard words, so a stray max_bits or sub[] store shows. Covered: the four encode modes and
U = 1, the size edges around a block, unaligned start bits with lead bits, blocks that leave k_pack_write
for k_pack_cold or its direct path, one table filled by three calls as the streaming archive fills it, the
rejections, the range plan at its smallest size, a decode from the table, and graph capture.

Tolerance: none -- every check is bit-exact."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_stream  # noqa: E402
from table_books import book  # noqa: E402

pytestmark = pytest.mark.gpu

BLK = 2048
GUARD = 64
HZ_EINVAL = -1
BOOKS = ["fixed16", "dense12", "dense16", "hot25", "fib41", "fib57", "one", "zipf21"]
SIZES = [1, 2047, 2048, 2049, 3 * BLK, 5 * BLK + 7]
START_BITS = [0, 5, 37]
SENTINEL = 0x5A5A5A5A5A5A5A5A
PACK_SLOT_BITS = 1024 * 32   # the largest LDS output slot of a pack wave (kPackCopyIters x 64 words)


@pytest.fixture(scope="module")
def codec(built_lib):
    from huffman_amd.pipeline import StreamCodec
    return StreamCodec(0)


def _lead(start_bit):
    k = start_bit % 32
    return ((0x15a5f3c7 & ((1 << k) - 1)) | 1) if k else 0


def _draw(bk, nsym, seed, longest=False):
    """u16 symbols drawn uniformly from the book's alphabet (longest: from its longest codes alone)."""
    rng = np.random.default_rng(seed)
    alphabet = np.nonzero(bk.ln)[0].astype(np.uint16)
    if longest:
        alphabet = alphabet[bk.ln[alphabet] == bk.ln.max()]
    return np.ascontiguousarray(alphabet[rng.integers(0, alphabet.size, nsym)], dtype="<u2")


def _guarded(nbytes, fill=0xA5):
    import torch
    buf = torch.full((GUARD + nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + nbytes]


def _guards_intact(buf, nbytes, fill=0xA5):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + nbytes:] == fill).all())


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _both(codec, bk, sym, start_bit):
    """hz_pack with a block index and hz_pack_seek of the same arguments, each into guarded buffers:
    (model, hz_pack's payload, its index bytes, hz_pack_seek's payload, its table as u64, guards intact)."""
    from huffman_amd import index_bytes, seek_bytes
    dev = codec.dev
    nsym = sym.size
    m = ref_stream.model(sym, bk.ln, bk.code, start_bit, _lead(start_bit))
    nbytes = m.payload.size
    x = _dev(sym)
    p1buf, p1 = _guarded(nbytes)
    i1buf, i1 = _guarded(index_bytes(nsym))
    dev.pack(x.data_ptr(), x.numel(), start_bit, m.lead, p1.data_ptr(), nbytes, i1.data_ptr())
    p2buf, p2 = _guarded(nbytes)
    sbytes = seek_bytes(nsym)
    assert sbytes == 8 * (ref_stream.nblocks(nsym) + 1)
    s2buf, s2 = _guarded(sbytes)
    dev.pack_seek(x.data_ptr(), x.numel(), start_bit, m.lead, p2.data_ptr(), nbytes, s2.data_ptr())
    codec.sync()
    ok = _guards_intact(p1buf, nbytes) and _guards_intact(i1buf, index_bytes(nsym)) and _guards_intact(p2buf, nbytes)
    return m, p1.cpu().numpy(), i1.cpu().numpy(), p2.cpu().numpy(), _u64(s2), ok and _guards_intact(s2buf, sbytes)


def _check(codec, bk, sym, start_bit, what):
    m, pay, idx, pay_seek, table, guards = _both(codec, bk, sym, start_bit)
    first = 4 * (start_bit // 32)
    assert np.array_equal(table, m.start), (what, "table differs from the model", table[:4], m.start[:4])
    assert np.array_equal(table.view(np.uint8), idx[:table.size * 8]), (what, "table differs from hz_pack's index words")
    assert np.array_equal(idx, m.index), (what, "hz_pack's index differs from the model")
    assert np.array_equal(pay_seek, pay), (what, "payload differs from hz_pack's")
    assert np.array_equal(pay[first:], m.payload[first:]), (what, "payload differs from the model")
    assert guards, (what, "a guard word was written")
    return m


# ---- 1. every mode, the size edges, the start bits ------------------------------------------------
@pytest.mark.parametrize("start_bit", START_BITS)
@pytest.mark.parametrize("name", BOOKS)
def test_table_and_payload(codec, name, start_bit):
    bk = book(name)
    codec.dev.upload(bk.cb)
    for nsym in SIZES:
        what = f"{name}-{nsym}-s{start_bit}"
        _check(codec, bk, _draw(bk, nsym, zlib.crc32(what.encode())), start_bit, what)


# ---- 2. blocks that leave the wave's LDS slot ---------------------------------------------------------
@pytest.mark.parametrize("name", ["hot25", "fib57"])
def test_cold_blocks(codec, name):
    """Blocks of the longest code alone: 2048 x 25 bits under hot25 (past the wave's LDS slot: k_pack_cold),
    2048 x 56 bits under fib57 (past 65 536 bits: the WIDE kernel's direct path)."""
    bk = book(name)
    codec.dev.upload(bk.cb)
    sym = _draw(bk, 3 * BLK + 5, 7, longest=True)
    m = _check(codec, bk, sym, 5, name)
    blocks = np.diff(m.start.astype(np.int64))
    assert int(blocks[:3].min()) > (65536 if name == "fib57" else PACK_SLOT_BITS)


# ---- 3. placement: three calls fill one table -----------------------------------------------------------
@pytest.mark.parametrize("name", ["zipf21", "dense12", "fib41", "fixed16"])
def test_three_calls_one_table(codec, name):
    """A 5 x 2048 + 7 symbol stream packed in calls of 2, 2 and 1 + 7 blocks, start bit, lead bits and output
    position carried as the streaming archive carries them, bit_base = 8 x the bytes already emitted."""
    import torch
    from huffman_amd import seek_bytes
    bk = book(name)
    dev = codec.dev
    dev.upload(bk.cb)
    nsym = 5 * BLK + 7
    sym = _draw(bk, nsym, 11)
    start_bit = 5
    m = _check(codec, bk, sym, start_bit, name)
    nb = ref_stream.nblocks(nsym)
    x = _dev(sym)
    nbytes = m.payload.size
    pbuf, pay = _guarded(nbytes + 8)
    tbuf, tab = _guarded(seek_bytes(nsym))
    tab.view(torch.int64).fill_(SENTINEL)
    expect = np.full(nb + 1, SENTINEL, dtype=np.uint64)
    sbit, lead, emitted, done = start_bit, m.lead, 0, 0
    for count in (2 * BLK, 2 * BLK, BLK + 7):
        b0, last = done // BLK, done + count == nsym
        out = pay[emitted:]
        dev.pack_seek(x[2 * done:].data_ptr(), 2 * count, sbit, lead, out.data_ptr(), out.numel(), tab.data_ptr(),
                      None, done, 8 * emitted, nsym)
        codec.sync()
        got = _u64(tab)
        hi = nb if last else b0 + count // BLK
        expect[b0:hi + 1] = m.start[b0:hi + 1]
        assert np.array_equal(got, expect), (name, done, got, expect)   # the window's entries, nothing else
        end_bit = int(got[hi]) - 8 * emitted          # the call's end, from the table
        nbyte = (end_bit + 7) // 8 if last else end_bit // 32 * 4
        sbit, lead = end_bit % 32, 0
        if sbit and not last:                         # the partial word travels as the next call's lead bits
            w = int.from_bytes(out[nbyte:nbyte + 4].cpu().numpy().tobytes(), "big")
            lead = w >> (32 - sbit)
        emitted += nbyte
        done += count
    assert emitted == (m.end_bit + 7) // 8
    assert np.array_equal(pay[:emitted].cpu().numpy(), m.payload[:emitted])
    assert _guards_intact(pbuf, nbytes + 8) and _guards_intact(tbuf, seek_bytes(nsym))


# ---- 4. rejections ------------------------------------------------------------------------------------
def test_rejections(codec):
    import torch
    from huffman_amd import HZError, seek_bytes
    bk = book("zipf21")
    dev = codec.dev
    dev.upload(bk.cb)
    nsym = 3 * BLK
    x = _dev(_draw(bk, nsym, 3))
    out = torch.zeros(4 * nsym, dtype=torch.uint8, device="cuda")
    tbuf, tab = _guarded(seek_bytes(4 * nsym))
    tab.view(torch.int64).fill_(SENTINEL)

    def call(n=2 * nsym, sym_base=0, stream_nsym=4 * nsym, seek=tab.data_ptr()):
        dev.pack_seek(x.data_ptr(), n, 0, 0, out.data_ptr(), out.numel(), seek, None, sym_base, 0, stream_nsym)

    for kw in (dict(sym_base=100),                              # not a block boundary
               dict(n=2 * (BLK + 9)),                           # ragged, and not the stream's last call
               dict(sym_base=2 * BLK, stream_nsym=4 * BLK),     # sym_base + n / 2 > stream_nsym
               dict(seek=None)):                                # no table
        with pytest.raises(HZError) as e:
            call(**kw)
        assert e.value.status == HZ_EINVAL, kw
    call(n=0)                                                   # nothing to pack: HZ_OK
    call(n=1)
    codec.sync()
    assert bool((tab.view(torch.int64) == SENTINEL).all()) and _guards_intact(tbuf, seek_bytes(4 * nsym))
    call(n=2 * (BLK + 9), sym_base=BLK, stream_nsym=2 * BLK + 9)  # ragged and last: accepted
    codec.sync()
    got = _u64(tab)
    assert [int(v) != SENTINEL for v in got[:5]] == [False, True, True, True, False]


# ---- 5. the range plan, at its smallest size -------------------------------------------------------------
def test_range_plan(codec):
    """256 MiB of Zipf: hz_pack_seek takes the plan of hz_hist16_ranges like hz_pack_ranges, through
    Device.pack_seek and through StreamCodec.pack_seek's identity rule."""
    import torch
    from huffman_amd import seek_bytes
    n = 256 << 20
    dev = codec.dev
    assert dev.ranges_bytes(n) != 0 and dev.ranges_bytes(n - 64 * 4096) == 0   # 1024 ranges of 64 blocks: the fewest
    x = torch.empty(n, dtype=torch.uint8, device="cuda")
    dev.generate(x.data_ptr(), n, offset=0, kind=1, alpha=1.1, seed=42)
    plan, payload, index = codec.encode(x)          # hist16_ranges, then pack_ranges with the block index
    codec.sync()
    assert dev.last_pack_ranges() == 1
    nsym = n // 2
    nb = nsym // BLK
    words = seek_bytes(nsym) // 8
    assert words == nb + 1
    nbytes = plan.words * 4
    for through_codec in (False, True):
        out = torch.full_like(payload, 0xA5)
        tbuf, tab = _guarded(8 * words)
        if through_codec:
            codec.histogram(x)
            codec.pack_seek(x, plan, out, tab.view(torch.int64))
        else:
            dev.pack_seek(x.data_ptr(), n, plan.start_bit, plan.lead, out.data_ptr(), out.numel(), tab.data_ptr(),
                          codec.ranges.data_ptr())
        codec.sync()
        assert dev.last_pack_ranges() == 1
        assert torch.equal(tab.view(torch.int64), index[:words])
        assert torch.equal(out[:nbytes], payload[:nbytes])
        assert _guards_intact(tbuf, 8 * words)
    # without a plan (its identity is used once): the same table from count + scan + write
    tbuf, tab = _guarded(8 * words)
    codec.pack_seek(x, plan, out, tab.view(torch.int64))
    codec.sync()
    assert dev.last_pack_ranges() == 0
    assert torch.equal(tab.view(torch.int64), index[:words]) and torch.equal(out[:nbytes], payload[:nbytes])
    assert _guards_intact(tbuf, 8 * words)


# ---- 6. round trip: ranges decoded from the writer's table ------------------------------------------------
def test_decode_ranges_from_the_table(codec):
    import torch
    from huffman_amd import seek_bytes
    bk = book("zipf21")
    dev = codec.dev
    dev.upload(bk.cb)
    nsym = 5 * BLK + 7
    sym = _draw(bk, nsym, 21)
    m = ref_stream.model(sym, bk.ln, bk.code, 5, _lead(5))
    x = _dev(sym)
    pay = torch.zeros(m.payload.size + 64, dtype=torch.uint8, device="cuda")
    tab = torch.zeros(seek_bytes(nsym) // 8, dtype=torch.int64, device="cuda")
    dev.pack_seek(x.data_ptr(), x.numel(), 5, m.lead, pay.data_ptr(), m.payload.size, tab.data_ptr())
    rows, want, at = [], [], 0
    for begin, count in ((BLK - 3, 10), (2 * BLK - 1, BLK + 2), (4 * BLK + 1000, BLK + 7 - 1000)):
        rows.append([begin, count, at])
        want.append(x[2 * begin:2 * (begin + count)])
        at += 2 * count
    rg = torch.tensor(rows, dtype=torch.int64, device="cuda")
    out = torch.zeros(at, dtype=torch.uint8, device="cuda")
    codec.decode_ranges(pay, nsym, tab, rg, out, full_index=False)
    codec.sync()
    assert torch.equal(out, torch.cat(want))


# ---- 7. graph capture ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zipf21", "fixed16"])
def test_graph_capture(codec, name):
    """Stream-ordered: captured after an eager call (scratch and kernel attributes in place), replayed on a
    second input of the same length."""
    import torch
    from huffman_amd import seek_bytes
    bk = book(name)
    dev = codec.dev
    dev.upload(bk.cb)
    nsym = 5 * BLK + 7
    a, b = _draw(bk, nsym, 31), _draw(bk, nsym, 32)
    ma = ref_stream.model(a, bk.ln, bk.code, 5, _lead(5))
    mb = ref_stream.model(b, bk.ln, bk.code, 5, _lead(5))
    cap = max(ma.payload.size, mb.payload.size)
    x = _dev(a)
    pay = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    tab = torch.zeros(seek_bytes(nsym) // 8, dtype=torch.int64, device="cuda")

    def call():
        dev.pack_seek(x.data_ptr(), x.numel(), 5, ma.lead, pay.data_ptr(), cap, tab.data_ptr())

    call()
    codec.sync()
    assert np.array_equal(_u64(tab), ma.start)
    assert np.array_equal(pay[:ma.payload.size].cpu().numpy(), ma.payload)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=codec.stream):  # a host synchronisation inside would break the capture
        call()
    torch.cuda.synchronize()
    x.copy_(_dev(b))
    pay.zero_()
    tab.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    got_tab, got_pay = _u64(tab).copy(), pay.cpu().numpy().copy()
    assert np.array_equal(got_tab, mb.start)
    assert np.array_equal(got_pay[:mb.payload.size], mb.payload)
    pay.zero_()
    tab.zero_()
    call()                                          # the eager run on the second input
    codec.sync()
    assert np.array_equal(_u64(tab), got_tab) and np.array_equal(pay.cpu().numpy(), got_pay)
