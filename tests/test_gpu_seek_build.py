"""The seek table as a by-product of the index-less walk: hz_seek_build, hz_decode_indexless_seek (with
an output and table only, whole streams and windows placed by hand) and hz_indexless_seek (parts),
against hz_pack's start[] (index[:nb + 1]) or the host model (tests/ref_stream.py). Every comparison
is exact, u64 for u64; decoded bytes and tables land between guards of 0xA5.

Run as a script it builds one table and prints "ok", in a fresh process for the test hooks the library
reads once: `nolead` (HZ_SEG_LEAD=0, a Zipf stream whose chains get heads) and `wide`
(HZ_CHAIN_MIN_BITS=131072, fib57 `longest`: chains whose decode blocks span more than 65 536 bits).
The rare paths of k_chain_seek are pinned by its own counters (hz_debug_seek_stats), not by arithmetic
about the chain geometry alone.

Tolerance: none -- every check is bit-exact."""
import ctypes
import os
import subprocess
import sys
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

BLK = 2048
GUARD = 64
ONES = (1 << 64) - 1
UNKNOWN_ENTRY = ONES
WAVES = 40 * BLK + 777


@pytest.fixture(scope="module")
def codec(built_lib):
    from huffman_amd.pipeline import StreamCodec
    return StreamCodec(0)


def _encode(codec, x):
    """Encode a device tensor once: the stream and pack's start[] on the host (u64)."""
    nsym = x.numel() // 2
    plan, payload, index = codec.encode(x)
    codec.sync()
    nb = (nsym + BLK - 1) // BLK
    start = index[:nb + 1].cpu().numpy().view(np.uint64).copy()
    return SimpleNamespace(x=x, nsym=nsym, nb=nb, plan=plan, payload=payload, start=start, start_bit=plan.start_bit)


def _zipf(codec, nsym, seed=7):
    import torch
    x = torch.empty(2 * nsym, dtype=torch.uint8, device="cuda")
    codec.dev.generate(x.data_ptr(), 2 * nsym, offset=0, kind=1, alpha=1.1, seed=seed)
    return _encode(codec, x)


def _guarded(nbytes):
    """nbytes (from a 16-byte aligned address) between two 64-byte guards, all 0xA5."""
    import torch
    buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0
    return buf, buf[GUARD:GUARD + nbytes]


def _guards_intact(buf, nbytes):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all())


def _u64(t):
    return t.cpu().numpy().view(np.uint64).copy()


def _same(got, want):
    """Two u64 arrays, exactly; the first difference in the message."""
    got, want = np.asarray(got, np.uint64), np.asarray(want, np.uint64)
    assert got.size == want.size, (got.size, want.size)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "entry %d = %d, expected %d (%d differ)" % (bad[0], got[bad[0]], want[bad[0]], bad.size)


def _stats(codec):
    """The last k_chain_seek's counters: entries found (in a head, past the record capacity, through the
    delta rebuild of record positions, in a chain that has a head)."""
    from huffman_amd import load
    out = (ctypes.c_uint64 * 4)()
    assert load().hz_debug_seek_stats(codec.dev.h, out) == 0
    return SimpleNamespace(head=int(out[0]), past_cap=int(out[1]), wide=int(out[2]), headed_chain=int(out[3]))


def _seek_build(codec, payload, nbytes, start_bit, nsym):
    """hz_seek_build into a guarded table; returns its entries (u64, host)."""
    nb = (nsym + BLK - 1) // BLK
    tbuf, tab = _guarded(8 * (nb + 1))
    codec.dev.seek_build(payload.data_ptr(), nbytes, start_bit, nsym, tab.data_ptr())
    codec.sync()
    assert _guards_intact(tbuf, 8 * (nb + 1))
    return _u64(tab)


def _with_output(codec, s, table_only):
    """hz_decode_indexless_seek over the whole stream: (table, end bit, output equal to the input)."""
    import torch
    tbuf, tab = _guarded(8 * (s.nb + 1))
    obuf, out = _guarded(2 * s.nsym)
    end = torch.full((8,), 0xA5, dtype=torch.uint8, device="cuda")
    codec.dev.decode_indexless_seek(s.payload.data_ptr(), s.payload.numel(), s.start_bit, s.nsym,
                                    None if table_only else out.data_ptr(), tab.data_ptr(), end.data_ptr())
    codec.sync()
    assert _guards_intact(tbuf, 8 * (s.nb + 1)) and _guards_intact(obuf, 2 * s.nsym)
    if table_only:
        assert bool((out == 0xA5).all())     # no output buffer was passed: nothing decoded anywhere
    return _u64(tab), int(_u64(end)[0]), table_only or bool(torch.equal(out, s.x[:2 * s.nsym]))


# ---- 1. edges, Zipf generator --------------------------------------------------------------------
@pytest.mark.parametrize("nsym", [1, 7, 2047, 2048, 2049, 5 * BLK + 3])
def test_edges_zipf(codec, nsym):
    """Sizes around a block (1 and 7: payloads under 16 bytes, the one-thread path): hz_seek_build and
    hz_decode_indexless_seek, with an output and table only, equal pack's table; the output equals the
    input and the end bit equals start[nb]."""
    s = _zipf(codec, nsym, seed=nsym % 97)
    codec.upload_decode(s.plan)
    if nsym <= 7:
        assert (int(s.start[-1]) + 7) // 8 < 16
    _same(_seek_build(codec, s.payload, s.payload.numel(), s.start_bit, nsym), s.start)
    for table_only in (False, True):
        tab, end, ok = _with_output(codec, s, table_only)
        _same(tab, s.start)
        assert end == int(s.start[-1]), (table_only, end, int(s.start[-1]))
        assert ok


# ---- 2. designed books -----------------------------------------------------------------------------
DESIGNED = [("fib57", "longest"), ("hot25", "uniform"), ("dense16", "uniform"), ("fixed16", "uniform")]
DESIGNED_CASES = [(b, k, n, sb) for b, k in DESIGNED for n in (3 * BLK + 5, WAVES) for sb in (5, 45)] + \
                 [("zipf21", "sweep", 2 * 65536 + 5, 5), ("zipf21", "sweep", 2 * 65536 + 5, 45)]


@pytest.mark.parametrize("case", DESIGNED_CASES, ids=lambda c: "%s-%s-%d-s%d" % c)
def test_designed_books(codec, case):
    """Foreign codebooks on streams drawn by design: fib57 `longest` (stream blocks past 65 536 bits, DEEP
    escapes, the serial record decoder; its CHAINS are a few thousand bits here, so the delta rebuild of
    record positions is test_wide_chain_blocks' business), hot25, dense16 (DENSE: the chain LUT), fixed16 (arithmetic) and
    the full alphabet of zipf21. The table, from hz_seek_build and beside a decode, equals the model's
    start[]."""
    import torch
    import ref_stream
    from table_books import book
    from test_gpu_designed_streams import _lead, _stream
    b, kind, nsym, start_bit = case
    bk = book(b)
    rng = np.random.default_rng(zlib.crc32(("seek-%s-%s-%d-%d" % case).encode()))
    sym = _stream(bk, kind, nsym, rng)
    m = ref_stream.model(sym, bk.ln, bk.code, start_bit, _lead(start_bit))
    if b == "fib57":
        assert int(np.diff(m.start.astype(np.int64))[0]) >= 65536
    codec.dev.upload(bk.cb)
    pbuf, pay = _guarded(m.payload.size)
    pay.copy_(torch.from_numpy(m.payload))
    _same(_seek_build(codec, pay, m.payload.size, start_bit, nsym), m.start)
    nb = ref_stream.nblocks(nsym)
    tbuf, tab = _guarded(8 * (nb + 1))
    obuf, out = _guarded(2 * nsym)
    end = torch.full((8,), 0xA5, dtype=torch.uint8, device="cuda")
    codec.dev.decode_indexless_seek(pay.data_ptr(), m.payload.size, start_bit, nsym, out.data_ptr(), tab.data_ptr(),
                                    end.data_ptr())
    codec.sync()
    _same(_u64(tab), m.start)
    assert int(_u64(end)[0]) == m.end_bit
    assert torch.equal(out.cpu(), torch.from_numpy(sym.view(np.uint8).copy()))
    assert _guards_intact(tbuf, 8 * (nb + 1)) and _guards_intact(obuf, 2 * nsym) and _guards_intact(pbuf, m.payload.size)


# ---- 3. the fix-up path ------------------------------------------------------------------------------
def test_fixups_without_lead_in(built_lib):
    """HZ_SEG_LEAD=0 (test hook, read once: a fresh process): no lead-in, so nearly every one of the about
    40 one-block chains of a Zipf stream of 40 * 2048 + 777 symbols starts unsynchronised and gets a head
    from k_chain_fix; entries inside heads are walked from the chain's true entry. Table equals pack's."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "nolead"], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, HZ_SEG_LEAD="0"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_entries_inside_heads(codec):
    """tri36 (seven 3-bit and eight 6-bit codes) never resynchronises off phase, and a chain's lead-in
    starts on the codewords' phase one time in three: most chains never meet one of their own records and
    are head from end to end, so the entries inside them are walked from the chain's true entry (the
    counter says how many). Table equals the model's."""
    import torch
    import ref_stream
    from test_ranges_model import tri36_stream
    cb, ln, code, sym = tri36_stream(WAVES)
    m = ref_stream.model(sym, ln, code, 0, 0)
    codec.dev.upload_decode(cb)
    pbuf, pay = _guarded(m.payload.size)
    pay.copy_(torch.from_numpy(m.payload))
    _same(_seek_build(codec, pay, m.payload.size, 0, WAVES), m.start)
    st = _stats(codec)
    assert st.head >= 5 and st.headed_chain >= st.head, vars(st)


def test_wide_chain_blocks(built_lib):
    """HZ_CHAIN_MIN_BITS=131072 (test hook, read once: a fresh process) makes every chain at least
    131 072 bits long. Under fib57 `longest` (codes of 50 bits and more) such a chain holds about 2 400
    codewords, 300 records: its first decode block (256 records, 2048 codewords) spans more than
    100 000 bits, so chain_rec_pos is inexact there and k_chain_seek rebuilds record positions from the
    record deltas (the counter says for how many entries). Table only: the decoders of such chains'
    records are not this test's. Table equals the model's start[]."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "wide"], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, HZ_CHAIN_MIN_BITS="131072"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ---- 4. records past the capacity -----------------------------------------------------------------
def test_records_past_capacity(codec):
    """nsym = 2^20, symbols uniform in 1..32768 (15-16 bit codes) with a contiguous 20 % run of symbol 0
    (about 2 bits): 0.8 * 15.1 + 0.2 * 2 = about 12.5 bits per codeword. The payload (13 Mbit) is far
    below one decode block per walk lane, so chain_geom takes chains of one expected block,
    2048 * 12.5 = 25 600 bits (about 512 chains), with a capacity of 25 600 / 12.5 / 8 * 1.25 + 64 = 384
    -> 512 records (2 decode blocks). A chain inside the run holds 25 600 / 2.3 = about 11 000
    codewords, about 1 390 records: entries there lie past the capacity and are walked from the chain's
    last checkpoint. Table equals pack's."""
    import torch
    rng = np.random.default_rng(11)
    nsym = 1 << 20
    sym = rng.integers(1, 32769, nsym).astype("<u2")
    sym[nsym // 3: nsym // 3 + nsym // 5] = 0
    s = _encode(codec, torch.from_numpy(sym.view(np.uint8).copy()).cuda())
    codec.upload_decode(s.plan)
    bits = np.diff(s.start.astype(np.int64))
    assert int(bits.min()) < 2048 * 3 and int(np.median(bits)) > 2048 * 14   # the run's blocks and the others
    _same(_seek_build(codec, s.payload, s.payload.numel(), s.start_bit, nsym), s.start)
    st = _stats(codec)
    assert st.past_cap >= 10, vars(st)       # the run is 100 blocks: many entries lie past a chain's capacity
    tab, end, ok = _with_output(codec, s, table_only=False)
    _same(tab, s.start)
    assert ok and end == int(s.start[-1])


# ---- 5. windows by hand ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ten(codec):
    return _zipf(codec, 10 * BLK + 333, seed=21)


@pytest.mark.parametrize("table_only", [False, True])
def test_two_windows(codec, ten, table_only):
    """One stream in two hz_decode_indexless_seek calls split at symbol 3 * 2048 + 100 (no entry at the
    split): the second call starts at the byte of the first call's end bit, with bit_base = 8 * (end // 8)
    and sym_base at the split. The one device table equals pack's; with outputs the halves equal the input."""
    import torch
    s = ten
    codec.upload_decode(s.plan)
    split = 3 * BLK + 100
    nbytes = s.payload.numel()
    tbuf, tab = _guarded(8 * (s.nb + 1))
    o1buf, o1 = _guarded(2 * split)
    o2buf, o2 = _guarded(2 * (s.nsym - split))
    end = torch.full((8,), 0xA5, dtype=torch.uint8, device="cuda")
    codec.dev.decode_indexless_seek(s.payload.data_ptr(), nbytes, s.start_bit, split,
                                    None if table_only else o1.data_ptr(), tab.data_ptr(), end.data_ptr(),
                                    sym_base=0, bit_base=0, stream_nsym=s.nsym)
    codec.sync()
    e1 = int(_u64(end)[0])
    assert s.start[3] < e1 < s.start[4]
    assert _u64(tab)[4] == 0xA5A5A5A5A5A5A5A5       # entries past the call's codewords are not written
    byte = e1 // 8
    codec.dev.decode_indexless_seek(s.payload.data_ptr() + byte, nbytes - byte, e1 % 8, s.nsym - split,
                                    None if table_only else o2.data_ptr(), tab.data_ptr(), end.data_ptr(),
                                    sym_base=split, bit_base=8 * byte, stream_nsym=s.nsym)
    codec.sync()
    _same(_u64(tab), s.start)
    assert int(_u64(end)[0]) + 8 * byte == int(s.start[-1])
    assert _guards_intact(tbuf, 8 * (s.nb + 1)) and _guards_intact(o1buf, 2 * split)
    assert _guards_intact(o2buf, 2 * (s.nsym - split))
    if table_only:
        assert bool((o1 == 0xA5).all()) and bool((o2 == 0xA5).all())
    else:
        assert torch.equal(o1, s.x[:2 * split]) and torch.equal(o2, s.x[2 * split:2 * s.nsym])


# ---- 6. parts ------------------------------------------------------------------------------------------
def test_parts_in_one_context(codec, ten):
    """hz_indexless_scan over three bit parts of one stream in one context (refixed where a part's walked
    entry is not the previous part's exit), hz_indexless_seek with the prefix of the counts: the union of
    the parts' entries is pack's table, and a boundary entry two parts share gets equal values."""
    import torch
    s = ten
    codec.upload_decode(s.plan)
    dev = codec.dev
    P = int(s.start[-1]) - s.start_bit
    bounds = [0, P // 3 + 5, 2 * P // 3 + 1, P]
    tbuf, tab = _guarded(8 * (s.nb + 1))
    summ = torch.zeros(32, dtype=torch.uint8, device="cuda")
    first, entry = 0, s.start_bit
    for pb, pe in zip(bounds, bounds[1:]):
        dev.indexless_scan(s.payload.data_ptr(), s.payload.numel(), s.start_bit, pb, pe, UNKNOWN_ENTRY, summ.data_ptr(),
                           nsym=s.nsym)
        codec.sync()
        cnt, xit, ent = (int(v) for v in _u64(summ)[:3])
        if ent != entry:
            dev.indexless_refix(entry, summ.data_ptr())
            codec.sync()
            cnt, xit, ent = (int(v) for v in _u64(summ)[:3])
        assert ent == entry
        dev.indexless_seek(first, cnt, s.nsym, tab.data_ptr())
        codec.sync()
        got = _u64(tab)
        lo, hi = -(-first // BLK), (first + cnt) // BLK if first + cnt < s.nsym else s.nb
        _same(got[lo:hi + 1], s.start[lo:hi + 1])          # this part's entries, as soon as it wrote them
        first += cnt
        entry = xit
    assert first == s.nsym and entry == int(s.start[-1])
    _same(_u64(tab), s.start)
    assert _guards_intact(tbuf, 8 * (s.nb + 1))


# ---- 7. a short payload ----------------------------------------------------------------------------------
def test_short_payload(codec, ten):
    """The payload cut to half: the entries of codewords that start inside it are right, every later entry
    and the end are all ones (as hz_index_build leaves start[nblocks])."""
    import torch
    s = ten
    codec.upload_decode(s.plan)
    cut = s.payload.numel() // 2
    inside = s.start < 8 * cut
    assert 2 <= int(inside.sum()) <= s.nb - 2 and not bool((s.start == 8 * cut).any())
    want = np.where(inside, s.start, np.uint64(ONES))
    _same(_seek_build(codec, s.payload, cut, s.start_bit, s.nsym), want)
    tbuf, tab = _guarded(8 * (s.nb + 1))
    end = torch.zeros(8, dtype=torch.uint8, device="cuda")
    codec.dev.decode_indexless_seek(s.payload.data_ptr(), cut, s.start_bit, s.nsym, None, tab.data_ptr(), end.data_ptr())
    codec.sync()
    _same(_u64(tab), want)
    assert int(_u64(end)[0]) == ONES and _guards_intact(tbuf, 8 * (s.nb + 1))


def _cut_at_entry(codec, bname, nsym):
    """A designed stream at start bit 0, cut exactly where one of its blocks starts (an entry on a byte
    boundary): (model, payload tensor, entry number, cut bytes)."""
    import torch
    import ref_stream
    from table_books import book
    from test_gpu_designed_streams import _stream
    bk = book(bname)
    sym = _stream(bk, "uniform", nsym, np.random.default_rng(zlib.crc32(("cut-" + bname).encode())))
    m = ref_stream.model(sym, bk.ln, bk.code, 0, 0)
    nb = ref_stream.nblocks(nsym)
    hits = [b for b in range(2, nb) if int(m.start[b]) % 8 == 0]
    assert hits, "no block of the stream starts on a byte"
    codec.dev.upload(bk.cb)
    pay = torch.from_numpy(m.payload).cuda()
    return m, pay, hits[0], int(m.start[hits[0]]) // 8


@pytest.mark.parametrize("bname", ["hot25", "fixed16"])
def test_codeword_at_the_payload_end(codec, bname):
    """The payload cut exactly at the first bit of block b's first codeword: that codeword has no bit in the
    payload, so entry b is all ones like every later one (the chain path and the arithmetic FIXED16 one).
    Cut there with nsym = 2048 b, the same position is the call's END and is reported: entry b and
    *d_end_bit equal start[b]."""
    import torch
    m, pay, b, cut = _cut_at_entry(codec, bname, WAVES)
    want = m.start.copy()
    want[b:] = np.uint64(ONES)
    _same(_seek_build(codec, pay, cut, 0, WAVES), want)
    tbuf, tab = _guarded(8 * (b + 1))
    end = torch.zeros(8, dtype=torch.uint8, device="cuda")
    codec.dev.decode_indexless_seek(pay.data_ptr(), cut, 0, BLK * b, None, tab.data_ptr(), end.data_ptr())
    codec.sync()
    _same(_u64(tab), m.start[:b + 1])
    assert int(_u64(end)[0]) == int(m.start[b]) == 8 * cut and _guards_intact(tbuf, 8 * (b + 1))


# ---- 8. graph capture ---------------------------------------------------------------------------------
def test_seek_build_graph_capture(codec, ten):
    """hz_seek_build is stream-ordered: captured after an eager first call (scratch and tables in place),
    the table cleared, it is replayed twice and rebuilds the table each time."""
    import torch
    s = ten
    codec.upload_decode(s.plan)
    tab = torch.zeros(s.nb + 1, dtype=torch.int64, device="cuda")

    def call():
        codec.dev.seek_build(s.payload.data_ptr(), s.payload.numel(), s.start_bit, s.nsym, tab.data_ptr())

    call()
    codec.sync()
    _same(_u64(tab), s.start)
    tab.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=codec.stream):
        call()
    torch.cuda.synchronize()
    for _ in range(2):
        tab.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _same(_u64(tab), s.start)


def _main_nolead(c):
    assert os.environ.get("HZ_SEG_LEAD") == "0"
    s = _zipf(c, WAVES, seed=5)
    c.upload_decode(s.plan)
    _same(_seek_build(c, s.payload, s.payload.numel(), s.start_bit, s.nsym), s.start)
    st = _stats(c)
    print("stats", vars(st))
    assert st.headed_chain >= 20, vars(st)     # nearly every entry lies in a chain that got a head
    tab, end, ok = _with_output(c, s, table_only=False)
    _same(tab, s.start)
    assert ok and end == int(s.start[-1])


def _main_wide(c):
    import torch
    import ref_stream
    from table_books import book
    from test_gpu_designed_streams import _lead, _stream
    assert os.environ.get("HZ_CHAIN_MIN_BITS") == "131072"
    bk = book("fib57")
    sym = _stream(bk, "longest", WAVES, np.random.default_rng(57))
    m = ref_stream.model(sym, bk.ln, bk.code, 45, _lead(45))
    assert (m.end_bit - 45) // 131072 >= 16     # at least 16 chains of that length
    c.dev.upload(bk.cb)
    pbuf, pay = _guarded(m.payload.size)
    pay.copy_(torch.from_numpy(m.payload))
    _same(_seek_build(c, pay, m.payload.size, 45, WAVES), m.start)
    st = _stats(c)
    print("stats", vars(st))
    assert st.wide >= 10, vars(st)
    assert _guards_intact(pbuf, m.payload.size)


if __name__ == "__main__":
    assert sys.argv[1:] in (["nolead"], ["wide"]), sys.argv
    from huffman_amd.pipeline import StreamCodec
    (_main_nolead if sys.argv[1] == "nolead" else _main_wide)(StreamCodec(0))
    print("ok")
