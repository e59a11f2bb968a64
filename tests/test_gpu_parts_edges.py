"""The split decode's parts (hz_indexless_scan / _refix / _decode / _seek) at their edges: narrow parts,
isolated slices, and the call contract.

1. The tiling list of tests/parts_cases.py for six codebooks and two start bits, walked twice: from the
   whole payload, and from ISOLATED SLICES -- the least bytes the header asks for, copied into a buffer of
   their own between seeded random bytes, at every residue of the slice's first byte modulo 16 and of the
   pointer modulo 64. A load that leaves the view, or a bit the kernel should have read as zero, meets
   random bytes there and not the stream's. Every part's summary, symbols, end-bit word and seek entries
   equal arithmetic on the model's codeword positions (no decoder involved); outputs sit between 0xA5
   guards, tables in a sentinel.
2. The non-tiling list ([0, E) for 128 consecutive E: the last chain 1 .. 128 bits wide modulo 128) and a
   part that runs into the payload's zero padding (against ref_stream.span_decode).
3. The call contract by raw return codes: what is refused with HZ_EINVAL before anything is launched, for
   a chain codebook and FIXED16 alike, and which calls end a pending part and which leave it alone.

Every refusal here is made on the host: no case launches a kernel on arguments the library should refuse.
Tolerance: none -- every check is bit-exact."""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import parts_cases as pc  # noqa: E402
import ref_stream  # noqa: E402

pytestmark = pytest.mark.gpu

BLK = 2048
GUARD = 64
MARGIN = 128            # random bytes before and after a placed buffer, at least
ONES = (1 << 64) - 1
SENT = 0x5A5A5A5A5A5A5A5A
HZ_EINVAL = -1
HZ_EHIP = -3
CASES = [(b, s) for b in pc.BOOKS for s in pc.START_BITS]


@pytest.fixture(scope="module")
def codec(built_lib):
    from huffman_amd.pipeline import StreamCodec
    return StreamCodec(0)


@contextlib.contextmanager
def _device_errors_end_the_run():
    """A HIP runtime error: nothing more runs on this device."""
    from huffman_amd import HZError
    try:
        yield
    except HZError as e:
        if e.status == HZ_EHIP:
            pytest.exit("HIP error: %s" % e, returncode=3)
        raise


def _place(host, r64, seed):
    """Host bytes on the device at an address = r64 (mod 64), in a buffer of their own with at least MARGIN
    seeded random bytes on either side. Returns (the buffer, the view of the bytes)."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    buf = torch.randint(0, 256, (host.size + 2 * MARGIN + 64,), dtype=torch.uint8, device="cuda", generator=g)
    off = MARGIN + (r64 - (buf.data_ptr() + MARGIN)) % 64
    buf[off:off + host.size] = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    view = buf[off:off + host.size]
    assert view.data_ptr() % 64 == r64 and off >= MARGIN and buf.numel() - off - host.size >= MARGIN
    return buf, view


def _guarded(nbytes):
    import torch
    buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 16 == 0
    return buf, buf[GUARD:GUARD + nbytes]


def _u64(t):
    return [int(v) for v in t.cpu().numpy().view(np.uint64)]


def _table(nb):
    """A seek table of nb + 1 entries between eight guard words, the sentinel everywhere."""
    import torch
    buf = torch.full((8 + nb + 1 + 8,), SENT, dtype=torch.int64, device="cuda")
    return buf, buf[8:8 + nb + 1]


def _seek_expect(m, first, count):
    """The header's placement rule: entry b for every b with first <= min(2048 b, nsym) <= first + count,
    nothing for a call without codewords; the sentinel elsewhere, the guard words included."""
    nb = ref_stream.nblocks(m.nsym)
    exp = np.full(8 + nb + 1 + 8, SENT, dtype=np.uint64)
    if count:
        for b in range(nb + 1):
            if first <= min(BLK * b, m.nsym) <= first + count:
                exp[8 + b] = m.start[b]
    return exp


class Walker:
    """One context, one stream: scans a part from a view, brings it to its true entry and checks the summary,
    the decoded symbols, the end-bit word and the seek entries against the model."""

    def __init__(self, codec, bk, m):
        import torch
        self.codec, self.dev, self.bk, self.m = codec, codec.dev, bk, m
        self.nb = ref_stream.nblocks(m.nsym)
        self.max_len = int(bk.ln.max())
        self.summ = torch.zeros(4, dtype=torch.int64, device="cuda")
        self.keep, self.whole = _place(m.payload, 0, 1)
        self.tabbuf, self.tab = _table(self.nb)

    def view(self, p, k, slices):
        """(device view, payload_bit_base, what to keep alive) of part p."""
        if not slices:
            return self.whole, 0, None
        b0, b1, r64 = pc.slice_of(self.m, self.max_len, p.pb, p.pe, k)
        buf, v = _place(self.m.payload[b0:b1], r64, 100 + k)
        return v, 8 * b0, buf

    def summary(self):
        self.codec.sync()
        return tuple(_u64(self.summ)[:3])

    def scan(self, p, view, base, given, what):
        m = self.m
        self.dev.indexless_scan(view.data_ptr(), view.numel(), m.start_bit, p.pb, p.pe, given, self.summ.data_ptr(),
                                nsym=m.nsym, payload_bit_base=base)
        got = self.summary()
        if p.pb == 0 and given == ONES:
            assert got[2] == m.start_bit, (what, "the first part's walked entry", got)
        if got[2] != p.entry:
            assert given == ONES, (what, "the entry in use is not the one given", got)
            self.dev.indexless_refix(p.entry, self.summ.data_ptr())
            got = self.summary()
        assert got == (p.count, p.exit, p.entry), (what, "(count, exit, entry)", got, (p.count, p.exit, p.entry))

    def decode(self, p, what):
        """The pending part's codewords, its end-bit word and its seek entries; returns the table written."""
        import torch
        m = self.m
        rest = m.nsym - p.first                     # the stream's symbols from the part's first on
        take = min(p.count, rest)
        obuf, _ = _guarded(2 * take)
        d_out = obuf.data_ptr() + GUARD             # (an empty view has no pointer of its own)
        end = torch.full((1,), 0x2525252525252525, dtype=torch.int64, device="cuda")
        if take == 0:                               # nothing asked for: HZ_OK, nothing written
            self.dev.indexless_decode(0, d_out, end.data_ptr())
            self.codec.sync()
            assert bool((obuf == 0xA5).all()) and _u64(end)[0] == ONES, (what, "decode of 0 symbols")
        self.dev.indexless_decode(rest, d_out, end.data_ptr())
        self.tabbuf.fill_(SENT)
        self.dev.indexless_seek(p.first, take, m.nsym, self.tab.data_ptr())
        self.codec.sync()
        got = obuf.cpu().numpy()
        assert bool((got[:GUARD] == 0xA5).all()) and bool((got[GUARD + 2 * take:] == 0xA5).all()), (what, "guards")
        sym = got[GUARD:GUARD + 2 * take].view("<u2")
        assert np.array_equal(sym, p.sym[:take]), (what, "symbols", int(np.argmax(sym != p.sym[:take])))
        last = take > 0 and p.first + take == m.nsym
        assert _u64(end)[0] == (m.end_bit if last else ONES), (what, "end-bit word", _u64(end)[0], last)
        tab = self.tabbuf.cpu().numpy().view(np.uint64)
        exp = _seek_expect(m, p.first, take)
        assert np.array_equal(tab, exp), (what, "seek entries", np.nonzero(tab != exp)[0][:4].tolist())
        return sym, tab[8:8 + self.nb + 1]


# ---- 1. the tiling list, from the whole payload and from isolated slices -------------------------------------
@pytest.mark.parametrize("form", ["whole", "slices"])
@pytest.mark.parametrize("name,start_bit", CASES, ids=lambda v: str(v))
def test_tiling_parts(codec, name, start_bit, form):
    bk, m = pc.stream(name, start_bit)
    parts = pc.tiling_parts(bk, m)
    with _device_errors_end_the_run():
        codec.dev.upload(bk.cb)
        w = Walker(codec, bk, m)
        out = np.zeros(m.nsym, dtype="<u2")
        union = np.full(w.nb + 1, SENT, dtype=np.uint64)
        for k, p in enumerate(parts):
            what = "%s s%d %s part %d [%d, %d)" % (name, start_bit, form, k, p.pb, p.pe)
            view, base, keep = w.view(p, k, form == "slices")
            # every third part is handed its true entry; the others walk theirs (part 0 among them)
            w.scan(p, view, base, p.entry if pc.entry_given(k) else ONES, what)
            sym, tab = w.decode(p, what)
            out[p.first:p.first + p.count] = sym
            wrote = tab != np.uint64(SENT)
            both = wrote & (union != np.uint64(SENT))
            assert np.array_equal(union[both], tab[both]), (what, "a shared boundary entry differs")
            union[wrote] = tab[wrote]
            del keep
        codec.sync()                                   # no status pending after the walk
    assert np.array_equal(out, m.sym)
    assert np.array_equal(union, m.start)


# ---- 2. the last chain's width; the zero padding -----------------------------------------------------------------
@pytest.mark.parametrize("name", pc.BOOKS)
def test_last_chain_widths(codec, name):
    """[0, E) for 128 consecutive E up to one bit below the end bit, whole payload, known entry: the summary
    of every one, decode and output of three of them."""
    start_bit = pc.START_BITS[pc.BOOKS.index(name) % 2]
    bk, m = pc.stream(name, start_bit, pc.WAVES)
    parts = pc.last_width_parts(m)
    with _device_errors_end_the_run():
        codec.dev.upload(bk.cb)
        w = Walker(codec, bk, m)
        for k, p in enumerate(parts):
            what = "%s s%d [0, %d)" % (name, start_bit, p.pe)
            w.scan(p, w.whole, 0, p.entry, what)
            if k in (0, 63, 127):
                w.decode(p, what)
        codec.sync()


@pytest.mark.parametrize("name,start_bit", CASES, ids=lambda v: str(v))
def test_padding_part(codec, name, start_bit):
    """The stream's last part run to the payload's last bit, into the zero bits after the end bit: count,
    exit and symbols of the serial walk (the padding decodes as codewords too); the stream's symbols and
    its end bit come out as for a part that stops at the end bit."""
    bk, m = pc.stream(name, start_bit)
    p = pc.padding_part(bk, m, pc.tiling_cuts(bk, m)[-2])
    with _device_errors_end_the_run():
        codec.dev.upload(bk.cb)
        w = Walker(codec, bk, m)
        for given in (p.entry, ONES):
            what = "%s s%d padding [%d, %d) given=%d" % (name, start_bit, p.pb, p.pe, given)
            w.dev.indexless_scan(w.whole.data_ptr(), w.whole.numel(), m.start_bit, p.pb, p.pe, given, w.summ.data_ptr(),
                                 nsym=m.nsym, payload_bit_base=0)
            got = w.summary()
            if got[2] != p.entry:
                assert given == ONES
                w.dev.indexless_refix(p.entry, w.summ.data_ptr())
                got = w.summary()
            assert got == (p.count, p.exit, p.entry), (what, got, (p.count, p.exit, p.entry))
            w.decode(p, what)
        codec.sync()


# ---- 3. the call contract ----------------------------------------------------------------------------------------
class Contract:
    """A mid-stream part of a stream, its isolated view at a base above 0, guarded outputs, raw calls."""

    def __init__(self, codec, name):
        import torch
        self.codec, self.lib, self.h = codec, codec.dev.lib, codec.dev.h
        self.bk, self.m = pc.stream(name, 5)
        bk, m = self.bk, self.m
        codec.dev.upload(bk.cb)
        self.w = Walker(codec, bk, m)
        rel = lambda i: int(m.pos[i]) - m.start_bit  # noqa: E731
        self.p = pc.part_ref(m, rel(2000) + 3, rel(3000) + 1)
        self.q = pc.part_ref(m, rel(4000) + 1, rel(4300))        # another part (a second scan)
        p = self.p
        assert p.count > 8 and p.entry > m.start_bit + p.pb
        # the view: one byte more than the lead-in below, max_len bits and a byte above
        self.b0 = (m.start_bit + p.pb - pc.LEAD_BITS) // 8 - 1
        self.b1 = (m.start_bit + p.pe + int(bk.ln.max())) // 8 + 2
        self.keep, self.view = _place(m.payload[self.b0:self.b1], 16, 7)
        self.base = 8 * self.b0
        self.summ = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        self.obuf, self.out = _guarded(2 * p.count)
        self.end = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        self.tabbuf, self.tab = _table(self.w.nb)

    def scan(self, ptr, nbytes, base, pb, pe, entry, h=None):
        m = self.m
        return self.lib.hz_indexless_scan(h or self.h, ptr, nbytes, base, m.start_bit, m.nsym, pb, pe, entry,
                                          self.summ.data_ptr())

    def refix(self, entry):
        return self.lib.hz_indexless_refix(self.h, entry, self.summ.data_ptr())

    def decode(self, nsym, ptr=None):
        return self.lib.hz_indexless_decode(self.h, nsym, self.out.data_ptr() if ptr is None else ptr,
                                            self.end.data_ptr())

    def seek(self, nsym):
        return self.lib.hz_indexless_seek(self.h, self.p.first, nsym, self.m.nsym, self.tab.data_ptr())

    def untouched(self):
        """Nothing was launched: no status pending, every guarded output as it was."""
        self.codec.sync()
        return (bool((self.summ == -1).all()) and bool((self.obuf == 0xA5).all()) and bool((self.end == -1).all())
                and bool((self.tabbuf == SENT).all()))

    def no_part(self, what):
        assert self.refix(self.p.entry) == HZ_EINVAL, what
        assert self.decode(self.p.count) == HZ_EINVAL, what
        assert self.seek(self.p.count) == HZ_EINVAL, what
        assert self.seek(0) == HZ_EINVAL, what
        assert self.untouched(), what

    def part_is_good(self, p, what):
        """The pending part p refixes, decodes and seeks to the model's results."""
        w = self.w
        w.dev.indexless_refix(p.entry, w.summ.data_ptr())
        got = w.summary()
        assert got == (p.count, p.exit, p.entry), (what, got)
        w.decode(p, what)


@pytest.mark.parametrize("name", ["hot25", "fixed16"])
def test_refused_at_the_call(codec, name):
    """HZ_EINVAL, nothing launched, nothing written, hz_ctx_sync clean. In each case every other condition of
    the call holds, so the refusal is the named check's."""
    from huffman_amd.codec import Device
    with _device_errors_end_the_run():
        c = Contract(codec, name)
        m, p, v, base = c.m, c.p, c.view, c.base
        ptr, n = v.data_ptr(), v.numel()
        lead_lo = m.start_bit + p.pb - pc.LEAD_BITS          # the first bit of the lead-in
        assert base + 8 <= lead_lo and m.start_bit + p.pe + 8 <= base + 8 * n
        below = m.start_bit + 16 * ((base - m.start_bit) // 16) - 16     # on FIXED16's grid, below the view
        before = int(m.pos[p.first - 1])                                 # a codeword start in the lead-in
        assert m.start_bit <= below < base <= lead_lo < before < m.start_bit + p.pb <= p.entry
        # hz_indexless_scan
        assert c.scan(ptr, n, base, p.pb, p.pe, ONES) == 0 and c.scan(ptr, n, base, p.pb, p.pe, p.entry) == 0
        codec.sync()
        c.codec.dev.upload_decode(c.bk.cb)                   # (ends that part)
        c.summ.fill_(-1)
        assert c.scan(ptr, n, base + 4, p.pb, p.pe, ONES) == HZ_EINVAL          # payload_bit_base % 8
        assert c.scan(ptr, n, base + 1, p.pb, p.pe, p.entry) == HZ_EINVAL
        assert c.scan(ptr, n, base, p.pb, p.pe, below) == HZ_EINVAL             # entry below the view
        assert c.scan(ptr, n, base, p.pb, p.pe, base - 1) == HZ_EINVAL
        assert c.scan(ptr, n, base, p.pb, p.pe, before) == HZ_EINVAL            # entry before the part
        assert c.scan(ptr, n, base, p.pb, p.pe, m.start_bit + p.pb - 1) == HZ_EINVAL
        whole = c.w.whole
        assert c.scan(whole.data_ptr(), 15, 0, 0, 64, ONES) == HZ_EINVAL        # a view under 16 bytes
        assert c.scan(whole.data_ptr(), 16, 0, 0, 64, ONES) == 0                # (and the same part from 16)
        codec.sync()
        tiny = pc.part_ref(m, 0, 64)
        assert tuple(_u64(c.summ)[:3]) == (tiny.count, tiny.exit, tiny.entry), (_u64(c.summ), vars(tiny))
        c.codec.dev.upload_decode(c.bk.cb)
        c.summ.fill_(-1)
        assert c.scan(ptr, n, base, p.pb, p.pb, ONES) == HZ_EINVAL              # part_end <= part_begin
        assert c.scan(ptr, n, base, p.pe, p.pb, ONES) == HZ_EINVAL
        assert c.scan(ptr + 2, n - 2, base + 16, p.pb, p.pe, ONES) == HZ_EINVAL  # the lead-in not in the view
        short = (m.start_bit + p.pe - 1) // 8 - c.b0
        assert short >= 16 and base + 8 * short < m.start_bit + p.pe
        assert c.scan(ptr, short, base, p.pb, p.pe, ONES) == HZ_EINVAL          # the part not in the view
        bare = Device(0)                                                        # a context without decode tables
        assert c.scan(ptr, n, base, p.pb, p.pe, ONES, h=bare.h) == HZ_EINVAL
        bare.close()
        assert c.untouched()
        # no pending part: the refusals above left none
        c.no_part("after refused scans")
        # hz_indexless_refix against the pending part's base and first bit
        assert c.scan(ptr, n, base, p.pb, p.pe, ONES) == 0
        codec.sync()
        c.summ.fill_(-1)
        for entry in (below, base - 1 if name != "fixed16" else below - 16, before, m.start_bit + p.pb - 1):
            assert c.refix(entry) == HZ_EINVAL, entry
        # hz_indexless_decode: d_out off the 16-byte grid
        for off in (2, 8):
            assert c.decode(p.count, c.out.data_ptr() + off) == HZ_EINVAL
        assert c.decode(p.count, 0) == HZ_EINVAL
        # hz_indexless_seek without codewords: HZ_OK, nothing written
        assert c.seek(0) == 0
        assert c.untouched()
        # the refusals did not end the part
        c.part_is_good(p, name + " after refusals")
        codec.sync()


def _intervening(c):
    """(name, call, ends the part) for every call of the lifetime test, on buffers made once."""
    import torch
    from huffman_amd import block_sums_bytes, index_bytes
    from huffman_amd._lib import Codebook
    lib, h, m, bk = c.lib, c.h, c.m, c.bk
    nsym, nb, nbytes = m.nsym, c.w.nb, m.payload.size
    fixed = bk.name == "fixed16"
    x = torch.from_numpy(m.sym.view(np.uint8).copy()).cuda()
    pay = c.w.whole
    out = torch.zeros(2 * nsym + 64, dtype=torch.uint8, device="cuda")
    pout = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(index_bytes(nsym), dtype=torch.uint8, device="cuda")
    midx = torch.from_numpy(m.index.copy()).cuda()
    seek = torch.from_numpy(m.start.view(np.int64).copy()).cuda()
    tab = torch.zeros(nb + 1, dtype=torch.int64, device="cuda")
    end = torch.zeros(1, dtype=torch.int64, device="cuda")
    hist = torch.zeros(65536, dtype=torch.int64, device="cuda")
    sums = torch.zeros(block_sums_bytes(x.numel()), dtype=torch.uint8, device="cuda")
    dcb = torch.zeros((ctypes.sizeof(Codebook) + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    rg = torch.tensor([[10, 100, 0]], dtype=torch.int64, device="cuda")
    pieces = torch.tensor([[0, nbytes, 0, 0, 0, nb]], dtype=torch.int64, device="cuda")
    prg = torch.tensor([[10, 100, 0, 0]], dtype=torch.int64, device="cuda")
    c.bufs = [x, out, pout, idx, midx, seek, tab, end, hist, sums, dcb, stats, rg, pieces, prg]
    P = lambda t: t.data_ptr()  # noqa: E731
    cb = ctypes.byref(bk.cb)
    q = c.q
    return [
        ("hz_pack", lambda: lib.hz_pack(h, P(x), x.numel(), m.start_bit, m.lead, P(pout), nbytes, P(idx)), True),
        ("hz_pack_seek", lambda: lib.hz_pack_seek(h, P(x), x.numel(), m.start_bit, m.lead, P(pout), nbytes, None, 0, 0,
                                                  nsym, P(tab)), True),
        ("hz_index_build", lambda: lib.hz_index_build(h, P(pay), nbytes, m.start_bit, nsym, P(idx)), True),
        # FIXED16 decodes and builds its table by arithmetic, with no scratch: the part stays
        ("hz_decode_indexless", lambda: lib.hz_decode_indexless(h, P(pay), nbytes, m.start_bit, nsym, P(out), P(end)),
         not fixed),
        ("hz_seek_build", lambda: lib.hz_seek_build(h, P(pay), nbytes, m.start_bit, nsym, P(tab)), not fixed),
        ("hz_decode_range", lambda: lib.hz_decode_range(h, P(pay), nbytes, 0, P(seek), nsym, 10, 100, P(out), 0), True),
        ("hz_decode_ranges", lambda: lib.hz_decode_ranges(h, P(pay), nbytes, 0, P(seek), nsym, P(rg), 1, P(out),
                                                          out.numel(), P(stats), 0), True),
        ("hz_decode_ranges_pieces", lambda: lib.hz_decode_ranges_pieces(h, P(pay), nbytes, P(seek), nb + 1, P(pieces), 1,
                                                                        nsym, P(prg), 1, P(out), out.numel(), P(stats),
                                                                        0), True),
        ("hz_codebook_upload_decode", lambda: lib.hz_codebook_upload_decode(h, cb), True),
        ("hz_indexless_scan", lambda: lib.hz_indexless_scan(h, P(pay), nbytes, 0, m.start_bit, nsym, q.pb, q.pe, ONES,
                                                            c.w.summ.data_ptr()), "replaced"),
        ("hz_hist16", lambda: lib.hz_hist16(h, P(x), x.numel(), P(hist), 0), False),
        ("hz_block_sums", lambda: lib.hz_block_sums(h, P(x), x.numel(), P(sums)), False),
        ("hz_decode", lambda: lib.hz_decode(h, P(pay), nbytes, nsym, P(midx), P(out)), False),
        ("hz_index_expand", lambda: lib.hz_index_expand(h, P(pay), nbytes, P(seek), nsym, P(idx)), False),
        ("hz_codebook_upload_encode", lambda: lib.hz_codebook_upload_encode(h, cb), False),
        ("hz_codebook_build_device", lambda: lib.hz_codebook_build_device(h, P(hist), P(dcb)), False),
        ("hz_ctx_sync", lambda: lib.hz_ctx_sync(h), False),
    ]


@pytest.mark.parametrize("name", ["hot25", "fixed16"])
def test_pending_part_lifetime(codec, name):
    """Which calls end a pending part (hz_indexless_refix / _decode / _seek then return HZ_EINVAL: the guard
    against kernels launched with pointers into scratch that has been rewritten or freed) and which leave it
    alone (the part then refixes, decodes and seeks to the model's results: they did not write the
    scratch). Each call runs once before the scan, so the scratch has already grown to what it needs."""
    with _device_errors_end_the_run():
        c = Contract(codec, name)
        m, p = c.m, c.p
        whole = c.w.whole
        for call_name, call, ends in _intervening(c):
            what = "%s: %s" % (name, call_name)
            assert call() == 0, what
            codec.sync()
            c.w.scan(p, whole, 0, ONES, what)
            assert call() == 0, what
            codec.sync()
            c.summ.fill_(-1)
            if ends == "replaced":            # the second scan's part is the pending one
                c.part_is_good(c.q, what)
            elif ends:
                c.no_part(what)
            else:
                c.part_is_good(p, what)
        codec.sync()
