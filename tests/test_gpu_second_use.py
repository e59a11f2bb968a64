"""Second use: every stream-ordered call run again on ONE context with the same host arguments and
different device memory, eagerly (part 1) and as a graph captured on stream A and replayed on stream B
and on A again (part 2). The context's scratch only grows and is never cleared between calls, so what a
call does not reset it inherits from the call before; a replay on the data of its capture cannot tell a
stream-ordered call from one that baked something about that data into the graph on the host.

A pair is two streams A and B under one codebook with the same nsym, the same nonzero start bit and
the same buffers: the payload buffer is as long as the longer payload and one more 16-byte chunk, and each
payload is zero-filled to that size (every book is a complete prefix code, so the padding walks as
codewords; the extra chunk puts a whole codeword's bits behind the last bound of the split parts). Every host
argument of a call is then equal for A and B; only device memory differs. Each pair runs in both orders.

  records               zipf21   shortest / longest   A holds more records per chain than the capacity of
                                                      chain_geom (k_chain_tail); B leaves most rows of every
                                                      chain untouched, still holding A's records
  records-at-cap        hot25    shortest / longest   A fills every chain's rows exactly to the capacity
  largest-block-hot25   hot25    longest / uniform    A: a first block of 2048 x max_len bits and blocks over
  largest-block-zipf21  zipf21   longest / chains     the pack slot (the cold list); B has none
  blocks-chains         zipf21   blocks / chains      block sizes alternate against uniform
  no-resync             even     uniform / chains     fix-ups cascade from chain to chain
  serial-records        fib57    longest / shortest   k_chain_decode_serial, k_chain_walk<true>, WIDE pack
  dense                 dense16  uniform / shortest   the chain LUT beside DENSE tables
  fixed                 fixed16  two uniform draws    the arithmetic paths

Two pairs are not the ones first thought of, because a condition on the inputs (test_pairs_differ, on the
CPU, from the models alone) does not hold for them:
  * hot25 `shortest` is all 1-bit codes, yet chain_geom sizes a hot25 chain (4096 bits) for 512 records
    = 4096 codewords: no stream under hot25 can overrun the capacity. `records` therefore takes zipf21
    (634 records against a capacity of 512), and hot25 stays as `records-at-cap` (exactly 512).
  * zipf21 `uniform` draws from all 65 536 symbols, about 17 bits each: every block is over the pack slot.
    B of `largest-block-zipf21` is `chains` (no block over the slot).
fixed16 payloads have one size (16 bits a symbol): that pair differs in its bytes alone.

Every expected value comes from the numpy model (tests/ref_stream.py over the CPU oracle), np.bincount,
the host codebook builder and header writer, or the oracle's walk and header parse; never from a first
run's device output. Outputs and index buffers sit between 64-byte guards of 0xA5 refilled before each
call; the payload (an input) is compared with the model's after each consumer. A HIP runtime error ends
the session (Checks). hz_index_build synchronises inside (launch_index_build's loop reads its `changed`
word on the host) and the split parts take each part's true entry, a value read from the stream, as a host
argument: both are eager-only.

Run as a script (`python tests/test_gpu_second_use.py nolead`) it runs the `records` and `no-resync` pairs
through hz_decode_indexless and hz_seek_build in both orders and prints "ok": the test starts it in a
fresh process with HZ_SEG_LEAD=0, which the library reads once.

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
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import oracle_lib  # noqa: E402
import ref_stream  # noqa: E402
from table_books import book  # noqa: E402
from test_gpu_designed_streams import Checks, _guarded, _guards_intact, _lead, _stream  # noqa: E402

gpu = pytest.mark.gpu

BLK = 2048
GUARD = 64
ONES = (1 << 64) - 1
NSYM = 40 * BLK + 777       # several chains, several waves and middle blocks
START_BIT = 45
SLOT_CAP_BITS = 1024 * 32   # no pack slot is larger (tests/test_gpu_stagger_carry.py)
NCU = 256                   # MI355X; chain_geom is one chain per walk lane only far above these sizes

# name: (book, kind of A, kind of B)
PAIRS = {
    "records": ("zipf21", "shortest", "longest"),
    "records-at-cap": ("hot25", "shortest", "longest"),
    "largest-block-hot25": ("hot25", "longest", "uniform"),
    "largest-block-zipf21": ("zipf21", "longest", "chains"),
    "blocks-chains": ("zipf21", "blocks", "chains"),
    "no-resync": ("even", "uniform", "chains"),
    "serial-records": ("fib57", "longest", "shortest"),
    "dense": ("dense16", "uniform", "shortest"),
    "fixed": ("fixed16", "uniform", "uniform"),
}
ORDERS = ["AB", "BA"]
EAGER = [(name, order) for name in PAIRS for order in ORDERS]

# the calls: eager-only ones synchronise inside or take a value read from the stream as a host argument
INDEXLESS = ["indexless", "indexless_seek", "seek_build"]
RANGE = ["range seek blocks", "range seek ragged", "range full blocks", "range full ragged"]
CAPTURABLE = ["hist16", "pack", "decode", "index_expand"] + INDEXLESS + RANGE + ["ranges seek", "ranges full", "pieces"]
EAGER_ONLY = ["index_build", "parts"]
# part 2: the calls replayed under each pair
REPLAYED = {
    "records": CAPTURABLE,
    "records-at-cap": CAPTURABLE,
    "largest-block-hot25": CAPTURABLE,
    "largest-block-zipf21": CAPTURABLE,
    "no-resync": CAPTURABLE,
    "serial-records": INDEXLESS,
    "dense": INDEXLESS,
    "fixed": INDEXLESS + RANGE,
}
NOLEAD_PAIRS = ["records", "no-resync"]

_pairs = {}


def pair(name):
    """The two streams of a pair, their models and the sizes they share."""
    if name not in _pairs:
        b, ka, kb = PAIRS[name]
        bk = book(b)
        side = {}
        for w, kind in (("A", ka), ("B", kb)):
            rng = np.random.default_rng(zlib.crc32(("second-%s-%s" % (name, w)).encode()))
            sym = _stream(bk, kind, NSYM, rng)
            side[w] = SimpleNamespace(kind=kind, sym=sym, m=ref_stream.model(sym, bk.ln, bk.code, START_BIT, _lead(START_BIT)))
        nbytes = max(s.m.payload.size for s in side.values()) + 16
        for s in side.values():
            s.pay = np.zeros(nbytes, np.uint8)
            s.pay[:s.m.payload.size] = s.m.payload
        _pairs[name] = SimpleNamespace(name=name, bk=bk, side=side, nsym=NSYM, nb=ref_stream.nblocks(NSYM), nbytes=nbytes,
                                       start_bit=START_BIT, lead=_lead(START_BIT), ibytes=ref_stream.index_nbytes(NSYM))
    return _pairs[name]


def ranges_of(nsym):
    """Whole interior blocks, ragged edges inside the stream, and the stream's ragged tail."""
    return [(2 * BLK, 3 * BLK), (7 * BLK - 7, 2 * BLK + 19), (nsym - 100, 100)]


def cut_of(p):
    """A payload bit (after start_bit) near the middle of the shorter stream that lies inside a codeword of
    A or of B, of both where there is one (`shortest` under hot25 and fib57 is 1-bit codes: every bit
    starts a codeword there)."""
    rel = [s.m.pos.astype(np.int64) - p.start_bit for s in p.side.values()]
    mid = int(min(r[-1] for r in rel)) // 2
    span = np.arange(mid, mid + 256)
    inside = [~np.isin(span, r) for r in rel]
    both = np.nonzero(inside[0] & inside[1])[0]
    one = np.nonzero(inside[0] | inside[1])[0]
    assert one.size, p.name
    return int(span[both[0] if both.size else one[0]])


# ---- the conditions on the inputs (CPU) ---------------------------------------------------------------
def chain_geom(bk, payload_bytes, start_bit, nsym):
    """(cbits, cap) as hz_chain.hip chain_geom takes them for hz_decode_indexless over this buffer: the
    bits a walk of nsym codewords can reach (clamp_reach), chains of one expected block, the capacity
    their expected records with 25 % headroom and 64, in whole decode blocks of 256 records."""
    ln = bk.ln[bk.ln > 0].astype(np.float64)
    reach = (start_bit + nsym * int(ln.max()) + 7) // 8 + 8
    pbits = 8 * min(payload_bytes, reach) - start_bit
    kraft = float((ln * np.exp2(-ln)).sum())
    avg = pbits / nsym
    if 0.5 < kraft < avg:
        avg = kraft
    avg = max(avg, 1.0)
    lanes = 16 * 64 * NCU
    cb = max((pbits + lanes - 1) // lanes, int(BLK * avg))
    cb = (cb + 127) & ~127
    recs = cb / avg / 8.0 * 1.25 + 64.0
    return cb, int((recs + 255) // 256) * 256


def chain_records(m, cbits):
    """Records (8 codewords each) of every cbits window of the stream's own bits."""
    rel = m.pos[:-1].astype(np.int64) - m.start_bit
    return (np.bincount(rel // cbits) + 7) // 8


def blocks_bits(m):
    return np.diff(m.start.astype(np.int64))


def test_pairs_differ(built_lib):
    """Each pair differs in the quantity it is named for; from the models alone."""
    for name in PAIRS:
        p = pair(name)
        a, b = p.side["A"].m, p.side["B"].m
        used = p.bk.ln[p.bk.ln > 0]
        assert sum(1 << (56 - int(v)) for v in used) == 1 << 56, name          # a complete prefix code
        assert a.nsym == b.nsym == NSYM and a.start_bit == b.start_bit == START_BIT != 0
        assert p.side["A"].pay.size == p.side["B"].pay.size == p.nbytes
        assert not np.array_equal(p.side["A"].pay, p.side["B"].pay)
        if name == "fixed":
            assert a.payload.size == b.payload.size
        else:
            assert abs(a.payload.size - b.payload.size) >= 16, name
        over = [int((blocks_bits(m) > SLOT_CAP_BITS).sum()) for m in (a, b)]
        cbits, cap = chain_geom(p.bk, p.nbytes, START_BIT, NSYM)
        ra, rb = chain_records(a, cbits), chain_records(b, cbits)
        if name == "records":
            assert int(ra[0]) > cap and int(ra[1:-1].min()) > cap      # past the capacity: k_chain_tail
            assert int(rb.max()) < cap // 2                            # most rows keep A's records
        if name == "records-at-cap":
            assert int(ra[0]) == cap == int(ra[:-1].min()) and int(rb.max()) < cap // 8
        if name == "serial-records":
            assert int(p.bk.ln.max()) == 56 and int(blocks_bits(a)[0]) >= 65536
            assert int(ra.max()) < cap // 8 and int(rb[0]) == cap
        if name.startswith("largest-block"):
            assert a.max_bits == int(blocks_bits(a)[0]) == BLK * int(p.bk.ln.max()) > SLOT_CAP_BITS
            assert over[0] >= 1 and over[1] == 0 and b.max_bits <= SLOT_CAP_BITS
        if name == "blocks-chains":
            full = blocks_bits(a)[:NSYM // BLK]
            assert int(full[0::2].min()) > 2 * int(full[1::2].max())
            fullb = blocks_bits(b)[:NSYM // BLK]
            assert int(fullb.max()) < 1.1 * int(fullb.min())
        if name == "no-resync":
            assert not (used & 1).any()
        if name == "dense":
            assert sorted(set(used.tolist())) == [15, 16]
        c = cut_of(p)
        assert 0 < c < min(a.end_bit, b.end_bit) - START_BIT


def test_case_matrix_is_complete():
    """Every pair of the table in both orders in part 1; every replayed call on the pairs it is due on."""
    assert {n for n, _ in EAGER} == set(PAIRS) and all((n, o) in EAGER for n in PAIRS for o in ORDERS)
    assert len(EAGER) == len(set(EAGER)) == 2 * len(PAIRS)
    assert {b for b, _, _ in PAIRS.values()} == {"hot25", "zipf21", "even", "fib57", "dense16", "fixed16"}
    assert set(CALLS) == set(CAPTURABLE) | set(EAGER_ONLY) and not set(CAPTURABLE) & set(EAGER_ONLY)
    for n in ("records", "largest-block-hot25", "largest-block-zipf21", "no-resync"):
        assert REPLAYED[n] == CAPTURABLE
    for n in ("serial-records", "dense"):
        assert set(REPLAYED[n]) == set(INDEXLESS)
    assert set(REPLAYED["fixed"]) == set(INDEXLESS) | set(RANGE)
    assert set(REPLAYED) <= set(PAIRS) and set(NOLEAD_PAIRS) <= set(PAIRS)
    assert NSYM <= 1 << 21


# ---- one pair's buffers on one context ------------------------------------------------------------------
@pytest.fixture(scope="module")
def hz(built_lib):
    import huffman_amd
    return huffman_amd


@pytest.fixture(scope="module")
def codec(built_lib):
    from huffman_amd.pipeline import StreamCodec
    return StreamCodec(0)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


class Rig:
    """The device buffers of one pair: inputs refilled in place with A's or B's bytes (load), outputs
    between guards refilled with 0xA5; `src` holds each side's inputs and expected outputs, from the models."""

    def __init__(self, codec, p, pieces=True):
        import torch
        import huffman_amd
        self.codec, self.dev, self.p = codec, codec.dev, p
        self.ranges = ranges_of(p.nsym)
        self.src = {}
        for w, s in p.side.items():
            hist = np.bincount(s.sym, minlength=65536).astype(np.uint64)
            self.src[w] = SimpleNamespace(m=s.m, own=s.m.payload.size, x=_dev(s.sym), payload=_dev(s.pay), index=_dev(s.m.index),
                                          seek=_dev(s.m.start), hist=_dev(hist), nsym=p.nsym, host_pay=s.pay)
        u8 = lambda n: torch.empty(n, dtype=torch.uint8, device="cuda")  # noqa: E731
        self.x = u8(2 * p.nsym)
        self.paybuf, self.pay = _guarded(p.nbytes)
        self.index_in = u8(p.ibytes)
        self.seek_in = u8(8 * (p.nb + 1))
        self.outs = {}
        for name, n in (("pk", p.nbytes), ("idx", p.ibytes), ("out", 2 * p.nsym), ("tab", 8 * (p.nb + 1)), ("hist", 8 * 65536),
                        ("end", 8), ("summ", 32)):
            buf, region = _guarded(n)
            self.outs[name] = (buf, GUARD, n)
            setattr(self, name, region)
        for i, (_, count) in enumerate(self.ranges[:2]):     # hz_decode_range's outputs: 16- and 2-byte aligned
            buf = torch.empty(GUARD + 16 + 2 * count + GUARD, dtype=torch.uint8, device="cuda")
            self.outs["r%d" % i] = (buf, GUARD + 2 * i, 2 * count)
        # the batch: one list, one layout; the gathered form is planned per side (its pieces follow the table)
        import test_gpu_ranges_batch as trb
        self.trb = trb
        self.offs, self.size = trb.layout(self.ranges)
        self.outs["batch"] = (torch.empty(self.size, dtype=torch.uint8, device="cuda"), 0, 0)
        self.rg = torch.tensor([[b, c, o] for (b, c), o in zip(self.ranges, self.offs)], dtype=torch.int64, device="cuda")
        self.stats = torch.zeros(4, dtype=torch.int64, device="cuda")
        self.has_pieces = pieces
        if pieces:
            import test_gpu_ranges_pieces as tpc
            for i, s in enumerate(self.src.values()):
                s.plan = tpc.plan_of(huffman_amd, s, self.ranges, self.offs)
                s.g = tpc.on_device(s.plan, seed=30 + i)
            plans = [s.plan for s in self.src.values()]
            self.g_buf = u8(max(pl.buf_bytes for pl in plans) + 64)
            self.g_seek = torch.empty(max(pl.seek_words for pl in plans) + 3, dtype=torch.int64, device="cuda")
            self.g_pieces = torch.empty((len(self.ranges), 6), dtype=torch.int64, device="cuda")
            self.g_rgs = torch.empty((len(self.ranges), 4), dtype=torch.int64, device="cuda")
        self.dev.upload(p.bk.cb)

    def load(self, w):
        """Side w into the input buffers, in place; every output and its guards back to 0xA5."""
        s = self.src[w]
        self.x.copy_(s.x)
        self.pay.copy_(s.payload)
        self.index_in.copy_(s.index)
        self.seek_in.copy_(s.seek)
        for buf, _, _ in self.outs.values():
            buf.fill_(0xA5)
        self.stats.fill_(-1)
        if self.has_pieces:
            k = len(s.plan.pieces)
            self.g_buf.fill_(0x3C)
            self.g_buf[:s.g.buf.numel()] = s.g.buf
            self.g_seek.fill_(-1)
            self.g_seek[:s.g.seek.numel()] = s.g.seek
            self.g_pieces.fill_(-1)                      # pieces not in use: nothing names them
            self.g_pieces[:k] = s.g.pieces[:k]
            self.g_rgs.copy_(s.g.ranges)
        return s

    def intact(self, name):
        buf, lo, n = self.outs[name]
        return bool((buf[:lo] == 0xA5).all()) and bool((buf[lo + n:] == 0xA5).all())

    def region(self, name):
        buf, lo, n = self.outs[name]
        return buf[lo:lo + n]

    def u64(self, name):
        return [int(v) for v in self.region(name).cpu().numpy().view(np.uint64)]

    def payload_unchanged(self, s):
        import torch
        return torch.equal(self.pay, s.payload) and _guards_intact(self.paybuf, self.p.nbytes)


# ---- the calls: (issue, check against side s's model); every argument of `issue` is the pair's -----------
def _same(ck, tag, got, want):
    import torch
    ok = torch.equal(got, want)
    ck.expect(tag, ok, "" if ok else "first differing byte %d of %d" % (int(torch.nonzero(got != want)[0]), want.numel()))


def _untouched(ck, tag, r, names):
    for n in names:
        ck.expect("%s: %s written" % (tag, n), bool((r.outs[n][0] == 0xA5).all()))


def _i_hist(r):
    r.dev.hist16(r.x.data_ptr(), r.x.numel(), r.hist.data_ptr(), False)


def _k_hist(r, ck, t, s):
    _same(ck, t, r.hist, s.hist)
    ck.expect(t + " guards", r.intact("hist"))


def _i_pack(r):
    p = r.p
    r.dev.pack(r.x.data_ptr(), r.x.numel(), p.start_bit, p.lead, r.pk.data_ptr(), p.nbytes, r.idx.data_ptr())


def _k_pack(r, ck, t, s):
    first = 4 * (r.p.start_bit // 32)
    _same(ck, t + " payload", r.pk[first:s.own], s.payload[first:s.own])
    ck.expect(t + " wrote before start_bit's word", bool((r.pk[:first] == 0xA5).all()))
    ck.expect(t + " wrote past the stream's last word", bool((r.pk[s.own:] == 0xA5).all()))
    _same(ck, t + " index", r.idx, s.index)
    ck.expect(t + " guards", r.intact("pk") and r.intact("idx"))


def _i_decode(r):
    r.dev.decode(r.pay.data_ptr(), r.p.nbytes, r.p.nsym, r.index_in.data_ptr(), r.out.data_ptr())


def _k_out(r, ck, t, s):
    _same(ck, t + " symbols", r.out, s.x)
    ck.expect(t + " guards", r.intact("out"))


def _i_index_build(r):
    r.dev.index_build(r.pay.data_ptr(), r.p.nbytes, r.p.start_bit, r.p.nsym, r.idx.data_ptr())


def _i_index_expand(r):
    r.dev.index_expand(r.pay.data_ptr(), r.p.nbytes, r.seek_in.data_ptr(), r.p.nsym, r.idx.data_ptr())


def _k_index(r, ck, t, s):
    _same(ck, t, r.idx, s.index)
    ck.expect(t + " guards", r.intact("idx"))


def _i_indexless(r):
    r.dev.decode_indexless(r.pay.data_ptr(), r.p.nbytes, r.p.start_bit, r.p.nsym, r.out.data_ptr(), r.end.data_ptr())


def _k_end(r, ck, t, s):
    got = r.u64("end")[0]
    ck.expect(t + " end bit", got == s.m.end_bit, "%d != %d" % (got, s.m.end_bit))
    ck.expect(t + " end bit guards", r.intact("end"))


def _k_indexless(r, ck, t, s):
    _k_out(r, ck, t, s)
    _k_end(r, ck, t, s)


def _i_indexless_seek(r):
    r.dev.decode_indexless_seek(r.pay.data_ptr(), r.p.nbytes, r.p.start_bit, r.p.nsym, r.out.data_ptr(), r.tab.data_ptr(),
                                r.end.data_ptr())


def _k_tab(r, ck, t, s):
    _same(ck, t + " table", r.tab, s.seek)
    ck.expect(t + " table guards", r.intact("tab"))


def _k_indexless_seek(r, ck, t, s):
    _k_indexless(r, ck, t, s)
    _k_tab(r, ck, t, s)


def _i_seek_build(r):
    r.dev.seek_build(r.pay.data_ptr(), r.p.nbytes, r.p.start_bit, r.p.nsym, r.tab.data_ptr())


def _k_seek_build(r, ck, t, s):
    _k_tab(r, ck, t, s)
    _untouched(ck, t, r, ["out"])


def _range(i, full):
    def issue(r):
        begin, count = r.ranges[i]
        buf, lo, _ = r.outs["r%d" % i]
        r.dev.decode_range(r.pay.data_ptr(), r.p.nbytes, (r.index_in if full else r.seek_in).data_ptr(), r.p.nsym, begin, count,
                           buf[lo:].data_ptr(), full)

    def check(r, ck, t, s):
        begin, count = r.ranges[i]
        _same(ck, t, r.region("r%d" % i), s.x[2 * begin:2 * (begin + count)])
        ck.expect(t + " guards", r.intact("r%d" % i))
    return issue, check


def _ranges(full):
    def issue(r):
        r.codec.decode_ranges(r.pay, r.p.nsym, r.index_in if full else r.seek_in, r.rg, r.outs["batch"][0], stats=r.stats,
                              full_index=full)
    return issue, _k_batch


def _k_batch(r, ck, t, s):
    _same(ck, t, r.outs["batch"][0], r.trb.image(s, r.ranges, r.offs, r.size))
    st = [int(v) for v in r.stats.cpu()]
    ck.expect(t + " stats", st[0] == sum(r.trb.nblk(b, c) for b, c in r.ranges) and st[3] == 0, str(st))


def _i_pieces(r):
    r.codec.decode_ranges_pieces(r.g_buf, r.g_seek, r.g_pieces, r.p.nsym, r.g_rgs, r.outs["batch"][0], stats=r.stats)


CALLS = {
    "hist16": (_i_hist, _k_hist),
    "pack": (_i_pack, _k_pack),
    "decode": (_i_decode, _k_out),
    "index_build": (_i_index_build, _k_index),
    "index_expand": (_i_index_expand, _k_index),
    "indexless": (_i_indexless, _k_indexless),
    "indexless_seek": (_i_indexless_seek, _k_indexless_seek),
    "seek_build": (_i_seek_build, _k_seek_build),
    "range seek blocks": _range(0, False),
    "range seek ragged": _range(1, False),
    "range full blocks": _range(0, True),
    "range full ragged": _range(1, True),
    "ranges seek": _ranges(False),
    "ranges full": _ranges(True),
    "pieces": (_i_pieces, _k_batch),
    "parts": None,      # _parts: several calls with the stream's own entry bits between them
}
PRODUCERS = ("hist16", "pack")   # they read x, not the payload


def _eager(r, name, order):
    """call(first), sync, check; call(second), sync, check: one call after the other on the two streams."""
    ck = Checks(r.codec)
    for w in order:
        s = r.load(w)
        t = "%s on %s (order %s)" % (name, w, order)
        if name == "parts":
            _parts(r, ck, t, s)
        else:
            issue, check = CALLS[name]
            ck.run(t, lambda: issue(r))
            check(r, ck, t, s)
        if name not in PRODUCERS:
            ck.expect(t + ": payload (an input) changed", r.payload_unchanged(s))
    return ck.failed


# ---- part 1 ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,order", EAGER, ids=["%s-%s" % c for c in EAGER])
def test_eager_second_use(codec, name, order):
    """Every call on the first stream of the pair, then on the second: one context, the same buffers."""
    p = pair(name)
    r = Rig(codec, p)
    failed = []
    for call in CALLS:
        if call == "parts":
            continue            # test_eager_parts
        failed += _eager(r, call, order)
    assert not failed, "\n".join(failed)


@gpu
@pytest.mark.parametrize("name,order", EAGER, ids=["%s-%s" % c for c in EAGER])
def test_eager_parts(codec, name, order):
    """The split parts (scan -> refix -> decode -> seek) of the first stream, then of the second."""
    p = pair(name)
    r = Rig(codec, p, pieces=False)
    failed = _eager(r, "parts", order)
    assert not failed, "\n".join(failed)


def _parts(r, ck, t, s):
    """hz_indexless_scan over two parts cut inside a codeword (the second first from its walked entry, then
    refixed to the first part's exit) -> hz_indexless_decode (into the 16-byte aligned output, then copied to
    its place) -> hz_indexless_seek. Each summary equals the oracle's serial walk of the model's payload from
    the part's true entry."""
    import torch
    p, dev = r.p, r.dev
    start, nsym = p.start_bit, p.nsym
    bounds = [0, cut_of(p), 8 * p.nbytes - start - 64]   # past both streams, a whole codeword's bits behind it
    whole = torch.full((2 * nsym,), 0xA5, dtype=torch.uint8, device="cuda")
    entry, first = start, 0
    for k, (pb, pe) in enumerate(zip(bounds, bounds[1:])):
        ref_n, ref_exit, _ = oracle_lib.walk(s.host_pay, p.bk.ln, p.bk.code, entry, start + pe, max_count=pe - pb + 1)
        ck.run("%s scan %d" % (t, k), lambda: dev.indexless_scan(r.pay.data_ptr(), p.nbytes, start, pb, pe, ONES,
                                                                 r.summ.data_ptr(), nsym=nsym))
        cnt, xit, ent = r.u64("summ")[:3]
        if k == 0:
            ck.expect("%s first part's walked entry" % t, ent == start, "%d != %d" % (ent, start))
        if ent != entry:
            ck.run("%s refix %d" % (t, k), lambda: dev.indexless_refix(entry, r.summ.data_ptr()))
            cnt, xit, ent = r.u64("summ")[:3]
        ck.expect("%s summary %d" % (t, k), (cnt, xit, ent) == (ref_n, ref_exit, entry),
                  "(count, exit, entry) = %s, serial walk %s" % ((cnt, xit, ent), (ref_n, ref_exit, entry)))
        take = min(ref_n, nsym - first)
        r.outs["out"][0].fill_(0xA5)
        ck.run("%s decode %d" % (t, k), lambda: dev.indexless_decode(take, r.out.data_ptr(), r.end.data_ptr()))
        ck.expect("%s decode %d guards" % (t, k), r.intact("out") and bool((r.out[2 * take:] == 0xA5).all()))
        whole[2 * first:2 * (first + take)] = r.out[:2 * take]
        ck.run("%s seek %d" % (t, k), lambda: dev.indexless_seek(first, take, nsym, r.tab.data_ptr()))
        first += take
        entry = ref_exit
    assert first == nsym                                # the oracle's own walk covers the stream
    _same(ck, t + " symbols", whole, s.x)
    _k_end(r, ck, t, s)
    _k_tab(r, ck, t, s)
    ck.expect(t + " summary guards", r.intact("summ"))


@gpu
@pytest.mark.parametrize("name", ["records", "largest-block-hot25"])
def test_end_bit_after_a_short_payload(codec, name):
    """hz_decode_indexless of one stream with payload_bytes cut to half its own payload (too few codewords:
    the end bit is all ones), then the other stream whole: its end bit and symbols from the model, not what the
    cut run left in info[2]. Both orders."""
    p = pair(name)
    r = Rig(codec, p, pieces=False)
    ck = Checks(codec)
    for cut, whole in ("AB", "BA"):
        s = r.load(cut)
        half = s.own // 2
        t = "%s: %s cut to %d bytes" % (name, cut, half)
        ck.run(t, lambda: r.dev.decode_indexless(r.pay.data_ptr(), half, p.start_bit, p.nsym, r.out.data_ptr(), r.end.data_ptr()))
        got = r.u64("end")[0]
        ck.expect(t + " end bit", got == ONES, "%d" % got)
        ck.expect(t + " guards", r.intact("out") and r.intact("end") and r.payload_unchanged(s))
        s = r.load(whole)
        t = "%s: %s whole after %s cut" % (name, whole, cut)
        ck.run(t, lambda: _i_indexless(r))
        _k_indexless(r, ck, t, s)
        ck.expect(t + ": payload (an input) changed", r.payload_unchanged(s))
    assert not ck.failed, "\n".join(ck.failed)


# ---- the codebook workspace ---------------------------------------------------------------------------------
HEAD_N, HEAD_LAST = 2 * 12345 + 1, 0x5a      # the header's N and last byte: host arguments, one value for every histogram
HEAD_CAP = 16 + 65536 * 11


def _hists():
    s = np.arange(65536, dtype=np.uint64)
    d = ((s & np.uint64(255)) + np.uint64(1)) * ((s >> np.uint64(8)) + np.uint64(1))
    zipf = np.uint64(1 << 30) // d + np.uint64(1)          # tests/table_books.py zipf21
    three = np.zeros(65536, np.uint64)
    three[[5, 0x8005, 0xfffe]] = [1, 1, 2]
    one = np.zeros(65536, np.uint64)
    one[0x1234] = 7
    return {"zipf21": zipf, "three": three, "one": one}


class CbRig:
    """Device codebook builder, header writer and header parser on fixed buffers. Expected: the host builder,
    the host writer, the oracle's parse of the host writer's header (zero-filled to the longest one)."""

    def __init__(self, codec, hz):
        import torch
        from huffman_amd._lib import Codebook
        self.codec, self.dev, self.Codebook = codec, codec.dev, Codebook
        self.want = {}
        for name, h in _hists().items():
            cb = hz.build_codebook(h)
            head, pbits, pend = hz.write_header(cb, HEAD_N, HEAD_LAST)
            self.want[name] = SimpleNamespace(hist=_dev(h), cb=cb, head=head, pbits=pbits, pend=pend,
                                              blob=head + (bytes([pend]) if pbits else b"") + bytes(16))
        assert np.array_equal(hz.codebook_arrays(self.want["zipf21"].cb)[1], book("zipf21").ln)
        self.flen = max(len(w.blob) for w in self.want.values())
        for w in self.want.values():
            w.blob = w.blob + bytes(self.flen - len(w.blob))
            w.file = _dev(np.frombuffer(w.blob, np.uint8))
            w.parse = oracle_lib.parse_header(w.blob)
        z = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
        self.hist, self.file = z(8 * 65536), z(self.flen)
        self.cb, self.cb2 = z(ctypes.sizeof(Codebook)), z(ctypes.sizeof(Codebook))
        self.headbuf, self.head = _guarded(HEAD_CAP)
        self.info, self.pinfo = z(4, torch.int64), z(6, torch.int64)

    def load(self, name):
        w = self.want[name]
        self.hist.copy_(w.hist)
        self.file.copy_(w.file)
        self.headbuf.fill_(0xA5)
        for t in (self.cb, self.cb2, self.info, self.pinfo):
            t.fill_(0x77)
        return w

    def issue(self):
        d = self.dev
        d.codebook_build(self.hist.data_ptr(), self.cb.data_ptr())
        d.header_write(self.cb.data_ptr(), HEAD_N, HEAD_LAST, self.head.data_ptr(), HEAD_CAP, self.info.data_ptr())
        d.header_parse(self.file.data_ptr(), self.flen, self.cb2.data_ptr(), self.pinfo.data_ptr())

    def snapshot(self):
        """What the three calls wrote, on the host (taken in stream order, no synchronisation)."""
        return [t.clone() for t in (self.cb, self.info, self.headbuf, self.cb2, self.pinfo)]

    def check(self, ck, t, w, snap, hz):
        cb_t, info, headbuf, cb2_t, pinfo = snap
        got = self.Codebook.from_buffer_copy(cb_t.cpu().numpy().tobytes())
        oa, la, ca = hz.codebook_arrays(got)
        ob, lb, cbb = hz.codebook_arrays(w.cb)
        ck.expect(t + " codebook", (got.nsym, got.max_len, got.min_len) == (w.cb.nsym, w.cb.max_len, w.cb.min_len)
                  and np.array_equal(oa, ob) and np.array_equal(la, lb) and np.array_equal(ca, cbb))
        nb, pbits, pend, bits = [int(v) for v in info.cpu()]
        head = headbuf[GUARD:GUARD + HEAD_CAP].cpu().numpy()
        ck.expect(t + " header", (nb, pbits, bits) == (len(w.head), w.pbits, 8 * len(w.head) + w.pbits)
                  and head[:len(w.head)].tobytes() == w.head, str((nb, pbits, bits)))
        if w.pbits:
            ck.expect(t + " pending bits", pend >> (8 - pbits) == w.pend >> (8 - w.pbits) if pbits else False)
        ck.expect(t + " header guards", bool((headbuf[:GUARD] == 0xA5).all()) and bool((headbuf[GUARD + HEAD_CAP:] == 0xA5).all()))
        dev = self.Codebook.from_buffer_copy(cb2_t.cpu().numpy().tobytes())
        order, ln, code, oinfo = w.parse
        u = len(order)
        dcode = np.frombuffer(dev.code, dtype=np.uint64)
        ck.expect(t + " parse", dev.nsym == u and [int(v) for v in pinfo.cpu()] == oinfo
                  and np.array_equal(np.frombuffer(dev.order, dtype=np.uint16)[:u], order)
                  and np.array_equal(np.frombuffer(dev.len, dtype=np.uint8), ln) and np.array_equal(dcode[ln > 0], code[ln > 0])
                  and dev.max_len == int(ln.max()) and dev.min_len == int(ln[ln > 0].min()))


CB_EAGER = ["zipf21", "three", "one", "zipf21"]
CB_REPLAY = ["three", "zipf21"]      # after the eager run and the capture on zipf21: U = 65 536 -> 3 -> 65 536


@gpu
def test_codebook_workspace_eager(codec, hz):
    """k_cb_*, k_hw_* and k_hdr_* share one workspace: U = 65 536, then 3 symbols, then 1, then 65 536 again on
    one context without a synchronisation in between (each run's results are copied aside in stream order)."""
    r = CbRig(codec, hz)
    ck = Checks(codec)
    snaps = []
    for name in CB_EAGER:
        w = r.load(name)
        r.issue()
        snaps.append((name, w, r.snapshot()))
    ck.run("the four runs", lambda: None)
    for i, (name, w, snap) in enumerate(snaps):
        r.check(ck, "run %d (%s)" % (i, name), w, snap, hz)
    assert not ck.failed, "\n".join(ck.failed)


@gpu
def test_codebook_workspace_replayed(codec, hz):
    """The three calls captured as one graph on the zipf21 histogram; replayed on the 3-symbol histogram and on
    zipf21 again: only the histogram and the header file's bytes change, in place."""
    import torch
    r = CbRig(codec, hz)
    ck = Checks(codec)
    w = r.load("zipf21")
    ck.run("eager", r.issue)
    r.check(ck, "eager (zipf21)", w, r.snapshot(), hz)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=codec.stream):
        r.issue()
    for name in CB_REPLAY:
        w = r.load(name)
        torch.cuda.synchronize()
        ck.run("replay on %s" % name, g.replay)
        torch.cuda.synchronize()
        r.check(ck, "replay on %s" % name, w, r.snapshot(), hz)
    assert not ck.failed, "\n".join(ck.failed)


# ---- part 2: capture on A, replay on B, replay on A ----------------------------------------------------------
def _replay(r, name):
    """Eager on A (scratch and kernel attributes in place), captured on A, replayed on B and then on A."""
    import torch
    ck = Checks(r.codec)
    issue, check = CALLS[name]
    s = r.load("A")
    t = "%s eager on A" % name
    ck.run(t, lambda: issue(r))
    check(r, ck, t, s)
    r.load("A")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=r.codec.stream):    # a host synchronisation inside would break the capture
        issue(r)
    for w in "BA":
        s = r.load(w)                                   # the device buffers are all the replay reads
        torch.cuda.synchronize()
        t = "%s captured on A, replayed on %s" % (name, w)
        ck.run(t, g.replay)
        torch.cuda.synchronize()
        check(r, ck, t, s)
        if name not in PRODUCERS:
            ck.expect(t + ": payload (an input) changed", r.payload_unchanged(s))
    return ck.failed


@gpu
@pytest.mark.parametrize("name", list(REPLAYED))
def test_replay_on_the_other_stream(codec, name):
    p = pair(name)
    r = Rig(codec, p, pieces="pieces" in REPLAYED[name])
    failed = []
    for call in REPLAYED[name]:
        failed += _replay(r, call)
    assert not failed, "\n".join(failed)


# ---- no lead-in: nearly every chain takes the fix-up and head paths -------------------------------------------
@gpu
def test_fixups_without_lead_in(built_lib):
    """HZ_SEG_LEAD=0 (test hook, read once: a fresh process): the `records` and `no-resync` pairs through
    hz_decode_indexless and hz_seek_build in both orders. Without a lead-in a chain starts synchronised only
    where its first bit happens to start a codeword -- one bit in two of the right parity under `even` (mean
    length 4, every length even), one in five or fewer under zipf21 -- so about half and about four fifths of
    the 42 seek entries lie in chains that got a head; k_chain_seek's own counter (hz_debug_seek_stats) must
    say so for at least a quarter of them after every hz_seek_build, in both runs of each order."""
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "nolead"], capture_output=True, text=True,
                         timeout=300, env=dict(os.environ, HZ_SEG_LEAD="0"))
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stdout + res.stderr


def _headed_entries(codec):
    """Entries the context's last k_chain_seek found in a chain that has a head."""
    from huffman_amd import load
    out = (ctypes.c_uint64 * 4)()
    assert load().hz_debug_seek_stats(codec.dev.h, out) == 0
    return int(out[3])


def _main_nolead(c):
    bad = []
    for name in NOLEAD_PAIRS:
        r = Rig(c, pair(name), pieces=False)
        for order in ORDERS:
            bad += _eager(r, "indexless", order)
            ck = Checks(c)
            for w in order:
                s = r.load(w)
                t = "seek_build on %s (order %s)" % (w, order)
                ck.run(t, lambda: _i_seek_build(r))
                _k_seek_build(r, ck, t, s)
                headed = _headed_entries(c)
                print(name, t, "entries in headed chains:", headed)
                ck.expect(t + " headed chains", headed >= (r.p.nb + 1) // 4, str(headed))
                ck.expect(t + ": payload (an input) changed", r.payload_unchanged(s))
            bad += ck.failed
    return bad


if __name__ == "__main__":
    assert sys.argv[1:] == ["nolead"] and os.environ.get("HZ_SEG_LEAD") == "0", sys.argv
    from huffman_amd.pipeline import StreamCodec
    _bad = _main_nolead(StreamCodec(0))
    if _bad:
        print("\n".join(_bad))
        sys.exit(1)
    print("ok")
