"""hz_decode_ranges_pieces on the device: a batch of ranges decoded from gathered pieces -- only the
payload bytes and seek words each range needs, in one small buffer -- and the host and file forms on
top of it (hz_decode_ranges_host_pieces, hz_decode_ranges_file).

The gathered buffer is built HERE from a stream's payload and hz_seek_pieces' plan: random bytes before,
between and after the pieces (and in the compact table's unused words), so a read outside a piece cannot
look right by accident. Outputs follow tests/test_gpu_ranges_batch.py: one 0xA5 buffer per call, compared
as a whole with its expected image. Tolerance: none -- every check is bit-exact.

Run as a script (`python tests/test_gpu_ranges_pieces.py cold`) it runs the edge case with every block on
the cold path and prints "ok": the test starts it in a fresh process to set HZ_RANGES_SLOT_WORDS, which
the library reads once."""
import glob
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_designed_streams as tds  # noqa: E402
import test_gpu_range as tgr  # noqa: E402
import test_gpu_ranges_batch as trb  # noqa: E402
from table_books import book  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden")
BLK = 2048
PAD = 256            # random bytes before and after the gathered buffer (keeps its 256-byte alignment)
HZ_EINVAL, HZ_EFORMAT, HZ_ENOENT = -1, -5, -10
HZ_POS_LIMIT = (1 << 64) - 1 - 0xFFFF
nblk = trb.nblk


@pytest.fixture(scope="module")
def hz(built_lib):
    import huffman_amd
    return huffman_amd


@pytest.fixture(scope="module")
def codec(built_lib):
    from huffman_amd.pipeline import StreamCodec
    return StreamCodec(0)


# ---- the gathered form of a list of ranges ------------------------------------------------------------
def plan_of(hz, s, ranges, offs):
    """hz_seek_pieces' plan for ranges [(sym_begin, sym_count)] at out_bytes offs, as plain lists: pieces
    (six numbers each), what each holds (the payload's bytes), the ranges (four numbers each) and the
    compact table."""
    seek = s.seek.cpu().numpy().view(np.uint64)
    pay = s.payload.cpu().numpy()
    pieces, out, bb, sw = hz.seek_pieces(seek, s.nsym, pay.size, [(b, c, o) for (b, c), o in zip(ranges, offs)])
    pl = SimpleNamespace(pieces=[[int(v) for v in p] for p in pieces], ranges=[[int(v) for v in r] for r in out],
                         buf_bytes=bb, seek_words=sw)
    pl.contents = [pay[p[0]:p[0] + p[1]].copy() for p in pl.pieces]
    pl.tables = [seek[p[3]:p[3] + p[5] + 1].copy() for p in pl.pieces]
    assert all(c.size == p[1] for c, p in zip(pl.contents, pl.pieces))
    return pl


def relayout(pl, delta):
    """Every piece at a new buf_byte with (buf_byte - stream_byte) % 64 == delta, in order, 64-byte gaps."""
    end = 0
    for p in pl.pieces:
        p[2] = (end + 63) // 64 * 64 + (p[0] + delta) % 64
        end = p[2] + p[1]
    pl.buf_bytes = (end + 15) // 16 * 16


def on_device(pl, seed=1):
    """The plan as device tensors: buf (a view PAD bytes into a larger random buffer), seek, pieces, ranges."""
    import torch
    rng = np.random.default_rng(seed)
    host = rng.integers(0, 256, PAD + pl.buf_bytes + PAD, dtype=np.uint8)
    words = rng.integers(0, 1 << 62, max(pl.seek_words, 1)).astype(np.uint64)
    for p, c, t in zip(pl.pieces, pl.contents, pl.tables):
        host[PAD + p[2]:PAD + p[2] + p[1]] = c
        words[p[4]:p[4] + p[5] + 1] = t
    as_i64 = lambda rows, cols: torch.from_numpy(  # noqa: E731
        np.array([[v & ((1 << 64) - 1) for v in r] for r in rows] or [[0] * cols], dtype=np.uint64).view(np.int64)).cuda()
    hold = torch.from_numpy(host).cuda()
    return SimpleNamespace(hold=hold, buf=hold[PAD:PAD + pl.buf_bytes], seek=torch.from_numpy(words.view(np.int64)).cuda(),
                           pieces=as_i64(pl.pieces, 6), ranges=as_i64(pl.ranges, 4))


def launch(codec, s, g, size):
    """One hz_decode_ranges_pieces call into a fresh 0xA5 buffer; (buffer, stats), not yet synchronised."""
    import torch
    out = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    stats = torch.full((4,), -1, dtype=torch.int64, device="cuda")   # the call zeroes them
    codec.decode_ranges_pieces(g.buf, g.seek, g.pieces, s.nsym, g.ranges, out, stats=stats)
    return out, stats


def same(got, exp, what=""):
    import torch
    if not torch.equal(got, exp):
        bad = int(torch.nonzero(got != exp)[0])
        raise AssertionError(f"first differing byte {bad} of {exp.numel()} {what}")


def check(codec, hz, s, ranges, skip=(), seed=1, change=None):
    """Plans, gathers, runs, synchronises and compares the whole buffer; returns (stats list, plan)."""
    offs, size = trb.layout(ranges)
    pl = plan_of(hz, s, ranges, offs)
    if change:
        change(pl)
    out, stats = launch(codec, s, on_device(pl, seed), size)
    codec.sync()
    same(out, trb.image(s, ranges, offs, size, skip))
    return [int(v) for v in stats.cpu()], pl


def fails(codec, hz, s, g, ranges, offs, size, status, skip):
    """A run that reports `status` at the sync: everything but the ranges in `skip` is decoded."""
    out, stats = launch(codec, s, g, size)
    with pytest.raises(hz.HZError) as e:
        codec.sync()
    assert e.value.status == status
    same(out, trb.image(s, ranges, offs, size, skip))
    return [int(v) for v in stats.cpu()]


# ---- 1. edges on the smallest stream that has them ----------------------------------------------------
@pytest.fixture(scope="module")
def small(codec):
    return tgr._zipf(codec, 5 * 4096 + 6)


@pytest.fixture(scope="module")
def zipf8(codec):
    return tgr._zipf(codec, tgr.ZIPF_N)


TWO_PIECES = [(5, 10), (2047, 2), (5 * BLK, 3), (5 * BLK - 1, 2), (7, 0), (100, 1900)]   # blocks 0 - 1 and 4 - 5


def edges_check(codec, hz, s, cold=False):
    assert s.nsym == 5 * BLK + 3 and s.nb == 6
    codec.upload_decode(s.plan)
    ranges = trb.edge_list(s.nsym)
    st, pl = check(codec, hz, s, ranges)
    assert st[0] == sum(nblk(b, c) for b, c in ranges), st
    assert st[3] == 0 and 0 <= st[2] <= 64, st
    assert st[1] == (st[0] if cold else 0), st
    for delta in (4, 47):                          # the stream's first piece off the 16-byte grid (the cold reader's chunks)
        st, pl = check(codec, hz, s, ranges, change=lambda pl: relayout(pl, delta), seed=delta)
        assert st[3] == 0 and st[1] == (st[0] if cold else 0) and st[0] == sum(nblk(b, c) for b, c in ranges), st
    st, pl = check(codec, hz, s, TWO_PIECES)       # and a list that leaves the middle of the stream out
    assert len(pl.pieces) == 2 and pl.pieces[0][0] == 0 and pl.pieces[1][0] > 0
    assert st[0] == sum(nblk(b, c) for b, c in TWO_PIECES) and st[3] == 0 and st[1] == (st[0] if cold else 0), st


def test_edges_smallest_stream(codec, hz, small):
    edges_check(codec, hz, small)


# ---- 2. equal to the hull form, more jobs than waves ----------------------------------------------------
def test_equal_to_the_hull_form(codec, hz, zipf8):
    s = zipf8
    assert s.nb == 2049
    codec.upload_decode(s.plan)
    ranges = tgr._random_ranges(s.nsym)
    assert len(ranges) == 40 and sum(nblk(b, c) for b, c in ranges) > 16 * 512
    offs, size = trb.layout(ranges)
    hull, _, hstats = trb.run(codec, s, ranges, False, offs=offs, size=size)
    out, stats = launch(codec, s, on_device(plan_of(hz, s, ranges, offs)), size)
    codec.sync()
    same(out, hull)
    same(out, trb.image(s, ranges, offs, size))
    assert [int(v) for v in stats.cpu()] == [int(v) for v in hstats.cpu()]
    # scattered single blocks: many pieces, a few table words each
    scattered = [(b * BLK + b % 1000, 300) for b in range(3, 2040, 97)]
    st, pl = check(codec, hz, s, scattered)
    assert len(pl.pieces) == len(scattered) and st[0] == len(scattered) and st[3] == 0
    assert 20 * pl.buf_bytes < s.payload.numel()


# ---- 3. every table mode -------------------------------------------------------------------------------
@pytest.mark.parametrize("start_bit", [0, 45])
@pytest.mark.parametrize("kind", ["longest", "uniform"])
@pytest.mark.parametrize("name", tds.BOOKS)
def test_table_modes(codec, hz, name, kind, start_bit):
    bk = book(name)
    nsym = 40 * BLK + 777
    rng = np.random.default_rng([tds.BOOKS.index(name), len(kind), start_bit])
    s = trb.model_stream(bk, tds._stream(bk, kind, nsym, rng), start_bit, tds._lead(start_bit))
    codec.dev.upload_decode(bk.cb)
    ranges = tgr._eight_ranges(nsym, 5)
    st, _ = check(codec, hz, s, ranges)
    assert st[0] == sum(nblk(b, c) for b, c in ranges) and st[3] == 0, st
    if name == "fib57" and kind == "longest":   # a block of 2048 x 56 bits fits no slot: the cold path, through a piece view
        assert st[1] >= 1, st


# ---- 4. alignment -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [0, 1, 4, 16, 47, 63])
def test_alignment(codec, hz, small, delta):
    """(buf_byte - stream_byte) % 64 == delta for every piece; 47 makes head < r in the view's arithmetic
    (the borrow). The second list has a piece that does not start the stream."""
    s = small
    codec.upload_decode(s.plan)
    for ranges in (trb.edge_list(s.nsym), TWO_PIECES):
        st, pl = check(codec, hz, s, ranges, change=lambda pl: relayout(pl, delta), seed=delta + 2)
        assert all((p[2] - p[0]) % 64 == delta for p in pl.pieces)
        assert st[0] == sum(nblk(b, c) for b, c in ranges) and st[3] == 0, st


# ---- 5. the cold path on ordinary data ----------------------------------------------------------------
def test_cold_path_on_ordinary_data(built_lib):
    """HZ_RANGES_SLOT_WORDS=4: no staging window fits, so every job of case 1 goes cold, through its piece's view."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "cold"], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, HZ_RANGES_SLOT_WORDS="4"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ---- 6. far positions ---------------------------------------------------------------------------------------
def move_far(pl, base):
    """The plan as pieces of a stream `base` bytes (a multiple of 64) longer in front: every stream_byte and
    seek word moved up. The piece that started the stream now lies inside one, so it takes 64 bytes of lead
    (tests/test_gpu_far_offsets.py LEAD_PAD), which nothing decodes."""
    assert base % 64 == 0
    for k, p in enumerate(pl.pieces):
        if p[0] == 0:
            pl.contents[k] = np.concatenate([np.full(64, 0x3C, np.uint8), pl.contents[k]])
            p[0], p[1] = base - 64, p[1] + 64
        else:
            p[0] += base
        pl.tables[k] = pl.tables[k] + np.uint64(8 * base)
    relayout(pl, 0)


@pytest.mark.parametrize("base", [(1 << 32) + 64, (1 << 45) + 4096], ids=["bit2p35", "bit2p48"])
def test_far_positions(codec, hz, small, base):
    s = small
    codec.upload_decode(s.plan)
    assert 8 * base > (1 << 35)
    for ranges in (trb.edge_list(s.nsym), TWO_PIECES):
        st, pl = check(codec, hz, s, ranges, change=lambda pl: move_far(pl, base))   # the base-0 image
        assert min(p[0] for p in pl.pieces) >= base - 64
        assert st[0] == sum(nblk(b, c) for b, c in ranges) and st[3] == 0, st


@pytest.mark.parametrize("how", ["limit", "wraps"])
def test_position_limit(codec, hz, small, how):
    """A piece whose 8 * (stream_byte + bytes) reaches HZ_POS_LIMIT, or leaves 64 bits: its ranges are
    refused in the plan (no block is flagged), the other piece's are decoded."""
    s = small
    codec.upload_decode(s.plan)
    offs, size = trb.layout(TWO_PIECES)
    pl = plan_of(hz, s, TWO_PIECES, offs)
    g = on_device(pl)
    max_byte = (HZ_POS_LIMIT - 1) // 8           # the largest stream_byte + bytes with 8 x it below the limit
    far = max_byte - pl.pieces[1][1] + 1 if how == "limit" else -64
    g.pieces[1, 0] = far
    ok = [i for i, r in enumerate(pl.ranges) if r[3] == 0 or r[1] == 0]
    skip = set(range(len(TWO_PIECES))) - set(ok)
    assert skip == {2, 3}
    st = fails(codec, hz, s, g, TWO_PIECES, offs, size, HZ_EINVAL, skip)
    assert st[3] == 0 and st[0] == sum(nblk(*TWO_PIECES[i]) for i in ok), st
    if how == "limit":      # one byte lower it is an ordinary (if absurd) position: the blocks are outside it
        g.pieces[1, 0] = far - 1
        st = fails(codec, hz, s, g, TWO_PIECES, offs, size, HZ_EINVAL, skip)
        assert st[3] == sum(nblk(*TWO_PIECES[i]) for i in skip), st
    check(codec, hz, s, TWO_PIECES)


# ---- 7. refusals found on the device ---------------------------------------------------------------------
def four(s):
    return [(0, 3000), (700 * BLK + 5, 100), (1500 * BLK, 2 * BLK), (s.nsym - 5, 5), (9, 0)]


@pytest.mark.parametrize("bad", ["piece", "buf", "seek", "block", "odd", "out"])
def test_refused_ranges(codec, hz, zipf8, bad):
    s = zipf8
    codec.upload_decode(s.plan)
    ranges = four(s)
    offs, size = trb.layout(ranges)
    if bad == "odd":
        offs[1] += 1
    if bad == "out":
        offs[1] = size - 50       # 200 bytes from 50 before the buffer's end
    pl = plan_of(hz, s, ranges, offs)
    assert len(pl.pieces) == 4 and [r[3] for r in pl.ranges] == [0, 1, 2, 3, 0]
    g = on_device(pl)
    p1 = pl.pieces[1]
    if bad == "piece":
        g.ranges[1, 3] = 4                                   # piece >= npieces
    if bad == "buf":
        g.pieces[1, 1] = pl.buf_bytes - p1[2] + 1            # buf_byte + bytes > buf_bytes
    if bad == "seek":
        g.pieces[1, 4] = pl.seek_words - p1[5]               # seek_index + nblocks + 1 > seek_words
    if bad == "block":
        ranges[1] = ((p1[3] + p1[5]) * BLK + 5, 100)         # one block past the piece's blocks
        g.ranges[1, 0] = ranges[1][0]
    st = fails(codec, hz, s, g, ranges, offs, size, HZ_EINVAL, {1})
    assert st[3] == 0 and st[0] == sum(nblk(*ranges[i]) for i in (0, 2, 3)), st
    check(codec, hz, s, four(s))                             # the context is usable afterwards


def test_short_piece_and_moved_word(codec, hz, zipf8):
    s = zipf8
    codec.upload_decode(s.plan)
    ranges = four(s)
    offs, size = trb.layout(ranges)
    pl = plan_of(hz, s, ranges, offs)
    g = on_device(pl)
    g.pieces[2, 1] -= 48                  # the last block's margins are missing: that block alone is flagged
    out, stats = launch(codec, s, g, size)
    with pytest.raises(hz.HZError) as e:
        codec.sync()
    assert e.value.status == HZ_EINVAL
    exp = trb.image(s, ranges, offs, size)
    exp[offs[2] + 2 * BLK:offs[2] + 4 * BLK] = 0xA5
    same(out, exp)
    st = [int(v) for v in stats.cpu()]
    assert st[3] == 1 and st[0] == sum(nblk(*r) for r in ranges) - 1, st
    # a moved word of the compact table: block b starts one bit late, and that block alone stores nothing
    b = trb._moved_entry(s)
    ranges = [(0, 10), (b * BLK + 5, 100), ((b + 5) * BLK, BLK), ((b + 10) * BLK - 3, 6)]
    offs, size = trb.layout(ranges)
    pl = plan_of(hz, s, ranges, offs)
    assert pl.pieces[1][3] == b and pl.pieces[1][5] == 1
    g = on_device(pl)
    g.seek[pl.pieces[1][4]] += 1
    st = fails(codec, hz, s, g, ranges, offs, size, HZ_EFORMAT, {1})
    assert st[3] == 1 and st[0] == sum(nblk(*r) for r in ranges) - 1, st
    check(codec, hz, s, ranges)


# ---- 8. cheap checks at the call -----------------------------------------------------------------------------
def test_cheap_checks_at_the_call(codec, hz, small):
    import torch
    s = small
    codec.upload_decode(s.plan)
    pl = plan_of(hz, s, [(0, 1)], [0])
    g = on_device(pl)
    out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    stats = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    lib, h = codec.dev.lib, codec.dev.h
    good = dict(buf=g.buf.data_ptr(), seek=g.seek.data_ptr(), pieces=g.pieces.data_ptr(), ranges=g.ranges.data_ptr(),
                out=out.data_ptr(), flags=0, h=h, n=1, stats=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.hz_decode_ranges_pieces(a["h"], a["buf"], g.buf.numel(), a["seek"], g.seek.numel(), a["pieces"], 1,
                                           s.nsym, a["ranges"], a["n"], a["out"], 4096, a["stats"], a["flags"])

    for kw in (dict(buf=None), dict(seek=None), dict(pieces=None), dict(ranges=None), dict(out=None), dict(h=None),
               dict(flags=1), dict(flags=2), dict(out=out.data_ptr() + 1), dict(buf=g.buf.data_ptr() + 1),
               dict(buf=g.buf.data_ptr() + 2)):
        assert call(**kw) == HZ_EINVAL, kw
    assert call(n=0, stats=stats.data_ptr()) == 0          # nothing launched: d_stats untouched
    assert call() == 0                                     # d_stats may be null
    codec.sync()
    assert [int(v) for v in stats.cpu()] == [-1] * 4
    assert int(out[2:].sum().item()) == 0 and torch.equal(out[:2], s.x[:2])
    from huffman_amd import Device
    torch.cuda.synchronize()
    dev = Device(0)              # no decode tables
    try:
        assert call(h=dev.h) == HZ_EINVAL
    finally:
        dev.close()


# ---- 9. graph capture ----------------------------------------------------------------------------------------
def test_graph_capture(codec, hz, zipf8):
    import torch
    s = zipf8
    codec.upload_decode(s.plan)
    first = [(3 * BLK + 11, 5 * BLK + 77), (0, 1), (s.nsym - 1, 1), (2047, 2), (900 * BLK, BLK), (17, 4000), (1500 * BLK - 9, 18),
             (7, 0)]
    other = [(1200 * BLK + 1, 3 * BLK), (5, 5), (s.nsym - 3 * BLK, 3 * BLK), (1, 0), (640 * BLK - 1, 2), (3, 0), (4, 0), (6, 0)]
    third = [(77 * BLK + 100, 6000), (2048, 2048), (9, 0), (10, 0), (11, 0), (12, 0), (13, 0), (s.nsym - 2, 1)]
    lists = [first, other, third]
    lay = [trb.layout(r) for r in lists]
    size = max(n for _, n in lay)
    plans = [plan_of(hz, s, r, o) for r, (o, _) in zip(lists, lay)]
    assert len({len(p.pieces) for p in plans}) == 3           # a different number of live pieces each
    gs = [on_device(p, seed=20 + i) for i, p in enumerate(plans)]
    cap_buf, cap_words = max(p.buf_bytes for p in plans) + 64, max(p.seek_words for p in plans) + 3
    buf = torch.zeros(cap_buf, dtype=torch.uint8, device="cuda")
    seek = torch.zeros(cap_words, dtype=torch.int64, device="cuda")
    pieces = torch.zeros((8, 6), dtype=torch.int64, device="cuda")
    rgs = torch.zeros((8, 4), dtype=torch.int64, device="cuda")
    out = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")

    def load(i):
        g = gs[i]
        buf.copy_(torch.randint(0, 256, (cap_buf,), dtype=torch.uint8, device="cuda"))
        buf[:g.buf.numel()] = g.buf
        seek.fill_(-1)
        seek[:g.seek.numel()] = g.seek
        pieces.fill_(-1)                                      # pieces not in use: nothing names them
        pieces[:len(plans[i].pieces)] = g.pieces[:len(plans[i].pieces)]
        rgs.copy_(g.ranges)
        out.fill_(0xA5)

    def call():
        codec.decode_ranges_pieces(buf, seek, pieces, s.nsym, rgs, out, stats=stats)

    load(0)
    call()  # eager: also sizes the scratch
    codec.sync()
    same(out, trb.image(s, first, lay[0][0], size))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=codec.stream):  # a host synchronisation inside would break the capture
        call()
    for i in (0, 1, 2):
        load(i)                                         # the device arrays are all the replay reads
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        same(out, trb.image(s, lists[i], lay[i][0], size), f"replay {i}")
        assert int(stats[0]) == sum(nblk(b, c) for b, c in lists[i]) and int(stats[3]) == 0
    codec.sync()


# ---- 10. host and file forms -------------------------------------------------------------------------------------
def _pieces_of_pairs(hz, blob, seek, pairs):
    """The plan the host flow makes for byte ranges: the covering symbols of every pair."""
    _, info = hz.parse_header(blob)
    nsym = info.n // 2
    rows = []
    for off, cnt in pairs:
        s0, s1 = off // 2, min((off + cnt + 1) // 2, nsym)
        rows.append((s0, s1 - s0 if cnt and s1 > s0 else 0, 0))
    pieces, _, bb, sw = hz.seek_pieces(seek, nsym, len(blob) - info.payload_byte, rows)
    return info, pieces, bb, sw


def test_host_and_file_forms(hz, tmp_path):
    rng = np.random.default_rng(77)
    data = np.minimum(rng.zipf(1.3, 150 * 1024).astype(np.uint64), 2000).astype("<u2").view(np.uint8).tobytes() + b"\x5b"
    n = len(data)
    assert n % 2 == 1 and n > 300 * 1024
    blob = hz.encode(data)
    seek = hz.build_seek(blob)
    path = tmp_path / "image.compressed"
    path.write_bytes(blob)
    pairs = [(200001, 4097), (1, 1), (n - 1, 1), (4095, 3), (100 * 1024, 8192), (n - 3, 3), (5, 0), (n, 0), (200001, 4097),
             (n // 2 | 1, 4098), (1, 1), (250000, 2)]
    want = [data[o:o + c] for o, c in pairs]
    assert hz.decode_ranges(blob, seek, pairs) == want
    assert hz.decode_ranges(blob, seek, pairs, pieces=True) == want
    assert hz.decode_ranges_file(str(path), seek, pairs) == want
    assert hz.decode_ranges_file(str(path), seek, []) == [] and hz.decode_ranges(blob, seek, [], pieces=True) == []
    assert hz.decode_ranges_file(str(path), seek, [(n - 1, 1), (7, 0)]) == [data[n - 1:], b""]   # no symbol at all
    # nothing outside the pieces bears on the result
    info, pieces, bb, sw = _pieces_of_pairs(hz, blob, seek, pairs)
    pay = len(blob) - info.payload_byte
    assert 1 < len(pieces) < len(pairs) and 2 * bb < pay
    keep = np.zeros(len(blob), dtype=bool)
    keep[:info.payload_byte + (1 if info.payload_bit else 0)] = True     # the header, its last bits included
    for p in pieces:
        keep[info.payload_byte + int(p["stream_byte"]):info.payload_byte + int(p["stream_byte"]) + int(p["bytes"])] = True
    holed = np.where(keep, np.frombuffer(blob, dtype=np.uint8), 0xFF).astype(np.uint8)
    assert int((~keep).sum()) > pay // 2
    copy = tmp_path / "holed.compressed"
    copy.write_bytes(holed.tobytes())
    assert hz.decode_ranges_file(str(copy), seek, pairs) == want
    assert hz.decode_ranges(holed, seek, pairs, pieces=True) == want
    # refusals
    with pytest.raises(hz.HZError) as e:
        hz.decode_ranges_file(str(tmp_path / "absent.compressed"), seek, pairs)
    assert e.value.status == HZ_ENOENT
    for past in ([(0, 1), (n, 1)], [(n + 1, 0)], [(n - 1, 2)]):
        for form in (lambda r: hz.decode_ranges_file(str(path), seek, r), lambda r: hz.decode_ranges(blob, seek, r, pieces=True)):
            with pytest.raises(hz.HZError) as e:
                form(past)
            assert e.value.status == HZ_EINVAL
    far = seek + np.uint64(8 * len(blob))          # a table of some longer payload: the spans start past this one's end
    with pytest.raises(hz.HZError) as e:
        hz.decode_ranges_file(str(path), far, [(4096, 10)])
    assert e.value.status == HZ_EFORMAT


BASELINES = sorted(glob.glob(os.path.join(GOLD, "*.baseline.compressed")))


def test_reference_written_file(hz):
    assert BASELINES
    for comp in BASELINES:
        with open(comp[:-len(".baseline.compressed")], "rb") as f:
            data = f.read()
        with open(comp, "rb") as f:
            blob = f.read()
        n = len(data)
        seek = hz.build_seek(blob)
        pairs = [(o, min(c, n - o)) for o, c in [(n - 1, 1), (1, 1), (4095, 3), (n // 2, 1000), (n - 3, 3), (0, 7)]]
        want = [data[o:o + c] for o, c in pairs]
        assert hz.decode_ranges_file(comp, seek, pairs) == want, comp
        assert hz.decode_ranges(blob, seek, pairs, pieces=True) == want, comp


# ---- 11. names exported ------------------------------------------------------------------------------------------
def test_names_exported(hz):
    from huffman_amd import _lib
    lib = hz.load()
    names = {name for name, _, _ in _lib.PROTOTYPES}
    for name in ("hz_decode_ranges_pieces", "hz_seek_pieces", "hz_decode_ranges_host_pieces", "hz_decode_ranges_file"):
        assert name in names and hasattr(lib, name)
    for name in ("seek_pieces", "decode_ranges_file"):
        assert name in hz.__all__ and callable(getattr(hz, name))
    import ctypes
    assert ctypes.sizeof(_lib.Piece) == 48 and ctypes.sizeof(_lib.PieceRange) == 32


if __name__ == "__main__":
    assert sys.argv[1:] == ["cold"], sys.argv
    import huffman_amd as _hz
    from huffman_amd.pipeline import StreamCodec
    _c = StreamCodec(0)
    edges_check(_c, _hz, tgr._zipf(_c, 5 * 4096 + 6), cold=True)
    print("ok")
