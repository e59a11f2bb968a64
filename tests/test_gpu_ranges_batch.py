"""hz_decode_ranges on the device: many ranges of one stream in one call, a wave per block, from the
seek table (the cooperative walk) and from a full index; the cold path, the many-round walk, payload
slices, wrong tables and wrong ranges, graph capture with the ranges replaced between replays, and
the host forms.

Every decode lands in ONE buffer filled with 0xA5: range i sits at an out_byte that cycles through
0, 2 and 14 modulo 16, with at least 64 untouched bytes between neighbours, and the whole buffer is
compared with its expected image (the input's bytes, or for foreign books the model's symbols), so
every byte outside the ranges must still be 0xA5. Tolerance: none -- every check is bit-exact.

Run as a script (`python tests/test_gpu_ranges_batch.py cold`) it runs the edge case with every
block on the cold path and prints "ok": the test starts it in a fresh process to set
HZ_RANGES_SLOT_WORDS, which the library reads once."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ranges_model  # noqa: E402
import ref_stream  # noqa: E402
import test_gpu_designed_streams as tds  # noqa: E402
import test_gpu_range as tgr  # noqa: E402
import test_ranges_model as trm  # noqa: E402
from table_books import book  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden")
BLK = 2048
GAP = 64
HZ_EINVAL, HZ_EFORMAT = -1, -5


@pytest.fixture(scope="module")
def hz(built_lib):
    import huffman_amd
    return huffman_amd


@pytest.fixture(scope="module")
def codec(built_lib):
    from huffman_amd.pipeline import StreamCodec
    return StreamCodec(0)


def nblk(begin, count):
    return 0 if count == 0 else (begin + count - 1) // BLK - begin // BLK + 1


def layout(ranges):
    """out_byte of every range (cycling through 0, 2 and 14 modulo 16, 64 or more untouched bytes between
    neighbours and at both ends) and the buffer's size."""
    offs, cur = [], GAP
    for i, (_, count) in enumerate(ranges):
        off = (cur + 15) // 16 * 16 + (0, 2, 14)[i % 3]
        offs.append(off)
        cur = off + 2 * count + GAP
    return offs, cur + 16


def run(codec, s, ranges, full, payload=None, base=0, table=None, offs=None, size=None):
    """One hz_decode_ranges call of `ranges` [(sym_begin, sym_count)] into a fresh 0xA5 buffer; returns
    (buffer, out_bytes, stats tensor), not yet synchronised."""
    import torch
    if offs is None:
        offs, size = layout(ranges)
    buf = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    rows = [[b, c, o] for (b, c), o in zip(ranges, offs)]
    rg = torch.tensor(rows, dtype=torch.int64, device="cuda").reshape(-1, 3)
    stats = torch.full((4,), -1, dtype=torch.int64, device="cuda")   # the call zeroes them
    pay = s.payload if payload is None else payload
    if table is None:
        table = s.index if full else s.seek
    codec.decode_ranges(pay, s.nsym, table, rg, buf, stats=stats, full_index=full, payload_byte_base=base)
    return buf, offs, stats


def image(s, ranges, offs, size, skip=()):
    """The expected buffer: 0xA5 but for the ranges' bytes (ranges in `skip` write nothing)."""
    import torch
    exp = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    for i, ((b, c), o) in enumerate(zip(ranges, offs)):
        if i not in skip and c:
            exp[o:o + 2 * c] = s.x[2 * b:2 * (b + c)]
    return exp


def check(codec, s, ranges, full, skip=(), **kw):
    """Runs the batch, synchronises, compares the whole buffer; returns the stats as a list."""
    import torch
    offs, size = layout(ranges)
    buf, offs, stats = run(codec, s, ranges, full, offs=offs, size=size, **kw)
    codec.sync()
    exp = image(s, ranges, offs, size, skip)
    if not torch.equal(buf, exp):
        bad = int(torch.nonzero(buf != exp)[0])
        raise AssertionError(f"first differing byte {bad} of {size}; offsets {offs[:12]}; full={full}")
    return [int(v) for v in stats.cpu()]


# ---- 1. edges on the smallest stream that has them ------------------------------------------
def edge_list(nsym):
    e = tgr._edge_ranges(nsym, 5 * BLK)
    assert len(e) == 11 and (7, 0) in e
    return list(reversed([r for r in e for _ in (0, 1)]))   # each of them twice, the list reversed


def edges_check(codec, s, cold=False):
    assert s.nsym == 5 * BLK + 3 and s.nb == 6
    codec.upload_decode(s.plan)
    ranges = edge_list(s.nsym)
    for full in (False, True):
        st = check(codec, s, ranges, full)
        assert st[0] == sum(nblk(b, c) for b, c in ranges), st
        assert st[3] == 0 and 0 <= st[2] <= 64, st
        assert st[1] == (st[0] if cold else 0), st


@pytest.fixture(scope="module")
def small(codec):
    return tgr._zipf(codec, 5 * 4096 + 6)


def test_edges_smallest_stream(codec, small):
    edges_check(codec, small)


# ---- 2. more jobs than waves ------------------------------------------------------------------
@pytest.fixture(scope="module")
def zipf8(codec):
    return tgr._zipf(codec, tgr.ZIPF_N)


@pytest.mark.parametrize("full", [False, True])
def test_more_jobs_than_waves(codec, zipf8, full):
    import torch
    s = zipf8
    assert s.nb == 2049
    codec.upload_decode(s.plan)
    ranges = tgr._random_ranges(s.nsym)
    assert len(ranges) == 40 and sum(nblk(b, c) for b, c in ranges) > 16 * 512   # more jobs than a device has waves
    offs, size = layout(ranges)
    buf, offs, stats = run(codec, s, ranges, full, offs=offs, size=size)
    codec.sync()
    assert torch.equal(buf, image(s, ranges, offs, size))
    st = [int(v) for v in stats.cpu()]
    assert st[0] == sum(nblk(b, c) for b, c in ranges) and st[3] == 0, st
    one = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")   # the same by 40 hz_decode_range calls
    for (b, c), o in zip(ranges, offs):
        codec.decode_range(s.payload, s.nsym, s.index if full else s.seek, b, c, one[o:], full_index=full)
    codec.sync()
    assert torch.equal(buf, one)


# ---- 3. every table shape -----------------------------------------------------------------------
def model_stream(bk, sym, start_bit, lead=0):
    """A stream of the host model on the device: payload, index and seek table are the model's."""
    import torch
    m = ref_stream.model(sym, bk.ln, bk.code, start_bit, lead)
    nb = ref_stream.nblocks(m.nsym)
    index = torch.from_numpy(np.concatenate([m.index, np.zeros((-m.index.size) % 8, np.uint8)]).view(np.int64).copy()).cuda()
    return SimpleNamespace(x=torch.from_numpy(m.sym.view(np.uint8).copy()).cuda(), nsym=m.nsym, nb=nb, m=m,
                           payload=torch.from_numpy(m.payload.copy()).cuda(), index=index,
                           seek=torch.from_numpy(m.start.view(np.int64).copy()).cuda())


@pytest.mark.parametrize("start_bit", [0, 5, 45])
@pytest.mark.parametrize("kind", ["longest", "chains", "uniform"])
@pytest.mark.parametrize("name", tds.BOOKS)
def test_table_shapes(codec, name, kind, start_bit):
    bk = book(name)
    nsym = 40 * BLK + 777
    rng = np.random.default_rng([tds.BOOKS.index(name), len(kind), start_bit])
    s = model_stream(bk, tds._stream(bk, kind, nsym, rng), start_bit, tds._lead(start_bit))
    codec.dev.upload_decode(bk.cb)
    ranges = tgr._eight_ranges(nsym, 5)
    assert ranges[0] == (0, 1) and ranges[1] == (nsym - 1, 1) and len(ranges) == 8
    for full in (False, True):
        st = check(codec, s, ranges, full)
        assert st[0] == sum(nblk(b, c) for b, c in ranges) and st[3] == 0, (full, st)
        if name == "fib57" and kind == "longest":   # a block of 2048 x 56 bits fits no slot sized for the mean
            assert int(s.m.start[1] - s.m.start[0]) == BLK * 56 and st[1] >= 1, st


# ---- 4. the cold path on ordinary data -------------------------------------------------------------
def test_cold_path_on_ordinary_data(built_lib):
    """HZ_RANGES_SLOT_WORDS=4: a staging window has 7 words or more (the pad before the block, the words read
    past its end), so none fits and every job of case 1 goes cold."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "cold"], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, HZ_RANGES_SLOT_WORDS="4"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ---- 5. many rounds ------------------------------------------------------------------------------------
def test_many_rounds(codec):
    cb, ln, code, sym = trm.tri36_stream(3 * BLK + 5)
    s = model_stream(SimpleNamespace(ln=ln, code=code), sym, 0)
    codec.dev.upload_decode(cb)
    ranges = [(0, s.nsym), (BLK - 1, 2), (BLK + 7, BLK), (s.nsym - 1, 1)]
    st = check(codec, s, ranges, False)
    assert st[0] == sum(nblk(b, c) for b, c in ranges) and st[3] == 0, st
    assert 8 <= st[2] <= 64, st     # the true path is handed from lane to lane (tests/test_ranges_model.py)
    check(codec, s, ranges, True)


# ---- 6. slices ---------------------------------------------------------------------------------------------
def test_slices(codec, zipf8, hz):
    import torch
    s = zipf8
    codec.upload_decode(s.plan)
    seek_host = s.seek.cpu().numpy().view(np.uint64)
    inside = [(1000 * BLK - 1, 70000), (1010 * BLK + 5, 3), (1100 * BLK, 2 * BLK)]
    spans = [codec.dev.seek_span(seek_host, s.nsym, b, c) for b, c in inside]
    bb, be = min(a for a, _ in spans), min(max(e for _, e in spans), s.payload.numel())
    g = torch.Generator(device="cuda")
    g.manual_seed(31)
    buf = torch.randint(0, 256, (8192 + be - bb,), dtype=torch.uint8, device="cuda", generator=g)
    buf[4096:4096 + be - bb] = s.payload[bb:be]
    pay = buf[4096:4096 + be - bb]
    for full in (False, True):
        st = check(codec, s, inside, full, payload=pay, base=bb)
        assert st[0] == sum(nblk(b, c) for b, c in inside) and st[3] == 0, st
    outside = (5 * BLK + 1, 2 * BLK)       # blocks 5 .. 7: their bytes are not in the slice
    ranges = inside + [outside]
    offs, size = layout(ranges)
    for full in (False, True):
        out, offs, stats = run(codec, s, ranges, full, payload=pay, base=bb, offs=offs, size=size)
        with pytest.raises(hz.HZError) as e:
            codec.sync()
        assert e.value.status == HZ_EINVAL
        assert torch.equal(out, image(s, ranges, offs, size, skip={3}))
        st = [int(v) for v in stats.cpu()]
        assert st[3] == nblk(*outside) and st[0] == sum(nblk(b, c) for b, c in inside), st
    check(codec, s, inside, False)        # the context is usable again


# ---- 7. wrong tables and wrong ranges ------------------------------------------------------------------------
def _moved_entry(s):
    """The first entry b >= 700 of start[] that, moved one bit up, leaves BOTH blocks beside it wrong by the
    format's own rule: block b - 1 then ends one bit late (its 2048 codewords end at the true bit: always
    wrong), and block b starts one bit late -- a walk from there may fall back onto the true boundaries
    with the same number of codewords, which no check can tell from a right table, so such entries are
    passed over. Decided with the host model's lengths (tests/ranges_model.py), not with the device."""
    from huffman_amd import codebook_arrays
    _, ln, code = codebook_arrays(s.plan.cb)
    seek = s.seek.cpu().numpy().view(np.uint64)
    pay = s.payload.cpu().numpy()
    for b in range(700, 720):
        s0, s1 = int(seek[b]) + 1, int(seek[b + 1])
        byte0 = s0 // 8
        lens = ranges_model.Lengths(pay[byte0:s1 // 8 + 16], ln, code)
        p, k = s0 - 8 * byte0, 0
        while p < s1 - 8 * byte0 and k <= BLK:
            L = lens.at(p)
            if L == 0:
                break
            p += L
            k += 1
        if not (k == BLK and p == s1 - 8 * byte0):
            return b
    raise AssertionError("no such entry")


def test_wrong_seek_table(codec, zipf8, hz):
    import torch
    s = zipf8
    codec.upload_decode(s.plan)
    b = _moved_entry(s)
    bad = s.seek.clone()
    bad[b] += 1
    ranges = [((b - 3) * BLK + 9, BLK), ((b - 1) * BLK + 5, 100), (b * BLK + 5, 100), ((b + 1) * BLK, 3 * BLK), (0, 10),
              ((b - 2) * BLK, 5 * BLK)]
    offs, size = layout(ranges)
    out, offs, stats = run(codec, s, ranges, False, table=bad, offs=offs, size=size)
    with pytest.raises(hz.HZError) as e:
        codec.sync()
    assert e.value.status == HZ_EFORMAT
    exp = image(s, ranges, offs, size, skip={1, 2})
    lo = offs[5] + 2 * BLK * 2                      # the last range: blocks b - 1 and b store nothing, the rest does
    exp[lo - 2 * BLK:lo + 2 * BLK] = 0xA5
    assert torch.equal(out, exp)
    st = [int(v) for v in stats.cpu()]
    assert st[3] == 4 and st[0] == sum(nblk(*r) for r in ranges) - 4, st
    # a full index whose start[b] moved: sub[b][0] no longer agrees with it, and block b - 1 is too long by a bit,
    # which the full index does not walk to find
    idx = s.index.clone()
    idx[b] += 1
    out, offs, stats = run(codec, s, ranges, True, table=idx, offs=offs, size=size)
    with pytest.raises(hz.HZError) as e:
        codec.sync()
    assert e.value.status == HZ_EFORMAT
    exp = image(s, ranges, offs, size, skip={2})
    exp[lo:lo + 2 * BLK] = 0xA5
    assert torch.equal(out, exp)
    # a descending pair
    desc = s.seek.clone()
    desc[300] = desc[298]
    ranges = [(299 * BLK, 10), (100 * BLK + 1, 5 * BLK)]
    offs, size = layout(ranges)
    out, offs, stats = run(codec, s, ranges, False, table=desc, offs=offs, size=size)
    with pytest.raises(hz.HZError) as e:
        codec.sync()
    assert e.value.status == HZ_EFORMAT
    assert torch.equal(out, image(s, ranges, offs, size, skip={0}))
    check(codec, s, ranges, False)


def test_wrong_ranges(codec, zipf8, hz):
    import torch
    s = zipf8
    codec.upload_decode(s.plan)
    ranges = [(0, 3000), (s.nsym - 5, 6), (7 * BLK, 100), (9 * BLK + 1, 50), (11 * BLK, 2 * BLK), (s.nsym + 1, 0)]
    offs, size = layout(ranges)
    offs[2] += 1                  # an odd out_byte
    offs[3] = size - 50           # 100 bytes from 50 before the buffer's end
    out, offs, stats = run(codec, s, ranges, False, offs=offs, size=size)
    with pytest.raises(hz.HZError) as e:
        codec.sync()
    assert e.value.status == HZ_EINVAL
    assert torch.equal(out, image(s, ranges, offs, size, skip={1, 2, 3, 5}))
    st = [int(v) for v in stats.cpu()]
    assert st[0] == nblk(0, 3000) + 2 and st[3] == 0, st
    check(codec, s, [ranges[0], ranges[4]], False)


def test_cheap_checks_at_the_call(codec, zipf8):
    import torch
    s = zipf8
    codec.upload_decode(s.plan)
    out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    rg = torch.tensor([[0, 1, 0]], dtype=torch.int64, device="cuda")
    stats = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    lib, h = codec.dev.lib, codec.dev.h
    p, sk, r, o, n = s.payload.data_ptr(), s.seek.data_ptr(), rg.data_ptr(), out.data_ptr(), s.payload.numel()
    args = [(None, sk, r, o, 0), (p, None, r, o, 0), (p, sk, None, o, 0), (p, sk, r, None, 0), (p, sk, r, o + 1, 0),
            (p, sk, r, o, 2)]
    for pay, seek, ranges, dst, flags in args:
        assert lib.hz_decode_ranges(h, pay, n, 0, seek, s.nsym, ranges, 1, dst, 4096, None, flags) == HZ_EINVAL
    assert lib.hz_decode_ranges(None, p, n, 0, sk, s.nsym, r, 1, o, 4096, None, 0) == HZ_EINVAL
    assert lib.hz_decode_ranges(h, p, n, 0, sk, s.nsym, r, 0, o, 4096, stats.data_ptr(), 0) == 0   # nothing launched
    assert lib.hz_decode_ranges(h, p, n, 0, sk, s.nsym, r, 1, o, 4096, None, 0) == 0              # d_stats may be null
    codec.sync()
    assert int(out[2:].sum().item()) == 0 and torch.equal(out[:2], s.x[:2])
    from huffman_amd import Device
    torch.cuda.synchronize()
    dev = Device(0)              # no decode tables
    try:
        assert dev.lib.hz_decode_ranges(dev.h, p, n, 0, sk, s.nsym, r, 1, o, 4096, None, 0) == HZ_EINVAL
    finally:
        dev.close()


# ---- 8. graph capture -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True])
def test_graph_capture(codec, zipf8, full):
    import torch
    s = zipf8
    codec.upload_decode(s.plan)
    first = [(3 * BLK + 11, 5 * BLK + 77), (0, 1), (s.nsym - 1, 1), (2047, 2), (900 * BLK, BLK), (17, 4000), (1500 * BLK - 9, 18),
             (7, 0)]
    other = [(1200 * BLK + 1, 3 * BLK), (5, 5), (s.nsym - 3 * BLK, 3 * BLK), (2048, 2048), (1, 0), (640 * BLK - 1, 2),
             (77 * BLK + 100, 6000), (s.nsym - 2, 1)]
    o1, n1 = layout(first)
    o2, n2 = layout(other)
    size = max(n1, n2)
    buf = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    rows = lambda ranges, offs: torch.tensor([[b, c, o] for (b, c), o in zip(ranges, offs)], dtype=torch.int64,  # noqa: E731
                                             device="cuda")
    rg = rows(first, o1)
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    table = s.index if full else s.seek

    def call():
        codec.decode_ranges(s.payload, s.nsym, table, rg, buf, stats=stats, full_index=full)

    call()  # eager: also sizes the scratch
    codec.sync()
    assert torch.equal(buf, image(s, first, o1, size))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=codec.stream):  # a host synchronisation inside would break the capture
        call()
    for ranges, offs in ((first, o1), (other, o2), (first, o1)):
        rg.copy_(rows(ranges, offs))                # the device list is all the replay reads
        buf.fill_(0xA5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf, image(s, ranges, offs, size))
        assert int(stats[0]) == sum(nblk(b, c) for b, c in ranges) and int(stats[3]) == 0
    codec.sync()


# ---- 9. host forms ------------------------------------------------------------------------------------------------
def test_host_forms(hz):
    with open(os.path.join(GOLD, "romeo.txt"), "rb") as f:
        romeo = f.read()
    odd = np.random.default_rng(12).integers(0, 7, 3 * 4096 + 1, dtype=np.uint8).tobytes()
    for data in (romeo, odd):
        n = len(data)
        blob = hz.encode(data)
        seek = hz.build_seek(blob)
        pairs = [(0, n), (1, 1), (n - 1, 1), (4095, 3), (4097, 8191), (n - 3, 3), (5, 0), (n, 0), (n // 2 | 1, 4097),
                 (1, 1)]
        got = hz.decode_ranges(blob, seek, pairs)
        assert [len(g) for g in got] == [c for _, c in pairs]
        for (off, cnt), g in zip(pairs, got):
            assert g == data[off:off + cnt], (off, cnt)
        assert hz.decode_ranges(blob, seek, []) == []
        assert hz.decode_ranges(blob, seek, [(n - 1, 1)]) == [data[n - 1:]]   # the last byte alone
        for past in ([(0, 1), (n, 1)], [(n + 1, 0)], [(n - 1, 2)]):
            with pytest.raises(hz.HZError) as e:
                hz.decode_ranges(blob, seek, past)
            assert e.value.status == HZ_EINVAL
    assert len(odd) % 2 == 1


def test_names_exported(hz):
    assert "decode_ranges" in hz.__all__ and callable(hz.decode_ranges)
    from huffman_amd import _lib
    assert _lib.HZ_RANGES_STATS_WORDS == 4


if __name__ == "__main__":
    assert sys.argv[1:] == ["cold"], sys.argv
    from huffman_amd.pipeline import StreamCodec
    _c = StreamCodec(0)
    edges_check(_c, tgr._zipf(_c, 5 * 4096 + 6), cold=True)
    print("ok")
