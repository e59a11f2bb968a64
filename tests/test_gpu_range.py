"""Random access on the device: hz_decode_range from the seek table alone and from a full block
index, hz_index_expand, payload slices, the error paths, graph capture and the host forms.
Bit-exact throughout; every decode lands between 64 guard bytes of 0xA5 on both sides.

Run as a script (`python tests/test_gpu_range.py zipf`) it decodes the random ranges of the Zipf
stream once and prints "ok": the tests start it in a fresh process to set HZ_RANGE_TILE_BLOCKS and
HZ_DEC_PIPE, which the library reads once."""
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

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden")
BLK = 2048
GUARD = 64
HZ_EINVAL, HZ_EFORMAT = -1, -5
ZIPF_N = (8 << 20) + 6


@pytest.fixture(scope="module")
def hz(built_lib):
    import huffman_amd
    return huffman_amd


@pytest.fixture(scope="module")
def codec(built_lib):
    from huffman_amd.pipeline import StreamCodec
    return StreamCodec(0)


def _encode(codec, x):
    """Encode a device tensor once: the stream, its index and its seek table (a tensor of its own, so a
    decode from the seek table cannot find sub[] behind it)."""
    nsym = x.numel() // 2
    plan, payload, index = codec.encode(x)
    codec.sync()
    nb = (nsym + BLK - 1) // BLK
    return SimpleNamespace(x=x, nsym=nsym, nb=nb, plan=plan, payload=payload, index=index,
                           seek=index[:nb + 1].clone())


def _zipf(codec, n, seed=7):
    import torch
    x = torch.empty(n, dtype=torch.uint8, device="cuda")
    codec.dev.generate(x.data_ptr(), n, offset=0, kind=1, alpha=1.1, seed=seed)
    return _encode(codec, x)


def _decode(codec, s, begin, count, full, off=0, payload=None, base=0, seek=None):
    """One range into a guarded buffer at byte offset `off` of an aligned address; returns the buffer
    (not yet synchronised) and the range's position in it."""
    import torch
    buf = torch.full((GUARD + 16 + 2 * count + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    lo = GUARD + off
    pay = s.payload if payload is None else payload
    table = s.index if full else (s.seek if seek is None else seek)
    codec.decode_range(pay, s.nsym, table, begin, count, buf[lo:], full_index=full, payload_byte_base=base)
    return buf, lo


def _guards_intact(buf, lo, count):
    return bool((buf[:lo] == 0xA5).all()) and bool((buf[lo + 2 * count:] == 0xA5).all())


def _check(codec, s, begin, count, full, off=0, **kw):
    import torch
    buf, lo = _decode(codec, s, begin, count, full, off, **kw)
    codec.sync()
    assert _guards_intact(buf, lo, count), (begin, count, full, off)
    assert torch.equal(buf[lo:lo + 2 * count], s.x[2 * begin:2 * (begin + count)]), (begin, count, full, off)


def _edge_ranges(nsym, last):
    """The issue's edge list for a stream whose last block starts at symbol `last`."""
    return [(0, nsym), (0, 1), (nsym - 1, 1), (2047, 2), (2048, 2048), (1, 2046), (3, 4099), (4096, nsym - 4096),
            (last, 3), (last - 1, 2), (7, 0)]


# ---- 1. edges on the smallest stream that has them ---------------------------------
@pytest.fixture(scope="module")
def small(codec):
    return _zipf(codec, 5 * 4096 + 6)


@pytest.mark.parametrize("full", [False, True])
def test_edges_smallest_stream(codec, small, full):
    s = small
    assert s.nsym == 5 * BLK + 3 and s.nb == 6
    codec.upload_decode(s.plan)
    for i, (begin, count) in enumerate(_edge_ranges(s.nsym, 5 * BLK)):
        _check(codec, s, begin, count, full, off=(0, 2, 14)[i % 3])


# ---- 2. many waves and tiles ----------------------------------------------------------
def _random_ranges(nsym, k=40, seed=2024):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        begin = int(rng.integers(0, nsym))
        out.append((begin, int(rng.integers(1, nsym - begin + 1))))
    return out


def _zipf_ranges_check(codec, s):
    ranges = _random_ranges(s.nsym)
    assert sum(2 * c > (1 << 20) for _, c in ranges) >= 5
    assert sum((b // BLK) % 2 == 1 for b, _ in ranges) >= 5
    assert sum(((b + c - 1) // BLK - b // BLK + 1) % 2 == 1 for b, c in ranges) >= 5
    codec.upload_decode(s.plan)
    for i, (begin, count) in enumerate(ranges):
        _check(codec, s, begin, count, full=bool(i & 1), off=(0, 2, 14)[i % 3])


@pytest.fixture(scope="module")
def zipf8(codec):
    return _zipf(codec, ZIPF_N)


def test_random_ranges_many_waves(codec, zipf8):
    assert zipf8.nb == 2049
    _zipf_ranges_check(codec, zipf8)


def _child(env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "zipf"], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_random_ranges_small_tiles(built_lib):
    """HZ_RANGE_TILE_BLOCKS=64: the ranges (up to 2049 blocks) span up to 33 tiles, odd tile tails included."""
    _child({"HZ_RANGE_TILE_BLOCKS": "64"})


# ---- 3. every table shape -------------------------------------------------------------
def _eight_ranges(nsym, seed):
    rng = np.random.default_rng(seed)
    out = [(0, 1), (nsym - 1, 1)]
    while len(out) < 8:
        begin = int(rng.integers(0, nsym))
        out.append((begin, int(rng.integers(1, min(nsym - begin, 40 * BLK) + 1))))
    return out


@pytest.mark.parametrize("name", ["dense8", "short", "mid20", "long24", "fib31", "fib34"])
def test_table_shapes(codec, name):
    import torch
    from huffman_amd import codebook_arrays
    from test_gpu import _fib_input, _shape_stream
    from test_gpu_extract import _fib_stream
    if name == "fib31":
        host = _fib_stream(1)
    elif name == "fib34":
        host = np.frombuffer(_fib_input(34), dtype=np.uint8)
    else:
        host = _shape_stream(name)
    s = _encode(codec, torch.from_numpy(np.array(host, dtype=np.uint8)).cuda())
    _, ln, _ = codebook_arrays(s.plan.cb)
    mx = int(ln.max())
    assert {"dense8": mx == 8, "short": mx <= 16, "mid20": 16 < mx <= 22, "long24": mx > 22, "fib31": mx == 31,
            "fib34": mx == 34}[name], mx
    for i, (begin, count) in enumerate(_eight_ranges(s.nsym, 5)):
        _check(codec, s, begin, count, full=bool(i & 1), off=(0, 2, 14)[i % 3])
        _check(codec, s, begin, count, full=not (i & 1), off=(2, 14, 0)[i % 3])


@pytest.mark.parametrize("pipe", ["0", "1"])
def test_pipelined_forms(built_lib, pipe):
    """HZ_DEC_PIPE=0 / 1 (2 is the default, every other test): the plain and the one-block pipelined
    LUT forms of the range decoder."""
    _child({"HZ_DEC_PIPE": pipe})


# ---- 4. FIXED16 ------------------------------------------------------------------------
def test_fixed16(codec):
    import torch
    from huffman_amd import codebook_arrays
    sym = np.repeat(np.arange(65536, dtype=np.uint16), 2)
    np.random.default_rng(3).shuffle(sym)
    s = _encode(codec, torch.from_numpy(sym.view(np.uint8)).cuda())
    assert s.x.numel() == 256 << 10 and s.nb == 64
    _, ln, _ = codebook_arrays(s.plan.cb)
    assert int(ln.min()) == int(ln.max()) == 16 and s.plan.cb.min_len == s.plan.cb.max_len == 16
    for full in (False, True):
        for i, (begin, count) in enumerate(_edge_ranges(s.nsym, 63 * BLK)):
            _check(codec, s, begin, count, full, off=(0, 2, 14)[i % 3])


# ---- 5. a block of 65 536 bits or more --------------------------------------------------
def _long_block_stream(codec):
    """Codebook from a Fibonacci histogram of 41 counts (codes up to 40 bits); the stream: three blocks
    of the eight rarest symbols (33 to 40 bits each), then 5000 symbols drawn from all 41."""
    import torch
    from huffman_amd import build_codebook, codebook_arrays
    fib = [1, 1]
    while len(fib) < 41:
        fib.append(fib[-1] + fib[-2])
    syms = (np.arange(41, dtype=np.uint32) * 257 + 3).astype(np.uint16)
    hist = np.zeros(65536, dtype=np.uint64)
    hist[syms] = fib
    cb = build_codebook(hist)
    _, ln, _ = codebook_arrays(cb)
    assert int(ln.max()) == 40 and int(ln[syms[:8]].min()) >= 33
    rng = np.random.default_rng(9)
    stream = np.concatenate([syms[rng.integers(0, 8, 3 * BLK)], syms[rng.integers(0, 41, 5000)]]).astype(np.uint16)
    x = torch.from_numpy(stream.view(np.uint8)).cuda()
    nsym = stream.size
    actual = np.bincount(stream, minlength=65536).astype(np.uint64)
    plan = codec.make_plan(hist, x.numel(), hist_local=actual, cb=cb)
    payload, index = codec.alloc_payload(plan, nsym)
    codec.pack(x, plan, payload, index)
    codec.upload_decode(plan)
    codec.sync()
    nb = (nsym + BLK - 1) // BLK
    s = SimpleNamespace(x=x, nsym=nsym, nb=nb, plan=plan, payload=payload, index=index, seek=index[:nb + 1].clone())
    starts = index[:nb + 1].cpu().numpy().view(np.uint64)
    assert int(np.diff(starts.astype(np.int64))[:3].min()) >= 65536  # the case itself: blocks past 2^16 bits
    return s


@pytest.fixture(scope="module")
def longblk(codec):
    return _long_block_stream(codec)


@pytest.mark.parametrize("full", [False, True])
def test_blocks_of_65536_bits(codec, longblk, full):
    s = longblk
    codec.upload_decode(s.plan)
    ranges = [(0, s.nsym), (5, 100), (BLK - 3, 10), (BLK, BLK), (2 * BLK + 17, BLK + 900), (3 * BLK - 1, 2),
              (3 * BLK, s.nsym - 3 * BLK), (3 * BLK + 2049, 700), (s.nsym - 1, 1)]
    for i, (begin, count) in enumerate(ranges):
        _check(codec, s, begin, count, full, off=(0, 2, 14)[i % 3])


# ---- 6. hz_index_expand == hz_pack's index ----------------------------------------------
def _expand_equals_pack(codec, s, in_place):
    import torch
    from huffman_amd import index_bytes
    codec.upload_decode(s.plan)
    out = torch.full_like(s.index, -1)
    if in_place:
        out[:s.nb + 1] = s.seek
        codec.index_expand(s.payload, s.nsym, out, out)
    else:
        codec.index_expand(s.payload, s.nsym, s.seek, out)
    codec.sync()
    nbytes = index_bytes(s.nsym)
    assert np.array_equal(s.index.cpu().numpy().view(np.uint8)[:nbytes], out.cpu().numpy().view(np.uint8)[:nbytes])


@pytest.mark.parametrize("n,in_place", [((8 << 20) + 2, False), ((8 << 20) + 2, True), (4097 * 2 + 1, False), (3, False)])
def test_index_expand_zipf(codec, n, in_place):
    _expand_equals_pack(codec, _zipf(codec, n, seed=5), in_place)


@pytest.mark.parametrize("name", ["dense8", "short", "mid20", "long24"])
def test_index_expand_table_shapes(codec, name):
    import torch
    from test_gpu import _shape_stream
    _expand_equals_pack(codec, _encode(codec, torch.from_numpy(_shape_stream(name)).cuda()), False)


def test_index_expand_long_blocks(codec, longblk):
    _expand_equals_pack(codec, longblk, False)


# ---- 7. slices ------------------------------------------------------------------------------
SLICE_RANGES = [(0, 3000), (2047, 2), (5 * BLK + 1, 9 * BLK), (1000 * BLK - 1, 70000), (2048 * BLK - 5, 5 + 2),
                ((ZIPF_N // 2) - 1, 1)]


def _slice(codec, s, begin, count, fill, cut_front=0, cut_back=0):
    """Only hz_seek_span's bytes of the payload (minus the cuts), in the middle of a fresh buffer."""
    import torch
    seek_host = s.seek.cpu().numpy().view(np.uint64)
    bb, be = codec.dev.seek_span(seek_host, s.nsym, begin, count)
    be = min(be, s.payload.numel())
    assert bb % 16 == 0 and bb < be
    bb, be = bb + cut_front, be - cut_back
    pad = 4096
    if fill == "zero":
        buf = torch.zeros(2 * pad + be - bb, dtype=torch.uint8, device="cuda")
    else:
        g = torch.Generator(device="cuda")
        g.manual_seed(31)
        buf = torch.randint(0, 256, (2 * pad + be - bb,), dtype=torch.uint8, device="cuda", generator=g)
    buf[pad:pad + be - bb] = s.payload[bb:be]
    return buf[pad:pad + be - bb], bb


@pytest.mark.parametrize("fill", ["zero", "random"])
def test_slices(codec, zipf8, fill):
    s = zipf8
    codec.upload_decode(s.plan)
    for i, (begin, count) in enumerate(SLICE_RANGES):
        pay, base = _slice(codec, s, begin, count, fill)
        _check(codec, s, begin, count, full=False, off=(0, 2, 14)[i % 3], payload=pay, base=base)
        _check(codec, s, begin, count, full=True, off=(14, 0, 2)[i % 3], payload=pay, base=base)


@pytest.mark.parametrize("cut", ["front", "back"])
def test_short_slice_is_invalid(codec, zipf8, hz, cut):
    s = zipf8
    codec.upload_decode(s.plan)
    begin, count = 1000 * BLK - 1, 70000
    pay, base = _slice(codec, s, begin, count, "random", cut_front=64 if cut == "front" else 0,
                       cut_back=64 if cut == "back" else 0)
    for full in (False, True):
        buf, lo = _decode(codec, s, begin, count, full, off=2, payload=pay, base=base)
        with pytest.raises(hz.HZError) as e:
            codec.sync()
        assert e.value.status == HZ_EINVAL
        assert _guards_intact(buf, lo, count)
    _check(codec, s, begin, count, full=False)  # the context is usable again


# ---- 8. a wrong seek table ends cleanly -------------------------------------------------------
def test_wrong_seek_table(codec, zipf8, hz):
    s = zipf8
    codec.upload_decode(s.plan)
    bad = s.seek.clone()
    bad[700] += 1
    # block 699 now ends one bit late: its 2048 codewords end at the true bit, never at start[700]
    # (block 700 starts one bit late: a walk from there may fall back onto the true boundaries with
    # the same count, which no check can tell from a right table -- so it is not asserted alone)
    for begin, count in [(699 * BLK + 5, 100), (690 * BLK, 30 * BLK)]:
        buf, lo = _decode(codec, s, begin, count, False, seek=bad)
        with pytest.raises(hz.HZError) as e:
            codec.sync()
        assert e.value.status == HZ_EFORMAT, (begin, count)
        assert _guards_intact(buf, lo, count)
    # nothing was written for the single wrong block
    buf, lo = _decode(codec, s, 699 * BLK + 5, 100, False, seek=bad)
    with pytest.raises(hz.HZError):
        codec.sync()
    assert bool((buf == 0xA5).all())
    # a full index whose start[700] moved: sub[700][0] no longer agrees with it
    s_bad = SimpleNamespace(**{**vars(s), "index": s.index.clone()})
    s_bad.index[700] += 1
    buf, lo = _decode(codec, s_bad, 700 * BLK + 5, 100, True)
    with pytest.raises(hz.HZError) as e:
        codec.sync()
    assert e.value.status == HZ_EFORMAT
    assert bool((buf == 0xA5).all())
    # a descending table
    desc = s.seek.clone()
    desc[300] = desc[298]
    buf, lo = _decode(codec, s, 299 * BLK, 10, False, seek=desc)
    with pytest.raises(hz.HZError) as e:
        codec.sync()
    assert e.value.status == HZ_EFORMAT
    # elsewhere in the same stream, on a fresh call, the wrong table still decodes
    _check(codec, s, 100 * BLK + 1, 5 * BLK, False, seek=bad)
    _check(codec, s, 701 * BLK, 5 * BLK, False, seek=bad)


def test_cheap_checks_at_the_call(codec, zipf8, hz):
    import torch
    s = zipf8
    out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    lib, h = codec.dev.lib, codec.dev.h
    p, sk = s.payload.data_ptr(), s.seek.data_ptr()
    args = [(None, sk, 0, 1, out.data_ptr(), 0), (p, None, 0, 1, out.data_ptr(), 0), (p, sk, 0, 1, None, 0),
            (p, sk, s.nsym, 1, out.data_ptr(), 0), (p, sk, 1, s.nsym, out.data_ptr(), 0),
            (p, sk, 0, 1, out.data_ptr() + 1, 0), (p, sk, 0, 1, out.data_ptr(), 2)]
    for pay, seek, begin, count, o, flags in args:
        assert lib.hz_decode_range(h, pay, s.payload.numel(), 0, seek, s.nsym, begin, count, o, flags) == HZ_EINVAL
    assert lib.hz_decode_range(h, p, s.payload.numel(), 0, sk, s.nsym, 7, 0, out.data_ptr(), 0) == 0
    codec.sync()
    assert int(out.sum().item()) == 0


# ---- 9. graph capture --------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True])
def test_graph_capture(codec, zipf8, full):
    import torch
    s = zipf8
    codec.upload_decode(s.plan)
    begin, count = 3 * BLK + 11, 900 * BLK + 77
    out = torch.zeros(2 * count + 16, dtype=torch.uint8, device="cuda")
    table = s.index if full else s.seek

    def call():
        codec.decode_range(s.payload, s.nsym, table, begin, count, out[2:], full_index=full)

    call()  # eager: also sizes the scratch
    codec.sync()
    want = s.x[2 * begin:2 * (begin + count)]
    assert torch.equal(out[2:2 + 2 * count], want)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=codec.stream):  # a host synchronisation inside would break the capture
        call()
    for _ in range(2):
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[2:2 + 2 * count], want)
    codec.sync()


# ---- 10. host forms on reference-written files ----------------------------------------------------
BASELINES = sorted(os.path.basename(p)[:-len(".baseline.compressed")]
                   for p in glob.glob(os.path.join(GOLD, "*.baseline.compressed")))


@pytest.mark.parametrize("name", BASELINES)
def test_host_forms_on_reference_files(hz, name):
    import torch
    with open(os.path.join(GOLD, name), "rb") as f:
        data = f.read()
    with open(os.path.join(GOLD, name + ".baseline.compressed"), "rb") as f:
        blob = f.read()
    n = len(data)
    seek = hz.build_seek(blob)
    nsym = n // 2
    assert seek.dtype == np.uint64 and seek.size * 8 == hz.seek_bytes(nsym)
    pairs = [(0, n), (1, 1), (n - 1, 1), (4095, 3), (4097, 8191)]
    if name == "synth_zipf_65537.bin":
        assert n == 65537
        pairs.append((n - 3, 3))  # ends with the trailing byte the header carries
    for off, length in pairs:
        length = min(length, n - off)  # the 4099-byte file ends inside the last pair
        assert length > 0
        assert hz.decode_range(blob, seek, off, length) == data[off:off + length], (off, length)
    # the table is the head of hz_index_build's index for the same payload
    cb, info = hz.parse_header(blob)
    pay = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8)[info.payload_byte:].copy()).cuda()
    pay = torch.cat([pay, torch.zeros(16, dtype=torch.uint8, device="cuda")])
    index = torch.full(((hz.index_bytes(nsym) + 7) // 8,), -1, dtype=torch.int64, device="cuda")
    dev = hz.Device(0)
    try:
        torch.cuda.synchronize()
        dev.upload_decode(cb)
        dev.index_build(pay.data_ptr(), pay.numel() - 16, info.payload_bit, nsym, index.data_ptr())
        dev.sync()
    finally:
        dev.close()
    assert np.array_equal(index[:seek.size].cpu().numpy().view(np.uint64), seek)


def test_names_exported(hz):
    for name in ("build_seek", "decode_range", "seek_bytes", "seek_span"):
        assert name in hz.__all__ and callable(getattr(hz, name))


if __name__ == "__main__":
    assert sys.argv[1:] == ["zipf"], sys.argv
    from huffman_amd.pipeline import StreamCodec
    _c = StreamCodec(0)
    _zipf_ranges_check(_c, _zipf(_c, ZIPF_N))
    print("ok")
