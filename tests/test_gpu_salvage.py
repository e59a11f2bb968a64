"""salvage (hz_seekable_salvage_file) end to end on the GPU: seekable files are damaged in Python -- payload
bits, seek entries, sum words -- and every case asserts the returned list of bad blocks, that every block not
listed equals the original, that every listed block is zeros (with keep_unverified: whatever it decoded to,
which for a damaged sum word is the original), and the output's size n, the odd last byte included. Every case
runs at the smallest window (four blocks a window, so damage also sits on window edges) and at the default one,
and again without an output (the scan: the same list, no file created).

Inputs: Zipf bytes of 40 blocks + 777 symbols + an odd byte; the two-bit stream of tests/test_gpu_seekable.py
at 8 blocks (a flipped bit never desynchronises: only the sum sees it); 65 536 distinct values with equal
counts (every code 16 bits, 32 blocks); and the reference encoder's tests/golden/synth_zipf_65537 file made
seekable in place.

What a damaged seek entry costs is not fixed by the format: entry i is shared by blocks i - 1 and i, the block
that ends there is always lost (its codewords end at the true bit), the one that starts there may or may not
decode to bytes that still match (a walk from a wrong bit can fall back onto the true boundaries). So those
cases assert a non-empty subset of {i - 1, i}. A replacement value that equals the true entry is no damage
(entry 0 is the payload's first bit, which may be bit 0): the list is then empty.

Tolerance: none -- every check is bit-exact."""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden")
HZ_EINVAL, HZ_EFORMAT, HZ_ENOENT, HZ_ECHECKSUM = -1, -5, -10, -11
BLOCK, BLK = 4096, 2048
MIN_WINDOW = 16384
WINDOWS = [MIN_WINDOW, 256 << 20]
INPUTS = ["zipf", "two_bit", "fixed16", "golden"]


@pytest.fixture(scope="module")
def hz(built_lib):
    import huffman_amd
    return huffman_amd


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _make(hz, name, d):
    """(the original, the seekable file's bytes) of an input."""
    if name == "golden":
        path = str(d / "golden.compressed")
        shutil.copyfile(os.path.join(GOLD, "synth_zipf_65537.bin.baseline.compressed"), path)
        assert hz.make_seekable(path) is True
        return _read(os.path.join(GOLD, "synth_zipf_65537.bin")), _read(path)
    if name == "zipf":
        import oracle_lib
        data = oracle_lib.generate(2 * (40 * BLK + 777) + 1, offset=0, kind=1, seed=5).tobytes()
        src, out = str(d / "zipf.bin"), str(d / "zipf.compressed")
        with open(src, "wb") as f:
            f.write(data)
        hz.archive_seekable(src, out, chunk_bytes=65536)
        return data, _read(out)
    if name == "two_bit":
        sym = np.random.default_rng(11).permutation(np.repeat(np.array([0x1234, 0x00ff, 0xabcd, 0x8000], dtype="<u2"), 2 * BLK))
    else:
        sym = np.random.default_rng(12).permutation(65536).astype("<u2")
    data = sym.tobytes()
    return data, hz.encode_seekable(data)


@pytest.fixture(scope="module", params=INPUTS)
def inp(request, hz, tmp_path_factory):
    """An input, its seekable file and where things stand in it; the undamaged file is written once."""
    d = tmp_path_factory.mktemp("salvage_" + request.param)
    data, blob = _make(hz, request.param, d)
    info = hz.seekable_info(blob)
    cb, hinfo = hz.parse_header(blob)
    nb = info["nblocks"]
    seek = [int(v) for v in np.frombuffer(blob, dtype="<u8", count=nb + 1, offset=info["seek_off"])]
    assert info["n"] == len(data) and nb == {"zipf": 41, "two_bit": 8, "fixed16": 32, "golden": 16}[request.param]
    if request.param == "two_bit":
        assert cb.min_len == cb.max_len == 2
    if request.param == "fixed16":
        assert cb.min_len == cb.max_len == 16
    whole = str(d / "whole.compressed")
    with open(whole, "wb") as f:
        f.write(blob)
    return dict(name=request.param, data=data, blob=blob, info=info, nb=nb, seek=seek, payload_byte=hinfo.payload_byte,
                whole=whole, dir=d)


# ---- damage -----------------------------------------------------------------------------------------------
def _flip(raw, inp, bit):
    raw[inp["payload_byte"] + bit // 8] ^= 0x80 >> (bit % 8)


def _middle(inp, b):
    return (inp["seek"][b] + inp["seek"][b + 1]) // 2


def _set_entry(raw, inp, i, value):
    at = inp["info"]["seek_off"] + 8 * i
    raw[at:at + 8] = int(value).to_bytes(8, "little")


def _write(inp, name, raw):
    path = str(inp["dir"] / name)
    with open(path, "wb") as f:
        f.write(raw)
    return path


# ---- the call and its judge ---------------------------------------------------------------------------------
def _judge(inp, bad, out, keep):
    """The output against the original: its size, every block not listed, every listed block, the odd byte."""
    data, n = inp["data"], len(inp["data"])
    assert len(out) == n
    body = n // 2 * 2
    for b in range(inp["nb"]):
        lo, hi = BLOCK * b, min(BLOCK * (b + 1), body)
        if b not in bad:
            assert out[lo:hi] == data[lo:hi], ("block", b)
        elif not keep:
            assert out[lo:hi] == bytes(hi - lo), ("block", b)
    assert out[body:] == data[body:]


def _salvage(hz, inp, path, keep=False):
    """salvage at both windows, with and without an output: one list (returned), every output judged."""
    lists = []
    for window in WINDOWS:
        out = path + ".out%d%d" % (window, keep)
        bad = hz.salvage(path, out, window_bytes=window, keep_unverified=keep)
        assert bad == sorted(set(bad)) and all(0 <= b < inp["nb"] for b in bad)
        _judge(inp, bad, _read(out), keep)
        before = sorted(os.listdir(inp["dir"]))
        assert hz.salvage(path, None, window_bytes=window, keep_unverified=keep) == bad
        assert sorted(os.listdir(inp["dir"])) == before
        lists.append(bad)
    if not keep:
        assert hz.salvage(path) == lists[0]                  # every default: the scan
    assert lists[0] == lists[1]
    return lists[0], _read(path + ".out%d%d" % (WINDOWS[0], keep))


# ---- cases --------------------------------------------------------------------------------------------------
def test_undamaged(hz, inp):
    bad, out = _salvage(hz, inp, inp["whole"])
    assert bad == [] and out == inp["data"]
    bad, out = _salvage(hz, inp, inp["whole"], keep=True)
    assert bad == [] and out == inp["data"]


def test_one_flipped_bit_in_block_7(hz, inp):
    raw = bytearray(inp["blob"])
    _flip(raw, inp, _middle(inp, 7))
    bad, _ = _salvage(hz, inp, _write(inp, "flip7.compressed", raw))
    assert bad == [7]


def test_flips_in_several_blocks(hz, inp):
    blocks = sorted({b for b in (0, 7, 8, inp["nb"] - 1) if b < inp["nb"]})
    raw = bytearray(inp["blob"])
    for b in blocks:
        _flip(raw, inp, _middle(inp, b))
    path = _write(inp, "flips.compressed", raw)
    bad, _ = _salvage(hz, inp, path)
    assert bad == blocks
    # a capacity below the count, through ctypes: the first blocks and the full count
    lib = hz.load()
    nbad = ctypes.c_uint64()
    for cap in (0, 1, 2):
        arr = (ctypes.c_uint64 * 4)(*([99] * 4))
        rc = lib.hz_seekable_salvage_file(os.fsencode(path), None, MIN_WINDOW, 0, arr if cap else None, cap, ctypes.byref(nbad))
        assert rc == 0 and nbad.value == len(blocks) and list(arr) == blocks[:cap] + [99] * (4 - cap)


def test_the_two_bits_on_a_block_boundary(hz, inp):
    a = min(7, inp["nb"] - 2)
    raw = bytearray(inp["blob"])
    _flip(raw, inp, inp["seek"][a + 1] - 1)      # the last bit of block a
    _flip(raw, inp, inp["seek"][a + 1])          # the first bit of block a + 1
    bad, _ = _salvage(hz, inp, _write(inp, "edge.compressed", raw))
    assert bad == [a, a + 1]


@pytest.mark.parametrize("value", ["zero", "2^63", "plus1", "plus2^20"])
@pytest.mark.parametrize("entry", [5, 0, "last"])
def test_damaged_seek_entry(hz, inp, entry, value):
    i = inp["nb"] if entry == "last" else entry
    true = inp["seek"][i]
    v = {"zero": 0, "2^63": 1 << 63, "plus1": true + 1, "plus2^20": true + (1 << 20)}[value]
    raw = bytearray(inp["blob"])
    _set_entry(raw, inp, i, v)
    bad, _ = _salvage(hz, inp, _write(inp, "entry%s%s.compressed" % (entry, value), raw))
    print(inp["name"], "entry", i, value, "->", bad)
    if v == true:
        assert bad == []
    else:
        assert bad and set(bad) <= {b for b in (i - 1, i) if 0 <= b < inp["nb"]}, bad
        assert i - 1 in bad or i == 0      # the block that ends at the entry is always lost


def test_damaged_sum_word(hz, inp):
    b = 9 if inp["nb"] > 9 else inp["nb"] - 1
    raw = bytearray(inp["blob"])
    raw[inp["info"]["sums_off"] + 4 * b + 2] ^= 0x04
    path = _write(inp, "sum.compressed", raw)
    bad, _ = _salvage(hz, inp, path)
    assert bad == [b]
    bad, out = _salvage(hz, inp, path, keep=True)
    assert bad == [b] and out == inp["data"]       # the bytes were right, and keep_unverified keeps them


def test_refusals(hz, tmp_path):
    import oracle_lib
    lib = hz.load()
    data = oracle_lib.generate(3 * BLOCK + 1235, offset=0, kind=1, seed=6).tobytes()
    blob = hz.encode_seekable(data)
    info = hz.seekable_info(blob)
    nbad = ctypes.c_uint64(5)
    out = str(tmp_path / "never.bin")

    def call(path, window=MIN_WINDOW, flags=0):
        return lib.hz_seekable_salvage_file(os.fsencode(path), os.fsencode(out), window, flags, None, 0, ctypes.byref(nbad))

    def put(name, raw):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(raw)
        return path

    whole, plain = put("whole.compressed", blob), put("plain.compressed", blob[:info["image_bytes"]])
    nosums = put("nosums.compressed", hz.encode_seekable(data, sums=False))
    assert call(plain) == HZ_EFORMAT
    assert call(nosums) == HZ_EINVAL
    assert call(str(tmp_path / "missing")) == HZ_ENOENT
    assert call(whole, window=MIN_WINDOW - 1) == HZ_EINVAL
    assert call(whole, flags=2) == HZ_EINVAL
    # the header's N (its last 64 bits, low byte first) changed by 2: it parses, and differs from the footer's
    raw = bytearray(blob)
    hinfo = hz.parse_header(blob)[1]
    nbit = 8 * hinfo.payload_byte + hinfo.payload_bit - 64 + 6
    raw[nbit // 8] ^= 0x80 >> (nbit % 8)
    assert hz.parse_header(bytes(raw))[1].n == len(data) ^ 2
    other = put("other_n.compressed", raw)
    assert call(other) == HZ_EFORMAT
    assert not os.path.exists(out) and nbad.value == 0
    for path, status in ((plain, HZ_EFORMAT), (nosums, HZ_EINVAL), (other, HZ_EFORMAT), (str(tmp_path / "missing"), HZ_ENOENT)):
        with pytest.raises(hz.HZError) as e:
            hz.salvage(path)
        assert e.value.status == status
    assert call(whole) == 0 and nbad.value == 0 and _read(out) == data


def test_the_context_is_left_clean(hz, inp):
    """After salvages that met flagged blocks: the verified extract of the undamaged file passes, and a verified
    read of a damaged one still stops at its first bad block."""
    raw = bytearray(inp["blob"])
    _set_entry(raw, inp, 5, 0)
    _flip(raw, inp, _middle(inp, 2))
    path = _write(inp, "after.compressed", raw)
    bad = hz.salvage(path, window_bytes=MIN_WINDOW)
    assert 2 in bad and 4 in bad
    out = str(inp["dir"] / "after.bin")
    hz.extract_verified(inp["whole"], out, window_bytes=MIN_WINDOW)
    assert _read(out) == inp["data"]
    if inp["name"] in ("two_bit", "fixed16"):        # a flipped bit keeps the structure: the sum alone sees it
        raw = bytearray(inp["blob"])
        _flip(raw, inp, _middle(inp, 3))
        _flip(raw, inp, _middle(inp, 6))
        with pytest.raises(hz.HZError) as e:
            hz.read_seekable(_write(inp, "read.compressed", raw), [(0, len(inp["data"]))], verify=True)
        assert e.value.status == HZ_ECHECKSUM and e.value.block == 3
