"""Seekable files end to end on the GPU: archive_seekable / encode_seekable write the plain writer's image
and the model's trailer (tests/seekable_model.py: the table build_seek finds in the image, zlib's sums of
the original); read_seekable returns the original's bytes through the trailer, by path and from bytes,
with and without verification; every existing reader gives on the seekable file what it gives on the plain
one; a by-path read touches only the bytes it needs; and damage that keeps the stream's structure -- which
the unverified read cannot see -- is caught by the block sums.

Tolerance: none -- every check is bit-exact."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import seekable_model as model  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden")
HZ_EFORMAT, HZ_ECHECKSUM = -5, -11
CHUNKS = [4096, 65536, 1 << 30]
INPUTS = ["romeo.txt", "synth_zipf_4099.bin", "synth_unif_65536.bin", "synth_zipf_65537.bin", "zipf-1MiB+3",
          "bytes-0", "bytes-1", "bytes-2", "bytes-4097"]


@pytest.fixture(scope="module")
def hz(built_lib):
    import huffman_amd
    return huffman_amd


def _data(name):
    import oracle_lib
    if name == "zipf-1MiB+3":
        return oracle_lib.generate((1 << 20) + 3, offset=0, kind=1, seed=31).tobytes()
    if name.startswith("bytes-"):
        return oracle_lib.generate(int(name[6:]), offset=5, kind=1, seed=77).tobytes()
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


def _make(hz, d, name):
    """An input archived once each way: the original, the plain file and its bytes, the seekable file
    (chunk 65536, with sums) and its bytes, and the directory."""
    data = _data(name)
    src, plain, seekable = str(d / "in.bin"), str(d / "plain.compressed"), str(d / "seekable.compressed")
    with open(src, "wb") as f:
        f.write(data)
    hz.archive_stream(src, plain, chunk_bytes=1 << 20)
    assert hz.archive_seekable(src, seekable, chunk_bytes=65536) == seekable
    with open(plain, "rb") as f:
        pblob = f.read()
    with open(seekable, "rb") as f:
        sblob = f.read()
    return dict(data=data, src=src, plain=plain, pblob=pblob, seekable=seekable, sblob=sblob, dir=d)


@pytest.fixture(scope="module", params=INPUTS)
def made(request, hz, tmp_path_factory):
    return _make(hz, tmp_path_factory.mktemp("seekable"), request.param)


@pytest.fixture(scope="module")
def made_zipf(hz, tmp_path_factory):
    return _make(hz, tmp_path_factory.mktemp("seekable_zipf"), "zipf-1MiB+3")


def _want(hz, data, pblob, sums):
    flags = model.SUMS if sums else 0
    return pblob + model.trailer(len(pblob), len(data), hz.build_seek(pblob), model.block_sums(data) if sums else [], flags)


# ---- writers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", CHUNKS)
def test_archive_seekable_is_image_plus_model_trailer(hz, made, chunk):
    data, pblob = made["data"], made["pblob"]
    out = str(made["dir"] / ("s%d.compressed" % chunk))
    hz.archive_seekable(made["src"], out, chunk_bytes=chunk)
    with open(out, "rb") as f:
        got = f.read()
    assert got[:len(pblob)] == pblob
    assert got == _want(hz, data, pblob, True)
    info = hz.seekable_info(out)
    assert info == model.info(len(pblob), len(data), model.SUMS)
    assert np.array_equal(hz.load_seek(out), hz.build_seek(pblob))
    assert np.array_equal(hz.load_sums(out), model.block_sums(data))


def test_archive_seekable_without_sums_and_default_name(hz, made):
    data, pblob = made["data"], made["pblob"]
    assert hz.archive_seekable(made["src"], sums=False, chunk_bytes=8192) == made["src"] + ".compressed"
    with open(made["src"] + ".compressed", "rb") as f:
        assert f.read() == _want(hz, data, pblob, False)
    assert hz.load_sums(made["src"] + ".compressed") is None


def test_encode_seekable_is_image_plus_model_trailer(hz, made):
    data, pblob = made["data"], made["pblob"]
    assert hz.encode(data) == pblob
    assert hz.encode_seekable(data) == _want(hz, data, pblob, True) == made["sblob"]
    assert hz.encode_seekable(data, sums=False) == _want(hz, data, pblob, False)


# ---- readers ------------------------------------------------------------------------------------------
def _ranges(n):
    """Odd offsets and ends, a block boundary inside, empty, a repeat, the last partial block and the odd
    last byte, the whole: those that fit n."""
    want = [(1, 5), (4095, 3), (4091, 4202), (7, 0), (1, 5), (n - 1, 1), (n - 4097, 4097), (n - 3, 3), (n, 0), (0, n),
            (3 * 4096 + 1, 2 * 4096 + 1)]
    return [(o, c) for o, c in want if o >= 0 and o + c <= n]


@pytest.mark.parametrize("verify", [False, True])
@pytest.mark.parametrize("by_path", [True, False])
def test_read_seekable(hz, made, by_path, verify):
    data = made["data"]
    rg = _ranges(len(data))
    got = hz.read_seekable(made["seekable"] if by_path else made["sblob"], rg, verify=verify)
    assert got == [data[o:o + c] for o, c in rg]
    assert hz.read_seekable(made["seekable"] if by_path else made["sblob"], [], verify=verify) == []
    for o, c in [(len(data), 1), (len(data) + 1, 0)]:
        with pytest.raises(hz.HZError) as e:
            hz.read_seekable(made["seekable"] if by_path else made["sblob"], [(0, 0), (o, c)], verify=verify)
        assert e.value.status == -1


def test_plain_file_is_eformat(hz, made):
    for src in (made["plain"], made["pblob"]):
        with pytest.raises(hz.HZError) as e:
            hz.read_seekable(src, [(0, 0)])
        assert e.value.status == HZ_EFORMAT
    with pytest.raises(hz.HZError) as e:
        hz.verify_seekable(made["plain"])
    assert e.value.status == HZ_EFORMAT


def test_verify_without_sums_is_einval(hz, made):
    blob = hz.encode_seekable(made["data"], sums=False)
    with pytest.raises(hz.HZError) as e:
        hz.read_seekable(blob, [(0, 0)], verify=True)
    assert e.value.status == -1
    assert hz.read_seekable(blob, _ranges(len(made["data"]))) == [made["data"][o:o + c] for o, c in _ranges(len(made["data"]))]


def test_verify_seekable_passes(hz, made):
    hz.verify_seekable(made["seekable"])


def test_existing_readers_ignore_the_trailer(hz, made):
    data, pblob, sblob = made["data"], made["pblob"], made["sblob"]
    out = str(made["dir"] / "extracted.bin")
    for window in (4096, 1 << 30):
        hz.extract_stream(made["seekable"], out, chunk_bytes=window)
        with open(out, "rb") as f:
            assert f.read() == data
    assert hz.decode(sblob) == hz.decode(pblob) == data
    seek = hz.build_seek(pblob)
    assert np.array_equal(hz.build_seek(sblob), seek)
    assert np.array_equal(hz.build_seek_file(made["seekable"]), hz.build_seek_file(made["plain"]))
    assert np.array_equal(hz.build_seek_file(made["seekable"], window_bytes=4096), seek)
    table = hz.load_seek(made["seekable"])
    assert np.array_equal(table, seek)
    rg = _ranges(len(data))
    want = [data[o:o + c] for o, c in rg]
    for o, c in rg:
        assert hz.decode_range_file(made["seekable"], table, o, c) == hz.decode_range_file(made["plain"], table, o, c) \
            == data[o:o + c]
        assert hz.decode_range(sblob, table, o, c) == data[o:o + c]
    assert hz.decode_ranges_file(made["seekable"], table, rg) == hz.decode_ranges_file(made["plain"], table, rg) == want
    assert hz.decode_ranges(sblob, table, rg) == hz.decode_ranges(sblob, table, rg, pieces=True) == want


def test_extract_cli_ignores_the_trailer(hz, made_zipf):
    import subprocess
    made = made_zipf
    d = made["dir"] / "cli"
    d.mkdir()
    subprocess.run([os.path.join(hz.BIN_DIR, "extract"), made["seekable"]], cwd=d, check=True, capture_output=True, timeout=120)
    assert (d / "DECOMPRESSED_FILE").read_bytes() == made["data"]


# ---- what a by-path read touches ----------------------------------------------------------------------
def _rchar():
    """(bytes this process has read so far, bytes of the one read that asked): the counter is shown as it
    stood before that read, so the next look counts them."""
    fd = os.open("/proc/self/io", os.O_RDONLY)
    try:
        text = os.read(fd, 4096)
    finally:
        os.close(fd)
    for line in text.decode().split("\n"):
        if line.startswith("rchar:"):
            return int(line.split()[1]), len(text)
    raise AssertionError("no rchar in /proc/self/io")


BY_PATH = [(10 * 4096 + 100, 100), (200 * 4096 + 1001, 100)]    # two 100-byte ranges, each inside one block


def test_by_path_read_touches_only_what_it_needs(hz, made_zipf):
    """The bytes the process reads during the call (rchar of /proc/self/io counts every pread) stay below
    the footer, the header read (the file's first bytes, at most 1 MiB: of this file, which is smaller, the
    whole image), two blocks of at most 4 KiB of payload with their margins, and 64 bytes of table and
    sums. And they are exactly the list in include/huffman_amd.h: the footer, the header read, each range's
    hz_seek_span bytes, two table words per range and, verified, one sums word per block -- so nothing of
    the table's other 254 words is read. What the result depends on is the next test's."""
    from huffman_amd import _lib
    made = made_zipf
    data = made["data"]
    rg = BY_PATH
    want = [data[o:o + c] for o, c in rg]
    info = hz.seekable_info(made["seekable"])
    header = min(info["image_bytes"], 1 << 20)
    margins = _lib.HZ_RANGE_LEAD_BYTES + _lib.HZ_RANGE_TAIL_BYTES + 16
    bound = 64 + header + 2 * (4096 + margins) + 64
    seek = hz.load_seek(made["seekable"])
    _, hinfo = hz.parse_header(made["sblob"])
    spans = 0
    for off, cnt in rg:
        bb, be = hz.seek_span(seek, info["nsym"], off // 2, (off + cnt + 1) // 2 - off // 2)
        spans += min(be, info["image_bytes"] - hinfo.payload_byte) - bb
    for verify in (False, True):
        hz.read_seekable(made["seekable"], rg, verify=verify)   # everything the first call loads is loaded
        before, asked = _rchar()
        got = hz.read_seekable(made["seekable"], rg, verify=verify)
        read = _rchar()[0] - before - asked
        assert got == want
        print("by-path read, verify=%s: %d bytes read, bound %d" % (verify, read, bound))
        assert read < bound
        assert read == 64 + header + spans + 2 * 16 + (2 * 4 if verify else 0)


def test_by_path_read_depends_only_on_what_it_needs(hz, made_zipf):
    """Every payload byte outside the two ranges' hz_seek_span bytes, every table word but the two blocks'
    entries and every sums word but theirs overwritten with 0xFF in a copy of the file: the ranges still
    read right, verified too, so nothing else of payload, table or sums decides the result."""
    made = made_zipf
    data, blob = made["data"], made["sblob"]
    info = hz.seekable_info(blob)
    _, hinfo = hz.parse_header(blob)
    seek = hz.load_seek(made["seekable"])
    pay0, pay1 = hinfo.payload_byte, info["image_bytes"]
    raw = np.full(len(blob), 0xFF, dtype=np.uint8)
    src = np.frombuffer(blob, dtype=np.uint8)
    raw[:pay0 + 1] = src[:pay0 + 1]          # the header's last bits share the payload's first byte
    raw[-64:] = src[-64:]
    for off, cnt in BY_PATH:
        s0, s1 = off // 2, (off + cnt + 1) // 2
        b = s0 // 2048
        assert (s1 - 1) // 2048 == b
        bb, be = hz.seek_span(seek, info["nsym"], s0, s1 - s0)
        be = min(be, pay1 - pay0)
        raw[pay0 + bb:pay0 + be] = src[pay0 + bb:pay0 + be]
        for lo, hi in ((info["seek_off"] + 8 * b, info["seek_off"] + 8 * (b + 2)),
                       (info["sums_off"] + 4 * b, info["sums_off"] + 4 * (b + 1))):
            raw[lo:hi] = src[lo:hi]
    assert (raw != src).sum() > len(blob) // 2
    path = str(made["dir"] / "scribbled.compressed")
    raw.tofile(path)
    want = [data[o:o + c] for o, c in BY_PATH]
    for verify in (False, True):
        assert hz.read_seekable(path, BY_PATH, verify=verify) == want
        assert hz.read_seekable(raw.tobytes(), BY_PATH, verify=verify) == want


# ---- damage that keeps the structure ------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_bit(hz, tmp_path_factory):
    """8192 symbols from four 16-bit values with equal counts: every code is 2 bits, so a flipped payload
    bit changes one symbol and no length -- nothing desynchronises and every block still ends where the
    table says. The original, its seekable image, and where things stand in it."""
    rng = np.random.default_rng(11)
    sym = rng.permutation(np.repeat(np.array([0x1234, 0x00ff, 0xabcd, 0x8000], dtype="<u2"), 2048))
    data = sym.tobytes()
    blob = hz.encode_seekable(data)
    cb, hinfo = hz.parse_header(blob)
    assert cb.nsym == 4 and cb.min_len == cb.max_len == 2
    info = hz.seekable_info(blob)
    seek = np.frombuffer(blob, dtype="<u8", count=5, offset=info["seek_off"])
    assert [int(b - a) for a, b in zip(seek, seek[1:])] == [4096] * 4
    return dict(data=data, blob=blob, info=info, seek=seek, payload_byte=hinfo.payload_byte,
                dir=tmp_path_factory.mktemp("two_bit"))


def _flip_payload_bit(tb, bit):
    raw = bytearray(tb["blob"])
    raw[tb["payload_byte"] + bit // 8] ^= 0x80 >> (bit % 8)
    return bytes(raw)


def test_flipped_payload_bit_passes_unverified_and_fails_verified(hz, two_bit):
    data = two_bit["data"]
    bad = _flip_payload_bit(two_bit, int(two_bit["seek"][1]) + 1001)      # in block 1
    path = str(two_bit["dir"] / "payload.compressed")
    with open(path, "wb") as f:
        f.write(bad)
    assert hz.seekable_info(bad) == two_bit["info"]
    for src in (bad, path):
        got = hz.read_seekable(src, [(4096, 4096)])                       # the gap: HZ_OK and wrong bytes
        assert len(got[0]) == 4096 and got[0] != data[4096:8192]
        assert sum(a != b for a, b in zip(got[0], data[4096:8192])) <= 2  # one symbol
        for rg in ([(4096, 4096)], [(0, len(data))], [(9000, 10), (5000, 1)]):
            with pytest.raises(hz.HZError) as e:
                hz.read_seekable(src, rg, verify=True)
            assert e.value.status == HZ_ECHECKSUM and e.value.block == 1
        assert hz.read_seekable(src, [(0, 4096), (8192, 8192)], verify=True) == [data[:4096], data[8192:]]
    with pytest.raises(hz.HZError) as e:
        hz.verify_seekable(path)
    assert e.value.status == HZ_ECHECKSUM and e.value.block == 1


def test_flipped_sums_word_fails_verified_only(hz, two_bit):
    data, info = two_bit["data"], two_bit["info"]
    raw = bytearray(two_bit["blob"])
    raw[info["sums_off"] + 4 * 2 + 1] ^= 0x10                             # block 2's word
    path = str(two_bit["dir"] / "sums.compressed")
    with open(path, "wb") as f:
        f.write(raw)
    for src in (bytes(raw), path):
        assert hz.read_seekable(src, [(0, len(data))]) == [data]
        with pytest.raises(hz.HZError) as e:
            hz.read_seekable(src, [(0, len(data))], verify=True)
        assert e.value.status == HZ_ECHECKSUM and e.value.block == 2
        assert hz.read_seekable(src, [(0, 8192), (3 * 4096, 4096)], verify=True) == [data[:8192], data[3 * 4096:]]
    with pytest.raises(hz.HZError) as e:
        hz.verify_seekable(path)
    assert e.value.status == HZ_ECHECKSUM and e.value.block == 2


def test_out_is_not_written_on_a_mismatch(hz, two_bit):
    import ctypes
    bad = np.frombuffer(_flip_payload_bit(two_bit, int(two_bit["seek"][1]) + 1), dtype=np.uint8)
    out = np.full(8192, 0xEE, dtype=np.uint8)
    offs, cnts = np.array([0], dtype=np.uint64), np.array([8192], dtype=np.uint64)
    blk = ctypes.c_uint64(99)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lib = hz.load()
    assert lib.hz_seekable_read_host(p(bad), bad.size, p(offs), p(cnts), 1, p(out), 2, ctypes.byref(blk)) == HZ_ECHECKSUM
    assert blk.value == 1 and bytes(out) == b"\xee" * 8192
    assert lib.hz_seekable_read_host(p(bad), bad.size, p(offs), p(cnts), 1, p(out), 2, None) == HZ_ECHECKSUM
