"""extract_verified (hz_extract_stream_verified) end to end on the GPU: the streaming extract of a seekable file
with sums, every 4 KiB block checked against its stored sum before its round is written. Whole files come
back byte for byte; damage that keeps the stream's structure (one flipped payload bit under a code whose
every word is 2 bits) stops the extract at the round that holds it and leaves the verified rounds before it;
a stored sums word that is wrong is named; a stored table word that is wrong gives a complete, correct output
and HZ_EFORMAT; and on every file extract_verified and verify_seekable agree.

Tolerance: none -- every check is bit-exact."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_gpu_seekable import INPUTS, _data  # noqa: E402

pytestmark = pytest.mark.gpu

HZ_EINVAL, HZ_EFORMAT, HZ_ECHECKSUM = -1, -5, -11
WINDOWS = [16384, 65536]
NSYM = 131072            # the two-bit stream: 64 blocks, 32 KiB of payload
BAD_BLOCK = 37


@pytest.fixture(scope="module")
def hz(built_lib):
    import huffman_amd
    return huffman_amd


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _status(hz, fn):
    """(status, block) of a call: (0, None) when it returns, the block only with HZ_ECHECKSUM."""
    try:
        fn()
    except hz.HZError as e:
        return e.status, (e.block if e.status == HZ_ECHECKSUM else None)
    return 0, None


def _agree(hz, path, want):
    """extract_verified (check only) and verify_seekable on one file: both give `want`."""
    got = _status(hz, lambda: hz.extract_verified(path, window_bytes=16384))
    old = _status(hz, lambda: hz.verify_seekable(path))
    print("%s: extract_verified %s, verify_seekable %s" % (os.path.basename(path), got, old))
    assert got == old == want


@pytest.fixture(scope="module", params=INPUTS)
def made(request, hz, tmp_path_factory):
    d = tmp_path_factory.mktemp("verified")
    data = _data(request.param)
    src, plain, seekable, nosums = (str(d / n) for n in ("in.bin", "plain.compressed", "seekable.compressed", "nosums.compressed"))
    with open(src, "wb") as f:
        f.write(data)
    hz.archive_stream(src, plain, chunk_bytes=1 << 20)
    hz.archive_seekable(src, seekable, chunk_bytes=65536)
    hz.archive_seekable(src, nosums, chunk_bytes=65536, sums=False)
    return dict(data=data, plain=plain, seekable=seekable, nosums=nosums, dir=d)


@pytest.mark.parametrize("window", WINDOWS)
def test_whole_files_come_back(hz, made, window):
    out = str(made["dir"] / ("out-%d.bin" % window))
    hz.extract_verified(made["seekable"], out, window_bytes=window)
    assert _read(out) == made["data"]                     # the odd last byte included
    before = sorted(os.listdir(made["dir"]))
    assert hz.extract_verified(made["seekable"], window_bytes=window) is None
    assert sorted(os.listdir(made["dir"])) == before      # check only: nothing written
    _agree(hz, made["seekable"], (0, None))


def test_plain_file_and_trailer_without_sums(hz, made):
    out = str(made["dir"] / "never.bin")
    for path, status in ((made["plain"], HZ_EFORMAT), (made["nosums"], HZ_EINVAL)):
        for o in (out, None):
            assert _status(hz, lambda: hz.extract_verified(path, o, window_bytes=16384)) == (status, None)
        assert _status(hz, lambda: hz.verify_seekable(path)) == (status, None)
    assert not os.path.exists(out)
    assert _status(hz, lambda: hz.extract_verified(made["seekable"], out, window_bytes=16383)) == (HZ_EINVAL, None)
    assert not os.path.exists(out)


# ---- damage that keeps the structure ------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_bit(hz, tmp_path_factory):
    """131 072 symbols from four 16-bit values with equal counts: every code is 2 bits, so a flipped payload
    bit changes one symbol and no length, and every block still ends where the table says. 32 KiB of payload
    and 64 blocks: a 16384-byte window takes many rounds."""
    rng = np.random.default_rng(12)
    sym = rng.permutation(np.repeat(np.array([0x1234, 0x00ff, 0xabcd, 0x8000], dtype="<u2"), NSYM // 4))
    data = sym.tobytes()
    blob = hz.encode_seekable(data)
    cb, hinfo = hz.parse_header(blob)
    assert cb.nsym == 4 and cb.min_len == cb.max_len == 2
    info = hz.seekable_info(blob)
    assert info["nblocks"] == 64 and info["image_bytes"] - hinfo.payload_byte in (NSYM // 4, NSYM // 4 + 1)
    seek = np.frombuffer(blob, dtype="<u8", count=65, offset=info["seek_off"])
    assert [int(b - a) for a, b in zip(seek, seek[1:])] == [4096] * 64
    return dict(data=data, blob=blob, info=info, seek=seek, cb=cb, hinfo=hinfo, dir=tmp_path_factory.mktemp("two_bit"))


def _write(tb, name, raw):
    path = str(tb["dir"] / name)
    with open(path, "wb") as f:
        f.write(raw)
    return path


def test_flipped_payload_bit_leaves_a_verified_prefix(hz, two_bit):
    import ref_stream
    data, info, hinfo = two_bit["data"], two_bit["info"], two_bit["hinfo"]
    bit = int(two_bit["seek"][BAD_BLOCK]) + 1001
    raw = bytearray(two_bit["blob"])
    raw[hinfo.payload_byte + bit // 8] ^= 0x80 >> (bit % 8)
    # on the CPU: the flipped stream still decodes to 131 072 symbols that end where the original's end, and
    # differs from it in one symbol of block 37 -- the only failure is the sum
    _, ln, code = hz.codebook_arrays(two_bit["cb"])
    payload = np.frombuffer(bytes(raw[hinfo.payload_byte:info["image_bytes"]]), dtype=np.uint8)
    end = int(two_bit["seek"][-1])
    n, xit, sym = ref_stream.span_decode(payload, ln, code, hinfo.payload_bit, end)
    assert (n, xit) == (NSYM, end)
    diff = np.nonzero(sym != np.frombuffer(data, dtype="<u2"))[0]
    assert diff.size == 1 and int(diff[0]) // 2048 == BAD_BLOCK
    assert hz.seekable_info(bytes(raw)) == info
    path = _write(two_bit, "payload.compressed", raw)
    for W in (16384, 65536):
        out = str(two_bit["dir"] / ("payload-%d.bin" % W))
        with pytest.raises(hz.HZError) as e:
            hz.extract_verified(path, out, window_bytes=W)
        assert e.value.status == HZ_ECHECKSUM and e.value.block == BAD_BLOCK
        size = os.path.getsize(out)
        print("window %d: verified prefix of %d bytes (block %d begins at %d)" % (W, size, BAD_BLOCK, BAD_BLOCK * 4096))
        # whole rounds before the failing one: a round writes at most W bytes
        assert size % 4096 == 0 and BAD_BLOCK * 4096 - W < size <= BAD_BLOCK * 4096
        assert _read(out) == data[:size]
    assert os.path.getsize(str(two_bit["dir"] / "payload-16384.bin")) > 0      # many rounds: some came before
    _agree(hz, path, (HZ_ECHECKSUM, BAD_BLOCK))


@pytest.mark.parametrize("j", [0, 21, 63])
def test_wrong_stored_sums_word_is_named(hz, two_bit, j):
    data, info = two_bit["data"], two_bit["info"]
    raw = bytearray(two_bit["blob"])
    raw[info["sums_off"] + 4 * j + 1] ^= 0x10
    path = _write(two_bit, "sums%d.compressed" % j, raw)
    out = str(two_bit["dir"] / ("sums%d.bin" % j))
    with pytest.raises(hz.HZError) as e:
        hz.extract_verified(path, out, window_bytes=16384)
    assert e.value.status == HZ_ECHECKSUM and e.value.block == j
    size = os.path.getsize(out)
    assert size % 4096 == 0 and j * 4096 - 16384 < size <= j * 4096 and _read(out) == data[:size]
    _agree(hz, path, (HZ_ECHECKSUM, j))


def test_wrong_stored_table_word_is_eformat_with_a_complete_output(hz, two_bit):
    """Entry 5 moved one codeword on, the footer's own check still valid (it covers the footer alone): every
    block matches its sum, so the output is complete and correct; the status says the stored table is not
    this payload's."""
    data, info = two_bit["data"], two_bit["info"]
    raw = bytearray(two_bit["blob"])
    word = info["seek_off"] + 8 * 5
    raw[word:word + 8] = int(int(two_bit["seek"][5]) + 2).to_bytes(8, "little")
    assert hz.seekable_info(bytes(raw)) == info
    path = _write(two_bit, "table.compressed", raw)
    out = str(two_bit["dir"] / "table.bin")
    assert _status(hz, lambda: hz.extract_verified(path, out, window_bytes=16384)) == (HZ_EFORMAT, None)
    assert _read(out) == data
    _agree(hz, path, (HZ_EFORMAT, None))


def test_undamaged_two_bit_file(hz, two_bit):
    path = _write(two_bit, "whole.compressed", two_bit["blob"])
    out = str(two_bit["dir"] / "whole.bin")
    hz.extract_verified(path, out, window_bytes=16384)
    assert _read(out) == two_bit["data"]
    _agree(hz, path, (0, None))
