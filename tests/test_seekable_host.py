"""The seekable trailer on the host (hz_seekable.cpp: no device call, so all of it runs without a GPU),
through ctypes on the built library, against tests/seekable_model.py: the writer's bytes, the footer's
parse, plain files, damaged footers, and the drop-in property -- a golden .compressed file with a trailer
behind it still decodes to the original with the CPU oracle and with the reference's own `extract`.

Tolerance: none -- every check is bit-exact."""
import ctypes
import glob
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib  # noqa: E402
import ref_stream  # noqa: E402
import seekable_model as model  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
HZ_OK, HZ_EINVAL, HZ_EFORMAT, HZ_ECAP, HZ_ENOENT = 0, -1, -5, -6, -10
SIZES = [0, 1, 2, 3, 4095, 4096, 4097, 4098, 8193]
IMAGES = [11 + r for r in range(8)] + [1000 + r for r in range(8)]   # every residue modulo 8, twice
GOLDENS = sorted(glob.glob(os.path.join(GOLD, "*.compressed")))


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _words(n, flags, seed):
    rng = np.random.default_rng(seed)
    seek = np.sort(rng.integers(0, 1 << 62, model.seek_words(n), dtype=np.uint64))
    sums = rng.integers(0, 1 << 32, model.nblocks(n), dtype=np.uint32) if flags & model.SUMS else np.zeros(0, np.uint32)
    return seek, sums


def _write(lib, image_bytes, n, seek, sums, flags):
    want = lib.hz_seekable_trailer_bytes(image_bytes, n, flags)
    out = np.full(want + 16, 0xAB, dtype=np.uint8)   # what the writer leaves alone stays 0xAB
    got = ctypes.c_uint64()
    rc = lib.hz_seekable_trailer_write(image_bytes, n, _ptr(seek) if seek.size else None, _ptr(sums) if sums.size else None,
                                       flags, _ptr(out), want, ctypes.byref(got))
    assert rc == HZ_OK and got.value == want and bytes(out[want:]) == b"\xab" * 16
    return out[:want].tobytes()


def _parse(lib, last64, file_bytes):
    from huffman_amd._lib import SeekableInfo
    info = SeekableInfo()
    buf = np.frombuffer(last64, dtype=np.uint8) if last64 is not None else None
    rc = lib.hz_seekable_footer_parse(None if buf is None else _ptr(buf), file_bytes, ctypes.byref(info))
    d = info.as_dict()
    d["reserved"] = info.reserved
    return rc, d


@pytest.mark.parametrize("flags", [0, model.SUMS])
@pytest.mark.parametrize("n", SIZES)
def test_writer_equals_the_model(built_lib, n, flags):
    for image_bytes in IMAGES:
        seek, sums = _words(n, flags, n + image_bytes)
        want = model.trailer(image_bytes, n, seek, sums, flags)
        assert built_lib.hz_seekable_trailer_bytes(image_bytes, n, flags) == len(want)
        got = _write(built_lib, image_bytes, n, seek, sums, flags)
        assert got == want, (n, image_bytes)
        rc, info = _parse(built_lib, got[-64:], image_bytes + len(got))
        assert rc == HZ_OK and info == dict(model.info(image_bytes, n, flags), reserved=0)


def test_writer_refuses(built_lib):
    lib = built_lib
    seek, sums = _words(8193, model.SUMS, 1)
    out = np.zeros(4096, dtype=np.uint8)
    got = ctypes.c_uint64()
    need = lib.hz_seekable_trailer_bytes(100, 8193, model.SUMS)
    assert need == len(model.trailer(100, 8193, seek, sums, model.SUMS))
    assert lib.hz_seekable_trailer_write(100, 8193, _ptr(seek), _ptr(sums), model.SUMS, _ptr(out), need - 1,
                                         ctypes.byref(got)) == HZ_ECAP and got.value == need
    assert lib.hz_seekable_trailer_write(100, 8193, _ptr(seek), _ptr(sums), 2, _ptr(out), 4096, ctypes.byref(got)) == HZ_EINVAL
    assert lib.hz_seekable_trailer_write(100, 8193, None, _ptr(sums), model.SUMS, _ptr(out), 4096, ctypes.byref(got)) == HZ_EINVAL
    assert lib.hz_seekable_trailer_write(100, 8193, _ptr(seek), None, model.SUMS, _ptr(out), 4096, ctypes.byref(got)) == HZ_EINVAL
    assert lib.hz_seekable_trailer_write(100, 8193, _ptr(seek), _ptr(sums), 0, _ptr(out), 4096, None) == HZ_EINVAL
    # sizes that do not fit 64 bits: no trailer, nothing written
    assert lib.hz_seekable_trailer_bytes((1 << 64) - 3, 8193, 0) == 0
    assert lib.hz_seekable_trailer_bytes((1 << 64) - 100, 1 << 40, model.SUMS) == 0
    assert lib.hz_seekable_trailer_write((1 << 64) - 3, 8193, _ptr(seek), _ptr(sums), 0, _ptr(out), 4096,
                                         ctypes.byref(got)) == HZ_EINVAL


@pytest.mark.parametrize("path", GOLDENS, ids=os.path.basename)
def test_plain_goldens_have_no_trailer(built_lib, path):
    import huffman_amd
    with open(path, "rb") as f:
        blob = f.read()
    rc, info = _parse(built_lib, blob[-64:], len(blob))
    assert rc == HZ_OK and info["present"] == 0 and info["file_bytes"] == len(blob)
    assert huffman_amd.seekable_info(path) is None and huffman_amd.seekable_info(blob) is None
    with pytest.raises(huffman_amd.HZError) as e:
        huffman_amd.load_seek(path)
    assert e.value.status == HZ_EFORMAT


def test_short_files_are_plain(built_lib):
    foot = model.footer(0, 0, 0)
    for size in (0, 1, 63):
        rc, info = _parse(built_lib, None, size)
        assert rc == HZ_OK and info["present"] == 0
        rc, info = _parse(built_lib, foot, size)   # even a good footer: a file that short cannot hold it
        assert rc == HZ_OK and info["present"] == 0


# A valid footer and, per field, values that cannot fit it. n moves by whole blocks: a change of n inside
# its last block leaves every offset as it was, and only the header's N (which the flows compare) tells.
def _mutations(image_bytes, n, flags):
    l = model.layout(image_bytes, n, flags)
    return [("version", "<I", 0), ("version", "<I", 2), ("flags", "<I", flags | 2), ("flags", "<I", flags ^ 1),
            ("flags", "<I", flags | 0x80000000), ("n", "<Q", n + 4096), ("n", "<Q", n + 2 * 4096 + 7),
            ("n", "<Q", (1 << 64) - 1), ("n", "<Q", (1 << 64) - 4096), ("image_bytes", "<Q", image_bytes + 8),
            ("image_bytes", "<Q", image_bytes - 8), ("image_bytes", "<Q", (1 << 64) - 1),
            ("seek_off", "<Q", l["seek_off"] + 8), ("seek_off", "<Q", l["seek_off"] + 1), ("seek_off", "<Q", 0),
            ("sums_off", "<Q", l["sums_off"] + 4), ("sums_off", "<Q", (1 << 63)), ("block_syms", "<I", 1024),
            ("block_syms", "<I", 0), ("zero0", "<I", 1), ("zero1", "<I", 1)]


@pytest.mark.parametrize("flags", [0, model.SUMS])
def test_a_footer_that_does_not_fit_is_eformat(built_lib, flags):
    image_bytes, n = 1003, 3 * 4096 + 5
    good = model.footer(image_bytes, n, flags)
    size = model.layout(image_bytes, n, flags)["file_bytes"]
    assert _parse(built_lib, good, size)[0] == HZ_OK and _parse(built_lib, good, size)[1]["present"] == 1
    for name, fmt, value in _mutations(image_bytes, n, flags):
        bad = bytearray(good)
        struct.pack_into(fmt, bad, model.FIELDS[name], value)
        assert bytes(bad) != good, name
        rc, info = _parse(built_lib, model.reseal(bad), size)
        assert rc == HZ_EFORMAT and info["present"] == 0, (name, value)
        rc, info = _parse(built_lib, bytes(bad), size)    # the check not recomputed: no trailer at all
        assert rc == HZ_OK and info["present"] == 0, (name, value)
    for size_off in (-8, 8, 64):                           # the right footer at the end of the wrong file
        assert _parse(built_lib, good, size + size_off)[0] == HZ_EFORMAT
    bad = bytearray(good)
    bad[0] ^= 1                                            # the magic, resealed: a plain file
    rc, info = _parse(built_lib, model.reseal(bad), size)
    assert rc == HZ_OK and info["present"] == 0


def test_info_and_load_of_a_file(built_lib, tmp_path):
    import huffman_amd
    n = 8193
    seek, sums = _words(n, model.SUMS, 5)
    image = bytes(range(251)) * 3
    for flags in (0, model.SUMS):
        p = tmp_path / ("t%d" % flags)
        p.write_bytes(image + model.trailer(len(image), n, seek, sums, flags))
        assert huffman_amd.seekable_info(p) == model.info(len(image), n, flags)
        assert huffman_amd.seekable_info(p.read_bytes()) == model.info(len(image), n, flags)
        got = huffman_amd.load_seek(p)
        assert got.dtype == np.uint64 and np.array_equal(got, seek)
        got = huffman_amd.load_sums(p)
        assert got is None if not flags else (got.dtype == np.uint32 and np.array_equal(got, sums))
    lib = built_lib
    nsym = ctypes.c_uint64()
    path = os.fsencode(str(tmp_path / "t1"))
    buf = np.zeros(seek.size, dtype=np.uint64)
    assert lib.hz_seekable_load_file(path, _ptr(buf), 8 * seek.size - 8, None, 0, ctypes.byref(nsym)) == HZ_ECAP
    assert nsym.value == n // 2
    sbuf = np.zeros(sums.size, dtype=np.uint32)
    assert lib.hz_seekable_load_file(path, _ptr(buf), 8 * seek.size, _ptr(sbuf), 4 * sums.size - 4, ctypes.byref(nsym)) == HZ_ECAP
    assert lib.hz_seekable_load_file(os.fsencode(str(tmp_path / "t0")), _ptr(buf), 8 * seek.size, _ptr(sbuf), 4 * sums.size,
                                     ctypes.byref(nsym)) == HZ_EINVAL   # sums asked of a file without them
    assert lib.hz_seekable_load_file(os.fsencode(str(tmp_path / "none")), _ptr(buf), 8 * seek.size, None, 0,
                                     ctypes.byref(nsym)) == HZ_ENOENT
    from huffman_amd._lib import SeekableInfo
    assert lib.hz_seekable_info_file(os.fsencode(str(tmp_path / "none")), ctypes.byref(SeekableInfo())) == HZ_ENOENT


def test_new_entry_points_refuse_before_any_device_call(built_lib):
    """Bad arguments, a missing file and a plain file are decided on the host: these statuses come back
    where there is no GPU at all."""
    lib = built_lib
    import huffman_amd
    bad = ctypes.c_uint64()
    off = np.zeros(1, dtype=np.uint64)
    cnt = np.full(1, 4, dtype=np.uint64)
    out = np.zeros(16, dtype=np.uint8)
    missing = os.path.join(GOLD, "no-such-file.compressed").encode()
    plain = GOLDENS[0].encode()
    assert lib.hz_seekable_read_file(None, _ptr(off), _ptr(cnt), 1, _ptr(out), 0, ctypes.byref(bad)) == HZ_EINVAL
    assert lib.hz_seekable_read_file(missing, _ptr(off), _ptr(cnt), 1, _ptr(out), 0, ctypes.byref(bad)) == HZ_ENOENT
    assert lib.hz_seekable_read_file(plain, _ptr(off), _ptr(cnt), 1, _ptr(out), 0, ctypes.byref(bad)) == HZ_EFORMAT
    assert lib.hz_seekable_verify_file(missing, ctypes.byref(bad)) == HZ_ENOENT
    assert lib.hz_seekable_verify_file(plain, None) == HZ_EFORMAT
    assert lib.hz_seekable_read_host(None, 0, _ptr(off), _ptr(cnt), 1, _ptr(out), 0, None) == HZ_EINVAL
    assert lib.hz_encode_host_seekable(_ptr(out), 16, _ptr(out), 16, ctypes.byref(bad), 2) == HZ_EINVAL
    assert lib.hz_archive_stream_seekable(plain, b"/nonexistent-dir/x", 1 << 20, 0, 4) == HZ_EINVAL
    assert lib.hz_archive_stream_seekable(missing, b"/nonexistent-dir/x", 1 << 20, 0, 1) == HZ_ENOENT
    assert lib.hz_block_sums(None, None, 16, None) == HZ_EINVAL
    assert [lib.hz_block_sums_bytes(v) for v in (0, 1, 4096, 4097, 3 * 4096)] == [0, 4, 4, 8, 12]
    assert lib.hz_strerror(-11) == b"decoded block does not match its checksum"
    with pytest.raises(huffman_amd.HZError) as e:
        huffman_amd.read_seekable(GOLDENS[0], [(0, 4)])
    assert e.value.status == HZ_EFORMAT and e.value.block is None
    # a trailer on a seekable image of a different original: the header's N decides
    with open(GOLDENS[0], "rb") as f:
        blob = f.read()
    _, _, _, hinfo = oracle_lib.parse_header(blob)
    n = hinfo[0] + 2
    lying = blob + model.trailer(len(blob), n, np.zeros(model.seek_words(n), np.uint64), [], 0)
    lbuf = np.frombuffer(lying, dtype=np.uint8)
    assert lib.hz_seekable_read_host(_ptr(lbuf), lbuf.size, _ptr(off), _ptr(cnt), 1, _ptr(out), 0, None) == HZ_EFORMAT


def test_sums_definition_is_zlib():
    """The closed form of the issue, against zlib on zero-extended blocks; all-0xFF is the accumulator bound."""
    assert model.adler_blocks(b"\xff" * 4096, 4096)[0] == 0x8161f0e2
    rng = np.random.default_rng(3)
    for nbytes in (1, 4095, 4096):
        d = rng.integers(0, 256, nbytes, dtype=np.uint8).astype(np.int64)
        k = np.arange(nbytes)
        a, b = (1 + d.sum()) % 65521, (4096 + ((4096 - k) * d).sum()) % 65521
        assert model.adler_blocks(d.astype(np.uint8).tobytes(), nbytes)[0] == (b << 16 | a)
    assert 4096 + 255 * 4096 * 4097 // 2 == 2139621376 < 1 << 32


# ---- drop-in: a trailer is invisible to readers that stop at the last codeword ------------------------
def _original(path):
    base = path[:-len(".compressed")]
    base = base[:-len(".baseline")] if base.endswith(".baseline") else base
    with open(base, "rb") as f:
        return f.read()


@pytest.fixture(scope="module", params=GOLDENS, ids=os.path.basename)
def with_trailer(request):
    """A golden file with the model's trailer behind it: the table from the codeword positions under the
    oracle's parse of the header, the sums from zlib."""
    with open(request.param, "rb") as f:
        blob = f.read()
    data = _original(request.param)
    _, ln, code, hinfo = oracle_lib.parse_header(blob)
    n, pay_byte, pay_bit = hinfo[0], hinfo[1], hinfo[2]
    assert n == len(data)
    sym = np.frombuffer(data[:n // 2 * 2], dtype="<u2")
    pos = ref_stream.positions(sym, ln, pay_bit)
    seek = np.concatenate([pos[0:n // 2:ref_stream.BLK], pos[n // 2:]]) if n // 2 else np.zeros(0, np.uint64)
    assert int(seek[-1]) <= 8 * (len(blob) - pay_byte)
    return data, blob + model.trailer(len(blob), n, seek, model.block_sums(data), model.SUMS)


def test_goldens_are_there():
    assert len(GOLDENS) >= 8


def test_oracle_decodes_a_file_with_a_trailer(built_lib, with_trailer):
    import huffman_amd
    data, blob = with_trailer
    assert oracle_lib.decode(blob) == data
    info = huffman_amd.seekable_info(blob)
    assert info is not None and info["n"] == len(data) and info["file_bytes"] == len(blob)


def test_reference_extract_decodes_a_file_with_a_trailer(tmp_path, with_trailer):
    exe = oracle_lib.ref_binary("extract")
    if exe is None:
        pytest.skip("reference decoder not built (oracle/Makefile ref)")
    data, blob = with_trailer
    (tmp_path / "x.compressed").write_bytes(blob)
    subprocess.run([exe, "x.compressed"], cwd=tmp_path, check=True, capture_output=True, timeout=120)
    assert (tmp_path / "DECOMPRESSED_FILE").read_bytes() == data
