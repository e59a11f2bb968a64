"""What hz_seekable_attach_file, hz_extract_stream_verified and hz_block_sums_check decide before any device
call, so without a GPU: refused arguments, a missing file, a plain file and a trailer without sums for the
verified extract, and a file whose trailer already holds what the attach asks for (left untouched). The
trailers are the model's (tests/seekable_model.py) behind arbitrary image bytes: none of these paths reads
the image."""
import ctypes
import os

import numpy as np
import pytest

import seekable_model as model

HZ_EINVAL, HZ_EFORMAT, HZ_ENOENT = -1, -5, -10
MIN_WINDOW = 16384


@pytest.fixture(scope="module")
def lib(built_lib):
    return built_lib


def _with_trailer(n, flags):
    image = bytes(range(256)) * 3 + b"\x07" * 5
    seek = np.arange(model.seek_words(n), dtype=np.uint64) * np.uint64(4096)
    sums = np.arange(model.nblocks(n), dtype=np.uint32)
    return image + model.trailer(len(image), n, seek, sums if flags & model.SUMS else [], flags)


def test_min_window_is_one_block_of_the_longest_codes():
    from huffman_amd import _lib
    assert _lib.HZ_SEEKABLE_MIN_WINDOW == MIN_WINDOW >= 2048 * 56 // 8
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "huffman_amd.h")) as f:
        assert "#define HZ_SEEKABLE_MIN_WINDOW 16384" in f.read()


def test_attach_refusals(lib, tmp_path):
    path = tmp_path / "plain.compressed"
    path.write_bytes(b"\x01" * 100)
    p = os.fsencode(str(path))
    attached = ctypes.c_int(7)
    assert lib.hz_seekable_attach_file(None, MIN_WINDOW, 0, ctypes.byref(attached)) == HZ_EINVAL
    assert attached.value == 0
    for flags in (2, 3, 1 << 31):
        assert lib.hz_seekable_attach_file(p, MIN_WINDOW, flags, None) == HZ_EINVAL
    for window in (0, 4096, MIN_WINDOW - 1):
        assert lib.hz_seekable_attach_file(p, window, 1, None) == HZ_EINVAL
    assert path.read_bytes() == b"\x01" * 100
    missing = os.fsencode(str(tmp_path / "missing"))
    for flags in (0, 1):
        assert lib.hz_seekable_attach_file(missing, MIN_WINDOW, flags, ctypes.byref(attached)) == HZ_ENOENT
    assert not (tmp_path / "missing").exists()
    # a window too small is refused before the file is looked at
    assert lib.hz_seekable_attach_file(missing, MIN_WINDOW - 1, 0, None) == HZ_EINVAL


@pytest.mark.parametrize("n", [0, 1, 5000, 3 * 4096])
def test_attach_leaves_a_file_that_has_what_is_asked(lib, tmp_path, n):
    for have, ask in ((model.SUMS, model.SUMS), (model.SUMS, 0), (0, 0)):
        raw = _with_trailer(n, have)
        path = tmp_path / ("t%d%d" % (have, ask))
        path.write_bytes(raw)
        before = os.stat(path).st_mtime_ns
        attached = ctypes.c_int(7)
        assert lib.hz_seekable_attach_file(os.fsencode(str(path)), MIN_WINDOW, ask, ctypes.byref(attached)) == 0
        assert attached.value == 0 and path.read_bytes() == raw and os.stat(path).st_mtime_ns == before
        assert lib.hz_seekable_attach_file(os.fsencode(str(path)), 1 << 30, ask, None) == 0


def test_verified_extract_refusals(lib, tmp_path):
    out = tmp_path / "out.bin"
    o = os.fsencode(str(out))
    bad = ctypes.c_uint64(99)
    plain = tmp_path / "plain.compressed"
    plain.write_bytes(b"\x02" * 1000)
    nosums = tmp_path / "nosums.compressed"
    nosums.write_bytes(_with_trailer(5000, 0))
    assert lib.hz_extract_stream_verified(None, o, MIN_WINDOW, 0, ctypes.byref(bad)) == HZ_EINVAL
    assert lib.hz_extract_stream_verified(os.fsencode(str(plain)), o, MIN_WINDOW - 1, 0, None) == HZ_EINVAL
    assert lib.hz_extract_stream_verified(os.fsencode(str(tmp_path / "missing")), o, MIN_WINDOW, 0, None) == HZ_ENOENT
    for dst in (o, None):
        assert lib.hz_extract_stream_verified(os.fsencode(str(plain)), dst, MIN_WINDOW, 0, ctypes.byref(bad)) == HZ_EFORMAT
        assert lib.hz_extract_stream_verified(os.fsencode(str(nosums)), dst, MIN_WINDOW, 0, None) == HZ_EINVAL
    assert not out.exists() and bad.value == 99


def test_block_sums_check_refuses_a_null_context(lib):
    assert lib.hz_block_sums_check(None, None, 16, None, 0, None) == HZ_EINVAL
