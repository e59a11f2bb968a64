"""What hz_seekable_salvage_file and hz_block_sums_mark decide before any device call, so without a GPU: refused
arguments, a window below the minimum, a missing file, a plain file and a trailer without sums. The trailers are
the model's (tests/seekable_model.py) behind arbitrary image bytes: none of these paths reads the image. And the
Python names exist."""
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


def test_flags_match_the_header():
    from huffman_amd import _lib
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "huffman_amd.h")) as f:
        text = f.read()
    assert "#define HZ_SUMS_ZERO_BAD 1u" in text and _lib.HZ_SUMS_ZERO_BAD == 1
    assert "#define HZ_SALVAGE_KEEP_UNVERIFIED 1u" in text and _lib.HZ_SALVAGE_KEEP_UNVERIFIED == 1


def test_salvage_refusals(lib, tmp_path):
    plain, nosums, out = tmp_path / "plain.compressed", tmp_path / "nosums.compressed", tmp_path / "never.bin"
    plain.write_bytes(b"\x01" * 100)
    nosums.write_bytes(_with_trailer(3 * 4096, 0))
    p, o = os.fsencode(str(plain)), os.fsencode(str(out))
    nbad = ctypes.c_uint64(7)
    arr = (ctypes.c_uint64 * 2)()
    assert lib.hz_seekable_salvage_file(None, o, MIN_WINDOW, 0, None, 0, ctypes.byref(nbad)) == HZ_EINVAL
    assert nbad.value == 0
    assert lib.hz_seekable_salvage_file(p, o, MIN_WINDOW, 0, None, 0, None) == HZ_EINVAL          # nowhere to put the count
    assert lib.hz_seekable_salvage_file(p, o, MIN_WINDOW, 0, None, 2, ctypes.byref(nbad)) == HZ_EINVAL  # room without an array
    for flags in (2, 3, 1 << 31):
        assert lib.hz_seekable_salvage_file(p, o, MIN_WINDOW, flags, arr, 2, ctypes.byref(nbad)) == HZ_EINVAL
    for window in (0, 4096, MIN_WINDOW - 1):
        assert lib.hz_seekable_salvage_file(p, o, window, 0, arr, 2, ctypes.byref(nbad)) == HZ_EINVAL
    missing = os.fsencode(str(tmp_path / "missing"))
    assert lib.hz_seekable_salvage_file(missing, o, MIN_WINDOW, 0, arr, 2, ctypes.byref(nbad)) == HZ_ENOENT
    assert lib.hz_seekable_salvage_file(missing, o, MIN_WINDOW - 1, 0, arr, 2, ctypes.byref(nbad)) == HZ_EINVAL
    for dst in (o, None):
        assert lib.hz_seekable_salvage_file(p, dst, MIN_WINDOW, 0, arr, 2, ctypes.byref(nbad)) == HZ_EFORMAT
        assert lib.hz_seekable_salvage_file(os.fsencode(str(nosums)), dst, MIN_WINDOW, 0, arr, 2, ctypes.byref(nbad)) == HZ_EINVAL
    assert not out.exists() and not (tmp_path / "missing").exists()
    assert plain.read_bytes() == b"\x01" * 100


def test_block_sums_mark_refuses_before_the_device(lib):
    assert lib.hz_block_sums_mark(None, None, 16, None, 0, None, 0) == HZ_EINVAL


def test_python_names(tmp_path):
    import huffman_amd
    from huffman_amd.codec import Device
    from huffman_amd.pipeline import StreamCodec
    assert callable(huffman_amd.salvage) and "salvage" in huffman_amd.__all__
    assert callable(Device.block_sums_mark) and callable(StreamCodec.block_sums_mark)
    with pytest.raises(huffman_amd.HZError) as e:
        huffman_amd.salvage(str(tmp_path / "missing.compressed"))
    assert e.value.status == HZ_ENOENT
