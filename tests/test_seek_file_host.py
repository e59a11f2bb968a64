"""What the seek-table entry points decide on the host, before any device call (so all of it runs
without a GPU): the exported names and their argument types, the status of a missing file and of bad
arguments, and the entry rule of a seek table."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_stream  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
HZ_OK, HZ_EINVAL, HZ_ECAP, HZ_ENOENT = 0, -1, -6, -10
NAMES = ["hz_seek_build", "hz_decode_indexless_seek", "hz_indexless_seek", "hz_extract_stream_seek",
         "hz_decode_range_file"]
MISSING = os.path.join(GOLD, "no-such-file.compressed").encode()
ROMEO = os.path.join(GOLD, "romeo.txt.baseline.compressed").encode()


def _declared_params(name):
    """Parameter count of `int name(...)` in include/huffman_amd.h."""
    with open(os.path.join(ROOT, "include", "huffman_amd.h")) as f:
        text = f.read()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name
    return len([p for p in m.group(1).split(",") if p.strip()])


# ---- 12 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_exported_with_declared_argtypes(built_lib, name):
    from huffman_amd._lib import PROTOTYPES
    proto = {n: (res, args) for n, res, args in PROTOTYPES}
    assert name in proto and hasattr(built_lib, name)
    res, args = proto[name]
    fn = getattr(built_lib, name)
    assert fn.restype is res is ctypes.c_int and list(fn.argtypes) == args
    assert len(args) == _declared_params(name)


def test_python_forms_exist(built_lib):
    import huffman_amd
    from huffman_amd.pipeline import StreamCodec
    for name in ("build_seek_file", "decode_range_file"):
        assert callable(getattr(huffman_amd, name)) and name in huffman_amd.__all__
    for name in ("seek_build", "decode_indexless_seek", "indexless_seek"):
        assert callable(getattr(huffman_amd.Device, name))
    assert callable(StreamCodec.seek_build)


# ---- 13 ------------------------------------------------------------------------------------------------
def test_missing_file_is_enoent(built_lib):
    lib = built_lib
    seek = np.zeros(4, dtype=np.uint64)
    out = np.zeros(16, dtype=np.uint8)
    nsym = ctypes.c_uint64(77)
    assert lib.hz_decode_range_file(MISSING, seek.ctypes.data_as(ctypes.c_void_p), 0, 8,
                                    out.ctypes.data_as(ctypes.c_void_p)) == HZ_ENOENT
    for out_path in (None, os.path.join(GOLD, "never-written").encode()):
        assert lib.hz_extract_stream_seek(MISSING, out_path, 1 << 20, 0, seek.ctypes.data_as(ctypes.c_void_p), 32,
                                          ctypes.byref(nsym)) == HZ_ENOENT
    assert not os.path.exists(os.path.join(GOLD, "never-written"))
    import huffman_amd
    for call in (lambda: huffman_amd.build_seek_file(MISSING.decode()),
                 lambda: huffman_amd.decode_range_file(MISSING.decode(), seek, 0, 8)):
        with pytest.raises(huffman_amd.HZError) as e:
            call()
        assert e.value.status == HZ_ENOENT


# ---- 14 ------------------------------------------------------------------------------------------------
def test_bad_arguments_are_einval_before_any_device_call(built_lib):
    """None of these reaches the device: they return HZ_EINVAL where there is no GPU at all (a device call
    would be HZ_ENODEV or HZ_EHIP there)."""
    lib = built_lib
    seek = np.zeros(4, dtype=np.uint64)
    sp = seek.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros(16, dtype=np.uint8)
    op = out.ctypes.data_as(ctypes.c_void_p)
    nsym = ctypes.c_uint64()
    assert lib.hz_decode_range_file(None, sp, 0, 8, op) == HZ_EINVAL
    assert lib.hz_extract_stream_seek(None, None, 1 << 20, 0, sp, 32, ctypes.byref(nsym)) == HZ_EINVAL
    assert lib.hz_extract_stream_seek(ROMEO, None, 1 << 20, 0, sp, 32, None) == HZ_EINVAL
    assert lib.hz_extract_stream_seek(ROMEO, None, 4095, 0, sp, 32, ctypes.byref(nsym)) == HZ_EINVAL
    assert lib.hz_extract_stream_seek(MISSING, None, 4095, 0, sp, 32, ctypes.byref(nsym)) == HZ_EINVAL
    # no context: the device forms
    assert lib.hz_seek_build(None, op, 16, 0, 1, sp) == HZ_EINVAL
    assert lib.hz_decode_indexless_seek(None, op, 16, 0, 1, None, None, 0, 0, 1, sp) == HZ_EINVAL
    assert lib.hz_indexless_seek(None, 0, 1, 1, sp) == HZ_EINVAL


def test_range_file_host_side_of_an_existing_file(built_lib):
    """With the header parsed on the host: a range past the original's size is HZ_EINVAL, an empty range
    HZ_OK, a null table or output for a range with symbols HZ_EINVAL -- all before the device."""
    lib = built_lib
    import huffman_amd
    with open(ROMEO.decode(), "rb") as f:
        _, info = huffman_amd.parse_header(f.read())
    n = info.n
    seek = np.zeros(huffman_amd.seek_bytes(n // 2) // 8, dtype=np.uint64)
    sp = seek.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros(16, dtype=np.uint8)
    op = out.ctypes.data_as(ctypes.c_void_p)
    assert lib.hz_decode_range_file(ROMEO, sp, n, 1, op) == HZ_EINVAL
    assert lib.hz_decode_range_file(ROMEO, sp, n + 1, 0, op) == HZ_EINVAL
    assert lib.hz_decode_range_file(ROMEO, sp, 5, 0, op) == HZ_OK
    assert lib.hz_decode_range_file(ROMEO, sp, n, 0, None) == HZ_OK
    assert lib.hz_decode_range_file(ROMEO, sp, 0, 8, None) == HZ_EINVAL
    assert lib.hz_decode_range_file(ROMEO, None, 0, 8, op) == HZ_EINVAL


# ---- 15 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsym", [0, 1, 7, 2047, 2048, 2049, 5 * 2048 + 3, 40 * 2048 + 777, 1 << 20])
def test_entry_rule_agrees_with_the_model(built_lib, nsym):
    """seek_entries restates s_b = min(2048 b, nsym), b = 0 .. nblocks(nsym): one entry per seek_bytes
    word, ascending, the first codeword 0 and the last the stream's end."""
    import huffman_amd
    s = huffman_amd.seek_entries(nsym)
    assert len(s) == huffman_amd.seek_bytes(nsym) // 8
    if nsym == 0:
        assert s == []
        return
    nb = ref_stream.nblocks(nsym)
    assert len(s) == nb + 1 and s[0] == 0 and s[-1] == nsym
    assert s[:nb] == list(range(0, nsym, ref_stream.BLK))
    assert all(a < b for a, b in zip(s, s[1:]))
