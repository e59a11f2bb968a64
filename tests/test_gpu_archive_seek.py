"""The seek table from the writer at file level: huffman_amd.archive_stream_seek (hz_archive_stream_seek),
archive_seek (hz_archive_file_seek, resident and chunked) and encode_seek (hz_encode_host_seek). The
.compressed bytes equal the plain forms'; the table equals what build_seek_file finds by walking the
finished file and what build_seek finds in the image, so the tables are interchangeable; ranges read back
through decode_range_file from the writer's table; a table too small is refused before anything is
written.

Tolerance: none -- every check is bit-exact."""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden")
BLK = 2048
HZ_ECAP = -6
CHUNKS = [4096, 5000, 65536, 1 << 30]   # 5000: rounded down to 4096 by the seek form
ORIGINALS = sorted(p[:-len(".baseline.compressed")] for p in glob.glob(os.path.join(GOLD, "*.baseline.compressed")))
SMALL = [0, 1, 2, 4097]


@pytest.fixture(scope="module")
def hz(built_lib):
    import huffman_amd
    return huffman_amd


@pytest.fixture(scope="module")
def inputs(hz, tmp_path_factory):
    """name -> (path of the original, its bytes, the plain archive_stream's .compressed bytes, build_seek of
    them): the goldens' originals, a 1 MiB + 3 byte Zipf file and files of 0, 1, 2 and 4097 bytes. The
    references are computed once and shared."""
    import oracle_lib
    d = tmp_path_factory.mktemp("archseek")
    files = {os.path.basename(p): open(p, "rb").read() for p in ORIGINALS}
    files["zipf.bin"] = oracle_lib.generate((1 << 20) + 3, offset=0, kind=1, seed=31).tobytes()
    zipf = files["zipf.bin"]
    for n in SMALL:
        files["small%d.bin" % n] = zipf[:n]
    out = {}
    for name, data in files.items():
        src = str(d / name)
        with open(src, "wb") as f:
            f.write(data)
        plain = hz.archive_stream(src, str(d / (name + ".plain")), chunk_bytes=1 << 20)
        with open(plain, "rb") as f:
            blob = f.read()
        out[name] = (src, data, blob, hz.build_seek(blob))
    return out


NAMES = [os.path.basename(p) for p in ORIGINALS] + ["zipf.bin"] + ["small%d.bin" % n for n in SMALL]


def test_inputs_are_there():
    assert len(ORIGINALS) >= 4


def _same_table(got, want, nbytes):
    assert got.dtype == np.uint64
    assert got.size == (((nbytes // 2 + BLK - 1) // BLK + 1) if nbytes // 2 else 0)
    assert np.array_equal(got, want), (got[:4], want[:4])


# ---- archive_stream_seek ---------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", NAMES)
def test_archive_stream_seek(hz, tmp_path, inputs, name, chunk):
    src, data, blob, want = inputs[name]
    dst = str(tmp_path / "out.compressed")
    got = hz.archive_stream_seek(src, dst, chunk_bytes=chunk)
    t = hz.stream_timing()                            # of this call: hz_stream_last_timing covers the seek form
    assert t["bytes_in"] >= len(data) and t["bytes_out"] == len(blob) and t["total_ms"] > 0
    with open(dst, "rb") as f:
        assert f.read() == blob                       # byte-identical to archive_stream's
    _same_table(got, want, len(data))                 # build_seek(blob)
    assert np.array_equal(got, hz.build_seek_file(dst))


# ---- archive_seek ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_chunk", ["65536", None])   # 65536: the 1 MiB file stays resident (one pack); default: chunked
@pytest.mark.parametrize("name", NAMES)
def test_archive_seek(hz, tmp_path, monkeypatch, inputs, name, env_chunk):
    _, data, blob, want = inputs[name]
    src = str(tmp_path / name)
    with open(src, "wb") as f:
        f.write(data)
    if env_chunk is None:
        monkeypatch.delenv("HZ_ARCHIVE_CHUNK", raising=False)
    else:
        monkeypatch.setenv("HZ_ARCHIVE_CHUNK", env_chunk)
    out, got = hz.archive_seek(src, verbose=False)
    assert out == src + ".compressed" and sorted(os.listdir(tmp_path)) == sorted([name, name + ".compressed"])
    with open(out, "rb") as f:
        assert f.read() == blob
    _same_table(got, want, len(data))
    assert np.array_equal(got, hz.build_seek_file(out))


# ---- encode_seek -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_encode_seek(hz, inputs, name):
    _, data, blob, want = inputs[name]
    got_blob, got = hz.encode_seek(data)
    assert got_blob == hz.encode(data) == blob
    _same_table(got, want, len(data))


# ---- reading back from the writer's table --------------------------------------------------------------------
def test_read_back(hz, tmp_path, inputs):
    src, data, _, _ = inputs["zipf.bin"]
    n = len(data)
    assert n % 2 == 1
    dst = str(tmp_path / "zipf.compressed")
    seek = hz.archive_stream_seek(src, dst, chunk_bytes=4096)
    for off, cnt in ((4097, 301),              # an odd offset
                     (4096 - 10, 20),          # across the first chunk boundary of the 4096-byte-chunk run
                     (7 * 4096 - 1, 4098),     # a whole chunk and a byte of each neighbour
                     (n - 3, 3)):              # the last 3 bytes: the odd one comes from the header
        assert hz.decode_range_file(dst, seek, off, cnt) == data[off:off + cnt], (off, cnt)


# ---- a table too small -----------------------------------------------------------------------------------
def test_capacity(hz, tmp_path, inputs):
    _, data, _, want = inputs["zipf.bin"]
    src = str(tmp_path / "zipf.bin")
    with open(src, "wb") as f:
        f.write(data)
    lib = hz.load()
    tab = np.zeros(want.size, dtype=np.uint64)
    short = 8 * want.size - 8
    p = tab.ctypes.data_as(ctypes.c_void_p)
    nsym = ctypes.c_uint64()
    dst = str(tmp_path / "never.compressed")
    assert lib.hz_archive_stream_seek(os.fsencode(src), os.fsencode(dst), 65536, 0, p, short, ctypes.byref(nsym)) == HZ_ECAP
    assert nsym.value == len(data) // 2
    nsym = ctypes.c_uint64()
    assert lib.hz_archive_file_seek(os.fsencode(src), 0, p, short, ctypes.byref(nsym)) == HZ_ECAP
    assert nsym.value == len(data) // 2
    assert os.listdir(tmp_path) == ["zipf.bin"]      # no output file appeared
    assert not tab.any()
    arr = np.frombuffer(data, dtype=np.uint8)
    out = np.zeros(len(data) + 1024, dtype=np.uint8)
    got = ctypes.c_uint64()
    assert lib.hz_encode_host_seek(arr.ctypes.data_as(ctypes.c_void_p), arr.size, out.ctypes.data_as(ctypes.c_void_p),
                                   out.size, ctypes.byref(got), p, short) == HZ_ECAP
    assert not tab.any() and not out.any()
    # an empty table needs no buffer
    empty = str(tmp_path / "empty.bin")
    open(empty, "wb").close()
    nsym = ctypes.c_uint64(99)
    assert lib.hz_archive_stream_seek(os.fsencode(empty), os.fsencode(dst), 65536, 0, None, 0, ctypes.byref(nsym)) == 0
    assert nsym.value == 0 and os.path.getsize(dst) > 0
