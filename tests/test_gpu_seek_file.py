"""The file-level forms of random access: huffman_amd.build_seek_file (hz_extract_stream_seek: the seek
table as a by-product of the windowed extract, with and without an output file) and
huffman_amd.decode_range_file (hz_decode_range_file: a range read from the file on disk), on the
reference-written goldens and on a Zipf file archived here. Every comparison is exact.

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
HZ_EFORMAT = -5
WINDOWS = [4096, 65536, None]   # None: the default (256 MiB)
BASELINES = sorted(glob.glob(os.path.join(GOLD, "*.baseline.compressed")))


@pytest.fixture(scope="module")
def hz(built_lib):
    import huffman_amd
    return huffman_amd


@pytest.fixture(scope="module")
def zipf_file(hz, tmp_path_factory):
    """A 1 MiB + 3 byte Zipf file (an odd size: the last byte travels in the header), archived once: the
    original's bytes, the .compressed path, its image and its table from the whole-buffer form."""
    import oracle_lib
    d = tmp_path_factory.mktemp("seekfile")
    data = oracle_lib.generate((1 << 20) + 3, offset=0, kind=1, seed=31).tobytes()
    src, dst = str(d / "zipf.bin"), str(d / "zipf.bin.compressed")
    with open(src, "wb") as f:
        f.write(data)
    hz.archive_stream(src, dst, chunk_bytes=1 << 20)
    with open(dst, "rb") as f:
        blob = f.read()
    return data, dst, blob, hz.build_seek(blob)


def _build(hz, path, window, out_path=None):
    return hz.build_seek_file(path, out_path=out_path) if window is None else \
        hz.build_seek_file(path, window_bytes=window, out_path=out_path)


# ---- 9. build_seek_file -------------------------------------------------------------------------------
def test_goldens_are_there():
    assert len(BASELINES) >= 4


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("path", BASELINES, ids=os.path.basename)
def test_build_seek_file_goldens(hz, tmp_path, path, window):
    """Files the reference wrote, through windows of 4096 and 65 536 bytes (many rounds, entries placed by
    sym_base / bit_base) and the default: the table equals build_seek(blob); with out_path the output is
    the original, without it no file appears."""
    with open(path, "rb") as f:
        blob = f.read()
    with open(path[:-len(".baseline.compressed")], "rb") as f:
        data = f.read()
    want = hz.build_seek(blob)
    before = sorted(os.listdir(os.getcwd()))
    got = _build(hz, path, window)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    assert sorted(os.listdir(os.getcwd())) == before and os.listdir(tmp_path) == []
    out = str(tmp_path / "out.bin")
    got = _build(hz, path, window, out_path=out)
    assert np.array_equal(got, want)
    with open(out, "rb") as f:
        assert f.read() == data


@pytest.mark.parametrize("window", WINDOWS)
def test_build_seek_file_zipf(hz, tmp_path, zipf_file, window):
    data, path, blob, want = zipf_file
    assert want.size == ((len(data) // 2 + BLK - 1) // BLK) + 1
    assert np.array_equal(_build(hz, path, window), want)
    assert os.listdir(tmp_path) == []
    out = str(tmp_path / "out.bin")
    assert np.array_equal(_build(hz, path, window, out_path=out), want)
    with open(out, "rb") as f:
        assert f.read() == data


# ---- 10. decode_range_file ---------------------------------------------------------------------------
def _ranges(n):
    return [(1, 1), (0, 7), (3, 4098), (4095, 3 * 4096 + 3), (n - 1, 1), (n - 5, 5), (n - 4097, 4097), (17, 0), (n, 0),
            (0, n)]


def test_decode_range_file(hz, zipf_file):
    """Odd offsets, odd lengths, the last byte of an odd-sized original (from the header), length 0, one
    range crossing three blocks, the whole file; past the end raises."""
    data, path, blob, seek = zipf_file
    n = len(data)
    assert n % 2 == 1
    for off, cnt in _ranges(n):
        assert hz.decode_range_file(path, seek, off, cnt) == data[off:off + cnt], (off, cnt)
    b0, b1 = 4095 // 4096, (4095 + 3 * 4096 + 3 - 1) // 4096
    assert b1 - b0 + 1 >= 3
    for off, cnt in [(n, 1), (n - 1, 2), (n + 1, 0)]:
        with pytest.raises(hz.HZError) as e:
            hz.decode_range_file(path, seek, off, cnt)
        assert e.value.status == -1


def test_decode_range_file_reads_only_the_span(hz, tmp_path, zipf_file):
    """Every payload byte outside hz_seek_span's bytes of the range overwritten with 0xFF in a copy of the
    file: the range still decodes right, so nothing else of the payload is read."""
    data, path, blob, seek = zipf_file
    _, info = hz.parse_header(blob)
    nsym = info.n // 2
    off, cnt = 5 * 4096 + 1, 3 * 4096 + 2       # blocks 5 .. 8
    s0, s1 = off // 2, (off + cnt + 1) // 2
    bb, be = hz.seek_span(seek, nsym, s0, s1 - s0)
    pay = len(blob) - info.payload_byte
    be = min(be, pay)
    assert 0 < bb < be < pay
    raw = bytearray(blob)
    raw[info.payload_byte:info.payload_byte + bb] = b"\xff" * bb
    raw[info.payload_byte + be:] = b"\xff" * (pay - be)
    assert bytes(raw) != blob
    scr = str(tmp_path / "scribbled.compressed")
    with open(scr, "wb") as f:
        f.write(raw)
    assert hz.decode_range_file(scr, seek, off, cnt) == data[off:off + cnt]


# ---- 11. a truncated file ----------------------------------------------------------------------------
@pytest.mark.parametrize("with_out", [False, True])
def test_truncated_file_is_eformat(hz, tmp_path, zipf_file, with_out):
    data, path, blob, seek = zipf_file
    _, info = hz.parse_header(blob)
    cut = str(tmp_path / "cut.compressed")
    with open(cut, "wb") as f:
        f.write(blob[:info.payload_byte + (len(blob) - info.payload_byte) // 2])
    lib = hz.load()
    tab = np.zeros(seek.size, dtype=np.uint64)
    nsym = ctypes.c_uint64()
    out = os.fsencode(str(tmp_path / "cut.out")) if with_out else None
    rc = lib.hz_extract_stream_seek(os.fsencode(cut), out, 65536, 0, tab.ctypes.data_as(ctypes.c_void_p), tab.size * 8,
                                    ctypes.byref(nsym))
    assert rc == HZ_EFORMAT and nsym.value == len(data) // 2
    with pytest.raises(hz.HZError) as e:
        hz.build_seek_file(cut, window_bytes=65536)
    assert e.value.status == HZ_EFORMAT
