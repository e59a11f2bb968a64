"""make_seekable (hz_seekable_attach_file) end to end on the GPU: an existing .compressed file gets, in place,
the trailer archive_seekable would have written. For a file this library's archive wrote the result is byte
for byte archive_seekable's of the same original; for any other valid file (the reference-written goldens, a
designed stream under a foreign codebook with 56-bit codes) it is the file's bytes plus the model's trailer
(tests/seekable_model.py: the table build_seek finds in the image, zlib's sums of the original). A second
call changes nothing, a trailer without sums is upgraded, and a file that is refused stays what it was.

Tolerance: none -- every check is bit-exact."""
import os
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import seekable_model as model  # noqa: E402
from test_gpu_seekable import GOLD, INPUTS, _data, _ranges  # noqa: E402

pytestmark = pytest.mark.gpu

HZ_EINVAL, HZ_EFORMAT, HZ_ENOENT = -1, -5, -10
WINDOWS = [16384, 65536, 1 << 30]
BASELINES = ["romeo.txt", "synth_zipf_4099.bin", "synth_unif_65536.bin", "synth_zipf_65537.bin"]
BLK = 2048


@pytest.fixture(scope="module")
def hz(built_lib):
    import huffman_amd
    return huffman_amd


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module", params=INPUTS)
def made(request, hz, tmp_path_factory):
    """An input archived once each way: the plain file and what archive_seekable writes with and without sums."""
    d = tmp_path_factory.mktemp("attach")
    data = _data(request.param)
    src, plain = str(d / "in.bin"), str(d / "plain.compressed")
    with open(src, "wb") as f:
        f.write(data)
    hz.archive_stream(src, plain, chunk_bytes=1 << 20)
    want = {}
    for sums in (False, True):
        out = str(d / ("seekable%d.compressed" % sums))
        hz.archive_seekable(src, out, chunk_bytes=65536, sums=sums)
        want[sums] = _read(out)
    return dict(data=data, plain=plain, pblob=_read(plain), want=want, dir=d)


def _model_result(hz, blob, data, sums):
    flags = model.SUMS if sums else 0
    return blob + model.trailer(len(blob), len(data), hz.build_seek(blob), model.block_sums(data) if sums else [], flags)


@pytest.mark.parametrize("sums", [False, True])
@pytest.mark.parametrize("window", WINDOWS)
def test_attach_equals_archive_seekable(hz, made, window, sums):
    path = str(made["dir"] / ("a-%d-%d.compressed" % (window, sums)))
    shutil.copyfile(made["plain"], path)
    assert hz.make_seekable(path, sums=sums, window_bytes=window) is True
    got = _read(path)
    assert got[:len(made["pblob"])] == made["pblob"]
    assert got == made["want"][sums] == _model_result(hz, made["pblob"], made["data"], sums)
    # a second call: nothing to attach, nothing written (and with sums present, none asked for is satisfied too)
    before = os.stat(path).st_mtime_ns
    assert hz.make_seekable(path, sums=sums, window_bytes=window) is False
    if sums:
        assert hz.make_seekable(path, sums=False, window_bytes=window) is False
    assert _read(path) == got and os.stat(path).st_mtime_ns == before


@pytest.mark.parametrize("window", [16384, 1 << 30])
def test_upgrade_a_trailer_without_sums(hz, made, window):
    path = str(made["dir"] / ("up-%d.compressed" % window))
    shutil.copyfile(made["plain"], path)
    assert hz.make_seekable(path, sums=False, window_bytes=window) is True
    assert _read(path) == made["want"][False]
    assert hz.make_seekable(path, sums=True, window_bytes=window) is True
    assert _read(path) == made["want"][True]
    assert len(made["want"][True]) >= len(made["want"][False])


@pytest.mark.parametrize("window", [16384, 256 << 20])
@pytest.mark.parametrize("name", BASELINES)
def test_reference_written_files(hz, tmp_path, name, window):
    import oracle_lib
    data = _read(os.path.join(GOLD, name))
    blob = _read(os.path.join(GOLD, name + ".baseline.compressed"))
    path = str(tmp_path / "ref.compressed")
    for sums in (False, True):
        with open(path, "wb") as f:
            f.write(blob)
        assert hz.make_seekable(path, sums=sums, window_bytes=window) is True
        got = _read(path)
        assert got == _model_result(hz, blob, data, sums)
    hz.verify_seekable(path)
    rg = _ranges(len(data))
    assert hz.read_seekable(path, rg, verify=True) == [data[o:o + c] for o, c in rg]
    assert oracle_lib.decode(got) == data          # the reference's reader never reads to the end of the file


@pytest.fixture(scope="module")
def designed(hz):
    """A file under the foreign codebook fib57 (tests/table_books.py: codes of 1 to 56 bits): four blocks of
    the 1-bit code, then three blocks and 777 symbols of the eight longest codes (50 to 56 bits), the first of
    those blocks 2048 x 56 bits; an odd original. The file's mean code length (about 24 bits) promises a
    16384-byte window two blocks of the long codes where it holds one (2340 codes of 56 bits): every such
    round overruns and is redone at one block. The header is the library's writer's, the payload the model's
    (tests/ref_stream.py)."""
    import ref_stream
    from table_books import book
    from test_gpu_designed_streams import _stream
    bk = book("fib57")
    rng = np.random.default_rng(57)
    sym = np.concatenate([_stream(bk, "shortest", 4 * BLK, rng), _stream(bk, "longest", 3 * BLK + 777, rng)])
    data = sym.astype("<u2").tobytes() + b"\x5a"
    head, pbits, pend = hz.write_header(bk.cb, len(data), data[-1])
    m = ref_stream.model(sym, bk.ln, bk.code, pbits, pend >> (8 - pbits) if pbits else 0)
    lens = bk.ln[sym].astype(np.int64)
    assert int(lens[:4 * BLK].max()) == 1 and int(lens[4 * BLK:5 * BLK].min()) == 56 and int(lens[5 * BLK:].min()) >= 50
    assert 2 * BLK * 50 > 8 * 16384 > BLK * 56             # one block of the long codes fits the window, two do not
    mean = (m.end_bit - pbits) / sym.size
    assert 8 * 16384 / (mean * 1.03) >= 2 * BLK            # and the plan's estimate asks for two and more
    blob = head + m.payload[:(m.end_bit + 7) // 8].tobytes()
    return dict(data=data, blob=blob, start=m.start, sym=sym)


@pytest.mark.parametrize("sums", [False, True])
def test_designed_56_bit_stream_at_the_smallest_window(hz, tmp_path, designed, sums):
    import oracle_lib
    data, blob = designed["data"], designed["blob"]
    assert oracle_lib.decode(blob) == data
    assert np.array_equal(hz.build_seek(blob), designed["start"])
    path = str(tmp_path / "designed.compressed")
    with open(path, "wb") as f:
        f.write(blob)
    assert hz.make_seekable(path, sums=sums, window_bytes=16384) is True
    got = _read(path)
    assert got == _model_result(hz, blob, data, sums)
    assert np.array_equal(hz.load_seek(path), designed["start"])
    if sums:
        hz.verify_seekable(path)
        assert hz.read_seekable(path, [(0, len(data))], verify=True) == [data]


def _refused(hz, path, status, **kw):
    before = _read(path) if os.path.exists(path) else None
    with pytest.raises(hz.HZError) as e:
        hz.make_seekable(path, **kw)
    assert e.value.status == status
    if before is not None:
        assert _read(path) == before
    return e.value


@pytest.mark.parametrize("sums", [False, True])
def test_refused_files_stay_what_they_were(hz, made, tmp_path, sums):
    pblob = made["pblob"]
    path = str(tmp_path / "cut.compressed")
    if len(made["data"]) >= 4096:
        # cut inside the header, and with a sixteenth of the payload left: fewer bits than its symbols need at
        # the shortest code (a cut that leaves more can decode, to other bytes: the format has no end mark)
        pay = hz.parse_header(pblob)[1].payload_byte
        for keep in (pay // 2, pay + (len(pblob) - pay) // 16):
            with open(path, "wb") as f:
                f.write(pblob[:keep])
            _refused(hz, path, HZ_EFORMAT, sums=sums, window_bytes=16384)
            _refused(hz, path, HZ_EFORMAT, sums=sums)
    with open(path, "wb") as f:
        f.write(pblob)
    for window in (0, 4096, 16383):           # below HZ_SEEKABLE_MIN_WINDOW
        _refused(hz, path, HZ_EINVAL, sums=sums, window_bytes=window)
    lib = hz.load()
    assert lib.hz_seekable_attach_file(os.fsencode(path), 65536, 2, None) == HZ_EINVAL      # an unknown flag
    assert lib.hz_seekable_attach_file(None, 65536, 0, None) == HZ_EINVAL
    assert _read(path) == pblob
    _refused(hz, str(tmp_path / "missing.compressed"), HZ_ENOENT, sums=sums)
    assert not os.path.exists(str(tmp_path / "missing.compressed"))
