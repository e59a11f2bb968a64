"""The host side of the streaming `archive` / `extract` that needs no GPU: the file reader and writer
(hz_file_io.cpp, the library's only multi-threaded host code) on real files, and the flows' window and
chunk arithmetic (hz_stream_plan.h), through tests/stream_probe.cpp: a stand-alone host program built here
twice, with AddressSanitizer and UndefinedBehaviorSanitizer and with ThreadSanitizer (host code only: every
sanitizer flag goes to the host compilation through -Xarch_host), and run as a plain child process.

Files hold fill(i) at byte i, restated here from the probe. The window's properties are checked from the
code lengths alone; the round and redo counts are those of the loop hz_extract_stream ran before its
arithmetic moved into ExtractWindow."""
import concurrent.futures
import os
import subprocess

import numpy as np
import pytest

from huffman_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HZ_EIO, HZ_ENOENT = -8, -10
MIB = 1 << 20
SANITIZERS = {
    "asan_ubsan": ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"],
    "tsan": ["-Xarch_host", "-fsanitize=thread"],
}
READ_SIZES = [0, 1, 4095, 16 * MIB - 1, 16 * MIB, 16 * MIB + 4097]  # both sides of the 8-thread threshold
WRITE_SIZES = [1, 8 * MIB - 1, 8 * MIB + 4097]                      # one thread, one thread, eight


def fill(off, n):
    i = np.arange(off, off + n, dtype=np.uint64)
    return ((i * np.uint64(2654435761)) >> np.uint64(13)).astype(np.uint8)


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    if not os.path.exists(build.HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("stream_probe")
    csrc = os.path.join(ROOT, "huffman_amd", "csrc")

    def compile_one(name):
        exe = str(out / ("stream_probe_" + name))
        cmd = [build.HIPCC, "-O1", "-g", "-std=c++17"] + SANITIZERS[name] + [
            "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "stream_probe.cpp"),
            os.path.join(csrc, "hz_file_io.cpp"), "-o", exe]
        return name, exe, subprocess.run(cmd, capture_output=True, text=True)

    exes = {}
    with concurrent.futures.ThreadPoolExecutor(2) as pool:
        for name, exe, r in pool.map(compile_one, SANITIZERS):
            assert r.returncode == 0, r.stderr
            exes[name] = exe
    return exes


@pytest.fixture(scope="module")
def read_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("stream_read")
    paths = []
    for n in READ_SIZES:
        p = d / ("f%d" % n)
        p.write_bytes(fill(0, n).tobytes())
        paths.append(str(p))
    return paths, str(d / "missing")


def run(exe, *args):
    """The probe's output lines; it must end with status 0 and nothing on stderr (no sanitizer report)."""
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    return r.stdout.split("\n")[:-1]


@pytest.mark.parametrize("san", sorted(SANITIZERS))
def test_reader(probes, read_files, san):
    paths, missing = read_files
    lines = run(probes[san], "reader", missing, *paths)
    assert len(lines) == len(READ_SIZES) + 1
    for n, line in zip(READ_SIZES, lines):
        asked = n + max(n - 1, 0) + max(n - 4097, 0)
        # whole, from 1 and from 4097 equal the fill; bytes_in is what was asked for; a read one byte past
        # the end is refused and adds nothing
        assert [int(v) for v in line.split()] == [n, 1, 1, 1, asked, HZ_EIO, asked], n
    assert lines[-1] == "missing %d" % HZ_ENOENT


@pytest.mark.parametrize("san", sorted(SANITIZERS))
def test_writer(probes, tmp_path, san):
    out = tmp_path / "written"
    lines = run(probes[san], "writer", str(out))
    total = sum(WRITE_SIZES)
    assert lines == ["0 0 0 0 %d" % total]
    assert os.path.getsize(out) == total        # reserved at twice that; close() cut it at the last written byte
    assert np.array_equal(np.fromfile(out, dtype=np.uint8), fill(0, total))


@pytest.mark.parametrize("san", sorted(SANITIZERS))
def test_writer_on_a_full_device(probes, san):
    if not os.path.exists("/dev/full"):
        pytest.skip("no /dev/full")
    lines = run(probes[san], "full", "/dev/full")
    assert lines == ["0 %d %d" % (HZ_EIO, HZ_EIO), "joined"]


# (name, code lengths, W, start bit, max_len, rounds, redone rounds)
def _window_cases():
    a, b = [16] * 20000, [1] * 20000
    return [
        ("16s-then-1s-bit5", a + b, 4096, 5, 16, 20, 9),
        ("16s-then-1s-bit0", a + b, 4096, 0, 16, 20, 0),
        ("1s-then-16s", b + a, 4096, 5, 16, 20, 9),
        ("16s", [16] * 10000, 4096, 3, 16, 6, 0),
        ("1s", [1] * 100000, 4096, 0, 1, 49, 0),
        ("56s", [56] * 3000, 4096, 7, 56, 6, 0),
        ("three", [3, 5, 7], 4096, 2, 7, 1, 0),
        ("random", [int(v) for v in np.random.default_rng(1).integers(1, 26, 200000)], 5008, 6, 25, 98, 0),
    ]


WINDOW_CASES = _window_cases()


@pytest.mark.parametrize("san", sorted(SANITIZERS))
@pytest.mark.parametrize("case", WINDOW_CASES, ids=[c[0] for c in WINDOW_CASES])
def test_extract_window(probes, tmp_path, san, case):
    _, lengths, W, start, max_len, rounds, redone = case
    inp = tmp_path / "window.bin"
    inp.write_bytes(np.array([W, start, max_len, len(lengths)] + lengths, dtype="<u8").tobytes())
    rows = [[int(v) for v in line.split()] for line in run(probes[san], "window", str(inp))]
    pos = [start]
    for ln in lengths:
        pos.append(pos[-1] + ln)
    nsym, pay = len(lengths), (pos[-1] + 7) // 8
    have, consumed, done = min(W, pay), 0, 0
    for k, used, tail, refill, red in rows:
        assert k >= 1 and done + k <= nsym
        bit = pos[done] - 8 * consumed          # the round's first codeword, in the window's first byte
        assert 0 <= bit < 8
        assert consumed + have <= pay
        if red:
            assert k == max((8 * have - bit) // max_len, 1)
        end = pos[done + k] - 8 * consumed      # its k codewords lie in the window
        assert end <= 8 * have and used == end // 8 and tail == have - used
        done += k
        if done < nsym:
            assert tail + refill <= W
            consumed += used
            have = tail + refill
        else:
            assert refill == 0
    assert done == nsym
    assert (len(rows), sum(r[4] for r in rows)) == (rounds, redone)


@pytest.mark.parametrize("san", sorted(SANITIZERS))
def test_archive_carry(probes, tmp_path, san):
    """Chunk end bits to payload bytes: nothing lost and nothing written twice between chunks."""
    rng = np.random.default_rng(7)
    for trial in range(40):
        start = int(rng.integers(0, 8))
        nchunks = int(rng.integers(1, 30))
        bits = [int(v) for v in rng.integers(1, 5000, nchunks)]
        if trial % 4 == 0:
            bits = [32 * int(v) for v in rng.integers(1, 100, nchunks)]  # chunks that end on a word
        inp = tmp_path / "carry.bin"
        inp.write_bytes(np.array([start, nchunks] + bits, dtype="<u8").tobytes())
        rows = [[int(v) for v in line.split()] for line in run(probes[san], "carry", str(inp))]
        assert len(rows) == nchunks
        sbit = start
        for i, (nbytes, next_sbit, needs_lead) in enumerate(rows):
            end = sbit + bits[i]
            last = i == nchunks - 1
            assert next_sbit == end % 32
            if not last:
                assert nbytes == end // 32 * 4      # whole words; the partial word is the next chunk's lead
            assert needs_lead == (1 if next_sbit and not last else 0)
            sbit = next_sbit
        assert sum(r[0] for r in rows) == (start + sum(bits) + 7) // 8
