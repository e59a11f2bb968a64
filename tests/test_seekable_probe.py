"""hz_seekable.cpp under the address and undefined-behaviour sanitizers: tests/seekable_probe.cpp, a
stand-alone host program with its own main, built here from hz_seekable.cpp and hz_file_io.cpp (host code
only: every sanitizer flag goes to the host compilation through -Xarch_host, as tests/test_stream_host.py
builds its probe) and run as a plain child process. Trailers are written into buffers of exactly their
size and loaded into arrays of exactly theirs, so a byte too many is a report; the footers it feeds the
parser carry a right check over offsets past the file and sizes that would wrap."""
import os
import subprocess

import pytest

from huffman_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
HZ_EINVAL, HZ_EFORMAT, HZ_ENOENT = -1, -5, -10


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(build.HIPCC):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "huffman_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("seekable_probe") / "seekable_probe")
    cmd = [build.HIPCC, "-O1", "-g", "-std=c++17"] + SANITIZE + [
        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "seekable_probe.cpp"),
        os.path.join(csrc, "hz_seekable.cpp"), os.path.join(csrc, "hz_file_io.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_probe(probe, tmp_path):
    r = subprocess.run([probe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.split("\n")[:-1] == [
        # shorter than a footer: plain (present 0), and nothing to load from a plain file
        "short 0 0 0 %d" % HZ_EFORMAT,
        "short 1 0 0 %d" % HZ_EFORMAT,
        "short 63 0 0 %d" % HZ_EFORMAT,
        # exactly 64 bytes: the footer alone is a whole trailer (n = 0); 64 bytes of anything else are plain
        "footer-only 0 64",
        "junk64 0 0",
        "roundtrip ok",
        # seven footers that lie, each HZ_EFORMAT; the honest one is present
        "lying " + " ".join([str(HZ_EFORMAT)] * 7) + " 1",
        "missing %d %d" % (HZ_ENOENT, HZ_ENOENT),
        "null %d %d %d" % (HZ_EINVAL, HZ_EINVAL, HZ_EINVAL),
    ]
