"""The build's file lists are derived from the source directory, its job count is bounded, and every
header compiles on its own."""
import concurrent.futures
import os
import shutil
import subprocess

import pytest

from huffman_amd import build


def test_every_source_is_listed():
    """The lists come from the directory, so this fails only for a source named outside the build's
    hz_* pattern (which would be left out of the library and of BUILD_ID without a word)."""
    listed = set(os.path.join(build.CSRC, f) for f in build.LIB_SOURCES) | set(build.HEADERS)
    for f in os.listdir(build.CSRC):
        if f.endswith((".h", ".hip", ".cpp")) and not f.startswith("cli_"):
            assert os.path.join(build.CSRC, f) in listed, f
    assert os.path.join(build.INCLUDE, "huffman_amd.h") in listed


def test_source_id_follows_a_header(tmp_path):
    src, inc = tmp_path / "csrc", tmp_path / "include"
    shutil.copytree(build.CSRC, src)
    shutil.copytree(build.INCLUDE, inc)
    before = build.source_id(str(src), str(inc))
    assert before == build.source_id()
    with open(src / "hz_internal.h", "ab") as f:
        f.write(b"\n")
    assert build.source_id(str(src), str(inc)) != before
    assert build.source_id() == before  # the tree itself is untouched


@pytest.mark.skipif(not os.path.exists(build.HIPCC), reason="no hipcc")
def test_every_header_compiles_alone(tmp_path):
    """A unit that holds nothing but the header compiles for the device with the build's flags, so no
    header depends on what its includer happened to include first."""
    names = sorted(f for f in os.listdir(build.CSRC) if f.endswith(".h"))
    assert names

    def check(name):
        tu = tmp_path / (name + ".hip")
        tu.write_text(f'#include "{name}"\n')
        cmd = [build.HIPCC] + build.CFLAGS + [f"-I{build.INCLUDE}", f"-I{build.CSRC}", "-x", "hip",
                                              "--cuda-device-only", "-fsyntax-only", str(tu)]
        return name, subprocess.run(cmd, capture_output=True, text=True)

    with concurrent.futures.ThreadPoolExecutor(build.build_jobs(len(names))) as pool:
        for name, r in pool.map(check, names):
            assert r.returncode == 0, f"{name}:\n{r.stderr}"


def test_job_count_is_bounded(monkeypatch):
    units = len(build.LIB_SOURCES)
    for var in ("MAX_JOBS", "CMAKE_BUILD_PARALLEL_LEVEL"):
        monkeypatch.delenv(var, raising=False)
    assert 1 <= build.build_jobs(units) <= min(16, units)
    assert build.build_jobs(1000) <= 16
    monkeypatch.setenv("MAX_JOBS", "2")
    assert build.build_jobs(1000) == 2
    monkeypatch.setenv("MAX_JOBS", "64")
    assert build.build_jobs(1000) <= 16
    monkeypatch.delenv("MAX_JOBS")
    monkeypatch.setenv("CMAKE_BUILD_PARALLEL_LEVEL", "3")
    assert build.build_jobs(1000) == 3
