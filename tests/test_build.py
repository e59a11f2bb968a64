"""The build's file lists are derived from the source directory, and its job count is bounded."""
import os
import shutil

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
