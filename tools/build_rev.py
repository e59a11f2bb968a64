"""Build libhuffman_amd.so from the sources of a git revision into huffman_amd/<dir>/ (an A/B baseline,
loaded with HZ_LIB_VARIANT=<dir>). Development tool; the product build is huffman_amd/build.py.
The file list is the revision's own (its huffman_amd/csrc), so a revision with another source layout builds.
usage: python tools/build_rev.py REV DIR [-DFLAG ...]"""
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from huffman_amd import build as b  # noqa: E402


def git(*args):
    return subprocess.run(["git"] + list(args), check=True, capture_output=True, cwd=b.ROOT).stdout


rev, name, flags = sys.argv[1], sys.argv[2], sys.argv[3:]
out_dir = os.path.join(b.PKG, name)
with tempfile.TemporaryDirectory() as td:
    src = os.path.join(td, "csrc")
    inc = os.path.join(td, "include")
    os.makedirs(src)
    os.makedirs(inc)
    for f in git("ls-tree", "--name-only", f"{rev}:huffman_amd/csrc").decode().split():
        with open(os.path.join(src, f), "wb") as fh:
            fh.write(git("show", f"{rev}:huffman_amd/csrc/{f}"))
    with open(os.path.join(inc, "huffman_amd.h"), "wb") as fh:
        fh.write(git("show", f"{rev}:include/huffman_amd.h"))
    b.compile_library(src, inc, os.path.join(td, "obj"), os.path.join(out_dir, "libhuffman_amd.so"), flags, force=True)
print(out_dir)
