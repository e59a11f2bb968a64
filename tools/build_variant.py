"""Build an A/B variant of libhuffman_amd.so with extra -D flags into huffman_amd/<dir>/ (load it with
HZ_LIB_VARIANT=<dir>). Development tool: the product build is huffman_amd/build.py.
usage: python tools/build_variant.py DIR -DNAME=VALUE ..."""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from huffman_amd import build as b  # noqa: E402

out_dir = os.path.join(b.PKG, sys.argv[1])
with tempfile.TemporaryDirectory() as td:
    b.compile_library(b.CSRC, b.INCLUDE, td, os.path.join(out_dir, "libhuffman_amd.so"), sys.argv[2:], force=True)
print(out_dir)
