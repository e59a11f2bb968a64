"""Timing of the two whole-block flows (DESIGN.md section 5b "Seekable files", section 6 (k)) on one Zipf(1.1)
file (default 2 GiB, hz_generate) written to --dir and archived once plain and once seekable with sums:

  attach   make_seekable with and without sums on the plain file (cut back to its image after every run),
           beside build_seek_file of the same file: the same windowed index-less walk, which the attach
           without sums repeats and the attach with sums adds a decode and hz_block_sums to.
  verify   extract_verified(out_path=None) beside verify_seekable on the seekable file: the windowed
           index-less decode with hz_block_sums_check beside the batch decoder in 64 MiB tiles.

All forms alternate in one loop of one process after one warm-up run each: wall-clock ms, and
hz_stream_last_timing's split of the streamed ones. With --parent-lib (an A/B build of the parent commit,
huffman_amd/build.py) that library's hz_extract_stream_seek and hz_seekable_verify_file run in the same loop,
from a second handle with its own context. The attached files are compared with archive_seekable's.
Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import huffman_amd  # noqa: E402
from huffman_amd import _lib  # noqa: E402
from huffman_amd.pipeline import StreamCodec  # noqa: E402


def stats(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 2), "median": round(float(np.median(xs)), 2), "max": round(xs[-1], 2)}


def _read(path, off=0):
    with open(path, "rb") as f:
        f.seek(off)
        return f.read()


def _parent(path):
    lib = ctypes.CDLL(path)
    for name, res, args in _lib.PROTOTYPES:
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def _walk(lib, path, window, nsym):
    """hz_extract_stream_seek without an out_path (build_seek_file), through `lib`."""
    seek = np.zeros(max(lib.hz_seek_bytes(nsym) // 8, 1), dtype=np.uint64)
    got = ctypes.c_uint64()
    rc = lib.hz_extract_stream_seek(os.fsencode(path), None, window, 0, seek.ctypes.data_as(ctypes.c_void_p), 8 * seek.size,
                                    ctypes.byref(got))
    assert rc == 0 and got.value == nsym, rc
    return seek


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--file-gib", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window", type=int, default=256 << 20)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else ".")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = a.file_gib << 30
    c = StreamCodec(0)
    src = os.path.join(a.dir, "attach_timing.bin")
    plain, seekable, nosums = (os.path.join(a.dir, "attach_timing.%s.compressed" % k) for k in ("plain", "seekable", "nosums"))
    lib = huffman_amd.load()
    parent = _parent(a.parent_lib) if a.parent_lib else None
    try:
        x = torch.empty(n, dtype=torch.uint8, device="cuda")
        c.dev.generate(x.data_ptr(), n, offset=0, kind=1, alpha=1.1, seed=44)
        c.sync()
        x.cpu().numpy().tofile(src)
        del x
        torch.cuda.empty_cache()
        huffman_amd.archive_stream(src, plain)
        huffman_amd.archive_seekable(src, seekable, sums=True)
        huffman_amd.archive_seekable(src, nosums, sums=False)
        image_bytes = os.path.getsize(plain)
        want = {True: _read(seekable, image_bytes), False: _read(nosums, image_bytes)}
        os.remove(nosums)
        equal = {}

        def attach(sums):
            def run():
                assert huffman_amd.make_seekable(plain, sums=sums, window_bytes=a.window) is True
                return huffman_amd.stream_timing()

            def after():
                equal[sums] = equal.get(sums, True) and _read(plain, image_bytes) == want[sums]
                os.truncate(plain, image_bytes)
            return run, after

        def walk(which):
            def run():
                _walk(which, plain, a.window, n // 2)
                t = _lib.StreamTiming()
                which.hz_stream_last_timing(ctypes.byref(t))
                return t.as_dict()
            return run, None

        def verified():
            huffman_amd.extract_verified(seekable, window_bytes=a.window)
            return huffman_amd.stream_timing()

        def verify(which):
            def run():
                assert which.hz_seekable_verify_file(os.fsencode(seekable), None) == 0
                return None
            return run, None

        forms = [("make_seekable_sums",) + attach(True), ("make_seekable_table_only",) + attach(False),
                 ("build_seek_file",) + walk(lib), ("extract_verified_check_only", verified, None),
                 ("verify_seekable",) + verify(lib)]
        if parent is not None:
            forms += [("parent_build_seek_file",) + walk(parent), ("parent_verify_seekable",) + verify(parent)]
        wall = {name: [] for name, _, _ in forms}
        split = {}
        for rep in range(a.reps + 1):                          # the first run of each form is its warm-up
            for name, run, after in forms:                     # alternating
                t0 = time.perf_counter()
                s = run()
                ms = (time.perf_counter() - t0) * 1e3
                if after:
                    after()
                if rep:
                    wall[name].append(ms)
                    split[name] = s
    finally:
        for p in (src, plain, seekable, nosums):
            if os.path.exists(p):
                os.remove(p)
    res = {"tool": "attach_timing", "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(0), "bytes": n, "image_bytes": image_bytes, "dir": a.dir,
           "window_bytes": a.window, "reps": a.reps, "parent_lib": bool(parent),
           "attached_equals_archive_seekable": {"sums": equal[True], "table_only": equal[False]},
           "note": "wall-clock ms, forms alternating after one warm-up each; split: hz_stream_last_timing of the last run"}
    for name, _, _ in forms:
        res[name + "_wall_ms"] = stats(wall[name])
        res[name + "_GBps_of_original"] = round(n / (float(np.median(wall[name])) * 1e-3) / 1e9, 2)
        if split.get(name):
            res[name + "_last_split"] = {k: round(v, 3) if isinstance(v, float) else v for k, v in split[name].items()}
    s = json.dumps(res)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
