"""Timing of the seekable trailer's two costs (DESIGN.md section 5b "Seekable files", section 6 (j)):

  sums   hz_block_sums beside hz_hist16 on one resident Zipf(1.1) buffer (default 16 GiB, hz_generate), the
         two alternating in one loop of one process, each warmed up, each between two device events on the
         codec's stream. Both read the input once, so the histogram's time is the yardstick. The sums of
         the first 64 MiB are compared with zlib on the host.
  file   on a Zipf file (default 2 GiB) written to --dir: hz_archive_stream_seekable with sums beside
         hz_archive_stream_seek, wall clock and hz_stream_last_timing's split, alternating. With
         --parent-lib (an A/B build of the parent commit, huffman_amd/build.py) that library's
         hz_archive_stream_seek runs in the same loop, from a second handle with its own context. The
         seekable file's image is compared with the plain output and its table with the returned one.

--only sums / --only file runs one figure. Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes
import json
import os
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import huffman_amd  # noqa: E402
from huffman_amd import _lib  # noqa: E402
from huffman_amd.pipeline import StreamCodec  # noqa: E402


def stats(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 4), "median": round(float(np.median(xs)), 4), "max": round(xs[-1], 4),
            "spread": round(xs[-1] - xs[0], 4)}


def sums_figure(c, n, reps):
    x = torch.empty(n, dtype=torch.uint8, device="cuda")
    c.dev.generate(x.data_ptr(), n, offset=0, kind=1, alpha=1.1, seed=42)
    sums = torch.empty(huffman_amd.block_sums_bytes(n) // 4, dtype=torch.int32, device="cuda")
    forms = [("hist16", lambda: c.dev.hist16(x.data_ptr(), n, c.hist.data_ptr())),
             ("block_sums", lambda: c.dev.block_sums(x.data_ptr(), n, sums.data_ptr()))]
    for _, fn in forms:                                  # warm-up: code objects, kernel attributes
        fn()
        c.sync()
    ms = {name: [] for name, _ in forms}
    for _ in range(reps):                                # alternating
        for name, fn in forms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            c.sync()
            a.record(c.stream)
            fn()
            b.record(c.stream)
            c.sync()
            ms[name].append(a.elapsed_time(b))           # hist16's includes the memset of its 512 KiB of bins
    k = min(n, 64 << 20)
    host = x[:k].cpu().numpy().tobytes()
    want = np.array([zlib.adler32(host[o:o + 4096].ljust(4096, b"\0")) for o in range(0, k, 4096)], dtype=np.uint32)
    ok = bool(np.array_equal(sums[:want.size].cpu().numpy().view(np.uint32), want))
    res = {"bytes": n, "first_64MiB_equal_zlib": ok}
    for name, _ in forms:
        res[name + "_ms"] = stats(ms[name])
        res[name + "_GBps"] = round(n / (float(np.median(ms[name])) * 1e-3) / 1e9, 1)
    res["block_sums_over_hist16_median"] = round(float(np.median(ms["block_sums"]) / np.median(ms["hist16"])), 4)
    return res


def _stream_seek(lib, src, dst, chunk, n):
    words = max(lib.hz_seek_bytes(n // 2) // 8, 1)
    seek = np.zeros(words, dtype=np.uint64)
    nsym = ctypes.c_uint64()
    rc = lib.hz_archive_stream_seek(os.fsencode(src), os.fsencode(dst), chunk, 0, seek.ctypes.data_as(ctypes.c_void_p),
                                    8 * words, ctypes.byref(nsym))
    assert rc == 0, rc
    t = _lib.StreamTiming()
    lib.hz_stream_last_timing(ctypes.byref(t))
    return seek, t.as_dict()


def file_figure(c, n, reps, where, chunk, parent_lib):
    src = os.path.join(where, "seekable_timing.bin")
    outs = {k: os.path.join(where, "seekable_timing.%s.compressed" % k) for k in ("seekable", "seek", "parent")}
    x = torch.empty(n, dtype=torch.uint8, device="cuda")
    c.dev.generate(x.data_ptr(), n, offset=0, kind=1, alpha=1.1, seed=43)
    c.sync()
    x.cpu().numpy().tofile(src)
    del x
    torch.cuda.empty_cache()
    lib = huffman_amd.load()
    parent = None
    if parent_lib:
        parent = ctypes.CDLL(parent_lib)
        for name, res, args in _lib.PROTOTYPES:
            if hasattr(parent, name):
                getattr(parent, name).restype, getattr(parent, name).argtypes = res, args

    def seekable():
        huffman_amd.archive_seekable(src, outs["seekable"], chunk_bytes=chunk, sums=True)
        return huffman_amd.stream_timing()

    forms = [("archive_seekable_sums", seekable), ("archive_stream_seek", lambda: _stream_seek(lib, src, outs["seek"], chunk, n)[1])]
    if parent is not None:
        forms.append(("parent_archive_stream_seek", lambda: _stream_seek(parent, src, outs["parent"], chunk, n)[1]))
    wall = {name: [] for name, _ in forms}
    split = {}
    try:
        for _, fn in forms:                              # warm-up: the contexts, the page cache
            fn()
        for _ in range(reps):                            # alternating
            for name, fn in forms:
                t0 = time.perf_counter()
                split[name] = fn()
                wall[name].append((time.perf_counter() - t0) * 1e3)
        table, _ = _stream_seek(lib, src, outs["seek"], chunk, n)
        info = huffman_amd.seekable_info(outs["seekable"])
        with open(outs["seek"], "rb") as f:
            plain = f.read()
        with open(outs["seekable"], "rb") as f:
            image_equal = f.read(info["image_bytes"]) == plain
        table_equal = bool(np.array_equal(huffman_amd.load_seek(outs["seekable"]), table[:info["nblocks"] + 1]))
        sizes = {"image_bytes": info["image_bytes"], "file_bytes": info["file_bytes"]}
    finally:
        for p in [src] + list(outs.values()):
            if os.path.exists(p):
                os.remove(p)
    res = {"bytes": n, "dir": where, "chunk_bytes": chunk, "image_equal": image_equal, "table_equal": table_equal, **sizes}
    for name, _ in forms:
        res[name + "_wall_ms"] = stats(wall[name])
        res[name + "_last_split"] = {k: round(v, 3) if isinstance(v, float) else v for k, v in split[name].items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--gib", type=int, default=16)
    ap.add_argument("--file-gib", type=int, default=2)
    ap.add_argument("--file-reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=256 << 20)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else ".")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--only", default="", choices=["", "sums", "file"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    c = StreamCodec(0)
    res = {"tool": "seekable_timing", "build_id": _lib.build_id(), "reps": a.reps, "file_reps": a.file_reps,
           "note": "sums: ms between device events, forms alternating; file: wall-clock ms and hz_stream_last_timing"}
    if a.only != "file":
        res["sums"] = sums_figure(c, a.gib << 30, a.reps)
        torch.cuda.empty_cache()
    if a.only != "sums":
        res["file"] = file_figure(c, a.file_gib << 30, a.file_reps, a.dir, a.chunk, a.parent_lib)
    s = json.dumps(res)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
