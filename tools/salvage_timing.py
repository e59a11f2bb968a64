"""Timing of salvage (DESIGN.md section 5b "Seekable files", section 6) on one Zipf(1.1) file (default 2 GiB,
hz_generate) written to --dir and archived seekable with sums, and on a copy of it with one flipped payload bit
in every 1024th block:

  salvage              undamaged, with an output file
  salvage_damaged      the damaged copy, with an output file (the list must be exactly the damaged blocks)
  salvage_scan         undamaged, out_path=None
  extract_verified     the undamaged file with an output file, and check only: the index-less walk beside the
                       table-driven batch decode, both with the sums checked on the device
  verify_seekable      the undamaged file: the batch decoder in 64 MiB tiles, sums compared on the host

All forms alternate in one loop of one process after one warm-up run each: wall-clock ms, and
hz_stream_last_timing's split of the streamed ones. Beside them the device time (events around ten calls) of
hz_block_sums_check and hz_block_sums_mark over one window's worth of output, 256 MiB, every block matching, and
of hz_block_sums_mark with HZ_SUMS_ZERO_BAD and every 1024th block failing.
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import shutil
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


def device_ms(c, fn, reps=10):
    fn()
    c.sync()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(c.stream)
    for _ in range(reps):
        fn()
    b.record(c.stream)
    c.sync()
    return round(a.elapsed_time(b) / reps, 4)


def kernel_times(c, nbytes):
    """hz_block_sums_check beside hz_block_sums_mark on nbytes of Zipf bytes, device ms per call."""
    x = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    c.dev.generate(x.data_ptr(), nbytes, offset=0, kind=1, alpha=1.1, seed=45)
    sums = c.block_sums(x)
    nb = sums.numel()
    bad = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    bits = torch.zeros((nb + 31) // 32, dtype=torch.int32, device="cuda")
    wrong = sums.clone()
    wrong[::1024] ^= 1
    out = {"bytes": nbytes,
           "k_block_sums_check": device_ms(c, lambda: c.block_sums_check(x, sums, bad)),
           "k_block_sums_mark": device_ms(c, lambda: c.block_sums_mark(x, sums, bits)),
           "k_block_sums_mark_zero_bad_all_match": device_ms(c, lambda: c.block_sums_mark(x, sums, bits, zero_bad=True))}
    assert int(bad.item()) == -1 and int(bits.abs().sum()) == 0
    out["k_block_sums_mark_zero_bad_every_1024th"] = device_ms(c, lambda: c.block_sums_mark(x, wrong, bits, zero_bad=True))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--file-gib", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=int, default=256 << 20)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else ".")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = a.file_gib << 30
    c = StreamCodec(0)
    src, seekable, damaged, out = (os.path.join(a.dir, "salvage_timing." + k) for k in ("bin", "compressed", "damaged", "out"))
    try:
        kernels = kernel_times(c, min(a.window, n))
        x = torch.empty(n, dtype=torch.uint8, device="cuda")
        c.dev.generate(x.data_ptr(), n, offset=0, kind=1, alpha=1.1, seed=44)
        c.sync()
        x.cpu().numpy().tofile(src)
        del x
        torch.cuda.empty_cache()
        huffman_amd.archive_seekable(src, seekable, sums=True)
        os.remove(src)
        shutil.copyfile(seekable, damaged)
        seek = huffman_amd.load_seek(seekable)
        nb = seek.size - 1
        with open(seekable, "rb") as f:
            payload_byte = huffman_amd.parse_header(f.read(1 << 20))[1].payload_byte
        hit = list(range(0, nb, 1024))
        with open(damaged, "r+b") as f:
            for b in hit:
                bit = (int(seek[b]) + int(seek[b + 1])) // 2
                f.seek(payload_byte + bit // 8)
                byte = f.read(1)[0]
                f.seek(payload_byte + bit // 8)
                f.write(bytes([byte ^ (0x80 >> (bit % 8))]))
        lists = {}

        def salvage(name, path, dst):
            def run():
                lists[name] = huffman_amd.salvage(path, dst, window_bytes=a.window)
                return huffman_amd.stream_timing()
            return name, run

        def verified(name, dst):
            def run():
                huffman_amd.extract_verified(seekable, dst, window_bytes=a.window)
                return huffman_amd.stream_timing()
            return name, run

        def verify():
            huffman_amd.verify_seekable(seekable)
            return None

        forms = [salvage("salvage", seekable, out), salvage("salvage_damaged", damaged, out), salvage("salvage_scan", seekable, None),
                 verified("extract_verified", out), verified("extract_verified_check_only", None), ("verify_seekable", verify)]
        wall = {name: [] for name, _ in forms}
        split = {}
        for rep in range(a.reps + 1):                          # the first run of each form is its warm-up
            for name, run in forms:                            # alternating
                t0 = time.perf_counter()
                s = run()
                ms = (time.perf_counter() - t0) * 1e3
                if rep:
                    wall[name].append(ms)
                    split[name] = s
    finally:
        for p in (src, seekable, damaged, out):
            if os.path.exists(p):
                os.remove(p)
    res = {"tool": "salvage_timing", "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(0), "bytes": n, "blocks": nb,
           "dir": a.dir, "window_bytes": a.window, "reps": a.reps, "damaged_blocks": len(hit),
           "lists_are_exact": lists["salvage"] == [] and lists["salvage_scan"] == [] and lists["salvage_damaged"] == hit,
           "sums_kernels_device_ms": kernels,
           "note": "wall-clock ms, forms alternating after one warm-up each; split: hz_stream_last_timing of the last run"}
    for name, _ in forms:
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
