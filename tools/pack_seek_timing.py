"""Timing of the seek table from the writer (DESIGN.md "The table from the writer"):

  pack   on a resident Zipf(1.1) stream (default 16 GiB, hz_generate), the range plan on, the pack forms
         alternating in one loop of one process, each warmed up: hz_pack_ranges without an index, with the
         full block index, and hz_pack_seek; hz_last_kernel_ms(HZ_STAGE_PACK) of every call. Every
         repeat's table is compared with the full index's start[] and every payload with the first one's.
         A library without hz_pack_seek (an A/B build of an older revision, HZ_LIB_VARIANT) runs the two
         forms it has, so the same tool measures the parent.
  file   on a Zipf file (default 2 GiB) written to --dir: archive_seek beside archive followed by
         build_seek_file, wall clock, alternating; the tables compared.

--only pack / --only file runs one figure. Prints one JSON line (and writes it to --out)."""
import argparse
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
    return {"min": round(xs[0], 4), "median": round(float(np.median(xs)), 4), "max": round(xs[-1], 4),
            "spread": round(xs[-1] - xs[0], 4)}


def pack_figure(c, n, reps):
    dev = c.dev
    x = torch.empty(n, dtype=torch.uint8, device="cuda")
    dev.generate(x.data_ptr(), n, offset=0, kind=1, alpha=1.1, seed=42)
    c.histogram(x)                                    # with the range plan: c.ranges
    h = c.hist.cpu().numpy().view(np.uint64)
    plan = c.make_plan(h, n)
    nsym = n // 2
    out, index = c.alloc_payload(plan, nsym)
    words = huffman_amd.seek_bytes(nsym) // 8
    seek = torch.empty(words, dtype=torch.int64, device="cuda")
    rp = c.ranges.data_ptr() if c.ranges is not None and dev.ranges_bytes(n) else None
    args = (x.data_ptr(), n, plan.start_bit, plan.lead, out.data_ptr(), out.numel())

    def no_index():
        dev.pack_ranges(*args, None, rp) if rp else dev.pack(*args, None)

    def full_index():
        dev.pack_ranges(*args, index.data_ptr(), rp) if rp else dev.pack(*args, index.data_ptr())

    def seek_table():
        dev.pack_seek(*args, seek.data_ptr(), rp)

    forms = [("no_index", no_index), ("full_index", full_index)]
    if hasattr(dev.lib, "hz_pack_seek"):
        forms.append(("seek_table", seek_table))
    nbytes = plan.words * 4
    for _, fn in forms:                               # warm-up: code objects, kernel attributes, the scratch
        fn()
        c.sync()
    first = out[:nbytes].clone()
    ms = {name: [] for name, _ in forms}
    plans, ok_pay, ok_tab = set(), True, True
    for _ in range(reps):                             # alternating
        for name, fn in forms:
            out[:nbytes].zero_()
            if name == "seek_table":
                seek.fill_(-1)
            c.sync()
            fn()
            c.sync()
            ms[name].append(dev.kernel_ms(_lib.STAGE_PACK))
            plans.add(dev.last_pack_ranges())
            ok_pay = ok_pay and bool(torch.equal(out[:nbytes], first))
            if name == "seek_table":
                ok_tab = ok_tab and bool(torch.equal(seek, index[:words]))
    res = {"bytes": n, "payload_bytes": (plan.start_bit + plan.payload_bits + 7) // 8, "range_plan_taken": sorted(plans),
           "every_payload_equal": ok_pay}
    for name, _ in forms:
        res[name + "_ms"] = stats(ms[name])
    if "seek_table" in ms:
        res["every_table_equals_full_index"] = ok_tab
        res["seek_minus_no_index_median_ms"] = round(float(np.median(ms["seek_table"]) - np.median(ms["no_index"])), 4)
        res["seek_minus_full_index_median_ms"] = round(float(np.median(ms["seek_table"]) - np.median(ms["full_index"])), 4)
    return res


def file_figure(c, n, reps, where):
    path = os.path.join(where, "pack_seek_timing.bin")
    x = torch.empty(n, dtype=torch.uint8, device="cuda")
    c.dev.generate(x.data_ptr(), n, offset=0, kind=1, alpha=1.1, seed=43)
    c.sync()
    x.cpu().numpy().tofile(path)
    del x
    torch.cuda.empty_cache()
    a, b1, b2, ok = [], [], [], True
    try:
        huffman_amd.archive_seek(path, verbose=False)  # warm-up: the process-wide context, the page cache
        for _ in range(reps):                          # alternating
            t0 = time.perf_counter()
            name, tab = huffman_amd.archive_seek(path, verbose=False)
            t1 = time.perf_counter()
            huffman_amd.archive(path, verbose=False)
            t2 = time.perf_counter()
            walked = huffman_amd.build_seek_file(name)
            t3 = time.perf_counter()
            a.append((t1 - t0) * 1e3)
            b1.append((t2 - t1) * 1e3)
            b2.append((t3 - t2) * 1e3)
            ok = ok and bool(np.array_equal(tab, walked))
    finally:
        for p in (path, path + ".compressed"):
            if os.path.exists(p):
                os.remove(p)
    return {"bytes": n, "dir": where, "archive_seek_ms": stats(a), "archive_ms": stats(b1), "build_seek_file_ms": stats(b2),
            "archive_then_build_seek_file_ms": stats([u + v for u, v in zip(b1, b2)]), "tables_equal": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--gib", type=int, default=16)
    ap.add_argument("--file-gib", type=int, default=2)
    ap.add_argument("--file-reps", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else ".")
    ap.add_argument("--only", default="", choices=["", "pack", "file"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    c = StreamCodec(0)
    res = {"tool": "pack_seek_timing", "build_id": _lib.build_id(), "lib": os.environ.get("HZ_LIB_VARIANT", "lib"),
           "reps": a.reps, "note": "pack: ms of hz_last_kernel_ms(HZ_STAGE_PACK), forms alternating; file: wall-clock ms"}
    if a.only != "file":
        res["pack"] = pack_figure(c, a.gib << 30, a.reps)
        torch.cuda.empty_cache()
    if a.only != "pack":
        res["file"] = file_figure(c, a.file_gib << 30, a.file_reps, a.dir)
    s = json.dumps(res)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
