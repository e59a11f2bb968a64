"""Timing of the gathered batch (DESIGN.md "Gathered pieces"), two figures, one JSON line:

  k  the kernel cost of the per-job view: 50 seeded ranges of 4 KiB on a resident Zipf(1.1) stream of
     --gib GiB, hz_decode_ranges over the whole payload beside hz_decode_ranges_pieces over the gathered
     buffer of hz_seek_pieces' plan (gathered on the device), HIP events on the codec's stream, both warmed
     up, the two sides alternating in one loop, every result compared with the input
  p  end to end by path: a Zipf(1.1) file of --file-gib GiB archived with its seek table, 64 seeded ranges
     of 4 KiB; wall time of decode_ranges_file, of 64 decode_range_file calls and of decode_ranges(blob)
     (the hull form, the file read into memory before the clock starts), alternating in one loop after a
     warm-up of each, and the bytes each form moves host-to-device (payload + seek words)

usage: python tools/pieces_timing.py [--gib 16] [--file-gib 2] [--reps 9] [--dir DIR] [--only k|p] [--out FILE]
"""
import argparse
import json
import os
import shutil
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import huffman_amd as hz  # noqa: E402
from huffman_amd import _lib  # noqa: E402
from huffman_amd.pipeline import StreamCodec  # noqa: E402

BLK = 2048


def stats(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 4), "median": round(float(np.median(xs)), 4), "max": round(xs[-1], 4)}


def timed(c, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(c.stream)
    fn()
    e1.record(c.stream)
    c.sync()
    return e0.elapsed_time(e1)


def kernel_figure(c, n, reps, k=50, nbytes=4 << 10):
    x = torch.empty(n, dtype=torch.uint8, device="cuda")
    c.dev.generate(x.data_ptr(), n, offset=0, kind=1, alpha=1.1, seed=42)
    plan, payload, index = c.encode(x)
    c.sync()
    nsym = n // 2
    seek = index[:(nsym + BLK - 1) // BLK + 1].clone()
    del index
    cnt = nbytes // 2
    begins = [int(v) for v in np.random.default_rng(2).integers(0, nsym - cnt + 1, k)]
    want = torch.cat([x[2 * b:2 * b + nbytes] for b in begins])
    rows = [(b, cnt, i * nbytes) for i, b in enumerate(begins)]
    pieces, prg, buf_bytes, seek_words = hz.seek_pieces(seek.cpu().numpy().view(np.uint64), nsym, payload.numel(), rows)
    buf = torch.zeros(buf_bytes, dtype=torch.uint8, device="cuda")
    words = torch.zeros(seek_words, dtype=torch.int64, device="cuda")
    for p in pieces:
        sb, nb, bb, fb, si, nblk = (int(v) for v in p)
        buf[bb:bb + nb] = payload[sb:sb + nb]
        words[si:si + nblk + 1] = seek[fb:fb + nblk + 1]
    to_dev = lambda a, cols: torch.from_numpy(a.view(np.uint64).reshape(-1, cols).view(np.int64).copy()).cuda()  # noqa: E731
    d_pieces, d_prg = to_dev(pieces, 6), to_dev(prg, 4)
    rg = torch.tensor(rows, dtype=torch.int64, device="cuda")
    out = torch.empty(k * nbytes + 16, dtype=torch.uint8, device="cuda")
    st_h, st_p = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")

    def hull():
        c.decode_ranges(payload, nsym, seek, rg, out, stats=st_h, full_index=False)

    def gathered():
        c.decode_ranges_pieces(buf, words, d_pieces, nsym, d_prg, out, stats=st_p)

    for fn in (hull, gathered):                # warm-up (also sizes the scratch)
        timed(c, fn)
    ta, tb, ok = [], [], True
    for rep in range(reps + 1):                # alternating; the first round is warm-up too: torch loads its fill
        for fn, ts in ((hull, ta), (gathered, tb)):   # and compare kernels in it, and the call after that paid 0.06 ms
            out.zero_()
            c.sync()
            t = timed(c, fn)
            if rep:
                ts.append(t)
            ok = ok and bool(torch.equal(out[:k * nbytes], want))
    return {"bytes": n, "payload_bytes": int(payload.numel()), "ranges": k, "range_bytes": nbytes, "pieces": int(len(pieces)),
            "buf_bytes": buf_bytes, "seek_words": seek_words, "decode_ranges_ms": stats(ta),
            "decode_ranges_pieces_ms": stats(tb), "all_equal_input": ok, "stats_hull": [int(v) for v in st_h.cpu()],
            "stats_pieces": [int(v) for v in st_p.cpu()],
            "median_difference_ms": round(float(np.median(tb)) - float(np.median(ta)), 4),
            "raw_ms_in_order": {"decode_ranges": [round(t, 4) for t in ta], "decode_ranges_pieces": [round(t, 4) for t in tb]}}


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def path_figure(n, reps, where, k=64, nbytes=4 << 10):
    c = StreamCodec(0)
    x = torch.empty(n, dtype=torch.uint8, device="cuda")
    c.dev.generate(x.data_ptr(), n, offset=0, kind=1, alpha=1.1, seed=42)
    c.sync()
    data = x.cpu().numpy()
    del x, c
    torch.cuda.empty_cache()
    src = os.path.join(where, "pieces_timing.bin")
    data.tofile(src)
    try:
        name, seek = hz.archive_seek(src, verbose=False)
        os.remove(src)
        offs = [int(v) for v in np.random.default_rng(3).integers(0, n - nbytes + 1, k)]
        pairs = [(o, nbytes) for o in offs]
        want = [data[o:o + nbytes].tobytes() for o in offs]
        blob = np.fromfile(name, dtype=np.uint8)
        _, info = hz.parse_header(blob[:1 << 20])
        pay = blob.size - info.payload_byte
        nsym = n // 2
        rows = [(o // 2, (o + nbytes + 1) // 2 - o // 2, 0) for o in offs]
        pieces, _, buf_bytes, seek_words = hz.seek_pieces(seek, nsym, pay, rows)
        spans = [hz.seek_span(seek, nsym, b, cn) for b, cn, _ in rows]
        blocks = [(b // BLK, (b + cn - 1) // BLK) for b, cn, _ in rows]
        moved = {"pieces": buf_bytes + 8 * seek_words,
                 "calls": sum(min(e, pay) - b + 16 for b, e in spans) + 8 * sum(b1 - b0 + 2 for b0, b1 in blocks),
                 "hull": min(max(e for _, e in spans), pay) - min(b for b, _ in spans) + 16 +
                 8 * (max(b1 for _, b1 in blocks) - min(b0 for b0, _ in blocks) + 2)}
        forms = {"pieces": lambda: hz.decode_ranges_file(name, seek, pairs),
                 "calls": lambda: [hz.decode_range_file(name, seek, o, nbytes) for o in offs],
                 "hull": lambda: hz.decode_ranges(blob, seek, pairs)}
        ok = {f: True for f in forms}
        ts = {f: [] for f in forms}
        for f, fn in forms.items():            # warm-up: the context, the page cache, the allocator
            ok[f] = ok[f] and fn() == want
        for _ in range(reps):                  # alternating
            for f, fn in forms.items():
                t, got = wall(fn)
                ts[f].append(t)
                ok[f] = ok[f] and got == want
        return {"bytes": n, "file_bytes": int(blob.size), "ranges": k, "range_bytes": nbytes, "pieces": int(len(pieces)),
                "wall_ms": {f: stats(v) for f, v in ts.items()}, "h2d_bytes": moved, "all_equal_input": ok,
                "note": "wall clock around the Python call, the file in the page cache; h2d_bytes: payload and seek words"}
    finally:
        for f in (src, src + ".compressed"):
            if os.path.exists(f):
                os.remove(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=16)
    ap.add_argument("--file-gib", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--dir", default="")
    ap.add_argument("--only", default="", choices=["", "k", "p"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = {"tool": "pieces_timing", "build_id": _lib.build_id(), "reps": a.reps}
    if a.only != "p":
        res["k_zipf_%dGiB" % a.gib] = kernel_figure(StreamCodec(0), a.gib << 30, a.reps)
        torch.cuda.empty_cache()
    if a.only != "k":
        where = a.dir or next(d for d in (os.environ.get("TMPDIR"), "/tmp") if d and os.path.isdir(d) and
                              shutil.disk_usage(d).free > 2 * (a.file_gib << 30))
        res["p_file_%dGiB" % a.file_gib] = path_figure(a.file_gib << 30, a.reps, where)
    s = json.dumps(res)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
