"""Timing of random access (DESIGN.md "Random access") on resident Zipf(1.1) streams of 1 GiB and
16 GiB, one StreamCodec.encode each, device events on the codec's stream, every shape warmed up:

  a  hz_decode of the whole stream (the yardstick)
  b  hz_decode_range of the whole stream with HZ_RANGE_FULL_INDEX, alternating with a
  c  hz_decode_range of the whole stream from the seek table alone
  d  hz_index_expand beside hz_index_build
  e  median and p95 latency of 50 seeded random ranges each of 4 KiB, 1 MiB and 64 MiB of output,
     from the seek table and with the full index

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from huffman_amd import _lib  # noqa: E402
from huffman_amd.pipeline import StreamCodec  # noqa: E402


def timed(c, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(c.stream)
    fn()
    e1.record(c.stream)
    c.sync()
    return e0.elapsed_time(e1)


def stats(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 4), "median": round(float(np.median(xs)), 4), "max": round(xs[-1], 4)}


def case(c, n, reps):
    x = torch.empty(n, dtype=torch.uint8, device="cuda")
    c.dev.generate(x.data_ptr(), n, offset=0, kind=1, alpha=1.1, seed=42)
    plan, payload, index = c.encode(x)
    c.sync()
    nsym = n // 2
    nb = (nsym + 2047) // 2048
    seek = index[:nb + 1].clone()
    out = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    res = {"bytes": n, "payload_bytes": (plan.start_bit + plan.payload_bits + 7) // 8}

    def dec():
        c.decode(payload, nsym, index, out)

    def rng_full():
        c.decode_range(payload, nsym, index, 0, nsym, out, full_index=True)

    def rng_seek():
        c.decode_range(payload, nsym, seek, 0, nsym, out, full_index=False)

    for fn in (dec, rng_full, rng_seek):  # warm-up (also sizes the scratch)
        timed(c, fn)
    a, b = [], []
    for _ in range(reps):  # alternating
        a.append(timed(c, dec))
        b.append(timed(c, rng_full))
    res["a_decode_ms"] = stats(a)
    res["b_range_full_index_ms"] = stats(b)
    res["b_equals_input"] = bool(torch.equal(out[:2 * nsym], x[:2 * nsym]))
    res["c_range_seek_table_ms"] = stats([timed(c, rng_seek) for _ in range(reps)])
    res["c_equals_input"] = bool(torch.equal(out[:2 * nsym], x[:2 * nsym]))

    rebuilt = torch.full_like(index, -1)

    def expand():
        c.index_expand(payload, nsym, seek, rebuilt)

    def build():
        c.dev.index_build(payload.data_ptr(), payload.numel(), plan.start_bit, nsym, rebuilt.data_ptr())

    timed(c, expand)
    res["d_expand_equals_pack_index"] = bool(torch.equal(rebuilt, index))
    res["d_index_expand_ms"] = stats([timed(c, expand) for _ in range(reps)])
    timed(c, build)
    res["d_index_build_ms"] = stats([timed(c, build) for _ in range(reps)])
    del rebuilt

    rng = np.random.default_rng(1)
    for label, nbytes in (("4KiB", 4 << 10), ("1MiB", 1 << 20), ("64MiB", 64 << 20)):
        cnt = nbytes // 2
        begins = [int(v) for v in rng.integers(0, nsym - cnt + 1, 50)]
        for mode, table, full in (("seek_table", seek, False), ("full_index", index, True)):
            def one(begin):
                return timed(c, lambda: c.decode_range(payload, nsym, table, begin, cnt, out, full_index=full))
            one(begins[0])
            one(begins[1])
            ts = [one(b0) for b0 in begins]
            ok = bool(torch.equal(out[:nbytes], x[2 * begins[-1]:2 * begins[-1] + nbytes]))
            res[f"e_{label}_{mode}_ms"] = {"median": round(float(np.median(ts)), 4),
                                           "p95": round(float(np.percentile(ts, 95)), 4), "last_equals_input": ok}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes-gib", type=int, nargs="*", default=[1, 16])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    c = StreamCodec(0)
    res = {"tool": "range_timing", "build_id": _lib.build_id(), "reps": a.reps,
           "note": "ms, HIP events on the codec's stream around each call; a and b alternate in one loop"}
    for g in a.sizes_gib:
        res[f"zipf_{g}GiB"] = case(c, g << 30, a.reps)
        torch.cuda.empty_cache()
    s = json.dumps(res)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
