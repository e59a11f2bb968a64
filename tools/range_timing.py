"""Timing of random access (DESIGN.md "Random access") on resident Zipf(1.1) streams of 1 GiB and
16 GiB, one StreamCodec.encode each, device events on the codec's stream, every shape warmed up:

  a  hz_decode of the whole stream (the yardstick)
  b  hz_decode_range of the whole stream with HZ_RANGE_FULL_INDEX, alternating with a
  c  hz_decode_range of the whole stream from the seek table alone
  d  hz_index_expand beside hz_index_build
  e  median and p95 latency of 50 seeded random ranges each of 4 KiB, 1 MiB and 64 MiB of output,
     from the seek table and with the full index
  f  hz_decode_ranges (one call for the whole list, a wave per block) beside hz_decode_range (one call per
     range), the two sides alternating in one loop and every result compared with the input: 50 random
     4 KiB ranges and 50 of 1 MiB from the seek table and with the full index, one 4 KiB range from the seek
     table; with stats[2], the most fix-up rounds any block of the run needed
  g  the seek table from the index-less walk: hz_seek_build beside hz_index_build, and
     hz_decode_indexless_seek (with an output) beside hz_decode_indexless, the sides of each pair
     alternating in one loop, every repeat's table compared with pack's start[]; the by-product's cost is
     the difference of the second pair against that pair's own spread

--only f / --only g runs that figure alone. Prints one JSON line (and writes it to --out)."""
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


def batch_figures(c, x, payload, index, seek, nsym, reps):
    """Figure f: (label, ranges, bytes each, modes)."""
    res = {}
    rng = np.random.default_rng(2)
    for label, k, nbytes, modes in (("50x4KiB", 50, 4 << 10, (False, True)), ("1x4KiB", 1, 4 << 10, (False,)),
                                    ("50x1MiB", 50, 1 << 20, (False, True))):
        cnt = nbytes // 2
        begins = [int(v) for v in rng.integers(0, nsym - cnt + 1, k)]
        out = torch.empty(k * nbytes + 16, dtype=torch.uint8, device="cuda")
        want = torch.cat([x[2 * b:2 * b + nbytes] for b in begins])
        rg = torch.tensor([[b, cnt, i * nbytes] for i, b in enumerate(begins)], dtype=torch.int64, device="cuda")
        st = torch.zeros(4, dtype=torch.int64, device="cuda")
        for full in modes:
            table = index if full else seek

            def batch():
                c.decode_ranges(payload, nsym, table, rg, out, stats=st, full_index=full)

            def calls():
                for i, b in enumerate(begins):
                    c.decode_range(payload, nsym, table, b, cnt, out[i * nbytes:], full_index=full)

            ta, tb, ok = [], [], True
            for fn in (batch, calls):  # warm-up (also sizes the scratch)
                timed(c, fn)
            for _ in range(reps):      # alternating
                for fn, ts in ((batch, ta), (calls, tb)):
                    out.zero_()
                    c.sync()
                    ts.append(timed(c, fn))
                    ok = ok and bool(torch.equal(out[:k * nbytes], want))
            timed(c, batch)
            res[f"f_{label}_{'full_index' if full else 'seek_table'}"] = {
                "decode_ranges_ms": stats(ta), "decode_range_calls_ms": stats(tb), "all_equal_input": ok,
                "batch_below_calls_in_every_repeat": max(ta) < min(tb), "stats": [int(v) for v in st.cpu()]}
    return res


def seek_figures(c, x, plan, payload, index, seek, nsym, reps):
    """Figure g."""
    nb = seek.numel() - 1
    pp, pn, sb = payload.data_ptr(), payload.numel(), plan.start_bit
    tab = torch.empty(nb + 1, dtype=torch.int64, device="cuda")
    idx = torch.empty_like(index)
    out = torch.empty(2 * nsym + 16, dtype=torch.uint8, device="cuda")
    end = torch.zeros(2, dtype=torch.int64, device="cuda")

    def seek_build():
        c.dev.seek_build(pp, pn, sb, nsym, tab.data_ptr())

    def index_build():
        c.dev.index_build(pp, pn, sb, nsym, idx.data_ptr())

    def indexless_seek():
        c.dev.decode_indexless_seek(pp, pn, sb, nsym, out.data_ptr(), tab.data_ptr(), end.data_ptr())

    def indexless():
        c.dev.decode_indexless(pp, pn, sb, nsym, out.data_ptr(), end.data_ptr())

    res = {}
    for name, (fa, fb), (ka, kb) in (("g_table", (seek_build, index_build), ("seek_build_ms", "index_build_ms")),
                                     ("g_byproduct", (indexless_seek, indexless),
                                      ("decode_indexless_seek_ms", "decode_indexless_ms"))):
        for fn in (fa, fb):  # warm-up (also sizes the scratch)
            timed(c, fn)
        ta, tb, ok, ok_b = [], [], True, True
        for _ in range(reps):  # alternating
            tab.fill_(-1)
            idx[:nb + 1].fill_(-1)
            end.fill_(-1)
            c.sync()
            ta.append(timed(c, fa))
            ok = ok and bool(torch.equal(tab, seek))
            if name == "g_byproduct":
                ok = ok and int(end[0].item()) == int(seek[-1].item())
                end.fill_(-1)
                c.sync()
            tb.append(timed(c, fb))
            ok_b = ok_b and (bool(torch.equal(idx[:nb + 1], seek)) if name == "g_table"
                             else int(end[0].item()) == int(seek[-1].item()))
        res[name] = {ka: stats(ta), kb: stats(tb), "every_table_equals_pack": ok, "other_side_right": ok_b,
                     "first_below_second_in_every_repeat": max(ta) < min(tb),
                     "median_difference_ms": round(float(np.median(ta)) - float(np.median(tb)), 4)}
    res["g_byproduct"]["output_equals_input"] = bool(torch.equal(out[:2 * nsym], x[:2 * nsym]))
    return res


def case(c, n, reps, only=""):
    x = torch.empty(n, dtype=torch.uint8, device="cuda")
    c.dev.generate(x.data_ptr(), n, offset=0, kind=1, alpha=1.1, seed=42)
    plan, payload, index = c.encode(x)
    c.sync()
    nsym = n // 2
    nb = (nsym + 2047) // 2048
    seek = index[:nb + 1].clone()
    out = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    res = {"bytes": n, "payload_bytes": (plan.start_bit + plan.payload_bits + 7) // 8}
    if only == "f":
        del out
        res.update(batch_figures(c, x, payload, index, seek, nsym, reps))
        return res
    if only == "g":
        del out
        res.update(seek_figures(c, x, plan, payload, index, seek, nsym, reps))
        return res

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
    del out
    res.update(batch_figures(c, x, payload, index, seek, nsym, reps))
    res.update(seek_figures(c, x, plan, payload, index, seek, nsym, reps))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes-gib", type=int, nargs="*", default=[1, 16])
    ap.add_argument("--only", default="", choices=["", "f", "g"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    c = StreamCodec(0)
    res = {"tool": "range_timing", "build_id": _lib.build_id(), "reps": a.reps,
           "note": "ms, HIP events on the codec's stream around each call; a and b alternate in one loop"}
    for g in a.sizes_gib:
        res[f"zipf_{g}GiB"] = case(c, g << 30, a.reps, a.only)
        torch.cuda.empty_cache()
    s = json.dumps(res)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
