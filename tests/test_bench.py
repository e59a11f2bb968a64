"""bench.py's command line: a plain run prints the headline line alone, --full adds the other
measurements, --dump-outputs writes what the last timed step computed.

Tolerance: none (the dumped arrays are bytes and counts, exact in float32 / float64)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}


def test_dump_outputs_sample_is_fixed(tmp_path):
    """A long array is dumped as the same DUMP_SAMPLE elements every time, in order; short arrays,
    host bytes and 64-bit counts are dumped whole and exact."""
    import torch
    import bench
    n = bench.DUMP_SAMPLE + 12345
    long = (torch.arange(n, dtype=torch.int64) % 251).to(torch.uint8)
    counts = torch.tensor([0, 1, (1 << 40) + 1], dtype=torch.int64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"long": long, "short": long[:1000], "raw": b"\x00\x07\xff",
                                               "empty": b"", "counts": counts})
    a = np.load(tmp_path / "a" / "long.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_SAMPLE,)
    assert np.array_equal(a, np.load(tmp_path / "b" / "long.npy"))
    # the sample is long[pos] for sorted positions: every 251-cycle of the ramp shows in it
    assert len(np.unique(a)) == 251 and np.all((np.diff(a) >= 0) | (np.diff(a) < -200))
    assert np.array_equal(np.load(tmp_path / "a" / "short.npy"), long[:1000].numpy().astype(np.float32))
    assert np.load(tmp_path / "a" / "raw.npy").tolist() == [0.0, 7.0, 255.0]
    assert np.load(tmp_path / "a" / "empty.npy").shape == (0,)
    c = np.load(tmp_path / "a" / "counts.npy")
    assert c.dtype == np.float64 and c.tolist() == [0.0, 1.0, float((1 << 40) + 1)]


def _bench(tmp_path, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--size", str((1 << 20) + 2), *extra]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines  # the JSON line alone goes to stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """1 MiB + 2 B of the bench stream (below DUMP_SAMPLE: every array whole): header + payload is the
    oracle's .compressed file, decoded is the input, the histogram is the oracle's; the line holds the
    headline and none of --full's measurements."""
    line = _bench(tmp_path, "--dump-outputs", str(tmp_path / "dump"))
    assert HEADLINE <= set(line) and line["steps"] == 2 and line["warmup"] == 1
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["roundtrip_bit_exact"] is True and line["ms_per_step"] > 0
    n = (1 << 20) + 2
    assert abs(line["value"] - n / (line["ms_per_step"] / 1e3) / 1e9) <= 0.01 * line["value"] + 0.01
    for key in ("dropin", "kernel_ms", "roofline", "cpu_baseline", "extract_indexless", "index_build_from_payload"):
        assert key not in line
    got = {f[:-4]: np.load(tmp_path / "dump" / f) for f in sorted(os.listdir(tmp_path / "dump"))}
    assert sorted(got) == ["decoded", "header", "histogram", "index", "payload"]
    assert got["histogram"].dtype == np.float64 and all(got[k].dtype == np.float32 for k in got if k != "histogram")
    data = oracle_lib.generate(n, offset=0, kind=1, seed=42)
    assert np.array_equal(got["decoded"], data.astype(np.float32))
    assert np.array_equal(got["histogram"], oracle_lib.hist16(data).astype(np.float64))
    image = got["header"].astype(np.uint8).tobytes() + got["payload"].astype(np.uint8).tobytes()
    assert image == oracle_lib.encode(data)
    import huffman_amd
    assert got["index"].size == huffman_amd.index_bytes(n // 2)


@pytest.mark.gpu
def test_full_run_keeps_the_other_measurements(tmp_path):
    line = _bench(tmp_path, "--full", "--no-cpu-baseline")
    assert HEADLINE <= set(line) and line["roundtrip_bit_exact"] is True
    for key in ("dropin", "kernel_ms", "kernel_GBps", "roofline", "encode_roofline", "extract_roofline",
                "index_roofline", "extract_indexless", "index_build_from_payload", "file_roundtrip"):
        assert key in line, key
    assert line["dropin"]["roundtrip_bit_exact"] and line["dropin"]["steps"] == 2
    assert line["index_build_from_payload"]["matches_pack_index"] and line["extract_indexless"]["bit_exact"]
