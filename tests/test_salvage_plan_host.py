"""The windows of hz_seekable_salvage_file (hz_salvage_plan.h: SalvagePlan) over seek tables that may be damaged,
through tests/salvage_probe.cpp: a stand-alone host program built here with AddressSanitizer and
UndefinedBehaviorSanitizer, unsigned wrap-around trapped too (host code only: every sanitizer flag goes to the
host compilation through -Xarch_host), and run as a plain child process. No GPU.

Tables come from block lengths drawn per block between 2048 x 1 and 2048 x 56 bits (the last block may be
partial), damaged by replacing seeded entries with values from {0, 1, entry - 1, entry + 1, entry + 2^20, 2^63,
2^64 - 1}. Judged from the printed windows alone, with hz_seek_span restated below:
  1. every block lies in exactly one window and the windows ascend;
  2. with an undamaged table every window's span is hz_seek_span of its symbols, stays within chunk_bytes
     (one block may exceed it; none does at these sizes), holds no more output than chunk_bytes, and ends only
     where the next block would not fit;
  3. with damaged entries, every block whose own two entries are undamaged has its hz_seek_span inside its
     window's span, and every span stays within chunk_bytes and the payload plus the tail margin;
  4. nothing wraps: the probe exits 0 with nothing on stderr."""
import os
import subprocess

import numpy as np
import pytest

from huffman_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLK = 2048
MAX_LEN = 56
LEAD = TAIL = 32
MIN_WINDOW = 16384
CHUNKS = [MIN_WINDOW, 64 << 10, 1 << 30]
NBLOCKS = [1, 2, 37, 1000]
FRACTIONS = [0.01, 0.03, 0.10]
SAN = ["-Xarch_host", "-fsanitize=address,undefined,unsigned-integer-overflow", "-Xarch_host", "-fno-sanitize-recover=all"]


def damage_values(e):
    """What a damaged entry e may hold (never e itself)."""
    return [v for v in (0, 1, e - 1, e + 1, e + (1 << 20), 1 << 63, (1 << 64) - 1) if v != e and v >= 0]


def table(nb, partial, seed):
    """(entries as Python ints, payload_bytes) of nb blocks, the last one of 777 symbols when partial."""
    rng = np.random.default_rng(seed)
    syms = [BLK] * nb
    if partial:
        syms[-1] = 777
    t = [int(rng.integers(0, 8))]
    for s in syms:
        t.append(t[-1] + int(rng.integers(s * 1, s * MAX_LEN + 1)))
    return t, (t[-1] + 7) // 8


def cases():
    """(true table, table handed to the plan, damaged indices, payload_bytes, chunk_bytes) of every case."""
    out = []
    for nb in NBLOCKS:
        for partial in (False, True):
            true, pay = table(nb, partial, 1000 * nb + partial)
            variants = [(true, set())]
            for k, frac in enumerate(FRACTIONS):
                for seed in (0, 1):
                    rng = np.random.default_rng(7 * nb + 100 * k + seed)
                    idx = rng.choice(nb + 1, size=max(1, round(frac * (nb + 1))), replace=False)
                    t = list(true)
                    for i in idx:
                        vals = damage_values(true[i])
                        t[i] = vals[int(rng.integers(0, len(vals)))]
                    variants.append((t, {int(i) for i in idx}))
            for i in (0, nb):                       # the first and the last entry, every value
                for j in range(len(damage_values(true[i]))):
                    t = list(true)
                    t[i] = damage_values(true[i])[j]
                    variants.append((t, {i}))
            # runs of entries moved by one amount agree with each other: trust by neighbours would keep them
            if nb >= 37:
                t = list(true)
                for i in (10, 11, 12):
                    t[i] = true[i] + (1 << 20)
                variants.append((t, {10, 11, 12}))
            for t, idx in variants:
                assert all(t[i] != true[i] for i in idx)
                for chunk in CHUNKS:
                    out.append((true, t, idx, pay, chunk))
    return out


CASES = cases()


def span(s0, s1):
    """hz_seek_span of a run of blocks that starts at bit s0 and ends at bit s1."""
    first, last = s0 // 8, (s1 + 7) // 8
    return (((first - LEAD) & ~15) if first > LEAD else 0), last + TAIL


@pytest.fixture(scope="module")
def windows(tmp_path_factory):
    """The probe built and run once over every case: per case, its windows as tuples of ints."""
    if not os.path.exists(build.HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("salvage_probe")
    exe = str(d / "salvage_probe")
    csrc = os.path.join(ROOT, "huffman_amd", "csrc")
    r = subprocess.run([build.HIPCC, "-O1", "-g", "-std=c++17"] + SAN + [
        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "salvage_probe.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    words = []
    for true, t, idx, pay, chunk in CASES:
        words += [len(t) - 1, pay, MAX_LEN, chunk] + t
    inp = d / "cases.bin"
    inp.write_bytes(np.array(words, dtype=np.uint64).astype("<u8").tobytes())
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])     # property 4
    per = []
    for line in r.stdout.split("\n")[:-1]:
        if line.startswith("case "):
            assert int(line.split()[1]) == len(per)
            per.append([])
        else:
            per[-1].append(tuple(int(v) for v in line.split()))
    assert len(per) == len(CASES)
    return per


def test_cases_cover_what_they_should():
    assert {len(c[0]) - 1 for c in CASES} == set(NBLOCKS)
    assert any(0 in c[2] for c in CASES) and any(len(c[1]) - 1 in c[2] for c in CASES)
    assert any(len(c[2]) >= 100 for c in CASES)


def test_every_block_in_exactly_one_window(windows):
    for (true, t, idx, pay, chunk), ws in zip(CASES, windows):
        at = 0
        for first, nb, begin, end in ws:
            assert first == at and nb >= 1, (first, at)
            at += nb
        assert at == len(t) - 1


def test_undamaged_windows_are_seek_spans(windows):
    seen = 0
    for (true, t, idx, pay, chunk), ws in zip(CASES, windows):
        if idx:
            continue
        seen += 1
        cap = max(chunk // (2 * BLK), 1)
        for k, (first, nb, begin, end) in enumerate(ws):
            assert (begin, end) == span(t[first], t[first + nb]), (chunk, first, nb)
            assert end - begin <= chunk and nb <= cap
            if k + 1 < len(ws):     # greedy: the next block did not fit
                b, e = span(t[first], t[first + nb + 1])
                assert nb == cap or e - b > chunk, (chunk, first, nb)
        if chunk == 1 << 30:
            assert len(ws) == 1
        if chunk == MIN_WINDOW and len(t) > 3:
            assert len(ws) > 1
    assert seen == len(NBLOCKS) * 2 * len(CHUNKS)


def test_undamaged_blocks_keep_their_span(windows):
    checked = lost = 0
    for (true, t, idx, pay, chunk), ws in zip(CASES, windows):
        for first, nb, begin, end in ws:
            assert 0 <= begin <= end <= pay + TAIL, (begin, end, pay)
            assert end - begin <= chunk, (chunk, first, nb, begin, end)
            for b in range(first, first + nb):
                if b in idx or b + 1 in idx:
                    lost += 1
                    continue
                lo, hi = span(true[b], true[b + 1])
                assert begin <= lo and hi <= end, (sorted(idx)[:8], chunk, b, (lo, hi), (begin, end))
                checked += 1
    assert checked > 10000 and lost > 1000
