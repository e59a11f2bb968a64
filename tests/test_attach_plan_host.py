"""The extract window in rounds of whole blocks (hz_stream_plan.h: ExtractWindow's whole_blocks), the plan of
hz_seekable_attach_file and hz_extract_stream_verified, through tests/attach_probe.cpp: a stand-alone host
program built here with AddressSanitizer and UndefinedBehaviorSanitizer (host code only: every sanitizer flag
goes to the host compilation through -Xarch_host) and run as a plain child process. No GPU.

With the flag on, every round but a file's last is a positive multiple of 2048 symbols, the rounds add up to
the file, each round's codewords lie in its window, and a redo asks for no more than the window holds at
max_len. With the flag off, the rounds are those the struct computed before it had the option:
tests/golden/attach_plan_flag_off.json holds, per case, the round count, the redone rounds and the CRC-32 of
the probe's lines, printed by the probe built against the header as it stood before (-DATTACH_PROBE_NO_FLAG).

Code lengths follow length() below, restated from the probe; everything is judged from them alone."""
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

from huffman_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLK = 2048
MIB = 1 << 20
WINDOWS = [16384, 16400, 65536, MIB]
MAX_LENS = [1, 2, 16, 31, 56]
NSYMS = [1, 2047, 2048, 2049, 40000, 300001]
PATTERNS = [0, 1, 2, 3, 4, 5]        # means from min_len to max_len, the half-and-half ones force redos
RECORDED = os.path.join(ROOT, "tests", "golden", "attach_plan_flag_off.json")
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


def cases():
    """(W, start_bit, max_len, nsym, pattern, min_len, salt) of every case, in the order both runs use."""
    out = []
    for W in WINDOWS:
        for max_len in MAX_LENS:
            for nsym in NSYMS:
                for pattern in PATTERNS:
                    i = len(out)
                    out.append((W, i % 8, max_len, nsym, pattern, 1, i))
    return out


CASES = cases()


def length(nsym, pattern, min_len, max_len, salt):
    i = np.arange(nsym, dtype=np.uint64)
    if pattern == 0:
        return np.full(nsym, min_len, dtype=np.uint64)
    if pattern == 1:
        return np.full(nsym, max_len, dtype=np.uint64)
    if pattern == 2:
        return np.where(i < nsym // 2, min_len, max_len).astype(np.uint64)
    if pattern == 3:
        return np.where(i < nsym // 2, max_len, min_len).astype(np.uint64)
    if pattern == 4:
        return np.uint64(min_len) + (((i + np.uint64(salt)) * np.uint64(2654435761)) >> np.uint64(7)) \
            % np.uint64(max_len - min_len + 1)
    return np.where((i // np.uint64(3000)) % np.uint64(2) == 1, max_len, min_len).astype(np.uint64)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(build.HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("attach_probe") / "attach_probe")
    csrc = os.path.join(ROOT, "huffman_amd", "csrc")
    r = subprocess.run([build.HIPCC, "-O1", "-g", "-std=c++17"] + SAN + [
        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "attach_probe.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_cases(exe, d, flag):
    """The probe on every case with the flag on or off: per case, its lines (status 0 and nothing on stderr:
    no sanitizer report)."""
    inp = d / ("cases%d.bin" % flag)
    inp.write_bytes(np.array([[flag] + list(c) for c in CASES], dtype="<u8").tobytes())
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    per = []
    for line in r.stdout.split("\n")[:-1]:
        if line.startswith("case "):
            assert int(line.split()[1]) == len(per)
            per.append([])
        else:
            per[-1].append(line)
    assert len(per) == len(CASES)
    return per


def check_rounds(case, lines, whole_blocks):
    """The rounds of one case against its code lengths: what tests/test_stream_host.py asks of the plain
    window, and with whole_blocks the block multiples and the redo bound."""
    W, start, max_len, nsym, pattern, min_len, salt = case
    assert "truncated" not in lines, case
    rows = [[int(v) for v in line.split()] for line in lines]
    pos = np.concatenate([[np.uint64(start)], np.uint64(start) + np.cumsum(length(nsym, pattern, min_len, max_len, salt))])
    pos = [int(v) for v in pos] if nsym < 5000 else pos
    pay = (int(pos[-1]) + 7) // 8
    have, consumed, done = min(W, pay), 0, 0
    for k, used, tail, refill, red in rows:
        assert k >= 1 and done + k <= nsym, case
        last = done + k == nsym
        if whole_blocks and not last:
            assert k % BLK == 0, (case, done, k)          # (k >= 1: a positive multiple)
        bit = int(pos[done]) - 8 * consumed               # the round's first codeword, in the window's first byte
        assert 0 <= bit < 8 and consumed + have <= pay
        if red:
            assert k * max_len <= 8 * have - bit, (case, done, k)     # no more than the window holds at max_len
            if not whole_blocks:
                assert k == max((8 * have - bit) // max_len, 1)
        end = int(pos[done + k]) - 8 * consumed           # its k codewords lie in the window
        assert end <= 8 * have and used == end // 8 and tail == have - used, (case, done, k)
        done += k
        if done < nsym:
            assert tail + refill <= W
            consumed += used
            have = tail + refill
        else:
            assert refill == 0
    assert done == nsym, case
    return len(rows), sum(r[4] for r in rows)


def test_whole_block_rounds(probe, tmp_path):
    per = run_cases(probe, tmp_path, 1)
    redone = 0
    for case, lines in zip(CASES, per):
        redone += check_rounds(case, lines, True)[1]
    assert redone > 100          # the sweep does reach the redo path, many times
    # the smallest window holds one block of 56-bit codes and not two: every round but the last is one block
    for case, lines in zip(CASES, per):
        if case[0] == 16384 and case[2] == 56 and case[4] == 1 and case[3] > BLK:
            ks = [int(line.split()[0]) for line in lines]
            assert ks[:-1] == [BLK] * (len(ks) - 1), case


def test_flag_off_is_what_it_was(probe, tmp_path):
    per = run_cases(probe, tmp_path, 0)
    with open(RECORDED) as f:
        recorded = json.load(f)
    assert len(recorded) == len(CASES)
    for case, lines, want in zip(CASES, per, recorded):
        rounds, redone = check_rounds(case, lines, False)
        assert [rounds, redone, zlib.crc32("\n".join(lines).encode())] == want, case
