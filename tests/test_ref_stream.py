"""The host model of a packed stream (tests/ref_stream.py) against the CPU oracle and the golden
files: no device, no product kernel. The device tests (test_gpu_designed_streams.py) then compare
hz_pack, the index writers and every decoder with this model.

The model's start[] for romeo.txt equals huffman_amd.build_seek's table, but build_seek runs
hz_index_build on a device (hz_seek_build_host) and has no host form: that comparison lives in the
device tests (test_gpu_designed_streams.py::test_romeo_seek_table_equals_model), and here the model
is pinned by the golden .compressed files and by the oracle's own walk.

Tolerance: none -- bit-exact."""
import os

import numpy as np
import pytest

import oracle_lib
import ref_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _fib_code(k):
    fib = [1, 1]
    while len(fib) < k:
        fib.append(fib[-1] + fib[-2])
    syms = (np.arange(k, dtype=np.uint32) * 257 + 3).astype(np.uint16)
    hist = np.zeros(65536, dtype=np.uint64)
    hist[syms] = fib
    _, ln, code = oracle_lib.codebook(hist)
    return syms, ln, code


@pytest.mark.parametrize("nsym,start_bit,lead", [(1, 0, 0), (7, 5, 0x15), (2048, 31, 0x5a5a5a5b), (2049, 32, 0),
                                                 (3 * 2048 + 5, 45, 0x1234 | 1), (5000, 77, 0x1fff)])
def test_model_payload_round_trips_through_the_oracle_walk(nsym, start_bit, lead):
    syms, ln, code = _fib_code(41)
    rng = np.random.default_rng(nsym)
    sym = syms[rng.integers(0, 41, nsym)]
    sym[: nsym // 2] = syms[rng.integers(0, 8, nsym // 2)]   # long codes first
    m = ref_stream.model(sym, ln, code, start_bit, lead)
    assert m.payload.size % 4 == 0 and 8 * m.payload.size - m.end_bit < 32
    n, xit, out = ref_stream.span_decode(m.payload, ln, code, start_bit, m.end_bit)
    assert n == nsym and xit == m.end_bit and np.array_equal(out, sym)
    # the bits before start_bit in its word are `lead`; the words before it and the bits past the end are zero
    bits = np.unpackbits(m.payload)
    w0 = 32 * (start_bit // 32)
    k = start_bit - w0
    assert not bits[:w0].any() and not bits[m.end_bit:].any()
    assert int("".join(map(str, bits[w0:start_bit])) or "0", 2) == lead & ((1 << k) - 1) == lead


def test_model_index_layout():
    syms, ln, code = _fib_code(41)
    rng = np.random.default_rng(3)
    nsym = 2 * 2048 + 13
    sym = syms[rng.integers(0, 8, nsym)]      # 33..40 bits each: blocks past 65 536 bits
    m = ref_stream.model(sym, ln, code, 5, 1)
    nb = 3
    assert m.index.size == ref_stream.index_nbytes(nsym) == 8 * (nb + 2) + 512 * nb
    start = m.index[:8 * (nb + 1)].view(np.uint64)
    assert int(start[0]) == 5 and int(start[-1]) == m.end_bit and np.all(np.diff(start.astype(np.int64)) > 0)
    assert int(np.diff(start.astype(np.int64))[:2].min()) >= 65536
    assert int(m.index[8 * (nb + 1):8 * (nb + 2)].view(np.uint64)[0]) == m.max_bits == int(np.diff(start).max())
    sub = m.index[8 * (nb + 2):].view("<u2").reshape(nb, 256)
    # every chain start, one codeword at a time
    pos = 5
    for i in range(nsym):
        if i % 8 == 0:
            assert sub[i // 2048, (i % 2048) // 8] == pos & 0xffff
        pos += int(ln[sym[i]])
    assert pos == m.end_bit
    assert (sub[2, 2:] == (m.end_bit & 0xffff)).all()      # chains past the end: the end bit


@pytest.mark.parametrize("name", ["romeo.txt", "synth_zipf_4099.bin"])
def test_model_payload_equals_golden_file(name):
    """The model's payload for a golden input under the file's own codebook, with the header's last
    bits as `lead`, is the golden file's payload byte for byte."""
    with open(os.path.join(GOLD, name), "rb") as f:
        data = np.frombuffer(f.read(), dtype=np.uint8)
    with open(os.path.join(GOLD, name + ".compressed"), "rb") as f:
        blob = np.frombuffer(f.read(), dtype=np.uint8)
    _, ln, code, info = oracle_lib.parse_header(blob)
    pbyte, pbit = info[1], info[2]
    sym = data[: 2 * (data.size // 2)].view("<u2")
    lead = int(blob[pbyte]) >> (8 - pbit) if pbit else 0
    m = ref_stream.model(sym, ln, code, pbit, lead)
    tail = blob[pbyte:]
    assert m.payload.size - 4 < tail.size <= m.payload.size
    assert np.array_equal(m.payload[:tail.size], tail) and not m.payload[tail.size:].any()
    assert int(m.start[0]) == pbit and int(m.start[-1]) == m.end_bit
