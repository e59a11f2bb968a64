"""hz_block_sums_mark (hz_sums.hip: k_block_sums_mark) against the model's sums (tests/seekable_model.py:
zlib.adler32 of the zero-extended 4096-byte blocks): every block whose expected word was changed sets its bit
block_base + i in the caller's bitmap and no other bit changes (the bitmap starts as a seeded pattern: the call
ORs into it); with HZ_SUMS_ZERO_BAD exactly those blocks' bytes below n become zeros and every other byte stays
-- the data sits between 0xA5 guard bytes at a 16-byte aligned address, so a store at or past n, in the last
word of a partial block too, shows; without the flag nothing is written. Two calls fold into one bitmap, n == 0
launches nothing, the refused arguments, and a captured graph replayed on other data with other damaged words.

Tolerance: none -- every check is bit-exact."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import seekable_model as model  # noqa: E402

pytestmark = pytest.mark.gpu

BLOCK = 4096
SIZES = [1, 15, 16, 17, 4095, 4096, 4097, 4096 + 4080, 3 * 4096 + 5, 65 * 4096 + 1]
BASES = [0, 1, 31, 33, (1 << 20) + 7]
FRONT, BACK = 64, 4096 + 64
GUARD = 0xA5


@pytest.fixture(scope="module")
def codec(built_lib):
    from huffman_amd.pipeline import StreamCodec
    return StreamCodec(0)


def _host(n, seed=0):
    return np.random.default_rng(n + 7919 * seed).integers(1, 256, n, dtype=np.uint8)    # no zero byte: a zeroed one shows


def _guarded(codec, host):
    """host's bytes on the device between guard bytes: (the whole tensor, the view of the data)."""
    import torch
    buf = torch.full((FRONT + host.size + BACK,), GUARD, dtype=torch.uint8, device=codec.device)
    buf[FRONT:FRONT + host.size] = torch.from_numpy(host).to(codec.device)
    x = buf[FRONT:FRONT + host.size]
    assert x.data_ptr() % 16 == 0
    return buf, x


def _dev(codec, a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).view(np.int32).copy()).to(codec.device)


def _damage_sets(nb):
    sets = [set(), set(range(nb)), {0}, {nb - 1}]
    if nb == 66:
        sets.append({31, 32, 33})
    return sets


def _model(host, pattern, base, damaged, zero):
    """(bitmap, data) after a call whose expected words differ for the blocks of `damaged`."""
    bits = pattern.copy()
    data = host.copy()
    for b in damaged:
        g = base + b
        bits[g >> 5] |= np.uint32(1 << (g & 31))
        if zero:
            data[b * BLOCK:(b + 1) * BLOCK] = 0
    return bits, data


def _expect(want, damaged, salt):
    e = want.copy()
    for k, b in enumerate(sorted(damaged)):
        e[b] ^= np.uint32(1 << ((k + salt) % 32))
    return e


@pytest.mark.parametrize("n", SIZES)
def test_marks_and_zeros_exactly_the_damaged_blocks(codec, n):
    host = _host(n)
    want = model.adler_blocks(host, n)
    nb = want.size
    rng = np.random.default_rng(n)
    for base in BASES:
        words = (base + nb + 31) // 32 + 2
        pattern = rng.integers(0, 1 << 32, words, dtype=np.uint64).astype(np.uint32)
        for k, damaged in enumerate(_damage_sets(nb)):
            for zero in (False, True):
                buf, x = _guarded(codec, host)
                bits = _dev(codec, pattern, np.uint32)
                codec.block_sums_mark(x, _dev(codec, _expect(want, damaged, k), np.uint32), bits, block_base=base, zero_bad=zero)
                codec.sync()
                want_bits, want_data = _model(host, pattern, base, damaged, zero)
                assert np.array_equal(bits.cpu().numpy().view(np.uint32), want_bits), (base, sorted(damaged)[:4], zero)
                got = buf.cpu().numpy()
                assert np.array_equal(got[FRONT:FRONT + n], want_data), (base, sorted(damaged)[:4], zero)
                assert (got[:FRONT] == GUARD).all() and (got[FRONT + n:] == GUARD).all(), (base, sorted(damaged)[:4], zero)


def test_second_call_accumulates(codec):
    n = 5 * 4096 + 1234
    host = _host(n)
    want = model.adler_blocks(host, n)
    _, x = _guarded(codec, host)
    bits = _dev(codec, np.zeros(8, dtype=np.uint32), np.uint32)
    codec.block_sums_mark(x, _dev(codec, _expect(want, {3}, 0), np.uint32), bits, block_base=100)      # 103
    codec.block_sums_mark(x, _dev(codec, _expect(want, {5}, 0), np.uint32), bits, block_base=0)        # 5
    codec.block_sums_mark(x, _dev(codec, want, np.uint32), bits, block_base=0)                         # a clean call: nothing
    codec.block_sums_mark(x, _dev(codec, _expect(want, {3, 5}, 0), np.uint32), bits, block_base=100)   # 103 again, 105
    codec.sync()
    got = bits.cpu().numpy().view(np.uint32)
    assert [g for g in range(256) if got[g >> 5] >> (g & 31) & 1] == [5, 103, 105]


def test_empty_input_launches_nothing(codec):
    import torch
    bits = _dev(codec, np.array([0x12345678], dtype=np.uint32), np.uint32)
    x = torch.empty(0, dtype=torch.uint8, device=codec.device)
    codec.block_sums_mark(x, torch.empty(0, dtype=torch.int32, device=codec.device), bits, zero_bad=True)
    codec.dev.block_sums_mark(0, 0, 0, 0, 0, 1)
    codec.sync()
    assert int(bits.cpu().numpy().view(np.uint32)[0]) == 0x12345678


def test_refused_arguments(codec):
    import huffman_amd
    import torch
    buf = torch.full((8192,), 7, dtype=torch.uint8, device=codec.device)
    exp = torch.zeros(4, dtype=torch.int32, device=codec.device)
    bits = torch.zeros(4, dtype=torch.int32, device=codec.device)
    x, e, b = buf.data_ptr(), exp.data_ptr(), bits.data_ptr()
    refused = [(0, e, b, 0), (x, 0, b, 0), (x, e, 0, 1), (x + 1, e, b, 0), (x + 4, e, b, 1), (x + 8, e, b, 0), (x, e + 2, b, 0),
               (x, e + 1, b, 1), (x, e, b + 2, 0), (x, e, b + 1, 1), (x, e, b, 2), (x, e, b, 3), (x, e, b, 1 << 31)]
    for d_data, d_exp, d_bits, flags in refused:
        with pytest.raises(huffman_amd.HZError) as err:
            codec.dev.block_sums_mark(d_data, 4096, d_exp, 0, d_bits, flags)
        assert err.value.status == -1, (d_data - x, d_exp - e, d_bits - b, flags)
    assert huffman_amd.load().hz_block_sums_mark(None, x, 4096, e, 0, b, 0) == -1
    codec.sync()
    assert int(bits.abs().sum()) == 0 and int((buf != 7).sum()) == 0


def test_captured_graph_replays_on_other_data(codec):
    """Eager first (the call takes no scratch and no tables), captured on data A with one damaged word, replayed
    on data B with other damaged words: the bitmap and the bytes are B's model's."""
    import torch
    n = 3 * 4096 + 100
    a, b = _host(n, 1), _host(n, 2)
    buf, x = _guarded(codec, a)
    exp = _dev(codec, _expect(model.adler_blocks(a, n), {1}, 0), np.uint32)
    bits = _dev(codec, np.zeros(2, dtype=np.uint32), np.uint32)
    codec.block_sums_mark(x, exp, bits, block_base=30, zero_bad=True)
    codec.sync()
    assert bits.cpu().numpy().view(np.uint32).tolist() == [1 << 31, 0]
    x.copy_(torch.from_numpy(a).to(codec.device))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=codec.stream):           # a host wait inside would break the capture
        codec.block_sums_mark(x, exp, bits, block_base=30, zero_bad=True)
    for damaged in ({0, 3}, {2}, set()):
        x.copy_(torch.from_numpy(b).to(codec.device))
        exp.copy_(_dev(codec, _expect(model.adler_blocks(b, n), damaged, 3), np.uint32))
        bits.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want_bits, want_data = _model(b, np.zeros(2, dtype=np.uint32), 30, damaged, True)
        assert np.array_equal(bits.cpu().numpy().view(np.uint32), want_bits), damaged
        got = buf.cpu().numpy()
        assert np.array_equal(got[FRONT:FRONT + n], want_data), damaged
        assert (got[:FRONT] == GUARD).all() and (got[FRONT + n:] == GUARD).all()
