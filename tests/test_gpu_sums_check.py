"""hz_block_sums_check (hz_sums.hip: k_block_sums_check) against the model's sums (tests/seekable_model.py:
zlib.adler32 of the zero-extended 4096-byte blocks): equal words leave the caller's bad-block word alone,
wrong words fold the smallest block_base + i into it (block bases past 2^32 too), several calls fold into one
word, n == 0 launches nothing, the refused arguments, one large buffer that takes the grid stride, and a
captured graph replayed after the data changed. The input sits in a larger tensor whose bytes from n on are
0xFF: a kernel that sums past n reports a mismatch. hz_block_sums on the same inputs gives the same words.

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

ONES = (1 << 64) - 1
SIZES = [1, 17, 4095, 4096, 4097, 5 * 4096 + 1234]
BIG = (33 << 20) + 4097      # 8450 blocks: more than 8 workgroups x 256 CUs x 4 blocks, the last one byte long
BASES = [0, (1 << 32) + 5]
PAD = 4096 + 64


@pytest.fixture(scope="module")
def codec(built_lib):
    from huffman_amd.pipeline import StreamCodec
    return StreamCodec(0)


def _host(n):
    return np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)


def _want(host):
    """The model's words of host's bytes; for an even size they are block_sums() of an original."""
    want = model.adler_blocks(host, host.size)
    if host.size % 2 == 0:
        assert np.array_equal(want, model.block_sums(host.tobytes()))
    return want


def _padded(codec, host):
    import torch
    buf = torch.full((host.size + PAD,), 0xFF, dtype=torch.uint8, device=codec.device)
    buf[:host.size] = torch.from_numpy(host).to(codec.device)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[:host.size]


def _words(codec, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to(codec.device)


def _bad(codec, value=ONES):
    import torch
    return torch.from_numpy(np.array([value], dtype=np.uint64).view(np.int64).copy()).to(codec.device)


def _get(codec, bad):
    codec.sync()
    return int(bad.cpu().numpy().view(np.uint64)[0])


@pytest.fixture(scope="module")
def big(codec):
    """The large buffer, generated on the device, its bytes on the host and the model's words: made once."""
    import torch
    buf = torch.full((BIG + PAD,), 0xFF, dtype=torch.uint8, device=codec.device)
    codec.dev.generate(buf.data_ptr(), BIG, offset=0, kind=1, alpha=1.1, seed=9)
    codec.sync()
    host = buf[:BIG].cpu().numpy()
    return buf, buf[:BIG], host, _want(host)


@pytest.mark.parametrize("n", SIZES)
def test_equal_words_leave_bad_alone(codec, n):
    host = _host(n)
    buf, x = _padded(codec, host)
    want = _want(host)
    for start in (ONES, 7):
        bad = _bad(codec, start)
        codec.block_sums_check(x, _words(codec, want), bad, block_base=3)
        assert _get(codec, bad) == start
    assert bytes(buf[n:].cpu().numpy()) == b"\xff" * PAD
    assert np.array_equal(codec.block_sums(x).cpu().numpy().view(np.uint32), want)     # hz_block_sums: as before


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("n", SIZES)
def test_wrong_words_give_the_smallest_block(codec, n, base):
    host = _host(n)
    _, x = _padded(codec, host)
    want = _want(host)
    nb = want.size
    for j, k in {(0, nb - 1), (nb // 2, nb - 1), (nb - 1, nb - 1)}:
        exp = want.copy()
        exp[j] ^= 1
        exp[k] ^= 0x10000
        bad = _bad(codec)
        codec.block_sums_check(x, _words(codec, exp), bad, block_base=base)
        assert _get(codec, bad) == base + j, (n, j, k)
    # the last, partial block's zero extension is part of its sum: the bytes alone (no ljust) do not match
    if n % 4096:
        import zlib
        exp = want.copy()
        exp[-1] = zlib.adler32(host[(nb - 1) * 4096:].tobytes())
        bad = _bad(codec)
        codec.block_sums_check(x, _words(codec, exp), bad, block_base=base)
        assert _get(codec, bad) == base + nb - 1


def test_large_buffer_takes_the_grid_stride(codec, big):
    buf, x, host, want = big
    assert want.size == 8450 > 8 * 256 * 4
    exp = _words(codec, want)
    bad = _bad(codec)
    codec.block_sums_check(x, exp, bad)
    assert _get(codec, bad) == ONES
    assert np.array_equal(codec.block_sums(x).cpu().numpy().view(np.uint32), want)
    for base in BASES:
        for j, k in ((8449, 8449), (8200, 8449), (4097, 8300), (0, 1)):
            e = want.copy()
            e[j] ^= 0x80000000
            e[k] ^= 2
            bad = _bad(codec)
            codec.block_sums_check(x, _words(codec, e), bad, block_base=base)
            assert _get(codec, bad) == base + j, (base, j, k)
    assert bytes(buf[BIG:].cpu().numpy()) == b"\xff" * PAD


def test_two_calls_fold_into_one_word(codec):
    n = 5 * 4096 + 1234
    host = _host(n)
    _, x = _padded(codec, host)
    want = _want(host)
    e3, e5 = want.copy(), want.copy()
    e3[3] ^= 4
    e5[5] ^= 4
    bad = _bad(codec)
    codec.block_sums_check(x, _words(codec, e3), bad, block_base=100)     # 103
    codec.block_sums_check(x, _words(codec, e5), bad, block_base=0)       # 5: the smaller one stays
    codec.block_sums_check(x, _words(codec, want), bad, block_base=0)     # a clean call changes nothing
    codec.block_sums_check(x, _words(codec, e3), bad, block_base=6)       # 9
    assert _get(codec, bad) == 5
    bad = _bad(codec)
    codec.block_sums_check(x, _words(codec, e5), bad, block_base=0)
    codec.block_sums_check(x, _words(codec, e3), bad, block_base=1 << 40)
    assert _get(codec, bad) == 5


def test_empty_input_launches_nothing(codec):
    import torch
    bad = _bad(codec, 12345)
    x = torch.empty(0, dtype=torch.uint8, device=codec.device)
    codec.block_sums_check(x, torch.empty(0, dtype=torch.int32, device=codec.device), bad)
    codec.dev.block_sums_check(0, 0, 0, 0, 0)
    assert _get(codec, bad) == 12345


def test_refused_arguments(codec):
    import huffman_amd
    import torch
    buf = torch.zeros(8192, dtype=torch.uint8, device=codec.device)
    exp = torch.zeros(4, dtype=torch.int32, device=codec.device)
    bad = torch.zeros(2, dtype=torch.int64, device=codec.device)
    x, e, b = buf.data_ptr(), exp.data_ptr(), bad.data_ptr()
    refused = [(0, e, b), (x, 0, b), (x, e, 0), (x + 1, e, b), (x + 4, e, b), (x + 8, e, b), (x, e + 2, b), (x, e + 1, b),
               (x, e, b + 4), (x, e, b + 1)]
    for d_in, d_exp, d_bad in refused:
        with pytest.raises(huffman_amd.HZError) as err:
            codec.dev.block_sums_check(d_in, 4096, d_exp, 0, d_bad)
        assert err.value.status == -1, (d_in - x, d_exp - e, d_bad - b)
    assert huffman_amd.load().hz_block_sums_check(None, x, 4096, e, 0, b) == -1
    codec.sync()
    assert int(bad.abs().sum()) == 0 and int(exp.abs().sum()) == 0


def test_captured_graph_replays_after_the_data_changed(codec):
    """Eager first (nothing to allocate or upload: the call takes no scratch and no tables), captured on data
    that matches, replayed after the data changed so that one block fails, then another, then none."""
    import torch
    n = 3 * 4096 + 100
    host = _host(n)
    _, x = _padded(codec, host)
    exp = _words(codec, _want(host))
    bad = _bad(codec)
    codec.block_sums_check(x, exp, bad, block_base=10)
    assert _get(codec, bad) == ONES
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=codec.stream):           # a host wait inside would break the capture
        codec.block_sums_check(x, exp, bad, block_base=10)
    for byte, block in ((2 * 4096 + 5, 2), (4096 - 1, 0), (n - 1, 3), (None, None)):
        now = host.copy()
        if byte is not None:
            now[byte] ^= 0x40
        x.copy_(torch.from_numpy(now).to(codec.device))
        bad.copy_(_bad(codec))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert _get(codec, bad) == (ONES if block is None else 10 + block), byte
