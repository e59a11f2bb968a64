"""hz_block_sums (hz_sums.hip: k_block_sums) against zlib.adler32 of the zero-extended 4096-byte blocks:
sizes around a word, a vector and a block, contents that reach the accumulator bound, an input that sits
in a larger tensor whose bytes from n on are 0xFF (a kernel that sums past n fails), one large buffer
(many workgroups, the grid stride), an unaligned input, and a captured graph replayed on new contents.

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

SIZES = [1, 2, 15, 16, 17, 4095, 4096, 4097, 8190, 3 * 4096, 5 * 4096 + 1234]
CONTENTS = ["zeros", "ones", "random", "ramp"]
PAD = 4096 + 64      # 0xFF bytes behind the input: a whole block and more


def _content(kind, n):
    if kind == "zeros":
        return np.zeros(n, dtype=np.uint8)
    if kind == "ones":
        return np.full(n, 0xFF, dtype=np.uint8)
    if kind == "random":
        return np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
    return (np.arange(n, dtype=np.uint64) % 251).astype(np.uint8)


@pytest.fixture(scope="module")
def codec(built_lib):
    from huffman_amd.pipeline import StreamCodec
    return StreamCodec(0)


def _padded(codec, host):
    """The bytes on the device with PAD bytes of 0xFF behind them; returns (whole tensor, the input's view)."""
    import torch
    buf = torch.full((host.size + PAD,), 0xFF, dtype=torch.uint8, device=codec.device)
    buf[:host.size] = torch.from_numpy(host).to(codec.device)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[:host.size]


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("n", SIZES)
def test_block_sums_equal_zlib(codec, n, kind):
    import huffman_amd
    host = _content(kind, n)
    buf, x = _padded(codec, host)
    sums = codec.block_sums(x)
    codec.sync()
    got = sums.cpu().numpy().view(np.uint32)
    assert got.size == (n + 4095) // 4096 == huffman_amd.block_sums_bytes(n) // 4
    assert np.array_equal(got, model.adler_blocks(host, n)), (n, kind)
    assert bytes(buf[n:].cpu().numpy()) == b"\xff" * PAD      # and nothing was written there


def test_all_ff_block_is_the_accumulator_bound(codec):
    _, x = _padded(codec, np.full(4096, 0xFF, dtype=np.uint8))
    sums = codec.block_sums(x)
    codec.sync()
    assert int(sums.cpu().numpy().view(np.uint32)[0]) == 0x8161f0e2


def test_large_zipf_buffer_in_one_call(codec):
    """16 MiB + 4097 bytes: 4098 blocks, more than one block per wave of the grid, the last one byte long."""
    import torch
    n = (16 << 20) + 4097
    buf = torch.full((n + PAD,), 0xFF, dtype=torch.uint8, device=codec.device)
    codec.dev.generate(buf.data_ptr(), n, offset=0, kind=1, alpha=1.1, seed=9)
    sums = codec.block_sums(buf[:n])
    codec.sync()
    host = buf[:n].cpu().numpy()
    assert np.array_equal(sums.cpu().numpy().view(np.uint32), model.adler_blocks(host, n))


def test_empty_input_launches_nothing(codec):
    import torch
    x = torch.empty(0, dtype=torch.uint8, device=codec.device)
    assert codec.block_sums(x).numel() == 0
    codec.dev.block_sums(0, 0, 0)
    codec.sync()


def test_unaligned_input_is_einval(codec):
    import huffman_amd
    import torch
    buf = torch.zeros(8192, dtype=torch.uint8, device=codec.device)
    sums = torch.zeros(4, dtype=torch.int32, device=codec.device)
    for off in (1, 4, 8):
        with pytest.raises(huffman_amd.HZError) as e:
            codec.dev.block_sums(buf.data_ptr() + off, 4096, sums.data_ptr())
        assert e.value.status == -1
    codec.sync()
    assert int(sums.abs().sum()) == 0


def test_captured_graph_replays_on_new_contents(codec):
    import torch
    n = 3 * 4096 + 100
    buf, x = _padded(codec, _content("random", n))
    sums = torch.zeros(4, dtype=torch.int32, device=codec.device)
    codec.dev.block_sums(x.data_ptr(), n, sums.data_ptr())     # eager first
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=codec.stream):           # a host wait inside would break the capture
        codec.dev.block_sums(x.data_ptr(), n, sums.data_ptr())
    for kind in ("ramp", "ones", "random"):
        host = _content(kind, n)[::-1].copy()
        x.copy_(torch.from_numpy(host).to(codec.device))
        sums.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(sums.cpu().numpy().view(np.uint32), model.adler_blocks(host, n)), kind
