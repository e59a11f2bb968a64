"""The block decoder's staggered two-block pipeline (dec_wave_pipe2: a wave's two blocks run half a
block out of phase) at the block counts where its prologue, its loop and its dropped successor meet
the stream's end.

A grid sweep of the decoder is 4096 blocks (256 CUs x 8 waves x 2 blocks), so the streams are
  1, 2, 3, 5        one workgroup: a wave with one block of its pair, waves with none;
  4095 .. 4099      a last pair of one block, exactly one pair per wave, the first second-sweep pairs;
  8193              two full sweeps and one block of a third,
each with a ragged last block, under a LUT codebook with global levels (the codebook of 32 MiB of
Zipf(1.1) bytes) and under the designed hot25 book (lengths 1 .. 25). Every stream goes through
hz_pack and hz_decode; the output equals the input, and for the counts up to 5 and for 4097 the
payload and the block index equal the host model's (tests/ref_stream.py over the CPU oracle).
Outputs sit between 64-byte guards.

And the range pack's carried tail bits (k_pack_write<HOT, RNG>: the 32 bits before a block come from
the emit before it), at 256 MiB plus a few bytes, where the range plan is on (64-block ranges):
a stream whose dominant symbol has a 1-bit code under HOT tables, with block ends of 32 and 40 such
symbols (the last lane holds exactly 32 bits); and a Zipf stream with blocks over any pack slot (the
cold list) as the first block of a range, mid-range with ordinary blocks after it, the last block of
a range, two in a row, and a range's last beside the next one's first. Payload and index equal the
three-pass hz_pack's, the file equals the oracle's, the stream decodes back, and the plan ran.

Tolerance: none -- every check is bit-exact."""
import numpy as np
import pytest

import ref_stream
from test_gpu_designed_streams import _guarded, _guards_intact, _stream, book

pytestmark = pytest.mark.gpu

BLK = 2048
BLOCK_COUNTS = [1, 2, 3, 5, 4095, 4096, 4097, 4099, 8193]
MODEL_COUNTS = {1, 2, 3, 5, 4097}
MAX_SYMS = max(BLOCK_COUNTS) * BLK


def _ragged(nb):
    """nb blocks, the last one partial (1 .. 2047 symbols, another count for every nb)."""
    return (nb - 1) * BLK + 1 + (nb * 613) % (BLK - 1)


@pytest.fixture(scope="module")
def codec(built_lib):
    from huffman_amd.pipeline import StreamCodec
    return StreamCodec(0)


@pytest.fixture(scope="module")
def zipf(codec):
    """(book, symbols): 8193 blocks of Zipf(1.1) bytes from the device generator and their own codebook."""
    import torch
    from types import SimpleNamespace
    from huffman_amd import build_codebook, codebook_arrays
    x = torch.empty(2 * MAX_SYMS, dtype=torch.uint8, device="cuda")
    codec.dev.generate(x.data_ptr(), x.numel(), offset=0, kind=1, alpha=1.1, seed=11)
    codec.sync()
    sym = x.cpu().numpy().view("<u2").copy()
    cb = build_codebook(np.bincount(sym, minlength=65536).astype(np.uint64))
    _, ln, code = codebook_arrays(cb)
    # LUT tables whose long codes leave the LDS levels (level 1 is at most 14 bits wide)
    assert 18 <= int(cb.max_len) <= 25 and int(cb.min_len) < int(cb.max_len) - 3
    return SimpleNamespace(name="zipf", cb=cb, ln=ln, code=code), sym


@pytest.fixture(scope="module")
def hot25():
    """(book, symbols): the 26 symbols of hot25 drawn evenly, about 13 bits a symbol."""
    bk = book("hot25")
    return bk, _stream(bk, "uniform", MAX_SYMS, np.random.default_rng(25))


def _round_trip(codec, bk, sym, with_model):
    import torch
    dev = codec.dev
    nsym = sym.size
    dev.upload(bk.cb)
    pos = ref_stream.positions(sym, bk.ln, 0)
    nbytes = 4 * ((int(pos[-1]) + 31) // 32)
    ibytes = ref_stream.index_nbytes(nsym)
    x = torch.from_numpy(sym.view(np.uint8)).cuda()
    paybuf, pay = _guarded(nbytes)
    idxbuf, idx = _guarded(ibytes)
    dev.pack(x.data_ptr(), x.numel(), 0, 0, pay.data_ptr(), nbytes, idx.data_ptr())
    obuf, out = _guarded(2 * nsym)
    dev.decode(pay.data_ptr(), nbytes, nsym, idx.data_ptr(), out.data_ptr())
    codec.sync()
    assert torch.equal(out, x), "decoded symbols differ from the input"
    assert _guards_intact(obuf, 2 * nsym), "hz_decode wrote outside its output"
    assert _guards_intact(paybuf, nbytes) and _guards_intact(idxbuf, ibytes), "hz_pack wrote outside its outputs"
    if with_model:
        m = ref_stream.model(sym, bk.ln, bk.code)
        assert np.array_equal(pay.cpu().numpy(), m.payload), "payload differs from the model's"
        assert np.array_equal(idx.cpu().numpy(), m.index), "block index differs from the model's"


@pytest.mark.parametrize("nb", BLOCK_COUNTS)
def test_staggered_decode_zipf_lut(codec, zipf, nb):
    bk, sym = zipf
    _round_trip(codec, bk, sym[:_ragged(nb)], nb in MODEL_COUNTS)


@pytest.mark.parametrize("nb", BLOCK_COUNTS)
def test_staggered_decode_hot25(codec, hot25, nb):
    bk, sym = hot25
    _round_trip(codec, bk, sym[:_ragged(nb)], nb in MODEL_COUNTS)


# ---- pack: the range plan's carried tail bits (k_pack_write RNG: a block's leading 32 bits come
# from the emit before it; a range's first block and the block after a cold-listed one form them) --
MIB = 1 << 20
RANGE_BLOCKS = 64            # blocks per range at 256 MiB (hz_internal.h range_geom)
SLOT_CAP_BITS = 1024 * 32    # no pack slot is larger (kPackCopyIters x 64 words): a larger block is cold


def _one_bit_stream(n):
    """n bytes of u16 symbols: 60 % symbol 0 (a 1-bit code), the rest 1 / rank^1.3 over 20 000 symbols
    (codes up to 17 .. 25 bits: HOT tables). Every third block ends in 32 zeros and every seventh in
    40, so the last lane of those blocks holds exactly 32 bits, all of them carried into the next block."""
    rng = np.random.default_rng(60)
    nsym = n // 2
    w = 1.0 / np.arange(1, 20001) ** 1.3
    base = np.where(rng.random(1 << 22) < 0.6, 0, 1 + rng.choice(20000, 1 << 22, p=w / w.sum())).astype("<u2")
    sym = np.tile(base, (nsym + base.size - 1) // base.size)[:nsym]
    sym[(1 << 22):(1 << 23)] = sym[(1 << 22):(1 << 23)][::-1]    # not periodic in the tile
    blocks = sym[:nsym // BLK * BLK].reshape(-1, BLK)
    blocks[::3, BLK - 32:] = 0
    blocks[::7, BLK - 40:] = 0
    return sym


def _check_range_pack(x, host, n):
    """The range plan and the three-pass hz_pack agree byte for byte (payload and index), the plan ran,
    its file equals the oracle's, and the stream decodes back. Returns (plan, start[] of the index)."""
    import torch
    import oracle_lib
    from huffman_amd.codec import Device
    from huffman_amd.pipeline import StreamCodec
    from test_gpu_ranges import _both
    nsym = n // 2
    ((_, p3, i3, _, _), (_, pr, ir, took, rb)), nb, _ = _both(Device(0), x, 0, 0)
    assert rb > 0 and took == 1, "the range plan did not run"
    assert np.array_equal(p3, pr), "payload: range plan != three-pass"
    assert np.array_equal(i3.view(np.uint8)[:nb], ir.view(np.uint8)[:nb]), "index: range plan != three-pass"
    del p3, pr
    c = StreamCodec(0)
    plan, payload, index = c.encode(x)
    assert c.dev.last_pack_ranges() == 1
    assert c.file_image(plan, payload) == oracle_lib.encode(host), "file differs from the oracle's"
    # the file's stream starts plan.start_bit bits in (the header's pending bits), the two above at bit 0:
    # the same index, every start bit moved by that much (max_bits as it is)
    nblk = ref_stream.nblocks(nsym)
    got, want = index.cpu().numpy().view(np.uint8)[:nb], ir.view(np.uint8)[:nb]
    shift = np.uint64(plan.start_bit)
    assert np.array_equal(got[:8 * (nblk + 1)].view(np.uint64), want[:8 * (nblk + 1)].view(np.uint64) + shift)
    assert np.array_equal(got[8 * (nblk + 1):8 * (nblk + 2)], want[8 * (nblk + 1):8 * (nblk + 2)])
    assert np.array_equal(got[8 * (nblk + 2):].view("<u2"), want[8 * (nblk + 2):].view("<u2") + np.uint16(plan.start_bit & 0xffff))
    out =torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    c.decode(payload, nsym, index, out)
    c.sync()
    assert torch.equal(out[:2 * nsym], x[:2 * nsym]), "decode round trip"
    return plan, ir.view(np.uint64)[:ref_stream.nblocks(nsym) + 1]


def test_carried_tail_one_bit_code(built_lib):
    import torch
    from huffman_amd import codebook_arrays
    n = 256 * MIB + 2 * 555
    sym = _one_bit_stream(n)
    host = sym.view(np.uint8)
    x = torch.from_numpy(host).cuda()
    plan, _ = _check_range_pack(x, host, n)
    _, ln, _ = codebook_arrays(plan.cb)
    assert int(ln[0]) == 1 and 17 <= int(plan.cb.max_len) <= 25   # a 1-bit code under HOT tables
    del x
    torch.cuda.empty_cache()


# blocks of rare symbols only (>= 17 bits a symbol: over any slot), by their place in a range
COLD_BLOCKS = [5 * RANGE_BLOCKS,                               # the first block of a range
               9 * RANGE_BLOCKS + 17,                          # mid-range, ordinary blocks after it
               12 * RANGE_BLOCKS + RANGE_BLOCKS - 1,           # the last block of a range
               20 * RANGE_BLOCKS + 30, 20 * RANGE_BLOCKS + 31,  # two in a row, then ordinary blocks
               30 * RANGE_BLOCKS + RANGE_BLOCKS - 1, 31 * RANGE_BLOCKS,  # a range's last and the next one's first
               1000 * RANGE_BLOCKS + 1]                        # the second block of a range


def test_carried_tail_around_cold_blocks(built_lib):
    import torch
    from test_gpu_ranges import _zipf
    n = 256 * MIB + 2 * 901
    x = _zipf(n, 8)
    host = x.cpu().numpy()
    sym = host.view("<u2")
    rng = np.random.default_rng(12)
    for b in COLD_BLOCKS:
        sym[b * BLK:(b + 1) * BLK] = rng.integers(20000, 65536, BLK)
    x.copy_(torch.from_numpy(host))
    torch.cuda.synchronize()
    plan, start = _check_range_pack(x, host, n)
    assert 17 <= int(plan.cb.max_len) <= 25                    # HOT tables
    assert (n // 2 + BLK - 1) // BLK // RANGE_BLOCKS >= 1024   # 64-block ranges
    bits = np.diff(start.astype(np.int64))
    assert int(bits[COLD_BLOCKS].min()) > SLOT_CAP_BITS, "a designed block fits a slot"
    near = [b + d for b in COLD_BLOCKS for d in (-1, 1) if b + d not in COLD_BLOCKS]
    assert int(bits[near].max()) <= SLOT_CAP_BITS
    del x
    torch.cuda.empty_cache()
