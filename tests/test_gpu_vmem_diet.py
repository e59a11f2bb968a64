"""The staging chunk the block decoder no longer loads per block, at the places where leaving it out
could change a result, and the range pack's stores at the places where thinning them could.

Decode (dec_wave_pipe2, the two-blocks-per-wave decoder of LUT codebooks up to 25 bits):
  * streams of 1, 2, 3 and 4097 blocks with a ragged last block, with three and with four staging
    chunks per block, so the prologue, the loop and the dropped successor run under both counts (the
    chain starts by one 8-byte load per lane and a transposition through the slot, measured beside
    it and not kept -- DESIGN.md section 9, round 8 -- would meet its edges at the same counts);
  * three staging chunks per block where the payload's mean block fits 3 KiB: a stream built block
    by block under the hot25 book (every length 1 .. 25, so any block size in bits can be hit) whose
    mean is below the launcher's bound while it holds a block whose staging window is exactly the
    768 words three chunks cover, that block one word shorter, one bit longer and one word longer,
    blocks between 3 and 4 KiB and blocks over 4 KiB up to the largest there is (2048 x 25 bits).
    hz_last_decode_chunks says which count ran, so the test cannot pass on 4.
  A block of 65 536 bits or more (dec_chain_offsets' rebuild from deltas) cannot reach that decoder:
  its codes end at 25 bits, 51 200 bits a block. The rebuild is shared with the other decoders, so
  the fib57 stream of the designed-streams tests (blocks of 2048 x 56 bits) is decoded here too.
  Run as a script (`python tests/test_gpu_vmem_diet.py pipe`) the decode cases run once and print
  "ok": HZ_DEC_PIPE=0 / 1, read once per process, select the other decoder forms.

Pack (k_pack_write<HOT, RNG, SPLIT>, one wave writing a range's blocks in order). Two changes to its
stores were measured beside the decoder's and not kept: whole 16-byte
chunks only, with a block's trailing words carried in the LDS slot into the next block's first chunk,
and block start bits stored 64 at a time. What they would have had to preserve is pinned here for
the copy-out as it is and for any later attempt: the 16-byte chunk two waves share at a range boundary,
the chunks a cold-listed block shares with its neighbours, and every index entry.
One Zipf stream of 256 MiB (64-block ranges) plus 62 blocks and a
partial one, with blocks over any slot (cold-listed) planted first, mid and last in a range, two in a
row and on both sides of a range boundary; its prefixes end in a range of 63, 2 and 1 blocks. Payload,
start[] (entry by entry, start[nblocks] included), max_bits and sub[] equal the host model's
(tests/ref_stream.py), the 16-byte chunks around every range boundary are compared on their own, the
stream decodes back to the input, and all four values of (first word & 3) occur at block starts inside
ranges (0 among them: nothing carried). Ranges of 65 and 129 blocks need 512 MiB and 1 GiB of input:
there the plan's payload and index equal the three-pass hz_pack's (itself pinned against the oracle
in the other pack tests), boundary chunks named, and the stream decodes back.

Every output sits between 64-byte guards of 0xA5 (the three-pass comparison: 0xA5 fill past the end).
Tolerance: none -- every check is bit-exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import ref_stream  # noqa: E402
from test_gpu_designed_streams import _guarded, _guards_intact, _stream, book  # noqa: E402

pytestmark = pytest.mark.gpu

BLK = 2048
MIB = 1 << 20
PIPE2 = os.environ.get("HZ_DEC_PIPE", "2") not in ("0", "1")   # else the forms without a chunk count
CHUNK_WORDS = 4 * 64            # one staging chunk per lane: 1 KiB
FEW = 3


# ---- decode ------------------------------------------------------------------------------------
def _ragged(nb):
    return (nb - 1) * BLK + 1 + (nb * 613) % (BLK - 1)


def _mixed(bk, nsym, p_short, rng):
    """hot25 symbols: the 1-bit symbol with probability p_short, else any of the 26 evenly
    (13.5 bits a symbol at p_short = 0: 3.4 KiB a block; 10.3 bits at 0.25: 2.6 KiB)."""
    alphabet = np.nonzero(bk.ln)[0].astype(np.uint16)
    one = alphabet[bk.ln[alphabet] == 1]
    assert one.size == 1
    sym = alphabet[rng.integers(0, alphabet.size, nsym)]
    sym[rng.random(nsym) < p_short] = one[0]
    return np.ascontiguousarray(sym, dtype="<u2")


def _window_words(start):
    """Words of every block's staging window (dec_stage_commit): from the 16-byte chunk before the
    one holding the block's first bit to two words past the word of its end bit."""
    b0, b1 = start[:-1].astype(np.int64), start[1:].astype(np.int64)
    return (b1 >> 5) + 2 - (((b0 >> 5) & ~3) - 4)


def _sized_stream(bk, rng):
    """Blocks of chosen bit counts under hot25, in stream order (the start bit of each is known when
    it is drawn): see the module docstring. Returns (symbols, the designed blocks' numbers by kind)."""
    by_len = {int(bk.ln[s]): s for s in np.nonzero(bk.ln)[0]}
    assert sorted(by_len) == list(range(1, 26))

    def block(bits):
        assert BLK <= bits <= 25 * BLK
        lens = np.ones(BLK, dtype=np.int64)
        n25, rem = divmod(bits - BLK, 24)
        lens[:n25] = 25
        if rem:
            lens[n25] = 1 + rem
        rng.shuffle(lens)
        return np.array([by_len[int(v)] for v in lens], dtype="<u2")

    out, kinds, pos = [], {}, 0

    def add(bits, kind=None):
        nonlocal pos
        if kind:
            kinds.setdefault(kind, []).append(len(out))
        out.append(block(bits))
        pos += bits

    def small():
        add(8 * (2500 + int(rng.integers(0, 200))))

    for _ in range(3):
        small()
    for d, kind in ((0, "exact"), (-32, "word_less"), (1, "bit_more"), (32, "word_more")):
        first_chunk = (pos >> 5) & ~3
        # the largest block whose window is FEW chunks: its end bit is the last of word first_chunk + 762
        add(32 * (first_chunk + FEW * CHUNK_WORDS - 5) - 1 - pos + d, kind)
        small()
        small()
    for bits in (8 * 3250, 8 * 3750, 8 * 4000):
        add(bits, "to_4k")
        small()
    for bits in (8 * 4200, 8 * 5000, 25 * BLK):
        add(bits, "over_4k")
        small()
    for _ in range(30):
        small()
    sym = np.concatenate(out + [block(8 * 2500)[:777]])   # a ragged last block
    return sym, kinds


def _decode_check(codec, bk, sym, chunks):
    """hz_decode of the model's payload and index: the input, inside the guards; the chunk count."""
    import torch
    dev = codec.dev
    m = ref_stream.model(sym, bk.ln, bk.code)
    dev.upload(bk.cb)
    nsym, nbytes = sym.size, m.payload.size
    paybuf, pay = _guarded(nbytes)
    pay.copy_(torch.from_numpy(m.payload))
    assert pay.data_ptr() % 64 == 0          # the stream's bit 0 is the view's bit 0 (window sizes as designed)
    index = torch.from_numpy(m.index).cuda()
    want = torch.from_numpy(sym.view(np.uint8).copy()).cuda()
    obuf, out = _guarded(2 * nsym)
    torch.cuda.synchronize()
    dev.decode(pay.data_ptr(), nbytes, nsym, index.data_ptr(), out.data_ptr())
    codec.sync()
    got = dev.last_decode_chunks()
    assert torch.equal(out, want), "decoded symbols differ from the input"
    assert _guards_intact(obuf, 2 * nsym), "hz_decode wrote outside its output"
    assert np.array_equal(pay.cpu().numpy(), m.payload) and _guards_intact(paybuf, nbytes), "the payload changed"
    if chunks is not None:
        assert got == (chunks if PIPE2 else 0), f"{got} staging chunks per block, expected {chunks}"
    return m


@pytest.fixture(scope="module")
def codec(built_lib):
    from huffman_amd.pipeline import StreamCodec
    return StreamCodec(0)


BLOCK_COUNTS = [1, 2, 3, 4097]


def _count_case(codec, nb, chunks):
    bk = book("hot25")
    sym = _mixed(bk, _ragged(nb), 0.25 if chunks == FEW else 0.0, np.random.default_rng(100 * nb + chunks))
    m = _decode_check(codec, bk, sym, chunks)
    mean = m.payload.size / nb
    assert (mean < 2800) if chunks == FEW else (mean > 3072 or nb < 3)


@pytest.mark.parametrize("chunks", [3, 4])
@pytest.mark.parametrize("nb", BLOCK_COUNTS)
def test_decode_block_counts(codec, nb, chunks):
    if chunks == 4 and nb < 3:
        # a ragged block or two: the mean is whatever the tail makes it; either count must decode
        bk = book("hot25")
        _decode_check(codec, bk, _mixed(bk, _ragged(nb), 0.0, np.random.default_rng(nb)), None)
        return
    _count_case(codec, nb, chunks)


def _sized_case(codec):
    bk = book("hot25")
    sym, kinds = _sized_stream(bk, np.random.default_rng(3))
    m = _decode_check(codec, bk, sym, FEW)
    ww = _window_words(m.start)
    three = FEW * CHUNK_WORDS
    assert [int(ww[b]) for k in ("exact", "word_less", "bit_more", "word_more") for b in kinds[k]] == \
        [three, three - 1, three + 1, three + 1]
    assert all(three < ww[b] <= 4 * CHUNK_WORDS for b in kinds["to_4k"])
    assert all(ww[b] > 4 * CHUNK_WORDS for b in kinds["over_4k"])
    assert int(np.diff(m.start.astype(np.int64)).max()) == 25 * BLK       # the largest block this decoder can meet
    assert m.payload.size / ref_stream.nblocks(sym.size) < 2900           # the mean block: three chunks chosen


def test_decode_three_chunks_at_their_edge(codec):
    _sized_case(codec)


def _rebuild_case(codec):
    bk = book("fib57")
    sym = _stream(bk, "longest", 3 * BLK + 5, np.random.default_rng(57))
    m = _decode_check(codec, bk, sym, 0)      # 56-bit codes: the plain block loop, no chunk choice
    assert int(np.diff(m.start.astype(np.int64))[:3].min()) >= 65536


def test_decode_blocks_past_65536_bits(codec):
    _rebuild_case(codec)


@pytest.mark.parametrize("pipe", ["0", "1"])
def test_decoder_forms_agree(built_lib, pipe):
    """The same cases under HZ_DEC_PIPE=0 / 1 (a fresh process each: the library reads it once): every form
    returns the input, so the forms agree."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "pipe"], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, HZ_DEC_PIPE=pipe))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ---- pack --------------------------------------------------------------------------------------
RANGE_BLOCKS = 64                      # blocks per range up to 512 MiB (hz_internal.h range_geom)
BASE_BLOCKS = 1024 * RANGE_BLOCKS      # 256 MiB: the smallest input with a plan
SLOT_CAP_BITS = 1024 * 32              # no pack slot is larger: a larger block is cold-listed
COLD_BLOCKS = [5 * RANGE_BLOCKS,                                          # the first block of a range
               9 * RANGE_BLOCKS + 17,                                     # mid-range
               12 * RANGE_BLOCKS + RANGE_BLOCKS - 1,                      # the last block of a range
               20 * RANGE_BLOCKS + 30, 20 * RANGE_BLOCKS + 31,            # two in a row
               30 * RANGE_BLOCKS + RANGE_BLOCKS - 1, 31 * RANGE_BLOCKS,   # a range's last and the next one's first
               BASE_BLOCKS - 1]                                           # the last whole range's last block
LAST_RANGES = {63: 777, 2: 2047, 1: 5}     # blocks of the stream's last range -> symbols of its partial block


@pytest.fixture(scope="module")
def big(built_lib):
    """The longest stream (device tensor), its codebook and the host model's positions and payload,
    computed once; the prefixes' models are cut from them."""
    import torch
    from types import SimpleNamespace
    from huffman_amd import build_codebook, codebook_arrays
    from test_gpu_ranges import _zipf
    nsym = (BASE_BLOCKS + 63 - 1) * BLK + LAST_RANGES[63]
    x = _zipf(2 * nsym, 8)
    host = x.cpu().numpy()
    sym = host.view("<u2")
    rng = np.random.default_rng(12)
    for b in COLD_BLOCKS:
        sym[b * BLK:(b + 1) * BLK] = rng.integers(20000, 65536, BLK)
    x.copy_(torch.from_numpy(host))
    torch.cuda.synchronize()
    hist = np.zeros(65536, dtype=np.uint64)
    for i in range(0, nsym, 1 << 25):
        hist += np.bincount(sym[i:i + (1 << 25)], minlength=65536).astype(np.uint64)
    cb = build_codebook(hist)
    _, ln, code = codebook_arrays(cb)
    assert 17 <= int(cb.max_len) <= 25                       # HOT tables
    pos = ref_stream.positions(sym, ln, 0)
    payload = ref_stream.payload_bytes(sym, ln, code, 0, 0, pos)
    yield SimpleNamespace(x=x, sym=sym, cb=cb, ln=ln, code=code, pos=pos, payload=payload)
    del x
    torch.cuda.empty_cache()


def _prefix_model(big, nsym):
    """(payload, start[], max_bits, sub[][]) of the stream's first nsym symbols."""
    pos = big.pos[:nsym + 1]
    end = int(pos[-1])
    pay = big.payload[:4 * ((end + 31) // 32)].copy()
    if end % 8:
        pay[end // 8] &= (0xff00 >> (end % 8)) & 0xff
    pay[(end + 7) // 8:] = 0
    return (pay,) + ref_stream.index_arrays(pos, nsym)


def _boundary_chunks_differ(got, want, start, bpr):
    """Range boundaries (their first block's number) where the 16-byte chunk holding the boundary, the
    one before it or the one after it differs."""
    nb = start.size - 1
    first = np.arange(bpr, nb, bpr)
    chunk = ((start[first].astype(np.int64) >> 5) & ~3) * 4 - 16
    at = np.clip(chunk[:, None] + np.arange(48)[None, :], 0, min(got.size, want.size) - 1)
    return first[(got[at] != want[at]).any(axis=1)]


def _plan_pack(dev, x, n, nbytes, ibytes):
    """hz_hist16_ranges + hz_pack_ranges of x[:n] under the uploaded codebook into guarded buffers."""
    import torch
    rb = dev.ranges_bytes(n)
    assert rb > 0
    ranges = torch.empty(rb, dtype=torch.uint8, device="cuda")
    hist = torch.zeros(65536, dtype=torch.int64, device="cuda")
    paybuf, pay = _guarded(nbytes)
    idxbuf, idx = _guarded(ibytes)
    torch.cuda.synchronize()
    dev.hist16_ranges(x.data_ptr(), n, hist.data_ptr(), ranges.data_ptr())
    dev.pack_ranges(x.data_ptr(), n, 0, 0, pay.data_ptr(), nbytes, idx.data_ptr(), ranges.data_ptr())
    assert dev.last_pack_ranges() == 1, "the range plan did not run"
    dev.sync()
    return paybuf, pay, idxbuf, idx


@pytest.mark.parametrize("last", sorted(LAST_RANGES, reverse=True))
def test_range_pack_equals_model(big, last):
    import torch
    from huffman_amd.codec import Device
    dev = Device(0)
    nblk = BASE_BLOCKS + last
    nsym = (nblk - 1) * BLK + LAST_RANGES[last]
    n = 2 * nsym
    want_pay, start, max_bits, sub = _prefix_model(big, nsym)
    nbytes, ibytes = want_pay.size, ref_stream.index_nbytes(nsym)
    bits = np.diff(start.astype(np.int64))
    # the stream itself: cold blocks where they were planted and nowhere else but the stream's end
    assert int(bits[COLD_BLOCKS].min()) > SLOT_CAP_BITS and int(np.delete(bits, COLD_BLOCKS).max()) <= SLOT_CAP_BITS
    inside = np.ones(nblk, dtype=bool)
    inside[::RANGE_BLOCKS] = False
    inside[np.array(COLD_BLOCKS)] = False
    inside[np.array(COLD_BLOCKS) + 1] = False
    assert set(((start[:-1][inside] >> np.uint64(5)) & np.uint64(3)).tolist()) == {0, 1, 2, 3}
    dev.upload(big.cb)
    paybuf, pay, idxbuf, idx = _plan_pack(dev, big.x, n, nbytes, ibytes)
    got = pay.cpu().numpy()
    bad = _boundary_chunks_differ(got, want_pay, start, RANGE_BLOCKS)
    assert bad.size == 0, f"chunks at the range boundaries before blocks {bad[:8].tolist()} differ from the model"
    assert np.array_equal(got, want_pay), "payload: first differing byte %d" % int(np.nonzero(got != want_pay)[0][0])
    assert _guards_intact(paybuf, nbytes), "hz_pack_ranges wrote outside the payload"
    gi = idx.cpu().numpy()
    gstart = gi[:8 * (nblk + 1)].view(np.uint64)
    diff = np.nonzero(gstart != start)[0]
    assert diff.size == 0, f"start[{int(diff[0])}] = {int(gstart[diff[0]])}, model {int(start[diff[0]])} ({diff.size} entries differ)"
    assert int(gi[8 * (nblk + 1):8 * (nblk + 2)].view(np.uint64)[0]) == max_bits
    gsub = gi[8 * (nblk + 2):].view("<u2").reshape(nblk, 256)
    assert np.array_equal(gsub, sub), "sub[] differs first at %s" % np.argwhere(gsub != sub)[:1].tolist()
    assert _guards_intact(idxbuf, ibytes), "hz_pack_ranges wrote outside the index"
    obuf, out = _guarded(n)
    torch.cuda.synchronize()
    dev.decode(pay.data_ptr(), nbytes, nsym, idx.data_ptr(), out.data_ptr())
    dev.sync()
    assert torch.equal(out, big.x[:n]), "decode round trip"
    assert _guards_intact(obuf, n)


@pytest.mark.parametrize("bpr", [65, 129])
def test_range_pack_wider_ranges(built_lib, bpr):
    import torch
    from huffman_amd.codec import Device
    from test_gpu_ranges import _both, _zipf
    dev = Device(0)
    nblk = 2048 * (bpr - 1) + 5                    # more than 2048 ranges of bpr - 1 blocks: bpr blocks each
    nsym = (nblk - 1) * BLK + 333
    n = 2 * nsym
    x = _zipf(n, 9 + bpr)
    ((_, p3, i3, _, _), (_, pr, ir, took, rb)), nb, cb = _both(dev, x, 0, 0)
    assert rb > 0 and took == 1, "the range plan did not run"
    assert 17 <= int(cb.max_len) <= 25             # HOT tables
    start = ir.view(np.uint64)[:nblk + 1]
    s3 = i3.view(np.uint64)[:nblk + 1]
    diff = np.nonzero(start != s3)[0]
    assert diff.size == 0, f"start[{int(diff[0])}] = {int(start[diff[0]])}, three-pass {int(s3[diff[0]])}"
    assert np.array_equal(ir.view(np.uint8)[:nb], i3.view(np.uint8)[:nb]), "index: range plan != three-pass"
    inside = np.ones(nblk, dtype=bool)
    inside[::bpr] = False
    assert set(((start[:-1][inside] >> np.uint64(5)) & np.uint64(3)).tolist()) == {0, 1, 2, 3}
    bad = _boundary_chunks_differ(pr, p3, start, bpr)
    assert bad.size == 0, f"chunks at the range boundaries before blocks {bad[:8].tolist()} differ from the three-pass pack"
    assert np.array_equal(pr, p3), "payload: range plan != three-pass"
    end = 4 * ((int(start[nblk]) + 31) // 32)
    assert bool((pr[end:] == 0xA5).all()), "hz_pack_ranges wrote past the payload's end"
    dev.upload_decode(cb)
    pay = torch.from_numpy(pr).cuda()
    idx = torch.from_numpy(ir).cuda()
    del p3, pr
    obuf, out = _guarded(n)
    torch.cuda.synchronize()
    dev.decode(pay.data_ptr(), end, nsym, idx.data_ptr(), out.data_ptr())
    dev.sync()
    assert torch.equal(out, x[:n]), "decode round trip"
    assert _guards_intact(obuf, n)
    del x, pay, idx, out, obuf
    torch.cuda.empty_cache()


if __name__ == "__main__":
    assert sys.argv[1:] == ["pipe"], sys.argv
    from huffman_amd.pipeline import StreamCodec
    _c = StreamCodec(0)
    for _nb in BLOCK_COUNTS:
        _count_case(_c, _nb, 3)
        if _nb >= 3:
            _count_case(_c, _nb, 4)
    _sized_case(_c)
    _rebuild_case(_c)
    print("ok")
