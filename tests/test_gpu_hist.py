"""hz_hist16 directly, against np.bincount of the host copy of the same bytes (and, where a repeated
pattern builds the input, against the exact counts that follow from the pattern).

The kernel counts in 16-bit LDS halves, two symbols 2k, 2k + 1 per 32-bit word, and repairs a half
that wraps through the value the LDS atomic returned (hz_hist.hip hist_fix): the high half's wrap,
the low half's carry into the high half, and the undo of a carry that wrapped a high half sitting
at 0xffff. An error there is +-65 536 in one bin, which can leave the codebook -- and with it every
file-level comparison -- unchanged; so the inputs here are designed to put both halves of one word at
0xffff, in one workgroup and in every workgroup of the full grid.

Tolerance: none -- integer counts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64
NBINS = 65536
A, B = 0x1234, 0x1235      # the low and the high half of one LDS word
PIECE = 8192               # symbols per 16 KiB piece: one vector per lane of a 1024-thread workgroup


@pytest.fixture(scope="module")
def codec(built_lib):
    from huffman_amd.pipeline import StreamCodec
    return StreamCodec(0)   # its stream is torch's current stream: torch's fills and the library's kernels are ordered


def _hist_buffer(prefill=None):
    """The 65 536 x u64 histogram between two 64-byte guards of 0xA5; prefill: a uint64 array, else 0xA5 bytes
    (accumulate = 0 must overwrite them)."""
    import torch
    buf = torch.full((GUARD + 8 * NBINS + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    if prefill is not None:
        buf[GUARD:GUARD + 8 * NBINS] = torch.from_numpy(prefill.view(np.uint8).copy()).cuda()
    return buf


def _read(codec, buf):
    codec.sync()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + 8 * NBINS:] == 0xA5).all(), "histogram guards"
    return host[GUARD:GUARD + 8 * NBINS].view(np.uint64).copy()


def _hist16(codec, x, n=None, accumulate=False, buf=None):
    """hz_hist16 of the first n bytes of the device byte tensor x -> host uint64 counts."""
    buf = _hist_buffer() if buf is None else buf
    n = x.numel() if n is None else n
    codec.dev.hist16(x.data_ptr(), n, buf.data_ptr() + GUARD, accumulate)
    return _read(codec, buf)


def _bincount(host_bytes, n):
    """The reference: np.bincount of the u16 symbols of the first n bytes (an odd n ignores its last byte)."""
    sym = np.ascontiguousarray(host_bytes[:2 * (n // 2)]).view("<u2")
    h = np.zeros(NBINS, dtype=np.uint64)
    for i in range(0, sym.size, 1 << 25):     # in slices: bincount widens its input to 8 bytes per symbol
        h += np.bincount(sym[i:i + (1 << 25)], minlength=NBINS).astype(np.uint64)
    return h


def _diff(got, want):
    bad = np.nonzero(got != want)[0]
    return [(hex(int(s)), int(got[s]), int(want[s])) for s in bad[:8]]


def _assert_equal(got, want):
    assert np.array_equal(got, want), f"(bin, got, want): {_diff(got, want)}"


# ---- small edges --------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 2], ids=["aligned", "scalar"])
@pytest.mark.parametrize("n", [0, 1, 2, 15, 16, 17, 4097, 2 * 65536 + 6])
def test_small_edges(codec, n, offset):
    """Byte counts around one vector, one workgroup's step and one workgroup's share; an odd n ignores its
    trailing byte; a pointer 2 bytes off 16-byte alignment takes the scalar kernel. The symbols come from
    few values (pairs 2k, 2k + 1 among them), so bins collect many adds."""
    import torch
    rng = np.random.default_rng(n)
    vals = np.array([0, 1, 2, 0x00ff, 0x0100, 0xfffe, 0xffff, A, B, 0x8000], dtype="<u2")
    host = vals[rng.integers(0, vals.size, (offset + n + 48) // 2 + 1)].view(np.uint8)
    x = torch.from_numpy(host).cuda()
    view = x[offset:]
    assert view.data_ptr() % 16 == offset
    got = _hist16(codec, view, n)
    want = _bincount(host[offset:], n)
    assert int(want.sum()) == n // 2
    _assert_equal(got, want)


# ---- one workgroup: a half wraps exactly at the last add -------------------------------------------
@pytest.mark.parametrize("offset", [0, 2], ids=["aligned", "scalar"])
@pytest.mark.parametrize("s", [A, B], ids=["even", "odd"])
def test_one_workgroup_wraps_at_the_last_add(codec, s, offset):
    """65 536 copies of one symbol are one workgroup's share: its 16-bit half wraps exactly at the last add,
    so the LDS image is zero and the whole count reaches the histogram through hist_fix -- for an even
    symbol with the carry taken back out of its odd neighbour."""
    import torch
    host = np.full(65536 + 8, s, dtype="<u2").view(np.uint8)
    x = torch.from_numpy(host).cuda()
    got = _hist16(codec, x[offset:], 2 * 65536)
    want = np.zeros(NBINS, dtype=np.uint64)
    want[s] = 65536
    _assert_equal(want, _bincount(host[offset:], 2 * 65536))
    _assert_equal(got, want)


# ---- both halves of one LDS word, in every workgroup ---------------------------------------------------
def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _lockstep(ncu, extra=0):
    """Every 16-byte vector A,B,A,B,A,B,A,B: both halves of the word cross 0xffff within a lane's drift
    of each other, four times per workgroup, however the work is split. 4 * 65 536 symbols per CU."""
    import torch
    nsym = 4 * 65536 * ncu + extra
    x = torch.empty(nsym, dtype=torch.int16, device="cuda")
    x[0::2] = A
    x[1::2] = B
    return x.view(torch.uint8)


def _parked(ncu):
    """Per workgroup: exactly 65 535 B, then filler from other LDS words, then more than 65 536 A, so the
    high half sits at 0xffff when the low half carries: the carry wraps it, and the undo takes the 65 536
    back out of B's count.

    This mirrors launch_hist16 (hz_hist.hip): for 4 * 65 536 * CUs symbols the grid is one workgroup per
    CU, and workgroup g sweeps the 16 KiB pieces g + k * grid, k = 0 .. 31, in order. So piece p holds what
    its k = p // grid says: k 0..7 B (the last symbol of piece k = 7 a filler: 8 * 8192 - 1 = 65 535),
    k 8..22 filler, k 23..31 A (9 * 8192 = 73 728). A workgroup has 32 pieces at this size, so 15 of them
    are filler; the carry comes with the 65 536th A, 23 pieces after the last B."""
    import torch
    grid = ncu
    k = torch.arange(32 * grid * PIECE, dtype=torch.int32, device="cuda")
    filler = (0x4000 + (k % 4096)).to(torch.int16)
    k //= PIECE * grid
    x = torch.where(k < 8, torch.tensor(B, dtype=torch.int16, device="cuda"),
                    torch.where(k >= 23, torch.tensor(A, dtype=torch.int16, device="cuda"), filler))
    last = x.view(-1, PIECE)[7 * grid:8 * grid]
    last[:, PIECE - 1] = filler.view(-1, PIECE)[7 * grid:8 * grid, PIECE - 1]
    return x.view(torch.uint8)


@pytest.fixture(scope="module")
def lockstep(codec):
    import torch
    ncu = _cus()
    buf = _lockstep(ncu, extra=8)                   # 16 bytes more: room for the unaligned view
    n = 2 * 4 * 65536 * ncu
    host = buf.cpu().numpy()
    ref = {0: _bincount(host, n), 2: _bincount(host[2:], n)}
    exact = np.zeros(NBINS, dtype=np.uint64)
    exact[A] = exact[B] = n // 4
    _assert_equal(ref[0], exact)
    _assert_equal(ref[2], exact)
    yield buf, n, exact
    del buf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("offset", [0, 2], ids=["aligned", "scalar"])
def test_both_halves_lockstep(codec, lockstep, offset):
    buf, n, exact = lockstep
    view = buf[offset:]
    assert view.data_ptr() % 16 == offset
    _assert_equal(_hist16(codec, view, n), exact)


def test_both_halves_parked(codec):
    import torch
    ncu = _cus()
    x = _parked(ncu)
    n = x.numel()
    assert n == 2 * 4 * 65536 * ncu and x.data_ptr() % 16 == 0
    got = _hist16(codec, x)
    want = _bincount(x.cpu().numpy(), n)
    # what the layout says, per workgroup: 65 535 B, 73 728 A, 15 * 8192 + 1 filler symbols over 4096 values
    assert int(want[B]) == 65535 * ncu and int(want[A]) == 73728 * ncu
    assert int(want[0x4000:0x5000].sum()) == (15 * PIECE + 1) * ncu and np.count_nonzero(want) == 4098
    _assert_equal(got, want)
    del x
    torch.cuda.empty_cache()


# ---- accumulate -----------------------------------------------------------------------------------------
def _prefill():
    h = np.zeros(NBINS, dtype=np.uint64)
    h[A] = (1 << 32) - 3
    h[B] = (1 << 40) + 5
    h[7] = 11
    return h


def test_accumulate_adds_and_overwrite_replaces(codec, lockstep):
    """accumulate = 1 twice over a pre-filled histogram: the pre-fill plus twice the counts (u64 bins: past
    2^32 and 2^40); accumulate = 0 over the same pre-fill: the counts alone."""
    buf, n, exact = lockstep
    pre = _prefill()
    hb = _hist_buffer(pre)
    _assert_equal(_hist16(codec, buf, n, accumulate=True, buf=hb), pre + exact)
    _assert_equal(_hist16(codec, buf, n, accumulate=True, buf=hb), pre + 2 * exact)
    _assert_equal(_hist16(codec, buf, n, accumulate=False, buf=_hist_buffer(pre)), exact)


@pytest.mark.parametrize("offset", [0, 2], ids=["aligned", "scalar"])
def test_accumulate_small(codec, offset):
    """The same on one workgroup's wrap (65 536 copies of A and of B, interleaved) and a ragged tail."""
    import torch
    n = 2 * (2 * 65536 + 5)
    sym = np.tile(np.array([A, B], dtype="<u2"), 65536 + 8)
    sym[2 * 65536:] = 9
    host = sym.view(np.uint8)
    x = torch.from_numpy(host).cuda()
    want = _bincount(host[offset:], n)
    assert int(want.sum()) == n // 2 and int(want[B]) == 65536 and int(want[A]) == 65536 - offset // 2
    pre = _prefill()
    hb = _hist_buffer(pre)
    _assert_equal(_hist16(codec, x[offset:], n, accumulate=True, buf=hb), pre + want)
    _assert_equal(_hist16(codec, x[offset:], n, accumulate=True, buf=hb), pre + 2 * want)
    _assert_equal(_hist16(codec, x[offset:], n, accumulate=False, buf=_hist_buffer(pre)), want)
