"""The cooperative walk of one block (hz_decode_ranges), on the CPU: tests/ranges_model.py restates
the kernel's cut, walk, fix-up rounds and select in numpy; here its boundary bitmap must equal the
codeword positions of the plain stream model (tests/ref_stream.py) for every designed book, and its
round counts must show both ends: a code whose lengths share a factor hands the true path from lane
to lane (many rounds), a Zipf book resynchronises at once (few)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib  # noqa: E402
import ranges_model  # noqa: E402
import ref_stream  # noqa: E402
from table_books import DESIGNED, book  # noqa: E402

BLK = 2048


def _blocks(sym, ln, code, start_bit, blocks):
    """(bitmap, chain starts, rounds, true starts, true chain starts) of the given blocks of a stream."""
    m = ref_stream.model(sym, ln, code, start_bit, 0)
    out = []
    for b in blocks:
        lo, hi = b * BLK, min((b + 1) * BLK, m.nsym)
        s0, s1 = int(m.pos[lo]), int(m.pos[hi])
        bm, cs, rounds = ranges_model.block_starts(m.payload, ln, code, s0, s1, hi - lo)
        truth = (m.pos[lo:hi] - np.uint64(s0)).astype(np.int64)
        chains = np.full(256, s1 - s0, dtype=np.int64)
        chains[:(hi - lo + 7) // 8] = truth[::8]
        out.append((bm, cs, rounds, truth, chains))
    return out


def _assert_exact(res, what):
    for bm, cs, rounds, truth, chains in res:
        assert np.array_equal(np.nonzero(bm)[0], truth), what
        assert cs is not None and np.array_equal(cs, chains), what
        assert rounds <= ranges_model.MAX_ROUNDS, what


def tri36():
    """Seven 3-bit and eight 6-bit codes: every length a multiple of 3."""
    from huffman_amd import build_codebook, codebook_arrays
    hist = np.zeros(65536, dtype=np.uint64)
    syms = (np.arange(15, dtype=np.uint32) * 4099 + 11).astype(np.uint16)
    hist[syms[:7]] = 8
    hist[syms[7:]] = 1
    cb = build_codebook(hist)
    _, ln, code = codebook_arrays(cb)
    assert sorted(ln[syms].tolist()) == [3] * 7 + [6] * 8
    return cb, ln, code, syms


def tri36_stream(nsym, seed=36):
    cb, ln, code, syms = tri36()
    rng = np.random.default_rng(seed)
    p = np.array([8] * 7 + [1] * 8, dtype=np.float64) / 64
    return cb, ln, code, np.ascontiguousarray(syms[rng.choice(15, nsym, p=p)], dtype="<u2")


@pytest.mark.parametrize("start_bit", [0, 5, 45])
@pytest.mark.parametrize("name", DESIGNED)
def test_bitmap_equals_positions(name, start_bit):
    bk = book(name)
    alphabet = np.nonzero(bk.ln)[0].astype(np.uint16)
    rng = np.random.default_rng(1000 + start_bit)
    sym = np.ascontiguousarray(alphabet[rng.integers(0, alphabet.size, BLK + 19)], dtype="<u2")
    _assert_exact(_blocks(sym, bk.ln, bk.code, start_bit, [0, 1]), (name, start_bit))   # a whole block, a ragged tail


def test_segment_rule():
    for n in (0, 1, 63, 64, 65, 2047, 2048, 2049, 6912, 20000, 65536, 2048 * 56):
        g = ranges_model.segment_bits(n)
        assert g % 32 == 0 and 64 * g >= n and (n == 0 or 64 * (g - 32) < n + 64 * 31)
    assert ranges_model.segment_bits(6912) == 128


def test_tri36_hands_the_path_from_lane_to_lane():
    _, ln, code, sym = tri36_stream(BLK + 5)
    res = _blocks(sym, ln, code, 0, [0, 1])
    _assert_exact(res, "tri36")
    assert res[0][2] >= 8, res[0][2]


def test_zipf_resynchronises_at_once():
    from huffman_amd import build_codebook, codebook_arrays
    data = oracle_lib.generate(8 * 2 * BLK, kind=1, seed=7, alpha=1.1)
    sym = np.ascontiguousarray(np.frombuffer(data.tobytes(), dtype="<u2"))
    cb = build_codebook(np.bincount(sym, minlength=65536).astype(np.uint64))
    _, ln, code = codebook_arrays(cb)
    res = _blocks(sym, ln, code, 0, range(8))
    _assert_exact(res, "zipf")
    assert max(r[2] for r in res) <= 4, [r[2] for r in res]
