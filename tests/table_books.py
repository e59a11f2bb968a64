"""The codebooks of the table-image checks (tests/test_table_images.py, on the CPU) and of the designed
streams (tests/test_gpu_designed_streams.py, on the GPU), by name, each with the shape it claims asserted.
A book is SimpleNamespace(name, cb, ln, code): the Codebook the uploads take, and numpy copies of
len[65536] (u8) and code[65536] (u64). Every named histogram is defined in integers; the seeded random
books (`rand00` ..) draw their shapes as tests/test_gpu_extract.py _random_stream draws its
distributions and are scaled to integer counts."""
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DESIGNED = ["fib57", "fib41", "hot25", "dense16", "dense12", "even", "fixed16"]
FULL = ["zipf21", "sq32"]                      # whole alphabets: the benchmark's table classes
SMALL = ["one", "two", "three"]
FOREIGN = ["cat4096", "zipf21cut"]             # prefix codes that are not the Huffman code of a histogram
NRANDOM = 64
RANDOM = ["rand%02d" % i for i in range(NRANDOM)]
ALL = DESIGNED + FULL + ["ragged"] + SMALL + FOREIGN + RANDOM


def _fib_hist(k):
    fib = [1, 1]
    while len(fib) < k:
        fib.append(fib[-1] + fib[-2])
    syms = (np.arange(k, dtype=np.uint32) * 257 + 3).astype(np.uint16)
    hist = np.zeros(65536, dtype=np.uint64)
    hist[syms] = fib
    return hist, syms


def _ragged_hist():
    """Counts 1000, 1001, 2000, 2001 by an integer hash of the symbol; an eighth of the symbols absent."""
    s = np.arange(65536, dtype=np.uint64)
    h = ((s * np.uint64(2654435761)) >> np.uint64(13)) & np.uint64(0xffffffff)
    counts = np.array([1000, 1001, 2000, 2001], dtype=np.uint64)[((h >> np.uint64(3)) & np.uint64(3)).astype(np.int64)]
    return np.where((h & np.uint64(7)) == 0, np.uint64(0), counts)


def _random_hist(i):
    rng = np.random.default_rng(20261020 + i)
    U = int(rng.choice([1, 2, 3, 5, 17, 255, 4096, 40000, 65536]))
    kind = int(rng.integers(0, 4))
    r = np.arange(1, U + 1, dtype=np.float64)
    if kind == 0:
        p = r ** -rng.uniform(0.5, 2.5)
    elif kind == 1:
        p = rng.uniform(0.5, 0.999) ** r
    elif kind == 2:
        p = rng.dirichlet(np.full(U, 0.05)) + 1e-12
    else:
        p = np.ones(U)
    p /= p.sum()
    vals = rng.permutation(65536)[:U]
    hist = np.zeros(65536, dtype=np.uint64)
    hist[vals] = (p * float(1 << 36)).astype(np.uint64) + np.uint64(1)   # at most 2^37 in all: codes below 56 bits
    return hist


def _foreign(ln, code):
    """A Codebook of a given prefix code (not built from a histogram: the tables take any prefix code)."""
    from huffman_amd._lib import Codebook
    cb = Codebook()
    syms = np.nonzero(ln)[0]
    cb.nsym, cb.max_len, cb.min_len = syms.size, int(ln.max()), int(ln[syms].min())
    np.ctypeslib.as_array(cb.order)[:syms.size] = syms
    np.ctypeslib.as_array(cb.len)[:] = ln
    np.ctypeslib.as_array(cb.code)[:] = code
    return cb


def caterpillars():
    """4096 caterpillars under 12-bit prefixes (tests/test_gpu.py test_lut_narrow_global_levels): lengths
    13 .. 22, so every level-1 (13-bit) prefix ending in 0 has a 9-bit-deep subtree and 9-bit global levels
    would not fit the LUT's global table."""
    ln = np.zeros(65536, np.uint8)
    code = np.zeros(65536, np.uint64)
    for g in range(4096):
        for j in range(11):
            s = g * 11 + j
            L = 13 + j if j < 10 else 22               # prefix g, then 0^j 1 (j < 10) or 0^10
            ln[s] = L
            code[s] = (g << (L - 12)) | (1 if j < 10 else 0)
    return ln, code


def _book(name):
    from huffman_amd import build_codebook, codebook_arrays
    hist = np.zeros(65536, dtype=np.uint64)
    syms = None
    if name in ("fib57", "fib41"):
        hist, syms = _fib_hist(int(name[3:]))
    elif name == "hot25":     # weights 2^i: a path of 26 leaves, the walker's escape table at its limit
        hist[np.arange(25) * 257] = [1 << i for i in range(25)]
        hist[25 * 257] = 1
    elif name == "dense16":   # 40 000 equal counts: 15 and 16 bits (DENSE, no room for output slots)
        hist[:40000] = 1
    elif name == "dense12":   # 3000 equal counts: 11 and 12 bits (DEC_DENSE)
        hist[np.arange(3000) * 19 + 7] = 1
    elif name == "even":      # every length even: an odd-bit entry never resynchronises
        hist[np.arange(10) * 1000 + 1] = [16, 16, 16, 4, 4, 4, 1, 1, 1, 1]
    elif name == "fixed16":
        hist[:] = 1
    elif name in ("zipf21", "zipf21cut", "sq32"):
        s = np.arange(65536, dtype=np.uint64)
        d = ((s & np.uint64(255)) + np.uint64(1)) * ((s >> np.uint64(8)) + np.uint64(1))
        hist = np.uint64(1 << 30) // (d * d if name == "sq32" else d) + np.uint64(1)
    elif name == "ragged":
        hist = _ragged_hist()
    elif name == "one":
        hist[0x1234] = 7
    elif name == "two":
        hist[[0x00ff, 0x8001]] = [3, 5]
    elif name == "three":
        hist[[5, 0x8005, 0xfffe]] = [1, 1, 2]
    elif name == "cat4096":
        pass
    elif name in RANDOM:
        hist = _random_hist(int(name[4:]))
    else:
        raise ValueError(name)
    if name == "cat4096":
        ln, code = caterpillars()
        cb = _foreign(ln, code)
    else:
        cb = build_codebook(hist)
        order, ln, code = codebook_arrays(cb)
        if name == "zipf21cut":   # the 100 rarest symbols leave: a foreign, incomplete prefix code
            ln[order[:100]] = 0
            code[order[:100]] = 0
            cb = _foreign(ln, code)
    used = ln[ln > 0]
    lo, hi = int(used.min()), int(used.max())
    assert (cb.min_len, cb.max_len, cb.nsym) == (lo, hi, used.size)
    if name == "fib57":
        assert (lo, hi) == (1, 56) and sorted(ln[syms[:8]].tolist()) == [50, 51, 52, 53, 54, 55, 56, 56]
    elif name == "fib41":
        assert (lo, hi) == (1, 40) and int(ln[syms[:8]].min()) >= 33
    elif name == "hot25":
        assert (lo, hi) == (1, 25) and used.size == 26
    elif name == "dense16":
        assert (lo, hi) == (15, 16) and used.size == 40000
    elif name == "dense12":
        assert (lo, hi) == (11, 12) and used.size == 3000
    elif name == "even":
        assert ln[np.arange(10) * 1000 + 1].tolist() == [2, 2, 2, 4, 4, 4, 6, 6, 6, 6]
    elif name == "fixed16":
        assert (lo, hi) == (16, 16) and used.size == 65536
    elif name == "zipf21":
        assert (lo, hi) == (5, 21) and used.size == 65536
    elif name == "zipf21cut":
        assert (lo, hi) == (5, 21) and used.size == 65436
    elif name == "sq32":
        assert (lo, hi) == (1, 32) and used.size == 65536
    elif name == "ragged":
        assert 15 <= lo and hi <= 17 and 56000 < used.size < 58700
    elif name == "cat4096":
        assert (lo, hi) == (13, 22) and used.size == 4096 * 11
    elif name == "one":
        assert (lo, hi) == (1, 1) and used.size == 1 and int(code[0x1234]) == 0
    elif name == "two":
        assert (lo, hi) == (1, 1) and used.size == 2
    elif name == "three":
        assert (lo, hi) == (1, 2) and used.size == 3
    return SimpleNamespace(name=name, cb=cb, ln=ln, code=code)


_books = {}


def book(name):
    if name not in _books:
        _books[name] = _book(name)
    return _books[name]
