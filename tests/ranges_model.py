"""A plain host model of the cooperative walk of one block (hz_decode_ranges, k_ranges_decode's
coop_starts; DESIGN.md "A batch of ranges"), with the kernel's own segment rule: the cut into 64
segments, the walk from guessed entries, the fix-up rounds and the select of the 256 chain starts.
numpy and Python integers only; the code lengths come from a dictionary of the prefix code, not
from any device table. tests/test_ranges_model.py compares it with ref_stream.positions."""
import numpy as np

LANES = 64
MAX_ROUNDS = 64
CHAIN = 8
CHAINS = 256
DEAD = 0xffffffff     # exit of a path that met an invalid code


def segment_bits(n):
    """g: bits per lane, a multiple of 32 (a lane owns whole bitmap words); 64 g >= n."""
    return 32 * (((n + 63) // 64 + 31) // 32)


class Lengths:
    """length_at(bit) for a payload under the prefix code (ln, code): 0 where no code matches."""

    def __init__(self, payload, ln, code):
        data = bytes(np.asarray(payload, dtype=np.uint8).tobytes()) + bytes(16)   # zeros past the payload
        self.big = int.from_bytes(data, "big")
        self.nbits = 8 * len(data)
        ln = np.asarray(ln)
        syms = np.nonzero(ln)[0]
        self.codes = {(int(ln[s]), int(code[s])) for s in syms}
        self.lens = sorted({int(ln[s]) for s in syms})
        self.memo = {}

    def at(self, bit):
        L = self.memo.get(bit)
        if L is None:
            w = (self.big >> (self.nbits - bit - 64)) & ((1 << 64) - 1)
            L = 0
            for k in self.lens:
                if (k, w >> (64 - k)) in self.codes:
                    L = k
                    break
            self.memo[bit] = L
        return L


def coop_walk(length_at, n):
    """Steps 1-3 on a block of n bits; length_at(p): the code length at block bit p.
    Returns (bitmap: bool[n], the lanes' exits, the fix-up rounds needed, stuck)."""
    g = segment_bits(n)
    bm = np.zeros(max(n, 1), dtype=bool)
    ss = [i * g for i in range(LANES)]
    se = [min(s + g, n) for s in ss]
    entry = [min(s, n) for s in ss]      # lane 0 enters at bit 0, which is true; lane i guesses i g
    ex = [0] * LANES
    for i in range(LANES):
        p = entry[i]
        while p < se[i]:
            bm[p] = True
            L = length_at(p)
            if L == 0:
                p = DEAD
                break
            p += L
        ex[i] = p
    rounds, stuck = 0, False
    while True:
        te = [0] + ex[:-1]               # taken across the lanes before any of them moves
        dirty = [te[i] != entry[i] for i in range(LANES)]
        if not any(dirty):
            break
        if rounds == MAX_ROUNDS:
            stuck = True
            break
        rounds += 1
        for i in range(LANES):
            if not dirty[i]:
                continue
            entry[i] = te[i]
            if te[i] >= se[i]:           # the true path skips the segment
                bm[ss[i]:max(se[i], ss[i])] = False
                ex[i] = te[i]
                continue
            bm[ss[i]:te[i]] = False
            p = te[i]
            while True:
                if p >= se[i]:
                    ex[i] = p
                    break
                if bm[p]:                # on the old path: its exit stands
                    break
                bm[p] = True
                L = length_at(p)
                if L == 0:
                    bm[p + 1:se[i]] = False
                    ex[i] = DEAD
                    break
                bm[p + 1:min(p + L, se[i])] = False
                p += L
    return bm[:n], ex, rounds, stuck


def chain_starts(bm, cnt, n):
    """Step 4: None unless the bitmap holds cnt starts; else the 256 chain starts (every 8th start by
    rank; chains past the stream's end are idle at n)."""
    pos = np.nonzero(bm)[0]
    if pos.size != cnt:
        return None
    out = np.full(CHAINS, n, dtype=np.int64)
    k = (cnt + CHAIN - 1) // CHAIN
    out[:k] = pos[::CHAIN]
    return out


def block_starts(payload, ln, code, s0, s1, cnt):
    """The whole of steps 1-4 for the block at stream bits [s0, s1) with cnt codewords:
    (bitmap, chain starts or None when a check fails, rounds)."""
    lens = Lengths(payload, ln, code)
    n = s1 - s0
    bm, ex, rounds, stuck = coop_walk(lambda p: lens.at(s0 + p), n)
    ok = not stuck and ex[-1] == n
    return bm, (chain_starts(bm, cnt, n) if ok else None), rounds
