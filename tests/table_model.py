"""What each kernel does with a device table image, restated in numpy from the documented entry formats
(the comments of huffman_amd/csrc/hz_internal.h and hz_codebook.cpp) -- the plain reference that
tests/test_table_images.py holds the images of tests/table_probe.cpp against. Every resolver takes
WINDOWS: a codeword followed by arbitrary suffix bits, MSB first, as u64 (bit 63 = the code's first bit)
or as the u32 of its top half, for all symbols of a book at once. numpy only; nothing here reads the
builders' code or calls the library."""
import numpy as np

U64 = np.uint64
NSYM = 65536

# hz_internal.h
K_LDS_BYTES = 160 * 1024
K_LUT_GLOBAL = 65536
K_LUT_MAX_L2 = (1 << 21) - K_LUT_GLOBAL
K_DEC_LUT_MAX_K1 = 13
K_DEC_LEVEL_BITS = 12
K_DEC_MAX_WAVES = 16
K_DEC_MIN_WAVES = 8
K_DEC_MIN_LDS_WORDS = 32
K_WALK_K = 17
K_WALK_MAX_LEN = 25
K_CHAIN_ESC_MAX_BITS = 25
K_HOT_MAX_LEN = 25
K_NARROW_MAX_LEN = 26
K_BLOCK_SYMS = 2048
K_CHAIN_SYMS = 8
ENC_DENSE, ENC_HOT, ENC_WIDE, ENC_FIXED16 = 0, 1, 2, 3
DEC_DENSE, DEC_LUT, DEC_FIXED16 = 0, 1, 2
CONSTS = {"kLdsBytes": K_LDS_BYTES, "kLutGlobal": K_LUT_GLOBAL, "kLutMaxL2": K_LUT_MAX_L2,
          "kDecLutMaxK1": K_DEC_LUT_MAX_K1, "kDecLevelBits": K_DEC_LEVEL_BITS, "kDecMaxWaves": K_DEC_MAX_WAVES,
          "kDecMinLdsWords": K_DEC_MIN_LDS_WORDS, "kWalkK": K_WALK_K, "kWalkMaxLen": K_WALK_MAX_LEN,
          "kChainEscMaxBits": K_CHAIN_ESC_MAX_BITS, "kHotMaxLen": K_HOT_MAX_LEN, "kNarrowMaxLen": K_NARROW_MAX_LEN,
          "kBlockSyms": K_BLOCK_SYMS, "kChainSyms": K_CHAIN_SYMS}    # as the probe reports them
HOT_MASKS = [0x8000, 0xffff, 0x8080, 0xc0c0, 0x80ff, 0xff80, 0xa0a0, 0xf0f0,
             0x8888, 0xcccc, 0xaaaa, 0x8001, 0xff00, 0x80c0, 0xe0e0, 0x9999]

# Global hops of the pipelined decoders. dec_wave_pipe2 (hz_decode.hip) and dec_wave_chain under
# k_chain_decode (hz_chain.hip) walk a codeword with dec_pipe_ldsn -- level 1, at most ONE LDS hop -- and
# then issue exactly ONE gather from the global table (raw_buffer_load at PipeLane::gi); finish() takes
# max(entry after LDS, gathered entry) as the leaf, with no loop and no fall-back. The launchers send a
# codebook there only when pipelined() holds (decode_dispatch: max_len <= 32 and max_len <= k + level
# bits; chain_pipelined: max_len <= chain_k + chain_level_bits); every other LUT codebook takes the
# looping forms (dec_group, k_chain_decode_serial through dec_lookup).
PIPE_LDS_HOPS = 1
PIPE_GLOBAL_HOPS = 1


def pipelined(max_len, k1, lvl):
    return max_len <= 32 and max_len <= k1 + lvl


class ModelError(AssertionError):
    pass


def _fail(what, idx, syms=None):
    """Names the first offending window's symbol."""
    idx = np.atleast_1d(idx)
    i = int(np.nonzero(idx)[0][0]) if idx.dtype == bool else int(idx[0])
    s = int(syms[i]) if syms is not None else i
    raise ModelError("%s (symbol 0x%04x, window %d)" % (what, s, i))


# ---- windows ------------------------------------------------------------------------------------
def windows64(ln, code, syms, suffix):
    """The codes of `syms`, each followed by the bits of `suffix` (u64 per symbol or one value, MSB first)."""
    L = ln[syms].astype(U64)
    c = code[syms].astype(U64)
    suf = np.broadcast_to(np.asarray(suffix, dtype=U64), L.shape)
    return (c << (U64(64) - L)) | (suf >> L)          # 1 <= L <= 56: no shift by 64


def top32(win64):
    return (win64 >> U64(32)).astype(np.uint32)


def prefix_bits(ln, code, s):
    """The code of symbol s, left aligned in a u64 (the bits of a successor codeword)."""
    return U64(int(code[s]) << (64 - int(ln[s])))


def _ubfe(W, e):
    """v_bfe_u32(W, e, e >> 5): offset e[4:0], width e[9:5]."""
    off = (e & np.uint32(31)).astype(U64)
    width = ((e >> np.uint32(5)) & np.uint32(31)).astype(U64)
    return (((W.astype(U64) >> off) & ((U64(1) << width) - U64(1)))).astype(np.int64)


def _leaf(e):
    return (e >> np.uint32(31)) == 1


def _leaf_len(e):
    return ((e >> np.uint32(24)) & np.uint32(63)).astype(np.int64)


def _leaf_sym(e):
    return ((e >> np.uint32(8)) & np.uint32(0xffff)).astype(np.int64)


def _lut_at(img, l2, idx, what, syms):
    """lut_at: raw index < kLutGlobal in the LDS image, else the global table; in bounds."""
    lds = idx < K_LUT_GLOBAL
    bad = (idx < 0) | (lds & (idx >= img.size)) | (~lds & (idx - K_LUT_GLOBAL >= l2.size))
    if bad.any():
        _fail("%s: index outside its table" % what, bad, syms)
    out = np.empty(idx.shape, np.uint32)
    out[lds] = img[idx[lds]]
    out[~lds] = l2[idx[~lds] - K_LUT_GLOBAL]
    return out


# ---- decode -------------------------------------------------------------------------------------
def lut64(img, l2, k1, win64, syms=None):
    """dec_lookup<DEC_LUT> (hz_decode_device.h; deep_len of hz_chain.hip is the same walk): level 1 by the
    top k1 bits, then links by nb with the depth D tracked by the caller. -> (sym, len, hops)."""
    e = img[(win64 >> U64(64 - k1)).astype(np.int64)]
    D = np.full(win64.shape, k1, np.int64)
    hops = np.zeros(win64.shape, np.int64)
    for _ in range(64):
        go = ~_leaf(e)
        if not go.any():
            return _leaf_sym(e), _leaf_len(e), hops
        nb = ((e[go] >> np.uint32(5)) & np.uint32(15)).astype(np.int64)
        if (nb == 0).any() or (D[go] + nb > 64).any():
            _fail("lut64: a link of no index bits, or past 64 bits", go, syms)
        bits = ((win64[go] << D[go].astype(U64)) >> (64 - nb).astype(U64)).astype(np.int64)
        idx = (e[go] >> np.uint32(10)).astype(np.int64) + bits
        e = e.copy()
        e[go] = _lut_at(img, l2, idx, "lut64", None if syms is None else syms[go])
        D[go] += nb
        hops[go] += 1
    _fail("lut64: no leaf after 64 links", ~_leaf(e), syms)


def lut32(img, l2, k1, W, syms=None):
    """The 32-bit form: dec_pipe_ldsn (hz_decode_device.h; dec_pipe_lds / dec_pipe_lds2 of hz_decode.hip and
    lut_len2 of hz_index.hip alike) then the global step. Level 1; at most one LDS hop, taken when
    lut_lds_link holds; then global hops, each at (e >> 10) + ubfe(W, e, e >> 5), with no depth kept.
    -> (sym, len, lds_hops, global_hops). The pipelined decoders take one global hop only
    (PIPE_GLOBAL_HOPS): the caller asserts the count where they run."""
    e = img[(W >> np.uint32(32 - k1)).astype(np.int64)]
    h = e < np.uint32(K_LUT_GLOBAL << 10)               # lut_lds_link: false for leaves (bit 31)
    lds_hops = h.astype(np.int64)
    if h.any():
        idx = (e[h] >> np.uint32(10)).astype(np.int64) + _ubfe(W[h], e[h])
        if (idx >= img.size).any():
            _fail("lut32: LDS hop outside the LDS image", h, syms)
        e = e.copy()
        e[h] = img[idx]
    ghops = np.zeros(W.shape, np.int64)
    for _ in range(32):
        go = ~_leaf(e)
        if not go.any():
            return _leaf_sym(e), _leaf_len(e), lds_hops, ghops
        idx = (e[go] >> np.uint32(10)).astype(np.int64) + _ubfe(W[go], e[go]) - K_LUT_GLOBAL   # lut_gnext32
        bad = (idx < 0) | (idx >= l2.size)
        if bad.any():
            _fail("lut32: global hop outside l2 (a second LDS link reads as a global one)", go, syms)
        e = e.copy()
        e[go] = l2[idx]
        ghops[go] += 1
    _fail("lut32: no leaf after 32 global hops", ~_leaf(e), syms)


def dense_decode(img, k, min_len, win64):
    """dec_lookup<DEC_DENSE>: u16 symbol per k-bit window, then 2-bit (L - min_len) per window."""
    idx = (win64 >> U64(64 - k)).astype(np.int64)
    sym = img.view("<u2")[idx].astype(np.int64)
    lw = img[(1 << k) // 2 + (idx >> 4)]
    return sym, min_len + ((lw >> ((idx & 15) * 2).astype(np.uint32)) & np.uint32(3)).astype(np.int64)


def fixed16_decode(img, win64):
    """dec_lookup<DEC_FIXED16>: u16 symbol per 16-bit code."""
    return img.view("<u2")[(win64 >> U64(48)).astype(np.int64)].astype(np.int64), np.full(win64.shape, 16, np.int64)


# ---- encode -------------------------------------------------------------------------------------
def hot_slot(s, m):
    return np.where(s & 0x8000, s ^ m, s)


def hot_word(slot):
    return slot ^ ((slot >> 8) & 0x3f)


def hot_lookup(img, esc, mask, syms):
    """hot_issue / hot_finish (hz_pack.hip): the slot by hot_slot and hot_word; a hit when the slot's tag
    (bit 31) equals the symbol's bit 15; otherwise the escape word at the same hot_word. -> (len, code, hit).
    The register entry's length is its 5-bit field at bit 26 (ent_len), its code the 26 bits below."""
    s = syms.astype(np.int64)
    w = hot_word(hot_slot(s, mask) & 0x7fff)
    x = img[w]
    hit = ((x ^ (s << 16).astype(np.uint32)) >> np.uint32(31)) == 0
    e = np.where(hit, x, esc[w])
    return ((e >> np.uint32(26)) & np.uint32(31)).astype(np.int64), (e & np.uint32((1 << 26) - 1)).astype(np.int64), hit


def hot_owner(ln, mask):
    """Who owns each HOT slot, by the documented rule alone: of the pair (slot, slot ^ mask) the symbol
    whose code fits 25 bits and is shorter; a tie goes to the symbol below 0x8000. -> owns[65536] (bool)."""
    a = np.arange(32768)
    b = a ^ (mask & 0x7fff) ^ 0x8000
    la, lb = ln[a].astype(np.int64), ln[b].astype(np.int64)
    ea, eb = (la > 0) & (la <= K_HOT_MAX_LEN), (lb > 0) & (lb <= K_HOT_MAX_LEN)
    a_owns = ea & (~eb | (la <= lb))
    b_owns = eb & ~a_owns
    owns = np.zeros(NSYM, bool)
    owns[a[a_owns]] = True
    owns[b[b_owns]] = True
    return owns


def hot_miss_mass(ln, mask):
    """Escaped probability mass of a pairing mask in units of 2^-25: the lighter of each pair (weights
    2^-L of the codes that fit a slot)."""
    L = ln.astype(np.int64)
    w = np.where((L > 0) & (L <= K_HOT_MAX_LEN), np.int64(1) << np.clip(K_HOT_MAX_LEN - L, 0, 62), 0)
    a = np.arange(32768)
    return int(np.minimum(w[a], w[a ^ mask]).sum())


def dense_encode(img, syms):
    """pack_lookup<ENC_DENSE> (hz_pack.hip): the 17-bit entry at bit 17 s, (code << 1 | 1) << (16 - L)."""
    bit = syms.astype(np.int64) * 17
    w = bit >> 5
    two = (img[w + 1].astype(U64) << U64(32)) | img[w].astype(U64)
    f = ((two >> (bit & 31).astype(U64)) & U64(0x1ffff)).astype(np.int64)
    low = np.maximum(f & -f, 1)                          # the sentinel: the lowest set bit, 2^ctz <= 2^16
    ctz = np.round(np.log2(low.astype(np.float64))).astype(np.int64)
    L = np.where(f != 0, 16 - ctz, 0)
    return L, np.where(f != 0, f >> np.maximum(17 - L, 0), 0)


def wide_encode(img64, syms):
    """pack_lookup<ENC_WIDE>: len << 56 | code."""
    e = img64[syms.astype(np.int64)]
    return (e >> U64(56)).astype(np.int64), e & U64((1 << 56) - 1)


def len8_lookup(img, syms):
    """The count pass's length table: u8 at len8_index(s)."""
    s = syms.astype(np.int64)
    return img.view(np.uint8)[s ^ (((s >> 8) & 0x3f) << 2)].astype(np.int64)


def lenpair_lookup(img, syms):
    """k_range_dot's table: u16 per histogram word in hist_word order, len[2 s'] | len[2 s' + 1] << 8."""
    s = syms.astype(np.int64)
    w = (s >> 1) ^ (((s >> 8) * 13) & 0x3f)
    return ((img.view("<u2")[w].astype(np.int64) >> (8 * (s & 1))) & 0xff)


# ---- walkers ------------------------------------------------------------------------------------
def idx_walk(img, esc, k, m, bias, W):
    """k_idx_walk (hz_index.hip): the nibble of the top k window bits (the high nibble for odd windows) plus
    bias, or 0 and then esc[W >> (32 - m)]. -> (len, escaped)."""
    t = img.view(np.uint8)
    byte = t[(W >> np.uint32(33 - k)).astype(np.int64)]
    nib = ((byte >> ((W >> np.uint32(30 - k)) & np.uint32(4)).astype(np.uint8)) & np.uint8(15)).astype(np.int64)
    e8 = esc.view(np.uint8)
    ei = (W >> np.uint32(32 - m)).astype(np.int64)
    esc_len = e8[np.minimum(ei, e8.size - 1)].astype(np.int64)
    out_of_table = (nib == 0) & (ei >= e8.size)
    if out_of_table.any():
        _fail("idx_walk: escape outside the escape table", out_of_table)
    return np.where(nib != 0, nib + bias, esc_len), nib == 0


def chain_walk(w8, k8, esc, m, W):
    """k_chain_walk (hz_chain.hip): the byte table by the top k8 bits, then chain_esc by the top m bits.
    -> (len, escaped, deep): deep where the escape table reads 0 (k_chain_walk<DEEP> then takes deep_len,
    the decode LUT's 64-bit form)."""
    t = w8.view(np.uint8)
    e = t[(W >> np.uint32(32 - k8)).astype(np.int64)].astype(np.int64)
    e8 = esc.view(np.uint8)
    ei = (W >> np.uint32(32 - m)).astype(np.int64)
    esc_on = e == 0
    out_of_table = esc_on & (ei >= e8.size)
    if out_of_table.any():
        _fail("chain_walk: escape outside the escape table", out_of_table)
    ev = e8[np.minimum(ei, e8.size - 1)].astype(np.int64)
    return np.where(esc_on, ev, e), esc_on, esc_on & (ev == 0)


# ---- geometry -----------------------------------------------------------------------------------
def dec_slot_words(max_bits, max_len):
    bits = max_bits + K_CHAIN_SYMS * max_len
    w = (bits + 31) // 32 + 4 + 3 + 4
    return (w + 3) & ~3


def est_bits(ln):
    """build_dec_lut's estimate of a block's bits: the Kraft-weighted mean code length, summed in symbol
    order in double precision, times 2048 x 1.0625, plus 256."""
    L = ln[ln > 0].astype(np.float64)
    kbits = float(np.cumsum(np.ldexp(L, -L.astype(np.int64)))[-1])   # sequential, as the builder's loop
    return int(kbits * K_BLOCK_SYMS * 1.0625) + 256


def touched(ln, code, bits):
    """touched[w]: some code starts in, or covers, the `bits`-bit window w."""
    s = np.nonzero(ln)[0]
    L = ln[s].astype(np.int64)
    c = code[s].astype(np.int64)
    d = np.zeros((1 << bits) + 1, np.int32)
    short = L <= bits
    lo = np.where(short, c << np.maximum(bits - L, 0), c >> np.maximum(L - bits, 0))
    hi = np.where(short, (c + 1) << np.maximum(bits - L, 0), lo + 1)
    np.add.at(d, lo, 1)
    np.add.at(d, hi, -1)
    return np.cumsum(d[:-1]) > 0


def gaps64(ln, code):
    """The code space no code covers, as [lo, hi] inclusive u64 window ranges (incomplete codes only)."""
    s = np.nonzero(ln)[0]
    L = ln[s].astype(np.int64)
    lo = [int(code[x]) << (64 - int(l)) for x, l in zip(s, L)]
    hi = [((int(code[x]) + 1) << (64 - int(l))) for x, l in zip(s, L)]
    order = np.argsort(np.array(lo, dtype=U64), kind="stable")
    out, at = [], 0
    for i in order:
        assert lo[i] >= at, "not a prefix code"
        if lo[i] > at:
            out.append((at, lo[i] - 1))
        at = hi[i]
    if at < 1 << 64:
        out.append((at, (1 << 64) - 1))
    return out
