// hz_decode_device.h -- device code of the block decoders that more than one decode-side unit uses
// (hz_decode.hip, hz_index.hip, hz_chain.hip): the decoders' arguments, the LUT entry helpers and the
// table lookup, the staging loads and the pieces of the pipelined block decoder that k_decode and
// k_chain_decode share, and the per-lane bit reader. Force-inlined device functions, plain structs
// and constants only (no kernel, no relocatable device code); fill_dec_args is the one host helper.
#pragma once
#include "hz_device.h"

namespace hz {

// Arguments of the block decoders (hz_decode.hip) and of every kernel that looks codes up in the decode
// tables (the index builder's and the chain decode's walkers and fix-ups).
struct DecArgs {
    const uint32_t* words;   // payload view, 64-byte aligned
    uint64_t nwords;
    uint32_t bit_adj;        // payload bit 0 = bit bit_adj of words
    uint64_t nsym;
    uint64_t nblocks;
    const unsigned long long* starts;  // block index (hz_internal.h)
    const unsigned long long* subs;    // four u16 chain start bits per lane (low 16 bits)
    uint64_t start0;         // FIXED16 without an index: the stream's first bit (starts null)
    const uint32_t* lds_img;
    uint32_t lds_words;      // table words; the staging region follows
    uint32_t region_words;   // staging region per workgroup (slots sized in-kernel from max_bits)
    int k;
    int min_len;
    int max_len;
    int level_bits;          // LUT: widest global subtable (Tables::dec_level_bits)
    const uint32_t* l2;
    uint8_t* out;
    uint32_t* err;
};

// LUT entries (hz_internal.h): a link's subtable index is the next nb window
// bits; pos (bits [4:0]) places them in a 32-bit window, so a pipelined
// decoder extracts them with one v_bfe_u32 and no depth bookkeeping.
HZ_DEV bool lut_leaf(uint32_t e) { return (int32_t)e < 0; }
HZ_DEV bool lut_lds_link(uint32_t e) { return e < (kLutGlobal << 10); }  // false for leaves (bit 31)
HZ_DEV uint32_t lut_nb(uint32_t e) { return (e >> 5) & 15u; }
// index (raw space: < kLutGlobal LDS, else global + kLutGlobal) of window W's entry under link e
HZ_DEV uint32_t lut_next32(uint32_t e, uint32_t W) { return (e >> 10) + __builtin_amdgcn_ubfe(W, e, e >> 5); }
// entry at raw index i
HZ_DEV uint32_t lut_at(const uint32_t* lds, const uint32_t* l2, uint32_t i) {
    return i < kLutGlobal ? lds[i] : l2[i - kLutGlobal];
}
// l2 index of window W's entry under a global link e (one v_add3 after the bfe)
HZ_DEV uint32_t lut_gnext32(uint32_t e, uint32_t W) {
    return (e >> 10) + __builtin_amdgcn_ubfe(W, e, e >> 5) - kLutGlobal;
}

template <int MODE>
HZ_DEV void dec_lookup(const DecArgs& a, const uint32_t* lds, uint64_t win, uint32_t& sym, uint32_t& L) {
    if (MODE == DEC_FIXED16) {
        sym = reinterpret_cast<const uint16_t*>(lds)[(uint32_t)(win >> 48)];
        L = 16;
    } else if (MODE == DEC_DENSE) {
        const uint32_t idx = (uint32_t)(win >> (64 - a.k));
        sym = reinterpret_cast<const uint16_t*>(lds)[idx];
        const uint32_t lw = lds[(1u << a.k) / 2 + (idx >> 4)];
        L = (uint32_t)a.min_len + ((lw >> ((idx & 15) * 2)) & 3u);
    } else {
        uint32_t e = lds[(uint32_t)(win >> (64 - a.k))];
        uint32_t D = (uint32_t)a.k;
        while (!lut_leaf(e)) {  // 64-bit windows: depth tracked here (pos covers 32-bit windows only)
            const uint32_t nb = lut_nb(e);
            e = lut_at(lds, a.l2, (e >> 10) + (uint32_t)((win << D) >> (64 - nb)));
            D += nb;
        }
        L = lut_leaf_len(e);
        sym = lut_leaf_sym(e);
    }
}

// MSB-first window at bit `pos` of a staged (byte-swapped) slot: the top 33+
// bits are valid, or all 64 when WIDE (codes longer than 32 bits).
template <bool WIDE>
HZ_DEV uint64_t stage_window(const uint32_t* stg, uint32_t pos) {
    const uint32_t wi = pos >> 5, sh = pos & 31;
    const uint64_t two = (((uint64_t)stg[wi]) << 32) | stg[wi + 1];
    if (!WIDE) return two << sh;
    return (two << sh) | ((((uint64_t)stg[wi + 2]) << sh) >> 32);
}

// 16 staged payload bytes at word w (zeros past the payload; w may have wrapped below 0).
HZ_DEV uint4 dec_stage_load(const DecArgs& a, uint64_t w) {
    uint4 v;
    if (w < a.nwords && w + 4 <= a.nwords) {
        v = *reinterpret_cast<const uint4*>(a.words + w);
    } else {
        v.x = w < a.nwords ? a.words[w] : 0u;
        v.y = w + 1 < a.nwords ? a.words[w + 1] : 0u;
        v.z = w + 2 < a.nwords ? a.words[w + 2] : 0u;
        v.w = 0u;
    }
    return v;
}

// 16-byte staging loads a lane issues before any is used (dec_stage, dec_stage_prefetch: one memory
// round trip for blocks up to 4 KiB of payload).
constexpr int kStageUnroll = 4;

// Chain start bits relative to the block start (chain 64 c + l in slot c of lane l): sub holds the
// low 16 bits of each chain's stream bit, bs the block's start bit; offsets are mod 2^16, rebuilt from
// deltas when the block is that long.
HZ_DEV void dec_chain_offsets(uint64_t sub, uint64_t bs, uint64_t bits, int lane,
                                   uint32_t (&off)[kChainsPerLane]) {
    constexpr int C = kChainsPerLane;
#pragma unroll
    for (int c = 0; c < C; ++c) off[c] = ((uint32_t)(sub >> (16 * c)) - (uint32_t)bs) & 0xffffu;
    if (bits >= 65536) {  // rebuild from deltas in chain order: (c, l - 1) precedes (c, l), (c - 1, 63) (c, 0)
        uint32_t carry = 0, last = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            uint32_t pv = shfl_up_u32(off[c], 1);
            if (lane == 0) pv = last;
            last = __builtin_amdgcn_readlane(off[c], 63);
            uint32_t sc = (off[c] - pv) & 0xffffu;
#pragma unroll
            for (int dd = 1; dd < 64; dd <<= 1) {
                const uint32_t o = shfl_up_u32(sc, dd);
                if (lane >= dd) sc += o;
            }
            off[c] = carry + sc;
            carry = __builtin_amdgcn_readlane(off[c], 63);
        }
    }
}

// A chain of the pipelined decoders between its LDS step and its global lookup: the entry after LDS,
// the address of its global entry (an l2 index, or a byte offset in lut_l2_rsrc: dec_pipe_ldsn).
struct PipeLane {
    uint32_t e, gi;
};

// Phase fences of the NC-chain walk: keep each phase's LDS reads issued
// together whatever the scheduler would do (the decoder is order-sensitive).
#define HZ_WALK_FENCE() __builtin_amdgcn_sched_barrier(0)

// Global table l2 as a buffer whose byte 0 lies kLutGlobal words before l2[0]:
// the byte offset of a global link's entry is (raw + index bits) * 4, one
// v_add_lshl_u32; num_records covers the largest table (kLutMaxL2 entries).
// Lanes resolved in LDS read past num_records (0, no memory access) instead of l2[0]:
// 12.27-12.29 vs 12.33-12.37 ms at 16 GiB Zipf (round 3, A/B in one run). A leaf's offset
// computed as a link's is >= 4 * 2^21 and < 2^27 (hz_internal.h lut_leaf_entry): no wrap.
static_assert(kLutGlobal + kLutMaxL2 == (1u << 21), "a leaf (bit 31) read as a link lands past num_records");
HZ_DEV __amdgpu_buffer_rsrc_t lut_l2_rsrc(const uint32_t* l2) {
    return __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void*>(reinterpret_cast<uintptr_t>(l2) - 4ull * kLutGlobal), 0,
        4u * (kLutGlobal + kLutMaxL2), 0x00020000);
}

// The LDS steps of NC chains at once: all window reads, then all level-1
// reads, then all LDS-second-level reads in flight together, so NC chain
// steps cost three LDS round trips. p1[c] = the LDS bit address of chain c's
// next bit, minus 1 (>= 127 bits into its staging slot); k_decode has no
// static LDS, so the table and slots are addressed from LDS byte 0. r[c].e: the entry
// after LDS; r[c].gi: byte offset of its global entry in lut_l2_rsrc.
template <int NC>
HZ_DEV void dec_pipe_ldsn(const DecArgs& a, const uint32_t* lds, const uint32_t* p1, PipeLane* r, uint32_t adj = 0) {
    const uint32_t k = (uint32_t)a.k;
    uint32_t W[NC], e[NC], x[NC];
    bool h[NC];
    // descending slot (dec_stage_commit<true>): p1 holds m, stream word t + 1 at byte (m >> 3) & ~3,
    // word t just above it, and m & 31 is the funnel shift (no v_not per step); adj: bytes the
    // window lies above (p1 short by 128 bits per step taken, a multiple of 32: the shift holds).
    // All window reads issue before the first shift: without the fence the chain decoder's register
    // allocation reused one pair for all four (four serial LDS round trips per step; extract
    // 21.14-21.23 -> 20.91-21.01 ms, A/B).
    uint32_t whi[NC], wlo[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const uint32_t wb = ((p1[c] >> 3) & ~3u) + adj;
        whi[c] = lds_at(wb + 4);
        wlo[c] = lds_at(wb);
    }
    HZ_WALK_FENCE();
#pragma unroll
    for (int c = 0; c < NC; ++c) W[c] = __builtin_amdgcn_alignbit(whi[c], wlo[c], p1[c]);
    HZ_WALK_FENCE();
#pragma unroll
    for (int c = 0; c < NC; ++c) e[c] = lds_at((W[c] >> (32 - k)) << 2);
    HZ_WALK_FENCE();
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        h[c] = lut_lds_link(e[c]);
        const uint32_t byte = ((e[c] >> 10) + __builtin_amdgcn_ubfe(W[c], e[c], e[c] >> 5)) << 2;
        // a leaf's or a global link's byte address is >= 256 KiB, past the workgroup's LDS: that
        // read returns nothing anyone uses (the select below keeps e), so no address select
        x[c] = lds_at(byte);
    }
    HZ_WALK_FENCE();
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const uint32_t ee = h[c] ? x[c] : e[c];
        const uint32_t byte = ((ee >> 10) + __builtin_amdgcn_ubfe(W[c], ee, ee >> 5)) << 2;
        r[c].e = ee;
        // a leaf's byte offset lies in [4 * 2^21, 2^27): past num_records of lut_l2_rsrc, so the
        // load returns 0 without a memory access, with no select (lut_leaf_entry)
        r[c].gi = byte;
    }
}

// Block metadata of the pipelined decoder: start and end bit, the lane's chain offsets.
struct PipeMeta {
    uint64_t b0, b1, sub;
};

// The first NS 16-byte chunks of a block's staging window, always
// exactly NS loads per lane (static vmcnt for the pipelined waits):
// chunks past the window or the payload read a clamped address and are fixed
// up in registers. Requires nwords >= 4 (host check).
template <int NS>
HZ_DEV void dec_stage_prefetch(const DecArgs& a, const PipeMeta& m, int lane, uint4 (&v)[NS]) {
    const uint64_t w0 = (((m.b0 + a.bit_adj) >> 5) & ~3ull) - 4;
#pragma unroll
    for (int u = 0; u < NS; ++u) {
        const uint64_t w = w0 + 4ull * ((uint32_t)lane + (uint32_t)u * kWave);
        const bool in = w < a.nwords;  // also false for a window that wrapped below word 0
        const uint64_t wl = !in ? 0 : (w + 4 <= a.nwords ? w : a.nwords - 4);
        v[u] = *reinterpret_cast<const uint4*>(a.words + wl);
    }
}

// Writes the NS prefetched chunks (fixed up for the payload's end) and any
// further chunks of a longer window into the slot, loaded here (correct for any NS >= 1).
// DESC: the slot holds the words in descending order (stream word t at slot word 4 npc_max - 1 - t).
template <bool DESC = false, int NS>
HZ_DEV void dec_stage_commit(const DecArgs& a, const PipeMeta& m, uint32_t npc_max, uint32_t* stg, int lane,
                             const uint4 (&v)[NS], uint64_t& w0) {
    const uint64_t b0 = m.b0 + a.bit_adj, b1 = m.b1 + a.bit_adj;
    w0 = ((b0 >> 5) & ~3ull) - 4;
    const uint64_t wend = (b1 >> 5) + 2;
    uint32_t npc = (uint32_t)((wend - w0 + 3) >> 2);
    npc = npc < npc_max ? npc : npc_max;
#pragma unroll
    for (int u = 0; u < NS; ++u) {
        const uint32_t p = (uint32_t)lane + (uint32_t)u * kWave;
        if (p < npc) {
            const uint64_t w = w0 + 4ull * p;
            uint4 x = v[u];
            if (!(w < a.nwords && w + 4 <= a.nwords)) {  // tail of the payload (or wrapped): shift, zero-fill
                const uint64_t base = a.nwords - 4;
                uint32_t q[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const uint64_t wt = w + t;
                    q[t] = wt < a.nwords && w < a.nwords ? pick4(x, (uint32_t)(wt - base)) : 0u;
                }
                x = make_uint4(q[0], q[1], q[2], q[3]);
            }
            if (DESC)
                reinterpret_cast<uint4*>(stg)[npc_max - 1 - p] = make_uint4(bswap32(x.w), bswap32(x.z), bswap32(x.y), bswap32(x.x));
            else
                reinterpret_cast<uint4*>(stg)[p] = make_uint4(bswap32(x.x), bswap32(x.y), bswap32(x.z), bswap32(x.w));
        }
    }
    for (uint32_t p = (uint32_t)lane + NS * kWave; p < npc; p += kWave) {  // oversized block: rare
        const uint4 x = dec_stage_load(a, w0 + 4ull * p);
        if (DESC)
            reinterpret_cast<uint4*>(stg)[npc_max - 1 - p] = make_uint4(bswap32(x.w), bswap32(x.z), bswap32(x.y), bswap32(x.x));
        else
            reinterpret_cast<uint4*>(stg)[p] = make_uint4(bswap32(x.x), bswap32(x.y), bswap32(x.z), bswap32(x.w));
    }
}

constexpr int kPfStep = 4;  // chain step at which the next block's staging loads issue (2-6 measured equal)
constexpr int kDecPipe2Threads = 512;  // two staging slots per wave (1024 with smaller hot heads: 15.2 ms vs 13.1)

// Per-lane bit reader over the payload. Words come from 16-byte chunks with
// the next chunk always in flight (128 bits of lookahead, a quarter of the
// load instructions of word reads); past the payload it reads zeros.
struct BitReader {
    uint64_t buf;
    uint32_t nb;
    uint32_t nxt;
    uint4 cur, ahead;   // current chunk (raw words), the next one (in flight)
    uint32_t ci;        // next word of cur
    uint64_t abase;     // word index of `ahead`
};

// The reader's chunk load. br_init / br_word / br_next call it unqualified on their argument type A, so
// a type derived from DecArgs in namespace hz may overload it (a non-template beats this template; it is
// found by argument-dependent lookup where the readers are instantiated). hz_ranges.hip does, for
// PieceDecArgs, whose view also ends at its lower end: keep that type and its overload in namespace hz
// and the overload's parameter the derived type itself, or the readers fall back to this one silently.
template <typename A>
HZ_DEV uint4 ld_chunk(const A& a, uint64_t w) {  // w % 4 == 0
    if (w + 4 <= a.nwords) return *reinterpret_cast<const uint4*>(a.words + w);
    uint4 v;
    v.x = w < a.nwords ? a.words[w] : 0u;
    v.y = w + 1 < a.nwords ? a.words[w + 1] : 0u;
    v.z = w + 2 < a.nwords ? a.words[w + 2] : 0u;
    v.w = 0u;
    return v;
}

template <typename A>
HZ_DEV uint32_t br_word(BitReader& r, const A& a) {
    const uint32_t v = pick4(r.cur, r.ci);
    if (++r.ci == 4) {
        r.cur = r.ahead;
        r.ci = 0;
        r.abase += 4;
        r.ahead = ld_chunk(a, r.abase);
    }
    return bswap32(v);
}

template <typename A>
HZ_DEV void br_init(BitReader& r, const A& a, uint64_t p) {
    const uint64_t w = p >> 5;
    const uint32_t sh = (uint32_t)(p & 31);
    const uint64_t base = w & ~3ull;
    r.cur = ld_chunk(a, base);
    r.abase = base + 4;
    r.ahead = ld_chunk(a, r.abase);
    r.ci = (uint32_t)(w & 3);
    const uint32_t w0 = br_word(r, a);
    const uint32_t w1 = br_word(r, a);
    r.buf = (((uint64_t)w0 << 32) | w1) << sh;
    r.nb = 64 - sh;
    r.nxt = br_word(r, a);
}

// Length (and symbol) of the codeword at the reader, then advance past it. A: DecArgs or a type derived
// from it (the reader's loads are ld_chunk's of that type).
template <int MODE, typename A>
HZ_DEV uint32_t br_next(BitReader& r, const A& a, const uint32_t* lds, uint32_t& sym) {
    if (r.nb <= 32) {
        r.buf |= (uint64_t)r.nxt << (32 - r.nb);
        r.nb += 32;
        r.nxt = br_word(r, a);
    }
    const uint64_t win = r.nb >= 56 ? r.buf : (r.buf | ((uint64_t)r.nxt >> (r.nb - 32)));
    uint32_t L;
    dec_lookup<MODE>(a, lds, win, sym, L);
    if (L < r.nb) {
        r.buf <<= L;
        r.nb -= L;
    } else {
        const uint32_t rr = L - r.nb;
        r.buf = (uint64_t)r.nxt << (32 + rr);
        r.nb = 32 - rr;
        r.nxt = br_word(r, a);
    }
    return L;
}

// The decode tables of a codebook and the payload view into a decoder's arguments (host).
inline void fill_dec_args(DecArgs& a, const Tables& t, const uint8_t* d_payload, uint64_t payload_bytes,
                          uint64_t nsym) {
    // View the payload from the 64-byte boundary at or below it (inside the
    // same allocation: device allocations are 256-byte aligned). The last word
    // may extend up to 3 bytes past payload_bytes (include/huffman_amd.h).
    const uintptr_t base = (uintptr_t)d_payload & ~(uintptr_t)63;
    a.words = reinterpret_cast<const uint32_t*>(base);
    a.bit_adj = (uint32_t)(((uintptr_t)d_payload & 63) * 8);
    a.nwords = (payload_bytes + ((uintptr_t)d_payload & 63) + 3) / 4;
    a.nsym = nsym;
    a.nblocks = index_blocks(nsym);
    a.lds_img = t.d_dec_lds;
    a.lds_words = t.dec_lds_bytes / 4;
    a.k = t.dec_k;
    a.level_bits = t.dec_level_bits;
    a.min_len = t.dec_min_len;
    a.max_len = t.dec_max_len;
    a.l2 = t.d_dec_l2;
}

}  // namespace hz
