// hz_kernels.hip -- gfx950 (MI355X, CDNA4) kernels of the decode side of the Huffman hot path
// (the generator and histogram: hz_hist.hip; the pack: hz_pack.hip).
//
//   k_decode   block-parallel table decode              <- Decompressor.cu:259-291
//   k_sync_*   block index of an index-less stream (reference files), parallel, self-synchronising
//   k_chain_*  index-less decode in chain blocks
//
// Layout, roofline and design notes: DESIGN.md. All integer/bit work; no MFMA.
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>

#include "hz_device.h"

namespace hz {

// ===========================================================================
// Decode (replaces translateFile, Decompressor.cu:259-291).
//
// Block decoder: one wave per 2048-symbol pack block. The block's payload
// bits [start[b], start[b+1]) are staged into the wave's LDS slot with
// coalesced 16-byte loads (byte-swapped once on the way in); then each lane
// decodes its 32 symbols as two independent 16-symbol chains whose start bits
// come from the block index, reading every window straight from LDS. There
// is no per-lane refill state, so a symbol costs a window read, a table
// lookup and an add. Tables (LDS, one copy per workgroup):
//   DENSE: 2^K u16 symbols + 2-bit (len - min_len), K = max_len;
//   LUT:   2^K1 u32 level-1 entries (leaf / link, hz_internal.h),
//          deeper levels in global memory.
// Every code 16 bits (FIXED16): symbol i sits at bit start + 16 i, so that
// decoder needs no index and no staging (k_decode_fixed16).
// ===========================================================================
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

// Stage payload words [w0, w0 + 4 npc) of block b into `stg`, byte-swapped.
// The first kStageUnroll 16-byte loads of every lane are issued before any
// is used (one memory round trip for blocks up to 4 KiB of payload).
constexpr int kStageUnroll = 4;
template <bool WIDE>
HZ_DEV void dec_stage(const DecArgs& a, uint64_t b0, uint64_t b1, uint32_t npc_max, uint32_t* stg, int lane,
                      uint64_t& w0) {
    w0 = ((b0 >> 5) & ~3ull) - 4;  // one 16-byte pad before the block: every position is >= 128 (may wrap: zeros)
    const uint64_t wend = (b1 >> 5) + (WIDE ? 3 : 2);
    uint32_t npc = (uint32_t)((wend - w0 + 3) >> 2);
    npc = npc < npc_max ? npc : npc_max;
    uint4 v[kStageUnroll];
#pragma unroll
    for (int u = 0; u < kStageUnroll; ++u) {
        const uint32_t p = (uint32_t)lane + (uint32_t)u * kWave;
        if (p < npc) v[u] = dec_stage_load(a, w0 + 4ull * p);
    }
#pragma unroll
    for (int u = 0; u < kStageUnroll; ++u) {
        const uint32_t p = (uint32_t)lane + (uint32_t)u * kWave;
        if (p < npc)
            reinterpret_cast<uint4*>(stg)[p] = make_uint4(bswap32(v[u].x), bswap32(v[u].y), bswap32(v[u].z), bswap32(v[u].w));
    }
    for (uint32_t p = (uint32_t)lane + kStageUnroll * kWave; p < npc; p += kWave) {
        const uint4 x = dec_stage_load(a, w0 + 4ull * p);
        reinterpret_cast<uint4*>(stg)[p] = make_uint4(bswap32(x.x), bswap32(x.y), bswap32(x.z), bswap32(x.w));
    }
}

// Chain slot c of lane l decodes the block's chain 64 c + l (its symbols 8 (64 c + l) .. + 7), so the
// lane's chain-c symbols are the 16 output bytes at 1024 c + 16 l and each of a block's four output stores
// covers 1 KiB (lane-major chains -- the lane's 32 symbols as 64 contiguous bytes -- left every store
// touching 64 separate 64-byte pieces: 12.3 vs 11.15 ms at 16 GiB Zipf, round 3 A/B). The index keeps
// its layout (sub[b * 64 + l] = chains 4 l .. 4 l + 3), so a lane reads its four chain starts as u16s.
HZ_DEV uint64_t dec_sub_load(const DecArgs& a, uint64_t b, int lane) {
    const uint16_t* s16 = reinterpret_cast<const uint16_t*>(a.subs) + b * kChainsPerBlock + (uint32_t)lane;
    return (uint64_t)s16[0] | ((uint64_t)s16[64] << 16) | ((uint64_t)s16[128] << 32) | ((uint64_t)s16[192] << 48);
}

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

HZ_DEV void dec_store(const DecArgs& a, uint64_t b, int lane, const uint32_t* pk) {
    const uint64_t sym0 = b * kBlockSyms;
    if (sym0 + kBlockSyms <= a.nsym) {
        // non-temporal (streaming) stores: the output is not read again by this kernel
        // (10.70 vs 11.15-11.37 ms at 16 GiB Zipf, round 3 A/B; buffer stores with nt / sc0 nt /
        // nt sc1 / sc0 nt sc1 10.13-10.48 vs 10.01-10.02 ms)
        uint4* o = reinterpret_cast<uint4*>(a.out + 2 * sym0) + lane;
#pragma unroll
        for (int c = 0; c < kChainsPerLane; ++c)
            store_nt16(o + c * kWave, make_uint4(pk[4 * c], pk[4 * c + 1], pk[4 * c + 2], pk[4 * c + 3]));
    } else {
#pragma unroll
        for (int c = 0; c < kChainsPerLane; ++c) {
            const uint64_t s0 = sym0 + (uint64_t)kChainSyms * (uint32_t)(c * kWave + lane);
            if (s0 >= a.nsym) continue;
            uint8_t* ob = a.out + 2 * s0;
            const uint32_t cnt = a.nsym - s0 < (uint64_t)kChainSyms ? (uint32_t)(a.nsym - s0) : kChainSyms;
            for (uint32_t q = 0; q < cnt; ++q) {
                const uint32_t v = (pk[4 * c + (q >> 1)] >> (16 * (q & 1))) & 0xffffu;
                ob[2 * q] = (uint8_t)v;
                ob[2 * q + 1] = (uint8_t)(v >> 8);
            }
        }
    }
}

// One wave decodes NB blocks at once (NB * kChainsPerLane independent chains
// per lane: every table wait covers more symbols). Block g of the group uses
// staging slot g. Blocks past the stream's end decode nothing.
template <int MODE, bool WIDE, int NB, typename A>
HZ_DEV void dec_group(const A& a, const uint32_t* lds, uint32_t* stg0, uint32_t slot, uint64_t bfirst,
                      int lane) {
    constexpr int C1 = kChainsPerLane;
    constexpr int C = NB * C1;
    const uint32_t npc_max = slot >> 2;
    uint32_t pos[C];
#pragma unroll
    for (int g = 0; g < NB; ++g) {
        const uint64_t b = bfirst + g < a.nblocks ? bfirst + g : a.nblocks - 1;  // duplicates decode, never store
        const uint64_t b0 = a.starts[b] + a.bit_adj, b1 = a.starts[b + 1] + a.bit_adj;
        const uint64_t sub = dec_sub_load(a, b, lane);
        uint64_t w0;
        dec_stage<WIDE>(a, b0, b1, npc_max, stg0 + g * slot, lane, w0);
        uint32_t off[C1];
        dec_chain_offsets(sub, b0 - a.bit_adj, b1 - b0, lane, off);
        const uint32_t base = (uint32_t)(b0 - (w0 << 5)) + (uint32_t)g * slot * 32u;
#pragma unroll
        for (int c = 0; c < C1; ++c) pos[g * C1 + c] = base + off[c];
    }
    __builtin_amdgcn_wave_barrier();  // LDS ops of one wave complete in order
    uint32_t pk[NB][kSPT / 2];
    // Windows: 32 bits (bit 31 = the chain's next bit) for codes <= 32 bits,
    // one funnel shift of two staged words; 64 bits for WIDE.
    using Win = typename std::conditional<WIDE, uint64_t, uint32_t>::type;
    constexpr uint32_t WB = WIDE ? 64 : 32;
#pragma unroll
    for (int q = 0; q < kChainSyms; ++q) {
        Win win[C];
        uint32_t sym[C], L[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if constexpr (WIDE) {
                win[c] = stage_window<true>(stg0, pos[c]);
            } else {
                const uint32_t p1 = pos[c] - 1u;  // >= 127 (staging pad)
                const uint32_t* w = stg0 + (p1 >> 5);
                win[c] = __builtin_amdgcn_alignbit(w[0], w[1], 31u - p1);
            }
        }
        if (MODE == DEC_DENSE) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const uint32_t idx = (uint32_t)(win[c] >> (WB - (uint32_t)a.k));
                sym[c] = reinterpret_cast<const uint16_t*>(lds)[idx];
                const uint32_t lw = lds[(1u << a.k) / 2 + (idx >> 4)];
                L[c] = (uint32_t)a.min_len + ((lw >> ((idx & 15) * 2)) & 3u);
            }
        } else {
            uint32_t e[C], e2[C], D[C];
#pragma unroll
            for (int c = 0; c < C; ++c) { e[c] = lds[(uint32_t)(win[c] >> (WB - (uint32_t)a.k))]; D[c] = (uint32_t)a.k; }
#pragma unroll
            for (int c = 0; c < C; ++c) {  // LDS-resident second level (hot subtables)
                if (lut_lds_link(e[c])) {
                    const uint32_t nb = lut_nb(e[c]);
                    e[c] = lds[(e[c] >> 10) + (uint32_t)((Win)(win[c] << D[c]) >> (WB - nb))];
                    D[c] += nb;
                }
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {  // first global level of every chain before one wait
                e2[c] = e[c];
                if (!lut_leaf(e[c])) {
                    const uint32_t nb = lut_nb(e[c]);
                    e2[c] = a.l2[(e[c] >> 10) - kLutGlobal + (uint32_t)((Win)(win[c] << D[c]) >> (WB - nb))];
                }
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                uint32_t ee = e2[c];
                if (!lut_leaf(e[c])) {
                    uint32_t Dd = D[c] + lut_nb(e[c]);
                    while (!lut_leaf(ee)) {  // deeper global levels: rare
                        const uint32_t nb = lut_nb(ee);
                        ee = a.l2[(ee >> 10) - kLutGlobal + (uint32_t)((Win)(win[c] << Dd) >> (WB - nb))];
                        Dd += nb;
                    }
                }
                L[c] = lut_leaf_len(ee);
                sym[c] = lut_leaf_sym(ee);
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            pos[c] += L[c];
            const int g = c / C1;
            const int i = ((c % C1) * kChainSyms + q) >> 1;  // symbol (c%C1)*8+q of the lane in block g
            if (q & 1) pk[g][i] |= sym[c] << 16;
            else pk[g][i] = sym[c];
        }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int g = 0; g < NB; ++g)
        if (bfirst + g < a.nblocks) dec_store(a, bfirst + g, lane, pk[g]);
}

// Two-level LUT decode of one block with the global lookups software
// pipelined. Needs max_len <= k + level bits (every global lookup ends in
// a leaf) and max_len <= 32. The lane's chains are two halves, {0,1} and
// {2,3}; a half's LDS step (window, level 1, LDS second level) issues its
// global lookups unconditionally (lanes that do not need one read l2[0]:
// same-address lanes coalesce), and those are consumed only after the other
// half's LDS step has issued its own, so every wait is vmcnt(2) in
// straight-line code and one half's table walk hides the other's gather.
struct PipeLane {
    uint32_t e, gi;
};

// One chain's LDS step: window, level 1, the LDS second level (hot heads).
// r.gi: the l2 index of the global entry to read (0 -- one coalesced address
// -- when the chain is resolved in LDS).
HZ_DEV PipeLane dec_pipe_lds(const DecArgs& a, const uint32_t* lds, const uint32_t* stg, uint32_t pos) {
    const uint32_t p1 = pos - 1u;  // >= 127 (staging pad)
    const uint32_t* w = stg + (p1 >> 5);
    const uint32_t W = __builtin_amdgcn_alignbit(w[0], w[1], 31u - p1);
    uint32_t e = lds[W >> (32 - a.k)];
    if (lut_lds_link(e)) e = lds[lut_next32(e, W)];
    PipeLane r;
    r.e = e;
    r.gi = lut_leaf(e) ? 0u : lut_gnext32(e, W);
    return r;
}

// The LDS steps of two chains at once, branch-free so the compiler keeps one
// basic block: both window reads, then both level-1 reads, then both
// LDS-second-level reads are in flight together (three LDS round trips for the
// pair instead of three per chain). Lanes without an LDS second level read
// word 0 (a broadcast, no bank conflict) and keep their level-1 entry.
HZ_DEV void dec_pipe_lds2(const DecArgs& a, const uint32_t* lds, const uint32_t* stg, uint32_t pos0, uint32_t pos1,
                          PipeLane& r0, PipeLane& r1) {
    const uint32_t k = (uint32_t)a.k;
    const uint32_t pa = pos0 - 1u, pb = pos1 - 1u;  // >= 127 (staging pad)
    const uint32_t* wa = stg + (pa >> 5);
    const uint32_t* wb = stg + (pb >> 5);
    const uint32_t a0 = wa[0], a1 = wa[1], b0 = wb[0], b1 = wb[1];
    const uint32_t Wa = __builtin_amdgcn_alignbit(a0, a1, 31u - pa);
    const uint32_t Wb = __builtin_amdgcn_alignbit(b0, b1, 31u - pb);
    uint32_t ea = lds[Wa >> (32 - k)];
    uint32_t eb = lds[Wb >> (32 - k)];
    const bool ha = lut_lds_link(ea), hb = lut_lds_link(eb);
    const uint32_t xa = lds[ha ? lut_next32(ea, Wa) : 0u], xb = lds[hb ? lut_next32(eb, Wb) : 0u];
    ea = ha ? xa : ea;
    eb = hb ? xb : eb;
    r0.e = ea;
    r1.e = eb;
    r0.gi = lut_leaf(ea) ? 0u : lut_gnext32(ea, Wa);
    r1.gi = lut_leaf(eb) ? 0u : lut_gnext32(eb, Wb);
}

// The LDS steps of NC chains at once (dec_pipe_lds2 generalised): all window
// reads, then all level-1 reads, then all LDS-second-level reads in flight
// together, so NC chain steps cost three LDS round trips.
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

HZ_DEV void dec_meta_load(const DecArgs& a, uint64_t b, int lane, PipeMeta& m) {
    const uint64_t bb = b < a.nblocks ? b : a.nblocks - 1;  // past the end: any block, never used
    // the block's bounds through the scalar cache (the index is read-only here): the window
    // arithmetic that follows stays on the scalar unit
    typedef const __attribute__((address_space(4))) unsigned long long* cu64p;
    const uint64_t bu = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(bb >> 32)) << 32) |
                        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)bb);
    m.b0 = ((cu64p)a.starts)[bu];
    m.b1 = ((cu64p)a.starts)[bu + 1];
    m.sub = dec_sub_load(a, bb, lane);
}

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
// Persistent pipelined decoder of one wave: blocks b, b + stride, ... The
// staging chunks of the next block and the metadata of the one after are
// loaded halfway through this block's steps, so no block waits on HBM.
template <typename A>
HZ_DEV void dec_wave_pipe(const A& a, const uint32_t* lds, uint32_t* stg, uint32_t slot, uint64_t b,
                          uint64_t stride, int lane) {
    const uint32_t* l2g = a.l2;
    constexpr int C = kChainsPerLane;
    static_assert(C == 4, "two halves of two chains");
    PipeMeta mc, mn, mn2;
    uint4 sc[kStageUnroll], sn[kStageUnroll];
    dec_meta_load(a, b, lane, mc);
    dec_meta_load(a, b + stride, lane, mn);
    dec_stage_prefetch(a, mc, lane, sc);
    for (; b < a.nblocks; b += stride) {
        uint64_t w0;
        dec_stage_commit(a, mc, slot >> 2, stg, lane, sc, w0);
        uint32_t off[C];
        dec_chain_offsets(mc.sub, mc.b0, mc.b1 - mc.b0, lane, off);
        const uint32_t base = (uint32_t)(mc.b0 + a.bit_adj - (w0 << 5));
        uint32_t pos[C];
#pragma unroll
        for (int c = 0; c < C; ++c) pos[c] = base + off[c];
        __builtin_amdgcn_wave_barrier();  // LDS ops of one wave complete in order
        uint32_t pk[kSPT / 2];
        PipeLane st[C];
        uint32_t g[C];
        auto finish = [&](int c, int q) {
            const uint32_t ee = (st[c].e >> 31) ? st[c].e : g[c];
            pos[c] += lut_leaf_len(ee);
            const uint32_t sym = lut_leaf_sym(ee);
            const int i = (c * kChainSyms + q) >> 1;
            if (q & 1) pk[i] |= sym << 16;
            else pk[i] = sym;
        };
        auto issue2 = [&](int c) {
            dec_pipe_lds2(a, lds, stg, pos[c], pos[c + 1], st[c], st[c + 1]);
            g[c] = l2g[st[c].gi];
            g[c + 1] = l2g[st[c + 1].gi];
        };
        issue2(0);
#pragma unroll
        for (int q = 0; q < kChainSyms; ++q) {
            issue2(2);
            if (q == kPfStep) {  // next block's staging chunks, the metadata after it
                dec_stage_prefetch(a, mn, lane, sn);
                dec_meta_load(a, b + 2 * stride, lane, mn2);
            }
            finish(0, q);
            finish(1, q);
            if (q + 1 < kChainSyms) issue2(0);
            finish(2, q);
            finish(3, q);
        }
        __builtin_amdgcn_wave_barrier();
        dec_store(a, b, lane, pk);
        mc = mn;
        mn = mn2;
#pragma unroll
        for (int u = 0; u < kStageUnroll; ++u) sc[u] = sn[u];
    }
}

// Two blocks per wave (8 chains per lane in 4 pairs): each pair's global
// lookups are consumed after the other three pairs' LDS walks, so a gather
// has three walks to land in instead of one. Half as many waves (two staging
// slots each) hold the same LDS; blocks b, b + 1, then b + stride, ...
// The two blocks run half a block out of phase: block X (slot 0) is at steps
// 4-7 while block Y (slot 1) is at steps 0-3, then Y at 4-7 beside X's
// successor at 0-3, so one quad is mid-block whenever the other drains,
// stores and refills its slot. The wave's first block runs steps 0-3 alone;
// after the last pair the successor in slot 0 is a duplicate that is dropped
// mid-block.
// NS: staging chunks prefetched per block (kStageUnroll, or 3 where the launcher knows the mean block
// fits them: dec_stage_chunks).
template <int NS, typename A>
HZ_DEV void dec_wave_pipe2(const A& a, const uint32_t* lds, uint32_t* stg, uint32_t slot, uint64_t b,
                           uint64_t stride, int lane) {
    constexpr int C = 2 * kChainsPerLane;
    constexpr int H = kChainSyms / 2;
    static_assert(kChainsPerLane == 4, "four pairs of chains over two blocks");
    static_assert(kChainSyms == 8 && kPfStep == H, "a block's prefetch issues at the top of its second half");
    const __amdgpu_buffer_rsrc_t l2r = lut_l2_rsrc(a.l2);
    PipeMeta mn[2], mn2;  // mn[j]: the block slot j takes next; mn2: the one after it, from prefetch to commit
    uint4 sn[NS];  // one block's prefetch is in flight at a time
    uint32_t p1[C];
    uint32_t pk[2][kSPT / 2];
    PipeLane st[C];
    uint32_t g[C];
    // slot j takes the block of mn[j] (its chunks are in sn); mn[j] moves on to mn2
    auto commit = [&](int j) {
        uint64_t w0;
        dec_stage_commit<true>(a, mn[j], slot >> 2, stg + j * slot, lane, sn, w0);
        uint32_t off[kChainsPerLane];
        dec_chain_offsets(mn[j].sub, mn[j].b0, mn[j].b1 - mn[j].b0, lane, off);
        // m = (E - 1) * 32 + 31 - r for the slot's top word E and r = the chain's next bit - 1,
        // relative to stream word w0; a step of L bits subtracts L
        const uint32_t top = (uint32_t)(stg - lds) + (uint32_t)(j + 1) * slot - 1u;
        const uint32_t base = top * 32u - (uint32_t)(mn[j].b0 + a.bit_adj - (w0 << 5));
#pragma unroll
        for (int c = 0; c < kChainsPerLane; ++c) p1[j * kChainsPerLane + c] = base - off[c];
        mn[j] = mn2;
    };
    // the staging chunks of slot j's next block, the metadata of block `after` (the one behind it)
    auto prefetch = [&](int j, uint64_t after) {
        dec_stage_prefetch(a, mn[j], lane, sn);
        dec_meta_load(a, after, lane, mn2);
    };
    auto finish = [&](int c, int q) {
        // a leaf in LDS (bit 31) beats its gather's 0 (read past num_records); a link loses to its
        // gathered leaf: one v_max; and the leaf's byte 3 is 0x80 | L, subtracted whole (128 bits
        // more per step, which the window address takes back: dec_pipe_ldsn's adj). 12 % fewer VALU
        // per block pair; k_decode 10.09 -> 9.97 ms, chain decode 11.30 -> 11.13 ms (A/B, 16 GiB Zipf)
        const uint32_t ee = st[c].e > g[c] ? st[c].e : g[c];
        p1[c] -= ee >> 24;
        const int i = ((c % kChainsPerLane) * kChainSyms + q) >> 1;
        // an even step keeps the whole entry; the odd step packs both symbols (leaf bytes 1-2) by one v_perm
        if (q & 1) pk[c / kChainsPerLane][i] = __builtin_amdgcn_perm(ee, pk[c / kChainsPerLane][i], 0x06050201u);
        else pk[c / kChainsPerLane][i] = ee;
    };
    // two quads (one per block): a quad's gathers land behind the other quad's walk
    auto issue4 = [&](int c, int q) {
        // issue priority over the quad's LDS walk and gathers (decode 9.96-9.99 -> 9.88-9.91 ms, A/B)
        __builtin_amdgcn_s_setprio(2);
        dec_pipe_ldsn<4>(a, lds, p1 + c, st + c, 16u * (uint32_t)q);  // q steps taken: 16 q bytes
#pragma unroll
        for (int t = 0; t < 4; ++t)
            g[c + t] = __builtin_amdgcn_raw_buffer_load_b32(l2r, st[c + t].gi, 0, 0);
        __builtin_amdgcn_s_setprio(0);
    };
    auto finish4 = [&](int c, int q) {
#pragma unroll
        for (int t = 0; t < 4; ++t) finish(c + t, q);
    };
    // prologue: both slots filled, the first block through steps 0 .. H - 1 alone
    if (b >= a.nblocks) return;
    dec_meta_load(a, b, lane, mn[0]);
    dec_meta_load(a, b + 1, lane, mn[1]);
    prefetch(0, b + stride);
    commit(0);
    prefetch(1, b + 1 + stride);
    commit(1);
    __builtin_amdgcn_wave_barrier();  // LDS ops of one wave complete in order
    issue4(0, 0);
#pragma unroll
    for (int q = 0; q < H; ++q) {
        finish4(0, q);
        issue4(0, q + 1);
    }
    for (; b < a.nblocks; b += stride) {
        // X = block b (slot 0) at steps H .. 7 beside Y = block b + 1 (slot 1) at steps 0 .. H - 1
#pragma unroll
        for (int t = 0; t < H; ++t) {
            issue4(4, t);
            if (t == 0) prefetch(0, b + 2 * stride);  // X's successor X', the metadata of the one after
            finish4(0, H + t);
            if (t + 1 < H) {
                issue4(0, H + t + 1);
            } else {
                // X is done: its stores go out behind Y's gathers (stores and loads share vmcnt and
                // complete in order), X' takes the slot after X's last window read
                __builtin_amdgcn_wave_barrier();
                dec_store(a, b, lane, pk[0]);
                commit(0);
                __builtin_amdgcn_wave_barrier();
                issue4(0, 0);
            }
            finish4(4, t);
        }
        // Y at steps H .. 7 beside X' at steps 0 .. H - 1 (a duplicate past the stream's end, never stored)
#pragma unroll
        for (int t = 0; t < H; ++t) {
            issue4(4, H + t);
            if (t == 0) prefetch(1, b + 1 + 2 * stride);
            finish4(0, t);
            issue4(0, t + 1);
            finish4(4, H + t);
        }
        __builtin_amdgcn_wave_barrier();
        if (b + 1 < a.nblocks) dec_store(a, b + 1, lane, pk[1]);
        commit(1);
        __builtin_amdgcn_wave_barrier();
    }
}

constexpr int kDecPipe2Threads = 512;  // two staging slots per wave (1024 with smaller hot heads: 15.2 ms vs 13.1)
// PIPE: 0 plain block loop, 1 pipelined (one block per wave), 2 pipelined, two blocks per wave
// NS: dec_wave_pipe2's staging chunks per block (PIPE 2 only)
template <int MODE, bool WIDE, int PIPE, int NS = kStageUnroll>
__global__ __launch_bounds__(PIPE == 2 ? kDecPipe2Threads : 1024) void k_decode(DecArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    copy_lds_table(lds, a.lds_img, a.lds_words);
    const int lane = threadIdx.x & 63;
    const uint32_t wid = wave_id();
    // slots fit the stream's largest block; waves without a slot have nothing to do
    const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)dec_slot_words(a.starts[a.nblocks + 1], a.max_len));
    const uint32_t nwave = blockDim.x >> 6;
    if constexpr (PIPE == 2) {
        uint32_t nw2 = a.region_words / (2 * slot);
        nw2 = nw2 < nwave ? nw2 : nwave;
        if (nw2 > 0) {  // else one block per wave below (a stream whose largest block needs more)
            if (wid >= nw2) return;
            const uint64_t b = 2 * ((uint64_t)blockIdx.x * nw2 + wid), stride = 2 * (uint64_t)gridDim.x * nw2;
            dec_wave_pipe2<NS>(a, lds, lds + a.lds_words + wid * 2 * slot, slot, b, stride, lane);
            return;
        }
    }
    uint32_t nw = a.region_words / slot;
    nw = nw < nwave ? nw : nwave;
    if (wid >= nw) return;
    uint32_t* stg = lds + a.lds_words + wid * slot;
    const uint64_t b = (uint64_t)blockIdx.x * nw + wid, stride = (uint64_t)gridDim.x * nw;
    if constexpr (PIPE != 0) {
        dec_wave_pipe(a, lds, stg, slot, b, stride, lane);
    } else {
        for (uint64_t bb = b; bb < a.nblocks; bb += stride) dec_group<MODE, WIDE, 1>(a, lds, stg, slot, bb, lane);
    }
}

// The FIXED16 step: five byte-swapped stream words whose bit pos % 32 is a code's first bit -> the
// eight symbols of the next 128 bits as four output words.
HZ_DEV void fixed16_step(const uint16_t* t16, const uint32_t (&ww)[5], uint32_t pos, uint32_t (&o)[4]) {
    const uint32_t sh = pos & 31;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const uint32_t cw = sh ? __builtin_amdgcn_alignbit(ww[t], ww[t + 1], 32u - sh) : ww[t];
        o[t] = (uint32_t)t16[cw >> 16] | ((uint32_t)t16[cw & 0xffffu] << 16);
    }
}

// Every code 16 bits: lane j decodes symbols [32 j, 32 j + 32) from the 17
// words starting at stream word (p0 >> 5) + 16 j.
// Full blocks [0, nb) of a FIXED16 stream (k_pack_fixed16_blk's mapping): lane l's sub-run c decodes the block's symbols 8 (64 c + l) .. + 7 from 4 words at a
// 1 KiB-coalesced offset plus the next sub-run's first word (lane l + 1 by DPP, sub-run c + 1's lane 0,
// or the next block's first word), and stores 16 bytes at a 1 KiB-coalesced offset.
__global__ __launch_bounds__(1024) void k_decode_fixed16_blk(DecArgs a, uint64_t nb) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    copy_lds_table(lds, a.lds_img, a.lds_words);
    const uint16_t* t16 = reinterpret_cast<const uint16_t*>(lds);
    const uint64_t p0 = (a.starts ? a.starts[0] : a.start0) + a.bit_adj;
    const uint32_t* w = a.words + (p0 >> 5);  // any word of the payload view
    const u32x4a4* w4 = reinterpret_cast<const u32x4a4*>(w);
    uint4* o4 = reinterpret_cast<uint4*>(a.out);
    const int lane = threadIdx.x & 63;
    const uint64_t W = (uint64_t)gridDim.x * (blockDim.x >> 6);
    uint64_t b = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    constexpr uint32_t kBW = kBlockSyms / 2;  // words per block
    auto load = [&](uint64_t bb, u32x4a4 (&x)[kChainsPerLane], uint32_t& nw) {
        bb = bb < nb ? bb : 0;
#pragma unroll
        for (int c = 0; c < kChainsPerLane; ++c) x[c] = w4[bb * (kBW / 4) + c * kWave + lane];
        nw = w[(bb + 1) * kBW];  // the next block's first word (the stream's last block follows block nb - 1)
    };
    u32x4a4 nx[kChainsPerLane];
    uint32_t nn = 0;
    if (b < nb) load(b, nx, nn);
    for (; b < nb; b += W) {
        u32x4a4 x[kChainsPerLane];
#pragma unroll
        for (int c = 0; c < kChainsPerLane; ++c) x[c] = nx[c];
        const uint32_t after = nn;
        load(b + W, nx, nn);
#pragma unroll
        for (int c = 0; c < kChainsPerLane; ++c) {
            uint32_t nxt = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x[c].x, kDppWaveShl1, 0xf, 0xf, false);
            const uint32_t first_next = c + 1 < kChainsPerLane ? readlane(x[c + 1 < kChainsPerLane ? c + 1 : c].x, 0) : after;
            if (lane == 63) nxt = first_next;
            const uint32_t ww[5] = {bswap32(x[c].x), bswap32(x[c].y), bswap32(x[c].z), bswap32(x[c].w), bswap32(nxt)};
            uint32_t o[4];
            fixed16_step(t16, ww, (uint32_t)p0, o);
            store_nt16(o4 + b * (kBlockSyms / 8) + c * kWave + lane, make_uint4(o[0], o[1], o[2], o[3]));
        }
    }
}

// Lane runs of 32 symbols: those after the nb blocks k_decode_fixed16_blk decodes, or all of them.
// (Its 17-word step keeps its 64-bit shift: through fixed16_step the kernel compiles to other instructions.)
__global__ __launch_bounds__(1024) void k_decode_fixed16(DecArgs a, uint64_t nb) {
    const uint64_t j_begin = nb * kWave;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    copy_lds_table(lds, a.lds_img, a.lds_words);
    const uint64_t p0 = (a.starts ? a.starts[0] : a.start0) + a.bit_adj;  // the stream's first bit (all FIXED16 needs)
    const uint16_t* t16 = reinterpret_cast<const uint16_t*>(lds);
    const uint32_t sh = (uint32_t)(p0 & 31);
    const uint64_t W0 = p0 >> 5;
    const bool vec = (W0 & 3) == 0;
    const uint64_t nl = (a.nsym + kSPT - 1) / kSPT;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = j_begin + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nl; j += stride) {
        const uint64_t ws = W0 + 16 * j;
        uint32_t w[17];
        if (vec && ws + 17 <= a.nwords) {
            const uint4* p = reinterpret_cast<const uint4*>(a.words + ws);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint4 v = p[q];
                w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
            }
            w[16] = a.words[ws + 16];
        } else {
#pragma unroll
            for (int k = 0; k < 17; ++k) w[k] = ws + k < a.nwords ? a.words[ws + k] : 0u;
        }
#pragma unroll
        for (int k = 0; k < 17; ++k) w[k] = bswap32(w[k]);
        uint32_t o[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const uint32_t c = (uint32_t)(((((uint64_t)w[t]) << 32 | w[t + 1]) << sh) >> 32);
            o[t] = (uint32_t)t16[c >> 16] | ((uint32_t)t16[c & 0xffffu] << 16);
        }
        const uint64_t sym0 = j * kSPT;
        if (sym0 + kSPT <= a.nsym) {
            uint4* d = reinterpret_cast<uint4*>(a.out + 2 * sym0);
#pragma unroll
            for (int q = 0; q < 4; ++q) d[q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
        } else {
            uint8_t* ob = a.out + 2 * sym0;
            const uint32_t cnt = (uint32_t)(a.nsym - sym0);
            for (uint32_t q = 0; q < cnt; ++q) {
                const uint32_t v = (o[q >> 1] >> (16 * (q & 1))) & 0xffffu;
                ob[2 * q] = (uint8_t)v;
                ob[2 * q + 1] = (uint8_t)(v >> 8);
            }
        }
    }
}

static void fill_dec_args(DecArgs& a, const Tables& t, const uint8_t* d_payload, uint64_t payload_bytes,
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

// The random access view of the block decoders (DESIGN.md "Random access"; launchers below).
struct RangeDecArgs : DecArgs {
    uint64_t w_first;    // first word of the view that exists (words below it are only addressed, never read)
    const uint8_t* bad;  // per tile block: nonzero = failed a check, nothing is stored for it
    uint64_t blk0;       // the tile's first block in the stream (a.starts / a.subs / a.nblocks are the tile's)
    uint64_t lo, hi;     // stream symbols [lo, hi) go to out + 2 (sym - lo); nothing else is written
};

// dec_stage_prefetch for a moved view: chunks outside the payload read the view's first real chunk
// (dec_stage_commit zero-fills them as it does for the plain view's word 0).
template <int NS>
HZ_DEV void dec_stage_prefetch(const RangeDecArgs& a, const PipeMeta& m, int lane, uint4 (&v)[NS]) {
    const uint64_t w0 = (((m.b0 + a.bit_adj) >> 5) & ~3ull) - 4;
#pragma unroll
    for (int u = 0; u < NS; ++u) {
        const uint64_t w = w0 + 4ull * ((uint32_t)lane + (uint32_t)u * kWave);
        const bool in = w < a.nwords && w >= a.w_first;
        const uint64_t wl = !in ? a.w_first : (w + 4 <= a.nwords ? w : a.nwords - 4);
        v[u] = *reinterpret_cast<const uint4*>(a.words + wl);
    }
}

// dec_store clipped to [lo, hi): whole blocks inside the range as chain_store writes them (16-byte
// non-temporal stores at a 2-byte aligned address), edge blocks symbol by symbol.
HZ_DEV void dec_store(const RangeDecArgs& a, uint64_t b, int lane, const uint32_t* pk) {
    if (a.bad[b]) return;
    const uint64_t sym0 = (a.blk0 + b) * kBlockSyms;
    uint16_t* out16 = reinterpret_cast<uint16_t*>(a.out);
    if (sym0 >= a.lo && sym0 + kBlockSyms <= a.hi) {
        uint16_t* ob = out16 + (sym0 - a.lo);
#pragma unroll
        for (int c = 0; c < kChainsPerLane; ++c) {
            u32x4a2 v = u32x4a2{pk[4 * c], pk[4 * c + 1], pk[4 * c + 2], pk[4 * c + 3]};
            __builtin_nontemporal_store(v, reinterpret_cast<u32x4a2*>(ob + kChainSyms * (kWave * c + lane)));
        }
        return;
    }
#pragma unroll
    for (int c = 0; c < kChainsPerLane; ++c) {
        const uint64_t s0 = sym0 + (uint64_t)kChainSyms * (uint32_t)(c * kWave + lane);
        for (uint32_t q = 0; q < (uint32_t)kChainSyms; ++q) {
            const uint64_t sy = s0 + q;
            if (sy >= a.lo && sy < a.hi) out16[sy - a.lo] = (uint16_t)(pk[4 * c + (q >> 1)] >> (16 * (q & 1)));
        }
    }
}

// k_decode over the moved view: the same body (as one force-inlined function templated on the argument
// type it compiles to other instructions in all ten instances, so it is kept twice).
template <int MODE, bool WIDE, int PIPE, int NS = kStageUnroll>
__global__ __launch_bounds__(PIPE == 2 ? kDecPipe2Threads : 1024) void k_decode_range(RangeDecArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    copy_lds_table(lds, a.lds_img, a.lds_words);
    const int lane = threadIdx.x & 63;
    const uint32_t wid = wave_id();
    // slots fit the stream's largest block; waves without a slot have nothing to do
    const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)dec_slot_words(a.starts[a.nblocks + 1], a.max_len));
    const uint32_t nwave = blockDim.x >> 6;
    if constexpr (PIPE == 2) {
        uint32_t nw2 = a.region_words / (2 * slot);
        nw2 = nw2 < nwave ? nw2 : nwave;
        if (nw2 > 0) {  // else one block per wave below (a stream whose largest block needs more)
            if (wid >= nw2) return;
            const uint64_t b = 2 * ((uint64_t)blockIdx.x * nw2 + wid), stride = 2 * (uint64_t)gridDim.x * nw2;
            dec_wave_pipe2<NS>(a, lds, lds + a.lds_words + wid * 2 * slot, slot, b, stride, lane);
            return;
        }
    }
    uint32_t nw = a.region_words / slot;
    nw = nw < nwave ? nw : nwave;
    if (wid >= nw) return;
    uint32_t* stg = lds + a.lds_words + wid * slot;
    const uint64_t b = (uint64_t)blockIdx.x * nw + wid, stride = (uint64_t)gridDim.x * nw;
    if constexpr (PIPE != 0) {
        dec_wave_pipe(a, lds, stg, slot, b, stride, lane);
    } else {
        for (uint64_t bb = b; bb < a.nblocks; bb += stride) dec_group<MODE, WIDE, 1>(a, lds, stg, slot, bb, lane);
    }
}

// Launch shape: slots are sized for the average block (estimated from the
// payload size) with headroom; the kernel sizes the real slots from the
// index's max_bits and idles the waves that do not get one. Up to two
// workgroups per CU (each holds its own table copy): whichever shape runs
// more waves.
template <int MODE, bool WIDE, int PIPE, int NS, typename A>
static const void* decode_fn() {
    if constexpr (std::is_same<A, DecArgs>::value) return (const void*)k_decode<MODE, WIDE, PIPE, NS>;
    else return (const void*)k_decode_range<MODE, WIDE, PIPE, NS>;
}

// Staging chunks the two-blocks-per-wave decoder prefetches per block: 3 where three chunks (3 KiB)
// hold the mean block's window, else kStageUnroll. From the view's size alone (no device read):
// nwords * 4 / nblocks bounds the mean block's bytes; the window adds the 16-byte pad before the block
// and the two words read past its last bit; the slack (1/64 of the mean + 16 bytes) covers the first
// word's offset in its chunk (up to 12 bytes) and the spread of the block sizes about their mean (a
// block is 2048 codes: at a code-length deviation of 8 bits, 8 sqrt(2048) = 362 bits = 45 bytes, 1/64
// of 3 KiB). Any choice decodes any stream: a longer window's further chunks are loaded at the commit.
constexpr int kStageFew = 3;
static int dec_stage_chunks(uint64_t nwords, uint64_t nblocks) {
    const uint64_t mean = (nwords * 4 + nblocks - 1) / nblocks;
    return mean + 16 + 8 + mean / 64 + 16 < 16ull * kWave * kStageFew ? kStageFew : kStageUnroll;
}

template <int MODE, bool WIDE, int PIPE, typename A = DecArgs, int NS = kStageUnroll>
static hipError_t run_decode(const A& a, uint64_t payload_bits, int ncu, hipStream_t s) {
    const void* fn = decode_fn<MODE, WIDE, PIPE, NS, A>();
    {
        hipError_t e = ensure_lds_limit(fn, kLdsBytes);
        if (e != hipSuccess) return e;
    }
    // a block never exceeds 2048 x max_len bits, whatever follows the stream in the buffer
    uint64_t avg = (payload_bits + a.nblocks - 1) / a.nblocks;
    avg = avg < (uint64_t)kBlockSyms * (uint32_t)a.max_len ? avg : (uint64_t)kBlockSyms * (uint32_t)a.max_len;
    const uint32_t worst = dec_slot_words_max(a.max_len);
    uint32_t est = dec_slot_words(avg + avg / 16 + 256, a.max_len);
    est = est < worst ? est : worst;
    const uint32_t table = a.lds_words;
    if (MODE == DEC_LUT && PIPE == 2 && table < kDecMinLdsWords) return hipErrorInvalidValue;  // biased windows
    int best_w = 0, best_g = 1;
    for (int g = 1; g <= 2; ++g) {
        const uint32_t room = kLdsBytes / 4 / (uint32_t)g;
        if (room <= table + est) continue;
        int w = (int)((room - table) / est);
        const int maxw = PIPE == 2 ? 2 * kDecPipe2Threads / 64 : kDecMaxWaves;  // slots
        w = w > maxw ? maxw : w;
        if (g * w > best_g * best_w) { best_w = w; best_g = g; }
    }
    if (best_w == 0) return hipErrorInvalidValue;
    A b = a;
    b.region_words = (uint32_t)best_w * est;
    if (b.region_words < worst && table + worst <= kLdsBytes / 4) b.region_words = worst;  // any stream decodes
    if (table + b.region_words > kLdsBytes / 4 / (uint32_t)best_g) best_g = 1;
    if (table + b.region_words > kLdsBytes / 4) return hipErrorInvalidValue;
    const uint32_t lds = 4 * (table + b.region_words);
    uint64_t wgs = (a.nblocks + best_w - 1) / best_w;
    const uint64_t cap = (uint64_t)ncu * best_g;
    if (wgs > cap) wgs = cap;
    // PIPE 2: a wave takes two slots
    const int threads = PIPE == 2 ? (64 * ((best_w + 1) / 2) < kDecPipe2Threads ? 64 * ((best_w + 1) / 2)
                                                                                 : kDecPipe2Threads)
                                  : 64 * best_w;
    void* kargs[] = {&b};
    return hipLaunchKernel(fn, dim3(wgs), dim3(threads), kargs, lds, s);
}

static int dec_pipe_mode() {
    static const int v = [] { const char* e = getenv("HZ_DEC_PIPE"); return e ? atoi(e) : 2; }();
    return v;
}

// The block decoder of a codebook. pipe_ok: the caller's view holds the four words the pipelined
// decoders' staging prefetch needs; payload_bits: see run_decode.
// *stage_chunks (nullable): the staging chunks prefetched per block, 0 for a decoder without that choice.
template <typename A>
static hipError_t decode_dispatch(const Tables& t, const A& a, bool pipe_ok, uint64_t payload_bits, int ncu,
                                  hipStream_t s, int* stage_chunks = nullptr) {
    if (stage_chunks) *stage_chunks = 0;
    if (t.dec_mode == DEC_DENSE) return run_decode<DEC_DENSE, false, 0>(a, payload_bits, ncu, s);
    if (t.dec_max_len > 32) return run_decode<DEC_LUT, true, 0>(a, payload_bits, ncu, s);
    // two levels suffice (no lookup chain past a global subtable): pipelined gathers
    const int pipe_env = dec_pipe_mode();
    if (pipe_env && t.dec_max_len <= t.dec_k + t.dec_level_bits && pipe_ok) {
        if (pipe_env == 1) return run_decode<DEC_LUT, false, 1>(a, payload_bits, ncu, s);
        const int ns = dec_stage_chunks(a.nwords, a.nblocks);
        if (stage_chunks) *stage_chunks = ns;
        return ns == kStageFew ? run_decode<DEC_LUT, false, 2, A, kStageFew>(a, payload_bits, ncu, s)
                               : run_decode<DEC_LUT, false, 2>(a, payload_bits, ncu, s);
    }
    return run_decode<DEC_LUT, false, 0>(a, payload_bits, ncu, s);
}

hipError_t launch_decode(const Tables& t, const uint8_t* d_payload, uint64_t payload_bytes, uint64_t nsym,
                         const unsigned long long* d_index, uint8_t* d_out, uint32_t* d_err, int ncu,
                         hipStream_t s, uint64_t start0, int* stage_chunks) {
    if (stage_chunks) *stage_chunks = 0;
    if (nsym == 0) return hipSuccess;
    if (!d_index && t.dec_mode != DEC_FIXED16) return hipErrorInvalidValue;
    DecArgs a;
    fill_dec_args(a, t, d_payload, payload_bytes, nsym);
    a.starts = d_index;
    a.subs = d_index ? d_index + index_sub_offset(a.nblocks) : nullptr;
    a.start0 = start0;
    a.out = d_out; a.err = d_err;
    if (t.dec_mode == DEC_FIXED16) {
        hipError_t e = ensure_lds_limit((const void*)k_decode_fixed16, kFixed16LdsBytes);
        if (e != hipSuccess) return e;
        if ((e = ensure_lds_limit((const void*)k_decode_fixed16_blk, kFixed16LdsBytes)) != hipSuccess) return e;
        const uint64_t nl = (nsym + kSPT - 1) / kSPT;
        // every block but the last through the coalesced kernel; the lane-run kernel takes the last
        const uint64_t nb = kFixed16Blk && a.nblocks > 1 ? a.nblocks - 1 : 0;
        if (nb) {
            uint64_t wgs = (nb + 15) / 16;
            if (wgs > (uint64_t)ncu) wgs = ncu;
            hipLaunchKernelGGL(k_decode_fixed16_blk, dim3(wgs), dim3(1024), kFixed16LdsBytes, s, a, nb);
        }
        uint64_t wgs = (nl + 1023) / 1024;
        if (wgs > (uint64_t)ncu) wgs = ncu;
        hipLaunchKernelGGL(k_decode_fixed16, dim3(wgs), dim3(1024), kFixed16LdsBytes, s, a, nb);
        return hipGetLastError();
    }
    return decode_dispatch(t, a, a.nwords >= 4, payload_bytes * 8, ncu, s, stage_chunks);
}

// ===========================================================================
// Block index of an index-less stream (a .compressed file from the reference
// encoder; Decompressor.cu:259-291 decodes it serially). Huffman codes
// resynchronise: a decoder started at an arbitrary bit falls onto the true
// codeword boundaries after some codewords (measured on Zipf(1.1): median 83
// bits, p99 590). The stream is cut into 4096-bit segments, one lane each, and
// every segment keeps a BOUNDARY BITMAP (bit d of its row = a codeword starts
// at segment bit d), one bit per payload bit:
//   k_sync_scan   : decode segment k from its first bit to the first boundary
//                   past its end -> exit[k], count[k] and the bitmap of every
//                   boundary of that path in the segment
//   k_sync_iter   : the true path enters k at exit[k-1]; follow it until it
//                   lands on a bitmap boundary (from there both paths agree)
//                   or leaves the segment, rewriting the bitmap up to there
//                   with the true boundaries (count and exit follow). Repeated
//                   (host loop) for segments whose entry changed, until no
//                   exit changes: chains of unsynchronised segments are rare.
//   k_scan_*      : exclusive scan of counts -> first codeword number per segment
//   k_sync_select : the bitmap now holds exactly the true boundaries; every
//                   8th one (a chain start) and every 2048th (a block start)
//                   is picked by popcounts -- no second walk of the stream
//   k_sync_subs   : chain positions relative to their block, max block bits
// ===========================================================================
constexpr uint32_t kSegBits = 4096;
constexpr int kSyncThreads = 1024;
constexpr uint32_t kBmpWords = kSegBits / 32;  // bitmap row of a segment

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

// Length (and symbol) of the codeword at the reader, then advance past it.
template <int MODE>
HZ_DEV uint32_t br_next(BitReader& r, const DecArgs& a, const uint32_t* lds, uint32_t& sym) {
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

struct SyncArgs {
    uint64_t start;                 // stream bit of the first symbol (payload view: + bit_adj)
    uint64_t nseg;
    uint32_t* bmp;                  // boundary bitmap, kBmpWords per segment
    unsigned long long* ent;        // entry of a dirty segment: the previous segment's exit
    unsigned long long* cnt;        // boundaries in the segment's bitmap row
    uint32_t* dirty[2];             // segments to check against their entry, ping-pong between iterations
    uint32_t* changed;              // segments whose walk left them in this iteration
};

template <int MODE>
__global__ __launch_bounds__(kSyncThreads) void k_sync_scan(DecArgs a, SyncArgs y) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    copy_lds_table(lds, a.lds_img, a.lds_words);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < y.nseg; k += stride) {
        const uint64_t s0 = y.start + k * kSegBits, s1 = s0 + kSegBits;
        // bitmap words leave four at a time (16-byte stores): every store is a
        // vmcnt entry that later load waits queue behind
        uint4* bm = reinterpret_cast<uint4*>(y.bmp + k * kBmpWords);
        BitReader r;
        br_init(r, a, s0 + a.bit_adj);
        uint64_t pos = s0, n = 0;
        uint32_t cw = 0, cur = 0;  // bitmap word being filled
        uint4 q = make_uint4(0, 0, 0, 0);
        auto put = [&]() {
            const uint32_t j = cw & 3;
            q.x = j == 0 ? cur : q.x;
            q.y = j == 1 ? cur : q.y;
            q.z = j == 2 ? cur : q.z;
            q.w = j == 3 ? cur : q.w;
            if (j == 3) bm[cw >> 2] = q;
            cur = 0;
            ++cw;
        };
        while (pos < s1) {
            const uint32_t d = (uint32_t)(pos - s0);
            while ((d >> 5) != cw) put();
            cur |= 1u << (d & 31);
            uint32_t sym;
            const uint32_t L = br_next<MODE>(r, a, lds, sym);
            if (L == 0) { atomicOr(a.err, 2u); break; }
            pos += L;
            ++n;
        }
        while (cw < kBmpWords) put();
        if (k + 1 < y.nseg) { y.ent[k + 1] = pos; y.dirty[0][k + 1] = 1u; }
        y.cnt[k] = n;
    }
}

// Two segments per lane in lockstep (codebooks the pipelined decoder takes:
// codes <= 32 bits, every global lookup a leaf): both streams' LUT walks and
// gathers are in flight together, so one stream's lookup latency hides the
// other's. Same outputs as the one-segment kernel.
template <typename A>
HZ_DEV void br_refill(BitReader& r, const A& a) {
    if (r.nb <= 32) {
        r.buf |= (uint64_t)r.nxt << (32 - r.nb);
        r.nb += 32;
        r.nxt = br_word(r, a);
    }
}

// Lengths of the codewords at two readers (top 32 bits of each window).
HZ_DEV void lut_len2(const DecArgs& a, const uint32_t* lds, const BitReader (&r)[2], uint32_t (&L)[2]) {
    const uint32_t k = (uint32_t)a.k;
    uint32_t W[2], e[2], x[2], gi[2];
    bool h[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) W[c] = (uint32_t)(r[c].buf >> 32);
#pragma unroll
    for (int c = 0; c < 2; ++c) e[c] = lds[W[c] >> (32 - k)];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        h[c] = lut_lds_link(e[c]);
        x[c] = lds[h[c] ? lut_next32(e[c], W[c]) : 0u];
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        e[c] = h[c] ? x[c] : e[c];
        gi[c] = lut_leaf(e[c]) ? 0u : lut_gnext32(e[c], W[c]);
    }
    const uint32_t g0 = a.l2[gi[0]], g1 = a.l2[gi[1]];
    L[0] = lut_leaf_len((e[0] >> 31) ? e[0] : g0);
    L[1] = lut_leaf_len((e[1] >> 31) ? e[1] : g1);
}

__global__ __launch_bounds__(kSyncThreads) void k_sync_scan2(DecArgs a, SyncArgs y) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    copy_lds_table(lds, a.lds_img, a.lds_words);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k0 < y.nseg; k0 += 2 * stride) {
        BitReader r[2];
        uint64_t s0[2];
        uint32_t d[2], n[2], cw[2], cur[2];  // 32-bit: bits and codewords relative to the segment
        uint4 q[2];
        bool act[2];
        uint4* bm[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const uint64_t k = k0 + c * stride;
            act[c] = k < y.nseg;
            s0[c] = y.start + (act[c] ? k : k0) * kSegBits;
            d[c] = n[c] = 0;
            cw[c] = cur[c] = 0;
            q[c] = make_uint4(0, 0, 0, 0);
            bm[c] = reinterpret_cast<uint4*>(y.bmp + (act[c] ? k : k0) * kBmpWords);
            br_init(r[c], a, s0[c] + a.bit_adj);
        }
        auto put = [&](int c) {
            const uint32_t j = cw[c] & 3;
            q[c].x = j == 0 ? cur[c] : q[c].x;
            q[c].y = j == 1 ? cur[c] : q[c].y;
            q[c].z = j == 2 ? cur[c] : q[c].z;
            q[c].w = j == 3 ? cur[c] : q[c].w;
            if (j == 3) bm[c][cw[c] >> 2] = q[c];
            cur[c] = 0;
            ++cw[c];
        };
        while (act[0] || act[1]) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                // codes <= 32 bits: the boundary's bitmap word advances by at most one per step
                if (act[c]) {
                    if ((d[c] >> 5) != cw[c]) put(c);
                    cur[c] |= 1u << (d[c] & 31);
                }
                br_refill(r[c], a);
            }
            uint32_t L[2];
            lut_len2(a, lds, r, L);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if (!act[c]) continue;
                if (L[c] == 0) { atomicOr(a.err, 2u); act[c] = false; continue; }
                r[c].buf <<= L[c];
                r[c].nb -= L[c];
                d[c] += L[c];
                ++n[c];
                act[c] = d[c] < kSegBits;
            }
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const uint64_t k = k0 + c * stride;
            if (k >= y.nseg) continue;
            while (cw[c] < kBmpWords) put(c);
            if (k + 1 < y.nseg) { y.ent[k + 1] = s0[c] + d[c]; y.dirty[0][k + 1] = 1u; }
            y.cnt[k] = n[c];
        }
    }
}

// ---------------------------------------------------------------------------
// Index walker for the pipelined decoder's codebooks (codes <= 32 bits, one
// global LUT level): LONG chains -- each lane walks kWalkChains stretches of spc whole
// segments, each starting kWalkLead bits early so the walk has resynchronised
// (P(not) ~ 4e-4 on Zipf) when it reaches its first segment: one start per
// ~10^5 codewords instead of one per segment. Each chain streams its payload
// through a 4-chunk LDS ring (16-byte chunks, one refill load per round,
// issued a round ahead) and marks boundaries into a 4-chunk LDS mark ring
// (ds_or), flushed one chunk per round as a 16-byte store into the bitmap;
// per-segment counts come from popcounts of the flushed chunks.
// Lookups use the decoder's level 1 with hot heads sized to the LDS the rings
// leave; a chain whose code needs the global level PARKS for the rest of the
// round, and the round ends with one gather for all parked chains: every wait
// is the round's single vmcnt(0) (refill + gathers), never a gather queued
// behind a refill in mid-walk.
// A chain's exit becomes the entry of the next chain's first segment
// (ent/dirty): k_sync_iter checks it against the bitmap, which lands at once
// when the lead-in resynchronised.
// ---------------------------------------------------------------------------
// steps per round: u8 table 8: 25.5 ms, 10: 25.3 ms; 4-bit table 10/12/14: 24.7/24.4/24.6 ms;
// round 4 (16 GiB Zipf, A/B in one run, k_idx_walk alone): 12 / 14 / 16 steps 17.32 / 17.11 / 17.44 ms
constexpr int kWalkSteps = 14;
// parked chains resume after each part of a round: 2 parts of 6 steps 23.6-23.9 ms, 1 part
// 23.7-24.3, 2 x 8 23.4-23.9, 3 x 6 23.2-24.3, 3 x 4 24.8, 4 x 4 23.5-24.2 (A/B in one run);
// round 3 (2.3 % escapes): 2 / 1 / 3 parts 22.1 / 22.1-22.3 / 23.4 ms
constexpr int kWalkHalves = 2;
constexpr uint32_t kWalkLead = 1024;    // lead-in bits before a chain's first segment

struct WalkArgs {
    const uint32_t* words;    // payload view, 64-byte aligned
    uint64_t nwords;          // >= 4 (host check)
    uint32_t bit_adj;         // payload bit 0 = bit bit_adj of words
    uint64_t start;           // stream bit of the first symbol
    uint64_t nseg, spc, nchains;
    const uint32_t* lds_img;  // 4-bit code length - bias per k-bit window (0: longer than k bits)
    uint32_t lds_words;
    int k, bias;
    const uint8_t* esc;       // u8 code length per m-bit window (escapes only)
    int m;
    uint32_t* bmp;
    unsigned long long* cnt;
    unsigned long long* ent;
    uint32_t* dirty;
    uint32_t lead;            // k_chain_walk: lead-in bits before a chain's first bit
    const uint32_t* w8_img;   // k_chain_walk: u8 code length per k8-bit window (0: escape)
    uint32_t w8_words;
    int k8;
    const uint32_t* lut1;     // k_chain_walk<DEEP>: the decode LUT (level-1 image, global levels) that
    const uint32_t* lut2;     // resolves escapes the m-bit escape table leaves at 0 (codes > m bits)
    int lutk;
};

// 16 payload bytes at word w (4-aligned): zeros before word 0 / past the end.
HZ_DEV uint4 walk_load(const WalkArgs& a, uint64_t w) {
    const bool in = w < a.nwords;  // false for a window that wrapped below word 0
    const uint64_t wl = !in ? 0 : (w + 4 <= a.nwords ? w : a.nwords - 4);
    return *reinterpret_cast<const uint4*>(a.words + wl);
}
HZ_DEV uint4 walk_fix(const WalkArgs& a, uint64_t w, uint4 x) {
    if (w < a.nwords && w + 4 <= a.nwords) return x;
    const uint64_t base = a.nwords - 4;
    uint32_t q[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const uint64_t wt = w + t;
        q[t] = wt < a.nwords && w < a.nwords ? pick4(x, (uint32_t)(wt - base)) : 0u;
    }
    return make_uint4(q[0], q[1], q[2], q[3]);
}

// Chunk slot q (0..3) of a payload ring, byte-swapped.
template <uint32_t ROW>
HZ_DEV void ring_put(uint32_t* ring, uint32_t q, const uint4& x) {
    const uint32_t v[4] = {bswap32(x.x), bswap32(x.y), bswap32(x.z), bswap32(x.w)};
#pragma unroll
    for (int i = 0; i < 4; ++i) ring[(4 * q + i) * ROW] = v[i];
}

// Payload chunks reach a chain's ring from a register group of kWalkGroup
// chunks loaded together (one 64/128-byte run per lane, issued as soon as the
// previous group is in the ring), and finished mark chunks leave as a run of
// kWalkMarkGroup chunks: every lane touches a different stretch of the stream,
// so 16-byte accesses spread over many rounds let L2 evict a line between them
// (fetches ~10x the payload, writes ~3.5x the bitmap with single chunks).
// Measured (u32 LUT walker): 1/1 chunks 41.7 ms, 4/4 38.7, 1/8 38.9, 8/8 41.7; (4-bit walker)
// 4/4 23.9-24.3 ms, 2/4 24.9, 8/4 24.9, 4/2 26.8, 4/8 24.1, 8/8 25.0.
constexpr uint32_t kWalkGroup = 4;
constexpr uint32_t kWalkMarkGroup = 4;
static_assert((kWalkGroup & (kWalkGroup - 1)) == 0 && kWalkGroup >= 1 && kWalkGroup <= 8, "walk group");
static_assert((kWalkMarkGroup & (kWalkMarkGroup - 1)) == 0 && kWalkMarkGroup >= 1 && kWalkMarkGroup <= 8,
              "mark group");

template <uint32_t G>
HZ_DEV uint4 pick_group(const uint4 (&g)[G], uint32_t i) {
    uint4 x = g[0];
#pragma unroll
    for (uint32_t t = 1; t < G; ++t) {
        const bool s = i == t;
        x.x = s ? g[t].x : x.x;
        x.y = s ? g[t].y : x.y;
        x.z = s ? g[t].z : x.z;
        x.w = s ? g[t].w : x.w;
    }
    return x;
}

__global__ __launch_bounds__(kWalkWaves * 64) void k_idx_walk(WalkArgs a) {
    // the length table at LDS address 0 (a static array: its address folds into
    // the ds_read offset), the rings after it
    __shared__ __attribute__((aligned(16))) uint32_t wtab[(1u << kWalkK) / 8];
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    copy_lds_table(wtab, a.lds_img, a.lds_words);
    const uint8_t* lds8 = reinterpret_cast<const uint8_t*>(wtab);
    constexpr int C = kWalkChains;
    constexpr uint32_t kRow = 1;  // ring word stride
    constexpr uint32_t G = kWalkGroup, GM = kWalkMarkGroup;
    constexpr uint32_t kMarkRow = 16;  // ring words 0..15 payload, then kWalkMarkChunks mark chunks, 1 pad
    constexpr uint32_t kMW = 4 * kWalkMarkChunks;  // mark ring words
    const uint32_t k = (uint32_t)a.k, bias = (uint32_t)a.bias;
    const int lane = threadIdx.x & 63;
    const uint32_t wid = threadIdx.x >> 6;
    const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t* ring[C];
    uint32_t off[C], off0[C], ms[C], end[C], f[C], mcount[C], nmc[C], rc[C];
    uint64_t bch[C], x0[C], seg0[C], seg1[C];
    bool live[C], pk[C], on[C];  // on: the walk has reached ms (marks count)
    uint4 pre[C][G];   // payload group holding chunk f
    uint4 mk[C][GM];   // finished mark chunks of the current run
    // window registers: the 32 bits at off are alignbit(w0, w1, sh) (sh in 0..31;
    // 32 - sh bits of w0 consumed), nxt = ring word wn, the one after w1
    uint32_t w0[C], w1[C], sh[C], wn[C], nxt[C];
    bool gin[C];  // the payload group in pre[] lies inside the payload (no clamping)
#pragma unroll
    for (int c = 0; c < C; ++c) {
        ring[c] = lds + ((wid * C + c) * 64 + lane) * kRingWords;
        const uint64_t ch = tid + c * T;
        live[c] = ch < a.nchains;
        const uint64_t chc = live[c] ? ch : 0;
        seg0[c] = chc * a.spc;
        seg1[c] = seg0[c] + a.spc < a.nseg ? seg0[c] + a.spc : a.nseg;
        const uint64_t cs = seg0[c] * kSegBits, ce = seg1[c] * kSegBits;
        x0[c] = cs - (cs < kWalkLead ? cs : kWalkLead);
        const uint64_t P0 = a.start + a.bit_adj + x0[c];
        bch[c] = (P0 >> 7) - 1;  // one chunk before the walk (wraps to ~0 at the payload's start: zeros)
        off0[c] = off[c] = (uint32_t)(P0 - 128 * bch[c]);
        ms[c] = off[c] + (uint32_t)(cs - x0[c]);
        end[c] = live[c] ? off[c] + (uint32_t)(ce - x0[c]) : off[c];
        nmc[c] = live[c] ? (uint32_t)((ce - cs) / 128) : 0u;
        mcount[c] = rc[c] = 0;
        pk[c] = false;
        on[c] = ms[c] == off[c];
#pragma unroll
        for (uint32_t i = kMarkRow; i < kRingWords; ++i) ring[c][i * kRow] = 0u;
#pragma unroll
        for (uint32_t i = 0; i < GM; ++i) mk[c][i] = make_uint4(0, 0, 0, 0);
    }
    // prologue: chunks 0..2 of every chain, and the group holding chunk 3
#pragma unroll
    for (int c = 0; c < C; ++c) {
        uint4 v[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) v[g] = walk_load(a, 4 * (bch[c] + g));
        const uint64_t gb = (bch[c] + 3) & ~(uint64_t)(G - 1);
        gin[c] = 4 * (gb + G) <= a.nwords && gb < a.nwords;
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) pre[c][g] = walk_load(a, 4 * (gb + g));
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            ring_put<kRow>(ring[c], (uint32_t)g, walk_fix(a, 4 * (bch[c] + g), v[g]));
        }
        f[c] = 3;
        const uint32_t q0 = (off[c] - 1) >> 5;
        w0[c] = ring[c][q0 * kRow];
        w1[c] = ring[c][(q0 + 1) * kRow];
        sh[c] = (0u - off[c]) & 31;
        wn[c] = q0 + 2;
    }
    uint32_t pW[C];  // a parked chain's window
    // chunk f goes into the ring at a round's end when it fits (the chain no
    // longer needs chunk f - 4), ahead of the round's bitmap stores
    for (;;) {
        bool alive = false;
#pragma unroll
        for (int c = 0; c < C; ++c) alive |= off[c] < end[c] || mcount[c] < nmc[c];
        if (!__any(alive)) break;
        // the round's steps stay below: chain end, filled data (w0, w1 and nxt: the
        // bits below off + 96), free mark slots
        uint32_t lim[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            lim[c] = min(on[c] ? end[c] : ms[c], min(128 * f[c] - 96, ms[c] + 128 * (mcount[c] + kWalkMarkChunks)));
            nxt[c] = ring[c][(wn[c] & 15) * kRow];  // (re)read after the ring's refill
        }
        // branch-free steps: one LDS length lookup per chain and step; a chain that
        // cannot step only leaves off unchanged, a code longer than k bits parks the
        // chain for the rest of the round
        // parked chains: one gather from the escape table for all of them, then
        // the codeword is marked and stepped over (mid-round and at the round's end)
        auto resolve = [&]() {
            uint32_t g[C];
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (pk[c]) g[c] = a.esc[pW[c] >> (32 - a.m)];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (!pk[c]) continue;
                if (off[c] >= ms[c]) {
                    const uint32_t rel = off[c] - ms[c];
                    atomicOr(ring[c] + (kMarkRow + ((rel >> 5) & (kMW - 1))) * kRow, 1u << (rel & 31));
                }
                const uint32_t L = g[c];
                off[c] += L;
                const int32_t r = (int32_t)sh[c] - (int32_t)L;
                if (r < 0) {
                    w0[c] = w1[c];
                    w1[c] = nxt[c];
                    ++wn[c];
                    nxt[c] = ring[c][(wn[c] & 15) * kRow];
                }
                sh[c] = (uint32_t)(r < 0 ? r + 32 : r);
                pk[c] = false;
            }
        };
#pragma unroll
        for (int half = 0; half < kWalkHalves; ++half) {
#pragma unroll
            for (int t = 0; t < kWalkSteps / kWalkHalves; ++t) {
                uint32_t W[C], e[C];
                bool ok[C];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    ok[c] = !pk[c] & (off[c] < lim[c]);
                    W[c] = __builtin_amdgcn_alignbit(w0[c], w1[c], sh[c]);
                    e[c] = lds8[W[c] >> (33 - k)];  // two windows per byte (k >= 2)
                }
                HZ_WALK_FENCE();
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    e[c] = __builtin_amdgcn_ubfe(e[c], (W[c] >> (30 - k)) & 4u, 4);  // the window's nibble
                    const bool adv = ok[c] & (e[c] != 0u), park = ok[c] ^ adv;
                    // lead-in marks (off < ms) land in the ring too; it is cleared when
                    // the walk reaches ms
                    const uint32_t rel = off[c] - ms[c];
                    const uint32_t bit = adv ? (1u << (rel & 31)) : 0u;
                    atomicOr(ring[c] + (kMarkRow + ((rel >> 5) & (kMW - 1))) * kRow, bit);  // the mark ring (a zero bit: no mark)
                    const uint32_t L = adv ? e[c] + bias : 0u;
                    off[c] += L;
                    const int32_t r = (int32_t)sh[c] - (int32_t)L;  // >= -32 (codes <= 32 bits)
                    const bool cr = r < 0;                         // w0 used up: shift the words
                    w0[c] = cr ? w1[c] : w0[c];
                    w1[c] = cr ? nxt[c] : w1[c];
                    sh[c] = (uint32_t)(cr ? r + 32 : r);
                    wn[c] += cr ? 1u : 0u;
                    nxt[c] = ring[c][(wn[c] & 15) * kRow];
                    pk[c] |= park;
                    pW[c] = park ? W[c] : pW[c];
                }
            }
            resolve();
        }
        bool fl[C], ld[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (!on[c] && off[c] >= ms[c]) {  // the lead-in is over: drop its marks
#pragma unroll
                for (uint32_t i = kMarkRow; i < kMarkRow + kMW; ++i) ring[c][i * kRow] = 0u;
                on[c] = true;
            }
            ld[c] = false;
            if (f[c] <= ((off[c] - 1) >> 7) + 3) {
                const uint64_t q = bch[c] + f[c];
                uint4 x = pick_group<G>(pre[c], (uint32_t)q & (G - 1));
                if (!gin[c]) x = walk_fix(a, 4 * q, x);
                ring_put<kRow>(ring[c], f[c] & 3, x);
                ++f[c];
                ld[c] = ((q + 1) & (G - 1)) == 0;  // the group is in the ring: load the next one
            }
            // mark chunk mcount is done once the walk is past it
            fl[c] = mcount[c] < nmc[c] && off[c] >= ms[c] && off[c] - ms[c] >= 128 * (mcount[c] + 1);
            if (fl[c]) {
                uint32_t* slot = ring[c] + (kMarkRow + 4 * (mcount[c] & (kWalkMarkChunks - 1))) * kRow;
                const uint4 m = make_uint4(slot[0], slot[kRow], slot[2 * kRow], slot[3 * kRow]);
#pragma unroll
                for (int i = 0; i < 4; ++i) slot[i * kRow] = 0u;
                rc[c] = ((mcount[c] & 31) ? rc[c] : 0u) + __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w);
#pragma unroll
                for (uint32_t i = 0; i + 1 < GM; ++i) mk[c][i] = mk[c][i + 1];  // shift in (constant indices)
                mk[c][GM - 1] = m;
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {  // the next group's loads, then this round's bitmap stores
            if (!ld[c]) continue;
            const uint64_t q = bch[c] + f[c];
            gin[c] = 4 * (q + G) <= a.nwords;
            if (gin[c]) {
                const uint4* src = reinterpret_cast<const uint4*>(a.words) + q;
#pragma unroll
                for (uint32_t i = 0; i < G; ++i) pre[c][i] = src[i];
            } else {
#pragma unroll
                for (uint32_t i = 0; i < G; ++i) pre[c][i] = walk_load(a, 4 * (q + i));
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (!fl[c]) continue;
            const uint64_t j = seg0[c] * (kSegBits / 128) + mcount[c];
            if ((mcount[c] & (GM - 1)) == GM - 1) {
                uint4* dst = reinterpret_cast<uint4*>(a.bmp) + (j - (GM - 1));
#pragma unroll
                for (uint32_t i = 0; i < GM; ++i)
                    store_nt16(dst + i, mk[c][i]);  // read back by k_sync_select only (16.0 vs 16.3 ms walk, round 3)
            }
            if ((mcount[c] & 31) == 31) a.cnt[j >> 5] = rc[c];
            ++mcount[c];
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (!live[c] || seg1[c] >= a.nseg) continue;
        a.ent[seg1[c]] = a.start + x0[c] + (off[c] - off0[c]);
        a.dirty[seg1[c]] = 1u;
    }
}

// Fix-up of a dirty segment k from its true entry ent[k] (the previous
// segment's exit): walk until the path lands on a boundary of the segment's
// bitmap (the paths agree from there) or leaves the segment. The bitmap words
// the walk passes are rewritten with the walked boundaries (the landing word
// keeps its bits from the landing point on), so the row keeps holding one
// consistent path, and its count follows. A walk that leaves the segment
// hands its end to segment k + 1 for the next iteration.
template <int MODE>
__global__ __launch_bounds__(kSyncThreads) void k_sync_iter(DecArgs a, SyncArgs y, int it) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    copy_lds_table(lds, a.lds_img, a.lds_words);
    const uint32_t* dr = y.dirty[it & 1];
    uint32_t* dw = y.dirty[(it + 1) & 1];
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < y.nseg; k += stride) {
        if (!dr[k]) continue;
        const uint64_t s0 = y.start + k * kSegBits, s1 = s0 + kSegBits;
        uint32_t* bm = y.bmp + k * kBmpWords;
        uint64_t p = y.ent[k];
        uint32_t walked = 0, below = 0, acc = 0, cw = 0;
        uint32_t old = bm[0];  // the row's word cw before the rewrite
        bool landed = false;
        BitReader r;
        br_init(r, a, p + a.bit_adj);
        while (p < s1) {
            const uint32_t d = (uint32_t)(p - s0);
            while ((d >> 5) != cw) {  // words the walk has passed: the walked boundaries replace them
                below += __popc(old);
                bm[cw] = acc;
                acc = 0;
                old = bm[++cw];
            }
            if ((old >> (d & 31)) & 1u) { landed = true; break; }
            acc |= 1u << (d & 31);
            uint32_t sym;
            const uint32_t L = br_next<MODE>(r, a, lds, sym);
            if (L == 0) { atomicOr(a.err, 2u); break; }
            p += L;
            ++walked;
        }
        if (landed) {
            const uint32_t lowm = (1u << ((uint32_t)(p - s0) & 31)) - 1u;
            below += __popc(old & lowm);
            bm[cw] = acc | (old & ~lowm);
            y.cnt[k] = y.cnt[k] - below + walked;
        } else {
            for (; cw < kBmpWords; ++cw) { bm[cw] = acc; acc = 0; }
            y.cnt[k] = walked;
            if (k + 1 < y.nseg) { y.ent[k + 1] = p; dw[k + 1] = 1u; }
            atomicAdd(y.changed, 1u);
        }
    }
}

// Position (0..31) of the r-th (0-based) set bit of m; r < popc(m).
HZ_DEV uint32_t select_bit(uint32_t m, uint32_t r) {
    uint32_t pos = 0, c;
    c = __popc(m & 0xffffu); if (r >= c) { r -= c; pos += 16; m >>= 16; }
    c = __popc(m & 0xffu);   if (r >= c) { r -= c; pos += 8;  m >>= 8; }
    c = __popc(m & 0xfu);    if (r >= c) { r -= c; pos += 4;  m >>= 4; }
    c = __popc(m & 0x3u);    if (r >= c) { r -= c; pos += 2;  m >>= 2; }
    return pos + ((r >= (m & 1u)) ? 1u : 0u);
}

// One workgroup per tile of kSelTileSegs bitmap rows (64 Kbit); thread t
// holds words [8 t, 8 t + 8). A workgroup scan of popcounts numbers every
// boundary from the tile's first (first[] of its first row). Boundary i < nsym
// with i % 8 == 0 is a chain start (raw position, low 16 bits, staged in LDS
// and stored as one contiguous run, the form hz_pack writes),
// i % 2048 == 0 also a block start; boundary nsym is the end of the stream.
constexpr int kSelectThreads = 256;
constexpr uint32_t kSelTileSegs = 16;
constexpr uint32_t kSelTileWords = kSelTileSegs * kBmpWords;  // 2048 = 8 words per thread
constexpr uint32_t kSelMaxChains = kSelTileWords * 32 / kChainSyms + 2;
constexpr int kSelAhead = 1;
__global__ __launch_bounds__(kSelectThreads) void k_sync_select(SyncArgs y, uint64_t nsym, uint64_t nblocks,
                                                                const unsigned long long* first,
                                                                unsigned long long* starts, uint16_t* subs) {
    __shared__ uint16_t ch[kSelMaxChains];
    __shared__ uint32_t wsum[kSelectThreads / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t ntile = (y.nseg + kSelTileSegs - 1) / kSelTileSegs;
    const uint64_t nch_all = (nsym + kChainSyms - 1) / kChainSyms;  // chains with a start inside the stream
    const uint64_t nw = y.nseg * kBmpWords;
    // the next tile's first[] and bitmap words are loaded while this one is processed
    auto load = [&](uint64_t tile, uint64_t& f, uint32_t (&mm)[8]) {
        const uint64_t w0 = tile * kSelTileWords + 8u * threadIdx.x;
        f = first[tile * kSelTileSegs];
        if (w0 + 8 <= nw) {
            const uint4* q = reinterpret_cast<const uint4*>(y.bmp + w0);
            const uint4 a = q[0], b = q[1];
            mm[0] = a.x; mm[1] = a.y; mm[2] = a.z; mm[3] = a.w; mm[4] = b.x; mm[5] = b.y; mm[6] = b.z; mm[7] = b.w;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) mm[i] = w0 + i < nw ? y.bmp[w0 + i] : 0u;
        }
    };
    // kSelAhead tiles in flight per thread (16 GiB Zipf: 1 / 3 / 5 ahead 4.61 / 4.89 / 5.03 ms, round 3)
    uint64_t fn[kSelAhead] = {};
    uint32_t mn[kSelAhead][8];
#pragma unroll
    for (int d = 0; d < kSelAhead; ++d)
        if (blockIdx.x + d * (uint64_t)gridDim.x < ntile) load(blockIdx.x + d * (uint64_t)gridDim.x, fn[d], mn[d]);
    for (uint64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const uint64_t seg0 = tile * kSelTileSegs;
        const uint64_t f0 = fn[0];
        uint32_t m[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) m[i] = mn[0][i];
#pragma unroll
        for (int d = 0; d + 1 < kSelAhead; ++d) {
            fn[d] = fn[d + 1];
#pragma unroll
            for (int i = 0; i < 8; ++i) mn[d][i] = mn[d + 1][i];
        }
        if (tile + kSelAhead * (uint64_t)gridDim.x < ntile)
            load(tile + kSelAhead * (uint64_t)gridDim.x, fn[kSelAhead - 1], mn[kSelAhead - 1]);
        if (f0 > nsym) break;  // workgroup-uniform; later tiles start later still
        const uint64_t w0 = seg0 * kBmpWords + 8u * threadIdx.x;
        uint32_t c[8], tot = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) { c[i] = __popc(m[i]); tot += c[i]; }
        const uint32_t incl = wave_incl_sum(tot);
        if (lane == 63) wsum[wid] = incl;
        __syncthreads();
        uint32_t wpre = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kSelectThreads / 64; ++w) {
            const uint32_t v = wsum[w];
            wpre += w < wid ? v : 0u;
            all += v;
        }
        // 32-bit arithmetic relative to the tile's first boundary f0
        const uint32_t d0 = wpre + incl - tot;  // the thread's first boundary: number f0 + d0
        const uint64_t left = nsym - f0;
        const uint32_t dn = left < 0xffffffffull ? (uint32_t)left : 0xffffffffu;  // boundaries before nsym
        const uint32_t q = (uint32_t)(f0 & 7), qb = (uint32_t)(f0 & (kBlockSyms - 1));
        const uint64_t base = y.start + w0 * 32;
        const uint64_t cb = (f0 + kChainSyms - 1) / kChainSyms;  // first chain starting in the tile
        uint32_t cum[8];
        cum[0] = 0;
#pragma unroll
        for (int h = 1; h < 8; ++h) cum[h] = cum[h - 1] + c[h - 1];
        // the thread's boundary of rank r (0-based): word h = #(cum[1..7] <= r), bit = select in m[h]
        // the select operands pass through an empty asm: a select between two loads
        // of m[] / cum[] is otherwise folded into one dynamically indexed (scratch) load
        auto pos_of = [&](uint32_t r) -> uint64_t {
            uint32_t mh = m[0], ch0 = 0, sh = 0;
            asm volatile("" : "+v"(mh));
#pragma unroll
            for (int h = 1; h < 8; ++h) {
                uint32_t mv = m[h], cv = cum[h];
                asm volatile("" : "+v"(mv), "+v"(cv));
                const bool in = r >= cv;
                mh = in ? mv : mh;
                ch0 = in ? cv : ch0;
                sh = in ? 32u * h : sh;
            }
            return base + sh + select_bit(mh, r - ch0);
        };
        if (d0 <= dn && dn < d0 + tot) starts[nblocks] = pos_of(dn - d0);
        // chain starts: boundaries whose number is a multiple of 8
        for (uint32_t r = (8u - ((q + d0) & 7)) & 7; r < tot && d0 + r < dn; r += 8) {
            const uint32_t d = d0 + r;
            const uint64_t pos = pos_of(r);
            ch[((q + d) >> 3) - (q ? 1u : 0u)] = (uint16_t)pos;
            if (((qb + d) & (kBlockSyms - 1)) == 0) starts[(f0 + d) / kBlockSyms] = pos;
        }
        // the rows hold exactly nsym boundaries: the last codeword ends at the bitmap's end
        if (threadIdx.x == 0 && seg0 + kSelTileSegs >= y.nseg && f0 + all == nsym)
            starts[nblocks] = y.start + y.nseg * kSegBits;
        __syncthreads();
        uint64_t ce = (f0 + all + kChainSyms - 1) / kChainSyms;
        ce = ce < nch_all ? ce : nch_all;
        for (uint64_t t = cb + threadIdx.x; t < ce; t += kSelectThreads) subs[t] = ch[t - cb];
        __syncthreads();
    }
}

// Chains past the stream's end (all in the last block) start at the end, and
// the largest block's bits. The select already wrote every other chain's
// start (low 16 bits of its stream bit, as hz_pack does).
__global__ __launch_bounds__(256) void k_sync_subs(uint64_t nsym, uint64_t nblocks, unsigned long long* starts,
                                                   unsigned long long* sub64) {
    if (nblocks == 0) return;  // no block: nothing to fix (the launcher never sends one; a guard, not a path)
    const uint64_t end = starts[nblocks];
    if (blockIdx.x == 0 && threadIdx.x < kWave) {
        const uint64_t q = (nblocks - 1) * kWave + threadIdx.x;
        const uint64_t raw = sub64[q];
        uint64_t out = 0;
#pragma unroll
        for (int t = 0; t < kChainsPerLane; ++t) {
            const uint64_t c = q * kChainsPerLane + t;
            const uint64_t p = c * kChainSyms < nsym ? (raw >> (16 * t)) & 0xffffu : end & 0xffffu;
            out |= p << (16 * t);
        }
        sub64[q] = out;
    }
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long mx = 0;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nblocks; b += stride) {
        const unsigned long long bits = starts[b + 1] - starts[b];
        mx = bits > mx ? bits : mx;
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t lo = shfl_xor_u32((uint32_t)mx, m), hi = shfl_xor_u32((uint32_t)(mx >> 32), m);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(starts + nblocks + 1, mx);
}

uint64_t index_scratch_words(uint64_t payload_bytes, uint64_t start_bit) {
    const uint64_t bits = payload_bytes * 8 > start_bit ? payload_bytes * 8 - start_bit : 0;
    const uint64_t nseg = (bits + kSegBits - 1) / kSegBits;
    const uint64_t ntiles = (nseg + kScanTile - 1) / kScanTile;
    // ent, cnt, first (u64), bitmap (kBmpWords u32), dirty[2] (u32), counter, tiles
    return nseg * (3 + kBmpWords / 2 + 1) + 1 + ntiles + 24;
}

// Common tail of the index build, after the boundary bitmap and the dirty
// entries exist: fix-ups to a fixed point, count scan, select, subs.
template <int MODE>
static hipError_t finish_index(const DecArgs& a, SyncArgs y, unsigned long long* first, unsigned long long* tiles,
                               unsigned long long* d_index, uint32_t* h_changed, uint32_t lds, int ncu,
                               hipStream_t s) {
    {
        hipError_t e = ensure_lds_limit((const void*)k_sync_iter<MODE>, kLdsBytes);
        if (e != hipSuccess) return e;
    }
    const uint64_t cap = (uint64_t)ncu * (lds ? (kLdsBytes / lds < 2 ? 1 : 2) : 2);
    const uint64_t wgs = grid_clamp((y.nseg + kSyncThreads - 1) / kSyncThreads, cap);
    // resolve entries until no walk leaves its segment (host loop; typically 1-2 passes)
    for (int it = 0;; ++it) {
        hipError_t e = hipMemsetAsync(y.changed, 0, 4, s);
        if (e != hipSuccess) return e;
        if ((e = hipMemsetAsync(y.dirty[(it + 1) & 1], 0, 4 * y.nseg, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_sync_iter<MODE>, dim3(wgs), dim3(kSyncThreads), lds, s, a, y, it);
        if ((e = hipMemcpyAsync(h_changed, y.changed, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        if (*h_changed == 0 || it > (int)y.nseg) break;
    }
    hipError_t e = launch_scan(y.cnt, y.nseg, tiles, first, 0xffffffffull, 0ull, s);
    if (e != hipSuccess) return e;
    uint16_t* subs = reinterpret_cast<uint16_t*>(d_index + index_sub_offset(a.nblocks));
    // end bit = all ones unless the payload holds nsym codewords (k_sync_select writes it then)
    if ((e = hipMemsetAsync(d_index + a.nblocks, 0xff, 8, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(d_index + a.nblocks + 1, 0, 8, s)) != hipSuccess) return e;
    {
        // tiles in order over a grid-stride loop: a workgroup stops at the first tile past the stream
        uint64_t sg = (y.nseg + kSelTileSegs - 1) / kSelTileSegs;
        sg = sg < (uint64_t)ncu * 8 ? sg : (uint64_t)ncu * 8;
        hipLaunchKernelGGL(k_sync_select, dim3(sg), dim3(kSelectThreads), 0, s, y, a.nsym, a.nblocks,
                           (const unsigned long long*)first, d_index, subs);
    }
    const uint64_t sw = grid_clamp((a.nblocks + 255) / 256, (uint64_t)ncu * 4);
    hipLaunchKernelGGL(k_sync_subs, dim3(sw), dim3(256), 0, s, a.nsym, a.nblocks, d_index,
                       d_index + index_sub_offset(a.nblocks));
    return hipGetLastError();
}

// Boundary bitmap by the LUT walkers (one or two 4096-bit segments per lane).
template <int MODE>
static hipError_t scan_lut(const DecArgs& a, SyncArgs y, uint32_t lds, int ncu, hipStream_t s) {
    {
        hipError_t e = ensure_lds_limit((const void*)k_sync_scan<MODE>, kLdsBytes);
        if (e != hipSuccess) return e;
    }
    // 16-wave workgroups: one table copy per workgroup, as many waves as a CU holds
    const uint64_t cap = (uint64_t)ncu * (lds ? (kLdsBytes / lds < 2 ? 1 : 2) : 2);
    const uint64_t wgs = grid_clamp((y.nseg + kSyncThreads - 1) / kSyncThreads, cap);
    // two segments per lane where the pipelined decoder's table shape holds
    const bool two = MODE == DEC_LUT && a.max_len <= 32 && a.max_len <= a.k + a.level_bits;
    if (two) {
        hipError_t e = ensure_lds_limit((const void*)k_sync_scan2, kLdsBytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_sync_scan2, dim3(wgs), dim3(kSyncThreads), lds, s, a, y);
    } else {
        hipLaunchKernelGGL(k_sync_scan<MODE>, dim3(wgs), dim3(kSyncThreads), lds, s, a, y);
    }
    return hipGetLastError();
}

// Boundary bitmap by the long-chain walker.
static hipError_t scan_walk(const Tables& t, const DecArgs& a, SyncArgs y, int ncu, hipStream_t s) {
    hipError_t e = ensure_lds_limit((const void*)k_idx_walk, (int)kWalkLdsRingBytes);  // + the static table
    if (e != hipSuccess) return e;
    WalkArgs w;
    w.words = a.words; w.nwords = a.nwords; w.bit_adj = a.bit_adj;
    w.start = y.start; w.nseg = y.nseg;
    const uint64_t per_wg = (uint64_t)kWalkWaves * 64 * kWalkChains;
    const uint64_t target = per_wg * (uint64_t)ncu;
    w.spc = (y.nseg + target - 1) / target;
    w.nchains = (y.nseg + w.spc - 1) / w.spc;
    w.lds_img = t.d_walk_lds; w.lds_words = t.walk_lds_bytes / 4;
    w.k = t.walk_k; w.bias = t.walk_bias; w.esc = reinterpret_cast<const uint8_t*>(t.d_walk_esc); w.m = t.walk_m;
    w.bmp = y.bmp; w.cnt = y.cnt; w.ent = y.ent; w.dirty = y.dirty[0]; w.lead = kWalkLead;
    w.w8_img = nullptr; w.w8_words = 0; w.k8 = 0;
    // chains tid and tid + T of every thread
    const uint64_t threads_needed = (w.nchains + kWalkChains - 1) / kWalkChains;
    uint64_t wgs = (threads_needed + kWalkWaves * 64 - 1) / (kWalkWaves * 64);
    wgs = wgs ? wgs : 1;
    hipLaunchKernelGGL(k_idx_walk, dim3(wgs), dim3(kWalkWaves * 64), kWalkLdsRingBytes, s, w);
    return hipGetLastError();
}

// Every code 16 bits: codeword i starts at start + 16 i, so the index is
// arithmetic (no walk). Same layout as k_pack_fixed16 writes.
__global__ __launch_bounds__(256) void k_idx_fixed16(uint64_t start, uint64_t nsym, uint64_t nblocks,
                                                     unsigned long long* index) {
    unsigned long long* sub = index + index_sub_offset(nblocks);
    const uint64_t nl = nblocks * kWave;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nl; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t blk = j / kWave;
        const uint32_t lane = (uint32_t)(j % kWave);
        const uint64_t left = nsym - blk * kBlockSyms;
        const uint32_t cnt = (uint32_t)(left < (uint64_t)kBlockSyms ? left : (uint64_t)kBlockSyms);
        uint64_t v = 0;
#pragma unroll
        for (int c = 0; c < kChainsPerLane; ++c) {
            const uint32_t at = kSPT * lane + kChainSyms * c;
            v |= (uint64_t)(((uint32_t)(start + blk * kBlockSyms * 16) + 16 * (at < cnt ? at : cnt)) & 0xffffu)
                 << (16 * c);
        }
        sub[j] = v;
        if (lane == 0) index[blk] = start + blk * kBlockSyms * 16;
        if (j == 0) {
            index[nblocks] = start + 16 * nsym;
            index[nblocks + 1] = 16ull * (nsym < (uint64_t)kBlockSyms ? nsym : (uint64_t)kBlockSyms);
        }
    }
}

hipError_t launch_index_build(const Tables& t, const uint8_t* d_payload, uint64_t payload_bytes, uint64_t start_bit,
                              uint64_t nsym, unsigned long long* d_index, unsigned long long* d_scratch, uint32_t* d_err,
                              uint32_t* h_scratch, int ncu, hipStream_t s) {
    if (nsym == 0) return hipSuccess;
    DecArgs a;
    fill_dec_args(a, t, d_payload, payload_bytes, nsym);
    a.starts = nullptr; a.subs = nullptr; a.out = nullptr; a.err = d_err;
    const uint64_t bits = payload_bytes * 8 > start_bit ? payload_bytes * 8 - start_bit : 0;
    SyncArgs y;
    y.start = start_bit;
    y.nseg = (bits + kSegBits - 1) / kSegBits;
    if (y.nseg == 0) return hipErrorInvalidValue;
    unsigned long long* p = d_scratch;
    y.ent = p; p += y.nseg;
    y.cnt = p; p += y.nseg;
    unsigned long long* first = p; p += y.nseg;
    p += ((128 - (reinterpret_cast<uintptr_t>(p) & 127)) & 127) / 8;  // 128-byte aligned bitmap (run stores)
    y.bmp = reinterpret_cast<uint32_t*>(p); p += y.nseg * (kBmpWords / 2);
    y.dirty[0] = reinterpret_cast<uint32_t*>(p);
    y.dirty[1] = y.dirty[0] + y.nseg;
    p += y.nseg;
    y.changed = reinterpret_cast<uint32_t*>(p); p += 1;
    unsigned long long* tiles = p;
    if (t.dec_mode == DEC_FIXED16) {
        const uint64_t w = grid_clamp((a.nblocks * kWave + 255) / 256, (uint64_t)ncu * 8);
        hipLaunchKernelGGL(k_idx_fixed16, dim3(w), dim3(256), 0, s, start_bit, nsym, a.nblocks, d_index);
        return hipGetLastError();
    }
    const uint32_t lds = t.dec_lds_bytes;
    hipError_t e = hipMemsetAsync(y.dirty[0], 0, 4 * y.nseg, s);  // the scan marks the segments to check
    if (e != hipSuccess) return e;
    const bool walk = t.walk_lds_bytes > 0 && a.nwords >= 4;
    if (walk) e = scan_walk(t, a, y, ncu, s);
    else if (t.dec_mode == DEC_DENSE) e = scan_lut<DEC_DENSE>(a, y, lds, ncu, s);
    else e = scan_lut<DEC_LUT>(a, y, lds, ncu, s);
    if (e != hipSuccess) return e;
    if (t.dec_mode == DEC_DENSE) return finish_index<DEC_DENSE>(a, y, first, tiles, d_index, h_scratch, lds, ncu, s);
    return finish_index<DEC_LUT>(a, y, first, tiles, d_index, h_scratch, lds, ncu, s);
}

// ===========================================================================
// Index-less decode in CHAIN BLOCKS: the `extract` path of a reference file
// (Decompressor.cu:259-291 decodes it serially; the format carries no index,
// Compressor.cu:427-601). Stream-ordered end to end (no host synchronisation):
//   k_chain_walk    : one walk CHAIN per lane over cbits payload bits (lengths
//                     only: k_idx_walk's 4-bit table, payload ring, escape
//                     parking), starting kWalkLead bits early so it has
//                     resynchronised by its first bit. From its ENTRY (the first
//                     codeword start at or after the chain's first bit) it
//                     records the stream bit of every 8th codeword (u16 low
//                     bits, the block index's sub[] format) and of every 2048th
//                     (u64 checkpoint: a decode BLOCK of 256 records); per chain
//                     its EXIT (the first codeword start at or after its end)
//                     and codeword count
//   k_chain_fix     : a chain whose entry disagrees with the previous chain's
//                     exit walks the true path from that exit until it lands on
//                     one of its own records: the codewords before it are the
//                     chain's HEAD (decoded serially by k_chain_tail), the
//                     records from it on are valid. One grid pass, then one
//                     workgroup iterating on the chains whose exit moved
//                     (rare: the lead-in resynchronises with P ~ 1 - 4e-4)
//   k_scan_*        : output index of every chain, first decode block of every chain
//   k_chain_meta    : block descriptors (start, end, records, output index)
//   k_chain_decode  : k_decode's pipelined block decoder (two blocks per wave,
//                     quad walks, hot heads, gathers consumed a quad later) over
//                     the chain blocks, each written at its chain's output index
//   k_chain_tail    : heads, records past a chain's capacity, the end bit
// Records are chain-phased: every piece but a chain's last decodes exactly 8
// codewords, so the decoder has no partial pieces at segment ends.
// ===========================================================================
constexpr int kChainWalkWaves = 16;
constexpr uint32_t kChainRecs = 256;  // records per decode block (2048 codewords)
// Per-lane payload ring of k_chain_walk: 4 chunks of 4 words, then a copy of word 0 (so the window's two
// words q, q + 1 never wrap).
constexpr uint32_t kSegRing = 16 + 1;
// Ring word j of lane t at LDS word j * kRingRow + t: all of a lane's words lie in bank t mod 32, so the
// window's two words (one ds_read2st64_b32) and the chunk stores never conflict between lanes (a ring
// per lane at an odd stride: random banks, 12.43 vs 12.10 ms at 16 GiB Zipf, A/B in one run).
constexpr uint32_t kRingRow = kChainWalkWaves * 64;

struct ChainBlk {
    unsigned long long b0, b1;  // stream bits of the block's first record and of the one after its last
    unsigned long long rec;     // index of the block's first record in ChainArgs::rec
    long long out;              // output index of the block's first record's first symbol
    uint32_t lo, hi;            // valid records [lo, hi) of the block
    uint32_t last;              // symbols of record hi - 1 (8 unless it is the chain's last codewords)
    uint32_t lhl;               // lo | hi << 9 | last << 18: one SGPR per block in the block decoder
};
static_assert(sizeof(ChainBlk) == 48, "ChainBlk");

struct ChainArgs {
    uint64_t nchains, cbits;         // chain c walks payload bits [pbeg + c cbits, min(pbeg + (c + 1) cbits, pend))
    uint64_t pbeg, pend;             // the part of the payload (bits after start) these chains cover
    uint64_t start;                  // stream bit of the first symbol
    uint64_t entry0;                 // true entry of chain 0 (~0: its walked entry -- the stream's start)
    uint32_t bpc, cap;               // decode blocks per chain, records per chain (kChainRecs * bpc)
    uint16_t* rec;                   // [nchains][cap] low 16 bits of the stream bit of chain codeword 8 r
    unsigned long long* ckpt;        // [nchains][bpc + 1] stream bit of record 256 j; after the last block, the exit
    unsigned long long* ent;         // [nchains] walked entry
    unsigned long long* xit;         // [nchains] walked exit (first codeword start >= the chain's end)
    unsigned long long* txit;        // [nchains] true exit (k_chain_fix): the next chain's true entry
    unsigned long long* cnt;         // [nchains] codewords from the walked entry to the exit
    unsigned long long* tcnt;        // [nchains] codewords of the chain on the true path
    unsigned long long* nblk;        // [nchains] decode blocks of the chain
    unsigned long long* first;       // [nchains] output index of the chain's first true codeword
    unsigned long long* bbase;       // [nchains] the chain's first decode block
    uint32_t* hd;                    // [nchains] head: true codewords before the first valid record
    uint32_t* r0;                    // [nchains] first valid record (nrec: none)
    uint32_t* list[2];               // k_chain_fix_loop: chains to check, ping-pong
    uint32_t* lcnt;                  // [2] their counts
    ChainBlk* blk;                   // [nchains * bpc] decode block descriptors
    unsigned long long* info;        // [0] decode blocks, [1] largest block (bits), [2] end bit, [3] codewords,
                                     // [4] true exit of the last chain, [5] entry of chain 0 in use
    uint32_t* err;
};

// The ring holds its 16 words in DESCENDING order: ring word u (bit 32 u .. 32 u + 31 of the ring) at
// index 15 - (u & 15), plus index 16 = a copy of index 0, so a window's two words are adjacent
// (ds_read2_b32) and never wrap. The walk keeps its position as m = kRingM0 - p (decreasing): then the
// pair's lower index is (m >> 5) & 15 and the funnel shift is m itself (kRingM0 = 0 mod 512; m's low 5
// bits are 31 - ((p - 1) & 31)): two VALU for the address, none for the shift.
constexpr uint32_t kRingM0 = 0x7fffffe0u;
HZ_DEV uint32_t seg_window(const uint32_t* ring, uint32_t m) {
    uint32_t i;
    asm("v_bfe_u32 %0, %1, 5, 4" : "=v"(i) : "v"(m));  // (kept whole: the compiler's shift + and + add is one more)
    const uint32_t* w = ring + i * kRingRow;
    return __builtin_amdgcn_alignbit(w[kRingRow], w[0], m);
}

// Chunk slot q of a ring (ring words 4 q .. 4 q + 3), byte-swapped, descending; slot 3's last word
// (index 0) also at index 16.
HZ_DEV void seg_ring_put(uint32_t* ring, uint32_t q, const uint4& x) {
    const uint32_t v[4] = {bswap32(x.x), bswap32(x.y), bswap32(x.z), bswap32(x.w)};
#pragma unroll
    for (int i = 0; i < 4; ++i) ring[(15 - 4 * q - i) * kRingRow] = v[i];
    if (q == 3) ring[16 * kRingRow] = v[3];
}

// The ring's loader state: the next chunk f and the 64-byte register group it comes from.
struct SegFeed {
    uint4 pre[kWalkGroup];
    bool gin;
    uint64_t bch;  // payload chunk of ring chunk 0
    uint32_t f;    // next chunk to put (chunks below f are in the ring)
};

// Chunks 0..2 of a ring whose bit 0 is payload word 4 * bch, and the group holding chunk 3.
HZ_DEV void seg_feed_init(const WalkArgs& a, uint32_t* ring, SegFeed& fd, uint64_t bch) {
    constexpr uint32_t G = kWalkGroup;
    fd.bch = bch;
    uint4 v[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) v[g] = walk_load(a, 4 * (bch + g));
    const uint64_t gb = (bch + 3) & ~(uint64_t)(G - 1);
    fd.gin = 4 * (gb + G) <= a.nwords && gb < a.nwords;
#pragma unroll
    for (uint32_t g = 0; g < G; ++g) fd.pre[g] = walk_load(a, 4 * (gb + g));
#pragma unroll
    for (int g = 0; g < 3; ++g) seg_ring_put(ring, (uint32_t)g, walk_fix(a, 4 * (bch + g), v[g]));
    fd.f = 3;
}

// Once per round: chunk f goes into the ring when the chain at p no longer needs chunk f - 4; the
// next group is loaded once the current one is in the ring.
HZ_DEV void seg_feed(const WalkArgs& a, uint32_t* ring, SegFeed& fd, uint32_t p) {
    constexpr uint32_t G = kWalkGroup;
    bool ld = false;
    if (fd.f <= ((p - 1) >> 7) + 3) {
        const uint64_t q = fd.bch + fd.f;
        uint4 x = pick_group<G>(fd.pre, (uint32_t)q & (G - 1));
        if (!fd.gin) x = walk_fix(a, 4 * q, x);
        seg_ring_put(ring, fd.f & 3, x);
        ++fd.f;
        ld = ((q + 1) & (G - 1)) == 0;
    }
    if (ld) {
        const uint64_t q = fd.bch + fd.f;
        fd.gin = 4 * (q + G) <= a.nwords;
        if (fd.gin) {
            const uint4* src = reinterpret_cast<const uint4*>(a.words) + q;
#pragma unroll
            for (uint32_t i = 0; i < G; ++i) fd.pre[i] = src[i];
        } else {
#pragma unroll
            for (uint32_t i = 0; i < G; ++i) fd.pre[i] = walk_load(a, 4 * (q + i));
        }
    }
}

// Steps per round of the walk: two halves of 7 steps, so a half-round (plus its escape gather) moves
// at most 8 codewords and takes at most one record. (Segment walk, 16 GiB Zipf, round 4: 10 / 12 / 14
// steps 14.4 / 13.9 / 13.4 ms; 3 parts of 6 steps 14.4 ms; a second chunk fed per round 15.2 ms.)
constexpr int kSegSteps = 14;
static_assert(kSegSteps / kWalkHalves + 1 <= 8, "one record per half-round");

// Length of the code at view bit P through the decode LUT in global memory (k_chain_walk<DEEP>: codes
// longer than the escape table's m bits; rare, never on the path of codebooks within m bits).
HZ_DEV uint32_t deep_len(const WalkArgs& a, uint64_t P) {
    const uint64_t w = P >> 5;
    const uint32_t sh = (uint32_t)(P & 31);
    const uint32_t w0 = w < a.nwords ? bswap32(a.words[w]) : 0u;
    const uint32_t w1 = w + 1 < a.nwords ? bswap32(a.words[w + 1]) : 0u;
    const uint32_t w2 = w + 2 < a.nwords ? bswap32(a.words[w + 2]) : 0u;
    const uint64_t win = ((((uint64_t)w0 << 32) | w1) << sh) | (sh ? ((uint64_t)w2 << sh) >> 32 : 0ull);
    uint32_t e = a.lut1[(uint32_t)(win >> (64 - a.lutk))];
    uint32_t D = (uint32_t)a.lutk;
    while (!(e >> 31)) {
        const uint32_t nb = (e >> 5) & 15u;
        const uint32_t idx = (e >> 10) + (uint32_t)((win << D) >> (64 - nb));
        e = idx < kLutGlobal ? a.lut1[idx] : a.lut2[idx - kLutGlobal];
        D += nb;
    }
    return lut_leaf_len(e);
}

template <bool DEEP>
__global__ __launch_bounds__(kChainWalkWaves * 64) void k_chain_walk(WalkArgs a, ChainArgs y) {
    // the byte length table (build_walk8: 2^16 windows at most, 64 KiB) at LDS address 0, the rings and
    // record buffers after it (+ one zero word: the byte a lane past its limit reads)
    __shared__ __attribute__((aligned(16))) uint32_t wtab[(1u << 16) / 4 + 4];
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    if (threadIdx.x == 0) wtab[(1u << 16) / 4] = 0;
    copy_lds_table(wtab, a.w8_img, a.w8_words);
    const uint8_t* lds8 = reinterpret_cast<const uint8_t*>(wtab);
    const uint32_t k8 = (uint32_t)a.k8;
    uint32_t* ring = lds + threadIdx.x;
    uint16_t* rbuf = reinterpret_cast<uint16_t*>(lds + kSegRing * kRingRow) + 8 * threadIdx.x;
    const uint64_t ch = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = ch < y.nchains;
    const uint64_t chc = live ? ch : 0;
    const uint64_t cs = y.pbeg + chc * y.cbits;
    const uint64_t ce = cs + y.cbits < y.pend ? cs + y.cbits : y.pend;
    const uint64_t x0 = cs - (cs < a.lead ? cs : a.lead);  // lead-in: resynchronised by cs (mostly)
    const uint64_t P0 = y.start + a.bit_adj + x0;
    SegFeed fd;
    seg_feed_init(a, ring, fd, (P0 >> 7) - 1);  // one chunk before the walk (wraps to ~0 at the payload's start: zeros)
    uint32_t p = (uint32_t)(P0 - 128 * fd.bch);    // ring bit position of the walk (>= 128)
    const uint64_t abs0 = y.start + x0 - p;        // absolute stream bit of ring position q: abs0 + q
    const uint32_t end = live ? p + (uint32_t)(ce - x0) : p;
    const uint32_t csr = p + (uint32_t)(cs - x0);  // the chain's first bit
    uint16_t* recp = y.rec + chc * y.cap;
    unsigned long long* ckp = y.ckpt + chc * (y.bpc + 1);
    uint32_t rj = 0;  // records so far (record r = chain codeword 8 r)
    uint32_t cc = 0;  // codewords since the entry
    // record r: the codeword's stream bit, low 16 bits, into the lane's 16-byte LDS buffer (stored 8 at
    // a time); every 256th also as a u64 checkpoint (a decode block's start). Past the capacity
    // nothing is stored (k_chain_tail decodes those codewords).
    // (the buffer write needs no capacity test: rows past the capacity are never stored)
    auto rec_put = [&](uint32_t rp) {
        const uint64_t ab = abs0 + rp;
        rbuf[rj & 7] = (uint16_t)ab;
        const bool in = rj < y.cap;
        const bool row = in & ((rj & 7) == 7);
        const bool ck = (in & ((rj & (kChainRecs - 1)) == 0)) | (rj == y.cap);  // at the capacity: the first codeword past it
        if (row | ck) {  // one branch for both rare stores
            if (row) *reinterpret_cast<uint4*>(recp + (rj & ~7u)) = *reinterpret_cast<const uint4*>(rbuf);
            if (ck) ckp[in ? rj / kChainRecs : y.bpc] = ab;
        }
        ++rj;
    };
    bool on = p >= csr;  // past the lead-in: counting from the entry
    uint32_t ent = p;
    if (on && p < end) rec_put(p);
    uint32_t m = kRingM0 - p;  // the walk's position, descending (seg_window)
    const uint32_t mend = kRingM0 - end;
    for (;;) {
        if (!__any(m > mend)) break;
        const uint32_t fill = 128 * fd.f - 96;  // filled data: both window words lie below p + 64
        const uint32_t mlim = kRingM0 - min(on ? end : csr, fill);  // a step needs m > mlim
#pragma unroll
        for (int half = 0; half < kWalkHalves; ++half) {
            // the half's codewords end at q[0 .. na - 1] (the advancing steps are a prefix: a chain
            // that parks or reaches its limit stays put for the rest of the half), then at m for an escape
            // A step reads the code's length (0: an escape), or, past the limit, the zero byte after the
            // table: a chain that reads 0 stays put and reads 0 again, so the advancing steps are a prefix
            // with no park flags, and an escape's window is the half's last (no lane masks and no SALU
            // per step: 281 vs 330 clocks per step in tools/microbench/mb_walk_step.hip).
            constexpr int S = kSegSteps / kWalkHalves;
            uint32_t q[S];
            uint32_t na = 0, W = 0, e = 0;
            bool ok = false;
            // issue priority over the dependent steps and the escape gather's issue, normal for the
            // record select, feed and stores (extract 21.14-21.45 -> 20.48-20.62 ms, A/B)
            __builtin_amdgcn_s_setprio(2);
#pragma unroll
            for (int t = 0; t < S; ++t) {
                ok = m > mlim;
                W = seg_window(ring, m);
                e = lds8[ok ? W >> (32 - k8) : 1u << 16];
                HZ_WALK_FENCE();
                m -= e;
                na += e != 0u ? 1u : 0u;
                q[t] = m;
            }
            const bool pk = ok & (e == 0u);  // parked on an escape
            const uint32_t nm = na + (pk ? 1u : 0u);
            // the escape's gather by every lane (the others read byte 0): no branch, and its wait sits at
            // the first use, behind the record select (11.2 vs 11.5 ms, A/B in one run)
            uint32_t ev = a.esc[pk ? W >> (32 - a.m) : 0u];
            __builtin_amdgcn_s_setprio(0);
            // record of codeword 8 i: it starts where the half's codeword j1 ends (1-based): q[j1 - 1],
            // or m after the escape when j1 is the escaped codeword (jj = 0); a three-level select
            const uint32_t j1 = 8u - (cc & 7u);
            const uint32_t jj = j1 <= na ? j1 : 0u;
            static_assert(S <= 7, "q[jj - 1] for jj < 8");
            uint32_t v[8];
            v[0] = 0;
#pragma unroll
            for (int t = 0; t < 7; ++t) v[t + 1] = t < S ? q[t < S ? t : 0] : 0u;
            const bool b0 = jj & 1u, b1 = jj & 2u, b2 = jj & 4u;
            const uint32_t a0 = b0 ? v[1] : v[0], a1 = b0 ? v[3] : v[2], a2 = b0 ? v[5] : v[4], a3 = b0 ? v[7] : v[6];
            const uint32_t sel = b2 ? (b1 ? a3 : a2) : (b1 ? a1 : a0);
            if constexpr (DEEP) {  // the escape table holds 0: a code longer than its m bits (decode LUT)
                const bool deep = pk & (ev == 0u);
                if (__any(deep)) {
                    if (deep) ev = deep_len(a, abs0 + (kRingM0 - m) + a.bit_adj);
                }
            }
            m -= pk ? ev : 0u;
            // the round's feed right after its last escape wait and before the half's record stores: its
            // wait on the group registers then waits for no fresh store (12.23 vs 12.60 ms at the round's
            // end, 16 GiB Zipf, A/B in one run; without the record stores 11.67 ms)
            if (half == kWalkHalves - 1) seg_feed(a, ring, fd, kRingM0 - m);
            const uint32_t pc = kRingM0 - m;
            const uint32_t rm = jj ? sel : m;
            // the lead-in's last step lands on the entry: the entry is the record, counting starts there
            const bool enter = !on & (pc >= csr);
            const uint32_t rp = on ? kRingM0 - rm : pc;
            const bool rec = (on ? j1 <= nm : enter) & (rp < end);  // (a codeword starting at the end is the next chain's)
            ent = enter ? pc : ent;
            cc = on ? cc + nm : 0u;
            on |= enter;
            if (rec) rec_put(rp);
        }
    }
    p = kRingM0 - m;
    if (!live) return;
    if ((rj & 7u) && (rj & ~7u) < y.cap)  // the last, partial group of records
        *reinterpret_cast<uint4*>(recp + (rj & ~7u)) = *reinterpret_cast<const uint4*>(rbuf);
    if (rj <= y.cap) ckp[(rj + kChainRecs - 1) / kChainRecs] = abs0 + p;  // after the last block: the exit
    y.ent[ch] = abs0 + (on ? ent : p);
    y.xit[ch] = abs0 + p;
    y.txit[ch] = abs0 + p;
    y.cnt[ch] = cc;
}

// Stream bit of record r (< cap) of chain c.
HZ_DEV uint64_t chain_rec_pos(const ChainArgs& y, uint64_t c, uint32_t r) {
    const uint64_t ck = y.ckpt[c * (y.bpc + 1) + r / kChainRecs];
    return ck + (uint16_t)(y.rec[c * y.cap + r] - (uint16_t)ck);
}

HZ_DEV uint32_t chain_nrec(uint64_t n) { return (uint32_t)((n + 7) / 8); }
HZ_DEV uint64_t chain_blocks(uint32_t navail, uint32_t r0) {
    const uint32_t nb = (navail + kChainRecs - 1) / kChainRecs, j0 = r0 / kChainRecs;
    return r0 < navail ? nb - j0 : 0;
}

// Chain i against chain i - 1's true exit (its true entry; chain 0: entry0). When that is not the walked entry,
// walk the true path until it lands on one of the chain's records (from there both paths agree):
// head, first valid record, true count and decode blocks follow. The chain's true exit is its walked
// exit when a record was met, else where the true path left the chain (the whole chain is head).
// Returns true when the true exit changed (the next chain must be checked again). Idempotent: a chain
// checked against a stale entry (another chain's exit moving concurrently) is checked again.
template <int MODE>
HZ_DEV bool chain_fix_one(const DecArgs& a, const ChainArgs& y, const uint32_t* lds, uint64_t i) {
    uint64_t p = i ? y.txit[i - 1] : y.entry0;
    const uint64_t n = y.cnt[i];
    const uint32_t nrec = chain_nrec(n), navail = nrec < y.cap ? nrec : y.cap;
    uint32_t rr = 0;
    uint64_t h = 0;
    bool met = p == y.ent[i];
    if (!met) {
        const uint64_t cend = y.pbeg + (i + 1) * y.cbits;
        const uint64_t ce = y.start + (cend < y.pend ? cend : y.pend);
        BitReader r;
        br_init(r, a, p + a.bit_adj);
        uint64_t R = navail ? chain_rec_pos(y, i, 0) : ~0ull;
        for (;;) {
            while (rr < navail && R < p) {
                ++rr;
                R = rr < navail ? chain_rec_pos(y, i, rr) : ~0ull;
            }
            if (rr < navail && R == p) { met = true; break; }
            if (p >= ce) break;
            uint32_t sym;
            const uint32_t L = br_next<MODE>(r, a, lds, sym);
            if (L == 0) { atomicOr(a.err, 2u); break; }
            p += L;
            ++h;
        }
    }
    y.hd[i] = (uint32_t)h;
    y.r0[i] = met ? rr : nrec;
    y.tcnt[i] = met ? h + n - 8ull * rr : h;
    y.nblk[i] = met ? chain_blocks(navail, rr) : 0;
    const uint64_t tx = met ? y.xit[i] : p;
    if (tx != y.txit[i]) {
        y.txit[i] = tx;
        return true;
    }
    return false;
}

// Every chain once (chain 0 starts on its walked entry unless entry0 says otherwise); chains whose
// predecessor's exit moved go on a list.
template <int MODE>
__global__ __launch_bounds__(kSyncThreads) void k_chain_fix(DecArgs a, ChainArgs y) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    copy_lds_table(lds, a.lds_img, a.lds_words);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < y.nchains; i += stride) {
        if (i == 0 && y.entry0 == ~0ull) {
            const uint64_t n = y.cnt[0];
            const uint32_t nrec = chain_nrec(n);
            y.hd[0] = 0;
            y.r0[0] = 0;
            y.tcnt[0] = n;
            y.nblk[0] = chain_blocks(nrec < y.cap ? nrec : y.cap, 0);
            y.txit[0] = y.xit[0];
            continue;
        }
        if (chain_fix_one<MODE>(a, y, lds, i) && i + 1 < y.nchains) {
            const uint32_t s = atomicAdd(y.lcnt, 1u);
            y.list[0][s] = (uint32_t)(i + 1);
        }
    }
}

// The listed chains again, one workgroup, until no exit moves: each pass moves the frontier of a run
// of unsynchronised chains by one chain (bounded by nchains passes).
template <int MODE>
__global__ __launch_bounds__(kSyncThreads) void k_chain_fix_loop(DecArgs a, ChainArgs y) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    copy_lds_table(lds, a.lds_img, a.lds_words);
    for (uint64_t it = 0; it <= y.nchains; ++it) {
        const uint32_t cur = (uint32_t)(it & 1);
        const uint32_t n = __hip_atomic_load(y.lcnt + cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n == 0) break;  // every thread read the same count (the adds happened before the barrier)
        for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) {
            const uint64_t i = y.list[cur][j];
            if (chain_fix_one<MODE>(a, y, lds, i) && i + 1 < y.nchains) {
                const uint32_t s = atomicAdd(y.lcnt + (cur ^ 1u), 1u);
                y.list[cur ^ 1u][s] = (uint32_t)(i + 1);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(y.lcnt + cur, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
    }
}

// Decode block descriptors of every chain (after the scans of tcnt -> first and nblk -> bbase), the
// largest block and the number of blocks.
__global__ __launch_bounds__(256) void k_chain_meta(ChainArgs y) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t maxb = 0;
    if (c < y.nchains) {
        const uint64_t nb = y.nblk[c];
        if (c + 1 == y.nchains) {  // the part's summary
            y.info[0] = y.bbase[c] + nb;
            y.info[3] = y.first[c] + y.tcnt[c];
            y.info[4] = y.txit[c];
            y.info[5] = y.entry0 != ~0ull ? y.entry0 : y.ent[0];  // the entry in use
        }
        if (nb) {
            const uint64_t n = y.cnt[c];
            const uint32_t nrec = chain_nrec(n), navail = nrec < y.cap ? nrec : y.cap;
            const uint32_t r0 = y.r0[c], j0 = r0 / kChainRecs;
            const long long out0 = (long long)(y.first[c] + y.hd[c]) - 8ll * r0;  // output index of record 0
            const unsigned long long* ckp = y.ckpt + c * (y.bpc + 1);
            ChainBlk* bk = y.blk + y.bbase[c];
            for (uint32_t j = j0; j < j0 + (uint32_t)nb; ++j) {
                ChainBlk d;
                d.b0 = ckp[j];
                d.b1 = ckp[j + 1];
                d.rec = c * y.cap + (uint64_t)kChainRecs * j;
                d.out = out0 + 8ll * kChainRecs * j;
                d.lo = r0 > kChainRecs * j ? r0 - kChainRecs * j : 0u;
                const uint32_t hi = navail - kChainRecs * j;
                d.hi = hi < kChainRecs ? hi : kChainRecs;
                // the chain's last record (not cut by the capacity) holds n - 8 (nrec - 1) codewords
                d.last = nrec <= y.cap && kChainRecs * j + d.hi == nrec ? (uint32_t)(n - 8ull * (nrec - 1)) : 8u;
                d.lhl = d.lo | d.hi << 9 | d.last << 18;
                bk[j - j0] = d;
                maxb = d.b1 - d.b0 > maxb ? d.b1 - d.b0 : maxb;
            }
        }
    }
    // one atomic per wave
#pragma unroll
    for (int mm = 1; mm < 64; mm <<= 1) {
        const uint64_t o = ((uint64_t)shfl_xor_u32((uint32_t)(maxb >> 32), mm) << 32) | shfl_xor_u32((uint32_t)maxb, mm);
        maxb = o > maxb ? o : maxb;
    }
    if ((threadIdx.x & 63) == 0 && maxb) atomicMax(y.info + 1, (unsigned long long)maxb);
}

// Block metadata of the chain decoder, as loaded: the descriptor (scalar loads that nothing waits for
// until the next block iteration, so they never turn an LDS wait of the current one into lgkmcnt(0))
// and the lane's four record low bits (chain slots 64 k + lane), loaded a whole block iteration
// before they are used (chain_rec_load) and unconditionally: a select of the loaded values in the same
// iteration made the compiler branch around each load, splitting the block loop (k_chain_decode 10.76
// against k_decode's 9.89 ms). Records past hi read stale rows of the chain's capacity and are
// replaced by the block start in chain_meta_sub.
struct ChainMeta {
    uint64_t b0, b1, rec;
    long long out;
    uint32_t lhl;  // ChainBlk::lhl
    bool valid;    // a block of the decode (else: any block, decoded, never stored)
    uint64_t sub;  // the four record words as loaded
};

HZ_DEV void chain_meta_load(const ChainArgs& y, uint64_t b, uint64_t nb, ChainMeta& m) {
    const uint64_t bb = b < nb ? b : (nb ? nb - 1 : 0);  // past the end: any block, never stored
    // the descriptor through the scalar cache (b0, b1, rec, out, lhl)
    typedef const __attribute__((address_space(4))) unsigned long long* cu64p;
    const uint64_t bu = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(bb >> 32)) << 32) |
                        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)bb);
    const cu64p d = (cu64p)y.blk + 6 * bu;
    m.b0 = d[0];
    m.b1 = d[1];
    m.rec = d[2];
    m.out = (long long)d[3];
    m.lhl = (uint32_t)(d[5] >> 32);
    m.valid = b < nb;
}

// The lane's four records of a block whose descriptor has landed (one load per slot, always issued;
// y.rec holds a whole capacity of rows per chain, so rows past the block's valid ones exist).
HZ_DEV void chain_rec_load(const ChainArgs& y, int lane, ChainMeta& m) {
    const uint16_t* s16 = y.rec + m.rec + (uint32_t)lane;
    uint64_t sub = 0;
#pragma unroll
    for (int c = 0; c < kChainsPerLane; ++c) sub |= (uint64_t)s16[64 * c] << (16 * c);
    m.sub = sub;
}

HZ_DEV uint32_t chain_meta_hi(const ChainMeta& m) { return m.valid ? (m.lhl >> 9) & 0x1ffu : 0u; }

// The lane's chain starts (low 16 bits): its records below hi, else the block start.
HZ_DEV uint64_t chain_meta_sub(const ChainMeta& m, int lane) {
    const uint32_t hi = chain_meta_hi(m);
    uint64_t sub = 0;
#pragma unroll
    for (int c = 0; c < kChainsPerLane; ++c) {
        const uint32_t t = 64u * c + (uint32_t)lane;
        const uint64_t v = t < hi ? (m.sub >> (16 * c)) & 0xffffu : (uint64_t)(uint16_t)m.b0;
        sub |= v << (16 * c);
    }
    return sub;
}

// A chain block's symbols: record t = 64 c + lane of the block, 8 symbols at output index out + 8 t
// (2-byte aligned: the 16-byte stores of adjacent lanes are adjacent), the last record's and the
// stream end's symbol by symbol.
HZ_DEV void chain_store(const DecArgs& a, const ChainMeta& m, int lane, const uint32_t* pk) {
    uint16_t* out16 = reinterpret_cast<uint16_t*>(a.out);
    const uint32_t lo = m.lhl & 0x1ffu, hi = chain_meta_hi(m), last = m.lhl >> 18;
    const bool full = lo == 0 && hi == kChainRecs && last == 8 && m.out >= 0 &&
                      (uint64_t)m.out + (uint64_t)kBlockSyms <= a.nsym;
    if (full) {
        const long long ob = m.out;
#pragma unroll
        for (int c = 0; c < kChainsPerLane; ++c) {
            uint32_t* q = reinterpret_cast<uint32_t*>(out16 + ob + 8 * (64 * c + lane));
            u32x4a2 v = u32x4a2{pk[4 * c], pk[4 * c + 1], pk[4 * c + 2], pk[4 * c + 3]};
            __builtin_nontemporal_store(v, reinterpret_cast<u32x4a2*>(q));
        }
        return;
    }
#pragma unroll
    for (int c = 0; c < kChainsPerLane; ++c) {
        const uint32_t t = 64u * c + (uint32_t)lane;
        if (t < lo || t >= hi) continue;
        const long long o = m.out + 8ll * t;
        if (o < 0 || (uint64_t)o >= a.nsym) continue;
        uint32_t cn = t + 1 == hi ? last : 8u;
        cn = a.nsym - (uint64_t)o < cn ? (uint32_t)(a.nsym - (uint64_t)o) : cn;
        if (cn == 8) {
            *reinterpret_cast<u32x4a2*>(out16 + o) = u32x4a2{pk[4 * c], pk[4 * c + 1], pk[4 * c + 2], pk[4 * c + 3]};
        } else {
            for (uint32_t q = 0; q < cn; ++q) out16[o + q] = (uint16_t)(pk[4 * c + (q >> 1)] >> (16 * (q & 1)));
        }
    }
}

// k_decode's two-blocks-per-wave pipelined walk (dec_wave_pipe2) over chain blocks b, b + 1, then
// b + stride, ...: the same staging, quad walks and deferred gathers; block metadata from the
// descriptors, output at each block's chain position.
HZ_DEV void dec_wave_chain(const DecArgs& a, const ChainArgs& y, uint64_t nb, const uint32_t* lds, uint32_t* stg,
                           uint32_t slot, uint64_t b, uint64_t stride, int lane) {
    constexpr int C = 2 * kChainsPerLane;
    const __amdgpu_buffer_rsrc_t l2r = lut_l2_rsrc(a.l2);
    ChainMeta mc[2], mn[2], mn2[2];
    uint4 sc[2][kStageUnroll], sn[2][kStageUnroll];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        chain_meta_load(y, b + j, nb, mc[j]);
        chain_meta_load(y, b + stride + j, nb, mn[j]);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) chain_rec_load(y, lane, mc[j]);
    auto as_pipe = [](const ChainMeta& m) { PipeMeta p; p.b0 = m.b0; p.b1 = m.b1; p.sub = 0; return p; };
#pragma unroll
    for (int j = 0; j < 2; ++j) dec_stage_prefetch(a, as_pipe(mc[j]), lane, sc[j]);
    for (; b < nb; b += stride) {
        // the next blocks' records, a block iteration ahead (their descriptors landed last iteration)
#pragma unroll
        for (int j = 0; j < 2; ++j) chain_rec_load(y, lane, mn[j]);
        uint32_t p1[C];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            uint64_t w0;
            dec_stage_commit<true>(a, as_pipe(mc[j]), slot >> 2, stg + j * slot, lane, sc[j], w0);
            uint32_t off[kChainsPerLane];
            dec_chain_offsets(chain_meta_sub(mc[j], lane), mc[j].b0, mc[j].b1 - mc[j].b0, lane, off);
            const uint32_t top = (uint32_t)(stg - lds) + (uint32_t)(j + 1) * slot - 1u;
            const uint32_t base = top * 32u - (uint32_t)(mc[j].b0 + a.bit_adj - (w0 << 5));
#pragma unroll
            for (int c = 0; c < kChainsPerLane; ++c) p1[j * kChainsPerLane + c] = base - off[c];
        }
        __builtin_amdgcn_wave_barrier();  // LDS ops of one wave complete in order
        uint32_t pk[2][kSPT / 2];
        PipeLane st[C];
        uint32_t g[C];
        auto finish = [&](int c, int q) {
            // a leaf in LDS (bit 31) beats its gather's 0 (read past num_records); a link loses to its
            // gathered leaf: one v_max; and the leaf's byte 3 is 0x80 | L, subtracted whole (128 bits
            // more per step, which the window address takes back: dec_pipe_ldsn's adj). 12 % fewer VALU
            // per block pair; k_decode 10.09 -> 9.97 ms, chain decode 11.30 -> 11.13 ms (A/B, 16 GiB Zipf)
            const uint32_t ee = st[c].e > g[c] ? st[c].e : g[c];
            p1[c] -= ee >> 24;
            const int i = ((c % kChainsPerLane) * kChainSyms + q) >> 1;
            if (q & 1) pk[c / kChainsPerLane][i] = __builtin_amdgcn_perm(ee, pk[c / kChainsPerLane][i], 0x06050201u);
            else pk[c / kChainsPerLane][i] = ee;
        };
        auto issue4 = [&](int c, int q) {
            // issue priority over the quad's LDS walk and gathers (decode 9.96-9.99 -> 9.88-9.91 ms, A/B)
            __builtin_amdgcn_s_setprio(2);
            dec_pipe_ldsn<4>(a, lds, p1 + c, st + c, 16u * (uint32_t)q);  // q steps taken: 16 q bytes
#pragma unroll
            for (int t = 0; t < 4; ++t)
                g[c + t] = __builtin_amdgcn_raw_buffer_load_b32(l2r, st[c + t].gi, 0, 0);
            __builtin_amdgcn_s_setprio(0);
        };
        issue4(0, 0);
#pragma unroll
        for (int q = 0; q < kChainSyms; ++q) {
            issue4(4, q);
            if (q == kPfStep) {  // the next two blocks' staging chunks, the metadata after them
#pragma unroll
                for (int j = 0; j < 2; ++j) dec_stage_prefetch(a, as_pipe(mn[j]), lane, sn[j]);
#pragma unroll
                for (int j = 0; j < 2; ++j) chain_meta_load(y, b + 2 * stride + j, nb, mn2[j]);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) finish(c, q);
            if (q + 1 < kChainSyms) issue4(0, q + 1);
#pragma unroll
            for (int c = 4; c < 8; ++c) finish(c, q);
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (b + j < nb) chain_store(a, mc[j], lane, pk[j]);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            mc[j] = mn[j];
            mn[j] = mn2[j];
#pragma unroll
            for (int u = 0; u < kStageUnroll; ++u) sc[j][u] = sn[j][u];
        }
    }
}

// Persistent: the block count and the largest block come from the device (k_chain_meta); slots are
// sized in-kernel from the largest block, waves without a slot pair idle (k_decode's rule).
__global__ __launch_bounds__(kDecPipe2Threads) void k_chain_decode(DecArgs a, ChainArgs y) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    copy_lds_table(lds, a.lds_img, a.lds_words);
    const int lane = threadIdx.x & 63;
    const uint32_t wid = wave_id();
    typedef const __attribute__((address_space(4))) unsigned long long* cu64p;
    const uint64_t nb = ((cu64p)y.info)[0];
    if (nb == 0) return;  // no chain has a block (every codeword in heads / tails)
    const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)dec_slot_words(((cu64p)y.info)[1], a.max_len));
    const uint32_t nwave = blockDim.x >> 6;
    uint32_t nw2 = a.region_words / (2 * slot);
    nw2 = nw2 < nwave ? nw2 : nwave;
    if (nw2 == 0) {  // a block larger than the region (cannot happen: the host sizes it for 2048 x max_len)
        if (threadIdx.x == 0) atomicOr(a.err, 128u);
        return;
    }
    if (wid >= nw2) return;
    const uint64_t b = 2 * ((uint64_t)blockIdx.x * nw2 + wid), stride = 2 * (uint64_t)gridDim.x * nw2;
    dec_wave_chain(a, y, nb, lds, lds + a.lds_words + wid * 2 * slot, slot, b, stride, lane);
}

// Codebooks past the pipelined decoder's two table levels (codes longer than chain_k +
// chain_level_bits bits): every record of every block serially, one thread per record of 8 codewords,
// through br_next's multi-level lookup; the block count from the device (k_chain_meta).
__global__ __launch_bounds__(kSyncThreads) void k_chain_decode_serial(DecArgs a, ChainArgs y) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    copy_lds_table(lds, a.lds_img, a.lds_words);
    uint16_t* out16 = reinterpret_cast<uint16_t*>(a.out);
    const uint64_t nrec = y.info[0] * kChainRecs;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nrec; i += stride) {
        const ChainBlk& d = y.blk[i / kChainRecs];
        const uint32_t t = (uint32_t)(i % kChainRecs);
        if (t < d.lo || t >= d.hi) continue;
        const long long o = d.out + 8ll * t;
        const uint32_t cn = t + 1 == d.hi ? d.last : 8u;
        BitReader r;
        br_init(r, a, d.b0 + (uint16_t)(y.rec[d.rec + t] - (uint16_t)d.b0) + a.bit_adj);
        for (uint32_t q = 0; q < cn; ++q) {
            uint32_t sym;
            const uint32_t L = br_next<DEC_LUT>(r, a, lds, sym);
            if (L == 0) { atomicOr(a.err, 2u); break; }
            if (o + q >= 0 && (uint64_t)(o + q) < a.nsym) out16[o + q] = (uint16_t)sym;
        }
    }
}

// One thread per chain: its head (true codewords before its first valid record), the codewords past
// its record capacity, and the end bit of codeword nsym - 1, decoded serially (rare, short).
template <int MODE>
__global__ __launch_bounds__(kSyncThreads) void k_chain_tail(DecArgs a, ChainArgs y) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    copy_lds_table(lds, a.lds_img, a.lds_words);
    uint16_t* out16 = reinterpret_cast<uint16_t*>(a.out);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t last = a.nsym - 1;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < y.nchains; c += stride) {
        const uint64_t F = y.first[c], T = y.tcnt[c], n = y.cnt[c];
        const uint32_t h = y.hd[c], r0 = y.r0[c], nrec = chain_nrec(n);
        const bool has_end = a.nsym > 0 && F <= last && last < F + T;
        // serial decode of k codewords from stream bit p into output index o, noting the end bit
        auto serial = [&](uint64_t p, uint64_t o, uint64_t k) {
            BitReader r;
            br_init(r, a, p + a.bit_adj);
            for (uint64_t t = 0; t < k; ++t) {
                uint32_t sym;
                const uint32_t L = br_next<MODE>(r, a, lds, sym);
                if (L == 0) { atomicOr(a.err, 2u); return; }
                p += L;
                if (o + t < a.nsym) out16[o + t] = (uint16_t)sym;
                if (o + t == last) y.info[2] = p;
            }
        };
        if (h) serial(c ? y.txit[c - 1] : y.entry0, F, h);
        if (r0 < nrec && nrec > y.cap)      // records past the capacity: the rest of the chain
            serial(y.ckpt[c * (y.bpc + 1) + y.bpc], F + h + 8ull * (y.cap - r0), n - 8ull * y.cap);
        if (has_end && last >= F + h) {     // the end bit inside a piece: walk that piece up to it
            const uint64_t q = last - (F + h);
            const uint64_t m = r0 + q / 8;
            if (m < y.cap) {
                BitReader r;
                uint64_t p = chain_rec_pos(y, c, (uint32_t)m);
                br_init(r, a, p + a.bit_adj);
                for (uint32_t t = 0; t <= (uint32_t)(q % 8); ++t) {
                    uint32_t sym;
                    const uint32_t L = br_next<MODE>(r, a, lds, sym);
                    if (L == 0) { atomicOr(a.err, 2u); break; }
                    p += L;
                }
                y.info[2] = p;
            }
        }
    }
}

// ---- host side -----------------------------------------------------------------------------
// Chain geometry of a part of the payload (bits [pbeg, pend) after start): chains of cbits bits, about
// one per walk lane of the device (16 waves per CU), but at least kChainMinBlocks decode block long;
// each chain's record capacity holds its expected records with 25 % headroom (more go to
// k_chain_tail, serially). avg: expected payload bits per codeword (the lower of the payload's own
// and the codebook's Kraft estimate: more records, more headroom).
// (one: a part of ~2 Gbit -- the CLI's 256 MiB payload windows -- gets 90 K chains instead of 23 K, so
// the walk is not occupancy-starved: 1.85 -> 0.96 ms per window call, 1 GiB 2.50 -> 1.93 ms; 2 blocks:
// 1.21 / 1.94 ms; long parts are lane-limited and unaffected)
constexpr uint64_t kChainMinBlocks = 1;
struct ChainGeom {
    uint64_t nchains = 0, cbits = 0, pbeg = 0, pend = 0;
    uint32_t bpc = 0, cap = 0;
    uint64_t off_rec, off_ckpt, off_arr, off_u32, off_list, off_info, off_tiles, off_blk, words;
};

static ChainGeom chain_geom(uint64_t pbeg, uint64_t pend, double avg, int ncu) {
    ChainGeom g;
    g.pbeg = pbeg;
    g.pend = pend;
    const uint64_t bits = pend > pbeg ? pend - pbeg : 0;
    if (bits == 0) return g;
    if (!(avg >= 1.0)) avg = 1.0;
    const uint64_t lanes = (uint64_t)kChainWalkWaves * 64 * (uint64_t)(ncu > 0 ? ncu : 1);
    const uint64_t minbits = (uint64_t)(kChainMinBlocks * kBlockSyms * avg);
    uint64_t cb = (bits + lanes - 1) / lanes;
    cb = cb > minbits ? cb : minbits;
    cb = (cb + 127) & ~127ull;
    g.cbits = cb;
    g.nchains = (bits + cb - 1) / cb;
    const double recs = (double)cb / avg / 8.0 * 1.25 + 64.0;
    g.bpc = (uint32_t)((recs + kChainRecs - 1) / kChainRecs);
    g.cap = g.bpc * kChainRecs;
    const uint64_t nc = g.nchains;
    const uint64_t ntiles = (nc + kScanTile - 1) / kScanTile;
    uint64_t w = 0;
    g.off_rec = w;   w += (nc * g.cap * 2 + 15) / 16 * 2;       // u16 records (16-byte rows)
    g.off_ckpt = w;  w += nc * (g.bpc + 1);                     // u64 checkpoints
    g.off_arr = w;   w += 8 * nc;                               // ent, xit, txit, cnt, tcnt, nblk, first, bbase
    g.off_u32 = w;   w += nc;                                   // hd, r0 (u32)
    g.off_list = w;  w += nc + 1;                               // list[2] (u32), lcnt
    g.off_info = w;  w += 8;
    g.off_tiles = w; w += ntiles + 2;
    g.off_blk = w;   w += nc * g.bpc * (sizeof(ChainBlk) / 8);
    g.words = w + 8;
    return g;
}

static double chain_avg(const Tables& t, uint64_t bits, uint64_t nsym) {
    double avg = nsym ? (double)bits / (double)nsym : t.dec_avg_bits;
    if (t.dec_avg_bits > 0.5 && t.dec_avg_bits < avg) avg = t.dec_avg_bits;
    return avg;
}

uint64_t chain_scratch_words(uint64_t part_begin, uint64_t part_end, uint64_t nsym, const Tables& t, int ncu) {
    return chain_geom(part_begin, part_end, chain_avg(t, part_end > part_begin ? part_end - part_begin : 0, nsym), ncu)
        .words;
}

bool seg_decode_supported(const Tables& t) {
    return t.dec_mode >= 0 && t.dec_mode != DEC_FIXED16 && t.chain_lds_bytes > 0 && t.walk8_bytes > 0 &&
           t.chain_esc != nullptr;
}

// Codes the pipelined chain decoder resolves (an LDS level, then one global level); longer codebooks
// decode their records serially (k_chain_decode_serial).
static bool chain_pipelined(const Tables& t) { return t.dec_max_len <= t.chain_k + t.chain_level_bits; }

// The decoder arguments of the chain phases: the chain's LUT images (the decode tables' for a LUT
// codebook, the LUT built beside a DENSE one).
static void fill_chain_dec_args(DecArgs& d, const Tables& t, const uint8_t* d_payload, uint64_t payload_bytes,
                                uint64_t nsym) {
    fill_dec_args(d, t, d_payload, payload_bytes, nsym);
    d.lds_img = t.chain_lds;
    d.lds_words = t.chain_lds_bytes / 4;
    d.k = t.chain_k;
    d.level_bits = t.chain_level_bits;
    d.l2 = t.chain_l2;
}

// Payloads under 16 bytes (the walk's 16-byte loads need at least 4 words): one thread decodes the
// codewords serially from start_bit, as Decompressor.cu:259-291 does, stream-ordered; a payload with
// fewer than nsym codewords reports the end bit UINT64_MAX.
__global__ __launch_bounds__(64) void k_decode_tiny(DecArgs a, uint64_t start, uint64_t payload_bits,
                                                    unsigned long long* end) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    copy_lds_table(lds, a.lds_img, a.lds_words);
    if (threadIdx.x) return;
    uint16_t* out16 = reinterpret_cast<uint16_t*>(a.out);
    BitReader r;
    br_init(r, a, start + a.bit_adj);
    uint64_t p = start, i = 0;
    for (; i < a.nsym && p <= payload_bits; ++i) {  // (every code >= 1 bit: at most 128 steps)
        uint32_t sym;
        const uint32_t L = br_next<DEC_LUT>(r, a, lds, sym);
        if (L == 0) { atomicOr(a.err, 2u); break; }
        p += L;
        if (p <= payload_bits) out16[i] = (uint16_t)sym;
    }
    if (end) *end = i == a.nsym && p <= payload_bits ? p : ~0ull;
}

hipError_t chain_decode_tiny(const Tables& t, const uint8_t* d_payload, uint64_t payload_bytes, uint64_t start_bit,
                             uint64_t nsym, uint8_t* d_out, unsigned long long* d_end, uint32_t* d_err, hipStream_t s) {
    if (!seg_decode_supported(t)) return hipErrorInvalidValue;
    DecArgs d;
    fill_chain_dec_args(d, t, d_payload, payload_bytes, nsym);
    d.starts = nullptr; d.subs = nullptr; d.out = d_out; d.err = d_err;
    hipError_t e = ensure_lds_limit((const void*)k_decode_tiny, kLdsBytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_decode_tiny, dim3(1), dim3(64), t.chain_lds_bytes, s, d, start_bit, payload_bytes * 8, d_end);
    return hipGetLastError();
}

// HZ_CAPTURE_DEBUG=1 (debug): the stream's capture status after each step of the launchers.
static void cap_check(hipStream_t s, const char* tag) {
    static const bool on = getenv("HZ_CAPTURE_DEBUG") != nullptr;
    if (!on) return;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    const hipError_t e = hipStreamGetCaptureInfo(s, &st, &id);
    fprintf(stderr, "[hz capture] %-12s status %d (err %d)\n", tag, (int)st, (int)e);
}

// The state a chain decode keeps between its phases (scan, refix, decode): geometry, kernel arguments
// (device pointers into the context's scratch and tables), the part's summary in y.info.
struct ChainState {
    ChainGeom g;
    ChainArgs y;
    DecArgs d;
    WalkArgs w;
    unsigned long long* tiles = nullptr;  // scan scratch
    uint64_t base = 0;                     // stream bit of byte 0 of the payload view (hz_indexless_scan)
    bool valid = false;
};
ChainState* chain_state_create() { return new ChainState(); }
void chain_state_destroy(ChainState* st) { delete st; }
const unsigned long long* chain_info(const ChainState* st) { return st->valid ? st->y.info : nullptr; }
void chain_invalidate(ChainState* st) { st->valid = false; }

// The part's summary in stream bits: codewords, true exit, entry in use (view bits + base).
__global__ void k_chain_summary(const unsigned long long* info, unsigned long long* dst, uint64_t base) {
    if (threadIdx.x == 0) {
        dst[0] = info[3];
        dst[1] = info[4] + base;
        dst[2] = info[5] + base;
    }
}
// The end bit in stream bits (all ones: not in this part).
__global__ void k_chain_end(const unsigned long long* info, unsigned long long* dst, uint64_t base) {
    if (threadIdx.x == 0) dst[0] = info[2] == ~0ull ? ~0ull : info[2] + base;
}
__global__ void k_put3(unsigned long long* dst, uint64_t a, uint64_t b, uint64_t c) {
    if (threadIdx.x == 0) {
        dst[0] = a;
        dst[1] = b;
        dst[2] = c;
    }
}
struct StageArgs {
    const uint8_t* src;
    StageSeg seg[kStageMaxSegs];
};
// Segment blockIdx.y of the staging buffer to its table: 16-byte vectors, then the 4-byte tail.
__global__ __launch_bounds__(256) void k_stage_scatter(StageArgs a) {
    const StageSeg g = a.seg[blockIdx.y];
    const uint4* src = reinterpret_cast<const uint4*>(a.src + g.off);
    uint4* dst = reinterpret_cast<uint4*>(g.dst);
    const uint64_t nv = g.bytes / 16;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (uint64_t)gridDim.x * blockDim.x)
        dst[i] = src[i];
    if (blockIdx.x == 0 && threadIdx.x < (g.bytes % 16) / 4) {
        const uint64_t w = nv * 4 + threadIdx.x;
        reinterpret_cast<uint32_t*>(g.dst)[w] = reinterpret_cast<const uint32_t*>(a.src + g.off)[w];
    }
}

hipError_t stage_scatter(const uint8_t* h_src, const StageSeg* segs, int nseg, hipStream_t s) {
    for (int i0 = 0; i0 < nseg; i0 += kStageMaxSegs) {
        StageArgs a;
        a.src = h_src;
        const int n = nseg - i0 < kStageMaxSegs ? nseg - i0 : kStageMaxSegs;
        uint64_t most = 0;
        for (int i = 0; i < n; ++i) {
            a.seg[i] = segs[i0 + i];
            most = a.seg[i].bytes > most ? a.seg[i].bytes : most;
        }
        uint64_t blocks = (most / 16 + 255) / 256;
        blocks = blocks < 1 ? 1 : (blocks > 512 ? 512 : blocks);
        hipLaunchKernelGGL(k_stage_scatter, dim3((uint32_t)blocks, (uint32_t)n), dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t put3(unsigned long long* d_dst, uint64_t a, uint64_t b, uint64_t c, hipStream_t s) {
    hipLaunchKernelGGL(k_put3, dim3(1), dim3(64), 0, s, d_dst, a, b, c);
    return hipGetLastError();
}
hipError_t chain_summary(const ChainState* st, unsigned long long* d_dst, hipStream_t s) {
    if (!st->valid) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_chain_summary, dim3(1), dim3(64), 0, s, (const unsigned long long*)st->y.info, d_dst, st->base);
    return hipGetLastError();
}

// fix-ups (every chain once, then the listed ones on one workgroup), the scans and the descriptors
static hipError_t chain_fix_and_meta(ChainState* st, const Tables& t, int ncu, hipStream_t s) {
    ChainArgs& y = st->y;
    hipError_t e;
    if ((e = hipMemsetAsync(y.lcnt, 0, 8, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(y.info, 0, 16, s)) != hipSuccess) return e;  // blocks, largest block (atomicMax)
    if ((e = ensure_lds_limit((const void*)k_chain_fix<DEC_LUT>, kLdsBytes)) != hipSuccess) return e;
    if ((e = ensure_lds_limit((const void*)k_chain_fix_loop<DEC_LUT>, kLdsBytes)) != hipSuccess) return e;
    const uint64_t wgs = grid_clamp((y.nchains + kSyncThreads - 1) / kSyncThreads, (uint64_t)ncu);
    hipLaunchKernelGGL(k_chain_fix<DEC_LUT>, dim3(wgs), dim3(kSyncThreads), t.chain_lds_bytes, s, st->d, y);
    hipLaunchKernelGGL(k_chain_fix_loop<DEC_LUT>, dim3(1), dim3(kSyncThreads), t.chain_lds_bytes, s, st->d, y);
    cap_check(s, "fix");
    if ((e = launch_scan(y.tcnt, y.nchains, st->tiles, y.first, ~0ull, 0ull, s)) != hipSuccess) return e;
    if ((e = launch_scan(y.nblk, y.nchains, st->tiles, y.bbase, ~0ull, 0ull, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_chain_meta, dim3((y.nchains + 255) / 256), dim3(256), 0, s, y);
    cap_check(s, "scan+meta");
    return hipGetLastError();
}

hipError_t chain_scan(ChainState* st, const Tables& t, const uint8_t* d_payload, uint64_t payload_bytes,
                      uint64_t base, uint64_t start_bit, uint64_t nsym, uint64_t part_begin, uint64_t part_end,
                      uint64_t entry0, unsigned long long* d_scratch, uint32_t* d_err, int ncu, hipStream_t s) {
    st->valid = false;
    // bits of the view from here on: stream bit b is view bit b - base (mod 2^64: start_bit may lie
    // before the view when it begins inside the stream)
    st->base = base;
    start_bit -= base;
    if (entry0 != ~0ull) entry0 -= base;
    if (!seg_decode_supported(t)) return hipErrorInvalidValue;
    DecArgs& d = st->d;
    fill_chain_dec_args(d, t, d_payload, payload_bytes, nsym);
    d.starts = nullptr; d.subs = nullptr; d.out = nullptr; d.err = d_err;
    if (d.nwords < 4) return hipErrorInvalidValue;
    const ChainGeom& g = st->g = chain_geom(part_begin, part_end,
                                             chain_avg(t, part_end > part_begin ? part_end - part_begin : 0, nsym), ncu);
    if (g.nchains == 0 || g.nchains >= (1ull << 32)) return hipErrorInvalidValue;
    ChainArgs& y = st->y;
    y.nchains = g.nchains; y.cbits = g.cbits; y.pbeg = g.pbeg; y.pend = g.pend; y.start = start_bit;
    y.entry0 = entry0;
    y.bpc = g.bpc; y.cap = g.cap;
    unsigned long long* sc = d_scratch;
    y.rec = reinterpret_cast<uint16_t*>(sc + g.off_rec);
    y.ckpt = sc + g.off_ckpt;
    unsigned long long* arr = sc + g.off_arr;
    y.ent = arr; y.xit = arr + g.nchains; y.txit = arr + 2 * g.nchains; y.cnt = arr + 3 * g.nchains;
    y.tcnt = arr + 4 * g.nchains; y.nblk = arr + 5 * g.nchains; y.first = arr + 6 * g.nchains;
    y.bbase = arr + 7 * g.nchains;
    y.hd = reinterpret_cast<uint32_t*>(sc + g.off_u32);
    y.r0 = y.hd + g.nchains;
    y.list[0] = reinterpret_cast<uint32_t*>(sc + g.off_list);
    y.list[1] = y.list[0] + g.nchains;
    y.lcnt = y.list[1] + g.nchains;
    y.info = sc + g.off_info;
    y.blk = reinterpret_cast<ChainBlk*>(sc + g.off_blk);
    y.err = d_err;
    st->tiles = sc + g.off_tiles;
    WalkArgs& w = st->w;
    w.words = d.words; w.nwords = d.nwords; w.bit_adj = d.bit_adj;
    w.start = start_bit; w.nseg = 0;
    w.lds_img = nullptr; w.lds_words = 0; w.k = 0; w.bias = 0;
    w.esc = t.chain_esc; w.m = t.chain_esc_m;
    w.w8_img = t.d_walk8; w.w8_words = t.walk8_bytes / 4; w.k8 = t.walk8_k;
    w.lut1 = t.chain_lds; w.lut2 = t.chain_l2; w.lutk = t.chain_k;
    w.bmp = nullptr; w.cnt = nullptr; w.ent = nullptr; w.dirty = nullptr;
    // test hook: HZ_SEG_LEAD=<bits> (0: no lead-in, so nearly every chain takes the fix-up path)
    static const uint32_t lead = [] { const char* v = getenv("HZ_SEG_LEAD"); return v ? (uint32_t)atoi(v) : kWalkLead; }();
    w.lead = lead;
    hipError_t e;
    // 1. the walk: one chain per lane; small chain counts spread over every CU (fewer waves per workgroup)
    {
        uint64_t wpg = (g.nchains + 64ull * ncu - 1) / (64ull * ncu);
        wpg = wpg < 1 ? 1 : (wpg > (uint64_t)kChainWalkWaves ? (uint64_t)kChainWalkWaves : wpg);
        const uint32_t threads = (uint32_t)(64 * wpg);
        const uint32_t ring_bytes = kSegRing * kRingRow * 4 + threads * 16;  // ring rows (1024 lanes), record buffers
        // DEEP: escapes past the escape table's bits (codes longer than kChainEscMaxBits)
        const bool deep = t.dec_max_len > t.chain_esc_m;
        const void* fn = deep ? (const void*)k_chain_walk<true> : (const void*)k_chain_walk<false>;
        if ((e = ensure_lds_limit(fn, (int)(kChainWalkWaves * 64 * (kSegRing * 4 + 16)))) != hipSuccess) return e;
        const uint64_t wgs = (g.nchains + threads - 1) / threads;
        if (deep) hipLaunchKernelGGL(k_chain_walk<true>, dim3(wgs), dim3(threads), ring_bytes, s, w, y);
        else hipLaunchKernelGGL(k_chain_walk<false>, dim3(wgs), dim3(threads), ring_bytes, s, w, y);
        cap_check(s, "walk");
    }
    // 2.-4. fix-ups, scans, block descriptors and the part's summary
    if ((e = chain_fix_and_meta(st, t, ncu, s)) != hipSuccess) return e;
    st->valid = true;
    return hipSuccess;
}

hipError_t chain_refix(ChainState* st, const Tables& t, uint64_t entry0, int ncu, hipStream_t s) {
    if (!st->valid) return hipErrorInvalidValue;
    st->y.entry0 = entry0 != ~0ull ? entry0 - st->base : entry0;
    return chain_fix_and_meta(st, t, ncu, s);
}

hipError_t chain_decode(ChainState* st, const Tables& t, uint64_t nsym, uint8_t* d_out, unsigned long long* d_end,
                        int ncu, hipStream_t s) {
    if (!st->valid) return hipErrorInvalidValue;
    DecArgs d = st->d;
    const ChainArgs& y = st->y;
    d.out = d_out;
    d.nsym = nsym;
    hipError_t e;
    if ((e = hipMemsetAsync(y.info + 2, 0xff, 8, s)) != hipSuccess) return e;  // end bit: not found
    if (nsym && !chain_pipelined(t)) {
        // 5'. codes past two table levels: the records one thread each
        if ((e = ensure_lds_limit((const void*)k_chain_decode_serial, kLdsBytes)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_chain_decode_serial, dim3(4 * ncu), dim3(kSyncThreads), t.chain_lds_bytes, s, d, y);
    }
    if (nsym && chain_pipelined(t)) {
        // 5. the block decoder: k_decode's slot sizing, two slots per wave, persistent over every CU
        if ((e = ensure_lds_limit((const void*)k_chain_decode, kLdsBytes)) != hipSuccess) return e;
        const uint64_t bits = st->g.pend - st->g.pbeg;
        uint64_t avg = (uint64_t)(chain_avg(t, bits, nsym) * kBlockSyms);  // expected block bits
        avg = avg < (uint64_t)kBlockSyms * (uint32_t)d.max_len ? avg : (uint64_t)kBlockSyms * (uint32_t)d.max_len;
        const uint32_t worst = dec_slot_words_max(d.max_len);
        uint32_t est = dec_slot_words(avg + avg / 16 + 256, d.max_len);
        est = est < worst ? est : worst;
        const uint32_t table = d.lds_words;
        if (table < kDecMinLdsWords || table + worst > kLdsBytes / 4) return hipErrorInvalidValue;  // (biased windows)
        uint32_t nslot = (kLdsBytes / 4 - table) / est;
        nslot = nslot > 2 * kDecPipe2Threads / 64 ? 2 * kDecPipe2Threads / 64 : nslot;
        nslot &= ~1u;
        DecArgs b = d;
        b.region_words = nslot * est;
        if (b.region_words < 2 * worst && table + 2 * worst <= kLdsBytes / 4) b.region_words = 2 * worst;
        const int threads = 64 * (int)((nslot / 2) ? nslot / 2 : 1);
        const uint32_t lds = 4 * (table + b.region_words);
        hipLaunchKernelGGL(k_chain_decode, dim3(ncu), dim3(threads), lds, s, b, y);
        cap_check(s, "decode");
    }
    if (nsym) {
        // 6. heads, records past the capacity, the end bit
        if ((e = ensure_lds_limit((const void*)k_chain_tail<DEC_LUT>, kLdsBytes)) != hipSuccess) return e;
        const uint64_t wgs = grid_clamp((y.nchains + kSyncThreads - 1) / kSyncThreads, (uint64_t)ncu);
        hipLaunchKernelGGL(k_chain_tail<DEC_LUT>, dim3(wgs), dim3(kSyncThreads), t.chain_lds_bytes, s, d, y);
    }
    if (d_end) {
        if (st->base == 0) {
            if ((e = hipMemcpyAsync(d_end, y.info + 2, 8, hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
        } else {
            hipLaunchKernelGGL(k_chain_end, dim3(1), dim3(64), 0, s, (const unsigned long long*)y.info, d_end, st->base);
        }
    }
    cap_check(s, "tail+end");
    return hipGetLastError();
}

// ===========================================================================
// Random access (hz_decode_range, hz_index_expand; DESIGN.md "Random access").
// The seek table is start[] alone. A range of symbols is decoded in TILES of
// whole blocks: per tile one pass checks every block's bounds and, from the
// seek table, walks its codewords to rebuild the sub row (one lane per block:
// the walk is serial in a block and independent across blocks); then the block
// decoders of k_decode run over the tile through a small index of the tile in
// scratch (start[] clamped into the payload view, the tile's max_bits, the sub
// rows) with a store clipped to the range. Blocks that fail a check are flagged
// and never stored. The payload view may be a slice of the stream: bits stay
// stream bits, the view's word 0 is moved down instead (never dereferenced below
// w_first).
// ===========================================================================
struct SeekArgs {
    const unsigned long long* seek;  // the stream's start[]: block b at seek[b]
    const unsigned long long* isub;  // a full index's sub rows (chain 0 is checked against start[b]); else null
    unsigned long long* tstart;      // the tile's index in scratch: start[nb + 1] clamped into the view; null: none
    unsigned long long* rows;        // sub rows out, 64 words per block of the tile
    unsigned long long* maxp;        // the tile's largest block in bits (atomicMax; zeroed by the launcher)
    uint8_t* bad;                    // per block of the tile; null: none
    uint64_t blk0, nb, nsym;
    uint64_t clamp_lo, bit_hi;       // stream bits a block may start at / end at inside the view
};

constexpr int kSeekThreads = 256;

// One lane per block of the tile. Checks: start[b] <= start[b + 1] and at most cnt * max_len bits apart
// (else format), the staging window inside the view (else invalid argument). WALK: the block's cnt
// codewords from start[b] must end exactly at start[b + 1]; every 8th one's low 16 bits go to the sub
// row (chain c of the block at u16 c, as hz_pack writes it), chains past the stream's end = the end bit.
// The walk stops at cnt codewords or past start[b + 1], whichever comes first, and the reader clamps
// its loads to the view.
template <int MODE, bool WALK>
__global__ __launch_bounds__(kSeekThreads) void k_seek_subs(DecArgs a, SeekArgs y) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    if constexpr (WALK && MODE != DEC_FIXED16) copy_lds_table(lds, a.lds_img, a.lds_words);
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long mx = 0;
    if (j < y.nb) {
        const uint64_t b = y.blk0 + j;
        const uint64_t s0 = y.seek[b], s1 = y.seek[b + 1];
        const uint64_t left = y.nsym - b * kBlockSyms;
        const uint32_t cnt = left < (uint64_t)kBlockSyms ? (uint32_t)left : (uint32_t)kBlockSyms;
        uint32_t err = 0;
        if (s1 < s0 || s1 - s0 > (uint64_t)cnt * (uint32_t)a.max_len) err = 1u;
        else if (s0 < y.clamp_lo || s1 > y.bit_hi) err = 16u;
        else if (y.isub && (uint32_t)(y.isub[b * kWave] & 0xffffu) != (uint32_t)(s0 & 0xffffu)) err = 1u;
        if (y.tstart) {
            auto clamp = [&](uint64_t x) { return x < y.clamp_lo ? y.clamp_lo : (x > y.bit_hi ? y.bit_hi : x); };
            y.tstart[j] = clamp(s0);
            if (j + 1 == y.nb) y.tstart[y.nb] = clamp(s1);
        }
        if (WALK && !err) {
            unsigned long long* row = y.rows + j * kWave;
            unsigned long long acc = 0;
            auto put = [&](uint32_t ch, uint64_t pos) {
                acc |= (unsigned long long)(pos & 0xffffu) << (16 * (ch & 3));
                if ((ch & 3) == 3) { row[ch >> 2] = acc; acc = 0; }
            };
            if constexpr (MODE == DEC_FIXED16) {
                if (s1 - s0 != 16ull * cnt) {
                    err = 1u;
                } else {
                    for (uint32_t ch = 0; ch < (uint32_t)kChainsPerBlock; ++ch)
                        put(ch, ch * kChainSyms < cnt ? s0 + 16ull * kChainSyms * ch : s1);
                }
            } else {
                BitReader r;
                br_init(r, a, s0 + a.bit_adj);
                uint64_t pos = s0;
                uint32_t i = 0;
                for (; i < cnt; ++i) {
                    if ((i & (kChainSyms - 1)) == 0) put(i / kChainSyms, pos);
                    uint32_t sym;
                    const uint32_t L = br_next<MODE>(r, a, lds, sym);
                    pos += L;
                    if (L == 0 || pos > s1) break;
                }
                if (i < cnt || pos != s1) {
                    err = 1u;
                } else {
                    for (uint32_t ch = (cnt + kChainSyms - 1) / kChainSyms; ch < (uint32_t)kChainsPerBlock; ++ch) put(ch, s1);
                }
            }
        }
        if (y.bad) y.bad[j] = (uint8_t)(err != 0);
        if (err) atomicOr(a.err, err);
        else mx = s1 - s0;
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t lo = shfl_xor_u32((uint32_t)mx, m), hi = shfl_xor_u32((uint32_t)(mx >> 32), m);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(y.maxp, mx);
}

// FIXED16 range: symbol s of block b sits at start[b] + 16 (s - 2048 b); a thread decodes 8 symbols.
__global__ __launch_bounds__(1024) void k_range_fixed16(RangeDecArgs a, SeekArgs y) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    copy_lds_table(lds, a.lds_img, a.lds_words);
    const uint16_t* t16 = reinterpret_cast<const uint16_t*>(lds);
    const uint64_t b = a.lo / kBlockSyms, cnt = a.hi - a.lo;
    const uint64_t sb = y.seek[b];
    const uint64_t p = sb + 16 * (a.lo - b * kBlockSyms);
    if (sb < y.clamp_lo || sb > y.bit_hi || p > y.bit_hi || 16 * cnt > y.bit_hi - p) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.err, 16u);
        return;
    }
    uint16_t* out16 = reinterpret_cast<uint16_t*>(a.out);
    const uint64_t ng = (cnt + kChainSyms - 1) / kChainSyms, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ng; g += stride) {
        const uint64_t P = p + 16ull * kChainSyms * g + a.bit_adj;
        const uint64_t W = P >> 5;
        uint32_t w[5], o[4];
#pragma unroll
        for (int k = 0; k < 5; ++k) w[k] = W + k < a.nwords ? bswap32(a.words[W + k]) : 0u;
        fixed16_step(t16, w, (uint32_t)P, o);
        const uint64_t s0 = g * kChainSyms;
        if (s0 + kChainSyms <= cnt) {
            *reinterpret_cast<u32x4a2*>(out16 + s0) = u32x4a2{o[0], o[1], o[2], o[3]};
        } else {
            for (uint32_t q = 0; s0 + q < cnt; ++q) out16[s0 + q] = (uint16_t)(o[q >> 1] >> (16 * (q & 1)));
        }
    }
}

// Blocks per tile: 131 072 (256 MiB of output) give the one-lane-per-block walk 8 waves on each of
// 256 CUs and keep the scratch at 65 MiB whatever the range. HZ_RANGE_TILE_BLOCKS (read once) overrides.
// With a full index a tile keeps 9 bytes per block instead of 521 (no sub rows), so its tiles are
// kRangeFullTileFactor times as long: every tile costs a launch prologue and tail (about 45 us measured).
constexpr uint64_t kRangeTileBlocks = 131072;
constexpr uint64_t kRangeFullTileFactor = 16;
static uint64_t range_tile_blocks() {
    static const uint64_t v = [] {
        const char* e = getenv("HZ_RANGE_TILE_BLOCKS");
        const long long x = e ? atoll(e) : 0;
        return x > 0 ? (uint64_t)x : kRangeTileBlocks;
    }();
    return v;
}

uint64_t range_scratch_words(uint64_t sym_begin, uint64_t sym_count) {
    if (!sym_count) return 0;
    const uint64_t nb = (sym_begin + sym_count - 1) / kBlockSyms - sym_begin / kBlockSyms + 1;
    const uint64_t T = nb < range_tile_blocks() ? nb : range_tile_blocks();
    const uint64_t Tf = nb < kRangeFullTileFactor * range_tile_blocks() ? nb : kRangeFullTileFactor * range_tile_blocks();
    const uint64_t seek = (T + 2) + (T + 7) / 8 + (uint64_t)kWave * T, full = (Tf + 2) + (Tf + 7) / 8;
    return seek > full ? seek : full;  // either mode, so a context's scratch settles after one call
}

// The view of a payload slice that holds stream bytes [base, base + payload_bytes): stream bit p is
// bit p + bit_adj of `words`, whose word 0 lies below the slice when base > 0.
static void fill_range_view(RangeDecArgs& a, SeekArgs& y, const Tables& t, const uint8_t* d_payload,
                            uint64_t payload_bytes, uint64_t base, uint64_t nsym) {
    fill_dec_args(a, t, d_payload, payload_bytes, nsym);
    const uint64_t head = (uintptr_t)d_payload & 63, r = base & 63;
    uint64_t shift = base >> 6;  // 64-byte units the view's word 0 moves down
    uint64_t adj = head - r;
    if (head < r) { adj = head + 64 - r; shift += 1; }
    a.words = reinterpret_cast<const uint32_t*>(((uintptr_t)d_payload & ~(uintptr_t)63) - 64 * shift);
    a.bit_adj = (uint32_t)(8 * adj);
    a.w_first = 16 * shift;
    a.nwords = a.w_first + (payload_bytes + head + 3) / 4;
    a.start0 = 0;
    // a block's staging window starts 16 bytes below the 16-byte chunk of its first bit: inside the slice
    // unless the slice starts the stream (base 0: words below the payload read as zeros, as in hz_decode)
    const uint64_t vlo = 8 * base + a.bit_adj;
    y.clamp_lo = base ? 128 * ((vlo + 127) / 128 + 1) - a.bit_adj : 0;
    y.bit_hi = 8 * (base + payload_bytes);
    if (y.clamp_lo > y.bit_hi) y.clamp_lo = y.bit_hi;  // a slice too small for any block: every block fails
    y.nsym = nsym;
}

template <int MODE, bool WALK>
static hipError_t seek_subs_launch(const Tables& t, const DecArgs& a, const SeekArgs& y, hipStream_t s) {
    const uint32_t lds = WALK && MODE != DEC_FIXED16 ? t.dec_lds_bytes : 0;
    hipError_t e = ensure_lds_limit((const void*)k_seek_subs<MODE, WALK>, kLdsBytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_seek_subs<MODE, WALK>), dim3((y.nb + kSeekThreads - 1) / kSeekThreads), dim3(kSeekThreads), lds, s,
                       a, y);
    return hipGetLastError();
}

static hipError_t seek_walk_launch(const Tables& t, const DecArgs& a, const SeekArgs& y, hipStream_t s) {
    if (t.dec_mode == DEC_FIXED16) return seek_subs_launch<DEC_FIXED16, true>(t, a, y, s);
    if (t.dec_mode == DEC_DENSE) return seek_subs_launch<DEC_DENSE, true>(t, a, y, s);
    return seek_subs_launch<DEC_LUT, true>(t, a, y, s);
}

hipError_t launch_decode_range(const Tables& t, const uint8_t* d_payload, uint64_t payload_bytes, uint64_t base,
                               const unsigned long long* d_seek, uint64_t nsym, uint64_t sym_begin, uint64_t sym_count,
                               uint8_t* d_out, bool full_index, unsigned long long* d_scratch, uint32_t* d_err, int ncu,
                               hipStream_t s) {
    if (sym_count == 0) return hipSuccess;
    RangeDecArgs a{};
    SeekArgs y{};
    fill_range_view(a, y, t, d_payload, payload_bytes, base, nsym);
    a.out = d_out; a.err = d_err;
    a.lo = sym_begin; a.hi = sym_begin + sym_count;
    y.seek = d_seek;
    hipError_t e;
    if (t.dec_mode == DEC_FIXED16) {
        if ((e = ensure_lds_limit((const void*)k_range_fixed16, kFixed16LdsBytes)) != hipSuccess) return e;
        uint64_t wgs = ((sym_count + kChainSyms - 1) / kChainSyms + 1023) / 1024;
        if (wgs > (uint64_t)ncu) wgs = ncu;
        hipLaunchKernelGGL(k_range_fixed16, dim3(wgs), dim3(1024), kFixed16LdsBytes, s, a, y);
        return hipGetLastError();
    }
    const uint64_t nblk = index_blocks(nsym);
    y.isub = full_index ? d_seek + index_sub_offset(nblk) : nullptr;
    const uint64_t bf = sym_begin / kBlockSyms, bl = (sym_begin + sym_count - 1) / kBlockSyms;
    const uint64_t tile = (full_index ? kRangeFullTileFactor : 1) * range_tile_blocks();
    const uint64_t T = bl - bf + 1 < tile ? bl - bf + 1 : tile;
    y.tstart = d_scratch;
    y.bad = reinterpret_cast<uint8_t*>(d_scratch + T + 2);
    y.rows = d_scratch + (T + 2) + (T + 7) / 8;
    const double avg = t.dec_avg_bits > (double)t.dec_min_len ? t.dec_avg_bits : (double)(t.dec_min_len > 0 ? t.dec_min_len : 1);
    for (uint64_t tb = bf; tb <= bl; tb += T) {
        const uint64_t nb = bl - tb + 1 < T ? bl - tb + 1 : T;
        y.blk0 = tb; y.nb = nb;
        y.maxp = y.tstart + nb + 1;
        if ((e = hipMemsetAsync(y.maxp, 0, 8, s)) != hipSuccess) return e;
        e = full_index ? seek_subs_launch<DEC_LUT, false>(t, a, y, s) : seek_walk_launch(t, a, y, s);
        if (e != hipSuccess) return e;
        a.starts = y.tstart;
        a.subs = full_index ? y.isub + tb * kWave : y.rows;
        a.nblocks = nb;
        a.nsym = nb * kBlockSyms;
        a.blk0 = tb;
        a.bad = y.bad;
        const uint64_t pbits = (uint64_t)(avg * (double)kBlockSyms * (double)nb);
        if ((e = decode_dispatch(t, a, a.nwords - a.w_first >= 4, pbits, ncu, s)) != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_index_expand(const Tables& t, const uint8_t* d_payload, uint64_t payload_bytes,
                               const unsigned long long* d_seek, uint64_t nsym, unsigned long long* d_index,
                               uint32_t* d_err, hipStream_t s) {
    if (nsym == 0) return hipSuccess;
    const uint64_t nblk = index_blocks(nsym);
    hipError_t e;
    if (d_seek != d_index &&
        (e = hipMemcpyAsync(d_index, d_seek, 8 * (nblk + 1), hipMemcpyDeviceToDevice, s)) != hipSuccess)
        return e;
    if ((e = hipMemsetAsync(d_index + nblk + 1, 0, 8, s)) != hipSuccess) return e;
    RangeDecArgs a{};
    SeekArgs y{};
    fill_range_view(a, y, t, d_payload, payload_bytes, 0, nsym);
    a.err = d_err;
    y.seek = d_index;
    y.rows = d_index + index_sub_offset(nblk);
    y.maxp = d_index + nblk + 1;
    y.blk0 = 0; y.nb = nblk;
    return seek_walk_launch(t, a, y, s);
}

}  // namespace hz
