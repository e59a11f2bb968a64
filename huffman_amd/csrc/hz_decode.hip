// hz_decode.hip -- gfx950 (MI355X, CDNA4) block decoders of the Huffman hot path and the random access
// on them (the index they read: hz_pack.hip or hz_index.hip; without an index: hz_chain.hip).
//
//   k_decode         block-parallel table decode              <- Decompressor.cu:259-291
//   k_decode_range   the same over a tile of a range, k_seek_subs rebuilds its sub rows
//
// What the index builder and the chain decode share with these kernels: hz_decode_device.h.
// Layout, roofline and design notes: DESIGN.md. All integer/bit work; no MFMA.
#include <stdlib.h>

#include <type_traits>

#include "hz_range_device.h"

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

// Stage payload words [w0, w0 + 4 npc) of block b into `stg`, byte-swapped.
// The first kStageUnroll 16-byte loads of every lane are issued before any
// is used (one memory round trip for blocks up to 4 KiB of payload).
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

// The random access view of the block decoders (RangeDecArgs): hz_range_device.h; launchers below.
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
// (SeekArgs, the per-block checks and fill_range_view: hz_range_device.h, shared with hz_ranges.hip.)
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
        uint32_t err = 0;  // (seek_block_err's checks in place: through the function the kernel compiles to other instructions)
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
