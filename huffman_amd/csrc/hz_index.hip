// hz_index.hip -- gfx950 (MI355X, CDNA4) kernels that build the block index of an index-less stream.
//
//   k_sync_*   block index of an index-less stream (reference files), parallel, self-synchronising
//   k_idx_walk its boundary bitmap by long chains, for the pipelined decoder's codebooks
//
// The table lookup and the bit reader: hz_decode_device.h; what k_chain_walk shares with k_idx_walk:
// hz_walk_device.h. Layout, roofline and design notes: DESIGN.md. All integer/bit work; no MFMA.
#include "hz_decode_device.h"
#include "hz_walk_device.h"

namespace hz {

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
constexpr uint32_t kBmpWords = kSegBits / 32;  // bitmap row of a segment

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
// (WalkArgs, walk_load / walk_fix, the payload group and its constants: hz_walk_device.h, with k_chain_walk.)

// Chunk slot q (0..3) of a payload ring, byte-swapped.
template <uint32_t ROW>
HZ_DEV void ring_put(uint32_t* ring, uint32_t q, const uint4& x) {
    const uint32_t v[4] = {bswap32(x.x), bswap32(x.y), bswap32(x.z), bswap32(x.w)};
#pragma unroll
    for (int i = 0; i < 4; ++i) ring[(4 * q + i) * ROW] = v[i];
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

}  // namespace hz
