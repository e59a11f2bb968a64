// hz_chain.hip -- gfx950 (MI355X, CDNA4) kernels of the index-less decode of the Huffman hot path.
//
//   k_chain_*  index-less decode in chain blocks
//
// The pipelined block decoder k_chain_decode shares with k_decode, and the bit reader:
// hz_decode_device.h; what k_chain_walk shares with k_idx_walk: hz_walk_device.h.
// Layout, roofline and design notes: DESIGN.md. All integer/bit work; no MFMA.
#include <stdio.h>
#include <stdlib.h>

#include "hz_decode_device.h"
#include "hz_walk_device.h"

namespace hz {

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

// ---- the seek table as a by-product of the walk (DESIGN.md "Seek table from the walk") ----------------
// Entries b0 .. b0 + nent - 1 of a stream's seek table from a call that covers codewords
// [sym_base, sym_base + nsym) of the stream: entry b is the start of codeword min(2048 b, stream_nsym)
// - sym_base of the call. Positions are view bits until they are stored.
struct ChainSeekArgs {
    unsigned long long* seek;  // the table, addressed from entry 0
    unsigned long long* end;   // nullable: the start of codeword nsym (= the end of nsym - 1), view bit + base
    uint64_t b0, nent;
    uint64_t sym_base, nsym, stream_nsym;
    uint64_t base;             // stream bit of view bit 0
    uint64_t add;              // what an entry adds to its view bit: base + the caller's bit_base
    uint64_t limit;            // bits the view holds: a codeword of the call is held when it starts below them,
                               // the call's end (codeword nsym, the next call's first) when it starts at or below
    unsigned long long* stats; // nullable (k_chain_seek): entries found [0] in a head, [1] past the record
                               // capacity, [2] through the delta rebuild, [3] in a chain that has a head
                               // (hz_debug_seek_stats: what the tests pin)
};

// Codeword of the call that lane i of a seek pass locates: an entry's, or (i == nent) the end's.
HZ_DEV uint64_t seek_sym(const ChainSeekArgs& z, uint64_t i) {
    if (i == z.nent) return z.nsym;
    const uint64_t s = (z.b0 + i) * (uint64_t)kBlockSyms;
    return (s < z.stream_nsym ? s : z.stream_nsym) - z.sym_base;
}

HZ_DEV void seek_put(const ChainSeekArgs& z, uint64_t i, uint64_t p) {
    // a codeword that starts exactly at the view's end has no bit in it: only the call's end may stand there
    const bool held = p != ~0ull && (seek_sym(z, i) == z.nsym ? p <= z.limit : p < z.limit);
    if (i == z.nent) *z.end = held ? p + z.base : ~0ull;
    else z.seek[z.b0 + i] = held ? p + z.add : ~0ull;
}

// Stream bit of record m (< cap, walked) of chain c. chain_rec_pos is exact while the record lies
// within 65 536 bits of its checkpoint; a decode block of 2048 codewords of up to 56 bits spans up to
// 114 688, and then the position is rebuilt from the deltas of consecutive records (at most 8 x 56
// bits apart), as the block decoder does (dec_chain_offsets); wide: that path was taken.
HZ_DEV uint64_t chain_rec_pos_wide(const ChainArgs& y, uint64_t c, uint32_t m, bool& wide) {
    const unsigned long long* ckp = y.ckpt + c * (y.bpc + 1);
    const uint16_t* rc = y.rec + c * y.cap;
    const uint32_t j = m / kChainRecs;
    uint64_t p = ckp[j];
    wide = ckp[j + 1] - p >= 65536ull;
    if (!wide) return p + (uint16_t)(rc[m] - (uint16_t)p);
    uint16_t prev = (uint16_t)p;
    for (uint32_t i = j * kChainRecs + 1; i <= m; ++i) {
        const uint16_t v = rc[i];
        p += (uint16_t)(v - prev);
        prev = v;
    }
    return p;
}

// Start of the codeword k codewords after the one at view bit p (all ones: an invalid code on the way).
HZ_DEV uint64_t seek_walk(const DecArgs& a, const uint32_t* lds, uint64_t p, uint64_t k) {
    if (k == 0) return p;
    BitReader r;
    br_init(r, a, p + a.bit_adj);
    for (uint64_t t = 0; t < k; ++t) {
        uint32_t sym;
        const uint32_t L = br_next<DEC_LUT>(r, a, lds, sym);
        if (L == 0) { atomicOr(a.err, 2u); return ~0ull; }
        p += L;
    }
    return p;
}

// One lane per entry (and one for the end bit): a binary search over the chains' output indices, then
// k_chain_tail's end-bit computation for that codeword -- the record at or before it and at most 7
// codewords, or a serial walk through a head or past the record capacity. One lane per entry and not
// one per chain: a chain holds anything from no entry to dozens (it is cbits bits long, an entry is
// 2048 codewords, and a run of short codes packs many entries into one chain), so lanes per chain would
// loop over uneven counts, while the search costs every entry the same ~log2(nchains) cached loads.
__global__ __launch_bounds__(kSyncThreads) void k_chain_seek(DecArgs a, ChainArgs y, ChainSeekArgs z) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    copy_lds_table(lds, a.lds_img, a.lds_words);
    const uint64_t total = y.info[3];  // codewords of the part (k_chain_meta)
    const uint64_t n = z.nent + (z.end ? 1 : 0);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t S = seek_sym(z, i);
        uint64_t p = ~0ull;  // past the part's codewords: not held
        if (S == total) {
            p = y.info[4];  // the first codeword after the part: the last chain's true exit
        } else if (S < total) {
            // the last chain with first <= S: chains without codewords repeat their successor's first,
            // so the search never ends on one (first[0] = 0 <= S)
            uint64_t lo = 0, hi = y.nchains;
            while (hi - lo > 1) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (y.first[mid] <= S) lo = mid;
                else hi = mid;
            }
            const uint64_t c = lo, k = S - y.first[c];
            const uint32_t h = y.hd[c], r0 = y.r0[c];
            int path = -1;  // the rare paths, counted
            if (k < h) {  // in the head: from the chain's true entry
                p = seek_walk(a, lds, c ? y.txit[c - 1] : y.entry0, k);
                path = 0;
            } else {
                const uint64_t q = k - h, m = r0 + q / 8;
                if (m < y.cap) {
                    bool wide;
                    p = seek_walk(a, lds, chain_rec_pos_wide(y, c, (uint32_t)m, wide), q % 8);
                    path = wide ? 2 : -1;
                } else {  // past the capacity
                    p = seek_walk(a, lds, y.ckpt[c * (y.bpc + 1) + y.bpc], 8 * (m - y.cap) + q % 8);
                    path = 1;
                }
            }
            if (path >= 0 && z.stats) atomicAdd(z.stats + path, 1ull);
            if (h && z.stats) atomicAdd(z.stats + 3, 1ull);
        }
        seek_put(z, i, p);
    }
}

// Payloads under 16 bytes (k_decode_tiny's case): one thread walks from the start and stores the
// entries (at most two lie within 128 codewords) and the end as it passes them.
__global__ __launch_bounds__(64) void k_seek_tiny(DecArgs a, uint64_t start, ChainSeekArgs z) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    copy_lds_table(lds, a.lds_img, a.lds_words);
    if (threadIdx.x) return;
    BitReader r;
    br_init(r, a, start + a.bit_adj);
    uint64_t p = start, at = 0;
    bool bad = false;
    const uint64_t n = z.nent + (z.end ? 1 : 0);
    for (uint64_t i = 0; i < n; ++i) {  // ascending codewords
        const uint64_t S = seek_sym(z, i);
        while (!bad && at < S && p <= z.limit) {  // (every code >= 1 bit: at most 129 steps in all)
            uint32_t sym;
            const uint32_t L = br_next<DEC_LUT>(r, a, lds, sym);
            if (L == 0) { atomicOr(a.err, 2u); bad = true; break; }
            p += L;
            ++at;
        }
        seek_put(z, i, !bad && at == S ? p : ~0ull);
    }
}

// FIXED16: codeword S of the call starts at view bit start + 16 S; the call holds `total` codewords.
__global__ __launch_bounds__(256) void k_seek_fixed16(uint64_t start, uint64_t total, ChainSeekArgs z) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= z.nent) return;
    const uint64_t S = seek_sym(z, i);
    seek_put(z, i, S <= total ? start + 16 * S : ~0ull);
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
    uint64_t off_rec, off_ckpt, off_arr, off_u32, off_list, off_info, off_tiles, off_blk, off_seek, words;
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
    // test hook: HZ_CHAIN_MIN_BITS=<bits> (read once) makes chains at least that long, so a small stream
    // has chains whose decode blocks span 65 536 bits and more (chain_rec_pos_wide's delta rebuild)
    static const uint64_t floor_bits = [] { const char* v = getenv("HZ_CHAIN_MIN_BITS"); return v ? strtoull(v, nullptr, 10) : 0ull; }();
    cb = cb > floor_bits ? cb : floor_bits;
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
    g.off_seek = w;  w += 4;                                    // k_chain_seek's path counters
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
    uint64_t view_bits = 0;                // bits the payload view holds (chain_seek: what lies past them is not held)
    unsigned long long* seek_stats = nullptr;  // the last chain_seek's path counters (in the scratch)
    bool valid = false;
};
ChainState* chain_state_create() { return new ChainState(); }
void chain_state_destroy(ChainState* st) { delete st; }
const unsigned long long* chain_info(const ChainState* st) { return st->valid ? st->y.info : nullptr; }
const unsigned long long* chain_seek_stats(const ChainState* st) { return st->seek_stats; }
void chain_forget_seek_stats(ChainState* st) { st->seek_stats = nullptr; }
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
    st->view_bits = payload_bytes * 8;
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
    st->seek_stats = nullptr;
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

// The entries a call over codewords [sym_base, sym_base + nsym) of a stream of stream_nsym writes:
// every b with sym_base <= min(2048 b, stream_nsym) <= sym_base + nsym.
static void seek_entries(ChainSeekArgs& z, uint64_t sym_base, uint64_t nsym, uint64_t stream_nsym) {
    z.sym_base = sym_base;
    z.nsym = nsym;
    z.stream_nsym = stream_nsym;
    z.b0 = (sym_base + kBlockSyms - 1) / kBlockSyms;
    const uint64_t e = sym_base + nsym;
    const uint64_t b1 = e == stream_nsym ? index_blocks(stream_nsym) : e / kBlockSyms;  // the last entry
    z.nent = b1 >= z.b0 ? b1 - z.b0 + 1 : 0;
}

hipError_t chain_seek(ChainState* st, const Tables& t, uint64_t sym_base, uint64_t nsym, uint64_t stream_nsym,
                      uint64_t bit_base, unsigned long long* d_seek, unsigned long long* d_end, int ncu, hipStream_t s) {
    if (!st->valid) return hipErrorInvalidValue;
    ChainSeekArgs z;
    seek_entries(z, sym_base, nsym, stream_nsym);
    z.seek = d_seek;
    z.end = d_end;
    z.base = st->base;
    z.add = st->base + bit_base;
    z.limit = st->view_bits;
    z.stats = reinterpret_cast<unsigned long long*>(st->y.rec) - st->g.off_rec + st->g.off_seek;  // (the scratch)
    const uint64_t n = z.nent + (d_end ? 1 : 0);
    if (n == 0) return hipSuccess;
    hipError_t e;
    if ((e = hipMemsetAsync(z.stats, 0, 32, s)) != hipSuccess) return e;
    st->seek_stats = z.stats;
    if ((e = ensure_lds_limit((const void*)k_chain_seek, kLdsBytes)) != hipSuccess) return e;
    const uint64_t wgs = grid_clamp((n + kSyncThreads - 1) / kSyncThreads, (uint64_t)ncu);
    hipLaunchKernelGGL(k_chain_seek, dim3(wgs), dim3(kSyncThreads), t.chain_lds_bytes, s, st->d, st->y, z);
    cap_check(s, "seek");
    return hipGetLastError();
}

hipError_t chain_seek_tiny(const Tables& t, const uint8_t* d_payload, uint64_t payload_bytes, uint64_t start_bit,
                           uint64_t nsym, uint64_t sym_base, uint64_t bit_base, uint64_t stream_nsym,
                           unsigned long long* d_seek, unsigned long long* d_end, uint32_t* d_err, hipStream_t s) {
    if (!seg_decode_supported(t)) return hipErrorInvalidValue;
    DecArgs d;
    fill_chain_dec_args(d, t, d_payload, payload_bytes, nsym);
    d.starts = nullptr; d.subs = nullptr; d.out = nullptr; d.err = d_err;
    ChainSeekArgs z;
    seek_entries(z, sym_base, nsym, stream_nsym);
    z.seek = d_seek;
    z.end = d_end;
    z.base = 0;
    z.add = bit_base;
    z.limit = payload_bytes * 8;
    z.stats = nullptr;
    if (z.nent + (d_end ? 1 : 0) == 0) return hipSuccess;
    hipError_t e = ensure_lds_limit((const void*)k_seek_tiny, kLdsBytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_seek_tiny, dim3(1), dim3(64), t.chain_lds_bytes, s, d, start_bit, z);
    return hipGetLastError();
}

hipError_t seek_fixed16(uint64_t start_bit, uint64_t total, uint64_t limit, uint64_t sym_base, uint64_t nsym,
                        uint64_t stream_nsym, uint64_t bit_base, unsigned long long* d_seek, hipStream_t s) {
    ChainSeekArgs z;
    seek_entries(z, sym_base, nsym, stream_nsym);
    z.seek = d_seek;
    z.end = nullptr;
    z.base = 0;
    z.add = bit_base;
    z.limit = limit;
    z.stats = nullptr;
    if (z.nent == 0) return hipSuccess;
    hipLaunchKernelGGL(k_seek_fixed16, dim3((z.nent + 255) / 256), dim3(256), 0, s, start_bit, total, z);
    return hipGetLastError();
}

}  // namespace hz
