// hz_ranges.hip -- gfx950 (MI355X, CDNA4) batch random access: many ranges of one stream in one call
// (hz_decode_ranges, hz_decode_ranges_pieces; DESIGN.md "Random access", "A batch of ranges", "Gathered
// pieces").
//
//   k_ranges_plan    per range: checks, block jobs, exclusive scan of the job counts
//   k_ranges_decode  one wave per block job: stage, cooperative walk, decode, clipped store
//
// Both come in two compile-time forms. PIECES = false: one payload slice and one seek table for the whole
// call, the view fixed by the host. PIECES = true: every range names a piece of a gathered buffer, and
// the wave of a job builds the view of that piece (wave-uniform, in scalar registers) before it touches
// the block; everything after that is the same code.
//
// The view, the per-block checks and the FIXED16 step are hz_decode.hip's (hz_range_device.h); the
// lookup, the staged window and the bit reader are the block decoders' (hz_decode_device.h). A unit of
// its own: its callers of that shared force-inlined code must not change what the compiler assumes
// inside it for the kernels of hz_decode.hip (DESIGN.md "Source layout"). All integer/bit work; no MFMA.
#include <stdlib.h>

#include <type_traits>

#include "hz_range_device.h"

namespace hz {

struct RangesArgs {
    const hz_range* ranges;    // device list, never read by the host
    uint32_t nranges;
    unsigned long long* offs;  // scratch: first job of every range; offs[nranges] = all jobs
    uint64_t out_bytes;
    unsigned long long* stats; // HZ_RANGES_STATS_WORDS counters; null: none
    uint32_t slot_words;       // payload slot of a wave (u32 words, a multiple of 4); the bitmap has as many
    uint32_t wave_words;       // LDS of a wave: slot, bitmap, kChainsPerBlock chain starts
};

// The gathered form: ranges that name pieces, the pieces, the buffer they sit in and the compact table.
struct PieceRangesArgs : RangesArgs {
    const hz_piece_range* pranges;  // device list (`ranges` is unset)
    const hz_piece* pieces;         // device list
    uint32_t npieces;
    const uint8_t* buf;
    uint64_t buf_bytes;
    const unsigned long long* cseek;  // the words the pieces name, seek_words of them
    uint64_t seek_words;
};
template <bool PIECES> using RangesArgsOf = std::conditional_t<PIECES, PieceRangesArgs, RangesArgs>;

// The gathered form's decoder arguments: a type of its own, so that the bit reader's chunk loads
// (br_init / br_word / br_next of this type) are the ld_chunk below and keep to the piece at its lower
// end as well. The slice forms keep the shared ld_chunk, whose view ends on a 64-byte line below.
struct PieceDecArgs : RangeDecArgs {};
template <bool PIECES> using DecArgsOf = std::conditional_t<PIECES, PieceDecArgs, RangeDecArgs>;

HZ_DEV uint4 ld_chunk(const PieceDecArgs& a, uint64_t w) {  // w % 4 == 0; zeros outside [w_first, nwords)
    if (w >= a.w_first && w + 4 <= a.nwords) return *reinterpret_cast<const uint4*>(a.words + w);
    uint32_t t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = w + k >= a.w_first && w + k < a.nwords ? a.words[w + k] : 0u;
    return make_uint4(t[0], t[1], t[2], t[3]);
}

// Range i of a call's list.
HZ_DEV hz_range range_at(const RangesArgs& p, uint64_t i) { return p.ranges[i]; }
HZ_DEV hz_piece_range range_at(const PieceRangesArgs& p, uint64_t i) { return p.pranges[i]; }

// What the plan asks of a non-empty range's piece before any job of the range exists: the piece is one of
// the list, its bytes lie in the buffer, its table words in the compact table, its positions below
// HZ_POS_LIMIT, and every block of the range is one of its blocks.
HZ_DEV bool piece_ok(const PieceRangesArgs& p, const hz_piece_range& r) {
    if (r.sym_count == 0) return true;  // an empty range names no piece
    if (r.piece >= p.npieces) return false;
    const hz_piece pc = p.pieces[r.piece];
    constexpr uint64_t kMaxByte = (HZ_POS_LIMIT - 1) / 8;  // 8 * byte < HZ_POS_LIMIT
    const uint64_t b0 = r.sym_begin / kBlockSyms, b1 = (r.sym_begin + r.sym_count - 1) / kBlockSyms;
    return pc.bytes <= p.buf_bytes && pc.buf_byte <= p.buf_bytes - pc.bytes && pc.nblocks < p.seek_words &&
           pc.seek_index <= p.seek_words - pc.nblocks - 1 && b0 >= pc.first_block && b1 - pc.first_block < pc.nblocks &&
           pc.stream_byte <= kMaxByte && pc.bytes <= kMaxByte - pc.stream_byte;
}

// The view of a job's piece into the wave's copy of the kernel arguments: fill_range_view's arithmetic on
// the piece's place in the buffer, its first existing word the one that holds the piece's first byte, and
// the table addressed so that block b of the stream stands at seek[b]. All of it is wave-uniform.
HZ_DEV void piece_view(RangeDecArgs& a, SeekArgs& y, const PieceRangesArgs& p, const hz_piece& pc) {
    const RangeView v = range_view((uint64_t)reinterpret_cast<uintptr_t>(p.buf) + pc.buf_byte, pc.bytes, pc.stream_byte);
    // through a global-address-space pointer: from a bare integer the compiler cannot tell, and every
    // payload load of the kernel would be a flat load
    a.words = (const uint32_t*)reinterpret_cast<const __attribute__((address_space(1))) uint32_t*>((uintptr_t)v.words_addr);
    a.bit_adj = v.bit_adj;
    a.w_first = v.w0 + v.head / 4;
    a.nwords = v.nwords;
    y.clamp_lo = v.clamp_lo;
    y.bit_hi = v.bit_hi;
    y.seek = p.cseek + pc.seek_index - pc.first_block;
}

constexpr int kPlanThreads = 1024;
constexpr int kRangesMaxWaves = 16;
constexpr uint32_t kRangesMaxRounds = 64;  // lane i holds the true path after round i at the latest
constexpr uint32_t kDead = 0xffffffffu;    // exit of a path that met an invalid code

// Jobs of a range = the blocks it touches (none for an empty or a refused one). One workgroup takes the
// list 1024 ranges at a time and carries the running sum, so any length takes nranges + 1 words of
// scratch and one launch (launch_scan would need the counts and its tile sums beside the offsets).
template <bool PIECES>
__global__ __launch_bounds__(kPlanThreads) void k_ranges_plan(RangesArgsOf<PIECES> p, uint64_t nsym, uint32_t* err) {
    __shared__ uint64_t sh[kPlanThreads / 64 + 1];
    uint64_t carry = 0;
    bool refused = false;
    for (uint64_t i0 = 0; i0 < p.nranges; i0 += kPlanThreads) {
        const uint64_t i = i0 + threadIdx.x;
        uint64_t nb = 0;
        if (i < p.nranges) {
            const auto r = range_at(p, i);
            bool ok = r.sym_begin <= nsym && r.sym_count <= nsym - r.sym_begin && !(r.out_byte & 1) &&
                      r.out_byte <= p.out_bytes && 2 * r.sym_count <= p.out_bytes - r.out_byte;
            if constexpr (PIECES) {
                if (ok) ok = piece_ok(p, r);
            }
            refused |= !ok;
            if (ok && r.sym_count) nb = (r.sym_begin + r.sym_count - 1) / kBlockSyms - r.sym_begin / kBlockSyms + 1;
        }
        uint64_t total;
        const uint64_t ex = block_exclusive_scan(nb, sh, total);
        if (i < p.nranges) p.offs[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) p.offs[p.nranges] = carry;
    if (refused) atomicOr(err, 16u);
}

// Code length at bit `pos` of a staged slot (0: no code of the book starts with those bits).
template <int MODE, bool WIDE>
HZ_DEV uint32_t slot_len(const DecArgs& a, const uint32_t* lds, const uint32_t* stg, uint32_t pos) {
    uint32_t sym, L;
    dec_lookup<MODE>(a, lds, stage_window<WIDE>(stg, pos), sym, L);
    return L;
}

// Clears bits [lo, hi) of a bitmap.
HZ_DEV void bmp_clear(uint32_t* bm, uint32_t lo, uint32_t hi) {
    if (lo >= hi) return;
    const uint32_t wl = lo >> 5, wh = (hi - 1) >> 5;
    for (uint32_t w = wl; w <= wh; ++w) {
        uint32_t m = 0xffffffffu;
        if (w == wl) m &= 0xffffffffu << (lo & 31);
        if (w == wh) m &= 0xffffffffu >> (31 - ((hi - 1) & 31));
        bm[w] &= ~m;
    }
}

// The 256 chain starts of a staged block of n bits, relative to its first bit, into cs[]; false when its
// codewords do not number cnt or do not end at bit n. The block is cut into 64 segments of g bits (whole
// bitmap words: a lane writes only its own). Lane 0 walks code lengths from bit 0, lane i from its guess
// i g, each to the first start at or past its segment's end (its exit), setting the bit of every start.
// Then rounds: a lane whose entry is not its left neighbour's exit clears what lies below the true entry
// and walks from there until it lands on a start of its old path (the rest of that path, and its exit,
// are the true ones) or leaves the segment. Lane i is right after round i at the latest. Every walk ends
// at its segment's end, which is at most n. `rounds`: how many were needed.
template <int MODE, bool WIDE>
HZ_DEV bool coop_starts(const DecArgs& a, const uint32_t* lds, const uint32_t* stg, uint32_t base, uint32_t n,
                        uint32_t cnt, uint32_t* bm, uint32_t* cs, int lane, uint32_t& rounds) {
    const uint32_t g = 32u * (((n + 63) / 64 + 31) / 32);
    const uint32_t ss = (uint32_t)lane * g;
    const uint32_t se = ss + g < n ? ss + g : n;       // <= ss: the lane has no bits
    const uint32_t wl = ss >> 5, wh = ss < se ? (se + 31) >> 5 : wl;  // its bitmap words [wl, wh)
    for (uint32_t w = wl; w < wh; ++w) bm[w] = 0u;
    uint32_t entry = ss < n ? ss : n;
    uint32_t ex;
    {
        uint32_t p = entry;
        while (p < se) {
            bm[p >> 5] |= 1u << (p & 31);
            const uint32_t L = slot_len<MODE, WIDE>(a, lds, stg, base + p);
            if (L == 0) { p = kDead; break; }
            p += L;
        }
        ex = p;
    }
    rounds = 0;
    bool stuck = false;
    for (;;) {
        uint32_t te = shfl_up_u32(ex, 1);
        if (lane == 0) te = 0;
        const bool dirty = te != entry;
        if (!__any(dirty)) break;
        if (rounds == kRangesMaxRounds) { stuck = true; break; }
        ++rounds;
        if (dirty) {
            entry = te;
            if (te >= se) {  // the true path skips the segment
                for (uint32_t w = wl; w < wh; ++w) bm[w] = 0u;
                ex = te;
            } else {
                bmp_clear(bm, ss, te);
                uint32_t p = te;
                for (;;) {
                    if (p >= se) { ex = p; break; }
                    const uint32_t w = p >> 5, bit = 1u << (p & 31), m = bm[w];
                    if (m & bit) break;  // on the old path: its exit stands
                    bm[w] = m | bit;
                    const uint32_t L = slot_len<MODE, WIDE>(a, lds, stg, base + p);
                    if (L == 0) { bmp_clear(bm, p + 1, se); ex = kDead; break; }
                    bmp_clear(bm, p + 1, p + L < se ? p + L : se);
                    p += L;
                }
            }
        }
    }
    // the bitmap holds exactly the true starts: count them, pick every 8th by rank
    uint32_t c = 0;
    for (uint32_t w = wl; w < wh; ++w) c += __popc(bm[w]);
    const uint32_t incl = wave_incl_sum(c);
    const bool ok = !stuck && readlane(incl, 63) == cnt && readlane(ex, 63) == n;
    if (!ok) return false;
    uint32_t run = incl - c;  // starts before the lane's words
    for (uint32_t w = wl; w < wh; ++w) {
        const uint32_t m = bm[w], pc = __popc(m);
        for (uint32_t r = (8u - (run & 7u)) & 7u; r < pc; r += 8) cs[(run + r) >> 3] = 32u * w + select_bit(m, r);
        run += pc;
    }
#pragma unroll
    for (int k = 0; k < kChainsPerLane; ++k) {  // chains past the stream's end (its last block) are idle
        const uint32_t ch = (uint32_t)(k * kWave + lane);
        if (ch * kChainSyms >= cnt) cs[ch] = n;
    }
    return true;
}

// The cold path's chain starts: lane 0 walks the block's cnt codewords over global memory as
// k_seek_subs does (the reader clamps its loads to the view, A's ld_chunk; the walk stops at cnt codewords or past
// bit n, whichever comes first).
template <int MODE, typename A>
HZ_DEV bool cold_starts(const A& a, const uint32_t* lds, uint64_t s0, uint32_t n, uint32_t cnt, uint32_t* cs,
                        int lane) {
    uint32_t ok = 0;
    if (lane == 0) {
        BitReader r;
        br_init(r, a, s0 + a.bit_adj);
        uint32_t pos = 0, i = 0;
        for (; i < cnt; ++i) {
            if ((i & (kChainSyms - 1)) == 0) cs[i / kChainSyms] = pos;
            uint32_t sym;
            const uint32_t L = br_next<MODE>(r, a, lds, sym);
            pos += L;
            if (L == 0 || pos > n) break;
        }
        ok = i == cnt && pos == n;
        for (uint32_t ch = (cnt + kChainSyms - 1) / kChainSyms; ch < (uint32_t)kChainsPerBlock; ++ch) cs[ch] = n;
    }
    return readlane(ok, 0) != 0;
}

// One wave per block job, persistent over jobs j, j + W, ... (job j of the call = block j - offs[r] of
// range r, found by a binary search in the plan's offsets). LDS: the decode table, then per wave a
// payload slot, a boundary bitmap of as many words and 256 chain starts. A block whose staging window
// does not fit the slot takes the cold path (a wave-uniform branch): one lane finds the chain starts over
// global memory and every lane decodes its chains through its own bit reader.
// PIECES: the view (a.words, a.bit_adj, a.w_first, a.nwords, y.clamp_lo, y.bit_hi, y.seek) is the job's
// piece's, rebuilt per job in the wave's own copy of the arguments.
template <int MODE, bool WIDE, bool PIECES>
__global__ __launch_bounds__(kRangesMaxWaves * 64) void k_ranges_decode(DecArgsOf<PIECES> a, SeekArgs y, RangesArgsOf<PIECES> p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint64_t total = p.offs[p.nranges];
    const uint32_t nw = blockDim.x >> 6;
    if ((uint64_t)blockIdx.x * nw >= total) return;  // before the table copy: most workgroups of a short list
    copy_lds_table(lds, a.lds_img, a.lds_words);
    const int lane = threadIdx.x & 63;
    const uint32_t wid = wave_id();
    uint32_t* stg = lds + a.lds_words + wid * p.wave_words;
    uint32_t* bm = stg + p.slot_words;
    uint32_t* cs = bm + p.slot_words;
    const uint64_t W = (uint64_t)gridDim.x * nw;
    uint32_t st_done = 0, st_cold = 0, st_rounds = 0, st_bad = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * nw + wid; j < total; j += W) {
        uint32_t ri = 0, rh = p.nranges;  // offs[ri] <= j < offs[rh]
        while (rh - ri > 1) {
            const uint32_t mid = ri + (rh - ri) / 2;
            if (p.offs[mid] <= j) ri = mid;
            else rh = mid;
        }
        const auto rg = range_at(p, ri);
        if constexpr (PIECES) piece_view(a, y, p, p.pieces[rg.piece]);
        const uint64_t lo = rg.sym_begin, hi = rg.sym_begin + rg.sym_count;
        const uint64_t b = lo / kBlockSyms + (j - p.offs[ri]);
        const uint64_t s0 = y.seek[b], s1 = y.seek[b + 1];
        const uint64_t left = y.nsym - b * kBlockSyms;
        const uint32_t cnt = left < (uint64_t)kBlockSyms ? (uint32_t)left : (uint32_t)kBlockSyms;
        uint32_t err = seek_block_err(a, y, b, s0, s1, cnt);
        const uint32_t n = (uint32_t)(s1 - s0);  // <= 2048 * max_len once the checks passed
        uint32_t pk[kSPT / 2];
        bool bad = false;  // per lane: an invalid code among the lane's symbols
        if (err) {
            // nothing of the block is read
        } else if constexpr (MODE == DEC_FIXED16) {
            if (n != 16u * cnt) err = 1u;
            const uint16_t* t16 = reinterpret_cast<const uint16_t*>(lds);
#pragma unroll
            for (int c = 0; c < kChainsPerLane; ++c) {
                const uint32_t ch = (uint32_t)(c * kWave + lane);
                const uint64_t P = s0 + 16ull * kChainSyms * ch + a.bit_adj;
                const uint64_t Wd = P >> 5;
                uint32_t w[5], o[4];
#pragma unroll
                for (int k = 0; k < 5; ++k)
                    w[k] = !err && ch * kChainSyms < cnt && Wd + k >= a.w_first && Wd + k < a.nwords ? bswap32(a.words[Wd + k]) : 0u;
                fixed16_step(t16, w, (uint32_t)P, o);
#pragma unroll
                for (int k = 0; k < 4; ++k) pk[4 * c + k] = o[k];
            }
        } else {
            const uint64_t b0 = s0 + a.bit_adj, b1 = s1 + a.bit_adj;
            const uint64_t w0 = ((b0 >> 5) & ~3ull) - 4;  // dec_stage's window: one 16-byte pad before the block
            const uint64_t npc = ((b1 >> 5) + 3 - w0 + 3) >> 2;
            const bool fits = 4 * npc <= p.slot_words;
            const uint32_t base = (uint32_t)(b0 - (w0 << 5));  // the block's first bit in the slot: 128 .. 255
            uint32_t off[kChainsPerLane];
            bool have = false;
            if (y.isub) {  // a full index: the row is there
                const uint16_t* s16 = reinterpret_cast<const uint16_t*>(y.isub) + b * kChainsPerBlock + (uint32_t)lane;
                const uint64_t sub = (uint64_t)s16[0] | ((uint64_t)s16[64] << 16) | ((uint64_t)s16[128] << 32) |
                                     ((uint64_t)s16[192] << 48);
                dec_chain_offsets(sub, s0, n, lane, off);
                have = true;
            }
            if (fits) {
                for (uint32_t q = (uint32_t)lane; q < (uint32_t)npc; q += kWave) {
                    const uint64_t w = w0 + 4ull * q;
                    uint4 v;
                    if (w >= a.w_first && w < a.nwords && w + 4 <= a.nwords) {
                        v = *reinterpret_cast<const uint4*>(a.words + w);
                    } else {  // the view's ends (w may have wrapped below word 0): zeros outside
                        uint32_t t[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const uint64_t wt = w + k;
                            t[k] = wt >= a.w_first && wt < a.nwords ? a.words[wt] : 0u;
                        }
                        v = make_uint4(t[0], t[1], t[2], t[3]);
                    }
                    reinterpret_cast<uint4*>(stg)[q] = make_uint4(bswap32(v.x), bswap32(v.y), bswap32(v.z), bswap32(v.w));
                }
                __builtin_amdgcn_wave_barrier();  // LDS ops of one wave complete in order
                if (!have) {
                    uint32_t rounds;
                    if (!coop_starts<MODE, WIDE>(a, lds, stg, base, n, cnt, bm, cs, lane, rounds)) err = 1u;
                    st_rounds = rounds > st_rounds ? rounds : st_rounds;
                }
            } else {
                ++st_cold;
                if (!have && !cold_starts<MODE>(a, lds, s0, n, cnt, cs, lane)) err = 1u;
            }
            if (!have && !err) {
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int c = 0; c < kChainsPerLane; ++c) off[c] = cs[c * kWave + lane];
            }
            if (!err) {
                uint32_t nv[kChainsPerLane];  // symbols of the stream in each chain
#pragma unroll
                for (int c = 0; c < kChainsPerLane; ++c) {
                    const uint32_t f = (uint32_t)kChainSyms * (uint32_t)(c * kWave + lane);
                    nv[c] = f >= cnt ? 0u : (cnt - f < (uint32_t)kChainSyms ? cnt - f : (uint32_t)kChainSyms);
                    off[c] = off[c] < n ? off[c] : n;  // whatever an index says, no window leaves the block's slot
                }
                if (fits) {
                    uint32_t pos[kChainsPerLane];
                    const uint32_t lim = base + n;
#pragma unroll
                    for (int c = 0; c < kChainsPerLane; ++c) pos[c] = base + off[c];
#pragma unroll
                    for (int q = 0; q < kChainSyms; ++q) {
                        uint32_t sym[kChainsPerLane], L[kChainsPerLane];
#pragma unroll
                        for (int c = 0; c < kChainsPerLane; ++c)
                            dec_lookup<MODE>(a, lds, stage_window<WIDE>(stg, pos[c]), sym[c], L[c]);
#pragma unroll
                        for (int c = 0; c < kChainsPerLane; ++c) {
                            bad |= L[c] == 0 && (uint32_t)q < nv[c];
                            pos[c] = pos[c] + L[c] < lim ? pos[c] + L[c] : lim;
                            const int i = (c * kChainSyms + q) >> 1;
                            if (q & 1) pk[i] |= sym[c] << 16;
                            else pk[i] = sym[c];
                        }
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < kChainsPerLane; ++c) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) pk[4 * c + k] = 0u;
                        if (nv[c] == 0) continue;
                        BitReader r;
                        br_init(r, a, s0 + off[c] + a.bit_adj);
                        for (uint32_t q = 0; q < nv[c]; ++q) {
                            uint32_t sym;
                            const uint32_t L = br_next<MODE>(r, a, lds, sym);
                            bad |= L == 0;
                            if (L == 0) break;
                            const uint32_t v = (sym & 0xffffu) << (16 * (q & 1)), i = 4 * c + (q >> 1);
#pragma unroll
                            for (int k = 0; k < 4; ++k) pk[4 * c + k] |= i == (uint32_t)(4 * c + k) ? v : 0u;
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();  // the slot is restaged by the next job
            }
        }
        if (!err && __any(bad)) err = 1u;
        if (err) {  // a flagged block stores nothing
            if (lane == 0) atomicOr(a.err, err);
            ++st_bad;
            continue;
        }
        ++st_done;
        const uint64_t sym0 = b * kBlockSyms;
        uint16_t* out16 = reinterpret_cast<uint16_t*>(a.out + rg.out_byte);
        if (sym0 >= lo && sym0 + kBlockSyms <= hi) {  // a whole block: dec_store's layout, 1 KiB per instruction
            uint16_t* ob = out16 + (sym0 - lo);
#pragma unroll
            for (int c = 0; c < kChainsPerLane; ++c) {
                u32x4a2 v = u32x4a2{pk[4 * c], pk[4 * c + 1], pk[4 * c + 2], pk[4 * c + 3]};
                __builtin_nontemporal_store(v, reinterpret_cast<u32x4a2*>(ob + kChainSyms * (kWave * c + lane)));
            }
        } else {
#pragma unroll
            for (int c = 0; c < kChainsPerLane; ++c) {
                const uint64_t f = sym0 + (uint64_t)kChainSyms * (uint32_t)(c * kWave + lane);
#pragma unroll
                for (uint32_t q = 0; q < (uint32_t)kChainSyms; ++q) {
                    const uint64_t sy = f + q;
                    if (sy >= lo && sy < hi) out16[sy - lo] = (uint16_t)(pk[4 * c + (q >> 1)] >> (16 * (q & 1)));
                }
            }
        }
    }
    if (p.stats && lane == 0) {
        if (st_done) atomicAdd(p.stats + 0, (unsigned long long)st_done);
        if (st_cold) atomicAdd(p.stats + 1, (unsigned long long)st_cold);
        if (st_rounds) atomicMax(p.stats + 2, (unsigned long long)st_rounds);
        if (st_bad) atomicAdd(p.stats + 3, (unsigned long long)st_bad);
    }
}

// Slot words per wave: HZ_RANGES_SLOT_WORDS (read once; tests send every block down the cold path with it), else 0.
static uint32_t ranges_slot_override() {
    static const uint32_t v = [] {
        const char* e = getenv("HZ_RANGES_SLOT_WORDS");
        const long long x = e ? atoll(e) : 0;
        return x > 0 ? (uint32_t)((x + 3) & ~3ll) : 0u;
    }();
    return v;
}

uint64_t ranges_scratch_words(uint32_t nranges) { return (uint64_t)nranges + 2; }

template <int MODE, bool WIDE, bool PIECES>
static hipError_t ranges_launch(const DecArgsOf<PIECES>& a, const SeekArgs& y, const RangesArgsOf<PIECES>& p, int waves,
                                uint32_t lds_bytes, int ncu, hipStream_t s) {
    hipError_t e = ensure_lds_limit((const void*)k_ranges_decode<MODE, WIDE, PIECES>, kLdsBytes);
    if (e != hipSuccess) return e;
    const uint32_t per_cu = kLdsBytes / lds_bytes < 2 ? 1 : 2;
    hipLaunchKernelGGL((k_ranges_decode<MODE, WIDE, PIECES>), dim3((uint32_t)ncu * per_cu), dim3(64 * waves), lds_bytes, s, a, y, p);
    return hipGetLastError();
}

// The plan, then the decode kernel of the codebook's table mode with its slots sized (both forms).
template <bool PIECES>
static hipError_t ranges_run(const Tables& t, const DecArgsOf<PIECES>& a, const SeekArgs& y, RangesArgsOf<PIECES>& p, uint64_t nsym,
                             uint32_t* d_err, int ncu, hipStream_t s) {
    hipError_t e;
    hipLaunchKernelGGL(k_ranges_plan<PIECES>, dim3(1), dim3(kPlanThreads), 0, s, p, nsym, d_err);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const uint32_t table = a.lds_words, room = kLdsBytes / 4;
    if (t.dec_mode == DEC_FIXED16) {  // positions are arithmetic: no slot, no walk
        return ranges_launch<DEC_FIXED16, false, PIECES>(a, y, p, kRangesMaxWaves, 4 * table, ncu, s);
    }
    // slots for the codebook's mean block with headroom, as run_decode sizes them; the largest that fits
    // beside the table when not even one such wave does
    const double avg = t.dec_avg_bits > (double)t.dec_min_len ? t.dec_avg_bits : (double)(t.dec_min_len > 0 ? t.dec_min_len : 1);
    const uint64_t bits = (uint64_t)(avg * (double)kBlockSyms);
    const uint32_t worst = dec_slot_words_max(a.max_len);
    uint32_t slot = dec_slot_words(bits + bits / 16 + 256, a.max_len);
    slot = slot < worst ? slot : worst;
    if (ranges_slot_override()) slot = ranges_slot_override();
    if (table + kChainsPerBlock + 8 > room) return hipErrorInvalidValue;
    const uint32_t fit = ((room - table - kChainsPerBlock) / 2) & ~3u;
    slot = slot < fit ? slot : fit;
    p.slot_words = slot;
    p.wave_words = 2 * slot + kChainsPerBlock;
    uint32_t waves = (room - table) / p.wave_words;
    waves = waves < (uint32_t)kRangesMaxWaves ? waves : (uint32_t)kRangesMaxWaves;
    const uint32_t lds_bytes = 4 * (table + waves * p.wave_words);
    if (t.dec_mode == DEC_DENSE) return ranges_launch<DEC_DENSE, false, PIECES>(a, y, p, (int)waves, lds_bytes, ncu, s);
    if (t.dec_max_len > 32) return ranges_launch<DEC_LUT, true, PIECES>(a, y, p, (int)waves, lds_bytes, ncu, s);
    return ranges_launch<DEC_LUT, false, PIECES>(a, y, p, (int)waves, lds_bytes, ncu, s);
}

hipError_t launch_decode_ranges(const Tables& t, const uint8_t* d_payload, uint64_t payload_bytes, uint64_t base,
                                const unsigned long long* d_seek, uint64_t nsym, const hz_range* d_ranges,
                                uint32_t nranges, uint8_t* d_out, uint64_t out_bytes, unsigned long long* d_stats,
                                bool full_index, unsigned long long* d_scratch, uint32_t* d_err, int ncu,
                                hipStream_t s) {
    hipError_t e;
    if (d_stats && (e = hipMemsetAsync(d_stats, 0, 8 * HZ_RANGES_STATS_WORDS, s)) != hipSuccess) return e;
    if (nranges == 0) return hipSuccess;
    RangeDecArgs a{};
    SeekArgs y{};
    fill_range_view(a, y, t, d_payload, payload_bytes, base, nsym);
    a.out = d_out; a.err = d_err;
    y.seek = d_seek;
    y.isub = full_index && t.dec_mode != DEC_FIXED16 ? d_seek + index_sub_offset(index_blocks(nsym)) : nullptr;
    RangesArgs p{};
    p.ranges = d_ranges; p.nranges = nranges; p.offs = d_scratch; p.out_bytes = out_bytes; p.stats = d_stats;
    return ranges_run<false>(t, a, y, p, nsym, d_err, ncu, s);
}

hipError_t launch_decode_ranges_pieces(const Tables& t, const uint8_t* d_buf, uint64_t buf_bytes,
                                       const unsigned long long* d_seek, uint64_t seek_words, const hz_piece* d_pieces,
                                       uint32_t npieces, uint64_t nsym, const hz_piece_range* d_ranges, uint32_t nranges,
                                       uint8_t* d_out, uint64_t out_bytes, unsigned long long* d_stats,
                                       unsigned long long* d_scratch, uint32_t* d_err, int ncu, hipStream_t s) {
    hipError_t e;
    if (d_stats && (e = hipMemsetAsync(d_stats, 0, 8 * HZ_RANGES_STATS_WORDS, s)) != hipSuccess) return e;
    if (nranges == 0) return hipSuccess;
    PieceDecArgs a{};
    SeekArgs y{};
    fill_dec_args(a, t, d_buf, buf_bytes, nsym);  // the tables; every job sets its own view (piece_view)
    a.start0 = 0;
    a.out = d_out; a.err = d_err;
    y.nsym = nsym;
    PieceRangesArgs p{};
    p.pranges = d_ranges; p.nranges = nranges; p.offs = d_scratch; p.out_bytes = out_bytes; p.stats = d_stats;
    p.pieces = d_pieces; p.npieces = npieces; p.buf = d_buf; p.buf_bytes = buf_bytes;
    p.cseek = d_seek; p.seek_words = seek_words;
    return ranges_run<true>(t, a, y, p, nsym, d_err, ncu, s);
}

}  // namespace hz
