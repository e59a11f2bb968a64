// hz_pack.hip -- the pack, its range plan, and the launch helpers no one stage owns: the u64 scan every
// stage shares, ensure_lds_limit and the table upload (stage_scatter).
//
//   k_pack     codeword lookup + bit-length scan + pack  <- Compressor.cu:50-61,541-576,182-313
#include <mutex>
#include <set>
#include <utility>

#include "hz_device.h"

namespace hz {

// Dynamic-LDS limit of a kernel: hipFuncSetAttribute is per device, so the
// (kernel, device) pairs already raised are remembered under a lock (any
// number of contexts on any devices, from any host threads).
hipError_t ensure_lds_limit(const void* fn, int bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    static std::mutex mu;
    static std::set<std::pair<std::pair<const void*, int>, int>> done;
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_pair(std::make_pair(fn, dev), bytes);
    if (done.count(key)) return hipSuccess;
    if ((e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes)) != hipSuccess) return e;
    done.insert(key);
    return hipSuccess;
}

// Table upload (hz_internal.h StageSeg): every table set of a codebook, whichever stage reads it.
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

// ===========================================================================
// Pack. A block is 2048 symbols (4 KiB of input): one wavefront, 64 lanes x
// 32 contiguous symbols. Three stream-ordered steps replace the reference's
// populateCWLength + transform_inclusive_scan + encodeFromCW
// (Compressor.cu:50-61,541-576,182-313):
//   k_pack_count : per block, bit count and the block's last 32 code bits
//   k_scan_*     : exclusive scan of block bit counts -> absolute start bits
//   k_pack_write : per block, codeword lookup + wave scan of (bits, tail) +
//                  each lane writes the 32-bit words whose LAST bit falls in
//                  its run (every word written exactly once, plain stores, no
//                  pre-zeroing, no atomics, no inter-workgroup waits)
// Code tables live in LDS (DENSE 17-bit sentinel entries, or HOT tagged
// slots) and are loaded once per workgroup of a grid-stride kernel.
// ===========================================================================
struct PackArgs {
    const uint8_t* in;
    uint64_t nsym;
    uint64_t nblocks;
    const uint32_t* lds_img;
    uint32_t lds_words;
    const unsigned long long* wide;
    const uint32_t* esc;         // HOT escapes: len << 26 | code
    const uint32_t* len8_img;    // count pass: u8 lengths (LDS image, 64 KiB)
    uint32_t hot_mask;
    uint32_t hw_mask;            // HOT: 0x003f003f, in an SGPR (a literal keeps the compiler from one v_bitop3)
    uint32_t* out;
    uint64_t out_words;          // stores beyond this are dropped and flagged
    uint32_t lead;               // bits before the stream's first bit (header pending bits)
    unsigned long long* blk;     // per block bit count (k_pack_count)
    const unsigned long long* blk_start;
    unsigned long long* index;   // block index start[] (optional, hz_internal.h)
    unsigned long long* index_sub;  // block index sub[] (four u16 chain start bits per lane, low 16 bits)
    uint32_t* err;
    uint32_t slot_words;         // k_pack_write: per-wave LDS output slot (0: store from the lanes)
    const unsigned long long* rstart;  // range plan: start bit of every range (k_range_scan)
    uint64_t bpr, nranges;       // range plan: blocks per range, ranges
    // blocks k_pack_write leaves to k_pack_cold (all but WIDE): [0] = count, then (block, start bit)
    // pairs -- the stream's last block and blocks larger than the wave's LDS slot
    unsigned long long* cold;
};

template <int MODE> struct PackEnt { using T = uint32_t; static constexpr int kShift = 26; };
template <> struct PackEnt<ENC_WIDE> { using T = uint64_t; static constexpr int kShift = 56; };
// Code length of a register entry. A HOT hit keeps its slot's tag in bit 31, so the u32 forms
// read the 5-bit field (every u32 entry is <= 26 bits long: kNarrowMaxLen).
template <int MODE>
HZ_DEV uint32_t ent_len(typename PackEnt<MODE>::T e) {
    if constexpr (MODE == ENC_WIDE) return (uint32_t)(e >> 56);
    else return __builtin_amdgcn_ubfe((uint32_t)e, 26, 5);
}

template <typename T, int SH>
HZ_DEV T pack_dense_one(const uint32_t* lds, uint32_t s) {
    const uint32_t bit = s * 17u;
    const uint32_t w = bit >> 5;
    const uint64_t two = ((uint64_t)lds[w + 1] << 32) | lds[w];
    const uint32_t f = (uint32_t)(two >> (bit & 31)) & 0x1ffffu;
    const uint32_t L = f ? 16u - (uint32_t)__builtin_ctz(f) : 0u;
    return f ? (T)((L << SH) | (f >> (17u - L))) : (T)0;
}

// The lane's 32 input symbols (64 bytes) of block `blk` and, for lanes 0..31,
// one of the previous block's last 32 symbols. Issued one block ahead of use
// (k_pack_write); lanes past a full run load from the buffer start and are
// re-read byte by byte in pack_lookup.
struct PackIn {
    uint32_t raw[kSPT / 2];
    uint32_t psym;
    uint64_t bstart;
};

// PSYM false: no previous-block symbol (the range pack carries the previous block's last bits).
template <bool PSYM = true>
HZ_DEV void pack_prefetch(const PackArgs& a, uint64_t blk, int lane, PackIn& x) {
    const uint64_t sym0 = blk * kBlockSyms + (uint64_t)lane * kSPT;
    const uint64_t ls = sym0 + kSPT <= a.nsym ? sym0 : 0;
    const uint4* p = reinterpret_cast<const uint4*>(a.in + 2 * ls);
#pragma unroll
    for (int q = 0; q < kSPT / 8; ++q) {
        const uint4 v = p[q];
        x.raw[4 * q] = v.x; x.raw[4 * q + 1] = v.y; x.raw[4 * q + 2] = v.z; x.raw[4 * q + 3] = v.w;
    }
    x.psym = 0;
    if constexpr (PSYM) {
        const uint64_t ps = blk ? blk * kBlockSyms - 32 + (uint64_t)(lane & 31) : 0;
        x.psym = *reinterpret_cast<const uint16_t*>(a.in + 2 * ps);
    }
    x.bstart = a.blk_start ? a.blk_start[blk] : 0;  // range pack: a running sum instead
}

// HOT lookups of one block in two halves, for k_pack_write's pipelined loop: issue (slot
// addresses, LDS reads, hit tests, the 33 escape loads) and, a block later, finish (the blends),
// so the escape loads' latency is covered by the previous block's count and emit.
struct HotLook {
    uint32_t x[kSPT], mk[kSPT], v[kSPT];
    uint32_t xx, xmk, xv;
};
// Slot arithmetic on both symbols of a word at once (packed 16-bit shifts): slot = s ^ (mask if
// bit 15), LDS word hot_word(slot); byte addresses (the table sits at LDS byte 0 of the pack
// kernels). A slot's entry carries its owner's bit 15 as the tag in bit 31: hit <=> bit 31 of
// entry ^ (s << 16) is 0. A miss is the slot's other symbol, whose entry the escape table holds at
// the same byte offset, so the escape address is one AND. !FULL: symbols k >= nvalid read 0.
// !XS: the lane's 32 symbols only, no 33rd lookup of xs.
template <bool FULL, bool XS = true>
HZ_DEV void hot_issue(const PackArgs& a, const uint32_t (&raw)[kSPT / 2], uint32_t xs, HotLook& h, int nvalid = kSPT) {
    const uint32_t m2 = a.hot_mask | (a.hot_mask << 16);
    uint32_t ad[kSPT];
#pragma unroll
    for (int j = 0; j < kSPT / 2; ++j) {
        const uint32_t r = raw[j];
        // (inline asm with an inline-constant shift would shift the high half by 0: VOP3P takes
        // a constant for the low half only; vector types let the compiler place the operands)
        const uint32_t sgn = __builtin_bit_cast(uint32_t, __builtin_bit_cast(hz_i16x2, r) >> (hz_i16x2){15, 15});
        const uint32_t sl = r ^ (sgn & m2);
        const uint32_t hi8 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(hz_u16x2, sl) >> (hz_u16x2){8, 8});
        // hw = sl ^ (hi8 & 0x003f003f) as one v_bitop3 (the mask in an SGPR: the compiler emits an
        // AND and an XOR for the literal), and each half's slot byte address as one SDWA shift
        // (pack 8.62 -> 8.50 ms, A/B)
        uint32_t hw, a0, a1;
        asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x6c" : "=v"(hw) : "s"(a.hw_mask), "v"(sl), "v"(hi8));
        asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0"
            : "=v"(a0) : "v"(2u), "v"(hw));
        asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1"
            : "=v"(a1) : "v"(2u), "v"(hw));
        ad[2 * j] = a0;
        ad[2 * j + 1] = a1;
    }
#pragma unroll
    for (int k = 0; k < kSPT; ++k) {
        h.x[k] = lds_at(ad[k]);
        if (!FULL) h.x[k] = k < nvalid ? h.x[k] : 0u;
    }
    uint32_t xslot = xs ^ ((uint32_t)((int32_t)(xs << 16) >> 31) & a.hot_mask);
    xslot = hot_word(xslot & 0x7fffu) << 2;
    if constexpr (XS) h.xx = lds_at(xslot);
    const char* esc = reinterpret_cast<const char*>(a.esc);
#pragma unroll
    for (int k = 0; k < kSPT; ++k) {
        const uint32_t tag = (k & 1) ? raw[k >> 1] : raw[k >> 1] << 16;
        h.mk[k] = (uint32_t)((int32_t)(h.x[k] ^ tag) >> 31);
        h.v[k] = *reinterpret_cast<const uint32_t*>(esc + (ad[k] & h.mk[k]));
    }
    if constexpr (XS) {
        h.xmk = (uint32_t)((int32_t)(h.xx ^ (xs << 16)) >> 31);
        h.xv = *reinterpret_cast<const uint32_t*>(esc + (xslot & h.xmk));
    }
}
// the blend is a v_bfi the compiler cannot turn back into a select: written as `miss ? esc[s] : e`
// the loads become 33 exec-masked branches (12.73-12.87 vs 12.61-12.67 ms at 16 GiB Zipf, round 3 A/B)
template <bool XS = true>
HZ_DEV void hot_finish(const HotLook& h, uint32_t (&e)[kSPT], uint32_t& xe) {
#pragma unroll
    for (int k = 0; k < kSPT; ++k) {
        uint32_t r;
        asm volatile("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(h.mk[k]), "v"(h.v[k]), "v"(h.x[k]));
        e[k] = r;
    }
    if constexpr (XS) {
        uint32_t r;
        asm volatile("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(h.xmk), "v"(h.xv), "v"(h.xx));
        xe = r;
    }
}

// (len, code) of the lane's 32 symbols in register format (len << SH | code),
// plus the entry of one more symbol `xs` (the previous block's tail). HOT
// slots hold tag << 31 | len << 26 | code, and every occurring symbol's code
// fits a slot (HOT mode needs max_len <= 25): an entry is a hit when its tag
// (bit 31) equals bit 15 of the symbol, i.e. when bit 31 of entry ^ tag is 0.
// Misses (the slot holds the partner symbol) come from the escape table, all
// issued before one wait. FULL: all 32 symbols valid (no per-symbol masking).
// mid() runs once the lookups' global loads are in flight and before any is
// waited on (k_pack_write issues the previous block's stores there).
struct NoMid {
    HZ_DEV void operator()() const {}
};
template <int MODE, bool FULL, typename Mid = NoMid>
HZ_DEV void pack_lookup(const PackArgs& a, const uint32_t* lds, uint64_t sym0, int nvalid, uint32_t (&raw)[kSPT / 2],
                        typename PackEnt<MODE>::T (&e)[kSPT], uint32_t xs, typename PackEnt<MODE>::T& xe,
                        Mid mid = Mid()) {
    using T = typename PackEnt<MODE>::T;
    constexpr int SH = PackEnt<MODE>::kShift;
    if (!FULL) {
#pragma unroll
        for (int k = 0; k < kSPT / 2; ++k) {
            uint32_t w = 0;
            if (2 * k < nvalid) w = (uint32_t)a.in[2 * (sym0 + 2 * k)] | ((uint32_t)a.in[2 * (sym0 + 2 * k) + 1] << 8);
            if (2 * k + 1 < nvalid)
                w |= ((uint32_t)a.in[2 * (sym0 + 2 * k + 1)] | ((uint32_t)a.in[2 * (sym0 + 2 * k + 1) + 1] << 8)) << 16;
            raw[k] = w;
        }
    }
    if constexpr (MODE == ENC_DENSE) {
#pragma unroll
        for (int k = 0; k < kSPT; ++k) {
            const uint32_t s = (raw[k >> 1] >> (16 * (k & 1))) & 0xffffu;
            const uint32_t bit = s * 17u;
            const uint32_t w = bit >> 5;
            const uint64_t two = ((uint64_t)lds[w + 1] << 32) | lds[w];
            const uint32_t f = (uint32_t)(two >> (bit & 31)) & 0x1ffffu;
            const uint32_t L = f ? 16u - (uint32_t)__builtin_ctz(f) : 0u;
            e[k] = ((FULL || k < nvalid) && f) ? (T)((L << SH) | (f >> (17u - L))) : (T)0;
        }
        xe = pack_dense_one<T, SH>(lds, xs);
        mid();
    } else if constexpr (MODE == ENC_HOT) {
        HotLook h;
        hot_issue<FULL>(a, raw, xs, h, nvalid);
        mid();
        hot_finish(h, e, xe);
    } else {
#pragma unroll
        for (int k = 0; k < kSPT; ++k) {
            const uint32_t s = (raw[k >> 1] >> (16 * (k & 1))) & 0xffffu;
            e[k] = (FULL || k < nvalid) ? (T)a.wide[s] : (T)0;
        }
        xe = (T)a.wide[xs];
        mid();
    }
}

// Bit count per block from a 64 KiB u8 length table (one LDS read per symbol).
constexpr int kCountThreads = 1024;
constexpr int kCountUnroll = 2;  // blocks in flight per wave

__global__ __launch_bounds__(kCountThreads) void k_pack_count(PackArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    {
        const uint4* src = reinterpret_cast<const uint4*>(a.len8_img);
        uint4* dst = reinterpret_cast<uint4*>(lds);
        for (uint32_t i = threadIdx.x; i < kLen8LdsBytes / 16; i += blockDim.x) dst[i] = src[i];
        __syncthreads();
    }
    const uint8_t* l8 = reinterpret_cast<const uint8_t*>(lds);
    const int lane = threadIdx.x & 63;
    const uint64_t W = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint64_t full = a.nsym / kBlockSyms;  // blocks without a tail
    uint64_t blk = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    for (; blk + (kCountUnroll - 1) * W < full; blk += kCountUnroll * W) {
        uint4 v[kCountUnroll][kSPT / 8];
#pragma unroll
        for (int u = 0; u < kCountUnroll; ++u) {
            // the sum is order-free: instruction q reads bytes [1024 q + 16 lane, +16) (fully coalesced)
            const uint4* p = reinterpret_cast<const uint4*>(a.in + 2 * (blk + u * W) * kBlockSyms) + lane;
#pragma unroll
            for (int q = 0; q < kSPT / 8; ++q) v[u][q] = p[q * kWave];
        }
#pragma unroll
        for (int u = 0; u < kCountUnroll; ++u) {
            uint32_t n = 0;
#pragma unroll
            for (int q = 0; q < kSPT / 8; ++q) {
                const uint32_t wd[4] = {v[u][q].x, v[u][q].y, v[u][q].z, v[u][q].w};
#pragma unroll
                for (int k = 0; k < 8; ++k) n += l8[len8_index((wd[k >> 1] >> (16 * (k & 1))) & 0xffffu)];
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) n += shfl_xor_u32(n, m);
            if (lane == 0) a.blk[blk + u * W] = n;
        }
    }
    for (; blk < a.nblocks; blk += W) {
        const uint64_t sym0 = blk * kBlockSyms + (uint64_t)lane * kSPT;
        uint32_t n = 0;
        if (blk < full) {
            const uint4* p = reinterpret_cast<const uint4*>(a.in + 2 * sym0);
#pragma unroll
            for (int q = 0; q < kSPT / 8; ++q) {
                const uint4 v = p[q];
                const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 8; ++k) n += l8[len8_index((wd[k >> 1] >> (16 * (k & 1))) & 0xffffu)];
            }
        } else {
            for (int k = 0; k < kSPT; ++k) {
                const uint64_t i = sym0 + k;
                if (i < a.nsym) n += l8[len8_index((uint32_t)a.in[2 * i] | ((uint32_t)a.in[2 * i + 1] << 8))];
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) n += shfl_xor_u32(n, m);
        if (lane == 0) a.blk[blk] = n;
    }
}

// Emits the lane's codes into `dst` (LDS slot or global words) starting with
// `na` bits pending in `acc`; every completed 32-bit word is stored.
template <int MODE, bool TO_LDS, typename P>
HZ_DEV void pack_emit(const typename PackEnt<MODE>::T (&e)[kSPT], uint64_t& acc, uint32_t& na, P dst, bool ok) {
    using T = typename PackEnt<MODE>::T;
    constexpr int SH = PackEnt<MODE>::kShift;
    constexpr T CMASK = (T(1) << SH) - 1;
#pragma unroll
    for (int k = 0; k < kSPT; ++k) {
        const uint32_t L = ent_len<MODE>(e[k]);
        const uint64_t c = (uint64_t)(e[k] & CMASK);
        if (MODE == ENC_WIDE && L > 32) {
            const uint32_t Lh = L - 32;
            acc = (acc << Lh) | (c >> 32);
            na += Lh;
            if (na >= 32) { na -= 32; const uint32_t w = (uint32_t)(acc >> na); if (ok) *dst = TO_LDS ? w : bswap32(w); ++dst; }
            acc = (acc << 32) | (c & 0xffffffffull);
            na += 32;
            if (na >= 32) { na -= 32; const uint32_t w = (uint32_t)(acc >> na); if (ok) *dst = TO_LDS ? w : bswap32(w); ++dst; }
        } else if (L) {
            acc = (acc << L) | c;
            na += L;
            if (na >= 32) { na -= 32; const uint32_t w = (uint32_t)(acc >> na); if (ok) *dst = TO_LDS ? w : bswap32(w); ++dst; }
        }
    }
}

// Branch-free emit into the wave's LDS slot. t = bit position in the slot;
// after each code the last completed word, (t >> 5) - 1, is (re)written, so
// no per-code branch: a word is rewritten with the same bits until the next
// one completes. Before the lane completes its first word the write goes to
// that first word (clamp; overwritten once it completes -- every lane of a
// slot-path block holds >= 32 bits, so it does). On return the low t % 32
// bits of acc are the lane's trailing partial word.
template <int MODE>
HZ_DEV void pack_emit_lds(const typename PackEnt<MODE>::T (&e)[kSPT], uint64_t& acc, uint32_t t, uint32_t* slot) {
    constexpr int SH = PackEnt<MODE>::kShift;
    const uint32_t lo = (t >> 5) + 1;
    uint32_t* base = slot - 1;
#pragma unroll
    for (int k = 0; k < kSPT; ++k) {
        const uint32_t L = ent_len<MODE>(e[k]);
        const uint32_t c = (uint32_t)e[k] & ((1u << SH) - 1u);
        acc = (acc << L) | c;
        t += L;
        const uint32_t w = __builtin_amdgcn_alignbit((uint32_t)(acc >> 32), (uint32_t)acc, t);
        const uint32_t idx = (t >> 5) > lo ? (t >> 5) : lo;
        base[idx] = w;
    }
}

// <= 8 waves: room for a block of registers in flight per lane (16 GiB Zipf, round 3: 9 / 10 waves under a
// 168-VGPR cap 11.7 / 11.0 ms vs 8 waves 9.6 ms for k_pack_write)
constexpr int kPackMaxWaves = 8;
constexpr double kPackSlotMargin = 1.12;  // LDS output slot: the Kraft-estimated block bits x this
constexpr int kPackWriteThreads = 64 * kPackMaxWaves;
constexpr int kPackCopyIters = 16;       // slot copy-out covers 16 x 64 words: a 1024-word slot

// One block of a wave between its lookup and its emit: the lane's 32 entries,
// the entry of one of the previous block's last 32 symbols, the lane's bits,
// its offset in the block, its decode-chain offsets, and the block's bits
// (wave uniform).
template <int MODE>
struct PackBlk {
    typename PackEnt<MODE>::T e[kSPT];
    typename PackEnt<MODE>::T pe;
    uint32_t n, ex_n, bits;
    uint32_t nc[kChainsPerLane];
    int nvalid;
};

// FULL_ONLY: every lane's 32 symbols are in the stream (k_pack_write's split loop: the stream's last
// block, the only partial one, is packed again by k_pack_cold; this pass only needs its lookups to be
// in bounds, which pack_prefetch's clamp gives)
template <int MODE, bool FULL_ONLY = false, typename Mid = NoMid>
HZ_DEV void pack_block_lookup(const PackArgs& a, const uint32_t* lds, uint64_t blk, int lane, PackIn& in,
                              PackBlk<MODE>& b, Mid mid = Mid()) {
    const uint64_t sym0 = blk * kBlockSyms + (uint64_t)lane * kSPT;
    if constexpr (FULL_ONLY) {
        b.nvalid = kSPT;
        pack_lookup<MODE, true>(a, lds, sym0, b.nvalid, in.raw, b.e, in.psym, b.pe, mid);
        return;
    }
    b.nvalid = sym0 >= a.nsym ? 0 : (a.nsym - sym0 >= (uint64_t)kSPT ? kSPT : (int)(a.nsym - sym0));
    // a wave-uniform choice: mid() may run wave-wide code (DPP scans of the pipelined emit), so it
    // must not run once per branch of a divergent split (the stream's last block mixes full and
    // partial lanes; the partial path handles full lanes too)
    if (__ballot(b.nvalid != kSPT) == 0)
        pack_lookup<MODE, true>(a, lds, sym0, b.nvalid, in.raw, b.e, in.psym, b.pe, mid);
    else
        pack_lookup<MODE, false>(a, lds, sym0, b.nvalid, in.raw, b.e, in.psym, b.pe, mid);
}

// A block whose words wait in the wave's LDS slot: its global stores (payload
// copy-out and index entries) are issued during the NEXT block's lookup, after
// that block's escape loads. On gfx9 stores count in vmcnt and loads wait in
// order behind them, so stores issued just before a load wait stall the wave for
// their write latency; deferred, they complete under a whole block of work.
struct PackOut {
    bool pending, fits;
    uint64_t base4, blk, bstart, sub;
    uint32_t sh4, nwords;
};

// SEEK (hz_pack_seek): a.index holds start[] alone -- the block's start bit and nothing else is stored
// (no sub[] row), and the existing instances compile as before.
template <bool SEEK = false>
HZ_DEV void pack_copyout(const PackArgs& a, const uint32_t* slot, int lane, const PackOut& p) {
    if (!p.pending) return;
    if (p.fits) {
        // Output words [wfirst, wfirst + nwords): a partial first 16-byte chunk
        // (its words before wfirst are the previous block's), whole chunks,
        // a partial last chunk. A fixed count of stores (1 + 4 + 1; lanes with
        // nothing to write rewrite the block's first word with its own value),
        // so later load waits count them statically. nwords >= 64.
        const uint32_t sh4 = p.sh4;
        const uint32_t wend = sh4 + p.nwords;                // slot index past the block
        const uint32_t cf = sh4 ? 1u : 0u, cl = wend >> 2;  // whole chunks [cf, cl)
        const uint32_t nhead = sh4 ? 4u - sh4 : 0u, ntail = wend & 3u;
        {
            const uint32_t i = (uint32_t)lane < nhead ? sh4 + (uint32_t)lane : sh4;
            a.out[p.base4 + i] = bswap32(slot[i]);
        }
#pragma unroll
        for (int it = 0; it < kPackCopyIters / 4; ++it) {
            uint32_t c = cf + (uint32_t)lane + (uint32_t)it * kWave;
            c = c < cl ? c : cl - 1;
            const uint4 v = reinterpret_cast<const uint4*>(slot)[c];
            reinterpret_cast<uint4*>(a.out + p.base4)[c] = make_uint4(bswap32(v.x), bswap32(v.y), bswap32(v.z), bswap32(v.w));
        }
        {
            const uint32_t i = (uint32_t)lane < ntail ? 4u * cl + (uint32_t)lane : sh4;
            a.out[p.base4 + i] = bswap32(slot[i]);
        }
    }
    if constexpr (SEEK) {
        if (lane == 0) a.index[p.blk] = p.bstart;
    } else if (a.index) {
        a.index_sub[p.blk * kWave + lane] = p.sub;
        if (lane == 0) a.index[p.blk] = p.bstart;
    }
    __builtin_amdgcn_wave_barrier();  // the slot's reads complete before the next emit rewrites it
}

// Lane bits, decode-chain offsets, wave scan of the bit counts.
template <int MODE>
HZ_DEV void pack_block_count(int lane, PackBlk<MODE>& b) {
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < kSPT; ++k) {
        if (k % kChainSyms == 0) b.nc[k / kChainSyms] = n;
        n += ent_len<MODE>(b.e[k]);
    }
    const uint32_t sn = wave_incl_sum(n);
    b.n = n;
    b.ex_n = sn - n;
    b.bits = readlane(sn, 63);
}

// The 32 bits before a block from pe, the entry of one of the previous block's last 32 symbols in
// each of lanes 0..31 (each code >= 1 bit): a concatenation scan (associative; (0, 0) is its
// identity, which is what DPP lanes without a source read) over the rows, then row 0 into row 1.
template <int MODE>
HZ_DEV uint32_t pack_tail_scan(typename PackEnt<MODE>::T pe) {
    using T = typename PackEnt<MODE>::T;
    constexpr T CMASK = (T(1) << PackEnt<MODE>::kShift) - 1;
    uint32_t pn = ent_len<MODE>(pe);
    uint32_t pt = (uint32_t)(pe & CMASK);  // low 32 bits of the code
    auto step = [&](uint32_t on, uint32_t ot) {
        pt = pn >= 32 ? pt : ((ot << pn) | pt);
        pn += on;
    };
    step(dpp0<kDppRowShr1>(pn), dpp0<kDppRowShr1>(pt));
    step(dpp0<kDppRowShr2>(pn), dpp0<kDppRowShr2>(pt));
    step(dpp0<kDppRowShr4>(pn), dpp0<kDppRowShr4>(pt));
    step(dpp0<kDppRowShr8>(pn), dpp0<kDppRowShr8>(pt));
    step(dpp0<kDppRowBcast15, 0xa>(pn), dpp0<kDppRowBcast15, 0xa>(pt));
    return readlane(pt, 31);
}

// The 32 bits before block `blk` of a HOT stream, looked up from the input: what a range's first
// block needs (the blocks after it take them from the emit before, pack_block_emit's CARRY).
HZ_DEV uint32_t hot_prev_tail(const PackArgs& a, uint64_t blk, int lane) {
    if (blk == 0) return a.lead;
    const uint32_t xs = *reinterpret_cast<const uint16_t*>(a.in + 2 * (blk * kBlockSyms - 32 + (uint64_t)(lane & 31)));
    uint32_t xslot = xs ^ ((uint32_t)((int32_t)(xs << 16) >> 31) & a.hot_mask);
    xslot = hot_word(xslot & 0x7fffu) << 2;
    const uint32_t xx = lds_at(xslot);
    const uint32_t xmk = (uint32_t)((int32_t)(xx ^ (xs << 16)) >> 31);  // a miss: the escape table's entry
    const uint32_t xv = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(a.esc) + (xslot & xmk));
    return pack_tail_scan<ENC_HOT>((xv & xmk) | (xx & ~xmk));
}

// The last 32 bits of a block from the entries of its last lane (32 codes of >= 1 bit), for the
// block after one that was not emitted here.
template <int MODE>
HZ_DEV uint32_t pack_own_tail(const PackBlk<MODE>& b) {
    static_assert(MODE != ENC_WIDE, "u32 entries");
    uint32_t t = 0;
#pragma unroll
    for (int k = 0; k < kSPT; ++k) t = (t << ent_len<MODE>(b.e[k])) | (b.e[k] & ((1u << PackEnt<MODE>::kShift) - 1u));
    return readlane(t, 63);
}

// Writes block `blk` starting at absolute bit `bstart`, plus its index entries. SLOT_ONLY: the caller
// has checked that the block goes through the wave's LDS slot (not the last block, fits the slot), so
// the direct path is not compiled in. CARRY (with SLOT_ONLY): *tail holds the 32 bits before the
// block (b.pe is not read) and returns the block's own last 32 bits -- the low word of lane 63's
// accumulator, since every lane holds 32 codes of >= 1 bit. SEEK: the index is start[] alone (the
// block's start bit, the stream's end after the last block; no sub[] row, no max_bits).
template <int MODE, bool SLOT_ONLY = false, bool CARRY = false, bool SEEK = false>
HZ_DEV void pack_block_emit(const PackArgs& a, uint32_t* slot, uint64_t blk, int lane, const PackBlk<MODE>& b,
                            uint64_t bstart, uint64_t& max_bits, PackOut* defer = nullptr, uint32_t* tail = nullptr) {
    static_assert(!CARRY || (SLOT_ONLY && MODE != ENC_WIDE), "the carried tail is the slot path's");
    using T = typename PackEnt<MODE>::T;
    constexpr int SH = PackEnt<MODE>::kShift;
    constexpr T CMASK = (T(1) << SH) - 1;
    const uint64_t sym0 = blk * kBlockSyms + (uint64_t)lane * kSPT;
    const uint32_t n = b.n, ex_n = b.ex_n;
    const uint64_t bend = bstart + b.bits;
    // The 32 bits before the block: codes of the previous block's last 32
    // symbols (each code >= 1 bit), combined across lanes 0..31.
    uint32_t ptail = a.lead;
    if constexpr (CARRY) ptail = *tail;
    else if (blk > 0) ptail = pack_tail_scan<MODE>(b.pe);
    const uint64_t o = bstart + ex_n;
    // every word this block writes lies below ceil(bend / 32)
    const bool fits = ((bend + 31) >> 5) <= a.out_words;
    if (!fits && lane == 0) atomicOr(a.err, 4u);
    const bool last = blk + 1 == a.nblocks;
    const uint64_t wfirst = bstart >> 5;
    const uint32_t nwords = (uint32_t)((bend >> 5) - wfirst);  // words completed inside the block
    const uint32_t sh4 = (uint32_t)(wfirst & 3);  // slot word i holds output word (wfirst & ~3) + i
    if (SLOT_ONLY || (slot && !last && nwords + sh4 <= a.slot_words)) {
        // Every lane holds 32 codes of >= 1 bit, so its last 32 bits are its
        // own: emit with the leading bits zero, then OR in the previous
        // lane's tail once all lanes are done. The slot is laid out like the
        // output modulo 16 bytes, so the copy-out moves aligned 16-byte chunks.
        uint32_t* sl = slot + sh4;  // sl[w] = output word wfirst + w
        uint64_t acc = 0;
        if constexpr (MODE == ENC_WIDE) {  // codes may exceed 32 bits
            uint32_t na = (uint32_t)(o & 31);
            pack_emit<MODE, true>(b.e, acc, na, sl + (uint32_t)((o >> 5) - wfirst), true);
        } else {
            pack_emit_lds<MODE>(b.e, acc, (uint32_t)(o - (wfirst << 5)), sl);
        }
        const uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp((int)ptail, (int)(uint32_t)acc, kDppWaveShr1,
                                                                    0xf, 0xf, false);  // lane 0: ptail
        if constexpr (CARRY) *tail = readlane((uint32_t)acc, 63);
        const uint32_t h = (uint32_t)(o & 31);
        if (h) sl[(uint32_t)((o >> 5) - wfirst)] |= prev << (32 - h);
        __builtin_amdgcn_wave_barrier();
        if (MODE != ENC_WIDE && defer) {
            defer->pending = true;
            defer->fits = fits;
            defer->base4 = wfirst & ~3ull;
            defer->sh4 = sh4;
            defer->nwords = nwords;
            defer->blk = blk;
            defer->bstart = bstart;
            if constexpr (!SEEK) {
                uint64_t sub = 0;
#pragma unroll
                for (int c = 0; c < kChainsPerLane; ++c)
                    sub |= (uint64_t)(((uint32_t)bstart + ex_n + b.nc[c]) & 0xffffu) << (16 * c);
                defer->sub = sub;
                max_bits = b.bits > max_bits ? b.bits : max_bits;
            }
            return;
        }
        if (fits) {
            if constexpr (MODE != ENC_WIDE) {  // host: slot_words <= kPackCopyIters * kWave
                // Output words [wfirst, wfirst + nwords): a partial first 16-byte chunk
                // (its words before wfirst are the previous block's), whole chunks,
                // a partial last chunk. A fixed count of stores (1 + 4 + 1; lanes with
                // nothing to write rewrite the block's first word with its own value),
                // so later load waits count them statically. nwords >= 64.
                const uint64_t base4 = wfirst & ~3ull;
                const uint32_t wend = sh4 + nwords;                 // slot index past the block
                const uint32_t cf = sh4 ? 1u : 0u, cl = wend >> 2;  // whole chunks [cf, cl)
                const uint32_t nhead = sh4 ? 4u - sh4 : 0u, ntail = wend & 3u;
                {
                    const uint32_t i = (uint32_t)lane < nhead ? sh4 + (uint32_t)lane : sh4;
                    a.out[base4 + i] = bswap32(slot[i]);
                }
#pragma unroll
                for (int it = 0; it < kPackCopyIters / 4; ++it) {
                    uint32_t c = cf + (uint32_t)lane + (uint32_t)it * kWave;
                    c = c < cl ? c : cl - 1;
                    const uint4 v = reinterpret_cast<const uint4*>(slot)[c];
                    reinterpret_cast<uint4*>(a.out + base4)[c] =
                        make_uint4(bswap32(v.x), bswap32(v.y), bswap32(v.z), bswap32(v.w));
                }
                {
                    const uint32_t i = (uint32_t)lane < ntail ? 4u * cl + (uint32_t)lane : sh4;
                    a.out[base4 + i] = bswap32(slot[i]);
                }
            } else {
                for (uint32_t w = lane; w < nwords; w += kWave) a.out[wfirst + w] = bswap32(sl[w]);
            }
        }
        __builtin_amdgcn_wave_barrier();
    } else if constexpr (!SLOT_ONLY) {
        // direct path: each lane needs the 32 bits before its run from the
        // (bits, tail) scan, since a lane of the last block may hold < 32 bits
        uint64_t t64 = 0;
#pragma unroll
        for (int k = 0; k < kSPT; ++k) {
            const uint32_t L = ent_len<MODE>(b.e[k]);
            t64 = L ? ((t64 << L) | (uint64_t)(b.e[k] & CMASK)) : t64;
        }
        uint32_t tn = n, st = (uint32_t)t64;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t on = shfl_up_u32(tn, d), ot = shfl_up_u32(st, d);
            if (lane >= d) {
                st = tn >= 32 ? st : (tn == 0 ? ot : ((ot << tn) | st));
                tn += on;
            }
        }
        uint32_t ex_t = shfl_up_u32(st, 1);
        if (lane == 0) ex_t = 0;
        const uint32_t pre = ex_n >= 32 ? ex_t : (ex_n == 0 ? ptail : ((ptail << ex_n) | ex_t));
        uint32_t na = (uint32_t)(o & 31);
        uint64_t acc = na ? (uint64_t)(pre & ((1u << na) - 1u)) : 0ull;
        uint32_t* dst = a.out + (o >> 5);
        pack_emit<MODE, false>(b.e, acc, na, dst, fits);
        dst += (uint32_t)(((o & 31) + n) >> 5);
        if (fits && b.nvalid > 0 && sym0 + (uint64_t)b.nvalid == a.nsym && na > 0)
            *dst = bswap32((uint32_t)(acc << (32 - na)));
    }
    if constexpr (SEEK) {
        if (lane == 0) {
            a.index[blk] = bstart;
            if (last) a.index[a.nblocks] = bend;
        }
    } else if (a.index) {  // block index (hz_internal.h): start bits + the lane's chain offsets
        uint64_t sub = 0;
#pragma unroll
        for (int c = 0; c < kChainsPerLane; ++c)
            sub |= (uint64_t)(((uint32_t)bstart + ex_n + b.nc[c]) & 0xffffu) << (16 * c);
        a.index_sub[blk * kWave + lane] = sub;
        if (lane == 0) {
            a.index[blk] = bstart;
            if (last) a.index[a.nblocks] = bend;
        }
        max_bits = bend - bstart > max_bits ? bend - bstart : max_bits;
    }
}


// Pack of blocks whose start bits are known: the three-pass pack (after
// k_pack_count + k_scan_*; wave w packs blocks w, w + W, ...) or, RNG, the
// range plan (after k_range_dot + k_range_scan; wave w packs the blocks of
// ranges w, w + W, ... in order, each block starting where the one before it
// ended: a running sum, no count pass). SEEK (hz_pack_seek): instances of their own that store the
// seek table -- a.index is start[] alone, written by the wave that holds each block's start bit (the
// range plan has no blk_start array to copy from); the instances without it are the code they were.
template <int MODE, bool RNG, bool SPLIT, bool SEEK = false>
__global__ __launch_bounds__(kPackWriteThreads) void k_pack_write(PackArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    if constexpr (MODE != ENC_WIDE) copy_lds_table(lds, a.lds_img, a.lds_words);
    const int lane = threadIdx.x & 63;
    // Output slot of this wave: the block's words are assembled in LDS and
    // leave as contiguous 256-byte stores. A block that does not fit, and the
    // stream's last block, go to k_pack_cold (SPLIT: the host's choice when the
    // workgroup has slots; WIDE, and a DENSE table too large for slots beside
    // it, keep the in-line direct path): without that path in the loop the
    // kernel needs 70 SGPRs and 152 VGPRs instead of 106 (51 spilled to VGPR
    // lanes, reloaded every block) and 175 (pack 8.6 -> 8.1-8.3 ms, 16 GiB Zipf).
    constexpr bool kSplit = SPLIT && MODE != ENC_WIDE;
    // (the wave index stays a VGPR value here: as a scalar, 12.4-12.7 vs 11.8-12.2 ms pack stage)
    uint32_t* slot = a.slot_words ? lds + a.lds_words + (threadIdx.x >> 6) * a.slot_words : nullptr;
    const uint64_t W = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint64_t gw = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    uint64_t max_bits = 0;  // largest block of this wave (index max_bits: one atomic per wave)
    uint64_t blk = gw, r = gw, rend = 0, run = 0;
    if (RNG) {
        blk = r < a.nranges ? r * a.bpr : a.nblocks;
        rend = blk + a.bpr < a.nblocks ? blk + a.bpr : a.nblocks;
        run = r < a.nranges ? a.rstart[r] : 0;
    }
    PackOut po;
    po.pending = false;
    if constexpr (MODE == ENC_HOT && kSplit) {
        // Pipelined: block k is finished (blends) and emitted while block k+1's escape loads and
        // block k+2's input are in flight; the wave's block sequence runs two ahead of the emit.
        // 239 VGPRs (LDS already holds the kernel at 2 waves per SIMD); pack 8.42 -> 8.33 ms mean
        // of 5 paired runs. The escapes cost issue/TA throughput more than latency: without them
        // pack takes 7.8-7.9 ms, and skipping a load no lane needs (a uniform branch) is slower
        // (8.95-9.06 ms: +2 VALU per symbol).
        auto next = [&](uint64_t b, bool& newr, uint64_t& nrun) -> uint64_t {
            newr = false;
            nrun = 0;
            if (!RNG) return b + W;
            if (b + 1 < rend) return b + 1;
            r += W;  // the wave's next range
            newr = true;
            const uint64_t n = r < a.nranges ? r * a.bpr : a.nblocks;
            rend = n + a.bpr < a.nblocks ? n + a.bpr : a.nblocks;
            nrun = r < a.nranges ? a.rstart[r] : 0;
            return n;
        };
        // RNG: a wave packs the blocks of a range in order, so the 32 bits before a block are the
        // last 32 bits of the emit before it (tail, valid when have_tail): no previous-block symbol,
        // 33rd lookup, 33rd escape load or concatenation scan per block. A range's first block looks
        // them up (hot_prev_tail); the block after a cold-listed one takes them from that block's
        // last lane (pack_own_tail).
        constexpr bool kCarry = RNG;
        uint32_t tail = 0;
        bool have_tail = false;
        bool nb_newr;
        uint64_t nb_run;
        uint64_t nb = next(blk, nb_newr, nb_run);
        PackIn nx;
        HotLook hl;
        uint64_t bst_cur = run;
        if (blk < a.nblocks) {
            PackIn cur;
            pack_prefetch<!kCarry>(a, blk, lane, cur);
            hot_issue<true, !kCarry>(a, cur.raw, cur.psym, hl);
            if (!RNG) bst_cur = cur.bstart;
            pack_prefetch<!kCarry>(a, nb < a.nblocks ? nb : blk, lane, nx);
        }
        while (blk < a.nblocks) {
            bool nn_newr;
            uint64_t nn_run;
            const uint64_t nnb = next(nb, nn_newr, nn_run);
            PackBlk<MODE> b;
            hot_finish<!kCarry>(hl, b.e, b.pe);
            b.nvalid = kSPT;
            // issue priority while the lookups and escape loads go out (the SIMD's other wave computes):
            // pack 8.31-8.33 -> 8.23-8.26 ms, A/B
            __builtin_amdgcn_s_setprio(2);
            hot_issue<true, !kCarry>(a, nx.raw, nx.psym, hl);  // block k+1 (past the wave's end: a repeat, unused)
            __builtin_amdgcn_s_setprio(0);
            const uint64_t nbst = nx.bstart;
            pack_copyout<SEEK>(a, slot, lane, po);  // block k-1's stores, behind the escape loads
            po.pending = false;
            const uint64_t pb = nnb < a.nblocks ? nnb : (nb < a.nblocks ? nb : blk);
            pack_prefetch<!kCarry>(a, pb, lane, nx);
            pack_block_count<MODE>(lane, b);
            const uint64_t bst = bst_cur;
            const uint64_t wfirst = bst >> 5;
            const uint32_t nwords = (uint32_t)(((bst + b.bits) >> 5) - wfirst), sh4 = (uint32_t)(wfirst & 3);
            if (blk + 1 == a.nblocks || nwords + sh4 > a.slot_words) {
                if (lane == 0) {
                    const unsigned long long i = atomicAdd(a.cold, 1ull);
                    a.cold[1 + 2 * i] = blk;
                    a.cold[2 + 2 * i] = bst;
                }
                if constexpr (kCarry) tail = pack_own_tail<MODE>(b);
            } else if constexpr (kCarry) {
                if (!have_tail) tail = hot_prev_tail(a, blk, lane);  // the first block of a range
                pack_block_emit<MODE, true, true, SEEK>(a, slot, blk, lane, b, bst, max_bits, &po, &tail);
            } else {
                pack_block_emit<MODE, true, false, SEEK>(a, slot, blk, lane, b, bst, max_bits, &po);
            }
            have_tail = !nb_newr;
            if (RNG) run = nb_newr ? nb_run : run + b.bits;
            bst_cur = RNG ? run : nbst;
            blk = nb;
            nb = nnb;
            nb_newr = nn_newr;
            nb_run = nn_run;
        }
        pack_copyout<SEEK>(a, slot, lane, po);
        if (!SEEK && a.index && lane == 0 && max_bits) atomicMax(a.index + a.nblocks + 1, (unsigned long long)max_bits);
        return;
    }
    PackIn nx;  // the next block's inputs, in flight while this block is packed
    if (blk < a.nblocks) pack_prefetch(a, blk, lane, nx);
    while (blk < a.nblocks) {
        uint64_t nb = blk + W, nrun = 0;
        bool newr = false;
        if (RNG) {
            if (blk + 1 < rend) {
                nb = blk + 1;
            } else {  // the wave's next range: its start bit lands during this block
                r += W;
                newr = true;
                nb = r < a.nranges ? r * a.bpr : a.nblocks;
                rend = nb + a.bpr < a.nblocks ? nb + a.bpr : a.nblocks;
                nrun = r < a.nranges ? a.rstart[r] : 0;
            }
        }
        PackIn cur = nx;
        PackBlk<MODE> b;
        // the previous block's stores go out behind this block's escape loads
        pack_block_lookup<MODE, kSplit>(a, lds, blk, lane, cur, b, [&]() { pack_copyout<SEEK>(a, slot, lane, po); });
        po.pending = false;
        // next block's loads: after this block's escapes, so no wait covers them early
        pack_prefetch(a, nb < a.nblocks ? nb : blk, lane, nx);
        pack_block_count<MODE>(lane, b);
        const uint64_t bst = RNG ? run : cur.bstart;
        if constexpr (kSplit) {
            const uint64_t wfirst = bst >> 5;
            const uint32_t nwords = (uint32_t)(((bst + b.bits) >> 5) - wfirst), sh4 = (uint32_t)(wfirst & 3);
            if (blk + 1 == a.nblocks || nwords + sh4 > a.slot_words) {  // slot_words 0: no slots, all cold
                if (lane == 0) {
                    const unsigned long long i = atomicAdd(a.cold, 1ull);
                    a.cold[1 + 2 * i] = blk;
                    a.cold[2 + 2 * i] = bst;
                }
            } else {
                pack_block_emit<MODE, true, false, SEEK>(a, slot, blk, lane, b, bst, max_bits, &po);
            }
        } else {
            pack_block_emit<MODE, false, false, SEEK>(a, slot, blk, lane, b, bst, max_bits, &po);
        }
        if (RNG) run = newr ? nrun : run + b.bits;
        blk = nb;
    }
    pack_copyout<SEEK>(a, slot, lane, po);
    if (!SEEK && a.index && lane == 0 && max_bits) atomicMax(a.index + a.nblocks + 1, (unsigned long long)max_bits);
}

// The blocks k_pack_write listed in a.cold (the stream's last block, which may be partial, and blocks
// larger than a wave's LDS slot): per-symbol masked lookups, each lane's codes stored straight to the
// output, the index entries. Usually one block; workgroups past the list leave before loading the table.
template <int MODE, bool SEEK = false>
__global__ __launch_bounds__(kPackWriteThreads) void k_pack_cold(PackArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint64_t n = a.cold[0];
    const uint64_t waves = blockDim.x >> 6, W = (uint64_t)gridDim.x * waves;
    if ((uint64_t)blockIdx.x * waves >= n) return;  // uniform over the workgroup
    if constexpr (MODE != ENC_WIDE) copy_lds_table(lds, a.lds_img, a.lds_words);
    const int lane = threadIdx.x & 63;
    uint64_t max_bits = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * waves + (threadIdx.x >> 6); i < n; i += W) {
        const uint64_t blk = a.cold[1 + 2 * i], bst = a.cold[2 + 2 * i];
        PackIn in;
        pack_prefetch(a, blk, lane, in);
        PackBlk<MODE> b;
        pack_block_lookup<MODE>(a, lds, blk, lane, in, b);
        pack_block_count<MODE>(lane, b);
        pack_block_emit<MODE, false, false, SEEK>(a, nullptr, blk, lane, b, bst, max_bits, nullptr);
    }
    if (!SEEK && a.index && lane == 0 && max_bits) atomicMax(a.index + a.nblocks + 1, (unsigned long long)max_bits);
}

// ---- every code 16 bits (U = 65 536, min_len = max_len = 16) ---------------
// Symbol i starts at bit start_bit + 16 i: no count pass and no scan. Lane j
// packs symbols [32 j, 32 j + 32) into the 16 words whose last bit lies in its
// run; word t is a funnel shift of code pairs t-1 and t by start_bit % 32.
// Full blocks [0, nb) of a FIXED16 stream: one wave per block; lane l's sub-run c is the block's symbols 8 (64 c + l) .. + 7, i.e. 16 input bytes and 4
// output words at 1 KiB-coalesced offsets (the lane-run kernel below moves 64 contiguous bytes per
// lane, so each of its 16-byte accesses touches 64 separate pieces). Word t of a sub-run is a funnel
// shift of code pairs t - 1 and t; pair -1 is lane l - 1's last (DPP), sub-run c - 1's lane 63 for
// lane 0, or, for the block's first, the pair before the block (loaded) or the header's pending bits.
__global__ __launch_bounds__(kPackThreads) void k_pack_fixed16_blk(PackArgs a, uint64_t start_bit, uint64_t nb) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    copy_lds_table(lds, a.lds_img, a.lds_words);
    const uint16_t* c16 = reinterpret_cast<const uint16_t*>(lds);
    const uint32_t sb = (uint32_t)(start_bit & 31);
    const int lane = threadIdx.x & 63;
    const uint4* in4 = reinterpret_cast<const uint4*>(a.in);
    u32x4a4* out4 = reinterpret_cast<u32x4a4*>(a.out + (start_bit >> 5));  // any word of the stream
    const uint64_t W = (uint64_t)gridDim.x * (blockDim.x >> 6);
    uint64_t b = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    auto load = [&](uint64_t bb, uint4 (&x)[kChainsPerLane]) {
        bb = bb < nb ? bb : 0;
#pragma unroll
        for (int c = 0; c < kChainsPerLane; ++c) x[c] = in4[bb * (kBlockSyms / 8) + c * kWave + lane];
    };
    uint4 nx[kChainsPerLane];
    if (b < nb) load(b, nx);
    for (; b < nb; b += W) {
        uint4 x[kChainsPerLane];
#pragma unroll
        for (int c = 0; c < kChainsPerLane; ++c) x[c] = nx[c];
        load(b + W, nx);
        uint32_t p0 = a.lead;  // the pair before the block (same address on every lane)
        if (b > 0) {
            const uint32_t pr = *reinterpret_cast<const uint32_t*>(a.in + 2 * (b * kBlockSyms - 2));
            p0 = ((uint32_t)c16[pr & 0xffffu] << 16) | c16[pr >> 16];
        }
        uint32_t last = p0;  // sub-run c - 1's last pair on lane 63 (wave-uniform)
#pragma unroll
        for (int c = 0; c < kChainsPerLane; ++c) {
            const uint32_t raw[4] = {x[c].x, x[c].y, x[c].z, x[c].w};
            uint32_t v[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] = ((uint32_t)c16[raw[t] & 0xffffu] << 16) | c16[raw[t] >> 16];
            uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v[3], kDppWaveShr1, 0xf, 0xf, false);
            if (lane == 0) prev = last;
            last = readlane(v[3], 63);
            uint32_t o[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const uint32_t pp = t ? v[t - 1] : prev;
                o[t] = sb ? __builtin_amdgcn_alignbit(pp, v[t], sb) : v[t];
            }
            u32x4a4 ov;
            ov.x = bswap32(o[0]); ov.y = bswap32(o[1]); ov.z = bswap32(o[2]); ov.w = bswap32(o[3]);
            out4[b * (kBlockSyms / 8) + c * kWave + lane] = ov;
        }
        if (a.index) {
            const uint32_t bs = (uint32_t)(start_bit + (uint64_t)b * kBlockSyms * 16);
            uint64_t sub = 0;
#pragma unroll
            for (int c = 0; c < kChainsPerLane; ++c)
                sub |= (uint64_t)((bs + 16u * (kSPT * (uint32_t)lane + kChainSyms * c)) & 0xffffu) << (16 * c);
            a.index_sub[b * kWave + lane] = sub;
            if (lane == 0) a.index[b] = start_bit + (uint64_t)b * kBlockSyms * 16;
            if (b == 0 && lane == 0) a.index[a.nblocks + 1] = 16ull * kBlockSyms;
        }
    }
}

// Lane runs [j_begin, ...) of 32 symbols (the stream's tail after k_pack_fixed16_blk, or all of it).
__global__ __launch_bounds__(kPackThreads) void k_pack_fixed16(PackArgs a, uint64_t start_bit, uint64_t j_begin) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    copy_lds_table(lds, a.lds_img, a.lds_words);
    const uint16_t* c16 = reinterpret_cast<const uint16_t*>(lds);
    const uint32_t sb = (uint32_t)(start_bit & 31);
    const uint64_t W0 = start_bit >> 5;
    const uint64_t nl = (a.nsym + kSPT - 1) / kSPT;
    const uint64_t end_word = (start_bit + 16 * a.nsym + 31) >> 5;  // words holding stream bits
    const bool fits = end_word <= a.out_words;
    if (!fits && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.err, 4u);
    const bool vec_out = (W0 & 3) == 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    // the lane's 64 input bytes of run j (full runs; 0 past them), loaded one
    // iteration ahead so a load is always in flight beside the table lookups
    auto load_run = [&](uint64_t j, uint32_t (&raw)[kSPT / 2]) {
        const uint64_t ls = j < nl && (j + 1) * kSPT <= a.nsym ? j * kSPT : 0;
        const uint4* p = reinterpret_cast<const uint4*>(a.in + 2 * ls);
#pragma unroll
        for (int q = 0; q < kSPT / 8; ++q) {
            const uint4 v = p[q];
            raw[4 * q] = v.x; raw[4 * q + 1] = v.y; raw[4 * q + 2] = v.z; raw[4 * q + 3] = v.w;
        }
    };
    uint32_t nraw[kSPT / 2];
    const uint64_t j0 = j_begin + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    load_run(j0, nraw);
    for (uint64_t j = j0; j < nl; j += stride) {  // the loop is uniform except in the last round
        const uint64_t sym0 = j * kSPT;
        const int nvalid = a.nsym - sym0 >= (uint64_t)kSPT ? kSPT : (int)(a.nsym - sym0);
        uint32_t raw[kSPT / 2];
#pragma unroll
        for (int k = 0; k < kSPT / 2; ++k) raw[k] = nraw[k];
        load_run(j + stride, nraw);
        if (nvalid != kSPT) {
#pragma unroll
            for (int k = 0; k < kSPT / 2; ++k) raw[k] = 0;
            for (int k = 0; k < nvalid; ++k)
                raw[k >> 1] |= ((uint32_t)a.in[2 * (sym0 + k)] | ((uint32_t)a.in[2 * (sym0 + k) + 1] << 8)) << (16 * (k & 1));
        }
        uint32_t v[kSPT / 2];
#pragma unroll
        for (int t = 0; t < kSPT / 2; ++t) {
            const uint32_t lo = (uint32_t)c16[raw[t] & 0xffffu], hi = (uint32_t)c16[raw[t] >> 16];
            v[t] = (2 * t < nvalid ? lo << 16 : 0u) | (2 * t + 1 < nvalid ? hi : 0u);
        }
        // the previous run's last code pair (or the header's pending bits): from
        // lane - 1 by DPP (run j - 1 when that lane is active in this round), else loaded
        uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v[kSPT / 2 - 1], kDppWaveShr1, 0xf, 0xf, false);
        if ((threadIdx.x & 63) == 0 && j > 0) {
            const uint32_t pr = *reinterpret_cast<const uint32_t*>(a.in + 2 * (sym0 - 2));
            prev = ((uint32_t)c16[pr & 0xffffu] << 16) | c16[pr >> 16];
        }
        if (j == 0) prev = a.lead;
        uint32_t o[kSPT / 2];
#pragma unroll
        for (int t = 0; t < kSPT / 2; ++t) {
            const uint32_t p = t ? v[t - 1] : prev;
            o[t] = sb ? (uint32_t)(((((uint64_t)p) << 32) | v[t]) >> sb) : v[t];
        }
        const uint64_t wj = W0 + 16 * j;
        if (fits) {
            if (nvalid == kSPT && j + 1 < nl && vec_out) {
                uint4* d = reinterpret_cast<uint4*>(a.out + wj);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    d[q] = make_uint4(bswap32(o[4 * q]), bswap32(o[4 * q + 1]), bswap32(o[4 * q + 2]), bswap32(o[4 * q + 3]));
            } else {
                // words whose first bit is a stream bit; the last lane also
                // writes the word its final bits spill into
#pragma unroll
                for (int t = 0; t < kSPT / 2; ++t)
                    if (wj + t < end_word) a.out[wj + t] = bswap32(o[t]);
                if (j + 1 == nl && wj + 16 < end_word)
                    a.out[wj + 16] = bswap32((uint32_t)(((uint64_t)v[15] << 32) >> sb));
            }
        }
        if (a.index) {
            const uint64_t blk = j / kWave;
            const uint32_t lane = (uint32_t)(j % kWave);
            const uint32_t cnt = (uint32_t)(a.nsym - blk * kBlockSyms < (uint64_t)kBlockSyms ? a.nsym - blk * kBlockSyms
                                                                                        : (uint64_t)kBlockSyms);
            uint64_t sub = 0;
            const uint32_t bs = (uint32_t)(start_bit + (uint64_t)blk * kBlockSyms * 16);
#pragma unroll
            for (int c = 0; c < kChainsPerLane; ++c) {
                const uint32_t at = kSPT * lane + kChainSyms * c;
                sub |= (uint64_t)((bs + 16 * (at < cnt ? at : cnt)) & 0xffffu) << (16 * c);
            }
            a.index_sub[j] = sub;
            if (lane == 0) a.index[blk] = start_bit + (uint64_t)blk * kBlockSyms * 16;
            if (j + 1 == nl) {
                a.index[a.nblocks] = start_bit + 16 * a.nsym;
                // the last block's lanes past the stream's end run no iteration: their chains start at
                // the end bit, as pack_block_emit / hz_index_build / hz_index_expand write them
                const uint64_t e16 = (start_bit + 16 * a.nsym) & 0xffffu;
                for (uint64_t q = nl; q < a.nblocks * kWave; ++q) a.index_sub[q] = e16 * 0x0001000100010001ull;
            }
            if (j == 0) a.index[a.nblocks + 1] = 16ull * (a.nsym < (uint64_t)kBlockSyms ? a.nsym : (uint64_t)kBlockSyms);
        }
    }
}

// ---- exclusive scan of block bit counts (low 32 bits of blk[]) -------------
// (tile constants and block_exclusive_scan: hz_device.h)
// mask: the bits of each entry that are its count (the pack's block entries: the low 32; chain counts: all)
__global__ __launch_bounds__(kScanThreads) void k_scan_reduce(const unsigned long long* blk, uint64_t nblocks,
                                                              unsigned long long* tile_sum, uint64_t mask) {
    __shared__ uint64_t sh[17];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPer;
    uint64_t s = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k)
        if (base + k < nblocks) s += blk[base + k] & mask;
    uint64_t total;
    block_exclusive_scan(s, sh, total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kScanThreads) void k_scan_tiles(unsigned long long* tile_sum, uint64_t ntiles,
                                                             uint64_t start_bit) {
    __shared__ uint64_t sh[17];
    uint64_t carry = start_bit;
    for (uint64_t b = 0; b < ntiles; b += kScanThreads) {
        const uint64_t i = b + threadIdx.x;
        const uint64_t v = i < ntiles ? tile_sum[i] : 0;
        uint64_t total;
        const uint64_t ex = block_exclusive_scan(v, sh, total);
        if (i < ntiles) tile_sum[i] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(kScanThreads) void k_scan_apply(const unsigned long long* blk, uint64_t nblocks,
                                                             const unsigned long long* tile_off,
                                                             unsigned long long* blk_start, uint64_t mask) {
    __shared__ uint64_t sh[17];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPer;
    uint64_t c[kScanPer];
    uint64_t s = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        c[k] = base + k < nblocks ? blk[base + k] & mask : 0u;
        s += c[k];
    }
    uint64_t total;
    uint64_t run = tile_off[blockIdx.x] + block_exclusive_scan(s, sh, total);
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        if (base + k < nblocks) blk_start[base + k] = run;
        run += c[k];
    }
}

hipError_t launch_scan(const unsigned long long* v, uint64_t n, unsigned long long* tiles, unsigned long long* out,
                       uint64_t mask, uint64_t seed, hipStream_t s) {
    const uint64_t ntiles = (n + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(k_scan_reduce, dim3(ntiles), dim3(kScanThreads), 0, s, v, n, tiles, mask);
    hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(kScanThreads), 0, s, tiles, ntiles, seed);
    hipLaunchKernelGGL(k_scan_apply, dim3(ntiles), dim3(kScanThreads), 0, s, v, n, (const unsigned long long*)tiles,
                       out, mask);
    return hipGetLastError();
}

// ---- range plan: bits and start of every range ------------------------------
// dot[j] = sum over bins of len * (the cumulative count of workgroup j % groups
// after its range j): the snapshot's u16 halves plus 65 536 x its carry records
// up to range j. lenpair: the two code lengths of every histogram word (u8 each,
// hist_word order, hz_codebook_upload_encode).
constexpr int kDotThreads = 256;
__global__ __launch_bounds__(kDotThreads) void k_range_dot(RangeArgs r, const uint32_t* __restrict__ lenpair) {
    __shared__ unsigned long long red[kDotThreads / 64];
    const uint16_t* lp16 = reinterpret_cast<const uint16_t*>(lenpair);
    for (uint64_t j = blockIdx.x; j < r.nranges; j += gridDim.x) {
        const uint4* sp = reinterpret_cast<const uint4*>(r.snap) + j * 8192;
        const uint2* lp = reinterpret_cast<const uint2*>(lenpair);  // 4 length pairs per 16 snapshot bytes
        auto mac = [](uint32_t v, uint32_t l) { return (v & 0xffffu) * (l & 0xffu) + (v >> 16) * ((l >> 8) & 0xffu); };
        uint32_t acc = 0;  // <= 32 x 4 x 2 x 65535 x 56 < 2^32
        for (uint32_t q = threadIdx.x; q < 8192; q += kDotThreads) {
            const uint4 v = sp[q];
            const uint2 l = lp[q];
            acc += mac(v.x, l.x) + mac(v.y, l.x >> 16) + mac(v.z, l.y) + mac(v.w, l.y >> 16);
        }
        uint64_t sum = acc;
        const uint32_t g = (uint32_t)(j % r.groups), k = (uint32_t)(j / r.groups);
        const uint32_t* list = r.list + (uint64_t)g * (1 + r.list_cap);
        const uint32_t n = list[0] < r.list_cap ? list[0] : r.list_cap;
        for (uint32_t t = threadIdx.x; t < n; t += kDotThreads) {
            const uint32_t e = list[1 + t];
            if ((e >> 17) > k) continue;
            const uint32_t bin = e & 0xffffu;
            const uint64_t L = (lp16[hist_word(bin)] >> (8 * (bin & 1))) & 0xffu;
            sum += (e >> 16) & 1u ? (uint64_t)0 - (L << 16) : L << 16;  // mod 2^64: the total is >= 0
        }
        sum = wave_sum_u64(sum);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t t = 0;
            for (int w = 0; w < kDotThreads / 64; ++w) t += red[w];
            r.dot[j] = t;
        }
        __syncthreads();
    }
}

// start[j] = start_bit + sum of bits of ranges < j; bits_j = dot[j] - dot[j - groups]
// (the same workgroup's previous snapshot); start[nranges] = the stream's end.
__global__ __launch_bounds__(kScanThreads) void k_range_scan(RangeArgs r, uint64_t start_bit) {
    __shared__ uint64_t sh[17];
    uint64_t carry = start_bit;
    for (uint64_t b = 0; b < r.nranges; b += kScanThreads) {
        const uint64_t j = b + threadIdx.x;
        const uint64_t v = j < r.nranges ? r.dot[j] - (j >= r.groups ? r.dot[j - r.groups] : 0ull) : 0ull;
        uint64_t total;
        const uint64_t ex = block_exclusive_scan(v, sh, total);
        if (j < r.nranges) r.start[j] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) r.start[r.nranges] = carry;
}

uint64_t pack_scratch_words(uint64_t nsym) {
    const uint64_t nblocks = (nsym + kBlockSyms - 1) / kBlockSyms;
    const uint64_t ntiles = (nblocks + kScanTile - 1) / kScanTile;
    return 2 * nblocks + ntiles + 1 + 2 * nblocks;  // counts, starts, scan tiles, k_pack_cold's list
}

// The k_pack_write instance: SPLIT (cold blocks to k_pack_cold) for HOT, and for DENSE when the
// workgroup has output slots; WIDE and a slot-less DENSE keep the direct path in the loop (split,
// every block of a slot-less pack would be looked up twice).
template <bool SEEK>
static const void* pack_write_inst(int mode, bool rng, bool split) {
    if (mode == ENC_HOT)
        return rng ? (const void*)k_pack_write<ENC_HOT, true, true, SEEK> : (const void*)k_pack_write<ENC_HOT, false, true, SEEK>;
    if (mode == ENC_DENSE) {
        if (split)
            return rng ? (const void*)k_pack_write<ENC_DENSE, true, true, SEEK>
                       : (const void*)k_pack_write<ENC_DENSE, false, true, SEEK>;
        return rng ? (const void*)k_pack_write<ENC_DENSE, true, false, SEEK> : (const void*)k_pack_write<ENC_DENSE, false, false, SEEK>;
    }
    return rng ? (const void*)k_pack_write<ENC_WIDE, true, false, SEEK> : (const void*)k_pack_write<ENC_WIDE, false, false, SEEK>;
}
static const void* pack_write_fn(int mode, bool rng, bool split, bool seek) {
    return seek ? pack_write_inst<true>(mode, rng, split) : pack_write_inst<false>(mode, rng, split);
}
static const void* pack_cold_fn(int mode, bool seek) {
    if (mode == ENC_DENSE) return seek ? (const void*)k_pack_cold<ENC_DENSE, true> : (const void*)k_pack_cold<ENC_DENSE>;
    return seek ? (const void*)k_pack_cold<ENC_HOT, true> : (const void*)k_pack_cold<ENC_HOT>;
}
static hipError_t pack_write_launch(const void* fn, uint64_t grid, int threads, uint32_t lds, hipStream_t s, PackArgs a) {
    void* args[] = {&a};
    return hipLaunchKernel(fn, dim3((uint32_t)grid), dim3(threads), args, lds, s);
}

// k_pack_write's list of blocks for k_pack_cold: zero the count first, run the cold pass after.
static hipError_t pack_cold_reset(const PackArgs& a, hipStream_t s) {
    return hipMemsetAsync(a.cold, 0, sizeof(unsigned long long), s);
}
static void pack_cold_launch(const Tables& t, const PackArgs& a, uint32_t lds, int ncu, hipStream_t s, bool seek) {
    const uint64_t waves = kPackWriteThreads / 64;
    uint64_t g = (a.nblocks + waves - 1) / waves;
    if (g > (uint64_t)ncu) g = ncu;  // table-sized LDS: one workgroup per CU
    // (WIDE keeps the direct path inside k_pack_write)
    if (t.enc_mode == ENC_DENSE || t.enc_mode == ENC_HOT)
        (void)pack_write_launch(pack_cold_fn(t.enc_mode, seek), g, kPackWriteThreads, lds, s, a);
}

hipError_t launch_pack(const Tables& t, const uint8_t* d_in, uint64_t nsym, uint64_t start_bit, uint32_t lead,
                       uint32_t* d_out, uint64_t out_words, unsigned long long* d_scratch,
                       unsigned long long* d_index, uint32_t* d_err, int ncu, hipStream_t s, void* d_ranges,
                       int* used_ranges, bool seek) {
    if (used_ranges) *used_ranges = 0;
    if (nsym == 0) return hipSuccess;
    const uint64_t nblocks = (nsym + kBlockSyms - 1) / kBlockSyms;
    const uint64_t ntiles = (nblocks + kScanTile - 1) / kScanTile;
    PackArgs a;
    a.in = d_in; a.nsym = nsym; a.nblocks = nblocks;
    a.lds_img = t.d_enc_lds; a.lds_words = t.enc_lds_bytes / 4;
    a.wide = reinterpret_cast<const unsigned long long*>(t.d_enc_wide);
    a.esc = t.d_enc_esc; a.len8_img = t.d_len8; a.hot_mask = t.hot_mask; a.hw_mask = 0x003f003fu;
    a.out = d_out; a.out_words = out_words; a.lead = lead;
    a.blk = d_scratch;
    unsigned long long* blk_start = d_scratch + nblocks;
    unsigned long long* tiles = d_scratch + 2 * nblocks;
    a.blk_start = blk_start; a.index = d_index; a.err = d_err;
    a.index_sub = d_index && !seek ? d_index + index_sub_offset(nblocks) : nullptr;
    // seek: d_index is start[] alone (nblocks + 1 words). Every code of a FIXED16 stream starts at
    // start_bit + 16 i: the caller writes that table without the kernels (seek_fixed16)
    if (seek && t.enc_mode == ENC_FIXED16) a.index = nullptr;
    a.rstart = nullptr; a.bpr = 0; a.nranges = 0;
    a.cold = tiles + ntiles;
    if (d_index && !seek && t.enc_mode != ENC_FIXED16) {
        hipError_t e = hipMemsetAsync(d_index + nblocks + 1, 0, 8, s);  // max_bits, raised per block
        if (e != hipSuccess) return e;
    }
    if (t.enc_mode == ENC_FIXED16) {
        hipError_t e = ensure_lds_limit((const void*)k_pack_fixed16, kFixed16LdsBytes);
        if (e != hipSuccess) return e;
        if ((e = ensure_lds_limit((const void*)k_pack_fixed16_blk, kFixed16LdsBytes)) != hipSuccess) return e;
        const uint64_t nl = (nsym + kSPT - 1) / kSPT;
        // every block but the last through the coalesced kernel when it fits; the lane-run kernel
        // takes the rest (the stream's end, the index end)
        const uint64_t nb = nblocks - 1;
        const bool blk = kFixed16Blk && nb > 0 && (start_bit >> 5) + nb * (kBlockSyms / 2) <= out_words;
        uint64_t jb = 0;
        if (blk) {
            uint64_t wgs = (nb + kPackThreads / 64 - 1) / (kPackThreads / 64);
            if (wgs > (uint64_t)ncu) wgs = ncu;  // 128 KiB table: one workgroup per CU
            hipLaunchKernelGGL(k_pack_fixed16_blk, dim3(wgs), dim3(kPackThreads), kFixed16LdsBytes, s, a, start_bit, nb);
            jb = nb * kWave;
        }
        uint64_t wgs = (nl - jb + kPackThreads - 1) / kPackThreads;
        if (wgs > (uint64_t)ncu) wgs = ncu;  // 128 KiB table: one workgroup per CU
        hipLaunchKernelGGL(k_pack_fixed16, dim3(wgs), dim3(kPackThreads), kFixed16LdsBytes, s, a, start_bit, jb);
        return hipGetLastError();
    }
    // Waves per workgroup: as many output slots of the expected block size
    // (Kraft estimate from the code lengths, +12 %) as fit beside the table.
    const uint32_t table_words = t.enc_mode == ENC_WIDE ? 0 : t.enc_lds_bytes / 4;
    a.lds_words = table_words;
    const uint32_t free_words = kLdsBytes / 4 - table_words;
    const uint32_t est_words = (uint32_t)(t.enc_avg_bits * kBlockSyms * kPackSlotMargin / 32.0) + 4;
    constexpr uint32_t kMaxWaves = kPackWriteThreads / 64;
    uint32_t waves = free_words / est_words;
    waves = waves > kMaxWaves ? kMaxWaves : waves;
    a.slot_words = 0;
    if (waves >= 6) a.slot_words = free_words / waves & ~3u;  // 16-byte aligned slots
    else waves = kMaxWaves;  // no room for slots: lanes store directly
    if (t.enc_mode != ENC_WIDE && a.slot_words > (uint32_t)(kPackCopyIters * kWave))
        a.slot_words = kPackCopyIters * kWave;  // larger blocks take the direct path
    const int threads = (int)waves * 64;
    uint64_t wgs = (nblocks + waves - 1) / waves;
    const uint32_t lds = 4 * (table_words + waves * a.slot_words);
    const uint64_t cap = (uint64_t)ncu * (lds ? kLdsBytes / lds : 4);
    if (wgs > cap) wgs = cap;
    // Range plan (the histogram's snapshots, hz_hist16_ranges): every pack wave takes whole ranges,
    // so the plan is used when the waves cover the ranges evenly; else count + scan + write.
    // k_pack_write leaves its cold blocks to k_pack_cold (HOT always has slots: mean code <= 17 bits)
    const bool split = t.enc_mode == ENC_HOT || (t.enc_mode == ENC_DENSE && a.slot_words > 0);
    if (split) {
        hipError_t e = ensure_lds_limit(pack_cold_fn(t.enc_mode, seek), kLdsBytes);
        if (e != hipSuccess) return e;
        if ((e = pack_cold_reset(a, s)) != hipSuccess) return e;
    }
    const RangeGeom g = d_ranges ? range_geom(nsym) : RangeGeom{};
    if (g.bytes && t.d_lenpair) {
        uint64_t rw = (g.nranges + waves - 1) / waves;
        if (rw > cap) rw = cap;
        const uint64_t W = rw * waves;
        if (W >= g.nranges || g.nranges % W == 0) {
            const void* fr = pack_write_fn(t.enc_mode, true, split, seek);
            hipError_t e = ensure_lds_limit(fr, kLdsBytes);
            if (e != hipSuccess) return e;
            const RangeArgs r = range_args(d_ranges, g, d_err);
            uint64_t dg = g.nranges < (uint64_t)ncu * 4 ? g.nranges : (uint64_t)ncu * 4;
            hipLaunchKernelGGL(k_range_dot, dim3(dg), dim3(kDotThreads), 0, s, r, (const uint32_t*)t.d_lenpair);
            hipLaunchKernelGGL(k_range_scan, dim3(1), dim3(kScanThreads), 0, s, r, start_bit);
            a.rstart = r.start; a.bpr = g.bpr; a.nranges = g.nranges; a.blk_start = nullptr;
            if ((e = pack_write_launch(fr, rw, threads, lds, s, a)) != hipSuccess) return e;
            if (split) pack_cold_launch(t, a, 4 * table_words, ncu, s, seek);
            if (used_ranges) *used_ranges = 1;
            return hipGetLastError();
        }
    }
    {
        hipError_t e = ensure_lds_limit((const void*)k_pack_count, kLen8LdsBytes);
        if (e != hipSuccess) return e;
        if ((e = ensure_lds_limit(pack_write_fn(t.enc_mode, false, split, seek), kLdsBytes)) != hipSuccess) return e;
    }
    {
        const uint64_t cw = kCountThreads / 64;
        uint64_t cg = (nblocks + cw - 1) / cw;
        if (cg > (uint64_t)ncu * 2) cg = (uint64_t)ncu * 2;  // two 64 KiB-LDS workgroups per CU
        hipLaunchKernelGGL(k_pack_count, dim3(cg), dim3(kCountThreads), kLen8LdsBytes, s, a);
    }
    {
        hipError_t e = launch_scan(a.blk, nblocks, tiles, blk_start, 0xffffffffull, start_bit, s);
        if (e != hipSuccess) return e;
        if ((e = pack_write_launch(pack_write_fn(t.enc_mode, false, split, seek), wgs, threads, lds, s, a)) != hipSuccess) return e;
    }
    if (split) pack_cold_launch(t, a, 4 * table_words, ncu, s, seek);
    return hipGetLastError();
}

// hz_pack_seek's placement: the n entries at d (the call's window of the stream's table) count from
// byte 0 of the call's output; the table counts bit_base further.
__global__ __launch_bounds__(256) void k_seek_add(unsigned long long* d, uint64_t n, uint64_t add) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] += add;
}

hipError_t launch_seek_add(unsigned long long* d, uint64_t n, uint64_t add, hipStream_t s) {
    if (n == 0 || add == 0) return hipSuccess;
    hipLaunchKernelGGL(k_seek_add, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, d, n, add);
    return hipGetLastError();
}

}  // namespace hz
