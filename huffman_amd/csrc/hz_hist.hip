// hz_hist.hip -- the synthetic input generator and the 65 536-bin histogram.
//
//   k_generate synthetic Zipf / uniform byte streams (this build's generator)
//   k_hist16   65 536-bin histogram of u16 symbols      <- Compressor.cu:38-48
#include "hz_device.h"

namespace hz {

HZ_DEV uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// ===========================================================================
// Synthetic input generator (not a reference function).
// ===========================================================================
HZ_DEV uint8_t gen_byte(uint64_t j, int kind, uint64_t seed, const unsigned long long* t) {
    uint64_t u = splitmix64(seed ^ j);
    if (kind == 0) return (uint8_t)u;
    int lo = 0, hi = 255;
    while (lo < hi) {
        int m = (lo + hi) >> 1;
        if (u < t[m]) hi = m; else lo = m + 1;
    }
    return (uint8_t)lo;
}

__global__ __launch_bounds__(256) void k_generate(uint8_t* __restrict__ out, uint64_t n, uint64_t offset,
                                                 int kind, uint64_t seed,
                                                 const unsigned long long* __restrict__ thr) {
    __shared__ unsigned long long t[256];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) t[i] = thr ? thr[i] : 0ull;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const bool aligned = (((uintptr_t)out) & 7) == 0;
    const uint64_t nv = aligned ? n / 8 : 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < nv; i += stride) {
        uint64_t w = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) w |= (uint64_t)gen_byte(offset + i * 8 + k, kind, seed, t) << (8 * k);
        reinterpret_cast<uint64_t*>(out)[i] = w;
    }
    for (uint64_t j = nv * 8 + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += stride)
        out[j] = gen_byte(offset + j, kind, seed, t);
}

hipError_t launch_generate(uint8_t* d_out, uint64_t n, uint64_t offset, int kind, uint64_t seed,
                           const unsigned long long* d_thr, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const unsigned grid = (unsigned)grid_clamp((n / 8 + 255) / 256, 8192);
    hipLaunchKernelGGL(k_generate, dim3(grid), dim3(256), 0, s, d_out, n, offset, kind, seed, d_thr);
    return hipGetLastError();
}

// ===========================================================================
// Histogram: 65 536 u16 counters packed two per LDS dword (128 KiB, one
// 1024-thread workgroup per CU). A counter half that wraps is corrected
// exactly through the value the LDS atomic returns (DESIGN.md "Histogram").
// ===========================================================================
constexpr int kHistThreads = 1024;

// (LDS word of a symbol pair: hist_word, hz_internal.h)

// Fix-up after `old = atomicAdd(&lds[hist_word(s)], inc)`; rare (once per 65 536 adds of a bin).
// rec(bin, negative) sees every +-65 536 the global histogram receives (range snapshots).
struct NoRec {
    HZ_DEV void operator()(uint32_t, uint32_t) const {}
};
template <typename Rec = NoRec>
HZ_DEV void hist_fix(uint32_t* lds, unsigned long long* hist, uint32_t s, uint32_t old, Rec rec = Rec()) {
    const uint32_t inc = (s & 1) ? 0x10000u : 1u;
    if (old + inc < old) {  // the dword (high half) wrapped
        atomicAdd(&hist[s | 1], 65536ull);
        rec(s | 1, 0u);
    }
    if (!(s & 1) && (old & 0xffffu) == 0xffffu) {  // low half crossed 65 536: undo its carry
        atomicAdd(&hist[s], 65536ull);
        rec(s, 0u);
        uint32_t o2 = atomicSub(&lds[hist_word(s)], 0x10000u);
        if (o2 < 0x10000u) {
            atomicAdd(&hist[s | 1], (unsigned long long)(-65536ll));
            rec(s | 1, 1u);
        }
    }
}

HZ_DEV bool hist_needs_fix(uint32_t s, uint32_t old) {
    const uint32_t inc = (s & 1) ? 0x10000u : 1u;
    return (old + inc < old) | (!(s & 1) & ((old & 0xffffu) == 0xffffu));
}

template <typename Rec = NoRec>
HZ_DEV void hist_one(uint32_t* lds, unsigned long long* hist, uint32_t s, Rec rec = Rec()) {
    uint32_t old = atomicAdd(&lds[hist_word(s)], (s & 1) ? 0x10000u : 1u);
    if (hist_needs_fix(s, old)) hist_fix(lds, hist, s, old, rec);
}

// The 8 symbols of a 16-byte vector: 8 LDS atomics; a fix-up is due exactly when the
// incremented half was 0xffff (the half a symbol counts in is its bit 0, the shift 16 * bit 0).
// hist_word of both symbols of a dword at once (packed 16-bit shifts and multiply).
template <typename Rec = NoRec>
HZ_DEV void hist_count8(uint32_t* lds, unsigned long long* hist, const uint4& v, Rec rec = Rec()) {
    const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
    uint32_t old[8], sh[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const hz_u16x2 w = __builtin_bit_cast(hz_u16x2, wd[j]);
        const hz_u16x2 hw = (w >> (hz_u16x2){1, 1}) ^ (((w >> (hz_u16x2){8, 8}) * (hz_u16x2){13, 13}) & (hz_u16x2){0x3f, 0x3f});
        const uint32_t a = __builtin_bit_cast(uint32_t, hw);  // hist_word of both symbols (< 32768 each)
        sh[2 * j] = (wd[j] << 4) & 16u;
        sh[2 * j + 1] = (wd[j] >> 12) & 16u;
        old[2 * j] = atomicAdd(&lds[a & 0x7fffu], 1u << sh[2 * j]);
        old[2 * j + 1] = atomicAdd(&lds[a >> 16], 1u << sh[2 * j + 1]);
    }
    bool any = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) any |= __builtin_amdgcn_ubfe(old[k], sh[k], 16) == 0xffffu;
    if (__builtin_expect(any, 0)) {
        for (int k = 0; k < 8; ++k) {
            const uint32_t s = (wd[k >> 1] >> (16 * (k & 1))) & 0xffffu;
            if (hist_needs_fix(s, old[k])) hist_fix(lds, hist, s, old[k], rec);
        }
    }
}

// Vectors [i0, end) of in4 with stride `step` from this thread's i0: software pipelined over
// kHistDepth register buffers (no copies). One workgroup per CU leaves 16 waves to cover
// HBM latency, so each lane keeps DEPTH - 1 loads in flight while one vector's LDS atomics
// run (loads and LDS ops use separate counters). Refills past the end re-read the last
// vector (branch-free, so the waits stay vmcnt(DEPTH - 1)); the tail counts what is left.
constexpr int kHistDepth = 8;
template <typename Rec = NoRec>
HZ_DEV void hist_sweep(uint32_t* lds, unsigned long long* hist, const uint4* in4, uint64_t i, uint64_t end,
                       uint64_t step, Rec rec = Rec()) {
    constexpr int D = kHistDepth;
    if (i >= end) return;
    const uint64_t last = end - 1;
    uint4 v[D];
#pragma unroll
    for (int k = 0; k < D; ++k) v[k] = in4[i + k * step < end ? i + k * step : last];
    for (; i + (D - 1) * step < end; i += D * step) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
            hist_count8(lds, hist, v[k], rec);
            const uint64_t nx = i + (k + D) * step;
            v[k] = in4[nx < end ? nx : last];
        }
    }
#pragma unroll
    for (int k = 0; k < D - 1; ++k)
        if (i + k * step < end) hist_count8(lds, hist, v[k], rec);
}

// Adds the workgroup's LDS histogram to the global one.
HZ_DEV void hist_flush(const uint32_t* lds, unsigned long long* hist) {
    for (int i = threadIdx.x; i < 32768; i += blockDim.x) {
        const uint32_t v = lds[i];
        const uint32_t s2 = hist_word_inv((uint32_t)i) << 1;  // the symbol pair this word counts
        if (v & 0xffffu) atomicAdd(&hist[s2], (unsigned long long)(v & 0xffffu));
        if (v >> 16) atomicAdd(&hist[s2 + 1], (unsigned long long)(v >> 16));
    }
}

template <bool VEC>
__global__ __launch_bounds__(kHistThreads) void k_hist16(const uint8_t* __restrict__ in, uint64_t nsym,
                                                         unsigned long long* __restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    for (int i = threadIdx.x; i < 32768; i += blockDim.x) lds[i] = 0;
    __syncthreads();
    uint64_t tail_begin = 0;
    if (VEC) {
        // the whole chip sweeps the input together (neighbouring 16 KiB pieces),
        // one vector (8 symbols) per lane per step
        const uint64_t nvec = nsym / 8;
        hist_sweep(lds, hist, reinterpret_cast<const uint4*>(in), (uint64_t)blockIdx.x * blockDim.x + threadIdx.x,
                   nvec, (uint64_t)gridDim.x * blockDim.x);
        tail_begin = nvec * 8;
    }
    // Scalar symbols: the < 8-symbol tail (VEC) or everything (unaligned input).
    {
        const uint64_t nscalar = nsym - tail_begin;
        const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
        for (uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; k < nscalar; k += stride) {
            const uint64_t i = tail_begin + k;
            hist_one(lds, hist, (uint32_t)in[2 * i] | ((uint32_t)in[2 * i + 1] << 8));
        }
    }
    __syncthreads();
    hist_flush(lds, hist);
}

// ---- range plan histogram (hz_internal.h RangeGeom) -------------------------

// Workgroup g sweeps ranges g, g + groups, ... (each a contiguous stretch of whole
// blocks; the last one ends at the stream's end) and stores its CUMULATIVE LDS
// image after each: range j's bits are then dot(j) - dot(j - groups), the
// difference of two snapshots weighted by the code lengths plus the carries the
// workgroup made in between (k_range_dot). The global histogram equals k_hist16's.
// Input 16-byte aligned (ranges start on block boundaries: whole vectors).
__global__ __launch_bounds__(kHistThreads) void k_hist16_rng(const uint8_t* __restrict__ in,
                                                             unsigned long long* __restrict__ hist, RangeArgs r) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    for (int i = threadIdx.x; i < 32768; i += blockDim.x) lds[i] = 0;
    if (threadIdx.x == 0) r.list[(uint64_t)blockIdx.x * (1 + r.list_cap)] = 0u;
    __syncthreads();
    const uint4* in4 = reinterpret_cast<const uint4*>(in);
    uint32_t* list = r.list + (uint64_t)blockIdx.x * (1 + r.list_cap);
    uint32_t k = 0;  // the range's index among this workgroup's (< 2^15)
    for (uint64_t j = blockIdx.x; j < r.nranges; j += r.groups, ++k) {
        const uint64_t s0 = j * r.bpr * kBlockSyms;
        const uint64_t s1 = s0 + r.bpr * kBlockSyms < r.nsym ? s0 + r.bpr * kBlockSyms : r.nsym;
        auto rec = [&](uint32_t bin, uint32_t neg) {
            const uint32_t i = atomicAdd(list, 1u);
            if (i < r.list_cap) list[1 + i] = (k << 17) | (neg << 16) | bin;
            else atomicOr(r.err, 16u);  // cannot happen (RangeGeom bound): flagged, never silent
        };
        const uint64_t v1 = s1 / 8;
        hist_sweep(lds, hist, in4, s0 / 8 + threadIdx.x, v1, blockDim.x, rec);
        for (uint64_t q = v1 * 8 + threadIdx.x; q < s1; q += blockDim.x)  // the stream's < 8-symbol tail
            hist_one(lds, hist, (uint32_t)in[2 * q] | ((uint32_t)in[2 * q + 1] << 8), rec);
        __syncthreads();
        uint4* dst = reinterpret_cast<uint4*>(r.snap) + j * 8192;
        const uint4* src = reinterpret_cast<const uint4*>(lds);
        for (int q = threadIdx.x; q < 8192; q += blockDim.x) dst[q] = src[q];
        __syncthreads();
    }
    hist_flush(lds, hist);
}

hipError_t launch_hist16(const uint8_t* d_in, uint64_t n, unsigned long long* d_hist, int ncu, hipStream_t s) {
    const uint64_t nsym = n / 2;
    if (nsym == 0) return hipSuccess;
    const bool vec = (((uintptr_t)d_in) & 15) == 0;
    const void* fn = vec ? (const void*)k_hist16<true> : (const void*)k_hist16<false>;
    hipError_t e = ensure_lds_limit(fn, 131072);
    if (e != hipSuccess) return e;
    // One workgroup per CU; fewer for small inputs (every WG zeroes + flushes 128 KiB).
    const unsigned grid = (unsigned)grid_clamp((nsym + 65535) / 65536, (uint64_t)ncu);
    if (vec)
        hipLaunchKernelGGL(k_hist16<true>, dim3(grid), dim3(kHistThreads), 131072, s, d_in, nsym, d_hist);
    else
        hipLaunchKernelGGL(k_hist16<false>, dim3(grid), dim3(kHistThreads), 131072, s, d_in, nsym, d_hist);
    return hipGetLastError();
}

hipError_t launch_hist16_ranges(const uint8_t* d_in, uint64_t n, unsigned long long* d_hist, void* d_ranges,
                                uint32_t* d_err, hipStream_t s) {
    const RangeGeom g = range_geom(n / 2);
    if (!g.bytes || (((uintptr_t)d_in) & 15) || (((uintptr_t)d_ranges) & 15)) return hipErrorInvalidValue;
    hipError_t e = ensure_lds_limit((const void*)k_hist16_rng, 131072);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_hist16_rng, dim3(g.groups), dim3(kHistThreads), 131072, s, d_in, d_hist,
                       range_args(d_ranges, g, d_err));
    return hipGetLastError();
}

}  // namespace hz
