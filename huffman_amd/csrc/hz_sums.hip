// hz_sums.hip -- block checksums of data on the device (the seekable trailer's sums, hz_seekable.h).
//
//   k_block_sums        one Adler-32 (RFC 1950) per 4096 bytes, the last block zero-extended
//   k_block_sums_check  the same words compared with expected ones: the smallest block that differs
//   k_block_sums_mark   the same comparison with every block that differs marked in a bitmap, and zeroed on request
//
// The reference has no counterpart: its format carries no checksum.
#include "hz_device.h"

namespace hz {

constexpr uint32_t kSumBlockBytes = 2 * kBlockSyms;  // 4096: one seek-table block of output
constexpr uint32_t kAdlerMod = 65521;
constexpr int kSumThreads = 256;                     // four waves: four blocks per workgroup and step
static_assert(kSumBlockBytes == HZ_SUM_BLOCK_BYTES, "one sum per seek-table block");
static_assert(kSumBlockBytes == 4 * 16 * kWave, "a lane takes four 16-byte loads of its block");

// The 16 bytes at in + a that lie below n, bytes at or past n as zeros. Whole vectors take one
// 16-byte load; the vector that holds byte n - 1 is read word by word, only the words that begin
// below n, so no load leaves [in, in + n) rounded up to a 4-byte word.
HZ_DEV uint4 sums_load16(const uint8_t* __restrict__ in, uint64_t a, uint64_t n) {
    if (a + 16 <= n) return *reinterpret_cast<const uint4*>(in + a);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint64_t wa = a + 4 * k;
        if (wa < n) {
            w[k] = *reinterpret_cast<const uint32_t*>(in + wa);
            if (n - wa < 4) w[k] &= (1u << (8 * (uint32_t)(n - wa))) - 1u;
        }
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// A 16-byte vector at byte `o` of its block, bytes d_0 .. d_15: s1 takes their sum S (four SADs
// against zero), s2 takes sum (4096 - o - k) d_k = (4096 - o) S - sum k d_k (four dot4s with the
// byte weights k).
HZ_DEV void sums_add16(const uint4& v, uint32_t o, uint32_t& s1, uint32_t& s2) {
    uint32_t s = __builtin_amdgcn_sad_u8(v.x, 0u, 0u);
    s = __builtin_amdgcn_sad_u8(v.y, 0u, s);
    s = __builtin_amdgcn_sad_u8(v.z, 0u, s);
    s = __builtin_amdgcn_sad_u8(v.w, 0u, s);
    uint32_t p = __builtin_amdgcn_udot4(v.x, 0x03020100u, 0u, false);
    p = __builtin_amdgcn_udot4(v.y, 0x07060504u, p, false);
    p = __builtin_amdgcn_udot4(v.z, 0x0b0a0908u, p, false);
    p = __builtin_amdgcn_udot4(v.w, 0x0f0e0d0cu, p, false);
    s1 += s;
    s2 += (kSumBlockBytes - o) * s - p;
}

// One block's word, uniform over its wave. Lane l reads at 16 l + 1024 j of the block, j = 0..3: a wave-load
// is 1 KiB contiguous. 4096 + s2 <= 4096 + 255 * 4096 * 4097 / 2 < 2^32, and every lane's share is
// non-negative, so 32-bit sums need no reduction before the end.
HZ_DEV uint32_t sums_block(const uint8_t* __restrict__ in, uint64_t n, uint64_t b, uint32_t lane) {
    const uint64_t base = b * kSumBlockBytes;
    uint4 v[4];
    if (base + kSumBlockBytes <= n) {  // wave-uniform: every block but the last partial one
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const uint4*>(in + base + 16u * lane + 1024u * j);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = sums_load16(in, base + 16u * lane + 1024u * j, n);
    }
    uint32_t s1 = 0, s2 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) sums_add16(v[j], 16u * lane + 1024u * j, s1, s2);
    s1 = readlane(wave_incl_sum(s1), 63);  // DPP sums; the wave's totals are uniform from here
    s2 = readlane(wave_incl_sum(s2), 63);
    return ((kSumBlockBytes + s2) % kAdlerMod) << 16 | (1u + s1) % kAdlerMod;
}

// One wave per block, grid-stride over the blocks.
__global__ __launch_bounds__(kSumThreads) void k_block_sums(const uint8_t* __restrict__ in, uint64_t n,
                                                           uint64_t nblocks, uint32_t* __restrict__ sums) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t step = (uint64_t)gridDim.x * (kSumThreads / kWave);
    for (uint64_t b = (uint64_t)blockIdx.x * (kSumThreads / kWave) + wave_id(); b < nblocks; b += step) {
        const uint32_t word = sums_block(in, n, b, lane);
        if (lane == 0u) sums[b] = word;
    }
}

// The same pass with nothing stored: block b's word against expect[b], and the smallest block_base + b that
// differs folded into *bad (the caller's, never initialised here: calls accumulate into one word).
__global__ __launch_bounds__(kSumThreads) void k_block_sums_check(const uint8_t* __restrict__ in, uint64_t n,
                                                                 uint64_t nblocks, const uint32_t* __restrict__ expect,
                                                                 uint64_t block_base, unsigned long long* __restrict__ bad) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t step = (uint64_t)gridDim.x * (kSumThreads / kWave);
    for (uint64_t b = (uint64_t)blockIdx.x * (kSumThreads / kWave) + wave_id(); b < nblocks; b += step) {
        const uint32_t word = sums_block(in, n, b, lane);
        if (lane == 0u && word != expect[b]) atomicMin(bad, (unsigned long long)(block_base + b));
    }
}

// Zeros over block b's bytes below n: the layout of sums_block's loads, a 16-byte store wherever the whole
// vector lies below n. The vector that holds byte n - 1 goes out as its whole words below n and then single
// bytes, so no store touches a byte at or past n.
HZ_DEV void sums_zero_block(uint8_t* data, uint64_t n, uint64_t b, uint32_t lane) {
    const uint64_t base = b * kSumBlockBytes;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint64_t a = base + 16u * lane + 1024u * j;
        if (a + 16 <= n) {
            *reinterpret_cast<uint4*>(data + a) = make_uint4(0u, 0u, 0u, 0u);
        } else if (a < n) {
            for (uint64_t q = a; q < n;) {
                if (q + 4 <= n) {
                    *reinterpret_cast<uint32_t*>(data + q) = 0u;
                    q += 4;
                } else {
                    data[q++] = 0;
                }
            }
        }
    }
}

// The comparison again, every verdict kept: a block whose word differs sets bit (block_base + b) & 31 of
// bits[(block_base + b) >> 5] (the caller's bitmap, never initialised here: the windows of one file fold into
// one) and, with `zero`, loses its bytes below n. The word and expect[b] are the same in every lane: the
// branch is wave-uniform, and a block that matches is never written.
__global__ __launch_bounds__(kSumThreads) void k_block_sums_mark(uint8_t* data, uint64_t n, uint64_t nblocks,
                                                                const uint32_t* __restrict__ expect, uint64_t block_base,
                                                                uint32_t* bits, bool zero) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t step = (uint64_t)gridDim.x * (kSumThreads / kWave);
    for (uint64_t b = (uint64_t)blockIdx.x * (kSumThreads / kWave) + wave_id(); b < nblocks; b += step) {
        const uint32_t word = sums_block(data, n, b, lane);
        if (word == expect[b]) continue;
        const uint64_t g = block_base + b;
        if (lane == 0u) atomicOr(bits + (g >> 5), 1u << (uint32_t)(g & 31u));
        if (zero) sums_zero_block(data, n, b, lane);
    }
}

// eight workgroups (32 waves, 128 KiB of loads in flight) per CU, the rest by the grid stride
static unsigned sums_grid(uint64_t nblocks, int ncu) { return (unsigned)grid_clamp((nblocks + 3) / 4, (uint64_t)ncu * 8); }

hipError_t launch_block_sums(const uint8_t* d_in, uint64_t n, uint32_t* d_sums, int ncu, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t nblocks = (n + kSumBlockBytes - 1) / kSumBlockBytes;
    hipLaunchKernelGGL(k_block_sums, dim3(sums_grid(nblocks, ncu)), dim3(kSumThreads), 0, s, d_in, n, nblocks, d_sums);
    return hipGetLastError();
}

hipError_t launch_block_sums_check(const uint8_t* d_in, uint64_t n, const uint32_t* d_expect, uint64_t block_base,
                                   unsigned long long* d_bad, int ncu, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t nblocks = (n + kSumBlockBytes - 1) / kSumBlockBytes;
    hipLaunchKernelGGL(k_block_sums_check, dim3(sums_grid(nblocks, ncu)), dim3(kSumThreads), 0, s, d_in, n, nblocks, d_expect,
                       block_base, d_bad);
    return hipGetLastError();
}

hipError_t launch_block_sums_mark(uint8_t* d_data, uint64_t n, const uint32_t* d_expect, uint64_t block_base,
                                  uint32_t* d_bits, bool zero_bad, int ncu, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t nblocks = (n + kSumBlockBytes - 1) / kSumBlockBytes;
    hipLaunchKernelGGL(k_block_sums_mark, dim3(sums_grid(nblocks, ncu)), dim3(kSumThreads), 0, s, d_data, n, nblocks, d_expect,
                       block_base, d_bits, zero_bad);
    return hipGetLastError();
}

}  // namespace hz
