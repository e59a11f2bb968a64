// hz_device.h -- what every gfx950 translation unit shares: wave and LDS helpers (force-inlined
// device functions; no relocatable device code) and the launch helpers that cross units (defined in
// hz_pack.hip, as is stage_scatter, hz_internal.h). What only the decode side shares: hz_decode_device.h,
// hz_walk_device.h.
#pragma once
#include "hz_internal.h"

namespace hz {

#define HZ_DEV __device__ __forceinline__

// Raises a kernel's dynamic-LDS limit once per device (one definition, hz_pack.hip: it keeps the set
// of (kernel, device) pairs already raised).
hipError_t ensure_lds_limit(const void* fn, int bytes);

// Workgroups of a grid-stride launch: what the work asks for, at least one, at most cap.
inline uint64_t grid_clamp(uint64_t want, uint64_t cap) { return want < cap ? (want ? want : 1) : cap; }

HZ_DEV uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

typedef short hz_i16x2 __attribute__((ext_vector_type(2)));           // packed 16-bit lanes (v_pk_*)
typedef unsigned short hz_u16x2 __attribute__((ext_vector_type(2)));

// 16 bytes at a 4-byte aligned address (global_load/store_dwordx4 need only dword alignment): the
// FIXED16 block kernels move a stream that starts at any word behind the header.
typedef uint32_t u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x4a2 __attribute__((ext_vector_type(4), aligned(2)));  // 16 bytes at a 2-byte aligned address

// One 16-byte non-temporal store (global_store_dwordx4 ... nt).
HZ_DEV void store_nt16(uint4* p, uint4 v) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    __builtin_nontemporal_store(v.x, q);
    __builtin_nontemporal_store(v.y, q + 1);
    __builtin_nontemporal_store(v.z, q + 2);
    __builtin_nontemporal_store(v.w, q + 3);
}
HZ_DEV uint32_t shfl_up_u32(uint32_t v, int d) { return (uint32_t)__shfl_up((int)v, d, 64); }
HZ_DEV uint32_t shfl_u32(uint32_t v, int src) { return (uint32_t)__shfl((int)v, src, 64); }
HZ_DEV uint32_t shfl_xor_u32(uint32_t v, int m) { return (uint32_t)__shfl_xor((int)v, m, 64); }
// DPP lane moves (VALU, no LDS round trip). Lanes whose source lies outside
// the row (row_shr) or outside row_mask read 0.
template <int CTRL, int ROWS = 0xf>
HZ_DEV uint32_t dpp0(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xf, false);
}
constexpr int kDppRowShr1 = 0x111, kDppRowShr2 = 0x112, kDppRowShr4 = 0x114, kDppRowShr8 = 0x118;
constexpr int kDppRowBcast15 = 0x142, kDppRowBcast31 = 0x143, kDppWaveShr1 = 0x138, kDppWaveShl1 = 0x130;
constexpr bool kFixed16Blk = true;  // FIXED16 streams: the 1 KiB-coalesced full-block kernels

// Inclusive prefix sum over the 64 lanes.
HZ_DEV uint32_t wave_incl_sum(uint32_t v) {
    v += dpp0<kDppRowShr1>(v);
    v += dpp0<kDppRowShr2>(v);
    v += dpp0<kDppRowShr4>(v);
    v += dpp0<kDppRowShr8>(v);
    v += dpp0<kDppRowBcast15, 0xa>(v);
    v += dpp0<kDppRowBcast31, 0xc>(v);
    return v;
}

HZ_DEV uint32_t readlane(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }

// LDS word at byte address `byte` of a kernel without static LDS (its dynamic
// LDS starts at address 0): no base add per access.
typedef __attribute__((address_space(3))) const uint32_t lds_cu32;
HZ_DEV uint32_t lds_at(uint32_t byte) { return *reinterpret_cast<lds_cu32*>(byte); }
// The wave's index in its workgroup as a wave-uniform (SGPR) value: block numbers derived from it,
// and the index / start loads they address, stay on the scalar unit.
HZ_DEV uint32_t wave_id() {
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

HZ_DEV uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        uint32_t lo = shfl_xor_u32((uint32_t)v, m), hi = shfl_xor_u32((uint32_t)(v >> 32), m);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

HZ_DEV uint32_t pick4(const uint4& v, uint32_t i) {
    return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w));
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

HZ_DEV void copy_lds_table(uint32_t* lds, const uint32_t* img, uint32_t words) {
    const uint4* src = reinterpret_cast<const uint4*>(img);
    uint4* dst = reinterpret_cast<uint4*>(lds);
    for (uint32_t i = threadIdx.x; i < words / 4; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}

// ---- exclusive scan of u64 counts (k_scan_*, hz_pack.hip) ---------------------
constexpr int kScanThreads = 1024;
constexpr int kScanPer = 16;                         // counts per thread
constexpr int kScanTile = kScanThreads * kScanPer;   // 16 384 blocks per tile

HZ_DEV uint64_t block_exclusive_scan(uint64_t v, uint64_t* sh, uint64_t& total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint64_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t lo = shfl_up_u32((uint32_t)x, d), hi = shfl_up_u32((uint32_t)(x >> 32), d);
        if (lane >= d) x += ((uint64_t)hi << 32) | lo;
    }
    if (lane == 63) sh[wid] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t s = 0;
        for (int w = 0; w < nw; ++w) { const uint64_t t = sh[w]; sh[w] = s; s += t; }
        sh[nw] = s;
    }
    __syncthreads();
    total = sh[nw];
    const uint64_t r = sh[wid] + x - v;
    __syncthreads();
    return r;
}

// out[i] = seed + sum of (v[j] & mask) over j < i (stream ordered; tiles: (n + kScanTile - 1) / kScanTile
// words of scratch). mask: the bits of each entry that are its count (the pack's block entries: the low
// 32; chain counts: all).
hipError_t launch_scan(const unsigned long long* v, uint64_t n, unsigned long long* tiles, unsigned long long* out,
                       uint64_t mask, uint64_t seed, hipStream_t s);  // hz_pack.hip

}  // namespace hz
