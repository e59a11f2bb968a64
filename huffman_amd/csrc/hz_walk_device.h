// hz_walk_device.h -- what the chain walker (hz_chain.hip, k_chain_walk) takes from the index walker
// (hz_index.hip, k_idx_walk): the walkers' arguments, the clamped payload loads, the register group a
// ring is fed from and the walk's tuning constants; and kSyncThreads, the launch bound of the index
// builder's and the chain decode's one-lane-per-item kernels. Force-inlined device functions only.
#pragma once
#include "hz_device.h"

namespace hz {

constexpr int kSyncThreads = 1024;  // one lane per segment / chain / record: 16 waves share a table copy

// The walkers (k_idx_walk, hz_index.hip, describes the walk; k_chain_walk, hz_chain.hip).
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

}  // namespace hz
