// hz_host.h -- what the three host units share: the context (hz_host.cpp: contexts, table uploads, the
// stream-ordered stage calls), and the status and RAII helpers the whole-buffer flows (hz_image.cpp) and
// the streaming archive / extract (hz_stream.cpp) use beside it. Private to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <new>
#include <vector>

#include "huffman_amd.h"
#include "hz_internal.h"

namespace hz {

// HZ_DEBUG=1: a failing HIP call is named on stderr (file line, call, HIP's message) before HZ_EHIP.
static inline int hz_hip_fail(hipError_t e, const char* what, const char* file, int line) {
    static const bool dbg = getenv("HZ_DEBUG") != nullptr;
    if (dbg) fprintf(stderr, "[huffman_amd] %s:%d %s: %s\n", file, line, what, hipGetErrorString(e));
    return HZ_EHIP;
}
// (__FILE_NAME__: the unit the failing call stands in, without the build's directories)
#define HZ_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return hz::hz_hip_fail(_e, #x, __FILE_NAME__, __LINE__); } while (0)

// No C++ exception crosses the C ABI: entry points that allocate host
// containers run their body through this guard.
template <typename F>
static int guarded(F&& f) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return HZ_ENOMEM;
    } catch (...) {
        return HZ_EINVAL;
    }
}

// Pinned host staging for table uploads (see hz_codebook_upload_encode).
struct Staging {
    uint8_t* p = nullptr;
    size_t cap = 0, used = 0;
    hipEvent_t done = nullptr;
    std::vector<StageSeg> pend;  // staged, not yet copied (staging_flush)
};

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t n) { return hipMalloc(&p, n ? n : 16) == hipSuccess ? HZ_OK : HZ_ENOMEM; }
};

// No file header is longer: 12 + 65 536 x (3 + 8) bytes, and the device writer stores whole words. What
// the by-path calls read of a file before they parse it, and the device header writer's buffer.
constexpr uint64_t kMaxHeaderBytes = 1u << 20;
static_assert(kMaxHeaderBytes >= 12 + 65536ull * 11 + 4, "the longest header, in whole words");

// The process-wide context of the hz_*_host and file calls (created on first use, device 0).
int default_ctx(hz_ctx** out);

}  // namespace hz

struct hz_ctx {
    int device = 0;
    int ncu = 0;
    hz::ChainState* chain = nullptr;  // the index-less decoder's phases (hz_decode_indexless, hz_indexless_*)
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hz::Tables t;
    unsigned long long* d_desc = nullptr;  // pack scratch: block counts, starts, tile sums
    uint64_t desc_cap = 0;          // u64 words
    uint32_t* d_err = nullptr;
    uint32_t* h_err = nullptr;      // pinned
    unsigned long long* d_thr = nullptr;
    unsigned long long* d_cbws = nullptr;  // hz_codebook_build_device workspace
    double thr_alpha = -1.0;
    hipEvent_t ev[5][2] = {};
    bool ev_used[5] = {false, false, false, false, false};
    // encode tables, decode tables, and the index-less decoder's tables (walk length and escape tables,
    // a DENSE codebook's chain LUT): built with the decode tables, copied by the first call that needs
    // them (hz_decode_indexless, hz_indexless_scan, hz_index_build) -- a decode with a block index never
    // uploads them
    hz::Staging stage_enc, stage_dec, stage_walk;
    size_t cap_enc_lds = 0, cap_enc_esc = 0, cap_enc_wide = 0, cap_len8 = 0, cap_lenpair = 0, cap_dec_lds = 0,
           cap_dec_l2 = 0, cap_walk_lds = 0, cap_walk_esc = 0, cap_walk8 = 0, cap_chain_lds = 0, cap_chain_l2 = 0,
           cap_chain_esc = 0;
    int last_pack_ranges = 0;       // the last hz_pack_ranges call took the range plan
    int last_decode_chunks = 0;     // staging chunks per block of the last hz_decode (launch_decode)
    // a FIXED16 part of hz_indexless_scan (every code 16 bits: positions are arithmetic, no chains)
    struct {
        bool on = false;
        const uint8_t* payload = nullptr;
        uint64_t bytes = 0, base = 0, start = 0, entry = 0, xit = 0;
    } fx;
    // the least explicit entry bit of the pending part (chains or FIXED16): its first bit, start_bit +
    // part_begin, which the view holds (hz_indexless_scan checks; hz_indexless_refix checks against this)
    uint64_t part_floor = 0;
};
