// hz_salvage_plan.h -- the windows of hz_seekable_salvage_file (hz_stream.cpp): a file's blocks cut into
// runs whose payload bytes fit a bounded buffer, from a seek table THAT MAY ITSELF BE DAMAGED. Integers only,
// no HIP call, no device memory, header only, so a stand-alone host program drives it over arbitrary tables
// under the sanitizers (tests/salvage_probe.cpp). Private to the library.
//
// Trust is per BLOCK, not per entry. Block b is trusted when its own two entries could be a block's:
// seek[b] <= seek[b + 1], at most 2048 * max_len bits apart, and seek[b + 1] inside the payload. That is the
// check the decoder makes before it reads anything of a block (seek_block_err, hz_range_device.h), so a
// block that is not trusted is flagged there whatever bytes it is given, and no span has to cover it. A
// window's span is the hull of hz_seek_span of its trusted blocks (empty, 0 .. 0, when it has none).
// What follows, whatever the entries hold:
//   - a block whose own two entries are undamaged is trusted (a valid file's entries are a block's), so its
//     hz_seek_span lies inside its window's span. Judging an entry by its neighbours cannot promise that:
//     three neighbouring entries moved by one amount agree with each other, and a span anchored on the
//     middle one starts behind an undamaged block further on.
//   - with an undamaged table the spans ascend, and the hull is hz_seek_span of the window's symbols.
//   - every entry is compared with the payload's bits before anything is computed from it, so a byte
//     position is at most payload_bytes + HZ_RANGE_TAIL_BYTES and nothing wraps.
// Windows are cut greedily: a block joins the window while the hull stays within chunk_bytes and the
// window's output within chunk_bytes too (4096 bytes a block, one block at the least). Damaged entries that
// happen to look like a block far away (0 and 1, say) stretch a hull; the cut then falls before them, so
// damage costs small windows, never a large buffer. A window of one block exceeds chunk_bytes only when that
// block's own span does, which HZ_SEEKABLE_MIN_WINDOW rules out (a block is at most 2048 * 56 bits).
#pragma once
#include <stdint.h>

#include <algorithm>

#include "huffman_amd.h"

namespace hz {

constexpr uint64_t kSalvageBlockSyms = 2048;  // kBlockSyms (hz_internal.h, which needs HIP); hz_stream.cpp asserts it

struct SalvageWindow {
    uint64_t first_block, nblocks;
    uint64_t byte_begin, byte_end;  // payload bytes, hz_seek_span's: byte_end is not clamped to the payload
};

struct SalvagePlan {
    const uint64_t* seek;     // host, nblocks + 1 entries
    uint64_t nblocks;
    uint64_t limit_bits;      // the payload's bits
    uint64_t max_block_bits;  // 2048 * max_len
    uint64_t chunk_bytes;
    uint64_t max_blocks;      // output blocks a window may hold
    uint64_t at = 0;          // the next window's first block

    SalvagePlan(const uint64_t* seek_, uint64_t nblocks_, uint64_t payload_bytes, uint32_t max_len, uint64_t chunk_bytes_)
        : seek(seek_), nblocks(nblocks_), limit_bits(payload_bytes > UINT64_MAX / 8 ? UINT64_MAX : 8 * payload_bytes),
          max_block_bits(kSalvageBlockSyms * std::max<uint32_t>(max_len, 1)), chunk_bytes(chunk_bytes_),
          max_blocks(std::max<uint64_t>(chunk_bytes_ / (2 * kSalvageBlockSyms), 1)) {}

    bool trusted(uint64_t b) const {
        const uint64_t s0 = seek[b], s1 = seek[b + 1];
        return s0 <= s1 && s1 <= limit_bits && s1 - s0 <= max_block_bits;
    }
    // hz_seek_span of a trusted block (hz_seek_plan.cpp)
    void block_span(uint64_t b, uint64_t* begin, uint64_t* end) const {
        const uint64_t s0 = seek[b], s1 = seek[b + 1];
        const uint64_t first = s0 / 8, last = s1 / 8 + (s1 % 8 ? 1 : 0);
        *begin = first > HZ_RANGE_LEAD_BYTES ? (first - HZ_RANGE_LEAD_BYTES) & ~(uint64_t)15 : 0;
        *end = last + HZ_RANGE_TAIL_BYTES;
    }
    // The next window; false after the last.
    bool next(SalvageWindow* w) {
        if (at >= nblocks) return false;
        w->first_block = at;
        w->nblocks = 0;
        uint64_t begin = UINT64_MAX, end = 0;  // begin > end: no trusted block yet
        while (at < nblocks && w->nblocks < max_blocks) {
            uint64_t nb = begin, ne = end;
            if (trusted(at)) {
                uint64_t b0, b1;
                block_span(at, &b0, &b1);
                nb = std::min(nb, b0);
                ne = std::max(ne, b1);
            }
            if (w->nblocks && nb < ne && ne - nb > chunk_bytes) break;
            begin = nb;
            end = ne;
            ++w->nblocks;
            ++at;
        }
        w->byte_begin = begin < end ? begin : 0;
        w->byte_end = begin < end ? end : 0;
        return true;
    }
};

}  // namespace hz
