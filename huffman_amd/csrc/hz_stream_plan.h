// hz_stream_plan.h -- the arithmetic of the streaming `archive` / `extract` (hz_stream.cpp) and of a
// payload's bounds: integers and one double, no HIP call, no device memory, header only, so a stand-alone
// host program drives it round by round (tests/stream_probe.cpp). Private to the library.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace hz {

constexpr uint64_t kPlanBlockSyms = 2048;  // kBlockSyms (hz_internal.h, which needs HIP); hz_stream.cpp asserts it

// ---- what a payload can hold: every codeword is at least min_len bits ----
// pay_bytes: from the byte of the first payload bit to the end of the file; payload_bit: that bit's place in its byte.
inline uint64_t payload_most_syms(uint64_t pay_bytes, uint32_t payload_bit, uint32_t min_len) {
    const uint64_t pay_bits = pay_bytes * 8 > payload_bit ? pay_bytes * 8 - payload_bit : 0;
    return pay_bits / std::max<uint32_t>(min_len, 1);
}
// a header that claims more symbols than its payload can hold is malformed
inline bool payload_holds(uint64_t pay_bytes, uint32_t payload_bit, uint64_t nsym, uint32_t min_len) {
    return nsym <= payload_most_syms(pay_bytes, payload_bit, min_len);
}
// the most bytes the payload can decode to (the odd last byte travels in the header)
inline uint64_t payload_most_bytes(uint64_t pay_bytes, uint32_t payload_bit, uint32_t min_len, bool is_odd) {
    return 2 * payload_most_syms(pay_bytes, payload_bit, min_len) + (is_odd ? 1 : 0);
}

// ---- the extract's payload window ----
// The payload passes through a device window of W bytes. A round decodes the k codewords the window
// surely holds (round_syms: the file's mean code length with a 3 % margin); a round whose codes overran
// the window is redone at the max_len bound (redo_syms), exactly. advance() then drops the bytes the
// round consumed: the unconsumed tail moves to the front of the next window and the file refills the rest.
struct ExtractWindow {
    uint64_t W;        // window bytes
    uint64_t nsym;     // the file's symbols
    double mean;       // mean bits per symbol of this file
    uint64_t max_len;
    uint64_t sym_cap;  // output per round <= W bytes
    uint64_t have = 0;      // payload bytes in the window
    uint64_t bit;           // the round's first codeword: this bit of the window
    uint64_t done = 0;      // symbols decoded by the rounds before this one
    uint64_t consumed = 0;  // payload bytes before the window (the seek entries' bit base)
    uint64_t file_left;     // payload bytes not yet read
    bool whole_blocks;      // every round but the file's last is a positive multiple of kPlanBlockSyms

    // whole_blocks: each round's output then starts on a block of the seek table and of the block sums
    // (hz_seekable_attach_file, hz_extract_stream_verified), on the redo path too: sym_cap is whole blocks,
    // an estimate below one block becomes one block (it may overrun and be redone) and the redo bound is
    // rounded down to blocks. The window must hold a block at max_len (HZ_SEEKABLE_MIN_WINDOW).
    ExtractWindow(uint64_t window, uint64_t nsym_, uint64_t pay_total, uint32_t payload_bit, uint32_t cb_max_len,
                  bool whole_blocks_ = false)
        : W(window), nsym(nsym_), max_len(std::max<uint32_t>(cb_max_len, 1)),
          sym_cap(std::max<uint64_t>(W / 2, kPlanBlockSyms)), bit(payload_bit), file_left(pay_total),
          whole_blocks(whole_blocks_) {
        mean = pay_total ? ((double)pay_total * 8 - payload_bit) / (double)nsym : (double)max_len;
        if (whole_blocks) sym_cap = sym_cap / kPlanBlockSyms * kPlanBlockSyms;
    }
    // bytes of the first read: they fill the window from its front
    uint64_t first_fill() {
        const uint64_t r = std::min(W, file_left);
        have = r;
        file_left -= r;
        return r;
    }
    // symbols this round decodes from the window: what it surely holds
    uint64_t round_syms() const {
        const uint64_t left = nsym - done, avail = have * 8 - bit;
        if (file_left == 0) return std::min(left, sym_cap);
        uint64_t k = (uint64_t)((double)avail / (mean * 1.03));
        k = std::min(std::min(left, sym_cap), k);
        if (whole_blocks) return k < left ? std::min(left, whole(k)) : k;
        // whole blocks when the window holds at least one; a smaller window keeps k
        if (k < left && k >= kPlanBlockSyms) k = k / kPlanBlockSyms * kPlanBlockSyms;
        return std::max<uint64_t>(k, 1);
    }
    // the round's codes overran the window and the file has more: redo at the bound
    bool overran(uint64_t end_bit) const { return end_bit > have * 8 && file_left > 0; }
    uint64_t redo_syms() const {
        const uint64_t k = (have * 8 - bit) / max_len;
        // (the overrun round asked for no more than min(left, sym_cap), and the bound's codes surely fit)
        if (whole_blocks) return std::min(std::min(nsym - done, sym_cap), whole(k));
        return std::max<uint64_t>(k, 1);
    }
    // k rounded down to blocks, one block at the least
    static uint64_t whole(uint64_t k) { return std::max(k / kPlanBlockSyms * kPlanBlockSyms, kPlanBlockSyms); }
    // (after the redo) the codes end past all the file has: a truncated file
    bool truncated(uint64_t end_bit) const { return end_bit > have * 8; }

    struct Step {
        uint64_t used;  // whole bytes the round's codewords took from the window's front
        uint64_t tail;  // bytes behind them, moved to the front of the next window
        uint64_t r;     // bytes the file refills behind the tail (0 after the last round)
        bool more;      // another round follows
    };
    // The round decoded k codewords ending at end_bit. The window moves on only when a round follows.
    Step advance(uint64_t end_bit, uint64_t k) {
        Step s;
        s.used = end_bit / 8;
        s.tail = have - s.used;
        s.more = done + k < nsym;
        s.r = s.more ? std::min(W - s.tail, file_left) : 0;
        if (s.more) {
            have = s.tail + s.r;
            file_left -= s.r;
            consumed += s.used;
            bit = end_bit % 8;
        }
        done += k;
        return s;
    }
};

// ---- the archive's chunks ----
struct ArchiveChunks {
    uint64_t chunk_bytes;  // the caller's, rounded: even (whole symbols), 16-byte aligned device reads
    uint64_t chunk;        // bytes per read, upload and pack: no more than the file needs

    // whole_blocks: with a seek table every chunk but the last is whole blocks (hz_pack_seek)
    ArchiveChunks(uint64_t asked, bool whole_blocks, uint64_t n) {
        chunk_bytes = asked & ~(uint64_t)15;
        if (whole_blocks)
            chunk_bytes = std::max<uint64_t>(chunk_bytes / (2 * kPlanBlockSyms) * (2 * kPlanBlockSyms), 2 * kPlanBlockSyms);
        chunk = std::min<uint64_t>(chunk_bytes, std::max<uint64_t>(n, 16));
    }
    // bytes a packed chunk can take: a lead word and max_len bits per symbol, in whole words and one more
    uint64_t out_cap(uint32_t max_len) const {
        const uint64_t csym = chunk / 2;
        return ((32 + csym * (uint64_t)max_len + 31) / 32 + 1) * 4;
    }
    struct Carry {
        uint64_t bytes;   // payload bytes this chunk hands to the file
        uint32_t sbit;    // bit of the next chunk's first code in its first word
        bool needs_lead;  // the partial word, carried into the next chunk as its lead bits
    };
    // end_bit: where the chunk's codes end, counted from its first output word
    static Carry carry_after(uint64_t end_bit, bool last) {
        Carry c;
        c.bytes = last ? (end_bit + 7) / 8 : end_bit / 32 * 4;  // complete words until the end
        c.sbit = (uint32_t)(end_bit % 32);
        c.needs_lead = c.sbit && !last;
        return c;
    }
};

}  // namespace hz
