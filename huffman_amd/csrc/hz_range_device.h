// hz_range_device.h -- what the two random-access units share (hz_decode.hip: hz_decode_range and
// hz_index_expand; hz_ranges.hip: hz_decode_ranges, hz_decode_ranges_pieces): the moved payload view, the seek pass's arguments,
// the per-block checks and the FIXED16 step. Plain structs, force-inlined device
// functions and one host helper; no kernel (DESIGN.md "Source layout": a new caller of shared
// force-inlined code gets a unit of its own).
#pragma once
#include "hz_decode_device.h"

namespace hz {

// The random access view of the block decoders (DESIGN.md "Random access").
struct RangeDecArgs : DecArgs {
    uint64_t w_first;    // first word of the view that exists (words below it are only addressed, never read)
    const uint8_t* bad;  // per tile block: nonzero = failed a check, nothing is stored for it
    uint64_t blk0;       // the tile's first block in the stream (a.starts / a.subs / a.nblocks are the tile's)
    uint64_t lo, hi;     // stream symbols [lo, hi) go to out + 2 (sym - lo); nothing else is written
};

struct SeekArgs {
    const unsigned long long* seek;  // the stream's start[]: block b at seek[b]
    const unsigned long long* isub;  // a full index's sub rows (chain 0 is checked against start[b]); else null
    unsigned long long* tstart;      // the tile's index in scratch: start[nb + 1] clamped into the view; null: none
    unsigned long long* rows;        // sub rows out, 64 words per block of the tile
    unsigned long long* maxp;        // the tile's largest block in bits (atomicMax; zeroed by the launcher)
    uint8_t* bad;                    // per block of the tile; null: none
    uint64_t blk0, nb, nsym;
    uint64_t clamp_lo, bit_hi;       // stream bits a block may start at / end at inside the view
};

// The checks of one block before anything of it is read: start[b] <= start[b + 1] and at most
// cnt * max_len bits apart (else format, bit 1), the staging window inside the view (else invalid
// argument, bit 16), a full index's first sub[] entry against start[b] (format).
HZ_DEV uint32_t seek_block_err(const DecArgs& a, const SeekArgs& y, uint64_t b, uint64_t s0, uint64_t s1, uint32_t cnt) {
    uint32_t err = 0;
    if (s1 < s0 || s1 - s0 > (uint64_t)cnt * (uint32_t)a.max_len) err = 1u;
    else if (s0 < y.clamp_lo || s1 > y.bit_hi) err = 16u;
    else if (y.isub && (uint32_t)(y.isub[b * kWave] & 0xffffu) != (uint32_t)(s0 & 0xffffu)) err = 1u;
    return err;
}

// The FIXED16 step: five byte-swapped stream words whose bit pos % 32 is a code's first bit -> the
// eight symbols of the next 128 bits as four output words.
HZ_DEV void fixed16_step(const uint16_t* t16, const uint32_t (&ww)[5], uint32_t pos, uint32_t (&o)[4]) {
    const uint32_t sh = pos & 31;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const uint32_t cw = sh ? __builtin_amdgcn_alignbit(ww[t], ww[t + 1], 32u - sh) : ww[t];
        o[t] = (uint32_t)t16[cw >> 16] | ((uint32_t)t16[cw & 0xffffu] << 16);
    }
}

// The arithmetic of a moved view: stream bytes [base, base + bytes) stand at device address addr. Stream
// bit p is bit p + bit_adj of the words at words_addr (64-byte aligned), whose word 0 lies below addr
// when base > 0. Host and device: the slice forms fix it at the call, the gathered form per job.
struct RangeView {
    uint64_t words_addr;
    uint64_t w0;       // word of the 64-byte line that holds addr
    uint64_t head;     // addr's byte in that line
    uint64_t nwords;   // one past the word of the last byte
    uint64_t clamp_lo, bit_hi;
    uint32_t bit_adj;
};
__host__ __device__ __forceinline__ RangeView range_view(uint64_t addr, uint64_t bytes, uint64_t base) {
    RangeView v;
    const uint64_t head = addr & 63, r = base & 63;
    uint64_t shift = base >> 6;  // 64-byte units the view's word 0 moves down
    uint64_t adj = head - r;
    if (head < r) { adj = head + 64 - r; shift += 1; }
    v.words_addr = (addr & ~(uint64_t)63) - 64 * shift;
    v.bit_adj = (uint32_t)(8 * adj);
    v.head = head;
    v.w0 = 16 * shift;
    v.nwords = v.w0 + (bytes + head + 3) / 4;
    // a block's staging window starts 16 bytes below the 16-byte chunk of its first bit: inside the slice
    // unless the slice starts the stream (base 0: words below the payload read as zeros, as in hz_decode)
    const uint64_t vlo = 8 * base + v.bit_adj;
    v.clamp_lo = base ? 128 * ((vlo + 127) / 128 + 1) - v.bit_adj : 0;
    v.bit_hi = 8 * (base + bytes);
    if (v.clamp_lo > v.bit_hi) v.clamp_lo = v.bit_hi;  // a slice too small for any block: every block fails
    return v;
}

// The view of a payload slice that holds stream bytes [base, base + payload_bytes).
inline void fill_range_view(RangeDecArgs& a, SeekArgs& y, const Tables& t, const uint8_t* d_payload,
                            uint64_t payload_bytes, uint64_t base, uint64_t nsym) {
    fill_dec_args(a, t, d_payload, payload_bytes, nsym);
    const RangeView v = range_view((uint64_t)(uintptr_t)d_payload, payload_bytes, base);
    a.words = reinterpret_cast<const uint32_t*>((uintptr_t)v.words_addr);
    a.bit_adj = v.bit_adj;
    a.w_first = v.w0;
    a.nwords = v.nwords;
    a.start0 = 0;
    y.clamp_lo = v.clamp_lo;
    y.bit_hi = v.bit_hi;
    y.nsym = nsym;
}

}  // namespace hz
