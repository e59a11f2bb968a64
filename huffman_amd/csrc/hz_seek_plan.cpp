// hz_seek_plan.cpp -- host arithmetic on a host seek table: which payload bytes a range decode reads
// (hz_seek_span) and the plan of a gathered buffer for a list of ranges (hz_seek_pieces). No device call
// and no HIP call: a unit that links alone, so a stand-alone host program can run it under a sanitizer
// (tests/pieces_probe.cpp).
#include <stdint.h>

#include <algorithm>
#include <new>
#include <vector>

#include "huffman_amd.h"
#include "hz_internal.h"

using namespace hz;

namespace {

uint64_t table_word(const void* seek, uint64_t i) { return static_cast<const uint64_t*>(seek)[i]; }

}  // namespace

int hz::seek_span_by(SeekWordFn word, const void* arg, uint64_t nsym, uint64_t sym_begin, uint64_t sym_count,
                     uint64_t* byte_begin, uint64_t* byte_end) {
    if (!byte_begin || !byte_end) return HZ_EINVAL;
    if (sym_begin > nsym || sym_count > nsym - sym_begin) return HZ_EINVAL;
    *byte_begin = *byte_end = 0;
    if (sym_count == 0) return HZ_OK;
    if (!arg) return HZ_EINVAL;
    const uint64_t b0 = sym_begin / kBlockSyms, b1 = (sym_begin + sym_count - 1) / kBlockSyms;
    const uint64_t w0 = word(arg, b0), w1 = word(arg, b1 + 1);
    const uint64_t first = w0 / 8, last = w1 / 8 + (w1 % 8 ? 1 : 0);
    if (last < first) return HZ_EINVAL;
    // the staging window of a block starts 16 bytes below the 16-byte chunk of its first bit
    // (dec_stage_prefetch / dec_stage_commit; the walk's reader starts at that chunk, br_init) and
    // ends with the chunk two words past its last bit; the reader runs one chunk ahead
    *byte_begin = first > kRangeLeadBytes ? (first - kRangeLeadBytes) & ~15ull : 0;
    *byte_end = last + kRangeTailBytes;
    return HZ_OK;
}

extern "C" int hz_seek_span(const uint64_t* seek, uint64_t nsym, uint64_t sym_begin, uint64_t sym_count,
                            uint64_t* byte_begin, uint64_t* byte_end) {
    return seek_span_by(table_word, seek, nsym, sym_begin, sym_count, byte_begin, byte_end);
}

namespace {

struct Span {
    uint64_t begin, end;  // payload bytes, clamped
    uint64_t b0, b1;      // first and last block
    uint32_t range;
};

int seek_pieces(SeekWordFn word, const void* arg, uint64_t nsym, uint64_t payload_bytes, const hz_range* ranges, uint32_t nranges,
                hz_piece* pieces, uint32_t* npieces, hz_piece_range* out, uint64_t* buf_bytes, uint64_t* seek_words) {
    std::vector<Span> spans;
    spans.reserve(nranges);
    for (uint32_t i = 0; i < nranges; ++i) {
        out[i].sym_begin = ranges[i].sym_begin;
        out[i].sym_count = ranges[i].sym_count;
        out[i].out_byte = ranges[i].out_byte;
        out[i].piece = 0;
        Span s;
        const int rc = seek_span_by(word, arg, nsym, ranges[i].sym_begin, ranges[i].sym_count, &s.begin, &s.end);
        if (rc) return rc;
        if (ranges[i].sym_count == 0) continue;
        if (s.begin >= payload_bytes) return HZ_EFORMAT;
        s.end = std::min(s.end, payload_bytes);
        s.b0 = ranges[i].sym_begin / kBlockSyms;
        s.b1 = (ranges[i].sym_begin + ranges[i].sym_count - 1) / kBlockSyms;
        s.range = i;
        spans.push_back(s);
    }
    std::sort(spans.begin(), spans.end(), [](const Span& a, const Span& b) {
        return a.begin != b.begin ? a.begin < b.begin : a.range < b.range;
    });
    uint32_t np = 0;
    uint64_t buf_end = 0, words = 0;
    for (size_t k = 0; k < spans.size(); ++k) {
        const Span& s = spans[k];
        if (np && s.begin <= pieces[np - 1].stream_byte + pieces[np - 1].bytes) {  // overlaps or touches: one piece
            hz_piece& p = pieces[np - 1];
            p.bytes = std::max(p.stream_byte + p.bytes, s.end) - p.stream_byte;
            const uint64_t last = std::max(p.first_block + p.nblocks - 1, s.b1);
            p.first_block = std::min(p.first_block, s.b0);
            p.nblocks = last - p.first_block + 1;
        } else {
            hz_piece& p = pieces[np++];
            p.stream_byte = s.begin;
            p.bytes = s.end - s.begin;
            p.first_block = s.b0;
            p.nblocks = s.b1 - s.b0 + 1;
            p.buf_byte = p.seek_index = 0;
        }
        out[s.range].piece = np - 1;
    }
    for (uint32_t k = 0; k < np; ++k) {  // places, once every piece has its final size
        hz_piece& p = pieces[k];
        p.buf_byte = ((buf_end + 63) & ~63ull) + (p.stream_byte & 63);
        buf_end = p.buf_byte + p.bytes;
        p.seek_index = words;
        words += p.nblocks + 1;
    }
    *npieces = np;
    *buf_bytes = (buf_end + 15) & ~15ull;
    *seek_words = words;
    return HZ_OK;
}

}  // namespace

int hz::seek_pieces_by(SeekWordFn word, const void* arg, uint64_t nsym, uint64_t payload_bytes, const hz_range* ranges,
                       uint32_t nranges, hz_piece* pieces, uint32_t* npieces, hz_piece_range* out, uint64_t* buf_bytes,
                       uint64_t* seek_words) {
    if (!npieces || !buf_bytes || !seek_words) return HZ_EINVAL;
    *npieces = 0;
    *buf_bytes = *seek_words = 0;
    if (nranges == 0) return HZ_OK;
    if (!ranges || !pieces || !out) return HZ_EINVAL;
    try {
        return seek_pieces(word, arg, nsym, payload_bytes, ranges, nranges, pieces, npieces, out, buf_bytes, seek_words);
    } catch (const std::bad_alloc&) {
        return HZ_ENOMEM;
    }
}

extern "C" int hz_seek_pieces(const uint64_t* seek, uint64_t nsym, uint64_t payload_bytes, const hz_range* ranges,
                              uint32_t nranges, hz_piece* pieces, uint32_t* npieces, hz_piece_range* out,
                              uint64_t* buf_bytes, uint64_t* seek_words) {
    return seek_pieces_by(table_word, seek, nsym, payload_bytes, ranges, nranges, pieces, npieces, out, buf_bytes,
                          seek_words);
}
