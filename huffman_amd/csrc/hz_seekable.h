// hz_seekable.h -- the trailer of a seekable file (include/huffman_amd.h "seekable files") as the flows
// that meet one use it: where a file's .compressed image ends, and positional reads of trailer words.
// hz_seekable.cpp makes no HIP call and links with hz_file_io.cpp alone (tests/seekable_probe.cpp).
// Private to the library.
#pragma once
#include <stdint.h>

#include "huffman_amd.h"

namespace hz {

constexpr uint64_t kSeekableBlockSyms = 2048;  // kBlockSyms (hz_internal.h, which needs HIP)

// RFC 1950 Adler-32 of p[0..n), continued from `adler` (1 to begin).
uint32_t adler32(uint32_t adler, const uint8_t* p, uint64_t n);

// hz_seek_bytes (hz_host.cpp) for this unit: 8 * (nblocks + 1), 0 for nsym 0. Never wraps.
inline uint64_t seekable_blocks(uint64_t nsym) { return nsym / kSeekableBlockSyms + (nsym % kSeekableBlockSyms ? 1 : 0); }
inline uint64_t seekable_seek_bytes(uint64_t nsym) { return nsym ? 8 * (seekable_blocks(nsym) + 1) : 0; }

// Where the trailer's sections stand behind an image of image_bytes of an n-byte original: the one place
// that knows the layout (include/huffman_amd.h "seekable files"). ok = false: a size that does not fit 64
// bits. sums_off is 0 without HZ_SEEKABLE_SUMS (the sums would begin at seek_off + seek_bytes).
struct SeekableLayout {
    bool ok = false;
    uint64_t seek_off = 0, seek_bytes = 0, sums_off = 0, sums_bytes = 0, file_bytes = 0;
};
SeekableLayout seekable_layout(uint64_t image_bytes, uint64_t n, uint32_t flags);

// The 64-byte footer of the trailer behind an image of image_bytes of an n-byte original. HZ_EINVAL: unknown
// flags, or sizes that do not fit 64 bits.
int seekable_footer(uint64_t image_bytes, uint64_t n, uint32_t flags, uint8_t out[HZ_SEEKABLE_FOOTER_BYTES]);

// Where the .compressed image of a file in memory ends: len for a plain file, image_bytes for a file
// with a trailer (*info, nullable, receives the parse). HZ_EFORMAT for a trailer whose fields do not fit.
int image_end(const uint8_t* file, uint64_t len, uint64_t* image_bytes, hz_seekable_info* info);
// The same for an open file: reads its last 64 bytes (nothing of a file shorter than that).
int image_end_fd(int fd, uint64_t file_bytes, uint64_t* image_bytes, hz_seekable_info* info);

}  // namespace hz
