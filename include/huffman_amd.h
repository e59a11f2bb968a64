/*
 * huffman_amd.h -- C ABI of the MI355X-native Huffman codec (gfx950 / CDNA4).
 *
 * Drop-in boundary for the reference yechuan51/huffman path: the `archive` /
 * `extract` executables and their on-disk `.compressed` format. The reference
 * has no library API; every entry point below replaces one
 * stage of Compressor.cu / Decompressor.cu, cited per function.
 *
 * Conventions
 *   - Plain pointers and sizes only. `d_*` arguments are device pointers
 *     (hipMalloc / torch CUDA tensors) and are used stream-ordered on the
 *     context's stream; host arguments are plain host memory.
 *   - The caller owns every buffer. A context owns only its scratch, its
 *     device code tables and (optionally) its stream.
 *   - Errors: negative HZ_E* status, never abort(). hz_strerror() names them.
 *   - Threading: one context per device per host thread.
 *   - Symbols are 16-bit little-endian byte pairs (Compressor.cu:45); an odd
 *     trailing byte is carried raw in the header (Compressor.cu:339-351).
 */
#ifndef HUFFMAN_AMD_H
#define HUFFMAN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HZ_NSYM 65536  /* alphabet: every u16 value (Compressor.cu:323 kMaxSymbolSize) */
#define HZ_MAXLEN 56   /* longest supported code (needs > ~5e11 symbols to exceed) */

enum {
    HZ_OK = 0,
    HZ_EINVAL = -1,    /* bad argument / alignment */
    HZ_ENOMEM = -2,    /* host or device allocation failed */
    HZ_EHIP = -3,      /* HIP runtime error */
    HZ_ETOOLONG = -4,  /* a code longer than HZ_MAXLEN bits */
    HZ_EFORMAT = -5,   /* malformed or truncated .compressed stream */
    HZ_ECAP = -6,      /* output capacity too small */
    HZ_ETIMEOUT = -7,  /* a device-side wait exceeded its bound (reserved) */
    HZ_EIO = -8,       /* file I/O error */
    HZ_ENODEV = -9,    /* no usable gfx950 device */
    HZ_ENOENT = -10,   /* input file does not exist (the reference CLIs exit 0 on it) */
    HZ_ECHECKSUM = -11 /* a decoded block does not match its stored checksum (seekable files) */
};

/* Codebook in the reference's order and bit conventions. */
typedef struct hz_codebook {
    uint32_t nsym;              /* U, number of symbols with nonzero count */
    uint32_t max_len;           /* longest code */
    uint32_t min_len;           /* shortest code */
    uint32_t reserved;
    uint16_t order[HZ_NSYM];    /* header order: (count asc, symbol asc) */
    uint8_t len[HZ_NSYM];       /* code length per symbol value (0 = absent) */
    uint64_t code[HZ_NSYM];     /* code per symbol, right aligned; first bit = MSB */
} hz_codebook;

/* Parsed .compressed header (Decompressor.cu:65-103). */
typedef struct hz_header_info {
    uint64_t n;                 /* original size in bytes */
    uint64_t payload_byte;      /* file byte holding the first payload bit */
    uint32_t payload_bit;       /* bit (MSB = 0) of that byte where the payload starts */
    uint32_t is_odd;
    uint32_t last_byte;
    uint32_t nsym;
} hz_header_info;

typedef struct hz_ctx hz_ctx;

/* Stream positions. Bit positions, seek entries and bases are u64 and may lie
 * anywhere in a stream of any size: a base lets a small device buffer stand for
 * a piece of a much larger stream. UINT64_MAX marks a position that does not
 * exist (a codeword the payload does not hold), and the kernels add alignment
 * offsets and margins of less than 2^16 bits to a position, so every position a
 * call can reach stays below HZ_POS_LIMIT. A base-taking call whose largest
 * position is HZ_POS_LIMIT or more, or does not fit 64 bits at all, returns
 * HZ_EINVAL at the call with nothing launched:
 *   hz_decode_range, hz_decode_ranges   8 * (payload_byte_base + payload_bytes)
 *   hz_decode_ranges_pieces             8 * buf_bytes (a piece's 8 * (stream_byte +
 *                                       bytes): found on the device, that range refused)
 *   hz_pack_seek                        bit_base + 8 * out_cap
 *   hz_decode_indexless_seek            bit_base + 8 * payload_bytes
 *   hz_indexless_scan                   payload_bit_base + 8 * payload_bytes */
#define HZ_POS_LIMIT (UINT64_MAX - 0xFFFFu)

const char *hz_strerror(int status);
int hz_version(void);

/* Context: device + stream (stream may be NULL: the context creates its own). */
int hz_ctx_create(int device, void *stream, hz_ctx **out);
int hz_ctx_destroy(hz_ctx *ctx);
int hz_ctx_set_stream(hz_ctx *ctx, void *stream);
int hz_ctx_sync(hz_ctx *ctx);

/* ---- encode stages ----------------------------------------------------- */

/* 65 536-bin histogram of the u16 symbols of d_in[0..n) into d_hist (u64 x
 * 65536); accumulate != 0 adds to d_hist instead of overwriting.
 * Stream-ordered, no host synchronisation and no scratch: a HIP graph can capture
 * it and replay it on whatever d_in holds then.
 * Replaces calculateFrequency (Compressor.cu:38-48, launch :369-372). */
int hz_hist16(hz_ctx *ctx, const uint8_t *d_in, uint64_t n, uint64_t *d_hist, int accumulate);

/* Block checksums of data on the device: word i of d_sums (hz_block_sums_bytes(n) = 4 * ceil(n / 4096)
 * bytes) is the Adler-32 (RFC 1950, zlib's adler32) of bytes [4096 i, min(4096 (i + 1), n)) of d_in
 * EXTENDED WITH ZERO BYTES TO 4096, so every sum is over exactly 4096 bytes and the last block is no
 * special case: with d_k the block's bytes (0 past n), a = (1 + sum d_k) mod 65521, b = (4096 +
 * sum (4096 - k) d_k) mod 65521, word = b << 16 | a. A block is one seek-table block of output
 * (2 * hz_index_stride() bytes). One read pass: a wave per block, 1 KiB per wave-load.
 * d_in must be 16-byte aligned (HZ_EINVAL otherwise; d_sums 4-byte aligned). Stream-ordered, no
 * scratch and no host wait: a HIP graph can capture it and replay it on whatever d_in holds then.
 * n == 0: HZ_OK, nothing launched. No load leaves [d_in, d_in + n) rounded up to a 4-byte word, and
 * bytes of that word at or past n are masked, never summed. The reference has no counterpart (its
 * format carries no checksum). */
#define HZ_SUM_BLOCK_BYTES 4096
uint64_t hz_block_sums_bytes(uint64_t n);
int hz_block_sums(hz_ctx *ctx, const uint8_t *d_in, uint64_t n, uint32_t *d_sums);

/* The same pass with nothing stored: block i's word is compared with d_expect[i] (4 * ceil(n / 4096)
 * bytes, 4-byte aligned), and only a block that differs does a 64-bit atomic minimum of block_base + i
 * into *d_bad (8-byte aligned). *d_bad is the caller's: the call never initialises it, so several
 * calls (the rounds of hz_extract_stream_verified, each at its block_base) fold into one word; write
 * UINT64_MAX first, and the word is then the smallest failing block or still UINT64_MAX. Alignment of
 * d_in, bounds, grid shape, stream order and capturability are hz_block_sums' (the same loads and the
 * same arithmetic: one per-block body in hz_sums.hip). No scratch, and the context's error word is
 * not touched. n == 0: HZ_OK, nothing launched. HZ_EINVAL: a null pointer, d_in not 16-byte aligned,
 * d_expect not 4-byte aligned, d_bad not 8-byte aligned. */
int hz_block_sums_check(hz_ctx *ctx, const uint8_t *d_in, uint64_t n, const uint32_t *d_expect,
                        uint64_t block_base, uint64_t *d_bad);

/* The comparison with EVERY verdict kept, and the damaged blocks blanked on request: block i's word is
 * compared with d_expect[i] as above, and a block that differs does a 32-bit atomic OR of bit
 * (block_base + i) & 31 into d_bits[(block_base + i) >> 5] (4-byte aligned; the caller sizes it for the
 * largest block_base + i it will pass). The bitmap is the caller's: the call never initialises it, so
 * several calls (the windows of hz_seekable_salvage_file, each at its block_base) fold into one bitmap;
 * zero it first, and afterwards its set bits are exactly the failing blocks. With flags =
 * HZ_SUMS_ZERO_BAD a block that differs also has its bytes [4096 i, min(4096 (i + 1), n)) of d_data
 * overwritten with zeros by the wave that summed it (a wave-uniform branch): 16-byte stores wherever the
 * whole vector lies below n, and the vector that holds byte n - 1 as whole words and then single bytes,
 * so no store touches a byte at or past n. A block that matches is never written, and without the flag
 * nothing of d_data is. Loads, alignment of d_data, grid shape, stream order and capturability are
 * hz_block_sums' (one per-block body in hz_sums.hip). No scratch, and the context's error word is not
 * touched. n == 0: HZ_OK, nothing launched. HZ_EINVAL: a null pointer, d_data not 16-byte aligned,
 * d_expect or d_bits not 4-byte aligned, a flag other than HZ_SUMS_ZERO_BAD. */
#define HZ_SUMS_ZERO_BAD 1u
int hz_block_sums_mark(hz_ctx *ctx, uint8_t *d_data, uint64_t n, const uint32_t *d_expect,
                       uint64_t block_base, uint32_t *d_bits, uint32_t flags);

/* Host codebook from a host histogram with the reference's semantics: thrust
 * stable sort (Compressor.cu:378-393,414,419-425) + GenerateCL / GenerateCW /
 * toCpu (gpuHuffmanConstruction.h:353-494,551-579). U == 1 gets code "0"
 * (reference defect B4). */
int hz_codebook_build(const uint64_t *hist, hz_codebook *cb);

/* The same codebook built on the device: d_hist (u64 x 65536,
 * device) -> d_cb (a device buffer of sizeof(hz_codebook), the same layout),
 * stream-ordered on the context's stream, one workgroup, GenerateCL's rounds
 * (gpuHuffmanConstruction.h:353-494) without a grid barrier. Errors surface at
 * hz_ctx_sync: HZ_EINVAL (a count >= 2^47), HZ_ETOOLONG (a code > HZ_MAXLEN).
 * This call, hz_header_write_device and hz_header_parse_device share one workspace
 * of the context, allocated by the first of them (the one host wait). No result
 * depends on what an earlier call left there (tests/test_gpu_second_use.py: U =
 * 65 536, then 3, then 1 without a synchronisation), so the calls may follow one
 * another in stream order, and after that first call a HIP graph can capture them
 * and replay them on whatever d_hist, d_cb and d_file hold then. */
int hz_codebook_build_device(hz_ctx *ctx, const uint64_t *d_hist, hz_codebook *d_cb);

/* Header bit length for a codebook and input size: 8*(3 + odd) + sum(24 + L) + 64.
 * The payload starts at that bit (Compressor.cu:431-487). */
int hz_header_bits(const hz_codebook *cb, uint64_t n, uint64_t *bits);

/* Payload bits: sum over symbols of hist[s] * len[s]. */
int hz_payload_bits(const hz_codebook *cb, const uint64_t *hist, uint64_t *bits);

/* Write the header (Compressor.cu:431-487; writers :637-669). Writes
 * floor(header_bits/8) complete bytes to out; the remaining header_bits%8
 * bits are returned MSB-aligned in *pending (they begin the payload's first
 * byte, Compressor.cu:541). */
int hz_header_write(const hz_codebook *cb, uint64_t n, uint8_t last_byte, uint8_t *out,
                     uint64_t cap, uint64_t *bytes, uint32_t *pending_bits, uint8_t *pending);

/* The header written on the device from a device codebook
 * (hz_codebook_build_device): d_out (4-byte aligned, cap bytes) receives the
 * header bit stream -- floor(bits/8) complete bytes, then the pending bits
 * MSB-aligned in the next byte, zeros after. d_info (device, 4 x u64):
 * complete bytes, pending bit count, pending byte, header bits. */
int hz_header_write_device(hz_ctx *ctx, const hz_codebook *d_cb, uint64_t n, uint8_t last_byte, uint8_t *d_out,
                           uint64_t cap, uint64_t *d_info);

/* Parse a header from the first `len` bytes of a .compressed file.
 * Replaces Decompressor.cu:65-103 (U 0 => 65536 :69-71; L 0 => 65536 :94-95). */
int hz_header_parse(const uint8_t *file, uint64_t len, hz_codebook *cb, hz_header_info *info);

/* The same parse on the device: d_file (device) -> d_cb
 * (device hz_codebook) and d_info (device, 6 x u64: n, payload byte, payload
 * bit, is_odd, last byte, nsym). Malformed headers surface as HZ_EFORMAT at
 * hz_ctx_sync. */
int hz_header_parse_device(hz_ctx *ctx, const uint8_t *d_file, uint64_t len, hz_codebook *d_cb, uint64_t *d_info);

/* Upload a codebook's device tables to the context: encode tables (needed by
 * hz_pack), decode tables (needed by hz_decode / hz_index_build /
 * hz_decode_indexless / hz_indexless_*), or both. Asynchronous on the context
 * stream: the tables are built on the host (the decode half while a hz_pack
 * launched before it runs), staged in pinned memory and copied by one device
 * kernel per table set. The index-less decoder's tables (walk length and escape
 * tables, a DENSE codebook's chain LUT) are copied by the first call that reads
 * them (hz_decode_indexless, hz_decode_indexless_seek / hz_seek_build,
 * hz_indexless_scan, hz_index_build), in its stream
 * order, so a decode through a block index never copies them; under stream
 * capture that copy is part of the captured work. */
int hz_codebook_upload(hz_ctx *ctx, const hz_codebook *cb);
int hz_codebook_upload_encode(hz_ctx *ctx, const hz_codebook *cb);
int hz_codebook_upload_decode(hz_ctx *ctx, const hz_codebook *cb);

/* Block index written by hz_pack / hz_index_build and read by hz_decode
 * (hz_index_bytes(nsym) bytes, 8-byte aligned): u64 start[nblocks + 1] -- the
 * absolute start bit of every hz_index_stride() = 2048-symbol block, then the
 * stream's end bit -- then u64 max_bits, the largest block in bits (sizes the
 * decoder's LDS slots), then u16 sub[nblocks][256]: the low 16 bits of the
 * absolute start bit of every 8-symbol chain of the block (its offset from
 * start[b] is (sub - start[b]) mod 2^16). The reference
 * has no index (its decoder is serial,
 * Decompressor.cu:259-291); this is the side band that makes decode parallel.
 *
 * Bits are counted from byte 0 of the d_payload pointer the index is used
 * with. A caller that hands hz_decode a pointer D bytes before (after) the one
 * the index was built for must rebase BOTH arrays together: add (subtract)
 * 8*D to every start[] entry and 8*D mod 2^16 to every sub[] entry; max_bits
 * is unchanged. Rebasing start[] alone decodes wrong data.
 *
 * hz_index_format() identifies this layout. Format 2 (this build) stores
 * sub[] as absolute low bits; format 1 (builds before it) stored offsets
 * from start[b]. An index kept across builds must be rebuilt (hz_index_build)
 * when the formats differ. */
#define HZ_INDEX_FORMAT 2
int hz_index_format(void);
uint64_t hz_index_stride(void);
uint64_t hz_index_bytes(uint64_t nsym);
uint64_t hz_scratch_bytes(uint64_t nsym);

/* Pack the n/2 symbols of d_in (16-byte aligned: HZ_EINVAL otherwise) with the
 * uploaded codebook into d_out as one MSB-first bit stream beginning at bit
 * `start_bit` of d_out (d_out 4-byte aligned; bits of d_out's first word before start_bit are taken from `lead`,
 * right aligned, i.e. the header's pending bits). Bits after the stream's end
 * up to the next 32-bit word are zero. d_index (optional, hz_index_bytes())
 * receives the block index. Stream-ordered and capturable by a HIP graph (it
 * replays on whatever d_in holds then); the host waits only when the context's
 * scratch must grow. Replaces
 * populateCWLength + transform_inclusive_scan + encodeFromCW
 * (Compressor.cu:50-61,541-576,182-313) and writeFileContent (:673-684,597-601). */
int hz_pack(hz_ctx *ctx, const uint8_t *d_in, uint64_t n, uint64_t start_bit, uint32_t lead,
            uint8_t *d_out, uint64_t out_cap, uint64_t *d_index);

/* ---- two-pass encode: the range plan ------------------------------------
 * The reference reads its input three times on the device: the histogram
 * (Compressor.cu:369-372), populateCWLength + the length scan (:543-553) and
 * encodeFromCW (:573-576). hz_hist16 + hz_pack do the same (count pass, scan,
 * write). The range plan removes the middle pass: hz_hist16_ranges computes the
 * same histogram and also leaves, in d_ranges (hz_ranges_bytes(n) bytes,
 * 16-byte aligned, caller-owned), the cumulative histogram of the input at the
 * end of every range of whole blocks (about 2048 ranges); hz_pack_ranges turns
 * them into every range's start bit with the codebook (a dot product with the
 * code lengths and a scan, no input read) and packs each range in one pass.
 * The output equals hz_pack's byte for byte.
 *   - hz_ranges_bytes(n) is 0 for inputs too small for a plan (< 256 MiB);
 *     both calls then behave as hz_hist16 / hz_pack and ignore d_ranges.
 *   - d_in must be 16-byte aligned and must not change between the two calls
 *     (stream order); d_ranges is overwritten by the next hz_hist16_ranges.
 *   - hz_pack_ranges falls back to count + scan + write (same output) when the
 *     codebook's packing waves cannot take the ranges evenly;
 *     hz_last_pack_ranges(ctx) says which path the last hz_pack_ranges took. */
uint64_t hz_ranges_bytes(uint64_t n);
int hz_hist16_ranges(hz_ctx *ctx, const uint8_t *d_in, uint64_t n, uint64_t *d_hist, int accumulate,
                     void *d_ranges);
int hz_pack_ranges(hz_ctx *ctx, const uint8_t *d_in, uint64_t n, uint64_t start_bit, uint32_t lead,
                   uint8_t *d_out, uint64_t out_cap, uint64_t *d_index, void *d_ranges);
int hz_last_pack_ranges(hz_ctx *ctx);

/* Decode nsym symbols from d_payload (bit stream as hz_pack writes it) into
 * d_out (2*nsym bytes, 16-byte aligned). d_index: the block index (from
 * hz_pack, or hz_index_build for an index-less stream). d_payload
 * must stay readable up to the next 4-byte boundary after payload_bytes.
 * Stream-ordered, no host synchronisation and no scratch: a HIP graph can capture
 * it and replay it on whatever d_payload and d_index hold then.
 * Replaces translateFile (Decompressor.cu:259-291). */
int hz_decode(hz_ctx *ctx, const uint8_t *d_payload, uint64_t payload_bytes, uint64_t nsym,
              const uint64_t *d_index, uint8_t *d_out);
/* Diagnostic: 16-byte staging chunks per lane the last hz_decode prefetched for
 * every block (3 where the payload's mean block fits 3 KiB, else 4), 0 when its
 * decoder has no such choice. The decoded bytes do not depend on it. */
int hz_last_decode_chunks(hz_ctx *ctx);

/* Build the block index of an index-less stream (a .compressed file from
 * the reference encoder) on the device. If the payload holds fewer than nsym
 * codewords, start[nblocks] (the end bit) is left at UINT64_MAX.
 * NOT capturable: the host waits for the stream after every fix-up round (it
 * reads whether a round changed anything). Under stream capture use
 * hz_seek_build and hz_index_expand, which are stream-ordered. */
int hz_index_build(hz_ctx *ctx, const uint8_t *d_payload, uint64_t payload_bytes, uint64_t start_bit,
                   uint64_t nsym, uint64_t *d_index);

/* ---- random access: seek table and range decode ---------------------------
 * A stream's SEEK TABLE is u64 start[nblocks + 1], the first nblocks + 1 words
 * of its block index (so a block-index pointer is a valid seek-table pointer):
 * the start bit of every 2048-symbol (4 KiB of output) block, then the
 * stream's end bit; 8 bytes per 4 KiB of output. Bits count from byte 0 of the
 * stream's payload buffer, as in the index. To keep one: hz_pack (or
 * hz_index_build) into an index buffer, copy its first hz_seek_bytes(nsym)
 * bytes to the host and store them beside the stream, or in it: a seekable file
 * carries its table in a trailer (below, "seekable files"). To read symbols back:
 * load the table, ask hz_seek_span which payload bytes the range needs, put
 * those bytes (or the whole payload) and the table on the device, upload the
 * codebook (hz_codebook_upload_decode) and call hz_decode_range. */
#define HZ_RANGE_LEAD_BYTES 32  /* payload bytes kept before the first block's start byte */
#define HZ_RANGE_TAIL_BYTES 32  /* payload bytes kept after the last block's end byte */
#define HZ_RANGE_FULL_INDEX 1u  /* hz_decode_range flag: d_seek is a complete block index */

uint64_t hz_seek_bytes(uint64_t nsym);            /* 8 * (nblocks + 1); 0 for nsym 0 */

/* Host arithmetic on a HOST seek table: the payload bytes [*byte_begin, *byte_end)
 * a range decode of symbols [sym_begin, sym_begin + sym_count) reads, margins
 * included (HZ_RANGE_LEAD_BYTES before the first block's start byte, or the
 * stream's byte 0; HZ_RANGE_TAIL_BYTES after the last block's end byte, which the
 * caller clamps to the payload it has). byte_begin is a multiple of 16. Only
 * seek[b0 .. b1 + 1] of the range's blocks are read. sym_count 0 gives an empty
 * span (0, 0); sym_begin + sym_count > nsym or a descending table HZ_EINVAL. */
int hz_seek_span(const uint64_t *seek, uint64_t nsym, uint64_t sym_begin, uint64_t sym_count,
                 uint64_t *byte_begin, uint64_t *byte_end);

/* Decode symbols [sym_begin, sym_begin + sym_count) of a stream into d_out
 * (2 * sym_count bytes, 2-byte aligned). Nothing outside those bytes is written.
 * d_seek: the stream's seek table on the device (entries b0 .. b1 + 1 of the
 * range's blocks are read, addressed from d_seek[0]). d_payload holds the stream's
 * payload bytes [payload_byte_base, payload_byte_base + payload_bytes): the
 * whole payload (base 0) or any slice that covers hz_seek_span's bytes, clamped
 * to the payload's end (bytes past it read as zeros). Keep d_payload congruent to
 * payload_byte_base modulo 16 or better, as hipMalloc'd buffers with
 * hz_seek_span's byte_begin are.
 * flags: HZ_RANGE_FULL_INDEX = d_seek is a complete format-2 block index of the
 * stream, so sub[] is read from it and no walk runs.
 * Needs the decode tables only (hz_codebook_upload_decode). Stream-ordered on the
 * context's stream and capturable by a HIP graph; the host waits only when the
 * context's scratch must grow (at most 65 MiB whatever the range: long ranges
 * run as tiles of 131 072 blocks, a walk and a decode per tile; 16 times as
 * many blocks per tile with a full index, which needs no sub[] rows). Ends a pending
 * index-less part like every scratch user.
 * HZ_EINVAL at the call: null pointers, sym_begin + sym_count > nsym, an odd
 * d_out, unknown flags, no decode tables, 8 * (payload_byte_base + payload_bytes)
 * not below HZ_POS_LIMIT. sym_count 0: HZ_OK, nothing launched.
 * Found on the device and reported by hz_ctx_sync, with nothing written for the
 * block concerned: HZ_EINVAL for a block whose bytes and margins are not inside
 * the slice; HZ_EFORMAT for a descending start[], for a block longer than its
 * symbols times the longest code, for a block whose codewords do not end exactly
 * at start[b + 1] (seek table) or whose first sub[] entry disagrees with start[b]
 * (full index: the rest of sub[] is trusted as in hz_decode). Every walk is
 * bounded by the block's symbol count and its end bit, and no load leaves
 * [d_payload, d_payload + payload_bytes) rounded out to 64-byte lines below (base
 * 0 only, as hz_decode) and to a 4-byte word above. */
int hz_decode_range(hz_ctx *ctx, const uint8_t *d_payload, uint64_t payload_bytes, uint64_t payload_byte_base,
                    const uint64_t *d_seek, uint64_t nsym, uint64_t sym_begin, uint64_t sym_count,
                    uint8_t *d_out, uint32_t flags);

/* Many ranges of one stream in one stream-ordered call. d_ranges is a DEVICE array
 * of nranges entries that the host never reads, so a captured HIP graph can be
 * replayed with new ranges written into the same array. Range i is symbols
 * [sym_begin, sym_begin + sym_count) and goes to d_out + out_byte (2 * sym_count
 * bytes); nothing else of d_out is written. Ranges may overlap, repeat and come in
 * any order; where their OUTPUT bytes overlap, what lands there is unspecified.
 * d_payload, payload_bytes, payload_byte_base, d_seek, nsym, the margins and
 * HZ_RANGE_FULL_INDEX mean what they mean for hz_decode_range; the one slice
 * covers the hz_seek_span of every range. One wave decodes one block of one
 * range: from the seek table it finds the block's chain starts cooperatively
 * (DESIGN.md "A batch of ranges"), with a full index it reads them.
 * d_stats (nullable, HZ_RANGES_STATS_WORDS u64 on the device, zeroed by the call
 * in stream order): [0] blocks decoded and stored, [1] blocks that took the cold
 * path (their payload did not fit a wave's LDS slot), [2] the most fix-up rounds
 * any block's walk needed (<= 64), [3] blocks flagged (nothing stored for them).
 * Needs the decode tables and nranges + 2 u64 of the context's scratch: ends a
 * pending index-less part like every scratch user, and the host waits only when
 * the scratch must grow. No other host synchronisation and no host copy.
 * HZ_EINVAL at the call: null pointers (d_stats may be null), unknown flags, an
 * odd d_out, no decode tables, 8 * (payload_byte_base + payload_bytes) not below
 * HZ_POS_LIMIT. nranges 0: HZ_OK, nothing launched (d_stats is left as it was).
 * Found on the device and reported by hz_ctx_sync: HZ_EINVAL for a range with
 * sym_begin + sym_count > nsym, an odd out_byte or out_byte + 2 * sym_count >
 * out_bytes (nothing is written for that range) and for a block whose bytes and
 * margins are not inside the slice; HZ_EFORMAT for the blocks hz_decode_range
 * reports it for, and for an invalid code. A flagged block stores nothing; every
 * other block of every range is decoded. Every walk is bounded by its lane's
 * segment of the block, by 64 rounds and by the block's end bit, and no load
 * leaves the bounds hz_decode_range documents. */
typedef struct hz_range {
    uint64_t sym_begin;  /* first symbol of the range */
    uint64_t sym_count;  /* symbols; 0 = nothing written */
    uint64_t out_byte;   /* even byte offset in d_out of the range's 2 * sym_count bytes */
} hz_range;
#define HZ_RANGES_STATS_WORDS 4
int hz_decode_ranges(hz_ctx *ctx, const uint8_t *d_payload, uint64_t payload_bytes, uint64_t payload_byte_base,
                     const uint64_t *d_seek, uint64_t nsym, const hz_range *d_ranges, uint32_t nranges,
                     uint8_t *d_out, uint64_t out_bytes, uint64_t *d_stats, uint32_t flags);

/* The same batch from GATHERED PIECES: instead of one slice that covers every
 * range's span (and whatever lies between the spans), d_buf holds only the
 * payload bytes the ranges need, as pieces, and d_seek only the table words the
 * pieces name. Scattered reads of a large stream then move a block and its margins
 * per range, not the hull. hz_seek_pieces plans such a buffer on the host.
 * A PIECE is a contiguous run of the stream's payload, bytes [stream_byte,
 * stream_byte + bytes), standing at d_buf + buf_byte, with the seek entries of
 * blocks first_block .. first_block + nblocks (nblocks + 1 words, contiguous) at
 * d_seek[seek_index ...]. A range names the piece that holds its span (several
 * ranges may name one piece); everything else of a range means what it means for
 * hz_decode_ranges, and so do nsym, d_out, out_bytes and d_stats.
 * d_pieces and d_ranges are DEVICE arrays that the host never reads: the call is
 * stream-ordered and capturable, and a captured graph can be replayed after new
 * pieces, ranges, buffer bytes and table words have been written into the same
 * arrays (entries not in use: sym_count 0, which names no piece).
 * The wave of a block builds the view of its range's piece before it touches the
 * block (DESIGN.md "Gathered pieces"). buf_byte and stream_byte may have any
 * congruence (hz_seek_pieces keeps them equal modulo 64, which keeps the 16-byte
 * staging loads whole). A piece whose stream_byte is 0 starts the stream: its first
 * block needs no margin below. For every other piece, and above, the margins are
 * hz_seek_span's, clamped to the payload's end.
 * flags must be 0 (a full index has no gathered form). Needs the decode tables and
 * nranges + 2 u64 of the context's scratch: ends a pending index-less part like
 * every scratch user, and the host waits only when the scratch must grow.
 * HZ_EINVAL at the call, nothing launched: null pointers (d_stats may be null),
 * nonzero flags, an odd d_out, a d_buf that is not 4-byte aligned, no decode
 * tables, 8 * buf_bytes not below HZ_POS_LIMIT. nranges 0: HZ_OK, nothing launched (d_stats is left as it was).
 * Found on the device and reported by hz_ctx_sync as HZ_EINVAL, with nothing
 * written for the range concerned and every other range decoded: what
 * hz_decode_ranges refuses a range for; piece >= npieces; buf_byte + bytes >
 * buf_bytes; seek_index + nblocks + 1 > seek_words; a block of the range outside
 * [first_block, first_block + nblocks); 8 * (stream_byte + bytes) not below
 * HZ_POS_LIMIT or not fitting 64 bits. Per block, against the piece: HZ_EINVAL
 * for a block whose bytes and margins are not inside the piece, HZ_EFORMAT for
 * what hz_decode_ranges reports it for (a flagged block stores nothing).
 * No load of a block leaves its piece's bytes rounded out to 4-byte words, on the
 * cold path's bit readers included; words of a 16-byte chunk outside the piece
 * read as zeros. So no load leaves [d_buf, d_buf + buf_bytes) rounded up to a
 * 4-byte word (d_buf is 4-byte aligned: the call refuses another). */
typedef struct hz_piece {
    uint64_t stream_byte;  /* payload byte of the stream its first byte is */
    uint64_t bytes;        /* its length */
    uint64_t buf_byte;     /* where it sits in d_buf */
    uint64_t first_block;  /* the block whose seek entry stands at d_seek[seek_index] */
    uint64_t seek_index;   /* entries first_block .. first_block + nblocks at d_seek[seek_index ...] */
    uint64_t nblocks;      /* blocks whose entries (nblocks + 1 words) the piece carries */
} hz_piece;
typedef struct hz_piece_range {
    uint64_t sym_begin, sym_count, out_byte;  /* hz_range's */
    uint64_t piece;                           /* index into d_pieces (not read when sym_count is 0) */
} hz_piece_range;
int hz_decode_ranges_pieces(hz_ctx *ctx, const uint8_t *d_buf, uint64_t buf_bytes,
                            const uint64_t *d_seek, uint64_t seek_words,
                            const hz_piece *d_pieces, uint32_t npieces, uint64_t nsym,
                            const hz_piece_range *d_ranges, uint32_t nranges,
                            uint8_t *d_out, uint64_t out_bytes, uint64_t *d_stats, uint32_t flags);

/* Host arithmetic on a HOST seek table, beside hz_seek_span: the plan of a gathered
 * buffer for a list of ranges. Every non-empty range's hz_seek_span, clamped to
 * payload_bytes, is taken; spans that overlap or touch merge into one piece. Pieces
 * come out in ascending stream_byte, disjoint and not touching; piece k stands at
 * buf_byte = (end of piece k - 1, rounded up to 64) + (stream_byte & 63), so every
 * piece is congruent to its stream position modulo 64; *buf_bytes is the end of the
 * last piece rounded up to 16. A piece carries the seek entries of the hull of its
 * ranges' blocks: seek_index counts up in piece order and *seek_words is the total
 * (the caller gathers seek[first_block .. first_block + nblocks] to seek_index).
 * out[i] is ranges[i] with its piece (an empty range: piece 0, which nothing reads).
 * pieces has room for nranges entries; *npieces receives their number. The sum of
 * the pieces' bytes is at most the sum of the spans', and *buf_bytes at most that
 * sum + 128 * *npieces. HZ_EINVAL: what hz_seek_span refuses, null outputs (ranges,
 * pieces and out may be null when nranges is 0, which gives zeros). HZ_EFORMAT: a
 * span that starts at or past payload_bytes (the table is not this payload's). */
int hz_seek_pieces(const uint64_t *seek, uint64_t nsym, uint64_t payload_bytes,
                   const hz_range *ranges, uint32_t nranges,
                   hz_piece *pieces, uint32_t *npieces,
                   hz_piece_range *out, uint64_t *buf_bytes, uint64_t *seek_words);

/* Expand a seek table into the complete block index of the stream (start[] copied,
 * max_bits and sub[] computed, chains past the end as hz_pack writes them): byte for
 * byte what hz_pack / hz_index_build write. d_payload is the whole payload;
 * d_index holds hz_index_bytes(nsym); d_seek and d_index may be the same pointer.
 * Stream-ordered and capturable, no scratch. A block that fails hz_decode_range's checks leaves
 * its sub[] row unwritten and reports HZ_EFORMAT / HZ_EINVAL at hz_ctx_sync. */
int hz_index_expand(hz_ctx *ctx, const uint8_t *d_payload, uint64_t payload_bytes, const uint64_t *d_seek,
                    uint64_t nsym, uint64_t *d_index);

/* Decode the first nsym codewords of an index-less stream (a .compressed file
 * from the reference encoder; Decompressor.cu:259-291 decodes it serially) into
 * d_out (2*nsym bytes, 16-byte aligned) with no block index: a length walk of
 * long chains over the payload (one chain per lane, recording the start of every
 * 8th codeword of the chain), device-side fix-ups of chains whose lead-in had not
 * resynchronised, then k_decode's block decoder over the chains' 2048-codeword
 * blocks placed by the scanned counts. *d_end_bit (device u64, optional)
 * receives the end bit of codeword nsym - 1, counted from byte 0 of d_payload; a
 * payload with fewer than nsym codewords leaves it at UINT64_MAX (past
 * payload_bytes * 8) with undefined output (the caller checks, as `extract`
 * does). Stream-ordered: no host synchronisation (a HIP graph can capture it)
 * unless the context's scratch grows. A FIXED16 codebook (every code 16 bits)
 * needs no walk: symbol i sits at start_bit + 16 i, decoded directly (also
 * stream-ordered). Every other codebook takes the chain path: DENSE codebooks
 * through a LUT built beside their tables, codes longer than 25 bits through
 * DEEP escapes (the walk resolves them in the decode LUT) and a serial record
 * decoder. Payloads under 16 bytes decode serially in one device thread (also
 * stream-ordered). */
int hz_decode_indexless(hz_ctx *ctx, const uint8_t *d_payload, uint64_t payload_bytes, uint64_t start_bit,
                        uint64_t nsym, uint8_t *d_out, uint64_t *d_end_bit);

/* ---- the seek table from the index-less walk -------------------------------
 * After its walk, fix-ups and scans the index-less decoder knows where every 8th
 * codeword of the stream starts, so a stream's seek table (above) is a light
 * extra pass over that state: no block index is built (hz_index_build computes
 * 256 chain starts per block that a seek table does not keep) and nothing has to
 * be decoded. Entry b of a stream of stream_nsym symbols is the start bit of
 * codeword s_b = min(2048 b, stream_nsym); the last entry is the stream's end.
 *
 * hz_seek_build: the seek table of a bare payload (hz_seek_bytes(nsym) bytes at
 * d_seek), with the scratch of hz_decode_indexless and no output buffer:
 * hz_decode_indexless_seek with d_out NULL, bases 0 and stream_nsym = nsym.
 *
 * hz_decode_indexless_seek: hz_decode_indexless (same arguments, same decoded
 * bytes, same *d_end_bit) that also writes the call's seek entries. The call
 * covers codewords [sym_base, sym_base + nsym) of a longer stream (a window of a
 * file): it writes d_seek[b], addressed from entry 0 of the stream's table, for
 * every b with sym_base <= s_b <= sym_base + nsym. The value is the bit at which
 * codeword s_b - sym_base of the call starts, counted from byte 0 of d_payload,
 * plus bit_base; for s_b = sym_base + nsym that is the call's end bit. Two
 * adjacent calls both write their shared boundary, with equal values. A codeword
 * the payload does not hold (it would start at or past payload_bytes * 8: one
 * that starts exactly at the payload's end has no bit in it) gets UINT64_MAX, as
 * hz_index_build leaves start[nblocks]; only the call's own end, codeword nsym,
 * may stand exactly at the payload's end. d_out may be NULL: table
 * only -- the walk, the fix-ups, the scans and the seek pass run, nothing is
 * decoded, and *d_end_bit (optional) comes from the seek pass (UINT64_MAX where
 * the payload holds fewer than nsym codewords).
 *
 * hz_indexless_seek: the same for a pending part (after hz_indexless_scan /
 * _refix): the part's first codeword is codeword sym_base of the stream (the sum
 * of the earlier parts' counts), nsym at most the part's codewords; values are
 * the scan's stream bits. Does not end the pending part.
 *
 * Stream-ordered and capturable; the host waits only when the scratch grows.
 * HZ_EINVAL at the call: a null d_seek, sym_base + nsym > stream_nsym, no decode
 * tables, a non-null d_out that is not 16-byte aligned, no pending part,
 * bit_base + 8 * payload_bytes not below HZ_POS_LIMIT. nsym 0: HZ_OK, nothing
 * written -- for hz_indexless_seek too (a part that holds no codeword start writes
 * no entry, not even one that its entry bit would fill), where it still needs a
 * pending part. An invalid code reports HZ_EFORMAT at hz_ctx_sync. */
int hz_seek_build(hz_ctx *ctx, const uint8_t *d_payload, uint64_t payload_bytes, uint64_t start_bit,
                  uint64_t nsym, uint64_t *d_seek);
int hz_decode_indexless_seek(hz_ctx *ctx, const uint8_t *d_payload, uint64_t payload_bytes, uint64_t start_bit,
                             uint64_t nsym, uint8_t *d_out, uint64_t *d_end_bit,
                             uint64_t sym_base, uint64_t bit_base, uint64_t stream_nsym, uint64_t *d_seek);
int hz_indexless_seek(hz_ctx *ctx, uint64_t sym_base, uint64_t nsym, uint64_t stream_nsym, uint64_t *d_seek);

/* ---- the seek table from the writer ----------------------------------------
 * The pack holds every block's start bit while it writes, so the table is a
 * by-product of the encode: no walk of the finished stream and no full block
 * index (520 bytes per block to keep 8 of them).
 *
 * hz_pack_seek: hz_pack (d_ranges NULL) or hz_pack_ranges (d_ranges non-null and
 * hz_ranges_bytes(n) != 0; same fallback, same hz_last_pack_ranges) with the same
 * arguments and the same bytes at d_out, that also writes the call's seek entries
 * under the placement rule of hz_decode_indexless_seek. The call covers symbols
 * [sym_base, sym_base + n / 2) of a stream of stream_nsym symbols: it writes
 * d_seek[b], addressed from entry 0 of the stream's table, for every b with
 * sym_base <= s_b <= sym_base + n / 2; the value is the block's start bit counted
 * from byte 0 of d_out, plus bit_base, and for s_b = sym_base + n / 2 the call's
 * end bit. Two adjacent calls both write their shared boundary, with equal
 * values. Nothing else of d_seek is written: no max_bits word, no sub[] rows.
 * With sym_base = bit_base = 0 and stream_nsym = n / 2 the table is the first
 * hz_seek_bytes(n / 2) bytes of the index hz_pack writes.
 * Stream-ordered and capturable like hz_pack. HZ_EINVAL at the call: what hz_pack
 * rejects, a null d_seek, sym_base not a multiple of 2048, sym_base + n / 2 >
 * stream_nsym, a call that is neither whole blocks nor the stream's last,
 * bit_base + 8 * out_cap not below HZ_POS_LIMIT.
 * n / 2 == 0: HZ_OK, nothing written. */
int hz_pack_seek(hz_ctx *ctx, const uint8_t *d_in, uint64_t n, uint64_t start_bit, uint32_t lead,
                 uint8_t *d_out, uint64_t out_cap, void *d_ranges /* nullable */,
                 uint64_t sym_base, uint64_t bit_base, uint64_t stream_nsym, uint64_t *d_seek);

/* ---- one index-less stream over several devices ------------
 * The same decode in PARTS: every device (rank) decodes the payload bits
 * [part_begin, part_end) (counted after start_bit) of one stream, found by
 * self-synchronisation; the parts then exchange three numbers (huffman_amd/
 * dist.py decode_indexless_split):
 *   hz_indexless_scan : walk and fix-ups of the part's chains. entry_bit: the
 *       part's true first codeword start if known, else UINT64_MAX (its walked
 *       entry: right for the stream's first part, and for every part whose
 *       lead-in resynchronised). d_summary (device, 3 x u64): codewords of the
 *       part, its true exit bit (the next part's true entry), the entry bit in
 *       use (entry_bit, or the walked entry for UINT64_MAX).
 *       Bits are STREAM bits: bit 0 is bit 0 of the stream's payload buffer
 *       (the one hz_decode_indexless takes), and d_payload holds stream bits
 *       [payload_bit_base, payload_bit_base + 8 * payload_bytes) -- a rank may
 *       pass only its slice. payload_bit_base is a multiple of 8 and
 *       payload_bytes at least 16 (the walk loads 16-byte chunks), else
 *       HZ_EINVAL. d_payload may have any byte alignment: the kernels view the
 *       slice from the 64-byte line at or below d_payload to the 4-byte word
 *       that holds its last byte (both inside the caller's allocation), no load
 *       leaves that view, and what lies outside it reads as zeros. The slice must
 *       hold the part and the HZ_INDEXLESS_LEAD_BITS before it (or the stream
 *       from its start) and end below HZ_POS_LIMIT, else HZ_EINVAL; the part's
 *       last codeword may run up to max_len bits past part_end (missing bits
 *       read as zeros: keep them in the slice). An explicit entry_bit is a
 *       codeword start of this part: below start_bit + part_begin (the part's
 *       first bit, which the slice holds, so never below payload_bit_base) it is
 *       HZ_EINVAL -- a walk from there would count the previous part's
 *       codewords. part_end <= part_begin and a context without decode tables
 *       are HZ_EINVAL too; every refusal is made at the call, with nothing
 *       launched. nsym: the stream's symbols
 *       (sizes the part's record capacity from its mean bits per codeword;
 *       0 = unknown: the codebook's estimate).
 *   hz_indexless_refix : the part again from its true entry (the previous
 *       part's exit, when it differs from the walked entry); d_summary updated.
 *       entry_bit obeys the scan's rule, against the pending part's first bit
 *       (UINT64_MAX: its walked entry again), else HZ_EINVAL.
 *   hz_indexless_decode : the part's codewords into d_out (2 bytes each, from
 *       the part's first codeword), at most nsym of them (the stream's symbols
 *       from the part's first on); *d_end_bit as hz_decode_indexless when the
 *       stream's last codeword falls in this part (a stream bit).
 * The three calls keep their state in the context's scratch and point at its
 * decode tables: one part per context at a time, and any other call that uses
 * the scratch or replaces the tables ends the pending part -- hz_indexless_refix /
 * _decode / _seek then return HZ_EINVAL, whatever their nsym. (With a pending
 * part and nsym != 0, hz_indexless_decode refuses a d_out that is null or not
 * 16-byte aligned.) The calls that end a part are hz_pack,
 * hz_pack_ranges, hz_pack_seek, hz_index_build, hz_decode_range, hz_decode_ranges,
 * hz_decode_ranges_pieces, hz_codebook_upload_decode (and hz_codebook_upload), a
 * further hz_indexless_scan (its part replaces the pending one) and, under every
 * codebook but FIXED16, hz_decode_indexless, hz_decode_indexless_seek and
 * hz_seek_build of a payload of at least 16 bytes. A call with nothing to do
 * (no symbols, no ranges) returns before it touches the scratch. These use no
 * scratch and leave a pending part good: hz_hist16, hz_block_sums(_check),
 * hz_decode through a block index, hz_index_expand, hz_codebook_upload_encode,
 * hz_codebook_build_device, hz_ctx_sync; under FIXED16 also hz_decode_indexless,
 * hz_decode_indexless_seek and hz_seek_build (arithmetic positions, no walk),
 * and under every codebook the serial decode of a payload under 16 bytes.
 * The same holds for a HIP graph that captured
 * hz_decode_indexless: replay it only while no call on the context has grown
 * the scratch or replaced the decode tables since the capture.
 * Every codebook takes this path; a FIXED16 part (every code 16 bits) is
 * arithmetic: codeword i at start_bit + 16 i, no walk. */
#define HZ_INDEXLESS_LEAD_BITS 1024
int hz_indexless_scan(hz_ctx *ctx, const uint8_t *d_payload, uint64_t payload_bytes, uint64_t payload_bit_base,
                      uint64_t start_bit, uint64_t nsym, uint64_t part_begin, uint64_t part_end, uint64_t entry_bit,
                      uint64_t *d_summary);
int hz_indexless_refix(hz_ctx *ctx, uint64_t entry_bit, uint64_t *d_summary);
int hz_indexless_decode(hz_ctx *ctx, uint64_t nsym, uint8_t *d_out, uint64_t *d_end_bit);

/* Kernel timings of the last hz_hist16 / hz_pack / hz_decode / hz_index_build /
 * hz_decode_indexless call on this context, in milliseconds (HIP events on the
 * context stream). */
int hz_last_kernel_ms(hz_ctx *ctx, int stage, float *ms);
enum { HZ_STAGE_HIST = 0, HZ_STAGE_PACK = 1, HZ_STAGE_DECODE = 2, HZ_STAGE_INDEX = 3, HZ_STAGE_EXTRACT = 4 };

/* Synthetic inputs on the device (DESIGN.md "Synthetic inputs"): byte i of the
 * stream = f(splitmix64(seed ^ (offset + i))); kind 0 uniform, 1 Zipf(alpha). */
int hz_generate(hz_ctx *ctx, uint8_t *d_out, uint64_t n, uint64_t offset, int kind, double alpha,
                uint64_t seed);

/* ---- file level: the CLI contract ---------------------------------------- */

/* `archive <path>`: writes <path>.compressed (Compressor.cu:315-632). */
int hz_archive_file(const char *path, int verbose);
/* Streaming archive of in_path into out_path with bounded memory: two passes
 * over the file in chunk_bytes pieces (histogram, then pack at the running bit
 * offset with the previous chunk's partial word carried as `lead`). Output is
 * byte-identical to the whole-buffer encoder. hz_archive_file uses it with
 * 256 MiB chunks. Replaces the whole-file buffers of Compressor.cu:343-367,585-601. */
int hz_archive_stream(const char *in_path, const char *out_path, uint64_t chunk_bytes, int verbose);
/* hz_archive_stream / hz_archive_file that also return the file's seek table,
 * from the writer (hz_pack_seek): the same output bytes, no pass over the
 * finished file. Bits count from the file byte that holds the first payload bit
 * (hz_header_info's payload_byte), as hz_seek_build_host and
 * hz_extract_stream_seek count, so the tables are interchangeable. Every chunk
 * packs into one device table (sym_base = the symbols packed, bit_base = 8 x the
 * payload bytes handed to the writer), copied out once at the end; the chunk's
 * end bit is read from the table, no per-chunk block index. chunk_bytes is
 * rounded down to a multiple of 4096 (at least 4096) so every chunk is whole
 * blocks; the output does not depend on it. hz_archive_file_seek writes
 * <path>.compressed, honours HZ_ARCHIVE_CHUNK and keeps the input resident under
 * hz_archive_file's condition (then: one hz_pack_seek over the whole input).
 * *nsym receives the file's symbols (size / 2); seek_cap_bytes <
 * hz_seek_bytes(*nsym): HZ_ECAP with *nsym set, before any device work and before
 * the output file is created. seek may be NULL when the table is empty. */
int hz_archive_stream_seek(const char *in_path, const char *out_path, uint64_t chunk_bytes, int verbose,
                           uint64_t *seek, uint64_t seek_cap_bytes, uint64_t *nsym);
int hz_archive_file_seek(const char *path, int verbose, uint64_t *seek, uint64_t seek_cap_bytes, uint64_t *nsym);
/* Streaming extract of in_path into out_path through a device window of
 * chunk_bytes of payload, bounded host and device memory: each round decodes
 * the codewords the window surely holds with hz_decode_indexless (no block
 * index) and carries the unconsumed tail into the next window; the host waits
 * once per round (for the round's end bit), and the next window's file read
 * and this round's fwrite overlap the device. hz_extract_file uses it with
 * 256 MiB windows. Replaces the whole-file buffers of
 * Decompressor.cu:65-114,259-291. */
int hz_extract_stream(const char *in_path, const char *out_path, uint64_t chunk_bytes, int verbose);
/* hz_extract_stream that also returns the file's seek table (bits from the file
 * byte that holds the first payload bit, as hz_seek_build_host counts): every
 * round is hz_decode_indexless_seek into one device table (0.2 % of the output),
 * copied out once at the end. out_path NULL: no output file, nothing decoded,
 * table only. *nsym receives the file's symbols; cap_bytes < hz_seek_bytes(*nsym):
 * HZ_ECAP with *nsym set (nothing else done). Host memory: two windows and the
 * table, whatever the file's size. A truncated file: HZ_EFORMAT. */
int hz_extract_stream_seek(const char *in_path, const char *out_path, uint64_t chunk_bytes, int verbose,
                           uint64_t *seek, uint64_t cap_bytes, uint64_t *nsym);
/* Bytes [offset, offset + count) of the original, from the file on disk and its
 * host seek table, with hz_decode_range_host's semantics (odd offsets and counts,
 * the odd last byte from the header, HZ_EINVAL past the original's size): reads
 * the header (at most 1 MiB) and the hz_seek_span bytes of the range, nothing
 * else. A missing file: HZ_ENOENT (before any device call). */
int hz_decode_range_file(const char *path, const uint64_t *seek, uint64_t offset, uint64_t count, uint8_t *out);
/* Stage split of the calling thread's last hz_archive_stream /
 * hz_extract_stream call (hz_archive_file / hz_extract_file included). Stage
 * times are busy times: host file reads and writes overlap the device's
 * copies and kernels, so they do not add up to total_ms. */
typedef struct hz_stream_timing {
    double total_ms;   /* wall clock of the call */
    double fread_ms;   /* host: file reads */
    double fwrite_ms;  /* host: file writes */
    double alloc_ms;   /* host: device context, device buffers, pinned host buffers */
    double host_ms;    /* host: codebook build, header write / parse, table uploads */
    double h2d_ms;     /* device: host-to-device copies */
    double kernel_ms;  /* device: histogram, pack, index build, decode */
    double d2h_ms;     /* device: device-to-host copies */
    uint64_t bytes_in;   /* bytes read from in_path */
    uint64_t bytes_out;  /* bytes written to out_path */
} hz_stream_timing;
int hz_stream_last_timing(hz_stream_timing *t);
/* `extract <path>`: writes ./DECOMPRESSED_FILE or DECOMPRESSED_FILE(k)
 * (Decompressor.cu:47-114,185-219). out_name may be NULL. */
int hz_extract_file(const char *path, char *out_name, size_t out_name_cap, int verbose);

/* Whole-buffer host API (device work inside): encode host bytes to a complete
 * .compressed image / decode one. */
int hz_encode_host(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len);
int hz_encoded_size(const uint8_t *in, uint64_t n, uint64_t *out_len);
int hz_decode_host(const uint8_t *file, uint64_t len, uint8_t *out, uint64_t cap, uint64_t *out_n);
/* hz_encode_host that also returns the image's seek table from the writer (the
 * table hz_seek_build_host finds in the image): hz_seek_bytes(n / 2) bytes at
 * seek; seek_cap_bytes below that: HZ_ECAP before any device work. */
int hz_encode_host_seek(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len,
                        uint64_t *seek, uint64_t seek_cap_bytes);

/* Whole-buffer host forms of random access (device work inside). hz_seek_build_host:
 * the seek table of a .compressed image (reference-written files included) into
 * seek (cap_bytes >= hz_seek_bytes(*nsym), else HZ_ECAP with *nsym set); bits
 * count from the file byte that holds the first payload bit (hz_header_info's
 * payload_byte). hz_decode_range_host: bytes [offset, offset + count) of the
 * original from an image and its host seek table into out; odd offsets and counts
 * are served by decoding the covering symbols, and the odd trailing byte of an
 * odd-sized original comes from the header. Only the header's codebook, the
 * range's seek entries and the span's payload bytes go to the device.
 * offset + count past the original's size: HZ_EINVAL.
 * hz_decode_ranges_host: nranges byte ranges [offsets[i], offsets[i] + counts[i])
 * in one hz_decode_ranges call, their bytes concatenated in out in list order; one
 * payload slice goes to the device, from the smallest byte_begin to the largest
 * byte_end of the ranges' spans (whatever lies between them included).
 * hz_decode_ranges_host_pieces: the same bytes for the same arguments, from gathered
 * pieces: hz_seek_pieces' plan, one staging buffer of its buf_bytes with each piece
 * copied in, the compact table, one hz_decode_ranges_pieces call. What goes to the
 * device is buf_bytes + 8 * seek_words + the two lists, whatever lies between the
 * ranges. hz_decode_ranges_file: that flow on a file on disk, as
 * hz_decode_range_file reads one range: the header (at most 1 MiB) and each piece's
 * bytes are read (pread), nothing else. A missing file: HZ_ENOENT before any device
 * call. Both: a span that starts at or past the payload's end: HZ_EFORMAT. */
int hz_decode_ranges_host_pieces(const uint8_t *file, uint64_t len, const uint64_t *seek, const uint64_t *offsets,
                                 const uint64_t *counts, uint32_t nranges, uint8_t *out);
int hz_decode_ranges_file(const char *path, const uint64_t *seek, const uint64_t *offsets,
                          const uint64_t *counts, uint32_t nranges, uint8_t *out);
int hz_decode_ranges_host(const uint8_t *file, uint64_t len, const uint64_t *seek, const uint64_t *offsets,
                          const uint64_t *counts, uint32_t nranges, uint8_t *out);
int hz_seek_build_host(const uint8_t *file, uint64_t len, uint64_t *seek, uint64_t cap_bytes, uint64_t *nsym);
int hz_decode_range_host(const uint8_t *file, uint64_t len, const uint64_t *seek, uint64_t offset,
                         uint64_t count, uint8_t *out);

/* ---- seekable files: seek table and block checksums in a file trailer -------
 * The reference `extract` reads the header, decodes N / 2 codewords and stops
 * (Decompressor.cu:103-108,259-291): it never reads to the end of the file. Bytes
 * behind the payload are invisible to it, so a SEEKABLE file is a .compressed file
 * with a trailer, and stays a valid .compressed file for the reference and for every
 * reader here:
 *
 *   [ the .compressed image, byte for byte what the plain writer produces ]  image_bytes
 *   [ 0..7 zero bytes up to a multiple of 8 ]
 *   [ seek table: u64 x (nblocks + 1), little-endian ]   at seek_off
 *   [ block sums: u32 x nblocks ]                        at sums_off, only with HZ_SEEKABLE_SUMS
 *   [ zero bytes up to a multiple of 8 ]
 *   [ footer, 64 bytes, at the end of the file ]
 *
 * The seek table is the one hz_archive_stream_seek returns: bits count from the file
 * byte that holds the first payload bit. Sum b is hz_block_sums' word of the original's
 * bytes [4096 b, min(4096 (b + 1), 2 nsym)), zero-extended to 4096. The odd last byte
 * of an odd-sized original lives in the header and is NOT covered by a sum.
 * Footer, little-endian:
 *    0  8 bytes magic "HZSKTRL1"
 *    8  u32 version = 1
 *   12  u32 flags (bit 0: sums present; other bits 0)
 *   16  u64 n, the original's size in bytes
 *   24  u64 image_bytes
 *   32  u64 seek_off
 *   40  u64 sums_off (0 when absent)
 *   48  u32 block symbols = 2048
 *   52  u32 0
 *   56  u32 0
 *   60  u32 Adler-32 of footer bytes [0, 60)
 * A file HAS A TRAILER when the magic and the footer check both match; any other file
 * is a plain file, which is not an error (present = 0). A file whose magic and check
 * match but whose fields do not fit is HZ_EFORMAT; they fit when version = 1, no
 * unknown flag bit is set, block symbols = 2048, seek_off is a multiple of 8 with
 * image_bytes <= seek_off < image_bytes + 8, sums_off = seek_off + hz_seek_bytes(n / 2)
 * when sums are present (0 when not), and the file's size is the end of the last
 * section rounded up to 8, plus 64 -- all of it computed without a wrap, whatever n
 * claims. Flows that also parse the header return HZ_EFORMAT when its N differs from
 * the footer's. n < 2 still gets a trailer: an empty table, no sums words, the footer.
 *
 * EXISTING READERS IGNORE THE TRAILER: for hz_extract_stream, hz_extract_stream_seek,
 * hz_extract_file, hz_decode_host, hz_seek_build_host, hz_decode_range_host,
 * hz_decode_ranges_host, hz_decode_ranges_host_pieces, hz_decode_range_file and
 * hz_decode_ranges_file (and the `extract` CLI) a file with a trailer ends at
 * image_bytes; files without one take the path they always took.
 *
 * Host only, no device call (hz_seekable.cpp links without HIP):
 *   hz_seekable_trailer_bytes: bytes of the trailer behind an image of image_bytes
 *     (padding, table, sums with HZ_SEEKABLE_SUMS, padding, footer); 0 when they do not
 *     fit 64 bits.
 *   hz_seekable_trailer_write: those bytes into out (cap below them: HZ_ECAP with *len
 *     set). seek / sums may be NULL when the table / the sums are empty.
 *   hz_seekable_footer_parse: the last 64 bytes of a file of file_bytes (last64 may be
 *     NULL when file_bytes < 64: a plain file) into info; nsym = n / 2, nblocks =
 *     ceil(nsym / 2048).
 *   hz_seekable_info_file: the same for a path (HZ_ENOENT for a missing file); reads
 *     the footer only.
 *   hz_seekable_load_file: the table (hz_seek_bytes(*nsym) bytes) and, with sums non-NULL,
 *     the sums (4 * nblocks bytes) of a file with a trailer; a capacity too small:
 *     HZ_ECAP with *nsym set; a plain file: HZ_EFORMAT; sums asked of a file without
 *     them: HZ_EINVAL. */
#define HZ_SEEKABLE_FOOTER_BYTES 64
#define HZ_SEEKABLE_SUMS   1u   /* writers: store block sums */
#define HZ_SEEKABLE_VERIFY 2u   /* readers: check every decoded block against its sum */
typedef struct hz_seekable_info {
    uint32_t present, version, flags, reserved;
    uint64_t n, nsym, nblocks, image_bytes, seek_off, sums_off, file_bytes;
} hz_seekable_info;
uint64_t hz_seekable_trailer_bytes(uint64_t image_bytes, uint64_t n, uint32_t flags);
int hz_seekable_trailer_write(uint64_t image_bytes, uint64_t n, const uint64_t *seek, const uint32_t *sums,
                              uint32_t flags, uint8_t *out, uint64_t cap, uint64_t *len);
int hz_seekable_footer_parse(const uint8_t *last64, uint64_t file_bytes, hz_seekable_info *info);
int hz_seekable_info_file(const char *path, hz_seekable_info *info);
int hz_seekable_load_file(const char *path, uint64_t *seek, uint64_t seek_cap_bytes,
                          uint32_t *sums, uint64_t sums_cap_bytes, uint64_t *nsym);

/* Writers (device work inside). The first image_bytes of the output are byte for byte
 * what hz_encode_host / hz_archive_stream write for the same input; the table comes from
 * the writer as in hz_encode_host_seek / hz_archive_stream_seek (no pass over the finished
 * file), and with HZ_SEEKABLE_SUMS the sums from hz_block_sums on the input while it is on
 * the device for the pack: chunk k writes its words at block (chunk offset / 4096) of one
 * device array, copied out once at the end like the table. The streaming form's host
 * memory is its chunks plus the table and the sums, and the output's final size, trailer
 * included, is reserved before the first write. flags other than HZ_SEEKABLE_SUMS:
 * HZ_EINVAL. hz_encode_host_seekable: cap too small gives HZ_ECAP with *out_len set. */
int hz_encode_host_seekable(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len, uint32_t flags);
int hz_archive_stream_seekable(const char *in_path, const char *out_path, uint64_t chunk_bytes, int verbose, uint32_t flags);

/* Readers. hz_seekable_read_host / hz_seekable_read_file: byte ranges of the original with
 * the semantics of hz_decode_ranges_host_pieces / hz_decode_ranges_file (odd offsets and
 * counts, the odd last byte from the header, list order, HZ_EINVAL past the original's
 * size), with the table taken from the file's trailer; a file without one: HZ_EFORMAT.
 * The file form reads the 64-byte footer, the header (at most 1 MiB), the seek words
 * [first_block, first_block + nblocks] of each piece (pread at seek_off + 8 first_block;
 * first each range's own words b0 .. b1 + 1, which is all hz_seek_span reads, then
 * hz_seek_pieces on the words it has), each piece's payload bytes and, with
 * HZ_SEEKABLE_VERIFY, the sums words of the blocks it decodes: never the whole table.
 * flags = HZ_SEEKABLE_VERIFY: every range is rounded out to whole blocks (down to a
 * multiple of 2048 symbols, up to the next one or nsym) and decoded, by the same single
 * hz_decode_ranges_pieces call, into a zero-filled device temporary at a 4096-aligned
 * offset; one hz_block_sums runs over the temporary and every block's word is compared
 * with the file's (the zero fill makes the stream's last, partial block match). A
 * mismatch: HZ_ECHECKSUM, *bad_block (nullable) the smallest failing block, out not
 * written. HZ_SEEKABLE_VERIFY on a file without sums: HZ_EINVAL.
 * hz_seekable_verify_file: the verified read over [0, n) in tiles of at most 64 MiB of
 * output, the bytes discarded: HZ_OK, HZ_ECHECKSUM with the first bad block, or the
 * decoder's own status. */
int hz_seekable_read_host(const uint8_t *file, uint64_t len, const uint64_t *offsets, const uint64_t *counts,
                          uint32_t nranges, uint8_t *out, uint32_t flags, uint64_t *bad_block);
int hz_seekable_read_file(const char *path, const uint64_t *offsets, const uint64_t *counts,
                          uint32_t nranges, uint8_t *out, uint32_t flags, uint64_t *bad_block);
int hz_seekable_verify_file(const char *path, uint64_t *bad_block);

/* Existing files, in place, and the verified whole-file read. Both are the windowed index-less
 * extract (hz_extract_stream_seek: a payload window of chunk_bytes, the walk's own table collected) run
 * in ROUNDS OF WHOLE BLOCKS: every round but the file's last decodes a positive multiple of 2048
 * symbols, on the redo path too, so a round's output, while it is still on the device, begins at block
 * (symbols done / 2048) of the file's block sums. A window must hold one block of the longest codes,
 * 2048 x 56 bits = 14 336 bytes: chunk_bytes below HZ_SEEKABLE_MIN_WINDOW is HZ_EINVAL before anything
 * is touched. A missing file: HZ_ENOENT before any device call.
 *
 * hz_seekable_attach_file: put a trailer behind a .compressed file that has none (the reference
 * encoder's, hz_archive_stream's, the `archive` CLI's), or sums into a trailer written without them.
 * flags is 0 or HZ_SEEKABLE_SUMS (anything else: HZ_EINVAL). With HZ_SEEKABLE_SUMS every round decodes
 * into the device output buffer and one hz_block_sums over it writes the round's words into one device
 * array, copied out once at the end like the table: no pinned output buffer, no file write. Without
 * the flag nothing is decoded (hz_extract_stream_seek without an out_path). The trailer is composed by
 * hz_seekable_trailer_write and appended once EVERY round has succeeded: padding, table and sums
 * first, the footer last; bytes [0, image_bytes) are never rewritten. A truncated or malformed file
 * returns its status (HZ_EFORMAT ...) and stays byte for byte what it was. A file that has a trailer
 * with everything flags asks for: HZ_OK, *attached (nullable) = 0, the file untouched. One whose
 * trailer lacks the sums asked for: the image ends at image_bytes and the new trailer is written from
 * there over the old one (the file grows). Otherwise *attached = 1. Host memory: one pinned window,
 * the table and the sums and the trailer composed from them, whatever the file's size. The result is
 * what hz_archive_stream_seekable writes for the same original and flags when this library wrote the
 * image, and for any valid image the file's bytes, the table hz_seek_build_host finds in them and
 * hz_block_sums' words of the original.
 *
 * hz_extract_stream_verified: hz_extract_stream of a seekable file with sums, every block checked
 * before it is written. A plain file: HZ_EFORMAT; a trailer without sums: HZ_EINVAL; a header N that
 * differs from the footer's: HZ_EFORMAT. The stored table and sums are read from the trailer, the sums
 * uploaded once; each round is hz_decode_indexless_seek and then hz_block_sums_check on its output at
 * block_base = symbols done / 2048, into one device word (UINT64_MAX at first) that comes home with the
 * round's end bit -- the one host wait a round already has. A round's bytes go to out_path only after
 * the round matched. On a mismatch: HZ_ECHECKSUM, *bad_block (nullable) the smallest failing block,
 * and the output ends after the rounds before the failing one: a verified prefix whose size is a
 * multiple of 4096 (on any other failure too the output ends at its last written round, never at a
 * reserved size). After the last round the table the walk produced is compared with the stored one
 * on the host: HZ_EFORMAT when they differ -- the output is then complete and correct (every block
 * matched), the status says the stored table is not this payload's, so range reads would fail.
 * out_path NULL: decode and check, write nothing. */
#define HZ_SEEKABLE_MIN_WINDOW 16384
int hz_seekable_attach_file(const char *path, uint64_t chunk_bytes, uint32_t flags, int *attached);
int hz_extract_stream_verified(const char *in_path, const char *out_path, uint64_t chunk_bytes, int verbose,
                               uint64_t *bad_block);

/* Salvage of a damaged seekable file: EVERY bad block named, the rest kept. The readers above stop at the
 * first problem; one flipped payload bit damages one block, and the file carries what recovery needs: the
 * table restarts the decode at every block independently of the block before it, and the sums say which
 * blocks came out right. hz_seekable_salvage_file writes to out_path the original with every block that
 * could not be verified replaced by 4096 zero bytes (its share of n for the last block), and lists those
 * blocks: *nbad their number, bad_blocks[0 .. min(*nbad, bad_cap)) the blocks in ascending order
 * (bad_blocks may be NULL with bad_cap 0). The output's size is exactly n, the odd last byte from the
 * header included. A COMPLETED SALVAGE RETURNS HZ_OK whether or not blocks were lost. out_path NULL:
 * decode and check, write nothing -- the whole-file scan that names every bad block.
 *
 * Refusals: a plain file HZ_EFORMAT; a trailer without sums HZ_EINVAL; a header N that differs from the
 * footer's HZ_EFORMAT; chunk_bytes below HZ_SEEKABLE_MIN_WINDOW, a NULL in_path or nbad, an unknown flag
 * HZ_EINVAL; a missing file HZ_ENOENT before any device call; a header that does not parse: its status,
 * nothing written. A DAMAGED CODEBOOK OR FOOTER IS NOT SALVAGEABLE: without the codebook no block decodes,
 * and without the footer the file is a plain file.
 *
 * The stored table and sums are read from the trailer and uploaded once, and a device bitmap of
 * ceil(nblocks / 32) words is zeroed. The blocks are cut into WINDOWS from the stored table, WHICH MAY
 * ITSELF BE DAMAGED (hz_salvage_plan.h): a block is trusted when its own two entries ascend, lie at most
 * 2048 x max_len bits apart and end inside the payload -- the decoder's own check, so a block that is not
 * trusted is flagged whatever it is given -- and a window's payload span is the hull of hz_seek_span of its
 * trusted blocks; a block joins the window while that span and the window's output (4096 bytes a block)
 * stay within chunk_bytes. Per window: its span is read and uploaded, its device output zero-filled, ONE
 * hz_decode_ranges call with one range decodes it (a block the decoder flags stores nothing and keeps
 * the zeros), hz_block_sums_mark judges every block of the output at block_base = the window's first
 * block (with HZ_SUMS_ZERO_BAD unless HZ_SALVAGE_KEEP_UNVERIFIED is set), the output is copied out, and
 * one hz_ctx_sync -- the window's only host wait -- brings the decoder's status home: HZ_EFORMAT or
 * HZ_EINVAL with flagged blocks counted (d_stats[3] > 0) is the expected report and the flow goes on, any
 * other status ends it. The window's bytes go to file offset 4096 x first block beside the next window's
 * work. Host and device memory are bounded by chunk_bytes, the table, the sums and the bitmap, whatever
 * the file's size. Whatever ends the flow early, the output ends at its last written byte.
 *
 * WHAT A VERDICT MEANS. A block is reported bad when its output does not match its stored sum. The cause
 * may be damage to its payload bits, a damaged table entry (which can cost the two blocks that share it) or
 * a damaged sum word; in the last case the decoded bytes were right, and HZ_SALVAGE_KEEP_UNVERIFIED keeps
 * every block's decoded bytes in the output (a flagged block's are still zeros: it decoded to nothing), so
 * the caller can judge them by other means. A block the decoder flagged whose stored sum is that of 4096
 * zero bytes is reported good: its output is zeros and matches, the same strength of evidence every other
 * block has. */
#define HZ_SALVAGE_KEEP_UNVERIFIED 1u
int hz_seekable_salvage_file(const char *in_path, const char *out_path, uint64_t chunk_bytes, uint32_t flags,
                             uint64_t *bad_blocks, uint64_t bad_cap, uint64_t *nbad);

#ifdef __cplusplus
}
#endif
#endif /* HUFFMAN_AMD_H */
