"""MI355X-native Huffman codec (gfx950): drop-in for yechuan51/huffman's
`archive` / `extract` path. See DESIGN.md and include/huffman_amd.h."""
from ._lib import HZError, LIB_PATH, BIN_DIR, load  # noqa: F401
from .codec import (Device, archive, archive_seek, archive_stream, archive_stream_seek, encode_seek, build_codebook, codebook_arrays, decode, encode, extract, extract_stream, stream_timing,  # noqa: F401
                    header_bits, index_bytes, index_starts, parse_header, payload_bits, write_header,
                    build_seek, build_seek_file, decode_range, decode_range_file, decode_ranges, decode_ranges_file,
                    seek_bytes, seek_entries, seek_pieces, seek_span,
                    archive_seekable, block_sums_bytes, encode_seekable, load_seek, load_sums, read_seekable,
                    seekable_info, verify_seekable, make_seekable, extract_verified, salvage)

__all__ = ["Device", "HZError", "archive", "archive_stream", "extract", "extract_stream", "stream_timing", "encode", "decode", "build_codebook", "codebook_arrays",
           "header_bits", "payload_bits", "write_header", "parse_header", "index_bytes", "index_starts", "load", "LIB_PATH",
           "BIN_DIR", "build_seek", "build_seek_file", "decode_range", "decode_range_file", "decode_ranges", "seek_bytes",
           "seek_entries", "seek_span", "seek_pieces", "decode_ranges_file", "archive_seek", "archive_stream_seek", "encode_seek",
           "archive_seekable", "block_sums_bytes", "encode_seekable", "load_seek", "load_sums", "read_seekable",
           "seekable_info", "verify_seekable", "make_seekable", "extract_verified", "salvage"]
