"""A plain restatement of the seekable trailer (include/huffman_amd.h "seekable files") with struct, numpy
and zlib.adler32: the trailer's bytes, the footer's fields, the block sums of an original. It does not
touch the library, so the tests compare the library with this file.

    [ image ][ zeros to a multiple of 8 ][ u64 seek[nblocks + 1] ][ u32 sums[nblocks], if flagged ]
    [ zeros to a multiple of 8 ][ 64-byte footer ]"""
import struct
import zlib

import numpy as np

MAGIC = b"HZSKTRL1"
VERSION = 1
FOOTER_BYTES = 64
BLOCK_SYMS = 2048
BLOCK_BYTES = 2 * BLOCK_SYMS
SUMS, VERIFY = 1, 2
FOOTER = struct.Struct("<8sIIQQQQIII")   # the 60 bytes the check covers
# byte offset of every footer field
FIELDS = {"magic": 0, "version": 8, "flags": 12, "n": 16, "image_bytes": 24, "seek_off": 32, "sums_off": 40,
          "block_syms": 48, "zero0": 52, "zero1": 56, "check": 60}


def nblocks(n):
    return (n // 2 + BLOCK_SYMS - 1) // BLOCK_SYMS


def seek_words(n):
    return nblocks(n) + 1 if n // 2 else 0


def up8(x):
    return (x + 7) // 8 * 8


def block_sums(data):
    """One zlib.adler32 per 4096 bytes of the original's 2 * (n // 2) symbol bytes, the last block
    extended with zero bytes to 4096 (the odd last byte lives in the header and is not covered)."""
    body = bytes(data[:len(data) // 2 * 2])
    return np.array([zlib.adler32(body[o:o + BLOCK_BYTES].ljust(BLOCK_BYTES, b"\0"))
                     for o in range(0, len(body), BLOCK_BYTES)], dtype=np.uint32)


def adler_blocks(buf, n):
    """hz_block_sums of buf[:n]: ceil(n / 4096) words (every byte of buf[:n] is covered)."""
    b = bytes(buf[:n])
    return np.array([zlib.adler32(b[o:o + BLOCK_BYTES].ljust(BLOCK_BYTES, b"\0")) for o in range(0, n, BLOCK_BYTES)],
                    dtype=np.uint32)


def layout(image_bytes, n, flags):
    seek_off = up8(image_bytes)
    sums_at = seek_off + 8 * seek_words(n)
    end = sums_at + (4 * nblocks(n) if flags & SUMS else 0)
    return dict(seek_off=seek_off, sums_off=sums_at if flags & SUMS else 0, file_bytes=up8(end) + FOOTER_BYTES)


def footer(image_bytes, n, flags):
    l = layout(image_bytes, n, flags)
    body = FOOTER.pack(MAGIC, VERSION, flags, n, image_bytes, l["seek_off"], l["sums_off"], BLOCK_SYMS, 0, 0)
    return body + struct.pack("<I", zlib.adler32(body))


def reseal(foot):
    """A footer with its check recomputed over whatever its first 60 bytes now hold."""
    return bytes(foot[:60]) + struct.pack("<I", zlib.adler32(bytes(foot[:60])))


def trailer(image_bytes, n, seek, sums, flags):
    """The bytes behind an image of image_bytes: seek (u64 words) and sums (u32 words, with SUMS)."""
    seek = np.asarray(seek, dtype="<u8")
    assert seek.size == seek_words(n)
    l = layout(image_bytes, n, flags)
    out = b"\0" * (l["seek_off"] - image_bytes) + seek.tobytes()
    if flags & SUMS:
        sums = np.asarray(sums, dtype="<u4")
        assert sums.size == nblocks(n)
        out += sums.tobytes()
    out += b"\0" * (l["file_bytes"] - FOOTER_BYTES - image_bytes - len(out))
    out += footer(image_bytes, n, flags)
    assert image_bytes + len(out) == l["file_bytes"]
    return out


def info(image_bytes, n, flags):
    """What hz_seekable_footer_parse reports for that trailer."""
    l = layout(image_bytes, n, flags)
    return dict(present=1, version=VERSION, flags=flags, n=n, nsym=n // 2, nblocks=nblocks(n), image_bytes=image_bytes,
                seek_off=l["seek_off"], sums_off=l["sums_off"], file_bytes=l["file_bytes"])
