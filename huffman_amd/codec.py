"""Host-side mirror of the reference's interface for the Huffman path.

The reference exposes two executables:
  archive <file>             -> <file>.compressed          (Compressor.cu:315-632)
  extract <file.compressed>  -> ./DECOMPRESSED_FILE[(k)]   (Decompressor.cu:47-114)
`archive()` / `extract()` here are those entry points (same outputs, same
file names); `encode()` / `decode()` are their in-memory forms; `Device`
exposes the stages on device pointers (calculateFrequency -> hist16,
gpuCodebookConstruction -> build_codebook, populateCWLength + scan +
encodeFromCW -> pack, translateFile -> decode). Every call goes to the gfx950
kernels of libhuffman_amd.so.
"""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import Codebook, HeaderInfo, check, load

HZ_NSYM = _lib.HZ_NSYM


def _buf(data):
    arr = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    arr = np.ascontiguousarray(arr, dtype=np.uint8)
    return arr, arr.ctypes.data_as(ctypes.c_void_p)


def encode(data):
    """Bytes -> complete .compressed image (what `archive` writes)."""
    lib = load()
    arr, p = _buf(data)
    n = arr.size
    need = ctypes.c_uint64()
    check(lib.hz_encoded_size(p, n, ctypes.byref(need)), "hz_encoded_size")
    out = np.empty(max(need.value, 1), dtype=np.uint8)
    got = ctypes.c_uint64()
    check(lib.hz_encode_host(p, n, out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(got)),
          "hz_encode_host")
    return out[:got.value].tobytes()


def _seek_table(nsym):
    """A host seek table for nsym symbols: (the array to return, the buffer handed to the library)."""
    words = seek_bytes(nsym) // 8
    buf = np.zeros(max(words, 1), dtype=np.uint64)
    return buf[:words], buf


def encode_seek(data):
    """Bytes -> (complete .compressed image, its seek table): encode() with the table the writer knows
    while it packs (uint64 start[nblocks + 1], as build_seek counts), no pass over the finished image."""
    lib = load()
    arr, p = _buf(data)
    n = arr.size
    need = ctypes.c_uint64()
    check(lib.hz_encoded_size(p, n, ctypes.byref(need)), "hz_encoded_size")
    out = np.empty(max(need.value, 1), dtype=np.uint8)
    seek, buf = _seek_table(n // 2)
    got = ctypes.c_uint64()
    check(lib.hz_encode_host_seek(p, n, out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(got),
                                  buf.ctypes.data_as(ctypes.c_void_p), buf.size * 8), "hz_encode_host_seek")
    return out[:got.value].tobytes(), seek


def decode(blob):
    """.compressed image -> original bytes (what `extract` writes)."""
    lib = load()
    arr, p = _buf(blob)
    cb, info = parse_header(_image(arr))
    n_out = 2 * (info.n // 2) + (1 if info.is_odd else 0)
    out = np.empty(max(n_out, 1), dtype=np.uint8)
    got = ctypes.c_uint64()
    check(lib.hz_decode_host(p, arr.size, out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(got)),
          "hz_decode_host")
    return out[:got.value].tobytes()


def archive(path, verbose=True):
    """`archive <path>`: writes <path>.compressed; returns its name."""
    check(load().hz_archive_file(str(path).encode(), int(verbose)), "hz_archive_file")
    return str(path) + ".compressed"


def archive_stream(path, out_path, chunk_bytes=1 << 30, verbose=False):
    """Streaming `archive` with bounded memory (chunks of chunk_bytes)."""
    check(load().hz_archive_stream(str(path).encode(), str(out_path).encode(), chunk_bytes, int(verbose)),
          "hz_archive_stream")
    return str(out_path)


def archive_seek(path, verbose=True):
    """archive() that also returns the file's seek table, from the writer: (name, seek). The table is
    what build_seek_file(name) would find, without reading the .compressed file back."""
    seek, buf = _seek_table(os.path.getsize(path) // 2)
    nsym = ctypes.c_uint64()
    check(load().hz_archive_file_seek(os.fsencode(path), int(verbose), buf.ctypes.data_as(ctypes.c_void_p), buf.size * 8,
                                      ctypes.byref(nsym)), "hz_archive_file_seek")
    return str(path) + ".compressed", seek[:seek_bytes(nsym.value) // 8]


def archive_stream_seek(path, out_path, chunk_bytes=1 << 30, verbose=False):
    """archive_stream() that returns the file's seek table, from the writer (chunks are rounded down
    to whole 4096-byte blocks; the output does not depend on the chunk size)."""
    seek, buf = _seek_table(os.path.getsize(path) // 2)
    nsym = ctypes.c_uint64()
    check(load().hz_archive_stream_seek(os.fsencode(path), os.fsencode(out_path), chunk_bytes, int(verbose),
                                        buf.ctypes.data_as(ctypes.c_void_p), buf.size * 8, ctypes.byref(nsym)),
          "hz_archive_stream_seek")
    return seek[:seek_bytes(nsym.value) // 8]


def extract_stream(path, out_path, chunk_bytes=1 << 30, verbose=False):
    """Streaming `extract` with bounded memory (payload windows of chunk_bytes)."""
    check(load().hz_extract_stream(str(path).encode(), str(out_path).encode(), chunk_bytes, int(verbose)),
          "hz_extract_stream")
    return str(out_path)


def stream_timing():
    """Stage split (dict) of this thread's last archive_stream / extract_stream call."""
    from ._lib import StreamTiming
    t = StreamTiming()
    check(load().hz_stream_last_timing(ctypes.byref(t)), "hz_stream_last_timing")
    return t.as_dict()


def extract(path, verbose=True):
    """`extract <path>`: writes ./DECOMPRESSED_FILE (or (k)); returns its name."""
    name = ctypes.create_string_buffer(256)
    check(load().hz_extract_file(str(path).encode(), name, 256, int(verbose)), "hz_extract_file")
    return name.value.decode()


def build_codebook(hist):
    """65 536-entry host histogram -> Codebook with the reference's semantics."""
    h = np.ascontiguousarray(hist, dtype=np.uint64)
    assert h.size == HZ_NSYM
    cb = Codebook()
    check(load().hz_codebook_build(h.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cb)), "hz_codebook_build")
    return cb


def codebook_arrays(cb):
    """(order[U], len[65536], code[65536]) numpy views of a Codebook."""
    order = np.ctypeslib.as_array(cb.order)[:cb.nsym].copy()
    return order, np.ctypeslib.as_array(cb.len).copy(), np.ctypeslib.as_array(cb.code).copy()


def header_bits(cb, n):
    v = ctypes.c_uint64()
    check(load().hz_header_bits(ctypes.byref(cb), n, ctypes.byref(v)), "hz_header_bits")
    return v.value


def payload_bits(cb, hist):
    h = np.ascontiguousarray(hist, dtype=np.uint64)
    v = ctypes.c_uint64()
    check(load().hz_payload_bits(ctypes.byref(cb), h.ctypes.data_as(ctypes.c_void_p), ctypes.byref(v)),
          "hz_payload_bits")
    return v.value


def write_header(cb, n, last_byte=0):
    """-> (complete header bytes, pending bit count, pending byte MSB-aligned)."""
    hb = header_bits(cb, n)
    out = np.zeros(hb // 8 + 8, dtype=np.uint8)
    nb, pb, pend = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint8()
    check(load().hz_header_write(ctypes.byref(cb), n, last_byte, out.ctypes.data_as(ctypes.c_void_p), out.size,
                                 ctypes.byref(nb), ctypes.byref(pb), ctypes.byref(pend)), "hz_header_write")
    return out[:nb.value].tobytes(), pb.value, pend.value


def parse_header(blob):
    arr, p = _buf(blob)
    cb, info = Codebook(), HeaderInfo()
    check(load().hz_header_parse(p, arr.size, ctypes.byref(cb), ctypes.byref(info)), "hz_header_parse")
    return cb, info


def index_bytes(nsym):
    """Bytes of the block index hz_pack writes for nsym symbols (include/huffman_amd.h)."""
    return load().hz_index_bytes(nsym)


def index_starts(index, nsym):
    """The u64 start[] part of a block index (numpy or torch int64 view)."""
    nb = (nsym + load().hz_index_stride() - 1) // load().hz_index_stride()
    return index[:nb + 1]


def seek_bytes(nsym):
    """Bytes of a stream's seek table: the first words (start[]) of its block index."""
    return load().hz_seek_bytes(nsym)


def seek_span(seek_host, nsym, sym_begin, sym_count):
    """(byte_begin, byte_end) of the payload a range decode reads (hz_seek_span): host arithmetic."""
    seek = np.ascontiguousarray(seek_host, dtype=np.uint64)
    if seek.size * 8 < seek_bytes(nsym):
        raise ValueError("seek table shorter than seek_bytes(nsym)")
    b, e = ctypes.c_uint64(), ctypes.c_uint64()
    check(load().hz_seek_span(seek.ctypes.data_as(ctypes.c_void_p), nsym, sym_begin, sym_count, ctypes.byref(b),
                              ctypes.byref(e)), "hz_seek_span")
    return b.value, e.value


PIECE_DTYPE = np.dtype([(n, np.uint64) for n in ("stream_byte", "bytes", "buf_byte", "first_block", "seek_index", "nblocks")])
PIECE_RANGE_DTYPE = np.dtype([(n, np.uint64) for n in ("sym_begin", "sym_count", "out_byte", "piece")])


def seek_pieces(seek_host, nsym, payload_bytes, ranges):
    """The plan of a gathered buffer (hz_seek_pieces): host arithmetic. ranges: [(sym_begin, sym_count,
    out_byte), ...]. Returns (pieces, piece_ranges, buf_bytes, seek_words): numpy structured arrays of
    PIECE_DTYPE (one per piece) and PIECE_RANGE_DTYPE (one per range), and the two totals."""
    seek = np.ascontiguousarray(seek_host, dtype=np.uint64)
    if seek.size * 8 < seek_bytes(nsym):
        raise ValueError("seek table shorter than seek_bytes(nsym)")
    rg = np.ascontiguousarray(np.array([[int(v) for v in r] for r in ranges], dtype=np.uint64).reshape(-1, 3))
    n = rg.shape[0]
    pieces = np.zeros(max(n, 1), dtype=PIECE_DTYPE)
    out = np.zeros(max(n, 1), dtype=PIECE_RANGE_DTYPE)
    np_, bb, sw = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64()
    check(load().hz_seek_pieces(seek.ctypes.data_as(ctypes.c_void_p), nsym, payload_bytes, rg.ctypes.data_as(ctypes.c_void_p),
                                n, pieces.ctypes.data_as(ctypes.c_void_p), ctypes.byref(np_),
                                out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(bb), ctypes.byref(sw)), "hz_seek_pieces")
    return pieces[:np_.value], out[:n], bb.value, sw.value


def build_seek(blob):
    """.compressed image -> its seek table (uint64 start[nblocks + 1]; bits count from the file byte
    that holds the first payload bit). Works on files the reference wrote."""
    lib = load()
    arr, p = _buf(blob)
    _, info = parse_header(_image(arr))
    seek = np.zeros(max(seek_bytes(info.n // 2) // 8, 1), dtype=np.uint64)
    nsym = ctypes.c_uint64()
    check(lib.hz_seek_build_host(p, arr.size, seek.ctypes.data_as(ctypes.c_void_p), seek.size * 8, ctypes.byref(nsym)),
          "hz_seek_build_host")
    return seek[:seek_bytes(nsym.value) // 8]


def decode_range(blob, seek, offset, length):
    """Bytes [offset, offset + length) of the original from a .compressed image and its seek table."""
    lib = load()
    arr, p = _buf(blob)
    sk = np.ascontiguousarray(seek, dtype=np.uint64)
    out = np.empty(max(length, 1), dtype=np.uint8)
    check(lib.hz_decode_range_host(p, arr.size, sk.ctypes.data_as(ctypes.c_void_p), offset, length,
                                   out.ctypes.data_as(ctypes.c_void_p)), "hz_decode_range_host")
    return out[:length].tobytes()


def seek_entries(nsym):
    """The codeword every seek entry points at: s_b = min(2048 b, nsym) for b = 0 .. nblocks(nsym); the
    last one is the stream's end. Empty for nsym 0 (seek_bytes(0) == 0)."""
    stride = 2048
    if nsym == 0:
        return []
    nb = (nsym + stride - 1) // stride
    return [min(stride * b, nsym) for b in range(nb + 1)]


def build_seek_file(path, window_bytes=256 << 20, out_path=None):
    """The seek table of a .compressed file on disk (uint64 start[nblocks + 1], as build_seek counts),
    streamed through windows of window_bytes of payload: host memory is two windows and the table,
    whatever the file's size. With out_path the file is extracted there in the same pass; without it
    nothing is decoded (hz_extract_stream_seek)."""
    lib = load()
    src = os.fsencode(path)
    dst = os.fsencode(out_path) if out_path is not None else None
    nsym = ctypes.c_uint64()
    rc = lib.hz_extract_stream_seek(src, None, window_bytes, 0, None, 0, ctypes.byref(nsym))  # the size: HZ_ECAP
    if rc not in (0, -6):
        check(rc, "hz_extract_stream_seek")
    seek = np.zeros(max(seek_bytes(nsym.value) // 8, 1), dtype=np.uint64)
    check(lib.hz_extract_stream_seek(src, dst, window_bytes, 0, seek.ctypes.data_as(ctypes.c_void_p), seek.size * 8,
                                     ctypes.byref(nsym)), "hz_extract_stream_seek")
    return seek[:seek_bytes(nsym.value) // 8]


def decode_range_file(path, seek, offset, length):
    """Bytes [offset, offset + length) of the original from a .compressed file on disk and its seek
    table: the header and the range's payload bytes are read, nothing else (hz_decode_range_file)."""
    lib = load()
    sk = np.ascontiguousarray(seek, dtype=np.uint64)
    out = np.empty(max(length, 1), dtype=np.uint8)
    check(lib.hz_decode_range_file(os.fsencode(path), sk.ctypes.data_as(ctypes.c_void_p), offset, length,
                                   out.ctypes.data_as(ctypes.c_void_p)), "hz_decode_range_file")
    return out[:length].tobytes()


def _byte_ranges(ranges):
    offs = np.array([int(o) for o, _ in ranges], dtype=np.uint64)
    cnts = np.array([int(c) for _, c in ranges], dtype=np.uint64)
    return offs, cnts, np.empty(max(int(cnts.sum()), 1), dtype=np.uint8)


def _split(out, cnts):
    ends = np.cumsum(cnts).astype(np.int64)
    return [out[int(e) - int(c):int(e)].tobytes() for e, c in zip(ends, cnts)]


def decode_ranges(blob, seek, ranges, pieces=False):
    """[(offset, length), ...] byte ranges of the original from a .compressed image and its seek table,
    decoded in one device call: a list of bytes, in the ranges' order. By default one payload slice that
    covers every range goes to the device (hz_decode_ranges_host); pieces=True sends only the bytes and
    table words each range needs, gathered (hz_decode_ranges_host_pieces)."""
    lib = load()
    arr, p = _buf(blob)
    sk = np.ascontiguousarray(seek, dtype=np.uint64)
    offs, cnts, out = _byte_ranges(ranges)
    fn, name = (lib.hz_decode_ranges_host_pieces, "hz_decode_ranges_host_pieces") if pieces else \
        (lib.hz_decode_ranges_host, "hz_decode_ranges_host")
    check(fn(p, arr.size, sk.ctypes.data_as(ctypes.c_void_p), offs.ctypes.data_as(ctypes.c_void_p),
             cnts.ctypes.data_as(ctypes.c_void_p), offs.size, out.ctypes.data_as(ctypes.c_void_p)), name)
    return _split(out, cnts)


def decode_ranges_file(path, seek, ranges):
    """[(offset, length), ...] byte ranges of the original from a .compressed file on disk and its seek
    table, in one device call from gathered pieces: the header and each piece's bytes are read, nothing
    else (hz_decode_ranges_file). A list of bytes, in the ranges' order."""
    lib = load()
    sk = np.ascontiguousarray(seek, dtype=np.uint64)
    offs, cnts, out = _byte_ranges(ranges)
    check(lib.hz_decode_ranges_file(os.fsencode(path), sk.ctypes.data_as(ctypes.c_void_p),
                                    offs.ctypes.data_as(ctypes.c_void_p), cnts.ctypes.data_as(ctypes.c_void_p), offs.size,
                                    out.ctypes.data_as(ctypes.c_void_p)), "hz_decode_ranges_file")
    return _split(out, cnts)


# ---- seekable files: the seek table and block checksums in a trailer behind the image ----------------
def block_sums_bytes(n):
    """Bytes of the block sums of n bytes: one u32 per 4096 (hz_block_sums_bytes)."""
    return load().hz_block_sums_bytes(n)


def _image(arr):
    """The .compressed image of a file's bytes: all of them, or what stands before a seekable trailer (a
    header without symbols is told from one with 65 536 by where the image ends)."""
    info = seekable_info(arr)
    return arr if info is None else arr[:info["image_bytes"]]


def _seekable_flags(sums):
    return _lib.HZ_SEEKABLE_SUMS if sums else 0


def encode_seekable(data, sums=True):
    """Bytes -> a seekable .compressed image: encode()'s bytes, then a trailer with the writer's seek table
    and (sums=True) one Adler-32 per 4 KiB block of the original. Every reader of plain files reads it."""
    lib = load()
    arr, p = _buf(data)
    n = arr.size
    need = ctypes.c_uint64()
    check(lib.hz_encoded_size(p, n, ctypes.byref(need)), "hz_encoded_size")
    flags = _seekable_flags(sums)
    out = np.empty(need.value + lib.hz_seekable_trailer_bytes(need.value, n, flags), dtype=np.uint8)
    got = ctypes.c_uint64()
    check(lib.hz_encode_host_seekable(p, n, out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(got), flags),
          "hz_encode_host_seekable")
    return out[:got.value].tobytes()


def archive_seekable(path, out_path=None, chunk_bytes=1 << 30, sums=True, verbose=False):
    """Streaming archive of path into a seekable file (default: path + ".compressed"): archive_stream()'s
    bytes, then the trailer. Returns the output's name."""
    out_path = str(path) + ".compressed" if out_path is None else out_path
    check(load().hz_archive_stream_seekable(os.fsencode(path), os.fsencode(out_path), chunk_bytes, int(verbose),
                                            _seekable_flags(sums)), "hz_archive_stream_seekable")
    return str(out_path)


def seekable_info(path_or_bytes):
    """The trailer of a file (a path) or an image (bytes): a dict of hz_seekable_info's fields, or None
    for a plain file. A trailer whose fields do not fit raises HZ_EFORMAT."""
    lib = load()
    info = _lib.SeekableInfo()
    if isinstance(path_or_bytes, (str, os.PathLike)):
        check(lib.hz_seekable_info_file(os.fsencode(path_or_bytes), ctypes.byref(info)), "hz_seekable_info_file")
    else:
        arr, _ = _buf(path_or_bytes)
        last = np.ascontiguousarray(arr[-64:]) if arr.size >= 64 else None
        check(lib.hz_seekable_footer_parse(None if last is None else last.ctypes.data_as(ctypes.c_void_p), arr.size,
                                           ctypes.byref(info)), "hz_seekable_footer_parse")
    return info.as_dict() if info.present else None


def _load_trailer(path, want_sums):
    lib = load()
    info = seekable_info(path)
    if info is None:
        raise _lib.HZError(-5, "hz_seekable_load_file")
    if want_sums and not info["flags"] & _lib.HZ_SEEKABLE_SUMS:
        return None
    seek, buf = _seek_table(info["nsym"])
    sums = np.zeros(max(info["nblocks"], 1), dtype=np.uint32)
    nsym = ctypes.c_uint64()
    check(lib.hz_seekable_load_file(os.fsencode(path), buf.ctypes.data_as(ctypes.c_void_p), buf.size * 8,
                                    sums.ctypes.data_as(ctypes.c_void_p) if want_sums else None, sums.size * 4,
                                    ctypes.byref(nsym)), "hz_seekable_load_file")
    return sums[:info["nblocks"]] if want_sums else seek


def load_seek(path):
    """The seek table (uint64) stored in a seekable file's trailer; a plain file raises HZ_EFORMAT."""
    return _load_trailer(path, False)


def load_sums(path):
    """The block sums (uint32) stored in a seekable file's trailer, or None when it was written without."""
    return _load_trailer(path, True)


def read_seekable(path_or_bytes, ranges, verify=False):
    """[(offset, length), ...] byte ranges of the original from a seekable file (a path: only the footer,
    the header, the table words and payload bytes of the ranges are read) or image (bytes), the table
    taken from its trailer: a list of bytes, in the ranges' order. verify=True checks every decoded block
    against its stored sum; a mismatch raises HZError(HZ_ECHECKSUM) with .block the smallest bad block."""
    lib = load()
    offs, cnts, out = _byte_ranges(ranges)
    flags = _lib.HZ_SEEKABLE_VERIFY if verify else 0
    bad = ctypes.c_uint64()
    tail = (offs.ctypes.data_as(ctypes.c_void_p), cnts.ctypes.data_as(ctypes.c_void_p), offs.size,
            out.ctypes.data_as(ctypes.c_void_p), flags, ctypes.byref(bad))
    if isinstance(path_or_bytes, (str, os.PathLike)):
        rc, name = lib.hz_seekable_read_file(os.fsencode(path_or_bytes), *tail), "hz_seekable_read_file"
    else:
        arr, p = _buf(path_or_bytes)
        rc, name = lib.hz_seekable_read_host(p, arr.size, *tail), "hz_seekable_read_host"
    if rc == _lib.HZ_ECHECKSUM:
        raise _lib.HZError(rc, name, block=bad.value)
    check(rc, name)
    return _split(out, cnts)


def verify_seekable(path):
    """Decode the whole of a seekable file and check every block against its stored sum (nothing is
    kept). Raises HZError(HZ_ECHECKSUM) with .block the first bad block."""
    bad = ctypes.c_uint64()
    rc = load().hz_seekable_verify_file(os.fsencode(path), ctypes.byref(bad))
    if rc == _lib.HZ_ECHECKSUM:
        raise _lib.HZError(rc, "hz_seekable_verify_file", block=bad.value)
    check(rc, "hz_seekable_verify_file")


def make_seekable(path, sums=True, window_bytes=256 << 20):
    """Make an existing .compressed file seekable in place: the trailer archive_seekable() would have written
    (the table from the index-less walk, with sums=True the block sums of the decoded rounds) is appended and
    the image's bytes stay as they are; a trailer without sums gets them when sums=True. Returns True when a
    trailer was written, False when the file already had what was asked for (hz_seekable_attach_file)."""
    attached = ctypes.c_int()
    check(load().hz_seekable_attach_file(os.fsencode(path), window_bytes, _seekable_flags(sums), ctypes.byref(attached)),
          "hz_seekable_attach_file")
    return bool(attached.value)


def extract_verified(path, out_path=None, window_bytes=256 << 20, verbose=False):
    """Streaming extract of a seekable file with sums, every block checked against its stored sum before it
    is written (out_path=None: decode and check only). A mismatch raises HZError(HZ_ECHECKSUM) with .block
    the smallest bad block; the output then holds the verified rounds before it
    (hz_extract_stream_verified)."""
    bad = ctypes.c_uint64()
    rc = load().hz_extract_stream_verified(os.fsencode(path), None if out_path is None else os.fsencode(out_path),
                                           window_bytes, int(verbose), ctypes.byref(bad))
    if rc == _lib.HZ_ECHECKSUM:
        raise _lib.HZError(rc, "hz_extract_stream_verified", block=bad.value)
    check(rc, "hz_extract_stream_verified")


def salvage(path, out_path=None, window_bytes=256 << 20, keep_unverified=False):
    """Recover what a damaged seekable file (with sums) still holds: every block is decoded from the stored
    table on its own and checked against its stored sum. Returns the list of ALL blocks that failed, ascending
    (block b is bytes [4096 b, 4096 (b + 1)) of the original); out_path receives the original with those
    blocks as zeros (keep_unverified=True: as whatever they decoded to) and its full size. out_path=None:
    scan only. A completed salvage does not raise, whatever it lost (hz_seekable_salvage_file)."""
    lib = load()
    args = (os.fsencode(path), None if out_path is None else os.fsencode(out_path), window_bytes,
            _lib.HZ_SALVAGE_KEEP_UNVERIFIED if keep_unverified else 0)
    nbad = ctypes.c_uint64()
    # room for every block (the footer alone says how many; a file the call will refuse gets one word)
    info = _lib.SeekableInfo()
    known = lib.hz_seekable_info_file(args[0], ctypes.byref(info)) == 0 and info.present
    bad = np.zeros(max(info.nblocks if known else 0, 1), dtype=np.uint64)
    check(lib.hz_seekable_salvage_file(*args, bad.ctypes.data_as(ctypes.c_void_p), bad.size, ctypes.byref(nbad)),
          "hz_seekable_salvage_file")
    return [int(b) for b in bad[:nbad.value]]


class Device:
    """Stage API on device pointers (ints), stream-ordered on one HIP stream."""

    def __init__(self, device=0, stream=None):
        self.lib = load()
        h = ctypes.c_void_p()
        check(self.lib.hz_ctx_create(device, ctypes.c_void_p(stream) if stream else None, ctypes.byref(h)),
              "hz_ctx_create")
        self.h = h

    def close(self):
        if self.h:
            self.lib.hz_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream):
        check(self.lib.hz_ctx_set_stream(self.h, ctypes.c_void_p(stream)), "hz_ctx_set_stream")

    def sync(self):
        check(self.lib.hz_ctx_sync(self.h), "hz_ctx_sync")

    def hist16(self, d_in, n, d_hist, accumulate=False):
        check(self.lib.hz_hist16(self.h, d_in, n, d_hist, int(accumulate)), "hz_hist16")

    def block_sums(self, d_in, n, d_sums):
        """One Adler-32 per 4096 bytes of d_in[0..n) (16-byte aligned), the last block zero-extended, into
        d_sums (block_sums_bytes(n) bytes): hz_block_sums."""
        check(self.lib.hz_block_sums(self.h, d_in, n, d_sums), "hz_block_sums")

    def block_sums_check(self, d_in, n, d_expect, block_base, d_bad):
        """The same sums compared with the words at d_expect: the smallest block_base + i whose block differs
        is folded (atomic minimum) into the u64 at d_bad, which the caller set (hz_block_sums_check)."""
        check(self.lib.hz_block_sums_check(self.h, d_in, n, d_expect, block_base, d_bad), "hz_block_sums_check")

    def block_sums_mark(self, d_data, n, d_expect, block_base, d_bits, flags=0):
        """The same comparison with every verdict kept: bit block_base + i of the u32 bitmap at d_bits (the
        caller's, zeroed by the caller) is set for every block that differs, and with HZ_SUMS_ZERO_BAD that
        block's bytes below n are overwritten with zeros (hz_block_sums_mark)."""
        check(self.lib.hz_block_sums_mark(self.h, d_data, n, d_expect, block_base, d_bits, flags), "hz_block_sums_mark")

    def codebook_build(self, d_hist, d_cb):
        """Device codebook: d_hist (u64 x 65536) -> d_cb (sizeof(Codebook) bytes)."""
        check(self.lib.hz_codebook_build_device(self.h, d_hist, d_cb), "hz_codebook_build_device")

    def header_write(self, d_cb, n, last_byte, d_out, cap, d_info):
        """Device header writer; d_info: 4 x u64 (bytes, pending bits, pending byte, bits)."""
        check(self.lib.hz_header_write_device(self.h, d_cb, n, last_byte, d_out, cap, d_info), "hz_header_write_device")

    def header_parse(self, d_file, length, d_cb, d_info):
        """Device header parser; d_info: 6 x u64 (n, payload byte, payload bit, odd, last, nsym)."""
        check(self.lib.hz_header_parse_device(self.h, d_file, length, d_cb, d_info), "hz_header_parse_device")

    def upload(self, cb):
        check(self.lib.hz_codebook_upload(self.h, ctypes.byref(cb)), "hz_codebook_upload")

    def upload_encode(self, cb):
        check(self.lib.hz_codebook_upload_encode(self.h, ctypes.byref(cb)), "hz_codebook_upload_encode")

    def upload_decode(self, cb):
        check(self.lib.hz_codebook_upload_decode(self.h, ctypes.byref(cb)), "hz_codebook_upload_decode")

    def pack(self, d_in, n, start_bit, lead, d_out, out_cap, d_index=None):
        check(self.lib.hz_pack(self.h, d_in, n, start_bit, lead, d_out, out_cap, d_index), "hz_pack")

    # -- two-pass encode (range plan): hist16_ranges then pack_ranges on the same input ----------
    def ranges_bytes(self, n):
        """Bytes of the range plan buffer for an n-byte input (0: too small, plain passes)."""
        return self.lib.hz_ranges_bytes(n)

    def hist16_ranges(self, d_in, n, d_hist, d_ranges, accumulate=False):
        check(self.lib.hz_hist16_ranges(self.h, d_in, n, d_hist, int(accumulate), d_ranges), "hz_hist16_ranges")

    def pack_ranges(self, d_in, n, start_bit, lead, d_out, out_cap, d_index, d_ranges):
        check(self.lib.hz_pack_ranges(self.h, d_in, n, start_bit, lead, d_out, out_cap, d_index, d_ranges),
              "hz_pack_ranges")

    def pack_seek(self, d_in, n, start_bit, lead, d_out, out_cap, d_seek, d_ranges=None, sym_base=0, bit_base=0,
                  stream_nsym=None):
        """pack (or, with d_ranges, pack_ranges) that also writes the call's seek entries into the stream's
        table d_seek: the call covers symbols [sym_base, sym_base + n // 2) of a stream of stream_nsym
        (default: n // 2); entries are bits from byte 0 of d_out plus bit_base. No block index."""
        check(self.lib.hz_pack_seek(self.h, d_in, n, start_bit, lead, d_out, out_cap, d_ranges, sym_base, bit_base,
                                    n // 2 if stream_nsym is None else stream_nsym, d_seek), "hz_pack_seek")

    def last_pack_ranges(self):
        """1 when the last pack_ranges took the range plan (no count pass), 0 for count + scan + write."""
        return self.lib.hz_last_pack_ranges(self.h)

    def decode(self, d_payload, payload_bytes, nsym, d_index, d_out):
        check(self.lib.hz_decode(self.h, d_payload, payload_bytes, nsym, d_index, d_out), "hz_decode")

    def last_decode_chunks(self):
        """Staging chunks per block the last decode prefetched (3 or 4; 0: a decoder without the choice)."""
        return self.lib.hz_last_decode_chunks(self.h)

    def index_build(self, d_payload, payload_bytes, start_bit, nsym, d_index):
        check(self.lib.hz_index_build(self.h, d_payload, payload_bytes, start_bit, nsym, d_index), "hz_index_build")

    # -- random access: seek table (the start[] words of a block index) and range decode ---------
    def seek_span(self, seek_host, nsym, sym_begin, sym_count):
        """Payload bytes (byte_begin, byte_end) a range decode of the symbols reads, margins included;
        clamp byte_end to the payload. seek_host: the stream's start[] as a host uint64 array."""
        return seek_span(seek_host, nsym, sym_begin, sym_count)

    def decode_range(self, d_payload, payload_bytes, d_seek, nsym, sym_begin, sym_count, d_out, full_index=False,
                     payload_byte_base=0):
        """Symbols [sym_begin, sym_begin + sym_count) into d_out (2-byte aligned). d_payload holds the
        payload bytes from payload_byte_base on; d_seek: the seek table, or a full block index."""
        check(self.lib.hz_decode_range(self.h, d_payload, payload_bytes, payload_byte_base, d_seek, nsym, sym_begin,
                                       sym_count, d_out, _lib.HZ_RANGE_FULL_INDEX if full_index else 0),
              "hz_decode_range")

    def decode_ranges(self, d_payload, payload_bytes, d_seek, nsym, d_ranges, nranges, d_out, out_bytes, d_stats=None,
                      full_index=False, payload_byte_base=0):
        """A batch of ranges in one call (hz_decode_ranges). d_ranges: nranges x (sym_begin, sym_count,
        out_byte) u64 on the device, range i into d_out + out_byte; d_stats: 4 u64 on the device, or None."""
        check(self.lib.hz_decode_ranges(self.h, d_payload, payload_bytes, payload_byte_base, d_seek, nsym, d_ranges,
                                        nranges, d_out, out_bytes, d_stats,
                                        _lib.HZ_RANGE_FULL_INDEX if full_index else 0), "hz_decode_ranges")

    def decode_ranges_pieces(self, d_buf, buf_bytes, d_seek, seek_words, d_pieces, npieces, nsym, d_ranges, nranges,
                             d_out, out_bytes, d_stats=None, flags=0):
        """A batch of ranges from gathered pieces (hz_decode_ranges_pieces). d_pieces: npieces x 6 u64,
        d_ranges: nranges x (sym_begin, sym_count, out_byte, piece) u64, d_seek: the compact table, all on
        the device; d_stats: 4 u64 on the device, or None."""
        check(self.lib.hz_decode_ranges_pieces(self.h, d_buf, buf_bytes, d_seek, seek_words, d_pieces, npieces, nsym,
                                               d_ranges, nranges, d_out, out_bytes, d_stats, flags),
              "hz_decode_ranges_pieces")

    def index_expand(self, d_payload, payload_bytes, d_seek, nsym, d_index):
        """Seek table -> the complete block index (d_seek may be d_index)."""
        check(self.lib.hz_index_expand(self.h, d_payload, payload_bytes, d_seek, nsym, d_index), "hz_index_expand")

    def decode_indexless(self, d_payload, payload_bytes, start_bit, nsym, d_out, d_end_bit=None):
        """Decode an index-less stream (the `extract` path): no block index; d_end_bit (device u64) gets
        the end bit of the last codeword (past payload_bytes * 8: too few codewords)."""
        check(self.lib.hz_decode_indexless(self.h, d_payload, payload_bytes, start_bit, nsym, d_out, d_end_bit),
              "hz_decode_indexless")

    # -- one index-less stream in parts (one per rank; huffman_amd/dist.py decode_indexless_split) -----
    def indexless_scan(self, d_payload, payload_bytes, start_bit, part_begin, part_end, entry_bit, d_summary,
                       nsym=0, payload_bit_base=0):
        """Walk + fix-ups of payload bits [part_begin, part_end) after start_bit; entry_bit: the part's true
        entry or 2**64 - 1 (its walked entry). d_summary (device, 3 x u64): codewords, true exit, entry in
        use. Stream bits throughout; d_payload holds stream bits from payload_bit_base (a rank's slice:
        the part plus HZ_INDEXLESS_LEAD_BITS before it). nsym: the stream's symbols (0: unknown)."""
        check(self.lib.hz_indexless_scan(self.h, d_payload, payload_bytes, payload_bit_base, start_bit, nsym,
                                         part_begin, part_end, entry_bit, d_summary), "hz_indexless_scan")

    def indexless_refix(self, entry_bit, d_summary):
        check(self.lib.hz_indexless_refix(self.h, entry_bit, d_summary), "hz_indexless_refix")

    def indexless_decode(self, nsym, d_out, d_end_bit=None):
        check(self.lib.hz_indexless_decode(self.h, nsym, d_out, d_end_bit), "hz_indexless_decode")

    # -- the seek table from the index-less walk (no block index) ------------------------------------
    def seek_build(self, d_payload, payload_bytes, start_bit, nsym, d_seek):
        """The seek table of a bare payload into d_seek (seek_bytes(nsym) bytes): nothing decoded."""
        check(self.lib.hz_seek_build(self.h, d_payload, payload_bytes, start_bit, nsym, d_seek), "hz_seek_build")

    def decode_indexless_seek(self, d_payload, payload_bytes, start_bit, nsym, d_out, d_seek, d_end_bit=None,
                              sym_base=0, bit_base=0, stream_nsym=None):
        """decode_indexless that also writes the call's seek entries into the stream's table d_seek. The
        call covers codewords [sym_base, sym_base + nsym) of a stream of stream_nsym (default: nsym);
        entries are bits from byte 0 of d_payload plus bit_base. d_out None: table only."""
        check(self.lib.hz_decode_indexless_seek(self.h, d_payload, payload_bytes, start_bit, nsym, d_out, d_end_bit,
                                                sym_base, bit_base, nsym if stream_nsym is None else stream_nsym,
                                                d_seek), "hz_decode_indexless_seek")

    def indexless_seek(self, sym_base, nsym, stream_nsym, d_seek):
        """The seek entries of the pending part (after indexless_scan / _refix): its first codeword is
        codeword sym_base of the stream, nsym its codewords; values are the scan's stream bits."""
        check(self.lib.hz_indexless_seek(self.h, sym_base, nsym, stream_nsym, d_seek), "hz_indexless_seek")

    def generate(self, d_out, n, offset=0, kind=1, alpha=1.1, seed=42):
        check(self.lib.hz_generate(self.h, d_out, n, offset, kind, alpha, seed), "hz_generate")

    def kernel_ms(self, stage):
        v = ctypes.c_float()
        check(self.lib.hz_last_kernel_ms(self.h, stage, ctypes.byref(v)), "hz_last_kernel_ms")
        return v.value
