"""Device-resident encode/decode of a byte stream (torch tensors in HBM).

This is the flow `archive` runs, kept on the device end to end so it can be
timed with inputs already resident in HBM (bench.py) and sharded across ranks
(huffman_amd/dist.py):

    hist16 (GPU, + the range plan) -> host codebook + header (reference
    semantics) -> encode table upload -> pack (GPU, one bit stream + decode-unit
    index; range starts from the plan, one pass over the input) -> decode table
    upload (host build overlaps the pack kernel) -> decode (GPU)

PyTorch provides device memory and the stream; every compute stage is a
gfx950 kernel of libhuffman_amd.so.
"""
import time
import weakref

import numpy as np
import torch

from . import _lib
from .codec import Device, block_sums_bytes, build_codebook, header_bits, index_bytes, payload_bits, seek_bytes, write_header


class Plan:
    """Codebook and stream geometry for one encode."""

    def __init__(self, cb, n_total, hist_local, first_shard=True, shard_bit_offset=0, last_byte=0):
        self.cb = cb
        self.n_total = n_total
        self.header_bits = header_bits(cb, n_total)
        self.payload_bits = payload_bits(cb, hist_local)        # bits of this shard
        # absolute payload bit where this shard starts (header pending bits first)
        self.stream_bit = self.header_bits % 8 + shard_bit_offset
        self.start_bit = self.stream_bit % 32 if not first_shard else self.stream_bit
        self.first_shard = first_shard
        self.last_byte = last_byte
        self._header = None
        # The header's last header_bits % 8 bits open the payload's first byte.
        # They are the low bits of N's top byte, the last of the 8 N bytes the
        # header ends with (Compressor.cu:487,661-669), so pack needs no header.
        pbits = self.header_bits % 8
        self.lead = ((n_total >> 56) & ((1 << pbits) - 1)) if first_shard else 0
        self.words = (self.start_bit + self.payload_bits + 31) // 32

    @property
    def header(self):
        """Complete header bytes (first shard only); written on first use, so a
        caller can launch pack/decode before paying for it on the host."""
        if self._header is None:
            self._header = b""
            if self.first_shard:
                self._header, pbits, pend = write_header(self.cb, self.n_total, self.last_byte)
                assert ((pend >> (8 - pbits)) if pbits else 0) == self.lead
        return self._header


class _PlanKey:
    """Identity of a histogram's input for its range plan: the very tensor object (a weak
    reference: a freed tensor whose address the caching allocator hands out again never matches),
    its view and its in-place version counter."""

    def __init__(self, x):
        self.ref = weakref.ref(x)
        self.key = (x.data_ptr(), x.numel(), x._version)

    def __eq__(self, other):
        if not isinstance(other, _PlanKey):
            return NotImplemented
        a, b = self.ref(), other.ref()
        return a is not None and a is b and self.key == other.key


class StreamCodec:
    def __init__(self, device_index=0, use_ranges=True):
        self.device = torch.device("cuda", device_index)
        torch.cuda.set_device(self.device)
        # A real (non-null) stream shared by torch and the library, so torch
        # ops and the HIP kernels are ordered on one queue.
        self.stream = torch.cuda.Stream(device=self.device)
        torch.cuda.set_stream(self.stream)
        self.dev = Device(device_index, stream=self.stream.cuda_stream)
        self.hist = torch.zeros(_lib.HZ_NSYM, dtype=torch.int64, device=self.device)
        self.timings = {}
        # two-pass encode (hz_hist16_ranges / hz_pack_ranges): the plan of the last histogram's input
        self.use_ranges = use_ranges
        self.ranges = None
        self._ranges_of = None

    # -- stages ---------------------------------------------------------------
    def block_sums(self, x):
        """The block checksums of a uint8 device tensor (16-byte aligned): an int32 tensor holding the u32
        words, one Adler-32 per 4096 bytes with the last block zero-extended (hz_block_sums)."""
        sums = torch.empty(block_sums_bytes(x.numel()) // 4, dtype=torch.int32, device=self.device)
        self.dev.block_sums(x.data_ptr(), x.numel(), sums.data_ptr())
        return sums

    def block_sums_check(self, x, expect, bad, block_base=0):
        """Compare the block checksums of a uint8 device tensor (16-byte aligned) with `expect` (int32, one
        word per block): the smallest block_base + i that differs is folded into bad[0] (int64 holding a
        u64; set it to -1, all ones, first). Nothing else is written (hz_block_sums_check)."""
        assert expect.numel() * 4 >= block_sums_bytes(x.numel()) and expect.element_size() == 4
        self.dev.block_sums_check(x.data_ptr(), x.numel(), expect.data_ptr(), block_base, bad.data_ptr())

    def block_sums_mark(self, x, expect, bits, block_base=0, zero_bad=False):
        """Compare the block checksums of a uint8 device tensor (16-byte aligned) with `expect` (int32, one
        word per block): bit block_base + i of the bitmap `bits` (int32 words, the caller's: zero it first,
        calls accumulate) is set for every block that differs. zero_bad=True also overwrites those blocks'
        bytes of x with zeros; a matching block is never written (hz_block_sums_mark)."""
        nblocks = block_sums_bytes(x.numel()) // 4
        assert expect.numel() >= nblocks and expect.element_size() == 4 and bits.element_size() == 4
        assert bits.numel() * 32 >= block_base + nblocks
        self.dev.block_sums_mark(x.data_ptr(), x.numel(), expect.data_ptr(), block_base, bits.data_ptr(),
                                 _lib.HZ_SUMS_ZERO_BAD if zero_bad else 0)

    def histogram(self, x, accumulate=False):
        n = x.numel()
        # the range plan needs a 16-byte aligned input (hz_hist16_ranges); offset views take hz_hist16
        aligned = x.data_ptr() % 16 == 0
        rb = self.dev.ranges_bytes(n) if self.use_ranges and not accumulate and aligned else 0
        if rb:
            if self.ranges is None or self.ranges.numel() < rb:
                self.ranges = torch.empty(rb, dtype=torch.uint8, device=self.device)
            self.dev.hist16_ranges(x.data_ptr(), n, self.hist.data_ptr(), self.ranges.data_ptr(), accumulate)
            self._ranges_of = self._ident(x)
        else:
            self.dev.hist16(x.data_ptr(), n, self.hist.data_ptr(), accumulate)
            self._ranges_of = None
        return self.hist

    @staticmethod
    def _ident(x):
        """What a range plan is valid for: the same tensor's storage, view and contents (its
        in-place version counter), so a reused address or an in-place change falls back to
        count + scan + write instead of packing with stale range starts."""
        return _PlanKey(x)

    def make_plan(self, hist_host, n_total, hist_local=None, first_shard=True, shard_bit_offset=0, last_byte=0,
                  cb=None):
        t0 = time.perf_counter()
        cb = build_codebook(hist_host) if cb is None else cb
        plan = Plan(cb, n_total, hist_host if hist_local is None else hist_local, first_shard, shard_bit_offset,
                    last_byte)
        t1 = time.perf_counter()
        self.dev.upload_encode(cb)   # decode tables follow the pack launch (upload_decode)
        t2 = time.perf_counter()
        self.timings["codebook_ms"] = (t1 - t0) * 1e3
        self.timings["upload_ms"] = (t2 - t1) * 1e3
        return plan

    def upload_decode(self, plan):
        """Decode tables; call after launching pack so the host build overlaps it."""
        t0 = time.perf_counter()
        self.dev.upload_decode(plan.cb)
        self.timings["upload_decode_ms"] = (time.perf_counter() - t0) * 1e3

    def alloc_payload(self, plan, nsym):
        out = torch.empty(max(plan.words, 1) * 4 + 16, dtype=torch.uint8, device=self.device)
        index = torch.empty(max((index_bytes(nsym) + 7) // 8, 1), dtype=torch.int64, device=self.device)
        return out, index

    def pack(self, x, plan, out, index):
        """Pack x; with the range plan of x's histogram (the last histogram() call, same tensor,
        unchanged since: stream order) in one pass over x, else count + scan + write. A plan is
        used once. index may be None: no block index is written (the drop-in file path)."""
        iptr = index.data_ptr() if index is not None else 0
        if x.data_ptr() % 16:
            # hz_pack reads 16-byte vectors (include/huffman_amd.h): an unaligned view is packed from an
            # aligned copy (its histogram took hz_hist16, so there is no range plan to match)
            x = x.clone()
        if self._ranges_of is not None and self._ranges_of == self._ident(x):
            self._ranges_of = None
            self.dev.pack_ranges(x.data_ptr(), x.numel(), plan.start_bit, plan.lead, out.data_ptr(), out.numel(),
                                 iptr, self.ranges.data_ptr())
        else:
            self.dev.pack(x.data_ptr(), x.numel(), plan.start_bit, plan.lead, out.data_ptr(), out.numel(), iptr)
        return out

    def pack_seek(self, x, plan, out, seek, sym_base=0, bit_base=0, stream_nsym=None):
        """pack() that writes the stream's seek table instead of a block index: the start bit of every
        block, known to the writer while it packs (hz_pack_seek). The range plan is used under pack()'s
        identity rule. seek: an int64 device tensor of seek_bytes(stream_nsym) // 8 entries, the table of
        the whole stream; this call covers symbols [sym_base, sym_base + x.numel() // 2) of its stream_nsym
        (default: the call's own) and writes their entries, bits from byte 0 of `out` plus bit_base."""
        nsym = x.numel() // 2
        total = nsym if stream_nsym is None else stream_nsym
        if seek.dtype != torch.int64 or not seek.is_contiguous() or seek.numel() < seek_bytes(total) // 8:
            raise ValueError("seek: a contiguous int64 tensor of seek_bytes(stream_nsym) // 8 entries")
        if x.data_ptr() % 16:
            x = x.clone()  # as pack(): 16-byte vector reads, and no range plan to match
        ranges = None
        if self._ranges_of is not None and self._ranges_of == self._ident(x):
            self._ranges_of = None
            ranges = self.ranges.data_ptr()
        self.dev.pack_seek(x.data_ptr(), x.numel(), plan.start_bit, plan.lead, out.data_ptr(), out.numel(),
                           seek.data_ptr(), ranges, sym_base, bit_base, total)
        return seek

    def decode(self, payload, nsym, index, out):
        self.dev.decode(payload.data_ptr(), payload.numel(), nsym, index.data_ptr(), out.data_ptr())
        return out

    def decode_range(self, payload, nsym, index, sym_begin, sym_count, out, full_index=True, payload_byte_base=0):
        """Symbols [sym_begin, sym_begin + sym_count) into `out` (2-byte aligned, 2 * sym_count bytes).
        index: the block index (full_index=True) or only its start[] words, the seek table;
        payload: the payload from payload_byte_base on (0: all of it, else Device.seek_span's bytes)."""
        self.dev.decode_range(payload.data_ptr(), payload.numel(), index.data_ptr(), nsym, sym_begin, sym_count,
                              out.data_ptr(), full_index, payload_byte_base)
        return out

    def decode_ranges(self, payload, nsym, index, ranges, out, stats=None, full_index=True, payload_byte_base=0):
        """A batch of ranges of one stream in one call. ranges: an int64 / uint64 device tensor of shape
        (k, 3), rows (sym_begin, sym_count, out_byte): range i goes to out[out_byte : out_byte + 2 * sym_count].
        stats: a device tensor of 4 int64 (hz_decode_ranges' d_stats), or None. The call reads `ranges`
        on the device only, so a captured graph replays with whatever the tensor holds then."""
        if ranges.dim() != 2 or ranges.shape[1] != 3 or ranges.element_size() != 8 or not ranges.is_contiguous():
            raise ValueError("ranges: a contiguous (k, 3) tensor of 64-bit integers")
        self.dev.decode_ranges(payload.data_ptr(), payload.numel(), index.data_ptr(), nsym, ranges.data_ptr(),
                               ranges.shape[0], out.data_ptr(), out.numel(), None if stats is None else stats.data_ptr(),
                               full_index, payload_byte_base)
        return out

    def decode_ranges_pieces(self, buf, seek, pieces, nsym, ranges, out, stats=None):
        """A batch of ranges from gathered pieces (hz_decode_ranges_pieces). buf: the gathered payload
        bytes (uint8, 4-byte aligned); seek: the compact table, the words the pieces name (64-bit); pieces: (k, 6) rows
        (stream_byte, bytes, buf_byte, first_block, seek_index, nblocks); ranges: (k, 4) rows (sym_begin,
        sym_count, out_byte, piece), all 64-bit device tensors that the call reads on the device only, so
        a captured graph replays with whatever they hold then. huffman_amd.seek_pieces plans them."""
        for name, t, cols in (("pieces", pieces, 6), ("ranges", ranges, 4)):
            if t.dim() != 2 or t.shape[1] != cols or t.element_size() != 8 or not t.is_contiguous():
                raise ValueError(f"{name}: a contiguous (k, {cols}) tensor of 64-bit integers")
        if seek.element_size() != 8 or not seek.is_contiguous():
            raise ValueError("seek: a contiguous tensor of 64-bit integers")
        self.dev.decode_ranges_pieces(buf.data_ptr(), buf.numel(), seek.data_ptr(), seek.numel(), pieces.data_ptr(),
                                      pieces.shape[0], nsym, ranges.data_ptr(), ranges.shape[0], out.data_ptr(),
                                      out.numel(), None if stats is None else stats.data_ptr())
        return out

    def index_expand(self, payload, nsym, seek, index):
        """The complete block index from the seek table (seek may be index itself)."""
        self.dev.index_expand(payload.data_ptr(), payload.numel(), seek.data_ptr(), nsym, index.data_ptr())
        return index

    def seek_build(self, payload, start_bit, nsym):
        """The seek table (int64 tensor, seek_bytes(nsym) / 8 entries) of a bare payload from the
        index-less walk: no block index, nothing decoded. Needs the decode tables (upload_decode)."""
        seek = torch.empty(max(seek_bytes(nsym) // 8, 1), dtype=torch.int64, device=self.device)
        self.dev.seek_build(payload.data_ptr(), payload.numel(), start_bit, nsym, seek.data_ptr())
        return seek[:seek_bytes(nsym) // 8]

    def sync(self):
        self.dev.sync()

    def kernel_ms(self):
        return {
            "hist": self.dev.kernel_ms(_lib.STAGE_HIST),
            "pack": self.dev.kernel_ms(_lib.STAGE_PACK),
            "decode": self.dev.kernel_ms(_lib.STAGE_DECODE),
        }

    # -- whole stream (one device) ----------------------------------------------
    def encode(self, x):
        """Encode a device tensor. Returns (plan, payload tensor, index tensor)."""
        n = x.numel()
        self.histogram(x)
        h = self.hist.cpu().numpy().view(np.uint64)
        last = int(x[-1].item()) if n % 2 else 0
        plan = self.make_plan(h, n, last_byte=last)
        out, index = self.alloc_payload(plan, n // 2)
        if n // 2:
            self.pack(x, plan, out, index)
        self.upload_decode(plan)
        return plan, out, index

    def file_image(self, plan, payload):
        """Complete .compressed bytes (header + payload) on the host."""
        total = plan.header_bits + plan.payload_bits
        nbytes = (total + 7) // 8 - plan.header_bits // 8
        pay = payload[:nbytes].cpu().numpy().tobytes() if nbytes else b""
        if not pay and plan.header_bits % 8:
            pay = bytes([plan.lead << (8 - plan.header_bits % 8)])
        return plan.header + pay
