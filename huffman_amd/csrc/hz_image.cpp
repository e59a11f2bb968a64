// hz_image.cpp -- the whole-buffer flows behind hz_*_host (used by the tests and the Python package): a
// complete .compressed image in host memory encoded, decoded, indexed and decoded by ranges on the
// process-wide context, device work inside.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "hz_file_io.h"
#include "hz_host.h"
#include "hz_seekable.h"
#include "hz_stream_plan.h"

using namespace hz;

namespace {

struct EncodePlan {
    std::unique_ptr<hz_codebook> cb{new hz_codebook()};
    std::vector<uint64_t> hist = std::vector<uint64_t>(HZ_NSYM);
    uint64_t header_bits = 0, payload_bits = 0;
};

// A host buffer to the process-wide context's device (din); histogram on the device, codebook on the host.
int plan_encode(const uint8_t* in, uint64_t n, hz_ctx** ctx, DevBuf& din, EncodePlan& p) {
    int rc = default_ctx(ctx);
    if (rc) return rc;
    hz_ctx* c = *ctx;
    HZ_TRY(hipSetDevice(c->device));
    if ((rc = din.alloc(n))) return rc;
    if (n) HZ_TRY(hipMemcpyAsync(din.p, in, n, hipMemcpyHostToDevice, c->stream));
    DevBuf dh;
    if ((rc = dh.alloc(HZ_NSYM * 8))) return rc;
    if ((rc = hz_hist16(c, (const uint8_t*)din.p, n, (uint64_t*)dh.p, 0))) return rc;
    HZ_TRY(hipMemcpyAsync(p.hist.data(), dh.p, HZ_NSYM * 8, hipMemcpyDeviceToHost, c->stream));
    if ((rc = hz_ctx_sync(c))) return rc;
    if ((rc = hz_codebook_build(p.hist.data(), p.cb.get()))) return rc;
    hz_header_bits(p.cb.get(), n, &p.header_bits);
    hz_payload_bits(p.cb.get(), p.hist.data(), &p.payload_bits);
    return HZ_OK;
}

// Encode a host buffer into a complete .compressed image. seek (nullable): the image's seek table from the
// writer (hz_pack_seek), hz_seek_bytes(n / 2) bytes: the pack's output starts at the file byte of the first
// payload bit, which is where the table's bits count from.
// sums (nullable): hz_block_sums' words of the input's 2 * (n / 2) symbol bytes, while it is on the device.
int encode_image(const uint8_t* in, uint64_t n, std::vector<uint8_t>& out, uint32_t* nsym_out, uint64_t* seek = nullptr,
                 std::vector<uint32_t>* sums = nullptr) {
    hz_ctx* c;
    DevBuf din;
    EncodePlan p;
    int rc = plan_encode(in, n, &c, din, p);
    if (rc) return rc;
    if (nsym_out) *nsym_out = p.cb->nsym;
    const uint64_t hbytes_full = p.header_bits / 8;
    const uint64_t total_bits = p.header_bits + p.payload_bits;
    const uint64_t file_bytes = (total_bits + 7) / 8;
    out.assign(file_bytes + 8, 0);
    uint64_t hb;
    uint32_t pend_bits;
    uint8_t pend;
    rc = hz_header_write(p.cb.get(), n, n & 1 ? in[n - 1] : 0, out.data(), out.size(), &hb, &pend_bits, &pend);
    if (rc) return rc;
    if (hb != hbytes_full) return HZ_EINVAL;
    const uint64_t nsym = n / 2;
    if (nsym > 0) {
        if ((rc = hz_codebook_upload(c, p.cb.get()))) return rc;
        const uint64_t start_bit = pend_bits;
        const uint64_t pay_bytes = file_bytes - hbytes_full;
        const uint64_t words = (start_bit + p.payload_bits + 31) / 32;
        DevBuf dout, dseek, dsums;
        if ((rc = dout.alloc(words * 4))) return rc;
        const uint32_t lead = (uint32_t)(pend >> (8 - pend_bits)) * (pend_bits ? 1 : 0);
        if (seek) {
            if ((rc = dseek.alloc(hz_seek_bytes(nsym)))) return rc;
            rc = hz_pack_seek(c, (const uint8_t*)din.p, n, start_bit, lead, (uint8_t*)dout.p, words * 4, nullptr, 0, 0, nsym,
                              (uint64_t*)dseek.p);
        } else {
            rc = hz_pack(c, (const uint8_t*)din.p, n, start_bit, lead, (uint8_t*)dout.p, words * 4, nullptr);
        }
        if (rc) return rc;
        HZ_TRY(hipMemcpyAsync(out.data() + hbytes_full, dout.p, pay_bytes, hipMemcpyDeviceToHost, c->stream));
        if (seek) HZ_TRY(hipMemcpyAsync(seek, dseek.p, hz_seek_bytes(nsym), hipMemcpyDeviceToHost, c->stream));
        if (sums) {
            const uint64_t sums_bytes = hz_block_sums_bytes(2 * nsym);
            sums->resize(sums_bytes / 4);
            if ((rc = dsums.alloc(sums_bytes))) return rc;
            if ((rc = hz_block_sums(c, (const uint8_t*)din.p, 2 * nsym, (uint32_t*)dsums.p))) return rc;
            HZ_TRY(hipMemcpyAsync(sums->data(), dsums.p, sums_bytes, hipMemcpyDeviceToHost, c->stream));
        }
        if ((rc = hz_ctx_sync(c))) return rc;
    } else if (pend_bits) {
        out[hbytes_full] = pend;  // unreachable (header is byte aligned without symbols) but kept exact
    }
    out.resize(file_bytes);
    return HZ_OK;
}

// A complete .compressed image, opened: the header parsed, the payload located. In host memory (open), or
// a file on disk (open_file) of which only the header and the payload bytes asked for are read.
struct OpenedImage {
    const uint8_t* f = nullptr;
    FileReader file{nullptr};       // open_file: the file (its reads are untimed)
    std::vector<uint8_t> head;      // open_file: its first bytes (kMaxHeaderBytes holds every header)
    // open_file: the payload bytes of the last upload. The async copy reads them until the caller's next
    // hz_ctx_sync, so an image takes ONE upload per flow (every flow here does) and outlives that sync;
    // mutable because upload() is const for the in-memory form, which needs no buffer
    mutable std::vector<uint8_t> span;
    std::unique_ptr<hz_codebook> cb{new hz_codebook()};
    hz_header_info info;
    hz_seekable_info si;  // the file's trailer (present = 0: a plain file); the image ends where it begins
    uint64_t nsym = 0;  // symbols
    uint64_t pay = 0;   // payload bytes: from info.payload_byte to the end of the image

    int open(const uint8_t* file, uint64_t len) {
        uint64_t end;
        int rc = image_end(file, len, &end, &si);
        if (rc) return rc;
        if ((rc = hz_header_parse(file, end, cb.get(), &info))) return rc;
        if (info.payload_byte > end || (si.present && si.n != info.n)) return HZ_EFORMAT;
        f = file;
        nsym = info.n / 2;
        pay = end - info.payload_byte;
        return HZ_OK;
    }
    int open_file(const char* path) {
        int rc = file.open(path);
        if (rc) return rc;
        uint64_t fsize;
        if ((rc = image_end_fd(file.fd(), file.size(), &fsize, &si))) return rc;
        head.resize(std::min<uint64_t>(fsize, kMaxHeaderBytes));
        if ((rc = read_at(head.data(), head.size(), 0))) return rc;
        if ((rc = hz_header_parse(head.data(), head.size(), cb.get(), &info))) return rc;
        if (info.payload_byte > fsize || (si.present && si.n != info.n)) return HZ_EFORMAT;
        nsym = info.n / 2;
        pay = fsize - info.payload_byte;
        return HZ_OK;
    }
    // trailer words (si.present): seek entries [first, first + count), the sums of blocks [first, first + count)
    int seek_words(uint64_t* dst, uint64_t first, uint64_t count) const {
        return bytes_at((uint8_t*)dst, 8 * count, si.seek_off + 8 * first);
    }
    int sum_words(uint32_t* dst, uint64_t first, uint64_t count) const {
        return bytes_at((uint8_t*)dst, 4 * count, si.sums_off + 4 * first);
    }
    // file bytes [off, off + n): from memory, or read from the file (these bytes and no others)
    int bytes_at(uint8_t* dst, uint64_t n, uint64_t off) const {
        if (!f) return read_at(dst, n, off);
        memcpy(dst, f + off, n);
        return HZ_OK;
    }
    // on the calling thread whatever the size (parallel piece reads are open: DESIGN.md section 10, item 6)
    int read_at(uint8_t* dst, uint64_t n, uint64_t off) const { return pread_all(file.fd(), dst, n, off); }
    // a header claiming more symbols than the payload can hold is malformed (checked before anything is allocated)
    bool holds_its_symbols() const { return payload_holds(pay, info.payload_bit, nsym, cb->min_len); }
    // payload bytes [b, e) to the device, with 16 zero bytes behind them
    int upload(hz_ctx* c, uint64_t b, uint64_t e, DevBuf& d) const {
        const int rc = d.alloc(e - b + 16);
        if (rc) return rc;
        HZ_TRY(hipMemsetAsync(d.p, 0, e - b + 16, c->stream));
        const uint8_t* src = f ? f + info.payload_byte + b : nullptr;
        if (!f) {  // from the file: these bytes and no others
            span.resize(e - b);
            const int r2 = read_at(span.data(), e - b, info.payload_byte + b);
            if (r2) return r2;
            src = span.data();
        }
        HZ_TRY(hipMemcpyAsync(d.p, src, e - b, hipMemcpyHostToDevice, c->stream));
        return HZ_OK;
    }
};

// Entries b0 .. b1 + 1 of a seek table to the device. The device reads those entries only, addressed
// from entry 0: *d_seek0 is where entry 0 would stand.
int upload_seek_slice(hz_ctx* c, const uint64_t* seek, uint64_t b0, uint64_t b1, DevBuf& d, const uint64_t** d_seek0) {
    const int rc = d.alloc(8 * (b1 - b0 + 2));
    if (rc) return rc;
    HZ_TRY(hipMemcpyAsync(d.p, seek + b0, 8 * (b1 - b0 + 2), hipMemcpyHostToDevice, c->stream));
    *d_seek0 = (const uint64_t*)d.p - b0;
    return HZ_OK;
}

// Decode a complete .compressed image.
int decode_image(const uint8_t* f, uint64_t len, std::vector<uint8_t>& out) {
    OpenedImage im;
    int rc = im.open(f, len);
    if (rc) return rc;
    if (!im.holds_its_symbols()) return HZ_EFORMAT;
    try {
        out.assign(2 * im.nsym + (im.info.is_odd ? 1 : 0), 0);
    } catch (const std::bad_alloc&) {
        return HZ_ENOMEM;
    }
    if (im.nsym > 0) {
        hz_ctx* c;
        if ((rc = default_ctx(&c))) return rc;
        HZ_TRY(hipSetDevice(c->device));
        if ((rc = hz_codebook_upload(c, im.cb.get()))) return rc;
        DevBuf dpay, didx, dout;
        if ((rc = im.upload(c, 0, im.pay, dpay))) return rc;
        if ((rc = didx.alloc(16))) return rc;
        if ((rc = dout.alloc(2 * im.nsym + 16))) return rc;
        // index-less decode (no block index); a payload with fewer than nsym codewords (truncated
        // or corrupt file) ends past the payload: rejected
        if ((rc = hz_decode_indexless(c, (const uint8_t*)dpay.p, im.pay, im.info.payload_bit, im.nsym, (uint8_t*)dout.p,
                                      (uint64_t*)didx.p)))
            return rc;
        uint64_t end_bit = 0;
        HZ_TRY(hipMemcpyAsync(&end_bit, didx.p, 8, hipMemcpyDeviceToHost, c->stream));
        if ((rc = hz_ctx_sync(c))) return rc;
        if (end_bit > im.pay * 8) return HZ_EFORMAT;
        HZ_TRY(hipMemcpyAsync(out.data(), dout.p, 2 * im.nsym, hipMemcpyDeviceToHost, c->stream));
        if ((rc = hz_ctx_sync(c))) return rc;
    }
    if (im.info.is_odd) out[2 * im.nsym] = (uint8_t)im.info.last_byte;
    return HZ_OK;
}

// The seek table of a complete .compressed image: hz_seek_build's (the index-less walk's; no block index).
int seek_build_image(const uint8_t* f, uint64_t len, uint64_t* seek, uint64_t cap_bytes, uint64_t* nsym_out) {
    OpenedImage im;
    int rc = im.open(f, len);
    if (rc) return rc;
    *nsym_out = im.nsym;
    if (im.nsym == 0) return HZ_OK;
    if (!im.holds_its_symbols()) return HZ_EFORMAT;
    if (!seek || cap_bytes < hz_seek_bytes(im.nsym)) return HZ_ECAP;
    hz_ctx* c;
    if ((rc = default_ctx(&c))) return rc;
    HZ_TRY(hipSetDevice(c->device));
    if ((rc = hz_codebook_upload_decode(c, im.cb.get()))) return rc;
    DevBuf dpay, didx;
    if ((rc = im.upload(c, 0, im.pay, dpay))) return rc;
    if ((rc = didx.alloc(hz_seek_bytes(im.nsym)))) return rc;
    if ((rc = hz_seek_build(c, (const uint8_t*)dpay.p, im.pay, im.info.payload_bit, im.nsym, (uint64_t*)didx.p))) return rc;
    HZ_TRY(hipMemcpyAsync(seek, didx.p, hz_seek_bytes(im.nsym), hipMemcpyDeviceToHost, c->stream));
    if ((rc = hz_ctx_sync(c))) return rc;
    if (seek[index_blocks(im.nsym)] > im.pay * 8) return HZ_EFORMAT;  // fewer than nsym codewords in the payload
    return HZ_OK;
}

// Bytes [offset, offset + count) of the original of an opened image, from its seek table.
int decode_range_opened(const OpenedImage& im, const uint64_t* seek, uint64_t offset, uint64_t count, uint8_t* out) {
    int rc;
    if (offset > im.info.n || count > im.info.n - offset) return HZ_EINVAL;
    if (count == 0) return HZ_OK;
    if (!out) return HZ_EINVAL;
    const uint64_t s0 = offset / 2, s1 = std::min((offset + count + 1) / 2, im.nsym);  // covering symbols
    if (s1 > s0) {
        if (!seek) return HZ_EINVAL;
        uint64_t bb, be;
        if ((rc = hz_seek_span(seek, im.nsym, s0, s1 - s0, &bb, &be))) return rc;
        if (bb >= im.pay) return HZ_EFORMAT;
        be = std::min(be, im.pay);
        const uint64_t b0 = s0 / kBlockSyms, b1 = (s1 - 1) / kBlockSyms;
        hz_ctx* c;
        if ((rc = default_ctx(&c))) return rc;
        HZ_TRY(hipSetDevice(c->device));
        if ((rc = hz_codebook_upload_decode(c, im.cb.get()))) return rc;
        DevBuf dpay, dseek, dout;
        const uint64_t* d_seek0;
        if ((rc = im.upload(c, bb, be, dpay))) return rc;
        if ((rc = upload_seek_slice(c, seek, b0, b1, dseek, &d_seek0))) return rc;
        if ((rc = dout.alloc(2 * (s1 - s0)))) return rc;
        if ((rc = hz_decode_range(c, (const uint8_t*)dpay.p, be - bb, bb, d_seek0, im.nsym, s0, s1 - s0, (uint8_t*)dout.p, 0)))
            return rc;
        std::vector<uint8_t> tmp(2 * (s1 - s0));
        HZ_TRY(hipMemcpyAsync(tmp.data(), dout.p, tmp.size(), hipMemcpyDeviceToHost, c->stream));
        if ((rc = hz_ctx_sync(c))) return rc;
        const uint64_t skip = offset - 2 * s0;
        memcpy(out, tmp.data() + skip, std::min<uint64_t>(count, tmp.size() - skip));
    }
    if (im.info.is_odd && offset + count == im.info.n) out[count - 1] = (uint8_t)im.info.last_byte;
    return HZ_OK;
}

int decode_range_image(const uint8_t* f, uint64_t len, const uint64_t* seek, uint64_t offset, uint64_t count,
                       uint8_t* out) {
    OpenedImage im;
    const int rc = im.open(f, len);
    return rc ? rc : decode_range_opened(im, seek, offset, count, out);
}

// The covering symbol ranges of byte ranges [offsets[i], offsets[i] + counts[i]) of the original, their
// symbols laid end to end in a temporary of *tmp_bytes; *total: the bytes asked for.
int byte_ranges(const OpenedImage& im, const uint64_t* offsets, const uint64_t* counts, uint32_t nranges,
                std::vector<hz_range>& rg, uint64_t* tmp_bytes, uint64_t* total) {
    rg.resize(nranges);
    *tmp_bytes = *total = 0;
    for (uint32_t i = 0; i < nranges; ++i) {
        if (offsets[i] > im.info.n || counts[i] > im.info.n - offsets[i]) return HZ_EINVAL;
        const uint64_t s0 = offsets[i] / 2, s1 = std::min((offsets[i] + counts[i] + 1) / 2, im.nsym);  // covering symbols
        rg[i].sym_begin = s0;
        rg[i].sym_count = counts[i] && s1 > s0 ? s1 - s0 : 0;
        rg[i].out_byte = *tmp_bytes;
        *tmp_bytes += 2 * rg[i].sym_count;
        *total += counts[i];
    }
    return HZ_OK;
}

// The decoded temporary to the caller: odd offsets clipped, the odd last byte from the header, list order.
void give_byte_ranges(const OpenedImage& im, const std::vector<hz_range>& rg, const std::vector<uint8_t>& tmp,
                      const uint64_t* offsets, const uint64_t* counts, uint32_t nranges, uint8_t* out) {
    uint8_t* o = out;
    for (uint32_t i = 0; i < nranges; ++i) {
        if (!counts[i]) continue;
        const uint64_t skip = offsets[i] - 2 * rg[i].sym_begin, have = 2 * rg[i].sym_count;
        if (have > skip) memcpy(o, tmp.data() + rg[i].out_byte + skip, std::min<uint64_t>(counts[i], have - skip));
        if (im.info.is_odd && offsets[i] + counts[i] == im.info.n) o[counts[i] - 1] = (uint8_t)im.info.last_byte;
        o += counts[i];
    }
}

// Byte ranges [offsets[i], offsets[i] + counts[i]) of the original, concatenated in `out`: one
// hz_decode_ranges call over one payload slice (the smallest byte_begin to the largest byte_end).
int decode_ranges_image(const uint8_t* f, uint64_t len, const uint64_t* seek, const uint64_t* offsets,
                        const uint64_t* counts, uint32_t nranges, uint8_t* out) {
    OpenedImage im;
    int rc = im.open(f, len);
    if (rc) return rc;
    if (nranges == 0) return HZ_OK;
    if (!offsets || !counts) return HZ_EINVAL;
    std::vector<hz_range> rg;
    uint64_t tmp_bytes, total, bb = UINT64_MAX, be = 0, b0 = UINT64_MAX, b1 = 0;
    if ((rc = byte_ranges(im, offsets, counts, nranges, rg, &tmp_bytes, &total))) return rc;
    for (uint32_t i = 0; i < nranges; ++i) {
        if (rg[i].sym_count) {
            if (!seek) return HZ_EINVAL;
            uint64_t rb, re;
            if ((rc = hz_seek_span(seek, im.nsym, rg[i].sym_begin, rg[i].sym_count, &rb, &re))) return rc;
            bb = std::min(bb, rb);
            be = std::max(be, re);
            b0 = std::min(b0, rg[i].sym_begin / kBlockSyms);
            b1 = std::max(b1, (rg[i].sym_begin + rg[i].sym_count - 1) / kBlockSyms);
        }
    }
    if (total && !out) return HZ_EINVAL;
    std::vector<uint8_t> tmp(tmp_bytes);
    if (tmp_bytes) {
        if (bb >= im.pay) return HZ_EFORMAT;
        be = std::min(be, im.pay);
        hz_ctx* c;
        if ((rc = default_ctx(&c))) return rc;
        HZ_TRY(hipSetDevice(c->device));
        if ((rc = hz_codebook_upload_decode(c, im.cb.get()))) return rc;
        DevBuf dpay, dseek, drg, dout;
        const uint64_t* d_seek0;
        if ((rc = im.upload(c, bb, be, dpay))) return rc;
        if ((rc = upload_seek_slice(c, seek, b0, b1, dseek, &d_seek0))) return rc;
        if ((rc = drg.alloc(sizeof(hz_range) * (uint64_t)nranges))) return rc;
        HZ_TRY(hipMemcpyAsync(drg.p, rg.data(), sizeof(hz_range) * (uint64_t)nranges, hipMemcpyHostToDevice, c->stream));
        if ((rc = dout.alloc(tmp_bytes))) return rc;
        if ((rc = hz_decode_ranges(c, (const uint8_t*)dpay.p, be - bb, bb, d_seek0, im.nsym, (const hz_range*)drg.p, nranges,
                                   (uint8_t*)dout.p, tmp_bytes, nullptr, 0)))
            return rc;
        HZ_TRY(hipMemcpyAsync(tmp.data(), dout.p, tmp_bytes, hipMemcpyDeviceToHost, c->stream));
        if ((rc = hz_ctx_sync(c))) return rc;
    }
    give_byte_ranges(im, rg, tmp, offsets, counts, nranges, out);
    return HZ_OK;
}

// One gathered batch on the device: one copy each of buffer, compact table, pieces and ranges up, one
// hz_decode_ranges_pieces into a device temporary of tmp.size() bytes, one copy back, one sync.
// sums (nullable; tmp.size() a multiple of 4096): the temporary is zero-filled first, and
// hz_block_sums' words of what the decode left there come back with it.
int run_gathered(const OpenedImage& im, const std::vector<uint8_t>& buf, const std::vector<uint64_t>& words,
                 const hz_piece* pieces, uint32_t np, const hz_piece_range* prg, uint32_t nranges,
                 std::vector<uint8_t>& tmp, std::vector<uint32_t>* sums) {
    int rc;
    hz_ctx* c;
    if ((rc = default_ctx(&c))) return rc;
    HZ_TRY(hipSetDevice(c->device));
    if ((rc = hz_codebook_upload_decode(c, im.cb.get()))) return rc;
    DevBuf dbuf, dseek, dpc, drg, dout, dsums;
    const uint64_t buf_bytes = buf.size(), seek_words = words.size(), tmp_bytes = tmp.size();
    const uint64_t pc_bytes = sizeof(hz_piece) * (uint64_t)np, rg_bytes = sizeof(hz_piece_range) * (uint64_t)nranges;
    if ((rc = dbuf.alloc(buf_bytes)) || (rc = dseek.alloc(8 * seek_words)) || (rc = dpc.alloc(pc_bytes)) ||
        (rc = drg.alloc(rg_bytes)) || (rc = dout.alloc(tmp_bytes)))
        return rc;
    HZ_TRY(hipMemcpyAsync(dbuf.p, buf.data(), buf_bytes, hipMemcpyHostToDevice, c->stream));
    HZ_TRY(hipMemcpyAsync(dseek.p, words.data(), 8 * seek_words, hipMemcpyHostToDevice, c->stream));
    HZ_TRY(hipMemcpyAsync(dpc.p, pieces, pc_bytes, hipMemcpyHostToDevice, c->stream));
    HZ_TRY(hipMemcpyAsync(drg.p, prg, rg_bytes, hipMemcpyHostToDevice, c->stream));
    if (sums) HZ_TRY(hipMemsetAsync(dout.p, 0, tmp_bytes, c->stream));
    if ((rc = hz_decode_ranges_pieces(c, (const uint8_t*)dbuf.p, buf_bytes, (const uint64_t*)dseek.p, seek_words,
                                      (const hz_piece*)dpc.p, np, im.nsym, (const hz_piece_range*)drg.p, nranges,
                                      (uint8_t*)dout.p, tmp_bytes, nullptr, 0)))
        return rc;
    if (sums) {
        sums->resize(hz_block_sums_bytes(tmp_bytes) / 4);
        if ((rc = dsums.alloc(hz_block_sums_bytes(tmp_bytes)))) return rc;
        if ((rc = hz_block_sums(c, (const uint8_t*)dout.p, tmp_bytes, (uint32_t*)dsums.p))) return rc;
        HZ_TRY(hipMemcpyAsync(sums->data(), dsums.p, hz_block_sums_bytes(tmp_bytes), hipMemcpyDeviceToHost, c->stream));
    }
    HZ_TRY(hipMemcpyAsync(tmp.data(), dout.p, tmp_bytes, hipMemcpyDeviceToHost, c->stream));
    return hz_ctx_sync(c);  // the host buffers of the copies live until here
}

// The same bytes from gathered pieces, of an image in memory or a file on disk: hz_seek_pieces' plan,
// one zeroed host buffer with each piece copied (or read) into its place, the compact table, one copy
// each of buffer, table, pieces and ranges to the device, one hz_decode_ranges_pieces, one copy back,
// one sync. Nothing of the payload outside the pieces is touched.
int decode_ranges_pieces_opened(const OpenedImage& im, const uint64_t* seek, const uint64_t* offsets,
                                const uint64_t* counts, uint32_t nranges, uint8_t* out) {
    int rc;
    if (nranges == 0) return HZ_OK;
    if (!offsets || !counts) return HZ_EINVAL;
    std::vector<hz_range> rg;
    uint64_t tmp_bytes, total;
    if ((rc = byte_ranges(im, offsets, counts, nranges, rg, &tmp_bytes, &total))) return rc;
    if (tmp_bytes && !seek) return HZ_EINVAL;
    if (total && !out) return HZ_EINVAL;
    std::vector<uint8_t> tmp(tmp_bytes);
    if (tmp_bytes) {
        std::vector<hz_piece> pieces(nranges);
        std::vector<hz_piece_range> prg(nranges);
        uint32_t np;
        uint64_t buf_bytes, seek_words;
        if ((rc = hz_seek_pieces(seek, im.nsym, im.pay, rg.data(), nranges, pieces.data(), &np, prg.data(), &buf_bytes,
                                 &seek_words)))
            return rc;
        std::vector<uint8_t> buf(buf_bytes, 0);
        std::vector<uint64_t> words(seek_words);
        for (uint32_t k = 0; k < np; ++k) {
            const hz_piece& p = pieces[k];
            if (im.f) memcpy(buf.data() + p.buf_byte, im.f + im.info.payload_byte + p.stream_byte, p.bytes);
            else if ((rc = im.read_at(buf.data() + p.buf_byte, p.bytes, im.info.payload_byte + p.stream_byte))) return rc;
            std::copy(seek + p.first_block, seek + p.first_block + p.nblocks + 1, words.begin() + p.seek_index);
        }
        if ((rc = run_gathered(im, buf, words, pieces.data(), np, prg.data(), nranges, tmp, nullptr))) return rc;
    }
    give_byte_ranges(im, rg, tmp, offsets, counts, nranges, out);
    return HZ_OK;
}

// ---- seekable files: ranges through the trailer (include/huffman_amd.h "seekable files") ----

// The seek words a read holds of a table that stays in the file: one run per range, its entries b0 .. b1 + 1.
struct SeekRuns {
    struct Run {
        uint64_t first;
        std::vector<uint64_t> w;
    };
    std::vector<Run> runs;
    const Run* find(uint64_t first, uint64_t count) const {
        for (const Run& r : runs)
            if (r.first <= first && first + count <= r.first + r.w.size()) return &r;
        return nullptr;
    }
    // (seek_pieces_by asks only for words the runs hold: entries b0 and b1 + 1 of the ranges they were read for)
    static uint64_t word(const void* arg, uint64_t i) {
        const Run* r = static_cast<const SeekRuns*>(arg)->find(i, 1);
        return r ? r->w[i - r->first] : UINT64_MAX;
    }
};

// Byte ranges of the original of an opened image with a trailer, the table read from it: per range its
// words b0 .. b1 + 1 (all hz_seek_span reads), the plan from those, then each piece's words and bytes.
// verify: every range rounded out to whole blocks, each at a 4096-aligned place of a zero-filled
// temporary, the temporary's block sums compared with the file's. discard: nothing is given to `out`.
int seekable_read_opened(const OpenedImage& im, const uint64_t* offsets, const uint64_t* counts, uint32_t nranges,
                         uint8_t* out, uint32_t flags, uint64_t* bad_block, bool discard = false) {
    int rc;
    if (!im.si.present) return HZ_EFORMAT;
    if (flags & ~HZ_SEEKABLE_VERIFY) return HZ_EINVAL;
    const bool verify = (flags & HZ_SEEKABLE_VERIFY) != 0;
    if (verify && !(im.si.flags & HZ_SEEKABLE_SUMS)) return HZ_EINVAL;
    if (nranges == 0) return HZ_OK;
    if (!offsets || !counts) return HZ_EINVAL;
    std::vector<hz_range> rg;  // the covering symbols of every range, where give_byte_ranges finds them
    uint64_t tmp_bytes, total;
    if ((rc = byte_ranges(im, offsets, counts, nranges, rg, &tmp_bytes, &total))) return rc;
    if (total && !out && !discard) return HZ_EINVAL;
    std::vector<hz_range> dec = rg;  // what the device decodes: the same, or the blocks around them
    if (verify) {
        tmp_bytes = 0;
        for (uint32_t i = 0; i < nranges; ++i) {
            if (!rg[i].sym_count) continue;
            const uint64_t s0 = rg[i].sym_begin / kBlockSyms * kBlockSyms;
            const uint64_t s1 = std::min(index_blocks(rg[i].sym_begin + rg[i].sym_count) * kBlockSyms, im.nsym);
            dec[i] = hz_range{s0, s1 - s0, tmp_bytes};
            rg[i].out_byte = tmp_bytes + 2 * (rg[i].sym_begin - s0);
            tmp_bytes += index_blocks(s1 - s0) * HZ_SUM_BLOCK_BYTES;
        }
    }
    std::vector<uint8_t> tmp(tmp_bytes);
    if (tmp_bytes) {
        SeekRuns held;
        for (uint32_t i = 0; i < nranges; ++i) {
            if (!dec[i].sym_count) continue;
            const uint64_t b0 = dec[i].sym_begin / kBlockSyms, b1 = (dec[i].sym_begin + dec[i].sym_count - 1) / kBlockSyms;
            if (held.find(b0, b1 - b0 + 2)) continue;
            held.runs.push_back({b0, std::vector<uint64_t>(b1 - b0 + 2)});
            if ((rc = im.seek_words(held.runs.back().w.data(), b0, b1 - b0 + 2))) return rc;
        }
        std::vector<hz_piece> pieces(nranges);
        std::vector<hz_piece_range> prg(nranges);
        uint32_t np;
        uint64_t buf_bytes, seek_words;
        if ((rc = seek_pieces_by(SeekRuns::word, &held, im.nsym, im.pay, dec.data(), nranges, pieces.data(), &np, prg.data(),
                                 &buf_bytes, &seek_words)))
            return rc;
        std::vector<uint8_t> buf(buf_bytes, 0);
        std::vector<uint64_t> words(seek_words);
        for (uint32_t k = 0; k < np; ++k) {
            const hz_piece& p = pieces[k];
            if ((rc = im.bytes_at(buf.data() + p.buf_byte, p.bytes, im.info.payload_byte + p.stream_byte))) return rc;
            // a piece's words: held already when one range spans it, else read (the hull of several ranges)
            if (const SeekRuns::Run* r = held.find(p.first_block, p.nblocks + 1))
                std::copy_n(r->w.begin() + (p.first_block - r->first), p.nblocks + 1, words.begin() + p.seek_index);
            else if ((rc = im.seek_words(words.data() + p.seek_index, p.first_block, p.nblocks + 1)))
                return rc;
        }
        std::vector<uint32_t> got;
        if ((rc = run_gathered(im, buf, words, pieces.data(), np, prg.data(), nranges, tmp, verify ? &got : nullptr))) return rc;
        if (verify) {
            uint64_t bad = UINT64_MAX;
            std::vector<uint32_t> want;
            for (uint32_t i = 0; i < nranges; ++i) {
                if (!dec[i].sym_count) continue;
                const uint64_t b0 = dec[i].sym_begin / kBlockSyms, nb = index_blocks(dec[i].sym_count);
                want.resize(nb);
                if ((rc = im.sum_words(want.data(), b0, nb))) return rc;
                for (uint64_t k = 0; k < nb; ++k)
                    if (want[k] != got[dec[i].out_byte / HZ_SUM_BLOCK_BYTES + k]) bad = std::min(bad, b0 + k);
            }
            if (bad != UINT64_MAX) {
                if (bad_block) *bad_block = bad;
                return HZ_ECHECKSUM;
            }
        }
    }
    if (!discard) give_byte_ranges(im, rg, tmp, offsets, counts, nranges, out);
    return HZ_OK;
}

// hz_seekable_verify_file: the verified read over the whole original, a tile of output at a time.
int seekable_verify_opened(const OpenedImage& im, uint64_t* bad_block) {
    if (!im.si.present) return HZ_EFORMAT;
    if (!(im.si.flags & HZ_SEEKABLE_SUMS)) return HZ_EINVAL;
    constexpr uint64_t kTile = 64ull << 20;
    for (uint64_t off = 0; off < im.info.n; off += kTile) {
        const uint64_t cnt = std::min(kTile, im.info.n - off);
        if (int rc = seekable_read_opened(im, &off, &cnt, 1, nullptr, HZ_SEEKABLE_VERIFY, bad_block, true)) return rc;
    }
    return HZ_OK;
}

}  // namespace

// A flow's result to the caller's buffer: its size always, its bytes when they fit.
static int give(const std::vector<uint8_t>& v, uint8_t* out, uint64_t cap, uint64_t* len) {
    *len = v.size();
    if (cap < v.size() || (!out && v.size())) return HZ_ECAP;
    if (v.size()) memcpy(out, v.data(), v.size());
    return HZ_OK;
}

extern "C" int hz_encode_host(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* out_len) {
    if ((!in && n) || !out_len) return HZ_EINVAL;
    return guarded([&]() -> int {
        std::vector<uint8_t> img;  // (never empty: the header alone is 11 bytes)
        const int rc = encode_image(in, n, img, nullptr);
        return rc ? rc : give(img, out, cap, out_len);
    });
}

extern "C" int hz_encode_host_seek(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* out_len,
                                   uint64_t* seek, uint64_t seek_cap_bytes) {
    if ((!in && n) || !out_len) return HZ_EINVAL;
    if (seek_cap_bytes < hz_seek_bytes(n / 2) || (!seek && n / 2)) return HZ_ECAP;
    return guarded([&]() -> int {
        std::vector<uint8_t> img;
        const int rc = encode_image(in, n, img, nullptr, seek);
        return rc ? rc : give(img, out, cap, out_len);
    });
}

extern "C" int hz_encoded_size(const uint8_t* in, uint64_t n, uint64_t* out_len) {
    if ((!in && n) || !out_len) return HZ_EINVAL;
    return guarded([&]() -> int {
        hz_ctx* c;
        DevBuf din;
        EncodePlan p;
        const int rc = plan_encode(in, n, &c, din, p);
        if (!rc) *out_len = (p.header_bits + p.payload_bits + 7) / 8;
        return rc;
    });
}

extern "C" int hz_decode_host(const uint8_t* file, uint64_t len, uint8_t* out, uint64_t cap, uint64_t* out_n) {
    if (!file || !out_n) return HZ_EINVAL;
    return guarded([&]() -> int {
        std::vector<uint8_t> dec;
        const int rc = decode_image(file, len, dec);
        return rc ? rc : give(dec, out, cap, out_n);
    });
}

extern "C" int hz_seek_build_host(const uint8_t* file, uint64_t len, uint64_t* seek, uint64_t cap_bytes, uint64_t* nsym) {
    if (!file || !nsym) return HZ_EINVAL;
    return guarded([&] { return seek_build_image(file, len, seek, cap_bytes, nsym); });
}

extern "C" int hz_decode_range_host(const uint8_t* file, uint64_t len, const uint64_t* seek, uint64_t offset,
                                    uint64_t count, uint8_t* out) {
    if (!file) return HZ_EINVAL;
    return guarded([&] { return decode_range_image(file, len, seek, offset, count, out); });
}

extern "C" int hz_decode_ranges_host(const uint8_t* file, uint64_t len, const uint64_t* seek, const uint64_t* offsets,
                                     const uint64_t* counts, uint32_t nranges, uint8_t* out) {
    if (!file) return HZ_EINVAL;
    return guarded([&] { return decode_ranges_image(file, len, seek, offsets, counts, nranges, out); });
}

extern "C" int hz_decode_ranges_host_pieces(const uint8_t* file, uint64_t len, const uint64_t* seek, const uint64_t* offsets,
                                            const uint64_t* counts, uint32_t nranges, uint8_t* out) {
    if (!file) return HZ_EINVAL;
    return guarded([&]() -> int {
        OpenedImage im;
        const int rc = im.open(file, len);
        return rc ? rc : decode_ranges_pieces_opened(im, seek, offsets, counts, nranges, out);
    });
}

extern "C" int hz_decode_ranges_file(const char* path, const uint64_t* seek, const uint64_t* offsets, const uint64_t* counts,
                                     uint32_t nranges, uint8_t* out) {
    if (!path) return HZ_EINVAL;
    return guarded([&]() -> int {
        OpenedImage im;
        const int rc = im.open_file(path);
        return rc ? rc : decode_ranges_pieces_opened(im, seek, offsets, counts, nranges, out);
    });
}

extern "C" int hz_decode_range_file(const char* path, const uint64_t* seek, uint64_t offset, uint64_t count, uint8_t* out) {
    if (!path) return HZ_EINVAL;
    return guarded([&]() -> int {
        OpenedImage im;
        const int rc = im.open_file(path);
        return rc ? rc : decode_range_opened(im, seek, offset, count, out);
    });
}

extern "C" int hz_encode_host_seekable(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* out_len,
                                       uint32_t flags) {
    if ((!in && n) || !out_len || (flags & ~HZ_SEEKABLE_SUMS)) return HZ_EINVAL;
    return guarded([&]() -> int {
        std::vector<uint8_t> img;
        std::vector<uint64_t> seek(hz_seek_bytes(n / 2) / 8);
        std::vector<uint32_t> sums;
        int rc = encode_image(in, n, img, nullptr, seek.data(), flags & HZ_SEEKABLE_SUMS ? &sums : nullptr);
        if (rc) return rc;
        const uint64_t image_bytes = img.size();
        uint64_t len = hz_seekable_trailer_bytes(image_bytes, n, flags);
        if (!len) return HZ_EINVAL;
        img.resize(image_bytes + len);
        rc = hz_seekable_trailer_write(image_bytes, n, seek.data(), sums.data(), flags, img.data() + image_bytes, len, &len);
        return rc ? rc : give(img, out, cap, out_len);
    });
}

extern "C" int hz_seekable_read_host(const uint8_t* file, uint64_t len, const uint64_t* offsets, const uint64_t* counts,
                                     uint32_t nranges, uint8_t* out, uint32_t flags, uint64_t* bad_block) {
    if (!file) return HZ_EINVAL;
    return guarded([&]() -> int {
        OpenedImage im;
        const int rc = im.open(file, len);
        return rc ? rc : seekable_read_opened(im, offsets, counts, nranges, out, flags, bad_block);
    });
}

extern "C" int hz_seekable_read_file(const char* path, const uint64_t* offsets, const uint64_t* counts, uint32_t nranges,
                                     uint8_t* out, uint32_t flags, uint64_t* bad_block) {
    if (!path) return HZ_EINVAL;
    return guarded([&]() -> int {
        OpenedImage im;
        const int rc = im.open_file(path);
        return rc ? rc : seekable_read_opened(im, offsets, counts, nranges, out, flags, bad_block);
    });
}

extern "C" int hz_seekable_verify_file(const char* path, uint64_t* bad_block) {
    if (!path) return HZ_EINVAL;
    return guarded([&]() -> int {
        OpenedImage im;
        const int rc = im.open_file(path);
        return rc ? rc : seekable_verify_opened(im, bad_block);
    });
}
