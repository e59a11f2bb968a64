// hz_stream.cpp -- the file-level `archive` / `extract` flows (Compressor.cu:315-632,
// Decompressor.cu:47-114), streamed through bounded host and device memory on the process-wide context,
// and the flows of seekable files that walk a whole file the same way (attach, verified extract, salvage).
// Each flow is a struct with one function per step; its file I/O is hz_file_io.cpp and its chunk and
// window arithmetic hz_stream_plan.h and hz_salvage_plan.h, all free of HIP calls.
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "hz_file_io.h"
#include "hz_host.h"
#include "hz_salvage_plan.h"
#include "hz_seekable.h"
#include "hz_stream_plan.h"

using namespace hz;

static_assert(kPlanBlockSyms == (uint64_t)kBlockSyms, "hz_stream_plan.h counts in the kernels' blocks");
static_assert(kSalvageBlockSyms == (uint64_t)kBlockSyms, "hz_salvage_plan.h counts in the kernels' blocks");

namespace {

struct PinnedBuf {
    uint8_t* p = nullptr;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    int alloc(size_t n) { return hipHostMalloc(&p, n ? n : 16, hipHostMallocDefault) == hipSuccess ? HZ_OK : HZ_ENOMEM; }
};

constexpr uint64_t kArchiveChunk = 256ull << 20;  // archive: 256 MiB per streamed chunk (~1.2 GB pinned)
constexpr uint64_t kExtractWindow = 256ull << 20; // extract: 256 MiB payload windows (16 GiB: 1.9 s vs 2.6 s at 512 MiB, 3.2 s at 128)

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

thread_local hz_stream_timing g_timing;  // the calling thread's last streamed call

// Device busy time per stage: an event pair around each copy or kernel
// launch (events are never shared between spans), folded into its stage once
// the end event has completed.
class Spans {
  public:
    ~Spans() {
        for (auto& s : open_) {
            (void)hipEventDestroy(s.a);
            (void)hipEventDestroy(s.b);
        }
        for (auto e : free_) (void)hipEventDestroy(e);
    }
    // body()'s device work on st, timed into *acc. Whatever body returns, no event is lost.
    template <typename F>
    int timed(hipStream_t st, double* acc, F&& body) {
        const hipEvent_t a = mark(st);
        const int rc = body();
        add(a, rc ? nullptr : mark(st), acc);
        return rc;
    }
    // one copy on st, timed into *acc
    int copy(hipStream_t st, double* acc, void* dst, const void* src, size_t n, hipMemcpyKind kind) {
        return timed(st, acc, [&]() -> int {
            HZ_TRY(hipMemcpyAsync(dst, src, n, kind, st));
            return HZ_OK;
        });
    }
    void fold() {
        for (size_t i = 0; i < open_.size();) {
            if (hipEventQuery(open_[i].b) != hipSuccess) { ++i; continue; }
            float ms = 0;
            if (hipEventElapsedTime(&ms, open_[i].a, open_[i].b) == hipSuccess) *open_[i].acc += ms;
            free_.push_back(open_[i].a);
            free_.push_back(open_[i].b);
            open_[i] = open_.back();
            open_.pop_back();
        }
    }
  private:
    hipEvent_t mark(hipStream_t st) {
        hipEvent_t e = nullptr;
        if (!free_.empty()) {
            e = free_.back();
            free_.pop_back();
        } else if (hipEventCreate(&e) != hipSuccess) {
            return nullptr;
        }
        if (hipEventRecord(e, st) != hipSuccess) {
            free_.push_back(e);
            return nullptr;
        }
        return e;
    }
    void add(hipEvent_t a, hipEvent_t b, double* acc) {
        if (a && b) open_.push_back({a, b, acc});
        else {
            if (a) free_.push_back(a);
            if (b) free_.push_back(b);
        }
    }
    struct Span { hipEvent_t a, b; double* acc; };
    std::vector<Span> open_;
    std::vector<hipEvent_t> free_;
};

// The guards of a flow. MEMBER ORDER CARRIES THE LIFETIME RULES of the two flow structs below: members
// are destroyed last to first, so every host or device buffer that an async copy or a writer thread
// touches (pinned and device buffers, hist, cb, head, the info words, end_bit, the lead word) is declared
// BEFORE the guard that waits for that work. The FileWriter joins its writer threads when it is destroyed
// and stands after the pinned buffers they read; the DrainGuard and the StreamGuard synchronise their
// streams and stand after everything a copy reads or writes. An early return from any step therefore
// waits for the work in flight before a byte it touches is freed.
struct StreamGuard {  // a stream of the flow's own
    hipStream_t s = nullptr;
    ~StreamGuard() {
        if (s) {
            (void)hipStreamSynchronize(s);  // no copy may outlive the buffers it targets
            (void)hipStreamDestroy(s);
        }
    }
};

struct DrainGuard {  // the context's stream, once the flow has a context
    hipStream_t s = nullptr;
    ~DrainGuard() { if (s) (void)hipStreamSynchronize(s); }
};

struct EventPair {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~EventPair() {
        for (auto x : e)
            if (x) (void)hipEventDestroy(x);
    }
    int create(bool timing = false) {
        for (auto& x : e)
            if (hipEventCreateWithFlags(&x, timing ? hipEventDefault : hipEventDisableTiming) != hipSuccess) return HZ_EHIP;
        return HZ_OK;
    }
};

// Where a streamed call leaves the file's seek table (hz_archive_stream_seek, hz_extract_stream_seek).
struct SeekSink {
    uint64_t* seek;      // host, cap_bytes
    uint64_t cap_bytes;
    uint64_t* nsym;      // out: the file's symbols
};

// The process-wide context, its creation counted as allocation.
int timed_default_ctx(hz_ctx** c) {
    const auto tc = Clock::now();
    const int rc = default_ctx(c);
    g_timing.alloc_ms += ms_since(tc);
    if (rc) return rc;
    HZ_TRY(hipSetDevice((*c)->device));
    return HZ_OK;
}

// The flow's device seek table to the sink, once.
int table_out(Spans& spans, hz_ctx* c, const SeekSink* sink, const DevBuf& dseek, uint64_t nsym) {
    if (!sink || !nsym) return HZ_OK;
    const int rc = spans.copy(c->stream, &g_timing.d2h_ms, sink->seek, dseek.p, hz_seek_bytes(nsym), hipMemcpyDeviceToHost);
    return rc ? rc : hz_ctx_sync(c);
}

// ---- streaming archive: bounded host and device memory ----
// Pass 1 reads the file in chunks and accumulates the histogram on the device;
// pass 2 packs chunk by chunk at the running bit offset. Each chunk's last,
// partial word is carried into the next chunk as its `lead` bits, so the file
// is byte-identical to the whole-buffer encoder's. Double-buffered pinned and
// device buffers keep the host's read of chunk k + 1 and write of chunk
// k - 1 beside the device's upload and pack of chunk k, and the copy-out of
// chunk k runs on a second stream beside the upload and pack of chunk k + 1.
//
// resident: keep the input on the device after pass 1 when the file fits
// (hz_archive_file; Compressor.cu:324-367 reads the file once into pinned
// memory), so pass 2 packs it in one launch without reading the file again.
//
// With a SeekSink the writer also leaves the file's seek table (hz_archive_stream_seek): every pack is
// hz_pack_seek at sym_base = the symbols packed and bit_base = 8 x the payload bytes handed to the file
// writer (the pack's output starts at the file byte of the first payload bit, which is where the table's
// bits count from), into one device table copied out once at the end. Chunks are whole blocks, and a
// chunk's end bit comes back from the table: no per-chunk block index.
//
// seekable >= 0 (hz_archive_stream_seekable, its flags): the flow is its own sink and puts the table behind
// the image as a trailer (hz_seekable.h). With HZ_SEEKABLE_SUMS every chunk's hz_block_sums follows its pack
// on the same device bytes: chunks are whole blocks, so chunk k's words stand at block off / 4096 of one
// device array, copied out once at the end like the table.
struct ArchiveFlow {
    const char* in_path;
    const char* out_path;
    uint64_t chunk_bytes;
    int verbose;
    bool resident;
    const SeekSink* sink;
    int seekable = -1;

    hz_ctx* c = nullptr;
    uint64_t n = 0, nsym_total = 0;
    ArchiveChunks ch{64, false, 0};
    uint8_t last_byte = 0;
    Clock::time_point t_hist, t_enc;
    uint64_t hbits = 0, pbits = 0;
    uint64_t hb = 0;         // the header's whole bytes
    uint32_t pend_bits = 0;  // and the bits behind them, in pend's high bits: the payload starts in that byte
    uint8_t pend = 0;
    uint64_t written = 0;
    // pass 2, streamed: the carry between chunks and the chunk waiting for its write
    uint64_t out_cap = 0;
    uint32_t sbit = 0, lead = 0;
    int wbuf = -1;
    uint64_t wbytes = 0;
    uint64_t emitted = 0;  // payload bytes of the chunks before this one

    // buffers first, guards last (see StreamGuard)
    FileReader fin{&g_timing};
    Spans spans;
    PinnedBuf hin[2], hout[2];
    DevBuf din[2], dhist, dall, dcb, dhead, dinfo, dpay, dseek, dsums, dout[2], didx;
    std::vector<uint64_t> hist = std::vector<uint64_t>(HZ_NSYM);
    std::vector<uint64_t> table;  // seekable: the trailer's table and sums, and the sink that fills the table
    std::vector<uint32_t> sums;
    uint64_t own_nsym = 0;
    SeekSink own_sink{nullptr, 0, nullptr};
    std::unique_ptr<hz_codebook> cb{new hz_codebook()};
    std::vector<uint8_t> head;
    uint64_t dinfo_h[4] = {0, 0, 0, 0};
    uint64_t end_bit = 0;
    uint32_t lead_word = 0;
    EventPair done, cbt, packed, copied;
    FileWriter fout{&g_timing};
    DrainGuard drain;
    StreamGuard cs;  // copy-out stream

    // the codebook is built on the device from the device histogram (k_cb_*, 0.26 ms for
    // U = 65 536 against 0.43 ms on the host plus the histogram's D2H; profiles/r03_codebook_*);
    // HZ_HOST_CODEBOOK=1 builds it on the host instead. Both are bit-exact with GenerateCL.
    // And so is the header (k_hw_*, 0.014 ms against 0.25 ms on the host).
    static bool host_codebook() {
        static const bool on = [] { const char* v = getenv("HZ_HOST_CODEBOOK"); return v && v[0] == '1'; }();
        return on;
    }

    bool with_sums() const { return seekable >= 0 && ((uint32_t)seekable & HZ_SEEKABLE_SUMS); }
    uint64_t image_bytes() const { return (hbits + pbits + 7) / 8; }

    int open_and_size() {
        if (!in_path || !out_path || chunk_bytes < 64) return HZ_EINVAL;
        if (sink && !sink->nsym) return HZ_EINVAL;
        int rc = fin.open(in_path);
        if (rc) return rc;
        n = fin.size();
        nsym_total = n / 2;
        if (seekable >= 0) {
            if ((uint32_t)seekable & ~HZ_SEEKABLE_SUMS) return HZ_EINVAL;
            table.resize(hz_seek_bytes(nsym_total) / 8);
            if (with_sums()) sums.resize(hz_block_sums_bytes(2 * nsym_total) / 4);
            own_sink = SeekSink{table.data(), 8 * table.size(), &own_nsym};
            sink = &own_sink;
        }
        ch = ArchiveChunks(chunk_bytes, sink != nullptr, n);
        if (sink) {
            *sink->nsym = n / 2;
            if (sink->cap_bytes < hz_seek_bytes(n / 2) || (!sink->seek && n / 2)) return HZ_ECAP;
        }
        return HZ_OK;
    }

    int allocate() {
        int rc = timed_default_ctx(&c);
        if (rc) return rc;
        drain.s = c->stream;
        const auto ta = Clock::now();
        if (resident && n > ch.chunk) {
            // the whole input plus a payload of the same size must fit in free device memory
            size_t fr = 0, tot = 0;
            resident = hipMemGetInfo(&fr, &tot) == hipSuccess && 2 * n + (1ull << 30) <= fr && dall.alloc(n + 16) == HZ_OK;
        } else {
            resident = false;
        }
        for (int i = 0; i < 2; ++i) {
            if ((rc = hin[i].alloc(ch.chunk))) return rc;
            if (!resident && (rc = din[i].alloc(ch.chunk + 16))) return rc;
        }
        if ((rc = dhist.alloc(HZ_NSYM * 8))) return rc;
        g_timing.alloc_ms += ms_since(ta);
        return HZ_OK;
    }

    // ---- pass 1: histogram (resident: the chunks stay in dall)
    int histogram_pass() {
        int rc;
        t_hist = Clock::now();  // "Histograming took" (Compressor.cu:395-399): read + upload + histogram
        HZ_TRY(hipMemsetAsync(dhist.p, 0, HZ_NSYM * 8, c->stream));
        if ((rc = done.create())) return rc;
        for (uint64_t off = 0, k = 0; off < n; off += ch.chunk, ++k) {
            const uint64_t len = std::min(ch.chunk, n - off);
            const int b = (int)(k & 1);
            if (k >= 2) HZ_TRY(hipEventSynchronize(done.e[b]));  // buffer b's previous chunk is consumed
            spans.fold();
            if ((rc = fin.read(hin[b].p, len, off))) return rc;
            if (off + len == n && (n & 1)) last_byte = hin[b].p[len - 1];
            uint8_t* dst = resident ? (uint8_t*)dall.p + off : (uint8_t*)din[b].p;
            if ((rc = spans.copy(c->stream, &g_timing.h2d_ms, dst, hin[b].p, len, hipMemcpyHostToDevice))) return rc;
            rc = spans.timed(c->stream, &g_timing.kernel_ms, [&] { return hz_hist16(c, dst, len, (uint64_t*)dhist.p, 1); });
            if (rc) return rc;
            HZ_TRY(hipEventRecord(done.e[b], c->stream));
        }
        return HZ_OK;
    }

    // The device codebook and header, launched; cbt brackets "construction time"
    // (gpuHuffmanConstruction.h:776-782): the device codebook.
    int device_codebook() {
        int rc;
        if ((rc = dcb.alloc(sizeof(hz_codebook))) || (rc = dhead.alloc(kMaxHeaderBytes)) || (rc = dinfo.alloc(4 * 8))) return rc;
        head.resize(kMaxHeaderBytes);
        return spans.timed(c->stream, &g_timing.kernel_ms, [&]() -> int {
            HZ_TRY(hipEventRecord(cbt.e[0], c->stream));
            if (int r2 = hz_codebook_build_device(c, (const uint64_t*)dhist.p, (hz_codebook*)dcb.p)) return r2;
            HZ_TRY(hipEventRecord(cbt.e[1], c->stream));
            return hz_header_write_device(c, (const hz_codebook*)dcb.p, n, last_byte, (uint8_t*)dhead.p, kMaxHeaderBytes,
                                          (uint64_t*)dinfo.p);
        });
    }

    // What hz_header_write_device leaves in its four info words.
    int header_from_info_words() {
        hb = dinfo_h[0];
        pend_bits = (uint32_t)dinfo_h[1];
        pend = (uint8_t)dinfo_h[2];
        return dinfo_h[3] != hbits ? HZ_EFORMAT : HZ_OK;  // the device writer disagrees with the header length
    }

    int codebook_and_header() {
        int rc;
        const bool host_cb = host_codebook();
        if ((rc = cbt.create(true))) return rc;
        if (!host_cb && (rc = device_codebook())) return rc;
        rc = spans.timed(c->stream, &g_timing.d2h_ms, [&]() -> int {
            HZ_TRY(hipMemcpyAsync(hist.data(), dhist.p, HZ_NSYM * 8, hipMemcpyDeviceToHost, c->stream));
            if (!host_cb) {
                HZ_TRY(hipMemcpyAsync(cb.get(), dcb.p, sizeof(hz_codebook), hipMemcpyDeviceToHost, c->stream));
                HZ_TRY(hipMemcpyAsync(dinfo_h, dinfo.p, sizeof(dinfo_h), hipMemcpyDeviceToHost, c->stream));
                HZ_TRY(hipMemcpyAsync(head.data(), dhead.p, kMaxHeaderBytes, hipMemcpyDeviceToHost, c->stream));
            }
            return HZ_OK;
        });
        if (rc) return rc;
        if ((rc = hz_ctx_sync(c))) return rc;
        const double hist_ms = ms_since(t_hist);
        const auto th = Clock::now();
        if (host_cb && (rc = hz_codebook_build(hist.data(), cb.get()))) return rc;
        float cb_ms = 0.0f;
        if (host_cb) cb_ms = (float)ms_since(th);
        else HZ_TRY(hipEventElapsedTime(&cb_ms, cbt.e[0], cbt.e[1]));
        hz_header_bits(cb.get(), n, &hbits);
        hz_payload_bits(cb.get(), hist.data(), &pbits);
        if (verbose) {  // the reference's stdout lines, its stage timers included
            std::cout << "The size of the sum of ORIGINAL files is: " << n << " bytes" << std::endl;
            std::cout << "Unique symbols count: " << cb->nsym << std::endl;
            std::cout << "Histograming took " << hist_ms << " ms" << std::endl;
            printf("construction time: %.3f ms, symbols/s: %.3f\n", cb_ms,
                   cb_ms > 0 ? (float)cb->nsym / (cb_ms * 1e-3f) : 0.0f);
            fflush(stdout);
        }
        t_enc = Clock::now();  // "Encoding took" (Compressor.cu:588-593): header, pack, payload out
        if (host_cb) {
            head.resize(hbits / 8 + 8);
            rc = hz_header_write(cb.get(), n, last_byte, head.data(), head.size(), &hb, &pend_bits, &pend);
        } else {
            rc = header_from_info_words();
        }
        if (rc) return rc;
        g_timing.host_ms += ms_since(th);
        return HZ_OK;
    }

    int open_output() {
        int rc;
        if ((rc = fout.open(out_path))) return rc;
        fout.reserve(hb + (pend_bits + pbits + 7) / 8 +
                     (seekable >= 0 ? hz_seekable_trailer_bytes(image_bytes(), n, (uint32_t)seekable) : 0));
        if ((rc = fout.write_now(head.data(), hb, 0))) return rc;
        written = hb;
        lead = pend_bits ? (uint32_t)(pend >> (8 - pend_bits)) : 0u;
        if (sink && nsym_total && (rc = dseek.alloc(hz_seek_bytes(nsym_total)))) return rc;
        if (!sums.empty() && (rc = dsums.alloc(4 * sums.size()))) return rc;
        return HZ_OK;
    }

    int upload_codebook() {
        const auto tu = Clock::now();
        const int rc = hz_codebook_upload_encode(c, cb.get());
        if (!rc) g_timing.host_ms += ms_since(tu);
        return rc;
    }

    // One pack of `len` input bytes whose first code lands at bit `start` of d_out's first word; with a
    // sink, the table's entries too (sym_base: the symbols before; bit_base: the payload bits before d_out).
    int pack_call(const void* d_in, uint64_t len, uint32_t start, void* d_out, uint64_t cap, uint64_t* d_index,
                  uint64_t sym_base, uint64_t bit_base) {
        return spans.timed(c->stream, &g_timing.kernel_ms, [&]() -> int {
            if (!sink) return hz_pack(c, (const uint8_t*)d_in, len, start, lead, (uint8_t*)d_out, cap, d_index);
            const int rc = hz_pack_seek(c, (const uint8_t*)d_in, len, start, lead, (uint8_t*)d_out, cap, nullptr, sym_base,
                                        bit_base, nsym_total, (uint64_t*)dseek.p);
            if (rc || sums.empty()) return rc;
            // the call's symbols begin a block (hz_pack_seek: sym_base is a multiple of 2048)
            return hz_block_sums(c, (const uint8_t*)d_in, len & ~(uint64_t)1, (uint32_t*)dsums.p + sym_base / kBlockSyms);
        });
    }

    // ---- pass 2, resident: one pack launch over the whole input, then the payload
    // leaves in chunks (copy-out double-buffered against the parallel file writes).
    // No room for the payload beside the input: resident is dropped and pass 2 streams from the file.
    int pack_resident() {
        int rc;
        const uint64_t pay_bytes = (pend_bits + pbits + 7) / 8;
        const uint64_t cap = ((pend_bits + pbits + 31) / 32 + 1) * 4;
        const auto tb = Clock::now();
        resident = dpay.alloc(cap) == HZ_OK;
        g_timing.alloc_ms += ms_since(tb);
        if (!resident) {
            (void)hipFree(dall.p);
            dall.p = nullptr;
            return HZ_OK;
        }
        if ((rc = upload_codebook())) return rc;
        if ((rc = pack_call(dall.p, 2 * nsym_total, pend_bits, dpay.p, cap, nullptr, 0, 0))) return rc;
        for (uint64_t off = 0, k = 0; off < pay_bytes; off += ch.chunk, ++k) {
            const int b = (int)(k & 1);
            const uint64_t len = std::min(ch.chunk, pay_bytes - off);
            rc = spans.copy(c->stream, &g_timing.d2h_ms, hin[b].p, (const uint8_t*)dpay.p + off, len, hipMemcpyDeviceToHost);
            if (rc) return rc;
            HZ_TRY(hipEventRecord(done.e[b], c->stream));
            HZ_TRY(hipEventSynchronize(done.e[b]));
            if ((rc = hz_ctx_sync(c))) return rc;
            spans.fold();
            if ((rc = fout.wait())) return rc;  // the write of chunk k - 1 (buffer 1 - b)
            fout.start(hin[b].p, len, written);
            written += len;
        }
        return HZ_OK;
    }

    // The chunk that waits for its write goes to the writer once its copy-out is done.
    int hand_to_writer() {
        if (wbuf < 0) return HZ_OK;
        HZ_TRY(hipEventSynchronize(copied.e[wbuf]));
        if (int rc = fout.wait()) return rc;  // the other hout is free again after this
        fout.start(hout[wbuf].p, wbytes, written);
        written += wbytes;
        wbuf = -1;
        return HZ_OK;
    }

    // ---- pass 2: pack chunk by chunk at the running bit offset
    int pack_streamed() {
        int rc;
        const uint64_t body = 2 * nsym_total;  // the odd last byte travels in the header
        if ((rc = upload_codebook())) return rc;
        out_cap = ch.out_cap(cb->max_len);
        const auto tb = Clock::now();
        for (int i = 0; i < 2; ++i) {
            if (!din[i].p && (rc = din[i].alloc(ch.chunk + 16))) return rc;
            if ((rc = dout[i].alloc(out_cap))) return rc;
            if ((rc = hout[i].alloc(out_cap))) return rc;
        }
        if (!sink && (rc = didx.alloc(hz_index_bytes(ch.chunk / 2)))) return rc;
        g_timing.alloc_ms += ms_since(tb);
        HZ_TRY(hipStreamCreateWithFlags(&cs.s, hipStreamNonBlocking));
        if ((rc = packed.create()) || (rc = copied.create())) return rc;
        sbit = pend_bits;  // bit of the chunk's first code in its first word
        if ((rc = fin.read(hin[0].p, std::min(ch.chunk, body), 0))) return rc;
        for (uint64_t off = 0, k = 0; off < body; off += ch.chunk, ++k)
            if ((rc = pack_chunk(off, k, body))) return rc;
        if ((rc = hand_to_writer())) return rc;
        if ((rc = fout.wait())) return rc;
        HZ_TRY(hipStreamSynchronize(cs.s));
        return HZ_OK;
    }

    // Chunk k: upload and pack on the context's stream, the host's write of chunk k - 1 and read of
    // chunk k + 1 beside them, then the carry into chunk k + 1 and the copy-out on the second stream.
    int pack_chunk(uint64_t off, uint64_t k, uint64_t body) {
        int rc;
        const int b = (int)(k & 1);
        const uint64_t len = std::min(ch.chunk, body - off);
        if ((rc = spans.copy(c->stream, &g_timing.h2d_ms, din[b].p, hin[b].p, len, hipMemcpyHostToDevice))) return rc;
        if (k >= 2) HZ_TRY(hipStreamWaitEvent(c->stream, copied.e[b], 0));  // dout[b] copied out
        if ((rc = pack_call(din[b].p, len, sbit, dout[b].p, out_cap, (uint64_t*)didx.p, off / 2, 8 * emitted))) return rc;
        HZ_TRY(hipEventRecord(packed.e[b], c->stream));
        const uint64_t nb = (len / 2 + 2047) / 2048;
        // the chunk's end: the index's last start[] word or, in the table, the entry after its last block
        const uint64_t* d_end = sink ? (const uint64_t*)dseek.p + off / 2 / kBlockSyms + nb : (const uint64_t*)didx.p + nb;
        HZ_TRY(hipMemcpyAsync(&end_bit, d_end, 8, hipMemcpyDeviceToHost, c->stream));
        // host work beside the upload and pack: the previous chunk's write, the next chunk's read
        if ((rc = hand_to_writer())) return rc;
        const uint64_t next = off + len;
        if (next < body && (rc = fin.read(hin[1 - b].p, std::min(ch.chunk, body - next), next))) return rc;
        if ((rc = hz_ctx_sync(c))) return rc;
        spans.fold();
        if (sink) end_bit -= 8 * emitted;  // the table counts from the payload's first byte
        const ArchiveChunks::Carry carry = ArchiveChunks::carry_after(end_bit, next >= body);
        sbit = carry.sbit;
        lead = 0;
        if (carry.needs_lead) {
            HZ_TRY(hipMemcpyAsync(&lead_word, (const uint8_t*)dout[b].p + carry.bytes, 4, hipMemcpyDeviceToHost, c->stream));
            if ((rc = hz_ctx_sync(c))) return rc;
            lead = __builtin_bswap32(lead_word) >> (32 - sbit);
        }
        if ((rc = fout.wait())) return rc;  // hout[b] may still be leaving from two chunks back
        HZ_TRY(hipStreamWaitEvent(cs.s, packed.e[b], 0));
        rc = spans.timed(cs.s, &g_timing.d2h_ms, [&]() -> int {
            if (carry.bytes) HZ_TRY(hipMemcpyAsync(hout[b].p, dout[b].p, carry.bytes, hipMemcpyDeviceToHost, cs.s));
            return HZ_OK;
        });
        if (rc) return rc;
        HZ_TRY(hipEventRecord(copied.e[b], cs.s));
        wbuf = b;
        wbytes = carry.bytes;
        emitted += carry.bytes;
        return HZ_OK;
    }

    // The trailer behind the image, in hz_seekable_trailer_write's layout: the table and the sums leave from
    // the vectors that hold them (no second copy of either), the padding and the footer around them.
    int write_trailer() {
        int rc;
        if (!sums.empty()) {
            rc = spans.copy(c->stream, &g_timing.d2h_ms, sums.data(), dsums.p, 4 * sums.size(), hipMemcpyDeviceToHost);
            if (rc || (rc = hz_ctx_sync(c))) return rc;
        }
        if (written != image_bytes()) return HZ_EFORMAT;
        const SeekableLayout l = seekable_layout(written, n, (uint32_t)seekable);
        if (!l.ok || l.seek_bytes != 8 * table.size() || l.sums_bytes != 4 * sums.size()) return HZ_EINVAL;
        const uint64_t sums_at = l.seek_off + l.seek_bytes, tail_off = sums_at + l.sums_bytes;
        const uint64_t tail_len = l.file_bytes - tail_off;  // under 8 bytes of padding, then the footer
        uint8_t pad[8] = {0}, tail[8 + HZ_SEEKABLE_FOOTER_BYTES] = {0};
        if ((rc = seekable_footer(written, n, (uint32_t)seekable, tail + tail_len - HZ_SEEKABLE_FOOTER_BYTES))) return rc;
        if ((rc = fout.write_now(pad, l.seek_off - written, written)) ||
            (rc = fout.write_now((const uint8_t*)table.data(), l.seek_bytes, l.seek_off)) ||
            (rc = fout.write_now((const uint8_t*)sums.data(), l.sums_bytes, sums_at)) ||
            (rc = fout.write_now(tail, tail_len, tail_off)))
            return rc;
        return HZ_OK;
    }

    int close_and_report() {
        if (int rc = fout.close()) return rc;
        spans.fold();
        if (written != (hbits + pbits + 7) / 8) return HZ_EFORMAT;
        if (verbose) {
            std::cout << "Encoding took " << ms_since(t_enc) << " ms" << std::endl;
            std::cout << "The size of the COMPRESSED file is: " << written << " bytes" << std::endl;
            const float ratio = 100.0f * (float)written / (float)(n ? n : 1);
            std::cout << "Compressed file's size is [" << ratio << "%] of the original files." << std::endl;
            if (written > n) std::cout << "\nWARNING: The compressed file's size is larger than the sum of the originals.\n\n";
            std::cout << std::endl << "Created compressed file: " << out_path << std::endl;
            std::cout << "Compression is complete" << std::endl;
        }
        return HZ_OK;
    }

    int run() {
        int rc;
        if ((rc = open_and_size()) || (rc = allocate()) || (rc = histogram_pass()) || (rc = codebook_and_header()) ||
            (rc = open_output()))
            return rc;
        if (nsym_total == 0) {  // an empty input or a single byte: the header alone
            if (pend_bits && (rc = fout.write_now(&pend, 1, written))) return rc;
            written += pend_bits ? 1 : 0;
        } else {
            if (resident && (rc = pack_resident())) return rc;
            if (!resident && (rc = pack_streamed())) return rc;
        }
        if ((rc = table_out(spans, c, sink, dseek, nsym_total))) return rc;
        if (seekable >= 0 && (rc = write_trailer())) return rc;
        return close_and_report();
    }
};

}  // namespace

extern "C" int hz_stream_last_timing(hz_stream_timing* t) {
    if (!t) return HZ_EINVAL;
    *t = g_timing;
    return HZ_OK;
}

// A streamed call: the thread's timing record started afresh, the body guarded, its wall time kept.
template <typename F>
static int timed_call(F&& body) {
    g_timing = hz_stream_timing();
    const auto t0 = Clock::now();
    const int rc = guarded(body);
    g_timing.total_ms = ms_since(t0);
    return rc;
}

extern "C" int hz_archive_stream_seekable(const char* in_path, const char* out_path, uint64_t chunk_bytes, int verbose,
                                          uint32_t flags) {
    if (flags & ~HZ_SEEKABLE_SUMS) return HZ_EINVAL;
    return timed_call([&] { return ArchiveFlow{in_path, out_path, chunk_bytes, verbose, false, nullptr, (int)flags}.run(); });
}

extern "C" int hz_archive_stream(const char* in_path, const char* out_path, uint64_t chunk_bytes, int verbose) {
    return timed_call([&] { return ArchiveFlow{in_path, out_path, chunk_bytes, verbose, false, nullptr}.run(); });
}

namespace {

// What hz_header_parse_device leaves in its six info words.
hz_header_info header_info_from_words(const uint64_t hi[6]) {
    hz_header_info info;
    info.n = hi[0];
    info.payload_byte = hi[1];
    info.payload_bit = (uint32_t)hi[2];
    info.is_odd = (uint32_t)hi[3];
    info.last_byte = (uint32_t)hi[4];
    info.nsym = (uint32_t)hi[5];
    return info;
}

// The header of a file to extract: parsed on the device (k_hdr_*, 0.05 ms for
// U = 65 536 against 0.25+ ms on the host; profiles/r03_codebook_*), the codebook
// and the info copied back for the host-built decode tables. HZ_HOST_HEADER=1
// parses on the host. Both follow Decompressor.cu:65-103 and reject the same files.
int parse_header_for_extract(const std::vector<uint8_t>& head, hz_codebook* cb, hz_header_info* info) {
    static const bool host_hdr = [] { const char* v = getenv("HZ_HOST_HEADER"); return v && v[0] == '1'; }();
    const auto th = Clock::now();
    int rc;
    if (host_hdr || head.size() < 12) {  // a header-only file: no device work at all
        rc = hz_header_parse(head.data(), head.size(), cb, info);
        g_timing.host_ms += ms_since(th);
        return rc;
    }
    hz_ctx* c;
    if ((rc = default_ctx(&c))) return rc;
    HZ_TRY(hipSetDevice(c->device));
    DevBuf dhead, dcb, dinfo;
    if ((rc = dhead.alloc(head.size())) || (rc = dcb.alloc(sizeof(hz_codebook))) || (rc = dinfo.alloc(6 * 8))) return rc;
    g_timing.alloc_ms += ms_since(th);  // context and buffers: allocation, as on the host path
    const auto tp = Clock::now();
    uint64_t hi[6];
    HZ_TRY(hipMemcpyAsync(dhead.p, head.data(), head.size(), hipMemcpyHostToDevice, c->stream));
    if ((rc = hz_header_parse_device(c, (const uint8_t*)dhead.p, head.size(), (hz_codebook*)dcb.p, (uint64_t*)dinfo.p)))
        return rc;
    HZ_TRY(hipMemcpyAsync(cb, dcb.p, sizeof(hz_codebook), hipMemcpyDeviceToHost, c->stream));
    HZ_TRY(hipMemcpyAsync(hi, dinfo.p, sizeof(hi), hipMemcpyDeviceToHost, c->stream));
    if ((rc = hz_ctx_sync(c))) return rc;  // HZ_EFORMAT for a malformed header
    *info = header_info_from_words(hi);
    g_timing.host_ms += ms_since(tp);
    return HZ_OK;
}

// Streaming extract: the payload passes through a device window of chunk_bytes (ExtractWindow,
// hz_stream_plan.h). Each round decodes as many symbols as the window surely holds (a round whose codes
// overrun the window is redone at the max_len bound), and moves the unconsumed tail of the window to
// the front of the other buffer before refilling it. The host's read of the
// next window overlaps the decode, and its write of a round's output overlaps
// the next round's upload and index-less decode (hz_decode_indexless).
//
// With a SeekSink the rounds also leave the file's seek table (hz_extract_stream_seek): every round is
// hz_decode_indexless_seek at sym_base = the symbols done and bit_base = 8 x the payload bytes the
// earlier rounds consumed, into one device table copied out once at the end. A round redone after an
// overrun rewrites its entries, and later rounds overwrite what the overrun attempt wrote past its
// window. Without an out_path (sink only) nothing is decoded, copied out or written.
//
// The seekable flows run the same rounds in whole blocks (ExtractWindow's whole_blocks), as their own sink,
// so a round's output, while it is still in dout, begins at block done / 2048 of the file's block sums:
//   kAttach (hz_seekable_attach_file)      the table and, with HZ_SEEKABLE_SUMS, one hz_block_sums per round
//     into one device array copied out once at the end like the table; no pinned output, no file write.
//     Without the flag nothing is decoded.
//   kVerified (hz_extract_stream_verified)  the trailer's sums uploaded once, and one hz_block_sums_check per
//     round into one device word that comes home with the round's end bit; a round's bytes leave for the
//     file only after that word said the round matched. An overrun attempt's word is discarded (reset before
//     the redo). After the last round the walk's table is compared with the stored one.
struct ExtractFlow {
    enum Mode { kExtract, kAttach, kVerified };

    const char* in_path;
    const char* out_path;
    uint64_t chunk_bytes;
    int verbose;
    const SeekSink* sink;
    Mode mode = kExtract;
    uint32_t want = 0;              // kAttach: the flags asked for
    uint64_t* bad_block = nullptr;  // kVerified: out, the smallest failing block

    hz_ctx* c = nullptr;
    bool write = false;
    bool decode = false;   // the rounds decode into dout (kExtract: the same as write)
    bool has_all = false;  // kAttach: the file's trailer already holds what `want` asks for
    hz_seekable_info si;
    uint64_t fsize = 0, nsym = 0;
    hz_header_info info;
    ExtractWindow w{0, 0, 0, 0, 0};
    uint64_t read_off = 0;  // the file byte the next refill starts at
    uint64_t out_off = 0;
    uint64_t k = 0;         // symbols of the round in flight
    int cur = 0, ob = 0;    // the window and the output buffer of the round in flight

    // buffers first, guards last (see StreamGuard)
    FileReader fin{&g_timing};
    Spans spans;
    std::vector<uint8_t> head;
    std::unique_ptr<hz_codebook> cb{new hz_codebook()};
    DevBuf dwin[2], didx, dout, dseek, dsums, dbad;
    PinnedBuf hin, hout[2];  // hout: a round's output leaves (parallel writes) beside the next round
    uint64_t end_bit = 0;
    uint64_t bad = UINT64_MAX;     // kVerified: the device's bad-block word, home with end_bit
    std::vector<uint64_t> table;   // the seekable flows: the walk's table and the sink that fills it,
    std::vector<uint64_t> stored;  // kVerified: the trailer's table,
    std::vector<uint32_t> sums;    // and the sums: kAttach's from the rounds, kVerified's from the trailer
    uint64_t own_nsym = 0;
    SeekSink own_sink{nullptr, 0, nullptr};
    FileWriter fout{&g_timing};
    DrainGuard drain;

    bool with_sums() const { return mode == kAttach && (want & HZ_SEEKABLE_SUMS); }

    int open_and_parse() {
        if (!in_path || (!out_path && !sink && mode == kExtract) || chunk_bytes < 4096) return HZ_EINVAL;
        if (sink && !sink->nsym) return HZ_EINVAL;
        write = out_path != nullptr;
        chunk_bytes &= ~(uint64_t)15;
        int rc = fin.open(in_path);
        if (rc) return rc;
        // a file with a trailer (hz_seekable.h) ends where its image ends: the trailer is no payload
        if ((rc = image_end_fd(fin.fd(), fin.size(), &fsize, &si))) return rc;
        if (mode == kVerified && !si.present) return HZ_EFORMAT;
        if (mode == kVerified && !(si.flags & HZ_SEEKABLE_SUMS)) return HZ_EINVAL;
        if (mode == kAttach && si.present && (si.flags & want) == want) {
            has_all = true;
            return HZ_OK;
        }
        head.resize(std::min<uint64_t>(fsize, kMaxHeaderBytes));
        if ((rc = fin.read(head.data(), head.size(), 0))) return rc;
        if ((rc = parse_header_for_extract(head, cb.get(), &info))) return rc;
        if (si.present && si.n != info.n) return HZ_EFORMAT;
        nsym = info.n / 2;
        if (mode != kExtract && (rc = own_table())) return rc;
        if (sink) {
            *sink->nsym = nsym;
            if (hz_seek_bytes(nsym) && (!sink->seek || sink->cap_bytes < hz_seek_bytes(nsym))) return HZ_ECAP;
        }
        return HZ_OK;
    }

    // The seekable flows' own table, sized by what the file can hold, and kVerified's trailer words.
    int own_table() {
        const uint64_t pay_bytes = fsize > info.payload_byte ? fsize - info.payload_byte : 0;
        // a header whose N overstates the payload must not size the table: the decode would reject it anyway
        if (!payload_holds(pay_bytes, info.payload_bit, nsym, cb->min_len)) return HZ_EFORMAT;
        table.resize(hz_seek_bytes(nsym) / 8);
        own_sink = SeekSink{table.data(), 8 * table.size(), &own_nsym};
        sink = &own_sink;
        if (mode != kVerified) return HZ_OK;
        stored.resize(table.size());
        sums.resize(si.nblocks);  // (the footer's own sizes add up to the file's: hz_seekable_footer_parse)
        int rc;
        if (!stored.empty() && (rc = pread_all(fin.fd(), (uint8_t*)stored.data(), 8 * stored.size(), si.seek_off))) return rc;
        if (!sums.empty() && (rc = pread_all(fin.fd(), (uint8_t*)sums.data(), 4 * sums.size(), si.sums_off))) return rc;
        return HZ_OK;
    }

    // Reserve no more than the payload can decode to: a header whose N overstates it (corrupt or
    // crafted) must not allocate disk before the decode rejects it.
    int open_output() {
        if (!write) return HZ_OK;
        if (int rc = fout.open(out_path)) return rc;
        const uint64_t pay_bytes = fsize > info.payload_byte ? fsize - info.payload_byte : 0;
        fout.reserve(std::min<uint64_t>(info.n, payload_most_bytes(pay_bytes, info.payload_bit, cb->min_len, info.is_odd)));
        return HZ_OK;
    }

    // The context, the decode tables, the buffers, and the first window with its round in flight.
    int first_window() {
        int rc = timed_default_ctx(&c);
        if (rc) return rc;
        drain.s = c->stream;
        const auto tu = Clock::now();
        if ((rc = hz_codebook_upload_decode(c, cb.get()))) return rc;
        g_timing.host_ms += ms_since(tu);
        const uint64_t pay_bytes = fsize > info.payload_byte ? fsize - info.payload_byte : 0;
        // (the seekable flows: no window larger than the payload, so a small file takes small buffers)
        const uint64_t window = mode == kExtract ? chunk_bytes
                                                 : std::min(chunk_bytes, std::max<uint64_t>((pay_bytes + 15) & ~(uint64_t)15,
                                                                                            HZ_SEEKABLE_MIN_WINDOW));
        w = ExtractWindow(window, nsym, pay_bytes, info.payload_bit, cb->max_len, mode != kExtract);
        decode = write || with_sums() || mode == kVerified;
        const auto ta = Clock::now();
        for (int i = 0; i < 2; ++i)
            if ((rc = dwin[i].alloc(w.W + 16))) return rc;
        if ((rc = didx.alloc(16))) return rc;  // the round's end bit
        if (decode && (rc = dout.alloc(2 * w.sym_cap + 16))) return rc;
        if (sink && (rc = dseek.alloc(hz_seek_bytes(nsym)))) return rc;
        if (with_sums()) sums.resize(hz_block_sums_bytes(2 * nsym) / 4);
        if (mode != kExtract && (rc = dsums.alloc(4 * sums.size()))) return rc;
        if (mode == kVerified && (rc = dbad.alloc(8))) return rc;
        if ((rc = hin.alloc(w.W))) return rc;
        for (int i = 0; i < 2; ++i)
            if (write && (rc = hout[i].alloc(2 * w.sym_cap))) return rc;
        g_timing.alloc_ms += ms_since(ta);
        if (mode == kVerified) {
            HZ_TRY(hipMemsetAsync(dbad.p, 0xFF, 8, c->stream));
            if ((rc = spans.copy(c->stream, &g_timing.h2d_ms, dsums.p, sums.data(), 4 * sums.size(), hipMemcpyHostToDevice)))
                return rc;
        }
        read_off = info.payload_byte;
        const uint64_t r = w.first_fill();
        if ((rc = refill_read(r))) return rc;
        HZ_TRY(hipMemsetAsync(dwin[cur].p, 0, w.W + 16, c->stream));
        if ((rc = upload_refill(cur, 0, r))) return rc;
        k = w.round_syms();
        return launch();
    }

    int refill_read(uint64_t r) {
        const int rc = fin.read(hin.p, r, read_off);
        read_off += r;
        return rc;
    }

    int upload_refill(int win, uint64_t at, uint64_t r) {
        return spans.copy(c->stream, &g_timing.h2d_ms, (uint8_t*)dwin[win].p + at, hin.p, r, hipMemcpyHostToDevice);
    }

    // a round: the window's first k codewords decoded index-less into dout (with a sink, their seek
    // entries; without an out_path dout is null and nothing is decoded), and their end bit
    int decode_call() {
        return spans.timed(c->stream, &g_timing.kernel_ms, [&] {
            return sink ? hz_decode_indexless_seek(c, (const uint8_t*)dwin[cur].p, w.have, w.bit, k, (uint8_t*)dout.p,
                                                   (uint64_t*)didx.p, w.done, 8 * w.consumed, nsym, (uint64_t*)dseek.p)
                        : hz_decode_indexless(c, (const uint8_t*)dwin[cur].p, w.have, w.bit, k, (uint8_t*)dout.p,
                                              (uint64_t*)didx.p);
        });
    }
    // the round's blocks begin at block w.done / 2048 (whole-block rounds): their sums stored (kAttach with
    // sums) or compared with the trailer's (kVerified), on the output while it is in dout
    int sums_call() {
        if (!with_sums() && mode != kVerified) return HZ_OK;
        uint32_t* words = (uint32_t*)dsums.p + w.done / kBlockSyms;
        return spans.timed(c->stream, &g_timing.kernel_ms, [&] {
            return mode == kVerified ? hz_block_sums_check(c, (const uint8_t*)dout.p, 2 * k, words, w.done / kBlockSyms,
                                                           (uint64_t*)dbad.p)
                                     : hz_block_sums(c, (const uint8_t*)dout.p, 2 * k, words);
        });
    }
    int launch() {
        int rc;
        if ((rc = decode_call()) || (rc = sums_call())) return rc;
        HZ_TRY(hipMemcpyAsync(&end_bit, didx.p, 8, hipMemcpyDeviceToHost, c->stream));
        if (mode == kVerified) HZ_TRY(hipMemcpyAsync(&bad, dbad.p, 8, hipMemcpyDeviceToHost, c->stream));
        return HZ_OK;
    }

    // One round: wait for the decode in flight (redo it at the bound if its codes overran the window),
    // copy its output out, move the unconsumed tail to the other window and read the refill behind the
    // decode; then the next window's upload and decode go out beside this round's file write.
    int round() {
        int rc;
        if ((rc = hz_ctx_sync(c))) return rc;
        if (w.overran(end_bit)) {
            k = w.redo_syms();
            // what the attempt's sums said of symbols past the window is no verdict
            if (mode == kVerified) HZ_TRY(hipMemsetAsync(dbad.p, 0xFF, 8, c->stream));
            if ((rc = launch()) || (rc = hz_ctx_sync(c))) return rc;
        }
        if (w.truncated(end_bit)) return HZ_EFORMAT;
        if (mode == kVerified && bad != UINT64_MAX) {  // the rounds before this one are the verified prefix
            if (bad_block) *bad_block = bad;
            return HZ_ECHECKSUM;
        }
        if (write && (rc = spans.copy(c->stream, &g_timing.d2h_ms, hout[ob].p, dout.p, 2 * k, hipMemcpyDeviceToHost))) return rc;
        const uint64_t kdone = k;
        const int nxt = cur ^ 1;
        const ExtractWindow::Step s = w.advance(end_bit, kdone);
        if (s.more) {
            if (s.tail) HZ_TRY(hipMemcpyAsync(dwin[nxt].p, (const uint8_t*)dwin[cur].p + s.used, s.tail,
                                              hipMemcpyDeviceToDevice, c->stream));
            if ((rc = refill_read(s.r))) return rc;
        }
        if ((rc = hz_ctx_sync(c))) return rc;    // decode, output copy and tail move done
        spans.fold();
        if (s.more) {  // next window and its decode, beside this round's write
            if (s.r < w.W - s.tail)
                HZ_TRY(hipMemsetAsync((uint8_t*)dwin[nxt].p + s.tail + s.r, 0, w.W + 16 - s.tail - s.r, c->stream));
            if (s.r && (rc = upload_refill(nxt, s.tail, s.r))) return rc;
            cur = nxt;
            k = w.round_syms();
            if ((rc = launch())) return rc;
        }
        if ((rc = fout.wait())) return rc;  // the previous round's write: hout[ob ^ 1] free for the next
        if (write) fout.start(hout[ob].p, 2 * kdone, out_off);
        out_off += 2 * kdone;
        ob ^= 1;
        return HZ_OK;
    }

    int odd_byte_and_close() {
        int rc;
        if (write && info.is_odd) {
            const uint8_t b = (uint8_t)info.last_byte;
            if ((rc = fout.write_now(&b, 1, out_off))) return rc;
        }
        if (write && (rc = fout.close())) return rc;
        if (verbose) std::cout << "Decompression is complete" << std::endl;
        return HZ_OK;
    }

    // kAttach: the rounds' sums to the host, once
    int sums_out() {
        if (!with_sums() || sums.empty()) return HZ_OK;
        const int rc = spans.copy(c->stream, &g_timing.d2h_ms, sums.data(), dsums.p, 4 * sums.size(), hipMemcpyDeviceToHost);
        return rc ? rc : hz_ctx_sync(c);
    }

    int run() {
        int rc;
        if ((rc = open_and_parse()) || has_all || (rc = open_output())) return rc;
        if (nsym > 0) {
            if ((rc = first_window())) return rc;
            while (w.done < nsym)
                if ((rc = round())) return rc;
            if ((rc = fout.wait()) || (rc = table_out(spans, c, sink, dseek, nsym)) || (rc = sums_out())) return rc;
            spans.fold();
        }
        return odd_byte_and_close();
    }

    // kVerified: whatever ends the flow early, the output ends at the last verified round's last byte (never
    // at its reserved size); and a complete output whose stored table is not the walk's is HZ_EFORMAT.
    int run_verified() {
        const int rc = run();
        if (rc) {
            (void)fout.wait();
            (void)fout.close();
            return rc;
        }
        return table == stored ? HZ_OK : HZ_EFORMAT;
    }

    // kAttach: the trailer behind the image, written once every round has succeeded: padding, table and sums
    // first, the footer last (until it stands the file is a plain file, or still ends in its old footer's
    // place). The image's bytes are never rewritten.
    int run_attach(int* attached) {
        int rc = run();
        if (rc || has_all) return rc;
        uint64_t len = hz_seekable_trailer_bytes(fsize, info.n, want);
        if (!len) return HZ_EINVAL;
        std::vector<uint8_t> tr(len);
        if ((rc = hz_seekable_trailer_write(fsize, info.n, table.data(), sums.data(), want, tr.data(), len, &len))) return rc;
        const int fd = ::open(in_path, O_WRONLY);
        if (fd < 0) return HZ_EIO;
        const uint64_t body = len - HZ_SEEKABLE_FOOTER_BYTES;
        rc = pwrite_all(fd, tr.data(), body, fsize);
        if (!rc && ::ftruncate(fd, (off_t)(fsize + len)) != 0) rc = HZ_EIO;
        if (!rc) rc = pwrite_all(fd, tr.data() + body, HZ_SEEKABLE_FOOTER_BYTES, fsize + body);
        if (::close(fd) != 0 && !rc) rc = HZ_EIO;
        if (!rc && attached) *attached = 1;
        return rc;
    }
};

}  // namespace

extern "C" int hz_extract_stream(const char* in_path, const char* out_path, uint64_t chunk_bytes, int verbose) {
    return timed_call([&] { return ExtractFlow{in_path, out_path, chunk_bytes, verbose, nullptr}.run(); });
}

extern "C" int hz_extract_stream_seek(const char* in_path, const char* out_path, uint64_t chunk_bytes, int verbose,
                                      uint64_t* seek, uint64_t cap_bytes, uint64_t* nsym) {
    if (!in_path || !nsym || chunk_bytes < 4096) return HZ_EINVAL;
    const SeekSink sink{seek, cap_bytes, nsym};
    return timed_call([&] { return ExtractFlow{in_path, out_path, chunk_bytes, verbose, &sink}.run(); });
}

extern "C" int hz_seekable_attach_file(const char* path, uint64_t chunk_bytes, uint32_t flags, int* attached) {
    if (attached) *attached = 0;
    if (!path || (flags & ~HZ_SEEKABLE_SUMS) || chunk_bytes < HZ_SEEKABLE_MIN_WINDOW) return HZ_EINVAL;
    return timed_call([&] {
        return ExtractFlow{path, nullptr, chunk_bytes, 0, nullptr, ExtractFlow::kAttach, flags}.run_attach(attached);
    });
}

extern "C" int hz_extract_stream_verified(const char* in_path, const char* out_path, uint64_t chunk_bytes, int verbose,
                                          uint64_t* bad_block) {
    if (!in_path || chunk_bytes < HZ_SEEKABLE_MIN_WINDOW) return HZ_EINVAL;
    return timed_call([&] {
        return ExtractFlow{in_path, out_path, chunk_bytes, verbose, nullptr, ExtractFlow::kVerified, 0, bad_block}.run_verified();
    });
}

namespace {

// Salvage of a damaged seekable file (hz_seekable_salvage_file): the table restarts the decode at every block
// and the sums say which blocks came out right, so the file is walked in windows of blocks (SalvagePlan,
// hz_salvage_plan.h: cut from a table that may itself be damaged) and every block is judged on its own.
// A window: its payload span read and uploaded, its output zero-filled, ONE hz_decode_ranges call with one
// range (a block that fails the decoder's checks is flagged and stores nothing: it keeps the zeros),
// hz_block_sums_mark on the output into one device bitmap for the whole file, the output copied out, one
// hz_ctx_sync, and the window's bytes handed to the writer beside the next window's read and device work.
// The sync's HZ_EFORMAT / HZ_EINVAL with flagged blocks counted is the decoder's report of those blocks, not
// a failure of the flow. Memory: one payload window and one output window on the device, one pinned payload
// window and two pinned output windows, the table, the sums and the bitmap.
struct SalvageFlow {
    const char* in_path;
    const char* out_path;
    uint64_t chunk_bytes;
    uint32_t flags;
    uint64_t* bad_blocks;
    uint64_t bad_cap;
    uint64_t* nbad;

    hz_ctx* c = nullptr;
    bool write = false;
    hz_seekable_info si;
    hz_header_info info;
    uint64_t fsize = 0, nsym = 0, nblocks = 0, pay_bytes = 0;
    uint64_t in_cap = 0, out_cap = 0;
    int ob = 0;  // the pinned output buffer of the window in flight

    // buffers first, guards last (see StreamGuard)
    FileReader fin{&g_timing};
    Spans spans;
    std::vector<uint8_t> head;
    std::unique_ptr<hz_codebook> cb{new hz_codebook()};
    std::vector<uint64_t> table;
    std::vector<uint32_t> sums, bits;
    DevBuf dwin, dout, dseek, dsums, dbits, dstats, drange;
    PinnedBuf hin, hout[2], hrange;
    uint64_t stats[HZ_RANGES_STATS_WORDS] = {0, 0, 0, 0};
    FileWriter fout{&g_timing};
    DrainGuard drain;

    int open_and_parse() {
        if (nbad) *nbad = 0;
        if (!in_path || !nbad || (flags & ~HZ_SALVAGE_KEEP_UNVERIFIED) || (bad_cap && !bad_blocks)) return HZ_EINVAL;
        if (chunk_bytes < HZ_SEEKABLE_MIN_WINDOW) return HZ_EINVAL;
        write = out_path != nullptr;
        chunk_bytes &= ~(uint64_t)15;
        int rc = fin.open(in_path);
        if (rc) return rc;
        if ((rc = image_end_fd(fin.fd(), fin.size(), &fsize, &si))) return rc;
        if (!si.present) return HZ_EFORMAT;
        if (!(si.flags & HZ_SEEKABLE_SUMS)) return HZ_EINVAL;
        head.resize(std::min<uint64_t>(fsize, kMaxHeaderBytes));
        if ((rc = fin.read(head.data(), head.size(), 0))) return rc;
        if ((rc = parse_header_for_extract(head, cb.get(), &info))) return rc;
        if (si.n != info.n) return HZ_EFORMAT;
        nsym = info.n / 2;
        nblocks = si.nblocks;
        pay_bytes = fsize > info.payload_byte ? fsize - info.payload_byte : 0;
        // a header whose N overstates the payload must not size the output: no decode could fill it
        if (!payload_holds(pay_bytes, info.payload_bit, nsym, cb->min_len)) return HZ_EFORMAT;
        table.resize(hz_seek_bytes(nsym) / 8);
        sums.resize(nblocks);
        bits.assign((nblocks + 31) / 32, 0u);
        if (!table.empty() && (rc = pread_all(fin.fd(), (uint8_t*)table.data(), 8 * table.size(), si.seek_off))) return rc;
        if (!sums.empty() && (rc = pread_all(fin.fd(), (uint8_t*)sums.data(), 4 * sums.size(), si.sums_off))) return rc;
        return HZ_OK;
    }

    int open_output() {
        if (!write) return HZ_OK;
        if (int rc = fout.open(out_path)) return rc;
        fout.reserve(info.n);
        return HZ_OK;
    }

    // The context, the decode tables, the buffers; the table and the sums uploaded once, the bitmap zeroed.
    int prepare() {
        int rc = timed_default_ctx(&c);
        if (rc) return rc;
        drain.s = c->stream;
        const auto tu = Clock::now();
        if ((rc = hz_codebook_upload_decode(c, cb.get()))) return rc;
        g_timing.host_ms += ms_since(tu);
        // no window larger than the file needs, so a small file takes small buffers
        in_cap = std::min(chunk_bytes, std::max<uint64_t>((pay_bytes + 15) & ~(uint64_t)15, 16));
        out_cap = std::min(std::max<uint64_t>(chunk_bytes / HZ_SUM_BLOCK_BYTES, 1), nblocks) * HZ_SUM_BLOCK_BYTES;
        const auto ta = Clock::now();
        if ((rc = dwin.alloc(in_cap + 16)) || (rc = dout.alloc(out_cap)) || (rc = dseek.alloc(8 * table.size())) ||
            (rc = dsums.alloc(4 * sums.size())) || (rc = dbits.alloc(4 * bits.size())) ||
            (rc = dstats.alloc(8 * HZ_RANGES_STATS_WORDS)) || (rc = drange.alloc(sizeof(hz_range))))
            return rc;
        if ((rc = hin.alloc(in_cap)) || (rc = hrange.alloc(sizeof(hz_range)))) return rc;
        for (int i = 0; i < 2; ++i)
            if (write && (rc = hout[i].alloc(out_cap))) return rc;
        g_timing.alloc_ms += ms_since(ta);
        HZ_TRY(hipMemsetAsync(dbits.p, 0, 4 * bits.size(), c->stream));
        if ((rc = spans.copy(c->stream, &g_timing.h2d_ms, dseek.p, table.data(), 8 * table.size(), hipMemcpyHostToDevice)) ||
            (rc = spans.copy(c->stream, &g_timing.h2d_ms, dsums.p, sums.data(), 4 * sums.size(), hipMemcpyHostToDevice)))
            return rc;
        return HZ_OK;
    }

    int window(const SalvageWindow& w) {
        int rc;
        const uint64_t begin = std::min(w.byte_begin, pay_bytes), len = std::min(w.byte_end, pay_bytes) - begin;
        const uint64_t sym0 = w.first_block * kBlockSyms, syms = std::min(nsym - sym0, w.nblocks * kBlockSyms);
        if (len > in_cap || 2 * syms > out_cap) return HZ_EFORMAT;  // (the plan keeps both within chunk_bytes)
        if (len) {
            if ((rc = fin.read(hin.p, len, info.payload_byte + begin))) return rc;
            if ((rc = spans.copy(c->stream, &g_timing.h2d_ms, dwin.p, hin.p, len, hipMemcpyHostToDevice))) return rc;
        }
        // (the wait of the window before this one is behind us: its copy of the range has been made)
        *reinterpret_cast<hz_range*>(hrange.p) = hz_range{sym0, syms, 0};
        HZ_TRY(hipMemcpyAsync(drange.p, hrange.p, sizeof(hz_range), hipMemcpyHostToDevice, c->stream));
        HZ_TRY(hipMemsetAsync(dout.p, 0, 2 * syms, c->stream));
        rc = spans.timed(c->stream, &g_timing.kernel_ms, [&]() -> int {
            if (int r2 = hz_decode_ranges(c, (const uint8_t*)dwin.p, len, begin, (const uint64_t*)dseek.p, nsym,
                                          (const hz_range*)drange.p, 1, (uint8_t*)dout.p, 2 * syms, (uint64_t*)dstats.p, 0))
                return r2;
            HZ_TRY(hipMemcpyAsync(stats, dstats.p, sizeof(stats), hipMemcpyDeviceToHost, c->stream));
            return hz_block_sums_mark(c, (uint8_t*)dout.p, 2 * syms, (const uint32_t*)dsums.p + w.first_block, w.first_block,
                                      (uint32_t*)dbits.p, (flags & HZ_SALVAGE_KEEP_UNVERIFIED) ? 0u : HZ_SUMS_ZERO_BAD);
        });
        if (rc) return rc;
        if (write && (rc = spans.copy(c->stream, &g_timing.d2h_ms, hout[ob].p, dout.p, 2 * syms, hipMemcpyDeviceToHost))) return rc;
        rc = hz_ctx_sync(c);  // the window's one host wait
        spans.fold();
        // flagged blocks are what a salvage expects to meet: they stored nothing and their sums judge them
        if (rc && !((rc == HZ_EFORMAT || rc == HZ_EINVAL) && stats[3] > 0)) return rc;
        if (write) {
            if ((rc = fout.wait())) return rc;  // the previous window's write: the other buffer is free again
            fout.start(hout[ob].p, 2 * syms, (uint64_t)HZ_SUM_BLOCK_BYTES * w.first_block);
            ob ^= 1;
        }
        return HZ_OK;
    }

    // The bitmap home, its set bits counted and listed in ascending order.
    int report() {
        int rc;
        if (!bits.empty()) {
            rc = spans.copy(c->stream, &g_timing.d2h_ms, bits.data(), dbits.p, 4 * bits.size(), hipMemcpyDeviceToHost);
            if (rc || (rc = hz_ctx_sync(c))) return rc;
            spans.fold();
        }
        uint64_t count = 0;
        for (uint64_t b = 0; b < nblocks; ++b) {
            if (!(bits[b >> 5] >> (b & 31) & 1u)) continue;
            if (count < bad_cap) bad_blocks[count] = b;
            ++count;
        }
        *nbad = count;
        return HZ_OK;
    }

    // Whatever ends the flow early, the output ends at its last written window, never at its reserved size.
    int run() {
        const int rc = windows();
        if (rc) {
            (void)fout.wait();
            (void)fout.close();
        }
        return rc;
    }

    int windows() {
        int rc;
        if ((rc = open_and_parse()) || (rc = open_output())) return rc;
        if (nblocks) {
            if ((rc = prepare())) return rc;
            SalvagePlan plan(table.data(), nblocks, pay_bytes, cb->max_len, chunk_bytes);
            SalvageWindow w;
            while (plan.next(&w))
                if ((rc = window(w))) return rc;
            if ((rc = fout.wait()) || (rc = report())) return rc;
        }
        if (write && info.is_odd) {
            const uint8_t b = (uint8_t)info.last_byte;
            if ((rc = fout.write_now(&b, 1, 2 * nsym))) return rc;
        }
        return write ? fout.close() : HZ_OK;
    }
};

}  // namespace

extern "C" int hz_seekable_salvage_file(const char* in_path, const char* out_path, uint64_t chunk_bytes, uint32_t flags,
                                        uint64_t* bad_blocks, uint64_t bad_cap, uint64_t* nbad) {
    return timed_call([&] { return SalvageFlow{in_path, out_path, chunk_bytes, flags, bad_blocks, bad_cap, nbad}.run(); });
}

extern "C" int hz_archive_stream_seek(const char* in_path, const char* out_path, uint64_t chunk_bytes, int verbose,
                                      uint64_t* seek, uint64_t seek_cap_bytes, uint64_t* nsym) {
    if (!nsym) return HZ_EINVAL;
    const SeekSink sink{seek, seek_cap_bytes, nsym};
    return timed_call([&] { return ArchiveFlow{in_path, out_path, chunk_bytes, verbose, false, &sink}.run(); });
}

static int archive_file_impl(const char* path, int verbose, const SeekSink* sink) {
    if (!path) return HZ_EINVAL;
    struct stat st;
    if (stat(path, &st) != 0) {
        if (verbose) std::cout << path << " file does not exist" << std::endl << "Process has been terminated" << std::endl;
        return HZ_ENOENT;
    }
    const std::string outname = std::string(path) + ".compressed";
    // HZ_ARCHIVE_CHUNK: chunk bytes of the file reads and payload writes (tests use small ones)
    const uint64_t chunk = env_u64("HZ_ARCHIVE_CHUNK", 64, kArchiveChunk);
    if (sink) {  // a table too small is refused here: whatever stands at outname stays as it is
        *sink->nsym = (uint64_t)st.st_size / 2;
        if (sink->cap_bytes < hz_seek_bytes(*sink->nsym) || (!sink->seek && *sink->nsym)) return HZ_ECAP;
    }
    // resident: the input stays on the device between the passes when it fits
    const int rc = timed_call([&] { return ArchiveFlow{path, outname.c_str(), chunk, verbose, true, sink}.run(); });
    if (rc) {
        remove(outname.c_str());  // never leave a truncated archive behind
        if (verbose) std::cerr << "archive: " << hz_strerror(rc) << std::endl;
    }
    return rc;
}

// Compressor.cu:315-632, stdout lines kept (:335-336,385,612-631).
extern "C" int hz_archive_file(const char* path, int verbose) { return archive_file_impl(path, verbose, nullptr); }

extern "C" int hz_archive_file_seek(const char* path, int verbose, uint64_t* seek, uint64_t seek_cap_bytes, uint64_t* nsym) {
    if (!nsym) return HZ_EINVAL;
    const SeekSink sink{seek, seek_cap_bytes, nsym};
    return archive_file_impl(path, verbose, &sink);
}

// Decompressor.cu:47-114.
extern "C" int hz_extract_file(const char* path, char* out_name, size_t out_name_cap, int verbose) {
    if (!path) return HZ_EINVAL;
    struct stat st;
    if (stat(path, &st) != 0) {
        if (verbose) std::cout << path << " does not exist" << std::endl;
        return HZ_ENOENT;
    }
    std::string name = output_name();
    // HZ_EXTRACT_WINDOW: payload window bytes (>= 4096)
    const uint64_t window = env_u64("HZ_EXTRACT_WINDOW", 4096, kExtractWindow);
    int rc = hz_extract_stream(path, name.c_str(), window, 0);
    if (rc) {
        remove(name.c_str());
        if (verbose) std::cerr << "extract: " << hz_strerror(rc) << std::endl;
        return rc;
    }
    if (out_name && out_name_cap) {
        strncpy(out_name, name.c_str(), out_name_cap - 1);
        out_name[out_name_cap - 1] = 0;
    }
    if (verbose) std::cout << "Decompression is complete" << std::endl;
    return HZ_OK;
}
