// hz_stream.cpp -- the file-level `archive` / `extract` flows (Compressor.cu:315-632,
// Decompressor.cu:47-114), streamed through bounded host and device memory on the process-wide context.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <iostream>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "hz_host.h"

using namespace hz;

// ---- streaming archive: bounded host and device memory ----
// Pass 1 reads the file in chunks and accumulates the histogram on the device;
// pass 2 packs chunk by chunk at the running bit offset. Each chunk's last,
// partial word is carried into the next chunk as its `lead` bits, so the file
// is byte-identical to the whole-buffer encoder's. Double-buffered pinned and
// device buffers keep the host's fread of chunk k + 1 and fwrite of chunk
// k - 1 beside the device's upload and pack of chunk k, and the copy-out of
// chunk k runs on a second stream beside the upload and pack of chunk k + 1.
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
    struct Span { hipEvent_t a, b; double* acc; };
    std::vector<Span> open_;
    std::vector<hipEvent_t> free_;
};

// Reads of 16 MiB and more go through 8 threads' positional reads (from the
// stream's logical position, which is then moved past them): a single fread
// copies out of the page cache at ~15 GB/s on the MI355X host.
int read_exact(FILE* fp, uint8_t* p, uint64_t n) {
    if (n == 0) return HZ_OK;
    const auto t0 = Clock::now();
    bool ok;
    if (n < (16u << 20)) {
        ok = fread(p, 1, n, fp) == n;
    } else {
        const off_t pos = ftello(fp);
        const int fd = fileno(fp);
        constexpr uint64_t kReaders = 8;
        const uint64_t piece = ((n + kReaders - 1) / kReaders + 4095) & ~(uint64_t)4095;
        std::atomic<bool> bad{pos < 0};
        std::vector<std::thread> th;
        // joins every started reader on every exit, a failed thread spawn (std::system_error,
        // turned into an HZ_ status by guarded()) included
        struct Joiner {
            std::vector<std::thread>& v;
            ~Joiner() { for (auto& t : v) if (t.joinable()) t.join(); }
        } joiner{th};
        for (uint64_t a = 0; a < n && !bad; a += piece) {
            const uint64_t len = std::min(piece, n - a);
            th.emplace_back([&bad, fd, p, a, len, pos] {
                uint64_t done = 0;
                while (done < len) {
                    const ssize_t r = ::pread(fd, p + a + done, len - done, (off_t)(pos + a + done));
                    if (r <= 0) { bad = true; return; }
                    done += (uint64_t)r;
                }
            });
        }
        for (auto& t : th) t.join();
        th.clear();
        ok = !bad && fseeko(fp, pos + (off_t)n, SEEK_SET) == 0;
    }
    g_timing.fread_ms += ms_since(t0);
    g_timing.bytes_in += ok ? n : 0;
    return ok ? HZ_OK : HZ_EIO;
}

// Output file written by background positional writes, so a chunk's write
// overlaps the next chunk's device work. The file's final size is reserved
// first (posix_fallocate): into page cache, 8 threads then write ~12 GB/s on
// the MI355X host, against ~5 GB/s for one or 8 threads into a file that grows
// (block allocation under the inode lock), 6.8 GB/s with O_DIRECT and 1.7 GB/s
// copying into a shared mmap (tools/debug/write_bw.py, 8 GiB). start() hands a
// buffer to kWriters threads (one slice each) and returns; wait() joins them.
// One write is in flight at a time, so the caller double-buffers.
class FileWriter {
  public:
    ~FileWriter() {
        (void)wait();
        if (fd_ >= 0) ::close(fd_);
    }
    int open(const char* path) {
        fd_ = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
        return fd_ >= 0 ? HZ_OK : HZ_EIO;
    }
    // Reserve the file's final size (best effort: a file system without
    // fallocate only loses the speed-up).
    void reserve(uint64_t size) {
        if (fd_ >= 0 && size > 0) reserved_ = ::posix_fallocate(fd_, 0, (off_t)size) == 0;
    }
    void start(const uint8_t* p, uint64_t n, uint64_t off) {
        if (n == 0) return;
        t0_ = Clock::now();
        end_ = std::max(end_, off + n);
        const uint64_t nt = n < (8u << 20) ? 1 : kWriters;
        const uint64_t piece = ((n + nt - 1) / nt + 4095) & ~(uint64_t)4095;
        for (uint64_t a = 0; a < n; a += piece) {
            const uint64_t len = std::min(piece, n - a);
            th_.emplace_back([this, p, a, len, off] {
                uint64_t done = 0;
                while (done < len) {
                    const ssize_t w = ::pwrite(fd_, p + a + done, len - done, (off_t)(off + a + done));
                    if (w <= 0) { err_ = true; return; }
                    done += (uint64_t)w;
                }
            });
        }
        g_timing.bytes_out += n;
    }
    int wait() {
        if (th_.empty()) return err_ ? HZ_EIO : HZ_OK;
        for (auto& t : th_) t.join();
        th_.clear();
        g_timing.fwrite_ms += ms_since(t0_);
        return err_ ? HZ_EIO : HZ_OK;
    }
    int write_now(const uint8_t* p, uint64_t n, uint64_t off) {
        int rc = wait();
        if (rc) return rc;
        start(p, n, off);
        return wait();
    }
    int close() {
        int rc = wait();
        // the file ends at its last written byte, whatever reserve() allocated
        if (fd_ >= 0 && reserved_ && ::ftruncate(fd_, (off_t)end_) != 0) rc = HZ_EIO;
        if (fd_ >= 0 && ::close(fd_) != 0) rc = HZ_EIO;
        fd_ = -1;
        return rc;
    }
  private:
    static constexpr uint64_t kWriters = 8;
    int fd_ = -1;
    bool reserved_ = false;
    uint64_t end_ = 0;
    std::vector<std::thread> th_;
    std::atomic<bool> err_{false};
    Clock::time_point t0_;
};

// Declared after the host buffers a FileWriter reads: an early return waits
// for the writes in flight before those buffers are freed.
struct WriterDrain {
    FileWriter& w;
    ~WriterDrain() { (void)w.wait(); }
};

struct StreamGuard {
    hipStream_t s = nullptr;
    ~StreamGuard() {
        if (s) {
            (void)hipStreamSynchronize(s);  // no copy may outlive the buffers it targets
            (void)hipStreamDestroy(s);
        }
    }
};

// Declared after a function's pinned and device buffers, so it runs before
// they are freed: an early return (I/O error) waits for the copies in flight.
struct DrainGuard {
    hipStream_t s;
    explicit DrainGuard(hipStream_t st) : s(st) {}
    ~DrainGuard() { (void)hipStreamSynchronize(s); }
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

// Decompressor.cu:185-219: "DECOMPRESSED_FILE", else "DECOMPRESSED_FILE(k)", k = 1..9.
std::string output_name() {
    const std::string base = "DECOMPRESSED_FILE";
    std::string name = base;
    for (int k = 1; k < 10 && access(name.c_str(), F_OK) == 0; ++k) name = base + "(" + std::to_string(k) + ")";
    return name;
}

}  // namespace

extern "C" int hz_stream_last_timing(hz_stream_timing* t) {
    if (!t) return HZ_EINVAL;
    *t = g_timing;
    return HZ_OK;
}

// Where a streamed call leaves the file's seek table (hz_archive_stream_seek, hz_extract_stream_seek).
struct SeekSink {
    uint64_t* seek;      // host, cap_bytes
    uint64_t cap_bytes;
    uint64_t* nsym;      // out: the file's symbols
};

// resident: keep the input on the device after pass 1 when the file fits
// (hz_archive_file; Compressor.cu:324-367 reads the file once into pinned
// memory), so pass 2 packs it in one launch without reading the file again.
//
// With a SeekSink the writer also leaves the file's seek table (hz_archive_stream_seek): every pack is
// hz_pack_seek at sym_base = the symbols packed and bit_base = 8 x the payload bytes handed to the file
// writer (the pack's output starts at the file byte of the first payload bit, which is where the table's
// bits count from), into one device table copied out once at the end. Chunks are whole blocks, and a
// chunk's end bit comes back from the table: no per-chunk block index.
static int hz_archive_stream_impl(const char* in_path, const char* out_path, uint64_t chunk_bytes, int verbose,
                                  bool resident, const SeekSink* sink = nullptr) {
    if (!in_path || !out_path || chunk_bytes < 64) return HZ_EINVAL;
    if (sink && !sink->nsym) return HZ_EINVAL;
    chunk_bytes &= ~(uint64_t)15;  // even (whole symbols) and 16-byte aligned device reads
    if (sink) chunk_bytes = std::max<uint64_t>(chunk_bytes / (2 * kBlockSyms) * (2 * kBlockSyms), 2 * kBlockSyms);
    struct stat st;
    if (stat(in_path, &st) != 0) return HZ_ENOENT;
    const uint64_t n = (uint64_t)st.st_size;
    if (sink) {
        *sink->nsym = n / 2;
        if (sink->cap_bytes < hz_seek_bytes(n / 2) || (!sink->seek && n / 2)) return HZ_ECAP;
    }
    hz_ctx* c;
    const auto tc = Clock::now();
    int rc = default_ctx(&c);
    g_timing.alloc_ms += ms_since(tc);
    if (rc) return rc;
    HZ_TRY(hipSetDevice(c->device));
    Spans spans;
    const uint64_t chunk = std::min<uint64_t>(chunk_bytes, std::max<uint64_t>(n, 16));
    PinnedBuf hin[2];
    DevBuf din[2], dhist, dall;
    const auto ta = Clock::now();
    if (resident && n > chunk) {
        // the whole input plus a payload of the same size must fit in free device memory
        size_t fr = 0, tot = 0;
        resident = hipMemGetInfo(&fr, &tot) == hipSuccess && 2 * n + (1ull << 30) <= fr && dall.alloc(n + 16) == HZ_OK;
    } else {
        resident = false;
    }
    for (int i = 0; i < 2; ++i) {
        if ((rc = hin[i].alloc(chunk))) return rc;
        if (!resident && (rc = din[i].alloc(chunk + 16))) return rc;
    }
    if ((rc = dhist.alloc(HZ_NSYM * 8))) return rc;
    g_timing.alloc_ms += ms_since(ta);
    DrainGuard drain_in(c->stream);
    uint8_t last_byte = 0;
    FILE* fp = fopen(in_path, "rb");
    if (!fp) return HZ_EIO;
    std::unique_ptr<FILE, int (*)(FILE*)> fin(fp, fclose);
    // ---- pass 1: histogram (resident: the chunks stay in dall)
    const auto t_hist = Clock::now();  // "Histograming took" (Compressor.cu:395-399): read + upload + histogram
    HZ_TRY(hipMemsetAsync(dhist.p, 0, HZ_NSYM * 8, c->stream));
    EventPair done;
    if ((rc = done.create())) return rc;
    for (uint64_t off = 0, k = 0; off < n; off += chunk, ++k) {
        const uint64_t len = std::min(chunk, n - off);
        const int b = (int)(k & 1);
        if (k >= 2) HZ_TRY(hipEventSynchronize(done.e[b]));  // buffer b's previous chunk is consumed
        spans.fold();
        if ((rc = read_exact(fp, hin[b].p, len))) return rc;
        if (off + len == n && (n & 1)) last_byte = hin[b].p[len - 1];
        uint8_t* dst = resident ? (uint8_t*)dall.p + off : (uint8_t*)din[b].p;
        hipEvent_t t0 = spans.mark(c->stream);
        HZ_TRY(hipMemcpyAsync(dst, hin[b].p, len, hipMemcpyHostToDevice, c->stream));
        spans.add(t0, spans.mark(c->stream), &g_timing.h2d_ms);
        hipEvent_t t1 = spans.mark(c->stream);
        if ((rc = hz_hist16(c, dst, len, (uint64_t*)dhist.p, 1))) return rc;
        spans.add(t1, spans.mark(c->stream), &g_timing.kernel_ms);
        HZ_TRY(hipEventRecord(done.e[b], c->stream));
    }
    // the codebook is built on the device from the device histogram (k_cb_*, 0.26 ms for
    // U = 65 536 against 0.43 ms on the host plus the histogram's D2H; profiles/r03_codebook_*);
    // HZ_HOST_CODEBOOK=1 builds it on the host instead. Both are bit-exact with GenerateCL.
    static const bool host_cb = [] { const char* v = getenv("HZ_HOST_CODEBOOK"); return v && v[0] == '1'; }();
    // and so is the header (k_hw_*, 0.014 ms against 0.25 ms on the host)
    std::vector<uint64_t> hist(HZ_NSYM);
    std::unique_ptr<hz_codebook> cb(new hz_codebook());
    constexpr uint64_t kHeadCap = 16 + 65536ull * 11;  // the longest header
    std::vector<uint8_t> head;
    uint64_t dinfo_h[4] = {0, 0, 0, 0};
    DevBuf dcb, dhead, dinfo;
    EventPair cbt;  // "construction time" (gpuHuffmanConstruction.h:776-782): the device codebook
    if ((rc = cbt.create(true))) return rc;
    if (!host_cb) {
        if ((rc = dcb.alloc(sizeof(hz_codebook))) || (rc = dhead.alloc(kHeadCap)) || (rc = dinfo.alloc(4 * 8))) return rc;
        head.resize(kHeadCap);
        hipEvent_t t0 = spans.mark(c->stream);
        HZ_TRY(hipEventRecord(cbt.e[0], c->stream));
        if ((rc = hz_codebook_build_device(c, (const uint64_t*)dhist.p, (hz_codebook*)dcb.p))) return rc;
        HZ_TRY(hipEventRecord(cbt.e[1], c->stream));
        if ((rc = hz_header_write_device(c, (const hz_codebook*)dcb.p, n, last_byte, (uint8_t*)dhead.p, kHeadCap,
                                         (uint64_t*)dinfo.p)))
            return rc;
        spans.add(t0, spans.mark(c->stream), &g_timing.kernel_ms);
    }
    {
        hipEvent_t t0 = spans.mark(c->stream);
        HZ_TRY(hipMemcpyAsync(hist.data(), dhist.p, HZ_NSYM * 8, hipMemcpyDeviceToHost, c->stream));
        if (!host_cb) {
            HZ_TRY(hipMemcpyAsync(cb.get(), dcb.p, sizeof(hz_codebook), hipMemcpyDeviceToHost, c->stream));
            HZ_TRY(hipMemcpyAsync(dinfo_h, dinfo.p, sizeof(dinfo_h), hipMemcpyDeviceToHost, c->stream));
            HZ_TRY(hipMemcpyAsync(head.data(), dhead.p, kHeadCap, hipMemcpyDeviceToHost, c->stream));
        }
        spans.add(t0, spans.mark(c->stream), &g_timing.d2h_ms);
    }
    if ((rc = hz_ctx_sync(c))) return rc;
    const double hist_ms = ms_since(t_hist);
    const auto th = Clock::now();
    if (host_cb && (rc = hz_codebook_build(hist.data(), cb.get()))) return rc;
    float cb_ms = 0.0f;
    if (host_cb) cb_ms = (float)ms_since(th);
    else HZ_TRY(hipEventElapsedTime(&cb_ms, cbt.e[0], cbt.e[1]));
    uint64_t hbits = 0, pbits = 0;
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
    const auto t_enc = Clock::now();  // "Encoding took" (Compressor.cu:588-593): header, pack, payload out
    // ---- header
    uint64_t hb;
    uint32_t pend_bits;
    uint8_t pend;
    if (host_cb) {
        head.resize(hbits / 8 + 8);
        if ((rc = hz_header_write(cb.get(), n, last_byte, head.data(), head.size(), &hb, &pend_bits, &pend))) return rc;
    } else {
        hb = dinfo_h[0];
        pend_bits = (uint32_t)dinfo_h[1];
        pend = (uint8_t)dinfo_h[2];
        if (dinfo_h[3] != hbits) return HZ_EFORMAT;  // the device writer disagrees with the header length
    }
    g_timing.host_ms += ms_since(th);
    FileWriter fout;
    if ((rc = fout.open(out_path))) return rc;
    fout.reserve(hb + (pend_bits + pbits + 7) / 8);
    if ((rc = fout.write_now(head.data(), hb, 0))) return rc;
    uint64_t written = hb;
    const uint64_t nsym_total = n / 2;
    const uint64_t body = 2 * nsym_total;  // the odd last byte travels in the header
    uint32_t lead = pend_bits ? (uint32_t)(pend >> (8 - pend_bits)) : 0u;
    DevBuf dpay, dseek;
    if (sink && nsym_total && (rc = dseek.alloc(hz_seek_bytes(nsym_total)))) return rc;
    if (resident && nsym_total) {
        const uint64_t pay_bytes = (pend_bits + pbits + 7) / 8;
        const uint64_t cap = ((pend_bits + pbits + 31) / 32 + 1) * 4;
        const auto tb = Clock::now();
        resident = dpay.alloc(cap) == HZ_OK;
        g_timing.alloc_ms += ms_since(tb);
        if (resident) {
            // ---- pass 2, resident: one pack launch over the whole input, then the payload
            // leaves in chunks (copy-out double-buffered against the parallel file writes)
            const auto tu = Clock::now();
            if ((rc = hz_codebook_upload_encode(c, cb.get()))) return rc;
            g_timing.host_ms += ms_since(tu);
            hipEvent_t t1 = spans.mark(c->stream);
            rc = sink ? hz_pack_seek(c, (const uint8_t*)dall.p, body, pend_bits, lead, (uint8_t*)dpay.p, cap, nullptr, 0, 0,
                                     nsym_total, (uint64_t*)dseek.p)
                      : hz_pack(c, (const uint8_t*)dall.p, body, pend_bits, lead, (uint8_t*)dpay.p, cap, nullptr);
            if (rc) return rc;
            spans.add(t1, spans.mark(c->stream), &g_timing.kernel_ms);
            for (uint64_t off = 0, k = 0; off < pay_bytes; off += chunk, ++k) {
                const int b = (int)(k & 1);
                const uint64_t len = std::min(chunk, pay_bytes - off);
                hipEvent_t t2 = spans.mark(c->stream);
                HZ_TRY(hipMemcpyAsync(hin[b].p, (const uint8_t*)dpay.p + off, len, hipMemcpyDeviceToHost, c->stream));
                spans.add(t2, spans.mark(c->stream), &g_timing.d2h_ms);
                HZ_TRY(hipEventRecord(done.e[b], c->stream));
                HZ_TRY(hipEventSynchronize(done.e[b]));
                if ((rc = hz_ctx_sync(c))) return rc;
                spans.fold();
                if ((rc = fout.wait())) return rc;  // the write of chunk k - 1 (buffer 1 - b)
                fout.start(hin[b].p, len, written);
                written += len;
            }
        } else {  // no room for the payload beside the input: stream pass 2 from the file
            (void)hipFree(dall.p);
            dall.p = nullptr;
        }
    }
    if (nsym_total == 0) {
        if (pend_bits && (rc = fout.write_now(&pend, 1, written))) return rc;
        written += pend_bits ? 1 : 0;
    } else if (!resident) {
        // ---- pass 2: pack chunk by chunk at the running bit offset
        const auto tu = Clock::now();
        if ((rc = hz_codebook_upload_encode(c, cb.get()))) return rc;
        g_timing.host_ms += ms_since(tu);
        const uint64_t csym = chunk / 2;
        const uint64_t out_cap = ((32 + csym * (uint64_t)cb->max_len + 31) / 32 + 1) * 4;
        DevBuf dout[2], didx;
        PinnedBuf hout[2];
        const auto tb = Clock::now();
        for (int i = 0; i < 2; ++i) {
            if (!din[i].p && (rc = din[i].alloc(chunk + 16))) return rc;
            if ((rc = dout[i].alloc(out_cap))) return rc;
            if ((rc = hout[i].alloc(out_cap))) return rc;
        }
        if (!sink && (rc = didx.alloc(hz_index_bytes(csym)))) return rc;
        g_timing.alloc_ms += ms_since(tb);
        WriterDrain wdrain{fout};
        DrainGuard drain_out(c->stream);
        StreamGuard cs;  // copy-out stream
        HZ_TRY(hipStreamCreateWithFlags(&cs.s, hipStreamNonBlocking));
        EventPair packed, copied;
        if ((rc = packed.create()) || (rc = copied.create())) return rc;
        if (fseek(fp, 0, SEEK_SET) != 0) return HZ_EIO;
        uint32_t sbit = pend_bits;                       // bit of the chunk's first code in its first word
        if ((rc = read_exact(fp, hin[0].p, std::min(chunk, body)))) return rc;
        int wbuf = -1;          // chunk waiting for its write: buffer, bytes
        uint64_t wbytes = 0;
        uint64_t emitted = 0;   // payload bytes of the chunks before this one
        for (uint64_t off = 0, k = 0; off < body; off += chunk, ++k) {
            const int b = (int)(k & 1);
            const uint64_t len = std::min(chunk, body - off);
            hipEvent_t t0 = spans.mark(c->stream);
            HZ_TRY(hipMemcpyAsync(din[b].p, hin[b].p, len, hipMemcpyHostToDevice, c->stream));
            spans.add(t0, spans.mark(c->stream), &g_timing.h2d_ms);
            if (k >= 2) HZ_TRY(hipStreamWaitEvent(c->stream, copied.e[b], 0));  // dout[b] copied out
            hipEvent_t t1 = spans.mark(c->stream);
            rc = sink ? hz_pack_seek(c, (const uint8_t*)din[b].p, len, sbit, lead, (uint8_t*)dout[b].p, out_cap, nullptr,
                                     off / 2, 8 * emitted, nsym_total, (uint64_t*)dseek.p)
                      : hz_pack(c, (const uint8_t*)din[b].p, len, sbit, lead, (uint8_t*)dout[b].p, out_cap, (uint64_t*)didx.p);
            if (rc) return rc;
            spans.add(t1, spans.mark(c->stream), &g_timing.kernel_ms);
            HZ_TRY(hipEventRecord(packed.e[b], c->stream));
            const uint64_t nb = (len / 2 + 2047) / 2048;
            uint64_t end_bit = 0;
            // the chunk's end: the index's last start[] word or, in the table, the entry after its last block
            const uint64_t* d_end = sink ? (const uint64_t*)dseek.p + off / 2 / kBlockSyms + nb : (const uint64_t*)didx.p + nb;
            HZ_TRY(hipMemcpyAsync(&end_bit, d_end, 8, hipMemcpyDeviceToHost, c->stream));
            // host work beside the upload and pack: the previous chunk's write, the next chunk's fread
            if (wbuf >= 0) {
                HZ_TRY(hipEventSynchronize(copied.e[wbuf]));
                if ((rc = fout.wait())) return rc;  // hout[b] (two chunks back) is free again after this
                fout.start(hout[wbuf].p, wbytes, written);
                written += wbytes;
                wbuf = -1;
            }
            const uint64_t next = off + len;
            if (next < body && (rc = read_exact(fp, hin[1 - b].p, std::min(chunk, body - next)))) return rc;
            if ((rc = hz_ctx_sync(c))) return rc;
            spans.fold();
            if (sink) end_bit -= 8 * emitted;  // the table counts from the payload's first byte
            const bool last = next >= body;
            const uint64_t bytes = last ? (end_bit + 7) / 8 : end_bit / 32 * 4;  // complete words until the end
            sbit = (uint32_t)(end_bit % 32);
            lead = 0;
            if (sbit && !last) {  // the partial word, carried into the next chunk as its lead bits
                uint32_t w = 0;
                HZ_TRY(hipMemcpyAsync(&w, (const uint8_t*)dout[b].p + bytes, 4, hipMemcpyDeviceToHost, c->stream));
                if ((rc = hz_ctx_sync(c))) return rc;
                lead = __builtin_bswap32(w) >> (32 - sbit);
            }
            if ((rc = fout.wait())) return rc;  // hout[b] may still be leaving from two chunks back
            HZ_TRY(hipStreamWaitEvent(cs.s, packed.e[b], 0));
            hipEvent_t t2 = spans.mark(cs.s);
            if (bytes) HZ_TRY(hipMemcpyAsync(hout[b].p, dout[b].p, bytes, hipMemcpyDeviceToHost, cs.s));
            spans.add(t2, spans.mark(cs.s), &g_timing.d2h_ms);
            HZ_TRY(hipEventRecord(copied.e[b], cs.s));
            wbuf = b;
            wbytes = bytes;
            emitted += bytes;
        }
        if (wbuf >= 0) {
            HZ_TRY(hipEventSynchronize(copied.e[wbuf]));
            if ((rc = fout.wait())) return rc;
            fout.start(hout[wbuf].p, wbytes, written);
            written += wbytes;
        }
        if ((rc = fout.wait())) return rc;
        HZ_TRY(hipStreamSynchronize(cs.s));
    }
    if (sink && nsym_total) {  // the table, once
        hipEvent_t t3 = spans.mark(c->stream);
        HZ_TRY(hipMemcpyAsync(sink->seek, dseek.p, hz_seek_bytes(nsym_total), hipMemcpyDeviceToHost, c->stream));
        spans.add(t3, spans.mark(c->stream), &g_timing.d2h_ms);
        if ((rc = hz_ctx_sync(c))) return rc;
    }
    if ((rc = fout.close())) return rc;
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

// A streamed call: the thread's timing record started afresh, the body guarded, its wall time kept.
template <typename F>
static int timed_call(F&& body) {
    g_timing = hz_stream_timing();
    const auto t0 = Clock::now();
    const int rc = guarded(body);
    g_timing.total_ms = ms_since(t0);
    return rc;
}

extern "C" int hz_archive_stream(const char* in_path, const char* out_path, uint64_t chunk_bytes, int verbose) {
    return timed_call([&] { return hz_archive_stream_impl(in_path, out_path, chunk_bytes, verbose, false); });
}

// The header of a file to extract: parsed on the device (k_hdr_*, 0.05 ms for
// U = 65 536 against 0.25+ ms on the host; profiles/r03_codebook_*), the codebook
// and the info copied back for the host-built decode tables. HZ_HOST_HEADER=1
// parses on the host. Both follow Decompressor.cu:65-103 and reject the same files.
static int parse_header_for_extract(const std::vector<uint8_t>& head, hz_codebook* cb, hz_header_info* info) {
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
    info->n = hi[0];
    info->payload_byte = hi[1];
    info->payload_bit = (uint32_t)hi[2];
    info->is_odd = (uint32_t)hi[3];
    info->last_byte = (uint32_t)hi[4];
    info->nsym = (uint32_t)hi[5];
    g_timing.host_ms += ms_since(tp);
    return HZ_OK;
}

// Streaming extract: the payload passes through a device window of chunk_bytes.
// Each round decodes as many symbols as the window surely holds (the file's
// mean code length with a margin; a round whose codes overrun the window is
// redone at the max_len bound), and moves the unconsumed tail of the window to
// the front of the other buffer before refilling it. The host's fread of the
// next window overlaps the decode, and its fwrite of a round's output overlaps
// the next round's upload and index-less decode (hz_decode_indexless).
//
// With a SeekSink the rounds also leave the file's seek table (hz_extract_stream_seek): every round is
// hz_decode_indexless_seek at sym_base = the symbols done and bit_base = 8 x the payload bytes the
// earlier rounds consumed, into one device table copied out once at the end. A round redone after an
// overrun rewrites its entries, and later rounds overwrite what the overrun attempt wrote past its
// window. Without an out_path (sink only) nothing is decoded, copied out or written.
static int hz_extract_stream_impl(const char* in_path, const char* out_path, uint64_t chunk_bytes, int verbose,
                                  const SeekSink* sink = nullptr) {
    if (!in_path || (!out_path && !sink) || chunk_bytes < 4096) return HZ_EINVAL;
    if (sink && !sink->nsym) return HZ_EINVAL;
    const bool write = out_path != nullptr;
    chunk_bytes &= ~(uint64_t)15;
    struct stat st;
    if (stat(in_path, &st) != 0) return HZ_ENOENT;
    const uint64_t fsize = (uint64_t)st.st_size;
    FILE* fp = fopen(in_path, "rb");
    if (!fp) return HZ_EIO;
    std::unique_ptr<FILE, int (*)(FILE*)> fin(fp, fclose);
    // the header is at most 12 + 65536 * (3 + 8) bytes
    std::vector<uint8_t> head(std::min<uint64_t>(fsize, 1u << 20));
    int rc = read_exact(fp, head.data(), head.size());
    if (rc) return rc;
    std::unique_ptr<hz_codebook> cb(new hz_codebook());
    hz_header_info info;
    if ((rc = parse_header_for_extract(head, cb.get(), &info))) return rc;
    if (sink) {
        *sink->nsym = info.n / 2;
        if (hz_seek_bytes(info.n / 2) && (!sink->seek || sink->cap_bytes < hz_seek_bytes(info.n / 2))) return HZ_ECAP;
    }
    FileWriter fout;
    if (write && (rc = fout.open(out_path))) return rc;
    if (write) {
        // Reserve no more than the payload can decode to: a header whose N overstates it (corrupt or
        // crafted) must not allocate disk before the decode rejects it. nsym codewords need at least
        // nsym * min_len payload bits.
        const uint64_t pay_bits = fsize > info.payload_byte ? (fsize - info.payload_byte) * 8 - info.payload_bit : 0;
        const uint64_t min_len = std::max<uint32_t>(cb->min_len, 1);
        const uint64_t most = 2 * (pay_bits / min_len) + (info.is_odd ? 1 : 0);
        fout.reserve(std::min<uint64_t>(info.n, most));
    }
    uint64_t out_off = 0;
    const uint64_t nsym = info.n / 2;
    if (nsym > 0) {
        hz_ctx* c;
        const auto tc = Clock::now();
        rc = default_ctx(&c);
        g_timing.alloc_ms += ms_since(tc);
        if (rc) return rc;
        HZ_TRY(hipSetDevice(c->device));
        Spans spans;
        const auto tu = Clock::now();
        if ((rc = hz_codebook_upload_decode(c, cb.get()))) return rc;
        g_timing.host_ms += ms_since(tu);
        const uint64_t W = chunk_bytes;               // window bytes
        const uint64_t pay_total = fsize > info.payload_byte ? fsize - info.payload_byte : 0;
        const uint64_t max_len = std::max<uint32_t>(cb->max_len, 1);
        // mean bits per symbol of this file, 3% margin (a mispredicted round is redone exactly)
        const double mean = pay_total ? ((double)pay_total * 8 - info.payload_bit) / (double)nsym : (double)max_len;
        const uint64_t sym_cap = std::max<uint64_t>(W / 2, kBlockSyms);  // output per round <= W bytes
        DevBuf dwin[2], didx, dout, dseek;
        PinnedBuf hin, hout[2];  // hout: a round's output leaves (parallel writes) beside the next round
        int ob = 0;
        const auto ta = Clock::now();
        for (int i = 0; i < 2; ++i)
            if ((rc = dwin[i].alloc(W + 16))) return rc;
        if ((rc = didx.alloc(16))) return rc;  // the round's end bit
        if (write && (rc = dout.alloc(2 * sym_cap + 16))) return rc;
        if (sink && (rc = dseek.alloc(hz_seek_bytes(nsym)))) return rc;
        if ((rc = hin.alloc(W))) return rc;
        for (int i = 0; i < 2; ++i)
            if (write && (rc = hout[i].alloc(2 * sym_cap))) return rc;
        WriterDrain wdrain{fout};
        g_timing.alloc_ms += ms_since(ta);
        DrainGuard drain(c->stream);
        if (fseek(fp, (long)info.payload_byte, SEEK_SET) != 0) return HZ_EIO;
        uint64_t file_left = pay_total, have = 0, done = 0;
        uint64_t consumed = 0;  // payload bytes before the window (the seek entries' bit base)
        uint64_t bit = info.payload_bit;
        int cur = 0;
        // symbols this round decodes from the window: what it surely holds
        auto round_syms = [&]() {
            const uint64_t left = nsym - done, avail = have * 8 - bit;
            if (file_left == 0) return std::min(left, sym_cap);
            uint64_t k = (uint64_t)((double)avail / (mean * 1.03));
            k = std::min(std::min(left, sym_cap), k);
            // whole blocks when the window holds at least one; a smaller window keeps k
            if (k < left && k >= (uint64_t)kBlockSyms) k = k / kBlockSyms * kBlockSyms;
            return std::max<uint64_t>(k, 1);
        };
        uint64_t end_bit = 0;
        // a round: the window's first kk codewords decoded index-less into dout, and their end bit
        auto launch_index = [&](uint64_t kk) -> int {
            hipEvent_t t0 = spans.mark(c->stream);
            int r2 = sink ? hz_decode_indexless_seek(c, (const uint8_t*)dwin[cur].p, have, bit, kk, (uint8_t*)dout.p,
                                                     (uint64_t*)didx.p, done, 8 * consumed, nsym, (uint64_t*)dseek.p)
                          : hz_decode_indexless(c, (const uint8_t*)dwin[cur].p, have, bit, kk, (uint8_t*)dout.p,
                                                (uint64_t*)didx.p);
            if (r2) return r2;
            spans.add(t0, spans.mark(c->stream), &g_timing.kernel_ms);
            HZ_TRY(hipMemcpyAsync(&end_bit, didx.p, 8, hipMemcpyDeviceToHost, c->stream));
            return HZ_OK;
        };
        // first fill
        uint64_t r = std::min(W, file_left);
        if ((rc = read_exact(fp, hin.p, r))) return rc;
        HZ_TRY(hipMemsetAsync(dwin[cur].p, 0, W + 16, c->stream));
        {
            hipEvent_t t0 = spans.mark(c->stream);
            HZ_TRY(hipMemcpyAsync(dwin[cur].p, hin.p, r, hipMemcpyHostToDevice, c->stream));
            spans.add(t0, spans.mark(c->stream), &g_timing.h2d_ms);
        }
        have = r;
        file_left -= r;
        uint64_t k = round_syms();
        if ((rc = launch_index(k))) return rc;
        while (done < nsym) {
            if ((rc = hz_ctx_sync(c))) return rc;
            if (end_bit > have * 8 && file_left > 0) {  // the round's codes overran the window: redo at the bound
                k = std::max<uint64_t>((have * 8 - bit) / max_len, 1);
                if ((rc = launch_index(k)) || (rc = hz_ctx_sync(c))) return rc;
            }
            if (end_bit > have * 8) return HZ_EFORMAT;    // truncated file
            if (write) {
                hipEvent_t t1 = spans.mark(c->stream);
                HZ_TRY(hipMemcpyAsync(hout[ob].p, dout.p, 2 * k, hipMemcpyDeviceToHost, c->stream));
                spans.add(t1, spans.mark(c->stream), &g_timing.d2h_ms);
            }
            // move the unconsumed tail to the other window and read the refill behind the decode
            const uint64_t used = end_bit / 8, tail = have - used;
            const int nxt = cur ^ 1;
            const bool more = done + k < nsym;
            r = 0;
            if (more) {
                if (tail) HZ_TRY(hipMemcpyAsync(dwin[nxt].p, (const uint8_t*)dwin[cur].p + used, tail,
                                                hipMemcpyDeviceToDevice, c->stream));
                r = std::min(W - tail, file_left);
                if ((rc = read_exact(fp, hin.p, r))) return rc;
            }
            if ((rc = hz_ctx_sync(c))) return rc;    // decode, output copy and tail move done
            spans.fold();
            const uint64_t kdone = k;
            if (more) {  // next window and its index build, beside this round's fwrite
                if (r < W - tail) HZ_TRY(hipMemsetAsync((uint8_t*)dwin[nxt].p + tail + r, 0, W + 16 - tail - r, c->stream));
                if (r) {
                    hipEvent_t t2 = spans.mark(c->stream);
                    HZ_TRY(hipMemcpyAsync((uint8_t*)dwin[nxt].p + tail, hin.p, r, hipMemcpyHostToDevice, c->stream));
                    spans.add(t2, spans.mark(c->stream), &g_timing.h2d_ms);
                }
                have = tail + r;
                file_left -= r;
                consumed += used;
                bit = end_bit % 8;
                cur = nxt;
                done += kdone;
                k = round_syms();
                if ((rc = launch_index(k))) return rc;
            } else {
                done += kdone;
            }
            if ((rc = fout.wait())) return rc;  // the previous round's write: hout[ob ^ 1] free for the next
            if (write) fout.start(hout[ob].p, 2 * kdone, out_off);
            out_off += 2 * kdone;
            ob ^= 1;
        }
        if ((rc = fout.wait())) return rc;
        if (sink) {  // the table, once
            hipEvent_t t3 = spans.mark(c->stream);
            HZ_TRY(hipMemcpyAsync(sink->seek, dseek.p, hz_seek_bytes(nsym), hipMemcpyDeviceToHost, c->stream));
            spans.add(t3, spans.mark(c->stream), &g_timing.d2h_ms);
            if ((rc = hz_ctx_sync(c))) return rc;
        }
        spans.fold();
    }
    if (write && info.is_odd) {
        const uint8_t b = (uint8_t)info.last_byte;
        if ((rc = fout.write_now(&b, 1, out_off))) return rc;
    }
    if (write && (rc = fout.close())) return rc;
    if (verbose) std::cout << "Decompression is complete" << std::endl;
    return HZ_OK;
}

extern "C" int hz_extract_stream(const char* in_path, const char* out_path, uint64_t chunk_bytes, int verbose) {
    return timed_call([&] { return hz_extract_stream_impl(in_path, out_path, chunk_bytes, verbose); });
}

extern "C" int hz_extract_stream_seek(const char* in_path, const char* out_path, uint64_t chunk_bytes, int verbose,
                                      uint64_t* seek, uint64_t cap_bytes, uint64_t* nsym) {
    if (!in_path || !nsym || chunk_bytes < 4096) return HZ_EINVAL;
    const SeekSink sink{seek, cap_bytes, nsym};
    return timed_call([&] { return hz_extract_stream_impl(in_path, out_path, chunk_bytes, verbose, &sink); });
}

extern "C" int hz_archive_stream_seek(const char* in_path, const char* out_path, uint64_t chunk_bytes, int verbose,
                                      uint64_t* seek, uint64_t seek_cap_bytes, uint64_t* nsym) {
    if (!nsym) return HZ_EINVAL;
    const SeekSink sink{seek, seek_cap_bytes, nsym};
    return timed_call([&] { return hz_archive_stream_impl(in_path, out_path, chunk_bytes, verbose, false, &sink); });
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
    const char* ce = getenv("HZ_ARCHIVE_CHUNK");
    const uint64_t chunk = ce && strtoull(ce, nullptr, 10) >= 64 ? strtoull(ce, nullptr, 10) : kArchiveChunk;
    if (sink) {  // a table too small is refused here: whatever stands at outname stays as it is
        *sink->nsym = (uint64_t)st.st_size / 2;
        if (sink->cap_bytes < hz_seek_bytes(*sink->nsym) || (!sink->seek && *sink->nsym)) return HZ_ECAP;
    }
    // resident: the input stays on the device between the passes when it fits
    const int rc = timed_call([&] { return hz_archive_stream_impl(path, outname.c_str(), chunk, verbose, true, sink); });
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
    const char* we = getenv("HZ_EXTRACT_WINDOW");
    const uint64_t window = we && strtoull(we, nullptr, 10) >= 4096 ? strtoull(we, nullptr, 10) : kExtractWindow;
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
