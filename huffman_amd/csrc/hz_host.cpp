// hz_host.cpp -- C ABI implementation: contexts, table uploads and every stream-ordered stage call. (The
// whole-buffer flows behind hz_*_host are hz_image.cpp, the streaming `archive` / `extract` hz_stream.cpp.)
// Device work always runs through the gfx950 kernels of the hz_*.hip files; there is no CPU fallback
// for any stage.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>

#include "hz_host.h"

using namespace hz;

extern "C" const char* hz_strerror(int st) {
    switch (st) {
        case HZ_OK: return "ok";
        case HZ_EINVAL: return "invalid argument";
        case HZ_ENOMEM: return "out of memory";
        case HZ_EHIP: return "HIP runtime error";
        case HZ_ETOOLONG: return "code longer than supported";
        case HZ_EFORMAT: return "malformed compressed stream";
        case HZ_ECAP: return "output capacity too small";
        case HZ_ETIMEOUT: return "device wait timed out";
        case HZ_EIO: return "file I/O error";
        case HZ_ENODEV: return "no usable gfx950 device";
        case HZ_ENOENT: return "input file does not exist";
        case HZ_ECHECKSUM: return "decoded block does not match its checksum";
        default: return "unknown error";
    }
}

extern "C" int hz_version(void) { return 1; }

static void free_tables(Tables& t) {
    void* const owned[] = {t.d_enc_lds, t.d_enc_wide, t.d_enc_esc, t.d_len8,      t.d_lenpair,  t.d_dec_lds,  t.d_dec_l2,
                           t.d_walk_lds, t.d_walk_esc, t.d_walk8,   t.d_chain_lds, t.d_chain_l2, t.d_chain_esc};
    for (void* p : owned) (void)hipFree(p);
    t = Tables();
}

extern "C" int hz_ctx_create(int device, void* stream, hz_ctx** out) {
    if (!out) return HZ_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device || device < 0) return HZ_ENODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return HZ_ENODEV;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return HZ_ENODEV;
    std::unique_ptr<hz_ctx> c(new hz_ctx());
    c->device = device;
    c->ncu = prop.multiProcessorCount;
    c->chain = chain_state_create();
    HZ_TRY(hipSetDevice(device));
    if (stream) {
        c->stream = (hipStream_t)stream;
    } else {
        HZ_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    HZ_TRY(hipMalloc(&c->d_err, 16));
    HZ_TRY(hipMemset(c->d_err, 0, 16));
    HZ_TRY(hipHostMalloc(&c->h_err, 16, hipHostMallocDefault));
    *c->h_err = 0;
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 2; ++j) HZ_TRY(hipEventCreate(&c->ev[i][j]));
    *out = c.release();
    return HZ_OK;
}

extern "C" int hz_ctx_destroy(hz_ctx* c) {
    if (!c) return HZ_EINVAL;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    free_tables(c->t);
    for (Staging* st : {&c->stage_enc, &c->stage_dec, &c->stage_walk}) {
        if (st->done) (void)hipEventDestroy(st->done);
        (void)hipHostFree(st->p);
    }
    chain_state_destroy(c->chain);
    (void)hipFree(c->d_desc);
    (void)hipFree(c->d_err);
    (void)hipFree(c->d_thr);
    (void)hipFree(c->d_cbws);
    (void)hipHostFree(c->h_err);
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 2; ++j) (void)hipEventDestroy(c->ev[i][j]);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return HZ_OK;
}

extern "C" int hz_ctx_set_stream(hz_ctx* c, void* stream) {
    if (!c || !stream) return HZ_EINVAL;
    if (c->own_stream) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamDestroy(c->stream);
        c->own_stream = false;
    }
    c->stream = (hipStream_t)stream;
    return HZ_OK;
}

extern "C" int hz_ctx_sync(hz_ctx* c) {
    if (!c) return HZ_EINVAL;
    (void)hipSetDevice(c->device);
    HZ_TRY(hipStreamSynchronize(c->stream));
    if (*c->h_err) {
        const uint32_t e = *c->h_err;
        *c->h_err = 0;
        HZ_TRY(hipMemset(c->d_err, 0, 16));
        return (e & 4u) ? HZ_ECAP : (e & 8u) ? HZ_ETIMEOUT : (e & 16u) ? HZ_EINVAL : (e & 32u) ? HZ_ETOOLONG : HZ_EFORMAT;
    }
    return HZ_OK;
}

// Stage timing events: skipped while the stream is being captured into a graph (the stage calls
// themselves are stream-ordered and capturable; hz_last_kernel_ms then reports the last eager call).
static hipError_t stage_event(hz_ctx* c, int stage, int which) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    hipError_t e = hipStreamIsCapturing(c->stream, &st);
    if (e != hipSuccess) return e;
    if (st != hipStreamCaptureStatusNone) return hipSuccess;
    return hipEventRecord(c->ev[stage][which], c->stream);
}

static int arm_err_check(hz_ctx* c) {
    HZ_TRY(hipMemcpyAsync(c->h_err, c->d_err, 4, hipMemcpyDeviceToHost, c->stream));
    return HZ_OK;
}

// A stage's launches (their hipError_t; `what` names them in the HZ_DEBUG message) between its two
// timing events; then the stage has a time to report and, with `check`, the device's error word follows
// the launches home (hz_ctx_sync reads it).
template <typename F>
static int timed_stage(hz_ctx* c, int stage, const char* what, F&& stage_launch, bool check = true) {
    HZ_TRY(stage_event(c, stage, 0));
    const hipError_t e = stage_launch();
    if (e != hipSuccess) return hz_hip_fail(e, what, __FILE_NAME__, __LINE__);
    HZ_TRY(stage_event(c, stage, 1));
    c->ev_used[stage] = true;
    return check ? arm_err_check(c) : HZ_OK;
}

// Stream-ordered store of a u64 to device memory.
static hipError_t put_u64(uint64_t* d_dst, uint64_t v, hipStream_t s) {
    const hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_dst), (int)(uint32_t)v, 1, s);
    if (e != hipSuccess) return e;
    return hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(reinterpret_cast<uint32_t*>(d_dst) + 1),
                             (int)(uint32_t)(v >> 32), 1, s);
}

// The workspace of the device codebook builder, header writer and header parser, on first use.
static int ensure_cbws(hz_ctx* c) {
    if (!c->d_cbws) HZ_TRY(hipMalloc(&c->d_cbws, codebook_ws_words() * sizeof(unsigned long long)));
    return HZ_OK;
}

extern "C" int hz_last_kernel_ms(hz_ctx* c, int stage, float* ms) {
    if (!c || !ms || stage < 0 || stage > 4) return HZ_EINVAL;
    if (!c->ev_used[stage]) { *ms = 0.f; return HZ_OK; }
    HZ_TRY(hipEventElapsedTime(ms, c->ev[stage][0], c->ev[stage][1]));
    return HZ_OK;
}

extern "C" int hz_hist16(hz_ctx* c, const uint8_t* d_in, uint64_t n, uint64_t* d_hist, int accumulate) {
    if (!c || !d_hist || (n && !d_in)) return HZ_EINVAL;
    HZ_TRY(hipSetDevice(c->device));
    if (!accumulate) HZ_TRY(hipMemsetAsync(d_hist, 0, HZ_NSYM * sizeof(uint64_t), c->stream));
    return timed_stage(c, HZ_STAGE_HIST, "launch_hist16", [&] {
        return launch_hist16(d_in, n, reinterpret_cast<unsigned long long*>(d_hist), c->ncu, c->stream);
    }, false);  // (the kernel reports no errors)
}

extern "C" uint64_t hz_block_sums_bytes(uint64_t n) {
    return 4 * (n / HZ_SUM_BLOCK_BYTES + (n % HZ_SUM_BLOCK_BYTES ? 1 : 0));
}

extern "C" int hz_block_sums(hz_ctx* c, const uint8_t* d_in, uint64_t n, uint32_t* d_sums) {
    if (!c) return HZ_EINVAL;
    if (n == 0) return HZ_OK;
    if (!d_in || !d_sums || (((uintptr_t)d_in) & 15) || (((uintptr_t)d_sums) & 3)) return HZ_EINVAL;
    HZ_TRY(hipSetDevice(c->device));
    const hipError_t e = launch_block_sums(d_in, n, d_sums, c->ncu, c->stream);  // (the kernel reports no errors)
    return e == hipSuccess ? HZ_OK : hz_hip_fail(e, "launch_block_sums", __FILE_NAME__, __LINE__);
}

extern "C" int hz_block_sums_check(hz_ctx* c, const uint8_t* d_in, uint64_t n, const uint32_t* d_expect, uint64_t block_base,
                                   uint64_t* d_bad) {
    if (!c) return HZ_EINVAL;
    if (n == 0) return HZ_OK;
    if (!d_in || !d_expect || !d_bad || (((uintptr_t)d_in) & 15) || (((uintptr_t)d_expect) & 3) || (((uintptr_t)d_bad) & 7))
        return HZ_EINVAL;
    HZ_TRY(hipSetDevice(c->device));
    const hipError_t e = launch_block_sums_check(d_in, n, d_expect, block_base, reinterpret_cast<unsigned long long*>(d_bad),
                                                 c->ncu, c->stream);  // (the kernel reports no errors)
    return e == hipSuccess ? HZ_OK : hz_hip_fail(e, "launch_block_sums_check", __FILE_NAME__, __LINE__);
}

extern "C" int hz_block_sums_mark(hz_ctx* c, uint8_t* d_data, uint64_t n, const uint32_t* d_expect, uint64_t block_base,
                                  uint32_t* d_bits, uint32_t flags) {
    if (!c || (flags & ~HZ_SUMS_ZERO_BAD)) return HZ_EINVAL;
    if (n == 0) return HZ_OK;
    if (!d_data || !d_expect || !d_bits || (((uintptr_t)d_data) & 15) || (((uintptr_t)d_expect) & 3) || (((uintptr_t)d_bits) & 3))
        return HZ_EINVAL;
    HZ_TRY(hipSetDevice(c->device));
    const hipError_t e = launch_block_sums_mark(d_data, n, d_expect, block_base, d_bits, (flags & HZ_SUMS_ZERO_BAD) != 0, c->ncu,
                                                c->stream);  // (the kernel reports no errors)
    return e == hipSuccess ? HZ_OK : hz_hip_fail(e, "launch_block_sums_mark", __FILE_NAME__, __LINE__);
}

extern "C" uint64_t hz_ranges_bytes(uint64_t n) { return range_geom(n / 2).bytes; }

extern "C" int hz_hist16_ranges(hz_ctx* c, const uint8_t* d_in, uint64_t n, uint64_t* d_hist, int accumulate,
                                void* d_ranges) {
    if (!c || !d_hist || (n && !d_in)) return HZ_EINVAL;
    if (!range_geom(n / 2).bytes) return hz_hist16(c, d_in, n, d_hist, accumulate);  // too small for a plan
    if (!d_ranges || (((uintptr_t)d_in) & 15) || (((uintptr_t)d_ranges) & 15)) return HZ_EINVAL;
    HZ_TRY(hipSetDevice(c->device));
    if (!accumulate) HZ_TRY(hipMemsetAsync(d_hist, 0, HZ_NSYM * sizeof(uint64_t), c->stream));
    return timed_stage(c, HZ_STAGE_HIST, "launch_hist16_ranges", [&] {
        return launch_hist16_ranges(d_in, n, reinterpret_cast<unsigned long long*>(d_hist), d_ranges, c->d_err,
                                    c->stream);
    });
}

extern "C" int hz_codebook_build_device(hz_ctx* c, const uint64_t* d_hist, hz_codebook* d_cb) {
    if (!c || !d_hist || !d_cb) return HZ_EINVAL;
    HZ_TRY(hipSetDevice(c->device));
    if (int rc = ensure_cbws(c)) return rc;
    HZ_TRY(launch_codebook(reinterpret_cast<const unsigned long long*>(d_hist), d_cb, c->d_cbws, c->d_err, c->stream));
    return arm_err_check(c);
}

#ifdef HZ_CB_PROF  // variant builds only: k_cb_generate's phase timestamps (tools/debug/cb_prof.py)
extern "C" int hz_debug_cb_prof(hz_ctx* c, uint64_t* out) {
    HZ_TRY(hipStreamSynchronize(c->stream));
    HZ_TRY(hipMemcpy(out, c->d_cbws + 65536, 512 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return HZ_OK;
}
#endif

extern "C" int hz_header_write_device(hz_ctx* c, const hz_codebook* d_cb, uint64_t n, uint8_t last_byte,
                                      uint8_t* d_out, uint64_t cap, uint64_t* d_info) {
    if (!c || !d_cb || !d_out || !d_info || (((uintptr_t)d_out) & 3)) return HZ_EINVAL;
    HZ_TRY(hipSetDevice(c->device));
    if (int rc = ensure_cbws(c)) return rc;
    HZ_TRY(launch_header_write(d_cb, n, last_byte, d_out, cap, reinterpret_cast<unsigned long long*>(d_info), c->d_cbws,
                               c->d_err, c->stream));
    return arm_err_check(c);
}

extern "C" int hz_header_parse_device(hz_ctx* c, const uint8_t* d_file, uint64_t len, hz_codebook* d_cb,
                                      uint64_t* d_info) {
    if (!c || !d_file || !d_cb || !d_info) return HZ_EINVAL;
    HZ_TRY(hipSetDevice(c->device));
    if (int rc = ensure_cbws(c)) return rc;
    HZ_TRY(launch_header_parse(d_file, len, d_cb, reinterpret_cast<unsigned long long*>(d_info), c->d_cbws, c->d_err,
                               c->stream));
    return arm_err_check(c);
}

// Device tables live in per-context buffers that only grow; host images are
// staged in pinned memory and copied asynchronously on the context stream (one
// scatter kernel per set), so an upload never synchronises and the decode tables
// can be built on the host while the pack kernel runs (bench step: upload_encode
// -> pack -> upload_decode -> decode). Stream order keeps in-flight kernels on the
// previous tables; a staging buffer is reused only after its last copy's event.
static int staging_begin(Staging& st) {
    if (!st.done) HZ_TRY(hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
    else HZ_TRY(hipEventSynchronize(st.done));
    st.used = 0;
    st.pend.clear();  // (a set never flushed is dropped)
    return HZ_OK;
}

// The staged segments to their tables, stream-ordered. Under stream capture the copy is captured and
// the segments stay pending, so a later uncaptured call copies them again.
static int staging_flush(hz_ctx* c, Staging& st) {
    if (st.pend.empty()) return HZ_OK;
    HZ_TRY(stage_scatter(st.p, st.pend.data(), (int)st.pend.size(), c->stream));
    HZ_TRY(hipEventRecord(st.done, c->stream));
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    HZ_TRY(hipStreamIsCapturing(c->stream, &cs));
    if (cs == hipStreamCaptureStatusNone) st.pend.clear();
    return HZ_OK;
}

// An image into its slot of the staging buffer: its one host copy. An empty image (a table the
// codebook does not have) takes no slot and leaves its device table alone.
template <typename T>
static int stage_copy(hz_ctx* c, Staging& st, T** dptr, size_t* dcap, const std::vector<T>& v) {
    const size_t bytes = v.size() * sizeof(T);
    if (!bytes) return HZ_OK;
    if (*dcap < bytes) {
        HZ_TRY(hipStreamSynchronize(c->stream));
        (void)hipFree(*dptr);
        *dptr = nullptr;
        HZ_TRY(hipMalloc(dptr, bytes));
        *dcap = bytes;
    }
    if (st.used + bytes > st.cap) {
        // grow (rare): the segments staged so far move along (no copy of this staging is in flight:
        // staging_begin waited for the last one)
        uint8_t* np = nullptr;
        const size_t ncap = std::max(st.cap * 2, st.used + bytes + (1u << 20));
        HZ_TRY(hipHostMalloc(&np, ncap, hipHostMallocDefault));
        if (st.used) memcpy(np, st.p, st.used);
        (void)hipHostFree(st.p);
        st.p = np;
        st.cap = ncap;
    }
    static_assert(sizeof(T) % 4 == 0, "tables of 4-byte words (k_stage_scatter)");
    memcpy(st.p + st.used, v.data(), bytes);
    st.pend.push_back(StageSeg{(void*)*dptr, (uint64_t)st.used, (uint64_t)bytes});
    st.used += (bytes + 255) & ~(size_t)255;
    return HZ_OK;
}

extern "C" int hz_codebook_upload_encode(hz_ctx* c, const hz_codebook* cb) {
    return guarded([&]() -> int {
        if (!c || !cb) return HZ_EINVAL;
        if (cb->max_len > HZ_MAXLEN) return HZ_ETOOLONG;
        HZ_TRY(hipSetDevice(c->device));
        Tables& t = c->t;
        t.enc_mode = -1;
        if (cb->nsym == 0) return HZ_OK;
        EncImages e;
        build_enc_images(cb, e);
        Staging& st = c->stage_enc;
        int rc;
        if ((rc = staging_begin(st)) || (rc = stage_copy(c, st, &t.d_enc_lds, &c->cap_enc_lds, e.lds)) ||
            (rc = stage_copy(c, st, &t.d_enc_esc, &c->cap_enc_esc, e.esc)) ||
            (rc = stage_copy(c, st, &t.d_enc_wide, &c->cap_enc_wide, e.wide)) ||
            (rc = stage_copy(c, st, &t.d_len8, &c->cap_len8, e.len8)) ||
            (rc = stage_copy(c, st, &t.d_lenpair, &c->cap_lenpair, e.lenpair)))
            return rc;
        t.max_len = (int)cb->max_len;
        t.min_len = (int)cb->min_len;
        t.enc_avg_bits = e.enc_avg_bits;
        t.enc_lds_bytes = (uint32_t)(e.lds.size() * 4);
        t.hot_mask = e.hot_mask;
        if ((rc = staging_flush(c, st))) return rc;
        t.enc_mode = e.mode;
        return HZ_OK;
    });
}

extern "C" int hz_codebook_upload_decode(hz_ctx* c, const hz_codebook* cb) {
    return guarded([&]() -> int {
        if (!c || !cb) return HZ_EINVAL;
        if (cb->max_len > HZ_MAXLEN) return HZ_ETOOLONG;
        HZ_TRY(hipSetDevice(c->device));
        Tables& t = c->t;
        t.dec_mode = -1;
        chain_invalidate(c->chain);  // its arguments point at the tables replaced here
        c->fx.on = false;
        if (cb->nsym == 0) return HZ_OK;
        DecImages d;
        int rc = build_dec_images(cb, d);
        if (rc) return rc;
        if ((rc = staging_begin(c->stage_dec)) ||
            (rc = stage_copy(c, c->stage_dec, &t.d_dec_lds, &c->cap_dec_lds, d.lds)) ||
            (rc = stage_copy(c, c->stage_dec, &t.d_dec_l2, &c->cap_dec_l2, d.l2)))
            return rc;
        t.dec_max_len = (int)cb->max_len;
        t.dec_min_len = (int)cb->min_len;
        t.dec_k = d.k;
        t.dec_level_bits = d.level_bits;
        t.dec_avg_bits = d.dec_avg_bits;
        t.dec_lds_bytes = (uint32_t)(d.lds.size() * 4);
        t.dec_l2_entries = d.l2.size();
        if ((rc = staging_flush(c, c->stage_dec))) return rc;
        // the index-less tables (none for FIXED16: positions are arithmetic), staged now and copied by the
        // first call that needs them (staging_flush from hz_decode_indexless, hz_indexless_scan or
        // hz_index_build)
        IndexlessImages x;
        Staging& st = c->stage_walk;
        if ((rc = staging_begin(st)) || (rc = build_indexless_images(cb, d, x)) ||
            (rc = stage_copy(c, st, &t.d_walk_lds, &c->cap_walk_lds, x.walk_lds)) ||
            (rc = stage_copy(c, st, &t.d_walk_esc, &c->cap_walk_esc, x.walk_esc)) ||
            (rc = stage_copy(c, st, &t.d_walk8, &c->cap_walk8, x.walk8)) ||
            (rc = stage_copy(c, st, &t.d_chain_esc, &c->cap_chain_esc, x.chain_esc)) ||
            (rc = stage_copy(c, st, &t.d_chain_lds, &c->cap_chain_lds, x.chain_lds)) ||
            (rc = stage_copy(c, st, &t.d_chain_l2, &c->cap_chain_l2, x.chain_l2)))
            return rc;
        t.walk_lds_bytes = (uint32_t)(x.walk_lds.size() * 4);  // 0: no walker tables
        t.walk_k = x.walk_k;
        t.walk_m = x.walk_m;
        t.walk_bias = x.walk_bias;
        t.walk8_bytes = (uint32_t)(x.walk8.size() * 4);
        t.walk8_k = x.walk8_k;
        t.chain_lds_bytes = 0;  // no chain tables (FIXED16)
        if (!x.walk8.empty()) {
            // the chain decoder's views: the walker's escape table where there is one, a LUT book's own
            // decode tables
            const bool own_lut = !x.chain_lds.empty();
            t.chain_esc = reinterpret_cast<const uint8_t*>(x.chain_esc.empty() ? t.d_walk_esc : t.d_chain_esc);
            t.chain_esc_m = x.chain_esc_m;
            t.chain_lds = own_lut ? t.d_chain_lds : t.d_dec_lds;
            t.chain_l2 = own_lut ? t.d_chain_l2 : t.d_dec_l2;
            t.chain_lds_bytes = own_lut ? (uint32_t)(x.chain_lds.size() * 4) : t.dec_lds_bytes;
            t.chain_k = x.chain_k;
            t.chain_level_bits = x.chain_level_bits;
        }
        t.dec_mode = d.mode;
        return HZ_OK;
    });
}

extern "C" int hz_codebook_upload(hz_ctx* c, const hz_codebook* cb) {
    int rc = hz_codebook_upload_encode(c, cb);
    return rc ? rc : hz_codebook_upload_decode(c, cb);
}

extern "C" int hz_index_format(void) { return HZ_INDEX_FORMAT; }
extern "C" uint64_t hz_index_stride(void) { return kBlockSyms; }
extern "C" uint64_t hz_index_bytes(uint64_t nsym) { return index_bytes(nsym); }
extern "C" uint64_t hz_scratch_bytes(uint64_t nsym) { return pack_scratch_words(nsym) * sizeof(uint64_t); }

// Every call that writes the context's scratch (or reallocates it, or replaces the decode tables) ends
// a pending index-less part (hz_indexless_scan ... hz_indexless_decode): its chain state points there.
static int ensure_scratch(hz_ctx* c, uint64_t words) {
    chain_invalidate(c->chain);
    c->fx.on = false;
    if (c->desc_cap >= words) return HZ_OK;
    HZ_TRY(hipStreamSynchronize(c->stream));
    (void)hipFree(c->d_desc);
    chain_forget_seek_stats(c->chain);
    c->d_desc = nullptr;
    c->desc_cap = 0;
    HZ_TRY(hipMalloc(&c->d_desc, words * sizeof(unsigned long long)));
    c->desc_cap = words;
    return HZ_OK;
}

// The bytes of a payload buffer a walk of nsym codewords from start_bit can reach: they end within
// nsym * max_len bits, so the rest of a longer buffer is never walked.
static uint64_t clamp_reach(const hz_ctx* c, uint64_t payload_bytes, uint64_t start_bit, uint64_t nsym) {
    const uint64_t reach = (start_bit + nsym * (uint64_t)std::max(c->t.dec_max_len, 1) + 7) / 8 + 8;
    return nsym <= (UINT64_MAX - start_bit) / 64 && payload_bytes > reach ? reach : payload_bytes;
}

// A base-taking call's largest stream position, base_bits + 8 * bytes, computed without a wrap: it must
// stay below HZ_POS_LIMIT (include/huffman_amd.h "Stream positions"), else the call is refused before
// anything is launched.
static bool far_pos_ok(uint64_t base_bits, uint64_t bytes) {
    return bytes <= (HZ_POS_LIMIT - 1) / 8 && base_bits <= HZ_POS_LIMIT - 1 - 8 * bytes;
}
static bool far_byte_pos_ok(uint64_t base_bytes, uint64_t bytes) {
    return base_bytes <= (HZ_POS_LIMIT - 1) / 8 && far_pos_ok(8 * base_bytes, bytes);
}

// hz_pack_seek's placement: the call packs symbols [sym_base, sym_base + n / 2) of a stream of stream_nsym
// and writes their entries of the table at d_seek (addressed from entry 0), each counted bit_base
// further than from byte 0 of d_out.
struct PackSeek {
    uint64_t sym_base, bit_base, stream_nsym;
    uint64_t* d_seek;
};

static int pack_impl(hz_ctx* c, const uint8_t* d_in, uint64_t n, uint64_t start_bit, uint32_t lead, uint8_t* d_out,
                     uint64_t out_cap, uint64_t* d_index, void* d_ranges, const PackSeek* sk = nullptr) {
    if (!c || !d_out) return HZ_EINVAL;
    if (((uintptr_t)d_out) & 3) return HZ_EINVAL;
    const uint64_t nsym = n / 2;
    if (nsym == 0) return HZ_OK;
    if (!d_in || (((uintptr_t)d_in) & 15)) return HZ_EINVAL;
    if (c->t.enc_mode < 0) return HZ_EINVAL;
    // d_out must hold ceil((start_bit + payload_bits) / 32) words; the kernel
    // drops (and flags HZ_ECAP) any block that would write past out_cap.
    if (out_cap < 4) return HZ_ECAP;
    HZ_TRY(hipSetDevice(c->device));
    int rc = ensure_scratch(c, pack_scratch_words(nsym));
    if (rc) return rc;
    if (sk) {
        // the writer waves store start[] of the call's blocks straight into its window of the table (the
        // stream's end after the last block), then the window moves by bit_base; no scratch beyond the pack's
        unsigned long long* win = reinterpret_cast<unsigned long long*>(sk->d_seek) + sk->sym_base / kBlockSyms;
        return timed_stage(c, HZ_STAGE_PACK, "launch_pack (seek)", [&] {
            hipError_t e = launch_pack(c->t, d_in, nsym, start_bit, lead, reinterpret_cast<uint32_t*>(d_out), out_cap / 4,
                                       c->d_desc, win, c->d_err, c->ncu, c->stream, d_ranges, &c->last_pack_ranges, true);
            if (e != hipSuccess) return e;
            if (c->t.enc_mode == ENC_FIXED16)  // symbol i at start_bit + 16 i
                return seek_fixed16(start_bit, nsym, UINT64_MAX, sk->sym_base, nsym, sk->stream_nsym, sk->bit_base,
                                    reinterpret_cast<unsigned long long*>(sk->d_seek), c->stream);
            return launch_seek_add(win, index_blocks(nsym) + 1, sk->bit_base, c->stream);
        });
    }
    return timed_stage(c, HZ_STAGE_PACK, "launch_pack", [&] {
        return launch_pack(c->t, d_in, nsym, start_bit, lead, reinterpret_cast<uint32_t*>(d_out), out_cap / 4,
                           c->d_desc, reinterpret_cast<unsigned long long*>(d_index), c->d_err, c->ncu, c->stream,
                           d_ranges, &c->last_pack_ranges);
    });
}

extern "C" int hz_pack(hz_ctx* c, const uint8_t* d_in, uint64_t n, uint64_t start_bit, uint32_t lead, uint8_t* d_out,
                       uint64_t out_cap, uint64_t* d_index) {
    return pack_impl(c, d_in, n, start_bit, lead, d_out, out_cap, d_index, nullptr);
}

extern "C" int hz_pack_ranges(hz_ctx* c, const uint8_t* d_in, uint64_t n, uint64_t start_bit, uint32_t lead,
                              uint8_t* d_out, uint64_t out_cap, uint64_t* d_index, void* d_ranges) {
    if (c) c->last_pack_ranges = 0;
    if (range_geom(n / 2).bytes && (!d_ranges || (((uintptr_t)d_ranges) & 15))) return HZ_EINVAL;
    return pack_impl(c, d_in, n, start_bit, lead, d_out, out_cap, d_index, range_geom(n / 2).bytes ? d_ranges : nullptr);
}

extern "C" int hz_pack_seek(hz_ctx* c, const uint8_t* d_in, uint64_t n, uint64_t start_bit, uint32_t lead, uint8_t* d_out,
                            uint64_t out_cap, void* d_ranges, uint64_t sym_base, uint64_t bit_base, uint64_t stream_nsym,
                            uint64_t* d_seek) {
    if (c) c->last_pack_ranges = 0;
    const uint64_t nsym = n / 2;
    if (!d_seek || (((uintptr_t)d_seek) & 7)) return HZ_EINVAL;
    if (sym_base % kBlockSyms || sym_base > stream_nsym || nsym > stream_nsym - sym_base) return HZ_EINVAL;
    // whole blocks, or the stream's last call: every entry of the window is a block start of this call
    if (nsym % kBlockSyms && sym_base + nsym != stream_nsym) return HZ_EINVAL;
    if (!far_pos_ok(bit_base, out_cap)) return HZ_EINVAL;  // no entry can wrap: a block ends within out_cap
    const bool plan = d_ranges && range_geom(nsym).bytes;
    if (plan && (((uintptr_t)d_ranges) & 15)) return HZ_EINVAL;
    const PackSeek sk{sym_base, bit_base, stream_nsym, d_seek};
    return pack_impl(c, d_in, n, start_bit, lead, d_out, out_cap, nullptr, plan ? d_ranges : nullptr, &sk);
}

extern "C" int hz_last_pack_ranges(hz_ctx* c) { return c ? c->last_pack_ranges : 0; }

extern "C" int hz_decode(hz_ctx* c, const uint8_t* d_payload, uint64_t payload_bytes, uint64_t nsym,
                         const uint64_t* d_index, uint8_t* d_out) {
    if (!c) return HZ_EINVAL;
    if (nsym == 0) return HZ_OK;
    if (!d_payload || !d_index || !d_out || (((uintptr_t)d_out) & 15)) return HZ_EINVAL;
    if (c->t.dec_mode < 0) return HZ_EINVAL;
    HZ_TRY(hipSetDevice(c->device));
    return timed_stage(c, HZ_STAGE_DECODE, "launch_decode", [&] {
        return launch_decode(c->t, d_payload, payload_bytes, nsym, reinterpret_cast<const unsigned long long*>(d_index),
                             d_out, c->d_err, c->ncu, c->stream, 0, &c->last_decode_chunks);
    });
}

extern "C" int hz_last_decode_chunks(hz_ctx* c) { return c ? c->last_decode_chunks : 0; }

extern "C" int hz_index_build(hz_ctx* c, const uint8_t* d_payload, uint64_t payload_bytes, uint64_t start_bit,
                              uint64_t nsym, uint64_t* d_index) {
    if (!c) return HZ_EINVAL;
    if (nsym == 0) return HZ_OK;
    if (!d_payload || !d_index) return HZ_EINVAL;
    if (c->t.dec_mode < 0) return HZ_EINVAL;
    HZ_TRY(hipSetDevice(c->device));
    payload_bytes = clamp_reach(c, payload_bytes, start_bit, nsym);
    int rc = ensure_scratch(c, index_scratch_words(payload_bytes, start_bit));
    if (rc) return rc;
    if ((rc = staging_flush(c, c->stage_walk))) return rc;  // the walk tables
    return timed_stage(c, HZ_STAGE_INDEX, "launch_index_build", [&] {
        return launch_index_build(c->t, d_payload, payload_bytes, start_bit, nsym,
                                  reinterpret_cast<unsigned long long*>(d_index), c->d_desc, c->d_err, c->h_err + 2,
                                  c->ncu, c->stream);
    });
}

// ---- random access: seek table and range decode ----------------------------
extern "C" uint64_t hz_seek_bytes(uint64_t nsym) { return nsym ? 8 * (index_blocks(nsym) + 1) : 0; }

// (hz_seek_span and hz_seek_pieces, host arithmetic on a host table: hz_seek_plan.cpp)

extern "C" int hz_decode_range(hz_ctx* c, const uint8_t* d_payload, uint64_t payload_bytes, uint64_t payload_byte_base,
                               const uint64_t* d_seek, uint64_t nsym, uint64_t sym_begin, uint64_t sym_count,
                               uint8_t* d_out, uint32_t flags) {
    if (!c || !d_payload || !d_seek || !d_out) return HZ_EINVAL;
    if ((flags & ~HZ_RANGE_FULL_INDEX) || (((uintptr_t)d_out) & 1)) return HZ_EINVAL;
    if (sym_begin > nsym || sym_count > nsym - sym_begin) return HZ_EINVAL;
    if (!far_byte_pos_ok(payload_byte_base, payload_bytes)) return HZ_EINVAL;
    if (sym_count == 0) return HZ_OK;
    if (c->t.dec_mode < 0) return HZ_EINVAL;
    HZ_TRY(hipSetDevice(c->device));
    int rc = ensure_scratch(c, range_scratch_words(sym_begin, sym_count));
    if (rc) return rc;
    return timed_stage(c, HZ_STAGE_DECODE, "launch_decode_range", [&] {
        return launch_decode_range(c->t, d_payload, payload_bytes, payload_byte_base,
                                   reinterpret_cast<const unsigned long long*>(d_seek), nsym, sym_begin, sym_count,
                                   d_out, (flags & HZ_RANGE_FULL_INDEX) != 0, c->d_desc, c->d_err, c->ncu, c->stream);
    });
}

extern "C" int hz_decode_ranges(hz_ctx* c, const uint8_t* d_payload, uint64_t payload_bytes, uint64_t payload_byte_base,
                                const uint64_t* d_seek, uint64_t nsym, const hz_range* d_ranges, uint32_t nranges,
                                uint8_t* d_out, uint64_t out_bytes, uint64_t* d_stats, uint32_t flags) {
    if (!c || !d_payload || !d_seek || !d_ranges || !d_out) return HZ_EINVAL;
    if ((flags & ~HZ_RANGE_FULL_INDEX) || (((uintptr_t)d_out) & 1)) return HZ_EINVAL;
    if (c->t.dec_mode < 0) return HZ_EINVAL;
    if (!far_byte_pos_ok(payload_byte_base, payload_bytes)) return HZ_EINVAL;
    if (nranges == 0) return HZ_OK;
    HZ_TRY(hipSetDevice(c->device));
    int rc = ensure_scratch(c, ranges_scratch_words(nranges));
    if (rc) return rc;
    return timed_stage(c, HZ_STAGE_DECODE, "launch_decode_ranges", [&] {
        return launch_decode_ranges(c->t, d_payload, payload_bytes, payload_byte_base,
                                    reinterpret_cast<const unsigned long long*>(d_seek), nsym, d_ranges, nranges, d_out,
                                    out_bytes, reinterpret_cast<unsigned long long*>(d_stats),
                                    (flags & HZ_RANGE_FULL_INDEX) != 0, c->d_desc, c->d_err, c->ncu, c->stream);
    });
}

extern "C" int hz_decode_ranges_pieces(hz_ctx* c, const uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* d_seek,
                                       uint64_t seek_words, const hz_piece* d_pieces, uint32_t npieces, uint64_t nsym,
                                       const hz_piece_range* d_ranges, uint32_t nranges, uint8_t* d_out,
                                       uint64_t out_bytes, uint64_t* d_stats, uint32_t flags) {
    if (!c || !d_buf || !d_seek || !d_pieces || !d_ranges || !d_out) return HZ_EINVAL;
    if (flags || (((uintptr_t)d_out) & 1)) return HZ_EINVAL;
    // a piece's first word is the one that holds its first byte: with d_buf off the 4-byte grid that
    // word would begin below the buffer
    if (((uintptr_t)d_buf) & 3) return HZ_EINVAL;
    if (c->t.dec_mode < 0) return HZ_EINVAL;
    if (!far_byte_pos_ok(0, buf_bytes)) return HZ_EINVAL;
    if (nranges == 0) return HZ_OK;
    HZ_TRY(hipSetDevice(c->device));
    int rc = ensure_scratch(c, ranges_scratch_words(nranges));
    if (rc) return rc;
    return timed_stage(c, HZ_STAGE_DECODE, "launch_decode_ranges_pieces", [&] {
        return launch_decode_ranges_pieces(c->t, d_buf, buf_bytes, reinterpret_cast<const unsigned long long*>(d_seek),
                                           seek_words, d_pieces, npieces, nsym, d_ranges, nranges, d_out, out_bytes,
                                           reinterpret_cast<unsigned long long*>(d_stats), c->d_desc, c->d_err, c->ncu,
                                           c->stream);
    });
}

extern "C" int hz_index_expand(hz_ctx* c, const uint8_t* d_payload, uint64_t payload_bytes, const uint64_t* d_seek,
                               uint64_t nsym, uint64_t* d_index) {
    if (!c) return HZ_EINVAL;
    if (nsym == 0) return HZ_OK;
    if (!d_payload || !d_seek || !d_index) return HZ_EINVAL;
    if (c->t.dec_mode < 0) return HZ_EINVAL;
    HZ_TRY(hipSetDevice(c->device));
    return timed_stage(c, HZ_STAGE_INDEX, "launch_index_expand", [&] {
        return launch_index_expand(c->t, d_payload, payload_bytes, reinterpret_cast<const unsigned long long*>(d_seek),
                                   nsym, reinterpret_cast<unsigned long long*>(d_index), c->d_err, c->stream);
    });
}

// Where a call's codewords lie in a longer stream and the table that takes their seek entries
// (hz_decode_indexless_seek); null: no table (hz_decode_indexless).
struct SeekReq {
    uint64_t sym_base, bit_base, stream_nsym;
    unsigned long long* d_seek;
};

// hz_decode_indexless, and with sk its seek entries too; d_out null (with sk only): nothing decoded, the
// end bit from the seek pass.
static int decode_indexless_impl(hz_ctx* c, const uint8_t* d_payload, uint64_t payload_bytes, uint64_t start_bit,
                                 uint64_t nsym, uint8_t* d_out, uint64_t* d_end_bit, const SeekReq* sk) {
    HZ_TRY(hipSetDevice(c->device));
    payload_bytes = clamp_reach(c, payload_bytes, start_bit, nsym);
    unsigned long long* d_end = reinterpret_cast<unsigned long long*>(d_end_bit);
    if (c->t.dec_mode == DEC_FIXED16) {
        // every code 16 bits: symbol i at start_bit + 16 i, so no index and no walk (stream-ordered)
        const uint64_t endb = nsym <= (UINT64_MAX - start_bit) / 16 ? start_bit + 16 * nsym : ~0ull;
        const bool fits = endb <= payload_bytes * 8;  // else: the end bit past the payload, nothing decoded
        return timed_stage(c, HZ_STAGE_EXTRACT, "put_u64 / launch_decode (FIXED16)", [&] {
            hipError_t e = d_end_bit ? put_u64(d_end_bit, fits ? endb : ~0ull, c->stream) : hipSuccess;
            if (e == hipSuccess && fits && d_out)
                e = launch_decode(c->t, d_payload, payload_bytes, nsym, nullptr, d_out, c->d_err, c->ncu, c->stream,
                                  start_bit);
            if (e == hipSuccess && sk)
                e = seek_fixed16(start_bit, nsym, payload_bytes * 8, sk->sym_base, nsym, sk->stream_nsym, sk->bit_base,
                                 sk->d_seek, c->stream);
            return e;
        });
    }
    if (!seg_decode_supported(c->t)) return HZ_EINVAL;  // (every codebook but FIXED16 has chain tables)
    int rc = staging_flush(c, c->stage_walk);  // the chain tables
    if (rc) return rc;
    if (payload_bytes < 16)  // too short for the walk: one thread, serially (stream-ordered too)
        return timed_stage(c, HZ_STAGE_EXTRACT, "chain_decode_tiny", [&] {
            hipError_t e = hipSuccess;
            if (d_out)
                e = chain_decode_tiny(c->t, d_payload, payload_bytes, start_bit, nsym, d_out, d_end, c->d_err, c->stream);
            if (e == hipSuccess && sk)
                e = chain_seek_tiny(c->t, d_payload, payload_bytes, start_bit, nsym, sk->sym_base, sk->bit_base,
                                    sk->stream_nsym, sk->d_seek, d_out ? nullptr : d_end, c->d_err, c->stream);
            return e;
        });
    // stream-ordered from here: walk, fix-ups, scans, block decode, tails (no host synchronisation
    // unless the context's scratch has to grow)
    const uint64_t pbits = payload_bytes * 8 > start_bit ? payload_bytes * 8 - start_bit : 0;
    if ((rc = ensure_scratch(c, chain_scratch_words(0, pbits, nsym, c->t, c->ncu)))) return rc;
    return timed_stage(c, HZ_STAGE_EXTRACT, "chain_scan / chain_decode", [&] {
        hipError_t e = chain_scan(c->chain, c->t, d_payload, payload_bytes, 0, start_bit, nsym, 0, pbits, ~0ull,
                                  c->d_desc, c->d_err, c->ncu, c->stream);
        if (e == hipSuccess && d_out) e = chain_decode(c->chain, c->t, nsym, d_out, d_end, c->ncu, c->stream);
        if (e == hipSuccess && sk)  // table only: the seek pass finds the end bit, no decode and no tail
            e = chain_seek(c->chain, c->t, sk->sym_base, nsym, sk->stream_nsym, sk->bit_base, sk->d_seek,
                           d_out ? nullptr : d_end, c->ncu, c->stream);
        if (e == hipSuccess) chain_invalidate(c->chain);  // not a part: hz_indexless_refix / _decode may not continue it
        return e;
    });
}

extern "C" int hz_decode_indexless(hz_ctx* c, const uint8_t* d_payload, uint64_t payload_bytes, uint64_t start_bit,
                                   uint64_t nsym, uint8_t* d_out, uint64_t* d_end_bit) {
    if (!c) return HZ_EINVAL;
    if (nsym == 0) return HZ_OK;
    if (!d_payload || !d_out || (((uintptr_t)d_out) & 15)) return HZ_EINVAL;
    if (c->t.dec_mode < 0) return HZ_EINVAL;
    return decode_indexless_impl(c, d_payload, payload_bytes, start_bit, nsym, d_out, d_end_bit, nullptr);
}

extern "C" int hz_decode_indexless_seek(hz_ctx* c, const uint8_t* d_payload, uint64_t payload_bytes, uint64_t start_bit,
                                        uint64_t nsym, uint8_t* d_out, uint64_t* d_end_bit, uint64_t sym_base,
                                        uint64_t bit_base, uint64_t stream_nsym, uint64_t* d_seek) {
    if (!c || !d_seek || (((uintptr_t)d_out) & 15)) return HZ_EINVAL;
    if (sym_base > stream_nsym || nsym > stream_nsym - sym_base) return HZ_EINVAL;
    if (!far_pos_ok(bit_base, payload_bytes)) return HZ_EINVAL;  // no entry can wrap: a held codeword starts in the payload
    if (c->t.dec_mode < 0) return HZ_EINVAL;
    if (nsym == 0) return HZ_OK;
    if (!d_payload) return HZ_EINVAL;
    const SeekReq sk{sym_base, bit_base, stream_nsym, reinterpret_cast<unsigned long long*>(d_seek)};
    return decode_indexless_impl(c, d_payload, payload_bytes, start_bit, nsym, d_out, d_end_bit, &sk);
}

extern "C" int hz_seek_build(hz_ctx* c, const uint8_t* d_payload, uint64_t payload_bytes, uint64_t start_bit,
                             uint64_t nsym, uint64_t* d_seek) {
    return hz_decode_indexless_seek(c, d_payload, payload_bytes, start_bit, nsym, nullptr, nullptr, 0, 0, nsym, d_seek);
}

// ---- one stream over several devices: the index-less decode in parts -----------------
// (a scanned or refixed part's summary, where asked for, and the error check behind the phase)
static int part_summary(hz_ctx* c, uint64_t* d_summary) {
    if (d_summary && !chain_info(c->chain)) return HZ_EINVAL;
    if (d_summary) HZ_TRY(chain_summary(c->chain, reinterpret_cast<unsigned long long*>(d_summary), c->stream));
    return arm_err_check(c);
}

// FIXED16 parts: codeword i starts at start + 16 i, so a part's entry, exit and count are arithmetic.
static int fixed_part_summary(hz_ctx* c, uint64_t* d_summary) {
    if (!d_summary) return HZ_OK;
    HZ_TRY(put3(reinterpret_cast<unsigned long long*>(d_summary), (c->fx.xit - c->fx.entry) / 16, c->fx.xit,
                c->fx.entry, c->stream));
    return HZ_OK;
}

extern "C" int hz_indexless_scan(hz_ctx* c, const uint8_t* d_payload, uint64_t payload_bytes, uint64_t payload_bit_base,
                                 uint64_t start_bit, uint64_t nsym, uint64_t part_begin, uint64_t part_end,
                                 uint64_t entry_bit, uint64_t* d_summary) {
    // (under 16 bytes the walk's 16-byte loads have no whole chunk to clamp to: such a view is refused)
    if (!c || !d_payload || part_end <= part_begin || payload_bytes < 16) return HZ_EINVAL;
    if (c->t.dec_mode < 0) return HZ_EINVAL;
    if (payload_bit_base % 8) return HZ_EINVAL;  // the view begins on a byte of the stream
    if (start_bit > UINT64_MAX - part_end || !far_pos_ok(payload_bit_base, payload_bytes)) return HZ_EINVAL;
    // the view must hold the part, and the lead-in before it (the stream's bits from its start, when the
    // part begins less than HZ_INDEXLESS_LEAD_BITS into it)
    const uint64_t lead = part_begin < HZ_INDEXLESS_LEAD_BITS ? part_begin : HZ_INDEXLESS_LEAD_BITS;
    if (start_bit + part_begin - lead < payload_bit_base) return HZ_EINVAL;
    if (start_bit + part_end > payload_bit_base + payload_bytes * 8) return HZ_EINVAL;
    // an explicit entry is a codeword start of this part: not before the part's first bit (a walk from
    // there would count the previous part's codewords) and not below the view (FIXED16 decodes from
    // entry - base)
    const uint64_t floor = std::max(payload_bit_base, start_bit + part_begin);
    if (entry_bit != UINT64_MAX && entry_bit < floor) return HZ_EINVAL;
    HZ_TRY(hipSetDevice(c->device));
    chain_invalidate(c->chain);
    c->fx.on = false;
    c->part_floor = floor;
    if (c->t.dec_mode == DEC_FIXED16) {
        c->fx.payload = d_payload;
        c->fx.bytes = payload_bytes;
        c->fx.base = payload_bit_base;
        c->fx.start = start_bit;
        c->fx.entry = entry_bit != UINT64_MAX ? entry_bit : start_bit + 16 * ((part_begin + 15) / 16);
        c->fx.xit = start_bit + 16 * ((part_end + 15) / 16);
        if (c->fx.entry < start_bit || (c->fx.entry - start_bit) % 16 || c->fx.entry > c->fx.xit) return HZ_EINVAL;
        c->fx.on = true;
        return fixed_part_summary(c, d_summary);
    }
    if (!seg_decode_supported(c->t)) return HZ_EINVAL;
    // record capacity from the stream's own bits per codeword when the caller knows its symbols
    const uint64_t pbits = payload_bit_base + payload_bytes * 8 > start_bit ? payload_bit_base + payload_bytes * 8 - start_bit : 0;
    const uint64_t hint = nsym ? std::max<uint64_t>(1, (uint64_t)((double)nsym * (double)(part_end - part_begin) /
                                                                  (double)std::max<uint64_t>(pbits, 1))) : 0;
    int rc = ensure_scratch(c, chain_scratch_words(part_begin, part_end, hint, c->t, c->ncu));
    if (rc) return rc;
    if ((rc = staging_flush(c, c->stage_walk))) return rc;  // the chain tables
    HZ_TRY(chain_scan(c->chain, c->t, d_payload, payload_bytes, payload_bit_base, start_bit, hint, part_begin, part_end,
                      entry_bit, c->d_desc, c->d_err, c->ncu, c->stream));
    return part_summary(c, d_summary);
}

extern "C" int hz_indexless_refix(hz_ctx* c, uint64_t entry_bit, uint64_t* d_summary) {
    if (c && c->fx.on) {
        if (entry_bit < c->part_floor) return HZ_EINVAL;
        if (entry_bit < c->fx.start || (entry_bit - c->fx.start) % 16 || entry_bit > c->fx.xit) return HZ_EINVAL;
        HZ_TRY(hipSetDevice(c->device));
        c->fx.entry = entry_bit;
        return fixed_part_summary(c, d_summary);
    }
    if (!c || !chain_info(c->chain)) return HZ_EINVAL;
    if (entry_bit != UINT64_MAX && entry_bit < c->part_floor) return HZ_EINVAL;  // (UINT64_MAX: the walked entry again)
    HZ_TRY(hipSetDevice(c->device));
    HZ_TRY(chain_refix(c->chain, c->t, entry_bit, c->ncu, c->stream));
    return part_summary(c, d_summary);
}

extern "C" int hz_indexless_decode(hz_ctx* c, uint64_t nsym, uint8_t* d_out, uint64_t* d_end_bit) {
    if (c && c->fx.on) {
        if (nsym && (!d_out || (((uintptr_t)d_out) & 15))) return HZ_EINVAL;
        HZ_TRY(hipSetDevice(c->device));
        const uint64_t count = (c->fx.xit - c->fx.entry) / 16;
        const uint64_t take = nsym < count ? nsym : count;
        if (take)
            HZ_TRY(launch_decode(c->t, c->fx.payload, c->fx.bytes, take, nullptr, d_out, c->d_err, c->ncu, c->stream,
                                 c->fx.entry - c->fx.base));
        if (d_end_bit)
            HZ_TRY(put_u64(d_end_bit, nsym && nsym <= count ? c->fx.entry + 16 * nsym : UINT64_MAX, c->stream));
        return arm_err_check(c);
    }
    if (!c || !chain_info(c->chain)) return HZ_EINVAL;
    if (nsym && (!d_out || (((uintptr_t)d_out) & 15))) return HZ_EINVAL;
    HZ_TRY(hipSetDevice(c->device));
    HZ_TRY(chain_decode(c->chain, c->t, nsym, d_out, reinterpret_cast<unsigned long long*>(d_end_bit), c->ncu,
                        c->stream));
    return arm_err_check(c);
}

extern "C" int hz_indexless_seek(hz_ctx* c, uint64_t sym_base, uint64_t nsym, uint64_t stream_nsym, uint64_t* d_seek) {
    if (!c || !d_seek) return HZ_EINVAL;
    if (sym_base > stream_nsym || nsym > stream_nsym - sym_base) return HZ_EINVAL;
    unsigned long long* sk = reinterpret_cast<unsigned long long*>(d_seek);
    if (!c->fx.on && !chain_info(c->chain)) return HZ_EINVAL;  // no pending part
    if (nsym == 0) return HZ_OK;  // no codewords of the part: no entry is this call's
    if (c->fx.on) {  // stream bits throughout: the part's codeword S at entry + 16 S
        HZ_TRY(hipSetDevice(c->device));
        HZ_TRY(seek_fixed16(c->fx.entry, (c->fx.xit - c->fx.entry) / 16, c->fx.base + 8 * c->fx.bytes, sym_base, nsym,
                            stream_nsym, 0, sk, c->stream));
        return arm_err_check(c);
    }
    if (!chain_info(c->chain)) return HZ_EINVAL;
    HZ_TRY(hipSetDevice(c->device));
    HZ_TRY(chain_seek(c->chain, c->t, sym_base, nsym, stream_nsym, 0, sk, nullptr, c->ncu, c->stream));
    return arm_err_check(c);
}

// Debug (not in the public header; tests/test_gpu_seek_build.py pins the rare paths with it): how many
// entries the context's last k_chain_seek found in a head, past the record capacity, through the
// delta rebuild and in a chain that has a head (4 x u64). Synchronises the stream. HZ_EINVAL: no such pass since the scratch last grew.
extern "C" int hz_debug_seek_stats(hz_ctx* c, uint64_t* out) {
    if (!c || !out || !chain_seek_stats(c->chain)) return HZ_EINVAL;
    HZ_TRY(hipSetDevice(c->device));
    HZ_TRY(hipStreamSynchronize(c->stream));
    HZ_TRY(hipMemcpy(out, chain_seek_stats(c->chain), 32, hipMemcpyDeviceToHost));
    return HZ_OK;
}

// Zipf thresholds: thr[r-1] = floor(2^64 * sum_{j<=r} j^-alpha / H); thr[255] = max.
static void zipf_thresholds(double alpha, unsigned long long* thr) {
    double H = 0.0;
    for (int r = 1; r <= 256; ++r) H += pow((double)r, -alpha);
    double cum = 0.0;
    for (int r = 1; r <= 256; ++r) {
        cum += pow((double)r, -alpha);
        const double x = cum / H;
        thr[r - 1] = (r == 256 || x >= 1.0) ? ~0ull : (unsigned long long)ldexp(x, 64);
    }
}

extern "C" int hz_generate(hz_ctx* c, uint8_t* d_out, uint64_t n, uint64_t offset, int kind, double alpha,
                           uint64_t seed) {
    if (!c || (n && !d_out) || kind < 0 || kind > 1) return HZ_EINVAL;
    HZ_TRY(hipSetDevice(c->device));
    if (!c->d_thr) HZ_TRY(hipMalloc(&c->d_thr, 256 * sizeof(unsigned long long)));
    if (kind == 1 && c->thr_alpha != alpha) {
        static unsigned long long thr[256];
        zipf_thresholds(alpha, thr);
        HZ_TRY(hipMemcpy(c->d_thr, thr, sizeof(thr), hipMemcpyHostToDevice));
        c->thr_alpha = alpha;
    }
    HZ_TRY(launch_generate(d_out, n, offset, kind, seed, c->d_thr, c->stream));
    return HZ_OK;
}

int hz::default_ctx(hz_ctx** out) {
    static std::mutex mu;
    static hz_ctx* ctx = nullptr;
    std::lock_guard<std::mutex> lk(mu);
    if (!ctx) {
        int rc = hz_ctx_create(0, nullptr, &ctx);
        if (rc) return rc;
    }
    *out = ctx;
    return HZ_OK;
}
