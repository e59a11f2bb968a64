// hz_seekable.cpp -- the trailer of a seekable file (include/huffman_amd.h "seekable files"): its layout,
// its writer, the footer's parse and the by-path loads of the table and the sums. Host arithmetic and
// positional file reads only, no HIP call: the unit links with hz_file_io.cpp alone, so a stand-alone
// host program runs it under the address and undefined-behaviour sanitizers (tests/seekable_probe.cpp).
// The flows that put a trailer behind an image or read ranges through one are hz_image.cpp and
// hz_stream.cpp. Words are stored as the host holds them: little-endian, like every gfx950 host.
#include "hz_seekable.h"

#include <string.h>

#include "hz_file_io.h"

namespace hz {

uint32_t adler32(uint32_t adler, const uint8_t* p, uint64_t n) {
    uint32_t a = adler & 0xffffu, b = adler >> 16;
    while (n) {
        const uint64_t run = n < 5552 ? n : 5552;  // the most bytes whose sums fit 32 bits unreduced (zlib's NMAX)
        for (uint64_t i = 0; i < run; ++i) {
            a += p[i];
            b += a;
        }
        a %= 65521u;
        b %= 65521u;
        p += run;
        n -= run;
    }
    return b << 16 | a;
}

namespace {

const uint8_t kMagic[8] = {'H', 'Z', 'S', 'K', 'T', 'R', 'L', '1'};
constexpr uint32_t kVersion = 1;

bool add(uint64_t a, uint64_t b, uint64_t* r) { return !__builtin_add_overflow(a, b, r); }
bool round8(uint64_t a, uint64_t* r) {
    if (!add(a, 7, r)) return false;
    *r &= ~7ull;
    return true;
}

void put32(uint8_t* p, uint32_t v) { memcpy(p, &v, 4); }
void put64(uint8_t* p, uint64_t v) { memcpy(p, &v, 8); }
uint32_t get32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
uint64_t get64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }

}  // namespace

SeekableLayout seekable_layout(uint64_t image_bytes, uint64_t n, uint32_t flags) {
    SeekableLayout l;
    const uint64_t nsym = n / 2;
    l.seek_bytes = seekable_seek_bytes(nsym);  // nblocks < 2^53: neither product wraps
    l.sums_bytes = flags & HZ_SEEKABLE_SUMS ? 4 * seekable_blocks(nsym) : 0;
    uint64_t sums_at, end;
    if (!round8(image_bytes, &l.seek_off) || !add(l.seek_off, l.seek_bytes, &sums_at) ||
        !add(sums_at, l.sums_bytes, &end) || !round8(end, &end) || !add(end, HZ_SEEKABLE_FOOTER_BYTES, &l.file_bytes))
        return l;
    l.sums_off = flags & HZ_SEEKABLE_SUMS ? sums_at : 0;
    l.ok = true;
    return l;
}

int seekable_footer(uint64_t image_bytes, uint64_t n, uint32_t flags, uint8_t* f) {
    const SeekableLayout l = seekable_layout(image_bytes, n, flags);
    if (!l.ok || (flags & ~HZ_SEEKABLE_SUMS)) return HZ_EINVAL;
    memset(f, 0, HZ_SEEKABLE_FOOTER_BYTES);
    memcpy(f, kMagic, 8);
    put32(f + 8, kVersion);
    put32(f + 12, flags);
    put64(f + 16, n);
    put64(f + 24, image_bytes);
    put64(f + 32, l.seek_off);
    put64(f + 40, l.sums_off);
    put32(f + 48, (uint32_t)kSeekableBlockSyms);
    put32(f + 60, adler32(1, f, 60));
    return HZ_OK;
}

int image_end(const uint8_t* file, uint64_t len, uint64_t* image_bytes, hz_seekable_info* info) {
    hz_seekable_info mine;
    hz_seekable_info* si = info ? info : &mine;
    const int rc = hz_seekable_footer_parse(len >= HZ_SEEKABLE_FOOTER_BYTES ? file + len - HZ_SEEKABLE_FOOTER_BYTES : nullptr,
                                            len, si);
    if (rc) return rc;
    *image_bytes = si->present ? si->image_bytes : len;
    return HZ_OK;
}

int image_end_fd(int fd, uint64_t file_bytes, uint64_t* image_bytes, hz_seekable_info* info) {
    uint8_t last[HZ_SEEKABLE_FOOTER_BYTES];
    hz_seekable_info mine;
    hz_seekable_info* si = info ? info : &mine;
    const bool has = file_bytes >= HZ_SEEKABLE_FOOTER_BYTES;
    if (has)
        if (int rc = pread_all(fd, last, HZ_SEEKABLE_FOOTER_BYTES, file_bytes - HZ_SEEKABLE_FOOTER_BYTES)) return rc;
    const int rc = hz_seekable_footer_parse(has ? last : nullptr, file_bytes, si);
    if (rc) return rc;
    *image_bytes = si->present ? si->image_bytes : file_bytes;
    return HZ_OK;
}

}  // namespace hz

using namespace hz;

extern "C" uint64_t hz_seekable_trailer_bytes(uint64_t image_bytes, uint64_t n, uint32_t flags) {
    const SeekableLayout l = seekable_layout(image_bytes, n, flags);
    return l.ok ? l.file_bytes - image_bytes : 0;
}

extern "C" int hz_seekable_trailer_write(uint64_t image_bytes, uint64_t n, const uint64_t* seek, const uint32_t* sums,
                                         uint32_t flags, uint8_t* out, uint64_t cap, uint64_t* len) {
    if (!len || (flags & ~HZ_SEEKABLE_SUMS)) return HZ_EINVAL;
    const SeekableLayout l = seekable_layout(image_bytes, n, flags);
    if (!l.ok) return HZ_EINVAL;
    *len = l.file_bytes - image_bytes;
    if (cap < *len || !out) return HZ_ECAP;
    if ((l.seek_bytes && !seek) || (l.sums_bytes && !sums)) return HZ_EINVAL;
    memset(out, 0, *len);
    uint8_t* p = out + (l.seek_off - image_bytes);
    if (l.seek_bytes) memcpy(p, seek, l.seek_bytes);
    if (l.sums_bytes) memcpy(p + l.seek_bytes, sums, l.sums_bytes);
    return seekable_footer(image_bytes, n, flags, out + *len - HZ_SEEKABLE_FOOTER_BYTES);
}

extern "C" int hz_seekable_footer_parse(const uint8_t* last64, uint64_t file_bytes, hz_seekable_info* info) {
    if (!info) return HZ_EINVAL;
    memset(info, 0, sizeof(*info));
    info->file_bytes = file_bytes;
    if (!last64 || file_bytes < HZ_SEEKABLE_FOOTER_BYTES) return HZ_OK;  // a plain file
    if (memcmp(last64, kMagic, 8) != 0 || get32(last64 + 60) != adler32(1, last64, 60)) return HZ_OK;
    // a trailer: from here a field that does not fit is an error, not a plain file
    const uint32_t version = get32(last64 + 8), flags = get32(last64 + 12);
    const uint64_t n = get64(last64 + 16), image_bytes = get64(last64 + 24);
    if (version != kVersion || (flags & ~HZ_SEEKABLE_SUMS)) return HZ_EFORMAT;
    if (get32(last64 + 48) != kSeekableBlockSyms || get32(last64 + 52) || get32(last64 + 56)) return HZ_EFORMAT;
    const SeekableLayout l = seekable_layout(image_bytes, n, flags);  // the one layout these fields allow
    if (!l.ok || get64(last64 + 32) != l.seek_off || get64(last64 + 40) != l.sums_off || file_bytes != l.file_bytes)
        return HZ_EFORMAT;
    info->present = 1;
    info->version = version;
    info->flags = flags;
    info->n = n;
    info->nsym = n / 2;
    info->nblocks = seekable_blocks(n / 2);
    info->image_bytes = image_bytes;
    info->seek_off = l.seek_off;
    info->sums_off = l.sums_off;
    return HZ_OK;
}

extern "C" int hz_seekable_info_file(const char* path, hz_seekable_info* info) {
    if (!path || !info) return HZ_EINVAL;
    FileReader f(nullptr);
    if (int rc = f.open(path)) return rc;
    uint64_t image_bytes;
    return image_end_fd(f.fd(), f.size(), &image_bytes, info);
}

extern "C" int hz_seekable_load_file(const char* path, uint64_t* seek, uint64_t seek_cap_bytes, uint32_t* sums,
                                     uint64_t sums_cap_bytes, uint64_t* nsym) {
    if (!path || !nsym) return HZ_EINVAL;
    FileReader f(nullptr);
    if (int rc = f.open(path)) return rc;
    hz_seekable_info si;
    uint64_t image_bytes;
    if (int rc = image_end_fd(f.fd(), f.size(), &image_bytes, &si)) return rc;
    if (!si.present) return HZ_EFORMAT;
    *nsym = si.nsym;
    if (sums && !(si.flags & HZ_SEEKABLE_SUMS)) return HZ_EINVAL;
    const uint64_t seek_bytes = seekable_seek_bytes(si.nsym), sums_bytes = 4 * si.nblocks;
    if (seek_cap_bytes < seek_bytes || (seek_bytes && !seek) || (sums && sums_cap_bytes < sums_bytes)) return HZ_ECAP;
    if (seek_bytes)
        if (int rc = pread_all(f.fd(), (uint8_t*)seek, seek_bytes, si.seek_off)) return rc;
    if (sums && sums_bytes)
        if (int rc = pread_all(f.fd(), (uint8_t*)sums, sums_bytes, si.sums_off)) return rc;
    return HZ_OK;
}
