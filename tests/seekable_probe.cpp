// seekable_probe.cpp -- a stand-alone host program over hz_seekable.cpp and hz_file_io.cpp (no HIP call,
// no device), built by tests/test_seekable_probe.py with the address and undefined-behaviour sanitizers
// and run as a plain child process. It writes trailers to files and parses them back, feeds the parser
// footers whose check is right and whose fields lie, and asks for a missing path. One line per case;
// the test knows what each must say.
//   seekable_probe <directory>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "huffman_amd.h"
#include "hz_seekable.h"

namespace {

void put64(uint8_t* p, uint64_t v) { memcpy(p, &v, 8); }
void put32(uint8_t* p, uint32_t v) { memcpy(p, &v, 4); }

bool write_file(const std::string& path, const std::vector<uint8_t>& bytes) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = bytes.empty() || fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    return fclose(f) == 0 && ok;
}

// An image of image_bytes (a byte pattern) with the trailer of an n-byte original behind it, written to
// path; then the file's info and its table and sums loaded back and compared.
int roundtrip(const std::string& path, uint64_t image_bytes, uint64_t n, uint32_t flags) {
    const uint64_t nsym = n / 2, nblocks = hz::seekable_blocks(nsym), words = hz::seekable_seek_bytes(nsym) / 8;
    std::vector<uint64_t> seek(words);
    std::vector<uint32_t> sums(flags & HZ_SEEKABLE_SUMS ? nblocks : 0);
    for (uint64_t i = 0; i < words; ++i) seek[i] = 1000 * i + 7;
    for (uint64_t i = 0; i < sums.size(); ++i) sums[i] = (uint32_t)(0x9E3779B9u * (i + 1));
    std::vector<uint8_t> file(image_bytes);
    for (uint64_t i = 0; i < image_bytes; ++i) file[i] = (uint8_t)(i * 37 + 1);
    const uint64_t len = hz_seekable_trailer_bytes(image_bytes, n, flags);
    file.resize(image_bytes + len);  // exactly: a write past len is the sanitizer's to report
    uint64_t got = 0;
    int rc = hz_seekable_trailer_write(image_bytes, n, seek.data(), sums.data(), flags, file.data() + image_bytes, len, &got);
    if (rc || got != len || !write_file(path, file)) return 100;
    hz_seekable_info si;
    if ((rc = hz_seekable_info_file(path.c_str(), &si))) return rc;
    if (!si.present || si.n != n || si.nsym != nsym || si.nblocks != nblocks || si.image_bytes != image_bytes ||
        si.file_bytes != file.size() || si.flags != flags || si.seek_off % 8 || si.seek_off < image_bytes)
        return 101;
    std::vector<uint64_t> seek2(words);  // exactly the capacity the file needs
    std::vector<uint32_t> sums2(sums.size());
    uint64_t nsym2 = 0;
    rc = hz_seekable_load_file(path.c_str(), seek2.data(), 8 * words, sums.empty() ? nullptr : sums2.data(), 4 * sums2.size(), &nsym2);
    if (rc) return rc;
    if (nsym2 != nsym || seek2 != seek || sums2 != sums) return 102;
    if (words && hz_seekable_load_file(path.c_str(), seek2.data(), 8 * words - 1, nullptr, 0, &nsym2) != HZ_ECAP) return 103;
    return 0;
}

// A footer with a right check over lying fields, parsed as the end of a file of file_bytes.
int lying(uint64_t file_bytes, uint64_t n, uint64_t image_bytes, uint64_t seek_off, uint64_t sums_off, uint32_t flags) {
    uint8_t f[HZ_SEEKABLE_FOOTER_BYTES] = {0};
    memcpy(f, "HZSKTRL1", 8);
    put32(f + 8, 1);
    put32(f + 12, flags);
    put64(f + 16, n);
    put64(f + 24, image_bytes);
    put64(f + 32, seek_off);
    put64(f + 40, sums_off);
    put32(f + 48, 2048);
    put32(f + 60, hz::adler32(1, f, 60));
    hz_seekable_info si;
    const int rc = hz_seekable_footer_parse(f, file_bytes, &si);
    return rc ? rc : (int)si.present;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const std::string dir = argv[1];
    // files shorter than a footer, and of exactly its size: plain, whatever they hold
    for (uint64_t size : {0ull, 1ull, 63ull}) {
        const std::string p = dir + "/short" + std::to_string(size);
        hz_seekable_info si;
        if (!write_file(p, std::vector<uint8_t>(size, 0x48))) return 3;
        const int rc = hz_seekable_info_file(p.c_str(), &si);
        uint64_t nsym = 77;
        printf("short %llu %d %u %d\n", (unsigned long long)size, rc, si.present,
               hz_seekable_load_file(p.c_str(), nullptr, 0, nullptr, 0, &nsym));
    }
    // exactly 64 bytes: the trailer of an empty image of an empty original is the footer alone
    printf("footer-only %d %llu\n", roundtrip(dir + "/only", 0, 0, 0),
           (unsigned long long)hz_seekable_trailer_bytes(0, 0, HZ_SEEKABLE_SUMS));
    {
        const std::string p = dir + "/junk64";
        hz_seekable_info si;
        if (!write_file(p, std::vector<uint8_t>(64, 0x5A))) return 3;
        const int rc = hz_seekable_info_file(p.c_str(), &si);
        printf("junk64 %d %u\n", rc, si.present);
    }
    const uint64_t sizes[] = {0, 1, 2, 3, 4095, 4096, 4097, 4098, 8193, 1 << 20};
    for (uint64_t n : sizes)
        for (uint32_t flags = 0; flags < 2; ++flags)
            for (uint64_t image = 11; image < 19; ++image)
                if (int rc = roundtrip(dir + "/rt", image, n, flags)) {
                    printf("roundtrip %llu %u %llu %d\n", (unsigned long long)n, flags, (unsigned long long)image, rc);
                    return 1;
                }
    printf("roundtrip ok\n");
    // offsets that point past the file, and sizes whose table would not fit 64 bits
    const uint64_t M = UINT64_MAX;
    printf("lying %d %d %d %d %d %d %d %d\n",
           lying(1 << 20, 8192, 1000, 1000, 0, 0),               // the honest one needs 1000 + 24 + 64 bytes
           lying(1 << 20, 8192, 1000, 1 << 21, 0, 0),            // the table past the file
           lying(1 << 20, 8192, 1000, 1000, 1 << 22, 1),         // the sums past the file
           lying(1 << 20, M, 1000, 1000, 0, 0),                  // 8 * (nblocks + 1) of a huge n
           lying(1 << 20, M - 1, M - 70, M - 63, 0, 1),          // every sum wraps
           lying(M, M, M - 64, M - 64, 0, 0),
           lying(64, 0, M, 0, 0, 0),
           lying(1000 + 24 + 64, 8192, 1000, 1000, 0, 0));       // and the honest footer, accepted
    hz_seekable_info si;
    uint64_t nsym = 0;
    printf("missing %d %d\n", hz_seekable_info_file((dir + "/no-such-file").c_str(), &si),
           hz_seekable_load_file((dir + "/no-such-file").c_str(), nullptr, 0, nullptr, 0, &nsym));
    printf("null %d %d %d\n", hz_seekable_info_file(nullptr, &si), hz_seekable_footer_parse(nullptr, 100, nullptr),
           hz_seekable_trailer_write(0, 0, nullptr, nullptr, 0, nullptr, 0, nullptr));
    return 0;
}
