// pieces_probe.cpp -- hz_seek_pieces over lists of ranges read from a file, its plans printed as text for
// tests/test_seek_pieces_host.py to compare with what the library returns through ctypes. It decides
// nothing itself. A stand-alone host program: no HIP call, no GPU code; it links hz_seek_plan.cpp only, so
// the test builds it with the host's AddressSanitizer and UndefinedBehaviorSanitizer (their runtimes
// linked into the program: it needs nothing preloaded) and runs it as a child process in the
// environment it has. Host code only: it never opens a GPU, wherever it runs.
//
// Build (from the repository root):
//   hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined
//         -Iinclude -Ihuffman_amd/csrc tests/pieces_probe.cpp huffman_amd/csrc/hz_seek_plan.cpp -o pieces_probe
//
// Usage: pieces_probe IN
// IN (little endian u64 words): nsym, payload_bytes, nwords, seek[nwords], nlists, then per list
//   n, n x (sym_begin, sym_count, out_byte).
// Output, per list: "rc npieces buf_bytes seek_words", then one line of six numbers per piece and one
// line "sym_begin sym_count out_byte piece" per range (neither when rc is not 0).
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "huffman_amd.h"

namespace {

bool get(FILE* f, uint64_t* v, size_t n) { return fread(v, 8, n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t head[3], nlists;
    if (!get(f, head, 3)) return 2;
    std::vector<uint64_t> seek(head[2]);
    if (!get(f, seek.data(), seek.size()) || !get(f, &nlists, 1)) return 2;
    for (uint64_t l = 0; l < nlists; ++l) {
        uint64_t n;
        if (!get(f, &n, 1)) return 2;
        // exactly n entries each: a write past what the interface promises is the sanitizer's to find
        std::vector<hz_range> rg(n);
        std::vector<hz_piece> pieces(n);
        std::vector<hz_piece_range> out(n);
        for (uint64_t i = 0; i < n; ++i) {
            uint64_t w[3];
            if (!get(f, w, 3)) return 2;
            rg[i].sym_begin = w[0]; rg[i].sym_count = w[1]; rg[i].out_byte = w[2];
        }
        uint32_t np = 0;
        uint64_t buf_bytes = 0, seek_words = 0;
        const int rc = hz_seek_pieces(seek.data(), head[0], head[1], rg.data(), (uint32_t)n, pieces.data(), &np, out.data(),
                                      &buf_bytes, &seek_words);
        printf("%d %u %" PRIu64 " %" PRIu64 "\n", rc, np, buf_bytes, seek_words);
        if (rc) continue;
        for (uint32_t k = 0; k < np; ++k)
            printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", pieces[k].stream_byte,
                   pieces[k].bytes, pieces[k].buf_byte, pieces[k].first_block, pieces[k].seek_index, pieces[k].nblocks);
        for (uint64_t i = 0; i < n; ++i)
            printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", out[i].sym_begin, out[i].sym_count, out[i].out_byte,
                   out[i].piece);
    }
    fclose(f);
    return 0;
}
