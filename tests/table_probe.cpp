// table_probe.cpp -- the device table images of a codebook, built on the host through the uploads' own
// plan (hz_codebook.cpp build_enc_images / build_dec_images / build_indexless_images, which hz_host.cpp's
// hz_codebook_upload_encode / hz_codebook_upload_decode stage), written to a file for
// tests/test_table_images.py to check entry by entry against tests/table_model.py. It decides nothing
// itself: it names the sections and writes what the plan returns.
// A stand-alone host program: no HIP call, no GPU code; it links hz_codebook.cpp only.
//
// Build (from the repository root):
//   hipcc -O1 -std=c++17 -Iinclude -Ihuffman_amd/csrc tests/table_probe.cpp huffman_amd/csrc/hz_codebook.cpp
//         -o table_probe
// and, for the manual sanitizer run on a CPU machine (never on a GPU machine, never from pytest):
//   hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined
//         -Iinclude -Ihuffman_amd/csrc tests/table_probe.cpp huffman_amd/csrc/hz_codebook.cpp -o table_probe_san
//
// Usage: table_probe BOOK OUT [BOOK OUT ...]
// BOOK (little endian): u32 nsym, u32 min_len, u32 max_len, u8 len[65536], u64 code[65536].
// OUT: the magic "HZTP0001", then sections until the end of the file, each
//   char name[24]; u32 nparam; u32 word_bytes (4 or 8); u64 nwords;
//   nparam x { char name[24]; i64 value };  nwords x word (little endian)
// A builder that fails leaves a section of no words with its status in the parameter "rc".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "huffman_amd.h"
#include "hz_internal.h"

using namespace hz;

namespace {

using Params = std::vector<std::pair<const char*, int64_t>>;

void put_name(FILE* f, const char* name) {
    char b[24] = {0};
    strncpy(b, name, 23);
    fwrite(b, 1, 24, f);
}

template <typename T>
void section(FILE* f, const char* name, const Params& params, const std::vector<T>& words) {
    put_name(f, name);
    const uint32_t np = (uint32_t)params.size(), wb = (uint32_t)sizeof(T);
    const uint64_t nw = words.size();
    fwrite(&np, 4, 1, f);
    fwrite(&wb, 4, 1, f);
    fwrite(&nw, 8, 1, f);
    for (const auto& p : params) {
        put_name(f, p.first);
        fwrite(&p.second, 8, 1, f);
    }
    if (nw) fwrite(words.data(), sizeof(T), nw, f);
}

const std::vector<uint32_t> kNone;

// What hz_codebook_upload_encode stages.
void probe_encode(FILE* f, const hz_codebook* cb) {
    EncImages e;
    build_enc_images(cb, e);
    section(f, "enc", {{"mode", e.mode}}, kNone);
    // an image exists where it is not empty; the mode only names the LDS image
    const char* names[] = {"enc_dense", "enc_hot", "enc_wide", "enc_fixed16"};
    const Params mask = e.esc.empty() ? Params{} : Params{{"mask", e.hot_mask}};  // the pair that shares it
    if (!e.lds.empty()) section(f, names[e.mode], mask, e.lds);
    if (!e.esc.empty()) section(f, "enc_esc", mask, e.esc);
    if (!e.wide.empty()) section(f, "enc_wide", {}, e.wide);
    if (!e.len8.empty()) section(f, "len8", {}, e.len8);
    if (!e.lenpair.empty()) section(f, "lenpair", {}, e.lenpair);
}

// What hz_codebook_upload_decode stages: the decode set, then the index-less set.
void probe_decode(FILE* f, const hz_codebook* cb) {
    DecImages d;
    const int rc = build_dec_images(cb, d);
    section(f, "dec", {{"mode", d.mode}, {"rc", rc}}, kNone);
    if (rc) return;
    const char* names[] = {"dec_dense", "dec_lut", "dec_fixed16"};
    section(f, names[d.mode], {{"k", d.k}, {"lvl", d.level_bits}}, d.lds);
    section(f, "dec_l2", {}, d.l2);
    IndexlessImages x;
    const int crc = build_indexless_images(cb, d, x);
    if (!x.walk_lds.empty()) {
        section(f, "walk_len", {{"k", x.walk_k}, {"m", x.walk_m}, {"bias", x.walk_bias}}, x.walk_lds);
        section(f, "walk_esc", {{"m", x.walk_m}}, x.walk_esc);
    }
    if (x.walk8.empty()) return;  // FIXED16: no index-less tables
    section(f, "walk8", {{"k", x.walk8_k}}, x.walk8);
    // shared: the index walker's table, no words here
    section(f, "chain_esc", {{"m", x.chain_esc_m}, {"shared", x.chain_esc.empty()}}, x.chain_esc);
    if (!x.chain_lds.empty() || crc) {  // DENSE: a LUT image beside the DENSE decoder's (or its failure)
        section(f, "chain_lut", {{"k", x.chain_k}, {"lvl", x.chain_level_bits}, {"rc", crc}}, x.chain_lds);
        section(f, "chain_l2", {}, x.chain_l2);
    }
}

int probe(const char* in, const char* out) {
    static hz_codebook cb;
    memset(&cb, 0, sizeof(cb));
    FILE* f = fopen(in, "rb");
    if (!f) { perror(in); return 1; }
    uint32_t head[3];
    const bool ok = fread(head, 4, 3, f) == 3 && fread(cb.len, 1, HZ_NSYM, f) == HZ_NSYM &&
                    fread(cb.code, 8, HZ_NSYM, f) == HZ_NSYM;
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: short codebook file\n", in); return 1; }
    cb.nsym = head[0];
    cb.min_len = head[1];
    cb.max_len = head[2];
    if (cb.nsym == 0 || cb.nsym > HZ_NSYM || cb.min_len < 1 || cb.max_len > HZ_MAXLEN || cb.min_len > cb.max_len) {
        fprintf(stderr, "%s: not a codebook the uploads take\n", in);
        return 1;
    }
    f = fopen(out, "wb");
    if (!f) { perror(out); return 1; }
    fwrite("HZTP0001", 1, 8, f);
    section(f, "consts",
            {{"kLdsBytes", kLdsBytes}, {"kLutGlobal", kLutGlobal}, {"kLutMaxL2", kLutMaxL2},
             {"kDecLutMaxK1", kDecLutMaxK1}, {"kDecLevelBits", kDecLevelBits}, {"kDecMaxWaves", kDecMaxWaves},
             {"kDecMinLdsWords", kDecMinLdsWords}, {"kWalkK", kWalkK}, {"kWalkMaxLen", kWalkMaxLen},
             {"kChainEscMaxBits", kChainEscMaxBits}, {"kHotMaxLen", kHotMaxLen}, {"kNarrowMaxLen", kNarrowMaxLen},
             {"kBlockSyms", kBlockSyms}, {"kChainSyms", kChainSyms}},
            kNone);
    probe_encode(f, &cb);
    probe_decode(f, &cb);
    const bool bad = ferror(f) != 0;
    return (fclose(f) != 0 || bad) ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3 || (argc - 1) % 2) {
        fprintf(stderr, "usage: %s BOOK OUT [BOOK OUT ...]\n", argv[0]);
        return 2;
    }
    for (int i = 1; i + 1 < argc; i += 2)
        if (probe(argv[i], argv[i + 1])) return 1;
    return 0;
}
