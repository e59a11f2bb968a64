// table_probe.cpp -- the device table images of a codebook, built on the host exactly as the uploads
// (hz_host.cpp hz_codebook_upload_encode_impl / hz_codebook_upload_decode_impl) decide to, written to a
// file for tests/test_table_images.py to check entry by entry against tests/table_model.py.
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

// hz_codebook_upload_encode_impl
void probe_encode(FILE* f, const hz_codebook* cb) {
    const int mode = select_enc_mode(cb);
    section(f, "enc", {{"mode", mode}}, kNone);
    if (mode == ENC_FIXED16) {
        section(f, "enc_fixed16", {}, build_enc_fixed16(cb));
    } else if (mode == ENC_DENSE) {
        section(f, "enc_dense", {}, build_enc_dense(cb));
    } else if (mode == ENC_HOT) {
        const uint32_t mask = choose_hot_mask(cb);
        section(f, "enc_hot", {{"mask", mask}}, build_enc_hot(cb, mask));
        section(f, "enc_esc", {{"mask", mask}}, build_enc_esc(cb, mask));
    }
    if (mode == ENC_WIDE) section(f, "enc_wide", {}, build_enc_wide(cb));
    if (mode != ENC_FIXED16) {
        section(f, "len8", {}, build_len8(cb));
        section(f, "lenpair", {}, build_lenpair(cb));
    }
}

// hz_codebook_upload_decode_impl
void probe_decode(FILE* f, const hz_codebook* cb) {
    const int mode = select_dec_mode(cb);
    std::vector<uint32_t> dimg, l2, wimg, wesc;
    int k = 0, lvl = 0, rc = HZ_OK;
    if (mode == DEC_FIXED16) { dimg = build_dec_fixed16(cb); k = 16; }
    else if (mode == DEC_DENSE) rc = build_dec_dense(cb, dimg, k);
    else rc = build_dec_lut(cb, dimg, l2, k, lvl);
    if (!rc) {
        while (dimg.size() % 4) dimg.push_back(0);
        if (mode != DEC_FIXED16 && dimg.size() * 4 + 4 * dec_slot_words_max((int)cb->max_len) > kLdsBytes) rc = HZ_ENOMEM;
    }
    section(f, "dec", {{"mode", mode}, {"rc", rc}}, kNone);
    if (rc) return;
    if (l2.empty()) l2.push_back(lut_leaf_entry(1, 0));
    const char* names[] = {"dec_dense", "dec_lut", "dec_fixed16"};
    section(f, names[mode], {{"k", k}, {"lvl", lvl}}, dimg);
    section(f, "dec_l2", {}, l2);
    bool walker = false;
    int walk_m = 0;
    if (mode != DEC_FIXED16 && cb->max_len >= 1 && cb->max_len <= (uint32_t)kWalkMaxLen) {
        int wk = 0, wm = 0, bias = 0;
        build_walk_len(cb, wimg, wesc, wk, wm, bias);
        if (wimg.size() * 4 <= (1u << kWalkK) / 2) {
            if (wesc.empty()) wesc.push_back(0x01010101u);
            section(f, "walk_len", {{"k", wk}, {"m", wm}, {"bias", bias}}, wimg);
            section(f, "walk_esc", {{"m", wm}}, wesc);
            walker = true;
            walk_m = wm;
        }
    }
    if (mode != DEC_FIXED16 && cb->max_len >= 1) {
        std::vector<uint32_t> w8;
        int k8 = 0;
        build_walk8(cb, w8, k8);
        section(f, "walk8", {{"k", k8}}, w8);
        if (walker) {
            section(f, "chain_esc", {{"m", walk_m}, {"shared", 1}}, kNone);  // the index walker's table
        } else {
            std::vector<uint32_t> cesc;
            int m = 0;
            build_chain_esc(cb, cesc, m);
            section(f, "chain_esc", {{"m", m}, {"shared", 0}}, cesc);
        }
        if (mode != DEC_LUT) {  // DENSE: a LUT image beside the DENSE decoder's
            std::vector<uint32_t> cimg, cl2;
            int ck = 0, clvl = 0;
            const int crc = build_dec_lut(cb, cimg, cl2, ck, clvl);
            if (!crc) {
                while (cimg.size() % 4) cimg.push_back(0);
                if (cl2.empty()) cl2.push_back(lut_leaf_entry(1, 0));
            } else {
                cimg.clear();
                cl2.clear();
            }
            section(f, "chain_lut", {{"k", ck}, {"lvl", clvl}, {"rc", crc}}, cimg);
            section(f, "chain_l2", {}, cl2);
        }
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
