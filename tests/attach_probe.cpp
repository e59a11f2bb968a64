// attach_probe.cpp -- the extract window's arithmetic (hz_stream_plan.h: ExtractWindow) in rounds of whole
// blocks, the option hz_seekable_attach_file and hz_extract_stream_verified run it with, driven round by
// round the way tests/stream_probe.cpp drives the plain window, with results printed as text for
// tests/test_attach_plan_host.py to judge. It decides nothing itself. A stand-alone host program: no HIP
// call, no GPU code, header only, so the test builds it with the host's AddressSanitizer and
// UndefinedBehaviorSanitizer (their runtimes linked into the program: it needs nothing preloaded) and runs it
// as a child process. Host code only: it never opens a GPU, wherever it runs.
//
// Build (from the repository root):
//   hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined
//         -Iinclude -Ihuffman_amd/csrc tests/attach_probe.cpp -o attach_probe
// With -DATTACH_PROBE_NO_FLAG it builds against a hz_stream_plan.h from before the option (the flag-off
// values recorded in tests/golden/attach_plan_flag_off.json were printed that way) and refuses flag = 1.
//
// attach_probe IN
//   IN (little endian u64 words), 8 words per case: flag, W, start_bit, max_len, nsym, pattern, min_len, salt.
//   Codeword i of a case is length(i) bits long (below; restated in the test), the codewords' positions are
//   the prefix sums from start_bit, and the "device" answers a round of k codewords with the true end bit
//   of codeword done + k. Per case "case I", then per round "k used tail refill redone", and "truncated"
//   if the window says so.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "hz_stream_plan.h"

using namespace hz;

namespace {

// pattern 0: every code min_len; 1: every code max_len; 2: the first half min_len, then max_len (the file's
// mean underestimates the second half: overruns and redos); 3: the other way round; 4: scattered over
// [min_len, max_len]; 5: runs of 3000 codes, min_len and max_len in turn.
uint64_t length(uint64_t i, uint64_t nsym, uint64_t pattern, uint64_t min_len, uint64_t max_len, uint64_t salt) {
    switch (pattern) {
        case 0: return min_len;
        case 1: return max_len;
        case 2: return i < nsym / 2 ? min_len : max_len;
        case 3: return i < nsym / 2 ? max_len : min_len;
        case 4: return min_len + (((i + salt) * 2654435761ull) >> 7) % (max_len - min_len + 1);
        default: return (i / 3000) % 2 ? max_len : min_len;
    }
}

bool words(const char* path, std::vector<uint64_t>& v) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint64_t x;
    while (fread(&x, 8, 1, f) == 1) v.push_back(x);
    fclose(f);
    return true;
}

int one_case(const uint64_t* c) {
    const uint64_t flag = c[0], W = c[1], start_bit = c[2], max_len = c[3], nsym = c[4];
    std::vector<uint64_t> pos(nsym + 1);  // pos[i]: the first bit of codeword i, from the payload's first byte
    pos[0] = start_bit;
    for (uint64_t i = 0; i < nsym; ++i) pos[i + 1] = pos[i] + length(i, nsym, c[5], c[6], max_len, c[7]);
    const uint64_t pay_total = (pos[nsym] + 7) / 8;
#ifdef ATTACH_PROBE_NO_FLAG
    if (flag) return 2;
    ExtractWindow w(W, nsym, pay_total, (uint32_t)start_bit, (uint32_t)max_len);
#else
    ExtractWindow w(W, nsym, pay_total, (uint32_t)start_bit, (uint32_t)max_len, flag != 0);
#endif
    auto device = [&](uint64_t k) { return pos.at(w.done + k) - 8 * w.consumed; };
    w.first_fill();
    uint64_t k = w.round_syms();
    while (w.done < nsym) {
        uint64_t end_bit = device(k);
        int redone = 0;
        if (w.overran(end_bit)) {
            k = w.redo_syms();
            end_bit = device(k);
            redone = 1;
        }
        if (w.truncated(end_bit)) {
            printf("truncated\n");
            return 0;
        }
        const ExtractWindow::Step s = w.advance(end_bit, k);
        printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %d\n", k, s.used, s.tail, s.r, redone);
        if (s.more) k = w.round_syms();
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    std::vector<uint64_t> v;
    if (argc != 2 || !words(argv[1], v) || v.size() % 8) return 2;
    for (size_t i = 0; i < v.size() / 8; ++i) {
        printf("case %zu\n", i);
        if (int rc = one_case(&v[8 * i])) return rc;
    }
    return 0;
}
