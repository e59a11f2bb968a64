// salvage_probe.cpp -- the windows of hz_seekable_salvage_file (hz_salvage_plan.h: SalvagePlan) over seek
// tables that the test wrote, damaged entries included, with the windows printed as text for
// tests/test_salvage_plan_host.py to judge. It decides nothing itself. A stand-alone host program: no HIP
// call, no GPU code, header only, so the test builds it with the host's AddressSanitizer and
// UndefinedBehaviorSanitizer, unsigned wrap-around trapped as well (the plan promises that nothing wraps
// whatever the entries hold), their runtimes linked into the program: it needs nothing preloaded and runs as
// a child process. Host code only: it never opens a GPU, wherever it runs.
//
// Build (from the repository root):
//   hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined,unsigned-integer-overflow
//         -Xarch_host -fno-sanitize-recover=all -Iinclude -Ihuffman_amd/csrc tests/salvage_probe.cpp -o salvage_probe
//
// salvage_probe IN
//   IN (little endian u64 words), per case: nblocks, payload_bytes, max_len, chunk_bytes, then the nblocks + 1
//   entries of the table. Per case "case I", then per window "first_block nblocks byte_begin byte_end".
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "hz_salvage_plan.h"

using namespace hz;

namespace {

bool words(const char* path, std::vector<uint64_t>& v) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint64_t x;
    while (fread(&x, 8, 1, f) == 1) v.push_back(x);
    fclose(f);
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    std::vector<uint64_t> v;
    if (argc != 2 || !words(argv[1], v)) return 2;
    size_t at = 0;
    for (size_t i = 0; at < v.size(); ++i) {
        if (v.size() - at < 4) return 2;
        const uint64_t nblocks = v[at], payload_bytes = v[at + 1], max_len = v[at + 2], chunk_bytes = v[at + 3];
        at += 4;
        if (nblocks >= v.size() - at) return 2;
        // a copy of exactly nblocks + 1 entries: a read past the table is a read past the allocation
        const std::vector<uint64_t> table(v.begin() + (ptrdiff_t)at, v.begin() + (ptrdiff_t)(at + nblocks + 1));
        at += nblocks + 1;
        printf("case %zu\n", i);
        SalvagePlan plan(table.data(), nblocks, payload_bytes, (uint32_t)max_len, chunk_bytes);
        SalvageWindow w;
        while (plan.next(&w))
            printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", w.first_block, w.nblocks, w.byte_begin, w.byte_end);
    }
    return 0;
}
