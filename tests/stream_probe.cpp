// stream_probe.cpp -- the file reader and writer of `archive` / `extract` (hz_file_io.cpp) on real files,
// and the flows' window and chunk arithmetic (hz_stream_plan.h) driven round by round, with results
// printed as text for tests/test_stream_host.py to judge. It decides nothing itself. A stand-alone host
// program: no HIP call, no GPU code; it links hz_file_io.cpp only (hz_stream_plan.h is header-only), so the
// test builds it twice, with the host's AddressSanitizer and UndefinedBehaviorSanitizer and with
// ThreadSanitizer (their runtimes linked into the program: it needs nothing preloaded), and runs it as a
// child process in the environment it has. Host code only: it never opens a GPU, wherever it runs.
//
// Build (from the repository root), either
//   hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined
//         -Iinclude -Ihuffman_amd/csrc tests/stream_probe.cpp huffman_amd/csrc/hz_file_io.cpp -o stream_probe
// or the same with -Xarch_host -fsanitize=thread in place of the two sanitizer options.
//
// Byte i of every file read or written here is fill(i) below.
//
// stream_probe reader MISSING FILE...
//   per FILE "size whole at1 at4097 bytes_in past_rc bytes_in_after": the file read whole and from offsets
//   1 and 4097 to its end (1 when the bytes equal fill, 0 otherwise; an offset past the end reads nothing),
//   the timing record's bytes_in after the three, the status of a read of size + 1 bytes, bytes_in after
//   it; then "missing rc": the status of opening MISSING.
// stream_probe writer PATH
//   1 byte by start, 8 MiB - 1 by start after wait, 8 MiB + 4097 by write_now, at increasing offsets, into
//   a file reserved at twice their sum: "rc_open rc_wait rc_write_now rc_close bytes_out".
// stream_probe full PATH
//   PATH is a device that takes no byte: "rc_open rc_write_now rc_close", then a second writer left to
//   its destructor with a write in flight, then "joined".
// stream_probe window IN
//   IN (little endian u64 words): W, start_bit, max_len, n, then n code lengths. The codewords' positions
//   are the prefix sums from start_bit; the "device" answers a round of k codewords with the true end bit
//   of codeword done + k. Per round "k used tail refill redone"; "truncated" if the window says so.
// stream_probe carry IN
//   IN (u64 words): start_bit, nchunks, then the code bits of each chunk. Per chunk "bytes sbit needs_lead",
//   the chunk's end bit being its first code's bit in its first word plus its code bits.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "hz_file_io.h"
#include "hz_stream_plan.h"

using namespace hz;

namespace {

uint8_t fill(uint64_t i) { return (uint8_t)((i * 2654435761ull) >> 13); }

std::vector<uint8_t> filled(uint64_t off, uint64_t n) {
    std::vector<uint8_t> v(n);
    for (uint64_t i = 0; i < n; ++i) v[i] = fill(off + i);
    return v;
}

// [off, size) of the file through the reader, into a buffer of exactly that size: 1 when it equals fill
int read_from(FileReader& f, uint64_t off) {
    if (off > f.size()) return 1;
    std::vector<uint8_t> got(f.size() - off, 0xEE);
    if (f.read(got.data(), got.size(), off)) return 0;
    return got == filled(off, got.size()) ? 1 : 0;
}

int reader(int nfiles, char** files, const char* missing) {
    for (int i = 0; i < nfiles; ++i) {
        hz_stream_timing t = hz_stream_timing();
        FileReader f(&t);
        if (f.open(files[i])) return 2;
        const int whole = read_from(f, 0), at1 = read_from(f, 1), at4097 = read_from(f, 4097);
        const uint64_t bytes_in = t.bytes_in;
        std::vector<uint8_t> past(f.size() + 1);
        const int past_rc = f.read(past.data(), past.size(), 0);
        printf("%" PRIu64 " %d %d %d %" PRIu64 " %d %" PRIu64 "\n", f.size(), whole, at1, at4097, bytes_in, past_rc,
               (uint64_t)t.bytes_in);
    }
    FileReader f(nullptr);
    printf("missing %d\n", f.open(missing));
    return 0;
}

int writer(const char* path) {
    const uint64_t n0 = 1, n1 = (8u << 20) - 1, n2 = (8u << 20) + 4097;
    const std::vector<uint8_t> b0 = filled(0, n0), b1 = filled(n0, n1), b2 = filled(n0 + n1, n2);  // before the writer
    hz_stream_timing t = hz_stream_timing();
    FileWriter w(&t);
    const int rc_open = w.open(path);
    w.reserve(2 * (n0 + n1 + n2));
    w.start(b0.data(), n0, 0);
    const int rc_w0 = w.wait();
    w.start(b1.data(), n1, n0);  // in flight when write_now comes: it waits first
    const int rc_now = w.write_now(b2.data(), n2, n0 + n1);
    const int rc_close = w.close();
    printf("%d %d %d %d %" PRIu64 "\n", rc_open, rc_w0, rc_now, rc_close, (uint64_t)t.bytes_out);
    return 0;
}

int full(const char* path) {
    const std::vector<uint8_t> big = filled(0, (8u << 20) + 4097);
    hz_stream_timing t = hz_stream_timing();
    {
        FileWriter w(&t);
        const int rc_open = w.open(path);
        const int rc_now = w.write_now(big.data(), big.size(), 0);
        const int rc_close = w.close();
        printf("%d %d %d\n", rc_open, rc_now, rc_close);
    }
    {
        FileWriter w(&t);
        if (w.open(path)) return 2;
        w.start(big.data(), big.size(), 0);
    }
    printf("joined\n");
    return 0;
}

bool words(const char* path, std::vector<uint64_t>& v) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint64_t x;
    while (fread(&x, 8, 1, f) == 1) v.push_back(x);
    fclose(f);
    return true;
}

int window(const char* in) {
    std::vector<uint64_t> v;
    if (!words(in, v) || v.size() < 4 || v.size() != 4 + v[3]) return 2;
    const uint64_t W = v[0], start_bit = v[1], max_len = v[2], nsym = v[3];
    std::vector<uint64_t> pos(nsym + 1);  // pos[i]: the first bit of codeword i, from the payload's first byte
    pos[0] = start_bit;
    for (uint64_t i = 0; i < nsym; ++i) pos[i + 1] = pos[i] + v[4 + i];
    const uint64_t pay_total = (pos[nsym] + 7) / 8;
    ExtractWindow w(W, nsym, pay_total, (uint32_t)start_bit, (uint32_t)max_len);
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
            return 1;
        }
        const ExtractWindow::Step s = w.advance(end_bit, k);
        printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %d\n", k, s.used, s.tail, s.r, redone);
        if (s.more) k = w.round_syms();
    }
    return 0;
}

int carry(const char* in) {
    std::vector<uint64_t> v;
    if (!words(in, v) || v.size() < 2 || v.size() != 2 + v[1]) return 2;
    uint32_t sbit = (uint32_t)v[0];
    for (uint64_t i = 0; i < v[1]; ++i) {
        const ArchiveChunks::Carry c = ArchiveChunks::carry_after(sbit + v[2 + i], i + 1 == v[1]);
        printf("%" PRIu64 " %u %d\n", c.bytes, c.sbit, c.needs_lead ? 1 : 0);
        sbit = c.sbit;
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string cmd = argv[1];
    if (cmd == "reader") return reader(argc - 3, argv + 3, argv[2]);
    if (cmd == "writer") return writer(argv[2]);
    if (cmd == "full") return full(argv[2]);
    if (cmd == "window") return window(argv[2]);
    if (cmd == "carry") return carry(argv[2]);
    return 2;
}
