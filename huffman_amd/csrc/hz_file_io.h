// hz_file_io.h -- the file I/O of the file-level flows: positional reads and writes that loop until done,
// a reader and a writer that go through 8 threads for large transfers, the extract's output name and the
// environment's sizes. No HIP call and no device memory: hz_file_io.cpp links alone, so a stand-alone
// host program runs it under the address, undefined-behaviour and thread sanitizers
// (tests/stream_probe.cpp). Private to the library.
#pragma once
#include <stdint.h>

#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "huffman_amd.h"

namespace hz {

// n bytes at file offset off, however many calls that takes. HZ_EIO for an error and for a file that
// ends (a device that is full) before n bytes.
int pread_all(int fd, uint8_t* p, uint64_t n, uint64_t off);
int pwrite_all(int fd, const uint8_t* p, uint64_t n, uint64_t off);

// A size from the environment: the variable's decimal value when it is at least `floor`, else dflt.
uint64_t env_u64(const char* name, uint64_t floor, uint64_t dflt);

// Decompressor.cu:185-219: "DECOMPRESSED_FILE", else "DECOMPRESSED_FILE(k)", k = 1..9.
std::string output_name();

// An input file: opened, sized by fstat of the descriptor it reads, read at the offsets the caller
// names (no stream position). Reads of 16 MiB and more go through 8 threads' positional reads: a single
// read copies out of the page cache at ~15 GB/s on the MI355X host. `timing` (nullable) takes the
// reads' wall time and bytes, added by the calling thread only.
class FileReader {
  public:
    explicit FileReader(hz_stream_timing* timing) : t_(timing) {}
    ~FileReader();
    FileReader(const FileReader&) = delete;
    FileReader& operator=(const FileReader&) = delete;
    int open(const char* path);  // HZ_ENOENT for a missing path, HZ_EIO for any other failure
    uint64_t size() const { return size_; }
    int fd() const { return fd_; }
    int read(uint8_t* p, uint64_t n, uint64_t off);  // all of [off, off + n), or HZ_EIO
  private:
    static constexpr uint64_t kReaders = 8;
    hz_stream_timing* t_;
    int fd_ = -1;
    uint64_t size_ = 0;
};

// Output file written by background positional writes, so a chunk's write
// overlaps the next chunk's device work. The file's final size is reserved
// first (posix_fallocate): into page cache, 8 threads then write ~12 GB/s on
// the MI355X host, against ~5 GB/s for one or 8 threads into a file that grows
// (block allocation under the inode lock), 6.8 GB/s with O_DIRECT and 1.7 GB/s
// copying into a shared mmap (tools/debug/write_bw.py, 8 GiB). start() hands a
// buffer to kWriters threads (one slice each) and returns; wait() joins them.
// One write is in flight at a time, so the caller double-buffers. `timing`
// (nullable) is touched by the calling thread only, never by the writers.
class FileWriter {
  public:
    explicit FileWriter(hz_stream_timing* timing) : t_(timing) {}
    ~FileWriter();
    FileWriter(const FileWriter&) = delete;
    FileWriter& operator=(const FileWriter&) = delete;
    int open(const char* path);
    // Reserve the file's final size (best effort: a file system without
    // fallocate only loses the speed-up).
    void reserve(uint64_t size);
    void start(const uint8_t* p, uint64_t n, uint64_t off);
    int wait();
    int write_now(const uint8_t* p, uint64_t n, uint64_t off);
    int close();
  private:
    using Clock = std::chrono::steady_clock;
    static constexpr uint64_t kWriters = 8;
    hz_stream_timing* t_;
    int fd_ = -1;
    bool reserved_ = false;
    uint64_t end_ = 0;
    std::vector<std::thread> th_;
    std::atomic<bool> err_{false};
    Clock::time_point t0_;
};

}  // namespace hz
