// hz_file_io.cpp -- the file reader and writer of `archive` / `extract` and of the by-path range reads
// (hz_file_io.h). The only multi-threaded host code of the library; it makes no HIP call.
#include "hz_file_io.h"

#include <errno.h>
#include <fcntl.h>
#include <stdlib.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>

namespace hz {

namespace {

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

}  // namespace

int pread_all(int fd, uint8_t* p, uint64_t n, uint64_t off) {
    for (uint64_t done = 0; done < n;) {
        const ssize_t r = ::pread(fd, p + done, n - done, (off_t)(off + done));
        if (r <= 0) return HZ_EIO;
        done += (uint64_t)r;
    }
    return HZ_OK;
}

int pwrite_all(int fd, const uint8_t* p, uint64_t n, uint64_t off) {
    for (uint64_t done = 0; done < n;) {
        const ssize_t w = ::pwrite(fd, p + done, n - done, (off_t)(off + done));
        if (w <= 0) return HZ_EIO;
        done += (uint64_t)w;
    }
    return HZ_OK;
}

uint64_t env_u64(const char* name, uint64_t floor, uint64_t dflt) {
    const char* v = getenv(name);
    const uint64_t x = v ? strtoull(v, nullptr, 10) : 0;
    return v && x >= floor ? x : dflt;
}

std::string output_name() {
    const std::string base = "DECOMPRESSED_FILE";
    std::string name = base;
    for (int k = 1; k < 10 && access(name.c_str(), F_OK) == 0; ++k) name = base + "(" + std::to_string(k) + ")";
    return name;
}

FileReader::~FileReader() {
    if (fd_ >= 0) ::close(fd_);
}

int FileReader::open(const char* path) {
    fd_ = ::open(path, O_RDONLY);
    if (fd_ < 0) return errno == ENOENT || errno == ENOTDIR ? HZ_ENOENT : HZ_EIO;
    struct stat st;
    if (fstat(fd_, &st) != 0) return HZ_EIO;
    size_ = (uint64_t)st.st_size;
    return HZ_OK;
}

int FileReader::read(uint8_t* p, uint64_t n, uint64_t off) {
    if (n == 0) return HZ_OK;
    const auto t0 = Clock::now();
    bool ok;
    if (n < (16u << 20)) {
        ok = pread_all(fd_, p, n, off) == HZ_OK;
    } else {
        const int fd = fd_;
        const uint64_t piece = ((n + kReaders - 1) / kReaders + 4095) & ~(uint64_t)4095;
        std::atomic<bool> bad{false};
        std::vector<std::thread> th;
        // joins every started reader on every exit, a failed thread spawn (std::system_error,
        // turned into an HZ_ status by the caller's guard) included
        struct Joiner {
            std::vector<std::thread>& v;
            ~Joiner() { for (auto& t : v) if (t.joinable()) t.join(); }
        } joiner{th};
        for (uint64_t a = 0; a < n && !bad; a += piece) {
            const uint64_t len = std::min(piece, n - a);
            th.emplace_back([&bad, fd, p, a, len, off] {
                if (pread_all(fd, p + a, len, off + a)) bad = true;
            });
        }
        for (auto& t : th) t.join();
        th.clear();
        ok = !bad;
    }
    if (t_) {
        t_->fread_ms += ms_since(t0);
        t_->bytes_in += ok ? n : 0;
    }
    return ok ? HZ_OK : HZ_EIO;
}

FileWriter::~FileWriter() {
    (void)wait();
    if (fd_ >= 0) ::close(fd_);
}

int FileWriter::open(const char* path) {
    fd_ = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    return fd_ >= 0 ? HZ_OK : HZ_EIO;
}

void FileWriter::reserve(uint64_t size) {
    if (fd_ >= 0 && size > 0) reserved_ = ::posix_fallocate(fd_, 0, (off_t)size) == 0;
}

void FileWriter::start(const uint8_t* p, uint64_t n, uint64_t off) {
    if (n == 0) return;
    t0_ = Clock::now();
    end_ = std::max(end_, off + n);
    const uint64_t nt = n < (8u << 20) ? 1 : kWriters;
    const uint64_t piece = ((n + nt - 1) / nt + 4095) & ~(uint64_t)4095;
    for (uint64_t a = 0; a < n; a += piece) {
        const uint64_t len = std::min(piece, n - a);
        th_.emplace_back([this, p, a, len, off] {
            if (pwrite_all(fd_, p + a, len, off + a)) err_ = true;
        });
    }
    if (t_) t_->bytes_out += n;
}

int FileWriter::wait() {
    if (th_.empty()) return err_ ? HZ_EIO : HZ_OK;
    for (auto& t : th_) t.join();
    th_.clear();
    if (t_) t_->fwrite_ms += ms_since(t0_);
    return err_ ? HZ_EIO : HZ_OK;
}

int FileWriter::write_now(const uint8_t* p, uint64_t n, uint64_t off) {
    int rc = wait();
    if (rc) return rc;
    start(p, n, off);
    return wait();
}

int FileWriter::close() {
    int rc = wait();
    // the file ends at its last written byte, whatever reserve() allocated
    if (fd_ >= 0 && reserved_ && ::ftruncate(fd_, (off_t)end_) != 0) rc = HZ_EIO;
    if (fd_ >= 0 && ::close(fd_) != 0) rc = HZ_EIO;
    fd_ = -1;
    return rc;
}

}  // namespace hz
