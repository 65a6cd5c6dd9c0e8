// Small POSIX helpers shared by the file-level sources (ec_files.cpp,
// verify_files.cpp, ec_read.cpp, ec_index.cpp): one copy of each.
#pragma once
#include <unistd.h>

#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>

#include "hec_internal.hpp"

namespace hec {

// A file descriptor closed on scope exit.
struct Fd {
    int fd = -1;
    ~Fd() {
        if (fd >= 0) ::close(fd);
    }
};

// A codec handle freed on scope exit.
struct RsGuard {
    hec_rs_t* rs = nullptr;
    ~RsGuard() { hec_rs_free(rs); }
};

inline std::string shard_name(const std::string& base, int i) {
    char ext[8];
    std::snprintf(ext, sizeof ext, ".ec%02d", i);  // to_ext, helyim-ec/src/lib.rs:84-86
    return base + ext;
}

inline uint64_t be64(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i) v = (v << 8) | p[i];
    return v;
}
inline uint32_t be32(const uint8_t* p) {
    return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | p[3];
}

// HEC_ERR_IO from errno: the calling thread's error ...
inline int io(const std::string& what) { return fail_errno(HEC_ERR_IO, what, errno); }
// ... or the first-error record shared by a pipeline's threads.
inline void io_error(ErrorSlot& e, const std::string& what) {
    const int err = errno;
    ErrorValues v;
    v.os_errno = err;
    e.set(HEC_ERR_IO, what + ": " + std::strerror(err), v);
}

// pread until n bytes or EOF, retrying EINTR: bytes read (< n: the file ended
// at off + that many), or -1 with errno set. What a short read means is the
// caller's policy.
inline ssize_t pread_full(int fd, uint8_t* dst, size_t n, uint64_t off) {
    size_t got = 0;
    while (got < n) {
        const ssize_t r = ::pread(fd, dst + got, n - got, off_t(off + got));
        if (r < 0) {
            if (errno == EINTR) continue;
            return -1;
        }
        if (r == 0) break;
        got += size_t(r);
    }
    return ssize_t(got);
}

// pwrite until n bytes are written, retrying EINTR and short writes; false
// with errno set on an error.
inline bool pwrite_full(int fd, const uint8_t* src, size_t n, uint64_t off) {
    size_t put = 0;
    while (put < n) {
        const ssize_t w = ::pwrite(fd, src + put, n - put, off_t(off + put));
        if (w < 0) {
            if (errno == EINTR) continue;
            return false;
        }
        put += size_t(w);
    }
    return true;
}

}  // namespace hec
