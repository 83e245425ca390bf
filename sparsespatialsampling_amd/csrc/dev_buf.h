// The one owner of a device allocation in libs3hip.so: a move-only pointer to `n` elements of T that frees what it holds
// when it goes out of scope.  Handles keep their tables in DevBufs and every per-call temporary is a local DevBuf, so an
// early return (S3_REQUIRE, S3_HIP_CHECK, an exception) releases by scope and nothing is freed by name.
//
// No HIP header here: Mem is a policy with `static int alloc(void **, size_t bytes)` (0 = success, else the allocator's
// status code) and `static void free(void *)`.  The library's policy is s3::HipMem (common.h: hipMalloc / hipFree, no pool);
// tests/native/dev_buf_test.cpp instantiates the class over a counting host allocator.
#pragma once

#include <cstddef>
#include <utility>

namespace s3 {

struct HipMem;

template <typename T, typename Mem = HipMem>
class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.release()) {}
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.release();
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    // max(n, 1) elements; what was held is freed first; null on failure
    int alloc(size_t n) {
        reset();
        void *q = nullptr;
        const int e = Mem::alloc(&q, sizeof(T) * (n ? n : 1));
        if (e == 0) p_ = static_cast<T *>(q);
        return e;
    }
    void reset() {
        if (p_) Mem::free(p_);
        p_ = nullptr;
    }
    T *release() { return std::exchange(p_, nullptr); }
    T *get() const { return p_; }
    operator T *() const { return p_; }      // kernel arguments and pointer arithmetic read as with a raw pointer

  private:
    T *p_ = nullptr;
};

}  // namespace s3
