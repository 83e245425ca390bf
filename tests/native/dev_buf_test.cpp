// CPU test driver of the device-memory owner (sparsespatialsampling_amd/csrc/dev_buf.h), built by tests/test_sanitizers.py with
// -fsanitize=address,undefined.  DevBuf is instantiated over a counting host allocator: every case ends with zero outstanding
// blocks, asserted on the counter (not left to LeakSanitizer); a free of a pointer the allocator does not know aborts.
#include "dev_buf.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <set>
#include <stdexcept>
#include <utility>

struct CountingMem {
    static std::set<void *> live;
    static int allocs;                 // allocations attempted so far
    static int fail_at;                // the allocs-th attempt (1-based) fails; 0 = none
    static size_t last_bytes;
    static int alloc(void **p, size_t bytes) {
        ++allocs;
        last_bytes = bytes;
        if (allocs == fail_at) {
            *p = nullptr;
            return 2;                  // any non-zero status
        }
        *p = std::malloc(bytes);
        if (!*p) std::abort();
        live.insert(*p);
        return 0;
    }
    static void free(void *p) {
        if (live.erase(p) != 1) {
            std::fprintf(stderr, "dev_buf_test: free of an unknown pointer\n");
            std::abort();
        }
        std::free(p);
    }
    static void fail_next(int n) { fail_at = allocs + n; }
    static int outstanding() { return (int)live.size(); }
};
std::set<void *> CountingMem::live;
int CountingMem::allocs = 0;
int CountingMem::fail_at = 0;
size_t CountingMem::last_bytes = 0;

template <typename T>
using Buf = s3::DevBuf<T, CountingMem>;

static int checks = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        ++checks;                                                                         \
        if (!(cond)) {                                                                    \
            std::fprintf(stderr, "dev_buf_test: %s (line %d)\n", #cond, __LINE__);        \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)
#define CASE_END() CHECK(CountingMem::outstanding() == 0)

struct Handle {                        // a handle of several owners, as s3_knn / s3_interp_plan
    Buf<double> pts;
    Buf<int32_t> orig, cell_start;
    int n = 0;
};

static int create(int fail_nth, Handle **out) {      // the creators' pattern: unique_ptr, release() on success
    *out = nullptr;
    std::unique_ptr<Handle> h(new Handle());
    if (fail_nth) CountingMem::fail_next(fail_nth);
    Buf<int32_t> tmp;
    if (int e = h->pts.alloc(30)) return e;
    if (int e = tmp.alloc(10)) return e;
    if (int e = h->orig.alloc(10)) return e;
    if (int e = h->cell_start.alloc(11)) return e;
    h->n = 10;
    *out = h.release();
    return 0;
}

static void throws_between(bool do_throw) {
    Buf<double> a, b;
    if (a.alloc(8) != 0) std::abort();
    if (do_throw) throw std::runtime_error("between two allocations");
    if (b.alloc(8) != 0) std::abort();
}

int main() {
    {   // default state, destructor
        Buf<double> a;
        CHECK(a.get() == nullptr && !a);
        {
            Buf<double> b;
            CHECK(b.alloc(16) == 0 && b.get() != nullptr && CountingMem::last_bytes == 16 * sizeof(double));
            b[3] = 1.5;                                    // through operator T *
            double *raw = b;
            CHECK(raw == b.get() && raw[3] == 1.5 && b + 3 == raw + 3);
            CHECK(CountingMem::outstanding() == 1);
        }
        CASE_END();
    }
    {   // reset, twice
        Buf<int32_t> a;
        CHECK(a.alloc(4) == 0);
        a.reset();
        CHECK(a.get() == nullptr && CountingMem::outstanding() == 0);
        a.reset();
        CASE_END();
    }
    {   // move construction leaves the source null
        Buf<int32_t> a;
        CHECK(a.alloc(4) == 0);
        int32_t *raw = a.get();
        Buf<int32_t> b(std::move(a));
        CHECK(a.get() == nullptr && b.get() == raw && CountingMem::outstanding() == 1);
    }
    CASE_END();
    {   // move assignment over a live buffer frees it; from a null owner it empties
        Buf<int32_t> a, b, c;
        CHECK(a.alloc(4) == 0 && b.alloc(4) == 0);
        int32_t *raw = a.get();
        b = std::move(a);
        CHECK(a.get() == nullptr && b.get() == raw && CountingMem::outstanding() == 1);
        b = std::move(c);
        CHECK(b.get() == nullptr && CountingMem::outstanding() == 0);
    }
    CASE_END();
    {   // self-move keeps the buffer
        Buf<int32_t> a;
        CHECK(a.alloc(4) == 0);
        int32_t *raw = a.get();
        Buf<int32_t> &same = a;
        a = std::move(same);
        CHECK(a.get() == raw && CountingMem::outstanding() == 1);
    }
    CASE_END();
    {   // release gives the pointer up
        Buf<int32_t> a;
        CHECK(a.alloc(4) == 0);
        int32_t *raw = a.release();
        CHECK(a.get() == nullptr && raw != nullptr && CountingMem::outstanding() == 1);
        CountingMem::free(raw);
    }
    CASE_END();
    {   // std::swap, also with a null owner
        Buf<double> a, b, c;
        CHECK(a.alloc(4) == 0 && b.alloc(4) == 0);
        double *ra = a.get(), *rb = b.get();
        std::swap(a, b);
        CHECK(a.get() == rb && b.get() == ra && CountingMem::outstanding() == 2);
        std::swap(a, c);
        CHECK(a.get() == nullptr && c.get() == rb && CountingMem::outstanding() == 2);
    }
    CASE_END();
    {   // alloc over a live buffer frees it first; alloc(0) holds one element
        Buf<double> a;
        CHECK(a.alloc(4) == 0 && a.alloc(8) == 0 && CountingMem::outstanding() == 1);
        CHECK(a.alloc(0) == 0 && a.get() != nullptr && CountingMem::last_bytes == sizeof(double));
        a[0] = 2.0;
        CHECK(CountingMem::outstanding() == 1);
    }
    CASE_END();
    {   // a failing alloc: status handed on, owner null, counter unchanged -- on an empty owner and over a live buffer
        Buf<double> a, b;
        CHECK(b.alloc(4) == 0);
        CountingMem::fail_next(1);
        CHECK(a.alloc(4) == 2 && a.get() == nullptr && CountingMem::outstanding() == 1);
        CountingMem::fail_next(1);
        CHECK(b.alloc(4) == 2 && b.get() == nullptr && CountingMem::outstanding() == 0);
        CHECK(a.alloc(4) == 0 && CountingMem::outstanding() == 1);           // usable afterwards
    }
    CASE_END();
    {   // a handle of several owners: released on success, dropped on failure at every allocation
        Handle *h = nullptr;
        CHECK(create(0, &h) == 0 && h != nullptr && h->n == 10 && CountingMem::outstanding() == 3);
        delete h;
        CASE_END();
        for (int nth = 1; nth <= 4; ++nth) {
            CHECK(create(nth, &h) == 2 && h == nullptr);
            CASE_END();
        }
    }
    {   // an exception between two allocations
        bool caught = false;
        try {
            throws_between(true);
        } catch (const std::runtime_error &) {
            caught = true;
        }
        CHECK(caught);
        CASE_END();
        throws_between(false);
        CASE_END();
    }
    std::printf("dev_buf_test ok (%d checks)\n", checks);
    return 0;
}
