// Shared host/device helpers of libs3hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "dev_buf.h"
#include "s3hip.h"
#include "topo_core.h"

namespace s3 {

void set_error(const char *fmt, ...);

// device memory of DevBuf (csrc/dev_buf.h): the runtime's allocator as it is, no pool, no stream order
struct HipMem {
    static int alloc(void **p, size_t bytes) { return (int)hipMalloc(p, bytes); }
    static void free(void *p) { (void)hipFree(p); }
};

// (the cast: DevBuf::alloc hands the allocator's status on as an int)
#define S3_HIP_CHECK(expr)                                                                       \
    do {                                                                                         \
        const hipError_t _e = static_cast<hipError_t>(expr);                                     \
        if (_e != hipSuccess) {                                                                  \
            s3::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return _e == hipErrorNoDevice || _e == hipErrorInvalidDevice ? S3_ENODEV : S3_EHIP;  \
        }                                                                                        \
    } while (0)

// for the sites that tell the caller when the device is out of memory (construction of an index, a plan, an engine)
#define S3_HIP_CHECK_MEM(expr)                                                                   \
    do {                                                                                         \
        const hipError_t _e = static_cast<hipError_t>(expr);                                     \
        if (_e != hipSuccess) {                                                                  \
            s3::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return _e == hipErrorOutOfMemory ? S3_ENOMEM : S3_EHIP;                              \
        }                                                                                        \
    } while (0)

#define S3_REQUIRE(cond, ...)              \
    do {                                   \
        if (!(cond)) {                     \
            s3::set_error(__VA_ARGS__);    \
            return S3_EINVAL;              \
        }                                  \
    } while (0)

#define S3_LAUNCH_CHECK() S3_HIP_CHECK(hipGetLastError())

inline hipStream_t as_stream(s3_stream s) { return reinterpret_cast<hipStream_t>(s); }

inline unsigned grid_for(int64_t n, int block, int64_t cap = (int64_t)1 << 30) {
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// child / node direction table of the reference: the one of the topology core (csrc/topo_core.h)
__device__ __forceinline__ double dir_comp(int /*dim*/, int c, int j) { return s3topo::dir_comp(c, j); }

// (factor*width)/2^level exactly as torch evaluates it at s_cube.py:441 (all operations are exact scalings)
__device__ __forceinline__ double cell_offset(double factor_width, int level) {
    return factor_width / (double)(1ull << level);
}

}  // namespace s3
