// Rows of float32 or float64 read where they lie, VEC elements per load instruction: the vector type of (T, VEC), the loads, the host
// rule that picks VEC for a launch and the step from (dtype, VEC) at run time to <T, VEC> at compile time.  Shared by every kernel
// family that takes a `dtype` argument (metric.hip, export.hip, recon.hip, differential.hip, sample.hip, iso.hip, regions.hip, and through mfma_stage.h
// svd.hip and spectral.hip).  gfx950 only.
//
// VEC is chosen per LAUNCH, never per lane: every vector address of a launch is the base address plus multiples of a few byte
// quantities (the row pitch; the row length where VEC-wide pieces tile a row or where component rows follow one another; the hop of
// the segments of spectral.hip), so the alignment all of them share is the one of the OR of those quantities (row_width).  What each
// entry point instantiates, and the condition that selects it (lengths in elements, addresses in bytes):
//
//   entry                                  float32                                         float64
//   s3_row_moments, s3_row_abs_moments     4: stride%4, base%16; 2: stride%2, base%8;      2: stride%2, base%16; else 1
//                                          else 1
//   s3_interp                              4: row_len%4, in%16, out%16; 2: row_len%2,      2: row_len%2, in%16, out%16; else 1
//                                          in%8, out%16; else 1
//   s3_recon_error (width follows the      4: row_len%4, grid%16; else 1                   2: row_len%2, grid%16; else 1
//   grid; x orig f32 / f64)
//   s3_grad_apply, s3_cell_sample,         4: row_len%4, stride%4, base%16; else 1         2: row_len%2, stride%2, base%16; else 1
//   s3_iso_count, s3_iso_emit
//   s3_gram, s3_weighted_gram,             4 / 2 / 1 by base | stride*4 [| hop*4]          always 1
//   s3_tall_gemm and the centred GEMMs,
//   s3_segment_dft / s3_segment_psd
//   s3_region_label (the accesses next to      always 1                                        always 1
//   the loads are per-element atomics)
#ifndef S3_TYPED_ROWS_H
#define S3_TYPED_ROWS_H

#include "common.h"

namespace s3 {

template <typename T, int VEC> struct RowVec;
template <> struct RowVec<float, 4> { using type = float4; };
template <> struct RowVec<float, 2> { using type = float2; };
template <> struct RowVec<float, 1> { using type = float; };
template <> struct RowVec<double, 2> { using type = double2; };
template <> struct RowVec<double, 1> { using type = double; };
// (the same bytes as a clang vector, which indexes: the form load_piece of mfma_stage.h has always loaded; through HIP's structs the
// matrix-core kernels come out with other instruction streams)
template <typename T, int VEC> using RowVecNative = T __attribute__((ext_vector_type(VEC)));

// one load of VEC elements, kept as it came (a kernel with many loads in flight widens at use: differential.hip) ...
template <typename T, int VEC>
__device__ __forceinline__ typename RowVec<T, VEC>::type row_load(const T *__restrict__ p) {
    return *reinterpret_cast<const typename RowVec<T, VEC>::type *>(p);
}

// ... element i of it as a double ...
template <typename T, int VEC>
__device__ __forceinline__ double row_elem(const typename RowVec<T, VEC>::type &raw, int i) {
    return (double)reinterpret_cast<const T *>(&raw)[i];
}

// ... or both at once: v[i] = (double)p[i]
template <typename T, int VEC>
__device__ __forceinline__ void row_load_wide(const T *__restrict__ p, double (&v)[VEC]) {
    const typename RowVec<T, VEC>::type raw = row_load<T, VEC>(p);
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = row_elem<T, VEC>(raw, i);
}

// VEC doubles, 16 bytes per store
template <int VEC>
__device__ __forceinline__ void row_store(double *__restrict__ p, const double (&a)[VEC]) {
    if constexpr (VEC == 4) {
        *reinterpret_cast<double2 *>(p) = make_double2(a[0], a[1]);
        *reinterpret_cast<double2 *>(p + 2) = make_double2(a[2], a[3]);
    } else if constexpr (VEC == 2) {
        *reinterpret_cast<double2 *>(p) = make_double2(a[0], a[1]);
    } else {
        p[0] = a[0];
    }
}

// The widths a family instantiates per element type, as the OR of them (1 is always among them): a family declares this once.
template <int F32, int F64> struct RowWidths { static constexpr int f32 = F32, f64 = F64; };
using EveryRowWidth = RowWidths<4 | 2 | 1, 2 | 1>;      // s3_row_moments, s3_interp
using WidestRowWidth = RowWidths<4 | 1, 2 | 1>;         // s3_recon_error, s3_grad_apply, s3_cell_sample, s3_iso_*: 16-byte loads or element loads
using StagedRowWidths = RowWidths<4 | 2 | 1, 1>;        // the f64 matrix-core kernels: float64 keeps the scalar form it always had
using ScalarRows = RowWidths<1, 1>;                     // the element type alone (s3_region_label)

inline size_t dtype_bytes(int dtype) { return dtype == S3_DTYPE_F32 ? sizeof(float) : sizeof(double); }

// the widest width of the family W that divides everything the vector addresses of a launch are made of: the base address and, in
// elements, the row pitch and whatever else the kernel steps by
template <typename W, typename... Steps>
inline int row_width(int dtype, const void *base, Steps... step_elements) {
    const uintptr_t elem = dtype_bytes(dtype);
    const uintptr_t shared = (reinterpret_cast<uintptr_t>(base) | ... | ((uintptr_t)step_elements * elem));
    const int widths = dtype == S3_DTYPE_F32 ? W::f32 : W::f64;
    for (int vec = 4; vec > 1; vec >>= 1)
        if ((widths & vec) && shared % (vec * elem) == 0) return vec;
    return 1;
}

// f(RowTag<T, VEC>{}) for the element type and width of a launch; only the widths of W are instantiated
template <typename T, int VEC> struct RowTag {
    using type = T;
    static constexpr int vec = VEC;
};

template <typename W, typename F>
inline auto dispatch_rows(int dtype, int width, F &&f) {
    if (dtype == S3_DTYPE_F32) {
        if constexpr ((W::f32 & 4) != 0)
            if (width == 4) return f(RowTag<float, 4>{});
        if constexpr ((W::f32 & 2) != 0)
            if (width == 2) return f(RowTag<float, 2>{});
        return f(RowTag<float, 1>{});
    }
    if constexpr ((W::f64 & 2) != 0)
        if (width == 2) return f(RowTag<double, 2>{});
    return f(RowTag<double, 1>{});
}

}  // namespace s3

#endif
