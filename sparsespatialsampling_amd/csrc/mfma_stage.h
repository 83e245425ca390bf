// Operand staging of the f64 matrix-core kernels (v_mfma_f64_16x16x4_f64), shared by csrc/svd.hip (Gram matrix, tall GEMMs) and
// csrc/spectral.hip (segment DFT): tile constants, the 16-byte pieces of a panel (their vector type and the host's choice
// of its width come from csrc/typed_rows.h), the transposed L tile of a tall product and the MFMA step of a wavefront over one LDS buffer.  gfx950 only.
#ifndef S3_MFMA_STAGE_H
#define S3_MFMA_STAGE_H

#include "typed_rows.h"

namespace s3 {

constexpr int GB = 128;            // block edge of G / rows of a tall product per workgroup
constexpr int GK = 16;             // rows of the data matrix (Gram) or columns of L (tall product) per step
constexpr int GLD = GB + 16;       // LDS row pitch in doubles: consecutive rows start 128 B apart modulo 256 B (no bank conflicts
                                   // between the four 16-lane groups of a ds_read_b64)

typedef double double4_t __attribute__((ext_vector_type(4)));

// Operand staging by element type.  T = double is the matrix the interpolation kernel wrote (compute_svd); T = float is a field
// read where it lies (the DMD of the original CFD field and of a float32 Dataloader: dmd.py) -- widened to f64 in registers,
// BEFORE centring and weighting, so the staged value is the one the f64 staging makes of the matrix's .double() copy and the
// two Gram matrices agree to the bit.  A 16-byte piece is PW = 2 doubles or 4 floats: 16 threads per row of a 16 x 128 panel take
// 4 pieces at columns c0 + 32 p (double) or 2 pieces at c0 + 64 p (float), eight values per thread and panel either way.
// VEC = elements per load instruction of a piece that lies inside the matrix: chosen per LAUNCH on the host from the alignment
// every row start shares (row_width<StagedRowWidths>: the base, the row pitch and, for the segments of spectral.hip, which start a
// multiple of the hop into a row, the hop), never per lane; a piece across the matrix's edge is read element by element.
// (T = double keeps the scalar form it always had: VEC = 1.)
template <typename T> struct stage_traits;
template <> struct stage_traits<double> { static constexpr int PW = 2; };
template <> struct stage_traits<float> { static constexpr int PW = 4; };

// out[j] = p[j] widened for j < avail, `fill` for the others (avail <= 0: nothing is read)
template <typename T, int VEC, int PW>
__device__ __forceinline__ void load_piece(const T *__restrict__ p, int avail, double fill, double (&out)[PW]) {
    if constexpr (VEC > 1) {
        if (avail >= PW) {
#pragma unroll
            for (int q = 0; q < PW; q += VEC) {
                const RowVecNative<T, VEC> v = *reinterpret_cast<const RowVecNative<T, VEC> *>(p + q);
#pragma unroll
                for (int j = 0; j < VEC; ++j) out[q + j] = (double)v[j];
            }
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < PW; ++j) out[j] = j < avail ? (double)p[j] : fill;
}

// L tile of a tall product, the role of thread (lrow = tid >> 1, lk = (tid & 1) * 8): ra[i] = lr[kk0 + i] - mu for the eight
// consecutive columns kk0 + i < k of one row (64 contiguous bytes of a double row), 0 for rows / columns past the matrix
template <typename T, int VEC>
__device__ __forceinline__ void load_l_tile(const T *__restrict__ lr, bool row_ok, int kk0, int k, double mu, double (&ra)[8]) {
    if constexpr (sizeof(T) == 8) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int kk = kk0 + i;
            ra[i] = row_ok && kk < k ? lr[kk] - mu : 0.0;      // rows / columns past the matrix contribute nothing
        }
    } else {                                                   // float: two 16-byte pieces of four columns, widened, then centred
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int kk = kk0 + 4 * h;
            double piece[4];
            load_piece<T, VEC, 4>(lr + kk, row_ok ? k - kk : 0, mu, piece);
#pragma unroll
            for (int j = 0; j < 4; ++j) ra[4 * h + j] = piece[j] - mu;   // (mu - mu = 0 past the matrix)
        }
    }
}

// ... written transposed: sA[k][row], so that both MFMA operands are read the same way
__device__ __forceinline__ void store_l_tile(double (*sa)[GLD], int lk, int lrow, const double (&ra)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) sa[lk + i][lrow] = ra[i];
}

// the MFMAs of one step of GK: wavefront (wi, wj) adds its 4 x NJ tiles, rows wi * 64 + 16 i of pa and columns wj * 16 NJ + 16 j of pb
// (LDS row pitches GLD and LDB doubles)
template <int NJ, int LDB>
__device__ __forceinline__ void mfma_step(const double (*pa)[GLD], const double (*pb)[LDB], int wi, int wj, int lane, double4_t (&acc)[4][NJ]) {
#pragma unroll
    for (int k4 = 0; k4 < GK / 4; ++k4) {
        const int kr = k4 * 4 + (lane >> 4), cl = lane & 15;
        double a[4], bb[NJ];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = pa[kr][wi * 64 + i * 16 + cl];
#pragma unroll
        for (int j = 0; j < NJ; ++j) bb[j] = pb[kr][wj * (16 * NJ) + j * 16 + cl];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], bb[j], acc[i][j], 0, 0, 0);
    }
}

}  // namespace s3

#endif
