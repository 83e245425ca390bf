// Windowed DFT of the overlapping segments of every row of a snapshot matrix, on the f64 matrix cores -- the step behind Welch
// spectra and spectral POD (sparsespatialsampling_amd/spectral.py).  gfx950 only.
//
// Reference behaviour: post_processing/compare_svd_OAT.py:56-70 passes every POD coefficient through scipy.signal.welch; here the
// same estimator runs per cell of a field [N, T], float32 or float64, read where it lies.
//
//     c[i, b, f] = sum_{l < L} (x[i, b hop + l] - mean[i]) (Bre[l, f] + i Bim[l, f])
//
// Bre / Bim [L, n_f] hold window, per-segment detrend and twiddles (built on the host: spectral.segment_matrix), so a segment's
// transform is a row of a tall product with k = L -- any L, no radix restriction -- and carries the GEMM's per-element error bound.
// A direct DFT, not an FFT: about 13 x the flops of a radix-2 transform at L = 256.
//
// Kernel: one 256-thread workgroup per (128 rows, 32 frequencies); it loops over the segments itself.  The k-loop over L is the one
// of centered_gemm_kernel at NJ = 2 (csrc/mfma_stage.h: the transposed L tile, the GLD pitch, the MFMA step; the raw loads of step
// s + 1 are issued before the MFMAs of step s) and runs on across the segment boundaries: the first tile of segment b + 1 is in
// flight while the last MFMAs of segment b issue.  The two 16-column tiles of a wavefront are the Re and the Im plane of the SAME 16
// frequencies, so a lane holds Re and Im of the same (row, frequency) in acc[i][0][r] and acc[i][1][r] and the power needs no
// cross-lane step.
//   MODE 0: coef[i][f][b][2] written at the end of every segment.
//   MODE 1: power += re^2 + im^2 in registers, segment after segment; psd[i][f] = scale[f] * power written once.  No atomics, no
//           partial results: two runs give the same bits.
// Columns l >= L of a segment's last step are valid samples of the next segment: they are masked in the loader (kk < k), not by a
// zero row of B.  Samples past the last segment are never addressed.
#include "mfma_stage.h"

namespace s3 {

constexpr int SF = 32;              // frequencies per workgroup: 16 per wavefront column, a Re and an Im tile each
constexpr int SLD = 2 * SF + 16;    // LDS row pitch of the B tile in doubles (64 columns; rows 128 B apart modulo 256 B, like GLD)

template <typename T, int VEC, int MODE>
__global__ void __launch_bounds__(256, 2)
segment_dft_kernel(const T *__restrict__ x, int64_t n_rows, int64_t in_stride, const double *__restrict__ mean, int nperseg, int64_t hop,
                   int n_blk, const double *__restrict__ bre, const double *__restrict__ bim, int n_f, const double *__restrict__ scale,
                   double *__restrict__ out) {
    __shared__ double sA[2][GK][GLD];
    __shared__ double sB[2][GK][SLD];
    const int64_t m0 = (int64_t)blockIdx.x * GB;
    const int f0 = blockIdx.y * SF;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = wave >> 1, wj = wave & 1;

    double4_t acc[4][2], power[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        acc[a][0] = acc[a][1] = double4_t{0.0, 0.0, 0.0, 0.0};
        power[a] = double4_t{0.0, 0.0, 0.0, 0.0};
    }

    // staging roles.  x: two threads per row of the block, eight consecutive samples each, written transposed (load_l_tile);
    // B: sixteen threads per row l of the step, two pieces of two columns.  Column c of the tile: wavefront column c >> 5,
    // plane (c >> 4) & 1 (0 Re, 1 Im), frequency f0 + 16 (c >> 5) + (c & 15)
    const int lrow = threadIdx.x >> 1, lk = (threadIdx.x & 1) * 8;
    const int64_t row_l = m0 + lrow;
    const bool row_ok = row_l < n_rows;
    const double mu = row_ok && mean ? mean[row_l] : 0.0;
    const T *xr = x + (row_ok ? row_l : 0) * in_stride;
    const int brow = threadIdx.x >> 4, c2 = (threadIdx.x & 15) * 2;
    const double *__restrict__ plane = (c2 & 16) ? bim : bre;
    const int fb = f0 + (c2 & 15);
    double ra[8], rb[2][2];
    auto load = [&](int seg, int k0) {
        load_l_tile<T, VEC>(xr + (int64_t)seg * hop, row_ok, k0 + lk, nperseg, mu, ra);
        const int kb = k0 + brow;
        const double *br = plane + (int64_t)(kb < nperseg ? kb : 0) * n_f;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int f = fb + 16 * p;
            rb[p][0] = kb < nperseg && f < n_f ? br[f] : 0.0;
            rb[p][1] = kb < nperseg && f + 1 < n_f ? br[f + 1] : 0.0;
        }
    };
    auto store = [&](int buf) {
        store_l_tile(sA[buf], lk, lrow, ra);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            sB[buf][brow][c2 + 32 * p] = rb[p][0];
            sB[buf][brow][c2 + 32 * p + 1] = rb[p][1];
        }
    };

    // C/D layout of v_mfma_f64_16x16x4_f64: column = lane & 15 (frequency), row = (lane >> 4) + 4 * register (row of x)
    const int gf = f0 + wj * 16 + (lane & 15);
    const int64_t gr0 = m0 + wi * 64 + (lane >> 4);

    int buf = 0;
    load(0, 0);
    store(0);
    __syncthreads();
    for (int seg = 0; seg < n_blk; ++seg) {
        for (int k0 = 0; k0 < nperseg; k0 += GK) {
            const bool last_k = k0 + GK >= nperseg;
            const bool more = !last_k || seg + 1 < n_blk;
            if (more) load(last_k ? seg + 1 : seg, last_k ? 0 : k0 + GK);
            mfma_step<2, SLD>(sA[buf], sB[buf], wi, wj, lane, acc);
            if (more) store(buf ^ 1);
            __syncthreads();
            buf ^= 1;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double re = acc[i][0][r], im = acc[i][1][r];
                if constexpr (MODE == 0) {
                    const int64_t gr = gr0 + i * 16 + 4 * r;
                    if (gr < n_rows && gf < n_f) {
                        double *o = out + ((gr * n_f + gf) * n_blk + seg) * 2;
                        o[0] = re;
                        o[1] = im;
                    }
                } else {
                    power[i][r] += re * re + im * im;
                }
            }
            acc[i][0] = acc[i][1] = double4_t{0.0, 0.0, 0.0, 0.0};
        }
    }

    if constexpr (MODE == 1) {
        const double sc = gf < n_f ? scale[gf] : 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t gr = gr0 + i * 16 + 4 * r;
                if (gr < n_rows && gf < n_f) out[gr * n_f + gf] = sc * power[i][r];
            }
    }
}

template <typename T, int VEC>
static void launch_segments(const T *d_x, int64_t n_rows, int64_t in_stride, const double *d_mean, int nperseg, int64_t hop, int n_blk,
                            const double *d_bre, const double *d_bim, int n_f, const double *d_scale, double *d_out, hipStream_t st) {
    const dim3 grid((unsigned)((n_rows + GB - 1) / GB), (unsigned)((n_f + SF - 1) / SF));
    if (d_scale)
        segment_dft_kernel<T, VEC, 1><<<grid, 256, 0, st>>>(d_x, n_rows, in_stride, d_mean, nperseg, hop, n_blk, d_bre, d_bim, n_f, d_scale, d_out);
    else
        segment_dft_kernel<T, VEC, 0><<<grid, 256, 0, st>>>(d_x, n_rows, in_stride, d_mean, nperseg, hop, n_blk, d_bre, d_bim, n_f, nullptr, d_out);
}

// d_scale != NULL: MODE 1 (PSD), else MODE 0 (coefficients)
static int segments_run(const char *who, const void *d_x, int dtype, int64_t n_rows, int64_t t, int64_t in_stride, const double *d_mean,
                        int64_t nperseg, int64_t hop, int64_t n_blk, const double *d_bre, const double *d_bim, int64_t n_f,
                        const double *d_scale, double *d_out, s3_stream stream) {
    S3_REQUIRE(d_x && d_bre && d_bim && d_out, "%s: null array", who);
    S3_REQUIRE(dtype == S3_DTYPE_F32 || dtype == S3_DTYPE_F64, "%s: dtype %d is neither f32 nor f64", who, dtype);
    S3_REQUIRE(n_rows >= 1 && nperseg >= 1 && nperseg < (1 << 24) && n_f >= 1 && n_f < (1 << 24) && hop >= 1 && n_blk >= 1 &&
                   n_blk < (1 << 24) && hop < ((int64_t)1 << 38) && t <= in_stride && (n_blk - 1) * hop + nperseg <= t,
               "%s: bad sizes (rows %lld, t %lld, stride %lld, nperseg %lld, hop %lld, segments %lld, frequencies %lld)", who, (long long)n_rows,
               (long long)t, (long long)in_stride, (long long)nperseg, (long long)hop, (long long)n_blk, (long long)n_f);
    const int64_t gx = (n_rows + GB - 1) / GB, gy = (n_f + SF - 1) / SF;
    S3_REQUIRE(gx < ((int64_t)1 << 31) && gy <= 65535, "%s: shape too large for one launch", who);
    hipStream_t st = as_stream(stream);
    // a segment starts b * hop elements into its row: an odd hop breaks the 16-byte alignment even where the rows are aligned
    const int width = row_width<StagedRowWidths>(dtype, d_x, in_stride, n_blk > 1 ? hop : 0);
    dispatch_rows<StagedRowWidths>(dtype, width, [&](auto row) {
        using T = typename decltype(row)::type;
        launch_segments<T, decltype(row)::vec>(static_cast<const T *>(d_x), n_rows, in_stride, d_mean, (int)nperseg, hop, (int)n_blk, d_bre, d_bim,
                                               (int)n_f, d_scale, d_out, st);
    });
    S3_LAUNCH_CHECK();
    return S3_OK;
}

}  // namespace s3

using namespace s3;

extern "C" {

int s3_segment_dft(const void *d_x, int dtype, int64_t n_rows, int64_t t, int64_t in_stride, const double *d_mean, int64_t nperseg,
                   int64_t hop, int64_t n_blk, const double *d_bre, const double *d_bim, int64_t n_f, double *d_coef, s3_stream stream) {
    return segments_run("s3_segment_dft", d_x, dtype, n_rows, t, in_stride, d_mean, nperseg, hop, n_blk, d_bre, d_bim, n_f, nullptr, d_coef, stream);
}

int s3_segment_psd(const void *d_x, int dtype, int64_t n_rows, int64_t t, int64_t in_stride, const double *d_mean, int64_t nperseg,
                   int64_t hop, int64_t n_blk, const double *d_bre, const double *d_bim, int64_t n_f, const double *d_scale, double *d_psd,
                   s3_stream stream) {
    S3_REQUIRE(d_scale, "s3_segment_psd: null array");
    return segments_run("s3_segment_psd", d_x, dtype, n_rows, t, in_stride, d_mean, nperseg, hop, n_blk, d_bre, d_bim, n_f, d_scale, d_psd, stream);
}

}  // extern "C"
