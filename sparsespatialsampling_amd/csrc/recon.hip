// Reconstruction error of a generated grid: the exported fields interpolated BACK onto the points of the original CFD mesh and
// compared with the original fields there, fused into one launch per snapshot batch.  gfx950 only.
//
// Reference behaviour restated here: post_processing/compute_error_OAT.py:208-233
//     fitted = KNeighborsRegressor(k, weights="distance").fit(centres, grid_fields).predict(points)      [N, T] on the host
//     d      = s * (fitted - orig),  ref = s * orig                                   (s = sqrt of the original cell area)
//     ||d[:, t]|| / ||ref[:, t]||,  ||d|| / ||ref||,  mean_t |d|,  std_t |d|
// The fitted field ([N, T] f64: 40 GB for the 3-D cylinder) is never written: every value lives in a register between the
// gather and the reductions.
//
// Regime: the reverse of csrc/export.hip.  The table that is gathered from (the grid, Nc rows) is small and stays in L2 /
// Infinity Cache; the targets (N points) are many and stream: per point 12*k bytes of weights / ids and one original row.
//
// Work split: the point slots of csrc/point_slots.h.  A workgroup owns one REDUCTION BLOCK of S3_RECON_BLOCK consecutive points
// of the launch order; the staged tables are the weights and ids (12*k bytes per point and chunk; one chunk up to 256 fp32 /
// 128 f64 columns).  A lane's columns are fixed while it walks its points, so the column sums stay in registers.
//
// Order of every floating-point sum (no atomics: same inputs, same bits):
//   fitted value      f64 fma chain over the neighbours 0..k-1 (independent of row_len, VEC and LP)
//   per-point moments chunk sum -> chunk mean -> squared deviations from the values still in registers (xor butterflies over
//                     the LP lanes), chunks merged with Chan's update: the scheme of row_moments_kernel (csrc/metric.hip)
//   column sums       a lane adds its points in ascending order, the slots are added in ascending order, the blocks by
//                     recon_reduce_kernel: 16 contiguous runs of blocks, each in ascending order, then the runs in order
#include "point_slots.h"
#include "typed_rows.h"

#include <cmath>

namespace s3 {

namespace {

constexpr int RECON_THREADS = POINT_THREADS;
constexpr int RECON_RUNS = 16;          // runs of blocks in the second pass
constexpr int RECON_RCOLS = 16;         // columns per workgroup of the second pass

__device__ __forceinline__ double slot_sum(double v, int lp) {
    for (int off = lp >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off);     // xor butterfly inside the aligned group of lp lanes
    return v;
}

// scikit-learn's weights="distance" as KNeighborsRegressor.predict uses them (sklearn/neighbors/_base.py, _get_weights, and the
// division by the weights' sum in _regression.py): a row with zero distances gets the indicator of the zeros, any other row
// 1/dist; either way normalised to sum 1.  The sum is compensated (Kahan): the weights are the correctly rounded quotients of
// 1/dist and its exact sum to 2 ulp, whatever k.
__global__ void idw_weights_exact_kernel(const double *__restrict__ dist, int64_t n, int k, double *__restrict__ w) {
    const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (c >= n) return;
    const double *d = dist + c * k;
    int zeros = 0;
    double s = 0.0, comp = 0.0;
    for (int m = 0; m < k; ++m) {
        const double v = d[m];
        if (v == 0.0) ++zeros;
        const double y = 1.0 / v - comp, t = s + y;
        comp = (t - s) - y;
        s = t;
    }
    if (zeros) {
        const double hit = 1.0 / (double)zeros;
        for (int m = 0; m < k; ++m) w[c * k + m] = d[m] == 0.0 ? hit : 0.0;
    } else {
        for (int m = 0; m < k; ++m) w[c * k + m] = (1.0 / d[m]) / s;
    }
}

template <typename TG, typename TO, int VEC>
__global__ void __launch_bounds__(RECON_THREADS)
recon_kernel(const double *__restrict__ w, const int32_t *__restrict__ idx, int64_t n, int k, const TG *__restrict__ grid,
             int64_t row_len, const TO *__restrict__ orig, int64_t orig_stride, const int32_t *__restrict__ rows,
             const double *__restrict__ scale, double *__restrict__ mean_out, double *__restrict__ m2_out,
             double *__restrict__ partial, int lp, int stage_pts, int n_chunks, int64_t n_blocks, int64_t blocks_per_xcd) {
    extern __shared__ double lds[];
    const int pg = RECON_THREADS / lp;                                          // point slots = points per pass (divides stage_pts)
    double *s_red = lds;                                                        // [2*VEC][256] column sums of the slots
    double *s_mom = s_red + 2 * VEC * RECON_THREADS;                            // [S3_RECON_BLOCK][2] (rows of several chunks only)
    double *s_w = s_mom + (n_chunks > 1 ? 2 * S3_RECON_BLOCK : 0);              // [stage_pts*k]
    int32_t *s_idx = reinterpret_cast<int32_t *>(s_w + (size_t)stage_pts * k);  // [stage_pts*k]

    const int64_t blk = xcd_block(blockIdx.x, blocks_per_xcd);
    if (blk >= n_blocks) return;
    const int64_t p0 = blk * S3_RECON_BLOCK;
    const int n_p = (int)min((int64_t)S3_RECON_BLOCK, n - p0);
    const int t = threadIdx.x, lane = t & (lp - 1), slot = t / lp;

    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        const int64_t chunk0 = (int64_t)chunk * lp * VEC;
        const int64_t col0 = chunk0 + (int64_t)lane * VEC;
        const bool col_ok = col0 < row_len;                                     // VEC divides row_len: a piece is inside or outside
        const double n_chunk = (double)min((int64_t)lp * VEC, row_len - chunk0);
        double cs_d[VEC], cs_r[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) cs_d[i] = cs_r[i] = 0.0;

        for (int sb = 0; sb < n_p; sb += stage_pts) {
          // the tables of stage_pts points at a time (one barrier pair per stage, several passes of the slots per stage)
          const int n_st = min(stage_pts, n_p - sb);
          __syncthreads();                                                      // the previous stage's tables have been read
          const int n_stage = n_st * k;
          const int64_t g0 = (p0 + sb) * k;
          for (int i = t; i < n_stage; i += RECON_THREADS) {
              s_w[i] = w[g0 + i];
              s_idx[i] = idx[g0 + i];
          }
          __syncthreads();
          for (int pb = sb; pb < sb + n_st; pb += pg) {
            const int n_in = min(pg, sb + n_st - pb);
            const bool live = slot < n_in;                                      // dead slots and columns still take part in the shuffles
            const bool act = live && col_ok;
            const int64_t p = p0 + pb + (live ? slot : 0);
            const int64_t orow = rows ? (int64_t)rows[p] : p;
            double x[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) x[i] = 0.0;
            if (act) {
                const double *wp = s_w + (pb - sb + slot) * k;
                const int32_t *ip = s_idx + (pb - sb + slot) * k;
                const TG *col = grid + col0;
                double acc[VEC];
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[i] = 0.0;
                int m = 0;
                // eight independent row reads in flight per lane before the first FMA, as in interp_kernel
                for (; m + 8 <= k; m += 8) {
                    double v[8][VEC];
#pragma unroll
                    for (int u = 0; u < 8; ++u) row_load_wide<TG, VEC>(col + (int64_t)ip[m + u] * row_len, v[u]);
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const double wu = wp[m + u];
#pragma unroll
                        for (int i = 0; i < VEC; ++i) acc[i] = fma(wu, v[u][i], acc[i]);
                    }
                }
                for (; m + 2 <= k; m += 2) {
                    double v0[VEC], v1[VEC];
                    row_load_wide<TG, VEC>(col + (int64_t)ip[m] * row_len, v0);
                    row_load_wide<TG, VEC>(col + (int64_t)ip[m + 1] * row_len, v1);
                    const double w0 = wp[m], w1 = wp[m + 1];
#pragma unroll
                    for (int i = 0; i < VEC; ++i) acc[i] = fma(w1, v1[i], fma(w0, v0[i], acc[i]));
                }
                for (; m < k; ++m) {
                    double v0[VEC];
                    row_load_wide<TG, VEC>(col + (int64_t)ip[m] * row_len, v0);
                    const double w0 = wp[m];
#pragma unroll
                    for (int i = 0; i < VEC; ++i) acc[i] = fma(w0, v0[i], acc[i]);
                }
                // the original row may start anywhere (orig_stride is arbitrary): element loads
                const TO *op = orig + orow * orig_stride + col0;
                const double s = scale ? scale[p] : 1.0;
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    const double o = (double)op[i];
                    const double d = s * (acc[i] - o), r = s * o;
                    cs_d[i] = fma(d, d, cs_d[i]);
                    cs_r[i] = fma(r, r, cs_r[i]);
                    x[i] = fabs(d);
                }
            }
            double sum = 0.0;
#pragma unroll
            for (int i = 0; i < VEC; ++i) sum += x[i];
            const double mc = slot_sum(sum, lp) / n_chunk;
            double q = 0.0;
            if (act) {
#pragma unroll
                for (int i = 0; i < VEC; ++i) q += (x[i] - mc) * (x[i] - mc);
            }
            q = slot_sum(q, lp);
            if (live && lane == 0) {
                double mean = mc, m2 = q;
                if (chunk > 0) {                                                // Chan's update with the chunks before this one
                    const double na = (double)chunk0, nn = na + n_chunk;
                    const double ma = s_mom[2 * (pb + slot)], qa = s_mom[2 * (pb + slot) + 1];
                    const double delta = mc - ma;
                    mean = ma + delta * (n_chunk / nn);
                    m2 = qa + q + delta * delta * (na * n_chunk / nn);
                }
                if (chunk + 1 < n_chunks) {
                    s_mom[2 * (pb + slot)] = mean;
                    s_mom[2 * (pb + slot) + 1] = m2;
                } else {
                    mean_out[orow] = mean;
                    m2_out[orow] = m2;
                }
            }
          }
        }

        // column sums of this chunk: the slots in ascending order
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            s_red[i * RECON_THREADS + t] = cs_d[i];
            s_red[(VEC + i) * RECON_THREADS + t] = cs_r[i];
        }
        __syncthreads();
        if (t < lp && col_ok) {
            double *out_d = partial + blk * 2 * row_len + col0, *out_r = out_d + row_len;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                double a = 0.0, r = 0.0;
                for (int s = 0; s < pg; ++s) {
                    a += s_red[i * RECON_THREADS + s * lp + t];
                    r += s_red[(VEC + i) * RECON_THREADS + s * lp + t];
                }
                out_d[i] = a;
                out_r[i] = r;
            }
        }
    }
}

// partial[n_blocks][n_cols] -> out[n_cols]: RECON_RUNS contiguous runs of blocks, each added in ascending block order by one
// thread (eight loads in flight), then the runs in ascending order
__global__ void __launch_bounds__(RECON_THREADS)
recon_reduce_kernel(const double *__restrict__ partial, int64_t n_blocks, int64_t n_cols, double *__restrict__ out) {
    __shared__ double s_run[RECON_RUNS][RECON_RCOLS];
    const int tx = threadIdx.x % RECON_RCOLS, run = threadIdx.x / RECON_RCOLS;
    const int64_t col = (int64_t)blockIdx.x * RECON_RCOLS + tx;
    const int64_t per_run = (n_blocks + RECON_RUNS - 1) / RECON_RUNS;
    const int64_t b0 = min(n_blocks, run * per_run), b1 = min(n_blocks, b0 + per_run);
    double acc = 0.0;
    if (col < n_cols) {
        const double *p = partial + col;
        int64_t bl = b0;
        for (; bl + 8 <= b1; bl += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[(bl + u) * n_cols];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += v[u];
        }
        for (; bl < b1; ++bl) acc += p[bl * n_cols];
    }
    s_run[run][tx] = acc;
    __syncthreads();
    if (run == 0 && col < n_cols) {
        double total = 0.0;
        for (int r = 0; r < RECON_RUNS; ++r) total += s_run[r][tx];
        out[col] = total;
    }
}

int64_t recon_blocks(int64_t n) { return (n + S3_RECON_BLOCK - 1) / S3_RECON_BLOCK; }

template <typename TG, typename TO, int VEC>
int launch_recon(const double *w, const int32_t *idx, int64_t n, int k, const void *grid, int64_t row_len, const void *orig,
                 int64_t orig_stride, const int32_t *rows, const double *scale, double *mean, double *m2, double *colsum,
                 double *partial, hipStream_t st) {
    // LDS (slot_shape, csrc/point_slots.h): the column scratch, the moments of rows of several chunks, and per point of a stage its
    // weights and ids (64 points: 19.5 KB at k = 26)
    const size_t scratch = sizeof(double) * 2 * VEC * RECON_THREADS, moments = sizeof(double) * 2 * S3_RECON_BLOCK;
    SlotShape shape;
    if (const int rc = slot_shape("s3_recon_error", row_len, row_len / VEC, (size_t)k * (sizeof(double) + sizeof(int32_t)), scratch,
                                  scratch + moments, shape))
        return rc;
    const int64_t n_blocks = recon_blocks(n);
    const XcdGrid xcd = xcd_grid(n_blocks);
    S3_REQUIRE(xcd.fits(), "s3_recon_error: too many points");
    recon_kernel<TG, TO, VEC><<<(unsigned)xcd.grid, RECON_THREADS, shape.lds_bytes, st>>>(
        w, idx, n, k, static_cast<const TG *>(grid), row_len, static_cast<const TO *>(orig), orig_stride, rows, scale, mean, m2,
        partial, shape.lanes, shape.stage_pts, (int)shape.n_chunks, n_blocks, xcd.per_xcd);
    S3_LAUNCH_CHECK();
    const int64_t n_cols = 2 * row_len;
    recon_reduce_kernel<<<(unsigned)((n_cols + RECON_RCOLS - 1) / RECON_RCOLS), RECON_THREADS, 0, st>>>(partial, n_blocks, n_cols,
                                                                                                       colsum);
    S3_LAUNCH_CHECK();
    return S3_OK;
}

}  // namespace

}  // namespace s3

using namespace s3;

extern "C" {

int s3_idw_weights_exact(const double *d_dist, int64_t n, int k, double *d_w, s3_stream stream) {
    S3_REQUIRE(n >= 0 && k >= 1 && k <= S3_MAX_K, "s3_idw_weights_exact: bad shape n=%lld k=%d", (long long)n, k);
    S3_REQUIRE(n == 0 || (d_dist && d_w), "s3_idw_weights_exact: null array");
    if (n == 0) return S3_OK;
    idw_weights_exact_kernel<<<grid_for(n, 256), 256, 0, as_stream(stream)>>>(d_dist, n, k, d_w);
    S3_LAUNCH_CHECK();
    return S3_OK;
}

size_t s3_recon_error_scratch_bytes(int64_t n, int64_t row_len) {
    if (n < 1 || row_len < 1) return 0;
    return sizeof(double) * 2 * (size_t)row_len * (size_t)recon_blocks(n);
}

int s3_recon_error(const double *d_w, const int32_t *d_idx, int64_t n, int k, const void *d_grid, int grid_dtype, int64_t nc,
                   const void *d_orig, int orig_dtype, int64_t n_orig, int64_t orig_stride, int64_t row_len,
                   const int32_t *d_rows, const double *d_scale, double *d_mean, double *d_m2, double *d_colsum, void *d_scratch,
                   s3_stream stream) {
    S3_REQUIRE(n >= 0 && row_len >= 1 && nc >= 1 && n_orig >= n, "s3_recon_error: bad shape n=%lld row_len=%lld nc=%lld n_orig=%lld",
               (long long)n, (long long)row_len, (long long)nc, (long long)n_orig);
    S3_REQUIRE(k >= 1 && k <= S3_MAX_K, "s3_recon_error: k=%d outside [1,%d]", k, S3_MAX_K);
    S3_REQUIRE((grid_dtype == S3_DTYPE_F32 || grid_dtype == S3_DTYPE_F64) && (orig_dtype == S3_DTYPE_F32 || orig_dtype == S3_DTYPE_F64),
               "s3_recon_error: unknown dtype %d / %d", grid_dtype, orig_dtype);
    S3_REQUIRE(nc < ((int64_t)1 << 31) && n_orig < ((int64_t)1 << 31), "s3_recon_error: row ids must fit int32");
    S3_REQUIRE(d_rows != nullptr || n_orig == n, "s3_recon_error: without a row list every original row is a point");
    if (orig_stride <= 0) orig_stride = row_len;
    S3_REQUIRE(orig_stride >= row_len, "s3_recon_error: orig_stride %lld < row_len %lld", (long long)orig_stride, (long long)row_len);
    S3_REQUIRE(d_colsum != nullptr, "s3_recon_error: null array");
    hipStream_t st = as_stream(stream);
    if (n == 0) {
        S3_HIP_CHECK(hipMemsetAsync(d_colsum, 0, sizeof(double) * 2 * (size_t)row_len, st));
        return S3_OK;
    }
    S3_REQUIRE(d_w && d_idx && d_grid && d_orig && d_mean && d_m2 && d_scratch, "s3_recon_error: null array");
    double *partial = static_cast<double *>(d_scratch);
    // the width of a lane's piece follows the GRID rows (k reads per element; the original row is read once, by elements)
    return dispatch_rows<WidestRowWidth>(grid_dtype, row_width<WidestRowWidth>(grid_dtype, d_grid, row_len), [&](auto g) {
        return dispatch_rows<ScalarRows>(orig_dtype, 1, [&](auto o) {
            return launch_recon<typename decltype(g)::type, typename decltype(o)::type, decltype(g)::vec>(
                d_w, d_idx, n, k, d_grid, row_len, d_orig, orig_stride, d_rows, d_scale, d_mean, d_m2, d_colsum, partial, st);
        });
    });
}

}  // extern "C"
