// Spatial derivatives of fields that live on a point cloud (the S^3 cell centres or the points of the original CFD mesh):
// weighted least-squares gradients over the k nearest neighbours, and divergence, vorticity, Q and gradient magnitude formed from
// them in the same launch.  gfx950 only.  No counterpart in the reference, whose grid is a bare point cloud.
//
// Definition (include/s3hip.h restates it): for point i with neighbours idx[m], m < k (the point itself is not among them),
//     dx_m = x[idx_m] - x_i,  r_m = |dx_m|,  h = max_m r_m,  dxs_m = dx_m / h,  rs_m = r_m / h
//     w_m  = rs_m^-p (p = 0 | 1 | 2), 0 where r_m = 0             M = sum_m w_m dxs_m dxs_m^T = L L^T (Cholesky)
//     c[i, m, :] = w_m * M^-1 dxs_m / h                           d f / d x_a (i) = sum_m c[i, m, a] * (f[idx_m] - f[i])
// A row with h = 0 or a Cholesky pivot <= 2^-40 * trace(M) (collinear / coplanar neighbours) is DEGENERATE: its coefficients are
// all zero and its flag is set.
//
// s3_grad_coeff runs once per cloud (one thread per point, three passes over the point's neighbours, nothing kept between them
// but h, M and L).  s3_grad_apply is the hot path.
//
// Regime of the apply: per point k * (8 dim + 4) bytes of coefficients / ids stream, k neighbour rows of n_comp * T values are
// gathered from the field itself (the neighbours of consecutive points of the Hilbert launch order overlap: L2 / Infinity Cache),
// n_out * T f64 values are written.  The n_comp x dim gradient entries never leave the registers.
//
// Work split: the point slots of csrc/point_slots.h, as in recon_kernel (csrc/recon.hip) without its reductions.  A workgroup owns
// GRAD_BLOCK consecutive points of the launch order; lane l of a slot owns the columns [(chunk*LP + l)*VEC, +VEC) of EVERY component;
// the staged tables are the coefficients and ids.
//
// Order of every floating-point sum: an f64 fma chain over the neighbours m = 0..k-1 per (component, axis, column), independent
// of row_len, VEC, LP and n_comp; the derived quantities are formed from the finished chains in a fixed order.  No atomics on
// floating-point values: the same inputs give the same bits on every run.
#include "point_slots.h"
#include "typed_rows.h"

#include <cmath>

namespace s3 {

namespace {

constexpr int GRAD_THREADS = POINT_THREADS;
constexpr int GRAD_BLOCK = 256;         // points per workgroup
constexpr int GRAD_FLIGHT = 4;          // neighbour rows (all components) a lane has in flight before the first fma

// ---- coefficients ---------------------------------------------------------------------------------------------------------
template <int DIM>
__global__ void __launch_bounds__(256)
grad_coeff_kernel(const double *__restrict__ pts, int64_t n, const int32_t *__restrict__ idx, int k, int power,
                  const int32_t *__restrict__ rows, double *__restrict__ coef, uint8_t *__restrict__ flag,
                  unsigned long long *__restrict__ n_degenerate) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int64_t i = rows ? (int64_t)rows[j] : j;
    const int32_t *ip = idx + j * k;
    double *cp = coef + j * k * DIM;
    double x[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) x[a] = pts[i * DIM + a];

    double h = 0.0;
    for (int m = 0; m < k; ++m) {
        const double *q = pts + (int64_t)ip[m] * DIM;
        double r2 = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            const double d = q[a] - x[a];
            r2 += d * d;
        }
        h = fmax(h, sqrt(r2));
    }

    double M[DIM][DIM], L[DIM][DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
        for (int b = 0; b < DIM; ++b) M[a][b] = L[a][b] = 0.0;
    bool degenerate = !(h > 0.0);
    if (!degenerate) {
        for (int m = 0; m < k; ++m) {
            const double *q = pts + (int64_t)ip[m] * DIM;
            double d[DIM], r2 = 0.0;
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                const double dx = q[a] - x[a];
                r2 += dx * dx;
                d[a] = dx / h;
            }
            const double rs = sqrt(r2) / h;
            const double w = !(rs > 0.0) ? 0.0 : (power == 0 ? 1.0 : (power == 1 ? 1.0 / rs : 1.0 / (rs * rs)));
#pragma unroll
            for (int a = 0; a < DIM; ++a)
#pragma unroll
                for (int b = 0; b <= a; ++b) M[a][b] += w * d[a] * d[b];
        }
        double trace = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) trace += M[a][a];
        const double floor_pivot = 0x1p-40 * trace;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            if (degenerate) break;
            double s = M[a][a];
#pragma unroll
            for (int q = 0; q < a; ++q) s -= L[a][q] * L[a][q];
            if (!(s > floor_pivot)) {
                degenerate = true;
                break;
            }
            L[a][a] = sqrt(s);
#pragma unroll
            for (int b = a + 1; b < DIM; ++b) {
                double t = M[b][a];
#pragma unroll
                for (int q = 0; q < a; ++q) t -= L[b][q] * L[a][q];
                L[b][a] = t / L[a][a];
            }
        }
    }
    flag[j] = degenerate ? 1 : 0;
    if (degenerate) {
        for (int m = 0; m < k * DIM; ++m) cp[m] = 0.0;
        atomicAdd(n_degenerate, 1ull);
        return;
    }
    for (int m = 0; m < k; ++m) {
        const double *q = pts + (int64_t)ip[m] * DIM;
        double z[DIM], r2 = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            const double dx = q[a] - x[a];
            r2 += dx * dx;
            z[a] = dx / h;
        }
        const double rs = sqrt(r2) / h;
        const double w = !(rs > 0.0) ? 0.0 : (power == 0 ? 1.0 : (power == 1 ? 1.0 / rs : 1.0 / (rs * rs)));
        // L y = dxs, L^T z = y (in place)
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
#pragma unroll
            for (int q2 = 0; q2 < a; ++q2) z[a] -= L[a][q2] * z[q2];
            z[a] /= L[a][a];
        }
#pragma unroll
        for (int a = DIM - 1; a >= 0; --a) {
#pragma unroll
            for (int q2 = a + 1; q2 < DIM; ++q2) z[a] -= L[q2][a] * z[q2];
            z[a] /= L[a][a];
        }
#pragma unroll
        for (int a = 0; a < DIM; ++a) cp[m * DIM + a] = w * z[a] / h;
    }
}

// ---- apply ----------------------------------------------------------------------------------------------------------------
__host__ __device__ constexpr int grad_n_out(int mode, int dim, int n_comp) {
    return mode == S3_GRAD_GRADIENT ? n_comp * dim : mode == S3_GRAD_MAGNITUDE ? n_comp : mode == S3_GRAD_VORTICITY ? (dim == 2 ? 1 : 3) : 1;
}

// the requested quantity of one column from its finished gradient G[comp][axis]; o[] takes grad_n_out values
template <int DIM, int NCOMP, int MODE>
__device__ __forceinline__ void grad_finish(const double (&G)[NCOMP][DIM], double *o) {
    if constexpr (MODE == S3_GRAD_GRADIENT) {
#pragma unroll
        for (int c = 0; c < NCOMP; ++c)
#pragma unroll
            for (int a = 0; a < DIM; ++a) o[c * DIM + a] = G[c][a];
    } else if constexpr (MODE == S3_GRAD_MAGNITUDE) {
#pragma unroll
        for (int c = 0; c < NCOMP; ++c) {
            double s = G[c][0] * G[c][0];
#pragma unroll
            for (int a = 1; a < DIM; ++a) s = fma(G[c][a], G[c][a], s);
            o[c] = sqrt(s);
        }
    } else if constexpr (MODE == S3_GRAD_DIVERGENCE) {
        double s = G[0][0];
#pragma unroll
        for (int a = 1; a < DIM; ++a) s += G[a][a];
        o[0] = s;
    } else if constexpr (MODE == S3_GRAD_VORTICITY) {
        if constexpr (DIM == 2) {
            o[0] = G[1][0] - G[0][1];
        } else {
            o[0] = G[2][1] - G[1][2];
            o[1] = G[0][2] - G[2][0];
            o[2] = G[1][0] - G[0][1];
        }
    } else if constexpr (MODE == S3_GRAD_VORTICITY_MAGNITUDE) {
        if constexpr (DIM == 2) {
            o[0] = fabs(G[1][0] - G[0][1]);
        } else {
            const double a = G[2][1] - G[1][2], b = G[0][2] - G[2][0], c = G[1][0] - G[0][1];
            o[0] = sqrt(fma(c, c, fma(b, b, a * a)));
        }
    } else {                                                                    // Q = -1/2 sum_ab G_ab G_ba
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a)
#pragma unroll
            for (int b = 0; b < DIM; ++b) s = fma(G[a][b], G[b][a], s);
        o[0] = -0.5 * s;
    }
}

template <typename T, int VEC, int DIM, int NCOMP, int MODE>
__global__ void __launch_bounds__(GRAD_THREADS)
grad_apply_kernel(const double *__restrict__ coef, const int32_t *__restrict__ idx, int64_t n, int k, const T *__restrict__ field,
                  int64_t row_len, int64_t in_stride, const int32_t *__restrict__ rows, double *__restrict__ out, int64_t out_stride,
                  int lp, int stage_pts, int n_chunks, int64_t n_blocks, int64_t blocks_per_xcd) {
    using V = typename RowVec<T, VEC>::type;
    constexpr int NOUT = grad_n_out(MODE, DIM, NCOMP);
    extern __shared__ double lds[];
    double *s_c = lds;                                                                    // [stage_pts * k * DIM]
    int32_t *s_i = reinterpret_cast<int32_t *>(s_c + (size_t)stage_pts * k * DIM);        // [stage_pts * k]
    const int pg = GRAD_THREADS / lp;                                           // point slots = points per pass (divides stage_pts)

    const int64_t blk = xcd_block(blockIdx.x, blocks_per_xcd);
    if (blk >= n_blocks) return;
    const int64_t p0 = blk * GRAD_BLOCK;
    const int n_p = (int)min((int64_t)GRAD_BLOCK, n - p0);
    const int t = threadIdx.x, lane = t & (lp - 1), slot = t / lp;
    const int kd = k * DIM;

    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        const int64_t col0 = ((int64_t)chunk * lp + lane) * VEC;
        const bool col_ok = col0 < row_len;                                     // VEC divides row_len: a piece is inside or outside
        for (int sb = 0; sb < n_p; sb += stage_pts) {
            const int n_st = min(stage_pts, n_p - sb);
            __syncthreads();                                                    // the previous stage's tables have been read
            const double *gc = coef + (p0 + sb) * kd;
            for (int i = t; i < n_st * kd; i += GRAD_THREADS) s_c[i] = gc[i];
            const int32_t *gi = idx + (p0 + sb) * k;
            for (int i = t; i < n_st * k; i += GRAD_THREADS) s_i[i] = gi[i];
            __syncthreads();
            for (int pb = sb; pb < sb + n_st; pb += pg) {
                if (!(col_ok && pb + slot < sb + n_st)) continue;
                const int64_t p = p0 + pb + slot;
                const int64_t orow = rows ? (int64_t)rows[p] : p;
                const double *cp = s_c + (pb - sb + slot) * kd;
                const int32_t *ip = s_i + (pb - sb + slot) * k;
                const T *col = field + col0;

                double fc[NCOMP][VEC], acc[NCOMP][DIM][VEC];
#pragma unroll
                for (int c = 0; c < NCOMP; ++c) {
                    const V raw = row_load<T, VEC>(col + orow * in_stride + c * row_len);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) fc[c][i] = row_elem<T, VEC>(raw, i);
#pragma unroll
                    for (int a = 0; a < DIM; ++a)
#pragma unroll
                        for (int i = 0; i < VEC; ++i) acc[c][a][i] = 0.0;
                }
                int m = 0;
                for (; m + GRAD_FLIGHT <= k; m += GRAD_FLIGHT) {
                    V raw[GRAD_FLIGHT][NCOMP];
#pragma unroll
                    for (int u = 0; u < GRAD_FLIGHT; ++u) {
                        const T *row = col + (int64_t)ip[m + u] * in_stride;
#pragma unroll
                        for (int c = 0; c < NCOMP; ++c) raw[u][c] = row_load<T, VEC>(row + c * row_len);
                    }
#pragma unroll
                    for (int u = 0; u < GRAD_FLIGHT; ++u) {
                        double cu[DIM];
#pragma unroll
                        for (int a = 0; a < DIM; ++a) cu[a] = cp[(m + u) * DIM + a];
#pragma unroll
                        for (int c = 0; c < NCOMP; ++c)
#pragma unroll
                            for (int i = 0; i < VEC; ++i) {
                                const double d = row_elem<T, VEC>(raw[u][c], i) - fc[c][i];
#pragma unroll
                                for (int a = 0; a < DIM; ++a) acc[c][a][i] = fma(cu[a], d, acc[c][a][i]);
                            }
                    }
                }
                for (; m < k; ++m) {
                    V raw[NCOMP];
                    const T *row = col + (int64_t)ip[m] * in_stride;
#pragma unroll
                    for (int c = 0; c < NCOMP; ++c) raw[c] = row_load<T, VEC>(row + c * row_len);
                    double cu[DIM];
#pragma unroll
                    for (int a = 0; a < DIM; ++a) cu[a] = cp[m * DIM + a];
#pragma unroll
                    for (int c = 0; c < NCOMP; ++c)
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            const double d = row_elem<T, VEC>(raw[c], i) - fc[c][i];
#pragma unroll
                            for (int a = 0; a < DIM; ++a) acc[c][a][i] = fma(cu[a], d, acc[c][a][i]);
                        }
                }

                double *op = out + orow * out_stride + col0;                    // (the output row may start anywhere: element stores)
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    double G[NCOMP][DIM], o[NOUT];
#pragma unroll
                    for (int c = 0; c < NCOMP; ++c)
#pragma unroll
                        for (int a = 0; a < DIM; ++a) G[c][a] = acc[c][a][i];
                    grad_finish<DIM, NCOMP, MODE>(G, o);
#pragma unroll
                    for (int q = 0; q < NOUT; ++q) op[q * row_len + i] = o[q];
                }
            }
        }
    }
}

struct GradArgs {
    const double *coef;
    const int32_t *idx;
    int64_t n;
    int k;
    const void *field;
    int64_t row_len, in_stride;
    const int32_t *rows;
    double *out;
    int64_t out_stride;
    hipStream_t st;
};

template <typename T, int VEC, int DIM, int NCOMP, int MODE>
int launch_grad(const GradArgs &g) {
    // LDS (slot_shape, csrc/point_slots.h): per point of a stage its coefficients and ids (64 points: 46.6 KB at k = 26 in 3-D)
    SlotShape shape;
    if (const int rc = slot_shape("s3_grad_apply", g.row_len, g.row_len / VEC, (size_t)g.k * (sizeof(double) * DIM + sizeof(int32_t)), 0, 0, shape))
        return rc;
    const int64_t n_blocks = (g.n + GRAD_BLOCK - 1) / GRAD_BLOCK;
    const XcdGrid xcd = xcd_grid(n_blocks);
    S3_REQUIRE(xcd.fits(), "s3_grad_apply: too many points");
    grad_apply_kernel<T, VEC, DIM, NCOMP, MODE><<<(unsigned)xcd.grid, GRAD_THREADS, shape.lds_bytes, g.st>>>(
        g.coef, g.idx, g.n, g.k, static_cast<const T *>(g.field), g.row_len, g.in_stride, g.rows, g.out, g.out_stride, shape.lanes,
        shape.stage_pts, (int)shape.n_chunks, n_blocks, xcd.per_xcd);
    S3_LAUNCH_CHECK();
    return S3_OK;
}

template <typename T, int VEC, int DIM, int MODE>
int grad_by_comp(const GradArgs &g, int n_comp) {
    if (n_comp == 1) return launch_grad<T, VEC, DIM, 1, MODE>(g);
    if (n_comp == 2) return launch_grad<T, VEC, DIM, 2, MODE>(g);
    return launch_grad<T, VEC, DIM, 3, MODE>(g);
}

template <typename T, int VEC, int DIM>
int grad_by_mode(const GradArgs &g, int n_comp, int mode) {
    switch (mode) {
    case S3_GRAD_GRADIENT: return grad_by_comp<T, VEC, DIM, S3_GRAD_GRADIENT>(g, n_comp);
    case S3_GRAD_MAGNITUDE: return grad_by_comp<T, VEC, DIM, S3_GRAD_MAGNITUDE>(g, n_comp);
    case S3_GRAD_DIVERGENCE: return launch_grad<T, VEC, DIM, DIM, S3_GRAD_DIVERGENCE>(g);
    case S3_GRAD_VORTICITY: return launch_grad<T, VEC, DIM, DIM, S3_GRAD_VORTICITY>(g);
    case S3_GRAD_VORTICITY_MAGNITUDE: return launch_grad<T, VEC, DIM, DIM, S3_GRAD_VORTICITY_MAGNITUDE>(g);
    default: return launch_grad<T, VEC, DIM, DIM, S3_GRAD_Q>(g);
    }
}

}  // namespace

}  // namespace s3

using namespace s3;

extern "C" {

int s3_grad_coeff(const double *d_pts, int64_t n, int dim, const int32_t *d_idx, int k, int power, const int32_t *d_rows,
                  double *d_coef, uint8_t *d_flag, int64_t *h_n_degenerate, s3_stream stream) {
    S3_REQUIRE(h_n_degenerate != nullptr, "s3_grad_coeff: null output");
    *h_n_degenerate = 0;
    S3_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) && (dim == 2 || dim == 3), "s3_grad_coeff: bad shape n=%lld dim=%d", (long long)n, dim);
    S3_REQUIRE(k >= 1 && k <= S3_MAX_K, "s3_grad_coeff: k=%d outside [1,%d]", k, S3_MAX_K);
    S3_REQUIRE(power >= 0 && power <= 2, "s3_grad_coeff: power=%d outside [0,2]", power);
    if (n == 0) return S3_OK;
    S3_REQUIRE(d_pts && d_idx && d_coef && d_flag, "s3_grad_coeff: null array");
    hipStream_t st = as_stream(stream);
    DevBuf<unsigned long long> count;
    S3_HIP_CHECK(count.alloc(1));
    S3_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(unsigned long long), st));
    if (dim == 2)
        grad_coeff_kernel<2><<<grid_for(n, 256), 256, 0, st>>>(d_pts, n, d_idx, k, power, d_rows, d_coef, d_flag, count);
    else
        grad_coeff_kernel<3><<<grid_for(n, 256), 256, 0, st>>>(d_pts, n, d_idx, k, power, d_rows, d_coef, d_flag, count);
    S3_LAUNCH_CHECK();
    unsigned long long h_count = 0;
    S3_HIP_CHECK(hipMemcpyAsync(&h_count, count, sizeof(h_count), hipMemcpyDeviceToHost, st));
    S3_HIP_CHECK(hipStreamSynchronize(st));
    *h_n_degenerate = (int64_t)h_count;
    return S3_OK;
}

int s3_grad_apply(const double *d_coef, const int32_t *d_idx, int64_t n, int k, int dim, const void *d_field, int dtype, int n_comp,
                  int64_t row_len, int64_t in_stride, const int32_t *d_rows, int mode, double *d_out, int64_t out_stride,
                  s3_stream stream) {
    S3_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) && row_len >= 1 && (dim == 2 || dim == 3), "s3_grad_apply: bad shape n=%lld row_len=%lld dim=%d",
               (long long)n, (long long)row_len, dim);
    S3_REQUIRE(k >= 1 && k <= S3_MAX_K, "s3_grad_apply: k=%d outside [1,%d]", k, S3_MAX_K);
    S3_REQUIRE(n_comp >= 1 && n_comp <= 3, "s3_grad_apply: n_comp=%d outside [1,3] (wider fields go in groups of components)", n_comp);
    S3_REQUIRE(mode >= S3_GRAD_GRADIENT && mode <= S3_GRAD_Q, "s3_grad_apply: unknown mode %d", mode);
    S3_REQUIRE(mode == S3_GRAD_GRADIENT || mode == S3_GRAD_MAGNITUDE || n_comp == dim,
               "s3_grad_apply: mode %d needs a vector field with n_comp == dim, got n_comp=%d dim=%d", mode, n_comp, dim);
    S3_REQUIRE(dtype == S3_DTYPE_F32 || dtype == S3_DTYPE_F64, "s3_grad_apply: unknown dtype %d", dtype);
    const int64_t n_out = grad_n_out(mode, dim, n_comp);
    if (in_stride <= 0) in_stride = n_comp * row_len;
    if (out_stride <= 0) out_stride = n_out * row_len;
    S3_REQUIRE(in_stride >= n_comp * row_len && out_stride >= n_out * row_len, "s3_grad_apply: in_stride %lld / out_stride %lld shorter than a row",
               (long long)in_stride, (long long)out_stride);
    if (n == 0) return S3_OK;
    S3_REQUIRE(d_coef && d_idx && d_field && d_out, "s3_grad_apply: null array");
    const GradArgs g{d_coef, d_idx, n, k, d_field, row_len, in_stride, d_rows, d_out, out_stride, as_stream(stream)};
    // the width of a lane's piece: every component row of every field row must start on a 16-byte boundary
    return dispatch_rows<WidestRowWidth>(dtype, row_width<WidestRowWidth>(dtype, d_field, row_len, in_stride), [&](auto row) {
        using T = typename decltype(row)::type;
        constexpr int VEC = decltype(row)::vec;
        return dim == 2 ? grad_by_mode<T, VEC, 2>(g, n_comp, mode) : grad_by_mode<T, VEC, 3>(g, n_comp, mode);
    });
}

}  // extern "C"
