// KNN inverse-distance interpolation of snapshot fields onto the S^3 cells (the roofline kernel).  gfx950 only.
//
// Reference behaviour restated here: interpolate_data, export.py:446-468
//     out[c, j, t] = sum_m  w[c, m] * data[idx[c, m], j, t]          (f64 weights, f32/f64 data, f64 output)
// and the metric re-interpolation at export.py:215 (row_len = 1).
//
// HBM layout: data is the caller's [n_src][row_len] matrix with row_len = n_comp*T contiguous per source point, so a
// neighbour's contribution to one output row is one contiguous row read.  A workgroup (256 threads = 4 wavefronts)
// owns a tile of TC consecutive output cells: it stages the tile's k neighbour indices (i32) and weights (f64) in LDS
// once, then its threads sweep the tile's TC*row_len outputs in row-major order so that the 64 lanes of a wavefront read
// 64 consecutive VEC-wide pieces of the same source row (1 KiB per wave-instruction for f32 x4) and write 64
// consecutive pieces of the output row.  Accumulation is f64 FMA in neighbour order (the reference forms the rounded
// product and then sums; the difference is <= k ulp, the contract is 1e-5 relative).  No MFMA: this is a gather +
// weighted reduce with ~0.5 flop per byte.
//
// Workgroup -> tile mapping is XCD-aware (xcd_block, csrc/point_slots.h): XCD x sweeps the x-th contiguous eighth of the
// tiles and spatially adjacent cells (which share neighbours) hit the same 4 MiB L2.
#include "point_slots.h"
#include "typed_rows.h"

#include <type_traits>

namespace s3 {

constexpr int INTERP_BLOCK = 256;

template <typename T, int VEC>
__global__ void __launch_bounds__(INTERP_BLOCK)
interp_kernel(const double *__restrict__ w, const int32_t *__restrict__ idx, int64_t nc, int k,
              const T *__restrict__ data, int64_t row_len, double *__restrict__ out, int tc, int64_t n_tiles,
              int64_t tiles_per_xcd) {
    extern __shared__ double lds[];
    double *s_w = lds;                                                  // [tc*k]
    int32_t *s_idx = reinterpret_cast<int32_t *>(lds + (size_t)tc * k); // [tc*k]

    const int64_t tile = xcd_block(blockIdx.x, tiles_per_xcd);
    if (tile >= n_tiles) return;
    const int64_t c0 = tile * tc;
    const int n_c = (int)min((int64_t)tc, nc - c0);

    const int n_stage = n_c * k;
    for (int i = threadIdx.x; i < n_stage; i += INTERP_BLOCK) {
        s_w[i] = w[c0 * k + i];
        s_idx[i] = idx[c0 * k + i];
    }
    __syncthreads();

    const int lv_count = (int)(row_len / VEC);            // VEC-wide pieces per row
    const int n_items = n_c * lv_count;
    for (int item = threadIdx.x; item < n_items; item += INTERP_BLOCK) {
        const int cl = item / lv_count;
        const int lv = item - cl * lv_count;
        const double *wp = s_w + cl * k;
        const int32_t *ip = s_idx + cl * k;
        const T *col = data + (int64_t)lv * VEC;
        double acc[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = 0.0;
        int m = 0;
        // eight independent row reads in flight per lane before the first FMA (the kernel is bound by gather latency /
        // Infinity-Cache bandwidth, not by arithmetic)
        for (; m + 8 <= k; m += 8) {
            double v[8][VEC];
#pragma unroll
            for (int u = 0; u < 8; ++u) row_load_wide<T, VEC>(col + (int64_t)ip[m + u] * row_len, v[u]);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const double wu = wp[m + u];
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[i] = fma(wu, v[u][i], acc[i]);
            }
        }
        for (; m + 4 <= k; m += 4) {
            double v0[VEC], v1[VEC], v2[VEC], v3[VEC];
            const int64_t r0 = ip[m], r1 = ip[m + 1], r2 = ip[m + 2], r3 = ip[m + 3];
            row_load_wide<T, VEC>(col + r0 * row_len, v0);
            row_load_wide<T, VEC>(col + r1 * row_len, v1);
            row_load_wide<T, VEC>(col + r2 * row_len, v2);
            row_load_wide<T, VEC>(col + r3 * row_len, v3);
            const double w0 = wp[m], w1 = wp[m + 1], w2 = wp[m + 2], w3 = wp[m + 3];
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                acc[i] = fma(w0, v0[i], acc[i]);
                acc[i] = fma(w1, v1[i], acc[i]);
                acc[i] = fma(w2, v2[i], acc[i]);
                acc[i] = fma(w3, v3[i], acc[i]);
            }
        }
        for (; m < k; ++m) {
            double v0[VEC];
            row_load_wide<T, VEC>(col + (int64_t)ip[m] * row_len, v0);
            const double w0 = wp[m];
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = fma(w0, v0[i], acc[i]);
        }
        row_store<VEC>(out + (c0 + cl) * row_len + (int64_t)lv * VEC, acc);
    }
}

// ---- storage-type conversions of the file path, by integer arithmetic ------------------------------------------------
// The single-precision file stores round(f64) once, to nearest even, and must equal the host's cast (numpy astype, x86
// cvtsd2ss) bit for bit over the whole range: ties, results that are f32 subnormals, magnitudes below half the smallest
// subnormal (+-0, sign kept), the overflow boundary (+-inf).  Whether v_cvt_f32_f64 produces f32 subnormals depends on the
// kernel's MODE.fp_denorm field; these conversions do not look at it: they work on the bit patterns.
__device__ __forceinline__ uint32_t f64_to_f32_bits(double x) {
    const uint64_t u = (uint64_t)__double_as_longlong(x);
    const uint32_t sign = (uint32_t)(u >> 32) & 0x80000000u;
    const int e = (int)((u >> 52) & 0x7ff);
    const uint64_t m = u & 0x000fffffffffffffull;
    if (e == 0x7ff) return sign | 0x7f800000u | (m ? 0x00400000u | (uint32_t)(m >> 29) : 0u);   // inf; NaN: quieted, payload's top bits
    const int ef = e - 896;                                              // biased f32 exponent (1023 - 127)
    if (ef >= 255) return sign | 0x7f800000u;
    if (ef > 0) {
        uint32_t r = ((uint32_t)ef << 23) | (uint32_t)(m >> 29);
        const uint32_t rem = (uint32_t)m & 0x1fffffffu;                  // the 29 bits that leave
        r += (rem > 0x10000000u) | ((rem == 0x10000000u) & (r & 1u));    // a carry walks into the exponent: 0x7f800000 = inf at the boundary
        return sign | r;
    }
    // the result is a subnormal (unit 2^-149) or zero: the 53-bit significand moves right by 30 - ef >= 30 places
    const int shift = 30 - ef;
    if (shift > 53) return sign;                                         // |x| < 2^-150 (f64 subnormals included): below half a unit
    const uint64_t sig = m | 0x0010000000000000ull;
    uint32_t r = (uint32_t)(sig >> shift);                               // (shift = 53: 0)
    const uint64_t rem = sig & (((uint64_t)1 << shift) - 1), half = (uint64_t)1 << (shift - 1);
    r += (rem > half) | ((rem == half) & (r & 1u));                      // 0x007fffff + 1 = the smallest normal
    return sign | r;
}

__device__ __forceinline__ uint64_t f32_to_f64_bits(uint32_t v) {      // exact
    const uint64_t sign = (uint64_t)(v & 0x80000000u) << 32;
    int e = (int)((v >> 23) & 0xff);
    uint32_t m = v & 0x007fffffu;
    if (e == 0xff) return sign | 0x7ff0000000000000ull | (m ? 0x0008000000000000ull | ((uint64_t)m << 29) : 0ull);
    if (e == 0) {
        if (m == 0) return sign;
        const int sh = __clz((int)m) - 8;                                // a subnormal: its leading one moves to bit 23
        m = (m << sh) & 0x007fffffu;
        e = 1 - sh;
    }
    return sign | ((uint64_t)(e + 896) << 52) | ((uint64_t)m << 29);
}

// the bits of `v` in the storage type Out, kept in an unsigned word of Out's size (what LDS tiles and stores carry)
template <typename Out> struct Word;
template <> struct Word<float> { using type = uint32_t; };
template <> struct Word<double> { using type = uint64_t; };

template <typename Out, typename In>
__device__ __forceinline__ typename Word<Out>::type stored_bits(In v) {
    if constexpr (sizeof(In) == 8 && sizeof(Out) == 4) return f64_to_f32_bits(v);
    else if constexpr (sizeof(In) == 4 && sizeof(Out) == 8) return f32_to_f64_bits(__float_as_uint(v));
    else if constexpr (sizeof(In) == 8) return (uint64_t)__double_as_longlong(v);
    else return __float_as_uint(v);
}

// [nc][n_comp][T] -> [T][n_out][n_comp]: snapshot-major image of an interpolated batch for the HDF5 sink, which writes one
// dataset per snapshot (reference export.py:283-299 slices out[:, :, i] on the host).  32x32 tiles through LDS: reads run
// along t, writes along the cell axis.  `rows` (optional): input cell c is row rows[c] of the output (a rank's shard of the
// cells -- ascending ids, mostly runs of siblings -- written into the batch buffer all ranks share); NULL: row c, n_out = nc.
// OutT = float: the value is rounded once on its way out (f64_to_f32_bits); this form serves more than 3 components.
template <typename OutT>
__global__ void __launch_bounds__(256)
snapshot_major_kernel(const double *__restrict__ in, int64_t nc, int n_comp, int64_t T, const int32_t *__restrict__ rows,
                      int64_t n_out, OutT *__restrict__ out) {
    __shared__ double tile[32][33];
    const int j = blockIdx.z;
    const int64_t c0 = (int64_t)blockIdx.x * 32, t0 = (int64_t)blockIdx.y * 32;   // cells on x: up to 2^31 tiles
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;            // 32 x 8 threads
    for (int r = ty; r < 32; r += 8) {
        const int64_t c = c0 + r, t = t0 + tx;
        if (c < nc && t < T) tile[r][tx] = in[(c * n_comp + j) * T + t];
    }
    __syncthreads();
    const int64_t c = c0 + tx;
    const int64_t row = c < nc ? (rows ? (int64_t)rows[c] : c) : 0;
    for (int r = ty; r < 32; r += 8) {
        const int64_t t = t0 + r;
        if (c < nc && t < T) {
            if constexpr (sizeof(OutT) == 8) out[(t * n_out + row) * n_comp + j] = tile[tx][r];
            else reinterpret_cast<uint32_t *>(out)[(t * n_out + row) * n_comp + j] = f64_to_f32_bits(tile[tx][r]);
        }
    }
}

// The single-precision image for 1 to 3 components: a workgroup owns SM_CELLS cells x 32 snapshots x ALL components, so that
// what it writes per snapshot is ONE run of n_c * n_comp floats (256 to 768 bytes), stored VEC floats per lane.  VEC comes
// from the launch: the output's base address and its row length n_out * n_comp decide what every run is aligned to.  With a
// row list (VEC = 1) a cell's n_comp floats go to row rows[c].  LDS holds the rounded bits, [32][SM_LD] words (odd pitch: the
// transposed reads of the first phase's columns are conflict-free).
constexpr int SM_CELLS = 64, SM_MAX_COMP = 3, SM_LD = SM_CELLS * SM_MAX_COMP + 1;

template <int VEC>
__global__ void __launch_bounds__(256)
snapshot_major_f32_kernel(const double *__restrict__ in, int64_t nc, int n_comp, int64_t T, const int32_t *__restrict__ rows,
                          int64_t n_out, uint32_t *__restrict__ out) {
    __shared__ uint32_t tile[32 * SM_LD];
    __shared__ int32_t s_row[SM_CELLS];
    const int64_t c0 = (int64_t)blockIdx.x * SM_CELLS, t0 = (int64_t)blockIdx.y * 32;
    const int n_c = (int)min((int64_t)SM_CELLS, nc - c0), n_t = (int)min((int64_t)32, T - t0);
    const int n_r = n_c * n_comp;                                       // input rows (cell, component) of this tile: contiguous
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    if (rows != nullptr && (int)threadIdx.x < n_c) s_row[threadIdx.x] = rows[c0 + threadIdx.x];
    if (tx < n_t) {
        const double *src = in + (c0 * n_comp) * T + t0 + tx;
        for (int r = ty; r < n_r; r += 8) tile[tx * SM_LD + r] = f64_to_f32_bits(src[(int64_t)r * T]);
    }
    __syncthreads();
    if (rows != nullptr) {                                              // (VEC = 1)
        for (int item = threadIdx.x; item < n_t * n_r; item += 256) {
            const int tl = item / n_r, e = item - tl * n_r;
            const int cl = e / n_comp, j = e - cl * n_comp;
            out[((t0 + tl) * n_out + (int64_t)s_row[cl]) * n_comp + j] = tile[tl * SM_LD + e];
        }
        return;
    }
    const int n_v = n_r / VEC;                                          // (the launch has checked that VEC divides every run)
    for (int item = threadIdx.x; item < n_t * n_v; item += 256) {
        const int tl = item / n_v, e = (item - tl * n_v) * VEC;
        const uint32_t *w = tile + tl * SM_LD + e;
        uint32_t *dst = out + ((t0 + tl) * n_out + c0) * n_comp + e;
        if constexpr (VEC == 4) *reinterpret_cast<uint4 *>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
        else if constexpr (VEC == 2) *reinterpret_cast<uint2 *>(dst) = make_uint2(w[0], w[1]);
        else dst[0] = w[0];
    }
}

// The loader's inverse: snapshots [T_b][n_rows] (n_rows = nc * n_comp, a dataset per snapshot as the file holds them, In = f32
// or f64) -> columns [t0, t0 + T_b) of the cell-major matrix out[n_rows][ld] of type Out that SVD and DMD read (reference
// data.py:249-300 stacks the datasets on the host).  A workgroup moves 64 rows x TW snapshots through LDS: it reads runs of 64
// consecutive input values per snapshot (256 / 512 bytes) and writes TW consecutive columns per output row.  TW (4, 16, 32)
// follows T_b, so that short groups do not idle most lanes of the second phase.  LDS keeps the converted bits; its pitch
// 64 + 32 / TW puts the second phase's reads (TW columns x 64 / TW rows per wavefront) on different banks.
template <typename In, typename Out, int TW>
__global__ void __launch_bounds__(256)
cell_major_kernel(const In *__restrict__ in, int64_t n_rows, int64_t T_b, typename Word<Out>::type *__restrict__ out, int64_t ld,
                  int64_t t0) {
    using W = typename Word<Out>::type;
    constexpr int LD = 64 + 32 / TW;
    __shared__ W tile[TW * LD];
    const int64_t r0 = (int64_t)blockIdx.x * 64, b0 = (int64_t)blockIdx.y * TW;
    const int n_r = (int)min((int64_t)64, n_rows - r0), n_b = (int)min((int64_t)TW, T_b - b0);
    {
        const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;        // 64 rows x 4 snapshots per pass
        if (lx < n_r)
            for (int b = ly; b < n_b; b += 4) tile[b * LD + lx] = stored_bits<Out, In>(in[(b0 + b) * n_rows + r0 + lx]);
    }
    __syncthreads();
    const int tx = threadIdx.x % TW, ty = threadIdx.x / TW;            // TW snapshots x 256 / TW rows per pass
    if (tx < n_b)
        for (int r = ty; r < n_r; r += 256 / TW) out[(r0 + r) * ld + t0 + b0 + tx] = tile[tx * LD + r];
}

template <typename T, int VEC>
static int launch_interp(const double *w, const int32_t *idx, int64_t nc, int k, const void *data, int64_t row_len,
                         double *out, hipStream_t st) {
    const int64_t lv_count = row_len / VEC;
    // tile height: enough outputs per workgroup to amortise the LDS staging, bounded by 48 KiB of LDS (12 B per
    // (cell, neighbour): a few workgroups stay resident per CU and the launch needs no opt-in to a larger LDS window)
    int64_t tc = (2048 + lv_count - 1) / lv_count;
    const int64_t tc_lds = (48 * 1024) / ((int64_t)k * (sizeof(double) + sizeof(int32_t)));
    if (tc > 256) tc = 256;
    if (tc > tc_lds) tc = tc_lds;
    if (tc < 1) tc = 1;
    if (tc > nc) tc = nc;
    const int64_t n_tiles = (nc + tc - 1) / tc;
    const XcdGrid xcd = xcd_grid(n_tiles);
    S3_REQUIRE(xcd.fits(), "s3_interp: too many tiles (%lld)", (long long)xcd.grid);
    S3_REQUIRE(tc * lv_count < ((int64_t)1 << 31), "s3_interp: row_len %lld too long", (long long)row_len);
    size_t lds = (size_t)tc * k * (sizeof(double) + sizeof(int32_t));
    interp_kernel<T, VEC><<<(unsigned)xcd.grid, INTERP_BLOCK, lds, st>>>(w, idx, nc, k, static_cast<const T *>(data),
                                                                        row_len, out, (int)tc, n_tiles, xcd.per_xcd);
    S3_LAUNCH_CHECK();
    return S3_OK;
}

}  // namespace s3

using namespace s3;

extern "C" {

int s3_interp(const double *d_w, const int32_t *d_idx, int64_t nc, int k, const void *d_data, int dtype, int64_t n_src,
              int64_t row_len, double *d_out, s3_stream stream) {
    S3_REQUIRE(nc >= 0 && row_len >= 0 && n_src >= 1, "s3_interp: bad shape nc=%lld row_len=%lld n_src=%lld",
               (long long)nc, (long long)row_len, (long long)n_src);
    S3_REQUIRE(k >= 1 && k <= S3_MAX_K, "s3_interp: k=%d outside [1,%d]", k, S3_MAX_K);
    S3_REQUIRE(dtype == S3_DTYPE_F32 || dtype == S3_DTYPE_F64, "s3_interp: unknown dtype %d", dtype);
    if (nc == 0 || row_len == 0) return S3_OK;
    S3_REQUIRE(d_w && d_idx && d_data && d_out, "s3_interp: null array");
    S3_REQUIRE(n_src < ((int64_t)1 << 31), "s3_interp: n_src must fit int32");
    hipStream_t st = as_stream(stream);
    // (the output is stored 16 bytes at a time whatever the width of the loads)
    const int width = reinterpret_cast<uintptr_t>(d_out) % 16 == 0 ? row_width<EveryRowWidth>(dtype, d_data, row_len) : 1;
    return dispatch_rows<EveryRowWidth>(dtype, width, [&](auto row) {
        return launch_interp<typename decltype(row)::type, decltype(row)::vec>(d_w, d_idx, nc, k, d_data, row_len, d_out, st);
    });
}

int s3_snapshot_major_rows_as(const double *d_in, int64_t nc, int n_comp, int64_t n_snapshots, const int32_t *d_rows,
                              int64_t n_out, int out_dtype, void *d_out, s3_stream stream) {
    S3_REQUIRE(nc >= 0 && n_comp >= 1 && n_snapshots >= 0 && n_out >= nc, "s3_snapshot_major: bad shape");
    S3_REQUIRE(out_dtype == S3_DTYPE_F32 || out_dtype == S3_DTYPE_F64, "s3_snapshot_major: unknown output type %d", out_dtype);
    if (nc == 0 || n_snapshots == 0) return S3_OK;
    S3_REQUIRE(d_in && d_out && (const void *)d_in != d_out, "s3_snapshot_major: null or aliased array");
    S3_REQUIRE(d_rows != nullptr || n_out == nc, "s3_snapshot_major: without a row list the output has the input's rows");
    const int64_t gy = (n_snapshots + 31) / 32;
    hipStream_t st = as_stream(stream);
    if (out_dtype == S3_DTYPE_F32 && n_comp <= SM_MAX_COMP) {
        const int64_t gx = (nc + SM_CELLS - 1) / SM_CELLS;
        S3_REQUIRE(gx < ((int64_t)1 << 31) && gy <= 65535, "s3_snapshot_major: shape too large for one launch");
        S3_REQUIRE(reinterpret_cast<uintptr_t>(d_out) % 4 == 0, "s3_snapshot_major: output not aligned to its elements");
        // every run starts at d_out + ((t * n_out + c0) * n_comp) floats, c0 a multiple of 64, and is as long as the row or 64 * n_comp
        const uintptr_t a = reinterpret_cast<uintptr_t>(d_out);
        const int64_t row = n_out * n_comp;
        const dim3 grid((unsigned)gx, (unsigned)gy);
        uint32_t *o = static_cast<uint32_t *>(d_out);
        if (d_rows == nullptr && a % 16 == 0 && row % 4 == 0)
            snapshot_major_f32_kernel<4><<<grid, 256, 0, st>>>(d_in, nc, n_comp, n_snapshots, nullptr, n_out, o);
        else if (d_rows == nullptr && a % 8 == 0 && row % 2 == 0)
            snapshot_major_f32_kernel<2><<<grid, 256, 0, st>>>(d_in, nc, n_comp, n_snapshots, nullptr, n_out, o);
        else
            snapshot_major_f32_kernel<1><<<grid, 256, 0, st>>>(d_in, nc, n_comp, n_snapshots, d_rows, n_out, o);
        S3_LAUNCH_CHECK();
        return S3_OK;
    }
    const int64_t gx = (nc + 31) / 32;
    S3_REQUIRE(gx < ((int64_t)1 << 31) && gy <= 65535 && n_comp <= 65535, "s3_snapshot_major: shape too large for one launch");
    const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)n_comp);
    if (out_dtype == S3_DTYPE_F32) {
        S3_REQUIRE(reinterpret_cast<uintptr_t>(d_out) % 4 == 0, "s3_snapshot_major: output not aligned to its elements");
        snapshot_major_kernel<float><<<grid, 256, 0, st>>>(d_in, nc, n_comp, n_snapshots, d_rows, n_out, static_cast<float *>(d_out));
    } else {
        snapshot_major_kernel<double><<<grid, 256, 0, st>>>(d_in, nc, n_comp, n_snapshots, d_rows, n_out, static_cast<double *>(d_out));
    }
    S3_LAUNCH_CHECK();
    return S3_OK;
}

int s3_snapshot_major_as(const double *d_in, int64_t nc, int n_comp, int64_t n_snapshots, int out_dtype, void *d_out,
                         s3_stream stream) {
    return s3_snapshot_major_rows_as(d_in, nc, n_comp, n_snapshots, nullptr, nc, out_dtype, d_out, stream);
}

int s3_snapshot_major_rows(const double *d_in, int64_t nc, int n_comp, int64_t n_snapshots, const int32_t *d_rows,
                           int64_t n_out, double *d_out, s3_stream stream) {
    return s3_snapshot_major_rows_as(d_in, nc, n_comp, n_snapshots, d_rows, n_out, S3_DTYPE_F64, d_out, stream);
}

int s3_snapshot_major(const double *d_in, int64_t nc, int n_comp, int64_t n_snapshots, double *d_out, s3_stream stream) {
    return s3_snapshot_major_rows_as(d_in, nc, n_comp, n_snapshots, nullptr, nc, S3_DTYPE_F64, d_out, stream);
}

int s3_cell_major(const void *d_in, int in_dtype, int64_t n_snapshots, int64_t nc, int n_comp, void *d_out, int out_dtype,
                  int64_t n_cols, int64_t out_stride, int64_t t0, s3_stream stream) {
    S3_REQUIRE(nc >= 0 && n_comp >= 1 && n_snapshots >= 0, "s3_cell_major: bad shape");
    S3_REQUIRE((in_dtype == S3_DTYPE_F32 || in_dtype == S3_DTYPE_F64) && (out_dtype == S3_DTYPE_F32 || out_dtype == S3_DTYPE_F64),
               "s3_cell_major: unknown element type %d -> %d", in_dtype, out_dtype);
    S3_REQUIRE(t0 >= 0 && t0 + n_snapshots <= n_cols && n_cols <= out_stride,
               "s3_cell_major: columns [%lld, %lld) do not lie in a matrix of %lld columns with a row pitch of %lld",
               (long long)t0, (long long)(t0 + n_snapshots), (long long)n_cols, (long long)out_stride);
    if (nc == 0 || n_snapshots == 0) return S3_OK;
    S3_REQUIRE(d_in && d_out && d_in != d_out, "s3_cell_major: null or aliased array");
    S3_REQUIRE(reinterpret_cast<uintptr_t>(d_in) % (in_dtype == S3_DTYPE_F32 ? 4 : 8) == 0 &&
               reinterpret_cast<uintptr_t>(d_out) % (out_dtype == S3_DTYPE_F32 ? 4 : 8) == 0, "s3_cell_major: array not aligned to its elements");
    const int64_t n_rows = nc * n_comp;
    const int tw = n_snapshots <= 4 ? 4 : (n_snapshots <= 16 ? 16 : 32);
    const int64_t gx = (n_rows + 63) / 64, gy = (n_snapshots + tw - 1) / tw;
    S3_REQUIRE(gx < ((int64_t)1 << 31) && gy <= 65535, "s3_cell_major: shape too large for one launch");
    const dim3 grid((unsigned)gx, (unsigned)gy);
    hipStream_t st = as_stream(stream);
    dispatch_rows<ScalarRows>(in_dtype, 1, [&](auto in) {
        dispatch_rows<ScalarRows>(out_dtype, 1, [&](auto o) {
            using IN = typename decltype(in)::type;
            using OUT = typename decltype(o)::type;
            auto launch = [&](auto tile) {
                cell_major_kernel<IN, OUT, decltype(tile)::value><<<grid, 256, 0, st>>>(static_cast<const IN *>(d_in), n_rows, n_snapshots,
                                                                                       static_cast<typename Word<OUT>::type *>(d_out), out_stride, t0);
            };
            if (tw == 4) launch(std::integral_constant<int, 4>{});
            else if (tw == 16) launch(std::integral_constant<int, 16>{});
            else launch(std::integral_constant<int, 32>{});
        });
    });
    S3_LAUNCH_CHECK();
    return S3_OK;
}

}  // extern "C"
