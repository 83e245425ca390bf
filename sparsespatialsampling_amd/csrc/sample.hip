// Sampling of fields on a generated grid at arbitrary positions (probe points, lines, planes, rasters) by EXACT cell location: the
// grid is a set of disjoint axis-aligned dyadic boxes, so "which cell holds this point" has one answer, and the field there is the
// cell's own value or the multilinear blend of its corner values.  gfx950 only.  No counterpart in the reference, whose
// post-processing hands the cell centres to a plotting library as a bare point cloud.
//
// Definition (include/s3hip.h restates it).  With L = max level, lmin = min level, h(l) = width / 2^l, h_min = h(L), H = h(lmin):
//     corner = c_j - H/2 for the first cell j of level lmin       lo = min over cells of c - h/2, per axis
//     origin = corner - ceil((corner - lo)/H - 1e-9) * H          a lattice of step h_min on which every leaf is aligned
//     a      = rint(((c - h/2) - origin) / h_min)                 the leaf's anchor, a multiple of 2^(L-l) per axis
//     leaf   = the Morton keys [key(a), key(a) + 2^(d (L-l)))     key: bit b of axis a at position b*d + a
// A query x lies in lattice cell i = floor((x - origin)/h_min) (half-open: a point on a face belongs to the upper cell) and in the
// leaf whose range holds key(i), found by a binary search over the sorted range starts.
//
// s3_cell_index runs once per grid (a one-workgroup reduction for the lattice, one thread per cell for the keys, the radix sort of
// csrc/scan_sort.h behind s3_sort_pairs, one thread per cell for the range ends and the overlap check); s3_cell_locate once per
// set of points (one query per thread, not tuned).  s3_cell_sample is the hot path.
//
// Regime of the sample: per query one row (cell mode) or 2^d rows (linear mode) of n_comp * T values are gathered from the field
// itself (neighbouring queries of the Hilbert launch order share cells and corners: L2 / Infinity Cache), n_comp * T f64 values are
// written.  A 1024^2 plane through 461 130 cells reads every touched row about twice and writes 8 bytes per value: the writes
// dominate.
//
// Work split: the point slots of csrc/point_slots.h, as in grad_apply_kernel (csrc/differential.hip).  A workgroup owns SAMPLE_BLOCK
// consecutive queries of the launch order; lane l of a slot owns the columns [(chunk*LP + l)*VEC, +VEC) of EVERY component; the staged
// tables are the row ids and, in linear mode, the 2^d corner weights of each query, formed in the kernel from the query's position
// (nothing of size [n_queries, 2^d] is stored).
//
// Order of every floating-point operation of linear mode: xi_a = clamp((x_a - (c_a - h/2)) / h, 0, 1) in f64 as written;
// w_m: t = (s_m0 > 0 ? xi_0 : 1 - xi_0), then per further axis t = s_ma > 0 ? t * xi_a : fma(-xi_a, t, t) (one rounding per axis);
// out = f64 fma chain over the corners m = 0 .. 2^d - 1 from 0, independent of row_len, VEC, LP and n_comp.  No atomics on
// floating-point values: the same inputs give the same bits on every run.
#include "cell_lookup.h"
#include "point_slots.h"
#include "typed_rows.h"

#include <cmath>

namespace s3 {

namespace {

constexpr int SAMPLE_THREADS = POINT_THREADS;
constexpr int SAMPLE_BLOCK = 256;       // queries per workgroup

// what the one-workgroup reduction over the cells leaves for the host
struct LatticeSeed {
    int lmin, lmax;
    long long first_coarse;             // the first cell of level lmin
    double lo[3];
};

// ---- index ----------------------------------------------------------------------------------------------------------------
template <int DIM>
__global__ void __launch_bounds__(1024)
lattice_seed_kernel(const double *__restrict__ c, const int32_t *__restrict__ level, int64_t n, double width, LatticeSeed *__restrict__ seed) {
    __shared__ int s_min[1024], s_max[1024];
    __shared__ long long s_first[1024];
    __shared__ double s_lo[DIM][1024];
    const int t = threadIdx.x;
    int lmin = INT32_MAX, lmax = INT32_MIN;
    for (int64_t i = t; i < n; i += 1024) {
        lmin = min(lmin, level[i]);
        lmax = max(lmax, level[i]);
    }
    s_min[t] = lmin, s_max[t] = lmax;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (t < s) s_min[t] = min(s_min[t], s_min[t + s]), s_max[t] = max(s_max[t], s_max[t + s]);
        __syncthreads();
    }
    lmin = s_min[0], lmax = s_max[0];
    long long first = INT64_MAX;
    double lo[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) lo[a] = INFINITY;
    if (lmin >= 0 && lmax <= 63) {                                              // (other levels are refused by the host: no shift by them)
        for (int64_t i = t; i < n; i += 1024) {
            const int l = level[i];
            if (l == lmin && i < first) first = i;
            const double h = cell_size(width, l);
#pragma unroll
            for (int a = 0; a < DIM; ++a) lo[a] = fmin(lo[a], c[i * DIM + a] - h / 2);
        }
    }
    s_first[t] = first;
#pragma unroll
    for (int a = 0; a < DIM; ++a) s_lo[a][t] = lo[a];
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (t < s) {
            s_first[t] = min(s_first[t], s_first[t + s]);
#pragma unroll
            for (int a = 0; a < DIM; ++a) s_lo[a][t] = fmin(s_lo[a][t], s_lo[a][t + s]);
        }
        __syncthreads();
    }
    if (t == 0) {
        seed->lmin = lmin, seed->lmax = lmax, seed->first_coarse = s_first[0];
#pragma unroll
        for (int a = 0; a < DIM; ++a) seed->lo[a] = s_lo[a][0];
    }
}

// counts[0]: cells with an anchor more than 1e-6 lattice units off an integer (or outside the lattice); counts[1]: misaligned anchors
template <int DIM>
__global__ void __launch_bounds__(256)
cell_keys_kernel(const double *__restrict__ c, const int32_t *__restrict__ level, int64_t n, double width, Lattice lat,
                 uint64_t *__restrict__ keys, int32_t *__restrict__ ids, unsigned long long *__restrict__ counts) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int l = level[j];
    const double h = cell_size(width, l), extent = (double)(1ull << lat.depth);
    const uint64_t low_bits = (1ull << (lat.depth - l)) - 1;
    uint64_t a[DIM];
    bool off = false, misaligned = false;
#pragma unroll
    for (int ax = 0; ax < DIM; ++ax) {
        const double v = ((c[j * DIM + ax] - h / 2) - lat.origin[ax]) / lat.h_min;
        const double r = rint(v);
        if (!(fabs(v - r) <= 1e-6 && r >= 0.0 && r < extent)) {                 // (NaN and inf fail here, before the conversion)
            off = true;
            a[ax] = 0;
        } else {
            a[ax] = (uint64_t)r;
            misaligned |= (a[ax] & low_bits) != 0;
        }
    }
    if (off) atomicAdd(counts + 0, 1ull);
    else if (misaligned) atomicAdd(counts + 1, 1ull);
    keys[j] = morton_key<DIM>(a, lat.depth);
    ids[j] = (int32_t)j;
}

// ends of the sorted ranges; counts[2]: ranges that reach into their successor
__global__ void __launch_bounds__(256)
cell_ranges_kernel(const uint64_t *__restrict__ starts, const int32_t *__restrict__ ids, const int32_t *__restrict__ level, int64_t n,
                   int dim, int depth, uint64_t *__restrict__ ends, unsigned long long *__restrict__ counts) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t end = starts[i] + (1ull << (dim * (depth - level[ids[i]])));
    ends[i] = end;
    if (i + 1 < n && end > starts[i + 1]) atomicAdd(counts + 2, 1ull);
}

// ---- locate ---------------------------------------------------------------------------------------------------------------
template <int DIM>
__global__ void __launch_bounds__(256)
cell_locate_kernel(const uint64_t *__restrict__ starts, const uint64_t *__restrict__ ends, const int32_t *__restrict__ ids, int64_t n_cells,
                   Lattice lat, const double *__restrict__ x, int64_t nq, const int32_t *__restrict__ rows, int32_t *__restrict__ out) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= nq) return;
    const int64_t q = rows ? (int64_t)rows[j] : j;
    double p[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) p[a] = x[q * DIM + a];
    uint64_t i[DIM];
    int32_t id = -1;
    if (lattice_index<DIM>(lat, p, i)) id = search_leaf(starts, ends, ids, n_cells, morton_key<DIM>(i, lat.depth));
    out[q] = id;
}

// ---- sample ---------------------------------------------------------------------------------------------------------------
// (the corner order of `faces` and the weight chain: corner_plus, local_xi and corner_weight of csrc/cell_lookup.h)
struct SampleArgs {
    const int32_t *cell;
    int64_t nq;
    const int32_t *rows;
    const void *field;
    int64_t n_field_rows, row_len, in_stride;
    const double *x, *centers;
    const int32_t *level, *faces;
    int64_t n_cells;
    double width;
    double *out;
    int64_t out_stride;
    hipStream_t st;
};

// DIM = 0: cell mode (one row per query, copied); DIM = 2 | 3: linear mode over the 2^DIM corner rows
template <typename T, int VEC, int DIM, int NCOMP>
__global__ void __launch_bounds__(SAMPLE_THREADS)
cell_sample_kernel(const int32_t *__restrict__ cell, int64_t nq, const int32_t *__restrict__ rows, const T *__restrict__ field,
                   int64_t n_field_rows, int64_t row_len, int64_t in_stride, const double *__restrict__ x, const double *__restrict__ centers,
                   const int32_t *__restrict__ level, const int32_t *__restrict__ faces, int64_t n_cells, double width,
                   double *__restrict__ out, int64_t out_stride, int lp, int stage_pts, int n_chunks, int64_t n_blocks, int64_t blocks_per_xcd) {
    using V = typename RowVec<T, VEC>::type;
    constexpr int NCORN = DIM == 0 ? 1 : 1 << DIM;
    extern __shared__ double lds[];
    double *s_w = lds;                                                          // [stage_pts * NCORN] (linear mode only)
    int32_t *s_i = reinterpret_cast<int32_t *>(lds + (DIM == 0 ? 0 : (size_t)stage_pts * NCORN));      // [stage_pts * NCORN], -1: no row
    const int pg = SAMPLE_THREADS / lp;

    const int64_t blk = xcd_block(blockIdx.x, blocks_per_xcd);
    if (blk >= n_blocks) return;
    const int64_t p0 = blk * SAMPLE_BLOCK;
    const int n_p = (int)min((int64_t)SAMPLE_BLOCK, nq - p0);
    const int t = threadIdx.x, lane = t & (lp - 1), slot = t / lp;

    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        const int64_t col0 = ((int64_t)chunk * lp + lane) * VEC;
        const bool col_ok = col0 < row_len;                                     // VEC divides row_len: a piece is inside or outside
        for (int sb = 0; sb < n_p; sb += stage_pts) {
            const int n_st = min(stage_pts, n_p - sb);
            __syncthreads();                                                    // the previous stage's tables have been read
            for (int e = t; e < n_st * NCORN; e += SAMPLE_THREADS) {
                const int64_t p = p0 + sb + e / NCORN;
                const int m = e % NCORN;
                const int64_t q = rows ? (int64_t)rows[p] : p;
                const int64_t id = cell[q];
                int32_t row = -1;
                if constexpr (DIM == 0) {
                    if (id >= 0 && id < n_field_rows) row = (int32_t)id;
                } else if (id >= 0 && id < n_cells) {
                    const double h = cell_size(width, level[id]);
                    double xi[DIM];
#pragma unroll
                    for (int a = 0; a < DIM; ++a) xi[a] = local_xi(x[q * DIM + a], centers[id * DIM + a], h);
                    const int32_t node = faces[id * NCORN + m];
                    s_w[e] = corner_weight<DIM>(xi, m);
                    if (node >= 0 && node < n_field_rows) row = node;
                }
                s_i[e] = row;
            }
            __syncthreads();
            for (int pb = sb; pb < sb + n_st; pb += pg) {
                if (!(col_ok && pb + slot < sb + n_st)) continue;
                const int64_t p = p0 + pb + slot;
                const int64_t q = rows ? (int64_t)rows[p] : p;
                const int32_t *ip = s_i + (pb - sb + slot) * NCORN;
                const T *col = field + col0;
                double *op = out + q * out_stride + col0;                       // (the output row may start anywhere: element stores)

                bool hit = true;
#pragma unroll
                for (int m = 0; m < NCORN; ++m) hit &= ip[m] >= 0;
                if (!hit) {                                                     // outside the domain, inside a body, or a bad id
#pragma unroll
                    for (int c = 0; c < NCOMP; ++c)
#pragma unroll
                        for (int i = 0; i < VEC; ++i) op[c * row_len + i] = NAN;
                    continue;
                }
                V raw[NCORN][NCOMP];
#pragma unroll
                for (int m = 0; m < NCORN; ++m) {
                    const T *row = col + (int64_t)ip[m] * in_stride;
#pragma unroll
                    for (int c = 0; c < NCOMP; ++c) raw[m][c] = row_load<T, VEC>(row + c * row_len);
                }
                if constexpr (DIM == 0) {
#pragma unroll
                    for (int c = 0; c < NCOMP; ++c)
#pragma unroll
                        for (int i = 0; i < VEC; ++i) op[c * row_len + i] = row_elem<T, VEC>(raw[0][c], i);
                } else {
                    const double *wp = s_w + (pb - sb + slot) * NCORN;
                    double acc[NCOMP][VEC];
#pragma unroll
                    for (int c = 0; c < NCOMP; ++c)
#pragma unroll
                        for (int i = 0; i < VEC; ++i) acc[c][i] = 0.0;
#pragma unroll
                    for (int m = 0; m < NCORN; ++m) {
                        const double w = wp[m];
#pragma unroll
                        for (int c = 0; c < NCOMP; ++c)
#pragma unroll
                            for (int i = 0; i < VEC; ++i) acc[c][i] = fma(w, row_elem<T, VEC>(raw[m][c], i), acc[c][i]);
                    }
#pragma unroll
                    for (int c = 0; c < NCOMP; ++c)
#pragma unroll
                        for (int i = 0; i < VEC; ++i) op[c * row_len + i] = acc[c][i];
                }
            }
        }
    }
}

template <typename T, int VEC, int DIM, int NCOMP>
int launch_sample(const SampleArgs &g) {
    // LDS (slot_shape, csrc/point_slots.h): per query of a stage its row ids and, in linear mode, its corner weights (64 queries: 6 KB in 3-D)
    constexpr int NCORN = DIM == 0 ? 1 : 1 << DIM;
    SlotShape shape;
    if (const int rc = slot_shape("s3_cell_sample", g.row_len, g.row_len / VEC, NCORN * (sizeof(int32_t) + (DIM == 0 ? 0 : sizeof(double))), 0, 0, shape))
        return rc;
    const int64_t n_blocks = (g.nq + SAMPLE_BLOCK - 1) / SAMPLE_BLOCK;
    const XcdGrid xcd = xcd_grid(n_blocks);
    S3_REQUIRE(xcd.fits(), "s3_cell_sample: too many points");
    cell_sample_kernel<T, VEC, DIM, NCOMP><<<(unsigned)xcd.grid, SAMPLE_THREADS, shape.lds_bytes, g.st>>>(
        g.cell, g.nq, g.rows, static_cast<const T *>(g.field), g.n_field_rows, g.row_len, g.in_stride, g.x, g.centers, g.level, g.faces,
        g.n_cells, g.width, g.out, g.out_stride, shape.lanes, shape.stage_pts, (int)shape.n_chunks, n_blocks, xcd.per_xcd);
    S3_LAUNCH_CHECK();
    return S3_OK;
}

template <typename T, int VEC, int DIM>
int sample_by_comp(const SampleArgs &g, int n_comp) {
    if (n_comp == 1) return launch_sample<T, VEC, DIM, 1>(g);
    if (n_comp == 2) return launch_sample<T, VEC, DIM, 2>(g);
    return launch_sample<T, VEC, DIM, 3>(g);
}

}  // namespace

}  // namespace s3

using namespace s3;

extern "C" {

int s3_cell_index(const double *d_centers, const int32_t *d_levels, int64_t n, int dim, double width, uint64_t *d_starts,
                  uint64_t *d_ends, int32_t *d_ids, s3_grid *h_grid, int64_t *h_refused, s3_stream stream) {
    S3_REQUIRE(h_grid && h_refused, "s3_cell_index: null output");
    for (int i = 0; i < 4; ++i) h_refused[i] = 0;
    S3_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && (dim == 2 || dim == 3), "s3_cell_index: bad shape n=%lld dim=%d", (long long)n, dim);
    S3_REQUIRE(width > 0.0 && std::isfinite(width), "s3_cell_index: width %g is no cell size", width);
    S3_REQUIRE(d_centers && d_levels && d_starts && d_ends && d_ids, "s3_cell_index: null array");
    hipStream_t st = as_stream(stream);

    DevBuf<LatticeSeed> d_seed;
    DevBuf<unsigned long long> d_counts;
    S3_HIP_CHECK(d_seed.alloc(1));
    S3_HIP_CHECK(d_counts.alloc(3));
    S3_HIP_CHECK(hipMemsetAsync(d_counts, 0, 3 * sizeof(unsigned long long), st));
    if (dim == 2)
        lattice_seed_kernel<2><<<1, 1024, 0, st>>>(d_centers, d_levels, n, width, d_seed);
    else
        lattice_seed_kernel<3><<<1, 1024, 0, st>>>(d_centers, d_levels, n, width, d_seed);
    S3_LAUNCH_CHECK();
    LatticeSeed seed;
    S3_HIP_CHECK(hipMemcpyAsync(&seed, d_seed, sizeof(seed), hipMemcpyDeviceToHost, st));
    S3_HIP_CHECK(hipStreamSynchronize(st));
    S3_REQUIRE(seed.lmin >= 0, "s3_cell_index: negative level %d", seed.lmin);
    if ((int64_t)dim * seed.lmax > 63) {
        h_refused[3] = (int64_t)dim * seed.lmax;
        S3_REQUIRE(false, "s3_cell_index: %d levels in %d-D need %lld key bits, 63 are there", seed.lmax, dim, (long long)h_refused[3]);
    }

    Lattice lat{};
    lat.depth = seed.lmax;
    lat.h_min = cell_size(width, seed.lmax);
    const double H = cell_size(width, seed.lmin);
    double first[3] = {0.0, 0.0, 0.0};
    S3_HIP_CHECK(hipMemcpyAsync(first, d_centers + seed.first_coarse * dim, sizeof(double) * dim, hipMemcpyDeviceToHost, st));
    S3_HIP_CHECK(hipStreamSynchronize(st));
    for (int a = 0; a < dim; ++a) {
        const double corner = first[a] - H / 2;
        lat.origin[a] = corner - std::ceil((corner - seed.lo[a]) / H - 1e-9) * H;
    }

    if (dim == 2)
        cell_keys_kernel<2><<<grid_for(n, 256), 256, 0, st>>>(d_centers, d_levels, n, width, lat, d_starts, d_ids, d_counts);
    else
        cell_keys_kernel<3><<<grid_for(n, 256), 256, 0, st>>>(d_centers, d_levels, n, width, lat, d_starts, d_ids, d_counts);
    S3_LAUNCH_CHECK();
    unsigned long long counts[3] = {0, 0, 0};
    S3_HIP_CHECK(hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost, st));
    S3_HIP_CHECK(hipStreamSynchronize(st));
    h_refused[0] = (int64_t)counts[0], h_refused[1] = (int64_t)counts[1];
    S3_REQUIRE(counts[0] == 0 && counts[1] == 0, "s3_cell_index: %llu of %lld cells lie more than 1e-6 lattice units off the lattice, %llu are not aligned to their own size",
               counts[0], (long long)n, counts[1]);

    const int bits = dim * lat.depth > 0 ? dim * lat.depth : 1;
    if (const int rc = s3_sort_pairs(d_starts, d_ids, n, bits, stream)) return rc;
    cell_ranges_kernel<<<grid_for(n, 256), 256, 0, st>>>(d_starts, d_ids, d_levels, n, dim, lat.depth, d_ends, d_counts);
    S3_LAUNCH_CHECK();
    S3_HIP_CHECK(hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost, st));
    S3_HIP_CHECK(hipStreamSynchronize(st));
    h_refused[2] = (int64_t)counts[2];
    S3_REQUIRE(counts[2] == 0, "s3_cell_index: %llu of %lld cells overlap their successor in Morton order", counts[2], (long long)n);

    *h_grid = s3_grid{d_starts, d_ends, d_ids, dim, lat.depth, {lat.origin[0], lat.origin[1], lat.origin[2]}, lat.h_min, n, d_centers, d_levels,
                      width, nullptr};
    return S3_OK;
}

int s3_cell_locate(const s3_grid *grid, const double *d_points, int64_t nq, const int32_t *d_rows, int32_t *d_out, s3_stream stream) {
    S3_REQUIRE(nq >= 0 && nq < ((int64_t)1 << 31), "s3_cell_locate: bad shape nq=%lld", (long long)nq);
    if (const int rc = check_grid("s3_cell_locate", grid, false, nq > 0)) return rc;
    if (nq == 0) return S3_OK;
    S3_REQUIRE(d_points && d_out, "s3_cell_locate: null array");
    const Lattice lat = make_lattice(*grid);
    hipStream_t st = as_stream(stream);
    if (grid->dim == 2)
        cell_locate_kernel<2><<<grid_for(nq, 256), 256, 0, st>>>(grid->d_starts, grid->d_ends, grid->d_ids, grid->n_cells, lat, d_points, nq, d_rows, d_out);
    else
        cell_locate_kernel<3><<<grid_for(nq, 256), 256, 0, st>>>(grid->d_starts, grid->d_ends, grid->d_ids, grid->n_cells, lat, d_points, nq, d_rows, d_out);
    S3_LAUNCH_CHECK();
    return S3_OK;
}

int s3_cell_sample(int mode, const int32_t *d_cell, int64_t nq, const int32_t *d_rows, const void *d_field, int dtype, int n_comp,
                   int64_t row_len, int64_t in_stride, int64_t n_field_rows, const s3_grid *grid, const double *d_points, double *d_out,
                   int64_t out_stride, s3_stream stream) {
    S3_REQUIRE(mode == S3_SAMPLE_CELL || mode == S3_SAMPLE_LINEAR, "s3_cell_sample: unknown mode %d", mode);
    S3_REQUIRE(nq >= 0 && nq < ((int64_t)1 << 31) && row_len >= 1 && n_field_rows >= 1 && n_field_rows < ((int64_t)1 << 31),
               "s3_cell_sample: bad shape nq=%lld row_len=%lld rows=%lld", (long long)nq, (long long)row_len, (long long)n_field_rows);
    S3_REQUIRE(n_comp >= 1 && n_comp <= 3, "s3_cell_sample: n_comp=%d outside [1,3] (wider fields go in groups of components)", n_comp);
    S3_REQUIRE(dtype == S3_DTYPE_F32 || dtype == S3_DTYPE_F64, "s3_cell_sample: unknown dtype %d", dtype);
    if (in_stride <= 0) in_stride = n_comp * row_len;
    if (out_stride <= 0) out_stride = n_comp * row_len;
    S3_REQUIRE(in_stride >= n_comp * row_len && out_stride >= n_comp * row_len, "s3_cell_sample: in_stride %lld / out_stride %lld shorter than a row",
               (long long)in_stride, (long long)out_stride);
    const bool linear = mode == S3_SAMPLE_LINEAR;
    if (linear)
        if (const int rc = check_grid("s3_cell_sample", grid, true, nq > 0)) return rc;
    if (nq == 0) return S3_OK;
    S3_REQUIRE(d_cell && d_field && d_out && (!linear || d_points), "s3_cell_sample: null array%s", linear ? " (linear mode needs the points)" : "");
    const s3_grid none{};                                                       // S3_SAMPLE_CELL reads no grid
    const s3_grid &gr = linear ? *grid : none;
    const SampleArgs g{d_cell, nq, d_rows, d_field, n_field_rows, row_len, in_stride, d_points, gr.d_centers, gr.d_levels, gr.d_faces, gr.n_cells,
                       gr.width, d_out, out_stride, as_stream(stream)};
    // the width of a lane's piece: every component row of every field row must start on a 16-byte boundary
    return dispatch_rows<WidestRowWidth>(dtype, row_width<WidestRowWidth>(dtype, d_field, row_len, in_stride), [&](auto row) {
        using T = typename decltype(row)::type;
        constexpr int VEC = decltype(row)::vec;
        if (mode == S3_SAMPLE_CELL) return sample_by_comp<T, VEC, 0>(g, n_comp);
        return gr.dim == 2 ? sample_by_comp<T, VEC, 2>(g, n_comp) : sample_by_comp<T, VEC, 3>(g, n_comp);
    });
}

}  // extern "C"
