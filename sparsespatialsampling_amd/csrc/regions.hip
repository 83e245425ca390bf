// Connected regions of thresholded CELL fields: the face-neighbour table of a generated grid, connected-component labels of every
// snapshot of a batch, and a table of the regions (count, volume, centroid, bounding box, integral and extrema of a second field).
// gfx950 only.  No counterpart in the reference, which has no notion of adjacent cells after the grid is written.
//
// Definition: include/s3hip.h states it (neighbour: the same-or-coarser leaf across a face, -1 otherwise; in: lo <= (double) f <= hi,
// NaN out; label: the smallest cell id of the face-connected in-cells; region r of column t: the r-th root by ascending cell id).
//
// Launches:
//     s3_cell_neighbours   one lane per cell: anchor and size as s3_cell_index derives them, per face one morton_key + search_leaf
//     s3_region_label      init (labels[c][t] = in ? c : -1), hook (union-find on the label array itself), flatten: three launches
//     s3_region_count      count[t][c] = (labels[c][t] == c), transposed through LDS; the caller scans it (s3_exclusive_scan)
//     s3_region_emit       keys[t][c] = the region of (c, t) through LDS (out: a sentinel past the last region), stable radix sort by
//                          region (s3_sort_pairs: the cells of a region then stand in ascending id), one group of 16 lanes per region,
//                          then one workgroup per region of more than 1024 cells
//
// The hooking launch (union-find per column; parent of (x, t) is labels[x][t]) and why it is safe on a chip whose L2s are not
// coherent with each other.  INVARIANT: every value ever stored at (x, t) of an in-cell is the id of an in-cell of x's component at
// t and is <= x: the init stores x, a hook stores b < a at the root a (compare-and-swap with the expected value a, so only a root is
// ever hooked and no link is lost), the compression stores a root found by chasing from x (atomicMin).  Therefore
//   * a pointer chase strictly decreases and ends at the latest at cell 0, WHATEVER it reads: a stale value is an older value of the
//     same word, which the invariant covers as well; a value that breaks the invariant (> x, < 0: foreign labels) ends the chase;
//   * a failed compare-and-swap returns a value < a, the retry goes on from it: it strictly decreases too;
//   * "a and b have the same root" is never concluded wrongly from stale data: every value on a chase from a is of a's component;
//   * no lane waits for another lane's store: no flag, no spin, no grid barrier.  Every access to the label array inside the hooking
//     launch is an agent-scope atomic (relaxed load, compare-and-swap, min); the three phases are separate launches, so that what one
//     phase stored is visible to the next by the kernel boundary.
// When the launch has ended every edge of the table with two in-ends joins one tree, and since the larger root always goes under the
// smaller one the root of a tree is its smallest cell: the result is a pure function of the inputs, whatever the schedule was.
//
// Work split: the point slots of csrc/point_slots.h over blocks of REGION_BLOCK cells (hook: of the launch order, s3_spatial_order):
// lanes of a slot take adjacent columns of one cell, so the rows of the field, of the labels and of the 2 dim neighbours are read
// coalesced; nothing is staged in LDS (the 2 dim neighbour ids of a cell are one broadcast load per face).  Element loads: the atomics
// are per element anyway.  A first merge of a workgroup's tile in LDS before the global hooks was not built: DESIGN 5.16 says why.
//
// Floating-point sums of the table (volume, centroid numerator, integral): never atomics.  The cells of a region in ascending id,
// lane k of the 16 of a group takes the cells k, k + 16, .. in that order (volume: a chain of adds; the others: fma chains from 0),
// then the fixed tree lane += lane + 8, + 4, + 2, + 1; a region of more than 1024 cells is left to a second launch, a workgroup per
// region: thread k of 256, the tree of every wavefront, then the four wavefronts in order.  The order is a function of the region's
// size alone: equal inputs give equal bits.  Counts and min / max are exact in any order.
#include "cell_lookup.h"
#include "dev_buf.h"
#include "point_slots.h"
#include "typed_rows.h"

#include <cmath>

namespace s3 {

namespace {

constexpr int REGION_THREADS = POINT_THREADS;
constexpr int REGION_BLOCK = 256;       // cells per workgroup
constexpr int REGION_TILE = 64;         // cells x columns of a transposed tile
constexpr int REGION_GROUP = 16;        // lanes per region of the emit
constexpr int REGION_BIG = 1024;        // a region of more cells gets a workgroup of its own

// ---- neighbours -----------------------------------------------------------------------------------------------------------------
template <int DIM>
__global__ void __launch_bounds__(256)
cell_neighbours_kernel(const uint64_t *__restrict__ starts, const uint64_t *__restrict__ ends, const int32_t *__restrict__ ids,
                       const double *__restrict__ c, const int32_t *__restrict__ level, int64_t n, double width, Lattice lat,
                       int32_t *__restrict__ nbr) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    int32_t *out = nbr + j * (2 * DIM);
#pragma unroll
    for (int f = 0; f < 2 * DIM; ++f) out[f] = -1;
    const int l = level[j];
    if (l < 0 || l > lat.depth) return;                                         // (a grid s3_cell_index would have refused)
    const double h = cell_size(width, l), extent = (double)(1ull << lat.depth);
    uint64_t a[DIM];
#pragma unroll
    for (int ax = 0; ax < DIM; ++ax) {
        const double r = rint(((c[j * DIM + ax] - h / 2) - lat.origin[ax]) / lat.h_min);
        if (!(r >= 0.0 && r < extent)) return;                                  // (NaN and inf fail here, before the conversion)
        a[ax] = (uint64_t)r;
    }
    const uint64_t s = 1ull << (lat.depth - l), side_len = 1ull << lat.depth;
#pragma unroll
    for (int ax = 0; ax < DIM; ++ax) {
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            if (side == 0 ? a[ax] == 0 : a[ax] + s >= side_len) continue;       // the domain edge
            uint64_t q[DIM];
#pragma unroll
            for (int b = 0; b < DIM; ++b) q[b] = a[b];
            q[ax] = side == 0 ? a[ax] - 1 : a[ax] + s;
            const int32_t id = search_leaf(starts, ends, ids, n, morton_key<DIM>(q, lat.depth));
            if (id >= 0 && id < n && level[id] <= l) out[2 * ax + side] = id;
        }
    }
}

// ---- labels ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t parent_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x in the column whose entries are par[cell * stride]: strictly decreasing, so it ends whatever it reads
__device__ __forceinline__ int32_t find_root(const int32_t *par, int64_t stride, int32_t x) {
    for (;;) {
        const int32_t p = parent_load(par + (int64_t)x * stride);
        if (p >= x || p < 0) return x;
        x = p;
    }
}

// joins the trees of a and b: the larger root goes under the smaller one, by a compare-and-swap that hooks a ROOT only
__device__ __forceinline__ void unite(int32_t *par, int64_t stride, int32_t a, int32_t b) {
    for (;;) {
        a = find_root(par, stride, a);
        b = find_root(par, stride, b);
        if (a == b) return;
        if (a < b) {
            const int32_t s = a;
            a = b, b = s;
        }
        int32_t seen = a;
        if (__hip_atomic_compare_exchange_strong(par + (int64_t)a * stride, &seen, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return;
        if (seen >= a || seen < 0) return;                                      // (not under the invariant: foreign labels end here)
        a = seen;                                                               // a has been hooked meanwhile: go on from its parent, < a
    }
}

enum { PHASE_INIT = 0, PHASE_HOOK = 1, PHASE_FLATTEN = 2 };

template <typename T, int PHASE, int DIM>
__global__ void __launch_bounds__(REGION_THREADS)
region_label_kernel(const T *__restrict__ field, int64_t row_len, int64_t in_stride, const int32_t *__restrict__ nbr, int64_t n_cells, double lo,
                    double hi, const int32_t *__restrict__ order, int32_t *labels, int64_t out_stride, int lp, int n_chunks, int64_t n_blocks,
                    int64_t blocks_per_xcd) {
    const int64_t blk = xcd_block(blockIdx.x, blocks_per_xcd);
    if (blk >= n_blocks) return;
    const int64_t p0 = blk * REGION_BLOCK;
    const int n_p = (int)min((int64_t)REGION_BLOCK, n_cells - p0);
    const int t = threadIdx.x, lane = t & (lp - 1), slot = t / lp, pg = REGION_THREADS / lp;

    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        const int64_t col = (int64_t)chunk * lp + lane;
        if (col >= row_len) continue;
        int32_t *par = labels + col;                                            // the column: parent of x at par[x * out_stride]
        for (int pb = slot; pb < n_p; pb += pg) {
            const int64_t c = order ? (int64_t)order[p0 + pb] : p0 + pb;
            if (c < 0 || c >= n_cells) continue;
            if constexpr (PHASE == PHASE_INIT) {
                const double v = (double)row_load<T, 1>(field + c * in_stride + col);
                par[c * out_stride] = v >= lo && v <= hi ? (int32_t)c : -1;     // (both false for NaN)
            } else if constexpr (PHASE == PHASE_HOOK) {
                if (parent_load(par + c * out_stride) < 0) continue;
                bool hooked = false;
#pragma unroll
                for (int f = 0; f < 2 * DIM; ++f) {
                    const int64_t j = nbr[c * (2 * DIM) + f];
                    if (j < 0 || j >= n_cells || j == c) continue;
                    if (parent_load(par + j * out_stride) < 0) continue;
                    unite(par, out_stride, (int32_t)c, (int32_t)j);
                    hooked = true;
                }
                if (hooked) {                                                   // compression: c points at a root found from c (<= its parent)
                    const int32_t r = find_root(par, out_stride, (int32_t)c);
                    if (r < c) __hip_atomic_fetch_min(par + c * out_stride, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            } else {
                // (a launch of its own: the hooks are complete and visible.  A lane may read a word another lane has flattened already:
                // that is a root, the chase ends there)
                if (parent_load(par + c * out_stride) < 0) continue;
                const int32_t r = find_root(par, out_stride, (int32_t)c);
                __hip_atomic_store(par + c * out_stride, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

struct LabelArgs {
    const void *field;
    int64_t row_len, in_stride;
    const int32_t *nbr;
    int64_t n_cells;
    double lo, hi;
    const int32_t *order;
    int32_t *labels;
    int64_t out_stride;
    hipStream_t st;
};

template <typename T, int PHASE, int DIM>
int launch_label(const LabelArgs &g) {
    SlotShape shape;
    if (const int rc = slot_shape("s3_region_label", g.row_len, g.row_len, 0, 0, 0, shape)) return rc;
    const int64_t n_blocks = (g.n_cells + REGION_BLOCK - 1) / REGION_BLOCK;
    const XcdGrid xcd = xcd_grid(n_blocks);
    S3_REQUIRE(xcd.fits(), "s3_region_label: too many cells");
    region_label_kernel<T, PHASE, DIM><<<(unsigned)xcd.grid, REGION_THREADS, 0, g.st>>>(
        static_cast<const T *>(g.field), g.row_len, g.in_stride, g.nbr, g.n_cells, g.lo, g.hi, PHASE == PHASE_HOOK ? g.order : nullptr, g.labels,
        g.out_stride, shape.lanes, (int)shape.n_chunks, n_blocks, xcd.per_xcd);
    S3_LAUNCH_CHECK();
    return S3_OK;
}

// ---- table ----------------------------------------------------------------------------------------------------------------------
// KEYS = false: count[t][c] = (labels[c][t] == c); true: keys[t][c] = the region of (c, t) (sentinel: out, or a label that names no
// root), vals[t][c] = c.  A tile of 64 cells x 64 columns goes through LDS, so that both sides are read and written in runs.
template <bool KEYS>
__global__ void __launch_bounds__(256)
region_transpose_kernel(const int32_t *__restrict__ labels, int64_t row_len, int64_t stride, int64_t n_cells, int32_t *__restrict__ count,
                        const int32_t *__restrict__ scan, uint64_t sentinel, uint64_t *__restrict__ keys, int32_t *__restrict__ vals) {
    __shared__ int32_t s[REGION_TILE][REGION_TILE + 1];
    const int64_t c0 = (int64_t)blockIdx.x * REGION_TILE, t0 = (int64_t)blockIdx.y * REGION_TILE;
    for (int e = threadIdx.x; e < REGION_TILE * REGION_TILE; e += 256) {
        const int i = e / REGION_TILE, j = e % REGION_TILE;
        if (c0 + i < n_cells && t0 + j < row_len) s[i][j] = labels[(c0 + i) * stride + t0 + j];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < REGION_TILE * REGION_TILE; e += 256) {
        const int j = e / REGION_TILE, i = e % REGION_TILE;
        const int64_t c = c0 + i, t = t0 + j;
        if (!(c < n_cells && t < row_len)) continue;
        const int32_t root = s[i][j];
        if constexpr (!KEYS) {
            count[t * n_cells + c] = root == c ? 1 : 0;
        } else {
            uint64_t key = sentinel;
            if (root >= 0 && root < n_cells && labels[(int64_t)root * stride + t] == root) {
                const int32_t r = scan[t * n_cells + root];
                if (r >= 0 && (uint64_t)r < sentinel) key = (uint64_t)r;
            }
            keys[t * n_cells + c] = key;
            vals[t * n_cells + c] = (int32_t)c;
        }
    }
}

__device__ __forceinline__ int64_t lower_bound_key(const uint64_t *__restrict__ keys, int64_t n, uint64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct RegionOut {
    int32_t *label;
    int64_t *n_cells;
    double *volume, *centroid, *lo, *hi, *integral, *g_min, *g_max;
};

struct RegionIn {
    const uint64_t *keys;               // sorted: the region of every pair, the sentinel n_regions last
    const int32_t *vals;                // the cell of every pair
    int64_t n_pairs, n_regions;
    const int32_t *scan;
    int64_t row_len, n_cells;
    const double *centers;
    const int32_t *level;
    double width;
    const void *g;
    int64_t g_stride;
};

// the sums, the box and the extrema of some cells of a region
template <typename T, int DIM, bool WEIGHT>
struct RegionAcc {
    double vol, num[DIM], lo[DIM], hi[DIM], integral, g_min, g_max;

    __device__ __forceinline__ void clear() {
        vol = 0.0, integral = 0.0, g_min = INFINITY, g_max = -INFINITY;
#pragma unroll
        for (int a = 0; a < DIM; ++a) num[a] = 0.0, lo[a] = INFINITY, hi[a] = -INFINITY;
    }
    // the pairs first, first + step, .. below end, in that order; t: the column of the region
    __device__ __forceinline__ void add_cells(const RegionIn &in, int64_t first, int64_t end, int step, int64_t t) {
        for (int64_t i = first; i < end; i += step) {
            const int64_t c = in.vals[i];
            if (c < 0 || c >= in.n_cells) continue;
            const int l = in.level[c];
            if (l < 0 || l > 63) continue;
            const double h = cell_size(in.width, l);
            double v = h * h;
            if constexpr (DIM == 3) v = v * h;
            vol += v;
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                const double x = in.centers[c * DIM + a];
                num[a] = fma(v, x, num[a]);
                lo[a] = fmin(lo[a], x - h / 2);
                hi[a] = fmax(hi[a], x + h / 2);
            }
            if constexpr (WEIGHT) {
                const double gv = (double)static_cast<const T *>(in.g)[c * in.g_stride + t];
                integral = fma(v, gv, integral);
                g_min = fmin(g_min, gv);
                g_max = fmax(g_max, gv);
            }
        }
    }
    __device__ __forceinline__ void merge(const RegionAcc &o) {
        vol += o.vol;
#pragma unroll
        for (int a = 0; a < DIM; ++a) num[a] += o.num[a], lo[a] = fmin(lo[a], o.lo[a]), hi[a] = fmax(hi[a], o.hi[a]);
        if constexpr (WEIGHT) integral += o.integral, g_min = fmin(g_min, o.g_min), g_max = fmax(g_max, o.g_max);
    }
    // lane += lane + d of a group of `width` lanes
    __device__ __forceinline__ void merge_down(int d, int width) {
        RegionAcc o;
        o.vol = __shfl_down(vol, d, width);
#pragma unroll
        for (int a = 0; a < DIM; ++a) o.num[a] = __shfl_down(num[a], d, width), o.lo[a] = __shfl_down(lo[a], d, width), o.hi[a] = __shfl_down(hi[a], d, width);
        o.integral = 0.0, o.g_min = INFINITY, o.g_max = -INFINITY;
        if constexpr (WEIGHT) o.integral = __shfl_down(integral, d, width), o.g_min = __shfl_down(g_min, d, width), o.g_max = __shfl_down(g_max, d, width);
        merge(o);
    }
    __device__ __forceinline__ void write(const RegionIn &in, const RegionOut &out, int64_t r, int64_t begin, int64_t end) const {
        out.label[r] = begin < end ? in.vals[begin] : -1;
        out.n_cells[r] = end - begin;
        out.volume[r] = vol;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            out.centroid[r * DIM + a] = num[a] / vol;
            out.lo[r * DIM + a] = lo[a];
            out.hi[r * DIM + a] = hi[a];
        }
        if constexpr (WEIGHT) out.integral[r] = integral, out.g_min[r] = g_min, out.g_max[r] = g_max;
    }
};

// the pairs [begin, end) of region r and its column
template <bool WEIGHT>
__device__ __forceinline__ void region_range(const RegionIn &in, int64_t r, int64_t &begin, int64_t &end, int64_t &t) {
    begin = lower_bound_key(in.keys, in.n_pairs, (uint64_t)r), end = lower_bound_key(in.keys, in.n_pairs, (uint64_t)r + 1);
    t = 0;
    if constexpr (WEIGHT) {                                                     // the last t whose slice starts at or before r
        int64_t a = 0, b = in.row_len;
        while (a < b) {
            const int64_t mid = (a + b) >> 1;
            if (in.scan[mid * in.n_cells] <= r) a = mid + 1;
            else b = mid;
        }
        t = a > 0 ? a - 1 : 0;
    }
}

// one group of 16 lanes per region; a region of more than REGION_BIG cells is put on the list big[1 ..] (big[0]: their number; the
// order of the list is the schedule's, the result of a region does not depend on it) for region_emit_big_kernel
template <typename T, int DIM, bool WEIGHT>
__global__ void __launch_bounds__(256)
region_emit_kernel(RegionIn in, RegionOut out, int32_t *__restrict__ big) {
    const int64_t r = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / REGION_GROUP;
    if (r >= in.n_regions) return;                                              // (whole groups: 256 is a multiple of 16)
    const int lane = threadIdx.x & (REGION_GROUP - 1);
    int64_t begin, end, t;
    region_range<WEIGHT>(in, r, begin, end, t);
    if (end - begin > REGION_BIG) {
        if (lane == 0) big[1 + atomicAdd(big, 1)] = (int32_t)r;
        return;
    }
    RegionAcc<T, DIM, WEIGHT> acc;
    acc.clear();
    acc.add_cells(in, begin + lane, end, REGION_GROUP, t);
#pragma unroll
    for (int d = REGION_GROUP / 2; d > 0; d >>= 1) acc.merge_down(d, REGION_GROUP);
    if (lane == 0) acc.write(in, out, r, begin, end);
}

// one workgroup per listed region: thread k of 256 takes the cells k, k + 256, .., then lane += lane + 32, .. + 1 in every wavefront,
// then wavefront 0 += 1, += 2, += 3
template <typename T, int DIM, bool WEIGHT>
__global__ void __launch_bounds__(256)
region_emit_big_kernel(RegionIn in, RegionOut out, const int32_t *__restrict__ big) {
    __shared__ RegionAcc<T, DIM, WEIGHT> s_acc[4];
    const int n_big = big[0];
    for (int k = blockIdx.x; k < n_big; k += gridDim.x) {
        const int64_t r = big[1 + k];
        int64_t begin, end, t;
        region_range<WEIGHT>(in, r, begin, end, t);
        RegionAcc<T, DIM, WEIGHT> acc;
        acc.clear();
        acc.add_cells(in, begin + threadIdx.x, end, 256, t);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) acc.merge_down(d, 64);
        __syncthreads();                                                        // the previous region's partial sums have been read
        if ((threadIdx.x & 63) == 0) s_acc[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; ++w) acc.merge(s_acc[w]);
            acc.write(in, out, r, begin, end);
        }
    }
}

template <typename T, int DIM, bool WEIGHT>
void launch_emit(const RegionIn &in, const RegionOut &out, int32_t *big, hipStream_t st) {
    region_emit_kernel<T, DIM, WEIGHT><<<grid_for(in.n_regions * REGION_GROUP, 256), 256, 0, st>>>(in, out, big);
    region_emit_big_kernel<T, DIM, WEIGHT><<<grid_for(in.n_pairs / REGION_BIG + 1, 1, 2048), 256, 0, st>>>(in, out, big);
}

int label_shape(const char *who, int64_t row_len, int64_t stride, int64_t n_cells) {
    S3_REQUIRE(row_len >= 1 && n_cells >= 1 && n_cells < ((int64_t)1 << 31), "%s: bad shape row_len=%lld cells=%lld", who, (long long)row_len,
               (long long)n_cells);
    S3_REQUIRE(stride >= row_len, "%s: stride %lld shorter than a row", who, (long long)stride);
    S3_REQUIRE((double)n_cells * (double)row_len < 2147483647.0, "%s: %lld cells x %lld snapshots are 2^31 entries or more: split the batch", who,
               (long long)n_cells, (long long)row_len);
    S3_REQUIRE((row_len + REGION_TILE - 1) / REGION_TILE <= 65535, "%s: row_len %lld too long", who, (long long)row_len);
    return S3_OK;
}

}  // namespace

}  // namespace s3

using namespace s3;

extern "C" {

int s3_cell_neighbours(const s3_grid *grid, int32_t *d_nbr, s3_stream stream) {
    if (const int rc = check_grid("s3_cell_neighbours", grid, false, true)) return rc;
    S3_REQUIRE(d_nbr, "s3_cell_neighbours: null array");
    const Lattice lat = make_lattice(*grid);
    hipStream_t st = as_stream(stream);
    const int64_t n = grid->n_cells;
    if (grid->dim == 2)
        cell_neighbours_kernel<2><<<grid_for(n, 256), 256, 0, st>>>(grid->d_starts, grid->d_ends, grid->d_ids, grid->d_centers, grid->d_levels, n,
                                                                   grid->width, lat, d_nbr);
    else
        cell_neighbours_kernel<3><<<grid_for(n, 256), 256, 0, st>>>(grid->d_starts, grid->d_ends, grid->d_ids, grid->d_centers, grid->d_levels, n,
                                                                   grid->width, lat, d_nbr);
    S3_LAUNCH_CHECK();
    return S3_OK;
}

int s3_region_label(const void *d_field, int dtype, int64_t row_len, int64_t in_stride, const int32_t *d_nbr, int64_t n_cells, int dim, double lo,
                    double hi, const int32_t *d_order, int phases, int32_t *d_labels, int64_t out_stride, s3_stream stream) {
    S3_REQUIRE(dim == 2 || dim == 3, "s3_region_label: dim=%d", dim);
    S3_REQUIRE(dtype == S3_DTYPE_F32 || dtype == S3_DTYPE_F64, "s3_region_label: unknown dtype %d", dtype);
    S3_REQUIRE(phases >= 1 && phases <= S3_REGION_ALL, "s3_region_label: phases=%d", phases);
    S3_REQUIRE(!(std::isnan(lo) || std::isnan(hi)), "s3_region_label: the bounds must not be NaN");
    if (in_stride <= 0) in_stride = row_len;
    if (out_stride <= 0) out_stride = row_len;
    if (const int rc = label_shape("s3_region_label", row_len, out_stride, n_cells)) return rc;
    S3_REQUIRE(in_stride >= row_len, "s3_region_label: in_stride %lld shorter than a row", (long long)in_stride);
    S3_REQUIRE(d_labels && (!(phases & S3_REGION_INIT) || d_field) && (!(phases & S3_REGION_HOOK) || d_nbr), "s3_region_label: null array");
    const LabelArgs g{d_field, row_len, in_stride, d_nbr, n_cells, lo, hi, d_order, d_labels, out_stride, as_stream(stream)};
    return dispatch_rows<ScalarRows>(dtype, 1, [&](auto row) {
        using T = typename decltype(row)::type;
        if (phases & S3_REGION_INIT)
            if (const int rc = launch_label<T, PHASE_INIT, 2>(g)) return rc;
        if (phases & S3_REGION_HOOK)
            if (const int rc = dim == 2 ? launch_label<T, PHASE_HOOK, 2>(g) : launch_label<T, PHASE_HOOK, 3>(g)) return rc;
        if (phases & S3_REGION_FLATTEN)
            if (const int rc = launch_label<T, PHASE_FLATTEN, 2>(g)) return rc;
        return (int)S3_OK;
    });
}

int s3_region_count(const int32_t *d_labels, int64_t row_len, int64_t label_stride, int64_t n_cells, int32_t *d_count, s3_stream stream) {
    if (label_stride <= 0) label_stride = row_len;
    if (const int rc = label_shape("s3_region_count", row_len, label_stride, n_cells)) return rc;
    S3_REQUIRE(d_labels && d_count, "s3_region_count: null array");
    const dim3 tiles((unsigned)((n_cells + REGION_TILE - 1) / REGION_TILE), (unsigned)((row_len + REGION_TILE - 1) / REGION_TILE));
    region_transpose_kernel<false><<<tiles, 256, 0, as_stream(stream)>>>(d_labels, row_len, label_stride, n_cells, d_count, nullptr, 0, nullptr, nullptr);
    S3_LAUNCH_CHECK();
    return S3_OK;
}

int s3_region_emit(const int32_t *d_labels, int64_t row_len, int64_t label_stride, const s3_grid *grid, const int32_t *d_offset, int64_t n_regions,
                   const void *d_weight, int dtype, int64_t weight_stride, int32_t *d_label, int64_t *d_n_cells, double *d_volume,
                   double *d_centroid, double *d_lo, double *d_hi, double *d_integral, double *d_g_min, double *d_g_max, s3_stream stream) {
    if (const int rc = check_grid("s3_region_emit", grid, false, true)) return rc;
    if (label_stride <= 0) label_stride = row_len;
    if (const int rc = label_shape("s3_region_emit", row_len, label_stride, grid->n_cells)) return rc;
    const int64_t n_cells = grid->n_cells, n_pairs = n_cells * row_len;
    S3_REQUIRE(n_regions >= 0 && n_regions <= n_pairs, "s3_region_emit: %lld regions of %lld entries", (long long)n_regions, (long long)n_pairs);
    if (n_regions == 0) return S3_OK;
    S3_REQUIRE(d_labels && d_offset && d_label && d_n_cells && d_volume && d_centroid && d_lo && d_hi, "s3_region_emit: null array");
    const bool weight = d_weight != nullptr;
    if (weight) {
        S3_REQUIRE(dtype == S3_DTYPE_F32 || dtype == S3_DTYPE_F64, "s3_region_emit: unknown dtype %d", dtype);
        if (weight_stride <= 0) weight_stride = row_len;
        S3_REQUIRE(weight_stride >= row_len, "s3_region_emit: weight_stride %lld shorter than a row", (long long)weight_stride);
        S3_REQUIRE(d_integral && d_g_min && d_g_max, "s3_region_emit: null array");
    }
    hipStream_t st = as_stream(stream);
    DevBuf<uint64_t> keys;
    DevBuf<int32_t> vals;
    S3_HIP_CHECK(keys.alloc((size_t)n_pairs));
    S3_HIP_CHECK(vals.alloc((size_t)n_pairs));
    const dim3 tiles((unsigned)((n_cells + REGION_TILE - 1) / REGION_TILE), (unsigned)((row_len + REGION_TILE - 1) / REGION_TILE));
    region_transpose_kernel<true><<<tiles, 256, 0, st>>>(d_labels, row_len, label_stride, n_cells, nullptr, d_offset, (uint64_t)n_regions, keys, vals);
    S3_LAUNCH_CHECK();
    int bits = 1;
    while (bits < 63 && ((uint64_t)n_regions >> bits) != 0) ++bits;             // the sentinel n_regions is the largest key
    if (const int rc = s3_sort_pairs(keys, vals, n_pairs, bits, stream)) return rc;
    const RegionOut out{d_label, d_n_cells, d_volume, d_centroid, d_lo, d_hi, d_integral, d_g_min, d_g_max};
    const RegionIn in{keys, vals, n_pairs, n_regions, d_offset, row_len, n_cells, grid->d_centers, grid->d_levels, grid->width, d_weight, weight_stride};
    DevBuf<int32_t> big;                                                        // [0]: how many, then the regions of more than REGION_BIG cells
    S3_HIP_CHECK(big.alloc((size_t)(n_pairs / REGION_BIG + 2)));
    S3_HIP_CHECK(hipMemsetAsync(big, 0, sizeof(int32_t), st));
    const int dim = grid->dim;
    if (!weight) {
        if (dim == 2) launch_emit<float, 2, false>(in, out, big, st);
        else launch_emit<float, 3, false>(in, out, big, st);
    } else if (dtype == S3_DTYPE_F32) {
        if (dim == 2) launch_emit<float, 2, true>(in, out, big, st);
        else launch_emit<float, 3, true>(in, out, big, st);
    } else {
        if (dim == 2) launch_emit<double, 2, true>(in, out, big, st);
        else launch_emit<double, 3, true>(in, out, big, st);
    }
    S3_LAUNCH_CHECK();
    S3_HIP_CHECK(hipStreamSynchronize(st));                                     // the scratch arrays go away after it
    return S3_OK;
}

}  // extern "C"
