// The overlap table of two label arrays of one grid (include/s3overlap.h states the definitions): which regions of A share cells with
// which regions of B, per column, with the shared cells counted and their volume summed in units of the finest cell.  With A and B
// two windows of one labelling, shifted by one snapshot, these are the links regions are tracked by.  gfx950 only.  No counterpart in
// the reference.
//
// Launches (count -> scan -> emit -> sort -> heads -> scan -> reduce; the caller owns every array and runs the scans and the sort):
//     s3_overlap_count     flag[t][c] = c is in both at t, transposed through LDS
//     s3_overlap_emit      one (key, cell) per flagged (c, t) at its scanned position through the same tile; or, for the second of two
//                          sort passes, the keys of the pairs rewritten in place
//     s3_overlap_heads     head[j] = the sorted pair j starts a new (t, a, b)
//     s3_overlap_reduce    units per edge by wavefront sums and integer atomics, then one lane per edge for the five output arrays
//
// Work split of count and emit: a tile of OVERLAP_TILE cells x LP columns, LP the lanes per point slot of csrc/point_slots.h for the row
// (4 .. 64).  Reading, LP adjacent lanes take adjacent columns of one cell: both label rows and the two root rows A[a][..], B[b][..] are
// read in runs (a region that persists keeps its root, so the lanes of a slot mostly gather from one row).  Writing, 64 adjacent lanes
// take adjacent cells of one column of the snapshot-major arrays.  The tile of regions.hip is the same with LP fixed at 64; at 25
// columns it would leave 39 of 64 lanes idle while reading.
//
// Why the units may be summed with atomics: they are integers (2^(dim (depth - level)), the sum over disjoint leaves at most 2^63), so
// every order gives the same bits.  A wavefront walks OVERLAP_CHUNKS x 64 consecutive sorted pairs, sums each run of one edge with a
// segmented shuffle scan, carries the run that crosses a chunk boundary in registers and issues one 64-bit atomic add per run it ends:
// an edge of a million cells costs about a thousand atomics on its word, spread over as many wavefronts, and no lane walks a run.
// Nothing waits for an atomic's result; the counts come from the positions of the heads, not from atomics.
//
// Every index read from an array is checked before it is followed (cells, levels, columns, scanned positions, edge numbers): arrays
// that do not belong together give wrong numbers, never an access outside an allocation.
#include "s3overlap.h"

#include "cell_lookup.h"
#include "point_slots.h"

namespace s3 {

namespace {

constexpr int OVERLAP_TILE = 64;        // cells of a transposed tile
constexpr int OVERLAP_CHUNKS = 16;      // chunks of 64 sorted pairs a wavefront of the units launch walks

struct Labels {
    const int32_t *a, *b;
    int64_t a_stride, b_stride, row_len, n_cells;
};

// the bits of the largest value below n
inline int bits_below(int64_t n) {
    int bits = 0;
    while (bits < 63 && ((uint64_t)(n - 1) >> bits) != 0) ++bits;
    return bits;
}
inline int cell_bits(int64_t n_cells) { return n_cells > 2 ? bits_below(n_cells) : 1; }

__device__ __forceinline__ bool names_root(const int32_t *__restrict__ x, int64_t stride, int64_t n_cells, int64_t t, int32_t v) {
    return v >= 0 && v < n_cells && x[(int64_t)v * stride + t] == v;
}

// PASS < 0: count[t][c] = in both; otherwise the pairs of S3_OVERLAP_ONE_KEY / S3_OVERLAP_BY_B at their scanned positions
template <int PASS>
__global__ void __launch_bounds__(256)
overlap_tile_kernel(Labels in, int lp, int32_t *__restrict__ count, const int32_t *__restrict__ scan, int64_t n_pairs, int w, uint64_t *__restrict__ keys,
                    int32_t *__restrict__ vals) {
    __shared__ int32_t sa[OVERLAP_TILE][64 + 1], sb[OVERLAP_TILE][64 + 1];
    const int64_t c0 = (int64_t)blockIdx.x * OVERLAP_TILE, t0 = (int64_t)blockIdx.y * lp;
    for (int e = threadIdx.x; e < OVERLAP_TILE * lp; e += 256) {
        const int i = e / lp, j = e % lp;
        const int64_t c = c0 + i, t = t0 + j;
        int32_t a = -1, b = -1;
        if (c < in.n_cells && t < in.row_len) {
            a = in.a[c * in.a_stride + t], b = in.b[c * in.b_stride + t];
            if (!(names_root(in.a, in.a_stride, in.n_cells, t, a) && names_root(in.b, in.b_stride, in.n_cells, t, b))) a = -1;
        }
        sa[i][j] = a, sb[i][j] = b;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < OVERLAP_TILE * lp; e += 256) {
        const int j = e / OVERLAP_TILE, i = e % OVERLAP_TILE;
        const int64_t c = c0 + i, t = t0 + j;
        if (!(c < in.n_cells && t < in.row_len)) continue;
        const int32_t a = sa[i][j], b = sb[i][j];
        if constexpr (PASS < 0) {
            count[t * in.n_cells + c] = a >= 0 ? 1 : 0;
        } else {
            if (a < 0) continue;
            const int64_t pos = scan[t * in.n_cells + c];
            if (pos < 0 || pos >= n_pairs) continue;                            // (a scan of other labels)
            keys[pos] = PASS == S3_OVERLAP_ONE_KEY ? ((uint64_t)t << (2 * w)) | ((uint64_t)a << w) | (uint64_t)b : ((uint64_t)t << w) | (uint64_t)b;
            vals[pos] = (int32_t)c;
        }
    }
}

// the second of two passes: the key t << w | b of every pair becomes t << w | a
__global__ void __launch_bounds__(256)
overlap_rekey_kernel(Labels in, int64_t n_pairs, int w, uint64_t *__restrict__ keys, const int32_t *__restrict__ vals) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= n_pairs) return;
    const int64_t t = (int64_t)(keys[j] >> w), c = vals[j];
    if (t >= in.row_len || c < 0 || c >= in.n_cells) return;                    // (pairs of another batch: left as they are)
    const int32_t a = in.a[c * in.a_stride + t];
    if (a >= 0 && a < in.n_cells) keys[j] = ((uint64_t)t << w) | (uint64_t)a;
}

struct Pairs {
    const uint64_t *keys;
    const int32_t *vals;
    int64_t n_pairs;
    int two_pass, w;
    const int32_t *b;                   // two_pass: where b is read
    int64_t b_stride, row_len, n_cells;
};

// (t, a) packed and b of the sorted pair j; false where the pair does not belong to these arrays
__device__ __forceinline__ bool pair_of(const Pairs &p, int64_t j, uint64_t &ta, int32_t &b) {
    const uint64_t key = p.keys[j];
    if (!p.two_pass) {
        ta = key >> p.w, b = (int32_t)(key & ((1ull << p.w) - 1ull));
        return true;
    }
    ta = key;
    const int64_t t = (int64_t)(key >> p.w), c = p.vals[j];
    if (t >= p.row_len || c < 0 || c >= p.n_cells) return false;
    b = p.b[c * p.b_stride + t];
    return true;
}

__global__ void __launch_bounds__(256)
overlap_heads_kernel(Pairs p, int32_t *__restrict__ head) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= p.n_pairs) return;
    uint64_t ta = 0, ta0 = 0;
    int32_t b = -1, b0 = -1;
    const bool ok = pair_of(p, j, ta, b);
    bool first = j == 0 || !ok;
    if (!first) first = !pair_of(p, j - 1, ta0, b0) || ta0 != ta || b0 != b;
    head[j] = first ? 1 : 0;
}

// the units of every pair added to its edge: see the head of this file
template <int DIM>
__global__ void __launch_bounds__(256)
overlap_units_kernel(const int32_t *__restrict__ vals, int64_t n_pairs, const int32_t *__restrict__ edge, int64_t n_edges, const int32_t *__restrict__ level,
                     int64_t n_cells, int depth, unsigned long long *__restrict__ units) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t base = wave * (64 * OVERLAP_CHUNKS);
    unsigned long long carry = 0;
    int32_t carry_e = -1;
    for (int k = 0; k < OVERLAP_CHUNKS; ++k) {
        if (base + (int64_t)k * 64 >= n_pairs) break;                           // (the same for every lane of the wavefront)
        const int64_t j = base + (int64_t)k * 64 + lane;
        int32_t e = -2;
        unsigned long long u = 0;
        if (j < n_pairs) {
            e = edge[j + 1] - 1;
            if (e < 0 || e >= n_edges) e = -2;
            const int64_t c = vals[j];
            if (e >= 0 && c >= 0 && c < n_cells) {
                const int l = level[c];
                if (l >= 0 && l <= depth) u = 1ull << (DIM * (depth - l));
            }
        }
        // inclusive sums inside every run of equal e (the runs are contiguous: the pairs are sorted)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long u_up = __shfl_up(u, d, 64);
            const int32_t e_up = __shfl_up(e, d, 64);
            if (lane >= d && e_up == e) u += u_up;
        }
        const int32_t e_first = __shfl(e, 0, 64);
        if (carry_e >= 0) {
            if (e == carry_e) u += carry;                                       // the first run goes on from the last chunk
            else if (lane == 0 && e_first != carry_e) atomicAdd(units + carry_e, carry);
        }
        const int32_t e_next = __shfl_down(e, 1, 64);
        if (e >= 0 && lane != 63 && e_next != e) atomicAdd(units + e, u);       // the last lane of a run that ends inside the chunk
        carry = __shfl(u, 63, 64), carry_e = __shfl(e, 63, 64);
    }
    if (lane == 0 && carry_e >= 0) atomicAdd(units + carry_e, carry);
}

// the first j in [0, n] whose edge[j] >= value (edge: the scanned heads, ascending, n + 1 entries)
__device__ __forceinline__ int64_t first_at_least(const int32_t *__restrict__ edge, int64_t n, int64_t value) {
    int64_t lo = 0, hi = n + 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (edge[mid] < value) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one lane per edge: its pairs are those with edge[j + 1] - 1 == e, that is j + 1 in [first(e + 1), first(e + 2))
__global__ void __launch_bounds__(256)
overlap_edges_kernel(Pairs p, const int32_t *__restrict__ edge, int64_t n_edges, double hd, int32_t *__restrict__ src, int32_t *__restrict__ dst,
                     int64_t *__restrict__ n_cells, const unsigned long long *__restrict__ units, double *__restrict__ volume) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e >= n_edges) return;
    const int64_t begin = first_at_least(edge, p.n_pairs, e + 1) - 1, end = first_at_least(edge, p.n_pairs, e + 2) - 1;
    uint64_t ta = 0;
    int32_t b = -1;
    const bool ok = begin >= 0 && begin < p.n_pairs && pair_of(p, begin, ta, b);
    src[e] = ok ? (int32_t)(ta & ((1ull << p.w) - 1ull)) : -1;
    dst[e] = ok ? b : -1;
    n_cells[e] = ok ? end - begin : 0;
    volume[e] = (double)units[e] * hd;
}

int overlap_shape(const char *who, const s3_grid *grid, int64_t row_len, int64_t &a_stride, int64_t &b_stride) {
    if (const int rc = check_grid(who, grid, false, true)) return rc;
    const int64_t n_cells = grid->n_cells;
    S3_REQUIRE(row_len >= 1, "%s: row_len=%lld", who, (long long)row_len);
    S3_REQUIRE((double)n_cells * (double)row_len < 2147483647.0, "%s: %lld cells x %lld columns are 2^31 entries or more: split the batch", who,
               (long long)n_cells, (long long)row_len);
    if (a_stride <= 0) a_stride = row_len;
    if (b_stride <= 0) b_stride = row_len;
    S3_REQUIRE(a_stride >= row_len && b_stride >= row_len, "%s: a stride (%lld, %lld) shorter than a row of %lld", who, (long long)a_stride,
               (long long)b_stride, (long long)row_len);
    return S3_OK;
}

int tile_launch(const char *who, const Labels &in, int &lp, dim3 &tiles) {
    SlotShape shape;
    if (const int rc = slot_shape(who, in.row_len, in.row_len, 0, 0, 0, shape)) return rc;
    lp = shape.lanes;
    const int64_t column_tiles = (in.row_len + lp - 1) / lp;
    S3_REQUIRE(column_tiles <= 65535, "%s: row_len %lld too long", who, (long long)in.row_len);
    tiles = dim3((unsigned)((in.n_cells + OVERLAP_TILE - 1) / OVERLAP_TILE), (unsigned)column_tiles);
    return S3_OK;
}

int pairs_of(const char *who, const s3_grid *grid, const uint64_t *d_keys, const int32_t *d_vals, int64_t n_pairs, int two_pass, const int32_t *d_b,
             int64_t b_stride, int64_t row_len, Pairs &p) {
    int64_t a_stride = 0;
    if (const int rc = overlap_shape(who, grid, row_len, a_stride, b_stride)) return rc;
    S3_REQUIRE(n_pairs >= 0 && n_pairs <= grid->n_cells * row_len, "%s: %lld pairs of %lld entries", who, (long long)n_pairs,
               (long long)(grid->n_cells * row_len));
    S3_REQUIRE(n_pairs == 0 || (d_keys && d_vals && (!two_pass || d_b)), "%s: null array", who);
    p = Pairs{d_keys, d_vals, n_pairs, two_pass ? 1 : 0, cell_bits(grid->n_cells), d_b, b_stride, row_len, grid->n_cells};
    return S3_OK;
}

}  // namespace

}  // namespace s3

using namespace s3;

extern "C" {

int s3_overlap_count(const s3_grid *grid, const int32_t *d_a, int64_t a_stride, const int32_t *d_b, int64_t b_stride, int64_t row_len, int32_t *d_count,
                     s3_stream stream) {
    if (const int rc = overlap_shape("s3_overlap_count", grid, row_len, a_stride, b_stride)) return rc;
    S3_REQUIRE(d_a && d_b && d_count, "s3_overlap_count: null array");
    const Labels in{d_a, d_b, a_stride, b_stride, row_len, grid->n_cells};
    int lp;
    dim3 tiles;
    if (const int rc = tile_launch("s3_overlap_count", in, lp, tiles)) return rc;
    overlap_tile_kernel<-1><<<tiles, 256, 0, as_stream(stream)>>>(in, lp, d_count, nullptr, 0, 0, nullptr, nullptr);
    S3_LAUNCH_CHECK();
    return S3_OK;
}

int s3_overlap_emit(const s3_grid *grid, const int32_t *d_a, int64_t a_stride, const int32_t *d_b, int64_t b_stride, int64_t row_len, const int32_t *d_scan,
                    int64_t n_pairs, int pass, uint64_t *d_keys, int32_t *d_vals, s3_stream stream) {
    if (const int rc = overlap_shape("s3_overlap_emit", grid, row_len, a_stride, b_stride)) return rc;
    const int64_t n_cells = grid->n_cells;
    S3_REQUIRE(pass == S3_OVERLAP_ONE_KEY || pass == S3_OVERLAP_BY_B || pass == S3_OVERLAP_BY_TA, "s3_overlap_emit: pass=%d", pass);
    S3_REQUIRE(n_pairs >= 0 && n_pairs <= n_cells * row_len, "s3_overlap_emit: %lld pairs of %lld entries", (long long)n_pairs, (long long)(n_cells * row_len));
    const int w = cell_bits(n_cells), tb = bits_below(row_len);
    S3_REQUIRE(tb + (pass == S3_OVERLAP_ONE_KEY ? 2 : 1) * w <= 64, "s3_overlap_emit: (t, a, b) of %lld columns and %lld cells does not fit one key: two passes",
               (long long)row_len, (long long)n_cells);
    if (n_pairs == 0) return S3_OK;
    S3_REQUIRE(d_a && d_b && d_keys && d_vals && (pass == S3_OVERLAP_BY_TA || d_scan), "s3_overlap_emit: null array");
    const Labels in{d_a, d_b, a_stride, b_stride, row_len, n_cells};
    hipStream_t st = as_stream(stream);
    if (pass == S3_OVERLAP_BY_TA) {
        overlap_rekey_kernel<<<grid_for(n_pairs, 256), 256, 0, st>>>(in, n_pairs, w, d_keys, d_vals);
    } else {
        int lp;
        dim3 tiles;
        if (const int rc = tile_launch("s3_overlap_emit", in, lp, tiles)) return rc;
        if (pass == S3_OVERLAP_ONE_KEY) overlap_tile_kernel<S3_OVERLAP_ONE_KEY><<<tiles, 256, 0, st>>>(in, lp, nullptr, d_scan, n_pairs, w, d_keys, d_vals);
        else overlap_tile_kernel<S3_OVERLAP_BY_B><<<tiles, 256, 0, st>>>(in, lp, nullptr, d_scan, n_pairs, w, d_keys, d_vals);
    }
    S3_LAUNCH_CHECK();
    return S3_OK;
}

int s3_overlap_heads(const s3_grid *grid, const uint64_t *d_keys, const int32_t *d_vals, int64_t n_pairs, int two_pass, const int32_t *d_b, int64_t b_stride,
                     int64_t row_len, int32_t *d_head, s3_stream stream) {
    Pairs p;
    if (const int rc = pairs_of("s3_overlap_heads", grid, d_keys, d_vals, n_pairs, two_pass, d_b, b_stride, row_len, p)) return rc;
    if (n_pairs == 0) return S3_OK;
    S3_REQUIRE(d_head, "s3_overlap_heads: null array");
    overlap_heads_kernel<<<grid_for(n_pairs, 256), 256, 0, as_stream(stream)>>>(p, d_head);
    S3_LAUNCH_CHECK();
    return S3_OK;
}

int s3_overlap_reduce(const s3_grid *grid, const uint64_t *d_keys, const int32_t *d_vals, int64_t n_pairs, int two_pass, const int32_t *d_b, int64_t b_stride,
                      int64_t row_len, const int32_t *d_edge, int64_t n_edges, int32_t *d_src, int32_t *d_dst, int64_t *d_n_cells, uint64_t *d_units,
                      double *d_volume, s3_stream stream) {
    Pairs p;
    if (const int rc = pairs_of("s3_overlap_reduce", grid, d_keys, d_vals, n_pairs, two_pass, d_b, b_stride, row_len, p)) return rc;
    S3_REQUIRE(n_edges >= 0 && n_edges <= n_pairs, "s3_overlap_reduce: %lld edges of %lld pairs", (long long)n_edges, (long long)n_pairs);
    if (n_edges == 0) return S3_OK;
    S3_REQUIRE(d_edge && d_src && d_dst && d_n_cells && d_units && d_volume, "s3_overlap_reduce: null array");
    hipStream_t st = as_stream(stream);
    const double h = grid->h_min;
    const double hd = grid->dim == 2 ? h * h : (h * h) * h;
    unsigned long long *units = reinterpret_cast<unsigned long long *>(d_units);
    S3_HIP_CHECK(hipMemsetAsync(d_units, 0, sizeof(uint64_t) * (size_t)n_edges, st));
    const unsigned blocks = grid_for(n_pairs, 4 * 64 * OVERLAP_CHUNKS);         // four wavefronts of OVERLAP_CHUNKS chunks
    if (grid->dim == 2) overlap_units_kernel<2><<<blocks, 256, 0, st>>>(d_vals, n_pairs, d_edge, n_edges, grid->d_levels, grid->n_cells, grid->depth, units);
    else overlap_units_kernel<3><<<blocks, 256, 0, st>>>(d_vals, n_pairs, d_edge, n_edges, grid->d_levels, grid->n_cells, grid->depth, units);
    overlap_edges_kernel<<<grid_for(n_edges, 256), 256, 0, st>>>(p, d_edge, n_edges, hd, d_src, d_dst, d_n_cells, units, d_volume);
    S3_LAUNCH_CHECK();
    return S3_OK;
}

}  // extern "C"
