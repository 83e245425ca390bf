// Line-of-sight integrals of a grid field: the integral of a cell field, or of the multilinear blend of a node field, along straight
// rays through a generated grid, ray-marched from leaf to leaf on the integer lattice.  gfx950 only.  No counterpart in the reference.
//
// Definition (include/s3rays.h is normative; restated here).  Plain f64, -ffp-contract=off, fma where it is written; max / min are the
// comparisons `b > a ? b : a` / `b < a ? b : a` with a the value held so far.
//   ray       x(t) = o + t d; BAD_RAY: a component not finite, or d zero.  |d| = sqrt of the squares summed in axis order.  An axis
//             with d_a == 0 is fixed: no parameter, x_a = o_a, lattice index floor((o_a - origin_a) / h_min) with the range test before
//             the conversion (lattice_index of cell_lookup.h); out of range: MISSED.  Half-open: a ray in a face plane belongs to the
//             upper cells.
//   planes    tau_a(j) = (fma((double) j, h_min, origin_a) - o_a) / d_a: from the lattice, never from cell centres, so a shared face
//             has one parameter and chords telescope.
//   block     a leaf (morton_key, search_leaf's upper bound and range test; s = L - level) or, where the key k falls into a gap
//             [g0, g1) of the sorted ranges, the empty block of the largest s with [k & ~(2^(dim s) - 1), + 2^(dim s)) inside the gap;
//             anchor a = (i >> s) << s.
//   chord     t_in = max(t_min, tau_a(near)), t_out = min tau_a(far) over the moving axes in axis order, exit axis e the lowest that
//             attains t_out; len = min(t_out, t_max) - t_in; a leaf with len > 0 is a segment.
//   segment   CELL: acc = fma((double) field[id][c][t], len, acc).  LINEAR: half = len / 2, mid = t_in + half, g = half *
//             0.57735026918962576, b_1 and b_2 the blend of cell_lookup.h in that leaf at x(mid - g) and x(mid + g) (x_a = fma(t_g,
//             d_a, o_a)), acc = fma(half, b_1 + b_2, acc).  lenacc += len.
//   start     the domain block (0, L); len not > 0: MISSED.  First index floor((fma(t_in, d_a, o_a) - origin_a) / h_min) clamped to
//             [0, 2^L - 1]; exactly 0 or 2^L - 1 on the axes whose near plane gave t_in.
//   step      ends when t_out >= t_max; else i_e = the far plane's index (d_e > 0) or that minus one (d_e < 0), ending when it leaves
//             [0, 2^L); the other moving axes floor the point at t_out, clamped into the block just left.  max_steps steps without an
//             end: TRUNCATED.
//   broken    a leaf with an id, a level or (LINEAR) a corner out of range: nothing is loaded through it, the row becomes NaN, the
//             status BROKEN, the walk goes on.
//   outputs   out = |d| * acc, length = |d| * lenacc, segments, status.
//
// Regime.  A lane runs a dependent chain: per block one binary search (log2(n_cells) dependent 8-byte loads), the leaf's level (and in
// linear mode its centre and 2^d corner ids), then n_comp (x 2^d) field loads and a few dozen f64 operations.  Latency bound, like
// trace_kernel: what hides it is the number of rays in flight.  No LDS, no atomics, no scratch.
//
// Work split.  One lane per (ray, column), the column running fastest: lane p = (launch slot, column) = (p / T, p % T).  The lanes of
// a wavefront that share a ray walk identically (no divergence) and their loads of field[id][c][t ..] coalesce; with short rows a
// wavefront holds the neighbouring rays of d_order.  Every lane of a ray computes the same length, segments and status; the lane of
// column 0 writes them.  A finished lane idles until its wavefront is through.
#include "s3rays.h"

#include "cell_lookup.h"
#include "typed_rows.h"

#include <cmath>

namespace s3 {

namespace {

constexpr int RAY_THREADS = 256;
constexpr double GAUSS2 = 0.57735026918962576;

struct RayArgs {
    const uint64_t *starts, *ends;
    const int32_t *ids;
    int64_t n_cells;
    Lattice lat;
    const double *centers;
    const int32_t *level;
    double width;
    const int32_t *faces;
    const void *field;
    int n_comp;
    int64_t row_len, in_stride, n_field_rows;
    const double *origins, *dirs;
    int64_t n_rays;
    const int32_t *order;
    double t_min, t_max;
    int64_t max_steps;
    double *out;
    int64_t out_stride;
    double *length;
    int32_t *segments, *status;
};

template <int DIM>
struct Ray {
    double o[DIM], d[DIM];
};

// the parameter of lattice plane j of the moving axis a
template <int DIM>
__device__ __forceinline__ double plane_tau(const Lattice &lat, const Ray<DIM> &r, int a, uint64_t j) {
    return (fma((double)j, lat.h_min, lat.origin[a]) - r.o[a]) / r.d[a];
}

// the chord of the block (anchor, s) before the clamp to t_max: t_in from t_min, t_out and the exit axis
template <int DIM>
__device__ __forceinline__ void block_chord(const Lattice &lat, const Ray<DIM> &r, const uint64_t (&anchor)[DIM], int s, double t_min,
                                            double &t_in, double &t_out, int &e) {
    t_in = t_min, t_out = 0.0, e = -1;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        if (r.d[a] == 0.0) continue;
        const uint64_t lo = anchor[a], hi = anchor[a] + (1ull << s);
        const double tn = plane_tau<DIM>(lat, r, a, r.d[a] > 0.0 ? lo : hi), tf = plane_tau<DIM>(lat, r, a, r.d[a] > 0.0 ? hi : lo);
        if (tn > t_in) t_in = tn;
        if (e < 0 || tf < t_out) t_out = tf, e = a;
    }
}

// floor((fma(t, d_a, o_a) - origin_a) / h_min) clamped into [lo, hi] (NaN: lo)
template <int DIM>
__device__ __forceinline__ uint64_t point_index(const Lattice &lat, const Ray<DIM> &r, int a, double t, uint64_t lo, uint64_t hi) {
    const double q = floor((fma(t, r.d[a], r.o[a]) - lat.origin[a]) / lat.h_min);
    if (!(q >= (double)lo)) return lo;
    return q > (double)hi ? hi : (uint64_t)q;
}

template <typename T, int DIM, int MODE>
__global__ void __launch_bounds__(RAY_THREADS)
ray_kernel(const RayArgs g) {
    constexpr int NCORN = 1 << DIM;
    const int64_t p = blockIdx.x * (int64_t)RAY_THREADS + threadIdx.x;
    if (p >= g.n_rays * g.row_len) return;
    const int64_t slot = p / g.row_len, col = p % g.row_len;
    const int64_t ray = g.order ? (int64_t)g.order[slot] : slot;
    if (ray < 0 || ray >= g.n_rays) return;                                     // (a hostile launch order: nothing is written through it)
    const int depth = g.lat.depth;
    const uint64_t extent = 1ull << depth;

    Ray<DIM> r;
    bool finite = true, moving = false;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        r.o[a] = g.origins[ray * DIM + a], r.d[a] = g.dirs[ray * DIM + a];
        finite &= fabs(r.o[a]) < INFINITY && fabs(r.d[a]) < INFINITY;           // (false for NaN)
        moving |= r.d[a] != 0.0;
    }

    double acc[3] = {0.0, 0.0, 0.0}, lenacc = 0.0, norm = 0.0;
    int32_t segments = 0, status = S3_RAY_MISSED;
    bool broken = false;
    const T *field = static_cast<const T *>(g.field) + col;

    if (!(finite && moving)) {
        status = S3_RAY_BAD_RAY;
        broken = true;                                                          // (the row is NaN)
    } else {
        double s2 = r.d[0] * r.d[0];
#pragma unroll
        for (int a = 1; a < DIM; ++a) s2 = s2 + r.d[a] * r.d[a];
        norm = sqrt(s2);

        // the fixed axes' indices and the domain's chord
        uint64_t i[DIM], anchor[DIM];
        bool inside = true;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            anchor[a] = 0, i[a] = 0;
            if (r.d[a] != 0.0) continue;
            const double t = floor((r.o[a] - g.lat.origin[a]) / g.lat.h_min);  // (lattice_index of cell_lookup.h, one axis)
            const bool ok = t >= 0.0 && t < (double)extent;
            inside &= ok;
            i[a] = ok ? (uint64_t)t : 0;
        }
        double t_in, t_out;
        int e;
        block_chord<DIM>(g.lat, r, anchor, depth, g.t_min, t_in, t_out, e);
        const double len0 = (g.t_max < t_out ? g.t_max : t_out) - t_in;
        if (inside && len0 > 0.0) {
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                if (r.d[a] == 0.0) continue;
                const double tn = plane_tau<DIM>(g.lat, r, a, r.d[a] > 0.0 ? 0 : extent);
                i[a] = tn == t_in ? (r.d[a] > 0.0 ? 0 : extent - 1) : point_index<DIM>(g.lat, r, a, t_in, 0, extent - 1);
            }

            bool ended = false;
            for (int64_t step = 0; step < g.max_steps; ++step) {
                // the block of i: a leaf or an empty block
                const uint64_t key = morton_key<DIM>(i, depth);
                int64_t lo = 0, hi = g.n_cells;                                 // (search_leaf's upper bound, kept for the gap)
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (g.starts[mid] <= key) lo = mid + 1;
                    else hi = mid;
                }
                const uint64_t g0 = lo > 0 ? g.ends[lo - 1] : 0;
                int s = 0;
                int64_t id = -1;
                bool leaf = false, leaf_ok = false;
                if (lo > 0 && key < g0) {
                    leaf = true;
                    id = g.ids[lo - 1];
                    if (id >= 0 && id < g.n_cells && (MODE == S3_RAY_LINEAR || id < g.n_field_rows)) {
                        const int l = g.level[id];
                        if (l >= 0 && l <= depth) s = depth - l, leaf_ok = true;
                    }
                } else {
                    const uint64_t g1 = lo < g.n_cells ? g.starts[lo] : 1ull << (DIM * depth);      // (dim * L <= 63: check_grid)
                    while (s < depth) {                                         // (the fit is monotone in s: the first failure ends it)
                        const uint64_t size = 1ull << (DIM * (s + 1)), base = key & ~(size - 1);
                        if (!(base >= g0 && base + size <= g1)) break;
                        ++s;
                    }
                }
#pragma unroll
                for (int a = 0; a < DIM; ++a) anchor[a] = (i[a] >> s) << s;
                block_chord<DIM>(g.lat, r, anchor, s, g.t_min, t_in, t_out, e);
                const double len = (g.t_max < t_out ? g.t_max : t_out) - t_in;

                if (leaf && len > 0.0) {
                    if constexpr (MODE == S3_RAY_CELL) {
                        if (leaf_ok) {
                            const T *row = field + id * g.in_stride;
#pragma unroll
                            for (int c = 0; c < 3; ++c)
                                if (c < g.n_comp) acc[c] = fma((double)row[c * g.row_len], len, acc[c]);
                        }
                    } else {
                        int32_t node[NCORN];
                        if (leaf_ok) {
#pragma unroll
                            for (int m = 0; m < NCORN; ++m) {
                                node[m] = g.faces[id * NCORN + m];
                                leaf_ok &= node[m] >= 0 && node[m] < g.n_field_rows;
                            }
                        }
                        if (leaf_ok) {
                            const double h = cell_size(g.width, depth - s), half = len / 2, mid = t_in + half, gp = half * GAUSS2;
                            double xi1[DIM], xi2[DIM];
#pragma unroll
                            for (int a = 0; a < DIM; ++a) {
                                const double c = g.centers[id * DIM + a];
                                const bool mv = r.d[a] != 0.0;
                                xi1[a] = local_xi(mv ? fma(mid - gp, r.d[a], r.o[a]) : r.o[a], c, h);
                                xi2[a] = local_xi(mv ? fma(mid + gp, r.d[a], r.o[a]) : r.o[a], c, h);
                            }
                            double b1[3] = {0.0, 0.0, 0.0}, b2[3] = {0.0, 0.0, 0.0};
#pragma unroll
                            for (int m = 0; m < NCORN; ++m) {
                                const double w1 = corner_weight<DIM>(xi1, m), w2 = corner_weight<DIM>(xi2, m);
                                const T *row = field + (int64_t)node[m] * g.in_stride;
#pragma unroll
                                for (int c = 0; c < 3; ++c)
                                    if (c < g.n_comp) {
                                        const double v = (double)row[c * g.row_len];
                                        b1[c] = fma(w1, v, b1[c]), b2[c] = fma(w2, v, b2[c]);
                                    }
                            }
#pragma unroll
                            for (int c = 0; c < 3; ++c)
                                if (c < g.n_comp) acc[c] = fma(half, b1[c] + b2[c], acc[c]);
                        }
                    }
                    broken |= !leaf_ok;
                    lenacc = lenacc + len;
                    ++segments;
                }

                if (t_out >= g.t_max) {
                    ended = true;
                    break;
                }
                // across the exit face, in integers
                bool leaves = false;                                            // (a == e under unroll: no array is indexed by a register)
#pragma unroll
                for (int a = 0; a < DIM; ++a)
                    if (a == e) leaves = r.d[a] > 0.0 ? anchor[a] + (1ull << s) >= extent : anchor[a] == 0;
                if (leaves) {
                    ended = true;
                    break;
                }
#pragma unroll
                for (int a = 0; a < DIM; ++a) {
                    if (r.d[a] == 0.0) continue;
                    if (a == e) i[a] = r.d[a] > 0.0 ? anchor[a] + (1ull << s) : anchor[a] - 1;
                    else i[a] = point_index<DIM>(g.lat, r, a, t_out, anchor[a], anchor[a] + (1ull << s) - 1);
                }
            }
            status = broken ? S3_RAY_BROKEN : !ended ? S3_RAY_TRUNCATED : segments > 0 ? S3_RAY_CROSSED : S3_RAY_MISSED;
        }
    }

    const double scale = segments > 0 ? norm : 0.0;                             // (a ray without segments: 0, whatever |d| is)
    double *out = g.out + ray * g.out_stride + col;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (c < g.n_comp) out[c * g.row_len] = broken ? (double)NAN : scale * acc[c];
    if (col == 0) {
        g.length[ray] = scale * lenacc;
        g.segments[ray] = segments;
        g.status[ray] = status;
    }
}

template <typename T, int DIM>
int launch_rays(int mode, const RayArgs &g, hipStream_t st) {
    const unsigned blocks = grid_for(g.n_rays * g.row_len, RAY_THREADS);
    if (mode == S3_RAY_CELL) ray_kernel<T, DIM, S3_RAY_CELL><<<blocks, RAY_THREADS, 0, st>>>(g);
    else ray_kernel<T, DIM, S3_RAY_LINEAR><<<blocks, RAY_THREADS, 0, st>>>(g);
    S3_LAUNCH_CHECK();
    return S3_OK;
}

}  // namespace

}  // namespace s3

using namespace s3;

extern "C" {

int s3_ray_integrate(int mode, const s3_grid *grid, const double *d_origins, const double *d_dirs, int64_t n_rays, const int32_t *d_order,
                     double t_min, double t_max, int64_t max_steps, const void *d_field, int dtype, int n_comp, int64_t row_len,
                     int64_t in_stride, int64_t n_field_rows, double *d_out, int64_t out_stride, double *d_length, int32_t *d_segments,
                     int32_t *d_status, s3_stream stream) {
    S3_REQUIRE(mode == S3_RAY_CELL || mode == S3_RAY_LINEAR, "s3_ray_integrate: unknown mode %d", mode);
    const bool linear = mode == S3_RAY_LINEAR;
    if (const int rc = check_grid("s3_ray_integrate", grid, linear, n_rays != 0)) return rc;
    S3_REQUIRE(dtype == S3_DTYPE_F32 || dtype == S3_DTYPE_F64, "s3_ray_integrate: unknown dtype %d", dtype);
    S3_REQUIRE(n_comp >= 1 && n_comp <= 3, "s3_ray_integrate: n_comp=%d outside [1,3] (wider fields go in groups of components)", n_comp);
    S3_REQUIRE(row_len >= 1 && n_field_rows >= 1 && n_field_rows < ((int64_t)1 << 31), "s3_ray_integrate: bad field row_len=%lld rows=%lld",
               (long long)row_len, (long long)n_field_rows);
    S3_REQUIRE(n_rays >= 0 && n_rays < ((int64_t)1 << 31) && n_rays * row_len < ((int64_t)1 << 31),
               "s3_ray_integrate: too many lanes (n_rays=%lld row_len=%lld): split the batch", (long long)n_rays, (long long)row_len);
    if (in_stride <= 0) in_stride = n_comp * row_len;
    if (out_stride <= 0) out_stride = n_comp * row_len;
    S3_REQUIRE(in_stride >= n_comp * row_len && out_stride >= n_comp * row_len, "s3_ray_integrate: in_stride %lld / out_stride %lld shorter than a row",
               (long long)in_stride, (long long)out_stride);
    S3_REQUIRE(t_min <= t_max, "s3_ray_integrate: t_min %g .. t_max %g is no range of the ray parameter", t_min, t_max);   // (false for NaN)
    S3_REQUIRE(max_steps >= 1, "s3_ray_integrate: max_steps=%lld", (long long)max_steps);
    if (n_rays == 0) return S3_OK;
    S3_REQUIRE(d_origins && d_dirs && d_field, "s3_ray_integrate: null input array");
    S3_REQUIRE(d_out && d_length && d_segments && d_status, "s3_ray_integrate: null output array");
    const RayArgs g{grid->d_starts, grid->d_ends, grid->d_ids, grid->n_cells, make_lattice(*grid), grid->d_centers, grid->d_levels, grid->width,
                    grid->d_faces, d_field, n_comp, row_len, in_stride, n_field_rows, d_origins, d_dirs, n_rays, d_order, t_min, t_max,
                    max_steps, d_out, out_stride, d_length, d_segments, d_status};
    hipStream_t st = as_stream(stream);
    // element loads: the lanes of a ray take adjacent columns, one element each
    return dispatch_rows<ScalarRows>(dtype, 1, [&](auto row) {
        using T = typename decltype(row)::type;
        return grid->dim == 2 ? launch_rays<T, 2>(mode, g, st) : launch_rays<T, 3>(mode, g, st);
    });
}

}  // extern "C"
