// Streamlines and pathlines of a velocity field on the NODES of a generated grid: classical RK4 through the multilinear blend of the
// containing cell's corner values, one lane per particle, the whole locate / gather / advance loop of a particle in one launch.
// gfx950 only.  No counterpart in the reference.
//
// Definition (include/s3hip.h is normative; restated here).
//   velocity at x in column t: locate x as s3_cell_locate does (floored f64 lattice quotient, range test before the integer
//       conversion, half-open cells, the upper cell on a face); blend the 2^d corner rows of that cell as cell_sample_kernel does in
//       linear mode (xi clamp, one rounding per axis in a weight, f64 fma chain over the corners in the order of `faces` from 0): the
//       bits s3_cell_sample returns at x.  Both are the functions of csrc/cell_lookup.h.
//   time (pathlines): a snapshot interval [c, c+1] takes `substeps` RK4 steps; the stage at (m + s) / substeps of the way through it,
//       s in {0, 1/2, 1}, sits at p / (2 substeps) from column c with the integer p = 2m + 2s forward and 2 substeps - (2m + 2s)
//       backward.  n = c, theta = (double)p / (double)(2 substeps) while p < 2 substeps; n = c + 1, theta = 0 at p = 2 substeps; where
//       that n is the last column, n = T - 2 and theta = 1.  v = fma(theta, v_{n+1}(x) - v_n(x), v_n(x)) per component, both blends in
//       the same cell.  Forward the intervals run c = 0 .. T-2, backward c = T-2 .. 0.
//   one step: k1 = v(x), x2 = fma(dt/2, k1, x), k2 = v(x2), x3 = fma(dt/2, k2, x), k3 = v(x3), x4 = fma(dt, k3, x), k4 = v(x4),
//       x' = fma(dt/6, (k1 + k4) + 2 (k2 + k3), x) per component.
//   step size: S3_TRACE_STEP_TIME: dt = direction * step.  S3_TRACE_STEP_CELL (streamlines): dt = direction * ((step * h) / |k1|), h
//       the edge of the cell of x and |k1| = sqrt(((k1_0 k1_0) + k1_1 k1_1) + k1_2 k1_2), products and sums rounded one by one.
//   termination: the seed is located first (none: SEED_OUTSIDE, length 0, every row NaN).  A step is accepted only when x2, x3, x4 and
//       x' all have a cell (the cell of x' serves the next step's k1); otherwise the particle stays at x with status LEFT.  A cell
//       counts as missing too when its id, its level or one of its corner ids is out of range: nothing is loaded through them.
//       Cell rule with |k1| zero or not finite: STAGNANT.  All steps taken: DONE.  Row 0 of a path is the seed, row r the position
//       after r * every accepted steps (pathlines: after r snapshot intervals); `length` counts the rows written, the rest is NaN.
//
// Same-cell shortcut.  A lane keeps the lattice index i* of the point that found its current leaf and the leaf's s = L - l.  A point
// with lattice index i lies in that leaf exactly when (i ^ i*) >> s is 0 on every axis (the leaf is the aligned box of 2^s lattice
// cells that holds i*: a <= i < a + 2^s), an integer test on the same floored quotient, so it cannot disagree with the binary search
// it skips; what is kept of the leaf (corner position, edge, corner ids) is what the search would load again.
//
// Regime.  A lane runs a dependent chain: per stage one locate (the integer test, or log2(n_cells) dependent 8-byte loads), 2^d
// gathers of d values (twice that in a pathline) and a few dozen f64 operations; the whole state is d doubles and the leaf.  Latency
// bound: what hides it is the number of particles in flight.  No LDS, no atomics, no scratch.
//
// Work split.  One lane per particle, 256 per workgroup.  Streamlines: particle p = (launch slot j, column t) = (p / T, p % T), the
// column running fastest across lanes, so the lanes of a wavefront start in the same cell and their loads of field[node][c][t .. ]
// coalesce for as long as their paths agree.  Pathlines: a particle is a seed, launched in the order of d_order (s3_spatial_order).
// Terminated lanes idle until their wavefront is through; there is no compaction.
#include "cell_lookup.h"

#include <cmath>

namespace s3 {

namespace {

constexpr int TRACE_THREADS = 256;

struct TraceArgs {
    const uint64_t *starts, *ends;
    const int32_t *ids;
    int64_t n_cells;
    Lattice lat;
    const double *centers;
    const int32_t *level;
    double width;
    const int32_t *faces;
    const void *field;
    int64_t row_len, in_stride, n_nodes;
    const double *seeds;
    int64_t n_seeds;
    const int32_t *order;
    int64_t n_steps;                    // RK4 steps of a particle
    int every;                          // a row per `every` accepted steps (pathlines: substeps)
    int cell_rule;
    double step;
    int direction;
    int64_t n_out;
    double *paths;
    int32_t *length, *status, *cell;
};

// the leaf a lane stands in
template <int DIM>
struct Leaf {
    int32_t id;                         // -1: none yet
    int shift;                          // L - l
    uint32_t i[DIM];                    // the lattice index that found it (below 2^31: dim * L <= 63)
    double center[DIM], h;
    int32_t node[1 << DIM];
};

// puts the lane into the leaf of x; false where x has none
template <int DIM>
__device__ __forceinline__ bool enter_leaf(const TraceArgs &g, const double (&x)[DIM], Leaf<DIM> &leaf) {
    uint64_t i[DIM];
    if (!lattice_index<DIM>(g.lat, x, i)) return false;
    if (leaf.id >= 0) {
        bool same = true;
#pragma unroll
        for (int a = 0; a < DIM; ++a) same &= (((uint32_t)i[a] ^ leaf.i[a]) >> leaf.shift) == 0;
        if (same) return true;
    }
    leaf.id = -1;
    const int64_t id = search_leaf(g.starts, g.ends, g.ids, g.n_cells, morton_key<DIM>(i, g.lat.depth));
    if (id < 0 || id >= g.n_cells) return false;
    const int l = g.level[id];
    if (l < 0 || l > g.lat.depth) return false;
    bool nodes_ok = true;
#pragma unroll
    for (int m = 0; m < (1 << DIM); ++m) {
        leaf.node[m] = g.faces[id * (1 << DIM) + m];
        nodes_ok &= leaf.node[m] >= 0 && leaf.node[m] < g.n_nodes;
    }
    if (!nodes_ok) return false;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        leaf.i[a] = (uint32_t)i[a];
        leaf.center[a] = g.centers[id * DIM + a];
    }
    leaf.h = cell_size(g.width, l);
    leaf.shift = g.lat.depth - l;
    leaf.id = (int32_t)id;
    return true;
}

// the velocity at x, which lies in `leaf`: column col (and col + 1, blended by theta, in a pathline)
template <typename T, int DIM, bool UNSTEADY>
__device__ __forceinline__ void velocity(const TraceArgs &g, const Leaf<DIM> &leaf, const double (&x)[DIM], int64_t col, double theta,
                                         double (&v)[DIM]) {
    double xi[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) xi[a] = local_xi(x[a], leaf.center[a], leaf.h);
    double v0[DIM], v1[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) v0[c] = 0.0, v1[c] = 0.0;
    const T *field = static_cast<const T *>(g.field) + col;
#pragma unroll
    for (int m = 0; m < (1 << DIM); ++m) {
        const double w = corner_weight<DIM>(xi, m);
        const T *row = field + (int64_t)leaf.node[m] * g.in_stride;
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            v0[c] = fma(w, (double)row[c * g.row_len], v0[c]);
            if constexpr (UNSTEADY) v1[c] = fma(w, (double)row[c * g.row_len + 1], v1[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < DIM; ++c) v[c] = UNSTEADY ? fma(theta, v1[c] - v0[c], v0[c]) : v0[c];
}

// (n, theta) of the stage at p / s2 of the interval [c, c + 1], p = 0 .. s2
__device__ __forceinline__ void stage_time(int64_t c, int p, int s2, int64_t last, int64_t &n, double &theta) {
    n = p == s2 ? c + 1 : c;
    theta = p == s2 ? 0.0 : (double)p / (double)s2;
    if (n >= last) n = last - 1, theta = 1.0;
}

template <typename T, int DIM, bool UNSTEADY>
__global__ void __launch_bounds__(TRACE_THREADS)
trace_kernel(const TraceArgs g) {
    const int64_t p = blockIdx.x * (int64_t)TRACE_THREADS + threadIdx.x;
    const int64_t n_particles = UNSTEADY ? g.n_seeds : g.n_seeds * g.row_len;
    if (p >= n_particles) return;
    const int64_t slot = UNSTEADY ? p : p / g.row_len, col = UNSTEADY ? 0 : p % g.row_len;
    const int64_t seed = g.order ? (int64_t)g.order[slot] : slot;
    if (seed < 0 || seed >= g.n_seeds) return;                                  // (a hostile launch order: nothing is written through it)
    const int64_t particle = UNSTEADY ? seed : seed * g.row_len + col;
    const int64_t last = g.row_len - 1;                                         // pathlines: the last column
    const bool backward = g.direction < 0;
    // row r of this particle: streamlines [particle][r][DIM]; pathlines [seed][column][DIM], column r forward, T-1-r backward
    double *out = g.paths + (UNSTEADY ? seed * g.row_len : particle * g.n_out) * DIM;
    auto row_of = [&](int64_t r) { return out + (UNSTEADY && backward ? last - r : r) * DIM; };

    double x[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) x[a] = g.seeds[seed * DIM + a];
    Leaf<DIM> leaf;
    leaf.id = -1;
    leaf.shift = 0;
    int32_t status = S3_TRACE_DONE, cell_x = -1;
    int64_t length = 0;
    if (!enter_leaf<DIM>(g, x, leaf)) {
        status = S3_TRACE_SEED_OUTSIDE;
    } else {
        cell_x = leaf.id;
        double *r0 = row_of(0);
#pragma unroll
        for (int a = 0; a < DIM; ++a) r0[a] = x[a];
        length = 1;
        const int s2 = 2 * g.every;
        for (int64_t step = 0; step < g.n_steps; ++step) {
            // pathlines: step m of the interval c
            int64_t c = 0, n = col;
            int m2 = 0;
            double theta = 0.0;
            if constexpr (UNSTEADY) {
                const int64_t k = step / g.every;
                c = backward ? last - 1 - k : k;
                m2 = 2 * (int)(step % g.every);
                stage_time(c, backward ? s2 - m2 : m2, s2, last, n, theta);
            }
            double k1[DIM], k23[DIM], k[DIM], y[DIM];
            velocity<T, DIM, UNSTEADY>(g, leaf, x, n, theta, k1);
            double dt = g.step;
            if (g.cell_rule) {
                double s = k1[0] * k1[0];
#pragma unroll
                for (int a = 1; a < DIM; ++a) s = s + k1[a] * k1[a];
                const double norm = sqrt(s);
                if (!(norm > 0.0 && norm < INFINITY)) {
                    status = S3_TRACE_STAGNANT;
                    break;
                }
                dt = (g.step * leaf.h) / norm;
            }
            if (backward) dt = -dt;
            const double half = dt / 2, sixth = dt / 6;

#pragma unroll
            for (int a = 0; a < DIM; ++a) y[a] = fma(half, k1[a], x[a]);
            if (!enter_leaf<DIM>(g, y, leaf)) {
                status = S3_TRACE_LEFT;
                break;
            }
            if constexpr (UNSTEADY) stage_time(c, backward ? s2 - m2 - 1 : m2 + 1, s2, last, n, theta);
            velocity<T, DIM, UNSTEADY>(g, leaf, y, n, theta, k23);

#pragma unroll
            for (int a = 0; a < DIM; ++a) y[a] = fma(half, k23[a], x[a]);
            if (!enter_leaf<DIM>(g, y, leaf)) {
                status = S3_TRACE_LEFT;
                break;
            }
            velocity<T, DIM, UNSTEADY>(g, leaf, y, n, theta, k);
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                k23[a] = k23[a] + k[a];
                y[a] = fma(dt, k[a], x[a]);
            }
            if (!enter_leaf<DIM>(g, y, leaf)) {
                status = S3_TRACE_LEFT;
                break;
            }
            if constexpr (UNSTEADY) stage_time(c, backward ? s2 - m2 - 2 : m2 + 2, s2, last, n, theta);
            velocity<T, DIM, UNSTEADY>(g, leaf, y, n, theta, k);

#pragma unroll
            for (int a = 0; a < DIM; ++a) y[a] = fma(sixth, (k1[a] + k[a]) + 2.0 * k23[a], x[a]);
            if (!enter_leaf<DIM>(g, y, leaf)) {
                status = S3_TRACE_LEFT;
                break;
            }
#pragma unroll
            for (int a = 0; a < DIM; ++a) x[a] = y[a];
            cell_x = leaf.id;
            if ((step + 1) % g.every == 0) {
                double *r = row_of(length);
#pragma unroll
                for (int a = 0; a < DIM; ++a) r[a] = x[a];
                ++length;
            }
        }
    }
    for (int64_t r = length; r < g.n_out; ++r) {
        double *row = row_of(r);
#pragma unroll
        for (int a = 0; a < DIM; ++a) row[a] = NAN;
    }
    g.length[particle] = (int32_t)length;
    g.status[particle] = status;
    g.cell[particle] = cell_x;
}

template <typename T, int DIM, bool UNSTEADY>
int launch_trace(const TraceArgs &g, hipStream_t st) {
    const int64_t n_particles = UNSTEADY ? g.n_seeds : g.n_seeds * g.row_len;
    trace_kernel<T, DIM, UNSTEADY><<<grid_for(n_particles, TRACE_THREADS), TRACE_THREADS, 0, st>>>(g);
    S3_LAUNCH_CHECK();
    return S3_OK;
}

template <typename T>
int trace_by_shape(const TraceArgs &g, int dim, bool unsteady, hipStream_t st) {
    if (dim == 2) return unsteady ? launch_trace<T, 2, true>(g, st) : launch_trace<T, 2, false>(g, st);
    return unsteady ? launch_trace<T, 3, true>(g, st) : launch_trace<T, 3, false>(g, st);
}

}  // namespace

}  // namespace s3

using namespace s3;

extern "C" {

int s3_trace(int mode, const s3_grid *grid, const void *d_field, int dtype, int64_t row_len, int64_t in_stride, int64_t n_nodes,
             const double *d_seeds, int64_t n_seeds, const int32_t *d_order, int64_t n_steps, int substeps, int every, int step_rule,
             double step, int direction, double *d_paths, int32_t *d_length, int32_t *d_status, int32_t *d_cell, s3_stream stream) {
    S3_REQUIRE(mode == S3_TRACE_STREAM || mode == S3_TRACE_PATH, "s3_trace: unknown mode %d", mode);
    const bool path = mode == S3_TRACE_PATH;
    if (const int rc = check_grid("s3_trace", grid, true, n_seeds != 0)) return rc;
    const int dim = grid->dim;
    S3_REQUIRE(dtype == S3_DTYPE_F32 || dtype == S3_DTYPE_F64, "s3_trace: unknown dtype %d", dtype);
    S3_REQUIRE(row_len >= (path ? 2 : 1) && n_nodes >= 1 && n_nodes < ((int64_t)1 << 31), "s3_trace: bad field row_len=%lld n_nodes=%lld%s",
               (long long)row_len, (long long)n_nodes, path ? " (a pathline needs two snapshots)" : "");
    if (in_stride <= 0) in_stride = dim * row_len;
    S3_REQUIRE(in_stride >= dim * row_len, "s3_trace: in_stride %lld shorter than the %d component rows of a node", (long long)in_stride, dim);
    S3_REQUIRE(n_seeds >= 0 && n_seeds < ((int64_t)1 << 31) && (path || n_seeds * row_len < ((int64_t)1 << 31)),
               "s3_trace: too many particles (n_seeds=%lld row_len=%lld)", (long long)n_seeds, (long long)row_len);
    S3_REQUIRE(step_rule == S3_TRACE_STEP_TIME || step_rule == S3_TRACE_STEP_CELL, "s3_trace: unknown step rule %d", step_rule);
    S3_REQUIRE(!(path && step_rule == S3_TRACE_STEP_CELL), "s3_trace: a pathline steps in time (S3_TRACE_STEP_TIME)");
    S3_REQUIRE(std::isfinite(step) && step > 0.0, "s3_trace: step %g is no positive %s", step, step_rule == S3_TRACE_STEP_CELL ? "cfl" : "dt");
    S3_REQUIRE(direction == 1 || direction == -1, "s3_trace: direction %d is neither 1 nor -1", direction);
    if (path) {
        S3_REQUIRE(substeps >= 1 && substeps < (1 << 20), "s3_trace: substeps=%d", substeps);
        n_steps = (row_len - 1) * substeps;
        every = substeps;
    } else {
        S3_REQUIRE(n_steps >= 1 && n_steps < ((int64_t)1 << 31) && every >= 1, "s3_trace: n_steps=%lld every=%d", (long long)n_steps, every);
    }
    const int64_t n_out = path ? row_len : 1 + n_steps / every;
    if (n_seeds == 0) return S3_OK;
    S3_REQUIRE(d_field && d_seeds, "s3_trace: null input array");
    S3_REQUIRE(d_paths && d_length && d_status && d_cell, "s3_trace: null output array");
    const TraceArgs g{grid->d_starts, grid->d_ends, grid->d_ids, grid->n_cells, make_lattice(*grid), grid->d_centers, grid->d_levels, grid->width,
                      grid->d_faces, d_field, row_len, in_stride, n_nodes, d_seeds, n_seeds, d_order, n_steps, every, step_rule == S3_TRACE_STEP_CELL,
                      step, direction, n_out, d_paths, d_length, d_status, d_cell};
    hipStream_t st = as_stream(stream);
    return dtype == S3_DTYPE_F32 ? trace_by_shape<float>(g, dim, path, st) : trace_by_shape<double>(g, dim, path, st);
}

}  // extern "C"
