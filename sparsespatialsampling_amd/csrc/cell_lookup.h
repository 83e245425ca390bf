// Which leaf of a generated grid holds a position, and the multilinear weights of its corners there: the pieces of the definition in
// include/s3hip.h ("sampling a grid field at arbitrary positions") that more than one kernel family evaluates -- sample.hip (index,
// locate, sample) and trace.hip (the locate / gather / advance loop of a particle).  gfx950 only.
//
// Every function here is the definition operation by operation, in plain f64 (the build has -ffp-contract=off; fma where it is
// written):
//     lattice_index   i_a = floor((x_a - origin_a) / h_min), the range test 0 <= i_a < 2^L BEFORE the integer conversion (NaN, +-inf
//                     and whatever lies outside fail it); half-open cells: a point on a face belongs to the upper cell
//     morton_key      bit b of axis a at position b*DIM + a
//     search_leaf     upper bound of the key over the sorted range starts, then the range test: the cell id or -1
//     local_xi        xi_a = clamp((x_a - (c_a - h/2)) / h, 0, 1)
//     corner_weight   t = (s_m0 > 0 ? xi_0 : 1 - xi_0), then per further axis t = s_ma > 0 ? t * xi_a : fma(-xi_a, t, t): one rounding
//                     per axis; corner m in the order `faces` lists them
#ifndef S3_CELL_LOOKUP_H
#define S3_CELL_LOOKUP_H

#include "common.h"

#include <cmath>

namespace s3 {

struct Lattice {
    double origin[3];
    double h_min;
    int depth;                          // L
};

__host__ __device__ inline double cell_size(double width, int level) { return width / (double)(1ull << level); }

// what every entry point that takes an s3_grid requires of it (include/s3hip.h states it once); `work`: something is looked up, so
// the arrays are read; `need_faces`: node fields are read through d_faces
inline int check_grid(const char *who, const s3_grid *g, bool need_faces, bool work) {
    S3_REQUIRE(g, "%s: null grid", who);
    S3_REQUIRE(g->n_cells >= 1 && g->n_cells < ((int64_t)1 << 31) && (g->dim == 2 || g->dim == 3), "%s: bad grid n_cells=%lld dim=%d", who,
               (long long)g->n_cells, g->dim);
    S3_REQUIRE(g->depth >= 0 && g->dim * g->depth <= 63 && g->h_min > 0.0, "%s: bad lattice (depth %d, h_min %g)", who, g->depth, g->h_min);
    S3_REQUIRE(g->width > 0.0 && std::isfinite(g->width), "%s: width %g is no cell size", who, g->width);
    S3_REQUIRE(!work || (g->d_starts && g->d_ends && g->d_ids && g->d_centers && g->d_levels), "%s: null array in the grid", who);
    S3_REQUIRE(!work || !need_faces || g->d_faces, "%s: the grid has no faces (d_faces) to read node fields through", who);
    return S3_OK;
}

inline Lattice make_lattice(const s3_grid &g) {
    Lattice lat{};
    for (int a = 0; a < g.dim; ++a) lat.origin[a] = g.origin[a];
    lat.h_min = g.h_min;
    lat.depth = g.depth;
    return lat;
}

template <int DIM>
__device__ __forceinline__ uint64_t morton_key(const uint64_t (&i)[DIM], int depth) {
    uint64_t key = 0;
    for (int b = 0; b < depth; ++b)
#pragma unroll
        for (int a = 0; a < DIM; ++a) key |= ((i[a] >> b) & 1ull) << (b * DIM + a);
    return key;
}

// the lattice cell of x; false where x has none (i is 0 on the axes that fail)
template <int DIM>
__device__ __forceinline__ bool lattice_index(const Lattice &lat, const double (&x)[DIM], uint64_t (&i)[DIM]) {
    const double extent = (double)(1ull << lat.depth);
    bool inside = true;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        const double t = floor((x[a] - lat.origin[a]) / lat.h_min);
        const bool ok = t >= 0.0 && t < extent;                                 // false for NaN, +-inf and whatever lies outside
        inside &= ok;
        i[a] = ok ? (uint64_t)t : 0;
    }
    return inside;
}

// the leaf whose range holds the key, -1 where none does
__device__ __forceinline__ int32_t search_leaf(const uint64_t *__restrict__ starts, const uint64_t *__restrict__ ends,
                                               const int32_t *__restrict__ ids, int64_t n_cells, uint64_t key) {
    int64_t lo = 0, hi = n_cells;                                               // upper bound: the first range that starts past the key
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (starts[mid] <= key) lo = mid + 1;
        else hi = mid;
    }
    return lo > 0 && key < ends[lo - 1] ? ids[lo - 1] : -1;
}

// corner m of a cell in the order `faces` lists them: 2-D (-,-), (-,+), (+,+), (+,-); 3-D that order at z+, then at z-
__device__ __forceinline__ bool corner_plus(int m, int axis) {
    const int q = m & 3;
    return axis == 0 ? q >= 2 : axis == 1 ? (q == 1 || q == 2) : m < 4;
}

__device__ __forceinline__ double local_xi(double x, double center, double h) {
    const double xi = (x - (center - h / 2)) / h;
    return fmin(fmax(xi, 0.0), 1.0);
}

template <int DIM>
__device__ __forceinline__ double corner_weight(const double (&xi)[DIM], int m) {
    double w = corner_plus(m, 0) ? xi[0] : 1.0 - xi[0];
#pragma unroll
    for (int a = 1; a < DIM; ++a) w = corner_plus(m, a) ? w * xi[a] : fma(-xi[a], w, w);
    return w;
}

}  // namespace s3

#endif
