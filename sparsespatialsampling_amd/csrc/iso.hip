// Isosurfaces (3-D) and contour lines (2-D) of fields on the grid NODES by marching simplices on the leaves: every leaf is cut into
// d! simplices (Kuhn's decomposition along the diagonal from the (-, .., -) corner to the (+, .., +) corner), every simplex emits 0, 1
// or 2 primitives (triangles | segments), a whole snapshot batch per launch.  gfx950 only.  No counterpart in the reference, whose
// post-processing writes files for a viewer.
//
// Definition: include/s3hip.h states it (inside: (double) f >= level; a cell with a non-finite corner value or a bad corner id emits
// nothing; simplices in lexicographic order of the axis permutation; vertex on the edge between the nodes a < b in GLOBAL node id:
// t = (level - f_a) / (f_b - f_a), x = fma(t, x_b - x_a, x_a), so that the same edge gives the same bits in every simplex and cell).
//
// Two passes and the scan of csrc/scan_sort.h between them, positions never from atomics:
//     s3_iso_count   count[t][cell] = sum over the simplices of min(|I|, d + 1 - |I|), I the inside positions of the simplex
//     s3_exclusive_scan (in place), the caller reads back the total
//     s3_iso_emit    a (cell, t) with primitives writes them at offset[t][cell] ..: ordered by (snapshot, cell, simplex, primitive)
//
// Regime: per cell 2^d node rows of T values are gathered from the field itself (neighbouring cells share corners: L2 / Infinity
// Cache), 4 T bytes are written by the count; the emit gathers the same rows again, and only the few percent of the (cell, t) that
// are cut go on -- 124 bytes per triangle (52 per segment) and the coordinates of the edge ends.  It is the regime of
// cell_sample_kernel in linear mode (csrc/sample.hip) with half the bytes written.
//
// Work split: the point slots of csrc/point_slots.h over blocks of ISO_BLOCK consecutive cells in the caller's numbering; the staged
// table is the 2^d corner ids of each cell of a stage (-1: outside [0, n_nodes)); lane l of a slot owns the snapshots
// [(chunk*LP + l)*VEC, +VEC).  A lane loads its 2^d pieces in their storage type before the first compare.  The counts of a stage go
// through LDS (a byte each) and leave as runs of consecutive cells of one row of count[t][cell].  A cut (cell, t) is rare,
// so the emit does not keep the corner values in registers for it: it reads the two values of a crossing edge again (element loads
// that hit the lines the pieces came from), which keeps every index into registers a compile-time one (no scratch).
#include "point_slots.h"
#include "typed_rows.h"

#include <cmath>

namespace s3 {

namespace {

constexpr int ISO_THREADS = POINT_THREADS;
constexpr int ISO_BLOCK = 256;          // cells per workgroup

// ---- the tables ---------------------------------------------------------------------------------------------------------------
// corner m of `faces`: 2-D (-,-), (-,+), (+,+), (+,-); 3-D that order at z+, then at z-.  KUHN[s][p]: the corner at position p of the
// path of the s-th permutation of the axes in lexicographic order, from (-, .., -) by switching axis pi(i) to + in step i.
__device__ constexpr unsigned char KUHN3[6][4] = {{4, 7, 6, 2}, {4, 7, 3, 2}, {4, 5, 6, 2}, {4, 5, 1, 2}, {4, 0, 3, 2}, {4, 0, 1, 2}};
__device__ constexpr unsigned char KUHN2[2][3] = {{0, 3, 2}, {0, 1, 2}};
// bit s: permutation s is odd
constexpr unsigned ODD3 = 1u << 1 | 1u << 2 | 1u << 5, ODD2 = 1u << 1;
// bit m (bit p of m: path position p is inside): in a simplex of an EVEN permutation the natural vertex order of the primitives has
// its normal towards f >= level (2-D: the inside to the right), so the last two vertices are swapped; odd permutations: the others
constexpr unsigned SWAP3 = 1u << 2 | 1u << 5 | 1u << 8 | 1u << 10 | 1u << 11 | 1u << 14, SWAP2 = 1u << 2 | 1u << 3 | 1u << 6;

template <int DIM> __device__ __forceinline__ int kuhn_corner(int s, int p) {
    if constexpr (DIM == 3) return KUHN3[s][p];
    else return KUHN2[s][p];
}

template <int DIM> struct Simplices {
    static constexpr int count = DIM == 3 ? 6 : 2;
    static constexpr unsigned odd = DIM == 3 ? ODD3 : ODD2, swap = DIM == 3 ? SWAP3 : SWAP2;
};

// the mask of simplex s (bit p: position p inside) from the mask of the cell (bit m: corner m inside)
template <int DIM> __device__ __forceinline__ unsigned simplex_mask(unsigned corners, int s) {
    unsigned m = 0;
#pragma unroll
    for (int p = 0; p <= DIM; ++p) m |= ((corners >> kuhn_corner<DIM>(s, p)) & 1u) << p;
    return m;
}

template <int DIM> __device__ __forceinline__ int primitives_of(unsigned corners) {
    int n = 0;
#pragma unroll
    for (int s = 0; s < Simplices<DIM>::count; ++s) {
        const int in = __popc(simplex_mask<DIM>(corners, s));
        n += min(in, DIM + 1 - in);
    }
    return n;
}

// (corner mask, all finite) of snapshot i of a lane's pieces
template <typename T, int VEC, int NCORN>
__device__ __forceinline__ unsigned corner_mask(const typename RowVec<T, VEC>::type (&raw)[NCORN], int i, double level, bool &finite) {
    unsigned corners = 0;
    finite = true;
#pragma unroll
    for (int m = 0; m < NCORN; ++m) {
        const double v = row_elem<T, VEC>(raw[m], i);
        finite &= fabs(v) < INFINITY;                                           // (false for NaN)
        corners |= (v >= level ? 1u : 0u) << m;
    }
    return corners;
}

struct IsoArgs {
    const void *field;
    int64_t row_len, in_stride, n_nodes;
    const int32_t *faces;
    int64_t n_cells;
    double level;
    int32_t *count;                     // count pass: [row_len][n_cells]; emit pass: its exclusive scan
    const double *nodes;
    int64_t capacity;
    double *verts;
    int32_t *edges;
    double *frac;
    int32_t *cells;
    hipStream_t st;
};

// the primitives of one cut (cell, snapshot), written at pos, pos + 1, ..: fcol = the field at this snapshot's column
template <typename T, int DIM>
__device__ __forceinline__ void emit_cell(const T *__restrict__ fcol, int64_t in_stride, const int32_t *ip, unsigned corners, double level,
                                          const double *__restrict__ nodes, int64_t pos, int64_t capacity, int32_t cell,
                                          double *__restrict__ verts, int32_t *__restrict__ edges, double *__restrict__ frac,
                                          int32_t *__restrict__ cells) {
    constexpr unsigned FULL = (1u << (DIM + 1)) - 1;
    for (int s = 0; s < Simplices<DIM>::count; ++s) {
        const unsigned m = simplex_mask<DIM>(corners, s);
        const int in = __popc(m), n_prim = min(in, DIM + 1 - in);
        if (n_prim == 0) continue;
        // the up to four crossing edges q0 .. q3 as pairs of path positions, 4 bits each: (first | second << 2) << 4 k
        unsigned pairs = 0;
        if (n_prim == 1) {                                                      // one position alone on its side: (s, a), (s, b) (, (s, c))
            const int lone = __ffs(in == 1 ? m : ~m & FULL) - 1;
            int k = 0;
#pragma unroll
            for (int o = 0; o <= DIM; ++o)
                if (o != lone) pairs |= (unsigned)(lone | o << 2) << (4 * k++);
        } else {                                                                // I = {i, j}, O = {k, l}: (i,k), (i,l), (j,l), (j,k)
            const unsigned out = ~m & FULL;
            const int i = __ffs(m) - 1, j = 31 - __clz(m), k = __ffs(out) - 1, l = 31 - __clz(out);
            pairs = (unsigned)(i | k << 2) | (unsigned)(i | l << 2) << 4 | (unsigned)(j | l << 2) << 8 | (unsigned)(j | k << 2) << 12;
        }
        const bool swap = (((Simplices<DIM>::swap >> m) ^ (Simplices<DIM>::odd >> s)) & 1u) != 0;
        for (int pr = 0; pr < n_prim; ++pr, ++pos) {
            if (pos < 0 || pos >= capacity) continue;
#pragma unroll
            for (int v = 0; v < DIM; ++v) {
                const int w = swap && v >= DIM - 2 ? 2 * DIM - 3 - v : v;       // the last two vertices change places
                const unsigned pq = pairs >> (4 * (w == 0 ? 0 : w + pr)) & 15u;  // triangle pr of a quad: (q0, q1, q2), (q0, q2, q3)
                const int32_t n0 = ip[kuhn_corner<DIM>(s, pq & 3)], n1 = ip[kuhn_corner<DIM>(s, pq >> 2)];
                const int32_t a = min(n0, n1), b = max(n0, n1);
                const double fa = (double)fcol[(int64_t)a * in_stride], fb = (double)fcol[(int64_t)b * in_stride];
                const double t = (level - fa) / (fb - fa);
                const int64_t o = pos * DIM + v;
                frac[o] = t;
                edges[2 * o] = a, edges[2 * o + 1] = b;
#pragma unroll
                for (int ax = 0; ax < DIM; ++ax) {
                    const double xa = nodes[(int64_t)a * DIM + ax], xb = nodes[(int64_t)b * DIM + ax];
                    verts[o * DIM + ax] = fma(t, xb - xa, xa);
                }
            }
            cells[pos] = cell;
        }
    }
}

// EMIT = false: the count pass; true: the emit pass
template <typename T, int VEC, int DIM, bool EMIT>
__global__ void __launch_bounds__(ISO_THREADS)
iso_kernel(const T *__restrict__ field, int64_t row_len, int64_t in_stride, int64_t n_nodes, const int32_t *__restrict__ faces, int64_t n_cells,
           double level, int32_t *__restrict__ count, const double *__restrict__ nodes, int64_t capacity, double *__restrict__ verts,
           int32_t *__restrict__ edges, double *__restrict__ frac, int32_t *__restrict__ cells, int lp, int stage_pts, int n_chunks,
           int64_t n_blocks, int64_t blocks_per_xcd) {
    using V = typename RowVec<T, VEC>::type;
    constexpr int NCORN = 1 << DIM;
    constexpr unsigned ALL = (1u << NCORN) - 1;
    extern __shared__ int32_t s_i[];                                            // [stage_pts * NCORN], -1: no such node
    // count pass: the counts of a stage, [lp * VEC columns][stage_pts cells] (they fit a byte), so that they leave as runs of consecutive
    // cells of one snapshot row of count[][] and not as one element per lane
    unsigned char *s_c = reinterpret_cast<unsigned char *>(s_i + stage_pts * NCORN);
    const int pg = ISO_THREADS / lp;

    const int64_t blk = xcd_block(blockIdx.x, blocks_per_xcd);
    if (blk >= n_blocks) return;
    const int64_t p0 = blk * ISO_BLOCK, n_total = row_len * n_cells;
    const int n_p = (int)min((int64_t)ISO_BLOCK, n_cells - p0);
    const int t = threadIdx.x, lane = t & (lp - 1), slot = t / lp;

    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        const int64_t col0 = ((int64_t)chunk * lp + lane) * VEC;
        const bool col_ok = col0 < row_len;                                     // VEC divides row_len: a piece is inside or outside
        for (int sb = 0; sb < n_p; sb += stage_pts) {
            const int n_st = min(stage_pts, n_p - sb);
            __syncthreads();                                                    // the previous stage's table has been read
            for (int e = t; e < n_st * NCORN; e += ISO_THREADS) {
                const int32_t node = faces[(p0 + sb) * NCORN + e];
                s_i[e] = node >= 0 && node < n_nodes ? node : -1;
            }
            __syncthreads();
            for (int pb = sb; pb < sb + n_st; pb += pg) {
                if (!(col_ok && pb + slot < sb + n_st)) continue;
                const int64_t cell = p0 + pb + slot;
                const int32_t *ip = s_i + (pb - sb + slot) * NCORN;
                const T *col = field + col0;
                const int64_t at = col0 * n_cells + cell;                       // (snapshot, cell) of piece element 0 in count[][]

                bool hit = true;
#pragma unroll
                for (int m = 0; m < NCORN; ++m) hit &= ip[m] >= 0;
                if constexpr (!EMIT) {
                    if (!hit) {                                                 // a bad id: nothing at any snapshot, nothing loaded
#pragma unroll
                        for (int i = 0; i < VEC; ++i) s_c[(lane * VEC + i) * stage_pts + (pb - sb + slot)] = 0;
                        continue;
                    }
                } else {
                    // a (cell, snapshot) without primitives does no further work: its offset equals its successor's (the last
                    // entry of all has no successor and is decided by its values)
                    int64_t pos[VEC];
                    bool any = false;
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        const int64_t e = at + i * n_cells;
                        pos[i] = count[e];
                        if (e + 1 < n_total && count[e + 1] == pos[i]) pos[i] = -1;
                        any |= pos[i] >= 0;
                    }
                    if (!(hit && any)) continue;
                    V raw[NCORN];
#pragma unroll
                    for (int m = 0; m < NCORN; ++m) raw[m] = row_load<T, VEC>(col + (int64_t)ip[m] * in_stride);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        bool finite;
                        const unsigned corners = corner_mask<T, VEC, NCORN>(raw, i, level, finite);
                        if (pos[i] < 0 || !finite || corners == 0 || corners == ALL) continue;
                        emit_cell<T, DIM>(col + i, in_stride, ip, corners, level, nodes, pos[i], capacity, (int32_t)cell, verts, edges, frac, cells);
                    }
                    continue;
                }
                V raw[NCORN];
#pragma unroll
                for (int m = 0; m < NCORN; ++m) raw[m] = row_load<T, VEC>(col + (int64_t)ip[m] * in_stride);
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    bool finite;
                    const unsigned corners = corner_mask<T, VEC, NCORN>(raw, i, level, finite);
                    s_c[(lane * VEC + i) * stage_pts + (pb - sb + slot)] = (unsigned char)(finite ? primitives_of<DIM>(corners) : 0);
                }
            }
            if constexpr (!EMIT) {
                __syncthreads();                                                // the stage's counts are complete
                const int64_t c0 = (int64_t)chunk * lp * VEC;
                const int n_cols = (int)min((int64_t)lp * VEC, row_len - c0);
                for (int e = t; e < n_cols * n_st; e += ISO_THREADS) {
                    const int c = e / n_st, j = e - c * n_st;
                    count[(c0 + c) * n_cells + p0 + sb + j] = s_c[c * stage_pts + j];
                }
            }
        }
    }
}

template <typename T, int VEC, int DIM, bool EMIT>
int launch_iso(const char *who, const IsoArgs &g) {
    // LDS (slot_shape, csrc/point_slots.h): the 2^d corner ids of each cell of a stage (64 cells: 2 KB in 3-D)
    constexpr int NCORN = 1 << DIM;
    SlotShape shape;
    if (const int rc = slot_shape(who, g.row_len, g.row_len / VEC, NCORN * sizeof(int32_t), 0, 0, shape)) return rc;
    const int64_t n_blocks = (g.n_cells + ISO_BLOCK - 1) / ISO_BLOCK;
    const XcdGrid xcd = xcd_grid(n_blocks);
    S3_REQUIRE(xcd.fits(), "%s: too many cells", who);
    // (count pass: a byte per column of a chunk and cell of a stage on top, 16 KB at the most)
    const size_t lds_bytes = shape.lds_bytes + (EMIT ? 0 : (size_t)shape.lanes * VEC * shape.stage_pts);
    iso_kernel<T, VEC, DIM, EMIT><<<(unsigned)xcd.grid, ISO_THREADS, lds_bytes, g.st>>>(
        static_cast<const T *>(g.field), g.row_len, g.in_stride, g.n_nodes, g.faces, g.n_cells, g.level, g.count, g.nodes, g.capacity, g.verts,
        g.edges, g.frac, g.cells, shape.lanes, shape.stage_pts, (int)shape.n_chunks, n_blocks, xcd.per_xcd);
    S3_LAUNCH_CHECK();
    return S3_OK;
}

template <bool EMIT>
int iso_pass(const char *who, IsoArgs g, int dtype, int dim) {
    S3_REQUIRE(dim == 2 || dim == 3, "%s: dim=%d", who, dim);
    S3_REQUIRE(dtype == S3_DTYPE_F32 || dtype == S3_DTYPE_F64, "%s: unknown dtype %d", who, dtype);
    S3_REQUIRE(g.row_len >= 1 && g.n_nodes >= 1 && g.n_nodes < ((int64_t)1 << 31) && g.n_cells >= 0, "%s: bad shape row_len=%lld nodes=%lld cells=%lld",
               who, (long long)g.row_len, (long long)g.n_nodes, (long long)g.n_cells);
    // int32 counts and offsets: at most 12 (3-D) | 2 (2-D) primitives per cell and snapshot
    S3_REQUIRE((double)(dim == 3 ? 12 : 2) * (double)g.n_cells * (double)g.row_len < 2147483648.0,
               "%s: %lld cells x %lld snapshots may give 2^31 primitives or more: split the batch", who, (long long)g.n_cells, (long long)g.row_len);
    S3_REQUIRE(std::isfinite(g.level), "%s: the level must be finite", who);
    if (g.in_stride <= 0) g.in_stride = g.row_len;
    S3_REQUIRE(g.in_stride >= g.row_len, "%s: in_stride %lld shorter than a row", who, (long long)g.in_stride);
    if (g.n_cells == 0) return S3_OK;
    S3_REQUIRE(g.field && g.faces && g.count, "%s: null array", who);
    if (EMIT) {
        S3_REQUIRE(g.capacity >= 0, "%s: negative capacity", who);
        S3_REQUIRE(g.nodes && (g.capacity == 0 || (g.verts && g.edges && g.frac && g.cells)), "%s: null array", who);
    }
    // the width of a lane's piece: every row must start on a 16-byte boundary (the rule of s3_cell_sample)
    return dispatch_rows<WidestRowWidth>(dtype, row_width<WidestRowWidth>(dtype, g.field, g.row_len, g.in_stride), [&](auto row) {
        using T = typename decltype(row)::type;
        constexpr int VEC = decltype(row)::vec;
        return dim == 2 ? launch_iso<T, VEC, 2, EMIT>(who, g) : launch_iso<T, VEC, 3, EMIT>(who, g);
    });
}

}  // namespace

}  // namespace s3

using namespace s3;

extern "C" {

int s3_iso_count(const void *d_field, int dtype, int64_t row_len, int64_t in_stride, int64_t n_nodes, const int32_t *d_faces, int64_t n_cells,
                 int dim, double level, int32_t *d_count, s3_stream stream) {
    const IsoArgs g{d_field, row_len, in_stride, n_nodes, d_faces, n_cells, level, d_count, nullptr, 0, nullptr, nullptr, nullptr, nullptr,
                    as_stream(stream)};
    return iso_pass<false>("s3_iso_count", g, dtype, dim);
}

int s3_iso_emit(const void *d_field, int dtype, int64_t row_len, int64_t in_stride, int64_t n_nodes, const int32_t *d_faces, int64_t n_cells,
                int dim, double level, const double *d_nodes, const int32_t *d_offset, int64_t capacity, double *d_verts, int32_t *d_edges,
                double *d_frac, int32_t *d_cells, s3_stream stream) {
    const IsoArgs g{d_field, row_len, in_stride, n_nodes, d_faces, n_cells, level, const_cast<int32_t *>(d_offset), d_nodes, capacity, d_verts,
                    d_edges, d_frac, d_cells, as_stream(stream)};
    return iso_pass<true>("s3_iso_emit", g, dtype, dim);
}

}  // extern "C"
