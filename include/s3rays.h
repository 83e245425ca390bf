/*
 * s3rays.h -- line-of-sight integrals of a grid field, exported from libs3hip.so next to the entry points of s3hip.h.
 *
 * The integral of a cell field or of the multilinear blend of a node field along straight rays through a generated grid: a numerical
 * schlieren or shadowgraph image, a column density, a spanwise average, a sinogram.  A cell field is piecewise constant on disjoint
 * dyadic boxes, so its integral along a line is sum value x chord, exactly; a blended node field is a polynomial of degree <= dim <= 3
 * in the ray parameter inside one cell, so two Gauss points per chord integrate it exactly too.  Plain C11; the caller owns every
 * array, nothing is allocated or kept by the library, and the entry point queues all its work on the stream it is given and returns
 * without waiting for it.
 *
 * Definition (normative; csrc/rays.hip and tests/ray_cases.py restate it).  Everything is plain f64, no contraction: an fma only
 * where one is written.  "max(a, b)" below is  b > a ? b : a,  "min(a, b)" is  b < a ? b : a,  with a the value held so far.
 *   grid        an s3_grid as s3_cell_index describes it: the lattice (origin, h_min, L = depth), the sorted Morton ranges and the
 *               cells.  2:1 balance is not assumed.
 *   ray         x(t) = o + t d, row r of d_origins and d_dirs (f64 [R][dim]).  BAD_RAY when an o_a or d_a is not finite or when d is
 *               zero: the output row is NaN, length 0, segments 0.  |d| = sqrt of the squares summed in axis order.  An axis with
 *               d_a == 0 is FIXED: it takes no part in any parameter (no 0 * inf), x_a = o_a, and its lattice index is
 *               floor((o_a - origin_a) / h_min) for the whole walk, the range test 0 <= . < 2^L before the integer conversion as in
 *               s3_cell_locate; where that fails the ray is MISSED.  This is the half-open rule: a ray lying in a face plane belongs to
 *               the upper cells only.  The other axes are MOVING.
 *   planes      tau_a(j) = (fma((double) j, h_min, origin_a) - o_a) / d_a: the parameter of lattice plane j of a moving axis.  Planes
 *               come from the lattice, not from cell centres, so a face shared by two leaves has ONE parameter and the chords of a
 *               ray telescope.
 *   block       an aligned cube of 2^s lattice cells per axis with the anchor a: a leaf or an empty block.  With i the lattice index
 *               that is looked up and k = key(i): the leaf whose range holds k (upper bound over the sorted starts, range test; s =
 *               L - level, a = (i >> s) << s), or, where k falls into a gap [g0, g1) between consecutive sorted ranges (bounded by 0
 *               and 2^(dim L) too), the EMPTY block of the largest s <= L with [k & ~(2^(dim s) - 1), that + 2^(dim s)) inside
 *               [g0, g1), a = (i >> s) << s.  Empty blocks contribute nothing; they let a ray cross a body or a coarse hole in
 *               O(depth) steps.
 *   chord       of a block: t_in = t_min, then max over the moving axes in axis order of tau_a(near plane); t_out = min over the
 *               moving axes in axis order of tau_a(far plane), the exit axis e the LOWEST axis that attains it; far plane = a_a + 2^s
 *               for d_a > 0, else a_a, the near plane the other one.  len = min(t_out, t_max) - t_in.  A leaf with len > 0 is a
 *               SEGMENT.
 *   segment     per component c and column t, one accumulator acc from 0 per (ray, c, t), segments added front to back:
 *                   S3_RAY_CELL     acc = fma((double) field[id][c][t], len, acc)
 *                   S3_RAY_LINEAR   half = len / 2, mid = t_in + half, g = half * 0.57735026918962576; for t_g = mid - g, then
 *                                   mid + g: x_a = fma(t_g, d_a, o_a) on the moving axes, b = the blend of s3_cell_sample at x in
 *                                   THAT leaf (xi with its clamp, one rounding per axis in a weight, the f64 fma chain over the corners
 *                                   in the order of d_faces from 0); acc = fma(half, b_1 + b_2, acc)
 *               and lenacc = lenacc + len, segments + 1.
 *   start       the domain is the block (a = 0, s = L).  Fixed axes first (above).  If its len is not > 0 the ray is MISSED: out 0,
 *               length 0, segments 0.  Else the first index of a moving axis is floor((fma(t_in, d_a, o_a) - origin_a) / h_min)
 *               clamped to [0, 2^L - 1] (NaN: 0); on every moving axis whose near plane has tau == t_in it is set exactly, to 0 for
 *               d_a > 0 and to 2^L - 1 otherwise.
 *   step        look the block of i up, take its chord, add the segment; that is one step.  The walk ends when t_out >= t_max.
 *               Otherwise i_e = a_e + 2^s for d_e > 0 and a_e - 1 for d_e < 0; the walk ends when that leaves [0, 2^L).  The other
 *               moving axes take floor((fma(t_out, d_a, o_a) - origin_a) / h_min) clamped into the block just left,
 *               [a_a, a_a + 2^s - 1] (NaN: a_a); fixed axes keep their index.  The exit axis is set in integers, never by a nudged
 *               point: the walk neither stalls on a face nor skips a thin cell.  A walk that has not ended after max_steps steps
 *               is TRUNCATED; what it has summed so far is written.
 *   bounds      every loop is bounded: the binary search by 32 iterations, the block search by L + 1, the walk by max_steps.
 *   broken      a leaf whose id is outside [0, n_cells) (S3_RAY_CELL: or outside [0, n_field_rows)) or whose level is outside
 *               [0, L] is BROKEN and is walked as the lattice cell i itself (s = 0); in S3_RAY_LINEAR a corner id outside
 *               [0, n_field_rows) makes the leaf BROKEN too (its own s).  Nothing is loaded through a broken leaf; a broken leaf with
 *               len > 0 makes every column of the ray's row NaN and the status BROKEN, and the walk goes on.
 *   NaN values  of the field propagate by arithmetic.
 *   outputs     out[r][c][t] = |d| * acc, d_length[r] = |d| * lenacc (the length of the ray inside leaves; both 0 for a ray without
 *               segments, whatever |d| is), d_segments[r], and
 *               d_status[r]: S3_RAY_BAD_RAY, else S3_RAY_MISSED from the start, else S3_RAY_BROKEN, else S3_RAY_TRUNCATED, else
 *               S3_RAY_CROSSED with >= 1 segment and S3_RAY_MISSED with none (only holes were crossed).
 * No atomics, no reductions across lanes: the bits depend on neither row_len, n_comp, the pitches, the batch split, d_order, the
 * element type (an f32 field gives the bits of its f64 copy) nor the run.
 *
 * s3_ray_integrate, one launch per snapshot batch: d_field rows [n_comp][row_len] f32 or f64 (dtype: S3_DTYPE_*) with pitch in_stride
 * ELEMENTS (0 = n_comp * row_len), read where they lie; n_comp is 1, 2 or 3 per launch (a wider field goes in groups: offset d_field
 * and d_out, keep the pitches), exactly as s3_cell_sample.  In S3_RAY_CELL the field lives on the cells (n_field_rows of them) and
 * grid->d_faces is not read; in S3_RAY_LINEAR it lives on the nodes and grid->d_faces is required.  Row r of d_out (f64, pitch
 * out_stride elements, 0 = n_comp * row_len) receives [n_comp][row_len].  Launch slot j takes ray d_order[j] (NULL: ray j; an entry
 * outside [0, R) writes nothing).  t_min <= t_max are launch scalars in units of the ray parameter, -inf .. +inf the whole line; NaN is
 * refused.  1 <= max_steps.  R * row_len < 2^31.
 */
#ifndef S3RAYS_H
#define S3RAYS_H

#include "s3hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define S3_RAY_CELL 0
#define S3_RAY_LINEAR 1

#define S3_RAY_CROSSED 0
#define S3_RAY_MISSED 1
#define S3_RAY_BAD_RAY 2
#define S3_RAY_TRUNCATED 3
#define S3_RAY_BROKEN 4

int s3_ray_integrate(int mode, const s3_grid *grid, const double *d_origins /*[R,dim]*/, const double *d_dirs /*[R,dim]*/, int64_t n_rays,
                     const int32_t *d_order /*[R] or NULL*/, double t_min, double t_max, int64_t max_steps, const void *d_field, int dtype,
                     int n_comp, int64_t row_len, int64_t in_stride, int64_t n_field_rows, double *d_out, int64_t out_stride,
                     double *d_length /*[R]*/, int32_t *d_segments /*[R]*/, int32_t *d_status /*[R]*/, s3_stream stream);

#ifdef __cplusplus
}
#endif

#endif
