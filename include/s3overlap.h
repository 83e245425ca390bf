/*
 * s3overlap.h -- the overlap table of two label arrays of one grid, exported from libs3hip.so next to the entry points of s3hip.h.
 *
 * Which regions of A coincide with which regions of B, and by how much.  With A = labels[:, 0 : T-1] and B = labels[:, 1 : T] of one
 * labelling (two windows of one allocation, one pitch) the edges link every region of snapshot t to the regions of t + 1 it shares
 * cells with: the table behind tracking.  With two labellings of the same snapshots (Q above a threshold, pressure below one) they
 * say which regions of the one lie in which of the other.  Plain C11; the caller owns every array, nothing is allocated or kept
 * by the library, and every entry point queues all its work on the stream it is given and returns without waiting for it.
 *
 * Definitions (normative):
 *   inputs      a grid as s3_cell_index describes it (s3_grid; d_faces is not read) and two label arrays d_a, d_b: int32
 *               [n_cells][row_len] with pitches a_stride, b_stride in ELEMENTS (0 = row_len), read where they lie.
 *   in          cell c is IN X at column t iff 0 <= X[c][t] < n_cells and X[X[c][t]][t] == X[c][t]: the rule of s3_region_emit, a
 *               label that names no root counts as out.  Every end of an edge is therefore a row of the region table of its array.
 *   units       u(c) = 2^(dim (depth - level[c])): the volume of c in cells of the finest lattice, a uint64.  dim * depth <= 63 for
 *               every grid that has an index and the leaves are disjoint, so a sum of units over any set of cells is at most 2^63:
 *               it never wraps, it is an exact integer and any order of addition gives the same bits.
 *   edge        of column t: a pair (a, b) = (A[c][t], B[c][t]) that occurs at a cell c in both.  Per edge, over those cells:
 *                   d_src int32 = a; d_dst int32 = b; d_n_cells int64 = their number; d_units uint64 = sum u(c);
 *                   d_volume f64 = (double) units * hd, hd = h_min * h_min (2-D) or (h_min * h_min) * h_min (3-D), formed on the
 *                   host in f64 as written
 *               The edges of column t stand by ascending (a, b), one column after the other.  Everything is a pure function of the
 *               inputs: the bits do not depend on the run, the pitches, the batch split, the sort route or the launch order.
 *   chain       count -> scan -> emit -> sort -> heads -> scan -> reduce; no position comes from an atomic.
 *               s3_overlap_count writes d_count[t][c] = 1 where c is in both at t, else 0 (int32 [row_len][n_cells], snapshot-major);
 *               the caller scans it in place with one entry more (s3_exclusive_scan, elem_bytes 4): the scan at [t][0] is where the
 *               pairs of column t start, the last entry n_pairs.
 *               s3_overlap_emit writes one (key, cell) pair per in-both (c, t) at its scanned position (positions outside
 *               [0, n_pairs) are not written).  With w = the bits of n_cells - 1 (at least 1) and tb = the bits of row_len - 1:
 *                   S3_OVERLAP_ONE_KEY   key = t << 2w | a << w | b; the caller sorts by tb + 2w bits (s3_sort_pairs, stable)
 *                   S3_OVERLAP_BY_B      key = t << w | b; the caller sorts by the low w bits: by b alone
 *                   S3_OVERLAP_BY_TA     d_scan is not read: the key of every pair already there becomes t << w | a (a read from d_a at
 *                                        the pair's cell); the caller sorts by tb + w bits.  The sort is stable, so after the two
 *                                        passes the pairs stand by (t, a, b) as after the one key.
 *               One key holds (t, a, b) while tb + 2w <= 64; the two passes serve any shape.
 *               s3_overlap_heads writes d_head[j] = 1 where the sorted pair j is the first of its (t, a, b), else 0 (int32 [n_pairs];
 *               two_pass != 0: the keys are those of S3_OVERLAP_BY_TA and b is read from d_b).  The caller scans d_head in place with
 *               one entry more: x[j] = the heads before j, x[n_pairs] = n_edges, the edge of pair j is x[j + 1] - 1, and the scan at the
 *               first pair of column t is where the edges of column t start.
 *               s3_overlap_reduce takes that scan as d_edge and writes the five arrays of the n_edges edges.  d_n_cells is the length of
 *               the edge's run of pairs.  d_units: every wavefront sums the units of its pairs per run with shuffles and adds each
 *               partial sum with one 64-bit INTEGER atomic to the array, which the entry point zeroes first: exact in any order.
 *               No floating-point atomics, no lane waits for another lane.  A pair whose cell, level, column or edge number is out of
 *               range (arrays that do not belong together) is skipped, never followed.
 * All four refuse n_cells * row_len >= 2^31 - 1 with S3_EINVAL, as s3_region_* do: split the batch.
 */
#ifndef S3OVERLAP_H
#define S3OVERLAP_H

#include "s3hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define S3_OVERLAP_ONE_KEY 0
#define S3_OVERLAP_BY_B 1
#define S3_OVERLAP_BY_TA 2

int s3_overlap_count(const s3_grid *grid, const int32_t *d_a, int64_t a_stride, const int32_t *d_b, int64_t b_stride, int64_t row_len,
                     int32_t *d_count /*[row_len,n_cells]*/, s3_stream stream);
int s3_overlap_emit(const s3_grid *grid, const int32_t *d_a, int64_t a_stride, const int32_t *d_b, int64_t b_stride, int64_t row_len,
                    const int32_t *d_scan /*[row_len,n_cells]*/, int64_t n_pairs, int pass, uint64_t *d_keys /*[n_pairs]*/,
                    int32_t *d_vals /*[n_pairs]*/, s3_stream stream);
int s3_overlap_heads(const s3_grid *grid, const uint64_t *d_keys, const int32_t *d_vals, int64_t n_pairs, int two_pass, const int32_t *d_b,
                     int64_t b_stride, int64_t row_len, int32_t *d_head /*[n_pairs]*/, s3_stream stream);
int s3_overlap_reduce(const s3_grid *grid, const uint64_t *d_keys, const int32_t *d_vals, int64_t n_pairs, int two_pass, const int32_t *d_b,
                      int64_t b_stride, int64_t row_len, const int32_t *d_edge /*[n_pairs+1]*/, int64_t n_edges, int32_t *d_src, int32_t *d_dst,
                      int64_t *d_n_cells, uint64_t *d_units, double *d_volume, s3_stream stream);

#ifdef __cplusplus
}
#endif

#endif
