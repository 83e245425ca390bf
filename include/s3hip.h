/*
 * s3hip.h -- C ABI of libs3hip.so: the MI355X (gfx950) implementation of the S^3 hot path.
 *
 * The reference (JanisGeise/sparseSpatialSampling) is pure Python and has no FFI; its boundary for this path is the
 * set of Python call sites listed per function below (file:line relative to the reference checkout).  A maintainer
 * binds this library with ctypes.  Conventions:
 *
 *   - every pointer named d_* is a DEVICE pointer (HBM of the current HIP device); h_* are host pointers;
 *   - arrays are dense row-major; `double` = IEEE f64; indices are int32 on the device (N < 2^31);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous on that stream unless
 *     stated otherwise; nothing allocates inside a call except s3_knn_create / s3_malloc;
 *   - return value 0 = success, negative = error (S3_E*); s3_last_error() returns the message of the last failure on
 *     the calling thread;
 *   - there is NO CPU fallback: without a HIP device every compute entry point fails with S3_ENODEV.
 *
 * Cell conventions (reference s_cube.py:188-194, 399-445): a cell is (centre[dim] f64, level i32); children and
 * nodes are enumerated in the reference's direction-table order; child centre = centre + dir*(0.25*width)/2^level,
 * node = centre + dir*(0.5*width)/2^level.
 */
#ifndef S3HIP_H
#define S3HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S3_OK 0
#define S3_EINVAL (-1)   /* bad argument (shape, k, dim, null pointer) */
#define S3_ENODEV (-2)   /* no usable HIP device */
#define S3_EHIP (-3)     /* HIP runtime error, see s3_last_error() */
#define S3_ENOMEM (-4)

#define S3_DTYPE_F32 0
#define S3_DTYPE_F64 1

#define S3_MAX_K 64

/* what s3_abi_version() of a library built from this header returns; the bindings refuse a library that reports another
 * number (a stale build) with the command that rebuilds it */
#define S3_ABI_VERSION 18

typedef struct s3_knn s3_knn; /* opaque: grid-sorted copy of the original point cloud, resident in HBM */
typedef void *s3_stream;

/* ---- runtime / plumbing ------------------------------------------------------------------------------------ */
const char *s3_last_error(void);
int s3_abi_version(void);
/* stop and join the library's own host threads (transfer lanes); returns their number.  Call once at process exit, before the
 * HIP runtime goes away (the Python bindings register it with atexit); safe at any time -- later calls start new lanes. */
int s3_shutdown(void);
/* debugging aid: install a SIGABRT handler that prints the native frames of the aborting thread to stderr, then aborts as usual */
int s3_debug_abort_backtrace(void);
int s3_device_count(int *h_count);
int s3_set_device(int device);
int s3_malloc(void **d_ptr, size_t bytes);
int s3_free(void *d_ptr);
/* host <-> device copies.  PAGE-LOCKED host memory (hipHostMalloc / s3_host_register): one asynchronous copy on `stream`.  PAGEABLE
 * host memory is never handed to the runtime's copy engine (which would pin the caller's pages on the fly): it goes through the
 * library's page-locked lanes (s3_upload_rows / s3_download) and the call returns when the copy is complete. */
int s3_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes, s3_stream stream);
int s3_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes, s3_stream stream);
int s3_stream_synchronize(s3_stream stream);
/* device -> pageable host array through persistent pinned buffers drained by several host threads (a plain copy into
 * pageable memory runs at 12-15 GB/s); returns when h_dst is complete */
int s3_download(void *h_dst, const void *d_src, size_t bytes, s3_stream stream);
/* page-lock host memory that was not allocated through HIP (a POSIX shared-memory mapping shared by the ranks of a node) and
 * map it into the device's address space: *d_ptr is what kernels write through.  Undo with s3_host_unregister. */
int s3_host_register(void *h_ptr, size_t bytes, void **d_ptr);
int s3_host_unregister(void *h_ptr);
/* upload target of a snapshot batch (the .to(device) of a host tensor handed to ExportData.export, export.py:128-167):
 * pageable host rows [n_rows][row_bytes] -> device rows with pitch dst_pitch_bytes, staged through persistent pinned
 * buffers filled by several host threads; asynchronous on `stream` (the host data may be reused on return).  The
 * bytes between row_bytes and dst_pitch_bytes of every row but the last are padding and may be overwritten. */
int s3_upload_rows(const void *h_src, int64_t n_rows, int64_t row_bytes, void *d_dst, int64_t dst_pitch_bytes,
                   s3_stream stream);
/* the same for a selection of the host rows: row h_rows[i] of h_src becomes device row i.  A generated grid references
 * only the source points near its cell centres (k neighbours each): uploading just those rows cuts the PCIe volume by
 * the sparsity of the grid. */
int s3_upload_rows_indexed(const void *h_src, const int32_t *h_rows /*[n_sel]*/, int64_t n_sel, int64_t row_bytes,
                           void *d_dst, int64_t dst_pitch_bytes, s3_stream stream);
/* the same for a PIECE of every (selected) row: source row r (h_rows[i], or i when h_rows is NULL) starts at h_src +
 * r * src_row_stride_bytes + src_offset_bytes and contributes n_segments segments of segment_bytes, segment_stride_bytes
 * apart; device row i holds them back to back.  This is how ExportData pipelines one export() call (reference
 * export.py:128-167 hands over the whole batch [N, n_comp, T]): the snapshots [t0, t1) of a field are n_comp segments of
 * (t1 - t0) values, T values apart, so piece j + 1 crosses PCIe while piece j is interpolated and piece j - 1 comes back. */
int s3_upload_row_pieces(const void *h_src, const int32_t *h_rows /*[n_rows] or NULL*/, int64_t n_rows,
                         int64_t src_row_stride_bytes, int64_t src_offset_bytes, int n_segments, int64_t segment_bytes,
                         int64_t segment_stride_bytes, void *d_dst, int64_t dst_pitch_bytes, s3_stream stream);

/* ---- KNN index over the original CFD points -------------------------------------------------------------------
 * Replaces KNeighborsRegressor(...).fit(vertices, target)           s_cube.py:161-163
 *      and NearestNeighbors(...).fit(coordinates)                   export.py:120,423
 * Builds a two-level bucket index on the device (bounding box, counting sort into a uniform grid; buckets holding more
 * than 8x the target occupancy get their own sub-lattice, which keeps strongly graded clouds fast).  Synchronous
 * (returns after the build finished).  `target_occupancy` <= 0 selects the default (3 points per bucket in 2-D, 8 in
 * 3-D). */
int s3_knn_create(const double *d_pts /*[n,dim]*/, int64_t n, int dim, double target_occupancy, s3_stream stream,
                  s3_knn **out);
void s3_knn_destroy(s3_knn *knn);
int s3_knn_info(const s3_knn *knn, int64_t *h_n_buckets, int64_t *h_n_refined);
/* attach the regression target y[n] (the S^3 metric, original point order); permuted into grid order */
int s3_knn_set_values(s3_knn *knn, const double *d_y /*[n]*/, s3_stream stream);

/* exact k nearest neighbours, ascending in (distance, original index); dist = sqrt(sum_j (q_j-p_j)^2).
 * Replaces NearestNeighbors.kneighbors(centers)                      export.py:425,438 */
int s3_knn_query(const s3_knn *knn, const double *d_q /*[nq,dim]*/, int64_t nq, int k, int32_t *d_idx /*[nq,k]*/,
                 double *d_dist /*[nq,k]*/, s3_stream stream);

/* inverse-distance KNN regression with scikit-learn's exact-hit rule and numpy's summation order.
 * Replaces self._knn.predict(...)                                    s_cube.py:224,328,372 */
int s3_idw_predict(const s3_knn *knn, const double *d_q /*[nq,dim]*/, int64_t nq, int k, double *d_yhat /*[nq]*/,
                   s3_stream stream);

/* ---- refine kernels ---------------------------------------------------------------------------------------- */
/* a3: children of `n_par` parents.  Child c of parent p_i gets cell id new_index + i*2^dim + c; its centre/level
 * are written into the cell arrays.  Replaces _compute_cell_centers(to_refine, keep_parent=False)
 *                                                                    s_cube.py:875,399-445 */
int s3_make_children(double *d_center /*[cap,dim]*/, int32_t *d_level /*[cap]*/, const int32_t *d_parents /*[n_par]*/,
                     int64_t n_par, int64_t new_index, int dim, double width, s3_stream stream);

/* a4: metric at the centre of each of n cells (ids first..first+n-1) and at its 2^dim candidate child centres, then
 * gain = level_factor[level] * sum_j |m0 - mj| / gain0.  d_level_factor[64] holds the reference's Python expression
 * 1/2^d*(width/2^level)^d evaluated on the host.  d_scratch: n*(2^dim+1) doubles.
 * Replaces SamplingTree._update_gain + _update_gain                  s_cube.py:207-241,1840-1859 */
int s3_child_gain(const s3_knn *knn, int k, const double *d_center, const int32_t *d_level, int64_t first, int64_t n,
                  int dim, double width, const double *d_level_factor, double gain0, double *d_metric /*[cap]*/,
                  double *d_gain /*[cap]*/, double *d_scratch, s3_stream stream);
/* the same with the predictions of a cell's 2^dim candidate child centres kept in d_child_metric[cap][2^dim]: the centre of
 * a new cell is candidate child c of its parent, a point the parent's call predicted already (same coordinates, same
 * deterministic search -- the reference predicts it a second time, s_cube.py:221-233, and obtains the same number), so with
 * d_parents given only the 2^dim child points of a new cell are searched (8 of 9 queries in 3-D) and its centre's value is
 * d_child_metric[parent][c].  The n cells first..first+n-1 are children number parents_offset.. of the ORDERED parents
 * d_parents[] (2^dim consecutive cells per parent, as s3_make_children creates them).  d_parents == NULL: all 2^dim + 1
 * points are searched (cells whose parent has no entry: the root).  Either way the children's values of the n cells are
 * stored in d_child_metric.  d_scratch: n*(2^dim+1) doubles + 2*(2 + n*2^dim) int32.  With d_parents every cell is given to
 * one wavefront (shared candidate box of the 2^dim child points; selection by histogram instead of sorted insertion:
 * csrc/knn.hip); the queries that scheme cannot answer are listed behind the doubles and handed on: to a grouped search
 * (2^dim queries per wavefront, each its own small box: cells too large for one box), then to one wavefront per query
 * (next to a body, at the edge of the cloud, outside it), and what is still left (refined buckets, ties in distance, k > 48)
 * to the per-lane search.  Same bits whichever kernel answers.
 * After a call with d_parents, the int32 words behind the n*(2^dim+1) doubles of d_scratch (R = that address, L = 2 + n*2^dim)
 * hold the hand-off counts, in child points: R[L+1] = what the per-cell wavefronts left to the grouped search, R[L] = what the
 * grouped search left to the one-wavefront-per-query search, R[0] = what that left to the per-lane search.  Without d_parents
 * these words are not touched. */
int s3_child_gain_reuse(const s3_knn *knn, int k, const double *d_center, const int32_t *d_level, int64_t first, int64_t n,
                        int dim, double width, const double *d_level_factor, double gain0, double *d_metric /*[cap]*/,
                        double *d_gain /*[cap]*/, double *d_scratch, const int32_t *d_parents /*or NULL*/,
                        int64_t parents_offset, double *d_child_metric /*[cap][2^dim]*/, s3_stream stream);

/* a12: geometry predicates on the nodes of cells.  s3_mask_cells describes the cells of a launch once, for every body; it is a
 * plain description of memory the caller owns, read during the call only.  Each call ORs its verdict into d_invalid[n] (zero it
 * first): GeometryObject._apply_mask policy, geometry_base.py:40-76.  Every s3_mask_* requires: a non-null struct; dim among the
 * body's dimensions (box, sphere: 2 | 3; polygon, triangle: 2; cylinder, prism, tetrahedra, mesh: 3); n >= 0 and first >= 0;
 * d_center, d_level and d_invalid non-null unless n == 0 (then nothing is launched).  All of it is checked before any launch. */
typedef struct s3_mask_cells {
    const double  *d_center;   /* [*, dim] */
    const int32_t *d_level;    /* [*] */
    const int32_t *d_cells;    /* [n] ordered ids, or NULL: the range first .. first+n-1 (first is ignored with a list) */
    int64_t first, n;
    int dim;                   /* 2 | 3 */
    double width;              /* of the root cell */
    uint8_t *d_invalid;        /* [n], OR-ed into */
} s3_mask_cells;
/*   box:      lo <= x <= hi in every dimension                       cube_geometry.py:50-74
 *   sphere:   ||x - pos|| <= radius                                  sphere_geometry.py:47-72
 *   cylinder: 0 <= proj <= norm && normal distance <= local radius   cylinder_geometry.py:126-157
 *   polygon:  strictly inside (boundary excluded)                    coordinates_2d.py:54-75
 *   triangle: edge cross products not of mixed sign (outline inside) triangle_geometry.py:80-103
 *   prism:    0 <= proj <= norm && in-plane point inside triangle    prism_geometry.py:90-118
 *   tetrahedra (1 = tetrahedron, 2 = the two halves of a pyramid, union): no inward face normal sees the point
 *             behind its face                                        tetrahedron_geometry.py:121-140,
 *                                                                    pyramid_geometry.py:156-170
 *   mesh (closed triangle surface): on the surface, or the +x ray crosses it an odd number of times -- the package's own
 *             exact rule (geometry/geometry_STL_3d.py states it per facet); stands in for vtkSelectEnclosedPoints of
 *                                                                    geometry_STL_3d.py:86-104 */
int s3_mask_box(const s3_mask_cells *cells, const double *h_lo /*[dim]*/, const double *h_hi /*[dim]*/, int refine_mode,
                int keep_inside, s3_stream stream);
int s3_mask_sphere(const s3_mask_cells *cells, const double *h_pos /*[dim]*/, double radius, int refine_mode, int keep_inside,
                   s3_stream stream);
int s3_mask_cylinder(const s3_mask_cells *cells, const double *h_p0, const double *h_axis, double norm, double r0, double r1,
                     int is_cone, int refine_mode, int keep_inside, s3_stream stream);
int s3_mask_polygon(const s3_mask_cells *cells, const double *d_poly /*[nv,2] device*/, int nv, int refine_mode,
                    int keep_inside, s3_stream stream);
int s3_mask_triangle(const s3_mask_cells *cells, const double *h_points /*[3][2]*/, int refine_mode, int keep_inside,
                     s3_stream stream);
int s3_mask_prism(const s3_mask_cells *cells, const double *h_origin /*[3] first point of the first triangle*/,
                  const double *h_axis /*[3] extrusion*/, double norm, const int32_t *h_dims /*[2] in-plane axes*/,
                  const double *h_triangle /*[3][2] first triangle in those axes*/, int refine_mode, int keep_inside,
                  s3_stream stream);
int s3_mask_tetrahedra(const s3_mask_cells *cells, const double *h_positions /*[n_tets][4][3]*/,
                       const double *h_normals /*[n_tets][3][4] inward, column p belongs to point p*/, int n_tets,
                       int refine_mode, int keep_inside, s3_stream stream);

/* d_tri: facets with their vertices in lexicographic (x, y, z) order; h_lo / h_hi: bounding box of the surface (a node outside
 * it is outside before any table is read); d_bin_start / d_bin_facet: CSR lists of a uniform ny x nz grid of (y, z) columns over
 * that box, column (iy, iz) at iy*nz + iz with i = clamp(floor((v - lo) * (n / (hi - lo))), 0, n - 1) (scale 0 for a flat extent),
 * each listing every facet whose closed projected bounding box touches the column (ny = nz = 1: all facets, brute force).  One
 * lane per (cell, node); facet ids must be < nt and bin_start[ny*nz] the length of d_bin_facet (not checked on the device). */
int s3_mask_mesh(const s3_mask_cells *cells, const double *d_tri /*[nt][3][3]*/, int nt, const double *h_lo /*[3]*/,
                 const double *h_hi /*[3]*/, const int32_t *d_bin_start /*[ny*nz+1]*/, const int32_t *d_bin_facet, int ny,
                 int nz, int refine_mode, int keep_inside, s3_stream stream);

/* bookkeeping of one refine batch on the device-resident cell arrays: parents stop being leaves, valid children
 * become leaves, invalid children get gain 0 (s_cube.py:721-723, 250-251) */
int s3_commit_batch(uint8_t *d_leaf /*[cap]*/, double *d_gain /*[cap]*/, const int32_t *d_parents, int64_t n_par,
                    int64_t first, int64_t n_new, const uint8_t *d_invalid /*[n_new] or NULL*/, s3_stream stream);

/* a6 local part: sum over leaf cells of metric^2 (the captured-metric numerator, s_cube.py:327-335), restricted to
 * cell ids in [begin, end) so that ranks can split the array; deterministic two-stage reduction.  d_out: 1 double.
 * d_scratch: 1024 doubles. */
int s3_sumsq_leaf(const double *d_metric, const uint8_t *d_leaf, int64_t begin, int64_t end, double *d_out,
                  double *d_scratch, s3_stream stream);

/* a8: the n_top leaf cells with the largest (gain, -id), ordered like heapq.nlargest (s_cube.py:601-602).
 * Radix select on the device, final ordering of the n_top survivors on the host: writes the ordered ids to the HOST
 * array h_out[n_top]; h_count receives min(n_top, #leaves).  Synchronous.  d_scratch: s3_topn_scratch_bytes(). */
size_t s3_topn_scratch_bytes(int64_t n_cells, int64_t n_top);
int s3_topn_leaf(const double *d_gain, const uint8_t *d_leaf, int64_t n_cells, int64_t n_top, int32_t *h_out,
                 int64_t *h_count, void *d_scratch, s3_stream stream);

/* ---- export kernels ---------------------------------------------------------------------------------------- */
/* a16: w = 1/clamp(dist, 1e-12), rows normalised to sum 1 (torch's summation order).  export.py:428-429 */
int s3_idw_weights(const double *d_dist /*[nc,k]*/, int64_t nc, int k, double *d_w /*[nc,k]*/, s3_stream stream);

/* a17/a18: out[c, l] = sum_m w[c,m] * data[idx[c,m], l], l over the contiguous (n_comp*T) axis, f64 accumulate,
 * f64 output.  Replaces interpolate_data                             export.py:446-468, and :215 with row_len=1 */
int s3_interp(const double *d_w /*[nc,k]*/, const int32_t *d_idx /*[nc,k]*/, int64_t nc, int k, const void *d_data,
              int dtype, int64_t n_src, int64_t row_len, double *d_out /*[nc,row_len]*/, s3_stream stream);

/* a19 hand-over: [nc][n_comp][T] -> [T][nc][n_comp], the snapshot-major image of an interpolated batch, so that the HDF5
 * sink (one dataset per snapshot, export.py:283-299) gets contiguous snapshots instead of slicing out[:, :, i] on the host. */
int s3_snapshot_major(const double *d_in, int64_t nc, int n_comp, int64_t n_snapshots, double *d_out, s3_stream stream);
/* the same for a SHARD of the cells (several ranks): input cell c becomes row d_rows[c] of an output with n_out
 * rows, [T][n_out][n_comp] -- every rank writes its rows of the one batch buffer the ranks share (host memory registered with
 * s3_host_register: the values cross this rank's own PCIe link, nothing is sent to the rank that writes the file). */
int s3_snapshot_major_rows(const double *d_in, int64_t nc, int n_comp, int64_t n_snapshots, const int32_t *d_rows /*[nc]*/,
                           int64_t n_out, double *d_out, s3_stream stream);
/* Both with the STORAGE TYPE of the file as an argument (out_dtype: S3_DTYPE_*; this build's addition, the reference always
 * stores float64 at export.py:283-299).  S3_DTYPE_F64: the bytes of the two entry points above.  S3_DTYPE_F32: every value is
 * rounded ONCE, to nearest even, after the float64 accumulation -- by integer arithmetic on the bit pattern, so the result is
 * the host's cast (numpy astype(float32)) whatever the kernel's denormal mode: ties, results that are f32 subnormals, +-0 for
 * magnitudes below 2^-150 (sign kept), +-inf from FLT_MAX + 2^103 on.  d_out then holds floats (4-byte aligned; the store
 * width follows the alignment of d_out and of the row length n_out * n_comp), download, staging and file bytes halve. */
int s3_snapshot_major_as(const double *d_in, int64_t nc, int n_comp, int64_t n_snapshots, int out_dtype, void *d_out,
                         s3_stream stream);
int s3_snapshot_major_rows_as(const double *d_in, int64_t nc, int n_comp, int64_t n_snapshots, const int32_t *d_rows /*[nc]*/,
                              int64_t n_out, int out_dtype, void *d_out, s3_stream stream);
/* The loader's inverse (reference data.py:249-300 reads one dataset per write time and stacks them on the host): n_snapshots
 * datasets [nc][n_comp] of in_dtype, back to back as the file holds them, become columns [t0, t0 + n_snapshots) of the
 * cell-major matrix d_out [nc][n_comp][n_cols] of out_dtype (row pitch out_stride >= n_cols elements) that SVD and DMD read.
 * f64 -> f32 rounds as above, f32 -> f64 is exact, equal types copy the bits.  Columns outside the range and the padding
 * of the rows are not written. */
int s3_cell_major(const void *d_in, int in_dtype, int64_t n_snapshots, int64_t nc, int n_comp, void *d_out, int out_dtype,
                  int64_t n_cols, int64_t out_stride, int64_t t0, s3_stream stream);

/* Metric upstream of S^3 (what the reference's example scripts compute with torch before the grid is generated:
 * metric = pt.std(field, dim=1), examples/s3_for_OAT15_airfoil.py:91): temporal mean and standard deviation of every row
 * of a snapshot matrix [n_rows][row_len] (row pitch in_stride elements, 0 = row_len), f64 accumulation, one pass over
 * the data.  ddof = 1: torch's default (unbiased), 0: population.  Either output may be NULL. */
int s3_row_moments(const void *d_data, int dtype, int64_t n_rows, int64_t row_len, int64_t in_stride, int ddof,
                   double *d_mean /*[n_rows] or NULL*/, double *d_std /*[n_rows] or NULL*/, s3_stream stream);
/* the same of |x|: mean_t sum_c |U_c| of a vector field [N, n_comp, T] (examples/s3_for_cylinder2D_Re100.py:55) is n_comp times
 * the mean over the cell's [n_comp * T] row */
int s3_row_abs_moments(const void *d_data, int dtype, int64_t n_rows, int64_t row_len, int64_t in_stride, int ddof,
                   double *d_mean /*[n_rows] or NULL*/, double *d_std /*[n_rows] or NULL*/, s3_stream stream);

/* Planned form of a17 for a static neighbour table (the table ExportData caches at export.py:431-432 and reuses for
 * every snapshot batch and field): the plan de-duplicates the source rows of spatially adjacent cells once (built on the
 * device; Hilbert order of d_centers[nc,dim] when given), the kernel then stages each distinct row once per tile in LDS.
 * Same results as s3_interp.  Source rows must start on 16-byte boundaries and be readable up to the next multiple of
 * 16 bytes (in_stride % 4 == 0 for f32 / % 2 == 0 for f64, in_stride >= row_len rounded up to that multiple); the row
 * length itself is arbitrary (25-snapshot batches of examples/s3_for_cylinder3D_Re3900.py:28-69: pitch 28 or 32).
 * Rows of up to 64 bytes take a short-row kernel (several workgroups per CU, no chunk pipeline); rows of up to 1 KiB on
 * plans with the reference's neighbour counts (k = 8 | 26, export.py:84-85) the persistent kernel (two workgroups per CU
 * walking all tiles, the next tile's rows / weights / ids in flight while the current one is accumulated). */
typedef struct s3_interp_plan s3_interp_plan;
int s3_interp_plan_create(const int32_t *d_idx /*[nc,k]*/, int64_t nc, int k, int64_t n_src,
                          const double *d_centers /*[nc,dim] or NULL*/, int dim, int tile_cells /*0 (=64), 64 or 128*/,
                          s3_stream stream, s3_interp_plan **out);
void s3_interp_plan_destroy(s3_interp_plan *plan);
int s3_interp_plan_info(const s3_interp_plan *plan, int64_t *h_n_tiles, int64_t *h_total_rows);
/* leaf-cell shards for `world` ranks: the plan's tiles (cells in Hilbert order: a run of tiles is a compact
 * blob of the grid) are cut into `world` consecutive runs of nearly equal cost = bytes the kernel moves per snapshot
 * (4 per staged source row, halo included, + 8 per output row + the weights' share).  d_order[nc] (may be NULL) receives
 * the plan's processing order (position -> cell id); rank r owns the cells d_order[h_cuts[r] .. h_cuts[r+1]).
 * h_cuts: world + 1 entries on the host. */
int s3_interp_plan_partition(const s3_interp_plan *plan, int world, int32_t *d_order, int64_t *h_cuts, s3_stream stream);
/* the same cost, cumulated along the plan's processing order and sampled at n_samples + 1 equally spaced cell positions
 * i * nc / n_samples (h_out[0] = 0, h_out[n_samples] = total; linear inside a tile): what a rank that holds the plan of ONE
 * stretch of the Hilbert curve publishes so that all ranks can cut the curve into stretches of equal cost without anybody
 * building the table of all cells (parallel.LeafShards) */
int s3_interp_plan_cost_profile(const s3_interp_plan *plan, int n_samples, double *h_out /*[n_samples + 1]*/, s3_stream stream);
/* in_stride: elements between consecutive source rows of d_data (>= row_len; 0 = row_len).  Rows padded to a multiple
 * of 128 bytes keep every staged segment on one cache line. */
/* the weights of the table, [nc,k] in the caller's cell order, are kept inside the plan in tile order (one contiguous
 * stream per tile): set them once per KNN cache, then pass d_w = NULL to s3_interp_planned; a non-NULL d_w re-attaches
 * the weights before the launch (one extra pass over the table) */
int s3_interp_plan_set_weights(s3_interp_plan *plan, const double *d_w /*[nc,k]*/, s3_stream stream);
int s3_interp_planned(s3_interp_plan *plan, const double *d_w /*[nc,k] or NULL*/, const void *d_data, int dtype,
                      int64_t row_len, int64_t in_stride, double *d_out /*[nc,row_len]*/, s3_stream stream);
/* A batch that already lives in HBM as the reference hands it over -- data[N, n_comp * T], every row of the CFD mesh,
 * export.py:446-468 -- is read WHERE IT LIES: no pass that first gathers the referenced rows into a pitched copy.
 *   s3_interp_plan_set_source_ids  d_ids[n_src]: the row of the full table behind each source row the plan was built on
 *                                  (the `used` list of s3_compact_rows); once per KNN cache
 *   s3_interp_planned_src          d_table[n_table_rows][in_stride]: the full batch; same results as s3_interp_planned on
 *                                  the gathered copy
 * Rows that are not 16-byte aligned (25 fp32 snapshots: 100-byte rows) are read with element alignment by the persistent
 * kernel (plans with k = 8 | 26, rows of at least 16 bytes); nothing beyond the end of a row is touched.  The same
 * relaxed alignment holds for s3_interp_planned on such plans. */
int s3_interp_plan_set_source_ids(s3_interp_plan *plan, const int32_t *d_ids /*[n_src]*/, int64_t n_table_rows, s3_stream stream);
int s3_interp_planned_src(s3_interp_plan *plan, const void *d_table, int dtype, int64_t n_table_rows, int64_t row_len,
                          int64_t in_stride, double *d_out /*[nc,row_len]*/, s3_stream stream);
/* Which kernel s3_interp_planned (src = 0) or s3_interp_planned_src (src != 0) would launch for these rows; launches nothing.
 * d_data is only looked at as an address.  h_out[5] = {route (S3_ROUTE_*), template width, EVEN, gy, tail}:
 *   width  K (8 | 26) of the persistent kernel (the three STREAM routes), KQ (2 | 7 | 8) of SHORT_QUAD, KM (8 | 26 | 32) of
 *          SHORT_REG; 0 for the others
 *   EVEN   the persistent kernel's even-row-length form (row_len even); 0 for the other routes
 *   gy     SHIFT / CHUNK*: workgroups that split the column chunks of a tile (1 = one workgroup per tile); 1 for the others
 *   tail   SHIFT / CHUNK*: the last tiles of every XCD's share are cut into runs (tail map); 0 for the others */
#define S3_ROUTE_STREAM_ELEM   1   /* persistent kernel, rows read with element alignment (not 16-byte aligned) */
#define S3_ROUTE_STREAM_WIDE   2   /* persistent kernel, 16-byte aligned rows of 5 .. 24 chunks of 128 bytes */
#define S3_ROUTE_STREAM_NARROW 3   /* persistent kernel, narrow layout: rows of two to four 16-byte vectors */
#define S3_ROUTE_SHORT_QUAD    4   /* rows of four vectors, k <= 32: the lanes of a cell share its tables (DPP quad) */
#define S3_ROUTE_SHORT_REG     5   /* rows of one to four vectors, k <= 32: weights in registers */
#define S3_ROUTE_SHORT         6   /* rows of one to four vectors, any k: the generic short-row kernel */
#define S3_ROUTE_SHIFT         7   /* 64-cell tiles, rows off the 128-byte grid: whole aligned lines per load */
#define S3_ROUTE_CHUNK64       8   /* chunk kernel, 64-cell tiles */
#define S3_ROUTE_CHUNK128      9   /* chunk kernel, 128-cell tiles */
int s3_interp_plan_route(const s3_interp_plan *plan, int src, const void *d_data, int dtype, int64_t row_len, int64_t in_stride,
                         int32_t *h_out /*[5]*/);

/* ---- reconstruction error: the exported fields back on the original CFD mesh (post_processing/compute_error_OAT.py:208-233) ----
 * The reverse direction of a17: the table is the generated grid (nc cell centres, small, cache resident), the targets are the n
 * points of the original mesh.  The reference fits KNeighborsRegressor(n_neighbors = 8 | 26, weights="distance") on the centres,
 * predicts the whole field at the points ([n, T] f64 on the host) and reduces it to T + 1 + 2n numbers; here the prediction lives
 * in registers only.
 *
 * s3_idw_weights_exact: scikit-learn's "distance" weights as the regressor applies them: a row with zero distances gets 1 at the
 * zeros and 0 elsewhere, any other row 1/dist, and either way the row is normalised to sum 1.  NOT s3_idw_weights, whose
 * 1/clamp(dist, 1e-12) belongs to export.py:428 (a point ON a cell centre gets 1e-10 of its neighbours there).
 *
 * s3_recon_error, one launch per snapshot batch.  Point i of the launch (i < n) is original row r = d_rows[i] (d_rows NULL: r = i,
 * n_orig = n); d_w / d_idx / d_scale are in LAUNCH order (launch the points in the order of s3_spatial_order: neighbouring lanes
 * then gather the same few grid rows), d_idx holds rows of d_grid (< nc, not checked on the device).  For every element l < row_len
 *     fit = sum_{m<k} w[i,m] * grid[idx[i,m], l]      f64 fma chain over m = 0..k-1: the value does not depend on row_len
 *     d   = s * (fit - orig[r, l]),   ref = s * orig[r, l]             s = d_scale[i], 1 without d_scale
 * and the outputs are
 *     d_mean[r], d_m2[r]   mean and centred second moment sum (|d| - mean)^2 of |d| over the row's row_len values (chunk mean first,
 *                          then squared deviations, chunks merged with Chan's update: s3_row_moments' scheme, so that batches merge
 *                          the same way); rows that are no point of the launch are not touched
 *     d_colsum[2][row_len] sum_i d^2 and sum_i ref^2 per column: partial sums over blocks of S3_RECON_BLOCK consecutive points of the
 *                          launch order, reduced by a second small kernel in a fixed order
 * No floating-point atomics: the same inputs give the same bits on every run.  d_grid [nc][row_len] dense; d_orig rows with pitch
 * orig_stride >= row_len elements (0 = row_len), any alignment; both f32 or f64 independently.  d_scratch:
 * s3_recon_error_scratch_bytes(n, row_len) bytes. */
#define S3_RECON_BLOCK 1024
int s3_idw_weights_exact(const double *d_dist /*[n,k]*/, int64_t n, int k, double *d_w /*[n,k]*/, s3_stream stream);
size_t s3_recon_error_scratch_bytes(int64_t n, int64_t row_len);
int s3_recon_error(const double *d_w /*[n,k]*/, const int32_t *d_idx /*[n,k]*/, int64_t n, int k, const void *d_grid,
                   int grid_dtype, int64_t nc, const void *d_orig, int orig_dtype, int64_t n_orig, int64_t orig_stride,
                   int64_t row_len, const int32_t *d_rows /*[n] or NULL*/, const double *d_scale /*[n] or NULL*/,
                   double *d_mean /*[n_orig]*/, double *d_m2 /*[n_orig]*/, double *d_colsum /*[2][row_len]*/, void *d_scratch,
                   s3_stream stream);

/* ---- spatial derivatives on a point cloud (csrc/differential.hip; no counterpart in the reference) -----------------------------
 * Weighted least-squares gradients over the k nearest neighbours of every point of a cloud x [n][dim] (dim 2 | 3), and the
 * quantities derived from them.  For entry j of the tables, which describes point i = d_rows[j] (d_rows NULL: i = j; launch the
 * points in the order of s3_spatial_order), with the neighbours d_idx[j][m], m < k, none of them i itself:
 *     dx_m = x[idx_m] - x_i,  r_m = |dx_m|,  h = max_m r_m,  dxs_m = dx_m / h,  rs_m = r_m / h
 *     w_m  = rs_m^-power (power 0 | 1 | 2), 0 where r_m = 0 (a coincident copy says nothing about the slope)
 *     M    = sum_m w_m dxs_m dxs_m^T = L L^T                      c[j][m][:] = w_m * M^-1 dxs_m / h
 * A row is DEGENERATE when h = 0 or a pivot of the Cholesky factorisation (the value under its square root) is <= 2^-40 trace(M):
 * collinear / coplanar neighbours.  Its coefficients are all zero and d_flag[j] = 1 (0 otherwise); *h_n_degenerate counts them.
 * s3_grad_coeff returns when the tables are complete.
 *
 * s3_grad_apply, one launch per snapshot batch: d_field rows [n_comp][row_len] f32 or f64 (dtype: S3_DTYPE_*) with pitch in_stride
 * ELEMENTS (0 = n_comp * row_len), read where they lie; row r of the field belongs to point r.  With
 *     G[a][b][t] = sum_{m<k} c[j][m][b] * (f[idx_m][a][t] - f[i][a][t])      f64 fma chain over m = 0..k-1 from 0; the difference is
 *                                                                           formed in f64 first: a constant field gives exact zeros
 * row i = d_rows[j] of d_out (f64, pitch out_stride elements, 0 = n_out * row_len) receives [n_out][row_len]:
 *     S3_GRAD_GRADIENT             G, ordered [comp][axis][t]                          n_out = n_comp * dim
 *     S3_GRAD_MAGNITUDE            sqrt(sum_b G[a][b]^2) per component a               n_out = n_comp
 *     S3_GRAD_DIVERGENCE           sum_a G[a][a]                                       n_out = 1        (these four: n_comp == dim)
 *     S3_GRAD_VORTICITY            G[1][0] - G[0][1] in 2-D; (G[2][1] - G[1][2], G[0][2] - G[2][0], G[1][0] - G[0][1]) in 3-D
 *     S3_GRAD_VORTICITY_MAGNITUDE  Euclidean norm of the vorticity                     n_out = 1
 *     S3_GRAD_Q                    -1/2 sum_ab G[a][b] G[b][a]                         n_out = 1
 * n_comp is 1, 2 or 3 per launch; a wider field goes in groups of components (offset d_field and d_out, keep the pitches).  The
 * gradient entries stay in registers: only the requested quantity is written.  d_idx holds rows of the field (< n, not checked on
 * the device).  No floating-point atomics: the same inputs give the same bits on every run, whatever row_len and n_comp. */
#define S3_GRAD_GRADIENT 0
#define S3_GRAD_MAGNITUDE 1
#define S3_GRAD_DIVERGENCE 2
#define S3_GRAD_VORTICITY 3
#define S3_GRAD_VORTICITY_MAGNITUDE 4
#define S3_GRAD_Q 5
int s3_grad_coeff(const double *d_pts /*[n,dim]*/, int64_t n, int dim, const int32_t *d_idx /*[n,k]*/, int k, int power,
                  const int32_t *d_rows /*[n] or NULL*/, double *d_coef /*[n,k,dim]*/, uint8_t *d_flag /*[n]*/,
                  int64_t *h_n_degenerate, s3_stream stream);
int s3_grad_apply(const double *d_coef /*[n,k,dim]*/, const int32_t *d_idx /*[n,k]*/, int64_t n, int k, int dim, const void *d_field,
                  int dtype, int n_comp, int64_t row_len, int64_t in_stride, const int32_t *d_rows /*[n] or NULL*/, int mode,
                  double *d_out, int64_t out_stride, s3_stream stream);

/* ---- sampling a grid field at arbitrary positions by exact cell location (csrc/sample.hip; no counterpart in the reference) ----
 * A generated grid is a set of disjoint axis-aligned dyadic boxes: cell j has the centre c_j [dim] (dim 2 | 3), the level l_j and the
 * edge h(l_j) = width / 2^l_j, `width` being the size of the initial cell.  The root's position is not an input (S^3 files do not
 * store it); a lattice is derived instead.  With L = max l, lmin = min l, h_min = h(L), H = h(lmin), per axis and in plain f64:
 *     corner = c_j - H/2 for the first cell j of level lmin        lo = min over the cells of c - h/2
 *     origin = corner - ceil((corner - lo)/H - 1e-9) * H
 *     a      = rint(((c - h/2) - origin) / h_min)                  the anchor of a leaf: an integer vector, a multiple of 2^(L-l)
 *     key(i) = bit b of i[axis] at position b*dim + axis           the leaf owns the keys [key(a), key(a) + 2^(dim (L-l)))
 * s3_grid describes such a grid once, for every entry point that looks something up in it (here and in the tracer below).  It is a
 * plain description of memory the caller owns; nothing is allocated or kept by the library:
 *     d_starts, d_ends, d_ids      the index: sorted range starts and ends (uint64 keys) and the cell of each range, n_cells entries each
 *     dim, depth, origin, h_min    the lattice: dim 2 | 3, depth = L, origin[3] (the entries past dim are not read), h_min = h(L)
 *     n_cells, d_centers, d_levels, width      the grid itself: centres [n_cells][dim] f64, levels [n_cells] int32, the initial cell size
 *     d_faces                      [n_cells][2^dim] int32, the corner nodes of every cell; NULL where no node field is read
 * An entry point that takes a grid requires: n_cells in [1, 2^31), dim 2 | 3, depth >= 0 and dim * depth <= 63, h_min > 0, width finite
 * and positive and, when there is work, every array but d_faces non-null; d_faces non-null where the mode reads node fields.
 * Which leaf lies across each face of a cell (s3_cell_neighbours: the same-or-coarser leaf or -1) is stated with the connected regions below.
 *
 * s3_cell_index computes the keys on the device, sorts (key, cell) with s3_sort_pairs and checks that the sorted ranges are
 * disjoint.  It writes the sorted range starts, ends and cell ids (d_starts, d_ends, d_ids: n entries each) and returns when they
 * are complete; then *h_grid describes the grid: these three arrays, the lattice, n, d_centers, d_levels and width, d_faces NULL
 * (the caller sets it).  A grid is REFUSED with S3_EINVAL, *h_grid untouched, the counts in h_refused[4]: [0] cells with an anchor
 * more than 1e-6 lattice units off an integer or outside [0, 2^L), [1] cells whose anchor is no multiple of 2^(L-l), [2] sorted
 * ranges that reach into their successor, [3] dim * L where that exceeds 63.  2:1 balance is not assumed.
 *
 * s3_cell_locate, one query per thread: i = floor((x - origin)/h_min) per axis (half-open: a point on a face belongs to the upper
 * cell), binary search of key(i) over the sorted starts, range test.  d_out[q] (int32, one entry per point, caller's cell
 * numbering) = the cell that holds point q, or -1 where no leaf does: outside the domain, inside a body, NaN or infinite
 * coordinates (tested before the conversion to an integer).  Thread j takes point d_rows[j] (d_rows NULL: point j; launch the
 * points in the order of s3_spatial_order).
 *
 * s3_cell_sample, one launch per snapshot batch: d_field rows [n_comp][row_len] f32 or f64 (dtype: S3_DTYPE_*) with pitch in_stride
 * ELEMENTS (0 = n_comp * row_len), read where they lie; n_comp is 1, 2 or 3 per launch (a wider field goes in groups: offset d_field
 * and d_out, keep the pitches).  Row q of d_out (f64, pitch out_stride elements, 0 = n_comp * row_len) receives [n_comp][row_len]
 * for point q = d_rows[j] (d_rows NULL: q = j) with id = d_cell[q]:
 *     S3_SAMPLE_CELL    (double) field[id]: a bit-exact copy; n_field_rows = rows of the field (cells).  grid and d_points are not
 *                       read (NULL will do).
 *     S3_SAMPLE_LINEAR  the field lives on the grid NODES (n_field_rows of them), grid->d_faces lists the corners of a
 *                       cell in the order (-,-), (-,+), (+,+), (+,-) in 2-D and that order at z+, then at z-, in 3-D:
 *                           xi_a = clamp((x_a - (c_a - h/2)) / h, 0, 1)                                    in f64, as written
 *                           w_m  = prod_a (s_ma > 0 ? xi_a : 1 - xi_a), evaluated as t = (s_m0 > 0 ? xi_0 : 1 - xi_0), then
 *                                  t = s_ma > 0 ? t * xi_a : fma(-xi_a, t, t) for a = 1 .. dim-1           one rounding per axis
 *                           out  = sum_m w_m f[faces[id][m]]                  f64 fma chain over m = 0 .. 2^dim - 1 from 0
 *                       The weights are formed in the kernel; nothing of size [nq][2^dim] is stored.
 * In both modes a row with id outside [0, n_cells) (-1: no cell) or with a corner outside [0, n_field_rows) is NaN in every column.
 * No floating-point atomics: the same inputs give the same bits on every run, whatever row_len and n_comp. */
#define S3_SAMPLE_CELL 0
#define S3_SAMPLE_LINEAR 1
typedef struct s3_grid {
    const uint64_t *d_starts, *d_ends; /*[n_cells]*/
    const int32_t *d_ids;              /*[n_cells]*/
    int dim, depth;
    double origin[3], h_min;
    int64_t n_cells;
    const double *d_centers;           /*[n_cells,dim]*/
    const int32_t *d_levels;           /*[n_cells]*/
    double width;
    const int32_t *d_faces;            /*[n_cells,2^dim] or NULL*/
} s3_grid;
int s3_cell_index(const double *d_centers /*[n,dim]*/, const int32_t *d_levels /*[n]*/, int64_t n, int dim, double width,
                  uint64_t *d_starts /*[n]*/, uint64_t *d_ends /*[n]*/, int32_t *d_ids /*[n]*/, s3_grid *h_grid,
                  int64_t *h_refused /*[4]*/, s3_stream stream);
int s3_cell_locate(const s3_grid *grid, const double *d_points /*[nq,dim]*/, int64_t nq, const int32_t *d_rows /*[nq] or NULL*/,
                   int32_t *d_out /*[nq]*/, s3_stream stream);
int s3_cell_sample(int mode, const int32_t *d_cell /*[nq]*/, int64_t nq, const int32_t *d_rows /*[nq] or NULL*/, const void *d_field,
                   int dtype, int n_comp, int64_t row_len, int64_t in_stride, int64_t n_field_rows, const s3_grid *grid,
                   const double *d_points /*[nq,dim]*/, double *d_out, int64_t out_stride, s3_stream stream);

/* ---- streamlines and pathlines of node velocity fields (csrc/trace.hip; no counterpart in the reference) ----
 * The grid is the s3_grid of s3_cell_index with d_faces set (its fields are stated there); the velocity lives on the grid NODES:
 * d_field rows [dim][row_len] f32 or f64 (dtype: S3_DTYPE_*) with pitch in_stride ELEMENTS (0 = dim * row_len), read where they lie, component c of node n at column t at
 * d_field[n * in_stride + c * row_len + t].  One lane per particle carries the whole loop.  This text is normative.
 *   velocity    at a position x in column t: the cell s3_cell_locate gives x (floored f64 lattice quotient, range test before the
 *               integer conversion, half-open cells, the upper cell on a face) and the S3_SAMPLE_LINEAR blend of its 2^dim corner rows
 *               (the xi clamp, one rounding per axis in a weight, the f64 fma chain over the corners in the order of d_faces from 0):
 *               the bits s3_cell_sample returns at x.
 *   time        S3_TRACE_PATH only.  A snapshot interval [c, c+1] takes `substeps` RK4 steps; the stage s in {0, 1/2, 1} of step m sits
 *               at p / (2 substeps) from column c, with the integer p = 2m + 2s forward and 2 substeps - (2m + 2s) backward.
 *                   p < 2 substeps: n = c, theta = (double) p / (double) (2 substeps)     p = 2 substeps: n = c + 1, theta = 0
 *                   where that n is the last column: n = row_len - 2, theta = 1
 *                   v(x) = fma(theta, v_{n+1}(x) - v_n(x), v_n(x))  per component, both blends in the same cell
 *               (n = floor(tau), theta = tau - n for tau = c + p / (2 substeps), without the rounding of forming tau).  Forward the
 *               intervals run c = 0 .. row_len - 2, backward c = row_len - 2 .. 0.
 *   one step    k1 = v(x); x2 = fma(dt/2, k1, x); k2 = v(x2); x3 = fma(dt/2, k2, x); k3 = v(x3); x4 = fma(dt, k3, x); k4 = v(x4);
 *               x' = fma(dt/6, (k1 + k4) + 2 (k2 + k3), x)  per component, in f64 as written.
 *   step size   S3_TRACE_STEP_TIME: dt = direction * step (pathlines: step = snapshot spacing / substeps, formed by the caller).
 *               S3_TRACE_STEP_CELL (streamlines only): dt = direction * ((step * h) / |k1|) with h the edge of the cell of x, step the
 *               CFL number and |k1| = sqrt((k1_0 k1_0 + k1_1 k1_1) + k1_2 k1_2), every product and sum rounded on its own.
 *   particles   S3_TRACE_STREAM: (seed, column) pairs, n_seeds * row_len of them; column t of the field is a steady velocity of its own;
 *               n_steps steps each.  S3_TRACE_PATH: the seeds; (row_len - 1) * substeps steps each (n_steps and every are not read).
 *   the end     the seed is located first; one that no cell holds has length 0, status S3_TRACE_SEED_OUTSIDE and only NaN rows.  A step
 *               is accepted only when x2, x3, x4 and x' all have a cell (the cell of x' is the next step's first locate, done once);
 *               otherwise the particle stays at x with status S3_TRACE_LEFT and x' is not recorded: a path holds points inside the grid
 *               only.  A cell whose id, level or one of whose corner ids is out of range counts as missing: nothing is loaded through
 *               them.  S3_TRACE_STEP_CELL with |k1| zero or not finite: S3_TRACE_STAGNANT.  All steps taken: S3_TRACE_DONE.
 *   output      d_paths f64: S3_TRACE_STREAM [n_seeds][row_len][n_out][dim], n_out = 1 + n_steps / every: row 0 the seed, row r the
 *               position after r * every accepted steps; S3_TRACE_PATH [n_seeds][row_len][dim]: the position at every snapshot, the
 *               seed in column 0 forward and in column row_len - 1 backward.  d_length (rows written, in the order they were written),
 *               d_status, d_cell (the cell of the last position, -1 for a seed outside): int32 [n_seeds][row_len] | [n_seeds].  Rows
 *               past the length are NaN.
 *   launch      slot j of the launch takes seed d_order[j] (NULL: seed j; pathlines: the order of s3_spatial_order).  Streamline
 *               lanes run the column fastest.  Terminated lanes idle; no compaction.
 * A lane remembers its leaf and skips the binary search for a stage point whose lattice index lies in the leaf's aligned box, an integer
 * test on the same quotient: the bits do not depend on it, nor on row_len, the order of the seeds, d_order, `every`, the element type
 * (an f32 field gives the bits of its f64 copy) or the run.  No atomics, no LDS. */
#define S3_TRACE_STREAM 0
#define S3_TRACE_PATH 1
#define S3_TRACE_STEP_TIME 0
#define S3_TRACE_STEP_CELL 1
#define S3_TRACE_DONE 0
#define S3_TRACE_LEFT 1
#define S3_TRACE_STAGNANT 2
#define S3_TRACE_SEED_OUTSIDE 3
int s3_trace(int mode, const s3_grid *grid, const void *d_field, int dtype, int64_t row_len, int64_t in_stride, int64_t n_nodes,
             const double *d_seeds /*[n_seeds,dim]*/, int64_t n_seeds, const int32_t *d_order /*[n_seeds] or NULL*/, int64_t n_steps,
             int substeps, int every, int step_rule, double step /*dt or cfl, > 0*/, int direction /*1 | -1*/, double *d_paths,
             int32_t *d_length, int32_t *d_status, int32_t *d_cell, s3_stream stream);

/* ---- isosurfaces (3-D) and contour lines (2-D) of node fields by marching simplices (csrc/iso.hip; no counterpart in the reference) ----
 * Inputs: d_nodes [n_nodes][dim] f64; d_faces [n_cells][2^dim] int32 in the corner order above ((-,-), (-,+), (+,+), (+,-) in 2-D;
 * that order at z+, then at z-, in 3-D); a field on the nodes, rows [row_len] f32 or f64 with pitch in_stride ELEMENTS (0 =
 * row_len), read where they lie; a finite level.  Centres, levels and the width of the grid are not needed.
 *   inside      node n at snapshot t iff (double) f[n][t] >= level: -0.0 is inside at level 0.0, a value equal to the level is inside
 *   nothing     is emitted at t by a cell with a corner value that is NaN or +-inf at t, or with a corner id outside [0, n_nodes)
 *               (nothing is loaded through such an id)
 *   simplices   for each permutation pi of the axes, in lexicographic order of pi, the path p_0 = (-, .., -), p_{i+1} = p_i with
 *               axis pi(i) switched to + (Kuhn): six tetrahedra around the diagonal from corner 4 to corner 2 of d_faces in 3-D, two
 *               triangles around the diagonal from corner 0 to corner 2 in 2-D.  The decomposition is translation invariant and
 *               matches across a face between two cells of one level; across a level jump the surface may crack at hanging nodes
 *               (documented, not repaired).
 *   primitives  of a simplex with path positions 0 .. dim, I the inside and O the outside positions, both ascending:
 *                 3-D, one position s alone on its side (|I| = 1 | 3): one triangle over the edges (s,a), (s,b), (s,c), a < b < c
 *                 3-D, I = {i,j}, O = {k,l}: the quad (i,k), (i,l), (j,l), (j,k) as the triangles (q0,q1,q2) and (q0,q2,q3)
 *                 2-D: one segment over (s,a), (s,b)
 *               per cell and snapshot sum over the simplices of min(|I|, dim + 1 - |I|): at most 12 in 3-D and 2 in 2-D
 *   orientation the right-hand normal of a triangle points to the side f < level; in 2-D the side f >= level lies to the left of
 *               q0 -> q1.  Where the natural order above gives the opposite, the last two vertices of the primitive are swapped
 *               (both triangles of a quad together); that depends on the parity of pi and the inside mask only.
 *   vertex      on a crossing edge, between the nodes a < b in GLOBAL node id whatever its direction in the simplex, in f64 as written:
 *                 t = (level - f_a) / (f_b - f_a)        x = fma(t, x_b - x_a, x_a) per axis
 *               t lies in [0, 1]; the same edge gives the same bits in every simplex and cell that shares it, so the output can be
 *               welded by the key (a, b) without a tolerance.  Degenerate primitives (a vertex exactly on a node) are kept.
 *   output      primitives ordered by (snapshot, cell in the caller's numbering, simplex, primitive within the simplex):
 *               d_verts [n][dim][dim] f64, d_edges [n][dim][2] int32 (a < b), d_frac [n][dim] f64 (t), d_cells [n] int32
 * s3_iso_count writes d_count[t][cell] (int32 [row_len][n_cells]); the caller scans it in place (s3_exclusive_scan, elem_bytes 4:
 * positions never come from atomics) and reads back the total; s3_iso_emit takes the scan as d_offset and writes the primitives of
 * (t, cell) at d_offset[t][cell] .. .  A (t, cell) whose offset equals its successor's does no further work; nothing is written at a
 * position outside [0, capacity), whatever d_offset holds.  Both refuse a batch with 12 * n_cells * row_len >= 2^31 (2 * .. in 2-D).
 * The bits depend on neither row_len, the load width, the element type (an f32 field gives the bits of its f64 copy) nor the run. */
int s3_iso_count(const void *d_field, int dtype, int64_t row_len, int64_t in_stride, int64_t n_nodes, const int32_t *d_faces /*[n_cells,2^dim]*/,
                 int64_t n_cells, int dim, double level, int32_t *d_count /*[row_len,n_cells]*/, s3_stream stream);
int s3_iso_emit(const void *d_field, int dtype, int64_t row_len, int64_t in_stride, int64_t n_nodes, const int32_t *d_faces /*[n_cells,2^dim]*/,
                int64_t n_cells, int dim, double level, const double *d_nodes /*[n_nodes,dim]*/, const int32_t *d_offset /*[row_len,n_cells]*/,
                int64_t capacity, double *d_verts /*[capacity,dim,dim]*/, int32_t *d_edges /*[capacity,dim,2]*/, double *d_frac /*[capacity,dim]*/,
                int32_t *d_cells /*[capacity]*/, s3_stream stream);

/* ---- connected regions of thresholded cell fields (csrc/regions.hip; no counterpart in the reference) ----
 * The grid is the s3_grid of s3_cell_index (d_faces is not read).  This text is normative.
 *   neighbours  face f = 2 * axis + side of cell c, side 0 the lower face.  With the anchor a and the level l of c as s3_cell_index derives
 *               them and s = 2^(L-l), the lattice cell looked up is a with a[axis] - 1 (side 0) or a[axis] + s (side 1) in place of a[axis];
 *               a coordinate outside [0, 2^L) is the domain edge.
 *                   nbr[c][f] = j   if a leaf j holds that lattice cell (key, binary search and range test of s3_cell_locate) and l_j <= l_c
 *                   nbr[c][f] = -1  otherwise: the domain edge, a body or a hole, or FINER cells across the face
 *               The table holds every pair of leaves that share a face of positive area exactly once from the finer side, and from both
 *               sides at equal level; 2:1 balance is not assumed.  s3_cell_neighbours writes d_nbr [n_cells][2 dim] int32, one lane per cell.
 *   in          cell c at column t iff lo <= (double) f[c][t] <= hi.  NaN is out; lo = -inf and hi = +inf are allowed, NaN bounds are not.
 *               d_field: rows [row_len] f32 or f64 (dtype: S3_DTYPE_*) with pitch in_stride ELEMENTS (0 = row_len), read where they lie.
 *   labels      d_labels int32 [n_cells][row_len] with pitch out_stride (0 = row_len): -1 where the cell is out, otherwise the SMALLEST cell id,
 *               in the caller's numbering, among the in-cells connected to c at column t through pairs of the table (shared faces; edges and
 *               corners do not connect).  A pure function of the inputs: the bits do not depend on the run, the batch split, row_len, the
 *               pitches, d_order or the element type (an f32 field gives the bits of its f64 copy).
 *               s3_region_label runs the phases named by `phases` (S3_REGION_ALL for a labelling; single phases for measurements), each a
 *               launch of its own: S3_REGION_INIT labels[c][t] = in ? c : -1; S3_REGION_HOOK union-find per column on the label array itself
 *               (for every table pair with two in-ends the larger root is hooked under the smaller one by an agent-scope compare-and-swap;
 *               every value ever stored at (x, t) is <= x, so every chase and every retry strictly decreases: no lane waits for another);
 *               S3_REGION_FLATTEN labels[c][t] = its root.  d_order [n_cells] or NULL: the order in which the hooking launch takes the cells
 *               (s3_spatial_order of the centres).  No floating-point atomics.
 *   table       a root is a (c, t) with labels[c][t] == c.  s3_region_count writes d_count[t][c] = 1 for a root, 0 otherwise (int32
 *               [row_len][n_cells], snapshot-major); the caller scans it in place with one entry more (s3_exclusive_scan, elem_bytes 4): the
 *               scan at [t][0] is where column t's slice of the table starts, the last entry the number of regions.  Region r of column t is
 *               the r-th root of the column by ascending cell id.  s3_region_emit takes the scan as d_offset and writes for each of the
 *               n_regions regions, with h = width / 2^l and V = h * h (2-D) or (h * h) * h (3-D) in f64 as written, over the cells of the region:
 *                   d_label int32 the root; d_n_cells int64; d_volume f64 = sum V; d_centroid f64 [dim] = (sum V c) / (sum V);
 *                   d_lo / d_hi f64 [dim] = min of c - h/2 / max of c + h/2 (f64 as written)
 *               and with a second cell field d_weight (g; rows like d_field with pitch weight_stride; NULL: none, the three arrays are not
 *               written): d_integral = sum V g, d_g_min / d_g_max = fmin / fmax over (double) g from +inf / -inf.
 *               Counts, the box and the extrema are exact.  Every sum runs over the cells of the region in ascending id in a fixed order
 *               without atomics: lane k of 16 takes the cells k, k + 16, .. (volume: adds; numerator and integral: fma(V, x, acc) from 0),
 *               then lane += lane + 8, + 4, + 2, + 1; a region of more than 1024 cells: thread k of 256 takes the cells k, k + 256, ..,
 *               then lane += lane + 32, .., + 1 in each of the four wavefronts, then wavefront 0 += 1, += 2, += 3.  The order depends on
 *               the size of the region alone: equal inputs give equal bits.  A label that names no root counts as out.
 * s3_region_label, s3_region_count and s3_region_emit refuse n_cells * row_len >= 2^31 - 1: split the batch. */
#define S3_REGION_INIT 1
#define S3_REGION_HOOK 2
#define S3_REGION_FLATTEN 4
#define S3_REGION_ALL 7
int s3_cell_neighbours(const s3_grid *grid, int32_t *d_nbr /*[n_cells,2*dim]*/, s3_stream stream);
int s3_region_label(const void *d_field, int dtype, int64_t row_len, int64_t in_stride, const int32_t *d_nbr /*[n_cells,2*dim]*/, int64_t n_cells,
                    int dim, double lo, double hi, const int32_t *d_order /*[n_cells] or NULL*/, int phases, int32_t *d_labels, int64_t out_stride,
                    s3_stream stream);
int s3_region_count(const int32_t *d_labels, int64_t row_len, int64_t label_stride, int64_t n_cells, int32_t *d_count /*[row_len,n_cells]*/,
                    s3_stream stream);
int s3_region_emit(const int32_t *d_labels, int64_t row_len, int64_t label_stride, const s3_grid *grid,
                   const int32_t *d_offset /*[row_len*n_cells+1]*/, int64_t n_regions, const void *d_weight /*or NULL*/, int dtype,
                   int64_t weight_stride, int32_t *d_label /*[n_regions]*/, int64_t *d_n_cells /*[n_regions]*/, double *d_volume /*[n_regions]*/,
                   double *d_centroid /*[n_regions,dim]*/, double *d_lo /*[n_regions,dim]*/, double *d_hi /*[n_regions,dim]*/,
                   double *d_integral /*[n_regions]*/, double *d_g_min /*[n_regions]*/, double *d_g_max /*[n_regions]*/, s3_stream stream);

/* ---- yardsticks of the measurement (bench.py's roofline line; no counterpart in the reference, not on any product path) ----
 * s3_yard_stream      a hand-written streaming kernel over d_src: every lane reads `reads` 16-byte vectors (coalesced) and
 *                     writes `writes` vectors derived from them; (reads, writes) = (1, 1) float4 copy, (7, 2) the read / write
 *                     mix of the headline launch (78 % / 22 %), (4, 0) reads only.  Short-lived workgroups, one contiguous block each (the
 *                     fastest form measured, csrc/yardstick.hip).
 *                     *h_bytes_read / *h_bytes_written = what the launch moved.
 * s3_yard_plan_loads  the loads of a tile plan and nothing else, at the headline kernel's occupancy and load schedule, on the
 *                     table s3_interp_planned_src reads (n_table_rows > 0) or s3_interp_planned's compacted one (0):
 *                     variant 0 one 128-byte line of a row per visit (the shift kernel's schedule), variant 1 two consecutive
 *                     lines (256 contiguous bytes) per visit with the same bytes and loads in flight.  *h_staged_bytes =
 *                     rows staged over all tiles x lines x 128. */
int s3_yard_stream(const void *d_src, void *d_dst, int64_t src_bytes, int64_t dst_bytes, int reads, int writes,
                   int nontemporal, s3_stream stream, int64_t *h_bytes_read, int64_t *h_bytes_written);
int s3_yard_plan_loads(s3_interp_plan *plan, const void *d_table, int64_t n_table_rows, int64_t row_bytes, int64_t stride_bytes,
                       int variant, s3_stream stream, int64_t *h_staged_bytes);


/* ---- device-side bookkeeping of the KNN cache (replaces torch.unique / fancy indexing on the a16 path) ----------
 * A generated grid that is sparser than the CFD mesh references only part of the source rows (export.py:403-444 keeps
 * the full table; here only the referenced rows are uploaded per batch):
 *   s3_mark_rows     d_flag[idx[i]] = 1 for every entry of a neighbour table (d_flag zeroed by the caller, int32[n_src])
 *   s3_compact_rows  d_flag -> remap in place (position among the marked rows, ascending row id; -1 = unused),
 *                    d_used[0..n_used) = the marked row ids ascending; *h_n_used = their number
 *   s3_remap_indices idx[i] = d_remap[idx[i]] in place
 *   s3_gather_rows   d_dst row i (pitch dst_pitch_bytes) = d_src row ids[i] (ids NULL: row i), row_bytes % 4 == 0:
 *                    the device-side form of the indexed upload for batches that already live in HBM, and the re-pitch
 *                    of dense ragged rows for s3_interp_planned */
int s3_mark_rows(const int32_t *d_idx, int64_t n, int64_t n_src, int32_t *d_flag, s3_stream stream);
int s3_compact_rows(int32_t *d_flag_remap /*[n_src] in: 0/1, out: remap*/, int64_t n_src, int32_t *d_used /*[n_src]*/,
                    int64_t *h_n_used, s3_stream stream);
int s3_remap_indices(int32_t *d_idx, int64_t n, const int32_t *d_remap, int64_t n_src, s3_stream stream);
/* Hilbert-curve order of n points [n,dim] (dim 2 | 3): d_perm[position] = point.  The export path keeps the referenced
 * source rows in this order in HBM, so that the rows a tile of neighbouring cells gathers lie close together (fewer
 * DRAM pages / address translations per tile than with the CFD mesh's arbitrary numbering). */
int s3_spatial_order(const double *d_points, int64_t n, int dim, int32_t *d_perm, s3_stream stream);
/* The two device-wide primitives behind the planner and the device topology (csrc/scan_sort.h, hand-written: three-launch
 * exclusive scan; stable LSD radix sort with 8-bit digits), exported for the tests.  s3_exclusive_scan: d_out[i] = sum of
 * d_in[0 .. i-1], int32 (elem_bytes 4) or int64 (8), in place allowed.  s3_sort_pairs: (key, value) pairs ascending by the low
 * `bits` bits of the keys, stable, in place.  Both return when the work is done.  No counterpart in the reference (torch.unique /
 * numpy fancy indexing do this work there, export.py:403-444). */
int s3_exclusive_scan(const void *d_in, void *d_out, int64_t n, int elem_bytes, s3_stream stream);
int s3_sort_pairs(uint64_t *d_keys, int32_t *d_vals, int64_t n, int bits, s3_stream stream);
/* d_remap[d_ids[i]] = i for the n distinct row ids, every other entry of d_remap[n_src] = -1 */
int s3_positions_of(const int32_t *d_ids, int64_t n, int32_t *d_remap, int64_t n_src, s3_stream stream);
int s3_gather_rows(const void *d_src, int64_t n_src_rows, int64_t row_bytes, int64_t src_pitch_bytes,
                   const int32_t *d_ids /*[n] or NULL*/, int64_t n, void *d_dst, int64_t dst_pitch_bytes, s3_stream stream);


/* ---- multi-GPU (one process per GPU, RCCL over xGMI) -----------------------------------------------------
 * The interpolation shards over the generated cells with no collective.  The refine loop has one exchange per batch:
 * every rank evaluates s3_child_gain for its 1/W slice of the new cells (the reference farms the same work out to a
 * process pool, s_cube.py:207-241) and ONE grouped in-place all-gather returns metric and gain to everybody
 * (s3_comm_allgather_inplace); the captured metric (s_cube.py:317-336) is reduced as per-block partial sums
 * (s3_sumsq_blocks, every rank a share of the blocks), gathered the same way and added in block order on every rank
 * (s3_sum_ordered), so that the result is bit-identical for any number of ranks.
 * Bootstrap: rank 0 calls s3_comm_unique_id and hands the 128 bytes to the other ranks by any host channel. */
typedef struct s3_comm s3_comm;
#define S3_COMM_ID_BYTES 128
/* 1 when the RCCL library can be loaded in this process (creates nothing, never blocks): ranks exchange this BEFORE anybody
 * enters s3_comm_init, whose ncclCommInitRank is a collective without a timeout */
int s3_comm_available(void);
int s3_comm_unique_id(void *h_id_out, size_t bytes /* >= S3_COMM_ID_BYTES */);
int s3_comm_init(const void *h_id, size_t bytes, int rank, int world, s3_comm **out);   /* the current device is used */
void s3_comm_destroy(s3_comm *comm);
int s3_comm_rank(const s3_comm *comm, int *rank, int *world);
int s3_comm_allgather_inplace(s3_comm *comm, void *const *d_arrays, const size_t *bytes_per_rank, int n_arrays,
                              s3_stream stream);
/* every rank's block to ONE rank (the one that writes the export's file): rank r sends bytes_per_rank[r] bytes from d_send,
 * `root` receives the blocks in rank order into d_recv (d_recv may be NULL on the other ranks).  Point-to-point sends in one
 * group: every byte crosses xGMI once, where an all-gather would deliver all blocks to every rank. */
int s3_comm_gather_to_root(s3_comm *comm, const void *d_send, void *d_recv, const size_t *bytes_per_rank /*[world]*/, int root,
                           s3_stream stream);
int s3_comm_allreduce_f64(s3_comm *comm, double *d_buf, int64_t n, int op /*0 sum, 1 max*/, s3_stream stream);
/* captured-metric numerator in a form that does not depend on how the work is split: partial[b] = sum of metric^2 over the
 * leaf cells of the 1024-cell block b (fixed reduction tree inside a block), for blocks [block_begin, block_end);
 * s3_sum_ordered adds n values in index order (fixed tree) into d_out[0] */
#define S3_SUMSQ_BLOCK 1024
int s3_sumsq_blocks(const double *d_metric, const uint8_t *d_leaf, int64_t n_cells, int64_t block_begin, int64_t block_end,
                    double *d_partial /*[n_blocks total], entries [block_begin, block_end) written*/, s3_stream stream);
int s3_sum_ordered(const double *d_values, int64_t n, double *d_out, s3_stream stream);


/* ---- weighted SVD downstream of S^3 (utils.py:302-346, data.py:240-247) -------------------------
 * G[t,t] = sum_n w[n] (x[n,:] - mean[n]) (x[n,:] - mean[n])^T over the rows of the interpolated snapshot matrix x
 * [n_rows, t] (f64, row pitch in_stride), accumulated with v_mfma_f64_16x16x4_f64; centring and weighting are fused into
 * the operand staging.  d_mean: temporal mean per row (s3_row_moments), d_weight: cell area / volume per row.  The
 * eigen-decomposition of the small G is a library call (sparsespatialsampling_amd/svd.py); the mode GEMM: s3_centered_gemm. */
size_t s3_weighted_gram_scratch_bytes(int64_t n_rows, int64_t t);
int s3_weighted_gram(const double *d_x, int64_t n_rows, int64_t t, int64_t in_stride, const double *d_mean,
                     const double *d_weight, double *d_gram /*[t,t]*/, void *d_scratch, s3_stream stream);

/* the tall GEMMs of the same SVD, on the same matrix cores (rows of L may be pitched: the interpolated matrix as it stands):
 *   d_e == NULL:  C = (L - lmean 1^T) B                    modes U = (X - mean) V S^-1 (utils.py:302-346 takes U from the SVD),
 *                                                           coefficients A = (X - mean) V of the directions already found
 *   d_e != NULL:  C = (E - emean 1^T) - (L - lmean 1^T) B   residual (X - mean) - A V^T of a deflation level, in row chunks
 * L [m][k] row pitch l_stride, B [k][n] contiguous, E [m][n] row pitch e_stride, C [m][n] contiguous; means may be NULL. */
int s3_centered_gemm(const double *d_l, int64_t m, int64_t k, int64_t l_stride, const double *d_lmean, const double *d_b,
                     int64_t n, const double *d_e, int64_t e_stride, const double *d_emean, double *d_c, s3_stream stream);

/* The same two kernels for a matrix read WHERE IT LIES, f32 or f64 (dtype: S3_DTYPE_*), behind the dynamic mode decomposition
 * (post_processing/compare_dmd_OAT.py:150-178; sparsespatialsampling_amd/dmd.py): the original CFD field is f32 and 20 GB at the
 * cylinder3D shape, a f64 copy of it is what these entry points avoid.  An f32 element is widened to f64 in the operand staging,
 * before centring and weighting; the MFMA part and the slice-ordered reduction are the ones above, so
 *   - s3_gram of an f32 matrix equals s3_gram of its f64 copy to the bit, and s3_tall_gemm likewise;
 *   - s3_gram(f64, mean, weight) equals s3_weighted_gram, s3_tall_gemm(f64) equals s3_centered_gemm without means and d_e.
 * s3_gram: d_mean NULL = no centring (DMD does not centre), d_weight NULL = 1.  s3_tall_gemm: C [m][n] = L [m][k] B [k][n], B and C
 * f64 contiguous.  Rows may be pitched (in_stride / l_stride in ELEMENTS) and need the element's alignment only: f32 rows that
 * are not all 16-byte aligned are read with 8- or 4-byte loads, chosen per launch from (pointer | stride * 4) & 15. */
size_t s3_gram_scratch_bytes(int64_t n_rows, int64_t t);
int s3_gram(const void *d_x, int dtype, int64_t n_rows, int64_t t, int64_t in_stride, const double *d_mean /*[n_rows] or NULL*/,
            const double *d_weight /*[n_rows] or NULL*/, double *d_gram /*[t,t]*/, void *d_scratch, s3_stream stream);
int s3_tall_gemm(const void *d_l, int dtype, int64_t m, int64_t k, int64_t l_stride, const double *d_b /*[k,n]*/, int64_t n,
                 double *d_c /*[m,n]*/, s3_stream stream);

/* Windowed DFT of the overlapping segments of every row, on the same matrix cores -- the step behind Welch spectra and spectral POD
 * (sparsespatialsampling_amd/spectral.py; the reference's post_processing/compare_svd_OAT.py:56-70 calls scipy.signal.welch).  Row i,
 * segment b (samples b * hop ... b * hop + nperseg - 1), frequency column f:
 *   c[i,b,f] = sum_l (x[i, b * hop + l] - mean[i]) (bre[l,f] + i bim[l,f])
 * d_x [n_rows][t] f32 or f64 (dtype: S3_DTYPE_*), read where it lies, row pitch in_stride ELEMENTS (f32 load width chosen per launch
 * from (pointer | in_stride * 4 | hop * 4) & 15); d_mean [n_rows] or NULL; d_bre / d_bim [nperseg][n_f] f64 contiguous: window,
 * detrend and twiddles of the caller's choice (any nperseg: a direct DFT).  Needs (n_blk - 1) * hop + nperseg <= t <= in_stride;
 * samples past the last segment are not read.
 *   s3_segment_dft: d_coef [n_rows][n_f][n_blk][2] f64 contiguous (Re, Im).  Frequency f's matrix is the pitched real
 *                   [n_rows][2 n_blk] matrix at d_coef + f * 2 * n_blk with row pitch n_f * n_blk * 2: s3_gram / s3_tall_gemm take it.
 *   s3_segment_psd: d_psd [n_rows][n_f] = d_scale[f] * sum_b |c[i,b,f]|^2, summed in registers in segment order and written once:
 *                   nothing of size n_rows * n_blk * n_f exists, no atomics, the same bits in every run. */
int s3_segment_dft(const void *d_x, int dtype, int64_t n_rows, int64_t t, int64_t in_stride, const double *d_mean /*[n_rows] or NULL*/,
                   int64_t nperseg, int64_t hop, int64_t n_blk, const double *d_bre, const double *d_bim, int64_t n_f,
                   double *d_coef /*[n_rows][n_f][n_blk][2]*/, s3_stream stream);
int s3_segment_psd(const void *d_x, int dtype, int64_t n_rows, int64_t t, int64_t in_stride, const double *d_mean /*[n_rows] or NULL*/,
                   int64_t nperseg, int64_t hop, int64_t n_blk, const double *d_bre, const double *d_bim, int64_t n_f,
                   const double *d_scale /*[n_f]*/, double *d_psd /*[n_rows][n_f]*/, s3_stream stream);

/* Symmetric eigenproblem of the T x T Gram matrix (the step between s3_weighted_gram and the modes; the reference gets the whole
 * decomposition from flowtorch.analysis.SVD, utils.py:302-346).  The one LIBRARY call of the SVD path: rocSOLVER's dsyevd, looked up
 * with dlopen at the first call (s3_sym_eig_available: 1 when it loads); the scaling to a unit diagonal maximum and back is done
 * around it.  d_g [t][t] symmetric (read only), d_lam [t] eigenvalues ASCENDING, d_vec [t][t] row-major with eigenvector j in ROW j,
 * d_scratch s3_sym_eig_scratch_bytes(t) bytes.  Complete on return. */
int s3_sym_eig_available(void);
size_t s3_sym_eig_scratch_bytes(int64_t t);
int s3_sym_eig(const double *d_g, int64_t t, double *d_lam, double *d_vec, void *d_scratch, s3_stream stream);

/* ---- device-resident topology of the sampling tree (a9-a11, a15) ------------------------------------------
 * Neighbour links, shared-node numbering, invalid-cell bookkeeping and the final renumbering of s_cube.py:904-1536,
 * 721-728, 734-772, 1695-1736 on tables that live in HBM.  Every update takes the ORDERED id list the host decided on
 * (the iteration order of the reference's sets) as a host array, copies it, and runs asynchronously on the engine's own
 * stream; the result is the one of the reference's sequential procedure (stale links included).  s3_topo_sync waits.
 * The host engine libs3topo.so (csrc/topology.cpp) implements the same operations and serves the 2:1-balance mode. */
typedef struct s3_topo s3_topo;
int s3_topo_create(int dim, double width, const double *h_root_center /*[dim]*/, s3_topo **out);
void s3_topo_destroy(s3_topo *topo);
/* children of the listed parents in list order (s_cube.py:879-895 / 531-544); relink != 0: all their links once more after
 * the batch (uniform levels, s_cube.py:547-549).  *h_first (may be NULL) = id of the first new cell */
int s3_topo_refine(s3_topo *topo, const int64_t *h_parents, int64_t n, int relink, int64_t *h_first);
/* cell.parent.children = _assign_neighbors(cell.parent, ...) for every listed cell, in list order (s_cube.py:609, 834) */
int s3_topo_relink_parent_of(s3_topo *topo, const int64_t *h_cells, int64_t n);
/* children = [] and removal from the neighbours' rows, in list order (s_cube.py:721-728) */
int s3_topo_mark_invalid(s3_topo *topo, const int64_t *h_cells, int64_t n);
/* wait for the submitted updates; *h_error: 0 ok, 1 a listed parent was not a leaf or listed twice, 2 internal (a node
 * reference chain of a batch did not resolve) */
int s3_topo_sync(s3_topo *topo, int64_t *h_n_cells, int64_t *h_n_nodes, int *h_error);
/* device pointer of a table: 0 level i32, 1 parent i32, 2 first_child i32 (-1 leaf, -2 invalid), 3 nb i32 [n][8|26],
 * 4 node_idx i64 [n][2^d], 5 center f64 [n][d], 6 nodes f64 [n_nodes][d]; valid until the next update */
int s3_topo_table(s3_topo *topo, int which, const void **d_ptr);
/* renumbering (s_cube.py:734-772): leaves, nodes that keep a slot; then the grid into the caller's DEVICE arrays:
 * faces [n_leaf][2^d] (int32 when as32, else int64; leaves in ascending cell id), nodes [n_unique][d] */
int s3_topo_finalize(s3_topo *topo, int64_t *h_n_leaf, int64_t *h_n_unique_nodes);
int s3_topo_export_grid(s3_topo *topo, void *d_faces, int as32, double *d_nodes);
/* centres [n][d] / levels [n] (int64) of the listed cells into DEVICE arrays */
int s3_topo_gather_cells(s3_topo *topo, const int64_t *h_ids, int64_t n, double *d_centers, int64_t *d_levels);

#ifdef __cplusplus
}
#endif
#endif /* S3HIP_H */
