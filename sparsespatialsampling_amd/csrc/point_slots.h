// The work split of the kernels that gather rows for the points of a cloud in launch order (recon.hip, differential.hip, sample.hip, iso.hip, regions.hip; export.hip's
// interp_kernel and the planned kernels use the block order alone): the XCD-aware order of the blocks and the host choice of lanes per
// point slot, points per stage and chunks per row.  gfx950 only.
//
// A workgroup of 256 threads owns a block of consecutive points.  Its threads form 256 / LP point slots of LP lanes (LP = 4..64, the
// power of two that covers a row's VEC-wide pieces); a slot takes every (256 / LP)-th point of the block, its lane l the columns
// [(chunk * LP + l) * VEC, +VEC) of the row.  The block is walked in STAGES of stage_pts points (64 unless LDS is short): the tables of
// a whole stage (weights or coefficients, ids) are put into LDS between one pair of barriers, then the slots sweep the stage in
// stage_pts / (256 / LP) passes without a barrier.  Rows longer than LP * VEC columns are swept in chunks (chunk loop outside, stage and
// point loops inside), so a lane's columns are fixed while it walks its points; the price is that the block's tables are read from
// global memory and staged once PER CHUNK.  (The copy of a stage into LDS is a loop in each kernel: as a shared inline function it
// compiles to other instruction orders in grad_apply_kernel and interp_kernel.)
#ifndef S3_POINT_SLOTS_H
#define S3_POINT_SLOTS_H

#include "common.h"

namespace s3 {

// Consecutive blocks of the spatial order gather the same rows.  Workgroups that share blockIdx % 8 share an XCD's L2 (MI355X deals
// workgroups round-robin over its 8 XCDs), so each XCD walks one contiguous eighth of the blocks (speed only): workgroup b of a grid
// of 8 * per_xcd takes the block below, and returns at once if that is past the last one.
__device__ __forceinline__ int64_t xcd_block(int64_t b, int64_t per_xcd) { return (b & 7) * per_xcd + (b >> 3); }

struct XcdGrid {
    int64_t per_xcd, grid;
    bool fits() const { return grid < ((int64_t)1 << 31); }
};
inline XcdGrid xcd_grid(int64_t n_blocks) {
    const int64_t per_xcd = (n_blocks + 7) / 8;
    return XcdGrid{per_xcd, per_xcd * 8};
}

// LDS of a launch: `fixed` bytes (fixed_chunked instead where a row takes several chunks) and the tables of one stage of points, per_point
// bytes each -- up to 64 points, halved while the total exceeds POINT_LDS_MAX, never fewer than one pass of the slots.  At least 4 lanes
// per point, so at most 64 points' tables in LDS; short rows with many neighbours get fewer, wider slots until a pass fits.
constexpr int POINT_THREADS = 256;
constexpr size_t POINT_LDS_MAX = 48 * 1024;
struct SlotShape {
    int lanes, stage_pts;
    int64_t n_chunks;
    size_t lds_bytes;
};
inline int slot_shape(const char *who, int64_t row_len, int64_t pieces, size_t per_point, size_t fixed, size_t fixed_chunked, SlotShape &shape) {
    auto with = [&](int lanes) {
        const int64_t chunks = (pieces + lanes - 1) / lanes;
        const size_t rest = chunks > 1 ? fixed_chunked : fixed;
        int stage_pts = 64;
        while (stage_pts > POINT_THREADS / lanes && rest + stage_pts * per_point > POINT_LDS_MAX) stage_pts /= 2;
        return SlotShape{lanes, stage_pts, chunks, rest + stage_pts * per_point};
    };
    int lanes = 4;
    while (lanes < 64 && lanes < pieces) lanes *= 2;
    shape = with(lanes);
    while (shape.lanes < 64 && shape.lds_bytes > POINT_LDS_MAX) shape = with(shape.lanes * 2);
    S3_REQUIRE(shape.n_chunks < ((int64_t)1 << 20), "%s: row_len %lld too long", who, (long long)row_len);
    S3_REQUIRE(shape.lds_bytes <= POINT_LDS_MAX, "%s: %zu bytes of LDS needed", who, shape.lds_bytes);
    return S3_OK;
}

}  // namespace s3

#endif
