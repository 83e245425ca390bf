// Device-side plan construction (plan_build.hip), used by s3_interp_plan_create (interp_plan.hip).
#pragma once

#include "common.h"

namespace s3 {

// device tables of a plan (host only: no kernel takes the struct); whatever was allocated before an error goes with the struct
struct PlanTables {
    DevBuf<int32_t> perm;             // [nc] processing position -> cell id
    DevBuf<int32_t> tile_cell_begin;  // [n_tiles+1]
    DevBuf<int32_t> tile_row_begin;   // [n_tiles+1]
    DevBuf<int32_t> rows;             // [total_rows] distinct source rows, tile after tile
    DevBuf<uint16_t> loc;             // [nc*k] per tile: [m][cell in tile] -> position in the tile's row list
    int64_t n_tiles = 0, total_rows = 0;
};

// returns S3_OK or a negative S3_E* code (message in s3_last_error)
int build_plan_tables(const int32_t *d_idx, int64_t nc, int k, int64_t n_src, const double *d_centers, int dim, int tc,
                      int ucap, hipStream_t st, PlanTables *out);

}  // namespace s3
