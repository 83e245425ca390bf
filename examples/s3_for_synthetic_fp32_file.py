"""
Single-precision S^3 file from end to end: the synthetic OAT15-style case of examples/s3_for_synthetic_OAT15.py (6 * 10^4 points,
200 snapshots by default) exported with ``file_dtype=torch.float32``, loaded back ONTO THE GPU and decomposed there:

    python examples/s3_for_synthetic_fp32_file.py [save_path] [n_snapshots]

The exported datasets hold the float64 interpolation result rounded once (the file is half as large as the float64 one; grid,
levels and metric stay float64); ``Dataloader.load_snapshot(..., device=True)`` returns the data matrix as a CUDA tensor, which
``compute_svd`` and ``DMD`` read where it lies.  Needs an MI355X and the HDF5 sink.
"""
import os
import sys
from os.path import abspath, dirname, join

import numpy as np
import torch as pt

sys.path.insert(0, dirname(dirname(abspath(__file__))))
sys.path.insert(0, dirname(abspath(__file__)))
from s3_for_synthetic_OAT15 import naca0012_outline, synthetic_fields                   # noqa: E402
from sparsespatialsampling_amd import DMD                                               # noqa: E402
from sparsespatialsampling_amd.data import Dataloader                                   # noqa: E402
from sparsespatialsampling_amd.export import ExportData                                 # noqa: E402
from sparsespatialsampling_amd.geometry import CubeGeometry, GeometryCoordinates2D      # noqa: E402
from sparsespatialsampling_amd.metrics import temporal_std                              # noqa: E402
from sparsespatialsampling_amd.sparse_spatial_sampling import SparseSpatialSampling     # noqa: E402
from sparsespatialsampling_amd.svd import compute_svd                                   # noqa: E402

if __name__ == "__main__":
    save_path = sys.argv[1] if len(sys.argv) > 1 else join("run", "OAT15_synthetic_fp32_file")
    n_snapshots = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    save_name, dt = "OAT15_synthetic_fp32", 1e-3

    rng = np.random.default_rng(1)
    outline = naca0012_outline()
    far = rng.random((30000, 2)) * [1.4, 1.0] + [-0.2, -0.5]
    near = outline[rng.integers(0, len(outline), 30000)] + 0.02 * rng.standard_normal((30000, 2))
    xz = np.concatenate([far, near])
    xz = np.ascontiguousarray(xz[(xz[:, 0] >= -0.2) & (xz[:, 0] <= 1.2) & (xz[:, 1] >= -0.5) & (xz[:, 1] <= 0.5)])
    write_times = [str(round(dt * i, 3)) for i in range(n_snapshots)]
    p = synthetic_fields(xz, 0, n_snapshots)[0]                             # [N, 1, T] float32

    bounds = [[-0.2, -0.5], [1.2, 0.5]]
    geometry = [CubeGeometry("domain", True, bounds[0], bounds[1]), GeometryCoordinates2D("OAT15", False, outline, refine=True)]
    s_cube = SparseSpatialSampling(pt.from_numpy(xz), temporal_std(p[:, 0, :]).reshape(-1), geometry, save_path, save_name, "OAT15",
                                   uniform_levels=5, n_cells_max=8000, max_delta_level=False)
    s_cube.execute_grid_generation()

    # batches of 50 snapshots, stored in single precision
    export = ExportData(s_cube, write_times=write_times, file_dtype=pt.float32)
    for t0 in range(0, n_snapshots, 50):
        export.export(pt.from_numpy(xz), p[:, :, t0:t0 + 50], "p", n_snapshots_total=n_snapshots)
    print(f"{join(save_path, save_name)}.h5: {os.path.getsize(join(save_path, save_name + '.h5'))} bytes")

    loader = Dataloader(save_path, save_name + ".h5")                       # float32 matrices, like the reference's default
    field = loader.load_snapshot("p", device=True)                          # [N_cells, T] on the GPU
    print(f"{xz.shape[0]} original points -> {tuple(field.shape)} {field.dtype} on {field.device}")

    s, u, v = compute_svd(field, loader.weights)
    print(f"weighted SVD: rank {len(s)}, leading singular values {[round(float(x), 4) for x in s[:4]]}")
    dmd = DMD(field, dt=dt, optimal=True, cell_area=loader.weights)
    top = dmd.top_modes(integral=True, f_min=0)[1:4]
    print("DMD, leading frequencies:", [round(float(dmd.frequency[int(i)]), 2) for i in top],
          f"largest reconstruction error of a snapshot {float(dmd.reconstruction_error.max()):.3e}")
