"""
Dynamic mode decomposition of the original field and of the field on the S^3 grid, side by side -- the call sequence of the
reference's post_processing/compare_dmd_OAT.py:150-178 without its plots, on the synthetic OAT15-style case of
examples/s3_for_synthetic_OAT15.py (smaller: 6 * 10^4 points, 400 snapshots by default):

    python examples/s3_for_synthetic_dmd.py [save_path] [n_snapshots]

The source field is float32 and is decomposed where it lies (no float64 copy); the exported field is weighted with the cell areas
of the grid.  Prints the leading eigenvalues and frequencies of both decompositions, ordered by their integral contribution, the
rank the optimal hard threshold selects and the largest reconstruction error of a snapshot.  Needs an MI355X.
"""
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

if __name__ == "__main__":
    save_path = sys.argv[1] if len(sys.argv) > 1 else join("run", "OAT15_synthetic_dmd")
    n_snapshots = int(sys.argv[2]) if len(sys.argv) > 2 else 400
    save_name, dt = "OAT15_synthetic_dmd", 1e-3

    rng = np.random.default_rng(1)
    outline = naca0012_outline()
    far = rng.random((30000, 2)) * [1.4, 1.0] + [-0.2, -0.5]
    near = outline[rng.integers(0, len(outline), 30000)] + 0.02 * rng.standard_normal((30000, 2))
    xz = np.concatenate([far, near])
    xz = np.ascontiguousarray(xz[(xz[:, 0] >= -0.2) & (xz[:, 0] <= 1.2) & (xz[:, 1] >= -0.5) & (xz[:, 1] <= 0.5)])
    write_times = [str(round(dt * i, 3)) for i in range(n_snapshots)]
    p = synthetic_fields(xz, 0, n_snapshots)[0]                             # [N, 1, T] float32
    p += 1e-3 * pt.randn(p.shape, generator=pt.Generator().manual_seed(0))
    orig_field = p[:, 0, :].cuda()                                          # resident, float32: read where it lies

    bounds = [[-0.2, -0.5], [1.2, 0.5]]
    geometry = [CubeGeometry("domain", True, bounds[0], bounds[1]), GeometryCoordinates2D("OAT15", False, outline, refine=True)]
    s_cube = SparseSpatialSampling(pt.from_numpy(xz), temporal_std(p[:, 0, :]).reshape(-1), geometry, save_path, save_name, "OAT15",
                                   uniform_levels=5, n_cells_max=8000, max_delta_level=False)
    s_cube.execute_grid_generation()
    export = ExportData(s_cube, write_times=write_times)
    try:
        export.export(pt.from_numpy(xz), p, "p")
        loader = Dataloader(save_path, save_name + ".h5")                   # (float32 by default, like the reference's)
        interpolated_field, cell_area = loader.load_snapshot("p", write_times), loader.weights
    except ImportError:                       # neither libs3h5.so nor h5py: take the interpolated field as it stands
        interpolated_field, cell_area = export._interpolated_fields.centers[:, 0, :], None
    interpolated_field = interpolated_field.reshape(interpolated_field.shape[0], -1)
    print(f"{xz.shape[0]} original points -> {interpolated_field.shape[0]} cells, {n_snapshots} snapshots")

    # the synthetic cloud has no cell areas: every point weighs the same (with CFD data: cell_area=cell_area_orig)
    dmd_orig = DMD(orig_field, dt=dt, optimal=True)
    dmd_inter = DMD(interpolated_field, dt=dt, optimal=True, cell_area=cell_area)
    print(f"optimal rank: original {dmd_orig.svd.opt_rank}, interpolated {dmd_inter.svd.opt_rank}")

    # sort the modes by their integral contribution, one member per conjugate pair, omit the mean value
    idx_orig = dmd_orig.top_modes(integral=True, f_min=0)[1:]
    idx_inter = dmd_inter.top_modes(integral=True, f_min=0)[1:]
    print(f"{'':>4} {'original: eigenvalue':>28} {'f':>9} {'interpolated: eigenvalue':>28} {'f':>9}")
    for i in range(min(6, len(idx_orig), len(idx_inter))):
        a, b = int(idx_orig[i]), int(idx_inter[i])
        la, lb = complex(dmd_orig.eigvals[a]), complex(dmd_inter.eigvals[b])
        print(f"{i + 1:>4} {la.real:>13.6f} {la.imag:>+13.6f}i {float(dmd_orig.frequency[a]):>9.3f} "
              f"{lb.real:>13.6f} {lb.imag:>+13.6f}i {float(dmd_inter.frequency[b]):>9.3f}")
    print(f"largest reconstruction error of a snapshot: original {float(dmd_orig.reconstruction_error.max()):.3e}, "
          f"interpolated {float(dmd_inter.reconstruction_error.max()):.3e}")
    snapshot = dmd_inter.reconstruction(100, 101)                           # one snapshot of the field on the grid, [N_cells, 1]
    print(f"reconstructed snapshot 100 on the grid: {tuple(snapshot.shape)}, modes {tuple(dmd_inter.modes.shape)}")
