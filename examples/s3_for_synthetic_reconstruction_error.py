"""
How good is the grid S^3 generated?  The reconstruction error of the reference's post-processing
(reference post_processing/compute_error_OAT.py:208-233) on the synthetic cylinder2D case of
examples/s3_for_synthetic_cylinder2D.py: the grid is generated for three values of ``min_metric``, the field is exported
onto each grid, interpolated BACK onto the original points and compared with the original field there.

    python examples/s3_for_synthetic_reconstruction_error.py [save_path]

Prints the total relative L2 error, the largest error of a snapshot and the largest time-averaged error of a point against
``min_metric`` -- the error-versus-metric curve of the S^3 paper.  Needs an MI355X.
"""
import sys
from os.path import abspath, dirname, join

import torch as pt

sys.path.insert(0, dirname(dirname(abspath(__file__))))
from sparsespatialsampling_amd import ReconstructionError                               # noqa: E402
from sparsespatialsampling_amd.data import Dataloader                                   # noqa: E402
from sparsespatialsampling_amd.export import ExportData                                 # noqa: E402
from sparsespatialsampling_amd.geometry import CubeGeometry, SphereGeometry             # noqa: E402
from sparsespatialsampling_amd.metrics import temporal_std                              # noqa: E402
from sparsespatialsampling_amd.sparse_spatial_sampling import SparseSpatialSampling     # noqa: E402

if __name__ == "__main__":
    save_path = sys.argv[1] if len(sys.argv) > 1 else join("run", "cylinder2D_synthetic_error")

    # the synthetic "CFD" data of s3_for_synthetic_cylinder2D.py
    bounds = [[0, 0], [2.2, 0.41]]
    cylinder = [[0.2, 0.2], 0.05]
    pt.manual_seed(0)
    coord = pt.rand(14000, 2) * pt.tensor(bounds[1])
    coord = coord[(coord - pt.tensor(cylinder[0])).norm(dim=1) > cylinder[1]]
    x, y, t = coord[:, 0:1], coord[:, 1:2], pt.arange(400.0)[None, :]
    wake = pt.exp(-((y - 0.2) / 0.08) ** 2) * pt.exp(-(x - 0.2).clamp(min=0)) * (x > 0.2)
    field = (wake * pt.sin(2 * pt.pi * (x - 0.2) / 0.4 - 2 * pt.pi * t / 40) + 1e-3 * pt.randn(len(coord), 400)).float()
    write_times = [str(round(0.01 * i, 2)) for i in range(400)]
    metric = temporal_std(field)
    # the synthetic cloud has no cell areas: every point weighs the same (with CFD data: the square roots of the cell areas,
    # ``cell_area_orig`` of the reference's script after its .sqrt())
    point_scale = None

    print(f"{'min_metric':>10} {'cells':>8} {'error_total':>12} {'max error_time':>15} {'max error_space_mean':>21}")
    for min_metric in (0.25, 0.50, 0.75):
        save_name = "metric_{:.2f}".format(min_metric)
        domain = CubeGeometry("domain", True, bounds[0], bounds[1])
        geometry = SphereGeometry("cylinder", False, cylinder[0], cylinder[1], refine=True, min_refinement_level=9)
        s_cube = SparseSpatialSampling(coord, metric, [domain, geometry], save_path, save_name, "cylinder2D",
                                       min_metric=min_metric)
        s_cube.execute_grid_generation()
        export = ExportData(s_cube, write_times=write_times)
        try:
            export.export(coord, field.unsqueeze(1), "p")
            loader = Dataloader(save_path, save_name + ".h5")
            centers, on_grid = loader.vertices, loader.load_snapshot("p", write_times)
        except ImportError:                   # neither libs3h5.so nor h5py: take the interpolated field as it stands
            centers, on_grid = s_cube.centers, export._interpolated_fields.centers
        original = field.reshape((len(coord),) + tuple(on_grid.shape[1:]))
        error = ReconstructionError(centers, coord, point_scale=point_scale)
        for t0 in range(0, 400, 100):         # snapshot batches: nothing of size N x T is ever held on the device
            error.update(on_grid[..., t0:t0 + 100], original[..., t0:t0 + 100])
        print(f"{min_metric:>10.2f} {centers.shape[0]:>8d} {error.error_total:>12.4e} {float(error.error_time.max()):>15.4e} "
              f"{float(error.error_space_mean.max()):>21.4e}")
