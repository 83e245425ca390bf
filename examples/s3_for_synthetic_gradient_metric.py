"""
A derivative as the refinement metric.  S^3 refines where the metric is large; for a shock problem (the OAT15 buffet case) the natural
sensors are derivatives -- the time-mean ``|grad rho|`` (numerical schlieren), vorticity magnitude, Q -- not the temporal moments of
the raw field.  ``sparsespatialsampling_amd.Gradient`` computes them on the cloud of the original points on the GPU, so the metric
is one line and nothing is carried over from another tool.

    python examples/s3_for_synthetic_gradient_metric.py [save_path]

The synthetic density has a ``tanh`` front whose position oscillates in time, on a randomly numbered 2-D cloud.  Two grids with the
same ``n_cells_max`` are generated, one from ``std(rho)`` and one from the time-mean ``|grad rho|``, and exported; ``Gradient`` then
runs on each exported grid, and the script prints where the cells went: the share of the cells inside the band the front sweeps,
and the largest time-mean ``|grad rho|`` seen on the grid.  Needs an MI355X.
"""
import sys
from os.path import abspath, dirname, join

import torch as pt

sys.path.insert(0, dirname(dirname(abspath(__file__))))
from sparsespatialsampling_amd import Gradient                                          # noqa: E402
from sparsespatialsampling_amd.data import Dataloader                                   # noqa: E402
from sparsespatialsampling_amd.export import ExportData                                 # noqa: E402
from sparsespatialsampling_amd.geometry import CubeGeometry                             # noqa: E402
from sparsespatialsampling_amd.metrics import RunningMoments, temporal_mean, temporal_std   # noqa: E402
from sparsespatialsampling_amd.sparse_spatial_sampling import SparseSpatialSampling     # noqa: E402

if __name__ == "__main__":
    save_path = sys.argv[1] if len(sys.argv) > 1 else join("run", "gradient_metric_synthetic")

    # the synthetic "CFD" data: a front at x_s(y, t) = 1 + 0.15 sin(2 pi t / 50) + 0.1 (y - 0.5), thickness 0.02
    bounds = [[0.0, 0.0], [2.0, 1.0]]
    n_t = 200
    pt.manual_seed(0)
    coord = pt.rand(20000, 2) * pt.tensor(bounds[1])            # pt.rand numbers the points at random
    x, y, t = coord[:, 0:1], coord[:, 1:2], pt.arange(float(n_t))[None, :]
    front = 1.0 + 0.15 * pt.sin(2 * pt.pi * t / 50) + 0.1 * (y - 0.5)
    rho = (1.0 + 0.5 * pt.tanh((x - front) / 0.02) + 0.05 * pt.sin(2 * pt.pi * x) * pt.cos(2 * pt.pi * t / 20)).float()
    write_times = [str(round(0.01 * i, 2)) for i in range(n_t)]
    in_band = lambda c: ((c[:, 0] - 1.0 - 0.1 * (c[:, 1] - 0.5)).abs() <= 0.17)          # noqa: E731

    # the two metrics.  The schlieren arrives in snapshot batches, as with data too large to hold at once
    grad = Gradient(coord)
    schlieren = RunningMoments()
    for t0 in range(0, n_t, 50):
        schlieren.update(grad.magnitude(rho[:, t0:t0 + 50]))
    metrics = {"std_rho": temporal_std(rho), "mean_grad_rho": schlieren.mean()}

    print(f"{'metric':>14} {'cells':>8} {'cells in the front band':>24} {'max mean |grad rho| on the grid':>32}")
    for name, metric in metrics.items():
        domain = CubeGeometry("domain", True, bounds[0], bounds[1])
        s_cube = SparseSpatialSampling(coord, metric, [domain], save_path, name, "front2D", n_cells_max=6000)
        s_cube.execute_grid_generation()
        export = ExportData(s_cube, write_times=write_times)
        try:
            export.export(coord, rho.unsqueeze(1), "rho")
            loader = Dataloader(save_path, name + ".h5")
            on_grid = loader.load_snapshot("rho", write_times)
            grid_grad = Gradient.from_dataloader(loader)
            centers = loader.vertices
        except ImportError:                   # neither libs3h5.so nor h5py: take the interpolated field as it stands
            centers, on_grid = s_cube.centers, export._interpolated_fields.centers
            grid_grad = Gradient(centers)
        sensor = temporal_mean(grid_grad.magnitude(on_grid.reshape(len(centers), -1)))
        share = float(in_band(centers).double().mean())
        print(f"{name:>14} {len(centers):>8d} {share:>23.1%} {float(sensor.max()):>32.3f}")
