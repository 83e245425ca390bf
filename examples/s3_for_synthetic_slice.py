"""
Looking at a field on the generated grid: a z-plane of vorticity magnitude through the synthetic 3-D cylinder, and the spectrum of
the velocity at a probe in its wake.  The reference plots the cell centres as a point cloud
(post_processing/animate_fields.py); ``sparsespatialsampling_amd.Probe`` finds the cell that HOLDS every pixel instead -- exactly,
also where the level changes -- and copies the cell's value, so the picture shows the grid as it is: blocky where the cells are
large, NaN inside the cylinder and outside the domain.

    python examples/s3_for_synthetic_slice.py [n_points] [save_path]

The synthetic velocity is a Karman-like street of Gaussian vortices travelling downstream of the cylinder, shed with period 40
snapshots.  It is a function of position, so the script evaluates it at the cell centres of the generated grid (an exported field
would take its place: ``Probe.from_dataloader(loader, points)``).  Printed: how many pixels found a cell, the peak of the
time-mean vorticity magnitude on the plane, and the frequency the probe sees.  With matplotlib installed the plane is saved as
``slice.png``.  Needs an MI355X.
"""
import sys
from os.path import abspath, dirname, join

import torch as pt

sys.path.insert(0, dirname(dirname(abspath(__file__))))
from sparsespatialsampling_amd import Gradient, Grid, Probe, hipops, welch              # noqa: E402
from sparsespatialsampling_amd.geometry import CubeGeometry, CylinderGeometry3D         # noqa: E402
from sparsespatialsampling_amd.metrics import temporal_std                              # noqa: E402
from sparsespatialsampling_amd.sampling import plane                                    # noqa: E402
from sparsespatialsampling_amd.sparse_spatial_sampling import SparseSpatialSampling     # noqa: E402

PERIOD, CORE = 40.0, 0.12         # shedding period in snapshots, core radius of a vortex


def velocity(coord: pt.Tensor, t0: int, t1: int) -> pt.Tensor:
    """[N, 3, t1 - t0] float32: uniform flow plus two rows of counter-rotating Gaussian vortices behind the cylinder at (0.8, 1.0)"""
    x, y, z = coord[:, 0:1].double(), coord[:, 1:2].double(), coord[:, 2:3].double()
    t = pt.arange(t0, t1, dtype=pt.float64)[None, :]
    u, v = pt.ones(len(coord), t1 - t0, dtype=pt.float64), pt.zeros(len(coord), t1 - t0, dtype=pt.float64)
    for row, sign in ((0.07, 1.0), (-0.07, -1.0)):
        for j in range(4):
            xc = 0.9 + ((t / PERIOD + 0.5 * (sign < 0) + j) % 4.0) * 0.35             # a vortex every 0.35, moving 0.35 per period
            dx, dy = x - xc, y - (1.0 + row)
            g = sign * 0.3 * pt.exp(-(dx ** 2 + dy ** 2) / CORE ** 2) * (1 + 0.1 * pt.cos(20 * z))
            u, v = u - g * dy / CORE, v + g * dx / CORE
    return pt.stack([u, v, pt.zeros_like(u)], dim=1).float()


if __name__ == "__main__":
    n_points = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    save_path = sys.argv[2] if len(sys.argv) > 2 else join("run", "slice_synthetic")
    n_snapshots, dt = 200, 1.0
    bounds = [[0.0, 0.0, 0.0], [2.4, 2.0, 0.314]]
    cylinder = [[(0.8, 1.0, -1.0), (0.8, 1.0, 1.0)], 0.05]

    pt.manual_seed(0)
    coord = pt.rand(n_points, 3) * pt.tensor(bounds[1])
    coord = coord[((coord[:, :2] - pt.tensor([0.8, 1.0])) ** 2).sum(1) > cylinder[1] ** 2]
    metric = temporal_std(velocity(coord, 0, n_snapshots)[:, 1])                        # where v fluctuates: the vortex street

    domain = CubeGeometry("domain", True, bounds[0], bounds[1])
    body = CylinderGeometry3D("cylinder", False, cylinder[0], cylinder[1], refine=True)
    s_cube = SparseSpatialSampling(coord, metric, [domain, body], save_path, "slice", "cylinder3D", min_metric=0.75)
    s_cube.execute_grid_generation()
    centers = s_cube.centers
    print(f"generated {len(centers)} cells, levels {int(s_cube.levels.min())} .. {int(s_cube.levels.max())}")

    # the field on the grid, and its vorticity magnitude [N_cells, T] (one fused launch per batch)
    u_grid = hipops.to_device(velocity(centers, 0, n_snapshots))
    vort = Gradient(centers).vorticity_magnitude(u_grid)

    # a z-plane at mid-span, 600 x 500 pixels over the whole domain and a margin: every pixel gets the value of the cell that holds it
    shape = (600, 500)
    pixels = plane([-0.1, -0.1, 0.157], [2.6, 0.0, 0.0], [0.0, 2.2, 0.0], shape)
    grid = Grid.from_s_cube(s_cube)                 # uploaded once, indexed once, for the plane and for the station below
    probe = Probe.from_grid(grid, pixels)
    inside = probe.inside.reshape(shape)
    frames = hipops.snapshot_major(probe.sample(vort), 1, n_snapshots).view(n_snapshots, *shape)      # [T, 600, 500] on the device
    mean_frame = frames.mean(dim=0).cpu()
    print(f"{int(inside.sum())} of {inside.size} pixels lie in a cell ({int((~inside).sum())} outside the domain or inside the cylinder); "
          f"time-mean vorticity magnitude on the plane: up to {float(mean_frame[pt.from_numpy(inside)].max()):.2f}")

    # the time series of v at a probe position in the wake, straight into welch
    station = Probe.from_grid(grid, pt.tensor([[1.5, 1.07, 0.157]], dtype=pt.float64))
    series = station.sample(u_grid[:, 1, :].contiguous())                              # [1, T] float64, on the device
    freq, psd = welch(series, dt, nperseg=160)
    peak = int(psd[0, 1:].argmax()) + 1
    print(f"probe in cell {int(station.cell_ids[0])}: spectral peak at f = {float(freq[peak]):.4f} (shedding: {1 / PERIOD:.4f})")

    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        plt.imshow(mean_frame.numpy().T, origin="lower", extent=(-0.1, 2.5, -0.1, 2.1), cmap="viridis")
        plt.colorbar(label="time-mean vorticity magnitude")
        plt.savefig(join(save_path, "slice.png"), dpi=200)
        print(f"wrote {join(save_path, 'slice.png')}")
    except ImportError:
        pass
