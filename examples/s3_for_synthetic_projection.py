"""
Looking THROUGH a field on the generated grid: the numerical schlieren of the synthetic 3-D cylinder integrated along the span, next
to the plane at mid-span that ``examples/s3_for_synthetic_slice.py`` can show.  A schlieren image is the integral of ``|grad rho|``
along the optical axis; ``Gradient`` gives the integrand per cell and ``Rays`` integrates it exactly -- a cell field is piecewise
constant on disjoint dyadic boxes, so its integral along a line is the sum of value x chord over the cells crossed, through the
cylinder and across every level jump.  The reference has nothing of the kind.

    python examples/s3_for_synthetic_projection.py [n_points] [save_path]

The synthetic "density" is the spanwise-modulated vortex street of the slice example (``1 - |v - v_inf|^2``, a low where a vortex
sits).  Printed: the pixels whose ray crosses the grid, the span every ray has inside cells (less where it passes the cylinder:
there it has none), and how far the spanwise mean of the schlieren (``Rays.mean``) lies from the mid-span plane.  With matplotlib
installed both images are saved as ``projection.png``.  Needs an MI355X.
"""
import sys
from os.path import abspath, dirname, join

import torch as pt

sys.path.insert(0, dirname(dirname(abspath(__file__))))
from s3_for_synthetic_slice import velocity                                             # noqa: E402
from sparsespatialsampling_amd import Gradient, Grid, Probe, Rays, hipops               # noqa: E402
from sparsespatialsampling_amd.geometry import CubeGeometry, CylinderGeometry3D         # noqa: E402
from sparsespatialsampling_amd.metrics import temporal_std                              # noqa: E402
from sparsespatialsampling_amd.projection import parallel                               # noqa: E402
from sparsespatialsampling_amd.sampling import plane                                    # noqa: E402
from sparsespatialsampling_amd.sparse_spatial_sampling import SparseSpatialSampling     # noqa: E402


def density(coord: pt.Tensor, t0: int, t1: int) -> pt.Tensor:
    """[N, t1 - t0] float32: low where a vortex of the street sits"""
    v = velocity(coord, t0, t1).double()
    return (1.0 - (v[:, 0] - 1.0) ** 2 - v[:, 1] ** 2).float()


if __name__ == "__main__":
    n_points = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    save_path = sys.argv[2] if len(sys.argv) > 2 else join("run", "projection_synthetic")
    n_snapshots = 40
    bounds = [[0.0, 0.0, 0.0], [2.4, 2.0, 0.314]]
    cylinder = [[(0.8, 1.0, -1.0), (0.8, 1.0, 1.0)], 0.05]

    pt.manual_seed(0)
    coord = pt.rand(n_points, 3) * pt.tensor(bounds[1])
    coord = coord[((coord[:, :2] - pt.tensor([0.8, 1.0])) ** 2).sum(1) > cylinder[1] ** 2]
    metric = temporal_std(velocity(coord, 0, 200)[:, 1])

    domain = CubeGeometry("domain", True, bounds[0], bounds[1])
    body = CylinderGeometry3D("cylinder", False, cylinder[0], cylinder[1], refine=True)
    s_cube = SparseSpatialSampling(coord, metric, [domain, body], save_path, "projection", "cylinder3D", min_metric=0.75)
    s_cube.execute_grid_generation()
    centers = s_cube.centers
    print(f"generated {len(centers)} cells, levels {int(s_cube.levels.min())} .. {int(s_cube.levels.max())}")

    # the numerical schlieren per cell: |grad rho| [N_cells, T], one fused launch per batch
    rho = hipops.to_device(density(centers, 0, n_snapshots))
    schlieren = Gradient(centers).magnitude(rho)

    # rays along the span through the pixel centres of a 600 x 500 image over the x-y extent of the domain
    shape = (600, 500)
    grid = Grid.from_s_cube(s_cube)                 # uploaded once, indexed once, for the rays and for the plane
    lo, hi = grid.bounds
    window_lo, window_hi = [0.0, 0.0, float(lo[2])], [2.4, 2.0, float(hi[2])]
    origins, directions, order = parallel(grid, (0.0, 0.0, 1.0), shape, lo=window_lo, hi=window_hi)
    rays = Rays.from_grid(grid, origins, directions, order=order)
    image = rays.mean(schlieren)                    # [n_pixels, T] on the device: the integral over the span / the span inside cells
    crossed = rays.status == hipops.RAY_STATUS["CROSSED"]
    span = rays.length[crossed]
    print(f"{int(crossed.sum())} of {len(origins)} rays cross the grid, {int(rays.segments.max())} cells at the most; "
          f"span inside cells {float(span.min()):.3f} .. {float(span.max()):.3f}")

    # the mid-span plane of the same field at the same pixels
    pixels = plane([0.0, 0.0, 0.157], [2.4, 0.0, 0.0], [0.0, 2.0, 0.0], shape)
    mid = Probe.from_grid(grid, pixels).sample(schlieren)
    both = pt.isfinite(mid[:, 0]) & pt.isfinite(image[:, 0])
    diff = (mid[both] - image[both]).abs().max() / mid[both].abs().max()
    print(f"spanwise mean against the mid-span plane: up to {float(diff):.2f} of the plane's maximum apart (the street is modulated along the span)")

    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        fig, axes = plt.subplots(1, 2, figsize=(12, 5))
        for ax, values, title in ((axes[0], image, "schlieren, mean over the span"), (axes[1], mid, "schlieren, plane at mid-span")):
            ax.imshow(values[:, 0].reshape(shape).cpu().numpy().T, origin="lower", extent=(0.0, 2.4, 0.0, 2.0), cmap="gray_r")
            ax.set_title(title)
        fig.savefig(join(save_path, "projection.png"), dpi=200)
        print(f"wrote {join(save_path, 'projection.png')}")
    except ImportError:
        pass
