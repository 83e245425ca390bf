"""
Counting what a field shows: the vortices (connected regions of Q > q0) and the reversed flow (u_x < 0) in the wake of the synthetic
3-D cylinder, for every snapshot in one pass on the GPU.  The reference stops at the written grid; on the host the route would be
``scipy.sparse.csgraph``, one snapshot at a time.  ``sparsespatialsampling_amd.Regions`` labels the face-connected cells of a whole
snapshot batch and tabulates every region: cells, volume, centroid, bounding box, and the integral and extrema of a second field.

    python examples/s3_for_synthetic_regions.py [n_points] [save_path]

The synthetic velocity (``s3_for_synthetic_slice.velocity``) is a function of position, so the script evaluates it at the cell CENTRES
of the generated grid (the fields of an export would take its place: ``Regions.from_dataloader(loader)``); ``Gradient(centers)`` gives
Q and the vorticity magnitude there.  Printed: the number of vortices per snapshot, the three largest of a few snapshots with their
cells, volume, centroid and peak vorticity, and the volume of reversed and of slow flow over time.  Needs an MI355X.
"""
import sys
from os.path import abspath, dirname, join

import torch as pt

sys.path.insert(0, dirname(dirname(abspath(__file__))))
sys.path.insert(0, dirname(abspath(__file__)))
from s3_for_synthetic_isosurface import grid                                             # noqa: E402
from s3_for_synthetic_slice import velocity                                              # noqa: E402
from sparsespatialsampling_amd import Gradient, Grid, Regions, hipops                   # noqa: E402
from sparsespatialsampling_amd.geometry import CubeGeometry, CylinderGeometry3D         # noqa: E402


if __name__ == "__main__":
    n_points = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    save_path = sys.argv[2] if len(sys.argv) > 2 else join("run", "regions_synthetic")
    n_snapshots = 40
    pt.manual_seed(0)

    bounds = [[0.0, 0.0, 0.0], [2.4, 2.0, 0.314]]
    cylinder = [[(0.8, 1.0, -1.0), (0.8, 1.0, 1.0)], 0.05]
    coord = pt.rand(n_points, 3) * pt.tensor(bounds[1])
    coord = coord[((coord[:, :2] - pt.tensor([0.8, 1.0])) ** 2).sum(1) > cylinder[1] ** 2]
    s_cube = grid(coord, n_snapshots, [CubeGeometry("domain", True, bounds[0], bounds[1]),
                                       CylinderGeometry3D("cylinder", False, cylinder[0], cylinder[1], refine=True)], save_path, "cylinder3D")
    centers = s_cube.centers
    u = hipops.to_device(velocity(centers, 0, n_snapshots))                              # [N_cells, 3, T] fp32
    gradient = Gradient(centers)
    q, vorticity = gradient.q_criterion(u), gradient.vorticity_magnitude(u)              # [N_cells, T] f64 on the device

    regions = Regions.from_grid(Grid.from_s_cube(s_cube))                                # the neighbour table is built once
    q0 = 0.25 * float(q.max())
    vortices = regions.extract(q, lo=q0, weight=vorticity)                               # every snapshot in one batch
    per_snapshot = vortices.n_regions
    print(f"Q > {q0:.3g}: {len(vortices)} regions in {n_snapshots} snapshots ({int(per_snapshot.min())} .. {int(per_snapshot.max())} each)")
    top = vortices.largest(3)
    for t in range(0, n_snapshots, 10):
        for r, rows in enumerate(zip(*(top.of_snapshot(t)[k].tolist() for k in ("n_cells", "volume", "centroid", "g_max")))):
            cells, volume, centroid, peak = rows
            print(f"  snapshot {t:2d} vortex {r}: {cells:5d} cells, volume {volume:.3e}, centroid ({', '.join(f'{x:.3f}' for x in centroid)}), "
                  f"peak vorticity {peak:.2f}")

    # reversed flow, u_x < 0 (this synthetic wake has none: its vortices slow the flow by 13 % at most), and slow flow, u_x < 0.9
    u_x = u[:, 0, :].contiguous()
    for name, bound in (("reversed flow (u_x < 0)", 0.0), ("slow flow (u_x < 0.9)", 0.9)):
        below = regions.extract(u_x, hi=float(pt.nextafter(pt.tensor(bound, dtype=pt.float32), pt.tensor(-1.0))))    # the interval is closed
        offsets = pt.from_numpy(below.offsets)
        volume = pt.zeros(n_snapshots, dtype=pt.float64).index_add_(
            0, pt.repeat_interleave(pt.arange(n_snapshots), offsets[1:] - offsets[:-1]), below.volume.cpu())
        print(f"{name}: " + ", ".join(f"t={t}: {int(below.n_regions[t])} regions, volume {float(volume[t]):.3e}" for t in range(0, n_snapshots, 10)))
