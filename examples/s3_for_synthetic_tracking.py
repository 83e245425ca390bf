"""
Following what a field shows through time: the vortices (connected regions of Q > q0) in the wake of the synthetic 3-D cylinder are
labelled for every snapshot in one pass on the GPU (``s3_for_synthetic_regions.py``), then linked from snapshot to snapshot by the
cells they share -- the overlap table of ``labels[:, :T-1]`` and ``labels[:, 1:]``, built on the GPU too -- and chained into tracks:
when a vortex appears, how fast it convects, what it merges with, when it leaves.  The reference stops at the written grid.

    python examples/s3_for_synthetic_tracking.py [n_points] [save_path]

The synthetic wake sheds a vortex every 0.35 downstream and moves it 0.35 per period of 40 snapshots, so a track should convect at
0.35 / 40 = 0.00875 per snapshot along x until its vortex wraps round at the end of the street.  Printed: the tracks and events of the
batch, the lifetimes of the tracks, and the convection speed of the longest ones against that figure.  Needs an MI355X.
"""
import sys
from os.path import abspath, dirname, join

import numpy as np
import torch as pt

sys.path.insert(0, dirname(dirname(abspath(__file__))))
sys.path.insert(0, dirname(abspath(__file__)))
from s3_for_synthetic_isosurface import grid                                             # noqa: E402
from s3_for_synthetic_slice import PERIOD, velocity                                      # noqa: E402
from sparsespatialsampling_amd import Gradient, Grid, Regions, hipops                   # noqa: E402
from sparsespatialsampling_amd.geometry import CubeGeometry, CylinderGeometry3D         # noqa: E402


if __name__ == "__main__":
    n_points = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    save_path = sys.argv[2] if len(sys.argv) > 2 else join("run", "tracking_synthetic")
    n_snapshots, dt = 40, 1.0
    pt.manual_seed(0)

    bounds = [[0.0, 0.0, 0.0], [2.4, 2.0, 0.314]]
    cylinder = [[(0.8, 1.0, -1.0), (0.8, 1.0, 1.0)], 0.05]
    coord = pt.rand(n_points, 3) * pt.tensor(bounds[1])
    coord = coord[((coord[:, :2] - pt.tensor([0.8, 1.0])) ** 2).sum(1) > cylinder[1] ** 2]
    s_cube = grid(coord, n_snapshots, [CubeGeometry("domain", True, bounds[0], bounds[1]),
                                       CylinderGeometry3D("cylinder", False, cylinder[0], cylinder[1], refine=True)], save_path, "cylinder3D")
    centers = s_cube.centers
    u = hipops.to_device(velocity(centers, 0, n_snapshots))                              # [N_cells, 3, T] fp32
    q = Gradient(centers).q_criterion(u)                                                 # [N_cells, T] f64 on the device

    regions = Regions.from_grid(Grid.from_s_cube(s_cube))
    q0 = 0.25 * float(q.max())
    labels = regions.label(q, lo=q0)                                                     # int32 [N_cells, T], stays on the device
    table = regions.table(labels)
    smallest = float(table.volume.min())
    tracks = regions.track(labels, table=table, min_volume=0.5 * smallest)               # links that share less than half the smallest vortex do not count
    print(f"Q > {q0:.3g}: {len(table)} regions in {n_snapshots} snapshots, {len(tracks.edges)} overlap edges, {len(tracks)} tracks")
    print("events: " + ", ".join(f"{int(getattr(tracks, k).sum())} {k}" for k in ("born", "died", "merged", "split")))

    length, first = tracks.length.cpu().numpy(), tracks.first.cpu().numpy()
    print(f"lifetimes in snapshots: median {int(np.median(length))}, longest {int(length.max())}; "
          f"{int((length == n_snapshots).sum())} tracks last the whole batch, {int((length == 1).sum())} a single snapshot")
    speed = tracks.velocity(dt).cpu().numpy()                                            # [R, 3]; NaN at the first row of a track
    centroid = table.centroid.cpu().numpy()
    for k in np.argsort(-length, kind="stable")[:5]:
        rows = tracks.rows(k)
        if len(rows) < 2:
            break
        v = speed[rows[1:]]
        print(f"  track {int(k):3d}: snapshots {int(first[k]):2d} .. {int(first[k] + length[k] - 1):2d}, x {centroid[rows[0], 0]:.3f} -> {centroid[rows[-1], 0]:.3f}, "
              f"convection speed ({', '.join(f'{x:.5f}' for x in np.median(v, axis=0))}) per snapshot (the street moves at {0.35 / PERIOD:.5f})")
