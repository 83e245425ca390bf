"""
Looking at a 3-D field in 3-D: the isosurface of Q in the wake of the synthetic 3-D cylinder, coloured by the velocity magnitude and
written as STL -- and its 2-D sibling, contour lines of the vorticity behind the synthetic 2-D cylinder.  The reference writes files
for a viewer, one snapshot at a time; ``sparsespatialsampling_amd.Isosurface`` extracts the triangles of a whole snapshot batch on
the GPU, from fields on the grid NODES.

    python examples/s3_for_synthetic_isosurface.py [n_points] [save_path]

The synthetic velocity (``s3_for_synthetic_slice.velocity``) is a function of position, so the script evaluates it at the NODES of
the generated grid (the fields of an ``interpolate_at_vertices=True`` export would take its place:
``Isosurface.from_dataloader(loader)``); ``Gradient(nodes)`` gives Q and the vorticity there.  Printed: the triangles per snapshot,
the welded size of one of them, and the range of the colour.  Needs an MI355X.
"""
import sys
from os.path import abspath, dirname, join

import torch as pt

sys.path.insert(0, dirname(dirname(abspath(__file__))))
sys.path.insert(0, dirname(abspath(__file__)))
from s3_for_synthetic_slice import velocity                                              # noqa: E402
from sparsespatialsampling_amd import Gradient, Isosurface, hipops                      # noqa: E402
from sparsespatialsampling_amd.geometry import CubeGeometry, CylinderGeometry3D, SphereGeometry     # noqa: E402
from sparsespatialsampling_amd.metrics import temporal_std                              # noqa: E402
from sparsespatialsampling_amd.sparse_spatial_sampling import SparseSpatialSampling     # noqa: E402


def grid(coord, n_snapshots, geometries, save_path, name):
    metric = temporal_std(velocity(coord if coord.shape[1] == 3 else pt.cat([coord, pt.zeros(len(coord), 1)], dim=1), 0, n_snapshots)[:, 1])
    s_cube = SparseSpatialSampling(coord, metric, geometries, save_path, name, name, min_metric=0.75)
    s_cube.execute_grid_generation()
    print(f"{name}: {len(s_cube.centers)} cells, {len(s_cube.vertices)} nodes, levels {int(s_cube.levels.min())} .. {int(s_cube.levels.max())}")
    return s_cube


if __name__ == "__main__":
    n_points = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    save_path = sys.argv[2] if len(sys.argv) > 2 else join("run", "isosurface_synthetic")
    n_snapshots = 40
    pt.manual_seed(0)

    # ---- 3-D: Q on the nodes, its isosurface coloured by |u| -----------------------------------------------------------------
    bounds = [[0.0, 0.0, 0.0], [2.4, 2.0, 0.314]]
    cylinder = [[(0.8, 1.0, -1.0), (0.8, 1.0, 1.0)], 0.05]
    coord = pt.rand(n_points, 3) * pt.tensor(bounds[1])
    coord = coord[((coord[:, :2] - pt.tensor([0.8, 1.0])) ** 2).sum(1) > cylinder[1] ** 2]
    s_cube = grid(coord, n_snapshots, [CubeGeometry("domain", True, bounds[0], bounds[1]),
                                       CylinderGeometry3D("cylinder", False, cylinder[0], cylinder[1], refine=True)], save_path, "cylinder3D")
    nodes = s_cube.vertices
    u_nodes = hipops.to_device(velocity(nodes, 0, n_snapshots))                          # [N_nodes, 3, T] fp32
    q = Gradient(nodes).q_criterion(u_nodes)                                             # [N_nodes, T] f64 on the device
    speed = u_nodes.double().norm(dim=1)

    iso = Isosurface.from_s_cube(s_cube)
    level = 0.25 * float(q.max())
    surface = iso.extract(q, level)                                                      # every snapshot in one batch
    per_snapshot = surface.offsets[1:] - surface.offsets[:-1]
    print(f"Q = {level:.3g}: {len(surface)} triangles in {n_snapshots} snapshots ({int(per_snapshot.min())} .. {int(per_snapshot.max())} each)")
    colour = surface.interpolate(speed)                                                  # |u| at every vertex, [n, 3]
    points, index = surface.weld(0)
    print(f"snapshot 0: {len(index)} triangles over {len(points)} distinct vertices, |u| on the surface {float(colour.min()):.3f} .. {float(colour.max()):.3f}")
    surface.write_stl(join(save_path, "q_isosurface.stl"), 0)
    print(f"wrote {join(save_path, 'q_isosurface.stl')}")

    # ---- 2-D: contour lines of the vorticity ---------------------------------------------------------------------------------
    coord2 = pt.rand(n_points // 4, 2) * pt.tensor(bounds[1][:2])
    coord2 = coord2[((coord2 - pt.tensor([0.8, 1.0])) ** 2).sum(1) > cylinder[1] ** 2]
    s_cube2 = grid(coord2, n_snapshots, [CubeGeometry("domain", True, bounds[0][:2], bounds[1][:2]),
                                         SphereGeometry("cylinder", False, [0.8, 1.0], cylinder[1], refine=True)], save_path, "cylinder2D")
    nodes2 = s_cube2.vertices
    u2 = hipops.to_device(velocity(pt.cat([nodes2, pt.zeros(len(nodes2), 1, dtype=nodes2.dtype)], dim=1), 0, n_snapshots)[:, :2].contiguous())
    vorticity = Gradient(nodes2).vorticity(u2)                                           # [N_nodes, T]
    contour = Isosurface.from_s_cube(s_cube2)
    for sign in (1.0, -1.0):
        lines = contour.extract(vorticity, sign * 0.5 * float(vorticity.abs().max()))
        segments = lines.snapshot(0)[0]                                                  # [n, 2, 2]: the inside lies to the left
        print(f"vorticity = {sign * 0.5:+.1f} max: {len(lines)} segments in {n_snapshots} snapshots, {len(segments)} in snapshot 0")
