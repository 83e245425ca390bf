"""
Following the flow on the generated grid: streamlines and pathlines behind the synthetic 2-D cylinder, coloured by the vorticity
magnitude.  The reference writes files for a viewer, which integrates particles on the host one snapshot at a time;
``sparsespatialsampling_amd.Tracer`` traces a whole set of particles in one launch on the GPU, through the velocity on the grid NODES.

    python examples/s3_for_synthetic_streamlines.py [n_points] [save_path]

The synthetic velocity (``s3_for_synthetic_slice.velocity``, a Karman-like street of Gaussian vortices) is sampled on a random point
cloud, the grid is generated from its fluctuation and the velocity is exported with ``interpolate_at_vertices=True``: the file then
carries ``data/<t>/u_vertices``, the velocity at the corner nodes of the cells, which is what the tracer reads.  Streamlines start
on a line of seeds upstream of the cylinder and run in both directions; pathlines are released in the wake and carried through
the snapshots.  ``Gradient`` on the node cloud gives the vorticity magnitude and ``Paths.sample`` its value along every path.
Printed: how the paths end, their lengths and the range of the colour.  With matplotlib installed the streamlines of the first
snapshot are saved as ``streamlines.png``.  Needs an MI355X.
"""
import sys
from os.path import abspath, dirname, join

import numpy as np
import torch as pt

sys.path.insert(0, dirname(dirname(abspath(__file__))))
sys.path.insert(0, dirname(abspath(__file__)))
from s3_for_synthetic_slice import velocity                                              # noqa: E402
from sparsespatialsampling_amd import Gradient, Grid, Tracer, hipops                    # noqa: E402
from sparsespatialsampling_amd.const import DATA                                        # noqa: E402
from sparsespatialsampling_amd.data import Dataloader                                   # noqa: E402
from sparsespatialsampling_amd.export import ExportData                                 # noqa: E402
from sparsespatialsampling_amd.geometry import CubeGeometry, SphereGeometry             # noqa: E402
from sparsespatialsampling_amd.h5io import open_h5                                      # noqa: E402
from sparsespatialsampling_amd.metrics import temporal_std                              # noqa: E402
from sparsespatialsampling_amd.sampling import line                                     # noqa: E402
from sparsespatialsampling_amd.sparse_spatial_sampling import SparseSpatialSampling     # noqa: E402
from sparsespatialsampling_amd.tracing import STATUS                                    # noqa: E402


def velocity_2d(coord: pt.Tensor, t0: int, t1: int) -> pt.Tensor:
    """[N, 2, t1 - t0] float32: the plane z = 0 of the synthetic street"""
    return velocity(pt.cat([coord, pt.zeros(len(coord), 1, dtype=coord.dtype)], dim=1), t0, t1)[:, :2].contiguous()


def endings(status) -> str:
    status = np.asarray(status).ravel()
    return ", ".join(f"{int((status == code).sum())} {name}" for name, code in STATUS.items())


if __name__ == "__main__":
    n_points = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000
    save_path = sys.argv[2] if len(sys.argv) > 2 else join("run", "streamlines_synthetic")
    n_snapshots, dt_snapshot = 40, 0.01                     # a vortex moves 0.35 in 40 snapshots at speed one: 0.00875 per snapshot
    bounds = [[0.0, 0.0], [2.4, 2.0]]
    centre, radius = [0.8, 1.0], 0.05
    pt.manual_seed(0)
    coord = pt.rand(n_points, 2) * pt.tensor(bounds[1])
    coord = coord[((coord - pt.tensor(centre)) ** 2).sum(1) > radius ** 2]
    u_cloud = velocity_2d(coord, 0, n_snapshots)

    geometries = [CubeGeometry("domain", True, bounds[0], bounds[1]), SphereGeometry("cylinder", False, centre, radius, refine=True)]
    s_cube = SparseSpatialSampling(coord, temporal_std(u_cloud[:, 1]), geometries, save_path, "streamlines", "cylinder2D", min_metric=0.75)
    s_cube.execute_grid_generation()
    print(f"generated {len(s_cube.centers)} cells, {len(s_cube.vertices)} nodes, levels {int(s_cube.levels.min())} .. {int(s_cube.levels.max())}")

    # the export puts the velocity onto the cell centres AND the nodes; the tracer reads the nodes
    times = [str(t) for t in range(n_snapshots)]
    ExportData(s_cube, write_times=times, interpolate_at_vertices=True, file_dtype=pt.float32).export(coord, u_cloud, "u")
    loader = Dataloader(save_path, "streamlines.h5")
    with open_h5(join(save_path, "streamlines.h5"), "r") as f:
        u_nodes = hipops.to_device(np.stack([f.read(f"{DATA}/{t}/u_vertices") for t in times], axis=-1))      # [N_nodes, 2, T] fp32
    grid = Grid.from_dataloader(loader)             # uploaded once, indexed once: the tracer and every colouring below rest on it
    tracer = Tracer.from_grid(grid)

    # streamlines of every snapshot from a line of seeds upstream, both ways, about half a cell per step
    seeds = line([0.3, 0.6], [0.3, 1.4], 41)
    lines = tracer.streamlines(u_nodes, seeds, n_steps=600, step="cell", cfl=0.5, direction="both", every=2)
    print(f"streamlines: {lines.points.shape[0]} seeds x {lines.points.shape[1]} snapshots, up to {lines.points.shape[2]} points each; "
          f"rows per path {int(lines.length.min())} .. {int(lines.length.max())}")
    print(f"    upstream ends: {endings(lines.status[..., 0])}; downstream ends: {endings(lines.status[..., 1])}")

    # pathlines released in the wake at the first snapshot; points[:, -1] is the flow map
    wake = np.stack(np.meshgrid(np.linspace(0.9, 1.3, 21), np.linspace(0.85, 1.15, 13), indexing="ij"), axis=-1).reshape(-1, 2)
    paths = tracer.pathlines(u_nodes, wake, dt_snapshot, substeps=4)
    moved = np.linalg.norm(paths.points[:, -1] - paths.points[:, 0], axis=1)
    print(f"pathlines: {len(wake)} particles through {n_snapshots} snapshots: {endings(paths.status)}; "
          f"displacement of those that arrive {np.nanmin(moved):.3f} .. {np.nanmax(moved):.3f}")

    # colour: the vorticity magnitude on the nodes (least squares on the node cloud), blended along the paths
    vort = Gradient(loader.nodes.double()).vorticity_magnitude(u_nodes)                  # [N_nodes, T] on the device
    along_lines = lines.sample(vort[:, :1].contiguous(), mode="linear")[..., 0]          # snapshot 0 on every streamline
    along_paths = paths.sample(vort, mode="linear")                                      # [particles, T (positions), T (field)]
    step = pt.arange(n_snapshots, device=along_paths.device)
    own_time = along_paths[:, step, step].cpu().numpy()                                  # the field at the time of each position
    print(f"vorticity magnitude along the streamlines of snapshot 0: up to {float(np.nanmax(along_lines[:, 0].cpu().numpy())):.2f}; "
          f"along the pathlines: up to {float(np.nanmax(own_time)):.2f}")

    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        colour = along_lines[:, 0].cpu().numpy()
        for j in range(len(seeds)):
            plt.scatter(lines.points[j, 0, :, 0], lines.points[j, 0, :, 1], c=colour[j], s=0.3, cmap="viridis", vmin=0.0, vmax=float(np.nanmax(colour)))
        plt.plot(paths.points[:, :, 0].T, paths.points[:, :, 1].T, color="k", linewidth=0.3)
        plt.gca().set_aspect("equal")
        plt.savefig(join(save_path, "streamlines.png"), dpi=200)
        print(f"wrote {join(save_path, 'streamlines.png')}")
    except ImportError:
        pass
