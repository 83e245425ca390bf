"""
S^3 around a body given as an STL file (reference geometry/geometry_STL_3d.py; its README, "Significant increase in runtime
when using STL files as geometry objects"): a tessellated ellipsoid in a 3-D box, the grid refined at its surface, one scalar
field exported.

    python examples/s3_for_synthetic_STL_body.py [save_path] [n_points] [subdivisions] [min_refinement_level]

The STL file is written by the helper below (20 * 4^subdivisions facets).  The point-in-mesh test of every new cell runs in
the ``s3_mask_mesh`` kernel against the full surface; ``reduce_by`` is not needed.  Needs an MI355X.
"""
import sys
from os import makedirs
from os.path import abspath, dirname, join
from time import time

import numpy as np
import torch as pt

sys.path.insert(0, dirname(dirname(abspath(__file__))))
from sparsespatialsampling_amd.export import ExportData                                 # noqa: E402
from sparsespatialsampling_amd.geometry import CubeGeometry, GeometrySTL3D              # noqa: E402
from sparsespatialsampling_amd.sparse_spatial_sampling import SparseSpatialSampling     # noqa: E402

CENTER, SEMI_AXES = np.array([0.8, 0.5, 0.5]), np.array([0.3, 0.12, 0.2])


def write_ellipsoid_stl(path: str, subdivisions: int) -> int:
    """subdivided icosahedron, its vertices pushed onto the ellipsoid; binary STL.  Returns the number of facets."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [np.array(v, dtype=np.float64) / np.linalg.norm(v) for v in
             [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1),
              (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
             (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
             (9, 8, 1)]
    for _ in range(subdivisions):
        middle, finer = {}, []
        for a, b, c in faces:
            mids = []
            for i, j in ((a, b), (b, c), (c, a)):
                key = (min(i, j), max(i, j))
                if key not in middle:                      # one vertex per edge, shared by both facets: the surface stays closed
                    verts.append((verts[i] + verts[j]) / np.linalg.norm(verts[i] + verts[j]))
                    middle[key] = len(verts) - 1
                mids.append(middle[key])
            ab, bc, ca = mids
            finer += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = finer
    points = np.array(verts) * SEMI_AXES + CENTER
    record = np.zeros(len(faces), dtype=np.dtype([("normal", "<f4", 3), ("vertices", "<f4", (3, 3)), ("attr", "<u2")]))
    record["vertices"] = points[np.array(faces)]
    with open(path, "wb") as f:
        f.write(b"ellipsoid".ljust(80))
        f.write(np.uint32(len(faces)).tobytes())
        f.write(record.tobytes())
    return len(faces)


if __name__ == "__main__":
    save_path = sys.argv[1] if len(sys.argv) > 1 else join("run", "STL_body_synthetic")
    n_points = int(sys.argv[2]) if len(sys.argv) > 2 else 400_000
    subdivisions = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    min_level = int(sys.argv[4]) if len(sys.argv) > 4 else 7
    makedirs(save_path, exist_ok=True)
    stl_file = join(save_path, "ellipsoid.stl")
    n_facets = write_ellipsoid_stl(stl_file, subdivisions)

    bounds = [[0.0, 0.0, 0.0], [2.4, 1.0, 1.0]]
    domain = CubeGeometry("domain", True, bounds[0], bounds[1])
    body = GeometrySTL3D("ellipsoid", False, stl_file, refine=True, min_refinement_level=min_level)

    # points of the original simulation (none inside the body) and a wake behind it as the field
    pt.manual_seed(0)
    coord = pt.rand(n_points, 3, dtype=pt.float64) * pt.tensor(bounds[1], dtype=pt.float64)
    coord = coord[~pt.from_numpy(body.inside(coord.numpy()))]
    x, r = coord[:, 0] - CENTER[0], ((coord[:, 1] - CENTER[1]) ** 2 + (coord[:, 2] - CENTER[2]) ** 2).sqrt()
    t = pt.arange(20, dtype=pt.float64)[None, :]
    p = (pt.exp(-(r / 0.2) ** 2) * pt.exp(-0.8 * x.clamp(min=0)) * (x > 0))[:, None] * pt.sin(2 * pt.pi * (x[:, None] / 0.5 - t / 20))
    metric = p.std(dim=1)

    s_cube = SparseSpatialSampling(coord, metric, [domain, body], save_path, "metric_0.75", "STL_body", min_metric=0.75)
    t_start = time()
    s_cube.execute_grid_generation()
    print(f"body with {n_facets} facets: generated {s_cube.centers.shape[0]} cells from {coord.shape[0]} original cells in "
          f"{time() - t_start:.2f} s")

    export = ExportData(s_cube, write_times=[str(i) for i in range(p.shape[1])])
    export.export(coord, p.float().unsqueeze(1), "p")
    print(f"wrote {join(save_path, 'metric_0.75')}.h5 / .xdmf")
