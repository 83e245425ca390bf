"""Cost of the mesh predicate (``s3_mask_mesh``): 10^6 random cells around an icosphere of 20 480 and of 81 920 facets.

    python tools/mesh_mask_probe.py [n_cells] [host_cells] [out.json]

Per surface: device time (HIP events around 20 warm calls each, the median) of ``s3_mask_mesh`` with the table the constructor
builds, with the 1 x 1 table (every node walks all facets) and, as a yardstick, of ``s3_mask_box`` with the body's bounding box on
the same cells; and the wall time of the host path (``tree_backend.host_mask``: ``check_cell`` per cell, what a body without a
device predicate costs) on the first ``host_cells`` cells, scaled to ``n_cells``.  The flags of the two tables are compared, and
those of the host path with the device's.  Needs an MI355X.
"""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsespatialsampling_amd import hipops, tree_backend                                          # noqa: E402
from sparsespatialsampling_amd.geometry import GeometrySTL3D                                        # noqa: E402
from sparsespatialsampling_amd.geometry.geometry_STL_3d import build_column_bins                   # noqa: E402


def write_icosphere(path, subdivisions, center, radius):
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
                if key not in middle:
                    verts.append((verts[i] + verts[j]) / np.linalg.norm(verts[i] + verts[j]))
                    middle[key] = len(verts) - 1
                mids.append(middle[key])
            ab, bc, ca = mids
            finer += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = finer
    record = np.zeros(len(faces), dtype=np.dtype([("normal", "<f4", 3), ("vertices", "<f4", (3, 3)), ("attr", "<u2")]))
    record["vertices"] = (np.array(verts) * radius + np.asarray(center))[np.array(faces)]
    with open(path, "wb") as f:
        f.write(b"icosphere".ljust(80))
        f.write(np.uint32(len(faces)).tobytes())
        f.write(record.tobytes())


def median_ms(call, repeats=20, warm=3):
    for _ in range(warm):
        call()
    pt.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = pt.cuda.Event(enable_timing=True), pt.cuda.Event(enable_timing=True)
        start.record()
        call()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return statistics.median(times), min(times), max(times)


def main():
    n_cells = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    host_cells = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000
    out = sys.argv[3] if len(sys.argv) > 3 else None
    hipops.device()
    center_of_body, radius = np.array([0.31, -0.17, 0.43]), 0.77
    rng = np.random.default_rng(31)
    center = np.ascontiguousarray(center_of_body + (rng.random((n_cells, 3)) - 0.5) * 2.6 * radius)
    level = rng.integers(2, 9, n_cells).astype(np.int32)
    width = 4.0 * radius
    d_center, d_level = hipops.to_device(center), hipops.to_device(level)
    result = {"device": pt.cuda.get_device_name(0), "n_cells": n_cells, "host_cells": host_cells, "surfaces": []}
    with tempfile.TemporaryDirectory() as folder:
        for subdivisions in (5, 6):
            path = os.path.join(folder, f"ico{subdivisions}.stl")
            write_icosphere(path, subdivisions, center_of_body, radius)
            body = GeometrySTL3D("ball", False, path)
            _, tri, lo, hi, ny, nz, bin_start, bin_facet = body.kernel_spec()
            tables = {"binned": hipops.MeshTable(tri, lo, hi, ny, nz, bin_start, bin_facet),
                      "brute": hipops.MeshTable(tri, lo, hi, *build_column_bins(tri, lo, hi, 1, 1))}
            flags = {k: pt.zeros(n_cells, dtype=pt.uint8, device="cuda") for k in ("binned", "brute", "box")}
            cells = {k: hipops.MaskCells(d_center, d_level, width, v) for k, v in flags.items()}
            row = {"facets": int(len(tri)), "table": [int(ny), int(nz)], "facets_per_column": float(len(bin_facet) / (ny * nz))}
            for name, mesh in tables.items():
                repeats = 20 if name == "binned" or len(tri) <= 20480 else 5
                row[name + "_ms"] = median_ms(lambda: hipops.mask_mesh(cells[name], mesh, 0, 0), repeats=repeats, warm=2)
            row["box_ms"] = median_ms(lambda: hipops.mask_box(cells["box"], lo, hi, 0, 0))
            row["tables_agree"] = bool(pt.equal(flags["binned"], flags["brute"]))
            start = time.perf_counter()
            host = tree_backend.host_mask(body, pt.from_numpy(center[:host_cells]), pt.from_numpy(level[:host_cells]), width, False)
            row["host_s_measured"] = time.perf_counter() - start
            row["host_s_scaled"] = row["host_s_measured"] * n_cells / host_cells
            row["host_agrees"] = bool(np.array_equal(host, flags["binned"][:host_cells].cpu().numpy()))
            row["removed_cells"] = int(flags["binned"].sum().item())
            result["surfaces"].append(row)
            print(json.dumps(row), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
