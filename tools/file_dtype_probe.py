"""dev helper: what single-precision files buy at the cylinder3D shape.

    python tools/file_dtype_probe.py [T] [n_batches] [rounds] [directory]

1. ``ExportData.export()`` with the HDF5 file at its end, float64 against float32 storage: `rounds` runs of each, interleaved
   (f64, fp32, f64, ...: other work shares the host and the disk), `n_batches` host batches of `T` snapshots per run; per run the
   median of the steady calls (the first builds the KNN cache and writes the grid, the last closes the file) and the bytes written.
2. ``Dataloader.load_snapshot`` of the files of the last round, host path against ``device=True`` (each followed by what SVD / DMD
   need anyway: the matrix on the device), interleaved as well.

Times are host clocks around work that ends in a device synchronise / a closed file.  Needs an MI355X; prints ms and bytes."""
import logging
import os
import shutil
import sys
import tempfile
import time
import types

import numpy as np
import torch as pt

sys.path.insert(0, ".")
import bench                                                                                # noqa: E402
from sparsespatialsampling_amd import geometry                                              # noqa: E402
from sparsespatialsampling_amd.data import Dataloader                                       # noqa: E402
from sparsespatialsampling_amd.export import ExportData                                     # noqa: E402
from sparsespatialsampling_amd.s_cube import SamplingTree                                   # noqa: E402

logging.getLogger().setLevel(logging.ERROR)
t = int(sys.argv[1]) if len(sys.argv) > 1 else 25
n_batches = int(sys.argv[2]) if len(sys.argv) > 2 else 12
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
if len(sys.argv) > 4:
    tempfile.tempdir = sys.argv[4]

cfg = dict(bench.WORKLOADS["cylinder3D_Re3900"])
x, metric, geos, kw = bench.build_case("cylinder3D_Re3900", cfg, geometry)
tree = SamplingTree(pt.from_numpy(x), pt.from_numpy(metric), geos, **kw)
tree.refine()
centers, vertices, faces, levels, width = tree.all_centers, tree.all_nodes, tree.face_ids, tree.all_levels, float(tree.width)
tree.close()
coords = pt.from_numpy(x)
batches = [pt.empty((len(x), 1, t), dtype=pt.float32).normal_() for _ in range(2)]
times = [str(i) for i in range(t * n_batches)]
print(f"{len(x)} points -> {len(centers)} cells, {n_batches} batches of {t} snapshots, {rounds} interleaved rounds", flush=True)


def export_once(file_dtype, keep=None):
    d = tempfile.mkdtemp(prefix="s3_dtype_")
    try:
        s = types.SimpleNamespace(n_dimensions=3, faces=faces, centers=centers, vertices=vertices, levels=levels, metric=pt.from_numpy(metric),
                                  size_initial_cell=width, save_path=d, save_name="probe", grid_name="g")
        ex = ExportData(s, write_times=times, n_neighbors=26, file_dtype=file_dtype)
        per = []
        for b in range(n_batches):
            tb = time.perf_counter()
            ex.export(coords, batches[b % 2], "p", n_snapshots_total=t * n_batches)
            per.append((time.perf_counter() - tb) * 1e3)
        size = os.path.getsize(os.path.join(d, "probe.h5"))
        if keep is not None:
            shutil.move(os.path.join(d, "probe.h5"), keep)
        return float(np.median(per[2:-1])), per[-1], size
    finally:
        shutil.rmtree(d, ignore_errors=True)


keep_dir = tempfile.mkdtemp(prefix="s3_dtype_files_")
try:
    export_once(pt.float64), export_once(pt.float32)                                         # warm-up of both: code objects, pinned stages
    result = {pt.float64: [], pt.float32: []}
    for r in range(rounds):
        for file_dtype in (pt.float64, pt.float32):
            keep = os.path.join(keep_dir, f"{'f32' if file_dtype == pt.float32 else 'f64'}.h5") if r == rounds - 1 else None
            steady, last, size = export_once(file_dtype, keep)
            result[file_dtype].append(steady)
            print(f"round {r} {str(file_dtype):>14}: steady {steady:6.2f} ms per export() call, closing call {last:7.1f} ms, file {size} bytes", flush=True)
    for file_dtype, v in result.items():
        print(f"{str(file_dtype):>14}: median {np.median(v):.2f} ms, range {min(v):.2f}-{max(v):.2f} ms per {t}-snapshot batch")

    def timed(fn):
        pt.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        pt.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for name in ("f64.h5", "f32.h5"):
        loader = Dataloader(keep_dir, name)                                                  # float32 matrices, like the reference's default
        timed(lambda: loader.load_snapshot("p", device=True))
        host_ms, dev_ms = [], []
        for r in range(rounds):
            host_ms.append(timed(lambda: loader.load_snapshot("p").cuda())[0])
            dev_ms.append(timed(lambda: loader.load_snapshot("p", device=True))[0])
        same = bool((loader.load_snapshot("p").cuda() == loader.load_snapshot("p", device=True)).all())
        print(f"load_snapshot of {name} ({os.path.getsize(os.path.join(keep_dir, name))} bytes, {len(times)} write times) onto the device: "
              f"host path + upload {np.median(host_ms):.1f} ms ({min(host_ms):.1f}-{max(host_ms):.1f}), device=True {np.median(dev_ms):.1f} ms "
              f"({min(dev_ms):.1f}-{max(dev_ms):.1f}); equal {same}", flush=True)
finally:
    shutil.rmtree(keep_dir, ignore_errors=True)
