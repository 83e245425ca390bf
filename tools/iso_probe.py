"""dev probe (not part of the suite): the isosurface of a smooth node field on a 3-D grid of the cylinder3D size (461 130 cells: a
random octree in a box, levels 4 .. 9, no body), fp32 field [N_nodes, T_b], T_b = 25 | 100, a level that cuts a few percent of the
cells -- HIP-event medians, 7 interleaved rounds, of
    count     hipops.iso_count                  (gathers eight node rows per cell, writes [T_b, N_cells] int32)
    scan      s3_exclusive_scan in place over T_b * N_cells + 1 entries
    emit      hipops.iso_emit                   (gathers the same rows again; 124 bytes per triangle)
against
    (a) hipops.cell_sample(mode="linear") with one query per cell at its centre, in cell order: the kernel with the same 2^d-row
        gather that writes 8 T_b bytes per cell where the count writes 4 T_b
    (b) the floor: every node row once per pass, faces, the count array (written, read and written by the scan, read by the emit)
        and 124 bytes per triangle, at this box's streaming-read rate (s3_yard_stream, reads only: the "read_only" yardstick of
        bench.py)
One JSON line per batch size; writes no file.
    python tools/iso_probe.py [reps]
The measurement runs in a process of its own under a time limit."""
import json
import subprocess
import sys
from os.path import abspath, dirname

sys.path.insert(0, dirname(abspath(__file__)))
from sample_probe import median_ms, octree            # noqa: E402

N_CELLS, LIMIT_S = 461_130, 420


def rounds_ms(fns, reps, warmup=2):
    """HIP-event times of several variants in interleaved rounds -> {name: (median, min, max)}"""
    import numpy as np
    import torch as pt
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = pt.cuda.Event(enable_timing=True), pt.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            pt.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    return {name: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for name, v in times.items()}


def probe(reps):
    import numpy as np
    import torch as pt
    sys.path.insert(0, ".")
    from sparsespatialsampling_amd import _lib, hipops

    width = 2.4
    centers, levels, nodes, faces = octree(N_CELLS, width)
    n_nodes = len(nodes)
    index = hipops.cell_index(hipops.to_device(centers), hipops.to_device(levels), width)
    d_nodes, d_faces, d_centers = hipops.to_device(nodes), hipops.to_device(faces), hipops.to_device(centers)
    ids = pt.arange(N_CELLS, dtype=pt.int32, device="cuda")
    lib = _lib.hip_lib()

    src = pt.empty((2 << 30) // 4, dtype=pt.float32, device="cuda").normal_()
    dst = pt.empty_like(src)
    moved = hipops.yard_stream(src, dst, 4, 0)
    read_ms = median_ms({"read": lambda: hipops.yard_stream(src, dst, 4, 0)}, reps)["read"][0]
    read_gbs = sum(moved) / (read_ms * 1e-3) / 1e9
    del src, dst

    # concentric shells (cos of the distance) round a centre that drifts from snapshot to snapshot: the surface cuts a few percent of the cells
    rng = np.random.default_rng(0)
    for t_b in (25, 100):
        c = width * (0.5 + 0.1 * rng.standard_normal((t_b, 3)))
        f_node = hipops.to_device(np.stack([np.cos(2 * np.pi / 0.9 * np.linalg.norm(nodes - c[t], axis=1)) for t in range(t_b)], axis=1).astype(np.float32))
        level = 0.0
        n = t_b * N_CELLS
        count = pt.zeros(n + 1, dtype=pt.int32, device="cuda")
        scan = pt.empty_like(count)
        hipops.iso_count(f_node, d_faces, level, out=count)
        hipops.check(lib.s3_exclusive_scan(hipops._ptr(count), hipops._ptr(scan), n + 1, 4, hipops._stream()), "s3_exclusive_scan")
        total = int(scan[n])
        cut = int((count[:n] > 0).sum())
        outs = hipops.iso_emit(f_node, d_faces, level, d_nodes, scan, total)
        work = pt.empty_like(count)
        out = pt.empty((N_CELLS, 1, t_b), dtype=pt.float64, device="cuda")

        def do_scan():
            work.copy_(count)
            hipops.check(lib.s3_exclusive_scan(hipops._ptr(work), hipops._ptr(work), n + 1, 4, hipops._stream()), "s3_exclusive_scan")

        ms = rounds_ms({"count": lambda: hipops.iso_count(f_node, d_faces, level, out=work),
                        "copy_plus_scan": do_scan,
                        "copy": lambda: work.copy_(count),
                        "emit": lambda: hipops.iso_emit(f_node, d_faces, level, d_nodes, scan, total, *outs),
                        "linear": lambda: hipops.cell_sample(ids, f_node, "linear", out=out, index=index, points=d_centers, faces=d_faces)}, reps)
        rows = n_nodes * t_b * 4
        floor = {"count": rows + N_CELLS * 32 + n * 4, "scan": 3 * n * 4, "emit": rows + N_CELLS * 32 + n * 4 + total * 124,
                 "linear": rows + N_CELLS * (32 + 24 + 4 + 24 + 4) + n * 8}
        floor_ms = {k: b / (read_gbs * 1e9) * 1e3 for k, b in floor.items()}
        scan_ms = ms["copy_plus_scan"][0] - ms["copy"][0]
        med = {"count": ms["count"][0], "scan": scan_ms, "emit": ms["emit"][0], "linear": ms["linear"][0]}
        print(json.dumps(dict(
            n_cells=N_CELLS, n_nodes=n_nodes, t_b=t_b, reps=reps, triangles=total, cut_cell_snapshots=cut, cut_share=round(cut / n, 4),
            median_ms={k: round(v, 4) for k, v in med.items()}, min_ms={k: round(v[1], 4) for k, v in ms.items()},
            max_ms={k: round(v[2], 4) for k, v in ms.items()}, read_only_GBs=round(read_gbs, 1), floor_bytes=floor,
            floor_ms={k: round(v, 4) for k, v in floor_ms.items()}, over_floor={k: round(med[k] / floor_ms[k], 2) for k in floor},
            count_over_linear=round(med["count"] / med["linear"], 3),
            count_over_linear_range=[round(ms["count"][1] / ms["linear"][2], 3), round(ms["count"][2] / ms["linear"][1], 3)],
            emit_over_count=round(med["emit"] / med["count"], 3), device=pt.cuda.get_device_name(0))), flush=True)
        del f_node, count, scan, work, out, outs


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--run":
        probe(int(sys.argv[2]))
    else:
        reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
        # a fresh process under its own time limit
        done = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, __file__, "--run", str(reps)])
        if done.returncode != 0:
            sys.exit(f"iso_probe: ended with status {done.returncode}")
