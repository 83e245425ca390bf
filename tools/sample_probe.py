"""dev probe (not part of the suite): sampling a 1024 x 1024 plane through a 3-D grid of the cylinder3D size (461 130 cells: a random
octree in a box, levels 4 .. 8, no body) -- HIP-event medians, fp32 fields [rows, T_b], T_b = 25 | 100, queries in Hilbert launch
order, of
    cell      hipops.cell_sample, mode "cell"   (reads one cell row per query, writes [Nq, T_b] f64)
    linear    hipops.cell_sample, mode "linear" (reads eight node rows per query, writes [Nq, T_b] f64)
    locate    hipops.cell_locate of the 1024^2 queries (runs once per probe set; not tuned)
against
    (a) hipops.gather_rows with the same ids and the same row bytes in the same run: the pure-copy yardstick of the cell mode (it
        writes fp32 rows, half the bytes the sample writes; ``gather_rows_f64`` copies f64 rows: the sample's output bytes)
    (b) the floor: every touched field row once, the query tables and the output once, at this box's streaming-read rate
        (s3_yard_stream, reads only: the "read_only" yardstick of bench.py)
One JSON line per batch size; writes no file.
    python tools/sample_probe.py [reps]
The measurement runs in a process of its own under a time limit."""
import json
import subprocess
import sys

N_CELLS, SIDE, LIMIT_S = 461_130, 1024, 420


def median_ms(fns, reps, warmup=2):
    """HIP-event medians of several variants, timed in interleaved rounds"""
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
    return {name: (float(np.median(v)), float(np.min(v))) for name, v in times.items()}


def octree(n_cells, width, seed=0, first_level=4, max_level=9):
    """a random octree with exactly ``n_cells`` leaves: every round splits a random third of the leaves that may still be split;
    the last round splits as many as are needed and up to six leaves are dropped (a full octree has 1 mod 7 leaves)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    side = np.arange(1 << first_level)
    pos = np.array(np.meshgrid(side, side, side, indexing="ij")).reshape(3, -1).T.astype(np.int64) << (max_level - first_level)
    lev = np.full(len(pos), first_level)
    kids = np.array(np.meshgrid([0, 1], [0, 1], [0, 1], indexing="ij")).reshape(3, -1).T
    while len(pos) < n_cells:
        can = np.flatnonzero(lev < max_level)
        take = rng.permutation(can)[:min(len(can) // 3 + 1, (n_cells - len(pos) + 6) // 7)]
        size = 1 << (max_level - lev[take] - 1)
        new_pos = (pos[take][:, None, :] + kids[None] * size[:, None, None]).reshape(-1, 3)
        keep = np.ones(len(pos), dtype=bool)
        keep[take] = False
        pos, lev = np.concatenate([pos[keep], new_pos]), np.concatenate([lev[keep], np.repeat(lev[take] + 1, 8)])
    order = rng.permutation(len(pos))[:n_cells]
    pos, lev = pos[order], lev[order]
    size = 1 << (max_level - lev)
    h_min = width / 2.0 ** max_level
    signs = np.array([s + (z,) for z in (1, 0) for s in [(0, 0), (0, 1), (1, 1), (1, 0)]])
    corners = (pos[:, None, :] + signs[None] * size[:, None, None]).reshape(-1, 3)
    uniq, inverse = np.unique(corners, axis=0, return_inverse=True)
    return (pos + size[:, None] / 2) * h_min, lev.astype(np.int32), uniq * h_min, inverse.reshape(-1, 8).astype(np.int32)


def probe(reps):
    import numpy as np
    import torch as pt
    sys.path.insert(0, ".")
    from sparsespatialsampling_amd import hipops, sampling

    width = 2.4
    centers, levels, nodes, faces = octree(N_CELLS, width)
    pts = sampling.plane([0.0, 0.0, 0.37 * width], [width, 0.0, 0.0], [0.0, width, 0.0], (SIDE, SIDE))
    index = hipops.cell_index(hipops.to_device(centers), hipops.to_device(levels), width)
    d_pts, d_faces = hipops.to_device(pts), hipops.to_device(faces)
    rows = hipops.spatial_order(d_pts)
    ids = hipops.cell_locate(index, d_pts, rows=rows)
    hipops.synchronize()
    nq, hit = int(ids.numel()), int((ids >= 0).sum())
    safe = ids.clamp(min=0)
    ids_launch = hipops.gather_rows(safe.view(-1, 1), rows, pt.empty_like(safe.view(-1, 1))).view(-1)       # the ids in launch order
    cells_hit = pt.unique(safe)
    n_cells_hit, n_nodes_hit = int(cells_hit.numel()), int(pt.unique(d_faces[cells_hit.long()]).numel())

    src = pt.empty((2 << 30) // 4, dtype=pt.float32, device="cuda").normal_()
    dst = pt.empty_like(src)
    moved = hipops.yard_stream(src, dst, 4, 0)
    read_ms = median_ms({"read": lambda: hipops.yard_stream(src, dst, 4, 0)}, reps)["read"][0]
    read_gbs = sum(moved) / (read_ms * 1e-3) / 1e9
    del src, dst
    locate_ms = median_ms({"locate": lambda: hipops.cell_locate(index, d_pts, rows=rows, out=ids)}, reps)["locate"]

    for t_b in (25, 100):
        f_cell = pt.empty((N_CELLS, t_b), dtype=pt.float32, device="cuda").normal_()
        f_node = pt.empty((len(nodes), t_b), dtype=pt.float32, device="cuda").normal_()
        f_cell64 = f_cell.double()
        out = pt.empty((nq, 1, t_b), dtype=pt.float64, device="cuda")
        copy32, copy64 = pt.empty((nq, t_b), dtype=pt.float32, device="cuda"), pt.empty((nq, t_b), dtype=pt.float64, device="cuda")
        ms = median_ms({"cell": lambda: hipops.cell_sample(ids, f_cell, "cell", rows=rows, out=out),
                        "linear": lambda: hipops.cell_sample(ids, f_node, "linear", rows=rows, out=out, index=index, points=d_pts, faces=d_faces),
                        "cell_file_order": lambda: hipops.cell_sample(ids, f_cell, "cell", out=out),
                        "gather_rows": lambda: hipops.gather_rows(f_cell, ids_launch, copy32),
                        "gather_rows_f64": lambda: hipops.gather_rows(f_cell64, ids_launch, copy64)}, reps)
        hipops.cell_sample(ids, f_cell, "cell", rows=rows, out=out)
        hipops.gather_rows(f_cell, safe, copy32)
        same = bool(pt.equal(out[:, 0][ids >= 0], copy32.double()[ids >= 0]))
        floor = {"cell": n_cells_hit * t_b * 4 + nq * (8 * t_b + 8),
                 "linear": n_nodes_hit * t_b * 4 + n_cells_hit * (24 + 4 + 32) + nq * (8 * t_b + 8 + 24)}
        floor_ms = {k: b / (read_gbs * 1e9) * 1e3 for k, b in floor.items()}
        print(json.dumps(dict(
            n_cells=N_CELLS, n_nodes=len(nodes), queries=nq, hits=hit, cells_hit=n_cells_hit, nodes_hit=n_nodes_hit, depth=index.depth,
            t_b=t_b, reps=reps, median_ms={k: round(v[0], 4) for k, v in ms.items()}, min_ms={k: round(v[1], 4) for k, v in ms.items()},
            locate_median_ms=round(locate_ms[0], 4), read_only_GBs=round(read_gbs, 1), floor_bytes=floor,
            floor_ms={k: round(v, 4) for k, v in floor_ms.items()},
            over_floor={k: round(ms[k][0] / floor_ms[k], 2) for k in floor},
            cell_over_gather_rows=round(ms["cell"][0] / ms["gather_rows"][0], 2),
            cell_over_gather_rows_f64=round(ms["cell"][0] / ms["gather_rows_f64"][0], 2),
            linear_over_cell=round(ms["linear"][0] / ms["cell"][0], 2), cell_equals_gather=same, device=pt.cuda.get_device_name(0))), flush=True)
        del f_cell, f_node, f_cell64, out, copy32, copy64


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--run":
        probe(int(sys.argv[2]))
    else:
        reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
        # a fresh process under its own time limit
        done = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, __file__, "--run", str(reps)])
        if done.returncode != 0:
            sys.exit(f"sample_probe: ended with status {done.returncode}")
