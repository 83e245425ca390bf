"""dev probe (not part of the suite): connected regions on a 3-D grid of the cylinder3D size (461 130 cells: a random octree in a box,
levels 4 .. 9, no body), fp32 cell field [N_cells, T_b], T_b = 25 | 100 -- HIP-event medians, 7 interleaved rounds, of
    neighbours    hipops.cell_neighbours            (once per grid: per cell 2 d keys and binary searches)
    init          hipops.region_label, phase init   (reads the field, writes [N_cells, T_b] int32)
    hook          ..., phase hook, after an init    (union-find on the label array: agent-scope atomics, cells in Hilbert order)
    flatten       ..., phase flatten, after a hook  (one chase per in-cell)
    table         hipops.region_table               (count, scan, keys, radix sort by region, one group of 16 lanes per region; its
                                                    host work -- allocations, the read-back of the totals -- is inside the figure)
for three masks: random with a share of 30 % and of 70 % in (drawn per column; the second percolates: one region holds most in-cells)
and a serpentine (slabs in x joined at alternating ends in y: one region whose diameter is its length, the deep-tree worst case),
against
    (a) the floor: the bytes each pass has to move at this box's streaming-read rate (s3_yard_stream, reads only: the "read_only"
        yardstick of bench.py) -- init: field + labels; hook: labels read and written + the table; flatten: labels read and written;
        table: labels twice, the count array three times, 12 bytes a pair four times per radix pass
    (b) hipops.cell_sample in cell mode with one query per cell, in the same run: the kernel that reads the same field rows once and
        writes 8 T_b bytes per cell
    (c) the host: field.cpu(), then per snapshot the mask, the in-subgraph and scipy.sparse.csgraph.connected_components (timed on
        HOST_SNAPSHOTS snapshots, per snapshot; the neighbour table is downloaded once, outside the figure)
One JSON line per mask and batch size; writes no file.
    python tools/region_probe.py [reps]
The measurement runs in a process of its own under a time limit."""
import json
import subprocess
import sys
import time
from os.path import abspath, dirname

sys.path.insert(0, dirname(abspath(__file__)))
from iso_probe import rounds_ms                        # noqa: E402
from sample_probe import median_ms, octree            # noqa: E402

N_CELLS, LIMIT_S, HOST_SNAPSHOTS = 461_130, 540, 3


def probe(reps):
    import numpy as np
    import torch as pt
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    sys.path.insert(0, ".")
    from sparsespatialsampling_amd import hipops

    width = 2.4
    centers, levels, _, _ = octree(N_CELLS, width)
    index = hipops.cell_index(hipops.to_device(centers), hipops.to_device(levels), width)
    nbr = hipops.cell_neighbours(index)
    order = hipops.spatial_order(index.centers)
    ids = pt.arange(N_CELLS, dtype=pt.int32, device="cuda")
    h_nbr = nbr.cpu().numpy()
    e_i, e_f = np.nonzero(h_nbr >= 0)
    e_j = h_nbr[e_i, e_f]

    src = pt.empty((2 << 30) // 4, dtype=pt.float32, device="cuda").normal_()
    dst = pt.empty_like(src)
    moved = hipops.yard_stream(src, dst, 4, 0)
    read_ms = median_ms({"read": lambda: hipops.yard_stream(src, dst, 4, 0)}, reps)["read"][0]
    read_gbs = sum(moved) / (read_ms * 1e-3) / 1e9
    del src, dst
    nbr_ms = rounds_ms({"neighbours": lambda: hipops.cell_neighbours(index, out=nbr)}, reps)["neighbours"]

    rng = np.random.default_rng(0)
    band = width / 32
    slab = np.floor(centers[:, 0] / band).astype(np.int64)
    snake = (slab % 2 == 0) | ((slab % 4 == 1) & (centers[:, 1] > width - 2 * band)) | ((slab % 4 == 3) & (centers[:, 1] < 2 * band))
    for t_b in (25, 100):
        for mask_name in ("random30", "random70", "serpentine"):
            if mask_name == "serpentine":
                mask = np.repeat(snake[:, None], t_b, axis=1)
            else:
                mask = rng.random((N_CELLS, t_b)) < (0.3 if mask_name == "random30" else 0.7)
            field = hipops.to_device(mask.astype(np.float32))
            del mask
            labels = hipops.region_label(field, nbr, 0.5, np.inf, order=order)
            table = hipops.region_table(labels, index)
            n_regions, largest = int(table["offsets"][-1]), int(table["n_cells"].max())
            work, hooked = pt.empty_like(labels), pt.empty_like(labels)
            hipops.region_label(field, nbr, 0.5, np.inf, order=order, out=hooked, phases=("init", "hook"))
            out = pt.empty((N_CELLS, 1, t_b), dtype=pt.float64, device="cuda")

            def init_plus_hook():
                hipops.region_label(field, nbr, 0.5, np.inf, order=order, out=work, phases=("init", "hook"))

            def copy_plus_flatten():
                work.copy_(hooked)
                hipops.region_label(field, nbr, 0.5, np.inf, out=work, phases=("flatten",))

            ms = rounds_ms({"init": lambda: hipops.region_label(field, nbr, 0.5, np.inf, out=work, phases=("init",)),
                            "init_plus_hook": init_plus_hook, "copy_plus_flatten": copy_plus_flatten, "copy": lambda: work.copy_(hooked),
                            "table": lambda: hipops.region_table(labels, index),
                            "cell_sample": lambda: hipops.cell_sample(ids, field, "cell", out=out)}, reps)
            med = {"init": ms["init"][0], "hook": ms["init_plus_hook"][0] - ms["init"][0],
                   "flatten": ms["copy_plus_flatten"][0] - ms["copy"][0], "table": ms["table"][0], "cell_sample": ms["cell_sample"][0]}
            med["label"] = med["init"] + med["hook"] + med["flatten"]
            n = t_b * N_CELLS
            passes = max(1, -(-max(n_regions, 1).bit_length() // 8))
            floor = {"init": 8 * n, "hook": 8 * n + N_CELLS * 24, "flatten": 8 * n, "table": 8 * n + 12 * n + passes * 48 * n,
                     "cell_sample": 4 * n + 8 * n + 4 * N_CELLS}
            floor["label"] = floor["init"] + floor["hook"] + floor["flatten"]
            floor_ms = {k: b / (read_gbs * 1e9) * 1e3 for k, b in floor.items()}

            pt.cuda.synchronize()
            t0 = time.perf_counter()
            h_field = field.cpu().numpy()
            download_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            for t in range(HOST_SNAPSHOTS):
                m = h_field[:, t] >= 0.5
                keep = m[e_i] & m[e_j]
                connected_components(coo_matrix((np.ones(int(keep.sum()), dtype=np.int8), (e_i[keep], e_j[keep])), shape=(N_CELLS, N_CELLS)),
                                     directed=False)
            host_ms = (download_s / t_b + (time.perf_counter() - t0) / HOST_SNAPSHOTS) * 1e3

            print(json.dumps(dict(
                n_cells=N_CELLS, t_b=t_b, mask=mask_name, reps=reps, regions=n_regions, largest_region_cells=largest,
                neighbours_ms=[round(v, 4) for v in nbr_ms], median_ms={k: round(v, 4) for k, v in med.items()},
                min_ms={k: round(v[1], 4) for k, v in ms.items()}, max_ms={k: round(v[2], 4) for k, v in ms.items()},
                read_only_GBs=round(read_gbs, 1), floor_bytes=floor, floor_ms={k: round(v, 4) for k, v in floor_ms.items()},
                over_floor={k: round(med[k] / floor_ms[k], 2) for k in floor}, label_over_cell_sample=round(med["label"] / med["cell_sample"], 3),
                host_ms_per_snapshot=round(host_ms, 2), host_over_gpu_per_snapshot=round(host_ms / ((med["label"]) / t_b), 1),
                device=pt.cuda.get_device_name(0))), flush=True)
            del field, labels, work, hooked, out, table


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--run":
        probe(int(sys.argv[2]))
    else:
        reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
        # a fresh process under its own time limit
        done = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, __file__, "--run", str(reps)])
        if done.returncode != 0:
            sys.exit(f"region_probe: ended with status {done.returncode}")
