"""dev probe (not part of the suite): the overlap table behind region tracking on a 3-D grid of the cylinder3D size (461 130 cells: the
random octree of tools/region_probe.py, levels 4 .. 9), labels int32 [N_cells, T_b + 1] from ``hipops.region_label``, the overlap of
the windows ``[:, :T_b]`` and ``[:, 1:]``, T_b = 25 | 100 -- HIP-event times in interleaved rounds, median [min .. max], of
    count, scan, emit, sort, heads, scan2, reduce       every launch of the chain on the arrays the one before it left
    overlap       hipops.overlap_table                  (the whole chain; its host work -- allocations, two read-backs -- is inside)
    region_table  hipops.region_table of the same window, IN THE SAME RUN: the same count / scan / emit / sort skeleton, the yardstick
for the three masks of tools/region_probe.py: random with a share of 30 % and of 70 % in, drawn per column (the second percolates: most
in-cells of a column lie in one region, and so in one edge), and the serpentine (one region in every column: one edge of every
in-cell), against
    (a) the floor: the bytes the chain has to move at this box's streaming-read rate (s3_yard_stream, reads only) -- both windows
        once for the count and once for the emit, the flag array three times for its scan and once for the emit, 12 bytes a pair
        written, 12 bytes a pair four times per radix pass, keys and cells once for the heads, the heads three times for their scan,
        cells and edge numbers once for the sums
    (b) the host: both windows downloaded, then per step ``numpy.unique`` on the pairs (a, b) of the cells in both, with counts (timed
        on HOST_STEPS steps; the volume would be a ``bincount`` more)
One JSON line per mask and batch size; writes no file.
    python tools/overlap_probe.py [reps]
The measurement runs in a process of its own under a time limit."""
import json
import subprocess
import sys
import time
from os.path import abspath, dirname

sys.path.insert(0, dirname(abspath(__file__)))
from iso_probe import rounds_ms                        # noqa: E402
from sample_probe import median_ms, octree            # noqa: E402

N_CELLS, LIMIT_S, HOST_STEPS = 461_130, 540, 3


def probe(reps):
    import numpy as np
    import torch as pt
    sys.path.insert(0, ".")
    from sparsespatialsampling_amd import hipops

    width = 2.4
    centers, levels, _, _ = octree(N_CELLS, width)
    index = hipops.cell_index(hipops.to_device(centers), hipops.to_device(levels), width)
    nbr = hipops.cell_neighbours(index)
    order = hipops.spatial_order(index.centers)

    src = pt.empty((2 << 30) // 4, dtype=pt.float32, device="cuda").normal_()
    dst = pt.empty_like(src)
    moved = hipops.yard_stream(src, dst, 4, 0)
    read_ms = median_ms({"read": lambda: hipops.yard_stream(src, dst, 4, 0)}, reps)["read"][0]
    read_gbs = sum(moved) / (read_ms * 1e-3) / 1e9
    del src, dst

    rng = np.random.default_rng(0)
    band = width / 32
    slab = np.floor(centers[:, 0] / band).astype(np.int64)
    snake = (slab % 2 == 0) | ((slab % 4 == 1) & (centers[:, 1] > width - 2 * band)) | ((slab % 4 == 3) & (centers[:, 1] < 2 * band))
    for t_b in (25, 100):
        for mask_name in ("random30", "random70", "serpentine"):
            if mask_name == "serpentine":
                mask = np.repeat(snake[:, None], t_b + 1, axis=1)
            else:
                mask = rng.random((N_CELLS, t_b + 1)) < (0.3 if mask_name == "random30" else 0.7)
            field = hipops.to_device(mask.astype(np.float32))
            del mask
            labels = hipops.region_label(field, nbr, 0.5, np.inf, order=order)
            del field
            a, b = labels[:, :t_b], labels[:, 1:]
            table = hipops.overlap_table(a, b, index)
            n_edges, largest = int(table["offsets"][-1]), int(table["n_cells"].max())

            # the arrays every launch of the chain works on, made once in the order of the chain
            n = t_b * N_CELLS
            w, tb = hipops.overlap_key_bits(N_CELLS, t_b)
            flags = pt.zeros(n + 1, dtype=pt.int32, device="cuda")
            hipops.overlap_count(a, b, index, out=flags)
            scan = hipops.exclusive_scan(flags)
            n_pairs = int(scan[-1])
            keys, vals = pt.empty(n_pairs, dtype=pt.int64, device="cuda"), pt.empty(n_pairs, dtype=pt.int32, device="cuda")
            hipops.overlap_emit(a, b, index, scan, keys, vals)
            raw_keys, raw_vals = keys.clone(), vals.clone()
            hipops.sort_pairs(keys, vals, tb + 2 * w)
            heads = pt.zeros(n_pairs + 1, dtype=pt.int32, device="cuda")
            hipops.overlap_heads(keys, vals, index, b, out=heads)
            edge = hipops.exclusive_scan(heads)
            work_k, work_v = pt.empty_like(keys), pt.empty_like(vals)

            def copy_pairs():
                work_k.copy_(raw_keys), work_v.copy_(raw_vals)

            def copy_plus_sort():
                copy_pairs()
                hipops.sort_pairs(work_k, work_v, tb + 2 * w)

            ms = rounds_ms({"count": lambda: hipops.overlap_count(a, b, index, out=flags),
                            "scan": lambda: hipops.exclusive_scan(flags),
                            "emit": lambda: hipops.overlap_emit(a, b, index, scan, work_k, work_v),
                            "copy": copy_pairs, "copy_plus_sort": copy_plus_sort,
                            "heads": lambda: hipops.overlap_heads(keys, vals, index, b, out=heads),
                            "scan2": lambda: hipops.exclusive_scan(heads),
                            "reduce": lambda: hipops.overlap_reduce(keys, vals, index, b, edge, n_edges),
                            "overlap": lambda: hipops.overlap_table(a, b, index),
                            "region_table": lambda: hipops.region_table(a, index)}, reps)
            ms["sort"] = tuple(x - y for x, y in zip(ms.pop("copy_plus_sort"), ms.pop("copy")))
            passes = -(-(tb + 2 * w) // 8)
            floor = 8 * n + 12 * n + 8 * n + 4 * n + 12 * n_pairs + passes * 48 * n_pairs + 12 * n_pairs + 12 * n_pairs + 8 * n_pairs
            floor_ms = floor / (read_gbs * 1e9) * 1e3

            pt.cuda.synchronize()
            t0 = time.perf_counter()
            h_a, h_b = a.cpu().numpy(), b.cpu().numpy()
            download_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            for t in range(HOST_STEPS):
                both = (h_a[:, t] >= 0) & (h_b[:, t] >= 0)              # (what region_label gave: every label names a root)
                np.unique((h_a[both, t].astype(np.int64) << 32) | h_b[both, t], return_counts=True)
            host_ms = (download_s / t_b + (time.perf_counter() - t0) / HOST_STEPS) * 1e3

            print(json.dumps(dict(
                n_cells=N_CELLS, t_b=t_b, mask=mask_name, reps=reps, pairs=n_pairs, edges=n_edges, largest_edge_cells=largest, key_bits=tb + 2 * w,
                median_ms={k: round(v[0], 4) for k, v in ms.items()}, min_ms={k: round(v[1], 4) for k, v in ms.items()},
                max_ms={k: round(v[2], 4) for k, v in ms.items()}, read_only_GBs=round(read_gbs, 1), floor_bytes=floor, floor_ms=round(floor_ms, 4),
                overlap_over_floor=round(ms["overlap"][0] / floor_ms, 2), overlap_over_region_table=round(ms["overlap"][0] / ms["region_table"][0], 3),
                host_ms_per_step=round(host_ms, 2), host_over_gpu_per_step=round(host_ms / (ms["overlap"][0] / t_b), 1),
                device=pt.cuda.get_device_name(0))), flush=True)
            del labels, a, b, table, flags, scan, keys, vals, raw_keys, raw_vals, heads, edge, work_k, work_v


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--run":
        probe(int(sys.argv[2]))
    else:
        reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
        # a fresh process under its own time limit
        done = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, __file__, "--run", str(reps)])
        if done.returncode != 0:
            sys.exit(f"overlap_probe: ended with status {done.returncode}")
