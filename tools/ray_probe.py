"""dev probe (not part of the suite): line-of-sight integrals through a 3-D grid of the cylinder3D size (461 130 cells: the random octree
of tools/sample_probe.py, leaves of levels 4 .. 8) -- a 1024^2 orthographic image along z (``projection.parallel``), fp32 field, T_b = 1 | 25,
cell and linear mode, HIP-event times in interleaved rounds, median [min .. max], of
    tiles       hipops.ray_integrate with the pixels launched in 8 x 8 tiles (what ``parallel`` returns)
    scanline    the same rays in scanline order: what the tile order is worth
    planes      the route there was before, IN THE SAME RUN (cell mode): ``cell_locate`` + ``cell_sample`` on a stack of planes, as many
                as the finest level of the grid has cells along the axis, summed in torch; its accuracy against the fused result is printed
against the floor: the bytes a launch has to move (rays 48 B, results 8 T + 16 B per ray; every field row and the index once) at this
box's streaming-read rate (s3_yard_stream, reads only).  Also: time per ray and per segment, and the share of lanes that idle at the
end of the walk (per wavefront of 64 lanes: 1 - sum segments / (64 max segments)).
One JSON line per mode and batch size; writes no file.
    python tools/ray_probe.py [reps]
The measurement runs in a process of its own under a time limit."""
import json
import subprocess
import sys
from os.path import abspath, dirname

sys.path.insert(0, dirname(abspath(__file__)))
from iso_probe import rounds_ms                        # noqa: E402
from sample_probe import median_ms, octree            # noqa: E402

N_CELLS, LIMIT_S, SIDE = 461_130, 540, 1024


def idle_share(segments, order, lanes_per_ray):
    """the share of lane-steps a wavefront spends waiting for its longest ray (``lanes_per_ray`` adjacent lanes walk one ray)"""
    import numpy as np
    rays_per_wave = max(64 // lanes_per_ray, 1)
    seg = segments[order].astype(np.int64)
    pad = -len(seg) % rays_per_wave
    waves = np.concatenate([seg, np.zeros(pad, dtype=np.int64)]).reshape(-1, rays_per_wave)
    return 1.0 - float(seg.sum()) / float((waves.max(axis=1) * rays_per_wave).sum())


def probe(reps):
    import numpy as np
    import torch as pt
    sys.path.insert(0, ".")
    from sparsespatialsampling_amd import hipops, projection
    from sparsespatialsampling_amd.grid import Grid

    width = 2.4
    centers, levels, nodes, faces = octree(N_CELLS, width)
    grid = Grid(centers, levels, width, nodes, faces)
    index = grid.index
    origins, dirs, tiles = projection.parallel(grid, (0.0, 0.0, 1.0), (SIDE, SIDE))
    n_rays = len(origins)
    d_o, d_d = hipops.to_device(origins), hipops.to_device(dirs)
    orders = {"tiles": hipops.to_device(tiles), "scanline": hipops.to_device(np.arange(n_rays, dtype=np.int32))}

    src = pt.empty((2 << 30) // 4, dtype=pt.float32, device="cuda").normal_()
    dst = pt.empty_like(src)
    moved = hipops.yard_stream(src, dst, 4, 0)
    read_ms = median_ms({"read": lambda: hipops.yard_stream(src, dst, 4, 0)}, reps)["read"][0]
    read_gbs = sum(moved) / (read_ms * 1e-3) / 1e9
    del src, dst

    n_planes, h_min = 1 << index.depth, index.h_min                     # the finest level the grid has (the octree stops short of max_level)
    points = hipops.to_device(np.concatenate([origins[:, :2], np.zeros((n_rays, 1))], axis=1))
    rows = hipops.spatial_order(points)
    rng = np.random.default_rng(0)
    for t_b in (1, 25):
        fields = {"cell": hipops.to_device(rng.standard_normal((N_CELLS, t_b)).astype(np.float32)),
                  "linear": hipops.to_device(rng.standard_normal((len(nodes), t_b)).astype(np.float32))}
        ids = pt.empty(n_rays, dtype=pt.int32, device="cuda")
        plane = pt.empty((n_rays, 1, t_b), dtype=pt.float64, device="cuda")
        total = pt.zeros((n_rays, 1, t_b), dtype=pt.float64, device="cuda")

        def planes():
            total.zero_()
            for k in range(n_planes):
                points[:, 2] = (k + 0.5) * h_min
                hipops.cell_locate(index, points, rows, out=ids)
                hipops.cell_sample(ids, fields["cell"], "cell", rows, out=plane)
                total.add_(plane.nan_to_num_(nan=0.0), alpha=h_min)        # (the few holes of the octree: NaN samples count as nothing)

        for mode in ("cell", "linear"):
            fc = grid.faces if mode == "linear" else None
            outs = [pt.empty((n_rays, 1, t_b), dtype=pt.float64, device="cuda"), pt.empty(n_rays, dtype=pt.float64, device="cuda"),
                    pt.empty(n_rays, dtype=pt.int32, device="cuda"), pt.empty(n_rays, dtype=pt.int32, device="cuda")]
            run = {name: (lambda order=order: hipops.ray_integrate(index, d_o, d_d, fields[mode], mode, fc, order=order, out=outs[0], length=outs[1],
                                                                    segments=outs[2], status=outs[3])) for name, order in orders.items()}
            if mode == "cell":
                run["planes"] = planes
            ms = rounds_ms(run, reps, warmup=1)
            run["tiles"]()
            pt.cuda.synchronize()
            segments = outs[2].cpu().numpy()
            n_seg = int(segments.sum())
            n_rows = N_CELLS if mode == "cell" else len(nodes)
            floor = n_rays * (48 + 8 * t_b + 16) + n_rows * t_b * 4 + N_CELLS * 24 + (N_CELLS * (32 + 24) if mode == "linear" else 0)
            floor_ms = floor / (read_gbs * 1e9) * 1e3
            line = dict(n_cells=N_CELLS, image=[SIDE, SIDE], mode=mode, t_b=t_b, reps=reps, segments=n_seg, segments_per_ray=round(n_seg / n_rays, 1),
                        status_counts=np.bincount(outs[3].cpu().numpy(), minlength=5).tolist(),
                        median_ms={k: round(v[0], 3) for k, v in ms.items()}, min_ms={k: round(v[1], 3) for k, v in ms.items()},
                        max_ms={k: round(v[2], 3) for k, v in ms.items()}, ns_per_ray=round(ms["tiles"][0] * 1e6 / n_rays, 2),
                        ns_per_segment_column=round(ms["tiles"][0] * 1e6 / (n_seg * t_b), 3), scanline_over_tiles=round(ms["scanline"][0] / ms["tiles"][0], 3),
                        read_only_GBs=round(read_gbs, 1), floor_bytes=floor, floor_ms=round(floor_ms, 4), tiles_over_floor=round(ms["tiles"][0] / floor_ms, 1),
                        idle_lane_share={k: round(idle_share(segments, o.cpu().numpy(), min(t_b, 64)), 3) for k, o in orders.items()},
                        device=pt.cuda.get_device_name(0))
            if mode == "cell":
                planes()
                pt.cuda.synchronize()
                scale = float(outs[0].abs().max())
                line.update(planes=n_planes, planes_over_tiles=round(ms["planes"][0] / ms["tiles"][0], 1),
                            planes_over_tiles_range=[round(ms["planes"][1] / ms["tiles"][2], 1), round(ms["planes"][2] / ms["tiles"][1], 1)],
                            planes_max_error_over_max=float((total - outs[0]).abs().max()) / scale)
            print(json.dumps(line), flush=True)
        del fields, ids, plane, total


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--run":
        probe(int(sys.argv[2]))
    else:
        reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
        # a fresh process under its own time limit
        done = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, __file__, "--run", str(reps)])
        if done.returncode != 0:
            sys.exit(f"ray_probe: ended with status {done.returncode}")
