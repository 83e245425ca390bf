"""dev probe (not part of the suite): streamlines and pathlines of an fp32 node velocity on the random octree of sample_probe.py
(461 130 cells, levels 4 .. 9, no body) -- HIP-event medians of interleaved rounds of the fused launch
    stream    hipops.trace_stream, 4096 seeds x T_b = 25 | 100 columns, 16 RK4 steps of the time rule
    path      hipops.trace_path, 10^5 seeds in Hilbert order through 25 snapshots, 4 substeps per interval
against the UNFUSED route on the same seeds and steps in the same run: per RK4 stage hipops.cell_locate, hipops.cell_sample in linear
mode (twice and a torch lerp in a pathline) and a torch update, i.e. about fifteen launches and as many [N_p, 3] round trips through
HBM per step; the streamline columns are walked one after the other there, each on its own contiguous [N_nodes, 3, 1] copy, made
outside the timed region.  Before anything is timed the end points of the particles that take all their steps are compared: the two
routes may differ by the roundings of torch's update alone.
One JSON line per shape; writes no file.
    python tools/trace_probe.py [reps]
The measurement runs in a process of its own under a time limit."""
import json
import subprocess
import sys
from os.path import abspath, dirname

sys.path.insert(0, dirname(abspath(__file__)))
from iso_probe import rounds_ms                         # noqa: E402
from sample_probe import octree                         # noqa: E402

N_CELLS, LIMIT_S = 461_130, 900
N_STREAM, N_PATH, STREAM_STEPS, PATH_SNAPSHOTS, SUBSTEPS = 4096, 100_000, 16, 25, 4


def probe(reps):
    import numpy as np
    import torch as pt
    sys.path.insert(0, ".")
    from sparsespatialsampling_amd import hipops

    width = 2.4
    centers, levels, nodes, faces = octree(N_CELLS, width)
    index = hipops.cell_index(hipops.to_device(centers), hipops.to_device(levels), width)
    d_faces = hipops.to_device(faces)
    h_min = width / 2.0 ** int(levels.max())
    rng = np.random.default_rng(0)

    def swirl(t_b):
        """a vortex about a vertical axis that drifts from snapshot to snapshot, plus a uniform stream: speeds of order one"""
        out = np.empty((len(nodes), 3, t_b), dtype=np.float32)
        for t in range(t_b):
            c = width * (0.5 + 0.1 * np.array([np.cos(0.2 * t), np.sin(0.2 * t)]))
            r = nodes[:, :2] - c
            out[:, 0, t], out[:, 1, t], out[:, 2, t] = 0.3 - r[:, 1], r[:, 0], 0.2 * np.cos(2 * nodes[:, 0])
        return out

    def unfused(columns, seeds, dt, steps, substeps=None):
        """the same steps out of cell_locate + cell_sample + torch; columns: [N_nodes, 3, 1] tensors.  Streamline (substeps None): of
        columns[0]; pathline: through all of them.  -> the end points (NaN where a stage point had no cell)"""
        n = int(seeds.shape[0])
        ids = pt.empty(n, dtype=pt.int32, device="cuda")
        bufs = [pt.empty((n, 3, 1), dtype=pt.float64, device="cuda") for _ in range(2)]

        def velocity(x, col, theta):
            hipops.cell_locate(index, x, out=ids)
            v0 = hipops.cell_sample(ids, columns[col], "linear", out=bufs[0], index=index, points=x, faces=d_faces).view(n, 3)
            if substeps is None:
                return v0.clone()
            v1 = hipops.cell_sample(ids, columns[col + 1], "linear", out=bufs[1], index=index, points=x, faces=d_faces).view(n, 3)
            return pt.lerp(v0, v1, theta)

        x = seeds.clone()
        for s in range(steps):
            col, m = (0, 0) if substeps is None else divmod(s, substeps)
            th = [0.0] * 3 if substeps is None else [(m + f) / substeps for f in (0.0, 0.5, 1.0)]
            k1 = velocity(x, col, th[0])
            k2 = velocity(pt.add(x, k1, alpha=dt / 2), col, th[1])
            k3 = velocity(pt.add(x, k2, alpha=dt / 2), col, th[1])
            k4 = velocity(pt.add(x, k3, alpha=dt), col, th[2])
            x = pt.add(x, (k1 + k4) + 2.0 * (k2 + k3), alpha=dt / 6)
        return x

    def agree(fused_end, done, other):
        diff = (fused_end[done] - other[done]).abs().max().item()
        assert done.any() and diff <= 1e-9 * width, f"the two routes differ by {diff}"
        return diff

    dt = 0.5 * h_min / 1.5
    for t_b in (25, 100):
        field = hipops.to_device(swirl(t_b))
        columns = [field[:, :, t:t + 1].contiguous() for t in range(t_b)]
        seeds = hipops.to_device(width * (0.1 + 0.8 * rng.random((N_STREAM, 3))))
        kw = dict(n_steps=STREAM_STEPS, step="time", dt=dt, every=STREAM_STEPS)
        paths, length, status, _ = hipops.trace_stream(index, d_faces, field, seeds, **kw)
        done = status == hipops.TRACE_STATUS["DONE"]
        diff = max(agree(paths[:, t, 1], done[:, t], unfused(columns[t:t + 1], seeds, dt, STREAM_STEPS)) for t in (0, t_b - 1))
        outs = (paths, length, status, pt.empty_like(status))
        ms = rounds_ms({"fused": lambda: hipops.trace_stream(index, d_faces, field, seeds, **kw, paths=outs[0], length=outs[1],
                                                             status=outs[2], cells=outs[3]),
                        "unfused": lambda: [unfused(columns[t:t + 1], seeds, dt, STREAM_STEPS) for t in range(t_b)]}, reps)
        report("stream", t_b, N_STREAM * t_b, STREAM_STEPS, done.float().mean().item(), diff, ms, reps, pt)
        del field, columns

    field = hipops.to_device(swirl(PATH_SNAPSHOTS))
    columns = [field[:, :, t:t + 1].contiguous() for t in range(PATH_SNAPSHOTS)]
    seeds = hipops.to_device(width * (0.1 + 0.8 * rng.random((N_PATH, 3))))
    order = hipops.spatial_order(seeds)
    dt_snapshot = 2.0 * h_min / 1.5
    steps = (PATH_SNAPSHOTS - 1) * SUBSTEPS
    paths, length, status, _ = hipops.trace_path(index, d_faces, field, seeds, dt_snapshot, SUBSTEPS, order=order)
    done = status == hipops.TRACE_STATUS["DONE"]
    diff = agree(paths[:, -1], done, unfused(columns, seeds, dt_snapshot / SUBSTEPS, steps, SUBSTEPS))
    outs = (paths, length, status, pt.empty_like(status))
    ms = rounds_ms({"fused": lambda: hipops.trace_path(index, d_faces, field, seeds, dt_snapshot, SUBSTEPS, order=order, paths=outs[0],
                                                       length=outs[1], status=outs[2], cells=outs[3]),
                    "fused_file_order": lambda: hipops.trace_path(index, d_faces, field, seeds, dt_snapshot, SUBSTEPS, paths=outs[0],
                                                                  length=outs[1], status=outs[2], cells=outs[3]),
                    "unfused": lambda: unfused(columns, seeds, dt_snapshot / SUBSTEPS, steps, SUBSTEPS)}, reps)
    report("path", PATH_SNAPSHOTS, N_PATH, steps, done.float().mean().item(), diff, ms, reps, pt)


def report(kind, t_b, particles, steps, done_share, diff, ms, reps, pt):
    print(json.dumps(dict(
        kind=kind, n_cells=N_CELLS, t_b=t_b, particles=particles, steps=steps, reps=reps, done_share=round(done_share, 3),
        routes_differ_by=diff, median_ms={k: round(v[0], 4) for k, v in ms.items()}, min_ms={k: round(v[1], 4) for k, v in ms.items()},
        max_ms={k: round(v[2], 4) for k, v in ms.items()}, unfused_over_fused=round(ms["unfused"][0] / ms["fused"][0], 2),
        unfused_over_fused_range=[round(ms["unfused"][1] / ms["fused"][2], 2), round(ms["unfused"][2] / ms["fused"][1], 2)],
        ns_per_particle_step=round(ms["fused"][0] * 1e6 / (particles * steps), 3), device=pt.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--run":
        probe(int(sys.argv[2]))
    else:
        reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
        # a fresh process under its own time limit
        done = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, __file__, "--run", str(reps)])
        if done.returncode != 0:
            sys.exit(f"trace_probe: ended with status {done.returncode}")
