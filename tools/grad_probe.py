"""dev probe (not part of the suite): the fused least-squares derivatives (s3_grad_apply) at the cylinder3D shapes -- the generated
grid (461 130 cells) and the source cloud (4 991 774 points), k = 26, an fp32 velocity [N, 3, T_b], T_b = 25 | 100 -- HIP-event
medians of
    (a) the fused launches: vorticity magnitude (writes [N, T_b]) and the full gradient (writes [N, 9, T_b]), points in Hilbert
        launch order
    (b) the unfused route made of what the library had before: hipops.interp once per axis over a table of k + 1 columns (the
        coefficients and minus their sum for the point itself) into an [N, 3, 3, T_b] f64 tensor, then torch arithmetic for the
        vorticity magnitude
    (c) the fused launches with the points in file order (no row list; the clouds are numbered at random, which is the worst a
        file can do)
against the floor N * (k (8 d + 4) + n_comp T_b s_in + 8 n_out T_b) bytes -- the tables, every field row once, the output -- at
this box's streaming-read rate (s3_yard_stream, reads only: the "read_only" yardstick of bench.py).  The clouds are uniform
random in the cylinder3D box.  One JSON line per cloud and batch size; writes no file.
    python tools/grad_probe.py [reps]
Every cloud runs in a process of its own under a time limit; the first one that fails ends the probe."""
import json
import subprocess
import sys

N_GRID, N_CLOUD, K, DIM, N_COMP = 461_130, 4_991_774, 26, 3, 3
LIMIT_S = {"grid": 300, "cloud": 600}


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


def probe(which, reps):
    import numpy as np
    import torch as pt
    sys.path.insert(0, ".")
    from sparsespatialsampling_amd import hipops
    from sparsespatialsampling_amd.differential import drop_self

    n = N_GRID if which == "grid" else N_CLOUD
    rng = np.random.default_rng(0)
    x = hipops.to_device(rng.random((n, DIM)) * np.array([2.4, 2.0, 0.314]))
    knn = hipops.KnnIndex(x)
    idx = drop_self(knn.query(x, K + 1)[0])
    knn.close()
    rows = hipops.spatial_order(x)
    idx_s = hipops.gather_rows(idx, rows, pt.empty_like(idx))
    coef, _, n_deg = hipops.grad_coeff(x, idx, 2)
    coef_s = hipops.grad_coeff(x, idx_s, 2, rows=rows)[0]
    # the unfused route's tables: k + 1 columns, the last one the point itself with minus the sum of the others
    idx_x = pt.cat([idx, pt.arange(n, dtype=pt.int32, device="cuda").unsqueeze(1)], dim=1).contiguous()
    w_x = [pt.cat([coef[:, :, a], -coef[:, :, a].sum(dim=1, keepdim=True)], dim=1).contiguous() for a in range(DIM)]

    src = pt.empty((2 << 30) // 4, dtype=pt.float32, device="cuda").normal_()
    dst = pt.empty_like(src)
    moved = hipops.yard_stream(src, dst, 4, 0)
    read_ms = median_ms({"read": lambda: hipops.yard_stream(src, dst, 4, 0)}, reps)["read"][0]
    read_gbs = sum(moved) / (read_ms * 1e-3) / 1e9
    del src, dst

    for t_b in (25, 100):
        u = pt.empty((n, N_COMP, t_b), dtype=pt.float32, device="cuda").normal_().add_(2.0)
        out1 = pt.empty((n, 1, t_b), dtype=pt.float64, device="cuda")
        out9 = pt.empty((n, N_COMP * DIM, t_b), dtype=pt.float64, device="cuda")
        per_axis = pt.empty((DIM, n, N_COMP, t_b), dtype=pt.float64, device="cuda")
        keep = {}

        def unfused():
            for a in range(DIM):
                hipops.interp(w_x[a], idx_x, u, out=per_axis[a])
            g = per_axis                                                        # g[axis][:, comp]
            keep["b"] = ((g[1][:, 2] - g[2][:, 1]) ** 2 + (g[2][:, 0] - g[0][:, 2]) ** 2 + (g[0][:, 1] - g[1][:, 0]) ** 2).sqrt()

        def fused_vm():
            keep["a"] = hipops.grad_apply(coef_s, idx_s, u, "vorticity_magnitude", rows=rows, out=out1)

        ms = median_ms({"fused_vorticity_magnitude": fused_vm,
                        "fused_gradient": lambda: hipops.grad_apply(coef_s, idx_s, u, "gradient", rows=rows, out=out9),
                        "unfused_vorticity_magnitude": unfused,
                        "fused_vorticity_magnitude_file_order": lambda: hipops.grad_apply(coef, idx, u, "vorticity_magnitude", out=out1),
                        "fused_gradient_file_order": lambda: hipops.grad_apply(coef, idx, u, "gradient", out=out9)}, reps)
        fused_vm()
        unfused()
        agree = float((keep["a"][:, 0] - keep["b"]).abs().max() / keep["b"].abs().max())
        floor = {name: n * (K * (8 * DIM + 4) + N_COMP * t_b * 4 + 8 * n_out * t_b) for name, n_out in (("vorticity_magnitude", 1), ("gradient", 9))}
        floor_ms = {name: b / (read_gbs * 1e9) * 1e3 for name, b in floor.items()}
        print(json.dumps(dict(
            cloud=which, n=n, k=K, t_b=t_b, reps=reps, n_degenerate=n_deg, median_ms={k_: round(v[0], 3) for k_, v in ms.items()},
            min_ms={k_: round(v[1], 3) for k_, v in ms.items()}, read_only_GBs=round(read_gbs, 1), floor_bytes=floor,
            floor_ms={k_: round(v, 3) for k_, v in floor_ms.items()},
            fused_over_floor={name: round(ms["fused_" + name][0] / floor_ms[name], 2) for name in floor},
            unfused_over_fused=round(ms["unfused_vorticity_magnitude"][0] / ms["fused_vorticity_magnitude"][0], 2),
            file_order_over_hilbert={name: round(ms[f"fused_{name}_file_order"][0] / ms["fused_" + name][0], 2) for name in floor},
            fused_vs_unfused_max_rel_dev=agree, unfused_tensor_bytes=n * 9 * t_b * 8, fused_output_bytes=n * t_b * 8,
            device=pt.cuda.get_device_name(0))), flush=True)
        del u, out1, out9, per_axis, keep


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--case":
        probe(sys.argv[2], int(sys.argv[3]))
    else:
        reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
        for which in ("grid", "cloud"):
            # a fresh process per cloud, under its own time limit; nothing more is started on the device after a failure
            done = subprocess.run(["timeout", "-k", "10", str(LIMIT_S[which]), sys.executable, __file__, "--case", which, str(reps)])
            if done.returncode != 0:
                sys.exit(f"grad_probe: the {which} case ended with status {done.returncode}; nothing further is run")
