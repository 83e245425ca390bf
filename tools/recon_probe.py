"""dev probe (not part of the suite): the fused reconstruction-error launch at the cylinder3D shape -- N = 4 991 774 original
points, a 461 130-cell grid, k = 26, fp32 original rows, T_b = 25 | 100 snapshots per batch -- HIP-event medians of
    (a) the fused launch (s3_recon_error), points in Hilbert order
    (b) the unfused route made of what the library had before it: hipops.interp into an [N, T_b] f64 tensor + the torch
        reductions of the reference's script (post_processing/compute_error_OAT.py:223-233), points in file order
    (c) the fused launch with the points in file order
against (a)'s own traffic floor N * (12 k + 4 T_b) bytes at this box's streaming-read rate (s3_yard_stream, reads only: the
"read_only" yardstick of bench.py).  The clouds are uniform random in the cylinder3D box (the real grid is graded; the density
ratio, ~11 points per cell, is the same).  Prints one JSON line per batch size; writes no file.
    python tools/recon_probe.py [reps]
(a) is two kernels, recon_kernel and the small recon_reduce_kernel that adds the blocks' partial column sums; HIP events see
their sum.  Their split comes from a kernel trace of the same script, in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/recon_probe.py 3"""
import json
import sys

import numpy as np
import torch as pt

sys.path.insert(0, ".")
from sparsespatialsampling_amd import hipops

N, NC, K = 4_991_774, 461_130, 26
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7


def median_ms(fns, reps, warmup=2):
    """HIP-event medians of several variants, timed in interleaved rounds"""
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


rng = np.random.default_rng(0)
box = np.array([2.4, 2.0, 0.314])
x = hipops.to_device(rng.random((N, 3)) * box)
centers = hipops.to_device(rng.random((NC, 3)) * box)
scale = hipops.to_device(np.sqrt(rng.random(N) + 0.1))
knn = hipops.KnnIndex(centers)
idx, dist = knn.query(x, K)
w = hipops.idw_weights_exact(dist)
knn.close()
del dist
rows = hipops.spatial_order(x)
w_s, idx_s = hipops.gather_rows(w, rows, pt.empty_like(w)), hipops.gather_rows(idx, rows, pt.empty_like(idx))
scale_s = hipops.gather_rows(scale.reshape(-1, 1), rows, pt.empty(N, 1, dtype=pt.float64, device="cuda")).reshape(-1)

src = pt.empty((2 << 30) // 4, dtype=pt.float32, device="cuda").normal_()
dst = pt.empty_like(src)
moved = hipops.yard_stream(src, dst, 4, 0)
read_ms = median_ms({"read": lambda: hipops.yard_stream(src, dst, 4, 0)}, reps)["read"][0]
read_gbs = sum(moved) / (read_ms * 1e-3) / 1e9
del src, dst

for t_b in (25, 100):
    grid = pt.empty((NC, t_b), dtype=pt.float32, device="cuda").normal_().add_(2.0)
    orig = pt.empty((N, t_b), dtype=pt.float32, device="cuda").normal_().add_(2.0)
    mean, m2 = pt.empty(N, dtype=pt.float64, device="cuda"), pt.empty(N, dtype=pt.float64, device="cuda")
    fit = pt.empty((N, t_b), dtype=pt.float64, device="cuda")
    keep = {}

    def fused():
        keep["a"] = hipops.recon_error(w_s, idx_s, grid, orig, rows=rows, scale=scale_s, mean=mean, m2=m2)[2]

    def fused_file_order():
        keep["c"] = hipops.recon_error(w, idx, grid, orig, scale=scale, mean=mean, m2=m2)[2]

    def unfused():
        hipops.interp(w, idx, grid, out=fit)
        fitted = fit * scale[:, None]
        ref = orig.double() * scale[:, None]
        diff = fitted - ref
        e_time = pt.linalg.norm(diff, ord=2, dim=0) / pt.linalg.norm(ref, ord=2, dim=0)
        e_total = pt.linalg.norm(diff) / pt.linalg.norm(ref)
        a = diff.abs()
        keep["b"] = (e_time, e_total, a.mean(dim=1), a.std(dim=1))

    ms = median_ms({"fused": fused, "unfused": unfused, "fused_file_order": fused_file_order,
                    "interp_only_file_order": lambda: hipops.interp(w, idx, grid, out=fit),
                    "interp_only_hilbert_order": lambda: hipops.interp(w_s, idx_s, grid, out=fit)}, reps)
    e_time_fused = (keep["a"][0].sqrt() / keep["a"][1].sqrt())
    agree = float(((e_time_fused - keep["b"][0]).abs() / keep["b"][0].abs()).max())
    floor_bytes = N * (12 * K + 4 * t_b)
    floor_ms = floor_bytes / (read_gbs * 1e9) * 1e3
    print(json.dumps(dict(
        t_b=t_b, n=N, nc=NC, k=K, reps=reps, median_ms={k_: round(v[0], 3) for k_, v in ms.items()},
        min_ms={k_: round(v[1], 3) for k_, v in ms.items()}, read_only_GBs=round(read_gbs, 1), floor_bytes=floor_bytes,
        floor_ms=round(floor_ms, 3), fused_over_floor=round(ms["fused"][0] / floor_ms, 2),
        unfused_over_fused=round(ms["unfused"][0] / ms["fused"][0], 2),
        file_order_over_hilbert=round(ms["fused_file_order"][0] / ms["fused"][0], 2), error_time_max_rel_dev=agree,
        unfused_field_bytes=N * t_b * 8, device=pt.cuda.get_device_name(0))), flush=True)
    del grid, orig, fit, keep
