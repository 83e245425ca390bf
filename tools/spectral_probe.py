"""
What does fusing the power into the segment DFT buy a Welch spectrum?  Times with HIP events, at the grid shape of BASELINE config C3
(461 130 cells x 1000 snapshots, L = 256, 50 % overlap by default),

    a) s3_segment_psd: coefficients in the accumulators, the PSD [N, n_f] written once                     -- what welch does
    b) s3_segment_dft: the coefficients [N, n_f, n_blk, 2] written                                          -- the first step of SPOD
    c) s3_tall_gemm once per segment against the [L, 2 n_f] matrix + a torch reduction of [N, n_blk, 2 n_f] -- the unfused route,
       for comparison only (no mean: the product reads the raw rows)

    python tools/spectral_probe.py [n_rows] [n_snapshots] [nperseg] [repeats]

Not run by the tests; DESIGN 5.10 says "not measured" until somebody runs it on an MI355X.
"""
import os
import sys

import numpy as np
import torch as pt

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparsespatialsampling_amd import hipops, spectral                                  # noqa: E402


def timed(fn, repeats):
    """best of ``repeats`` in ms between two HIP events, after one warm-up call"""
    fn()
    pt.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        start, stop = pt.cuda.Event(enable_timing=True), pt.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        stop.record()
        stop.synchronize()
        best = min(best, start.elapsed_time(stop))
    return best, out


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 461130
    t = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    nperseg = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    hipops.device()
    hop = nperseg - nperseg // 2
    n_blk = (t - nperseg) // hop + 1
    x = pt.randn((n, t), dtype=pt.float32, device="cuda", generator=pt.Generator(device="cuda").manual_seed(0))
    bre, bim, w = spectral.segment_matrix(nperseg, "hann", "constant")
    n_f = bre.shape[1]
    scale = hipops.to_device(spectral.psd_scale(w, 1.0, n_blk, np.arange(n_f), nperseg, "density"))
    bre_d, bim_d = hipops.to_device(bre), hipops.to_device(bim)
    both = hipops.to_device(np.ascontiguousarray(np.concatenate([bre, bim], axis=1)))
    mean = hipops.row_means(x)
    flop = 2.0 * n * n_blk * nperseg * 2 * n_f

    def unfused():
        c = pt.empty((n_blk, n, 2 * n_f), dtype=pt.float64, device="cuda")
        for b in range(n_blk):
            hipops.tall_gemm(x[:, b * hop:b * hop + nperseg], both, out=c[b])
        return (c[:, :, :n_f] ** 2 + c[:, :, n_f:] ** 2).sum(0) * scale

    fused, psd = timed(lambda: hipops.segment_psd(x, mean, nperseg, hop, n_blk, bre_d, bim_d, scale), repeats)
    coefs, _ = timed(lambda: hipops.segment_dft(x, mean, nperseg, hop, n_blk, bre_d, bim_d), repeats)
    print(f"[{n}, {t}] float32, L {nperseg}, hop {hop}: {n_blk} segments, {n_f} frequencies, {flop / 1e12:.2f} TFLOP nominal")
    print(f"  s3_segment_psd (fused)                {fused:9.2f} ms   {flop / fused / 1e9:6.1f} TFLOP/s   writes {n * n_f * 8 / 2 ** 30:.2f} GiB")
    print(f"  s3_segment_dft (coefficients)         {coefs:9.2f} ms   {flop / coefs / 1e9:6.1f} TFLOP/s   writes {n * n_f * n_blk * 16 / 2 ** 30:.2f} GiB")
    try:
        loose, psd_u = timed(unfused, repeats)
        print(f"  s3_tall_gemm per segment + reduction  {loose:9.2f} ms   (+ {n * n_blk * 2 * n_f * 8 / 2 ** 30:.2f} GiB of coefficients)")
        print(f"  largest relative difference of the two PSDs (the unfused one keeps the row mean): "
              f"{float(((psd - psd_u).abs().max(1).values / psd_u.abs().max(1).values).max()):.2e}")
    except pt.cuda.OutOfMemoryError:
        print("  s3_tall_gemm per segment + reduction  does not fit the device")
