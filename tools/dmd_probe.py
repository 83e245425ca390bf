"""
What does reading float32 in place buy the Gram matrix of a DMD?  Times, at the grid shape of BASELINE config C3 (461 130 cells x
1000 snapshots by default),

    a) s3_gram on the float32 matrix where it lies (no mean, no weights)                       -- what dmd.py does
    b) x.double() + s3_weighted_gram with a zero mean and unit weights                         -- the route without s3_gram

and checks that both give the same bits.  (b) also holds a second matrix of twice the size.

    python tools/dmd_probe.py [n_rows] [n_snapshots] [repeats]

Not run by the tests; DESIGN 5.8 says "not measured" until somebody runs it on an MI355X.
"""
import os
import sys
import time

import torch as pt

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparsespatialsampling_amd import hipops, svd                                       # noqa: E402


def timed(fn, repeats):
    fn()
    pt.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        pt.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, out


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 461130
    t = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    hipops.device()
    x = pt.randn((n, t), dtype=pt.float32, device="cuda", generator=pt.Generator(device="cuda").manual_seed(0))
    zero, one = pt.zeros(n, dtype=pt.float64, device="cuda"), pt.ones(n, dtype=pt.float64, device="cuda")
    flop = 2.0 * n * t * t
    in_place, g_a = timed(lambda: hipops.gram(x), repeats)
    copied, g_b = timed(lambda: svd.weighted_gram(x.double(), zero, one), repeats)
    gram_only, _ = (lambda xd: timed(lambda: svd.weighted_gram(xd, zero, one), repeats))(x.double())
    print(f"[{n}, {t}] float32, {flop / 1e12:.2f} TFLOP nominal")
    print(f"  s3_gram in place                     {in_place * 1e3:9.2f} ms   {flop / in_place / 1e12:6.1f} TFLOP/s")
    print(f"  .double() + s3_weighted_gram         {copied * 1e3:9.2f} ms   (+ {n * t * 8 / 2 ** 30:.1f} GiB for the copy)")
    print(f"  s3_weighted_gram of a resident copy  {gram_only * 1e3:9.2f} ms")
    print(f"  same bits: {bool(pt.equal(g_a.view(pt.int64), g_b.view(pt.int64)))}")
