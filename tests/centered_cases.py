"""
Data, long-double references, per-element bounds and float64 emulations for the centred / weighted forms of the Gram kernel
(s3_weighted_gram, s3_gram with mean and weight) and of the GEMM (s3_centered_gemm with lmean and with minus_from), csrc/svd.hip.
Shared by tests/test_centered_checker.py (CPU) and tests/test_gpu_dmd.py.  numpy only.

Every reference takes the very doubles handed to the kernel as mean / weight / lmean / emean.  u = 2^-53.

Gram: ``G_ij = sum_n a_n d_ni d_nj``, ``d = x - mean`` in long double; bound ``(N + 8) u sum_n a_n |d_ni| |d_nj|``.  The kernel stages
``fl(fl(x - mean) fl(sqrt(a)))`` per factor -- three roundings each, six per term -- multiplies exactly inside the FMA and adds N
terms: at most (N - 1) + 6 roundings of quantities bounded by the running sum of |terms|, to first order (N + 5) u sum |terms|.

GEMM: ``C = (L - lmean) B``; bound ``(k + 4) u sum_k |l - lmean| |b|``: one rounding for the centring, k for the FMA chain.  Residual
form ``C = (E - emean) - (L - lmean) B``: plus ``2 u |e - emean|`` (the rounding of ``e - emean``, and that of the final subtraction
as far as this operand goes) ``+ u |c_ref|`` (the final subtraction, measured at the result).

The emulations below do the kernel's arithmetic in one long chain of fused multiply-adds (the kernel's chains are shorter); on the
shapes of the GPU test they reach 0.18 of the Gram bound, and 0.12 (product) / 0.25 (residual) of the GEMM bounds for k >= 17: a factor 4
of room, asserted by tests/test_centered_checker.py.  At k = 3 they reach 0.28 / 0.31: three or four roundings of up to one u each
stand against a bound of 7 u -- first-order worst cases leave no factor 4 at such a k whatever the constant short of 4 (k + 1), and
the bounds are not widened for it: they hold for every rounding pattern, which is what the GPU test relies on.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def rows(n, t, dtype, seed):
    """[n, t]: row means about 1e5 (5 % apart), fluctuation 1e-2 -- what a pressure field looks like to a centred product"""
    rng = np.random.default_rng(seed)
    return (1e5 * (1.0 + 0.05 * rng.standard_normal((n, 1))) + 1e-2 * rng.standard_normal((n, t))).astype(dtype)


def weights(n, seed):
    """cell areas spanning 1e-6 .. 1e2, both ends present"""
    w = 10.0 ** np.random.default_rng(seed).uniform(-6.0, 2.0, n)
    w[0], w[-1] = 1e-6, 1e2
    return w


def row_means(x):
    return np.asarray(x, dtype=np.float64).mean(axis=1)


# ---- Gram -------------------------------------------------------------------------------------------------------------------------
def gram_reference(x, mean=None, weight=None):
    """(G, sum of |terms|) [T, T] in long double"""
    d = np.asarray(x).astype(LD)
    if mean is not None:
        d = d - np.asarray(mean, dtype=np.float64).astype(LD)[:, None]
    a = np.ones(len(d), dtype=LD) if weight is None else np.asarray(weight, dtype=np.float64).astype(LD)
    return (d * a[:, None]).T @ d, (np.abs(d) * a[:, None]).T @ np.abs(d)


def ratio(got, ref, bound):
    """largest |got - ref| / bound over the elements (0 / 0 = 0, anything not a number = inf)"""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf))
    return float(np.where(np.isnan(r), np.inf, r).max())


def fma(a, b, c):
    """a * b + c rounded once to float64, as the matrix cores do it (formed in long double, whose 64-bit significand leaves the one
    rounding to float64 all but alone)"""
    return (np.asarray(a).astype(LD) * np.asarray(b).astype(LD) + np.asarray(c).astype(LD)).astype(np.float64)


def gram_bound(n, mag):
    return LD(n + 8) * LD(U) * mag


def gram_emulated(x, mean=None, weight=None, mistake=None):
    """float64: every factor ``(x - mean) * sqrt(a)``, the terms added row after row.  ``mistake``: "weight_twice" multiplies each factor
    by a instead of sqrt(a); "mean_f32" centres with the mean rounded to float32"""
    y = np.asarray(x).astype(np.float64)
    if mean is not None:
        y = y - (np.asarray(mean).astype(np.float32).astype(np.float64) if mistake == "mean_f32" else np.asarray(mean))[:, None]
    if weight is not None:
        y = y * (np.asarray(weight) if mistake == "weight_twice" else np.sqrt(np.asarray(weight)))[:, None]
    acc = np.zeros((y.shape[1], y.shape[1]))
    for row in y:
        acc = fma(row[:, None], row[None, :], acc)
    return acc


# ---- GEMM -------------------------------------------------------------------------------------------------------------------------
def gemm_reference(left, lmean, b, e=None, emean=None):
    """(C, bound) [m, n] in long double; ``lmean`` / ``emean`` may be None"""
    dl = np.asarray(left).astype(LD)
    if lmean is not None:
        dl = dl - np.asarray(lmean, dtype=np.float64).astype(LD)[:, None]
    bl = np.asarray(b, dtype=np.float64).astype(LD)
    k = dl.shape[1]
    prod, bound = dl @ bl, LD(k + 4) * LD(U) * (np.abs(dl) @ np.abs(bl))
    if e is None:
        return prod, bound
    de = np.asarray(e, dtype=np.float64).astype(LD)
    if emean is not None:
        de = de - np.asarray(emean, dtype=np.float64).astype(LD)[:, None]
    c = de - prod
    return c, bound + LD(2) * LD(U) * np.abs(de) + LD(U) * np.abs(c)


def gemm_emulated(left, lmean, b, e=None, emean=None, mistake=None):
    """float64, column after column of ``left``.  ``mistake``: "mean_f32" as above; "no_emean" forgets to centre ``e``"""
    dl = np.asarray(left).astype(np.float64)
    if lmean is not None:
        dl = dl - (np.asarray(lmean).astype(np.float32).astype(np.float64) if mistake == "mean_f32" else np.asarray(lmean))[:, None]
    b = np.asarray(b, dtype=np.float64)
    acc = np.zeros((dl.shape[0], b.shape[1]))
    for kk in range(dl.shape[1]):
        acc = fma(dl[:, kk][:, None], b[kk][None, :], acc)
    if e is None:
        return acc
    de = np.asarray(e, dtype=np.float64)
    if emean is not None and mistake != "no_emean":
        de = de - np.asarray(emean)[:, None]
    return de - acc
