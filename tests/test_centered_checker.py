"""
The per-element bounds of the centred / weighted Gram and GEMM tests (tests/centered_cases.py), on the CPU: a float64 emulation of the
kernels' arithmetic stays a factor 4 inside them on the shapes and data of the GPU test, and the mistakes they exist for do not.  No GPU.
"""
import numpy as np
import pytest

from tests import centered_cases as cc

WORST = {"gram": 0.0, "gemm": 0.0, "residual": 0.0}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,t", [(1, 3), (15, 17), (17, 33), (257, 33), (3000, 17), (3000, 40)])
def test_gram_emulation_has_a_factor_four_of_room(n, t, dtype):
    x = cc.rows(n, t, dtype, 7 * n + t)
    mean, weight = cc.row_means(x), cc.weights(n, n + t)
    for m, w in ((mean, weight), (mean, None), (None, weight)):
        ref, mag = cc.gram_reference(x, m, w)
        r = cc.ratio(cc.gram_emulated(x, m, w), ref, cc.gram_bound(n, mag))
        WORST["gram"] = max(WORST["gram"], r)
        assert r <= 0.25, (r, m is None, w is None)
    print(f"worst |error| / bound so far: {WORST}")


@pytest.mark.parametrize("m,k,n", [(1, 3, 1), (15, 17, 4), (17, 130, 65), (257, 130, 80), (257, 3, 64)])
def test_gemm_emulation_has_a_factor_four_of_room(m, k, n):
    """inside the bounds at every k; a factor 4 inside from k = 17 on (at k = 3 three roundings stand against 7 u: centered_cases.py)"""
    rng = np.random.default_rng(m + k + n)
    left = cc.rows(m, k, np.float64, m + 31 * n + k)
    lmean = cc.row_means(left)
    b = rng.standard_normal((k, n))
    e = cc.rows(m, n, np.float64, 5 + m)
    emean = cc.row_means(e) + 1e-3 * rng.standard_normal(m)
    for lm in (lmean, None):
        ref, bound = cc.gemm_reference(left, lm, b)
        r = cc.ratio(cc.gemm_emulated(left, lm, b), ref, bound)
        WORST["gemm"] = max(WORST["gemm"], r)
        assert r <= (0.25 if k >= 17 else 1.0), r
        for em in (emean, None):
            ref, bound = cc.gemm_reference(left, lm, b, e, em)
            r = cc.ratio(cc.gemm_emulated(left, lm, b, e, em), ref, bound)
            WORST["residual"] = max(WORST["residual"], r)
            assert r <= (0.25 if k >= 17 else 1.0), r
    print(f"worst |error| / bound so far: {WORST}")


def test_gram_mistakes_are_rejected():
    n, t = 257, 17
    x = cc.rows(n, t, np.float32, 1)
    mean, weight = cc.row_means(x), cc.weights(n, 2)
    ref, mag = cc.gram_reference(x, mean, weight)
    bound = cc.gram_bound(n, mag)
    assert cc.ratio(cc.gram_emulated(x, mean, weight), ref, bound) <= 0.25
    assert cc.ratio(cc.gram_emulated(x, mean, weight, mistake="weight_twice"), ref, bound) > 1e6
    assert cc.ratio(cc.gram_emulated(x, mean, weight, mistake="mean_f32"), ref, bound) > 1e6
    shifted = cc.gram_emulated(x, np.roll(mean, 1), weight)                       # the mean of the row before
    assert cc.ratio(shifted, ref, bound) > 1e6
    nan = cc.gram_emulated(x, mean, weight)
    nan[3, 5] = np.nan
    assert cc.ratio(nan, ref, bound) == np.inf
    # a norm-wise check would not see an error of this size in a small entry: one element off by 1e-13 of the largest
    small = cc.gram_emulated(x, mean, weight)
    i, j = np.unravel_index(np.argmin(np.abs(ref)), ref.shape)
    small[i, j] += 1e-13 * float(np.abs(ref).max())
    assert abs(small[i, j] - float(ref[i, j])) <= 1e-12 * float(np.abs(ref).max()) and cc.ratio(small, ref, bound) > 1.0


def test_gemm_mistakes_are_rejected():
    m, k, n = 65, 33, 17
    rng = np.random.default_rng(3)
    left, b, e = cc.rows(m, k, np.float64, 1), rng.standard_normal((k, n)), cc.rows(m, n, np.float64, 2)
    lmean, emean = cc.row_means(left), cc.row_means(e)
    ref, bound = cc.gemm_reference(left, lmean, b)
    assert cc.ratio(cc.gemm_emulated(left, lmean, b), ref, bound) <= 0.25
    assert cc.ratio(cc.gemm_emulated(left, lmean, b, mistake="mean_f32"), ref, bound) > 1e6
    ref, bound = cc.gemm_reference(left, lmean, b, e, emean)
    assert cc.ratio(cc.gemm_emulated(left, lmean, b, e, emean), ref, bound) <= 0.25
    assert cc.ratio(cc.gemm_emulated(left, lmean, b, e, emean, mistake="no_emean"), ref, bound) > 1e6
    assert cc.ratio(cc.gemm_emulated(left, lmean, b, e, np.roll(emean, 1)), ref, bound) > 1e6
