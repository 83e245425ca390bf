"""
The per-element checker of the interpolation accuracy tests (tests/interp_accuracy.py), on the CPU: it accepts an f64 FMA chain in
either order and rejects the mistakes it exists to catch.  No GPU.
"""
from fractions import Fraction

import numpy as np
import pytest

from tests.interp_accuracy import GUARD_BITS, assert_close, assert_guard, guard_intact, reference, violations


def fma(a, b, c):
    """correctly rounded a * b + c (exact rational arithmetic; float(Fraction) rounds to nearest even, subnormals included)"""
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def fma_chain(w, idx, x, order=1, skip_zero=False, acc_type=float, flush=False, col_shift=0):
    """what a kernel computes: out[c, j] = fma chain over the neighbours in the given order; the keyword arguments are the
    kernel bugs the checker must catch"""
    nc, k = w.shape
    L = x.shape[1]
    out = np.empty((nc, L))
    for c in range(nc):
        for j in range(L):
            acc = acc_type(0.0)
            for m in range(k)[::order]:
                v = float(x[idx[c, m], min(j + col_shift, L - 1)])
                if flush and v != 0.0 and abs(v) < np.finfo(np.float32).tiny:
                    v = 0.0
                if skip_zero and w[c, m] == 0.0:
                    continue
                if acc_type is float:
                    acc = fma(w[c, m], v, acc)
                else:                                        # accumulation in f32
                    acc = acc_type(acc_type(w[c, m] * v) + acc)
            out[c, j] = float(acc)
    return out


def case(seed=0, nc=12, k=26, L=6, n=60, dtype=np.float32, scale=1.0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, L)) * scale).astype(dtype)
    idx = rng.integers(0, n, (nc, k))
    w = rng.random((nc, k))
    w /= w.sum(1, keepdims=True)
    return w, idx, x


@pytest.mark.parametrize("order", [1, -1])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fma_chain_in_either_order_passes(order, dtype):
    w, idx, x = case(order + 3, dtype=dtype)
    x[::5] *= 1e30 if dtype == np.float32 else 1e300               # rows of very different magnitude
    x[1::5] = np.frombuffer(np.arange(1, x[1::5].size + 1, dtype=np.uint32 if dtype == np.float32 else np.uint64).tobytes(),
                            dtype=dtype).reshape(x[1::5].shape)     # subnormals
    x[2::5] = 1e4 + x[2::5] * 1e-3 if dtype == np.float32 else 1e12 + x[2::5] * 1e-6
    w[::3] -= 0.5 / w.shape[1]                                       # signed weights: cancellation
    ref, mag = reference(w, idx, x)
    got = fma_chain(w, idx, x, order=order)
    assert_close(got, ref, mag, w.shape[1], f64_data=dtype == np.float64, what="fma chain")


def test_reference_in_chunks_equals_one_pass():
    w, idx, x = case(1, nc=40)
    r1, m1 = reference(w, idx, x)
    r2, m2 = reference(w, idx, x, cells=np.arange(40)[::-1], cols=[5, 0], budget=7)
    assert np.array_equal(r1[::-1][:, [5, 0]], r2) and np.array_equal(m1[::-1][:, [5, 0]], m2)


def test_f32_accumulation_is_rejected():
    w, idx, x = case(2)
    ref, mag = reference(w, idx, x)
    got = fma_chain(w, idx, x, acc_type=np.float32)
    assert violations(got, ref, mag, w.shape[1]).any()
    with pytest.raises(AssertionError, match="off the long-double reference"):
        assert_close(got, ref, mag, w.shape[1])


def test_dropped_subnormal_is_rejected():
    w, idx, x = case(3)
    x[:] = np.float32(1e-42) * np.sign(x)                            # f32 subnormals only
    ref, mag = reference(w, idx, x)
    assert violations(fma_chain(w, idx, x), ref, mag, w.shape[1]).sum() == 0
    assert violations(fma_chain(w, idx, x, flush=True), ref, mag, w.shape[1]).all()


def test_skipped_zero_weight_neighbour_is_rejected():
    """the reference multiplies every neighbour: a NaN behind a weight of 0 poisons the cell"""
    w, idx, x = case(4, dtype=np.float64)
    w[3] = 0.0
    w[3, 0] = 1.0                                                    # an exact hit
    x[idx[3, 5], 2] = np.nan
    x[idx[7, 1], 4] = np.inf
    w[7, 1] = 0.0                                                    # 0 * Inf = NaN
    ref, mag = reference(w, idx, x)
    assert np.isnan(ref[3, 2]) and np.isnan(ref[7, 4])
    assert violations(fma_chain(w, idx, x), ref, mag, w.shape[1], f64_data=True).sum() == 0
    bad = violations(fma_chain(w, idx, x, skip_zero=True), ref, mag, w.shape[1], f64_data=True)
    assert bad[3, 2] and bad[7, 4]


def test_inf_signs_must_match():
    w, idx, x = case(5, dtype=np.float64)
    x[idx[0, 0], 1] = np.inf
    ref, mag = reference(w, idx, x)
    got = fma_chain(w, idx, x)
    assert violations(got, ref, mag, w.shape[1]).sum() == 0
    got[0, 1] = -np.inf
    assert violations(got, ref, mag, w.shape[1])[0, 1]
    got[0, 1] = np.nan
    assert violations(got, ref, mag, w.shape[1])[0, 1]


def test_off_by_one_column_is_rejected():
    w, idx, x = case(6)
    ref, mag = reference(w, idx, x)
    bad = violations(fma_chain(w, idx, x, col_shift=1), ref, mag, w.shape[1])
    assert bad[:, :-1].all() and not bad[:, -1].any()               # the last column reads itself (clamped)


def test_element_written_past_the_row_is_rejected():
    nc, L, G = 5, 7, 64
    bits = np.full(G + 1 + nc * L + G, GUARD_BITS, dtype=np.int64)
    lo, hi = G + 1, G + 1 + nc * L
    out = bits.view(np.float64)
    out[lo:hi] = 1.0
    assert guard_intact(bits, lo, hi)
    assert_guard(bits, lo, hi)
    for pos, val in ((hi, 1.0), (lo - 1, 0.0)):
        b = bits.copy()
        b.view(np.float64)[pos] = val
        assert not guard_intact(b, lo, hi)
        with pytest.raises(AssertionError, match="guard"):
            assert_guard(b, lo, hi)
    b = bits.copy()                                                  # a NaN written back quietened: other bits, still NaN
    b[hi + 3] |= np.int64(1 << 51)
    assert np.isnan(b.view(np.float64)[hi + 3]) and not guard_intact(b, lo, hi)
