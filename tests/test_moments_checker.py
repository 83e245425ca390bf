"""
The per-row checker of the temporal moment tests (tests/moments_cases.py), on the CPU: a float64 emulation of the kernel's scheme
(csrc/metric.hip, operation by operation) passes its bounds with room, the mistakes the checker exists for do not, and the shape
list reaches every path of the launcher.  No GPU.
"""
import numpy as np
import pytest

from tests import moments_cases as mc


def data(t, dtype, base, seed, n=4):
    rng = np.random.default_rng(seed)
    scale = abs(base) * 1e-6 if base else 1.0
    return (base + scale * rng.standard_normal((n, t))).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_emulation_of_the_kernel_passes_with_room(dtype):
    """T from 2 to 20000 (one chunk to hundreds), every vector width and group size, bases 0, 101325, 1e6, -3e4 and 1e-30 with small
    fluctuations, plain and abs, ddof 0 and 1: at most 0.5 of either bound (measured here: 0.28 of the mean bound, 0.11 of M2's)"""
    worst = [0.0, 0.0]
    vecs = (4, 2, 1) if dtype == np.float32 else (2, 1)
    for k, t in enumerate((2, 3, 7, 16, 63, 65, 130, 257, 1000, 1027, 4103, 20000)):
        for j, base in enumerate((0.0, 101325.0, 1e6, -3e4, 1e-30)):
            x = data(t, dtype, base, 100 * k + j, n=2 if t > 2000 else 4)
            for vec in vecs:
                for absolute in (False, True):
                    ref = mc.reference(x, absolute)
                    mean, std = mc.emulated_outputs(x, vec, (k + j) % 2, absolute=absolute)
                    got = mc.assert_moments(mean, std, ref, (k + j) % 2, f"T={t} base={base} vec={vec}")
                    worst = [max(a, b) for a, b in zip(worst, got)]
    # every group size on one row length (the launcher picks one; the kernel is right for each)
    x = data(1030, dtype, 101325.0, 7)
    for g in (4, 8, 16, 32, 64):
        mean, std = mc.emulated_outputs(x, vecs[0], 1, g=g)
        got = mc.assert_moments(mean, std, mc.reference(x), 1, f"G={g}")
        worst = [max(a, b) for a, b in zip(worst, got)]
    print(f"{np.dtype(dtype).name}: worst mean ratio {worst[0]:.3f}, worst M2 ratio {worst[1]:.3f}")
    assert worst[0] <= 0.5 and worst[1] <= 0.5


@pytest.mark.parametrize("dtype,first_kind", [(np.float32, 0), (np.float64, 2)])
def test_emulation_passes_on_the_rows_of_the_gpu_test(dtype, first_kind):
    for t in (1, 3, 66, 517):
        x = mc.make_rows(8, t, dtype, t, first_kind)
        for ddof in (0, 1):
            mean, std = mc.emulated_outputs(x, 2, ddof)
            mc.assert_moments(mean, std, mc.reference(x), ddof, f"T={t}")
            mean, std = mc.emulated_outputs(x, 1, ddof, absolute=True)
            mc.assert_moments(mean, std, mc.reference(x, True), ddof, f"abs T={t}")


def test_one_pass_formula_is_rejected():
    """sum x^2 - T m^2 on float32 pressure (101325 + 0.05 N): orders of magnitude beyond the M2 bound, while its mean passes"""
    x = (101325.0 + 0.05 * np.random.default_rng(1).standard_normal((6, 1000))).astype(np.float32)
    ref = mc.reference(x)
    mean, std = mc.emulated_outputs(x, 4, 1, mistake="one_pass")
    assert mc.mean_ratio(mean, ref).max() <= 1.0
    with np.errstate(invalid="ignore"):
        ratio = mc.m2_ratio(np.nan_to_num(std, nan=0.0), ref, 1)
    assert ratio.min() > 1e3
    with pytest.raises(AssertionError, match="M2 off the long-double reference"):
        mc.assert_moments(mean, np.nan_to_num(std, nan=0.0), ref, 1)


@pytest.mark.parametrize("first_kind", [0, 1, 2, 3])
def test_dropped_last_element_is_rejected(first_kind):
    """one row of each kind, one chunk and several: the mean leaves its bound in every row"""
    for t, vec in ((7, 1), (66, 4), (1030, 2)):
        x = mc.make_rows(4, t, np.float32, 3 + t, first_kind)
        ref = mc.reference(x)
        mean, std = mc.emulated_outputs(x, vec, 0, mistake="drop_last")
        assert (mc.mean_ratio(mean, ref) > 1.0).all(), t
        with pytest.raises(AssertionError, match="mean off the long-double reference"):
            mc.assert_moments(mean, std, ref, 0)


def test_chunks_merged_with_the_wrong_counts_are_rejected():
    """a partial last chunk merged as if it were full: mean and M2 both leave their bounds (rows of two to five chunks)"""
    for t, vec in ((17 * 4, 4), (33 * 2 + 1, 2), (1025, 1), (130, 1)):
        x = mc.make_rows(8, t, np.float32, t, 0)
        ref = mc.reference(x)
        good = mc.emulated_outputs(x, vec, 1)
        mc.assert_moments(good[0], good[1], ref, 1)
        mean, std = mc.emulated_outputs(x, vec, 1, mistake="wrong_counts")
        benign = np.arange(8) % 4 == 0                                    # (a chunk mean differs from the next by ~ sigma / sqrt(n))
        assert (mc.mean_ratio(mean, ref)[benign] > 1.0).all() and (mc.m2_ratio(std, ref, 1)[benign] > 1.0).all(), t
        with pytest.raises(AssertionError):
            mc.assert_moments(mean, std, ref, 1)


def test_checker_edges():
    x = np.array([[2.5], [-1.0]], dtype=np.float32)                       # T = 1
    ref = mc.reference(x)
    assert mc.assert_moments(np.array([2.5, -1.0]), np.array([np.nan, np.nan]), ref, 1) == (0.0, 0.0)
    assert mc.assert_moments(np.array([2.5, -1.0]), np.array([0.0, 0.0]), ref, 0) == (0.0, 0.0)
    assert np.isinf(mc.m2_ratio(np.array([0.0, np.nan]), ref, 1)).tolist() == [True, False]      # ddof 1 wants NaN
    assert np.isinf(mc.m2_ratio(np.array([np.nan, 0.0]), ref, 0)).tolist() == [True, False]      # ddof 0 wants 0
    assert np.isinf(mc.mean_ratio(np.array([np.nan, -1.0]), ref)).tolist() == [True, False]
    zero = mc.reference(np.zeros((1, 5)))
    assert mc.mean_ratio(np.array([0.0]), zero)[0] == 0.0 and np.isinf(mc.mean_ratio(np.array([1e-300]), zero)[0])
    const = mc.reference(np.full((1, 9), 3.0, dtype=np.float32))
    assert mc.m2_ratio(np.array([0.0]), const, 1)[0] == 0.0 and np.isinf(mc.m2_ratio(np.array([-0.5]), const, 1)[0])


def test_shapes_reach_every_path_of_the_launcher():
    """every (G, per_lane) launch_moments can choose, each with one chunk or several as far as it can have them, every ragged tail,
    rows shorter than a vector, every row count class per G; every vector width of both dtypes has a contiguous and a pitched layout"""
    reachable = {(4, 8), (8, 8), (8, 16), (16, 8), (16, 16), (32, 16), (64, 16)}
    assert {mc.lanes_per_row(n) for n in range(0, 3000)} == reachable
    for vec in (4, 2, 1):
        sh = mc.shapes(vec)
        assert {(s.g, s.per_lane) for s in sh} == reachable
        assert any(s.chunks == 1 and s.n_vec > 0 for s in sh) and all(any(s.g == g and s.chunks > 1 for s in sh) for g in (4, 8, 16, 32, 64))
        assert {s.n_tail for s in sh} == set(range(vec))
        assert vec == 1 or any(s.n_vec == 0 for s in sh)
        for g in (4, 8, 16, 32, 64):
            assert {s.n_rows for s in sh if s.g == g} >= set(mc.row_counts(g)), (vec, g)
            assert {s.n_tail for s in sh if s.g == g} == set(range(vec))
            for n_vec in (1, 4 * g - 1, 4 * g, 4 * g + 1, 8 * g + 1):
                assert n_vec in mc.N_VECS
    for (itemsize, vec), names in mc.LAYOUTS.items():
        for s in mc.shapes(vec):
            fits = [name for name in names if mc.layout_fits(name, s.row_len, itemsize, vec)]
            assert set(fits) >= set(names) - {"contiguous"}, (itemsize, s)
            for name in fits:
                stride, _ = mc.layout(name, s.row_len, itemsize)
                assert stride >= s.row_len and (name == "contiguous" or stride > s.row_len)
        assert any(mc.layout_fits("contiguous", s.row_len, itemsize, vec) for s in mc.shapes(vec))
    assert mc.kernel_vec(4, 8, 256) == 4 and mc.kernel_vec(4, 8, 264) == 2 and mc.kernel_vec(4, 6, 256) == 2 and mc.kernel_vec(4, 8, 260) == 1
    assert mc.kernel_vec(8, 4, 256) == 2 and mc.kernel_vec(8, 4, 264) == 1 and mc.kernel_vec(8, 3, 256) == 1
