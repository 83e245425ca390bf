"""The temporal moment kernels (s3_row_moments / s3_row_abs_moments, csrc/metric.hip) through the C ABI on the GPU: every row against
its long-double moments within the per-row bounds of tests/moments_cases.py, at every path of the launcher (vector width, lanes per
row, chunks, ragged tails, dead rows), in contiguous, pitched and misaligned layouts with NaN in the padding, with canaries around the
outputs; the conditions that need no tolerance (constant rows, T = 1, a poisoned row beside clean ones, two runs); RunningMoments
and temporal_mean_abs_sum on top."""
import ctypes as C

import numpy as np
import pytest
import torch as pt

from tests import moments_cases as mc

pytestmark = pytest.mark.gpu

LD = mc.LD
DTYPES = {4: np.float32, 8: np.float64}
GUARD = 64                                                   # canary doubles on each side of an output
CANARY = -7.25
WORST = {}                                                   # family -> worst (mean, M2) ratio seen, printed by each test


@pytest.fixture(scope="module")
def ops():
    from sparsespatialsampling_amd import hipops
    hipops.device()
    return hipops


def note(family, ratios):
    old = WORST.get(family, (0.0, 0.0))
    WORST[family] = (max(old[0], ratios[0]), max(old[1], ratios[1]))


def device_rows(dense, name):
    """-> (device buffer, address of the first row, row pitch): the rows of ``dense`` in layout ``name``; the padding of every row, the
    elements before the first row and a tail behind the last are NaN, so that a read outside a row shows in the result"""
    n, t = dense.shape
    stride, offset = mc.layout(name, t, dense.itemsize)
    buf = np.full(offset + n * stride + 16, np.nan, dtype=dense.dtype)
    buf[offset:offset + n * stride].reshape(n, stride)[:, :t] = dense
    dev = pt.from_numpy(buf).cuda()
    assert dev.data_ptr() % 256 == 0
    return dev, dev.data_ptr() + offset * dense.itemsize, stride


def moments(ops, address, itemsize, n, t, stride, ddof, want_mean=True, want_std=True, absolute=False):
    """one call of the entry point; -> (mean or None, std or None) as numpy, after checking the canaries around both outputs"""
    from sparsespatialsampling_amd import _lib
    lib = _lib.hip_lib()
    out = pt.full((2, GUARD + n + GUARD), CANARY, dtype=pt.float64, device="cuda")
    ptr = [C.c_void_p(out[i, GUARD:].data_ptr()) if want else None for i, want in enumerate((want_mean, want_std))]
    fn = lib.s3_row_abs_moments if absolute else lib.s3_row_moments
    ops.check(fn(C.c_void_p(address), 0 if itemsize == 4 else 1, n, t, stride, ddof, ptr[0], ptr[1], ops._stream()), "s3_row_moments")
    host = out.cpu().numpy()
    assert (host[:, :GUARD] == CANARY).all() and (host[:, GUARD + n:] == CANARY).all(), "a write outside an output"
    for i, want in enumerate((want_mean, want_std)):
        if not want:
            assert (host[i] == CANARY).all(), "a write to an output that was not asked for"
    return (host[0, GUARD:GUARD + n].copy() if want_mean else None), (host[1, GUARD:GUARD + n].copy() if want_std else None)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


_CASES = {}


def case(itemsize, shape):
    """(rows, reference, reference of |rows|) of one shape, made once and shared by the layouts"""
    key = (itemsize, shape.vec, shape.index)
    if key not in _CASES:
        x = mc.make_rows(shape.n_rows, shape.row_len, DTYPES[itemsize], 1000 * shape.vec + shape.index, first_kind=shape.index)
        _CASES[key] = (x, mc.reference(x), mc.reference(x, absolute=True))
    return _CASES[key]


@pytest.mark.parametrize("itemsize,vec,name", [(k[0], k[1], name) for k, names in mc.LAYOUTS.items() for name in names])
def test_every_row_within_its_bounds_of_the_long_double_moments(ops, itemsize, vec, name):
    """all shapes of moments_cases.shapes(vec) this layout can hold: mean and std (ddof 1) together, the mean alone (same bits), the std
    alone (ddof 0), the abs entry point, a second run (same bits)"""
    ran = 0
    for shape in mc.shapes(vec):
        if not mc.layout_fits(name, shape.row_len, itemsize, vec):
            continue
        x, ref, ref_abs = case(itemsize, shape)
        dev, address, stride = device_rows(x, name)
        assert mc.kernel_vec(itemsize, stride, address) == vec and stride >= shape.row_len
        args = (ops, address, itemsize, shape.n_rows, shape.row_len, stride)
        mean, std = moments(*args, 1)
        note("moments", mc.assert_moments(mean, std, ref, 1, f"{shape} {name}"))
        only_mean, none = moments(*args, 1, want_std=False)
        assert none is None and same_bits(only_mean, mean), shape
        none, biased = moments(*args, 0, want_mean=False)
        note("moments", mc.assert_moments(None, biased, ref, 0, f"{shape} {name} ddof 0"))
        ddof = shape.index % 2
        a_mean, a_std = moments(*args, ddof, absolute=True)
        note("abs moments", mc.assert_moments(a_mean, a_std, ref_abs, ddof, f"{shape} {name} abs"))
        again = moments(*args, 1)
        assert same_bits(again[0], mean) and same_bits(again[1], std), shape
        del dev
        ran += 1
    assert ran >= len(mc.shapes(vec)) // 4
    print(f"[{itemsize * 8}-bit vec {vec} {name}] {ran} shapes; worst |error| / bound so far: {WORST}")


@pytest.mark.parametrize("name,vec", [("pitch16", 4), ("pitch8", 2), ("odd", 1)])
def test_constant_float32_rows_are_exact(ops, name, vec):
    """a constant float32 row: every partial sum of n 24-bit values is exact in float64, so is its division by n, every deviation is 0
    and every merge adds 0: mean == float64(c) and std == 0.0 to the bit, for every row length in use"""
    consts = np.array([1.0, -3.0, 101325.0, 0.1, 1e-30, -16777215.0, 3.4e38, 1.401298464324817e-45, 0.0], dtype=np.float32)
    for shape in mc.shapes(vec):
        x = np.repeat(consts[:, None], shape.row_len, axis=1)
        dev, address, stride = device_rows(x, name)
        assert mc.kernel_vec(4, stride, address) == vec
        for absolute in (False, True):
            mean, std = moments(ops, address, 4, len(consts), shape.row_len, stride, 0, absolute=absolute)
            want = np.abs(consts) if absolute else consts
            assert same_bits(mean, want.astype(np.float64)), shape
            assert same_bits(std, np.zeros(len(consts))), shape


@pytest.mark.parametrize("itemsize", [4, 8])
def test_one_value_per_row(ops, itemsize):
    """T = 1: NaN for ddof 1, 0.0 for ddof 0, the mean is the value"""
    x = mc.make_rows(70, 1, DTYPES[itemsize], 5)
    for name in ("contiguous", "odd", "pitch16"):
        dev, address, stride = device_rows(x, name)
        mean, std = moments(ops, address, itemsize, 70, 1, stride, 1)
        assert same_bits(mean, x[:, 0].astype(np.float64)) and np.isnan(std).all()
        mean, std = moments(ops, address, itemsize, 70, 1, stride, 0)
        assert same_bits(mean, x[:, 0].astype(np.float64)) and same_bits(std, np.zeros(70))


@pytest.mark.parametrize("vec,n_vec", [(4, 16), (4, 33), (2, 65), (4, 129), (1, 257), (4, 1025)])
def test_a_poisoned_row_leaves_the_others_alone(ops, vec, n_vec):
    """NaN, +inf or -inf somewhere in ONE row -- the first, a middle and the last row of the second workgroup in turn: that row's std is
    NaN and its mean not finite (NaN for a NaN; for an infinity the exact mean is that infinity, and the kernel gives it or NaN
    depending on the chunk it sits in), and every other row has the bits of the run without it.  A shuffle wider than the row's lane
    group, or a merge across rows, would spread it."""
    g = mc.lanes_per_row(n_vec)[0]
    rows_per_group = 256 // g
    n, t = 3 * rows_per_group + 1, n_vec * vec + (vec - 1)
    x = mc.make_rows(n, t, np.float32, n_vec)
    name = {4: "pitch16", 2: "pitch8", 1: "odd"}[vec]
    dev, address, stride = device_rows(x, name)
    assert mc.kernel_vec(4, stride, address) == vec
    clean = {absolute: moments(ops, address, 4, n, t, stride, 1, absolute=absolute) for absolute in (False, True)}
    assert all(np.isfinite(out).all() for pair in clean.values() for out in pair)
    others = np.ones(n, dtype=bool)
    for row in (rows_per_group, rows_per_group + rows_per_group // 2, 2 * rows_per_group - 1):
        others[:] = True
        others[row] = False
        for poison, col in ((np.nan, 0), (np.inf, t - 1), (-np.inf, t // 2), (np.nan, t - 1)):
            y = x.copy()
            y[row, col] = poison
            dev, address, stride = device_rows(y, name)
            for absolute in (False, True):
                mean, std = moments(ops, address, 4, n, t, stride, 1, absolute=absolute)
                assert np.isnan(std[row]) and not np.isfinite(mean[row]), (row, poison)
                assert not np.isnan(poison) or np.isnan(mean[row])
                assert same_bits(mean[others], clean[absolute][0][others]) and same_bits(std[others], clean[absolute][1][others]), (row, poison)


def test_running_moments_of_ill_conditioned_batches(ops):
    """float32 pressure (101325 + 0.05 N) arriving in ragged batches, one of a single snapshot and an empty one: the merged moments
    against the long-double moments of the concatenation, with the bounds of the whole row (T = the total count)"""
    from sparsespatialsampling_amd import metrics
    n, t = 700, 407
    x = (101325.0 + 0.05 * np.random.default_rng(11).standard_normal((n, 2, t))).astype(np.float32)
    field = pt.from_numpy(x)
    run = metrics.RunningMoments()
    for a, b in ((0, 100), (100, 101), (101, 101), (101, 300), (300, 407)):
        run.update(field[:, :, a:b].cuda())
    assert run.count == t
    ref = mc.reference(x.reshape(-1, t))
    mean = run.mean().cpu().numpy().reshape(-1)
    for ddof, unbiased in ((1, True), (0, False)):
        note("RunningMoments", mc.assert_moments(mean, run.std(unbiased).cpu().numpy().reshape(-1), ref, ddof, f"running ddof {ddof}"))
    print(f"worst |error| / bound: {WORST['RunningMoments']}")


@pytest.mark.parametrize("dtype,t", [(np.float32, 37), (np.float64, 400)])
def test_mean_abs_sum_of_components_that_cancel(ops, dtype, t):
    """[N, 3, T] with components that cancel in sign (u, -u / 2 + noise, -u / 2 - noise): n_comp times the long-double mean of |x| over
    the cell's n_comp T values, within n_comp times the mean bound of that row"""
    from sparsespatialsampling_amd import metrics
    n = 333
    rng = np.random.default_rng(t)
    u = 101325.0 + 0.05 * rng.standard_normal((n, t))
    noise = 1e-3 * rng.standard_normal((n, t))
    x = np.stack([u, -0.5 * u + noise, -0.5 * u - noise], axis=1).astype(dtype)
    assert np.abs(x.astype(np.float64).sum(axis=1)).max() < 0.1                    # the plain sum cancels
    got = metrics.temporal_mean_abs_sum(pt.from_numpy(x).cuda()).cpu().numpy()
    ref = mc.reference(x.reshape(n, 3 * t), absolute=True)
    err = np.abs(got.astype(LD) - LD(3) * ref["m"])
    bound = LD(3) * mc.mean_bound(ref)
    ratio = float((err / bound).max())
    note("mean_abs_sum", (ratio, 0.0))
    print(f"worst |error| / bound: {ratio:.3g}")
    assert ratio <= 1.0
