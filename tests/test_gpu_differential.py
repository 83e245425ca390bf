"""
Least-squares derivatives on the GPU (csrc/differential.hip, sparsespatialsampling_amd/differential.py) against the long-double
reference of tests/grad_cases.py.

Bounds (none of them measured on the code under test):
  coefficients   per row, the largest deviation within ``(k + 16) * cond * 2**-52`` of the row's largest |c|: k summed products, a
                 d x d Cholesky factorisation and its two solves, amplified by the condition of M.  The definition in plain f64
                 on the CPU sits a factor 6 below it (tests/test_grad_checker.py).  The identity sum_m c[m, a] dx[m, b] = delta_ab
                 within the same bound.
  GRADIENT       per element ``(k + 3) * 2**-53 * mag``, mag = sum_m |c_m (f_m - f_i)|: one rounding of the difference (none for
                 f32 data) and an fma chain of k terms in any order.
  DIVERGENCE, VORTICITY   ``(k + 6) * 2**-53 *`` the summed mag of the entries involved: up to two further additions.
  MAGNITUDE, VORTICITY_MAGNITUDE, Q   within 1e-12 of the output's largest value: the contract of metrics.py and test_gpu_recon.py
                 (plain f64 on the CPU: 5e-16).

Shapes: 3001 points -- twelve workgroups of 256 launch positions, the last one ragged; T = 1 .. 300 covers one lane group of every
width (4 .. 64 lanes), vector and element loads, and rows of several chunks (T = 100 and 300 with element loads: 2 and 5 sweeps).
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch as pt

from tests import grad_cases as gc
from tests.interp_accuracy import GUARD_BITS, assert_guard
from sparsespatialsampling_amd import _lib, hipops
from sparsespatialsampling_amd.differential import Gradient, drop_self

pytestmark = pytest.mark.gpu

TOL = 1e-12
GUARD = 512
N = gc.N_POINTS
PERM = np.random.default_rng(99).permutation(N).astype(np.int32)


def dev(a):
    return pt.from_numpy(np.ascontiguousarray(a)).cuda()


def tables(cs, with_rows):
    """(coef, idx, rows) on the device: in the order of PERM with the row list, or in point order without one"""
    c64 = cs["c"].astype(np.float64)
    if with_rows:
        return dev(c64[PERM]), dev(cs["idx"][PERM]), dev(PERM)
    return dev(c64), dev(cs["idx"]), None


def run(coef, idx, field, mode, rows=None):
    """``hipops.grad_apply`` into an allocation with guard zones on both sides -> numpy [n, n_out, T]"""
    n, dim = int(coef.shape[0]), int(coef.shape[2])
    n_comp = int(field.shape[1]) if field.dim() == 3 else 1
    t = int(field.shape[-1]) if field.dim() > 1 else 1
    numel = n * hipops.grad_n_out(mode, dim, n_comp) * t
    buf = pt.full((GUARD + numel + GUARD,), int(GUARD_BITS), dtype=pt.int64, device="cuda")
    out = buf.view(pt.float64)[GUARD:GUARD + numel]
    res = hipops.grad_apply(coef, idx, field, mode, rows=rows, out=out)
    assert res is out
    assert_guard(buf.cpu().numpy(), GUARD, GUARD + numel, f"{mode} {tuple(field.shape)}")
    return out.cpu().numpy().reshape(n, -1, t)


def pitched(field2d):
    """the same rows with pitch T + 3 and NaN in the padding: rows that start off every vector boundary"""
    wide = pt.full((field2d.shape[0], field2d.shape[1] + 3), float("nan"), dtype=field2d.dtype, device="cuda")
    wide[:, :field2d.shape[1]] = field2d
    return wide[:, :field2d.shape[1]]


# ---- coefficients ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_rows", [False, True])
@pytest.mark.parametrize("name,k", gc.CASES)
def test_coefficients(name, k, with_rows):
    cs = gc.case(name, k)
    n = len(cs["points"])
    order = np.random.default_rng(7).permutation(n).astype(np.int32) if with_rows else np.arange(n, dtype=np.int32)
    coef, flag, n_deg = hipops.grad_coeff(dev(cs["points"]), dev(cs["idx"][order]), cs["power"], rows=dev(order) if with_rows else None)
    c = np.empty((n, k, cs["points"].shape[1]))
    c[order] = coef.cpu().numpy()
    f = np.empty(n, dtype=bool)
    f[order] = flag.cpu().numpy().astype(bool)
    assert np.array_equal(f, cs["flag"]) and n_deg == int(cs["flag"].sum()) == len(cs["planted"])
    assert not c[cs["flag"]].any()
    ok = ~cs["flag"]
    bound = (k + 16) * cs["cond"][ok] * 2.0 ** -52
    devn = (np.abs(c.astype(gc.LD) - cs["c"])[ok].max(axis=(1, 2)) / np.abs(cs["c"][ok]).max(axis=(1, 2))).astype(np.float64)
    ident = gc.identity_error(c, cs["points"], cs["idx"])[ok]
    print(f"{name} k {k} rows {with_rows}: coefficients at {(devn / bound).max():.3g} of the bound, identity at {(ident / bound).max():.3g}")
    assert (devn <= bound).all(), f"coefficients at {(devn / bound).max():.3g} of the bound"
    assert (ident <= bound).all(), f"identity at {(ident / bound).max():.3g} of the bound"


@pytest.mark.parametrize("power", [0, 1])
def test_coefficients_other_powers(power):
    cs = gc.case("lattice3d", 7, power)
    coef, flag, n_deg = hipops.grad_coeff(dev(cs["points"]), dev(cs["idx"]), power)
    c = coef.cpu().numpy()
    bound = (7 + 16) * cs["cond"] * 2.0 ** -52
    devn = (np.abs(c.astype(gc.LD) - cs["c"]).max(axis=(1, 2)) / np.abs(cs["c"]).max(axis=(1, 2))).astype(np.float64)
    assert n_deg == 0 and not flag.any() and (devn <= bound).all()


# ---- apply: linear outputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 6, 7, 25, 64, 100, 300])
@pytest.mark.parametrize("name,k", [("lattice2d", 8), ("lattice3d", 26)])
def test_linear_outputs_against_long_double(name, k, t):
    """GRADIENT of 1, 2 and 3 components, DIVERGENCE and VORTICITY, f32 and f64, dense and pitched rows, with and without a row
    list (the product is thinned: every T sees every value of each, not every combination).  Judged per element: on all points
    for the short rows, on 500 of them (first, last and a seeded sample) for the long ones."""
    cs = gc.case(name, k)
    d = cs["points"].shape[1]
    sample = np.arange(N) if t <= 7 else np.unique(np.concatenate([[0, N - 1], np.random.default_rng(t).choice(N, 498, replace=False)]))
    for f64 in (False, True):
        f = gc.field(N, d, t, f64, seed=100 * t + f64)
        f[5, 0, 0], f[N - 2, d - 1, t - 1], f[1500, 0, t // 2] = np.nan, np.inf, -np.inf
        g, mag = gc.apply(cs["c"].astype(np.float64), cs["idx"], f, sample)
        fd = dev(f)
        with_rows = bool((t + f64) % 2)
        what = f"{name} T {t} {'f64' if f64 else 'f32'}"
        coef, idx, rows = tables(cs, with_rows)
        got = run(coef, idx, fd, "gradient", rows).reshape(N, d, d, t)
        gc.assert_close(got[sample], g, mag, k + 3, f"{what} gradient of {d} components, rows {with_rows}")
        div, div_mag = gc.divergence(g, mag)
        gc.assert_close(run(coef, idx, fd, "divergence", rows)[sample, 0], div, div_mag, k + 6, f"{what} divergence, rows {with_rows}")
        vort, vort_mag = gc.vorticity(g, mag)
        got = run(coef, idx, fd, "vorticity", rows)
        gc.assert_close(got[sample, 0] if d == 2 else got[sample], vort, vort_mag, k + 6, f"{what} vorticity, rows {with_rows}")
        # the other row-list choice: one component, dense and pitched, and the component count that is not d
        coef, idx, rows = tables(cs, not with_rows)
        scalar = fd[:, 0, :].contiguous()
        for field, how in ((scalar, "dense"), (pitched(scalar), "pitched")):
            got = run(coef, idx, field, "gradient", rows).reshape(N, 1, d, t)
            gc.assert_close(got[sample], g[:, :1], mag[:, :1], k + 3, f"{what} gradient of 1 component, {how}, rows {not with_rows}")
        pick = [0, 1, 0] if d == 2 else [0, 1]
        got = run(coef, idx, fd[:, pick, :].contiguous(), "gradient", rows).reshape(N, len(pick), d, t)
        gc.assert_close(got[sample], g[:, pick], mag[:, pick], k + 3, f"{what} gradient of {len(pick)} components, rows {not with_rows}")


def test_one_dimensional_field_is_one_snapshot():
    cs = gc.case("lattice2d", 8)
    f = gc.field(N, 1, 1, True, seed=3)
    coef, idx, rows = tables(cs, True)
    g, mag = gc.apply(cs["c"].astype(np.float64), cs["idx"], f)
    gc.assert_close(run(coef, idx, dev(f.reshape(N)), "gradient", rows).reshape(N, 1, 2, 1), g, mag, 8 + 3, "field [N]")


# ---- apply: nonlinear outputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [7, 100])
@pytest.mark.parametrize("name,k", [("lattice2d", 8), ("lattice3d", 26)])
def test_nonlinear_outputs(name, k, t):
    cs = gc.case(name, k)
    d = cs["points"].shape[1]
    for f64 in (False, True):
        f = gc.field(N, d, t, f64, seed=200 * t + f64)
        g, _ = gc.apply(cs["c"].astype(np.float64), cs["idx"], f)
        coef, idx, rows = tables(cs, not f64)
        fd = dev(f)
        for mode, want in (("magnitude", gc.gradient_magnitude(g)), ("vorticity_magnitude", gc.vorticity_magnitude(g)[:, None]),
                           ("q", gc.q_criterion(g)[:, None])):
            err = gc.rel_err(run(coef, idx, fd, mode, rows), want)
            print(f"{name} T {t} {'f64' if f64 else 'f32'} {mode}: off the reference by {err:.2e} of its maximum")
            assert err <= TOL, f"{mode}: off the reference by {err:.3e} of its maximum (bound {TOL})"


# ---- exactness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("lattice2d", 8), ("lattice3d", 26), ("hostile2d", 8), ("hostile3d", 26)])
def test_constant_field_gives_exact_zeros(name, k):
    """the difference form: every output of every mode of a constant field is 0, not merely small"""
    cs = gc.case(name, k)
    n, d = cs["points"].shape
    coef, idx = dev(cs["c"].astype(np.float64)), dev(cs["idx"])
    for dtype, t in ((pt.float32, 8), (pt.float32, 7), (pt.float64, 6), (pt.float64, 3)):
        f = pt.full((n, d, t), 1.7, dtype=dtype, device="cuda")
        for mode in hipops.GRAD_MODES:
            out = run(coef, idx, f, mode)
            assert (out == 0).all(), f"{name} {dtype} T {t} {mode}: {np.count_nonzero(out)} values are not 0"


def test_two_runs_give_the_same_bits():
    cs = gc.case("lattice3d", 26)
    coef, idx, rows = tables(cs, True)
    for f64, t in ((False, 100), (True, 25)):
        f = dev(gc.field(N, 3, t, f64, seed=9))
        for mode in ("gradient", "vorticity_magnitude", "q"):
            a, b = run(coef, idx, f, mode, rows), run(coef, idx, f, mode, rows)
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), mode


@pytest.mark.parametrize("t,f64", [(7, False), (8, False), (6, True)])
def test_five_components_equal_five_single_calls(t, f64):
    """a field wider than the kernel's three components goes in groups; every component's chain is the one of a call of its own"""
    cs = gc.case("lattice2d", 8)
    coef, idx, rows = tables(cs, True)
    f = dev(gc.field(N, 5, t, f64, seed=11))
    for mode, per in (("gradient", 2), ("magnitude", 1)):
        wide = run(coef, idx, f, mode, rows).reshape(N, 5, per, t)
        for c in range(5):
            single = run(coef, idx, f[:, c, :].contiguous(), mode, rows)
            assert np.array_equal(wide[:, c].view(np.int64), single.view(np.int64)), f"{mode} component {c}"


# ---- arguments ------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise():
    cs = gc.case("hostile2d", 8)
    n = len(cs["points"])
    coef, idx, pts = dev(cs["c"].astype(np.float64)), dev(cs["idx"]), dev(cs["points"])
    f = pt.ones((n, 2, 4), dtype=pt.float32, device="cuda")
    with pytest.raises(TypeError):
        hipops.grad_apply(coef, idx.to(pt.int64), f, "gradient")
    with pytest.raises(TypeError):
        hipops.grad_apply(coef, idx, f.cpu(), "gradient")
    with pytest.raises(TypeError):
        hipops.grad_apply(coef, idx, f.to(pt.float16), "gradient")
    with pytest.raises(ValueError, match="rows"):
        hipops.grad_apply(coef, idx, f[:100], "gradient")
    with pytest.raises(ValueError, match="unknown mode"):
        hipops.grad_apply(coef, idx, f, "curl")
    for mode in ("divergence", "vorticity", "vorticity_magnitude", "q"):
        with pytest.raises(ValueError, match="vector field"):
            hipops.grad_apply(coef, idx, f[:, 0, :].contiguous(), mode)
        with pytest.raises(ValueError, match="vector field"):
            hipops.grad_apply(coef, idx, pt.ones((n, 5, 4), dtype=pt.float32, device="cuda"), mode)
    with pytest.raises(TypeError, match="out"):
        hipops.grad_apply(coef, idx, f, "gradient", out=pt.empty((n, 4, 3), dtype=pt.float64, device="cuda"))
    with pytest.raises(TypeError, match="rows"):
        hipops.grad_apply(coef, idx, f, "gradient", rows=pt.zeros(n, dtype=pt.int64, device="cuda"))
    with pytest.raises(TypeError):
        hipops.grad_apply(coef, idx, pt.ones((n, 2, 8), dtype=pt.float32, device="cuda")[:, :, :4], "gradient")
    # what only the library can refuse: k beyond S3_MAX_K, more than three components per launch, unknown dtype / mode / power
    with pytest.raises(_lib.S3HipError, match="k=65"):
        hipops.grad_apply(pt.zeros((n, 65, 2), dtype=pt.float64, device="cuda"), pt.zeros((n, 65), dtype=pt.int32, device="cuda"), f, "q")
    with pytest.raises(_lib.S3HipError, match="k=65"):
        hipops.grad_coeff(pts, pt.zeros((n, 65), dtype=pt.int32, device="cuda"))
    with pytest.raises(_lib.S3HipError, match="power=3"):
        hipops.grad_coeff(pts, idx, power=3)
    out = pt.zeros((n, 8, 4), dtype=pt.float64, device="cuda")
    lib = _lib.hip_lib()

    def raw(dim=2, dtype=0, n_comp=2, mode=0, in_stride=0):
        return lib.s3_grad_apply(C.c_void_p(coef.data_ptr()), C.c_void_p(idx.data_ptr()), n, 8, dim, C.c_void_p(f.data_ptr()), dtype, n_comp, 4,
                                 in_stride, None, mode, C.c_void_p(out.data_ptr()), 0, None)
    for kwargs, message in ((dict(n_comp=4), "n_comp=4"), (dict(dtype=7), "unknown dtype 7"), (dict(mode=9), "unknown mode 9"),
                            (dict(dim=4), "dim=4"), (dict(n_comp=1, mode=5), "n_comp == dim"), (dict(in_stride=7), "in_stride 7")):
        assert raw(**kwargs) == -1 and message in lib.s3_last_error().decode(), kwargs
    assert raw() == 0
    pt.cuda.synchronize()


# ---- the public class -----------------------------------------------------------------------------------------------------
def lstsq_gradient(cs, f):
    """f64 [N, n_comp, d, T] from numpy's least squares, zero on the planted rows"""
    n = len(cs["points"])
    ok = np.nonzero(~cs["flag"])[0]
    c = np.zeros((n,) + cs["c"].shape[1:])
    c[ok] = gc.lstsq_coefficients(cs["points"], cs["idx"], cs["power"], ok)
    df = f[cs["idx"]].astype(np.float64) - f.astype(np.float64)[:, None]
    return np.einsum("nmb,nmat->nabt", c, df)


@pytest.mark.parametrize("name", ["hostile2d", "hostile3d"])
def test_public_api_end_to_end(name, tmp_path):
    """search, drop-self, Hilbert order, coefficients and apply through ``Gradient`` on a cloud with exact copies and planted
    collinear / coplanar rows, against gradients built with ``np.linalg.lstsq``.  Bound: both sides solve the same least-squares
    problem in f64, each within (k + 16) * cond * 2**-52 <= 42 * 5 * 2.2e-16 = 5e-14 of the exact coefficients relative to the row's
    largest; the fields are O(1) differences over k terms: 1e-11 of the largest gradient leaves a factor 100 for the summation."""
    k = gc.default_neighbors(int(name[7]))
    cs = gc.case(name, k)
    n, d = cs["points"].shape
    with pytest.warns(RuntimeWarning) as record:
        grad = Gradient(cs["points"])
    ours = [str(w.message) for w in record if issubclass(w.category, RuntimeWarning) and "Gradient" in str(w.message)]
    assert len(ours) == 1 and f"{len(cs['planted'])} of {n} points" in ours[0]
    assert grad.n_points == n and grad.n_neighbors == k and grad.n_degenerate == len(cs["planted"])
    assert isinstance(grad.degenerate, np.ndarray) and np.array_equal(np.nonzero(grad.degenerate)[0], cs["planted"])
    # the device search with the drop-self rule finds the brute-force neighbours
    knn = hipops.KnnIndex(dev(cs["points"]))
    idx = drop_self(knn.query(dev(cs["points"]), k + 1)[0]).cpu().numpy()
    knn.close()
    assert np.array_equal(idx, cs["idx"])

    t = 6
    u = gc.field(n, d, t, False, seed=21)
    ref = lstsq_gradient(cs, u)
    top = np.abs(ref).max()
    got = grad.gradient(u)                                                       # host numpy in -> host numpy out
    assert isinstance(got, np.ndarray) and got.shape == (n, d, d, t) and got.dtype == np.float64
    assert np.abs(got - ref).max() <= 1e-11 * top and not got[cs["planted"]].any()
    g = got.astype(gc.LD)
    ud = dev(u)
    for fn, want in ((grad.divergence, gc.divergence(g, g)[0]), (grad.vorticity, gc.vorticity(g, g)[0]),
                     (grad.vorticity_magnitude, gc.vorticity_magnitude(g)), (grad.q_criterion, gc.q_criterion(g)),
                     (grad.magnitude, gc.gradient_magnitude(g))):
        out = fn(ud)                                                            # device in -> device out
        assert isinstance(out, pt.Tensor) and out.is_cuda and out.dtype == pt.float64 and tuple(out.shape) == want.shape
        assert gc.rel_err(out.cpu().numpy(), want) <= TOL
    # scalar fields: [N, T], a window of a resident field read where it lies, [N]; host torch in -> host torch out; ``out``
    rho = ud[:, 0, :].contiguous()
    full = grad.gradient(rho)
    assert tuple(full.shape) == (n, d, t) and np.array_equal(full.cpu().numpy(), got[:, 0])
    assert np.array_equal(grad.gradient(rho[:, 1:5]).cpu().numpy(), got[:, 0, :, 1:5])
    one = grad.magnitude(pt.from_numpy(u[:, 0, 0].copy()))
    assert isinstance(one, pt.Tensor) and not one.is_cuda and tuple(one.shape) == (n,)
    assert gc.rel_err(one.numpy(), gc.gradient_magnitude(g)[:, 0, 0]) <= TOL
    into = pt.empty((n, t), dtype=pt.float64, device="cuda")
    assert grad.q_criterion(ud, out=into) is into and np.array_equal(into.cpu().numpy(), grad.q_criterion(ud).cpu().numpy())
    host_out = np.empty((n, t))
    assert grad.divergence(u, out=host_out) is host_out and np.array_equal(host_out, grad.divergence(ud).cpu().numpy())
    for bad, err in ((lambda: grad.gradient(u[:100]), ValueError), (lambda: grad.divergence(u[:, 0]), ValueError),
                     (lambda: grad.vorticity(np.ones((n, d + 1, t))), ValueError), (lambda: grad.q_criterion(ud, out=into[:, :3]), ValueError),
                     (lambda: grad.q_criterion(ud, out=into.float()), TypeError), (lambda: grad.q_criterion(ud, out=host_out), TypeError)):
        with pytest.raises(err, match=r"\d+"):
            bad()

    # the grid of an S^3 file
    from sparsespatialsampling_amd.data import Dataloader, Datawriter
    wr = Datawriter(str(tmp_path), "g.h5")
    wr.write_data("centers", group="grid", data=cs["points"])
    loader = Dataloader(str(tmp_path), "g.h5", dtype=pt.float64)
    with pytest.warns(RuntimeWarning):
        from_file = Gradient.from_dataloader(loader)
    assert from_file.n_degenerate == len(cs["planted"])
    assert np.array_equal(from_file.gradient(u), got)


def test_a_regular_cloud_warns_of_nothing():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        grad = Gradient(dev(gc.cloud("lattice2d")[0]), n_neighbors=5, power=1)
    assert grad.n_degenerate == 0 and grad.n_neighbors == 5 and grad.degenerate.is_cuda and not grad.degenerate.any()
