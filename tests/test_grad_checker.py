"""
The reference of the least-squares derivatives and its judge (tests/grad_cases.py), checked on the CPU: the long-double
coefficients against ``np.linalg.lstsq``, the identity a least-squares gradient fulfils, the definition evaluated in plain f64 (what a
device does) against the bounds the GPU tests use, and the per-element judge against planted faults.  Plus the argument checks of
``differential.Gradient`` that need no device.

Bounds.  Coefficients and identity: ``(k + 16) * cond * 2**-52`` -- k summed products, a d x d Cholesky factorisation and its
two solves, amplified by the condition of M.  The plain-f64 evaluation sits a factor 6 or more below it on every cloud (printed).
"""
import numpy as np
import pytest

from tests import grad_cases as gc


@pytest.mark.parametrize("name,k", gc.CASES)
def test_reference_agrees_with_lstsq(name, k):
    """the normal-equation route of the definition and numpy's SVD-based least squares give the same coefficients: both are within
    cond * eps of the exact ones in f64 terms, the reference far closer"""
    cs = gc.case(name, k)
    rows = np.nonzero(~cs["flag"])[0][::7]
    ref = gc.lstsq_coefficients(cs["points"], cs["idx"], cs["power"], rows)
    top = np.abs(ref).max(axis=(1, 2))
    err = np.abs(ref - cs["c"][rows].astype(np.float64)).max(axis=(1, 2)) / top
    bound = (k + 16) * cs["cond"][rows] * 2.0 ** -52
    print(f"{name} k {k}: lstsq within {float((err / bound).max()):.3g} of the bound")
    assert (err <= bound).all()


@pytest.mark.parametrize("power", [0, 1, 2])
def test_reference_powers_agree_with_lstsq(power):
    cs = gc.case("lattice3d", 7, power)
    rows = np.arange(0, gc.N_POINTS, 31)
    ref = gc.lstsq_coefficients(cs["points"], cs["idx"], power, rows)
    err = np.abs(ref - cs["c"][rows].astype(np.float64)).max(axis=(1, 2)) / np.abs(ref).max(axis=(1, 2))
    assert (err <= (7 + 16) * cs["cond"][rows] * 2.0 ** -52).all()


@pytest.mark.parametrize("name,k", gc.CASES)
def test_plain_f64_meets_the_device_bounds(name, k):
    """the definition in plain f64: flags equal, coefficients per row within the bound of the row's largest, identity within it"""
    cs = gc.case(name, k)
    c64, flag64, _, _ = gc.coefficients(cs["points"], cs["idx"], cs["power"], dtype=np.float64)
    ok = ~cs["flag"]
    assert np.array_equal(flag64, cs["flag"]) and not c64[cs["flag"]].any() and not cs["c"][cs["flag"]].any()
    bound = (k + 16) * cs["cond"][ok] * 2.0 ** -52
    dev = (np.abs(c64.astype(gc.LD) - cs["c"])[ok].max(axis=(1, 2)) / np.abs(cs["c"][ok]).max(axis=(1, 2))).astype(np.float64)
    ident = gc.identity_error(c64, cs["points"], cs["idx"])[ok]
    print(f"{name} k {k}: cond <= {cs['cond'][ok].max():.3g}, pivot ratio >= {cs['ratio'][ok].min():.3g}, coefficients at "
          f"{(dev / bound).max():.3g} of the bound, identity at {(ident / bound).max():.3g}")
    assert (dev <= bound).all() and (ident <= bound).all()


def test_hostile_clouds_flag_exactly_the_planted_rows():
    for name, k, n_planted in (("hostile2d", 8, 12), ("hostile3d", 26, 36)):
        cs = gc.case(name, k)
        assert int(cs["flag"].sum()) == n_planted == len(cs["planted"])
        assert (cs["ratio"][cs["flag"]] == 0).all() and cs["ratio"][~cs["flag"]].min() >= 0.1
    # the exact copies are each other's first neighbour, at distance 0 and with weight 0; the copy finds ITSELF second
    cs = gc.case("hostile2d", 8)
    assert np.array_equal(cs["idx"][600:620, 0], np.arange(10, 30)) and np.array_equal(cs["idx"][10:30, 0], np.arange(600, 620))
    assert not cs["c"][600:620, 0].any() and not cs["flag"][600:620].any()


def test_drop_self_when_copies_crowd_the_point_out():
    """more than k coincident copies: the point is not among its own k + 1 nearest (the lowest indices win) -> the last goes"""
    x = np.concatenate([np.zeros((6, 2)), np.random.default_rng(0).random((10, 2)) + 1.0])
    idx = gc.neighbours(x, 3)
    assert np.array_equal(idx[5], [0, 1, 2]) and np.array_equal(idx[1], [0, 2, 3]) and (idx != np.arange(16)[:, None]).all()
    c, flag, _, ratio = gc.coefficients(x, idx)
    assert flag[:6].all() and not c[:6].any() and (ratio[:6] == 0).all()          # h = 0


# ---- the judge --------------------------------------------------------------------------------------------------------------
def _f64_apply(c, idx, f, order=None, skip=None, f32=False, no_centre=False):
    """G[i, a, b, t] as a device forms it: a chain over the neighbours in ``order``, in f64 (or f32)"""
    acc_t = np.float32 if f32 else np.float64
    n, k, d = c.shape
    order = range(k) if order is None else order
    g = np.zeros((n, f.shape[1], d, f.shape[2]), dtype=acc_t)
    with np.errstate(invalid="ignore"):
        for m in order:
            if m == skip:
                continue
            df = f[idx[:, m]].astype(np.float64) - (0.0 if no_centre else f.astype(np.float64))
            g += (c[:, m, None, :, None].astype(acc_t) * df[:, :, None, :].astype(acc_t)).astype(acc_t)
    return g.astype(np.float64)


@pytest.mark.parametrize("f64", [False, True])
def test_judge_rejects_planted_faults_and_accepts_a_reordered_sum(f64):
    cs = gc.case("lattice3d", 26)
    rows = np.arange(0, 400)
    k, t = 26, 7
    f = gc.field(gc.N_POINTS, 3, t, f64, seed=5)
    c64 = cs["c"].astype(np.float64)
    ref, mag = gc.apply(c64, cs["idx"], f, rows)
    sub = lambda g: g[rows]                                                     # noqa: E731
    good = _f64_apply(c64, cs["idx"], f)
    assert not gc.violations(sub(good), ref, mag, k + 3).any()
    assert not gc.violations(sub(_f64_apply(c64, cs["idx"], f, order=np.random.default_rng(1).permutation(k))), ref, mag, k + 3).any()
    faults = {
        "a skipped neighbour": sub(_f64_apply(c64, cs["idx"], f, skip=k - 1)),
        "f32 accumulation": sub(_f64_apply(c64, cs["idx"], f, f32=True)),
        "a swapped axis": sub(good)[:, :, [1, 0, 2]],
        "a wrong column": np.roll(sub(good), 1, axis=3),
        "a missing centre subtraction": sub(_f64_apply(c64, cs["idx"], f, no_centre=True)),
    }
    for what, got in faults.items():
        share = gc.violations(got, ref, mag, k + 3).mean()
        print(f"{what}: {share:.1%} of the elements rejected")
        assert share > 0.5, what
    # the derived linear quantities are judged with the summed magnitudes of their entries
    div, div_mag = gc.divergence(ref, mag)
    vort, vort_mag = gc.vorticity(ref, mag)
    g = sub(good)
    assert not gc.violations(g[:, 0, 0] + g[:, 1, 1] + g[:, 2, 2], div, div_mag, k + 6).any()
    got_vort = np.stack([g[:, 2, 1] - g[:, 1, 2], g[:, 0, 2] - g[:, 2, 0], g[:, 1, 0] - g[:, 0, 1]], axis=1)
    assert not gc.violations(got_vort, vort, vort_mag, k + 6).any()
    assert gc.violations(-got_vort, vort, vort_mag, k + 6).mean() > 0.9
    # nonlinear ones: the plain f64 evaluation meets the 1e-12 (of the output's largest value) the GPU tests ask for
    for name, got, want in (("Q", -0.5 * np.einsum("nabt,nbat->nt", g, g), gc.q_criterion(ref)),
                            ("vorticity magnitude", np.sqrt((got_vort ** 2).sum(axis=1)), gc.vorticity_magnitude(ref)),
                            ("magnitude", np.sqrt((g ** 2).sum(axis=2)), gc.gradient_magnitude(ref))):
        err = gc.rel_err(got, want)
        print(f"{name}: plain f64 off the reference by {err:.2e} of its maximum")
        assert err <= 1e-12


def test_judge_follows_nan_and_inf_classes():
    cs = gc.case("lattice2d", 8)
    f = gc.field(gc.N_POINTS, 1, 3, False, seed=6)
    f[100, 0, 0], f[200, 0, 1], f[300, 0, 2] = np.nan, np.inf, -np.inf
    c64 = cs["c"].astype(np.float64)
    ref, mag = gc.apply(c64, cs["idx"], f)
    got = _f64_apply(c64, cs["idx"], f)
    assert np.isnan(ref[100, 0, :, 0].astype(np.float64)).all() and not np.isfinite(ref[:, 0, :, 1].astype(np.float64)).all()
    assert not gc.violations(got, ref, mag, 8 + 3).any()
    assert gc.violations(np.nan_to_num(got, nan=0.0, posinf=1e300, neginf=-1e300), ref, mag, 8 + 3).any()


# ---- the public class without a device ---------------------------------------------------------------------------------------
def test_default_neighbour_counts_and_argument_checks():
    from sparsespatialsampling_amd import differential as df
    assert df._default(2, 1000, None) == 8 and df._default(3, 1000, None) == 26
    assert df._default(2, 5, None) == 4 and df._default(3, 1000, 500) == 63 and df._default(3, 4, None) == 3
    with pytest.raises(ValueError, match="at least 3 points"):
        df._default(2, 2, None)
    with pytest.raises(ValueError, match="at least 4 points"):
        df._default(3, 3, 5)
    with pytest.raises(ValueError, match="positive"):
        df._default(2, 100, 0)
    with pytest.raises(ValueError, match=r"\(10, 4\)"):
        df.Gradient(np.zeros((10, 4)))
    with pytest.raises(ValueError, match=r"\(10,\)"):
        df.Gradient(np.zeros(10))
    with pytest.raises(ValueError, match="power"):
        df.Gradient(np.zeros((10, 2)), power=3)
    with pytest.raises(ValueError, match="at least 3 points"):
        df.Gradient(np.zeros((2, 2)))
    with pytest.raises(TypeError):
        df.Gradient([[0.0, 1.0]] * 5)
    import sparsespatialsampling_amd as pkg
    assert pkg.Gradient is df.Gradient and "Gradient" in pkg.__all__
