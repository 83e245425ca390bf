"""The CPU reference of the DMD (tests/dmd_cases.py) against the planted dynamics, the Gram-block identities dmd.py is built on against
their direct N-sized forms, and the argument checks of ``DMD`` -- all without a GPU."""
import numpy as np
import pytest
import torch as pt

from tests import dmd_cases as dc
from sparsespatialsampling_amd import dmd

CASES = dc.NOISE_FREE


def unit_roundoff(case):
    return float(np.finfo(np.float32).eps) if case.dtype == pt.float32 else dc.EPS


def numpy_gram(built):
    """G = D^T diag(a) D of the data as the device sees it, plain float64 numpy"""
    d = built["data"].numpy().astype(np.float64)
    d = d.reshape(-1, d.shape[-1])
    sw = built["ref"]["weight_sqrt"]
    dw = d * sw[:, None]
    return d, dw, dw.T @ dw


def small_problem_of(case):
    """dmd._small_problem fed with a numpy Gram matrix and the REFERENCE's singular values / vectors of X"""
    built = case.build()
    ref = built["ref"]
    d, dw, gram = numpy_gram(built)
    _, s, vh = np.linalg.svd(dw[:, :-1], full_matrices=False)
    r = ref["rank"]
    small = dmd._small_problem(pt.from_numpy(gram), pt.from_numpy(s[:r].copy()), pt.from_numpy(vh[:r].T.copy()), case.dt, case.optimal)
    return built, d, dw, gram, small


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_reference_recovers_the_planted_dynamics(case):
    """eigenvalues, the products phi_j b_j and the data itself.  Bound: the data carry a relative rounding u of their dtype (float32
    cases) and the reference's SVD one of eps; either moves an eigenvalue of the projected operator by about kappa times as much,
    kappa = s_1 / s_r <= 100 -- 64 kappa u leaves room for the eigenvector basis.  Observed worst: 4.4e-9 (float32 cases, bound
    1.3e-5 and more), 3.0e-15 (float64 cases, bound 3.5e-14 and more)."""
    built = case.build()
    ref = built["ref"]
    order = dc.by_angle(ref["eigvals"])
    bound = 64.0 * built["kappa"] * unit_roundoff(case)
    e_lam = float(np.abs(ref["eigvals"][order] - built["lam"]).max())
    e_prod = dc.rel_max((ref["modes"] * ref["amplitude"])[:, order], built["products"])
    e_rec = dc.rel_max(ref["reconstruction"], built["truth"])
    print(f"{case.name}: kappa {built['kappa']:.2f}  e_lam {e_lam:.2e}  e_prod {e_prod:.2e}  e_rec {e_rec:.2e}  bound {bound:.2e}")
    assert ref["rank"] == case.r
    assert e_lam <= bound and e_prod <= bound and e_rec <= bound


def test_reference_rank_of_the_noisy_case():
    built = dc.NOISY.build()
    assert built["ref"]["opt_rank"] == built["ref"]["rank"] == dc.NOISY.r


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_gram_block_identities(case):
    """A~, Phi^H diag(a) Phi, the right-hand sides of both amplitude rules and the reconstruction error, each from the blocks of the
    T x T Gram matrix, against the direct form from the N-sized matrices.  Both sides are float64 sums over N rows and T columns of
    products with the factor S^-1 on each side: relative tolerance 64 eps kappa^2."""
    built, d, dw, gram, small = small_problem_of(case)
    ref = built["ref"]
    tol = 64.0 * dc.EPS * built["kappa"] ** 2
    xw, yw = dw[:, :-1], dw[:, 1:]
    order, order_ref = dc.by_angle(small["eigvals"].numpy()), dc.by_angle(ref["eigvals"])
    # A~ through its eigenvalues (the direct form is U^H Y V S^-1)
    assert np.abs(small["eigvals"].numpy()[order] - ref["eigvals"][order_ref]).max() <= tol
    b = small["b_matrix"].numpy()
    modes_w = yw.astype(np.complex128) @ b                                       # sqrt(a) Phi, direct
    direct = modes_w.conj().T @ modes_w
    assert np.abs(small["mode_gram"].numpy() - direct).max() <= tol * np.abs(direct).max()
    vm = small["vander"].numpy()[:, :-1]
    q_direct = np.diagonal(vm @ xw.T.astype(np.complex128) @ modes_w).conj()
    q_gram = np.diagonal(vm @ gram[:-1, 1:].astype(np.complex128) @ b).conj()
    assert np.abs(q_gram - q_direct).max() <= tol * np.abs(q_direct).max()
    rhs_direct = modes_w.conj().T @ dw[:, 0].astype(np.complex128)
    rhs_gram = b.conj().T @ gram[1:, 0].astype(np.complex128)
    assert np.abs(rhs_gram - rhs_direct).max() <= tol * np.abs(rhs_direct).max()
    # the products phi_j b_j of the Gram route against the reference's
    prod = ((d[:, 1:].astype(np.complex128) @ b) * small["amplitude"].numpy())[:, order]
    want = (ref["modes"] * ref["amplitude"])[:, order_ref]
    assert dc.rel_max(prod, want) <= max(tol, 16 * 64.0 * built["kappa"] * unit_roundoff(case))


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_reconstruction_error_from_the_gram_matrix(case):
    """(e_t - m_t)^T G (e_t - m_t) against the squared weighted norm of the materialised residual: within 64 T eps G_tt"""
    built, d, dw, gram, small = small_problem_of(case)
    dynamics = small["amplitude"].reshape(-1, 1) * small["vander"]
    coeff = dmd._coefficients(small["b_matrix"], dynamics)
    err, sq = dmd._error_from_gram(pt.from_numpy(gram), coeff)
    residual = dw - dw @ coeff.numpy()
    sq_direct = (residual ** 2).sum(axis=0)
    g_tt = np.diagonal(gram)
    assert (np.abs(sq.numpy() - sq_direct) <= 64.0 * case.t * dc.EPS * g_tt).all()
    assert np.allclose(err.numpy(), np.sqrt(np.maximum(sq.numpy(), 0.0) / g_tt), rtol=4 * dc.EPS, atol=0)     # (its definition)


def test_sort_eigenpairs_matches_the_reference():
    rng = np.random.default_rng(5)
    a = rng.standard_normal((8, 8))
    lam, w = np.linalg.eig(a)
    lam_r, w_r = dc.sort_eigenpairs(lam.astype(np.complex128), w.astype(np.complex128))
    lam_p, w_p = dmd.sort_eigenpairs(pt.from_numpy(lam.astype(np.complex128)), pt.from_numpy(w.astype(np.complex128)))
    assert np.array_equal(lam_p.numpy(), lam_r) and np.allclose(w_p.numpy(), w_r, rtol=0, atol=1e-15)
    assert (np.abs(lam_r)[:-1] >= np.abs(lam_r)[1:] - 1e-9).all()
    top = w_r[np.abs(w_r).argmax(axis=0), np.arange(8)]
    assert np.allclose(top.imag, 0, atol=1e-15) and (top.real > 0).all() and np.allclose(np.linalg.norm(w_r, axis=0), 1)


@pytest.mark.parametrize("kwargs,error", [
    (dict(data=pt.zeros(10, 2)), ValueError),                                   # T < 3
    (dict(data=pt.zeros(10, 5), rank=0), ValueError),
    (dict(data=pt.zeros(10, 5), dt=0.0), ValueError),
    (dict(data=pt.zeros(10, 5), dt=-1.0), ValueError),
    (dict(data=pt.zeros(10, 5), cell_area=pt.ones(9)), ValueError),
    (dict(data=pt.zeros(10, 3, 5), cell_area=pt.ones(30)), ValueError),         # one area per CELL, not per row
    (dict(data=pt.zeros(10, 5, dtype=pt.int32)), TypeError),
    (dict(data=pt.zeros(10, 5, dtype=pt.float16)), TypeError),
    (dict(data=pt.zeros(10, 10)[:, ::2]), ValueError),                          # inner stride 2
    (dict(data=pt.zeros(5, 10).T), ValueError),
    (dict(data=pt.zeros(10, 3, 8)[:, :, :5]), ValueError),                      # pitched vector field
    (dict(data=pt.zeros(10)), ValueError),
    (dict(data=np.zeros((10, 5))), TypeError),
])
def test_argument_errors_are_raised_before_any_device_call(kwargs, error, monkeypatch):
    from sparsespatialsampling_amd import hipops

    def no_device(*a, **k):
        raise AssertionError("a device call was made before the arguments were checked")
    monkeypatch.setattr(hipops, "device", no_device)
    monkeypatch.setattr(hipops, "to_device", no_device)
    kwargs = dict(kwargs)
    data = kwargs.pop("data")
    kwargs.setdefault("dt", 0.1)
    with pytest.raises(error):
        dmd.DMD(data, **kwargs)


def test_package_exports():
    import sparsespatialsampling_amd
    from sparsespatialsampling_amd import utils
    assert sparsespatialsampling_amd.DMD is dmd.DMD is utils.DMD and "DMD" in sparsespatialsampling_amd.__all__
