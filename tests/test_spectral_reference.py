"""Welch spectra and SPOD without a GPU: the long-double references of tests/spectral_cases.py against scipy's recorded output, the
checker itself (a float64 emulation of the kernel stays within every bound, every planted mistake leaves it), the host parts of
sparsespatialsampling_amd/spectral.py (segment_matrix, the small SPOD problem from Gram blocks alone) and the argument errors."""
import os

import numpy as np
import pytest
import torch as pt

from sparsespatialsampling_amd import _lib, spectral
from tests import centered_cases as cc
from tests import spectral_cases as sc

LD = np.longdouble
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "welch_scipy.npz")


# ---- the references against scipy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(sc.SCIPY_CASES)))
def test_long_double_reference_equals_scipy(i):
    """tolerance: 4 x scipy's own deviation from long double, measured by tests/golden/gen_welch_scipy.py and stored in the fixture,
    relative to the row's largest PSD value"""
    g = np.load(GOLDEN)
    n, t, nperseg, noverlap, win, detrend = sc.SCIPY_CASES[i]
    x = g[f"x{i}"]
    assert x.shape == (n, t) and np.array_equal(x, sc.scipy_case_data(i))
    freq, ref = sc.welch_reference(x, float(g["dt"]), nperseg, noverlap, win, detrend)
    assert np.allclose(freq, g[f"freq{i}"], rtol=1e-14, atol=0)
    dev = np.abs(g[f"psd{i}"] - ref).max(1) / np.abs(ref).max(1)
    print(f"case {i}: deviation {float(dev.max()):.2e}, tolerance {float(g[f'tol{i}']):.2e}")
    assert float(g[f"tol{i}"]) < 1e-12 and np.all(dev <= float(g[f"tol{i}"]))


@pytest.mark.parametrize("i", range(len(sc.SCIPY_CASES)))
def test_folded_matrix_gives_the_reference(i):
    """the route the kernel takes -- row mean subtracted, segment mean folded into B -- gives welch_reference within the bounds"""
    g = np.load(GOLDEN)
    n, t, nperseg, noverlap, win, detrend = sc.SCIPY_CASES[i]
    x, dt = g[f"x{i}"], float(g["dt"])
    hop, n_blk = sc.segments(t, nperseg, noverlap)
    bre, bim, w = spectral.segment_matrix(nperseg, win, detrend)
    k = np.arange(nperseg // 2 + 1)
    scale = spectral.psd_scale(w, dt, n_blk, k, nperseg, "density")
    mean = cc.row_means(x) if detrend == "constant" else None
    re, im, mre, mim = sc.coef_reference(x, mean, bre, bim, nperseg, hop, n_blk)
    _, ref = sc.welch_reference(x, dt, nperseg, noverlap, win, detrend)
    e0 = sc.reference_error(x, w, nperseg)
    bound = sc.psd_bound(re, im, sc.coef_bound(nperseg, mre, 1) + e0, sc.coef_bound(nperseg, mim, 1) + e0, scale, 1)
    _, psd = sc.emulated(x, mean, bre, bim, nperseg, hop, n_blk, scale)
    r = sc.ratio(psd, ref, bound)
    print(f"case {i}: emulated welch at {r:.3f} of the bound")
    assert r <= 1.0


# ---- the checker --------------------------------------------------------------------------------------------------------------------
def checker_case(folded):
    """pressure-like rows (mean 1e5, fluctuation 1e-2), T = 75 leaves a remainder of 3 at L = 16, hop = 8; even L: Nyquist present"""
    n, t, nperseg, noverlap, dt = 6, 75, 16, 8, 0.01
    x = cc.rows(n, t, np.float64, 3)
    hop, n_blk = sc.segments(t, nperseg, noverlap)
    w = sc.window("hann", nperseg)
    bre, bim = sc.dft_matrix(nperseg, w, folded)
    k = np.arange(nperseg // 2 + 1)
    return x, cc.row_means(x), bre, bim, nperseg, hop, n_blk, w, dt, k


@pytest.mark.parametrize("folded", [False, True])
def test_emulation_within_bounds(folded):
    x, mean, bre, bim, nperseg, hop, n_blk, w, dt, k = checker_case(folded)
    scale = sc.scale_vector(w, dt, n_blk, k, nperseg)
    re, im, mre, mim = sc.coef_reference(x, mean, bre, bim, nperseg, hop, n_blk)
    e_re, e_im = sc.coef_bound(nperseg, mre), sc.coef_bound(nperseg, mim)
    coef, psd = sc.emulated(x, mean, bre, bim, nperseg, hop, n_blk, scale)
    r_c = max(sc.ratio(coef[..., 0], re, e_re), sc.ratio(coef[..., 1], im, e_im))
    r_p = sc.ratio(psd, sc.psd_reference(re, im, scale), sc.psd_bound(re, im, e_re, e_im, scale))
    print(f"folded {folded}: coefficients at {r_c:.3f}, PSD at {r_p:.3f} of their bounds")
    assert r_c <= 1.0 and r_p <= 1.0


@pytest.mark.parametrize("mistake", ["mean_f32", "start_bL", "trailing", "no_doubling", "nyquist_doubled"])
def test_planted_mistakes_leave_the_bounds(mistake):
    """(the mean rounded to float32 shows where B is not folded: a folded column sums to zero and hides a constant offset)"""
    x, mean, bre, bim, nperseg, hop, n_blk, w, dt, k = checker_case(folded=False)
    scale = sc.scale_vector(w, dt, n_blk, k, nperseg)
    re, im, mre, mim = sc.coef_reference(x, mean, bre, bim, nperseg, hop, n_blk)
    e_re, e_im = sc.coef_bound(nperseg, mre), sc.coef_bound(nperseg, mim)
    wrong_scale = sc.scale_vector(w, dt, n_blk, k, nperseg, mistake=mistake)
    coef, psd = sc.emulated(x, mean, bre, bim, nperseg, hop, n_blk, wrong_scale, mistake)
    r_p = sc.ratio(psd, sc.psd_reference(re, im, scale), sc.psd_bound(re, im, e_re, e_im, scale))
    print(f"{mistake}: PSD at {r_p:.3g} of its bound")
    assert r_p > 1.0
    if mistake in ("mean_f32", "start_bL"):
        r_c = max(sc.ratio(coef[..., 0], re, e_re), sc.ratio(coef[..., 1], im, e_im))
        print(f"{mistake}: coefficients at {r_c:.3g} of their bound")
        assert r_c > 1.0


def test_folding_alone_loses_the_mean():
    """pressure rows, L = 64: without the row mean in the staging the product cancels 1e5 against 1e-2 and misses the bound computed
    on x - mean by orders of magnitude -- why welch hands the kernel d_mean"""
    n, t, nperseg, dt = 3, 64, 64, 0.01
    x = cc.rows(n, t, np.float64, 5)
    w = sc.window("hann", nperseg)
    bre, bim = sc.dft_matrix(nperseg, w, True)
    k = np.arange(nperseg // 2 + 1)
    scale = sc.scale_vector(w, dt, 1, k, nperseg)
    mean = cc.row_means(x)
    re, im, mre, mim = sc.coef_reference(x, mean, bre, bim, nperseg, nperseg, 1)
    bound = sc.psd_bound(re, im, sc.coef_bound(nperseg, mre), sc.coef_bound(nperseg, mim), scale)
    ref = sc.psd_reference(re, im, scale)
    _, with_mean = sc.emulated(x, mean, bre, bim, nperseg, nperseg, 1, scale)
    _, folded_only = sc.emulated(x, None, bre, bim, nperseg, nperseg, 1, scale)
    r_ok, r_bad = sc.ratio(with_mean[:, 1:], ref[:, 1:], bound[:, 1:]), sc.ratio(folded_only[:, 1:], ref[:, 1:], bound[:, 1:])
    print(f"with the row mean {r_ok:.3f}, folding alone {r_bad:.3g} of the bound")
    assert r_ok <= 1.0 and r_bad > 100.0


# ---- host parts of the product ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nperseg,win", [(4, "hann"), (7, "hamming"), (16, "boxcar"), (33, "hann"), (130, "hamming"), (1, "hann")])
@pytest.mark.parametrize("detrend", ["constant", False])
def test_segment_matrix(nperseg, win, detrend):
    bre, bim, w = spectral.segment_matrix(nperseg, win, detrend)
    assert bre.dtype == bim.dtype == w.dtype == np.float64 and bre.shape == bim.shape == (nperseg, nperseg // 2 + 1)
    assert bre.flags.c_contiguous and bim.flags.c_contiguous
    assert np.array_equal(w, sc.window(win, nperseg))
    ref_re, ref_im = sc.dft_matrix(nperseg, w, detrend == "constant")
    assert np.array_equal(bre, ref_re) and np.array_equal(bim, ref_im)
    if detrend == "constant":                                                # a folded column removes any constant
        assert np.abs(bre.sum(0)).max() <= 4 * nperseg * sc.U and np.abs(bim.sum(0)).max() <= 4 * nperseg * sc.U
    subset = np.array([nperseg // 2, 0]) if nperseg > 1 else np.array([0])
    sre, sim, _ = spectral.segment_matrix(nperseg, win, detrend, subset)
    assert np.array_equal(sre, bre[:, subset]) and np.array_equal(sim, bim[:, subset])
    w_arr = np.linspace(0.5, 1.5, nperseg)
    are, _, wa = spectral.segment_matrix(nperseg, w_arr, False)
    assert np.array_equal(wa, w_arr) and np.array_equal(are[:, 0], w_arr)


def test_windows_are_scipys():
    scipy_signal = pytest.importorskip("scipy.signal")
    for name in spectral.WINDOWS:
        for nperseg in (1, 2, 4, 7, 64, 130):
            assert np.abs(spectral._window(name, nperseg) - scipy_signal.get_window(name, nperseg)).max() <= 8 * sc.U


def test_scale_and_one_sided_factor():
    assert list(spectral.one_sided_factor(np.arange(5), 8)) == [1, 2, 2, 2, 1] and list(spectral.one_sided_factor(np.arange(4), 7)) == [1, 2, 2, 2]
    w = sc.window("hann", 8)
    for scaling in ("density", "spectrum"):
        assert np.array_equal(spectral.psd_scale(w, 0.01, 3, np.arange(5), 8, scaling), sc.scale_vector(w, 0.01, 3, np.arange(5), 8, scaling))


def spod_gram_blocks(x, area, c):
    """the real [2 n_blk, 2 n_blk] weighted Gram matrix of every frequency's coefficients (what s3_gram returns), in float64 numpy"""
    k = np.arange(c["nperseg"] // 2 + 1)
    re, im = sc.segment_coefficients(x, c["nperseg"], c["noverlap"], sc.window(c["window"], c["nperseg"]), c["detrend"], k)
    real = sc.interleave(re, im).astype(np.float64).reshape(re.shape[0], len(k), -1)        # [N, n_f, 2 n_blk]
    return np.einsum("i,ifb,ifc->fbc", area, real, real), re, im


def test_spod_small_problem_equals_direct_spod():
    c = sc.SPOD_CASE
    x, area, shapes = sc.spod_case()
    lam_ref, modes_ref = sc.spod_reference(x, c["dt"], c["nperseg"], c["noverlap"], c["window"], area, c["detrend"])
    grams, re, im = spod_gram_blocks(x, area, c)
    n_blk = re.shape[2]
    w = sc.window(c["window"], c["nperseg"])
    kappa = c["dt"] / ((w ** 2).sum() * n_blk)
    lam, theta = spectral._spod_small(pt.from_numpy(grams), kappa)
    k = np.arange(c["nperseg"] // 2 + 1)
    lam1 = lam.numpy() * spectral.one_sided_factor(k, c["nperseg"])[:, None]
    assert np.abs(lam1 - lam_ref).max() <= 1e-12 * lam_ref.max()
    # the trace identity: sum_k eigvals[f, k] = sum_i a_i psd_i(f) of welch with the same arguments
    _, psd = sc.welch_reference(x, c["dt"], c["nperseg"], c["noverlap"], c["window"], c["detrend"])
    weighted = (area.astype(LD)[:, None] * psd).sum(0)
    assert np.abs(lam1.sum(1) - weighted).max() <= 1e-13 * float(weighted.max())
    q = (re + 1j * im).astype(np.complex128)
    for j, kbin in enumerate(c["bins"]):
        gap = lam_ref[kbin, 0] / lam_ref[kbin, 1]
        print(f"bin {kbin}: lambda_1 / lambda_2 = {gap:.3g}")
        assert gap >= 1e3                                                    # the mode comparison is well posed
        rhs = spectral._mode_rhs(theta[kbin][:, :2], lam[kbin, :2], kappa).numpy()
        real = sc.interleave(re[:, kbin], im[:, kbin]).astype(np.float64).reshape(len(area), -1)
        phi = (real @ rhs).reshape(len(area), 2, 2)
        phi = phi[..., 0] + 1j * phi[..., 1]
        direct = np.sqrt(kappa) * (q[:, kbin, :] @ theta[kbin].numpy()[:, :2]) / np.sqrt(lam[kbin, :2].numpy())
        assert np.abs(phi - direct).max() <= 1e-12 * np.abs(direct).max()    # the real embedding is the complex product
        ortho = (phi.conj().T * area) @ phi
        assert np.abs(ortho - np.eye(2)).max() <= 1e-10
        for other in (phi[:, 0], modes_ref[kbin][:, 0]):
            align = abs((shapes[:, j].conj() * area * other).sum())
            print(f"bin {kbin}: alignment with the planted shape {align:.6f}")
            assert align > 0.9999
        assert abs((modes_ref[kbin][:, 0].conj() * area * phi[:, 0]).sum()) > 1 - 1e-10


def test_spod_perturbation_bound_covers_float64_coefficients():
    """the Weyl bound of spectral_cases: eigenvalues from float64-rounded coefficients stay within it"""
    c = sc.SPOD_CASE
    x, area, _ = sc.spod_case()
    hop, n_blk = sc.segments(c["t"], c["nperseg"], c["noverlap"])
    bre, bim, w = spectral.segment_matrix(c["nperseg"], c["window"], None)
    mean = cc.row_means(x)
    re, im, mre, mim = sc.coef_reference(x, mean, bre, bim, c["nperseg"], hop, n_blk)
    kappa = c["dt"] / ((w ** 2).sum() * n_blk)
    weyl = sc.spod_perturbation(re, im, sc.coef_bound(c["nperseg"], mre), sc.coef_bound(c["nperseg"], mim), area, kappa)
    real = sc.interleave(re, im).astype(np.float64).reshape(len(area), re.shape[1], -1)
    lam, _ = spectral._spod_small(pt.from_numpy(np.einsum("i,ifb,ifc->fbc", area, real, real)), kappa)
    q = re + 1j * im.astype(np.complex128)
    exact = np.stack([np.linalg.eigvalsh(kappa * ((q[:, f].conj().T * area) @ q[:, f]).astype(np.complex128))[::-1] for f in range(re.shape[1])])
    r = float((np.abs(lam.numpy() - exact) / np.asarray(weyl, dtype=np.float64)[:, None]).max())
    print(f"eigenvalues at {r:.3f} of the Weyl bound")
    assert r <= 1.0 and float(weyl.max()) < 1e-9 * exact.max()


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def test_exported_lazily():
    import sparsespatialsampling_amd as pkg
    assert pkg.welch is spectral.welch and pkg.SPOD is spectral.SPOD and "welch" in pkg.__all__ and "SPOD" in pkg.__all__


@pytest.mark.parametrize("kwargs,match", [
    (dict(nperseg=0), "nperseg"), (dict(nperseg=41), "nperseg"), (dict(nperseg=8, noverlap=8), "noverlap"), (dict(nperseg=8, noverlap=-1), "noverlap"),
    (dict(window="kaiser"), "window"), (dict(nperseg=8, window=np.ones(7)), "window"), (dict(detrend="linear"), "detrend"),
    (dict(scaling="power"), "scaling"), (dict(nperseg=8, frequencies=[5]), "frequencies"), (dict(nperseg=8, frequencies=[]), "frequencies"),
    (dict(nperseg=8, frequencies=[0.5]), "frequencies")])
def test_welch_argument_errors_need_no_device(kwargs, match):
    with pytest.raises(ValueError, match=match):
        spectral.welch(pt.zeros((4, 40)), 0.1, **kwargs)


def test_data_argument_errors_are_the_dmds():
    for call in (lambda d, dt, **kw: spectral.welch(d, dt, **kw), lambda d, dt, **kw: spectral.SPOD(d, dt, 8, **kw)):
        with pytest.raises(TypeError):
            call(np.zeros((4, 40)), 0.1)
        with pytest.raises(TypeError):
            call(pt.zeros((4, 40), dtype=pt.float16), 0.1)
        with pytest.raises(ValueError, match="expected"):
            call(pt.zeros(40), 0.1)
        with pytest.raises(ValueError, match="dt"):
            call(pt.zeros((4, 40)), 0.0)
        with pytest.raises(ValueError, match="inner stride"):
            call(pt.zeros((4, 80))[:, ::2], 0.1)
        with pytest.raises(ValueError, match="contiguous"):
            call(pt.zeros((4, 2, 80))[:, :, :40], 0.1)
    with pytest.raises(ValueError, match="cell_area"):
        spectral.SPOD(pt.zeros((4, 40)), 0.1, 8, cell_area=pt.ones(5))
    with pytest.raises(ValueError, match="detrend"):
        spectral.SPOD(pt.zeros((4, 40)), 0.1, 8, detrend="linear")
    with pytest.raises(ValueError, match="nperseg"):
        spectral.SPOD(pt.zeros((4, 40)), 0.1, 64)


def test_no_device_no_result():
    if pt.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.HipUnavailableError):
        spectral.welch(pt.zeros((4, 40)), 0.1, nperseg=8)
    with pytest.raises(_lib.HipUnavailableError):
        spectral.SPOD(pt.zeros((4, 40)), 0.1, 8)
