"""The segment DFT kernel (s3_segment_dft / s3_segment_psd: csrc/spectral.hip) and ``welch`` / ``SPOD`` built on it
(sparsespatialsampling_amd/spectral.py) on the GPU: coefficients and PSD per element against long double within the bounds of
tests/spectral_cases.py, bit parity between float32 input and its float64 copy in every row layout and between two runs, canaries in the
pitch gaps, in the dropped trailing samples and around both outputs, ``welch`` against scipy's recorded output, SPOD against the direct
CPU reference within the Weyl and Davis-Kahan bounds."""
import os

import numpy as np
import pytest
import torch as pt

from tests import centered_cases as cc
from tests import dmd_cases as dc
from tests import spectral_cases as sc

pytestmark = pytest.mark.gpu

LD = np.longdouble
LAYOUTS = ["contiguous", "pitch16", "odd"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "welch_scipy.npz")

# (n_rows, T, L, hop, folded): row-tile tails 1 / 15 / 17 / 129 / 257; k-step tails L = 4, 7, 17; even and odd L (Nyquist present / absent);
# L = 130: three column blocks of 32 frequencies; hop 1 / 2 / 3 / L // 2 / L (float32 load widths 1, 2, 1, 4 or 1, 4 or 1); one segment
# (L = T) up to 194; every T but those at hop 1 and L = T leaves a dropped remainder
KERNEL_CASES = [(1, 4, 4, 4, False), (15, 41, 7, 3, True), (17, 70, 16, 8, True), (129, 60, 17, 17, False), (257, 140, 33, 16, True),
                (17, 257, 64, 1, False), (15, 300, 130, 65, True), (129, 130, 130, 130, True), (257, 51, 4, 2, False), (17, 100, 64, 32, True)]


@pytest.fixture(scope="module")
def ops():
    from sparsespatialsampling_amd import hipops
    hipops.device()
    return hipops


def device_matrix(dense, layout, offset=0):
    """device tensor with the values of the host matrix ``dense`` in the row layout ``layout``, ``offset`` elements into its buffer; the
    pitch gaps hold NaN"""
    n, t = dense.shape
    stride = dc.layout_stride(t, layout, dense.element_size())
    buf = pt.full((n * stride + offset,), float("nan"), dtype=dense.dtype)
    buf[offset:].reshape(n, stride)[:, :t].copy_(dense)
    return buf.cuda()[offset:].reshape(n, stride)[:, :t]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(pt.equal(a.cpu().contiguous().view(pt.int64), b.cpu().contiguous().view(pt.int64)))


_KERNEL_INPUT = {}


def kernel_input(case):
    """float32 data (dropped trailing samples NaN), the operands handed to the kernel and the long-double references, once per case"""
    if case not in _KERNEL_INPUT:
        from sparsespatialsampling_amd import spectral
        n, t, nperseg, hop, folded = case
        n_blk = (t - nperseg) // hop + 1
        used = (n_blk - 1) * hop + nperseg
        x = cc.rows(n, t, np.float32, 11 * n + t) if folded else (np.random.default_rng(n + t).standard_normal((n, t)) + 0.5).astype(np.float32)
        mean = x[:, :used].astype(np.float64).mean(1)
        x[:, used:] = np.nan
        bre, bim, w = spectral.segment_matrix(nperseg, "hann", "constant" if folded else None)
        scale = sc.scale_vector(w, 0.01, n_blk, np.arange(nperseg // 2 + 1), nperseg)
        re, im, mre, mim = sc.coef_reference(x[:, :used], mean, bre, bim, nperseg, hop, n_blk)
        e_re, e_im = sc.coef_bound(nperseg, mre), sc.coef_bound(nperseg, mim)
        _KERNEL_INPUT[case] = dict(x=pt.from_numpy(x), mean=mean, bre=bre, bim=bim, scale=scale, n_blk=n_blk, re=re, im=im, e_re=e_re, e_im=e_im,
                                   psd=sc.psd_reference(re, im, scale), psd_bound=sc.psd_bound(re, im, e_re, e_im, scale))
    return _KERNEL_INPUT[case]


def launch(ops, xd, k, case, mode):
    n, t, nperseg, hop, _ = case
    args = (xd, ops.to_device(k["mean"]), nperseg, hop, k["n_blk"], ops.to_device(k["bre"]), ops.to_device(k["bim"]))
    return ops.segment_dft(*args) if mode == 0 else ops.segment_psd(*args, ops.to_device(k["scale"]))


@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "n{}_t{}_L{}_hop{}_{}".format(*c))
def test_kernel_per_element_parity_and_canaries(ops, case):
    k = kernel_input(case)
    n_blk = k["n_blk"]
    base = {}
    for mode in (0, 1):
        base[mode] = launch(ops, device_matrix(k["x"], "contiguous"), k, case, mode)
        assert same_bits(base[mode], launch(ops, device_matrix(k["x"], "contiguous"), k, case, mode))            # a second run
    coef, psd = base[0].cpu().numpy(), base[1].cpu().numpy()
    assert coef.shape == k["re"].shape + (2,) and psd.shape == k["psd"].shape
    r_c = max(sc.ratio(coef[..., 0], k["re"], k["e_re"]), sc.ratio(coef[..., 1], k["im"], k["e_im"]))
    r_p = sc.ratio(psd, k["psd"], k["psd_bound"])
    # MODE 1 against the PSD formed from MODE 0's own coefficients: the roundings of the power alone
    own = sc.psd_reference(coef[..., 0].astype(LD), coef[..., 1].astype(LD), k["scale"])
    r_o = sc.ratio(psd, own, LD(n_blk + 3) * LD(sc.U) * np.abs(own))
    print(f"{case}: coefficients at {r_c:.3f}, PSD at {r_p:.3f}, PSD of MODE 0's coefficients at {r_o:.3f} of their bounds")
    assert r_c <= 1.0 and r_p <= 1.0 and r_o <= 1.0
    # float32 and its float64 copy, every layout, buffer offsets 0 and 1: the same bits (NaN in the gaps and in the trailing samples)
    for layout in LAYOUTS:
        for offset in (0, 1):
            for x in (k["x"], k["x"].double()):
                for mode in (0, 1):
                    got = launch(ops, device_matrix(x, layout, offset), k, case, mode)
                    assert same_bits(got, base[mode]), (layout, offset, x.dtype, mode)


@pytest.mark.parametrize("case", [KERNEL_CASES[1], KERNEL_CASES[4], KERNEL_CASES[6]], ids=lambda c: "n{}_t{}_L{}_hop{}_{}".format(*c))
def test_kernel_leaves_the_bytes_around_its_outputs_alone(ops, case):
    k = kernel_input(case)
    n, n_f, n_blk = case[0], k["bre"].shape[1], k["n_blk"]
    xd = device_matrix(k["x"], "odd", 1)
    guard = 512
    mean, bre, bim, scale = (ops.to_device(k[name]) for name in ("mean", "bre", "bim", "scale"))
    for shape in ((n, n_f, n_blk, 2), (n, n_f)):
        size = int(np.prod(shape))
        buf = pt.full((guard + size + guard,), float("nan"), dtype=pt.float64, device="cuda")
        out = buf[guard:guard + size].view(shape)
        if len(shape) == 4:
            got, ref = ops.segment_dft(xd, mean, case[2], case[3], n_blk, bre, bim, out=out), ops.segment_dft(xd, mean, case[2], case[3], n_blk, bre, bim)
        else:
            got, ref = (ops.segment_psd(xd, mean, case[2], case[3], n_blk, bre, bim, scale, out=out),
                        ops.segment_psd(xd, mean, case[2], case[3], n_blk, bre, bim, scale))
        ops.synchronize()
        assert same_bits(got, ref) and not bool(pt.isnan(got).any())
        assert bool(pt.isnan(buf[:guard]).all()) and bool(pt.isnan(buf[guard + size:]).all())


def test_frequency_subset_equals_the_columns_of_the_full_result(ops):
    from sparsespatialsampling_amd import spectral
    case = KERNEL_CASES[6]
    k = kernel_input(case)
    n, t, nperseg, hop, _ = case
    subset = np.array([65, 3, 0, 40, 41, 33])
    idx = pt.from_numpy(subset).cuda()
    sre, sim, _ = spectral.segment_matrix(nperseg, "hann", "constant", subset)
    xd = device_matrix(k["x"], "pitch16")
    args = (xd, ops.to_device(k["mean"]), nperseg, hop, k["n_blk"])
    full_c, full_p = launch(ops, xd, k, case, 0), launch(ops, xd, k, case, 1)
    assert same_bits(ops.segment_dft(*args, ops.to_device(sre), ops.to_device(sim)), full_c[:, idx].contiguous())
    assert same_bits(ops.segment_psd(*args, ops.to_device(sre), ops.to_device(sim), ops.to_device(k["scale"][subset])), full_p[:, idx].contiguous())
    x = pt.from_numpy(np.ascontiguousarray(k["x"].numpy()[:, :260])).cuda()
    f_all, p_all = spectral.welch(x, 0.01, nperseg=nperseg, noverlap=nperseg - hop)
    f_sub, p_sub = spectral.welch(x, 0.01, nperseg=nperseg, noverlap=nperseg - hop, frequencies=subset)
    assert same_bits(f_sub, f_all[idx].contiguous()) and same_bits(p_sub, p_all[:, idx].contiguous())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_welch_of_pressure_rows(ops, dtype):
    """rows of mean 1e5 and fluctuation 1e-2, L = 64: within the bound computed on x - mean (folding alone misses it by orders of
    magnitude: tests/test_spectral_reference.py::test_folding_alone_loses_the_mean)"""
    from sparsespatialsampling_amd import spectral
    n, t, nperseg, noverlap, dt = 129, 200, 64, 32, 0.01
    x = cc.rows(n, t, dtype, 21)
    xd = device_matrix(pt.from_numpy(x), "pitch16")
    freq, psd = spectral.welch(xd, dt, nperseg=nperseg, noverlap=noverlap)
    hop, n_blk = sc.segments(t, nperseg, noverlap)
    mean = ops.row_means(xd).cpu().numpy()                                   # the very doubles handed to the kernel
    assert np.abs(mean - cc.row_means(x)).max() <= 1e-10
    bre, bim, w = spectral.segment_matrix(nperseg, "hann", "constant")
    scale = sc.scale_vector(w, dt, n_blk, np.arange(nperseg // 2 + 1), nperseg)
    re, im, mre, mim = sc.coef_reference(x, mean, bre, bim, nperseg, hop, n_blk)
    r = sc.ratio(psd.cpu().numpy(), sc.psd_reference(re, im, scale), sc.psd_bound(re, im, sc.coef_bound(nperseg, mre), sc.coef_bound(nperseg, mim), scale))
    print(f"pressure rows {np.dtype(dtype).name}: PSD at {r:.3f} of the bound")
    assert r <= 1.0 and psd.is_cuda and psd.shape == (n, nperseg // 2 + 1)
    # ... and against the estimator restated from the data alone
    _, ref = sc.welch_reference(x, dt, nperseg, noverlap, "hann", "constant")
    e0 = sc.reference_error(x, w, nperseg)
    r = sc.ratio(psd.cpu().numpy(), ref, sc.psd_bound(re, im, sc.coef_bound(nperseg, mre, 1) + e0, sc.coef_bound(nperseg, mim, 1) + e0, scale, 1))
    assert r <= 1.0


@pytest.mark.parametrize("i", range(len(sc.SCIPY_CASES)))
def test_welch_against_scipy(ops, i):
    """|welch - scipy| <= the kernel's bound against long double + the fixture's tolerance (4 x scipy's own deviation from long double, of
    the row's largest value)"""
    from sparsespatialsampling_amd import spectral
    g = np.load(GOLDEN)
    n, t, nperseg, noverlap, win, detrend = sc.SCIPY_CASES[i]
    x, dt = g[f"x{i}"], float(g["dt"])
    freq, psd = spectral.welch(pt.from_numpy(x), dt, nperseg=nperseg, noverlap=noverlap, window=win, detrend=detrend)
    assert not psd.is_cuda and psd.dtype == pt.float64 and psd.shape == g[f"psd{i}"].shape
    assert np.allclose(freq.numpy(), g[f"freq{i}"], rtol=1e-14, atol=0)
    hop, n_blk = sc.segments(t, nperseg, noverlap)
    bre, bim, w = spectral.segment_matrix(nperseg, win, detrend)
    mean = cc.row_means(x) if detrend == "constant" else None
    if mean is not None:
        xd = ops.to_device(x)
        mean = ops.row_means(xd).cpu().numpy()
    scale = sc.scale_vector(w, dt, n_blk, np.arange(nperseg // 2 + 1), nperseg)
    re, im, mre, mim = sc.coef_reference(x, mean, bre, bim, nperseg, hop, n_blk)
    _, ref = sc.welch_reference(x, dt, nperseg, noverlap, win, detrend)
    e0 = sc.reference_error(x, w, nperseg)
    bound = sc.psd_bound(re, im, sc.coef_bound(nperseg, mre, 1) + e0, sc.coef_bound(nperseg, mim, 1) + e0, scale, 1)
    r = sc.ratio(psd.numpy(), ref, bound)
    total = bound + LD(float(g[f"tol{i}"])) * np.abs(ref).max(1, keepdims=True)
    r_s = sc.ratio(psd.numpy(), g[f"psd{i}"].astype(LD), total)
    print(f"case {i}: at {r:.3f} of the bound against long double, {r_s:.3f} of bound + tolerance against scipy")
    assert r <= 1.0 and r_s <= 1.0
    if n % 2 == 0:                                                           # the same rows as a vector field [N / 2, 2, T], from the device
        f3, p3 = spectral.welch(pt.from_numpy(x).reshape(n // 2, 2, t).cuda(), dt, nperseg=nperseg, noverlap=noverlap, window=win, detrend=detrend)
        assert p3.is_cuda and p3.shape == (n // 2, 2, psd.shape[1]) and same_bits(p3.reshape(n, -1), psd)
    spec = spectral.welch(pt.from_numpy(x), dt, nperseg=nperseg, noverlap=noverlap, window=win, detrend=detrend, scaling="spectrum")[1]
    _, ref_s = sc.welch_reference(x, dt, nperseg, noverlap, win, detrend, "spectrum")
    factor = (w.astype(LD) ** 2).sum() / (LD(dt) * w.astype(LD).sum() ** 2)
    assert sc.ratio(spec.numpy(), ref_s, bound * factor) <= 1.0


# ---- SPOD -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_comp", [None, 2])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_spod_against_reference(ops, dtype, n_comp):
    from sparsespatialsampling_amd import spectral
    c = sc.SPOD_CASE
    x, area, shapes = sc.spod_case(dtype, n_comp)
    nperseg, noverlap, dt = c["nperseg"], c["noverlap"], c["dt"]
    model = spectral.SPOD(pt.from_numpy(x).cuda(), dt, nperseg, noverlap, window=c["window"], cell_area=pt.from_numpy(area), detrend=c["detrend"])
    x2 = x.reshape(-1, c["t"])
    a_rows = np.repeat(area, n_comp or 1)
    hop, n_blk = sc.segments(c["t"], nperseg, noverlap)
    assert model.n_blocks == n_blk == 15
    k = np.arange(nperseg // 2 + 1)
    assert np.allclose(model.frequency.cpu().numpy(), k / (nperseg * dt), rtol=1e-15, atol=0)
    # references from the very doubles handed to the kernel
    mean = ops.row_means(ops.to_device(x2)).cpu().numpy()
    bre, bim, w = spectral.segment_matrix(nperseg, c["window"], None)
    re, im, mre, mim = sc.coef_reference(x2, mean, bre, bim, nperseg, hop, n_blk)
    kappa = float(LD(dt) / ((w.astype(LD) ** 2).sum() * n_blk))
    weyl = np.asarray(sc.spod_perturbation(re, im, sc.coef_bound(nperseg, mre), sc.coef_bound(nperseg, mim), a_rows, kappa), dtype=np.float64)
    al = a_rows.astype(LD)[:, None, None]
    s_re = np.einsum("ifb,ifc->fbc", al * re, re) + np.einsum("ifb,ifc->fbc", al * im, im)
    s_im = np.einsum("ifb,ifc->fbc", al * re, im) - np.einsum("ifb,ifc->fbc", al * im, re)
    s_ref = kappa * (s_re.astype(np.float64) + 1j * s_im.astype(np.float64))
    lam_ref, theta_ref = np.linalg.eigh(s_ref)
    lam_ref, theta_ref = lam_ref[:, ::-1], theta_ref[:, :, ::-1]
    factor = sc.one_sided(k, nperseg)
    lam = model.eigvals.cpu().numpy()
    r = float((np.abs(lam - factor[:, None] * lam_ref) / (factor * weyl)[:, None]).max())
    print(f"{np.dtype(dtype).name} n_comp {n_comp}: eigenvalues at {r:.3f} of the Weyl bound (bound / lambda_1 at most {float((weyl / lam_ref[:, 0]).max()):.2e})")
    assert lam.shape == (len(k), n_blk) and r <= 1.0 and bool((np.diff(lam, axis=1) <= 0).all())
    frac = model.energy_fraction().cpu().numpy()
    assert np.abs(frac.sum(1) - 1.0).max() <= 1e-14 and frac.shape == lam.shape
    q = (re + 1j * im).astype(np.complex128)
    for j, kbin in enumerate(c["bins"]):
        l1, l2 = lam_ref[kbin, 0], lam_ref[kbin, 1]
        assert l1 / l2 >= 1e3                                                # the mode comparison is well posed
        phi = model.modes(kbin, 2)
        assert phi.is_cuda and phi.dtype == pt.complex128 and phi.shape == x.shape[:-1] + (2,)
        phi = phi.cpu().numpy().reshape(-1, 2)
        # orthonormal under a: the eigenvectors diagonalise the computed S, which is within `weyl` of the S of the coefficients; the mode
        # GEMM adds (2 n_blk + 4) u per term, by Cauchy-Schwarz at most g sqrt(trace S / lambda_m) in the a-norm, g = 2 (2 n_blk + 4) u
        g = 2 * (2 * n_blk + 4) * sc.U
        tol = 2 * weyl[kbin] / l2 + 2 * g * np.sqrt(lam_ref[kbin].sum() / l2)
        ortho = (phi.conj().T * a_rows) @ phi
        print(f"bin {kbin}: orthonormality defect {np.abs(ortho - np.eye(2)).max():.2e} (allowed {tol:.2e})")
        assert np.abs(ortho - np.eye(2)).max() <= tol
        # the leading mode against the CPU one: Davis-Kahan at the asserted gap
        ref_mode = np.sqrt(kappa) * (q[:, kbin, :] @ theta_ref[kbin][:, 0]) / np.sqrt(l1)
        sin_theta = 2 * weyl[kbin] / (l1 - l2)
        defect = 1.0 - abs((ref_mode.conj() * a_rows * phi[:, 0]).sum())
        print(f"bin {kbin}: 1 - alignment {defect:.2e} (allowed {sin_theta ** 2 + tol:.2e}), lambda_1 / lambda_2 = {l1 / l2:.3g}")
        assert defect <= sin_theta ** 2 + tol
        assert abs((shapes[:, j].conj() * a_rows * phi[:, 0]).sum()) > 0.9999
    with pytest.raises(ValueError):
        model.modes(len(k), 1)
    with pytest.raises(ValueError):
        model.modes(0, n_blk + 1)


def test_spod_trace_equals_the_weighted_welch_psd(ops):
    """sum_k eigvals[f, k] = sum_i a_i psd_i(f) of welch with the same arguments.  Both come from the same accumulators; they differ by the
    PSD's own roundings (psd_bound with exact coefficients) and by the trace of the perturbation of S, at most n_blk times its norm"""
    from sparsespatialsampling_amd import spectral
    c = sc.SPOD_CASE
    x, area, _ = sc.spod_case(np.float32)
    nperseg, noverlap, dt = c["nperseg"], c["noverlap"], c["dt"]
    xd = device_matrix(pt.from_numpy(x), "odd", 1)
    model = spectral.SPOD(xd, dt, nperseg, noverlap, window=c["window"], cell_area=pt.from_numpy(area), detrend="constant")
    _, psd = spectral.welch(xd, dt, nperseg=nperseg, noverlap=noverlap, window=c["window"], detrend="constant")
    hop, n_blk = sc.segments(c["t"], nperseg, noverlap)
    mean = ops.row_means(xd).cpu().numpy()
    bre, bim, w = spectral.segment_matrix(nperseg, c["window"], "constant")
    k = np.arange(nperseg // 2 + 1)
    re, im, mre, mim = sc.coef_reference(x, mean, bre, bim, nperseg, hop, n_blk)
    e_re, e_im = sc.coef_bound(nperseg, mre), sc.coef_bound(nperseg, mim)
    kappa = float(LD(dt) / ((w.astype(LD) ** 2).sum() * n_blk))
    weyl = sc.spod_perturbation(re, im, e_re, e_im, area, kappa)
    scale = sc.scale_vector(w, dt, n_blk, k, nperseg)
    al = area.astype(LD)
    bound = sc.one_sided(k, nperseg) * n_blk * weyl + (al[:, None] * sc.psd_bound(re, im, e_re, e_im, scale)).sum(0)
    weighted = (al[:, None] * psd.cpu().numpy().astype(LD)).sum(0)
    r = sc.ratio(model.eigvals.cpu().numpy().astype(LD).sum(1), weighted, bound + LD(len(area) + n_blk) * LD(sc.U) * np.abs(weighted))
    print(f"trace identity at {r:.3f} of the bound")
    assert r <= 1.0


def test_spod_from_the_host_equals_the_device_result(ops):
    from sparsespatialsampling_amd import spectral
    c = sc.SPOD_CASE
    x, area, _ = sc.spod_case(np.float32)
    args = (c["dt"], c["nperseg"], c["noverlap"])
    host = spectral.SPOD(pt.from_numpy(x), *args, cell_area=pt.from_numpy(area), frequencies=[4, 9])
    dev = spectral.SPOD(pt.from_numpy(x).cuda(), *args, cell_area=pt.from_numpy(area).cuda(), frequencies=[4, 9])
    assert not host.eigvals.is_cuda and dev.eigvals.is_cuda and same_bits(host.eigvals, dev.eigvals) and host.eigvals.shape == (2, 15)
    m_h, m_d = host.modes(1, 3), dev.modes(1, 3)
    assert not m_h.is_cuda and m_d.is_cuda and same_bits(pt.view_as_real(m_h), pt.view_as_real(m_d))


def test_spod_refuses_coefficients_larger_than_free_memory(ops):
    """from the sizes alone, before any allocation: 128 rows x 1025 bins x 197 953 segments x 16 bytes = 4.2e11"""
    from sparsespatialsampling_amd import spectral
    x = pt.zeros((128, 200000), dtype=pt.float32, device="cuda")
    before = pt.cuda.memory_allocated()
    with pytest.raises(ValueError, match="frequencies") as err:
        spectral.SPOD(x, 0.01, 2048, noverlap=2047)
    assert str(16 * 128 * 1025 * 197953) in str(err.value) and pt.cuda.memory_allocated() == before
