"""
Data, long-double references, per-element bounds and float64 emulations for the segment DFT kernel (s3_segment_dft / s3_segment_psd,
csrc/spectral.hip) and for ``welch`` / ``SPOD`` (sparsespatialsampling_amd/spectral.py).  Shared by tests/test_spectral_reference.py
(CPU) and tests/test_gpu_spectral.py.  numpy only; every sum is a direct sum, there is no FFT in this file.

Two kinds of reference.  ``welch_reference`` / ``spod_reference`` restate the estimators from the data alone, in long double: segment
mean removed from the samples (no folded matrix), window, direct DFT.  ``coef_reference`` / ``psd_reference`` take the very doubles
handed to the kernel (mean, Bre, Bim, scale) and are what the kernel's bounds are measured against.  u = 2^-53.

Coefficients: ``c = sum_l (x - mean) B``, Re and Im each a real product of length L; bound ``(L + 4) u sum_l |x - mean| |B|`` -- the GEMM
bound of tests/centered_cases.py: one rounding for the centring, L for the FMA chain, the rest is room.

PSD: ``p = scale sum_b (re_b^2 + im_b^2)``.  With e_b = hypot(e_re, e_im) the coefficient bound as a complex magnitude,
``| |c^_b|^2 - |c_b|^2 | <= 2 |c_b| e_b + e_b^2``.  The kernel rounds re^2, im^2 and their sum (2 u of the segment's power to first
order), adds n_blk of them (n_blk - 1 roundings) and multiplies by scale (1): ``(n_blk + 2) u p``.  Bound:
``scale sum_b (2 |c_b| e_b + e_b^2) + (n_blk + 3) u |p|``.

Against a reference that does not share the kernel's operands (``welch_reference``, scipy) one more u per term accounts for the rounding of
the folded matrix to float64 (``extra=1``) and one more u of the result for the rounding of ``scale`` (``extra_scale=1``).  Such a
reference removes the segment mean from the raw samples in long double and carries a rounding error of its own, negligible except where
the exact value is zero (the mean bin of a detrended boxcar segment): ``reference_error`` = (2 L + 4) 2^-64 max|x| sum|w| per coefficient,
L roundings for the mean and L for the sum; it is added to the coefficient bounds in those comparisons.

SPOD: ``S = kappa Q^H W Q``.  An element of the computed S differs from the one of the exact coefficients by at most
``kappa [ sum_i a_i (|q_ib| e_ib' + e_ib |q_ib'| + e_ib e_ib') + ((N + 8) u + 3 u) sum_i a_i (|A| + |B|)_ib (|A| + |B|)_ib' ]``: the
coefficient bounds carried through the product, the Gram bound of centered_cases for each of the four real blocks (their sum of |terms| is
below the last sum) and three roundings of the assembly (rr + ii, ri - ir, times kappa).  Weyl: every eigenvalue moves by at most the
2-norm of that perturbation, itself below the Frobenius norm of the element bounds; the Hermitian solver on the host is backward stable,
``10 n_blk u ||S||_F`` is allowed for it.  Davis-Kahan (in the form of Yu, Wang and Samworth 2015): the leading eigenvector turns by
``sin(theta) <= 2 ||E|| / (lambda_1 - lambda_2)``.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
PI = LD(4) * np.arctan(LD(1))

# (N, T, L, noverlap, window, detrend) -- the cases of tests/golden/welch_scipy.npz; the fifth is the reference's call
SCIPY_CASES = [(5, 8, 4, 2, "hann", "constant"), (17, 33, 7, 3, "hann", "constant"), (9, 130, 16, 0, "boxcar", False),
               (3, 257, 130, 65, "hamming", "constant"), (4, 100, 100, 0, "boxcar", "constant"), (6, 257, 64, 63, "hann", False),
               (6, 259, 33, 16, "hann", "constant")]


def scipy_case_data(i):
    """float64 [N, T] of fixture case i: row means about 1e3, unit fluctuation with two tones"""
    n, t = SCIPY_CASES[i][:2]
    rng = np.random.default_rng(100 + i)
    tt = np.arange(t)
    return (1e3 * (1.0 + 0.1 * rng.standard_normal((n, 1))) + rng.standard_normal((n, t))
            + np.sin(2 * np.pi * 0.11 * tt)[None, :] + 0.5 * np.cos(2 * np.pi * 0.27 * tt + rng.uniform(0, 6, (n, 1))))


def window(name, nperseg):
    """float64 [L], periodic form"""
    if not isinstance(name, str):
        return np.asarray(name, dtype=np.float64)
    if name == "boxcar" or nperseg == 1:
        return np.ones(nperseg)
    a0 = {"hann": LD("0.5"), "hamming": LD("0.54")}[name]
    return (a0 - (LD(1) - a0) * np.cos(2 * PI * np.arange(nperseg).astype(LD) / LD(nperseg))).astype(np.float64)


def segments(t, nperseg, noverlap):
    hop = nperseg - noverlap
    return hop, (t - noverlap) // hop


def twiddles(nperseg, k):
    """exp(-2 pi i l k / L) [L, n_f] in long double, from the integer phase"""
    angle = 2 * PI * ((np.arange(nperseg)[:, None] * np.asarray(k)[None, :]) % nperseg).astype(LD) / LD(nperseg)
    return np.cos(angle), -np.sin(angle)


def dft_matrix(nperseg, w, fold, k=None):
    """(Bre, Bim) float64 [L, n_f]: window times twiddle, the segment mean's removal folded in when ``fold``"""
    k = np.arange(nperseg // 2 + 1) if k is None else np.asarray(k)
    c, s = twiddles(nperseg, k)
    wl = np.asarray(w, dtype=np.float64).astype(LD)[:, None]
    bre, bim = wl * c, wl * s
    if fold:
        bre, bim = bre - bre.sum(0) / LD(nperseg), bim - bim.sum(0) / LD(nperseg)
    return bre.astype(np.float64), bim.astype(np.float64)


def one_sided(k, nperseg, mistake=None):
    k = np.asarray(k)
    if mistake == "no_doubling":
        return np.ones(len(k))
    if mistake == "nyquist_doubled":
        return np.where(k == 0, 1.0, 2.0)
    return np.where((k == 0) | ((nperseg % 2 == 0) & (k == nperseg // 2)), 1.0, 2.0)


def scale_vector(w, dt, n_blk, k, nperseg, scaling="density", mistake=None):
    wl = np.asarray(w, dtype=np.float64).astype(LD)
    base = LD(dt) / (wl * wl).sum() if scaling == "density" else LD(1) / wl.sum() ** 2
    return (base * one_sided(k, nperseg, mistake).astype(LD) / LD(n_blk)).astype(np.float64)


def ratio(got, ref, bound):
    """largest |got - ref| / bound over the elements (0 / 0 = 0, anything not a number = inf)"""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf))
    return float(np.where(np.isnan(r), np.inf, r).max())


# ---- from the data alone ----------------------------------------------------------------------------------------------------------
def segment_coefficients(x, nperseg, noverlap, w, detrend, k):
    """(re, im) long double [N, n_f, n_blk]: detrend on the samples, window, direct DFT.  ``detrend``: "constant" (segment mean), "mean"
    (the row's long-time mean), False / None"""
    x = np.asarray(x).astype(LD)
    hop, n_blk = segments(x.shape[1], nperseg, noverlap)
    if detrend == "mean":
        x = x - x.mean(1, keepdims=True)
    c, s = twiddles(nperseg, k)
    wl = np.asarray(w, dtype=np.float64).astype(LD)
    re, im = (np.empty((x.shape[0], len(k), n_blk), dtype=LD) for _ in range(2))
    for b in range(n_blk):
        seg = x[:, b * hop:b * hop + nperseg]
        if detrend == "constant":
            seg = seg - seg.mean(1, keepdims=True)
        seg = seg * wl
        re[:, :, b], im[:, :, b] = seg @ c, seg @ s
    return re, im


def welch_reference(x, dt, nperseg, noverlap, win, detrend, scaling="density", k=None):
    """(freq float64 [n_f], psd long double [N, n_f]) as scipy.signal.welch defines them"""
    k = np.arange(nperseg // 2 + 1) if k is None else np.asarray(k)
    w = window(win, nperseg)
    re, im = segment_coefficients(x, nperseg, noverlap, w, detrend, k)
    wl = w.astype(LD)
    base = LD(dt) / (wl * wl).sum() if scaling == "density" else LD(1) / wl.sum() ** 2
    return k / (nperseg * float(dt)), (re * re + im * im).mean(2) * base * one_sided(k, nperseg).astype(LD)


def spod_reference(x, dt, nperseg, noverlap, win, area, detrend):
    """direct SPOD in numpy: (eigenvalues [n_f, n_blk] descending, one-sided; modes complex128 [n_f, N, n_blk], a-orthonormal)"""
    k = np.arange(nperseg // 2 + 1)
    w = window(win, nperseg)
    re, im = segment_coefficients(x, nperseg, noverlap, w, detrend, k)
    q = (re + 1j * im).astype(np.complex128)                                 # [N, n_f, n_blk]
    n_blk = q.shape[2]
    kappa = float(LD(dt) / ((w.astype(LD) ** 2).sum() * n_blk))
    a = np.ones(q.shape[0]) if area is None else np.asarray(area, dtype=np.float64)
    lam, modes = np.empty((len(k), n_blk)), np.empty((len(k), q.shape[0], n_blk), dtype=np.complex128)
    for f in range(len(k)):
        qf = q[:, f, :]
        s = kappa * (qf.conj().T * a) @ qf
        ev, th = np.linalg.eigh(0.5 * (s + s.conj().T))
        ev, th = ev[::-1], th[:, ::-1]
        lam[f] = ev * one_sided(k, nperseg)[f]
        with np.errstate(divide="ignore", invalid="ignore"):
            modes[f] = np.sqrt(kappa) * (qf @ th) / np.sqrt(ev)
    return lam, modes


# ---- from the kernel's operands ---------------------------------------------------------------------------------------------------
def coef_reference(x, mean, bre, bim, nperseg, hop, n_blk):
    """(re, im, mag_re, mag_im) long double [N, n_f, n_blk]: the products and the sums of |terms| behind their bounds"""
    d = np.asarray(x).astype(LD)
    if mean is not None:
        d = d - np.asarray(mean, dtype=np.float64).astype(LD)[:, None]
    br, bi = np.asarray(bre, dtype=np.float64).astype(LD), np.asarray(bim, dtype=np.float64).astype(LD)
    out = [np.empty((d.shape[0], br.shape[1], n_blk), dtype=LD) for _ in range(4)]
    for b in range(n_blk):
        seg = d[:, b * hop:b * hop + nperseg]
        out[0][:, :, b], out[1][:, :, b] = seg @ br, seg @ bi
        out[2][:, :, b], out[3][:, :, b] = np.abs(seg) @ np.abs(br), np.abs(seg) @ np.abs(bi)
    return tuple(out)


def reference_error(x, w, nperseg):
    """[N, 1, 1]: rounding error of a coefficient of ``segment_coefficients`` itself (module docstring)"""
    x = np.asarray(x).astype(LD)
    return (LD(2 * nperseg + 4) * LD(2.0 ** -64) * np.abs(x).max(1) * np.abs(np.asarray(w, dtype=np.float64)).sum())[:, None, None]


def coef_bound(nperseg, mag, extra=0):
    return LD(nperseg + 4 + extra) * LD(U) * mag


def interleave(re, im):
    """[N, n_f, n_blk] x 2 -> the kernel's layout [N, n_f, n_blk, 2]"""
    return np.stack([re, im], axis=-1)


def psd_reference(re, im, scale):
    return (re * re + im * im).sum(2) * np.asarray(scale, dtype=np.float64).astype(LD)


def psd_bound(re, im, e_re, e_im, scale, extra_scale=0):
    n_blk = re.shape[2]
    e, c = np.hypot(e_re, e_im), np.hypot(re, im)
    sc = np.abs(np.asarray(scale, dtype=np.float64).astype(LD))
    return sc * (2 * c * e + e * e).sum(2) + LD(n_blk + 3 + extra_scale) * LD(U) * np.abs(psd_reference(re, im, scale))


def fma(a, b, c):
    """a * b + c rounded once to float64, as the matrix cores do it"""
    return (np.asarray(a).astype(LD) * np.asarray(b).astype(LD) + np.asarray(c).astype(LD)).astype(np.float64)


def emulated(x, mean, bre, bim, nperseg, hop, n_blk, scale, mistake=None):
    """float64 emulation of the kernel: (coef [N, n_f, n_blk, 2], psd [N, n_f]).  ``mistake``: "mean_f32" centres with the mean rounded to
    float32; "start_bL" starts segment b at min(b L, T - L) instead of b hop; "trailing" adds the samples past the last segment as one more,
    zero-padded segment to the power (coefficients unchanged)"""
    x = np.asarray(x).astype(np.float64)
    t = x.shape[1]
    if mean is not None:
        x = x - (np.asarray(mean).astype(np.float32).astype(np.float64) if mistake == "mean_f32" else np.asarray(mean))[:, None]
    bre, bim = np.asarray(bre, dtype=np.float64), np.asarray(bim, dtype=np.float64)

    def transform(seg):
        re, im = np.zeros((x.shape[0], bre.shape[1])), np.zeros((x.shape[0], bre.shape[1]))
        for l in range(seg.shape[1]):
            re, im = fma(seg[:, l][:, None], bre[l][None, :], re), fma(seg[:, l][:, None], bim[l][None, :], im)
        return re, im

    coef = np.empty((x.shape[0], bre.shape[1], n_blk, 2))
    power = np.zeros((x.shape[0], bre.shape[1]))
    for b in range(n_blk):
        start = min(b * nperseg, t - nperseg) if mistake == "start_bL" else b * hop
        re, im = transform(x[:, start:start + nperseg])
        coef[:, :, b, 0], coef[:, :, b, 1] = re, im
        power = power + (re * re + im * im)
    if mistake == "trailing":
        re, im = transform(x[:, n_blk * hop:])
        power = power + (re * re + im * im)
    return coef, np.asarray(scale, dtype=np.float64) * power


# ---- SPOD ---------------------------------------------------------------------------------------------------------------------------
SPOD_CASE = dict(n=257, t=260, nperseg=32, noverlap=16, dt=0.01, bins=(4, 9), window="hamming", detrend="mean")


def spod_case(dtype=np.float64, n_comp=None, seed=7):
    """(data [N, T] or [N, n_comp, T], areas [N], planted shapes complex [N * n_comp, 2]): two travelling waves at bins 4 and 9 of L = 32 with
    a-orthonormal shapes, amplitudes 1 and 0.6, noise 1e-3, offset 50; areas over 1e-3 .. 1e1"""
    c = SPOD_CASE
    rng = np.random.default_rng(seed)
    n = c["n"]
    rows = n * (n_comp or 1)
    area = 10.0 ** rng.uniform(-3.0, 1.0, n)
    area[0], area[-1] = 1e-3, 1e1
    a_rows = np.repeat(area, n_comp or 1)
    shapes = rng.standard_normal((rows, 2)) + 1j * rng.standard_normal((rows, 2))
    shapes[:, 0] /= np.sqrt((a_rows * np.abs(shapes[:, 0]) ** 2).sum())
    shapes[:, 1] -= shapes[:, 0] * (a_rows * shapes[:, 0].conj() * shapes[:, 1]).sum()
    shapes[:, 1] /= np.sqrt((a_rows * np.abs(shapes[:, 1]) ** 2).sum())
    tt = np.arange(c["t"])
    x = 50.0 + 1e-3 * rng.standard_normal((rows, c["t"]))
    for j, (kbin, amp) in enumerate(zip(c["bins"], (1.0, 0.6))):
        x = x + amp * np.real(shapes[:, j][:, None] * np.exp(2j * np.pi * kbin * tt / c["nperseg"])[None, :])
    x = x.astype(dtype)
    return (x.reshape(n, n_comp, c["t"]) if n_comp else x), area, shapes


def spod_perturbation(re, im, e_re, e_im, area, kappa):
    """Frobenius norm per frequency [n_f] of the element bounds of ``S_f`` (module docstring), plus the solver's allowance; ``re`` / ``im`` /
    bounds long double [N, n_f, n_blk]"""
    a = np.asarray(area, dtype=np.float64).astype(LD)[:, None, None]
    n, n_blk = re.shape[0], re.shape[2]
    q, e = np.hypot(re, im), np.hypot(e_re, e_im)
    s1 = np.abs(re) + np.abs(im) + e_re + e_im
    aq, ae, as1 = a * q, a * e, a * s1
    carried = np.einsum("ifb,ifc->fbc", aq, e) + np.einsum("ifb,ifc->fbc", ae, q) + np.einsum("ifb,ifc->fbc", ae, e)
    rounded = LD(n + 11) * LD(U) * np.einsum("ifb,ifc->fbc", as1, s1)
    s_abs = LD(kappa) * np.einsum("ifb,ifc->fbc", aq, q)
    elem = LD(kappa) * (carried + rounded)
    return np.sqrt((elem ** 2).sum((1, 2))) + LD(10 * n_blk) * LD(U) * np.sqrt((s_abs ** 2).sum((1, 2)))
