"""
Welch spectra and spectral POD of a field on the S^3 grid or on the original CFD mesh -- the time-frequency end of the workflow.
The reference's ``post_processing/compare_svd_OAT.py:56-70`` passes every POD coefficient through
``scipy.signal.welch(v, fs=1/dt, nperseg=n_samples, nfft=n_samples, window="boxcar")`` to find the buffet frequency; here the same
estimator runs per cell of a field (``welch``), and the cross-spectral matrix of the same segments gives the spectral POD (``SPOD``,
restated from Towne, Schmidt & Colonius 2018 and not pinned against another implementation, like ``dmd.DMD``).  Conventions are
scipy's: one-sided, interior frequencies doubled, mean over the segments, no zero padding (nfft = nperseg).

How it runs on the MI355X.  Every row of the data [N, T] is cut into ``n_blk = (T - noverlap) // (nperseg - noverlap)`` segments of
L = ``nperseg`` samples, ``hop = L - noverlap`` apart; samples past the last segment are dropped.  A segment's windowed, detrended
DFT is its product with the [L, 2 n_f] matrix ``segment_matrix`` builds on the host, so the whole step is ONE tall product on the f64
matrix cores (``segment_dft_kernel``, csrc/spectral.hip) -- any L, the per-element error bound of a GEMM.  The data is read where it
lies, float32 or float64, rows possibly pitched; float32 is widened in the kernel's operand staging.

* ``welch``: one ``s3_segment_psd`` launch.  The coefficients stay in the kernel's accumulators, the power is summed over the
  segments in registers and the PSD [N, n_f] is written once; nothing of size N x n_blk x n_f exists.
* ``SPOD``: one ``s3_segment_dft`` launch writes the coefficients ``Q [N, n_f, n_blk, 2]``; per frequency one ``s3_gram`` (weights =
  cell areas) of the pitched real view [N, 2 n_blk] gives A^T W A, A^T W B, B^T W B (Q_f = A + iB), from which the Hermitian
  ``S_f = kappa Q_f^H W Q_f`` [n_blk, n_blk] is assembled and solved on the host (``_spod_small``); modes on demand, one
  ``s3_tall_gemm`` per frequency, whose [N, 2 n_modes] result IS the complex matrix.

The long-time mean: with ``detrend="constant"`` the segment mean is removed by folding ``B <- B - 1 (1^T B) / L`` into the matrix.
Folding alone would leave the row's mean to cancel inside the product -- a pressure row of 1e5 +- 1e-2 keeps about 5e-6 relative
at L = 256 -- so the row's long-time mean (``s3_row_moments``) is subtracted in the kernel's staging first: removing the segment
mean of ``x - row mean`` gives the values of removing it from ``x``.
"""
import math

import numpy as np
import torch as pt

from . import hipops
from .arrays import Side, resident_matrix
from .dmd import _check_arguments

LD = np.longdouble
WINDOWS = ("boxcar", "hann", "hamming")


def _window(window, nperseg):
    """float64 [L]: a named window in its periodic (DFT-even) form -- the values of ``scipy.signal.get_window(name, L)`` -- or the
    caller's array"""
    if isinstance(window, str):
        if window not in WINDOWS:
            raise ValueError(f"window must be one of {WINDOWS} or an array of nperseg values, got {window!r}")
        if window == "boxcar" or nperseg == 1:
            return np.ones(nperseg, dtype=np.float64)
        a0 = LD("0.5") if window == "hann" else LD("0.54")
        n = np.arange(nperseg, dtype=np.int64).astype(LD)
        return (a0 - (LD(1) - a0) * np.cos(2 * _pi() * n / LD(nperseg))).astype(np.float64)
    w = np.asarray(pt.as_tensor(window).detach().cpu().numpy() if isinstance(window, pt.Tensor) else window, dtype=np.float64).reshape(-1)
    if len(w) != nperseg or not np.all(np.isfinite(w)):
        raise ValueError(f"a window array must hold nperseg = {nperseg} finite values, got {len(w)}")
    return w


def _pi():
    """pi to the precision of long double (np.pi is the float64 value)"""
    return LD(4) * np.arctan(LD(1))


def _frequencies(frequencies, nperseg):
    """indices of the one-sided bins kept: all of 0 .. L // 2, or the caller's subset (any order)"""
    if frequencies is None:
        return np.arange(nperseg // 2 + 1, dtype=np.int64)
    f = np.asarray(pt.as_tensor(frequencies).cpu().numpy() if isinstance(frequencies, pt.Tensor) else frequencies)
    if f.ndim != 1 or len(f) < 1 or not np.issubdtype(f.dtype, np.integer):
        raise ValueError("frequencies must be a non-empty 1-D list of integer bin indices")
    f = f.astype(np.int64)
    if f.min() < 0 or f.max() > nperseg // 2:
        raise ValueError(f"frequencies must be bin indices in [0, {nperseg // 2}] (one-sided, nperseg = {nperseg})")
    return f


def segment_matrix(nperseg, window, detrend, frequencies=None):
    """(Bre, Bim, w): the two float64 planes [L, n_f] with ``coefficient = segment @ (Bre + i Bim)`` and the window [L].  Column f is
    ``w[l] exp(-2 pi i l k_f / L)`` with the twiddle taken from the INTEGER phase ``(l k_f) mod L``, evaluated in long double and rounded
    once; ``detrend="constant"`` folds the removal of the segment mean into the columns, ``B <- B - 1 (1^T B) / L``.  ``frequencies``:
    bin indices k_f (None: 0 .. L // 2).  numpy only."""
    nperseg = int(nperseg)
    if nperseg < 1:
        raise ValueError(f"nperseg must be positive, got {nperseg}")
    if detrend not in ("constant", "mean", False, None):
        raise ValueError(f"detrend must be 'constant', 'mean', False or None, got {detrend!r}")
    w = _window(window, nperseg)
    k = _frequencies(frequencies, nperseg)
    phase = (np.arange(nperseg, dtype=np.int64)[:, None] * k[None, :]) % nperseg
    angle = 2 * _pi() * phase.astype(LD) / LD(nperseg)
    wl = w.astype(LD)[:, None]
    bre, bim = wl * np.cos(angle), -wl * np.sin(angle)
    if detrend == "constant":
        bre = bre - bre.sum(0, keepdims=True) / LD(nperseg)
        bim = bim - bim.sum(0, keepdims=True) / LD(nperseg)
    return np.ascontiguousarray(bre.astype(np.float64)), np.ascontiguousarray(bim.astype(np.float64)), w


def _segments(t, nperseg, noverlap, default_nperseg):
    """(L, noverlap, hop, n_blk) by scipy's rules"""
    nperseg = default_nperseg if nperseg is None else int(nperseg)
    if not 1 <= nperseg <= t:
        raise ValueError(f"nperseg must lie in [1, {t}] (the number of snapshots), got {nperseg}")
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    if not 0 <= noverlap < nperseg:
        raise ValueError(f"noverlap must lie in [0, nperseg = {nperseg}), got {noverlap}")
    hop = nperseg - noverlap
    return nperseg, noverlap, hop, (t - noverlap) // hop


def one_sided_factor(k, nperseg):
    """2 for the interior bins, 1 for the mean (k = 0) and, at even L, the Nyquist bin (k = L / 2)"""
    k = np.asarray(k)
    return np.where((k == 0) | ((nperseg % 2 == 0) & (k == nperseg // 2)), 1.0, 2.0)


def psd_scale(w, dt, n_blk, k, nperseg, scaling):
    """float64 [n_f]: what the summed power of bin k is multiplied by -- ``dt / sum w^2`` (density) or ``1 / (sum w)^2`` (spectrum),
    the one-sided factor, and 1 / n_blk for the mean over the segments"""
    wl = np.asarray(w, dtype=np.float64).astype(LD)
    base = LD(dt) / (wl * wl).sum() if scaling == "density" else LD(1) / wl.sum() ** 2
    return (base * one_sided_factor(k, nperseg).astype(LD) / LD(n_blk)).astype(np.float64)


def welch(data, dt, nperseg=None, noverlap=None, window="hann", detrend="constant", scaling="density", frequencies=None):
    """Power spectral density of every row of ``data`` [N, T] or [N, n_comp, T] (float32 or float64, host or device; a 2-D matrix may
    be pitched) by Welch's method, as ``scipy.signal.welch(data, fs=1/dt, ...)`` returns it: defaults ``nperseg = min(256, T)``,
    ``noverlap = nperseg // 2``, one-sided, mean over the segments.  ``window``: "boxcar", "hann", "hamming" or an array;
    ``detrend``: "constant" or False; ``scaling``: "density" or "spectrum"; ``frequencies``: bin indices to keep (None: all
    ``nperseg // 2 + 1``).  Returns ``(freq [n_f], psd data.shape[:-1] + (n_f,))``, float64, on the side the data came from.
    The reference's call is ``welch(V.T, dt, nperseg=T, noverlap=0, window="boxcar")``."""
    n_cells, n_comp, t = _check_arguments(data, dt, None, None, who="welch", min_snapshots=1)
    nperseg, noverlap, hop, n_blk = _segments(t, nperseg, noverlap, min(256, t))
    if detrend not in ("constant", False, None):
        raise ValueError(f"detrend must be 'constant' or False, got {detrend!r}")
    if scaling not in ("density", "spectrum"):
        raise ValueError(f"scaling must be 'density' or 'spectrum', got {scaling!r}")
    k = _frequencies(frequencies, nperseg)
    w = _window(window, nperseg)
    d2 = resident_matrix(data, n_cells, n_comp, t)                            # (HipUnavailableError without a device)
    bre, bim, w = segment_matrix(nperseg, w, detrend, k)
    scale = psd_scale(w, float(dt), n_blk, k, nperseg, scaling)
    mean = hipops.row_means(d2) if detrend == "constant" else None
    psd = hipops.segment_psd(d2, mean, nperseg, hop, n_blk, hipops.to_device(bre), hipops.to_device(bim), hipops.to_device(scale))
    psd = psd.reshape(tuple(data.shape[:-1]) + (len(k),))
    freq = pt.from_numpy(k.astype(np.float64) / (nperseg * float(dt)))
    hipops.synchronize()                                                      # (the caller's matrix is not kept alive)
    side = Side(data)
    return side.back(freq), side.back(psd)


def _spod_small(grams, kappa):
    """the host part of the SPOD, from the Gram blocks alone.  ``grams`` [n_f, 2 n_blk, 2 n_blk] float64: the weighted Gram matrix of
    the real view [N, 2 n_blk] of every frequency's coefficients, columns 2b, 2b + 1 = Re, Im of segment b.  With Q = A + iB,
    ``Q^H W Q = (A^T W A + B^T W B) + i (A^T W B - B^T W A)``.  Returns (eigenvalues [n_f, n_blk] of ``S_f = kappa Q^H W Q``, descending,
    clamped at 0; eigenvectors [n_f, n_blk, n_blk], columns, largest component real and positive)."""
    g = pt.as_tensor(grams, dtype=pt.float64)
    rr, ii, ri, ir = g[:, 0::2, 0::2], g[:, 1::2, 1::2], g[:, 0::2, 1::2], g[:, 1::2, 0::2]
    s = kappa * pt.complex(rr + ii, ri - ir)
    s = 0.5 * (s + s.conj().transpose(1, 2))
    lam, theta = pt.linalg.eigh(s)
    lam, theta = lam.flip(1).clamp_min(0.0), theta.flip(2)
    top = theta.abs().argmax(dim=1, keepdim=True)
    pivot = pt.gather(theta, 1, top)
    return lam, theta * (pivot.conj() / pivot.abs())


def _mode_rhs(theta, lam, kappa):
    """real [2 n_blk, 2 n_modes] embedding of ``C = sqrt(kappa) Theta Lambda^-1/2``: with the real view (A_b, B_b) of Q,
    ``Re(Q C) = A Cr - B Ci`` and ``Im(Q C) = A Ci + B Cr``; columns 2m, 2m + 1 are Re and Im of mode m"""
    c = math.sqrt(kappa) * theta / lam.sqrt().to(pt.complex128)
    rhs = pt.empty((2 * c.shape[0], 2 * c.shape[1]), dtype=pt.float64)
    rhs[0::2, 0::2], rhs[1::2, 0::2] = c.real, -c.imag
    rhs[0::2, 1::2], rhs[1::2, 1::2] = c.imag, c.real
    return rhs


class SPOD:
    """Spectral proper orthogonal decomposition of ``data`` [N_cells, T] or [N_cells, N_dims, T] (components stacked as
    ``compute_svd`` does, the weights repeated per component), float32 or float64, host or device, rows of a 2-D matrix possibly
    pitched.  At every frequency the eigenpairs of the Welch cross-spectral matrix under the inner product ``diag(cell_area)``:
    ``S_f = kappa Q_f^H diag(a) Q_f`` with ``kappa = dt / (sum w^2 n_blk)`` and Q_f [N, n_blk] the windowed DFT coefficients of the
    segments.  ``detrend``: "mean" (the row's long-time mean), "constant" (the segment mean as well) or None; ``frequencies``: bin
    indices to keep -- Q holds ``16 N n_f n_blk`` bytes on the device, and this bounds it.

    Members (on the side the data came from): ``frequency`` [n_f], ``n_blocks``, ``eigvals`` [n_f, n_blk] descending, one-sided (the
    interior bins doubled): ``eigvals.sum(1)`` is ``sum_i a_i psd_i(f)`` of ``welch`` with the same arguments; ``modes(i_freq, n_modes)``
    complex128 [N_cells, (N_dims,) n_modes], orthonormal under ``diag(a)``, computed on demand; ``energy_fraction()``."""

    def __init__(self, data, dt, nperseg, noverlap=None, window="hamming", cell_area=None, detrend="mean", frequencies=None):
        n_cells, n_comp, t = _check_arguments(data, dt, None, cell_area, who="SPOD", min_snapshots=1)
        nperseg, noverlap, hop, n_blk = _segments(t, nperseg, noverlap, None)
        if detrend not in ("mean", "constant", False, None):
            raise ValueError(f"detrend must be 'mean', 'constant' or None, got {detrend!r}")
        k = _frequencies(frequencies, nperseg)
        w = _window(window, nperseg)
        self.dt, self.nperseg, self.noverlap, self.n_blocks = float(dt), nperseg, noverlap, n_blk
        self._side = Side(data)
        self._shape = tuple(data.shape)
        n_rows = n_cells * (n_comp or 1)
        need = 16 * n_rows * len(k) * n_blk
        free = int(pt.cuda.mem_get_info(hipops.device())[0])                  # (HipUnavailableError without a device)
        if need > free:
            raise ValueError(f"SPOD: the coefficients of {n_rows} rows x {len(k)} frequencies x {n_blk} segments take {need} bytes "
                             f"({need / 2 ** 30:.1f} GiB), the device has {free} free; keep fewer bins with frequencies=")
        d2 = resident_matrix(data, n_cells, n_comp, t)
        bre, bim, w = segment_matrix(nperseg, w, "constant" if detrend == "constant" else None, k)
        wl = w.astype(LD)
        self._kappa = float(LD(self.dt) / ((wl * wl).sum() * LD(n_blk)))
        self._factor = pt.from_numpy(one_sided_factor(k, nperseg))
        self._frequency = pt.from_numpy(k.astype(np.float64) / (nperseg * self.dt))
        weight = None
        if cell_area is not None:
            weight = hipops.to_device(cell_area, pt.float64).reshape(-1)
            if n_comp is not None:
                weight = weight.repeat_interleave(n_comp)                     # row (n, c) keeps the area of cell n
        mean = hipops.row_means(d2) if detrend in ("mean", "constant") else None
        self._coef = hipops.segment_dft(d2, mean, nperseg, hop, n_blk, hipops.to_device(bre), hipops.to_device(bim))
        n_f, width = len(k), 2 * n_blk
        flat = self._coef.view(n_rows, n_f * width)
        grams = pt.empty((n_f, width, width), dtype=pt.float64, device=d2.device)
        scratch = hipops.gram_scratch(n_rows, width, d2.device)
        for f in range(n_f):                                                  # the pitched [N, 2 n_blk] matrix of frequency f, as it stands
            hipops.gram(flat[:, f * width:(f + 1) * width], None, weight, out=grams[f], scratch=scratch)
        self._lam, self._theta = _spod_small(pt.from_numpy(hipops.to_host(grams)), self._kappa)
        del grams, scratch, weight

    @property
    def frequency(self):
        return self._side.back(self._frequency)

    @property
    def eigvals(self):
        return self._side.back(self._lam * self._factor[:, None])

    def energy_fraction(self):
        """share of each mode in its frequency's total [n_f, n_blk]"""
        total = self._lam.sum(1, keepdim=True)
        return self._side.back(self._lam / pt.where(total > 0, total, pt.ones_like(total)))

    def modes(self, i_freq, n_modes=None):
        """the leading ``n_modes`` (None: all n_blk) SPOD modes of frequency ``i_freq``: ``sqrt(kappa) Q_f Theta Lambda^-1/2``, complex128
        [N_cells, (N_dims,) n_modes], orthonormal under ``diag(cell_area)``"""
        i_freq = int(i_freq)
        n_modes = self.n_blocks if n_modes is None else int(n_modes)
        if not 0 <= i_freq < len(self._frequency):
            raise ValueError(f"i_freq must lie in [0, {len(self._frequency)}), got {i_freq}")
        if not 1 <= n_modes <= self.n_blocks:
            raise ValueError(f"n_modes must lie in [1, {self.n_blocks}], got {n_modes}")
        lam = self._lam[i_freq, :n_modes]
        if float(lam.min()) <= 0.0:
            raise ValueError(f"mode {int((lam <= 0).nonzero()[0])} of frequency {i_freq} carries no energy: ask for fewer modes")
        rhs = _mode_rhs(self._theta[i_freq][:, :n_modes], lam, self._kappa)
        width = 2 * self.n_blocks
        flat = self._coef.view(self._coef.shape[0], -1)
        out = hipops.tall_gemm(flat[:, i_freq * width:(i_freq + 1) * width], hipops.to_device(rhs))
        z = pt.view_as_complex(out.reshape(-1, n_modes, 2)).reshape(self._shape[:-1] + (n_modes,))
        return self._side.back(z)
