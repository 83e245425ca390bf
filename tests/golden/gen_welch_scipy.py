"""Generator of tests/golden/welch_scipy.npz: what ``scipy.signal.welch(x, fs=1/dt, window, nperseg, noverlap, detrend)`` returns on the
seven cases of tests/spectral_cases.py (SCIPY_CASES; the fifth is the call of the reference's post_processing/compare_svd_OAT.py:56-70,
one boxcar segment as long as the series).  scipy is the source here (installed in the dev container; a third-party dependency of the
reference, not the reference); the GPU machine need not have it.

scipy works in float64 through an FFT, so it deviates from the long-double direct sums of ``spectral_cases.welch_reference``: the
generator measures that deviation per case -- the largest |scipy - reference| over a row, relative to the row's largest PSD value (a
detrended mean bin holds rounding noise only and has no relative accuracy of its own) -- and stores 4 x it as ``tol{i}``, the
tolerance tests/test_spectral_reference.py holds the reference to.
    python tests/golden/gen_welch_scipy.py"""
import os
import sys

import numpy as np
import scipy
import scipy.signal

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import spectral_cases as sc                                                     # noqa: E402

DT = 0.004
out = {"scipy_version": np.array(scipy.__version__), "dt": np.array(DT), "n_cases": np.array(len(sc.SCIPY_CASES))}
for i, (n, t, nperseg, noverlap, win, detrend) in enumerate(sc.SCIPY_CASES):
    x = sc.scipy_case_data(i)
    assert x.shape == (n, t)
    freq, psd = scipy.signal.welch(x, fs=1.0 / DT, window=win, nperseg=nperseg, noverlap=noverlap, detrend=detrend, axis=-1)
    f_ref, ref = sc.welch_reference(x, DT, nperseg, noverlap, win, detrend)
    assert np.allclose(freq, f_ref, rtol=1e-14, atol=0)
    dev = float((np.abs(psd - ref).max(1) / np.abs(ref).max(1)).max())
    out.update({f"x{i}": x, f"freq{i}": freq, f"psd{i}": psd, f"tol{i}": np.array(4.0 * dev)})
    print(f"case {i}: N {n} T {t} L {nperseg} noverlap {noverlap} {win} {detrend}: scipy deviates by {dev:.2e} of the row maximum")
np.savez_compressed(os.path.join(HERE, "welch_scipy.npz"), **out)
print("wrote", len(sc.SCIPY_CASES), "cases, scipy", scipy.__version__)
