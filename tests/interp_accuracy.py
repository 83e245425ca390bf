"""
Per-element judgement of an interpolation result ``out[c, j] = sum_m w[c, m] * x[idx[c, m], j]`` (reference export.py:467:
``(weights[..., None, None] * data[idx]).sum(1)``) against a long-double reference.  Used by the GPU accuracy tests of every
interpolation route and by the CPU tests of the checker itself; numpy only.

Bound: a sum of k products formed with f64 FMAs in ANY order is within ``(k + 2) * 2**-53 * sum_m |w_m x_m|`` of the exact
value (plus ``k * 2**-1074`` where f64 products reach the subnormal range), so a kernel that reorders its sum passes and one
that accumulates in f32, drops a subnormal, reads the wrong column or skips a term does not.  Non-finite values follow the
reference's IEEE semantics: ``0 * Inf`` and ``0 * NaN`` are NaN, so a NaN neighbour poisons its cell even where its weight is 0.
"""
import numpy as np

LD = np.longdouble
# a 64-bit significand (x86 extended precision): the reference's own rounding is 2**-11 of the bound
assert np.finfo(LD).nmant >= 63, "the accuracy reference needs an extended-precision long double"

U = 2.0 ** -53
F64_TINY = 2.0 ** -1074

# a signalling NaN with a payload: what the guard zones around an output hold, compared BIT for bit afterwards
GUARD_BITS = np.int64(0xFFF4_5A5A_F2F2_FFFF - (1 << 64))       # sign set, quiet bit clear, payload != 0
assert np.isnan(np.array([GUARD_BITS]).view(np.float64)[0])

NAN, POS, NEG, FIN = 1, 2, 3, 0


def classes(a):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf (elementwise)"""
    a = np.asarray(a)
    c = np.zeros(a.shape, dtype=np.int8)
    c[np.isnan(a)] = NAN
    c[np.isposinf(a)] = POS
    c[np.isneginf(a)] = NEG
    return c


def reference(w, idx, x, cells=None, cols=None, budget=1 << 22):
    """(ref, mag) in long double: ref[i, j] = sum_m w[c, m] x[idx[c, m], cols[j]] and mag = sum_m |w x| for c = cells[i].
    ``x`` [n_src, row_len] (f32 / f64), ``w`` f64 [nc, k], ``idx`` int [nc, k]; computed in chunks of cells."""
    w = np.asarray(w, dtype=np.float64)
    idx = np.asarray(idx)
    cells = np.arange(w.shape[0]) if cells is None else np.asarray(cells)
    cols = np.arange(x.shape[1]) if cols is None else np.asarray(cols)
    k = w.shape[1]
    ref = np.empty((len(cells), len(cols)), dtype=LD)
    mag = np.empty((len(cells), len(cols)), dtype=LD)
    step = max(1, budget // max(1, k * len(cols)))
    xc = np.asarray(x)[:, cols]
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, len(cells), step):
            c = cells[a:a + step]
            xs = xc[idx[c]].astype(LD)                                      # [n, k, ncols]
            prod = w[c].astype(LD)[:, :, None] * xs
            ref[a:a + step] = prod.sum(axis=1)
            mag[a:a + step] = np.abs(prod).sum(axis=1)
    return ref, mag


def violations(got, ref, mag, k, f64_data=False):
    """boolean mask of the elements of ``got`` that break the contract: a different NaN / +Inf / -Inf class than the
    reference, or a finite value outside the bound"""
    got = np.asarray(got, dtype=np.float64)
    cg, cr = classes(got), classes(ref)
    tol = LD(k + 2) * LD(U) * mag + (LD(k * F64_TINY) if f64_data else LD(0))
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(got.astype(LD) - ref)
        bad = (cg != cr) | ((cr == FIN) & ~(err <= tol))
    return bad


def assert_close(got, ref, mag, k, f64_data=False, what="", cells=None, cols=None):
    bad = violations(got, ref, mag, k, f64_data)
    if bad.any():
        i, j = np.nonzero(bad)
        rows = []
        for a, b in list(zip(i, j))[:6]:
            c = a if cells is None else cells[a]
            col = b if cols is None else cols[b]
            rows.append(f"cell {c} col {col}: got {float(got[a, b])!r} ref {float(ref[a, b])!r} sum|wx| {float(mag[a, b])!r}")
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements off the long-double reference\n  " + "\n  ".join(rows))


def guard_intact(bits, lo, hi):
    """``bits`` int64 view of the whole output allocation; [lo, hi) is the output: everything else still holds GUARD_BITS"""
    bits = np.asarray(bits)
    return bool((bits[:lo] == GUARD_BITS).all() and (bits[hi:] == GUARD_BITS).all())


def assert_guard(bits, lo, hi, what=""):
    bits = np.asarray(bits)
    outside = np.concatenate([np.nonzero(bits[:lo] != GUARD_BITS)[0], hi + np.nonzero(bits[hi:] != GUARD_BITS)[0]])
    assert outside.size == 0, f"{what}: {outside.size} guard elements changed, first at {outside[:4] - lo} relative to the output"
