"""
Cases, long-double reference and per-row bounds for the temporal moment kernels (s3_row_moments / s3_row_abs_moments,
sparsespatialsampling_amd/csrc/metric.hip), shared by tests/test_moments_checker.py (CPU) and tests/test_gpu_moments.py.  numpy only.

The reference, per row of T values, in ``np.longdouble``: ``m = sum x / T`` and ``M2 = sum (x - m)^2`` (of |x| for the abs entry point).

The bounds (eps = 2^-53, every quantity taken from the reference, none from the result under test):

* mean: ``|m_got - m| <= b_m = (T + 2) eps sum|x| / T``.  Any summation of T values in float64 that adds each value once is within
  ``(T - 1) eps sum|x|`` of the exact sum whatever its order; the chunk means' divisions and Chan's weighted merges add a few more
  roundings of quantities bounded by ``sum|x| / T`` -- a float64 emulation of the kernel's scheme measures 0.28 of the bound at
  most (test_moments_checker.py), the kernel itself 0.33 (test_gpu_moments.py).
* M2: with ``M2_got = std_got^2 (T - ddof)`` formed in long double,
  ``|M2_got - M2| <= (T + 8) eps M2 + 8 eps max|x| sum|x - m| + T b_m^2``.  The first term is the summation of T non-negative squares plus
  the square root, its square and the division by ``T - ddof``; the second the rounding of ``x - m'`` (an error of up to
  ``eps max|x|`` per deviation, entering the square twice, with room for the merges' ``delta^2`` terms); the third what a mean off by
  ``b_m`` adds to a sum of squared deviations taken about it (``sum (x - m')^2 = M2 + T (m - m')^2``).  A one-pass ``sum x^2 - T m^2``
  is off by about ``T eps m^2``: a factor ``m^2 / (max|x| sigma)`` ~ 10^6 beyond the bound for pressure-like data.
"""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53
KINDS = ("benign", "ill", "tiny", "outlier")


# ---- the kernel's dispatch, mirrored (csrc/metric.hip: row_moments_impl, launch_moments) ---------------------------------------
def kernel_vec(itemsize, stride, address):
    """elements per load the entry point chooses for rows ``stride`` elements apart starting at byte ``address``"""
    if itemsize == 4:
        if stride % 4 == 0 and address % 16 == 0:
            return 4
        return 2 if stride % 2 == 0 and address % 8 == 0 else 1
    return 2 if stride % 2 == 0 and address % 16 == 0 else 1


def lanes_per_row(n_vec):
    """(G, per_lane) of launch_moments for a row of ``n_vec`` whole vectors"""
    per_lane = 16 if n_vec >= 128 else 8
    for g in (64, 32, 16, 8):
        if n_vec > (g // 2) * per_lane:
            return g, per_lane
    return 4, per_lane


# ---- shapes ------------------------------------------------------------------------------------------------------------------------
# G follows from n_vec, so "n_vec in {1, 4G - 1, 4G, 4G + 1, 8G + 1} at each G" is the union below: one vector, every chunk size
# 4G = 16 .. 256 minus / plus one (the neighbours fall into the next G or the next chunk), the thresholds of launch_moments (32, 64, 128,
# 256, 512 and the per_lane switch at 128, which sends n_vec = 128 alone to G = 8 with 16 vectors per lane), and rows of three to five
# chunks at G = 32 and 64.  n_vec = 0 is a row shorter than one vector (tail only).
N_VECS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 384, 512, 513, 640, 768, 1025)
MANY_ROWS = 260


def row_counts(g):
    """one row, a workgroup of 256 / G rows less one / plus one (dead rows beside live ones), a few hundred"""
    return (1, max(1, 256 // g - 1), 256 // g + 1, MANY_ROWS)


class Shape:
    def __init__(self, vec, n_vec, n_tail, n_rows, index):
        self.vec, self.n_vec, self.n_tail, self.n_rows, self.index = vec, n_vec, n_tail, n_rows, index
        self.row_len = n_vec * vec + n_tail
        self.g, self.per_lane = lanes_per_row(n_vec)
        self.chunks = max(1, -(-n_vec // (4 * self.g)))

    def __repr__(self):
        return f"vec{self.vec}_nvec{self.n_vec}_tail{self.n_tail}_rows{self.n_rows}"


def shapes(vec):
    """every n_vec of N_VECS with every ragged tail 0 .. vec - 1; the row count cycles through row_counts(G) so that each G sees each"""
    out, seen = [], {}
    for n_vec in N_VECS:
        for n_tail in range(vec):
            if n_vec == 0 and n_tail == 0:
                continue
            g = lanes_per_row(n_vec)[0]
            out.append(Shape(vec, n_vec, n_tail, row_counts(g)[seen.get(g, 0) % 4], len(out)))
            seen[g] = seen.get(g, 0) + 1
    return out


# ---- layouts ---------------------------------------------------------------------------------------------------------------------
# name -> (stride(row_len), offset in elements); which vector width each gives: LAYOUTS
def _next(t, modulus, residue):
    """smallest s > t with s % modulus == residue"""
    s = t + 1
    while s % modulus != residue:
        s += 1
    return s


def layout(name, row_len, itemsize):
    """(row pitch, offset of the first row into its buffer), both in elements"""
    per16 = 16 // itemsize
    if name == "contiguous":
        return row_len, 0
    if name == "pitch16":                                    # rows 16-byte aligned, at least one element of padding
        return _next(row_len, per16, 0), 0
    if name == "pitch8":                                     # float32 rows 8- but not 16-byte aligned
        return _next(row_len, 4, 2), 0
    if name == "pitch16_off2":                               # float32: pitch of 16 bytes, the base 8 bytes into a 16-byte line
        return _next(row_len, 4, 0), 2
    if name == "odd":
        return _next(row_len, 2, 1), 0
    if name == "offset1":                                    # pitch of 16 bytes, the base one element off
        return _next(row_len, per16, 0), 1
    raise ValueError(name)


# (itemsize, vec) -> layouts that make the entry point choose that width ("contiguous" only for the row lengths that allow it)
LAYOUTS = {
    (4, 4): ("contiguous", "pitch16"),
    (4, 2): ("contiguous", "pitch8", "pitch16_off2"),
    (4, 1): ("contiguous", "odd", "offset1"),
    (8, 2): ("contiguous", "pitch16"),
    (8, 1): ("contiguous", "odd", "offset1"),
}


def layout_fits(name, row_len, itemsize, vec):
    """does this layout, on a buffer aligned to 256 bytes, give vector width ``vec`` for rows of ``row_len``"""
    stride, offset = layout(name, row_len, itemsize)
    return kernel_vec(itemsize, stride, offset * itemsize) == vec


# ---- data --------------------------------------------------------------------------------------------------------------------------
def make_rows(n_rows, t, dtype, seed, first_kind=0):
    """[n_rows, t] of ``dtype``; row r is of kind KINDS[(r + first_kind) % 4]:
    benign: 3 N(0,1) about a row offset in [-5, 5] (both signs); ill: float32 101325 + 0.05 N(0,1), float64 1e6 + 1e-4 N(0,1);
    tiny: 1e-30 N(0,1); outlier: N(0,1) with one value of 1e8"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n_rows, t))
    x = np.empty((n_rows, t), dtype=np.float64)
    kind = (np.arange(n_rows) + first_kind) % 4
    f32 = np.dtype(dtype) == np.float32
    for r in range(n_rows):
        if kind[r] == 0:
            x[r] = 3.0 * z[r] + rng.uniform(-5.0, 5.0)
        elif kind[r] == 1:
            x[r] = 101325.0 + 0.05 * z[r] if f32 else 1e6 + 1e-4 * z[r]
        elif kind[r] == 2:
            x[r] = 1e-30 * z[r]
        else:
            x[r] = z[r]
            x[r, rng.integers(t)] = 1e8
    return x.astype(dtype)


# ---- reference, bounds, checker ------------------------------------------------------------------------------------------------
def reference(x, absolute=False):
    """long-double moments of every row of ``x`` [n, T] (of |x| with ``absolute``) and the sums the bounds are made of"""
    xl = np.asarray(x).astype(LD)
    if absolute:
        xl = np.abs(xl)
    t = xl.shape[1]
    m = xl.sum(axis=1) / LD(t)
    dev = xl - m[:, None]
    return dict(t=t, m=m, m2=(dev * dev).sum(axis=1), sum_abs=np.abs(xl).sum(axis=1), max_abs=np.abs(xl).max(axis=1),
                sum_dev=np.abs(dev).sum(axis=1))


def mean_bound(ref, t=None):
    t = ref["t"] if t is None else t
    return LD(t + 2) * LD(EPS) * ref["sum_abs"] / LD(t)


def m2_bound(ref):
    t, b_m = ref["t"], mean_bound(ref)
    return LD(t + 8) * LD(EPS) * ref["m2"] + LD(8) * LD(EPS) * ref["max_abs"] * ref["sum_dev"] + LD(t) * b_m * b_m


def _ratio(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(r), np.inf, r).astype(np.float64)


def mean_ratio(mean_got, ref):
    """|m_got - m| / b_m per row (0 where both are 0, inf where the result is not a number)"""
    return _ratio(np.abs(np.asarray(mean_got, dtype=np.float64).astype(LD) - ref["m"]), mean_bound(ref))


def m2_ratio(std_got, ref, ddof):
    """|std_got^2 (T - ddof) - M2| / bound per row; T - ddof = 0: 0 where the result is NaN (the only right answer), inf elsewhere"""
    std_got = np.asarray(std_got, dtype=np.float64)
    dof = ref["t"] - ddof
    if dof <= 0:
        return np.where(np.isnan(std_got), 0.0, np.inf)
    s = std_got.astype(LD)
    bad_sign = std_got < 0
    return np.where(bad_sign, np.inf, _ratio(np.abs(s * s * LD(dof) - ref["m2"]), m2_bound(ref)))


def assert_moments(mean_got, std_got, ref, ddof, what=""):
    """-> (worst mean ratio, worst M2 ratio); either output may be None"""
    worst = [0.0, 0.0]
    if mean_got is not None:
        r = mean_ratio(mean_got, ref)
        worst[0] = float(r.max())
        assert worst[0] <= 1.0, f"{what}: mean off the long-double reference, row {int(r.argmax())}: {worst[0]:.3g} of the bound"
    if std_got is not None:
        r = m2_ratio(std_got, ref, ddof)
        worst[1] = float(r.max())
        assert worst[1] <= 1.0, f"{what}: M2 off the long-double reference, row {int(r.argmax())}: {worst[1]:.3g} of the bound"
    return tuple(worst)


# ---- float64 emulation of the kernel's scheme, and the mistakes the checker has to catch --------------------------------------------
def _merge(a, b):
    if b[0] == 0.0:
        return a
    if a[0] == 0.0:
        return b
    n, delta = a[0] + b[0], b[1] - a[1]
    return n, a[1] + delta * (b[0] / n), a[2] + b[2] + delta * delta * (a[0] * b[0] / n)


def _butterfly(v):
    off = len(v) // 2
    lanes = np.arange(len(v))
    while off > 0:
        v = v + v[lanes ^ off]
        off //= 2
    return v[0]


def emulate(row, vec, g=None, absolute=False, mistake=None):
    """(mean, M2, n) of one row as row_moments_kernel<T, vec, g> forms them, operation by operation in float64: lanes of strided
    vectors, chunk sum -> chunk mean -> squared deviations, xor-butterflies, Chan's merge.  ``mistake``: "wrong_counts" merges every
    chunk as if it were full; "drop_last" stops one element short of the row; "one_pass" is ``sum x^2 - T m^2`` on the same sums"""
    x = np.asarray(row).astype(np.float64)
    if absolute:
        x = np.abs(x)
    if mistake == "drop_last":
        x = x[:-1]
    t = len(x)
    if mistake == "one_pass":
        s, ss = float(np.sum(x)), float(np.sum(x * x))
        m = s / t
        return m, ss - t * m * m, float(t)
    n_vec = t // vec
    tail0 = n_vec * vec
    n_tail = t - tail0
    if g is None:
        g = lanes_per_row(n_vec)[0]
    xp = np.concatenate([x, np.zeros(vec)])
    acc = (0.0, 0.0, 0.0)
    base = 0
    while base < n_vec or (base == 0 and n_tail > 0):
        v = base + np.arange(g)[None, :] + g * np.arange(4)[:, None]
        ok = v < n_vec
        vals = xp[(np.where(ok, v, 0) * vec)[:, :, None] + np.arange(vec)[None, None, :]]
        last = base + 4 * g >= n_vec
        s = np.zeros(g)
        for u in range(4):
            for i in range(vec):
                s = s + np.where(ok[u], vals[u, :, i], 0.0)
        if last:
            for i in range(n_tail):
                s[0] = s[0] + x[tail0 + i]
        n_chunk = float(max(0, min(4 * g, n_vec - base)) * vec + (n_tail if last else 0))
        m = _butterfly(s) / n_chunk
        q = np.zeros(g)
        for u in range(4):
            for i in range(vec):
                d = vals[u, :, i] - m
                q = q + np.where(ok[u], d * d, 0.0)
        if last:
            for i in range(n_tail):
                d = x[tail0 + i] - m
                q[0] = q[0] + d * d
        acc = _merge(acc, (float(4 * g * vec) if mistake == "wrong_counts" else n_chunk, float(m), float(_butterfly(q))))
        base += 4 * g
    return acc[1], acc[2], acc[0]


def emulated_outputs(rows, vec, ddof, **kwargs):
    """(mean [n], std [n]) the kernel would write for ``rows`` [n, T]"""
    mean, std = np.empty(len(rows)), np.empty(len(rows))
    for r, row in enumerate(rows):
        m, m2, n = emulate(row, vec, **kwargs)
        mean[r] = m
        with np.errstate(invalid="ignore"):
            std[r] = np.sqrt(np.float64(m2) / (n - ddof)) if n - ddof > 0 else np.nan
    return mean, std
