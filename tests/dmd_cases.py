"""
CPU reference of the dynamic mode decomposition (sparsespatialsampling_amd/dmd.py) and the cases its tests share.  numpy / torch on
the host only.

The reference is the DIRECT route in complex128: ``torch.linalg.svd`` of ``sqrt(a) X``, ``A~ = U^H Y V S^-1``, ``eig``, the modes
``Phi = Y V S^-1 W`` and both amplitude rules from N-sized matrices -- no Gram matrix anywhere, so it does not square the condition
number and shares no code with the package (only the normalisation and the ordering of the eigenpairs are the same: unit
eigenvectors with the largest component real and positive, descending |lambda|, then descending imaginary part).

The cases are synthetic linear dynamics with KNOWN eigenvalues: ``D[:, t] = Re sum_j phi_j b_j lambda_j^t`` over r / 2 modes, which
makes r / 2 conjugate pairs, noise-free and of rank exactly r.
"""
import math

import numpy as np
import torch as pt

EPS = float(np.finfo(np.float64).eps)


# ---- the reference ----------------------------------------------------------------------------------------------------------
def sort_eigenpairs(lam, vec):
    vec = vec / np.linalg.norm(vec, axis=0, keepdims=True)
    pivot = vec[np.abs(vec).argmax(axis=0), np.arange(vec.shape[1])]
    vec = vec * (pivot.conj() / np.abs(pivot))
    order = np.lexsort((-lam.imag, -np.round(np.abs(lam) * 1e9)))
    return lam[order], vec[:, order]


def optimal_rank(s, n_rows, n_cols):
    """Gavish & Donoho's hard threshold for an unknown noise level, as flowtorch documents it"""
    beta = min(n_rows, n_cols) / max(n_rows, n_cols)
    omega = 0.56 * beta ** 3 - 0.95 * beta ** 2 + 1.82 * beta + 1.43
    return max(1, int((s > omega * np.median(s)).sum()))


def reference_dmd(data, dt, rank=None, optimal=False, area=None):
    """``data`` [N, T] or [N, C, T] (any float dtype; taken to float64), ``area`` [N] or None.  Returns a dict of numpy arrays:
    s (all singular values of sqrt(a) X), rank, opt_rank, eigvals, frequency, growth_rate, modes [rows, r] (physical), amplitude,
    dynamics [r, T], reconstruction [rows, T], mode_norm (weighted), integral"""
    d = np.asarray(data, dtype=np.float64)
    n_cells, t = d.shape[0], d.shape[-1]
    d = d.reshape(-1, t)
    sw = np.ones(len(d)) if area is None else np.sqrt(np.repeat(np.asarray(area, dtype=np.float64), len(d) // n_cells))
    xw, yw = d[:, :-1] * sw[:, None], d[:, 1:] * sw[:, None]
    u, s, vh = (a.numpy() for a in pt.linalg.svd(pt.from_numpy(xw), full_matrices=False))
    opt = optimal_rank(s, len(d), t - 1)
    r = min(opt if rank is None else rank, t - 1)
    u, sr, v = u[:, :r], s[:r], vh[:r].T
    a_tilde = u.T @ yw @ (v / sr)
    lam, w = np.linalg.eig(a_tilde)
    lam, w = sort_eigenpairs(lam.astype(np.complex128), w.astype(np.complex128))
    modes_w = (yw @ (v / sr)).astype(np.complex128) @ w
    vander = lam[:, None] ** np.arange(t)[None, :]
    if optimal:
        vm = vander[:, :-1]
        p = (modes_w.conj().T @ modes_w) * (vm @ vm.conj().T).conj()
        q = np.diagonal(vm @ xw.T.astype(np.complex128) @ modes_w).conj()
        b = np.linalg.solve(p, q)
    else:
        b = np.linalg.lstsq(modes_w, (d[:, 0] * sw).astype(np.complex128), rcond=None)[0]
    modes = modes_w / sw[:, None]
    dynamics = b[:, None] * vander
    mode_norm = np.linalg.norm(modes_w, axis=0)
    return dict(s=s, rank=r, opt_rank=opt, eigvals=lam, frequency=np.log(lam).imag / (2 * math.pi * dt), growth_rate=np.log(lam).real / dt,
                modes=modes, amplitude=b, dynamics=dynamics, reconstruction=(modes @ dynamics).real, mode_norm=mode_norm,
                integral=mode_norm * np.abs(dynamics).sum(axis=1), weight_sqrt=sw)


def by_angle(lam):
    """the ordering the tests compare in: by the eigenvalue's angle (the planted frequencies are distinct and well apart, a
    conjugate pair sits at +-theta), which no rounding of |lambda| can permute"""
    return np.argsort(np.angle(np.asarray(lam)), kind="stable")


# ---- the cases --------------------------------------------------------------------------------------------------------------
def layout_stride(t, layout, itemsize):
    """row pitch in elements: 'contiguous'; 'pitch16' = the next multiple of 16 bytes ABOVE the row; 'odd' = an odd number of
    elements (float32: rows on 4-byte boundaries only)"""
    if layout == "contiguous":
        return t
    if layout == "pitch16":
        per = 16 // itemsize
        return (t // per + 1) * per
    if layout == "odd":
        return t + 1 if t % 2 == 0 else t + 2
    raise ValueError(layout)


def with_layout(dense, layout):
    """a torch tensor with the values of ``dense`` [N, T] in the asked-for row layout (a column slice of a wider buffer)"""
    dense = pt.as_tensor(dense)
    n, t = dense.shape
    stride = layout_stride(t, layout, dense.element_size())
    buf = pt.full((n, stride), float("nan"), dtype=dense.dtype)
    buf[:, :t] = dense
    return buf[:, :t]


class Case:
    def __init__(self, name, n, t, r, dtype, layout="contiguous", comps=None, area=False, optimal=False, noise=0.0, seed=0):
        self.name, self.n, self.t, self.r, self.dtype, self.layout = name, n, t, r, dtype, layout
        self.comps, self.with_area, self.optimal, self.noise, self.seed = comps, area, optimal, noise, seed
        self.dt = 0.05
        self._built = None

    def __repr__(self):
        return self.name

    def build(self):
        """dict: data (torch, the case's dtype and layout), area (numpy or None), lam / products (the planted eigenvalues and
        phi_j b_j / 2 of BOTH members of every pair, ordered by angle), truth (planted D, float64, before any rounding to float32),
        ref (reference_dmd of the data as the device sees it), kappa = s_1 / s_r of the reference"""
        if self._built is not None:
            return self._built
        rng = np.random.default_rng(1000 + self.seed)
        rows = self.n * (self.comps or 1)
        pairs = self.r // 2
        theta = 0.25 + 2.3 * (np.arange(pairs) + 0.5 + 0.2 * (rng.random(pairs) - 0.5)) / pairs
        lam = rng.uniform(0.97, 1.0, pairs) * np.exp(1j * theta)
        # random smooth shapes: a few dozen cosines over the row coordinate with mildly decaying complex coefficients
        x = (np.arange(rows) + 0.5) / rows
        m = np.arange(max(2 * self.r, 8))
        basis = np.cos(np.pi * np.outer(x, m) + rng.uniform(0, 2 * np.pi, len(m))[None, :])
        coeff = (rng.standard_normal((len(m), pairs)) + 1j * rng.standard_normal((len(m), pairs))) / (1.0 + m[:, None] / len(m))
        phi = basis @ coeff + 0.3 * (rng.standard_normal((rows, pairs)) + 1j * rng.standard_normal((rows, pairs)))
        b = rng.uniform(1.0, 2.0, pairs) * np.exp(1j * rng.uniform(0, 2 * np.pi, pairs))
        truth = ((phi * b) @ (lam[:, None] ** np.arange(self.t)[None, :])).real
        data = truth
        if self.noise:
            data = truth + self.noise * np.sqrt((truth ** 2).mean()) * rng.standard_normal(truth.shape)
        area = 2.0 ** rng.uniform(-12, 0, self.n) if self.with_area else None
        if area is not None:
            area[0], area[-1] = 2.0 ** -12, 1.0
        tensor = pt.from_numpy(data).to(self.dtype)
        if self.comps:
            tensor = tensor.reshape(self.n, self.comps, self.t).contiguous()
        else:
            tensor = with_layout(tensor, self.layout)
        ref = reference_dmd(tensor.numpy(), self.dt, rank=None if self.noise else self.r, optimal=self.optimal, area=area)
        kappa = float(ref["s"][0] / ref["s"][ref["rank"] - 1])
        assert kappa <= 100.0, f"{self.name}: s_1 / s_r = {kappa:.1f} > 100 -- the 1e-4 rank cap must never bind in these cases"
        lam_all = np.concatenate([lam, lam.conj()])
        prod_all = np.concatenate([0.5 * phi * b, 0.5 * (phi * b).conj()], axis=1)
        order = by_angle(lam_all)
        self._built = dict(data=tensor, area=area, lam=lam_all[order], products=prod_all[:, order], truth=truth, ref=ref, kappa=kappa)
        return self._built


F32, F64 = pt.float32, pt.float64

# the smallest shapes that reach every staging path: N in {1 x 3 components, 15, 17, 257, 3000} (below / across one 16-row step, two
# 128-row GEMM blocks, several Gram slices), T in {3, 17, 33, 130} (below / across a 16-row step of the GEMM's inner dimension and
# one 128-column block; 130 gives three block pairs), r in {2, 6, 40} (2r <= 64: the narrow GEMM, 2r = 80: the wide one), both
# dtypes, the three row layouts (float32: 16-, 8- and 4-byte aligned rows), a vector field, with and without areas
NOISE_FREE = [
    Case("n1x3_t3_r2_f64", 1, 3, 2, F64, comps=3, seed=1),
    Case("n15_t3_r2_f32_area_opt", 15, 3, 2, F32, area=True, optimal=True, seed=2),
    Case("n15_t17_r6_f64_pitch_area_opt", 15, 17, 6, F64, "pitch16", area=True, optimal=True, seed=3),
    Case("n17_t17_r6_f32_pitch", 17, 17, 6, F32, "pitch16", seed=4),
    Case("n17_t33_r6_f32_odd_area", 17, 33, 6, F32, "odd", area=True, seed=5),
    Case("n257_t33_r6_f64_area_opt", 257, 33, 6, F64, area=True, optimal=True, seed=6),
    Case("n257_t130_r40_f32_odd_area_opt", 257, 130, 40, F32, "odd", area=True, optimal=True, seed=7),
    Case("n3000_t130_r40_f32", 3000, 130, 40, F32, seed=8),
    Case("n3000_t130_r40_f64_pitch_area_opt", 3000, 130, 40, F64, "pitch16", area=True, optimal=True, seed=9),
    Case("n3000_t130_r6_f32_pitch_area_opt", 3000, 130, 6, F32, "pitch16", area=True, optimal=True, seed=10),
    Case("n257x3_t33_r6_f32_area", 257, 33, 6, F32, comps=3, area=True, seed=11),
    Case("n3000_t17_r2_f32", 3000, 17, 2, F32, seed=12),
    Case("n257_t130_r6_f64_odd", 257, 130, 6, F64, "odd", seed=13),
]
NOISY = Case("n3000_t33_r6_f64_noise_area", 3000, 33, 6, F64, area=True, noise=1e-3, seed=20)


def rel_max(got, want):
    """max |got - want| / max |want|"""
    want = np.asarray(want)
    return float(np.abs(np.asarray(got) - want).max() / np.abs(want).max())
