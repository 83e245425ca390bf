"""
Dynamic mode decomposition of a field on the S^3 grid or on the original CFD mesh -- the third analysis the reference's workflow
ends in, ``post_processing/compare_dmd_OAT.py:150-178``: ``DMD(field * sqrt(area), dt, optimal=True)`` of the original and of the
interpolated field, then ``top_modes(integral=True)``, ``eigvals``, ``modes``, ``reconstruction`` and ``svd.opt_rank``.  The
reference takes the class from flowtorch (absent here); this one is restated from the papers -- exact DMD after Tu et al. 2014,
optimal amplitudes after Jovanovic et al. 2014 -- and not pinned against flowtorch, like ``svd.optimal_rank``.

How it runs on the MI355X (method of snapshots throughout; D [N, T] the data, a the cell areas, X = D[:, :-1], Y = D[:, 1:]):

1. ONE Gram matrix ``G = D^T diag(a) D`` [T, T] over all T columns -- ``s3_gram`` on the f64 matrix cores (csrc/svd.hip), no
   mean (DMD does not centre).  D is read where it lies, float32 or float64, rows possibly pitched: a float32 element is widened
   in the kernel's operand staging, no float64 copy of the matrix exists (the original field of the 3-D cylinder is 20 GB in
   float32).  ``G_XX = G[:-1, :-1]``, ``G_XY = G[:-1, 1:]``, ``G_YY = G[1:, 1:]`` are slices of the SMALL matrix: no
   column-shifted window of D is handed to a kernel.
2. ``G_XX = V S^2 V^T`` -- ``svd._eigh`` (the vendor's dense symmetric solver behind ``s3_sym_eig``).
3. Everything r x r on the host, from the Gram blocks alone (``_small_problem``): the projected operator
   ``A~ = S^-1 V^T G_XY V S^-1``, its eigenpairs (``torch.linalg.eig``), ``B = V S^-1 W`` and both amplitude rules.
4. Modes ``Phi = Y B = D [0; B]`` -- ONE real ``s3_tall_gemm`` against the [T, 2r] matrix whose columns 2j, 2j + 1 are Re and Im
   of column j; the [N, 2r] float64 result IS the complex128 [N, r] matrix (``view_as_complex``).  The weights cancel as in
   ``compute_svd``: modes and reconstruction are physical, not scaled by sqrt(area).
5. ``reconstruction`` / ``partial_reconstruction``: one ``s3_tall_gemm`` of the mode matrix against [2r, t1 - t0].

Deviation from a direct SVD: the rank is capped at the number of singular values >= ``RANK_RANGE`` (1e-4) of the largest one,
with a logged warning when the cap binds.  An eigenvalue of the Gram matrix carries an absolute error of about eps * s_1^2; below
that range 1 / s_j is noise, and the deflation that ``compute_svd`` refines its spectrum with is float64-only.
"""
import logging
import math
from types import SimpleNamespace

import numpy as np
import torch as pt

from . import hipops
from .arrays import Side, resident_matrix
from .svd import _eigh, optimal_rank

log = logging.getLogger(__name__)

RANK_RANGE = 1e-4           # singular values below this fraction of the largest one are not inverted (module docstring)


def _check_arguments(data_matrix, dt, rank, cell_area, who="DMD", min_snapshots=3):
    """argument errors, raised before any device call; returns (n_cells, n_comp or None, T)"""
    if not isinstance(data_matrix, pt.Tensor):
        raise TypeError(f"data_matrix must be a torch tensor, got {type(data_matrix).__name__}")
    shape = tuple(data_matrix.shape)
    if len(shape) not in (2, 3):
        raise ValueError(f"expected [N_cells, N_snapshots] or [N_cells, N_dims, N_snapshots], got {shape}")
    if data_matrix.dtype not in hipops.DTYPE_CODE:
        raise TypeError(f"data_matrix must be float32 or float64, got {data_matrix.dtype}")
    n_cells, t = shape[0], shape[-1]
    if t < min_snapshots:
        raise ValueError(f"{who} needs at least {min_snapshots} snapshots, got {t}")
    if n_cells < 1 or (len(shape) == 3 and shape[1] < 1):
        raise ValueError(f"the data matrix has no rows: {shape}")
    if data_matrix.stride(-1) != 1:
        raise ValueError(f"the snapshots of a row must be adjacent in memory (inner stride 1), got stride {data_matrix.stride(-1)}")
    if len(shape) == 3 and not data_matrix.is_contiguous():
        raise ValueError("a vector field [N_cells, N_dims, N_snapshots] must be contiguous (only a 2-D matrix may have a row pitch)")
    if len(shape) == 2 and data_matrix.stride(0) < t:
        raise ValueError(f"rows overlap: row stride {data_matrix.stride(0)} < {t} snapshots")
    try:
        dt_ok = float(dt) > 0 and math.isfinite(float(dt))
    except (TypeError, ValueError):
        dt_ok = False
    if not dt_ok:
        raise ValueError(f"dt must be a positive number, got {dt}")
    if rank is not None and int(rank) < 1:
        raise ValueError(f"rank must be positive, got {rank}")
    if cell_area is not None and int(np.prod(tuple(cell_area.shape))) != n_cells:
        raise ValueError(f"cell_area must hold one value per cell ({n_cells}), got {tuple(cell_area.shape)}")
    return n_cells, (shape[1] if len(shape) == 3 else None), t


def sort_eigenpairs(lam, vec):
    """eigenvectors (columns) to unit 2-norm with the largest component real and positive; eigenpairs by descending |lambda|, then
    descending imaginary part (|lambda| compared to 1e-9: the two members of a conjugate pair tie)"""
    vec = vec / pt.linalg.vector_norm(vec, dim=0, keepdim=True)
    top = vec.abs().argmax(dim=0)
    pivot = vec[top, pt.arange(vec.shape[1])]
    vec = vec * (pivot.conj() / pivot.abs())
    key_abs = np.round(lam.abs().numpy() * 1e9)
    order = pt.from_numpy(np.lexsort((-lam.imag.numpy(), -key_abs)).copy())
    return lam[order], vec[:, order]


def _small_problem(gram, s, v, dt, optimal):
    """everything of the DMD that is small, from the Gram matrix ``gram`` [T, T] of ALL snapshots and the leading r singular values
    ``s`` / right singular vectors ``v`` [T - 1, r] of X (float64, host).  Returns a dict of host tensors:

    ``eigvals`` [r], ``eigvecs`` [r, r], ``b_matrix`` B = V S^-1 W [T - 1, r], ``mode_gram`` Phi^H diag(a) Phi = B^H G_YY B [r, r],
    ``amplitude`` [r] (plain: the weighted least-squares fit of the first snapshot, (B^H G_YY B) b = B^H G[1:, 0]; optimal:
    ``P = (B^H G_YY B) o conj(Vand Vand^H)``, ``q = conj(diag(Vand G_XY B))``, ``b = P^-1 q`` with Vand[j, t] = lambda_j^t, t < T - 1)
    and ``vander`` [r, T] (all T columns)."""
    t = int(gram.shape[0])
    g_xy, g_yy = gram[:-1, 1:], gram[1:, 1:]
    vs = v / s                                                              # V S^-1  [T - 1, r]
    a_tilde = vs.T @ g_xy @ vs
    lam, w = pt.linalg.eig(a_tilde)
    lam, w = sort_eigenpairs(lam, w)
    b_matrix = vs.to(pt.complex128) @ w
    mode_gram = b_matrix.conj().T @ g_yy.to(pt.complex128) @ b_matrix
    mode_gram = 0.5 * (mode_gram + mode_gram.conj().T)
    vander = lam.reshape(-1, 1) ** pt.arange(t, dtype=pt.float64).reshape(1, -1)      # [r, T]
    if optimal:
        vm = vander[:, :t - 1]
        p = mode_gram * (vm @ vm.conj().T).conj()
        q = pt.diagonal(vm @ g_xy.to(pt.complex128) @ b_matrix).conj()
        amplitude = pt.linalg.solve(p, q)
    else:
        amplitude = pt.linalg.solve(mode_gram, b_matrix.conj().T @ gram[1:, 0].to(pt.complex128))
    return {"eigvals": lam, "eigvecs": w, "b_matrix": b_matrix, "mode_gram": mode_gram, "amplitude": amplitude, "vander": vander}


def _coefficients(b_matrix, dynamics):
    """M [T, n_t] real with ``reconstruction = D M``: Re([0; B] dynamics)"""
    m = pt.zeros((b_matrix.shape[0] + 1, dynamics.shape[1]), dtype=pt.float64)
    m[1:] = (b_matrix @ dynamics).real
    return m


def _error_from_gram(gram, coeff):
    """relative weighted L2 error per snapshot from the Gram matrix alone: sqrt((e_t - m_t)^T G (e_t - m_t) / G_tt), ``coeff`` [T, T]
    the coefficient columns m_t.  Returns (error [T], squared residual norms [T])"""
    r = pt.eye(gram.shape[0], dtype=pt.float64) - coeff
    sq = ((gram @ r) * r).sum(0)
    return (sq.clamp_min(0.0) / pt.diagonal(gram)).sqrt(), sq


def _interleave(z):
    """complex [k, r] -> real [k, 2r]: columns 2j, 2j + 1 are Re and Im of column j"""
    return pt.view_as_real(z.contiguous()).reshape(z.shape[0], -1).contiguous()


class DMD:
    """Exact dynamic mode decomposition of ``data_matrix`` [N_cells, N_snapshots] or [N_cells, N_dims, N_snapshots] (components stacked
    as ``compute_svd`` does), float32 or float64, host or device; the rows of a 2-D matrix may be pitched (unit inner stride).  The
    input is neither modified nor copied in another dtype.  ``dt``: time between two snapshots; ``rank``: number of modes
    (None: the optimal hard threshold, ``svd.optimal_rank``); ``optimal``: optimal amplitudes (Jovanovic et al.) instead of the fit
    of the first snapshot; ``cell_area`` [N_cells]: weights of the inner product (None: 1).  The reference's script multiplies the
    field by sqrt(area) and divides it out of the modes again; here the weights enter the Gram matrix and cancel in the modes.

    Members (on the side -- host / device -- the data came from): ``eigvals`` [r], ``eigvecs`` [r, r], ``modes`` [N_cells, (N_dims,) r]
    complex128, ``amplitude`` [r], ``frequency`` = Im log(lambda) / (2 pi dt), ``growth_rate`` = Re log(lambda) / dt, ``dynamics``
    [r, T] = diag(b) Vand, ``svd.s``, ``svd.V`` (of X, weighted), ``svd.rank``, ``svd.opt_rank``; ``top_modes``, ``reconstruction``,
    ``partial_reconstruction``, ``reconstruction_error``."""

    def __init__(self, data_matrix, dt, rank=None, optimal=False, cell_area=None):
        n_cells, n_comp, t = _check_arguments(data_matrix, dt, rank, cell_area)
        self.dt, self.optimal = float(dt), bool(optimal)
        self._side = Side(data_matrix)
        self._shape = tuple(data_matrix.shape)
        d2 = resident_matrix(data_matrix, n_cells, n_comp, t)               # read where it lies, or uploaded in its own dtype
        weight = None
        if cell_area is not None:
            weight = hipops.to_device(cell_area, pt.float64).reshape(-1)
            if n_comp is not None:
                weight = weight.repeat_interleave(n_comp)                     # row (n, c) keeps the area of cell n
        n_rows = int(d2.shape[0])

        gram_dev = hipops.gram(d2, None, weight)                              # (its scratch is released on return)
        del weight
        lam, vec = _eigh(gram_dev[:-1, :-1].contiguous())                     # ascending, host
        gram = pt.from_numpy(hipops.to_host(gram_dev))
        del gram_dev
        s_all = lam.flip(0).clamp_min(0.0).sqrt()
        vec = vec.flip(1)
        opt_rank = optimal_rank(s_all, n_rows, t - 1)
        r = min(opt_rank if rank is None else int(rank), t - 1)
        usable = max(1, int((s_all >= RANK_RANGE * s_all[0]).sum())) if float(s_all[0]) > 0 else 0
        if usable == 0:
            raise ValueError("the data matrix is zero")
        if r > usable:
            log.warning(f"DMD: rank {r} reaches below {RANK_RANGE:g} of the largest singular value, where the Gram matrix resolves "
                        f"nothing; {usable} modes are kept.")
            r = usable
        self.svd = SimpleNamespace(s=self._side.back(s_all[:r].clone()), V=self._side.back(vec[:, :r].contiguous()), rank=r, opt_rank=opt_rank)
        small = _small_problem(gram, s_all[:r], vec[:, :r], self.dt, self.optimal)
        self._gram, self._small = gram, small
        lam_c, b = small["eigvals"], small["amplitude"]
        self._dynamics = b.reshape(-1, 1) * small["vander"]                   # [r, T] host
        self._mode_norm = pt.diagonal(small["mode_gram"]).real.clamp_min(0.0).sqrt()
        log_lam = pt.log(lam_c)
        self._frequency, self._growth = log_lam.imag / (2.0 * math.pi * self.dt), log_lam.real / self.dt

        # Phi = D [0; B]: one real GEMM against [T, 2r]; the result is the complex matrix
        rhs = pt.zeros((t, 2 * r), dtype=pt.float64)
        rhs[1:] = _interleave(small["b_matrix"])
        self._modes2 = hipops.tall_gemm(d2, hipops.to_device(rhs))            # [N_rows, 2r] f64 on the device
        hipops.synchronize()                                                  # (the caller's matrix is not kept alive)

    # ---- small members ----
    @property
    def eigvals(self):
        return self._side.back(self._small["eigvals"])

    @property
    def eigvecs(self):
        return self._side.back(self._small["eigvecs"])

    @property
    def amplitude(self):
        return self._side.back(self._small["amplitude"])

    @property
    def frequency(self):
        return self._side.back(self._frequency)

    @property
    def growth_rate(self):
        return self._side.back(self._growth)

    @property
    def dynamics(self):
        return self._side.back(self._dynamics)

    @property
    def integral_contribution(self):
        """``||phi_j||_a * sum_t |b_j lambda_j^t|`` (the weighted mode norm from diag(B^H G_YY B))"""
        return self._side.back(self._mode_norm * self._dynamics.abs().sum(1))

    @property
    def modes(self):
        """[N_cells, (N_dims,) r] complex128: a view of the [N, 2r] float64 GEMM result"""
        r = self.svd.rank
        z = pt.view_as_complex(self._modes2.reshape(-1, r, 2))
        z = z.reshape(self._shape[:-1] + (r,))
        return self._side.back(z)

    def top_modes(self, n=None, integral=False, f_min=-math.inf, f_max=math.inf):
        """indices of the modes with ``f_min <= frequency < f_max``, ordered by descending |b_j| or (``integral``) by descending
        integral contribution; the first ``n`` of them (None: all).  Ties keep the order of the eigenvalues."""
        importance = (self._mode_norm * self._dynamics.abs().sum(1)) if integral else self._small["amplitude"].abs()
        inside = pt.nonzero((self._frequency >= f_min) & (self._frequency < f_max)).reshape(-1)
        order = inside[pt.argsort(importance[inside], descending=True, stable=True)]
        if n is not None:
            if int(n) < 0:
                raise ValueError(f"n must not be negative, got {n}")
            order = order[:int(n)]
        return self._side.back(order)

    # ---- N-sized members ----
    def _window(self, t0, t1):
        t = self._shape[-1]
        t1 = t if t1 is None else int(t1)
        t0 = int(t0)
        if not 0 <= t0 < t1 <= t:
            raise ValueError(f"expected 0 <= t0 < t1 <= {t}, got t0 = {t0}, t1 = {t1}")
        return t0, t1

    def _reconstruct(self, dynamics):
        # Re(Phi C) = Re Phi Re C - Im Phi Im C: rows 2j, 2j + 1 of the right-hand side are Re C_j and -Im C_j
        rhs = _interleave(dynamics.conj().T).T.contiguous()                   # [2r, n_t]
        out = hipops.tall_gemm(self._modes2, hipops.to_device(rhs))
        out = out.reshape(self._shape[:-1] + (dynamics.shape[1],))
        return self._side.back(out)

    def reconstruction(self, t0=0, t1=None):
        """``Re(Phi diag(b) Vand[:, t0:t1])``: real float64 [N_cells, (N_dims,) t1 - t0].  Nothing of size N x T exists unless all
        of T is asked for."""
        t0, t1 = self._window(t0, t1)
        return self._reconstruct(self._dynamics[:, t0:t1])

    def partial_reconstruction(self, mode_indices, t0=0, t1=None):
        """the same for a subset of the modes (the other rows of the dynamics are zero)"""
        t0, t1 = self._window(t0, t1)
        idx = pt.as_tensor(mode_indices, dtype=pt.int64).reshape(-1).cpu()
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.svd.rank):
            raise ValueError(f"mode indices must lie in [0, {self.svd.rank})")
        dyn = pt.zeros_like(self._dynamics[:, t0:t1])
        dyn[idx] = self._dynamics[idx, t0:t1]
        return self._reconstruct(dyn)

    @property
    def reconstruction_error(self):
        """relative weighted L2 error of the reconstruction per snapshot [T], ``||d_t - rec_t||_a / ||d_t||_a``, from the Gram matrix
        alone: with rec_t = D m_t it is sqrt((e_t - m_t)^T G (e_t - m_t) / G_tt) and touches no N-sized data.  Cancellation floor:
        the squared residual norm is the difference of terms of the size of G_tt and good to about 64 T eps G_tt only, so a
        relative error below about 1e-6 is not resolved (a materialised residual is, when it matters)."""
        err, _ = _error_from_gram(self._gram, _coefficients(self._small["b_matrix"], self._dynamics))
        return self._side.back(err)
