"""
Spatial derivatives of fields on a point cloud -- the cell centres of a generated grid or the points of the original CFD mesh:
gradient, gradient magnitude (numerical schlieren), divergence, vorticity and Q.  The reference has nothing of the kind: its
grid is a bare point cloud without a gradient operator.

The operator is a weighted least-squares fit over the ``k`` nearest neighbours of every point (8 in 2-D, 26 in 3-D by default,
as everywhere in this package).  With ``dx_m = x[idx_m] - x_i``, ``h = max_m |dx_m|`` and the scaled stencil ``dxs = dx / h``:

    w_m = |dxs_m|^-power  (0 for a coincident copy),   M = sum_m w_m dxs_m dxs_m^T,   c[i, m, :] = w_m * M^-1 dxs_m / h
    d f / d x_a (i) = sum_m c[i, m, a] * (f[idx_m] - f[i])

The difference form makes every derivative of a constant field exactly zero.  A point whose neighbours are collinear / coplanar /
coincident (``h = 0`` or a Cholesky pivot of ``M`` at or below ``2^-40 trace(M)``) is DEGENERATE: its derivatives are zero and it
is listed in ``Gradient.degenerate``.

Neighbour search, coefficients (``s3_grad_coeff``) and the fused apply (``s3_grad_apply``, csrc/differential.hip) run on the GPU.
One launch gathers every neighbour row once, keeps the ``n_comp x d`` gradient entries in registers and writes only the
requested quantity: vorticity magnitude or Q of a 3-D velocity write one ninth of what the gradient tensor would take.

A refinement metric is then one line, e.g. the time-mean numerical schlieren ``metrics.temporal_mean(Gradient(xyz).magnitude(rho))``
(``metrics.RunningMoments`` across snapshot batches).
"""
import warnings

import numpy as np
import torch as pt

from . import hipops
from .arrays import Side, as_tensor, default_neighbors, hilbert_knn, resident


def _default(dim, n_points, n_neighbors):
    """the stencil size: 8 | 26 by default, capped at the other points of the cloud and at what one search returns"""
    k = default_neighbors(dim, n_neighbors, min(n_points - 1, hipops.GRAD_MAX_K))
    if n_points < dim + 1:
        raise ValueError(f"a gradient in {dim}-D needs at least {dim + 1} points, got {n_points}")
    return k


def _check_points(points):
    if points.dim() != 2 or int(points.shape[1]) not in (2, 3):
        raise ValueError(f"expected points [N, 2 | 3], got {tuple(points.shape)}")


def _check_power(power):
    if power not in (0, 1, 2):
        raise ValueError(f"power must be 0, 1 or 2, got {power!r}")
    return int(power)


def drop_self(idx, rows=None):
    """``idx`` int32 [N, k + 1] on the device, the k + 1 nearest points of the cloud to each of its points in ``KnnIndex.query`` order
    -> [N, k]: the entry that is the point itself removed, or the last one where more than k coincident copies crowd it out.  Not
    column 0: among duplicates the point itself may be listed later.  ``rows`` int32 [N]: the point each row of ``idx`` belongs to
    (None: row j is point j)."""
    n = int(idx.shape[0])
    hit = idx == (pt.arange(n, dtype=pt.int32, device=idx.device) if rows is None else rows).unsqueeze(1)
    hit[:, -1] |= ~hit.any(dim=1)
    return idx[~hit].view(n, int(idx.shape[1]) - 1).contiguous()


class Gradient:
    """Least-squares derivatives on the cloud ``points`` [N, d] (d = 2 | 3; numpy or torch, host or device).

    ``n_neighbors``: 8 in 2-D and 26 in 3-D by default, capped at N - 1 and at 63; ``power`` (0 | 1 | 2): the exponent of the
    inverse-distance weights.  The constructor searches the neighbours once, puts the points into Hilbert launch order and builds
    the coefficients; it warns once when points are degenerate (``n_degenerate``, ``degenerate``: bool [N] on the side the
    points came from).

    Fields are [N, (n_comp,) T] (``[N]``: one snapshot), float32 or float64, numpy or torch, host or device; a window
    ``field[:, t0:t1]`` of a scalar field that lives on the device is read where it lies (``arrays.resident``).  Results are
    float64 and come back on the side (and as the kind of array) the field came from; ``out`` may name the array to fill."""

    def __init__(self, points, n_neighbors=None, power=2):
        points, self._side = as_tensor(points, "points"), Side(points)
        _check_points(points)
        power = _check_power(power)
        self.n_points, self.dim = int(points.shape[0]), int(points.shape[1])
        self.n_neighbors = _default(self.dim, self.n_points, n_neighbors)
        self.power = power
        pts = hipops.to_device(points, pt.float64)
        # the points are launched in Hilbert order: neighbouring slots then gather the same few field rows
        idx, _, self._rows = hilbert_knn(pts, pts, self.n_neighbors + 1)
        self._idx = drop_self(idx, self._rows)
        self._coef, flag, self.n_degenerate = hipops.grad_coeff(pts, self._idx, power, rows=self._rows)
        degenerate = pt.zeros(self.n_points, dtype=pt.bool, device=pts.device)
        degenerate[self._rows.long()] = flag.bool()
        self._degenerate = degenerate
        if self.n_degenerate:
            warnings.warn(f"Gradient: {self.n_degenerate} of {self.n_points} points have collinear, coplanar or coincident neighbours; "
                          f"their derivatives are zero (see Gradient.degenerate)", RuntimeWarning, stacklevel=2)

    @classmethod
    def from_dataloader(cls, loader, n_neighbors=None, power=2):
        """the grid of an S^3 file: ``loader.vertices`` are the cell centres"""
        return cls(loader.vertices, n_neighbors=n_neighbors, power=power)

    @property
    def degenerate(self):
        return self._side.back(self._degenerate)

    # ---- the six quantities ---------------------------------------------------------------------------------------------
    def gradient(self, field, out=None):
        """[N, (n_comp,) T] -> [N, (n_comp,) d, T]"""
        return self._apply("gradient", field, out)

    def magnitude(self, field, out=None):
        """``|grad f|`` per component: [N, (n_comp,) T] -> [N, (n_comp,) T]"""
        return self._apply("magnitude", field, out)

    def divergence(self, u, out=None):
        """[N, d, T] -> [N, T]"""
        return self._apply("divergence", u, out)

    def vorticity(self, u, out=None):
        """[N, d, T] -> [N, T] in 2-D (``dv/dx - du/dy``), [N, 3, T] in 3-D"""
        return self._apply("vorticity", u, out)

    def vorticity_magnitude(self, u, out=None):
        """[N, d, T] -> [N, T]"""
        return self._apply("vorticity_magnitude", u, out)

    def q_criterion(self, u, out=None):
        """``Q = -1/2 sum_ab (du_a/dx_b) (du_b/dx_a)``: [N, d, T] -> [N, T]"""
        return self._apply("q", u, out)

    # ---------------------------------------------------------------------------------------------------------------------
    def _out_shape(self, mode, shape):
        """public shape of the result for a field of (public) shape ``shape``"""
        n, t = shape[0], (shape[-1] if len(shape) > 1 else None)
        tail = () if t is None else (t,)
        comp = tuple(shape[1:-1])
        if mode == "gradient":
            return (n,) + comp + (self.dim,) + tail
        if mode == "magnitude":
            return (n,) + comp + tail
        if mode == "vorticity" and self.dim == 3:
            return (n, 3) + tail
        return (n,) + tail

    def _apply(self, mode, field, out):
        field, side = as_tensor(field, "field"), Side(field)
        as_numpy = side.numpy
        shape = tuple(int(v) for v in field.shape)
        vector = mode not in ("gradient", "magnitude")
        if vector:
            if len(shape) != 3 or shape[0] != self.n_points or shape[1] != self.dim:
                raise ValueError(f"{mode}: expected a vector field [{self.n_points}, {self.dim}, T], got {shape}")
        elif not 1 <= len(shape) <= 3 or shape[0] != self.n_points:
            raise ValueError(f"{mode}: expected a field [{self.n_points}, (n_comp,) T], got {shape}")
        if 0 in shape:
            raise ValueError(f"{mode}: empty field {shape}")
        want = self._out_shape(mode, shape)
        if out is not None:
            if not isinstance(out, np.ndarray if as_numpy else pt.Tensor):
                raise TypeError(f"{mode}: out must be the kind of array the field is ({'numpy.ndarray' if as_numpy else 'torch.Tensor'}), "
                                f"got {type(out).__name__} for a field {shape}")
            o = pt.from_numpy(out) if as_numpy else out
            if o.dtype != pt.float64 or o.is_cuda != field.is_cuda:
                raise TypeError(f"{mode}: out must be float64 on the side of the field, got {o.dtype} on {o.device}")
            if tuple(o.shape) != want:
                raise ValueError(f"{mode}: out has shape {tuple(o.shape)}, the result {want}")
        dev_field = resident(field)
        direct = out is not None and not side.host and out.is_contiguous() and out.device == dev_field.device
        res = hipops.grad_apply(self._coef, self._idx, dev_field, mode, rows=self._rows, out=out if direct else None)
        if direct:
            return out
        res = side.back(res.view(want))
        if out is None:
            return res
        o.copy_(pt.as_tensor(res))
        return out
