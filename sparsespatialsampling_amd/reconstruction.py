"""
Reconstruction error of a generated grid: "how good is the grid I just generated?" -- the last step of the S^3 workflow, the
reference's ``post_processing/compute_error_OAT.py:208-233``.  The exported fields are interpolated BACK onto the points of
the original CFD mesh (``KNeighborsRegressor(n_neighbors=8 | 26, weights="distance")`` fitted on the cell centres) and compared
with the original fields there:

    d = s * (fitted - original),  ref = s * original              (s: the square root of the original cell area)
    error_time  = ||d[:, t]|| / ||ref[:, t]||      error_total = ||d|| / ||ref||
    error_space_mean / error_space_std = mean / std over time of |d| per original point

The reference predicts the whole fitted field on the host ([N, T] float64: 40 GB for the 3-D cylinder) and reduces it three
times.  Here KNN search, weights, gather, subtraction and all reductions run on the GPU, and the gather is fused with the
reductions (``s3_recon_error``, csrc/recon.hip): nothing of size N x T is written, snapshots may arrive in batches.
"""
import numpy as np
import torch as pt

from . import hipops
from .arrays import Side, as_tensor, default_neighbors, hilbert_knn, knn_table, resident
from .metrics import RunningMoments


def _default_neighbors(dim, n_centers, n_neighbors):
    return default_neighbors(dim, n_neighbors, n_centers)                         # compute_error_OAT.py:209


def _check_clouds(grid_centers, coordinates):
    if grid_centers.dim() != 2 or coordinates.dim() != 2:
        raise ValueError(f"expected grid_centers [Nc, d] and coordinates [N, d], got {tuple(grid_centers.shape)} and "
                         f"{tuple(coordinates.shape)}")
    if grid_centers.shape[1] != coordinates.shape[1] or int(grid_centers.shape[1]) not in (2, 3):
        raise ValueError(f"grid_centers and coordinates must share their dimension (2 or 3), got {int(grid_centers.shape[1])} "
                         f"and {int(coordinates.shape[1])}")
    if grid_centers.shape[0] < 1:
        raise ValueError("the grid has no cells")


class ReconstructionError:
    """Error of the fields on a generated grid against the original CFD fields, measured at the original points.

    ``grid_centers`` [Nc, d]: the cell centres of the generated grid (``Dataloader.vertices``); ``coordinates`` [N, d]: the
    points of the original mesh; ``point_scale`` [N] (optional): the factor both fields are weighted with -- what the reference's
    script calls ``cell_area_orig`` AFTER its ``.sqrt()`` (compute_error_OAT.py:154, 189, 223), i.e. the square root of the
    original cell areas / volumes; ``n_neighbors``: 8 in 2-D, 26 in 3-D by default as in the script, capped at Nc.

    The constructor searches the neighbours once; ``update(grid_fields, orig_fields)`` then takes the same snapshots of both
    fields, [Nc, (n_comp,) T_b] and [N, (n_comp,) T_b] (float32 / float64, host or device), batch by batch; a window
    ``orig[:, t0:t1]`` of a scalar field that lives on the device is read where it lies (``arrays.resident``), other non-contiguous
    batches are copied once (the small grid batch always is).  The results cover all snapshots seen so far and come back on the side
    (host / device) the fields came from:

    ``error_time``        [T] f64: ``||d[:, :, t]|| / ||ref[:, :, t]||``, norms over points and components
    ``error_total``       float: ``||d||_F / ||ref||_F``
    ``error_space_mean``  [N] f64: mean of ``|d|`` over the point's n_comp * T values
    ``error_space_std``   [N] f64: ``torch.std`` of the same (unbiased)

    A zero reference norm divides as torch does (inf / nan)."""

    def __init__(self, grid_centers, coordinates, point_scale=None, n_neighbors=None):
        grid_centers, coordinates = as_tensor(grid_centers, "grid_centers"), as_tensor(coordinates, "coordinates")
        _check_clouds(grid_centers, coordinates)
        self.n_cells, self.n_points = int(grid_centers.shape[0]), int(coordinates.shape[0])
        self.n_neighbors = _default_neighbors(int(coordinates.shape[1]), self.n_cells, n_neighbors)
        if point_scale is not None:
            point_scale = as_tensor(point_scale, "point_scale")
            if point_scale.numel() != self.n_points:
                raise ValueError(f"point_scale must hold one value per point ({self.n_points}), got {tuple(point_scale.shape)}")
        self._side = Side(coordinates)
        pts = hipops.to_device(coordinates, pt.float64)
        # the points are launched in Hilbert order: neighbouring lanes then gather the same few grid rows
        self._idx, self._w, self._rows = hilbert_knn(grid_centers, pts, self.n_neighbors, exact_weights=True)
        self._scale = None
        if point_scale is not None:
            s = hipops.to_device(point_scale.reshape(-1, 1), pt.float64)
            self._scale = hipops.gather_rows(s, self._rows, pt.empty_like(s)).reshape(-1) if self.n_points else s.reshape(-1)
        assert self._w.shape == (self.n_points, self.n_neighbors)
        self.n_snapshots = 0
        self._moments = RunningMoments()                # of |d| per point, over its n_comp * n_snapshots values so far
        self._sum_d, self._sum_ref = [], []             # per batch: [T_b] device tensors
        self._trailing = None                           # n_comp part of the fields' shape

    @classmethod
    def from_dataloader(cls, loader, coordinates, point_scale=None, n_neighbors=None):
        """the grid of an S^3 file: ``loader.vertices`` are the cell centres"""
        return cls(loader.vertices, coordinates, point_scale=point_scale, n_neighbors=n_neighbors)

    def update(self, grid_fields, orig_fields) -> "ReconstructionError":
        grid_fields, orig_fields = as_tensor(grid_fields, "grid_fields"), as_tensor(orig_fields, "orig_fields")
        if grid_fields.dim() < 2 or orig_fields.dim() < 2:
            raise ValueError(f"expected fields [Nc, (n_comp,) T] and [N, (n_comp,) T], got {tuple(grid_fields.shape)} and "
                             f"{tuple(orig_fields.shape)}")
        if int(grid_fields.shape[0]) != self.n_cells or int(orig_fields.shape[0]) != self.n_points:
            raise ValueError(f"expected {self.n_cells} grid rows and {self.n_points} original rows, got "
                             f"{int(grid_fields.shape[0])} and {int(orig_fields.shape[0])}")
        if tuple(grid_fields.shape[1:]) != tuple(orig_fields.shape[1:]):
            raise ValueError(f"grid and original fields differ in their (n_comp, T) shape: {tuple(grid_fields.shape[1:])} and "
                             f"{tuple(orig_fields.shape[1:])}")
        trailing = tuple(int(v) for v in orig_fields.shape[1:-1])
        if self._trailing is not None and trailing != self._trailing:
            raise ValueError(f"the batches differ in their component shape: {self._trailing} and {trailing}")
        t_b = int(orig_fields.shape[-1])
        if t_b == 0 or (trailing and int(np.prod(trailing)) == 0):
            return self
        self._trailing = trailing
        self._side = Side(orig_fields)
        grid_dev, orig_dev = resident(grid_fields, pitched=False), resident(orig_fields)    # (the kernel has a row pitch for orig alone)
        mean_b, m2_b, colsum = hipops.recon_error(self._w, self._idx, grid_dev, orig_dev, rows=self._rows, scale=self._scale)
        self._moments.merge(int(np.prod(orig_fields.shape[1:])), mean_b, m2_b)
        per_snapshot = colsum.view(2, -1, t_b).sum(1)   # components into their snapshot
        self._sum_d.append(per_snapshot[0])
        self._sum_ref.append(per_snapshot[1])
        self.n_snapshots += t_b
        return self

    def _need_data(self):
        if self._moments.count == 0:
            raise RuntimeError("ReconstructionError: no snapshots yet, call update() first")

    @property
    def error_time(self) -> pt.Tensor:
        self._need_data()
        return self._side.back(pt.cat(self._sum_d).sqrt() / pt.cat(self._sum_ref).sqrt())

    @property
    def error_total(self) -> float:
        self._need_data()
        return float(pt.cat(self._sum_d).sum().sqrt() / pt.cat(self._sum_ref).sum().sqrt())

    @property
    def error_space_mean(self) -> pt.Tensor:
        self._need_data()
        return self._side.back(self._moments.mean())

    @property
    def error_space_std(self) -> pt.Tensor:
        self._need_data()
        return self._side.back(self._moments.std())


def reconstruct(grid_centers, grid_fields, coordinates, n_neighbors=None) -> pt.Tensor:
    """the fitted field itself, ``KNeighborsRegressor(n_neighbors, weights="distance").fit(grid_centers, grid_fields)
    .predict(coordinates)`` as float64 [N, ...]: the unfused path (``hipops.interp`` with the exact weights), for cases small
    enough to hold N x T values -- a plot of the fitted field.  Returned on the side ``grid_fields`` came from."""
    grid_centers, coordinates = as_tensor(grid_centers, "grid_centers"), as_tensor(coordinates, "coordinates")
    grid_fields = as_tensor(grid_fields, "grid_fields")
    _check_clouds(grid_centers, coordinates)
    if grid_fields.dim() < 1 or int(grid_fields.shape[0]) != int(grid_centers.shape[0]):
        raise ValueError(f"expected one row of grid_fields per cell centre ({int(grid_centers.shape[0])}), got "
                         f"{tuple(grid_fields.shape)}")
    k = _default_neighbors(int(coordinates.shape[1]), grid_centers.shape[0], n_neighbors)
    idx, w = knn_table(grid_centers, hipops.to_device(coordinates, pt.float64), k, exact_weights=True)
    return Side(grid_fields).back(hipops.interp(w, idx, resident(grid_fields, pitched=False)))
