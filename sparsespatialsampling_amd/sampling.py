"""
Sampling of fields on a generated grid at arbitrary positions: probe points, lines, planes, rasters.  The reference has nothing of
the kind: its post-processing hands the cell centres to a plotting library as a bare point cloud.

A generated grid is a set of disjoint axis-aligned boxes, each a dyadic fraction of the initial cell, so "which cell holds this
point" has exactly one answer -- and it is NOT the cell with the nearest centre wherever the level changes.  ``Probe`` answers it
exactly (``hipops.cell_index``: Morton ranges of the leaves on a lattice derived from the grid, sorted once; ``hipops.cell_locate``:
one binary search per point; a point on a face belongs to the upper cell) and then reads fields there (``hipops.cell_sample``,
csrc/sample.hip), batch by batch:

    mode="cell"     the value of the containing cell, a bit-exact copy: a slice shows the grid as it is
    mode="linear"   for fields on the grid NODES (``interpolate_at_vertices=True`` exports): the multilinear blend of the containing
                    cell's corner values, continuous inside a cell and across faces between cells of one level

Points that no cell holds -- outside the domain or inside a body -- come back as NaN (``Probe.inside`` tells them apart), so a
raster can go to ``imshow`` as it is.  ``line``, ``plane`` and ``raster`` only build point sets on the host.

    probe = Probe.from_dataloader(loader, raster(lo, hi, (ny, nx)))
    frames = hipops.snapshot_major(probe.sample(field), 1, n_snapshots)         # [T, ny * nx]
"""
import numpy as np
import torch as pt

from . import hipops
from .arrays import Side, as_tensor, resident
from .grid import Grid


# ---- point sets (host only) -------------------------------------------------------------------------------------------------
def _vector(v, what, dim=None):
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if v.size not in ((2, 3) if dim is None else (dim,)):
        raise ValueError(f"{what} must have {'2 or 3' if dim is None else dim} components, got {v.size}")
    return v


def _shape(shape, n_axes=None):
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
    if (n_axes is not None and len(shape) != n_axes) or not shape or min(shape) < 1:
        raise ValueError(f"shape must be {n_axes if n_axes is not None else 'a tuple of'} positive counts, got {shape}")
    return shape


def line(p0, p1, n):
    """``n`` points from ``p0`` to ``p1``, both ends included (``n = 1``: ``p0``) -> float64 [n, d]"""
    p0 = _vector(p0, "p0")
    p1 = _vector(p1, "p1", p0.size)
    (n,) = _shape(n, 1)
    s = np.arange(n, dtype=np.float64) / max(n - 1, 1)
    return p0 + s[:, None] * (p1 - p0)


def plane(origin, e1, e2, shape):
    """the points ``origin + (i + 1/2) / n1 * e1 + (j + 1/2) / n2 * e2`` of the parallelogram spanned by ``e1`` and ``e2`` at
    ``origin``, ``shape = (n1, n2)`` -> float64 [n1 * n2, d], ``i`` the slow index (``result.reshape(n1, n2, d)``)"""
    origin = _vector(origin, "origin")
    e1, e2 = _vector(e1, "e1", origin.size), _vector(e2, "e2", origin.size)
    n1, n2 = _shape(shape, 2)
    s1, s2 = (np.arange(n1) + 0.5) / n1, (np.arange(n2) + 0.5) / n2
    return (origin + s1[:, None, None] * e1 + s2[None, :, None] * e2).reshape(n1 * n2, origin.size)


def raster(lo, hi, shape):
    """pixel (voxel) centres of the uniform raster over the box ``[lo, hi]``: ``shape`` counts the pixels along x, y (, z) -- d
    entries -- and the result is float64 [prod(shape), d] with the LAST axis running fastest: ``values.reshape(shape)`` is indexed
    ``[ix, iy (, iz)]`` (``imshow`` wants its transpose)."""
    lo = _vector(lo, "lo")
    hi = _vector(hi, "hi", lo.size)
    shape = _shape(shape, lo.size)
    axes = [lo[a] + (np.arange(n) + 0.5) / n * (hi[a] - lo[a]) for a, n in enumerate(shape)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, lo.size)


# ---- the probe ---------------------------------------------------------------------------------------------------------------
class Probe:
    """``points`` [Nq, d] located once in the grid (``centers`` [Nc, d], ``levels`` [Nc] or [Nc, 1], ``width``: the size of the
    initial cell; numpy or torch, host or device: a ``grid.Grid``, kept as ``grid``; ``from_grid`` takes one that is there already).
    ``nodes`` [Nn, d] and ``faces`` [Nc, 2^d] (the corner nodes of every cell) are needed for ``mode="linear"`` only.  The grid is
    refused with ``ValueError`` when its cells are no disjoint dyadic boxes on one lattice.

    ``cell_ids`` (int32 [Nq], -1: no cell) and ``inside`` (bool [Nq]) come back in the caller's order, on the side (and as the kind
    of array) the points came from.  ``sample`` takes fields [rows, (n_comp,) T] (``[rows]``: one snapshot; rows = cells for
    ``mode="cell"``, nodes for ``mode="linear"``), float32 or float64, numpy or torch, host or device; a window ``field[:, t0:t1]``
    of a scalar field that lives on the device is read where it lies (``arrays.resident``).  Results are float64 [Nq, (n_comp,) T] on
    the side the field came from, NaN where ``inside`` is False."""

    def __init__(self, centers, levels, width, points, nodes=None, faces=None):
        self._locate(Grid(centers, levels, width, nodes, faces), points)

    def _locate(self, grid, points):
        points, self._side = as_tensor(points, "points"), Side(points)
        self.grid, self.dim, self.n_cells, self.n_nodes = grid, grid.dim, grid.n_cells, grid.n_nodes
        if points.dim() != 2 or int(points.shape[1]) != self.dim:
            raise ValueError(f"expected points [Nq, {self.dim}], got {tuple(points.shape)}")
        self.n_points = int(points.shape[0])
        self._index = grid.index
        self._points = hipops.to_device(points, pt.float64)
        if self.n_points:
            # the points are launched in Hilbert order: neighbouring slots then read the same few field rows
            self._rows = hipops.spatial_order(self._points)
            self._ids = hipops.cell_locate(self._index, self._points, rows=self._rows)
        else:
            self._rows, self._ids = None, pt.empty(0, dtype=pt.int32, device=self._points.device)

    @classmethod
    def from_grid(cls, grid, points):
        """``points`` located in a ``grid.Grid``, which is neither uploaded nor indexed again"""
        self = cls.__new__(cls)
        self._locate(grid, points)
        return self

    @classmethod
    def from_dataloader(cls, loader, points):
        """the grid of an S^3 file (``data.Dataloader``)"""
        return cls.from_grid(Grid.from_dataloader(loader), points)

    @classmethod
    def from_s_cube(cls, s_cube, points):
        """the grid of a ``SparseSpatialSampling`` after ``execute_grid_generation``"""
        return cls.from_grid(Grid.from_s_cube(s_cube), points)

    @property
    def cell_ids(self):
        return self._side.back(self._ids)

    @property
    def inside(self):
        return self._side.back(self._ids >= 0)

    def sample(self, field, mode="cell"):
        """[rows, (n_comp,) T] -> float64 [Nq, (n_comp,) T]"""
        if mode not in hipops.SAMPLE_MODES:
            raise ValueError(f"unknown mode {mode!r}, expected one of {sorted(hipops.SAMPLE_MODES)}")
        if mode == "linear" and self.grid.faces is None:
            raise ValueError("mode 'linear' blends the corner values of a cell: build the Probe with nodes and faces")
        field, side = as_tensor(field, "field"), Side(field)
        shape = tuple(int(v) for v in field.shape)
        n_rows = self.n_cells if mode == "cell" else self.n_nodes
        if not 1 <= len(shape) <= 3 or shape[0] != n_rows:
            raise ValueError(f"{mode}: expected a field [{n_rows}, (n_comp,) T] on the grid's {'cells' if mode == 'cell' else 'nodes'}, got {shape}")
        if 0 in shape:
            raise ValueError(f"{mode}: empty field {shape}")
        dev_field = resident(field)
        if self.n_points:
            res = hipops.cell_sample(self._ids, dev_field, mode, rows=self._rows, index=self._index, points=self._points, faces=self.grid.faces)
        else:
            res = pt.empty((0,) + shape[1:], dtype=pt.float64, device=dev_field.device)
        return side.back(res.view((self.n_points,) + shape[1:]))
