"""
Connected regions of thresholded fields on the grid CELLS (Q or vorticity magnitude from ``Gradient``, ``u_x < 0``, a schlieren above
a threshold): how many vortices or separation bubbles a snapshot has, how big they are and where they lie -- for a whole batch of
snapshots in one pass on the GPU (csrc/regions.hip).  The reference has nothing of the kind; on the host the route is
``scipy.sparse.csgraph`` one snapshot at a time, after downloading the field.

Two cells are connected when they share a face of positive area (edges and corners do not connect); across a level jump the finer
cells all touch the coarse one.  ``Grid.neighbours`` holds those pairs; include/s3hip.h states the definitions.  A cell is IN at
snapshot t iff ``lo <= field[c, t] <= hi`` (NaN is out); its label is the smallest cell id of its region, -1 where it is out, so
the labels are a pure function of the field: reruns, batch splits and element types give equal bits.

    regions = Regions.from_grid(grid)                           # the upload and the index are shared with Probe, Isosurface, Tracer
    table = regions.extract(q[:, t0:t1], lo=q0, weight=vorticity_magnitude[:, t0:t1])
    big = table.largest(3)                                      # the three largest vortices of every snapshot
    labels = regions.label(u_x, hi=0.0)                         # [Nc, T]: the recirculation bubbles themselves
"""
import numpy as np
import torch as pt

from . import hipops
from .arrays import Side, as_tensor, resident
from .grid import Grid


class RegionTable:
    """The regions of ``T`` snapshots, column after column, inside a column by ascending label: ``offsets`` int64 numpy [T + 1] (column
    t owns [offsets[t], offsets[t + 1])), ``label`` int32 [R] (the smallest cell id of the region), ``n_cells`` int64 [R], ``volume``
    f64 [R], ``centroid`` / ``lo`` / ``hi`` f64 [R, d] (volume-weighted centre and bounding box) and, with a weight field g,
    ``integral`` (sum of V g), ``g_min``, ``g_max`` f64 [R] (None without one) -- on the side (and as the kind of array) the labels
    came from."""

    FIELDS = hipops.REGION_FIELDS

    def __init__(self, offsets, **arrays):
        self.offsets = offsets
        for k in self.FIELDS:
            setattr(self, k, arrays[k])
        self.n_snapshots = len(offsets) - 1

    def __len__(self):
        return int(self.offsets[-1])

    @property
    def n_regions(self):
        """int64 numpy [T]"""
        return np.diff(self.offsets)

    def _rows(self, rows):
        return {k: None if getattr(self, k) is None else getattr(self, k)[rows] for k in self.FIELDS}

    def of_snapshot(self, t):
        """dict of views: the regions of snapshot ``t``"""
        t = int(t)
        if not 0 <= t < self.n_snapshots:
            raise IndexError(f"snapshot {t} outside [0, {self.n_snapshots})")
        return self._rows(slice(int(self.offsets[t]), int(self.offsets[t + 1])))

    def largest(self, n):
        """the ``n`` largest regions of each column by volume, ties broken by the smaller label -> ``RegionTable`` (a column with
        fewer regions keeps them all)"""
        n = int(n)
        if n < 1:
            raise ValueError(f"n must be positive, got {n}")
        volume = as_tensor(self.volume, "volume").cpu().numpy()
        keep, offsets = [], [0]
        for t in range(self.n_snapshots):
            a, b = int(self.offsets[t]), int(self.offsets[t + 1])
            # (inside a column the regions stand by ascending label: a stable sort by falling volume breaks ties by label)
            keep.append(a + np.argsort(-volume[a:b], kind="stable")[:n])
            offsets.append(offsets[-1] + len(keep[-1]))
        rows = np.concatenate(keep) if keep else np.zeros(0, dtype=np.int64)
        if not isinstance(self.volume, np.ndarray):
            rows = pt.from_numpy(rows).to(self.volume.device)
        return RegionTable(np.asarray(offsets, dtype=np.int64), **self._rows(rows))


class Regions:
    """``centers`` [Nc, d], ``levels`` [Nc] or [Nc, 1] and ``width`` (the size of the initial cell) of a generated grid, d = 2 | 3;
    numpy or torch, host or device: the cell part of a ``grid.Grid``, kept as ``grid``; ``from_grid`` takes one that is there already.
    Fields are [Nc] or [Nc, T], float32 or float64 (a boolean mask is taken as it is: True is in), numpy or torch, host or device; a
    window ``field[:, t0:t1]`` of a field that lives on the device is read where it lies (``arrays.resident``).  Results come back on
    the side (and as the kind of array) the input came from.  Argument errors are ``ValueError``."""

    def __init__(self, centers, levels, width):
        self._on(Grid(centers, levels, width))

    def _on(self, grid):
        if grid.centers is None:
            raise ValueError("regions are sets of cells: build the Grid with centers, levels and width")
        self.grid, self.dim, self.n_cells = grid, grid.dim, grid.n_cells
        self._index, self._neighbours = grid.index, grid.neighbours
        # the hooking launch takes the cells in Hilbert order: neighbouring slots then chase through the same few label rows
        self._order = hipops.spatial_order(grid.centers)

    @classmethod
    def from_grid(cls, grid):
        """a ``grid.Grid`` with its cell part, which is neither uploaded nor indexed again"""
        self = cls.__new__(cls)
        self._on(grid)
        return self

    @classmethod
    def from_dataloader(cls, loader):
        """the grid of an S^3 file (``data.Dataloader``)"""
        return cls.from_grid(Grid.from_dataloader(loader))

    @classmethod
    def from_s_cube(cls, s_cube):
        """the grid of a ``SparseSpatialSampling`` after ``execute_grid_generation``"""
        return cls.from_grid(Grid.from_s_cube(s_cube))

    def _cells(self, field, what, dtypes=None):
        try:
            field = as_tensor(field, what)
        except TypeError as e:
            raise ValueError(str(e)) from e
        shape = tuple(int(v) for v in field.shape)
        if not 1 <= len(shape) <= 2 or shape[0] != self.n_cells:
            raise ValueError(f"expected {what} [{self.n_cells}] or [{self.n_cells}, T] on the grid's cells, got {shape}")
        if 0 in shape:
            raise ValueError(f"empty {what} {shape}")
        if dtypes is not None and field.dtype not in dtypes:
            raise ValueError(f"expected {what} of {' / '.join(str(d) for d in dtypes)}, got {field.dtype}")
        return field

    @staticmethod
    def _bounds(lo, hi):
        try:
            lo, hi = float(lo), float(hi)
        except (TypeError, ValueError) as e:
            raise ValueError(f"lo and hi must be numbers, got {lo!r} and {hi!r}") from e
        if np.isnan(lo) or np.isnan(hi) or lo > hi:
            raise ValueError(f"expected lo <= hi, neither NaN, got {lo!r} and {hi!r}")
        return lo, hi

    def _label(self, field, lo, hi, out=None):
        """-> (labels on the device [Nc, T], the field's shape)"""
        field = self._cells(field, "field")
        lo, hi = self._bounds(lo, hi)
        if field.dtype == pt.bool:                      # a mask: float32 0 / 1, in above one half
            field, lo, hi = field.to(pt.float32), 0.5, np.inf
        elif not field.is_floating_point():
            raise ValueError(f"expected a float32 / float64 field or a boolean mask, got {field.dtype}")
        dev = resident(field)
        if out is not None:
            if not (isinstance(out, pt.Tensor) and out.is_cuda and out.dtype == pt.int32 and tuple(out.shape) == tuple(field.shape)
                    and (out.is_contiguous() or (out.dim() == 2 and out.stride(1) == 1 and out.stride(0) >= out.shape[1]))):
                raise ValueError(f"out must be an int32 device tensor {tuple(field.shape)} with unit inner stride")
        labels = hipops.region_label(dev, self._neighbours, lo, hi, order=self._order, out=out)
        return labels, tuple(field.shape)

    def label(self, field, lo=-np.inf, hi=np.inf, out=None):
        """-> int32 labels in the field's shape: -1 where the cell is out, otherwise the smallest cell id of its region.  ``out``: an
        int32 device tensor of that shape to write into (rows may be pitched)"""
        labels, shape = self._label(field, lo, hi, out)
        return out if out is not None else Side(field).back(labels.view(shape))

    def _table(self, labels, weight, shape, side):
        g = None
        if weight is not None:
            weight = self._cells(weight, "weight")
            if tuple(weight.shape) != shape:
                raise ValueError(f"the weight {tuple(weight.shape)} differs in shape from {shape}")
            g = resident(weight)
        try:
            res = hipops.region_table(labels, self._index, g)
        except TypeError as e:                          # (device labels whose rows cannot be read where they lie)
            raise ValueError(str(e)) from e
        return RegionTable(res["offsets"], **{k: None if res[k] is None else side.back(res[k]) for k in RegionTable.FIELDS})

    def table(self, labels, weight=None):
        """labels [Nc] or [Nc, T] as ``label`` gave them (int32; on the device they are read where they lie) -> ``RegionTable``;
        ``weight``: a second cell field g of the same shape for ``integral``, ``g_min`` and ``g_max``"""
        labels, side = self._cells(labels, "labels", (pt.int32,)), Side(labels)
        return self._table(labels if labels.is_cuda else hipops.to_device(labels), weight, tuple(labels.shape), side)

    def extract(self, field, lo=-np.inf, hi=np.inf, weight=None):
        """``label`` and ``table`` in one: the labels stay on the device -> ``RegionTable`` on the side the field came from"""
        labels, shape = self._label(field, lo, hi)
        return self._table(labels, weight, shape, Side(field))
