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

Following a region through time: the overlap table of ``labels[:, :T-1]`` and ``labels[:, 1:]`` (csrc/overlap.hip; include/s3overlap.h
states the definitions) links every region of snapshot t to the regions of t + 1 it shares cells with, the shared volume an exact
integer; ``RegionTracks`` chains the mutual best links into tracks on the host.

    tracks = regions.track(labels)                              # born / died / merged / split per region, tracks.velocity(dt)
    edges = regions.overlap(labels_q, labels_p)                 # the same table for two labellings of the same snapshots
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


class OverlapTable:
    """The overlap edges of two label arrays [Nc, T] of one grid (include/s3overlap.h), column after column, inside a column by
    ascending (src, dst): ``offsets`` int64 numpy [T + 1] (column t owns [offsets[t], offsets[t + 1])), ``src`` / ``dst`` int32 [E] (a
    label of the first and of the second array that share cells at that column), ``n_cells`` int64 [E] (how many), ``units`` int64 [E]
    (their volume in cells of the finest level: an exact integer, the unsigned bits) and ``volume`` f64 [E] -- on the side (and as the
    kind of array) the labels came from."""

    FIELDS = hipops.OVERLAP_FIELDS

    def __init__(self, offsets, **arrays):
        self.offsets = offsets
        for k in self.FIELDS:
            setattr(self, k, arrays[k])
        self.n_columns = len(offsets) - 1

    def __len__(self):
        return int(self.offsets[-1])

    @property
    def n_edges(self):
        """int64 numpy [T]"""
        return np.diff(self.offsets)

    def of_column(self, t):
        """dict of views: the edges of column ``t``"""
        t = int(t)
        if not 0 <= t < self.n_columns:
            raise IndexError(f"column {t} outside [0, {self.n_columns})")
        rows = slice(int(self.offsets[t]), int(self.offsets[t + 1]))
        return {k: getattr(self, k)[rows] for k in self.FIELDS}


def _host(x):
    return x if isinstance(x, np.ndarray) else x.detach().cpu().numpy()


def _best(group, units, label, other, n_rows):
    """per row of the table the ``other`` end of its best edge, -1 without one: the largest ``units``, ties to the smaller ``label``"""
    out = np.full(n_rows, -1, dtype=np.int64)
    if len(group):
        order = np.lexsort((label, ~units, group))      # by group, then falling units (~u = 2^64 - 1 - u), then rising label
        g = group[order]
        heads = np.flatnonzero(np.r_[True, g[1:] != g[:-1]])
        out[g[heads]] = other[order][heads]
    return out


class RegionTracks:
    """Regions followed from snapshot to snapshot.  ``table``: the ``RegionTable`` of a labelling [Nc, T]; ``edges``: the
    ``OverlapTable`` of ``labels[:, :T-1]`` against ``labels[:, 1:]`` (column t links snapshot t to t + 1); edges whose ``volume`` is
    below ``min_volume`` are ignored throughout.  Per row of the table, int64 [R] unless said otherwise:

        n_in, n_out     edges into the row from t - 1 / out of it to t + 1
        successor       the row at t + 1 it shares the most ``units`` with, ties to the smaller label; -1 without an edge
        predecessor     the same rule backwards
        track           the track the row lies in
        born, died, merged, split       bool: n_in == 0 and t > 0; n_out == 0 and t < T - 1; n_in >= 2; n_out >= 2

    A link a -> b is a CONTINUATION iff it is mutual (successor[a] == b and predecessor[b] == a); the tracks are the chains of
    continuations, so every row lies in exactly one, and they are numbered by (first snapshot, label there).  Per track ``first`` (its
    first snapshot) and ``length`` (its rows), int64 [n_tracks]; ``rows(k)`` are its rows in time.

    No kernel is involved here: this is bookkeeping on tables of R regions and E edges, done on the host with numpy -- one global
    ``searchsorted`` on ``t * n_cells + label`` maps the edge ends to rows, a ``lexsort`` per direction picks the best edges, pointer
    jumping (log2 T rounds) finds the first row of every chain.  No Python loop over regions or edges.  The arrays are handed back on
    the side the labels came from."""

    def __init__(self, table, edges, n_cells, min_volume=0.0, side=None):
        self.table, self.edges, self.min_volume = table, edges, float(min_volume)
        n_cells, n_t = int(n_cells), table.n_snapshots
        if edges.n_columns != max(n_t - 1, 0):
            raise ValueError(f"a table of {n_t} snapshots needs edges of {max(n_t - 1, 0)} columns, got {edges.n_columns}")
        n_rows = len(table)
        t_row = np.repeat(np.arange(n_t, dtype=np.int64), np.diff(table.offsets))
        row_key = t_row * n_cells + _host(table.label).astype(np.int64)
        t_edge = np.repeat(np.arange(edges.n_columns, dtype=np.int64), np.diff(edges.offsets))
        src, dst = _host(edges.src).astype(np.int64), _host(edges.dst).astype(np.int64)
        ends = np.concatenate([t_edge * n_cells + src, (t_edge + 1) * n_cells + dst])
        rows = np.searchsorted(row_key, ends)
        if len(ends) and not (n_rows and np.array_equal(row_key[np.minimum(rows, n_rows - 1)], ends)):
            raise ValueError("an edge ends at a label that is no region of the table: the table and the edges are of other labels")
        keep = _host(edges.volume) >= self.min_volume
        a, b = rows[:len(src)][keep], rows[len(src):][keep]
        units = _host(edges.units).view(np.uint64)[keep]
        n_out, n_in = np.bincount(a, minlength=n_rows).astype(np.int64), np.bincount(b, minlength=n_rows).astype(np.int64)
        successor, predecessor = _best(a, units, dst[keep], b, n_rows), _best(b, units, src[keep], a, n_rows)
        ids = np.arange(n_rows, dtype=np.int64)
        linked = (predecessor >= 0) & (successor[np.maximum(predecessor, 0)] == ids)        # the continuation that ends at the row
        self._before = np.where(linked, predecessor, -1)
        head = np.where(linked, predecessor, ids)
        while True:                                     # pointer jumping: every round doubles the links a row looks back over
            jumped = head[head]
            if np.array_equal(jumped, head):
                break
            head = jumped
        starts = np.flatnonzero(~linked)                # ascending rows: by (snapshot, label)
        number = np.full(n_rows, -1, dtype=np.int64)
        number[starts] = np.arange(len(starts))
        track = number[head]
        self._order = np.lexsort((t_row, track))
        self._starts = np.searchsorted(track[self._order], np.arange(len(starts) + 1))
        self._t_row, self._side, self.n_tracks = t_row, side, len(starts)
        back = self._back
        self.n_in, self.n_out, self.successor, self.predecessor, self.track = back(n_in), back(n_out), back(successor), back(predecessor), back(track)
        self.born, self.died = back((n_in == 0) & (t_row > 0)), back((n_out == 0) & (t_row < n_t - 1))
        self.merged, self.split = back(n_in >= 2), back(n_out >= 2)
        self.first, self.length = back(t_row[starts]), back(np.diff(self._starts))

    def _back(self, a):
        return a if self._side is None else self._side.back(pt.from_numpy(np.ascontiguousarray(a)))

    def __len__(self):
        return self.n_tracks

    def rows(self, k):
        """int64 numpy: the rows of the table that make up track ``k``, in time"""
        k = int(k)
        if not 0 <= k < self.n_tracks:
            raise IndexError(f"track {k} outside [0, {self.n_tracks})")
        return self._order[self._starts[k]:self._starts[k + 1]]

    def velocity(self, dt):
        """f64 [R, d]: (centroid of the row - centroid of the row before it in its track) / dt, NaN at the first row of a track"""
        dt = float(dt)
        if not dt > 0.0:
            raise ValueError(f"dt must be positive, got {dt!r}")
        centroid = _host(self.table.centroid)
        v = (centroid - centroid[np.maximum(self._before, 0)]) / dt
        v[self._before < 0] = np.nan
        return self._back(v)


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

    def _overlap(self, a, b, side):
        try:
            res = hipops.overlap_table(a, b, self._index)
        except TypeError as e:                          # (device labels whose rows cannot be read where they lie)
            raise ValueError(str(e)) from e
        return OverlapTable(res["offsets"], **{k: side.back(res[k]) for k in OverlapTable.FIELDS})

    def overlap(self, labels_a, labels_b):
        """two label arrays of one shape, [Nc] or [Nc, T], as ``label`` gave them (int32; on the device they are read where they lie,
        two windows of one array included) -> ``OverlapTable``: per column which regions of the first share cells with which regions
        of the second, and how much.  On the side ``labels_a`` came from"""
        a, b, side = self._cells(labels_a, "labels_a", (pt.int32,)), self._cells(labels_b, "labels_b", (pt.int32,)), Side(labels_a)
        if tuple(a.shape) != tuple(b.shape):
            raise ValueError(f"labels_b {tuple(b.shape)} differs in shape from labels_a {tuple(a.shape)}")
        return self._overlap(*(x if x.is_cuda else hipops.to_device(x) for x in (a, b)), side)

    def track(self, labels, table=None, min_volume=0.0):
        """labels [Nc, T] as ``label`` gave them -> ``RegionTracks``: the regions of snapshot t linked to those of t + 1 they share
        cells with (the overlap of ``labels[:, :T-1]`` and ``labels[:, 1:]``, two windows read where they lie).  ``table``: the
        ``RegionTable`` of these labels where there is one already (built here otherwise, without a weight); ``min_volume``: edges
        that share less volume are ignored.  A single snapshot has no edges: every region is its own track"""
        labels, side = self._cells(labels, "labels", (pt.int32,)), Side(labels)
        try:
            min_volume = float(min_volume)
        except (TypeError, ValueError) as e:
            raise ValueError(f"min_volume must be a number, got {min_volume!r}") from e
        if not min_volume >= 0.0:
            raise ValueError(f"min_volume must not be negative or NaN, got {min_volume!r}")
        shape = tuple(labels.shape)
        n_t = shape[1] if len(shape) == 2 else 1
        if table is not None and not (isinstance(table, RegionTable) and table.n_snapshots == n_t):
            raise ValueError(f"table must be the RegionTable of these labels ({n_t} snapshots)")
        dev = labels if labels.is_cuda else hipops.to_device(labels)
        if dev.dim() == 1:
            dev = dev.contiguous().view(-1, 1)
        if table is None:
            table = self._table(dev, None, tuple(dev.shape), side)
        if n_t > 1:
            edges = self._overlap(dev[:, :n_t - 1], dev[:, 1:], side)
        else:
            empty = {k: side.back(pt.empty(0, dtype=d, device=dev.device))
                     for k, d in zip(OverlapTable.FIELDS, (pt.int32, pt.int32, pt.int64, pt.int64, pt.float64))}
            edges = OverlapTable(np.zeros(1, dtype=np.int64), **empty)
        return RegionTracks(table, edges, self.n_cells, min_volume, side)

    def extract(self, field, lo=-np.inf, hi=np.inf, weight=None):
        """``label`` and ``table`` in one: the labels stay on the device -> ``RegionTable`` on the side the field came from"""
        labels, shape = self._label(field, lo, hi)
        return self._table(labels, weight, shape, Side(field))
