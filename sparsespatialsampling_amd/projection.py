"""
Line-of-sight integrals through a generated grid: the pictures that are integrals along an optical axis -- a schlieren or shadowgraph
image (the integral of ``|grad rho|`` or ``d rho / dy``), a column density, an optical depth, the spanwise average of a 3-D wake
drawn as a 2-D image and, in 2-D, a sinogram or any line average.  The reference has nothing of the kind.

On an S^3 grid the answer is exact and cheap: a cell field is piecewise constant on disjoint dyadic boxes, so its integral along a
line is sum value x chord; a node field blended multilinearly is a polynomial of degree <= d along a line inside one cell, so two
Gauss points per chord integrate it exactly too.  ``Rays`` walks every ray from leaf to leaf on the integer lattice of the cell index
(``hipops.ray_integrate``, csrc/rays.hip, include/s3rays.h), through bodies and holes and across level jumps, 2:1 balance not
assumed, and reads the field once per cell crossed:

    mode="cell"     the field lives on the cells
    mode="linear"   the field lives on the grid NODES (``interpolate_at_vertices=True`` exports); the blend is discontinuous at
                    hanging nodes, as in ``Probe``, and its integral is still exact per cell

    origins, directions, order = parallel(grid, (0, 0, 1), (ny, nx))            # an orthographic bundle along z
    rays = Rays.from_grid(grid, origins, directions, order=order)
    image = rays.integrate(schlieren)[:, 0].reshape(ny, nx)                     # [R, T] -> one snapshot as an image

``parallel`` and ``between`` only build rays on the host.  Not here: maximum / minimum projections, perspective cameras (free rays
serve: give every pixel its own direction), emission-absorption rendering.
"""
import numpy as np
import torch as pt

from . import hipops
from .arrays import Side, as_tensor, resident
from .grid import Grid
from .sampling import _shape, _vector

RAY_OUT_BYTES = 256 << 20           # the largest output [R, n_comp, T_b] f64 of one launch
TILE = 8                            # image pixels are launched in TILE x TILE tiles


# ---- ray builders (host only) -------------------------------------------------------------------------------------------------
def _box(grid, lo, hi):
    if lo is None or hi is None:
        if not isinstance(grid, Grid):
            raise ValueError("parallel: give a Grid, or the window lo and hi")
        g_lo, g_hi = grid.bounds
        lo, hi = g_lo if lo is None else lo, g_hi if hi is None else hi
    lo = _vector(lo, "lo")
    hi = _vector(hi, "hi", lo.size)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
        raise ValueError(f"parallel: [{lo}, {hi}] is no box")
    return lo, hi


def tile_order(shape, tile=TILE):
    """the pixels of an image ``shape = (n1, n2)`` (the last index running fastest) in ``tile`` x ``tile`` tiles, row by row inside a
    tile: the launch order that keeps the rays of a wavefront together -> int32 [n1 * n2], a permutation"""
    n1, n2 = _shape(shape, 2)
    i, j = np.meshgrid(np.arange(n1), np.arange(n2), indexing="ij")
    key = ((i // tile) * ((n2 + tile - 1) // tile) + j // tile) * (tile * tile) + (i % tile) * tile + j % tile
    return np.argsort(key.reshape(-1), kind="stable").astype(np.int32)


def parallel(grid, direction, shape, up=None, lo=None, hi=None):
    """an orthographic bundle: parallel rays along ``direction`` through the pixel centres of an image that covers the lattice domain
    of ``grid`` (``Grid.bounds``) or the window ``[lo, hi]``.  3-D: ``shape = (n1, n2)``, the image axes are ``e1 = e2 x d`` and
    ``e2`` = the part of ``up`` (default: the last coordinate axis not along ``direction``) perpendicular to ``direction``; 2-D:
    ``shape = (n,)`` or ``n``, the one image axis is ``direction`` turned by -90 degrees.  -> (origins f64 [n, d] on the plane through
    the centre of the box, directions f64 [n, d]: ``direction`` as given, order int32 [n]: the pixels in 8 x 8 tiles).  Pixel
    ``(i, j)`` is ray ``i * n2 + j``: the user reshapes results to ``shape``."""
    lo, hi = _box(grid, lo, hi)
    dim = lo.size
    d = _vector(direction, "direction", dim)
    norm = float(np.sqrt((d * d).sum()))
    if not (np.isfinite(norm) and norm > 0.0):
        raise ValueError(f"parallel: direction {d} is no direction")
    unit = d / norm
    shape = _shape(shape, dim - 1)
    if dim == 2:
        axes = [np.array([unit[1], -unit[0]])]
    else:
        if up is None:
            up = np.eye(3)[max(a for a in range(3) if abs(unit[a]) < 0.9)]
        e2 = _vector(up, "up", 3)
        e2 = e2 - (e2 @ unit) * unit
        if not np.sqrt((e2 * e2).sum()) > 1e-12 * max(np.abs(_vector(up, "up", 3)).max(), 1e-300):
            raise ValueError("parallel: up is parallel to the direction")
        e2 = e2 / np.sqrt((e2 * e2).sum())
        axes = [np.cross(e2, unit), e2]
    center = lo + (hi - lo) / 2
    corners = np.array(np.meshgrid(*[[0.0, 1.0]] * dim, indexing="ij")).reshape(dim, -1).T * (hi - lo) + lo - center
    coords = []
    for e, n in zip(axes, shape):
        s = corners @ e
        coords.append(s.min() + (np.arange(n) + 0.5) / n * (s.max() - s.min()))
    mesh = np.meshgrid(*coords, indexing="ij")
    origins = center + sum(m.reshape(-1, 1) * e for m, e in zip(mesh, axes))
    order = tile_order(shape) if dim == 3 else np.arange(shape[0], dtype=np.int32)
    return np.ascontiguousarray(origins), np.tile(d, (len(origins), 1)), order


def between(p0, p1):
    """chords from point to point: ``p0``, ``p1`` [n, d] (or one point [d] against many) -> (origins ``p0``, directions ``p1 - p0``,
    t_range ``(0.0, 1.0)``), float64"""
    p0, p1 = np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64)
    p0, p1 = np.broadcast_arrays(np.atleast_2d(p0), np.atleast_2d(p1))
    if p0.ndim != 2 or p0.shape[1] not in (2, 3):
        raise ValueError(f"between: expected points [n, 2 | 3], got {p0.shape}")
    return np.ascontiguousarray(p0), np.ascontiguousarray(p1 - p0), (0.0, 1.0)


# ---- the rays -----------------------------------------------------------------------------------------------------------------
class Rays:
    """``origins`` and ``directions`` [R, d]: the rays ``x(t) = o + t d`` through the grid (``centers`` [Nc, d], ``levels`` [Nc] or
    [Nc, 1], ``width``: the size of the initial cell; numpy or torch, host or device: a ``grid.Grid``, kept as ``grid``; ``from_grid``
    takes one that is there already).  ``nodes`` and ``faces`` are needed for ``mode="linear"`` only.  ``t_range = (t_min, t_max)``:
    the part of every ray that is integrated, in units of its parameter (default: the whole line).  ``order`` int32 [R]: the launch
    order (``parallel`` returns the tile order of an image); by default the rays are launched in the Hilbert order of the points
    where they enter the lattice domain.  The directions need not be normalised: results are in units of length.

    After ``integrate`` or ``mean``: ``length`` (f64 [R]: the length of every ray inside cells), ``segments`` (int32 [R]: the cells it
    crossed) and ``status`` (int32 [R]: ``hipops.RAY_STATUS`` -- CROSSED, MISSED, BAD_RAY for a ray that is not finite or has no
    direction, TRUNCATED, BROKEN for a grid whose ids are out of range), on the side the origins came from."""

    def __init__(self, centers, levels, width, origins, directions, nodes=None, faces=None, t_range=None, order=None):
        self._on(Grid(centers, levels, width, nodes, faces), origins, directions, t_range, order)

    def _on(self, grid, origins, directions, t_range, order):
        self._side = Side(origins)
        origins, directions = as_tensor(origins, "origins"), as_tensor(directions, "directions")
        self.grid, self.dim, self.n_cells, self.n_nodes = grid, grid.dim, grid.n_cells, grid.n_nodes
        if origins.dim() != 2 or int(origins.shape[1]) != self.dim or tuple(directions.shape) != tuple(origins.shape):
            raise ValueError(f"expected origins and directions [R, {self.dim}], got {tuple(origins.shape)} and {tuple(directions.shape)}")
        self.n_rays = int(origins.shape[0])
        t_min, t_max = (-np.inf, np.inf) if t_range is None else (float(v) for v in t_range)
        if not t_min <= t_max:
            raise ValueError(f"t_range {t_range!r} is no range of the ray parameter")
        self.t_range = (t_min, t_max)
        self._index = grid.index
        self._origins, self._dirs = hipops.to_device(origins, pt.float64), hipops.to_device(directions, pt.float64)
        if order is not None:
            order = as_tensor(order, "order")
            if order.is_floating_point() or order.numel() != self.n_rays or order.dim() != 1:
                raise ValueError(f"expected an integer order [{self.n_rays}], got {tuple(order.shape)} {order.dtype}")
            host = order.detach().cpu().numpy().astype(np.int64)
            if self.n_rays and (host.min() < 0 or host.max() >= self.n_rays or np.bincount(host, minlength=self.n_rays).min() != 1):
                raise ValueError("order must be a permutation of the rays")
            self._order = hipops.to_device(order, pt.int32)
        elif self.n_rays:
            self._order = hipops.spatial_order(self._entry_points())
        else:
            self._order = None
        self.length = self.segments = self.status = None

    def _entry_points(self):
        """where every ray enters the lattice domain (its origin clamped into the domain where it does not), on the device"""
        lo, hi = self.grid.bounds
        lo, hi = pt.from_numpy(lo).to(self._origins.device), pt.from_numpy(hi).to(self._origins.device)
        o, d = self._origins, self._dirs
        safe = pt.where(d != 0, d, pt.ones_like(d))
        near = pt.where(d > 0, lo - o, hi - o) / safe
        near = pt.where(d != 0, near, pt.full_like(near, -np.inf)).amax(dim=1).clamp_(min=self.t_range[0])
        near = pt.where(pt.isfinite(near), near, pt.zeros_like(near))
        entry = pt.nan_to_num(o + near[:, None] * d, nan=0.0, posinf=0.0, neginf=0.0)
        return pt.maximum(pt.minimum(entry, hi), lo).contiguous()

    @classmethod
    def from_grid(cls, grid, origins, directions, t_range=None, order=None):
        """rays through a ``grid.Grid``, which is neither uploaded nor indexed again"""
        self = cls.__new__(cls)
        self._on(grid, origins, directions, t_range, order)
        return self

    @classmethod
    def from_dataloader(cls, loader, origins, directions, t_range=None, order=None):
        """the grid of an S^3 file (``data.Dataloader``)"""
        return cls.from_grid(Grid.from_dataloader(loader), origins, directions, t_range, order)

    @classmethod
    def from_s_cube(cls, s_cube, origins, directions, t_range=None, order=None):
        """the grid of a ``SparseSpatialSampling`` after ``execute_grid_generation``"""
        return cls.from_grid(Grid.from_s_cube(s_cube), origins, directions, t_range, order)

    def _field(self, field, mode):
        if mode not in hipops.RAY_MODES:
            raise ValueError(f"unknown mode {mode!r}, expected one of {sorted(hipops.RAY_MODES)}")
        if mode == "linear" and self.grid.faces is None:
            raise ValueError("mode 'linear' blends the corner values of a cell: build the Rays with nodes and faces")
        side = Side(field)
        field = as_tensor(field, "field")
        shape = tuple(int(v) for v in field.shape)
        n_rows = self.n_cells if mode == "cell" else self.n_nodes
        if not 1 <= len(shape) <= 3 or shape[0] != n_rows:
            raise ValueError(f"{mode}: expected a field [{n_rows}, (n_comp,) T] on the grid's {'cells' if mode == 'cell' else 'nodes'}, got {shape}")
        if 0 in shape:
            raise ValueError(f"{mode}: empty field {shape}")
        return resident(field), shape, side

    def integrate(self, field, mode="cell", max_steps=None, out_bytes=RAY_OUT_BYTES):
        """the integral of ``field`` [rows, (n_comp,) T] (``[rows]``: one snapshot; rows = cells for ``mode="cell"``, nodes for
        ``mode="linear"``; float32 or float64, numpy or torch, host or device; on the device, and a snapshot window ``field[:, t0:t1]``
        of a scalar field too, it is read where it lies) along every ray -> float64 [R, (n_comp,) T] on the side the field came from:
        0 for a ray that misses, NaN for a bad ray.  The snapshots go in batches whose output stays below ``out_bytes``.  A ray that
        is still walking after ``max_steps`` blocks raises ``RuntimeError`` unless ``max_steps`` was given: then its status says
        TRUNCATED and what it had summed is returned."""
        dev_field, shape, side = self._field(field, mode)
        steps = hipops.RAY_MAX_STEPS if max_steps is None else int(max_steps)
        if steps < 1:
            raise ValueError(f"max_steps must be positive, got {max_steps!r}")
        n_comp, t = (shape[1] if len(shape) == 3 else 1), (shape[-1] if len(shape) > 1 else 1)
        res = pt.empty((self.n_rays, n_comp, t), dtype=pt.float64, device=dev_field.device)
        state = [pt.empty(self.n_rays, dtype=dt, device=dev_field.device) for dt in (pt.float64, pt.int32, pt.int32)]
        if self.n_rays:
            per_col = max(self.n_rays * n_comp * 8, 1)
            t_b = int(max(1, min(t, out_bytes // per_col, ((1 << 31) - 1) // self.n_rays)))
            launch = dict(mode=mode, faces=self.grid.faces if mode == "linear" else None, t_range=self.t_range, order=self._order, max_steps=steps,
                          length=state[0], segments=state[1], status=state[2])
            if t_b >= t:
                hipops.ray_integrate(self._index, self._origins, self._dirs, dev_field, out=res, **launch)
            else:
                # windows of the snapshots, component by component: field[:, c, t0:t1] is a pitched 2-D view, read where it lies
                rows = dev_field.reshape(shape[0], n_comp, t)
                for t0 in range(0, t, t_b):
                    t1 = min(t, t0 + t_b)
                    for c in range(n_comp):
                        part = hipops.ray_integrate(self._index, self._origins, self._dirs, rows[:, c, t0:t1], **launch)[0]
                        res[:, c, t0:t1] = part[:, 0]
            if max_steps is None and bool((state[2] == hipops.RAY_STATUS["TRUNCATED"]).any()):
                raise RuntimeError(f"rays were still walking after {steps} blocks: pass max_steps to allow more, or to accept the truncated sums")
        self.length, self.segments, self.status = (self._side.back(v) for v in state)
        self._length = state[0]
        return side.back(res.view((self.n_rays,) + shape[1:]))

    def mean(self, field, mode="cell", max_steps=None, out_bytes=RAY_OUT_BYTES):
        """the line average: ``integrate`` divided by ``length``, NaN where the length is 0"""
        dev_field, shape, side = self._field(field, mode)
        res = self.integrate(dev_field, mode, max_steps, out_bytes)
        res = res / self._length.view((self.n_rays,) + (1,) * (len(shape) - 1))         # (0 / 0: NaN)
        return side.back(res)
