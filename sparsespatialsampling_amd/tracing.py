"""
Streamlines and pathlines of a velocity field on the NODES of a generated grid (``interpolate_at_vertices=True`` exports), traced on
the GPU.  The reference has nothing of the kind.

The velocity at a position is what ``Probe.sample(velocity, mode="linear")`` returns there, bit for bit: the multilinear blend of the
corner values of the one cell that holds the position.  ``Tracer`` integrates it with classical RK4 (``hipops.trace_stream`` /
``hipops.trace_path``, csrc/trace.hip: one lane per particle carries the whole locate / gather / advance loop; include/s3hip.h has the
definition operation by operation):

    streamlines     of every snapshot of ``velocity`` at once, ``step="cell"``: ``dt = cfl * h / |v|``, about ``cfl`` cell sizes per
                    step whatever the level, or ``step="time"``: a fixed ``dt``; forward, backward or both
    pathlines       through the snapshots, the velocity blended linearly in time, ``substeps`` RK4 steps per snapshot interval; the
                    positions at every snapshot time come back, ``points[:, -1]`` is the flow map

A particle ends where a stage point of a step has no cell (outside the domain, inside a body: ``LEFT``; the path holds only points
inside the grid), where the velocity is zero or not finite under ``step="cell"`` (``STAGNANT``), or after its steps (``DONE``); a seed
that no cell holds gives a path of NaN rows (``SEED_OUTSIDE``).  The blend is continuous across faces between cells of one level; at
hanging nodes of a level jump the velocity has a small discontinuity, as the isosurface has cracks there (documented, not repaired).

    tracer = Tracer.from_dataloader(loader)
    lines = tracer.streamlines(velocity, line(p0, p1, 50), n_steps=400, direction="both")       # points [50, T, 801, d]
    colour = lines.sample(vorticity_at_nodes, mode="linear")                                    # [50, T, 801, T_field]
"""
import numpy as np
import torch as pt

from . import hipops
from .arrays import Side, as_tensor, resident
from .grid import Grid
from .sampling import Probe

STATUS = hipops.TRACE_STATUS        # name -> code of ``Paths.status``


class Paths:
    """what a trace returns, every array on the side the seeds came from:

    ``points``      float64 [n_seeds, (T,) n_out, d]; rows that were never reached are NaN
    ``first``, ``length``   int32 [n_seeds (, T)]: the rows ``first .. first + length - 1`` of a path are valid (``first`` is 0 for a
                    forward trace)
    ``status``      int32 [n_seeds (, T)], the codes of ``STATUS``; with ``direction="both"`` a last axis of two: the backward end,
                    the forward end
    ``cell_ids``    int32, shaped like ``status``: the cell of the last position (-1: the seed had none)
    """

    def __init__(self, tracer, points, first, length, status, cell_ids):
        self._tracer = tracer
        self.points, self.first, self.length, self.status, self.cell_ids = points, first, length, status, cell_ids

    def sample(self, field, mode="linear"):
        """another field of the grid at the recorded positions (``Probe``): [rows, (n_comp,) T_f] -> float64
        ``points.shape[:-1] + field.shape[1:]`` on the side of the field; NaN rows of a path stay NaN"""
        grid = self._tracer.grid
        res = Probe.from_grid(grid, self.points.reshape(-1, grid.dim)).sample(field, mode)
        return res.reshape(tuple(self.points.shape[:-1]) + tuple(res.shape[1:]))


class Tracer:
    """the grid (``centers`` [Nc, d], ``levels`` [Nc] or [Nc, 1], ``width``: the size of the initial cell, ``nodes`` [Nn, d] and
    ``faces`` [Nc, 2^d]: the corner nodes of every cell; numpy or torch, host or device: a ``grid.Grid``, kept as ``grid``; ``from_grid``
    takes one that is there already), indexed once (``hipops.cell_index``; a grid whose cells are no disjoint dyadic boxes on one
    lattice is refused with ``ValueError``).

    ``velocity`` is [Nn, d, T] or [Nn, d] (one snapshot), float32 or float64, numpy or torch; on the device and contiguous it is read
    where it lies (``arrays.resident``).  ``seeds`` [n_seeds, d]; the results come back on their side."""

    def __init__(self, centers, levels, width, nodes, faces):
        self._on(Grid(centers, levels, width, nodes, faces))

    def _on(self, grid):
        if grid.faces is None:
            raise ValueError("a velocity lives on the grid's nodes: build the Grid with nodes and faces")
        self.grid, self.dim, self.n_cells, self.n_nodes = grid, grid.dim, grid.n_cells, grid.n_nodes
        self._index, self._faces = grid.index, grid.faces

    @classmethod
    def from_grid(cls, grid):
        """a ``grid.Grid`` with both parts, which is neither uploaded nor indexed again"""
        self = cls.__new__(cls)
        self._on(grid)
        return self

    @classmethod
    def from_dataloader(cls, loader):
        """the grid of an S^3 file (``data.Dataloader``) exported with ``interpolate_at_vertices=True``"""
        return cls.from_grid(Grid.from_dataloader(loader))

    @classmethod
    def from_s_cube(cls, s_cube):
        """the grid of a ``SparseSpatialSampling`` after ``execute_grid_generation``"""
        return cls.from_grid(Grid.from_s_cube(s_cube))

    # ---- arguments --------------------------------------------------------------------------------------------------------------
    def _velocity(self, velocity, min_snapshots):
        velocity = as_tensor(velocity, "velocity")
        shape = tuple(int(v) for v in velocity.shape)
        if len(shape) not in (2, 3) or shape[0] != self.n_nodes:
            raise ValueError(f"expected a velocity [{self.n_nodes}, {self.dim} (, T)] on the grid's nodes, got {shape}")
        if shape[1] != self.dim:
            raise ValueError(f"a velocity on a {self.dim}-D grid has {self.dim} components, got {shape[1]}")
        if len(shape) == 3 and shape[2] < 1:
            raise ValueError(f"empty velocity {shape}")
        if (shape[2] if len(shape) == 3 else 1) < min_snapshots:
            raise ValueError(f"a pathline needs at least {min_snapshots} snapshots, got a velocity {shape}")
        dev = resident(velocity, pitched=False)
        return dev.reshape(shape[0], shape[1], -1), len(shape) == 2

    def _seeds(self, seeds):
        seeds, side = as_tensor(seeds, "seeds"), Side(seeds)
        if seeds.dim() != 2 or int(seeds.shape[1]) != self.dim:
            raise ValueError(f"expected seeds [n_seeds, {self.dim}], got {tuple(seeds.shape)}")
        return hipops.to_device(seeds, pt.float64), side

    @staticmethod
    def _direction(direction, both=False):
        if direction == "both" and both:
            return (-1, 1)
        if isinstance(direction, str) or direction not in (1, -1):
            raise ValueError(f"direction must be 1, -1{' or both' if both else ''}, got {direction!r}")
        return (int(direction),)

    # ---- traces -----------------------------------------------------------------------------------------------------------------
    def streamlines(self, velocity, seeds, n_steps, step="cell", cfl=0.5, dt=None, direction=1, every=1):
        """``n_steps`` RK4 steps from every seed in every snapshot of ``velocity`` -> ``Paths`` with ``points``
        [n_seeds, T, n_out, d] ([n_seeds, n_out, d] for a velocity [Nn, d]), ``n_out = 1 + n_steps // every``: the seed and every
        ``every``-th accepted step.  ``direction="both"``: the backward and the forward trace joined, ``2 n_out - 1`` rows with the
        seed once, in row ``n_out - 1``."""
        if step not in hipops.TRACE_STEP_RULES:
            raise ValueError(f"unknown step rule {step!r}, expected one of {sorted(hipops.TRACE_STEP_RULES)}")
        if int(n_steps) != n_steps or int(n_steps) < 1:
            raise ValueError(f"n_steps must be a positive count, got {n_steps!r}")
        if int(every) != every or int(every) < 1:
            raise ValueError(f"every must be a positive count, got {every!r}")
        size = dt if step == "time" else cfl
        if size is None or not (np.isfinite(float(size)) and float(size) > 0.0):
            raise ValueError(f"step {step!r} needs a positive finite {'dt' if step == 'time' else 'cfl'}, got {size!r}")
        directions = self._direction(direction, both=True)
        field, single = self._velocity(velocity, 1)
        dev_seeds, side = self._seeds(seeds)
        n_out = 1 + int(n_steps) // int(every)
        if int(dev_seeds.shape[0]) == 0:
            rows = n_out if len(directions) == 1 else 2 * n_out - 1
            shape = (0, int(field.shape[2]))
            ints = pt.empty(shape if len(directions) == 1 else shape + (2,), dtype=pt.int32, device=field.device)
            parts = [pt.empty(shape + (rows, self.dim), dtype=pt.float64, device=field.device), pt.empty(shape, dtype=pt.int32, device=field.device),
                     pt.empty(shape, dtype=pt.int32, device=field.device), ints, ints.clone()]
        else:
            runs = [hipops.trace_stream(self._index, self._faces, field, dev_seeds, int(n_steps), step, cfl, dt, d, int(every))
                    for d in directions]
            if len(runs) == 1:
                points, length, status, cells = runs[0]
                first = pt.zeros_like(length)
            else:
                (pb, lb, sb, cb), (pf, lf, sf, cf) = runs
                points = pt.cat([pb[:, :, 1:].flip(2), pf], dim=2)
                back = (lb - 1).clamp_(min=0)
                first, length = (n_out - 1) - back, back + lf
                status, cells = pt.stack([sb, sf], dim=-1), pt.stack([cb, cf], dim=-1)
            parts = [points, first.to(pt.int32), length.to(pt.int32), status, cells]
        if single:
            parts = [p.squeeze(1) for p in parts]
        return Paths(self, *(side.back(p) for p in parts))

    def pathlines(self, velocity, seeds, dt_snapshot, substeps=4, direction=1, step="time"):
        """particles released at the seeds at the first snapshot (the last one with ``direction=-1``) and carried through the
        snapshots of ``velocity``, ``dt_snapshot`` apart -> ``Paths`` with ``points`` [n_seeds, T, d]: the position at every snapshot
        time, the seed in column 0 (``T - 1`` backward).  A pathline steps in time: ``step="cell"`` is refused."""
        if step != "time":
            raise ValueError(f"a pathline takes substeps of the snapshot spacing (step='time'), got step={step!r}")
        if int(substeps) != substeps or int(substeps) < 1:
            raise ValueError(f"substeps must be a positive count, got {substeps!r}")
        if not (np.isfinite(float(dt_snapshot)) and float(dt_snapshot) > 0.0):
            raise ValueError(f"dt_snapshot must be positive and finite, got {dt_snapshot!r}")
        (d,) = self._direction(direction)
        field, _ = self._velocity(velocity, 2)
        dev_seeds, side = self._seeds(seeds)
        n, t = int(dev_seeds.shape[0]), int(field.shape[2])
        if n == 0:
            ints = pt.empty(0, dtype=pt.int32, device=field.device)
            parts = [pt.empty((0, t, self.dim), dtype=pt.float64, device=field.device), ints, ints.clone(), ints.clone(), ints.clone()]
        else:
            # the seeds are launched in Hilbert order: neighbouring lanes then walk the same cells
            points, length, status, cells = hipops.trace_path(self._index, self._faces, field, dev_seeds, float(dt_snapshot), int(substeps), d,
                                                              order=hipops.spatial_order(dev_seeds))
            first = pt.zeros_like(length) if d > 0 else t - length
            parts = [points, first.to(pt.int32), length, status, cells]
        return Paths(self, *(side.back(p) for p in parts))
