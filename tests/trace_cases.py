"""
Cases and references for the particle tracer of csrc/trace.hip (CPU only: numpy, long double).  The grids are those of
tests/sample_cases.py.

The definition (include/s3hip.h is normative; csrc/trace.hip restates it):
    velocity    at x in column t: the cell s3_cell_locate gives x, the S3_SAMPLE_LINEAR blend of its corner rows there
    time        pathlines: v = v_n + theta (v_{n+1} - v_n) in one cell; the stage s in {0, 1/2, 1} of step m of the interval [c, c+1]
                sits at p / (2 substeps), p = 2m + 2s forward, 2 substeps - (2m + 2s) backward; p < 2 substeps: n = c, theta = p / (2
                substeps); else n = c + 1, theta = 0; where n is the last column n = T - 2, theta = 1
    step        RK4: x2 = x + dt/2 k1, x3 = x + dt/2 k2, x4 = x + dt k3, x' = x + dt/6 ((k1 + k4) + 2 (k2 + k3)), each update one fma
    step size   "time": dt = direction * step; "cell": dt = direction * (step * h(cell of x)) / |k1|
    the end     seed without a cell: SEED_OUTSIDE, length 0; a step counts only when x2, x3, x4 and x' all have a cell, else LEFT at x;
                "cell" with |k1| zero or not finite: STAGNANT; else DONE.  Row 0 is the seed, row r the position after r * every
                accepted steps, `length` the rows written, NaN after them.

References:
    rk4_oracle          the definition in long double on an ANALYTIC field, no blend and no node values; the grid enters only through
                        ``Grid.locate_exact`` (which cell holds a point, its size, and how far the point is from the cell's faces)
    grid_step_oracle    one step on a grid with arbitrary node values: brute-force location, the blend in long double
    emulate_trace       the definition in plain float64 numpy (a multiply and an add where the kernel has an fma), with the planted
                        mistakes of ``MISTAKES``

THE TWO BOUNDS (both come from the emulation and the arithmetic, never from the GPU code).

Affine bound.  A field v = A x + b(t), b linear in t, is reproduced by the multilinear blend on any grid, hanging nodes included, and
by the blend in time, so tracer and ``rk4_oracle`` integrate the same field with the same scheme and differ by rounding alone: per
step a few roundings of size u |x| (u = 2^-53; the node values, the blend, the fma of the update), and what earlier steps left grows
at most like exp(||A|| * elapsed time), the Lipschitz growth of the exact flow and of RK4 on it.  After r steps
    |x_r - X_r|  <=  r * K * u * max|x| * exp(||A||_2 * sum |dt|),        max|x| = the largest |coordinate| of a node of the grid
``K_EMULATION`` is the largest K the plain-float64 emulation needs over every case of ``AFFINE_RUNS`` and ``PATH_RUNS`` (measured by
tests/test_trace_checker.py, which asserts it), rounded up; the GPU's explicit fma differs from numpy's separate multiply and add in
up to three roundings per update, so the tests use K = 8 * K_EMULATION.

One-step bound on a random node field (no smoothness: every error is first order in u).  With L = (largest difference of two corner
values of the cell) / h, the Lipschitz constant of the blend inside a cell per axis, mag_s = sum_m |w_m f_m| at stage s, and
pos(x) = u (|x| + |c| + 2h) summed over the axes (the roundings of c - h/2, x - (c - h/2) and the quotient in xi, as a shift of x):
    e_s   = (2^d + 3) u mag_s + L (dx_s + pos(x_s))                      ``sample_cases.linear_bound`` at a shifted position
    dx_1  = 0      dx_2 = |dt/2| e_1 + u |x2|      dx_3 = |dt/2| e_2 + u |x3|      dx_4 = |dt| e_3 + u |x4|        (summed over axes)
    B     = |dt/6| (e_1 + 2 e_2 + 2 e_3 + e_4) + 5 u |dt/6| (|k1| + 2|k2| + 2|k3| + |k4|) + u |x'|
(the 5 u: three additions, the rounding of dt/6 and, in the emulation, of the product).  B bounds the emulation as it stands
(ONE_STEP_EMULATION = 1; the largest error / B it shows is 0.85, tree2d, asserted by the checker test to stay below 1); the GPU tests
use ONE_STEP_MARGIN * B = 8 B, the same margin as above.
Seeds with a stage point within 1e-6 cell sizes of a face are left out: there the cell decision itself may differ.
"""
import functools

import numpy as np

from tests import sample_cases as sc

LD = sc.LD
U = LD(2) ** -53
DONE, LEFT, STAGNANT, SEED_OUTSIDE = 0, 1, 2, 3
GRIDS = ["tree2d", "tree3d", "golden2d", "offset2d", "dyadic2d", "dyadic3d", "level3", "one_cell"]
NS = sc.NQ              # 3001 seeds: twelve workgroups of 256, the last one ragged
FACE_MARGIN = 1e-6      # cell sizes: closer to a face, the cell of a point is not asserted
EXCLUDED_CAP = 0.01
MISTAKES = ["k2_full_step", "equal_weights", "nearest_centre", "frozen_time", "left_by_end_point"]

K_EMULATION = 1.0       # the largest K tests/test_trace_checker.py sees is 0.83 (golden2d); that test asserts this figure
K_AFFINE = 8 * K_EMULATION
ONE_STEP_EMULATION = 1.0    # B is a bound: the emulation must stay inside it as it is (largest ratio seen: see the checker test)
ONE_STEP_MARGIN = 8 * ONE_STEP_EMULATION


# ---- grids ---------------------------------------------------------------------------------------------------------------------
class Grid:
    """a case of tests/sample_cases.py with what the references need, computed once"""

    def __init__(self, name):
        self.name, self.c = name, sc.case(name)
        c = self.c
        self.d, self.n_cells, self.n_nodes = c["centers"].shape[1], len(c["levels"]), len(c["nodes"])
        self.ix = sc.emulate_index(c)
        self.h = sc.cell_sizes(c)
        self.h_ld = LD(c["width"]) / LD(2) ** c["levels"].astype(LD)
        self.lo_ld = c["centers"].astype(LD) - self.h_ld[:, None] / 2
        self.max_x = float(np.abs(c["nodes"]).max())
        self.box_lo, self.box_hi = c["nodes"].min(axis=0), c["nodes"].max(axis=0)
        self.degenerate = bool(c["degenerate"])

    # the definition in float64 (sample_cases.emulate_locate with the index kept)
    def locate(self, q):
        ix = self.ix
        with np.errstate(invalid="ignore", over="ignore"):
            t = np.floor((q - ix["origin"]) / ix["h_min"])
            ok = ((t >= 0) & (t < 2.0 ** ix["depth"])).all(axis=1)
        key = sc.morton(np.where(ok[:, None], t, 0).astype(np.uint64), self.d, ix["depth"])
        pos = np.searchsorted(ix["starts"], key, side="right") - 1
        hit = ok & (pos >= 0)
        hit[hit] &= key[hit] < ix["ends"][pos[hit]]
        return np.where(hit, ix["ids"][np.maximum(pos, 0)], -1).astype(np.int32)

    def locate_exact(self, q):
        """q long double [n, d] -> (ids by the long-double box test, margin [n]: the distance to the nearest face of the cell, or
        for a point without a cell to the nearest cell, in units of that cell's size).  The float64 lattice search proposes, the
        long-double test decides; where they disagree, and for points without a cell, every cell is tried."""
        ids = self.locate(q.astype(np.float64))
        safe = np.maximum(ids, 0)
        xi = (q - self.lo_ld[safe]) / self.h_ld[safe][:, None]
        good = (ids >= 0) & ((xi >= 0) & (xi < 1)).all(axis=1)
        margin = np.minimum(xi, 1 - xi).min(axis=1)
        ids = np.where(good, ids, -1)
        for j in np.flatnonzero(~good):
            if not np.isfinite(q[j].astype(np.float64)).all():
                margin[j] = np.inf
                continue
            x = (q[j][None] - self.lo_ld) / self.h_ld[:, None]                  # [n_cells, d]
            inside = ((x >= 0) & (x < 1)).all(axis=1)
            if inside.any():
                k = int(np.argmax(inside))
                ids[j], margin[j] = k, np.minimum(x[k], 1 - x[k]).min()
            else:
                margin[j] = np.maximum(np.maximum(-x, x - 1), 0).max(axis=1).min()
        return ids, margin.astype(np.float64)


@functools.lru_cache(maxsize=None)
def grid(name):
    return Grid(name)


@functools.lru_cache(maxsize=None)
def seeds(name, n=NS):
    """uniform in the bounding box of the grid, widened by a twentieth on every side: some seeds outside, some in holes"""
    g = grid(name)
    rng = np.random.default_rng(1000 + len(name) * 13 + g.d)
    ext = g.box_hi - g.box_lo
    return g.box_lo - 0.05 * ext + 1.1 * ext * rng.random((n, g.d))


# ---- analytic fields -------------------------------------------------------------------------------------------------------------
class Affine:
    """v(x, tau) = A (x - x_c) + b0 + b1 tau (tau in snapshot intervals); ``norm`` = ||A||_2"""

    def __init__(self, g, b1_scale=0.0, seed=0):
        ext = float((g.box_hi - g.box_lo).max())
        self.center = (g.box_lo + g.box_hi) / 2
        if g.d == 2:                    # rotation plus shear plus translation
            self.a = np.array([[0.0, -1.0], [1.0, 0.0]]) + np.array([[0.0, 0.35], [0.0, 0.0]])
            self.b0 = np.array([0.21, -0.08]) * ext
        else:                           # a helix about the z axis through the centre
            self.a = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
            self.b0 = np.array([0.0, 0.0, 0.3]) * ext
        self.b1 = b1_scale * ext * np.random.default_rng(seed).uniform(-1, 1, g.d)
        self.norm = float(np.linalg.norm(self.a, 2))
        self.speed = float(np.abs(self.a).sum(axis=1).max() * ext / 2 + np.abs(self.b0).max())

    def __call__(self, x, tau=0):
        tau = np.asarray(tau, dtype=LD)
        return (x - self.center.astype(LD)) @ self.a.T.astype(LD) + self.b0.astype(LD) + self.b1.astype(LD) * tau[..., None]

    def nodes(self, g, n_snapshots=None):
        """the field at the nodes, in long double, rounded once: [nn, d] or [nn, d, T]"""
        x = g.c["nodes"].astype(LD)
        if n_snapshots is None:
            return self(x).astype(np.float64)
        return np.stack([self(x, t) for t in range(n_snapshots)], axis=-1).astype(np.float64)


def affine_bound(g, field, steps, elapsed):
    """steps, elapsed: arrays of one shape -> the affine bound WITHOUT K"""
    return steps.astype(LD) * U * LD(g.max_x) * np.exp(LD(field.norm) * elapsed.astype(LD))


# (case, step rule, step, n_steps): the step sizes move a particle about 0.45 cell sizes per step; n_steps keeps some of them inside
def affine_runs():
    runs = []
    for name in GRIDS:
        g = grid(name)
        n_cell = {"one_cell": 1, "level3": 4, "offset2d": 5}.get(name, 12)
        runs.append((name, "cell", 0.45, n_cell))
        dt = 0.45 * float(np.median(g.h)) / Affine(g).speed
        runs.append((name, "time", dt, {"one_cell": 2}.get(name, 24)))
    return runs


AFFINE_RUNS = affine_runs()
PATH_RUNS = [(name, 5, 4) for name in GRIDS]                    # (case, snapshots, substeps)


def path_dt(g):
    """the snapshot spacing of the pathline cases: about two median cell sizes per interval at the largest speed (one_cell: a tenth of the cell)"""
    return (0.1 if g.name == "one_cell" else 2.0) * float(np.median(g.h)) / Affine(g).speed


# ---- the oracle on an analytic field ---------------------------------------------------------------------------------------------
def stage_time(c, p, s2, last):
    """(n, theta) of the definition; long double theta"""
    n, theta = (c + 1, LD(0)) if p == s2 else (c, LD(p) / LD(s2))
    return (last - 1, LD(1)) if n >= last else (n, theta)


def rk4_oracle(field_fn, x, n_steps, rule, step, direction, g=None, substeps=None, n_snapshots=None):
    """the definition in long double on ``field_fn(x [n, d], tau) -> v`` (tau: snapshot time, 0 for a steady field).  ``g``: the grid
    that ends particles and gives the cell size (None: free space, time rule only).  ``substeps``: a pathline through
    ``n_snapshots`` snapshots, ``n_steps`` is ignored.  -> dict(points [n, n_steps + 1, d] NaN past the end, length (points
    recorded with every = 1), status, margin [n] (the least ``locate_exact`` margin over every point the particle located),
    elapsed [n, n_steps + 1] (sum of |dt|))"""
    x = np.asarray(x, dtype=LD).copy()
    n, d = x.shape
    if substeps is not None:
        n_steps = (n_snapshots - 1) * substeps
    points = np.full((n, n_steps + 1, d), np.nan, dtype=LD)
    elapsed = np.zeros((n, n_steps + 1), dtype=LD)
    length, status = np.zeros(n, dtype=np.int64), np.full(n, DONE, dtype=np.int64)
    margin = np.full(n, np.inf)

    def locate(idx, pts):
        if g is None:
            return np.zeros(len(idx), dtype=np.int64)
        ids, m = g.locate_exact(pts)
        margin[idx] = np.minimum(margin[idx], m)
        return ids

    act = np.arange(n)
    with np.errstate(invalid="ignore", over="ignore"):
        ids = locate(act, x)
    status[ids < 0] = SEED_OUTSIDE
    act, cell = act[ids >= 0], ids[ids >= 0]
    points[act, 0], length[act] = x[act], 1
    for s in range(n_steps):
        if not len(act):
            break
        if substeps is None:
            taus = [LD(0)] * 3
        else:
            k, m = divmod(s, substeps)
            last, s2 = n_snapshots - 1, 2 * substeps
            c = last - 1 - k if direction < 0 else k
            taus = []
            for half in (0, 1, 2):
                p = s2 - (2 * m + half) if direction < 0 else 2 * m + half
                nn, theta = stage_time(c, p, s2, last)
                taus.append(LD(nn) + theta)
        xa = x[act]
        k1 = field_fn(xa, taus[0])
        if rule == "cell":
            norm = np.sqrt((k1 * k1).sum(axis=1))
            stag = ~((norm > 0) & np.isfinite(norm.astype(np.float64)))
            status[act[stag]] = STAGNANT
            act, cell, xa, k1, norm = act[~stag], cell[~stag], xa[~stag], k1[~stag], norm[~stag]
            dt = (LD(step) * g.h_ld[cell] / norm)[:, None]
        else:
            dt = np.full((len(act), 1), LD(step))
        dt = dt * direction
        alive = np.ones(len(act), dtype=bool)
        x2 = xa + dt / 2 * k1
        alive &= locate(act, x2) >= 0
        k2 = field_fn(x2, taus[1])
        x3 = xa + dt / 2 * k2
        alive[alive] &= locate(act[alive], x3[alive]) >= 0
        k3 = field_fn(x3, taus[1])
        x4 = xa + dt * k3
        alive[alive] &= locate(act[alive], x4[alive]) >= 0
        k4 = field_fn(x4, taus[2])
        xn = xa + dt / 6 * ((k1 + k4) + 2 * (k2 + k3))
        new_cell = np.full(len(act), -1, dtype=np.int64)
        new_cell[alive] = locate(act[alive], xn[alive])
        alive &= new_cell >= 0
        status[act[~alive]] = LEFT
        act, cell = act[alive], new_cell[alive]
        x[act] = xn[alive]
        points[act, s + 1], length[act] = x[act], s + 2
        elapsed[act, s + 1] = elapsed[act, s] + np.abs(dt[alive, 0])
    return {"points": points, "length": length, "status": status, "margin": margin, "elapsed": elapsed}


def recorded(length, every):
    """the rows a particle of ``length`` (every = 1) writes when every ``every``-th accepted step is recorded"""
    return np.where(length > 0, 1 + (length - 1) // every, 0)


# ---- the blend on a grid -----------------------------------------------------------------------------------------------------------
def blend_ld(g, ids, x, node_field):
    """long double: (value [n, d], mag [n, d], lipschitz [n]) of the blend of ``node_field`` [nn, d] at x in the cells ``ids``"""
    signs = sc.corner_signs(g.d)
    xi = np.clip((x - g.lo_ld[ids]) / g.h_ld[ids][:, None], 0, 1)
    w = np.ones((len(x), 1 << g.d), dtype=LD)
    for a in range(g.d):
        w *= np.where(signs[None, :, a] > 0, xi[:, a:a + 1], 1 - xi[:, a:a + 1])
    f = node_field[g.c["faces"][ids]].astype(LD)                                # [n, 2^d, d]
    wf = w[:, :, None] * f
    lip = (f.max(axis=1) - f.min(axis=1)).max(axis=1) / g.h_ld[ids]
    return wf.sum(axis=1), np.abs(wf).sum(axis=1), lip


def grid_step_oracle(g, node_velocity, x, rule, step, direction):
    """one step from the float64 positions x [n, d] through ``node_velocity`` [nn, d] (float64 or float32 values): the cell by the
    long-double box test and the long-double blend at every stage.  The seeds are located by ``sample_cases.brute_force``; the later
    stage points by ``Grid.locate_exact``, which decides by the same long-double test and tries every cell wherever the float64
    search it starts from proposes none or a wrong one -- a fraction of the time, and asserted here to agree on the seeds.  -> dict(end [n, d] long double, ok [n]: all
    five points have a cell and |k1| is positive, cells [n, 5] (x, x2, x3, x4, x'), margin [n]: the least distance of a stage point
    to a face of its cell in cell sizes (0 where a point has no cell), bound [n, d]: B of the module docstring)"""
    n, d = x.shape
    xs = x.astype(LD)
    node_velocity = np.asarray(node_velocity, dtype=np.float64)
    cells = np.full((n, 5), -1, dtype=np.int64)
    margin = np.full(n, np.inf)
    ok = np.ones(n, dtype=bool)

    def locate(stage, pts):
        live = np.flatnonzero(ok)                                               # (a particle that lost its cell is followed no further)
        ids = np.full(n, -1, dtype=np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            ids[live] = g.locate_exact(pts[live])[0]
        if stage == 0:
            assert np.array_equal(ids, sc.brute_force(g.c, x)[0])
        safe = np.maximum(ids, 0)
        xi = (pts - g.lo_ld[safe]) / g.h_ld[safe][:, None]
        good = (ids >= 0) & ((xi >= 0) & (xi < 1)).all(axis=1)
        m = np.where(good, np.minimum(xi, 1 - xi).min(axis=1), 0).astype(np.float64)
        cells[:, stage] = np.where(good, ids, -1)
        margin[:] = np.minimum(margin, m)
        ok[:] &= good
        return safe

    def pos_u(pts, ids):
        return (U * (np.abs(pts) + np.abs(g.c["centers"][ids].astype(LD)) + 2 * g.h_ld[ids][:, None])).sum(axis=1)

    nd = (1 << d) + 3
    c1 = locate(0, xs)
    k1, mag, lip = blend_ld(g, c1, xs, node_velocity)
    e1 = nd * U * mag + (lip * pos_u(xs, c1))[:, None]
    if rule == "cell":
        norm = np.sqrt((k1 * k1).sum(axis=1))
        ok &= (norm > 0).astype(bool)
        dt = (LD(step) * g.h_ld[c1] / np.where(norm > 0, norm, 1))[:, None] * direction
    else:
        dt = np.full((n, 1), LD(step) * direction)
    adt = np.abs(dt)
    x2 = xs + dt / 2 * k1
    c2 = locate(1, x2)
    k2, mag, lip = blend_ld(g, c2, x2, node_velocity)
    dx = (adt / 2 * e1 + U * np.abs(x2)).sum(axis=1)
    e2 = nd * U * mag + (lip * (dx + pos_u(x2, c2)))[:, None]
    x3 = xs + dt / 2 * k2
    c3 = locate(2, x3)
    k3, mag, lip = blend_ld(g, c3, x3, node_velocity)
    dx = (adt / 2 * e2 + U * np.abs(x3)).sum(axis=1)
    e3 = nd * U * mag + (lip * (dx + pos_u(x3, c3)))[:, None]
    x4 = xs + dt * k3
    c4 = locate(3, x4)
    k4, mag, lip = blend_ld(g, c4, x4, node_velocity)
    dx = (adt * e3 + U * np.abs(x4)).sum(axis=1)
    e4 = nd * U * mag + (lip * (dx + pos_u(x4, c4)))[:, None]
    end = xs + dt / 6 * ((k1 + k4) + 2 * (k2 + k3))
    locate(4, end)
    bound = adt / 6 * (e1 + 2 * e2 + 2 * e3 + e4) + 5 * U * adt / 6 * (np.abs(k1) + 2 * np.abs(k2) + 2 * np.abs(k3) + np.abs(k4)) + U * np.abs(end)
    return {"end": end, "ok": ok, "cells": cells, "margin": margin, "bound": bound}


def random_nodes(g, seed, f32=False, n_snapshots=None):
    """standard normal node values scaled so that a step of the time rule stays local; [nn, d] or [nn, d, T]"""
    shape = (g.n_nodes, g.d) if n_snapshots is None else (g.n_nodes, g.d, n_snapshots)
    f = np.random.default_rng(seed).standard_normal(shape)
    return f.astype(np.float32) if f32 else f


# ---- the definition in float64 -----------------------------------------------------------------------------------------------------
def emulate_trace(g, field, x, n_steps, rule, step, direction=1, every=1, column=0, substeps=None, mistake=None):
    """the definition in plain float64 numpy (a*b + c where the kernel has fma(a, b, c)).  ``field`` [nn, d, T]; streamlines of column
    ``column``, or with ``substeps`` pathlines through all T columns (``n_steps`` and ``every`` are ignored).  ``mistake``: one of
    ``MISTAKES``.  -> dict(points [n, n_out, d], length, status, cells, accepted: steps accepted, crossed: of them into another
    cell, jumped: of them into a cell of another level)"""
    field = np.asarray(field, dtype=np.float64)
    x = np.array(x, dtype=np.float64)
    n, d = x.shape
    t_cols = field.shape[2]
    path = substeps is not None
    if path:
        n_steps, every = (t_cols - 1) * substeps, substeps
    n_out = 1 + n_steps // every
    signs = sc.corner_signs(d)
    faces, centers, levels = g.c["faces"], g.c["centers"], g.c["levels"]
    points = np.full((n, n_out, d), np.nan)
    length, status, cells = np.zeros(n, dtype=np.int32), np.full(n, DONE, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    stats = {"accepted": 0, "crossed": 0, "jumped": 0}

    def locate(q):
        with np.errstate(invalid="ignore", over="ignore"):
            ids = g.locate(q)
            if mistake == "nearest_centre":
                near = sc.nearest_center(g.c, np.nan_to_num(q))
                ids = np.where(ids >= 0, near, -1).astype(np.int32)
        return ids

    def blend(ids, q, col):
        h = g.h[ids][:, None]
        xi = np.clip((q - (centers[ids] - h / 2)) / h, 0.0, 1.0)
        acc = np.zeros((len(q), d))
        for m in range(1 << d):
            if mistake == "equal_weights":
                w = np.full(len(q), 1.0 / (1 << d))
            else:
                w = xi[:, 0] if signs[m, 0] > 0 else 1.0 - xi[:, 0]
                for a in range(1, d):
                    w = w * xi[:, a] if signs[m, a] > 0 else w - xi[:, a] * w
            acc = acc + w[:, None] * field[faces[ids, m], :, col]
        return acc

    def velocity(ids, q, n_col, theta):
        if not path:
            return blend(ids, q, column)
        v0 = blend(ids, q, n_col)
        if mistake == "frozen_time":
            return v0
        return v0 + theta * (blend(ids, q, n_col + 1) - v0)

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ids = locate(x)
        status[ids < 0] = SEED_OUTSIDE
        act = np.flatnonzero(ids >= 0)
        cell = ids[act].astype(np.int64)
        cells[act] = cell
        points[act, 0], length[act] = x[act], 1
        for s in range(n_steps):
            if not len(act):
                break
            times = [(0, 0.0)] * 3
            if path:
                k, m = divmod(s, substeps)
                last, s2 = t_cols - 1, 2 * substeps
                c = last - 1 - k if direction < 0 else k
                times = []
                for half in (0, 1, 2):
                    nn, theta = stage_time(c, s2 - (2 * m + half) if direction < 0 else 2 * m + half, s2, last)
                    times.append((nn, float(theta)))
            xa = x[act]
            k1 = velocity(cell, xa, *times[0])
            if rule == "cell":
                sq = k1[:, 0] * k1[:, 0]
                for a in range(1, d):
                    sq = sq + k1[:, a] * k1[:, a]
                norm = np.sqrt(sq)
                stag = ~((norm > 0) & (norm < np.inf))
                status[act[stag]] = STAGNANT
                act, cell, xa, k1, norm = act[~stag], cell[~stag], xa[~stag], k1[~stag], norm[~stag]
                dt = ((step * g.h[cell]) / norm)[:, None]
            else:
                dt = np.full((len(act), 1), float(step))
            if direction < 0:
                dt = -dt
            alive = np.ones(len(act), dtype=bool)

            def stage(q, when):
                ids = locate(q)
                if mistake == "left_by_end_point":          # a stage point without a cell takes the velocity of the cell of x
                    ids = np.where(ids >= 0, ids, cell)
                alive[:] &= ids >= 0
                return velocity(np.maximum(ids, 0), q, *when)

            k2 = stage(xa + dt * k1 if mistake == "k2_full_step" else xa + dt / 2 * k1, times[1])
            k3 = stage(xa + dt / 2 * k2, times[1])
            k4 = stage(xa + dt * k3, times[2])
            xn = xa + dt / 6 * ((k1 + k4) + 2.0 * (k2 + k3))
            new_cell = locate(xn).astype(np.int64)
            alive &= new_cell >= 0
            status[act[~alive]] = LEFT
            moved = alive & (new_cell != cell)
            stats["accepted"] += int(alive.sum())
            stats["crossed"] += int(moved.sum())
            stats["jumped"] += int((moved & (levels[np.maximum(new_cell, 0)] != levels[cell])).sum())
            act, cell = act[alive], new_cell[alive]
            x[act] = xn[alive]
            cells[act] = cell
            if (s + 1) % every == 0:
                points[act, (s + 1) // every] = x[act]
                length[act] = (s + 1) // every + 1
    if path and direction < 0:
        points = points[:, ::-1]
    return dict(stats, points=points, length=length, status=status, cells=cells)


# ---- comparing a trace with the oracle ---------------------------------------------------------------------------------------------
def violation(points, ref, bound, common=False):
    """the largest |points - ref| / bound over the rows the reference has; inf where a row exists on one side only (``common``: such
    rows are passed over instead)"""
    have, want = ~np.isnan(points).any(axis=-1), ~np.isnan(ref.astype(np.float64)).any(axis=-1)
    if common:
        want = want & have
    elif (have != want).any():
        return np.inf
    if not want.any():
        return 0.0
    err = np.abs(points[want].astype(LD) - ref[want])
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(err == 0, 0, err / bound[want][:, None]).max())


# ---- the exact case ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_case(name, n_steps=9):
    """dyadic grid, velocity (2^-3, 0 (, 0)) at every node, displacement 2^-(L+1) per step (half a finest cell), seeds on the faces
    and half-way between them (``sample_cases.face_queries``): every operation of the definition is exact, so the prediction is
    integer arithmetic in units of 2^-(L+2) -- done here in float64, which holds these numbers exactly, with the brute-force locate.
    -> dict(field [nn, d, 1], seeds, dt (time rule), cfl (cell rule: dt = cfl * h / 2^-3 with h of the cell of x), n_steps,
    time / cell: (points, length, status))"""
    g = grid(name)
    depth = int(g.c["levels"].max())
    speed, delta = 2.0 ** -3, 2.0 ** -(depth + 1)
    field = np.zeros((g.n_nodes, g.d, 1))
    field[:, 0, 0] = speed
    x0 = g.c["queries"]
    out = {"field": field, "seeds": x0, "dt": delta / speed, "cfl": 0.5, "n_steps": n_steps}
    for rule in ("time", "cell"):
        x = x0.copy()
        points = np.full((len(x), n_steps + 1, g.d), np.nan)
        length, status = np.zeros(len(x), dtype=np.int32), np.full(len(x), DONE, dtype=np.int32)
        ids = sc.brute_force(g.c, x)[0]
        status[ids < 0] = SEED_OUTSIDE
        act = np.flatnonzero(ids >= 0)
        cell = ids[act]
        points[act, 0], length[act] = x[act], 1
        for s in range(n_steps):
            step = np.zeros((len(act), g.d))
            step[:, 0] = delta if rule == "time" else 0.5 * g.h[cell]
            alive = np.ones(len(act), dtype=bool)
            for frac in (0.5, 1.0):
                alive &= sc.brute_force(g.c, x[act] + frac * step)[0] >= 0
            status[act[~alive]] = LEFT
            x[act[alive]] += step[alive]
            act = act[alive]
            cell = sc.brute_force(g.c, x[act])[0]
            points[act, s + 1], length[act] = x[act], s + 2
        out[rule] = (points, length, status)
    return out


# ---- references shared by the CPU checker and the GPU tests (computed once per process) ---------------------------------------------
@functools.lru_cache(maxsize=None)
def affine_reference(run, direction):
    """``rk4_oracle`` of AFFINE_RUNS[run] with ``bound`` (the affine bound without K, per row) and ``sure`` (the particles that keep
    FACE_MARGIN away from every face)"""
    name, rule, step, n_steps = AFFINE_RUNS[run]
    g = grid(name)
    ref = rk4_oracle(Affine(g), seeds(name), n_steps, rule, step, direction, g=g)
    steps = np.broadcast_to(np.arange(n_steps + 1), ref["elapsed"].shape)
    ref["bound"] = affine_bound(g, Affine(g), steps, ref["elapsed"])
    ref["sure"] = ref["margin"] > FACE_MARGIN
    return ref


def path_field(run):
    return Affine(grid(PATH_RUNS[run][0]), b1_scale=0.15, seed=run)


@functools.lru_cache(maxsize=None)
def path_reference(run, direction, dt_snapshot=None, start=None):
    """``rk4_oracle`` of PATH_RUNS[run] (``dt_snapshot``: another spacing than ``path_dt``; ``start``: a key of ``STARTS``, other
    seeds) reduced to the snapshot rows: ``points`` [n, T, d] with the seed in column 0 (T - 1 backward), ``rows`` (the length a
    pathline reports), ``status``, ``bound`` [n, T], ``sure``"""
    name, n_snap, substeps = PATH_RUNS[run]
    g, field = grid(name), path_field(run)
    dt = (path_dt(g) if dt_snapshot is None else dt_snapshot) / substeps
    x = seeds(name) if start is None else STARTS[start]
    ref = rk4_oracle(field, x, 0, "time", dt, direction, g=g, substeps=substeps, n_snapshots=n_snap)
    steps = np.broadcast_to(np.arange(ref["elapsed"].shape[1]), ref["elapsed"].shape)
    rows = recorded(ref["length"], substeps)
    points = ref["points"][:, ::substeps].copy()
    points[np.arange(points.shape[1])[None] >= rows[:, None]] = np.nan          # (a snapshot row exists only when its whole interval was walked)
    bound = affine_bound(g, field, steps, ref["elapsed"])[:, ::substeps]
    if direction < 0:
        points, bound = points[:, ::-1], bound[:, ::-1]
    return {"points": points, "rows": rows, "status": ref["status"], "bound": bound, "sure": ref["margin"] > FACE_MARGIN, "dt_snapshot": dt * substeps}


STARTS = {}             # seeds a test made from a result (the key goes through the cache of ``path_reference``)


def round_trip_dt(run):
    """a snapshot spacing at which RK4 retraces its own steps to rounding.  One step of x' = A x + b(t) maps x to R(dt A) x + ...
    with R the Taylor polynomial of exp of degree four, and R(z) R(-z) = 1 + z^6 / 72 + ...: backward from the forward end does NOT
    come back to the seed unless that term is below the rounding: ||A|| dt <= 2^-9 gives z^6 / 72 < 10^-18 per step."""
    return PATH_RUNS[run][2] * 2.0 ** -9 / path_field(run).norm


@functools.lru_cache(maxsize=None)
def one_step_reference(name, rule, f32=False):
    """(node field [nn, d], step, ``grid_step_oracle`` of it from ``seeds(name)``, forward)"""
    g = grid(name)
    field = random_nodes(g, 5, f32)
    step = 0.45 if rule == "cell" else 0.2 * float(np.median(g.h))
    return field, step, grid_step_oracle(g, field, seeds(name), rule, step, 1)
