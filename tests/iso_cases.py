"""
Cases, the reference and the checker for the isosurfaces and contour lines of csrc/iso.hip (CPU only: numpy, long double).

The definition (include/s3hip.h restates it).  ``nodes`` f64 [N, d], ``faces`` int [Nc, 2^d] in the corner order of
``sample_cases.corner_signs``, a node field [N, T] f32 | f64, a finite ``level``.

    inside      node n at snapshot t iff (double) f[n][t] >= level
    nothing     from a cell with a corner value that is NaN or +-inf at t, or with a corner id outside [0, N)
    simplices   per permutation pi of the axes, in lexicographic order: the path p_0 = (-, .., -), p_{i+1} = p_i with axis pi(i)
                switched to + (Kuhn): 6 tetrahedra around the diagonal corner 4 -> corner 2 in 3-D, 2 triangles around 0 -> 2 in 2-D
    primitives  path positions 0 .. d, I the inside ones, O the outside ones, ascending:
                3-D, one position s alone on its side: the triangle over the edges (s,a), (s,b), (s,c), a < b < c the others
                3-D, I = {i,j}, O = {k,l}: the quad (i,k), (i,l), (j,l), (j,k) as the triangles (q0,q1,q2) and (q0,q2,q3)
                2-D: the segment over (s,a), (s,b)
    orientation the right-hand normal of a triangle points to f < level; in 2-D f >= level lies to the left of q0 -> q1; where the
                natural order gives the opposite the last two vertices of the primitive are swapped (``swap_needed`` derives
                from affine fields for which (simplex, mask) that is)
    vertex      on the edge between the nodes a < b in GLOBAL node id: t = (level - f_a) / (f_b - f_a), x = fma(t, x_b - x_a, x_a)
    order       (snapshot, cell, simplex, primitive of the simplex)

``extract`` evaluates this in long double (the reference: ``frac`` and ``verts`` long double, with the bounds below) or in float64
operation by operation (``arith="f64"``: the emulation, which takes the planted mistakes the checker test needs).

Bounds of ``check`` (u = 2^-53; counts, offsets, cells and edges are compared EXACTLY, they depend on comparisons only):
    |t - t_ref| <= 4 u t                      one rounding in each difference and in the quotient
    |x - x_ref| <= u (5 t |x_b - x_a| + |x|)  the coordinate difference and the fma add two roundings
Test fields keep magnitudes within 2^+-100, so that no quotient is subnormal.
"""
import functools
import itertools
from fractions import Fraction

import numpy as np

from tests import sample_cases as sc

LD = np.longdouble
U = LD(2) ** -53
MISTAKES = ("gt", "simplex_dir", "swap", "quad", "cell_major", "nan")
KEYS = ("offsets", "verts", "edges", "frac", "cells")


# ---- the decomposition -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kuhn(d):
    """[(permutation, parity 0 | 1, the corners of ``faces`` along the path)] in lexicographic order of the permutation"""
    signs = sc.corner_signs(d)
    out = []
    for perm in itertools.permutations(range(d)):
        p = -np.ones(d, dtype=np.int64)
        path = []
        for step in (None,) + perm:
            if step is not None:
                p[step] = 1
            path.append(int(np.flatnonzero((signs == p).all(axis=1))[0]))
        parity = sum(1 for i in range(d) for j in range(i) if perm[j] > perm[i]) & 1
        out.append((perm, parity, tuple(path)))
    return out


def natural_primitives(d, mask, quad_cyclic=True):
    """the primitives of a simplex whose inside positions are the bits of ``mask``, before orientation: a tuple of primitives,
    each d pairs of path positions"""
    inside = [p for p in range(d + 1) if mask >> p & 1]
    outside = [p for p in range(d + 1) if not mask >> p & 1]
    if not inside or not outside:
        return ()
    if len(inside) == 1 or len(outside) == 1:
        s = inside[0] if len(inside) == 1 else outside[0]
        return (tuple((s, o) for o in range(d + 1) if o != s),)
    (i, j), (k, l) = inside, outside
    q = [(i, k), (i, l), (j, l), (j, k)] if quad_cyclic else [(i, k), (i, l), (j, k), (j, l)]
    return ((q[0], q[1], q[2]), (q[0], q[2], q[3]))


@functools.lru_cache(maxsize=None)
def swap_needed(d, simplex, mask):
    """does the natural order of the primitives of (simplex, mask) contradict the orientation rule?  Derived from the affine field
    with +1 at the inside and -1 at the outside positions of the simplex in the cell [-1, 1]^d, level 0."""
    path = kuhn(d)[simplex][2]
    x = sc.corner_signs(d)[list(path)].astype(np.float64)                       # [d + 1, d]
    v = np.array([1.0 if mask >> p & 1 else -1.0 for p in range(d + 1)])
    g = np.linalg.solve(x[1:] - x[0], v[1:] - v[0])
    answers = set()
    for prim in natural_primitives(d, mask):
        q = np.array([(x[a] + x[b]) / 2 for a, b in prim])
        if d == 3:
            answers.add(bool(np.cross(q[1] - q[0], q[2] - q[0]) @ g > 0))      # the normal has to point down the gradient
        else:
            e = q[1] - q[0]
            answers.add(bool(np.array([-e[1], e[0]]) @ g < 0))                  # the left of q0 -> q1 has to be the inside
    assert len(answers) == 1, "the triangles of a quad disagree"
    return answers.pop()


def primitives(d, simplex, mask, mistake=None):
    prims = natural_primitives(d, mask, quad_cyclic=mistake != "quad")
    swap = swap_needed(d, simplex, mask)
    if mistake == "swap" and simplex == 0 and mask == (5 if d == 3 else 2):
        swap = not swap
    return tuple(p[:-2] + (p[-1], p[-2]) for p in prims) if swap else prims


# ---- the definition ---------------------------------------------------------------------------------------------------------
def _fma(t, dx, xa):
    """float64 fma, elementwise and correctly rounded (exact rational arithmetic: a few thousand vertices at the most)"""
    out = np.empty(t.shape, dtype=np.float64)
    for i, (a, b, c) in enumerate(zip(t.ravel().tolist(), dx.ravel().tolist(), xa.ravel().tolist())):
        out.flat[i] = float(Fraction(a) * Fraction(b) + Fraction(c)) if np.isfinite([a, b, c]).all() else a * b + c
    return out


def extract(nodes, faces, field, level, arith="ld", mistake=None):
    """-> dict(offsets int64 [T + 1], verts [n, d, d], edges int32 [n, d, 2], frac [n, d], cells int32 [n], simplex [n]: the
    simplex of its cell a primitive came from); with ``arith="ld"`` also ``frac_bound`` and ``verts_bound``"""
    assert mistake is None or (mistake in MISTAKES and arith == "f64")
    nodes, faces = np.asarray(nodes, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    field = np.asarray(field)
    f = (field[:, None] if field.ndim == 1 else field).astype(np.float64)      # (float32 widens exactly)
    n_nodes, d = nodes.shape
    n_snap = f.shape[1]
    level = float(level)
    ok_id = ((faces >= 0) & (faces < n_nodes)).all(axis=1)
    vals = f[np.where(ok_id[:, None], faces, 0)]                                # [Nc, 2^d, T]
    valid = ok_id[:, None] & (np.isfinite(vals).all(axis=1) if mistake != "nan" else ~np.isinf(vals).any(axis=1))
    with np.errstate(invalid="ignore"):
        inside = (vals > level) if mistake == "gt" else (vals >= level)
    parts = []
    for s, (_, _, path) in enumerate(kuhn(d)):
        m = np.zeros(valid.shape, dtype=np.int64)
        for p, corner in enumerate(path):
            m |= inside[:, corner, :].astype(np.int64) << p
        m = np.where(valid, m, 0).T                                             # [T, Nc]
        for mask in range(1, (1 << (d + 1)) - 1):
            tt, cc = np.nonzero(m == mask)
            if not len(tt):
                continue
            for k, prim in enumerate(primitives(d, s, mask, mistake)):
                corners = np.array([[path[a], path[b]] for a, b in prim])        # [d, 2]
                parts.append((tt, cc, np.full(len(tt), s), np.full(len(tt), k), faces[cc][:, corners]))
    if parts:
        tt, cc, ss, kk, e = (np.concatenate([p[i] for p in parts]) for i in range(5))
    else:
        tt = cc = ss = kk = np.zeros(0, dtype=np.int64)
        e = np.zeros((0, d, 2), dtype=np.int64)
    order = np.lexsort((kk, ss, tt, cc) if mistake == "cell_major" else (kk, ss, cc, tt))
    tt, cc, ss, e = tt[order], cc[order], ss[order], e[order]
    a, b = (e[..., 0], e[..., 1]) if mistake == "simplex_dir" else (e.min(axis=-1), e.max(axis=-1))
    fa, fb = f[a, tt[:, None]], f[b, tt[:, None]]                               # [n, d]
    xa, xb = nodes[a], nodes[b]                                                 # [n, d, d]
    out = {"offsets": np.concatenate([[0], np.cumsum(np.bincount(tt, minlength=n_snap))]).astype(np.int64),
           "edges": np.stack([a, b], axis=-1).astype(np.int32), "cells": cc.astype(np.int32), "simplex": ss}
    with np.errstate(invalid="ignore", divide="ignore"):
        if arith == "ld":
            fa, fb, xa, xb, lv = fa.astype(LD), fb.astype(LD), xa.astype(LD), xb.astype(LD), LD(level)
            t = (lv - fa) / (fb - fa)
            x = xa + t[..., None] * (xb - xa)
            out.update(frac=t, verts=x, frac_bound=4 * U * np.abs(t), verts_bound=U * (5 * np.abs(t[..., None] * (xb - xa)) + np.abs(x)))
        else:
            t = (level - fa) / (fb - fa)
            out.update(frac=t, verts=_fma(np.broadcast_to(t[..., None], xa.shape), xb - xa, xa))
    return out


# ---- the checker ------------------------------------------------------------------------------------------------------------
def check(got, ref, what=""):
    """``got`` (float64, from the GPU or the emulation) against the long-double reference: raises AssertionError with the first
    figure that is off"""
    for key in ("offsets", "cells", "edges"):
        g, r = np.asarray(got[key]), ref[key]
        assert g.shape == r.shape, f"{what}: {key} has shape {g.shape}, expected {r.shape}"
        assert np.array_equal(g, r), f"{what}: {key} differs at {np.argwhere(g != r)[:3].tolist()} of {r.shape}"
    for key in ("frac", "verts"):
        g, r, bound = np.asarray(got[key]), ref[key], ref[key + "_bound"]
        assert g.shape == r.shape, f"{what}: {key} has shape {g.shape}, expected {r.shape}"
        if g.size:
            err = np.abs(g.astype(LD) - r)
            bad = ~(err <= bound)                                               # (NaN fails)
            worst = float((err / np.maximum(bound, LD(2) ** -1000)).max()) if not np.isnan(err).any() else float("nan")
            assert not bad.any(), f"{what}: {key} off at {int(bad.sum())} of {g.size} entries, worst {worst:.3g} x bound"
    f = np.asarray(got["frac"])
    assert not f.size or (f.min() >= 0.0 and f.max() <= 1.0), f"{what}: frac outside [0, 1]"


# ---- properties of a surface -------------------------------------------------------------------------------------------------
def vertex_keys(edges):
    """the weld key (a << 32) | b of every vertex, int64 [n, d]"""
    e = np.asarray(edges).astype(np.int64)
    return (e[..., 0] << 32) | e[..., 1]


def surface_report(res, t=0):
    """what the closed-surface conditions need of snapshot ``t``: dict(n, degenerate, undirected, directed, euler, same_bits)"""
    lo, hi = int(res["offsets"][t]), int(res["offsets"][t + 1])
    keys = vertex_keys(res["edges"][lo:hi])                                     # [n, d]
    verts = np.asarray(res["verts"][lo:hi], dtype=np.float64)
    n, d = keys.shape
    uniq, inverse = np.unique(keys.reshape(-1), return_inverse=True)
    flat = verts.reshape(n * d, d)
    first = np.zeros(len(uniq), dtype=np.int64)
    first[inverse[::-1]] = np.arange(n * d)[::-1]
    same_bits = bool(np.array_equal(flat.view(np.int64), flat[first[inverse]].view(np.int64)))
    idx = inverse.reshape(n, d)
    if d == 2:
        return {"n": n, "degenerate": int((idx[:, 0] == idx[:, 1]).sum()), "valence": np.bincount(inverse), "same_bits": same_bits}
    area2 = np.linalg.norm(np.cross(verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0]), axis=1)
    degenerate = int(((idx[:, 0] == idx[:, 1]) | (idx[:, 1] == idx[:, 2]) | (idx[:, 0] == idx[:, 2]) | ~(area2 > 0)).sum())
    pairs = np.concatenate([idx[:, [0, 1]], idx[:, [1, 2]], idx[:, [2, 0]]])   # directed
    nv = len(uniq)
    directed = np.bincount(pairs[:, 0] * nv + pairs[:, 1])
    und = np.sort(pairs, axis=1)
    undirected = np.bincount(und[:, 0] * nv + und[:, 1])
    return {"n": n, "degenerate": degenerate, "undirected": undirected[undirected > 0], "directed": directed[directed > 0],
            "euler": nv - int((undirected > 0).sum()) + n, "same_bits": same_bits}


def assert_closed(res, d, what=""):
    """the conditions on the uniform grids: 648 proper triangles of a closed oriented sphere | 32 segments of a closed curve"""
    rep = surface_report(res)
    assert rep["same_bits"], f"{what}: vertices with equal keys differ in their bits"
    assert rep["degenerate"] == 0, f"{what}: {rep['degenerate']} degenerate primitives"
    if d == 2:
        assert rep["n"] == 32, f"{what}: {rep['n']} segments, expected 32"
        assert (rep["valence"] == 2).all(), f"{what}: a vertex key does not occur exactly twice"
        return
    assert rep["n"] == 648, f"{what}: {rep['n']} triangles, expected 648"
    assert (rep["undirected"] == 2).all(), f"{what}: an undirected edge does not occur exactly twice"
    assert (rep["directed"] == 1).all(), f"{what}: a directed edge occurs twice (orientation)"
    assert rep["euler"] == 2, f"{what}: V - E + F = {rep['euler']}"


# ---- cases ------------------------------------------------------------------------------------------------------------------
UNIFORM_LEVEL = -0.21
GRIDS = ["tree2d", "tree3d", "golden2d", "golden3d", "chain3d", "one_cell", "uniform3d", "uniform2d"]


@functools.lru_cache(maxsize=None)
def uniform(d):
    """the uniform 8^d grid (level 3, width 0.7, root ROOT) and f = -|x - c|, c = ROOT + 0.7 (0.48, 0.53, 0.51)"""
    side = np.arange(8)
    anchors = np.array(np.meshgrid(*[side] * d, indexing="ij")).reshape(d, -1).T
    c = sc.grid_from_anchors(anchors, np.full(len(anchors), 3), 3, sc.WIDTH, sc.ROOT)
    centre = np.asarray(sc.ROOT[:d]) + sc.WIDTH * np.array([0.48, 0.53, 0.51])[:d]
    c["field"] = -np.linalg.norm(c["nodes"] - centre, axis=1)
    c["name"] = f"uniform{d}d"
    return c


def grid(name):
    return uniform(int(name[7])) if name.startswith("uniform") else sc.case(name)


SMOOTH_LEVEL = 0.0625


@functools.lru_cache(maxsize=None)
def smooth_field(name, n_snap):
    """field f64 [N, T] to be cut at SMOOTH_LEVEL: per column a distance to a point inside the grid plus an affine part, shifted by
    another amount per column (a different level per column, taken between the 0.2 and the 0.8 quantile of the column's node
    values -- from 100 columns on between the 0.01 and the 0.05 quantile, a small surface, to keep the reference quick -- so that
    every column is cut)"""
    nodes = grid(name)["nodes"]
    d = nodes.shape[1]
    rng = np.random.default_rng(1000 + n_snap + 7 * len(name))
    lo, hi = nodes.min(axis=0), nodes.max(axis=0)
    centre = lo + (hi - lo) * rng.uniform(0.3, 0.7, size=(n_snap, d))
    slope = rng.uniform(-0.4, 0.4, size=(n_snap, d))
    f = np.linalg.norm(nodes[:, None, :] - centre[None], axis=2) + np.einsum("nd,td->nt", nodes - lo, slope)
    q = rng.uniform(0.2, 0.8, size=n_snap) if n_snap < 100 else rng.uniform(0.01, 0.05, size=n_snap)
    levels = np.array([np.quantile(f[:, t], q[t]) for t in range(n_snap)])
    return f - levels[None] + SMOOTH_LEVEL


def every_mask(d, n_snap, seed=0):
    """three cells of different sizes (not joined: ``2^d`` nodes each) and a field [N, n_snap] whose sign pattern at the corners
    of every cell runs through all 2^(2^d) masks (3-D: 256 columns; 2-D: 16), magnitudes random in [0.1, 10); level 0.25"""
    rng = np.random.default_rng(seed + d)
    signs = sc.corner_signs(d)
    nc = 1 << d
    nodes, faces = [], []
    for j, (size, at) in enumerate([(0.7, 0.1), (0.11, 1.3), (2.3, -4.0)]):
        nodes.append(at + (signs + 1) / 2 * size * (1 + 0.1 * np.arange(d)))
        faces.append(rng.permutation(nc) + j * nc)
    nodes, faces = np.concatenate(nodes), np.array(faces)
    nodes = nodes[np.argsort(faces.reshape(-1))]                                # node faces[j][m] is corner m of cell j
    mask = (np.arange(n_snap) % (1 << nc))[None, :] >> np.arange(nc)[:, None] & 1      # [2^d, T]
    field = np.empty((3 * nc, n_snap))
    for j in range(3):
        mag = 10.0 ** rng.uniform(-1, 1, size=(nc, n_snap))
        field[faces[j]] = 0.25 + np.where(np.roll(mask, j, axis=1) > 0, mag, -mag)
    return nodes, faces.astype(np.int32), field, 0.25
