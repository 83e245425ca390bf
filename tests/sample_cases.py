"""
Cases and references for the cell index, the point location and the sampling of csrc/sample.hip (CPU only: numpy, long double).

A case is a dict: ``centers`` f64 [n, d], ``levels`` int32 [n], ``width``, ``nodes`` f64 [nn, d], ``faces`` int32 [n, 2^d] (the
corner nodes of every cell in the order of ``corner_signs``), ``degenerate`` (a grid too plain for the conditions on the queries)
and ``queries`` f64 [NQ, d].

    tree2d, tree3d      a random recursive subdivision, NOT 2:1 balanced, depth 7 | 6, a tenth of the leaves deleted (holes), cells
                        shuffled, width 0.7, root corner at a non-dyadic position
    golden2d, golden3d  refine_2d_polygon and refine_3d_metric of tests/golden (grids of the reference)
    offset2d            the lowest cells are fine ones at an odd position: the lattice origin is NOT the minimum corner
    one_cell, level3    a single cell; a uniform grid of one level
    chain2d, chain3d    refined towards one corner down to level 31 | 21: dim * L = 62 | 63 key bits (``chain(d, depth)`` one level
                        deeper is the grid the index has to refuse)
    dyadic2d, dyadic3d  root [0, 1]^d, width 1: every coordinate and every operation on it is exact, and the queries lie ON faces,
                        on the lower bound of the domain and on the upper one (which belongs to no cell)

Elsewhere the queries are ``origin + (i + f) * h_min`` with ``f`` in [0.1, 0.9] and the integer ``i`` from two lattice cells below
the grid's bounding box to two above it, so that no query is near a face and the brute force cannot be in doubt.

References: ``brute_force`` (long double: the one cell with ``c - h/2 <= q < c + h/2`` on every axis), ``nearest_center``,
``emulate_locate`` (the definition of include/s3hip.h in plain float64, with the planted mistakes the checker test needs) and
``linear_reference`` (the float64 ``xi`` of the definition, everything after it in long double).
"""
import functools
import os

import numpy as np

LD = np.longdouble
NQ = 3001               # twelve workgroups of 256 launch positions, the last one ragged
WIDTH = 0.7
ROOT = (0.137, 0.211, 0.059)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CASES = ["tree2d", "tree3d", "golden2d", "golden3d", "offset2d", "one_cell", "level3", "chain2d", "chain3d", "dyadic2d", "dyadic3d"]
CHAIN_DEPTH = {2: 31, 3: 21}


def corner_signs(d):
    """[2^d, d]: the corner order of ``faces``"""
    flat = [(-1, -1), (-1, 1), (1, 1), (1, -1)]
    if d == 2:
        return np.array(flat, dtype=np.int64)
    return np.array([s + (z,) for z in (1, -1) for s in flat], dtype=np.int64)


# ---- grids --------------------------------------------------------------------------------------------------------------------
def grid_from_anchors(anchors, levels, depth, width, root):
    """cells given by integer anchors (units of the finest size, ``depth`` levels below the root cell at ``root``) -> case dict
    without queries; coordinates are formed in long double and rounded once"""
    anchors, levels = np.asarray(anchors, dtype=np.int64), np.asarray(levels, dtype=np.int64)
    n, d = anchors.shape
    size = (1 << (depth - levels)).astype(np.int64)
    h_min = LD(width) / LD(2) ** depth
    root = np.asarray(root[:d], dtype=LD)
    centers = (root + (anchors.astype(LD) + size[:, None].astype(LD) / 2) * h_min).astype(np.float64)
    corners = anchors[:, None, :] + (corner_signs(d)[None] > 0) * size[:, None, None]          # [n, 2^d, d]
    uniq, inverse = np.unique(corners.reshape(-1, d), axis=0, return_inverse=True)
    nodes = (root + uniq.astype(LD) * h_min).astype(np.float64)
    return {"centers": centers, "levels": levels.astype(np.int32), "width": float(width), "nodes": nodes,
            "faces": inverse.reshape(n, 1 << d).astype(np.int32), "degenerate": False}


def random_tree_cells(d, depth, p_split, seed, holes=0.1, full_levels=2):
    """(anchors in units of the finest size, levels): every cell of a level below ``full_levels`` is split, a deeper one with
    probability ``p_split``; a share ``holes`` of the leaves is deleted and the rest shuffled"""
    rng = np.random.default_rng(seed)
    cells = np.zeros((1, d), dtype=np.int64)                    # integer position at the current level
    offsets = np.array(np.meshgrid(*[[0, 1]] * d, indexing="ij")).reshape(d, -1).T
    anchors, levels = [], []
    for level in range(depth + 1):
        split = np.zeros(len(cells), dtype=bool) if level == depth else (rng.random(len(cells)) < p_split) | (level < full_levels)
        leaves = cells[~split]
        anchors.append(leaves << (depth - level))
        levels.append(np.full(len(leaves), level))
        cells = (cells[split][:, None, :] * 2 + offsets[None]).reshape(-1, d)
    anchors, levels = np.concatenate(anchors), np.concatenate(levels)
    keep = rng.permutation(len(anchors))[:int(round(len(anchors) * (1 - holes)))]
    assert levels[keep].max() == depth
    return anchors[keep], levels[keep]


def random_tree(d, depth, p_split, seed, width=WIDTH, root=ROOT, holes=0.1):
    anchors, levels = random_tree_cells(d, depth, p_split, seed, holes)
    return grid_from_anchors(anchors, levels, depth, width, root)


def chain(d, depth, width=WIDTH, root=ROOT):
    """every level keeps 2^d - 1 leaves and refines the child at the lower corner; the last level keeps all 2^d"""
    offsets = np.array(np.meshgrid(*[[0, 1]] * d, indexing="ij")).reshape(d, -1).T
    anchors, levels = [], []
    for level in range(1, depth + 1):
        kids = offsets if level == depth else offsets[1:]
        anchors.append(kids << (depth - level))
        levels.append(np.full(len(kids), level))
    case = grid_from_anchors(np.concatenate(anchors), np.concatenate(levels), depth, width, root)
    case["degenerate"] = True
    return case


def golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {"centers": np.ascontiguousarray(z["all_centers"], dtype=np.float64), "levels": z["all_levels"].reshape(-1).astype(np.int32),
            "width": float(z["width"]), "nodes": np.ascontiguousarray(z["all_nodes"], dtype=np.float64),
            "faces": np.ascontiguousarray(z["face_ids"], dtype=np.int32), "degenerate": False}


def offset_grid():
    """the quadrant [4, 8)^2 [units of level 3] of a root cell, refined irregularly from level 2 on, and level-3 cells left of and
    below it: the minimum corner (3, 3) is an odd number of fine cells away from the coarse ones"""
    fine = np.array([(3, 3), (3, 5), (5, 3), (3, 4), (6, 3), (3, 7)])
    a_sub, l_sub = random_tree_cells(2, 4, 0.45, 11, holes=0.0, full_levels=1)          # level 5 of the root in the end
    assert l_sub.min() == 1
    anchors, levels = np.concatenate([fine << 2, (4 << 2) + a_sub]), np.concatenate([np.full(len(fine), 3), l_sub + 1])
    order = np.random.default_rng(5).permutation(len(anchors))
    return grid_from_anchors(anchors[order], levels[order], 5, WIDTH, ROOT)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "tree2d":
        c = random_tree(2, 7, 0.5, 1)
    elif name == "tree3d":
        c = random_tree(3, 6, 0.3, 2)
    elif name == "golden2d":
        c = golden("refine_2d_polygon")
    elif name == "golden3d":
        c = golden("refine_3d_metric")
    elif name == "offset2d":
        c = offset_grid()
    elif name == "one_cell":
        c = grid_from_anchors([[0, 0, 0]], [0], 0, WIDTH, ROOT)
        c["degenerate"] = True
    elif name == "level3":
        side = np.arange(8)
        c = grid_from_anchors(np.array(np.meshgrid(side, side, indexing="ij")).reshape(2, -1).T, np.full(64, 3), 3, WIDTH, ROOT)
        c["degenerate"] = True
    elif name in ("chain2d", "chain3d"):
        d = int(name[5])
        c = chain(d, CHAIN_DEPTH[d])
    elif name in ("dyadic2d", "dyadic3d"):
        d = int(name[6])
        c = random_tree(d, 5 if d == 2 else 4, 0.5 if d == 2 else 0.35, 3 + d, width=1.0, root=(0.0, 0.0, 0.0), holes=0.12)
    else:
        raise KeyError(name)
    c["name"] = name
    c["queries"] = face_queries(c) if name.startswith("dyadic") else lattice_queries(c, seed=len(name) + 7 * c["centers"].shape[1],
                                                                                      log_share=0.5 if name.startswith("chain") else 0.0)
    return c


# ---- the definition in float64 ------------------------------------------------------------------------------------------------
def cell_sizes(c):
    return c["width"] / 2.0 ** c["levels"].astype(np.float64)


def emulate_lattice(c, align=True):
    """(origin [d], h_min, L) as s3_cell_index derives them; ``align=False``: the planted mistake that takes the minimum corner"""
    lv, h = c["levels"], cell_sizes(c)
    depth, lmin = int(lv.max()), int(lv.min())
    h_min, big = c["width"] / 2.0 ** depth, c["width"] / 2.0 ** lmin
    corner = c["centers"][int(np.flatnonzero(lv == lmin)[0])] - big / 2
    lo = (c["centers"] - h[:, None] / 2).min(axis=0)
    origin = corner - np.ceil((corner - lo) / big - 1e-9) * big if align else lo
    return origin, h_min, depth


def morton(i, d, depth):
    key = np.zeros(len(i), dtype=np.uint64)
    for b in range(depth):
        for a in range(d):
            key |= ((i[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(b * d + a)
    return key


def emulate_index(c, align=True):
    """-> dict(starts, ends, ids, origin, h_min, depth, refused [4]): the sorted ranges and what the build step would refuse"""
    d = c["centers"].shape[1]
    origin, h_min, depth = emulate_lattice(c, align)
    refused = np.zeros(4, dtype=np.int64)
    if d * depth > 63:
        refused[3] = d * depth
        return {"refused": refused}
    h = cell_sizes(c)
    v = ((c["centers"] - h[:, None] / 2) - origin) / h_min
    r = np.rint(v)
    off = ~((np.abs(v - r) <= 1e-6) & (r >= 0) & (r < 2.0 ** depth)).all(axis=1)
    a = np.where(off[:, None], 0, r).astype(np.uint64)
    low = (np.uint64(1) << (depth - c["levels"]).astype(np.uint64)) - np.uint64(1)
    mis = ~off & ((a & low[:, None]) != 0).any(axis=1)
    refused[0], refused[1] = off.sum(), mis.sum()
    keys = morton(a, d, depth)
    order = np.argsort(keys, kind="stable")
    starts = keys[order]
    ends = starts + (np.uint64(1) << (d * (depth - c["levels"][order])).astype(np.uint64))
    refused[2] = 0 if refused[:2].any() else int((ends[:-1] > starts[1:]).sum())        # (the build step stops at the first refusal)
    return {"starts": starts, "ends": ends, "ids": order.astype(np.int32), "origin": origin, "h_min": h_min, "depth": depth,
            "refused": refused, "max_off": float(np.abs(v - r).max())}


def emulate_locate(c, q, align=True, closed=False):
    """the located cell of every query by the definition, in float64; ``closed``: the planted mistake that gives a point on a face
    to the LOWER cell"""
    ix = emulate_index(c, align)
    d = q.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        t = (q - ix["origin"]) / ix["h_min"]
        t = np.ceil(t) - 1 if closed else np.floor(t)
        ok = ((t >= 0) & (t < 2.0 ** ix["depth"])).all(axis=1)
    key = morton(np.where(ok[:, None], t, 0).astype(np.uint64), d, ix["depth"])
    pos = np.searchsorted(ix["starts"], key, side="right") - 1
    hit = ok & (pos >= 0)
    hit[hit] &= key[hit] < ix["ends"][pos[hit]]
    return np.where(hit, ix["ids"][np.maximum(pos, 0)], -1).astype(np.int32)


# ---- queries ------------------------------------------------------------------------------------------------------------------
def lattice_queries(c, seed, n=NQ, log_share=0.0):
    origin, h_min, depth = emulate_lattice(c)
    d = c["centers"].shape[1]
    h = cell_sizes(c)
    lo = np.floor(((c["centers"] - h[:, None] / 2).min(axis=0) - origin) / h_min + 0.5).astype(np.int64)
    hi = np.floor(((c["centers"] + h[:, None] / 2).max(axis=0) - origin) / h_min + 0.5).astype(np.int64)
    rng = np.random.default_rng(seed)
    i = rng.integers(lo - 2, hi + 2, size=(n, d))
    n_log = int(n * log_share)                      # (a chain: half of the queries in boxes of every scale at the refined corner)
    if n_log:
        i[:n_log] = lo + np.floor(2.0 ** (rng.random((n_log, 1)) * np.log2(hi - lo)) * rng.random((n_log, d))).astype(np.int64)
    f = rng.uniform(0.1, 0.9, size=(n, d))
    return origin + (i + f) * h_min


def face_queries(c, n=NQ):
    """dyadic grid on [0, 1]^d: per coordinate a lattice line k / 2^L (k = 0 and k = 2^L among them) or the middle between two;
    a third of the queries has every coordinate on a line"""
    d, depth = c["centers"].shape[1], int(c["levels"].max())
    rng = np.random.default_rng(17 + d)
    k = rng.integers(0, 2 ** depth + 1, size=(n, d)).astype(np.float64)
    on_line = rng.random((n, d)) < 0.6
    on_line[: n // 3] = True
    q = (k + np.where(on_line, 0.0, 0.5)) / 2.0 ** depth
    q[n // 3: n // 3 + 40] = rng.integers(0, 2, size=(40, d)).astype(np.float64)        # the corners of the domain
    return q


# ---- references ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def truth(name):
    """(ids int32 [NQ] by brute force, how many cells contain each query, the nearest centre of each query)"""
    c = case(name)
    return brute_force(c, c["queries"]) + (nearest_center(c, c["queries"]),)


def brute_force(c, q, chunk=256):
    ctr, h = c["centers"].astype(LD), (LD(c["width"]) / LD(2) ** c["levels"].astype(LD))[:, None]
    lo, hi = ctr - h / 2, ctr + h / 2
    ids, count = np.full(len(q), -1, dtype=np.int32), np.zeros(len(q), dtype=np.int64)
    for s in range(0, len(q), chunk):
        x = q[s:s + chunk].astype(LD)[:, None, :]
        inside = ((x >= lo[None]) & (x < hi[None])).all(axis=2)
        count[s:s + chunk] = inside.sum(axis=1)
        ids[s:s + chunk] = np.where(inside.any(axis=1), inside.argmax(axis=1), -1)
    return ids, count


def nearest_center(c, q, chunk=256):
    out = np.empty(len(q), dtype=np.int32)
    for s in range(0, len(q), chunk):
        out[s:s + chunk] = ((q[s:s + chunk, None, :] - c["centers"][None]) ** 2).sum(axis=2).argmin(axis=1)
    return out


def xi_f64(c, q, ids):
    """the local coordinates of the definition, float64 operation by operation; rows with id -1 are NaN"""
    safe = np.maximum(ids, 0)
    h = cell_sizes(c)[safe][:, None]
    xi = np.clip((q - (c["centers"][safe] - h / 2)) / h, 0.0, 1.0)
    return np.where((ids >= 0)[:, None], xi, np.nan)


def linear_reference(c, q, ids, node_field, signs=None):
    """node_field [nn, ...] -> (value, mag) long double [nq, ...]: sum_m w_m f_m and sum_m |w_m f_m| with the float64 xi of the
    definition and everything after it in long double; NaN rows where id is -1.  ``signs``: another corner order (a planted mistake)"""
    d = q.shape[1]
    signs = corner_signs(d) if signs is None else signs
    xi = xi_f64(c, q, ids).astype(LD)
    w = np.ones((len(q), 1 << d), dtype=LD)
    for a in range(d):
        w *= np.where(signs[None, :, a] > 0, xi[:, a:a + 1], 1 - xi[:, a:a + 1])
    f = node_field[c["faces"][np.maximum(ids, 0)]].astype(LD)                    # [nq, 2^d, ...]
    w = w.reshape(w.shape + (1,) * (f.ndim - 2))
    value, mag = (w * f).sum(axis=1), np.abs(w * f).sum(axis=1)
    miss = ids < 0
    value[miss], mag[miss] = np.nan, np.nan
    return value, mag


def linear_bound(d, mag):
    """(2^d + 3) * 2^-53 * sum_m |w_m f_m|: at most d roundings in a weight (one per axis: ``1 - xi`` or a product, a ``(1 - xi)``
    factor folded into one fma) and an fma chain of 2^d terms, to first order"""
    return ((1 << d) + 3) * LD(2) ** -53 * mag


def affine_nodes(c, coeff, offset):
    """f(x) = coeff . x + offset at the nodes, in long double, rounded once to float64"""
    return (c["nodes"].astype(LD) @ np.asarray(coeff, dtype=LD) + LD(offset)).astype(np.float64)


def affine_bound(c, q, ids, coeff, offset):
    """how far the blend of ``affine_nodes`` may sit from f(q): the bound of the blend itself, one rounding of every node value,
    and the roundings of the positions f64 cannot hold -- the node coordinates, c - h/2 and x - (c - h/2), each half an ulp of a
    coordinate no larger than |c| + h: 8 * 2^-53 * (|coeff| . (|c| + h) + |offset|) covers them with room"""
    coeff = np.abs(np.asarray(coeff, dtype=LD))
    safe = np.maximum(ids, 0)
    reach = np.abs(c["centers"][safe]).astype(LD) + cell_sizes(c)[safe][:, None].astype(LD)
    return 8 * LD(2) ** -53 * (reach @ coeff + abs(LD(offset)))


# ---- grids the index has to refuse ----------------------------------------------------------------------------------------------
REFUSALS = {"off": 0, "misaligned": 1, "overlap": 2, "bits2d": 3, "bits3d": 3}       # name -> the entry of the refusal counts


@functools.lru_cache(maxsize=None)
def refusal(name):
    """(case, expected count): tree2d with one planted fault, or a chain one level too deep"""
    if name.startswith("bits"):
        d = int(name[4])
        return chain(d, CHAIN_DEPTH[d] + 1), d * (CHAIN_DEPTH[d] + 1)
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case("tree2d").items()}
    origin, h_min, depth = emulate_lattice(c)
    h = cell_sizes(c)
    inner = ((c["centers"] - h[:, None] / 2 - origin) / h_min > 2.0 ** (depth - 1)).all(axis=1)     # far from the lower bounds
    if name == "off":                       # a finest cell 1e-3 lattice units off its place
        j = int(np.flatnonzero(inner & (c["levels"] == depth))[0])
        c["centers"][j, 0] += 1e-3 * h_min
    elif name == "misaligned":              # a cell of the level above the finest moved by one finest cell
        j = int(np.flatnonzero(inner & (c["levels"] == depth - 1))[0])
        c["centers"][j, 1] += h_min
    else:                                   # a child planted inside an existing leaf
        j = int(np.flatnonzero(c["levels"] == depth - 2)[0])
        c["centers"] = np.concatenate([c["centers"], c["centers"][j:j + 1] - h[j] / 4])
        c["levels"] = np.concatenate([c["levels"], c["levels"][j:j + 1] + 1])
    return c, 1
