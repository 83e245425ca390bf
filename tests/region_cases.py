"""
Cases and references for the face-neighbour table, the connected-component labels and the region table of csrc/regions.hip (CPU only:
numpy, scipy, long double).

Grids: every case of ``sample_cases.CASES`` (``chain2d`` / ``chain3d`` use the full 62 / 63 key bits) and two uniform ones whose cells
are numbered row-major, ``uniform2d`` (64 x 64, cell ``x * 64 + y``) and ``uniform3d`` (16^3), on which masks can be drawn by hand and
``scipy.ndimage.label`` is a second opinion.

References, all from integers or in long double, none from the code under test:
    boxes               integer anchors and sizes of the cells on the lattice of ``sample_cases.emulate_index``
    brute_edges         the pairs of boxes that share a face of positive area, O(n^2) in chunks
    emulate_neighbours  the definition of include/s3hip.h in numpy (``same_level``: the planted mistake that drops level jumps)
    reference_labels    ``csgraph.connected_components`` on the in-subgraph, every component renamed to its smallest cell
    reference_table     the table with its sums in long double over the float64 terms of the definition
and the comparisons the GPU test uses (``check_labels``, ``check_table``), which tests/test_region_checker.py holds against planted
mistakes: same-level edges only, corner and edge connectivity (``touching_edges``), the closed interval made open (``in_mask(..,
open_=True)``), a label that is a member but not the minimum (``relabel_max``), the volume of a level taken as h (``h_power=1``).
"""
import functools

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from tests import sample_cases as sc

LD = np.longdouble
U = LD(2) ** -53
UNIFORM = {"uniform2d": (2, 6), "uniform3d": (3, 4)}        # name -> (d, level): 64 x 64 and 16^3 cells
GRIDS = list(sc.CASES) + list(UNIFORM)
TREES = ["tree2d", "tree3d"]
T_RANDOM = 4


# ---- grids --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid(name):
    if name not in UNIFORM:
        return sc.case(name)
    d, level = UNIFORM[name]
    side = np.arange(1 << level)
    anchors = np.array(np.meshgrid(*[side] * d, indexing="ij")).reshape(d, -1).T
    c = sc.grid_from_anchors(anchors, np.full(len(anchors), level), level, sc.WIDTH, sc.ROOT)
    c["name"] = name
    return c


@functools.lru_cache(maxsize=None)
def boxes(name):
    """(anchors int64 [n, d], sizes int64 [n], depth) in units of the finest cell, as s3_cell_index derives them"""
    c = grid(name)
    ix = sc.emulate_index(c)
    assert not ix["refused"].any(), name
    h = sc.cell_sizes(c)
    a = np.rint(((c["centers"] - h[:, None] / 2) - ix["origin"]) / ix["h_min"]).astype(np.int64)
    return a, (np.int64(1) << (ix["depth"] - c["levels"]).astype(np.int64)), int(ix["depth"])


def _pairs(name, share, chunk=256):
    """the pairs i < j whose CLOSED boxes meet, as (i, j, number of axes on which they only touch)"""
    a, s = boxes(name)[:2]
    lo, hi = a, a + s[:, None]
    out = []
    for s0 in range(0, len(a), chunk):
        low = np.maximum(lo[s0:s0 + chunk, None, :], lo[None])
        high = np.minimum(hi[s0:s0 + chunk, None, :], hi[None])
        meet = (low <= high).all(axis=2)
        touch = (low == high).sum(axis=2)
        i, j = np.nonzero(meet & share(touch))
        i = i + s0
        keep = i < j
        out.append(np.stack([i[keep], j[keep]], axis=1))
    return np.concatenate(out).astype(np.int64)


@functools.lru_cache(maxsize=None)
def brute_edges(name):
    """int64 [m, 2], i < j, sorted: the boxes overlap with positive length on all axes but one, where they touch"""
    return _sorted(_pairs(name, lambda touch: touch == 1))


@functools.lru_cache(maxsize=None)
def touching_edges(name):
    """the planted mistake: boxes that share an edge or a corner are connected too"""
    return _sorted(_pairs(name, lambda touch: touch >= 1))


def _sorted(e):
    e = np.stack([e.min(axis=1), e.max(axis=1)], axis=1) if len(e) else e.reshape(0, 2)
    return np.unique(e, axis=0)


def emulate_neighbours(name, same_level=False):
    """int32 [n, 2 d]: face 2 * axis + side holds the same-or-coarser leaf across it, -1 otherwise"""
    c = grid(name)
    ix = sc.emulate_index(c)
    a, s, depth = boxes(name)
    n, d = a.shape
    lv = c["levels"]
    nbr = np.full((n, 2 * d), -1, dtype=np.int32)
    for axis in range(d):
        for side in range(2):
            q = a.copy()
            q[:, axis] = a[:, axis] - 1 if side == 0 else a[:, axis] + s
            ok = (q[:, axis] >= 0) & (q[:, axis] < (1 << depth))
            key = sc.morton(np.where(ok[:, None], q, 0).astype(np.uint64), d, depth)
            pos = np.searchsorted(ix["starts"], key, side="right") - 1
            hit = ok & (pos >= 0)
            hit[hit] &= key[hit] < ix["ends"][pos[hit]]
            j = ix["ids"][np.maximum(pos, 0)]
            hit &= (lv[j] == lv) if same_level else (lv[j] <= lv)
            nbr[:, 2 * axis + side] = np.where(hit, j, -1)
    return nbr


def table_edges(nbr):
    i, f = np.nonzero(nbr >= 0)
    return _sorted(np.stack([i, nbr[i, f]], axis=1).astype(np.int64))


# ---- labels -------------------------------------------------------------------------------------------------------------------
def in_mask(field, lo, hi, open_=False):
    """lo <= (double) f <= hi, NaN out; ``open_``: the planted mistake lo < f < hi"""
    f = np.asarray(field).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return ((f > lo) & (f < hi)) if open_ else ((f >= lo) & (f <= hi))


def reference_labels(edges, mask):
    """mask bool [n, T] -> int32 [n, T]: -1 where out, otherwise the smallest cell id of the component of the in-subgraph"""
    mask = mask.reshape(len(mask), -1)
    n, n_t = mask.shape
    out = np.full((n, n_t), -1, dtype=np.int32)
    ids = np.arange(n)
    for t in range(n_t):
        m = mask[:, t]
        e = edges[m[edges[:, 0]] & m[edges[:, 1]]]
        _, comp = connected_components(coo_matrix((np.ones(len(e), dtype=np.int8), (e[:, 0], e[:, 1])), shape=(n, n)), directed=False)
        smallest = np.full(comp.max() + 1, n, dtype=np.int64)
        np.minimum.at(smallest, comp[m], ids[m])
        out[m, t] = smallest[comp[m]]
    return out


def relabel_max(labels):
    """the planted mistake: every region named by its LARGEST cell (the same partition, other names)"""
    out = labels.copy()
    ids = np.arange(len(labels))
    for t in range(labels.shape[1]):
        m = labels[:, t] >= 0
        largest = np.full(len(labels), -1, dtype=np.int64)
        np.maximum.at(largest, labels[m, t], ids[m])
        out[m, t] = largest[labels[m, t]]
    return out


def check_labels(got, ref, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.int32, f"{what}: labels {got.shape} {got.dtype}, expected {ref.shape} int32"
    bad = np.argwhere(got != ref)
    assert not len(bad), f"{what}: {len(bad)} labels differ, the first at (cell, column) {tuple(bad[0])}: {got[tuple(bad[0])]} != {ref[tuple(bad[0])]}"


def describe(name, labels):
    """(regions of two cells or more, the largest region's cells, the largest level jump inside a region) of one column of labels"""
    e, lv = brute_edges(name), grid(name)["levels"].astype(np.int64)
    inside = (labels[e[:, 0]] >= 0) & (labels[e[:, 1]] >= 0)
    jump = np.abs(lv[e[inside, 0]] - lv[e[inside, 1]])
    sizes = np.bincount(labels[labels >= 0])
    return int((sizes >= 2).sum()), int(sizes.max(initial=0)), int(jump.max(initial=0))


# ---- the table ----------------------------------------------------------------------------------------------------------------
EXACT = ("offsets", "label", "n_cells", "lo", "hi", "g_min", "g_max")


def reference_table(name, labels, g=None, h_power=None):
    """the table of labels [n, T] (and the weight g [n, T]) by the definition: float64 terms h = width / 2^l, V = h * h (* h), V c,
    V g, c -/+ h/2; their sums in long double.  ``*_abs``: the sums of the absolute terms.  ``h_power=1``: the planted mistake V = h"""
    c = grid(name)
    ctr, d = c["centers"], c["centers"].shape[1]
    h = sc.cell_sizes(c)
    vol = h * h * h if d == 3 else h * h
    if h_power == 1:
        vol = h
    lower, upper = ctr - h[:, None] / 2, ctr + h[:, None] / 2
    res = {k: [] for k in ("label", "n_cells", "volume", "num", "num_abs", "lo", "hi", "integral", "integral_abs", "g_min", "g_max")}
    offsets = [0]
    for t in range(labels.shape[1]):
        lab = labels[:, t]
        cells = np.flatnonzero(lab >= 0)
        roots, idx = np.unique(lab[cells], return_inverse=True)
        order = np.argsort(idx, kind="stable")
        cells, starts = cells[order], np.searchsorted(idx[order], np.arange(len(roots)))
        offsets.append(offsets[-1] + len(roots))
        if not len(roots):
            continue
        v = vol[cells].astype(LD)
        res["label"].append(roots.astype(np.int32))
        res["n_cells"].append(np.diff(np.append(starts, len(cells))).astype(np.int64))
        res["volume"].append(np.add.reduceat(v, starts))
        terms = v[:, None] * ctr[cells].astype(LD)
        res["num"].append(np.add.reduceat(terms, starts, axis=0))
        res["num_abs"].append(np.add.reduceat(np.abs(terms), starts, axis=0))
        res["lo"].append(np.minimum.reduceat(lower[cells], starts, axis=0))
        res["hi"].append(np.maximum.reduceat(upper[cells], starts, axis=0))
        if g is not None:
            gv = g[cells, t].astype(np.float64)
            res["integral"].append(np.add.reduceat(v * gv.astype(LD), starts))
            res["integral_abs"].append(np.add.reduceat(np.abs(v * gv.astype(LD)), starts))
            res["g_min"].append(np.minimum.reduceat(gv, starts))
            res["g_max"].append(np.maximum.reduceat(gv, starts))
    empty = {"label": np.int32, "n_cells": np.int64, "lo": np.float64, "hi": np.float64, "g_min": np.float64, "g_max": np.float64}
    out = {"offsets": np.asarray(offsets, dtype=np.int64)}
    for k, parts in res.items():
        if g is None and k in ("integral", "integral_abs", "g_min", "g_max"):
            continue
        wide = k in ("num", "num_abs", "lo", "hi")
        out[k] = np.concatenate(parts) if parts else np.zeros((0, d) if wide else (0,), dtype=empty.get(k, LD))
    out["centroid"] = out["num"] / out["volume"][:, None]
    return out


def check_table(got, ref, what=""):
    """``got``: dict of numpy arrays as ``hipops.region_table`` names them.  Integers, the box and the extrema EQUAL the reference; a
    sum of n float64 terms formed in any order with one rounding per addition (an fma folds the product's rounding into it) lies
    within n * 2^-53 * sum |terms| of the exact sum; the centroid is the rounded quotient of two such sums: to first order
    (B_num + |c| B_vol) / vol + 2^-53 |c|, and the factor 1 + 2^-30 holds the second-order terms (n 2^-53 <= 2^-30 for n < 2^23)."""
    for k in EXACT:
        if k in ref:
            assert got[k] is not None and got[k].shape == ref[k].shape, f"{what} {k}: shape {None if got[k] is None else got[k].shape} != {ref[k].shape}"
            same = np.array_equal(got[k], ref[k]) if got[k].dtype.kind == "i" else np.array_equal(got[k].view(np.int64), ref[k].view(np.int64))
            assert same, f"{what} {k}: differs from the reference at {np.argwhere(got[k] != ref[k])[:3].tolist()}"
    n = ref["n_cells"].astype(LD)
    b_vol = n * U * ref["volume"]
    err = np.abs(got["volume"].astype(LD) - ref["volume"])
    assert (err <= b_vol).all(), f"{what} volume: {float((err / np.maximum(b_vol, LD(1e-4000))).max()):.3g} of the bound"
    if "integral" in ref:
        bound = n * U * ref["integral_abs"]
        err = np.abs(got["integral"].astype(LD) - ref["integral"])
        assert (err <= bound).all(), f"{what} integral: error {float(err.max()):.3g} over its bound"
    b_num = n[:, None] * U * ref["num_abs"]
    cen = np.abs(ref["centroid"])
    bound = ((b_num + cen * b_vol[:, None]) / ref["volume"][:, None] + U * cen) * (1 + LD(2) ** -30)
    err = np.abs(got["centroid"].astype(LD) - ref["centroid"])
    assert (err <= bound).all(), f"{what} centroid: {float((err / bound).max()):.3g} of the bound"


# ---- fields -------------------------------------------------------------------------------------------------------------------
def _rng(name, salt):
    return np.random.default_rng(1000 * GRIDS.index(name) + salt)


@functools.lru_cache(maxsize=None)
def random_mask(name, share, n_t=T_RANDOM):
    """bool [n, n_t], every column drawn on its own"""
    return _rng(name, int(share * 100) + 7 * n_t).random((len(grid(name)["centers"]), n_t)) < share


LO, HI = -0.25, 0.375          # exact in float32


@functools.lru_cache(maxsize=None)
def smooth_field(name, f64):
    """[n, 3] float32 | float64: a smooth field with values planted exactly AT lo and hi (in), one ulp outside them (out) and NaN"""
    c = grid(name)
    x = (c["centers"] - c["centers"].min(axis=0)) / sc.WIDTH
    base = np.sin(5 * x[:, 0] + 1.0) * np.cos(4 * x[:, 1]) + (0.3 * np.sin(6 * x[:, -1]) if x.shape[1] == 3 else 0.0)
    f = np.stack([base, 0.8 * base + 0.1, -base], axis=1).astype(np.float64 if f64 else np.float32)
    rng = _rng(name, 3 + f64)
    n = len(f)
    lo, hi = f.dtype.type(LO), f.dtype.type(HI)
    for t in range(f.shape[1]):
        picks = rng.permutation(n)[:min(n, 40)]
        for k, value in enumerate([lo, hi, np.nextafter(lo, f.dtype.type(-np.inf)), np.nextafter(hi, f.dtype.type(np.inf)), np.nan]):
            f[picks[k::5], t] = value
    return f


def uniform2d_masks():
    """name -> bool [4096]: hand-drawn masks on the 64 x 64 grid, cell x * 64 + y"""
    x, y = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    snake = (x % 2 == 0) | ((x % 4 == 1) & (y == 63)) | ((x % 4 == 3) & (y == 0))       # one region whose diameter is its length
    comb = (y == 0) | (x % 2 == 0)                                                     # a spine and 32 teeth: one region
    checker = (x + y) % 2 == 0                                                         # every in-cell is its own region
    return {"serpentine": snake.reshape(-1), "comb": comb.reshape(-1), "checkerboard": checker.reshape(-1)}


@functools.lru_cache(maxsize=None)
def cases(name):
    """mask name -> (field [n, T] float32 | float64, lo, hi)"""
    n = len(grid(name)["centers"])
    out = {f"random{share}": (random_mask(name, share).astype(np.float32), 0.5, np.inf) for share in (0.3, 0.5, 0.7)}
    out["smooth32"], out["smooth64"] = (smooth_field(name, False), LO, HI), (smooth_field(name, True), LO, HI)
    ends = np.zeros((n, 2), dtype=np.float32)
    ends[:, 1] = np.nan
    out["all_in_all_out"] = (ends, -np.inf, np.inf)                                    # column 0: every cell in; column 1: none
    if name == "uniform2d":
        out["drawn"] = (np.stack(list(uniform2d_masks().values()), axis=1).astype(np.float32), 0.5, np.inf)
    return out


@functools.lru_cache(maxsize=None)
def labels_of(name, mask_name):
    field, lo, hi = cases(name)[mask_name]
    return reference_labels(brute_edges(name), in_mask(field, lo, hi))


@functools.lru_cache(maxsize=None)
def weight_field(name, n_t):
    """float64 [n, n_t] of both signs"""
    return _rng(name, 99).standard_normal((len(grid(name)["centers"]), n_t))
