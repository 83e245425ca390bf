"""
Hostile inputs for the refine's child-metric search (csrc/knn.hip: the per-lane child_metric_kernel, and with parents the
chain coop -> near -> far -> per-lane rest), shared by tests/test_gpu_child_metric.py (the GPU against the oracle) and
tests/test_child_metric_oracle.py (the oracle and the cases themselves, CPU only).  No GPU here.

A case is ``(name, dim, k, occupancy, cloud, y, batches)``:
  occupancy -- the KNN index's target points per bucket (``hipops.knn_occupancy(k, dim)`` is the refine's own);
  cloud, y  -- the points [n, dim] and the metric [n] (float64);
  batches   -- ``Batch`` tuples: a root batch of cells (centres, levels, the root width, the id of its first cell) that is
               evaluated on its own, then ``n_par`` of its cells (a permuted subset) are refined and their children are
               evaluated in the slices cut at ``cuts`` (as ranks split a batch: parents_offset = the slice's start).
               ``routes`` maps a stage of the chain ("coop", "near", "far", "rest") to whether it must answer at least one
               child point of the children (True) or none (False); a stage not named is free.

The property sets below name the cases whose purpose depends on a property of the generated data; the CPU test checks that
the data still has it.
"""
import functools
from collections import namedtuple

import numpy as np

Batch = namedtuple("Batch", "centers level width first n_par cuts routes")

GAIN0 = 0.37
BRUTE_MAX_POINTS = 20_000          # above this the GPU test's reference is the oracle's bucket grid (same results) ...


def flat(x):
    """... unless the cloud has no extent along some axis: the oracle's grid then has buckets of about 1e-9 of the cloud's size
    along the others, and a query off the cloud walks through millions of rings of them"""
    return bool((x.max(0) == x.min(0)).any())

ZERO_CASES = ("lattice2d_k8", "lattice3d_k26", "planted2d_k8", "planted3d_k26", "tiny2d_n1_k1")   # zero distances
TIE_CASES = ("lattice2d_k8", "lattice2d_k7", "lattice3d_k26", "dup2d_r2_k9", "dup2d_r47_k48", "dup3d_r48_k49",
             "dup2d_r49_k47", "dup2d_r65_k64", "offset2d_k9")                 # a tie group straddles the k-th neighbour
OUTSIDE_CASES = ("outside3d_k8", "outside2d_k48")                             # cells outside the cloud's bounding box


def knn_occupancy(k, dim):
    """the refine's default occupancy (hipops.knn_occupancy; restated here so that no case needs the package)"""
    return max(1.0, k / (13.0 if dim == 3 else 6.7))


def wide_y(rng, n):
    """magnitudes 1e-8 .. 1e8 of both signs: any change of summation order changes the bits"""
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-8, 8, n) * (1 + rng.random(n))


def const_y(n):
    """a power of two: every prediction is exactly this value, every gain exactly 0"""
    return np.full(n, 2.0 ** -3)


def lattice(m, dim):
    return np.stack(np.meshgrid(*[np.arange(m) / m] * dim, indexing="ij"), -1).reshape(-1, dim)


def tree_cells(rng, dim, levels, per_level, lo=0.0, width=1.0):
    """random distinct cells of the tree over the cube [lo, lo + width)^dim at the given levels: (centres, levels)"""
    cs, lv = [], []
    for L in levels:
        side = 2 ** L
        ids = rng.choice(side ** dim, size=min(per_level, side ** dim), replace=False)
        ijk = np.stack(np.unravel_index(ids, (side,) * dim), -1)
        cs.append(lo + (ijk + 0.5) * (width / side))
        lv.append(np.full(len(ids), L, dtype=np.int32))
    return np.concatenate(cs), np.concatenate(lv)


def random_cells(rng, dim, levels, per_level, lo=-0.1, span=1.2):
    """cells of the given levels with centres anywhere in [lo, lo + span)^dim (not tree positions)"""
    cs = [lo + span * rng.random((per_level, dim)) for _ in levels]
    lv = [np.full(per_level, L, dtype=np.int32) for L in levels]
    return np.concatenate(cs), np.concatenate(lv)


def child_points(centers, level, width):
    """the 2^d child points of cells, the oracle's expression (centre + dir * (0.25 width) / 2^level): [n, 2^d, dim]"""
    from oracle.s3_oracle import DIRS
    d = DIRS[centers.shape[1]]
    off = (0.25 * width) / np.ldexp(1.0, level.astype(np.int64))
    return centers[:, None, :] + d[None, :, :] * off[:, None, None]


def _dup(rng, n_base, dim, r):
    base = rng.random((n_base, dim))
    x = np.repeat(base, r, axis=0)
    return x[rng.permutation(len(x))]                   # copies of a point scattered over the ids


def _clusters(rng, dim, n_per, scales, dense=0):
    parts = [rng.random((n_per, dim))]
    for s in scales:
        parts.append(rng.random(dim) * 0.8 + 0.1 + s * rng.standard_normal((n_per, dim)))
    if dense:
        parts.append(np.array([0.3] * dim) + 0.02 * rng.random((dense, dim)))
    return np.concatenate(parts)


def _case(name):
    seed = sum(map(ord, name)) * 7919
    rng = np.random.default_rng(seed)
    B = Batch
    if name == "lattice2d_k8":
        # child points of levels <= 6 on lattice points (exact hits), of level 7 halfway between four (ties); children one
        # level finer
        x = lattice(256, 2)
        c, lv = tree_cells(rng, 2, (4, 5, 6, 7), 500)
        return 2, 8, knn_occupancy(8, 2), x, wide_y(rng, len(x)), [B(c, lv, 1.0, 5, 1000, (1, 1799), {"rest": True})]
    if name == "lattice2d_k7":
        x = lattice(256, 2)
        c, lv = tree_cells(rng, 2, (6, 7, 8), 400)
        return 2, 7, 1.0, x, wide_y(rng, len(x)), [B(c, lv, 1.0, 1, 600, (3, 1203), {"rest": True})]
    if name == "lattice3d_k26":
        # 1 + 6 + 12 + 8 = 27 points within sqrt(3) spacings of a lattice point: the 26th falls inside the last group
        x = lattice(64, 3)
        c, lv = tree_cells(rng, 3, (3, 4, 5), 300)
        return 3, 26, 1.0, x, wide_y(rng, len(x)), [B(c, lv, 1.0, 9, 400, (1, 1801), {"rest": True})]
    if name == "planted2d_k8":
        # a uniform cloud plus points exactly at the child points of some cells and of their children: zero distances
        # without ties, for every stage
        c, lv = random_cells(rng, 2, (7, 9, 11), 400, lo=0.05, span=0.9)
        g = child_points(c, lv, 1.0)
        gg = child_points(g.reshape(-1, 2), np.repeat(lv + 1, 4), 1.0)
        x = np.concatenate([rng.random((40_000, 2)), g.reshape(-1, 2)[::3], gg.reshape(-1, 2)[::5]])
        x = x[rng.permutation(len(x))]
        return 2, 8, knn_occupancy(8, 2), x, wide_y(rng, len(x)), [
            B(c, lv, 1.0, 2, 1200, (1, 2401), {"coop": True, "rest": True})]
    if name == "planted3d_k26":
        c, lv = random_cells(rng, 3, (6, 8), 300, lo=0.05, span=0.9)
        g = child_points(c, lv, 1.0)
        gg = child_points(g.reshape(-1, 3), np.repeat(lv + 1, 8), 1.0)
        x = np.concatenate([rng.random((60_000, 3)), g.reshape(-1, 3)[::3], gg.reshape(-1, 3)[::7]])
        x = x[rng.permutation(len(x))]
        return 3, 26, knn_occupancy(26, 3), x, wide_y(rng, len(x)), [B(c, lv, 1.0, 3, 600, (5, 2405), {"coop": True})]
    if name == "dup2d_r2_k9":
        x = _dup(rng, 15_000, 2, 2)
        c, lv = random_cells(rng, 2, (5, 7, 9), 300)
        return 2, 9, knn_occupancy(9, 2), x, wide_y(rng, len(x)), [B(c, lv, 1.0, 4, 900, (1, 1801), {"rest": True})]
    if name == "dup2d_r47_k48":
        x = _dup(rng, 1_200, 2, 47)
        c, lv = random_cells(rng, 2, (4, 6, 8), 300)
        return 2, 48, 30.0, x, wide_y(rng, len(x)), [B(c, lv, 1.0, 1, 900, (3, 1803), {"rest": True})]
    if name == "dup3d_r48_k49":
        x = _dup(rng, 600, 3, 48)
        c, lv = random_cells(rng, 3, (3, 5), 300)
        return 3, 49, knn_occupancy(49, 3), x, wide_y(rng, len(x)), [
            B(c, lv, 1.0, 2, 500, (1, 2001), {"coop": False, "near": False, "far": False, "rest": True})]
    if name == "dup2d_r49_k47":
        x = _dup(rng, 900, 2, 49)
        c, lv = random_cells(rng, 2, (5, 8), 400)
        return 2, 47, knn_occupancy(47, 2), x, wide_y(rng, len(x)), [B(c, lv, 1.0, 7, 700, (1, 1403), {"rest": True})]
    if name == "dup2d_r65_k64":
        x = _dup(rng, 500, 2, 65)
        c, lv = random_cells(rng, 2, (4, 7), 300)
        return 2, 64, knn_occupancy(64, 2), x, wide_y(rng, len(x)), [
            B(c, lv, 1.0, 1, 500, (1, 1001), {"coop": False, "near": False, "far": False, "rest": True})]
    if name == "line3d_k7":
        # collinear: zero extent along y and z, cells on and off the line
        n = 20_000
        x = np.stack([rng.random(n), np.full(n, 0.3), np.full(n, 0.6)], -1)
        c, lv = random_cells(rng, 3, (2, 5, 8), 300, lo=0.0, span=1.0)
        c[::2, 1:] = [0.3, 0.6]
        return 3, 7, knn_occupancy(7, 3), x, wide_y(rng, n), [B(c, lv, 1.0, 1, 500, (1, 2001), {})]
    if name == "plane3d_k26":
        n = 40_000
        x = np.concatenate([rng.random((n, 2)), np.full((n, 1), 0.5)], 1)
        c, lv = random_cells(rng, 3, (3, 6, 9), 300, lo=0.0, span=1.0)
        c[::2, 2] = 0.5
        return 3, 26, knn_occupancy(26, 3), x, const_y(n), [B(c, lv, 1.0, 6, 500, (1, 2001), {})]
    if name == "line2d_k2":
        n = 5_000
        x = np.stack([rng.random(n), np.full(n, 0.25)], -1)
        c, lv = random_cells(rng, 2, (3, 7, 10), 200, lo=0.0, span=1.0)
        c[::3, 1] = 0.25
        return 2, 2, knn_occupancy(2, 2), x, wide_y(rng, n), [B(c, lv, 1.0, 1, 400, (1, 801), {})]
    if name == "clusters2d_k26":
        # clusters of widths 1e-6 .. 1 (refined buckets, two-level index) and one dense patch of 70 000 points
        x = _clusters(rng, 2, 3_000, 10.0 ** -np.arange(7), dense=70_000)
        near = x[rng.choice(len(x), 600)]
        lv = rng.integers(3, 22, 600).astype(np.int32)
        return 2, 26, 30.0, x, wide_y(rng, len(x)), [B(near, lv, 1.0, 4, 500, (1, 1001), {})]
    if name == "clusters3d_k8":
        x = _clusters(rng, 3, 4_000, 10.0 ** -np.arange(7))
        near = x[rng.choice(len(x), 800)] + 1e-7 * rng.standard_normal((800, 3))
        lv = rng.integers(2, 20, 800).astype(np.int32)
        return 3, 8, knn_occupancy(8, 3), x, wide_y(rng, len(x)), [B(near, lv, 1.0, 2, 500, (3, 2003), {})]
    if name == "offset2d_k9":
        # extent 1e-3 around 1e9: coordinates on a grid of 1.2e-7, distances round to equal values
        x = 1e9 + 1e-3 * rng.random((30_000, 2))
        c, lv = tree_cells(rng, 2, (3, 6, 9, 12), 300, lo=1e9, width=1e-3)
        return 2, 9, knn_occupancy(9, 2), x, wide_y(rng, len(x)), [B(c, lv, 1e-3, 1, 900, (1, 1801), {})]
    if name == "offset3d_k26":
        # extent 1e-3 around 1e4
        x = 1e4 + 1e-3 * rng.random((50_000, 3))
        c, lv = tree_cells(rng, 3, (2, 4, 7), 300, lo=1e4, width=1e-3)
        return 3, 26, knn_occupancy(26, 3), x, const_y(len(x)), [B(c, lv, 1e-3, 1, 300, (1, 1201), {})]
    if name == "tiny2d_n1_k1":
        x = np.array([[0.3, 0.7]])
        c, lv = tree_cells(rng, 2, (0, 1, 2, 5), 20)
        c = np.concatenate([c, x])                       # one cell centred on the point
        lv = np.concatenate([lv, [3]]).astype(np.int32)
        return 2, 1, knn_occupancy(1, 2), x, np.array([-3.25]), [B(c, lv, 1.0, 1, 13, (1, 25), {})]
    if name == "tiny3d_n7_k7":
        x = rng.random((7, 3))
        c, lv = random_cells(rng, 3, (0, 2, 4), 10)
        return 3, 7, 1.0, x, wide_y(rng, 7), [B(c, lv, 1.0, 1, 17, (1, 65), {})]
    if name == "tiny2d_n10_k9":
        x = rng.random((10, 2))
        c, lv = random_cells(rng, 2, (0, 3, 6), 12)
        return 2, 9, 30.0, x, wide_y(rng, 10), [B(c, lv, 1.0, 2, 21, (3, 43), {})]
    if name == "outside3d_k8":
        # cells 1.5 to 8 cloud widths away from the unit cube (boxes beyond FAR_RMAX / FAR_ROWS) and inside it
        n = 50_000
        x = rng.random((n, 3))
        d = rng.standard_normal((600, 3))
        c = 0.5 + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(1.5, 8.0, (600, 1))
        lv = rng.integers(0, 8, 600).astype(np.int32)
        return 3, 8, knn_occupancy(8, 3), x, wide_y(rng, n), [
            B(c, lv, 1.0, 1, 600, (1, 2401), {"far": True, "rest": True})]
    if name == "outside2d_k48":
        n = 40_000
        x = rng.random((n, 2)) * [1.0, 0.2]
        c = np.stack([rng.uniform(-3, 4, 700), rng.uniform(0.4, 2.0, 700) * rng.choice([-1, 1], 700) + 0.1], -1)
        lv = rng.integers(0, 9, 700).astype(np.int32)
        return 2, 48, knn_occupancy(48, 2), x, wide_y(rng, n), [B(c, lv, 1.0, 3, 700, (1, 1401), {"far": True})]
    if name == "sweep_near2d_k8":
        # 19 200 coarse children: coop gives every one up, near's grid-stride loop runs a second sweep (> 16 384 cells)
        n = 60_000
        x = rng.random((n, 2))
        c, lv = random_cells(rng, 2, (3,), 4_800, lo=-0.05, span=1.1)
        return 2, 8, knn_occupancy(8, 2), x, wide_y(rng, n), [
            B(c, lv, 1.0, 1, 4_800, (1, 17_003), {"coop": False, "near": True})]
    if name == "sweep_far2d_k47":
        # k = 47 at occupancy 1: the boxes of coop and near are too small for every query, far answers them (> 16 384 queries
        # in one slice: a second sweep)
        n = 60_000
        x = rng.random((n, 2))
        c, lv = random_cells(rng, 2, (5,), 1_100, lo=0.0, span=1.0)
        return 2, 47, 1.0, x, wide_y(rng, n), [B(c, lv, 1.0, 1, 1_100, (3, 4_303), {"coop": False, "far": True})]
    if name == "sweep_rest3d_k49":
        # k = 49 > COOP_CAP: every query to the per-lane rest, > 32 768 of them in one slice
        n = 100_000
        x = rng.random((n, 3))
        c, lv = random_cells(rng, 3, (4,), 700, lo=0.0, span=1.0)
        return 3, 49, knn_occupancy(49, 3), x, wide_y(rng, n), [
            B(c, lv, 1.0, 1, 700, (1, 5_001), {"coop": False, "near": False, "far": False, "rest": True})]
    if name == "uniform3d_k48":
        # fine cells of a uniform cloud with k = COOP_CAP: coop answers most
        n = 150_000
        x = rng.random((n, 3))
        c, lv = random_cells(rng, 3, (5, 6), 400, lo=0.05, span=0.9)
        return 3, 48, knn_occupancy(48, 3), x, wide_y(rng, n), [B(c, lv, 1.0, 1, 500, (5, 2005), {"coop": True})]
    if name == "uniform2d_k26_odd":
        # odd n (a half-empty workgroup) and n = 1 slices of an ordinary fine batch
        n = 80_000
        x = rng.random((n, 2))
        c, lv = random_cells(rng, 2, (6, 7), 500, lo=0.05, span=0.9)
        return 2, 26, knn_occupancy(26, 2), x, wide_y(rng, n), [B(c, lv, 1.0, 1, 801, (1, 2, 1601), {"coop": True})]
    raise KeyError(name)


NAMES = ("lattice2d_k8", "lattice2d_k7", "lattice3d_k26", "planted2d_k8", "planted3d_k26", "dup2d_r2_k9", "dup2d_r47_k48",
         "dup3d_r48_k49", "dup2d_r49_k47", "dup2d_r65_k64", "line3d_k7", "plane3d_k26", "line2d_k2", "clusters2d_k26",
         "clusters3d_k8", "offset2d_k9", "offset3d_k26", "tiny2d_n1_k1", "tiny3d_n7_k7", "tiny2d_n10_k9", "outside3d_k8",
         "outside2d_k48", "sweep_near2d_k8", "sweep_far2d_k47", "sweep_rest3d_k49", "uniform3d_k48", "uniform2d_k26_odd")


@functools.lru_cache(maxsize=None)
def case(name):
    """(name, dim, k, occupancy, cloud, y, batches); deterministic"""
    dim, k, occ, x, y, batches = _case(name)
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    assert x.shape[1] == dim and len(y) == len(x) and 1 <= k <= min(64, len(x))
    for b in batches:
        assert len(b.centers) == len(b.level) and b.n_par <= len(b.centers)
        assert list(b.cuts) == sorted(b.cuts) and 0 < b.cuts[0] and b.cuts[-1] < b.n_par * 2 ** dim
    return name, dim, k, float(occ), x, y, batches


def cases():
    return [case(n) for n in NAMES]


def children(b, dim, seed=0):
    """the parents of the second generation (ids of the root batch's cells, a permutation) and the children's centres and
    levels by the oracle's expression (the GPU's s3_make_children computes the same bits)"""
    rng = np.random.default_rng(seed + len(b.centers))
    pick = rng.permutation(len(b.centers))[:b.n_par]
    cen = child_points(b.centers[pick], b.level[pick], b.width).reshape(-1, dim)
    return b.first + pick, cen, np.repeat(b.level[pick] + 1, 2 ** dim).astype(np.int32)


def slices(b, dim):
    cuts = [0] + list(b.cuts) + [b.n_par * 2 ** dim]
    return list(zip(cuts[:-1], cuts[1:]))
