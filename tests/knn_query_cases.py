"""
Hostile inputs for the query path of the export's KNN cache (csrc/knn.hip: knn_query_kernel, idw_predict_kernel and
idw_weights_kernel, all on knn_search / ring_search and its second-level sub-lattices), shared by tests/test_gpu_knn_query.py
(the GPU against the oracle) and tests/test_knn_query_cases_oracle.py (the oracle and the cases themselves, CPU only).  No GPU
and no package import here.

A case is ``(name, dim, k, occupancy, cloud, y, queries)``:
  occupancy -- the KNN index's target points per bucket; 0.0 is the index default (3 in 2-D, 8 in 3-D);
  cloud, y  -- the points [n, dim] and the values [n] (float64);
  queries   -- [nq, dim] (float64).
A name that ends in ``_occ1`` / ``_occ40`` is the case without the suffix (same cloud, values and queries) at that occupancy.

The property sets below name the cases whose purpose depends on a property of the generated data; the CPU test checks that
the data still has it.

The pruning margin (MARGIN_CASES).  ring_search shrinks every lower bound by 1e-9 bucket sides; a bucket face
``lo + i * h`` carries a rounding error of about ulp(|lo|).  The margin no longer covers that error once
ulp(|lo|) > 1e-9 h, i.e. |lo| / h > 4.5e6:
  offset2d_lat_k8 / _k9   lattice(128, 2) * 1e-3 + 1e9: 74 x 74 buckets of side 1.34e-5,  |lo| / h = 7.5e13
  offset3d_lat_k26        lattice(32, 3) * 1e-3 + 1e4:  16^3 buckets of side 6.05e-5,     |lo| / h = 1.65e8
  wall{2,3}d_o4096_*      the graded wall cloud at +4096: ulp = 9.1e-13 against sub-bucket sides of 2.8e-5 .. 7.3e-4:
                          ulp / (1e-9 h_sub) = 12.8, 32.3, 1.24 in 2-D and 1.55, 5.17 in 3-D (default occupancy, 1, 40); in 3-D at
                          occupancy 40 it is 0.47: that case runs, but is not in MARGIN_CASES
  fine2d_o96_k8_occ1      at +96 (ulp = 1.4e-14) a sub-bucket side below 1.4e-5 is needed.  With spacings 2^-6 .. 2^-20 the top-level
                          side is sqrt(occupancy * 2^-6 * mean normal spacing) and a bucket of one column holds side / 2^-20
                          points, so the finest sub-bucket side is sqrt(side) / 1024 at occupancy 1 and larger at every other:
                          only a cloud whose layers are nearly all 2^-20 apart reaches it, and only in 2-D at occupancy 1.  This
                          case is that cloud (18 000 layers of 2^-20, then one of each coarser spacing, two columns): sub-bucket
                          side 1.11e-5, ulp / (1e-9 h_sub) = 1.28.
The wall{2,3}d_o96_* cases (ulp / (1e-9 h_sub) = 0.007 .. 0.5) run all the same; they are in REFINED_CASES, not in MARGIN_CASES.

The face between assignment and search (FACE_CASES).  What the margin covers in practice is the other end: a point is assigned
to a bucket by ``int((x - lo) * inv_h)``, the search takes the bucket's face as ``fl(lo + i * h)``, and h * inv_h != 1.  With
lo = 0 the double just below a computed face is assigned to the bucket above it for about a third of all faces.  face{2,3}d_top_k1
plant such points along every axis of the top-level grid, face{2,3}d_sub_k1 inside a refined bucket against sub_cell_of /
sub_lattice; see _face_case.  Without the margin in ring_search's gap2 these cases return the wrong neighbour.
"""
import functools
import os
import re

import numpy as np

from tests.child_metric_cases import _dup, const_y, flat, lattice, wide_y  # noqa: F401  (flat, const_y: for the tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _max_k():
    with open(os.path.join(ROOT, "include", "s3hip.h")) as f:
        return int(re.search(r"^#define\s+S3_MAX_K\s+(\d+)", f.read(), re.M).group(1))


S3_MAX_K = _max_k()
SUB_RES_MAX = 32                   # csrc/knn.hip
BRUTE_MAX_EVALS = 1.2e8            # distance evaluations of the brute-force reference per case

K_ENDS = (1, 2, 7, 8, 9, 15, 16, 17, 26, 32, S3_MAX_K - 1, S3_MAX_K)
WALL_OFFSETS = (96, 4096)


# ---- the index's own plan, restated (s3_knn_create and sub_plan_kernel) -------------------------------------------------------
def index_grid(x, occupancy):
    """(lo, h, inv_h, res, occ) of the top-level bucket grid s3_knn_create builds over x: h = e / res and inv_h = res / e, each
    rounded on its own (h * inv_h != 1)"""
    n, dim = x.shape
    lo, hi = x.min(0), x.max(0)
    occ = occupancy if occupancy > 0 else (3.0 if dim == 2 else 8.0)
    ext = hi - lo
    nz = int((ext > 0).sum())
    vol = float(np.prod(ext[ext > 0])) if nz else 1.0
    s = (vol / max(1.0, n / occ)) ** (1.0 / nz) if nz else 1.0
    rmax = 8192 if dim == 2 else 512
    res = np.ones(dim, dtype=np.int64)
    for j in range(dim):
        if ext[j] > 0 and s > 0:
            res[j] = int(min(float(rmax), max(1.0, np.ceil(ext[j] / s))))
    e = np.where(ext > 0, ext * (1.0 + 1e-12), 1.0)
    return lo, e / res, res / e, res, occ


def index_plan(x, occupancy):
    """(lo, h, res, occ) of that grid"""
    lo, h, _, res, occ = index_grid(x, occupancy)
    return lo, h, res, occ


def top_cell(x, lo, inv_h, res):
    """cell_coord of csrc/knn.hip: the bucket coordinates of points"""
    return np.clip((x - lo) * inv_h, 0.0, res - 1.0).astype(np.int64)


def unclamped_resolution(x, occupancy):
    """the resolution the create formula asks for before the clamp"""
    n, dim = x.shape
    ext = x.max(0) - x.min(0)
    occ = occupancy if occupancy > 0 else (3.0 if dim == 2 else 8.0)
    nz = int((ext > 0).sum())
    s = (float(np.prod(ext[ext > 0])) / max(1.0, n / occ)) ** (1.0 / nz)
    return np.where(ext > 0, np.ceil(ext / s), 1.0)


def sub_plan(x, occupancy):
    """per refined top-level bucket: (bucket coordinates [m, dim], count [m], r [m]) -- sub_plan_kernel's rule"""
    lo, h, inv_h, res, occ = index_grid(x, occupancy)
    dim = x.shape[1]
    t = top_cell(x, lo, inv_h, res)
    cells, cnt = np.unique(t, axis=0, return_counts=True)
    split = int(np.ceil(8.0 * occ))
    big = cnt > split
    r = np.ceil((cnt[big] / occ) ** (1.0 / dim)).astype(np.int64)
    r = np.minimum(np.maximum(r, 2), SUB_RES_MAX)
    return cells[big], cnt[big], r


def margin_ratio(x, occupancy):
    """max over the lattices the search walks (the top level, every refined bucket's sub-lattice) of
    ulp(|lo|) / (1e-9 * hmin): above 1 the pruning margin is smaller than the rounding error of a bucket face"""
    lo, h, res, _ = index_plan(x, occupancy)
    best = float(np.spacing(np.abs(lo)).max() / (1e-9 * h.min()))
    cells, _, r = sub_plan(x, occupancy)
    if len(cells):
        sub_lo = lo + cells * h
        best = max(best, float((np.spacing(np.abs(sub_lo)).max(1) / (1e-9 * h.min() / r)).max()))
    return best


# ---- clouds and queries ----------------------------------------------------------------------------------------------------
def _dup_cloud(rng, n_base, dim, r):
    """child_metric_cases._dup on a 2^-20 grid: the midpoint of two base points and its distances to both are exact"""
    return np.round(_dup(rng, n_base, dim, r) * 2.0 ** 20) / 2.0 ** 20


def _dup_queries(rng, x, n_each):
    """at base points (zero distances), midway between a base point and its nearest other base point (two whole tie groups at
    one exact distance), and random"""
    base = np.unique(x, axis=0)
    a = base[rng.choice(len(base), min(n_each, len(base)), replace=False)]
    d = ((a[:, None, :] - base[None, :, :]) ** 2).sum(-1)
    d[d == 0.0] = np.inf
    b = base[d.argmin(1)]
    return np.concatenate([a, (a + b) / 2, rng.random((n_each, x.shape[1])) * 1.2 - 0.1])


def wall_cloud(dim, n_wall, layers, offset):
    """a structured boundary-layer cloud: ``layers`` = ((p, m), ...) is m layers 2^-p apart, from the wall outwards, along the
    last axis; 2^-6 apart along the wall; everything translated by ``offset``.  Every coordinate is a multiple of 2^-20 below
    2^13: exact, and so is every distance between points and the queries of wall_queries"""
    normal = np.concatenate([[0.0], np.cumsum(np.concatenate([np.full(m, 2.0 ** -p) for p, m in layers]))])
    along = np.arange(n_wall) * 2.0 ** -6
    x = np.stack(np.meshgrid(*([along] * (dim - 1) + [normal]), indexing="ij"), -1).reshape(-1, dim)
    return x + float(offset), normal + float(offset)


WALL_LAYERS = tuple((p, max(1, 2 ** (p - 11))) for p in range(20, 5, -1))     # 2^-11 of each spacing 2^-20 .. 2^-11, then one each
FINE_LAYERS = ((20, 18_000),) + tuple((p, 1) for p in range(19, 5, -1))


def wall_queries(rng, x, normal, n_each):
    """at points; at midpoints of the finest spacing (next to the wall) and of the coarsest (the outer layers, between columns);
    just outside the cloud on the fine side"""
    dim = x.shape[1]
    lo = x.min(0)
    at = x[rng.choice(len(x), n_each, replace=False)]
    near_wall = x[x[:, -1] < normal[0] + 2.0 ** -12]
    fine = near_wall[rng.choice(len(near_wall), n_each)] + np.r_[np.zeros(dim - 1), 2.0 ** -21]
    outer = x[x[:, -1] >= normal[-3]]
    coarse = outer[rng.choice(len(outer), n_each)] + np.r_[np.full(dim - 1, 2.0 ** -7), -2.0 ** -7]
    below = near_wall[rng.choice(len(near_wall), n_each)].copy()
    below[:, -1] = lo[-1] - rng.choice([2.0 ** -21, 2.0 ** -20, 2.0 ** -10, 1e-7], n_each)
    below[::2, :-1] += 2.0 ** -7
    return np.concatenate([at, fine, coarse, below])


def outside_queries(rng, x):
    """1x, 10x and 1000x the cloud's largest extent away from its bounding box along each axis and along each diagonal; exactly
    on every face (random points and the face centre) and on every corner of the box"""
    dim = x.shape[1]
    lo, hi = x.min(0), x.max(0)
    c, half, big = (lo + hi) / 2, (hi - lo) / 2, (hi - lo).max()
    signs = np.stack(np.meshgrid(*[[-1.0, 1.0]] * dim, indexing="ij"), -1).reshape(-1, dim)
    q = []
    for m in OUTSIDE_MULTIPLES:
        for j in range(dim):
            for s in (-1.0, 1.0):
                e = np.zeros(dim)
                e[j] = s
                q.append(c + e * (half + m * big))
        q += [c + s * (half + m * big) for s in signs]
    for j in range(dim):
        for side in (lo, hi):
            f = lo + (hi - lo) * rng.random((6, dim))
            f[0] = c
            f[:, j] = side[j]
            q += list(f)
    q += [np.where(s > 0, hi, lo) for s in signs]
    return np.array(q)


OUTSIDE_MULTIPLES = (1, 10, 1000)


def _clamp_cloud(rng, dim):
    if dim == 3:
        return rng.random((100_000, 3)) * [1e4, 1.0, 1.0]
    return rng.random((60_000, 2)) * [1e6, 1.0]


def _clamp_queries(rng, x, n_each):
    """along the long axis, off its ends, and 100 x the short extent to the side"""
    dim = x.shape[1]
    L = x.max(0)
    inside = rng.random((n_each, dim)) * L
    ends = rng.random((n_each, dim)) * L
    ends[:, 0] = np.where(rng.random(n_each) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-3, 4.5, n_each)
    ends[ends[:, 0] > 0, 0] += L[0]
    side = rng.random((n_each, dim)) * L
    side[:, 1] = 100.0 * L[1] * rng.choice([-1.0, 1.0], n_each) + (side[:, 1] > 0.5 * L[1]) * L[1]
    return np.concatenate([inside, ends, side, x[rng.choice(len(x), n_each)]])


def face_slots(base, h, inv, r, first=2):
    """the buckets i of one axis of a lattice (origin ``base``, side ``h``, r buckets, points assigned by
    ``int((x - base) * inv)``) whose lower face the search computes one ulp ABOVE a point of bucket i:
    x = the double below fl(base + i * h) is assigned to i, q = x - 8 ulp to i - 1.  -> [(i, face, x, q, ulp)]"""
    out = []
    for i in range(first, r + 1 - first):
        face = base + i * h
        xx = np.nextafter(face, -np.inf)
        u = face - xx
        qq = xx - 8 * u
        if np.spacing(qq - 8 * u) == u and int((xx - base) * inv) == i and int((qq - base) * inv) == i - 1:
            out.append((i, face, xx, qq, u))
    return out


FACE_TRIPLETS = {}                 # name -> [(id of x, id of y, query number, axis, lattice)], filled by _face_case


def _face_case(rng, name, dim, sub):
    """a uniform cloud over [0, ext] whose only points near the queries are planted pairs: x one ulp below a computed bucket
    face and assigned to the bucket above it, the query q 8 ulp below x in the bucket below, and y in q's bucket, either 8 ulp
    below q (a tie; x has the smaller id) or, at the top level, 8 ulp below and 4 ulp aside (x strictly nearer).  The face is 9 ulp from q: a
    search that prunes bucket i by its computed face without a margin returns y.  ``sub``: inside a refined bucket, against
    the faces of its sub-lattice (sub_cell_of against sub_lattice)"""
    n, n_cluster = (3_000, 100) if dim == 2 else (20_000, 300)
    for _ in range(100):                                        # an extent with two such faces along every axis
        ext = 0.5 + 0.5 * rng.random(dim)
        pts = rng.random((n, dim)) * ext
        pts[0], pts[1] = 0.0, ext
        lo, h, inv_h, res, occ = index_grid(pts, 0.0)
        if sub:
            cc = res // 2
            cc[0] = 0            # (origin 0 along the axis of the faces: further out, the faces are resolved no finer than the points)
            base = lo + cc * h
            r = int(min(max(np.ceil((n_cluster / occ) ** (1.0 / dim)), 2), SUB_RES_MAX))
            lattices = [(0, base, h / r, r * inv_h, r, "sub")]
        else:
            lattices = [(j, lo, h, inv_h, int(res[j]), "top") for j in range(dim)]
        if all(len(face_slots(b[a], hh[a], inv[a], r_, 1 if sub else 2)) >= 2 for a, b, hh, inv, r_, _ in lattices):
            break
    else:
        raise AssertionError(name)
    planted, queries, triplets = [], [], []
    for axis, base, hh, inv, r, kind in lattices:
        slots = face_slots(base[axis], hh[axis], inv[axis], r, 1 if sub else 2)
        for variant, s in enumerate(rng.permutation(len(slots))[:2]):
            i, face, xx, qq, u = slots[s]
            side = (axis + 1) % dim
            for _ in range(100):
                if sub:
                    q = base + h * np.r_[0.0, 0.55 + 0.3 * variant, [0.5] * (dim - 2)][:dim]
                else:
                    q = (rng.integers(3, res - 3) + 0.5) * h
                q[axis] = qq
                x_, y_ = q.copy(), q.copy()
                x_[axis], y_[axis] = xx, qq - 8 * u
                strict = variant and not sub                  # (in a sub-lattice next to the origin 4 ulp aside is no double)
                if strict:
                    y_[side] += 4 * u
                dx, dy = ((q - x_) ** 2).sum(), ((q - y_) ** 2).sum()
                far = all(np.abs((q - q2) / h).max() > 3 for q2 in queries) or sub
                if far and (dx < dy < (face - qq) ** 2 if strict else dx == dy):
                    break
            else:
                raise AssertionError(name)
            planted += [x_, y_]
            queries.append(q)
            triplets.append((len(planted) - 2, len(planted) - 1, len(queries) - 1, axis, kind))
    queries = np.array(queries)
    first = 2
    if sub:
        # the refined bucket: the planted pairs and points in its lower third along axis 1, nothing else
        fill = base + h * rng.random((n_cluster - len(planted), dim)) * np.r_[1.0, 0.3, [1.0] * (dim - 2)][:dim]
        pts[2:2 + len(fill)] = fill
        first = 2 + len(fill)
    pts[first:first + len(planted)] = planted
    free = np.arange(first + len(planted), n)
    for _ in range(100):                                        # no other point within three bucket sides of a query
        near = (np.abs((pts[free, None, :] - queries[None, :, :]) / h).max(-1) < 3).any(1)
        if sub:
            near |= (top_cell(pts[free], lo, inv_h, res) == cc).all(1)
        if not near.any():
            break
        pts[free[near]] = rng.random((int(near.sum()), dim)) * ext
    else:
        raise AssertionError(name)
    FACE_TRIPLETS[name] = [(first + a, first + b, c, axis, kind) for a, b, c, axis, kind in triplets]
    q_all = np.concatenate([queries, rng.random((40, dim)) * ext])
    return dim, 1, 0.0, pts, wide_y(rng, n), q_all


def face_triplets(name):
    case(name)
    return FACE_TRIPLETS[name]


def _base_name(name):
    return re.sub(r"_occ(1|40)$", "", name)


def _case(name):
    base = _base_name(name)
    occ = {"": 0.0, "_occ1": 1.0, "_occ40": 40.0}[name[len(base):]]
    rng = np.random.default_rng(sum(map(ord, base)) * 7919)
    m = re.fullmatch(r"dup([23])d_r(\d+)_k(\d+)", base)
    if m:
        # every base point r times, the copies scattered over the ids: r < k, r = k and r = k + 1
        dim, r, k = map(int, m.groups())
        x = _dup_cloud(rng, 6_000 // r, dim, r)
        return dim, k, occ, x, wide_y(rng, len(x)), _dup_queries(rng, x, 120)
    if base == "bigdup2d_k26":
        # 10 000 copies of one point: its bucket is refined to SUB_RES_MAX and stays one sub-bucket
        x = np.concatenate([np.tile([0.37, 0.61], (10_000, 1)), rng.random((5_000, 2))])
        x = x[rng.permutation(len(x))]
        q = np.concatenate([[[0.37, 0.61]], [0.37, 0.61] + 1e-3 * rng.standard_normal((60, 2)), x[rng.choice(len(x), 60)],
                            rng.random((140, 2)) * 1.2 - 0.1])
        return 2, 26, occ, x, wide_y(rng, len(x)), q
    if base == "tiny2d_n1_k1":
        x = np.array([[0.3, 0.7]])
        return 2, 1, occ, x, np.array([-3.25]), np.concatenate([x, rng.random((8, 2)) * 4 - 2])
    if base == "tiny3d_n26_k26":
        x = rng.random((26, 3))
        return 3, 26, occ, x, wide_y(rng, 26), np.concatenate([x[:5], rng.random((40, 3)) * 3 - 1])
    m = re.fullmatch(r"same([23])d_n500_k(\d+)", base)
    if m:
        # all points identical: no extent at all (h = 1, one bucket)
        dim, k = map(int, m.groups())
        x = np.tile(rng.random(dim), (500, 1))
        return dim, k, occ, x, wide_y(rng, 500), np.concatenate([x[:3], x[:40] + rng.standard_normal((40, dim))])
    if base in ("line3d_k8", "plane3d_k26"):
        # two / one zero extents; queries on and off the line (plane) and beyond its ends
        n, fixed = 5_000, ((1, 0.3), (2, 0.6)) if base == "line3d_k8" else ((2, 0.5),)
        x = rng.random((n, 3))
        q = rng.random((300, 3))
        q[200:] = q[200:] * 30 - 15
        q[250:] *= 100
        for j, v in fixed:
            x[:, j] = v
            q[::2, j] = v
        q = np.concatenate([q, x[:20]])
        return 3, 8 if base == "line3d_k8" else 26, occ, x, wide_y(rng, n), q
    if base in ("clamp3d_k8", "clamp2d_k9"):
        dim = int(base[5])
        x = _clamp_cloud(rng, dim)
        return dim, int(base.split("_k")[1]), occ, x, wide_y(rng, len(x)), _clamp_queries(rng, x, 250)
    if base in ("offset2d_lat_k8", "offset2d_lat_k9", "offset3d_lat_k26"):
        # queries at lattice points, cell centres and edge midpoints (as float64 forms them from the translated points)
        dim = int(base[6])
        m_, off = (128, 1e9) if dim == 2 else (32, 1e4)
        x = off + 1e-3 * lattice(m_, dim)
        g = x.reshape((m_,) * dim + (dim,))
        inner = g[(slice(0, m_ - 1),) * dim].reshape(-1, dim)
        far = g[(slice(1, m_),) * dim].reshape(-1, dim)
        edge = g[(slice(1, m_),) + (slice(0, m_ - 1),) * (dim - 1)].reshape(-1, dim)
        pick = rng.choice(len(inner), 250, replace=False)
        q = np.concatenate([x[rng.choice(len(x), 250, replace=False)], (inner[pick] + far[pick]) / 2,
                            (inner[pick] + edge[pick]) / 2])
        return dim, int(base.split("_k")[1]), occ, x, wide_y(rng, len(x)), q
    m = re.fullmatch(r"wall([23])d_o(\d+)_k(\d+)", base)
    if m:
        dim, off, k = map(int, m.groups())
        x, normal = wall_cloud(dim, 16 if dim == 2 else 6, WALL_LAYERS, off)
        q = wall_queries(rng, x, normal, 120)
        p = rng.permutation(len(x))
        return dim, k, occ, x[p], wide_y(rng, len(x)), q
    if base == "fine2d_o96_k8":
        x, normal = wall_cloud(2, 2, FINE_LAYERS, 96)
        q = wall_queries(rng, x, normal, 120)
        p = rng.permutation(len(x))
        return 2, 8, occ, x[p], wide_y(rng, len(x)), q
    if base in ("outside3d_uniform_k8", "outside2d_graded_k8", "outside3d_clamp_k8"):
        if base == "outside3d_uniform_k8":
            x = rng.random((20_000, 3))
        elif base == "outside2d_graded_k8":
            x = wall_cloud(2, 16, WALL_LAYERS, 0)[0]
            x = x[rng.permutation(len(x))]
        else:
            x = _clamp_cloud(rng, 3)
        return x.shape[1], 8, occ, x, wide_y(rng, len(x)), outside_queries(rng, x)
    m = re.fullmatch(r"kend3d_k(\d+)", base)
    if m:
        # one cloud for every k; queries at points and at random
        k = int(m.group(1))
        cloud = np.random.default_rng(4242)
        x = cloud.random((3_000, 3))
        q = np.concatenate([x[cloud.choice(3_000, 150, replace=False)], cloud.random((250, 3)) * 1.2 - 0.1])
        return 3, k, occ, x, wide_y(rng, 3_000), q
    m = re.fullmatch(r"face([23])d_(top|sub)_k1", base)
    if m:
        return _face_case(rng, base, int(m.group(1)), m.group(2) == "sub")
    raise KeyError(name)


def _with_occupancies(names):
    return tuple(n + s for n in names for s in ("", "_occ1", "_occ40"))


DUP_BASE = tuple(f"dup{d}d_r{r}_k{k}" for d in (2, 3) for k in (8, 26) for r in (k - 1, k, k + 1))
WALL_BASE = tuple(f"wall{d}d_o{o}_k{k}" for d, k in ((2, 8), (3, 26)) for o in WALL_OFFSETS)
DUP_CASES = _with_occupancies(DUP_BASE)
WALL_CASES = _with_occupancies(WALL_BASE)
DEGENERATE_CASES = ("tiny2d_n1_k1", "tiny3d_n26_k26", "same2d_n500_k8", "same3d_n500_k26", "line3d_k8", "plane3d_k26")
LATTICE_CASES = ("offset2d_lat_k8", "offset2d_lat_k9", "offset3d_lat_k26")
K_END_CASES = tuple(f"kend3d_k{k}" for k in K_ENDS)

ZERO_CASES = DUP_CASES + ("bigdup2d_k26",) + DEGENERATE_CASES + LATTICE_CASES + WALL_CASES + ("fine2d_o96_k8_occ1",) \
    + K_END_CASES                                                             # a query on a point
TIE_CASES = DUP_CASES + ("bigdup2d_k26", "same2d_n500_k8", "same3d_n500_k26") + WALL_CASES + ("fine2d_o96_k8_occ1",)
#                                                                               a tie group straddles the k-th neighbour
OUTSIDE_CASES = ("outside3d_uniform_k8", "outside2d_graded_k8", "outside3d_clamp_k8")
REFINED_CASES = ("bigdup2d_k26", "same2d_n500_k8", "same3d_n500_k26") + WALL_CASES \
    + ("fine2d_o96_k8_occ1", "outside2d_graded_k8", "face2d_sub_k1", "face3d_sub_k1")
#                                                                               buckets with a sub-lattice
FULL_SUB_CASES = ("bigdup2d_k26",)                                            # ... one of them at SUB_RES_MAX
CLAMP_CASES = ("clamp3d_k8", "clamp2d_k9", "outside3d_clamp_k8")               # an axis at the resolution clamp
MARGIN_CASES = LATTICE_CASES + tuple(n for n in WALL_CASES if "_o4096_" in n and n != "wall3d_o4096_k26_occ40") \
    + ("fine2d_o96_k8_occ1",)
#                                                                               ulp(|lo|) > 1e-9 h on some lattice

FACE_CASES = ("face2d_top_k1", "face3d_top_k1", "face2d_sub_k1", "face3d_sub_k1")
#                                                                               a point one ulp on the far side of a computed face

NAMES = DUP_CASES + ("bigdup2d_k26",) + DEGENERATE_CASES + ("clamp3d_k8", "clamp2d_k9") + LATTICE_CASES + WALL_CASES \
    + ("fine2d_o96_k8_occ1",) + OUTSIDE_CASES + K_END_CASES + FACE_CASES


@functools.lru_cache(maxsize=None)
def case(name):
    """(name, dim, k, occupancy, cloud, y, queries); deterministic"""
    dim, k, occ, x, y, q = _case(name)
    x, y, q = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, q))
    assert x.shape[1] == dim == q.shape[1] and len(y) == len(x) and 1 <= k <= min(S3_MAX_K, len(x))
    assert len(x) <= 100_000 and len(q) <= 2_000 and len(x) * len(q) <= BRUTE_MAX_EVALS, name
    return name, dim, k, float(occ), x, y, q


def cases():
    return [case(n) for n in NAMES]


# ---- the weights' clamp -----------------------------------------------------------------------------------------------------
CLAMP_SPECIALS = (0.0, 0.0, 1e-12, float(np.nextafter(1e-12, 0.0)), 5e-324, 1e-300, 1.0)
WEIGHT_KS = (1, 7, 8, 9, 26, S3_MAX_K)
WEIGHT_ROWS = (1, 255, 256, 257)


def adversarial_dist(nc, k):
    """[nc, k] distances: the values at and below the 1e-12 clamp (exactly 0 twice, 1e-12, the double just below it, a
    denormal, 1e-300) and 1 at the head of every row, rotated by the row number, the rest 1e-14 .. 1e2"""
    rng = np.random.default_rng(1000 * k + nc)
    d = 10.0 ** rng.uniform(-14, 2, (nc, max(k, len(CLAMP_SPECIALS))))
    d[:, :len(CLAMP_SPECIALS)] = CLAMP_SPECIALS
    for c in range(nc):
        d[c] = np.roll(d[c], c)
    return np.ascontiguousarray(d[:, :k])
