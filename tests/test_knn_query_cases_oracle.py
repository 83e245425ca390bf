"""
The reference of tests/test_gpu_knn_query.py and the cases it runs, on the CPU: each case still has the property it exists for
(a zero distance, a tie group across the k-th neighbour, queries outside, refined buckets, the resolution clamp, a pruning
margin below the rounding error of a bucket face); the oracle's brute-force query equals a numpy restatement, returns a true
k-nearest set by exact long-double distances, and equals the oracle's bucket grid; its weights and predictions stay within
their rounding bound of a long-double evaluation.
"""
import numpy as np
import pytest

from oracle import s3_oracle as orc
from tests import knn_query_cases as kc

SMALL = 20_000               # points up to which every query is checked here; above, a sample (the GPU test checks them all)
SAMPLE = 200
EPS = 2.0 ** -53
FAR_SAMPLE = 4               # far queries of a clamp cloud put to the oracle's bucket grid


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _queries(name):
    _, dim, k, occ, x, y, q = kc.case(name)
    if len(x) > SMALL and len(q) > SAMPLE:
        q = q[np.sort(np.random.default_rng(len(q)).choice(len(q), SAMPLE, replace=False))]
    return q


def _rdist(x, q):
    """((q0-p0)**2 + (q1-p1)**2) + (q2-p2)**2 in float64, [len(q), len(x)]"""
    t = q[:, None, 0] - x[None, :, 0]
    d = t * t
    for j in range(1, x.shape[1]):
        t = q[:, None, j] - x[None, :, j]
        d = d + t * t
    return d


def _rdist_exact(x, q):
    xl, ql = x.astype(np.longdouble), q.astype(np.longdouble)
    d = np.zeros((len(q), len(x)), dtype=np.longdouble)
    for j in range(x.shape[1]):
        t = ql[:, None, j] - xl[None, :, j]
        d += t * t
    return d


def restated_knn(x, q, k, chunk=64):
    """neighbours by np.lexsort((idx, rd)) of the float64 reduced distances (over the points not beyond the k-th smallest
    value: the others cannot be among the first k), dist = sqrt(rd)"""
    idx = np.empty((len(q), k), dtype=np.int64)
    dist = np.empty((len(q), k))
    for s in range(0, len(q), chunk):
        rd = _rdist(x, q[s:s + chunk])
        kth = np.partition(rd, k - 1, axis=1)[:, k - 1]
        for r in range(len(rd)):
            cand = np.flatnonzero(rd[r] <= kth[r])
            order = cand[np.lexsort((cand, rd[r, cand]))][:k]
            idx[s + r], dist[s + r] = order, np.sqrt(rd[r, order])
    return idx, dist


_BRUTE = {}


def brute(name):
    """orc.knn on the case's (sampled) queries, computed once"""
    if name not in _BRUTE:
        _, dim, k, occ, x, y, q = kc.case(name)
        _BRUTE[name] = orc.knn(x, _queries(name), k)
    return _BRUTE[name]


def test_case_table_is_complete():
    assert len(set(kc.NAMES)) == len(kc.NAMES)
    for group in (kc.ZERO_CASES, kc.TIE_CASES, kc.OUTSIDE_CASES, kc.REFINED_CASES, kc.FULL_SUB_CASES, kc.CLAMP_CASES,
                  kc.MARGIN_CASES, kc.FACE_CASES):
        assert group and set(group) <= set(kc.NAMES)
    ks = {kc.case(n)[2] for n in kc.K_END_CASES}
    assert ks == {1, 2, 7, 8, 9, 15, 16, 17, 26, 32, kc.S3_MAX_K - 1, kc.S3_MAX_K}
    assert {(d, k, r - k) for d in (2, 3) for k in (8, 26) for r in (k - 1, k, k + 1)} == {
        (int(n[3]), kc.case(n)[2], int(n.split("_r")[1].split("_")[0]) - kc.case(n)[2]) for n in kc.DUP_BASE}
    for n in kc.DUP_CASES + kc.WALL_CASES:
        base = kc.case(kc._base_name(n))
        assert all(np.array_equal(a, b) for a, b in zip(kc.case(n)[4:], base[4:]))
    assert {kc.case(n)[3] for n in kc.DUP_CASES} == {0.0, 1.0, 40.0} == {kc.case(n)[3] for n in kc.WALL_CASES}


# ---- the data has its property ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", kc.ZERO_CASES)
def test_zero_cases_have_a_zero_distance(name):
    assert (brute(name)[1][:, 0] == 0.0).any()


@pytest.mark.parametrize("name", kc.TIE_CASES)
def test_tie_cases_straddle_the_kth_neighbour(name):
    """some query whose k-th and (k+1)-th reduced distances are equal in float64"""
    _, dim, k, occ, x, y, q = kc.case(name)
    assert k < len(x)
    for s in range(0, len(q), 64):
        two = np.partition(_rdist(x, q[s:s + 64]), (k - 1, k), axis=1)[:, k - 1:k + 1]
        if (two[:, 0] == two[:, 1]).any():
            return
    pytest.fail(f"{name}: no tie across the k-th neighbour")


@pytest.mark.parametrize("name", kc.OUTSIDE_CASES)
def test_outside_cases_are_outside(name):
    _, dim, k, occ, x, y, q = kc.case(name)
    lo, hi = x.min(0), x.max(0)
    gap = np.maximum(lo - q, q - hi)
    big = (hi - lo).max()
    for m in kc.OUTSIDE_MULTIPLES:
        for j in range(dim):                                          # along each axis, both ways
            others = np.delete(np.arange(dim), j)
            on_axis = (gap[:, j] == gap.max(1)) & (gap[:, others] <= 0).all(1) & np.isclose(gap[:, j], m * big, rtol=1e-6)
            assert (on_axis & (q[:, j] < lo[j])).any() and (on_axis & (q[:, j] > hi[j])).any(), (name, m, j)
        assert (np.isclose(gap, m * big, rtol=1e-6).all(1)).sum() >= 2 ** dim, (name, m)        # along each diagonal
    inside = (gap <= 0).all(1)
    for j in range(dim):
        assert (inside & (q[:, j] == lo[j])).any() and (inside & (q[:, j] == hi[j])).any()        # on every face
    assert ((q == lo) | (q == hi)).all(1).sum() >= 2 ** dim                                       # on every corner


@pytest.mark.parametrize("name", kc.REFINED_CASES)
def test_refined_cases_have_overfull_buckets(name):
    _, dim, k, occ, x, y, q = kc.case(name)
    cells, cnt, r = kc.sub_plan(x, occ)
    assert len(cells) > 0
    if name in kc.FULL_SUB_CASES:
        # refined to SUB_RES_MAX, and a group of identical points that no lattice can split
        assert r.max() == kc.SUB_RES_MAX
        assert np.unique(x, axis=0, return_counts=True)[1].max() >= 10_000


@pytest.mark.parametrize("name", kc.CLAMP_CASES)
def test_clamp_cases_reach_the_resolution_clamp(name):
    _, dim, k, occ, x, y, q = kc.case(name)
    rmax = 8192 if dim == 2 else 512
    assert kc.unclamped_resolution(x, occ).max() > rmax
    assert kc.index_plan(x, occ)[2].max() == rmax
    L = x.max(0) - x.min(0)
    if name.startswith("clamp"):                                      # off the ends of the long axis, 100 x to the side
        assert (q[:, 0] < x[:, 0].min()).any() and (q[:, 0] > x[:, 0].max()).any()
        assert (np.abs(q[:, 1]) >= 99.0 * L[1]).any()


@pytest.mark.parametrize("name", kc.MARGIN_CASES)
def test_margin_cases_have_face_errors_above_the_margin(name):
    """ulp(|lo|) > 1e-9 h on the finest lattice the index would choose (|lo| / h > 4.5e6)"""
    _, dim, k, occ, x, y, q = kc.case(name)
    assert kc.margin_ratio(x, occ) > 1.0
    if name in kc.LATTICE_CASES:
        lo, h, res, _ = kc.index_plan(x, occ)
        assert np.abs(lo).max() / h.min() > 4.5e6
    else:
        assert len(kc.sub_plan(x, occ)[0]) > 0


@pytest.mark.parametrize("name", kc.FACE_CASES)
def test_face_cases_have_a_point_beyond_a_computed_face(name):
    """per planted pair, in the index's own arithmetic: x is assigned to bucket i though it lies below the face the search
    computes for it, fl(base + i * h); q and y are assigned to bucket i - 1; x is the nearest point (or ties with y and has the
    smaller id) and y is nearer than that face: pruning bucket i by its face returns y.  With the margin of 1e-9 bucket sides the
    bound is zero and the bucket is visited"""
    _, dim, k, occ, x, y, q = kc.case(name)
    lo, h, inv_h, res, occ_ = kc.index_grid(x, occ)
    assert k == 1 and (lo == 0).all()
    idx_o, dist_o = brute(name)
    kinds = set()
    for ix, iy, iq, axis, kind in kc.face_triplets(name):
        base, hh, inv = lo, h, inv_h
        cell = kc.top_cell(x[[ix, iy]], lo, inv_h, res)
        assert (cell == kc.top_cell(q[[iq]], lo, inv_h, res)).all() or kind == "top"
        if kind == "sub":
            cells, cnt, r = kc.sub_plan(x, occ)
            assert len(cells) == 1 and (cells[0] == cell[0]).all()
            base, hh, inv = lo + cells[0] * h, h / r[0], r[0] * inv_h          # sub_lattice, sub_cell_of
        def coord(p):
            return int((p[axis] - base[axis]) * inv[axis])
        i = coord(x[ix])
        face = base[axis] + i * hh[axis]
        assert x[ix, axis] < face and coord(x[iy]) == i - 1 == coord(q[iq])
        others = np.delete(np.arange(dim), axis)
        assert (np.abs(x[ix, others] - q[iq, others]) < 0.5 * hh[others]).all()       # same bucket along the other axes
        d = _rdist(x[[ix, iy]], q[[iq]])[0]
        gap = face - q[iq, axis]
        assert d[0] < d[1] or (d[0] == d[1] and ix < iy)
        assert d[1] < gap * gap and gap - 1e-9 * hh.min() < 0
        assert idx_o[iq, 0] == ix and np.partition(_rdist(x, q[[iq]])[0], 2)[2] > (0.5 * hh.min()) ** 2
        kinds.add((kind, bool(d[0] < d[1])))
    assert kinds >= ({("sub", False)} if "_sub_" in name else {("top", False), ("top", True)})


def test_wall_clouds_are_exact():
    """spacings 2^-6 .. 2^-20 along the wall normal, 2^-6 along the wall, and exact coordinates: ties are real"""
    for name in kc.WALL_BASE:
        _, dim, k, occ, x, y, q = kc.case(name)
        off = float(name.split("_o")[1].split("_")[0])
        assert np.array_equal((x - off) * 2.0 ** 20, np.round((x - off) * 2.0 ** 20))
        normal = np.unique(x[:, -1])
        assert set(np.diff(normal)) == {2.0 ** -p for p in range(6, 21)}
        assert set(np.diff(np.unique(x[:, 0]))) == {2.0 ** -6}
        assert x.min() == off and (q[:, -1] < off).any()


# ---- the judge -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", kc.NAMES)
def test_oracle_equals_numpy_restatement(name):
    _, dim, k, occ, x, y, q = kc.case(name)
    idx_o, dist_o = brute(name)
    idx_r, dist_r = restated_knn(x, _queries(name), k)
    assert np.array_equal(idx_o, idx_r), name
    assert np.array_equal(_bits(dist_o), _bits(dist_r)), name


@pytest.mark.parametrize("name", kc.NAMES)
def test_oracle_returns_a_true_nearest_set(name):
    """by exact (long double) distances the farthest returned neighbour is no farther than the nearest excluded point times
    1 + 12 * 2^-53: each float64 reduced distance carries at most (dim + 2) * 2^-53 relative error; two of them and the ratio
    give 10, rounded up to 12"""
    _, dim, k, occ, x, y, q = kc.case(name)
    q = _queries(name)[:SAMPLE]
    idx = brute(name)[0][:SAMPLE]
    for s in range(0, len(q), 32):
        rd = _rdist_exact(x, q[s:s + 32])
        rows = np.arange(len(rd))[:, None]
        far_in = rd[rows, idx[s:s + 32]].max(1)
        assert all(len(set(r)) == k for r in idx[s:s + 32])
        if k == len(x):
            continue
        rd[rows, idx[s:s + 32]] = np.inf
        assert (far_in <= rd.min(1) * (1 + np.longdouble(12) * EPS)).all(), name


@pytest.mark.parametrize("name", [n for n in kc.NAMES if not kc.flat(kc.case(n)[4])])
def test_grid_oracle_equals_brute_force(name):
    """s3o_grid_knn == s3o_knn where the cloud is not flat (child_metric_cases.flat).  On the clamp clouds, 10^4 and 10^6 times
    longer than wide, of the queries farther from the box than 200 x its shortest side only FAR_SAMPLE are kept (the farthest
    among them): the oracle's buckets are cubes of the mean density's size, and such a query walks every one of 15 000 and more
    rings (0.6 s each)"""
    _, dim, k, occ, x, y, q = kc.case(name)
    q = _queries(name)
    keep = np.ones(len(q), dtype=bool)
    if name in kc.CLAMP_CASES:
        lo, hi = x.min(0), x.max(0)
        gap = np.maximum(lo - q, q - hi).max(1)
        keep = gap <= 200.0 * (hi - lo).min()
        far = np.flatnonzero(~keep)
        assert keep.sum() >= 40 and len(far) >= FAR_SAMPLE
        keep[far[np.argsort(gap[far])[np.linspace(0, len(far) - 1, FAR_SAMPLE).astype(int)]]] = True
    grid = orc.GridIndex(x)
    try:
        idx_g, dist_g = grid.knn(q[keep], k)
        pred_g = grid.idw_predict(y, q[keep], k)
    finally:
        grid.close()
    idx_o, dist_o = brute(name)
    assert np.array_equal(idx_g, idx_o[keep]) and np.array_equal(_bits(dist_g), _bits(dist_o[keep]))
    assert np.array_equal(_bits(pred_g), _bits(orc.idw_predict(x, y, q[keep], k)))


def weights_exact(dist):
    d = np.maximum(dist.astype(np.longdouble), np.longdouble(1e-12))
    w = 1 / d
    return w / w.sum(1, keepdims=True)


def _check_weights(dist):
    k = dist.shape[1]
    w, ref = orc.idw_weights(dist), weights_exact(dist)
    assert np.isfinite(w).all()
    assert (np.abs(w - ref) <= (k + 2) * EPS * ref).all()


@pytest.mark.parametrize("name", kc.NAMES)
def test_oracle_weights_and_predictions_match_long_double(name):
    """weights (1 / max(d, 1e-12)) / sum within (k + 2) * 2^-53 relative; predictions (indicator weights where a distance is
    zero) within (k + 2) * 2^-53 * sum|y_m w_m| / sum w_m"""
    _, dim, k, occ, x, y, q = kc.case(name)
    idx, dist = brute(name)
    _check_weights(dist)
    pred = orc.idw_predict(x, y, _queries(name), k)
    d = dist.astype(np.longdouble)
    zero = (d == 0).any(1, keepdims=True)
    with np.errstate(divide="ignore"):
        w = np.where(zero, (d == 0).astype(np.longdouble), 1 / d)
    yw = y[idx].astype(np.longdouble) * w
    ref = yw.sum(1) / w.sum(1)
    assert (np.abs(pred - ref) <= (k + 2) * EPS * np.abs(yw).sum(1) / w.sum(1)).all(), name
    if name in kc.ZERO_CASES:
        pred_c = orc.idw_predict(x, kc.const_y(len(x)), _queries(name), k)
        assert zero.any() and (pred_c == 2.0 ** -3).all()       # (scaling by a power of two is exact in every sum)


@pytest.mark.parametrize("k", kc.WEIGHT_KS)
@pytest.mark.parametrize("nc", kc.WEIGHT_ROWS)
def test_oracle_weights_on_adversarial_rows(nc, k):
    dist = kc.adversarial_dist(nc, k)
    flat_ = dist.ravel()
    for v in kc.CLAMP_SPECIALS[:min(k * nc, len(kc.CLAMP_SPECIALS))]:
        assert (flat_ == v).any()
    if k >= len(kc.CLAMP_SPECIALS):
        assert ((dist < 1e-12).sum(1) >= 4).all()             # several clamped distances in every row
    _check_weights(dist)
