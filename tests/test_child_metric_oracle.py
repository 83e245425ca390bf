"""
The reference of tests/test_gpu_child_metric.py and the cases it runs, on the CPU: the oracle's bucket-grid child gain equals
its brute-force one, both equal an independent numpy / torch restatement of the reference's arithmetic, and each case still
has the property it exists for (zero distances, a tie group across the k-th neighbour, cells outside the cloud).
"""
import numpy as np
import pytest
import torch as pt

from oracle import s3_oracle as orc
from tests import child_metric_cases as cmc

SAMPLE = 150                 # cells per batch and generation checked here (the GPU test checks them all)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _sample(n, seed):
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(n, min(n, SAMPLE), replace=False))


def _generations(name):
    """(centres, levels, width) of a sample of each batch's root cells and of its children"""
    _, dim, *_, batches = cmc.case(name)
    out = []
    for b in batches:
        pick = _sample(len(b.centers), 1)
        out.append((b.centers[pick], b.level[pick], b.width))
        _, ch_c, ch_l = cmc.children(b, dim)
        pick = _sample(len(ch_c), 2)
        out.append((ch_c[pick], ch_l[pick], b.width))
    return out


def _queries(centers, level, width):
    """the 2^d + 1 points of each cell (centre first), as the oracle forms them"""
    dim = centers.shape[1]
    return np.concatenate([centers[:, None, :], cmc.child_points(centers, level, width)], 1).reshape(-1, dim)


def _rdist(x, q):
    """squared distances summed in dimension order, [len(q), len(x)]"""
    d = np.zeros((len(q), len(x)))
    for j in range(x.shape[1]):
        t = q[:, j:j + 1] - x[None, :, j]
        d += t * t
    return d


def _predict(y, rd_sel, idx):
    """sklearn's "distance" weights (a row with a zero distance: indicator weights) and the weighted mean by numpy's own
    pairwise sum over the rows of C-contiguous [n, k] arrays"""
    dist = np.sqrt(rd_sel)
    with np.errstate(divide="ignore"):
        w = 1.0 / dist
    zero = (dist == 0.0).any(axis=1)
    w[zero] = (dist[zero] == 0.0).astype(np.float64)
    yw = np.ascontiguousarray(y[idx] * w)
    return yw.sum(axis=1) / np.ascontiguousarray(w).sum(axis=1)


def restated_child_gain(x, y, k, centers, level, width, gain0, chunk=64):
    """the reference's child gain from numpy and torch alone: neighbours by np.lexsort((ids, rdist)), sklearn's weights,
    numpy's pairwise predictions, torch's CPU sum of |m0 - mj|, gain = level_factor * sum / gain0"""
    dim = centers.shape[1]
    nq = 2 ** dim + 1
    q = _queries(centers, level, width)
    ids = np.arange(len(x))
    pred = np.empty(len(q))
    for s in range(0, len(q), chunk):
        rd = _rdist(x, q[s:s + chunk])
        order = np.lexsort((np.broadcast_to(ids, rd.shape), rd), axis=-1)[:, :k]
        pred[s:s + chunk] = _predict(y, np.take_along_axis(rd, order, 1), order)
    m = pred.reshape(-1, nq)
    sd = pt.sum(pt.abs(pt.from_numpy(m[:, :1]) - pt.from_numpy(np.ascontiguousarray(m[:, 1:]))), dim=1).numpy()
    lf = orc.level_factor_table(width, dim)
    return m, lf[level] * sd / gain0


@pytest.mark.parametrize("name", [n for n in cmc.NAMES if not cmc.flat(cmc.case(n)[4])])
def test_grid_oracle_equals_brute_force(name):
    """s3o_grid_child_gain (the GPU test's reference above BRUTE_MAX_POINTS points, flat clouds aside) == s3o_child_gain, bit
    for bit"""
    _, dim, k, _, x, y, _ = cmc.case(name)
    grid = orc.GridIndex(x)
    try:
        for centers, level, width in _generations(name):
            m_b, g_b = orc.child_gain(x, y, k, centers, level, width, cmc.GAIN0)
            m_g, g_g = grid.child_gain(y, k, centers, level, width, cmc.GAIN0)
            assert np.array_equal(_bits(m_g), _bits(m_b)) and np.array_equal(_bits(g_g), _bits(g_b))
    finally:
        grid.close()


SMALL = [n for n in cmc.NAMES if len(cmc.case(n)[4]) <= 70_000]


@pytest.mark.parametrize("name", SMALL)
def test_oracle_equals_numpy_torch_restatement(name):
    _, dim, k, _, x, y, _ = cmc.case(name)
    for centers, level, width in _generations(name):
        c, lv = centers[:40], level[:40]
        m_r, g_r = restated_child_gain(x, y, k, c, lv, width, cmc.GAIN0)
        m_o, g_o = orc.child_gain(x, y, k, c, lv, width, cmc.GAIN0)
        assert np.array_equal(_bits(m_o), _bits(m_r)), name
        assert np.array_equal(_bits(g_o), _bits(g_r)), name
        if len(y) > 1 and np.all(y == y[0]):               # (const_y: a power of two)
            assert np.all(g_o == 0.0)


def _tie_changes_answer(x, y, k, q):
    """some query whose tie group at the k-th neighbour crosses it, where taking the larger ids changes the prediction"""
    if k >= len(x):
        return False
    for s in range(0, len(q), 64):
        rd = _rdist(x, q[s:s + 64])
        kth = np.partition(rd, k - 1, axis=1)[:, k - 1:k]
        below, eq = rd < kth, rd == kth
        cross = below.sum(1) + eq.sum(1) > k
        for r in np.flatnonzero(cross):
            need = k - below[r].sum()
            group = np.flatnonzero(eq[r])
            sel = [np.r_[np.flatnonzero(below[r]), group[:need]], np.r_[np.flatnonzero(below[r]), group[::-1][:need]]]
            p = [_predict(y, rd[r, s_][None], s_[None])[0] for s_ in sel]
            if _bits(p[0]) != _bits(p[1]):
                return True
    return False


@pytest.mark.parametrize("name", cmc.TIE_CASES)
def test_tie_cases_straddle_the_kth_neighbour(name):
    _, dim, k, _, x, y, _ = cmc.case(name)
    for centers, level, width in _generations(name):
        if _tie_changes_answer(x, y, k, _queries(centers[:60], level[:60], width)):
            return
    pytest.fail(f"{name}: no tie group across the k-th neighbour that matters")


@pytest.mark.parametrize("name", cmc.ZERO_CASES)
def test_zero_distance_cases_hit_points(name):
    """query points (centres, child points) that coincide with data points"""
    _, dim, k, _, x, y, _ = cmc.case(name)
    grid = orc.GridIndex(x)
    try:
        hits = [int((grid.knn(_queries(c, lv, w), 1)[1] == 0.0).sum()) for c, lv, w in _generations(name)]
    finally:
        grid.close()
    assert sum(hits) > 0, name


@pytest.mark.parametrize("name", cmc.OUTSIDE_CASES)
def test_outside_cases_are_outside(name):
    _, dim, k, _, x, y, batches = cmc.case(name)
    lo, hi = x.min(0), x.max(0)
    for b in batches:
        gap = np.maximum(lo - b.centers, b.centers - hi).max(1)
        assert (gap > 0).all()
        assert (gap > 2 * (hi - lo).max()).any()
