"""
The query path of the export's KNN cache (csrc/knn.hip: s3_knn_query, s3_idw_weights, s3_idw_predict, i.e. knn_query_kernel,
idw_weights_kernel and idw_predict_kernel on knn_search / ring_search and its sub-lattices) against the CPU oracle's brute force
(oracle/s3_oracle.c: s3o_knn, s3o_idw_weights, s3o_idw_predict), bit for bit, on the hostile cases of
tests/knn_query_cases.py.  GPU only.

Per case, on one KnnIndex:
  a. query(q, k): the neighbour ids equal brute force, the distances bit for bit;
  b. idw_weights(dist) equals the oracle's weights bit for bit;
  c. predict(q, k) after set_values(y) equals the oracle's prediction bit for bit (y of magnitudes 1e-8 .. 1e8: any change of
     the summation order changes bits); on the zero-distance cases also with a constant power of two, where every prediction
     is exactly that value;
  d. the same queries in another order, split into two calls whose lengths are no multiples of the workgroup, give the same
     rows;
  e. the index has what the case is about: refined buckets, an axis at the resolution clamp.
"""
import functools

import numpy as np
import pytest

from tests import knn_query_cases as kc

pytestmark = pytest.mark.gpu

KNN_BLOCK = 128              # csrc/knn.hip: queries per workgroup


@pytest.fixture(scope="module")
def ops():
    from sparsespatialsampling_amd import hipops
    hipops.device()
    return hipops


@pytest.fixture(scope="module")
def orc():
    from oracle import s3_oracle
    return s3_oracle


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _rows(what, name, got, ref, q, as_bits):
    """'' when got and ref are the same, else: case, the count of differing queries, the first three with their rows"""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return f"{name} {what}: shape {got.shape} != {ref.shape}"
    a, b = (_bits(got), _bits(ref)) if as_bits else (got, ref)
    bad = np.flatnonzero((a != b).reshape(len(a), -1).any(1))
    if len(bad) == 0:
        return ""
    msg = [f"{name} {what}: {len(bad)} of {len(a)} queries differ"]
    for i in bad[:3]:
        msg.append(f"  query {i} at {q[i]!r}:\n    gpu    {got[i]!r}\n    oracle {ref[i]!r}")
    return "\n".join(msg)


@functools.lru_cache(maxsize=None)
def reference(name):
    """brute force on the CPU, computed once per case: (idx, dist, prediction)"""
    from oracle import s3_oracle as o
    _, dim, k, occ, x, y, q = kc.case(name)
    idx, dist = o.knn(x, q, k)
    return idx, dist, o.idw_predict(x, y, q, k)


@pytest.mark.parametrize("name", kc.NAMES)
def test_query_path_equals_brute_force(ops, orc, name):
    _, dim, k, occ, x, y, q = kc.case(name)
    nq = len(q)
    idx_o, dist_o, pred_o = reference(name)
    knn = ops.KnnIndex(x, occ)
    bad = []
    try:
        # ---- e. the index ----------------------------------------------------------------------------------------------------
        lo, h, res, _ = kc.index_plan(x, occ)
        assert knn.n_buckets == int(np.prod(res)), (name, knn.n_buckets, res)
        if name in kc.CLAMP_CASES:
            assert res.max() == (8192 if dim == 2 else 512) and knn.n_buckets % res.max() == 0
        if name in kc.REFINED_CASES:
            assert knn.n_refined_buckets > 0, name
        # ---- a. neighbours -----------------------------------------------------------------------------------------------------
        d_q = ops.to_device(q)
        idx, dist = knn.query(d_q, k)
        idx_h, dist_h = ops.to_host(idx), ops.to_host(dist)
        bad.append(_rows("idx", name, idx_h.astype(np.int64), idx_o, q, False))
        bad.append(_rows("dist", name, dist_h, dist_o, q, True))
        # ---- b. weights --------------------------------------------------------------------------------------------------------
        bad.append(_rows("idw_weights", name, ops.to_host(ops.idw_weights(dist)), orc.idw_weights(dist_h), q, True))
        # ---- c. predictions ----------------------------------------------------------------------------------------------------
        knn.set_values(y)
        pred = ops.to_host(knn.predict(d_q, k))
        bad.append(_rows("predict", name, pred, pred_o, q, True))
        # ---- d. another order, two calls -----------------------------------------------------------------------------------------
        perm = np.random.default_rng(nq).permutation(nq)
        cut = min(nq - 1, nq // 2 + 1)
        if cut % KNN_BLOCK == 0 or (nq - cut) % KNN_BLOCK == 0:
            cut -= 1
        parts = [perm[:cut], perm[cut:]]
        assert all(len(p) % KNN_BLOCK for p in parts) or nq <= 2
        got = [knn.query(ops.to_device(q[p]), k) for p in parts]
        idx2 = np.concatenate([ops.to_host(g[0]) for g in got])
        dist2 = np.concatenate([ops.to_host(g[1]) for g in got])
        pred2 = np.concatenate([ops.to_host(knn.predict(ops.to_device(q[p]), k)) for p in parts])
        bad.append(_rows("idx, permuted and split", name, idx2, idx_h[perm], q[perm], False))
        bad.append(_rows("dist, permuted and split", name, dist2, dist_h[perm], q[perm], True))
        bad.append(_rows("predict, permuted and split", name, pred2, pred[perm], q[perm], True))
        if name in kc.ZERO_CASES:
            assert (dist_o[:, 0] == 0.0).any()
            knn.set_values(kc.const_y(len(x)))
            pred_c = ops.to_host(knn.predict(d_q, k))
            bad.append(_rows("predict of a constant", name, pred_c, np.full(nq, 2.0 ** -3), q, True))
    finally:
        knn.close()
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("k", kc.WEIGHT_KS)
@pytest.mark.parametrize("nc", kc.WEIGHT_ROWS)
def test_idw_weights_on_adversarial_rows(ops, orc, nc, k):
    """distances of exactly 0, 1e-12, the double just below it, a denormal and 1e-300, several in one row, at the lengths where
    torch_inner_sum changes its lane pattern and around one workgroup of rows"""
    dist = kc.adversarial_dist(nc, k)
    w = ops.to_host(ops.idw_weights(ops.to_device(dist)))
    bad = _rows("idw_weights", f"nc={nc} k={k}", w, orc.idw_weights(dist), dist, True)
    assert not bad, bad
