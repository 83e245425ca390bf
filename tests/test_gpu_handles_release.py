"""KnnIndex and InterpPlan give their device memory back: handles created, used and closed in a loop -- with the calls the
library refuses mixed in -- leave the free device memory (hipMemGetInfo, which sees the library's own allocations) where it was.

Modelled on test_gpu_topology.py::test_device_engine_releases_its_memory: 12 rounds, the baseline taken after the second (the
first also loads code objects and creates pools), the same 8 MiB bound.  A live handle of a round owns between 6 and 15 MB (the
k = 5 plan: 1.5 MB), so a handle that is not released shows as tens of MiB over the ten rounds after the baseline.  The loss of
a single small buffer (`perm`: 80 KB a round) stays below the bound and is NOT seen here: that is covered by
tests/native/dev_buf_test.cpp (every way an owner can go out of scope, on a counting allocator) and by the library freeing no
buffer by name (csrc/dev_buf.h owns them all)."""
import numpy as np
import pytest
import torch as pt

pytestmark = pytest.mark.gpu

ROUNDS, BOUND = 12, 8 << 20
N_SRC, N_TGT, K = 200_000, 20_000, 26          # the cloud of tools/leak_probe.py


@pytest.fixture(scope="module")
def ops():
    from sparsespatialsampling_amd import hipops
    hipops.device()
    return hipops


@pytest.fixture(scope="module")
def cloud(ops):
    """device tensors shared by the tests of this module (made once, never modified)"""
    rng = np.random.default_rng(0)
    x, y, c = rng.random((N_SRC, 3)), rng.random(N_SRC), rng.random((N_TGT, 3))
    graded = x.copy()
    graded[: N_SRC // 2, 0] *= 1e-3              # half of the points in 1e-3 of one axis: buckets that get a sub-lattice
    x_inf = x.copy()
    x_inf[123, 1] = np.inf
    dev = lambda a, dt=pt.float64: pt.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)
    d = dict(x=dev(x), y=dev(y), c=dev(c), graded=dev(graded), x_inf=dev(x_inf))
    knn = ops.KnnIndex(d["x"])
    d["idx"], dist = knn.query(d["c"], K)
    d["w"] = ops.idw_weights(dist)
    knn.close()
    d["idx5"], d["w5"] = d["idx"][:, :5].contiguous(), d["w"][:, :5].contiguous()
    d["table"] = pt.from_numpy(rng.standard_normal((N_SRC, 16)).astype(np.float32)).cuda()      # 16 fp32 snapshots, 64-byte rows
    d["ids"] = pt.arange(N_SRC, dtype=pt.int32, device="cuda")
    d["ids_bad"] = d["ids"].clone()
    d["ids_bad"][int(d["idx"][0, 0])] = N_SRC    # a row the plan references, sent to row n_table
    d["idx_bad"] = pt.full((4, 8), N_SRC, dtype=pt.int32, device="cuda")
    pt.cuda.synchronize()
    return d


def _free():
    pt.cuda.synchronize()
    pt.cuda.empty_cache()
    return pt.cuda.mem_get_info()[0]


def _held_after(rounds_of, what):
    """free memory after the last round against the free memory after the second"""
    free_before = None
    for it in range(ROUNDS):
        rounds_of(it)
        if it == 1:
            free_before = _free()
    diff = free_before - _free()
    print(f"{what}: {diff / 2**20:+.2f} MiB held after {ROUNDS - 2} rounds (bound {BOUND >> 20} MiB)")
    return abs(diff)


@pytest.mark.parametrize("which", ["x", "graded"])
def test_knn_index_releases_its_memory(ops, cloud, which):
    """create / set_values / query at k = 26 / close, on the uniform cloud and on a graded one (second-level tables); once per
    round a cloud with an infinite coordinate, refused after the bounding-box pass"""
    from sparsespatialsampling_amd._lib import S3HipError

    def one_round(it):
        knn = ops.KnnIndex(cloud[which])
        assert (knn.n_refined_buckets > 0) == (which == "graded")
        knn.set_values(cloud["y"])
        idx, dist = knn.query(cloud["c"], K)
        assert idx.shape == (N_TGT, K) and bool(pt.isfinite(dist).all())
        knn.close()
        with pytest.raises(S3HipError):
            ops.KnnIndex(cloud["x_inf"])

    assert _held_after(one_round, f"KnnIndex[{which}]") <= BOUND, "device memory of closed KNN indices is not released"


def test_interp_plan_releases_its_memory(ops, cloud):
    """a k = 26 plan (tile schedule, lane tables, weights, source ids, interp + interp_src of 16 fp32 snapshots) and a k = 5 plan
    (no schedule; interp) per round, with a refused table (index n_src) and a refused set_source_ids (an id equal to n_table),
    after which the plan still interpolates"""
    from sparsespatialsampling_amd._lib import S3HipError
    table, w = cloud["table"], cloud["w"]

    def one_round(it):
        plan = ops.InterpPlan(cloud["idx"], N_SRC, cloud["c"])
        plan.set_weights(w)
        with pytest.raises(S3HipError):
            plan.set_source_ids(cloud["ids_bad"], N_SRC)
        out = plan.interp(w, table)
        assert out.shape == (N_TGT, 16) and bool(pt.isfinite(out).all())
        plan.set_source_ids(cloud["ids"], N_SRC)
        assert pt.equal(plan.interp_src(table), out)
        plan.close()
        with pytest.raises(S3HipError):
            ops.InterpPlan(cloud["idx_bad"], N_SRC)
        plan5 = ops.InterpPlan(cloud["idx5"], N_SRC)
        out5 = plan5.interp(cloud["w5"], table)
        assert out5.shape == (N_TGT, 16) and bool(pt.isfinite(out5).all())
        plan5.close()

    assert _held_after(one_round, "InterpPlan") <= BOUND, "device memory of closed interpolation plans is not released"
