"""
The reconstruction error on the GPU (csrc/recon.hip, sparsespatialsampling_amd/reconstruction.py): scikit-learn's exact distance
weights, the fused gather / subtract / reduce launch against a long-double reference (tests/recon_cases.py), and the public
``ReconstructionError`` / ``reconstruct`` end to end against scikit-learn's own prediction (tests/golden/recon_sklearn.npz).

Bound of every comparison: 1e-12 relative to the largest value of the output compared -- the contract metrics.py states for its
moments.  (What the arithmetic gives: an f64 fma chain over k <= 26 neighbours is within 28 * 2**-53 = 3e-15 of the exact sum of
magnitudes; the sums over 3001 points or 100 columns of non-negative terms add at most 3001 * 2**-53 = 3.4e-13 in the worst case
and ~sqrt(3001) * 2**-53 = 6e-15 as rounding errors go; 1e-12 is the worst case with room for the square roots and the
cancellation in fit - orig, which is measured against the output's maximum, not against the element.)

Shapes: 3001 points on 257 cells -- three reduction blocks of 1024 points, the last one ragged.
"""
import itertools

import numpy as np
import pytest
import torch as pt

from tests import recon_cases as rc
from sparsespatialsampling_amd import hipops
from sparsespatialsampling_amd.reconstruction import ReconstructionError, reconstruct

pytestmark = pytest.mark.gpu

TOL = 1e-12


def dev(a):
    return pt.from_numpy(np.ascontiguousarray(a)).cuda()


def check(name, got, ref, what):
    err = rc.rel_err(got.cpu().numpy() if isinstance(got, pt.Tensor) else got, ref)
    print(f"{what}: {name} off the reference by {err:.2e} of its maximum")
    assert err <= TOL, f"{what}: {name} off the reference by {err:.3e} of its maximum (bound {TOL})"


# ---- weights --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 8, 26])
def test_exact_weights(k):
    rng = np.random.default_rng(k)
    dist = np.sort(rng.random((rc.N_POINTS, k)) + 1e-3, axis=1)
    dist[::3, 0] = 0.0                      # one zero distance
    dist[::7, :2] = 0.0                     # two (and rows 0, 21, ... of both kinds)
    ref = rc.exact_weights(dist)
    w = hipops.idw_weights_exact(dev(dist)).cpu().numpy()
    zeros = (dist == 0.0).sum(axis=1)
    assert set(np.unique(zeros)) == {0, 1, 2}
    for nz in (0, 1, 2):
        err = np.abs(w[zeros == nz] - ref[zeros == nz]).max()
        print(f"k {k}, rows with {nz} zero distances: {err:.2e} off numpy")
        assert err <= 1e-15
    assert np.array_equal(w[zeros == 1][:, 0], np.ones((zeros == 1).sum())) and not w[zeros == 1][:, 1:].any()
    assert np.array_equal(w[zeros == 2][:, :2], np.full(((zeros == 2).sum(), 2), 0.5)) and not w[zeros == 2][:, 2:].any()
    assert np.abs(w.astype(rc.LD).sum(axis=1) - 1).max() <= 1e-15


# ---- the fused launch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_len", [1, 6, 7, 25, 64, 100])
@pytest.mark.parametrize("k", [5, 8, 26])
def test_fused_against_long_double(k, row_len):
    """every combination of grid f32 / f64, original f32 / f64, scale given / absent, row permutation given / absent and dense /
    pitched original rows (pitch row_len + 3: rows that start off every vector boundary)"""
    n = rc.N_POINTS
    perm = np.random.default_rng(99).permutation(n).astype(np.int32)
    for grid_f64, orig_f64 in itertools.product((False, True), repeat=2):
        case = rc.table_case(k, row_len, grid_f64, orig_f64, seed=1000 * k + row_len)
        fit = rc.fitted(case["w"], case["idx"], case["grid"])
        grid_d = dev(case["grid"])
        dense = dev(case["orig"])
        wide = pt.full((n, row_len + 3), float("nan"), dtype=dense.dtype, device="cuda")
        wide[:, :row_len] = dense
        for with_scale, with_rows, pitched in itertools.product((False, True), repeat=3):
            what = (f"k {k} row_len {row_len} grid {'f64' if grid_f64 else 'f32'} orig {'f64' if orig_f64 else 'f32'} "
                    f"scale {with_scale} rows {with_rows} pitched {pitched}")
            scale = case["scale"] if with_scale else None
            ref = rc.moments(fit, case["orig"], scale)
            order = perm if with_rows else np.arange(n)
            mean, m2, colsum = hipops.recon_error(
                dev(case["w"][order]), dev(case["idx"][order]), grid_d, wide[:, :row_len] if pitched else dense,
                rows=dev(perm) if with_rows else None, scale=dev(scale[order]) if with_scale else None)
            for name, got, want in zip(("mean", "m2", "sum d^2", "sum ref^2"), (mean, m2, colsum[0], colsum[1]), ref):
                check(name, got, want, what)


def test_fused_long_rows_take_several_chunks():
    """rows longer than one sweep of a point's lanes (64 lanes x 4 f32 / x 2 f64 / x 1 ragged): the per-point moments are merged
    across chunks"""
    for row_len, grid_f64 in ((300, False), (260, True), (131, False)):
        case = rc.table_case(8, row_len, grid_f64, False, seed=row_len, n=1500)
        ref = rc.moments(rc.fitted(case["w"], case["idx"], case["grid"]), case["orig"], case["scale"])
        mean, m2, colsum = hipops.recon_error(dev(case["w"]), dev(case["idx"]), dev(case["grid"]), dev(case["orig"]),
                                              scale=dev(case["scale"]))
        for name, got, want in zip(("mean", "m2", "sum d^2", "sum ref^2"), (mean, m2, colsum[0], colsum[1]), ref):
            check(name, got, want, f"row_len {row_len} grid f64 {grid_f64}")


def test_fused_rejects_bad_arguments():
    case = rc.table_case(8, 6, False, False, seed=3, n=100)
    w, idx, grid, orig = dev(case["w"]), dev(case["idx"]), dev(case["grid"]), dev(case["orig"])
    with pytest.raises(TypeError):
        hipops.recon_error(w, idx.to(pt.int64), grid, orig)
    with pytest.raises(TypeError):
        hipops.recon_error(w, idx, grid, orig[:, :5])
    with pytest.raises(TypeError):
        hipops.recon_error(w, idx, grid, orig[:50])
    with pytest.raises(hipops._lib.S3HipError):
        hipops.recon_error(pt.ones(100, 65, dtype=pt.float64, device="cuda"), pt.zeros(100, 65, dtype=pt.int32, device="cuda"),
                           grid, orig)


# ---- exactness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_points_on_centres_have_exactly_zero_error(dim):
    """every point is a copy of a cell centre and the original equals the grid's value there: all four numerators are exactly
    0.0 -- with the export's clamp rule each of them is not"""
    rng = np.random.default_rng(dim)
    c = rng.random((rc.N_CELLS, dim))
    cell = np.arange(rc.N_POINTS) % rc.N_CELLS
    grid = (rng.standard_normal((rc.N_CELLS, 25)) + 2.0).astype(np.float32)
    x, orig = c[cell], grid[cell]
    err = ReconstructionError(dev(c), dev(x), point_scale=dev(np.sqrt(rng.random(rc.N_POINTS) + 0.1))).update(dev(grid), dev(orig))
    assert not err.error_time.cpu().numpy().any() and err.error_total == 0.0
    assert not err.error_space_mean.cpu().numpy().any() and not err.error_space_std.cpu().numpy().any()
    # the clamp rule on the same table
    knn = hipops.KnnIndex(dev(c))
    idx, dist = knn.query(dev(x), err.n_neighbors)
    knn.close()
    assert not dist[:, 0].cpu().numpy().any()
    mean, _, colsum = hipops.recon_error(hipops.idw_weights(dist), idx, dev(grid), dev(orig))
    assert colsum[0].cpu().numpy().all() and mean.cpu().numpy().any()


# ---- end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 1])
def test_end_to_end_matches_sklearn(case):
    """device KNN -> exact weights -> fused launch, against the statistics of scikit-learn's stored prediction"""
    g = rc.fixture()
    c, x, f, o, s = (g[f"{name}{case}"] for name in ("centers", "points", "grid", "orig", "scale"))
    ref = rc.statistics(g[f"pred{case}"], o, s)
    err = ReconstructionError(dev(c), dev(x), point_scale=dev(s)).update(dev(f), dev(o))
    assert err.n_neighbors == int(g[f"k{case}"]) and err.n_snapshots == o.shape[1]
    got = (err.error_time, np.array(err.error_total), err.error_space_mean, err.error_space_std)
    for name, a, b in zip(("error_time", "error_total", "error_space_mean", "error_space_std"), got, ref):
        check(name, a, b, f"fixture case {case}")
    # the fitted field itself
    check("reconstruct", reconstruct(dev(c), dev(f), dev(x)), g[f"pred{case}"], f"fixture case {case}")


@pytest.fixture(scope="module")
def cloud():
    """a 2-D cloud with 25 snapshots (f32, as a Dataloader yields them) and the statistics torch computes from the fitted field"""
    c, x = rc.cloud_case(2, seed=7)
    rng = np.random.default_rng(8)
    f = (rng.standard_normal((rc.N_CELLS, 25)) + 2.0).astype(np.float32)
    o = (rng.standard_normal((rc.N_POINTS, 25)) + 2.0).astype(np.float32)
    s = np.sqrt(rng.random(rc.N_POINTS) + 0.1)
    fit = reconstruct(dev(c), dev(f), dev(x))
    d = dev(s)[:, None] * (fit - dev(o).double())
    ref = dev(s)[:, None] * dev(o).double()
    stats = (pt.linalg.norm(d, ord=2, dim=0) / pt.linalg.norm(ref, ord=2, dim=0), pt.linalg.norm(d) / pt.linalg.norm(ref),
             d.abs().mean(dim=1), d.abs().std(dim=1))
    return dict(c=c, x=x, f=f, o=o, s=s, torch=tuple(v.cpu().numpy() for v in stats))


def results(err):
    return (err.error_time, np.array(err.error_total), err.error_space_mean, err.error_space_std)


NAMES = ("error_time", "error_total", "error_space_mean", "error_space_std")


BATCHINGS = {"25x1": [1] * 25, "8+8+9": [8, 8, 9], "1x25": [25]}


@pytest.fixture(scope="module")
def batched(cloud):
    """the same 25 snapshots fed in three ways -> {name: the four results as numpy arrays}"""
    out = {}
    for name, batches in BATCHINGS.items():
        err = ReconstructionError(dev(cloud["c"]), dev(cloud["x"]), point_scale=dev(cloud["s"]))
        t0 = 0
        for n_b in batches:
            err.update(dev(cloud["f"][:, t0:t0 + n_b]), dev(cloud["o"][:, t0:t0 + n_b]))
            t0 += n_b
        assert err.n_snapshots == 25
        out[name] = [np.asarray(v.cpu().numpy() if isinstance(v, pt.Tensor) else v) for v in results(err)]
    return out


@pytest.mark.parametrize("batching", list(BATCHINGS))
def test_batches_agree_with_torch_on_the_unfused_field(cloud, batched, batching):
    for name, a, b in zip(NAMES, batched[batching], cloud["torch"]):
        check(name, a, b, f"batches {batching}")


@pytest.mark.parametrize("pair", [("25x1", "8+8+9"), ("25x1", "1x25"), ("8+8+9", "1x25")], ids="-".join)
def test_batchings_agree_with_one_another(batched, pair):
    for name, a, b in zip(NAMES, batched[pair[0]], batched[pair[1]]):
        check(name, a, b, f"batches {pair[0]} against {pair[1]}")


def test_window_of_a_resident_field_is_read_where_it_lies(cloud):
    """``orig[:, t0:t1]`` of a [N, T] device field reaches the kernel as a pitched view (no copy of N x T_b values) and gives
    the bits of the contiguous copy"""
    from sparsespatialsampling_amd import arrays
    c, x, f, o = dev(cloud["c"]), dev(cloud["x"]), dev(cloud["f"]), dev(cloud["o"])
    window = o[:, 3:12]
    assert not window.is_contiguous() and arrays.resident(window).data_ptr() == window.data_ptr()
    lies = ReconstructionError(c, x, point_scale=dev(cloud["s"])).update(f[:, 3:12], window)
    copy = ReconstructionError(c, x, point_scale=dev(cloud["s"])).update(f[:, 3:12].contiguous(), window.contiguous())
    for a, b in zip(results(lies), results(copy)):
        assert np.array_equal(np.asarray(a.cpu().numpy() if isinstance(a, pt.Tensor) else a).view(np.int64),
                              np.asarray(b.cpu().numpy() if isinstance(b, pt.Tensor) else b).view(np.int64))


def test_vector_field(cloud):
    """n_comp = 3: the components of a snapshot are summed into its norm, a point's moments run over its 3 * T values"""
    rng = np.random.default_rng(9)
    f = (rng.standard_normal((rc.N_CELLS, 3, 7)) + 2.0).astype(np.float32)
    o = rng.standard_normal((rc.N_POINTS, 3, 7)) + 2.0
    idx, dist = rc.knn_brute(cloud["c"], cloud["x"], 8)
    ref = rc.statistics(rc.fitted(rc.exact_weights(dist), idx, f), o, cloud["s"])
    whole = ReconstructionError(dev(cloud["c"]), dev(cloud["x"]), point_scale=dev(cloud["s"])).update(dev(f), dev(o))
    split = ReconstructionError(dev(cloud["c"]), dev(cloud["x"]), point_scale=dev(cloud["s"]))
    split.update(dev(f[:, :, :3]), dev(o[:, :, :3])).update(dev(f[:, :, 3:]), dev(o[:, :, 3:]))
    assert whole.error_time.shape == (7,) and whole.error_space_mean.shape == (rc.N_POINTS,)
    for err, what in ((whole, "n_comp 3"), (split, "n_comp 3 in two batches")):
        for name, a, b in zip(NAMES, results(err), ref):
            check(name, a, b, what)


def test_host_in_host_out(cloud):
    c, x, f, o, s = (pt.from_numpy(cloud[name]) for name in "cxfos")
    err = ReconstructionError(c, x, point_scale=s).update(f, o)
    for name, a, b in zip(NAMES, results(err), cloud["torch"]):
        assert not (isinstance(a, pt.Tensor) and a.is_cuda), name
        check(name, a, b, "host tensors")
    fit = reconstruct(c, f, x)
    assert not fit.is_cuda and fit.dtype == pt.float64 and tuple(fit.shape) == (rc.N_POINTS, 25)
    # numpy arrays are taken like host tensors
    err_np = ReconstructionError(cloud["c"], cloud["x"], point_scale=cloud["s"]).update(cloud["f"], cloud["o"])
    assert pt.equal(err_np.error_space_std, err.error_space_std) and not err_np.error_time.is_cuda


def test_device_in_device_out(cloud):
    err = ReconstructionError(dev(cloud["c"]), dev(cloud["x"])).update(dev(cloud["f"]), dev(cloud["o"]))
    assert err.error_time.is_cuda and err.error_space_mean.is_cuda and err.error_space_std.is_cuda
    assert isinstance(err.error_total, float)


def test_two_runs_give_the_same_bits(cloud):
    def run():
        err = ReconstructionError(dev(cloud["c"]), dev(cloud["x"]), point_scale=dev(cloud["s"]))
        for t0, t1 in ((0, 8), (8, 16), (16, 25)):
            err.update(dev(cloud["f"][:, t0:t1]), dev(cloud["o"][:, t0:t1]))
        return [np.asarray(v.cpu().numpy() if isinstance(v, pt.Tensor) else v).view(np.int64) for v in results(err)]
    for a, b in zip(run(), run()):
        assert np.array_equal(a, b)


def test_zero_reference_divides_as_torch():
    c, x = rc.cloud_case(2, seed=11, n=300, nc=40)
    f, o = np.ones((40, 3), dtype=np.float32), np.zeros((300, 3), dtype=np.float32)
    o[:, 1] = 1.0
    err = ReconstructionError(dev(c), dev(x)).update(dev(f), dev(o))
    e_t = err.error_time.cpu().numpy()
    assert np.isinf(e_t[0]) and e_t[1] <= 1e-15 and np.isinf(e_t[2])
    zero = ReconstructionError(dev(c), dev(x)).update(dev(0 * f), dev(0 * o))
    assert np.isnan(zero.error_time.cpu().numpy()).all() and np.isnan(zero.error_total)


def test_neighbours_are_capped_at_the_grid():
    c, x = rc.cloud_case(3, seed=12, n=200, nc=11)
    f = np.random.default_rng(13).standard_normal((11, 4))
    err = ReconstructionError(dev(c), dev(x))
    assert err.n_neighbors == 11
    idx, dist = rc.knn_brute(c, x, 11)
    check("reconstruct", reconstruct(dev(c), dev(f), dev(x)), rc.fitted(rc.exact_weights(dist), idx, f), "k capped at Nc")


def test_value_errors(cloud):
    c, x, f, o = dev(cloud["c"]), dev(cloud["x"]), dev(cloud["f"]), dev(cloud["o"])
    err = ReconstructionError(c, x)
    for grid_fields, orig_fields in ((f[:, 0], o[:, 0]),                    # rank < 2
                                    (f[:-1], o), (f, o[:-1]),              # Nc / N do not match
                                    (f[:, :5], o[:, :6]),                  # trailing shapes differ
                                    (f.reshape(-1, 5, 5), o),              # (n_comp, T) against (T,)
                                    (f.reshape(-1, 5, 5), o.reshape(-1, 25, 1))):
        with pytest.raises(ValueError):
            err.update(grid_fields, orig_fields)
    with pytest.raises(ValueError):
        ReconstructionError(c, dev(np.random.default_rng(0).random((50, 3))))
    with pytest.raises(ValueError):
        ReconstructionError(c, x, point_scale=dev(cloud["s"][:-1]))
    err.update(f.reshape(-1, 5, 5), o.reshape(-1, 5, 5))
    with pytest.raises(ValueError):
        err.update(f, o)                                                    # a later batch with another component shape
    with pytest.raises(RuntimeError):
        ReconstructionError(c, x).error_time
