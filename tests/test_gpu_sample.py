"""
Cell index, point location and sampling on the GPU (csrc/sample.hip, sparsespatialsampling_amd/sampling.py) against the references
of tests/sample_cases.py.

What is asserted (no figure comes from the code under test):
  locate        ids EQUAL the long-double brute force on every case, with and without a row list; hostile coordinates give -1.
  build         the four refusals raise ``ValueError``; the lattice equals the float64 evaluation of the definition bit for bit.
  cell mode     the output equals ``field[ids].astype(float64)`` bit for bit, misses are all-NaN rows, nothing outside the output
                is written (guard zones on both sides).
  linear mode   per element ``(2^d + 3) * 2^-53 * sum_m |w_m f_m|`` from the long-double value: at most d roundings in a weight
                (one per axis) and an fma chain of 2^d terms; the same for a field that is affine in x at the nodes, whose blend
                must also be the affine function itself within ``sample_cases.affine_bound``.

Shapes: 3001 queries -- twelve workgroups of 256 launch positions, the last one ragged; T = 1 .. 300 covers one lane group of every
width (4 .. 64 lanes), vector and element loads, and rows of several chunks.
"""
import numpy as np
import pytest
import torch as pt

from tests import sample_cases as sc
from tests.interp_accuracy import GUARD_BITS, assert_guard
from sparsespatialsampling_amd import hipops, sampling
from sparsespatialsampling_amd.sampling import Probe

pytestmark = pytest.mark.gpu

LD = sc.LD
GUARD = 512
NQ = sc.NQ
PERM = np.random.default_rng(99).permutation(NQ).astype(np.int32)
_INDEX = {}


def dev(a):
    return pt.from_numpy(np.ascontiguousarray(a)).cuda()


def index_of(name):
    if name not in _INDEX:
        c = sc.case(name)
        _INDEX[name] = hipops.cell_index(dev(c["centers"]), dev(c["levels"]), c["width"])
    return _INDEX[name]


def run(ids, field, mode, rows=None, **linear):
    """``hipops.cell_sample`` into an allocation with guard zones on both sides -> numpy [nq, n_comp, T]"""
    n_comp = int(field.shape[1]) if field.dim() == 3 else 1
    t = int(field.shape[-1]) if field.dim() > 1 else 1
    numel = int(ids.numel()) * n_comp * t
    buf = pt.full((GUARD + numel + GUARD,), int(GUARD_BITS), dtype=pt.int64, device="cuda")
    out = buf.view(pt.float64)[GUARD:GUARD + numel]
    res = hipops.cell_sample(ids, field, mode, rows=rows, out=out, **linear)
    assert res is out
    assert_guard(buf.cpu().numpy(), GUARD, GUARD + numel, f"{mode} {tuple(field.shape)}")
    return out.cpu().numpy().reshape(int(ids.numel()), n_comp, t)


def pitched(field2d):
    """the same rows with pitch T + 3 and NaN in the padding: rows that start off every vector boundary"""
    wide = pt.full((field2d.shape[0], field2d.shape[1] + 3), float("nan"), dtype=field2d.dtype, device="cuda")
    wide[:, :field2d.shape[1]] = field2d
    return wide[:, :field2d.shape[1]]


def random_field(shape, f64, seed):
    f = np.random.default_rng(seed).standard_normal(shape)
    return f if f64 else f.astype(np.float32)


# ---- build --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.CASES)
def test_index_is_the_definition(name):
    c, ix = sc.case(name), index_of(name)
    want = sc.emulate_index(c)
    d = c["centers"].shape[1]
    assert ix.depth == want["depth"] and ix.h_min == want["h_min"] and np.array_equal(ix.origin[:d], want["origin"])
    assert np.array_equal(ix.starts.cpu().numpy().view(np.uint64), want["starts"])
    assert np.array_equal(ix.ends.cpu().numpy().view(np.uint64), want["ends"])
    assert np.array_equal(ix.ids.cpu().numpy(), want["ids"])                    # (the sort is stable and no two keys are equal)


@pytest.mark.parametrize("name", sorted(sc.REFUSALS))
def test_build_refuses(name):
    c, count = sc.refusal(name)
    with pytest.raises(ValueError, match=rf"{('off the lattice', 'misaligned', 'overlapping', 'key bits')[sc.REFUSALS[name]]} {count}\b"):
        hipops.cell_index(dev(c["centers"]), dev(c["levels"]), c["width"])


def test_wrappers_validate():
    c = sc.case("tree2d")
    ctr, lv = dev(c["centers"]), dev(c["levels"])
    with pytest.raises(TypeError):
        hipops.cell_index(ctr.float(), lv, c["width"])
    with pytest.raises(TypeError):
        hipops.cell_index(ctr, lv.double(), c["width"])
    with pytest.raises(ValueError):
        hipops.cell_index(ctr, lv, -1.0)
    ix = index_of("tree2d")
    with pytest.raises(TypeError):
        hipops.cell_locate(ix, dev(sc.case("tree3d")["queries"]))
    with pytest.raises(TypeError):
        hipops.cell_locate(ix, dev(c["queries"]).float())
    ids = dev(sc.truth("tree2d")[0])
    field = dev(random_field((len(c["levels"]), 4), True, 0))
    with pytest.raises(ValueError):
        hipops.cell_sample(ids, field, "nearest")
    with pytest.raises(ValueError):
        hipops.cell_sample(ids, field, "linear")
    with pytest.raises(TypeError):
        hipops.cell_sample(ids.long(), field)
    with pytest.raises(TypeError):
        hipops.cell_sample(ids, field.cpu())


# ---- locate -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_rows", [False, True])
@pytest.mark.parametrize("name", sc.CASES)
def test_locate_equals_brute_force(name, with_rows):
    c = sc.case(name)
    got = hipops.cell_locate(index_of(name), dev(c["queries"]), rows=dev(PERM) if with_rows else None).cpu().numpy()
    want = sc.truth(name)[0]
    assert np.array_equal(got, want), f"{(got != want).sum()} of {NQ} queries in another cell, first {np.flatnonzero(got != want)[:5]}"


@pytest.mark.parametrize("name", ["tree2d", "tree3d", "chain2d", "chain3d", "one_cell"])
def test_locate_hostile_coordinates(name):
    c = sc.case(name)
    q = c["queries"][:64].copy()
    ids = sc.truth(name)[0][:64].copy()
    bad = [np.nan, np.inf, -np.inf, 1e300, -1e300, 1e19, -1e19, 2.0 ** 63, -2.0 ** 63]
    for j, v in enumerate(bad * 3):
        q[j, j % q.shape[1]] = v
        ids[j] = -1
    q[40], q[41], q[42], q[43] = np.nan, np.inf, -1e300, 1e300                  # every coordinate
    ids[40:44] = -1
    got = hipops.cell_locate(index_of(name), dev(q)).cpu().numpy()
    assert np.array_equal(got, ids)


# ---- cell mode ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("t", [1, 3, 25, 100, 300])
def test_cell_mode_is_a_bit_exact_copy(t, f64):
    name = "tree3d" if t % 2 else "tree2d"
    c, ids = sc.case(name), sc.truth(name)[0]
    nc = len(c["levels"])
    miss = ids < 0
    d_ids = dev(ids)
    for n_comp in (1, 3):
        f = random_field((nc, n_comp, t), f64, 10 * t + n_comp)
        f[ids[~miss][0], 0, 0], f[ids[~miss][-1], n_comp - 1, t - 1], f[ids[~miss][7], 0, t // 2] = np.inf, -np.inf, -0.0
        want = f[np.maximum(ids, 0)].astype(np.float64)
        want[miss] = np.nan
        rows = dev(PERM) if (t + n_comp + f64) % 2 else None
        fields = [(dev(f), "dense")] if n_comp == 3 else [(dev(f[:, 0]), "dense"), (pitched(dev(f[:, 0])), "pitched")]
        for field, how in fields:
            got = run(d_ids, field, "cell", rows)
            what = f"{name} T {t} {'f64' if f64 else 'f32'} n_comp {n_comp} {how} rows {rows is not None}"
            assert np.isnan(got[miss]).all(), what
            assert np.array_equal(got[~miss].view(np.int64), want[~miss].view(np.int64)), what


def test_cell_mode_wide_fields_and_one_snapshot():
    """more components than one launch takes (groups of three), and a field [rows] of one snapshot"""
    c, ids = sc.case("golden3d"), sc.truth("golden3d")[0]
    f = random_field((len(c["levels"]), 7, 6), False, 3)
    got = hipops.cell_sample(dev(ids), dev(f)).cpu().numpy()
    hit = ids >= 0
    assert got.shape == (NQ, 7, 6) and np.array_equal(got[hit], f[ids[hit]].astype(np.float64)) and np.isnan(got[~hit]).all()
    one = hipops.cell_sample(dev(ids), dev(f[:, 0, 0].copy())).cpu().numpy()
    assert one.shape == (NQ, 1, 1) and np.array_equal(one[hit, 0, 0], f[ids[hit], 0, 0].astype(np.float64))


def test_ids_outside_the_field_are_misses():
    c = sc.case("tree2d")
    nc = len(c["levels"])
    ids = np.array([0, nc - 1, nc, -1, -7, 2 ** 31 - 1, 5], dtype=np.int32)
    f = random_field((nc, 5), True, 1)
    got = run(dev(ids), dev(f), "cell")[:, 0]
    ok = np.array([True, True, False, False, False, False, True])
    assert np.array_equal(got[ok], f[ids[ok]]) and np.isnan(got[~ok]).all()


# ---- linear mode ------------------------------------------------------------------------------------------------------------------
def linear_inputs(name):
    c = sc.case(name)
    return c, dict(index=index_of(name), points=dev(c["queries"]), faces=dev(c["faces"]))


def assert_linear(got, value, mag, d, hit, what):
    assert np.isnan(got[~hit]).all(), f"{what}: misses must be NaN"
    err, bound = np.abs(got[hit].astype(LD) - value[hit]), sc.linear_bound(d, mag[hit])
    worst = float((err / np.maximum(bound, LD(1e-300))).max())
    print(f"{what}: at {worst:.3g} of the bound")
    assert (err <= bound).all(), f"{what}: at {worst:.3g} of the bound"


@pytest.mark.parametrize("t", [1, 3, 25, 100, 300])
@pytest.mark.parametrize("name", ["tree2d", "tree3d", "golden2d", "golden3d"])
def test_linear_mode_against_long_double(name, t):
    """f32 and f64, 1 and 3 components, dense and pitched rows, with and without a row list (thinned: every T sees every value of
    each, not every combination).  Judged per element: on all queries for the short rows, on 400 for the long ones."""
    c, lin = linear_inputs(name)
    d, nn = c["centers"].shape[1], len(c["nodes"])
    ids = sc.truth(name)[0]
    pick = np.arange(NQ) if t <= 25 else np.unique(np.concatenate([[0, NQ - 1], np.random.default_rng(t).choice(NQ, 398, replace=False)]))
    hit = ids[pick] >= 0
    d_ids = dev(ids)
    for f64 in (False, True):
        n_comp = 3 if (t + f64) % 2 else 1
        f = random_field((nn, n_comp, t), f64, 100 * t + f64)
        value, mag = sc.linear_reference(c, c["queries"][pick], ids[pick], f)
        rows = dev(PERM) if (t // 2 + f64) % 2 else None
        fields = [(dev(f), "dense")] if n_comp == 3 else [(dev(f[:, 0]), "dense"), (pitched(dev(f[:, 0])), "pitched")]
        for field, how in fields:
            got = run(d_ids, field, "linear", rows, **lin)
            assert_linear(got[pick], value, mag, d, hit, f"{name} T {t} {'f64' if f64 else 'f32'} n_comp {n_comp} {how} rows {rows is not None}")


@pytest.mark.parametrize("name", ["tree2d", "tree3d", "golden2d", "golden3d", "chain3d"])
def test_linear_mode_reproduces_affine_fields(name):
    c, lin = linear_inputs(name)
    d = c["centers"].shape[1]
    ids = sc.truth(name)[0]
    hit = ids >= 0
    coeffs, offsets = [(1.25, -0.75, 2.5)[:d], (-3.0, 0.5, 0.125)[:d]], [0.3, -1.0]
    f = np.stack([sc.affine_nodes(c, k, o) for k, o in zip(coeffs, offsets)], axis=1)[:, :, None]          # [nn, 2, 1]
    value, mag = sc.linear_reference(c, c["queries"], ids, f)
    got = run(dev(ids), dev(f), "linear", dev(PERM), **lin)
    assert_linear(got, value, mag, d, hit, f"{name} affine")
    for j, (k, o) in enumerate(zip(coeffs, offsets)):
        exact = c["queries"].astype(LD) @ np.asarray(k, dtype=LD) + LD(o)
        bound = sc.linear_bound(d, mag[:, j, 0]) + sc.affine_bound(c, c["queries"], ids, k, o)
        err = np.abs(got[:, j, 0].astype(LD) - exact)
        assert (err[hit] <= bound[hit]).all(), f"{name}: the blend of an affine field is off the field by {float((err[hit] / bound[hit]).max()):.3g} bounds"


@pytest.mark.parametrize("name", ["dyadic2d", "dyadic3d"])
def test_linear_mode_at_cell_centres_is_the_corner_mean(name):
    """on the dyadic grid xi = 1/2 and the weights 2^-d are exact: what is left is the fma chain"""
    c = sc.case(name)
    d, nc = c["centers"].shape[1], len(c["levels"])
    q = c["centers"].copy()
    ids = hipops.cell_locate(index_of(name), dev(q))
    assert np.array_equal(ids.cpu().numpy(), np.arange(nc))
    f = random_field((len(c["nodes"]), 3), True, 8)
    got = run(ids, dev(f), "linear", index=index_of(name), points=dev(q), faces=dev(c["faces"]))[:, 0]
    corners = f[c["faces"]].astype(LD)
    mean, mag = corners.sum(axis=1) / (1 << d), np.abs(corners).sum(axis=1) / (1 << d)
    assert (np.abs(got.astype(LD) - mean) <= sc.linear_bound(d, mag)).all()


# ---- the public interface -----------------------------------------------------------------------------------------------------------
def test_probe_orders_sides_and_batches():
    c = sc.case("tree3d")
    ids = sc.truth("tree3d")[0]
    hit = ids >= 0
    f = random_field((len(c["levels"]), 3), False, 4)
    want = np.where(hit[:, None], f[np.maximum(ids, 0)].astype(np.float64), np.nan)
    # numpy in, numpy out, caller's order
    probe = Probe(c["centers"], c["levels"], c["width"], c["queries"])
    assert isinstance(probe.cell_ids, np.ndarray) and np.array_equal(probe.cell_ids, ids) and np.array_equal(probe.inside, hit)
    got = probe.sample(f)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True)
    # batching: T split 2 + 1 equals one call; a device window is read where it lies
    fd = dev(f)
    parts = [probe.sample(fd[:, :2]), probe.sample(fd[:, 2:])]
    assert all(p.is_cuda for p in parts) and np.array_equal(pt.cat(parts, dim=1).cpu().numpy(), want, equal_nan=True)
    assert np.array_equal(probe.sample(pt.from_numpy(f)).numpy(), want, equal_nan=True)
    one = probe.sample(f[:, 0].copy())
    assert one.shape == (NQ,) and np.array_equal(one, want[:, 0], equal_nan=True)
    vec = probe.sample(np.stack([f, 2 * f], axis=1))
    assert vec.shape == (NQ, 2, 3) and np.array_equal(vec[:, 1], 2 * want, equal_nan=True)
    # device points: ids stay on the device
    on_dev = Probe(dev(c["centers"]), dev(c["levels"]).long().unsqueeze(-1), c["width"], dev(c["queries"]))
    assert on_dev.cell_ids.is_cuda and np.array_equal(on_dev.cell_ids.cpu().numpy(), ids) and on_dev.inside.dtype == pt.bool
    with pytest.raises(ValueError, match="nodes and faces"):
        probe.sample(f, mode="linear")
    with pytest.raises(ValueError):
        probe.sample(f[:-1])
    with pytest.raises(ValueError):
        probe.sample(f, mode="nearest")


def test_probe_linear_and_refusal():
    c = sc.case("golden2d")
    ids = sc.truth("golden2d")[0]
    probe = Probe(c["centers"], c["levels"], c["width"], c["queries"], nodes=c["nodes"], faces=c["faces"])
    f = random_field((len(c["nodes"]), 2, 4), True, 6)
    value, mag = sc.linear_reference(c, c["queries"], ids, f)
    assert_linear(probe.sample(f, mode="linear"), value, mag, 2, ids >= 0, "Probe linear")
    with pytest.raises(ValueError):
        probe.sample(f[:len(c["levels"])], mode="linear")            # a field on the cells
    bad, _ = sc.refusal("overlap")
    with pytest.raises(ValueError, match="overlapping 1"):
        Probe(bad["centers"], bad["levels"], bad["width"], c["queries"])
    with pytest.raises(ValueError):
        Probe(c["centers"], c["levels"], c["width"], c["queries"], nodes=c["nodes"])


def test_probe_from_dataloader(golden_dir):
    from sparsespatialsampling_amd.data import Dataloader
    loader = Dataloader(golden_dir, "s_cube_test_dataset.h5")
    ctr = loader.vertices.numpy()
    case = {"centers": ctr.astype(np.float64), "levels": loader.levels.numpy().astype(np.int32), "width": float(loader._size_initial_cell)}
    shape = (37, 41)
    pts = sampling.raster(ctr.min(axis=0) - 0.02, ctr.max(axis=0) + 0.02, shape)
    probe = Probe.from_dataloader(loader, pts)
    ids, count = sc.brute_force(case, pts)
    assert count.max() == 1 and 0.3 < (ids >= 0).mean() < 0.98
    assert np.array_equal(probe.cell_ids, ids)
    p = loader.load_snapshot("p", "0.4")
    image = probe.sample(p).numpy().reshape(shape)
    want = np.where(ids >= 0, p.numpy()[np.maximum(ids, 0), 0].astype(np.float64), np.nan).reshape(shape)
    assert np.array_equal(image, want, equal_nan=True)
    # the nodes of the file carry a linear blend: x itself comes back
    x_nodes = loader.nodes.numpy()[:, :1].astype(np.float64).copy()
    back = probe.sample(x_nodes, mode="linear")[:, 0]
    hit = ids >= 0
    assert np.abs(back[hit] - pts[hit, 0]).max() <= 64 * 2.0 ** -53 and np.isnan(back[~hit]).all()


def test_probe_from_s_cube_object():
    import types
    c = sc.case("tree2d")
    grid = types.SimpleNamespace(centers=pt.from_numpy(c["centers"]), levels=pt.from_numpy(c["levels"]).long().unsqueeze(-1),
                                 size_initial_cell=c["width"], vertices=pt.from_numpy(c["nodes"]), faces=pt.from_numpy(c["faces"]))
    probe = Probe.from_s_cube(grid, c["queries"])
    assert np.array_equal(probe.cell_ids, sc.truth("tree2d")[0])
    with pytest.raises(ValueError, match="execute_grid_generation"):
        Probe.from_s_cube(types.SimpleNamespace(centers=None), c["queries"])


def test_point_set_helpers():
    ln = sampling.line([0.0, 1.0, 2.0], [1.0, 1.0, 0.0], 5)
    assert ln.shape == (5, 3) and np.array_equal(ln[0], [0, 1, 2]) and np.array_equal(ln[-1], [1, 1, 0]) and np.array_equal(ln[2], [0.5, 1, 1])
    assert np.array_equal(sampling.line([1.0, 2.0], [3.0, 4.0], 1), [[1.0, 2.0]])
    pl = sampling.plane([0.0, 0.0, 0.5], [2.0, 0.0, 0.0], [0.0, 1.0, 0.0], (4, 2))
    assert pl.shape == (8, 3) and np.array_equal(pl.reshape(4, 2, 3)[1, 1], [0.75, 0.75, 0.5]) and (pl[:, 2] == 0.5).all()
    ra = sampling.raster([0.0, 10.0], [4.0, 12.0], (4, 2))
    assert ra.shape == (8, 2) and np.array_equal(ra.reshape(4, 2, 2)[3, 0], [3.5, 10.5]) and np.array_equal(ra[1], [0.5, 11.5])
    vol = sampling.raster([0, 0, 0], [1, 1, 1], (2, 3, 4))
    assert vol.shape == (24, 3) and np.allclose(vol.reshape(2, 3, 4, 3)[1, 2, 3], [0.75, 5 / 6, 0.875])
    with pytest.raises(ValueError):
        sampling.raster([0, 0], [1, 1], (2, 3, 4))
    with pytest.raises(ValueError):
        sampling.line([0, 0], [1, 1, 1], 3)
