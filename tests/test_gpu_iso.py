"""
Isosurfaces and contour lines on the GPU (csrc/iso.hip, sparsespatialsampling_amd/isosurface.py) against the long-double reference
of tests/iso_cases.py.

What is asserted (no figure comes from the code under test):
  counts, offsets, cells, edges     EQUAL the reference: they depend on comparisons only
  frac                              |t - t_ref| <= 4 * 2^-53 * t: one rounding in each difference and in the quotient
  verts                             |x - x_ref| <= 2^-53 * (5 t |x_b - x_a| + |x|): the coordinate difference and the fma add two roundings
  guard zones                       round all five outputs and the count array stay intact
  independence                      the bits depend on neither row_len, the load width, the element type, the run nor the batch split

Shapes: grids of a few thousand cells with holes, shuffled numbering and a ragged last workgroup; T = 1 .. 300 covers one lane
group of every width (4 .. 64 lanes), vector and element loads (dense rows | rows pitched by 3 elements), and rows of several chunks.
"""
import functools

import numpy as np
import pytest
import torch as pt

from tests import iso_cases as ic
from tests.interp_accuracy import GUARD_BITS, assert_guard
from sparsespatialsampling_amd import hipops
from sparsespatialsampling_amd.isosurface import Isosurface

pytestmark = pytest.mark.gpu

GUARD = 512                 # int64 words on either side
T_SIZES = [1, 3, 4, 25, 100, 300]


def dev(a):
    return pt.from_numpy(np.ascontiguousarray(a)).cuda()


def pitched(field2d):
    """the same rows with pitch T + 3 and NaN in the padding: rows that start off every vector boundary"""
    wide = pt.full((field2d.shape[0], field2d.shape[1] + 3), float("nan"), dtype=field2d.dtype, device="cuda")
    wide[:, :field2d.shape[1]] = field2d
    return wide[:, :field2d.shape[1]]


class Guarded:
    """a device array of ``shape`` between two zones of GUARD_BITS"""

    def __init__(self, shape, dtype):
        self.numel, self.item = int(np.prod(shape)), pt.empty(0, dtype=dtype).element_size()
        words = (self.numel * self.item + 7) // 8
        self.buf = pt.full((GUARD + words + GUARD,), int(GUARD_BITS), dtype=pt.int64, device="cuda")
        self.out = self.buf[GUARD:GUARD + words].view(dtype)[:self.numel].view(shape)
        self.hi = GUARD + words

    def check(self, what):
        bits = self.buf.cpu().numpy()
        assert_guard(bits, GUARD, self.hi, what)
        used = self.numel * self.item % 8                                       # the rest of the last word of an int32 array
        if used:
            assert np.array_equal(bits[self.hi - 1:self.hi].view(np.uint8)[used:], np.array([GUARD_BITS]).view(np.uint8)[used:]), f"{what}: tail written"
        return bits[GUARD:self.hi]


def run(field, faces, nodes, level, short=0, what=""):
    """count -> scan -> emit through ``hipops``, every array inside guard zones -> dict of numpy arrays as ``iso_cases.extract``
    gives them; ``short``: the capacity handed to the emit is that much smaller than the total"""
    t = int(field.shape[1]) if field.dim() == 2 else 1
    n_cells, d = int(faces.shape[0]), int(nodes.shape[1])
    n = t * n_cells
    count = Guarded((n + 1,), pt.int32)
    count.out[n:].zero_()                                                       # (one entry more: its scan is the total)
    hipops.iso_count(field, faces, level, out=count.out)
    count.check(f"{what} count")
    counts = count.out[:n].cpu().numpy().reshape(t, n_cells)
    scan = hipops.exclusive_scan(count.out)
    total = int(scan[n])
    assert total == counts.sum()
    outs = {"verts": Guarded((total, d, d), pt.float64), "edges": Guarded((total, d, 2), pt.int32), "frac": Guarded((total, d), pt.float64),
            "cells": Guarded((total,), pt.int32)}
    hipops.iso_emit(field, faces, level, nodes, scan, total - short, **{k: g.out for k, g in outs.items()})
    res = {"offsets": np.concatenate([[0], np.cumsum(counts.sum(axis=1))]).astype(np.int64), "counts": counts}
    for key, g in outs.items():
        g.check(f"{what} {key}")
        res[key] = g.out.cpu().numpy()
    return res


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.int64) if a[k].dtype == np.float64 else a[k], b[k].view(np.int64) if b[k].dtype == np.float64 else b[k])
               for k in ic.KEYS)


@functools.lru_cache(maxsize=None)
def device_grid(name):
    c = ic.grid(name)
    return dev(c["nodes"]), dev(c["faces"])


# ---- every mask: the kernel's tables ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("d,n_snap", [(3, 256), (2, 16)])
def test_every_mask(d, n_snap, f64):
    nodes, faces, field, level = ic.every_mask(d, n_snap)
    field = field if f64 else field.astype(np.float32)
    ref = ic.extract(nodes, faces, field, level)
    got = run(dev(field), dev(faces), dev(nodes), level, what="every mask")
    ic.check(got, ref, f"every mask {d}-D {'f64' if f64 else 'f32'}")
    assert len(ref["cells"]) > 3 * n_snap // 2


# ---- grids -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_snap", T_SIZES)
@pytest.mark.parametrize("name", ic.GRIDS)
def test_grids(name, n_snap):
    c = ic.grid(name)
    nodes, faces = device_grid(name)
    smooth = ic.smooth_field(name, n_snap)
    for f64 in (True, False):
        field = smooth if f64 else smooth.astype(np.float32)
        ref = ic.extract(c["nodes"], c["faces"], field, ic.SMOOTH_LEVEL)
        assert (np.diff(ref["offsets"]) > 0).all()
        d_field = dev(field)
        for layout in ("dense", "pitched"):
            what = f"{name} T={n_snap} {'f64' if f64 else 'f32'} {layout}"
            got = run(d_field if layout == "dense" else pitched(d_field), faces, nodes, ic.SMOOTH_LEVEL, what=what)
            ic.check(got, ref, what)


# ---- weldability on the device output ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3])
def test_device_output_is_weldable(d):
    c = ic.uniform(d)
    got = run(dev(c["field"]), dev(c["faces"]), dev(c["nodes"]), ic.UNIFORM_LEVEL, what="uniform")
    ic.assert_closed(got, d, f"uniform {d}-D on the device")


# ---- ties and refusals ----------------------------------------------------------------------------------------------------------
def hostile_case(d):
    """the uniform grid, level 0: node values equal to the level, -0.0, NaN and +-inf planted at nodes of cut cells, three snapshots"""
    c = ic.uniform(d)
    base = c["field"] - ic.UNIFORM_LEVEL
    cut = np.unique(ic.extract(c["nodes"], c["faces"], base, 0.0)["cells"])
    picks = c["faces"][cut[:: max(1, len(cut) // 12)]][:, 0]
    field = np.stack([base, base + 0.013, base - 0.017], axis=1)
    for j, node in enumerate(picks):
        field[node, j % 3] = [0.0, -0.0, np.nan, np.inf, -np.inf, 0.0][j % 6]
    return c, field


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("d", [2, 3])
def test_ties_and_non_finite_corners(d, f64):
    c, field = hostile_case(d)
    field = field if f64 else field.astype(np.float32)
    ref = ic.extract(c["nodes"], c["faces"], field, 0.0)
    tie = ic.extract(c["nodes"], c["faces"], field, 0.0, arith="f64", mistake="gt")
    assert tie["edges"].shape != ref["edges"].shape or not np.array_equal(tie["edges"], ref["edges"])      # the planted ties decide primitives
    got = run(dev(field), dev(c["faces"]), dev(c["nodes"]), 0.0, what="hostile")
    ic.check(got, ref, f"hostile {d}-D")


def test_bad_corner_ids_load_nothing():
    c = ic.grid("tree3d")
    n = len(c["nodes"])
    faces = c["faces"].copy()
    rng = np.random.default_rng(3)
    bad = rng.permutation(len(faces))[:40]
    faces[bad[:20], rng.integers(0, 8, 20)] = -1
    faces[bad[20:], rng.integers(0, 8, 20)] = n
    smooth = ic.smooth_field("tree3d", 4)
    ref = ic.extract(c["nodes"], faces, smooth, ic.SMOOTH_LEVEL)
    assert len(ref["cells"]) < len(ic.extract(c["nodes"], c["faces"], smooth, ic.SMOOTH_LEVEL)["cells"])
    # the field is a window of a larger allocation whose rows -1 and n would give primitives: a missing check shows as a wrong result
    big = np.concatenate([smooth[:1] - 1.0, smooth, smooth[-1:] + 1.0])
    window = dev(big)[1:n + 1]
    got = run(window, dev(faces), dev(c["nodes"]), ic.SMOOTH_LEVEL, what="bad ids")
    ic.check(got, ref, "bad ids")
    assert not np.isin(got["cells"], bad).any()


def test_capacity_one_short():
    c = ic.uniform(3)
    args = (dev(c["field"]), dev(c["faces"]), dev(c["nodes"]), ic.UNIFORM_LEVEL)
    full, short = run(*args), run(*args, short=1)
    guard_f64 = np.array([GUARD_BITS]).view(np.float64)[0]
    for key in ("verts", "edges", "frac", "cells"):
        a, b = full[key], short[key]
        assert np.array_equal(a[:-1].view(np.int64) if a.dtype == np.float64 else a[:-1], b[:-1].view(np.int64) if a.dtype == np.float64 else b[:-1])
        if a.dtype == np.float64:
            assert (b[-1].view(np.int64) == GUARD_BITS).all() and not np.isnan(a[-1]).any() and np.isnan(guard_f64)
        else:
            assert np.isin(b[-1], np.array([GUARD_BITS]).view(np.int32)).all() and (a[-1] >= 0).all()


def test_level_must_be_finite():
    c = ic.uniform(2)
    field, faces = dev(c["field"]), dev(c["faces"])
    for level in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            hipops.iso_count(field, faces, level)
        with pytest.raises(ValueError):
            Isosurface(c["nodes"], c["faces"]).extract(c["field"], level)
    with pytest.raises(TypeError):
        hipops.iso_count(field, faces.long(), 0.0)
    with pytest.raises(TypeError):
        hipops.iso_count(field.cpu(), faces, 0.0)
    with pytest.raises(ValueError):
        Isosurface(c["nodes"], c["faces"]).extract(c["field"][:-1], 0.0)
    with pytest.raises(ValueError):
        Isosurface(c["nodes"], c["faces"] + 1)


# ---- independence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tree3d", "tree2d"])
def test_bits_do_not_depend_on_the_launch(name):
    c = ic.grid(name)
    nodes, faces = device_grid(name)
    field32 = dev(ic.smooth_field(name, 100).astype(np.float32))
    batch = run(field32, faces, nodes, ic.SMOOTH_LEVEL)
    assert same_bits(batch, run(field32, faces, nodes, ic.SMOOTH_LEVEL))                           # two runs
    assert same_bits(batch, run(field32.double(), faces, nodes, ic.SMOOTH_LEVEL))                  # f32 gives the bits of its f64 copy
    assert same_bits(batch, run(pitched(field32), faces, nodes, ic.SMOOTH_LEVEL))                  # element loads
    for t in (0, 37, 99):
        alone = run(field32[:, t].contiguous(), faces, nodes, ic.SMOOTH_LEVEL)
        lo, hi = batch["offsets"][t], batch["offsets"][t + 1]
        assert hi - lo == alone["offsets"][1] > 0
        for key in ("verts", "edges", "frac", "cells"):
            assert np.array_equal(batch[key][lo:hi].view(np.int32), alone[key].view(np.int32)), (t, key)
    # the split into sub-batches: 7 snapshots per launch instead of one launch
    iso = Isosurface(c["nodes"], c["faces"])
    one = iso.extract(field32, ic.SMOOTH_LEVEL)
    split = iso.extract(field32, ic.SMOOTH_LEVEL, _count_bytes=7 * 4 * len(c["faces"]))
    assert hipops.iso_batch_columns(len(c["faces"]), nodes.shape[1], 7 * 4 * len(c["faces"])) == 7
    assert np.array_equal(one.offsets, batch["offsets"]) and np.array_equal(split.offsets, batch["offsets"])
    assert np.array_equal(iso.count(field32, ic.SMOOTH_LEVEL, _count_bytes=7 * 4 * len(c["faces"])), np.diff(batch["offsets"]))
    for res in (one, split):
        assert res.vertices.is_cuda
        got = {"offsets": res.offsets, "verts": res.vertices.cpu().numpy(), "edges": res.edges.cpu().numpy(), "frac": res.frac.cpu().numpy(),
               "cells": res.cells.cpu().numpy()}
        assert same_bits(batch, got)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_end_to_end_on_a_generated_grid(tmp_path):
    from inputs import refine_inputs
    from sparsespatialsampling_amd import geometry
    from sparsespatialsampling_amd.geometry.geometry_STL_3d import read_stl
    from sparsespatialsampling_amd.sparse_spatial_sampling import SparseSpatialSampling

    # the unit cube with a refined sphere body of radius 0.12 at (0.4, 0.5, 0.5)
    x, y, geos, kw = refine_inputs("refine_3d_delta", geometry)
    kw = {{"uniform_level": "uniform_levels"}.get(k, k): v for k, v in kw.items()}
    centre = pt.tensor([0.4, 0.5, 0.5], dtype=pt.float64)
    s_cube = SparseSpatialSampling(pt.from_numpy(x), pt.from_numpy(y), geos, str(tmp_path), "iso", **kw)
    s_cube.execute_grid_generation()
    nodes, faces = s_cube.vertices.numpy().astype(np.float64), s_cube.faces.numpy()
    # a plane through the body (where the grid has no cells the surface simply ends) and a sphere round another point
    field = np.stack([nodes @ np.array([0.3, 1.0, -0.2]), np.linalg.norm(nodes - np.array([0.2, 0.3, 0.4]), axis=1)], axis=1)
    level = float(np.array([0.3, 1.0, -0.2]) @ centre.numpy())
    ref = ic.extract(nodes, faces, field, level)
    iso = Isosurface.from_s_cube(s_cube)
    res = iso.extract(field, level)
    assert isinstance(res.vertices, np.ndarray)
    got = {"offsets": res.offsets, "verts": res.vertices, "edges": res.edges, "frac": res.frac, "cells": res.cells}
    ic.check(got, ref, "generated grid")
    assert np.array_equal(iso.count(field, level), np.diff(ref["offsets"])) and (np.diff(ref["offsets"]) > 0).all()

    back = res.interpolate(field)
    fa, fb = field[res.edges[..., 0]], field[res.edges[..., 1]]                  # [n, 3, 2]
    col = np.repeat(np.arange(2), np.diff(res.offsets))[:, None]
    mag = np.abs(np.take_along_axis(fa, col[..., None], axis=2)[..., 0]) + np.abs(np.take_along_axis(fb, col[..., None], axis=2)[..., 0])
    assert (np.abs(back - level) <= 4 * 2.0 ** -53 * mag).all()
    for t in (0, 1):
        points, index = res.weld(t)
        assert np.array_equal(points[index].view(np.int64), res.snapshot(t)[0].view(np.int64))
        assert len(points) == len(np.unique(ic.vertex_keys(res.snapshot(t)[1])))
    path = str(tmp_path / "iso.stl")
    res.write_stl(path, 0)
    assert np.array_equal(read_stl(path), res.snapshot(0)[0].astype(np.float32).astype(np.float64))
    with pytest.raises(ValueError, match="execute_grid_generation"):
        Isosurface.from_s_cube(type("Empty", (), {"centers": None})())
