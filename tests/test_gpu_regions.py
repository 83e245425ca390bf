"""
Face neighbours, connected-region labels and the region table on the GPU (csrc/regions.hip, sparsespatialsampling_amd/regions.py)
against the references of tests/region_cases.py.

What is asserted (no figure comes from the code under test):
  neighbour table                       EQUALS the definition in numpy, which tests/test_region_checker.py holds against brute force
  labels                                EQUAL csgraph's components named by their smallest cell, for every mask of ``region_cases.cases``
  offsets, label, n_cells, box, g_min, g_max    EQUAL the reference
  volume, integral, centroid            within n * 2^-53 * sum |terms| of the long-double sums (``region_cases.check_table``)
  independence                          label bits do not depend on the run, the batch split, dense or pitched rows, the launch order
                                        or, for values float32 holds, the element type; table bits not on the run, the pitch or the split
  guard zones                           round the neighbour table and the labels stay intact

Shapes: the grids of tests/sample_cases.py (a few thousand cells with holes, shuffled numbering and a ragged last workgroup; level
jumps up to 5) and two uniform ones; T = 1 .. 300 covers one lane group of every width (4 .. 64 lanes) and rows of several chunks;
rows dense or pitched by 3 elements with NaN padding, float32 and float64.
"""
import functools

import numpy as np
import pytest
import torch as pt

from tests import region_cases as rc
from tests.interp_accuracy import GUARD_BITS, assert_guard
from sparsespatialsampling_amd import hipops
from sparsespatialsampling_amd.grid import Grid
from sparsespatialsampling_amd.regions import Regions, RegionTable
from sparsespatialsampling_amd.sampling import Probe

pytestmark = pytest.mark.gpu

GUARD = 512                 # int64 words on either side
T_SIZES = [1, 3, 4, 25, 100, 300]
PAD = 3


def dev(a):
    return pt.from_numpy(np.ascontiguousarray(a)).cuda()


def pitched(rows, fill=float("nan")):
    """the same rows with pitch T + 3 and ``fill`` in the padding: rows that start off every vector boundary"""
    wide = pt.full((rows.shape[0], rows.shape[1] + PAD), fill, dtype=rows.dtype, device="cuda")
    wide[:, :rows.shape[1]] = rows
    return wide[:, :rows.shape[1]]


class GuardedLabels:
    """int32 [n, t] (pitch t + ``pad``) between two zones of GUARD_BITS; the padding holds GUARD_BITS too"""

    def __init__(self, n, t, pad=0):
        self.words = (n * (t + pad) * 4 + 7) // 8
        self.buf = pt.full((GUARD + self.words + GUARD,), int(GUARD_BITS), dtype=pt.int64, device="cuda")
        self.flat = self.buf[GUARD:GUARD + self.words].view(pt.int32)
        self.out = self.flat[:n * (t + pad)].view(n, t + pad)[:, :t]
        self.n, self.t, self.pad = n, t, pad

    def check(self, what):
        assert_guard(self.buf.cpu().numpy(), GUARD, GUARD + self.words, what)
        flat = self.flat.cpu().numpy()
        fill = np.array([GUARD_BITS]).view(np.int32)
        rows = flat[:self.n * (self.t + self.pad)].reshape(self.n, self.t + self.pad)
        expect = np.tile(fill, flat.size // 2 + 1)[:flat.size]
        assert np.array_equal(flat[self.n * (self.t + self.pad):], expect[self.n * (self.t + self.pad):]), f"{what}: tail written"
        if self.pad:
            assert np.array_equal(rows[:, self.t:], expect[:rows.size].reshape(rows.shape)[:, self.t:]), f"{what}: padding written"
        return rows[:, :self.t].copy()


@functools.lru_cache(maxsize=None)
def device_grid(name):
    c = rc.grid(name)
    index = hipops.cell_index(dev(c["centers"]), dev(c["levels"]), c["width"])
    return index, hipops.cell_neighbours(index), hipops.spatial_order(index.centers)


def label(name, field, lo, hi, **kw):
    _, nbr, order = device_grid(name)
    kw.setdefault("order", order)
    return hipops.region_label(field, nbr, lo, hi, **kw).cpu().numpy()


def table_arrays(res):
    return {k: (v if isinstance(v, np.ndarray) or v is None else v.cpu().numpy()) for k, v in res.items()}


def same_table(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k].view(np.int64) if a[k].dtype == np.float64 else a[k],
                                                               b[k].view(np.int64) if b[k].dtype == np.float64 else b[k]) for k in a)


# ---- neighbours ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.GRIDS)
def test_neighbour_table(name):
    index = device_grid(name)[0]
    n, d = index.n_cells, index.dim
    out = GuardedLabels(n, 2 * d)
    hipops.cell_neighbours(index, out=out.out)
    assert np.array_equal(out.check(f"{name} neighbours"), rc.emulate_neighbours(name))


def test_grid_neighbours_are_built_once():
    c = rc.grid("tree3d")
    grid = Grid(c["centers"], c["levels"], c["width"])
    assert grid._neighbours is None
    nbr = grid.neighbours
    assert grid.neighbours is nbr and np.array_equal(nbr.cpu().numpy(), rc.emulate_neighbours("tree3d"))
    with pytest.raises(ValueError):
        Grid(nodes=c["nodes"], faces=c["faces"]).neighbours


# ---- labels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.GRIDS)
def test_labels_of_every_mask(name):
    for mask_name, (field, lo, hi) in rc.cases(name).items():
        rc.check_labels(label(name, dev(field), lo, hi), rc.labels_of(name, mask_name), f"{name} {mask_name}")


@pytest.mark.parametrize("n_t", T_SIZES)
@pytest.mark.parametrize("name", rc.TREES)
def test_labels_of_every_row_length(name, n_t):
    mask = rc.random_mask(name, 0.5, n_t)
    ref = rc.reference_labels(rc.brute_edges(name), mask)
    n = len(mask)
    dense = GuardedLabels(n, n_t)
    hipops.region_label(dev(mask.astype(np.float32)), device_grid(name)[1], 0.5, np.inf, order=device_grid(name)[2], out=dense.out)
    rc.check_labels(dense.check(f"{name} T={n_t} dense"), ref, f"{name} T={n_t} f32 dense")
    wide = GuardedLabels(n, n_t, PAD)
    hipops.region_label(pitched(dev(mask.astype(np.float64))), device_grid(name)[1], 0.5, np.inf, out=wide.out)
    rc.check_labels(wide.check(f"{name} T={n_t} pitched"), ref, f"{name} T={n_t} f64 pitched")


@pytest.mark.parametrize("name", rc.TREES + ["uniform2d"])
def test_label_bits_depend_on_the_inputs_alone(name):
    for mask_name in ("random0.5", "smooth32"):
        field, lo, hi = rc.cases(name)[mask_name]
        ref = rc.labels_of(name, mask_name)
        d_field = dev(field)
        n, n_t = field.shape
        runs = {"again": label(name, d_field, lo, hi), "natural order": label(name, d_field, lo, hi, order=None),
                "pitched": label(name, pitched(d_field), lo, hi), "float64": label(name, dev(field.astype(np.float64)), lo, hi)}
        split = pt.full((n, n_t), -7, dtype=pt.int32, device="cuda")
        for c0 in range(0, n_t, 2):                                            # windows of the field into windows of the labels
            label(name, d_field[:, c0:c0 + 2], lo, hi, out=split[:, c0:c0 + 2])
        runs["split"] = split.cpu().numpy()
        for what, got in runs.items():
            rc.check_labels(got, ref, f"{name} {mask_name} {what}")


def test_label_phases_are_launches_of_their_own():
    name = "tree2d"
    field, lo, hi = rc.cases(name)["random0.5"]
    _, nbr, order = device_grid(name)
    out = hipops.region_label(dev(field), nbr, lo, hi, phases=("init",))
    assert np.array_equal(out.cpu().numpy(), np.where(field > 0.5, np.arange(len(field))[:, None], -1))
    hipops.region_label(dev(field), nbr, lo, hi, order=order, out=out, phases=("hook",))
    hipops.region_label(dev(field), nbr, lo, hi, out=out, phases=("flatten",))
    rc.check_labels(out.cpu().numpy(), rc.labels_of(name, "random0.5"), "phase by phase")


# ---- the table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("name", rc.TREES + ["uniform2d", "chain3d"])
def test_table(name, f64):
    labels = rc.labels_of(name, "random0.5")
    g = rc.weight_field(name, labels.shape[1]).astype(np.float64 if f64 else np.float32)
    ref = rc.reference_table(name, labels, g)
    index = device_grid(name)[0]
    d_labels, d_g = dev(labels), dev(g)
    got = table_arrays(hipops.region_table(d_labels, index, d_g))
    rc.check_table(got, ref, f"{name} table")
    assert same_table(got, table_arrays(hipops.region_table(d_labels, index, d_g))), "another run, other bits"
    assert same_table(got, table_arrays(hipops.region_table(pitched(d_labels, -1), index, pitched(d_g)))), "pitched rows, other bits"
    assert same_table(got, table_arrays(hipops.region_table(d_labels, index, d_g, pair_bytes=12 * len(labels)))), "one column a launch, other bits"
    bare = table_arrays(hipops.region_table(d_labels, index))
    assert bare["integral"] is None and bare["g_min"] is None and bare["g_max"] is None
    assert same_table({k: v for k, v in got.items() if bare[k] is not None}, {k: v for k, v in bare.items() if v is not None})


@pytest.mark.parametrize("n_t", [25, 100])
def test_table_of_long_rows(n_t):
    name = "tree2d"
    labels = rc.reference_labels(rc.brute_edges(name), rc.random_mask(name, 0.5, n_t))
    g = rc.weight_field(name, n_t)
    got = table_arrays(hipops.region_table(dev(labels), device_grid(name)[0], dev(g)))
    rc.check_table(got, rc.reference_table(name, labels, g), f"{name} T={n_t}")


def test_table_of_drawn_masks():
    name = "uniform2d"
    labels = rc.labels_of(name, "drawn")
    g = rc.weight_field(name, 3).astype(np.float32)
    got = table_arrays(hipops.region_table(dev(labels), device_grid(name)[0], dev(g)))
    rc.check_table(got, rc.reference_table(name, labels, g), "drawn masks")               # (two regions of more than 1024 cells)
    assert same_table(got, table_arrays(hipops.region_table(pitched(dev(labels), -1), device_grid(name)[0], pitched(dev(g)))))
    assert got["offsets"].tolist() == [0, 1, 2, 2 + 2048] and got["n_cells"][0] > 1900


# ---- degenerate inputs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one_cell", "level3", "uniform3d"])
def test_all_in_and_all_out(name):
    field, lo, hi = rc.cases(name)["all_in_all_out"]
    n = len(field)
    got = label(name, dev(field), lo, hi)
    assert np.array_equal(got, np.stack([np.zeros(n, dtype=np.int32), np.full(n, -1, dtype=np.int32)], axis=1))
    table = table_arrays(hipops.region_table(dev(got), device_grid(name)[0], dev(rc.weight_field(name, 2))))
    rc.check_table(table, rc.reference_table(name, got, rc.weight_field(name, 2)), f"{name} all in / all out")
    assert table["offsets"].tolist() == [0, 1, 1] and table["label"].tolist() == [0] and table["n_cells"].tolist() == [n]
    none = hipops.region_table(dev(got[:, 1:].copy()), device_grid(name)[0])
    assert none["offsets"].tolist() == [0, 0] and none["label"].numel() == 0 and tuple(none["centroid"].shape) == (0, rc.grid(name)["centers"].shape[1])


# ---- the front end ------------------------------------------------------------------------------------------------------------
def test_regions_front_end(monkeypatch):
    name = "tree2d"
    c = rc.grid(name)
    calls = []
    real = hipops.cell_index
    monkeypatch.setattr(hipops, "cell_index", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    grid = Grid(c["centers"], c["levels"], c["width"])
    probe, regions = Probe.from_grid(grid, c["queries"]), Regions.from_grid(grid)
    assert len(calls) == 1 and regions._index is probe._index is grid.index and regions._neighbours is grid.neighbours
    field, lo, hi = rc.cases(name)["smooth64"]
    g = rc.weight_field(name, field.shape[1])
    ref_labels = rc.labels_of(name, "smooth64")
    labels = regions.label(field, lo, hi)
    assert isinstance(labels, np.ndarray)
    rc.check_labels(labels, ref_labels, "Regions.label")
    on_device = regions.label(dev(field)[:, 1:3], lo, hi)
    assert on_device.is_cuda and np.array_equal(on_device.cpu().numpy(), ref_labels[:, 1:3])
    assert np.array_equal(regions.label(field[:, 0], lo, hi), ref_labels[:, 0])
    out = pt.empty((len(field), 3), dtype=pt.int32, device="cuda")
    assert regions.label(field, lo, hi, out=out) is out and np.array_equal(out.cpu().numpy(), ref_labels)
    # a boolean mask is the field's own in-set
    mask = rc.in_mask(field, lo, hi)
    assert np.array_equal(regions.label(mask), ref_labels) and np.array_equal(regions.label(pt.from_numpy(mask)).numpy(), ref_labels)
    # table and extract: the hipops calls
    direct = table_arrays(hipops.region_table(dev(ref_labels), grid.index, dev(g)))
    for table in (regions.table(labels, weight=g), regions.extract(field, lo, hi, weight=g)):
        assert isinstance(table, RegionTable) and isinstance(table.volume, np.ndarray)
        assert same_table(direct, {"offsets": table.offsets, **{k: getattr(table, k) for k in RegionTable.FIELDS}})
    rc.check_table(direct, rc.reference_table(name, ref_labels, g), "Regions.table")
    assert np.array_equal(table.n_regions, np.diff(direct["offsets"])) and len(table) == direct["offsets"][-1]
    one = table.of_snapshot(1)
    assert np.array_equal(one["label"], direct["label"][direct["offsets"][1]:direct["offsets"][2]])
    assert regions.extract(dev(field), lo, hi).volume.is_cuda and regions.extract(dev(field), lo, hi).integral is None
    # largest: by volume, the reference's order
    top = table.largest(2)
    for t in range(3):
        a, b = direct["offsets"][t], direct["offsets"][t + 1]
        order = sorted(range(a, b), key=lambda r: (-direct["volume"][r], direct["label"][r]))[:2]
        assert np.array_equal(top.of_snapshot(t)["label"], direct["label"][order])
    # malformed arguments
    for bad in (lambda: regions.label(field[:-1], lo, hi), lambda: regions.label(field, hi, lo), lambda: regions.label(field, float("nan"), hi),
                lambda: regions.label(np.zeros(field.shape, dtype=np.int64), lo, hi), lambda: regions.label(field[:, :0], lo, hi),
                lambda: regions.label([1.0, 2.0], lo, hi), lambda: regions.table(labels.astype(np.int64)),
                lambda: regions.table(labels, weight=g[:, :2]), lambda: regions.label(field, lo, hi, out=pt.empty((len(field), 2), dtype=pt.int32, device="cuda")),
                lambda: table.largest(0), lambda: Regions.from_grid(Grid(nodes=c["nodes"], faces=c["faces"])),
                lambda: Regions(c["centers"], c["levels"][:-1], c["width"])):
        with pytest.raises(ValueError):
            bad()


def test_largest_breaks_ties_by_label():
    """the checkerboard: 2048 regions of one volume"""
    c = rc.grid("uniform2d")
    regions = Regions(c["centers"], c["levels"], c["width"])
    table = regions.extract(rc.uniform2d_masks()["checkerboard"])
    top = table.largest(3)
    assert top.label.tolist() == [0, 2, 4] and top.offsets.tolist() == [0, 3] and len(set(table.volume.tolist())) == 1
