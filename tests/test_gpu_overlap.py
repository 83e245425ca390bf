"""
The overlap table on the GPU (csrc/overlap.hip, ``hipops.overlap_table``) and the tracks built on it (``Regions.overlap``,
``Regions.track``) against the references of tests/track_cases.py.

What is asserted (no figure comes from the code under test, no tolerance anywhere):
  offsets, src, dst, n_cells, units     EQUAL ``reference_overlap`` (a dict over the cells, units from the integer levels)
  volume                                EQUAL ``np.float64(units) * hd`` bit for bit
  independence                          equal bits across reruns, the one-key and the two-pass sort route, dense and pitched rows,
                                        separate arrays and overlapping windows of one allocation, and batch splits
  inputs                                the label arrays, their padding and the guard zones round them stay as they were
  tracks, events, velocity              EQUAL ``reference_tracks`` on planted motion, from ``Regions.label`` to ``Regions.track``

The label arrays are uploaded from the CPU reference, so nothing here rests on the labelling kernel except the end-to-end test.
Shapes: every grid of ``region_cases.GRIDS`` (one cell to 6482 cells; chain2d / chain3d with 62 / 63 key bits and units up to 2^60);
row_len 1 .. 100 covers every tile width of the count and emit launches (4 .. 64 columns) and rows of two tiles.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch as pt

from tests import region_cases as rc
from tests import track_cases as tc
from tests.interp_accuracy import GUARD_BITS, assert_guard
from sparsespatialsampling_amd import _lib, hipops
from sparsespatialsampling_amd.regions import OverlapTable, Regions, RegionTable, RegionTracks

pytestmark = pytest.mark.gpu

GUARD = 512                 # int64 words on either side
T_SIZES = [1, 2, 3, 4, 25, 100]
PAD = 3
_HIP_ERROR = []


def _guarded(fn):
    """after a HIP error nothing more is started on the GPU in this process"""
    if _HIP_ERROR:
        pytest.fail("not run: an earlier test of this module ended with a HIP error: " + _HIP_ERROR[0], pytrace=False)
    try:
        return fn()
    except AssertionError:
        raise
    except Exception as e:                                      # noqa: BLE001
        text = f"{type(e).__name__}: {e}"
        if any(w in text.lower() for w in ("code -3", "illegal memory", "hip error", "hiperror", "memory access fault")):   # (-3: S3_EHIP)
            _HIP_ERROR.append(text[:300])
        raise


def guarded(test):
    @functools.wraps(test)
    def run(*args, **kwargs):
        return _guarded(lambda: test(*args, **kwargs))
    return run


def dev(a):
    return pt.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def index_of(name):
    c = rc.grid(name)
    return hipops.cell_index(dev(c["centers"]), dev(c["levels"]), c["width"])


def arrays(res):
    return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in res.items()}


def same(a, b):
    return all(np.array_equal(a[k].view(np.int64) if a[k].dtype == np.float64 else a[k], b[k].view(np.int64) if b[k].dtype == np.float64 else b[k]) for k in a)


class GuardedRows:
    """int32 [n, t + pad] holding ``labels`` with -1 in the padding, between two zones of GUARD_BITS; ``rows``: the [n, t] window"""

    def __init__(self, labels, pad):
        n, t = labels.shape
        host = np.full((n, t + pad), -1, dtype=np.int32)
        host[:, :t] = labels
        flat = np.full(2 * GUARD + (host.size * 4 + 7) // 8, GUARD_BITS, dtype=np.int64)
        flat[GUARD:len(flat) - GUARD].view(np.int32)[:host.size] = host.ravel()
        self.before = flat
        self.buf = dev(flat)
        self.rows = self.buf[GUARD:len(flat) - GUARD].view(pt.int32)[:host.size].view(n, t + pad)[:, :t]

    def check(self, what):
        after = self.buf.cpu().numpy()
        assert_guard(after, GUARD, len(after) - GUARD, what)
        assert np.array_equal(after, self.before), f"{what}: a label array was written"


@functools.lru_cache(maxsize=None)
def random_pair(name, n_t=None):
    """(a, b, reference): two labellings of other masks, column by column"""
    if n_t is None:
        a, b = rc.labels_of(name, "random0.5"), rc.labels_of(name, "random0.7")
    else:
        a, b = tc.columns(name, "random0.5", n_t), tc.columns(name, "random0.7", n_t, 3)
    return a, b, tc.reference_overlap(name, a, b)


# ---- the table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.GRIDS)
@guarded
def test_overlap_table_equals_the_reference(name):
    a, b, ref = random_pair(name)
    d_a, d_b = dev(a), dev(b)
    got = arrays(hipops.overlap_table(d_a, d_b, index_of(name)))
    tc.check_overlap(got, ref, name)
    assert same(got, arrays(hipops.overlap_table(d_a, d_b, index_of(name)))), f"{name}: a rerun gives other bits"
    two = arrays(hipops.overlap_table(d_a, d_b, index_of(name), two_pass=True))
    tc.check_overlap(two, ref, f"{name} two passes")
    assert same(got, two), f"{name}: the two-pass route gives other bits"
    assert np.array_equal(d_a.cpu().numpy(), a) and np.array_equal(d_b.cpu().numpy(), b)


@pytest.mark.parametrize("n_t", T_SIZES)
@pytest.mark.parametrize("name", rc.TREES)
@guarded
def test_row_lengths_pitches_and_windows(name, n_t):
    a, b, ref = random_pair(name, n_t)
    index = index_of(name)
    got = arrays(hipops.overlap_table(dev(a), dev(b), index))
    tc.check_overlap(got, ref, f"{name} T={n_t}")
    g_a, g_b = GuardedRows(a, PAD), GuardedRows(b, PAD)            # rows that start off every vector boundary, -1 in the padding
    for two_pass in (False, True):
        tc.check_overlap(arrays(hipops.overlap_table(g_a.rows, g_b.rows, index, two_pass=two_pass)), ref, f"{name} T={n_t} pitched two_pass={two_pass}")
    g_a.check(f"{name} T={n_t} a"), g_b.check(f"{name} T={n_t} b")
    # tracking's shape: A and B two windows of one allocation, one pitch
    one = tc.columns(name, "random0.7", n_t + 1)
    ref_w = tc.reference_overlap(name, one[:, :-1], one[:, 1:])
    g = GuardedRows(one, 0)
    for two_pass in (False, True):
        tc.check_overlap(arrays(hipops.overlap_table(g.rows[:, :n_t], g.rows[:, 1:], index, two_pass=two_pass)), ref_w, f"{name} T={n_t} windows")
    g.check(f"{name} T={n_t} windows")


@pytest.mark.parametrize("name", ["tree3d", "uniform2d"])
@guarded
def test_batch_splits_give_equal_bits(name):
    a, b, ref = random_pair(name, 25)
    index = index_of(name)
    d_a, d_b = dev(a), dev(b)
    whole = arrays(hipops.overlap_table(d_a, d_b, index))
    for columns in (1, 3, 7):                                   # 25 = 8 x 3 + 1 = 3 x 7 + 4: the last batch is a ragged one
        assert hipops.region_batch_columns(index.n_cells, 12 * index.n_cells * columns) == columns
        for two_pass in (False, True):
            part = arrays(hipops.overlap_table(d_a, d_b, index, pair_bytes=12 * index.n_cells * columns, two_pass=two_pass))
            tc.check_overlap(part, ref, f"{name} batches of {columns}")
            assert same(whole, part)


@guarded
def test_all_out_all_in_and_one_cell():
    index = index_of("uniform2d")
    out = dev(np.full((4096, 3), -1, dtype=np.int32))
    name, _, full = tc.motion("full")
    d_full = dev(full)
    for a, b in ((out, out), (out, d_full[:, :3]), (d_full[:, :3], out)):
        got = arrays(hipops.overlap_table(a, b, index))
        assert got["offsets"].tolist() == [0, 0, 0, 0] and all(len(got[k]) == 0 for k in hipops.OVERLAP_FIELDS)
        assert got["src"].dtype == np.int32 and got["units"].dtype == np.int64 and got["volume"].dtype == np.float64
    ref = tc.reference_overlap(name, full[:, :-1], full[:, 1:])
    assert (ref["n_cells"] > 1024).all()                       # one edge per column, all 4096 cells in it
    for two_pass in (False, True):
        tc.check_overlap(arrays(hipops.overlap_table(d_full[:, :-1], d_full[:, 1:], index, two_pass=two_pass)), ref, "all in")
    mixed = np.stack([full[:, 0], np.full(4096, -1, dtype=np.int32), full[:, 0]], axis=1)      # an empty column between two full ones
    tc.check_overlap(arrays(hipops.overlap_table(dev(mixed), dev(mixed), index)), tc.reference_overlap(name, mixed, mixed), "mixed")
    for lab in (np.zeros((1, 4), dtype=np.int32), np.array([[0, -1, 0, -1]], dtype=np.int32)):
        ref = tc.reference_overlap("one_cell", lab, lab[:, ::-1])
        tc.check_overlap(arrays(hipops.overlap_table(dev(lab), dev(np.ascontiguousarray(lab[:, ::-1])), index_of("one_cell"))), ref, "one_cell")
    vec = arrays(hipops.overlap_table(d_full[:, 0].contiguous(), d_full[:, 1].contiguous(), index))           # [n]: one column
    tc.check_overlap(vec, tc.reference_overlap(name, full[:, :1], full[:, 1:2]), "vectors")


@pytest.mark.parametrize("name", rc.TREES)
@guarded
def test_a_label_that_names_no_root_is_out(name):
    a, b, ref = random_pair(name)
    planted = tc.plant_non_root(a, b)
    by_rule = tc.reference_overlap(name, planted, b)
    assert by_rule["n_cells"].sum() == ref["n_cells"].sum() - 1
    for two_pass in (False, True):
        tc.check_overlap(arrays(hipops.overlap_table(dev(planted), dev(b), index_of(name), two_pass=two_pass)), by_rule, f"{name} planted")
    tc.check_overlap(arrays(hipops.overlap_table(dev(b), dev(planted), index_of(name))), tc.reference_overlap(name, b, planted), f"{name} planted in b")
    assert tc.reference_overlap(name, b, planted)["n_cells"].sum() == ref["n_cells"].sum() - 1


@guarded
def test_refusals():
    index = index_of("one_cell")
    lab = dev(np.zeros((1, 2), dtype=np.int32))
    grid, p = C.byref(index.s3_grid()), C.c_void_p(lab.data_ptr())
    lib = _lib.hip_lib()
    assert lib.s3_overlap_count(grid, p, 0, p, 0, (1 << 31) - 1, p, hipops._stream()) == -1          # n_cells * row_len >= 2^31 - 1, before any launch
    assert b"split the batch" in lib.s3_last_error()
    assert lib.s3_overlap_count(grid, p, 1, p, 0, 2, p, hipops._stream()) == -1                      # a pitch shorter than a row
    assert lib.s3_overlap_emit(grid, p, 0, p, 0, 2, p, 2, 3, p, p, hipops._stream()) == -1           # no such pass
    with pytest.raises(ValueError):
        hipops.overlap_table(lab, dev(np.zeros((1, 3), dtype=np.int32)), index)
    with pytest.raises(TypeError):
        hipops.overlap_table(lab.to(pt.int64), lab, index)
    with pytest.raises(TypeError):
        hipops.overlap_table(lab.cpu(), lab, index)
    with pytest.raises(ValueError):
        hipops.overlap_emit(lab, lab, index, None, pt.empty(2, dtype=pt.int64, device="cuda"), pt.empty(2, dtype=pt.int32, device="cuda"), "by_a")


# ---- the front-end --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def regions_of(name):
    c = rc.grid(name)
    return Regions(c["centers"], c["levels"], c["width"])


@pytest.mark.parametrize("name", rc.TREES)
@guarded
def test_regions_overlap_on_both_sides(name):
    a, b, ref = random_pair(name)
    regions = regions_of(name)
    host = regions.overlap(a, b)
    assert isinstance(host, OverlapTable) and isinstance(host.src, np.ndarray) and len(host) == len(ref["src"]) and host.n_columns == a.shape[1]
    tc.check_overlap({"offsets": host.offsets, **{k: getattr(host, k) for k in host.FIELDS}}, ref, name)
    there = regions.overlap(dev(a), dev(b))
    assert there.src.is_cuda and np.array_equal(there.n_edges, np.diff(ref["offsets"]))
    tc.check_overlap({"offsets": there.offsets, **{k: getattr(there, k).cpu().numpy() for k in there.FIELDS}}, ref, name)
    t = a.shape[1] - 1
    assert np.array_equal(host.of_column(t)["dst"], ref["dst"][ref["offsets"][t]:])
    with pytest.raises(ValueError):
        regions.overlap(dev(a).t().contiguous().t(), dev(b))     # rows that cannot be read where they lie


@pytest.mark.parametrize("kind", tc.MOTIONS + tc.TREE_MOTIONS)
@guarded
def test_label_then_track_equals_the_reference(kind):
    name, mask, ref_labels = tc.motion(kind)
    regions = regions_of(name)
    labels = regions.label(dev(mask))                           # on the device: the windows of the tracking are read where they lie
    rc.check_labels(labels.cpu().numpy(), ref_labels, kind)
    tracks = regions.track(labels)
    assert isinstance(tracks, RegionTracks) and isinstance(tracks.table, RegionTable) and tracks.track.is_cuda and tracks.edges.src.is_cuda
    ref_edges = tc.reference_overlap(name, ref_labels[:, :-1], ref_labels[:, 1:])
    tc.check_overlap({"offsets": tracks.edges.offsets, **{k: getattr(tracks.edges, k).cpu().numpy() for k in OverlapTable.FIELDS}}, ref_edges, kind)
    dt = 0.125
    for min_volume in (0.0, float(ref_edges["volume"].min()) * 1.5):
        got = regions.track(labels, table=tracks.table, min_volume=min_volume)
        ref = tc.reference_tracks(name, ref_labels, tracks.table.centroid.cpu().numpy(), dt, min_volume)
        tc.check_tracks(tc.tracks_as_dict(got, dt), ref, f"{kind} min_volume={min_volume}")
    host = regions.track(ref_labels)                            # numpy in, numpy out
    assert isinstance(host.track, np.ndarray) and isinstance(host.velocity(dt), np.ndarray) and isinstance(host.table.centroid, np.ndarray)
    tc.check_tracks(tc.tracks_as_dict(host, dt), tc.reference_tracks(name, ref_labels, host.table.centroid, dt), f"{kind} host")
    if kind == "moving":                                        # one cell per snapshot along x, h = width / 64
        h = rc.grid(name)["width"] / 64
        v = host.velocity(dt)
        assert np.isnan(v[0]).all() and np.allclose(v[1:], [[h / dt, 0.0]] * (tc.T_MOTION - 1), rtol=1e-12, atol=1e-15)


@guarded
def test_a_single_snapshot_has_no_edges():
    name, _, labels = tc.motion("scene")
    regions = regions_of(name)
    for lab in (labels[:, :1], labels[:, 0], dev(labels[:, :1])):
        tracks = regions.track(lab)
        n = len(tracks.table)
        assert n == 5 and len(tracks) == n and len(tracks.edges) == 0 and tracks.edges.offsets.tolist() == [0]
        track = tracks.track if isinstance(tracks.track, np.ndarray) else tracks.track.cpu().numpy()
        assert track.tolist() == list(range(n))
        born = tracks.born if isinstance(tracks.born, np.ndarray) else tracks.born.cpu().numpy()
        assert not born.any()
