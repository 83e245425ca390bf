"""The entry points of include/s3overlap.h and ``Regions.track`` held to the stream they are given, with the harness of
tests/stream_cases.py (want / side / control; see there).  The cases are built here and never registered in ``sc.CASES``: that table
belongs to include/s3hip.h.  GPU only.

Poison: other valid label arrays of the same grid (the labellings of another random mask, or A and B exchanged), and for the later
launches of the chain the pairs, scans and heads that belong to those.  Every control must differ.
"""
import numpy as np
import pytest
import torch as pt

from tests import region_cases as rc
from tests import stream_cases as sc
from tests import track_cases as tc

pytestmark = pytest.mark.gpu

NAME, T_ROW = "tree2d", 3
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


@pytest.fixture(scope="module", autouse=True)
def device():
    from sparsespatialsampling_amd import hipops
    hipops.device()
    sc.sleep_cycles_per_ms()
    yield
    pt.cuda.synchronize()


def _index():
    g = rc.grid(NAME)
    ix = sc.ops().cell_index(sc.dev(g["centers"]), sc.dev(g["levels"]), g["width"])
    pt.cuda.synchronize()
    return ix


def _labels():
    """(a, b) real and (a, b) poison: four labellings, every one valid"""
    cut = lambda mask: np.ascontiguousarray(rc.labels_of(NAME, mask)[:, :T_ROW])          # noqa: E731
    return (cut("random0.5"), cut("random0.7")), (cut("random0.7")[:, ::-1].copy(), cut("random0.3"))


def _chain(a, b):
    """what the chain hands from launch to launch for the labels (a, b), on the host: the scanned flags [T * n + 1], the sorted pairs
    of the one-key route and the scanned heads [n_pairs + 1]"""
    n, n_t = a.shape
    both = (tc.is_in(a) & tc.is_in(b)).T                                                # snapshot-major
    scan = np.concatenate([[0], np.cumsum(both.reshape(-1))]).astype(np.int32)
    t, c = np.nonzero(both)
    w = sc.ops().overlap_key_bits(n, n_t)[0]
    keys = (t.astype(np.int64) << (2 * w)) | (a[c, t].astype(np.int64) << w) | b[c, t].astype(np.int64)
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], c[order].astype(np.int32)
    head = np.r_[True, keys[1:] != keys[:-1]] if len(keys) else np.zeros(0, dtype=bool)
    edge = np.concatenate([[0], np.cumsum(head)]).astype(np.int32)
    return scan, keys, vals, edge


CASES = {}


def case(name, *covers, may_refuse=False):
    def register(make):
        CASES[name] = sc.Case(name, covers, make, may_refuse=may_refuse)
        return make
    return register


@case("overlap_count", "s3_overlap_count")
def _():
    b = sc.Built()
    ix = _index()
    (ra, rb), (pa, pb) = _labels()
    a, lab_b = b.inp(ra, pa), b.inp(rb, pb)
    out = b.new((T_ROW * len(ra),), sc.I32)
    b.call = lambda: [sc.ops().overlap_count(a, lab_b, ix, out=out)]
    return b


def _emit(route):
    def make():
        b = sc.Built()
        ix = _index()
        (ra, rb), (pa, pb) = _labels()
        a, lab_b = b.inp(ra, pa), b.inp(rb, pb)
        real, poison = _chain(ra, rb), _chain(pa, pb)
        scan = b.inp(real[0], np.minimum(poison[0], real[0][-1]))          # (positions past the pair arrays are not written anyway)
        n_pairs = int(real[0][-1])
        keys, vals = b.new((n_pairs,), sc.I64), b.new((n_pairs,), sc.I32)
        b.call = lambda: list(sc.ops().overlap_emit(a, lab_b, ix, scan, keys, vals, route))
        return b
    return make


case("overlap_emit_one_key", "s3_overlap_emit")(_emit("one_key"))
case("overlap_emit_by_b", "s3_overlap_emit")(_emit("by_b"))


@case("overlap_emit_by_ta", "s3_overlap_emit")
def _():
    """the second pass: the keys are read and rewritten in place, their real content goes in late"""
    b = sc.Built()
    ix = _index()
    (ra, rb), (pa, pb) = _labels()
    a, lab_b = b.inp(ra, pa), b.inp(rb, pb)
    w = sc.ops().overlap_key_bits(len(ra), T_ROW)[0]

    def by_b(la, lb):                                                       # the pairs of the first pass, sorted by b
        both = (tc.is_in(la) & tc.is_in(lb)).T
        t, c = np.nonzero(both)
        order = np.argsort(lb[c, t], kind="stable")
        return ((t.astype(np.int64) << w) | lb[c, t].astype(np.int64))[order], c[order].astype(np.int32)
    (rk, rv), (pk, pv) = by_b(ra, rb), by_b(pa, pb)
    n = min(len(rk), len(pk))
    keys = b.out(pt.zeros(n, dtype=sc.I64, device="cuda"), init=(rk[:n], pk[:n]))
    vals = b.inp(rv[:n], pv[:n])
    b.call = lambda: list(sc.ops().overlap_emit(a, lab_b, ix, None, keys, vals, "by_ta"))
    return b


def _sorted_pairs(b):
    """the sorted pairs and scanned heads of (a, b) as inputs; poison: those of (b, a), as many pairs and edges"""
    (ra, rb), _ = _labels()
    real, poison = _chain(ra, rb), _chain(rb, ra)
    assert len(real[1]) == len(poison[1]) and real[3][-1] == poison[3][-1]
    return ra, rb, b.inp(real[1], poison[1]), b.inp(real[2], poison[2]), real[3], poison[3]


@case("overlap_heads", "s3_overlap_heads")
def _():
    b = sc.Built()
    ix = _index()
    ra, rb, keys, vals, _, _ = _sorted_pairs(b)
    lab_b = sc.dev(rb)
    head = b.new((len(keys),), sc.I32)
    b.call = lambda: [sc.ops().overlap_heads(keys, vals, ix, lab_b, out=head)]
    return b


@case("overlap_reduce", "s3_overlap_reduce")
def _():
    b = sc.Built()
    ix = _index()
    ra, rb, keys, vals, real_edge, poison_edge = _sorted_pairs(b)
    lab_b = sc.dev(rb)
    edge = b.inp(real_edge, poison_edge)
    b.call = lambda: [sc.ops().overlap_reduce(keys, vals, ix, lab_b, edge, int(real_edge[-1]))]
    return b


def _table(two_pass):
    def make():
        b = sc.Built()
        ix = _index()
        (ra, rb), (pa, pb) = _labels()
        a, lab_b = b.inp(ra, pa), b.inp(rb, pb)
        b.call = lambda: [sc.ops().overlap_table(a, lab_b, ix, two_pass=two_pass)]
        return b
    return make


CHAIN = ("s3_overlap_count", "s3_overlap_emit", "s3_overlap_heads", "s3_overlap_reduce", "s3_exclusive_scan", "s3_sort_pairs")
case("overlap_table_one_key", *CHAIN)(_table(False))
case("overlap_table_two_passes", *CHAIN)(_table(True))


# In the control the region table is made of the poison; its scans end with a release of scratch (hipFree: a wait for the whole device),
# so the overlap launches after it read the real labels: ``RegionTracks`` finds edge ends that are no rows of that table and says so.
@case("Regions.track", "Regions.track", may_refuse=True)
def _():
    from sparsespatialsampling_amd.regions import OverlapTable, Regions, RegionTable
    b = sc.Built()
    g = rc.grid(NAME)
    regions = Regions(sc.dev(g["centers"]), sc.dev(g["levels"]), g["width"])
    pt.cuda.synchronize()
    one = tc.columns(NAME, "random0.7", T_ROW + 1)
    labels = b.inp(one, np.ascontiguousarray(tc.columns(NAME, "random0.5", T_ROW + 1)[:, ::-1]))
    names = ("n_in", "n_out", "successor", "predecessor", "track", "born", "died", "merged", "split", "first", "length")

    def call():
        tracks = regions.track(labels)
        return [tracks.table.offsets, [getattr(tracks.table, k) for k in RegionTable.FIELDS[:6]], tracks.edges.offsets,
                [getattr(tracks.edges, k) for k in OverlapTable.FIELDS], [getattr(tracks, k) for k in names], tracks.velocity(0.5)]
    b.call = call
    return b


def test_every_entry_point_of_the_header_has_a_case():
    from sparsespatialsampling_amd import _lib
    covered = {entry for c in CASES.values() for entry in c.covers}
    assert set(_lib.OVERLAP_SIGNATURES) <= covered and "Regions.track" in covered
    assert not set(CASES) & (set(sc.CASES) | set(sc.SIDE_ONLY))


@pytest.mark.parametrize("name", list(CASES))
def test_entry_point_on_the_stream_it_is_given(name):
    rep = _guarded(lambda: sc.check_case(CASES[name]))
    print(f"{name}: side == want, control != want ({rep['n_bytes']} bytes in {rep['n_results']} results; call {rep['ms']:.2f} ms, "
          f"delay {rep['delay_ms']:.1f} ms, the control's call was done {rep['lead_ms']:.1f} ms before its end)")
    assert rep["side_equals_want"] and rep["control_differs"] and (CASES[name].may_refuse or not rep["refused"])
