"""Every streamed entry point of include/s3hip.h, and every front-end that chains them, held to the stream it is given
(tests/stream_cases.py has the harness and the table).  GPU only; one process, two side streams.

Each case runs on the default stream (``want``), under a side stream behind a device-side delay with late inputs and a late output
fill (``side``: must equal ``want`` bit for bit), and once more with the planted mistake, the call on the default stream while the
delay is pending (``control``: must differ, or the case proves nothing).

Delay: ``max(DELAY_FLOOR_MS, 4 x the warm default-stream wall time of the call)``, the time taken from the second run with a host
timer around call + synchronise.  Measured on an MI355X over the table and the front-ends (137 calls): median 0.10 ms.  Three calls
are long because of what the device or the host lanes have to do, and take four times their own time as the delay: knn_create_2d_refined
79 ms (10 000 copies of one point), to_host_large 38 ms (two downloads of 40 MiB), child_gain_reuse_parents_k49 24 ms (the per-lane
search on 48-fold duplicates).  Of the others the longest launch sequence is 3.2 ms (the two refined KNN queries; DMD 1.9 ms).
DELAY_FLOOR_MS is 10 ms, three times that and not that figure itself: a control that loses to one scheduling hiccup of the host
between queuing the delay and making the call would fail the suite, and the floor costs 20 ms a case.  With it the control's call
was done 9 ms or more before the end of the delay in every case whose call does not itself wait for the device (hipFree).
Sufficiency is enforced by the control of every case, not by these numbers.
"""
import numpy as np
import pytest
import torch as pt

from tests import stream_cases as sc

pytestmark = pytest.mark.gpu

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


@pytest.mark.parametrize("name", list(sc.CASES))
def test_entry_point_on_the_stream_it_is_given(name):
    rep = _guarded(lambda: sc.check_case(sc.CASES[name]))
    print(f"{name}: side == want, control != want ({rep['n_bytes']} bytes in {rep['n_results']} results; call {rep['ms']:.2f} ms, "
          f"delay {rep['delay_ms']:.1f} ms, the control's call was done {rep['lead_ms']:.1f} ms before its end"
          f"{', refused by its own checks' if rep['refused'] else ''})")
    assert rep["side_equals_want"] and rep["control_differs"] and (sc.CASES[name].may_refuse or not rep["refused"])


@pytest.mark.parametrize("name", list(sc.SIDE_ONLY))
def test_call_without_a_control_under_a_side_stream(name):
    """calls that wait for the whole device before their main launch: no planted mistake can show, the side run still must hold"""
    rep = _guarded(lambda: sc.check_case(sc.SIDE_ONLY[name]))
    print(f"{name}: side == want ({rep['n_bytes']} bytes in {rep['n_results']} results); no control: {sc.SIDE_ONLY[name].insensitive}")
    assert rep["side_equals_want"] and "control_differs" not in rep


def test_transfer_lanes_across_two_streams():
    """the pinned lane buffers of runtime.hip are shared by every call and stream: uploads queued on two streams, one of them behind
    a delay, and a download in between, all arrive"""
    def run():
        from sparsespatialsampling_amd import hipops
        rng = np.random.default_rng(11)
        a = pt.from_numpy(rng.standard_normal((3000, 25)).astype(np.float32))
        b = pt.from_numpy(rng.standard_normal((5000, 7)))
        ids = np.sort(rng.permutation(5000)[:777]).astype(np.int32)
        third = sc.dev(rng.standard_normal((257, 33)))
        big = pt.from_numpy(rng.standard_normal((9, 1 << 17)))                  # 9 MiB in 1-MiB rows: a lane wraps its two buffers
        pieces = pt.from_numpy(rng.standard_normal((1000, 2, 9)).astype(np.float32))
        d_a = pt.zeros((3000, 32), dtype=pt.float32, device="cuda")
        d_b = pt.zeros((777, 8), dtype=pt.float64, device="cuda")
        d_big = pt.zeros((9, 1 << 17), dtype=pt.float64, device="cuda")
        d_p = pt.zeros((1000, 8), dtype=pt.float32, device="cuda")
        pt.cuda.synchronize()
        s1, s2 = sc.side_stream(0), sc.side_stream(1)
        with pt.cuda.stream(s1):
            sc.delay(sc.DELAY_FLOOR_MS)
            hipops.upload_rows(a, d_a[:, :25])
        with pt.cuda.stream(s2):
            hipops.upload_rows_indexed(b, ids, d_b[:, :7])
            got_third = hipops.to_host(third)
            hipops.upload_rows(big, d_big)
        with pt.cuda.stream(s1):
            hipops.upload_row_pieces(pieces, None, 3, 7, d_p)
        s1.synchronize()
        s2.synchronize()
        assert pt.equal(d_a[:, :25].cpu(), a)
        assert pt.equal(d_b[:, :7].cpu(), b[pt.from_numpy(ids).long()])
        assert np.array_equal(got_third, third.cpu().numpy())
        assert pt.equal(d_big.cpu(), big)
        assert pt.equal(d_p.cpu(), pieces[:, :, 3:7].reshape(1000, 8))
    _guarded(run)


# ---- the front-ends: several kernels chained with torch temporaries --------------------------------------------------------------
# Each is constructed on the default stream and synchronised; the method runs under the side stream with late inputs and is compared
# with its default-stream result bit for bit (the harness of the table: want, side, control).  The shapes are the small grids and
# clouds of the table.
FRONT_ENDS = {}


def front_end(name, insensitive=""):
    def register(make):
        FRONT_ENDS[name] = sc.Case(name, (name,), make, insensitive=insensitive)
        return make
    return register


def _grid_inputs(name):
    g = sc._grid(name)
    return g, [sc.dev(g[k]) for k in ("centers", "levels")], g["width"], sc.dev(g["nodes"]), sc.dev(g["faces"])


def _attrs(obj, names):
    return [getattr(obj, n) for n in names]


@front_end("Probe.sample")
def _():
    from sparsespatialsampling_amd.sampling import Probe
    b, r = sc.Built(), sc.rng_of("probe")
    g, (c, lv), width, nodes, faces = _grid_inputs("tree2d")
    probe = Probe(c, lv, width, sc.dev(sc._queries(g, r, 777)), nodes=nodes, faces=faces)
    pt.cuda.synchronize()
    cells = b.inp(*sc._field(r, len(g["centers"]), 2, sc.F32))
    node_field = b.inp(*sc._field(r, len(g["nodes"]), 0, sc.F64))
    b.call = lambda: [probe.sample(cells, "cell"), probe.sample(node_field, "linear")]
    return b


@front_end("Regions.extract")
def _():
    from sparsespatialsampling_amd.regions import Regions, RegionTable
    b, r = sc.Built(), sc.rng_of("regions")
    g, (c, lv), width, _, _ = _grid_inputs("tree2d")
    regions = Regions(c, lv, width)
    real, poison, lo, hi = sc._region_fields("tree2d", "smooth32")
    pt.cuda.synchronize()
    field = b.inp(real, poison)
    weight = b.inp(*[r.standard_normal(real.shape) for _ in range(2)])
    b.call = lambda: [(t.offsets, _attrs(t, RegionTable.FIELDS)) for t in [regions.extract(field, lo, hi, weight=weight)]]
    return b


@front_end("Isosurface.extract")
def _():
    from sparsespatialsampling_amd.isosurface import Isosurface
    b, r = sc.Built(), sc.rng_of("isosurface")
    g, _, _, nodes, faces = _grid_inputs("tree3d")
    iso = Isosurface(nodes, faces)
    pt.cuda.synchronize()
    field = b.inp(*sc._node_field(g, r, sc.F32))
    b.call = lambda: [_attrs(iso.extract(field, 0.125), ("offsets", "vertices", "edges", "frac", "cells"))]
    return b


def _tracer(path):
    def make():
        from sparsespatialsampling_amd.tracing import Tracer
        b, r = sc.Built(), sc.rng_of(f"tracer{path}")
        g, (c, lv), width, nodes, faces = _grid_inputs("tree2d")
        tracer = Tracer(c, lv, width, nodes, faces)
        pt.cuda.synchronize()
        vel = b.inp(*sc._field(r, len(g["nodes"]), 2, sc.F64))
        seeds = b.inp(sc._seeds(g, r, 333), sc._seeds(g, r, 333))
        names = ("points", "first", "length", "status", "cell_ids")
        if path:
            b.call = lambda: [_attrs(tracer.pathlines(vel, seeds, 1e-3, substeps=2), names)]
        else:
            b.call = lambda: [_attrs(tracer.streamlines(vel, seeds, 6, every=2, direction="both"), names)]
        return b
    return make


front_end("Tracer.streamlines")(_tracer(False))
# pathlines launch the seeds in Hilbert order: ``hipops.spatial_order`` (tracing.py) comes first, and s3_spatial_order ends with the
# release of its scratch buffers (csrc/plan_build.hip, ``PermScratch tmp``; hipFree waits for the whole device) before the trace is
# launched.  The order itself does not change a bit of the result, so a control cannot differ: want and side alone.
front_end("Tracer.pathlines", insensitive="s3_spatial_order waits for the whole device before the trace is launched")(_tracer(True))


@front_end("Gradient")
def _():
    from sparsespatialsampling_amd.differential import Gradient
    b, r = sc.Built(), sc.rng_of("gradient")
    pts, _ = sc._stencils(2)
    grad = Gradient(sc.dev(pts))
    pt.cuda.synchronize()
    scalar = b.inp(*sc._field(r, len(pts), 0, sc.F32))
    u = b.inp(*sc._field(r, len(pts), 2, sc.F64))
    b.call = lambda: [grad.gradient(scalar), grad.vorticity(u), grad.q_criterion(u)]
    return b


@front_end("ReconstructionError.update")
def _():
    import copy
    from sparsespatialsampling_amd.metrics import RunningMoments
    from sparsespatialsampling_amd.reconstruction import ReconstructionError
    b, r = sc.Built(), sc.rng_of("reconstruction")
    base = ReconstructionError(sc.dev(r.random((300, 2))), sc.dev(r.random((1500, 2))), point_scale=sc.dev(r.random(1500) + 0.5))
    pt.cuda.synchronize()
    grid = b.inp(*sc._field(r, 300, 0, sc.F64))
    orig = b.inp(*sc._field(r, 1500, 0, sc.F32))

    def call():
        err = copy.copy(base)                               # the tables of ``base``, fresh sums
        err.n_snapshots, err._moments, err._sum_d, err._sum_ref = 0, RunningMoments(), [], []
        err.update(grid, orig)
        return [err.error_time, err.error_space_mean, err.error_space_std, err.error_total]
    b.call = call
    return b


@front_end("temporal_mean_std")
def _():
    from sparsespatialsampling_amd import metrics
    b, r = sc.Built(), sc.rng_of("metrics")
    x = b.inp(*[r.standard_normal((sc.N_ROWS, 2, sc.N_T)).astype(np.float32) for _ in range(2)])
    b.call = lambda: [metrics.temporal_mean(x), metrics.temporal_std(x), metrics.temporal_mean_abs_sum(x)]
    return b


def _snapshots(b, r, dtype):
    """[257, 33]: a few travelling waves and noise, so that the small eigenproblems are well separated"""
    out = []
    for _ in range(2):
        phase, t = r.random((sc.N_ROWS, 1)) * 6.28, np.arange(sc.N_T)[None]
        x = sum(a * np.sin(w * t + k * phase) for a, w, k in ((1.0, 0.3, 1.0), (0.5, 0.7, 2.0), (0.25, 1.1, 3.0)))
        out.append((x + 0.01 * r.standard_normal(x.shape)).astype(np.float32 if dtype == sc.F32 else np.float64))
    return b.inp(*out)


@front_end("compute_svd")
def _():
    from sparsespatialsampling_amd import svd
    b, r = sc.Built(), sc.rng_of("svd")
    x, area = _snapshots(b, r, sc.F64), b.inp(r.random(sc.N_ROWS) + 0.1, r.random(sc.N_ROWS) + 0.1)
    b.call = lambda: list(svd.compute_svd(x, area, 5))
    return b


@front_end("DMD")
def _():
    from sparsespatialsampling_amd.dmd import DMD
    b, r = sc.Built(), sc.rng_of("dmd")
    x, area = _snapshots(b, r, sc.F32), b.inp(r.random(sc.N_ROWS) + 0.1, r.random(sc.N_ROWS) + 0.1)
    b.call = lambda: [_attrs(DMD(x, 0.01, rank=6, cell_area=area), ("eigvals", "amplitude", "modes", "dynamics"))]
    return b


@front_end("welch_SPOD")
def _():
    from sparsespatialsampling_amd import spectral
    b, r = sc.Built(), sc.rng_of("spectral")
    x, area = _snapshots(b, r, sc.F32), b.inp(r.random(sc.N_ROWS) + 0.1, r.random(sc.N_ROWS) + 0.1)

    def call():
        model = spectral.SPOD(x, 0.01, 8, 3, cell_area=area)
        return list(spectral.welch(x, 0.01, nperseg=8, noverlap=3)) + [model.frequency, model.eigvals, model.modes(1, 2)]
    b.call = call
    return b


@pytest.mark.parametrize("name", list(FRONT_ENDS))
def test_front_end_under_a_side_stream(name):
    rep = _guarded(lambda: sc.check_case(FRONT_ENDS[name]))
    control = f"no control: {FRONT_ENDS[name].insensitive}" if FRONT_ENDS[name].insensitive else "control != want"
    print(f"{name}: side == want, {control} ({rep['n_bytes']} bytes in {rep['n_results']} results; call {rep['ms']:.2f} ms, "
          f"delay {rep['delay_ms']:.1f} ms)")
    assert rep["side_equals_want"] and (rep.get("control_differs", False) or bool(FRONT_ENDS[name].insensitive))
