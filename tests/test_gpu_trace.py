"""
The particle tracer on the GPU (csrc/trace.hip, sparsespatialsampling_amd/tracing.py) against the references of tests/trace_cases.py.

What is asserted (no figure comes from the code under test; the two bounds are derived in tests/trace_cases.py and held by the CPU
emulation with an eighth of the room, tests/test_trace_checker.py):
  affine fields     positions within K_AFFINE * r * u * max|x| * exp(||A|| * sum |dt|) of the long-double RK4 on the analytic field, both
                    step rules, both directions; lengths and statuses EQUAL the oracle's for every particle whose oracle path keeps
                    1e-6 cell sizes away from every face (the rest is capped at 1 % on the CPU side); every = 5 is every fifth row
  exact case        dyadic grids, a constant power-of-two velocity: positions bit for bit, lengths and statuses as the integer
                    prediction, particles ON faces (upper cell) and on the upper bound of the domain (no cell) among them
  random fields     one step within ONE_STEP_MARGIN * B of the long-double blend, fp32 and f64 storage
  identities        bit for bit: N steps = N chained calls of one step (so the same-cell shortcut never changes an answer); no
                    dependence on T_b, the order of the seeds, a launch-order list, `every`, fp32 storage against its f64 copy, the run
  pathlines         affine in space and linear in time within the affine bound; a field constant in time gives the time-rule
                    streamline bit for bit; backward from the forward end returns to the seed within twice the bound, at a step
                    where RK4 retraces itself (``trace_cases.round_trip_dt``) -- and meets the backward oracle at the ordinary step
  hostile input     NaN / inf / 1e300 seeds, a NaN node value, corner ids outside the field, guard zones round every output

Shapes: 3001 seeds (twelve workgroups of 256, the last one ragged), T_b in {1, 3, 25}, at most 24 steps.
"""
import numpy as np
import pytest
import torch as pt

from tests import sample_cases as sc
from tests import trace_cases as tc
from tests.interp_accuracy import GUARD_BITS, assert_guard
from sparsespatialsampling_amd import hipops
from sparsespatialsampling_amd.sampling import Probe
from sparsespatialsampling_amd.tracing import Paths, Tracer

pytestmark = pytest.mark.gpu

LD = tc.LD
GUARD = 512
NS = tc.NS
PERM = np.random.default_rng(77).permutation(NS).astype(np.int32)
_GRID = {}


def dev(a):
    return pt.from_numpy(np.ascontiguousarray(a)).cuda()


def on_device(name):
    """(CellIndex, faces) of a case, built once"""
    if name not in _GRID:
        c = sc.case(name)
        _GRID[name] = (hipops.cell_index(dev(c["centers"]), dev(c["levels"]), c["width"]), dev(c["faces"]))
    return _GRID[name]


def guarded(shape, dtype):
    """an output inside an allocation with guard zones on both sides -> (the allocation as int64, the output)"""
    item = pt.empty(0, dtype=dtype).element_size()
    words = (int(np.prod(shape)) * item + 7) // 8
    buf = pt.full((GUARD + words + GUARD,), int(GUARD_BITS), dtype=pt.int64, device="cuda")
    out = buf[GUARD:GUARD + words].view(dtype)[:int(np.prod(shape))].view(shape)
    return buf, out, words


def trace(name, field, seeds, path=False, faces=None, **kw):
    """``hipops.trace_stream`` / ``trace_path`` into guarded outputs -> numpy (points, length, status, cells)"""
    index, dev_faces = on_device(name)
    field = field if isinstance(field, pt.Tensor) else dev(field)
    seeds = seeds if isinstance(seeds, pt.Tensor) else dev(seeds)
    n, d, t = int(seeds.shape[0]), index.dim, int(field.shape[2])
    lead = (n,) if path else (n, t)
    n_out = t if path else 1 + kw["n_steps"] // kw.get("every", 1)
    bufs = [guarded(lead + (n_out, d), pt.float64)] + [guarded(lead, pt.int32) for _ in range(3)]
    outs = dict(zip(("paths", "length", "status", "cells"), (b[1] for b in bufs)))
    fn = hipops.trace_path if path else hipops.trace_stream
    res = fn(index, dev_faces if faces is None else faces, field, seeds, **kw, **outs)
    assert all(r is o for r, o in zip(res, outs.values()))
    pt.cuda.synchronize()
    for (buf, _, words), what in zip(bufs, outs):
        bits = buf.cpu().numpy()
        if int(np.prod(lead)) % 2 and what != "paths":                          # (an odd count of int32: the upper half of the last word is guard too)
            assert bits[GUARD + words - 1] >> 32 == int(GUARD_BITS) >> 32, what
        assert_guard(bits, GUARD, GUARD + words, f"{name} {what}")
    return tuple(r.cpu().numpy() for r in res)


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def rule_kw(rule, step):
    return {"step": rule, "cfl": step} if rule == "cell" else {"step": rule, "dt": step}


def assert_rows(points, length, n_out):
    """rows before the length are finite, rows after it NaN"""
    valid = np.arange(n_out)[None] < length.reshape(-1, 1)
    flat = points.reshape(-1, n_out, points.shape[-1])
    assert np.isfinite(flat[valid]).all() and np.isnan(flat[~valid]).all()


# ---- affine fields ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("run", range(len(tc.AFFINE_RUNS)), ids=[f"{r[0]}-{r[1]}" for r in tc.AFFINE_RUNS])
def test_affine_streamlines(run, direction):
    name, rule, step, n_steps = tc.AFFINE_RUNS[run]
    g = tc.grid(name)
    ref = tc.affine_reference(run, direction)
    sure = ref["sure"]
    assert 1 - sure.mean() <= tc.EXCLUDED_CAP
    field = tc.Affine(g).nodes(g)[:, :, None]
    points, length, status, cells = trace(name, field, tc.seeds(name), n_steps=n_steps, direction=direction, **rule_kw(rule, step))
    points, length, status = points[:, 0], length[:, 0], status[:, 0]
    assert_rows(points, length, n_steps + 1)
    assert np.array_equal(length[sure], ref["length"][sure]) and np.array_equal(status[sure], ref["status"][sure])
    k = tc.violation(points[sure], ref["points"][sure], ref["bound"][sure])
    print(f"{name} {rule} {direction:+d}: K needed {k:.3f} of {tc.K_AFFINE}")
    assert k <= tc.K_AFFINE
    # the cell of the last position
    last = points[np.arange(NS), np.maximum(length - 1, 0)]
    ids = sc.brute_force(g.c, np.nan_to_num(last))[0]
    assert np.array_equal(cells[:, 0][sure], np.where(length > 0, ids, -1)[sure])
    # every fifth accepted step
    if direction == 1:
        p5, l5, s5, c5 = trace(name, field, tc.seeds(name), n_steps=n_steps, direction=1, every=5, **rule_kw(rule, step))
        assert p5.shape[2] == 1 + n_steps // 5
        want = points[:, ::5][:, :p5.shape[2]].copy()
        want[np.arange(want.shape[1])[None] >= tc.recorded(length, 5)[:, None]] = np.nan
        assert np.array_equal(p5[:, 0], want, equal_nan=True) and np.array_equal(l5[:, 0], tc.recorded(length, 5))
        assert np.array_equal(s5[:, 0], status)


# ---- the exact case --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["time", "cell"])
@pytest.mark.parametrize("name", ["dyadic2d", "dyadic3d"])
def test_exact_on_dyadic_grids(name, rule):
    ex = tc.exact_case(name)
    want_points, want_length, want_status = ex[rule]
    on_face = (ex["seeds"] * 2.0 ** int(sc.case(name)["levels"].max()) % 1 == 0).all(axis=1)
    assert (on_face & (want_length > 1)).sum() > 50 and ((want_status == tc.LEFT) & (want_length > 1)).sum() > 50
    points, length, status, _ = trace(name, ex["field"], ex["seeds"], n_steps=ex["n_steps"],
                                      **rule_kw(rule, ex["dt"] if rule == "time" else ex["cfl"]))
    assert np.array_equal(length[:, 0], want_length) and np.array_equal(status[:, 0], want_status)
    assert np.array_equal(points[:, 0], want_points, equal_nan=True)


# ---- random node fields, one step ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("rule", ["cell", "time"])
@pytest.mark.parametrize("name", tc.GRIDS)
def test_one_step_on_random_fields(name, rule, f32):
    field, step, ref = tc.one_step_reference(name, rule, f32)
    near = ref["ok"] & (ref["margin"] <= tc.FACE_MARGIN)
    sure = ref["ok"] & ~near
    assert near.sum() <= tc.EXCLUDED_CAP * NS
    points, length, status, _ = trace(name, field[:, :, None], tc.seeds(name), n_steps=1, **rule_kw(rule, step))
    assert (length[sure, 0] == 2).all() and (status[sure, 0] == tc.DONE).all()
    ratio = float((np.abs(points[sure, 0, 1].astype(LD) - ref["end"][sure]) / ref["bound"][sure]).max())
    print(f"{name} {rule} {'f32' if f32 else 'f64'}: largest error / B {ratio:.3f} of {tc.ONE_STEP_MARGIN}")
    assert ratio <= tc.ONE_STEP_MARGIN


# ---- identities, bit for bit -----------------------------------------------------------------------------------------------------------
def identity_setup(name, t, f32=True):
    g = tc.grid(name)
    field = tc.random_nodes(g, 21, f32, n_snapshots=t)
    return g, field, tc.seeds(name)


@pytest.mark.parametrize("rule", ["cell", "time"])
@pytest.mark.parametrize("name", ["tree2d", "tree3d", "offset2d"])
def test_n_steps_are_n_chained_steps(name, rule):
    g, field, x = identity_setup(name, 1)
    step = 0.3 if rule == "cell" else 1.5 * float(np.median(g.h))
    n = 8
    points, length, status, cells = trace(name, field, x, n_steps=n, **rule_kw(rule, step))
    assert (length[:, 0] == n + 1).mean() > 0.05 and (status[:, 0] == tc.LEFT).mean() > 0.05
    dfield, cur = dev(field), dev(x)
    for s in range(n):
        p1, l1, s1, c1 = trace(name, dfield, cur, n_steps=1, **rule_kw(rule, step))
        assert np.array_equal(p1[:, 0, 1], points[:, 0, s + 1], equal_nan=True), f"step {s}"
        assert np.array_equal(p1[:, 0, 0], points[:, 0, s], equal_nan=True)
        at_end = length[:, 0] == s + 1                                          # the particles whose last row is row s: this step ends them
        assert np.array_equal(s1[at_end, 0], status[at_end, 0]) and np.array_equal(c1[at_end, 0], cells[at_end, 0])
        cur = dev(p1[:, 0, 1])


@pytest.mark.parametrize("name", ["tree2d", "tree3d"])
def test_results_do_not_depend_on_the_launch(name):
    g, field, x = identity_setup(name, 25)
    kw = dict(n_steps=12, step="cell", cfl=0.4)
    dfield = dev(field)
    base = trace(name, dfield, x, **kw)
    assert_rows(base[0], base[1], 13)
    assert same(base, trace(name, dfield, x, **kw)), "the run"
    # T_b: a column passed alone, three columns
    for t in (0, 7, 24):
        one = trace(name, np.ascontiguousarray(field[:, :, t:t + 1]), x, **kw)
        assert same([b[:, t] for b in base], [o[:, 0] for o in one]), f"column {t} alone"
    three = trace(name, np.ascontiguousarray(field[:, :, 3:6]), x, **kw)
    assert same([b[:, 3:6] for b in base], three), "three columns"
    # the order of the seeds, and a launch-order list
    shuffled = trace(name, dfield, x[PERM], **kw)
    assert same([b[PERM] for b in base], shuffled), "the order of the seeds"
    assert same(base, trace(name, dfield, x, order=dev(PERM), **kw)), "a launch-order list"
    # fp32 storage against the same values widened
    assert same(base, trace(name, field.astype(np.float64), x, **kw)), "f32 against its f64 copy"
    # every
    p4, l4, s4, c4 = trace(name, dfield, x, every=4, **kw)
    assert np.array_equal(l4, tc.recorded(base[1], 4)) and np.array_equal(s4, base[2]) and np.array_equal(c4, base[3])
    want = base[0][:, :, ::4].copy()
    want[np.arange(4)[None, None] >= l4[:, :, None]] = np.nan
    assert np.array_equal(p4, want, equal_nan=True), "every"
    # backward is another trace, and forward again from nowhere else than the definition: both directions differ
    back = trace(name, dfield, x, direction=-1, **kw)
    assert not np.array_equal(back[0][:, :, 1], base[0][:, :, 1], equal_nan=True)


def test_velocity_is_what_the_probe_samples():
    """the velocity a particle sees is not an output; its zero is: under the cell rule a particle is STAGNANT exactly where
    ``Probe.sample(velocity, "linear")`` is zero in every component"""
    name = "tree2d"
    g = tc.grid(name)
    field = tc.random_nodes(g, 3, True, n_snapshots=1)
    dead = np.unique(g.c["faces"][::7])                                         # every corner of a seventh of the cells: zero velocity there
    field[dead] = 0.0
    x = tc.seeds(name)
    _, length, status, _ = trace(name, field, x, n_steps=1, step="cell", cfl=0.3)
    probe = Probe(g.c["centers"], g.c["levels"], g.c["width"], x, nodes=g.c["nodes"], faces=g.c["faces"])
    v = probe.sample(field, mode="linear")[:, :, 0]
    zero = (v == 0).all(axis=1)
    assert zero.sum() > 100
    assert np.array_equal(status[:, 0] == tc.STAGNANT, zero) and (length[zero, 0] == 1).all()


# ---- pathlines -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("run", range(len(tc.PATH_RUNS)), ids=[r[0] for r in tc.PATH_RUNS])
def test_affine_pathlines(run, direction):
    name, n_snap, substeps = tc.PATH_RUNS[run]
    g = tc.grid(name)
    ref = tc.path_reference(run, direction)
    sure = ref["sure"]
    assert 1 - sure.mean() <= tc.EXCLUDED_CAP
    field = tc.path_field(run).nodes(g, n_snap)
    points, length, status, _ = trace(name, field, tc.seeds(name), path=True, dt_snapshot=ref["dt_snapshot"], substeps=substeps,
                                      direction=direction, order=dev(PERM))
    assert_rows(points[:, ::direction], length, n_snap)
    assert np.array_equal(length[sure], ref["rows"][sure]) and np.array_equal(status[sure], ref["status"][sure])
    k = tc.violation(points[sure], ref["points"][sure], ref["bound"][sure])
    print(f"{name} {direction:+d}: K needed {k:.3f} of {tc.K_AFFINE}")
    assert k <= tc.K_AFFINE


@pytest.mark.parametrize("run", [0, 1, 3])
def test_pathline_returns_to_its_seed(run):
    name, n_snap, substeps = tc.PATH_RUNS[run]
    g = tc.grid(name)
    field = dev(tc.path_field(run).nodes(g, n_snap))
    for dt_snapshot, against_seed in ((tc.round_trip_dt(run), True), (tc.path_dt(g), False)):
        kw = dict(path=True, dt_snapshot=dt_snapshot, substeps=substeps)
        fwd = trace(name, field, tc.seeds(name), direction=1, **kw)
        done = (fwd[2] == tc.DONE) & (fwd[1] == n_snap)
        assert done.mean() > 0.05
        ends = fwd[0][done, -1]
        back = trace(name, field, ends, direction=-1, **kw)
        key = (name, against_seed)
        tc.STARTS[key] = ends
        ref = tc.path_reference(run, -1, dt_snapshot, key)
        sure = ref["sure"]
        assert np.array_equal(back[1][sure], ref["rows"][sure]) and np.array_equal(back[2][sure], ref["status"][sure])
        assert tc.violation(back[0][sure], ref["points"][sure], ref["bound"][sure]) <= tc.K_AFFINE
        if against_seed:
            home = sure & (back[2] == tc.DONE)
            assert home.sum() > 100
            err = np.abs(back[0][home, 0].astype(LD) - tc.seeds(name)[done][home].astype(LD)).max(axis=1)
            assert (err <= 2 * tc.K_AFFINE * ref["bound"][home, 0]).all()


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("name", ["tree2d", "tree3d"])
def test_steady_pathline_is_the_time_rule_streamline(name, direction):
    g = tc.grid(name)
    one = tc.random_nodes(g, 8, True)
    n_snap, substeps = 4, 3
    field = np.ascontiguousarray(np.repeat(one[:, :, None], n_snap, axis=2))
    dt_snapshot = 3.0 * float(np.median(g.h))
    path = trace(name, field, tc.seeds(name), path=True, dt_snapshot=dt_snapshot, substeps=substeps, direction=direction)
    line = trace(name, field[:, :, :1], tc.seeds(name), n_steps=(n_snap - 1) * substeps, step="time", dt=dt_snapshot / substeps,
                 every=substeps, direction=direction)
    assert (path[2] == tc.LEFT).mean() > 0.05 and (path[2] == tc.DONE).mean() > 0.05
    assert np.array_equal(path[0][:, ::direction], line[0][:, 0], equal_nan=True)
    assert same(path[1:], [a[:, 0] for a in line[1:]])


# ---- hostile input ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [False, True])
def test_hostile_seeds(path):
    name = "tree3d"
    g = tc.grid(name)
    x = tc.seeds(name)[:300].copy()
    bad = np.arange(0, 300, 5)
    for j, v in zip(bad, np.resize([np.nan, np.inf, -np.inf, 1e300, -1e300], len(bad))):
        x[j, j % 3] = v
    field = tc.random_nodes(g, 2, False, n_snapshots=3)
    kw = dict(path=True, dt_snapshot=0.01, substeps=2) if path else dict(n_steps=4, step="cell", cfl=0.3)
    points, length, status, cells = trace(name, field, x, **kw)
    assert (status[bad] == tc.SEED_OUTSIDE).all() and (length[bad] == 0).all() and (cells[bad] == -1).all()
    assert np.isnan(points[bad]).all()
    clean = trace(name, field, tc.seeds(name)[:300], **kw)
    rest = np.setdiff1d(np.arange(300), bad)
    assert same([a[rest] for a in (points, length, status, cells)], [a[rest] for a in clean])


@pytest.mark.parametrize("rule", ["cell", "time"])
def test_a_nan_node_ends_the_particles_that_touch_it(rule):
    name = "tree2d"
    g = tc.grid(name)
    field, step, ref = tc.one_step_reference(name, rule)
    node = int(np.bincount(g.c["faces"].ravel(), weights=np.repeat(g.h ** g.d, 1 << g.d)).argmax())     # the node with the most room round it
    poisoned = field.copy()
    poisoned[node, 1] = np.nan
    clean = trace(name, field[:, :, None], tc.seeds(name), n_steps=1, **rule_kw(rule, step))
    got = trace(name, poisoned[:, :, None], tc.seeds(name), n_steps=1, **rule_kw(rule, step))
    has_node = (g.c["faces"] == node).any(axis=1)
    sure = ref["margin"] > tc.FACE_MARGIN                                       # (particles that take the whole step in the reference)
    cells = ref["cells"]
    touched = has_node[np.maximum(cells[:, :4], 0)].any(axis=1)                # a velocity is taken at x, x2, x3, x4
    first = has_node[np.maximum(cells[:, 0], 0)]
    assert (sure & touched).sum() >= 5 and (sure & touched & ~first).sum() >= 1
    want = np.where(first & (rule == "cell"), tc.STAGNANT, tc.LEFT)
    sel = sure & touched
    assert np.array_equal(got[2][sel, 0], want[sel]) and (got[1][sel, 0] == 1).all()
    assert np.array_equal(got[0][sel, 0, 0], tc.seeds(name)[sel]) and np.isnan(got[0][sel, 0, 1]).all()
    keep = sure & ~touched
    assert same([a[keep] for a in got], [a[keep] for a in clean])


def test_corner_ids_outside_the_field_end_the_particle():
    name = "tree3d"
    g = tc.grid(name)
    field, step, ref = tc.one_step_reference(name, "time")
    cells = ref["cells"]
    sure = ref["margin"] > tc.FACE_MARGIN
    entered = cells[sure][:, 1:][cells[sure][:, 1:] != cells[sure][:, :1]]
    busy = np.bincount(entered, minlength=g.n_cells).argsort()[-2:]             # the two cells most particles enter during the step
    faces = g.c["faces"].copy()
    faces[busy[0], 3], faces[busy[1], 6] = g.n_nodes + 5, -2
    got = trace(name, field[:, :, None], tc.seeds(name), n_steps=1, step="time", dt=step, faces=dev(faces))
    clean = trace(name, field[:, :, None], tc.seeds(name), n_steps=1, step="time", dt=step)
    hit = np.isin(cells, busy)
    seed_in = sure & hit[:, 0]
    later = sure & ~hit[:, 0] & hit.any(axis=1)
    assert seed_in.sum() >= 1 and later.sum() >= 1
    assert (got[2][seed_in, 0] == tc.SEED_OUTSIDE).all() and (got[1][seed_in, 0] == 0).all() and np.isnan(got[0][seed_in]).all()
    assert (got[2][later, 0] == tc.LEFT).all() and (got[1][later, 0] == 1).all()
    keep = sure & ~hit.any(axis=1)
    assert same([a[keep] for a in got], [a[keep] for a in clean])


def test_wrappers_validate():
    name = "tree2d"
    g = tc.grid(name)
    index, faces = on_device(name)
    field, x = dev(tc.random_nodes(g, 1, True, n_snapshots=3)), dev(tc.seeds(name))
    ok = dict(n_steps=3, step="cell", cfl=0.5)
    with pytest.raises(TypeError):
        hipops.trace_stream(index, faces, field.cpu(), x, **ok)
    with pytest.raises(TypeError):
        hipops.trace_stream(index, faces.long(), field, x, **ok)
    with pytest.raises(TypeError):
        hipops.trace_stream(index, faces, field, x.float(), **ok)
    with pytest.raises(ValueError):
        hipops.trace_stream(index, faces, dev(tc.random_nodes(tc.grid("tree3d"), 1))[:g.n_nodes, :, None].contiguous(), x, **ok)
    for bad in (dict(n_steps=0), dict(every=0), dict(cfl=float("nan")), dict(cfl=-1.0), dict(step="time"), dict(step="time", dt=float("inf")),
                dict(step="euler"), dict(direction=0)):
        with pytest.raises(ValueError):
            hipops.trace_stream(index, faces, field, x, **{**ok, **bad})
    with pytest.raises(ValueError):
        hipops.trace_path(index, faces, field[:, :, :1].contiguous(), x, 0.1)
    with pytest.raises(ValueError):
        hipops.trace_path(index, faces, field, x, 0.1, substeps=0)
    with pytest.raises(TypeError):
        hipops.trace_path(index, faces, field, x, 0.1, order=dev(PERM).long())


# ---- end to end through the API --------------------------------------------------------------------------------------------------------
def test_tracer_sides_windows_and_both_directions():
    name = "golden2d"
    g = tc.grid(name)
    c = g.c
    field = tc.random_nodes(g, 12, True, n_snapshots=6)
    x = tc.seeds(name)[:500]
    kw = dict(n_steps=10, step="cell", cfl=0.4)
    want = trace(name, field, x, **kw)
    tracer = Tracer(c["centers"], c["levels"], c["width"], c["nodes"], c["faces"])
    # numpy in, numpy out
    res = tracer.streamlines(field, x, **kw)
    assert isinstance(res, Paths) and isinstance(res.points, np.ndarray) and res.points.shape == (500, 6, 11, 2)
    assert same((res.points, res.length, res.status, res.cell_ids), want) and not res.first.any()
    # torch on the host, a device field read where it lies, a window of it, one snapshot
    dfield = dev(field)
    host = tracer.streamlines(pt.from_numpy(field), pt.from_numpy(x), **kw)
    assert isinstance(host.points, pt.Tensor) and not host.points.is_cuda and np.array_equal(host.points.numpy(), want[0], equal_nan=True)
    on_dev = tracer.streamlines(dfield, dev(x), **kw)
    assert on_dev.points.is_cuda and on_dev.status.is_cuda and np.array_equal(on_dev.points.cpu().numpy(), want[0], equal_nan=True)
    window = tracer.streamlines(dfield[..., 2:5], x, **kw)
    assert np.array_equal(window.points, want[0][:, 2:5], equal_nan=True) and np.array_equal(window.length, want[1][:, 2:5])
    single = tracer.streamlines(field[:, :, 1].copy(), x, **kw)
    assert single.points.shape == (500, 11, 2) and np.array_equal(single.points, want[0][:, 1], equal_nan=True)
    assert single.status.shape == (500,)
    # both directions: the backward trace reversed, the seed once, the forward trace
    back = trace(name, field, x, direction=-1, **kw)
    both = tracer.streamlines(field, x, direction="both", **kw)
    assert both.points.shape == (500, 6, 21, 2) and both.status.shape == (500, 6, 2)
    assert np.array_equal(both.points[:, :, 10:], want[0], equal_nan=True)
    assert np.array_equal(both.points[:, :, :11], back[0][:, :, ::-1], equal_nan=True)
    assert np.array_equal(both.status[..., 0], back[2]) and np.array_equal(both.status[..., 1], want[2])
    assert np.array_equal(both.length, np.maximum(back[1] - 1, 0) + want[1]) and np.array_equal(both.first, 10 - np.maximum(back[1] - 1, 0))
    rows = np.arange(21)[None, None]
    valid = (rows >= both.first[..., None]) & (rows < (both.first + both.length)[..., None])
    assert np.isfinite(both.points[valid]).all() and np.isnan(both.points[~valid]).all()
    # pathlines, and colouring by another field: the x coordinate of the nodes comes back as the x of the points
    dt_snapshot = 0.5 * float(np.median(g.h))
    for direction in (1, -1):
        pw = trace(name, field, x, path=True, dt_snapshot=dt_snapshot, substeps=4, direction=direction)
        paths = tracer.pathlines(field, x, dt_snapshot, substeps=4, direction=direction)
        assert paths.points.shape == (500, 6, 2) and same((paths.points, paths.length, paths.status, paths.cell_ids), pw)
        assert np.array_equal(paths.first, np.zeros(500) if direction == 1 else 6 - pw[1])
    colour = res.sample(c["nodes"][:, :1].copy(), mode="linear")
    assert colour.shape == (500, 6, 11, 1)
    seen = ~np.isnan(res.points[..., 0])
    assert np.abs(colour[..., 0][seen] - res.points[..., 0][seen]).max() <= 64 * 2.0 ** -53 * g.max_x and np.isnan(colour[..., 0][~seen]).all()
    # refusals
    for call in (lambda: tracer.streamlines(field[:, :1], x, **kw), lambda: tracer.streamlines(field, x, n_steps=0),
                 lambda: tracer.streamlines(field, x, n_steps=3, every=0), lambda: tracer.streamlines(field, x, n_steps=3, cfl=float("nan")),
                 lambda: tracer.streamlines(field, x, n_steps=3, step="time"), lambda: tracer.streamlines(field, x, n_steps=3, step="time", dt=float("inf")),
                 lambda: tracer.streamlines(field, x, n_steps=3, direction=2), lambda: tracer.pathlines(field, x, 0.1, step="cell"),
                 lambda: tracer.pathlines(field[:, :, :1], x, 0.1), lambda: tracer.pathlines(field, x, 0.1, direction="both"),
                 lambda: tracer.pathlines(field, x, float("nan")), lambda: tracer.streamlines(field[:-1], x, **kw),
                 lambda: tracer.streamlines(field, x[:, :1], **kw)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        tracer.streamlines(field.tolist(), x, **kw)
    empty = tracer.streamlines(field, x[:0], **kw)
    assert empty.points.shape == (0, 6, 11, 2) and empty.length.shape == (0, 6)


def test_tracer_from_dataloader_and_s_cube(tmp_path):
    import types
    from sparsespatialsampling_amd.const import CENTERS, FACES, GRID, VERTICES
    from sparsespatialsampling_amd.data import Dataloader, Datawriter
    name = "offset2d"
    g = tc.grid(name)
    c = g.c
    writer = Datawriter(str(tmp_path), "grid.h5")
    for key, values in ((CENTERS, c["centers"]), (VERTICES, c["nodes"]), (FACES, c["faces"])):
        writer.write_data(key, group=GRID, data=pt.from_numpy(values))
    writer.write_data("levels", data=pt.from_numpy(c["levels"]).unsqueeze(-1))
    writer.write_data("size_initial_cell", data=pt.tensor(c["width"], dtype=pt.float64))
    writer.close()
    field = tc.random_nodes(g, 4, False, n_snapshots=3)
    x = tc.seeds(name)
    want = trace(name, field, x, n_steps=6, step="cell", cfl=0.5)
    res = Tracer.from_dataloader(Dataloader(str(tmp_path), "grid.h5")).streamlines(field, x, 6)
    assert same((res.points, res.length, res.status, res.cell_ids), want)
    s_cube = types.SimpleNamespace(centers=pt.from_numpy(c["centers"]), levels=pt.from_numpy(c["levels"]).long().unsqueeze(-1),
                                   size_initial_cell=c["width"], vertices=pt.from_numpy(c["nodes"]), faces=pt.from_numpy(c["faces"]))
    res = Tracer.from_s_cube(s_cube).streamlines(field, x, 6)
    assert same((res.points, res.length, res.status, res.cell_ids), want)
    with pytest.raises(ValueError, match="execute_grid_generation"):
        Tracer.from_s_cube(types.SimpleNamespace(centers=None))
