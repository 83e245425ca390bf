"""The stream contract of include/s3hip.h as a tested property: the harness and the table of cases behind
tests/test_gpu_streams.py (GPU) and tests/test_stream_cases_table.py (CPU).

Every compute entry point takes an ``s3_stream`` and hipops hands it torch's current stream.  On the default stream a step queued on
the wrong stream is invisible, so a case is run twice:

want     real inputs, default stream, synchronised: the bytes every output must have.  A second run with the *poison* inputs must give
         other bytes (a case whose poison gives the same answer proves nothing).
side     the inputs hold the poison and the outputs an early pattern, written synchronously.  Then, all on one side stream: a
         device-side delay (``torch.cuda._sleep``), the copy of the real data into the inputs, the fill of every output buffer with the
         pattern the ``want`` run started from (read-modify-write outputs get their real initial content here), and the call.  After the
         stream is synchronised every output equals ``want`` bit for bit.  The delay makes a step that was queued on another stream run
         BEFORE its inputs arrive, or before the late output fill overwrites what it wrote: nothing is left to luck.
control  the planted mistake: the same preparation, but the call is made with the DEFAULT stream current while the delay is still
         pending on the side stream.  The outputs must differ from ``want`` -- read when the default stream is done (cases with device
         inputs: the call read the poison) and read again after the side stream is done (cases with caller-owned outputs: the late
         fill overwrote the call's result, which is what step 7 of the side run would have seen).  A delay that is too short shows up
         here and nowhere else: a control that equals ``want`` fails, it never skips.

Poison is always a VALID input of the call: ids, levels, neighbour tables and keys stay in range (another permutation, another table,
another mask), floats are finite unless the entry point documents NaN, and no buffer is ever read uninitialised -- whatever the
library does with its streams, nothing leaves an allocation.

``TABLE`` names the cases of every streamed entry point; ``NOT_CASES`` the few that have none, with the reason.  The CPU test holds
both against the header.
"""
import ctypes as C
import functools
import time

import numpy as np
import torch as pt

F32, F64, I32, I64, U8 = pt.float32, pt.float64, pt.int32, pt.int64, pt.uint8
FILL_LATE, FILL_EARLY = 0xA5, 0x3C          # the byte an output starts from in ``want`` (and gets late in ``side``); what it holds before
DELAY_FACTOR = 4                            # delay = max(DELAY_FLOOR_MS, DELAY_FACTOR x the warm default-stream time of the call)
DELAY_FLOOR_MS = 10.0                       # three times the longest host-side launch sequence of the table: see test_gpu_streams


def ops():
    from sparsespatialsampling_amd import hipops
    return hipops


def lib():
    from sparsespatialsampling_amd import _lib
    return _lib.hip_lib()


def dev(a, dtype=None):
    """host array -> device tensor, complete on return"""
    t = a if isinstance(a, pt.Tensor) else pt.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    t = t.cuda()
    pt.cuda.synchronize()
    return t


def raw_stream():
    return ops()._stream()


# ---- what a case is made of -----------------------------------------------------------------------------------------------------
class HostOut:
    """an output in page-locked host memory the device writes through (``s3_host_register``): filled on a stream by an asynchronous
    copy from a device pattern, read on the host"""

    def __init__(self, nbytes):
        self.array = np.zeros(nbytes + 4096, dtype=np.uint8)
        off = -self.array.ctypes.data % 4096
        self.array = self.array[off:off + nbytes]
        self.d_ptr = C.c_void_p(0)
        ops().check(lib().s3_host_register(C.c_void_p(self.array.ctypes.data), nbytes, C.byref(self.d_ptr)), "s3_host_register")
        self.patterns = {v: pt.full((nbytes,), v, dtype=U8, device="cuda") for v in (FILL_LATE, FILL_EARLY)}

    def fill(self, value):
        # device pattern -> the registered (page-locked) host bytes: one asynchronous copy on the current stream
        ops().check(lib().s3_memcpy_d2h(C.c_void_p(self.array.ctypes.data), C.c_void_p(self.patterns[value].data_ptr()),
                                         self.array.nbytes, raw_stream()), "s3_memcpy_d2h")

    def bytes(self):
        return self.array.tobytes()

    def close(self):
        lib().s3_host_unregister(C.c_void_p(self.array.ctypes.data))


class Built:
    """one case, built: the buffers the call reads (``inputs`` with their ``real`` and ``poison`` content on the device), the
    caller-owned buffers it writes (``outputs``; ``init``: (real, poison) initial content of a read-modify-write output, else a byte
    pattern; ``views``: the part of the buffer that is compared) and ``call``, which returns further results: device tensors the
    wrapper allocated, host arrays, numbers"""

    def __init__(self):
        self.inputs, self.real, self.poison = [], [], []
        self.outputs, self.init, self.views = [], [], []
        self.call, self.closers = None, []

    def inp(self, real, poison, dtype=None):
        real, poison = dev(real, dtype), dev(poison, dtype)
        assert real.shape == poison.shape and real.dtype == poison.dtype
        self.real.append(real), self.poison.append(poison)
        self.inputs.append(real.clone())
        return self.inputs[-1]

    def out(self, buf, init=None, view=None):
        if init is not None:
            init = tuple(dev(a, buf.dtype).reshape(buf.shape) for a in init)
        self.outputs.append(buf), self.init.append(init), self.views.append(buf if view is None else view)
        return buf

    def new(self, shape, dtype, init=None):
        return self.out(pt.zeros(shape, dtype=dtype, device="cuda"), init)

    def close(self):
        for f in self.closers:
            f()
        self.closers = []


def _set_inputs(b, poison):
    for buf, src in zip(b.inputs, b.poison if poison else b.real):
        buf.copy_(src, non_blocking=True)


def _fill_outputs(b, late):
    for o, init in zip(b.outputs, b.init):
        if isinstance(o, HostOut):
            o.fill(FILL_LATE if late else FILL_EARLY)
        elif init is not None:
            o.copy_(init[0] if late else init[1], non_blocking=True)
        else:
            o.view(-1).view(U8).fill_(FILL_LATE if late else FILL_EARLY)


def _bytes(x):
    if isinstance(x, pt.Tensor):
        return bytes(str(x.dtype), "ascii") + x.detach().contiguous().cpu().numpy().tobytes()
    if isinstance(x, HostOut):
        return x.bytes()
    if isinstance(x, np.ndarray):
        return bytes(str(x.dtype), "ascii") + np.ascontiguousarray(x).tobytes()
    if isinstance(x, dict):
        return b"".join(k.encode() + _bytes(v) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return b"".join(_bytes(v) for v in x)
    return repr(x).encode()


def _snapshot(b, results):
    return [_bytes(r) for r in (results or [])] + [_bytes(v) for v in b.views]


@functools.lru_cache(maxsize=None)
def sleep_cycles_per_ms():
    """``torch.cuda._sleep`` cycles per millisecond, measured once per process with two events"""
    e0, e1 = pt.cuda.Event(enable_timing=True), pt.cuda.Event(enable_timing=True)
    pt.cuda._sleep(1_000_000)
    pt.cuda.synchronize()
    cycles = 20_000_000
    e0.record()
    pt.cuda._sleep(cycles)
    e1.record()
    e1.synchronize()
    return cycles / max(e0.elapsed_time(e1), 1e-3)


_SIDE = []


def side_stream(i=0):
    """the two side streams of the process"""
    while len(_SIDE) <= i:
        assert len(_SIDE) < 2
        _SIDE.append(pt.cuda.Stream())
    return _SIDE[i]


def delay(ms):
    pt.cuda._sleep(int(ms * sleep_cycles_per_ms()))


def run_default(b, poison=False):
    _set_inputs(b, poison)
    _fill_outputs(b, True)
    pt.cuda.synchronize()
    t0 = time.perf_counter()
    results = b.call()
    pt.cuda.current_stream().synchronize()
    return _snapshot(b, results), (time.perf_counter() - t0) * 1e3


def _prepare_late(b, s, delay_ms):
    _set_inputs(b, True)
    _fill_outputs(b, False)
    pt.cuda.synchronize()
    with pt.cuda.stream(s):
        delay(delay_ms)
        _set_inputs(b, False)
        _fill_outputs(b, True)


def run_side(b, delay_ms):
    s = side_stream()
    _prepare_late(b, s, delay_ms)
    with pt.cuda.stream(s):
        results = b.call()
    s.synchronize()
    return _snapshot(b, results)


def run_control(b, delay_ms, may_refuse=False):
    """-> (lead_ms, early, late): the outputs read when the default stream is done, and again when the side stream is done;
    ``lead_ms``: how long before the end of the delay the default stream had finished the call's work (two events; negative: after it)"""
    from sparsespatialsampling_amd._lib import S3HipError
    s = side_stream()
    delay_end, call_end = pt.cuda.Event(enable_timing=True), pt.cuda.Event(enable_timing=True)
    _set_inputs(b, True)
    _fill_outputs(b, False)
    pt.cuda.synchronize()
    with pt.cuda.stream(s):
        delay(delay_ms)
        delay_end.record()
        _set_inputs(b, False)
        _fill_outputs(b, True)
    try:
        results = b.call()                              # the planted mistake: the default stream is current
    except (ValueError, S3HipError) as e:
        # The call's own argument checks refused what it read.  Poison and real data are each valid, so that can only happen to a call
        # whose first pass read the poison and whose later passes, after a hipFree of its own had waited for the side stream, read
        # the real data.  Only the cases that say so (``may_refuse``) may end here; there the refusal is a result like any other.
        if not may_refuse or (isinstance(e, S3HipError) and "code -1:" not in str(e)):
            raise
        results = [f"refused ({type(e).__name__})"]
    call_end.record()
    pt.cuda.current_stream().synchronize()
    early = _snapshot(b, results)
    s.synchronize()
    return call_end.elapsed_time(delay_end), early, _snapshot(b, results)


def check_case(case):
    """-> a report dict; raises AssertionError with what went wrong"""
    b = case.make()
    try:
        run_default(b)                                   # cold
        want, ms = run_default(b)                        # warm: the time behind the delay
        again, _ = run_default(b)
        assert again == want, f"{case.name}: two default-stream runs differ in results " \
                              f"{[i for i, (g, w) in enumerate(zip(again, want)) if g != w]}: the case is not deterministic"
        want_poison, _ = run_default(b, poison=True)
        if b.inputs:
            assert want_poison != want, f"{case.name}: the poison inputs give the same bytes as the real ones"
        delay_ms = max(DELAY_FLOOR_MS, DELAY_FACTOR * ms)
        got = run_side(b, delay_ms)
        wrong = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert len(got) == len(want) and not wrong, \
            f"{case.name}: under a side stream results {wrong} of {len(want)} differ from the default-stream run: a step of " \
            f"{', '.join(case.covers)} is not ordered on the stream it was given"
        report = dict(name=case.name, ms=ms, delay_ms=delay_ms, side_equals_want=True, n_results=len(want), n_bytes=sum(len(w) for w in want))
        if case.insensitive:
            return report
        lead_ms, early, late = run_control(b, delay_ms, case.may_refuse)
        seen = (bool(b.inputs) and early != want, bool(b.outputs) and late != want)
        assert (seen[0] or not b.inputs) and (seen[1] or not b.outputs) and any(seen), \
            f"{case.name}: delay too short or case insensitive: the control equals the default-stream run (read after the default " \
            f"stream: {'differs' if early != want else 'equal'}, {'equals' if early == want_poison else 'is not'} the poison run; read " \
            f"after the side stream: {'differs' if late != want else 'equal'}; the default stream was done {lead_ms:.2f} ms before the " \
            f"end of the {delay_ms:.1f} ms delay)"
        report.update(control_differs=True, lead_ms=lead_ms, refused=any(e.startswith(b"'refused") for e in early[:1]))
        return report
    finally:
        pt.cuda.synchronize()
        b.close()


class Case:
    def __init__(self, name, covers, make, note="", insensitive="", may_refuse=False):
        self.name, self.covers, self.make, self.note, self.insensitive = name, tuple(covers), make, note, insensitive
        self.may_refuse = may_refuse        # the control's call may be refused by its own argument checks: see run_control


CASES = {}          # the table's cases: want, side and control
SIDE_ONLY = {}      # want and side alone: calls whose control cannot differ (``insensitive``: why, with the source line); not in the table


def case(name, *covers, note="", insensitive="", may_refuse=False):
    def register(make):
        assert name not in CASES and name not in SIDE_ONLY, name
        (SIDE_ONLY if insensitive else CASES)[name] = Case(name, covers, make, note, insensitive, may_refuse)
        return make
    return register


def rng_of(name, salt=0):
    import zlib
    return np.random.default_rng(zlib.crc32(name.encode()) + salt)


# ---- interpolation ----------------------------------------------------------------------------------------------------------------
def _distances(rng, nc, k, zeros):
    d = np.sort(rng.random((nc, k)) + 1e-3, axis=1)
    if zeros:
        d[::7, 0] = 0.0
    return d


@case("idw_weights", "s3_idw_weights")
def _():
    b, r = Built(), rng_of("idw")
    d = b.inp(_distances(r, 257, 8, True), _distances(r, 257, 8, True))
    b.call = lambda: [ops().idw_weights(d)]
    return b


@case("idw_weights_exact", "s3_idw_weights_exact")
def _():
    b, r = Built(), rng_of("idwx")
    d = b.inp(_distances(r, 257, 26, True), _distances(r, 257, 26, True))
    b.call = lambda: [ops().idw_weights_exact(d)]
    return b


INTERP_GEOMS = {"g3_65": dict(d=3, n=400, nc=65),        # two tiles, the second with one cell: the smallest KNN table of
                "rand": dict(n=9_000, nc=1_037)}          # tests/test_gpu_interp_accuracy.py, and its arbitrary table (no centres)


@functools.lru_cache(maxsize=None)
def _interp_geometry(geom, k):
    """a neighbour table at the shapes of the interpolation's own accuracy test: -> (n_src, centers or None, idx int32, w).  ``g3_65``:
    the k nearest of 400 points to 65 cell centres with the export's weights (made on the device, default stream); ``rand``: ids in
    a band of 300 rows around each cell's base row, a repeated id per row, signed weights, zero weights and one-hot rows"""
    g = INTERP_GEOMS[geom]
    rng = rng_of(f"interp/{geom}/{k}")
    n, nc = g["n"], g["nc"]
    if geom == "rand":
        idx = ((np.arange(nc) * 8) % (n - 300))[:, None] + rng.integers(0, 300, (nc, k))
        if k >= 4:
            idx[:, 3] = idx[:, 2]
        w = rng.uniform(-1.0, 1.0, (nc, k))
        w[::7, 0] = 0.0
        w[::11] = 0.0
        w[::11, k - 1] = 1.0
        return n, None, idx.astype(np.int32), w
    pts, centers = rng.random((n, g["d"])), rng.random((nc, g["d"]))
    knn = ops().KnnIndex(pts)
    idx, dist = knn.query(centers, k)
    w = ops().idw_weights(dist).cpu().numpy()
    idx = idx.cpu().numpy()
    knn.close()
    return n, centers, idx.astype(np.int32), w


def _other_table(name, idx, n_src):
    """another valid neighbour table of the same shape: the ids reversed in the source range"""
    return (n_src - 1 - idx).astype(np.int32)


def _placed(host, layout, dtype):
    """``host`` [n, L] -> a device view laid out as ``layout`` ("dense"; "pitched": the pitch of ``padded_rows``; "offset16": dense rows
    starting 16 bytes off a 128-byte boundary) in an allocation whose other bytes are all 0xFF: nothing in it is uninitialised"""
    n, L = host.shape
    e = pt.empty((), dtype=dtype).element_size()
    pitch = ops().padded_rows(1, L, dtype, "cpu").stride(0) if layout == "pitched" else L
    lead = 256 + (16 if layout == "offset16" else 0)
    buf = pt.full((lead + n * pitch * e + 256,), 0xFF, dtype=U8, device="cuda")
    table = buf.view(dtype).as_strided((n, L), (pitch, 1), lead // e)
    table.copy_(pt.from_numpy(host).cuda())
    pt.cuda.synchronize()
    return table


def _values(geom, k, dtype, row_len, seed):
    """[n_src, row_len] finite rows whose size varies over six decades from row to row"""
    n = INTERP_GEOMS[geom]["n"]
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, row_len)) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    return x.astype(np.float32 if dtype == F32 else np.float64)


class _PlacedInput:
    """an input that is a strided view of a larger allocation (pitched rows, rows off the 16-byte grid)"""

    @staticmethod
    def add(b, real, poison, layout, dtype):
        view = _placed(real, layout, dtype)
        b.inputs.append(view), b.real.append(dev(real)), b.poison.append(dev(poison))
        return view


def _direct_interp(name, dtype, row_len):
    def make():
        b, r = Built(), rng_of(name)
        n_src, _, idx, w = _interp_geometry("g3_65", 26)
        d_w = b.inp(w, r.permutation(w.ravel()).reshape(w.shape))
        d_idx = b.inp(idx, _other_table(name, idx, n_src))
        data = b.inp(_values("g3_65", 26, dtype, row_len, 1), _values("g3_65", 26, dtype, row_len, 2))
        out = b.new((65, row_len), F64)
        b.call = lambda: [ops().interp(d_w, d_idx, data, out=out)]
        return b
    return make


case("interp_f32", "s3_interp")(_direct_interp("interp_f32", F32, 25))
case("interp_f64", "s3_interp")(_direct_interp("interp_f64", F64, 3))


# (name, geometry, k, dtype, row length, layout, entry, route): one route each of the persistent kernel, the shift kernel and the
# short-row kernels, at the smallest shapes tests/test_gpu_interp_accuracy.py drives them with
PLAN_ROUTES = [("plan_interp_stream", "g3_65", 26, F32, 75, "dense", "interp", "stream_elem"),
               ("plan_interp_shift", "g3_65", 26, F32, 20, "offset16", "interp", "shift"),
               ("plan_interp_short", "g3_65", 26, F32, 2, "pitched", "interp", "short_reg"),
               ("plan_src_stream", "g3_65", 26, F64, 9, "dense", "src", "stream_elem"),
               ("plan_src_short", "rand", 20, F64, 2, "dense", "src", "short_reg")]


def _plan(b, idx, n_src, centers):
    plan = ops().InterpPlan(dev(idx), n_src, None if centers is None else dev(centers))
    pt.cuda.synchronize()
    b.closers.append(plan.close)
    return plan


def _source_ids(n_src, n_table, seed):
    return np.sort(np.random.default_rng(seed).permutation(n_table)[:n_src]).astype(np.int32)


def _planned(name, geom, k, dtype, row_len, layout, entry, route):
    def make():
        b = Built()
        n_src, centers, idx, w = _interp_geometry(geom, k)
        nc = idx.shape[0]
        plan = _plan(b, idx, n_src, centers)
        d_w = dev(w)
        out = b.new((nc, row_len), F64)
        if entry == "interp":
            data = _PlacedInput.add(b, _values(geom, k, dtype, row_len, 1), _values(geom, k, dtype, row_len, 2), layout, dtype)
            assert plan.route(data)["route"] == route, (name, plan.route(data))
            plan.set_weights(d_w)
            b.call = lambda: [plan.interp(d_w, data, out=out)]
        else:
            n_table = n_src + 37
            ids = _source_ids(n_src, n_table, 5)
            full = [np.zeros((n_table, row_len), dtype=np.float32 if dtype == F32 else np.float64) for _ in range(2)]
            for seed, f in enumerate(full):
                f[:] = np.random.default_rng(seed).standard_normal(f.shape)
                f[ids] = _values(geom, k, dtype, row_len, 1 + seed)
            table = _PlacedInput.add(b, full[0], full[1], layout, dtype)
            plan.set_weights(d_w)
            plan.set_source_ids(dev(ids), n_table)
            assert plan.route(table, src=True)["route"] == route, (name, plan.route(table, src=True))
            b.call = lambda: [plan.interp_src(table, out=out)]
        pt.cuda.synchronize()
        return b
    return make


for _row in PLAN_ROUTES:
    case(_row[0], "s3_interp_planned" if _row[6] == "interp" else "s3_interp_planned_src")(_planned(*_row))


@case("plan_create", "s3_interp_plan_create")
def _():
    b = Built()
    n_src, centers, idx, w = _interp_geometry("g3_65", 26)
    d_idx = b.inp(idx, _other_table("plan_create", idx, n_src))
    d_ctr = b.inp(centers, centers[::-1].copy())
    d_w, data = dev(w), dev(_values("g3_65", 26, F32, 75, 1))
    plans = []
    b.closers.append(lambda: [p.close() for p in plans])

    def call():
        plans.append(ops().InterpPlan(d_idx, n_src, d_ctr))
        order, cuts = plans[-1].partition(3)
        return [plans[-1].n_tiles, plans[-1].total_rows, order, cuts, plans[-1].interp(d_w, data)]
    b.call = call
    return b


@case("plan_create_no_centers", "s3_interp_plan_create")
def _():
    b = Built()
    n_src, _, idx, w = _interp_geometry("rand", 5)
    d_idx = b.inp(idx, _other_table("plan_create_nc", idx, n_src))
    d_w, data = dev(w), dev(_values("rand", 5, F32, 16, 1))
    plans = []
    b.closers.append(lambda: [p.close() for p in plans])

    def call():
        plans.append(ops().InterpPlan(d_idx, n_src, None))
        return [plans[-1].n_tiles, plans[-1].total_rows, plans[-1].interp(d_w, data)]
    b.call = call
    return b


@case("plan_set_weights", "s3_interp_plan_set_weights")
def _():
    b, r = Built(), rng_of("set_weights")
    n_src, centers, idx, w = _interp_geometry("g3_65", 26)
    plan = _plan(b, idx, n_src, centers)
    d_w = b.inp(w, r.permutation(w.ravel()).reshape(w.shape))
    n_table = n_src + 37
    plan.set_source_ids(dev(_source_ids(n_src, n_table, 5)), n_table)
    table = dev(np.random.default_rng(3).standard_normal((n_table, 75)).astype(np.float32))
    out = b.new((65, 75), F64)

    def call():
        plan.set_weights(d_w)
        return [plan.interp_src(table, out=out)]
    b.call = call
    return b


@case("plan_set_source_ids", "s3_interp_plan_set_source_ids")
def _():
    b = Built()
    n_src, centers, idx, w = _interp_geometry("g3_65", 26)
    plan = _plan(b, idx, n_src, centers)
    n_table = n_src + 37
    ids = b.inp(_source_ids(n_src, n_table, 5), _source_ids(n_src, n_table, 6))
    plan.set_weights(dev(w))
    table = dev(np.random.default_rng(3).standard_normal((n_table, 75)).astype(np.float32))
    out = b.new((65, 75), F64)

    def call():
        plan.set_source_ids(ids, n_table)
        return [plan.interp_src(table, out=out)]
    b.call = call
    return b


@case("plan_partition", "s3_interp_plan_partition",
      note="the plan is the only input: the late fill of d_order is what a wrong-stream step would lose to")
def _():
    b = Built()
    n_src, centers, idx, _ = _interp_geometry("g3_65", 26)
    plan = _plan(b, idx, n_src, centers)
    order = b.new((65,), I32)

    def call():
        cuts = (C.c_int64 * 4)()
        ops().check(lib().s3_interp_plan_partition(plan._handle, 3, C.c_void_p(order.data_ptr()), cuts, raw_stream()), "s3_interp_plan_partition")
        return [[int(c) for c in cuts]]
    b.call = call
    return b


@case("plan_cost_profile", "s3_interp_plan_cost_profile", "s3_interp_plan_create",
      note="reads the plan's own tables and returns host values: the plan is built in the same call, on the same stream, from late inputs")
def _():
    b = Built()
    n_src, centers, idx, _ = _interp_geometry("g3_65", 26)
    d_idx = b.inp(idx, (idx // 3).astype(np.int32))                # fewer distinct rows per tile: another cost
    d_ctr = dev(centers)
    plans = []
    b.closers.append(lambda: [p.close() for p in plans])

    def call():
        plans.append(ops().InterpPlan(d_idx, n_src, d_ctr))
        return [plans[-1].cost_profile(8)]
    b.call = call
    return b


@case("yard_plan_loads", "s3_yard_plan_loads",
      note="a yardstick without a result on the device: the staged bytes it reports come from the plan, built in the same call from late inputs")
def _():
    b = Built()
    n_src, centers, idx, w = _interp_geometry("g3_65", 26)
    d_idx = b.inp(idx, (idx // 3).astype(np.int32))
    d_ctr = dev(centers)
    table = dev(np.random.default_rng(4).standard_normal((n_src + 8, 32)).astype(np.float32))     # (whole lines are loaded: rows to spare)
    plans = []
    b.closers.append(lambda: [p.close() for p in plans])

    def call():
        plans.append(ops().InterpPlan(d_idx, n_src, d_ctr))
        return [plans[-1].yard_loads(table, 0, in_place=False), plans[-1].total_rows]
    b.call = call
    return b


# ---- export plumbing --------------------------------------------------------------------------------------------------------------
def _snapshot_major(dtype):
    def make():
        b, r = Built(), rng_of("snapshot_major")
        v = b.inp(r.standard_normal((257, 2, 3)), r.standard_normal((257, 2, 3)))
        out = b.new((3, 257, 2), dtype)
        b.call = lambda: [ops().snapshot_major(v, 2, 3, out=out, dtype=dtype)]
        return b
    return make


case("snapshot_major", "s3_snapshot_major")(_snapshot_major(F64))
case("snapshot_major_as_f32", "s3_snapshot_major_as")(_snapshot_major(F32))


def _snapshot_major_rows(dtype):
    def make():
        b, r = Built(), rng_of("snapshot_major_rows")
        nc, n_out = 257, 300
        v = b.inp(r.standard_normal((nc, 2, 3)), r.standard_normal((nc, 2, 3)))
        rows = b.inp(np.sort(r.permutation(n_out)[:nc]).astype(np.int32), np.sort(r.permutation(n_out)[:nc]).astype(np.int32))
        host = HostOut(3 * n_out * 2 * (4 if dtype == F32 else 8))
        b.closers.append(host.close)
        b.out(host)
        b.call = lambda: ops().snapshot_major_rows(v, 2, 3, rows, n_out, host.d_ptr.value, dtype=dtype)
        return b
    return make


case("snapshot_major_rows", "s3_snapshot_major_rows")(_snapshot_major_rows(F64))
case("snapshot_major_rows_as_f32", "s3_snapshot_major_rows_as")(_snapshot_major_rows(F32))


def _cell_major(in_dtype, out_dtype):
    def make():
        b, r = Built(), rng_of("cell_major")
        npt = np.float32 if in_dtype == F32 else np.float64
        snaps = b.inp(r.standard_normal((3, 257, 2)).astype(npt), r.standard_normal((3, 257, 2)).astype(npt))
        out = b.new((257, 2, 5), out_dtype)
        b.call = lambda: [ops().cell_major(snaps, out, t0=1)]
        return b
    return make


case("cell_major_f32_f64", "s3_cell_major")(_cell_major(F32, F64))
case("cell_major_f64_f32", "s3_cell_major")(_cell_major(F64, F32))


def _gather_rows(with_ids):
    def make():
        b, r = Built(), rng_of("gather_rows")
        n = 129 if with_ids else 300
        src = b.inp(r.standard_normal((300, 7)).astype(np.float32), r.standard_normal((300, 7)).astype(np.float32))
        ids = b.inp(r.integers(0, 300, n).astype(np.int32), r.integers(0, 300, n).astype(np.int32)) if with_ids else None
        base = b.new((n, 8), F32)
        b.call = lambda: [ops().gather_rows(src, ids, base[:, :7])]
        b.views[-1] = base[:, :7]
        return b
    return make


case("gather_rows_ids", "s3_gather_rows",
     insensitive='csrc/plan_build.hip: s3_gather_rows: "s3::DevBuf<int32_t> d_bad;": with a row list the id check ends with the release '
                 "of this buffer (hipFree waits for the whole device) before the gather is launched, and a valid poison passes the check; "
                 "the re-pitch form below has no such wait")(_gather_rows(True))
case("gather_rows_repitch", "s3_gather_rows")(_gather_rows(False))


def _table(rng, nc, k, n_src, share):
    """a neighbour table that references about ``share`` of the source rows"""
    pool = np.sort(rng.permutation(n_src)[:max(k, int(n_src * share))])
    return pool[rng.integers(0, len(pool), (nc, k))].astype(np.int32)


@case("referenced_rows", "s3_mark_rows", "s3_compact_rows")
def _():
    b, r = Built(), rng_of("referenced_rows")
    t = b.inp(_table(r, 257, 8, 600, 0.5), _table(r, 257, 8, 600, 0.3))
    b.call = lambda: list(ops().referenced_rows([t], 600))
    return b


@case("referenced_rows_hilbert", "s3_mark_rows", "s3_compact_rows", "s3_positions_of", "s3_spatial_order", "s3_gather_rows")
def _():
    b, r = Built(), rng_of("referenced_rows_hilbert")
    t = b.inp(_table(r, 257, 8, 600, 0.5), _table(r, 257, 8, 600, 0.3))
    coords = b.inp(r.random((600, 3)), r.random((600, 3)))
    b.call = lambda: list(ops().referenced_rows([t], 600, coords))
    return b


@case("positions_of", "s3_positions_of")
def _():
    b, r = Built(), rng_of("positions_of")
    ids = b.inp(r.permutation(600)[:257].astype(np.int32), r.permutation(600)[:257].astype(np.int32))
    remap = b.new((600,), I32)

    def call():
        ops().check(lib().s3_positions_of(C.c_void_p(ids.data_ptr()), 257, C.c_void_p(remap.data_ptr()), 600, raw_stream()), "s3_positions_of")
    b.call = call
    return b


@case("remap_indices", "s3_remap_indices")
def _():
    b, r = Built(), rng_of("remap_indices")
    idx = b.inp(r.integers(0, 600, (257, 8)).astype(np.int32), r.integers(0, 600, (257, 8)).astype(np.int32))
    remap = b.inp(r.permutation(600).astype(np.int32), r.permutation(600).astype(np.int32))
    b.call = lambda: [ops().remap_indices(idx, remap)]
    return b


def _spatial_order(dim):
    def make():
        b, r = Built(), rng_of("spatial_order")
        p = b.inp(r.random((1000, dim)), r.random((1000, dim)))
        b.call = lambda: [ops().spatial_order(p)]
        return b
    return make


case("spatial_order_2d", "s3_spatial_order")(_spatial_order(2))
case("spatial_order_3d", "s3_spatial_order")(_spatial_order(3))


def _exclusive_scan(dtype):
    def make():
        b, r = Built(), rng_of("scan")
        x = b.inp(r.integers(0, 4, 4097), r.integers(0, 4, 4097), dtype)          # three levels
        out = b.new((4097,), dtype)

        def call():
            ops().check(lib().s3_exclusive_scan(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), 4097, x.element_size(), raw_stream()),
                        "s3_exclusive_scan")
        b.call = call
        return b
    return make


case("exclusive_scan_i32", "s3_exclusive_scan")(_exclusive_scan(I32))
case("exclusive_scan_i64", "s3_exclusive_scan")(_exclusive_scan(I64))


@case("sort_pairs", "s3_sort_pairs", note="in place: keys and values are inputs and outputs at once, the late copy of the real pairs is their late fill")
def _():
    b, r = Built(), rng_of("sort_pairs")
    n = 2049
    keys = b.inp(r.integers(0, 1 << 40, n), r.integers(0, 1 << 40, n), I64)
    vals = b.inp(r.permutation(n).astype(np.int32), r.permutation(n).astype(np.int32))
    b.call = lambda: list(ops().sort_pairs(keys, vals, 40))
    return b


def _pitched_target(b, n, row_len, dtype):
    pitch = ops().padded_rows(1, row_len, dtype, "cpu").stride(0)
    base = b.new((n, pitch), dtype)
    b.views[-1] = base[:, :row_len]                 # (the padding between two rows may be overwritten: not compared)
    return base[:, :row_len]


@case("upload_rows", "s3_upload_rows", note="the input is host memory: only the late output fill applies")
def _():
    b, r = Built(), rng_of("upload_rows")
    host = pt.from_numpy(r.standard_normal((3000, 25)).astype(np.float32))
    rows = _pitched_target(b, 3000, 25, F32)
    b.call = lambda: [ops().upload_rows(host, rows)]
    return b


@case("upload_rows_indexed", "s3_upload_rows_indexed", note="the input is host memory: only the late output fill applies")
def _():
    b, r = Built(), rng_of("upload_rows_indexed")
    host = pt.from_numpy(r.standard_normal((3000, 7)))
    ids = np.sort(r.permutation(3000)[:777]).astype(np.int32)
    rows = _pitched_target(b, 777, 7, F64)
    b.call = lambda: [ops().upload_rows_indexed(host, ids, rows)]
    return b


def _upload_row_pieces(with_ids):
    def make():
        b, r = Built(), rng_of("upload_row_pieces")
        host = pt.from_numpy(r.standard_normal((1000, 2, 9)).astype(np.float32))
        ids = np.sort(r.permutation(1000)[:333]).astype(np.int32) if with_ids else None
        rows = _pitched_target(b, 333 if with_ids else 1000, 2 * 4, F32)
        b.call = lambda: [ops().upload_row_pieces(host, ids, 3, 7, rows)]
        return b
    return make


case("upload_row_pieces", "s3_upload_row_pieces", note="the input is host memory: only the late output fill applies")(_upload_row_pieces(False))
case("upload_row_pieces_rows", "s3_upload_row_pieces", note="the input is host memory: only the late output fill applies")(_upload_row_pieces(True))


@case("to_host", "s3_download", note="the output is host memory: only the late input applies")
def _():
    b, r = Built(), rng_of("to_host")
    t = b.inp(r.standard_normal((257, 33)), r.standard_normal((257, 33)))
    b.call = lambda: [ops().to_host(t)]
    return b


@case("to_host_large", "s3_download",
      note="five chunks of 8 MiB and a ragged one: the path that waits for the given stream and then copies on the lanes' own streams "
           "from several host threads; the small cases go through one lane on the given stream")
def _():
    b, r = Built(), rng_of("to_host_large")
    n = 5 * (1 << 20) + 17
    t = b.inp(r.random(n), r.random(n))

    def call():
        out = np.empty(n)
        ops().check(lib().s3_download(C.c_void_p(out.ctypes.data), C.c_void_p(t.data_ptr()), out.nbytes, raw_stream()), "s3_download")
        return [out, ops().to_host(t)]          # on the given stream, and as the wrapper does it (after its own wait, stream NULL)
    b.call = call
    return b


@case("download_on_stream", "s3_download", note="the output is host memory: only the late input applies")
def _():
    b, r = Built(), rng_of("download")
    t = b.inp(r.standard_normal((257, 33)), r.standard_normal((257, 33)))

    def call():
        out = np.empty((257, 33))
        ops().check(lib().s3_download(C.c_void_p(out.ctypes.data), C.c_void_p(t.data_ptr()), out.nbytes, raw_stream()), "s3_download")
        return [out]
    b.call = call
    return b


def _memcpy_h2d(pinned):
    def make():
        b, r = Built(), rng_of("h2d")
        host = pt.from_numpy(r.standard_normal(3001))
        host = host.pin_memory() if pinned else host
        out = b.new((3001,), F64)

        def call():
            ops().check(lib().s3_memcpy_h2d(C.c_void_p(out.data_ptr()), C.c_void_p(host.data_ptr()), 3001 * 8, raw_stream()), "s3_memcpy_h2d")
        b.call = call
        return b
    return make


def _memcpy_d2h(pinned):
    def make():
        b, r = Built(), rng_of("d2h")
        t = b.inp(r.standard_normal(3001), r.standard_normal(3001))
        host = pt.zeros(3001, dtype=F64)
        host = host.pin_memory() if pinned else host

        def call():
            ops().check(lib().s3_memcpy_d2h(C.c_void_p(host.data_ptr()), C.c_void_p(t.data_ptr()), 3001 * 8, raw_stream()), "s3_memcpy_d2h")
            return [host.numpy()]           # (a view: read after the stream is synchronised)
        b.call = call
        return b
    return make


case("memcpy_h2d_pageable", "s3_memcpy_h2d", note="the input is host memory: only the late output fill applies")(_memcpy_h2d(False))
case("memcpy_h2d_pinned", "s3_memcpy_h2d", note="the input is host memory: only the late output fill applies")(_memcpy_h2d(True))
case("memcpy_d2h_pageable", "s3_memcpy_d2h", note="the output is host memory: only the late input applies")(_memcpy_d2h(False))
case("memcpy_d2h_pinned", "s3_memcpy_d2h", note="the output is host memory: only the late input applies")(_memcpy_d2h(True))


# ---- KNN and refine ---------------------------------------------------------------------------------------------------------------
def _query_case(name):
    """a cloud of tests/knn_query_cases.py -> (dim, k, occupancy, points, values, queries)"""
    from tests import knn_query_cases as kq
    return kq.case(name)[1:]


def _other_cloud(rng, x):
    """another valid cloud of the same shape and ANOTHER bounding box: the points mirrored, renumbered and stretched by another factor
    per axis about a corner outside the cloud.  The box of the result holds the box of ``x``: points of ``x`` binned on a lattice made
    for the result (what a build sees whose first pass read this cloud and whose later passes read ``x``) lie inside it, and
    s3_knn_create clamps lattice coordinates anyway (csrc/knn.hip, cell_coord)"""
    lo, ext = x.min(0), x.max(0) - x.min(0)
    ext = np.where(ext > 0, ext, 1.0)
    factor = np.array([1.5, 2.5, 2.0])[:x.shape[1]]
    mirrored = (x.min(0) + x.max(0) - x)[rng.permutation(len(x))]
    return np.ascontiguousarray(lo - 0.25 * ext + (mirrored - lo) * factor)


def _knn_create(name):
    def make():
        b, r = Built(), rng_of("knn_create" + name)
        dim, k, occ, x, _, q = _query_case(name)
        p = b.inp(x, _other_cloud(r, x))
        d_q = dev(q)
        made = []
        b.closers.append(lambda: [index.close() for index in made])

        def call():
            made.append(ops().KnnIndex(p, occ))
            idx, dist = made[-1].query(d_q, k)
            return [made[-1].n_buckets, made[-1].n_refined_buckets, idx, dist]
        b.call = call
        return b
    return make


# s3_knn_create releases the scratch of its bounding-box pass (hipFree: a wait for the whole device) before the launches that build
# the index, so in the control only that pass reads the poison: the poison's box is another one, and with it the lattice, n_buckets and
# n_refined_buckets the call returns
case("knn_create_3d", "s3_knn_create")(_knn_create("kend3d_k8"))
case("knn_create_2d_refined", "s3_knn_create")(_knn_create("bigdup2d_k26"))      # a refined bucket


def _knn(b, x, y, occ):
    knn = ops().KnnIndex(dev(x), occ)
    knn.set_values(dev(y))
    pt.cuda.synchronize()
    b.closers.append(knn.close)
    return knn


@case("knn_set_values", "s3_knn_set_values")
def _():
    b, r = Built(), rng_of("set_values")
    dim, k, occ, x, y, q = _query_case("kend3d_k8")
    knn = _knn(b, x, y, occ)
    d_y = b.inp(y, r.permutation(y))
    d_q = dev(q)

    def call():
        knn.set_values(d_y)
        return [knn.predict(d_q, k)]
    b.call = call
    return b


def _knn_query(name, predict):
    def make():
        b, r = Built(), rng_of(f"knn_query{name}{predict}")
        dim, k, occ, x, y, q = _query_case(name)
        knn = _knn(b, x, y, occ)
        d_q = b.inp(q, q[::-1] + 0.013)                                            # other valid queries
        b.call = (lambda: [knn.predict(d_q, k)]) if predict else (lambda: list(knn.query(d_q, k)))
        return b
    return make


# ties across the k-th neighbour in 2-D, k = 26 in 3-D, and the graded wall cloud with refined buckets
case("knn_query_2d_ties", "s3_knn_query")(_knn_query("dup2d_r8_k8", False))
case("knn_query_3d", "s3_knn_query")(_knn_query("kend3d_k26", False))
case("knn_query_2d_refined", "s3_knn_query")(_knn_query("wall2d_o96_k8", False))
case("knn_predict_2d_ties", "s3_idw_predict")(_knn_query("dup2d_r8_k8", True))
case("knn_predict_3d", "s3_idw_predict")(_knn_query("kend3d_k26", True))
case("knn_predict_2d_refined", "s3_idw_predict")(_knn_query("wall2d_o96_k8", True))


def _cells(rng, cap, dim, level):
    return rng.random((cap, dim)) * 1.2 - 0.1, np.full(cap, level, dtype=np.int32)


@case("make_children", "s3_make_children", note="centres and levels are read (the parents' rows) and written (the children's): their real content goes in late")
def _():
    b, r = Built(), rng_of("make_children")
    dim, n_par, first = 3, 37, 100
    cap = first + n_par * 8
    parents = b.inp(r.permutation(first)[:n_par].astype(np.int32), r.permutation(first)[:n_par].astype(np.int32))
    (c0, l0), (c1, l1) = _cells(r, cap, dim, 3), _cells(r, cap, dim, 2)
    center, level = b.new((cap, dim), F64, init=(c0, c1)), b.new((cap,), I32, init=(l0, l1))
    b.call = lambda: ops().make_children(center, level, parents, first, 1.0)
    return b


def _child_gain(cloud, reuse, with_parents):
    def make():
        from tests import child_metric_cases as cm
        b, r = Built(), rng_of(f"child_gain{cloud}{reuse}{with_parents}")
        _, dim, k, occ, x, y, _ = cm.case(cloud)                                   # the cloud, its values and k of the oracle's case
        knn = _knn(b, x, y, occ)
        nch, n = 2 ** dim, 304                                                    # whole parents in 2-D and 3-D
        first, n_par = nch, (n + nch - 1) // nch
        cap = first + n
        lf = dev(np.array([1 / nch * ((1.0 / 2 ** lv) ** dim) for lv in range(64)]))
        (c0, l0), (c1, l1) = _cells(r, cap, dim, 5), _cells(r, cap, dim, 4)
        center, level = b.inp(c0, c1), b.inp(l0, l1)
        metric, gain = b.new((cap,), F64, init=(np.zeros(cap), np.ones(cap))), b.new((cap,), F64, init=(np.zeros(cap), np.ones(cap)))
        words = n * (nch + 1) + 2 + n * nch
        scratch = b.new((words,), F64, init=(np.zeros(words), np.ones(words)))
        b.views[-1] = scratch[:n * (nch + 1)]            # the values of the centres and child points; the hand-off lists behind them
        if not reuse:                                    # are filled in the order the wavefronts finish: not compared
            b.call = lambda: ops().child_gain(knn, k, center, level, first, n, 1.0, lf, 0.37, metric, gain, scratch)
            return b
        rows = cap + n_par
        child = b.new((rows, nch), F64, init=(r.random((rows, nch)), r.random((rows, nch))))
        parents = b.inp((cap + r.permutation(n_par)).astype(np.int32), (cap + r.permutation(n_par)).astype(np.int32)) if with_parents else None
        b.call = lambda: ops().child_gain_reuse(knn, k, center, level, first, n, 1.0, lf, 0.37, metric, gain, scratch, parents, 0, child)
        return b
    return make


# lattice clouds: ties in distance at every turn; dup3d_r48_k49: k > 48 sends every query through coop -> near -> far -> per lane
case("child_gain_2d", "s3_child_gain")(_child_gain("lattice2d_k7", False, False))
case("child_gain_3d", "s3_child_gain")(_child_gain("lattice3d_k26", False, False))
case("child_gain_reuse_root", "s3_child_gain_reuse")(_child_gain("lattice2d_k7", True, False))
case("child_gain_reuse_parents_2d", "s3_child_gain_reuse")(_child_gain("lattice2d_k7", True, True))
case("child_gain_reuse_parents_3d", "s3_child_gain_reuse")(_child_gain("lattice3d_k26", True, True))
case("child_gain_reuse_parents_k49", "s3_child_gain_reuse")(_child_gain("dup3d_r48_k49", True, True))


@case("commit_batch", "s3_commit_batch", note="leaf flags and gains are updated in place: their real content goes in late")
def _():
    b, r = Built(), rng_of("commit_batch")
    first, n_par = 1000, 250
    n_new, cap = n_par * 4, 1000 + 250 * 4
    parents = b.inp(r.permutation(first)[:n_par].astype(np.int32), r.permutation(first)[:n_par].astype(np.int32))
    invalid = b.inp(r.random(n_new) < 0.3, r.random(n_new) < 0.6, U8)
    leaf = b.new((cap,), U8, init=(np.r_[np.ones(first), np.zeros(n_new)], np.zeros(cap)))
    gain = b.new((cap,), F64, init=(r.random(cap), r.random(cap)))
    b.call = lambda: ops().commit_batch(leaf, gain, parents, first, n_new, invalid)
    return b


def _metric_leaf(b, rng, n):
    return b.inp(rng.standard_normal(n), rng.standard_normal(n)), b.inp(rng.random(n) < 0.6, rng.random(n) < 0.4, U8)


@case("sumsq_leaf", "s3_sumsq_leaf")
def _():
    b, r = Built(), rng_of("sumsq_leaf")
    metric, leaf = _metric_leaf(b, r, 3001)
    out, scratch = b.new((1,), F64), b.new((1024,), F64, init=(np.zeros(1024), np.ones(1024)))
    b.call = lambda: ops().sumsq_leaf(metric, leaf, 5, 2999, out, scratch)
    return b


@case("sumsq_blocks", "s3_sumsq_blocks")
def _():
    b, r = Built(), rng_of("sumsq_blocks")
    metric, leaf = _metric_leaf(b, r, 3001)
    partial = b.new((3,), F64)
    b.call = lambda: ops().sumsq_blocks(metric, leaf, 3001, 0, 3, partial)
    return b


@case("sum_ordered", "s3_sum_ordered")
def _():
    b, r = Built(), rng_of("sum_ordered")
    v = b.inp(r.standard_normal(3001), r.standard_normal(3001))
    out = b.new((1,), F64)
    b.call = lambda: ops().sum_ordered(v, 3001, out)
    return b


@case("topn_leaf", "s3_topn_leaf")
def _():
    b, r = Built(), rng_of("topn_leaf")
    n, n_top = 3001, 129
    gain = b.inp(np.round(r.random(n), 2), np.round(r.random(n), 2))               # ties in the gain
    leaf = b.inp(r.random(n) < 0.6, r.random(n) < 0.4, U8)
    words = (int(lib().s3_topn_scratch_bytes(n, n_top)) + 7) // 8
    scratch = b.new((words,), F64, init=(np.zeros(words), np.ones(words)))
    b.call = lambda: [ops().topn_leaf(gain, leaf, n, n_top, scratch)]
    b.views[-1] = scratch[:0]                                                     # (working memory: filled late, not compared)
    return b


def _lattice_cells(dim, level, lo=-0.5, width=2.0, shift=0.0):
    m = 1 << level
    side = lo + (np.arange(m) + 0.5) * (width / m) + shift
    c = np.stack(np.meshgrid(*[side] * dim, indexing="ij"), -1).reshape(-1, dim)
    return c, np.full(len(c), level, dtype=np.int32)


def _mask_bodies(tmp=None):
    """kind -> (dim, geometry): bodies that cut through the level-4 lattice of [-0.5, 1.5]^dim"""
    from sparsespatialsampling_amd import geometry as G
    from tests import stl_meshes as M
    return {"box": (3, lambda: G.CubeGeometry("b", False, [0.1, 0.2, 0.0], [0.9, 0.7, 1.1])),
            "sphere": (2, lambda: G.SphereGeometry("s", False, [0.4, 0.6], 0.55)),
            "cylinder": (3, lambda: G.CylinderGeometry3D("c", False, [[0.0, 0.2, 0.3], [1.0, 0.8, 0.6]], [0.5, 0.2])),
            "polygon": (2, lambda: G.GeometryCoordinates2D("p", False, [[0.0, 0.0], [1.0, 0.1], [0.6, 0.5], [0.9, 1.2], [-0.2, 0.8]])),
            "triangle": (2, lambda: G.TriangleGeometry("t", False, [[-0.2, -0.1], [1.2, 0.3], [0.3, 1.3]])),
            "prism": (3, lambda: G.PrismGeometry3D("r", False, [[[-0.2, -0.1, 0.1], [1.2, 0.3, 0.1], [0.3, 1.3, 0.1]],
                                                                 [[-0.2, -0.1, 0.9], [1.2, 0.3, 0.9], [0.3, 1.3, 0.9]]])),
            "tetrahedra": (3, lambda: G.PyramidGeometry3D("y", False, [[-0.3, -0.3, 0.0], [1.3, -0.3, 0.0], [1.3, 1.3, 0.0], [-0.3, 1.3, 0.0],
                                                                       [0.5, 0.5, 1.4]])),
            "mesh": (3, lambda: G.GeometrySTL3D("cube", False, M.CUBE_STL))}


def _mask(kind):
    def make():
        b, r = Built(), rng_of("mask_" + kind)
        dim, body = _mask_bodies()[kind]
        spec = body().kernel_spec()
        assert spec[0] == kind, spec[0]
        (c0, l0), (c1, l1) = _lattice_cells(dim, 4), _lattice_cells(dim, 4, shift=0.031)
        n = len(c0)
        order = r.permutation(n)
        center, level = b.inp(c0, c1[order]), b.inp(l0, l1)
        cells = b.inp(r.permutation(n)[:n - 7].astype(np.int32), r.permutation(n)[:n - 7].astype(np.int32))
        operands, uploaded = ops().mask_operands(spec)
        if kind == "polygon":                                   # the vertices are a device input too
            xy = np.ascontiguousarray(spec[1], dtype=np.float64)
            operands = (b.inp(xy, xy[::-1] * 0.9 + 0.05),)
        pt.cuda.synchronize()
        flags = [b.new((n,), U8, init=(r.random(n) < 0.1, r.random(n) < 0.5)) for _ in range(2)]
        whole = ops().MaskCells(center, level, 2.0, flags[0])
        listed = ops().MaskCells(center, level, 2.0, flags[1], cells=cells)

        def call():
            ops().mask_body(whole, kind, operands, 0, 0)
            ops().mask_body(whole, kind, operands, 1, 1)       # ORs into the same flags
            ops().mask_body(listed, kind, operands, 1, 0)
        b.call = call
        return b
    return make


for _kind in ("box", "sphere", "cylinder", "polygon", "triangle", "prism", "tetrahedra", "mesh"):
    case("mask_" + _kind, "s3_mask_" + _kind,
         note="the invalid flags are OR-ed into: their real initial content goes in late")(_mask(_kind))


# ---- moments and linear algebra ---------------------------------------------------------------------------------------------------
N_ROWS, N_T = 257, 33


def _matrix(b, rng, dtype, pitched=True):
    npt = np.float32 if dtype == F32 else np.float64
    real, poison = (rng.standard_normal((N_ROWS, N_T + 3)).astype(npt) for _ in range(2))
    buf = b.inp(real, poison)
    return buf[:, :N_T] if pitched else buf


def _row_moments(entry, dtype):
    def make():
        b, r = Built(), rng_of(entry)
        x = _matrix(b, r, dtype)
        mean, std = b.new((N_ROWS,), F64), b.new((N_ROWS,), F64)

        def call():
            ops().check(getattr(lib(), entry)(C.c_void_p(x.data_ptr()), ops().DTYPE_CODE[dtype], N_ROWS, N_T, int(x.stride(0)), 1,
                                              C.c_void_p(mean.data_ptr()), C.c_void_p(std.data_ptr()), raw_stream()), entry)
        b.call = call
        return b
    return make


case("row_moments_f32", "s3_row_moments")(_row_moments("s3_row_moments", F32))
case("row_moments_f64", "s3_row_moments")(_row_moments("s3_row_moments", F64))
case("row_abs_moments_f32", "s3_row_abs_moments")(_row_moments("s3_row_abs_moments", F32))
case("row_abs_moments_f64", "s3_row_abs_moments")(_row_moments("s3_row_abs_moments", F64))


def _gram(dtype, centred):
    def make():
        b, r = Built(), rng_of(f"gram{dtype}{centred}")
        x = _matrix(b, r, dtype)
        mean = b.inp(r.standard_normal(N_ROWS), r.standard_normal(N_ROWS)) if centred else None
        weight = b.inp(r.random(N_ROWS) + 0.1, r.random(N_ROWS) + 0.1) if centred else None
        out = b.new((N_T, N_T), F64)
        words = (int(lib().s3_gram_scratch_bytes(N_ROWS, N_T)) + 7) // 8
        scratch = b.new((words,), F64, init=(np.zeros(words), np.ones(words)))
        b.views[-1] = scratch[:0]                                                 # (working memory: filled late, not compared)
        b.call = lambda: [ops().gram(x, mean, weight, out=out, scratch=scratch)]
        return b
    return make


case("gram_f32", "s3_gram")(_gram(F32, False))
case("gram_f64", "s3_gram")(_gram(F64, False))
case("gram_f32_mean_weight", "s3_gram")(_gram(F32, True))
case("gram_f64_mean_weight", "s3_gram")(_gram(F64, True))


@case("weighted_gram", "s3_weighted_gram")
def _():
    from sparsespatialsampling_amd import svd
    b, r = Built(), rng_of("weighted_gram")
    x = _matrix(b, r, F64)
    mean, weight = b.inp(r.standard_normal(N_ROWS), r.standard_normal(N_ROWS)), b.inp(r.random(N_ROWS) + 0.1, r.random(N_ROWS) + 0.1)
    b.call = lambda: [svd.weighted_gram(x, mean, weight)]
    return b


def _tall_gemm(dtype):
    def make():
        b, r = Built(), rng_of(f"tall_gemm{dtype}")
        left = _matrix(b, r, dtype)
        right = b.inp(r.standard_normal((N_T, 5)), r.standard_normal((N_T, 5)))
        out = b.new((N_ROWS, 5), F64)
        b.call = lambda: [ops().tall_gemm(left, right, out=out)]
        return b
    return make


case("tall_gemm_f32", "s3_tall_gemm")(_tall_gemm(F32))
case("tall_gemm_f64", "s3_tall_gemm")(_tall_gemm(F64))


def _centered_gemm(residual):
    def make():
        from sparsespatialsampling_amd import svd
        b, r = Built(), rng_of(f"centered_gemm{residual}")
        left = _matrix(b, r, F64)
        lmean = b.inp(r.standard_normal(N_ROWS), r.standard_normal(N_ROWS))
        right = b.inp(r.standard_normal((N_T, 5)), r.standard_normal((N_T, 5)))
        e = b.inp(r.standard_normal((N_ROWS, 8)), r.standard_normal((N_ROWS, 8)))[:, :5] if residual else None
        emean = b.inp(r.standard_normal(N_ROWS), r.standard_normal(N_ROWS)) if residual else None
        b.call = lambda: [svd.centered_gemm(left, lmean, right, e, emean)]
        return b
    return make


case("centered_gemm_modes", "s3_centered_gemm")(_centered_gemm(False))
case("centered_gemm_residual", "s3_centered_gemm")(_centered_gemm(True))


@case("sym_eig", "s3_sym_eig")
def _():
    from sparsespatialsampling_amd import svd
    b, r = Built(), rng_of("sym_eig")
    a = [r.standard_normal((N_ROWS, N_T)) for _ in range(2)]
    g = b.inp(a[0].T @ a[0], a[1].T @ a[1])
    assert lib().s3_sym_eig_available(), "rocSOLVER cannot be loaded: s3_sym_eig has nothing to run"
    b.call = lambda: [t.numpy() for t in svd._eigh(g)]
    return b


def _segment(psd, dtype, centred):
    def make():
        b, r = Built(), rng_of(f"segment{psd}{dtype}{centred}")
        nperseg, hop, n_blk, n_f = 8, 5, 6, 5                       # 5 * 5 + 8 = 33 samples
        x = _matrix(b, r, dtype)
        mean = b.inp(r.standard_normal(N_ROWS), r.standard_normal(N_ROWS)) if centred else None
        bre, bim = (b.inp(r.standard_normal((nperseg, n_f)), r.standard_normal((nperseg, n_f))) for _ in range(2))
        if psd:
            scale = b.inp(r.random(n_f) + 0.1, r.random(n_f) + 0.1)
            out = b.new((N_ROWS, n_f), F64)
            b.call = lambda: [ops().segment_psd(x, mean, nperseg, hop, n_blk, bre, bim, scale, out=out)]
        else:
            out = b.new((N_ROWS, n_f, n_blk, 2), F64)
            b.call = lambda: [ops().segment_dft(x, mean, nperseg, hop, n_blk, bre, bim, out=out)]
        return b
    return make


case("segment_dft_f32", "s3_segment_dft")(_segment(False, F32, False))
case("segment_dft_f64_mean", "s3_segment_dft")(_segment(False, F64, True))
case("segment_psd_f32_mean", "s3_segment_psd")(_segment(True, F32, True))
case("segment_psd_f64", "s3_segment_psd")(_segment(True, F64, False))


# ---- analysis kernels -------------------------------------------------------------------------------------------------------------
T_ROW = 3


def _grid(name):
    from tests import region_cases as rc
    return rc.grid(name)


def _index(g):
    ix = ops().cell_index(dev(g["centers"]), dev(g["levels"]), g["width"])
    pt.cuda.synchronize()
    return ix


def _field(rng, n, n_comp, dtype):
    shape = (n, T_ROW) if n_comp == 0 else (n, n_comp, T_ROW)
    return [rng.standard_normal(shape).astype(np.float32 if dtype == F32 else np.float64) for _ in range(2)]


def _recon(with_rows, grid_dtype, orig_dtype):
    def make():
        b, r = Built(), rng_of(f"recon{with_rows}")
        nc, n_orig, k = 300, 1500, 8
        n = 1100 if with_rows else n_orig                                         # two blocks of S3_RECON_BLOCK points
        w = [r.random((n, k)) for _ in range(2)]
        d_w = b.inp(*[v / v.sum(1, keepdims=True) for v in w])
        d_idx = b.inp(r.integers(0, nc, (n, k)).astype(np.int32), r.integers(0, nc, (n, k)).astype(np.int32))
        grid = b.inp(*_field(r, nc, 0, grid_dtype))
        orig = b.inp(*_field(r, n_orig, 0, orig_dtype))
        rows = b.inp(r.permutation(n_orig)[:n].astype(np.int32), r.permutation(n_orig)[:n].astype(np.int32)) if with_rows else None
        scale = b.inp(r.random(n) + 0.5, r.random(n) + 0.5) if with_rows else None
        mean, m2 = b.new((n_orig,), F64), b.new((n_orig,), F64)
        b.call = lambda: list(ops().recon_error(d_w, d_idx, grid, orig, rows, scale, mean, m2))
        return b
    return make


case("recon_error", "s3_recon_error")(_recon(False, F64, F32))
case("recon_error_rows_scale", "s3_recon_error")(_recon(True, F32, F64))


def _stencils(dim):
    """the hostile cloud of tests/grad_cases.py (632 | 636 points, planted degenerate rows) with its neighbour table
    -> (points, idx int32 [n, 8 | 26])"""
    from tests import grad_cases as gc
    pts = np.ascontiguousarray(gc.cloud(f"hostile{dim}d")[0], dtype=np.float64)
    return pts, gc.neighbours(pts, gc.default_neighbors(dim))


def _grad_coeff(dim, with_rows):
    def make():
        b, r = Built(), rng_of(f"grad_coeff{dim}{with_rows}")
        pts, idx = _stencils(dim)
        n = len(pts)
        flat = pts + 0.01 * r.random(pts.shape)
        flat[::5] = flat[0]                                                       # coincident points: other degenerate rows
        p = b.inp(pts, flat)
        if with_rows:
            o0, o1 = r.permutation(n), r.permutation(n)
            d_idx, rows = b.inp(idx[o0], idx[o1]), b.inp(o0.astype(np.int32), o1.astype(np.int32))
        else:
            d_idx, rows = b.inp(idx, idx[:, ::-1].copy()), None
        b.call = lambda: list(ops().grad_coeff(p, d_idx, 2, rows))
        return b
    return make


case("grad_coeff_2d", "s3_grad_coeff")(_grad_coeff(2, False))
case("grad_coeff_3d_rows", "s3_grad_coeff")(_grad_coeff(3, True))


def _grad_apply(dim, mode, dtype):
    def make():
        b, r = Built(), rng_of(f"grad_apply{dim}{mode}")
        pts, idx = _stencils(dim)
        n, k = idx.shape
        coef = b.inp(r.standard_normal((n, k, dim)), r.standard_normal((n, k, dim)))
        d_idx = b.inp(idx, idx[::-1].copy())
        n_comp = 4 if mode == "gradient" else dim                                  # "gradient": two launches (3 + 1 components)
        field = b.inp(*_field(r, n, n_comp, dtype))
        rows = b.inp(r.permutation(n).astype(np.int32), r.permutation(n).astype(np.int32))
        out = b.new((n, ops().grad_n_out(mode, dim, n_comp), T_ROW), F64)
        b.call = lambda: [ops().grad_apply(coef, d_idx, field, mode, rows, out=out)]
        return b
    return make


for _i, _mode in enumerate(("gradient", "magnitude", "divergence", "vorticity", "vorticity_magnitude", "q")):
    case(f"grad_apply_{_mode}", "s3_grad_apply")(_grad_apply(2 + _i % 2, _mode, F32 if _i % 2 else F64))


def _cell_index(name):
    def make():
        b, r = Built(), rng_of("cell_index" + name)
        g = _grid(name)
        order = r.permutation(len(g["centers"]))
        c = b.inp(g["centers"], g["centers"][order])                               # the same grid in another numbering
        lv = b.inp(g["levels"], g["levels"][order])

        def call():
            ix = ops().cell_index(c, lv, g["width"])
            return [ix.starts, ix.ends, ix.ids, ix.origin, ix.h_min, ix.depth]
        b.call = call
        return b
    return make


# (s3_cell_index sorts its keys with a scratch buffer that is released inside the call: in the control the keys come from the poison
# numbering and the overlap check reads the real one, and the call refuses the mixture as overlapping cells -- no write depends on it)
case("cell_index_2d", "s3_cell_index", "s3_sort_pairs", may_refuse=True)(_cell_index("tree2d"))
case("cell_index_3d", "s3_cell_index", "s3_sort_pairs", may_refuse=True)(_cell_index("tree3d"))


def _queries(g, rng, n):
    lo, hi = g["nodes"].min(0), g["nodes"].max(0)
    return lo + (hi - lo) * (rng.random((n, len(lo))) * 1.1 - 0.05)


def _cell_locate(name, with_rows):
    def make():
        b, r = Built(), rng_of("cell_locate" + name)
        g = _grid(name)
        ix = _index(g)
        q = b.inp(_queries(g, r, 777), _queries(g, r, 777))
        rows = b.inp(r.permutation(777).astype(np.int32), r.permutation(777).astype(np.int32)) if with_rows else None
        out = b.new((777,), I32)
        b.call = lambda: [ops().cell_locate(ix, q, rows, out=out)]
        return b
    return make


case("cell_locate_2d", "s3_cell_locate")(_cell_locate("tree2d", False))
case("cell_locate_3d_rows", "s3_cell_locate")(_cell_locate("tree3d", True))


def _located(g, ix, q):
    ids = ops().cell_locate(ix, dev(q)).cpu().numpy()
    pt.cuda.synchronize()
    return ids


def _cell_sample(name, mode, dtype):
    def make():
        b, r = Built(), rng_of("cell_sample" + name + mode)
        g = _grid(name)
        ix = _index(g)
        q = [_queries(g, r, 777) for _ in range(2)]
        ids = b.inp(*[_located(g, ix, v) for v in q])
        n_field = len(g["nodes"]) if mode == "linear" else len(g["centers"])
        field = b.inp(*_field(r, n_field, 4, dtype))                               # two launches (3 + 1 components)
        out = b.new((777, 4, T_ROW), F64)
        if mode == "linear":
            pts, faces = b.inp(*q), dev(g["faces"])
            rows = b.inp(r.permutation(777).astype(np.int32), r.permutation(777).astype(np.int32))
            b.call = lambda: [ops().cell_sample(ids, field, "linear", rows, out=out, index=ix, points=pts, faces=faces)]
        else:
            b.call = lambda: [ops().cell_sample(ids, field, "cell", out=out)]
        return b
    return make


case("cell_sample_cell_2d", "s3_cell_sample")(_cell_sample("tree2d", "cell", F32))
case("cell_sample_linear_3d", "s3_cell_sample")(_cell_sample("tree3d", "linear", F64))
case("cell_sample_linear_2d", "s3_cell_sample")(_cell_sample("tree2d", "linear", F32))


def _seeds(g, rng, n):
    c = g["centers"][rng.integers(0, len(g["centers"]), n)]
    return c + (rng.random(c.shape) - 0.5) * 1e-3


def _trace(name, path, dtype):
    def make():
        b, r = Built(), rng_of(f"trace{name}{path}")
        g = _grid(name)
        ix, faces, dim = _index(g), dev(g["faces"]), g["centers"].shape[1]
        vel = b.inp(*_field(r, len(g["nodes"]), dim, dtype))
        seeds = b.inp(_seeds(g, r, 333), _seeds(g, r, 333))
        order = b.inp(r.permutation(333).astype(np.int32), r.permutation(333).astype(np.int32))
        shape = (333,) if path else (333, T_ROW)
        outs = [b.new(shape + ((T_ROW, dim) if path else (1 + 6 // 2, dim)), F64)] + [b.new(shape, I32) for _ in range(3)]
        if path:
            b.call = lambda: list(ops().trace_path(ix, faces, vel, seeds, 1e-3, 2, 1, order, *outs))
        else:
            b.call = lambda: list(ops().trace_stream(ix, faces, vel, seeds, 6, "cell", 0.5, None, 1, 2, order, *outs))
        return b
    return make


case("trace_stream_2d", "s3_trace")(_trace("tree2d", False, F32))
case("trace_stream_3d", "s3_trace")(_trace("tree3d", False, F64))
case("trace_path_2d", "s3_trace")(_trace("tree2d", True, F64))
case("trace_path_3d", "s3_trace")(_trace("tree3d", True, F32))


def _node_field(g, rng, dtype):
    x = g["nodes"] - g["nodes"].mean(0)
    out = []
    for _ in range(2):
        a = rng.standard_normal((x.shape[1], T_ROW))
        out.append((np.sin(9 * x @ a) + 0.1 * rng.standard_normal((len(x), T_ROW))).astype(np.float32 if dtype == F32 else np.float64))
    return out


def _iso_count(name, dtype):
    def make():
        b, r = Built(), rng_of("iso_count" + name)
        g = _grid(name)
        field, faces = b.inp(*_node_field(g, r, dtype)), dev(g["faces"])
        out = b.new((T_ROW, len(g["faces"])), I32)
        b.call = lambda: [ops().iso_count(field, faces, 0.125, out=out)]
        return b
    return make


case("iso_count_2d", "s3_iso_count")(_iso_count("tree2d", F64))
case("iso_count_3d", "s3_iso_count")(_iso_count("tree3d", F32))


def _iso_emit(name, dtype):
    def make():
        b, r = Built(), rng_of("iso_emit" + name)
        g = _grid(name)
        dim, n_cells = g["centers"].shape[1], len(g["faces"])
        real, poison = _node_field(g, r, dtype)
        faces, nodes = dev(g["faces"]), dev(g["nodes"])
        scans = []
        for f in (real, poison):                                                   # the offsets of either field: both valid
            scan = pt.zeros(T_ROW * n_cells + 1, dtype=I32, device="cuda")
            ops().iso_count(dev(f), faces, 0.125, out=scan)
            scans.append(ops().exclusive_scan(scan).cpu().numpy())
        capacity = int(scans[0][-1])
        assert capacity > 0
        field, offsets = b.inp(real, poison), b.inp(scans[0], np.minimum(scans[1], capacity))
        outs = [b.new((capacity, dim, dim), F64), b.new((capacity, dim, 2), I32), b.new((capacity, dim), F64), b.new((capacity,), I32)]
        b.call = lambda: list(ops().iso_emit(field, faces, 0.125, nodes, offsets, capacity, *outs))
        return b
    return make


case("iso_emit_2d", "s3_iso_emit")(_iso_emit("tree2d", F32))
case("iso_emit_3d", "s3_iso_emit")(_iso_emit("tree3d", F64))


@case("iso_extract_3d", "s3_iso_count", "s3_exclusive_scan", "s3_iso_emit")
def _():
    b, r = Built(), rng_of("iso_extract")
    g = _grid("tree3d")
    field, faces, nodes = b.inp(*_node_field(g, r, F32)), dev(g["faces"]), dev(g["nodes"])
    b.call = lambda: list(ops().iso_extract(field, faces, nodes, 0.125))
    return b


def _cell_neighbours(name):
    def make():
        b, r = Built(), rng_of("cell_neighbours" + name)
        g = _grid(name)
        order = r.permutation(len(g["centers"]))
        c, lv = b.inp(g["centers"], g["centers"][order]), b.inp(g["levels"], g["levels"][order])
        out = b.new((len(order), 2 * g["centers"].shape[1]), I32)

        def call():                                                                # index and table in one go: both on the stream
            return [ops().cell_neighbours(ops().cell_index(c, lv, g["width"]), out=out)]
        b.call = call
        return b
    return make


case("cell_neighbours_2d", "s3_cell_neighbours", "s3_cell_index", may_refuse=True)(_cell_neighbours("tree2d"))
case("cell_neighbours_3d", "s3_cell_neighbours", "s3_cell_index", may_refuse=True)(_cell_neighbours("tree3d"))


def _neighbours(g):
    ix = _index(g)
    nbr = ops().cell_neighbours(ix)
    pt.cuda.synchronize()
    return ix, nbr


def _region_fields(name, mask):
    from tests import region_cases as rc
    field, lo, hi = rc.cases(name)[mask]
    field = np.ascontiguousarray(field[:, :T_ROW])
    # the same values on other cells, the columns in another order: a point reflection alone maps the checkerboard onto itself and
    # keeps the region counts of the other drawn masks, and such a poison gives the real table back
    other = np.ascontiguousarray(np.roll(field, len(field) // 3 + 1, axis=0)[::-1, ::-1])
    return field, other, lo, hi


def _region_label(name, mask, with_order):
    def make():
        b, r = Built(), rng_of("region_label" + name + mask)
        g = _grid(name)
        ix, nbr = _neighbours(g)
        real, poison, lo, hi = _region_fields(name, mask)
        field = b.inp(real, poison)
        n = len(real)
        order = b.inp(r.permutation(n).astype(np.int32), r.permutation(n).astype(np.int32)) if with_order else None
        out = b.new((n, real.shape[1]), I32)
        b.call = lambda: [ops().region_label(field, nbr, lo, hi, order, out=out)]
        return b
    return make


case("region_label_2d", "s3_region_label")(_region_label("tree2d", "smooth32", False))
case("region_label_3d_order", "s3_region_label")(_region_label("tree3d", "smooth64", True))


def _region_table(name, mask, weighted):
    def make():
        b, r = Built(), rng_of("region_table" + name + mask)
        g = _grid(name)
        ix, nbr = _neighbours(g)
        real, poison, lo, hi = _region_fields(name, mask)
        labels = b.inp(*[ops().region_label(dev(f), nbr, lo, hi).cpu().numpy() for f in (real, poison)])     # labellings of two fields: both valid
        weight = b.inp(*[r.standard_normal(real.shape) for _ in range(2)]) if weighted else None
        b.call = lambda: [ops().region_table(labels, ix, weight)]
        return b
    return make


case("region_table_2d", "s3_region_count", "s3_region_emit", "s3_exclusive_scan")(_region_table("tree2d", "smooth32", False))
case("region_table_3d_weight", "s3_region_count", "s3_region_emit", "s3_exclusive_scan")(_region_table("tree3d", "smooth64", True))
case("region_table_big_regions", "s3_region_count", "s3_region_emit", "s3_exclusive_scan",
     note="uniform2d 'drawn': regions of more than 1024 cells take the big-region launch of s3_region_emit")(_region_table("uniform2d", "drawn", True))


# ---- yardsticks -------------------------------------------------------------------------------------------------------------------
def _yard_stream(reads, writes):
    def make():
        b, r = Built(), rng_of("yard_stream")
        n = 7 * 4096 * 4
        src = b.inp(r.standard_normal(n).astype(np.float32), r.standard_normal(n).astype(np.float32))
        dst = b.new((n // 7 * 2 if reads == 7 else n,), F32)
        b.call = lambda: list(ops().yard_stream(src, dst, reads, writes))
        return b
    return make


case("yard_stream_copy", "s3_yard_stream")(_yard_stream(1, 1))
case("yard_stream_7_2", "s3_yard_stream")(_yard_stream(7, 2))


# ---- the table --------------------------------------------------------------------------------------------------------------------
# entry point -> its cases.  Written out by hand on purpose: tests/test_stream_cases_table.py holds it against the header (every
# function with an s3_stream parameter) and against what the cases above say they cover, so a name dropped on either side fails.
TABLE = {
    "s3_memcpy_h2d": ("memcpy_h2d_pageable", "memcpy_h2d_pinned"),
    "s3_memcpy_d2h": ("memcpy_d2h_pageable", "memcpy_d2h_pinned"),
    "s3_download": ("to_host", "to_host_large", "download_on_stream"),
    "s3_upload_rows": ("upload_rows",),
    "s3_upload_rows_indexed": ("upload_rows_indexed",),
    "s3_upload_row_pieces": ("upload_row_pieces", "upload_row_pieces_rows"),
    "s3_knn_create": ("knn_create_3d", "knn_create_2d_refined"),
    "s3_knn_set_values": ("knn_set_values",),
    "s3_knn_query": ("knn_query_2d_ties", "knn_query_3d", "knn_query_2d_refined"),
    "s3_idw_predict": ("knn_predict_2d_ties", "knn_predict_3d", "knn_predict_2d_refined"),
    "s3_make_children": ("make_children",),
    "s3_child_gain": ("child_gain_2d", "child_gain_3d"),
    "s3_child_gain_reuse": ("child_gain_reuse_root", "child_gain_reuse_parents_2d", "child_gain_reuse_parents_3d", "child_gain_reuse_parents_k49"),
    "s3_mask_box": ("mask_box",),
    "s3_mask_sphere": ("mask_sphere",),
    "s3_mask_cylinder": ("mask_cylinder",),
    "s3_mask_polygon": ("mask_polygon",),
    "s3_mask_triangle": ("mask_triangle",),
    "s3_mask_prism": ("mask_prism",),
    "s3_mask_tetrahedra": ("mask_tetrahedra",),
    "s3_mask_mesh": ("mask_mesh",),
    "s3_commit_batch": ("commit_batch",),
    "s3_sumsq_leaf": ("sumsq_leaf",),
    "s3_sumsq_blocks": ("sumsq_blocks",),
    "s3_sum_ordered": ("sum_ordered",),
    "s3_topn_leaf": ("topn_leaf",),
    "s3_idw_weights": ("idw_weights",),
    "s3_idw_weights_exact": ("idw_weights_exact",),
    "s3_interp": ("interp_f32", "interp_f64"),
    "s3_snapshot_major": ("snapshot_major",),
    "s3_snapshot_major_as": ("snapshot_major_as_f32",),
    "s3_snapshot_major_rows": ("snapshot_major_rows",),
    "s3_snapshot_major_rows_as": ("snapshot_major_rows_as_f32",),
    "s3_cell_major": ("cell_major_f32_f64", "cell_major_f64_f32"),
    "s3_row_moments": ("row_moments_f32", "row_moments_f64"),
    "s3_row_abs_moments": ("row_abs_moments_f32", "row_abs_moments_f64"),
    "s3_interp_plan_create": ("plan_create", "plan_create_no_centers", "plan_cost_profile"),
    "s3_interp_plan_partition": ("plan_partition",),
    "s3_interp_plan_cost_profile": ("plan_cost_profile",),
    "s3_interp_plan_set_weights": ("plan_set_weights",),
    "s3_interp_planned": ("plan_interp_stream", "plan_interp_shift", "plan_interp_short"),
    "s3_interp_plan_set_source_ids": ("plan_set_source_ids",),
    "s3_interp_planned_src": ("plan_src_stream", "plan_src_short"),
    "s3_recon_error": ("recon_error", "recon_error_rows_scale"),
    "s3_grad_coeff": ("grad_coeff_2d", "grad_coeff_3d_rows"),
    "s3_grad_apply": ("grad_apply_gradient", "grad_apply_magnitude", "grad_apply_divergence", "grad_apply_vorticity",
                      "grad_apply_vorticity_magnitude", "grad_apply_q"),
    "s3_cell_index": ("cell_index_2d", "cell_index_3d", "cell_neighbours_2d", "cell_neighbours_3d"),
    "s3_cell_locate": ("cell_locate_2d", "cell_locate_3d_rows"),
    "s3_cell_sample": ("cell_sample_cell_2d", "cell_sample_linear_3d", "cell_sample_linear_2d"),
    "s3_trace": ("trace_stream_2d", "trace_stream_3d", "trace_path_2d", "trace_path_3d"),
    "s3_iso_count": ("iso_count_2d", "iso_count_3d", "iso_extract_3d"),
    "s3_iso_emit": ("iso_emit_2d", "iso_emit_3d", "iso_extract_3d"),
    "s3_cell_neighbours": ("cell_neighbours_2d", "cell_neighbours_3d"),
    "s3_region_label": ("region_label_2d", "region_label_3d_order"),
    "s3_region_count": ("region_table_2d", "region_table_3d_weight", "region_table_big_regions"),
    "s3_region_emit": ("region_table_2d", "region_table_3d_weight", "region_table_big_regions"),
    "s3_yard_stream": ("yard_stream_copy", "yard_stream_7_2"),
    "s3_yard_plan_loads": ("yard_plan_loads",),
    "s3_mark_rows": ("referenced_rows", "referenced_rows_hilbert"),
    "s3_compact_rows": ("referenced_rows", "referenced_rows_hilbert"),
    "s3_remap_indices": ("remap_indices",),
    "s3_spatial_order": ("spatial_order_2d", "spatial_order_3d", "referenced_rows_hilbert"),
    "s3_exclusive_scan": ("exclusive_scan_i32", "exclusive_scan_i64", "iso_extract_3d", "region_table_2d", "region_table_3d_weight",
                          "region_table_big_regions"),
    "s3_sort_pairs": ("sort_pairs", "cell_index_2d", "cell_index_3d"),
    "s3_positions_of": ("positions_of", "referenced_rows_hilbert"),
    "s3_gather_rows": ("gather_rows_repitch", "referenced_rows_hilbert"),
    "s3_weighted_gram": ("weighted_gram",),
    "s3_centered_gemm": ("centered_gemm_modes", "centered_gemm_residual"),
    "s3_gram": ("gram_f32", "gram_f64", "gram_f32_mean_weight", "gram_f64_mean_weight"),
    "s3_tall_gemm": ("tall_gemm_f32", "tall_gemm_f64"),
    "s3_segment_dft": ("segment_dft_f32", "segment_dft_f64_mean"),
    "s3_segment_psd": ("segment_psd_f32_mean", "segment_psd_f64"),
    "s3_sym_eig": ("sym_eig",),
}

# streamed entry points without a case, and why.  Only these kinds are allowed (the CPU test says which): the wait itself, the
# collectives (they need a communicator of several ranks and run in child processes: tests/test_parallel_gloo.py and the multi-GPU
# tests), and entry points shown to synchronise the whole device before their FIRST launch -- ``csrc/<file>: <function>: "<statement>"``,
# which the CPU test looks up -- of which there is none today.  (SIDE_ONLY above is something else: cases of an entry point that HAS
# cases in the table, whose own control cannot differ; their reasons are cited and looked up the same way.)
NOT_CASES = {
    "s3_stream_synchronize": "the wait itself: every case with a host result goes through a wait on the given stream",
    "s3_comm_allgather_inplace": "collective: needs a communicator, runs in child processes",
    "s3_comm_gather_to_root": "collective: needs a communicator, runs in child processes",
    "s3_comm_allreduce_f64": "collective: needs a communicator, runs in child processes",
}
