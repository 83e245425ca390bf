"""
Every route of the interpolation, judged per element against a long-double reference (tests/interp_accuracy.py) on
adversarial data.  GPU only.

What a case does, on every entry point that applies -- the direct kernel (``hipops.interp``, each of its vector widths the row
length allows), ``InterpPlan.interp`` (the plan's compacted rows) and ``InterpPlan.interp_src`` (the full table read in place):
  (a) every byte of the source allocation that is not a referenced element is NaN: pitch padding, rows before and after the
      table, rows no cell references;
  (b) the output is a view in the middle of a buffer of signalling NaNs: afterwards every output element is finite and every
      guard element keeps its bits (16-byte and, for odd row lengths, 8-byte output offsets);
  (c) in a second pass NaN / +Inf / -Inf are planted in referenced rows, one of them behind a weight of exactly 0 in an
      exact-hit cell: the output's NaN / Inf pattern equals the reference's and every other column still meets the bound.
The data mixes, by region of the domain, rows scaled by 10^U(-30, 30) (f32) / 10^U(-300, 300) (f64), f32 subnormals, values
near the top of the f32 range and rows with a large common offset.  Each case asserts the route ``InterpPlan.route`` reports;
test_every_declared_route_is_reached checks that the cases reach every route s3hip.h declares.
"""
import functools
import os
import re
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch as pt

from tests.interp_accuracy import GUARD_BITS, assert_close, reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from sparsespatialsampling_amd import hipops
    hipops.device()
    return hipops


# ---- neighbour tables ------------------------------------------------------------------------------------------------------
# KNN geometries: ``n`` points, ``nc`` cell centres (``sub``: in the middle of the domain, so that part of the points is never
# referenced); every 97th cell sits exactly on a point (an exact hit: its weights are made 1 / 0 as the reference's are).
GEOMS = {
    "g3_4201": dict(d=3, n=20_000, nc=4_201),          # > 64 tiles, not a multiple of the tile height
    "g2_4201": dict(d=2, n=20_000, nc=4_201),
    "g3_65": dict(d=3, n=400, nc=65),                  # two tiles, the second with one cell
    "g3_1": dict(d=3, n=3_000, nc=1),
    "g3_5000": dict(d=3, n=50_000, nc=5_000, sub=True),
    "g3_160k": dict(d=3, n=300_000, nc=160_000),       # >= 2048 tiles of 64 cells: the tail map
    "g2_280k": dict(d=2, n=300_000, nc=280_000),       # >= 2048 tiles of 128 cells
    "g3_big": dict(d=3, n=300_000, nc=4_201, sub=True),
    "rand": dict(n=9_000, nc=1_037),                   # arbitrary table: signed weights, repeated ids, zero weights, no centres
}


@functools.lru_cache(maxsize=None)
def geometry(name, k):
    """host arrays: pts [n, d] (None for an arbitrary table), centers, idx int64 [nc, k], w f64 [nc, k], plant sites: (cell, m)
    pairs with w[cell, m] == 0 exactly"""
    from sparsespatialsampling_amd import hipops as ops
    g = GEOMS[name]
    rng = np.random.default_rng(zlib.crc32(f"{name}/{k}".encode()))
    n, nc = g["n"], g["nc"]
    if name == "rand":
        base = (np.arange(nc) * 8) % (n - 300)
        idx = base[:, None] + rng.integers(0, 300, (nc, k))
        if k >= 4:
            idx[:, 3] = idx[:, 2]                                      # a repeated id inside a row
        w = rng.uniform(-1.0, 1.0, (nc, k))
        w[::7, 0] = 0.0
        w[::11] = 0.0
        w[::11, k - 1] = 1.0                                           # one-hot rows
        zero = [(c, 0) for c in range(0, nc, 7) if k > 1]
        return None, None, idx, w, zero
    d = g["d"]
    pts = rng.random((n, d))
    centers = rng.random((nc, d)) * 0.5 + 0.25 if g.get("sub") else rng.random((nc, d))
    hits = np.arange(0, nc, 97)
    centers[hits] = pts[rng.integers(0, n, len(hits))]
    if g.get("sub"):                                                   # hits inside the middle of the domain as well
        inner = np.nonzero(((pts > 0.3) & (pts < 0.7)).all(1))[0]
        centers[hits] = pts[rng.choice(inner, len(hits))]
    knn = ops.KnnIndex(pts)
    idx_d, dist_d = knn.query(centers, k)
    w = ops.idw_weights(dist_d).cpu().numpy()
    idx, dist = idx_d.cpu().numpy().astype(np.int64), dist_d.cpu().numpy()
    knn.close()
    exact = np.nonzero(dist.min(1) == 0.0)[0]
    assert len(exact) >= len(hits) // 2
    w[exact] = 0.0
    w[exact, dist[exact].argmin(1)] = 1.0
    zero = [(c, int((dist[c].argmin() + 1) % k)) for c in exact[:4] if k > 1]
    return pts, centers, idx, w, zero


def values(name, k, dtype, row_len, seed):
    """[n, row_len] host data: by region of the domain (by id block for the arbitrary table) scaled normal rows whose decade
    varies smoothly over the domain (-30 .. 30 for f32, -300 .. 300 for f64), subnormals, values near the top of the range and
    rows with a large common offset"""
    pts, _, _, _, _ = geometry(name, k)
    n = GEOMS[name]["n"]
    rng = np.random.default_rng(seed)
    f32 = dtype == pt.float32
    if pts is None:
        region = (np.arange(n) // 300) % 5
        field = np.sin(np.arange(n) / 500.0)
    else:
        region = np.floor(pts[:, 0] * 10).astype(int) % 5
        field = np.sin(3.0 * pts[:, 1] + 2.0 * pts[:, 0] + (pts[:, 2] if pts.shape[1] > 2 else 0.0))
    npt = np.float32 if f32 else np.float64
    decade = (29.0 if f32 else 299.0) * field + rng.uniform(-1.0, 1.0, n)
    x = rng.standard_normal((n, row_len), dtype=npt)
    x *= (10.0 ** decade).astype(npt)[:, None]
    for r, rows in ((1, np.nonzero(region == 1)[0]), (2, np.nonzero(region == 2)[0]), (3, np.nonzero(region == 3)[0])):
        shape = (len(rows), row_len)
        sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0).astype(npt)
        if r == 1:                  # subnormals: f32 1.4e-45 .. 1e-40; f64 below 2**-1034
            v = rng.integers(1, 71_362, shape, dtype=np.uint32).view(np.float32) if f32 else \
                rng.integers(1, 1 << 40, shape, dtype=np.int64).view(np.float64)
            v = sign * v
        elif r == 2:                # near the top of the range
            v = sign * rng.uniform(2.5e38, 3.4e38, shape).astype(npt) if f32 else sign * rng.uniform(1e306, 2e306, shape)
        else:                       # a large common offset
            c = 1e4 if f32 else 1e12
            v = (c * (1.0 + (1e-3 if f32 else 1e-6) * rng.standard_normal(shape))).astype(npt)
        x[rows] = v
    assert np.isfinite(x).all()
    return x


# ---- layouts of a source table in a NaN-filled allocation ------------------------------------------------------------------
def place(host, layout, dtype, fill=True):
    """``host`` [n, L] (rows never referenced hold NaN) -> a device view laid out as ``layout`` in an allocation whose other
    bytes are all 0xFF (NaN in f32 and f64).  ``fill=False``: the same view of an allocation that is not initialised."""
    n, L = host.shape
    e = pt.empty((), dtype=dtype).element_size()
    if layout == "pitched":
        from sparsespatialsampling_amd import hipops
        pitch = hipops.padded_rows(1, L, dtype, "cpu").stride(0)
    elif layout == "pitch+1":               # element-aligned rows in a pitch of whole elements
        pitch = L + 1
    elif layout == "big":                   # 4-KiB pitch: a table of more than 1 GiB
        pitch = 4096 // e
    else:
        pitch = L
    lead = 256 + (16 if layout == "offset16" else 0) + (8 if layout == "offset8" else 0)
    body = n * pitch * e
    if layout == "tail":                    # the table ends with its allocation (on a 128-byte boundary)
        lead += -(lead + body) % 128
        trail = 0
    else:
        trail = 256
    buf = pt.empty(lead + body + trail, dtype=pt.uint8, device="cuda")
    if fill:
        buf.fill_(0xFF)
    table = buf.view(dtype).as_strided((n, L), (pitch, 1), lead // e)
    if fill:
        table.copy_(pt.from_numpy(host).cuda())
    return table


def with_nan_rows(x, keep):
    """x with every row not in ``keep`` set to NaN"""
    y = np.full_like(x, np.nan)
    y[keep] = x[keep]
    return y


GUARD = 64


def guarded_out(nc, L, offset):
    """an [nc, L] f64 output starting ``offset`` elements after a 128-byte boundary, GUARD signalling NaNs on either side"""
    n = GUARD + offset + nc * L + GUARD
    bits = pt.full((n,), int(GUARD_BITS), dtype=pt.int64, device="cuda")
    lo = GUARD + offset
    return bits, bits.view(pt.float64)[lo:lo + nc * L].view(nc, L), lo, lo + nc * L


def check_guard(bits, lo, hi, what):
    changed = int((bits[:lo] != int(GUARD_BITS)).sum()) + int((bits[hi:] != int(GUARD_BITS)).sum())
    assert changed == 0, f"{what}: {changed} guard elements outside the output were changed"


# ---- the cases: one per route and form, f32 and f64 ------------------------------------------------------------------------
Case = namedtuple("Case", "name geom k tc dtype row_len layout entry route width even split tail")
F32, F64 = pt.float32, pt.float64
CASES = [
    # persistent kernel, element-aligned rows
    Case("stream_elem_f32_odd", "g3_4201", 26, 64, F32, 25, "dense", "interp", "stream_elem", 26, 0, 0, 0),
    Case("stream_elem_f32_even", "g2_4201", 8, 64, F32, 26, "dense", "src", "stream_elem", 8, 1, 0, 0),
    Case("stream_elem_f64_odd", "g3_4201", 26, 64, F64, 9, "tail", "src", "stream_elem", 26, 0, 0, 0),
    Case("stream_elem_f64_even", "g2_4201", 8, 64, F64, 10, "pitch+1", "interp", "stream_elem", 8, 1, 0, 0),
    Case("stream_elem_65cells", "g3_65", 26, 64, F32, 75, "dense", "interp", "stream_elem", 26, 0, 0, 0),
    Case("stream_elem_1cell", "g3_1", 8, 64, F32, 5, "dense", "interp", "stream_elem", 8, 0, 0, 0),
    # persistent kernel, 16-byte aligned rows
    Case("stream_wide_f32_even", "g3_4201", 26, 64, F32, 100, "pitched", "interp", "stream_wide", 26, 1, 0, 0),
    Case("stream_wide_f32_odd", "g2_4201", 8, 64, F32, 75, "pitched", "src", "stream_wide", 8, 0, 0, 0),
    Case("stream_wide_f64_odd", "g3_4201", 26, 64, F64, 33, "pitched", "interp", "stream_wide", 26, 0, 0, 0),
    Case("stream_wide_f64_offset16", "g2_4201", 8, 64, F64, 50, "offset16", "src", "stream_wide", 8, 1, 0, 0),
    Case("stream_narrow_f32", "g3_4201", 26, 64, F32, 13, "pitched", "interp", "stream_narrow", 26, 0, 0, 0),
    Case("stream_narrow_f32_even", "g2_4201", 8, 64, F32, 8, "dense", "src", "stream_narrow", 8, 1, 0, 0),
    Case("stream_narrow_f64", "g3_4201", 26, 64, F64, 7, "pitched", "src", "stream_narrow", 26, 0, 0, 0),
    Case("stream_narrow_f64_even", "g2_4201", 8, 64, F64, 6, "dense", "interp", "stream_narrow", 8, 1, 0, 0),
    # short rows
    Case("short_quad2_f32", "rand", 5, 64, F32, 16, "dense", "interp", "short_quad", 2, 0, 0, 0),
    Case("short_quad2_k1_f64", "rand", 1, 64, F64, 7, "pitched", "src", "short_quad", 2, 0, 0, 0),
    Case("short_quad7_f64", "rand", 20, 64, F64, 8, "dense", "src", "short_quad", 7, 0, 0, 0),
    Case("short_quad8_f32", "rand", 32, 64, F32, 15, "pitched", "interp", "short_quad", 8, 0, 0, 0),
    Case("short_quad7_big_table", "g3_big", 26, 64, F32, 16, "big", "src", "short_quad", 7, 0, 0, 0),
    Case("short_reg8_rowlen1", "rand", 1, 64, F32, 1, "pitched", "interp", "short_reg", 8, 0, 0, 0),
    Case("short_reg26_rowlen2_f64", "rand", 20, 64, F64, 2, "dense", "src", "short_reg", 26, 0, 0, 0),
    Case("short_reg32_f32", "rand", 29, 64, F32, 9, "pitched", "src", "short_reg", 32, 0, 0, 0),
    Case("short_reg26_65cells", "g3_65", 26, 64, F32, 2, "pitched", "interp", "short_reg", 26, 0, 0, 0),
    Case("short_k64_f32", "rand", 64, 64, F32, 1, "pitched", "src", "short", 0, 0, 0, 0),
    Case("short_k40_f64", "rand", 40, 64, F64, 4, "dense", "interp", "short", 0, 0, 0, 0),
    # rows off the 128-byte grid: the shift kernel
    Case("shift_plain_f32", "g3_65", 26, 64, F32, 20, "offset16", "interp", "shift", 0, 0, 0, 0),
    Case("shift_plain_f64", "g3_1", 8, 64, F64, 12, "offset16", "src", "shift", 0, 0, 0, 0),
    Case("shift_split_f32", "g3_5000", 26, 64, F32, 1000, "dense", "src", "shift", 0, 0, 1, 0),
    Case("shift_split_f64", "g3_5000", 26, 64, F64, 514, "dense", "interp", "shift", 0, 0, 1, 0),
    Case("shift_tail_8chunks", "g3_160k", 26, 64, F32, 252, "dense", "src", "shift", 0, 0, 0, 1),
    Case("shift_tail_9chunks", "g3_160k", 26, 64, F32, 260, "dense", "src", "shift", 0, 0, 0, 1),
    Case("shift_tail_13chunks", "g3_160k", 26, 64, F32, 404, "dense", "src", "shift", 0, 0, 0, 1),
    Case("shift_tail_f64", "g3_160k", 26, 64, F64, 130, "dense", "src", "shift", 0, 0, 0, 1),
    # rows on the grid: the chunk kernels
    Case("chunk64_plain_f32", "rand", 5, 64, F32, 32, "pitched", "interp", "chunk64", 0, 0, 0, 0),
    Case("chunk64_plain_f64", "rand", 9, 64, F64, 11, "pitched", "src", "chunk64", 0, 0, 0, 0),
    Case("chunk64_split_f32", "g3_4201", 26, 64, F32, 1001, "pitched", "interp", "chunk64", 0, 0, 1, 0),
    Case("chunk64_split_f64", "rand", 9, 64, F64, 250, "pitched", "src", "chunk64", 0, 0, 1, 0),
    Case("chunk64_tail_f32", "g3_160k", 9, 64, F32, 260, "pitched", "src", "chunk64", 0, 0, 0, 1),
    Case("chunk64_tail_f64", "g3_160k", 9, 64, F64, 130, "pitched", "interp", "chunk64", 0, 0, 0, 1),
    Case("chunk128_plain_f32", "g3_4201", 26, 128, F32, 3, "pitched", "interp", "chunk128", 0, 0, 0, 0),
    Case("chunk128_plain_f64", "g3_4201", 26, 128, F64, 16, "offset16", "src", "chunk128", 0, 0, 0, 0),
    Case("chunk128_split_f32", "g3_4201", 26, 128, F32, 1000, "dense", "src", "chunk128", 0, 0, 1, 0),
    Case("chunk128_split_f64", "g3_4201", 26, 128, F64, 250, "pitched", "interp", "chunk128", 0, 0, 1, 0),
    Case("chunk128_tail_f32", "g2_280k", 8, 128, F32, 260, "dense", "src", "chunk128", 0, 0, 0, 1),
    Case("chunk128_tail_f64", "g2_280k", 8, 128, F64, 130, "dense", "interp", "chunk128", 0, 0, 0, 1),
]


class Built:
    """the plan of a case over the referenced rows (compacted ids + source ids of the full table)"""

    def __init__(self, ops, case):
        pts, centers, idx, w, zero = geometry(case.geom, case.k)
        self.idx, self.w, self.zero = idx, w, zero
        self.n = GEOMS[case.geom]["n"]
        self.idx_d = pt.from_numpy(idx.astype(np.int32)).cuda()
        self.w_d = pt.from_numpy(w).cuda()
        used, remap = ops.referenced_rows([self.idx_d], self.n, coords=pts)
        self.used = used.contiguous()
        idx_c = self.idx_d.clone()
        ops.remap_indices(idx_c, remap)
        self.plan = ops.InterpPlan(idx_c, int(used.numel()), centers, tile_cells=case.tc)
        self.plan.set_weights(self.w_d)
        self.plan.set_source_ids(self.used, self.n)
        self.used_h = self.used.cpu().numpy().astype(np.int64)

    def close(self):
        self.plan.close()


def route_tuple(r):
    return (r["route"], r["width"], r["even"], int(r["gy"] > 1), r["tail"])


def expected_tuple(case):
    return (case.route, case.width, case.even, case.split, case.tail)


def header_routes():
    text = open(os.path.join(ROOT, "include", "s3hip.h")).read()
    return {name.lower(): int(v) for name, v in re.findall(r"#define\s+S3_ROUTE_([A-Z0-9_]+)\s+(\d+)", text)}


def table_for_route(b, case, fill_host=None):
    L, dtype = case.row_len, case.dtype
    n = b.n if case.entry == "src" else len(b.used_h)
    if fill_host is None:
        return place(np.empty((n, L), dtype=np.float32 if dtype == F32 else np.float64), case.layout, dtype, fill=False)
    return place(fill_host, case.layout, dtype)


def check_columns(nc, L, dtype):
    """all columns of small outputs; on large ones the first and last element of every 128-byte chunk, the last column and
    a few more"""
    if nc * L <= 2_000_000:
        return np.arange(L)
    epc = 128 // pt.empty((), dtype=dtype).element_size()
    starts = np.arange(0, L, epc)
    cols = np.concatenate([starts, np.minimum(starts + epc - 1, L - 1), [L - 1], np.arange(1, L, max(1, L // 5))])
    return np.unique(cols)


def run_entries(ops, b, case, x_full, cols, ref, mag, what, expect_finite):
    """every entry point on source data ``x_full`` [n, L]: (a) NaN outside the referenced elements, (b) guard zones around the
    output, results judged per element on ``cols``"""
    nc, L = b.w.shape[0], case.row_len
    f64 = case.dtype == F64
    x_nan = with_nan_rows(x_full, b.used_h)
    runs = []
    # the direct kernel: the full table, dense; input and output offsets pick its vector width (4 / 2 / 1 for f32, 2 / 1 for f64)
    for in_layout, out_off in (("dense", 2), ("offset8", 2), ("dense", 1)):
        table = place(x_nan, in_layout, case.dtype)
        runs.append((f"direct {in_layout} out+{out_off * 8}B", out_off, lambda out, t=table: ops.interp(b.w_d, b.idx_d, t, out=out)))
    compact = place(x_full[b.used_h], case.layout, case.dtype)
    full = place(x_nan, case.layout, case.dtype)
    for out_off in ((2, 1) if L % 2 else (2,)):
        runs.append((f"interp {case.layout} out+{out_off * 8}B", out_off, lambda out, t=compact: b.plan.interp(b.w_d, t, out=out)))
        runs.append((f"interp_src {case.layout} out+{out_off * 8}B", out_off, lambda out, t=full: b.plan.interp_src(t, out=out)))
    for label, out_off, fn in runs:
        bits, out, lo, hi = guarded_out(nc, L, out_off)
        fn(out)
        pt.cuda.synchronize()
        check_guard(bits, lo, hi, f"{case.name} {what} {label}")
        if expect_finite:
            n_bad = int((~pt.isfinite(out)).sum())
            assert n_bad == 0, f"{case.name} {what} {label}: {n_bad} output elements are not finite"
        got = out[:, pt.from_numpy(cols).cuda()].cpu().numpy()
        assert_close(got, ref, mag, case.k, f64_data=f64, what=f"{case.name} {what} {label}", cols=cols)


def plant(b, case, x, rng):
    """NaN / +Inf / -Inf at chosen (row, column) positions of referenced rows, one NaN behind a zero weight of an exact-hit
    (or zero-weight) cell -> (poisoned copy, planted columns, rows)"""
    L = case.row_len
    y = x.copy()
    sites = []
    for c, m in b.zero[:2]:
        sites.append((int(b.idx[c, m]), int(rng.integers(0, L)), np.nan))
    rows = rng.choice(b.used_h, 3, replace=False) if len(b.used_h) >= 3 else np.resize(b.used_h, 3)
    sites += [(int(rows[0]), 0, np.inf), (int(rows[1]), L - 1, -np.inf), (int(rows[2]), L // 2, np.nan)]
    if len(b.used_h) >= 5:                                   # +Inf and -Inf in the same column of two rows: NaN where both meet
        r2 = rng.choice(b.used_h, 2, replace=False)
        j = int(rng.integers(0, L))
        sites += [(int(r2[0]), j, np.inf), (int(r2[1]), j, -np.inf)]
    for r, j, v in sites:
        y[r, j] = v
    return y, sorted({j for _, j, _ in sites}), sorted({r for r, _, _ in sites})


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_route_matches_long_double_reference(ops, case):
    b = Built(ops, case)
    try:
        nc, L = b.w.shape[0], case.row_len
        rng = np.random.default_rng(zlib.crc32(case.name.encode()))
        x = values(case.geom, case.k, case.dtype, L, zlib.crc32(case.name.encode()) + 1)
        # the route this case is meant to reach, on the layout of its entry point
        probe = table_for_route(b, case)
        assert route_tuple(b.plan.route(probe, src=case.entry == "src")) == expected_tuple(case), case
        del probe
        x_p, planted_cols, planted_rows = plant(b, case, x, rng)
        cols = np.unique(np.concatenate([check_columns(nc, L, case.dtype), planted_cols]))
        ref, mag = reference(b.w, b.idx, x, cols=cols)
        run_entries(ops, b, case, x, cols, ref, mag, "clean", expect_finite=True)
        # (c) the poisoned pass: the reference changes only in the cells that reference a planted row
        hit = np.nonzero(np.isin(b.idx, planted_rows).any(1))[0]
        ref_p, mag_p = reference(b.w, b.idx, x_p, cells=hit, cols=cols)
        ref[hit], mag[hit] = ref_p, mag_p
        assert (~np.isfinite(ref_p)).any()
        run_entries(ops, b, case, x_p, cols, ref, mag, "poisoned", expect_finite=False)
    finally:
        b.close()


# the template widths / forms of every route that the cases above must reach
REQUIRED_FORMS = {
    ("stream_elem", 8), ("stream_elem", 26), ("stream_wide", 8), ("stream_wide", 26), ("stream_narrow", 8), ("stream_narrow", 26),
    ("short_quad", 2), ("short_quad", 7), ("short_quad", 8), ("short_reg", 8), ("short_reg", 26), ("short_reg", 32),
}


def test_every_declared_route_is_reached(ops):
    """the plans of all cases, queried only (s3_interp_plan_route launches nothing): every route s3hip.h declares is reached, in
    f32 and in f64, with every template width, both EVEN forms of the persistent kernel and every launch form (plain, column
    split, tail map) of the shift and chunk kernels -- whatever other tests ran before"""
    declared = header_routes()
    assert set(declared) == set(ops.InterpPlan.ROUTES.values())
    assert {v: k for k, v in declared.items()} == ops.InterpPlan.ROUTES
    reached = set()
    for case in CASES:
        b = Built(ops, case)
        try:
            r = b.plan.route(table_for_route(b, case), src=case.entry == "src")
        finally:
            b.close()
        assert route_tuple(r) == expected_tuple(case), (case.name, r)
        reached.add((r["route"], case.dtype, r["width"], r["even"], r["gy"] > 1, r["tail"]))
    for name in declared:
        for dtype in (F32, F64):
            assert any(t[0] == name and t[1] == dtype for t in reached), f"route {name} not reached with {dtype}"
    forms = {(t[0], t[2]) for t in reached}
    assert REQUIRED_FORMS <= forms, REQUIRED_FORMS - forms
    for even in (0, 1):
        assert any(t[0] == "stream_elem" and t[3] == even for t in reached)
    for name in ("shift", "chunk64", "chunk128"):
        for form in ((False, 0), (True, 0), (False, 1)):
            assert any(t[0] == name and (t[4], t[5]) == form for t in reached), (name, form)


def test_route_query_launches_nothing_and_refuses_what_the_launch_refuses(ops):
    """the query needs no weights, reports the same refusals as the launch and leaves the stream idle"""
    from sparsespatialsampling_amd._lib import S3HipError
    pts, centers, idx, w, _ = geometry("rand", 5)
    plan = ops.InterpPlan(pt.from_numpy(idx.astype(np.int32)).cuda(), GEOMS["rand"]["n"], None)
    try:
        data = pt.empty((GEOMS["rand"]["n"], 25), dtype=pt.float32, device="cuda")
        with pytest.raises(TypeError):              # dense ragged rows need k = 8 | 26
            plan.route(data)
        rows = pt.empty((GEOMS["rand"]["n"], 24), dtype=pt.float32, device="cuda")
        with pytest.raises(RuntimeError):           # no source ids
            plan.route(rows, src=True)
        assert plan.route(rows)["route"] == "shift"                 # 96-byte rows off the line grid, 64-cell tiles
        from sparsespatialsampling_amd import _lib
        import ctypes as C
        h = (C.c_int32 * 5)()
        with pytest.raises(S3HipError):
            _lib.check(_lib.hip_lib().s3_interp_plan_route(plan._handle, 0, C.c_void_p(data.data_ptr()), 0, 0, 0, h), "route")
    finally:
        plan.close()
