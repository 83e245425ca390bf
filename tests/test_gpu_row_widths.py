"""
Every (kernel family, element type, load width) that libs3hip.so instantiates for rows read where they lie, launched at least once.

The width is a launch-time choice made from the layout alone (csrc/: the entry points of metric.hip, export.hip, recon.hip,
differential.hip, svd.hip and spectral.hip), so the layout is what the cases vary: a view that starts 0, 1 or 2 elements into a
256-byte-aligned flat allocation, even and odd row lengths and pitches, and for the segment DFT the parity of the hop.  ``*_width``
below restate the rule of each entry point; ``test_every_width_of_every_family_is_launched`` holds the cases to the full set.

What is asserted:
* ``s3_interp`` and ``s3_grad_apply`` ("gradient", "q") sum per element in an order that does not depend on the width: all layouts of
  float32 and of its float64 copy give the same bits.  The interpolation is also held to the long-double sum (tests/recon_cases.py)
  within the bound of tests/test_gpu_recon.py.
* ``s3_gram``, ``s3_tall_gemm``, ``s3_segment_dft`` and ``s3_segment_psd`` widen float32 in the staging: float32 in every layout gives the
  bits of the same call on the ``.double()`` copy.
* the moments are grouped by width, so they are held to references instead: ``s3_row_moments`` / ``s3_row_abs_moments`` to the per-row
  bounds of tests/moments_cases.py, ``s3_recon_error`` to the bound of tests/test_gpu_recon.py's long-double checker.
* NaN fills the elements before, between and behind the rows of every input view and the zones around every output: no result is NaN
  and the zones keep their bytes.

Shapes: a cloud of 1100 points (more than one reduction block of 1024 points and more than four gradient blocks of 256, the last one
partial) on 257 rows; 5 and 26 neighbours (the unrolled part of the gather loops skipped and taken); rows of 1, 6, 8 and 100 columns
and one of 300 (several chunks at 64 lanes per point); matrices of 257 rows with 8 and 33 columns, segments of 8 samples 3 and 4 apart.
"""
import ctypes as C

import numpy as np
import pytest
import torch as pt

from tests import moments_cases as mc
from tests import recon_cases as rc
from tests import test_gpu_moments as tgm          # moments(): one guarded call of the entry point
from tests import test_gpu_recon as tgr            # check(): the bound of the long-double checker

pytestmark = pytest.mark.gpu

F32, F64 = pt.float32, pt.float64
DTYPES = (F32, F64)
ITEM = {F32: 4, F64: 8}
N_CLOUD, N_ROWS = 1100, 257
CLOUD_CASES = [(k, row_len) for k in (5, 26) for row_len in (1, 6, 8, 100)] + [(26, 300)]
MATRIX_T = (8, 33)
NPERSEG, HOPS = 8, (3, 4)
GUARD = 64                                                   # NaN elements around every output and behind every input
NAN_BITS = int(np.array([np.nan]).view(np.int64)[0])


@pytest.fixture(scope="module")
def ops():
    from sparsespatialsampling_amd import hipops
    hipops.device()
    return hipops


def pitch_for(t, residue):
    """smallest row pitch >= t with pitch % 4 == residue (residue None: the smallest odd one)"""
    p = t
    while (p % 2 != 1) if residue is None else (p % 4 != residue):
        p += 1
    return p


def flat_view(dense, offset, pitch=None):
    """the host tensor ``dense`` [n, ...] on the device, its rows ``pitch`` elements apart (None: dense), the first one ``offset``
    elements into a 256-byte-aligned flat allocation; every other element of the allocation is NaN"""
    n, t = int(dense.shape[0]), int(np.prod(dense.shape[1:]))
    pitch = t if pitch is None else pitch
    buf = pt.full((offset + n * pitch + GUARD,), float("nan"), dtype=dense.dtype)
    buf[offset:offset + n * pitch].view(n, pitch)[:, :t] = dense.reshape(n, t)
    flat = buf.cuda()
    assert flat.data_ptr() % 256 == 0
    view = flat[offset:offset + n * pitch].view(n, pitch)[:, :t]
    return view.view(dense.shape) if pitch == t else view


class Guarded:
    """a float64 output of ``shape`` that starts ``offset`` doubles past a 256-byte boundary, NaN zones on both sides"""

    def __init__(self, shape, offset=0):
        self.shape, self.size, self.lo = tuple(shape), int(np.prod(shape)), GUARD + offset
        self.buf = pt.full((self.lo + self.size + GUARD,), float("nan"), dtype=F64, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.out = self.buf[self.lo:self.lo + self.size].view(self.shape)

    def result(self, what):
        host = self.buf.cpu()
        bits = host.view(pt.int64)
        assert bool((bits[:self.lo] == NAN_BITS).all()) and bool((bits[self.lo + self.size:] == NAN_BITS).all()), f"{what}: a write outside the output"
        got = host[self.lo:self.lo + self.size].view(self.shape).clone()
        assert not bool(pt.isnan(got).any()), f"{what}: NaN in the result"
        return got


def same_bits(a, b):
    return a.shape == b.shape and bool(pt.equal(a.contiguous().view(pt.int64), b.contiguous().view(pt.int64)))


def widest(itemsize, widths, byte_quantities):
    """the widest of ``widths`` (descending, 1 last) whose load size divides every one of ``byte_quantities``"""
    for v in widths:
        if all(q % (v * itemsize) == 0 for q in byte_quantities):
            return v
    return 1


# ---- the rule of each entry point, restated -----------------------------------------------------------------------------------
def moments_width(dtype, stride, offset):
    return mc.kernel_vec(ITEM[dtype], stride, offset * ITEM[dtype])


def interp_width(dtype, row_len, in_offset, out_offset):
    if (out_offset * 8) % 16:
        return 1
    return widest(ITEM[dtype], (4, 2) if dtype == F32 else (2,), (row_len * ITEM[dtype], in_offset * ITEM[dtype]))


def recon_width(dtype, row_len, offset):
    return widest(ITEM[dtype], (4,) if dtype == F32 else (2,), (row_len * ITEM[dtype], offset * ITEM[dtype]))


def grad_width(dtype, row_len, stride, offset):
    return widest(ITEM[dtype], (4,) if dtype == F32 else (2,), (row_len * ITEM[dtype], stride * ITEM[dtype], offset * ITEM[dtype]))


def matrix_width(dtype, stride, offset, hop=0):
    return widest(4, (4, 2), (stride * 4, offset * 4, hop * 4)) if dtype == F32 else 1


# ---- the layouts --------------------------------------------------------------------------------------------------------------
INTERP_LAYOUTS = ((0, 0), (1, 0), (2, 0), (0, 1))            # (elements the table starts into its allocation, doubles the output does)
RECON_OFFSETS = (0, 1, 2)


def row_layouts(t):
    """(offset, pitch) of pitched rows of ``t`` elements: dense, 16-byte pitch at offsets 0 / 1 / 2, a pitch of 8 bytes modulo 16, an odd one"""
    p0 = pitch_for(t, 0)
    return ((0, t), (0, p0), (1, p0), (2, p0), (0, pitch_for(t, 2)), (0, pitch_for(t, None)))


def segments(t):
    """(hop, n_blk) of the segment cases on rows of ``t`` samples: three segments where they fit, else one (whose hop does not count)"""
    return [(hop, 3 if 2 * hop + NPERSEG <= t else 1) for hop in HOPS]


def test_every_width_of_every_family_is_launched():
    seen = {}

    def note(family, dtype, width):
        seen.setdefault((family, dtype), set()).add(width)

    for dtype in DTYPES:
        for _, row_len in CLOUD_CASES:
            for layout in INTERP_LAYOUTS:
                note("interp", dtype, interp_width(dtype, row_len, *layout))
            for offset in RECON_OFFSETS:
                note("recon", dtype, recon_width(dtype, row_len, offset))
            for offset, pitch in row_layouts(row_len):
                note("grad", dtype, grad_width(dtype, row_len, pitch, offset))
                note("moments", dtype, moments_width(dtype, pitch, offset))
            for dim in (2, 3):
                for offset in RECON_OFFSETS:
                    note("grad q", dtype, grad_width(dtype, row_len, dim * row_len, offset))
        for t in MATRIX_T:
            for offset, pitch in row_layouts(t):
                note("matrix", dtype, matrix_width(dtype, pitch, offset))
                for hop, n_blk in segments(t):
                    note("segments", dtype, matrix_width(dtype, pitch, offset, hop if n_blk > 1 else 0))
    for family, f32, f64 in (("moments", {4, 2, 1}, {2, 1}), ("interp", {4, 2, 1}, {2, 1}), ("recon", {4, 1}, {2, 1}), ("grad", {4, 1}, {2, 1}),
                             ("grad q", {4, 1}, {2, 1}), ("matrix", {4, 2, 1}, {1}), ("segments", {4, 2, 1}, {1})):
        assert seen[(family, F32)] == f32 and seen[(family, F64)] == f64, (family, seen[(family, F32)], seen[(family, F64)])


# ---- interpolation and reconstruction error: one table per case ---------------------------------------------------------------
_CLOUD = {}


def cloud_case(k, row_len):
    """weights / ids of N_CLOUD points on N_ROWS grid rows, grid and original fields whose values are float32 numbers (so the float64
    copy holds the same values), and the long-double references, once per case"""
    if (k, row_len) not in _CLOUD:
        rng = np.random.default_rng(1000 * k + row_len)
        w = rng.random((N_CLOUD, k)) + 0.05
        w /= w.sum(axis=1, keepdims=True)
        idx = rng.integers(0, N_ROWS, size=(N_CLOUD, k)).astype(np.int32)
        grid = (rng.standard_normal((N_ROWS, row_len)) + 1.5).astype(np.float32)
        orig = (rng.standard_normal((N_CLOUD, row_len)) + 1.5).astype(np.float32)
        scale = np.sqrt(rng.random(N_CLOUD) + 0.1)
        fit = rc.fitted(w, idx, grid)
        _CLOUD[(k, row_len)] = dict(w=w, idx=idx, grid=pt.from_numpy(grid), orig=pt.from_numpy(orig), scale=scale, fit=fit,
                                    moments=rc.moments(fit, orig, scale))
    return _CLOUD[(k, row_len)]


@pytest.mark.parametrize("k,row_len", CLOUD_CASES)
def test_interp_gives_the_same_bits_at_every_width(ops, k, row_len):
    case = cloud_case(k, row_len)
    w, idx = tgr.dev(case["w"]), tgr.dev(case["idx"])
    base = None
    for dtype in DTYPES:
        for in_offset, out_offset in INTERP_LAYOUTS:
            what = f"interp k {k} row_len {row_len} {dtype} table +{in_offset} output +{out_offset}"
            out = Guarded((N_CLOUD, row_len), out_offset)
            ops.interp(w, idx, flat_view(case["grid"].to(dtype), in_offset), out=out.out)
            got = out.result(what)
            base = got if base is None else base
            assert same_bits(got, base), what
    tgr.check("interp", base.numpy(), case["fit"], f"interp k {k} row_len {row_len}")


def recon_error(ops, w, idx, grid, orig, scale, what):
    """s3_recon_error as hipops.recon_error calls it, with all three outputs between NaN zones -> (mean, m2, colsum)"""
    from sparsespatialsampling_amd import _lib
    lib = _lib.hip_lib()
    n, k = (int(v) for v in w.shape)
    row_len, pitch = int(grid.shape[1]), int(orig.stride(0))
    outs = [Guarded((n,)), Guarded((n,)), Guarded((2, row_len))]
    scratch = pt.empty((lib.s3_recon_error_scratch_bytes(n, row_len) + 7) // 8, dtype=F64, device="cuda")
    ops.check(lib.s3_recon_error(ops._ptr(w), ops._ptr(idx), n, k, ops._ptr(grid), ops.DTYPE_CODE[grid.dtype], int(grid.shape[0]),
                                 C.c_void_p(orig.data_ptr()), ops.DTYPE_CODE[orig.dtype], n, pitch, row_len, None, ops._ptr(scale),
                                 *(ops._ptr(o.out) for o in outs), ops._ptr(scratch), ops._stream()), "s3_recon_error")
    return [o.result(what) for o in outs]


@pytest.mark.parametrize("k,row_len", CLOUD_CASES)
def test_recon_error_within_its_bound_at_every_width(ops, k, row_len):
    """grid float32 / float64 at offsets 0, 1 and 2 against original rows of either type, pitched and off every vector boundary"""
    case = cloud_case(k, row_len)
    w, idx, scale = tgr.dev(case["w"]), tgr.dev(case["idx"]), tgr.dev(case["scale"])
    for grid_dtype in DTYPES:
        for orig_dtype in DTYPES:
            orig = flat_view(case["orig"].to(orig_dtype), 1, row_len + 3)
            for offset in RECON_OFFSETS:
                what = f"recon k {k} row_len {row_len} grid {grid_dtype} +{offset} orig {orig_dtype}"
                mean, m2, colsum = recon_error(ops, w, idx, flat_view(case["grid"].to(grid_dtype), offset), orig, scale, what)
                for name, got, want in zip(("mean", "m2", "sum d^2", "sum ref^2"), (mean, m2, colsum[0], colsum[1]), case["moments"]):
                    tgr.check(name, got.numpy(), want, what)


# ---- gradients ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,row_len", CLOUD_CASES)
def test_grad_apply_gives_the_same_bits_at_every_width(ops, k, row_len):
    """"gradient" of a scalar field [n, T] in every row layout and "q" of a vector field [n, dim, T] at offsets 0, 1 and 2, float32 and
    its float64 copy, in 2-D and 3-D.  (The stencils are random numbers: what the sum is worth is test_gpu_differential.py's matter.)"""
    for dim in (2, 3):
        rng = np.random.default_rng(100 * k + row_len + dim)
        coef = tgr.dev(rng.standard_normal((N_CLOUD, k, dim)))
        idx = tgr.dev(rng.integers(0, N_CLOUD, size=(N_CLOUD, k)).astype(np.int32))
        scalar = pt.from_numpy((rng.standard_normal((N_CLOUD, row_len)) + 1.5).astype(np.float32))
        vector = pt.from_numpy((rng.standard_normal((N_CLOUD, dim, row_len)) + 1.5).astype(np.float32))
        for mode, field, layouts in (("gradient", scalar, row_layouts(row_len)), ("q", vector, [(o, None) for o in RECON_OFFSETS])):
            base = None
            for dtype in DTYPES:
                for offset, pitch in layouts:
                    what = f"{mode} dim {dim} k {k} row_len {row_len} {dtype} +{offset} pitch {pitch}"
                    out = Guarded((N_CLOUD, ops.grad_n_out(mode, dim, 1 if mode == "gradient" else dim), row_len))
                    ops.grad_apply(coef, idx, flat_view(field.to(dtype), offset, pitch), mode, out=out.out)
                    got = out.result(what)
                    base = got if base is None else base
                    assert same_bits(got, base), what


# ---- moments ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", sorted({row_len for _, row_len in CLOUD_CASES} | set(MATRIX_T)))
def test_row_moments_within_their_bounds_at_every_width(ops, t):
    ddof = 1 if t > 1 else 0                                                   # (one value and ddof 1: NaN is the answer)
    for dtype in DTYPES:
        x = mc.make_rows(N_ROWS, t, np.float32 if dtype == F32 else np.float64, 7 * t + ITEM[dtype])
        ref = {False: mc.reference(x), True: mc.reference(x, absolute=True)}
        for offset, pitch in row_layouts(t):
            view = flat_view(pt.from_numpy(x), offset, pitch)
            for absolute in (False, True):
                what = f"moments T {t} {dtype} +{offset} pitch {pitch} abs {absolute}"
                mean, std = tgm.moments(ops, view.data_ptr(), ITEM[dtype], N_ROWS, t, pitch, ddof, absolute=absolute)
                assert not np.isnan(mean).any() and not np.isnan(std).any(), what
                mc.assert_moments(mean, std, ref[absolute], ddof, what)


# ---- the matrix-core families ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", MATRIX_T)
def test_matrix_families_equal_their_double_copy_at_every_width(ops, t):
    from sparsespatialsampling_amd import spectral
    rng = np.random.default_rng(t)
    x = pt.from_numpy((rng.standard_normal((N_ROWS, t)) + 0.5).astype(np.float32))
    mean, weight = tgr.dev(x.double().mean(1).numpy()), tgr.dev(rng.random(N_ROWS) + 0.1)
    b = tgr.dev(rng.standard_normal((t, 5)))
    bre, bim, _ = spectral.segment_matrix(NPERSEG, "hann", "constant")
    bre, bim = tgr.dev(bre), tgr.dev(bim)
    n_f = int(bre.shape[1])
    scale = tgr.dev(rng.random(n_f) + 0.1)
    calls = [("gram", (t, t), lambda xd, out: ops.gram(xd, mean, weight, out=out)),
             ("tall_gemm", (N_ROWS, 5), lambda xd, out: ops.tall_gemm(xd, b, out=out))]
    for hop, n_blk in segments(t):
        calls.append((f"segment_dft hop {hop}", (N_ROWS, n_f, n_blk, 2),
                      lambda xd, out, hop=hop, n_blk=n_blk: ops.segment_dft(xd, mean, NPERSEG, hop, n_blk, bre, bim, out=out)))
        calls.append((f"segment_psd hop {hop}", (N_ROWS, n_f),
                      lambda xd, out, hop=hop, n_blk=n_blk: ops.segment_psd(xd, mean, NPERSEG, hop, n_blk, bre, bim, scale, out=out)))
    for name, shape, call in calls:
        for offset, pitch in row_layouts(t):
            got = {}
            for dtype in DTYPES:
                what = f"{name} T {t} {dtype} +{offset} pitch {pitch}"
                out = Guarded(shape)
                call(flat_view(x.to(dtype), offset, pitch), out.out)
                got[dtype] = out.result(what)
            assert same_bits(got[F32], got[F64]), f"{name} T {t} +{offset} pitch {pitch}"
