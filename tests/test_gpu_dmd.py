"""The typed Gram / tall-GEMM entry points (s3_gram, s3_tall_gemm: csrc/svd.hip) and the DMD built on them
(sparsespatialsampling_amd/dmd.py) on the GPU: bit parity between float32 input and its float64 copy and between the new and the
float64-only entry points, long-double sums per element, canaries, and the DMD of every case of tests/dmd_cases.py against the
direct CPU reference and the planted dynamics; the centred / weighted forms (s3_weighted_gram, s3_gram with mean and weight,
s3_centered_gemm with lmean and with minus_from) per element against long double within the bounds of tests/centered_cases.py."""
import ctypes as C
import logging

import numpy as np
import pytest
import torch as pt

from tests import centered_cases as cc
from tests import dmd_cases as dc

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = dc.EPS
SHAPES_N = [1, 15, 17, 257, 3000]
SHAPES_T = [3, 17, 33, 130]
LAYOUTS = ["contiguous", "pitch16", "odd"]


@pytest.fixture(scope="module")
def ops():
    from sparsespatialsampling_amd import hipops
    hipops.device()
    return hipops


def device_matrix(dense, layout, offset=0):
    """device tensor with the values of the host matrix ``dense`` in the row layout ``layout``, starting ``offset`` elements into its
    buffer (offset 1: the first row is only element-aligned)"""
    n, t = dense.shape
    stride = dc.layout_stride(t, layout, dense.element_size())
    buf = pt.full((n * stride + offset,), float("nan"), dtype=dense.dtype)
    view = buf[offset:].reshape(n, stride)[:, :t]
    view.copy_(dense)
    return buf.cuda()[offset:].reshape(n, stride)[:, :t]


_GRAM_INPUT = {}


def gram_input(n, t):
    """float32 matrix [n, t] with its long-double Gram matrices (plain, and of |x|), computed once per shape"""
    if (n, t) not in _GRAM_INPUT:
        rng = np.random.default_rng(7 * n + t)
        x = (rng.standard_normal((n, t)) * (1 + 0.01 * np.arange(t))[None, :] + rng.standard_normal((n, 1))).astype(np.float32)
        xl = x.astype(LD)
        _GRAM_INPUT[(n, t)] = (pt.from_numpy(x), xl.T @ xl, np.abs(xl).T @ np.abs(xl))
    return _GRAM_INPUT[(n, t)]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(pt.equal(a.cpu().contiguous().view(pt.int64), b.cpu().contiguous().view(pt.int64)))


# ---- s3_gram ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", SHAPES_T)
@pytest.mark.parametrize("n", SHAPES_N)
def test_gram_f32_equals_its_double_copy_and_the_long_double_sum(ops, n, t):
    """float32 input in every row layout and alignment == the ``.double()`` copy, to the bit; symmetric to the bit; the same bits
    on a second run; each element within (N + 2) eps sum |terms| of the long-double sum"""
    x, ref, ref_abs = gram_input(n, t)
    want = ops.gram(x.double().cuda())
    assert same_bits(want, want.T.contiguous())
    got = (want.cpu().numpy().astype(LD) - ref)
    assert (np.abs(got) <= (n + 2) * EPS * ref_abs).all(), float((np.abs(got) / ref_abs).max() / EPS)
    for layout in LAYOUTS:
        for offset in (0, 1):
            xd = device_matrix(x, layout, offset)
            g = ops.gram(xd)
            assert same_bits(g, want), (layout, offset)
            assert same_bits(ops.gram(xd), g)
    for layout in ("pitch16", "odd"):
        assert same_bits(ops.gram(device_matrix(x.double(), layout)), want), layout


@pytest.mark.parametrize("n,t,pitch", [(3000, 130, 2), (257, 33, 0), (17, 3, 1)])
def test_gram_with_mean_and_weight_equals_weighted_gram(ops, n, t, pitch):
    from sparsespatialsampling_amd import svd
    rng = np.random.default_rng(n + t)
    x = pt.from_numpy(rng.standard_normal((n, t + pitch)) + 2.0).cuda()[:, :t]
    mean, weight = x.mean(1), pt.from_numpy(rng.random(n) + 0.1).cuda()
    assert same_bits(ops.gram(x, mean, weight), svd.weighted_gram(x, mean, weight))
    # float32 with mean and weight: widened BEFORE centring and weighting
    xf = x.float()
    assert same_bits(ops.gram(xf, mean, weight), ops.gram(xf.double(), mean, weight))
    only_w = ops.gram(x, None, weight).cpu()
    ref = (x.cpu() * weight.cpu().sqrt()[:, None])
    assert (only_w - ref.T @ ref).abs().max() <= 1e-12 * (ref.T @ ref).abs().max()


def test_weighted_gram_still_rejects_a_null_mean(ops):
    from sparsespatialsampling_amd import _lib
    x = pt.zeros((20, 4), dtype=pt.float64, device="cuda")
    g = pt.zeros((4, 4), dtype=pt.float64, device="cuda")
    lib = _lib.hip_lib()
    scratch = pt.zeros(int(lib.s3_weighted_gram_scratch_bytes(20, 4)), dtype=pt.uint8, device="cuda")
    w = pt.ones(20, dtype=pt.float64, device="cuda")
    rc = lib.s3_weighted_gram(C.c_void_p(x.data_ptr()), 20, 4, 4, C.c_void_p(0), C.c_void_p(w.data_ptr()), C.c_void_p(g.data_ptr()),
                              C.c_void_p(scratch.data_ptr()), ops._stream())
    assert rc != 0
    rc = lib.s3_gram(C.c_void_p(x.data_ptr()), 7, 20, 4, 4, C.c_void_p(0), C.c_void_p(0), C.c_void_p(g.data_ptr()),
                     C.c_void_p(scratch.data_ptr()), ops._stream())
    assert rc != 0                                                                # dtype code 7


@pytest.mark.parametrize("n,t", [(1, 3), (17, 17), (257, 33), (3000, 130)])
def test_gram_leaves_the_bytes_around_its_outputs_alone(ops, n, t):
    from sparsespatialsampling_amd import _lib
    x, _, _ = gram_input(n, t)
    xd = device_matrix(x, "odd", 1)
    need = int(_lib.hip_lib().s3_gram_scratch_bytes(n, t))
    guard = 512                                                                   # doubles on each side
    words = (need + 7) // 8
    g_buf = pt.full((guard + t * t + guard,), -7.25, dtype=pt.float64, device="cuda")
    s_buf = pt.full((guard + words + guard,), -7.25, dtype=pt.float64, device="cuda")
    g = ops.gram(xd, out=g_buf[guard:guard + t * t].view(t, t), scratch=s_buf[guard:guard + words])
    ops.synchronize()
    assert same_bits(g, ops.gram(xd))
    for buf, size in ((g_buf, t * t), (s_buf, words)):
        assert bool((buf[:guard] == -7.25).all()) and bool((buf[guard + size:] == -7.25).all())


# ---- s3_tall_gemm -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 64, 65, 80])
@pytest.mark.parametrize("m", [1, 15, 17, 257])
def test_tall_gemm_parity_and_long_double_sum(ops, m, n):
    """float32 == its ``.double()`` copy to the bit in every layout; float64 == s3_centered_gemm without means to the bit; each
    element within (k + 2) eps sum |terms| of the long-double product; inner dimensions below, across and above the 16-column step"""
    from sparsespatialsampling_amd import svd
    for k in (3, 17, 130):
        rng = np.random.default_rng(m + 31 * n + k)
        left = pt.from_numpy((rng.standard_normal((m, k)) + 1.0).astype(np.float32))
        b = pt.from_numpy(rng.standard_normal((k, n)))
        ll, bl = left.numpy().astype(LD), b.numpy().astype(LD)
        ref, ref_abs = ll @ bl, np.abs(ll) @ np.abs(bl)
        bd = b.cuda()
        want = ops.tall_gemm(left.double().cuda(), bd)
        assert want.shape == (m, n) and same_bits(want, svd.centered_gemm(left.double().cuda(), None, bd))
        err = np.abs(want.cpu().numpy().astype(LD) - ref)
        assert (err <= (k + 2) * EPS * ref_abs).all(), float((err / ref_abs).max() / EPS)
        for layout in LAYOUTS:
            for offset in (0, 1):
                assert same_bits(ops.tall_gemm(device_matrix(left, layout, offset), bd), want), (k, layout, offset)
        assert same_bits(ops.tall_gemm(device_matrix(left.double(), "odd"), bd), want)


def test_tall_gemm_leaves_the_bytes_around_its_output_alone(ops):
    m, k, n = 257, 33, 65
    rng = np.random.default_rng(3)
    left = device_matrix(pt.from_numpy(rng.standard_normal((m, k)).astype(np.float32)), "odd", 1)
    b = pt.from_numpy(rng.standard_normal((k, n))).cuda()
    guard = 512
    buf = pt.full((guard + m * n + guard,), -7.25, dtype=pt.float64, device="cuda")
    out = ops.tall_gemm(left, b, out=buf[guard:guard + m * n].view(m, n))
    ops.synchronize()
    assert same_bits(out, ops.tall_gemm(left, b))
    assert bool((buf[:guard] == -7.25).all()) and bool((buf[guard + m * n:] == -7.25).all())


# ---- DMD against the CPU reference and the planted dynamics ---------------------------------------------------------------------
def run_dmd(case, device=True, **kwargs):
    from sparsespatialsampling_amd.dmd import DMD
    built = case.build()
    data = built["data"]
    if device:
        data = device_matrix(data, case.layout) if data.dim() == 2 else data.cuda()
    area = None if built["area"] is None else pt.from_numpy(built["area"])
    kwargs.setdefault("rank", None if case.noise else case.r)
    return DMD(data, case.dt, optimal=case.optimal, cell_area=area, **kwargs)


def check_against_truth(case, built, got, report=print):
    """the comparisons of one noise-free case.  ``got``: eigvals, frequency, growth_rate, modes [rows, r], amplitude,
    reconstruction [rows, T] as numpy arrays.  The Gram route squares the condition number, so with e_ref the direct reference's own
    error against the planted truth and kappa = s_1 / s_r, the result has to be within max(16 e_ref, 64 eps kappa^2) of the truth,
    relative."""
    ref = built["ref"]
    floor = 64.0 * EPS * built["kappa"] ** 2
    o_ref, o_got = dc.by_angle(ref["eigvals"]), dc.by_angle(got["eigvals"])
    lam = built["lam"]
    rows = []
    for name, truth, r_val, g_val in (
            ("eigvals", lam, ref["eigvals"][o_ref], got["eigvals"][o_got]),
            ("frequency", np.log(lam).imag / (2 * np.pi * case.dt), ref["frequency"][o_ref], got["frequency"][o_got]),
            ("growth_rate", np.log(lam).real / case.dt, ref["growth_rate"][o_ref], got["growth_rate"][o_got]),
            ("products", built["products"], (ref["modes"] * ref["amplitude"])[:, o_ref], (got["modes"] * got["amplitude"])[:, o_got]),
            ("reconstruction", built["truth"], ref["reconstruction"], got["reconstruction"])):
        scale = np.abs(truth).max()
        e_ref, e_got = float(np.abs(r_val - truth).max() / scale), float(np.abs(g_val - truth).max() / scale)
        rows.append((name, e_ref, e_got, max(16 * e_ref, floor)))
    for name, e_ref, e_got, bound in rows:
        report(f"{case.name:36s} {name:15s} kappa {built['kappa']:6.2f}  e_ref {e_ref:.2e}  device {e_got:.2e}  bound {bound:.2e}")
    bad = [row for row in rows if not row[2] <= row[3]]
    assert not bad, bad


def as_numpy(model):
    r = model.svd.rank
    rec = model.reconstruction()
    return dict(eigvals=model.eigvals.cpu().numpy(), frequency=model.frequency.cpu().numpy(), growth_rate=model.growth_rate.cpu().numpy(),
                modes=model.modes.cpu().numpy().reshape(-1, r), amplitude=model.amplitude.cpu().numpy(),
                reconstruction=rec.cpu().numpy().reshape(-1, rec.shape[-1]))


@pytest.mark.parametrize("case", dc.NOISE_FREE, ids=repr)
def test_dmd_against_reference_and_truth(case, caplog):
    built = case.build()
    with caplog.at_level(logging.WARNING):
        model = run_dmd(case)
    assert not caplog.records, "the 1e-4 rank cap must not bind in these cases"
    assert model.svd.rank == case.r
    got = as_numpy(model)
    assert model.modes.shape == tuple(built["data"].shape[:-1]) + (case.r,) and model.modes.dtype == pt.complex128
    assert got["reconstruction"].dtype == np.float64 and model.dynamics.shape == (case.r, case.t)
    check_against_truth(case, built, got)
    # reconstruction_error (from G alone) against the materialised residual: squared norms within 64 T eps G_tt
    sw = built["ref"]["weight_sqrt"]
    dw = built["data"].numpy().astype(np.float64).reshape(-1, case.t) * sw[:, None]
    g_tt = (dw ** 2).sum(axis=0)
    sq_direct = ((dw - got["reconstruction"] * sw[:, None]) ** 2).sum(axis=0)
    err = model.reconstruction_error.cpu().numpy()
    assert err.shape == (case.t,)
    assert (np.abs(err ** 2 * g_tt - sq_direct) <= 64.0 * case.t * EPS * g_tt).all()
    # a window and a subset of the modes
    t0, t1 = 1, min(case.t, 3)
    assert np.array_equal(model.reconstruction(t0, t1).cpu().numpy().reshape(-1, t1 - t0), got["reconstruction"][:, t0:t1])
    every = model.partial_reconstruction(list(range(case.r)), t0, t1).cpu().numpy().reshape(-1, t1 - t0)
    assert np.array_equal(every, got["reconstruction"][:, t0:t1])
    pair = [int(i) for i in np.argsort(np.abs(got["frequency"]), kind="stable")[:2]]      # the slowest conjugate pair
    part = model.partial_reconstruction(pair, 0, case.t).cpu().numpy().reshape(-1, case.t)
    want = ((got["modes"][:, pair] * got["amplitude"][pair]) @ (got["eigvals"][pair][:, None] ** np.arange(case.t)[None, :])).real
    assert np.abs(part - want).max() <= 64 * EPS * case.r * np.abs(got["reconstruction"]).max()


def test_noisy_case_finds_the_reference_rank():
    built = dc.NOISY.build()
    model = run_dmd(dc.NOISY)
    assert model.svd.opt_rank == built["ref"]["opt_rank"] == model.svd.rank == dc.NOISY.r
    o_ref, o_got = dc.by_angle(built["ref"]["eigvals"]), dc.by_angle(model.eigvals.cpu().numpy())
    # (both routes see the same perturbed data and keep the same six directions: they differ by rounding only, the Gram route's floor)
    assert np.abs(model.eigvals.cpu().numpy()[o_got] - built["ref"]["eigvals"][o_ref]).max() <= 64 * EPS * built["kappa"] ** 2


TENSORS = ("eigvals", "eigvecs", "amplitude", "frequency", "growth_rate", "dynamics", "modes", "reconstruction_error", "integral_contribution")


def everything(model):
    out = {name: getattr(model, name) for name in TENSORS}
    out.update(s=model.svd.s, V=model.svd.V, reconstruction=model.reconstruction(), top=model.top_modes(integral=True),
               part=model.partial_reconstruction([0], 0, 2))
    return out


def complex_bits(a, b):
    a, b = a.cpu(), b.cpu()
    if a.is_complex():
        a, b = pt.view_as_real(a), pt.view_as_real(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(pt.equal(a, b)) and \
        (not a.is_floating_point() or same_bits(a.double(), b.double()))


@pytest.mark.parametrize("case", [dc.NOISE_FREE[9], dc.NOISE_FREE[10]], ids=repr)
def test_host_and_device_input_and_two_runs_agree_to_the_bit(case):
    """host in / host out == device in / device out; two runs give identical bits in every returned tensor; the input keeps its
    bits and dtype"""
    built = case.build()
    data_dev = device_matrix(built["data"], case.layout) if built["data"].dim() == 2 else built["data"].cuda()
    keep = data_dev.clone()
    area = pt.from_numpy(built["area"])
    from sparsespatialsampling_amd.dmd import DMD
    first = everything(DMD(data_dev, case.dt, rank=case.r, optimal=case.optimal, cell_area=area.cuda()))
    assert data_dev.dtype == case.dtype and same_bits(data_dev.double(), keep.double())
    second = everything(DMD(data_dev, case.dt, rank=case.r, optimal=case.optimal, cell_area=area.cuda()))
    host_in = built["data"].clone()
    host = everything(DMD(host_in, case.dt, rank=case.r, optimal=case.optimal, cell_area=area))
    assert pt.equal(host_in[..., :], built["data"]) and host_in.dtype == case.dtype
    for name in first:
        assert first[name].is_cuda and not host[name].is_cuda, name
        assert complex_bits(first[name], second[name]), name
        assert complex_bits(first[name], host[name]), name


def test_top_modes_order_matches_the_reference():
    case = dc.NOISE_FREE[6]                                                       # 20 conjugate pairs, areas, optimal amplitudes
    built = case.build()
    ref = built["ref"]
    model = run_dmd(case)
    freq = model.frequency.cpu().numpy()

    def ref_order(importance, f_min=-np.inf, f_max=np.inf):
        inside = np.nonzero((ref["frequency"] >= f_min) & (ref["frequency"] < f_max))[0]
        return inside[np.argsort(-importance[inside], kind="stable")]
    positive = np.sort(ref["frequency"][ref["frequency"] > 0])
    f_mid = float(0.5 * (positive[9] + positive[10]))                            # between two planted frequencies
    for integral, importance in ((False, np.abs(ref["amplitude"])), (True, ref["integral"])):
        # one member per pair (f >= 0): the order is decided by importances that differ between pairs
        got = model.top_modes(integral=integral, f_min=0).cpu().numpy()
        want = ref_order(importance, 0)
        assert np.allclose(freq[got], ref["frequency"][want], rtol=1e-9, atol=0), integral
        got = model.top_modes(n=5, integral=integral, f_min=0, f_max=f_mid).cpu().numpy()
        assert np.allclose(freq[got], ref["frequency"][ref_order(importance, 0, f_mid)[:5]], rtol=1e-9, atol=0) and len(got) == 5
        # all modes: the two members of a pair tie to rounding, so compare |frequency|
        got = model.top_modes(integral=integral).cpu().numpy()
        assert len(got) == case.r and np.allclose(np.abs(freq[got]), np.abs(ref["frequency"][ref_order(importance)]), rtol=1e-9, atol=0)
    assert np.allclose(model.integral_contribution.cpu().numpy()[dc.by_angle(model.eigvals.cpu().numpy())],
                       ref["integral"][dc.by_angle(ref["eigvals"])], rtol=1e-6)


def test_dmd_of_float32_needs_less_extra_memory_than_a_double_copy():
    """a condition, not a timing: the peak of extra device memory during ``DMD(float32 [3000, 130])`` -- every buffer dmd.py and
    hipops allocate comes from torch's allocator -- stays below one float64 copy of the input"""
    case = dc.NOISE_FREE[7]
    data = case.build()["data"].cuda()
    from sparsespatialsampling_amd.dmd import DMD
    DMD(data, case.dt, rank=case.r)                                               # (first call: library handles, staging buffers)
    pt.cuda.synchronize()
    pt.cuda.reset_peak_memory_stats()
    before = pt.cuda.memory_allocated()
    model = DMD(data, case.dt, rank=case.r)
    pt.cuda.synchronize()
    extra = pt.cuda.max_memory_allocated() - before
    print(f"extra peak {extra} bytes, a float64 copy {data.numel() * 8} bytes")
    assert model.svd.rank == case.r and extra < data.numel() * 8


# ---- centred and weighted Gram, centred and residual GEMM: per element against long double -----------------------------------------
WORST = {}


def note(family, r):
    WORST[family] = max(WORST.get(family, 0.0), r)
    return r


@pytest.mark.parametrize("t", SHAPES_T)
@pytest.mark.parametrize("n", SHAPES_N)
def test_centred_weighted_gram_per_element(ops, n, t):
    """rows of mean 1e5 and fluctuation 1e-2, weights from 1e-6 to 1e2, both dtypes, mean and weight / mean alone / weight alone: every
    element within (N + 8) u sum_n a_n |d_ni| |d_nj| of the long-double sum over d = x - mean with the doubles the kernel is given; every
    layout and offset gives the same bits; float64 input through s3_weighted_gram gives them too"""
    from sparsespatialsampling_amd import svd
    for dtype in (np.float32, np.float64):
        x = cc.rows(n, t, dtype, 7 * n + t)
        mean, weight = cc.row_means(x), cc.weights(n, n + t)
        xt, md, wd = pt.from_numpy(x), pt.from_numpy(mean).cuda(), pt.from_numpy(weight).cuda()
        forms = [(mean, weight), (mean, None) if dtype == np.float32 else (None, weight)]
        for m_host, w_host in forms:
            m_dev, w_dev = (md if m_host is not None else None), (wd if w_host is not None else None)
            ref, mag = cc.gram_reference(x, m_host, w_host)
            want = ops.gram(device_matrix(xt, "contiguous"), m_dev, w_dev)
            r = note("gram", cc.ratio(want.cpu().numpy(), ref, cc.gram_bound(n, mag)))
            assert r <= 1.0, (np.dtype(dtype).name, m_host is None, w_host is None, r)
            assert same_bits(want, want.T.contiguous())
            for layout in LAYOUTS:
                for offset in (0, 1):
                    assert same_bits(ops.gram(device_matrix(xt, layout, offset), m_dev, w_dev), want), (layout, offset)
            if dtype == np.float64 and m_host is not None and w_host is not None:
                for layout in LAYOUTS:
                    assert same_bits(svd.weighted_gram(device_matrix(xt, layout, 1), md, wd), want), layout
    print(f"worst |error| / bound so far: {WORST}")


@pytest.mark.parametrize("n", [1, 4, 64, 65, 80])
@pytest.mark.parametrize("m", [1, 15, 17, 257])
def test_centred_and_residual_gemm_per_element(ops, m, n):
    """(L - lmean) B within (k + 4) u sum |l - lmean| |b| per element; (E - emean) - (L - lmean) B within that plus
    2 u |e - emean| + u |c_ref|; with and without each mean; L and E in every layout and offset (same bits)"""
    from sparsespatialsampling_amd import svd
    for k in (3, 17, 130):
        rng = np.random.default_rng(m + 31 * n + k)
        left, e = cc.rows(m, k, np.float64, m + 31 * n + k), cc.rows(m, n, np.float64, 5 + m + n)
        lmean, emean = cc.row_means(left), cc.row_means(e) + 1e-3 * rng.standard_normal(m)
        b = rng.standard_normal((k, n))
        lt, et, bd = pt.from_numpy(left), pt.from_numpy(e), pt.from_numpy(b).cuda()
        lmd, emd = pt.from_numpy(lmean).cuda(), pt.from_numpy(emean).cuda()
        for lm_host, lm_dev in ((lmean, lmd), (None, None)):
            ref, bound = cc.gemm_reference(left, lm_host, b)
            want = svd.centered_gemm(device_matrix(lt, "contiguous"), lm_dev, bd)
            r = note("gemm", cc.ratio(want.cpu().numpy(), ref, bound))
            assert want.shape == (m, n) and r <= 1.0, (k, lm_host is None, r)
            for em_host, em_dev in ((emean, emd), (None, None)):
                ref_r, bound_r = cc.gemm_reference(left, lm_host, b, e, em_host)
                want_r = svd.centered_gemm(device_matrix(lt, "contiguous"), lm_dev, bd, minus_from=device_matrix(et, "contiguous"),
                                           minus_from_mean=em_dev)
                r = note("residual gemm", cc.ratio(want_r.cpu().numpy(), ref_r, bound_r))
                assert r <= 1.0, (k, lm_host is None, em_host is None, r)
                if lm_host is None or em_host is None:
                    continue
                for layout in LAYOUTS:
                    for offset in (0, 1):
                        ld, ed = device_matrix(lt, layout, offset), device_matrix(et, layout, 1 - offset)
                        assert same_bits(svd.centered_gemm(ld, lm_dev, bd), want), (k, layout, offset)
                        assert same_bits(svd.centered_gemm(ld, lm_dev, bd, minus_from=ed, minus_from_mean=em_dev), want_r), (k, layout, offset)
    print(f"worst |error| / bound so far: {WORST}")
