"""
Single-precision S^3 files on the GPU: the rounding transposes (``s3_snapshot_major_as`` / ``_rows_as``), the loader's inverse
(``s3_cell_major``), ``ExportData(file_dtype=float32)`` end to end and ``Dataloader.load_snapshot(device=True)``.

Every expectation is a numpy cast of this build's own float64 result, compared as bit patterns: the float32 file holds
``astype(float32)`` of what the float64 file holds, nothing else differs.
"""
import os
import types

import numpy as np
import pytest
import torch as pt

from sparsespatialsampling_amd import h5io

pytestmark = pytest.mark.gpu

NC = (1, 63, 64, 65, 257)
N_SNAP = (1, 2, 31, 32, 33, 100)
CANARY = -559038737                      # 0xDEADBEEF as int32
FLT_MAX = float(np.finfo(np.float32).max)


def planted():
    """the float64 values at which a float32 rounding can go wrong, and their negatives"""
    edge = FLT_MAX + 2.0 ** 103                                        # the overflow boundary: a tie between FLT_MAX and 2^128
    tie_zero = 2.0 ** -150                                             # a tie between 0 and the smallest subnormal
    v = []
    for tie in (1.0 + 2.0 ** -24, 1.0 + 3.0 * 2.0 ** -24):             # ties to even, downwards and upwards
        v += [tie, tie + 2.0 ** -52, tie - 2.0 ** -52]
    v += [FLT_MAX, edge, np.nextafter(edge, 0.0), np.nextafter(edge, np.inf), 1e-40, 2.0 ** -149, tie_zero,
          np.nextafter(tie_zero, 0.0), np.nextafter(tie_zero, 1.0), 0.0, np.inf, 2.0 ** -126, np.nextafter(2.0 ** -126, 0.0), 5e-324, 1e300]
    v = np.array(v, dtype=np.float64)
    return np.concatenate([v, -v])


def batch(nc, n_comp, n_snap, seed):
    """[nc, n_comp, T] float64: random values over the whole float32 range and beyond, with the planted set at random places"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nc, n_comp, n_snap)) * 10.0 ** rng.uniform(-47, 40, (nc, n_comp, n_snap))
    flat, p = x.reshape(-1), planted()
    where = rng.permutation(flat.size)[:len(p)]
    flat[where] = np.roll(p, seed)[:len(where)]
    return x


def as_f32(a):
    with np.errstate(over="ignore"):
        return a.astype(np.float32)


def bits(a):
    a = a.cpu().numpy() if isinstance(a, pt.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def ops():
    from sparsespatialsampling_amd import hipops
    hipops.device()
    return hipops


def test_planted_values_are_what_they_claim():
    """(host) the planted set does contain ties, subnormal results, signed zeros and both sides of the overflow boundary"""
    p = planted()
    f = as_f32(p)
    assert np.isinf(f[np.isfinite(p)]).any() and (f[np.isfinite(p)] == np.float32(FLT_MAX)).any()
    assert ((f != 0) & (np.abs(f) < np.finfo(np.float32).tiny)).any() and ((f == 0) & (p != 0)).any() and np.signbit(f[(f == 0)]).any()


@pytest.mark.parametrize("n_comp", [1, 2, 3, 5])
def test_snapshot_major_float32_equals_the_numpy_cast(ops, n_comp):
    for nc in NC:
        for n_snap in N_SNAP if n_comp <= 3 else (1, 33):
            x = batch(nc, n_comp, n_snap, seed=nc + n_snap)
            want = bits(as_f32(np.transpose(x, (2, 0, 1))))
            dev = pt.from_numpy(x).cuda()
            n = x.size
            for offset in (0, 1):                                      # 1: rows on 4-byte boundaries only -> the narrow stores
                buf = pt.full((n + offset + 16,), CANARY, dtype=pt.int32, device="cuda").view(pt.float32)
                out = ops.snapshot_major(dev, n_comp, n_snap, out=buf[offset:offset + n].view(n_snap, nc, n_comp), dtype=pt.float32)
                assert out.dtype == pt.float32 and out.data_ptr() == buf.data_ptr() + 4 * offset
                got = buf.cpu().numpy().view(np.uint32)
                assert np.array_equal(got[offset:offset + n].reshape(want.shape), want), (nc, n_comp, n_snap, offset)
                assert (got[:offset].view(np.int32) == CANARY).all() and (got[offset + n:].view(np.int32) == CANARY).all(), \
                    f"bytes around the float32 result were written ({nc}, {n_comp}, {n_snap}, offset {offset})"
            fresh = ops.snapshot_major(dev, n_comp, n_snap, dtype=pt.float32)
            assert tuple(fresh.shape) == (n_snap, nc, n_comp) and np.array_equal(bits(fresh), want)


@pytest.mark.parametrize("n_comp", [1, 2, 3])
def test_snapshot_major_float64_is_the_existing_one(ops, n_comp):
    from sparsespatialsampling_amd import _lib
    for nc in NC:
        for n_snap in N_SNAP:
            x = batch(nc, n_comp, n_snap, seed=7 * nc + n_snap)
            dev = pt.from_numpy(x).cuda()
            old = ops.snapshot_major(dev, n_comp, n_snap)
            new = ops.snapshot_major(dev, n_comp, n_snap, dtype=pt.float64)
            direct = pt.full_like(old, -1.0)
            ops.check(_lib.hip_lib().s3_snapshot_major_as(ops._ptr(dev), nc, n_comp, n_snap, 1, ops._ptr(direct), ops._stream()), "as")
            want = bits(np.transpose(x, (2, 0, 1)))
            assert old.dtype == new.dtype == pt.float64
            assert np.array_equal(bits(old), want) and np.array_equal(bits(new), want) and np.array_equal(bits(direct), want)


@pytest.mark.parametrize("dtype", [pt.float32, pt.float64])
@pytest.mark.parametrize("n_comp", [1, 2, 3])
def test_snapshot_major_rows_scatters_a_shard(ops, n_comp, dtype):
    np_bits = np.uint32 if dtype == pt.float32 else np.uint64
    for nc in NC:
        for n_snap in (1, 2, 33, 100):
            rng = np.random.default_rng(nc * n_snap)
            n_out = nc + 1 + nc // 3                                    # the shard holds fewer rows than the file
            rows = rng.permutation(n_out)[:nc].astype(np.int32)
            x = batch(nc, n_comp, n_snap, seed=3 * nc + n_snap)
            moved = np.transpose(x, (2, 0, 1))
            moved = as_f32(moved) if dtype == pt.float32 else moved
            words = 1 if dtype == pt.float32 else 2
            buf = pt.full(((n_snap * n_out * n_comp + 16) * words,), CANARY, dtype=pt.int32, device="cuda")
            ops.snapshot_major_rows(pt.from_numpy(x).cuda(), n_comp, n_snap, pt.from_numpy(rows).cuda(), n_out, buf.data_ptr(), dtype=dtype)
            got = buf.cpu().numpy()
            want = np.full(got.shape, CANARY, dtype=np.int32).view(np_bits)
            body = want[:n_snap * n_out * n_comp].reshape(n_snap, n_out, n_comp)
            body[:, rows, :] = bits(moved)
            assert np.array_equal(got.view(np_bits), want), (nc, n_comp, n_snap)


F32_PATTERNS = np.array([0x00000001, 0x007fffff, 0x00800000, 0x00400000, 0x7f7fffff, 0x7f800000, 0x00000000, 0x3f800001, 0x00012345],
                        dtype=np.uint32)


def snapshots(t_b, nc, n_comp, np_type, seed):
    """[T_b, nc, n_comp] as the file holds them; float32: random bit patterns (no NaN) with subnormals, extremes and signed zeros"""
    if np_type == np.float64:
        return np.ascontiguousarray(np.transpose(batch(nc, n_comp, t_b, seed), (2, 0, 1)))
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 2 ** 32, (t_b, nc, n_comp), dtype=np.uint64).astype(np.uint32)
    u[(u & 0x7f800000) == 0x7f800000] &= 0xbfffffff                     # exponent 255 (inf / NaN) -> an ordinary number
    flat = u.reshape(-1)
    p = np.concatenate([F32_PATTERNS, F32_PATTERNS | 0x80000000])
    where = rng.permutation(flat.size)[:len(p)]
    flat[where] = np.roll(p, seed)[:len(where)]
    return u.view(np.float32)


@pytest.mark.parametrize("out_type", [np.float32, np.float64])
@pytest.mark.parametrize("in_type", [np.float32, np.float64])
@pytest.mark.parametrize("n_comp", [1, 2, 3])
def test_cell_major_writes_its_columns_and_nothing_else(ops, n_comp, in_type, out_type):
    w_out = np.uint32 if out_type == np.float32 else np.uint64
    words = 1 if out_type == np.float32 else 2
    for nc in NC:
        for t_b in N_SNAP:
            s = snapshots(t_b, nc, n_comp, in_type, seed=nc + 5 * t_b)
            t0, n_cols = 3, t_b + 5
            pitch = n_cols + 3                                          # rows longer than the matrix: padding the kernel must skip
            base = pt.full((nc * n_comp, pitch * words), CANARY, dtype=pt.int32, device="cuda").view(pt.float32 if words == 1 else pt.float64)
            out = base[:, :n_cols].unflatten(0, (nc, n_comp))
            src = pt.from_numpy(s).cuda()
            back = ops.cell_major(src if n_comp > 1 else src[:, :, 0].contiguous(), out if n_comp > 1 else out[:, 0, :], t0)
            assert back.data_ptr() == base.data_ptr()
            want = np.full((nc * n_comp, pitch * words), CANARY, dtype=np.int32).view(w_out)
            moved = np.transpose(s, (1, 2, 0)).reshape(nc * n_comp, t_b)
            want[:, t0:t0 + t_b] = bits(as_f32(moved) if out_type == np.float32 else moved.astype(np.float64))
            assert np.array_equal(bits(base), want), (nc, n_comp, t_b, in_type, out_type)


@pytest.mark.parametrize("dtype", [pt.float32, pt.float64])
def test_round_trip_gives_the_batch_back(ops, dtype):
    for nc, n_comp, n_snap in ((257, 3, 33), (65, 1, 100), (63, 2, 2), (1, 1, 1)):
        x = batch(nc, n_comp, n_snap, seed=11)
        dev = pt.from_numpy(x).cuda()
        again = ops.cell_major(ops.snapshot_major(dev, n_comp, n_snap, dtype=dtype), pt.empty((nc, n_comp, n_snap), dtype=dtype, device="cuda"))
        assert np.array_equal(bits(again), bits(as_f32(x) if dtype == pt.float32 else x))


def test_bad_arguments_raise_before_any_launch(ops):
    x = pt.from_numpy(batch(65, 2, 4, seed=1)).cuda()
    out = pt.full((4, 65, 2), 7.0, dtype=pt.float32, device="cuda")
    with pytest.raises(TypeError):
        ops.snapshot_major(x.cpu(), 2, 4, dtype=pt.float32)
    with pytest.raises(TypeError):
        ops.snapshot_major(x.float(), 2, 4, out=out, dtype=pt.float32)
    with pytest.raises(TypeError):
        ops.snapshot_major(x, 2, 4, out=out.double(), dtype=pt.float32)            # out of the other type
    with pytest.raises(TypeError):
        ops.snapshot_major(x, 2, 4, out=out.cpu(), dtype=pt.float32)
    with pytest.raises(ValueError):
        ops.snapshot_major(x, 3, 4, out=out, dtype=pt.float32)                     # 65 x 8 values are not 3 components x 4
    with pytest.raises(ValueError):
        ops.snapshot_major(x, 2, 4, out=out, dtype=pt.float16)
    rows = pt.arange(65, dtype=pt.int32, device="cuda")
    with pytest.raises(TypeError):
        ops.snapshot_major_rows(x, 2, 4, rows.long(), 65, out.data_ptr(), dtype=pt.float32)
    with pytest.raises(TypeError):
        ops.snapshot_major_rows(x, 2, 4, rows[:64], 65, out.data_ptr(), dtype=pt.float32)
    with pytest.raises(ValueError):
        ops.snapshot_major_rows(x, 2, 4, rows, 64, out.data_ptr(), dtype=pt.float32)    # fewer output rows than input rows
    with pytest.raises(ValueError):
        ops.snapshot_major_rows(x, 2, 4, rows, 65, out.data_ptr() + 2, dtype=pt.float32)
    s = pt.zeros((4, 65, 2), dtype=pt.float64, device="cuda")
    m = pt.full((65, 2, 9), 7.0, dtype=pt.float32, device="cuda")
    with pytest.raises(TypeError):
        ops.cell_major(s.cpu(), m)
    with pytest.raises(TypeError):
        ops.cell_major(s, m.cpu())
    with pytest.raises(TypeError):
        ops.cell_major(s.long(), m)
    with pytest.raises(TypeError):
        ops.cell_major(s.permute(0, 2, 1), m.permute(1, 0, 2))                     # snapshots not contiguous
    with pytest.raises(ValueError):
        ops.cell_major(s, m[:64])
    with pytest.raises(ValueError):
        ops.cell_major(s, m, 6)                                                    # columns [6, 10) of 9
    with pytest.raises(ValueError):
        ops.cell_major(s, m, -1)
    with pytest.raises(ValueError):
        ops.cell_major(s, m[:, :, ::2][:, :, :4])                                  # no unit stride along T
    with pytest.raises(ValueError):
        ops.cell_major(s[:, :, 0].contiguous(), m)
    pt.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((m == 7.0).all())


# ----------------------------------------------------------------------------------------------------------------------
# end to end: the same export once per storage type
# ----------------------------------------------------------------------------------------------------------------------
N_CELLS, N_SRC, T = 300, 2500, 5
TIMES = [f"{0.1 * i:.1f}" for i in range(T)]


def scube(directory, d):
    rng = np.random.default_rng(d)
    return types.SimpleNamespace(n_dimensions=d, faces=pt.arange(N_CELLS * 2 ** d, dtype=pt.int32).reshape(N_CELLS, 2 ** d),
                                 centers=pt.from_numpy(rng.random((N_CELLS, d))), vertices=pt.from_numpy(rng.random((N_CELLS * 2 ** d, d))),
                                 levels=pt.ones((N_CELLS, 1), dtype=pt.int64), metric=pt.from_numpy(rng.random(N_SRC)), size_initial_cell=2.5,
                                 save_path=str(directory), save_name="case", grid_name="grid_s_cube")


def source(d):
    rng = np.random.default_rng(10 + d)
    x = rng.random((N_SRC, d))
    p = (np.sin(7 * x[:, :1] + np.arange(T)) * 10.0 ** rng.uniform(-3, 3, (N_SRC, 1))).astype(np.float32)[:, None, :]
    u = rng.standard_normal((N_SRC, d, T)).astype(np.float32)
    return x, p, u


def run_export(directory, d, file_dtype, on_device=False, vertices=False, new_file=False, append=False):
    """p in batches of 2, 2 and 1 snapshots, then U at once.  ``append``: p by a float64 object, U appended by one of ``file_dtype``"""
    from sparsespatialsampling_amd.export import ExportData
    os.makedirs(directory, exist_ok=True)
    x, p, u = source(d)
    put = (lambda a: pt.from_numpy(np.ascontiguousarray(a)).cuda()) if on_device else (lambda a: pt.from_numpy(np.ascontiguousarray(a)))
    xt = pt.from_numpy(x)
    kw = dict(write_times=TIMES, interpolate_at_vertices=vertices, write_new_file_for_each_field=new_file)
    first = ExportData(scube(directory, d), file_dtype=pt.float64 if append else file_dtype, **kw)
    for a, b in ((0, 2), (2, 4), (4, 5)):
        first.export(xt, put(p[:, :, a:b]), "p", n_snapshots_total=T)
    second = ExportData(scube(directory, d), append_existing=True, file_dtype=file_dtype, **kw) if append else first
    second.export(xt, put(u), "U")
    return directory


def datasets(path):
    """[(dataset path, array)] of a file in the file's own order"""
    out = []
    with h5io.open_h5(path, "r") as f:
        def walk(group):
            for k in f.keys(group):
                p = k if group == "/" else f"{group}/{k}"
                try:
                    out.append((p, f.read(p)))
                except (FileNotFoundError, h5io.H5Error):
                    walk(p)
        walk("/")
    return out


def compare_pair(dir64, dir32, single_fields=("p", "U")):
    files = sorted(f for f in os.listdir(dir64) if f.endswith(".h5"))
    assert files and files == sorted(f for f in os.listdir(dir32) if f.endswith(".h5"))
    for name in files:
        a, b = datasets(os.path.join(dir64, name)), datasets(os.path.join(dir32, name))
        assert [k for k, _ in a] == [k for k, _ in b] and [v.shape for _, v in a] == [v.shape for _, v in b]
        n_single = 0
        for (key, v64), (_, v32) in zip(a, b):
            single = key.startswith("data/") and key.rsplit("/", 1)[1].split("_")[0] in single_fields
            if single:
                n_single += 1
                assert v64.dtype == np.float64 and v32.dtype == np.float32, key
                assert np.array_equal(bits(v32), bits(as_f32(v64))), key
            else:
                assert v32.dtype == v64.dtype and v32.tobytes() == v64.tobytes(), key
        assert n_single
        x64, x32 = (open(os.path.join(d, name.replace(".h5", ".xdmf"))).read() for d in (dir64, dir32))
        assert 'Precision="4"' not in x64 and x32.count('Precision="4"') == n_single
        l64, l32 = x64.split("\n"), x32.split("\n")
        assert len(l64) == len(l32)
        for i, (u, v) in enumerate(zip(l64, l32)):
            if u != v:
                assert v == u.replace('Precision="8"', 'Precision="4"') and "/data/" in l32[i + 1] and l32[i - 1].startswith("<Attribute"), v


CONFIGS = {"host": {}, "device": dict(on_device=True), "vertices": dict(vertices=True), "vertices_device": dict(vertices=True, on_device=True),
           "new_file": dict(new_file=True), "append": dict(append=True)}


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("d", [2, 3])
def test_float32_file_is_the_cast_of_the_float64_file(tmp_path, d, config):
    kw = CONFIGS[config]
    dir64 = run_export(str(tmp_path / "f64"), d, pt.float64, **kw)
    dir32 = run_export(str(tmp_path / "f32"), d, pt.float32, **kw)
    compare_pair(dir64, dir32, single_fields=("U",) if config == "append" else ("p", "U"))


def test_float64_field_appended_to_a_float32_file(tmp_path):
    """the reverse of the append case: datasets carry their own type"""
    from sparsespatialsampling_amd.export import ExportData
    x, p, u = source(2)
    ex = ExportData(scube(tmp_path, 2), write_times=TIMES, file_dtype=pt.float32)
    ex.export(pt.from_numpy(x), pt.from_numpy(p), "p")
    ExportData(scube(tmp_path, 2), write_times=TIMES, append_existing=True).export(pt.from_numpy(x), pt.from_numpy(u), "U")
    found = dict(datasets(str(tmp_path / "case.h5")))
    assert found["data/0.3/p_center"].dtype == np.float32 and found["data/0.3/U_center"].dtype == np.float64
    text = open(tmp_path / "case.xdmf").read()
    assert text.count('Precision="4"') == T
    assert ex._interpolated_fields.centers is None or ex._interpolated_fields.centers.dtype == pt.float64


def test_pipelined_pieces_store_float32(tmp_path):
    """a device-resident scalar batch long enough to be cut into snapshot pieces (``_fit_pieces``: piece buffers, stage and copies
    in the storage type)"""
    from sparsespatialsampling_amd.export import ExportData
    rng = np.random.default_rng(5)
    n_t = 72
    x = rng.random((N_SRC, 2))
    p = pt.from_numpy(rng.standard_normal((N_SRC, 1, n_t)).astype(np.float32)).cuda()
    times = [str(i) for i in range(n_t)]
    found = {}
    for name, file_dtype in (("f64", pt.float64), ("f32", pt.float32)):
        os.makedirs(tmp_path / name)
        ex = ExportData(scube(tmp_path / name, 2), write_times=times, file_dtype=file_dtype)
        ex._chunk_size = 1
        assert len(ex._snapshot_pieces(p, 1, n_t)) > 1
        ex.export(pt.from_numpy(x), p, "p", chunk_size=1)
        found[name] = dict(datasets(str(tmp_path / name / "case.h5")))
    for t in times:
        a, b = found["f64"][f"data/{t}/p_center"], found["f32"][f"data/{t}/p_center"]
        assert b.dtype == np.float32 and np.array_equal(bits(b), bits(as_f32(a))), t


# ----------------------------------------------------------------------------------------------------------------------
# loader
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def written(tmp_path_factory):
    root = tmp_path_factory.mktemp("loader")
    return {pt.float64: run_export(str(root / "f64"), 3, pt.float64), pt.float32: run_export(str(root / "f32"), 3, pt.float32)}


@pytest.mark.parametrize("group", [2, 16])
@pytest.mark.parametrize("want", [pt.float32, pt.float64])
@pytest.mark.parametrize("stored", [pt.float32, pt.float64])
def test_device_loader_equals_the_host_loader(written, stored, want, group, monkeypatch):
    from sparsespatialsampling_amd.data import Dataloader
    monkeypatch.setattr(Dataloader, "DEVICE_GROUP_TIMES", group)        # 2: five write times in groups of 2, 2 and 1
    loader = Dataloader(written[stored], "case.h5", dtype=want)
    for fields, times in (("p", None), ("U", None), ("U", ["0.3", "0.0", "0.2"]), ("p", "0.4"), (["p", "U"], ["0.4", "0.1", "0.2"])):
        host = loader.load_snapshot(fields, times)
        dev = loader.load_snapshot(fields, times, device=True)
        for h, g in zip([host] if isinstance(fields, str) else host, [dev] if isinstance(fields, str) else dev):
            assert g.is_cuda and not h.is_cuda and g.dtype == h.dtype == want and g.shape == h.shape and g.is_contiguous()
            assert np.array_equal(bits(g), bits(h)), (fields, times)


def test_device_loader_feeds_the_svd(written):
    from sparsespatialsampling_amd.data import Dataloader
    from sparsespatialsampling_amd.svd import compute_svd
    loader = Dataloader(written[pt.float32], "case.h5")
    s_dev = compute_svd(loader.load_snapshot("p", device=True), loader.weights, rank=3)[0]
    s_host = compute_svd(loader.load_snapshot("p"), loader.weights, rank=3)[0]
    assert s_dev.is_cuda and np.allclose(s_dev.cpu().numpy(), s_host.numpy(), rtol=1e-10, atol=0)
