"""``s3_mask_mesh`` on the MI355X: the device predicate of GeometrySTL3D against the host predicate, byte for byte; the column
bins against the brute-force table; against the analytic bodies' kernels; a full refine; the example.  GPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as pt

pytestmark = pytest.mark.gpu

from inputs import sha                                                                     # noqa: E402
from sparsespatialsampling_amd.geometry import GeometrySTL3D                               # noqa: E402
from sparsespatialsampling_amd.geometry.geometry_STL_3d import build_column_bins          # noqa: E402
from tests import stl_meshes as M                                                          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(rm, ki) for rm in (0, 1) for ki in (0, 1)]


@pytest.fixture(scope="module")
def ops():
    from sparsespatialsampling_amd import hipops
    hipops.device()
    return hipops


def table(ops, body, brute_force=False):
    _, tri, lo, hi, ny, nz, bin_start, bin_facet = body.kernel_spec()
    if brute_force:
        ny, nz, bin_start, bin_facet = build_column_bins(tri, lo, hi, 1, 1)
        assert np.array_equal(bin_facet, np.arange(len(tri)))
    return ops.MeshTable(tri, lo, hi, ny, nz, bin_start, bin_facet)


def device_verdicts(ops, mesh, center, level, width, rm, ki, cells=None, first=0, n=None, preset=None):
    d_center, d_level = ops.to_device(center), ops.to_device(level)
    d_cells = None
    if cells is not None:
        n, d_cells = len(cells), ops.to_device(np.ascontiguousarray(cells, dtype=np.int32))
    n = len(center) - first if n is None else n
    invalid = pt.zeros(n, dtype=pt.uint8, device="cuda") if preset is None else ops.to_device(preset.copy())
    ops.mask_mesh(ops.MaskCells(d_center, d_level, width, invalid, d_cells, first, n), mesh, rm, ki)
    return invalid.cpu().numpy()


def host_nodes_inside(body, center, level, width):
    """the host predicate at the 8 nodes of every cell -> bool [n, 8] (it does not depend on the mode)"""
    return body.inside(M.cell_nodes(center, level, width).reshape(-1, 3)).reshape(-1, 8)


def host_bytes(per_node, rm, ki):
    """the truth table of ``_apply_mask`` on the per-node verdicts"""
    return M.apply_mask(per_node, bool(ki), bool(rm)).astype(np.uint8)


def check_against_host(ops, make_body, center, level, width, n_direct=100):
    """all four modes: whole range, an id list, a first/n range, OR into pre-set flags -- identical bytes; and the public
    ``check_cell`` itself on ``n_direct`` seeded cells"""
    rng = np.random.default_rng(17)
    ids = rng.permutation(len(center))[:max(len(center) // 3, 1)].astype(np.int32)
    first, n = len(center) // 7, len(center) - len(center) // 7 - len(center) // 11
    preset = (rng.random(len(center)) < 0.3).astype(np.uint8)
    direct = rng.choice(len(center), min(n_direct, len(center)), replace=False)
    per_node = host_nodes_inside(make_body(False), center, level, width)
    for rm, ki in MODES:
        body = make_body(bool(ki))
        mesh = table(ops, body)
        want = host_bytes(per_node, rm, ki)
        assert 0 < want.sum() < len(want)
        assert np.array_equal(M.host_verdicts(body, center[direct], level[direct], width, rm).astype(np.uint8), want[direct])
        got = device_verdicts(ops, mesh, center, level, width, rm, ki)
        assert np.array_equal(got, want), f"mode {(rm, ki)}: {np.count_nonzero(got != want)} of {len(want)} cells differ"
        assert np.array_equal(device_verdicts(ops, mesh, center, level, width, rm, ki, cells=ids), want[ids])
        assert np.array_equal(device_verdicts(ops, mesh, center, level, width, rm, ki, first=first, n=n), want[first:first + n])
        assert np.array_equal(device_verdicts(ops, mesh, center, level, width, rm, ki, preset=preset), want | preset)
        brute = table(ops, body, brute_force=True)
        assert np.array_equal(device_verdicts(ops, brute, center, level, width, rm, ki), want)


def stacked(cells):
    return np.concatenate([c for c, _ in cells]), np.concatenate([lv for _, lv in cells])


# -- 10 / 11: host predicate and brute-force table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["cube", "L"])
def test_exact_bodies_lattices_with_nodes_on_the_surface(ops, tmp_path, shape):
    """levels 3 and 4 of [-0.5, 1.5]^3: nodes on faces, edges and corners, rays in face planes and through edges"""
    path = M.CUBE_STL if shape == "cube" else M.write_binary_stl(tmp_path / "l.stl", M.l_shape_facets())
    center, level = stacked([M.lattice_cells(-0.5, 2.0, 3), M.lattice_cells(-0.5, 2.0, 4)])
    check_against_host(ops, lambda ki: GeometrySTL3D(shape, ki, path), center, level, 2.0)


@pytest.mark.parametrize("kind", ["tet", "prism", "pyramid", "box"])
def test_flat_bodies_lattices_and_the_analytic_kernels(ops, tmp_path, kind):
    """levels 4 and 5 of the unit domain: s3_mask_mesh = host predicate = s3_mask_tetrahedra / s3_mask_prism / s3_mask_box"""
    center, level = stacked([M.lattice_cells(0.0, 1.0, 4), M.lattice_cells(0.0, 1.0, 5)])
    check_against_host(ops, lambda ki: M.flat_body(kind, ki, tmp_path)[1], center, level, 1.0)
    d_center, d_level = ops.to_device(center), ops.to_device(level)
    for rm, ki in MODES:
        analytic, body = M.flat_body(kind, bool(ki), tmp_path)
        spec = analytic.kernel_spec()
        fn = {"tetrahedra": ops.mask_tetrahedra, "prism": ops.mask_prism, "box": ops.mask_box}[spec[0]]
        want = pt.zeros(len(center), dtype=pt.uint8, device="cuda")
        fn(ops.MaskCells(d_center, d_level, 1.0, want), *spec[1:], rm, ki)
        got = device_verdicts(ops, table(ops, body), center, level, 1.0, rm, ki)
        assert 0 < got.sum() < len(got) and np.array_equal(got, want.cpu().numpy())


def random_cells(rng, n, mid, side):
    """random centres in a cube 1.3 times the body's bounding cube, random levels 2-8 of a root cell twice its size"""
    center = mid + (rng.random((n, 3)) - 0.5) * 1.3 * side
    return np.ascontiguousarray(center), rng.integers(2, 9, n).astype(np.int32), 2.0 * side


def test_icosphere_random_cells(ops, tmp_path):
    path = M.write_binary_stl(tmp_path / "ball.stl", M.icosphere_facets(3, center=(0.31, -0.17, 0.43), radius=0.77))
    probe = GeometrySTL3D("ball", False, path)
    assert probe.kernel_spec()[1].shape == (1280, 3, 3) and probe.kernel_spec()[4] * probe.kernel_spec()[5] > 100
    center, level, width = random_cells(np.random.default_rng(23), 50000, probe.center.double().numpy(), probe.main_width)
    check_against_host(ops, lambda ki: GeometrySTL3D("ball", ki, path), center, level, width)


def test_icosphere_20480_facets_bins_against_brute_force(ops, tmp_path):
    """the table the constructor chooses for a large surface gives the bytes of the 1 x 1 table; the host predicate on a
    sample of the cells"""
    path = M.write_binary_stl(tmp_path / "ball.stl", M.icosphere_facets(5, center=(0.31, -0.17, 0.43), radius=0.77))
    center, level, width = random_cells(np.random.default_rng(29), 50000, np.array([0.31, -0.17, 0.43]), 1.54)
    per_node = host_nodes_inside(GeometrySTL3D("ball", False, path), center[:2000], level[:2000], width)
    for rm, ki in MODES:
        body = GeometrySTL3D("ball", bool(ki), path)
        assert body.kernel_spec()[1].shape == (20480, 3, 3)
        binned = device_verdicts(ops, table(ops, body), center, level, width, rm, ki)
        assert np.array_equal(binned, device_verdicts(ops, table(ops, body, brute_force=True), center, level, width, rm, ki))
        assert np.array_equal(binned[:2000], host_bytes(per_node, rm, ki))
        assert 0 < binned.sum() < len(binned)


def test_bad_arguments_are_refused(ops, tmp_path):
    body = GeometrySTL3D("cube", False, M.CUBE_STL)
    _, tri, lo, hi, ny, nz, bin_start, bin_facet = body.kernel_spec()
    with pytest.raises(ValueError):
        ops.MeshTable(tri, lo, hi, ny, nz, bin_start, bin_facet + 1)             # a facet id out of range
    with pytest.raises(ValueError):
        ops.MeshTable(tri, lo, hi, ny, nz, bin_start[:-1], bin_facet)
    flat = pt.zeros((4, 2), dtype=pt.float64, device="cuda")
    with pytest.raises(ValueError):
        ops.mask_mesh(ops.MaskCells(flat, pt.zeros(4, dtype=pt.int32, device="cuda"), 1.0, pt.zeros(4, dtype=pt.uint8, device="cuda")),
                      table(ops, body), 0, 0)


# -- 13: full refine ---------------------------------------------------------------------------------------------------------------------
def test_refine_with_tessellated_polytopes_gpu(monkeypatch, tmp_path):
    """case refine_3d_polytopes with its bodies as GeometrySTL3D: device predicate, host predicate behind the proxy, and the CPU
    run (oracle backend) give one grid -- the golden grid of the reference"""
    import sparsespatialsampling_amd.s_cube as s_cube
    from tests.oracle_backend import OracleTreeBackend
    from tests.test_tree_host_logic import check_outputs_against_golden, check_tree_against_golden, load

    def run(host_only):
        x, y, geos, kw = M.polytopes_case(tmp_path, mesh=True, host_only=host_only)
        tree = s_cube.SamplingTree(pt.from_numpy(x), pt.from_numpy(y), geometry_obj=geos, **kw)
        tree.refine()
        return tree

    device, host = run(False), run(True)
    assert device._backend.name == "hip" and host._backend.name == "hip"
    assert len(device._backend._poly_cache) == 3 and not host._backend._poly_cache
    monkeypatch.setattr(s_cube, "_make_backend", lambda v, t, k: OracleTreeBackend(v, t, k))
    cpu = run(True)
    assert cpu._backend.name != "hip"
    for a, b, c in zip(M.grid_of(device), M.grid_of(host), M.grid_of(cpu)):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert sha(*M.grid_of(device)) == sha(*M.grid_of(host)) == sha(*M.grid_of(cpu))
    z = load("refine_3d_polytopes")
    check_tree_against_golden(device, z)
    check_outputs_against_golden(device, z)


# -- 14: the example ---------------------------------------------------------------------------------------------------------------------
def test_example_script_runs_end_to_end(tmp_path):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "s3_for_synthetic_STL_body.py"), str(tmp_path), "40000",
                          "3", "5"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "body with 1280 facets" in run.stdout
    for name in ("ellipsoid.stl", "metric_0.75.h5", "metric_0.75.xdmf"):
        path = os.path.join(str(tmp_path), name)
        assert os.path.exists(path) and os.path.getsize(path) > 1000, (name, os.listdir(str(tmp_path)))
    from sparsespatialsampling_amd.data import Dataloader
    loader = Dataloader(str(tmp_path), "metric_0.75.h5")
    assert len(loader.write_times) == 20 and loader.vertices.shape[1] == 3
