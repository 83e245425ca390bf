"""GeometrySTL3D on the host: reader, closed-surface check, the exact point-in-mesh predicate (on the surface, or an odd
number of crossings of the ray in +x), column bins, and a full refine through the CPU oracle backend.  No GPU needed;
tests/test_gpu_mask_mesh.py holds the device kernel to the same verdicts byte for byte."""
import logging
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch as pt

import sparsespatialsampling_amd.s_cube as s_cube
from sparsespatialsampling_amd import geometry
from sparsespatialsampling_amd.geometry import GeometrySTL3D
from sparsespatialsampling_amd.geometry import geometry_STL_3d as stl
from tests import stl_meshes as M
from tests.oracle_backend import OracleTreeBackend
from tests.test_tree_host_logic import check_outputs_against_golden, check_tree_against_golden, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def oracle_backend(monkeypatch):
    monkeypatch.setattr(s_cube, "_make_backend", lambda v, t, k: OracleTreeBackend(v, t, k))


def node_lattice(lo, hi, n):
    axis = lo + (hi - lo) * np.arange(n + 1) / n
    return np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3)


# -- 1: the reference's own expectations (its tests/test_geometry_STL.py with tests/const.py:DummyCells) ---------------------------
INSIDE = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]]
DUMMY_CELLS = {"inside": pt.tensor(INSIDE, dtype=pt.float32), "outside": pt.tensor(INSIDE, dtype=pt.float32) + 5.0,
               "partially": pt.tensor(INSIDE, dtype=pt.float32) + 0.5}


@pytest.mark.parametrize("keep_inside, cell, expected", [(False, "outside", False), (False, "inside", True),
                                                         (False, "partially", False), (True, "outside", True),
                                                         (True, "inside", False), (True, "partially", False)])
def test_reference_expectations_check_cell(keep_inside, cell, expected):
    cube = GeometrySTL3D("cube", keep_inside=keep_inside, path_stl_file=M.CUBE_STL)
    assert cube.check_cell(DUMMY_CELLS[cell]) is expected
    assert cube.check_cell(DUMMY_CELLS[cell].double()) is expected


def test_reference_expectations_pre_check_and_attributes():
    cube = GeometrySTL3D("cube", keep_inside=False, path_stl_file=M.CUBE_STL)
    assert cube.pre_check_cell(DUMMY_CELLS["inside"]) is True
    assert cube.pre_check_cell(DUMMY_CELLS["outside"]) is False
    assert cube.type == "STL" and cube.main_width == 1.0 and cube.center.tolist() == [0.5, 0.5, 0.5]
    assert cube.name == "cube" and cube.keep_inside is False and cube.refine is False
    spec = cube.kernel_spec()
    assert spec[0] == "mesh" and spec[1].shape == (12, 3, 3) and spec[1].dtype == np.float64


# -- 2: exact bodies, every node of a lattice that puts nodes on faces, edges, corners and rays into face planes --------------------
def closed_box(p, lo, hi):
    return ((p >= np.asarray(lo)) & (p <= np.asarray(hi))).all(1)


def test_unit_cube_every_lattice_node():
    cube = GeometrySTL3D("cube", False, M.CUBE_STL)
    p = node_lattice(-0.5, 1.5, 16)            # spacing 1/8: holds the nodes of the level-3 cells of [-0.5, 1.5]^3 and their centres
    truth = closed_box(p, [0, 0, 0], [1, 1, 1])
    assert len(p) == 4913 and truth.sum() == 729
    assert np.array_equal(cube.inside(p), truth)


def test_l_shaped_body_every_lattice_node(tmp_path):
    """nodes in the notch are inside the bounding box and outside the body; their rays run in face planes and through the
    re-entrant edge"""
    body = GeometrySTL3D("L", False, M.write_binary_stl(tmp_path / "l.stl", M.l_shape_facets()))
    p = node_lattice(-0.5, 1.5, 16)
    truth = closed_box(p, [0, 0, 0], [1, 0.5, 1]) | closed_box(p, [0, 0, 0], [0.5, 1, 1])
    notch = closed_box(p, [0, 0, 0], [1, 1, 1]) & ~truth
    assert notch.sum() > 100 and truth.sum() == 9 * 9 * 9 - notch.sum()
    assert np.array_equal(body.inside(p), truth)


# -- 3: flat-faced bodies with float32-rounded, non-dyadic corners against the analytic classes -------------------------------------
def analytic_inside(analytic, points):
    if isinstance(analytic, geometry.CubeGeometry):
        return geometry.cube_geometry.mask_box(pt.from_numpy(points), analytic._lower_bound, analytic._upper_bound).numpy()
    return analytic._inside(pt.from_numpy(points)).numpy()


@pytest.mark.parametrize("kind", ["tet", "prism", "pyramid", "box"])
def test_flat_bodies_equal_the_analytic_classes_on_every_cell(tmp_path, kind):
    """all cells of the level-4 and level-5 lattices of the unit domain, both keep_inside, both refine_geometry, no cell left
    out.  The per-node predicates (what ``check_cell`` feeds to ``_apply_mask`` in either class) are evaluated once per lattice
    node -- the analytic tetrahedron takes four torch.dot calls per node -- and every cell's verdict is formed from them; the
    public ``check_cell`` of both classes is then compared directly on 300 seeded cells per level."""
    rng = np.random.default_rng(5)
    nodes32 = node_lattice(0.0, 1.0, 32)                              # the nodes of both levels, each once
    on_grid = {}
    for keep_inside in (False, True):
        analytic, mesh = M.flat_body(kind, keep_inside, tmp_path)
        if not on_grid:
            on_grid = {"analytic": analytic_inside(analytic, nodes32).reshape(33, 33, 33),
                       "mesh": mesh.inside(nodes32).reshape(33, 33, 33)}
            assert 0 < on_grid["mesh"].sum() < on_grid["mesh"].size
        for level in (4, 5):
            center, lv = M.lattice_cells(0.0, 1.0, level)
            nodes = M.cell_nodes(center, lv, 1.0)
            at = np.rint(nodes * 32).astype(np.int64)
            assert np.array_equal(at / 32.0, nodes)                   # the lattice is dyadic: node coordinates are exact
            per_node = {k: v[at[..., 0], at[..., 1], at[..., 2]] for k, v in on_grid.items()}
            sample = rng.choice(len(center), 300, replace=False)
            for refine_mode in (False, True):
                want = M.apply_mask(per_node["analytic"], keep_inside, refine_mode)
                got = M.apply_mask(per_node["mesh"], keep_inside, refine_mode)
                assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} of {len(want)} cells differ"
                direct = M.host_verdicts(mesh, center[sample], lv[sample], 1.0, refine_mode)
                assert np.array_equal(direct, got[sample])
                assert np.array_equal(direct, M.host_verdicts(analytic, center[sample], lv[sample], 1.0, refine_mode))


# -- 4: curved body against the generalised winding number --------------------------------------------------------------------------
def winding_number(tri, points):
    """sum of the signed solid angles of the facets (van Oosterom & Strackee) / 4 pi, in long double"""
    tri, total = tri.astype(np.longdouble), np.zeros(len(points), dtype=np.longdouble)
    for s in range(0, len(points), 256):
        p = points[s:s + 256].astype(np.longdouble)[:, None, :]
        a, b, c = tri[None, :, 0] - p, tri[None, :, 1] - p, tri[None, :, 2] - p
        la, lb, lc = (np.sqrt((v * v).sum(-1)) for v in (a, b, c))
        num = (a * np.cross(b, c)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        total[s:s + 256] = (2 * np.arctan2(num, den)).sum(1)
    return total / (4 * np.longdouble(np.pi))


def test_icosphere_against_the_winding_number(tmp_path):
    tri = M.icosphere_facets(3, center=(0.31, -0.17, 0.43), radius=0.77)
    assert len(tri) == 1280
    body = GeometrySTL3D("ball", False, M.write_binary_stl(tmp_path / "ball.stl", tri))
    lo, hi = np.array(body._lower_bound), np.array(body._upper_bound)
    mid, side = (lo + hi) / 2, (hi - lo).max()
    points = mid + (np.random.default_rng(11).random((20000, 3)) - 0.5) * side
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    to_plane = np.abs(((points[:, None, :] - tri[None, :, 0]) * normal[None]).sum(-1)).min(1)
    usable = to_plane >= 1e-9 * np.linalg.norm(hi - lo)
    assert np.count_nonzero(~usable) <= 0.001 * len(points)
    w = winding_number(tri, points)
    assert np.abs(np.abs(w) - np.rint(np.abs(w))).max() < 1e-9          # a closed surface: the oracle itself is sharp
    truth = np.abs(w) > 0.5
    assert 0.4 < truth.mean() < 0.6                                        # pi/6 of the cube
    assert np.array_equal(body.inside(points)[usable], truth[usable])


# -- 5: what the file's bookkeeping may not change ------------------------------------------------------------------------------------
def test_facet_order_and_orientation_do_not_matter(tmp_path):
    tri = M.icosphere_facets(2, radius=0.9)
    rng = np.random.default_rng(3)
    shuffled = tri[rng.permutation(len(tri))]
    for i in range(len(shuffled)):
        shuffled[i] = shuffled[i][rng.permutation(3)]                     # rotates and flips
    a = GeometrySTL3D("a", False, M.write_binary_stl(tmp_path / "a.stl", tri))
    b = GeometrySTL3D("b", False, M.write_binary_stl(tmp_path / "b.stl", shuffled))
    points = (rng.random((5000, 3)) - 0.5) * 2.0
    on_surface = np.concatenate([tri[:, 0], tri.mean(1), (tri[:, 0] + tri[:, 1]) / 2])
    assert a.inside(tri[:, 0]).all()                                      # vertices are on the surface
    for p in (points, on_surface):
        assert np.array_equal(a.inside(p), b.inside(p))


def test_ascii_and_binary_give_the_same_facets(tmp_path):
    tri = M.tetrahedron_facets(M.TET)
    binary = GeometrySTL3D("b", False, M.write_binary_stl(tmp_path / "b.stl", tri))
    ascii_ = GeometrySTL3D("a", False, M.write_ascii_stl(tmp_path / "a.stl", tri))
    assert np.array_equal(binary.kernel_spec()[1], ascii_.kernel_spec()[1])
    assert np.array_equal(np.sort(binary.kernel_spec()[1].reshape(-1, 3), axis=0), np.sort(tri.reshape(-1, 3), axis=0))
    ico = M.icosphere_facets(1)
    assert np.array_equal(stl.read_stl(M.write_ascii_stl(tmp_path / "i.stl", ico)), ico)
    assert np.array_equal(stl.read_stl(M.CUBE_STL).shape, (12, 3, 3))      # binary although it starts with text
    with open(M.CUBE_STL, "rb") as f:
        assert not f.read(84)[:80].strip(b"\0 ") == b""


# -- 6: errors, reduce_by, pickle ---------------------------------------------------------------------------------------------------------
def test_open_missing_and_truncated_files(tmp_path):
    tri = M.icosphere_facets(1)
    with pytest.raises(ValueError, match=r"open\.stl.*3 of"):
        GeometrySTL3D("open", False, M.write_binary_stl(tmp_path / "open.stl", tri[1:]))
    with pytest.raises(FileNotFoundError):
        GeometrySTL3D("none", False, str(tmp_path / "no_such.stl"))
    full = open(M.write_binary_stl(tmp_path / "full.stl", tri), "rb").read()
    for name, content in (("empty.stl", b""), ("cut.stl", full[:-7]), ("header.stl", full[:60])):
        (tmp_path / name).write_bytes(content)
        with pytest.raises(ValueError):
            GeometrySTL3D("bad", False, str(tmp_path / name))
    text = open(M.write_ascii_stl(tmp_path / "text.stl", tri)).read()
    (tmp_path / "cut_text.stl").write_text(text[:len(text) // 2])
    with pytest.raises(ValueError):
        GeometrySTL3D("bad", False, str(tmp_path / "cut_text.stl"))


@pytest.mark.parametrize("reduce_by, fragment", [(-1, "invalid negative value"), (0.5, "full surface"), (2, "reduce_by=0.99")])
def test_reduce_by_warns_and_changes_nothing(tmp_path, caplog, reduce_by, fragment):
    path = M.write_binary_stl(tmp_path / "ball.stl", M.icosphere_facets(2))
    plain = GeometrySTL3D("ball", False, path)
    with caplog.at_level(logging.WARNING):
        reduced = GeometrySTL3D("ball", False, path, reduce_by=reduce_by)
    assert any(fragment in r.getMessage() for r in caplog.records)
    assert sorted(os.listdir(tmp_path)) == ["ball.stl"]
    points = (np.random.default_rng(1).random((3000, 3)) - 0.5) * 2.2
    assert np.array_equal(plain.inside(points), reduced.inside(points))
    assert np.array_equal(plain.kernel_spec()[1], reduced.kernel_spec()[1])


def test_pickle_round_trip(tmp_path):
    body = GeometrySTL3D("ball", False, M.write_binary_stl(tmp_path / "ball.stl", M.icosphere_facets(2)), refine=True,
                         min_refinement_level=4)
    copy = pickle.loads(pickle.dumps(body))
    points = (np.random.default_rng(2).random((3000, 3)) - 0.5) * 2.2
    assert np.array_equal(body.inside(points), copy.inside(points))
    assert copy.name == "ball" and copy.refine and copy.min_refinement_level == 4 and copy.type == "STL"
    for a, b in zip(body.kernel_spec()[1:], copy.kernel_spec()[1:]):
        assert np.array_equal(a, b)


# -- 7: column bins -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subdivisions", [1, 3])
def test_column_bins_list_a_superset(tmp_path, subdivisions):
    body = GeometrySTL3D("ball", False, M.write_binary_stl(tmp_path / "ball.stl",
                                                           M.icosphere_facets(subdivisions, (0.1, 0.2, 0.3), 0.6)))
    _, tri, lo, hi, ny, nz, bin_start, bin_facet = body.kernel_spec()
    assert bin_start.dtype == np.int32 and bin_facet.dtype == np.int32 and bin_start.shape == (ny * nz + 1,)
    assert bin_start[0] == 0 and bin_start[-1] == len(bin_facet) and (np.diff(bin_start) >= 0).all()
    assert bin_facet.min() >= 0 and bin_facet.max() < len(tri)
    if subdivisions == 3:
        assert ny * nz > 100 and len(bin_facet) <= 8 * len(tri) + 64
    rng = np.random.default_rng(4)
    yz = lo[1:] + rng.random((10000, 2)) * (hi[1:] - lo[1:])
    yz[:100] = tri[rng.integers(0, len(tri), 100), 0, 1:]                 # and points exactly on bounding-box edges of facets
    col = (stl.bin_index(yz[:, 0], lo[1], stl.bin_scale(lo[1], hi[1], ny), ny) * nz
           + stl.bin_index(yz[:, 1], lo[2], stl.bin_scale(lo[2], hi[2], nz), nz))
    y_min, y_max, z_min, z_max = tri[:, :, 1].min(1), tri[:, :, 1].max(1), tri[:, :, 2].min(1), tri[:, :, 2].max(1)
    for (y, z), c in zip(yz, col):
        needed = np.flatnonzero((y_min <= y) & (y <= y_max) & (z_min <= z) & (z <= z_max))
        assert np.isin(needed, bin_facet[bin_start[c]:bin_start[c + 1]]).all()


# -- 8: a full refine on the CPU ------------------------------------------------------------------------------------------------------------
def test_refine_with_tessellated_polytopes_on_the_host(oracle_backend, tmp_path):
    """case refine_3d_polytopes with prism, tetrahedron and pyramid as GeometrySTL3D (host predicate): the grid of the analytic
    classes on the same float32-rounded corners, and the reference's golden grid"""
    grids = {}
    for mesh in (True, False):
        x, y, geos, kw = M.polytopes_case(tmp_path, mesh=mesh, host_only=True)
        assert mesh == any(isinstance(g, M.HostOnly) for g in geos)
        tree = s_cube.SamplingTree(pt.from_numpy(x), pt.from_numpy(y), geometry_obj=geos, **kw)
        tree.refine()
        grids[mesh] = M.grid_of(tree)
        if mesh:
            mesh_tree = tree
    for a, b in zip(grids[True], grids[False]):
        assert np.array_equal(a, b)
    # rounding the corners to float32 moves a face by ~1e-9, no lattice node is that close: the reference's grid too
    z = load("refine_3d_polytopes")
    check_tree_against_golden(mesh_tree, z)
    check_outputs_against_golden(mesh_tree, z)


# -- 9: the import-name alias ---------------------------------------------------------------------------------------------------------------
def test_alias_exports_the_class():
    code = ("import sparseSpatialSampling.geometry.geometry_STL_3d as m\n"
            "from sparseSpatialSampling.geometry import GeometrySTL3D\n"
            "import sparsespatialsampling_amd.geometry as g\n"
            "assert m.GeometrySTL3D is GeometrySTL3D is g.GeometrySTL3D and 'GeometrySTL3D' in g.__all__\n"
            "print('alias ok')\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "compat"), ROOT]))
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "alias ok" in out.stdout, out.stderr
