"""
The reference and the checker of tests/iso_cases.py (CPU only), and the host-side parts of sparsespatialsampling_amd/isosurface.py.

  tables       whether a primitive's last two vertices are swapped is DERIVED from affine fields (``iso_cases.swap_needed``); it
               depends on the parity of the permutation and the inside mask only, and equals the sets include/s3hip.h and the
               kernel file name for even permutations.
  affine       for every permutation and mask a field that is affine on the whole cell: every vertex lies on the plane within the
               bound, normals point down the gradient, the two triangles of a quad have the area of the convex hull of its points.
  closed       the uniform 8^3 grid with f = -|x - c| at level -0.21: 648 proper triangles, every undirected vertex-key pair twice,
               every directed pair once, V - E + F = 2, equal keys have equal bits; 2-D: 32 segments, every vertex key twice.
  checker      the float64 emulation passes; with one planted mistake at a time it fails.
"""
import numpy as np
import pytest

from tests import iso_cases as ic
from tests import sample_cases as sc

LD = ic.LD


def test_swap_depends_on_parity_and_mask_only():
    for d in (2, 3):
        sets = {0: set(), 1: set()}
        for s, (_, parity, _) in enumerate(ic.kuhn(d)):
            swapped = frozenset(m for m in range(1, (1 << (d + 1)) - 1) if ic.swap_needed(d, s, m))
            sets[parity].add(swapped)
        assert len(sets[0]) == 1 and len(sets[1]) == 1
        (even,), (odd,) = sets[0], sets[1]
        assert even | odd == set(range(1, (1 << (d + 1)) - 1)) and not even & odd
        if d == 3:
            assert even == {2, 5, 8, 10, 11, 14}
    assert [path for _, _, path in ic.kuhn(3)][0][0] == 4 and all(path[-1] == 2 for _, _, path in ic.kuhn(3))
    assert all(path[0] == 0 and path[-1] == 2 for _, _, path in ic.kuhn(2))


def affine_cell(d, simplex, mask, rng):
    """one cell with dyadic sizes and a field that is EXACTLY affine in float64, with the inside mask ``mask`` on simplex ``simplex``
    at level 0.5 -> (nodes, faces, field, level, gradient)"""
    perm, _, path = ic.kuhn(d)[simplex]
    size = 2.0 ** rng.integers(-2, 2, size=d)
    signs = sc.corner_signs(d)
    nodes = 0.25 * rng.integers(-8, 8, size=d) + (signs + 1) / 2 * size
    v = np.array([0.5 + (1 if mask >> p & 1 else -1) * rng.integers(1, 16) / 8 for p in range(d + 1)])
    g = np.zeros(d)
    for i, axis in enumerate(perm):
        g[axis] = (v[i + 1] - v[i]) / size[axis]
    field = (nodes.astype(LD) - nodes[path[0]].astype(LD)) @ g.astype(LD) + LD(v[0])
    assert np.array_equal(field.astype(np.float64).astype(LD), field)           # exactly representable
    return nodes, np.arange(1 << d)[None, :], field.astype(np.float64), 0.5, g


def hull_area(p):
    """area of the convex hull of four coplanar points in convex position"""
    c = p.mean(axis=0)
    n = np.cross(p[1] - p[0], p[2] - p[0])
    e1 = (p[0] - c) / np.linalg.norm(p[0] - c)
    e2 = np.cross(n / np.linalg.norm(n), e1)
    xy = np.stack([(p - c) @ e1, (p - c) @ e2], axis=1)
    xy = xy[np.argsort(np.arctan2(xy[:, 1], xy[:, 0]))]
    return 0.5 * abs(np.sum(xy[:, 0] * np.roll(xy[:, 1], -1) - np.roll(xy[:, 0], -1) * xy[:, 1]))


@pytest.mark.parametrize("d", [2, 3])
def test_affine_field_every_permutation_and_mask(d):
    rng = np.random.default_rng(d)
    for simplex in range(len(ic.kuhn(d))):
        for mask in range(1, (1 << (d + 1)) - 1):
            nodes, faces, field, level, g = affine_cell(d, simplex, mask, rng)
            ref = ic.extract(nodes, faces, field, level)
            emu = ic.extract(nodes, faces, field, level, arith="f64")
            ic.check(emu, ref, f"d={d} simplex {simplex} mask {mask}")
            assert (ref["simplex"] == simplex).sum() == len(ic.natural_primitives(d, mask))
            scale = np.abs(nodes).max() * np.abs(g).sum() + np.abs(field).max()
            for res, slack in ((ref, 0), (emu, ref["verts_bound"] @ np.abs(g).astype(LD))):
                x = res["verts"].astype(LD)
                on_plane = (x - nodes[0].astype(LD)) @ g.astype(LD) + LD(field[0]) - LD(level)
                assert (np.abs(on_plane) <= slack + LD(2) ** -58 * scale).all()
            x = emu["verts"]
            if d == 3:
                normal = np.cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0])
                mine = np.flatnonzero(ref["simplex"] == simplex)
                # (another simplex of the cell may have a corner exactly on the plane: its degenerate triangle has no normal)
                assert (normal[mine] @ g < 0).all() and ((normal @ g < 0) | (normal == 0).all(axis=1)).all()
                if len(mine) == 2:
                    quad = np.unique(x[mine].reshape(6, 3), axis=0)
                    assert len(quad) == 4
                    assert abs(0.5 * np.linalg.norm(normal[mine], axis=1).sum() - hull_area(quad)) <= 1e-12 * hull_area(quad)
            else:
                e = x[:, 1] - x[:, 0]
                left = np.stack([-e[:, 1], e[:, 0]], axis=1) @ g
                assert (left[ref["simplex"] == simplex] > 0).all() and ((left > 0) | (e == 0).all(axis=1)).all()


@pytest.mark.parametrize("d", [2, 3])
def test_uniform_grid_gives_a_closed_surface(d):
    c = ic.uniform(d)
    ref = ic.extract(c["nodes"], c["faces"], c["field"], ic.UNIFORM_LEVEL)
    emu = ic.extract(c["nodes"], c["faces"], c["field"], ic.UNIFORM_LEVEL, arith="f64")
    ic.assert_closed(ref, d, "long double")
    ic.assert_closed(emu, d, "float64")
    ic.check(emu, ref, "float64")
    assert ref["offsets"].tolist() == [0, 648 if d == 3 else 32]


def test_every_mask_case_reaches_every_mask():
    for d, n_snap in ((3, 256), (2, 16)):
        nodes, faces, field, level = ic.every_mask(d, n_snap)
        inside = field[faces] >= level                                          # [3, 2^d, T]
        for j in range(3):
            codes = (inside[j] << np.arange(1 << d)[:, None]).sum(axis=0)
            assert len(np.unique(codes)) == 1 << (1 << d)
        assert np.abs(field).max() < 2.0 ** 100 and np.abs(field - level).min() > 2.0 ** -100


def planted_case():
    """the uniform 3-D grid with two snapshots, a node value equal to the level and a NaN corner, both in cut cells"""
    c = ic.uniform(3)
    ref = ic.extract(c["nodes"], c["faces"], c["field"], ic.UNIFORM_LEVEL)
    field = np.stack([c["field"], c["field"] + 0.01], axis=1)
    field[c["faces"][ref["cells"][5], 0], 0] = ic.UNIFORM_LEVEL
    field[c["faces"][ref["cells"][400], 3], 1] = np.nan
    return c["nodes"], c["faces"], field, ic.UNIFORM_LEVEL


def test_honest_emulation_passes():
    nodes, faces, field, level = planted_case()
    ic.check(ic.extract(nodes, faces, field, level, arith="f64"), ic.extract(nodes, faces, field, level), "honest")


@pytest.mark.parametrize("mistake", ic.MISTAKES)
def test_planted_mistake_fails(mistake):
    nodes, faces, field, level = planted_case()
    ref = ic.extract(nodes, faces, field, level)
    with pytest.raises(AssertionError):
        ic.check(ic.extract(nodes, faces, field, level, arith="f64", mistake=mistake), ref, mistake)


@pytest.mark.parametrize("d", [2, 3])
def test_planted_mistake_fails_2d_and_3d_tables(d):
    """the swap table of either dimension: one flipped entry turns a primitive round"""
    c = ic.uniform(d)
    ref = ic.extract(c["nodes"], c["faces"], c["field"], ic.UNIFORM_LEVEL)
    with pytest.raises(AssertionError):
        ic.check(ic.extract(c["nodes"], c["faces"], c["field"], ic.UNIFORM_LEVEL, arith="f64", mistake="swap"), ref, "swap")


# ---- the host side of the package --------------------------------------------------------------------------------------------
def host_result(d):
    from sparsespatialsampling_amd.isosurface import IsoResult
    c = ic.uniform(d)
    field = np.stack([c["field"], c["field"] + 0.02, c["field"] - 5.0], axis=1)  # (the last snapshot is not cut)
    emu = ic.extract(c["nodes"], c["faces"], field, ic.UNIFORM_LEVEL, arith="f64")
    return c, field, IsoResult(emu["offsets"], emu["verts"], emu["edges"], emu["frac"], emu["cells"], n_nodes=len(c["nodes"]))


def test_package_exports():
    import sparsespatialsampling_amd as pkg
    from sparsespatialsampling_amd import isosurface
    assert pkg.Isosurface is isosurface.Isosurface and pkg.IsoResult is isosurface.IsoResult
    assert "Isosurface" in pkg.__all__ and "IsoResult" in pkg.__all__


@pytest.mark.parametrize("d", [2, 3])
def test_result_snapshot_weld_interpolate(d):
    c, field, res = host_result(d)
    assert len(res) == res.offsets[-1] and res.n_snapshots == 3 and res.dim == d
    assert len(res.snapshot(2)[0]) == 0
    with pytest.raises(IndexError):
        res.snapshot(3)
    for t in (0, 1):
        verts, edges, frac, cells = res.snapshot(t)
        points, index = res.weld(t)
        assert np.array_equal(points[index].view(np.int64), verts.view(np.int64))
        assert len(points) == len(np.unique(ic.vertex_keys(edges)))
    back = res.interpolate(field)
    fa = np.abs(field[res.edges[..., 0]]).max(axis=-1) + np.abs(field[res.edges[..., 1]]).max(axis=-1)
    assert (np.abs(back - ic.UNIFORM_LEVEL) <= 4 * 2.0 ** -53 * fa).all()
    one = res.interpolate(c["nodes"][:, 0].copy())
    assert np.allclose(one, res.vertices[..., 0], rtol=0, atol=1e-14)
    with pytest.raises(ValueError):
        res.interpolate(field[:, :2])


def test_write_stl_reads_back(tmp_path):
    from sparsespatialsampling_amd.geometry.geometry_STL_3d import read_stl
    _, _, res = host_result(3)
    path = str(tmp_path / "iso.stl")
    res.write_stl(path, 1)
    assert np.array_equal(read_stl(path), res.snapshot(1)[0].astype(np.float32).astype(np.float64))
    with pytest.raises(ValueError):
        res.write_stl(path, 2)
    with pytest.raises(ValueError):
        host_result(2)[2].write_stl(path, 0)
