"""Shared helpers of the GeometrySTL3D tests (CPU: test_geometry_stl.py, GPU: test_gpu_mask_mesh.py): STL writers, the
tessellated test bodies, cell lattices and the proxy that hides ``kernel_spec``.  Not a test module."""
import os

import numpy as np
import torch as pt

from sparsespatialsampling_amd import geometry
from sparsespatialsampling_amd.s_cube import _directions

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CUBE_STL = os.path.join(GOLDEN, "cube.stl")


def f32(values):
    """coordinates as the float32 numbers an STL file can hold, widened back to float64"""
    return np.asarray(values, dtype=np.float64).astype(np.float32).astype(np.float64)


# -- writers ---------------------------------------------------------------------------------------------------------
def write_binary_stl(path, tri, header=b"solid written as binary on purpose"):
    tri = np.asarray(tri, dtype=np.float32).reshape(-1, 3, 3)
    rec = np.zeros(len(tri), dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]))
    rec["v"] = tri
    with open(path, "wb") as f:
        f.write(header.ljust(80, b" ")[:80])
        f.write(np.uint32(len(tri)).tobytes())
        f.write(rec.tobytes())
    return str(path)


def write_ascii_stl(path, tri):
    tri = np.asarray(tri, dtype=np.float32).reshape(-1, 3, 3)
    with open(path, "w") as f:
        f.write("solid body\n")
        for t in tri:
            f.write(" facet normal 0 0 0\n  outer loop\n")
            for v in t:
                f.write("   vertex %.9g %.9g %.9g\n" % tuple(float(c) for c in v))
            f.write("  endloop\n endfacet\n")
        f.write("endsolid body\n")
    return str(path)


# -- bodies (facets [nt, 3, 3], outward orientation) ---------------------------------------------------------------------
def tetrahedron_facets(p):
    p = np.asarray(p, dtype=np.float64)
    tri = np.array([[p[0], p[1], p[2]], [p[0], p[1], p[3]], [p[0], p[2], p[3]], [p[1], p[2], p[3]]])
    return orient_outward(tri, p.mean(0))


def extruded_facets(outline_xy, z0, z1, cap_triangles):
    """polygon ``outline_xy`` (counter-clockwise) extruded from z0 to z1; ``cap_triangles`` = vertex triples of the outline
    that tile it using outline vertices only (so that the caps and the walls share every edge)"""
    xy = np.asarray(outline_xy, dtype=np.float64)
    lo = np.column_stack([xy, np.full(len(xy), z0)])
    hi = np.column_stack([xy, np.full(len(xy), z1)])
    tri = []
    for i, j, k in cap_triangles:
        tri += [[lo[i], lo[k], lo[j]], [hi[i], hi[j], hi[k]]]
    for i in range(len(xy)):
        j = (i + 1) % len(xy)
        tri += [[lo[i], lo[j], hi[j]], [lo[i], hi[j], hi[i]]]
    return np.array(tri)


def prism_facets(triangle_xy, z0, z1):
    return extruded_facets(triangle_xy, z0, z1, [(0, 1, 2)])


def box_facets(lo, hi):
    return extruded_facets([(lo[0], lo[1]), (hi[0], lo[1]), (hi[0], hi[1]), (lo[0], hi[1])], lo[2], hi[2],
                           [(0, 1, 2), (0, 2, 3)])


def l_shape_facets():
    """union of the closed boxes [0,1]x[0,0.5]x[0,1] and [0,0.5]x[0,1]x[0,1] as ONE closed surface (no interior wall)"""
    outline = [(0.0, 0.0), (1.0, 0.0), (1.0, 0.5), (0.5, 0.5), (0.5, 1.0), (0.0, 1.0)]
    return extruded_facets(outline, 0.0, 1.0, [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 5)])


def pyramid_facets(base, apex):
    """``base``: the four corners in order around the square"""
    b, a = np.asarray(base, dtype=np.float64), np.asarray(apex, dtype=np.float64)
    tri = [[b[0], b[1], b[2]], [b[0], b[2], b[3]]] + [[b[i], b[(i + 1) % 4], a] for i in range(4)]
    return orient_outward(np.array(tri), (b.sum(0) + a) / 5)


def orient_outward(tri, interior):
    tri = np.array(tri, dtype=np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    flip = ((tri.mean(1) - interior) * n).sum(1) < 0
    tri[flip] = tri[flip][:, [0, 2, 1]]
    return tri


def icosphere_facets(subdivisions, center=(0.0, 0.0, 0.0), radius=1.0):
    """20 * 4^subdivisions facets, consistently outward, vertices rounded to float32 (shared vertices stay shared)"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
             (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    verts = [np.asarray(v, dtype=np.float64) / np.linalg.norm(v) for v in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
             (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
             (9, 8, 1)]
    for _ in range(subdivisions):
        middle, finer = {}, []

        def mid(i, j):
            key = (min(i, j), max(i, j))
            if key not in middle:
                m = verts[i] + verts[j]
                verts.append(m / np.linalg.norm(m))
                middle[key] = len(verts) - 1
            return middle[key]

        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            finer += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = finer
    points = f32(np.asarray(verts) * radius + np.asarray(center, dtype=np.float64))
    return points[np.asarray(faces)]


# -- the flat-faced bodies of the comparisons with the analytic classes: float32-rounded, non-dyadic corners -----------------
TET = f32([[0.6, 0.1, 0.1], [0.95, 0.15, 0.1], [0.7, 0.45, 0.15], [0.75, 0.2, 0.5]])
PRISM_XY, PRISM_Z = f32([(0.1, 0.1), (0.3, 0.1), (0.1, 0.35)]), f32([0.1, 0.4])
PYRAMID_BASE = f32([[0.3, 0.55, 0.2], [0.7, 0.55, 0.2], [0.7, 0.9, 0.2], [0.3, 0.9, 0.2]])
PYRAMID_APEX = f32([0.5, 0.7, 0.7])
BOX_LO, BOX_HI = f32([0.21, 0.33, 0.17]), f32([0.83, 0.71, 0.93])


def flat_body(kind, keep_inside, folder, **kw):
    """-> (analytic geometry, GeometrySTL3D of the tessellated body), both from the same float32-rounded corners (the bodies of
    case ``refine_3d_polytopes`` of tests/golden/inputs.py, and a box)"""
    path = os.path.join(str(folder), f"{kind}.stl")
    if kind == "tet":
        analytic = geometry.TetrahedronGeometry3D(kind, keep_inside, TET.tolist(), **kw)
        tri = tetrahedron_facets(TET)
    elif kind == "prism":
        ends = [[(float(x), float(y), float(z)) for x, y in PRISM_XY] for z in PRISM_Z]
        analytic = geometry.PrismGeometry3D(kind, keep_inside, ends, **kw)
        tri = prism_facets(PRISM_XY, PRISM_Z[0], PRISM_Z[1])
    elif kind == "pyramid":
        analytic = geometry.PyramidGeometry3D(kind, keep_inside, PYRAMID_BASE.tolist() + [PYRAMID_APEX.tolist()], **kw)
        tri = pyramid_facets(PYRAMID_BASE, PYRAMID_APEX)
    else:
        analytic = geometry.CubeGeometry(kind, keep_inside, BOX_LO.tolist(), BOX_HI.tolist(), **kw)
        tri = box_facets(BOX_LO, BOX_HI)
    if not os.path.exists(path):
        write_binary_stl(path, tri)
    return analytic, geometry.GeometrySTL3D(kind, keep_inside, path, **kw)


# -- cells -----------------------------------------------------------------------------------------------------------
def lattice_cells(lo, width, level):
    """all cells of one level of the cube ``[lo, lo + width]^3`` -> (centres [n, 3] f64, levels [n] i32)"""
    n = 2 ** level
    axis = lo + (np.arange(n) + 0.5) * (width / n)
    c = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(c), np.full(len(c), level, dtype=np.int32)


def cell_nodes(center, level, width):
    """node coordinates [n, 8, 3] as the refine loop forms them: centre + direction * (0.5 * width) / 2^level"""
    half = (0.5 * float(width)) / (2.0 ** np.asarray(level, dtype=np.float64))
    return center[:, None, :] + _directions(3)[None, :, :] * half[:, None, None]


def apply_mask(inside, keep_inside, refine_mode):
    """GeometryObject._apply_mask for per-node masks [n, 8] -> verdicts [n]"""
    count = inside.sum(1)
    if refine_mode:
        return count != inside.shape[1] if keep_inside else count > 0
    return count == 0 if keep_inside else count == inside.shape[1]


def host_verdicts(geo, center, level, width, refine_mode):
    """``geo.check_cell`` cell by cell"""
    nodes = pt.from_numpy(cell_nodes(center, level, width))
    return np.array([bool(geo.check_cell(nodes[i], bool(refine_mode))) for i in range(len(nodes))])


class HostOnly:
    """a geometry seen through the reference's interface only: ``kernel_spec`` is hidden, so every verdict of the refine loop
    comes from the host ``check_cell`` (the DuckGeometry idea of tests/test_tree_host_logic.py)"""

    def __init__(self, inner):
        self._inner = inner

    def check_cell(self, cell_nodes, refine_geometry=False):
        return self._inner.check_cell(cell_nodes, refine_geometry)

    def __getattr__(self, item):
        if item == "kernel_spec":
            raise AttributeError(item)
        return getattr(self._inner, item)


def polytopes_case(folder, mesh, host_only):
    """inputs of case ``refine_3d_polytopes`` with its three bodies rebuilt from float32-rounded corners: as GeometrySTL3D of the
    tessellated bodies (``mesh``; behind ``HostOnly`` if asked) or as the analytic classes"""
    from inputs import refine_inputs
    x, y, geos, kw = refine_inputs("refine_3d_polytopes", geometry)
    bodies = []
    for kind, extra in (("prism", {}), ("tet", {}), ("pyramid", dict(refine=True))):
        analytic, stl = flat_body(kind, False, folder, **extra)
        body = stl if mesh else analytic
        bodies.append(HostOnly(body) if mesh and host_only else body)
    assert [g.name for g in geos[1:]] == ["prism", "tet", "pyramid"]
    return x, y, [geos[0]] + bodies, kw


def grid_of(tree):
    return (tree.all_centers.numpy(), tree.all_levels.numpy(), tree.face_ids.numpy(), tree.all_nodes.numpy())
