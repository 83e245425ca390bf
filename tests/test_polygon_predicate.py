"""
The polygon predicate of ``GeometryCoordinates2D`` (host: geometry/coordinates_2d.py ``_Outline``; device: ``mask_polygon``
kernel, csrc/tree.hip) against an INDEPENDENT implementation: winding number with exact rational arithmetic, boundary
points classified by exact collinearity.  The reference delegates to shapely (``Point.within(Polygon)``,
coordinates_2d.py:70: interior only, boundary excluded); shapely / GEOS are not installed here, so GEOS itself is pinned only
by the six expectations of the reference's tests/test_coordinates_2d_geometry.py:39-49 (restated in
tests/test_reference_expectations.py).  This file pins the *semantics* (strict interior of a simple polygon) on the cases
where crossing-number code usually goes wrong: rays through vertices, nodes exactly on edges and vertices, collinear
consecutive edges, horizontal edges at the ray's height, a duplicated closing point, clockwise outlines, concave shapes.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch as pt

from sparsespatialsampling_amd.geometry import GeometryCoordinates2D
from sparsespatialsampling_amd.geometry.coordinates_2d import _Outline

S = 1.0 / 16.0          # lattice pitch: every polygon vertex and every test node below is a multiple of S (exact in binary)

POLYGONS = {
    "square": [(4, 4), (12, 4), (12, 12), (4, 12)],
    "square_clockwise_closed": [(4, 4), (4, 12), (12, 12), (12, 4), (4, 4)],              # duplicate closing point
    "l_shape": [(2, 2), (14, 2), (14, 6), (6, 6), (6, 14), (2, 14)],
    "collinear_edges": [(2, 2), (8, 2), (14, 2), (14, 8), (14, 14), (8, 14), (2, 14), (2, 8)],
    "diamond": [(8, 1), (15, 8), (8, 15), (1, 8)],                                        # vertices at the ray height
    "comb": [(1, 1), (15, 1), (15, 13), (12, 13), (12, 5), (9, 5), (9, 13), (6, 13), (6, 5), (3, 5), (3, 13), (1, 13)],
    "star": [(8, 15), (10, 10), (15, 8), (10, 6), (8, 1), (6, 6), (1, 8), (6, 10)],
    "thin_triangle": [(1, 8), (15, 9), (15, 7)],
    "steps": [(2, 2), (6, 2), (6, 4), (10, 4), (10, 6), (14, 6), (14, 12), (2, 12)],      # horizontal edges at node heights
}


def outline(name):
    return np.array(POLYGONS[name], dtype=np.float64) * S


def exact_strict_interior(poly, px, py):
    """independent reference: boundary -> False; otherwise the winding number (Sunday) with exact rational arithmetic"""
    pts = [(Fraction(float(x)), Fraction(float(y))) for x, y in poly]
    if pts[0] == pts[-1]:
        pts = pts[:-1]
    p = (Fraction(float(px)), Fraction(float(py)))
    n, wn = len(pts), 0
    for i in range(n):
        a, b = pts[i], pts[(i + 1) % n]
        left = (b[0] - a[0]) * (p[1] - a[1]) - (p[0] - a[0]) * (b[1] - a[1])
        if left == 0 and min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1]):
            return False                                    # on the boundary
        if a[1] <= p[1]:
            if b[1] > p[1] and left > 0:
                wn += 1
        elif b[1] <= p[1] and left < 0:
            wn -= 1
    return wn != 0


def lattice_points():
    g = np.arange(0, 33) * (S / 2)                         # half-pitch lattice: hits vertices, edges and edge mid-points
    return np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)


@pytest.mark.parametrize("name", sorted(POLYGONS))
def test_host_predicate_vs_exact_winding_number(name):
    poly = outline(name)
    o = _Outline(poly)
    rng = np.random.default_rng(len(name))
    pts = np.concatenate([lattice_points(), rng.random((400, 2))])
    want = np.array([exact_strict_interior(poly, x, y) for x, y in pts])
    got = np.array([o.strictly_inside(float(x), float(y)) for x, y in pts])
    assert want.any() and (~want).any() and np.array_equal(got, want), pts[got != want][:5]
    # a vertex, an edge mid-point: boundary, hence outside
    assert not o.strictly_inside(*poly[0]) and not o.strictly_inside(*(0.5 * (poly[0] + poly[1])))


@pytest.mark.parametrize("name", ["square", "l_shape", "diamond"])
def test_check_cell_semantics(name):
    """keep_inside=False: a cell is removed only when ALL its nodes are strictly inside; in refine mode it is selected
    when ANY node is (reference geometry_base.py:58-76)"""
    poly = outline(name)
    g = GeometryCoordinates2D("body", False, poly, refine=True)
    rng = np.random.default_rng(3)
    for _ in range(200):
        c = (rng.integers(1, 31, 2) * (S / 2))
        h = S / 2 * rng.integers(1, 3)
        nodes = np.array([[c[0] - h, c[1] - h], [c[0] - h, c[1] + h], [c[0] + h, c[1] + h], [c[0] + h, c[1] - h]])
        inside = np.array([exact_strict_interior(poly, x, y) for x, y in nodes])
        t = pt.from_numpy(nodes)
        assert g.check_cell(t) == bool(inside.all()) and g.check_cell(t, refine_geometry=True) == bool(inside.any())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(POLYGONS))
def test_device_kernel_vs_exact_winding_number(name):
    """the ``mask_polygon`` kernel on every cell of the level-4 and level-5 lattices of the unit square (nodes on vertices,
    on edges, on the ray through vertices ...) against the exact reference, both modes, both ``keep_inside`` settings"""
    from sparsespatialsampling_amd import hipops
    poly = outline(name)
    poly_dev = hipops.to_device(np.ascontiguousarray(_Outline(poly).xy))
    for level in (4, 5):
        m = 2 ** level
        ij = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 2)
        centers = (ij + 0.5) / m
        h = 0.5 / m
        offs = np.array([[-h, -h], [-h, h], [h, h], [h, -h]])
        inside = np.array([[exact_strict_interior(poly, *(c + o)) for o in offs] for c in centers])
        d_center = hipops.to_device(np.ascontiguousarray(centers))
        d_level = hipops.to_device(np.full(len(centers), level, dtype=np.int32))
        for refine_mode in (0, 1):
            for keep_inside in (0, 1):
                flags = pt.zeros(len(centers), dtype=pt.uint8, device="cuda")
                hipops.mask_polygon(hipops.MaskCells(d_center, d_level, 1.0, flags), poly_dev, refine_mode, keep_inside)
                if not refine_mode:
                    want = inside.all(1) if not keep_inside else ~inside.any(1)
                else:
                    want = inside.any(1) if not keep_inside else ~inside.all(1)
                assert np.array_equal(flags.cpu().numpy().astype(bool), want), (level, refine_mode, keep_inside)
