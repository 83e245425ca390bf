"""Closed triangle meshes read from an STL file as 3-D bodies (or as the domain).  API mirror of the reference's
``geometry/geometry_STL_3d.py`` (constructor arguments, ``type == "STL"``, bounding-box ``main_width`` / ``center``,
``pre_check_cell``).

The reference delegates to pyvista / pymeshfix (``vtkSelectEnclosedPoints``: random rays, a tolerance of 0.1 % of the
bounding-box diagonal).  This package carries its own reader (numpy only) and its own point-in-mesh predicate, so that the
same float64 arithmetic runs on the host (``check_cell``) and in the ``s3_mask_mesh`` kernel:

    A point is inside iff it lies ON the surface or its ray in +x crosses the surface an odd number of times.

Per facet (vertices ``a < b < c`` in lexicographic (x, y, z) order, so that the stored orientation and vertex rotation of
the file do not matter and every shared edge is evaluated from the same endpoint by both of its facets)::

    n   = (b - a) x (c - a)                       vol = (nx*dx + ny*dy) + nz*dz     with d = p - a
    box = p's (y, z) within the closed (y, z) bounding box of the facet
    on      = box and vol == 0 and p within the closed triangle in the projection that drops n's dominant axis
    crossed = box and vol != 0 and nx != 0 and (vol < 0) != (nx < 0)          # ray/plane intersection at x > px
              and an odd number of the edges (a,b), (a,c), (b,c) has
              (Pz > pz) != (Qz > pz) and py < Py + (pz - Pz) * (Qy - Py) / (Qz - Pz)     # half-open crossing rule

No tolerance anywhere.  Facets are binned once into a uniform grid of (y, z) columns by their closed projected bounding
boxes; as ``box`` is part of the predicate, a point needs the facets of its own column only and the bins cannot change a
verdict.  Mesh repair and decimation are not implemented ("Deviations").
"""
import logging
import os
from typing import Union

import numpy as np
from torch import Tensor, from_numpy, tensor

from .cube_geometry import mask_box
from .geometry_base import GeometryObject

logger = logging.getLogger(__name__)

MAX_BINS = 1 << 20            # cap of the column table (ny * nz)
_HOST_BLOCK = 1 << 18         # point x facet pairs evaluated at once by the host predicate


# -- reader ----------------------------------------------------------------------------------------------------------
def read_stl(path: str) -> np.ndarray:
    """facets ``[nt, 3, 3]`` float64 (widened once from the file's float32) of a binary or ASCII STL file; the stored
    normals are ignored.  Binary is recognised by its size matching the count field, not by the word ``solid``."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"STL file '{path}' does not exist.")
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) >= 84:
        count = int(np.frombuffer(raw, dtype="<u4", count=1, offset=80)[0])
        if len(raw) == 84 + 50 * count:
            if count == 0:
                raise ValueError(f"STL file '{path}' holds no facets.")
            rec = np.frombuffer(raw, dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]),
                                count=count, offset=84)
            return _checked(rec["v"].astype(np.float64), path)
    tokens = raw.split()
    if not tokens or tokens[0] != b"solid":
        raise ValueError(f"STL file '{path}' is neither a complete binary STL (its size does not match its facet count) "
                         f"nor an ASCII STL (empty or truncated file?).")
    at = [i for i, t in enumerate(tokens) if t == b"vertex"]
    if not at or len(at) % 3 or at[-1] + 3 >= len(tokens):
        raise ValueError(f"ASCII STL file '{path}' is truncated: {len(at)} complete 'vertex' entries found.")
    try:
        xyz = np.array([[float(tokens[i + 1]), float(tokens[i + 2]), float(tokens[i + 3])] for i in at])
    except ValueError:
        raise ValueError(f"ASCII STL file '{path}' holds a vertex that is not three numbers.") from None
    return _checked(xyz.astype(np.float32).astype(np.float64).reshape(-1, 3, 3), path)


def _checked(tri: np.ndarray, path: str) -> np.ndarray:
    if not np.isfinite(tri).all():
        raise ValueError(f"STL file '{path}' holds non-finite vertex coordinates.")
    return tri


def close_check(tri: np.ndarray, path: str) -> np.ndarray:
    """weld vertices by exact coordinate equality, drop zero-area facets, require every undirected edge to be used by exactly
    two facets -> the facets with their vertices in lexicographic order ``[nt, 3, 3]``"""
    points, ids = np.unique(tri.reshape(-1, 3) + 0.0, axis=0, return_inverse=True)        # + 0.0: -0.0 and 0.0 are one point
    ids = np.sort(ids.reshape(-1, 3), axis=1)              # unique() sorts lexicographically: id order = (x, y, z) order
    facets = points[ids]
    normal = np.cross(facets[:, 1] - facets[:, 0], facets[:, 2] - facets[:, 0])
    keep = (ids[:, 0] != ids[:, 1]) & (ids[:, 1] != ids[:, 2]) & (normal != 0.0).any(1)
    ids, facets = ids[keep], facets[keep]
    edges = np.concatenate([ids[:, [0, 1]], ids[:, [0, 2]], ids[:, [1, 2]]])
    used = np.unique(edges, axis=0, return_counts=True)[1] if len(edges) else np.zeros(0, dtype=np.int64)
    bad = int(np.count_nonzero(used != 2))
    if bad or not len(ids):
        raise ValueError(f"STL file '{path}' is not a closed manifold surface: {bad} of {len(used)} edges are not shared by "
                         f"exactly two facets ({len(ids)} facets of non-zero area).  No repair is attempted here; close the "
                         f"surface before handing it over.")
    return np.ascontiguousarray(facets)


# -- column bins -----------------------------------------------------------------------------------------------------
def bin_scale(lo: float, hi: float, nb: int) -> float:
    """columns per unit length (0 for a flat extent: everything is in column 0)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.float64(nb) / (np.float64(hi) - np.float64(lo))
    return float(scale) if np.isfinite(scale) else 0.0


def bin_index(v, lo: float, scale: float, nb: int):
    """column of coordinate ``v`` -- monotone in ``v``, the kernel evaluates the same expression"""
    return np.clip(np.floor((np.asarray(v, dtype=np.float64) - lo) * scale), 0, nb - 1).astype(np.int64)


def build_column_bins(tri: np.ndarray, lo, hi, ny: int = None, nz: int = None):
    """CSR table ``(ny, nz, bin_start[ny*nz+1] int32, bin_facet[] int32)`` over the (y, z) bounding box: column ``iy*nz+iz``
    lists (ascending) every facet whose closed projected bounding box touches it.  Without ``ny`` / ``nz`` the grid is chosen
    from the facet count (about two facets per column, columns about square) and coarsened while the lists hold more than
    8 entries per facet."""
    nt = int(tri.shape[0])
    if ny is None or nz is None:
        ey, ez = float(hi[1] - lo[1]), float(hi[2] - lo[2])
        want = min(max(nt // 2, 1), MAX_BINS)
        aspect = ey / ez if ey > 0 and ez > 0 else 1.0
        ny = int(min(max(round(np.sqrt(want * aspect)), 1), want))
        nz = int(max(want // ny, 1))
    while True:
        sy, sz = bin_scale(lo[1], hi[1], ny), bin_scale(lo[2], hi[2], nz)
        y0, y1 = bin_index(tri[:, :, 1].min(1), lo[1], sy, ny), bin_index(tri[:, :, 1].max(1), lo[1], sy, ny)
        z0, z1 = bin_index(tri[:, :, 2].min(1), lo[2], sz, nz), bin_index(tri[:, :, 2].max(1), lo[2], sz, nz)
        span_z = z1 - z0 + 1
        per_facet = (y1 - y0 + 1) * span_z
        if int(per_facet.sum()) <= 8 * nt + 64 or ny * nz == 1:
            break
        ny, nz = max(ny // 2, 1), max(nz // 2, 1)
    facet = np.repeat(np.arange(nt, dtype=np.int64), per_facet)
    k = np.arange(len(facet), dtype=np.int64) - np.repeat(np.cumsum(per_facet) - per_facet, per_facet)
    column = (y0[facet] + k // span_z[facet]) * nz + z0[facet] + k % span_z[facet]
    order = np.argsort(column, kind="stable")
    bin_start = np.zeros(ny * nz + 1, dtype=np.int64)
    np.cumsum(np.bincount(column, minlength=ny * nz), out=bin_start[1:])
    return ny, nz, bin_start.astype(np.int32), facet[order].astype(np.int32)


# -- predicate (host) ------------------------------------------------------------------------------------------------
def _edge_hit(py, pz, p_y, p_z, q_y, q_z):
    straddle = (p_z > pz) != (q_z > pz)
    with np.errstate(divide="ignore", invalid="ignore"):
        y_int = p_y + (pz - p_z) * (q_y - p_y) / (q_z - p_z)
    return straddle & (py < y_int)


def _closed_triangle(pu, pv, au, av, bu, bv, cu, cv):
    s0 = (bu - au) * (pv - av) - (bv - av) * (pu - au)
    s1 = (cu - bu) * (pv - bv) - (cv - bv) * (pu - bu)
    s2 = (au - cu) * (pv - cv) - (av - cv) * (pu - cu)
    return ~(((s0 < 0) | (s1 < 0) | (s2 < 0)) & ((s0 > 0) | (s1 > 0) | (s2 > 0)))


def inside_mesh(tri: np.ndarray, lo, hi, points: np.ndarray) -> np.ndarray:
    """the predicate of the module docstring for ``points [m, 3]`` float64 against all facets ``tri [nt, 3, 3]`` (no bins:
    this is the brute-force statement of the rule; the operations and their order are those of ``s3_mask_mesh``)"""
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    result = np.zeros(len(points), dtype=bool)
    in_box = ((points >= np.asarray(lo)) & (points <= np.asarray(hi))).all(1)
    todo = np.flatnonzero(in_box)
    (ax, ay, az), (bx, by, bz), (cx, cy, cz) = (tri[None, :, v, :].transpose(2, 0, 1) for v in range(3))
    e1x, e1y, e1z, e2x, e2y, e2z = bx - ax, by - ay, bz - az, cx - ax, cy - ay, cz - az
    nx, ny, nz = e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x
    y_min, y_max = np.minimum(np.minimum(ay, by), cy), np.maximum(np.maximum(ay, by), cy)
    z_min, z_max = np.minimum(np.minimum(az, bz), cz), np.maximum(np.maximum(az, bz), cz)
    drop_x = (np.abs(nx) >= np.abs(ny)) & (np.abs(nx) >= np.abs(nz))
    drop_y = ~drop_x & (np.abs(ny) >= np.abs(nz))
    step = max(_HOST_BLOCK // max(tri.shape[0], 1), 1)
    for s in range(0, len(todo), step):
        rows = todo[s:s + step]
        px, py, pz = points[rows, 0, None], points[rows, 1, None], points[rows, 2, None]
        box = (py >= y_min) & (py <= y_max) & (pz >= z_min) & (pz <= z_max)
        vol = (nx * (px - ax) + ny * (py - ay)) + nz * (pz - az)
        flat = box & (vol == 0.0)
        on = np.zeros(len(rows), dtype=bool)
        if flat.any():
            on = (flat & np.where(drop_x, _closed_triangle(py, pz, ay, az, by, bz, cy, cz),
                                  np.where(drop_y, _closed_triangle(pz, px, az, ax, bz, bx, cz, cx),
                                           _closed_triangle(px, py, ax, ay, bx, by, cx, cy)))).any(1)
        odd = _edge_hit(py, pz, ay, az, by, bz) ^ _edge_hit(py, pz, ay, az, cy, cz) ^ _edge_hit(py, pz, by, bz, cy, cz)
        crossed = box & (vol != 0.0) & (nx != 0.0) & ((vol < 0.0) != (nx < 0.0)) & odd
        result[rows] = on | (np.count_nonzero(crossed, axis=1) % 2 == 1)
    return result


class GeometrySTL3D(GeometryObject):
    __short_description__ = "usage of STL files for geometries (3D)"

    def __init__(self, name: str, keep_inside: bool, path_stl_file: str, refine: bool = False,
                 min_refinement_level: int = None, reduce_by: Union[int, float] = 0):
        if reduce_by < 0:
            logger.warning(f"Found invalid negative value for 'reduce_by' of {reduce_by}. Disabling compression.")
            reduce_by = 0
        elif reduce_by >= 1:
            logger.warning(f"Found invalid value for 'reduce_by' of {reduce_by}. Compression factor needs to be "
                           f"0 <= reduce_by < 1. Correcting 'reduce_by' to reduce_by=0.99")
            reduce_by = 0.99
        super().__init__(name, keep_inside, refine, min_refinement_level)
        self._type = "STL"
        self._pwd = path_stl_file
        if reduce_by > 0:
            logger.warning(f"Geometry {name}: reduce_by={reduce_by} is ignored, the full surface is used (decimation only "
                           f"ever served to cut the cost of the per-cell query, which runs on the device here).")
        self._stl_file = read_stl(path_stl_file)
        self._check_geometry()
        self._lower_bound = [float(v) for v in self._stl_file.min((0, 1))]
        self._upper_bound = [float(v) for v in self._stl_file.max((0, 1))]
        self._bins = build_column_bins(self._stl_file, self._lower_bound, self._upper_bound)
        self._main_width = self._compute_main_width()
        self._center = self._compute_center()

    def inside(self, points) -> np.ndarray:
        """per-point verdict of the host predicate for ``points [m, 3]``"""
        return inside_mesh(self._stl_file, self._lower_bound, self._upper_bound, points)

    def check_cell(self, cell_nodes: Tensor, refine_geometry: bool = False) -> bool:
        mask = from_numpy(self.inside(cell_nodes.detach().cpu().double().numpy()))
        return self._apply_mask(mask, refine_geometry)

    def pre_check_cell(self, cell_nodes: Tensor, refine_geometry: bool = False) -> bool:
        return self._apply_mask(mask_box(cell_nodes, self._lower_bound, self._upper_bound), refine_geometry)

    def kernel_spec(self) -> tuple:
        """``("mesh", tri[nt,3,3], lo[3], hi[3], ny, nz, bin_start[ny*nz+1], bin_facet[])``"""
        return ("mesh", self._stl_file, np.array(self._lower_bound), np.array(self._upper_bound)) + tuple(self._bins)

    def _check_geometry(self) -> None:
        self._stl_file = close_check(self._stl_file, self._pwd)

    type = property(lambda self: self._type)
    main_width = property(lambda self: self._main_width)
    center = property(lambda self: self._center)

    def _compute_main_width(self) -> float:
        return max([abs(u - l) for l, u in zip(self._lower_bound, self._upper_bound)])

    def _compute_center(self) -> Tensor:
        return (tensor(self._lower_bound) + tensor(self._upper_bound)) / 2.0
