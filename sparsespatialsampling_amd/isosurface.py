"""
Isosurfaces (3-D) and contour lines (2-D) of fields on the grid NODES (``interpolate_at_vertices=True`` exports, ``Gradient`` on the
node cloud, POD / DMD / SPOD modes [N_nodes, r]), extracted on the GPU for a whole batch of snapshots (csrc/iso.hip).  The reference
has nothing of the kind: its post-processing writes files for a viewer, one snapshot at a time.

Marching simplices on the leaves: every leaf is cut into d! simplices (Kuhn), every simplex emits 0, 1 or 2 triangles (segments in
2-D); include/s3hip.h states the definition.  A vertex lies on a grid edge between the nodes a < b and is computed from a and b alone,
so the same edge gives the same bits in every cell that shares it: ``IsoResult.weld`` joins the triangle soup by the key (a, b),
exactly and without a tolerance.  Across a level jump of the grid the surface may crack at hanging nodes; where cells are missing
(inside a body) it simply ends.

    iso = Isosurface.from_dataloader(loader)
    res = iso.extract(q_on_nodes[:, t0:t1], level=0.5)         # the window is read where it lies
    colour = res.interpolate(velocity_magnitude_on_nodes[:, t0:t1])
    res.write_stl("q.stl", 0)
"""
import numpy as np
import torch as pt

from . import hipops
from .arrays import Side, as_tensor, resident
from .grid import Grid


class IsoResult:
    """The primitives of ``T`` snapshots, ordered by (snapshot, cell, simplex, primitive): ``offsets`` int64 numpy [T + 1] (snapshot
    t owns [offsets[t], offsets[t + 1])), ``vertices`` f64 [n, d, d], ``edges`` int32 [n, d, 2] (the nodes a < b of the grid edge a
    vertex lies on), ``frac`` f64 [n, d] (its position between a and b), ``cells`` int32 [n] -- on the side (and as the kind of
    array) the field came from."""

    def __init__(self, offsets, vertices, edges, frac, cells, n_nodes):
        self.offsets, self.vertices, self.edges, self.frac, self.cells = offsets, vertices, edges, frac, cells
        self.n_snapshots, self.dim, self.n_nodes = len(offsets) - 1, int(vertices.shape[1]), n_nodes

    def __len__(self):
        return int(self.offsets[-1])

    def _range(self, t):
        t = int(t)
        if not 0 <= t < self.n_snapshots:
            raise IndexError(f"snapshot {t} outside [0, {self.n_snapshots})")
        return int(self.offsets[t]), int(self.offsets[t + 1])

    def snapshot(self, t):
        """views (vertices, edges, frac, cells) of snapshot ``t``"""
        lo, hi = self._range(t)
        return self.vertices[lo:hi], self.edges[lo:hi], self.frac[lo:hi], self.cells[lo:hi]

    def interpolate(self, other):
        """another node field at the vertices: ``g_a + frac (g_b - g_a)`` -> f64 [n, d].  ``other`` is [N_nodes] (one field for
        every snapshot) or [N_nodes, T] (column t for the primitives of snapshot t).  Plain torch, not a hot path."""
        as_numpy = isinstance(self.vertices, np.ndarray)
        g = as_tensor(other, "other")
        if g.dim() not in (1, 2) or int(g.shape[0]) != self.n_nodes or (g.dim() == 2 and int(g.shape[1]) != self.n_snapshots):
            raise ValueError(f"expected a node field [{self.n_nodes}] or [{self.n_nodes}, {self.n_snapshots}], got {tuple(g.shape)}")
        edges, frac = as_tensor(self.edges, "edges"), as_tensor(self.frac, "frac")
        g = g.to(frac.device, pt.float64)
        a, b = edges[..., 0].long(), edges[..., 1].long()
        if g.dim() == 2:
            counts = pt.from_numpy(np.diff(self.offsets)).to(frac.device)
            col = pt.repeat_interleave(pt.arange(self.n_snapshots, device=frac.device), counts)[:, None].expand_as(a)
            ga, gb = g[a, col], g[b, col]
        else:
            ga, gb = g[a], g[b]
        out = ga + frac * (gb - ga)
        return out.numpy() if as_numpy else out

    def weld(self, t):
        """(points f64 [n_points, d], index int64 [n, d]) of snapshot ``t``: vertices with the same edge key ``(a << 32) | b`` are one
        point (they have the same bits), ``points[index]`` is the soup again.  Exact, no tolerance."""
        verts, edges, _, _ = self.snapshot(t)
        as_numpy = isinstance(verts, np.ndarray)
        verts, edges = as_tensor(verts, "vertices"), as_tensor(edges, "edges").long()
        d = self.dim
        key = ((edges[..., 0] << 32) | edges[..., 1]).reshape(-1)
        uniq, inverse = pt.unique(key, return_inverse=True)
        points = pt.empty((int(uniq.numel()), d), dtype=verts.dtype, device=verts.device)
        points[inverse] = verts.reshape(-1, d)
        index = inverse.reshape(-1, d)
        return (points.numpy(), index.numpy()) if as_numpy else (points, index)

    def write_stl(self, path, t):
        """the triangles of snapshot ``t`` as binary STL (coordinates rounded to float32, normals from the rounded vertices; 3-D only);
        ``geometry.geometry_STL_3d.read_stl`` reads it back"""
        if self.dim != 3:
            raise ValueError("STL holds triangles: 3-D only")
        tri = as_tensor(self.snapshot(t)[0], "vertices").cpu().numpy().astype("<f4")
        if not len(tri):
            raise ValueError(f"snapshot {int(t)} has no triangles")
        wide = tri.astype(np.float64)
        normal = np.cross(wide[:, 1] - wide[:, 0], wide[:, 2] - wide[:, 0])
        length = np.linalg.norm(normal, axis=1, keepdims=True)
        rec = np.zeros(len(tri), dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]))
        rec["n"], rec["v"] = np.divide(normal, length, out=np.zeros_like(normal), where=length > 0), tri
        with open(path, "wb") as f:
            f.write(b"isosurface".ljust(80, b" "))
            f.write(np.array([len(tri)], dtype="<u4").tobytes())
            f.write(rec.tobytes())


class Isosurface:
    """``nodes`` [N_nodes, d] and ``faces`` [N_cells, 2^d] (the corner nodes of every cell) of a generated grid, d = 2 | 3; numpy or
    torch, host or device: the corner part of a ``grid.Grid``, kept as ``grid``; ``from_grid`` takes one that is there already.
    ``extract`` and ``count`` take node fields [N_nodes] or [N_nodes, T], float32 or float64, numpy or torch,
    host or device; a window ``field[:, t0:t1]`` of a field that lives on the device is read where it lies (``arrays.resident``).
    Results come back on the side (and as the kind of array) the field came from."""

    def __init__(self, nodes, faces):
        self._on(Grid(nodes=nodes, faces=faces))

    def _on(self, grid):
        if grid.faces is None:
            raise ValueError("an isosurface cuts fields on the grid's nodes: build the Grid with nodes and faces")
        self.grid, self.dim, self.n_cells, self.n_nodes = grid, grid.dim, grid.n_cells, grid.n_nodes
        self._nodes, self._faces = grid.nodes, grid.faces

    @classmethod
    def from_grid(cls, grid):
        """a ``grid.Grid`` with its corner part (the cell part is not needed), which is not uploaded again"""
        self = cls.__new__(cls)
        self._on(grid)
        return self

    @classmethod
    def from_dataloader(cls, loader):
        """the grid of an S^3 file (``data.Dataloader``)"""
        return cls.from_grid(Grid.from_dataloader(loader))

    @classmethod
    def from_s_cube(cls, s_cube):
        """the grid of a ``SparseSpatialSampling`` after ``execute_grid_generation``"""
        return cls.from_grid(Grid.from_s_cube(s_cube))

    def _field(self, field, level):
        field, side = as_tensor(field, "field"), Side(field)
        shape = tuple(int(v) for v in field.shape)
        if not 1 <= len(shape) <= 2 or shape[0] != self.n_nodes:
            raise ValueError(f"expected a field [{self.n_nodes}] or [{self.n_nodes}, T] on the grid's nodes, got {shape}")
        if 0 in shape:
            raise ValueError(f"empty field {shape}")
        level = float(level)
        if not np.isfinite(level):
            raise ValueError(f"the level must be finite, got {level!r}")
        return resident(field), level, side

    def count(self, field, level, _count_bytes=hipops.ISO_COUNT_BYTES):
        """the number of primitives of every snapshot (the first pass alone) -> int64 numpy [T]"""
        dev_field, level, _ = self._field(field, level)
        (offsets,) = hipops.iso_extract(dev_field, self._faces, self._nodes, level, count_only=True, count_bytes=_count_bytes)
        return np.diff(offsets)

    def extract(self, field, level, _count_bytes=hipops.ISO_COUNT_BYTES):
        """-> ``IsoResult``: the triangles (segments) of ``field == level`` for every snapshot, oriented so that the right-hand normal
        points to ``field < level`` (2-D: ``field >= level`` lies to the left of a segment)"""
        dev_field, level, side = self._field(field, level)
        offsets, *arrays = hipops.iso_extract(dev_field, self._faces, self._nodes, level, count_bytes=_count_bytes)
        return IsoResult(offsets, *(side.back(a) for a in arrays), n_nodes=self.n_nodes)
