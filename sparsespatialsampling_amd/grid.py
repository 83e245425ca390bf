"""
One generated grid on the device, described once for everything that looks things up in it: ``sampling.Probe`` (fields at points),
``isosurface.Isosurface`` (cuts of node fields), ``tracing.Tracer`` (particles through node velocities) and ``regions.Regions``
(connected regions of cell fields) all rest on a ``Grid``.

A grid has two parts, and either may be absent:

    the cell part       ``centers`` [Nc, d], ``levels`` [Nc] or [Nc, 1] and ``width`` (the size of the initial cell): the disjoint dyadic
                        boxes points are located in (``index``: the ``hipops.CellIndex``, built on first use and kept;
                        ``neighbours``: which leaf lies across each face, built on first use and kept)
    the corner part     ``nodes`` [Nn, d] and ``faces`` [Nc, 2^d], the corner nodes of every cell: what node fields are blended and
                        cut through; its cells need not be dyadic boxes when the cell part is absent

    grid = Grid.from_dataloader(loader)
    tracer, iso = Tracer.from_grid(grid), Isosurface.from_grid(grid)        # one upload, one index
    probe = Probe.from_grid(grid, raster(lo, hi, (ny, nx)))
"""
import numpy as np
import torch as pt

from . import hipops
from .arrays import as_tensor


class Grid:
    """``centers``, ``levels``, ``width``, ``nodes``, ``faces`` as above, numpy or torch, host or device; arrays that lie on the device
    in the kernels' types (float64, int32) are kept, not copied.  Shapes, dtypes and the range of the face ids are checked before
    anything is uploaded: a malformed grid is a ``ValueError``.  Attributes: ``dim``, ``n_cells``, ``n_nodes`` (None without the corner
    part), the five device arrays (None where a part is absent, ``levels`` int32 [Nc]), ``index`` and ``neighbours``."""

    def __init__(self, centers=None, levels=None, width=None, nodes=None, faces=None):
        cell_part = [v is not None for v in (centers, levels, width)]
        if any(cell_part) != all(cell_part):
            raise ValueError("centers, levels and width go together")
        if (nodes is None) != (faces is None):
            raise ValueError("nodes and faces go together")
        if not (cell_part[0] or nodes is not None):
            raise ValueError("a grid is its cells (centers, levels, width), its corners (nodes and faces) or both")
        self.dim = self.n_cells = self.n_nodes = None
        if cell_part[0]:
            centers, levels = as_tensor(centers, "centers"), as_tensor(levels, "levels")
            if centers.dim() != 2 or int(centers.shape[1]) not in (2, 3):
                raise ValueError(f"expected centers [Nc, 2 | 3], got {tuple(centers.shape)}")
            self.n_cells, self.dim = int(centers.shape[0]), int(centers.shape[1])
            if levels.numel() != self.n_cells or levels.is_floating_point():
                raise ValueError(f"expected one integer level per cell ({self.n_cells}), got {tuple(levels.shape)} {levels.dtype}")
        if nodes is not None:
            nodes, faces = as_tensor(nodes, "nodes"), as_tensor(faces, "faces")
            if nodes.dim() != 2 or int(nodes.shape[1]) not in ((2, 3) if self.dim is None else (self.dim,)):
                raise ValueError(f"expected nodes [Nn, {'2 | 3' if self.dim is None else self.dim}], got {tuple(nodes.shape)}")
            self.n_nodes, self.dim = int(nodes.shape[0]), int(nodes.shape[1])
            if self.n_cells is None and faces.dim() == 2:
                self.n_cells = int(faces.shape[0])
            if tuple(faces.shape) != (self.n_cells, 1 << self.dim) or faces.is_floating_point():
                raise ValueError(f"expected integer faces [{'Nc' if self.n_cells is None else self.n_cells}, {1 << self.dim}], "
                                 f"got {tuple(faces.shape)} {faces.dtype}")
            if self.n_nodes < 1:
                raise ValueError("a grid without nodes")
            if self.n_cells and (int(faces.min()) < 0 or int(faces.max()) >= self.n_nodes):
                raise ValueError(f"faces name nodes outside [0, {self.n_nodes})")
        self.width = None if width is None else float(width)
        self.centers = self.levels = self.nodes = self.faces = self._index = self._neighbours = None
        if cell_part[0]:
            self.centers, self.levels = hipops.to_device(centers, pt.float64), hipops.to_device(levels.reshape(-1), pt.int32)
        if nodes is not None:
            self.nodes, self.faces = hipops.to_device(nodes, pt.float64), hipops.to_device(faces, pt.int32)

    @classmethod
    def from_dataloader(cls, loader):
        """the grid of an S^3 file (``data.Dataloader``, whose ``vertices`` are the cell centres and whose ``nodes`` the corners)"""
        return cls(loader.vertices, loader.levels, loader.size_initial_cell, loader.nodes, loader.faces)

    @classmethod
    def from_s_cube(cls, s_cube):
        """the grid of a ``SparseSpatialSampling`` after ``execute_grid_generation`` (its ``vertices`` are the corners)"""
        if getattr(s_cube, "centers", None) is None:
            raise ValueError("the grid has not been generated yet: call execute_grid_generation() first")
        return cls(s_cube.centers, s_cube.levels, float(s_cube.size_initial_cell), s_cube.vertices, s_cube.faces)

    @property
    def index(self):
        """the ``hipops.CellIndex`` of the cell part; a grid whose cells are no disjoint dyadic boxes on one lattice is refused with
        ``ValueError`` (``hipops.cell_index``)"""
        if self._index is None:
            if self.centers is None:
                raise ValueError("points are located in the cells of a grid: build the Grid with centers, levels and width")
            self._index = hipops.cell_index(self.centers, self.levels, self.width)
        return self._index

    @property
    def bounds(self):
        """``(lo, hi)``, float64 [d] each on the host: the lattice domain of the index, ``origin`` and ``origin + 2^depth * h_min``, the
        cube every leaf lies in (it may reach past the cells where the grid is no full cube)"""
        ix = self.index
        lo = np.array(ix.origin[:self.dim], dtype=np.float64)
        return lo, lo + float(1 << ix.depth) * ix.h_min

    @property
    def neighbours(self):
        """the face neighbours of the cell part (``hipops.cell_neighbours``): int32 [Nc, 2 d] on the device, face ``2 * axis + side``
        holds the same-or-coarser leaf across it or -1 (the domain edge, a body or a hole, finer cells): every pair of cells that
        share a face stands in it once from the finer side, and from both sides at equal level"""
        if self._neighbours is None:
            self._neighbours = hipops.cell_neighbours(self.index)
        return self._neighbours
