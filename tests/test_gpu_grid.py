"""
``grid.Grid`` on the GPU: one grid is uploaded and indexed once for every front-end that rests on it, the front-ends give the same
bits through ``from_grid`` as through their own constructors, either part of a grid may be absent, and the C entry points refuse a
malformed ``s3_grid`` by name before anything is launched.

Shapes: the grids tree2d and tree3d of tests/sample_cases.py (a few thousand cells) with their 3001 queries, 500 seeds, 3 snapshots;
``iso_cases.every_mask(3, 256)`` for the corner part alone (its three cells are no dyadic boxes).
"""
import ctypes as C

import numpy as np
import pytest
import torch as pt

from tests import iso_cases as ic
from tests import sample_cases as sc
from sparsespatialsampling_amd import _lib, hipops
from sparsespatialsampling_amd.grid import Grid
from sparsespatialsampling_amd.isosurface import Isosurface
from sparsespatialsampling_amd.sampling import Probe
from sparsespatialsampling_amd.tracing import Tracer

pytestmark = pytest.mark.gpu

GRID_KEYS = ("centers", "levels", "width", "nodes", "faces")
N_SEEDS, T = 500, 3


def dev(a):
    return pt.from_numpy(np.ascontiguousarray(a)).cuda()


def grid_arrays(name, on_device):
    c = sc.case(name)
    return {k: dev(c[k]) if on_device and k != "width" else c[k] for k in GRID_KEYS}


def fields(name):
    """(cell field [Nc, T], node field [Nn, 2, T], node velocity [Nn, d, T] f32, seeds [N_SEEDS, d]) of a case, random"""
    c = sc.case(name)
    d = c["centers"].shape[1]
    rng = np.random.default_rng(31 + d)
    lo, hi = c["nodes"].min(axis=0), c["nodes"].max(axis=0)
    return (rng.standard_normal((len(c["levels"]), T)), rng.standard_normal((len(c["nodes"]), 2, T)),
            rng.standard_normal((len(c["nodes"]), d, T)).astype(np.float32), lo + (hi - lo) * rng.random((N_SEEDS, d)))


def bits(x):
    x = x.cpu().numpy() if isinstance(x, pt.Tensor) else np.asarray(x)
    return x.view(np.int64) if x.dtype == np.float64 else x


def same(a, b):
    return type(a) is type(b) and np.array_equal(bits(a), bits(b))


def counting(monkeypatch):
    calls = []
    real = hipops.cell_index

    def counted(*args, **kw):
        calls.append(1)
        return real(*args, **kw)
    monkeypatch.setattr(hipops, "cell_index", counted)
    return calls


# ---- one index -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tree2d", "tree3d"])
def test_one_grid_is_indexed_once(name, monkeypatch):
    c = sc.case(name)
    _, node_field, velocity, seeds = fields(name)
    calls = counting(monkeypatch)
    grid = Grid(**grid_arrays(name, False))
    assert not calls                                                            # built on first use
    tracer = Tracer.from_grid(grid)
    probes = [Probe.from_grid(grid, c["queries"]), Probe.from_grid(grid, c["queries"][::-1].copy())]
    paths = tracer.streamlines(velocity, seeds, 6)
    colours = [paths.sample(node_field), paths.sample(node_field[:, :1].copy())]
    assert len(calls) == 1 and tracer.grid is grid and all(p.grid is grid for p in probes) and grid.index is probes[1]._index
    assert colours[0].shape == (N_SEEDS, T, 7, 2, T) and same(colours[0][..., :1, :], colours[1])
    assert same(probes[0].cell_ids, probes[1].cell_ids[::-1].copy())
    # the old constructor: the tracer's grid serves every colouring
    del calls[:]
    old = Tracer(*(c[k] for k in GRID_KEYS))
    paths = old.streamlines(velocity, seeds, 6)
    again = [paths.sample(node_field), paths.sample(node_field[:, :1].copy())]
    assert len(calls) == 1 and all(same(a, b) for a, b in zip(again, colours))


# ---- the same bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("name", ["tree2d", "tree3d"])
def test_from_grid_gives_the_bits_of_the_constructors(name, on_device):
    c = sc.case(name)
    a = grid_arrays(name, on_device)
    place = dev if on_device else (lambda x: x)
    cell_field, node_field, velocity, seeds = (place(x) for x in fields(name))
    queries = place(c["queries"])
    grid = Grid(**a)
    if on_device:                                                               # kept, not copied
        assert all(getattr(grid, k).data_ptr() == a[k].data_ptr() for k in ("centers", "levels", "nodes", "faces"))
    assert (grid.dim, grid.n_cells, grid.n_nodes, grid.width) == (c["centers"].shape[1], len(c["levels"]), len(c["nodes"]), c["width"])

    new, old = Probe.from_grid(grid, queries), Probe(a["centers"], a["levels"], a["width"], queries, nodes=a["nodes"], faces=a["faces"])
    assert same(new.cell_ids, old.cell_ids) and same(new.inside, old.inside) and np.array_equal(bits(new.cell_ids), sc.truth(name)[0])
    assert same(new.sample(cell_field), old.sample(cell_field))
    linear = new.sample(node_field, mode="linear")
    assert same(linear, old.sample(node_field, mode="linear")) and np.isfinite(bits(linear).view(np.float64)).any()

    new, old = Tracer.from_grid(grid), Tracer(*(a[k] for k in GRID_KEYS))
    dt_snapshot = 0.05 * c["width"]
    for run in (lambda t: t.streamlines(velocity, seeds, 6, direction="both"), lambda t: t.pathlines(velocity, seeds, dt_snapshot)):
        got, want = run(new), run(old)
        assert all(same(getattr(got, k), getattr(want, k)) for k in ("points", "first", "length", "status", "cell_ids"))
        assert (bits(got.length) > 1).any()

    field = place(ic.smooth_field(name, T))
    got, want = Isosurface.from_grid(grid).extract(field, ic.SMOOTH_LEVEL), Isosurface(a["nodes"], a["faces"]).extract(field, ic.SMOOTH_LEVEL)
    assert np.array_equal(got.offsets, want.offsets) and (np.diff(got.offsets) > 0).all()
    assert all(same(getattr(got, k), getattr(want, k)) for k in ("vertices", "edges", "frac", "cells"))


# ---- either part alone ------------------------------------------------------------------------------------------------------------
def test_corner_part_alone_and_cell_part_alone():
    nodes, faces, field, level = ic.every_mask(3, 256)
    corners = Grid(nodes=nodes, faces=faces)
    assert (corners.dim, corners.n_cells, corners.n_nodes, corners.centers, corners.width) == (3, 3, 24, None, None)
    res = Isosurface.from_grid(corners).extract(field, level)
    got = {"offsets": res.offsets, "verts": res.vertices, "edges": res.edges, "frac": res.frac, "cells": res.cells}
    ic.check(got, ic.extract(nodes, faces, field, level), "the corner part alone")
    with pytest.raises(ValueError, match="centers, levels and width"):
        Probe.from_grid(corners, nodes)
    with pytest.raises(ValueError, match="centers, levels and width"):
        Tracer.from_grid(corners)

    c = sc.case("tree2d")
    cells = Grid(c["centers"], c["levels"], c["width"])
    probe = Probe.from_grid(cells, c["queries"])
    assert np.array_equal(probe.cell_ids, sc.truth("tree2d")[0])
    with pytest.raises(ValueError, match="build the Probe with nodes and faces"):
        probe.sample(np.zeros((len(c["nodes"]), 2)), "linear")
    with pytest.raises(ValueError, match="nodes and faces"):
        Tracer.from_grid(cells)
    with pytest.raises(ValueError, match="nodes and faces"):
        Isosurface.from_grid(cells)


# ---- the C entry points refuse a malformed s3_grid by name ------------------------------------------------------------------------
def test_entry_points_refuse_a_malformed_grid():
    c = sc.case("tree2d")
    index = hipops.cell_index(dev(c["centers"]), dev(c["levels"]), c["width"])
    faces, points = dev(c["faces"]), dev(c["queries"])
    nq, n_nodes = len(c["queries"]), len(c["nodes"])
    ids = hipops.cell_locate(index, points)
    field = pt.zeros((n_nodes, 2, 1), dtype=pt.float64, device="cuda")
    lib, stream, ptr = _lib.hip_lib(), hipops._stream(), hipops._ptr
    mark = 1234567
    out_i = [pt.full((nq,), mark, dtype=pt.int32, device="cuda") for _ in range(4)]
    out_f = pt.full((nq, 2), float(mark), dtype=pt.float64, device="cuda")

    def refused(rc, who):
        message = lib.s3_last_error().decode()
        assert rc == -1 and message.startswith(who + ":"), (rc, message)        # S3_EINVAL
        pt.cuda.synchronize()
        assert all((o == mark).all() for o in out_i) and (out_f == mark).all(), f"{who} wrote to an output"

    refused(lib.s3_cell_locate(None, ptr(points), nq, None, ptr(out_i[0]), stream), "s3_cell_locate")
    no_faces = index.s3_grid()
    assert not no_faces.d_faces
    refused(lib.s3_trace(0, C.byref(no_faces), ptr(field), 1, 1, 2, n_nodes, ptr(points), nq, None, 3, 1, 1, 1, 0.5, 1, ptr(out_f),
                         ptr(out_i[0]), ptr(out_i[1]), ptr(out_i[2]), stream), "s3_trace")
    four = index.s3_grid(faces)
    four.dim = 4
    refused(lib.s3_cell_sample(1, ptr(ids), nq, None, ptr(field), 1, 2, 1, 2, n_nodes, C.byref(four), ptr(points), ptr(out_f), 2, stream),
            "s3_cell_sample")
    # the same calls with the grid as it should be go through
    good = index.s3_grid(faces)
    assert lib.s3_cell_locate(C.byref(good), ptr(points), nq, None, ptr(out_i[3]), stream) == 0
    assert lib.s3_cell_sample(1, ptr(ids), nq, None, ptr(field), 1, 2, 1, 2, n_nodes, C.byref(good), ptr(points), ptr(out_f), 2, stream) == 0
    pt.cuda.synchronize()
    assert pt.equal(out_i[3], ids) and not (out_f == mark).any()
