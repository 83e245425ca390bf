"""``mask_kernel`` on the MI355X at the ties of curved bodies and in the launch shapes ``refine()`` uses.  Sphere, cylinder, cone and
box against the real reference's verdicts (tests/golden/masks_curved.npz): one launch per body and mode pair over all cells of the
mixed-level lattice.  Cell lists, ranges with ``first > 0``, partial blocks, accumulation into ``invalid`` and canaries for every
mask kernel; polygon, triangle, prism, tetrahedra and mesh against their own one-cell launches, which the goldens judge.  GPU only."""
import os

import numpy as np
import pytest
import torch as pt

pytestmark = pytest.mark.gpu

from inputs import POLYTOPES, polytope                                                      # noqa: E402
from tests import masks_curved_cases as K                                                  # noqa: E402
from tests.oracle_backend import orc                                                       # noqa: E402

CANARY = 0xA5


@pytest.fixture(scope="module")
def ops():
    from sparsespatialsampling_amd import hipops
    hipops.device()
    return hipops


@pytest.fixture(scope="module")
def lattice(ops):
    """the fixture's cells on the device, per dimension: (centre, level, width, number of cells)"""
    out = {}
    for d in (2, 3):
        center, level, width = K.cells(d)
        out[d] = (ops.to_device(center), ops.to_device(level), width, len(center))
    return out


def launcher(ops, body):
    """(function, arguments between the cells and the mode pair) of the kernel that masks ``body``"""
    if body.kind == "sphere":
        return ops.mask_sphere, body.args
    if body.kind == "box":
        return ops.mask_box, body.args
    return ops.mask_cylinder, orc.cylinder_params(*body.args)


def launch(lattice, dim, fn, args, ki, rm, cells=None, first=0, n=None, invalid=None, pad=0):
    """one launch; returns the ``n`` verdict bytes and the ``pad`` canary bytes behind them"""
    from sparsespatialsampling_amd.hipops import MaskCells
    center, level, width, total = lattice[dim]
    d_cells = None
    if cells is not None:
        n, d_cells = len(cells), pt.from_numpy(np.ascontiguousarray(cells, dtype=np.int32)).cuda()
    n = total - first if n is None else n
    buf = pt.zeros(n + pad, dtype=pt.uint8, device="cuda") if invalid is None else pt.from_numpy(invalid.copy()).cuda()
    if pad:
        buf[n:] = CANARY
    fn(MaskCells(center, level, width, buf, d_cells, first, n), *args, rm, ki)
    out = buf.cpu().numpy()
    return out[:n], out[n:]


@pytest.mark.parametrize("kind,dim", [("sphere", 2), ("sphere", 3), ("cylinder", 3), ("box", 2), ("box", 3)])
def test_every_body_equals_the_reference(ops, lattice, kind, dim):
    """exact equality with the reference's verdicts, all cells with their real levels in one launch"""
    some = [b for b in K.bodies() if b.kind == kind and b.dim == dim]
    assert some
    for body in some:
        fn, args = launcher(ops, body)
        for ki, rm in K.MODES:
            got, _ = launch(lattice, dim, fn, args, ki, rm)
            want = body.want(ki, rm)
            assert np.array_equal(got, want), f"{body}, keep_inside={ki}, refine_mode={rm}: {K.differing(got, want)}"


def check_launch_shapes(lattice, dim, fn, args, want_of, fn2=None, args2=None, want2_of=None, what=""):
    """``want_of(ki, rm)``: the verdict byte per cell of the whole lattice.  Cell lists (``first`` must be ignored), ranges with
    ``first > 0``, n around the block size, accumulation, canaries behind ``n``."""
    total = lattice[dim][3]
    rng = np.random.default_rng(41)
    for ki, rm in K.MODES:
        want = want_of(ki, rm)
        tag = f"{what}, keep_inside={ki}, refine_mode={rm}"
        for n in sorted({1, 255, 256, 257, total}):
            ids = rng.permutation(total)[:n].astype(np.int32)
            got, tail = launch(lattice, dim, fn, args, ki, rm, cells=ids, first=total - 1, pad=64)
            assert np.array_equal(got, want[ids]), f"{tag}: list of {n}: {K.differing(got, want[ids])}"
            assert np.all(tail == CANARY), f"{tag}: list of {n}: bytes behind n written"
            first = int(rng.integers(1, total - n + 1)) if n < total else 0
            got, tail = launch(lattice, dim, fn, args, ki, rm, first=first, n=n, pad=64)
            assert np.array_equal(got, want[first:first + n]), f"{tag}: range {first}+{n}: {K.differing(got, want[first:first + n])}"
            assert np.all(tail == CANARY), f"{tag}: range {first}+{n}: bytes behind n written"
        ones, _ = launch(lattice, dim, fn, args, ki, rm, invalid=np.ones(total, dtype=np.uint8))
        assert np.all(ones == 1), f"{tag}: pre-set flags were cleared"
        if fn2 is not None:
            both, _ = launch(lattice, dim, fn, args, ki, rm)
            both, _ = launch(lattice, dim, fn2, args2, ki, rm, invalid=both)
            assert np.array_equal(both, want | want2_of(ki, rm)), f"{tag}: two bodies in turn are not the OR of both"


@pytest.mark.parametrize("family", ["sphere2", "sphere3", "cyl_radius", "cyl_cap", "cone", "box"])
def test_launch_shapes_against_the_reference(ops, lattice, family):
    body = [b for b in K.bodies() if b.kind == "box" and b.dim == 3][1] if family == "box" else K.first_of(family)
    other = next(b for b in K.bodies() if b.family == "exact" and b.dim == body.dim)
    fn, args = launcher(ops, body)
    fn2, args2 = launcher(ops, other)
    check_launch_shapes(lattice, body.dim, fn, args, body.want, fn2, args2, other.want, what=str(body))


def one_cell_launches(lattice, dim, fn, args):
    """verdict byte per cell and mode pair from launches of one cell each (``n = 1``, ``first = i``), the path the goldens judge"""
    from sparsespatialsampling_amd.hipops import MaskCells
    total = lattice[dim][3]
    center, level, width, _ = lattice[dim]
    out = {}
    for ki, rm in K.MODES:
        buf = pt.zeros(total, dtype=pt.uint8, device="cuda")
        for i in range(total):
            fn(MaskCells(center, level, width, buf[i:i + 1], None, i, 1), *args, rm, ki)
        out[(ki, rm)] = buf.cpu().numpy()
        assert 0 < out[(ki, rm)].sum() < total
    return out


@pytest.mark.parametrize("key", ["polygon", "tri_dyadic", "prism_dyadic", "tet_generic", "pyr_dyadic", "mesh"])
def test_launch_shapes_against_one_cell_launches(ops, lattice, key):
    """the bodies without a lattice fixture: every launch shape gives what that kernel's one-cell launches give"""
    from sparsespatialsampling_amd import geometry
    if key == "polygon":
        poly = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "masks.npz"))["poly"]
        dim, fn, args = 2, ops.mask_polygon, (ops.to_device(np.ascontiguousarray(poly)),)
    elif key == "mesh":
        from tests import stl_meshes as M
        _, tri, lo, hi, ny, nz, bin_start, bin_facet = geometry.GeometrySTL3D("cube", False, M.CUBE_STL).kernel_spec()
        dim, fn, args = 3, ops.mask_mesh, (ops.MeshTable(tri, lo, hi, ny, nz, bin_start, bin_facet),)
    else:
        spec = polytope(geometry, key, False).kernel_spec()
        assert key in POLYTOPES
        dim = 2 if spec[0] == "triangle" else 3
        fn = {"triangle": ops.mask_triangle, "prism": ops.mask_prism, "tetrahedra": ops.mask_tetrahedra}[spec[0]]
        args = tuple(spec[1:])
    if dim == 3:                                                    # one-cell launches of the 512 cells of level 3 and 512 of level 4
        center, level, width, total = lattice[3]
        keep = pt.arange(0, 1024, device="cuda")
        lattice = {3: (center[keep].contiguous(), level[keep].contiguous(), width, 1024)}
    single = one_cell_launches(lattice, dim, fn, args)
    check_launch_shapes(lattice, dim, fn, args, lambda ki, rm: single[(ki, rm)], what=key)


def body_calls(lib, ops):
    """per entry point: (the body's dimensions, a call with valid body arguments that takes the ``s3_mask_cells``)"""
    import ctypes as C
    from sparsespatialsampling_amd import geometry
    from tests import stl_meshes as M
    null = C.c_void_p(0)
    zero, one = (C.c_double * 3)(0.0, 0.0, 0.0), (C.c_double * 3)(1.0, 1.0, 1.0)
    tri, dims = (C.c_double * 6)(0.0, 0.0, 1.0, 0.0, 0.0, 1.0), (C.c_int32 * 2)(0, 1)
    pos = (C.c_double * 12)(0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1)
    nrm = (C.c_double * 12)(*np.eye(3, 4).ravel())
    poly = ops.to_device(np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]))
    mesh = ops.MeshTable(*geometry.GeometrySTL3D("cube", False, M.CUBE_STL).kernel_spec()[1:])
    lo, hi = mesh.lo.ctypes.data_as(C.c_void_p), mesh.hi.ctypes.data_as(C.c_void_p)
    return {"s3_mask_box": ((2, 3), lambda c: lib.s3_mask_box(c, zero, one, 0, 0, null)),
            "s3_mask_sphere": ((2, 3), lambda c: lib.s3_mask_sphere(c, zero, 1.0, 0, 0, null)),
            "s3_mask_cylinder": ((3,), lambda c: lib.s3_mask_cylinder(c, zero, one, 1.0, 0.5, 0.5, 0, 0, 0, null)),
            "s3_mask_polygon": ((2,), lambda c: lib.s3_mask_polygon(c, poly.data_ptr(), 3, 0, 0, null)),
            "s3_mask_triangle": ((2,), lambda c: lib.s3_mask_triangle(c, tri, 0, 0, null)),
            "s3_mask_prism": ((3,), lambda c: lib.s3_mask_prism(c, zero, one, 1.0, dims, tri, 0, 0, null)),
            "s3_mask_tetrahedra": ((3,), lambda c: lib.s3_mask_tetrahedra(c, pos, nrm, 1, 0, 0, null)),
            "s3_mask_mesh": ((3,), lambda c: lib.s3_mask_mesh(c, mesh.tri.data_ptr(), mesh.nt, lo, hi, mesh.bin_start.data_ptr(),
                                                               mesh.bin_facet.data_ptr(), mesh.ny, mesh.nz, 0, 0, null))}


def test_empty_launch_with_null_arrays_is_ok(ops):
    """``n = 0`` with null arrays returns S3_OK: every entry point, in each of its body's dimensions"""
    import ctypes as C
    from sparsespatialsampling_amd import _lib
    lib = _lib.hip_lib()
    for name, (dims, call) in body_calls(lib, ops).items():
        for dim in dims:
            assert call(C.byref(_lib.S3MaskCells(None, None, None, 0, 0, dim, 1.0, None))) == 0, (name, dim)


def test_cells_of_the_wrong_dimension_are_refused(ops, lattice):
    """a body of one dimension on four real cells of the other: an error that names the entry point, before any launch"""
    import ctypes as C
    from sparsespatialsampling_amd import _lib
    lib = _lib.hip_lib()
    for name, (dims, call) in body_calls(lib, ops).items():
        if len(dims) == 2:
            continue
        dim = 5 - dims[0]
        center, level, width, _ = lattice[dim]
        invalid = pt.full((4,), CANARY, dtype=pt.uint8, device="cuda")
        cells = _lib.S3MaskCells(center.data_ptr(), level.data_ptr(), None, 0, 4, dim, width, invalid.data_ptr())
        assert call(C.byref(cells)) != 0, name
        assert name in lib.s3_last_error().decode(), name
        pt.cuda.synchronize()
        assert np.all(invalid.cpu().numpy() == CANARY), f"{name}: flags written by a refused call"


def test_null_cells_are_refused(ops):
    """a null struct pointer: an error from the check, which runs before any launch"""
    from sparsespatialsampling_amd import _lib
    lib = _lib.hip_lib()
    for name, (_, call) in body_calls(lib, ops).items():
        assert call(None) != 0, name
        assert name in lib.s3_last_error().decode(), name


def test_mask_cells_refuses_short_flags(ops, lattice):
    center, level, width, _ = lattice[2]
    with pytest.raises(TypeError):
        ops.MaskCells(center, level, width, pt.zeros(3, dtype=pt.uint8, device="cuda"), None, 0, 4)
    with pytest.raises(TypeError):
        ops.MaskCells(center, level, width, pt.zeros(3, dtype=pt.uint8, device="cuda"),
                      pt.arange(4, dtype=pt.int32, device="cuda"))


def test_backend_mask_of_three_bodies_is_the_or_of_each(ops, lattice):
    """``HipTreeBackend.mask`` over [box, sphere, polytope] accumulates like three calls of one geometry each"""
    from sparsespatialsampling_amd import geometry
    from sparsespatialsampling_amd.tree_backend import HipTreeBackend
    center, level, width, total = lattice[3]
    rng = np.random.default_rng(5)
    backend = HipTreeBackend(rng.random((64, 3)), rng.random(64), 8)
    backend.center, backend.level, backend.width = center, level, width
    bodies = [geometry.CubeGeometry("box", False, [0.1, 0.2, 0.3], [0.6, 0.7, 0.8]),
              geometry.SphereGeometry("ball", False, [0.6, 0.5, 0.4], 0.45), polytope(geometry, "tet_generic", False)]
    ids = np.arange(total - 1, -1, -3, dtype=np.int32)
    for rm in (False, True):
        for kw in (dict(first=0, n=total), dict(first=512, n=4), dict(cells=ids)):
            each = [backend.mask([g], rm, **kw) for g in bodies]
            assert kw.get("n") == 4 or (all(e.any() for e in each) and len({e.tobytes() for e in each}) == 3)
            assert np.array_equal(backend.mask(bodies, rm, **kw), each[0] | each[1] | each[2])
    backend.close()
