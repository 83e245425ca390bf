"""
One field, eight ways in: what the analysis front-ends do with the array they are handed -- which side and kind of array comes back,
that the layout changes no bit, and what is read where it lies.  Public API only.

The grid is 2-D, 12 x 12 cells of one level with 169 nodes; a scalar field of T = 6 snapshots (for the windows: inside a buffer of 9
columns) and a vector field [N, 2, 6].  The same values go in as

    1 numpy f64        2 numpy f32        3 host tensor f64        4 a non-contiguous host window
    5 device f32       6 a device window ``buf[:, 1:7]`` in f64: rows that start 8 bytes off the 16-byte grid, the narrowest row width
    7 a device view with inner stride 2                            8 a host int32 field (widened to f64)

through ``Gradient.magnitude``, ``Probe.sample`` (both modes), ``Isosurface.count`` / ``.extract`` and ``ReconstructionError.update``
(the ``orig`` side); ``welch`` and ``DMD`` take tensors only: kinds 3, 5, 6.

Asserted: the result's kind and side are what the docstrings say; all kinds of one dtype give identical bits (every kernel here sums
in an order the layout does not touch, the layout only chooses the loads) and kind 8 the bits of its ``.double()``; a spy over ``hipops.to_device`` never sees
the field of kinds 5 and 6 -- nothing is copied -- and sees the field of kind 7 exactly once.
"""
import numpy as np
import pytest
import torch as pt

from tests import sample_cases as sc
from sparsespatialsampling_amd import hipops
from sparsespatialsampling_amd.differential import Gradient
from sparsespatialsampling_amd.dmd import DMD
from sparsespatialsampling_amd.isosurface import Isosurface
from sparsespatialsampling_amd.reconstruction import ReconstructionError
from sparsespatialsampling_amd.sampling import Probe
from sparsespatialsampling_amd.spectral import welch

pytestmark = pytest.mark.gpu

SIDE, T, PITCH = 12, 6, 9
NUMPY, HOST, DEVICE = "numpy", "host", "device"
SIDE_OF = {1: NUMPY, 2: NUMPY, 3: HOST, 4: HOST, 5: DEVICE, 6: DEVICE, 7: DEVICE, 8: HOST}
SAME_BITS = ((1, 3, 4, 6, 7), (2, 5))          # float64 / float32; kind 8 against its .double()
IN_PLACE, COPIED_ONCE = (5, 6), (7,)


def kinds(values, ints):
    """the eight kinds of the scalar field ``values`` f64 numpy [rows, T] (``ints`` int32 numpy: kind 8) and the field kind 8 must equal"""
    rows = len(values)
    host = pt.zeros((rows, PITCH), dtype=pt.float64)
    host[:, 1:1 + T] = pt.from_numpy(values)
    buf = pt.full((rows, PITCH), float("nan"), dtype=pt.float64, device="cuda")
    buf[:, 1:1 + T] = pt.from_numpy(values).cuda()
    wide = pt.full((rows, 2 * T), float("nan"), dtype=pt.float64, device="cuda")
    wide[:, ::2] = pt.from_numpy(values).cuda()
    out = {1: values, 2: values.astype(np.float32), 3: pt.from_numpy(values.copy()), 4: host[:, 1:1 + T],
           5: pt.from_numpy(values.astype(np.float32)).cuda(), 6: buf[:, 1:1 + T], 7: wide[:, ::2], 8: pt.from_numpy(ints.copy())}
    assert not out[4].is_contiguous() and not out[6].is_contiguous() and out[6].data_ptr() % 16 == 8 and out[7].stride(1) == 2
    return out, pt.from_numpy(ints.copy()).double()


@pytest.fixture(scope="module")
def world():
    side = np.arange(SIDE)
    grid = sc.grid_from_anchors(np.array(np.meshgrid(side, side, indexing="ij")).reshape(2, -1).T, np.full(SIDE * SIDE, 4), 4, 1.0,
                                (0.0, 0.0, 0.0))
    n_cells, n_nodes = len(grid["centers"]), len(grid["nodes"])
    assert (n_cells, n_nodes) == (144, 169)
    rng = np.random.default_rng(17)
    w = {"grid": grid, "queries": 0.05 + 0.65 * rng.random((301, 2))}             # inside [0, 0.75]^2, the 12 x 12 cells
    w["node"], w["node8"] = kinds(rng.standard_normal((n_nodes, T)), rng.integers(-3, 4, (n_nodes, T)).astype(np.int32))
    w["cell"], w["cell8"] = kinds(rng.standard_normal((n_cells, T)), rng.integers(-3, 4, (n_cells, T)).astype(np.int32))
    vec = rng.standard_normal((n_nodes, 2, T))
    w["vector"] = {1: vec, 3: pt.from_numpy(vec.copy()), 5: pt.from_numpy(vec.astype(np.float32)).cuda(), 6: pt.from_numpy(vec).cuda()}
    w["grid_field"] = pt.from_numpy(rng.standard_normal((n_cells, T))).cuda()
    w["grid_vector"] = pt.from_numpy(rng.standard_normal((n_cells, 2, T))).cuda()
    w["gradient"] = Gradient(grid["nodes"])
    w["probe"] = Probe(grid["centers"], grid["levels"], grid["width"], w["queries"], nodes=grid["nodes"], faces=grid["faces"])
    w["iso"] = Isosurface(grid["nodes"], grid["faces"])
    return w


class Spy:
    """counts the calls of ``hipops.to_device`` that are handed (a view of) the memory of ``field``"""

    def __init__(self, monkeypatch):
        self.seen, real = [], hipops.to_device

        def spy(x, dtype=None):
            self.seen.append(x)
            return real(x, dtype)
        monkeypatch.setattr(hipops, "to_device", spy)

    def count(self, field):
        base = field.untyped_storage().data_ptr()
        return sum(isinstance(x, pt.Tensor) and x.is_cuda and x.untyped_storage().data_ptr() == base for x in self.seen)


def assert_side(results, side, what):
    for r in results:
        if isinstance(r, float):
            continue
        if side == NUMPY:
            assert isinstance(r, np.ndarray), f"{what}: {type(r).__name__} for a numpy field"
        else:
            assert isinstance(r, pt.Tensor) and r.is_cuda == (side == DEVICE), f"{what}: a result on the wrong side of a {side} field"


def bits(r):
    a = np.ascontiguousarray(r.cpu().numpy() if isinstance(r, pt.Tensor) else r)
    if np.iscomplexobj(a):
        a = np.ascontiguousarray(np.stack([a.real, a.imag]))
    return a.view(np.int64) if a.dtype == np.float64 else a


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def through(entry, fields, widened, monkeypatch, what, sides=SIDE_OF, groups=SAME_BITS, in_place=IN_PLACE):
    """``entry(field)`` -> tuple of results, for every kind: sides, bits, copies"""
    got = {}
    for kind, field in fields.items():
        spy = Spy(monkeypatch)
        got[kind] = entry(field)
        monkeypatch.undo()
        assert_side(got[kind], sides[kind], f"{what}, kind {kind}")
        if kind in in_place:
            assert spy.count(field) == 0, f"{what}: the field of kind {kind} was copied"
        if kind in COPIED_ONCE:
            assert spy.count(field) == 1, f"{what}: the field of kind {kind} was copied {spy.count(field)} times"
    for group in groups:
        for kind in group[1:]:
            if group[0] in got and kind in got:
                assert same(got[group[0]], got[kind]), f"{what}: kinds {group[0]} and {kind} differ"
    if widened is not None:
        assert same(got[8], entry(widened)), f"{what}: the int32 field is not its .double()"
    return got


def test_gradient_magnitude(world, monkeypatch):
    grad = world["gradient"]
    got = through(lambda f: (grad.magnitude(f),), world["node"], world["node8"], monkeypatch, "Gradient.magnitude")
    assert all(tuple(r[0].shape) == (169, T) and bits(r[0]).dtype == np.int64 for r in got.values())
    got = through(lambda f: (grad.magnitude(f),), world["vector"], None, monkeypatch, "Gradient.magnitude [N, 2, T]",
                  sides={1: NUMPY, 3: HOST, 5: DEVICE, 6: DEVICE}, groups=((1, 3, 6),))
    assert all(tuple(r[0].shape) == (169, 2, T) for r in got.values())


@pytest.mark.parametrize("mode", ["cell", "linear"])
def test_probe_sample(world, monkeypatch, mode):
    probe = world["probe"]
    assert probe.inside.all()
    which = "cell" if mode == "cell" else "node"
    got = through(lambda f: (probe.sample(f, mode=mode),), world[which], world[which + "8"], monkeypatch, f"Probe.sample {mode}")
    assert all(tuple(r[0].shape) == (301, T) and not np.isnan(np.asarray(r[0].cpu() if isinstance(r[0], pt.Tensor) else r[0])).any()
               for r in got.values())
    if mode == "linear":
        got = through(lambda f: (probe.sample(f, mode=mode),), world["vector"], None, monkeypatch, "Probe.sample linear [N, 2, T]",
                      sides={1: NUMPY, 3: HOST, 5: DEVICE, 6: DEVICE}, groups=((1, 3, 6),))
        assert all(tuple(r[0].shape) == (301, 2, T) for r in got.values())


def test_isosurface(world, monkeypatch):
    iso = world["iso"]
    counts = through(lambda f: (iso.count(f, 0.25),), world["node"], world["node8"], monkeypatch, "Isosurface.count",
                     sides={k: NUMPY for k in SIDE_OF})                             # int64 numpy [T] whatever came in
    assert all(r[0].dtype == np.int64 and r[0].shape == (T,) and r[0].min() > 0 for r in counts.values())

    def extract(f):
        res = iso.extract(f, 0.25)
        assert isinstance(res.offsets, np.ndarray) and len(res) == res.offsets[-1]
        return res.offsets, res.vertices, res.edges, res.frac, res.cells
    got = through(lambda f: extract(f)[1:], world["node"], world["node8"], monkeypatch, "Isosurface.extract")
    for kind, r in got.items():
        assert len(r[0]) == counts[kind][0].sum() and tuple(r[0].shape[1:]) == (2, 2), f"kind {kind}"


def test_reconstruction_error_orig_side(world, monkeypatch):
    grid = world["grid"]

    def entry(grid_field):
        def run(f):
            err = ReconstructionError(grid["centers"], grid["nodes"]).update(grid_field, f)
            return err.error_time, err.error_total, err.error_space_mean, err.error_space_std
        return run
    tensor_sides = {k: (HOST if s == NUMPY else s) for k, s in SIDE_OF.items()}       # tensors on the field's side, also for numpy
    got = through(entry(world["grid_field"]), world["node"], world["node8"], monkeypatch, "ReconstructionError.update", sides=tensor_sides)
    assert all(tuple(r[0].shape) == (T,) and isinstance(r[1], float) and tuple(r[2].shape) == (169,) for r in got.values())
    assert all(got[1][1] == got[k][1] for k in SAME_BITS[0])
    # (a contiguous device field [N, 2, T] passes through ``to_device``, which hands it back as it is: no spy here)
    through(entry(world["grid_vector"]), world["vector"], None, monkeypatch, "ReconstructionError.update [N, 2, T]",
            sides={1: HOST, 3: HOST, 5: DEVICE, 6: DEVICE}, groups=((1, 3, 6),), in_place=())


def test_welch_and_dmd_take_tensors(world, monkeypatch):
    fields = {k: world["node"][k] for k in (3, 5, 6)}
    # detrend=False: with detrending the row means come first (s3_row_moments), whose summation order follows the vector width the
    # layout allows, so the bits of a pitched window are those of the dense matrix only without it
    got = through(lambda f: welch(f, 0.1, nperseg=4, detrend=False), fields, None, monkeypatch, "welch", groups=((3, 6),))
    assert all(tuple(r[0].shape) == (3,) and tuple(r[1].shape) == (169, 3) for r in got.values())

    def dmd(f):
        model = DMD(f, 0.1, rank=2)
        return model.eigvals, model.amplitude, model.modes, model.reconstruction(0, 2)
    got = through(dmd, fields, None, monkeypatch, "DMD", groups=((3, 6),))
    assert all(tuple(r[2].shape) == (169, 2) and tuple(r[3].shape) == (169, 2) for r in got.values())
