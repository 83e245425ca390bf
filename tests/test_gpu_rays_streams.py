"""``s3_ray_integrate`` (include/s3rays.h) and ``Rays.integrate`` held to the stream they are given, with the harness of
tests/stream_cases.py (want / side / control; see there).  The cases are built here and never registered in ``sc.CASES``: that table
belongs to include/s3hip.h.  GPU only.

Poison: other valid rays through the same grid, another field of the same shape and another launch order.  Every control must differ.
"""
import numpy as np
import pytest
import torch as pt

from tests import ray_cases as rc
from tests import sample_cases as cases
from tests import stream_cases as sc

pytestmark = pytest.mark.gpu

N_RAYS, T_ROW = 777, 3
_HIP_ERROR = []


def _guarded(fn):
    """after a HIP error nothing more is started on the GPU in this process"""
    if _HIP_ERROR:
        pytest.fail("not run: an earlier test of this module ended with a HIP error: " + _HIP_ERROR[0], pytrace=False)
    try:
        return fn()
    except AssertionError:
        raise
    except Exception as e:                                      # noqa: BLE001
        text = f"{type(e).__name__}: {e}"
        if any(w in text.lower() for w in ("code -3", "illegal memory", "hip error", "hiperror", "memory access fault")):   # (-3: S3_EHIP)
            _HIP_ERROR.append(text[:300])
        raise


@pytest.fixture(scope="module", autouse=True)
def device():
    from sparsespatialsampling_amd import hipops
    hipops.device()
    sc.sleep_cycles_per_ms()
    yield
    pt.cuda.synchronize()


def _rays(name, fam):
    """(origins, dirs) real and poison: the first and the last N_RAYS rays of a family"""
    o, d, _ = rc.family(name, fam)
    return (o[:N_RAYS], o[-N_RAYS:]), (d[:N_RAYS], d[-N_RAYS:])


def _fields(name, mode, n_comp, dtype):
    base = rc.fields(name)[0 if mode == "cell" else 1]
    rng = sc.rng_of("rays" + name + mode)
    shape = (len(base), n_comp, T_ROW)
    return [rng.standard_normal(shape).astype(np.float32 if dtype == sc.F32 else np.float64) for _ in range(2)]


CASES = {}


def case(name, *covers, may_refuse=False):
    def register(make):
        CASES[name] = sc.Case(name, covers, make, may_refuse=may_refuse)
        return make
    return register


def _integrate(name, fam, mode, n_comp, dtype, with_order):
    def make():
        b = sc.Built()
        c = cases.case(name)
        ix = sc.ops().cell_index(sc.dev(c["centers"]), sc.dev(c["levels"]), c["width"])
        pt.cuda.synchronize()
        faces = sc.dev(c["faces"]) if mode == "linear" else None
        (ro, po), (rd, pd) = _rays(name, fam)
        o, d = b.inp(ro, po), b.inp(rd, pd)
        field = b.inp(*_fields(name, mode, n_comp, dtype))
        r = sc.rng_of("order" + name)
        order = b.inp(r.permutation(N_RAYS).astype(np.int32), r.permutation(N_RAYS).astype(np.int32)) if with_order else None
        out = b.new((N_RAYS, n_comp, T_ROW), sc.F64)
        length, segments, status = b.new((N_RAYS,), sc.F64), b.new((N_RAYS,), sc.I32), b.new((N_RAYS,), sc.I32)
        t_range = rc.family(name, fam)[2]
        b.call = lambda: list(sc.ops().ray_integrate(ix, o, d, field, mode, faces, t_range, order, rc.MAX_STEPS, out, length, segments, status))
        return b
    return make


# (four components: two launches, 3 + 1)
case("ray_integrate_cell_2d", "s3_ray_integrate")(_integrate("tree2d", "chords", "cell", 4, sc.F32, True))
case("ray_integrate_linear_3d", "s3_ray_integrate")(_integrate("tree3d", "clipped", "linear", 2, sc.F64, False))
case("ray_integrate_linear_2d_order", "s3_ray_integrate")(_integrate("tree2d", "axis", "linear", 1, sc.F32, True))


def _front_end(mode):
    def make():
        from sparsespatialsampling_amd.projection import Rays
        b = sc.Built()
        name = "tree2d"
        c = cases.case(name)
        o, d, t_range = rc.family(name, "clipped")
        rays = Rays(sc.dev(c["centers"]), sc.dev(c["levels"]), c["width"], sc.dev(o[:N_RAYS]), sc.dev(d[:N_RAYS]), sc.dev(c["nodes"]), sc.dev(c["faces"]),
                    t_range=t_range)
        pt.cuda.synchronize()
        real, poison = _fields(name, mode, 2, sc.F64)
        field = b.inp(real, poison)

        def call():
            res = rays.integrate(field, mode, max_steps=rc.MAX_STEPS, out_bytes=N_RAYS * 2 * 8 * 2)      # two batches
            return [res, rays.length, rays.segments, rays.status, rays.mean(field, mode, max_steps=rc.MAX_STEPS)]
        b.call = call
        return b
    return make


case("Rays.integrate_cell", "Rays.integrate", "s3_ray_integrate")(_front_end("cell"))
case("Rays.integrate_linear", "Rays.integrate", "s3_ray_integrate")(_front_end("linear"))


def test_every_entry_point_of_the_header_has_a_case():
    from sparsespatialsampling_amd import _lib
    covered = {entry for c in CASES.values() for entry in c.covers}
    assert set(_lib.RAY_SIGNATURES) <= covered and "Rays.integrate" in covered
    assert not set(CASES) & (set(sc.CASES) | set(sc.SIDE_ONLY))


@pytest.mark.parametrize("name", list(CASES))
def test_entry_point_on_the_stream_it_is_given(name):
    rep = _guarded(lambda: sc.check_case(CASES[name]))
    print(f"{name}: side == want, control != want ({rep['n_bytes']} bytes in {rep['n_results']} results; call {rep['ms']:.2f} ms, "
          f"delay {rep['delay_ms']:.1f} ms, the control's call was done {rep['lead_ms']:.1f} ms before its end)")
    assert rep["side_equals_want"] and rep["control_differs"] and not rep["refused"]
