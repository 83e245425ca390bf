"""Curved bodies at exact and one-ulp ties (tests/golden/masks_curved.npz, verdicts of the real reference): the CPU oracle and the
package's host classes against them, and the conditions the fixture has to meet.  CPU only."""
import numpy as np
import pytest
import torch as pt

from oracle import s3_oracle as orc
from tests import masks_curved_cases as K


def oracle_verdicts(body, ki, rm):
    center, level, width = K.cells(body.dim)
    fn = {"sphere": orc.mask_sphere, "cylinder": orc.mask_cylinder, "box": orc.mask_box}[body.kind]
    return fn(center, level, width, *body.args, rm, ki).astype(np.uint8)


@pytest.mark.parametrize("kind", ["sphere", "cylinder", "box"])
def test_oracle_equals_the_reference_on_every_body(kind):
    """one call over all cells with their real levels per body and mode pair; exact equality"""
    for body in (b for b in K.bodies() if b.kind == kind):
        for ki, rm in K.MODES:
            got, want = oracle_verdicts(body, ki, rm), body.want(ki, rm)
            assert np.array_equal(got, want), f"{body}, keep_inside={ki}, refine_mode={rm}: {K.differing(got, want)}"


def test_fixture_conditions():
    """every family has at least 8 cell verdicts the plain sequential evaluation gets wrong; every exact-tie body has at least 8
    nodes exactly on its surface; the verdicts are no trivial tables"""
    z = K.fixture()
    for family in K.FAMILIES:
        assert int(z[f"seq_wrong_{family}"]) >= 8, (family, int(z[f"seq_wrong_{family}"]))
    for key in ("sphere2", "sphere3", "cyl"):
        assert z[key + "_on_surface"].min() >= 8, (key, z[key + "_on_surface"])
    assert str(z["torch_version"]) and str(z["cpu_capability"])
    for body in K.bodies():
        for ki, rm in K.MODES:
            assert 0 < body.want(ki, rm).sum() < len(body.bits), body
    assert {b.family for b in K.bodies()} == set(K.FAMILIES) | {"exact", "box"}


def test_host_classes_equal_the_reference():
    """SphereGeometry / CylinderGeometry3D / CubeGeometry .check_cell of this package, which take their roundings from torch as
    the reference does: on the cells around the chosen nodes, the cells the surface crosses and every eleventh cell"""
    from sparsespatialsampling_amd import geometry
    z = K.fixture()
    here = pt.backends.cpu.get_cpu_capability()
    if here != str(z["cpu_capability"]):
        pytest.skip(f"torch's CPU capability here is {here}, the fixture was made with {z['cpu_capability']}: the reference's own "
                    f"roundings differ between them")
    make = {"sphere": lambda ki, a: geometry.SphereGeometry("g", ki, list(a[0]), a[1]),
            "cylinder": lambda ki, a: geometry.CylinderGeometry3D("g", ki, list(a[0]), a[1]),
            "box": lambda ki, a: geometry.CubeGeometry("g", ki, list(a[0]), list(a[1]))}
    for body in K.bodies():
        center, level, width = K.cells(body.dim)
        h = (0.5 * width) / 2.0 ** level
        crossed = (body.want(0, 1) == 1) & (body.want(0, 0) == 0)                    # some node inside, not all
        near = np.zeros(len(center), dtype=bool)
        for x in body.nodes:
            near |= np.all(np.abs(center - x) <= h[:, None], axis=1)
        pick = np.flatnonzero(crossed | near | (np.arange(len(center)) % 11 == 0))
        nodes = [pt.from_numpy(n) for n in K.nodes_of(body.dim)[pick]]
        for ki, rm in K.MODES:
            g = make[body.kind](bool(ki), body.args)
            got = np.array([g.check_cell(n, bool(rm)) for n in nodes], dtype=np.uint8)
            want = body.want(ki, rm)[pick]
            assert np.array_equal(got, want), f"{body}, keep_inside={ki}, refine_mode={rm}: {K.differing(got, want)}"
