"""
The cases and references of tests/sample_cases.py judged on the CPU: the conditions every case has to meet, the definition of the
cell index in plain float64 against brute force, and planted mistakes that the references must catch -- a reference that passes a
wrong answer checks nothing on the GPU either.
"""
import numpy as np
import pytest

from tests import sample_cases as sc

LD = sc.LD


@pytest.mark.parametrize("name", sc.CASES)
def test_case_conditions(name):
    c = sc.case(name)
    ids, count, near = sc.truth(name)
    assert len(ids) == sc.NQ and count.max() <= 1, "a query lies in more than one cell: the cells overlap"
    hit = ids >= 0
    assert hit.any() and not hit.all() or name.startswith("chain")
    if not c["degenerate"]:
        differs = int((near[hit] != ids[hit]).sum())
        print(f"{name}: {hit.mean():.2f} hit, {differs} hits whose nearest centre is another cell")
        assert hit.mean() >= 0.30 and (~hit).mean() >= 0.05 and differs >= 50
    if name.startswith("chain"):            # the deepest cells are reached
        assert c["levels"][ids[hit]].max() == c["levels"].max() and (c["levels"][ids[hit]] >= c["levels"].max() - 3).sum() >= 100
    if name.startswith("tree"):
        assert c["levels"].max() >= 6 and c["width"] == 0.7


@pytest.mark.parametrize("name", sc.CASES)
def test_corner_order_of_faces(name):
    """``faces`` lists the corners (-,-), (-,+), (+,+), (+,-), at z+ then at z- in 3-D: on the reference's grids as on the synthetic"""
    c = sc.case(name)
    h = sc.cell_sizes(c)
    want = c["centers"][:, None, :] + sc.corner_signs(c["centers"].shape[1])[None] * h[:, None, None] / 2
    assert np.abs(c["nodes"][c["faces"]] - want).max() <= 1e-6 * h.min()


@pytest.mark.parametrize("name", sc.CASES)
def test_float64_definition_agrees_with_brute_force(name):
    c = sc.case(name)
    ix = sc.emulate_index(c)
    assert not ix["refused"].any() and ix["max_off"] <= 1e-6
    assert c["centers"].shape[1] * ix["depth"] <= 63
    assert (ix["starts"][1:] >= ix["ends"][:-1]).all()
    assert np.array_equal(sc.emulate_locate(c, c["queries"]), sc.truth(name)[0])


def test_chains_use_the_last_key_bits():
    assert sc.emulate_index(sc.case("chain2d"))["depth"] * 2 == 62 and sc.emulate_index(sc.case("chain3d"))["depth"] * 3 == 63


def test_dyadic_queries_lie_on_faces_and_bounds():
    for name in ("dyadic2d", "dyadic3d"):
        c = sc.case(name)
        q, depth = c["queries"], int(c["levels"].max())
        ids = sc.truth(name)[0]
        on_line = (q * 2.0 ** depth == np.rint(q * 2.0 ** depth))
        assert on_line.all(axis=1).sum() >= sc.NQ // 3
        assert (q == 0.0).any(axis=1).sum() >= 20 and (q == 1.0).any(axis=1).sum() >= 20
        assert (ids[(q == 1.0).any(axis=1)] == -1).all(), "the upper bound of the domain belongs to no cell"
        assert (ids[(q == 0.0).any(axis=1) & (q < 1.0).all(axis=1)] >= 0).any(), "the lower bound belongs to the domain"


# ---- planted mistakes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sc.CASES if not sc.case(n)["degenerate"]])
def test_nearest_centre_is_caught(name):
    ids, _, near = sc.truth(name)
    wrong = np.where(ids >= 0, near, -1)
    assert (wrong != ids).sum() >= 50


@pytest.mark.parametrize("name", ["dyadic2d", "dyadic3d"])
def test_closed_faces_are_caught(name):
    c = sc.case(name)
    assert (sc.emulate_locate(c, c["queries"], closed=True) != sc.truth(name)[0]).sum() >= 100


def test_missing_alignment_step_is_caught():
    """the root taken as the minimum corner: the coarse cells are then off their own lattice"""
    c = sc.case("offset2d")
    aligned, plain = sc.emulate_lattice(c), sc.emulate_lattice(c, align=False)
    assert not np.array_equal(aligned[0], plain[0])
    ix = sc.emulate_index(c, align=False)
    assert ix["refused"][1] > 0 or not np.array_equal(sc.emulate_locate(c, c["queries"], align=False), sc.truth("offset2d")[0])


@pytest.mark.parametrize("name", ["tree2d", "tree3d", "golden2d", "golden3d"])
def test_linear_reference_reproduces_affine_fields_and_catches_a_wrong_corner_order(name):
    c = sc.case(name)
    d = c["centers"].shape[1]
    ids = sc.truth(name)[0]
    coeff, offset = (1.25, -0.75, 2.5)[:d], 0.3
    f = sc.affine_nodes(c, coeff, offset)
    value, mag = sc.linear_reference(c, c["queries"], ids, f)
    hit = ids >= 0
    exact = c["queries"].astype(LD) @ np.asarray(coeff, dtype=LD) + LD(offset)
    bound = sc.linear_bound(d, mag) + sc.affine_bound(c, c["queries"], ids, coeff, offset)
    err = np.abs(value - exact)[hit]
    print(f"{name}: affine field at {float((err / bound[hit]).max()):.3g} of the bound")
    assert np.isnan(value[~hit].astype(np.float64)).all() and (err <= bound[hit]).all()
    swapped = sc.corner_signs(d).copy()
    swapped[[1, 3]] = swapped[[3, 1]]                   # counter-clockwise instead of the order of ``faces``
    wrong, _ = sc.linear_reference(c, c["queries"], ids, f, signs=swapped)
    assert (np.abs(wrong - exact)[hit] > 1e6 * bound[hit]).sum() >= hit.sum() // 2


@pytest.mark.parametrize("name", sorted(sc.REFUSALS))
def test_refusals_are_seen_by_the_definition(name):
    c, count = sc.refusal(name)
    refused = sc.emulate_index(c)["refused"]
    assert refused[sc.REFUSALS[name]] == count and np.count_nonzero(refused) == 1


def test_point_sets_are_built_on_the_host():
    """``line`` / ``plane`` / ``raster`` need no device"""
    from sparsespatialsampling_amd import sampling
    ln = sampling.line([0.0, 1.0, 2.0], [1.0, 1.0, 0.0], 5)
    assert ln.shape == (5, 3) and np.array_equal(ln[0], [0, 1, 2]) and np.array_equal(ln[-1], [1, 1, 0])
    pl = sampling.plane([0.0, 0.0, 0.5], [2.0, 0.0, 0.0], [0.0, 1.0, 0.0], (4, 2))
    assert pl.shape == (8, 3) and np.array_equal(pl.reshape(4, 2, 3)[1, 1], [0.75, 0.75, 0.5])
    ra = sampling.raster([0.0, 10.0], [4.0, 12.0], (4, 2))
    assert ra.shape == (8, 2) and np.array_equal(ra.reshape(4, 2, 2)[3, 0], [3.5, 10.5])
    assert sampling.raster([0, 0, 0], [1, 1, 1], (2, 3, 4)).shape == (24, 3)
    with pytest.raises(ValueError):
        sampling.plane([0, 0], [1, 0], [0, 1, 0], (2, 2))


def test_probe_is_exported():
    import sparsespatialsampling_amd as pkg
    from sparsespatialsampling_amd import sampling
    assert pkg.Probe is sampling.Probe and "Probe" in pkg.__all__
