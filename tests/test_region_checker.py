"""
The references of tests/region_cases.py against brute force and scipy, and the comparisons of tests/test_gpu_regions.py against
planted mistakes (CPU only).  The neighbour definition of include/s3hip.h is held against the integer brute force on every grid; the
GPU table itself (``hipops.cell_neighbours``, ``Grid.neighbours``) is compared with that definition in tests/test_gpu_regions.py.
"""
import numpy as np
import pytest
from scipy import ndimage

from tests import region_cases as rc


# ---- the neighbour definition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.GRIDS)
def test_neighbour_definition_gives_the_face_pairs(name):
    """same-or-coarser across every face = every pair of boxes sharing a face of positive area, whatever the level jump"""
    nbr = rc.emulate_neighbours(name)
    assert np.array_equal(rc.table_edges(nbr), rc.brute_edges(name))
    lv = rc.grid(name)["levels"]
    i, f = np.nonzero(nbr >= 0)
    assert (lv[nbr[i, f]] <= lv[i]).all()
    both = nbr[nbr[i, f], f ^ 1] == i                        # a pair stands on both sides exactly at equal level
    assert np.array_equal(both, lv[nbr[i, f]] == lv[i])


def test_the_front_end_exists():
    """what this family adds: fails where the package lacks it"""
    from sparsespatialsampling_amd import Grid, Regions, RegionTable, hipops
    assert isinstance(Grid.neighbours, property)
    assert all(callable(getattr(hipops, f)) for f in ("cell_neighbours", "region_label", "region_table"))
    assert callable(Regions.from_grid) and callable(RegionTable.largest)


@pytest.mark.parametrize("name", rc.TREES)
def test_tree_cases_are_tests(name):
    """by the reference alone: a random mask with two regions of two cells or more, one of them across a level jump of two or more"""
    seen = [rc.describe(name, rc.labels_of(name, f"random{share}")[:, t]) for share in (0.3, 0.5, 0.7) for t in range(rc.T_RANDOM)]
    assert any(many >= 2 and jump >= 2 for many, _, jump in seen), seen
    lv = rc.grid(name)["levels"].astype(np.int64)
    e = rc.brute_edges(name)
    assert np.abs(lv[e[:, 0]] - lv[e[:, 1]]).max() >= 3


# ---- the label reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.UNIFORM))
def test_reference_labels_partition_like_ndimage(name):
    d, level = rc.UNIFORM[name]
    for share in (0.3, 0.5, 0.7):
        mask = rc.random_mask(name, share)
        ref = rc.labels_of(name, f"random{share}")
        for t in range(mask.shape[1]):
            theirs, count = ndimage.label(mask[:, t].reshape((1 << level,) * d))         # (face connectivity is its default)
            theirs = theirs.reshape(-1)
            assert np.array_equal(ref[:, t] >= 0, theirs > 0)
            inside = theirs > 0
            pairs = np.unique(np.stack([ref[inside, t], theirs[inside]], axis=1), axis=0)
            assert len(pairs) == count == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1]))
            assert (ref[ref[inside, t], t] == ref[inside, t]).all() and (ref[inside, t] <= np.flatnonzero(inside)).all()


def test_drawn_masks_are_what_they_claim():
    lab = rc.labels_of("uniform2d", "drawn")
    masks = rc.uniform2d_masks()
    snake, comb, checker = (lab[:, k] for k in range(3))
    assert (np.unique(snake[snake >= 0]) == [0]).all() and 1900 <= (snake >= 0).sum() <= 2100
    assert (np.unique(comb[comb >= 0]) == [0]).all()
    assert np.array_equal(checker, np.where(masks["checkerboard"], np.arange(4096), -1))


# ---- planted mistakes ---------------------------------------------------------------------------------------------------------
def rejected(got, ref):
    with pytest.raises(AssertionError):
        rc.check_labels(got, ref)


@pytest.mark.parametrize("name", rc.TREES)
def test_label_check_rejects_planted_mistakes(name):
    ref = rc.labels_of(name, "random0.5")
    mask = rc.random_mask(name, 0.5)
    rc.check_labels(ref.copy(), ref)
    rejected(rc.reference_labels(rc.table_edges(rc.emulate_neighbours(name, same_level=True)), mask), ref)      # level jumps dropped
    rejected(rc.reference_labels(rc.touching_edges(name), mask), ref)                                          # corners connect
    rejected(rc.relabel_max(ref), ref)                                                                          # a member, not the minimum
    rejected(ref.astype(np.int64), ref)
    for f64 in (False, True):                                                                                   # the interval made open
        field = rc.smooth_field(name, f64)
        rejected(rc.reference_labels(rc.brute_edges(name), rc.in_mask(field, rc.LO, rc.HI, open_=True)), rc.labels_of(name, f"smooth{64 if f64 else 32}"))


def test_relabelled_partition_is_rejected_on_the_uniform_grid():
    ref = rc.labels_of("uniform2d", "drawn")
    other = rc.relabel_max(ref)
    assert np.array_equal(other >= 0, ref >= 0) and not np.array_equal(other, ref)
    rejected(other, ref)


@pytest.mark.parametrize("name", rc.TREES)
def test_table_check_rejects_planted_mistakes(name):
    labels, g = rc.labels_of(name, "random0.5"), rc.weight_field(name, rc.T_RANDOM)
    ref = rc.reference_table(name, labels, g)
    exact = {k: (v.astype(np.float64) if v.dtype == rc.LD else v) for k, v in ref.items()}
    rc.check_table(exact, ref)                                                          # (the rounded reference passes its own check)
    assert (np.diff(ref["offsets"]) >= 2).all() and (ref["n_cells"] >= 2).sum() >= 2
    wrong = rc.reference_table(name, labels, g, h_power=1)                              # V = h
    with pytest.raises(AssertionError):
        rc.check_table({k: (v.astype(np.float64) if v.dtype == rc.LD else v) for k, v in wrong.items()}, ref)
    for key, change in [("volume", lambda v: v * (1 + 2.0 ** -40)), ("n_cells", lambda v: v + 1), ("lo", lambda v: np.nextafter(v, -np.inf)),
                        ("g_max", lambda v: np.nextafter(v, np.inf)), ("centroid", lambda v: v * (1 + 2.0 ** -40)),
                        ("integral", lambda v: v + 2.0 ** -30 * np.abs(v).max()), ("label", lambda v: v[::-1].copy())]:
        with pytest.raises(AssertionError):
            rc.check_table({**exact, key: change(exact[key])}, ref)
