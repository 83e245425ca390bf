"""
The references of tests/trace_cases.py checked against each other on the CPU, before anything runs on a GPU:

  * the plain-float64 emulation of the definition stays inside the affine bound (with K_EMULATION, an eighth of what the GPU tests
    allow) and inside the one-step bound (with ONE_STEP_EMULATION, likewise) on every case, and agrees with the long-double oracle
    on every length and status away from the faces;
  * every planted mistake exceeds the bounds the GPU tests use by a factor of 10^6 at least on one case at least;
  * the inputs can show what they are meant to show: every status that can occur does, in 5 % of the particles at least; under the
    cell rule a fifth of the accepted steps enters another cell and 50 of them at least cross a level jump; the particles left out
    because a point comes within 1e-6 cell sizes of a face are at most 1 %.
"""
import functools

import numpy as np
import pytest

from tests import trace_cases as tc

LD = tc.LD
RUN_IDS = [f"{name}-{rule}" for name, rule, _, _ in tc.AFFINE_RUNS]


@functools.lru_cache(maxsize=None)
def affine_pair(run, direction, mistake=None):
    name, rule, step, n_steps = tc.AFFINE_RUNS[run]
    g = tc.grid(name)
    field = tc.Affine(g)
    ref = tc.affine_reference(run, direction)
    emu = tc.emulate_trace(g, field.nodes(g)[:, :, None], tc.seeds(name), n_steps, rule, step, direction, mistake=mistake)
    return g, field, ref, emu


def affine_violation(ref, emu, common=False):
    """K the trace needs (inf where a length or status differs), over the particles away from the faces; ``common``: over the rows
    both sides have, whatever the lengths"""
    sure = ref["sure"]
    if common:
        return tc.violation(emu["points"][sure], ref["points"][sure], ref["bound"][sure], common=True)
    if not (np.array_equal(emu["length"][sure], ref["length"][sure]) and np.array_equal(emu["status"][sure], ref["status"][sure])):
        return np.inf
    return tc.violation(emu["points"][sure], ref["points"][sure], ref["bound"][sure])


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("run", range(len(tc.AFFINE_RUNS)), ids=RUN_IDS)
def test_emulation_inside_affine_bound(run, direction):
    name, rule, _, _ = tc.AFFINE_RUNS[run]
    g, _, ref, emu = affine_pair(run, direction)
    k = affine_violation(ref, emu)
    share = np.bincount(ref["status"], minlength=4) / len(ref["status"])
    crossed = emu["crossed"] / max(emu["accepted"], 1)
    print(f"{name} {rule} {direction:+d}: K needed {k:.3f}, left out {1 - ref['sure'].mean():.4f}, status shares {np.round(share, 3)}, "
          f"{emu['accepted']} steps accepted, {crossed:.2f} into another cell, {emu['jumped']} across a level jump")
    assert k <= tc.K_EMULATION
    assert 1 - ref["sure"].mean() <= tc.EXCLUDED_CAP
    assert min(share[tc.DONE], share[tc.LEFT], share[tc.SEED_OUTSIDE]) >= 0.05 and share[tc.STAGNANT] == 0
    if rule == "cell" and not g.degenerate:
        assert crossed >= 0.2 and emu["jumped"] >= 50


@functools.lru_cache(maxsize=None)
def path_pair(run, direction, mistake=None):
    name, n_snap, substeps = tc.PATH_RUNS[run]
    g = tc.grid(name)
    ref = tc.path_reference(run, direction)
    emu = tc.emulate_trace(g, tc.path_field(run).nodes(g, n_snap), tc.seeds(name), 0, "time", ref["dt_snapshot"] / substeps, direction,
                           substeps=substeps, mistake=mistake)
    return g, ref, emu


def path_violation(ref, emu, common=False):
    """as ``affine_violation`` for the snapshot rows of a pathline"""
    sure = ref["sure"]
    if not common and not (np.array_equal(emu["length"][sure], ref["rows"][sure]) and np.array_equal(emu["status"][sure], ref["status"][sure])):
        return np.inf
    return tc.violation(emu["points"][sure], ref["points"][sure], ref["bound"][sure], common=common)


@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("run", range(len(tc.PATH_RUNS)), ids=[r[0] for r in tc.PATH_RUNS])
def test_emulation_inside_affine_bound_pathline(run, direction):
    name, _, substeps = tc.PATH_RUNS[run]
    _, ref, emu = path_pair(run, direction)
    k = path_violation(ref, emu)
    share = np.bincount(ref["status"], minlength=4) / len(ref["status"])
    print(f"{name} {direction:+d}: K needed {k:.3f}, left out {1 - ref['sure'].mean():.4f}, status shares {np.round(share, 3)}")
    assert k <= tc.K_EMULATION
    assert 1 - ref["sure"].mean() <= tc.EXCLUDED_CAP
    assert min(share[tc.DONE], share[tc.LEFT], share[tc.SEED_OUTSIDE]) >= 0.05


@pytest.mark.parametrize("rule", ["cell", "time"])
@pytest.mark.parametrize("name", tc.GRIDS)
def test_emulation_inside_one_step_bound(name, rule):
    g = tc.grid(name)
    field, step, ref = tc.one_step_reference(name, rule)
    emu = tc.emulate_trace(g, field[:, :, None], tc.seeds(name), 1, rule, step, 1)
    near = ref["ok"] & (ref["margin"] <= tc.FACE_MARGIN)
    sure = ref["ok"] & ~near
    print(f"{name} {rule}: {sure.sum()} seeds take the step, {near.sum()} of them left out near a face")
    assert near.sum() <= tc.EXCLUDED_CAP * len(near) and sure.sum() >= 0.05 * len(sure)
    assert (emu["length"][sure] == 2).all() and (emu["status"][sure] == tc.DONE).all()
    ratio = float((np.abs(emu["points"][sure, 1].astype(LD) - ref["end"][sure]) / ref["bound"][sure]).max())
    print(f"    largest error / B: {ratio:.3f}")
    assert ratio <= tc.ONE_STEP_EMULATION


@pytest.mark.parametrize("mistake", tc.MISTAKES)
def test_planted_mistakes_fail(mistake):
    worst = 0.0
    if mistake == "frozen_time":
        for run, (name, _, substeps) in enumerate(tc.PATH_RUNS):
            _, ref, emu = path_pair(run, 1, mistake)
            worst = max(worst, path_violation(ref, emu, common=True) / tc.K_AFFINE)
            if worst >= 1e6:
                break
    else:
        for run in range(len(tc.AFFINE_RUNS)):
            _, _, ref, emu = affine_pair(run, 1, mistake)
            # (positions on the rows both sides have; the mistake that only moves the end shows in the lengths alone)
            worst = max(worst, affine_violation(ref, emu, common=mistake != "left_by_end_point") / tc.K_AFFINE)
            if worst >= 1e6:
                break
    print(f"{mistake}: {worst:.3g} times the bound of the GPU tests")
    assert worst >= 1e6


def test_planted_mistakes_fail_one_step():
    """the one-step bound on a random field sees the mistakes that change a velocity"""
    for mistake in ("k2_full_step", "equal_weights", "nearest_centre"):
        g = tc.grid("tree2d")
        field, step, ref = tc.one_step_reference("tree2d", "cell")
        emu = tc.emulate_trace(g, field[:, :, None], tc.seeds("tree2d"), 1, "cell", step, 1, mistake=mistake)
        sure = ref["ok"] & (ref["margin"] > tc.FACE_MARGIN) & (emu["length"] == 2)
        ratio = float((np.abs(emu["points"][sure, 1].astype(LD) - ref["end"][sure]) / ref["bound"][sure]).max())
        assert ratio >= 1e6 * tc.ONE_STEP_MARGIN, mistake


@pytest.mark.parametrize("name", ["dyadic2d", "dyadic3d"])
def test_exact_case_is_exact_in_the_emulation(name):
    """where every operation is exact, the float64 emulation equals the integer prediction bit for bit -- also ON faces"""
    ex = tc.exact_case(name)
    g = tc.grid(name)
    for rule in ("time", "cell"):
        emu = tc.emulate_trace(g, ex["field"], ex["seeds"], ex["n_steps"], rule, ex["dt"] if rule == "time" else ex["cfl"], 1)
        points, length, status = ex[rule]
        assert np.array_equal(emu["length"], length) and np.array_equal(emu["status"], status)
        assert np.array_equal(emu["points"], points, equal_nan=True)
        share = np.bincount(status, minlength=4) / len(status)
        assert min(share[tc.DONE], share[tc.LEFT], share[tc.SEED_OUTSIDE]) >= 0.05
