"""The references of tests/ray_cases.py against each other, and include/s3rays.h against its binding table (CPU only).

The emulation (the walk of the definition in float64) is held to the oracle (long double, brute force over all leaves, no walk) on
every grid, family and mode.  The bound is ``ray_cases.size_bound``: K * 2^-53 * segments * (D + P) * |d| * max|v|, D the larger |t|
at the domain's entry and exit and P the largest |coordinate| of the domain over |d_a|: the rounding of a plane's own coordinate
``fma(j, h_min, origin_a)`` is 2^-53 |coordinate| whatever the ray's parameter is, so a bound in D alone cannot hold for a short
chord far from the coordinate origin (measured without P: the rays that clip the refined corner of chain2d, where D |d| is of the
order of h_min = 3e-10 and the planes lie at 0.137, would need K = 8e7; with P no ray of any grid, family or mode needs more than
K = 1.25).  LINEAR adds the blend's own rounding, ``sample_cases.linear_bound``, integrated along the ray.

K_EMULATION = 2 is that measured 1.25 with room for another platform's libm-free arithmetic (there is none: + - * / sqrt fma only).
The GPU tests allow GPU_FACTOR = 8 times as much, the allowance of DESIGN 5.15: the build has contraction off, so the GPU should
reproduce the emulation, and the factor covers a legal difference in evaluation order only.

``segments`` and ``status`` are compared where no leaf's chord is within 1e-9 of the domain's chord (or within 64 roundings of a
parameter) of zero; that leaves out no ray of any random family here (the cap is 1 %), and on the dyadic grids with dyadic rays
nothing is left out at all.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ray_cases as rc

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3rays.h")
K_EMULATION, GPU_FACTOR, compare = rc.K_EMULATION, rc.GPU_FACTOR, rc.compare      # K_EMULATION = 2: measured 1.25 (one_cell / scaled, cell mode)
CAP = 0.01              # the share of a random family's rays the count comparison may leave out
MAX_STEPS = rc.MAX_STEPS


@pytest.mark.parametrize("name", rc.GRIDS)
def test_the_emulation_agrees_with_the_oracle(name):
    cell, node = rc.fields(name)
    for fam in rc.FAMILIES:
        o, d, t_range = rc.family(name, fam)
        ref = rc.truth(name, fam)
        left_out = int((ref["unclear"] & ~rc.overflows(d)).sum())
        for mode, field in (("cell", cell), ("linear", node)):
            em = rc.emulate_rays(name, o, d, t_range, field, mode, max_steps=MAX_STEPS)
            size, length, counts, n_clear, need = compare(name, fam, em, mode, field, K_EMULATION)
            print(f"{name} {fam} {mode}: K needed {need:.3f}, {n_clear} rays clear, {left_out} left out, {int(em['steps'].max())} blocks at the most")
            assert (size, length, counts) == (0, 0, 0), (name, fam, mode, size, length, counts)
            assert not (em["status"] == rc.STATUS["TRUNCATED"]).any()
            over = rc.overflows(d)                                      # by arithmetic: inf or NaN, never a finite number
            assert not np.isfinite(em["out"][over & (em["segments"] > 0)]).any()
        if fam in rc.RANDOM_FAMILIES:
            assert left_out <= CAP * rc.NR, (name, fam, left_out)
        if (name, fam) in rc.DYADIC_EXACT:                              # exact arithmetic: the bits, and nothing left out
            ints = rc.fields(name, integers=True)[0]
            want_out, want_len = rc.exact_expectation(rc.truth(name, fam, integers=True), d)
            em = rc.emulate_rays(name, o, d, t_range, ints, "cell", max_steps=MAX_STEPS)
            assert np.array_equal(em["out"], want_out) and np.array_equal(em["length"], want_len)
            assert np.array_equal(em["segments"], ref["segments"]) and np.array_equal(em["status"], ref["status"])


# (grid, family) pairs on which each planted mistake must show; "nearest" costs a brute-force search per block, so one small grid
MISTAKE_CASES = {"closed": [("dyadic2d", "axis"), ("dyadic3d", "axis"), ("tree2d", "axis")], "stop_at_empty": [("tree2d", "chords"), ("dyadic3d", "chords")],
                 "midpoint": [("tree2d", "chords")], "no_norm": [("tree2d", "scaled")], "nearest": [("tree2d", "chords")],
                 "no_trange": [("tree2d", "clipped")], "centre_planes": [("tree3d", "diagonal")]}


@pytest.mark.parametrize("mistake", rc.MISTAKES)
def test_every_planted_mistake_is_beyond_the_gpu_allowance(mistake):
    """beyond GPU_FACTOR x K_EMULATION in out or length, or a wrong ``segments`` / ``status`` on a clear ray, on every pair listed.
    ``midpoint`` is a mistake of LINEAR mode alone.  ``centre_planes`` is no mistake of size on most grids (a centre -+ h/2 is the
    lattice plane to an ulp); it shows where thin chords at corners of a 3-D tree no longer telescope."""
    for name, fam in MISTAKE_CASES[mistake]:
        cell, node = rc.fields(name)
        o, d, t_range = rc.family(name, fam)
        seen = {}
        for mode, field in (("cell", cell), ("linear", node)):
            em = rc.emulate_rays(name, o, d, t_range, field, mode, max_steps=MAX_STEPS, mistake=mistake)
            seen[mode] = compare(name, fam, em, mode, field, GPU_FACTOR * K_EMULATION)[:3]
        print(f"{mistake} on {name} / {fam}: rays off in (out, length, counts): {seen}")
        assert any(seen["linear"]), (mistake, name, fam, seen)
        assert mistake == "midpoint" or any(seen["cell"]), (mistake, name, fam, seen)
        if mistake == "midpoint":
            assert not any(seen["cell"])


def test_the_families_cover_what_they_are_for():
    share = {s: 0.0 for s in ("CROSSED", "MISSED", "BAD_RAY")}
    jumps = holes = 0
    for name in rc.GRIDS:
        for fam in rc.FAMILIES:
            ref = rc.truth(name, fam)
            for s in share:
                share[s] = max(share[s], float((ref["status"] == rc.STATUS[s]).mean()))
            jumps += int(ref["jumps"].sum())
            holes += int((ref["hole"] > 1e-6 * np.maximum(ref["D"], 1e-300)).sum())
            if name.startswith("chain") and fam in ("axis", "diagonal"):
                assert (ref["finest"] > 0).sum() >= 20, (name, fam)          # the finest cells of a chain are hit
        if name in ("tree2d", "tree3d", "dyadic2d", "dyadic3d"):
            assert int((rc.truth(name, "clipped")["hole"] > 0).sum()) > rc.NR // 10
    print(f"largest share of a family per status: {share}; {jumps} level jumps crossed, {holes} rays cross holes")
    assert all(v >= 0.05 for v in share.values()), share
    assert jumps > 100000 and holes > 10000
    o, d, _ = rc.family("tree2d", "hostile")
    assert np.isnan(o).any() and np.isnan(d).any() and np.isinf(o).any() and np.isinf(d).any() and (np.abs(o) == 1e300).any()
    assert (d == 1e300).any() and (d == 0).all(axis=1).any() and rc.overflows(d).any()
    o, d, _ = rc.family("dyadic2d", "axis")
    g = rc.lattice("dyadic2d")
    on_plane = ((o - g["origin"]) / g["h_min"] == np.floor((o - g["origin"]) / g["h_min"])) & (d == 0)
    assert on_plane.any(axis=1).sum() > rc.NR // 4                           # rays lying exactly in face planes
    o3, d3, _ = rc.family("dyadic3d", "axis")
    assert ((d3 == 0).sum(axis=1) == 2).any() and ((d3 == 0).sum(axis=1) == 1).any()


def test_a_body_is_crossed_in_a_few_steps():
    """the empty-block step: a chain of depth 31 is crossed in a few dozen blocks, not 2^31 lattice cells"""
    for name in ("chain2d", "chain3d"):
        for fam in ("chords", "axis", "diagonal"):
            o, d, t_range = rc.family(name, fam)
            em = rc.emulate_rays(name, o, d, t_range, rc.fields(name)[0], "cell", max_steps=MAX_STEPS)
            assert em["steps"].max() < 200 and not (em["status"] == rc.STATUS["TRUNCATED"]).any()
    o, d, t_range = rc.family("tree2d", "chords")
    em = rc.emulate_rays("tree2d", o, d, t_range, rc.fields("tree2d")[0], "cell", max_steps=3)
    cut = em["status"] == rc.STATUS["TRUNCATED"]
    assert cut.sum() > rc.NR // 2 and (em["steps"][cut] == 3).all() and (em["segments"][cut] <= 3).all()


# ---- the header -----------------------------------------------------------------------------------------------------------------
def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return text, sorted(set(re.findall(r"\b(s3_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_what_is_bound_and_exported():
    from sparsespatialsampling_amd import _lib, hipops
    text, names = declared()
    assert names == sorted(_lib.RAY_SIGNATURES) == ["s3_ray_integrate"]
    assert not set(names) & (set(_lib.HIP_SIGNATURES) | set(_lib.OVERLAP_SIGNATURES))
    lib = _lib.hip_lib()
    for name in names:
        assert hasattr(lib, name), f"{name} declared in s3rays.h but not exported by libs3hip.so"
        assert list(getattr(lib, name).argtypes) == _lib.RAY_SIGNATURES[name][1]
        params = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", text, flags=re.S).group(1)
        assert len(params.split(",")) == len(_lib.RAY_SIGNATURES[name][1]), name
        assert re.search(r"\bs3_stream\s+stream\s*$", params.strip()), f"{name} takes no stream"
    for code, value in {**hipops.RAY_MODES, **hipops.RAY_STATUS}.items():
        assert re.search(r"#define\s+S3_RAY_" + code.upper() + r"\s+" + str(value) + r"\b", text), code
    assert hipops.RAY_STATUS == rc.STATUS


def test_a_library_without_the_symbol_is_refused(monkeypatch):
    from sparsespatialsampling_amd import _lib
    _lib.hip_lib()
    monkeypatch.setattr(_lib, "_hip", None)
    monkeypatch.setattr(_lib, "RAY_SIGNATURES", {**_lib.RAY_SIGNATURES, "s3_ray_no_such_symbol": (None, [])})
    with pytest.raises(_lib.HipUnavailableError, match="s3_ray_no_such_symbol.*rebuild"):
        _lib.hip_lib()


def test_header_is_plain_c_and_leaves_the_others_alone(tmp_path):
    text, _ = declared()
    assert "torch" not in text.lower() and "at::" not in text and "std::" not in text and "Tensor" not in text
    assert '#include "s3hip.h"' in text
    src = tmp_path / "use_rays.c"
    src.write_text('#include "s3rays.h"\nint main(void) { return S3_RAY_LINEAR == 1 && S3_RAY_BROKEN == 4 && sizeof(s3_grid) > 0 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    from sparsespatialsampling_amd import _lib
    assert _lib.ABI_VERSION == 18 and "s3_ray" not in open(os.path.join(ROOT, "include", "s3hip.h")).read()


def test_the_build_and_the_package_know_the_feature():
    import __graft_entry__ as entry
    assert "rays.hip" in entry.HIP_SOURCES
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "s3rays.h" in text[text.index("def build_hip"):text.index("def build_topo")]
    import sparsespatialsampling_amd as s3
    from sparsespatialsampling_amd import projection
    assert s3.Rays is projection.Rays and s3.between is projection.between and {"Rays", "between"} <= set(s3.__all__)
    for f in ("from_grid", "from_dataloader", "from_s_cube", "integrate", "mean"):
        assert callable(getattr(projection.Rays, f))


def test_the_ray_builders():
    from sparsespatialsampling_amd import projection
    o, d, order = projection.parallel(None, (0, 0, 2), (16, 24), lo=(0, 0, 0), hi=(1, 2, 3))
    assert o.shape == d.shape == (384, 3) and (d == (0, 0, 2)).all() and sorted(order.tolist()) == list(range(384))
    assert np.array_equal(order[:9], [0, 1, 2, 3, 4, 5, 6, 7, 24]) and order.dtype == np.int32                # 8 x 8 tiles
    img = o.reshape(16, 24, 3)
    assert np.allclose(img[:, 0, 0], (np.arange(16) + 0.5) / 16) and np.allclose(img[0, :, 1], (np.arange(24) + 0.5) / 24 * 2) and (o[:, 2] == 1.5).all()
    o, d, order = projection.parallel(None, (0, 1), 8, lo=(0, 0), hi=(1, 1))
    assert np.allclose(o[:, 0], (np.arange(8) + 0.5) / 8) and np.array_equal(order, np.arange(8))
    o, d, order = projection.parallel(None, (1, 1, 1), (5, 7), lo=(-1, -1, -1), hi=(1, 1, 1))
    assert np.allclose(o @ np.ones(3), 0) and np.abs(o).max() <= np.sqrt(3) + 1e-12                            # on the plane through the centre
    o, d, t_range = projection.between([0.0, 0.0], [[1.0, 1.0], [2.0, 3.0]])
    assert np.array_equal(o, np.zeros((2, 2))) and np.array_equal(d, [[1, 1], [2, 3]]) and t_range == (0.0, 1.0)
    for bad in (dict(direction=(0, 0, 0)), dict(direction=(0, 0, 1), up=(0, 0, 3)), dict(direction=(0, 0, 1), hi=(1, 2, -3)), dict(direction=(0, 1))):
        with pytest.raises(ValueError):
            projection.parallel(None, bad.pop("direction"), (4, 4), **{"lo": (0, 0, 0), "hi": (1, 2, 3), **bad})
    with pytest.raises(ValueError):
        projection.parallel(None, (0, 0, 1), (4, 4))                                                           # no grid and no window
