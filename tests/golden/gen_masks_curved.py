"""
Fixture ``masks_curved.npz``: verdicts of the REAL reference (through ``ref_stubs.py``) for spheres, cylinders, cones and boxes on
the mixed-level lattice ``inputs.curved_cells`` -- at exact ties and at one-ulp ties of the curved surfaces.

    python tests/golden/gen_masks_curved.py

Two groups of bodies per family (sphere 2-D, sphere 3-D, cylinder radius, cylinder cap, cone):

exact ties     ``inputs.CURVED_EXACT``: dyadic bodies whose surface passes through lattice nodes; every operation is exact.
one-ulp ties   generic bodies (``inputs.CURVED_GENERIC``).  For a chosen node the distance d that the reference itself computes is
               found by asking the reference (a cell whose nodes all are that node, radii around the plain value): d is the
               smallest radius that takes the node in.  Three bodies follow, with radius nextafter(d, 0), d, nextafter(d, inf).
               Nodes are chosen on purpose: mostly those where the plain sequential evaluation (sqrt((a0*a0 + a1*a1) + a2*a2),
               cross components a*b - c*d) differs from the reference's d, a few where it agrees.
    cone       the radius at the far end is fixed; the radius at the start is searched so that the local radius the reference
               interpolates at the node is nextafter(d, 0), d, nextafter(d, inf).
    cap        the projection on the axis and the axis length are the same operations in both evaluations, so a cap tie alone
               cannot tell them apart.  The chosen node lies on the rim: in the end plane and at the radius.  The axis has few
               bits and the start point is placed so that (x - p0).axis = axis.axis holds exactly; what is left is
               fl(N / fl(sqrt N)) against fl(sqrt N), which falls one ulp below, on, or one ulp above it depending on N.  Three
               axes, one per outcome; several rim nodes, each with the three radii around its d.  End points are exact in float32, through
               which the reference rounds them.

Stored per family: the constructor arguments, one byte per (body, cell) with bit ``2 * keep_inside + refine_mode`` = the reference's
``check_cell``, the number of cell verdicts the sequential evaluation gets wrong, per exact body the number of nodes on its surface
(exact rational arithmetic), and torch's version and CPU capability: the reference's roundings are those of the torch build.

Contains no reference code: it calls the reference's public classes.
"""
import os
import sys
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_stubs  # noqa: E402,F401

import numpy as np  # noqa: E402
import torch as pt  # noqa: E402

from inputs import CURVED_BOXES, CURVED_EXACT, CURVED_GENERIC, cell_nodes, curved_cells  # noqa: E402

MODES = [(ki, rm) for ki in (0, 1) for rm in (0, 1)]             # bit 2 * ki + rm
MIN_WRONG, MIN_ON_SURFACE = 8, 8


# ---- the plain sequential evaluation (numpy never fuses) ---------------------------------------------------------------------------
def seq_sphere_dist(x, pos):
    t = x - np.asarray(pos, dtype=np.float64)
    s = t[..., 0] * t[..., 0]
    for j in range(1, t.shape[-1]):
        s = s + t[..., j] * t[..., j]
    return np.sqrt(s)


def seq_cylinder(x, position):
    """(distance from the axis, projection on it, axis length) of the plain evaluation; end points through float32"""
    p = np.asarray(position, dtype=np.float32)
    p0, a = p[0].astype(np.float64), (p[1] - p[0]).astype(np.float64)
    norm = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    v = x - p0
    c0 = a[1] * v[..., 2] - a[2] * v[..., 1]
    c1 = a[2] * v[..., 0] - a[0] * v[..., 2]
    c2 = a[0] * v[..., 1] - a[1] * v[..., 0]
    nd = np.sqrt((c0 * c0 + c1 * c1) + c2 * c2) / norm
    proj = ((v[..., 0] * a[0] + v[..., 1] * a[1]) + v[..., 2] * a[2]) / norm
    return nd, proj, norm


def seq_cylinder_inside(x, position, radius):
    nd, proj, norm = seq_cylinder(x, position)
    rad = radius[0] + proj / norm * (radius[1] - radius[0]) if isinstance(radius, list) else radius
    return (0.0 <= proj) & (proj <= norm) & (nd <= rad)


def verdict_bits(inside):
    """[n_cells, n_nodes] bool -> one byte per cell, bit 2 * keep_inside + refine_mode (GeometryObject._apply_mask)"""
    all_in, any_in = inside.all(1), inside.any(1)
    out = np.zeros(len(inside), dtype=np.uint8)
    for ki, rm in MODES:
        v = (~all_in if ki else any_in) if rm else (~any_in if ki else all_in)
        out |= v.astype(np.uint8) << (2 * ki + rm)
    return out


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def ref_bits(make, nodes):
    """the reference's check_cell for every cell and mode"""
    out = np.zeros(len(nodes), dtype=np.uint8)
    cells = [pt.from_numpy(np.ascontiguousarray(n)) for n in nodes]
    for ki, rm in MODES:
        g = make(bool(ki))
        out |= np.array([g.check_cell(c, bool(rm)) for c in cells], dtype=np.uint8) << (2 * ki + rm)
    return out


def ref_takes(make, x):
    """does the reference count the point ``x`` as inside?  (a cell whose nodes all are x, all-inside rule)"""
    cell = pt.from_numpy(np.repeat(np.asarray(x, dtype=np.float64)[None], 2 ** len(x), 0))
    return bool(make(False).check_cell(cell, False))


def ref_threshold(make_with_radius, x, guess):
    """the smallest radius with which the reference takes ``x`` in = the distance the reference computes for it"""
    r = float(guess - 16 * np.spacing(guess))
    assert not ref_takes(make_with_radius(r), x), "the reference's distance is more than 16 ulps below the plain one"
    for _ in range(32):
        r = float(np.nextafter(r, np.inf))
        if ref_takes(make_with_radius(r), x):
            return r
    raise AssertionError("the reference's distance is more than 16 ulps above the plain one")


def around(d):
    return [float(np.nextafter(d, 0.0)), float(d), float(np.nextafter(d, np.inf))]


def lattice_nodes(d):
    center, level, width = curved_cells(d)
    n = cell_nodes(center, level, width)[level == 4].reshape(-1, d)
    return np.unique(n, axis=0)


def choose(rng, candidates, d_seq, d_ref_of, n_diff, n_same):
    """nodes in seeded random order: the first ``n_diff`` whose reference distance differs from the plain one, the first ``n_same``
    where both agree -> [(node, d_ref)]"""
    diff, same = [], []
    for i in rng.permutation(len(candidates)):
        if len(diff) >= n_diff and len(same) >= n_same:
            break
        d_ref = d_ref_of(candidates[i], d_seq[i])
        if d_ref != d_seq[i] and len(diff) < n_diff:
            diff.append((candidates[i], d_ref))
        elif d_ref == d_seq[i] and len(same) < n_same:
            same.append((candidates[i], d_ref))
    assert len(diff) == n_diff and len(same) == n_same
    return diff + same


# ---- exact count of nodes on a surface --------------------------------------------------------------------------------------------
def frac(v):
    return [Fraction(float(t)) for t in v]


def on_sphere(nodes, pos, r):
    c, r2 = frac(pos), Fraction(r) ** 2
    return sum(sum((Fraction(float(t)) - cj) ** 2 for t, cj in zip(x, c)) == r2 for x in nodes)


def on_cylinder(nodes, position, radius):
    """nodes on the lateral surface or on an end disc (the end points are dyadic: float32 keeps them)"""
    p0, p1 = frac(position[0]), frac(position[1])
    a = [q - p for p, q in zip(p0, p1)]
    aa = sum(t * t for t in a)
    r0, r1 = (Fraction(radius[0]), Fraction(radius[1])) if isinstance(radius, list) else (Fraction(radius),) * 2
    count = 0
    for x in nodes:
        v = [Fraction(float(t)) - p for t, p in zip(x, p0)]
        t = sum(vi * ai for vi, ai in zip(v, a)) / aa
        if not 0 <= t <= 1:
            continue
        dist2 = sum(vi * vi for vi in v) - t * t * aa
        rad = r0 + t * (r1 - r0)
        count += (dist2 == rad * rad) or (t in (0, 1) and dist2 <= rad * rad)
    return count


def main():
    from sparseSpatialSampling.geometry import CubeGeometry, CylinderGeometry3D, SphereGeometry
    out, wrong, rng = {}, {}, np.random.default_rng(2024)
    cells = {d: curved_cells(d) for d in (2, 3)}
    nodes = {d: cell_nodes(*cells[d]) for d in (2, 3)}
    uniq = {d: lattice_nodes(d) for d in (2, 3)}
    assert len(uniq[2]) == 17 ** 2 and len(uniq[3]) == 17 ** 3
    for d in (2, 3):
        out[f"center{d}"], out[f"level{d}"] = cells[d][0], cells[d][1]
    out["width"] = np.array(cells[2][2])

    # ---- spheres -------------------------------------------------------------------------------------------------------------------
    for d, n_diff, n_same in ((2, 10, 2), (3, 5, 1)):
        key = f"sphere{d}"
        bodies = [(list(p), float(r), 0) for p, r in CURVED_EXACT[key]]
        on = [on_sphere(uniq[d], p, r) for p, r, _ in bodies]
        assert min(on) >= MIN_ON_SURFACE, (key, on)
        pos = CURVED_GENERIC[key]
        d_seq = seq_sphere_dist(uniq[d], pos)
        cand = np.flatnonzero((d_seq > 0.2) & (d_seq < (1.1 if d == 2 else 0.8)))
        picked = choose(rng, uniq[d][cand], d_seq[cand],
                        lambda x, g: ref_threshold(lambda r: (lambda ki: SphereGeometry("g", ki, list(pos), r)), x, g), n_diff, n_same)
        for x, d_ref in picked:
            took = [ref_takes(lambda ki, r=r: SphereGeometry("g", ki, list(pos), r), x) for r in around(d_ref)]
            assert took == [False, True, True]
            bodies += [(list(pos), r, 1) for r in around(d_ref)]
        bits = np.stack([ref_bits(lambda ki, p=p, r=r: SphereGeometry("g", ki, p, r), nodes[d]) for p, r, _ in bodies])
        seq = np.stack([verdict_bits(seq_sphere_dist(nodes[d], p) <= r) for p, r, _ in bodies])
        wrong[key] = int(np.count_nonzero(bits != seq))
        assert np.array_equal(bits[:len(on)], seq[:len(on)]), "exact bodies: every evaluation order agrees"
        out.update({f"{key}_pos": np.array([b[0] for b in bodies]), f"{key}_radius": np.array([b[1] for b in bodies]),
                    f"{key}_ulp": np.array([b[2] for b in bodies], dtype=np.uint8), f"{key}_bits": bits,
                    f"{key}_on_surface": np.array(on), f"{key}_node": np.array([x for x, _ in picked])})

    # ---- cylinders and cones: one table, family 0 exact, 1 radius, 2 cap, 3 cone ------------------------------------------------------
    def cyl(position, radius):
        return lambda ki: CylinderGeometry3D("g", ki, [tuple(p) for p in position], radius)

    def axis_distance(position, x, guess):
        return ref_threshold(lambda r: cyl(position, r), x, guess)

    bodies = [(p, r, 0) for p, r in CURVED_EXACT["cyl"] + CURVED_EXACT["cone"]]
    on = [on_cylinder(uniq[3], p, r) for p, r, _ in bodies]
    assert min(on) >= MIN_ON_SURFACE, on
    chosen = []

    position = CURVED_GENERIC["cyl"]                                      # radius ties
    nd, proj, norm = seq_cylinder(uniq[3], position)
    cand = np.flatnonzero((proj > 0.15 * norm) & (proj < 0.85 * norm) & (nd > 0.25) & (nd < 0.6))
    for x, d_ref in choose(rng, uniq[3][cand], nd[cand], lambda x, g: axis_distance(position, x, g), 5, 1):
        assert [ref_takes(cyl(position, r), x) for r in around(d_ref)] == [False, True, True]
        bodies += [(position, r, 1) for r in around(d_ref)]
        chosen.append(x)

    # cap ties: axes of few bits whose fl(N / fl(sqrt N)) is below / on / above fl(sqrt N); rim node x, start point p0 = x - w - a with
    # w.a = 0 exactly, w a multiple of 2^-24, chosen so that the reference's distance of x differs from the plain one
    axes = {}
    for a0 in range(-41, 42, 2):
        for a1 in range(-41, 42, 2):
            a = np.array([a0, a1, 32.0]) / 64.0
            n2 = float(a @ a)
            s = float(np.sqrt(n2))
            if a0 and a1 and abs(a0) != abs(a1) and round(s * 64) != s * 64:
                axes.setdefault(int(np.sign(n2 / s - s)), a)
    assert sorted(axes) == [-1, 0, 1], sorted(axes)
    interior = uniq[3][np.all((uniq[3] > 0.0) & (uniq[3] < 1.0), axis=1)]
    for side in (-1, 0, 1, -1, 0, -1, 0):
        a = axes[side]
        for _ in range(50000):
            x = interior[rng.integers(len(interior))]
            w01 = rng.integers(-2 ** 18, 2 ** 18, 2) / 2.0 ** 19
            w = np.array([w01[0], w01[1], -(a[0] * w01[0] + a[1] * w01[1]) / a[2]])
            p1 = x - w
            p0 = p1 - a
            position = [tuple(p0.tolist()), tuple(p1.tolist())]
            exact = all(Fraction(float(t)) == Fraction(float(np.float32(t))) for t in (*p0, *p1))
            radial = float(np.sqrt(w @ w))
            if not exact or not 0.25 < radial < 0.5:
                continue
            nd_x, proj_x, norm = seq_cylinder(x, position)
            assert (np.float32(p1) - np.float32(p0)).astype(np.float64).tolist() == a.tolist()
            assert int(np.sign(proj_x - norm)) == side and abs(proj_x - norm) <= np.spacing(norm)
            if side > 0:                       # beyond the end plane for the reference: its distance there decides nothing
                d_ref = float(nd_x)
                break
            d_ref = axis_distance(position, x, float(nd_x))
            if d_ref != float(nd_x):
                break
        else:
            raise AssertionError("no rim node found")
        took = [ref_takes(cyl(position, r), x) for r in around(d_ref)]
        assert took == ([False, True, True] if side <= 0 else [False, False, False]), (side, took)
        bodies += [(position, r, 2) for r in around(d_ref)]
        chosen.append(x)

    position, r1 = CURVED_GENERIC["cone"], CURVED_GENERIC["cone_r1"]     # local-radius ties of a cone
    nd, proj, norm = seq_cylinder(uniq[3], position)
    # (start radius below 1 and |t * (r1 - r0)| below 1/2: every double near d can then be met by the interpolation)
    cand = np.flatnonzero((proj > 0.15 * norm) & (proj < 0.6 * norm) & (nd > 0.25) & (nd < 0.45))
    idx_of = {tuple(x): i for i, x in enumerate(uniq[3])}
    for x, d_ref in choose(rng, uniq[3][cand], nd[cand], lambda x, g: axis_distance(position, x, g), 5, 1):
        t = proj[idx_of[tuple(x)]] / norm
        for target in around(d_ref):
            for k in range(4096):                                 # (not every local radius is met with a given far radius)
                r1k = float(r1 + k * np.spacing(r1))
                r0 = (target - t * r1k) / (1.0 - t)
                span = r0 + np.arange(-400, 401) * np.spacing(r0)
                hit = span[span + t * (r1k - span) == target]
                if len(hit):
                    break
            assert len(hit), "no pair of radii gives the local radius wanted"
            bodies.append((position, [float(hit[0]), r1k], 3))
        took = [ref_takes(cyl(position, b[1]), x) for b in bodies[-3:]]
        assert took == [False, True, True], took
        chosen.append(x)

    bits = np.stack([ref_bits(cyl(p, r), nodes[3]) for p, r, _ in bodies])
    seq = np.stack([verdict_bits(seq_cylinder_inside(nodes[3], p, r)) for p, r, _ in bodies])
    family = np.array([b[2] for b in bodies], dtype=np.uint8)
    assert np.array_equal(bits[family == 0], seq[family == 0]), "exact bodies: every evaluation order agrees"
    for name, f in (("cyl_radius", 1), ("cyl_cap", 2), ("cone", 3)):
        wrong[name] = int(np.count_nonzero(bits[family == f] != seq[family == f]))
    out.update({"cyl_pos": np.array([b[0] for b in bodies], dtype=np.float64),
                "cyl_radius": np.array([b[1] if isinstance(b[1], list) else [b[1], b[1]] for b in bodies]),
                "cyl_cone": np.array([isinstance(b[1], list) for b in bodies]), "cyl_family": family, "cyl_bits": bits,
                "cyl_on_surface": np.array(on), "cyl_node": np.array(chosen)})

    # ---- boxes ---------------------------------------------------------------------------------------------------------------------
    for d in (2, 3):
        out[f"box{d}_lo"] = np.array([lo for lo, _ in CURVED_BOXES[d]])
        out[f"box{d}_hi"] = np.array([hi for _, hi in CURVED_BOXES[d]])
        out[f"box{d}_bits"] = np.stack([ref_bits(lambda ki, lo=lo, hi=hi: CubeGeometry("g", ki, list(lo), list(hi)), nodes[d])
                                        for lo, hi in CURVED_BOXES[d]])

    print("cell verdicts the sequential evaluation gets wrong:", wrong)
    assert all(v >= MIN_WRONG for v in wrong.values()), wrong
    for k, v in wrong.items():
        out[f"seq_wrong_{k}"] = np.array(v)
    out["torch_version"] = np.array(pt.__version__)
    out["cpu_capability"] = np.array(pt.backends.cpu.get_cpu_capability())
    path = os.path.join(HERE, "masks_curved.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
