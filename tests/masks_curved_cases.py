"""The bodies of tests/golden/masks_curved.npz (gen_masks_curved.py) as the tests use them: one record per body with the
reference's verdict byte per cell (bit ``2 * keep_inside + refine_mode``).  Loaded once and shared; nothing here is changed by a
test."""
import os
from functools import lru_cache

import numpy as np

from inputs import cell_nodes, curved_cells

MODES = [(ki, rm) for ki in (0, 1) for rm in (0, 1)]
FAMILIES = ("sphere2", "sphere3", "cyl_radius", "cyl_cap", "cone")
CYL_FAMILY = {0: "exact", 1: "cyl_radius", 2: "cyl_cap", 3: "cone"}


class Body:
    def __init__(self, name, kind, dim, args, bits, family, nodes):
        self.name, self.kind, self.dim, self.args, self.bits, self.family, self.nodes = name, kind, dim, args, bits, family, nodes

    def want(self, ki, rm):
        """the reference's verdict per cell for one mode pair, as the kernel's bytes"""
        return (self.bits >> (2 * ki + rm)) & 1

    def __repr__(self):
        return self.name


@lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "masks_curved.npz"))
    return {k: z[k] for k in z.files}


@lru_cache(maxsize=None)
def cells(dim):
    """(centre, level, width) of the fixture's lattice -- the fixture stores what ``inputs.curved_cells`` builds"""
    z = fixture()
    center, level, width = curved_cells(dim)
    assert np.array_equal(center, z[f"center{dim}"]) and np.array_equal(level, z[f"level{dim}"]) and width == float(z["width"])
    return center, level, width


@lru_cache(maxsize=None)
def bodies():
    z, out = fixture(), []
    for d in (2, 3):
        key = f"sphere{d}"
        for i, (pos, r, ulp) in enumerate(zip(z[key + "_pos"], z[key + "_radius"], z[key + "_ulp"])):
            out.append(Body(f"{key}[{i}] centre {pos.tolist()} radius {float(r)!r}", "sphere", d, (pos.tolist(), float(r)),
                            z[key + "_bits"][i], key if ulp else "exact", z[key + "_node"]))
    for i, (pos, rad, cone, fam) in enumerate(zip(z["cyl_pos"], z["cyl_radius"], z["cyl_cone"], z["cyl_family"])):
        position = [tuple(p) for p in pos.tolist()]
        radius = [float(rad[0]), float(rad[1])] if cone else float(rad[0])
        out.append(Body(f"{'cone' if cone else 'cylinder'}[{i}] {position} radius {radius!r}", "cylinder", 3, (position, radius),
                        z["cyl_bits"][i], CYL_FAMILY[int(fam)], z["cyl_node"]))
    for d in (2, 3):
        for i, (lo, hi) in enumerate(zip(z[f"box{d}_lo"], z[f"box{d}_hi"])):
            out.append(Body(f"box{d}[{i}] {lo.tolist()} .. {hi.tolist()}", "box", d, (lo.tolist(), hi.tolist()),
                            z[f"box{d}_bits"][i], "box", np.zeros((0, d))))
    return tuple(out)


def first_of(family):
    """the one-ulp tie body of a family whose radius equals the reference's distance (the middle one of the first triple)"""
    return [b for b in bodies() if b.family == family][1]


def differing(got, want, limit=8):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return f"{len(bad)} cells differ, first {bad[:limit].tolist()}: got {np.asarray(got)[bad[:limit]].tolist()}"


def nodes_of(dim):
    return cell_nodes(*cells(dim))
