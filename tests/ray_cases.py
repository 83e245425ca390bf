"""
Cases and references for the line-of-sight integrals of csrc/rays.hip (CPU only: numpy, long double).

Grids: the cases of tests/sample_cases.py (``GRIDS``).  Rays: ``family(grid, name)`` -> (origins [NR, d], dirs [NR, d], t_range):

    chords      random chords between points in and around the lattice domain, the whole line
    axis        axis-parallel rays with one or two zero components; half of the fixed coordinates lie exactly ON lattice planes (faces and
                edges of leaves, the lower and the upper bound of the domain among them), the others at dyadic fractions of a lattice cell;
                directions +-1/2, +-1, +-2: on the dyadic grids every operation on them is exact
    diagonal    rays through corners of leaves along diagonals (d = +-1 per axis; in 3-D a third of them face diagonals), exact on the
                dyadic grids too
    miss        four rays in five pass outside the domain or point away from it
    clipped     t_range = (0, 1) of chords from point to point: the ends lie inside the domain, a third of them inside holes
    scaled      chords with directions scaled by 10^-6 .. 10^6
    hostile     chords with NaN, +-inf, 10^300 and zero directions planted in two rays out of five

References:

    ray_oracle      long double, NO walk: per ray and leaf the chord by the slab test on the leaf's lattice planes, by brute force over
                    all leaves; the half-open index rule of the definition on the axes with d_a = 0; CELL: sum value x chord; LINEAR:
                    the blend integrated per chord with THREE Gauss points (exact for degree <= 5, independent of the kernel's two)
    emulate_rays    the definition of include/s3rays.h in plain float64 numpy (the walk), with the planted mistakes ``MISTAKES``
"""
import functools
import zlib

import numpy as np

from tests import sample_cases as sc

LD = np.longdouble
NR = 3001               # twelve workgroups of 256 lanes at one column, the last one ragged
GRIDS = ["tree2d", "tree3d", "dyadic2d", "dyadic3d", "offset2d", "one_cell", "level3", "chain2d", "chain3d"]
FAMILIES = ["chords", "axis", "diagonal", "miss", "clipped", "scaled", "hostile"]
RANDOM_FAMILIES = ["chords", "miss", "clipped", "scaled", "hostile"]
DYADIC_EXACT = [(g, f) for g in ("dyadic2d", "dyadic3d") for f in ("axis", "diagonal")]
STATUS = {"CROSSED": 0, "MISSED": 1, "BAD_RAY": 2, "TRUNCATED": 3, "BROKEN": 4}
MISTAKES = ["closed", "stop_at_empty", "midpoint", "no_norm", "nearest", "no_trange", "centre_planes"]
GAUSS2 = 0.57735026918962576
CLEAR = 1e-9            # counts are compared where no leaf's chord is within CLEAR x the domain's chord of zero
N_COL = 3               # columns of the reference fields


def fma(a, b, c):
    """a * b + c rounded once to float64 (formed in long double, whose 64-bit significand leaves the one rounding all but alone)"""
    with np.errstate(all="ignore"):
        return (np.asarray(a).astype(LD) * np.asarray(b).astype(LD) + np.asarray(c).astype(LD)).astype(np.float64)


# ---- grids --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice(name):
    """the grid with its index: anchors and sizes in lattice cells, the sorted ranges, the lattice"""
    c = sc.case(name)
    ix = sc.emulate_index(c)
    assert not ix["refused"].any()
    h = sc.cell_sizes(c)
    anchors = np.rint(((c["centers"] - h[:, None] / 2) - ix["origin"]) / ix["h_min"]).astype(np.int64)
    size = np.int64(1) << (ix["depth"] - c["levels"].astype(np.int64))
    return {"case": c, "dim": c["centers"].shape[1], "depth": int(ix["depth"]), "origin": ix["origin"], "h_min": float(ix["h_min"]),
            "starts": ix["starts"], "ends": ix["ends"], "ids": ix["ids"].astype(np.int64), "anchors": anchors, "size": size,
            "n_cells": len(anchors), "n_nodes": len(c["nodes"])}


@functools.lru_cache(maxsize=None)
def fields(name, integers=False):
    """(cell field [n_cells, N_COL], node field [n_nodes, N_COL]) float64 holding float32 values (``integers``: small integers)"""
    g = lattice(name)
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 5)
    if integers:
        make = lambda n: rng.integers(-4, 5, size=(n, N_COL)).astype(np.float64)          # noqa: E731
    else:
        make = lambda n: rng.standard_normal((n, N_COL)).astype(np.float32).astype(np.float64)      # noqa: E731
    return make(g["n_cells"]), make(g["n_nodes"])


def hole_points(g, rng, n):
    """points of the lattice domain that no leaf holds (fewer than n, none, where the grid has few holes)"""
    ext = 1 << g["depth"]
    q = g["origin"] + (rng.integers(0, ext, size=(4 * n, g["dim"])) + 0.5) * g["h_min"]
    return q[sc.emulate_locate(g["case"], q) < 0][:n]


# ---- rays ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family(name, fam, n=NR):
    g = lattice(name)
    dim, depth, origin, h = g["dim"], g["depth"], g["origin"], g["h_min"]
    ext = 1 << depth
    lo, size = origin, ext * h
    rng = np.random.default_rng(zlib.crc32((name + fam).encode()))
    t_range = (-np.inf, np.inf)

    def around(k):
        return lo + size * rng.uniform(-0.3, 1.3, size=(k, dim))

    def chords(k):
        p0, p1 = around(k), around(k)
        return p0, p1 - p0

    def lattice_coord(k, on_plane):
        """origin + (j + f) h: j uniform over the domain and a little beyond, or log-distributed towards the lower corner"""
        j = rng.integers(-ext // 4 - 1, ext + ext // 4 + 2, size=k)
        log = rng.random(k) < 0.5
        j = np.where(log, np.floor(2.0 ** (rng.random(k) * depth)).astype(np.int64) - (rng.random(k) < 0.2), j)
        j = np.where(rng.random(k) < 0.04, rng.choice([0, ext], size=k), j)                 # the bounds of the domain
        f = np.where(on_plane, 0.0, rng.choice([0.25, 0.5, 0.75], size=k))
        return (j + f) * h

    if fam in ("chords", "scaled", "hostile", "miss", "clipped"):
        o, d = chords(n)
    if fam == "scaled":
        d = d * 10.0 ** rng.uniform(-6, 6, size=(n, 1))
    elif fam == "clipped":
        t_range = (0.0, 1.0)
        inner = lo + size * rng.uniform(0.02, 0.98, size=(n, dim))
        holes = hole_points(g, rng, n // 3)
        inner[:len(holes)] = holes
        d = inner - o
    elif fam == "miss":
        k = n - n // 5
        ax = rng.integers(0, dim, size=k)
        side = rng.random(k) < 0.5
        o[np.arange(k), ax] = np.where(side, lo[ax] - size * rng.uniform(0.05, 1.0, size=k), lo[ax] + size * rng.uniform(1.05, 2.0, size=k))
        away = np.where(side, -1.0, 1.0) * rng.uniform(0.0, 1.0, size=k) * (rng.random(k) < 0.6)        # zero: parallel, outside
        d[np.arange(k), ax] = away
    elif fam == "hostile":
        k = 2 * n // 5
        what = rng.integers(0, 7, size=k)
        ax = rng.integers(0, dim, size=k)
        r = np.arange(k)
        for code, (arr, value) in enumerate([(o, np.nan), (d, np.nan), (o, np.inf), (d, -np.inf), (o, -1e300), (d, 1e300)]):
            m = what == code
            arr[r[m], ax[m]] = value
        d[r[what == 6]] = 0.0
    elif fam == "axis":
        o = np.empty((n, dim))
        d = np.zeros((n, dim))
        for a in range(dim):
            o[:, a] = lo[a] + lattice_coord(n, rng.random(n) < 0.5)
        n_moving = np.ones(n, dtype=np.int64) if dim == 2 else rng.integers(1, 3, size=n)
        first = rng.integers(0, dim, size=n)
        for m in range(2):
            a = (first + m) % dim
            sel = n_moving > m
            d[np.arange(n)[sel], a[sel]] = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], size=int(sel.sum()))
        o[:24] = lo + (np.arange(24)[:, None] % 3 + np.array([0.0, 0.5, 0.25])[:dim]) * h      # the finest cells of a chain, and the corner cell
        d[:24] = 0.0
        d[np.arange(24), np.arange(24) % dim] = np.where(np.arange(24) % 2, 1.0, -2.0)
    elif fam == "diagonal":
        cell = rng.integers(0, g["n_cells"], size=n)
        corner = g["anchors"][cell] + g["size"][cell][:, None] * rng.integers(0, 2, size=(n, dim))
        shift = rng.integers(-3, 4, size=(n, 1)) * g["size"][cell][:, None]               # along the diagonal: the ray, not its origin, is what counts
        d = rng.choice([-1.0, 1.0], size=(n, dim))
        if dim == 3:
            flat = rng.random(n) < 0.33
            d[np.arange(n)[flat], rng.integers(0, 3, size=n)[flat]] = 0.0
        o = lo + (corner + shift * d) * h
    else:
        assert fam in FAMILIES, fam
    o, d = np.ascontiguousarray(o, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64)
    o.setflags(write=False), d.setflags(write=False)
    return o, d, t_range


# ---- the oracle: long double, no walk ---------------------------------------------------------------------------------------------
def ray_oracle(name, o, d, t_range, cell_field=None, node_field=None, chunk=128):
    """-> dict: ``cell`` / ``linear`` LD [R, C] (NaN for bad rays), ``length`` LD [R], ``segments``, ``status``, ``norm`` LD (|d|), ``D``
    (the larger |t| at the domain's entry and exit; 0 where the line misses it), ``P`` (max over the moving axes of X_a / |d_a|, X_a the
    largest |coordinate| of the domain: what the rounding of a plane's own coordinate is in units of t), ``linmag`` LD [R, C] (the integral of sum_m |w_m f_m|:
    what the blend's rounding scales with), ``cell_t`` / ``length_t`` (the same in units of t, before |d|), ``unclear`` (a leaf's chord is within CLEAR x the
    domain's chord, or within 64 roundings of a parameter, of zero: the ray grazes it and the counts are not compared),
    ``jumps`` (changes of level between consecutive segments), ``hole`` (length of the ray inside the domain but in no leaf, in units
    of t) and ``finest`` (segments in cells of the deepest level)"""
    g = lattice(name)
    c, dim, depth = g["case"], g["dim"], g["depth"]
    origin, h_min = g["origin"].astype(LD), LD(g["h_min"])
    ext = 1 << depth
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    n_rays, n = len(o), g["n_cells"]
    p_lo = origin + g["anchors"].astype(LD) * h_min                                      # [n, dim]
    p_hi = origin + (g["anchors"] + g["size"][:, None]).astype(LD) * h_min
    levels = c["levels"].astype(np.int64)
    t_min, t_max = LD(t_range[0]), LD(t_range[1])
    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (d != 0).any(axis=1))
        fixed_q = np.floor((o - g["origin"]) / g["h_min"])                              # the index rule of the definition, in float64
    fixed_ok = (fixed_q >= 0) & (fixed_q < ext)
    fixed_i = np.where(fixed_ok, fixed_q, -1).astype(np.int64)
    n_col = 0 if cell_field is None else cell_field.shape[1]
    out = {"cell": np.full((n_rays, n_col), np.nan, dtype=LD), "linear": np.full((n_rays, n_col), np.nan, dtype=LD),
           "linmag": np.zeros((n_rays, n_col), dtype=LD), "length": np.zeros(n_rays, dtype=LD), "length_t": np.zeros(n_rays, dtype=LD),
           "cell_t": np.zeros((n_rays, n_col), dtype=LD), "segments": np.zeros(n_rays, dtype=np.int64),
           "norm": np.zeros(n_rays, dtype=LD), "D": np.zeros(n_rays), "P": np.zeros(n_rays), "unclear": np.zeros(n_rays, dtype=bool),
           "jumps": np.zeros(n_rays, dtype=np.int64), "hole": np.zeros(n_rays), "finest": np.zeros(n_rays, dtype=np.int64)}
    signs = sc.corner_signs(dim)
    gauss = [(-np.sqrt(LD(3) / 5), LD(5) / 9), (LD(0), LD(8) / 9), (np.sqrt(LD(3) / 5), LD(5) / 9)]
    good = np.flatnonzero(~bad)
    for s0 in range(0, len(good), chunk):
        rows = good[s0:s0 + chunk]
        oo, dd = o[rows].astype(LD), d[rows].astype(LD)
        k = len(rows)
        t_in, t_out = np.full((k, n), t_min), np.full((k, n), t_max)
        dom_in, dom_out = np.full(k, -np.inf, dtype=LD), np.full(k, np.inf, dtype=LD)
        admit = np.ones((k, n), dtype=bool)
        with np.errstate(all="ignore"):
            for a in range(dim):
                mv = d[rows, a] != 0
                da = np.where(mv, dd[:, a], 1)[:, None]
                t0, t1 = (p_lo[None, :, a] - oo[:, a:a + 1]) / da, (p_hi[None, :, a] - oo[:, a:a + 1]) / da
                tn, tf = np.minimum(t0, t1), np.maximum(t0, t1)
                t_in = np.where(mv[:, None], np.maximum(t_in, tn), t_in)
                t_out = np.where(mv[:, None], np.minimum(t_out, tf), t_out)
                fi = fixed_i[rows, a][:, None]
                admit &= mv[:, None] | ((fi >= g["anchors"][None, :, a]) & (fi < (g["anchors"][:, a] + g["size"])[None]))
                e0, e1 = (origin[a] - oo[:, a]) / da[:, 0], (origin[a] + ext * h_min - oo[:, a]) / da[:, 0]
                dom_in = np.where(mv, np.maximum(dom_in, np.minimum(e0, e1)), dom_in)
                dom_out = np.where(mv, np.minimum(dom_out, np.maximum(e0, e1)), dom_out)
            length = np.where(admit, t_out - t_in, -np.inf)
            seg = length > 0
            in_dom = (fixed_ok[rows] | (d[rows] != 0)).all(axis=1) & (dom_out > dom_in)
            dom_len = np.where(in_dom, np.minimum(dom_out, t_max) - np.maximum(dom_in, t_min), 0)
            dom_len = np.where(dom_len > 0, dom_len, 0)
            big = np.maximum(np.abs(np.maximum(dom_in, t_min)), np.abs(np.minimum(dom_out, t_max)))
            out["D"][rows] = np.where(in_dom & np.isfinite(big), big, 0).astype(np.float64)
            norm = np.sqrt((dd * dd).sum(axis=1))
            reach = np.maximum(np.abs(g["origin"]), np.abs(g["origin"] + ext * g["h_min"]))
            out["P"][rows] = np.where(d[rows] != 0, reach[None] / np.abs(d[rows]), 0).max(axis=1)
        seg_len = np.where(seg, length, 0)
        out["norm"][rows] = norm
        out["length"][rows] = norm * seg_len.sum(axis=1)
        out["segments"][rows] = seg.sum(axis=1)
        out["hole"][rows] = (dom_len - seg_len.sum(axis=1)).astype(np.float64)
        blur = np.maximum(CLEAR * dom_len, 64 * LD(2) ** -53 * (out["D"][rows] + out["P"][rows]))
        out["unclear"][rows] = (admit & (np.abs(length) <= blur[:, None])).any(axis=1)
        out["length_t"][rows] = seg_len.sum(axis=1)
        out["finest"][rows] = (seg & (levels == depth)[None]).sum(axis=1)
        order = np.argsort(np.where(seg, t_in, np.inf), axis=1, kind="stable")
        lv = np.take_along_axis(np.broadcast_to(levels, (k, n)), order, axis=1)
        n_seg = seg.sum(axis=1)
        out["jumps"][rows] = ((lv[:, 1:] != lv[:, :-1]) & (np.arange(1, n)[None] < n_seg[:, None])).sum(axis=1) if n > 1 else 0
        if cell_field is not None:
            out["cell_t"][rows] = seg_len @ cell_field.astype(LD)
            out["cell"][rows] = norm[:, None] * out["cell_t"][rows]
        if node_field is not None:
            r, j = np.nonzero(seg)
            half = length[r, j] / 2
            mid = t_in[r, j] + half
            total, mag = np.zeros((len(r), n_col), dtype=LD), np.zeros((len(r), n_col), dtype=LD)
            f = node_field[c["faces"][j]].astype(LD)                                    # [s, 2^d, C]
            edge = (p_hi[j, 0] - p_lo[j, 0])[:, None]
            for x_g, w_g in gauss:
                x = oo[r] + (mid + half * x_g)[:, None] * dd[r]
                xi = np.clip((x - p_lo[j]) / edge, 0, 1)
                w = np.ones((len(r), 1 << dim), dtype=LD)
                for a in range(dim):
                    w = w * np.where(signs[None, :, a] > 0, xi[:, a:a + 1], 1 - xi[:, a:a + 1])
                total += w_g * (w[:, :, None] * f).sum(axis=1)
                mag = np.maximum(mag, np.abs(w[:, :, None] * f).sum(axis=1))
            lin, linmag = np.zeros((k, n_col), dtype=LD), np.zeros((k, n_col), dtype=LD)
            np.add.at(lin, r, half[:, None] * total)
            np.add.at(linmag, r, length[r, j][:, None] * mag)
            out["linear"][rows] = norm[:, None] * lin
            out["linmag"][rows] = norm[:, None] * linmag
    out["status"] = np.where(bad, STATUS["BAD_RAY"], np.where(out["segments"] > 0, STATUS["CROSSED"], STATUS["MISSED"])).astype(np.int32)
    return out


@functools.lru_cache(maxsize=None)
def truth(name, fam, integers=False):
    """the oracle of a (grid, family) for ``fields(name, integers)``, computed once and shared"""
    o, d, t_range = family(name, fam)
    cell, node = fields(name, integers)
    return ray_oracle(name, o, d, t_range, cell, node)


def overflows(d):
    """rays whose |d| is not finite in float64 though every component is (10^300): by the definition's arithmetic their results are
    inf or NaN, which no oracle in another precision shares; they are held to the emulation"""
    with np.errstate(all="ignore"):
        return np.isfinite(d).all(axis=1) & ~np.isfinite(np.sqrt((d * d).sum(axis=1)))


def exact_expectation(ref, d):
    """dyadic rays on dyadic grids with small-integer cell fields: every operation before the last is exact, so the bits are those of
    the float64 |d| times the oracle's sums in units of t -> (out f64 [R, C], length f64 [R])"""
    s2 = d[:, 0] * d[:, 0]
    for a in range(1, d.shape[1]):
        s2 = s2 + d[:, a] * d[:, a]
    scale = np.where(ref["segments"] > 0, np.sqrt(s2), 0.0)
    return scale[:, None] * ref["cell_t"].astype(np.float64), scale * ref["length_t"].astype(np.float64)


def size_bound(ref, vmax, k_factor, mode, dim):
    """K * 2^-53 * segments * (D + P) * |d| * max|v| (+ the blend's own rounding, ``sample_cases.linear_bound``, integrated along the
    ray, in LINEAR mode) per ray and column, long double [R, C].  Every segment has two plane parameters; each carries the roundings of
    ``(plane - o_a) / d_a``, relative to |t| <= D, and the rounding of the plane's own coordinate ``fma(j, h_min, origin_a)``, at most
    2^-53 X_a, which is 2^-53 X_a / |d_a| <= 2^-53 P in units of t whatever D is: a parameter that is off moves that much length from a
    cell to its neighbour.  (Without P the bound cannot hold for a short chord far from the coordinate origin: a ray that clips the
    refined corner of a chain has D |d| of the order of h_min = 3e-10 and planes at 0.137 known to 1.4e-17.)"""
    core = LD(k_factor) * LD(2) ** -53 * (ref["segments"] * (ref["D"] + ref["P"])).astype(LD) * ref["norm"]
    bound = core[:, None] * np.asarray(vmax, dtype=LD)[None, :]
    if mode == "linear":
        bound = bound + LD(k_factor) * sc.linear_bound(dim, ref["linmag"])
    return bound


K_EMULATION = 2         # what the emulation needs against the oracle, measured: 1.25 (tests/test_ray_checker.py)
GPU_FACTOR = 8          # the GPU tests allow GPU_FACTOR x K_EMULATION: a legal difference in evaluation order
MAX_STEPS = 4000        # blocks a ray of these grids may visit: a chain of depth 31 takes a few dozen


def length_bound(ref, k_factor):
    return LD(k_factor) * LD(2) ** -53 * (ref["segments"] * (ref["D"] + ref["P"])).astype(LD) * ref["norm"]


def compare(name, fam, got, mode, field, k_factor):
    """-> (rays beyond the bound in out, in length, with a wrong count or status among the clear rays, clear rays, worst K needed)"""
    g = lattice(name)
    o, d, _ = family(name, fam)
    ref = truth(name, fam)
    keep = ~overflows(d)
    unit = size_bound(ref, np.abs(field).max(axis=0), 1, mode, g["dim"])
    err = np.abs(got["out"].astype(LD) - ref[mode])
    nan_differs = np.isnan(got["out"]) != np.isnan(ref[mode].astype(np.float64))
    with np.errstate(all="ignore"):
        need = np.where(unit > 0, err / unit, np.where(err == 0, 0, np.inf))
    need = np.where(np.isnan(ref[mode].astype(np.float64)), 0, need)
    size = ((need > k_factor) | nan_differs)[keep].any(axis=1)
    length = (np.abs(got["length"].astype(LD) - ref["length"]) > length_bound(ref, k_factor))[keep]
    clear = (~ref["unclear"] | ((name, fam) in DYADIC_EXACT)) & keep
    counts = ((got["segments"] != ref["segments"]) | (got["status"] != ref["status"]))[clear]
    return int(size.sum()), int(length.sum()), int(counts.sum()), int(clear.sum()), float(need[keep].max())


# ---- the definition in float64 ------------------------------------------------------------------------------------------------
def emulate_rays(name, o, d, t_range, field, mode="cell", max_steps=1 << 20, mistake=None):
    """include/s3rays.h operation by operation (well-formed grids: BROKEN does not occur) -> dict(out f64 [R, C], length, segments,
    status, steps: blocks visited).  ``mistake``: one of ``MISTAKES``"""
    assert mistake is None or mistake in MISTAKES
    g = lattice(name)
    c, dim, depth, origin, h_min = g["case"], g["dim"], g["depth"], g["origin"], g["h_min"]
    starts, ends, ids, n = g["starts"], g["ends"], g["ids"], g["n_cells"]
    levels = c["levels"].astype(np.int64)
    ext = 1 << depth
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    field = np.asarray(field).astype(np.float64)
    n_rays, n_col = len(o), field.shape[1]
    t_min, t_max = (-np.inf, np.inf) if mistake == "no_trange" else (float(t_range[0]), float(t_range[1]))
    signs = sc.corner_signs(dim)
    cell_h = sc.cell_sizes(c)
    mv = d != 0

    def tau_of(plane, rows, a):
        return (plane - o[rows, a]) / d[rows, a]

    def lattice_plane(j, a):
        return fma(j.astype(np.float64), h_min, origin[a])

    def chord(rows, p_lo, p_hi):
        """t_in, t_out, e of the blocks with the planes p_lo, p_hi [k, dim]"""
        k = len(rows)
        t_in, t_out, e = np.full(k, t_min), np.zeros(k), np.full(k, -1)
        for a in range(dim):
            pos = d[rows, a] > 0
            tn, tf = tau_of(np.where(pos, p_lo[:, a], p_hi[:, a]), rows, a), tau_of(np.where(pos, p_hi[:, a], p_lo[:, a]), rows, a)
            up = mv[rows, a] & (tn > t_in)
            t_in = np.where(up, tn, t_in)
            up = mv[rows, a] & ((e < 0) | (tf < t_out))
            t_out, e = np.where(up, tf, t_out), np.where(up, a, e)
        return t_in, t_out, e

    def point_index(rows, a, t, lo, hi):
        q = np.floor((fma(t, d[rows, a], o[rows, a]) - origin[a]) / h_min)
        return np.where(q >= lo, np.minimum(q, hi), lo).astype(np.int64)

    def blend(rows, cid, t_g):
        """the blend of the node field at x(t_g) in the leaves cid"""
        h = cell_h[cid]
        xi = np.empty((len(rows), dim))
        for a in range(dim):
            x = np.where(mv[rows, a], fma(t_g, d[rows, a], o[rows, a]), o[rows, a])
            xi[:, a] = np.minimum(np.maximum((x - (c["centers"][cid, a] - h / 2)) / h, 0.0), 1.0)
        b = np.zeros((len(rows), n_col))
        for m in range(1 << dim):
            w = xi[:, 0] if signs[m, 0] > 0 else 1.0 - xi[:, 0]
            for a in range(1, dim):
                w = w * xi[:, a] if signs[m, a] > 0 else fma(-xi[:, a], w, w)
            b = fma(w[:, None], field[c["faces"][cid, m]], b)
        return b

    def walk(fixed):
        acc, lenacc = np.zeros((n_rays, n_col)), np.zeros(n_rays)
        segments, steps = np.zeros(n_rays, dtype=np.int64), np.zeros(n_rays, dtype=np.int64)
        every = np.arange(n_rays)
        zero = np.zeros((n_rays, dim), dtype=np.int64)
        planes = lambda idx: np.stack([lattice_plane(idx[:, a], a) for a in range(dim)], axis=1)          # noqa: E731
        t_in, t_out, _ = chord(every, planes(zero), planes(zero + ext))
        started = ok & (np.where(t_max < t_out, t_max, t_out) - t_in > 0)
        i = fixed.copy()
        for a in range(dim):
            tn = tau_of(lattice_plane(np.where(d[:, a] > 0, 0, ext), a), every, a)
            first = np.where(tn == t_in, np.where(d[:, a] > 0, 0, ext - 1), point_index(every, a, t_in, 0, ext - 1))
            i[:, a] = np.where(mv[:, a], first, i[:, a])
        active = started.copy()
        for _ in range(max_steps):
            rows = np.flatnonzero(active)
            if not len(rows):
                break
            ii = i[rows]
            key = sc.morton(ii.astype(np.uint64), dim, depth)
            if mistake == "nearest":
                x = origin + (ii + 0.5) * h_min
                cid = ((x[:, None, :] - c["centers"][None]) ** 2).sum(axis=2).argmin(axis=1)
                leaf = np.ones(len(rows), dtype=bool)
            else:
                pos = np.searchsorted(starts, key, side="right")
                prev = np.maximum(pos - 1, 0)
                g0 = np.where(pos > 0, ends[prev], np.uint64(0))
                leaf = (pos > 0) & (key < g0)
                cid = np.where(leaf, ids[prev], 0)
            s = np.where(leaf, depth - levels[cid], 0)
            if not leaf.all():
                g1 = np.where(pos < n, starts[np.minimum(pos, n - 1)], np.uint64(1) << np.uint64(dim * depth))
                fits = ~leaf
                for s_try in range(1, depth + 1):
                    size = np.uint64(1) << np.uint64(dim * s_try)
                    base = key & ~(size - np.uint64(1))
                    fits = fits & (base >= g0) & (base + size <= g1)
                    s = np.where(fits, s_try, s)
            anchor = (ii >> s[:, None]) << s[:, None]
            p_lo, p_hi = planes(anchor), planes(anchor + (np.int64(1) << s)[:, None])
            if mistake == "centre_planes":
                ctr, half_h = c["centers"][cid], (cell_h[cid] / 2)[:, None]
                p_lo, p_hi = np.where(leaf[:, None], ctr - half_h, p_lo), np.where(leaf[:, None], ctr + half_h, p_hi)
            t_in, t_out, e = chord(rows, p_lo, p_hi)
            length = np.where(t_max < t_out, t_max, t_out) - t_in
            seg = leaf & (length > 0)
            rs, cs, ls, ts = rows[seg], cid[seg], length[seg], t_in[seg]
            if mode == "cell":
                acc[rs] = fma(field[cs], ls[:, None], acc[rs])
            elif mistake == "midpoint":
                acc[rs] = fma(ls[:, None], blend(rs, cs, ts + ls / 2), acc[rs])
            else:
                half = ls / 2
                mid, gp = ts + half, half * GAUSS2
                acc[rs] = fma(half[:, None], blend(rs, cs, mid - gp) + blend(rs, cs, mid + gp), acc[rs])
            lenacc[rs] = lenacc[rs] + ls
            segments[rs] += 1
            steps[rows] += 1
            span = np.int64(1) << s
            a_e = anchor[np.arange(len(rows)), e]
            d_e = d[rows, e]
            done = (t_out >= t_max) | np.where(d_e > 0, a_e + span >= ext, a_e == 0)
            if mistake == "stop_at_empty":
                done |= ~leaf
            active[rows[done]] = False
            go = ~done
            rg, eg = rows[go], e[go]
            for a in range(dim):
                nxt = np.where(eg == a, np.where(d[rg, a] > 0, anchor[go, a] + span[go], anchor[go, a] - 1),
                               point_index(rg, a, t_out[go], anchor[go, a], anchor[go, a] + span[go] - 1))
                i[rg, a] = np.where(mv[rg, a], nxt, i[rg, a])
        return acc, lenacc, segments, started, active, steps

    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & mv.any(axis=1))
        s2 = d[:, 0] * d[:, 0]
        for a in range(1, dim):
            s2 = s2 + d[:, a] * d[:, a]
        norm = np.ones(n_rays) if mistake == "no_norm" else np.sqrt(s2)
        q = np.floor((o - origin) / h_min)
        in_range = (q >= 0) & (q < ext)
        ok = ~bad & (in_range | mv).all(axis=1)
        fixed = np.where(~mv & in_range, q, 0).astype(np.int64)
        acc, lenacc, segments, started, truncated, steps = walk(fixed)
        if mistake == "closed":                                 # the lower cells of a ray that lies in a lattice plane, once more
            on_plane = ~mv & in_range & ((o - origin) / h_min == q) & (q >= 1)
            for a in range(dim):
                lower = fixed.copy()
                lower[:, a] -= 1
                ok_a, ok = ok, ok & on_plane[:, a]
                more = walk(lower)
                ok = ok_a
                acc, lenacc, segments = acc + more[0], lenacc + more[1], segments + more[2]
        scale = np.where(segments > 0, norm, 0.0)
        out = np.where(bad[:, None], np.nan, scale[:, None] * acc)
        status = np.where(bad, STATUS["BAD_RAY"], np.where(truncated, STATUS["TRUNCATED"],
                                                          np.where(segments > 0, STATUS["CROSSED"], STATUS["MISSED"]))).astype(np.int32)
    return {"out": out, "length": scale * lenacc, "segments": segments.astype(np.int32), "status": status, "steps": steps}
