"""
Cases and references for the overlap table of csrc/overlap.hip and the tracks of ``regions.RegionTracks`` (CPU only: numpy and plain
Python; the grids and the label arrays are those of tests/region_cases.py).

References, from integers and the definitions of include/s3overlap.h, none from the code under test:
    units               2^(d (depth - level)) per cell from the integer box sizes, as Python integers (chain3d: up to 2^60)
    reference_overlap   a dict over the cells of every column: (a, b) -> [cells, units]
    brute_overlap       a second opinion, O(n^2): one row of a one-hot matrix per label of A against one per label of B
    reference_tracks    dicts and loops: best edges, mutual links, chains walked one row at a time
and the comparisons the GPU test uses (``check_overlap``, ``check_tracks``), which tests/test_track_checker.py holds against planted
mistakes: units of 1 per cell (``unit_one``), the root rule dropped (``root_rule=False`` on labels with one non-root value planted,
``plant_non_root``), column t against t, src and dst swapped, ties to the larger label (``ties_larger``), a one-sided best edge taken
for a continuation (``one_sided``).

Planted motion on ``uniform2d`` (64 x 64, cell ``x * 64 + y``), ``MOTIONS``: a blob moving one cell per snapshot; two blobs that merge
(8 cells each in the merged one: a tie); the same backwards, one blob that splits; a blob that appears; one that vanishes; all of them in
one scene; one region filling all 4096 cells throughout.  On ``tree2d`` / ``tree3d`` a slab that moves across the random tree, whose
leaves are not balanced: its regions span level jumps of two and more.
"""
import functools

import numpy as np

from tests import region_cases as rc
from tests import sample_cases as sc

T_MOTION = 6
INT_FIELDS = ("src", "dst", "n_cells", "units")


# ---- the overlap table ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def units(name):
    """list of Python integers: the volume of every cell in cells of the finest level"""
    _, sizes, _ = rc.boxes(name)
    d = rc.grid(name)["centers"].shape[1]
    return [int(s) ** d for s in sizes]


@functools.lru_cache(maxsize=None)
def hd(name):
    """the volume of a finest cell as the library forms it: h_min * h_min (* h_min) in float64"""
    h = np.float64(sc.emulate_index(rc.grid(name))["h_min"])
    return h * h if rc.grid(name)["centers"].shape[1] == 2 else (h * h) * h


def is_in(x, root_rule=True):
    """bool like x: the label names a root of its column (``root_rule=False``: the planted mistake label >= 0)"""
    x = np.asarray(x)
    n = len(x)
    ok = (x >= 0) & (x < n)
    if not root_rule:
        return ok
    named = np.take_along_axis(x, np.where(ok, x, 0).astype(np.int64), axis=0)
    return ok & (named == x)


def _table(name, per_column):
    """per column a dict (a, b) -> [cells, units] -> the table as ``hipops.overlap_table`` names it (numpy)"""
    offsets, src, dst, cells, total = [0], [], [], [], []
    for edges in per_column:
        for (a, b), (n, u) in sorted(edges.items()):
            src.append(a), dst.append(b), cells.append(n), total.append(u)
        offsets.append(len(src))
    u64 = np.array(total, dtype=np.uint64)
    return {"offsets": np.asarray(offsets, dtype=np.int64), "src": np.asarray(src, dtype=np.int32), "dst": np.asarray(dst, dtype=np.int32),
            "n_cells": np.asarray(cells, dtype=np.int64), "units": u64.view(np.int64), "volume": u64.astype(np.float64) * hd(name)}


def reference_overlap(name, a, b, unit_one=False, root_rule=True):
    """a, b int32 [n, T] -> the overlap table by the definition.  ``unit_one``, ``root_rule=False``: planted mistakes"""
    a, b = np.asarray(a).reshape(len(a), -1), np.asarray(b).reshape(len(b), -1)
    both = is_in(a, root_rule) & is_in(b, root_rule)
    u = units(name)
    per_column = []
    for t in range(a.shape[1]):
        edges = {}
        for c in np.flatnonzero(both[:, t]):
            e = edges.setdefault((int(a[c, t]), int(b[c, t])), [0, 0])
            e[0] += 1
            e[1] += 1 if unit_one else u[c]
        per_column.append(edges)
    return _table(name, per_column)


def brute_overlap(name, a, b):
    """every label of A against every label of B, O(n^2) per column (small grids)"""
    a, b = np.asarray(a).reshape(len(a), -1), np.asarray(b).reshape(len(b), -1)
    n = len(a)
    u = np.array(units(name), dtype=object)
    ids = np.arange(n)
    per_column = []
    for t in range(a.shape[1]):
        in_a, in_b = is_in(a[:, t:t + 1])[:, 0], is_in(b[:, t:t + 1])[:, 0]
        hot_a = (a[:, t][None, :] == ids[:, None]) & in_a[None, :]              # [label, cell]
        hot_b = (b[:, t][None, :] == ids[:, None]) & in_b[None, :]
        shared = hot_a.astype(np.float64) @ hot_b.astype(np.float64).T          # [label of A, label of B]: cells (exact: below 2^53)
        edges = {}
        for la, lb in np.argwhere(shared > 0):
            cells = np.flatnonzero(hot_a[la] & hot_b[lb])
            edges[(int(la), int(lb))] = [len(cells), int(sum(u[cells]))]
        per_column.append(edges)
    return _table(name, per_column)


def check_overlap(got, ref, what=""):
    """every integer EQUAL, the volume EQUAL bit for bit to float64(units) * hd"""
    assert np.array_equal(np.asarray(got["offsets"]), ref["offsets"]), f"{what} offsets: {np.asarray(got['offsets']).tolist()[:8]} != {ref['offsets'].tolist()[:8]}"
    for k in INT_FIELDS:
        g = np.asarray(got[k])
        assert g.dtype == ref[k].dtype and g.shape == ref[k].shape, f"{what} {k}: {g.dtype} {g.shape}, expected {ref[k].dtype} {ref[k].shape}"
        bad = np.flatnonzero(g != ref[k])
        assert not len(bad), f"{what} {k}: {len(bad)} of {len(g)} differ, the first at edge {bad[0]}: {g[bad[0]]} != {ref[k][bad[0]]}"
    v = np.asarray(got["volume"])
    assert v.dtype == np.float64 and np.array_equal(v.view(np.int64), ref["volume"].view(np.int64)), f"{what} volume: not float64(units) * hd bit for bit"


def plant_non_root(labels, other):
    """a copy of ``labels`` with one cell of column 0 that is in both ``labels`` and ``other`` renamed to a member of some region that is
    no root: by the root rule that cell is out, and the overlap loses exactly one cell"""
    out = np.array(labels, copy=True).reshape(len(labels), -1)
    col = out[:, 0]
    members = np.flatnonzero((col >= 0) & (col != np.arange(len(col))))
    shared = members[is_in(np.asarray(other).reshape(len(out), -1))[members, 0]]
    assert len(members) >= 2 and len(shared), "the column needs two cells that are in and no roots, one of them in the other array too"
    victim = shared[len(shared) // 2]
    col[victim] = members[members != victim][0]
    return out


@functools.lru_cache(maxsize=None)
def columns(name, mask_name, n_t, stride=1):
    """int32 [n, n_t]: columns ``(j * stride) % T`` of ``rc.labels_of(name, mask_name)``: every column a valid labelling"""
    lab = rc.labels_of(name, mask_name)
    return np.ascontiguousarray(lab[:, (np.arange(n_t) * stride) % lab.shape[1]])


def edge_levels(name, a, b):
    """per edge of the reference table the set of levels of its cells: list of sets, in table order"""
    a, b = np.asarray(a).reshape(len(a), -1), np.asarray(b).reshape(len(b), -1)
    lv = rc.grid(name)["levels"]
    both = is_in(a) & is_in(b)
    out = []
    for t in range(a.shape[1]):
        sets = {}
        for c in np.flatnonzero(both[:, t]):
            sets.setdefault((int(a[c, t]), int(b[c, t])), set()).add(int(lv[c]))
        out += [sets[k] for k in sorted(sets)]
    return out


# ---- planted motion -------------------------------------------------------------------------------------------------------------
def _rect(x0, x1, y0, y1):
    x, y = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    return ((x >= x0) & (x < x1) & (y >= y0) & (y < y1)).reshape(-1)


def _motion_masks():
    t_all = range(T_MOTION)
    moving = np.stack([_rect(5 + t, 10 + t, 5, 10) for t in t_all], axis=1)
    # 4 x 4 blobs at speed 2 towards each other: apart until t = 3 ([16, 20) and [22, 26)), one region [18, 24) from t = 4 on, which
    # shares 8 cells with each of the two: a tie
    merge = np.stack([_rect(10 + 2 * t, 14 + 2 * t, 30, 34) | _rect(28 - 2 * t, 32 - 2 * t, 30, 34) for t in t_all], axis=1)
    split = np.stack([_rect(10 + 2 * t, 14 + 2 * t, 45, 49) | _rect(28 - 2 * t, 32 - 2 * t, 45, 49) for t in reversed(t_all)], axis=1)
    appear = np.stack([_rect(40, 44, 5, 9) & (t >= 3) for t in t_all], axis=1)
    vanish = np.stack([_rect(50, 54, 5, 9) & (t < 3) for t in t_all], axis=1)
    masks = {"moving": moving, "merge": merge, "split": split, "appear": appear, "vanish": vanish}
    masks["scene"] = np.logical_or.reduce(list(masks.values()))
    masks["full"] = np.ones((4096, T_MOTION), dtype=bool)
    return masks


MOTIONS = ("moving", "merge", "split", "appear", "vanish", "scene", "full")
TREE_MOTIONS = ("tree2d", "tree3d")


@functools.lru_cache(maxsize=None)
def motion(kind):
    """(grid name, mask bool [n, T], labels int32 [n, T])"""
    if kind in TREE_MOTIONS:
        c = rc.grid(kind)
        x = (c["centers"][:, 0] - c["centers"][:, 0].min()) / sc.WIDTH
        mask = np.stack([(x >= 0.1 + 0.08 * t) & (x < 0.45 + 0.08 * t) for t in range(5)], axis=1)
        name = kind
    else:
        name, mask = "uniform2d", _motion_masks()[kind]
    return name, mask, rc.reference_labels(rc.brute_edges(name), mask)


# ---- tracks ---------------------------------------------------------------------------------------------------------------------
def region_rows(labels):
    """list of (t, label): the rows of the region table of ``labels``"""
    labels = np.asarray(labels).reshape(len(labels), -1)
    inside = is_in(labels)
    return [(t, int(lab)) for t in range(labels.shape[1]) for lab in sorted(set(labels[inside[:, t], t].tolist()))]


def reference_tracks(name, labels, centroid, dt, min_volume=0.0, ties_larger=False, one_sided=False, edges=None):
    """labels [n, T]; centroid [R, d]: the centroids of the region table the tracks are made for (the velocity is their difference
    along a continuation over dt, the same float64 operations as the product's).  ``ties_larger``, ``one_sided``: planted mistakes;
    ``edges``: another overlap table in place of the reference's (for planted mistakes in the table)"""
    labels = np.asarray(labels).reshape(len(labels), -1)
    n_t = labels.shape[1]
    rows = region_rows(labels)
    row_of = {key: i for i, key in enumerate(rows)}
    if edges is None:
        edges = reference_overlap(name, labels[:, :-1], labels[:, 1:])
    out_edges, in_edges = {i: [] for i in range(len(rows))}, {i: [] for i in range(len(rows))}
    for t in range(n_t - 1):
        for e in range(int(edges["offsets"][t]), int(edges["offsets"][t + 1])):
            if edges["volume"][e] < min_volume:
                continue
            a, b, u = int(edges["src"][e]), int(edges["dst"][e]), int(edges["units"][e]) & (2 ** 64 - 1)
            out_edges[row_of[(t, a)]].append((u, b, row_of[(t + 1, b)]))
            in_edges[row_of[(t + 1, b)]].append((u, a, row_of[(t, a)]))

    def best(candidates):
        if not candidates:
            return -1
        return max(candidates, key=lambda e: (e[0], e[1] if ties_larger else -e[1]))[2]
    successor = [best(out_edges[i]) for i in range(len(rows))]
    predecessor = [best(in_edges[i]) for i in range(len(rows))]
    before = [-1] * len(rows)
    for i in range(len(rows)):
        j = successor[i]
        if j >= 0 and (one_sided or predecessor[j] == i):
            before[j] = i
    track, tracks = [-1] * len(rows), []
    for i in range(len(rows)):                                  # rows stand by (t, label): a row's predecessor comes before it
        if before[i] < 0:
            track[i] = len(tracks)
            tracks.append([i])
        else:
            track[i] = track[before[i]]
            tracks[track[i]].append(i)
    centroid = np.asarray(centroid, dtype=np.float64)
    velocity = np.full(centroid.shape, np.nan)
    for i in range(len(rows)):
        if before[i] >= 0:
            velocity[i] = (centroid[i] - centroid[before[i]]) / dt
    n_in, n_out = np.array([len(in_edges[i]) for i in range(len(rows))], dtype=np.int64), np.array([len(out_edges[i]) for i in range(len(rows))], dtype=np.int64)
    t_row = np.array([t for t, _ in rows], dtype=np.int64)
    return {"n_in": n_in, "n_out": n_out, "successor": np.array(successor, dtype=np.int64).reshape(-1), "predecessor": np.array(predecessor, dtype=np.int64).reshape(-1),
            "track": np.array(track, dtype=np.int64).reshape(-1), "born": (n_in == 0) & (t_row > 0), "died": (n_out == 0) & (t_row < n_t - 1),
            "merged": n_in >= 2, "split": n_out >= 2, "first": np.array([rows[tr[0]][0] for tr in tracks], dtype=np.int64).reshape(-1),
            "length": np.array([len(tr) for tr in tracks], dtype=np.int64).reshape(-1), "rows": [np.array(tr, dtype=np.int64) for tr in tracks],
            "velocity": velocity}


TRACK_FIELDS = ("n_in", "n_out", "successor", "predecessor", "track", "born", "died", "merged", "split", "first", "length")


def tracks_as_dict(tracks, dt):
    """a ``RegionTracks`` -> what ``reference_tracks`` returns, as numpy"""
    def host(x):
        return x if isinstance(x, np.ndarray) else x.detach().cpu().numpy()
    out = {k: host(getattr(tracks, k)) for k in TRACK_FIELDS}
    out["rows"] = [np.asarray(tracks.rows(k)) for k in range(len(tracks))]
    out["velocity"] = host(tracks.velocity(dt))
    return out


def check_tracks(got, ref, what=""):
    """every array EQUAL; the velocity bit for bit (NaN at the first row of a track)"""
    for k in TRACK_FIELDS:
        g = np.asarray(got[k])
        assert g.shape == ref[k].shape and g.dtype == ref[k].dtype, f"{what} {k}: {g.dtype} {g.shape}, expected {ref[k].dtype} {ref[k].shape}"
        assert np.array_equal(g, ref[k]), f"{what} {k}: differs at rows {np.flatnonzero(g != ref[k])[:5].tolist()}"
    assert len(got["rows"]) == len(ref["rows"]) and all(np.array_equal(g, r) for g, r in zip(got["rows"], ref["rows"])), f"{what}: the rows of a track differ"
    v = np.asarray(got["velocity"])
    assert v.shape == ref["velocity"].shape and np.array_equal(v.view(np.int64), ref["velocity"].view(np.int64)), f"{what} velocity: not equal bit for bit"
