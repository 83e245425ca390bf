"""
The references of tests/track_cases.py against brute force, the comparisons of tests/test_gpu_overlap.py against planted mistakes,
the host bookkeeping of ``regions.RegionTracks`` against the loops of ``reference_tracks``, and include/s3overlap.h against its
bindings (CPU only).
"""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import region_cases as rc
from tests import track_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3overlap.h")
SMALL = [name for name in rc.GRIDS if len(rc.grid(name)["centers"]) <= 800]


# ---- the references -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_reference_overlap_agrees_with_brute_force(name):
    a, b = rc.labels_of(name, "random0.5"), rc.labels_of(name, "random0.7")
    tc.check_overlap(tc.reference_overlap(name, a, b), tc.brute_overlap(name, a, b), name)
    shifted = tc.columns(name, "random0.7", 5)
    tc.check_overlap(tc.reference_overlap(name, shifted[:, :-1], shifted[:, 1:]), tc.brute_overlap(name, shifted[:, :-1], shifted[:, 1:]), name)


def test_units_are_the_integer_volumes():
    for name in ("chain2d", "chain3d", "tree3d", "uniform2d"):
        g, depth = rc.grid(name), rc.boxes(name)[2]
        d = g["centers"].shape[1]
        assert tc.units(name) == [1 << (d * (depth - int(l))) for l in g["levels"]]
        assert sum(tc.units(name)) <= 1 << 63
    assert max(tc.units("chain3d")) == 1 << 60 and max(tc.units("chain2d")) == 1 << 60


@pytest.mark.parametrize("kind", tc.TREE_MOTIONS)
def test_tree_motions_are_tests(kind):
    """by the reference alone: edges whose cells have two or more levels, one of them across a jump of two or more"""
    name, _, labels = tc.motion(kind)
    levels = tc.edge_levels(name, labels[:, :-1], labels[:, 1:])
    assert sum(len(s) >= 2 for s in levels) >= 1 and max(max(s) - min(s) for s in levels) >= 2
    ref = tc.reference_overlap(name, labels[:, :-1], labels[:, 1:])
    assert (np.diff(ref["offsets"]) >= 1).all() and (ref["units"] != ref["n_cells"]).any()


def test_planted_motions_are_what_they_claim():
    seen = {}
    for kind in tc.MOTIONS:
        name, mask, labels = tc.motion(kind)
        rows = tc.region_rows(labels)
        seen[kind] = tc.reference_tracks(name, labels, np.zeros((len(rows), 2)), 1.0)
        assert mask.shape == (4096, tc.T_MOTION)
    one = {k: (len(v["rows"]), int(v["merged"].sum()), int(v["split"].sum()), int(v["born"].sum()), int(v["died"].sum())) for k, v in seen.items()}
    assert one["moving"] == (1, 0, 0, 0, 0) and one["full"] == (1, 0, 0, 0, 0)
    assert one["merge"] == (2, 1, 0, 0, 0) and one["split"] == (2, 0, 1, 0, 0)
    assert one["appear"] == (1, 0, 0, 1, 0) and one["vanish"] == (1, 0, 0, 0, 1)
    assert one["scene"] == (7, 1, 1, 1, 1)
    assert seen["moving"]["length"].tolist() == [tc.T_MOTION] and seen["merge"]["length"].tolist() == [tc.T_MOTION, 4]
    full = tc.reference_overlap("uniform2d", *(lambda lab: (lab[:, :-1], lab[:, 1:]))(tc.motion("full")[2]))
    assert (full["n_cells"] == 4096).all() and len(full["src"]) == tc.T_MOTION - 1            # one edge of more than 1024 cells per column


# ---- planted mistakes in the table ----------------------------------------------------------------------------------------------
def rejected(got, ref):
    with pytest.raises(AssertionError):
        tc.check_overlap(got, ref)


@pytest.mark.parametrize("kind", tc.TREE_MOTIONS)
def test_overlap_check_rejects_planted_mistakes(kind):
    name, _, labels = tc.motion(kind)
    a, b = labels[:, :-1], labels[:, 1:]
    ref = tc.reference_overlap(name, a, b)
    tc.check_overlap({k: v.copy() for k, v in ref.items()}, ref)
    rejected(tc.reference_overlap(name, a, b, unit_one=True), ref)                          # units of 1 per cell
    rejected(tc.reference_overlap(name, a, a), ref)                                         # column t against t
    rejected({**ref, "src": ref["dst"], "dst": ref["src"]}, ref)                            # src and dst swapped
    rejected({**ref, "volume": ref["volume"] * (1 + 2.0 ** -52)}, ref)
    rejected({**ref, "units": ref["units"].astype(np.uint64)}, ref)
    rejected({**ref, "n_cells": ref["units"]}, ref)
    planted = tc.plant_non_root(a, b)                                                          # one non-root value: the cell is out
    assert (planted != a).sum() == 1
    by_rule = tc.reference_overlap(name, planted, b)
    assert by_rule["n_cells"].sum() == ref["n_cells"].sum() - 1
    rejected(tc.reference_overlap(name, planted, b, root_rule=False), by_rule)              # the root rule dropped


# ---- the tracks -----------------------------------------------------------------------------------------------------------------
def _tables(kind):
    """(name, labels, RegionTable, OverlapTable) from the references, as numpy"""
    from sparsespatialsampling_amd.regions import OverlapTable, RegionTable
    name, _, labels = tc.motion(kind)
    ref = rc.reference_table(name, labels)
    table = RegionTable(ref["offsets"], **{k: (ref[k].astype(np.float64) if k in ref and ref[k].dtype == rc.LD else ref.get(k)) for k in RegionTable.FIELDS})
    edges = tc.reference_overlap(name, labels[:, :-1], labels[:, 1:])
    return name, labels, table, OverlapTable(edges["offsets"], **{k: edges[k] for k in OverlapTable.FIELDS})


@pytest.mark.parametrize("kind", tc.MOTIONS + tc.TREE_MOTIONS)
def test_region_tracks_equal_the_loops(kind):
    """the vectorised host code of the product against dicts and loops, on the reference tables"""
    from sparsespatialsampling_amd.regions import RegionTracks
    name, labels, table, edges = _tables(kind)
    for min_volume in (0.0, float(np.min(edges.volume)) * 1.5):
        got = RegionTracks(table, edges, len(labels), min_volume)
        ref = tc.reference_tracks(name, labels, table.centroid, 0.125, min_volume)
        tc.check_tracks(tc.tracks_as_dict(got, 0.125), ref, f"{kind} min_volume={min_volume}")
        assert sorted(np.concatenate([got.rows(k) for k in range(len(got))]).tolist()) == list(range(len(table)))       # every row in exactly one track
        assert [tc.region_rows(labels)[int(got.rows(k)[0])] for k in range(len(got))] == sorted(tc.region_rows(labels)[int(got.rows(k)[0])] for k in range(len(got)))


def test_track_check_rejects_planted_mistakes():
    name, labels, table, edges = _tables("scene")
    ref = tc.reference_tracks(name, labels, table.centroid, 0.125)
    tc.check_tracks({k: (v.copy() if isinstance(v, np.ndarray) else list(v)) for k, v in ref.items()}, ref)
    swapped = {**{k: getattr(edges, k) for k in edges.FIELDS}, "offsets": edges.offsets, "src": edges.dst, "dst": edges.src}
    for wrong in (dict(ties_larger=True), dict(one_sided=True), dict(min_volume=float(np.min(edges.volume)) * 1.5)):
        with pytest.raises(AssertionError):
            tc.check_tracks(tc.reference_tracks(name, labels, table.centroid, 0.125, **wrong), ref)
    with pytest.raises((AssertionError, KeyError)):                                         # src and dst swapped: ends that are no rows
        tc.check_tracks(tc.reference_tracks(name, labels, table.centroid, 0.125, edges=swapped), ref)
    with pytest.raises(AssertionError):
        tc.check_tracks({**ref, "velocity": ref["velocity"] * (1 + 2.0 ** -52)}, ref)
    # the ties are there: the merged region shares the same units with both blobs, the splitting one with both halves
    _, labels_m, _, edges_m = _tables("merge")
    into = edges_m.of_column(3)
    assert len(into["src"]) == 2 and into["units"][0] == into["units"][1] and into["dst"][0] == into["dst"][1]


def test_a_single_snapshot_has_no_edges():
    from sparsespatialsampling_amd.regions import OverlapTable, RegionTable, RegionTracks
    name, _, labels = tc.motion("scene")
    ref = rc.reference_table(name, labels[:, :1])
    table = RegionTable(ref["offsets"], **{k: (ref[k].astype(np.float64) if k in ref and ref[k].dtype == rc.LD else ref.get(k)) for k in RegionTable.FIELDS})
    empty = tc.reference_overlap(name, labels[:, :0], labels[:, :0])
    tracks = RegionTracks(table, OverlapTable(empty["offsets"], **{k: empty[k] for k in OverlapTable.FIELDS}), len(labels))
    assert len(tracks) == len(table) and tracks.track.tolist() == list(range(len(table))) and np.isnan(tracks.velocity(1.0)).all()
    assert not (tracks.born.any() or tracks.died.any() or tracks.merged.any() or tracks.split.any())


# ---- the front-end --------------------------------------------------------------------------------------------------------------
def test_the_front_end_exists():
    """what this family adds: fails where the package lacks it"""
    import sparsespatialsampling_amd as pkg
    from sparsespatialsampling_amd import OverlapTable, Regions, RegionTracks, hipops
    assert "OverlapTable" in pkg.__all__ and "RegionTracks" in pkg.__all__
    assert all(callable(getattr(hipops, f)) for f in ("overlap_count", "overlap_emit", "overlap_heads", "overlap_reduce", "overlap_table"))
    assert callable(Regions.overlap) and callable(Regions.track) and callable(OverlapTable.of_column) and callable(RegionTracks.velocity)
    assert OverlapTable.FIELDS == ("src", "dst", "n_cells", "units", "volume")
    assert "no kernel" in RegionTracks.__doc__.lower()


def test_argument_errors_are_value_errors():
    """the checks that come before any device work (a ``Regions`` without its grid: nothing here reaches the device)"""
    from sparsespatialsampling_amd.regions import OverlapTable, Regions, RegionTable, RegionTracks
    regions = Regions.__new__(Regions)
    regions.n_cells = 10
    good = np.zeros((10, 3), dtype=np.int32)
    for a, b in [(good, np.zeros((10, 2), dtype=np.int32)), (good, good.astype(np.int64)), (good.astype(np.float32), good), (good[:9], good[:9]),
                 (np.zeros((10, 0), dtype=np.int32), np.zeros((10, 0), dtype=np.int32)), ("labels", good), (np.zeros((10, 3, 1), dtype=np.int32), good)]:
        with pytest.raises(ValueError):
            regions.overlap(a, b)
    for kwargs in (dict(min_volume=-1.0), dict(min_volume=float("nan")), dict(min_volume="much"), dict(table="table")):
        with pytest.raises(ValueError):
            regions.track(good, **kwargs)
    with pytest.raises(ValueError):
        regions.track(good.astype(np.int64))
    name, labels, table, edges = _tables("moving")
    with pytest.raises(ValueError):
        regions.n_cells = len(labels)
        regions.track(labels[:, :3], table=table)                                           # a table of other labels: 6 snapshots
    with pytest.raises(ValueError):
        RegionTracks(table, OverlapTable(edges.offsets[:-1], **{k: getattr(edges, k) for k in edges.FIELDS}), len(labels))
    with pytest.raises(ValueError):
        RegionTracks(table, OverlapTable(edges.offsets, **{**{k: getattr(edges, k) for k in edges.FIELDS}, "src": edges.src + 1}), len(labels))
    with pytest.raises(ValueError):
        RegionTracks(table, edges, len(labels)).velocity(0.0)
    with pytest.raises(IndexError):
        edges.of_column(len(edges.offsets) - 1)
    assert isinstance(table, RegionTable) and len(edges.of_column(0)["src"]) == 1


# ---- the header -----------------------------------------------------------------------------------------------------------------
def declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return text, sorted(set(re.findall(r"\b(s3_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_what_is_bound_and_exported():
    from sparsespatialsampling_amd import _lib
    text, names = declared()
    assert names == sorted(_lib.OVERLAP_SIGNATURES) and len(names) == 4
    assert not set(names) & set(_lib.HIP_SIGNATURES)
    lib = _lib.hip_lib()
    for name in names:
        assert hasattr(lib, name), f"{name} declared in s3overlap.h but not exported by libs3hip.so"
        assert list(getattr(lib, name).argtypes) == _lib.OVERLAP_SIGNATURES[name][1]
        params = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", text, flags=re.S).group(1)
        assert len(params.split(",")) == len(_lib.OVERLAP_SIGNATURES[name][1]), name
        assert re.search(r"\bs3_stream\s+stream\s*$", params.strip()), f"{name} takes no stream"
    for code, value in _lib_codes().items():
        assert re.search(r"#define\s+S3_OVERLAP_" + code.upper() + r"\s+" + str(value) + r"\b", text)


def _lib_codes():
    from sparsespatialsampling_amd import hipops
    return hipops.OVERLAP_PASSES


def test_a_library_without_the_symbols_is_refused(monkeypatch):
    from sparsespatialsampling_amd import _lib
    _lib.hip_lib()
    monkeypatch.setattr(_lib, "_hip", None)
    monkeypatch.setattr(_lib, "OVERLAP_SIGNATURES", {**_lib.OVERLAP_SIGNATURES, "s3_overlap_no_such_symbol": (None, [])})
    with pytest.raises(_lib.HipUnavailableError, match="s3_overlap_no_such_symbol.*rebuild"):
        _lib.hip_lib()


def test_header_has_no_torch_or_cxx_types():
    text, _ = declared()
    assert "torch" not in text.lower() and "at::" not in text and "std::" not in text and "Tensor" not in text
    assert '#include "s3hip.h"' in text


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "use_overlap.c"
    src.write_text('#include "s3overlap.h"\nint main(void) { return S3_OVERLAP_BY_TA == 2 && sizeof(s3_grid) > 0 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_the_build_knows_the_source_and_the_header():
    import __graft_entry__ as entry
    assert "overlap.hip" in entry.HIP_SOURCES
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "s3overlap.h" in text[text.index("def build_hip"):text.index("def build_topo")]
