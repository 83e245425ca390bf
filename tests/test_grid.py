"""
``grid.Grid`` without a device: every malformed grid is a ``ValueError`` before anything is uploaded, a well-formed one gets as far as
the device and no further; the two constructors from the loader and from the s_cube object map the two naming schemes; and the
``ctypes.Structure`` of ``_lib`` has the layout a C compiler gives ``s3_grid`` of include/s3hip.h.
"""
import contextlib
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch as pt

from sparsespatialsampling_amd import _lib
from sparsespatialsampling_amd.grid import Grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC, NN = 5, 12


def parts(d=2):
    """a well-formed grid of NC cells and NN nodes (the values are never looked at: the shapes, types and face ids are)"""
    rng = np.random.default_rng(d)
    return {"centers": rng.random((NC, d)), "levels": rng.integers(0, 4, NC).astype(np.int32), "width": 0.7,
            "nodes": rng.random((NN, d)), "faces": rng.integers(0, NN, (NC, 1 << d)).astype(np.int32)}


def changed(d=2, **kw):
    return {**parts(d), **kw}


def face_id(value):
    faces = parts()["faces"].copy()
    faces[3, 1] = value
    return faces


MALFORMED = {
    "centers [n, 4]": changed(centers=np.zeros((NC, 4))),
    "centers [n]": changed(centers=np.zeros(NC)),
    "float levels": changed(levels=np.zeros(NC)),
    "wrong level count": changed(levels=np.zeros(NC + 1, dtype=np.int32)),
    "faces [n, 3]": changed(faces=np.zeros((NC, 3), dtype=np.int32)),
    "faces of 3-D cells on a 2-D grid": changed(faces=np.zeros((NC, 8), dtype=np.int32)),
    "faces of another cell count": changed(faces=np.zeros((NC + 1, 4), dtype=np.int32)),
    "float faces": changed(faces=np.zeros((NC, 4))),
    "face id Nn": changed(faces=face_id(NN)),
    "face id -1": changed(faces=face_id(-1)),
    "nodes without faces": changed(faces=None),
    "faces without nodes": changed(nodes=None),
    "nodes [Nn, d + 1]": changed(nodes=np.zeros((NN, 3))),
    "nodes [Nn, d - 1]": changed(3, nodes=np.zeros((NN, 2))),
    "no width": changed(width=None),
    "no levels": changed(levels=None),
    "no centers": changed(centers=None),
    "zero nodes": {"nodes": np.zeros((0, 2)), "faces": np.zeros((0, 4), dtype=np.int32)},
    "corner part alone, nodes [Nn, 4]": {"nodes": np.zeros((NN, 4)), "faces": np.zeros((NC, 16), dtype=np.int32)},
    "corner part alone, face id Nn": {"nodes": parts()["nodes"], "faces": face_id(NN)},
    "nothing": {},
}


@pytest.mark.parametrize("what", sorted(MALFORMED))
@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_malformed_grid_is_refused_before_any_device_call(what, kind, monkeypatch):
    from sparsespatialsampling_amd import hipops
    monkeypatch.setattr(hipops, "to_device", lambda *a, **k: pytest.fail("an upload before the checks were through"))
    monkeypatch.setattr(hipops, "device", lambda: pytest.fail("a device call before the checks were through"))
    kw = {k: pt.from_numpy(v) if kind == "torch" and isinstance(v, np.ndarray) else v for k, v in MALFORMED[what].items()}
    with pytest.raises(ValueError):
        Grid(**kw)


def test_nodes_and_faces_go_together_in_words():
    with pytest.raises(ValueError, match="nodes and faces"):
        Grid(**changed(faces=None))
    with pytest.raises(ValueError, match="nodes and faces"):
        Grid(**changed(nodes=None))


@pytest.mark.parametrize("keys", [("centers", "levels", "width", "nodes", "faces"), ("centers", "levels", "width"), ("nodes", "faces")])
@pytest.mark.parametrize("d", [2, 3])
def test_well_formed_grid_reaches_the_device_and_nothing_else(keys, d):
    def built():                            # with a device the grid is simply built (tests/test_gpu_grid.py goes on from there)
        return contextlib.nullcontext() if pt.cuda.is_available() else pytest.raises(_lib.HipUnavailableError)
    p = parts(d)
    kw = {k: p[k] for k in keys}
    with built():
        Grid(**kw)
    if "levels" in keys:                    # [Nc, 1] levels of another integer type, as the files hold them
        with built():
            Grid(**{**kw, "levels": pt.from_numpy(p["levels"]).long().unsqueeze(-1)})
    with built():                           # a corner part without cells stays legal
        Grid(nodes=p["nodes"], faces=np.zeros((0, 1 << d), dtype=np.int32))


def record(cls, monkeypatch):
    """``Grid.__init__`` replaced by a recorder -> the dict the arguments land in"""
    seen = {}

    def init(self, centers=None, levels=None, width=None, nodes=None, faces=None):
        seen.update(centers=centers, levels=levels, width=width, nodes=nodes, faces=faces)
    monkeypatch.setattr(cls, "__init__", init)
    return seen


def test_the_two_naming_schemes(monkeypatch):
    arrays = {name: np.full((2, 2), i) for i, name in enumerate(("centres", "levels", "corners", "faces"))}
    loader = types.SimpleNamespace(vertices=arrays["centres"], levels=arrays["levels"], size_initial_cell=0.3, nodes=arrays["corners"],
                                   faces=arrays["faces"], _size_initial_cell=-1.0)
    s_cube = types.SimpleNamespace(centers=arrays["centres"], levels=arrays["levels"], size_initial_cell=pt.tensor(0.3, dtype=pt.float64),
                                   vertices=arrays["corners"], faces=arrays["faces"])
    seen = record(Grid, monkeypatch)
    for make, source in ((Grid.from_dataloader, loader), (Grid.from_s_cube, s_cube)):
        seen.clear()
        assert isinstance(make(source), Grid)
        assert seen["centers"] is arrays["centres"] and seen["levels"] is arrays["levels"] and seen["nodes"] is arrays["corners"]
        assert seen["faces"] is arrays["faces"] and float(seen["width"]) == 0.3


def test_from_s_cube_before_the_grid_is_generated():
    with pytest.raises(ValueError, match="execute_grid_generation"):
        Grid.from_s_cube(types.SimpleNamespace(centers=None))
    with pytest.raises(ValueError, match="execute_grid_generation"):
        Grid.from_s_cube(types.SimpleNamespace())


def test_dataloader_states_the_initial_cell_size(golden_dir):
    from sparsespatialsampling_amd.data import Dataloader
    loader = Dataloader(golden_dir, "s_cube_test_dataset.h5")
    assert loader.size_initial_cell == loader._size_initial_cell and float(loader.size_initial_cell) > 0.0
    with pytest.raises(AttributeError):
        loader.size_initial_cell = 1.0


def test_s3_grid_layout_is_the_compilers(tmp_path):
    """sizeof and every offsetof of ``s3_grid`` as gcc lays it out against ``_lib.S3Grid``, field by field, in the header's order"""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "s3hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct s3_grid \{(.*?)\} s3_grid;", header, flags=re.S).group(1)
    names = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"\**(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert names == [name for name, _ in _lib.S3Grid._fields_] and len(names) == 12
    lines = "".join(f'    printf("{n} %zu %zu\\n", offsetof(s3_grid, {n}), sizeof(((s3_grid *)0)->{n}));\n' for n in names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "s3hip.h"\nint main(void) {\n    printf("s3_grid %zu\\n", sizeof(s3_grid));\n'
                   + lines + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    assert out[0] == f"s3_grid {ctypes.sizeof(_lib.S3Grid)}"
    for line, (name, kind) in zip(out[1:], _lib.S3Grid._fields_):
        assert line == f"{name} {getattr(_lib.S3Grid, name).offset} {ctypes.sizeof(kind)}"
