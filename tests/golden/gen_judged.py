"""
Stored verdicts of the REAL reference (where ``ref_stubs.REFERENCE_ROOT`` points) for the tests that compare this package with it
(tests/test_compat_alias.py, tests/test_export_vs_reference.py).  Every verdict comes from ``ref_judge.py`` in its own process,
exactly as those tests used to run it; the tests now read the stored result, so they need nothing outside the repository.

Run where the reference is present, after ``build()``:

    python tests/golden/gen_judged.py            # writes tests/golden/judged/

What is stored (``judged/``):
    facade_<case>.json        ref_judge facade: what the reference's execute_grid_generation leaves behind (inputs.describe_facade)
    errors.json               ref_judge errors: outcome of every call of inputs.invalid_calls on the reference's classes
    logs.json                 ref_judge logs: every logging record of inputs.logged_run on the reference's classes
    load_<d>d.npz             ref_judge load: what the reference's Dataloader sees in the file THIS build writes
                              (test_export_vs_reference._write_with_build), plus the digest of that file's inventory
    xdmf.json                 ref_judge xdmf: the reference's XDMF text for each file this build writes, plus the file's digest
    datawriter/out.{h5,xdmf}  ref_judge write: the file the reference's Datawriter writes through inputs.datawriter_script
    fuzz_export/seed<i>/      ref_judge fuzz_export: every file the reference writes for inputs.random_export_case(i), i < 6

Contains no reference code: it calls ref_judge.py, which calls the reference's public classes.
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "judged")
FACADE_CASES = ("refine_2d_metric", "refine_3d_ncells_cone")
FUZZ_SEEDS = 6


def judge(*args):
    run = subprocess.run([sys.executable, os.path.join(HERE, "ref_judge.py"), *map(str, args)], capture_output=True, text=True,
                         timeout=900, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]


def main():
    sys.path[:0] = [ROOT, HERE]
    import numpy as np
    from tests.test_export_vs_reference import XDMF_CASES, file_digest, _write_with_build

    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    with tempfile.TemporaryDirectory() as tmp:
        for case in FACADE_CASES:
            d = os.path.join(tmp, "facade_" + case)
            os.makedirs(d)
            out = os.path.join(OUT, f"facade_{case}.json")
            judge("facade", d, case, out)
            want = json.load(open(out))
            for part in ("attributes", "pickled"):              # (the tests do not compare the output directory)
                want[part]["save_path"][1] = "<save_path>"
            json.dump(want, open(out, "w"))
        judge("errors", os.path.join(OUT, "errors.json"))
        os.makedirs(os.path.join(tmp, "logs"))
        judge("logs", os.path.join(tmp, "logs"), os.path.join(OUT, "logs.json"))

        for d in (2, 3):
            work = os.path.join(tmp, f"load{d}")
            os.makedirs(work)
            _write_with_build(work, d, n_t=21)
            judge("load", work, "mine.h5", os.path.join(work, "seen.npz"))
            seen = dict(np.load(os.path.join(work, "seen.npz")))
            np.savez_compressed(os.path.join(OUT, f"load_{d}d.npz"), file_digest=np.array(file_digest(os.path.join(work, "mine.h5"))), **seen)

        texts = {}
        for key, (d, with_data, with_const, mixed) in XDMF_CASES.items():
            work = os.path.join(tmp, "xdmf_" + key)
            os.makedirs(work)
            _write_with_build(work, d, n_t=12, with_data=with_data, with_const=with_const, seed=d)
            judge("xdmf", work, "mine.h5", mixed)
            texts[key] = {"file_digest": file_digest(os.path.join(work, "mine.h5")), "xdmf": open(os.path.join(work, "mine.xdmf")).read()}
        json.dump(texts, open(os.path.join(OUT, "xdmf.json"), "w"), indent=1, sort_keys=True)

        work = os.path.join(OUT, "datawriter")
        os.makedirs(work)
        shutil.copy(os.path.join(HERE, "s_cube_test_dataset.h5"), os.path.join(work, "src.h5"))
        judge("write", work, "src.h5", "out.h5")
        os.remove(os.path.join(work, "src.h5"))

        judge("fuzz_export", os.path.join(OUT, "fuzz_export"), 0, FUZZ_SEEDS)
    for dirpath, _, files in os.walk(OUT):                   # only what the tests read: the .h5 / .xdmf files and the verdicts
        for f in files:
            if not f.endswith((".h5", ".xdmf", ".json", ".npz")):
                os.remove(os.path.join(dirpath, f))
    total = sum(os.path.getsize(os.path.join(p, f)) for p, _, fs in os.walk(OUT) for f in fs)
    print(f"wrote {OUT} ({total / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
