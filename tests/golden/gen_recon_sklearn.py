"""Generator of tests/golden/recon_sklearn.npz: what scikit-learn predicts where the reconstruction error interpolates the grid's
fields back onto the original points -- ``KNeighborsRegressor(k, weights="distance").fit(centres, fields).predict(points)``, the
call of the reference's post_processing/compute_error_OAT.py:209-223.  Two clouds: 2-D with k = 8 and 3-D with k = 26, each with
150 uniform random centres, 600 points of which the first 20 are COPIES of the centres 0..19 (distance zero: scikit-learn's
indicator weights), and 7 snapshots.  scikit-learn itself is the source here (a third-party dependency of the reference, not
the reference).

No query may have its k-th and (k+1)-th neighbour at the same distance: the neighbour set would be ambiguous and a wrong answer
could hide behind the tolerance.  The generator checks that by brute force and stores the smallest gap.  For the same reason the
centres hold no duplicates (two centres at one place put a tie wherever both are among a point's neighbours).
    python tests/golden/gen_recon_sklearn.py"""
import os

import numpy as np
import sklearn
from sklearn.neighbors import KNeighborsRegressor

NC, N, N_COPIES, T = 150, 600, 20, 7
out = {"sklearn_version": np.array(sklearn.__version__), "n_cases": np.array(2)}
for i, (dim, k) in enumerate([(2, 8), (3, 26)]):
    rng = np.random.default_rng(i)
    c = rng.random((NC, dim))
    x = rng.random((N, dim))
    x[:N_COPIES] = c[:N_COPIES]
    f = rng.standard_normal((NC, T)) + 2.0                  # fields on the grid
    o = rng.standard_normal((N, T)) + 2.0                   # "original" fields at the points
    s = np.sqrt(rng.random(N) + 0.1)                        # square roots of the original cell areas
    dist = np.sqrt(((x[:, None, :] - c[None, :, :]) ** 2).sum(-1))
    dist.sort(axis=1)
    gap = float((dist[:, k] - dist[:, k - 1]).min())
    assert gap > 1e-7, f"case {i}: a query has its neighbours {k} and {k + 1} at one distance (gap {gap})"
    assert (dist[:N_COPIES, 0] == 0.0).all() and (dist[:, 1] > 0.0).all()
    knn = KNeighborsRegressor(n_neighbors=k, weights="distance").fit(c, f)
    assert knn._fit_method == "kd_tree"
    pred = knn.predict(x)
    assert np.array_equal(pred[:N_COPIES], f[:N_COPIES])     # the indicator rule
    out.update({f"centers{i}": c, f"points{i}": x, f"grid{i}": f, f"orig{i}": o, f"scale{i}": s, f"pred{i}": pred,
                f"k{i}": np.array(k), f"gap{i}": np.array(gap)})
    print(f"case {i}: dim {dim} k {k} smallest boundary gap {gap:.2e}")
np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "recon_sklearn.npz"), **out)
