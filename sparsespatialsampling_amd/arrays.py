"""
What the analysis front-ends (``differential``, ``sampling``, ``isosurface``, ``reconstruction``, ``spectral``, ``dmd``, ``metrics``,
``svd``) share in front of ``hipops``: none of it is kernel code, all of it decides what a kernel is handed -- which pointer, whether
a batch is copied or read where it lies, and on which side a result comes back.
"""
import numpy as np
import torch as pt

from . import hipops


def as_tensor(x, what):
    """numpy array -> tensor sharing its memory (a contiguous copy where the array is not); a tensor passes through"""
    if isinstance(x, np.ndarray):
        return pt.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, pt.Tensor):
        raise TypeError(f"{what} must be a numpy array or a torch tensor, got {type(x).__name__}")
    return x


def resident(x, pitched=True):
    """THE read-in-place rule.  A float32 / float64 tensor on ``hipops.device()`` is returned as it is -- the kernels read it where it
    lies -- when it is contiguous or, with ``pitched`` (the kernel takes a row pitch), a 2-D view with unit inner stride and
    ``stride(0) >= shape[1]``: a snapshot window ``field[:, t0:t1]``.  Everything else is uploaded / copied once into a contiguous
    device tensor, other dtypes widened to float64 first."""
    if x.dtype not in hipops.DTYPE_CODE:
        return hipops.to_device(x.to(pt.float64))
    if x.is_cuda and x.device == hipops.device() and (
            x.is_contiguous() or (pitched and x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= x.shape[1])):
        return x
    return hipops.to_device(x)


def resident_matrix(data, n_cells, n_comp, t):
    """``data`` [n_cells, t] (``n_comp`` None) or [n_cells, n_comp, t] as the 2-D device matrix [rows, t] the matrix-core kernels read:
    taken where it lies, pitch included, when it is on the device already, else uploaded in its own dtype.  For callers whose
    argument checks have refused every other dtype and stride; no widening, no contiguity demand (``resident`` has both)."""
    d = data if data.is_cuda and data.device == hipops.device() else hipops.to_device(data)
    return d.reshape(n_cells * n_comp, t) if n_comp is not None else d


class Side:
    """where results go: made from the input whose side decides, ``back`` is the one way home"""

    def __init__(self, x):
        self.numpy = isinstance(x, np.ndarray)
        self.host = self.numpy or not x.is_cuda

    def back(self, t):
        """a tensor onto the side of the input: host for a host input (after the stream is through with it; a numpy array for a
        numpy input), the device for a device input"""
        if not self.host:
            return t if t.is_cuda else t.to(hipops.device())
        if t.is_cuda:
            hipops.synchronize()
            t = t.cpu()
        return t.numpy() if self.numpy else t


def knn_table(cloud, queries, k, exact_weights=False):
    """the ``k`` nearest points of ``cloud`` to each of ``queries``: (idx int32 [nq, k], w f64 [nq, k] or None) on the device, in the
    order of the queries.  ``exact_weights``: scikit-learn's distance weights (``hipops.idw_weights_exact``)."""
    knn = hipops.KnnIndex(cloud)
    try:
        idx, dist = knn.query(queries, k)
        w = hipops.idw_weights_exact(dist) if exact_weights else None
        hipops.synchronize()
    finally:
        knn.close()
    return idx, w


def hilbert_knn(cloud, queries, k, *, exact_weights=False):
    """``knn_table`` put into Hilbert launch order of the device points ``queries``: neighbouring slots of a launch then gather the same
    few rows.  -> (idx, w, rows): slot j holds the table of query ``rows[j]`` (``rows`` int32 [nq] on the device)."""
    idx, w = knn_table(cloud, queries, k, exact_weights)
    if not int(queries.shape[0]):
        return idx, w, pt.empty(0, dtype=pt.int32, device=idx.device)
    rows = hipops.spatial_order(queries)
    return (hipops.gather_rows(idx, rows, pt.empty_like(idx)), None if w is None else hipops.gather_rows(w, rows, pt.empty_like(w)),
            rows)


def default_neighbors(dim, n_neighbors, cap):
    """the stencil size: 8 in 2-D and 26 in 3-D by default (the reference's counts), never more than ``cap``"""
    k = (8 if dim == 2 else 26) if n_neighbors is None else int(n_neighbors)
    if k < 1:
        raise ValueError(f"n_neighbors must be positive, got {k}")
    return min(k, int(cap))
