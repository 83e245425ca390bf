"""
Thin Python front-end of the libs3hip.so C ABI (include/s3hip.h).

torch is used here only as plumbing: device memory (``torch.empty(..., device="cuda")``), host<->device copies and the
current HIP stream.  Every function below ends in exactly one hand-written HIP kernel family of libs3hip.so; no torch
operator runs on the hot path.  All tensors passed in must live on the current CUDA(HIP) device and be contiguous.
"""
import ctypes as C

import numpy as np
import torch as pt

from . import _lib
from ._lib import check

DTYPE_CODE = {pt.float32: 0, pt.float64: 1}


def _stream():
    """torch's current HIP stream of the current device as a raw handle (the private getters skip the availability
    checks of ``torch.cuda.current_stream()``, which cost more than a small kernel launch)"""
    try:
        return C.c_void_p(pt._C._cuda_getCurrentRawStream(pt._C._cuda_getDevice()))
    except AttributeError:          # other torch build
        return C.c_void_p(pt.cuda.current_stream().cuda_stream)


def _ptr(t):
    if t is None:
        return C.c_void_p(0)
    if not (t.is_cuda and t.is_contiguous()):       # a host pointer handed to a kernel would fault the GPU
        raise TypeError("device-resident contiguous tensor required")
    return C.c_void_p(t.data_ptr())


def _host_f64(values, n=3):
    a = np.zeros(n, dtype=np.float64)
    v = np.asarray(values, dtype=np.float64).ravel()
    a[:len(v)] = v
    return a


def _host_ptr(a):
    """a numpy array's memory as a call argument (the pointer keeps the array alive)"""
    return a.ctypes.data_as(C.c_void_p)


def _row_layout(t):
    """(row_len, stride in elements) of a tensor whose leading axis is the row axis when its rows can be read where they lie:
    contiguous [n, ...], or a 2-D view with unit inner stride and a pitch >= the row length (``buf[:, a:b]``); None otherwise.
    Shape and strides alone: no device access."""
    if t.dim() < 1:
        return None
    row_len = int(np.prod(t.shape[1:])) if t.dim() > 1 else 1
    if t.is_contiguous():
        return row_len, row_len
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= row_len:
        return row_len, int(t.stride(0))
    return None


def _field_rows(field, who, max_dim=3):
    """(n_comp, T, in_stride) of a field [n] (one snapshot), [n, T] (rows may be pitched: read where they lie) or, with
    ``max_dim`` 3, [n, n_comp, T] contiguous.  Shape and strides alone; the caller answers for device and dtype."""
    if field.dim() == 3 and max_dim == 3:
        if not field.is_contiguous():
            raise TypeError(f"{who}: a field [n, n_comp, T] must be contiguous")
        n_comp, t = int(field.shape[1]), int(field.shape[2])
        return n_comp, t, n_comp * t
    layout = _row_layout(field) if field.dim() <= 2 else None
    if layout is None:
        raise TypeError(f"{who}: rows must be contiguous (a row pitch is allowed for a 2-D tensor)")
    return (1,) + layout


def _launch_rows(rows, n, who):
    """the launch order ``rows`` (None: slot i is row i): int32 [n] on the device, contiguous as the kernels index it"""
    if rows is not None and not (isinstance(rows, pt.Tensor) and rows.is_cuda and rows.dtype == pt.int32 and rows.numel() == n
                                 and rows.is_contiguous()):
        raise TypeError(f"{who}: rows must be a contiguous int32 device tensor [{n}]")
    return rows


def _out_tensor(out, shape, dtype, device, who, what="out", at_least=False):
    """``out`` when it can take ``shape`` values of ``dtype`` on ``device`` (``at_least``: or more), a new tensor for None"""
    if out is None:
        return pt.empty(shape, dtype=dtype, device=device)
    numel = int(np.prod(shape))
    if not (isinstance(out, pt.Tensor) and out.is_cuda and out.is_contiguous() and out.dtype == dtype and out.device == device
            and (out.numel() >= numel if at_least else out.numel() == numel)):
        raise TypeError(f"{who}: {what} must be a contiguous {dtype} device tensor of {'at least ' if at_least else ''}"
                        f"{' x '.join(str(int(v)) for v in shape)} values")
    return out


def _component_groups(n_comp):
    """(first component, components) of the launches of a field: the kernels take up to three components at a time"""
    return ((c0, min(3, n_comp - c0)) for c0 in range(0, n_comp, 3))


def _scratch(nbytes, device):
    """``nbytes`` of device scratch memory, 8-byte aligned"""
    return pt.empty((int(nbytes) + 7) // 8, dtype=pt.float64, device=device)


def device():
    """The torch device of the hot path; raises HipUnavailableError when there is none (no CPU fallback)."""
    _lib.require_device()
    if not pt.cuda.is_available():
        raise _lib.HipUnavailableError("torch sees no HIP device; it is needed for device memory and streams.")
    return pt.device("cuda", pt.cuda.current_device())


def synchronize():
    pt.cuda.current_stream().synchronize()


def to_device(x, dtype=None):
    """numpy / CPU tensor / CUDA tensor -> contiguous CUDA tensor (optionally cast).  Host tensors go through the native
    staged upload (s3_upload_rows: a memcpy into a page-locked buffer plus an asynchronous copy on the current stream -- a
    plain copy from pageable memory blocks the caller for ~0.2 ms however small it is, and the refine loop uploads two id
    lists per iteration), in 1-MiB rows when they are large."""
    if isinstance(x, np.ndarray):
        x = pt.from_numpy(np.ascontiguousarray(x))
    if dtype is not None and x.dtype != dtype:
        x = x.to(dtype)
    dev = device()
    if x.is_cuda or not x.is_contiguous() or x.numel() == 0:
        return x.to(dev, non_blocking=False).contiguous()
    nbytes = x.numel() * x.element_size()
    if nbytes <= (4 << 20):
        out = pt.empty(x.shape, dtype=x.dtype, device=dev)
        rc = _lib.hip_lib().s3_upload_rows(C.c_void_p(x.data_ptr()), 1, nbytes, C.c_void_p(out.data_ptr()), nbytes, _stream())
        if rc == 0:
            return out                                          # (x was copied into the staging buffer: it may be reused)
        return x.to(dev, non_blocking=False).contiguous()       # no page-locked staging memory on this host
    # (r5: every size goes through the library's own page-locked staging buffers -- no pageable pointer is handed to the HIP
    # runtime, which would pin the caller's pages on the fly; round 5 saw rare GPU memory faults, "write access to a read-only page"
    # at a host heap address, in copies the runtime had pinned that way: HISTORY 9)
    out = pt.empty(x.shape, dtype=x.dtype, device=dev)
    flat_h, flat_d = x.reshape(-1), out.reshape(-1)
    row = (1 << 20) // x.element_size()                     # 1-MiB rows, pitch = row length
    n_full = flat_h.numel() // row
    try:
        upload_rows(flat_h[:n_full * row].view(n_full, row), flat_d[:n_full * row].view(n_full, row))
        tail = flat_h.numel() - n_full * row
        if tail:
            upload_rows(flat_h[n_full * row:].view(1, tail), flat_d[n_full * row:].view(1, tail))
    except _lib.S3HipError:                                 # no page-locked staging memory on this host: plain copy
        flat_d.copy_(flat_h)
    synchronize()                                           # the caller may release or overwrite x
    return out


def knn_occupancy(k, dim):
    """target points per bucket for a k-nearest search: the sphere that holds k neighbours should span about 1.5 bucket
    sides -- smaller buckets waste fewer visited points, larger ones need fewer rings.  Measured on MI355X (5*10^6
    uniform 3-D points, k = 26, 360 000 predictions, before the pruning of far buckets): occupancy 8 / 4 / 2 / 1.5 / 1 ->
    3.58 / 2.94 / 2.63 / 2.36 / 3.60 ms; with pruning 2 / 1.5 / 1 -> 2.03 / 2.01 / 2.91 ms"""
    return max(1.0, k / (13.0 if dim == 3 else 6.7))


class KnnIndex:
    """Bucket-grid KNN index over the original CFD points (replaces sklearn's kd-tree, s_cube.py:161-163,
    export.py:120,423)."""

    def __init__(self, points, target_occupancy=0.0):
        pts = to_device(points, pt.float64)
        assert pts.dim() == 2 and pts.shape[1] in (2, 3), "points must be [N, 2|3]"
        self.n, self.dim = int(pts.shape[0]), int(pts.shape[1])
        self._handle = C.c_void_p(0)
        check(_lib.hip_lib().s3_knn_create(_ptr(pts), self.n, self.dim, float(target_occupancy), _stream(),
                                           C.byref(self._handle)), "s3_knn_create")
        self._has_values = False
        nb, nr = C.c_int64(0), C.c_int64(0)
        check(_lib.hip_lib().s3_knn_info(self._handle, C.byref(nb), C.byref(nr)), "s3_knn_info")
        self.n_buckets, self.n_refined_buckets = nb.value, nr.value

    def close(self):
        if getattr(self, "_handle", None) is not None and self._handle.value:
            _lib.hip_lib().s3_knn_destroy(self._handle)
            self._handle = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown
            pass

    def set_values(self, y):
        y = to_device(y, pt.float64)
        assert y.numel() == self.n
        check(_lib.hip_lib().s3_knn_set_values(self._handle, _ptr(y), _stream()), "s3_knn_set_values")
        pt.cuda.current_stream().synchronize()      # y may be freed by the caller
        self._has_values = True

    def query(self, q, k):
        """-> (idx int32 [nq,k], dist f64 [nq,k]) on the device, ascending in (dist, idx)."""
        q = to_device(q, pt.float64)
        nq = int(q.shape[0])
        idx = pt.empty((nq, k), dtype=pt.int32, device=q.device)
        dist = pt.empty((nq, k), dtype=pt.float64, device=q.device)
        check(_lib.hip_lib().s3_knn_query(self._handle, _ptr(q), nq, int(k), _ptr(idx), _ptr(dist), _stream()),
              "s3_knn_query")
        return idx, dist

    def predict(self, q, k):
        q = to_device(q, pt.float64)
        nq = int(q.shape[0])
        out = pt.empty(nq, dtype=pt.float64, device=q.device)
        check(_lib.hip_lib().s3_idw_predict(self._handle, _ptr(q), nq, int(k), _ptr(out), _stream()), "s3_idw_predict")
        return out

    @property
    def handle(self):
        return self._handle


def idw_weights(dist):
    w = pt.empty_like(dist)
    check(_lib.hip_lib().s3_idw_weights(_ptr(dist), int(dist.shape[0]), int(dist.shape[1]), _ptr(w), _stream()),
          "s3_idw_weights")
    return w


def interp(w, idx, data, out=None):
    """out[c, ...] = sum_m w[c,m] * data[idx[c,m], ...]   (export.py:446-468).  w f64 [nc,k], idx int32 [nc,k],
    data f32/f64 [n_src, ...] -- all on the device; returns f64 [nc, ...] on the device."""
    if not (w.dtype == pt.float64 and idx.dtype == pt.int32 and data.dtype in DTYPE_CODE and w.shape == idx.shape):
        raise TypeError("interp: w must be float64 [nc,k], idx int32 [nc,k], data float32/float64")
    nc, k = int(w.shape[0]), int(w.shape[1])
    n_src = int(data.shape[0])
    row_len = int(np.prod(data.shape[1:])) if data.dim() > 1 else 1
    if out is None:
        out = pt.empty((nc,) + tuple(data.shape[1:]), dtype=pt.float64, device=data.device)
    check(_lib.hip_lib().s3_interp(_ptr(w), _ptr(idx), nc, k, _ptr(data), DTYPE_CODE[data.dtype], n_src, row_len,
                                   _ptr(out), _stream()), "s3_interp")
    return out


def idw_weights_exact(dist):
    """scikit-learn's ``weights="distance"`` as ``KNeighborsRegressor.predict`` applies them (s3_idw_weights_exact): a row with
    zero distances gets 1 at the zeros and 0 elsewhere, any other row ``1 / dist``; rows normalised to sum 1.  Not
    ``idw_weights``, whose clamp at 1e-12 is the export's rule."""
    if not (dist.dtype == pt.float64 and dist.dim() == 2):
        raise TypeError("idw_weights_exact: dist must be float64 [n, k]")
    w = pt.empty_like(dist)
    check(_lib.hip_lib().s3_idw_weights_exact(_ptr(dist), int(dist.shape[0]), int(dist.shape[1]), _ptr(w), _stream()),
          "s3_idw_weights_exact")
    return w


RECON_BLOCK = 1024          # S3_RECON_BLOCK (s3hip.h): points per partial column sum


def _pitched_rows(t, who):
    """(row_len, stride in elements) of a device tensor whose leading axis is the row axis: contiguous [n, ...], or a 2-D column
    slice ``buf[:, :L]`` of a wider buffer"""
    if not t.is_cuda or t.dtype not in DTYPE_CODE or t.dim() < 1:
        raise TypeError(f"{who}: float32 / float64 device tensor [n, ...] required")
    layout = _row_layout(t)
    if layout is None:
        raise TypeError(f"{who}: rows must be contiguous (a row pitch is allowed for a 2-D tensor)")
    return layout


def recon_error(w, idx, grid, orig, rows=None, scale=None, mean=None, m2=None):
    """the fused reconstruction-error launch (s3_recon_error).  Point i of the launch is original row ``rows[i]`` (``rows`` None:
    row i); ``w`` f64 / ``idx`` int32 [n, k] (rows of ``grid``) and ``scale`` f64 [n] are in launch order.  With
    ``fit = sum_m w * grid[idx]``, ``d = scale * (fit - orig)`` and ``ref = scale * orig`` it returns
    ``(mean, m2, colsum)``: mean and centred second moment of ``|d|`` over each original row (f64 [n_orig], original order;
    written into ``mean`` / ``m2`` when given) and ``colsum`` f64 [2, row_len] = (sum_i d^2, sum_i ref^2) per column.
    ``grid`` [nc, ...] contiguous, ``orig`` [n_orig, ...] contiguous or a pitched 2-D view; nothing of size n x row_len is
    written."""
    if not (w.dtype == pt.float64 and idx.dtype == pt.int32 and w.dim() == 2 and w.shape == idx.shape):
        raise TypeError("recon_error: w must be float64 [n, k], idx int32 [n, k]")
    n, k = int(w.shape[0]), int(w.shape[1])
    row_len, g_stride = _pitched_rows(grid, "recon_error(grid)")
    o_len, o_stride = _pitched_rows(orig, "recon_error(orig)")
    if g_stride != row_len or o_len != row_len or row_len < 1:
        raise TypeError("recon_error: grid must be contiguous and grid / orig rows of one length >= 1")
    nc, n_orig = int(grid.shape[0]), int(orig.shape[0])
    _launch_rows(rows, n, "recon_error")
    if (rows is None and n_orig != n) or n_orig < n or nc < 1:
        raise TypeError("recon_error: one original row per point required (or a row list)")
    if scale is not None and not (scale.dtype == pt.float64 and scale.numel() == n):
        raise TypeError("recon_error: scale must be float64 [n]")
    dev = w.device
    mean = _out_tensor(mean, (n_orig,), pt.float64, dev, "recon_error", "mean")
    m2 = _out_tensor(m2, (n_orig,), pt.float64, dev, "recon_error", "m2")
    colsum = pt.empty((2, row_len), dtype=pt.float64, device=dev)
    lib = _lib.hip_lib()
    scratch = _scratch(lib.s3_recon_error_scratch_bytes(n, row_len), dev)
    check(lib.s3_recon_error(_ptr(w), _ptr(idx), n, k, _ptr(grid), DTYPE_CODE[grid.dtype], nc, C.c_void_p(orig.data_ptr()),
                             DTYPE_CODE[orig.dtype], n_orig, o_stride, row_len, _ptr(rows), _ptr(scale), _ptr(mean), _ptr(m2),
                             _ptr(colsum), _ptr(scratch), _stream()), "s3_recon_error")
    return mean, m2, colsum


GRAD_MODES = {"gradient": 0, "magnitude": 1, "divergence": 2, "vorticity": 3, "vorticity_magnitude": 4, "q": 5}    # S3_GRAD_* (s3hip.h)
GRAD_MAX_K = 63             # S3_MAX_K - 1: the search behind a stencil asks for one neighbour more, the point itself


def grad_n_out(mode, dim, n_comp):
    """values per point and snapshot of ``grad_apply``'s modes"""
    return {"gradient": n_comp * dim, "magnitude": n_comp, "vorticity": 1 if dim == 2 else 3}.get(mode, 1)


def grad_coeff(points, idx, power=2, rows=None):
    """least-squares gradient coefficients of a cloud (s3_grad_coeff).  ``points`` f64 [n, 2 | 3] and ``idx`` int32 [n, k] on the
    device; entry j of ``idx`` holds the neighbours of point ``rows[j]`` (``rows`` int32 [n] or None: point j), the point itself
    not among them.  -> ``(coef f64 [n, k, dim], flag uint8 [n], n_degenerate)`` in the order of ``idx``: a degenerate row
    (collinear / coplanar / coincident neighbours) has zero coefficients and flag 1."""
    if not (points.is_cuda and points.dtype == pt.float64 and points.dim() == 2 and int(points.shape[1]) in (2, 3)):
        raise TypeError("grad_coeff: points must be a float64 device tensor [n, 2 | 3]")
    n, dim = int(points.shape[0]), int(points.shape[1])
    if not (idx.is_cuda and idx.dtype == pt.int32 and idx.dim() == 2 and int(idx.shape[0]) == n):
        raise TypeError(f"grad_coeff: idx must be an int32 device tensor [{n}, k]")
    _launch_rows(rows, n, "grad_coeff")
    k = int(idx.shape[1])
    coef = pt.empty((n, k, dim), dtype=pt.float64, device=points.device)
    flag = pt.empty(n, dtype=pt.uint8, device=points.device)
    n_deg = C.c_int64(0)
    check(_lib.hip_lib().s3_grad_coeff(_ptr(points), n, dim, _ptr(idx), k, int(power), _ptr(rows), _ptr(coef), _ptr(flag),
                                       C.byref(n_deg), _stream()), "s3_grad_coeff")
    return coef, flag, n_deg.value


def grad_apply(coef, idx, field, mode, rows=None, out=None):
    """the fused gradient launch (s3_grad_apply): ``mode`` is a key of ``GRAD_MODES``.  ``coef`` f64 [n, k, dim] / ``idx`` int32
    [n, k] as ``grad_coeff`` made them (entry j: point ``rows[j]``), ``field`` float32 / float64 on the device: [n] (one snapshot),
    [n, T] (rows may be pitched: read where they lie) or [n, n_comp, T] contiguous.  -> f64 [n, n_out, T] (``grad_n_out``;
    "gradient" is ordered [comp][axis]), written into ``out`` when given.  The kernel takes up to three components per launch:
    a wider field goes in groups, for "gradient" and "magnitude" only."""
    if mode not in GRAD_MODES:
        raise ValueError(f"grad_apply: unknown mode {mode!r}, expected one of {sorted(GRAD_MODES)}")
    if not (coef.is_cuda and coef.dtype == pt.float64 and coef.dim() == 3 and idx.is_cuda and idx.dtype == pt.int32
            and tuple(idx.shape) == tuple(coef.shape[:2])):
        raise TypeError("grad_apply: coef must be float64 [n, k, dim], idx int32 [n, k], both on the device")
    n, k, dim = (int(v) for v in coef.shape)
    if not (isinstance(field, pt.Tensor) and field.is_cuda and field.dtype in DTYPE_CODE and 1 <= field.dim() <= 3):
        raise TypeError("grad_apply: float32 / float64 device field [n], [n, T] or [n, n_comp, T] required")
    if int(field.shape[0]) != n:
        raise ValueError(f"grad_apply: the field has {int(field.shape[0])} rows, the stencils {n}")
    n_comp, t, in_stride = _field_rows(field, "grad_apply")
    if t < 1 or n_comp < 1:
        raise ValueError(f"grad_apply: empty field {tuple(field.shape)}")
    vector_mode = mode not in ("gradient", "magnitude")
    if vector_mode and n_comp != dim:
        raise ValueError(f"grad_apply: {mode} needs a vector field [n, {dim}, T], got {tuple(field.shape)}")
    _launch_rows(rows, n, "grad_apply")
    n_out = grad_n_out(mode, dim, n_comp)
    out = _out_tensor(out, (n, n_out, t), pt.float64, field.device, "grad_apply")
    lib, item = _lib.hip_lib(), field.element_size()
    per_comp = dim if mode == "gradient" else 1
    for c0, group in _component_groups(n_comp):
        check(lib.s3_grad_apply(_ptr(coef), _ptr(idx), n, k, dim, C.c_void_p(field.data_ptr() + c0 * t * item), DTYPE_CODE[field.dtype],
                                group, t, in_stride, _ptr(rows), GRAD_MODES[mode], C.c_void_p(out.data_ptr() + c0 * per_comp * t * 8),
                                n_out * t, _stream()), "s3_grad_apply")
    return out


SAMPLE_MODES = {"cell": 0, "linear": 1}     # S3_SAMPLE_* (s3hip.h)


class CellIndex:
    """what ``cell_index`` made of a grid: the sorted Morton ranges of its leaves (``starts`` / ``ends`` int64 holding the unsigned
    keys, ``ids`` int32: the cell of each range), the lattice they live on (``origin`` float64 [3] on the host, ``h_min``,
    ``depth``) and the grid itself (``centers`` f64 [n, dim], ``levels`` int32 [n], ``width``), all arrays on the device"""

    def __init__(self, centers, levels, width, starts, ends, ids, origin, h_min, depth):
        for t in (centers, levels, starts, ends, ids):
            _ptr(t)                                 # (device-resident and contiguous: checked here once, not in every launch)
        self.centers, self.levels, self.width = centers, levels, float(width)
        self.starts, self.ends, self.ids = starts, ends, ids
        self.origin, self.h_min, self.depth = origin, float(h_min), int(depth)
        self.n_cells, self.dim = int(centers.shape[0]), int(centers.shape[1])
        self._origin = (C.c_double * 3)(*origin)

    def s3_grid(self, faces=None):
        """the ``s3_grid`` of one call (``faces``: checked by the caller, ``_grid_faces``): nothing is kept of it, the tensors here and
        ``faces`` own the memory it points to.  Plain ``data_ptr()`` reads: a launch-bound caller pays for every microsecond here."""
        return _lib.S3Grid(self.starts.data_ptr(), self.ends.data_ptr(), self.ids.data_ptr(), self.dim, self.depth, self._origin, self.h_min,
                           self.n_cells, self.centers.data_ptr(), self.levels.data_ptr(), self.width, None if faces is None else faces.data_ptr())


def _cell_index(index, who):
    if not isinstance(index, CellIndex):
        raise TypeError(f"{who}: index must be what cell_index returned")
    return index


def _grid_faces(faces, who, index=None):
    """-> (n_cells, dim) of ``faces`` as the kernels index them: contiguous int32 [n_cells, 2^dim] on the device, the cells and the
    dimension those of ``index`` where one is given"""
    shape = f"[{index.n_cells}, {1 << index.dim}]" if index is not None else "[n_cells, 4 | 8]"
    if not (isinstance(faces, pt.Tensor) and faces.is_cuda and faces.dtype == pt.int32 and faces.is_contiguous() and faces.dim() == 2
            and (int(faces.shape[1]) in (4, 8) if index is None else tuple(faces.shape) == (index.n_cells, 1 << index.dim))):
        raise TypeError(f"{who}: faces must be a contiguous int32 device tensor {shape}")
    return int(faces.shape[0]), 2 if int(faces.shape[1]) == 4 else 3


def cell_index(centers, levels, width):
    """the cell index of a generated grid (s3_cell_index): ``centers`` float64 [n, 2 | 3] and ``levels`` int32 / int64 [n] or [n, 1]
    on the device, ``width`` the size of the initial cell.  -> ``CellIndex``.  ``ValueError`` with the counts where the grid is no
    set of disjoint dyadic boxes on one lattice: cells off the lattice, misaligned cells, overlapping cells, or more than 63 key
    bits (dim * max level)."""
    if not (isinstance(centers, pt.Tensor) and centers.is_cuda and centers.dtype == pt.float64 and centers.dim() == 2
            and int(centers.shape[1]) in (2, 3)):
        raise TypeError("cell_index: centers must be a float64 device tensor [n, 2 | 3]")
    n, dim = int(centers.shape[0]), int(centers.shape[1])
    if not (isinstance(levels, pt.Tensor) and levels.is_cuda and levels.dtype in (pt.int32, pt.int64) and levels.numel() == n):
        raise TypeError(f"cell_index: levels must be an int32 / int64 device tensor with {n} entries")
    if n < 1:
        raise ValueError("cell_index: a grid without cells")
    width = float(width)
    if not (width > 0.0 and np.isfinite(width)):
        raise ValueError(f"cell_index: width must be a positive size, got {width!r}")
    centers = centers.contiguous()
    levels = levels.reshape(n).to(pt.int32).contiguous()
    starts = pt.empty(n, dtype=pt.int64, device=centers.device)
    ends, ids = pt.empty_like(starts), pt.empty(n, dtype=pt.int32, device=centers.device)
    grid, refused = _lib.S3Grid(), np.zeros(4, dtype=np.int64)
    lib = _lib.hip_lib()
    rc = lib.s3_cell_index(_ptr(centers), _ptr(levels), n, dim, width, _ptr(starts), _ptr(ends), _ptr(ids), C.byref(grid),
                           C.c_void_p(refused.ctypes.data), _stream())
    if rc == -1 and refused.any():
        raise ValueError(f"cell_index: the grid of {n} cells is refused: " + lib.s3_last_error().decode(errors="replace")
                         + f" (off the lattice {refused[0]}, misaligned {refused[1]}, overlapping {refused[2]}, key bits {refused[3]})")
    check(rc, "s3_cell_index")
    return CellIndex(centers, levels, width, starts, ends, ids, np.array(grid.origin, dtype=np.float64), grid.h_min, grid.depth)


def _query_points(points, dim, who):
    if not (isinstance(points, pt.Tensor) and points.is_cuda and points.dtype == pt.float64 and points.dim() == 2
            and int(points.shape[1]) == dim and points.is_contiguous()):
        raise TypeError(f"{who}: points must be a contiguous float64 device tensor [nq, {dim}]")
    return int(points.shape[0])


def cell_locate(index, points, rows=None, out=None):
    """the cell that holds each point (s3_cell_locate): ``points`` float64 [nq, dim] on the device -> int32 [nq] in the caller's
    cell numbering, -1 where no cell holds the point (outside the domain, inside a body, NaN / infinite coordinates).  A point on
    a face belongs to the upper cell.  ``rows`` int32 [nq]: the order in which the points are launched (``spatial_order``)."""
    nq = _query_points(points, _cell_index(index, "cell_locate").dim, "cell_locate")
    _launch_rows(rows, nq, "cell_locate")
    out = _out_tensor(out, (nq,), pt.int32, points.device, "cell_locate")
    check(_lib.hip_lib().s3_cell_locate(C.byref(index.s3_grid()), _ptr(points), nq, _ptr(rows), _ptr(out), _stream()), "s3_cell_locate")
    return out


def cell_sample(ids, field, mode="cell", rows=None, out=None, index=None, points=None, faces=None):
    """the field at located points (s3_cell_sample).  ``ids`` int32 [nq] as ``cell_locate`` returned them; ``field`` float32 / float64
    on the device: [rows] (one snapshot), [rows, T] (rows may be pitched: read where they lie) or [rows, n_comp, T] contiguous.
    -> f64 [nq, n_comp, T], written into ``out`` when given; rows with id -1 are NaN.

    ``mode="cell"``: the field has one row per cell, the result is a bit-exact copy of the row of the containing cell.
    ``mode="linear"``: the field has one row per grid NODE; ``index`` (the ``CellIndex``), ``points`` float64 [nq, dim] and
    ``faces`` int32 [n_cells, 2^dim] (the corner nodes of every cell) are required, the result is the multilinear blend of the
    containing cell's corner values.  ``rows`` int32 [nq]: the launch order.  The kernel takes up to three components per launch:
    a wider field goes in groups."""
    if mode not in SAMPLE_MODES:
        raise ValueError(f"cell_sample: unknown mode {mode!r}, expected one of {sorted(SAMPLE_MODES)}")
    if not (isinstance(ids, pt.Tensor) and ids.is_cuda and ids.dtype == pt.int32 and ids.dim() == 1 and ids.is_contiguous()):
        raise TypeError("cell_sample: ids must be a contiguous int32 device tensor [nq]")
    nq = int(ids.numel())
    if not (isinstance(field, pt.Tensor) and field.is_cuda and field.dtype in DTYPE_CODE and 1 <= field.dim() <= 3):
        raise TypeError("cell_sample: float32 / float64 device field [rows], [rows, T] or [rows, n_comp, T] required")
    n_comp, t, in_stride = _field_rows(field, "cell_sample")
    n_rows = int(field.shape[0])
    if t < 1 or n_comp < 1 or n_rows < 1:
        raise ValueError(f"cell_sample: empty field {tuple(field.shape)}")
    _launch_rows(rows, nq, "cell_sample")
    grid = None
    if mode == "linear":
        if index is None or points is None or faces is None:
            raise ValueError("cell_sample: mode 'linear' needs index, points and faces")
        if _query_points(points, _cell_index(index, "cell_sample").dim, "cell_sample") != nq:
            raise ValueError(f"cell_sample: {int(points.shape[0])} points for {nq} ids")
        _grid_faces(faces, "cell_sample", index)
        grid = C.byref(index.s3_grid(faces))
    else:
        points = None
    out = _out_tensor(out, (nq, n_comp, t), pt.float64, field.device, "cell_sample")
    lib, item = _lib.hip_lib(), field.element_size()
    for c0, group in _component_groups(n_comp):
        check(lib.s3_cell_sample(SAMPLE_MODES[mode], _ptr(ids), nq, _ptr(rows), C.c_void_p(field.data_ptr() + c0 * t * item),
                                 DTYPE_CODE[field.dtype], group, t, in_stride, n_rows, grid, _ptr(points),
                                 C.c_void_p(out.data_ptr() + c0 * t * 8), n_comp * t, _stream()), "s3_cell_sample")
    return out


TRACE_STEP_RULES = {"time": 0, "cell": 1}                                           # S3_TRACE_STEP_* (s3hip.h)
TRACE_STATUS = {"DONE": 0, "LEFT": 1, "STAGNANT": 2, "SEED_OUTSIDE": 3}             # S3_TRACE_* (s3hip.h)


def _trace(mode, who, index, faces, velocity, seeds, order, n_steps, substeps, every, rule, step, direction, paths, length, status, cells):
    dim = _cell_index(index, who).dim
    _grid_faces(faces, who, index)
    if not (isinstance(velocity, pt.Tensor) and velocity.is_cuda and velocity.dtype in DTYPE_CODE and velocity.dim() == 3
            and velocity.is_contiguous()):
        raise TypeError(f"{who}: velocity must be a contiguous float32 / float64 device tensor [n_nodes, {dim}, T]")
    n_nodes, n_comp, t = (int(v) for v in velocity.shape)
    if n_comp != dim:
        raise ValueError(f"{who}: a velocity on a {dim}-D grid has {dim} components, got {n_comp}")
    if n_nodes < 1 or t < (2 if mode else 1):
        raise ValueError(f"{who}: velocity {tuple(velocity.shape)} has too few {'snapshots for a pathline (two at least)' if n_nodes else 'nodes'}")
    n_seeds = _query_points(seeds, dim, who)
    _launch_rows(order, n_seeds, who)
    if rule not in TRACE_STEP_RULES:
        raise ValueError(f"{who}: unknown step rule {rule!r}, expected one of {sorted(TRACE_STEP_RULES)}")
    step = float(step)
    if not (np.isfinite(step) and step > 0.0):
        raise ValueError(f"{who}: the step ({'cfl' if rule == 'cell' else 'dt'}) must be positive and finite, got {step!r}")
    if direction not in (1, -1):
        raise ValueError(f"{who}: direction must be 1 or -1, got {direction!r}")
    if mode:
        if int(substeps) < 1:
            raise ValueError(f"{who}: substeps must be positive, got {substeps}")
        shape, n_out = (n_seeds,), t
    else:
        if int(n_steps) < 1 or int(every) < 1:
            raise ValueError(f"{who}: n_steps and every must be positive, got {n_steps} and {every}")
        if n_seeds * t >= 1 << 31:
            raise ValueError(f"{who}: {n_seeds} seeds x {t} columns are too many particles for one launch")
        shape, n_out = (n_seeds, t), 1 + int(n_steps) // int(every)
    paths = _out_tensor(paths, shape + (n_out, dim), pt.float64, seeds.device, who, "paths")
    length = _out_tensor(length, shape, pt.int32, seeds.device, who, "length")
    status = _out_tensor(status, shape, pt.int32, seeds.device, who, "status")
    cells = _out_tensor(cells, shape, pt.int32, seeds.device, who, "cells")
    check(_lib.hip_lib().s3_trace(mode, C.byref(index.s3_grid(faces)), _ptr(velocity), DTYPE_CODE[velocity.dtype], t, dim * t, n_nodes, _ptr(seeds),
                                  n_seeds, _ptr(order), int(n_steps), int(substeps), int(every), TRACE_STEP_RULES[rule], step, int(direction),
                                  _ptr(paths), _ptr(length), _ptr(status), _ptr(cells), _stream()), "s3_trace")
    return paths, length, status, cells


def trace_stream(index, faces, velocity, seeds, n_steps, step="cell", cfl=0.5, dt=None, direction=1, every=1, order=None,
                 paths=None, length=None, status=None, cells=None):
    """streamlines of every column of a node velocity (s3_trace, S3_TRACE_STREAM).  ``index``: the ``CellIndex`` of the grid; ``faces``
    int32 [n_cells, 2^dim]; ``velocity`` float32 / float64 [n_nodes, dim, T] contiguous; ``seeds`` float64 [n_seeds, dim]; all on the
    device.  ``n_steps`` RK4 steps of ``step="cell"`` (``dt = cfl * h / |v|`` at every step) or ``step="time"`` (fixed ``dt``) in
    ``direction`` 1 | -1; every ``every``-th accepted step is recorded.  ``order`` int32 [n_seeds]: the launch order of the seeds.
    -> (paths f64 [n_seeds, T, 1 + n_steps // every, dim] with the seed in row 0 and NaN rows past the length, length, status
    (``TRACE_STATUS``), cells (the cell of the last position): int32 [n_seeds, T]), written into the tensors given."""
    if step == "time" and dt is None:
        raise ValueError("trace_stream: step 'time' needs dt")
    return _trace(0, "trace_stream", index, faces, velocity, seeds, order, n_steps, 1, every, step, dt if step == "time" else cfl,
                  direction, paths, length, status, cells)


def trace_path(index, faces, velocity, seeds, dt_snapshot, substeps=4, direction=1, order=None, paths=None, length=None, status=None,
               cells=None):
    """pathlines through the snapshots of a node velocity (s3_trace, S3_TRACE_PATH): arguments as ``trace_stream``; ``substeps`` RK4
    steps of ``dt_snapshot / substeps`` per snapshot interval, the velocity blended linearly in time; ``direction`` -1 runs from the
    last column to the first.  ``order``: launch the seeds in ``spatial_order``.  -> (paths f64 [n_seeds, T, dim]: the position at
    every snapshot, the seed in column 0 (T - 1 backward), NaN past the length; length, status, cells: int32 [n_seeds])."""
    dt_snapshot = float(dt_snapshot)
    if not (np.isfinite(dt_snapshot) and dt_snapshot > 0.0) or int(substeps) < 1:
        raise ValueError(f"trace_path: dt_snapshot must be positive and finite and substeps positive, got {dt_snapshot!r} and {substeps}")
    return _trace(1, "trace_path", index, faces, velocity, seeds, order, 0, substeps, 1, "time", dt_snapshot / int(substeps), direction,
                  paths, length, status, cells)


RAY_MODES = {"cell": 0, "linear": 1}                                                            # S3_RAY_* (s3rays.h)
RAY_STATUS = {"CROSSED": 0, "MISSED": 1, "BAD_RAY": 2, "TRUNCATED": 3, "BROKEN": 4}            # S3_RAY_* (s3rays.h)
RAY_MAX_STEPS = 1 << 20


def ray_integrate(index, origins, dirs, field, mode="cell", faces=None, t_range=(-np.inf, np.inf), order=None, max_steps=RAY_MAX_STEPS,
                  out=None, length=None, segments=None, status=None):
    """line-of-sight integrals of a grid field (s3_ray_integrate, include/s3rays.h).  ``index``: the ``CellIndex`` of the grid;
    ``origins`` and ``dirs`` float64 [R, dim]: the rays ``x(t) = o + t d``; ``field`` float32 / float64 on the device: [rows] (one
    snapshot), [rows, T] (rows may be pitched: read where they lie) or [rows, n_comp, T] contiguous; ``mode="cell"``: one row per
    cell, the integral is sum value x chord; ``mode="linear"``: one row per grid NODE and ``faces`` int32 [n_cells, 2^dim] required,
    the integral of the multilinear blend, exact per cell.  ``t_range``: the part of every ray that is integrated, in units of its
    parameter; ``order`` int32 [R]: the launch order of the rays; a ray still walking after ``max_steps`` blocks is TRUNCATED.
    -> (out f64 [R, n_comp, T], length f64 [R]: the length of the ray inside cells, segments int32 [R]: the cells crossed, status
    int32 [R]: ``RAY_STATUS``), written into the tensors given.  The kernel takes up to three components per launch: a wider field
    goes in groups."""
    if mode not in RAY_MODES:
        raise ValueError(f"ray_integrate: unknown mode {mode!r}, expected one of {sorted(RAY_MODES)}")
    dim = _cell_index(index, "ray_integrate").dim
    n_rays = _query_points(origins, dim, "ray_integrate")
    if _query_points(dirs, dim, "ray_integrate") != n_rays:
        raise ValueError(f"ray_integrate: {int(dirs.shape[0])} directions for {n_rays} origins")
    if not (isinstance(field, pt.Tensor) and field.is_cuda and field.dtype in DTYPE_CODE and 1 <= field.dim() <= 3):
        raise TypeError("ray_integrate: float32 / float64 device field [rows], [rows, T] or [rows, n_comp, T] required")
    n_comp, t, in_stride = _field_rows(field, "ray_integrate")
    n_rows = int(field.shape[0])
    if t < 1 or n_comp < 1 or n_rows < 1:
        raise ValueError(f"ray_integrate: empty field {tuple(field.shape)}")
    if mode == "linear":
        if faces is None:
            raise ValueError("ray_integrate: mode 'linear' needs faces")
        _grid_faces(faces, "ray_integrate", index)
    else:
        faces = None
    _launch_rows(order, n_rays, "ray_integrate")
    t_min, t_max = (float(v) for v in t_range)
    if not t_min <= t_max:
        raise ValueError(f"ray_integrate: t_range {t_range!r} is no range of the ray parameter")
    if int(max_steps) < 1:
        raise ValueError(f"ray_integrate: max_steps must be positive, got {max_steps}")
    if n_rays * t >= 1 << 31:
        raise ValueError(f"ray_integrate: {n_rays} rays x {t} columns are too many lanes for one launch")
    out = _out_tensor(out, (n_rays, n_comp, t), pt.float64, field.device, "ray_integrate")
    length = _out_tensor(length, (n_rays,), pt.float64, field.device, "ray_integrate", "length")
    segments = _out_tensor(segments, (n_rays,), pt.int32, field.device, "ray_integrate", "segments")
    status = _out_tensor(status, (n_rays,), pt.int32, field.device, "ray_integrate", "status")
    lib, item, grid = _lib.hip_lib(), field.element_size(), C.byref(index.s3_grid(faces))
    for c0, group in _component_groups(n_comp):
        check(lib.s3_ray_integrate(RAY_MODES[mode], grid, _ptr(origins), _ptr(dirs), n_rays, _ptr(order), t_min, t_max, int(max_steps),
                                   C.c_void_p(field.data_ptr() + c0 * t * item), DTYPE_CODE[field.dtype], group, t, in_stride, n_rows,
                                   C.c_void_p(out.data_ptr() + c0 * t * 8), n_comp * t, _ptr(length), _ptr(segments), _ptr(status), _stream()),
              "s3_ray_integrate")
    return out, length, segments, status


ISO_COUNT_BYTES = 256 << 20         # the largest count array [T_b, n_cells] int32 of one isosurface launch
ISO_MAX_PRIMITIVES = {2: 2, 3: 12}  # per cell and snapshot


def _iso_inputs(field, faces, level, who):
    """-> (field as [n_nodes, T], T, in_stride, n_cells, dim, level)"""
    if not (isinstance(field, pt.Tensor) and field.is_cuda and field.dtype in DTYPE_CODE and 1 <= field.dim() <= 2):
        raise TypeError(f"{who}: float32 / float64 device field [n_nodes] or [n_nodes, T] required")
    if field.dim() == 1:
        field = field.contiguous().view(-1, 1)
    _, t, in_stride = _field_rows(field, who, 2)
    if t < 1 or int(field.shape[0]) < 1:
        raise ValueError(f"{who}: empty field {tuple(field.shape)}")
    n_cells, dim = _grid_faces(faces, who)
    level = float(level)
    if not np.isfinite(level):
        raise ValueError(f"{who}: the level must be finite, got {level!r}")
    return field, t, in_stride, n_cells, dim, level


def iso_count(field, faces, level, out=None):
    """primitives of the isosurface (3-D: triangles) or contour (2-D: segments) per snapshot and cell (s3_iso_count): ``field``
    float32 / float64 [n_nodes] or [n_nodes, T] on the device (rows may be pitched: read where they lie), ``faces`` int32
    [n_cells, 2^dim].  -> int32 [T, n_cells], written into ``out`` when given (a flat tensor with room to spare is taken)."""
    field, t, in_stride, n_cells, dim, level = _iso_inputs(field, faces, level, "iso_count")
    out = _out_tensor(out, (t, n_cells), pt.int32, field.device, "iso_count", at_least=True)
    check(_lib.hip_lib().s3_iso_count(C.c_void_p(field.data_ptr()), DTYPE_CODE[field.dtype], t, in_stride,
                                      int(field.shape[0]), _ptr(faces), n_cells, dim, level, _ptr(out), _stream()), "s3_iso_count")
    return out


def iso_emit(field, faces, level, nodes, offsets, capacity, verts=None, edges=None, frac=None, cells=None):
    """the primitives themselves (s3_iso_emit): ``offsets`` int32 [T, n_cells] is the exclusive scan of what ``iso_count`` gave
    for the same arguments, ``nodes`` float64 [n_nodes, dim], ``capacity`` the primitives the outputs have room for (nothing is
    written past it).  -> (verts f64 [capacity, dim, dim], edges int32 [capacity, dim, 2], frac f64 [capacity, dim], cells int32
    [capacity]), ordered by (snapshot, cell, simplex, primitive of the simplex)."""
    field, t, in_stride, n_cells, dim, level = _iso_inputs(field, faces, level, "iso_emit")
    n_nodes, capacity = int(field.shape[0]), int(capacity)
    if not (isinstance(nodes, pt.Tensor) and nodes.is_cuda and nodes.dtype == pt.float64 and nodes.is_contiguous() and tuple(nodes.shape) == (n_nodes, dim)):
        raise TypeError(f"iso_emit: nodes must be a contiguous float64 device tensor [{n_nodes}, {dim}]")
    if not (isinstance(offsets, pt.Tensor) and offsets.is_cuda and offsets.dtype == pt.int32 and offsets.is_contiguous() and offsets.numel() >= t * n_cells):
        raise TypeError(f"iso_emit: offsets must be a contiguous int32 device tensor of {t} x {n_cells} entries")
    if capacity < 0:
        raise ValueError(f"iso_emit: capacity {capacity}")
    dev = field.device
    verts = _out_tensor(verts, (capacity, dim, dim), pt.float64, dev, "iso_emit", "verts", at_least=True)
    edges = _out_tensor(edges, (capacity, dim, 2), pt.int32, dev, "iso_emit", "edges", at_least=True)
    frac = _out_tensor(frac, (capacity, dim), pt.float64, dev, "iso_emit", "frac", at_least=True)
    cells = _out_tensor(cells, (capacity,), pt.int32, dev, "iso_emit", "cells", at_least=True)
    check(_lib.hip_lib().s3_iso_emit(C.c_void_p(field.data_ptr()), DTYPE_CODE[field.dtype], t, in_stride, n_nodes, _ptr(faces), n_cells, dim, level,
                                     _ptr(nodes), _ptr(offsets), capacity, _ptr(verts), _ptr(edges), _ptr(frac), _ptr(cells), _stream()), "s3_iso_emit")
    return verts, edges, frac, cells


def iso_batch_columns(n_cells, dim, count_bytes=ISO_COUNT_BYTES):
    """the snapshots one launch may take: the count array [T_b, n_cells] int32 stays under ``count_bytes`` and
    max primitives * n_cells * T_b under 2^31, so that the int32 offsets cannot overflow"""
    n_cells = max(int(n_cells), 1)
    return max(1, min(int(count_bytes) // (4 * n_cells), ((1 << 31) - 1) // (ISO_MAX_PRIMITIVES[dim] * n_cells)))


def iso_extract(field, faces, nodes, level, count_only=False, count_bytes=ISO_COUNT_BYTES):
    """count, scan (s3_exclusive_scan, in place), read back the totals, emit -- in batches of ``iso_batch_columns`` snapshots.
    -> (offsets int64 numpy [T + 1], verts, edges, frac, cells) as ``iso_emit`` gives them, with exactly offsets[-1] primitives;
    ``count_only``: (offsets,) after the first pass and the scan alone."""
    field, t, _, n_cells, dim, level = _iso_inputs(field, faces, level, "iso_extract")
    lib, dev = _lib.hip_lib(), field.device
    offsets, parts = [np.zeros(1, dtype=np.int64)], []
    step = iso_batch_columns(n_cells, dim, count_bytes)
    for c0 in range(0, t, step):
        window = field[:, c0:c0 + step]
        t_b = int(window.shape[1])
        n = t_b * n_cells
        scan = pt.empty(n + 1, dtype=pt.int32, device=dev)                      # one entry more: its scan is the total
        scan[n:].zero_()
        if n_cells:
            iso_count(window, faces, level, out=scan)
        else:
            scan.zero_()
        check(lib.s3_exclusive_scan(_ptr(scan), _ptr(scan), n + 1, 4, _stream()), "s3_exclusive_scan")
        starts = scan[::max(n_cells, 1)][:t_b + 1] if n_cells else scan.new_zeros(t_b + 1)
        starts = starts.cpu().numpy().astype(np.int64)                          # (waits for the stream)
        offsets.append(offsets[-1][-1] + starts[1:])
        if not count_only:
            parts.append(iso_emit(window, faces, level, nodes, scan, int(starts[-1])))
    offsets = np.concatenate(offsets)
    if count_only:
        return (offsets,)
    return (offsets,) + tuple(p[0] if len(parts) == 1 else pt.cat(p) for p in zip(*parts))


REGION_PHASES = {"init": 1, "hook": 2, "flatten": 4}     # S3_REGION_* (s3hip.h)
REGION_PAIR_BYTES = 256 << 20                           # the largest (key, cell) array [T_b, n_cells] of one table launch: 12 bytes a pair
REGION_FIELDS = ("label", "n_cells", "volume", "centroid", "lo", "hi", "integral", "g_min", "g_max")


def cell_neighbours(index, out=None):
    """the face neighbours of every cell (s3_cell_neighbours): int32 [n_cells, 2 * dim], face ``2 * axis + side`` (side 0: the lower
    face) holds the same-or-coarser leaf across it or -1 (the domain edge, a body or a hole, finer cells).  Every pair of cells that
    share a face stands in the table once from the finer side, and from both sides at equal level."""
    _cell_index(index, "cell_neighbours")
    out = _out_tensor(out, (index.n_cells, 2 * index.dim), pt.int32, index.centers.device, "cell_neighbours")
    check(_lib.hip_lib().s3_cell_neighbours(C.byref(index.s3_grid()), _ptr(out), _stream()), "s3_cell_neighbours")
    return out


def _cell_rows(t, n_cells, dtypes, who, what):
    """-> (T, pitch in elements) of a device tensor [n_cells] or [n_cells, T] of one of ``dtypes`` whose rows are read where they lie"""
    if not (isinstance(t, pt.Tensor) and t.is_cuda and t.dtype in dtypes and 1 <= t.dim() <= 2):
        raise TypeError(f"{who}: {what} must be a device tensor [n_cells] or [n_cells, T] of {' / '.join(str(d) for d in dtypes)}")
    if int(t.shape[0]) != n_cells:
        raise ValueError(f"{who}: {what} has {int(t.shape[0])} rows, the grid {n_cells} cells")
    layout = _row_layout(t)
    if layout is None:
        raise TypeError(f"{who}: the rows of {what} must be contiguous (a row pitch is allowed for a 2-D tensor)")
    if layout[0] < 1 or n_cells < 1:
        raise ValueError(f"{who}: empty {what} {tuple(t.shape)}")
    return layout


def _neighbour_table(nbr, who):
    if not (isinstance(nbr, pt.Tensor) and nbr.is_cuda and nbr.dtype == pt.int32 and nbr.is_contiguous() and nbr.dim() == 2
            and int(nbr.shape[1]) in (4, 6)):
        raise TypeError(f"{who}: neighbours must be a contiguous int32 device tensor [n_cells, 4 | 6]")
    return int(nbr.shape[0]), int(nbr.shape[1]) // 2


def region_label(field, neighbours, lo=-np.inf, hi=np.inf, order=None, out=None, phases=("init", "hook", "flatten")):
    """connected regions of ``lo <= field <= hi`` in every column (s3_region_label).  ``field`` float32 / float64 [n_cells] or
    [n_cells, T] on the device (rows may be pitched: read where they lie), ``neighbours`` what ``cell_neighbours`` gave.  -> int32
    [n_cells, T]: -1 where the cell is out (NaN is out), otherwise the smallest cell id of the face-connected in-cells; written into
    ``out`` when given (int32, rows may be pitched).  ``order`` int32 [n_cells]: the order in which the hooking launch takes the cells
    (``spatial_order`` of the centres).  ``phases``: single launches, for measurements."""
    n_cells, dim = _neighbour_table(neighbours, "region_label")
    t, in_stride = _cell_rows(field, n_cells, tuple(DTYPE_CODE), "region_label", "field")
    lo, hi = float(lo), float(hi)
    if np.isnan(lo) or np.isnan(hi):
        raise ValueError(f"region_label: the bounds must not be NaN, got {lo!r} and {hi!r}")
    _launch_rows(order, n_cells, "region_label")
    code = 0
    for p in phases:
        if p not in REGION_PHASES:
            raise ValueError(f"region_label: unknown phase {p!r}, expected some of {sorted(REGION_PHASES)}")
        code |= REGION_PHASES[p]
    if not code:
        raise ValueError("region_label: no phase")
    if out is None:
        out = pt.empty((n_cells, t), dtype=pt.int32, device=field.device)
    if out.dim() == 1 and t == 1:
        out = out.view(-1, 1)
    if out.dim() != 2 or int(out.shape[1]) != t:
        raise ValueError(f"region_label: out must be [{n_cells}, {t}], got {tuple(out.shape)}")
    _, out_stride = _cell_rows(out, n_cells, (pt.int32,), "region_label", "out")
    check(_lib.hip_lib().s3_region_label(C.c_void_p(field.data_ptr()), DTYPE_CODE[field.dtype], t, in_stride, _ptr(neighbours), n_cells, dim, lo, hi,
                                         _ptr(order), code, C.c_void_p(out.data_ptr()), out_stride, _stream()), "s3_region_label")
    return out


def region_batch_columns(n_cells, pair_bytes=REGION_PAIR_BYTES):
    """the snapshots one table launch may take: its (key, cell) pairs stay under ``pair_bytes`` and n_cells * T_b under 2^31 - 1"""
    n_cells = max(int(n_cells), 1)
    return max(1, min(int(pair_bytes) // (12 * n_cells), ((1 << 31) - 2) // n_cells))


def region_table(labels, index, weight=None, pair_bytes=REGION_PAIR_BYTES):
    """the regions of ``labels`` int32 [n_cells, T] (what ``region_label`` gave; rows may be pitched): count (s3_region_count), scan
    (s3_exclusive_scan, in place), read back the totals, emit (s3_region_emit) -- in batches of ``region_batch_columns`` snapshots.
    ``index``: the ``CellIndex`` of the grid; ``weight``: a second cell field g like the field of ``region_label``, or None.
    -> dict: ``offsets`` int64 numpy [T + 1] (column t owns the regions [offsets[t], offsets[t + 1]), by ascending label) and on the
    device ``label`` int32 [R], ``n_cells`` int64 [R], ``volume`` f64 [R], ``centroid`` / ``lo`` / ``hi`` f64 [R, dim], ``integral`` /
    ``g_min`` / ``g_max`` f64 [R] (None without ``weight``).  Sums in a fixed order: equal inputs give equal bits."""
    n_cells, dim = _cell_index(index, "region_table").n_cells, index.dim
    if isinstance(labels, pt.Tensor) and labels.dim() == 1:
        labels = labels.contiguous().view(-1, 1)
    t, _ = _cell_rows(labels, n_cells, (pt.int32,), "region_table", "labels")
    if weight is not None:
        if isinstance(weight, pt.Tensor) and weight.dim() == 1:
            weight = weight.contiguous().view(-1, 1)
        if _cell_rows(weight, n_cells, tuple(DTYPE_CODE), "region_table", "weight")[0] != t:
            raise ValueError(f"region_table: weight has {int(weight.shape[1])} columns, the labels {t}")
    lib, dev, grid = _lib.hip_lib(), labels.device, C.byref(index.s3_grid())
    offsets, parts = [np.zeros(1, dtype=np.int64)], []
    step = region_batch_columns(n_cells, pair_bytes)
    for c0 in range(0, t, step):
        window = labels[:, c0:c0 + step]
        t_b, stride = int(window.shape[1]), int(window.stride(0))
        n = t_b * n_cells
        scan = pt.empty(n + 1, dtype=pt.int32, device=dev)                      # one entry more: its scan is the total
        scan[n:].zero_()
        check(lib.s3_region_count(C.c_void_p(window.data_ptr()), t_b, stride, n_cells, _ptr(scan), _stream()), "s3_region_count")
        check(lib.s3_exclusive_scan(_ptr(scan), _ptr(scan), n + 1, 4, _stream()), "s3_exclusive_scan")
        starts = scan[::n_cells].cpu().numpy().astype(np.int64)                 # [t_b + 1] (waits for the stream)
        offsets.append(offsets[-1][-1] + starts[1:])
        r = int(starts[-1])
        part = {"label": pt.empty(r, dtype=pt.int32, device=dev), "n_cells": pt.empty(r, dtype=pt.int64, device=dev),
                "volume": pt.empty(r, dtype=pt.float64, device=dev)}
        part.update((k, pt.empty((r, dim), dtype=pt.float64, device=dev)) for k in ("centroid", "lo", "hi"))
        part.update((k, pt.empty(r, dtype=pt.float64, device=dev) if weight is not None else None) for k in ("integral", "g_min", "g_max"))
        g = None if weight is None else weight[:, c0:c0 + step]
        check(lib.s3_region_emit(C.c_void_p(window.data_ptr()), t_b, stride, grid, _ptr(scan), r,
                                 None if g is None else C.c_void_p(g.data_ptr()), 0 if g is None else DTYPE_CODE[g.dtype],
                                 0 if g is None else int(g.stride(0)), *(_ptr(part[k]) for k in REGION_FIELDS), _stream()), "s3_region_emit")
        parts.append(part)
    table = {"offsets": np.concatenate(offsets)}
    for k in REGION_FIELDS:
        table[k] = None if parts[0][k] is None else (parts[0][k] if len(parts) == 1 else pt.cat([p[k] for p in parts]))
    return table


OVERLAP_PASSES = {"one_key": 0, "by_b": 1, "by_ta": 2}  # S3_OVERLAP_* (s3overlap.h)
OVERLAP_FIELDS = ("src", "dst", "n_cells", "units", "volume")


def overlap_key_bits(n_cells, row_len):
    """(w, tb) of include/s3overlap.h: the bits of a cell id and of a column of one batch.  One key holds (t, a, b) while
    tb + 2 w <= 64"""
    return max(1, (int(n_cells) - 1).bit_length()), (int(row_len) - 1).bit_length()


def _overlap_labels(a, b, index, who):
    """-> (a, b as [n_cells, T], T): two int32 label arrays on the device of one shape whose rows are read where they lie"""
    n_cells = _cell_index(index, who).n_cells
    if isinstance(a, pt.Tensor) and a.dim() == 1:
        a = a.contiguous().view(-1, 1)
    if isinstance(b, pt.Tensor) and b.dim() == 1:
        b = b.contiguous().view(-1, 1)
    t, _ = _cell_rows(a, n_cells, (pt.int32,), who, "a")
    if _cell_rows(b, n_cells, (pt.int32,), who, "b")[0] != t:
        raise ValueError(f"{who}: b has {int(b.shape[1])} columns, a {t}")
    if a.device != b.device:
        raise TypeError(f"{who}: a and b must live on one device")
    return a, b, t


def _overlap_pairs(keys, vals, who):
    if not (isinstance(keys, pt.Tensor) and isinstance(vals, pt.Tensor) and keys.is_cuda and vals.is_cuda and keys.is_contiguous()
            and vals.is_contiguous() and keys.dtype == pt.int64 and vals.dtype == pt.int32 and keys.dim() == 1 and keys.numel() == vals.numel()):
        raise TypeError(f"{who}: contiguous int64 keys and int32 values of one length on the device required")
    return int(keys.numel())


def overlap_count(a, b, index, out=None):
    """count[t][c] = 1 where cell c is in both label arrays at column t (s3_overlap_count; "in": the label names a root of its
    array).  ``a``, ``b`` int32 [n_cells, T] on the device (rows may be pitched; two windows of one allocation are fine).  -> int32
    [T * n_cells], snapshot-major, written into the front of ``out`` when given"""
    a, b, t = _overlap_labels(a, b, index, "overlap_count")
    out = _out_tensor(out, (t * index.n_cells,), pt.int32, a.device, "overlap_count", at_least=True)
    check(_lib.hip_lib().s3_overlap_count(C.byref(index.s3_grid()), C.c_void_p(a.data_ptr()), int(a.stride(0)), C.c_void_p(b.data_ptr()),
                                          int(b.stride(0)), t, _ptr(out), _stream()), "s3_overlap_count")
    return out


def overlap_emit(a, b, index, scan, keys, vals, route="one_key"):
    """one (key, cell) pair per in-both (c, t) at its position ``scan[t][c]`` (s3_overlap_emit): ``scan`` the exclusive scan of what
    ``overlap_count`` gave, ``keys`` int64 / ``vals`` int32 [n_pairs].  ``route``: "one_key" (key (t, a, b)), "by_b" (key (t, b): the
    first of two sort passes) or "by_ta" (re-keys the pairs that are there to (t, a): the second)"""
    a, b, t = _overlap_labels(a, b, index, "overlap_emit")
    if route not in OVERLAP_PASSES:
        raise ValueError(f"overlap_emit: unknown route {route!r}, expected one of {sorted(OVERLAP_PASSES)}")
    n_pairs = _overlap_pairs(keys, vals, "overlap_emit")
    if route != "by_ta" and not (isinstance(scan, pt.Tensor) and scan.is_cuda and scan.dtype == pt.int32 and scan.is_contiguous()
                                 and scan.numel() >= t * index.n_cells):
        raise TypeError(f"overlap_emit: scan must be a contiguous int32 device tensor of at least {t * index.n_cells} values")
    check(_lib.hip_lib().s3_overlap_emit(C.byref(index.s3_grid()), C.c_void_p(a.data_ptr()), int(a.stride(0)), C.c_void_p(b.data_ptr()),
                                         int(b.stride(0)), t, None if route == "by_ta" else _ptr(scan), n_pairs, OVERLAP_PASSES[route],
                                         _ptr(keys), _ptr(vals), _stream()), "s3_overlap_emit")
    return keys, vals


def overlap_heads(keys, vals, index, b, two_pass=False, out=None):
    """head[j] = 1 where the sorted pair j is the first of its (t, a, b) (s3_overlap_heads) -> int32 [n_pairs], written into the front
    of ``out`` when given.  ``b``: the second label array of the batch (read with ``two_pass``, whose keys hold (t, a) alone)"""
    n_pairs = _overlap_pairs(keys, vals, "overlap_heads")
    b, _, t = _overlap_labels(b, b, index, "overlap_heads")
    out = _out_tensor(out, (n_pairs,), pt.int32, keys.device, "overlap_heads", at_least=True)
    check(_lib.hip_lib().s3_overlap_heads(C.byref(index.s3_grid()), _ptr(keys), _ptr(vals), n_pairs, int(bool(two_pass)), C.c_void_p(b.data_ptr()),
                                          int(b.stride(0)), t, _ptr(out), _stream()), "s3_overlap_heads")
    return out


def overlap_reduce(keys, vals, index, b, edge, n_edges, two_pass=False):
    """the edges of the sorted pairs (s3_overlap_reduce): ``edge`` int32 [n_pairs + 1], the exclusive scan of what ``overlap_heads``
    gave with one entry more.  -> dict of device arrays ``src``, ``dst`` int32, ``n_cells`` int64, ``units`` int64 (the unsigned bits)
    and ``volume`` f64, [n_edges] each.  Integer sums: equal inputs give equal bits"""
    n_pairs, n_edges = _overlap_pairs(keys, vals, "overlap_reduce"), int(n_edges)
    b, _, t = _overlap_labels(b, b, index, "overlap_reduce")
    if not (isinstance(edge, pt.Tensor) and edge.is_cuda and edge.dtype == pt.int32 and edge.is_contiguous() and edge.numel() >= n_pairs + 1):
        raise TypeError(f"overlap_reduce: edge must be a contiguous int32 device tensor of at least {n_pairs + 1} values")
    if not 0 <= n_edges <= n_pairs:
        raise ValueError(f"overlap_reduce: {n_edges} edges of {n_pairs} pairs")
    dev = keys.device
    out = {"src": pt.empty(n_edges, dtype=pt.int32, device=dev), "dst": pt.empty(n_edges, dtype=pt.int32, device=dev),
           "n_cells": pt.empty(n_edges, dtype=pt.int64, device=dev), "units": pt.empty(n_edges, dtype=pt.int64, device=dev),
           "volume": pt.empty(n_edges, dtype=pt.float64, device=dev)}
    check(_lib.hip_lib().s3_overlap_reduce(C.byref(index.s3_grid()), _ptr(keys), _ptr(vals), n_pairs, int(bool(two_pass)), C.c_void_p(b.data_ptr()),
                                           int(b.stride(0)), t, _ptr(edge), n_edges, *(_ptr(out[k]) for k in OVERLAP_FIELDS), _stream()),
          "s3_overlap_reduce")
    return out


def overlap_table(a, b, index, pair_bytes=REGION_PAIR_BYTES, two_pass=None):
    """the overlap table of two label arrays int32 [n_cells, T] of one grid (include/s3overlap.h): per column the pairs (a, b) of labels
    that occur at a cell in both, by ascending (a, b).  count (s3_overlap_count), scan, read back the pairs per column, emit
    (s3_overlap_emit), sort (s3_sort_pairs), heads (s3_overlap_heads), scan, read back the edges per column, reduce
    (s3_overlap_reduce) -- in batches of ``region_batch_columns`` columns.  ``two_pass``: None sorts by one key where (t, a, b) fits 64
    bits and in two stable passes (b, then (t, a)) otherwise; True / False force a route (for tests and measurements).
    -> dict: ``offsets`` int64 numpy [T + 1] (column t owns the edges [offsets[t], offsets[t + 1])) and on the device ``src``, ``dst``
    int32 [E], ``n_cells`` int64 [E], ``units`` int64 [E] (the unsigned bits of the volume in finest cells) and ``volume`` f64 [E]."""
    a, b, t = _overlap_labels(a, b, index, "overlap_table")
    n_cells, lib, dev = index.n_cells, _lib.hip_lib(), a.device
    offsets, parts = [np.zeros(1, dtype=np.int64)], []
    step = region_batch_columns(n_cells, pair_bytes)
    for c0 in range(0, t, step):
        wa, wb = a[:, c0:c0 + step], b[:, c0:c0 + step]
        t_b = int(wa.shape[1])
        n = t_b * n_cells
        w, tb = overlap_key_bits(n_cells, t_b)
        two = tb + 2 * w > 64 if two_pass is None else bool(two_pass)
        if not two and tb + 2 * w > 64:
            raise ValueError(f"overlap_table: (t, a, b) of {t_b} columns and {n_cells} cells does not fit one key")
        scan = pt.empty(n + 1, dtype=pt.int32, device=dev)                      # one entry more: its scan is the total
        scan[n:].zero_()
        overlap_count(wa, wb, index, out=scan)
        check(lib.s3_exclusive_scan(_ptr(scan), _ptr(scan), n + 1, 4, _stream()), "s3_exclusive_scan")
        starts = scan[::n_cells].cpu()                                          # [t_b + 1]: the first pair of every column (waits for the stream)
        n_pairs = int(starts[-1])
        if n_pairs == 0:
            offsets.append(np.full(t_b, offsets[-1][-1], dtype=np.int64))
            continue
        keys, vals = pt.empty(n_pairs, dtype=pt.int64, device=dev), pt.empty(n_pairs, dtype=pt.int32, device=dev)
        if two:
            overlap_emit(wa, wb, index, scan, keys, vals, "by_b")
            sort_pairs(keys, vals, w)
            overlap_emit(wa, wb, index, None, keys, vals, "by_ta")
            sort_pairs(keys, vals, max(1, tb + w))
        else:
            overlap_emit(wa, wb, index, scan, keys, vals, "one_key")
            sort_pairs(keys, vals, tb + 2 * w)
        head = pt.empty(n_pairs + 1, dtype=pt.int32, device=dev)
        head[n_pairs:].zero_()
        overlap_heads(keys, vals, index, wb, two, out=head)
        check(lib.s3_exclusive_scan(_ptr(head), _ptr(head), n_pairs + 1, 4, _stream()), "s3_exclusive_scan")
        first = head[starts.to(dev, pt.int64)].cpu().numpy().astype(np.int64)   # [t_b + 1]: the first edge of every column
        offsets.append(offsets[-1][-1] + first[1:])
        parts.append(overlap_reduce(keys, vals, index, wb, head, int(first[-1]), two))
    table = {"offsets": np.concatenate(offsets)}
    for k, dtype in zip(OVERLAP_FIELDS, (pt.int32, pt.int32, pt.int64, pt.int64, pt.float64)):
        table[k] = pt.empty(0, dtype=dtype, device=dev) if not parts else parts[0][k] if len(parts) == 1 else pt.cat([p[k] for p in parts])
    return table


def _pitched_matrix(t, who):
    """row pitch in elements of a 2-D f32 / f64 device matrix with unit inner stride, read where it lies"""
    layout = _row_layout(t) if t.is_cuda and t.dtype in DTYPE_CODE and t.dim() == 2 else None
    if layout is None:
        raise TypeError(f"{who}: 2-D float32 / float64 device matrix with unit inner stride required")
    return layout[1]


def gram_scratch(n, t, device):
    """the scratch memory ``gram`` needs for a matrix [n, t]: allocate it once where many products of one size follow"""
    return _scratch(_lib.hip_lib().s3_gram_scratch_bytes(int(n), int(t)), device)


def gram(x, mean=None, weight=None, out=None, scratch=None):
    """``sum_n weight[n] (x[n] - mean[n]) (x[n] - mean[n])^T`` -> f64 [T, T] on the f64 matrix cores (s3_gram).  ``x`` [N, T] float32 or
    float64 on the device, rows may be pitched; it is read where it lies, float32 is widened in the kernel's staging (the result
    equals the one of ``x.double()`` to the bit).  ``mean`` / ``weight`` f64 device vectors [N] or None (no centring / weight 1)."""
    stride = _pitched_matrix(x, "gram")
    n, t = int(x.shape[0]), int(x.shape[1])
    if n < 1 or t < 1:
        raise ValueError(f"gram: empty matrix {tuple(x.shape)}")
    for name, v in (("mean", mean), ("weight", weight)):
        if v is not None and not (v.is_cuda and v.dtype == pt.float64 and v.numel() == n):
            raise TypeError(f"gram: {name} must be a float64 device vector [{n}]")
    if scratch is None:
        scratch = gram_scratch(n, t, x.device)
    elif scratch.numel() * scratch.element_size() < int(_lib.hip_lib().s3_gram_scratch_bytes(n, t)):
        raise ValueError("gram: scratch too small")
    out = _out_tensor(out, (t, t), pt.float64, x.device, "gram")
    check(_lib.hip_lib().s3_gram(C.c_void_p(x.data_ptr()), DTYPE_CODE[x.dtype], n, t, stride, _ptr(mean), _ptr(weight), _ptr(out), _ptr(scratch),
                      _stream()), "s3_gram")
    return out


def tall_gemm(left, b, out=None):
    """``left @ b`` -> f64 [m, n] on the f64 matrix cores (s3_tall_gemm).  ``left`` [m, k] float32 or float64 on the device, rows may be
    pitched, read where it lies; ``b`` [k, n] f64 contiguous on the device."""
    stride = _pitched_matrix(left, "tall_gemm")
    m, k = int(left.shape[0]), int(left.shape[1])
    if not (b.is_cuda and b.dtype == pt.float64 and b.dim() == 2 and b.is_contiguous() and int(b.shape[0]) == k):
        raise TypeError(f"tall_gemm: b must be a contiguous float64 device matrix [{k}, n]")
    n = int(b.shape[1])
    if m < 1 or k < 1 or n < 1:
        raise ValueError(f"tall_gemm: empty product [{m}, {k}] x [{k}, {n}]")
    out = _out_tensor(out, (m, n), pt.float64, left.device, "tall_gemm")
    check(_lib.hip_lib().s3_tall_gemm(C.c_void_p(left.data_ptr()), DTYPE_CODE[left.dtype], m, k, stride, _ptr(b), n, _ptr(out), _stream()),
          "s3_tall_gemm")
    return out


def row_means(x):
    """temporal mean of every row of a 2-D float32 / float64 device matrix, rows possibly pitched -> f64 [N] (s3_row_moments)"""
    stride = _pitched_matrix(x, "row_means")
    n, t = int(x.shape[0]), int(x.shape[1])
    mean = pt.empty(n, dtype=pt.float64, device=x.device)
    check(_lib.hip_lib().s3_row_moments(C.c_void_p(x.data_ptr()), DTYPE_CODE[x.dtype], n, t, stride, 0, _ptr(mean), C.c_void_p(0), _stream()),
          "s3_row_moments")
    return mean


def _segment_arguments(x, mean, nperseg, hop, n_blk, bre, bim, who):
    stride = _pitched_matrix(x, who)
    n, t = int(x.shape[0]), int(x.shape[1])
    nperseg, hop, n_blk = int(nperseg), int(hop), int(n_blk)
    if n < 1 or nperseg < 1 or hop < 1 or n_blk < 1 or (n_blk - 1) * hop + nperseg > t:
        raise ValueError(f"{who}: {n_blk} segments of {nperseg} samples, {hop} apart, do not fit rows of {t} samples ({n} rows)")
    for name, b in (("bre", bre), ("bim", bim)):
        if not (b.is_cuda and b.dtype == pt.float64 and b.dim() == 2 and b.is_contiguous() and int(b.shape[0]) == nperseg
                and b.shape == bre.shape and int(b.shape[1]) >= 1):
            raise TypeError(f"{who}: {name} must be a contiguous float64 device matrix [{nperseg}, n_f]")
    if mean is not None and not (mean.is_cuda and mean.dtype == pt.float64 and mean.numel() == n):
        raise TypeError(f"{who}: mean must be a float64 device vector [{n}]")
    return (C.c_void_p(x.data_ptr()), DTYPE_CODE[x.dtype], n, t, stride, _ptr(mean), nperseg, hop, n_blk, _ptr(bre), _ptr(bim),
            int(bre.shape[1]))


def segment_dft(x, mean, nperseg, hop, n_blk, bre, bim, out=None):
    """windowed DFT coefficients of the ``n_blk`` segments (``nperseg`` samples, ``hop`` apart) of every row of ``x`` (s3_segment_dft):
    ``c[i, b, f] = sum_l (x[i, b hop + l] - mean[i]) (bre[l, f] + i bim[l, f])`` -> f64 [N, n_f, n_blk, 2].  ``x`` [N, T] float32 or
    float64 on the device, rows may be pitched, read where it lies; ``mean`` f64 [N] or None; ``bre`` / ``bim`` f64 [nperseg, n_f]."""
    args = _segment_arguments(x, mean, nperseg, hop, n_blk, bre, bim, "segment_dft")
    shape = (args[2], args[-1], int(n_blk), 2)
    out = _out_tensor(out, shape, pt.float64, x.device, "segment_dft")
    check(_lib.hip_lib().s3_segment_dft(*args, _ptr(out), _stream()), "s3_segment_dft")
    return out


def segment_psd(x, mean, nperseg, hop, n_blk, bre, bim, scale, out=None):
    """``scale[f] * sum_b |c[i, b, f]|^2`` of the same coefficients -> f64 [N, n_f], summed in the kernel's registers (s3_segment_psd):
    the coefficients are never written.  ``scale`` f64 device vector [n_f]."""
    args = _segment_arguments(x, mean, nperseg, hop, n_blk, bre, bim, "segment_psd")
    shape = (args[2], args[-1])
    if not (scale.is_cuda and scale.dtype == pt.float64 and scale.numel() == shape[1]):
        raise TypeError(f"segment_psd: scale must be a float64 device vector [{shape[1]}]")
    out = _out_tensor(out, shape, pt.float64, x.device, "segment_psd")
    check(_lib.hip_lib().s3_segment_psd(*args, _ptr(scale), _ptr(out), _stream()), "s3_segment_psd")
    return out


# ExportData queues its device-to-host copies on a stream of their own and lets them complete behind its back (the host-logic
# tests replace this module by CPU stand-ins that do not have the attribute: there every copy is immediate)
ASYNC_TRANSFERS = True


def yard_stream(src, dst, reads, writes, nontemporal=True):
    """yardstick (bench.py): hand-written streaming kernel, ``reads`` 16-byte vectors read per ``writes`` written
    (s3_yard_stream); -> (bytes read, bytes written)"""
    r, w = C.c_int64(0), C.c_int64(0)
    check(_lib.hip_lib().s3_yard_stream(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), src.numel() * src.element_size(),
                                        dst.numel() * dst.element_size(), int(reads), int(writes), int(bool(nontemporal)),
                                        _stream(), C.byref(r), C.byref(w)), "s3_yard_stream")
    return r.value, w.value


def _batch_values(values, n_comp, n_snapshots, who):
    """checks of the interpolated batch ``[nc, n_comp*T]`` / ``[nc, n_comp, T]`` the transposes read; -> nc"""
    if not (isinstance(values, pt.Tensor) and values.is_cuda and values.is_contiguous() and values.dtype == pt.float64):
        raise TypeError(f"{who}: contiguous float64 device tensor required as input")
    n_comp, n_snapshots = int(n_comp), int(n_snapshots)
    if values.dim() < 1 or n_comp < 1 or n_snapshots < 0 or values.numel() != int(values.shape[0]) * n_comp * n_snapshots:
        raise ValueError(f"{who}: a batch of shape {tuple(values.shape)} does not hold {n_comp} component(s) x {n_snapshots} snapshot(s) per row")
    return int(values.shape[0])


def _storage_dtype(dtype, who):
    if dtype is None:
        return pt.float64
    if dtype not in DTYPE_CODE:
        raise ValueError(f"{who}: the storage type is float32 or float64, not {dtype}")
    return dtype


def snapshot_major(values, n_comp, n_snapshots, out=None, dtype=None):
    """device [nc, n_comp*T] (or [nc, n_comp, T]) f64 -> device [T, nc, n_comp]: contiguous snapshots for the HDF5 sink.
    ``dtype`` (default float64): the storage type of the result; float32 rounds every value once, to nearest even, exactly as
    ``numpy.astype(float32)`` does (s3_snapshot_major_as)."""
    dtype = _storage_dtype(dtype, "snapshot_major")
    nc = _batch_values(values, n_comp, n_snapshots, "snapshot_major")
    out = _out_tensor(out, (int(n_snapshots), nc, int(n_comp)), dtype, values.device, "snapshot_major")
    if dtype == pt.float64:
        check(_lib.hip_lib().s3_snapshot_major(_ptr(values), nc, int(n_comp), int(n_snapshots), _ptr(out), _stream()),
              "s3_snapshot_major")
    else:
        check(_lib.hip_lib().s3_snapshot_major_as(_ptr(values), nc, int(n_comp), int(n_snapshots), DTYPE_CODE[dtype], _ptr(out),
                                                  _stream()), "s3_snapshot_major_as")
    return out


def snapshot_major_rows(values, n_comp, n_snapshots, rows, n_out, out_ptr, dtype=None):
    """a shard's values, device [n_mine, n_comp*T] f64, -> rows ``rows`` (device int32 [n_mine]) of the snapshot-major batch
    buffer ``[T, n_out, n_comp]`` of ``dtype`` (default float64) at device address ``out_ptr`` (host memory all ranks share,
    s3_snapshot_major_rows).  The caller answers for the row ids lying in ``[0, n_out)`` and for the buffer's size."""
    dtype = _storage_dtype(dtype, "snapshot_major_rows")
    nc = _batch_values(values, n_comp, n_snapshots, "snapshot_major_rows")
    if not (isinstance(rows, pt.Tensor) and rows.is_cuda and rows.dtype == pt.int32 and rows.is_contiguous() and rows.numel() == nc):
        raise TypeError("snapshot_major_rows: one int32 device row id per input row required")
    if int(n_out) < nc or not int(out_ptr) or int(out_ptr) % (4 if dtype == pt.float32 else 8):
        raise ValueError(f"snapshot_major_rows: an output of {n_out} rows at address {int(out_ptr):#x} cannot take {nc} rows of {dtype}")
    if dtype == pt.float64:
        check(_lib.hip_lib().s3_snapshot_major_rows(_ptr(values), nc, int(n_comp), int(n_snapshots), _ptr(rows),
                                                    int(n_out), C.c_void_p(int(out_ptr)), _stream()), "s3_snapshot_major_rows")
    else:
        check(_lib.hip_lib().s3_snapshot_major_rows_as(_ptr(values), nc, int(n_comp), int(n_snapshots), _ptr(rows), int(n_out),
                                                       DTYPE_CODE[dtype], C.c_void_p(int(out_ptr)), _stream()),
              "s3_snapshot_major_rows_as")


def cell_major(snapshots, out, t0=0):
    """datasets as the file holds them, device ``[T_b, nc]`` or ``[T_b, nc, n_comp]`` float32 / float64 (contiguous), -> columns
    ``[t0, t0 + T_b)`` of the cell-major device matrix ``out`` ``[nc, T]`` / ``[nc, n_comp, T]`` float32 / float64 that SVD and DMD
    read (s3_cell_major).  ``out`` has unit stride along T and one pitch for all its (cell, component) rows; its other columns
    and the padding of its rows are left alone.  float64 -> float32 rounds to nearest even, float32 -> float64 is exact."""
    for name, t in (("snapshots", snapshots), ("out", out)):
        if not (isinstance(t, pt.Tensor) and t.is_cuda and t.dtype in DTYPE_CODE):
            raise TypeError(f"cell_major: {name} must be a float32 or float64 device tensor")
    if snapshots.device != out.device:
        raise TypeError("cell_major: snapshots and out live on different devices")
    if not snapshots.is_contiguous():
        raise TypeError("cell_major: contiguous snapshots required")
    if snapshots.dim() not in (2, 3) or out.dim() != snapshots.dim():
        raise ValueError(f"cell_major: snapshots [T_b, nc(, n_comp)] and out [nc(, n_comp), T] required, got {tuple(snapshots.shape)} "
                         f"and {tuple(out.shape)}")
    t_b, nc = int(snapshots.shape[0]), int(snapshots.shape[1])
    n_comp = int(snapshots.shape[2]) if snapshots.dim() == 3 else 1
    n_cols, t0 = int(out.shape[-1]), int(t0)
    if tuple(out.shape[:-1]) != tuple(snapshots.shape[1:]):
        raise ValueError(f"cell_major: out {tuple(out.shape)} does not match snapshots {tuple(snapshots.shape)}")
    if t0 < 0 or t0 + t_b > n_cols:
        raise ValueError(f"cell_major: columns [{t0}, {t0 + t_b}) lie outside the {n_cols} columns of out")
    if nc == 0 or t_b == 0:
        return out
    pitch = int(out.stride(0)) if n_comp == 1 else int(out.stride(-2))          # (the stride of an axis of length 1 says nothing)
    if out.stride(-1) != 1 or pitch < n_cols or (out.dim() == 3 and n_comp > 1 and int(out.stride(0)) != n_comp * pitch):
        raise ValueError("cell_major: out needs unit stride along T and one pitch >= T for all its rows")
    check(_lib.hip_lib().s3_cell_major(C.c_void_p(snapshots.data_ptr()), DTYPE_CODE[snapshots.dtype], t_b, nc, n_comp,
                                       C.c_void_p(out.data_ptr()), DTYPE_CODE[out.dtype], n_cols, pitch, t0, _stream()), "s3_cell_major")
    return out


class InterpPlan:
    """De-duplicated, LDS-tiled form of a static neighbour table (s3_interp_plan_*): build once per KNN cache, reuse for
    every snapshot batch.  ``centers`` (cell centres, [nc, dim]) gives the Hilbert-curve processing order."""

    def __init__(self, idx, n_src, centers=None, tile_cells=0):
        if not (idx.is_cuda and idx.dtype == pt.int32 and idx.is_contiguous() and idx.dim() == 2):
            raise TypeError("InterpPlan: idx must be a contiguous int32 [nc, k] device tensor")
        self.nc, self.k = int(idx.shape[0]), int(idx.shape[1])
        self.n_src = int(n_src)
        ctr = to_device(centers, pt.float64) if centers is not None else None
        dim = int(ctr.shape[1]) if ctr is not None else 0
        self._handle = C.c_void_p(0)
        check(_lib.hip_lib().s3_interp_plan_create(_ptr(idx), self.nc, self.k, self.n_src, _ptr(ctr), dim, int(tile_cells), _stream(),
                                                   C.byref(self._handle)), "s3_interp_plan_create")
        nt, nr = C.c_int64(0), C.c_int64(0)
        check(_lib.hip_lib().s3_interp_plan_info(self._handle, C.byref(nt), C.byref(nr)), "s3_interp_plan_info")
        self.n_tiles, self.total_rows = nt.value, nr.value
        self._w_ref = None              # the weights tensor whose values the plan holds (kept alive: see interp)
        self._w_version = None
        self.n_table = None             # rows of the full table behind the source rows (set_source_ids)

    def set_weights(self, w):
        """attach the weights of the table ([nc, k] float64, caller's cell order); the plan keeps a COPY in tile order.
        Call it again after rewriting ``w`` in place through a raw pointer (``idw_weights`` writes that way): such writes
        do not change the tensor's version counter, so ``interp`` cannot see them."""
        if not (w.is_cuda and w.dtype == pt.float64 and w.is_contiguous() and tuple(w.shape) == (self.nc, self.k)):
            raise TypeError("InterpPlan: weights must be a contiguous float64 [nc, k] device tensor")
        check(_lib.hip_lib().s3_interp_plan_set_weights(self._handle, _ptr(w), _stream()), "s3_interp_plan_set_weights")
        # the tensor itself, not its address: while the plan holds it the allocator cannot hand the same address to
        # another weights tensor, so `is` identifies it
        self._w_ref, self._w_version = w, w._version

    def set_source_ids(self, ids, n_table):
        """``ids`` (int32 device tensor [n_src]): the row of the caller's full table behind each source row the plan was built
        on; afterwards ``interp_src`` reads a full ``[n_table, ...]`` batch where it lies (s3_interp_plan_set_source_ids)"""
        if not (ids.is_cuda and ids.dtype == pt.int32 and ids.is_contiguous() and ids.numel() == self.n_src):
            raise TypeError("InterpPlan.set_source_ids: contiguous int32 device tensor with one id per source row required")
        check(_lib.hip_lib().s3_interp_plan_set_source_ids(self._handle, _ptr(ids), int(n_table), _stream()),
              "s3_interp_plan_set_source_ids")
        self.n_table = int(n_table)

    def partition(self, world):
        """cost-balanced leaf-cell shards (s3_interp_plan_partition): ``(order, cuts)`` -- ``order`` is the plan's processing
        order (device int32 [nc], position -> cell id: cells in Hilbert order) and rank r owns ``order[cuts[r]:cuts[r + 1]]``"""
        order = pt.empty(self.nc, dtype=pt.int32, device=device())
        cuts = (C.c_int64 * (int(world) + 1))()
        check(_lib.hip_lib().s3_interp_plan_partition(self._handle, int(world), _ptr(order), cuts, _stream()),
              "s3_interp_plan_partition")
        return order, [int(c) for c in cuts]

    def cost_profile(self, n_samples):
        """cumulative per-snapshot cost of the plan's tiles along its processing order at ``n_samples + 1`` equally spaced
        cell positions (s3_interp_plan_cost_profile) -> float64 numpy array"""
        out = np.zeros(int(n_samples) + 1, dtype=np.float64)
        check(_lib.hip_lib().s3_interp_plan_cost_profile(self._handle, int(n_samples), out.ctypes.data_as(C.c_void_p), _stream()),
              "s3_interp_plan_cost_profile")
        return out

    @staticmethod
    def _layout(data, k=None):
        """(row_len, in_stride) of a data matrix the planned kernels can read, None otherwise.  Every kernel takes rows
        that start on a 16-byte boundary and are readable up to the next multiple of 16 bytes (``padded_rows`` views always
        are; dense rows when their length is a multiple of 16 bytes).  Plans with the reference's neighbour counts
        (``k`` = 8 | 26) also take dense rows of any length >= 16 bytes where they lie (element alignment; the persistent
        kernel, s3hip.h)."""
        layout = _row_layout(data) if data.dtype in DTYPE_CODE else None
        if layout is None or layout[1] >= 1 << 31:
            return None
        row_len, in_stride = layout
        epv = 16 // data.element_size()
        padded = (row_len + epv - 1) // epv * epv
        if in_stride % epv or in_stride < padded or (data.is_cuda and data.data_ptr() % 16):
            if not (k in (8, 26) and row_len >= epv):
                return None
        return layout

    @staticmethod
    def supports(k, data):
        """can a plan with ``k`` neighbours read ``data`` as it stands?  ``k = None``: by the 16-byte rule alone (every plan)"""
        return (k is None or k <= 64) and InterpPlan._layout(data, k) is not None

    def close(self):
        if getattr(self, "_handle", None) is not None and self._handle.value:
            _lib.hip_lib().s3_interp_plan_destroy(self._handle)
            self._handle = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown
            pass

    def interp(self, w, data, out=None):
        """``data`` [n_src, ...]: contiguous, or a column slice ``buf[:, :L]`` of a wider 2-D buffer (rows padded to a
        multiple of 128 bytes keep every staged segment on one cache line, see ``padded_rows``)."""
        if not (w.dtype == pt.float64 and tuple(w.shape) == (self.nc, self.k) and int(data.shape[0]) == self.n_src
                and data.dtype in DTYPE_CODE):
            raise TypeError("InterpPlan.interp: weights / data do not match the plan")
        row_len, in_stride, out = self._check_batch(data, out, "interp")
        if w is not self._w_ref or w._version != self._w_version:    # another tensor, or modified through torch: re-attach
            self.set_weights(w)
        check(_lib.hip_lib().s3_interp_planned(self._handle, C.c_void_p(0), C.c_void_p(data.data_ptr()),
                                               DTYPE_CODE[data.dtype], row_len, in_stride, _ptr(out), _stream()),
              "s3_interp_planned")
        return out

    def _check_batch(self, data, out, who):
        layout = self._layout(data, self.k)
        if layout is None:
            raise TypeError(f"InterpPlan.{who}: source rows must be 16-byte aligned (see padded_rows), or dense rows of at "
                            f"least 16 bytes on a plan with k = 8 | 26")
        row_len, in_stride = layout
        if out is None:
            out = pt.empty((self.nc,) + tuple(data.shape[1:]), dtype=pt.float64, device=data.device)
        if not (data.is_cuda and out.is_cuda and out.is_contiguous() and out.dtype == pt.float64
                and out.numel() == self.nc * row_len):
            raise TypeError(f"InterpPlan.{who}: device tensors required, out must be contiguous float64 [nc, ...]")
        return row_len, in_stride, out

    ROUTES = {1: "stream_elem", 2: "stream_wide", 3: "stream_narrow", 4: "short_quad", 5: "short_reg", 6: "short", 7: "shift",
              8: "chunk64", 9: "chunk128"}             # S3_ROUTE_* (s3hip.h)

    def route(self, data, src=False):
        """the kernel ``interp(w, data)`` (``src``: ``interp_src(data)``) would launch, and how (s3_interp_plan_route; launches
        nothing) -> dict(route=<name>, width=<template width>, even=, gy=, tail=)"""
        layout = self._layout(data, self.k)
        if layout is None or not data.is_cuda:
            raise TypeError("InterpPlan.route: the planned kernels cannot read these rows (see interp)")
        if src and self.n_table is None:
            raise RuntimeError("InterpPlan.route: call set_source_ids first")
        row_len, in_stride = layout
        h = (C.c_int32 * 5)()
        check(_lib.hip_lib().s3_interp_plan_route(self._handle, int(bool(src)), C.c_void_p(data.data_ptr()), DTYPE_CODE[data.dtype],
                                                  row_len, in_stride, h), "s3_interp_plan_route")
        return dict(route=self.ROUTES[h[0]], width=h[1], even=h[2], gy=h[3], tail=h[4])

    def yard_loads(self, table, variant=0, in_place=True):
        """yardstick (bench.py): the loads of this plan on ``table`` and nothing else (s3_yard_plan_loads); -> staged bytes"""
        row_len, in_stride = self._layout(table, None)
        staged = C.c_int64(0)
        check(_lib.hip_lib().s3_yard_plan_loads(self._handle, C.c_void_p(table.data_ptr()), self.n_table if in_place else 0,
                                                row_len * table.element_size(), in_stride * table.element_size(), int(variant),
                                                _stream(), C.byref(staged)), "s3_yard_plan_loads")
        return staged.value

    def interp_src(self, table, out=None):
        """like ``interp`` for a FULL batch ``table`` [n_table, ...] that is read where it lies (no gather of the referenced
        rows first); needs ``set_weights`` and ``set_source_ids``"""
        if self.n_table is None or self._w_ref is None:
            raise RuntimeError("InterpPlan.interp_src: call set_weights and set_source_ids first")
        if int(table.shape[0]) != self.n_table or table.dtype not in DTYPE_CODE:
            raise TypeError("InterpPlan.interp_src: the table does not match the ids given to set_source_ids")
        row_len, in_stride, out = self._check_batch(table, out, "interp_src")
        check(_lib.hip_lib().s3_interp_planned_src(self._handle, C.c_void_p(table.data_ptr()), DTYPE_CODE[table.dtype],
                                                   self.n_table, row_len, in_stride, _ptr(out), _stream()),
              "s3_interp_planned_src")
        return out


def to_host(t):
    """contiguous device tensor -> numpy array in pageable host memory through the native staged download (s3_download);
    the result is complete on return"""
    t = t.contiguous()
    out = np.empty(tuple(t.shape), dtype=pt.empty((), dtype=t.dtype).numpy().dtype)
    if out.nbytes:
        synchronize()                      # t was produced on torch's current stream or on an engine stream that was waited for
        check(_lib.hip_lib().s3_download(out.ctypes.data_as(C.c_void_p), C.c_void_p(t.data_ptr()), out.nbytes, None), "s3_download")
    return out


def upload_rows(host, rows):
    """contiguous host tensor [n_rows, row_len] -> device rows ``rows`` (a ``padded_rows`` view: the bytes between two
    rows are padding and may be overwritten) through the native staged upload (s3_upload_rows); asynchronous on the
    current stream"""
    if host.is_cuda or not host.is_contiguous() or host.dim() != 2 or host.dtype != rows.dtype:
        raise TypeError("upload_rows: contiguous 2-D host tensor of the rows' dtype required")
    if not rows.is_cuda or rows.dim() != 2 or rows.stride(1) != 1 or tuple(rows.shape) != tuple(host.shape):
        raise TypeError("upload_rows: 2-D device rows of the same shape with unit inner stride required")
    item = host.element_size()
    check(_lib.hip_lib().s3_upload_rows(C.c_void_p(host.data_ptr()), int(host.shape[0]), int(host.shape[1]) * item,
                                        C.c_void_p(rows.data_ptr()), int(rows.stride(0)) * item, _stream()),
          "s3_upload_rows")
    return rows


def upload_rows_indexed(host, row_ids, rows):
    """rows ``row_ids`` (ascending int32 numpy array) of the contiguous host tensor [n, row_len] -> device rows ``rows``
    [len(row_ids), row_len] (see ``upload_rows``)"""
    if host.is_cuda or not host.is_contiguous() or host.dim() != 2 or host.dtype != rows.dtype:
        raise TypeError("upload_rows_indexed: contiguous 2-D host tensor of the rows' dtype required")
    ids = np.ascontiguousarray(row_ids, dtype=np.int32)
    if not rows.is_cuda or rows.dim() != 2 or rows.stride(1) != 1 or tuple(rows.shape) != (len(ids), int(host.shape[1])):
        raise TypeError("upload_rows_indexed: device rows [len(row_ids), row_len] with unit inner stride required")
    if len(ids) and (int(ids.min()) < 0 or int(ids.max()) >= int(host.shape[0])):
        raise IndexError("upload_rows_indexed: row id outside the host tensor")
    item = host.element_size()
    check(_lib.hip_lib().s3_upload_rows_indexed(C.c_void_p(host.data_ptr()), ids.ctypes.data_as(C.c_void_p), len(ids),
                                                int(host.shape[1]) * item, C.c_void_p(rows.data_ptr()),
                                                int(rows.stride(0)) * item, _stream()), "s3_upload_rows_indexed")
    return rows


def upload_row_pieces(host, row_ids, t0, t1, rows):
    """snapshots ``[t0, t1)`` of the rows ``row_ids`` (int32 numpy array, or None: all rows) of the contiguous host field
    ``host`` [N, n_comp, T] -> device rows ``rows`` [n_sel, n_comp * (t1 - t0)] (unit inner stride; the bytes between two rows
    may be overwritten) through the native staged upload (s3_upload_row_pieces); asynchronous on the current stream"""
    if host.is_cuda or not host.is_contiguous() or host.dim() != 3 or host.dtype != rows.dtype:
        raise TypeError("upload_row_pieces: contiguous host tensor [N, n_comp, T] of the rows' dtype required")
    n, n_comp, t = (int(v) for v in host.shape)
    if not 0 <= t0 < t1 <= t:
        raise ValueError(f"upload_row_pieces: snapshots [{t0}, {t1}) of {t}")
    ids = None if row_ids is None else np.ascontiguousarray(row_ids, dtype=np.int32)
    n_sel = n if ids is None else len(ids)
    if not rows.is_cuda or rows.dim() != 2 or rows.stride(1) != 1 or tuple(rows.shape) != (n_sel, n_comp * (t1 - t0)):
        raise TypeError("upload_row_pieces: device rows [n_sel, n_comp * (t1 - t0)] with unit inner stride required")
    if ids is not None and len(ids) and (int(ids.min()) < 0 or int(ids.max()) >= n):
        raise IndexError("upload_row_pieces: row id outside the host tensor")
    item = host.element_size()
    check(_lib.hip_lib().s3_upload_row_pieces(C.c_void_p(host.data_ptr()), None if ids is None else ids.ctypes.data_as(C.c_void_p),
                                              n_sel, n_comp * t * item, t0 * item, n_comp, (t1 - t0) * item, t * item,
                                              C.c_void_p(rows.data_ptr()), int(rows.stride(0)) * item, _stream()),
          "s3_upload_row_pieces")
    return rows


def gather_rows(src, ids, dst):
    """device rows: ``dst[i, :] = src[ids[i], :]`` (``ids`` int32 device tensor) or ``dst[i, :] = src[i, :]`` (``ids``
    None: a re-pitch).  ``src`` / ``dst`` are 2-D device tensors (or ``padded_rows`` views) with unit inner stride."""
    if not (src.is_cuda and dst.is_cuda and src.dim() == 2 and dst.dim() == 2 and src.stride(1) == 1 and dst.stride(1) == 1
            and src.dtype == dst.dtype and src.shape[1] == dst.shape[1]):
        raise TypeError("gather_rows: 2-D device tensors of one dtype and row length with unit inner stride required")
    n = int(dst.shape[0])
    if ids is not None and not (ids.is_cuda and ids.dtype == pt.int32 and ids.is_contiguous() and ids.numel() == n):
        raise TypeError("gather_rows: ids must be a contiguous int32 device tensor with one entry per destination row")
    item = src.element_size()
    check(_lib.hip_lib().s3_gather_rows(C.c_void_p(src.data_ptr()), int(src.shape[0]), int(src.shape[1]) * item,
                                        int(src.stride(0)) * item, _ptr(ids), n, C.c_void_p(dst.data_ptr()),
                                        int(dst.stride(0)) * item, _stream()), "s3_gather_rows")
    return dst


def exclusive_scan(x):
    """exclusive prefix sum of a contiguous int32 / int64 device tensor (csrc/scan_sort.h) -> new tensor"""
    if not (x.is_cuda and x.is_contiguous() and x.dtype in (pt.int32, pt.int64) and x.dim() == 1):
        raise TypeError("exclusive_scan: contiguous 1-D int32 / int64 device tensor required")
    out = pt.empty_like(x)
    check(_lib.hip_lib().s3_exclusive_scan(_ptr(x), _ptr(out), int(x.numel()), x.element_size(), _stream()), "s3_exclusive_scan")
    return out


def sort_pairs(keys, vals, bits=64):
    """stable ascending sort of (key, value) pairs by the low ``bits`` bits of the int64 keys (read as unsigned), in place"""
    if not (keys.is_cuda and vals.is_cuda and keys.is_contiguous() and vals.is_contiguous() and keys.dtype == pt.int64
            and vals.dtype == pt.int32 and keys.numel() == vals.numel()):
        raise TypeError("sort_pairs: contiguous int64 keys and int32 values of one length on the device required")
    check(_lib.hip_lib().s3_sort_pairs(_ptr(keys), _ptr(vals), int(keys.numel()), int(bits), _stream()), "s3_sort_pairs")
    return keys, vals


def spatial_order(points):
    """Hilbert-curve order of device points [n, 2|3] float64 -> int32 permutation (position -> point) on the device"""
    pts = to_device(points, pt.float64)
    perm = pt.empty(int(pts.shape[0]), dtype=pt.int32, device=pts.device)
    check(_lib.hip_lib().s3_spatial_order(_ptr(pts), int(pts.shape[0]), int(pts.shape[1]), _ptr(perm), _stream()),
          "s3_spatial_order")
    return perm


def referenced_rows(tables, n_src, coords=None):
    """the source rows the neighbour tables (int32 device tensors) reference: (used ids int32 [n_used] device, remap int32
    [n_src] device: position among the used rows or -1) -- mark / scan / compact on the device.  Ascending ids, or, with
    the points' coordinates ``coords`` [n_src, dim], the Hilbert-curve order of the referenced points."""
    dev = tables[0].device
    remap = pt.zeros(int(n_src), dtype=pt.int32, device=dev)
    for t in tables:
        check(_lib.hip_lib().s3_mark_rows(_ptr(t), int(t.numel()), int(n_src), _ptr(remap), _stream()), "s3_mark_rows")
    used = pt.empty(int(n_src), dtype=pt.int32, device=dev)
    n_used = C.c_int64(0)
    check(_lib.hip_lib().s3_compact_rows(_ptr(remap), int(n_src), _ptr(used), C.byref(n_used), _stream()),
          "s3_compact_rows")
    used = used[:n_used.value]
    if coords is not None and n_used.value > 1:
        # keep the referenced rows in Hilbert order of their coordinates instead of the CFD mesh's numbering
        pts = pt.empty((n_used.value, int(coords.shape[1])), dtype=pt.float64, device=dev)
        gather_rows(to_device(coords, pt.float64), used.contiguous(), pts)
        ordered = pt.empty((n_used.value, 1), dtype=pt.int32, device=dev)
        gather_rows(used.contiguous().reshape(-1, 1), spatial_order(pts), ordered)
        used = ordered.reshape(-1)
        check(_lib.hip_lib().s3_positions_of(_ptr(used), n_used.value, _ptr(remap), int(n_src), _stream()), "s3_positions_of")
    return used, remap


def remap_indices(idx, remap):
    """``idx[i] = remap[idx[i]]`` in place (int32 device tensors)"""
    check(_lib.hip_lib().s3_remap_indices(_ptr(idx), int(idx.numel()), _ptr(remap), int(remap.numel()), _stream()),
          "s3_remap_indices")
    return idx


def padded_rows(n_rows, row_len, dtype, dev, extra_lines=0):
    """[n_rows, row_len] view of a device buffer whose row pitch is a whole number of 128-byte lines (upload target for
    snapshot batches: every 128-B segment the planned kernel stages then sits on exactly one cache line).  For long rows
    the line count is moved to the next value = 3 (mod 4): a tile reads the same column of ~400 scattered rows at a
    time, and with a pitch of 2^n or 2^n + 1 lines those addresses load the memory channels unevenly (MI355X, 4000-B
    rows, same process: 32 lines 3.69 ms, 33: 3.66, 34: 3.41*, 35: 3.37*/3.54, 37..47: 3.52-3.53, 64: 3.44*; * = a
    faster box of the pool)"""
    item = pt.empty((), dtype=dtype).element_size()
    if row_len * item <= 64 and not extra_lines:
        # short rows (16 snapshots of a scalar field): whole 64-byte sectors, two rows per line -- half the footprint
        pitch = 16 // item if row_len * item <= 16 else (32 // item if row_len * item <= 32 else 64 // item)
        return pt.empty((n_rows, pitch), dtype=dtype, device=dev)[:, :row_len]
    per_line = 128 // item
    lines = (row_len + per_line - 1) // per_line
    if lines >= 16:
        while lines % 4 != 3 or lines % 32 == 31:
            lines += 1
    pitch = (lines + int(extra_lines)) * per_line
    return pt.empty((n_rows, pitch), dtype=dtype, device=dev)[:, :row_len]


# ---- refine kernels on the device-resident cell arrays ----------------------------------------------------------
def make_children(center, level, parents, new_index, width):
    dim = int(center.shape[1])
    check(_lib.hip_lib().s3_make_children(_ptr(center), _ptr(level), _ptr(parents), int(parents.numel()),
                                          int(new_index), dim, float(width), _stream()), "s3_make_children")


def child_gain(knn, k, center, level, first, n, width, level_factor, gain0, metric, gain, scratch):
    dim = int(center.shape[1])
    check(_lib.hip_lib().s3_child_gain(knn.handle, int(k), _ptr(center), _ptr(level), int(first), int(n), dim,
                                       float(width), _ptr(level_factor), float(gain0), _ptr(metric), _ptr(gain),
                                       _ptr(scratch), _stream()), "s3_child_gain")


def child_gain_reuse(knn, k, center, level, first, n, width, level_factor, gain0, metric, gain, scratch, parents,
                     parents_offset, child_metric):
    """``child_gain`` that keeps every cell's child predictions in ``child_metric`` [cap, 2^d] and, with ``parents`` (the
    batch's ordered parent ids), takes a new cell's centre value from its parent's entry instead of searching again"""
    dim = int(center.shape[1])
    check(_lib.hip_lib().s3_child_gain_reuse(knn.handle, int(k), _ptr(center), _ptr(level), int(first), int(n), dim,
                                             float(width), _ptr(level_factor), float(gain0), _ptr(metric), _ptr(gain),
                                             _ptr(scratch), _ptr(parents), int(parents_offset), _ptr(child_metric), _stream()),
          "s3_child_gain_reuse")


def child_gain_handoffs(scratch, n, dim):
    """the hand-off counts a ``child_gain_reuse`` call with ``parents`` over ``n`` cells left in its ``scratch`` (include/s3hip.h),
    in child points: (left by the per-cell wavefronts, left by the grouped search, left by the one-wavefront-per-query search
    to the per-lane search)"""
    nch = 2 ** int(dim)
    at = n * (nch + 1)                                      # the two lists: (counter, pad, n * 2^dim entries) int32 each
    rest = to_host(scratch[at:at + 1]).view(np.int32)
    rest2 = to_host(scratch[at + 1 + n * nch // 2:at + 2 + n * nch // 2]).view(np.int32)
    return int(rest2[1]), int(rest2[0]), int(rest[0])


class MaskCells:
    """the cells of a mask launch, described once for every ``mask_*`` (``s3_mask_cells`` of include/s3hip.h): ``center`` float64
    [rows, 2 | 3] and ``level`` int32 [rows] on the device, ``width`` of the root cell, and either ``cells`` (int32 [n] on the
    device: ordered ids) or the id range ``first .. first + n - 1`` (``n`` None: up to the last row).  Every launch ORs its verdicts
    into ``invalid`` uint8 [n or more] (zero it first).  Checked and turned into the C struct here once, not in every launch."""

    def __init__(self, center, level, width, invalid, cells=None, first=0, n=None):
        def array(t, dtype, least, what):               # (plain attribute reads: a refine loop builds one of these per batch)
            if not (isinstance(t, pt.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.numel() >= least):
                raise TypeError(f"MaskCells: {what} must be a contiguous {dtype} device tensor of at least {least} values")
            return t.data_ptr()
        if not (isinstance(center, pt.Tensor) and center.dim() == 2 and int(center.shape[1]) in (2, 3)):
            raise TypeError("MaskCells: center must be [rows, 2 | 3]")
        rows, self.dim = int(center.shape[0]), int(center.shape[1])
        self.n = int(len(cells) if cells is not None else (rows - first if n is None else n))
        self._arrays = (center, level, cells, invalid)                  # the struct points into them
        self.struct = _lib.S3MaskCells(array(center, pt.float64, rows * self.dim, "center"), array(level, pt.int32, rows, "level"),
                                       None if cells is None else array(cells, pt.int32, self.n, "cells"), int(first), self.n, self.dim,
                                       float(width), array(invalid, pt.uint8, self.n, "invalid"))
        self.ref = C.byref(self.struct)


def mask_box(cells, lo, hi, refine_mode, keep_inside):
    check(_lib.hip_lib().s3_mask_box(cells.ref, _host_ptr(_host_f64(lo)), _host_ptr(_host_f64(hi)), int(refine_mode), int(keep_inside),
                                     _stream()), "s3_mask_box")


def mask_sphere(cells, pos, radius, refine_mode, keep_inside):
    check(_lib.hip_lib().s3_mask_sphere(cells.ref, _host_ptr(_host_f64(pos)), float(radius), int(refine_mode), int(keep_inside),
                                        _stream()), "s3_mask_sphere")


def mask_cylinder(cells, p0, axis, norm, r0, r1, is_cone, refine_mode, keep_inside):
    check(_lib.hip_lib().s3_mask_cylinder(cells.ref, _host_ptr(_host_f64(p0)), _host_ptr(_host_f64(axis)), float(norm), float(r0),
                                          float(r1), int(is_cone), int(refine_mode), int(keep_inside), _stream()), "s3_mask_cylinder")


def mask_polygon(cells, poly_dev, refine_mode, keep_inside):
    check(_lib.hip_lib().s3_mask_polygon(cells.ref, _ptr(poly_dev), int(poly_dev.shape[0]), int(refine_mode), int(keep_inside),
                                         _stream()), "s3_mask_polygon")


def mask_triangle(cells, points, refine_mode, keep_inside):
    check(_lib.hip_lib().s3_mask_triangle(cells.ref, _host_ptr(_host_f64(points, 6)), int(refine_mode), int(keep_inside), _stream()),
          "s3_mask_triangle")


def mask_prism(cells, origin, axis, norm, dims, triangle, refine_mode, keep_inside):
    check(_lib.hip_lib().s3_mask_prism(cells.ref, _host_ptr(_host_f64(origin)), _host_ptr(_host_f64(axis)), float(norm),
                                       _host_ptr(np.ascontiguousarray(dims, dtype=np.int32)), _host_ptr(_host_f64(triangle, 6)),
                                       int(refine_mode), int(keep_inside), _stream()), "s3_mask_prism")


def mask_tetrahedra(cells, positions, normals, refine_mode, keep_inside):
    """positions [n_tets, 4, 3], normals [n_tets, 3, 4] (inward; column p belongs to point p)"""
    pos, nrm = np.ascontiguousarray(positions, dtype=np.float64), np.ascontiguousarray(normals, dtype=np.float64)
    n_tets = int(pos.shape[0])
    if pos.shape != (n_tets, 4, 3) or nrm.shape != (n_tets, 3, 4):
        raise ValueError("mask_tetrahedra: positions [n_tets,4,3] and normals [n_tets,3,4] expected")
    check(_lib.hip_lib().s3_mask_tetrahedra(cells.ref, _host_ptr(pos), _host_ptr(nrm), n_tets, int(refine_mode), int(keep_inside),
                                            _stream()), "s3_mask_tetrahedra")


class MeshTable:
    """device image of a closed triangle mesh for ``mask_mesh``: facets ``tri [nt, 3, 3]`` (vertices of a facet in
    lexicographic order), bounding box ``lo`` / ``hi`` and the CSR column table ``(ny, nz, bin_start, bin_facet)`` of
    ``geometry.geometry_STL_3d.build_column_bins`` -- uploaded once; the table is checked here, the kernel trusts it"""

    def __init__(self, tri, lo, hi, ny, nz, bin_start, bin_facet):
        tri = np.ascontiguousarray(tri, dtype=np.float64)
        bin_start = np.ascontiguousarray(bin_start, dtype=np.int32)
        bin_facet = np.ascontiguousarray(bin_facet, dtype=np.int32)
        self.nt, self.ny, self.nz = int(tri.shape[0]), int(ny), int(nz)
        if tri.shape != (self.nt, 3, 3) or self.nt < 1:
            raise ValueError("MeshTable: facets [nt, 3, 3] expected")
        if (self.ny < 1 or self.nz < 1 or bin_start.shape != (self.ny * self.nz + 1,) or bin_start[0] != 0
                or (np.diff(bin_start) < 0).any() or bin_start[-1] != len(bin_facet)
                or (len(bin_facet) and (bin_facet.min() < 0 or bin_facet.max() >= self.nt))):
            raise ValueError("MeshTable: inconsistent column table")
        self.lo, self.hi = _host_f64(lo), _host_f64(hi)
        self.tri = to_device(tri)
        self.bin_start = to_device(bin_start)
        self.bin_facet = to_device(bin_facet if len(bin_facet) else np.zeros(1, dtype=np.int32))


def mask_mesh(cells, mesh, refine_mode, keep_inside):
    if cells.dim != 3:
        raise ValueError("mask_mesh: a triangle mesh is a 3-D body")
    check(_lib.hip_lib().s3_mask_mesh(cells.ref, _ptr(mesh.tri), mesh.nt, _host_ptr(mesh.lo), _host_ptr(mesh.hi), _ptr(mesh.bin_start),
                                      _ptr(mesh.bin_facet), mesh.ny, mesh.nz, int(refine_mode), int(keep_inside), _stream()), "s3_mask_mesh")


# per kind a ``kernel_spec()`` can name (its first entry; geometry/geometry_base.py lists them): the launcher, and for what a kernel
# reads on the device the upload of the spec's operands (the vertices of a polygon, the table of a mesh)
MASK_BODIES = {"box": mask_box, "sphere": mask_sphere, "cylinder": mask_cylinder, "polygon": mask_polygon, "triangle": mask_triangle,
               "prism": mask_prism, "tetrahedra": mask_tetrahedra, "mesh": mask_mesh}
MASK_UPLOADS = {"polygon": lambda xy: to_device(np.ascontiguousarray(xy, dtype=np.float64)), "mesh": MeshTable}


def mask_operands(spec):
    """the operands ``mask_body`` takes for a ``kernel_spec()`` -> (operands, uploaded): with ``uploaded`` they are device-resident
    and worth keeping, once per geometry; the other kinds' pass through"""
    upload = MASK_UPLOADS.get(spec[0])
    return (tuple(spec[1:]), False) if upload is None else ((upload(*spec[1:]),), True)


def mask_body(cells, kind, operands, refine_mode, keep_inside):
    """one launch of the body ``kind`` (the first entry of a ``kernel_spec()``) with the ``operands`` of ``mask_operands``"""
    if kind not in MASK_BODIES:
        raise NotImplementedError(f"geometry kind {kind!r} has no device kernel")
    MASK_BODIES[kind](cells, *operands, refine_mode, keep_inside)


def commit_batch(leaf, gain, parents, first, n_new, invalid):
    n_par = int(parents.numel()) if parents is not None else 0
    check(_lib.hip_lib().s3_commit_batch(_ptr(leaf), _ptr(gain), _ptr(parents), n_par, int(first), int(n_new),
                                         _ptr(invalid), _stream()), "s3_commit_batch")


def sumsq_leaf(metric, leaf, begin, end, out, scratch):
    check(_lib.hip_lib().s3_sumsq_leaf(_ptr(metric), _ptr(leaf), int(begin), int(end), _ptr(out), _ptr(scratch),
                                       _stream()), "s3_sumsq_leaf")


def sumsq_blocks(metric, leaf, n_cells, block_begin, block_end, partial):
    check(_lib.hip_lib().s3_sumsq_blocks(_ptr(metric), _ptr(leaf), int(n_cells), int(block_begin), int(block_end),
                                         _ptr(partial), _stream()), "s3_sumsq_blocks")


def sum_ordered(values, n, out):
    check(_lib.hip_lib().s3_sum_ordered(_ptr(values), int(n), _ptr(out), _stream()), "s3_sum_ordered")


def topn_leaf(gain, leaf, n_cells, n_top, scratch):
    """-> numpy int32 ids ordered like heapq.nlargest(n_top, leaves, key=(gain, -id))  (s_cube.py:601-602)."""
    out = np.empty(max(int(n_top), 1), dtype=np.int32)
    cnt = C.c_int64(0)
    check(_lib.hip_lib().s3_topn_leaf(_ptr(gain), _ptr(leaf), int(n_cells), int(n_top),
                                      out.ctypes.data_as(C.c_void_p), C.byref(cnt), _ptr(scratch), _stream()),
          "s3_topn_leaf")
    return out[:cnt.value]


def topn_scratch(n_cells, n_top, dev):
    return _scratch(_lib.hip_lib().s3_topn_scratch_bytes(int(n_cells), int(n_top)), dev)
