"""
The array plumbing the front-ends and hipops share, without a device: the pure layout function of hipops and ``_field_rows`` on CPU
tensors, ``_component_groups``, and ``arrays.as_tensor`` / ``default_neighbors`` / ``Side`` (host inputs) / ``RunningMoments.merge``.

The expected layouts are literals, worked out by hand from the three functions that computed them separately before
(``_pitched_rows``, ``_pitched_matrix``, ``InterpPlan._layout``): ``(row_len, stride)`` is ``(prod(shape[1:]), the same)`` for a
contiguous tensor, ``(shape[1], stride(0))`` for a 2-D view with unit inner stride and ``stride(0) >= shape[1]``, refused otherwise.
torch calls a tensor contiguous whatever the stride of an axis of length 1 (or when it is empty), so a single row of a wider buffer
is dense.
"""
import numpy as np
import pytest
import torch as pt

from sparsespatialsampling_amd import arrays, hipops, metrics

N, T, L, C = 5, 6, 4, 3


def _cases(dtype):
    buf = pt.arange(N * T, dtype=dtype).reshape(N, T)
    cube = pt.arange(N * C * T, dtype=dtype).reshape(N, C, T)
    # name -> (tensor, _row_layout, _field_rows); None: refused
    return {
        "[n]": (buf[:, 0].clone(), (1, 1), (1, 1, 1)),
        "[n, T]": (buf, (6, 6), (1, 6, 6)),
        "buf[:, :L]": (buf[:, :L], (4, 6), (1, 4, 6)),
        "buf[:, 1:L]": (buf[:, 1:L], (3, 6), (1, 3, 6)),
        "buf[:, ::2]": (buf[:, ::2], None, None),
        "buf.t()": (buf.t(), None, None),
        "[n, c, T]": (cube, (18, 18), (3, 6, 18)),
        "[n, c, T][:, :, :L]": (cube[:, :, :L], None, None),
        "expanded row": (buf[:1].expand(N, T), None, None),
        "buf[:1, :L]": (buf[:1, :L], (4, 4), (1, 4, 4)),
        "buf[:, :0]": (buf[:, :0], (0, 0), (1, 0, 0)),
        "no rows": (buf[:0], (6, 6), (1, 6, 6)),
    }


@pytest.mark.parametrize("dtype", [pt.float32, pt.float64], ids=["f32", "f64"])
def test_row_layout_and_field_rows(dtype):
    for name, (t, layout, rows) in _cases(dtype).items():
        assert hipops._row_layout(t) == layout, name
        if rows is None:
            with pytest.raises(TypeError, match="probe"):
                hipops._field_rows(t, "probe")
        else:
            assert hipops._field_rows(t, "probe") == rows, name
    assert hipops._row_layout(pt.zeros((), dtype=dtype)) is None
    cube = pt.zeros((N, C, T), dtype=dtype)
    with pytest.raises(TypeError, match="iso_count"):                     # scalar node fields only
        hipops._field_rows(cube, "iso_count", 2)
    assert hipops._field_rows(cube[:, 0, :L], "iso_count", 2) == (1, 4, 18)


def test_layout_of_the_planned_kernels_keeps_its_own_rules():
    """``InterpPlan._layout`` adds the 16-byte rule and the k = 8 | 26 exception to the shared layout"""
    layout = hipops.InterpPlan._layout
    buf = pt.zeros((N, 8), dtype=pt.float64)
    assert layout(buf) == (8, 8) and layout(buf[:, :5]) == (5, 8) and layout(buf[:, :7][:, ::2]) is None
    ragged = pt.zeros((N, 5), dtype=pt.float64)
    assert layout(ragged) is None and layout(ragged, 8) == (5, 5) and layout(ragged, 26) == (5, 5) and layout(ragged, 7) is None
    assert layout(pt.zeros((N, 1), dtype=pt.float64), 8) is None          # shorter than one vector
    assert layout(buf.to(pt.int32)) is None and layout(pt.zeros(())) is None


def test_component_groups():
    want = {1: [(0, 1)], 2: [(0, 2)], 3: [(0, 3)], 4: [(0, 3), (3, 1)], 5: [(0, 3), (3, 2)], 6: [(0, 3), (3, 3)],
            7: [(0, 3), (3, 3), (6, 1)]}
    for n_comp, groups in want.items():
        assert list(hipops._component_groups(n_comp)) == groups


def test_as_tensor():
    a = np.arange(12.0).reshape(3, 4)
    t = arrays.as_tensor(a, "points")
    assert isinstance(t, pt.Tensor) and t.data_ptr() == a.ctypes.data
    strided = arrays.as_tensor(a[:, ::2], "points")
    assert strided.is_contiguous() and np.array_equal(strided.numpy(), a[:, ::2])
    assert arrays.as_tensor(t, "points") is t
    with pytest.raises(TypeError, match="points must be a numpy array or a torch tensor, got list"):
        arrays.as_tensor([[0.0, 1.0]], "points")


def test_default_neighbors_with_both_caps():
    # gradients: the other points of the cloud and what one search returns
    cap = lambda n_points: min(n_points - 1, hipops.GRAD_MAX_K)             # noqa: E731
    assert arrays.default_neighbors(2, None, cap(1000)) == 8 and arrays.default_neighbors(3, None, cap(1000)) == 26
    assert arrays.default_neighbors(2, None, cap(5)) == 4 and arrays.default_neighbors(3, 500, cap(1000)) == 63
    # reconstruction: the cell centres
    assert arrays.default_neighbors(3, None, 11) == 11 and arrays.default_neighbors(2, 5, 1000) == 5
    with pytest.raises(ValueError, match="positive"):
        arrays.default_neighbors(2, 0, 1000)


def test_side_of_host_inputs():
    result = pt.arange(4.0)
    back = arrays.Side(np.zeros(3)).back(result)
    assert isinstance(back, np.ndarray) and np.array_equal(back, result.numpy())
    side = arrays.Side(pt.zeros(3))
    assert side.host and not side.numpy and side.back(result) is result


def test_running_moments_merge_is_update(monkeypatch):
    """``update`` is ``merge`` of the batch's moments, and ``merge`` keeps the expressions of Chan's update as they were: the same bits"""
    monkeypatch.setattr(metrics, "temporal_moments", lambda b, unbiased=True: (b.mean(-1), b.std(-1, unbiased=unbiased)))
    rng = np.random.default_rng(3)
    batches = [pt.from_numpy(rng.standard_normal((7, n_b)) + 3.0) for n_b in (4, 1, 9)]
    updated, merged = metrics.RunningMoments(), metrics.RunningMoments()
    count, mean, m2 = 0, None, None
    for b in batches:
        n_b = b.shape[-1]
        mean_b, std_b = metrics.temporal_moments(b, unbiased=False)
        m2_b = std_b * std_b * n_b
        updated.update(b)
        assert merged.merge(n_b, mean_b, m2_b) is merged
        if count == 0:
            count, mean, m2 = n_b, mean_b, m2_b
        else:
            n = count + n_b
            delta = mean_b - mean
            mean = mean + delta * (n_b / n)
            m2 = m2 + m2_b + delta * delta * (count * n_b / n)
            count = n
        assert updated.count == merged.count == count
        for got in (updated, merged):
            assert np.array_equal(got.mean().numpy(), mean.numpy()) and np.array_equal(got._m2.numpy(), m2.numpy())
    assert np.array_equal(updated.std().numpy(), merged.std().numpy())
    assert np.abs(merged.std().numpy() - pt.cat(batches, 1).std(-1).numpy()).max() < 1e-12
