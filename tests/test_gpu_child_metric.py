"""
The refine's child-metric search (csrc/knn.hip) against the CPU oracle (oracle/s3_oracle.c: s3o_child_gain, a brute-force
restatement of sklearn's kd-tree query, its "distance" weights, numpy's pairwise sum and torch's inner sum; its bucket-grid
form above BRUTE_MAX_POINTS points), bit for bit, on the hostile cases of tests/child_metric_cases.py.  GPU only.

Per case and batch:
  a. the root batch through s3_child_gain (all 2^d + 1 points per lane) and s3_child_gain_reuse without parents: every
     per-point value (scratch rows, child-metric table), metric and gain;
  b. a second generation as the refine runs it: s3_make_children on a permuted subset of the root cells, then
     s3_child_gain_reuse with parents over the children in slices with first > 0 and parents_offset not a multiple of 2^d
     (the wavefront chain coop -> near -> far -> per-lane rest): every child value, metric and gain against the oracle
     evaluated on the children's centres as the GPU computed them.
The hand-off counts of every slice (hipops.child_gain_handoffs) say which stages answered; each batch's declared routes are
checked, and test_every_stage_and_sweep_is_reached checks that across the cases every stage answered and gave up something
and every grid-stride loop of the chain ran past its first sweep.
"""
import functools

import numpy as np
import pytest
import torch as pt

from tests import child_metric_cases as cmc

pytestmark = pytest.mark.gpu

STAGES = ("coop", "near", "far", "rest")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _mismatch(what, got, ref):
    """'' when got and ref are the same bits, else a short description of where they differ"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref)):
        return ""
    if got.shape != ref.shape:
        return f"{what}: shape {got.shape} != {ref.shape}"
    bad = np.argwhere(_bits(got) != _bits(ref))
    i = tuple(bad[0])
    return f"{what}: {len(bad)} of {got.size} differ, first at {i}: {got[i]!r} != {ref[i]!r}"


def _first_sweep(n, nch):
    """entries the first sweep of near / far / per-lane rest covers for a call over n cells (child_metric_launch's grids)"""
    near = min(-(-n // 2), 8192) * 2 * nch
    far = min(-(-(n * nch) // 2), 8192) * 2
    rest = min(-(-(n * nch) // 128), 256) * 128
    return near, far, rest


class _Reference:
    def __init__(self, x, y):
        from oracle import s3_oracle as orc
        self.orc, self.x, self.y = orc, x, y
        self.grid = orc.GridIndex(x) if len(x) > cmc.BRUTE_MAX_POINTS and not cmc.flat(x) else None

    def child_gain(self, k, centers, level, width):
        if self.grid is not None:
            return self.grid.child_gain(self.y, k, centers, level, width, cmc.GAIN0)
        return self.orc.child_gain(self.x, self.y, k, centers, level, width, cmc.GAIN0)

    def close(self):
        if self.grid is not None:
            self.grid.close()


@functools.lru_cache(maxsize=None)
def run_case(name):
    """runs one case on the GPU -> (mismatches, per batch [per slice (n, (coop_left, near_left, far_left))])"""
    from oracle import s3_oracle as orc
    from sparsespatialsampling_amd import hipops
    _, dim, k, occ, x, y, batches = cmc.case(name)
    nch, nq = 2 ** dim, 2 ** dim + 1
    dev = hipops.device()
    knn = hipops.KnnIndex(x, occ)
    knn.set_values(y)
    ref = _Reference(x, y)
    bad, handoffs = [], []
    const = len(y) > 1 and bool(np.all(y == y[0]))             # (const_y: a power of two, every gain exactly 0)
    try:
        for bi, b in enumerate(batches):
            n, first = len(b.centers), b.first
            parents, ch_c, ch_l = cmc.children(b, dim)
            F = first + n + 3                                    # first child id
            N = len(ch_c)
            cap = F + N + 2
            center = pt.full((cap, dim), float("nan"), dtype=pt.float64, device=dev)
            level = pt.zeros(cap, dtype=pt.int32, device=dev)
            center[first:first + n] = hipops.to_device(b.centers)
            level[first:first + n] = hipops.to_device(b.level)
            lf = hipops.to_device(orc.level_factor_table(b.width, dim))
            tag = f"batch {bi}"

            # ---- a. the root batch -------------------------------------------------------------------------------------
            m_ref, g_ref = ref.child_gain(k, b.centers, b.level, b.width)
            outside = np.r_[0:first, first + n:cap]
            for reuse in (False, True):
                metric = pt.full((cap,), float("nan"), dtype=pt.float64, device=dev)
                gain = pt.full((cap,), float("nan"), dtype=pt.float64, device=dev)
                scratch = pt.full((n * nq + 2 + n * nch,), float("nan"), dtype=pt.float64, device=dev)
                child = pt.full((cap, nch), float("nan"), dtype=pt.float64, device=dev)
                if reuse:
                    hipops.child_gain_reuse(knn, k, center, level, first, n, b.width, lf, cmc.GAIN0, metric, gain, scratch,
                                            None, 0, child)
                else:
                    hipops.child_gain(knn, k, center, level, first, n, b.width, lf, cmc.GAIN0, metric, gain, scratch)
                who = f"{tag} a {'s3_child_gain_reuse' if reuse else 's3_child_gain'}"
                m_h, g_h = hipops.to_host(metric), hipops.to_host(gain)
                bad += [f"{who} {e}" for e in (
                    _mismatch("scratch rows", hipops.to_host(scratch[:n * nq]).reshape(n, nq), m_ref),
                    _mismatch("metric", m_h[first:first + n], m_ref[:, 0]),
                    _mismatch("gain", g_h[first:first + n], g_ref)) if e]
                if not (np.isnan(m_h[outside]).all() and np.isnan(g_h[outside]).all()):
                    bad.append(f"{who}: metric / gain written outside the batch")
                if reuse:
                    c_h = hipops.to_host(child)
                    e = _mismatch("child-metric table", c_h[first:first + n], m_ref[:, 1:])
                    if e:
                        bad.append(f"{who} {e}")
                    if not np.isnan(c_h[outside]).all():
                        bad.append(f"{who}: child-metric table written outside the batch")
                if const and not np.all(g_h[first:first + n] == 0.0):
                    bad.append(f"{who}: a constant metric gave a non-zero gain")
            # (child holds the root batch's rows now: the second generation's centres take their values from it)

            # ---- b. the children, sliced as ranks slice a batch -------------------------------------------------------------
            d_par = hipops.to_device(parents.astype(np.int32))
            hipops.make_children(center, level, d_par, F, b.width)
            c_got = hipops.to_host(center[F:F + N])
            if not (np.array_equal(_bits(c_got), _bits(ch_c)) and np.array_equal(hipops.to_host(level[F:F + N]), ch_l)):
                bad.append(f"{tag} b: s3_make_children's centres or levels differ from the oracle's expression")
            m2, g2 = ref.child_gain(k, c_got, ch_l, b.width)
            metric = pt.full((cap,), float("nan"), dtype=pt.float64, device=dev)
            gain = pt.full((cap,), float("nan"), dtype=pt.float64, device=dev)
            per_slice = []
            for s, e in cmc.slices(b, dim):
                m = e - s
                scratch = pt.full((m * nq + 2 + m * nch,), float("nan"), dtype=pt.float64, device=dev)
                hipops.child_gain_reuse(knn, k, center, level, F + s, m, b.width, lf, cmc.GAIN0, metric, gain, scratch, d_par,
                                        s, child)
                ho = hipops.child_gain_handoffs(scratch, m, dim)
                per_slice.append((m, ho))
                err = _mismatch("scratch rows", hipops.to_host(scratch[:m * nq]).reshape(m, nq), m2[s:e])
                if err:
                    bad.append(f"{tag} b slice [{s}, {e}) hand-offs {ho}: {err}")
            c_h, m_h, g_h = hipops.to_host(child), hipops.to_host(metric), hipops.to_host(gain)
            bad += [f"{tag} b {e}" for e in (
                _mismatch("child values", c_h[F:F + N], m2[:, 1:]),
                _mismatch("metric", m_h[F:F + N], m2[:, 0]),
                _mismatch("gain", g_h[F:F + N], g2)) if e]
            if not (np.isnan(m_h[:F]).all() and np.isnan(m_h[F + N:]).all() and np.isnan(c_h[F + N:]).all()):
                bad.append(f"{tag} b: metric or child values written outside the children")
            if const and not np.all(g_h[F:F + N] == 0.0):
                bad.append(f"{tag} b: a constant metric gave a non-zero gain")
            handoffs.append(per_slice)
    finally:
        ref.close()
        knn.close()
    return bad, handoffs


def answered(n, ho, nch):
    """child points each stage answered in one call over n cells"""
    coop_left, near_left, far_left = ho
    return {"coop": n * nch - coop_left, "near": coop_left - near_left, "far": near_left - far_left, "rest": far_left}


def events(name):
    """what happened in the second generation of a case: stage answered / gave up, loop ran a second sweep"""
    _, dim, *_ = cmc.case(name)
    nch = 2 ** dim
    seen = set()
    for per_slice in run_case(name)[1]:
        for n, ho in per_slice:
            for st, cnt in answered(n, ho, nch).items():
                if cnt > 0:
                    seen.add(st)
            coop_left, near_left, far_left = ho
            seen |= {s for s, v in (("coop-", coop_left), ("near-", near_left), ("far-", far_left)) if v > 0}
            near1, far1, rest1 = _first_sweep(n, nch)
            seen |= {s for s, v in (("near sweep 2", coop_left > near1), ("far sweep 2", near_left > far1),
                                    ("rest sweep 2", far_left > rest1)) if v}
    return seen


@pytest.mark.parametrize("name", cmc.NAMES)
def test_child_metric_equals_oracle(name):
    bad, handoffs = run_case(name)
    assert not bad, f"{name}: " + "\n".join(bad)
    _, dim, *_, batches = cmc.case(name)
    nch = 2 ** dim
    for b, per_slice in zip(batches, handoffs):
        for n, ho in per_slice:
            coop_left, near_left, far_left = ho
            assert n * nch >= coop_left >= near_left >= far_left >= 0, (name, n, ho)
        total = {st: sum(answered(n, ho, nch)[st] for n, ho in per_slice) for st in STAGES}
        for st, want in b.routes.items():
            assert (total[st] > 0) == want, f"{name}: stage {st} answered {total[st]} child points ({per_slice})"


def test_every_stage_and_sweep_is_reached():
    """across the cases: every stage of the chain answered something, coop, near and far gave something up, and each
    grid-stride loop (near, far, per-lane rest) ran a second sweep -- no stage drops out of the suite unnoticed"""
    seen = set()
    for name in cmc.NAMES:
        seen |= events(name)
    want = {"coop", "coop-", "near", "near-", "far", "far-", "rest", "near sweep 2", "far sweep 2", "rest sweep 2"}
    assert want <= seen, f"never reached: {sorted(want - seen)}"
