"""The kernels that decide what the grid looks like (csrc/tree.hip) on the GPU: the leaf sums s3_sumsq_leaf / s3_sumsq_blocks /
s3_sum_ordered against long-double sums within a bound made of the depth of their fixed addition trees, and the radix select
s3_topn_leaf against the sorting oracle where its 96-bit key is hard: gains that differ in the bits of one chosen digit only, the
digit that straddles gain and id, ids at and beyond 2^24, every way of finishing, and both sides of the device / host ordering switch.

The sums' bound.  Every term m^2 >= 0 is one correctly rounded float64 product, the same in the kernel and in the reference (which
squares in float64, so that a square that underflows is zero for both, and adds in long double).  A sum of non-negative terms formed
by ANY tree of float64 additions is within ((1 + eps)^d - 1) ref <= (d + 2) eps ref of the exact sum, eps = 2^-53, d the longest
chain of additions a term passes through.  The trees (tree.hip):

* a workgroup of 256 lanes: each lane adds its terms one after the other (chain = the number of terms of the lane), then
  block_sum_256: six shuffle steps inside a wavefront (6) and ``(w0 + w1) + (w2 + w3)`` over the four wavefronts (2): 8.
* s3_sumsq_leaf over n cells: nb = min(1024, max(1, ceil(n / 1024))) workgroups, a lane takes every (256 nb)-th cell:
  ceil(n / (256 nb)) terms; a final workgroup adds the nb partial sums, ceil(nb / 256) per lane.
  d = ceil(n / (256 nb)) + 8 + ceil(nb / 256) + 8; 25 at n = 1024 * 1024 + 3.
* s3_sumsq_blocks: 1024 cells per workgroup, four per lane: d = 4 + 8 = 12 for each block sum.
* s3_sum_ordered over n values: d = ceil(n / 256) + 8; 28 at n = 5000.
"""
import numpy as np
import pytest
import torch as pt

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = 2.0 ** -53
CANARY = -7.25
GUARD = 64
WORST = {}


@pytest.fixture(scope="module")
def ops():
    from sparsespatialsampling_amd import hipops
    hipops.device()
    return hipops


@pytest.fixture(scope="module")
def orc():
    from oracle import s3_oracle
    return s3_oracle


def dev(a):
    return pt.from_numpy(np.ascontiguousarray(a)).cuda()


def ceil_div(a, b):
    return -(-a // b)


def depth_leaf(n):
    nb = min(1024, max(1, ceil_div(n, 1024)))
    return ceil_div(n, 256 * nb) + 8 + ceil_div(nb, 256) + 8


def depth_ordered(n):
    return ceil_div(n, 256) + 8


DEPTH_BLOCK = 4 + 8


def long_sum(values):
    """long-double sum of float64 values (exact to 2^-64 relative: the reference's own error is 2^-11 of one eps)"""
    return np.asarray(values, dtype=np.float64).astype(LD).sum() if len(values) else LD(0)


def within(got, ref, depth, family):
    assert depth < 64
    err, bound = abs(LD(got) - ref), LD(depth + 2) * LD(EPS) * ref
    ratio = 0.0 if err == 0 else float(err / bound) if bound > 0 else np.inf
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    return ratio <= 1.0


def metric_arrays(n, seed):
    """'wide': signed magnitudes from 1e-200 to 1e150, log-uniform (squares from 0 by underflow and subnormal to 1e300 in one array);
    'flat': magnitudes in [0.5, 2): every term matters to the sum, so the bound bites on all of them"""
    rng = np.random.default_rng(seed)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return {"wide": sign * 10.0 ** rng.uniform(-200.0, 150.0, n), "flat": sign * rng.uniform(0.5, 2.0, n)}


def squares(m):
    with np.errstate(under="ignore"):
        return m * m                                                               # float64, as the kernel forms them


def guarded(n, fill=CANARY):
    buf = pt.full((GUARD + n + GUARD,), fill, dtype=pt.float64, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf, n):
    host = buf.cpu().numpy()
    return bool((host[:GUARD] == CANARY).all() and (host[GUARD + n:] == CANARY).all())


# ---- leaf sums ------------------------------------------------------------------------------------------------------------------
N_LEAF = 1024 * 1024 + 3 + 1500


@pytest.fixture(scope="module")
def leaf_case():
    rng = np.random.default_rng(21)
    m = metric_arrays(N_LEAF, 21)
    leaf = rng.random(N_LEAF) < 0.6
    assert (squares(m["wide"]) == 0).any() and squares(m["wide"]).max() > 1e290
    return {k: (v, dev(v)) for k, v in m.items()}, leaf, dev(leaf.astype(np.uint8))


@pytest.mark.parametrize("kind", ["wide", "flat"])
def test_sumsq_leaf_ranges_against_the_long_double_sum(ops, leaf_case, kind):
    """ranges that start off a multiple of 256 and hold 0, 1, 255, 257 and 1024 * 1024 + 3 cells; output and scratch between canaries"""
    (m, m_dev), leaf, leaf_dev = leaf_case[0][kind], leaf_case[1], leaf_case[2]
    sq = squares(m)
    for begin in (3, 257, 1001):
        for count in (0, 1, 255, 257, 1024 * 1024 + 3):
            end = begin + count
            out_buf, out = guarded(1)
            s_buf, scratch = guarded(1024)
            ops.sumsq_leaf(m_dev, leaf_dev, begin, end, out, scratch)
            got = float(out.item())
            ref = long_sum(sq[begin:end][leaf[begin:end]])
            assert within(got, ref, depth_leaf(count), "sumsq_leaf"), (kind, begin, count, got, float(ref))
            if count == 0 or not leaf[begin:end].any():
                assert got == 0.0 and not np.signbit(got)
            if count == 1 and leaf[begin]:
                assert got == sq[begin]
            assert guards_intact(out_buf, 1) and guards_intact(s_buf, 1024)
            again = pt.zeros(1, dtype=pt.float64, device="cuda")
            ops.sumsq_leaf(m_dev, leaf_dev, begin, end, again, scratch)
            assert again.item() == got or (np.isnan(got) and np.isnan(again.item()))
    print(f"worst |error| / bound: {WORST}")


def test_sumsq_leaf_no_leaf_and_one_leaf(ops, leaf_case):
    """all leaves off: exactly 0.0; a single leaf anywhere in the range: exactly its m^2 (adding zeros is exact)"""
    m, m_dev = leaf_case[0]["wide"]
    n = N_LEAF
    out = pt.full((1,), CANARY, dtype=pt.float64, device="cuda")
    scratch = pt.full((1024,), CANARY, dtype=pt.float64, device="cuda")
    ops.sumsq_leaf(m_dev, pt.zeros(n, dtype=pt.uint8, device="cuda"), 5, n, out, scratch)
    assert out.item() == 0.0
    for i in (5, 260, 70_001, n - 1):
        leaf = pt.zeros(n, dtype=pt.uint8, device="cuda")
        leaf[i] = 1
        ops.sumsq_leaf(m_dev, leaf, 5, n, out, scratch)
        assert out.item() == squares(m[i:i + 1])[0], i
        ops.sumsq_leaf(m_dev, leaf, 5, i, out, scratch)                            # the leaf just outside the range
        assert out.item() == 0.0, i


@pytest.mark.parametrize("n_cells", [1, 1023, 1024, 1025, 5 * 1024 + 7])
def test_sumsq_blocks_and_sum_ordered(ops, n_cells):
    """every block sum against the long-double sum of its 1024 cells; a sub-range of blocks writes its own entries only; the ordered
    sum of the block sums against the long-double sum of all leaves"""
    rng = np.random.default_rng(n_cells)
    n_blocks = ceil_div(n_cells, 1024)
    for kind, m in metric_arrays(n_cells, n_cells).items():
        leaf = rng.random(n_cells) < 0.6
        if n_cells == 1:
            leaf[:] = True
        sq = np.where(leaf, squares(m), 0.0)
        m_dev, leaf_dev = dev(m), dev(leaf.astype(np.uint8))
        buf, partial = guarded(n_blocks)
        ops.sumsq_blocks(m_dev, leaf_dev, n_cells, 0, n_blocks, partial)
        got = partial.cpu().numpy()
        assert guards_intact(buf, n_blocks)
        for b in range(n_blocks):
            assert within(got[b], long_sum(sq[b * 1024:(b + 1) * 1024]), DEPTH_BLOCK, "sumsq_blocks"), (kind, b)
        if n_cells == 1:
            assert got[0] == sq[0]
        for b0, b1 in ((0, 0), (n_blocks - 1, n_blocks), (1, min(3, n_blocks))):
            if b0 > b1:
                continue
            buf2, part2 = guarded(n_blocks)
            part2.fill_(CANARY)
            ops.sumsq_blocks(m_dev, leaf_dev, n_cells, b0, b1, part2)
            host = part2.cpu().numpy()
            assert guards_intact(buf2, n_blocks)
            assert np.array_equal(host[b0:b1], got[b0:b1]) and (host[:b0] == CANARY).all() and (host[b1:] == CANARY).all(), (b0, b1)
        out_buf, out = guarded(1)
        ops.sum_ordered(partial, n_blocks, out)
        total = long_sum(sq)
        assert within(out.item(), total, DEPTH_BLOCK + depth_ordered(n_blocks), "sumsq_blocks + sum_ordered"), kind
        assert guards_intact(out_buf, 1)
    print(f"worst |error| / bound: {WORST}")


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 5000])
def test_sum_ordered_against_the_long_double_sum(ops, n):
    for kind, m in metric_arrays(max(n, 1), 77 + n).items():
        v = squares(m)[:n]
        buf, values = guarded(max(n, 1))
        values[:n] = dev(v) if n else values[:0]
        out_buf, out = guarded(1)
        ops.sum_ordered(values, n, out)
        got = out.item()
        assert within(got, long_sum(v), depth_ordered(n), "sum_ordered"), (kind, got)
        if n == 0:
            assert got == 0.0
        if n == 1:
            assert got == v[0]
        assert guards_intact(out_buf, 1) and guards_intact(buf, max(n, 1))
    print(f"worst |error| / bound: {WORST}")


# ---- top-N ------------------------------------------------------------------------------------------------------------------------
BYTE_GUARD = 512


def topn(ops, gain_dev, leaf_dev, n_cells, n_top):
    """s3_topn_leaf with its scratch buffer of exactly s3_topn_scratch_bytes between canary bytes"""
    from sparsespatialsampling_amd import _lib
    need = int(_lib.hip_lib().s3_topn_scratch_bytes(int(n_cells), int(n_top)))
    buf = pt.full((BYTE_GUARD + need + BYTE_GUARD,), 0xA5, dtype=pt.uint8, device="cuda")
    got = ops.topn_leaf(gain_dev, leaf_dev, n_cells, n_top, buf[BYTE_GUARD:BYTE_GUARD + need])
    assert bool((buf[:BYTE_GUARD] == 0xA5).all()) and bool((buf[BYTE_GUARD + need:] == 0xA5).all()), "a write outside the scratch buffer"
    return got


def check_topn(ops, orc, gain, leaf, n_tops):
    gain_dev, leaf_dev = dev(gain), dev(leaf.astype(np.uint8))
    ids = np.flatnonzero(leaf)
    for n_top in n_tops:
        got = topn(ops, gain_dev, leaf_dev, len(gain), n_top)
        want = orc.topn(gain[ids], ids, n_top)
        assert len(got) == min(n_top, len(ids)) and np.array_equal(got, want), n_top


def from_bits(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


ONE, INF, SUBNORMAL = 0x3FF0000000000000, 0x7FF0000000000000, 1 << 30


@pytest.mark.parametrize("base,sign", [(ONE, 1), (SUBNORMAL, 1), (INF, -1)], ids=["one", "subnormal", "inf"])
def test_topn_gains_that_differ_in_the_digit_that_straddles_gain_and_id(ops, orc, base, sign):
    """gains base + j ulp, j = 0 .. 15 (1.0 + j 2^-52; a subnormal; +inf and the fifteen largest finite numbers), each shared by some
    1500 leaves: the keys agree in digits 0 .. 4 and differ from digit 5 on, whose twelve bits are the gain's last four and the id's
    first eight.  Thresholds inside a gain class and exactly between two, n_top around the number of leaves"""
    n = 40_000
    rng = np.random.default_rng(base % 1000 + 3)
    j = rng.integers(0, 16, n)
    gain = from_bits(np.uint64(base) + (sign * j).astype(np.int64).astype(np.uint64))
    assert len(np.unique(gain)) == 16 and not np.isnan(gain).any() and (gain >= 0).all()
    leaf = rng.random(n) < 0.6
    leaves = int(leaf.sum())
    order = np.sort(gain[leaf])[::-1]
    between = [int((order >= g).sum()) for g in np.unique(gain)[[3, 8, 15]]]      # every leaf of the classes above taken, none below
    check_topn(ops, orc, gain, leaf, [1, 2, 777] + between + [between[1] + 1, between[1] - 1, leaves // 2, leaves - 1, leaves, leaves + 1])


@pytest.mark.parametrize("agree", [12, 24, 36, 48])
def test_topn_finishes_at_each_digit(ops, orc, agree):
    """gains whose top ``agree`` bits are those of 1.5 and whose next twelve take one of eight values (the rest zero): the first
    agree / 12 digit passes see one bin, the next one sees the eight classes.  n_top = the leaves of the classes above a value: the
    selection finishes there with the whole bin taken (s_in_bin == left); n_top inside a class: it runs on to the last digit, through
    the id bits"""
    n = 30_000
    rng = np.random.default_rng(agree)
    values = np.array([0, 5, 17, 900, 901, 2047, 3000, 4095], dtype=np.uint64)
    prefix = np.uint64(0x3FF8000000000000) & ~np.uint64((1 << (64 - agree)) - 1)
    gain = from_bits(prefix | (values[rng.integers(0, 8, n)] << np.uint64(64 - agree - 12)))
    assert len(np.unique(gain)) == 8 and (gain >= 1.0).all() and (gain < 2.0).all()
    leaf = rng.random(n) < 0.7
    leaves = int(leaf.sum())
    whole = [int((gain[leaf] >= g).sum()) for g in np.unique(gain)[[1, 4, 5, 7]]]
    check_topn(ops, orc, gain, leaf, whole + [w + 7 for w in whole] + [whole[1] - 1, 1, leaves - 1, leaves, leaves + 1])


def test_topn_ids_at_and_beyond_2_24(ops, orc):
    """2^24 + 4096 cells with equal gains, built on the device; some thousand leaves on both sides of 2^12, of 2^24 and at the end: the
    id bits alone decide (they fill digits 5 .. 7, and ids >= 2^24 reach into digit 5), the oracle only sorts the leaves"""
    n = (1 << 24) + 4096
    gain = pt.full((n,), 0.375, dtype=pt.float64, device="cuda")
    leaf = pt.zeros(n, dtype=pt.uint8, device="cuda")
    ids = np.concatenate([np.arange(0, 11), np.arange(4096 - 1000, 4096 + 1000, 1), np.arange((1 << 24) - 1500, (1 << 24) + 1500, 2),
                          np.arange((1 << 24) + 1501, (1 << 24) + 1600), np.arange(n - 1000, n)])
    leaf[pt.from_numpy(ids).cuda()] = 1
    ones = np.full(len(ids), 0.375)
    below_2_24 = int((ids < (1 << 24)).sum())
    for n_top in (1, 11 + 1000, 11 + 1001, below_2_24 - 1, below_2_24, below_2_24 + 1, below_2_24 + 900, len(ids) - 1, len(ids), len(ids) + 1):
        got = topn(ops, gain, leaf, n, n_top)
        assert np.array_equal(got, orc.topn(ones, ids, n_top)), n_top


@pytest.mark.parametrize("n_top", [262143, 262144, 262145])
def test_topn_at_the_switch_between_device_ranking_and_host_sort(ops, orc, n_top):
    """RANK_MAX = 262144 selected ids are ordered on the device, one more by the host's sort; fifty distinct gains over 320 000 leaves:
    the order inside the result is decided by the id on either side"""
    n = 400_000
    rng = np.random.default_rng(5)
    gain = rng.integers(0, 50, n) / 64.0
    leaf = rng.random(n) < 0.8
    assert leaf.sum() > 262145 + 1000
    check_topn(ops, orc, gain, leaf, [n_top])
