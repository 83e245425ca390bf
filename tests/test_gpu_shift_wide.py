"""
The in-place interpolation kernel in its 512-thread form (interp_planned_shift_kernel: eight lanes per cell and per staged row,
eight staging passes of 64 rows): what the lane mapping can get wrong, on tile plans whose shape is CHOSEN -- the neighbour
tables below are written tile by tile, so that the plan's greedy packing (plan_build.hip: cells in the order given when no
centres are passed, a tile closed at 64 cells, when the next cell would push it past `ucap` distinct rows, or at the end of a
512-cell packing block) produces tiles with exactly the cell and row counts a case asks for.  The reference is the direct
gather kernel on the same table, bit for bit; the first test also sends its tiles through the pitched-copy kernel
(interp_planned_kernel<T, 64>), which has the same workgroup shape.  GPU only.
"""
import numpy as np
import pytest
import torch as pt

pytestmark = pytest.mark.gpu

TC = 64                 # cells of a full tile
BLOCK = 8 * TC          # cells of a packing block: a tile never spans two
N_POINTS = 4096         # rows of the source table


@pytest.fixture(scope="module")
def ops():
    from sparsespatialsampling_amd import hipops
    hipops.device()
    return hipops


@pytest.fixture(scope="module")
def orc():
    from oracle import s3_oracle
    return s3_oracle


def ucap(k):
    """distinct rows a 64-cell tile may hold (plan_ucap: what 80 KiB of LDS leave beside the tile's tables, at most 512)"""
    return min((80 * 1024 - k * TC * 10) // 128 // 16 * 16, 512)


def tile_cells(rng, n_c, n_r, k, pool):
    """neighbour rows [n_c, k] of a tile that references exactly the first `n_r` rows of `pool`; the first cell holds
    min(k, n_r) distinct ones"""
    assert 1 <= n_r <= n_c * k and n_r <= len(pool)
    flat = np.concatenate([pool[:n_r], rng.choice(pool[:n_r], n_c * k - n_r)])
    head = min(k, n_r)
    flat[head:] = rng.permutation(flat[head:])
    return flat.reshape(n_c, k)


def build_table(rng, k, blocks, last=None):
    """idx [nc, k] from `blocks`: per 512-cell packing block a list of eight entries, each the row count n_r of a full tile or,
    as the LAST entry of a block only, a pair ((a, n_r_a), (64 - a, n_r_b)): a tile of `a` cells that is closed because the first
    cell of the next one (k fresh rows) would push it past ucap, and the tile the end of the block closes.  `last` = (n_c, n_r):
    one more tile of fewer than 64 cells, closed by the end of the table.  -> idx, [(n_c, n_r)] of the tiles in plan order"""
    cells, tiles = [], []
    for entries in blocks:
        assert len(entries) == 8
        for j, e in enumerate(entries):
            perm = rng.permutation(N_POINTS).astype(np.int32)
            if isinstance(e, tuple):
                (a, ra), (b, rb) = e
                assert j == 7 and a + b == TC and ra <= ucap(k) < ra + min(k, rb) and rb >= k
                cells += [tile_cells(rng, a, ra, k, perm[:ra]), tile_cells(rng, b, rb, k, perm[ra:ra + rb])]   # disjoint pools
                tiles += [(a, ra), (b, rb)]
            else:
                assert e <= ucap(k)
                cells.append(tile_cells(rng, TC, e, k, perm))
                tiles.append((TC, e))
    if last is not None:
        n_c, n_r = last
        assert n_c < TC
        cells.append(tile_cells(rng, n_c, n_r, k, rng.permutation(N_POINTS).astype(np.int32)))
        tiles.append((n_c, n_r))
    return np.concatenate(cells).astype(np.int32), tiles


def make_table(row_len, dtype, placement, seed):
    """a dense [N_POINTS, row_len] table: 16-byte aligned rows off the 128-byte line grid"""
    gen = pt.Generator(device="cuda").manual_seed(seed)
    numel = N_POINTS * row_len
    if placement == "dense":
        table = pt.empty((N_POINTS, row_len), dtype=dtype, device="cuda").normal_(generator=gen)
    elif placement == "offset16":                    # the table starts 16 bytes into a line
        skip = 16 // pt.empty((), dtype=dtype).element_size()
        buf = pt.empty(numel + skip, dtype=dtype, device="cuda").normal_(generator=gen)
        table = buf[skip:].view(N_POINTS, row_len)
        assert table.data_ptr() % 128 == 16
    else:                                            # "tail": the last row ends where the allocation ends
        item = pt.empty((), dtype=dtype).element_size()
        buf = pt.empty(32 * 2 * 1024 * 1024 // item, dtype=dtype, device="cuda").normal_(generator=gen)     # 32 x 2 MiB
        table = buf[buf.numel() - numel:].view(N_POINTS, row_len)
    row_bytes = table.stride(0) * table.element_size()
    assert row_bytes % 16 == 0 and table.data_ptr() % 16 == 0 and (row_bytes % 128 != 0 or table.data_ptr() % 128 != 0)
    return table


def run_case(ops, rng, k, idx_np, tiles, table, want_gy=None, want_tail=None):
    """plan the table, check the plan is the one that was written and the launch the one that was meant, interpolate and compare
    with the direct kernel bit for bit; -> (w, idx, got)"""
    nc = len(idx_np)
    idx = pt.from_numpy(idx_np).cuda()
    w = pt.from_numpy(rng.random((nc, k))).cuda()
    w /= w.sum(1, keepdim=True)
    plan = ops.InterpPlan(idx, N_POINTS)             # no centres: cells in the order given
    try:
        assert plan.n_tiles == len(tiles) and plan.total_rows == sum(r for _, r in tiles)
        route = plan.route(table)
        assert route["route"] == "shift"
        if want_gy is not None:
            assert (route["gy"] > 1) == want_gy
        if want_tail is not None:
            assert bool(route["tail"]) == want_tail
        got = plan.interp(w, table)
        assert pt.equal(got, ops.interp(w, idx, table.contiguous()))
        # the same tiles through the plan's source ids (s3_interp_planned_src, the benchmark's entry point)
        plan.set_source_ids(pt.arange(N_POINTS, dtype=pt.int32, device="cuda"), N_POINTS)
        assert plan.route(table, src=True)["route"] == "shift"
        assert pt.equal(plan.interp_src(table), got)
    finally:
        plan.close()
    return w, idx, got


# row counts around the boundaries of the eight 64-row staging passes: one pass, a pass boundary, the eighth pass partly filled
ROWS_26 = [[1, 63, 64, 65, 448, 449, 496, ((63, 480), (1, 26))],          # + tiles of 63 cells and of 1 cell
           [127, 128, 129, 470, 485, 26, 320, ((57, 471), (7, 30))],       # + 57 and 7 cells: a cell's lanes cut at a wave boundary
           [192, 193, 384, 385, 495, 2, 100, ((56, 496), (8, 200))],       # + 56 and 8 cells: the tile ends with a wavefront
           [256, 257, 447, 450, 460, 490, 33, ((55, 480), (9, 234))]]      # + 55 and 9 cells
ROWS_8 = [[1, 63, 64, 65, 448, 449, 496, 512],                             # k = 8: ucap = 512, all eight passes full
          [7, 8, 9, 127, 129, 500, 511, 300]]


@pytest.mark.parametrize("k,row_len,dtype,placement,last", [
    (26, 252, pt.float32, "dense", (7, 182)),        # 1008-byte rows: phases 0 .. 7, eight chunks, the last line partial
    (26, 200, pt.float32, "offset16", (1, 1)),       # 800-byte rows: phases 0 / 2 / 4 / 6 shifted by the table's 16 bytes; 7 chunks
    (26, 1000, pt.float32, "tail", (9, 40)),         # 4000-byte rows: phases 0 / 32 / 64 / 96 bytes; nothing behind the last row
    (26, 126, pt.float64, "dense", (63, 400)),       # f64: 1008-byte rows
    (8, 252, pt.float32, "dense", (8, 64)),          # k = 8 (up to 512 rows per tile)
    (8, 102, pt.float64, "tail", (1, 8)),            # f64: 816-byte rows, 7 chunks, the last one 48 bytes
    (11, 252, pt.float32, "dense", (9, 99)),         # a neighbour count outside {8, 26}, odd
    (5, 204, pt.float32, "offset16", (63, 1)),       # and a small odd one: 816-byte rows
])
def test_tiles_of_chosen_cell_and_row_counts(ops, orc, k, row_len, dtype, placement, last):
    """tiles of 1 / 7 / 8 / 9 / 55 / 56 / 57 / 63 / 64 cells and of 1 ... 496 (k = 8: 512) rows.  Shift route: dense rows whose
    length is a multiple of 16 but not of 128 bytes, six chunks or more (plan_route); the plans hold fewer than 2048 tiles, so the
    chunks of a tile are split into runs over several workgroups (gy > 1).  The first case is also held against the CPU oracle."""
    rng = np.random.default_rng(k * 1000 + row_len)
    blocks = ROWS_26 if k == 26 else ROWS_8 if k == 8 else [[min(r, ucap(k), TC * k) for r in b] for b in ROWS_8]
    idx_np, tiles = build_table(rng, k, blocks, last)
    for n_c in ((1, 7, 8, 9, 63, 64) if k == 26 else (last[0], 64)):
        assert any(t[0] == n_c for t in tiles)
    table = make_table(row_len, dtype, placement, seed=row_len + k)
    w, idx, got = run_case(ops, rng, k, idx_np, tiles, table, want_gy=True, want_tail=False)
    # the same tiles on a pitched copy of the table (rows on the 128-byte grid): interp_planned_kernel<T, 64>, which shares the
    # 512-thread shape (a plan of fewer than 64 tiles never takes the persistent kernel)
    pitched = ops.padded_rows(N_POINTS, row_len, dtype, "cuda")
    pitched.copy_(table)
    plan = ops.InterpPlan(idx, N_POINTS)
    try:
        assert plan.route(pitched)["route"] == "chunk64"
        assert pt.equal(plan.interp(w, pitched), got)
    finally:
        plan.close()
    if (k, row_len) == (26, 252):
        ref = orc.interp(w.cpu().numpy(), idx.cpu().numpy(), table.contiguous().cpu().numpy().reshape(N_POINTS, 1, row_len))
        assert np.abs(got.cpu().numpy() - ref.reshape(len(idx_np), row_len)).max() <= 1e-13 * np.abs(ref).max()


@pytest.mark.parametrize("k,row_len,dtype,n_blocks,gy,tail", [
    (26, 200, pt.float32, 128, True, False),         # 1024 tiles: two runs of the 7 chunks, 4 + 3 (the two-step loop ends mid-iteration)
    (26, 300, pt.float32, 128, True, False),         # 10 chunks in runs of 5 + 5, the last line 48 bytes
    (26, 200, pt.float32, 256, False, False),        # 2048 tiles: one workgroup sweeps all 7 chunks
    (26, 252, pt.float32, 256, False, True),         # 8 chunks: the default tail map (4 runs of 2) behind full sweeps of 8
    (26, 260, pt.float32, 256, False, True),         # 9 chunks: full sweeps of an odd count, tail runs of 3 / 3 / 3 / 0
    (8, 130, pt.float64, 256, False, True),          # f64, k = 8: 1040-byte rows, 9 chunks
])
def test_chunk_sweeps_runs_and_the_tail_map(ops, k, row_len, dtype, n_blocks, gy, tail):
    """plans large enough that a workgroup sweeps several chunks of its tile: odd and even chunk counts per sweep, chunk runs
    (gy > 1: fewer than 2048 tiles) and the default tail map (2048 tiles and more, eight chunks and more), with the tiles of
    the first test at the front of the plan.  Shift route: dense 16-byte aligned rows off the line grid, seven chunks and more."""
    rng = np.random.default_rng(k * 1000 + row_len + n_blocks)
    special = ROWS_26 if k == 26 else ROWS_8
    filler = [[int(r) for r in rng.integers(k, min(ucap(k), TC * k) + 1, 8)] for _ in range(n_blocks - len(special))]
    idx_np, tiles = build_table(rng, k, special + filler, (7, 3 * k))
    assert len(tiles) >= n_blocks * 8
    table = make_table(row_len, dtype, "dense", seed=row_len + k)
    run_case(ops, rng, k, idx_np, tiles, table, want_gy=gy, want_tail=tail)
