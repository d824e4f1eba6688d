"""The row-sorted form of the chunked SpMV sweep (spmv_chunk_kernel<SORTED>, layout 2 of the chunk cache): the 512 words of a chunk are
stored in row order with a storage index, a run-start bit and two bits of the chunk's window bitmap each, and the sweep sums runs of
equal rows with one accumulator per lane.  The cases place run ends, bitmap gaps, cuts and the padding where that form can go wrong.
Every case forces BMSP_SPMV_CHUNK=1 (but the last), poisons y with NaN, asks three sweeps to be bitwise equal, compares with the oracle
within the bound of test_spmv_chunked.check, and pins the layout (bmsp_spmv_chunk_layout)."""
import numpy as np
import pytest
import util

pytestmark = pytest.mark.gpu

V = 512  # stored values per chunk (kChV)
CHUNK = "spmv_chunk_kernel"


@pytest.fixture
def force_chunks(monkeypatch):
    monkeypatch.setenv("BMSP_SPMV_CHUNK", "1")


def storage_rows(A):
    """row of every stored value in storage order: tile by tile, inside a tile by bitmap position (most significant bit first)"""
    k, b, _, _ = A.host_arrays()
    bits = np.unpackbits(np.ascontiguousarray(b).astype(">u8").view(np.uint8).reshape(-1, 8), axis=1)
    t, p = np.nonzero(bits)
    return (k[t] >> 32).astype(np.int64) * 8 + p // 8


def sweeps(bmsp, A, x, nr, n=3):
    dx = bmsp.DeviceArray.from_host(x)
    ys = []
    for _ in range(n):
        y = bmsp.DeviceArray(nr, np.float32)
        assert bmsp.lib().bmsp_memset(y.ptr, 0xFF, nr * 4) == 0  # NaN poison: every row must be written
        bmsp.check(bmsp.lib().bmsp_spmv(A.h, dx.ptr, y.ptr, 0, None))
        ys.append(y.to_host())
    assert np.all(np.isfinite(ys[0]))
    for yk in ys[1:]:
        np.testing.assert_array_equal(ys[0].view(np.uint8), yk.view(np.uint8))
    return ys[0]


def against_oracle(oracle, y, nr, nc, r, c, v, x):
    y_ref = oracle.spmv_f32(oracle.bmsp_from_coo(oracle.Coo(nr, nc, r, c, v), 0, False), x)
    S = util.scipy_csr(nr, nc, r, c, np.asarray(v, np.float32).astype(np.float64))
    bound = 1e-5 * (abs(S) @ np.abs(x.astype(np.float64))) + 1e-30
    assert np.all(np.abs(y - y_ref) <= bound + 1e-5 * np.abs(y_ref)), np.max(np.abs(y - y_ref))


def run(oracle, bmsp, nr, nc, cells, seed, layout=2, x=None):
    """builds the matrix of the distinct `cells`, checks kernel, layout, sweeps and oracle; returns (A, y, rows, cols)"""
    from pybmsp import gen
    cells = np.unique(np.asarray(cells, dtype=np.int64), axis=0)
    r, c = cells[:, 0].astype(np.int32), cells[:, 1].astype(np.int32)
    v = np.random.default_rng(seed).uniform(0.1, 1.0, len(cells))
    A = bmsp.BmSpMatrix.from_coo(nr, nc, r, c, v)
    assert bmsp.spmv_launch_info(A)["kernel"] == CHUNK
    assert bmsp.spmv_chunk_layout(A) == layout
    x = gen.spmv_x(nc, "cusp") if x is None else x
    y = sweeps(bmsp, A, x, nr)
    against_oracle(oracle, y, nr, nc, r, c, v, x)
    return A, y, r, c


def zero_rows_are_exact(y, nr, r):
    empty = np.setdiff1d(np.arange(nr), r)
    assert empty.size and np.all(y[empty].view(np.uint32) == 0)  # +0, not a rounded remainder and not -0


@pytest.mark.parametrize("nc,layout", [(1 << 20, 2), ((1 << 20) + 1, 1)])
def test_column_limit(oracle, bmsp, force_chunks, nc, layout):
    # 20 column bits + 9 + 1 + 2 fill the word: 2^20 columns take the row-sorted form, one column more keeps round 7
    g = np.random.default_rng(1)
    cells = np.stack([g.integers(0, 2000, 1500), g.integers(0, nc, 1500)], axis=1)  # a chunk spans about 700 rows
    cells = np.concatenate([cells, [[0, nc - 1], [1999, nc - 1], [1000, 0]]])
    run(oracle, bmsp, 4096, nc, cells, 1, layout=layout)


def test_every_value_its_own_row(oracle, bmsp, force_chunks):
    # every position is a run start and a run end
    g = np.random.default_rng(2)
    run(oracle, bmsp, 1024, 5000, np.stack([np.arange(1024), g.integers(0, 5000, 1024)], axis=1), 2)


def test_window_of_1024_rows(oracle, bmsp, force_chunks):
    # chunk 0: one value in each of rows 0, 2, ..., 1022 -- the bitmap reaches all 32 words with alternating bits; chunk 1 is partial
    g = np.random.default_rng(3)
    cells = np.concatenate([np.stack([np.arange(0, 1024, 2), g.integers(0, 3000, V)], axis=1),
                            np.stack([1024 + g.integers(0, 90, 100), g.integers(0, 3000, 100)], axis=1)])
    A, y, r, _ = run(oracle, bmsp, 1120, 3000, cells, 3)
    rows = storage_rows(A)
    assert np.array_equal(np.sort(rows[:V]), np.arange(0, 1024, 2))
    zero_rows_are_exact(y, 1120, r)


def test_one_long_row(oracle, bmsp, force_chunks):
    # row 21 holds 3 * 512 + 40 values: runs across every lane of chunks 1 and 2, one fold over 4 chunks; sparse rows around it
    g = np.random.default_rng(4)
    n = 3 * V + 40
    long_row = np.stack([np.full(n, 21), g.choice(20000, n, replace=False)], axis=1)
    around = np.stack([np.concatenate([g.integers(0, 16, 60), g.integers(16, 24, 40), g.integers(24, 200, 150)]), g.integers(0, 20000, 250)], axis=1)
    A, _, _, _ = run(oracle, bmsp, 208, 20000, np.concatenate([long_row, around]), 4)
    rows = storage_rows(A)
    chunks_of_long_row = np.unique(np.nonzero(rows == 21)[0] // V)
    assert chunks_of_long_row.size == 4


@pytest.mark.parametrize("stride", [8, 1])
def test_runs_end_around_lane_boundaries(oracle, bmsp, force_chunks, stride):
    # rows of exactly 7, 8, 9, 63, 64, 65 values back to back (216 per cycle, so the alignment differs in every chunk): runs end on, one
    # before and one after a lane boundary.  stride 8: every row its own block-row; stride 1: eight rows share the tiles of a block-row
    g = np.random.default_rng(5)
    sizes = [7, 8, 9, 63, 64, 65] * 8
    cells = np.concatenate([np.stack([np.full(k, stride * i), g.choice(6000, k, replace=False)], axis=1) for i, k in enumerate(sizes)])
    run(oracle, bmsp, stride * len(sizes) + 3, 6000, cells, 5)


def test_row_8b_then_row_8b_plus_8(oracle, bmsp, force_chunks):
    # block-rows 0..9 hold 500 values; block-row 10 has 12 values of rows 81..87 in its low tiles and 20 values of row 80 in its high tiles, so
    # the cut at 512 leaves chunk 1 only row 80 of block-row 10, followed by a full block-row 11: the row after 80 is 88
    g = np.random.default_rng(6)
    parts = [np.stack([8 * b + g.integers(0, 8, 50), np.arange(50) * 100 + g.integers(0, 100, 50)], axis=1) for b in range(10)]
    parts.append(np.stack([81 + np.arange(12) % 7, np.arange(12) * 8], axis=1))
    parts.append(np.stack([np.full(20, 80), 4000 + np.arange(20) * 8], axis=1))
    parts.append(np.stack([88 + np.arange(64) % 8, g.choice(6000, 64, replace=False)], axis=1))
    parts.append(np.stack([96 + g.integers(0, 300, 600), g.integers(0, 6000, 600)], axis=1))
    A, _, _, _ = run(oracle, bmsp, 400, 6000, np.concatenate(parts), 6)
    rows = storage_rows(A)
    in_chunk_1 = np.unique(rows[V:2 * V])
    assert in_chunk_1[0] == 80 and np.array_equal(in_chunk_1[1:9], np.arange(88, 96)) and rows[V - 1] // 8 == 10


def test_partial_block_rows_at_cuts(oracle, bmsp, force_chunks):
    # 60 values per block-row in rows 8b+1, 8b+4 and 8b+6 only: every cut falls inside a block-row, and the other rows of the head and tail
    # carries are exact zeros
    g = np.random.default_rng(7)
    cells = np.concatenate([np.stack([8 * b + g.choice([1, 4, 6], 60), g.choice(8000, 60, replace=False)], axis=1) for b in range(40)])
    A, y, r, _ = run(oracle, bmsp, 320, 8000, cells, 7)
    rows = storage_rows(A)
    cuts = np.arange(V, rows.size, V)
    assert np.all(rows[cuts] // 8 == rows[cuts - 1] // 8)
    zero_rows_are_exact(y, 320, r)


def test_row_and_block_row_gaps(oracle, bmsp, force_chunks):
    # values in block-rows 1, 2, 5, 6, 7, 12, 20, 21, ... only and there in two or three of the 8 rows: empty rows and empty block-rows
    # inside every window, before the first value and after the last
    g = np.random.default_rng(8)
    brs = np.array([1, 2, 5, 6, 7, 12, 20, 21, 22, 30, 31, 40, 41, 55, 56, 57, 58, 70, 90, 91])
    cells = np.concatenate([np.stack([8 * b + g.choice(g.choice(8, 3, replace=False), 45), g.choice(4000, 45, replace=False)], axis=1) for b in brs])
    _, y, r, _ = run(oracle, bmsp, 800, 4000, cells, 8)
    zero_rows_are_exact(y, 800, r)


def test_padding_adds_nothing(oracle, bmsp, force_chunks):
    # nnz % 512 != 0: the padding words of the last chunk name column 0; x[0] = inf must not be read (inf * 0 would be NaN).  Nothing is
    # stored in columns 0..7: the oracle multiplies whole tiles, so a tile over column 0 would give it 0 * inf
    from pybmsp import gen
    g = np.random.default_rng(9)
    cells = np.stack([g.integers(0, 600, 1300), 8 + g.integers(0, 2992, 1300)], axis=1)
    x = gen.spmv_x(3000, "cusp")
    x[0] = np.inf
    A, _, _, _ = run(oracle, bmsp, 600, 3000, cells, 9, x=x)
    assert A.info()["nnz"] % V != 0


def test_value_invalidation_keeps_the_cache(oracle, bmsp, force_chunks):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(13, 3, seed=7)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    assert bmsp.spmv_chunk_layout(A) == 2
    x = gen.spmv_x(n, "cusp")
    against_oracle(oracle, sweeps(bmsp, A, x, n), n, n, r, c, v, x)
    v2 = 1.5 - v
    A2 = bmsp.BmSpMatrix.from_coo(n, n, r, c, v2)
    d, s = A.device_arrays()[3], A2.device_arrays()[3]
    bmsp.check(bmsp.lib().bmsp_memcpy_d2d(d.ptr, s.ptr, d.n * 4))
    A.invalidate()
    assert bmsp.spmv_launch_info(A)["kernel"] == CHUNK and bmsp.spmv_chunk_layout(A) == 2
    against_oracle(oracle, sweeps(bmsp, A, x, n), n, n, r, c, v2, x)


def test_same_structure_same_bits(bmsp, force_chunks):
    # the cache build counts positions, it does not rank them by the return order of atomics: two builds of one COO sweep alike
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(13, 3, seed=11)
    x = gen.spmv_x(n, "cusp")
    ys = []
    for _ in range(2):
        A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
        assert bmsp.spmv_chunk_layout(A) == 2
        ys.append(sweeps(bmsp, A, x, n))
    np.testing.assert_array_equal(ys[0].view(np.uint8), ys[1].view(np.uint8))


def test_fallback_switch(oracle, bmsp, force_chunks, monkeypatch):
    # BMSP_SPMV_CHUNK_SORTED=0 keeps the round-7 words and body; the report is the same (same kernel name, same bytes)
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(13, 3, seed=12)
    default = bmsp.spmv_launch_info(bmsp.BmSpMatrix.from_coo(n, n, r, c, v))
    monkeypatch.setenv("BMSP_SPMV_CHUNK_SORTED", "0")
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    assert bmsp.spmv_chunk_layout(A) == 1
    assert bmsp.spmv_launch_info(A) == default and default["kernel"] == CHUNK
    x = gen.spmv_x(n, "cusp")
    against_oracle(oracle, sweeps(bmsp, A, x, n), n, n, r, c, v, x)


def test_default_path_takes_the_sorted_form(oracle, bmsp):
    # nothing forced: rmat(16, 2) has 379 chunks (the default takes the chunked sweep from 128) and fewer than 2 values per tile
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(16, 2)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    assert bmsp.spmv_launch_info(A)["kernel"] == CHUNK
    assert bmsp.spmv_chunk_layout(A) == 2
    assert (A.info()["nnz"] + V - 1) // V == 379
    x = gen.spmv_x(n, "cusp")
    against_oracle(oracle, sweeps(bmsp, A, x, n), n, n, r, c, v, x)
