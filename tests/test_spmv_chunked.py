"""The chunked SpMV sweep (spmv_chunk_kernel): one wave per 512 stored values, cut anywhere in storage order, folded block-rows through
carry slots.  The cases reach it through BMSP_SPMV_CHUNK=1 (by default small matrices and tiles of >= 2 values keep the value-stream
kernel) -- except the two that check the default choice; every
case is checked against the oracle with NaN-poisoned outputs and must be bitwise identical across two sweeps."""
import numpy as np
import pytest
import util

pytestmark = pytest.mark.gpu

V = 512  # stored values per chunk (kChV)
CHUNK = "spmv_chunk_kernel"


@pytest.fixture
def force_chunks(monkeypatch):
    monkeypatch.setenv("BMSP_SPMV_CHUNK", "1")


def sweep(bmsp, A, x, nr, out_dtype=np.float32):
    dx = bmsp.DeviceArray.from_host(x)
    ys = []
    for _ in range(2):
        y = bmsp.DeviceArray(nr, out_dtype)
        assert bmsp.lib().bmsp_memset(y.ptr, 0xFF, nr * y.dtype.itemsize) == 0  # NaN poison: every row must be written
        bmsp.check(bmsp.lib().bmsp_spmv(A.h, dx.ptr, y.ptr, 0, None))
        ys.append(y.to_host())
    assert np.all(np.isfinite(ys[0]))
    np.testing.assert_array_equal(ys[0].view(np.uint8), ys[1].view(np.uint8))
    return ys[0]


def check(oracle, bmsp, nr, nc, r, c, v, kernel=CHUNK):
    """fp32 case: the launched kernel, then y against the oracle within check_spmv's bound"""
    from pybmsp import gen
    A = bmsp.BmSpMatrix.from_coo(nr, nc, r, c, v)
    name = bmsp.spmv_launch_info(A)["kernel"]
    assert name.startswith(kernel), name
    x = gen.spmv_x(nc, "cusp")
    y = sweep(bmsp, A, x, nr)
    y_ref = oracle.spmv_f32(oracle.bmsp_from_coo(oracle.Coo(nr, nc, r, c, v), 0, False), x)
    S = util.scipy_csr(nr, nc, r, c, np.asarray(v, np.float32).astype(np.float64))
    bound = 1e-5 * (abs(S) @ np.abs(x.astype(np.float64))) + 1e-30
    assert np.all(np.abs(y - y_ref) <= bound + 1e-5 * np.abs(y_ref)), np.max(np.abs(y - y_ref))
    return A


def coo(nr, nc, cells, seed=0):
    cells = np.unique(np.asarray(cells, dtype=np.int64), axis=0)
    vals = np.random.default_rng(seed).uniform(0.1, 1.0, len(cells))
    return nr, nc, cells[:, 0].astype(np.int32), cells[:, 1].astype(np.int32), vals


def random_cells(nr, nc, nnz, seed):
    g = np.random.default_rng(seed)
    return np.stack([g.integers(0, nr, nnz), g.integers(0, nc, nnz)], axis=1)


def test_chunk_boundary_inside_tile(oracle, bmsp, force_chunks):
    # about 5 values per tile: most of the 512-value cuts fall inside a tile
    nr = 4096
    g = np.random.default_rng(1)
    tiles = np.stack([g.integers(0, nr // 8, 1500), g.integers(0, nr // 8, 1500)], axis=1)
    cells = [(8 * br + p // 8, 8 * bc + p % 8) for br, bc in tiles for p in g.choice(64, 5, replace=False)]
    nr, nc, r, c, v = coo(nr, nr, cells, 1)
    A = check(oracle, bmsp, nr, nc, r, c, v)
    o = A.host_arrays()[2].astype(np.int64)
    assert np.any(o[:-1] // V != (o[1:] - 1) // V)  # some tile straddles a cut


def test_hub_block_row_many_chunks(oracle, bmsp, force_chunks):
    # block-row 3 holds > 20 K tiles (about 60 chunks): one fold over all of them; sparse rows around it
    nr, nc = 8192, 200000
    g = np.random.default_rng(2)
    hub = np.stack([24 + g.integers(0, 8, 30000), np.arange(30000) * 6 + g.integers(0, 6, 30000)], axis=1)
    rest = random_cells(nr, nc, 6000, 3)
    nr, nc, r, c, v = coo(nr, nc, np.concatenate([hub, rest]), 2)
    A = check(oracle, bmsp, nr, nc, r, c, v)
    k = A.host_arrays()[0]
    assert np.count_nonzero((k >> 32) == 3) > 20000


@pytest.mark.parametrize("nnz", [100, V, 3 * V - 36])
def test_nnz_around_one_chunk(oracle, bmsp, force_chunks, nnz):
    g = np.random.default_rng(nnz)
    cells = set()
    while len(cells) < nnz:  # 800 rows: every chunk within the 1024-row window
        cells.add((int(g.integers(0, 800)), int(g.integers(0, 3000))))
    nr, nc, r, c, v = coo(800, 3000, sorted(cells), nnz)
    assert r.size == nnz
    check(oracle, bmsp, nr, nc, r, c, v)


def test_empty_rows_and_block_rows_at_cuts(oracle, bmsp, force_chunks):
    # values only in every third block-row (16 each, so that a chunk spans < 1024 rows), rows 0..15 and the last 40 rows empty: empty
    # block-rows sit before the first value, between chunks and after the last value
    nr = 6000
    g = np.random.default_rng(4)
    brs = np.arange(2, nr // 8 - 5, 3)
    cells = [(8 * br + int(g.integers(0, 8)), int(g.integers(0, nr))) for br in brs for _ in range(16)]
    nr, nc, r, c, v = coo(nr, nr, cells, 4)
    check(oracle, bmsp, nr, nc, r, c, v)


def test_row_span_forces_fallback(oracle, bmsp, force_chunks):
    # one value per 64 rows: 512 values span 32 K rows, far beyond the 1024-row window -> the value-stream kernel
    nr = 200000
    cells = [(64 * i, (7919 * i) % nr) for i in range(nr // 64)]
    nr, nc, r, c, v = coo(nr, nr, cells, 5)
    check(oracle, bmsp, nr, nc, r, c, v, kernel="spmv_vstream_kernel")


def test_ragged_rows_and_wide_columns(oracle, bmsp, force_chunks):
    nr, nc = 5003, 9001  # num_rows % 8 != 0; more columns than rows, ragged last block column
    cells = np.concatenate([random_cells(nr, nc, 9000, 6), [[nr - 1, nc - 1], [nr - 2, nc - 2], [0, nc - 1]]])
    nr, nc, r, c, v = coo(nr, nc, cells, 6)
    check(oracle, bmsp, nr, nc, r, c, v)


def test_row_panel_view(bmsp, force_chunks):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(13, 4)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    assert bmsp.spmv_launch_info(A)["kernel"] == CHUNK
    nbr = (n + 7) // 8
    lo, hi = nbr // 3, 2 * nbr // 3
    M, sel = A.row_panel(lo, hi), slice(lo * 8, hi * 8)
    assert bmsp.spmv_launch_info(M)["kernel"].startswith("spmv_vstream_kernel")  # views take the value-stream kernel
    x = gen.spmv_x(n, "cusp")
    S = util.scipy_csr(n, n, r, c, np.asarray(v, np.float32).astype(np.float64))
    want, mag = (S @ x.astype(np.float64))[sel], (abs(S) @ np.abs(x.astype(np.float64)))[sel]
    dx = bmsp.DeviceArray.from_host(x)
    y = bmsp.DeviceArray(n, np.float32)
    assert bmsp.lib().bmsp_memset(y.ptr, 0xFF, n * 4) == 0
    bmsp.check(bmsp.lib().bmsp_spmv(M.h, dx.ptr, y.ptr, 0, None))
    got = y.to_host()
    assert np.all(np.abs(got[sel] - want) <= 1e-5 * mag + 1e-30)
    assert np.all(np.abs(sweep(bmsp, A, x, n) - S @ x.astype(np.float64)) <= 2e-5 * (abs(S) @ np.abs(x.astype(np.float64))) + 1e-30)


@pytest.mark.parametrize("dtype", [1, 2])
def test_fp16_fp64_take_the_value_stream_kernel(bmsp, force_chunks, dtype):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(13, 4)
    v = np.round(v * 4) / 4
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, dtype=dtype)
    assert bmsp.spmv_launch_info(A)["kernel"].startswith("spmv_vstream_kernel")
    x = np.ones(n) if dtype == 1 else gen.spmv_x(n, "cusp").astype(np.float64)
    y = sweep(bmsp, A, x.astype({1: np.float16, 2: np.float64}[dtype]), n, {1: np.float32, 2: np.float64}[dtype])
    S = util.scipy_csr(n, n, r, c, v)
    tol = {1: 1e-5, 2: 1e-13}[dtype]
    assert np.all(np.abs(y - S @ x.astype(np.float64)) <= tol * (abs(S) @ np.abs(x.astype(np.float64))) + 1e-30)


def test_value_invalidation_keeps_the_cache_valid(oracle, bmsp, force_chunks):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(14, 3, seed=7)
    A = check(oracle, bmsp, n, n, r, c, v)
    v2 = 1.5 - v
    A2 = bmsp.BmSpMatrix.from_coo(n, n, r, c, v2)
    d, s = A.device_arrays()[3], A2.device_arrays()[3]
    bmsp.check(bmsp.lib().bmsp_memcpy_d2d(d.ptr, s.ptr, d.n * 4))
    A.invalidate()
    assert bmsp.spmv_launch_info(A)["kernel"] == CHUNK
    x = gen.spmv_x(n, "cusp")
    y = sweep(bmsp, A, x, n)
    y_ref = oracle.spmv_f32(oracle.bmsp_from_coo(oracle.Coo(n, n, r, c, v2), 0, False), x)
    S = util.scipy_csr(n, n, r, c, np.asarray(v2, np.float32).astype(np.float64))
    bound = 1e-5 * (abs(S) @ np.abs(x.astype(np.float64))) + 1e-30
    assert np.all(np.abs(y - y_ref) <= bound + 1e-5 * np.abs(y_ref))


def expected_chunk_bytes(A):
    """the chunked layout's compulsory bytes, from the structure alone (mirrors the records the cache build writes)"""
    info = A.info()
    k, b, o, _ = A.host_arrays()
    nnz, n_rows, n_cols = info["nnz"], info["num_rows"], info["num_cols"]
    per_tile = np.diff(o.astype(np.int64))
    br = np.repeat((k >> 32).astype(np.int64), per_tile)  # block-row of every stored value, storage order
    nch = (nnz + V - 1) // V
    fb = br[np.arange(nch) * V]
    lb = br[np.minimum(np.arange(1, nch + 1) * V, nnz) - 1]
    head = np.zeros(nch, bool)
    head[1:] = lb[:-1] == fb[1:]
    tail = np.zeros(nch, bool)
    tail[:-1] = fb[1:] == lb[:-1]
    tail &= ~(head & (fb == lb))
    slots = int(head.sum() + tail.sum())
    return 8 * nnz + 32 * nch + 4 * n_cols + 4 * n_rows + 64 * slots + 8 * int(tail.sum())


def test_launch_info_headline_matrix(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(20, 2)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    del r, c, v
    li = bmsp.spmv_launch_info(A)
    assert li["kernel"] == CHUNK, li
    assert li["compulsory_bytes"] == expected_chunk_bytes(A), li
    y = bmsp.spmv(A, bmsp.DeviceArray.from_host(np.ones(n, np.float32))).to_host()
    vals = A.host_arrays()[3].astype(np.float64)
    assert np.all(np.isfinite(y)) and abs(float(y.sum()) - float(vals.sum())) <= 1e-4 * float(vals.sum())


def test_threshold_keeps_small_matrices(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(14, 2)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    assert bmsp.spmv_launch_info(A)["kernel"].startswith("spmv_vstream_kernel")
