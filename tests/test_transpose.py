"""GPU tests of the device-side transpose and tile-layout conversion (bmsp_matrix_transpose / bmsp_matrix_convert_layout /
bmsp_matrix_copy_values): every output against an independent build of the swapped (or same) COO -- the CPU oracle or the
library's own builder -- bit for bit."""
import ctypes as C
import os
import numpy as np
import pytest
import util
from stream_gate import _hip

pytestmark = pytest.mark.gpu

NPDT = {0: np.float32, 1: np.float16, 2: np.float64}
UINT = {0: np.uint32, 1: np.uint16, 2: np.uint64}
LAYOUTS = [(l1, l0) for l1 in (0, 1) for l0 in (0, 1)]


def swapped(oracle, coo):
    return oracle.Coo(coo.num_cols, coo.num_rows, coo.cols, coo.rows, coo.vals)


def check_exact(got, ref, np_dtype):
    """the four arrays, the shape, the layout and the block-row pointer of `got` against the oracle's build `ref`."""
    i = got.info()
    assert (i["num_rows"], i["num_cols"], i["nnz"], i["block_num"], i["transposed"]) == \
        (ref.num_rows, ref.num_cols, ref.nnz, ref.block_num, ref.transposed)
    util.assert_bmsp_equal_exact(ref, *got.host_arrays(), np_dtype)
    nbr = (ref.num_rows + 7) // 8
    exp = np.searchsorted((ref.keys >> np.uint64(32)).astype(np.int64), np.arange(nbr + 1), side="left")
    np.testing.assert_array_equal(got.block_row_ptr(), exp.astype(np.uint32))


def assert_same_arrays(a, b):
    assert a.info() == b.info()
    for x, y in zip(a.host_arrays(), b.host_arrays()):
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))


def snapshot(m):
    return [x.copy() for x in m.host_arrays()]


def assert_unchanged(m, snap):
    for x, y in zip(m.host_arrays(), snap):
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))


def check_all_layouts(oracle, bmsp, coo, dtype):
    """transpose and convert_layout from both input layouts into both output layouts, against the oracle's builds."""
    refs_t = {l: oracle.bmsp_from_coo(swapped(oracle, coo), dtype, l) for l in (0, 1)}
    refs_c = {l: oracle.bmsp_from_coo(coo, dtype, l) for l in (0, 1)}
    for lin in (0, 1):
        A = bmsp.BmSpMatrix.from_coo(coo.num_rows, coo.num_cols, coo.rows, coo.cols, coo.vals, transposed=lin, dtype=dtype)
        snap = snapshot(A)
        for lout in (0, 1):
            check_exact(A.transpose(lout), refs_t[lout], NPDT[dtype])
            check_exact(A.with_layout(lout), refs_c[lout], NPDT[dtype])
        assert_unchanged(A, snap)


# ---------------------------------------------------------------------------------------------------------
# 1. fixtures
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", util.all_fixture_mtx())
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_fixtures_match_builder_of_swapped_coo(oracle, bmsp, path, dtype):
    coo = oracle.mtx_read(path)
    refs_t = {l: oracle.bmsp_from_coo(swapped(oracle, coo), dtype, l) for l in (0, 1)}
    refs_c = {l: oracle.bmsp_from_coo(coo, dtype, l) for l in (0, 1)}
    for lin in (0, 1):
        A = bmsp.BmSpMatrix.from_mtx(path, transposed=lin, dtype=dtype)
        snap = snapshot(A)
        for lout in (0, 1):
            check_exact(A.transpose(lout), refs_t[lout], NPDT[dtype])
            check_exact(A.with_layout(lout), refs_c[lout], NPDT[dtype])
        assert_unchanged(A, snap)


# ---------------------------------------------------------------------------------------------------------
# 2. shapes
# ---------------------------------------------------------------------------------------------------------
def _shape_cases():
    from pybmsp import gen
    rng = np.random.default_rng(7)
    cases = {"empty": (37, 11, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))}
    cases["1x1"] = (1, 1, np.array([0]), np.array([0]), np.array([2.5]))
    for nr, nc, nnz in ((13, 1000, 3000), (1000, 13, 3000), (37, 29, 300), (203, 77, 4000)):
        _, _, r, c, v = gen.random_coo(nr, nc, nnz, seed=nr + nc)
        cases["%dx%d" % (nr, nc)] = (nr, nc, r, c, v)
    rr, cc = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    cases["full_tile"] = (8, 8, rr.ravel(), cc.ravel(), rng.uniform(-1, 1, 64))
    rr, cc = np.meshgrid(np.arange(21), np.arange(19), indexing="ij")
    cases["dense_21x19"] = (21, 19, rr.ravel(), cc.ravel(), rng.uniform(-1, 1, 21 * 19))
    # one block column holding 9000 tiles (A^T: one block-row of 9000 tiles), plus a scatter elsewhere
    nr = 9000 * 8 + 5
    r1 = np.arange(0, nr, 8)[:9000] + rng.integers(0, 8, 9000)
    c1 = rng.integers(0, 8, 9000)
    _, _, r2, c2, _ = gen.random_coo(nr, 300, 5000, seed=3)
    rc = np.unique(np.concatenate([r1.astype(np.int64) * 300 + c1, r2.astype(np.int64) * 300 + c2]))
    cases["long_column"] = (nr, 300, rc // 300, rc % 300, rng.uniform(-1, 1, rc.size))
    n, _, r, c, v = gen.rmat(14, 4)
    cases["rmat14"] = (n, n, r, c, v)
    n, _, r, c, v = gen.cage_like(3000)
    cases["cage_like"] = (n, n, r, c, v)
    _, _, r, c, v = gen.random_coo(300, 1700, 6000, seed=5)
    cases["random_300x1700"] = (300, 1700, r, c, v)
    _, _, r, c, v = gen.random_coo(1700, 300, 6000, seed=6)
    cases["random_1700x300"] = (1700, 300, r, c, v)
    return cases


_SHAPES = _shape_cases()


@pytest.mark.parametrize("name", sorted(_SHAPES))
def test_shapes_match_builder_of_swapped_coo(oracle, bmsp, name):
    nr, nc, r, c, v = _SHAPES[name]
    coo = oracle.Coo(nr, nc, r, c, v)
    for dtype in ((0, 1, 2) if coo.nnz < 50000 else (0, 1)):
        check_all_layouts(oracle, bmsp, coo, dtype)


# ---------------------------------------------------------------------------------------------------------
# 3. involution
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dtype", [("rmat", 0), ("fem", 1), ("rect", 2)])
def test_transpose_twice_is_identity(bmsp, kind, dtype):
    from pybmsp import gen
    if kind == "rmat":
        n, _, r, c, v = gen.rmat(12, 6)
        nr = nc = n
    elif kind == "fem":
        n, _, r, c, v = gen.fem_like(10, "27pt")
        nr = nc = n
    else:
        nr, nc = 333, 1210
        _, _, r, c, v = gen.random_coo(nr, nc, 20000, seed=9)
    for l1, l0 in LAYOUTS:
        A = bmsp.BmSpMatrix.from_coo(nr, nc, r, c, v, transposed=l0, dtype=dtype)
        T = A.transpose(l1)
        assert (T.num_rows, T.num_cols) == (nc, nr)
        assert_same_arrays(T.transpose(l0), A)


# ---------------------------------------------------------------------------------------------------------
# 4. raw bits
# ---------------------------------------------------------------------------------------------------------
def entries(keys, bmps, offsets, transposed):
    """(row, col, value index) of every stored entry, from the format definition (util.bmsp_host_to_dok's mapping)."""
    keys, bmps, offsets = (np.asarray(a, np.uint64) for a in (keys, bmps, offsets))
    p = np.arange(64, dtype=np.uint64)
    has = ((bmps[:, None] >> (np.uint64(63) - p)) & np.uint64(1)).astype(bool)
    rank = np.cumsum(has, axis=1) - 1
    b, pos = np.nonzero(has)
    idx = offsets[b].astype(np.int64) + rank[b, pos]
    hi, lo = pos // 8, pos % 8
    brow = (keys[b] >> np.uint64(32)).astype(np.int64)
    bcol = (keys[b] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    if transposed:
        return brow * 8 + lo, bcol * 8 + hi, idx
    return brow * 8 + hi, bcol * 8 + lo, idx


def special_bits(dtype, n, rng):
    """n values of raw bits with -0, +-Inf, NaNs with payloads and subnormals mixed into ordinary numbers."""
    u = UINT[dtype]
    bits = rng.standard_normal(n).astype(NPDT[dtype]).view(u).copy()
    w = np.dtype(u).itemsize * 8
    man = {16: 10, 32: 23, 64: 52}[w]
    sign = u(1) << u(w - 1)
    expo = ((u(1) << u(w - 1 - man)) - u(1)) << u(man)
    specials = [sign, expo, sign | expo, expo | u(1), expo | u(5), sign | expo | (u(1) << u(man - 1)) | u(3), u(1), sign | u(7),
                (u(1) << u(man)) - u(1)]
    for k, s in enumerate(specials):
        bits[k::len(specials) * 3] = s
    return bits


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_values_move_as_raw_bits(bmsp, dtype):
    from pybmsp import gen
    rng = np.random.default_rng(dtype)
    nr, nc = 203, 157
    _, _, r, c, v = gen.random_coo(nr, nc, 9000, seed=11)
    for lin in (0, 1):
        A = bmsp.BmSpMatrix.from_coo(nr, nc, r, c, v, transposed=lin, dtype=dtype)
        bits = special_bits(dtype, A.nnz, rng)
        k, b, o, vals = A.device_arrays()
        bmsp.check(bmsp.lib().bmsp_memcpy_h2d(vals.ptr, bits.ctypes.data, bits.nbytes))
        A.invalidate(False)
        ka, ba, oa, va = A.host_arrays()
        np.testing.assert_array_equal(va.view(UINT[dtype]), bits)
        ra, ca, ia = entries(ka, ba, oa, lin)
        lookup = np.argsort(ra * nc + ca)
        for lout in (0, 1):
            for swap in (True, False):
                T = A.transpose(lout) if swap else A.with_layout(lout)
                kt, bt, ot, vt = T.host_arrays()
                rt, ct, it = entries(kt, bt, ot, lout)
                sr, sc = (ct, rt) if swap else (rt, ct)
                src = ia[lookup[np.searchsorted(ra * nc + ca, sr * nc + sc, sorter=lookup)]]
                want = np.empty_like(bits)
                want[it] = bits[src]
                assert vt.size == bits.size
                np.testing.assert_array_equal(vt.view(UINT[dtype]), want)


# ---------------------------------------------------------------------------------------------------------
# 5. full size
# ---------------------------------------------------------------------------------------------------------
def test_headline_rmat_transpose_and_spmv(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(20, 2)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    At = A.transpose(0)
    ref = bmsp.BmSpMatrix.from_coo(n, n, c, r, v)
    assert_same_arrays(At, ref)
    del ref
    x = gen.spmv_x(n, "cusp")
    S = util.scipy_csr(n, n, c, r, np.asarray(v, np.float32).astype(np.float64))  # A^T
    y64 = S @ x.astype(np.float64)
    bound = 1e-5 * (abs(S) @ np.abs(x.astype(np.float64))) + 1e-30
    dx = bmsp.DeviceArray.from_host(x)
    du = bmsp.DeviceArray(n, np.float32)
    assert bmsp.lib().bmsp_memset(du.ptr, 0xFF, n * 4) == 0
    bmsp.spmv(At, dx, du)
    y = du.to_host()
    assert np.all(np.isfinite(y))
    assert np.all(np.abs(y - y64) <= bound), float(np.max(np.abs(y - y64) - bound))


# ---------------------------------------------------------------------------------------------------------
# 6. SpGEMM on transformed operands
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fem", "rmat"])
@pytest.mark.parametrize("dtype,tc", [(0, 5), (1, 4)])
def test_spgemm_on_transposed_operands(bmsp, kind, dtype, tc):
    from pybmsp import gen
    n, _, r, c, v = gen.fem_like(12, "27pt") if kind == "fem" else gen.rmat(12, 6)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, dtype=dtype)
    built = lambda rows, cols, lay: bmsp.BmSpMatrix.from_coo(n, n, rows, cols, v, transposed=lay, dtype=dtype)
    # A * A^T
    B = A.transpose(1)
    assert_same_arrays(B, built(c, r, 1))
    C1, _ = bmsp.spgemm(A, B, tc_version=tc)
    C2, _ = bmsp.spgemm(built(r, c, 0), built(c, r, 1), tc_version=tc)
    assert_same_arrays(C1, C2)
    # A^T * A
    L = A.transpose(0)
    R = L.transpose(1)
    assert_same_arrays(L, built(c, r, 0))
    assert_same_arrays(R, built(r, c, 1))
    C1, _ = bmsp.spgemm(L, R, tc_version=tc)
    C2, _ = bmsp.spgemm(built(c, r, 0), built(r, c, 1), tc_version=tc)
    assert_same_arrays(C1, C2)


# ---------------------------------------------------------------------------------------------------------
# 7. copy_values
# ---------------------------------------------------------------------------------------------------------
def _write_values(bmsp, M, host_vals):
    vals = M.device_arrays()[3]
    h = np.ascontiguousarray(host_vals, dtype=vals.dtype)
    assert h.size == vals.n
    bmsp.check(bmsp.lib().bmsp_memcpy_h2d(vals.ptr, h.ctypes.data, h.nbytes))


@pytest.mark.parametrize("dtype", [0, 1])
def test_copy_values_follows_new_values(bmsp, dtype):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(12, 6) if dtype == 0 else gen.fem_like(10, "27pt")
    v2 = np.random.default_rng(3).uniform(0.5, 2.0, v.size)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, dtype=dtype)
    outs = {(True, 0): A.transpose(0), (True, 1): A.transpose(1), (False, 1): A.with_layout(1), (False, 0): A.with_layout(0)}
    x = gen.spmv_x(n, "cusp")
    dx = bmsp.DeviceArray.from_host(x.astype(NPDT[dtype]))
    y_old = bmsp.spmv(outs[(True, 0)], dx).to_host()
    outs[(True, 1)].prepare(2)  # holds value-derived caches: copy_values must drop them
    # new values in A's own array (A2 has A's structure)
    A2 = bmsp.BmSpMatrix.from_coo(n, n, r, c, v2, dtype=dtype)
    assert_same_arrays(A2.with_layout(0), A2)
    _write_values(bmsp, A, A2.host_arrays()[3])
    A.invalidate(False)
    for (swap, lay), M in outs.items():
        M.copy_values_from(A)
        rows, cols = (c, r) if swap else (r, c)
        assert_same_arrays(M, bmsp.BmSpMatrix.from_coo(n, n, rows, cols, v2, transposed=lay, dtype=dtype))
    # the SpMV of A^T sees the new values
    y = bmsp.spmv(outs[(True, 0)], dx).to_host()
    S = util.scipy_csr(n, n, c, r, np.asarray(v2, NPDT[dtype]).astype(np.float64))
    xd = x.astype(NPDT[dtype]).astype(np.float64)
    tol = 1e-5 if dtype == 0 else 2e-3
    assert np.all(np.abs(y - S @ xd) <= tol * (abs(S) @ np.abs(xd)) + 1e-30)
    assert not np.array_equal(y, y_old)
    # the product with the refreshed right operand sees them too
    B = outs[(True, 1)]
    tc = 5 if dtype == 0 else 4
    C1, _ = bmsp.spgemm(A, B, tc_version=tc)
    C2, _ = bmsp.spgemm(A2, bmsp.BmSpMatrix.from_coo(n, n, c, r, v2, transposed=1, dtype=dtype), tc_version=tc)
    assert_same_arrays(C1, C2)


def test_copy_values_refuses_foreign_or_stale_sources(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(10, 4)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    At = A.transpose(0)
    At.copy_values_from(A)  # paired: fine
    other = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)  # same structure, another matrix
    fresh = bmsp.BmSpMatrix.from_coo(n, n, c, r, v)  # made by the builder, not by a transpose
    for dst, src in ((At, other), (fresh, A), (A, A)):
        with pytest.raises(bmsp.BmspError) as e:
            dst.copy_values_from(src)
        assert e.value.status == -1 and "copy_values" in str(e.value)
    A.invalidate(True)  # A's structure is declared changed: the record no longer applies
    with pytest.raises(bmsp.BmspError) as e:
        At.copy_values_from(A)
    assert e.value.status == -1
    # the output's own structure declared changed: it forgets its source
    B = A.transpose(1)
    B.invalidate(True)
    with pytest.raises(bmsp.BmspError) as e:
        B.copy_values_from(A)
    assert e.value.status == -1


# ---------------------------------------------------------------------------------------------------------
# 8. hygiene
# ---------------------------------------------------------------------------------------------------------
def test_row_panel_views_are_refused(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(10, 4)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    V = A.row_panel(3, 9)
    for op in (lambda: V.transpose(0), lambda: V.transpose(1), lambda: V.with_layout(1)):
        with pytest.raises(bmsp.BmspError) as e:
            op()
        assert e.value.status == -1 and "view" in str(e.value)


def test_non_default_stream(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(13, 6)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, dtype=2)
    H = _hip()
    s = C.c_void_p()
    assert H.hipStreamCreate(C.byref(s)) == 0
    try:
        T0, T1, L1 = A.transpose(0, stream=s.value), A.transpose(1, stream=s.value), A.with_layout(1, stream=s.value)
        assert H.hipStreamSynchronize(s) == 0
        assert_same_arrays(T0, A.transpose(0))
        assert_same_arrays(T1, A.transpose(1))
        assert_same_arrays(L1, A.with_layout(1))
        v2 = np.random.default_rng(5).uniform(-1, 1, v.size)
        _write_values(bmsp, A, bmsp.BmSpMatrix.from_coo(n, n, r, c, v2, dtype=2).host_arrays()[3])
        A.invalidate(False)
        for M in (T0, T1, L1):
            M.copy_values_from(A, stream=s.value)
        assert H.hipStreamSynchronize(s) == 0
        assert_same_arrays(T0, bmsp.BmSpMatrix.from_coo(n, n, c, r, v2, dtype=2))
        assert_same_arrays(T1, bmsp.BmSpMatrix.from_coo(n, n, c, r, v2, transposed=1, dtype=2))
        assert_same_arrays(L1, bmsp.BmSpMatrix.from_coo(n, n, r, c, v2, transposed=1, dtype=2))
    finally:
        H.hipStreamDestroy(s)


def test_cpp_wrappers_run(bmsp, tmp_path):
    """tests/cpp_transpose_check.cpp: bmSpMatrix<T>::transpose / with_layout on the data/real fixture, as the reference's user would."""
    import subprocess
    from conftest import REPO, MTX
    from test_transpose_api import build_cpp_transpose_check
    exe = str(tmp_path / "cpp_transpose_check")
    build_cpp_transpose_check(exe)
    out = subprocess.run([exe, os.path.join(MTX, "real", "A_matrix.mtx")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "CHECK transpose OK" in out.stdout and "CHECK with_layout OK" in out.stdout, out.stdout


@pytest.mark.parametrize("lanes", ["1", "8"])
def test_both_lane_groups_of_the_value_move(oracle, bmsp, monkeypatch, lanes):
    """the value move's two work shapes (a lane per tile, eight lanes per tile) forced on sparse and on full tiles"""
    from pybmsp import gen
    monkeypatch.setenv("BMSP_TRANSPOSE_LANES", lanes)
    for nr, nc, r, c, v in (gen.banded(200, 9), gen.rmat(11, 4)):
        check_all_layouts(oracle, bmsp, oracle.Coo(nr, nc, r, c, v), 1)
    n, _, r, c, v = gen.banded(300, 12)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, dtype=2)
    outs = [(A.transpose(0), c, r, 0), (A.transpose(1), c, r, 1), (A.with_layout(1), r, c, 1)]
    v2 = v * -3.0
    _write_values(bmsp, A, bmsp.BmSpMatrix.from_coo(n, n, r, c, v2, dtype=2).host_arrays()[3])
    A.invalidate(False)
    for M, rows, cols, lay in outs:
        M.copy_values_from(A)
        assert_same_arrays(M, bmsp.BmSpMatrix.from_coo(n, n, rows, cols, v2, transposed=lay, dtype=2))
