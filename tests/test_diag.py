"""GPU tests of the diagonal operations (bmsp_matrix_diagonal / _from_diagonal / _scale / _scale_values).  The expected values of every
case come from numpy on what the test reads back from the device: np.float32 / np.float64 arithmetic in the stated order (left factor,
then right, each operation rounded on its own) and .astype(np.float16) for F16.  Structures come from the CPU oracle's build of the COO in
the output layout.  Comparison is bit for bit (a NaN only has to be a NaN); A must come back unchanged from every out-of-place call."""
import ctypes as C
import os
import numpy as np
import pytest
from stream_gate import _hip
from test_transpose import entries, assert_same_arrays, snapshot, assert_unchanged, _write_values
from test_add import stored, check_structure, assert_same_values

pytestmark = pytest.mark.gpu

NPDT = {0: np.float32, 1: np.float16, 2: np.float64}
OUTDT = {0: np.float32, 1: np.float32, 2: np.float64}
UINT = {0: np.uint32, 1: np.uint16, 2: np.uint64}
VALID = [(False, False, 0), (True, False, 0), (True, False, 1), (False, True, 0), (False, True, 2), (True, True, 0), (True, True, 1),
         (True, True, 2), (True, True, 3)]  # (left given, right given, flags): a DIV flag needs its vector


def build(bmsp, nr, nc, r, c, v, lay, dtype):
    return bmsp.BmSpMatrix.from_coo(nr, nc, r, c, v, transposed=lay, dtype=dtype)


def factors(n, dtype, seed):
    """n factors of the vector type with magnitudes in [0.5, 2) and mixed signs"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(OUTDT[dtype])


def scale_ref(v, r, c, l, rt, flags, dtype):
    """the contract in numpy: v the stored values (storage dtype) at rows r / columns c; l, rt host vectors or None"""
    if l is None and rt is None:
        return v.copy()
    x = v.astype(OUTDT[dtype])
    with np.errstate(all="ignore"):
        if l is not None:
            x = x / l[r] if flags & 1 else x * l[r]
        if rt is not None:
            x = x / rt[c] if flags & 2 else x * rt[c]
        assert x.dtype == OUTDT[dtype]
        return x.astype(NPDT[dtype])


def dev(bmsp, h):
    return None if h is None else bmsp.DeviceArray.from_host(h)


class Converted:
    """A.with_layout(lout) and what the checks read from it, fetched once: its host arrays, block-row pointer and entry coordinates"""

    def __init__(self, A, lout):
        self.M = A.with_layout(lout)
        self.info = self.M.info()
        self.k, self.b, self.o, self.v = self.M.host_arrays()
        self.ptr = self.M.block_row_ptr()
        self.rows, self.cols, self.idx = entries(self.k, self.b, self.o, lout)


def check_scale(oracle, bmsp, A, l, rt, flags, lout, W=None, snap=None):
    """scale(A) into layout lout against numpy on the values of W = A.with_layout(lout) (made when None), W's structure; A unchanged."""
    dtype = A.dtype
    snap = snap or snapshot(A)
    S = bmsp.scale(A, dev(bmsp, l), dev(bmsp, rt), bool(flags & 1), bool(flags & 2), transposed=lout)
    assert_unchanged(A, snap)
    W = W or Converted(A, lout)
    assert S.info() == W.info
    sk, sb, so, sv = S.host_arrays()
    for x, y in ((sk, W.k), (sb, W.b), (so, W.o)):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(S.block_row_ptr(), W.ptr)
    assert_same_values(sv[W.idx], scale_ref(W.v[W.idx], W.rows, W.cols, l, rt, flags, dtype), dtype)
    return S


def oracle_structure(oracle, A, lay):
    r, c, v = stored(A)
    return oracle.bmsp_from_coo(oracle.Coo(A.num_rows, A.num_cols, r, c, np.nan_to_num(v.astype(np.float64))), A.dtype, lay)


# ---------------------------------------------------------------------------------------------------------
# 1. dtypes x layouts x flags x sides x lane groups
# ---------------------------------------------------------------------------------------------------------
def _matrices():
    from pybmsp import gen
    return {"random": gen.random_coo(203, 157, 203 * 26, seed=3), "banded": gen.banded(400, 12), "rmat_hubs": gen.rmat(14, 8)}


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("kind", ["random", "banded", "rmat_hubs"])
def test_scale_all_layouts_flags_sides_and_lane_groups(oracle, bmsp, dtype, kind, monkeypatch):
    nr, nc, r, c, v = _matrices()[kind]
    l, rt = factors(nr, dtype, 11), factors(nc, dtype, 12)
    for lin in (0, 1):
        A = build(bmsp, nr, nc, r, c, v, lin, dtype)
        if kind == "rmat_hubs":
            assert int(np.diff(A.block_row_ptr()).max()) > 1000
        for lout in (0, 1):
            W = Converted(A, lout)
            check_structure(W.M, oracle_structure(oracle, A, lout))
            for has_l, has_r, flags in VALID:
                outs = []
                for g in ("1", "8"):
                    monkeypatch.setenv("BMSP_SCALE_LANES", g)
                    outs.append(check_scale(oracle, bmsp, A, l if has_l else None, rt if has_r else None, flags, lout, W))
                assert_same_arrays(outs[0], outs[1])
                if not has_l and not has_r:
                    assert_same_arrays(outs[0], W.M)  # both sides NULL: the layout conversion, bit for bit
            monkeypatch.delenv("BMSP_SCALE_LANES")
            check_scale(oracle, bmsp, A, l, rt, 2, lout, W)  # the library's own choice of lane group
    # a DIV flag without its vector is refused on a real handle too
    for has_l, has_r, flags in ((False, True, 1), (True, False, 2), (False, False, 3)):
        with pytest.raises(bmsp.BmspError) as e:
            bmsp.scale(A, dev(bmsp, l) if has_l else None, dev(bmsp, rt) if has_r else None, bool(flags & 1), bool(flags & 2))
        assert e.value.status == -1 and "null" in str(e.value)


# ---------------------------------------------------------------------------------------------------------
# 2. special values
# ---------------------------------------------------------------------------------------------------------
def _pool(T):
    fi = np.finfo(T)
    sub_lo, sub_hi = fi.smallest_subnormal, np.nextafter(fi.tiny, T(0))
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, sub_lo, -sub_lo, sub_hi, -sub_hi, fi.tiny, -fi.tiny, fi.max, -fi.max, 1.0, -1.0, 0.5,
                     2.0, 3.0], dtype=T)


def _mixed(T, n, rng):
    pool = _pool(T)
    vals = rng.uniform(-2, 2, n).astype(T)
    pick = rng.random(n) < 0.6
    vals[pick] = pool[rng.integers(0, pool.size, int(pick.sum()))]
    vals[:pool.size] = pool
    return vals


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_special_values_follow_ieee(oracle, bmsp, dtype, monkeypatch):
    from pybmsp import gen
    rng = np.random.default_rng(70 + dtype)
    nr, nc = 64, 72
    _, _, r, c, v = gen.random_coo(nr, nc, 1500, seed=9)
    for lin in (0, 1):
        A = build(bmsp, nr, nc, r, c, v, lin, dtype)
        _write_values(bmsp, A, _mixed(NPDT[dtype], A.nnz, rng))
        A.invalidate(False)
        l, rt = _mixed(OUTDT[dtype], nr, rng), _mixed(OUTDT[dtype], nc, rng)
        for lout in (0, 1):
            W = Converted(A, lout)
            for g in ("1", "8"):
                monkeypatch.setenv("BMSP_SCALE_LANES", g)
                for has_l, has_r, flags in VALID:
                    S = check_scale(oracle, bmsp, A, l if has_l else None, rt if has_r else None, flags, lout, W)
                    if not has_l and not has_r:
                        assert_same_arrays(S, W.M)  # raw bits: -0, NaN payloads, subnormals


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_named_special_outcomes(bmsp, dtype, monkeypatch):
    """one entry per row of a 16 x 16 matrix, the left factor of the row chosen for a named IEEE outcome; the right factor is 1"""
    T, R = NPDT[dtype], OUTDT[dtype]
    fi = np.finfo(T)
    big = T(60000.0) if dtype == 1 else fi.max
    mul = [(fi.tiny, 0.5), (fi.smallest_subnormal, 1.0), (big, 2.0), (0.0, np.inf), (-0.0, 1.0), (np.nextafter(fi.tiny, T(0)), -1.0), (3.0, 0.0),
           (-3.0, 0.0)]
    div = [(1.0, 0.0), (-1.0, 0.0), (1.0, -0.0), (0.0, 0.0), (fi.tiny, 2.0), (np.inf, np.inf), (-0.0, 1.0), (fi.smallest_subnormal, 1.0)]
    n = 16
    rows = np.arange(n)
    cols = (3 * rows + 1) % n
    for lin in (0, 1):
        A = build(bmsp, n, n, rows, cols, np.ones(n), lin, dtype)
        rr, cc, idx = entries(*A.host_arrays()[:3], lin)
        a = np.array([x for x, _ in mul + div], dtype=T)
        hv = np.empty(n, T)
        hv[idx] = a[rr]
        _write_values(bmsp, A, hv)
        A.invalidate(False)
        l = np.array([x for _, x in mul + div], dtype=R)
        ones = np.ones(n, R)
        for lout in (0, 1):
            for g in ("1", "8"):
                monkeypatch.setenv("BMSP_SCALE_LANES", g)
                M = bmsp.scale(A, dev(bmsp, l), dev(bmsp, ones), transposed=lout)
                D = bmsp.scale(A, dev(bmsp, l), dev(bmsp, ones), div_left=True, div_right=True, transposed=lout)
                N = bmsp.scale(A, None, None, transposed=lout)
                mr, _, mv = stored(M)
                dr, _, dv = stored(D)
                m, d = mv[np.argsort(mr)], dv[np.argsort(dr)][8:]
                bits = lambda x: np.array([x], T).view(UINT[dtype])[0]
                # a subnormal result is present and not flushed
                assert m[0] == T(fi.tiny) * T(0.5) and 0 < float(m[0]) < float(fi.tiny)
                assert bits(m[1]) == bits(fi.smallest_subnormal)
                assert float(m[5]) == -float(np.nextafter(fi.tiny, T(0)))
                assert float(d[4]) == float(fi.tiny) / 2 and float(d[4]) > 0 and bits(d[7]) == bits(fi.smallest_subnormal)
                # overflow to Inf (fp16: 60000 * 2 = 120000 is finite in the fp32 arithmetic and rounds to Inf in fp16)
                assert np.isposinf(m[2])
                # 0 * Inf and 0 / 0 and Inf / Inf are NaN; x / 0 is +-Inf with the sign of x and of the zero
                assert np.isnan(m[3]) and np.isnan(d[3]) and np.isnan(d[5])
                assert np.isposinf(d[0]) and np.isneginf(d[1]) and np.isneginf(d[2])
                # -0 * 1 and -0 / 1 keep the sign; x * 0 is a stored zero with the sign of x
                assert bits(m[4]) == bits(T(-0.0)) and bits(d[6]) == bits(T(-0.0))
                assert bits(m[6]) == bits(T(0.0)) and bits(m[7]) == bits(T(-0.0))
                assert M.nnz == D.nnz == n  # every coordinate is kept, zeros, Inf and NaN included
                # a NULL side leaves -0 and the raw bits untouched
                assert_same_arrays(N, A.with_layout(lout))
                L1 = bmsp.scale(A, dev(bmsp, ones), None, transposed=lout)
                nr_, _, nv = stored(L1)
                assert bits(nv[np.argsort(nr_)][4]) == bits(T(-0.0))


# ---------------------------------------------------------------------------------------------------------
# 3. ragged shapes
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("nr,nc", [(203, 157), (157, 203), (9, 1001), (1001, 9), (13, 13)])
def test_ragged_shapes_do_not_read_past_the_stored_rows_and_columns(oracle, bmsp, dtype, nr, nc, monkeypatch):
    """rows and columns are no multiples of 8; the last rows / columns hold nothing and their factors (and the padding of the vectors up
    to and beyond the tile edge) are NaN: no NaN may reach a value"""
    from pybmsp import gen
    _, _, r, c, v = gen.random_coo(nr, nc, min(nr * nc // 3, 4000), seed=5)
    last_r, last_c = nr - 3, nc - 2
    keep = (r < last_r) & (c < last_c)
    r, c, v = r[keep], c[keep], v[keep]
    l = np.full((nr + 7) // 8 * 8 + 8, np.nan, OUTDT[dtype])
    rt = np.full((nc + 7) // 8 * 8 + 8, np.nan, OUTDT[dtype])
    l[:last_r], rt[:last_c] = factors(last_r, dtype, 21), factors(last_c, dtype, 22)
    for lin in (0, 1):
        A = build(bmsp, nr, nc, r, c, v, lin, dtype)
        for lout in (0, 1):
            W = Converted(A, lout)
            check_structure(W.M, oracle_structure(oracle, A, lout))
            for g in ("1", "8"):
                monkeypatch.setenv("BMSP_SCALE_LANES", g)
                for flags in (0, 3):
                    S = check_scale(oracle, bmsp, A, l, rt, flags, lout, W)
                    assert not np.isnan(S.host_arrays()[3].astype(np.float64)).any()
        d = check_diagonal(bmsp, A)
        assert d.size == min(nr, nc)


# ---------------------------------------------------------------------------------------------------------
# 4. diagonal
# ---------------------------------------------------------------------------------------------------------
def check_diagonal(bmsp, A):
    """diagonal(A) into a NaN-poisoned buffer against numpy on the stored entries; A unchanged"""
    i = A.info()
    dtype, n = i["dtype"], min(i["num_rows"], i["num_cols"])
    R = OUTDT[dtype]
    snap = snapshot(A)
    out = bmsp.DeviceArray(n, R)
    if n:
        assert bmsp.lib().bmsp_memset(out.ptr, 0xFF, n * out.dtype.itemsize) == 0
    bmsp.check(bmsp.lib().bmsp_matrix_diagonal(A.h, out.ptr, None))
    got = out.to_host()
    assert_unchanged(A, snap)
    r, c, v = stored(A)
    on = r == c
    if dtype == 1:
        want = np.zeros(n, np.float32)
        want[r[on]] = v[on].astype(np.float32)  # exact widening
        assert_same_values(got, want, 0)
    else:  # raw bits
        want = np.zeros(n, UINT[dtype])
        want[r[on]] = v[on].view(UINT[dtype])
        np.testing.assert_array_equal(got.view(UINT[dtype]), want)
    np.testing.assert_array_equal(bmsp.diagonal(A).to_host().view(np.uint8), got.view(np.uint8))
    return got


def _with_diagonal(nr, nc, r, c, v, which, seed=1):
    """the COO without its diagonal entries plus the diagonal entries `which` (indices) with random values"""
    off = r != c
    d = np.asarray(which, np.int64)
    dv = np.random.default_rng(seed).uniform(0.5, 2.0, d.size)
    return np.concatenate([r[off], d]), np.concatenate([c[off], d]), np.concatenate([v[off], dv])


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_diagonal_full_partial_empty_and_a_hole_in_the_middle(bmsp, dtype):
    from pybmsp import gen
    n = 203
    _, _, r, c, v = gen.random_coo(n, n, n * 12, seed=6)
    cases = {"full": np.arange(n), "partial": np.arange(n)[::3], "empty": np.zeros(0, np.int64), "last only": np.array([n - 1]),
             "first only": np.array([0])}
    for name, which in cases.items():
        rr, cc, vv = _with_diagonal(n, n, r, c, v, which)
        for lin in (0, 1):
            d = check_diagonal(bmsp, build(bmsp, n, n, rr, cc, vv, lin, dtype))
            assert np.count_nonzero(d) == which.size, name
    # block-row 5 holds no tile at all, block-row 9 holds tiles but not the diagonal one, block-row 11 only the diagonal one
    rr, cc, vv = _with_diagonal(n, n, r, c, v, np.arange(n))
    gone = (rr // 8 == 5) | ((rr // 8 == 9) & (cc // 8 == 9)) | ((rr // 8 == 11) & (cc // 8 != 11))
    rr, cc, vv = rr[~gone], cc[~gone], vv[~gone]
    for lin in (0, 1):
        A = build(bmsp, n, n, rr, cc, vv, lin, dtype)
        ptr = A.block_row_ptr()
        assert ptr[5] == ptr[6] and ptr[11] + 1 == ptr[12]
        d = check_diagonal(bmsp, A)
        assert not d[40:48].any() and not d[72:80].any() and d[88:96].all() and d[:40].all()
    # an empty matrix
    for lin in (0, 1):
        Z = build(bmsp, 37, 21, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), lin, dtype)
        assert not check_diagonal(bmsp, Z).any()


@pytest.mark.parametrize("dtype,lin", [(0, 0), (0, 1), (1, 0), (2, 1)])
def test_diagonal_on_hub_block_rows(bmsp, dtype, lin):
    """R-MAT 2^14 x 8 + I: the first block-rows hold thousands of tiles, the search runs through them"""
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(14, 8)
    A = build(bmsp, n, n, r, c, v, lin, dtype)
    assert int(np.diff(A.block_row_ptr()).max()) > 1000
    assert check_diagonal(bmsp, A).all()
    rr, cc, vv = _with_diagonal(n, n, r, c, v, np.arange(n)[1::5])
    check_diagonal(bmsp, build(bmsp, n, n, rr, cc, vv, lin, dtype))


@pytest.mark.parametrize("dtype", [0, 2])
def test_diagonal_moves_raw_bits(bmsp, dtype):
    T, U = NPDT[dtype], UINT[dtype]
    n = 40
    rows = np.concatenate([np.arange(n), np.arange(n - 1)])
    cols = np.concatenate([np.arange(n), np.arange(1, n)])
    w = np.dtype(U).itemsize * 8
    man = {32: 23, 64: 52}[w]
    expo = ((U(1) << U(w - 1 - man)) - U(1)) << U(man)
    sign = U(1) << U(w - 1)
    specials = np.array([sign, expo | U(1) << U(man - 1) | U(0x155), sign | expo | U(1) << U(man - 1) | U(3), U(1), sign | U(7), expo,
                         sign | expo, (U(1) << U(man)) - U(1)], U)  # -0, quiet NaNs with payloads, subnormals, +-Inf
    for lin in (0, 1):
        A = build(bmsp, n, n, rows, cols, np.ones(rows.size), lin, dtype)
        rr, cc, idx = entries(*A.host_arrays()[:3], lin)
        hv = np.ones(A.nnz, T)
        bits = hv.view(U)
        on = rr == cc
        bits[idx[on]] = specials[rr[on] % specials.size]
        _write_values(bmsp, A, hv)
        A.invalidate(False)
        out = bmsp.diagonal(A).to_host()
        np.testing.assert_array_equal(out.view(U), specials[np.arange(n) % specials.size])
        check_diagonal(bmsp, A)


# ---------------------------------------------------------------------------------------------------------
# 5. from_diagonal
# ---------------------------------------------------------------------------------------------------------
def _diag_values(dtype, n, seed):
    R = OUTDT[dtype]
    rng = np.random.default_rng(seed)
    d = rng.uniform(-2, 2, n).astype(R)
    pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, np.finfo(R).smallest_subnormal, np.finfo(R).tiny, 1e-9, 70000.0, 65520.0, 1.0 / 3.0,
                     6.1e-5, 5.96e-8, 2.9e-8], R)  # (the last ones round to fp16 Inf / subnormals / 0)
    k = min(n, pool.size)
    d[:k] = pool[:k]
    return d


def check_from_diagonal(bmsp, d, nr, nc, dtype, lay):
    n = min(nr, nc)
    D = bmsp.from_diagonal(bmsp.DeviceArray.from_host(d), nr, nc, dtype=dtype, transposed=lay)
    i = np.arange(n, dtype=np.int32)
    ref = bmsp.BmSpMatrix.from_coo(nr, nc, i, i, d[:n].astype(np.float64), transposed=lay, dtype=dtype)
    assert_same_arrays(D, ref)
    np.testing.assert_array_equal(D.block_row_ptr(), ref.block_row_ptr())
    info = D.info()
    assert (info["nnz"], info["block_num"]) == (n, (n + 7) // 8)
    return D


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_from_diagonal_equals_the_builder(bmsp, dtype):
    for lay in (0, 1):
        for n in (0, 1, 7, 8, 9, 203):
            D = check_from_diagonal(bmsp, _diag_values(dtype, n, 30 + n), n, n, dtype, lay)
            if n == 0:
                assert D.host_arrays()[2].tolist() == [0]
        for nr, nc in ((5, 203), (203, 5), (0, 9), (9, 0), (64, 65), (65, 64), (17, 16)):
            D = check_from_diagonal(bmsp, _diag_values(dtype, max(nr, nc), 3), nr, nc, dtype, lay)
            assert (D.num_rows, D.num_cols) == (nr, nc)
    # the default shape is d.n x d.n, the method form is the function
    d = _diag_values(dtype, 12, 1)
    assert_same_arrays(bmsp.BmSpMatrix.from_diagonal(bmsp.DeviceArray.from_host(d), dtype=dtype),
                       check_from_diagonal(bmsp, d, 12, 12, dtype, 0))
    with pytest.raises(ValueError):
        bmsp.from_diagonal(bmsp.DeviceArray.from_host(d), 13, 13, dtype=dtype)


@pytest.mark.parametrize("dtype", [0, 2])
def test_diagonal_of_from_diagonal_is_the_vector(bmsp, dtype):
    for lay in (0, 1):
        for nr, nc in ((203, 203), (9, 40), (40, 9), (1, 1)):
            d = _diag_values(dtype, min(nr, nc), 44)
            D = bmsp.from_diagonal(bmsp.DeviceArray.from_host(d), nr, nc, dtype=dtype, transposed=lay)
            np.testing.assert_array_equal(bmsp.diagonal(D).to_host().view(UINT[dtype]), d.view(UINT[dtype]))


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_from_diagonal_is_an_operand_of_add(bmsp, dtype):
    """diag(d) - A equals the sum of the same two matrices built from COO"""
    from pybmsp import gen
    nr, nc = 203, 157
    _, _, r, c, v = gen.random_coo(nr, nc, 4000, seed=7)
    d = factors(min(nr, nc), dtype, 8)
    i = np.arange(d.size, dtype=np.int32)
    for la, ld, lc in ((0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
        A = build(bmsp, nr, nc, r, c, v, la, dtype)
        D = bmsp.from_diagonal(bmsp.DeviceArray.from_host(d), nr, nc, dtype=dtype, transposed=ld)
        Dref = build(bmsp, nr, nc, i, i, d.astype(np.float64), ld, dtype)
        assert_same_arrays(bmsp.add(D, A, 1.0, -1.0, transposed=lc), bmsp.add(Dref, A, 1.0, -1.0, transposed=lc))


# ---------------------------------------------------------------------------------------------------------
# 6. against the product
# ---------------------------------------------------------------------------------------------------------
def test_scale_equals_the_product_with_a_diagonal_matrix(bmsp):
    """fp32, V15 numerics: a product with a diagonal matrix has one term per entry, 0 + fl(l * a) = fl(l * a) for finite non-zero values
    that do not underflow"""
    from pybmsp import gen
    nr, nc = 203, 157
    _, _, r, c, v = gen.random_coo(nr, nc, 5000, seed=13)
    v = np.where(v < 0, v - 0.25, v + 0.25)
    l, rt = factors(nr, 0, 14), factors(nc, 0, 15)
    A = build(bmsp, nr, nc, r, c, v, 0, 0)
    Dl = bmsp.from_diagonal(bmsp.DeviceArray.from_host(l), dtype=0)
    Dr = bmsp.from_diagonal(bmsp.DeviceArray.from_host(rt), dtype=0, transposed=True)
    P, _ = bmsp.spgemm(Dl, A.with_layout(1), tc_version=5)
    S = bmsp.scale(A, dev(bmsp, l), None)
    for x, y in zip(P.host_arrays(), S.host_arrays()):
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))
    P, _ = bmsp.spgemm(A, Dr, tc_version=5)
    S = bmsp.scale(A, None, dev(bmsp, rt))
    for x, y in zip(P.host_arrays(), S.host_arrays()):
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))


# ---------------------------------------------------------------------------------------------------------
# 7. SpMV identity
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["chunked", "rowgroup"])
def test_spmv_of_the_scaled_matrix(bmsp, kind):
    """values k/64, factors powers of two in [1/8, 8], a small-integer x: scaling by a power of two commutes with every rounding, so
    spmv(scale(A, l, r), x) = l o spmv(A, r o x) bit for bit"""
    from pybmsp import gen
    if kind == "chunked":
        n, _, r, c, v = gen.rmat(17, 2)
    else:
        n, _, r, c, v = gen.banded(1 << 12, 16)
    v = np.round(v * 64) / 64
    rng = np.random.default_rng(17)
    l, rt = (2.0 ** rng.integers(-3, 4, n)).astype(np.float32), (2.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    S = bmsp.scale(A, dev(bmsp, l), dev(bmsp, rt))
    want = "spmv_chunk_kernel" if kind == "chunked" else "spmv_rowgroup_kernel"
    for M in (A, S):
        assert bmsp.spmv_launch_info(M)["kernel"] == want, bmsp.spmv_launch_info(M)
    x = gen.spmv_x(n, "cusp")
    ys, ya = bmsp.DeviceArray(n, np.float32), bmsp.DeviceArray(n, np.float32)
    for y in (ys, ya):
        assert bmsp.lib().bmsp_memset(y.ptr, 0xFF, n * 4) == 0
    hs = bmsp.spmv(S, bmsp.DeviceArray.from_host(x), ys).to_host()
    ha = bmsp.spmv(A, bmsp.DeviceArray.from_host(rt * x), ya).to_host()
    assert np.all(np.isfinite(hs)) and np.any(hs != 0)
    np.testing.assert_array_equal(hs.view(np.uint32), (l * ha).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------
# 8. scale_values
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1])
def test_scale_in_place_equals_out_of_place_and_drops_the_caches(bmsp, dtype):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(12, 6) if dtype == 0 else gen.fem_like(10, "27pt")
    l, rt = factors(n, dtype, 31), factors(n, dtype, 32)
    dl, dr = dev(bmsp, l), dev(bmsp, rt)
    A = build(bmsp, n, n, r, c, v, 0, dtype)
    B = A.with_layout(1)
    x = bmsp.DeviceArray.from_host(gen.spmv_x(n, "cusp").astype(NPDT[dtype]))
    S = bmsp.scale(A, dl, dr, div_right=True)
    A2 = build(bmsp, n, n, r, c, v, 0, dtype)
    A2.prepare(3)  # the SpMV plan and the product's value-derived caches exist before the values change
    bmsp.spmv(A2, x)
    bmsp.spgemm(A2, B, tc_version=5)
    assert A2.scale_(dl, dr, div_right=True) is A2
    assert_same_arrays(A2, S)
    np.testing.assert_array_equal(bmsp.spmv(A2, x).to_host(), bmsp.spmv(S, x).to_host())
    P2, _ = bmsp.spgemm(A2, B, tc_version=5)
    PS, _ = bmsp.spgemm(S, B, tc_version=5)
    assert_same_arrays(P2, PS)
    # and as the right operand
    B2 = A.with_layout(1)
    B2.prepare(2)
    bmsp.spgemm(A, B2, tc_version=5)
    bmsp.scale_values(B2, B2, dl, None, div_left=True)
    P2, _ = bmsp.spgemm(A, B2, tc_version=5)
    PS, _ = bmsp.spgemm(A, bmsp.scale(A, dl, None, div_left=True, transposed=1), tc_version=5)
    assert_same_arrays(P2, PS)


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_scale_values_into_derived_matrices_follows_new_values(bmsp, dtype, monkeypatch):
    from pybmsp import gen
    nr, nc = 203, 157
    _, _, r, c, v = gen.random_coo(nr, nc, 5000, seed=23)
    v2 = np.random.default_rng(24).uniform(0.5, 2.0, v.size)
    l, rt = factors(nr, dtype, 25), factors(nc, dtype, 26)
    dl, dr = dev(bmsp, l), dev(bmsp, rt)
    for lin in (0, 1):
        A = build(bmsp, nr, nc, r, c, v, lin, dtype)
        outs = [bmsp.scale(A, dl, dr, transposed=0), bmsp.scale(A, None, dr, transposed=1), A.with_layout(0), A.with_layout(1)]
        outs[3].prepare(2)
        _write_values(bmsp, A, build(bmsp, nr, nc, r, c, v2, lin, dtype).host_arrays()[3])
        A.invalidate(False)
        for g in ("1", "8"):
            monkeypatch.setenv("BMSP_SCALE_LANES", g)
            for M in outs:
                lay = M.info()["transposed"]
                for kw in (dict(left=dl, right=dr), dict(left=dl, right=dr, div_left=True, div_right=True), dict(left=None, right=dr),
                           dict(left=dl, div_left=True), dict()):
                    assert bmsp.scale_values(M, A, **kw) is M
                    assert_same_arrays(M, bmsp.scale(A, transposed=lay, **kw))
        monkeypatch.delenv("BMSP_SCALE_LANES")
        # copy_values accepts what scale made
        outs[0].copy_values_from(A)
        assert_same_arrays(outs[0], A.with_layout(0))


def test_scale_values_refusals(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(10, 4)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    dl = dev(bmsp, factors(n, 0, 1))

    def refused(fn, word):
        with pytest.raises(bmsp.BmspError) as e:
            fn()
        assert e.value.status == -1 and word in str(e.value), str(e.value)

    S = bmsp.scale(A, dl, None)
    bmsp.scale_values(S, A, dl, None)
    refused(lambda: bmsp.scale_values(A.clone(), A, dl, None), "out")           # an unrelated handle of the same structure
    refused(lambda: bmsp.scale_values(bmsp.BmSpMatrix.from_coo(n, n, r, c, v), A, dl, None), "out")
    refused(lambda: bmsp.scale_values(A.transpose(0), A, dl, None), "out")      # a transpose has its own tile order
    refused(lambda: bmsp.scale_values(A.transpose(1), A, dl, None), "out")
    refused(lambda: bmsp.scale_values(A, S, dl, None), "out")                   # the roles swapped
    snap = snapshot(S)
    A.invalidate(True)
    refused(lambda: bmsp.scale_values(S, A, dl, None), "out")                   # A's structure may have changed
    refused(lambda: S.copy_values_from(A), "structure")
    assert_unchanged(S, snap)
    A.scale_(dl, None)                                                          # in place needs no history
    L = bmsp.lib()
    assert L.bmsp_matrix_scale_values(A.h, dl.ptr, None, 0, None, None) == -1 and "out" in L.bmsp_last_error().decode()
    assert L.bmsp_matrix_scale_values(A.h, dl.ptr, None, 4, A.h, None) == -1 and "flags" in L.bmsp_last_error().decode()
    assert L.bmsp_matrix_scale_values(A.h, None, None, 2, A.h, None) == -1 and "d_right" in L.bmsp_last_error().decode()
    h = C.c_void_p()
    assert L.bmsp_matrix_scale(A.h, dl.ptr, None, 0, 2, None, C.byref(h)) == -1 and "out_transposed" in L.bmsp_last_error().decode()
    assert L.bmsp_matrix_scale(A.h, dl.ptr, None, 0, 0, None, None) == -1 and "out" in L.bmsp_last_error().decode()
    assert L.bmsp_matrix_diagonal(A.h, None, None) == -1 and "d_diag" in L.bmsp_last_error().decode()
    assert h.value is None
    with pytest.raises(ValueError):
        bmsp.scale(A, bmsp.DeviceArray(n, np.float64), None)
    with pytest.raises(ValueError):
        bmsp.scale(A, None, bmsp.DeviceArray(n - 1, np.float32))


# ---------------------------------------------------------------------------------------------------------
# 9. streams, 10. views
# ---------------------------------------------------------------------------------------------------------
def test_non_default_stream(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(13, 6)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, dtype=2)
    dl, dr = dev(bmsp, factors(n, 2, 41)), dev(bmsp, factors(n, 2, 42))
    H = _hip()
    s = C.c_void_p()
    assert H.hipStreamCreate(C.byref(s)) == 0
    try:
        S0 = bmsp.scale(A, dl, dr, div_left=True, transposed=0, stream=s.value)
        S1 = bmsp.scale(A, dl, dr, div_left=True, transposed=1, stream=s.value)
        d = bmsp.diagonal(A, stream=s.value)
        D = bmsp.from_diagonal(d, dtype=2, transposed=True, stream=s.value)
        B = A.with_layout(1)
        bmsp.scale_values(B, A, None, dr, stream=s.value)
        assert H.hipStreamSynchronize(s) == 0
        assert_same_arrays(S0, bmsp.scale(A, dl, dr, div_left=True, transposed=0))
        assert_same_arrays(S1, bmsp.scale(A, dl, dr, div_left=True, transposed=1))
        np.testing.assert_array_equal(d.to_host(), bmsp.diagonal(A).to_host())
        assert_same_arrays(D, bmsp.from_diagonal(bmsp.diagonal(A), dtype=2, transposed=True))
        assert_same_arrays(B, bmsp.scale(A, None, dr, transposed=1))
    finally:
        H.hipStreamDestroy(s)


def test_row_panel_views_are_refused(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(10, 4)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    dl = dev(bmsp, factors(n, 0, 1))
    V = A.row_panel(3, 9)
    for fn in (lambda: bmsp.scale(V, dl, None), lambda: bmsp.scale(V), lambda: bmsp.scale_values(V, V, dl, None), lambda: V.scale_(None, dl),
               lambda: bmsp.diagonal(V), lambda: bmsp.scale_values(A.with_layout(0), V, dl, None)):
        with pytest.raises(bmsp.BmspError) as e:
            fn()
        assert e.value.status == -1 and "view" in str(e.value), str(e.value)


# ---------------------------------------------------------------------------------------------------------
# 11. full size, 12. C++
# ---------------------------------------------------------------------------------------------------------
def test_headline_rmat20_matches_the_builder_of_the_scaled_coo(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(20, 2)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    l, rt = factors(n, 0, 51), factors(n, 0, 52)
    dl, dr = dev(bmsp, l), dev(bmsp, rt)
    snap = snapshot(A)
    cr, cc, cv = A.to_coo()
    with np.errstate(all="ignore"):
        sv = ((cv.astype(np.float32) * l[cr]) / rt[cc]).astype(np.float64)
    ddr, ddc, ddv = (bmsp.DeviceArray.from_host(x) for x in (cr, cc, sv))
    for lout in (0, 1):
        ref = bmsp.BmSpMatrix.from_coo_device(n, n, ddr, ddc, ddv, transposed=lout)
        S = bmsp.scale(A, dl, dr, div_right=True, transposed=lout)
        assert_same_arrays(S, ref)
        np.testing.assert_array_equal(S.block_row_ptr(), ref.block_row_ptr())
    assert_unchanged(A, snap)
    d = bmsp.diagonal(A).to_host()
    want = np.zeros(n, np.float32)
    want[cr[cr == cc]] = cv[cr == cc].astype(np.float32)
    np.testing.assert_array_equal(d.view(np.uint32), want.view(np.uint32))
    assert d.all()  # (the generator adds the identity)


def test_cpp_wrappers_run(bmsp, tmp_path):
    """tests/cpp_diag_check.cpp: bmSpMatrix<T>::diagonal / ::scale / ::scale_inplace and the free functions on the data/real fixture"""
    import subprocess
    from conftest import MTX
    from test_diag_api import build_cpp_diag_check
    exe = str(tmp_path / "cpp_diag_check")
    build_cpp_diag_check(exe)
    out = subprocess.run([exe, os.path.join(MTX, "real", "A_matrix.mtx")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    for word in ("CHECK diagonal OK", "CHECK scale unit diagonal OK", "CHECK scale identity OK", "CHECK from_diagonal OK", "CHECK half OK"):
        assert word in out.stdout, out.stdout
