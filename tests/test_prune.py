"""GPU tests of device-side pruning (bmsp_matrix_prune / bmsp_matrix_row_absmax).  The reference of every case is built from what the
test reads back from the device plus numpy: the stored entries of A, the keep decision `not (|v| <= thr)` in float64 with thr = tol or
tol * rowmax[row], and the CPU oracle's build of the kept COO in the output layout.  Structure, block-row pointer and counts must match
it exactly and values bit for bit (a NaN only has to be a NaN); A must come back unchanged."""
import ctypes as C
import os
import numpy as np
import pytest
import util
from stream_gate import _hip
from test_transpose import entries, assert_same_arrays, snapshot, assert_unchanged, _write_values
from test_add import stored, check_structure, assert_same_values

pytestmark = pytest.mark.gpu

NPDT = {0: np.float32, 1: np.float16, 2: np.float64}
OUTDT = {0: np.float32, 1: np.float32, 2: np.float64}
UINT = {0: np.uint32, 1: np.uint16, 2: np.uint64}


def build(bmsp, nr, nc, r, c, v, lay, dtype):
    return bmsp.BmSpMatrix.from_coo(nr, nc, r, c, v, transposed=lay, dtype=dtype)


def rowmax_ref(nr, r, v):
    """float64 row maxima of |v| over the non-NaN entries (0 for a row with none)"""
    a = np.abs(v.astype(np.float64))
    ok = ~np.isnan(a)
    out = np.zeros(nr, np.float64)
    np.maximum.at(out, r[ok], a[ok])
    return out


def keep_mask(nr, r, c, v, tol, rule, keep_diagonal):
    a = np.abs(v.astype(np.float64))
    with np.errstate(all="ignore"):
        thr = np.float64(tol) * rowmax_ref(nr, r, v)[r] if rule == "row_rel" else np.float64(tol)
        keep = ~(a <= thr)
    if keep_diagonal:
        keep |= r == c
    return keep


def check_prune(oracle, bmsp, A, tol, rule="abs", keep_diagonal=False, lay=0):
    """prune(A) against the oracle's build of the kept COO; A unchanged.  Returns (the pruned matrix, keep mask, (r, c, v) of A)."""
    i = A.info()
    nr, nc, dtype = i["num_rows"], i["num_cols"], i["dtype"]
    snap = snapshot(A)
    P, st = bmsp.prune(A, tol, rule, keep_diagonal, transposed=lay)
    assert_unchanged(A, snap)
    r, c, v = stored(A)
    keep = keep_mask(nr, r, c, v, tol, rule, keep_diagonal)
    ref = oracle.bmsp_from_coo(oracle.Coo(nr, nc, r[keep], c[keep], v[keep].astype(np.float64)), dtype, lay)
    check_structure(P, ref)
    assert P.info()["dtype"] == dtype
    assert st == {"nnz_in": i["nnz"], "nnz_out": int(keep.sum()), "blocks_in": i["block_num"], "blocks_out": ref.block_num}, st
    k, b, o, pv = P.host_arrays()
    assert o.size == ref.block_num + 1
    rr, cc, idx = entries(k, b, o, lay)
    got_order, want_order = np.argsort(rr * nc + cc), np.argsort(r[keep] * nc + c[keep])
    np.testing.assert_array_equal((rr * nc + cc)[got_order], (r[keep] * nc + c[keep])[want_order])
    assert_same_values(pv[idx][got_order], v[keep][want_order], dtype)
    return P, keep, (r, c, v)


# ---------------------------------------------------------------------------------------------------------
# 1. dtypes x layouts x rules x diagonal flag
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_all_layouts_rules_and_flags(oracle, bmsp, dtype):
    from pybmsp import gen
    nr, nc = 203, 157
    _, _, r, c, v = gen.random_coo(nr, nc, nr * 26, seed=3)
    for lin in (0, 1):
        A = build(bmsp, nr, nc, r, c, v, lin, dtype)
        for lout in (0, 1):
            for rule in ("abs", "row_rel"):
                for kd in (False, True):
                    P, keep, _ = check_prune(oracle, bmsp, A, 0.5, rule, kd, lout)
                    dropped = 1.0 - keep.mean()
                    print("dtype %d lin %d lout %d %s kd %d: dropped %.3f" % (dtype, lin, lout, rule, kd, dropped))
                    assert 0.25 < dropped < 0.75, dropped


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_keep_diagonal_on_a_square_matrix(oracle, bmsp, dtype):
    """a full diagonal of small values: gone without the flag, whole with it, under both rules"""
    from pybmsp import gen
    n = 163
    _, _, r, c, v = gen.random_coo(n, n, n * 20, seed=8)
    off = r != c
    d = np.arange(n)
    r, c, v = np.concatenate([r[off], d]), np.concatenate([c[off], d]), np.concatenate([v[off], np.full(n, 0.0625)])
    for lin in (0, 1):
        A = build(bmsp, n, n, r, c, v, lin, dtype)
        for lout in (0, 1):
            for rule in ("abs", "row_rel"):
                P0, _, _ = check_prune(oracle, bmsp, A, 0.5, rule, False, lout)
                P1, _, _ = check_prune(oracle, bmsp, A, 0.5, rule, True, lout)
                r0, c0, _ = stored(P0)
                r1, c1, _ = stored(P1)
                assert not np.any(r0 == c0)
                assert np.array_equal(np.sort(r1[r1 == c1]), d)
                assert P1.nnz == P0.nnz + n


# ---------------------------------------------------------------------------------------------------------
# 2. special values
# ---------------------------------------------------------------------------------------------------------
def _special_values(dtype, n, x, rng):
    T = NPDT[dtype]
    fi = np.finfo(T)
    x = T(x)
    sub_lo, sub_hi = fi.smallest_subnormal, np.nextafter(fi.tiny, T(0))
    pool = np.array([0.0, -0.0, sub_lo, -sub_lo, sub_hi, -sub_hi, np.inf, -np.inf, np.nan, x, -x, np.nextafter(x, T(np.inf)),
                     np.nextafter(x, T(0)), -np.nextafter(x, T(np.inf)), fi.tiny, fi.max], dtype=T)
    vals = rng.uniform(-1, 1, n).astype(T)
    pick = rng.random(n) < 0.6
    vals[pick] = pool[rng.integers(0, pool.size, int(pick.sum()))]
    vals[:pool.size] = pool  # every special at least once
    return vals


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_special_values(oracle, bmsp, dtype):
    from pybmsp import gen
    T = NPDT[dtype]
    rng = np.random.default_rng(40 + dtype)
    nr, nc = 64, 72
    _, _, r, c, v = gen.random_coo(nr, nc, 1500, seed=9)
    # 0.3 is the double the storage type rounds to (representable); 0.1 is not representable in fp16 / fp32: float32(0.1) > 0.1 stays,
    # float16(0.1) < 0.1 goes -- the decision follows the double comparison
    for x in (float(T(0.3)), 0.1):
        for lin in (0, 1):
            A = build(bmsp, nr, nc, r, c, v, lin, dtype)
            vals = _special_values(dtype, A.nnz, x, rng)
            _write_values(bmsp, A, vals)
            A.invalidate(False)
            a64 = np.abs(vals.astype(np.float64))
            nan = np.isnan(a64)
            for lout in (0, 1):
                P, _, _ = check_prune(oracle, bmsp, A, 0.0, "abs", False, lout)
                assert P.nnz == int((nan | (a64 != 0)).sum())  # only +0 and -0 go; subnormals stay
                pv = P.host_arrays()[3]
                assert np.any(np.abs(pv.astype(np.float64)) == float(np.finfo(T).smallest_subnormal))
                P, _, _ = check_prune(oracle, bmsp, A, x, "abs", False, lout)
                assert P.nnz == int((nan | (a64 > x)).sum())
                kept = np.abs(P.host_arrays()[3].astype(np.float64))
                assert float(np.nextafter(T(x), T(np.inf))) in kept
                if float(T(x)) <= x:
                    assert float(T(x)) not in kept
                else:
                    assert float(T(x)) in kept
                P, _, _ = check_prune(oracle, bmsp, A, np.inf, "abs", False, lout)
                assert P.nnz == int(nan.sum()) and np.all(np.isnan(P.host_arrays()[3]))
                for tol in (0.0, 0.5, x, 1.0, 1e300):
                    check_prune(oracle, bmsp, A, tol, "row_rel", False, lout)
                check_prune(oracle, bmsp, A, x, "row_rel", True, lout)


def test_negative_zero_survives_a_rule_that_keeps_it(oracle, bmsp):
    """ROW_REL with tol = 0 in a row that holds an Inf: 0 * Inf is NaN, nothing of the row goes, -0 keeps its sign"""
    nr = nc = 16
    r, c = np.repeat(np.arange(4), 4), np.tile(np.arange(4) * 3, 4)
    A = build(bmsp, nr, nc, r, c, np.ones(16), 0, 0)
    vals = np.array([np.inf, -0.0, 0.0, 1.0] + [0.0, -0.0, 2.0, 3.0] + [1.0] * 8, np.float32)
    rr, cc, idx = entries(*A.host_arrays()[:3], 0)
    hv = np.empty(16, np.float32)
    hv[idx[np.argsort(rr * nc + cc)]] = vals
    _write_values(bmsp, A, hv)
    A.invalidate(False)
    P, keep, _ = check_prune(oracle, bmsp, A, 0.0, "row_rel", False, 0)
    assert P.nnz == 14
    pr, pc, pv = stored(P)
    row0 = pv[pr == 0][np.argsort(pc[pr == 0])]
    np.testing.assert_array_equal(row0.view(np.uint32), vals[:4].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------
# 3. tiles that empty out
# ---------------------------------------------------------------------------------------------------------
def _emptying_case():
    from pybmsp import gen
    nr, nc = 250, 230
    _, _, r, c, v = gen.random_coo(nr, nc, nr * 30, seed=12)
    v = np.where(v < 0, v - 0.5, v + 0.5)  # every |v| in [0.5, 1.5)
    br, bc = r // 8, c // 8
    key = br.astype(np.int64) * 1000 + bc
    small = (br == 3) | (br == 17) | ((br * 7 + bc) % 5 == 0) | (key == key.min()) | (key == key.max())
    small |= (np.arange(r.size) % 11 == 0)  # single entries inside tiles that stay
    return nr, nc, r, c, np.where(small, v * 1e-3, v), small


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_tiles_and_block_rows_that_empty_out(oracle, bmsp, dtype):
    nr, nc, r, c, v, small = _emptying_case()
    for lin in (0, 1):
        A = build(bmsp, nr, nc, r, c, v, lin, dtype)
        for lout in (0, 1):
            P, keep, _ = check_prune(oracle, bmsp, A, 0.1, "abs", False, lout)
            assert P.nnz == int((~small).sum())
            k = P.host_arrays()[0]
            brows = (k >> np.uint64(32)).astype(np.int64)
            assert 3 not in brows and 17 not in brows and P.block_num < A.block_num
            ka = A.host_arrays()[0]
            assert k[0] != ka[0] and k[-1] != ka[-1]  # the first and the last tile went
            ptr = P.block_row_ptr()
            assert ptr[3] == ptr[4] and ptr[17] == ptr[18] and ptr[-1] == P.block_num


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_everything_dropped_and_nothing_dropped(oracle, bmsp, dtype):
    from pybmsp import gen
    nr, nc, r, c, v, _ = _emptying_case()
    for lin in (0, 1):
        A = build(bmsp, nr, nc, r, c, v, lin, dtype)
        for lout in (0, 1):
            Z, _, _ = check_prune(oracle, bmsp, A, 10.0, "abs", False, lout)
            zi = Z.info()
            assert (zi["nnz"], zi["block_num"], zi["transposed"], zi["num_rows"], zi["num_cols"]) == (0, 0, lout, nr, nc)
            k, b, o, zv = Z.host_arrays()
            assert k.size == 0 and b.size == 0 and zv.size == 0 and o.tolist() == [0]
            assert not Z.block_row_ptr().any()
            # a valid matrix for the other operators
            S = bmsp.add(Z, A, transposed=lin)
            assert_same_arrays(S, A)
            assert Z.transpose(lout).info()["block_num"] == 0 and Z.with_layout(1 - lout).info()["block_num"] == 0
            Z2, st = bmsp.prune(Z, 0.0, transposed=lin)
            assert st == {"nnz_in": 0, "nnz_out": 0, "blocks_in": 0, "blocks_out": 0} and Z2.info()["block_num"] == 0
            assert not bmsp.row_absmax(Z).to_host().any()
            if lout == 0:  # (the SpMV takes row-major tiles)
                x = bmsp.DeviceArray.from_host(gen.spmv_x(nc, "cusp").astype(NPDT[dtype]))
                y = bmsp.DeviceArray(nr, OUTDT[dtype])
                assert bmsp.lib().bmsp_memset(y.ptr, 0xFF, nr * y.dtype.itemsize) == 0
                assert not bmsp.spmv(Z, x, y).to_host().any()
            # nothing dropped: the layout conversion, byte for byte
            for rule in ("abs", "row_rel"):
                N, st = bmsp.prune(A, 0.0, rule, transposed=lout)
                assert st["nnz_out"] == A.nnz and st["blocks_out"] == A.block_num
                assert_same_arrays(N, A.with_layout(lout))


# ---------------------------------------------------------------------------------------------------------
# 4. sums that cancel
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_cancelled_sums_prune_to_the_symmetric_difference(oracle, bmsp, dtype):
    from pybmsp import gen
    nr, nc = 203, 157
    _, _, r1, c1, v1 = gen.random_coo(nr, nc, 5000, seed=21)
    _, _, r2, c2, v2 = gen.random_coo(nr, nc, 3000, seed=22)
    fresh = ~np.isin(r2.astype(np.int64) * nc + c2, r1.astype(np.int64) * nc + c1)
    rb, cb, vb = np.concatenate([r1[::2], r2[fresh]]), np.concatenate([c1[::2], c2[fresh]]), np.concatenate([v1[::2], v2[fresh]])
    want = np.sort(np.concatenate([(r1.astype(np.int64) * nc + c1)[1::2], (r2.astype(np.int64) * nc + c2)[fresh]]))
    for la, lb, lc in ((0, 0, 0), (0, 1, 1), (1, 0, 0), (1, 1, 1)):
        A, B = build(bmsp, nr, nc, r1, c1, v1, la, dtype), build(bmsp, nr, nc, rb, cb, vb, lb, dtype)
        D = bmsp.add(A, A, 1.0, -1.0, transposed=lc)
        assert D.nnz == A.nnz
        Z, _, _ = check_prune(oracle, bmsp, D, 0.0, "abs", False, lc)
        assert Z.nnz == 0 and Z.block_num == 0
        D = bmsp.add(A, B, 1.0, -1.0, transposed=lc)
        for lout in (0, 1):
            P, _, _ = check_prune(oracle, bmsp, D, 0.0, "abs", False, lout)
            pr, pc, _ = stored(P)
            np.testing.assert_array_equal(np.sort(pr * nc + pc), want)


# ---------------------------------------------------------------------------------------------------------
# 5. products
# ---------------------------------------------------------------------------------------------------------
def _csr(bmsp, nr, nc, r, c, v):
    o = np.lexsort((c, r))
    ro = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=nr))])
    return bmsp.CSRMatrix.from_arrays(nr, nc, ro, c[o], v[o])


def test_pruned_product_matches_the_host_csr_product_and_multiplies_on(oracle, bmsp):
    """A = [Y, Y, W], B = [X; -X; Z] with small integer values: A B = W Z, every coordinate that only Y X reaches is a stored 0"""
    from pybmsp import gen
    n, m, w, p = 120, 64, 40, 104
    _, _, ry, cy, vy = gen.random_coo(n, m, 900, seed=31, lo=-3.0, hi=3.0, integer=True)
    _, _, rw, cw, vw = gen.random_coo(n, w, 300, seed=32, lo=-3.0, hi=3.0, integer=True)
    _, _, rx, cx, vx = gen.random_coo(m, p, 800, seed=33, lo=-3.0, hi=3.0, integer=True)
    _, _, rz, cz, vz = gen.random_coo(w, p, 300, seed=34, lo=-3.0, hi=3.0, integer=True)
    ra, ca, va = np.concatenate([ry, ry, rw]), np.concatenate([cy, cy + m, cw + 2 * m]), np.concatenate([vy, vy, vw])
    rb, cb, vb = np.concatenate([rx, rx + m, rz + 2 * m]), np.concatenate([cx, cx, cz]), np.concatenate([vx, -vx, vz])
    k = 2 * m + w
    A, Bm = build(bmsp, n, k, ra, ca, va, 0, 0), build(bmsp, k, p, rb, cb, vb, 1, 0)
    Cm, _ = bmsp.spgemm(A, Bm, tc_version=5)
    assert np.any(Cm.host_arrays()[3] == 0)  # the symbolic structure holds cancelled entries
    H = _csr(bmsp, n, k, ra, ca, va).multiply_host(_csr(bmsp, k, p, rb, cb, vb))
    hn, hp, hro, hc, hv = H.arrays()
    assert (hn, hp) == (n, p) and hv.size and not np.any(hv == 0)  # the host path dropped them
    hr = np.repeat(np.arange(n), np.diff(hro))
    for lout in (0, 1):
        P, _, _ = check_prune(oracle, bmsp, Cm, 0.0, "abs", False, lout)
        assert P.nnz < Cm.nnz
        pr, pc, pv = stored(P)
        o, ho = np.argsort(pr * p + pc), np.argsort(hr.astype(np.int64) * p + hc)
        np.testing.assert_array_equal((pr * p + pc)[o], (hr.astype(np.int64) * p + hc)[ho])
        np.testing.assert_array_equal(pv[o], hv[ho])
    # the fresh handle in every operator slot: P P^T with P on the left, P^T P with P (converted) on the right
    P, _ = bmsp.prune(Cm, 0.0)
    pr, pc, pv = stored(P)
    pv = pv.astype(np.float64)
    o_p0, o_p1 = oracle.bmsp_from_coo(oracle.Coo(n, p, pr, pc, pv), 0, 0), oracle.bmsp_from_coo(oracle.Coo(n, p, pr, pc, pv), 0, 1)
    o_t0, o_t1 = oracle.bmsp_from_coo(oracle.Coo(p, n, pc, pr, pv), 0, 0), oracle.bmsp_from_coo(oracle.Coo(p, n, pc, pr, pv), 0, 1)
    for left, right, ol, orr in ((P, P.transpose(1), o_p0, o_t1), (P.transpose(0), P.with_layout(1), o_t0, o_p1)):
        G, st = bmsp.spgemm(left, right, tc_version=5)
        oc, ost = oracle.spgemm(ol, orr)
        gk, gb, go, gv = G.host_arrays()
        np.testing.assert_array_equal(gk, oc.keys)
        np.testing.assert_array_equal(gb, oc.bmps)
        np.testing.assert_array_equal(go, oc.offsets)
        assert st["c_nnz"] == ost["c_nnz"]
        np.testing.assert_array_equal(gv.astype(np.float64), oc.values)  # small integers: every sum exact


# ---------------------------------------------------------------------------------------------------------
# 6. row_absmax
# ---------------------------------------------------------------------------------------------------------
def check_row_absmax(bmsp, A):
    i = A.info()
    snap = snapshot(A)
    got = bmsp.row_absmax(A).to_host()
    assert_unchanged(A, snap)
    r, _, v = stored(A)
    want = rowmax_ref(i["num_rows"], r, v).astype(OUTDT[i["dtype"]])
    assert got.dtype == want.dtype and got.shape == want.shape
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8))
    return got


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_row_absmax_matches_numpy(bmsp, dtype, monkeypatch):
    from pybmsp import gen
    T = NPDT[dtype]
    nr, nc = 203, 157
    _, _, r, c, v = gen.random_coo(nr, nc, nr * 26, seed=5)
    gone = (r == 5) | ((r >= 100) & (r < 111)) | (r == nr - 1)  # empty rows, a whole empty block-row among them
    r, c, v = r[~gone], c[~gone], v[~gone]
    for lin in (0, 1):
        A = build(bmsp, nr, nc, r, c, v, lin, dtype)
        check_row_absmax(bmsp, A)
        rr, cc, idx = entries(*A.host_arrays()[:3], lin)
        vals = A.host_arrays()[3].copy()
        vals[idx[rr == 7]] = np.nan                                    # an all-NaN row -> 0
        sub = np.finfo(T).smallest_subnormal
        vals[idx[rr == 9]] = sub                                       # a row whose maximum is a subnormal
        vals[idx[rr == 9][0]] = -T(3) * sub
        vals[idx[rr == 12][0]] = np.nan                                # a NaN next to ordinary values: skipped
        vals[idx[rr == 13][0]] = -np.inf
        vals[idx[rr == 14]] = -0.0
        _write_values(bmsp, A, vals)
        A.invalidate(False)
        for g in ("1", "8", None):
            if g is None:
                monkeypatch.delenv("BMSP_PRUNE_LANES")
            else:
                monkeypatch.setenv("BMSP_PRUNE_LANES", g)
            got = check_row_absmax(bmsp, A)
            assert got[7] == 0 and got[5] == 0 and got[nr - 1] == 0 and not got[100:111].any()
            assert got[9] == float(T(3) * sub) and np.isinf(got[13]) and got[14] == 0 and np.isfinite(got[12]) and got[12] > 0
    n, _, r, c, v = gen.banded(300, 12)
    for lin in (0, 1):
        check_row_absmax(bmsp, build(bmsp, n, n, r, c, v, lin, dtype))


@pytest.mark.parametrize("dtype,lin", [(0, 0), (0, 1), (1, 0), (1, 1), (2, 1)])
def test_row_absmax_on_hub_block_rows(bmsp, dtype, lin, monkeypatch):
    """R-MAT 2^14 x 8: the first block-rows hold thousands of tiles, spread over many waves"""
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(14, 8)
    A = build(bmsp, n, n, r, c, v, lin, dtype)
    assert int(np.diff(A.block_row_ptr()).max()) > 1000
    check_row_absmax(bmsp, A)
    monkeypatch.setenv("BMSP_PRUNE_LANES", "8")
    check_row_absmax(bmsp, A)


# ---------------------------------------------------------------------------------------------------------
# 7. lane groups
# ---------------------------------------------------------------------------------------------------------
def test_both_lane_groups_agree(oracle, bmsp, monkeypatch):
    from pybmsp import gen
    for nr, nc, r, c, v in (gen.banded(400, 12), gen.rmat(12, 4)):
        for dtype in (0, 1, 2):
            for lin in (0, 1):
                A = build(bmsp, nr, nc, r, c, v, lin, dtype)
                outs = {}
                for g in ("1", "8"):
                    monkeypatch.setenv("BMSP_PRUNE_LANES", g)
                    outs[g] = [bmsp.prune(A, 0.4, rule, kd, transposed=lout)[0] for rule in ("abs", "row_rel") for kd in (False, True)
                               for lout in (0, 1)]
                    check_prune(oracle, bmsp, A, 0.4, "row_rel", True, 1 - lin)
                    check_prune(oracle, bmsp, A, 0.4, "abs", False, lin)
                for x, y in zip(outs["1"], outs["8"]):
                    assert_same_arrays(x, y)
    monkeypatch.delenv("BMSP_PRUNE_LANES")


# ---------------------------------------------------------------------------------------------------------
# 8. SpMV after pruning
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["chunked", "rowgroup"])
def test_spmv_of_the_pruned_matrix_is_the_spmv_of_the_matrix(bmsp, kind):
    """values k/64 and a small-integer x: every product and sum is exact in fp32, so dropping stored zeros changes no bit of y"""
    from pybmsp import gen
    if kind == "chunked":
        n, _, r, c, v = gen.rmat(17, 2)
    else:
        n, _, r, c, v = gen.banded(1 << 12, 16)
    v = np.round(v * 64) / 64
    v[::3] = 0.0
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    assert A.nnz == v.size  # explicit zeros are stored
    P, st = bmsp.prune(A, 0.0)
    assert st["nnz_out"] == int(np.count_nonzero(v)) < st["nnz_in"]
    want = "spmv_chunk_kernel" if kind == "chunked" else "spmv_rowgroup_kernel"
    assert bmsp.spmv_launch_info(A)["kernel"] == want, bmsp.spmv_launch_info(A)
    if kind == "chunked":  # what is left still takes the chunked sweep (the banded tiles are no longer full: the library's choice)
        for M in (A, P):
            i = M.info()
            assert i["nnz"] < 2 * i["block_num"] and i["nnz"] >= 128 * 512
        assert bmsp.spmv_launch_info(P)["kernel"] == want, bmsp.spmv_launch_info(P)
    x = bmsp.DeviceArray.from_host(gen.spmv_x(n, "cusp"))
    ya, yp = bmsp.DeviceArray(n, np.float32), bmsp.DeviceArray(n, np.float32)
    for y in (ya, yp):
        assert bmsp.lib().bmsp_memset(y.ptr, 0xFF, n * 4) == 0
    ha, hp = bmsp.spmv(A, x, ya).to_host(), bmsp.spmv(P, x, yp).to_host()
    assert np.all(np.isfinite(ha))
    np.testing.assert_array_equal(ha, hp)
    S = util.scipy_csr(n, n, r, c, v)
    np.testing.assert_array_equal(ha.astype(np.float64), S @ gen.spmv_x(n, "cusp").astype(np.float64))


# ---------------------------------------------------------------------------------------------------------
# 9. count only, refusals, streams
# ---------------------------------------------------------------------------------------------------------
def test_count_only_equals_the_real_call(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(12, 6)
    for dtype in (0, 1, 2):
        for lin in (0, 1):
            A = build(bmsp, n, n, r, c, v, lin, dtype)
            for rule, tol, kd in (("abs", 0.5, False), ("abs", 0.0, False), ("row_rel", 0.3, True), ("abs", np.inf, True), ("row_rel", 1.0, False)):
                P, st = bmsp.prune(A, tol, rule, kd)
                assert bmsp.prune_count(A, tol, rule, kd) == st
                assert (P.nnz, P.block_num) == (st["nnz_out"], st["blocks_out"])
    # the raw call: out == NULL is left alone, stats filled
    st = bmsp.PruneStats()
    bmsp.check(bmsp.lib().bmsp_matrix_prune(A.h, 0, 0.5, 0, 0, None, None, C.byref(st)))
    assert st.nnz_in == A.nnz and 0 < st.nnz_out < st.nnz_in
    # and stats == NULL with an output
    h = C.c_void_p()
    bmsp.check(bmsp.lib().bmsp_matrix_prune(A.h, 0, 0.5, 0, 0, None, C.byref(h), None))
    assert bmsp.BmSpMatrix(h.value).nnz == st.nnz_out


def test_refusals_on_real_handles(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(10, 4)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)

    def refused(fn, word):
        with pytest.raises(bmsp.BmspError) as e:
            fn()
        assert e.value.status == -1 and word in str(e.value), str(e.value)

    V = A.row_panel(3, 9)
    refused(lambda: bmsp.prune(V, 0.5), "view")
    refused(lambda: bmsp.prune_count(V, 0.5), "view")
    refused(lambda: bmsp.row_absmax(V), "view")
    refused(lambda: bmsp.prune(A, -0.5), "tol")
    refused(lambda: bmsp.prune(A, float("nan")), "tol")
    refused(lambda: bmsp.prune(A, float("inf"), "row_rel"), "tol")
    refused(lambda: bmsp.prune_count(A, -1.0, "row_rel"), "tol")
    L = bmsp.lib()
    h, st = C.c_void_p(), bmsp.PruneStats()
    for args, word in (((A.h, 2, 0.5, 0, 0), "rule"), ((A.h, -1, 0.5, 0, 0), "rule"), ((A.h, 0, 0.5, 2, 0), "flags"), ((A.h, 1, 0.5, 4, 0), "flags"),
                       ((A.h, 0, 0.5, 0, 2), "out_transposed")):
        rc = L.bmsp_matrix_prune(*args, None, C.byref(h), C.byref(st))
        assert rc == -1 and word in L.bmsp_last_error().decode(), L.bmsp_last_error()
        assert h.value is None
    assert L.bmsp_matrix_prune(A.h, 0, 0.5, 0, 0, None, None, None) == -1
    assert L.bmsp_matrix_row_absmax(A.h, None, None) == -1 and "d_rowmax" in L.bmsp_last_error().decode()
    with pytest.raises(ValueError):
        bmsp.prune(A, 0.5, "column_rel")


def test_non_default_stream(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(13, 6)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, dtype=2)
    H = _hip()
    s = C.c_void_p()
    assert H.hipStreamCreate(C.byref(s)) == 0
    try:
        for rule in ("abs", "row_rel"):
            P, st = bmsp.prune(A, 0.3, rule, True, transposed=1, stream=s.value)
            P0, st0 = bmsp.prune(A, 0.3, rule, True, transposed=1)
            assert st == st0
            assert_same_arrays(P, P0)
        m = bmsp.row_absmax(A, stream=s.value)
        assert H.hipStreamSynchronize(s) == 0
        np.testing.assert_array_equal(m.to_host(), bmsp.row_absmax(A).to_host())
    finally:
        H.hipStreamDestroy(s)


# ---------------------------------------------------------------------------------------------------------
# 10. full size
# ---------------------------------------------------------------------------------------------------------
def test_headline_rmat20_matches_the_builder_of_the_filtered_coo(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(20, 2)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    vals = A.host_arrays()[3].copy()
    vals[::3] = 0.0
    _write_values(bmsp, A, vals)
    A.invalidate(False)
    snap = snapshot(A)
    cr, cc, cv = A.to_coo()
    keep = cv != 0
    assert abs(keep.mean() - 2 / 3) < 0.01
    dr, dc, dv = (bmsp.DeviceArray.from_host(x[keep]) for x in (cr, cc, cv))
    for lout in (0, 1):
        ref = bmsp.BmSpMatrix.from_coo_device(n, n, dr, dc, dv, transposed=lout)
        P, st = bmsp.prune(A, 0.0, transposed=lout)
        assert st["nnz_out"] == int(keep.sum()) and st["blocks_out"] == ref.block_num < A.block_num
        assert_same_arrays(P, ref)
        np.testing.assert_array_equal(P.block_row_ptr(), ref.block_row_ptr())
    assert_unchanged(A, snap)


def test_cpp_wrappers_run(bmsp, tmp_path):
    """tests/cpp_prune_check.cpp: bmSparse_prune / bmSpMatrix<T>::prune on the data/real fixture"""
    import subprocess
    from conftest import MTX
    from test_prune_api import build_cpp_prune_check
    exe = str(tmp_path / "cpp_prune_check")
    build_cpp_prune_check(exe)
    out = subprocess.run([exe, os.path.join(MTX, "real", "A_matrix.mtx")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    for word in ("CHECK prune zeros OK", "CHECK prune identity OK", "CHECK prune row_rel OK", "CHECK half OK"):
        assert word in out.stdout, out.stdout
