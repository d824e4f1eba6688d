"""GPU tests of bmsp_spgemm_masked / bmsp_spgemm_masked_values / bmsp_spgemm_masked_launch_info: C = alpha * (A * B) on the pattern of M
+ beta * M, or * M.

Expected values come from the host: oracle.spgemm(A_o, B_o, exact_products=(dtype is F16)) on oracle matrices built from the same COO (A
row-major, B column-major, as orc_spgemm requires), sampled at M's coordinates, +0 where the product stores nothing, then passed through
the epilogue in numpy in the arithmetic type, operation by operation.

1. Integer operands (a, b in [-3, 3], hub cases in {-1, 0, 1}, m in [-4, 4]): every partial sum and every result is exactly
   representable (the host self-check in test_spgemm_masked_api.py asserts it in int64 for the very arrays used here), so the four arrays
   of the output equal those of from_coo of the expected result, and one lane and eight lanes per tile agree in every bit.
2. The order, real operands with magnitudes in [0.5, 2): with alpha = 1 and beta = 0 the result EQUALS (==; the sign of a zero is free)
   the oracle's product sampled on M -- the same chain of fused multiply-adds, k ascending -- and, for F32 / F64, what
   pybmsp.spgemm(A, B, tc_version=5) stores at M's coordinates on the device; two calls give the same bits.
3. Special values: stored entries only (an Inf or NaN in A opposite an inner index B's column does not store does not reach the
   result, a stored 0 against a stored Inf gives NaN); a NaN stored in M with beta = 0 does not propagate; an F16 result beyond 65504 is
   Inf; subnormal products are kept.
4. Life cycle: in place, into a with_layout copy, a scale output, an sddmm output and an earlier masked output; refusals; A, B and M
   unchanged; value updates in place need no invalidate; invalidate(B, 1) rebuilds the view; value caches dropped; a gated stream.
5. launch_info: kernel name and lanes follow the switch and the default rule, pairs equals a numpy restatement."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from test_transpose import snapshot, assert_unchanged, assert_same_arrays, entries

pytestmark = pytest.mark.gpu

F32, F16, F64 = 0, 1, 2
NPDT = {0: np.float32, 1: np.float16, 2: np.float64}
ARITH = {0: np.float32, 1: np.float32, 2: np.float64}
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
DNAME = ("f32", "f16", "f64")
# (dtype of A and B, dtype of M and of the output): the four combinations the call takes
DTYPES = ((F32, F32), (F16, F16), (F16, F32), (F64, F64))
LANES = (None, "1", "8")
# (alpha, beta, mul_m) of test 1
EPILOGUES = ((1.0, 0.0, False), (-2.0, 1.0, False), (0.5, -1.0, False), (1.0, 0.0, True), (-0.5, 0.0, True))
HUBS = {"hub300x3": (300, 3), "hub3x300": (3, 300), "hub300x300": (300, 300), "hub_nomatch": (150, 3)}  # tiles in A's block-row, B's block-column
NAMES = ("1x1", "5x3x7", "13x70x11", "random", "dense", "rmat", "banded", "outside", "a0", "b0", "m0", "rows0") + tuple(HUBS)
FILL_THRESHOLD = 0  # mean values per M tile from which eight lanes are the default: always (spgemm_masked.hip, DESIGN section 4 "Masked SpGEMM")

_CACHE = {}


def _coo(x):
    return (np.asarray(x[2], np.int64), np.asarray(x[3], np.int64))


def _hub(rng, n_blocks, a_blocks, b_blocks):
    """A 8 x 8n with one value per tile in the block columns a_blocks, B 8n x 8 with one per tile in the block-rows b_blocks; the value
    of block K sits at inner index 8K + K % 8 on both sides, so a common block is a common inner index; M is the dense 8 x 8 tile"""
    ka, kb = np.asarray(a_blocks, np.int64), np.asarray(b_blocks, np.int64)
    A = (rng.integers(0, 8, ka.size), 8 * ka + ka % 8)
    B = (8 * kb + kb % 8, rng.integers(0, 8, kb.size))
    mr, mc = np.divmod(np.arange(64), 8)
    return (8, 8 * n_blocks, 8, A, B, (mr, mc))


def patterns():
    """{name: (m, n, p, (A rows, cols), (B rows, cols), (M rows, cols))}: the coordinates only, generated once"""
    if "coo" not in _CACHE:
        from pybmsp import gen
        rng = np.random.default_rng(4242)
        e = (np.zeros(0, np.int64), np.zeros(0, np.int64))
        dense = lambda nr, nc: tuple(np.divmod(np.arange(nr * nc), nc))
        rc = lambda nr, nc, nnz, seed: _coo(gen.random_coo(nr, nc, nnz, seed=seed))
        m = {}
        m["1x1"] = (1, 1, 1, dense(1, 1), dense(1, 1), dense(1, 1))
        m["5x3x7"] = (5, 3, 7, rc(5, 3, 9, 11), rc(3, 7, 12, 12), rc(5, 7, 20, 13))
        m["13x70x11"] = (13, 70, 11, rc(13, 70, 300, 14), rc(70, 11, 260, 15), rc(13, 11, 90, 16))
        m["random"] = (203, 157, 90, rc(203, 157, 203 * 12, 17), rc(157, 90, 157 * 9, 18), rc(203, 90, 203 * 9, 19))
        m["dense"] = (16, 40, 24, rc(16, 40, 250, 20), rc(40, 24, 400, 21), dense(16, 24))
        g = gen.rmat(10, 8)
        m["rmat"] = (g[0], g[0], g[0], _coo(g), _coo(g), _coo(g))
        g = gen.banded(133, 12)
        m["banded"] = (g[0], g[0], g[0], _coo(g), _coo(g), _coo(g))
        # the product lives in rows 0 .. 7 and columns 0 .. 15: most of the mask's coordinates and whole tiles of it lie outside
        ar, ac = rc(8, 24, 60, 22)
        br, bc = rc(24, 16, 90, 23)
        m["outside"] = (40, 24, 40, (ar, ac), (br, bc), rc(40, 40, 500, 24))
        m["a0"] = (37, 21, 11, e, rc(21, 11, 60, 25), rc(37, 11, 80, 26))
        m["b0"] = (37, 21, 11, rc(37, 21, 90, 27), e, rc(37, 11, 80, 28))
        m["m0"] = (37, 21, 11, rc(37, 21, 90, 29), rc(21, 11, 60, 30), e)
        m["rows0"] = (0, 21, 11, e, rc(21, 11, 60, 31), e)
        m["hub300x3"] = _hub(rng, 300, np.arange(300), [0, 137, 299])
        m["hub3x300"] = _hub(rng, 300, [0, 137, 299], np.arange(300))
        pick = lambda: np.sort(np.concatenate([[0, 399], 1 + rng.choice(398, 298, replace=False)]))
        m["hub300x300"] = _hub(rng, 400, pick(), pick())
        m["hub_nomatch"] = _hub(rng, 300, 1 + 2 * np.arange(150), [0, 150, 298])
        _CACHE["coo"] = {k: (x[0], x[1], x[2]) + tuple((np.asarray(y[0], np.int64), np.asarray(y[1], np.int64)) for y in x[3:]) for k, x in m.items()}
    return _CACHE["coo"]


def int_operands(name):
    """integer values per stored coordinate of A, B (in [-3, 3]; hub cases {-1, 0, 1}) and M (in [-4, 4]), fixed per pattern"""
    key = ("int", name)
    if key not in _CACHE:
        _, _, _, A, B, M = patterns()[name]
        rng = np.random.default_rng(300 + NAMES.index(name))
        lo, hi = (-1, 2) if name in HUBS else (-3, 4)
        _CACHE[key] = (rng.integers(lo, hi, A[0].size), rng.integers(lo, hi, B[0].size), rng.integers(-4, 5, M[0].size))
    return _CACHE[key]


def real_operands(name, dtype):
    """values with magnitudes in [0.5, 2) and random signs, all mantissa bits in use, rounded to the storage type of A and B"""
    key = ("real", name, dtype)
    if key not in _CACHE:
        _, _, _, A, B, M = patterns()[name]
        rng = np.random.default_rng(700 + 10 * NAMES.index(name) + dtype)
        draw = lambda n: (rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(NPDT[dtype]).astype(np.float64)
        _CACHE[key] = (draw(A[0].size), draw(B[0].size), draw(M[0].size))
    return _CACHE[key]


def dense_of(nr, nc, rc, vals, dtype=np.float64):
    d = np.zeros((nr, nc), dtype)
    d[rc[0], rc[1]] = vals
    return d


def int_dots(name):
    """(d, sum |a b|) at M's coordinates from a dense numpy product (float64: exact for these integers)"""
    key = ("int_dot", name)
    if key not in _CACHE:
        m, n, p, A, B, M = patterns()[name]
        a, b, _ = int_operands(name)
        Ad, Bd = dense_of(m, n, A, a), dense_of(n, p, B, b)
        d = (Ad @ Bd)[M[0], M[1]]
        s = (np.abs(Ad) @ np.abs(Bd))[M[0], M[1]]
        _CACHE[key] = (d.astype(np.int64), s.astype(np.int64))
    return _CACHE[key]


def oracle_dots(oracle, name, a, b, dtype):
    """the oracle's product (the chain of fused multiply-adds, k ascending; F16: exact products) sampled at M's coordinates, +0 where
    the product stores nothing, in the arithmetic type"""
    m, n, p, A, B, M = patterns()[name]
    if A[0].size == 0 or B[0].size == 0 or M[0].size == 0:  # (no product to sample, or nothing to sample it at)
        return np.zeros(M[0].size, ARITH[dtype])
    Ao = oracle.bmsp_from_coo(oracle.Coo(m, n, A[0], A[1], a), dtype, False)
    Bo = oracle.bmsp_from_coo(oracle.Coo(n, p, B[0], B[1], b), dtype, True)
    Co, _ = oracle.spgemm(Ao, Bo, exact_products=(dtype == F16))
    cr, cc, idx = entries(Co.keys, Co.bmps, Co.offsets, 0)
    return sample(cr, cc, Co.values[idx], M, p).astype(ARITH[dtype])


def sample(r, c, v, M, p):
    """the values of the COO (r, c, v) at M's coordinates, +0 where it holds none"""
    out = np.zeros(M[0].size, np.float64)
    if len(r) == 0 or M[0].size == 0:
        return out
    key = np.asarray(r, np.int64) * p + np.asarray(c, np.int64)
    order = np.argsort(key)
    key, v = key[order], np.asarray(v, np.float64)[order]
    want = M[0] * p + M[1]
    pos = np.minimum(np.searchsorted(key, want), key.size - 1)
    hit = key[pos] == want
    out[hit] = v[pos[hit]]
    return out


def epilogue_ref(d, mv, alpha, beta, mul_m, adtype, mdtype):
    """numpy arithmetic in the arithmetic type, one rounding per operation, then one rounding to the output type"""
    Fa = ARITH[adtype]
    with np.errstate(all="ignore"):
        t = Fa(alpha) * d.astype(Fa)
        if mul_m:
            out = t * mv.astype(Fa)
        elif Fa(beta) == 0:
            out = t
        else:
            out = t + Fa(beta) * mv.astype(Fa)
        return out.astype(NPDT[mdtype])


def int_expected(oracle, name, dt, e):
    """expected output values per stored coordinate of M for integer case (name, dtype pair, epilogue)"""
    key = ("int_exp", name, dt, e)
    if key not in _CACHE:
        a, b, mv = int_operands(name)
        dk = ("int_orc", name, DTYPES[dt][0])
        if dk not in _CACHE:
            _CACHE[dk] = oracle_dots(oracle, name, a.astype(np.float64), b.astype(np.float64), DTYPES[dt][0])
        _CACHE[key] = epilogue_ref(_CACHE[dk], mv.astype(np.float64), *EPILOGUES[e], DTYPES[dt][0], DTYPES[dt][1])
    return _CACHE[key]


def int_cases():
    """test 1: every pattern x dtype combination three times; the three operand layouts, the output layout, the lane switch and the
    epilogue drawn per case from a fixed stream (test_spgemm_masked_api.py asserts that every value of every parameter occurs)"""
    if "int_cases" not in _CACHE:
        rng = np.random.default_rng(20251)
        out = []
        for name in NAMES:
            for dt in range(len(DTYPES)):
                for rep in range(3):
                    out.append((name, dt, int(rng.integers(2)), int(rng.integers(2)), int(rng.integers(2)), int(rng.integers(2)),
                                LANES[rng.integers(3)], int(rng.integers(len(EPILOGUES)))))
        _CACHE["int_cases"] = out
    return _CACHE["int_cases"]


def case_id(c):
    return "%s-%s_%s-a%d-b%d-m%d-o%d-lanes%s-e%d" % (c[0], DNAME[DTYPES[c[1]][0]], DNAME[DTYPES[c[1]][1]], c[2], c[3], c[4], c[5], c[6] or "dflt", c[7])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def assert_exact(got, want, msg=""):
    """equal as values everywhere, bit for bit wherever the result is not zero (the sign of a zero result is not specified)"""
    assert got.dtype == want.dtype and got.shape == want.shape, msg
    np.testing.assert_array_equal(got, want, err_msg=msg)
    nz = want != 0
    np.testing.assert_array_equal(bits(got)[nz], bits(want)[nz], err_msg=msg)


def set_lanes(monkeypatch, lanes):
    if lanes is None:
        monkeypatch.delenv("BMSP_MASKED_LANES", raising=False)
    else:
        monkeypatch.setenv("BMSP_MASKED_LANES", lanes)


def build(bmsp, name, which, vals, lay, dtype):
    m, n, p, A, B, M = patterns()[name]
    nr, nc, rc = {"A": (m, n, A), "B": (n, p, B), "M": (m, p, M)}[which]
    return bmsp.BmSpMatrix.from_coo(nr, nc, rc[0], rc[1], np.asarray(vals, np.float64), transposed=lay, dtype=dtype)


def source(bmsp, name, which, dtype, lay):
    """the integer-valued operand `which` of a pattern, built once per (dtype, layout): the out-of-place calls never modify it"""
    key = ("src", name, which, dtype, lay)
    if key not in _CACHE:
        _CACHE[key] = build(bmsp, name, which, int_operands(name)["ABM".index(which)], lay, dtype)
    return _CACHE[key]


def expected_pairs(name):
    """numpy restatement of `pairs`: the boolean block-pattern product of A and B summed over M's tiles"""
    m, n, p, A, B, M = patterns()[name]
    nbr, nbk, nbc = (m + 7) // 8, (n + 7) // 8, (p + 7) // 8
    BA, BB = np.zeros((nbr, nbk)), np.zeros((nbk, nbc))
    BA[A[0] // 8, A[1] // 8] = 1
    BB[B[0] // 8, B[1] // 8] = 1
    P = BA @ BB
    tiles = np.unique((M[0] // 8) * nbc + M[1] // 8) if M[0].size else np.zeros(0, np.int64)
    return int(P.ravel()[tiles].sum()) if tiles.size else 0


def expected_info(bmsp, name, B, M, lanes):
    i = M.info()
    view = bmsp.spmv_op_launch_info(B, "T")["view_bytes"] if patterns()[name][3][0].size and B.info()["block_num"] else 0
    if i["block_num"] == 0 or i["nnz"] == 0:
        return {"kernel": "none (empty mask)", "lanes": 0, "pairs": 0, "view_bytes": view}
    g = int(lanes) if lanes else (1 if i["nnz"] < FILL_THRESHOLD * i["block_num"] else 8)
    return {"kernel": "spgemm_masked_kernel<%d>" % g, "lanes": g, "pairs": expected_pairs(name), "view_bytes": view}


# ---------------------------------------------------------------------------------------------------------
# 1. integer operands, bit for bit
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", int_cases(), ids=case_id)
def test_integer_operands_exact(bmsp, oracle, monkeypatch, case):
    name, dt, a_lay, b_lay, m_lay, o_lay, lanes, e = case
    adt, mdt = DTYPES[dt]
    alpha, beta, mul_m = EPILOGUES[e]
    m, n, p, _, _, Mc = patterns()[name]
    A, B, M = source(bmsp, name, "A", adt, a_lay), source(bmsp, name, "B", adt, b_lay), source(bmsp, name, "M", mdt, m_lay)
    snaps = [snapshot(x) for x in (A, B, M)]
    exp = int_expected(oracle, name, dt, e)
    want = bmsp.BmSpMatrix.from_coo(m, p, Mc[0], Mc[1], exp.astype(np.float64), transposed=o_lay, dtype=mdt)
    wk, wb, wo, wv = want.host_arrays()

    set_lanes(monkeypatch, lanes)
    info = bmsp.spgemm_masked_launch_info(A, B, M, o_lay)
    assert info == expected_info(bmsp, name, B, M, lanes), (info, expected_info(bmsp, name, B, M, lanes))
    Cm = bmsp.spgemm_masked(A, B, M, alpha, beta, mul_m, transposed=o_lay)
    assert Cm.info() == want.info()
    gk, gb, go, gv = Cm.host_arrays()
    for g, w in ((gk, wk), (gb, wb), (go, wo)):
        np.testing.assert_array_equal(g, w)
    assert_exact(gv, wv, case_id(case))
    np.testing.assert_array_equal(Cm.block_row_ptr(), want.block_row_ptr())
    conv = M.with_layout(o_lay)
    for g, w in zip(Cm.host_arrays()[:3], conv.host_arrays()[:3]):
        np.testing.assert_array_equal(g, w)
    np.testing.assert_array_equal(Cm.block_row_ptr(), conv.block_row_ptr())
    for x, s in zip((A, B, M), snaps):
        assert_unchanged(x, s)

    # one lane and eight lanes per tile agree in every bit, with each other and with the call above
    for g in ("1", "8"):
        set_lanes(monkeypatch, g)
        other = bmsp.spgemm_masked(A, B, M, alpha, beta, mul_m, transposed=o_lay).host_arrays()[3]
        np.testing.assert_array_equal(bits(other), bits(gv), err_msg=g)


# ---------------------------------------------------------------------------------------------------------
# 2. the order of summation
# ---------------------------------------------------------------------------------------------------------
ORDER_NAMES = ("random", "rmat", "banded") + tuple(HUBS)


def order_cases():
    rng = np.random.default_rng(909)
    return [(name, dt, int(rng.integers(2)), int(rng.integers(2)), int(rng.integers(2)), int(rng.integers(2)), LANES[rng.integers(3)])
            for name in ORDER_NAMES for dt in range(len(DTYPES))]


@pytest.mark.parametrize("case", order_cases(), ids=lambda c: "%s-%s_%s-a%d-b%d-m%d-o%d-lanes%s" % (c[0], DNAME[DTYPES[c[1]][0]], DNAME[DTYPES[c[1]][1]], c[2], c[3], c[4], c[5], c[6] or "dflt"))
def test_the_order_is_the_fma_chain(bmsp, oracle, monkeypatch, case):
    name, dt, a_lay, b_lay, m_lay, o_lay, lanes = case
    adt, mdt = DTYPES[dt]
    m, n, p, Ac, Bc, Mc = patterns()[name]
    a, b, mv = real_operands(name, adt)
    A, B, M = build(bmsp, name, "A", a, a_lay, adt), build(bmsp, name, "B", b, b_lay, adt), build(bmsp, name, "M", mv, m_lay, mdt)
    exp = oracle_dots(oracle, name, a, b, adt).astype(NPDT[mdt])  # alpha = 1, beta = 0: c = d, rounded once to an F16 output
    assert np.all(np.isfinite(exp))
    order = np.lexsort((Mc[1], Mc[0]))  # to_coo's order
    set_lanes(monkeypatch, lanes)
    Cm = bmsp.spgemm_masked(A, B, M, transposed=o_lay)
    gr, gc, gv = Cm.to_coo()
    np.testing.assert_array_equal(gr, Mc[0][order])
    np.testing.assert_array_equal(gc, Mc[1][order])
    got = np.asarray(gv).astype(NPDT[mdt])
    assert np.all(got == exp[order]), (case, int(np.sum(got != exp[order])))
    # two calls, the same bits
    again = bmsp.spgemm_masked(A, B, M, transposed=o_lay)
    assert_same_arrays(Cm, again)
    if adt in (F32, F64):  # the device's own V15 product (the same chain), sampled the same way
        A0 = A if a_lay == 0 else A.with_layout(0)
        B1 = B if b_lay == 1 else B.with_layout(1)
        P, _ = bmsp.spgemm(A0, B1, tc_version=5)
        pr, pc, pv = P.to_coo()
        dev = sample(pr, pc, pv, Mc, p).astype(NPDT[mdt])
        assert np.all(got == dev[order]), (case, int(np.sum(got != dev[order])))


# ---------------------------------------------------------------------------------------------------------
# 3. special values
# ---------------------------------------------------------------------------------------------------------
def small(bmsp, nr, nc, triples, lay, dtype):
    r, c, v = (np.array(x) for x in zip(*triples))
    return bmsp.BmSpMatrix.from_coo(nr, nc, r.astype(np.int64), c.astype(np.int64), v.astype(np.float64), transposed=lay, dtype=dtype)


def values_by_coord(Cm):
    r, c, v = Cm.to_coo()
    return {(int(i), int(j)): x for i, j, x in zip(r, c, v)}


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("lays", [(0, 0, 0, 0), (1, 1, 1, 1), (0, 1, 0, 1), (1, 0, 1, 0)])
@pytest.mark.parametrize("dt", range(len(DTYPES)))
def test_stored_entries_only(bmsp, monkeypatch, dt, lays, lanes):
    adt, mdt = DTYPES[dt]
    a_lay, b_lay, m_lay, o_lay = lays
    inf, nan = float("inf"), float("nan")
    # row 0 of A: Inf at k = 0 and NaN at k = 1 (B's columns store neither), 2 at k = 2, a stored 0 at k = 9, 3 at k = 10, -Inf at k = 17
    A = small(bmsp, 2, 20, [(0, 0, inf), (0, 1, nan), (0, 2, 2.0), (0, 9, 0.0), (0, 10, 3.0), (0, 17, -inf), (1, 3, 1.0)], a_lay, adt)
    # column 0 of B: 5 at k = 2, 1 at k = 10; column 1: Inf at k = 9 (against the stored 0); column 2: a NaN at k = 4, which A does not store
    B = small(bmsp, 20, 3, [(2, 0, 5.0), (10, 0, 1.0), (9, 1, inf), (4, 2, nan), (10, 2, 2.0)], b_lay, adt)
    M = small(bmsp, 2, 3, [(0, 0, 1.0), (0, 1, 1.0), (0, 2, 1.0), (1, 0, 1.0), (1, 2, 1.0)], m_lay, mdt)
    set_lanes(monkeypatch, lanes)
    got = values_by_coord(bmsp.spgemm_masked(A, B, M, transposed=o_lay))
    assert got[(0, 0)] == 13.0 and got[(0, 2)] == 6.0 and got[(1, 0)] == 0.0 and got[(1, 2)] == 0.0, got
    assert np.isnan(got[(0, 1)]), got


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("dt", range(len(DTYPES)))
def test_nan_in_mask_overflow_and_subnormals(bmsp, monkeypatch, dt, lanes):
    adt, mdt = DTYPES[dt]
    tiny = {F32: 2.0 ** -70, F16: 2.0 ** -12, F64: 2.0 ** -520}[adt]
    sub = tiny * tiny  # a subnormal of the arithmetic type (F16 operands: 2^-24, the smallest fp16 subnormal, a normal fp32)
    A = small(bmsp, 3, 9, [(0, 0, 300.0), (0, 8, 300.0), (1, 1, tiny), (2, 2, 1.0)], 0, adt)
    B = small(bmsp, 9, 2, [(0, 0, 300.0), (8, 0, 300.0), (1, 1, tiny), (2, 1, 1.0)], 1, adt)
    M = small(bmsp, 3, 2, [(0, 0, float("nan")), (1, 1, float("nan")), (2, 1, 2.0), (2, 0, float("nan"))], 0, mdt)
    set_lanes(monkeypatch, lanes)
    got = values_by_coord(bmsp.spgemm_masked(A, B, M))  # beta = 0: m is not read
    assert not any(np.isnan(v) for v in got.values()), got
    assert got[(1, 1)] == sub and sub > 0 and got[(2, 1)] == 1.0 and got[(2, 0)] == 0.0, got
    if mdt == F16:
        assert got[(0, 0)] == float("inf"), got  # 180000 is beyond 65504
    else:
        assert got[(0, 0)] == 180000.0, got
    got = values_by_coord(bmsp.spgemm_masked(A, B, M, 1.0, 1.0))  # beta != 0: the stored NaN is read
    assert np.isnan(got[(0, 0)]) and np.isnan(got[(1, 1)]) and got[(2, 1)] == 3.0, got
    got = values_by_coord(bmsp.spgemm_masked(A, B, M, 1.0, 0.0, True))
    assert np.isnan(got[(0, 0)]) and got[(2, 1)] == 2.0, got


# ---------------------------------------------------------------------------------------------------------
# 4. life cycle
# ---------------------------------------------------------------------------------------------------------
def refused(bmsp, fn, word):
    with pytest.raises(bmsp.BmspError) as e:
        fn()
    assert e.value.status == -1 and word in str(e.value), str(e.value)


def raw_values(bmsp, A, B, M, out, alpha=1.0, beta=0.0, flags=0):
    """bmsp_spgemm_masked_values through the raw C call (the Python wrapper refuses out == A / out == B itself)"""
    st = bmsp.lib().bmsp_spgemm_masked_values(A.h, B.h, M.h, alpha, beta, flags, out.h, None)
    return st, bmsp.lib().bmsp_last_error().decode()


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("dt", range(len(DTYPES)))
def test_values_into_existing_matrices(bmsp, oracle, monkeypatch, dt, lanes):
    name = "random"
    adt, mdt = DTYPES[dt]
    m, n, p, Ac, Bc, Mc = patterns()[name]
    a, b, mv = int_operands(name)
    set_lanes(monkeypatch, lanes)
    for lay in (0, 1):
        A, B = build(bmsp, name, "A", a, lay, adt), build(bmsp, name, "B", b, 1 - lay, adt)
        M = build(bmsp, name, "M", mv, lay, mdt)
        snaps = [snapshot(x) for x in (A, B, M)]
        ref = {(e, lo): bmsp.BmSpMatrix.from_coo(m, p, Mc[0], Mc[1], int_expected(oracle, name, dt, e).astype(np.float64), transposed=lo, dtype=mdt)
               for e in (1, 2, 4) for lo in (0, 1)}

        def same(X, e):
            x, y = X.host_arrays(), ref[(e, X.info()["transposed"])].host_arrays()
            for u, v in zip(x[:3], y[:3]):
                np.testing.assert_array_equal(u, v)
            assert_exact(x[3], y[3])

        first = bmsp.spgemm_masked(A, B, M, *EPILOGUES[1], transposed=1 - lay)
        same(first, 1)
        outs = [M.with_layout(1 - lay), M.with_layout(lay), bmsp.scale(M, transposed=1 - lay), first]
        if adt == mdt:  # (bmsp_sddmm takes dense factors of the pattern's own dtype)
            X = bmsp.DeviceArray.from_host(np.ones(m * 2), NPDT[mdt])
            Y = bmsp.DeviceArray.from_host(np.ones(p * 2), NPDT[mdt])
            outs.append(bmsp.sddmm(M, X, Y, 2, transposed=1 - lay))
        for X in outs:
            for e in (2, 4):
                assert bmsp.spgemm_masked_values(X, A, B, M, *EPILOGUES[e]) is X
                same(X, e)
        for x, s in zip((A, B, M), snaps):
            assert_unchanged(x, s)
        # what the masked product made is accepted by its siblings
        bmsp.scale_values(first, M)
        first.copy_values_from(M)
        assert_same_arrays(first, M.with_layout(1 - lay))
        # refusals: an unrelated handle, a transpose output, out == A, out == B
        other = build(bmsp, name, "M", mv, lay, mdt)
        refused(bmsp, lambda: bmsp.spgemm_masked_values(other, A, B, M), "out")
        refused(bmsp, lambda: bmsp.spgemm_masked_values(M.transpose(lay), A, B, M), "out")
        for x, s in zip((A, B, M), snaps):
            assert_unchanged(x, s)
        # in place
        assert bmsp.spgemm_masked_values(M, A, B, M, *EPILOGUES[2]) is M
        same(M, 2)
        # after invalidate(M, 1) every earlier output is refused; in place needs no history
        M.invalidate(True)
        for X in outs:
            refused(bmsp, lambda: bmsp.spgemm_masked_values(X, A, B, M), "out")
        bmsp.spgemm_masked_values(M, A, B, M, 1.0, 0.0)
        order = np.lexsort((Mc[1], Mc[0]))
        np.testing.assert_array_equal(M.to_coo()[2], int_dots(name)[0][order].astype(np.float64))


@pytest.mark.parametrize("dtype", [F32, F16, F64])
def test_out_aliasing_an_operand_is_refused(bmsp, dtype):
    """the triangle-counting call (M == A == B's pattern) works into a separate output and is refused into A or B"""
    name = "banded"
    m, n, p, Ac, Bc, Mc = patterns()[name]
    a, b, mv = int_operands(name)
    A = build(bmsp, name, "A", a, 0, dtype)
    B = build(bmsp, name, "B", b, 1, dtype)
    snap = snapshot(A)
    for (x, y, mm, out, who) in ((A, B, A, A, "A"), (A, B, B, B, "B"), (A, A, A, A, "A")):
        st, msg = raw_values(bmsp, x, y, mm, out)
        assert st == -1 and "out is " + who in msg, (st, msg)
        with pytest.raises(ValueError):
            bmsp.spgemm_masked_values(out, x, y, mm)
    assert_unchanged(A, snap)
    # M == A == B, one handle, a separate output: (A * A) on A's pattern
    T = bmsp.spgemm_masked(A, A, A)
    d = (dense_of(m, n, Ac, a) @ dense_of(m, n, Ac, a))[Ac[0], Ac[1]]
    order = np.lexsort((Ac[1], Ac[0]))
    np.testing.assert_array_equal(T.to_coo()[2], d[order])
    bmsp.spgemm_masked_values(T, A, A, A, 2.0)
    np.testing.assert_array_equal(T.to_coo()[2], 2.0 * d[order])
    assert_unchanged(A, snap)


def test_square_transpose_output_is_refused(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(8, 4)
    S = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    W = S.with_layout(1)
    refused(bmsp, lambda: bmsp.spgemm_masked_values(S.transpose(0), W, W, S), "out")
    refused(bmsp, lambda: bmsp.spgemm_masked_values(S.transpose(1), W, W, S), "out")


@pytest.mark.parametrize("dtype", [F32, F16, F64])
def test_value_updates_and_a_rebuilt_view(bmsp, dtype):
    """B's values written in place need no invalidate (the view holds structure only); after a structural change and invalidate(B, 1)
    the view is rebuilt"""
    name = "dense"  # B is 40 x 24: every bitmap position of every tile lies inside the matrix
    m, n, p, Ac, Bc, Mc = patterns()[name]
    a, b, mv = int_operands(name)
    Ad = dense_of(m, n, Ac, a)
    order = np.lexsort((Mc[1], Mc[0]))
    for lay in (0, 1):
        A, M = build(bmsp, name, "A", a, 1 - lay, dtype), build(bmsp, name, "M", mv, lay, dtype)
        B = build(bmsp, name, "B", b, lay, dtype)
        out = bmsp.spgemm_masked(A, B, M)
        np.testing.assert_array_equal(out.to_coo()[2], (Ad @ dense_of(n, p, Bc, b))[Mc[0], Mc[1]][order])
        view = bmsp.spgemm_masked_launch_info(A, B, M)["view_bytes"]
        assert view > 0
        # new values in place, no invalidate
        k, bm, o, v = B.host_arrays()
        dk, dbm, do, dv = B.device_arrays()
        nv = (-v.astype(np.float64) + 1).astype(NPDT[dtype])
        bmsp.check(bmsp.lib().bmsp_memcpy_h2d(dv.ptr, nv.ctypes.data, nv.nbytes))
        br, bc, idx = entries(k, bm, o, lay)
        Bd = np.zeros((n, p))
        Bd[br, bc] = nv[idx].astype(np.float64)
        bmsp.spgemm_masked_values(out, A, B, M)
        np.testing.assert_array_equal(out.to_coo()[2], (Ad @ Bd)[Mc[0], Mc[1]][order])
        # a new structure of the same sizes: every bitmap reversed (the same number of values per tile, so the offsets stand)
        rev = np.array([int(format(int(x), "064b")[::-1], 2) for x in bm], np.uint64)
        assert np.any(rev != bm)
        bmsp.check(bmsp.lib().bmsp_memcpy_h2d(dbm.ptr, rev.ctypes.data, rev.nbytes))
        B.invalidate(True)
        br, bc, idx = entries(k, rev, o, lay)
        Bd = np.zeros((n, p))
        Bd[br, bc] = nv[idx].astype(np.float64)
        out2 = bmsp.spgemm_masked(A, B, M)
        np.testing.assert_array_equal(out2.to_coo()[2], (Ad @ Bd)[Mc[0], Mc[1]][order])
        assert bmsp.spgemm_masked_launch_info(A, B, M)["view_bytes"] == view


@pytest.mark.parametrize("dtype", [F32, F16])
def test_in_place_drops_the_value_caches(bmsp, dtype):
    """after prepare(SPGEMM), a product and an in-place masked product into M, the next product with M equals that of a freshly built
    matrix with the same values"""
    name = "rmat"
    m, n, p, Ac, Bc, Mc = patterns()[name]
    a, b, mv = int_operands(name)
    A, B = build(bmsp, name, "A", a, 0, dtype), build(bmsp, name, "B", b, 1, dtype)
    M = build(bmsp, name, "M", mv, 0, dtype)
    W = M.with_layout(1)
    M.prepare(3)
    bmsp.spgemm(M, W, tc_version=5)
    bmsp.spgemm_masked_values(M, A, B, M, 0.5)
    fresh = build(bmsp, name, "M", 0.5 * int_dots(name)[0], 0, dtype)
    assert_same_arrays(M, fresh)
    P, _ = bmsp.spgemm(M, W, tc_version=5)
    Pf, _ = bmsp.spgemm(fresh, W, tc_version=5)
    assert_same_arrays(P, Pf)


@pytest.mark.parametrize("lanes", ["1", "8"])
def test_asynchronous_behind_a_gated_stream(bmsp, monkeypatch, lanes):
    """with B's view built, both calls on a non-blocking stream return while a timed gate still holds the stream; the results are
    bit-equal to the null-stream results"""
    from stream_gate import Gate, new_stream, destroy_stream
    name, dtype = "banded", F32
    a, b, mv = real_operands(name, dtype)
    A, B, M = build(bmsp, name, "A", a, 0, dtype), build(bmsp, name, "B", b, 0, dtype), build(bmsp, name, "M", mv, 1, dtype)
    set_lanes(monkeypatch, lanes)
    ref = bmsp.spgemm_masked(A, B, M, 1.5, 0.25, transposed=0)  # (builds A's block-row pointer and B's view)
    W = M.with_layout(1)
    bmsp.synchronize()
    s = new_stream()
    gate = Gate().close(s)
    try:
        C0 = bmsp.spgemm_masked(A, B, M, 1.5, 0.25, transposed=0, stream=s.value)
        bmsp.spgemm_masked_values(W, A, B, M, 1.5, 0.25, stream=s.value)
        closed = gate.is_closed()
    finally:
        gate.finish()
        destroy_stream(s)
    assert closed, "the calls returned only after the gate had opened"
    assert_same_arrays(C0, ref)
    assert_same_arrays(W, bmsp.spgemm_masked(A, B, M, 1.5, 0.25, transposed=1))


def test_refusals_with_real_handles(bmsp):
    name = "5x3x7"
    a, b, mv = int_operands(name)
    A, B, M = build(bmsp, name, "A", a, 0, F32), build(bmsp, name, "B", b, 0, F32), build(bmsp, name, "M", mv, 0, F32)
    L = bmsp.lib()
    msg = lambda: L.bmsp_last_error().decode()
    h = C.c_void_p()
    info = bmsp.SpgemmMaskedInfo()
    assert L.bmsp_spgemm_masked(A.h, B.h, M.h, 1.0, 0.0, 0, 0, None, None) == -1 and "out" in msg() and "null" in msg()
    assert L.bmsp_spgemm_masked(None, B.h, M.h, 1.0, 0.0, 0, 0, None, C.byref(h)) == -1 and "A" in msg() and "null" in msg()
    assert L.bmsp_spgemm_masked(A.h, None, M.h, 1.0, 0.0, 0, 0, None, C.byref(h)) == -1 and "B" in msg() and "null" in msg()
    assert L.bmsp_spgemm_masked(A.h, B.h, None, 1.0, 0.0, 0, 0, None, C.byref(h)) == -1 and "M" in msg() and "null" in msg()
    assert L.bmsp_spgemm_masked_values(A.h, B.h, M.h, 1.0, 0.0, 0, None, None) == -1 and "out" in msg() and "null" in msg()
    assert L.bmsp_spgemm_masked_launch_info(A.h, B.h, M.h, 0, None) == -1 and "info" in msg() and "null" in msg()
    assert L.bmsp_spgemm_masked_values(A.h, B.h, M.h, 1.0, 1.0, 1, M.h, None) == -1 and "beta" in msg()
    assert L.bmsp_spgemm_masked_launch_info(A.h, B.h, M.h, 2, C.byref(info)) == -1 and "out_transposed" in msg()
    # shapes that do not chain, a mask of another shape, dtype combinations
    assert L.bmsp_spgemm_masked(A.h, A.h, M.h, 1.0, 0.0, 0, 0, None, C.byref(h)) == -1 and "num_cols" in msg()
    assert L.bmsp_spgemm_masked(A.h, B.h, A.h, 1.0, 0.0, 0, 0, None, C.byref(h)) == -1 and "M is" in msg()
    B16, M16, M64 = build(bmsp, name, "B", b, 0, F16), build(bmsp, name, "M", mv, 0, F16), build(bmsp, name, "M", mv, 0, F64)
    assert L.bmsp_spgemm_masked(A.h, B16.h, M.h, 1.0, 0.0, 0, 0, None, C.byref(h)) == -1 and "dtype" in msg()
    assert L.bmsp_spgemm_masked(A.h, B.h, M16.h, 1.0, 0.0, 0, 0, None, C.byref(h)) == -1 and "dtype" in msg()
    assert L.bmsp_spgemm_masked(A.h, B.h, M64.h, 1.0, 0.0, 0, 0, None, C.byref(h)) == -1 and "dtype" in msg()
    for bad in ((A, B16, M), (A, B, M16), (A, B, M64), (A, A, M), (A, B, A)):
        with pytest.raises(ValueError):
            bmsp.spgemm_masked(*bad)
    panel = M.row_panel(0, 1)
    assert L.bmsp_spgemm_masked_values(A.h, B.h, panel.h, 1.0, 0.0, 0, panel.h, None) == -1 and "view" in msg()


# ---------------------------------------------------------------------------------------------------------
# 5. launch_info on every pattern under the default rule and the switch
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_launch_info_follows_the_rule(bmsp, monkeypatch, name):
    for dt in (0, 2):
        adt, mdt = DTYPES[dt]
        for lay in (0, 1):
            A, B, M = source(bmsp, name, "A", adt, lay), source(bmsp, name, "B", adt, 1 - lay), source(bmsp, name, "M", mdt, lay)
            for lanes in LANES:
                set_lanes(monkeypatch, lanes)
                for o_lay in (0, 1):
                    assert bmsp.spgemm_masked_launch_info(A, B, M, o_lay) == expected_info(bmsp, name, B, M, lanes), (name, lanes)
    set_lanes(monkeypatch, None)
    i = M.info()
    got = bmsp.spgemm_masked_launch_info(A, B, M)
    if i["nnz"] == 0:
        assert got["kernel"] == "none (empty mask)" and got["lanes"] == 0 and got["pairs"] == 0
    else:
        assert got["lanes"] == (8 if i["nnz"] >= FILL_THRESHOLD * i["block_num"] else 1)
    if name == "hub_nomatch":
        assert got["pairs"] == 0
    if name in ("hub300x3", "hub3x300"):
        assert got["pairs"] == 3


def test_cpp_wrapper_runs(tmp_path):
    """tests/cpp_spgemm_masked_check.cpp: bmSparse_mult_masked / bmSparse_mult_masked_values for float, half (both mask types) and
    double on a Laplacian fixture"""
    from conftest import MTX
    from test_spgemm_masked_api import build_cpp_spgemm_masked_check
    exe = str(tmp_path / "cpp_spgemm_masked_check")
    build_cpp_spgemm_masked_check(exe)
    out = subprocess.run([exe, os.path.join(MTX, "laplacian", "9pt_10x10.mtx")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("OK") == 4 and "FAIL" not in out.stdout, out.stdout
