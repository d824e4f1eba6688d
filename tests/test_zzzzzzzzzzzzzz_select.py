"""GPU tests of device-side selection (bmsp_matrix_select_band / bmsp_matrix_select_mask).  The reference of every case is built from
what the test reads back from the device plus numpy: the stored entries of A, the predicate (lo <= col - row <= hi, or membership of the
coordinate in M's stored coordinates) in int64, and the CPU oracle's build of the kept COO in the output layout.  Structure, block-row
pointer and counts must match it exactly and the values must be the bits A holds at the kept coordinates; A and M must come back
unchanged."""
import ctypes as C
import os
import sys
import numpy as np
import pytest
from test_transpose import entries, assert_same_arrays, snapshot, assert_unchanged, _write_values, special_bits
from test_add import stored, check_structure
from test_prune import keep_mask

pytestmark = pytest.mark.gpu

NPDT = {0: np.float32, 1: np.float16, 2: np.float64}
UINT = {0: np.uint32, 1: np.uint16, 2: np.uint64}
MIN, MAX = -(1 << 63), (1 << 63) - 1
NR, NC = 203, 157


def build(bmsp, nr, nc, r, c, v, lay, dtype):
    return bmsp.BmSpMatrix.from_coo(nr, nc, r, c, v, transposed=lay, dtype=dtype)


def in_band(r, c, lo, hi, complement=False):
    """the predicate in int64; Python integers on the right so that +-2^63 - 1 compare without overflow"""
    d = c.astype(np.int64) - r.astype(np.int64)
    keep = (d >= max(lo, -(1 << 62))) & (d <= min(hi, 1 << 62))
    return ~keep if complement else keep


def in_mask(nc, r, c, M, complement=False):
    mr, mc, _ = stored(M)
    keep = np.isin(r.astype(np.int64) * nc + c, mr.astype(np.int64) * nc + mc)
    return ~keep if complement else keep


def kept_entries(P, nc, lay):
    """(sorted linear coordinates, value bits in that order) of a device matrix"""
    k, b, o, pv = P.host_arrays()
    rr, cc, idx = entries(k, b, o, lay)
    lin = rr * nc + cc
    order = np.argsort(lin)
    return lin[order], pv[idx][order].view(UINT[P.info()["dtype"]])


def check_set(A_ent, nc, keep, P, st, lay):
    """P's entries as a set of (row, col, value bits) against the kept entries of A; the counts"""
    r, c, v = A_ent
    want = r[keep].astype(np.int64) * nc + c[keep]
    order = np.argsort(want)
    lin, bits = kept_entries(P, nc, lay)
    np.testing.assert_array_equal(lin, want[order])
    np.testing.assert_array_equal(bits, v[keep][order].view(bits.dtype))
    assert (st["nnz_in"], st["nnz_out"]) == (r.size, int(keep.sum())), st
    assert (P.nnz, P.block_num, P.info()["transposed"]) == (st["nnz_out"], st["blocks_out"], lay)


def check_full(oracle, A, A_ent, keep, P, st, lay):
    """P against the oracle's build of the kept COO: four arrays, block-row pointer, stats; values as A's bits"""
    i = A.info()
    nr, nc, dtype = i["num_rows"], i["num_cols"], i["dtype"]
    r, c, v = A_ent
    with np.errstate(all="ignore"):
        ref = oracle.bmsp_from_coo(oracle.Coo(nr, nc, r[keep], c[keep], v[keep].astype(np.float64)), dtype, lay)
    check_structure(P, ref)
    assert P.info()["dtype"] == dtype
    assert st == {"nnz_in": i["nnz"], "nnz_out": int(keep.sum()), "blocks_in": i["block_num"], "blocks_out": ref.block_num}, st
    assert P.host_arrays()[2].size == ref.block_num + 1
    check_set(A_ent, nc, keep, P, st, lay)
    return ref


def check_band(oracle, bmsp, A, A_ent, lo, hi, complement, lay):
    snap = snapshot(A)
    P, st = bmsp.select_band(A, lo, hi, complement, transposed=lay)
    assert_unchanged(A, snap)
    keep = in_band(A_ent[0], A_ent[1], lo, hi, complement)
    return P, keep, check_full(oracle, A, A_ent, keep, P, st, lay)


def check_mask(oracle, bmsp, A, A_ent, M, complement, lay):
    snaps = snapshot(A), snapshot(M)
    P, st = bmsp.select_mask(A, M, complement, transposed=lay)
    assert_unchanged(A, snaps[0])
    assert_unchanged(M, snaps[1])
    keep = in_mask(A.info()["num_cols"], A_ent[0], A_ent[1], M, complement)
    return P, keep, check_full(oracle, A, A_ent, keep, P, st, lay)


def random_a():
    from pybmsp import gen
    _, _, r, c, v = gen.random_coo(NR, NC, NR * 26, seed=3)
    assert r.size == 4855
    return r, c, v


# ---------------------------------------------------------------------------------------------------------
# 1. band sweep: every in-tile diagonal offset on a full small matrix
# ---------------------------------------------------------------------------------------------------------
FULL_BANDS = [(lo, hi) for lo, hi in [(-10, 10), (-10, -10), (10, 10), (0, 0), (-1, 1), (-7, 7), (-8, 8), (-9, 9), (1, 0), (5, 4), (10, -10),
                                      (-10, 0), (0, 10), (-10, -1), (1, 10), (-3, 5), (-5, 3), (7, 7), (-7, -7), (8, 8), (-8, -8), (9, 10),
                                      (-10, -9), (-6, -2), (2, 6), (-4, 0), (0, 4), (-9, -8), (8, 9), (3, 3), (-2, -2), (-8, 0), (0, 8),
                                      (-8, 7), (-7, 8), (4, 9), (-9, -4), (-1, 0), (0, 1), (6, 10)]]


@pytest.mark.parametrize("lin", [0, 1])
@pytest.mark.parametrize("lout", [0, 1])
def test_band_sweep_on_a_full_matrix(oracle, bmsp, lin, lout):
    """19 x 13 with every coordinate stored: block distances -2 .. 1, every (lo, hi) in [-10, 10]^2 (lo > hi and bands that empty tiles
    included), complement off and on, as sets of (row, col, value bits); a fixed list of 40 bands against the oracle's arrays too"""
    nr, nc = 19, 13
    r, c = np.repeat(np.arange(nr), nc), np.tile(np.arange(nc), nr)
    v = (1.0 + np.arange(nr * nc)) / 8.0
    A = build(bmsp, nr, nc, r, c, v, lin, 0)
    A_ent = stored(A)
    snap = snapshot(A)
    assert len(FULL_BANDS) == 40
    for lo in range(-10, 11):
        for hi in range(-10, 11):
            for comp in (False, True):
                P, st = bmsp.select_band(A, lo, hi, comp, transposed=lout)
                keep = in_band(A_ent[0], A_ent[1], lo, hi, comp)
                check_set(A_ent, nc, keep, P, st, lout)
                if (lo, hi) in FULL_BANDS:
                    check_full(oracle, A, A_ent, keep, P, st, lout)
    assert_unchanged(A, snap)


# ---------------------------------------------------------------------------------------------------------
# 2. band on a random matrix: dtypes x layouts, the stated shares
# ---------------------------------------------------------------------------------------------------------
BANDS = [((MIN, 0), 0.613, 329), ((0, MAX), 0.391, 210), ((MIN, -1), 0.609, None), ((1, MAX), 0.387, None), ((-20, 20), 0.191, 121),
         ((-3, 5), 0.041, 45), ((0, 0), 0.004, 12), ((9, 40), 0.134, None), ((-40, -9), 0.161, None)]


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_band_on_a_random_matrix(oracle, bmsp, dtype):
    r, c, v = random_a()
    for lin in (0, 1):
        A = build(bmsp, NR, NC, r, c, v, lin, dtype)
        assert A.block_num == 519
        A_ent = stored(A)
        for lout in (0, 1):
            for (lo, hi), share, tiles in BANDS:
                P, keep, ref = check_band(oracle, bmsp, A, A_ent, lo, hi, False, lout)
                assert abs(keep.mean() - share) <= 0.02, ((lo, hi), keep.mean())
                assert tiles is None or ref.block_num == tiles, ((lo, hi), ref.block_num)
            W = A.with_layout(lout)
            for lo, hi in ((-(1 << 62), 1 << 62), (MIN, MAX)):
                P, keep, _ = check_band(oracle, bmsp, A, A_ent, lo, hi, False, lout)
                assert keep.all()
                assert_same_arrays(P, W)
                np.testing.assert_array_equal(P.block_row_ptr(), W.block_row_ptr())
            P, keep, _ = check_band(oracle, bmsp, A, A_ent, 5, 4, False, lout)
            assert (P.block_num, P.nnz) == (0, 0) and P.host_arrays()[2].tolist() == [0]
            P, keep, _ = check_band(oracle, bmsp, A, A_ent, MIN, MAX, True, lout)
            assert P.block_num == 0


# ---------------------------------------------------------------------------------------------------------
# 3. lanes per tile of the place pass
# ---------------------------------------------------------------------------------------------------------
def test_lane_groups_give_the_same_arrays(oracle, bmsp, monkeypatch):
    from pybmsp import gen
    n, _, br, bc, bv = gen.banded(256, 24)
    r, c, v = random_a()
    cases = [(build(bmsp, n, n, br, bc, bv, 0, 0), (-5, 11)), (build(bmsp, NR, NC, r, c, v, 1, 2), (-20, 20))]
    M = build(bmsp, n, n, br[::2], bc[::2], bv[::2], 1, 1)
    for A, (lo, hi) in cases:
        A_ent = stored(A)
        outs = []
        for lanes in ("1", "8"):
            monkeypatch.setenv("BMSP_SELECT_LANES", lanes)
            for lout in (0, 1):
                outs.append(check_band(oracle, bmsp, A, A_ent, lo, hi, False, lout)[0])
                outs.append(check_band(oracle, bmsp, A, A_ent, lo, hi, True, lout)[0])
                if A.info()["num_rows"] == n:
                    outs.append(check_mask(oracle, bmsp, A, A_ent, M, False, lout)[0])
        half = len(outs) // 2
        for a, b in zip(outs[:half], outs[half:]):
            assert_same_arrays(a, b)


# ---------------------------------------------------------------------------------------------------------
# 4. round trips through addition and pruning
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_round_trips(bmsp, dtype):
    from pybmsp import gen
    r, c, v = random_a()
    _, _, mr, mc, mv = gen.random_coo(NR, NC, NR * 110, seed=11)
    for lin in (0, 1):
        A = build(bmsp, NR, NC, r, c, v, lin, dtype)
        M = build(bmsp, NR, NC, mr, mc, mv, 1 - lin, 0)
        for lout in (0, 1):
            W = A.with_layout(lout)
            assert_same_arrays(bmsp.add(bmsp.tril(A, -1), bmsp.triu(A, 0, transposed=1 - lin), transposed=lout), W)
            for lo, hi in ((-3, 5), (-40, -9), (0, 0)):
                assert_same_arrays(bmsp.add(A.band(lo, hi), A.band(lo, hi, complement=True, transposed=lout), transposed=lout), W)
            assert_same_arrays(bmsp.add(A.mask(M, transposed=lout), A.mask(M, complement=True), transposed=lout), W)
            assert_same_arrays(bmsp.add(bmsp.offdiagonal(A), A.band(0, 0), transposed=lout), W)
            # tril(A) is the pruning of A with its upper values overwritten by 0
            Z = A.with_layout(lin)
            zr, zc, zidx = entries(*Z.host_arrays()[:3], lin)
            hv = Z.host_arrays()[3].copy()
            hv[zidx[zc > zr]] = 0
            _write_values(bmsp, Z, hv)
            Z.invalidate(False)
            assert_same_arrays(bmsp.tril(A, transposed=lout), bmsp.prune(Z, 0.0, transposed=lout)[0])


# ---------------------------------------------------------------------------------------------------------
# 5. values move as raw bits; the predicate never looks at them
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_values_move_as_raw_bits(oracle, bmsp, dtype):
    rng = np.random.default_rng(70 + dtype)
    r, c, v = random_a()
    for lin in (0, 1):
        A = build(bmsp, NR, NC, r, c, v, lin, dtype)
        bits = special_bits(dtype, A.nnz, rng)
        _write_values(bmsp, A, bits.view(NPDT[dtype]))
        A.invalidate(False)
        np.testing.assert_array_equal(A.host_arrays()[3].view(UINT[dtype]), bits)
        A_ent = stored(A)
        for lo, hi in ((MIN, 0), (-20, 20)):
            keep = in_band(A_ent[0], A_ent[1], lo, hi)
            for side in (keep, ~keep):  # NaNs with payloads, infinities, -0 and subnormals inside and outside the band
                with np.errstate(all="ignore"):
                    f = A_ent[2][side].astype(np.float64)
                assert np.isnan(f).any() and np.isinf(f).any() and (np.signbit(f) & (f == 0)).any()
                assert ((f != 0) & (np.abs(f) < float(np.finfo(NPDT[dtype]).tiny))).any()
            for lout in (0, 1):
                for comp in (False, True):
                    check_band(oracle, bmsp, A, A_ent, lo, hi, comp, lout)
        check_mask(oracle, bmsp, A, A_ent, bmsp.tril(A, 3, transposed=1 - lin), False, 1 - lin)


# ---------------------------------------------------------------------------------------------------------
# 6. masks
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adt,mdt", [(2, 1), (1, 0), (0, 0)])
def test_mask_on_random_matrices(oracle, bmsp, adt, mdt):
    from pybmsp import gen
    r, c, v = random_a()
    for mul, share in ((110, 0.498), (60, 0.318)):
        _, _, mr, mc, mv = gen.random_coo(NR, NC, NR * mul, seed=11)
        for la in (0, 1):
            A = build(bmsp, NR, NC, r, c, v, la, adt)
            A_ent = stored(A)
            for lm in (0, 1):
                M = build(bmsp, NR, NC, mr, mc, mv, lm, mdt)
                for lout in (0, 1):
                    P, keep, _ = check_mask(oracle, bmsp, A, A_ent, M, False, lout)
                    assert abs(keep.mean() - share) <= 0.02, keep.mean()
                    check_mask(oracle, bmsp, A, A_ent, M, True, lout)


def test_mask_of_a_sparse_pair(oracle, bmsp):
    """tiles only in A, only in M and shared; few shared coordinates; both ways and complemented"""
    from pybmsp import gen
    _, _, ar, ac, av = gen.random_coo(NR, NC, 609, seed=5)
    _, _, br, bc, bv = gen.random_coo(NR, NC, 609, seed=6)
    ta, tb = np.unique((ar // 8) * 1000 + ac // 8), np.unique((br // 8) * 1000 + bc // 8)
    assert (np.setdiff1d(ta, tb).size, np.setdiff1d(tb, ta).size, np.intersect1d(ta, tb).size) == (96, 112, 258)
    for la in (0, 1):
        for lm in (0, 1):
            A, B_ = build(bmsp, NR, NC, ar, ac, av, la, 0), build(bmsp, NR, NC, br, bc, bv, lm, 2)
            for X, Y in ((A, B_), (B_, A)):
                X_ent = stored(X)
                for lout in (0, 1):
                    P, keep, _ = check_mask(oracle, bmsp, X, X_ent, Y, False, lout)
                    assert int(keep.sum()) == 11
                    check_mask(oracle, bmsp, X, X_ent, Y, True, lout)


def test_mask_edge_patterns(oracle, bmsp):
    r, c, v = random_a()
    none = np.zeros(0, np.int64)
    for la in (0, 1):
        A = build(bmsp, NR, NC, r, c, v, la, 0)
        A_ent = stored(A)
        E = build(bmsp, NR, NC, none, none, np.zeros(0), 1 - la, 1)
        Z = build(bmsp, NR, NC, r, c, np.zeros(v.size), 1 - la, 2)  # A's pattern, every value a stored zero
        assert (E.block_num, Z.nnz) == (0, A.nnz)
        for lout in (0, 1):
            W = A.with_layout(lout)
            assert_same_arrays(check_mask(oracle, bmsp, A, A_ent, A, False, lout)[0], W)
            assert check_mask(oracle, bmsp, A, A_ent, A, True, lout)[0].block_num == 0
            P = check_mask(oracle, bmsp, A, A_ent, E, False, lout)[0]
            assert P.block_num == 0 and P.host_arrays()[2].tolist() == [0]
            assert_same_arrays(check_mask(oracle, bmsp, A, A_ent, E, True, lout)[0], W)
            assert_same_arrays(check_mask(oracle, bmsp, A, A_ent, Z, False, lout)[0], W)
            assert check_mask(oracle, bmsp, E, stored(E), A, False, lout)[0].block_num == 0


def test_mask_search_in_a_long_block_row(oracle, bmsp):
    """8 x 40 000 with one block-row of 5 000 tiles against an M that stores every third column"""
    nr, nc = 8, 40000
    col = np.arange(nc)
    ar, ac = np.concatenate([(col * 5) % 8, (col * 3 + 1) % 8]), np.concatenate([col, col])
    A = build(bmsp, nr, nc, ar, ac, 1.0 + np.arange(ar.size) % 97, 0, 0)
    assert A.block_num == 5000
    third = col[col % 3 == 0]
    M = build(bmsp, nr, nc, np.tile(np.arange(8), third.size), np.repeat(third, 8), np.ones(8 * third.size), 1, 1)
    A_ent = stored(A)
    for lout in (0, 1):
        for comp in (False, True):
            P, keep, _ = check_mask(oracle, bmsp, A, A_ent, M, comp, lout)
            assert abs(keep.mean() - (2 / 3 if comp else 1 / 3)) < 0.01
    S = build(bmsp, nr, nc, np.zeros(1700, np.int64), col[5::23][:1700], np.ones(1700), 0, 0)  # a sparser M: tiles missing from the row
    check_mask(oracle, bmsp, A, A_ent, S, False, 0)
    check_mask(oracle, bmsp, A, A_ent, S, True, 1)


# ---------------------------------------------------------------------------------------------------------
# 7. count only, refusals on live handles
# ---------------------------------------------------------------------------------------------------------
def test_count_only_equals_the_real_call(bmsp):
    from pybmsp import gen
    r, c, v = random_a()
    _, _, mr, mc, mv = gen.random_coo(NR, NC, NR * 60, seed=11)
    for dtype in (0, 1, 2):
        for lin in (0, 1):
            A, M = build(bmsp, NR, NC, r, c, v, lin, dtype), build(bmsp, NR, NC, mr, mc, mv, 1, 0)
            for lo, hi, comp in ((None, 0, False), (0, None, True), (-3, 5, False), (5, 4, False), (0, 0, True)):
                P, st = bmsp.select_band(A, lo, hi, comp)
                assert bmsp.band_count(A, lo, hi, comp) == st and (P.nnz, P.block_num) == (st["nnz_out"], st["blocks_out"])
            for comp in (False, True):
                P, st = bmsp.select_mask(A, M, comp)
                assert bmsp.mask_count(A, M, comp) == st and (P.nnz, P.block_num) == (st["nnz_out"], st["blocks_out"])
    # stats == NULL with an output
    h = C.c_void_p()
    bmsp.check(bmsp.lib().bmsp_matrix_select_band(A.h, -3, 5, 0, 1, None, C.byref(h), None))
    P = bmsp.BmSpMatrix(h.value)
    assert P.nnz == bmsp.band_count(A, -3, 5)["nnz_out"] and P.info()["transposed"] == 1


def test_refusals_on_real_handles(bmsp):
    r, c, v = random_a()
    A = build(bmsp, NR, NC, r, c, v, 0, 0)

    def refused(fn, word):
        with pytest.raises(bmsp.BmspError) as e:
            fn()
        assert e.value.status == -1 and word in str(e.value), str(e.value)

    for nr, nc in ((NR + 1, NC), (NR, NC - 1), (NC, NR)):
        keep = (r < nr) & (c < nc)
        M = build(bmsp, nr, nc, r[keep], c[keep], v[keep], 0, 0)
        refused(lambda: bmsp.select_mask(A, M), "shape")
        refused(lambda: bmsp.mask_count(M, A), "shape")
    V = A.row_panel(3, 9)
    refused(lambda: bmsp.select_band(V, 0, 0), "view")
    refused(lambda: bmsp.band_count(V, 0, 0), "view")
    refused(lambda: bmsp.select_mask(V, V), "view")
    L = bmsp.lib()
    h, st = C.c_void_p(), bmsp.SelectStats()
    for flags, lay, word in ((2, 0, "flags"), (-1, 0, "flags"), (0, 2, "out_transposed")):
        assert L.bmsp_matrix_select_band(A.h, 0, 0, flags, lay, None, C.byref(h), C.byref(st)) == -1 and word in L.bmsp_last_error().decode()
        assert L.bmsp_matrix_select_mask(A.h, A.h, flags, lay, None, C.byref(h), C.byref(st)) == -1 and word in L.bmsp_last_error().decode()
    assert L.bmsp_matrix_select_mask(A.h, None, 0, 0, None, C.byref(h), C.byref(st)) == -1 and "M" in L.bmsp_last_error().decode()
    assert h.value is None


# ---------------------------------------------------------------------------------------------------------
# 8. the output is a complete matrix for the operators
# ---------------------------------------------------------------------------------------------------------
def test_product_of_a_selected_matrix(bmsp):
    from pybmsp import gen
    n = 150
    _, _, r, c, v = gen.random_coo(n, n, n * 20, seed=4)
    _, _, br, bc, bv = gen.random_coo(n, n, n * 12, seed=9)
    A, B_ = build(bmsp, n, n, r, c, v, 0, 0), build(bmsp, n, n, br, bc, bv, 1, 0)
    k = c <= r
    want, wst = bmsp.spgemm(build(bmsp, n, n, r[k], c[k], v[k], 0, 0), B_, tc_version=5)
    got, gst = bmsp.spgemm(bmsp.tril(A), B_, tc_version=5)
    assert_same_arrays(got, want)
    assert gst["c_nnz"] == wst["c_nnz"] and gst["surviving_tasks"] == wst["surviving_tasks"]
    x = bmsp.DeviceArray.from_host(gen.spmv_x(n, "cusp"))
    np.testing.assert_array_equal(bmsp.spmv(bmsp.triu(A, 1), x).to_host().view(np.uint32),
                                  bmsp.spmv(build(bmsp, n, n, r[~k], c[~k], v[~k], 0, 0), x).to_host().view(np.uint32))


# ---------------------------------------------------------------------------------------------------------
# 9. streams
# ---------------------------------------------------------------------------------------------------------
def _mask_operand(bmsp, o, S, alt, dtype):
    import test_streams as TS
    o.M = bmsp.tril(TS.mat(bmsp, S, alt, 1, lay=True, salt=1), 2)  # (its values are never read: not an input)


@pytest.mark.parametrize("which", ["band", "mask"])
def test_select_behind_a_gate_on_a_non_blocking_stream(bmsp, monkeypatch, which):
    """A's real values arrive on the stream behind a closed gate: the call must run behind them, synchronise, and give the bits of the
    null-stream call"""
    import test_streams as TS
    if which == "band":
        case = TS.derived_case("select_band", TS.SYNC, "rmat10", 0, {}, lambda bmsp, o, st: bmsp.select_band(o.A, -20, 20, transposed=1, stream=st)[0])
    else:
        case = TS.derived_case("select_mask", TS.SYNC, "rmat10", 2, {}, lambda bmsp, o, st: bmsp.select_mask(o.A, o.M, True, stream=st)[0],
                               operands=_mask_operand)
    assert TS.run_gated(bmsp, monkeypatch, case) == TS.SYNC


# ---------------------------------------------------------------------------------------------------------
# 10. the caller that existed: fsai_pattern
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta", [0.0, 0.05])
def test_fsai_pattern_without_torch(oracle, bmsp, monkeypatch, theta):
    """the lower triangle of the pruned matrix, as the oracle builds it from the COO; no torch in sight"""
    from pybmsp import gen
    monkeypatch.setitem(sys.modules, "torch", None)
    with pytest.raises(ImportError):
        import torch  # noqa: F401
    n, _, r, c, v = gen.poisson("27pt", 6, 6, 6)
    for lin in (0, 1):
        A = build(bmsp, n, n, r, c, v, lin, 0)
        ar, ac, av = stored(A)
        keep = keep_mask(n, ar, ac, av, theta, "row_rel", True) if theta > 0 else np.ones(ar.size, bool)
        keep &= ac <= ar
        for lay in (None, 0, 1):
            S = bmsp.fsai_pattern(A, theta, transposed=lay)
            out = lin if lay is None else lay
            ref = oracle.bmsp_from_coo(oracle.Coo(n, n, ar[keep], ac[keep], av[keep].astype(np.float64)), 0, out)
            check_structure(S, ref)
            np.testing.assert_array_equal(S.host_arrays()[3].view(np.uint32), ref.values.astype(np.float32).view(np.uint32))


def test_cpp_wrappers_run(bmsp, tmp_path):
    """tests/cpp_select_check.cpp: bmSpMatrix<T>::tril / ::triu / ::band / ::mask and bmSparse_select_* on the data/real fixture"""
    import subprocess
    from conftest import MTX
    from test_select_api import build_cpp_select_check
    exe = str(tmp_path / "cpp_select_check")
    build_cpp_select_check(exe)
    out = subprocess.run([exe, os.path.join(MTX, "real", "A_matrix.mtx")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    for word in ("CHECK select triangles OK", "CHECK select band OK", "CHECK select mask OK", "CHECK half OK"):
        assert word in out.stdout, out.stdout
