"""GPU tests of bmsp_matrix_fsai / bmsp_matrix_fsai_values and the bmsp_fsai_t handle (the reference is tests/fsai_ref.c through
tests/test_fsai_api.py, which also owns the inputs and their self-checks).  G is compared with the reference bit for bit unless stated.

1. lane classes: every longest row at which W changes, both dtypes, both ops, the three scales, every layout combination; the pivot;
   info; BMSP_FSAI_LANES=64 gives the same bits.
2. sizes and walks: n = 0, 1, 13, 70; block columns far apart; a hub row of A under a short P; columns A does not store; stored zeros.
3. special values.  4. refill.  5. operands unchanged.  6. refusals on real handles.
7. the handle: COLMAJOR applications are the test's own two bmsp_spmv_op calls bit for bit; row-major factors stay within the a-priori
   bound of two recursive sums; update.
8. solves: bit for bit against the restatements on a column-major A; convergence in fewer iterations than Jacobi; breakdown; n = 0.
9. a gated stream.  10. the C++ wrapper against the ctypes result."""
import ctypes as C
import subprocess
import numpy as np
import pytest
from test_spsv_api import VEC, NP, assert_same_bits
from test_transpose import snapshot, assert_unchanged
from test_krylov_api import restate, NO_CHECK, MAXITER, CONVERGED, BREAKDOWN
from test_gmres_api import restate_gmres
from test_zzzzz_krylov import same_as_restatement, refused
import test_fsai_api as F
from test_fsai_api import NONE, SQRT, UNIT, LONGEST, reference

pytestmark = pytest.mark.gpu
SCALES = {NONE: "none", SQRT: "sqrt", UNIT: "unit"}


def dev(bmsp, a):
    return bmsp.DeviceArray.from_host(np.ascontiguousarray(a))


def mat(bmsp, A, dtype, lay=0):
    return bmsp.BmSpMatrix.from_coo(A[0], A[0], A[1], A[2], A[3], transposed=bool(lay), dtype=dtype)


def pat(bmsp, S, lay=0, dtype=0):
    return bmsp.BmSpMatrix.from_coo(S[0], S[0], S[1], S[2], np.full(S[1].size, 3.0), transposed=bool(lay), dtype=dtype)


def values_of(G, S, dtype):
    """G's values in S's (row, col) order, after checking that G stores exactly S's coordinates"""
    r, c, v = G.to_coo()
    o = np.lexsort((c, r))
    assert np.array_equal(r[o], S[1]) and np.array_equal(c[o], S[2]), "G does not have S's pattern"
    return v[o].astype(VEC[dtype])


def lanes_rule(longest):
    w = 8
    while w < longest:
        w *= 2
    return w


def check_factor(bmsp, A, S, dtype, op, scale, lays=(0, 0, 0), dA=None, dS=None, msg=""):
    dA = dA or mat(bmsp, A, dtype, lays[0])
    dS = dS or pat(bmsp, S, lays[1])
    G, info, piv = bmsp.fsai(dA, dS, op, SCALES[scale], lays[2], pivot=True)
    g, p, bad = reference(A, S, dtype, op, scale)
    gi = G.info()
    assert (gi["dtype"], gi["transposed"], gi["nnz"], gi["num_rows"]) == (dtype, lays[2], S[1].size, S[0]), gi
    assert_same_bits(values_of(G, S, dtype), g, "G %s" % msg)
    assert_same_bits(piv.to_host(), p, "pivot %s" % msg)
    assert info["bad_rows"] == bad, (info, bad, msg)
    return G, info


# ---------------------------------------------------------------------------------------------------------
# 1. lane classes
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 2])
@pytest.mark.parametrize("longest", LONGEST)
def test_lane_classes_equal_the_reference_bit_for_bit(bmsp, monkeypatch, longest, dtype):
    monkeypatch.delenv("BMSP_FSAI_LANES", raising=False)
    A, S = F.dominant(200, 0.3, 11, dtype), F.lane_pattern(200, longest)
    dA, dS = mat(bmsp, A, dtype), pat(bmsp, S)
    lens = F.row_lengths(S).astype(np.int64)
    for op in ("N", "T"):
        for scale in (NONE, SQRT, UNIT):
            G, info = check_factor(bmsp, A, S, dtype, op, scale, dA=dA, dS=dS, msg="%s %d" % (op, scale))
            W = lanes_rule(longest)
            es = 8 if dtype == 2 else 4
            assert (info["lanes"], info["rows"], info["max_row"], info["pairs"]) == (W, 200, longest, int((lens * lens).sum())), info
            assert info["kernel"] == "fsai_row_kernel<%s, %d>" % ("F64" if dtype == 2 else "F32", W)
            assert info["lds_bytes"] == es * 64 * (W + 1) + es * 64 + 4 * 64 and info["bad_rows"] == 0
    want = values_of(bmsp.fsai(dA, dS, "T", "sqrt")[0], S, dtype)
    monkeypatch.setenv("BMSP_FSAI_LANES", "64")
    G, info = bmsp.fsai(dA, dS, "T", "sqrt")
    assert info["lanes"] == 64
    assert_same_bits(values_of(G, S, dtype), want, "BMSP_FSAI_LANES=64")
    monkeypatch.setenv("BMSP_FSAI_LANES", "8")          # a smaller W than the rule's is never taken
    assert bmsp.fsai(dA, dS, "T", "sqrt")[1]["lanes"] == lanes_rule(longest)


@pytest.mark.parametrize("lays", [(a, s, o) for a in (0, 1) for s in (0, 1) for o in (0, 1)])
def test_every_layout_combination(bmsp, lays):
    for dtype, op, scale in ((0, "N", SQRT), (2, "T", UNIT)):
        check_factor(bmsp, F.dominant(200, 0.3, 11, dtype), F.lane_pattern(200, 17), dtype, op, scale, lays, msg=str(lays))


# ---------------------------------------------------------------------------------------------------------
# 2. sizes and walks
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 13, 70])
def test_small_sizes(bmsp, n):
    for dtype in (0, 2):
        A = F.dominant(n, 0.5, 31, dtype) if n else (0, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))
        S = F.lower_of(A)
        S = (n, S[1], S[2])
        if n == 70:
            S = F.lane_pattern(70, 33)
        for op, scale in (("N", SQRT), ("T", NONE)):
            G, info = check_factor(bmsp, A, S, dtype, op, scale, msg="n %d" % n)
            assert info["rows"] == n
            if n == 0:
                assert info["kernel"].startswith("none") and info["bad_rows"] == 0


@pytest.mark.parametrize("case", ["far", "hub", "mismatch"])
@pytest.mark.parametrize("dtype", [0, 2])
def test_walks(bmsp, case, dtype):
    A, S = {"far": F.far_case, "hub": F.hub_case, "mismatch": F.mismatch_case}[case](dtype)
    dA = [mat(bmsp, A, dtype, lay) for lay in (0, 1)]
    dS = pat(bmsp, S)
    if case == "mismatch":
        assert dA[0].info()["nnz"] == A[1].size      # the stored zeros are stored
    for lay in (0, 1):
        for op, scale in (("N", SQRT), ("T", UNIT)):
            check_factor(bmsp, A, S, dtype, op, scale, (lay, 0, lay), dA=dA[lay], dS=dS, msg="%s lay %d %s" % (case, lay, op))


# ---------------------------------------------------------------------------------------------------------
# 3. special values
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 2])
@pytest.mark.parametrize("kind", F.SPECIALS)
def test_special_values(bmsp, kind, dtype):
    A, S = F.special_case(kind, dtype)
    for op in ("N", "T"):
        for scale in (NONE, SQRT, UNIT):
            G, info = check_factor(bmsp, A, S, dtype, op, scale, msg="%s %s %d" % (kind, op, scale))
            if scale == SQRT and op == "N":
                assert info["bad_rows"] >= 3, info


# ---------------------------------------------------------------------------------------------------------
# 4. refill; 5. operands unchanged
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 2])
def test_refill_after_a_value_update(bmsp, dtype):
    A, S = F.dominant(200, 0.3, 11, dtype), F.lane_pattern(200, 17)
    dA, dS = mat(bmsp, A, dtype), pat(bmsp, S)
    x = dev(bmsp, F.solve_rhs(200, dtype))
    for lay in (0, 1):
        G, _ = bmsp.fsai(dA, dS, "N", "sqrt", lay)
        bmsp.spmv_op(G, x, "N"); bmsp.spmv_op(G, x, "T")                 # the caches a product keeps on G
        left = dev(bmsp, (1.0 + (np.arange(200) % 4) / 4.0).astype(VEC[dtype]))
        B = dA.scale(left)                                              # new values, the same structure
        Bh = (A[0], A[1], A[2], A[3] * (1.0 + (A[1] % 4) / 4.0))
        _, info, piv = bmsp.fsai_values(B, G, "N", "sqrt", pivot=True)
        fresh, finfo = bmsp.fsai(B, dS, "N", "sqrt", lay)
        g, p, bad = reference(Bh, S, dtype, "N", SQRT)
        assert_same_bits(values_of(G, S, dtype), g, "refilled")
        assert_same_bits(values_of(fresh, S, dtype), g, "fresh")
        assert_same_bits(piv.to_host(), p)
        assert info == finfo
        for op in ("N", "T"):
            assert_same_bits(bmsp.spmv_op(G, x, op).to_host(), bmsp.spmv_op(fresh, x, op).to_host(), "product on the refilled G, op " + op)
    # a G of another legal pattern: a pattern matrix of A's dtype, built by hand
    S2 = F.lane_pattern(200, 9)
    G2 = pat(bmsp, S2, 1, dtype)
    bmsp.fsai_values(dA, G2, "T", "unit")
    assert_same_bits(values_of(G2, S2, dtype), reference(A, S2, dtype, "T", UNIT)[0], "another pattern")


def test_operands_unchanged_and_a_second_call_gives_the_same_bits(bmsp):
    A, S = F.dominant(200, 0.3, 11, 0), F.lane_pattern(200, 33)
    for lays in ((0, 0), (1, 1), (0, 1)):
        dA, dS = mat(bmsp, A, 0, lays[0]), pat(bmsp, S, lays[1], 2)      # (S's dtype is ignored)
        sa, ss = snapshot(dA), snapshot(dS)
        first = values_of(bmsp.fsai(dA, dS, "T", "unit")[0], S, 0)
        again = values_of(bmsp.fsai(dA, dS, "T", "unit")[0], S, 0)
        assert_same_bits(first, again)
        f = bmsp.Fsai(dA, dS, "general")
        f.apply(dev(bmsp, F.solve_rhs(200, 0)))
        assert_unchanged(dA, sa)
        assert_unchanged(dS, ss)


# ---------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------
def test_refusals_on_real_handles(bmsp):
    A, S = F.dominant(70, 0.3, 5, 0), F.lane_pattern(70, 9)
    dA, dS = mat(bmsp, A, 0), pat(bmsp, S)
    L = bmsp.lib()
    info, out = bmsp.FsaiInfo(), C.c_void_p(0x5a5a)

    def raw(a, op, s, scale, lay, o=out, i=info):
        return L.bmsp_matrix_fsai(a, op, s, scale, lay, None, None, C.byref(o) if o is not None else None, C.byref(i) if i is not None else None)

    for args, word in (((dA.h, 2, dS.h, 1, 0), "op"), ((dA.h, 0, dS.h, 3, 0), "scale"), ((dA.h, 0, dS.h, 1, 5), "out_transposed")):
        assert raw(*args) == -1 and L.bmsp_last_error().decode().startswith(word)
    assert raw(None, 0, dS.h, 1, 0) == -1 and "matrix A" in L.bmsp_last_error().decode()
    assert raw(dA.h, 0, None, 1, 0) == -1 and "matrix S" in L.bmsp_last_error().decode()
    assert raw(dA.h, 0, dS.h, 1, 0, o=None) == -1 and "out" in L.bmsp_last_error().decode()
    assert raw(dA.h, 0, dS.h, 1, 0, i=None) == -1 and "info" in L.bmsp_last_error().decode()
    assert L.bmsp_matrix_fsai_values(dA.h, 0, None, 1, None, None, C.byref(info)) == -1 and "matrix G" in L.bmsp_last_error().decode()
    e = np.arange(8)
    wide = bmsp.BmSpMatrix.from_coo(8, 16, e, e, np.ones(8))
    refused(bmsp, lambda: bmsp.fsai(wide, wide), "square")
    refused(bmsp, lambda: bmsp.fsai(dA, pat(bmsp, F.lane_pattern(13, 8))), "matrix S", "shape")
    refused(bmsp, lambda: bmsp.fsai(mat(bmsp, A, 1), dS), "F16", status=-5)
    big = mat(bmsp, F.dominant(200, 0.3, 11, 0), 0)
    refused(bmsp, lambda: bmsp.fsai(big.row_panel(1, 13), pat(bmsp, F.lane_pattern(200, 8))), "row-panel view")
    refused(bmsp, lambda: bmsp.fsai(big, pat(bmsp, F.lane_pattern(200, 8)).row_panel(1, 13)), "row-panel view")
    # the first row without a diagonal, the first row with an entry right of it: rows 31 and 44 are damaged, 31 is named
    n, r, c = S
    keep = ~(((r == 31) | (r == 44)) & (r == c))
    refused(bmsp, lambda: bmsp.fsai(dA, pat(bmsp, (n, r[keep], c[keep]))), "row 31 of S", "diagonal")
    r2, c2 = np.concatenate([r, [31, 44]]), np.concatenate([c, [33, 69]])
    for lay in (0, 1):
        refused(bmsp, lambda: bmsp.fsai(dA, pat(bmsp, F.sort_coo(n, r2, c2), lay)), "row 31 of S", "right of the diagonal")
    # 65 entries in rows 120 and 150 of a 200-row pattern
    S200 = F.lane_pattern(200, 17)
    r, c = S200[1], S200[2]
    keep = ~np.isin(r, (120, 150))
    r3 = np.concatenate([r[keep], np.full(65, 120), np.full(66, 150)])
    c3 = np.concatenate([c[keep], np.arange(56, 121), np.arange(85, 151)])
    for lay in (0, 1):
        refused(bmsp, lambda: bmsp.fsai(big, pat(bmsp, F.sort_coo(200, r3, c3), lay)), "row 120 of S", "65", status=-6)
    assert raw(dA.h, 0, wide.h, 1, 0) == -1 and out.value == 0x5a5a      # *out is untouched after every refusal above
    # fsai_values: G of another dtype, G == A
    refused(bmsp, lambda: bmsp.fsai_values(dA, pat(bmsp, S, 0, 2)), "matrix G", "dtype")
    refused(bmsp, lambda: bmsp.fsai_values(dA, dA), "matrix G")
    # the handle
    refused(bmsp, lambda: bmsp.Fsai(dA, wide), "shape")
    f = bmsp.Fsai(dA, dS)
    b = dev(bmsp, F.solve_rhs(70, 0))
    assert L.bmsp_fsai_apply(f.h, b.ptr, b.ptr, None) == -1 and "d_z must not be d_r" in L.bmsp_last_error().decode()
    assert L.bmsp_fsai_apply(f.h, None, b.ptr, None) == -1 and "d_r" in L.bmsp_last_error().decode()
    assert L.bmsp_fsai_solve(f.h, 0, b.ptr, b.ptr, 0, 1e-6, 0, None, None, None) == -1 and "d_x must not be d_b" in L.bmsp_last_error().decode()
    assert L.bmsp_fsai_solve(f.h, 2, b.ptr, None, 0, 1e-6, 0, None, None, None) == -1 and L.bmsp_last_error().decode().startswith("method")
    assert L.bmsp_fsai_solve_gmres(f.h, 257, b.ptr, None, 0, 1e-6, 0, None, None, None) == -1 and L.bmsp_last_error().decode().startswith("restart")
    assert np.array_equal(b.to_host(), F.solve_rhs(70, 0))
    with pytest.raises(ValueError):
        f.solve(b, "minres")
    # bmsp_krylov_solve is as it was: kind 4 is refused
    refused(bmsp, lambda: bmsp.krylov_solve(dA, b, precond=bmsp.Precond(4, None, 0)), "pc->kind")


# ---------------------------------------------------------------------------------------------------------
# 7. the handle
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 2])
@pytest.mark.parametrize("kind", ["spd", "general"])
@pytest.mark.parametrize("materialise", [True, False])
def test_colmajor_application_is_two_public_products(bmsp, kind, materialise, dtype):
    A = F.dominant(200, 0.3, 11, dtype) if kind == "general" else F.poisson7()
    S = F.lane_pattern(200, 17) if kind == "general" else F.lower_of(A)
    n = A[0]
    dA, dS = mat(bmsp, A, dtype, 1), pat(bmsp, S)
    f = bmsp.Fsai(dA, dS, kind, materialise, colmajor=True)
    G1, G2 = f.factors()
    info = f.info()
    assert (info["kind"], info["materialised"], info["n"]) == (0 if kind == "spd" else 1, int(materialise), n), info
    assert G1.info()["transposed"] == 1 and G2.info()["transposed"] == 1 and (G1.h == G2.h) == (kind == "spd")
    scales = (SQRT, SQRT) if kind == "spd" else (NONE, UNIT)
    assert_same_bits(values_of(G1, S, dtype), reference(A, S, dtype, "N", scales[0])[0], "G1")
    assert_same_bits(values_of(G2, S, dtype), reference(A, S, dtype, "N" if kind == "spd" else "T", scales[1])[0], "G2")
    r = dev(bmsp, F.solve_rhs(n, dtype))
    z = f.apply(r).to_host()
    t = bmsp.spmv_op(G1, r, "N")
    want = bmsp.spmv_op(G2.transpose(True), t, "N") if materialise else bmsp.spmv_op(G2, t, "T")
    assert_same_bits(z, want.to_host(), "%s materialise %s" % (kind, materialise))
    assert_same_bits(f.apply(r).to_host(), z, "a second application")


@pytest.mark.parametrize("dtype", [0, 2])
@pytest.mark.parametrize("kind", ["spd", "general"])
def test_row_major_application_stays_within_the_a_priori_bound(bmsp, kind, dtype):
    """|z - z64| <= (g_a + g_b + g_a g_b) |G2^T| (|G1| |r|) componentwise, g_k = k u / (1 - k u), a and b the longest rows of the two
    factors as applied (G1 by rows, G2^T by rows = G2 by columns), u the unit roundoff of R, z64 formed in float64 from the device's own
    factor values: two recursive sums in any order"""
    A, S = F.dominant(200, 0.3, 11, dtype), F.lane_pattern(200, 33)
    dA, dS = mat(bmsp, A, dtype), pat(bmsp, S)
    r = F.solve_rhs(200, dtype)
    u = 2.0 ** -53 if dtype == 2 else 2.0 ** -24
    for materialise in (True, False):
        f = bmsp.Fsai(dA, dS, kind, materialise)
        G1, G2 = (F.dense_factor(S, values_of(G, S, dtype).astype(np.float64)) for G in f.factors())
        z = f.apply(dev(bmsp, r)).to_host().astype(np.float64)
        z64 = G2.T @ (G1 @ r.astype(np.float64))
        a, b = int((G1 != 0).sum(1).max()), int((G2 != 0).sum(0).max())
        ga, gb = a * u / (1 - a * u), b * u / (1 - b * u)
        bound = (ga + gb + ga * gb) * (np.abs(G2).T @ (np.abs(G1) @ np.abs(r.astype(np.float64))))
        print("row-major %s materialise %s: max |z - z64| / bound = %.3f" % (kind, materialise, (np.abs(z - z64) / bound).max()))
        assert (np.abs(z - z64) <= bound).all()


@pytest.mark.parametrize("kind,flags", [("spd", (True, True)), ("general", (True, False)), ("general", (False, True))])
def test_update_equals_a_new_handle(bmsp, kind, flags):
    A, S = F.dominant(200, 0.3, 11, 0), F.lane_pattern(200, 17)
    if kind == "spd":
        A = F.poisson7(); S = F.lower_of(A)
    n = A[0]
    dA, dS = mat(bmsp, A, 0, 1), pat(bmsp, S)
    f = bmsp.Fsai(dA, dS, kind, *flags)
    r = dev(bmsp, F.solve_rhs(n, 0))
    before = f.apply(r).to_host()
    d = dev(bmsp, (1.0 + (np.arange(n) % 4) / 4.0).astype(np.float32))
    dA.scale_(d, d)                                             # D A D keeps the symmetry
    f.update()
    fresh = bmsp.Fsai(dA, dS, kind, *flags)
    z = f.apply(r).to_host()
    assert_same_bits(z, fresh.apply(r).to_host(), "update")
    assert not np.array_equal(z, before)
    for G, H in zip(f.factors(), fresh.factors()):
        assert_same_bits(values_of(G, S, 0), values_of(H, S, 0))


# ---------------------------------------------------------------------------------------------------------
# 8. solves
# ---------------------------------------------------------------------------------------------------------
def callables(bmsp, dA, f):
    return (lambda v: bmsp.spmv_op(dA, dev(bmsp, v), "N").to_host(), lambda v: f.apply(dev(bmsp, v)).to_host(),
            lambda x, y: float(bmsp.vec_dot(dev(bmsp, x), dev(bmsp, y)).to_host()[0]))


def solve(f, bmsp, b, method, max_iter=0, tol=1e-6, x0=None, history=True):
    dx = None if x0 is None else dev(bmsp, x0)
    out = f.solve(dev(bmsp, b), method, max_iter, tol, dx, x0 is not None, history)
    return (out[0].to_host(),) + tuple(out[1:])


def gmres_same(got, want, msg=""):
    x, info, hist = got
    assert (info["iterations"], info["status"]) == (want.iterations, want.status), (info, want[1:3], msg)
    assert_same_bits(x, want.x, msg)
    with np.errstate(all="ignore"):
        whist = np.sqrt(np.asarray(want.hist, np.float64) / want.bb)
    assert hist.shape == whist.shape and np.array_equal(hist.view(np.uint64), whist.view(np.uint64)), (hist, whist, msg)
    assert (info["products"], info["precond_applies"]) == (want.products, want.applies), (info, msg)


BITWISE = [("cg", "spd"), ("bicgstab", "general"), ("gmres(5)", "general")]
STOL = {0: 1e-5, 2: 1e-6}


@pytest.mark.parametrize("dtype", [0, 2])
@pytest.mark.parametrize("method,kind", BITWISE)
def test_solve_equals_the_restatement_bit_for_bit(bmsp, monkeypatch, method, kind, dtype):
    monkeypatch.delenv("BMSP_KRYLOV_CHECK", raising=False)
    A = F.poisson7() if kind == "spd" else F.nonsym7()
    S = F.lower_of(A)
    n, tol, cap = A[0], STOL[dtype], 100
    dA = mat(bmsp, A, dtype, 1)
    f = bmsp.Fsai(dA, pat(bmsp, S), kind, colmajor=True)
    call = callables(bmsp, dA, f)
    b = F.solve_rhs(n, dtype)
    x0 = (np.arange(n) % 5 - 2).astype(VEC[dtype]) / 4
    gm = method.startswith("gmres")

    def want_of(x0, m, t):
        return restate_gmres(*call, b, x0, 5, m, t) if gm else restate(method, *call, b, x0, m, t)

    def same(got, want, msg):
        if gm:
            gmres_same(got, want, msg)
        else:
            same_as_restatement(got, want, dtype, msg)

    got = solve(f, bmsp, b, method, cap, tol)
    same(got, want_of(None, cap, tol), "plain")
    info = got[1]
    assert info["status"] == CONVERGED and info["relres"] <= tol and info["method"] == method + "+fsai" and info["max_iterations"] == cap, info
    k = info["iterations"]
    assert info["precond_applies"] in ((2 * k, 2 * k - 1) if method == "bicgstab" else (k,)), info
    same(solve(f, bmsp, b, method, cap, tol, x0=x0), want_of(x0, cap, tol), "x0")
    for check in ("1", "3", "64"):
        monkeypatch.setenv("BMSP_KRYLOV_CHECK", check)
        x, i2, h2 = solve(f, bmsp, b, method, cap, tol)
        assert_same_bits(x, got[0], check)
        assert i2 == info and np.array_equal(h2.view(np.uint64), got[2].view(np.uint64))
    monkeypatch.delenv("BMSP_KRYLOV_CHECK")
    for m in (1, 3, 7):
        x, inf = solve(f, bmsp, b, method, m, NO_CHECK, history=False)
        w = want_of(None, m, NO_CHECK)
        assert tuple(w[1:3]) == (m, MAXITER)
        assert_same_bits(x, w[0], "NO_CHECK %d" % m)
        assert (inf["iterations"], inf["status"], inf["relres"], inf["bnorm"]) == (m, MAXITER, -1.0, -1.0), inf


CONVERGE = [("cg", "spd", "poisson"), ("bicgstab", "general", "nonsym"), ("gmres(30)", "general", "nonsym")]


@pytest.mark.parametrize("dtype", [0, 2])
@pytest.mark.parametrize("method,kind,which", CONVERGE)
def test_converges_in_fewer_iterations_than_jacobi(bmsp, method, kind, which, dtype):
    A = F.poisson7() if which == "poisson" else F.nonsym7()
    S = F.lower_of(A)
    n, tol = A[0], STOL[dtype]
    b = F.solve_rhs(n, dtype)
    dA = mat(bmsp, A, dtype)
    f = bmsp.Fsai(dA, pat(bmsp, S), kind)
    x, info, hist = solve(f, bmsp, b, method, 200, tol)
    jac = dA.solve(dev(bmsp, b), method, "jacobi", max_iter=200, tol=tol)[1]
    b64 = b.astype(np.float64)
    true = np.linalg.norm(b64 - F.dense_of(A) @ x.astype(np.float64))
    print("%s %s %s: fsai %d iterations, jacobi %d; true residual %.3e (10 tol ||b|| = %.3e)"
          % (method, which, "F64" if dtype else "F32", info["iterations"], jac["iterations"], true, 10 * tol * np.linalg.norm(b64)))
    assert info["status"] == CONVERGED and info["relres"] <= tol, info
    assert jac["status"] == CONVERGED and info["iterations"] < jac["iterations"], (info, jac)
    if dtype == 2:
        assert true <= 10 * tol * np.linalg.norm(b64)


@pytest.mark.parametrize("method", ["cg", "bicgstab", "gmres(5)"])
def test_bad_rows_end_in_a_breakdown_not_an_error(bmsp, method):
    A = F.poisson7()
    n, r, c, v = A[0], A[1], A[2], A[3].copy()
    v[(r == 77) & (c == 77)] = 0.0
    v[(r == 77) & (c != 77)] = 0.0
    v[(c == 77) & (r != 77)] = 0.0                       # row and column 77 are zero: B_mm = 0 in row 77, Inf in G
    Z = (n, r, c, v)
    f = bmsp.Fsai(mat(bmsp, Z, 0, 1), pat(bmsp, F.lower_of(A)), "spd" if method == "cg" else "general", colmajor=True)
    assert f.info()["factor"][0]["bad_rows"] >= 1, f.info()
    x, info, hist = solve(f, bmsp, F.solve_rhs(n, 0), method, 50, 1e-5)
    assert info["status"] == BREAKDOWN, info             # (the call returned BMSP_OK: no exception)


def test_empty_matrix(bmsp):
    E = (0, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))
    f = bmsp.Fsai(mat(bmsp, E, 0), pat(bmsp, E))
    e = bmsp.DeviceArray(0, np.float32)
    assert f.apply(e).n == 0 and f.info()["n"] == 0
    for method in ("cg", "bicgstab", "gmres"):
        x, info, hist = f.solve(e, method, history=True)
        assert (info["iterations"], info["status"], hist.size) == (0, CONVERGED, 0)


PATTERN_SCRIPT = """
import sys
import numpy as np
import torch                              # before pybmsp: one HIP runtime for both
sys.path.insert(0, sys.argv[1])
import pybmsp as B
from pybmsp import gen
n, _, r, c, v = gen.rmat(10, 8, seed=3)
v = np.where(r == c, 50.0, v)
A = B.BmSpMatrix.from_coo(n, n, r, c, v)
S = B.fsai_pattern(A)
sr, sc, _ = S.to_coo()
k = c <= r
assert np.array_equal(np.sort(sr.astype(np.int64) * n + sc), np.sort(r[k].astype(np.int64) * n + c[k]))
T = B.fsai_pattern(A, 0.5, transposed=True)
tr, tc, _ = T.to_coo()
assert T.info()["transposed"] == 1 and tr.size < sr.size and (tc <= tr).all() and np.array_equal(np.unique(tr[tr == tc]), np.arange(n))
longest = int(np.bincount(tr, minlength=n).max())
if longest <= 64:
    G, info = A.fsai(T)
    assert info["rows"] == n and info["max_row"] == longest, info
print("OK longest", longest)
"""


def test_fsai_pattern(bmsp, tmp_path):
    """pybmsp.fsai_pattern masks with torch, which has to be imported before pybmsp: a process of its own"""
    import os
    import sys
    script = tmp_path / "pattern.py"
    script.write_text(PATTERN_SCRIPT)
    out = subprocess.run([sys.executable, str(script), os.path.dirname(os.path.dirname(bmsp.__file__))], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr


# ---------------------------------------------------------------------------------------------------------
# 9. the stream
# ---------------------------------------------------------------------------------------------------------
def stream_case(kind):
    import test_streams as TS
    A = F.nonsym7()
    S = F.lower_of(A)
    n = A[0]

    def make(bmsp, alt):
        M = (A[0], A[1], A[2], A[3] * (1.0 + (A[1] % 3) / 8.0)) if alt and kind == "values" else A
        dA = mat(bmsp, M, 0, 1)
        f = bmsp.Fsai(dA, pat(bmsp, S), "general", colmajor=True)
        b = dev(bmsp, F.solve_rhs(n, 0) + (1 if alt and kind != "values" else 0))
        if kind == "values":
            G = f.factors()[1]
            return TS.Ops([TS.vals_of(dA)], [TS.vals_of(G)], f=f, A=dA, G=G, b=b)
        return TS.Ops([b], [bmsp.DeviceArray(n, np.float32)], f=f, A=dA, b=b)

    def call(bmsp, o, st):
        if kind == "values":
            bmsp.fsai_values(o.A, o.G, "T", "unit", stream=st)
        elif kind == "apply":
            o.f.apply(o.b, o.outputs[0], stream=st)
        else:
            o.f.solve(o.b, "bicgstab", 3, NO_CHECK, o.outputs[0], stream=st)

    def prepare(bmsp, o):                 # the workspace of the solve on A's handle, on a buffer of its own
        if kind == "no_check":
            o.f.solve(o.b, "bicgstab", 3, NO_CHECK, bmsp.DeviceArray(n, np.float32))

    def read(bmsp, o, res):
        return [o.outputs[0].to_host()]

    return TS.Case("fsai-" + kind, TS.SYNC if kind == "values" else TS.ASYNC, make, call, read, prepare)


@pytest.mark.parametrize("kind", ["values", "apply", "no_check"])
def test_on_a_gated_stream(bmsp, monkeypatch, kind):
    import test_streams as TS
    assert TS.run_gated(bmsp, monkeypatch, stream_case(kind)) == (TS.SYNC if kind == "values" else TS.ASYNC)


# ---------------------------------------------------------------------------------------------------------
# 10. the C++ wrapper
# ---------------------------------------------------------------------------------------------------------
def test_cpp_wrapper_gives_the_ctypes_result(bmsp, tmp_path):
    A = F.poisson7()
    S = F.lower_of(A)
    n = A[0]
    paths = []
    for name, m in (("A", A), ("S", (S[0], S[1], S[2], np.ones(S[1].size)))):
        path = tmp_path / (name + ".mtx")
        with open(path, "w") as fh:
            fh.write("%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n, m[1].size))
            for i, j, a in zip(m[1], m[2], m[3]):
                fh.write("%d %d %.17g\n" % (i + 1, j + 1, a))
        paths.append(str(path))
    exe, out_bin = str(tmp_path / "cpp_fsai_check"), str(tmp_path / "out.bin")
    F.build_cpp_fsai_check(exe)
    out = subprocess.run([exe] + paths + [out_bin], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("OK") == 2 and "FAIL" not in out.stdout, out.stdout
    got = np.fromfile(out_bin, np.float32)
    assert got.size == 2 * n
    i = np.arange(n)
    b = ((0.5 + ((i * 7) % 11) / 8.0) * np.where(i % 3, 1.0, -1.0)).astype(np.float32)
    f = bmsp.Fsai(mat(bmsp, A, 0, 1), pat(bmsp, S, 1), "spd", colmajor=True)
    assert_same_bits(got[:n], f.apply(dev(bmsp, b)).to_host(), "z")
    assert_same_bits(got[n:], f.solve(dev(bmsp, b), "cg", 0, 1e-5)[0].to_host(), "x")
