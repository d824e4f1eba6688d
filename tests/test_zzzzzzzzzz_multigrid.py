"""GPU tests of bmsp_mg_create / _info / _vcycle / _solve (the hierarchies, the C reference of the cycle and the restatement of the solvers
are those of tests/test_multigrid_api.py, whose self-checks run without a GPU).

1. row mode, bit for bit: vcycle equals tests/multigrid_ref.c on every input, F32 and F64, NaN / Inf rows included, all operators row-major
   and all column-major; on `two` all 2^3 layout combinations of (A, P, R).  A second call gives the same bits; the operators are unchanged.
2. BMSP_MG_RESTRICT=spmv and R=None promise no bits: ||z - z_ref(all double)||inf <= 4 * e_row with e_row = ||z_ref(float) -
   z_ref(all double)||inf from the C reference alone (both are float evaluations of one linear operator that differ in summation order only,
   so their a-priori bounds coincide; 4 is the margin for that); e_row == 0 demands equality.  F32: for F64 the all-double reference IS
   the reference and e_row is 0 by construction, so F64 is held to an a-priori bound of double rounding instead (written down in the test).
   Row mode is bit for bit under every walk of a block-row (BMSP_MG_WALK): the default is a function of the operator's structure.
3. the default restriction rule reports per level what the forced switch reports and gives that mode's bits.
4. the solve bit for bit on a COLUMN-MAJOR A[0] (bmsp_spmv_op's pure view case) in row mode: x, iterations, status and history equal
   restate(...) driven with the library's product and dot and the reference cycle; X0_GIVEN; NO_CHECK at fixed counts; BMSP_KRYLOV_CHECK
   decides nothing.
5. the solve on pybmsp.amg's hierarchy (Poisson 5pt 32 x 32, F64): converged in fewer iterations than unpreconditioned CG, true residual
   <= 10 tol ||b||; BiCGStab + cycle on `nonsym`.
6. a zero diagonal is a breakdown, not an error.  7. refusals on real handles.  8. streams.  9. the C++ wrapper."""
import ctypes as C
import itertools
import subprocess
import numpy as np
import pytest
from test_spsv_api import VEC, assert_same_bits
from test_transpose import snapshot, assert_unchanged
from test_krylov_api import restate, NO_CHECK, MAXITER, CONVERGED, BREAKDOWN
from test_zzzzz_krylov import same_as_restatement, refused
from test_multigrid_api import (CASES, MULTI, PREPOST, SOLVES, TOL, OMEGA, hierarchy, rhs, ref_cycle, _sp, build_cpp_multigrid_check)

pytestmark = pytest.mark.gpu


def dev(bmsp, a):
    return bmsp.DeviceArray.from_host(np.ascontiguousarray(a))


def op(bmsp, m, dtype, lay):
    return bmsp.BmSpMatrix.from_coo(m[0], m[1], m[2], m[3], m[4], transposed=bool(lay), dtype=dtype)


def build(bmsp, case, dtype, lays=(0, 0, 0), pre=1, post=1, explicit_r=True, omega=OMEGA):
    """(Multigrid, its operators) of a case with A, P, R in layouts `lays`"""
    h = hierarchy(case, dtype)
    A = [op(bmsp, m, dtype, lays[0]) for m in h["A"]]
    P = [op(bmsp, m, dtype, lays[1]) for m in h["P"]]
    R = [op(bmsp, m, dtype, lays[2]) for m in h["R"]] if explicit_r else None
    mg = bmsp.Multigrid(A, P, R, h["inv"], omega, pre, post, ld_inv=h["ld"] if h["inv"] is not None else None)
    return mg, A + P + (R or [])


def prepost_of(case):
    return ((1, 1), (0, 0)) if case.startswith("d:") else PREPOST


# ---------------------------------------------------------------------------------------------------------
# 1. row mode, bit for bit
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 2])
@pytest.mark.parametrize("case", CASES)
def test_vcycle_equals_the_reference_bit_for_bit(bmsp, monkeypatch, case, dtype):
    monkeypatch.setenv("BMSP_MG_RESTRICT", "row")
    r = rhs(case, dtype)
    for pre, post in prepost_of(case):
        with np.errstate(all="ignore"):
            want = ref_cycle(case, dtype, r, pre, post)
        for lay in (0, 1):
            mg, ops = build(bmsp, case, dtype, (lay, lay, lay), pre, post)
            snaps = [snapshot(m) for m in ops]
            dr = dev(bmsp, r)
            z = mg.vcycle(dr).to_host()
            assert_same_bits(z, want, "%s pre %d post %d lay %d" % (case, pre, post, lay))
            z2 = dev(bmsp, np.full(r.size, 7, VEC[dtype]))
            mg.vcycle(dr, z2)
            assert_same_bits(z2.to_host(), want, "second call")
            assert np.array_equal(dr.to_host(), r)
            for m, s in zip(ops, snaps):
                assert_unchanged(m, s)
            info = mg.info()
            assert info["levels"] == len(hierarchy(case, dtype)["A"]) and info["n"] == [A[0] for A in hierarchy(case, dtype)["A"]]
            assert all(m == bmsp.MG_RESTRICT_ROW for m in info["restrict_mode"]) and (info["pre"], info["post"]) == (pre, post)
            if r.size:
                assert info["launches_per_cycle"] >= 1 and ("MINOR" if lay else "MAJOR") in info["kernel"] and info["workspace_bytes"] > 0
    if case == "j:path203_nodiag":
        assert not np.isfinite(want).all()                 # the Inf / NaN rows were compared


@pytest.mark.parametrize("dtype", [0, 2])
@pytest.mark.parametrize("lays", list(itertools.product((0, 1), repeat=3)))
def test_every_layout_combination_gives_the_same_bits(bmsp, monkeypatch, lays, dtype):
    monkeypatch.setenv("BMSP_MG_RESTRICT", "row")
    monkeypatch.delenv("BMSP_MG_WALK", raising=False)
    r = rhs("two", dtype)
    mg, _ = build(bmsp, "two", dtype, lays, 2, 3)
    assert_same_bits(mg.vcycle(dev(bmsp, r)).to_host(), ref_cycle("two", dtype, r, 2, 3), str(lays))


# ---------------------------------------------------------------------------------------------------------
# 2. spmv mode and R = None: within the cap
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("explicit_r", [True, False])
@pytest.mark.parametrize("case", MULTI)
def test_spmv_restriction_stays_within_the_cap(bmsp, monkeypatch, case, explicit_r):
    monkeypatch.setenv("BMSP_MG_RESTRICT", "spmv")
    r = rhs(case, 0)
    for pre, post in ((1, 1), (0, 2)):
        zw = ref_cycle(case, 0, r, pre, post, wide=True)
        e_row = float(np.abs(ref_cycle(case, 0, r, pre, post).astype(np.float64) - zw).max())
        for lays in ((0, 0, 0), (1, 1, 1), (0, 1, 0)):
            mg, _ = build(bmsp, case, 0, lays, pre, post, explicit_r)
            want_mode = bmsp.MG_RESTRICT_SPMV if explicit_r else bmsp.MG_RESTRICT_PT
            assert all(m == want_mode for m in mg.info()["restrict_mode"]), mg.info()
            z = mg.vcycle(dev(bmsp, r)).to_host()
            err = float(np.abs(z.astype(np.float64) - zw).max())
            print("%-7s R %-5s pre %d post %d lays %s  e_row %.3e  ||z - z_ref(all double)|| %.3e" % (case, "given" if explicit_r else "None", pre, post,
                                                                                                 lays, e_row, err))
            if e_row == 0.0:
                assert err == 0.0
            assert err <= 4 * e_row, (err, e_row)


@pytest.mark.parametrize("explicit_r", [True, False])
@pytest.mark.parametrize("case", MULTI)
def test_spmv_restriction_in_f64_stays_within_double_rounding(bmsp, monkeypatch, case, explicit_r):
    """F64 has no wider reference here, so the cap is a-priori: the GPU result and the double reference are double evaluations of one
    linear operator that differ in the summation order of the restriction only; every chain has at most 530 terms of a strictly
    dominant operator, so each stays within 530 * 2^-53 * 8 * ||z||inf of the exact result (8: levels and steps -- the bound the CPU
    self-check holds the reversed-order reference to), and the two within twice that of each other"""
    monkeypatch.setenv("BMSP_MG_RESTRICT", "spmv")
    r = rhs(case, 2)
    for pre, post in ((1, 1), (0, 2)):
        want = ref_cycle(case, 2, r, pre, post)
        cap = 2 * 530 * 2.0 ** -53 * 8 * np.abs(want).max()
        for lays in ((0, 0, 0), (1, 1, 1)):
            mg, _ = build(bmsp, case, 2, lays, pre, post, explicit_r)
            z = mg.vcycle(dev(bmsp, r)).to_host()
            err = float(np.abs(z - want).max())
            print("%-7s R %-5s pre %d post %d lays %s  ||z - z_ref(double)|| %.3e  cap %.3e" % (case, "given" if explicit_r else "None", pre, post, lays, err, cap))
            assert err <= cap, (err, cap)


@pytest.mark.parametrize("walk", ["group1", "group4", "wave"])
@pytest.mark.parametrize("dtype", [0, 2])
def test_every_walk_gives_the_same_bits(bmsp, monkeypatch, walk, dtype):
    """the three walks of a block-row forced on inputs with long rows (star530: 67 tiles in block-row 0 of A and of R), ragged sizes
    and both layouts: the reference's bits, and a NO_CHECK solve's"""
    monkeypatch.setenv("BMSP_MG_RESTRICT", "row")
    monkeypatch.setenv("BMSP_MG_WALK", walk)
    for case, pre, post in (("star", 2, 3), ("j:star530", 2, 3), ("three", 1, 1), ("j:path203_nodiag", 1, 1), ("fat", 0, 2)):
        r = rhs(case, dtype)
        with np.errstate(all="ignore"):
            want = ref_cycle(case, dtype, r, pre, post)
        for lay in (0, 1):
            mg, _ = build(bmsp, case, dtype, (lay, lay, lay), pre, post)
            assert walk in mg.info()["kernel"]
            assert_same_bits(mg.vcycle(dev(bmsp, r)).to_host(), want, "%s %s lay %d" % (case, walk, lay))


def test_a_single_row_matches_exactly_in_every_mode(bmsp, monkeypatch):
    """n_0 = 2, n_1 = 1 with one entry per row everywhere: every sum has one term, so e_row compares equal roundings and spmv mode and
    R = None must give the row bits"""
    A = [(2, 2, np.array([0, 1]), np.array([0, 1]), np.array([2.0, 4.0])), (1, 1, np.array([0]), np.array([0]), np.array([0.5]))]
    P = (2, 1, np.array([0, 1]), np.array([0, 0]), np.array([0.5, 0.0]))
    Rm = (1, 2, np.array([0]), np.array([0]), np.array([0.5]))
    r = np.array([1.5, -0.75], np.float32)
    outs = []
    for mode, explicit in (("row", True), ("spmv", True), ("spmv", False)):
        monkeypatch.setenv("BMSP_MG_RESTRICT", mode)
        mg = bmsp.Multigrid([op(bmsp, m, 0, 0) for m in A], [op(bmsp, P, 0, 0)], [op(bmsp, Rm, 0, 0)] if explicit else None,
                            np.array([[2.0]], np.float32))
        outs.append(mg.vcycle(dev(bmsp, r)).to_host())
    assert_same_bits(outs[1], outs[0])
    assert_same_bits(outs[2], outs[0])
    assert np.isfinite(outs[0]).all() and outs[0].any()


# ---------------------------------------------------------------------------------------------------------
# 3. the default restriction rule
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MULTI)
def test_default_restriction_rule(bmsp, monkeypatch, case):
    """a function of R's structure alone: the row kernel up to 24 tiles per block-row in the mean (include/bmsp.h)"""
    r = rhs(case, 0)
    monkeypatch.delenv("BMSP_MG_RESTRICT", raising=False)
    mg, ops = build(bmsp, case, 0)
    h = hierarchy(case, 0)
    Rs = ops[len(h["A"]) + len(h["P"]):]
    rule = [bmsp.MG_RESTRICT_ROW if R.info()["block_num"] <= 24 * ((R.info()["num_rows"] + 7) // 8) else bmsp.MG_RESTRICT_SPMV for R in Rs]
    modes = mg.info()["restrict_mode"]
    assert modes == rule, (modes, rule)
    assert modes == ([bmsp.MG_RESTRICT_SPMV] if case == "fat" else [bmsp.MG_RESTRICT_ROW] * len(Rs))
    z = mg.vcycle(dev(bmsp, r)).to_host()
    forced = "spmv" if modes[0] == bmsp.MG_RESTRICT_SPMV else "row"
    monkeypatch.setenv("BMSP_MG_RESTRICT", forced)
    assert mg.info()["restrict_mode"] == modes                      # the forced switch reports the same: read per call
    assert_same_bits(mg.vcycle(dev(bmsp, r)).to_host(), z, forced)
    mg2, _ = build(bmsp, case, 0)
    assert_same_bits(mg2.vcycle(dev(bmsp, r)).to_host(), z, "a fresh handle under the forced switch")
    other = "row" if forced == "spmv" else "spmv"
    monkeypatch.setenv("BMSP_MG_RESTRICT", other)
    assert mg.info()["restrict_mode"] == [bmsp.MG_RESTRICT_ROW if other == "row" else bmsp.MG_RESTRICT_SPMV] * len(Rs)
    mg3, _ = build(bmsp, case, 0, explicit_r=False)
    assert mg3.info()["restrict_mode"] == [bmsp.MG_RESTRICT_PT] * len(Rs)


# ---------------------------------------------------------------------------------------------------------
# 4. the solve, bit for bit
# ---------------------------------------------------------------------------------------------------------
def gpu_callables(bmsp, A0, case, dtype):
    matvec = lambda x: bmsp.spmv_op(A0, dev(bmsp, x), "N").to_host()
    dot = lambda x, y: float(bmsp.vec_dot(dev(bmsp, x), dev(bmsp, y)).to_host()[0])
    return matvec, (lambda r: ref_cycle(case, dtype, r)), dot


def solve(mg, bmsp, b, method, max_iter=0, tol=1e-6, x0=None, history=True, stream=None):
    dx = None if x0 is None else dev(bmsp, x0)
    out = mg.solve(dev(bmsp, b), method, max_iter, tol, dx, x0 is not None, history, stream)
    return (out[0].to_host(),) + tuple(out[1:])


@pytest.mark.parametrize("dtype", [0, 2])
@pytest.mark.parametrize("case,method", SOLVES)
def test_solve_equals_the_restatement_bit_for_bit(bmsp, monkeypatch, case, method, dtype):
    monkeypatch.setenv("BMSP_MG_RESTRICT", "row")
    monkeypatch.delenv("BMSP_KRYLOV_CHECK", raising=False)
    mg, ops = build(bmsp, case, dtype, (1, 0, 0))
    snaps = [snapshot(m) for m in ops]
    b, tol = rhs(case, dtype), TOL[dtype]
    call = gpu_callables(bmsp, ops[0], case, dtype)
    got = solve(mg, bmsp, b, method, 200, tol)
    want = restate(method, *call, b, None, 200, tol)
    same_as_restatement(got, want, dtype, "%s %s" % (case, method))
    info = got[1]
    assert info["status"] == CONVERGED and info["relres"] <= tol and info["method"] == method + "+mg" and info["max_iterations"] == 200, info
    k = info["iterations"]
    assert info["products"] in ((2 * k, 2 * k - 1) if method == "bicgstab" else (k,)), info
    assert info["precond_applies"] in ((2 * k, 2 * k - 1) if method == "bicgstab" else (k,)), info
    true = np.linalg.norm(b.astype(np.float64) - _sp(hierarchy(case, dtype)["A"][0]) @ got[0].astype(np.float64)) / np.linalg.norm(b.astype(np.float64))
    assert true <= 2 * tol, true
    for m, s in zip(ops, snaps):
        assert_unchanged(m, s)
    # BMSP_KRYLOV_CHECK decides nothing
    for check in ("1", "3", "1000"):
        monkeypatch.setenv("BMSP_KRYLOV_CHECK", check)
        x, i2, h2 = solve(mg, bmsp, b, method, 200, tol)
        assert_same_bits(x, got[0], check)
        assert i2 == info and np.array_equal(h2.view(np.uint64), got[2].view(np.uint64))
    monkeypatch.delenv("BMSP_KRYLOV_CHECK")
    # NO_CHECK at fixed iteration counts
    for m in (1, 3):
        x, inf = solve(mg, bmsp, b, method, m, NO_CHECK, history=False)
        w = restate(method, *call, b, None, m, NO_CHECK)
        assert w[1:3] == (m, MAXITER)
        assert_same_bits(x, w[0], "NO_CHECK %d" % m)
        assert (inf["iterations"], inf["status"], inf["relres"], inf["bnorm"]) == (m, MAXITER, -1.0, -1.0), inf
        assert inf["precond_applies"] == (2 * m if method == "bicgstab" else m)


@pytest.mark.parametrize("case,method,dtype", [("two", "cg", 0), ("three", "bicgstab", 2)])
def test_solve_with_x0_given(bmsp, monkeypatch, case, method, dtype):
    monkeypatch.setenv("BMSP_MG_RESTRICT", "row")
    mg, ops = build(bmsp, case, dtype, (1, 1, 0))
    b, tol = rhs(case, dtype), TOL[dtype]
    call = gpu_callables(bmsp, ops[0], case, dtype)
    x0 = (np.arange(b.size) % 5 - 2).astype(VEC[dtype]) / 4
    got = solve(mg, bmsp, b, method, 200, tol, x0=x0)
    same_as_restatement(got, restate(method, *call, b, x0, 200, tol), dtype, "x0")
    assert got[1]["status"] == CONVERGED
    x, _ = solve(mg, bmsp, b, method, 2, NO_CHECK, x0=x0, history=False)
    assert_same_bits(x, restate(method, *call, b, x0, 2, NO_CHECK)[0], "NO_CHECK with x0")
    # one short of the stop: MAXITER and the restatement's iterate
    its = got[1]["iterations"]
    short = solve(mg, bmsp, b, method, its - 1, tol, x0=x0)
    want = restate(method, *call, b, x0, its - 1, tol)
    assert want[2] == MAXITER
    same_as_restatement(short, want, dtype, "one short")


def test_empty_hierarchy(bmsp):
    mg, _ = build(bmsp, "empty", 0)
    e = bmsp.DeviceArray(0, np.float32)
    assert mg.vcycle(e).n == 0 and mg.info()["launches_per_cycle"] == 0
    x, info, hist = mg.solve(e, "cg", history=True)
    assert (info["iterations"], info["status"], hist.size) == (0, CONVERGED, 0)


# ---------------------------------------------------------------------------------------------------------
# 5. pybmsp.amg's hierarchy
# ---------------------------------------------------------------------------------------------------------
def test_solve_on_the_amg_hierarchy(bmsp):
    from pybmsp import amg, gen
    n, _, r, c, v = gen.poisson("5pt", 32, 32)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, dtype=bmsp.F64)
    levels = amg.build_hierarchy(A)
    assert len(levels) >= 2 and levels[-1].inv_dense.shape == (levels[-1].n, levels[-1].n) and levels[-1].inv_dense.dtype == np.float64
    rng = np.random.default_rng(11)
    hb = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    b, tol = dev(bmsp, hb), 1e-8
    mg = amg.device_cycle(levels)
    assert mg.info()["levels"] == len(levels) and mg.info()["coarse_exact"] == 1
    x, info = mg.solve(b, "cg", tol=tol, max_iter=200)
    plain = bmsp.krylov_solve(levels[0].A, b, "cg", None, tol=tol, max_iter=1000)[1]
    host = amg.pcg(levels[0].A, b, levels, tol=tol, max_iter=200)[1]
    import scipy.sparse as sp
    S = sp.csr_matrix((np.asarray(v, np.float64), (r, c)), shape=(n, n))
    true = np.linalg.norm(hb - S @ x.to_host())
    print("amg hierarchy, %d levels: device cg+mg %d iterations, amg.pcg %d, unpreconditioned %d; true residual %.3e (10 tol ||b|| = %.3e)"
          % (len(levels), info["iterations"], host["iterations"], plain["iterations"], true, 10 * tol * np.linalg.norm(hb)))
    assert info["status"] == CONVERGED and plain["status"] == CONVERGED and info["iterations"] < plain["iterations"], (info, plain)
    assert true <= 10 * tol * np.linalg.norm(hb)
    # one cycle agrees with the Python-driven one to rounding (another summation order in its products)
    z = mg.vcycle(b).to_host()
    zh = amg.vcycle(levels, b).to_host()
    assert np.abs(z - zh).max() <= 1e-10 * np.abs(zh).max()


@pytest.mark.parametrize("dtype", [0, 2])
def test_bicgstab_on_a_nonsymmetric_input(bmsp, monkeypatch, dtype):
    """`nonsym` (chosen by the CPU self-check) with every operator row-major and the default restriction: converged, true residual <= 2 tol"""
    monkeypatch.delenv("BMSP_MG_RESTRICT", raising=False)
    mg, ops = build(bmsp, "nonsym", dtype)
    b, tol = rhs("nonsym", dtype), TOL[dtype]
    x, info, hist = solve(mg, bmsp, b, "bicgstab", 200, tol)
    plain = bmsp.krylov_solve(ops[0], dev(bmsp, b), "bicgstab", None, tol=tol, max_iter=400)[1]
    true = np.linalg.norm(b.astype(np.float64) - _sp(hierarchy("nonsym", dtype)["A"][0]) @ x.astype(np.float64)) / np.linalg.norm(b.astype(np.float64))
    assert info["status"] == CONVERGED and info["iterations"] < plain["iterations"] and true <= 2 * tol, (info, plain, true)


# ---------------------------------------------------------------------------------------------------------
# 6. breakdown; 7. refusals
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_a_zero_diagonal_is_a_breakdown_not_an_error(bmsp, monkeypatch, method):
    monkeypatch.setenv("BMSP_MG_RESTRICT", "row")
    h = hierarchy("two", 0)
    A0 = list(h["A"][0])
    v = A0[4].copy()
    v[(A0[2] == 77) & (A0[3] == 77)] = 0.0
    A0[4] = v
    A = [op(bmsp, tuple(A0), 0, 1), op(bmsp, h["A"][1], 0, 0)]
    mg = bmsp.Multigrid(A, [op(bmsp, h["P"][0], 0, 0)], [op(bmsp, h["R"][0], 0, 0)], h["inv"])
    x, info, hist = solve(mg, bmsp, rhs("two", 0), method, 50, TOL[0])
    assert info["status"] == BREAKDOWN, info                       # (the call returned BMSP_OK: no exception)
    x, info = solve(mg, bmsp, rhs("two", 0), method, 4, NO_CHECK, history=False)      # caught on the device too: x stays finite
    assert np.isfinite(x).all()


def test_refusals_on_real_handles(bmsp):
    h = hierarchy("two", 0)
    A = [op(bmsp, m, 0, 0) for m in h["A"]]
    P, Rm = op(bmsp, h["P"][0], 0, 0), op(bmsp, h["R"][0], 0, 0)
    inv = h["inv"]
    M = bmsp.Multigrid
    refused(bmsp, lambda: M(A, [Rm], None, inv), "P[0]", "chain")
    refused(bmsp, lambda: M(A, [P], [P], inv), "R[0]", "chain")
    refused(bmsp, lambda: M([A[0], P], [P], None, None), "A[1]", "square")
    refused(bmsp, lambda: M([A[0], op(bmsp, h["A"][1], 2, 0)], [P], None, None), "A[1]", "dtype")
    refused(bmsp, lambda: M(A, [op(bmsp, h["P"][0], 2, 0)], None, inv), "P[0]", "dtype")
    refused(bmsp, lambda: M([op(bmsp, m, 1, 0) for m in h["A"]], [op(bmsp, h["P"][0], 1, 0)], None, None), "F16", status=-5)
    refused(bmsp, lambda: M(A, [P], None, inv, ld_inv=47), "ld_inv")
    refused(bmsp, lambda: M(A, [P], None, inv, pre=0, post=0), "pre + post")
    refused(bmsp, lambda: M(A, [P], None, inv, omega=float("nan")), "omega")
    refused(bmsp, lambda: M([A[0].row_panel(1, 13), A[1]], [P], None, inv), "row-panel view")
    n = 4104
    eye = (n, n, np.arange(n), np.arange(n), np.ones(n))
    refused(bmsp, lambda: M([op(bmsp, eye, 0, 0)], [], None, bmsp.DeviceArray(16, np.float32), ld_inv=n), "d_coarse_inv", "4096")
    # *out stays untouched
    out = C.c_void_p(0x5a5a)
    hs = (C.c_void_p * 2)(A[0].h, A[1].h)
    ps = (C.c_void_p * 1)(Rm.h)
    assert bmsp.lib().bmsp_mg_create(2, hs, ps, None, None, 0, OMEGA, 1, 1, None, C.byref(out)) == -1 and out.value == 0x5a5a
    mg = M(A, [P], [Rm], inv)
    b = dev(bmsp, rhs("two", 0))
    L = bmsp.lib()
    assert L.bmsp_mg_vcycle(mg.h, b.ptr, b.ptr, None) == -1 and "d_z must not be d_r" in L.bmsp_last_error().decode()
    assert L.bmsp_mg_vcycle(mg.h, None, b.ptr, None) == -1 and "d_r" in L.bmsp_last_error().decode()
    assert L.bmsp_mg_solve(mg.h, 0, b.ptr, b.ptr, 0, 1e-6, 0, None, None, None) == -1 and "d_x must not be d_b" in L.bmsp_last_error().decode()
    assert L.bmsp_mg_solve(mg.h, 0, b.ptr, None, 0, 1e-6, 0, None, None, None) == -1 and "d_x" in L.bmsp_last_error().decode()
    assert L.bmsp_mg_solve(mg.h, 2, b.ptr, None, 0, 1e-6, 0, None, None, None) == -1 and L.bmsp_last_error().decode().startswith("method")
    assert np.array_equal(b.to_host(), rhs("two", 0))                 # nothing was done on the device
    with pytest.raises(ValueError):
        mg.solve(dev(bmsp, rhs("two", 2)))
    with pytest.raises(ValueError):
        mg.solve(b, x0_given=True)
    # bmsp_krylov_solve is as it was: kind 4 is refused on a real handle too
    refused(bmsp, lambda: bmsp.krylov_solve(A[0], b, precond=bmsp.Precond(4, None, 0)), "pc->kind")


# ---------------------------------------------------------------------------------------------------------
# 8. streams
# ---------------------------------------------------------------------------------------------------------
def stream_case(kind):
    import test_streams as TS
    case_name, dtype = "two", 0
    n = hierarchy(case_name, dtype)["A"][0][0]

    def make(bmsp, alt):
        mg, ops = build(bmsp, case_name, dtype, (1, 0, 1))
        b = dev(bmsp, rhs(case_name, dtype) + (1 if alt else 0))
        return TS.Ops([b], [bmsp.DeviceArray(n, np.float32)], mg=mg, keep=ops, b=b)

    def call(bmsp, o, st):
        if kind == "vcycle":
            o.mg.vcycle(o.b, o.outputs[0], stream=st)
        else:
            o.mg.solve(o.b, "bicgstab", 3, NO_CHECK if kind == "no_check" else 1e-30, o.outputs[0], stream=st)

    def prepare(bmsp, o):                 # the workspace of the solve on A[0]'s handle, on a buffer of its own
        if kind != "vcycle":
            o.mg.solve(o.b, "bicgstab", 3, NO_CHECK if kind == "no_check" else 1e-30, bmsp.DeviceArray(n, np.float32))

    def read(bmsp, o, res):
        return [o.outputs[0].to_host()]

    return TS.Case("mg-" + kind, TS.SYNC if kind == "checked" else TS.ASYNC, make, call, read, prepare, env={"BMSP_MG_RESTRICT": "row"})


@pytest.mark.parametrize("kind", ["vcycle", "no_check", "checked"])
def test_on_a_gated_stream(bmsp, monkeypatch, kind):
    import test_streams as TS
    assert TS.run_gated(bmsp, monkeypatch, stream_case(kind)) == (TS.SYNC if kind == "checked" else TS.ASYNC)


# ---------------------------------------------------------------------------------------------------------
# 9. the C++ wrapper
# ---------------------------------------------------------------------------------------------------------
def test_cpp_wrapper_runs(bmsp, tmp_path):
    h = hierarchy("two", 2)
    paths = []
    for name, m in (("A0", h["A"][0]), ("P", h["P"][0]), ("A1", h["A"][1])):
        path = tmp_path / (name + ".mtx")
        with open(path, "w") as f:
            f.write("%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (m[0], m[1], m[2].size))
            for i, j, a in zip(m[2], m[3], m[4]):
                f.write("%d %d %.17g\n" % (i + 1, j + 1, a))
        paths.append(str(path))
    exe = str(tmp_path / "cpp_multigrid_check")
    build_cpp_multigrid_check(exe)
    out = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("OK") == 2 and "FAIL" not in out.stdout, out.stdout
