"""GPU tests of bmsp_gmres_solve / bmsp_mg_solve_gmres (the restatement is tests/test_gmres_api.py's; the matrices, right-hand sides and
the callables made of the library's own calls are those of the Krylov tests).

1. a COLUMN-MAJOR A, where bmsp_spmv_op is a pure function of its inputs: x, iterations, status, the history, bnorm, relres, products and
   precond_applies equal the restatement's, driven with the library's own product, preconditioner pieces and dot product -- every case,
   dtype and preconditioner at restart 20 (n7 and n1 exhaust the Krylov space there), and restarts that make the basis cross 8 and 16
   vectors under a cap that ends inside a cycle.
2. BMSP_KRYLOV_CHECK and BMSP_GMRES_GROUP decide nothing.  3. NO_CHECK, X0_GIVEN, restart 1.  4. op T, an F16 factor.
5. a vector of more than 384 chunks under both BMSP_VEC_DOT_FINISH settings.
6. a row-major A (no bit claim): converged, relres <= tol, true residual <= max(2 tol, twice the CPU restatement's of the case).
7. b = 0 and a breakdown.  8. refusals on real handles, operands unchanged, CG -> GMRES -> CG on one handle.  9. a gated stream.
10. bmsp_mg_solve_gmres on hierarchies.  11. the C++ and Python wrappers."""
import subprocess
import numpy as np
import pytest
from test_spsv_api import VEC, assert_same_bits
from test_transpose import snapshot, assert_unchanged
from test_krylov_api import CASES, TOL, NO_CHECK, MAXITER, CONVERGED, BREAKDOWN, matrix, rhs, preconds_of, true_residual
from test_zzzzz_krylov import gpu_callables, build, factor, dev, pc_arg, refused, big_poisson, FDT, GPU_PRECONDS
from test_gmres_api import restate_gmres, cpu_gmres, build_cpp_gmres_check, CAP

pytestmark = pytest.mark.gpu


def solve(bmsp, A, b, pc, F, op="N", restart=20, max_iter=CAP, tol=1e-6, x0=None, history=True, stream=None):
    dx = None if x0 is None else dev(bmsp, x0)
    out = bmsp.gmres_solve(A, dev(bmsp, b), pc_arg(bmsp, pc, F), op, restart, max_iter, tol, dx, x0 is not None, history, stream)
    return (out[0].to_host(),) + tuple(out[1:])


def same_as_restatement(got, want, msg=""):
    x, info, hist = got
    assert (info["iterations"], info["status"]) == (want.iterations, want.status), (info, want[1:3], want[5:], msg)
    assert_same_bits(x, want.x, msg)
    with np.errstate(all="ignore"):
        whist = np.sqrt(np.asarray(want.hist, np.float64) / want.bb)
        wrel = 0.0 if want.bb == 0.0 else float(np.sqrt(np.float64(want.rr) / np.float64(want.bb)))
    assert hist.shape == whist.shape and np.array_equal(hist.view(np.uint64), whist.view(np.uint64)), (hist, whist, msg)
    assert info["bnorm"] == float(np.sqrt(want.bb)) and info["relres"] == wrel, (info, wrel, msg)
    assert (info["products"], info["precond_applies"]) == (want.products, want.applies), (info, want[6:], msg)


def operands(bmsp, name, dtype, pc, lay=1, fdtype=None):
    A = build(bmsp, name, dtype, lay)
    F = factor(bmsp, name, FDT[dtype] if fdtype is None else fdtype, lay) if pc.startswith("ilu") else None
    return A, F, rhs(name, dtype)


# ---------------------------------------------------------------------------------------------------------
# 1. bit for bit on a column-major A
# ---------------------------------------------------------------------------------------------------------
BITWISE = [(name, dtype, pc) for name in CASES for dtype in (0, 2) for pc in GPU_PRECONDS
           if pc in preconds_of(name) or (pc == "ilu_sweeps1" and "ilu" in preconds_of(name))]


@pytest.mark.parametrize("name,dtype,pc", BITWISE)
def test_solve_equals_the_restatement_bit_for_bit(bmsp, monkeypatch, name, dtype, pc):
    monkeypatch.delenv("BMSP_KRYLOV_CHECK", raising=False)
    monkeypatch.delenv("BMSP_GMRES_GROUP", raising=False)
    A, F, b = operands(bmsp, name, dtype, pc)
    snaps = [snapshot(m) for m in (A, F) if m is not None]
    got = solve(bmsp, A, b, pc, F, restart=20, tol=TOL[dtype])
    want = restate_gmres(*gpu_callables(bmsp, A, dtype, pc, "N", F), b, None, 20, CAP, TOL[dtype])
    same_as_restatement(got, want, "%s %s" % (name, pc))
    info = got[1]
    assert info["status"] == CONVERGED and info["relres"] <= TOL[dtype], info
    assert info["method"] == "gmres(20)+%s" % pc.rstrip("0123456789") and info["max_iterations"] == CAP
    k = info["iterations"]
    assert info["products"] in (k + (k - 1) // 20, k + k // 20) and info["precond_applies"] == (0 if pc == "none" else k), info
    assert true_residual(name, dtype, got[0]) <= 2 * TOL[dtype]
    for m, s in zip([m for m in (A, F) if m is not None], snaps):
        assert_unchanged(m, s)


@pytest.mark.parametrize("restart", [1, 2, 8, 9, 16, 17])
@pytest.mark.parametrize("name,dtype,pc", [("p5_12", 0, "jacobi"), ("ragged203", 2, "none")])
def test_the_basis_crosses_the_group_sizes(bmsp, monkeypatch, name, dtype, pc, restart):
    """25 iterations at most: the cap falls inside a cycle; the status is whatever the restatement says"""
    monkeypatch.delenv("BMSP_GMRES_GROUP", raising=False)
    A, F, b = operands(bmsp, name, dtype, pc)
    got = solve(bmsp, A, b, pc, F, restart=restart, max_iter=25, tol=TOL[dtype])
    want = restate_gmres(*gpu_callables(bmsp, A, dtype, pc, "N", F), b, None, restart, 25, TOL[dtype])
    same_as_restatement(got, want, "restart %d" % restart)
    assert got[1]["method"].startswith("gmres(%d)+" % restart) and got[1]["max_iterations"] == 25


# ---------------------------------------------------------------------------------------------------------
# 2. the switches decide nothing
# ---------------------------------------------------------------------------------------------------------
def test_check_interval_and_group_decide_nothing(bmsp, monkeypatch):
    """restart 4: stops and batch boundaries fall inside cycles"""
    name, dtype, pc = "p5_12", 0, "jacobi"
    A, F, b = operands(bmsp, name, dtype, pc)
    monkeypatch.delenv("BMSP_KRYLOV_CHECK", raising=False)
    monkeypatch.delenv("BMSP_GMRES_GROUP", raising=False)
    want = restate_gmres(*gpu_callables(bmsp, A, dtype, pc, "N", F), b, None, 4, CAP, TOL[dtype])
    assert want.status == CONVERGED and want.iterations % 4 != 0 and want.iterations > 64
    first = None
    for check in (None, "1", "3", "7", "64"):
        for group in (None, "1", "4", "16"):
            for var, val in (("BMSP_KRYLOV_CHECK", check), ("BMSP_GMRES_GROUP", group)):
                if val is None:
                    monkeypatch.delenv(var, raising=False)
                else:
                    monkeypatch.setenv(var, val)
            got = solve(bmsp, A, b, pc, F, restart=4, tol=TOL[dtype])
            if first is None:
                first = got
                same_as_restatement(got, want)
            assert_same_bits(got[0], first[0], "check %s group %s" % (check, group))
            assert got[1] == first[1] and np.array_equal(got[2].view(np.uint64), first[2].view(np.uint64)), (check, group)


@pytest.mark.parametrize("group", ["1", "3", "5", "16"])
def test_group_on_a_long_basis(bmsp, monkeypatch, group):
    """restart 20 on ragged203 F64: groups that do not divide the basis, a last group of one"""
    name, dtype, pc = "ragged203", 2, "none"
    A, F, b = operands(bmsp, name, dtype, pc)
    monkeypatch.delenv("BMSP_GMRES_GROUP", raising=False)
    want = solve(bmsp, A, b, pc, F, restart=20, tol=TOL[dtype])
    assert want[1]["iterations"] > 20
    monkeypatch.setenv("BMSP_GMRES_GROUP", group)
    got = solve(bmsp, A, b, pc, F, restart=20, tol=TOL[dtype])
    assert_same_bits(got[0], want[0])
    assert got[1] == want[1] and np.array_equal(got[2].view(np.uint64), want[2].view(np.uint64))


# ---------------------------------------------------------------------------------------------------------
# 3. NO_CHECK, X0_GIVEN, restart 1
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype,pc", [("p5_12", 0, "none"), ("p7_6", 2, "jacobi"), ("ragged203", 2, "ilu"), ("rmat10", 0, "ilu_sweeps3")])
def test_x0_given_max_iter_and_no_check(bmsp, name, dtype, pc):
    A, F, b = operands(bmsp, name, dtype, pc)
    call = gpu_callables(bmsp, A, dtype, pc, "N", F)
    tol = TOL[dtype]
    x0 = (np.arange(b.size) % 5 - 2).astype(VEC[dtype]) / 4
    got = solve(bmsp, A, b, pc, F, restart=5, tol=tol, x0=x0)
    want = restate_gmres(*call, b, x0, 5, CAP, tol)
    same_as_restatement(got, want, "x0")
    assert got[1]["status"] == CONVERGED
    # the solution of a finer tolerance as the start: converged after 0 iterations, x untouched, one product
    again = solve(bmsp, A, b, pc, F, restart=5, tol=100 * tol, x0=got[0])
    assert (again[1]["iterations"], again[1]["status"], again[2].size, again[1]["products"]) == (0, CONVERGED, 0, 1), again[1]
    assert again[1]["relres"] <= 100 * tol
    assert_same_bits(again[0], got[0])
    # NO_CHECK: exactly max_iter iterations, a partial last cycle, nothing read back
    for m, restart in ((7, 3), (1, 3), (6, 3), (2, 30)):
        x, info = solve(bmsp, A, b, pc, F, restart=restart, max_iter=m, tol=NO_CHECK, history=False)
        want = restate_gmres(*call, b, None, restart, m, NO_CHECK)
        if want.status == MAXITER:      # (a preconditioned solve may reach rr == 0 or break down before)
            assert want.iterations == m
            assert (info["iterations"], info["status"], info["relres"], info["bnorm"]) == (m, MAXITER, -1.0, -1.0), info
            assert (info["products"], info["precond_applies"]) == (want.products, want.applies), (info, want[6:])
        assert_same_bits(x, want.x, "NO_CHECK %d restart %d" % (m, restart))
    x, info = solve(bmsp, A, b, pc, F, restart=3, max_iter=7, tol=NO_CHECK, x0=x0, history=False)
    want = restate_gmres(*call, b, x0, 3, 7, NO_CHECK)
    assert_same_bits(x, want.x, "NO_CHECK with x0")
    assert info["products"] == want.products == 7 + 2 + 1
    # the checked solve of the same cap gives the same iterate
    same_as_restatement(solve(bmsp, A, b, pc, F, restart=3, max_iter=7, tol=1e-30, x0=x0), restate_gmres(*call, b, x0, 3, 7, 1e-30), "cap 7")


@pytest.mark.parametrize("tol", [3e-1, 1e-1, 3e-2, 1e-2, 1e-3])
@pytest.mark.parametrize("name,dtype,pc", [("p5_12", 0, "none"), ("ragged203", 0, "jacobi")])
def test_restart_one_with_a_loose_tolerance(bmsp, name, dtype, pc, tol):
    """every iteration is a cycle: the rule is applied to the recomputed residual between any two of them (a stop there adds no record)"""
    A, F, b = operands(bmsp, name, dtype, pc)
    got = solve(bmsp, A, b, pc, F, restart=1, max_iter=60, tol=tol)
    want = restate_gmres(*gpu_callables(bmsp, A, dtype, pc, "N", F), b, None, 1, 60, tol)
    same_as_restatement(got, want, "tol %g" % tol)


# ---------------------------------------------------------------------------------------------------------
# 4. operands
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])     # (op T on a row-major A sweeps the view too: a pure function)
@pytest.mark.parametrize("name,dtype,pc", [("p5_12", 0, "jacobi"), ("ragged203", 2, "ilu"), ("rmat10", 0, "ilu_sweeps3"), ("rmat10p", 2, "none")])
def test_op_t(bmsp, name, dtype, pc, lay):
    A, F, b = operands(bmsp, name, dtype, pc, lay)
    got = solve(bmsp, A, b, pc, F, op="T", restart=20, tol=TOL[dtype])
    same_as_restatement(got, restate_gmres(*gpu_callables(bmsp, A, dtype, pc, "T", F), b, None, 20, CAP, TOL[dtype]))
    assert got[1]["status"] == CONVERGED
    assert true_residual(name, dtype, got[0], "T") <= 2 * TOL[dtype]


@pytest.mark.parametrize("name,pc", [("p5_12", "ilu"), ("ragged203", "ilu_sweeps3"), ("rmat10", "ilu")])
def test_an_f16_factor_under_an_f32_matrix(bmsp, name, pc):
    A, F, b = operands(bmsp, name, 0, pc, 1, fdtype=1)
    assert F.info()["dtype"] == bmsp.F16
    got = solve(bmsp, A, b, pc, F, restart=20, tol=TOL[0])
    same_as_restatement(got, restate_gmres(*gpu_callables(bmsp, A, 0, pc, "N", F), b, None, 20, CAP, TOL[0]))
    assert got[1]["status"] == CONVERGED


# ---------------------------------------------------------------------------------------------------------
# 5. more chunks than the ticket takes
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", ["jacobi", "none"])
def test_a_vector_of_more_chunks_than_the_ticket_takes(bmsp, monkeypatch, pc):
    """400 chunks: the default path (second level by launch) and the forced ticket give the restatement's bits"""
    n, r, c, v, b = big_poisson()
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, transposed=True, dtype=bmsp.F32)
    monkeypatch.delenv("BMSP_VEC_DOT_FINISH", raising=False)
    want = restate_gmres(*gpu_callables(bmsp, A, 0, pc, "N", None), b, None, 3, 4, NO_CHECK)
    assert (want.iterations, want.status) == (4, MAXITER)
    for finish in (None, "ticket", "launch"):
        if finish:
            monkeypatch.setenv("BMSP_VEC_DOT_FINISH", finish)
        assert_same_bits(solve(bmsp, A, b, pc, None, restart=3, max_iter=4, tol=NO_CHECK, history=False)[0], want.x, str(finish))
    same_as_restatement(solve(bmsp, A, b, pc, None, restart=3, max_iter=4, tol=TOL[0]),
                        restate_gmres(*gpu_callables(bmsp, A, 0, pc, "N", None), b, None, 3, 4, TOL[0]))


@pytest.mark.parametrize("name,dtype,pc", [("p5_12", 0, "jacobi"), ("ragged203", 2, "ilu"), ("rmat10p", 0, "none")])
def test_second_level_by_launch_gives_the_same_solve(bmsp, monkeypatch, name, dtype, pc):
    A, F, b = operands(bmsp, name, dtype, pc)
    monkeypatch.delenv("BMSP_VEC_DOT_FINISH", raising=False)
    want = restate_gmres(*gpu_callables(bmsp, A, dtype, pc, "N", F), b, None, 20, CAP, TOL[dtype])
    for finish in ("launch", "ticket"):
        monkeypatch.setenv("BMSP_VEC_DOT_FINISH", finish)
        same_as_restatement(solve(bmsp, A, b, pc, F, restart=20, tol=TOL[dtype]), want, finish)


# ---------------------------------------------------------------------------------------------------------
# 6. a row-major A
# ---------------------------------------------------------------------------------------------------------
ROW_MAJOR = [(name, dtype, pc) for name in CASES for dtype in (0, 2) for pc in preconds_of(name)]


@pytest.mark.parametrize("name,dtype,pc", ROW_MAJOR)
def test_row_major_matrix_converges_to_the_tolerance(bmsp, monkeypatch, name, dtype, pc):
    monkeypatch.delenv("BMSP_KRYLOV_CHECK", raising=False)
    A, F, b = operands(bmsp, name, dtype, pc, 0)
    tol = TOL[dtype]
    x, info, hist = solve(bmsp, A, b, pc, F, restart=20, tol=tol)
    res, recorded = true_residual(name, dtype, x), cpu_gmres(name, dtype, pc, 20)[1]
    print("true residual %-9s %s %-11s iterations %3d  %.3e (CPU restatement %.3e)" % (name, "F64" if dtype else "F32", pc, info["iterations"],
                                                                                      res, recorded))
    assert info["status"] == CONVERGED and info["relres"] <= tol, info
    assert hist.size == info["iterations"] and (hist[:-1] > tol).all()
    assert res <= max(2 * tol, 2 * recorded), (res, recorded)


# ---------------------------------------------------------------------------------------------------------
# 7. stops and results
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 2])
def test_zero_right_hand_side_and_breakdown(bmsp, dtype):
    name = "p5_12"
    A = build(bmsp, name, dtype, 1)
    n = matrix(name, dtype)[0]
    zero = np.zeros(n, VEC[dtype])
    for x0 in (None, np.full(n, np.nan, VEC[dtype])):
        x, info, hist = solve(bmsp, A, zero, "jacobi", None, tol=TOL[dtype], x0=x0)
        assert (info["iterations"], info["status"], info["relres"], info["bnorm"], hist.size) == (0, CONVERGED, 0.0, 0.0, 0), info
        assert not x.any() and info["products"] == 0 and info["precond_applies"] == 0
    x, info = solve(bmsp, A, zero, "none", None, restart=2, max_iter=3, tol=NO_CHECK, x0=np.ones(n, VEC[dtype]), history=False)
    assert not x.any()
    # one stored zero on the diagonal under Jacobi: z_0 holds an Inf, the dots are not finite; x keeps the start
    n, r, c, v = matrix(name, dtype)
    v = v.copy()
    v[(r == 77) & (c == 77)] = 0.0
    Z = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, transposed=True, dtype=dtype)
    b = rhs(name, dtype)
    x0 = np.full(n, 0.25, VEC[dtype])
    call = gpu_callables(bmsp, Z, dtype, "jacobi", "N", None)
    for start in (None, x0):
        got = solve(bmsp, Z, b, "jacobi", None, restart=4, tol=TOL[dtype], x0=start)
        want = restate_gmres(*call, b, start, 4, CAP, TOL[dtype])
        assert (want.status, want.iterations) == (BREAKDOWN, 0)
        same_as_restatement(got, want)
        assert_same_bits(got[0], np.zeros(n, VEC[dtype]) if start is None else x0)
        x, info = solve(bmsp, Z, b, "jacobi", None, restart=4, max_iter=6, tol=NO_CHECK, x0=start, history=False)       # caught on the device too
        assert_same_bits(x, want.x)
    # a breakdown in a later cycle leaves the iterate of the last completed one: the Jacobi solve on Z restarted from a finished cycle of A's
    first = solve(bmsp, A, b, "jacobi", None, restart=4, max_iter=4, tol=TOL[dtype])
    assert first[1]["status"] == MAXITER
    got = solve(bmsp, Z, b, "jacobi", None, restart=4, tol=TOL[dtype], x0=first[0])
    assert (got[1]["status"], got[1]["iterations"], got[1]["products"]) == (BREAKDOWN, 0, 1)
    assert_same_bits(got[0], first[0])


# ---------------------------------------------------------------------------------------------------------
# 8. handles
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
def test_refusals_on_real_handles(bmsp, lay):
    name = "ragged203"
    n = matrix(name, 0)[0]
    A, A64, A16 = build(bmsp, name, 0, lay), build(bmsp, name, 2, lay), build(bmsp, name, 1, lay)
    F, F64 = factor(bmsp, name, 0, lay), factor(bmsp, name, 2, lay)
    b, b64 = dev(bmsp, rhs(name, 0)), dev(bmsp, rhs(name, 2))
    x = dev(bmsp, np.full(n, -7.0, np.float32))
    L = bmsp.lib()

    def call(db, dx, **kw):
        return L.bmsp_gmres_solve(A.h, kw.get("op", 0), None, kw.get("restart", 0), db, dx, kw.get("max_iter", 0), 1e-6, 0, None, None, None)

    assert call(None, x.ptr) == -1 and "d_b" in L.bmsp_last_error().decode()
    assert call(b.ptr, None) == -1 and "d_x" in L.bmsp_last_error().decode()
    assert call(b.ptr, b.ptr) == -1 and "d_x must not be d_b" in L.bmsp_last_error().decode()
    assert call(b.ptr, b.ptr, restart=257) == -1 and L.bmsp_last_error().decode().startswith("restart")
    assert call(b.ptr, x.ptr, restart=-1) == -1 and L.bmsp_last_error().decode().startswith("restart")
    assert call(b.ptr, x.ptr, op=2) == -1 and L.bmsp_last_error().decode().startswith("op")
    refused(bmsp, lambda: bmsp.gmres_solve(A16, b, x=x), "F16", status=-5)
    refused(bmsp, lambda: bmsp.gmres_solve(A, b, precond=bmsp.Precond(bmsp.PC_ILU_EXACT, None, 0), x=x), "pc->F")
    refused(bmsp, lambda: bmsp.gmres_solve(A, b, precond=bmsp.Precond(4, None, 0), x=x), "pc->kind")
    refused(bmsp, lambda: bmsp.gmres_solve(A, b, precond=("ilu_sweeps", F, 0), x=x), "pc->sweeps")
    refused(bmsp, lambda: bmsp.gmres_solve(A, b, precond=("ilu", F64), x=x), "pc->F", "dtype")
    refused(bmsp, lambda: bmsp.gmres_solve(A64, b64, precond=("ilu", F)), "pc->F", "dtype")
    refused(bmsp, lambda: bmsp.gmres_solve(A, b, precond=("ilu", factor(bmsp, "p5_12", 0, lay)), x=x), "pc->F", "shape")
    e = np.arange(8)
    W = bmsp.BmSpMatrix.from_coo(8, 16, e, e, np.ones(8), transposed=bool(lay))
    refused(bmsp, lambda: bmsp.gmres_solve(W, b, x=x), "square")
    if not lay:
        refused(bmsp, lambda: bmsp.gmres_solve(A.row_panel(1, 13), b, x=x), "row-panel view")
    assert (x.to_host() == np.float32(-7.0)).all()          # nothing was done on the device
    with pytest.raises(ValueError):
        bmsp.gmres_solve(A, b, x0_given=True)
    with pytest.raises(ValueError):
        bmsp.gmres_solve(A, b64)


def test_cg_then_gmres_then_cg_on_one_handle(bmsp):
    """the workspace is shared: a CG solve after a GMRES solve gives the bits of a fresh handle, and so does the GMRES solve after CG; it
    grows to the largest need and goes with bmsp_matrix_invalidate(A, 1)"""
    name = "p5_12"
    b = dev(bmsp, rhs(name, 0))
    A, fresh = build(bmsp, name, 0, 1), [build(bmsp, name, 0, 1) for _ in range(2)]
    sa = snapshot(A)
    want_cg = bmsp.krylov_solve(fresh[0], b, "cg", "jacobi", max_iter=CAP, tol=TOL[0], history=True)
    want_gm = bmsp.gmres_solve(fresh[1], b, "jacobi", restart=20, max_iter=CAP, tol=TOL[0], history=True)
    outs = [bmsp.krylov_solve(A, b, "cg", "jacobi", max_iter=CAP, tol=TOL[0], history=True),
            bmsp.gmres_solve(A, b, "jacobi", restart=20, max_iter=CAP, tol=TOL[0], history=True),
            bmsp.krylov_solve(A, b, "cg", "jacobi", max_iter=CAP, tol=TOL[0], history=True)]
    for got, want in zip(outs, (want_cg, want_gm, want_cg)):
        assert_same_bits(got[0].to_host(), want[0].to_host())
        assert np.array_equal(got[2].view(np.uint64), want[2].view(np.uint64))
        assert {k: v for k, v in got[1].items() if k != "workspace_bytes"} == {k: v for k, v in want[1].items() if k != "workspace_bytes"}
    assert outs[0][1]["workspace_bytes"] == want_cg[1]["workspace_bytes"] < outs[1][1]["workspace_bytes"] == outs[2][1]["workspace_bytes"]
    assert outs[1][1]["workspace_bytes"] == want_gm[1]["workspace_bytes"]
    bmsp.lib().bmsp_matrix_invalidate(A.h, 1)
    assert bmsp.krylov_solve(A, b, "cg", "jacobi", max_iter=3, tol=TOL[0])[1]["workspace_bytes"] < want_gm[1]["workspace_bytes"]
    assert_unchanged(A, sa)
    assert np.array_equal(b.to_host(), rhs(name, 0))


# ---------------------------------------------------------------------------------------------------------
# 9. the stream
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", ["none", "jacobi", "ilu"])
def test_no_check_on_a_gated_stream(bmsp, pc):
    import stream_gate as G
    name = "p5_12"
    A, F, hb = operands(bmsp, name, 0, pc)
    n = matrix(name, 0)[0]
    b = dev(bmsp, hb)
    m, restart = 7, 3
    null = bmsp.gmres_solve(A, b, pc_arg(bmsp, pc, F), restart=restart, max_iter=m, tol=NO_CHECK)[0].to_host()       # (plans, views, workspace)
    assert null.any()
    x = dev(bmsp, np.zeros(n, np.float32))
    bmsp.synchronize()
    st, side = G.new_stream(), G.Side()
    gate = G.Gate()
    try:
        gate.close(st)
        bmsp.gmres_solve(A, b, pc_arg(bmsp, pc, F), restart=restart, max_iter=m, tol=NO_CHECK, x=x, stream=st.value)
        closed = gate.is_closed()                      # the call came back while the gate held the stream
        held = side.read(x.ptr, n, np.float32)
        still = gate.is_closed()
        gate.finish()
        assert closed, "bmsp_gmres_solve (BMSP_KRYLOV_NO_CHECK) did not return while the gate was closed"
        if still:
            assert not held.any()                      # nothing ran ahead of the gate
        assert_same_bits(x.to_host(), null)
    finally:
        gate.finish()
        side.close()
        G.destroy_stream(st)


# ---------------------------------------------------------------------------------------------------------
# 10. the cycle as the preconditioner
# ---------------------------------------------------------------------------------------------------------
def mg_solve(mg, bmsp, b, restart, max_iter=0, tol=1e-6, x0=None):
    dx = None if x0 is None else dev(bmsp, x0)
    out = mg.solve(dev(bmsp, b), "gmres", max_iter, tol, dx, x0 is not None, True, None, restart)
    return (out[0].to_host(),) + tuple(out[1:])


def mg_callables(bmsp, mg, A0):
    return (lambda v: bmsp.spmv_op(A0, dev(bmsp, v), "N").to_host(), lambda v: mg.vcycle(dev(bmsp, v)).to_host(),
            lambda x, y: float(bmsp.vec_dot(dev(bmsp, x), dev(bmsp, y)).to_host()[0]))


@pytest.mark.parametrize("dtype", [0, 2])
def test_mg_solve_on_a_poisson_hierarchy_bit_for_bit(bmsp, monkeypatch, dtype):
    """pybmsp.amg's hierarchy of a 5-point Poisson matrix, A[0] column-major, the restriction in row mode: the cycle is a pure function"""
    from pybmsp import amg, gen
    monkeypatch.setenv("BMSP_MG_RESTRICT", "row")
    monkeypatch.delenv("BMSP_KRYLOV_CHECK", raising=False)
    n, _, r, c, v = gen.poisson("5pt", 24, 24)
    levels = amg.build_hierarchy(bmsp.BmSpMatrix.from_coo(n, n, r, c, v, dtype=dtype), coarse=40)
    assert len(levels) >= 2
    A0 = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, transposed=True, dtype=dtype)      # (build_hierarchy keeps a row-major copy)
    mg = bmsp.Multigrid([A0] + [lv.A for lv in levels[1:]], [lv.P for lv in levels[:-1]], [lv.R for lv in levels[:-1]], levels[-1].inv_dense)
    rng = np.random.default_rng(n)
    b = (rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(VEC[dtype])
    tol = TOL[dtype]
    call = mg_callables(bmsp, mg, A0)
    for restart, cap in ((3, 50), (30, 50), (2, 3)):
        got = mg_solve(mg, bmsp, b, restart, cap, tol)
        want = restate_gmres(*call, b, None, restart, cap, tol)
        same_as_restatement(got, want, "restart %d" % restart)
        assert got[1]["method"] == "gmres(%d)+mg" % restart and got[1]["precond_applies"] == got[1]["iterations"]
        assert got[1]["status"] == (CONVERGED if cap == 50 else MAXITER), got[1]
    x0 = (np.arange(n) % 3 - 1).astype(VEC[dtype])
    same_as_restatement(mg_solve(mg, bmsp, b, 4, 50, tol, x0), restate_gmres(*call, b, x0, 4, 50, tol), "x0")
    jac = bmsp.gmres_solve(A0, dev(bmsp, b), "jacobi", restart=30, max_iter=400, tol=tol)[1]
    assert mg_solve(mg, bmsp, b, 30, 50, tol)[1]["iterations"] < jac["iterations"]


@pytest.mark.parametrize("dtype", [0, 2])
def test_mg_solve_on_a_nonsymmetric_input(bmsp, monkeypatch, dtype):
    """the multigrid tests' `nonsym` hierarchy with a column-major A[0] and pre != post: converges where the restatement does"""
    import test_zzzzzzzzzz_multigrid as M
    monkeypatch.setenv("BMSP_MG_RESTRICT", "row")
    mg, ops = M.build(bmsp, "nonsym", dtype, lays=(1, 0, 0), pre=2, post=1)
    b, tol = M.rhs("nonsym", dtype), TOL[dtype]
    got = mg_solve(mg, bmsp, b, 10, 200, tol)
    want = restate_gmres(*mg_callables(bmsp, mg, ops[0]), b, None, 10, 200, tol)
    assert want.status == CONVERGED
    same_as_restatement(got, want)
    true = np.linalg.norm(b.astype(np.float64) - M._sp(M.hierarchy("nonsym", dtype)["A"][0]) @ got[0].astype(np.float64)) / np.linalg.norm(b.astype(np.float64))
    assert true <= 2 * tol, true


def test_mg_refusals_on_a_real_handle(bmsp):
    import test_zzzzzzzzzz_multigrid as M
    mg, ops = M.build(bmsp, "two", 0)
    b = dev(bmsp, M.rhs("two", 0))
    L = bmsp.lib()
    assert L.bmsp_mg_solve_gmres(mg.h, 0, b.ptr, b.ptr, 0, 1e-6, 0, None, None, None) == -1 and "d_x must not be d_b" in L.bmsp_last_error().decode()
    assert L.bmsp_mg_solve_gmres(mg.h, 257, b.ptr, None, 0, 1e-6, 0, None, None, None) == -1 and L.bmsp_last_error().decode().startswith("restart")
    assert L.bmsp_mg_solve_gmres(mg.h, 4, None, b.ptr, 0, 1e-6, 0, None, None, None) == -1 and "d_b" in L.bmsp_last_error().decode()
    with pytest.raises(ValueError):
        mg.solve(b, "minres")


# ---------------------------------------------------------------------------------------------------------
# 11. the wrappers
# ---------------------------------------------------------------------------------------------------------
def test_python_wrappers_agree(bmsp):
    A, F, hb = operands(bmsp, "ragged203", 0, "ilu")
    b = dev(bmsp, hb)
    want = bmsp.gmres_solve(A, b, ("ilu", F), restart=8, max_iter=CAP, tol=TOL[0], history=True)
    for got in (A.solve(b, "gmres(8)", ("ilu", F), max_iter=CAP, tol=TOL[0], history=True),
                A.solve_gmres(b, ("ilu", F), restart=8, max_iter=CAP, tol=TOL[0], history=True)):
        assert_same_bits(got[0].to_host(), want[0].to_host())
        assert got[1] == want[1] and np.array_equal(got[2], want[2])
    assert A.solve(b, "gmres", "jacobi", max_iter=CAP, tol=TOL[0])[1]["method"] == "gmres(30)+jacobi"
    assert bmsp.gmres_solve(A, b, restart=0, max_iter=2)[1]["method"] == "gmres(30)+none"


def test_cpp_wrapper_runs(bmsp, tmp_path):
    """tests/cpp_gmres_check.cpp: bmSparse_solve_gmres and bmSpMultigrid::solve_gmres for float and double on a fixture written here"""
    n, r, c, v = matrix("p5_12", 0)
    mtx = tmp_path / "spd.mtx"
    with open(mtx, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n, r.size))
        for i, j, a in zip(r, c, v):
            f.write("%d %d %.17g\n" % (i + 1, j + 1, a))
    exe = str(tmp_path / "cpp_gmres_check")
    build_cpp_gmres_check(exe)
    out = subprocess.run([exe, str(mtx)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("OK") == 2 and "FAIL" not in out.stdout, out.stdout
