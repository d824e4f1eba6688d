"""CPU tests of the surface of bmsp_gmres_solve / bmsp_mg_solve_gmres, and what tests/test_zzzzzzzzzzzz_gmres.py shares with them: a numpy
restatement of restarted GMRES as include/bmsp.h fixes it (right-preconditioned, classical Gram-Schmidt applied twice, Givens rotations)
that takes the product, the preconditioner and the dot product as callables -- float32 or float64 arrays, one rounding per numpy
operation, the scalars numpy doubles.  The matrices, right-hand sides, the C dot and the host preconditioners are those of
tests/test_krylov_api.py.

Checked here without a GPU: the prototypes and the text in bmsp.h; the refusals of the two C entry points (scalars before handles, the
argument named, `restart` among them); the Python and C++ wrappers; the restatement's stops; its convergence on every test case with a
scipy product and the C dot at restart 4 and 20; the gfx950 assembly of gmres.hip (every instantiation present, no scratch).

The bound on the true residual is 1.5 tol, test_krylov_api's margin for its restatements.  The reason it is not 1.0: the rule stops on
the residual of the least-squares problem, rr_k <= thr, which is the true residual only in exact arithmetic; x is then formed in the
vector type from J columns, and the two differ by the rounding of that sum, of the basis and of the product -- a few ulps of R times
||A|| ||x|| / ||b||, which for these matrices (||A|| ||x|| / ||b|| of order 1 to 10) is below 0.5 tol at tol = 1e-5 in F32 (ulp 6e-8) and
tol = 1e-10 in F64 (ulp 1.1e-16).

True residuals ||b - A x|| / ||b|| in float64 of the restatement on the CPU (scipy product, C dot), tol = 1e-5 for F32 and 1e-10 for F64,
max_iter 400, as test_restatement_converges_on_every_case prints them (-s); per case and restart: preconditioner, iterations, true
residual:
    p5_12     F32 m  4  none 93 it 9.867e-06; jacobi 93 it 9.867e-06; ilu 16 it 7.675e-06; ilu_sweeps3 18 it 6.743e-06
    p5_12     F32 m 20  none 39 it 7.022e-06; jacobi 39 it 7.022e-06; ilu 11 it 3.788e-06; ilu_sweeps3 11 it 8.066e-06
    p5_12     F64 m  4  none 203 it 9.440e-11; jacobi 203 it 9.440e-11; ilu 34 it 6.130e-11; ilu_sweeps3 38 it 7.528e-11
    p5_12     F64 m 20  none 78 it 8.067e-11; jacobi 78 it 8.067e-11; ilu 18 it 7.525e-11; ilu_sweeps3 19 it 4.830e-11
    p7_6      F32 m  4  none 28 it 9.163e-06; jacobi 28 it 9.158e-06; ilu 8 it 1.715e-06; ilu_sweeps3 8 it 2.487e-06
    p7_6      F32 m 20  none 18 it 9.871e-06; jacobi 18 it 9.864e-06; ilu 7 it 6.493e-06; ilu_sweeps3 7 it 4.943e-06
    p7_6      F64 m  4  none 66 it 7.199e-11; jacobi 66 it 7.199e-11; ilu 15 it 3.989e-11; ilu_sweeps3 16 it 1.823e-11
    p7_6      F64 m 20  none 35 it 9.970e-11; jacobi 35 it 9.970e-11; ilu 13 it 1.878e-11; ilu_sweeps3 13 it 5.878e-11
    ragged203 F32 m  4  none 47 it 9.387e-06; jacobi 8 it 3.629e-06; ilu 4 it 4.296e-07; ilu_sweeps3 4 it 4.363e-07
    ragged203 F32 m 20  none 35 it 5.363e-06; jacobi 8 it 3.549e-06; ilu 4 it 4.296e-07; ilu_sweeps3 4 it 4.363e-07
    ragged203 F64 m  4  none 95 it 9.244e-11; jacobi 15 it 9.694e-11; ilu 7 it 7.385e-12; ilu_sweeps3 7 it 8.026e-12
    ragged203 F64 m 20  none 68 it 8.546e-11; jacobi 15 it 6.727e-11; ilu 7 it 6.553e-12; ilu_sweeps3 7 it 7.136e-12
    rmat10    F32 m  4  jacobi 9 it 9.684e-06; ilu 4 it 4.736e-06; ilu_sweeps3 4 it 4.859e-06
    rmat10    F32 m 20  jacobi 9 it 9.487e-06; ilu 4 it 4.736e-06; ilu_sweeps3 4 it 4.859e-06
    rmat10    F64 m  4  jacobi 18 it 4.483e-11; ilu 8 it 1.321e-11; ilu_sweeps3 8 it 1.258e-11
    rmat10    F64 m 20  jacobi 18 it 3.711e-11; ilu 8 it 1.312e-11; ilu_sweeps3 8 it 1.238e-11
    rmat10p   F32 m  4  none 145 it 8.749e-06
    rmat10p   F32 m 20  none 85 it 9.028e-06
    rmat10p   F64 m  4  none 265 it 9.091e-11
    rmat10p   F64 m 20  none 166 it 8.766e-11
    n7        F32 m  4  none 8 it 7.493e-06; jacobi 8 it 7.493e-06; ilu 1 it 5.572e-08; ilu_sweeps3 1 it 5.572e-08
    n7        F32 m 20  none 6 it 7.997e-06; jacobi 6 it 7.997e-06; ilu 1 it 5.572e-08; ilu_sweeps3 1 it 5.572e-08
    n7        F64 m  4  none 17 it 3.168e-11; jacobi 17 it 3.168e-11; ilu 1 it 1.084e-16; ilu_sweeps3 1 it 1.084e-16
    n7        F64 m 20  none 7 it 2.655e-16; jacobi 7 it 2.655e-16; ilu 1 it 1.084e-16; ilu_sweeps3 1 it 1.084e-16
    n1        F32 m  4  none 1 it 0.000e+00; jacobi 1 it 0.000e+00; ilu 1 it 0.000e+00; ilu_sweeps3 1 it 0.000e+00
    n1        F32 m 20  none 1 it 0.000e+00; jacobi 1 it 0.000e+00; ilu 1 it 0.000e+00; ilu_sweeps3 1 it 0.000e+00
    n1        F64 m  4  none 1 it 2.021e-16; jacobi 1 it 2.021e-16; ilu 1 it 2.021e-16; ilu_sweeps3 1 it 2.021e-16
    n1        F64 m 20  none 1 it 2.021e-16; jacobi 1 it 2.021e-16; ilu 1 it 2.021e-16; ilu_sweeps3 1 it 2.021e-16
All are at most 1.00 tol.  rmat10 without a preconditioner is replaced by rmat10p, as in tests/test_krylov_api.py.
"""
import ctypes as C
import functools
import inspect
import os
import re
import subprocess
import numpy as np
import pytest
from conftest import REPO
from test_spsv_api import VEC, _msg, _flat
from test_krylov_api import (CASES, TOL, NO_CHECK, MAXITER, CONVERGED, BREAKDOWN, BMSP_ERR_INVALID, matrix, rhs, cdot, preconds_of,
                             true_residual, cpu_callables)

RESTARTS = (4, 20)
CAP = 400


# ---------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------
class Gmres(tuple):
    """(x, iterations, status, rr_history, bb, rr, products, applies): rr is the residual dot info->relres reports"""
    x, iterations, status, hist, bb, rr, products, applies = (property(lambda s, i=i: s[i]) for i in range(8))


def restate_gmres(matvec, precond, dot, b, x0=None, restart=30, max_iter=0, tol=1e-6):
    """GMRES(restart) as include/bmsp.h fixes it.  matvec(v) -> op(A) v, precond(v) -> M^-1 v (None: no preconditioner), dot(x, y) ->
    float; b and x0 arrays of the vector type R.  rr_history[k] is the residual dot recorded by iteration k + 1."""
    R, D = b.dtype.type, np.float64
    n = b.size
    cap = int(max_iter) if max_iter else min(n, 1 << 20)
    m = int(restart) if restart else 30
    hist = []
    products = applies = 0
    with np.errstate(all="ignore"):
        bb = D(dot(b, b))
        thr = D(-1.0) if tol == NO_CHECK else D(D(tol) * D(tol)) * bb
        x = np.zeros(n, R) if x0 is None else np.array(x0, R)

        def judge(rr):
            if not np.isfinite(rr):
                return BREAKDOWN
            if rr <= thr:
                return CONVERGED
            return BREAKDOWN if rr == 0.0 else None

        def out(k, status, rr):
            return Gmres((x, k, status, hist, float(bb), float(rr), products, applies))

        if bb == 0.0:
            x = np.zeros(n, R)
            return out(0, CONVERGED, D(0.0))
        if not np.isfinite(bb):
            return out(0, BREAKDOWN, D(0.0))
        if x0 is None:
            r, rr = b.copy(), bb
        else:
            r = b - matvec(x)
            products += 1
            rr = D(dot(r, r))
        k = 0
        last = rr
        while True:
            last = rr
            verdict = judge(rr)
            if verdict is not None:
                return out(k, verdict, rr)
            beta = np.sqrt(rr)
            V = [R(D(1.0) / beta) * r]
            Z, U, cs, sn, g = [], [], [], [], [beta]
            ended = None
            J = 0
            for j in range(m):
                z = V[j] if precond is None else precond(V[j])
                w = matvec(z)
                t = []
                for _ in range(2):
                    tp = [D(dot(V[i], w)) for i in range(j + 1)]
                    for i in range(j + 1):
                        w = w - R(tp[i]) * V[i]
                    t.append(tp)
                h = [t[0][i] + t[1][i] for i in range(j + 1)]
                hn = np.sqrt(D(dot(w, w)))
                if not (np.isfinite(t[0]).all() and np.isfinite(t[1]).all() and np.isfinite(h).all() and np.isfinite(hn)):
                    return out(k, BREAKDOWN, last)
                for i in range(j):
                    p, q = h[i], h[i + 1]
                    h[i] = cs[i] * p + sn[i] * q
                    h[i + 1] = cs[i] * q - sn[i] * p
                d = np.sqrt(h[j] * h[j] + hn * hn)
                if d == 0.0 or not np.isfinite(d):
                    return out(k, BREAKDOWN, last)
                cs.append(h[j] / d)
                sn.append(hn / d)
                h[j] = d
                gn = -(sn[j] * g[j])
                g[j] = cs[j] * g[j]
                g.append(gn)
                U.append(h)
                Z.append(z)
                k += 1
                products += 1
                applies += 0 if precond is None else 1
                last = gn * gn
                hist.append(float(last))
                J = j + 1
                verdict = judge(last)
                if verdict == BREAKDOWN:
                    return out(k, BREAKDOWN, last)
                if verdict == CONVERGED or k == cap:
                    ended = CONVERGED if verdict == CONVERGED else MAXITER
                    break
                if j < m - 1:
                    V.append(R(D(1.0) / hn) * w)
            y = [D(0.0)] * J
            for i in range(J - 1, -1, -1):
                s = g[i]
                for l in range(i + 1, J):
                    s = s - U[l][i] * y[l]
                y[i] = s / U[i][i]
            for i in range(J):
                x = x + R(y[i]) * Z[i]
            if ended is not None:
                return out(k, ended, last)
            r = b - matvec(x)
            products += 1
            rr = D(dot(r, r))


@functools.lru_cache(maxsize=None)
def cpu_gmres(name, dtype, pc, restart):
    """(the restatement's result on the CPU, its true residual): computed once, shared, never written"""
    matvec, precond = cpu_callables(name, dtype, pc)
    got = restate_gmres(matvec, precond, cdot, rhs(name, dtype), None, restart, CAP, TOL[dtype])
    got.x.setflags(write=False)
    return got, true_residual(name, dtype, got.x)


ALL_CPU = [(name, dtype, pc, m) for name in CASES for dtype in (0, 2) for pc in preconds_of(name) for m in RESTARTS]


@pytest.mark.parametrize("name,dtype,pc,restart", ALL_CPU)
def test_restatement_converges_on_every_case(name, dtype, pc, restart):
    got, res = cpu_gmres(name, dtype, pc, restart)
    print("true residual %-9s %s m %2d %-11s iterations %3d  %.3e" % (name, "F64" if dtype else "F32", restart, pc, got.iterations, res))
    thr = (TOL[dtype] * TOL[dtype]) * got.bb
    assert got.status == CONVERGED and 1 <= got.iterations <= CAP, (got.status, got.iterations)
    assert np.isfinite(got.x).all() and np.isfinite(got.hist).all() and len(got.hist) == got.iterations
    assert got.rr <= thr and all(h > thr for h in got.hist[:-1])
    for lo in range(0, got.iterations, restart):          # the residual of the least-squares problem never grows within a cycle
        cyc = got.hist[lo:lo + restart]
        assert all(b <= a for a, b in zip(cyc, cyc[1:])), (lo, cyc)
    restarts = (got.iterations - 1) // restart if got.rr == got.hist[-1] else got.iterations // restart
    assert got.products == got.iterations + restarts and got.applies == (0 if pc == "none" else got.iterations)
    assert res <= 1.5 * TOL[dtype], res


def test_restatement_stops_and_breaks_down_as_the_header_says():
    name, dtype = "p5_12", 0
    matvec, _ = cpu_callables(name, dtype, "none")
    b = rhs(name, dtype)
    full, _ = cpu_gmres(name, dtype, "none", 4)
    assert full.iterations > 9
    # a cap inside a cycle: MAXITER, the columns completed so far are in x; the history is the full solve's
    short = restate_gmres(matvec, None, cdot, b, None, 4, 6, TOL[dtype])
    assert (short.iterations, short.status) == (6, MAXITER) and short.hist == full.hist[:6] and short.products == 6 + 1 and short.x.any()
    # NO_CHECK runs them all, and gives the same iterates
    for m in (1, 4, 7):
        free = restate_gmres(matvec, None, cdot, b, None, 3, m, NO_CHECK)
        held = restate_gmres(matvec, None, cdot, b, None, 3, m, TOL[dtype])
        assert (free.iterations, free.status) == (m, MAXITER) and free.hist == held.hist and np.array_equal(free.x, held.x)
        assert free.products == m + (m - 1) // 3
    # b = 0
    zero = restate_gmres(matvec, None, cdot, np.zeros_like(b), np.ones_like(b), 4, 0, 1e-6)
    assert (zero.iterations, zero.status, len(zero.hist), zero.products) == (0, CONVERGED, 0, 0) and not zero.x.any()
    # a zero on the diagonal under Jacobi: Inf in z_0, the dots are not finite; x keeps the start
    d = np.ones_like(b)
    d[3] = 0
    x0 = np.full_like(b, 0.25)
    broke = restate_gmres(matvec, lambda v: v / d, cdot, b, x0, 4, 0, 1e-6)
    assert (broke.iterations, broke.status, len(broke.hist), broke.products) == (0, BREAKDOWN, 0, 1) and np.array_equal(broke.x, x0)
    # ... in the second cycle: x is the first cycle's iterate
    calls = []

    def late(v):
        calls.append(0)
        return v / (d if len(calls) > 4 else np.ones_like(d))
    broke = restate_gmres(matvec, late, cdot, b, None, 4, 0, 1e-6)
    one = restate_gmres(matvec, lambda v: v.copy(), cdot, b, None, 4, 4, 1e-6)
    assert (broke.iterations, broke.status, broke.products) == (4, BREAKDOWN, 5) and np.array_equal(broke.x, one.x) and broke.rr != broke.hist[-1]
    # a start that is the solution; a restart whose residual already meets the rule adds no record
    again = restate_gmres(matvec, None, cdot, b, full.x, 4, 0, 1e-4)
    assert (again.iterations, again.status, again.products) == (0, CONVERGED, 1) and np.array_equal(again.x, full.x)
    # the space is exhausted: one row
    b1 = rhs("n1", 2)
    mv1, _ = cpu_callables("n1", 2, "none")
    tiny = restate_gmres(mv1, None, cdot, b1, None, 20, 400, 1e-10)
    assert (tiny.iterations, tiny.status) == (1, CONVERGED) and true_residual("n1", 2, tiny.x) <= 1e-15


# ---------------------------------------------------------------------------------------------------------
# the entry points
# ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_interface_verbatim(bmsp):
    hdr = _flat(open(os.path.join(REPO, "include", "bmsp.h")).read())
    for line in (
            "int bmsp_gmres_solve(bmsp_matrix_t A, int op, const bmsp_precond *pc /* NULL = none */, int restart /* 0 = 30 */, "
            "const void *d_b, void *d_x, int64_t max_iter, double tol, int flags, double *relres_history, bmsp_krylov_info *info, void *stream);",
            "int bmsp_mg_solve_gmres(bmsp_mg_t mg, int restart, const void *d_b, void *d_x, int64_t max_iter, double tol, int flags, "
            "double *relres_history, bmsp_krylov_info *info, void *stream);"):
        assert _flat(line) in hdr, line
    for phrase in ("v_0 = fl(sR * r)", "w = fl(w - fl(tR_i * v_i))", "h_{j+1} = sqrt(dot(w, w))", "(not hypot)", "g_{j+1} = -fl(s_j g_j)",
                   "rr_k = fl(g_{j+1} g_{j+1})", "s = fl(s - fl(U_il y_l))", "x = fl(x + fl(yR_i * z_i))", "BMSP_GMRES_GROUP",
                   "x is NOT updated from the partial cycle", "gmres(<m>)+none", "the iterations plus the restarts performed"):
        assert _flat(phrase) in hdr, phrase
    for name in ("bmsp_gmres_solve", "bmsp_mg_solve_gmres"):
        assert name in bmsp.SYMBOLS and hasattr(bmsp.lib(), name)
    lib = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib", "libbmsp.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T bmsp_gmres_solve$", syms, re.M) and re.search(r" T bmsp_mg_solve_gmres$", syms, re.M)


def test_wrappers(bmsp):
    sig = inspect.signature(bmsp.gmres_solve).parameters
    assert list(sig) == ["A", "b", "precond", "op", "restart", "max_iter", "tol", "x", "x0_given", "history", "stream"]
    assert (sig["precond"].default, sig["op"].default, sig["restart"].default, sig["max_iter"].default, sig["tol"].default,
            sig["history"].default) == (None, "N", 30, 0, 1e-6, False)
    assert list(inspect.signature(bmsp.BmSpMatrix.solve_gmres).parameters)[1:] == list(sig)[1:]
    mg = inspect.signature(bmsp.Multigrid.solve).parameters
    assert mg["restart"].default == 30 and mg["method"].default == "cg"
    assert (bmsp._gmres_restart("gmres"), bmsp._gmres_restart("gmres(7)"), bmsp._gmres_restart("cg"), bmsp._gmres_restart("gmres(x)"),
            bmsp._gmres_restart(0)) == (30, 7, None, None, None)
    with pytest.raises(ValueError):
        bmsp._precond(("ilu",))


def test_scalars_are_refused_before_handles_and_named(bmsp):
    L = bmsp.lib()
    hist = (C.c_double * 4)()
    info = bmsp.KrylovInfo()
    P = bmsp.Precond

    def solve(op=0, pc=None, restart=0, max_iter=0, tol=1e-6, flags=0, h=None, A=None, b=None, x=None):
        return L.bmsp_gmres_solve(A, op, C.byref(pc) if pc is not None else None, restart, b, x, max_iter, tol, flags, h, C.byref(info), None)

    def mg_solve(restart=0, max_iter=0, tol=1e-6, flags=0, h=None):
        return L.bmsp_mg_solve_gmres(None, restart, None, None, max_iter, tol, flags, h, C.byref(info), None)

    for kw, word in ((dict(op=2, restart=-1), "op"), (dict(op=-1), "op"), (dict(restart=-1, pc=P(4, None, 0)), "restart"),
                     (dict(restart=257, max_iter=-1), "restart"), (dict(pc=P(4, None, 0), max_iter=-1), "pc->kind"),
                     (dict(pc=P(-1, None, 0)), "pc->kind"), (dict(pc=P(3, None, 0), tol=-3.0), "pc->sweeps"),
                     (dict(max_iter=-1, tol=float("nan")), "max_iter"), (dict(max_iter=(1 << 20) + 1), "max_iter"),
                     (dict(tol=float("nan"), flags=2), "tol"), (dict(tol=-0.5), "tol"), (dict(flags=2, tol=NO_CHECK, h=hist), "flags"),
                     (dict(tol=NO_CHECK, h=hist), "relres_history")):
        assert solve(**kw) == BMSP_ERR_INVALID, kw
        assert _msg(bmsp).startswith(word), (kw, _msg(bmsp))
    for kw, word in ((dict(restart=-1, max_iter=-1), "restart"), (dict(restart=300), "restart"), (dict(max_iter=-1, tol=-0.5), "max_iter"),
                     (dict(tol=-2.0, flags=4), "tol"), (dict(flags=2), "flags"), (dict(tol=NO_CHECK, h=hist), "relres_history")):
        assert mg_solve(**kw) == BMSP_ERR_INVALID, kw
        assert _msg(bmsp).startswith(word), (kw, _msg(bmsp))
    # good scalars (the limits of restart among them): the handle is named
    for restart in (0, 1, 256):
        assert solve(restart=restart, max_iter=1 << 20, tol=NO_CHECK, op=1, flags=1, pc=P(3, None, 1)) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)
        assert mg_solve(restart=restart) == BMSP_ERR_INVALID and "mg" in _msg(bmsp)
    # bmsp_krylov_solve still knows two methods and four kinds
    assert L.bmsp_krylov_solve(None, 0, 2, None, None, None, 0, 1e-6, 0, None, None, None) == BMSP_ERR_INVALID and _msg(bmsp).startswith("method")


def build_cpp_gmres_check(out_path):
    lib_dir = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp_gmres_check.cpp"), "-o", out_path, "-L" + lib_dir, "-lbmsp",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_gmres_wrappers_compile_and_link(bmsp, tmp_path):
    """include/bmSpMatrix.h with bmSparse_solve_gmres and bmSpMultigrid::solve_gmres instantiated for float and double links against
    libbmsp.so with a plain host compiler."""
    build_cpp_gmres_check(str(tmp_path / "cpp_gmres_check"))


# ---------------------------------------------------------------------------------------------------------
# the kernels in the assembly: every instantiation is there, and none uses scratch
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gmres_asm(tmp_path_factory):
    from test_fold_handoff_asm import to_asm, functions
    path = to_asm("gmres", str(tmp_path_factory.mktemp("gmres_asm")))
    return functions(path), open(path).read()


def test_every_instantiation_is_in_the_assembly_without_scratch(gmres_asm):
    fns, text = gmres_asm
    frag = lambda name, args: "%d%sI%sE" % (len(name), name, args)
    want = []
    for s in "fd":
        want += [frag("gmres_start_kernel", "%sLi%dE" % (s, k)) for k in (0, 1)]
        want += [frag("gmres_start_finish_kernel", "%sLi%dE" % (s, k)) for k in (0, 1)]
        want += [frag("gmres_dots_kernel", "%sLi%dELb%dE" % (s, nv, t)) for nv in (1, 2, 4, 8, 16) for t in (0, 1)]
        want += [frag("gmres_update_kernel", "%sLb%dE" % (s, w)) for w in (0, 1)]
        want += [frag(k, s) for k in ("gmres_zero_x_kernel", "gmres_scale_kernel", "gmres_jacobi_kernel", "gmres_dots_finish_kernel",
                                      "gmres_scalar_kernel", "gmres_y_kernel", "gmres_xform_kernel")]
    for f in want:
        assert sum(f in n for n in fns) == 1, f
    seen = 0
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        if any(f in m.group(1) for f in want):
            seen += 1
            assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", m.group(2)), m.group(1)
    assert seen == len(want)
