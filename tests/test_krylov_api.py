"""CPU tests of the surface of bmsp_vec_dot / bmsp_vec_axpby / bmsp_krylov_solve, and what tests/test_zzzzz_krylov.py shares with them: the
test matrices, the C reference of the vector primitives (tests/krylov_ref.c through ctypes) and a numpy restatement of the two solvers
that takes the product, the preconditioner and the dot product as callables -- float32 or float64 arrays, one rounding per numpy
operation, the scalars Python doubles, the stop and breakdown rules of include/bmsp.h.

Checked here without a GPU: the prototypes, the defines and the two structs in bmsp.h; the refusals of the C entry points (scalars before
handles, the argument named); the Python and C++ wrappers; the restatement's convergence on every test case with a scipy product and the C
dot; the gfx950 assembly of krylov.hip (every instantiation present, no scratch).

True residuals ||b - A x|| / ||b|| in float64 of the restatement on the CPU (scipy product, C dot), tol = 1e-5 for F32 and 1e-10 for F64,
max_iter 400 (n for n7 and n1), as test_restatement_converges_on_every_case prints them (-s); per case: preconditioner, iterations,
true residual:
    p5_12     cg       F32  none 31 it 5.491e-06; jacobi 31 it 5.491e-06; ilu 11 it 6.020e-06; ilu_sweeps3 12 it 5.105e-06
    p5_12     cg       F64  none 44 it 5.883e-11; jacobi 44 it 5.883e-11; ilu 18 it 9.070e-11; ilu_sweeps3 19 it 5.501e-11
    p5_12     bicgstab F32  none 23 it 8.360e-06; jacobi 23 it 8.360e-06; ilu 7 it 6.371e-06; ilu_sweeps3 7 it 9.125e-06
    p5_12     bicgstab F64  none 33 it 2.510e-11; jacobi 33 it 2.510e-11; ilu 11 it 5.430e-11; ilu_sweeps3 14 it 1.795e-11
    p7_6      cg       F32  none 19 it 4.548e-06; jacobi 19 it 4.533e-06; ilu 7 it 7.690e-06; ilu_sweeps3 7 it 5.461e-06
    p7_6      cg       F64  none 29 it 4.965e-11; jacobi 29 it 4.965e-11; ilu 13 it 1.993e-11; ilu_sweeps3 13 it 6.779e-11
    p7_6      bicgstab F32  none 14 it 3.197e-06; jacobi 14 it 3.190e-06; ilu 5 it 3.438e-06; ilu_sweeps3 5 it 5.649e-06
    p7_6      bicgstab F64  none 20 it 6.610e-11; jacobi 20 it 6.610e-11; ilu 8 it 3.865e-11; ilu_sweeps3 8 it 5.073e-11
    ragged203 bicgstab F32  none 30 it 1.480e-05; jacobi 4 it 4.475e-06; ilu 2 it 3.355e-06; ilu_sweeps3 2 it 3.954e-06
    ragged203 bicgstab F64  none 55 it 7.033e-11; jacobi 9 it 2.590e-11; ilu 4 it 1.798e-11; ilu_sweeps3 4 it 1.843e-11
    rmat10    bicgstab F32  jacobi 5 it 5.009e-06; ilu 3 it 3.025e-07; ilu_sweeps3 3 it 3.089e-07
    rmat10    bicgstab F64  jacobi 10 it 3.697e-11; ilu 4 it 1.834e-11; ilu_sweeps3 4 it 1.764e-11
    rmat10p   bicgstab F32  none 41 it 8.156e-06
    rmat10p   bicgstab F64  none 67 it 8.081e-11
    n7        cg       F32  none 6 it 7.952e-06; jacobi 6 it 7.952e-06; ilu 1 it 3.307e-08; ilu_sweeps3 1 it 3.307e-08
    n7        cg       F64  none 7 it 1.533e-16; jacobi 7 it 1.533e-16; ilu 1 it 6.258e-17; ilu_sweeps3 1 it 6.258e-17
    n7        bicgstab F32  none 5 it 1.315e-06; jacobi 5 it 1.315e-06; ilu 1 it 3.307e-08; ilu_sweeps3 1 it 3.307e-08
    n7        bicgstab F64  none 7 it 9.388e-17; jacobi 7 it 9.388e-17; ilu 1 it 6.258e-17; ilu_sweeps3 1 it 6.258e-17
    n1        cg       F32  none 1 it 0.000e+00; jacobi 1 it 0.000e+00; ilu 1 it 0.000e+00; ilu_sweeps3 1 it 0.000e+00
    n1        cg       F64  none 1 it 0.000e+00; jacobi 1 it 0.000e+00; ilu 1 it 0.000e+00; ilu_sweeps3 1 it 0.000e+00
    n1        bicgstab F32  none 1 it 0.000e+00; jacobi 1 it 0.000e+00; ilu 1 it 0.000e+00; ilu_sweeps3 1 it 0.000e+00
    n1        bicgstab F64  none 1 it 0.000e+00; jacobi 1 it 0.000e+00; ilu 1 it 0.000e+00; ilu_sweeps3 1 it 0.000e+00
All are at most 1.5 tol (the closest: ragged203 bicgstab F32 none, 1.48 tol).  One case was replaced: rmat10 without a preconditioner
(preconds_of below says why and by what).  On an MI355X the row-major solves of tests/test_zzzzz_krylov.py gave the
preconditioned and the Poisson figures to two digits; the unpreconditioned BiCGStab solves on the random matrices take another
summation order to other iterates: ragged203 1.415e-05 in 30 iterations (F32) and 4.781e-11 in 56 (F64), rmat10p 6.303e-06 in 40 and
7.064e-11 in 65.
"""
import ctypes as C
import functools
import inspect
import os
import re
import subprocess
import tempfile
import numpy as np
import pytest
from conftest import REPO
from test_spsv_api import NP, VEC, pattern, reference, assert_same_bits, _msg, _flat
from test_ilu0_api import ilu_values, csr_of, ref_sequential, Csr

BMSP_ERR_INVALID = -1
NO_CHECK = -1.0
MAXITER, CONVERGED, BREAKDOWN = 0, 1, 2
TOL = {0: 1e-5, 2: 1e-10}
# name -> the methods it is solved with.  p5_12 / p7_6: cusp's Poisson stencils (symmetric positive definite); ragged203 / rmat10: the
# patterns of tests/test_ilu0_api.py with their dominant diagonals (not symmetric); rmat10p: rmat10 with the diagonal made positive; n7: one ragged tile; n1: one row.
CASES = {"p5_12": ("cg", "bicgstab"), "p7_6": ("cg", "bicgstab"), "ragged203": ("bicgstab",), "rmat10": ("bicgstab",), "rmat10p": ("bicgstab",),
         "n7": ("cg", "bicgstab"), "n1": ("cg", "bicgstab")}
PRECONDS = ("none", "jacobi", "ilu", "ilu_sweeps3")


def preconds_of(name):
    """every kind, with one replacement: without a preconditioner the restatement does not converge on rmat10 (relative residual 9e-2 in
    fp32 and 3.5e-3 in F64 after 400 iterations: the diagonal's signs are mixed), so that case is replaced by rmat10p -- the same pattern
    and off-diagonal values with the diagonal made positive, still not symmetric -- which is solved without a preconditioner only"""
    return PRECONDS[1:] if name == "rmat10" else (PRECONDS[:1] if name == "rmat10p" else PRECONDS)


@functools.lru_cache(maxsize=None)
def matrix(name, dtype):
    """(n, r, c, v) sorted by (row, col), v as float64 holding values of the dtype"""
    from pybmsp import gen
    if name in ("ragged203", "rmat10"):
        return ilu_values(name, dtype)
    if name == "rmat10p":
        n, r, c, v = ilu_values("rmat10", dtype)
        v = np.where(r == c, np.abs(v), v)
        v.setflags(write=False)
        return n, r, c, v
    grid = {"p5_12": ("5pt", 12, 12), "p7_6": ("7pt", 6, 6, 6), "n7": ("5pt", 7, 1), "n1": ("5pt", 1, 1)}[name]
    n, _, r, c, v = gen.poisson(*grid)
    r, c, v = np.asarray(r, np.int64), np.asarray(c, np.int64), np.asarray(v, np.float64)
    v.setflags(write=False)
    return int(n), r, c, v


@functools.lru_cache(maxsize=None)
def rhs(name, dtype):
    n = matrix(name, dtype)[0]
    rng = np.random.default_rng(n + 17)
    b = (rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(VEC[dtype])
    b.setflags(write=False)
    return b


# ---------------------------------------------------------------------------------------------------------
# the reference of the vector primitives
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_lib():
    d = tempfile.mkdtemp(prefix="krylov_ref_")
    so = os.path.join(d, "libkrylov_ref.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(REPO, "tests", "krylov_ref.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp, i64 = C.c_void_p, C.c_int64
    for fn in (L.vec_dot_ref_f32, L.vec_dot_ref_f64):
        fn.argtypes = [i64, vp, vp]
        fn.restype = C.c_double
    L.vec_axpby_ref_f32.argtypes = [i64, C.c_float, vp, C.c_float, vp]
    L.vec_axpby_ref_f64.argtypes = [i64, C.c_double, vp, C.c_double, vp]
    L.vec_axpby_ref_f32.restype = L.vec_axpby_ref_f64.restype = None
    return L


def cdot(x, y):
    """bmsp_vec_dot's tree on the host"""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    assert x.dtype == y.dtype and x.size == y.size
    fn = ref_lib().vec_dot_ref_f64 if x.dtype == np.float64 else ref_lib().vec_dot_ref_f32
    return float(fn(x.size, x.ctypes.data, y.ctypes.data))


def caxpby(a, x, b, y):
    x, y = np.ascontiguousarray(x), np.array(y, copy=True)
    fn = ref_lib().vec_axpby_ref_f64 if x.dtype == np.float64 else ref_lib().vec_axpby_ref_f32
    fn(x.size, x.dtype.type(a), x.ctypes.data, x.dtype.type(b), y.ctypes.data)
    return y


def test_reference_dot_is_the_tree_of_the_header():
    """against a numpy restatement of the same tree.  The inputs hold float32 values (widened for the double variant), so every product
    is exact in double and fma(x, y, acc) is fl(x * y + acc) with one rounding, which numpy's two operations give as well."""
    def tree(acc):
        w = []
        for k in range(4):
            a = acc[64 * k:64 * k + 64].copy()
            for d in (32, 16, 8, 4, 2, 1):
                a = a + a[np.arange(64) ^ d]
            w.append(a[0])
        return ((w[0] + w[1]) + w[2]) + w[3]

    rng = np.random.default_rng(5)
    for R in (np.float32, np.float64):
        for n in (0, 1, 63, 65, 1023, 1025, 4097, 262145 + 1024):
            x = (rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32).astype(R)
            y = rng.uniform(-1.0, 1.0, n).astype(np.float32).astype(R)
            chunks = (n + 1023) // 1024
            px, py = np.zeros(chunks * 1024), np.zeros(chunks * 1024)
            px[:n], py[:n] = x, y
            live = np.arange(chunks * 1024) < n
            P = np.zeros(chunks)
            for c in range(chunks):
                acc = np.zeros(256)
                for q in range(4):
                    s = slice(1024 * c + 256 * q, 1024 * c + 256 * q + 256)
                    acc = np.where(live[s], px[s] * py[s] + acc, acc)
                P[c] = tree(acc)
            want = 0.0
            if chunks:
                acc = np.zeros(256)
                for c in range(chunks):
                    acc[c % 256] = acc[c % 256] + P[c]
                want = tree(acc)
            got = cdot(x, y)
            assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (R, n, got, want)
    ones = np.ones(5000, np.float32)
    assert cdot(ones, ones) == 5000.0 and cdot(ones[:0], ones[:0]) == 0.0
    y = np.array([1.0, np.nan, 3.0], np.float32)
    assert np.array_equal(caxpby(2.0, np.ones(3, np.float32), 0.0, y), np.full(3, 2.0, np.float32))      # (b == 0: y is not read)
    assert np.isnan(caxpby(2.0, np.ones(3, np.float32), 1.0, y)[1])


# ---------------------------------------------------------------------------------------------------------
# the restatement of the two solvers
# ---------------------------------------------------------------------------------------------------------
def _bad(v):
    return v == 0.0 or not np.isfinite(v)


def restate(method, matvec, precond, dot, b, x0=None, max_iter=0, tol=1e-6):
    """CG / BiCGStab as include/bmsp.h fixes them.  matvec(v) -> op(A) v, precond(r) -> M^-1 r (None: no preconditioner), dot(x, y) ->
    float; b and x0 arrays of the vector type R.  Returns (x, iterations, status, rr_history, bb): rr_history[k] the residual dot
    recorded by iteration k + 1."""
    R = b.dtype.type
    n = b.size
    m = int(max_iter) if max_iter else min(n, 1 << 20)
    hist = []
    with np.errstate(all="ignore"):
        bb = dot(b, b)
        thr = -1.0 if tol == NO_CHECK else (tol * tol) * bb
        x = np.zeros(n, R) if x0 is None else np.array(x0, R)

        def judge(rr):
            if not np.isfinite(rr):
                return BREAKDOWN
            if rr <= thr:
                return CONVERGED
            return BREAKDOWN if rr == 0.0 else None

        if bb == 0.0:
            return np.zeros(n, R), 0, CONVERGED, hist, bb
        if not np.isfinite(bb):
            return x, 0, BREAKDOWN, hist, bb
        if x0 is None:
            r, rr = b.copy(), bb
        else:
            r = b - matvec(x)
            rr = dot(r, r)
        j = judge(rr)
        if j is not None:
            return x, 0, j, hist, bb
        if method == "cg":
            z = r if precond is None else precond(r)
            rho = rr if precond is None else dot(r, z)
            if _bad(rho):
                return x, 0, BREAKDOWN, hist, bb
            p = z.copy()
            for k in range(1, m + 1):
                q = matvec(p)
                pq = dot(p, q)
                if _bad(pq):
                    return x, k - 1, BREAKDOWN, hist, bb
                aR = R(rho / pq)
                x = x + aR * p
                r = r - aR * q
                rr = dot(r, r)
                hist.append(rr)
                j = judge(rr)
                if j is not None:
                    return x, k, j, hist, bb
                if k == m:
                    break
                z = r if precond is None else precond(r)
                rho_new = rr if precond is None else dot(r, z)
                if _bad(rho_new):
                    return x, k, BREAKDOWN, hist, bb
                beta = rho_new / rho          # (before rho is overwritten)
                rho = rho_new
                p = z + R(beta) * p
            return x, m, MAXITER, hist, bb
        rh = r.copy()
        rho = rr                              # dot(rh, r) with rh = r
        alpha = omega = beta = 0.0
        p = v = None
        for k in range(1, m + 1):
            p = r.copy() if k == 1 else r + R(beta) * (p - R(omega) * v)
            ph = p if precond is None else precond(p)
            v = matvec(ph)
            rv = dot(rh, v)
            if _bad(rv):
                return x, k - 1, BREAKDOWN, hist, bb
            alpha = rho / rv
            aR = R(alpha)
            s = r - aR * v
            x = x + aR * ph
            ss = dot(s, s)
            if not np.isfinite(ss):
                return x, k - 1, BREAKDOWN, hist, bb
            if ss <= thr:
                hist.append(ss)
                return x, k, CONVERGED, hist, bb
            if ss == 0.0:
                return x, k - 1, BREAKDOWN, hist, bb
            sh = s if precond is None else precond(s)
            t = matvec(sh)
            ts, tt = dot(t, s), dot(t, t)
            if _bad(tt):
                return x, k - 1, BREAKDOWN, hist, bb
            omega = ts / tt
            if _bad(omega):
                return x, k - 1, BREAKDOWN, hist, bb
            wR = R(omega)
            x = x + wR * sh
            r = s - wR * t
            rr, rho_new = dot(r, r), dot(rh, r)
            hist.append(rr)
            j = judge(rr)
            if j is not None:
                return x, k, j, hist, bb
            if _bad(rho_new):
                return x, k, BREAKDOWN, hist, bb
            beta = (rho_new / rho) * (alpha / omega)
            rho = rho_new
        return x, m, MAXITER, hist, bb


def true_residual(name, dtype, x, op="N"):
    import scipy.sparse as sp
    n, r, c, v = matrix(name, dtype)
    A = sp.csr_matrix((v, (r, c)), shape=(n, n))
    A = A.T if op == "T" else A
    b = rhs(name, dtype).astype(np.float64)
    return float(np.linalg.norm(b - A @ np.asarray(x, np.float64)) / np.linalg.norm(b))


def cpu_callables(name, dtype, pc, op="N"):
    """(matvec, precond) on the host: a scipy product; Jacobi by numpy; the ILU kinds by tests/ilu0_ref.c's sequential factor applied by
    tests/spsv_ref.c (exact) or tests/spitsv_ref.c (`ilu_sweeps<m>`)"""
    import scipy.sparse as sp
    R = VEC[dtype]
    n, r, c, v = matrix(name, dtype)
    A = sp.csr_matrix((v.astype(R), (r, c)), shape=(n, n))
    A = (A.T if op == "T" else A).tocsr()
    matvec = lambda x: (A @ x).astype(R)
    if pc == "none":
        return matvec, None
    if pc == "jacobi":
        d = A.diagonal().astype(R)
        return matvec, lambda x: x / d
    f = ref_sequential(Csr(n, r, c), v, dtype).astype(np.float64)
    first, second = (("upper", False), ("lower", True)) if op == "T" else (("lower", True), ("upper", False))
    if pc == "ilu":
        def apply(x):
            y = reference(n, r, c, f, dtype, op, first[0], first[1], 1.0, x)
            return reference(n, r, c, f, dtype, op, second[0], second[1], 1.0, y)
        return matvec, apply
    from test_spitsv_api import ref_sweeps
    m = int(pc[len("ilu_sweeps"):])

    def sweeps(x):
        y = ref_sweeps(n, r, c, f, dtype, op, first[0], first[1], 1.0, x, m, NO_CHECK)[0]
        return ref_sweeps(n, r, c, f, dtype, op, second[0], second[1], 1.0, y, m, NO_CHECK)[0]
    return matvec, sweeps


@functools.lru_cache(maxsize=None)
def cpu_solution(name, method, dtype, pc):
    """(x, iterations, status, rr_history, bb, true residual) of the restatement on the CPU: computed once, shared, never written"""
    matvec, precond = cpu_callables(name, dtype, pc)
    x, its, status, hist, bb = restate(method, matvec, precond, cdot, rhs(name, dtype), None, 0 if name in ("n7", "n1") else 400, TOL[dtype])
    x.setflags(write=False)
    return x, its, status, tuple(hist), bb, true_residual(name, dtype, x)


ALL_CPU = [(name, method, dtype, pc) for name, methods in CASES.items() for method in methods for dtype in (0, 2) for pc in preconds_of(name)]


@pytest.mark.parametrize("name,method,dtype,pc", ALL_CPU)
def test_restatement_converges_on_every_case(name, method, dtype, pc):
    x, its, status, hist, bb, res = cpu_solution(name, method, dtype, pc)
    print("true residual %-9s %-8s %s %-11s iterations %3d  %.3e" % (name, method, "F64" if dtype else "F32", pc, its, res))
    assert status == CONVERGED and 1 <= its <= 400, (status, its)
    assert np.isfinite(x).all() and np.isfinite(hist).all()
    assert hist[-1] <= (TOL[dtype] * TOL[dtype]) * bb and all(h > (TOL[dtype] * TOL[dtype]) * bb for h in hist[:-1])
    assert res <= 1.5 * TOL[dtype], res


def test_restatement_stops_and_breaks_down_as_the_header_says():
    name, dtype = "p5_12", 0
    matvec, _ = cpu_callables(name, dtype, "none")
    b = rhs(name, dtype)
    x, its, status, hist, bb, _ = cpu_solution(name, "cg", dtype, "none")
    # one iteration short: MAXITER with the iterate before
    y, k, st, h, _ = restate("cg", matvec, None, cdot, b, None, its - 1, TOL[dtype])
    assert (k, st) == (its - 1, MAXITER) and tuple(h) == hist[:-1]
    # NO_CHECK runs them all
    for m in (1, 2, 5):
        y, k, st, h, _ = restate("cg", matvec, None, cdot, b, None, m, NO_CHECK)
        assert (k, st) == (m, MAXITER) and tuple(h) == hist[:m]
    # b = 0
    y, k, st, h, _ = restate("bicgstab", matvec, None, cdot, np.zeros_like(b), None, 0, 1e-6)
    assert (k, st, len(h)) == (0, CONVERGED, 0) and not y.any()
    # a zero on the diagonal under Jacobi: Inf in z, the first denominator is not finite
    d = np.ones_like(b)
    d[3] = 0
    y, k, st, h, _ = restate("cg", matvec, lambda r: r / d, cdot, b, None, 0, 1e-6)
    assert (k, st) == (0, BREAKDOWN) and not y.any()
    # a start that is the solution
    y, k, st, h, _ = restate("cg", matvec, None, cdot, b, x, 0, 1e-4)
    assert (k, st) == (0, CONVERGED) and np.array_equal(y, x)


# ---------------------------------------------------------------------------------------------------------
# the entry points
# ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_interface_verbatim(bmsp):
    hdr = _flat(open(os.path.join(REPO, "include", "bmsp.h")).read())
    for line in (
            "int bmsp_vec_dot (int64_t n, int vec_f64, const void *d_x, const void *d_y, double *d_result, void *stream);".replace("dot (", "dot("),
            "int bmsp_vec_axpby(int64_t n, int vec_f64, double a, const void *d_x, double b, void *d_y, void *stream);",
            "#define BMSP_KRYLOV_CG 0", "#define BMSP_KRYLOV_BICGSTAB 1", "#define BMSP_PC_NONE 0", "#define BMSP_PC_JACOBI 1",
            "#define BMSP_PC_ILU_EXACT 2", "#define BMSP_PC_ILU_SWEEPS 3",
            "typedef struct { int kind; bmsp_matrix_t F; int64_t sweeps; } bmsp_precond;",
            "#define BMSP_KRYLOV_X0_GIVEN 1", "#define BMSP_KRYLOV_NO_CHECK (-1.0)", "#define BMSP_KRYLOV_MAXITER 0",
            "#define BMSP_KRYLOV_CONVERGED 1", "#define BMSP_KRYLOV_BREAKDOWN 2",
            "typedef struct { char method[32]; int64_t iterations, max_iterations; int status; double relres, bnorm; "
            "int64_t products, precond_applies, workspace_bytes; } bmsp_krylov_info;",
            "int bmsp_krylov_solve(bmsp_matrix_t A, int op, int method, const bmsp_precond *pc /* NULL = none */, const void *d_b, void *d_x, "
            "int64_t max_iter, double tol, int flags, double *relres_history /* host, may be NULL */, "
            "bmsp_krylov_info *info /* may be NULL */, void *stream);"):
        assert _flat(line) in hdr, line
    for phrase in ("acc = fma((double)x_i, (double)y_i, acc)", "d = 32, 16, 8, 4, 2, 1", "P[c] = ((W[0] + W[1]) + W[2]) + W[3]",
                   "n == 0 gives +0", "no floating-point atomic", "BMSP_VEC_DOT_FINISH", "BMSP_KRYLOV_CHECK", "thr = fl(fl(tol * tol) * bb)",
                   "are wasted", "max_iter == 0 means min(n, 2^20)", "One stream per handle at a time", "tests/krylov_ref.c"):
        assert _flat(phrase) in hdr, phrase
    for name in ("bmsp_vec_dot", "bmsp_vec_axpby", "bmsp_krylov_solve"):
        assert name in bmsp.SYMBOLS and hasattr(bmsp.lib(), name)


def test_struct_layouts_and_wrappers(bmsp):
    P, I = bmsp.Precond, bmsp.KrylovInfo
    assert [f[0] for f in P._fields_] == ["kind", "F", "sweeps"] and C.sizeof(P) == 24
    assert (P.kind.offset, P.F.offset, P.sweeps.offset) == (0, 8, 16)
    assert [f[0] for f in I._fields_] == ["method", "iterations", "max_iterations", "status", "relres", "bnorm", "products", "precond_applies",
                                          "workspace_bytes"]
    assert C.sizeof(I) == 96
    assert (I.iterations.offset, I.max_iterations.offset, I.status.offset, I.relres.offset, I.bnorm.offset, I.products.offset,
            I.precond_applies.offset, I.workspace_bytes.offset) == (32, 40, 48, 56, 64, 72, 80, 88)
    assert set(I().as_dict()) == {f[0] for f in I._fields_}
    assert (bmsp.KRYLOV_CG, bmsp.KRYLOV_BICGSTAB, bmsp.PC_NONE, bmsp.PC_JACOBI, bmsp.PC_ILU_EXACT, bmsp.PC_ILU_SWEEPS) == (0, 1, 0, 1, 2, 3)
    assert (bmsp.KRYLOV_X0_GIVEN, bmsp.KRYLOV_NO_CHECK, bmsp.KRYLOV_MAXITER, bmsp.KRYLOV_CONVERGED, bmsp.KRYLOV_BREAKDOWN) == (1, -1.0, 0, 1, 2)
    sig = inspect.signature(bmsp.krylov_solve).parameters
    assert list(sig) == ["A", "b", "method", "precond", "op", "max_iter", "tol", "x", "x0_given", "history", "stream"]
    assert (sig["method"].default, sig["precond"].default, sig["op"].default, sig["max_iter"].default, sig["history"].default) == \
        ("cg", None, "N", 0, False)
    assert list(inspect.signature(bmsp.BmSpMatrix.solve).parameters)[1:] == list(sig)[1:]
    assert list(inspect.signature(bmsp.vec_dot).parameters) == ["x", "y", "n", "out", "stream"]
    assert list(inspect.signature(bmsp.vec_axpby).parameters) == ["a", "x", "b", "y", "n", "stream"]
    for bad in ("ilu", ("ilu",), ("ilu_sweeps", None), 3):
        with pytest.raises(ValueError):
            bmsp._precond(bad)
    with pytest.raises(ValueError):
        bmsp.krylov_solve(None, None, method="gmres")


def test_scalars_are_refused_before_handles_and_named(bmsp):
    L = bmsp.lib()
    hist = (C.c_double * 4)()
    info = bmsp.KrylovInfo()

    def solve(op=0, method=0, pc=None, max_iter=0, tol=1e-6, flags=0, h=None, A=None, b=None, x=None):
        return L.bmsp_krylov_solve(A, op, method, C.byref(pc) if pc is not None else None, b, x, max_iter, tol, flags, h, C.byref(info), None)

    P = bmsp.Precond
    for kw, word in ((dict(op=2, method=5), "op"), (dict(op=-1), "op"), (dict(method=2, max_iter=-1), "method"), (dict(method=-1), "method"),
                     (dict(pc=P(4, None, 0), max_iter=-1), "pc->kind"), (dict(pc=P(-1, None, 0)), "pc->kind"),
                     (dict(pc=P(3, None, 0), tol=-3.0), "pc->sweeps"), (dict(pc=P(3, None, -2)), "pc->sweeps"),
                     (dict(max_iter=-1, tol=float("nan")), "max_iter"), (dict(max_iter=(1 << 20) + 1), "max_iter"),
                     (dict(tol=float("nan"), flags=2), "tol"), (dict(tol=-0.5), "tol"), (dict(tol=-2.0), "tol"),
                     (dict(flags=2, tol=NO_CHECK, h=hist), "flags"), (dict(flags=-1), "flags"), (dict(tol=NO_CHECK, h=hist), "relres_history")):
        assert solve(**kw) == BMSP_ERR_INVALID, kw
        assert _msg(bmsp).startswith(word), (kw, _msg(bmsp))
    # good scalars: the handle is named, then the vectors
    assert solve(max_iter=1 << 20, tol=NO_CHECK, method=1, op=1, flags=1, pc=P(3, None, 1)) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)
    assert solve(h=hist, pc=P(2, None, 0)) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)
    out = C.c_double()
    for kw, word in ((dict(n=-1, f64=3), "n must"), (dict(n=4, f64=2), "vec_f64"), (dict(n=4, f64=-1), "vec_f64")):
        assert L.bmsp_vec_dot(kw["n"], kw["f64"], None, None, None, None) == BMSP_ERR_INVALID and _msg(bmsp).startswith(word), kw
        assert L.bmsp_vec_axpby(kw["n"], kw["f64"], 1.0, None, 0.0, None, None) == BMSP_ERR_INVALID and _msg(bmsp).startswith(word), kw
    assert L.bmsp_vec_dot(4, 0, None, None, None, None) == BMSP_ERR_INVALID and "d_result" in _msg(bmsp)
    del out


def build_cpp_krylov_check(out_path):
    lib_dir = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp_krylov_check.cpp"), "-o", out_path, "-L" + lib_dir, "-lbmsp",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_krylov_wrappers_compile_and_link(bmsp, tmp_path):
    """include/bmSpMatrix.h with bmSparse_solve / bmSparse_vec_dot instantiated for float and double links against libbmsp.so with a
    plain host compiler."""
    build_cpp_krylov_check(str(tmp_path / "cpp_krylov_check"))


# ---------------------------------------------------------------------------------------------------------
# the kernels in the assembly: every instantiation is there, and none uses scratch
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def krylov_asm(tmp_path_factory):
    from test_fold_handoff_asm import to_asm, functions
    path = to_asm("krylov", str(tmp_path_factory.mktemp("krylov_asm")))
    return functions(path), open(path).read()


def test_every_instantiation_is_in_the_assembly_without_scratch(krylov_asm):
    fns, text = krylov_asm
    want = ["18krylov_step_kernelI%sLi%dEE" % (s, k) for s in "fd" for k in range(13)]
    want += ["20krylov_finish_kernelI%sLi%dEE" % (s, k) for s in "fd" for k in (0, 1, 3, 4, 5, 6, 9, 10, 11, 12)]      # (the steps with dots)
    want += ["14vec_dot_kernelI%sLb%dEE" % (s, t) for s in "fd" for t in (0, 1)]
    want += ["16vec_axpby_kernelI%sEE" % s for s in "fd"] + ["21vec_dot_finish_kernel"]
    for frag in want:
        assert sum(frag in n for n in fns) == 1, frag
    seen = 0
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        if any(frag in m.group(1) for frag in want):
            seen += 1
            assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", m.group(2)), m.group(1)
    assert seen == len(want)
