"""GPU tests of bmsp_vec_dot / bmsp_vec_axpby / bmsp_krylov_solve (the matrices, the C reference and the restatement are those of
tests/test_krylov_api.py).

1. the vector primitives bit for bit against tests/krylov_ref.c at the wave, chunk and second-level edges.
2. the solve bit for bit on a COLUMN-MAJOR A, where bmsp_spmv_op is a pure function of its inputs: x, iterations, status and the history
   equal the restatement's when that is driven with the library's own product, preconditioner pieces and dot product.
3. BMSP_KRYLOV_CHECK decides nothing.
4. a row-major A (the product may take a kernel with LDS float adds, so no bit claim): converged, relres <= tol, and a true residual of at
   most max(2 tol, twice the CPU restatement's true residual of the case) -- the two differ in summation order only.
5. the stops, the refusals on real handles, operands unchanged.  6. a NO_CHECK solve on a gated stream returns before the gate opens."""
import ctypes as C
import functools
import subprocess
import numpy as np
import pytest
from test_spsv_api import NP, VEC, assert_same_bits
from test_transpose import snapshot, assert_unchanged
from test_krylov_api import (CASES, PRECONDS, TOL, NO_CHECK, MAXITER, CONVERGED, BREAKDOWN, matrix, rhs, cdot, caxpby, restate, preconds_of,
                             cpu_solution, true_residual, build_cpp_krylov_check)

pytestmark = pytest.mark.gpu
FDT = {0: 0, 2: 2}                           # the factor's dtype for an A of dtype 0 / 2 unless a test says F16


def dev(bmsp, a):
    return bmsp.DeviceArray.from_host(np.ascontiguousarray(a))


def build(bmsp, name, dtype, lay):
    n, r, c, v = matrix(name, dtype if dtype != 1 else 0)
    return bmsp.BmSpMatrix.from_coo(n, n, r, c, v, transposed=bool(lay), dtype=dtype)


def factor(bmsp, name, fdtype, lay):
    """the ILU(0) factor at its fixed point, of the matrix stored in fdtype"""
    F, info = bmsp.ilu0(build(bmsp, name, fdtype, lay), max_iter=0, tol=0.0)
    assert info["converged"] == 1, info
    return F


def pc_arg(bmsp, pc, F):
    if pc == "none":
        return None
    if pc == "jacobi":
        return "jacobi"
    return ("ilu", F) if pc == "ilu" else ("ilu_sweeps", F, int(pc[len("ilu_sweeps"):]))


def gpu_callables(bmsp, A, dtype, pc, op, F):
    """the restatement's callables from the library's own calls: bmsp_spmv_op, bmsp_vec_dot, and for the preconditioner
    bmsp_matrix_diagonal + a numpy division, two bmsp_spsv, or two bmsp_spitsv"""
    matvec = lambda x: bmsp.spmv_op(A, dev(bmsp, x), op).to_host()
    dot = lambda x, y: float(bmsp.vec_dot(dev(bmsp, x), dev(bmsp, y)).to_host()[0])
    if pc == "none":
        return matvec, None, dot
    if pc == "jacobi":
        d = bmsp.diagonal(A).to_host()
        with np.errstate(all="ignore"):
            return matvec, (lambda r: r / d), dot
    first, second = (("upper", False), ("lower", True)) if op == "T" else (("lower", True), ("upper", False))
    if pc == "ilu":
        def apply(r):
            y = bmsp.spsv(F, dev(bmsp, r), op, first[0], first[1])
            return bmsp.spsv(F, y, op, second[0], second[1]).to_host()
        return matvec, apply, dot
    m = int(pc[len("ilu_sweeps"):])

    def sweeps(r):
        y = bmsp.spitsv(F, dev(bmsp, r), op, first[0], first[1], max_iter=m, tol=bmsp.ITSV_NO_CHECK)[0]
        return bmsp.spitsv(F, y, op, second[0], second[1], max_iter=m, tol=bmsp.ITSV_NO_CHECK)[0].to_host()
    return matvec, sweeps, dot


def solve(bmsp, A, b, method, pc, F, op="N", max_iter=0, tol=1e-6, x0=None, history=True, stream=None):
    dx = None if x0 is None else dev(bmsp, x0)
    out = bmsp.krylov_solve(A, dev(bmsp, b), method, pc_arg(bmsp, pc, F), op, max_iter, tol, dx, x0 is not None, history, stream)
    return (out[0].to_host(),) + tuple(out[1:])


def same_as_restatement(got, want, dtype, msg=""):
    x, info, hist = got
    wx, wits, wstatus, wrr, wbb = want
    assert (info["iterations"], info["status"]) == (wits, wstatus), (info, wits, wstatus, msg)
    assert_same_bits(x, wx, msg)
    with np.errstate(all="ignore"):
        whist = np.sqrt(np.asarray(wrr, np.float64) / wbb)
    assert hist.shape == whist.shape and np.array_equal(hist.view(np.uint64), whist.view(np.uint64)), (hist, whist, msg)
    assert info["bnorm"] == float(np.sqrt(wbb))
    if wits:
        assert info["relres"] == whist[-1]


# ---------------------------------------------------------------------------------------------------------
# 1. the vector primitives
# ---------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 262143, 262144, 262145, 262145 + 1024)


@functools.lru_cache(maxsize=None)
def vectors(n, f64, seed=0):
    """mixed signs and a range of exponents; shared, never written"""
    R = np.float64 if f64 else np.float32
    rng = np.random.default_rng(1000 * seed + n % 997 + f64)
    x = (rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-12, 12, n)).astype(R)
    y = (rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-12, 12, n)).astype(R)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def dot_bits(bmsp, x, y):
    return bmsp.vec_dot(dev(bmsp, x), dev(bmsp, y)).to_host().view(np.uint64)[0]


@pytest.mark.parametrize("finish", [None, "launch"])
@pytest.mark.parametrize("f64", [0, 1])
def test_vec_dot_bit_for_bit_at_every_edge(bmsp, monkeypatch, f64, finish):
    if finish:
        monkeypatch.setenv("BMSP_VEC_DOT_FINISH", finish)
    else:
        monkeypatch.delenv("BMSP_VEC_DOT_FINISH", raising=False)
    for n in SIZES:
        x, y = vectors(n, f64)
        want = np.float64(cdot(x, y))
        assert dot_bits(bmsp, x, y) == want.view(np.uint64), (n, want)
    # pointers one element into an allocation, and the first n entries of longer arrays
    n = 4097
    x, y = vectors(n + 1, f64)
    bx, by = dev(bmsp, x), dev(bmsp, y)
    ox = bmsp.DeviceArray(n, x.dtype, ptr=bx.ptr + x.itemsize, owner=bx)
    oy = bmsp.DeviceArray(n, y.dtype, ptr=by.ptr + y.itemsize, owner=by)
    assert bmsp.vec_dot(ox, oy).to_host()[0] == cdot(x[1:], y[1:])
    assert bmsp.vec_dot(bx, by, n=1025).to_host()[0] == cdot(x[:1025], y[:1025])
    # two consecutive calls on the same scratch with different inputs (the ticket has reset itself), results in one array each
    a, b = vectors(262145, f64, seed=1), vectors(262145 + 1024, f64, seed=2)
    da, db = [dev(bmsp, v) for v in a], [dev(bmsp, v) for v in b]
    r1 = bmsp.vec_dot(*da)
    r2 = bmsp.vec_dot(*db)
    r3 = bmsp.vec_dot(*da)
    assert (r1.to_host()[0], r2.to_host()[0], r3.to_host()[0]) == (cdot(*a), cdot(*b), cdot(*a))
    # special values
    for n in (65, 4097):
        x, y = [v.copy() for v in vectors(n, f64)]
        x[n // 2] = np.inf
        y[n // 2] = abs(y[n // 2])
        assert bmsp.vec_dot(dev(bmsp, x), dev(bmsp, y)).to_host()[0] == np.inf == cdot(x, y)
        x[n - 1] = np.nan
        assert np.isnan(bmsp.vec_dot(dev(bmsp, x), dev(bmsp, y)).to_host()[0]) and np.isnan(cdot(x, y))


@pytest.mark.parametrize("finish", [None, "ticket", "launch"])
@pytest.mark.parametrize("f64", [0, 1])
def test_vec_dot_beyond_the_ticket_threshold(bmsp, monkeypatch, f64, finish):
    """384 chunks is where the second level becomes a launch of its own: on, just above and well above it, either way forced too"""
    if finish:
        monkeypatch.setenv("BMSP_VEC_DOT_FINISH", finish)
    else:
        monkeypatch.delenv("BMSP_VEC_DOT_FINISH", raising=False)
    for n in (384 * 1024, 384 * 1024 + 1, 400 * 1024 + 77):
        x, y = vectors(n, f64)
        assert dot_bits(bmsp, x, y) == np.float64(cdot(x, y)).view(np.uint64), n


def test_vec_dot_on_two_streams_shares_nothing(bmsp):
    """dots enqueued alternately on two non-blocking streams (a scratch and a ticket per stream), of sizes that make each scratch grow"""
    import stream_gate as G
    s1, s2 = G.new_stream(), G.new_stream()
    try:
        cases = [(s1, vectors(262145, 0, seed=3)), (s2, vectors(4097, 0, seed=4)), (s1, vectors(1025, 0, seed=5)),
                 (s2, vectors(400 * 1024 + 77, 0, seed=6)), (s1, vectors(262145 + 1024, 0, seed=7)), (s2, vectors(65, 0, seed=8))]
        keep = [[dev(bmsp, v) for v in xy] for _, xy in cases]
        outs = [bmsp.vec_dot(d[0], d[1], stream=st.value) for (st, _), d in zip(cases, keep)]
        G.stream_sync(s1)
        G.stream_sync(s2)
        for (st, (x, y)), out in zip(cases, outs):
            assert out.to_host()[0] == cdot(x, y), x.size
    finally:
        G.destroy_stream(s1)
        G.destroy_stream(s2)


@pytest.mark.parametrize("f64", [0, 1])
def test_vec_axpby_bit_for_bit(bmsp, f64):
    for n in SIZES:
        x, y = vectors(n, f64)
        for a, b in ((1.7, -0.3), (-2.0 ** -7 * 3, 1.0), (0.1, 0.0), (0.0, 2.5)):
            got = bmsp.vec_axpby(a, dev(bmsp, x), b, dev(bmsp, y)).to_host()
            assert_same_bits(got, caxpby(a, x, b, y), "n %d a %r b %r" % (n, a, b))
    n = 1025
    x, y = [v.copy() for v in vectors(n + 1, f64)]
    y[5] = np.nan
    y[6] = np.inf
    x[7] = np.inf
    bx, by = dev(bmsp, x), dev(bmsp, y)
    oy = bmsp.DeviceArray(n, y.dtype, ptr=by.ptr + y.itemsize, owner=by)
    ox = bmsp.DeviceArray(n, x.dtype, ptr=bx.ptr + x.itemsize, owner=bx)
    bmsp.vec_axpby(0.5, ox, 0.0, oy)                               # b == 0: y is not read, its NaN does not propagate
    got = by.to_host()
    assert got[0] == y[0] and np.isfinite(got[5]) and np.isfinite(got[6])
    assert_same_bits(got[1:], caxpby(0.5, x[1:], 0.0, y[1:]))
    assert_same_bits(bmsp.vec_axpby(0.5, ox, 2.0, dev(bmsp, y[1:])).to_host(), caxpby(0.5, x[1:], 2.0, y[1:]))
    assert_same_bits(bmsp.vec_axpby(1.5, bx, -0.5, bx).to_host(), caxpby(1.5, x, -0.5, x))      # x == y


# ---------------------------------------------------------------------------------------------------------
# 2. the solve bit for bit on a column-major A
# ---------------------------------------------------------------------------------------------------------
GPU_PRECONDS = ("none", "jacobi", "ilu", "ilu_sweeps1", "ilu_sweeps3")
BITWISE = [(name, method, dtype, pc) for name, methods in CASES.items() for method in methods for dtype in (0, 2) for pc in GPU_PRECONDS
           if pc in preconds_of(name) or (pc == "ilu_sweeps1" and "ilu" in preconds_of(name))]


def cap(name):
    return 0 if name in ("n7", "n1") else 400


@pytest.mark.parametrize("name,method,dtype,pc", BITWISE)
def test_solve_equals_the_restatement_bit_for_bit(bmsp, monkeypatch, name, method, dtype, pc):
    monkeypatch.delenv("BMSP_KRYLOV_CHECK", raising=False)
    A = build(bmsp, name, dtype, 1)
    F = factor(bmsp, name, FDT[dtype], 1) if pc.startswith("ilu") else None
    b = rhs(name, dtype)
    snaps = [snapshot(m) for m in (A, F) if m is not None]
    got = solve(bmsp, A, b, method, pc, F, max_iter=cap(name), tol=TOL[dtype])
    want = restate(method, *gpu_callables(bmsp, A, dtype, pc, "N", F), b, None, cap(name), TOL[dtype])
    same_as_restatement(got, want, dtype, "%s %s %s" % (name, method, pc))
    info = got[1]
    assert info["status"] == CONVERGED and info["relres"] <= TOL[dtype], info
    assert info["method"] == "%s+%s" % (method, pc.rstrip("0123456789")) and info["max_iterations"] == (cap(name) or matrix(name, dtype)[0])
    k, none, two = info["iterations"], pc == "none", method == "bicgstab"
    # (BiCGStab may stop at the half step: one product, one application less)
    assert info["products"] in ((2 * k, 2 * k - 1) if two else (k,)), info
    assert info["precond_applies"] in ((0,) if none else ((2 * k, 2 * k - 1) if two else (k,))), info
    for m, s in zip([m for m in (A, F) if m is not None], snaps):
        assert_unchanged(m, s)


@pytest.mark.parametrize("name,method,pc", [("p5_12", "cg", "ilu"), ("p5_12", "bicgstab", "ilu_sweeps3"), ("ragged203", "bicgstab", "ilu"),
                                            ("rmat10", "bicgstab", "ilu_sweeps1")])
def test_an_f16_factor_under_an_f32_matrix(bmsp, name, method, pc):
    A, F = build(bmsp, name, 0, 1), factor(bmsp, name, 1, 1)
    assert F.info()["dtype"] == bmsp.F16
    b = rhs(name, 0)
    got = solve(bmsp, A, b, method, pc, F, max_iter=400, tol=TOL[0])
    same_as_restatement(got, restate(method, *gpu_callables(bmsp, A, 0, pc, "N", F), b, None, 400, TOL[0]), 0)
    assert got[1]["status"] == CONVERGED


@pytest.mark.parametrize("lay", [0, 1])     # (op T on a row-major A sweeps the view too: a pure function)
@pytest.mark.parametrize("name,method,dtype,pc", [("p5_12", "cg", 0, "jacobi"), ("ragged203", "bicgstab", 2, "ilu"),
                                                  ("rmat10", "bicgstab", 0, "ilu_sweeps3"), ("p7_6", "cg", 2, "ilu")])
def test_op_t(bmsp, name, method, dtype, pc, lay):
    A = build(bmsp, name, dtype, lay)
    F = factor(bmsp, name, FDT[dtype], lay) if pc.startswith("ilu") else None
    b = rhs(name, dtype)
    got = solve(bmsp, A, b, method, pc, F, op="T", max_iter=400, tol=TOL[dtype])
    same_as_restatement(got, restate(method, *gpu_callables(bmsp, A, dtype, pc, "T", F), b, None, 400, TOL[dtype]), dtype)
    assert got[1]["status"] == CONVERGED
    assert true_residual(name, dtype, got[0], "T") <= 2 * TOL[dtype]


@pytest.mark.parametrize("name,method,dtype,pc", [("p5_12", "cg", 0, "none"), ("p7_6", "cg", 2, "jacobi"), ("p5_12", "bicgstab", 0, "jacobi"),
                                                  ("ragged203", "bicgstab", 2, "ilu")])
def test_x0_given_max_iter_and_no_check(bmsp, name, method, dtype, pc):
    A = build(bmsp, name, dtype, 1)
    F = factor(bmsp, name, FDT[dtype], 1) if pc.startswith("ilu") else None
    b = rhs(name, dtype)
    call = gpu_callables(bmsp, A, dtype, pc, "N", F)
    tol = TOL[dtype]
    # a given start: one product more
    x0 = (np.arange(b.size) % 5 - 2).astype(VEC[dtype]) / 4
    got = solve(bmsp, A, b, method, pc, F, max_iter=400, tol=tol, x0=x0)
    want = restate(method, *call, b, x0, 400, tol)
    same_as_restatement(got, want, dtype, "x0")
    assert got[1]["status"] == CONVERGED and got[1]["products"] in ((want[1] + 1,) if method == "cg" else (2 * want[1] + 1, 2 * want[1]))
    # the exact solution of a coarser tolerance as the start: converged after 0 iterations, x untouched
    loose = solve(bmsp, A, b, method, pc, F, max_iter=400, tol=tol)
    again = solve(bmsp, A, b, method, pc, F, max_iter=400, tol=100 * tol, x0=loose[0])
    assert (again[1]["iterations"], again[1]["status"], again[2].size) == (0, CONVERGED, 0) and again[1]["relres"] <= 100 * tol
    assert_same_bits(again[0], loose[0])
    # one iteration short of the stop: MAXITER and the restatement's iterate
    its = loose[1]["iterations"]
    assert its >= 2
    short = solve(bmsp, A, b, method, pc, F, max_iter=its - 1, tol=tol)
    want = restate(method, *call, b, None, its - 1, tol)
    assert want[2] == MAXITER
    same_as_restatement(short, want, dtype, "one short")
    assert short[1]["relres"] > tol
    # NO_CHECK: exactly m iterations, nothing read back
    for m in (1, 2, 5):
        x, info = solve(bmsp, A, b, method, pc, F, max_iter=m, tol=NO_CHECK, history=False)
        want = restate(method, *call, b, None, m, NO_CHECK)
        assert want[1:3] == (m, MAXITER)
        assert_same_bits(x, want[0], "NO_CHECK %d" % m)
        assert (info["iterations"], info["status"], info["relres"], info["bnorm"]) == (m, MAXITER, -1.0, -1.0), info
    x, info = solve(bmsp, A, b, method, pc, F, max_iter=2, tol=NO_CHECK, x0=x0, history=False)
    assert_same_bits(x, restate(method, *call, b, x0, 2, NO_CHECK)[0], "NO_CHECK with x0")


@pytest.mark.parametrize("name,method,dtype,pc", [("p5_12", "cg", 0, "jacobi"), ("p7_6", "cg", 2, "ilu"), ("p5_12", "bicgstab", 0, "none"),
                                                  ("ragged203", "bicgstab", 2, "jacobi"), ("rmat10", "bicgstab", 0, "ilu_sweeps3")])
def test_second_level_by_launch_gives_the_same_solve(bmsp, monkeypatch, name, method, dtype, pc):
    """BMSP_VEC_DOT_FINISH=launch: every dot of the solve finished, and every scalar step taken, by a launch of its own"""
    A = build(bmsp, name, dtype, 1)
    F = factor(bmsp, name, FDT[dtype], 1) if pc.startswith("ilu") else None
    b = rhs(name, dtype)
    monkeypatch.delenv("BMSP_VEC_DOT_FINISH", raising=False)
    want = restate(method, *gpu_callables(bmsp, A, dtype, pc, "N", F), b, None, 400, TOL[dtype])
    x0 = (np.arange(b.size) % 5 - 2).astype(VEC[dtype]) / 4
    want0 = restate(method, *gpu_callables(bmsp, A, dtype, pc, "N", F), b, x0, 3, NO_CHECK)
    for finish in ("launch", "ticket"):
        monkeypatch.setenv("BMSP_VEC_DOT_FINISH", finish)
        same_as_restatement(solve(bmsp, A, b, method, pc, F, max_iter=400, tol=TOL[dtype]), want, dtype, finish)
        assert_same_bits(solve(bmsp, A, b, method, pc, F, max_iter=3, tol=NO_CHECK, x0=x0, history=False)[0], want0[0], finish)


@functools.lru_cache(maxsize=None)
def big_poisson():
    """5pt 640 x 640: 409 600 rows, 400 chunks -- beyond the ticket threshold"""
    from pybmsp import gen
    n, _, r, c, v = gen.poisson("5pt", 640, 640)
    rng = np.random.default_rng(3)
    b = (rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    return int(n), r, c, v, b


@pytest.mark.parametrize("method,pc", [("cg", "jacobi"), ("bicgstab", "none")])
def test_a_vector_of_more_chunks_than_the_ticket_takes(bmsp, monkeypatch, method, pc):
    """the default path of a long vector (second level by launch) and the forced ticket give the restatement's bits"""
    n, r, c, v, b = big_poisson()
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, transposed=True, dtype=bmsp.F32)
    monkeypatch.delenv("BMSP_VEC_DOT_FINISH", raising=False)
    want = restate(method, *gpu_callables(bmsp, A, 0, pc, "N", None), b, None, 3, TOL[0])
    assert want[1:3] == (3, MAXITER)
    for finish in (None, "ticket"):
        if finish:
            monkeypatch.setenv("BMSP_VEC_DOT_FINISH", finish)
        same_as_restatement(solve(bmsp, A, b, method, pc, None, max_iter=3, tol=TOL[0]), want, 0, str(finish))
        assert_same_bits(solve(bmsp, A, b, method, pc, None, max_iter=3, tol=NO_CHECK, history=False)[0], want[0], str(finish))


# ---------------------------------------------------------------------------------------------------------
# 3. BMSP_KRYLOV_CHECK decides nothing
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,method,dtype,pc", [("p5_12", "cg", 0, "jacobi"), ("p5_12", "bicgstab", 2, "none"), ("p7_6", "cg", 2, "ilu"),
                                                  ("ragged203", "bicgstab", 0, "ilu_sweeps3"), ("rmat10", "bicgstab", 0, "jacobi"),
                                                  ("n7", "cg", 0, "none"), ("ragged203", "bicgstab", 2, "none"),
                                                  ("rmat10p", "bicgstab", 0, "none")])
def test_check_interval_decides_nothing(bmsp, monkeypatch, name, method, dtype, pc):
    A = build(bmsp, name, dtype, 1)
    F = factor(bmsp, name, FDT[dtype], 1) if pc.startswith("ilu") else None
    b = rhs(name, dtype)
    outs = []
    for check in (None, "1", "3", "1000"):
        if check is None:
            monkeypatch.delenv("BMSP_KRYLOV_CHECK", raising=False)
        else:
            monkeypatch.setenv("BMSP_KRYLOV_CHECK", check)
        outs.append(solve(bmsp, A, b, method, pc, F, max_iter=cap(name), tol=TOL[dtype]))
    x, info, hist = outs[0]
    assert info["status"] == CONVERGED
    for y, i2, h2 in outs[1:]:
        assert_same_bits(y, x)
        assert i2 == info and np.array_equal(h2.view(np.uint64), hist.view(np.uint64))


# ---------------------------------------------------------------------------------------------------------
# 4. a row-major A
# ---------------------------------------------------------------------------------------------------------
ROW_MAJOR = [(name, method, dtype, pc) for name, methods in CASES.items() for method in methods for dtype in (0, 2) for pc in preconds_of(name)]


@pytest.mark.parametrize("name,method,dtype,pc", ROW_MAJOR)
def test_row_major_matrix_converges_to_the_tolerance(bmsp, monkeypatch, name, method, dtype, pc):
    monkeypatch.delenv("BMSP_KRYLOV_CHECK", raising=False)
    A = build(bmsp, name, dtype, 0)
    F = factor(bmsp, name, FDT[dtype], 0) if pc.startswith("ilu") else None
    tol = TOL[dtype]
    x, info, hist = solve(bmsp, A, rhs(name, dtype), method, pc, F, max_iter=cap(name), tol=tol)
    res, recorded = true_residual(name, dtype, x), cpu_solution(name, method, dtype, pc)[5]
    print("true residual %-9s %-8s %s %-11s iterations %3d  %.3e (CPU restatement %.3e)" % (name, method, "F64" if dtype else "F32", pc,
                                                                                           info["iterations"], res, recorded))
    assert info["status"] == CONVERGED and info["relres"] <= tol, info
    assert hist.size == info["iterations"] and hist[-1] == info["relres"] and (hist[:-1] > tol).all()
    assert res <= max(2 * tol, 2 * recorded), (res, recorded)


# ---------------------------------------------------------------------------------------------------------
# 5. stops, refusals, operands
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
@pytest.mark.parametrize("dtype", [0, 2])
def test_zero_right_hand_side_and_breakdown(bmsp, method, dtype):
    name = "p5_12"
    A = build(bmsp, name, dtype, 1)
    n = matrix(name, dtype)[0]
    zero = np.zeros(n, VEC[dtype])
    for x0 in (None, np.full(n, np.nan, VEC[dtype])):
        x, info, hist = solve(bmsp, A, zero, method, "jacobi", None, tol=TOL[dtype], x0=x0)
        assert (info["iterations"], info["status"], info["relres"], info["bnorm"], hist.size) == (0, CONVERGED, 0.0, 0.0, 0), info
        assert not x.any() and info["products"] == 0 and info["precond_applies"] == 0
    x, info = solve(bmsp, A, zero, method, "none", None, max_iter=3, tol=NO_CHECK, x0=np.ones(n, VEC[dtype]), history=False)
    assert not x.any()
    # one stored zero on the diagonal under Jacobi: IEEE gives Inf, the first denominator is not finite
    n, r, c, v = matrix(name, dtype)
    v = v.copy()
    v[(r == 77) & (c == 77)] = 0.0
    Z = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, transposed=True, dtype=dtype)
    b = rhs(name, dtype)
    x, info, hist = solve(bmsp, Z, b, method, "jacobi", None, tol=TOL[dtype])
    want = restate(method, *gpu_callables(bmsp, Z, dtype, "jacobi", "N", None), b, None, 0, TOL[dtype])
    assert want[2] == BREAKDOWN
    same_as_restatement((x, info, hist), want, dtype)
    assert info["status"] == BREAKDOWN and np.isfinite(x).all()
    x, info = solve(bmsp, Z, b, method, "jacobi", None, max_iter=4, tol=NO_CHECK, history=False)       # caught on the device too
    assert_same_bits(x, want[0])


def refused(bmsp, fn, *words, status=-1):
    with pytest.raises(bmsp.BmspError) as e:
        fn()
    assert e.value.status == status, e.value
    for w in words:
        assert w in str(e.value), (w, str(e.value))


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
        return L.bmsp_krylov_solve(A.h, kw.get("op", 0), 0, None, db, dx, kw.get("max_iter", 0), 1e-6, 0, None, None, None)

    assert call(None, x.ptr) == -1 and "d_b" in L.bmsp_last_error().decode()
    assert call(b.ptr, None) == -1 and "d_x" in L.bmsp_last_error().decode()
    assert call(b.ptr, b.ptr) == -1 and "d_x must not be d_b" in L.bmsp_last_error().decode()
    assert call(b.ptr, b.ptr, max_iter=-1) == -1 and L.bmsp_last_error().decode().startswith("max_iter")
    assert call(b.ptr, x.ptr, op=2) == -1 and L.bmsp_last_error().decode().startswith("op")
    refused(bmsp, lambda: bmsp.krylov_solve(A16, b, x=x), "F16", status=-5)
    refused(bmsp, lambda: bmsp.krylov_solve(A, b, precond=bmsp.Precond(bmsp.PC_ILU_EXACT, None, 0), x=x), "pc->F")
    refused(bmsp, lambda: bmsp.krylov_solve(A, b, precond=bmsp.Precond(bmsp.PC_ILU_SWEEPS, None, 2), x=x), "pc->F")
    refused(bmsp, lambda: bmsp.krylov_solve(A, b, precond=("ilu_sweeps", F, 0), x=x), "pc->sweeps")
    refused(bmsp, lambda: bmsp.krylov_solve(A, b, precond=("ilu", F64), x=x), "pc->F", "dtype")
    refused(bmsp, lambda: bmsp.krylov_solve(A64, b64, precond=("ilu", F)), "pc->F", "dtype")
    refused(bmsp, lambda: bmsp.krylov_solve(A64, b64, "bicgstab", precond=("ilu_sweeps", factor(bmsp, name, 1, lay), 2)), "pc->F", "dtype")
    small = factor(bmsp, "p5_12", 0, lay)
    refused(bmsp, lambda: bmsp.krylov_solve(A, b, precond=("ilu", small), x=x), "pc->F", "shape")
    e = np.arange(8)
    W = bmsp.BmSpMatrix.from_coo(8, 16, e, e, np.ones(8), transposed=bool(lay))
    refused(bmsp, lambda: bmsp.krylov_solve(W, b, x=x), "square")
    if not lay:
        refused(bmsp, lambda: bmsp.krylov_solve(A.row_panel(1, 13), b, x=x), "row-panel view")
        refused(bmsp, lambda: bmsp.krylov_solve(A, b, precond=("ilu", F.row_panel(1, 13)), x=x), "row-panel view")
    # a factor without a diagonal entry: bmsp_spsv's own message
    n, r, c, v = matrix(name, 0)
    keep = ~((r == 77) & (c == 77))
    holed = bmsp.BmSpMatrix.from_coo(n, n, r[keep], c[keep], v[keep], transposed=bool(lay))
    refused(bmsp, lambda: bmsp.krylov_solve(A, b, "bicgstab", precond=("ilu", holed)), "diag", "row 77 ")
    assert (x.to_host() == np.float32(-7.0)).all()          # nothing was done on the device
    with pytest.raises(ValueError):
        bmsp.krylov_solve(A, b, x0_given=True)
    with pytest.raises(ValueError):
        bmsp.krylov_solve(A, b64)


def test_operands_and_workspace(bmsp):
    """A, F and b are unchanged; the workspace grows to the largest need and goes with bmsp_matrix_invalidate(A, 1)"""
    name = "rmat10"
    A, F = build(bmsp, name, 0, 0), factor(bmsp, name, 0, 1)           # (a row-major A with a column-major factor)
    b = dev(bmsp, rhs(name, 0))
    sa, sf = snapshot(A), snapshot(F)
    x, i1 = bmsp.krylov_solve(A, b, "cg", "jacobi", max_iter=3, tol=TOL[0])
    x2, i2 = bmsp.krylov_solve(A, b, "bicgstab", ("ilu", F), max_iter=50, tol=TOL[0])
    x, i3 = bmsp.krylov_solve(A, b, "cg", "jacobi", max_iter=3, tol=TOL[0])
    assert i2["status"] == CONVERGED and true_residual(name, 0, x2.to_host()) <= 2 * TOL[0]
    assert 0 < i1["workspace_bytes"] < i2["workspace_bytes"] == i3["workspace_bytes"]
    bmsp.lib().bmsp_matrix_invalidate(A.h, 1)
    assert bmsp.krylov_solve(A, b, "cg", "jacobi", max_iter=3, tol=TOL[0])[1]["workspace_bytes"] == i1["workspace_bytes"]
    assert_unchanged(A, sa)
    assert_unchanged(F, sf)
    assert np.array_equal(b.to_host(), rhs(name, 0))


# ---------------------------------------------------------------------------------------------------------
# 6. the stream; the C++ wrapper
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,pc", [("cg", "jacobi"), ("bicgstab", "ilu_sweeps3"), ("cg", "ilu")])
def test_no_check_on_a_gated_stream(bmsp, method, pc):
    import stream_gate as G
    name = "p5_12"
    A = build(bmsp, name, 0, 1)
    F = factor(bmsp, name, 0, 1) if pc.startswith("ilu") else None
    n = matrix(name, 0)[0]
    b = dev(bmsp, rhs(name, 0))
    m = 4
    null = bmsp.krylov_solve(A, b, method, pc_arg(bmsp, pc, F), max_iter=m, tol=NO_CHECK)[0].to_host()       # (plans, views, workspace)
    x = dev(bmsp, np.zeros(n, np.float32))
    bmsp.synchronize()
    st, side = G.new_stream(), G.Side()
    gate = G.Gate()
    try:
        gate.close(st)
        bmsp.krylov_solve(A, b, method, pc_arg(bmsp, pc, F), max_iter=m, tol=NO_CHECK, x=x, stream=st.value)
        closed = gate.is_closed()                      # the call came back while the gate held the stream
        held = side.read(x.ptr, n, np.float32)
        still = gate.is_closed()
        gate.finish()
        assert closed, "bmsp_krylov_solve (BMSP_KRYLOV_NO_CHECK) did not return while the gate was closed"
        if still:
            assert not held.any()                      # nothing ran ahead of the gate
        assert_same_bits(x.to_host(), null)
    finally:
        gate.finish()
        side.close()
        G.destroy_stream(st)


def test_cpp_wrapper_runs(bmsp, tmp_path):
    """tests/cpp_krylov_check.cpp: bmSparse_solve and bmSparse_vec_dot for float and double on a fixture written here"""
    n, r, c, v = matrix("p5_12", 0)
    mtx = tmp_path / "spd.mtx"
    with open(mtx, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n, r.size))
        for i, j, a in zip(r, c, v):
            f.write("%d %d %.17g\n" % (i + 1, j + 1, a))
    exe = str(tmp_path / "cpp_krylov_check")
    build_cpp_krylov_check(exe)
    out = subprocess.run([exe, str(mtx)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("OK") == 2 and "FAIL" not in out.stdout, out.stdout
