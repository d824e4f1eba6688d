"""Smoothed-aggregation algebraic multigrid chained from the library's device operators: the strength filter (scale + prune), MIS(2)
aggregation (aggregate), the tentative prolongator (from_aggregates, spmv_op, scale), its smoothing (scale, spgemm, add), the Galerkin
product (transpose + two spgemm), and a host-driven V-cycle and preconditioned CG (spmv_op, vec_dot, vec_axpby).  F32 and F64 matrices;
matrices and vectors stay on the device, and nothing but the library and numpy is used: a process that has loaded the library cannot
bring in PyTorch's own HIP runtime afterwards (pybmsp's docstring), so the element-wise products with 1 / diag(A) are products with
a diagonal matrix, and the scalars of CG come back through vec_dot -- two read-backs per iteration (p.q, then r.r and r.z together).

The coarsest level is solved exactly: it has a few dozen rows (`coarse`), so its operator is expanded once on the host, inverted there in
float64 and kept as a dense bmSparse matrix that one spmv_op applies per cycle.  A fixed number of damped-Jacobi steps there would keep
the cycle symmetric too, but leaves the smooth error components of the coarsest operator in the preconditioner, and the iteration count
then grows with the grid, which the hierarchy exists to prevent.  The small host steps of the set-up are that inverse and the square
roots of the aggregate sizes (and of the diagonal when theta != 0).

The cycle and the solve driven from Python here (vcycle, pcg) are the yardstick; device_cycle hands the same hierarchy to the library's
enqueued cycle (pybmsp.Multigrid: bmsp_mg_vcycle, bmsp_mg_solve with CG or BiCGStab, bmsp_mg_solve_gmres with GMRES for a cycle or a
matrix that is not symmetric), and tools/amg_bench.py times the two against each other."""
import numpy as np

import pybmsp as B


def _vt(A):
    dtype = A.info()["dtype"]
    if dtype == B.F16:
        raise ValueError("amg: F32 or F64 matrices (the vectors of an F16 matrix have two types)")
    return np.dtype(B.OUT_DTYPE[dtype])


def _copy(src):
    dst = B.DeviceArray(src.n, src.dtype)
    if src.n:
        B.check(B.lib().bmsp_memcpy_d2d(dst.ptr, src.ptr, src.n * src.dtype.itemsize))
    return dst


def _map_host(d, fn):
    """fn applied to a short device vector on the host (set-up only)"""
    return B.DeviceArray.from_host(fn(d.to_host()).astype(d.dtype))


def strength(A, theta):
    """the strength-of-connection matrix: the entries of D^-1/2 A D^-1/2 with |s_ij| > theta, the diagonal always kept.  theta = 0
    returns A itself (aggregation reads structure only, and a stored zero counts)."""
    if theta == 0:
        return A
    s = _map_host(B.diagonal(A), lambda d: np.sqrt(np.abs(d)))
    return B.prune(B.scale(A, s, s, div_left=True, div_right=True), theta, "abs", keep_diagonal=True)[0]


def tentative(A, agg, num_agg):
    """the tentative prolongator of the constant vector: one entry 1 / sqrt(|aggregate|) per row, column-major tiles (the right operand
    of spgemm).  Unit weights first, their column sums by spmv_op(P, ones, "T"), then the columns scaled."""
    i = A.info()
    P = B.from_aggregates(agg, num_agg, None, i["num_rows"], i["dtype"], True)
    size = B.spmv_op(P, B.DeviceArray.from_host(np.ones(i["num_rows"], _vt(A))), "T")
    return B.scale(P, None, _map_host(size, np.sqrt), div_right=True)


def smooth(A, Pt, omega):
    """P = Pt - omega * D^-1 A Pt (one damped-Jacobi step on the tentative prolongator), column-major tiles"""
    DA = B.scale(A, B.diagonal(A), None, div_left=True)
    return B.add(Pt, B.spgemm(DA, Pt if Pt.info()["transposed"] else Pt.with_layout(True))[0], 1.0, -omega, transposed=True)


def galerkin(A, P):
    """(P^T A P, P^T): the coarse operator by a transpose and two spgemm, row-major tiles"""
    A0 = A if not A.info()["transposed"] else A.with_layout(False)
    P1 = P if P.info()["transposed"] else P.with_layout(True)
    R = P.transpose(False)
    AP = B.spgemm(A0, P1)[0]
    return B.spgemm(R, AP.with_layout(True))[0], R


class Level:
    """A, diag(A)^-1 as a diagonal matrix and, except on the coarsest level, P and R = P^T (row-major tiles) to the next one; on the
    coarsest level the dense inverse of A (inv: a bmSparse matrix, what vcycle applies; inv_dense: the same float64 array)"""

    def __init__(self, A):
        i = A.info()
        self.A, self.n = A, i["num_rows"]
        ones = B.DeviceArray.from_host(np.ones(self.n, _vt(A)))
        self.Dinv = B.scale(B.from_diagonal(ones, dtype=i["dtype"]), B.diagonal(A), None, div_left=True)
        self.P = self.R = self.inv = self.inv_dense = self.info = None


def build_hierarchy(A, theta=0.0, omega=2.0 / 3.0, coarse=40, max_levels=10, seed=0):
    """the levels of a smoothed-aggregation hierarchy of a square A (F32 or F64): coarsening stops at `coarse` rows or fewer, at
    max_levels, or when aggregation no longer reduces the size.  The last level carries the dense inverse of its operator."""
    if A.info()["transposed"]:
        A = A.with_layout(False)
    levels = [Level(A)]
    while levels[-1].n > coarse and len(levels) < max_levels:
        lv = levels[-1]
        agg, num_agg, info = B.aggregate(strength(lv.A, theta), seed)
        if num_agg >= lv.n or num_agg == 0:
            break
        P = smooth(lv.A, tentative(lv.A, agg, num_agg), omega)
        Ac, R = galerkin(lv.A, P)
        lv.P, lv.R, lv.info = P.with_layout(False), R, info
        levels.append(Level(Ac))
    last = levels[-1]
    r, c, v = last.A.to_coo()
    dense = np.zeros((last.n, last.n))
    dense[r, c] = v
    rr, cc = [a.ravel() for a in np.meshgrid(np.arange(last.n), np.arange(last.n), indexing="ij")]
    last.inv_dense = np.linalg.inv(dense)
    last.inv = B.BmSpMatrix.from_coo(last.n, last.n, rr, cc, last.inv_dense.ravel(), dtype=A.info()["dtype"])
    return levels


def device_cycle(levels, omega=2.0 / 3.0, pre=1, post=1):
    """the hierarchy of build_hierarchy as a pybmsp.Multigrid: the same operators (borrowed, kept alive by the object), R = P^T as built,
    the dense inverse of the coarsest level rounded to the vector type"""
    return B.Multigrid([lv.A for lv in levels], [lv.P for lv in levels[:-1]], [lv.R for lv in levels[:-1]], levels[-1].inv_dense, omega,
                       pre, post)


def _residual(lv, b, x):
    r = _copy(b)
    B.spmv_op(lv.A, x, "N", -1.0, 1.0, r)
    return r


def vcycle(levels, r, omega=2.0 / 3.0, level=0):
    """one V-cycle for A e = r from e = 0: one damped-Jacobi step before and one after (the same step: the cycle is symmetric),
    restriction and interpolation by R and P, the coarsest level by its dense inverse.  r and the result are DeviceArrays."""
    lv = levels[level]
    if lv.P is None:
        return B.spmv_op(lv.inv, r, "N")
    x = B.spmv_op(lv.Dinv, r, "N", omega)
    ec = vcycle(levels, B.spmv_op(lv.R, _residual(lv, r, x), "N"), omega, level + 1)
    B.spmv_op(lv.P, ec, "N", 1.0, 1.0, x)
    B.spmv_op(lv.Dinv, _residual(lv, r, x), "N", omega, 1.0, x)
    return x


def pcg(A, b, levels, tol=1e-6, max_iter=1000, omega=2.0 / 3.0):
    """conjugate gradients for A x = b preconditioned by one V-cycle of `levels` (None: no preconditioner), driven from Python; stops at
    dot(r, r) <= tol^2 dot(b, b), bmsp_krylov_solve's rule.  b: DeviceArray (or a numpy array) of A's vector type.  Returns
    (x DeviceArray, {"status", "iterations", "relres"}) with the status constants of bmsp_krylov_solve."""
    A0 = levels[0].A if levels else A
    if not isinstance(b, B.DeviceArray):
        b = B.DeviceArray.from_host(np.asarray(b, _vt(A)))
    apply_pc = (lambda r: vcycle(levels, r, omega)) if levels else _copy
    pair = B.DeviceArray(2, np.float64)                                 # r.r and r.z, read back together
    halves = [B.DeviceArray(1, np.float64, ptr=pair.ptr + 8 * k, owner=pair) for k in (0, 1)]
    x, r = B.DeviceArray(b.n, b.dtype), _copy(b)
    x.zero()
    bb = float(B.vec_dot(b, b).to_host()[0])
    thr, rr, it, status = tol * tol * bb, bb, 0, B.KRYLOV_MAXITER
    if rr <= thr:
        status = B.KRYLOV_CONVERGED
    else:
        z = apply_pc(r)
        p, rho = _copy(z), float(B.vec_dot(r, z).to_host()[0])
        while it < max_iter:
            q = B.spmv_op(A0, p, "N")
            alpha = rho / float(B.vec_dot(p, q).to_host()[0])
            B.vec_axpby(alpha, p, 1.0, x)
            B.vec_axpby(-alpha, q, 1.0, r)
            it += 1
            z = apply_pc(r)
            B.vec_dot(r, r, out=halves[0])
            B.vec_dot(r, z, out=halves[1])
            rr, rho_new = (float(s) for s in pair.to_host())
            if rr <= thr:
                status = B.KRYLOV_CONVERGED
                break
            B.vec_axpby(1.0, z, rho_new / rho, p)
            rho = rho_new
    return x, {"status": status, "iterations": it, "relres": float(np.sqrt(rr / bb)) if bb else 0.0}
