#!/usr/bin/env python3
"""Times the block multi-colour ordering and what it does to the solver stack (reporting only), fp32, everything in one session, on
  banded_hb32  banded, 2^17 rows, half-bandwidth 32          fem27     fem_like 27pt, 47^3 rows
  rmat20       R-MAT 2^20 x 2 + I (webbase-1M-like)          rmat16x8  R-MAT 2^16 x 8 + I
  poisson7_128 cusp's Poisson 7pt on 128^3
with dominant diagonals on the first four (tools/ilu0_bench.py).  A = the matrix, B = P A P^T by A.reorder_multicolor().  Per matrix:
  color         blocks, colors, rounds; the colouring's first call (builds the op-T view) and with the view cached, wall ms
  permute       bmsp_matrix_permute_blocks(A, perm, perm), wall ms, against the route it replaces: to_coo_device + a torch gather through
                the inverse permutation + from_coo_device (when torch sees the GPU)
  spsv          levels and us of bmsp_spsv on tril of A and of B, op N and op T (HIP events, median of --reps)
  ilu0          sweeps of bmsp_matrix_ilu0 to the bitwise fixed point (tol = 0, at most --fixed-cap) on A and on B, wall ms
  krylov        bmsp_krylov_solve at tol = 1e-6 (CG on Poisson, BiCGStab elsewhere) under none, jacobi, ilu_sweeps (m = 4 on a factor of 6
                NO_CHECK sweeps) and ilu (exact solves on the fixed-point factor; at most --exact-cap iterations) on A and on B:
                iterations, status, setup_ms (factorisation; for B plus colouring, permutation and the two vector permutations) and
                time_to_solution_ms = setup + the checked call
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bmsparse-spgemm-spmv_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np  # noqa: E402
import pybmsp as B  # noqa: E402
from pybmsp import gen  # noqa: E402
from ilu0_bench import with_dominant_diagonal  # noqa: E402

TOL = 1e-6


def event_us(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    B.synchronize()
    e0, e1 = B.Event(), B.Event()
    samples = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        B.synchronize()
        samples.append(e0.elapsed_ms(e1) * 1e3)
    return round(statistics.median(samples), 1)


def wall_ms(fn):
    B.synchronize()
    t0 = time.perf_counter()
    out = fn()
    B.synchronize()
    return out, round((time.perf_counter() - t0) * 1e3, 3)


def median_wall_ms(fn, reps):
    return round(statistics.median([wall_ms(fn)[1] for _ in range(reps)]), 3)


def coo_route(torch, A, perm_host):
    """the route permute_blocks replaces, on the device: COO out, indices through the inverse permutation, the builder"""
    i = A.info()
    inv = np.empty(perm_host.size, np.int64)
    inv[perm_host.astype(np.int64)] = np.arange(perm_host.size)
    inv_t = torch.from_numpy(inv).cuda()
    wrap = lambda t, dt: B.DeviceArray(t.numel(), dt, ptr=t.data_ptr(), owner=t)

    def run():
        r, c, v = A.to_coo_device()
        tr = torch.empty(r.n, dtype=torch.int32, device="cuda")     # (torch's view of the two index arrays: one device copy each)
        tc = torch.empty(c.n, dtype=torch.int32, device="cuda")
        B.check(B.lib().bmsp_memcpy_d2d(tr.data_ptr(), r.ptr, 4 * r.n))
        B.check(B.lib().bmsp_memcpy_d2d(tc.data_ptr(), c.ptr, 4 * c.n))
        r2 = (inv_t[(tr >> 3).long()] * 8 + (tr & 7)).int()
        c2 = (inv_t[(tc >> 3).long()] * 8 + (tc & 7)).int()
        torch.cuda.synchronize()
        return B.BmSpMatrix.from_coo_device(i["num_rows"], i["num_cols"], wrap(r2, np.int32), wrap(c2, np.int32), v, dtype=i["dtype"])

    return run


def solves(M, b, method, a, extra_setup_ms, fixed, t_fixed, sweeps6, t6, wrap_rhs=None):
    """iterations and time to solution of the four preconditioners on M"""
    n = M.info()["num_rows"]
    x = B.DeviceArray(n, np.float32)
    out = {}
    for label, pc, setup, cap in (("none", None, 0.0, a.cap), ("jacobi", "jacobi", 0.0, a.cap),
                                  ("ilu_sweeps4", ("ilu_sweeps", sweeps6, 4), t6, a.cap), ("ilu", ("ilu", fixed), t_fixed, a.exact_cap)):
        run = lambda: B.krylov_solve(M, b, method, pc, x=x, max_iter=cap, tol=TOL)
        (_, info), first_ms = wall_ms(run)                        # (builds plans and views)
        call_ms = first_ms
        if label != "ilu" and info["status"] == B.KRYLOV_CONVERGED:
            call_ms = round(event_us(run, a.reps) / 1e3, 3)
        out[label] = {"iterations": info["iterations"], "status": info["status"], "relres": info["relres"],
                      "setup_ms": round(setup + extra_setup_ms, 3), "call_ms": call_ms,
                      "time_to_solution_ms": round(setup + extra_setup_ms + call_ms, 3)}
    return out


def bench(name, method, n, r, c, v, a, torch):
    A = B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32)
    row = {"matrix": name, "method": method, "rows": n, "nnz": A.info()["nnz"], "tiles": A.info()["block_num"]}
    # the colouring: first call (view missing), then cached
    (_, perm, info), first = wall_ms(lambda: A.color_blocks(0))
    row["color"] = dict(info, first_ms=first, cached_ms=median_wall_ms(lambda: A.color_blocks(0), a.reps))
    # the permutation and the route it replaces
    Bm, t_perm = wall_ms(lambda: A.permute_blocks(perm, perm))
    row["permute"] = {"first_ms": t_perm, "ms": median_wall_ms(lambda: A.permute_blocks(perm, perm), a.reps)}
    if torch is not None:
        route = coo_route(torch, A, perm.to_host())
        route()
        row["permute"]["coo_route_ms"] = median_wall_ms(route, a.reps)
        row["permute"]["coo_route_over_permute"] = round(row["permute"]["coo_route_ms"] / max(row["permute"]["ms"], 1e-9), 2)
    rng = np.random.default_rng(7)
    hb = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    b = B.DeviceArray.from_host(hb)
    bp, xp = B.DeviceArray(n, np.float32), B.DeviceArray(n, np.float32)
    row["vec_permute_us"] = event_us(lambda: B.vec_permute_blocks(perm, b, False, bp), a.reps, 2)
    # triangular solves
    row["spsv"] = {}
    for label, M, rhs in (("A", A, b), ("B", Bm, bp)):
        for op in ("N", "T"):
            lv = B.spsv_analyse(M, op, "lower")["levels"]
            row["spsv"]["%s_%s" % (label, op)] = {"levels": lv, "us": event_us(lambda: B.spsv(M, rhs, op, "lower", x=xp), a.reps)}
    # ILU(0) to the bitwise fixed point, and the six-sweep factor the sweep preconditioner uses
    row["ilu0"], fac = {}, {}
    for label, M in (("A", A), ("B", Bm)):
        (fixed, finfo), t_fixed = wall_ms(lambda: B.ilu0(M, max_iter=a.fixed_cap, tol=0.0))
        sweeps6, t6 = wall_ms(lambda: B.ilu0(M, max_iter=6, tol=B.ILU_NO_CHECK)[0])
        row["ilu0"][label] = {"sweeps": finfo["sweeps"], "converged": finfo["converged"], "ms": t_fixed, "six_sweeps_ms": t6}
        fac[label] = (fixed, t_fixed, sweeps6, t6)
    # Krylov: B pays for colouring, permutation and the two vector permutations
    reorder_ms = row["color"]["first_ms"] + row["permute"]["first_ms"] + 2 * row["vec_permute_us"] / 1e3
    row["reorder_setup_ms"] = round(reorder_ms, 3)
    row["krylov"] = {"A": solves(A, b, method, a, 0.0, *fac["A"]), "B": solves(Bm, bp, method, a, reorder_ms, *fac["B"])}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cap", type=int, default=2000)
    ap.add_argument("--exact-cap", type=int, default=40)
    ap.add_argument("--fixed-cap", type=int, default=64)
    ap.add_argument("--only", default="")
    ap.add_argument("--small", action="store_true", help="small shapes (a quick check of the tool itself)")
    a = ap.parse_args()
    try:
        import torch
        if not torch.cuda.is_available():
            torch = None
    except ImportError:
        torch = None
    B.set_device(0)
    if a.small:
        mats = [("poisson7_8", "cg", lambda: gen.poisson("7pt", 8, 8, 8), False), ("banded_small", "bicgstab", lambda: gen.banded(1 << 10, 8), True)]
    else:
        mats = [("banded_hb32", "bicgstab", lambda: gen.banded(1 << 17, 32), True), ("fem27", "bicgstab", lambda: gen.fem_like(47, "27pt"), True),
                ("rmat20 (webbase-1M-like)", "bicgstab", lambda: gen.rmat(20, 2), True), ("rmat16x8", "bicgstab", lambda: gen.rmat(16, 8), True),
                ("poisson7_128", "cg", lambda: gen.poisson("7pt", 128, 128, 128), False)]
    rows = []
    for name, method, make, dominant in mats:
        if a.only and name.split()[0] not in a.only.split(","):
            continue
        n, _, r, c, v = make()
        if dominant:
            r, c, v = with_dominant_diagonal(n, r, c, v)
        rows.append(bench(name, method, n, r, c, v, a, torch))
        print("row " + json.dumps(rows[-1]), file=sys.stderr, flush=True)          # (progress; the result is the one line on stdout)
    print(json.dumps({"tool": "reorder_bench", "dtype": "fp32", "tol": TOL, "torch": torch is not None, "rows": rows}))


if __name__ == "__main__":
    main()
