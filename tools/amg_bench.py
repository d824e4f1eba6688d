#!/usr/bin/env python3
"""Times the device-side aggregation, the prolongator builder and the smoothed-aggregation set-up and V-cycle chained from them in
pybmsp/amg.py (reporting only), fp32, everything in one session, on
  poisson7_128  cusp's Poisson 7pt on 128^3                  poisson27_64  cusp's Poisson 27pt on 64^3
  fem27         fem_like 27pt, 47^3 rows                     banded_hb32   banded, 2^17 rows, half-bandwidth 32
(dominant diagonals on the last two, tools/ilu0_bench.py) and, for the aggregation call alone,
  rmat20        R-MAT 2^20 x 2 + I (webbase-1M-like)         rmat16x8      R-MAT 2^16 x 8 + I
where a hub row is one lane's serial walk.  Per matrix:
  aggregate        nodes, aggregates, rounds, launches; first call (builds the op-T view) and with the view cached, wall ms; the cached
                   call under BMSP_AGG_CHECK = 1 / 2 / 4 / 8 and under the other schedule (BMSP_AGG_SCHEDULE=separate: its rounds and ms)
  from_aggregates  wall ms against bmsp_matrix_from_coo_device on the same triples (already on the device), both layouts
  amg              levels and their sizes, set-up wall ms (amg.build_hierarchy), then iterations and wall ms to 1e-6 of amg.pcg (CG with one
                   V-cycle, driven from Python) next to A.solve(b, precond=None) and precond="jacobi" (the enqueued solver: CG on the
                   Poisson matrices, BiCGStab on the other two, as tools/krylov_bench.py)
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


def wall_ms(fn):
    B.synchronize()
    t0 = time.perf_counter()
    out = fn()
    B.synchronize()
    return out, round((time.perf_counter() - t0) * 1e3, 3)


def median_wall_ms(fn, reps):
    return round(statistics.median([wall_ms(fn)[1] for _ in range(reps)]), 3)


def with_env(name, value, fn):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def bench_aggregate(A, a):
    (agg, num, info), first = wall_ms(lambda: A.aggregate(0))
    row = dict(info, first_ms=first, cached_ms=median_wall_ms(lambda: A.aggregate(0), a.reps))
    row["check_ms"] = {k: with_env("BMSP_AGG_CHECK", k, lambda: median_wall_ms(lambda: A.aggregate(0), a.reps)) for k in ("1", "2", "4", "8")}
    sep = with_env("BMSP_AGG_SCHEDULE", "separate", lambda: (A.aggregate(0)[2], median_wall_ms(lambda: A.aggregate(0), a.reps)))
    row["separate"] = {"rounds": sep[0]["rounds"], "launches": sep[0]["launches"], "cached_ms": sep[1]}
    return agg, num, row


def bench_from_aggregates(agg, num, n, a):
    rows = B.DeviceArray.from_host(np.arange(n, dtype=np.int32))
    cols = B.DeviceArray.from_host(agg.to_host().astype(np.int32))
    vals = B.DeviceArray.from_host(np.ones(n))
    out = {}
    for lay in (False, True):
        direct = lambda: B.from_aggregates(agg, num, None, n, B.F32, lay)
        route = lambda: B.BmSpMatrix.from_coo_device(n, num, rows, cols, vals, lay, B.F32)
        direct(), route()
        d, r = median_wall_ms(direct, a.reps), median_wall_ms(route, a.reps)
        out["layout%d" % int(lay)] = {"ms": d, "from_coo_device_ms": r, "coo_over_direct": round(r / max(d, 1e-9), 2)}
    return out


def bench_amg(A, method, n, a):
    from pybmsp import amg
    rng = np.random.default_rng(7)
    b = B.DeviceArray.from_host(rng.uniform(-1.0, 1.0, n).astype(np.float32))
    levels, setup = wall_ms(lambda: amg.build_hierarchy(A, coarse=a.coarse))
    out = {"levels": [lv.n for lv in levels], "rounds": [lv.info["rounds"] for lv in levels if lv.info], "setup_first_ms": setup,
           "setup_ms": median_wall_ms(lambda: amg.build_hierarchy(A, coarse=a.coarse), max(1, a.reps // 2))}
    amg.pcg(A, b, levels, tol=TOL, max_iter=20)                                    # warm-up
    (_, info), ms = wall_ms(lambda: amg.pcg(A, b, levels, tol=TOL, max_iter=a.cap))
    out["vcycle_pcg"] = dict(info, ms=ms, time_to_solution_ms=round(ms + out["setup_ms"], 3))
    (_, info), ms = wall_ms(lambda: amg.pcg(A, b, None, tol=TOL, max_iter=a.cap))
    out["python_cg_none"] = dict(info, ms=ms)
    x = B.DeviceArray(n, np.float32)
    for label, pc in (("none", None), ("jacobi", "jacobi")):
        run = lambda: B.krylov_solve(A, b, method, pc, x=x, max_iter=a.cap, tol=TOL)
        run()
        (_, info) = run()
        out["solve_" + label] = {"iterations": info["iterations"], "status": info["status"], "relres": info["relres"],
                                 "ms": median_wall_ms(run, a.reps)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cap", type=int, default=2000)
    ap.add_argument("--coarse", type=int, default=200)
    ap.add_argument("--only", default="")
    ap.add_argument("--small", action="store_true", help="small shapes (a quick check of the tool itself)")
    a = ap.parse_args()
    B.set_device(0)
    if a.small:
        mats = [("poisson7_8", "cg", lambda: gen.poisson("7pt", 8, 8, 8), False, True), ("rmat10", "bicgstab", lambda: gen.rmat(10, 4), True, False)]
    else:
        mats = [("poisson7_128", "cg", lambda: gen.poisson("7pt", 128, 128, 128), False, True),
                ("poisson27_64", "cg", lambda: gen.poisson("27pt", 64, 64, 64), False, True),
                ("fem27", "bicgstab", lambda: gen.fem_like(47, "27pt"), True, True),
                ("banded_hb32", "bicgstab", lambda: gen.banded(1 << 17, 32), True, True),
                ("rmat20 (webbase-1M-like)", "bicgstab", lambda: gen.rmat(20, 2), True, False),
                ("rmat16x8", "bicgstab", lambda: gen.rmat(16, 8), True, False)]
    rows = []
    for name, method, make, dominant, whole in mats:
        if a.only and name.split()[0] not in a.only.split(","):
            continue
        n, _, r, c, v = make()
        if dominant:
            r, c, v = with_dominant_diagonal(n, r, c, v)
        A = B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32)
        row = {"matrix": name, "method": method, "rows": n, "nnz": A.info()["nnz"], "tiles": A.info()["block_num"]}
        agg, num, row["aggregate"] = bench_aggregate(A, a)
        row["from_aggregates"] = bench_from_aggregates(agg, num, n, a)
        if whole:
            row["amg"] = bench_amg(A, method, n, a)
        rows.append(row)
        print("row " + json.dumps(rows[-1]), file=sys.stderr, flush=True)          # (progress; the result is the one line on stdout)
    print(json.dumps({"tool": "amg_bench", "dtype": "fp32", "tol": TOL, "rows": rows}))


if __name__ == "__main__":
    main()
