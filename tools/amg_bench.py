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
  multigrid        the enqueued cycle (pybmsp.Multigrid on the same hierarchy: amg.device_cycle) against the Python-driven route timed in
                   the same session -- every figure {"ms": median of five runs, "min", "max"}, a run being `inner` enqueued calls and one
                   synchronisation:
                     cycle       one application, device (default restriction rule, and forced row / spmv) against amg.vcycle
                     stages      per level: bmsp_spmv_op on A, R (op N) and P (op N, into x) alone; a Jacobi step (one-level handles of one
                                 and two steps: they differ by that launch), under the default walk and under each forced one
                                 (BMSP_MG_WALK); the restriction by the row kernel and by bmsp_spmv_op inside a two-level sub-cycle
                                 (first step, residual, restriction, first step, prolongation) -- the two differ in the restriction
                                 only -- with R's tiles per block-row, what the default rule reads
                     cg          Multigrid.solve CG against amg.pcg: to TOL where CG applies, and both at a fixed 50 iterations
                                 (tol = 0) for the time per iteration on every matrix
                     bicgstab    Multigrid.solve BiCGStab to TOL (the method for the matrices that are not symmetric)
                     gmres       Multigrid.solve GMRES(--restart) to TOL: one cycle per iteration where BiCGStab takes two
  --gmres            only the solves: BiCGStab and GMRES(--restart) under Jacobi and under the cycle (no aggregation, stage or crossover rows)
  restrict_crossover   the restriction on synthetic operators of 12 / 24 / 48 / 96 tiles per block-row of R, row mode under each walk
                   against spmv mode: where the default rule's threshold comes from
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


def spread(fn, inner=1, runs=5):
    """{"ms": median, "min", "max"} per call over `runs` runs of `inner` calls and one synchronisation each"""
    t = []
    for _ in range(runs):
        B.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        B.synchronize()
        t.append((time.perf_counter() - t0) * 1e3 / inner)
    return {"ms": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}


def bench_krylov_on_cycle(mg, n, b, setup_ms, create, a):
    """BiCGStab and GMRES(--restart) preconditioned by one cycle, to TOL: the two methods for matrices that are not symmetric"""
    out = {}
    x = B.DeviceArray(n, np.float32)
    for label, run in (("bicgstab", lambda: mg.solve(b, "bicgstab", a.cap, TOL, x)),
                       ("gmres", lambda: mg.solve(b, "gmres", a.cap, TOL, x, restart=a.restart))):
        run()
        info = run()[1]
        out[label] = {"iterations": info["iterations"], "status": info["status"], "relres": info["relres"], "products": info["products"],
                      "precond_applies": info["precond_applies"], **spread(run)}
        out[label]["time_to_solution_ms"] = round(out[label]["ms"] + setup_ms + create, 3)
    return out


def bench_multigrid(A, levels, method, n, b, setup_ms, a):
    from pybmsp import amg
    out = {}
    mg, create = wall_ms(lambda: amg.device_cycle(levels))
    if a.gmres:
        return bench_krylov_on_cycle(mg, n, b, setup_ms, create, a)
    info = mg.info()
    out["create_ms"] = create
    out["info"] = {k: info[k] for k in ("n", "restrict_mode", "launches_per_cycle", "workspace_bytes", "kernel", "coarse_kernel")}
    z = B.DeviceArray(n, np.float32)
    mg.vcycle(b, z)
    amg.vcycle(levels, b)
    out["cycle"] = {"device": spread(lambda: mg.vcycle(b, z), 20), "python": spread(lambda: amg.vcycle(levels, b), 3)}
    for mode in ("row", "spmv"):
        with_env("BMSP_MG_RESTRICT", mode, lambda: mg.vcycle(b, z))
        out["cycle"]["device_" + mode] = with_env("BMSP_MG_RESTRICT", mode, lambda: spread(lambda: mg.vcycle(b, z), 20))
    out["cycle"]["python_over_device"] = round(out["cycle"]["python"]["ms"] / max(out["cycle"]["device"]["ms"], 1e-9), 2)
    stages = []
    for l, lv in enumerate(levels):
        v = B.DeviceArray.from_host(np.linspace(-1.0, 1.0, lv.n).astype(np.float32))
        u = B.DeviceArray(lv.n, np.float32)
        st = {"level": l, "n": lv.n, "A_tiles_per_block_row": round(lv.A.info()["block_num"] / max((lv.n + 7) // 8, 1), 2)}
        B.spmv_op(lv.A, v, "N", 1.0, 0.0, u)
        st["spmv_op_A"] = spread(lambda: B.spmv_op(lv.A, v, "N", 1.0, 0.0, u), 20)
        # one-level handles that differ by exactly one launch, a Jacobi step of the row kernel (the residual is the same walk with a plain
        # store): both timings as measured, their difference, and the step under every walk
        one, two = B.Multigrid([lv.A], [], pre=1, post=0), B.Multigrid([lv.A], [], pre=2, post=0)
        one.vcycle(v, u), two.vcycle(v, u)
        t1, t2 = spread(lambda: one.vcycle(v, u), 20), spread(lambda: two.vcycle(v, u), 20)
        st["first_step"], st["first_plus_jacobi_step"] = t1, t2
        st["jacobi_step_ms"] = round(t2["ms"] - t1["ms"], 4)
        st["walk"] = two.info()["kernel"]
        st["jacobi_step_by_walk_ms"] = {}
        for walk in ("group1", "group4", "wave"):
            with_env("BMSP_MG_WALK", walk, lambda: two.vcycle(v, u))
            tw = with_env("BMSP_MG_WALK", walk, lambda: spread(lambda: two.vcycle(v, u), 20))
            st["jacobi_step_by_walk_ms"][walk] = round(tw["ms"] - t1["ms"], 4)
        if lv.P is not None:
            nc = levels[l + 1].n
            vc, uc = B.DeviceArray.from_host(np.linspace(-1.0, 1.0, nc).astype(np.float32)), B.DeviceArray(nc, np.float32)
            st["R_tiles_per_block_row"] = round(lv.R.info()["block_num"] / max((nc + 7) // 8, 1), 2)
            B.spmv_op(lv.R, v, "N", 1.0, 0.0, uc), B.spmv_op(lv.P, vc, "N", 1.0, 1.0, u)
            st["spmv_op_R"] = spread(lambda: B.spmv_op(lv.R, v, "N", 1.0, 0.0, uc), 20)
            st["spmv_op_P_into_x"] = spread(lambda: B.spmv_op(lv.P, vc, "N", 1.0, 1.0, u), 20)
            sub = B.Multigrid([lv.A, levels[l + 1].A], [lv.P], [lv.R], pre=1, post=0)
            for mode in ("row", "spmv"):
                with_env("BMSP_MG_RESTRICT", mode, lambda: sub.vcycle(v, u))
                st["sub_cycle_" + mode] = with_env("BMSP_MG_RESTRICT", mode, lambda: spread(lambda: sub.vcycle(v, u), 20))
            st["restrict_row_minus_spmv_ms"] = round(st["sub_cycle_row"]["ms"] - st["sub_cycle_spmv"]["ms"], 4)
        stages.append(st)
    out["stages"] = stages
    x = B.DeviceArray(n, np.float32)
    # CG: to TOL (meaningful where A is symmetric), and both drivers at a fixed 50 iterations for the time per iteration
    run = lambda: mg.solve(b, "cg", a.cap, TOL, x)
    run()
    info = run()[1]
    out["cg"] = {"iterations": info["iterations"], "status": info["status"], "relres": info["relres"], **spread(run)}
    out["cg"]["time_to_solution_ms"] = round(out["cg"]["ms"] + setup_ms + create, 3)
    fixed_dev = lambda: mg.solve(b, "cg", 50, 0.0, x)
    fixed_py = lambda: amg.pcg(A, b, levels, tol=0.0, max_iter=50)
    d_it, p_it = fixed_dev()[1]["iterations"], fixed_py()[1]["iterations"]
    d, p = spread(fixed_dev), spread(fixed_py)
    out["cg_fixed50"] = {"device": dict(d, iterations=d_it), "python_pcg": dict(p, iterations=p_it),
                         "device_ms_per_iteration": round(d["ms"] / max(d_it, 1), 4), "python_ms_per_iteration": round(p["ms"] / max(p_it, 1), 4)}
    out["cg_fixed50"]["python_over_device_per_iteration"] = round(out["cg_fixed50"]["python_ms_per_iteration"] /
                                                                  max(out["cg_fixed50"]["device_ms_per_iteration"], 1e-9), 2)
    out.update(bench_krylov_on_cycle(mg, n, b, setup_ms, create, a))
    return out


def bench_restrict_crossover(a):
    """the restriction alone on synthetic operators of exactly 12 / 24 / 48 / 96 tiles per block-row of R (8 192 block-rows, eight entries
    per tile): the two-level sub-cycle (first step, residual, restriction, first step, prolongation) on identity level operators under
    row mode with each walk and under spmv mode -- the runs differ in the restriction only"""
    out = []
    nc = 65536
    for tpb in (12, 24, 48, 96):
        n0 = nc * tpb
        i = np.repeat(np.arange(nc), tpb)
        j = (i // 8) * 8 * tpb + 8 * np.tile(np.arange(tpb), nc) + i % 8
        R = B.BmSpMatrix.from_coo(nc, n0, i, j, np.full(i.size, 0.25), dtype=B.F32)
        P = B.BmSpMatrix.from_coo(n0, nc, j, i, np.full(i.size, 0.25), dtype=B.F32)
        A0 = B.BmSpMatrix.from_coo(n0, n0, np.arange(n0), np.arange(n0), np.ones(n0), dtype=B.F32)
        A1 = B.BmSpMatrix.from_coo(nc, nc, np.arange(nc), np.arange(nc), np.ones(nc), dtype=B.F32)
        sub = B.Multigrid([A0, A1], [P], [R], pre=1, post=0)
        v, u = B.DeviceArray.from_host(np.linspace(-1.0, 1.0, n0).astype(np.float32)), B.DeviceArray(n0, np.float32)
        row = {"R_tiles_per_block_row": round(R.info()["block_num"] / (nc // 8), 2), "n0": n0, "n1": nc}
        for label, env in (("spmv", {"BMSP_MG_RESTRICT": "spmv"}), ("row_group1", {"BMSP_MG_RESTRICT": "row", "BMSP_MG_WALK": "group1"}),
                           ("row_group4", {"BMSP_MG_RESTRICT": "row", "BMSP_MG_WALK": "group4"}),
                           ("row_wave", {"BMSP_MG_RESTRICT": "row", "BMSP_MG_WALK": "wave"}), ("default", {})):
            old = {k: os.environ.get(k) for k in ("BMSP_MG_RESTRICT", "BMSP_MG_WALK")}
            for k in old:
                os.environ.pop(k, None)
            os.environ.update(env)
            try:
                sub.vcycle(v, u)
                row[label] = spread(lambda: sub.vcycle(v, u), 20)
                if label == "default":
                    row["default_mode"] = sub.info()["restrict_mode"]
            finally:
                for k, val in old.items():
                    os.environ.pop(k, None)
                    if val is not None:
                        os.environ[k] = val
        out.append(row)
    return out


def bench_amg(A, method, n, a):
    from pybmsp import amg
    rng = np.random.default_rng(7)
    b = B.DeviceArray.from_host(rng.uniform(-1.0, 1.0, n).astype(np.float32))
    levels, setup = wall_ms(lambda: amg.build_hierarchy(A, coarse=a.coarse))
    out = {"levels": [lv.n for lv in levels], "rounds": [lv.info["rounds"] for lv in levels if lv.info], "setup_first_ms": setup,
           "setup_ms": median_wall_ms(lambda: amg.build_hierarchy(A, coarse=a.coarse), max(1, a.reps // 2))}
    if a.gmres:
        x = B.DeviceArray(n, np.float32)
        for label, run in (("bicgstab_jacobi", lambda: B.krylov_solve(A, b, "bicgstab", "jacobi", x=x, max_iter=a.cap, tol=TOL)),
                           ("gmres_jacobi", lambda: B.gmres_solve(A, b, "jacobi", restart=a.restart, x=x, max_iter=a.cap, tol=TOL))):
            run()
            info = run()[1]
            out[label] = {"iterations": info["iterations"], "status": info["status"], "relres": info["relres"], "ms": median_wall_ms(run, a.reps)}
        out["multigrid"] = bench_multigrid(A, levels, method, n, b, out["setup_ms"], a)
        return out
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
    out["multigrid"] = bench_multigrid(A, levels, method, n, b, out["setup_ms"], a)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cap", type=int, default=2000)
    ap.add_argument("--coarse", type=int, default=200)
    ap.add_argument("--only", default="")
    ap.add_argument("--small", action="store_true", help="small shapes (a quick check of the tool itself)")
    ap.add_argument("--gmres", action="store_true", help="only the solves: BiCGStab and GMRES(--restart) under Jacobi and under the cycle")
    ap.add_argument("--restart", type=int, default=30)
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
        if not a.gmres:
            agg, num, row["aggregate"] = bench_aggregate(A, a)
            row["from_aggregates"] = bench_from_aggregates(agg, num, n, a)
        if whole:
            row["amg"] = bench_amg(A, method, n, a)
        rows.append(row)
        print("row " + json.dumps(rows[-1]), file=sys.stderr, flush=True)          # (progress; the result is the one line on stdout)
    out = {"tool": "amg_bench", "dtype": "fp32", "tol": TOL, "rows": rows}
    if not a.gmres and (not a.only or "crossover" in a.only.split(",")):
        out["restrict_crossover"] = bench_restrict_crossover(a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
