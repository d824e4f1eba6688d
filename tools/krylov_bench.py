#!/usr/bin/env python3
"""Times bmsp_krylov_solve (reporting only): time to solution of op(A) x = b at tol = 1e-6, fp32 and F64, for
  CG        on cusp's Poisson 27pt 64^3 and 7pt 128^3
  BiCGStab  on the README's banded_hb32 (2^17 rows) and fem27 (fem_like 27pt, 47^3 rows) patterns with their dominant diagonals, and on
            R-MAT 2^16 x 8 (hub block-rows)
under each preconditioner: none, jacobi, ilu (bmsp_spsv on the factor at its fixed point -- bmsp_matrix_ilu0 with tol = 0, at most
--fixed-cap sweeps) and ilu_sweeps m in {2, 4, 8} (bmsp_spitsv on a factor of 6 NO_CHECK ILU(0) sweeps).  Per case:
  iterations, status, relres   of the checked call (max_iter = --cap; ilu: --exact-cap, a triangular solve there is a chain of thousands
                               of dependent steps)
  setup_ms                     wall time of the factorisation (0 for none / jacobi: the diagonal is taken inside the call)
  iter_us                      one iteration in NO_CHECK mode: (t(17 iterations) - t(1 iteration)) / 16, HIP events, median of --reps
  call_us                      the whole checked call at the default read-back schedule (batches of 1, 2, 4, 8, then 16 iterations),
                               read-backs included, HIP events around it
  check_us                     the same for BMSP_KRYLOV_CHECK in {1, 4, 8, 16, all} ("all": --cap iterations enqueued at once); a case
                               that does not converge within --cap is reported with the wall time of its one call and nothing else
  host_loop                    the route a user had before: the same algorithm driven from Python -- the library's calls for products and
                               preconditioners, torch for dots and updates, one .item() per iteration: iterations, total and per iteration
                               (wall clock; not for ilu, whose solves dominate either way)
--gmres times bmsp_gmres_solve instead: GMRES(--restart) against BiCGStab with the same preconditioner on all five matrices, the checked
call at the default read-back schedule (iterations, status, relres, call_us, time_to_solution_ms; iter_us of GMRES from NO_CHECK runs of
one and of two full cycles).  --ortho times the orthogonalisation: one iteration of GMRES at basis size j + 1 on a diagonal matrix
(t(j + 1 iterations) - t(j iterations) under NO_CHECK, the median of 8 * reps + 1 back-to-back pairs: the product of one entry per row, two passes of dots and updates, the scalar
kernel, the normalisation) under BMSP_GMRES_GROUP in {4, 8, 16}, against the same two passes assembled from public calls -- j + 1
bmsp_vec_dot and j + 1 bmsp_vec_axpby each -- for j in {7, 15, 29} and n in {2^18, 2^21}, fp32.
--fsai times the FSAI preconditioner (bmsp_fsai_*), fp32, on the five matrices: the pattern is tril(A), thinned by fsai_pattern(A, theta)
with the smallest theta of 0, 0.02, 0.05, 0.1, 0.2, 0.4 at which no row exceeds 64 entries; per matrix theta, the longest row, W, the set-up
(pattern_ms, create_ms: factors, transposes and views; wall clock), one application against two bmsp_spmv_op on tril(A) and against
Jacobi's (the difference of a NO_CHECK iteration with jacobi and with none), and CG (symmetric matrices, SPD kind) / BiCGStab / GMRES(30)
(GENERAL kind) against none and jacobi: iterations, call_us, time to solution with and without set-up.  lanes_us: bmsp_matrix_fsai_values
under BMSP_FSAI_LANES in {default, 16, 32, 64}.
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

CHECKS = ("1", "4", "8", "16", str(1 << 31))
TOL = 1e-6


def set_check(value):
    if value is None:
        os.environ.pop("BMSP_KRYLOV_CHECK", None)
    else:
        os.environ["BMSP_KRYLOV_CHECK"] = value


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


def host_loop(torch, A, method, apply_pc, b_t, tol, cap):
    """the same algorithm with the host in the loop: torch tensors wrapped as DeviceArrays for the library's calls"""
    wrap = lambda t: B.DeviceArray(t.numel(), np.float64 if t.dtype == torch.float64 else np.float32, ptr=t.data_ptr(), owner=t)
    new = lambda: torch.empty_like(b_t)
    matvec = lambda src, dst: B.spmv_op(A, wrap(src), "N", u=wrap(dst))
    x, r = torch.zeros_like(b_t), b_t.clone()
    thr = tol * tol * float(torch.dot(b_t, b_t))
    z, q = new(), new()
    pc = (lambda src, dst: dst.copy_(src)) if apply_pc is None else (lambda src, dst: apply_pc(wrap(src), wrap(dst)))
    its = 0
    if method == "cg":
        pc(r, z)
        p = z.clone()
        rho = torch.dot(r, z)
        while its < cap:
            matvec(p, q)
            alpha = rho / torch.dot(p, q)
            x.add_(p * alpha)
            r.sub_(q * alpha)
            its += 1
            if torch.dot(r, r).item() <= thr:
                break
            pc(r, z)
            rho_new = torch.dot(r, z)
            p = z + p * (rho_new / rho)
            rho = rho_new
        return its
    rh, p, v, s, t, ph, sh = r.clone(), r.clone(), new(), new(), new(), new(), new()
    rho = torch.dot(rh, r)
    while its < cap:
        pc(p, ph)
        matvec(ph, v)
        alpha = rho / torch.dot(rh, v)
        s = r - v * alpha
        pc(s, sh)
        matvec(sh, t)
        omega = torch.dot(t, s) / torch.dot(t, t)
        x.add_(ph * alpha + sh * omega)
        r = s - t * omega
        its += 1
        if torch.dot(r, r).item() <= thr:
            break
        rho_new = torch.dot(rh, r)
        p = r + (p - v * omega) * ((rho_new / rho) * (alpha / omega))
        rho = rho_new
    return its


def bench(name, method, n, r, c, v, dtype, a, torch):
    R = np.float64 if dtype == B.F64 else np.float32
    A = B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=dtype)
    i = A.info()
    row = {"matrix": name, "method": method, "dtype": "fp64" if dtype == B.F64 else "fp32", "rows": n, "nnz": i["nnz"], "pc": {}}
    rng = np.random.default_rng(7)
    hb = rng.uniform(-1.0, 1.0, n).astype(R)
    b, x = B.DeviceArray.from_host(hb), B.DeviceArray(n, R)
    u = B.DeviceArray(n, R)
    row["spmv_us"] = event_us(lambda: B.spmv_op(A, b, "N", u=u), a.reps, 3)
    row["dot_us"] = {}
    for mode in ("ticket", "launch"):
        os.environ["BMSP_VEC_DOT_FINISH"] = mode
        out = B.DeviceArray(1, np.float64)
        row["dot_us"][mode] = round(event_us(lambda: [B.vec_dot(b, u, out=out) for _ in range(20)], a.reps, 2) / 20, 2)
    os.environ.pop("BMSP_VEC_DOT_FINISH", None)
    sweeps6, t6 = wall_ms(lambda: B.ilu0(A, max_iter=6, tol=B.ILU_NO_CHECK)[0])
    (fixed, finfo), tfix = wall_ms(lambda: B.ilu0(A, max_iter=a.fixed_cap, tol=0.0))
    row["ilu_fixed_point"] = {"sweeps": finfo["sweeps"], "converged": finfo["converged"], "ms": tfix}
    kinds = [("none", None, 0.0, a.cap), ("jacobi", "jacobi", 0.0, a.cap)]
    kinds += [("ilu_sweeps%d" % m, ("ilu_sweeps", sweeps6, m), t6, a.cap) for m in (2, 4, 8)]
    kinds += [("ilu", ("ilu", fixed), tfix, a.exact_cap)]
    for label, pc, setup, cap in kinds:
        set_check(None)
        run = lambda **kw: B.krylov_solve(A, b, method, pc, x=x, **kw)
        (_, info), first_ms = wall_ms(lambda: run(max_iter=cap, tol=TOL))          # (builds plans and views)
        per = {"iterations": info["iterations"], "status": info["status"], "relres": info["relres"], "setup_ms": setup,
               "products": info["products"], "precond_applies": info["precond_applies"]}
        if label != "ilu" and info["status"] != B.KRYLOV_CONVERGED:
            per["call_us"] = round(first_ms * 1e3, 1)                              # (not converged within --cap: the one call, no sweep over CHECK)
        elif label != "ilu":
            t1 = event_us(lambda: run(max_iter=1, tol=B.KRYLOV_NO_CHECK), a.reps)
            t17 = event_us(lambda: run(max_iter=17, tol=B.KRYLOV_NO_CHECK), a.reps)
            per["iter_us"] = round((t17 - t1) / 16, 2)
            per["call_us"] = event_us(lambda: run(max_iter=cap, tol=TOL), a.reps)
            per["check_us"] = {}
            for check in CHECKS:
                set_check(check)
                per["check_us"]["all" if int(check) >= 1 << 31 else check] = event_us(lambda: run(max_iter=cap, tol=TOL), a.reps)
            set_check(None)
            if torch is not None and label in ("none", "jacobi", "ilu_sweeps4"):
                bt = torch.from_numpy(hb).cuda()
                if label == "none":
                    apply_pc = None
                elif label == "jacobi":
                    d = torch.from_numpy(B.diagonal(A).to_host()).cuda()
                    apply_pc = lambda src, dst: torch.div(src._owner, d, out=dst._owner)
                else:
                    tmp = B.DeviceArray(n, R)

                    def apply_pc(src, dst, F=sweeps6, m=4):
                        B.spitsv(F, src, "N", "lower", True, max_iter=m, tol=B.ITSV_NO_CHECK, x=tmp)
                        B.spitsv(F, tmp, "N", "upper", False, max_iter=m, tol=B.ITSV_NO_CHECK, x=dst)
                host_loop(torch, A, method, apply_pc, bt, TOL, min(cap, 20))      # warm-up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hits = host_loop(torch, A, method, apply_pc, bt, TOL, cap)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e6
                per["host_loop"] = {"iterations": hits, "total_us": round(dt, 1), "iter_us": round(dt / max(hits, 1), 2)}
                per["host_over_library_per_iteration"] = round(per["host_loop"]["iter_us"] / max(per["call_us"] / max(info["iterations"], 1), 1e-9), 2)
        else:
            per["call_us"] = round(first_ms * 1e3, 1)                              # (one call: the solves are tens of milliseconds each)
        per["time_to_solution_ms"] = round(setup + per["call_us"] / 1e3, 3)
        row["pc"][label] = per
    return row


def bench_gmres(name, n, r, c, v, dtype, a):
    R = np.float64 if dtype == B.F64 else np.float32
    A = B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=dtype)
    row = {"matrix": name, "dtype": "fp64" if dtype == B.F64 else "fp32", "rows": n, "nnz": A.info()["nnz"], "restart": a.restart, "pc": {}}
    hb = np.random.default_rng(7).uniform(-1.0, 1.0, n).astype(R)
    b, x = B.DeviceArray.from_host(hb), B.DeviceArray(n, R)
    sweeps6, t6 = wall_ms(lambda: B.ilu0(A, max_iter=6, tol=B.ILU_NO_CHECK)[0])
    (fixed, finfo), tfix = wall_ms(lambda: B.ilu0(A, max_iter=a.fixed_cap, tol=0.0))
    kinds = [("none", None, 0.0, a.cap), ("jacobi", "jacobi", 0.0, a.cap)]
    kinds += [("ilu_sweeps%d" % m, ("ilu_sweeps", sweeps6, m), t6, a.cap) for m in (2, 4, 8)]
    kinds += [("ilu", ("ilu", fixed), tfix, a.exact_cap)]
    set_check(None)
    for label, pc, setup, cap in kinds:
        per = {"setup_ms": setup}
        for method, run in (("bicgstab", lambda **kw: B.krylov_solve(A, b, "bicgstab", pc, x=x, **kw)),
                            ("gmres", lambda **kw: B.gmres_solve(A, b, pc, restart=a.restart, x=x, **kw))):
            (_, info), first_ms = wall_ms(lambda: run(max_iter=cap, tol=TOL))      # (builds plans and views)
            m = {"iterations": info["iterations"], "status": info["status"], "relres": info["relres"], "products": info["products"],
                 "precond_applies": info["precond_applies"]}
            m["call_us"] = round(first_ms * 1e3, 1) if label == "ilu" else event_us(lambda: run(max_iter=cap, tol=TOL), a.reps)
            if method == "gmres" and label != "ilu":
                t1 = event_us(lambda: run(max_iter=a.restart, tol=B.KRYLOV_NO_CHECK), a.reps)
                t2 = event_us(lambda: run(max_iter=2 * a.restart, tol=B.KRYLOV_NO_CHECK), a.reps)
                m["iter_us"] = round((t2 - t1) / a.restart, 2)                      # (the mean over a cycle, its restart included)
            m["time_to_solution_ms"] = round(setup + m["call_us"] / 1e3, 3)
            per[method] = m
        row["pc"][label] = per
    return row


def bench_fsai(name, method, n, r, c, v, a):
    R = np.float32
    A = B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32)
    row = {"matrix": name, "dtype": "fp32", "rows": n, "nnz": A.info()["nnz"]}
    hb = np.random.default_rng(7).uniform(-1.0, 1.0, n).astype(R)
    b, x, z = B.DeviceArray.from_host(hb), B.DeviceArray(n, R), B.DeviceArray(n, R)
    symmetric = method == "cg"
    kind = "spd" if symmetric else "general"
    S = f = None
    for theta in (0.0, 0.02, 0.05, 0.1, 0.2, 0.4):
        S, row["pattern_ms"] = wall_ms(lambda: B.fsai_pattern(A, theta))
        try:
            f, row["create_ms"] = wall_ms(lambda: B.Fsai(A, S, kind))
        except B.BmspError as e:
            if e.status != -6:
                raise
            continue
        row["theta"] = theta
        break
    if f is None:
        row["error"] = "no theta up to 0.4 leaves rows of at most 64 entries"
        return row
    fi = f.info()["factor"][0]
    row.update({"pattern_nnz": S.info()["nnz"], "max_row": fi["max_row"], "lanes": fi["lanes"], "kernel": fi["kernel"], "bad_rows": fi["bad_rows"],
                "setup_ms": round(row["pattern_ms"] + row["create_ms"], 3)})
    G = B.fsai(A, S, "N", "sqrt")[0]
    row["lanes_us"] = {}
    for lanes in (None, "16", "32", "64"):
        if lanes is None:
            os.environ.pop("BMSP_FSAI_LANES", None)
        else:
            os.environ["BMSP_FSAI_LANES"] = lanes
        row["lanes_us"]["default" if lanes is None else lanes] = event_us(lambda: B.fsai_values(A, G, "N", "sqrt"), a.reps, 2)
    os.environ.pop("BMSP_FSAI_LANES", None)
    row["apply_us"] = event_us(lambda: f.apply(b, z), a.reps, 3)
    view = B.Fsai(A, S, kind, materialise=False)
    row["apply_no_materialise_us"] = event_us(lambda: view.apply(b, z), a.reps, 3)
    del view
    row["two_spmv_tril_us"] = event_us(lambda: (B.spmv_op(S, b, "N", u=z), B.spmv_op(S, z, "N", u=x)), a.reps, 3)
    row["spmv_us"] = event_us(lambda: B.spmv_op(A, b, "N", u=z), a.reps, 3)
    set_check(None)
    methods = (["cg"] if symmetric else []) + ["bicgstab", "gmres"]
    row["solve"] = {}
    handles = {"spd": f} if symmetric else {"general": f}
    if symmetric:
        handles["general"], row["create_general_ms"] = wall_ms(lambda: B.Fsai(A, S, "general"))
    for m in methods:
        per = {}
        h = handles["spd" if m == "cg" else "general"]
        setup = row["pattern_ms"] + (row["create_general_ms"] if symmetric and m != "cg" else row["create_ms"])
        runs = {"none": lambda **kw: (B.gmres_solve(A, b, None, restart=a.restart, x=x, **kw) if m == "gmres" else B.krylov_solve(A, b, m, None, x=x, **kw)),
                "jacobi": lambda **kw: (B.gmres_solve(A, b, "jacobi", restart=a.restart, x=x, **kw) if m == "gmres" else B.krylov_solve(A, b, m, "jacobi", x=x, **kw)),
                "fsai": lambda **kw: (h.solve_gmres(b, a.restart, x=x, **kw) if m == "gmres" else h.solve(b, m, x=x, **kw))}
        for label, run in runs.items():
            (_, info), first_ms = wall_ms(lambda: run(max_iter=a.cap, tol=TOL))
            q = {"iterations": info["iterations"], "status": info["status"], "relres": info["relres"]}
            q["call_us"] = event_us(lambda: run(max_iter=a.cap, tol=TOL), a.reps)
            steps = a.restart if m == "gmres" else 16
            t1 = event_us(lambda: run(max_iter=steps, tol=B.KRYLOV_NO_CHECK), a.reps)
            t2 = event_us(lambda: run(max_iter=2 * steps, tol=B.KRYLOV_NO_CHECK), a.reps)
            q["iter_us"] = round((t2 - t1) / steps, 2)
            q["time_to_solution_ms"] = round((setup if label == "fsai" else 0.0) + q["call_us"] / 1e3, 3)
            per[label] = q
        per["jacobi_apply_us"] = round((per["jacobi"]["iter_us"] - per["none"]["iter_us"]) / (2 if m == "bicgstab" else 1), 2)
        row["solve"][m] = per
    return row


def paired_us(short, long, pairs):
    """median over `pairs` of t(long) - t(short), the two timed back to back with HIP events"""
    e = [B.Event() for _ in range(3)]
    short(), long()
    B.synchronize()
    d = []
    for _ in range(pairs):
        e[0].record()
        short()
        e[1].record()
        long()
        e[2].record()
        B.synchronize()
        d.append((e[1].elapsed_ms(e[2]) - e[0].elapsed_ms(e[1])) * 1e3)
    return round(statistics.median(d), 1)


def bench_ortho(a):
    rows = []
    for n in (1 << 18, 1 << 21):
        e = np.arange(n)
        A = B.BmSpMatrix.from_coo(n, n, e, e, np.full(n, 1.5), dtype=B.F32)
        rng = np.random.default_rng(3)
        b, x = B.DeviceArray.from_host(rng.uniform(-1.0, 1.0, n).astype(np.float32)), B.DeviceArray(n, np.float32)
        w = B.DeviceArray.from_host(rng.uniform(-1.0, 1.0, n).astype(np.float32))
        out = B.DeviceArray(1, np.float64)
        run = lambda m: B.gmres_solve(A, b, None, restart=32, max_iter=m, tol=B.KRYLOV_NO_CHECK, x=x)
        run(32)
        for j in (7, 15, 29):
            def public():
                for _ in range(2):
                    for _ in range(j + 1):
                        B.vec_dot(b, w, out=out)
                    for _ in range(j + 1):
                        B.vec_axpby(-1e-3, b, 1.0, w)
            row = {"n": n, "j": j, "public_calls_us": event_us(public, a.reps, 2), "gmres_step_us": {}}
            for group in ("4", "8", "16"):
                os.environ["BMSP_GMRES_GROUP"] = group
                row["gmres_step_us"][group] = paired_us(lambda: run(j), lambda: run(j + 1), 8 * a.reps + 1)
            os.environ.pop("BMSP_GMRES_GROUP", None)
            rows.append(row)
            print("row " + json.dumps(row), file=sys.stderr, flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gmres", action="store_true", help="GMRES(--restart) against BiCGStab, time to solution")
    ap.add_argument("--ortho", action="store_true", help="the orthogonalisation step against public calls")
    ap.add_argument("--fsai", action="store_true", help="the FSAI preconditioner against none and jacobi, fp32")
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cap", type=int, default=2000)
    ap.add_argument("--exact-cap", type=int, default=40)
    ap.add_argument("--fixed-cap", type=int, default=64)
    ap.add_argument("--only", default="")
    ap.add_argument("--dtypes", default="fp32,fp64")
    ap.add_argument("--small", action="store_true", help="small shapes (a quick check of the tool itself)")
    a = ap.parse_args()
    try:
        import torch
        if not torch.cuda.is_available():
            torch = None
    except ImportError:
        torch = None
    B.set_device(0)
    if a.ortho:
        print(json.dumps({"tool": "krylov_bench", "mode": "ortho", "rows": bench_ortho(a)}))
        return
    if a.small:
        mats = [("poisson27_8", "cg", lambda: gen.poisson("27pt", 8, 8, 8), False), ("banded_small", "bicgstab", lambda: gen.banded(1 << 10, 8), True)]
    else:
        mats = [("poisson27_64", "cg", lambda: gen.poisson("27pt", 64, 64, 64), False),
                ("poisson7_128", "cg", lambda: gen.poisson("7pt", 128, 128, 128), False),
                ("banded_hb32", "bicgstab", lambda: gen.banded(1 << 17, 32), True), ("fem27", "bicgstab", lambda: gen.fem_like(47, "27pt"), True),
                ("rmat16x8", "bicgstab", lambda: gen.rmat(16, 8), True)]
    rows = []
    for name, method, make, dominant in mats:
        if a.only and name not in a.only.split(","):
            continue
        n, _, r, c, v = make()
        if dominant:
            r, c, v = with_dominant_diagonal(n, r, c, v)
        if a.fsai:
            rows.append(bench_fsai(name, method, n, r, c, v, a))
            print("row " + json.dumps(rows[-1]), file=sys.stderr, flush=True)
            continue
        for dt in a.dtypes.split(","):
            if a.gmres:
                rows.append(bench_gmres(name, n, r, c, v, B.F64 if dt == "fp64" else B.F32, a))
                print("row " + json.dumps(rows[-1]), file=sys.stderr, flush=True)
                continue
            rows.append(bench(name, method, n, r, c, v, B.F64 if dt == "fp64" else B.F32, a, torch))
            print("row " + json.dumps(rows[-1]), file=sys.stderr, flush=True)          # (progress; the result is the one line on stdout)
    print(json.dumps({"tool": "krylov_bench", "tol": TOL, "check_default": "1, 2, 4, 8, then 16 per batch", "torch": torch is not None, "rows": rows}))


if __name__ == "__main__":
    main()
