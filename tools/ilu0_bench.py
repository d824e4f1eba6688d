#!/usr/bin/env python3
"""Times bmsp_matrix_ilu0 / bmsp_matrix_ilu0_values (reporting only) on A = the generator's pattern with a dominant diagonal, fp32, for the
four matrix classes of tools/spitsv_bench.py:
  banded   2^17 rows, half-bandwidth 32
  fem27    fem_like 27pt (47^3 rows)
  rmat20   R-MAT 2^20 x 2 + I (the webbase-1M stand-in: a few hub block-rows and block-columns)
  rmat16   R-MAT 2^16 x 8 (hub x hub tiles: one lane group's serial chain bounds a sweep)
Per case:
  sweep_us     the time of one sweep: BMSP_ILU_NO_CHECK calls of 1 and of 33 sweeps into an existing F, HIP events around --batch calls
               after warm-up, the median of --reps samples; sweep_us = (t33 - t1) / 32, call_1_sweep_us = t1
  masked_us    bmsp_spgemm_masked_values(F, F, A -> out) on the same operands in the same session: the yardstick -- the sweep walks
               about half of its pairs (those with K <= min(I, J)) and adds the division; `pairs` is the masked product's count
  tol          for 2^-10 and 2^-20 (max_iter = --cap): sweeps, converged, the last delta / fmax and the whole call, read-backs included
  exact        tol = 0, max_iter = --cap-exact (until nothing changes): sweeps, converged, the call, and whether F then holds the bits
               of the host's sequential ILU(0) (tests/ilu0_ref.c, built here with gcc -O2 -ffp-contract=off)
  host route   what the call replaces: bmsp_matrix_to_csr_device, the three arrays copied down, the sequential factor of
               tests/ilu0_ref.c on one core, the values copied back -- wall clock, the one-off CSC index of the pattern apart.  Skipped
               (host_skipped) when the factor's merge cost, sum over the entries of len(row i) + len(column j), exceeds --host-cost.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bmsparse-spgemm-spmv_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np  # noqa: E402
import pybmsp as B  # noqa: E402
from pybmsp import gen  # noqa: E402
from spsv_bench import median_us  # noqa: E402

TOLS = (("2^-10", 2.0 ** -10), ("2^-20", 2.0 ** -20))


def ref_lib():
    so = os.path.join(tempfile.mkdtemp(prefix="ilu0_bench_"), "libilu0_ref.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(REPO, "tests", "ilu0_ref.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    L.ilu0_seq_f32.argtypes = [C.c_int64] + [C.c_void_p] * 8 + [C.c_int]
    L.ilu0_seq_f32.restype = None
    return L


def with_dominant_diagonal(n, r, c, v):
    """the off-diagonal pattern with magnitudes in [0.5, ..) and the diagonal 1 + the row's absolute sum, sorted by (row, col)"""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    key, first = np.unique(r * n + c, return_index=True)
    r, c, v = key // n, key % n, np.asarray(v, np.float64)[first]
    off = r != c
    r, c, v = r[off], c[off], v[off]
    v = np.sign(v + (v == 0)) * (0.5 + np.abs(v))
    d = 1.0 + np.bincount(r, weights=np.abs(v), minlength=n)
    e = np.arange(n, dtype=np.int64)
    r, c, v = np.concatenate([r, e]), np.concatenate([c, e]), np.concatenate([v, d])
    o = np.argsort(r * n + c, kind="stable")
    return r[o], c[o], v[o].astype(np.float32).astype(np.float64)


def wall_ms(fn):
    B.synchronize()
    t0 = time.perf_counter()
    out = fn()
    B.synchronize()
    return round((time.perf_counter() - t0) * 1e3, 3), out


def host_route(L, A, n, a):
    """(row, sequential factor in CSR order or None)"""
    out = {}

    def down():
        ro, co, va = A.to_csr_device()
        return ro.to_host().astype(np.int64), co.to_host(), va.to_host().astype(np.float32)

    out["to_csr_and_copy_down_ms"], (rowptr, col, val) = wall_ms(down)
    t0 = time.perf_counter()
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    order = np.lexsort((rows, col))
    colptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(col, minlength=n), out=colptr[1:])
    rowidx = np.ascontiguousarray(rows[order], np.int32)
    csc2csr = np.ascontiguousarray(order, np.int64)
    dpos = np.full(n, -1, np.int64)
    on = np.flatnonzero(rows == col)
    dpos[rows[on]] = on
    out["host_index_once_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    cost = int((np.diff(rowptr)[rows] + np.diff(colptr)[col]).sum())
    out["host_merge_cost"] = cost
    if cost > a.host_cost:
        out["host_skipped"] = True
        return out, None
    f = np.zeros_like(val)
    col = np.ascontiguousarray(col, np.int32)
    t0 = time.perf_counter()
    L.ilu0_seq_f32(n, rowptr.ctypes.data, col.ctypes.data, colptr.ctypes.data, rowidx.ctypes.data, csc2csr.ctypes.data, dpos.ctypes.data,
                   val.ctypes.data, f.ctypes.data, 0)
    out["host_factor_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    out["copy_back_ms"], _ = wall_ms(lambda: B.DeviceArray.from_host(f))
    out["host_route_ms"] = round(out["to_csr_and_copy_down_ms"] + out["host_factor_ms"] + out["copy_back_ms"], 3)
    return out, f


def stored(F, n):
    r, c, v = F.to_coo()
    return v[np.argsort(r.astype(np.int64) * n + c, kind="stable")].astype(np.float32)


def bench(L, name, n, r, c, v, a):
    r, c, v = with_dominant_diagonal(n, r, c, v)
    A = B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32)
    i = A.info()
    row = {"matrix": name, "dtype": "fp32", "rows": n, "nnz": i["nnz"], "tiles": i["block_num"]}
    make_ms, (F, info) = wall_ms(lambda: B.ilu0(A, max_iter=1, tol=B.ILU_NO_CHECK))
    row["first_call_ms"] = make_ms          # F, its op-T view, the diagonal index and the temporary are made here
    row["kernel"], row["view_bytes"] = info["kernel"], info["view_bytes"]
    t1 = median_us(lambda: B.ilu0_values(A, F, max_iter=1, tol=B.ILU_NO_CHECK), a.batch, a.reps, a.warmup)
    t33 = median_us(lambda: B.ilu0_values(A, F, max_iter=33, tol=B.ILU_NO_CHECK), a.batch, a.reps, a.warmup)
    row["call_1_sweep_us"], row["call_33_sweeps_us"], row["sweep_us"] = t1, t33, round((t33 - t1) / 32, 2)
    out = A.with_layout(0)
    row["pairs"] = B.spgemm_masked_launch_info(F, F, A)["pairs"]
    row["masked_us"] = median_us(lambda: B.spgemm_masked_values(out, F, F, A), a.batch, a.reps, a.warmup)
    row["sweep_over_masked"] = round(row["sweep_us"] / row["masked_us"], 2)
    row["tol"] = {}
    for label, tol in TOLS:
        _, info = B.ilu0_values(A, F, max_iter=a.cap, tol=tol)
        per = {"sweeps": info["sweeps"], "converged": info["converged"], "delta": info["delta"], "fmax": info["fmax"]}
        per["call_us"] = median_us(lambda: B.ilu0_values(A, F, max_iter=a.cap, tol=tol), a.batch, a.reps, a.warmup)
        row["tol"][label] = per
    _, info = B.ilu0_values(A, F, max_iter=a.cap_exact, tol=0.0)
    row["exact_sweeps"], row["exact_converged"] = info["sweeps"], info["converged"]
    row["exact_us"] = median_us(lambda: B.ilu0_values(A, F, max_iter=a.cap_exact, tol=0.0), 1, min(a.reps, 3), 0)
    host, f = host_route(L, A, n, a)
    row.update(host)
    if f is not None:
        row["exact_bits_equal_host"] = bool(np.array_equal(stored(F, n).view(np.uint32), f.view(np.uint32)))
        for label, _ in TOLS:
            row["tol"][label]["host_route_over_call"] = round(row["host_route_ms"] * 1e3 / row["tol"][label]["call_us"], 2)
        row["host_route_over_exact"] = round(row["host_route_ms"] * 1e3 / row["exact_us"], 2)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2, help="calls per timed sample")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cap", type=int, default=64, help="max_iter of the calls with a tolerance")
    ap.add_argument("--cap-exact", type=int, default=1024, help="max_iter of the calls run until nothing changes")
    ap.add_argument("--host-cost", type=float, default=3e9, help="merge cost above which the host factor is skipped")
    ap.add_argument("--quick", action="store_true", help="small matrices (a rehearsal of the tool, not a measurement)")
    a = ap.parse_args()
    B.set_device(0)
    L = ref_lib()
    if a.quick:
        mats = [("rmat12", lambda: gen.rmat(12, 2)), ("banded_s", lambda: gen.banded(1 << 10, 32))]
    else:
        mats = [("banded_hb32", lambda: gen.banded(1 << 17, 32)), ("fem27", lambda: gen.fem_like(47, "27pt")),
                ("rmat20 (webbase-1M-like)", lambda: gen.rmat(20, 2)), ("rmat16x8", lambda: gen.rmat(16, 8))]
    out = []
    for name, make in mats:
        n, _, r, c, v = make()
        out.append(bench(L, name, n, r, c, v, a))
        print(json.dumps(out[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"tool": "ilu0_bench", "reps": a.reps, "batch": a.batch, "cap": a.cap, "cap_exact": a.cap_exact, "results": out}))


if __name__ == "__main__":
    main()
