#!/usr/bin/env python3
"""Times bmsp_spitsv (reporting only) next to bmsp_spsv and bmsp_spmv on L = tril(A) + a dominant diagonal, for the four matrix classes of
tools/spsv_bench.py:
  banded   2^17 rows, half-bandwidth 32 (every block-row its own level: 16 384 dependent steps for the substitution)
  fem27    fem_like 27pt (47^3 rows)
  rmat20   R-MAT 2^20 x 2 + I (the webbase-1M stand-in: wide levels, a few hub block-rows)
  rmat16   R-MAT 2^16 x 8 (hub block-rows of thousands of tiles: one lane group's serial chain bounds a sweep)
Per case, fp32, for (N, lower) and (T, lower):
  sweep_us     the time of one sweep: BMSP_ITSV_NO_CHECK calls of 1 and of 33 sweeps, HIP events around --batch calls after warm-up, the
               median of --reps samples; sweep_us = (t33 - t1) / 32, call_1_sweep_us = t1 (with the zeroing of x^0 and the launch)
  tol          for 2^-10 and 2^-20 (max_iter = --cap): sweeps, converged, the last delta / xmax, and the whole call -- read-backs
               included -- for BMSP_SPITSV_CHECK in {1, 4, 8, 16, 2^31} ("all": everything enqueued at once), timed the same way; and
               its ratio to one bmsp_spsv
  exact_us     tol = 0, max_iter = 0 (until nothing changes: bmsp_spsv's bits) at the default BMSP_SPITSV_CHECK, with its sweeps
  spsv_us      one bmsp_spsv on the same triangle, same session (what the call replaces), and its levels
  spmv_us      bmsp_spmv (N) / bmsp_spmv_op (T) on the same triangle, same session (the byte floor of one sweep)
(L is row-dominant, so (N, lower) contracts; L^T is not column-dominant in general, and where the iteration does not contract the
tolerance is not met within --cap sweeps: that is reported, converged = 0, not hidden.)
Prints one JSON line."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bmsparse-spgemm-spmv_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np  # noqa: E402
import pybmsp as B  # noqa: E402
from pybmsp import gen  # noqa: E402
from spsv_bench import median_us, lower_with_dominant_diagonal  # noqa: E402

CHECKS = ("1", "4", "8", "16", str(1 << 31))
TOLS = (("2^-10", 2.0 ** -10), ("2^-20", 2.0 ** -20))


def set_check(value):
    if value is None:
        os.environ.pop("BMSP_SPITSV_CHECK", None)
    else:
        os.environ["BMSP_SPITSV_CHECK"] = value


def bench(name, n, r, c, v, a):
    r, c, v = lower_with_dominant_diagonal(n, r, c, v)
    L = B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32)
    i = L.info()
    b = B.DeviceArray.from_host(((np.arange(n) % 21) - 10).astype(np.float32))
    x = B.DeviceArray(n, np.float32)
    row = {"matrix": name, "dtype": "fp32", "rows": n, "nnz": i["nnz"], "tiles": i["block_num"], "block_rows": (n + 7) // 8}
    L.prepare(1)
    u = B.DeviceArray(n, np.float32)
    for op in ("N", "T"):
        set_check(None)
        plan = B.spsv_analyse(L, op, "lower")
        out = {"levels": plan["levels"], "spsv_launches": plan["launches"]}
        out["spsv_us"] = median_us(lambda: B.spsv(L, b, op, "lower", x=x), a.batch, a.reps, a.warmup)
        if op == "N":
            out["spmv_us"] = median_us(lambda: B.spmv(L, b, u), a.batch, a.reps, a.warmup)
        else:
            out["spmv_us"] = median_us(lambda: B.spmv_op(L, b, "T", u=u), a.batch, a.reps, a.warmup)
        t1 = median_us(lambda: B.spitsv(L, b, op, "lower", max_iter=1, tol=B.ITSV_NO_CHECK, x=x), a.batch, a.reps, a.warmup)
        t33 = median_us(lambda: B.spitsv(L, b, op, "lower", max_iter=33, tol=B.ITSV_NO_CHECK, x=x), a.batch, a.reps, a.warmup)
        out["kernel"] = B.spitsv(L, b, op, "lower", max_iter=1, tol=B.ITSV_NO_CHECK, x=x)[1]["kernel"]
        out["call_1_sweep_us"], out["call_33_sweeps_us"], out["sweep_us"] = t1, t33, round((t33 - t1) / 32, 2)
        out["sweep_over_spmv"] = round(out["sweep_us"] / out["spmv_us"], 2)
        out["spsv_over_sweep"] = round(out["spsv_us"] / out["sweep_us"], 1)
        out["tol"] = {}
        for label, tol in TOLS:
            _, info = B.spitsv(L, b, op, "lower", max_iter=a.cap, tol=tol, x=x)
            per = {"sweeps": info["sweeps"], "converged": info["converged"], "delta": info["delta"], "xmax": info["xmax"], "call_us": {}}
            for check in CHECKS:
                set_check(check)
                us = median_us(lambda: B.spitsv(L, b, op, "lower", max_iter=a.cap, tol=tol, x=x), a.batch, a.reps, a.warmup)
                per["call_us"]["all" if int(check) >= 1 << 31 else check] = us
            set_check(None)
            per["call_default_us"] = median_us(lambda: B.spitsv(L, b, op, "lower", max_iter=a.cap, tol=tol, x=x), a.batch, a.reps, a.warmup)
            per["spsv_over_call_default"] = round(out["spsv_us"] / per["call_default_us"], 2)
            out["tol"][label] = per
        _, info = B.spitsv(L, b, op, "lower", x=x)
        out["exact_sweeps"], out["exact_converged"] = info["sweeps"], info["converged"]
        if info["sweeps"] <= 4 * a.cap:
            out["exact_us"] = median_us(lambda: B.spitsv(L, b, op, "lower", x=x), a.batch, a.reps, a.warmup)
        exact = B.spsv(L, b, op, "lower").to_host()
        out["exact_bits_equal_spsv"] = bool(np.array_equal(x.to_host().view(np.uint32), exact.view(np.uint32)))
        row[op + "_lower"] = out
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2, help="calls per timed sample")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cap", type=int, default=64, help="max_iter of the calls with a tolerance")
    ap.add_argument("--quick", action="store_true", help="small matrices (a rehearsal of the tool, not a measurement)")
    a = ap.parse_args()
    B.set_device(0)
    if a.quick:
        mats = [("rmat12", lambda: gen.rmat(12, 2)), ("banded_s", lambda: gen.banded(1 << 10, 32))]
    else:
        mats = [("banded_hb32", lambda: gen.banded(1 << 17, 32)), ("fem27", lambda: gen.fem_like(47, "27pt")),
                ("rmat20 (webbase-1M-like)", lambda: gen.rmat(20, 2)), ("rmat16x8", lambda: gen.rmat(16, 8))]
    out = []
    for name, make in mats:
        n, _, r, c, v = make()
        out.append(bench(name, n, r, c, v, a))
        print(json.dumps(out[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"tool": "spitsv_bench", "reps": a.reps, "batch": a.batch, "cap": a.cap, "checks": ["1", "4", "8", "16", "all"],
                      "default_check": 8, "results": out}))


if __name__ == "__main__":
    main()
