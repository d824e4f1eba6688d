#!/usr/bin/env python3
"""Times bmsp_spsm (reporting only) next to k calls of bmsp_spsv on L = tril(A) + a dominant diagonal, for the four matrix classes of
tools/spsv_bench.py:
  banded   2^17 rows, half-bandwidth 32 (every block-row its own level: the longest dependency chain there is)
  fem27    fem_like 27pt (47^3 rows)
  rmat20   R-MAT 2^20 x 2 + I (the webbase-1M stand-in: wide levels, a few hub block-rows)
  rmat16   R-MAT 2^16 x 8 (hub block-rows of thousands of tiles)
Per case, fp32, for (N, lower) and (T, lower), at the default BMSP_SPSV_CHAIN:
  spsv_us   one bmsp_spsv: HIP events around --batch solves after warm-up, the median of --reps samples, per solve
  spsm      for k in {4, 8, 32, 128} and every lane width W that applies (BMSP_SPSM_LANES; W = 8, or at most twice k: wider slots would
            be more than half idle), the per-call time of bmsp_spsm timed the same way in the same session, and its ratio to k calls of
            bmsp_spsv, t_spsm(k) / (k * t_spsv); "default" names the width the library picks without the switch
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

KS = (4, 8, 32, 128)
WIDTHS = (8, 16, 32, 64)


def widths_for(k):
    return [w for w in WIDTHS if w == 8 or w // 2 <= k]


def bench(name, n, r, c, v, a):
    r, c, v = lower_with_dominant_diagonal(n, r, c, v)
    L = B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32)
    i = L.info()
    kmax = max(a.ks)
    pattern = ((np.arange(n * kmax, dtype=np.int64) % 21) - 10).astype(np.float32)
    Bd = B.DeviceArray.from_host(pattern)
    Xd = B.DeviceArray(n * kmax, np.float32)
    b = B.DeviceArray.from_host(pattern[:n])
    x = B.DeviceArray(n, np.float32)
    row = {"matrix": name, "rows": n, "nnz": i["nnz"], "tiles": i["block_num"], "block_rows": (n + 7) // 8}
    os.environ.pop("BMSP_SPSV_CHAIN", None)
    for op in ("N", "T"):
        os.environ.pop("BMSP_SPSM_LANES", None)
        plan = B.spsv_analyse(L, op, "lower")
        spsv_us = median_us(lambda: B.spsv(L, b, op, "lower", x=x), a.batch, a.reps, a.warmup)
        out = {"levels": plan["levels"], "launches": plan["launches"], "spsv_us": spsv_us, "spsm": {}}
        for k in a.ks:
            per_k = {"default": B.spsm_launch_info(L, op, "lower", k)["lanes"]}
            for w in widths_for(k):
                os.environ["BMSP_SPSM_LANES"] = str(w)
                us = median_us(lambda: B.spsm(L, Bd, k, op, "lower", X=Xd), a.batch, a.reps, a.warmup)
                per_k["W%d" % w] = {"us": us, "over_k_spsv": round(us / (k * spsv_us), 4)}
            os.environ.pop("BMSP_SPSM_LANES", None)
            out["spsm"]["k%d" % k] = per_k
        row[op + "_lower"] = out
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1, help="solves per timed sample")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ks", default=",".join(str(k) for k in KS), help="comma-separated numbers of right-hand sides")
    ap.add_argument("--quick", action="store_true", help="small matrices (a rehearsal of the tool, not a measurement)")
    a = ap.parse_args()
    a.ks = [int(k) for k in a.ks.split(",")]
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
    print(json.dumps({"tool": "spsm_bench", "reps": a.reps, "batch": a.batch, "ks": a.ks, "dtype": "fp32", "results": out}))


if __name__ == "__main__":
    main()
