#!/usr/bin/env python3
"""Times bmsp_spsv (reporting only) on L = tril(A) + a dominant diagonal for four matrix classes:
  banded   2^17 rows, half-bandwidth 32 (every block-row its own level: the longest dependency chain there is)
  fem27    fem_like 27pt (47^3 rows)
  rmat20   R-MAT 2^20 x 2 + I (the webbase-1M stand-in: wide levels, a few hub block-rows)
  rmat16   R-MAT 2^16 x 8 (hub block-rows of thousands of tiles)
Per case:
  plan      levels, widest level, a histogram of level widths (in block-rows), launches per BMSP_SPSV_CHAIN value
  analysis  host clock of bmsp_spsv_analyse on a fresh copy of L, for (N, lower) -- block pointer and other-index column to the host, one
            levelling pass, upload -- and for (T, lower), which builds the op-T view first
  solve     HIP events around --batch solves after warm-up, the median of --reps samples, per solve, for every BMSP_SPSV_CHAIN value of
            the sweep (0 = one launch per level; the plan is rebuilt per value) on (N, lower); (T, lower) at the default
  floor     bmsp_spmv on the same L (prepared): it moves the same bytes without the dependencies
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bmsparse-spgemm-spmv_amd"))
import numpy as np  # noqa: E402
import pybmsp as B  # noqa: E402
from pybmsp import gen  # noqa: E402

CHAINS = ("0", "32", "64", "128", "256", "1024", str(1 << 31))
DT = {B.F32: "fp32", B.F16: "fp16", B.F64: "fp64"}


def median_us(fn, batch, reps, warmup):
    for _ in range(warmup):
        fn()
    B.synchronize()
    e0, e1 = B.Event(), B.Event()
    samples = []
    for _ in range(reps):
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        samples.append(e0.elapsed_ms(e1) * 1e3 / batch)
    return round(statistics.median(samples), 2)


def wall_ms(fn):
    B.synchronize()
    t0 = time.perf_counter()
    fn()
    B.synchronize()
    return round((time.perf_counter() - t0) * 1e3, 3)


def lower_with_dominant_diagonal(n, r, c, v):
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    low = r > c
    r, c, v = r[low], c[low], np.asarray(v, np.float64)[low]
    v = np.sign(v + (v == 0)) * (0.5 + np.abs(v))
    d = 1.0 + np.bincount(r, weights=np.abs(v), minlength=n)
    e = np.arange(n, dtype=np.int64)
    return np.concatenate([r, e]), np.concatenate([c, e]), np.concatenate([v, d])


def width_histogram(n, r, c):
    blocks = (n + 7) // 8
    key = np.unique((r // 8) * blocks + c // 8)
    ptr = np.zeros(blocks + 1, np.uint32)
    np.cumsum(np.bincount(key // blocks, minlength=blocks), out=ptr[1:])
    _, _, lp, _ = B.spsv_plan(ptr, (key % blocks).astype(np.uint32), 1, 0)
    w = np.diff(lp.astype(np.int64))
    edges = [(1, 1), (2, 8), (9, 32), (33, 64), (65, 256), (257, 1024), (1025, 1 << 62)]
    hist = {("%d" % lo if lo == hi else ("%d+" % lo if hi > 1 << 40 else "%d-%d" % (lo, hi))): int(((w >= lo) & (w <= hi)).sum()) for lo, hi in edges}
    return hist, {("%d" % lo if lo == hi else ("%d+" % lo if hi > 1 << 40 else "%d-%d" % (lo, hi))): int(w[(w >= lo) & (w <= hi)].sum())
                  for lo, hi in edges}


def bench(name, n, r, c, v, dtype, a):
    r, c, v = lower_with_dominant_diagonal(n, r, c, v)
    L = B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=dtype)
    i = L.info()
    vt = B.OUT_DTYPE[dtype]
    b = B.DeviceArray.from_host(((np.arange(n) % 21) - 10).astype(vt))
    x = B.DeviceArray(n, vt)
    levels, rows_by_width = width_histogram(n, r, c)
    row = {"matrix": name, "dtype": DT[dtype], "rows": n, "nnz": i["nnz"], "tiles": i["block_num"], "block_rows": (n + 7) // 8,
           "levels_by_width": levels, "block_rows_by_level_width": rows_by_width}
    os.environ.pop("BMSP_SPSV_CHAIN", None)
    row["analysis_ms"] = {"N_lower": statistics.median(wall_ms(lambda F=L.clone(): B.spsv_analyse(F, "N", "lower")) for _ in range(a.shots)),
                          "T_lower": statistics.median(wall_ms(lambda F=L.clone(): B.spsv_analyse(F, "T", "lower")) for _ in range(a.shots))}
    sweep = {}
    for chain in CHAINS:
        os.environ["BMSP_SPSV_CHAIN"] = chain
        L.invalidate(True)
        info = B.spsv_analyse(L, "N", "lower")
        us = median_us(lambda: B.spsv(L, b, "N", "lower", x=x), a.batch, a.reps, a.warmup)
        sweep["all" if int(chain) >= 1 << 31 else chain] = {"us": us, "launches": info["launches"], "chain_launches": info["chain_launches"],
                                                           "chained_levels": info["chained_levels"]}
        row["levels"], row["max_level_width"], row["plan_bytes"], row["kernel"] = info["levels"], info["max_level_width"], info["plan_bytes"], info["kernel"]
    del os.environ["BMSP_SPSV_CHAIN"]
    row["solve_N_lower_by_chain"] = sweep
    L.invalidate(True)
    row["default"] = B.spsv_analyse(L, "N", "lower")
    row["solve_N_lower_us"] = median_us(lambda: B.spsv(L, b, "N", "lower", x=x), a.batch, a.reps, a.warmup)
    row["solve_T_lower_us"] = median_us(lambda: B.spsv(L, b, "T", "lower", x=x), a.batch, a.reps, a.warmup)
    v_in = B.DeviceArray.from_host(((np.arange(n) % 21) - 10).astype(B.NP_DTYPE[dtype]))
    L.prepare(1)
    u = B.DeviceArray(n, vt)
    row["spmv_same_triangle_us"] = median_us(lambda: B.spmv(L, v_in, u), a.batch, a.reps, a.warmup)
    row["solve_over_spmv"] = round(row["solve_N_lower_us"] / row["spmv_same_triangle_us"], 1)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2, help="solves per timed sample")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shots", type=int, default=3, help="analysis repetitions")
    ap.add_argument("--dtypes", default="fp32", help="comma-separated: fp32, fp16, fp64")
    ap.add_argument("--quick", action="store_true", help="small matrices (a rehearsal of the tool, not a measurement)")
    a = ap.parse_args()
    B.set_device(0)
    if a.quick:
        mats = [("rmat12", lambda: gen.rmat(12, 2)), ("banded_s", lambda: gen.banded(1 << 10, 32))]
    else:
        mats = [("banded_hb32", lambda: gen.banded(1 << 17, 32)), ("fem27", lambda: gen.fem_like(47, "27pt")),
                ("rmat20 (webbase-1M-like)", lambda: gen.rmat(20, 2)), ("rmat16x8", lambda: gen.rmat(16, 8))]
    names = {v: k for k, v in DT.items()}
    out = []
    for name, make in mats:
        n, _, r, c, v = make()
        for d in a.dtypes.split(","):
            out.append(bench(name, n, r, c, v, names[d.strip()], a))
            print(json.dumps(out[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"tool": "spsv_bench", "reps": a.reps, "batch": a.batch, "chains": list(CHAINS), "results": out}))


if __name__ == "__main__":
    main()
