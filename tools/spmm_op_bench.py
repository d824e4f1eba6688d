#!/usr/bin/env python3
"""Times bmsp_spmm_op where it replaces a materialised matrix or k single-vector calls: op = T on a row-major A, and op = N on a
column-major A, for k in {4, 16, 32, 64}, against the two routes that existed before it, in the same process:
  route 1   k calls of bmsp_spmv_op on the columns -- the only route without a second matrix; timed on CONTIGUOUS column vectors, which
            flatters it (a row-major X would have to be strided through or transposed first)
  route 2   bmsp_spmm on the materialised and prepared A.transpose(0) / A.with_layout(0)
on:
  rmat20   R-MAT 2^20 x 2 + I (the webbase-1M stand-in, hyper-sparse tiles, hub block-columns)
  banded   2^17 rows, half-bandwidth 32 (full and near-full tiles)
  fem27    fem_like 27pt (47^3 rows; 3.7 values per tile)
  rmat16   R-MAT 2^16 x 8 (hub block-rows and block-columns of thousands of tiles)
each in fp32 and fp16.  Per case:
  steady    HIP events around --batch launches (a launch of route 1 is its k calls), after warm-up, the sides interleaved; the median of
            --reps samples, per launch
  lanes     the same for BMSP_SPMM_OP_LANES = 8 / 16 / 32 / 64: the W sweep behind the default
  one_shot  (k = 32) host clock from a fresh copy of the matrix to the synchronised first result: view build + scratch + first sweep,
            against transpose (or layout conversion) + prepare + first bmsp_spmm
  memory    (k = 32) device memory the process holds more after the first call (pool trimmed on both sides)
Prints one JSON line."""
import argparse
import ctypes as C
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

DT = {B.F32: "fp32", B.F16: "fp16"}
LANES = ("8", "16", "32", "64")


def hip_runtime():
    """the HIP runtime libbmsp.so runs on (the same loaded file), for hipMemGetInfo"""
    for line in open("/proc/self/maps"):
        if "libamdhip64.so" in line:
            H = C.CDLL(line.split()[-1])
            H.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
            return H
    raise RuntimeError("libamdhip64 is not loaded")


def held(H):
    """bytes of device memory in use, with the library's free blocks given back first"""
    B.synchronize()
    B.check(B.lib().bmsp_trim_pool())
    free, total = C.c_size_t(), C.c_size_t()
    assert H.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return total.value - free.value


def steady_us(fns, batch, reps, warmup):
    """{name: median microseconds per launch}, the functions interleaved sample by sample"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    B.synchronize()
    samples = {k: [] for k in fns}
    e0, e1 = B.Event(), B.Event()
    for _ in range(reps):
        for k, f in fns.items():
            e0.record()
            for _ in range(batch):
                f()
            e1.record()
            samples[k].append(e0.elapsed_ms(e1) * 1e3 / batch)
    return {k: round(statistics.median(s), 2) for k, s in samples.items()}


def wall_ms(fn):
    B.synchronize()
    t0 = time.perf_counter()
    keep = fn()
    B.synchronize()
    return (time.perf_counter() - t0) * 1e3, keep


def bench_case(H, A, op, materialise, xh, k, a):
    """A under `op` with k vectors against the two routes; xh: in_len x k on the host in A's dtype"""
    i = A.info()
    n_out = i["num_cols"] if op == "T" else i["num_rows"]
    R = B.OUT_DTYPE[i["dtype"]]
    X = B.DeviceArray.from_host(np.ascontiguousarray(xh))
    cols = [B.DeviceArray.from_host(np.ascontiguousarray(xh[:, j])) for j in range(k)]
    Y, Y2 = B.DeviceArray(n_out * k, R), B.DeviceArray(n_out * k, R)
    us = [B.DeviceArray(n_out, R) for _ in range(k)]
    res = {"k": k}

    def route1():
        for j in range(k):
            B.spmv_op(A, cols[j], op, u=us[j])

    M = materialise(A).prepare(1)
    B.spmm(M, X, k, Y2)
    B.spmm_op(A, X, k, op, Y=Y)
    route1()
    B.synchronize()
    y = Y.to_host().reshape(n_out, k)
    res["results_agree"] = bool(np.allclose(y, Y2.to_host().reshape(n_out, k), rtol=1e-4, atol=1e-4) and
                                np.allclose(y[:, k - 1], us[k - 1].to_host(), rtol=1e-4, atol=1e-4))
    info = B.spmm_op_launch_info(A, op, k)
    st = steady_us({"op": lambda: B.spmm_op(A, X, k, op, Y=Y), "route1_k_spmv_op": route1, "route2_spmm": lambda: B.spmm(M, X, k, Y2)},
                   a.batch, a.reps, a.warmup)
    res["launch_info"] = info
    res["route2_kernel"] = B.spmm_launch_info(M, k)
    res["steady_us"] = st
    res["ratio_op_over_route1"] = round(st["op"] / st["route1_k_spmv_op"], 3)
    res["ratio_op_over_route2"] = round(st["op"] / st["route2_spmm"], 3)
    res["gbps_compulsory"] = round(info["compulsory_bytes"] / (st["op"] * 1e-6) / 1e9, 1)
    sw = {}
    for w in LANES:
        os.environ["BMSP_SPMM_OP_LANES"] = w
        sw["lanes" + w] = steady_us({"op": lambda: B.spmm_op(A, X, k, op, Y=Y)}, a.batch, max(5, a.reps // 2), 2)["op"]
    del os.environ["BMSP_SPMM_OP_LANES"]
    res["lanes_us"] = sw
    del M
    if k != 32 or not a.shots:
        return res

    def route2_first(G):
        Mg = materialise(G).prepare(1)
        B.spmm(Mg, X, k, Y2)
        return Mg

    shots = {"op": [], "route2": []}
    for rep in range(a.shots):
        m0 = held(H)
        F = A.clone()
        m1 = held(H)
        ms, _ = wall_ms(lambda: B.spmm_op(F, X, k, op, Y=Y))
        shots["op"].append(ms)
        m2 = held(H)
        G = A.clone()
        m3 = held(H)
        ms, Mg = wall_ms(lambda: route2_first(G))
        shots["route2"].append(ms)
        m4 = held(H)
        fi = B.spmm_op_launch_info(F, op, k)
        res["memory"] = {"matrix_bytes": m1 - m0, "op_held_bytes": m2 - m1, "view_bytes": fi["view_bytes"], "scratch_bytes": fi["scratch_bytes"],
                         "route2_held_bytes": m4 - m3}
        del F, G, Mg
    res["one_shot_ms"] = {key: round(statistics.median(s), 3) for key, s in shots.items()}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20, help="launches per timed sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shots", type=int, default=3, help="one-shot repetitions at k = 32 (0: none)")
    ap.add_argument("--ks", default="4,16,32,64")
    ap.add_argument("--matrices", default="", help="comma-separated subset of rmat20,banded,fem27,rmat16")
    ap.add_argument("--quick", action="store_true", help="small matrices (a rehearsal of the tool, not a measurement)")
    a = ap.parse_args()
    B.set_device(0)
    ks = [int(x) for x in a.ks.split(",")]
    if a.quick:
        mats = [("rmat12", lambda: gen.rmat(12, 2)), ("banded_s", lambda: gen.banded(1 << 10, 32))]
    else:
        mats = [("rmat20", lambda: gen.rmat(20, 2)), ("banded", lambda: gen.banded(1 << 17, 32)),
                ("fem27", lambda: gen.fem_like(47, "27pt")), ("rmat16", lambda: gen.rmat(16, 8))]
        if a.matrices:
            mats = [m for m in mats if m[0] in a.matrices.split(",")]
    B.DeviceArray(1, np.float32)  # the runtime is up before it is looked for
    H = hip_runtime()
    out = []
    rng = np.random.default_rng(1)
    for name, make in mats:
        nr, nc, r, c, vals = make()
        xall = rng.uniform(-1.0, 1.0, (nr, max(ks)))  # (square matrices: one X serves both ops)
        for dtype in (B.F32, B.F16):
            A0 = B.BmSpMatrix.from_coo(nr, nc, r, c, vals, dtype=dtype)
            A1 = A0.with_layout(1)
            i = A0.info()
            row = {"matrix": name, "dtype": DT[dtype], "rows": nr, "nnz": i["nnz"], "tiles": i["block_num"],
                   "values_per_tile": round(i["nnz"] / max(1, i["block_num"]), 2), "T_on_row_major": [], "N_on_column_major": []}
            for k in ks:
                xh = xall[:, :k].astype(B.NP_DTYPE[dtype])
                row["T_on_row_major"].append(bench_case(H, A0, "T", lambda M: M.transpose(0), xh, k, a))
                row["N_on_column_major"].append(bench_case(H, A1, "N", lambda M: M.with_layout(0), xh, k, a))
            out.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)  # progress: a long run that is cut short keeps what it measured
            del A0, A1
    print(json.dumps({"tool": "spmm_op_bench", "reps": a.reps, "batch": a.batch, "results": out}))


if __name__ == "__main__":
    main()
