#!/usr/bin/env python3
"""Times bmsp_spmv_op where it replaces a materialised matrix: op = T on a row-major A, and op = N on a column-major A, against the
yardstick that existed before it -- bmsp_spmv on A.transpose(0) / A.with_layout(0), prepared, in the same process -- on:
  rmat20   R-MAT 2^20 x 2 + I (the webbase-1M stand-in, hyper-sparse tiles, hub block-columns)
  banded   2^17 rows, half-bandwidth 32 (full and near-full tiles)
  fem27    fem_like 27pt (47^3 rows; 3.7 values per tile)
  rmat16   R-MAT 2^16 x 8 (hub block-rows and block-columns of thousands of tiles)
each in fp32 and fp16.  Per case:
  steady    HIP events around --batch launches, after warm-up, the two sides interleaved; the median of --reps samples, per launch
  one_shot  host clock from a fresh copy of the matrix to the synchronised first result: view build + first sweep, against transpose (or
            layout conversion) + prepare + first bmsp_spmv
  memory    device memory the process holds more after the first call (pool trimmed on both sides): the view, against the second matrix
            with its SpMV caches; view_bytes is the library's own figure for the view
  switches  BMSP_SPMV_OP_SLOTS = 1 / 8 (per call) and BMSP_SPMV_OP_SPLIT = 16 ... 1024 / none (per view build), steady state;
            slots_threshold: both SLOTS on banded matrices of 1.6 - 7 tiles per output block (fp32), where the default changes over
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
SPLITS = ("16", "32", "64", "128", "256", "1024", str(1 << 31))


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
    ms = (time.perf_counter() - t0) * 1e3
    return ms, keep


def bench_case(H, A, op, materialise, v, a):
    """A under `op` against bmsp_spmv on materialise(A)"""
    i = A.info()
    n_out = i["num_cols"] if op == "T" else i["num_rows"]
    u, uy = B.DeviceArray(n_out, B.OUT_DTYPE[i["dtype"]]), B.DeviceArray(n_out, B.OUT_DTYPE[i["dtype"]])
    res = {}

    def yardstick_first(G):
        M = materialise(G).prepare(1)
        B.spmv(M, v, uy)
        return M

    # one-shot and memory, on fresh copies (nothing cached on them)
    shots = {"op": [], "yardstick": []}
    for rep in range(a.shots):
        m0 = held(H)
        F = A.clone()
        m1 = held(H)
        ms, _ = wall_ms(lambda: B.spmv_op(F, v, op, u=u))
        shots["op"].append(ms)
        m2 = held(H)
        G = A.clone()
        m3 = held(H)
        ms, M = wall_ms(lambda: yardstick_first(G))
        shots["yardstick"].append(ms)
        m4 = held(H)
        res["memory"] = {"matrix_bytes": m1 - m0, "op_view_held_bytes": m2 - m1, "view_bytes": B.spmv_op_launch_info(F, op)["view_bytes"],
                         "yardstick_held_bytes": m4 - m3}
        del F, G, M
    res["one_shot_ms"] = {k: round(statistics.median(s), 3) for k, s in shots.items()}
    res["one_shot_ratio_yardstick_over_op"] = round(res["one_shot_ms"]["yardstick"] / res["one_shot_ms"]["op"], 2)
    # steady state
    M = materialise(A).prepare(1)
    B.spmv(M, v, uy)
    B.spmv_op(A, v, op, u=u)
    B.synchronize()
    same = bool(np.allclose(u.to_host(), uy.to_host(), rtol=1e-4, atol=1e-4))
    info = B.spmv_op_launch_info(A, op)
    st = steady_us({"op": lambda: B.spmv_op(A, v, op, u=u), "yardstick": lambda: B.spmv(M, v, uy)}, a.batch, a.reps, a.warmup)
    res["launch_info"] = info
    res["yardstick_kernel"] = B.spmv_launch_info(M)["kernel"]
    res["results_agree"] = same
    res["steady_us"] = st
    res["steady_ratio_op_over_yardstick"] = round(st["op"] / st["yardstick"], 2)
    res["steady_ratio_yardstick_over_op"] = round(st["yardstick"] / st["op"], 2)
    res["gbps_compulsory"] = round(info["compulsory_bytes"] / (st["op"] * 1e-6) / 1e9, 1)
    # the switches: SLOTS per call; SPLIT per view build (the view is dropped with the structure caches and built again)
    sw = {}
    for s in ("1", "8"):
        os.environ["BMSP_SPMV_OP_SLOTS"] = s
        sw["slots" + s] = steady_us({"op": lambda: B.spmv_op(A, v, op, u=u)}, a.batch, max(5, a.reps // 2), 2)["op"]
    del os.environ["BMSP_SPMV_OP_SLOTS"]
    for s in SPLITS:
        os.environ["BMSP_SPMV_OP_SPLIT"] = s
        A.invalidate(True)
        B.spmv_op(A, v, op, u=u)
        li = B.spmv_op_launch_info(A, op)
        key = "split" + (s if int(s) < (1 << 31) else "none")
        sw[key] = {"us": steady_us({"op": lambda: B.spmv_op(A, v, op, u=u)}, a.batch, max(5, a.reps // 2), 2)["op"],
                   "split_blocks": li["split_blocks"], "items": li["items"]}
    del os.environ["BMSP_SPMV_OP_SPLIT"]
    A.invalidate(True)
    res["switches_us"] = sw
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20, help="launches per timed sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shots", type=int, default=3, help="one-shot repetitions")
    ap.add_argument("--quick", action="store_true", help="small matrices (a rehearsal of the tool, not a measurement)")
    a = ap.parse_args()
    B.set_device(0)
    if a.quick:
        mats = [("rmat12", lambda: gen.rmat(12, 2)), ("banded_s", lambda: gen.banded(1 << 10, 32))]
    else:
        mats = [("rmat20 (webbase-1M-like)", lambda: gen.rmat(20, 2)), ("banded_hb32", lambda: gen.banded(1 << 17, 32)),
                ("fem27", lambda: gen.fem_like(47, "27pt")), ("rmat16x8", lambda: gen.rmat(16, 8))]
    B.DeviceArray(1, np.float32)  # the runtime is up before it is looked for
    H = hip_runtime()
    out = []
    for name, make in mats:
        nr, nc, r, c, vals = make()
        for dtype in (B.F32, B.F16):
            A0 = B.BmSpMatrix.from_coo(nr, nc, r, c, vals, dtype=dtype)
            A1 = A0.with_layout(1)
            i = A0.info()
            v = B.DeviceArray.from_host(gen.spmv_x(nr, "cusp").astype(B.NP_DTYPE[dtype]))  # (square matrices: one v serves both ops)
            row = {"matrix": name, "dtype": DT[dtype], "rows": nr, "nnz": i["nnz"], "tiles": i["block_num"],
                   "values_per_tile": round(i["nnz"] / max(1, i["block_num"]), 2),
                   "tiles_per_block": round(i["block_num"] / max(1, (nr + 7) // 8), 2),
                   "T_on_row_major": bench_case(H, A0, "T", lambda M: M.transpose(0), v, a),
                   "N_on_column_major": bench_case(H, A1, "N", lambda M: M.with_layout(0), v, a)}
            out.append(row)
            del A0, A1
    # where SLOTS = 8 starts to pay: banded matrices of few tiles per output block, both sweeps forced
    thr = []
    for hb in ((2, 8) if a.quick else (2, 4, 8, 12, 16, 20, 24, 28)):
        nr, nc, r, c, vals = gen.banded(1 << (10 if a.quick else 17), hb)
        A0 = B.BmSpMatrix.from_coo(nr, nc, r, c, vals, dtype=B.F32)
        A1 = A0.with_layout(1)
        v = B.DeviceArray.from_host(gen.spmv_x(nr, "cusp"))
        u = B.DeviceArray(nr, np.float32)
        row = {"half_bandwidth": hb, "tiles_per_block": round(A0.info()["block_num"] / ((nr + 7) // 8), 2)}
        for key, M, op in (("T_on_row_major", A0, "T"), ("N_on_column_major", A1, "N")):
            for s in ("1", "8"):
                os.environ["BMSP_SPMV_OP_SLOTS"] = s
                row["%s_slots%s_us" % (key, s)] = steady_us({"op": lambda: B.spmv_op(M, v, op, u=u)}, a.batch, max(5, a.reps // 2), 2)["op"]
        del os.environ["BMSP_SPMV_OP_SLOTS"]
        thr.append(row)
    print(json.dumps({"tool": "spmv_op_bench", "reps": a.reps, "batch": a.batch, "results": out, "slots_threshold": thr}))


if __name__ == "__main__":
    main()
