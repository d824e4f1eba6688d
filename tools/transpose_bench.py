#!/usr/bin/env python3
"""Times the device-side transpose / layout conversion (bmsp_matrix_transpose, bmsp_matrix_convert_layout, bmsp_matrix_copy_values)
against the route that existed before them (bmsp_matrix_to_coo_device + bmsp_matrix_from_coo_device of the swapped COO), interleaved
in one process, on:
  rmat20   R-MAT 2^20 x 2 + I, fp32 (the headline stand-in, hyper-sparse tiles)
  fem27    fem_like 27pt (47^3 rows), fp32 and fp16 (its window-shuffled numbering leaves 3.7 values per tile)
  rmat16   R-MAT 2^16 x 8, fp16 (its transpose has hub block-rows)
  banded   2^17 rows, half-bandwidth 32, fp32 (full and near-full tiles)
Each op: HIP events around one call, after warm-up; the median of --reps calls (>= 20).  Also the value move under each forced lane
group (BMSP_TRANSPOSE_LANES) for both transposes and copy_values.  Bytes are computed from the shapes:
  compulsory   read A's four arrays once, write the output's once (+ the 4-byte tile map of a transpose)
  sort         the radix passes over (8-byte key, 4-byte payload) per tile, read and written
  route        A's arrays read, 16-byte COO (int32 row, int32 col, float64 value) written and read back, output written -- the COO
               route's floor, before its two sorts.
Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bmsparse-spgemm-spmv_amd"))
import ctypes as C  # noqa: E402
import pybmsp as B  # noqa: E402
from pybmsp import gen  # noqa: E402

ES = {B.F32: 4, B.F16: 2, B.F64: 8}
RADIX_BITS = 9  # kRadixMaxBits of prims.hip.h


def timed(fn):
    e0, e1 = B.Event(), B.Event()
    e0.record()
    keep = fn()
    e1.record()
    ms = e0.elapsed_ms(e1)
    del keep
    return ms


def route(A, out_layout, swap):
    """the pre-existing way to the same result: expand to a device COO, build again."""
    r, c, v = A.to_coo_device()
    i = A.info()
    rows, cols = (c, r) if swap else (r, c)
    nr, nc = (i["num_cols"], i["num_rows"]) if swap else (i["num_rows"], i["num_cols"])
    h = C.c_void_p()
    B.check(B.lib().bmsp_matrix_from_coo_device(nr, nc, i["nnz"], rows.ptr, cols.ptr, v.ptr, int(out_layout), i["dtype"], None, C.byref(h)))
    return B.BmSpMatrix(h.value)


def bytes_of(A, op):
    i = A.info()
    nb, nz, es = i["block_num"], i["nnz"], ES[i["dtype"]]
    arrays = 24 * nb + 8 + es * nz  # keys, bitmaps, offsets (block_num + 1), values
    cbits = max(0, math.ceil(math.log2(max(1, (i["num_cols"] + 7) // 8))))
    passes = math.ceil(cbits / RADIX_BITS) if cbits else 0
    if op in ("transpose_flip", "transpose_same"):
        return {"compulsory": 2 * arrays + 4 * nb, "sort": 2 * 12 * nb * passes}
    if op == "convert":
        return {"compulsory": 2 * arrays, "sort": 0}
    if op == "copy_values":  # tile map, source bitmaps and both offsets, values both ways
        return {"compulsory": 4 * nb + 8 * nb + 16 * nb + 2 * es * nz, "sort": 0}
    return {"compulsory": 2 * arrays + 32 * nz, "sort": 0}


def median_ms(samples):
    return round(statistics.median(samples), 4)


def bench_matrix(name, n_rows, n_cols, r, c, v, dtype, reps, warmup):
    A = B.BmSpMatrix.from_coo(n_rows, n_cols, r, c, v, dtype=dtype)
    i = A.info()
    in_layout = 0
    flip = 1 - in_layout
    At = A.transpose(in_layout)  # target of copy_values: a same-layout transpose (values permuted inside tiles)
    ops = {
        "transpose_flip": lambda: A.transpose(flip),
        "transpose_same": lambda: A.transpose(in_layout),
        "convert": lambda: A.with_layout(flip),
        "copy_values": lambda: At.copy_values_from(A),
        "route_transpose_flip": lambda: route(A, flip, True),
        "route_transpose_same": lambda: route(A, in_layout, True),
        "route_convert": lambda: route(A, flip, False),
    }
    for _ in range(warmup):
        for f in ops.values():
            timed(f)
    samples = {k: [] for k in ops}
    for _ in range(reps):  # interleaved: every op once per round
        for k, f in ops.items():
            samples[k].append(timed(f))
    res = {"matrix": name, "dtype": {0: "fp32", 1: "fp16", 2: "fp64"}[dtype], "rows": i["num_rows"], "cols": i["num_cols"],
           "nnz": i["nnz"], "tiles": i["block_num"], "values_per_tile": round(i["nnz"] / max(1, i["block_num"]), 2), "ms": {}, "bytes": {},
           "gbps_compulsory": {}}
    for k in ops:
        res["ms"][k] = median_ms(samples[k])
        res["bytes"][k] = bytes_of(A, k if not k.startswith("route") else "route")
        res["gbps_compulsory"][k] = round(res["bytes"][k]["compulsory"] / (res["ms"][k] * 1e-3) / 1e9, 1)
    for k in ("transpose_flip", "transpose_same", "convert"):
        res["speedup_vs_route_" + k] = round(res["ms"]["route_" + k] / res["ms"][k], 2)
    # the value move's lane group, forced (read per call by the library)
    lanes = {}
    for g in ("1", "8"):
        os.environ["BMSP_TRANSPOSE_LANES"] = g
        for k in ("transpose_flip", "transpose_same", "copy_values"):
            for _ in range(2):
                timed(ops[k])
            lanes["%s_g%s" % (k, g)] = median_ms([timed(ops[k]) for _ in range(max(20, reps // 2))])
    del os.environ["BMSP_TRANSPOSE_LANES"]
    res["ms_by_lanes"] = lanes
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="small matrices (a rehearsal of the tool, not a measurement)")
    a = ap.parse_args()
    reps = max(20, a.reps)
    B.set_device(0)
    out = []
    if a.quick:
        cases = [("rmat12", gen.rmat(12, 2), B.F32), ("fem27_s10", gen.fem_like(10, "27pt"), B.F16)]
    else:
        cases = [("rmat20", gen.rmat(20, 2), B.F32), ("fem27", gen.fem_like(47, "27pt"), B.F32), ("fem27", gen.fem_like(47, "27pt"), B.F16),
                 ("rmat16x8", gen.rmat(16, 8), B.F16), ("banded_hb32", gen.banded(1 << 17, 32), B.F32)]
    for name, (nr, nc, r, c, v), dt in cases:
        out.append(bench_matrix(name, nr, nc, r, c, v, dt, reps, a.warmup))
    print(json.dumps({"tool": "transpose_bench", "reps": reps, "results": out}))


if __name__ == "__main__":
    main()
