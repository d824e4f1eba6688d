#!/usr/bin/env python3
"""Times the device-side sparse addition (bmsp_matrix_add, bmsp_matrix_add_values) against the route that existed before it
(bmsp_matrix_to_coo_device of both operands, a device concatenation, bmsp_matrix_from_coo_device, which sorts every entry again and sums
the duplicates), interleaved in one process, on:
  rmat20   R-MAT 2^20 x 2 + I, fp32: A + A^T, A^T from the layout-flipping transpose (the headline stand-in, hyper-sparse tiles)
  rmat16   R-MAT 2^16 x 8, fp16: A + A^T (hub block-rows)
  banded   2^17 rows, half-bandwidth 32, fp32: A - 0.5 I (full tiles; I lies inside A's pattern)
  fem27    fem_like 27pt (47^3 rows), fp32: 2 A - 0.5 A, A passed as both operands
Each op: HIP events around one call, after warm-up; the median of --reps calls (>= 20), the ops taking turns.  add_values and the route
are timed on the same operands; the route computes A + B (alpha = beta = 1: it has no scaling).  Also add's time under each forced lane
group of the value pass (BMSP_ADD_LANES).  Bytes are computed from the shapes:
  compulsory   A's and B's four arrays read once, C's four arrays written once, and C's two 4-byte source maps
  values       add_values: the source maps, C's bitmaps and offsets, the operands' bitmaps and offsets of the tiles used, every value of
               A, B and C once
Rates are compulsory bytes over the median call time (whole calls, launches and the read-back included), and their share of the 8 TB/s
HBM peak.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bmsparse-spgemm-spmv_amd"))
import numpy as np  # noqa: E402
import pybmsp as B  # noqa: E402
from pybmsp import gen  # noqa: E402

ES = {B.F32: 4, B.F16: 2, B.F64: 8}
HBM_PEAK = 8.0e12  # bytes/s, MI355X spec


def timed(fn):
    e0, e1 = B.Event(), B.Event()
    e0.record()
    keep = fn()
    e1.record()
    ms = e0.elapsed_ms(e1)
    del keep
    return ms


def _concat(parts, dtype):
    out = B.DeviceArray(sum(p.n for p in parts), dtype)
    off = 0
    for p in parts:
        if p.n:
            B.check(B.lib().bmsp_memcpy_d2d(out.ptr + off, p.ptr, p.n * p.dtype.itemsize))
        off += p.n * p.dtype.itemsize
    return out


def route(A, Bm, out_layout):
    """the pre-existing way to A + B: both operands to a device COO, concatenated, built again"""
    ra, ca, va = A.to_coo_device()
    rb, cb, vb = Bm.to_coo_device()
    r, c, v = _concat([ra, rb], np.int32), _concat([ca, cb], np.int32), _concat([va, vb], np.float64)
    i = A.info()
    h = C.c_void_p()
    B.check(B.lib().bmsp_matrix_from_coo_device(i["num_rows"], i["num_cols"], r.n, r.ptr, c.ptr, v.ptr, int(out_layout), i["dtype"], None,
                                                C.byref(h)))
    return B.BmSpMatrix(h.value)


def arrays_bytes(M):
    i = M.info()
    return 24 * i["block_num"] + 8 + ES[i["dtype"]] * i["nnz"]  # keys, bitmaps, offsets (block_num + 1), values


def bytes_of(A, Bm, Cm, op):
    ic = Cm.info()
    if op == "add_values":
        es = ES[ic["dtype"]]
        tiles = 8 * ic["block_num"] + 16 * ic["block_num"]  # source maps; C's bitmaps and offsets
        operands = 16 * (A.info()["block_num"] + Bm.info()["block_num"])  # bitmaps and offsets of every operand tile
        return tiles + operands + es * (A.info()["nnz"] + Bm.info()["nnz"] + ic["nnz"])
    return arrays_bytes(A) + arrays_bytes(Bm) + arrays_bytes(Cm) + 8 * ic["block_num"]


def median_ms(samples):
    return round(statistics.median(samples), 4)


def bench_case(name, A, Bm, alpha, beta, reps, warmup, note):
    lay = A.info()["transposed"]
    Cm = B.add(A, Bm, alpha, beta, transposed=lay)
    ops = {
        "add": lambda: B.add(A, Bm, alpha, beta, transposed=lay),
        "add_values": lambda: B.add_values(Cm, A, Bm, alpha, beta),
        "route": lambda: route(A, Bm, lay),
    }
    for _ in range(warmup):
        for f in ops.values():
            timed(f)
    samples = {k: [] for k in ops}
    for _ in range(reps):
        for k, f in ops.items():
            samples[k].append(timed(f))
    ia, ib, ic = A.info(), Bm.info(), Cm.info()
    res = {"case": name, "what": note, "dtype": {0: "fp32", 1: "fp16", 2: "fp64"}[ia["dtype"]], "rows": ia["num_rows"],
           "a_nnz": ia["nnz"], "a_tiles": ia["block_num"], "a_layout": ia["transposed"], "b_nnz": ib["nnz"], "b_tiles": ib["block_num"],
           "b_layout": ib["transposed"], "c_nnz": ic["nnz"], "c_tiles": ic["block_num"],
           "c_values_per_tile": round(ic["nnz"] / max(1, ic["block_num"]), 2), "ms": {}, "bytes": {}, "gbps": {}, "hbm_frac": {}}
    for k in ops:
        res["ms"][k] = median_ms(samples[k])
    for k in ("add", "add_values"):
        res["bytes"][k] = bytes_of(A, Bm, Cm, k)
        rate = res["bytes"][k] / (res["ms"][k] * 1e-3)
        res["gbps"][k] = round(rate / 1e9, 1)
        res["hbm_frac"][k] = round(rate / HBM_PEAK, 3)
    res["speedup_add_vs_route"] = round(res["ms"]["route"] / res["ms"]["add"], 2)
    res["speedup_add_values_vs_add"] = round(res["ms"]["add"] / res["ms"]["add_values"], 2)
    lanes = {}
    for g in ("1", "8"):
        os.environ["BMSP_ADD_LANES"] = g
        for k in ("add", "add_values"):
            for _ in range(2):
                timed(ops[k])
            lanes["%s_g%s" % (k, g)] = median_ms([timed(ops[k]) for _ in range(max(20, reps // 2))])
    del os.environ["BMSP_ADD_LANES"]
    res["ms_by_lanes"] = lanes
    return res


def cases(quick):
    """(name, A, B, alpha, beta, note) -- the operands are built here, outside the timed region"""
    if quick:
        n, _, r, c, v = gen.rmat(12, 2)
        A = B.BmSpMatrix.from_coo(n, n, r, c, v)
        yield "rmat12", A, A.transpose(1), 1.0, 1.0, "A + A^T (A^T in the other layout)"
        n, _, r, c, v = gen.banded(1 << 11, 32)
        A = B.BmSpMatrix.from_coo(n, n, r, c, v)
        d = np.arange(n)
        yield "banded_s", A, B.BmSpMatrix.from_coo(n, n, d, d, np.ones(n)), 1.0, -0.5, "A - 0.5 I"
        return
    n, _, r, c, v = gen.rmat(20, 2)
    A = B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32)
    yield "rmat20", A, A.transpose(1), 1.0, 1.0, "A + A^T (A^T in the other layout)"
    n, _, r, c, v = gen.rmat(16, 8)
    A = B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F16)
    yield "rmat16", A, A.transpose(1), 1.0, 1.0, "A + A^T (A^T in the other layout)"
    n, _, r, c, v = gen.banded(1 << 17, 32)
    A = B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32)
    d = np.arange(n)
    yield "banded", A, B.BmSpMatrix.from_coo(n, n, d, d, np.ones(n), dtype=B.F32), 1.0, -0.5, "A - 0.5 I"
    n, _, r, c, v = gen.fem_like(47, "27pt")
    A = B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32)
    yield "fem27", A, A, 2.0, -0.5, "2 A - 0.5 A (one handle as both operands)"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="small matrices (a rehearsal of the tool, not a measurement)")
    a = ap.parse_args()
    reps = max(20, a.reps)
    B.set_device(0)
    out = []
    for name, A, Bm, alpha, beta, note in cases(a.quick):
        out.append(bench_case(name, A, Bm, alpha, beta, reps, a.warmup, note))
        del A, Bm
    ok = all(r["ms"]["add"] < r["ms"]["route"] and r["ms"]["add_values"] < r["ms"]["add"] for r in out)
    print(json.dumps({"tool": "add_bench", "reps": reps, "add_faster_than_route_and_add_values_faster_than_add": ok, "results": out}))


if __name__ == "__main__":
    main()
