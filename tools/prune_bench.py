#!/usr/bin/env python3
"""Times device-side pruning (bmsp_matrix_prune, bmsp_matrix_row_absmax) against the only other route to the same matrix
(bmsp_matrix_to_coo_device, a boolean mask of the triples on the device -- torch on the same stream --, bmsp_matrix_from_coo_device,
which expands every tile to scalar triples and sorts the kept ones again), interleaved in one process, on the four matrices of
tools/add_bench.py:
  rmat20   R-MAT 2^20 x 2 + I, fp32 (the headline stand-in, hyper-sparse tiles)
  rmat16   R-MAT 2^16 x 8, fp16 (hub block-rows)
  banded   2^17 rows, half-bandwidth 32, fp32 (full tiles)
  fem27    fem_like 27pt (47^3 rows), fp32
each at three kept fractions (all, about a half, about a tenth; the tolerance is the matching quantile of |v|, or of |v| / rowmax for
the row-relative rule; ties at the quantile move it, so the kept fraction is reported per case), under both rules, plus row_absmax
alone and the count-only call.  Each op: HIP events around one call, after warm-up; the median of --reps calls (>= 20), the ops taking turns.  Bytes are computed from the shapes:
  compulsory   A's four arrays read once + the output's four arrays written once (+ the row maxima written and gathered, ROW_REL)
Rates are compulsory bytes over the median call time (whole calls: launches, the read-back and the allocation of the output included)
and their share of the 8 TB/s HBM peak.  Also prune's time under each forced lane group (BMSP_PRUNE_LANES), and one downstream line:
C = A A (fem27), C' = prune(C, row_rel), then y = C x and C A with and without the prune.  --one CASE makes a single headline call
(ABS, half kept) after one warm-up call, for a kernel trace of its own.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bmsparse-spgemm-spmv_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before pybmsp: both share one HIP runtime)
import pybmsp as B  # noqa: E402
from pybmsp import gen  # noqa: E402

ES = {B.F32: 4, B.F16: 2, B.F64: 8}
RM = {B.F32: 4, B.F16: 4, B.F64: 8}
HBM_PEAK = 8.0e12  # bytes/s, MI355X spec
FRACTIONS = (("all", 1.0), ("half", 0.5), ("tenth", 0.1))


def timed(fn):
    e0, e1 = B.Event(), B.Event()
    e0.record()
    keep = fn()
    e1.record()
    ms = e0.elapsed_ms(e1)
    del keep
    return ms


class _Raw:
    """a DeviceArray seen through __cuda_array_interface__ (no copy)"""

    def __init__(self, d):
        self.d = d
        self.__cuda_array_interface__ = {"shape": (d.n,), "typestr": d.dtype.str, "data": (d.ptr, False), "version": 2}


def as_tensor(d):
    return torch.as_tensor(_Raw(d), device="cuda")


def route(A, tol, rule, out_layout):
    """the pre-existing way to the pruned matrix: device COO, a mask of the triples, the builder"""
    r, c, v = A.to_coo_device()
    tr, tc, tv = as_tensor(r), as_tensor(c), as_tensor(v)
    a = tv.abs()
    if rule == "row_rel":
        rowmax = torch.zeros(A.info()["num_rows"], dtype=torch.float64, device="cuda")
        rowmax.scatter_reduce_(0, tr.long(), torch.nan_to_num(a, nan=0.0), "amax")
        keep = ~(a <= tol * rowmax[tr.long()])
    else:
        keep = ~(a <= tol)
    r2, c2, v2 = tr[keep].contiguous(), tc[keep].contiguous(), tv[keep].contiguous()
    i = A.info()
    h = C.c_void_p()
    B.check(B.lib().bmsp_matrix_from_coo_device(i["num_rows"], i["num_cols"], r2.numel(), r2.data_ptr(), c2.data_ptr(), v2.data_ptr(),
                                                int(out_layout), i["dtype"], None, C.byref(h)))
    return B.BmSpMatrix(h.value)


def arrays_bytes(M):
    i = M.info()
    return 24 * i["block_num"] + 8 + ES[i["dtype"]] * i["nnz"]  # keys, bitmaps, offsets (block_num + 1), values


def median_ms(samples):
    return round(statistics.median(samples), 4)


def tolerances(A, r, v):
    """{(rule, fraction name): tol}: quantiles of |v| (ABS) and of |v| / rowmax (ROW_REL) of the STORED values"""
    dt = B.NP_DTYPE[A.info()["dtype"]]
    a = np.abs(np.asarray(v, dt).astype(np.float64))
    rowmax = np.zeros(A.info()["num_rows"])
    np.maximum.at(rowmax, r, a)
    rel = a / np.maximum(rowmax[r], 1e-300)

    def pick(x, f):
        """the (1 - f) quantile of x; the value just below it when ties at the quantile (R-MAT: a third of the values are the identity's
        1.0) would take the kept fraction under f / 2"""
        if f == 1.0:
            return 0.0
        q = float(np.quantile(x, 1.0 - f))
        return q if np.mean(x > q) >= f / 2 else float(np.nextafter(q, 0.0))

    out = {}
    for name, f in FRACTIONS:
        out[("abs", name)] = pick(a, f)
        out[("row_rel", name)] = pick(rel, f)
    return out


def bench_case(name, A, r, v, reps, warmup, note):
    lay = A.info()["transposed"]
    tols = tolerances(A, r, v)
    ops = {"row_absmax": lambda: B.row_absmax(A)}
    for (rule, frac), tol in tols.items():
        ops["prune_%s_%s" % (rule, frac)] = (lambda rule=rule, tol=tol: B.prune(A, tol, rule, transposed=lay))
        ops["route_%s_%s" % (rule, frac)] = (lambda rule=rule, tol=tol: route(A, tol, rule, lay))
    ops["count_abs_half"] = lambda: B.prune_count(A, tols[("abs", "half")], "abs")
    ops["count_row_rel_half"] = lambda: B.prune_count(A, tols[("row_rel", "half")], "row_rel")
    for _ in range(warmup):
        for f in ops.values():
            timed(f)
    samples = {k: [] for k in ops}
    for _ in range(reps):
        for k, f in ops.items():
            samples[k].append(timed(f))
    ia = A.info()
    res = {"case": name, "what": note, "dtype": {0: "fp32", 1: "fp16", 2: "fp64"}[ia["dtype"]], "rows": ia["num_rows"], "nnz": ia["nnz"],
           "tiles": ia["block_num"], "values_per_tile": round(ia["nnz"] / max(1, ia["block_num"]), 2), "ms": {}, "kept": {}, "bytes": {},
           "gbps": {}, "hbm_frac": {}, "speedup_vs_route": {}}
    for k in ops:
        res["ms"][k] = median_ms(samples[k])
    for (rule, frac), tol in tols.items():
        k = "prune_%s_%s" % (rule, frac)
        P, st = B.prune(A, tol, rule, transposed=lay)
        res["kept"][k] = {"tol": tol, "nnz": st["nnz_out"], "tiles": st["blocks_out"], "fraction": round(st["nnz_out"] / max(1, st["nnz_in"]), 3)}
        nbytes = arrays_bytes(A) + arrays_bytes(P) + (2 * RM[ia["dtype"]] * ia["num_rows"] if rule == "row_rel" else 0)
        res["bytes"][k] = nbytes
        rate = nbytes / (res["ms"][k] * 1e-3)
        res["gbps"][k] = round(rate / 1e9, 1)
        res["hbm_frac"][k] = round(rate / HBM_PEAK, 3)
        res["speedup_vs_route"][k] = round(res["ms"]["route_%s_%s" % (rule, frac)] / res["ms"][k], 2)
    lanes = {}
    for g in ("1", "8"):
        os.environ["BMSP_PRUNE_LANES"] = g
        for k in ("prune_abs_half", "prune_row_rel_half", "prune_abs_all", "row_absmax"):
            for _ in range(2):
                timed(ops[k])
            lanes["%s_g%s" % (k, g)] = median_ms([timed(ops[k]) for _ in range(max(20, reps // 2))])
    del os.environ["BMSP_PRUNE_LANES"]
    res["ms_by_lanes"] = lanes
    return res


def downstream(reps, warmup, quick):
    """C = A A of the FEM-like matrix; the second product C A and y = C x on C and on prune(C, row_rel)"""
    n, _, r, c, v = gen.fem_like(12 if quick else 47, "27pt")
    A = B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32)
    Bm = A.with_layout(1)
    Cm, _ = B.spgemm(A, Bm, tc_version=5)
    tol = 0.25  # a strength-of-connection threshold
    Cp, st = B.prune(Cm, tol, "row_rel", keep_diagonal=True)
    x = B.DeviceArray.from_host(gen.spmv_x(n, "cusp"))
    y = B.DeviceArray(n, np.float32)
    ops = {
        "prune": lambda: B.prune(Cm, tol, "row_rel", keep_diagonal=True),
        "spmv_unpruned": lambda: B.spmv(Cm, x, y),
        "spmv_pruned": lambda: B.spmv(Cp, x, y),
        "second_product_unpruned": lambda: B.spgemm(Cm, Bm, tc_version=5),
        "second_product_pruned": lambda: B.spgemm(Cp, Bm, tc_version=5),
    }
    for _ in range(warmup):
        for f in ops.values():
            timed(f)
    samples = {k: [] for k in ops}
    for _ in range(reps):
        for k, f in ops.items():
            samples[k].append(timed(f))
    return {"what": "fem_like 27pt fp32: C = A A, C' = prune(C, %g, row_rel, keep_diagonal)" % tol, "rows": n, "c": st,
            "ms": {k: median_ms(s) for k, s in samples.items()}}


def cases(quick):
    """(name, A, rows, values, note) -- built outside the timed region"""
    if quick:
        n, _, r, c, v = gen.rmat(12, 2)
        yield "rmat12", B.BmSpMatrix.from_coo(n, n, r, c, v), r, v, "R-MAT 2^12 x 2 + I"
        n, _, r, c, v = gen.banded(1 << 11, 32)
        yield "banded_s", B.BmSpMatrix.from_coo(n, n, r, c, v), r, v, "banded 2^11, hb 32"
        return
    n, _, r, c, v = gen.rmat(20, 2)
    yield "rmat20", B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32), r, v, "R-MAT 2^20 x 2 + I"
    n, _, r, c, v = gen.rmat(16, 8)
    yield "rmat16", B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F16), r, v, "R-MAT 2^16 x 8 + I"
    n, _, r, c, v = gen.banded(1 << 17, 32)
    yield "banded", B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32), r, v, "banded 2^17, hb 32"
    n, _, r, c, v = gen.fem_like(47, "27pt")
    yield "fem27", B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32), r, v, "fem_like 27pt, 47^3 rows"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="small matrices (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--one", metavar="CASE", help="one headline call of this case only (ABS, half kept), for a kernel trace")
    a = ap.parse_args()
    reps = max(20, a.reps)
    B.set_device(0)
    torch.zeros(1, device="cuda")
    if a.one:
        for name, A, r, v, note in cases(a.quick):
            if name != a.one:
                continue
            tol = tolerances(A, r, v)[("abs", "half")]
            B.prune(A, tol)
            _, st = B.prune(A, tol)
            B.synchronize()
            print(json.dumps({"tool": "prune_bench", "one": name, "tol": tol, "stats": st}))
        return
    out = []
    for name, A, r, v, note in cases(a.quick):
        out.append(bench_case(name, A, r, v, reps, a.warmup, note))
        del A
    ok = all(s > 1.0 for res in out for s in res["speedup_vs_route"].values())
    print(json.dumps({"tool": "prune_bench", "reps": reps, "prune_faster_than_route_everywhere": ok, "results": out,
                      "downstream": downstream(reps, a.warmup, a.quick)}))


if __name__ == "__main__":
    main()
