#!/usr/bin/env python3
"""Times the device-side diagonal operations (bmsp_matrix_scale, bmsp_matrix_scale_values, bmsp_matrix_diagonal,
bmsp_matrix_from_diagonal) against the only other route to the scaled matrix (bmsp_matrix_to_coo_device, a gather-multiply of the
triples on the device -- torch on the same stream --, bmsp_matrix_from_coo_device, which expands every tile to scalar triples and sorts
them again), interleaved in one process, on the four matrices of tools/prune_bench.py:
  rmat20   R-MAT 2^20 x 2 + I, fp32 (the headline stand-in, hyper-sparse tiles)
  rmat16   R-MAT 2^16 x 8, fp16 (hub block-rows)
  banded   2^17 rows, half-bandwidth 32, fp32 (full tiles)
  fem27    fem_like 27pt (47^3 rows), fp32
Per case: scale (both sides, multiply) into the same and into the other layout, scale with both sides dividing, scale_values in place,
diagonal, from_diagonal, the COO route, and as yardsticks that move nearly the same bytes bmsp_matrix_copy_values and
bmsp_matrix_convert_layout on the same matrix.  Each op: HIP events around one call, after warm-up; the median of --reps calls (>= 25),
the ops taking turns.  Bytes are computed from the shapes:
  value pass   keys, bitmaps, offsets and values read once + values written once + the two vectors read once
  scale        the value pass + keys, bitmaps, offsets written once
Rates are these bytes over the median call time (whole calls: launches and the allocation of the output included) and their share of
the 8 TB/s HBM peak.  Also the value pass under each forced lane group (BMSP_SCALE_LANES), and one downstream line: the normalised
operator D^-1/2 A D^-1/2 of the R-MAT from deg = A 1, by scale and by the COO route.  --one CASE makes a single scale_values call after
one warm-up call, for a kernel trace of its own.  Prints one JSON line."""
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


def route(A, tl, tr_, div, out_layout):
    """the pre-existing way to the scaled matrix: device COO, a gather-multiply of the triples in the arithmetic type, the builder"""
    r, c, v = A.to_coo_device()
    rows, cols, vals = as_tensor(r), as_tensor(c), as_tensor(v)
    x = vals.to(tl.dtype)
    x = x / tl[rows.long()] if div else x * tl[rows.long()]
    x = x / tr_[cols.long()] if div else x * tr_[cols.long()]
    v2 = x.double().contiguous()
    i = A.info()
    h = C.c_void_p()
    B.check(B.lib().bmsp_matrix_from_coo_device(i["num_rows"], i["num_cols"], rows.numel(), rows.data_ptr(), cols.data_ptr(), v2.data_ptr(),
                                                int(out_layout), i["dtype"], None, C.byref(h)))
    return B.BmSpMatrix(h.value)


def median_ms(samples):
    return round(statistics.median(samples), 4)


def bench_case(name, A, reps, warmup, note):
    ia = A.info()
    lay, dt, n_r, n_c = ia["transposed"], ia["dtype"], ia["num_rows"], ia["num_cols"]
    rng = np.random.default_rng(1)
    l = B.DeviceArray.from_host(rng.uniform(0.5, 2.0, n_r).astype(B.OUT_DTYPE[dt]))
    r = B.DeviceArray.from_host(rng.uniform(0.5, 2.0, n_c).astype(B.OUT_DTYPE[dt]))
    tl, tr_ = as_tensor(l), as_tensor(r)
    T = A.clone()           # scaled in place over and over: factors in [0.5, 2) alternate multiply and divide, the values stay bounded
    W = A.with_layout(lay)  # the yardsticks' target
    d = B.diagonal(A)
    flip = [False]

    def in_place():
        flip[0] = not flip[0]
        return B.scale_values(T, T, l, r, div_left=flip[0], div_right=flip[0])

    ops = {
        "scale_same": lambda: B.scale(A, l, r, transposed=lay),
        "scale_other": lambda: B.scale(A, l, r, transposed=1 - lay),
        "scale_div_same": lambda: B.scale(A, l, r, div_left=True, div_right=True, transposed=lay),
        "scale_values_inplace": in_place,
        "scale_values_into": lambda: B.scale_values(W, A, l, r),
        "diagonal": lambda: B.diagonal(A),
        "from_diagonal": lambda: B.from_diagonal(d, n_r, n_c, dtype=dt, transposed=lay),
        "route_same": lambda: route(A, tl, tr_, False, lay),
        "route_div_same": lambda: route(A, tl, tr_, True, lay),
        "copy_values": lambda: W.copy_values_from(A),
        "convert_layout_same": lambda: A.with_layout(lay),
        "convert_layout_other": lambda: A.with_layout(1 - lay),
    }
    for _ in range(warmup):
        for f in ops.values():
            timed(f)
    samples = {k: [] for k in ops}
    for _ in range(reps):
        for k, f in ops.items():
            samples[k].append(timed(f))
    nb, nnz = ia["block_num"], ia["nnz"]
    value_pass = 24 * nb + 8 + 2 * ES[dt] * nnz + RM[dt] * (n_r + n_c)
    res = {"case": name, "what": note, "dtype": {0: "fp32", 1: "fp16", 2: "fp64"}[dt], "rows": n_r, "nnz": nnz, "tiles": nb,
           "values_per_tile": round(nnz / max(1, nb), 2), "ms": {k: median_ms(samples[k]) for k in ops},
           "bytes": {"value_pass": value_pass, "scale": value_pass + 24 * nb + 8}, "gbps": {}, "hbm_frac": {}}
    for k, nbytes in (("scale_same", res["bytes"]["scale"]), ("scale_other", res["bytes"]["scale"]), ("scale_div_same", res["bytes"]["scale"]),
                      ("scale_values_inplace", value_pass), ("scale_values_into", value_pass)):
        rate = nbytes / (res["ms"][k] * 1e-3)
        res["gbps"][k] = round(rate / 1e9, 1)
        res["hbm_frac"][k] = round(rate / HBM_PEAK, 3)
    ms = res["ms"]
    res["speedup_vs_route"] = {"scale_same": round(ms["route_same"] / ms["scale_same"], 2),
                               "scale_other": round(ms["route_same"] / ms["scale_other"], 2),
                               "scale_div_same": round(ms["route_div_same"] / ms["scale_div_same"], 2),
                               "scale_values_inplace": round(ms["route_same"] / ms["scale_values_inplace"], 2),
                               "scale_values_into": round(ms["route_same"] / ms["scale_values_into"], 2)}
    res["vs_yardstick"] = {"scale_values_into / copy_values": round(ms["scale_values_into"] / ms["copy_values"], 2),
                           "scale_values_inplace / copy_values": round(ms["scale_values_inplace"] / ms["copy_values"], 2),
                           "scale_same / convert_layout_same": round(ms["scale_same"] / ms["convert_layout_same"], 2),
                           "scale_other / convert_layout_other": round(ms["scale_other"] / ms["convert_layout_other"], 2)}
    lanes = {}
    for g in ("1", "8"):
        os.environ["BMSP_SCALE_LANES"] = g
        for k in ("scale_values_into", "scale_values_inplace", "scale_other", "scale_div_same"):
            for _ in range(2):
                timed(ops[k])
            lanes["%s_g%s" % (k, g)] = median_ms([timed(ops[k]) for _ in range(max(20, reps // 2))])
    del os.environ["BMSP_SCALE_LANES"]
    res["ms_by_lanes"] = lanes
    return res


def downstream(reps, warmup, quick):
    """D^-1/2 A D^-1/2 with D = diag(A 1): the SpMV, the square root and the two-sided division by scale, or by the COO route"""
    n, _, r, c, v = gen.rmat(12 if quick else 20, 2)
    A = B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32)
    ones = B.DeviceArray.from_host(np.ones(n, np.float32))
    deg = B.DeviceArray(n, np.float32)
    tdeg = as_tensor(deg)

    def by_scale():
        B.spmv(A, ones, deg)
        tdeg.sqrt_()
        return B.scale(A, deg, deg, div_left=True, div_right=True)

    def by_route():
        B.spmv(A, ones, deg)
        tdeg.sqrt_()
        return route(A, tdeg, tdeg, True, 0)

    ops = {"normalise_scale": by_scale, "normalise_route": by_route, "scale_alone": lambda: B.scale(A, deg, deg, div_left=True, div_right=True)}
    for _ in range(warmup):
        for f in ops.values():
            timed(f)
    samples = {k: [] for k in ops}
    for _ in range(reps):
        for k, f in ops.items():
            samples[k].append(timed(f))
    return {"what": "R-MAT 2^%d x 2 + I fp32: D^-1/2 A D^-1/2 from deg = A 1 (SpMV, sqrt, scale with both sides dividing)" % (12 if quick else 20),
            "rows": n, "nnz": A.nnz, "ms": {k: median_ms(s) for k, s in samples.items()}}


def cases(quick):
    """(name, A, note) -- built outside the timed region"""
    if quick:
        n, _, r, c, v = gen.rmat(12, 2)
        yield "rmat12", B.BmSpMatrix.from_coo(n, n, r, c, v), "R-MAT 2^12 x 2 + I"
        n, _, r, c, v = gen.banded(1 << 11, 32)
        yield "banded_s", B.BmSpMatrix.from_coo(n, n, r, c, v), "banded 2^11, hb 32"
        return
    n, _, r, c, v = gen.rmat(20, 2)
    yield "rmat20", B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32), "R-MAT 2^20 x 2 + I"
    n, _, r, c, v = gen.rmat(16, 8)
    yield "rmat16", B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F16), "R-MAT 2^16 x 8 + I"
    n, _, r, c, v = gen.banded(1 << 17, 32)
    yield "banded", B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32), "banded 2^17, hb 32"
    n, _, r, c, v = gen.fem_like(47, "27pt")
    yield "fem27", B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32), "fem_like 27pt, 47^3 rows"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="small matrices (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--one", metavar="CASE", help="one scale_values call of this case only, for a kernel trace")
    a = ap.parse_args()
    reps = max(25, a.reps)
    B.set_device(0)
    torch.zeros(1, device="cuda")
    if a.one:
        for name, A, note in cases(a.quick):
            if name != a.one:
                continue
            i = A.info()
            l = B.DeviceArray.from_host(np.full(i["num_rows"], 1.5, B.OUT_DTYPE[i["dtype"]]))
            r = B.DeviceArray.from_host(np.full(i["num_cols"], 0.75, B.OUT_DTYPE[i["dtype"]]))
            W = A.with_layout(i["transposed"])
            B.scale_values(W, A, l, r)
            W.copy_values_from(A)
            B.scale_values(W, A, l, r)
            W.copy_values_from(A)
            B.synchronize()
            print(json.dumps({"tool": "diag_bench", "one": name, "nnz": i["nnz"], "tiles": i["block_num"]}))
        return
    out = []
    for name, A, note in cases(a.quick):
        out.append(bench_case(name, A, reps, a.warmup, note))
        del A
    ok = all(s > 1.0 for res in out for s in res["speedup_vs_route"].values())
    print(json.dumps({"tool": "diag_bench", "reps": reps, "scale_faster_than_route_everywhere": ok, "results": out,
                      "downstream": downstream(reps, a.warmup, a.quick)}))


if __name__ == "__main__":
    main()
