#!/usr/bin/env python3
"""Times device-side selection (bmsp_matrix_select_band, bmsp_matrix_select_mask) beside two yardsticks in the same session --
bmsp_matrix_prune (ABS, about half kept) and the only other route to the same matrix (bmsp_matrix_to_coo_device, a boolean mask of the
triples on the device -- torch on the same stream --, bmsp_matrix_from_coo_device) -- interleaved in one process, on the four matrices
of tools/prune_bench.py:
  rmat20   R-MAT 2^20 x 2 + I, fp32 (the headline stand-in, hyper-sparse tiles)
  rmat16   R-MAT 2^16 x 8, fp16 (hub block-rows)
  banded   2^17 rows, half-bandwidth 32, fp32 (full tiles)
  fem27    fem_like 27pt (47^3 rows), fp32
The calls: tril(A), band(A, -32, 32), the off-diagonal part, select_mask(A A, A) and its complement (the product restricted to A's
pattern, and its fill-in), and the count-only forms of tril and of the mask.  Each op: HIP events around one call, after warm-up; the
median of --reps calls (>= 20), the ops taking turns.  Bytes are computed from the shapes:
  compulsory   the source's keys, bitmaps and offsets read once + the kept values read once + the output's four arrays written once
               (+ M's keys and bitmaps once for a mask; a count-only call: the keys and bitmaps alone)
Rates are compulsory bytes over the median call time (whole calls: launches, the read-back and the allocation of the output included).
Also tril's time under each forced lane group (BMSP_SELECT_LANES).  Prints one JSON line."""
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


def route_tril(A, out_layout):
    """the pre-existing way to tril(A): device COO, a mask of the triples, the builder"""
    r, c, v = A.to_coo_device()
    tr, tc, tv = as_tensor(r), as_tensor(c), as_tensor(v)
    keep = tc <= tr
    r2, c2, v2 = tr[keep].contiguous(), tc[keep].contiguous(), tv[keep].contiguous()
    i = A.info()
    h = C.c_void_p()
    B.check(B.lib().bmsp_matrix_from_coo_device(i["num_rows"], i["num_cols"], r2.numel(), r2.data_ptr(), c2.data_ptr(), v2.data_ptr(),
                                                int(out_layout), i["dtype"], None, C.byref(h)))
    return B.BmSpMatrix(h.value)


def arrays_bytes(M):
    i = M.info()
    return 24 * i["block_num"] + 8 + ES[i["dtype"]] * i["nnz"]  # keys, bitmaps, offsets (block_num + 1), values


def structure_bytes(M):
    return 24 * M.info()["block_num"] + 8


def median_ms(samples):
    return round(statistics.median(samples), 4)


def bench_case(name, A, v, reps, warmup, note):
    lay = A.info()["transposed"]
    ia = A.info()
    tol = float(np.median(np.abs(np.asarray(v, B.NP_DTYPE[ia["dtype"]]).astype(np.float64))))
    if np.mean(np.abs(v) > tol) < 0.25:  # ties at the median (R-MAT: a third of the values are the identity's 1.0)
        tol = float(np.nextafter(tol, 0.0))
    # the product's structure is all the mask reads (its values stay the zeros of the symbolic pass and move as such)
    AA, _ = B.spgemm_symbolic(A, A.with_layout(1), tc_version=4 if ia["dtype"] == B.F16 else 5)
    ops = {
        "tril": lambda: B.select_band(A, None, 0, transposed=lay),
        "band32": lambda: B.select_band(A, -32, 32, transposed=lay),
        "offdiag": lambda: B.select_band(A, 0, 0, True, transposed=lay),
        "mask_aa_by_a": lambda: B.select_mask(AA, A),
        "mask_aa_by_a_complement": lambda: B.select_mask(AA, A, True),
        "count_tril": lambda: B.band_count(A, None, 0),
        "count_mask": lambda: B.mask_count(AA, A),
        "prune_abs_half": lambda: B.prune(A, tol, "abs", transposed=lay),
        "route_tril": lambda: route_tril(A, lay),
    }
    for _ in range(warmup):
        for f in ops.values():
            timed(f)
    samples = {k: [] for k in ops}
    for _ in range(reps):
        for k, f in ops.items():
            samples[k].append(timed(f))
    iaa = AA.info()
    res = {"case": name, "what": note, "dtype": {0: "fp32", 1: "fp16", 2: "fp64"}[ia["dtype"]], "rows": ia["num_rows"], "nnz": ia["nnz"],
           "tiles": ia["block_num"], "values_per_tile": round(ia["nnz"] / max(1, ia["block_num"]), 2),
           "product": {"dtype": iaa["dtype"], "nnz": iaa["nnz"], "tiles": iaa["block_num"]}, "ms": {}, "kept": {}, "bytes": {}, "gbps": {},
           "hbm_frac": {}}
    for k in ops:
        res["ms"][k] = median_ms(samples[k])
    for k in ("tril", "band32", "offdiag", "mask_aa_by_a", "mask_aa_by_a_complement", "prune_abs_half"):
        P, st = ops[k]()
        src = AA if k.startswith("mask") else A
        res["kept"][k] = {"nnz": st["nnz_out"], "tiles": st["blocks_out"], "share": round(st["nnz_out"] / max(1, st["nnz_in"]), 3)}
        nbytes = structure_bytes(src) + ES[src.info()["dtype"]] * st["nnz_out"] + arrays_bytes(P)
        if k.startswith("mask"):
            nbytes += 16 * ia["block_num"]
        if k == "prune_abs_half":
            nbytes = arrays_bytes(A) + arrays_bytes(P)  # a value rule reads every value
        res["bytes"][k] = nbytes
    res["bytes"]["count_tril"] = 16 * ia["block_num"]
    res["bytes"]["count_mask"] = 16 * (iaa["block_num"] + ia["block_num"])
    for k, nbytes in res["bytes"].items():
        rate = nbytes / (res["ms"][k] * 1e-3)
        res["gbps"][k] = round(rate / 1e9, 1)
        res["hbm_frac"][k] = round(rate / HBM_PEAK, 3)
    res["tril_vs_prune"] = round(res["ms"]["prune_abs_half"] / res["ms"]["tril"], 2)
    res["tril_vs_route"] = round(res["ms"]["route_tril"] / res["ms"]["tril"], 2)
    res["losses"] = sorted(k for k in ("tril", "band32", "offdiag") if res["ms"][k] > res["ms"]["prune_abs_half"] or res["ms"][k] > res["ms"]["route_tril"])
    lanes = {}
    for g in ("1", "8"):
        os.environ["BMSP_SELECT_LANES"] = g
        for _ in range(2):
            timed(ops["tril"])
        lanes["tril_g" + g] = median_ms([timed(ops["tril"]) for _ in range(max(20, reps // 2))])
    del os.environ["BMSP_SELECT_LANES"]
    res["ms_by_lanes"] = lanes
    return res


def cases(quick):
    """(name, A, values, note) -- built outside the timed region"""
    if quick:
        n, _, r, c, v = gen.rmat(12, 2)
        yield "rmat12", B.BmSpMatrix.from_coo(n, n, r, c, v), v, "R-MAT 2^12 x 2 + I"
        n, _, r, c, v = gen.banded(1 << 11, 32)
        yield "banded_s", B.BmSpMatrix.from_coo(n, n, r, c, v), v, "banded 2^11, hb 32"
        return
    n, _, r, c, v = gen.rmat(20, 2)
    yield "rmat20", B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32), v, "R-MAT 2^20 x 2 + I"
    n, _, r, c, v = gen.rmat(16, 8)
    yield "rmat16", B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F16), v, "R-MAT 2^16 x 8 + I"
    n, _, r, c, v = gen.banded(1 << 17, 32)
    yield "banded", B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32), v, "banded 2^17, hb 32"
    n, _, r, c, v = gen.fem_like(47, "27pt")
    yield "fem27", B.BmSpMatrix.from_coo(n, n, r, c, v, dtype=B.F32), v, "fem_like 27pt, 47^3 rows"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="small matrices (a rehearsal of the tool, not a measurement)")
    a = ap.parse_args()
    reps = max(20, a.reps)
    B.set_device(0)
    torch.zeros(1, device="cuda")
    out = []
    for name, A, v, note in cases(a.quick):
        out.append(bench_case(name, A, v, reps, a.warmup, note))
        del A
    print(json.dumps({"tool": "select_bench", "reps": reps, "losses": {res["case"]: res["losses"] for res in out if res["losses"]},
                      "results": out}))


if __name__ == "__main__":
    main()
