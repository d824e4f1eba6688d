#!/usr/bin/env python3
"""Times bmsp_spgemm_masked_values (C = (A * B) on M's pattern; alpha = 1, beta = 0, into a prebuilt output) with M = A and B = A in the
other tile layout on
  fem27 fp32        fem_like 27pt (47^3 rows)
  cage12_like fp16  with an F32 mask (what bmsp_spgemm returns for F16 operands)
  rmat16x8 fp16     R-MAT 2^16 x 8 (hub block-rows and block-columns of thousands of tiles)
  banded fp32       2^17 rows, half-bandwidth 32 (full and near-full tiles)
and on fem27 fp32 with M = prune(A * A, 0.25, row_rel, keep diagonal).  Per case, all in one session:
  us            HIP events around one call each, the candidates interleaved sample by sample, the median of --reps samples:
                masked under BMSP_MASKED_LANES = 1 / 8 and the launcher's default; bmsp_spgemm(A, B) whole; bmsp_spgemm_numeric alone on
                a prebuilt C; and the only route to the same matrix there was before: the whole product, to_coo_device, a torch
                searchsorted sample at M's coordinates (M's own COO is made once, outside the timing), from_coo_device
  first_call_us the masked call on a B without its op-T view (host clock around call + synchronise: the view is built inside)
  pairs         bmsp_spgemm_masked_launch_info's count of (M tile, K) matches, pairs per second at the default, and the list lengths
                (tiles in A's block-row, in B's block-column) of the M tile with the longest shorter list: that tile is one lane
                group's serial chain
fill_sweep: one lane against eight lanes per tile on a half-bandwidth-32 band thinned at random to 3 .. 58 values per tile (M = A, B = A
in the other layout) -- where the default should change.
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
import torch  # noqa: E402  (before pybmsp: both share one HIP runtime)
import pybmsp as B  # noqa: E402
from pybmsp import gen  # noqa: E402

DT = {B.F32: "fp32", B.F16: "fp16", B.F64: "fp64"}
LANES = ("1", "8", "default")


class _Raw:
    """a DeviceArray seen through __cuda_array_interface__ (no copy)"""

    def __init__(self, d):
        self.d = d
        self.__cuda_array_interface__ = {"shape": (d.n,), "typestr": d.dtype.str, "data": (d.ptr, False), "version": 2}


def as_tensor(d):
    return torch.as_tensor(_Raw(d), device="cuda")


def force(lanes):
    if lanes == "default":
        os.environ.pop("BMSP_MASKED_LANES", None)
    else:
        os.environ["BMSP_MASKED_LANES"] = lanes


def steady_us(fns, reps, warmup):
    """{name: median microseconds per call}, the functions interleaved sample by sample"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    B.synchronize()
    samples = {k: [] for k in fns}
    e0, e1 = B.Event(), B.Event()
    for _ in range(reps):
        for k, f in fns.items():
            e0.record()
            f()
            e1.record()
            samples[k].append(e0.elapsed_ms(e1) * 1e3)
    return {k: round(statistics.median(s), 2) for k, s in samples.items()}


def route(A, Bm, tc, m_key, m_rows, m_cols, info):
    """the pre-existing way: the whole product, its device COO, a sorted look-up of M's coordinates, the builder"""
    P, _ = B.spgemm(A, Bm, tc_version=tc)
    r, c, v = P.to_coo_device()
    key = as_tensor(r).long() * info["num_cols"] + as_tensor(c).long()
    vals = as_tensor(v)
    pos = torch.searchsorted(key, m_key).clamp(max=max(0, key.numel() - 1))
    out = torch.where(key[pos] == m_key, vals[pos], torch.zeros((), dtype=vals.dtype, device=vals.device)).contiguous()
    h = C.c_void_p()
    B.check(B.lib().bmsp_matrix_from_coo_device(info["num_rows"], info["num_cols"], m_key.numel(), m_rows.ptr, m_cols.ptr, out.data_ptr(),
                                                info["transposed"], info["dtype"], None, C.byref(h)))
    return B.BmSpMatrix(h.value)


def longest_tile(A, Bm, M):
    """(tiles in A's block-row, tiles in B's block-column) of the M tile whose shorter list is the longest"""
    keys = M.host_arrays()[0]
    la = np.diff(A.block_row_ptr().astype(np.int64))
    bcols = (Bm.host_arrays()[0] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    lb = np.bincount(bcols, minlength=(Bm.info()["num_cols"] + 7) // 8)
    a = la[(keys >> np.uint64(32)).astype(np.int64)]
    b = lb[(keys & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    t = int(np.argmax(np.minimum(a, b)))
    return int(a[t]), int(b[t])


def bench_case(name, coo, dtype, mdtype, a, mask=None, with_route=True, yardsticks=True):
    nr, nc, r, c, vals = coo
    tc = 5 if dtype == B.F32 else 4
    A = B.BmSpMatrix.from_coo(nr, nc, r, c, vals, dtype=dtype)
    Bm = A.with_layout(1)
    if mask is None:
        M = A if mdtype == dtype else B.BmSpMatrix.from_coo(nr, nc, r, c, vals, dtype=mdtype)
    else:
        M = mask(A, Bm, tc)
    out = M.with_layout(0)
    i = M.info()
    # the first call on a B without its view
    B.synchronize()
    t0 = time.perf_counter()
    B.spgemm_masked_values(out, A, Bm, M)
    B.synchronize()
    first_us = (time.perf_counter() - t0) * 1e6
    infos = {}
    fns = {}
    for lanes in LANES:
        force(lanes)
        infos[lanes] = B.spgemm_masked_launch_info(A, Bm, M)

        def run(lanes=lanes):
            force(lanes)
            B.spgemm_masked_values(out, A, Bm, M)
        fns["masked_" + lanes] = run
    if yardsticks:
        P, st = B.spgemm(A, Bm, tc_version=tc)
        fns["spgemm"] = lambda: B.spgemm(A, Bm, tc_version=tc)
        fns["spgemm_numeric"] = lambda: B.spgemm_numeric(A, Bm, P, tc_version=tc)
    us = steady_us(fns, a.reps, a.warmup)
    force("default")
    faster = "8" if us["masked_8"] < us["masked_1"] else "1"
    if not yardsticks:
        return {"matrix": name, "dtype": DT[dtype], "m_values_per_tile": round(i["nnz"] / max(1, i["block_num"]), 2), "us": us,
                "faster_lanes": faster, "default_is_fastest": infos["default"]["kernel"] == infos[faster]["kernel"]}
    la, lb = longest_tile(A, Bm, M)
    pairs = infos["default"]["pairs"]
    res = {"matrix": name, "dtype": DT[dtype], "mask_dtype": DT[mdtype], "rows": nr, "a_nnz": A.info()["nnz"], "a_tiles": A.info()["block_num"],
           "m_nnz": i["nnz"], "m_tiles": i["block_num"], "m_values_per_tile": round(i["nnz"] / max(1, i["block_num"]), 2),
           "product_nnz": P.info()["nnz"], "product_tiles": P.info()["block_num"], "surviving_tasks": st["surviving_tasks"],
           "task_list_size": st["task_list_size"], "us": us, "first_call_us": round(first_us, 1),
           "kernel": {k: infos[k]["kernel"] for k in LANES}, "view_bytes": infos["default"]["view_bytes"], "pairs": pairs,
           "pairs_per_s": round(pairs / (us["masked_default"] * 1e-6), 0), "longest_tile_lists": [la, lb],
           "faster_lanes": faster, "default_is_fastest": infos["default"]["kernel"] == infos[faster]["kernel"],
           "speedup_vs_spgemm": round(us["spgemm"] / us["masked_default"], 2),
           "speedup_vs_numeric": round(us["spgemm_numeric"] / us["masked_default"], 2)}
    if with_route:
        mr, mc, _ = M.to_coo_device()
        m_key = as_tensor(mr).long() * i["num_cols"] + as_tensor(mc).long()
        rt = steady_us({"route": lambda: route(A, Bm, tc, m_key, mr, mc, i)}, max(3, a.reps // 5), 1)["route"]
        res["route_us"] = rt
        res["speedup_vs_route"] = round(rt / us["masked_default"], 1)
    return res


def pruned_product(A, Bm, tc):
    P, _ = B.spgemm(A, Bm, tc_version=tc)
    M, _ = B.prune(P, 0.25, "row_rel", keep_diagonal=True)
    return M


def thinned_band(n, hb, keep, seed=3):
    nr, nc, r, c, v = gen.banded(n, hb)
    m = np.random.default_rng(seed).random(r.size) < keep
    return nr, nc, r[m], c[m], v[m]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="small matrices (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--no-route", action="store_true", help="skip the torch route")
    a = ap.parse_args()
    B.set_device(0)
    if a.quick:
        cases = [("rmat12", lambda: gen.rmat(12, 2), B.F16, B.F16, None), ("banded_s", lambda: gen.banded(1 << 10, 32), B.F32, B.F32, None),
                 ("fem27_s10 pruned", lambda: gen.fem_like(10, "27pt"), B.F32, B.F32, pruned_product)]
        keeps, band_n = (0.1, 1.0), 1 << 10
    else:
        cases = [("fem27", lambda: gen.fem_like(47, "27pt"), B.F32, B.F32, None),
                 ("cage12_like", lambda: gen.cage_like(130228, 15.6), B.F16, B.F32, None),
                 ("rmat16x8", lambda: gen.rmat(16, 8), B.F16, B.F16, None),
                 ("banded_hb32", lambda: gen.banded(1 << 17, 32), B.F32, B.F32, None),
                 ("fem27, M = prune(A*A, 0.25 row_rel)", lambda: gen.fem_like(47, "27pt"), B.F32, B.F32, pruned_product)]
        keeps, band_n = (0.05, 0.08, 0.1, 0.12, 0.15, 0.2, 0.3, 0.5, 1.0), 1 << 16
    out = []
    for name, make, dtype, mdtype, mask in cases:
        out.append(bench_case(name, make(), dtype, mdtype, a, mask, with_route=not a.no_route))
    sweep = []
    for keep in keeps:
        coo = thinned_band(band_n, 32, keep)
        for dtype in (B.F16, B.F32):
            sweep.append(bench_case("band thinned to %g" % keep, coo, dtype, dtype, a, with_route=False, yardsticks=False))
    print(json.dumps({"tool": "spgemm_masked_bench", "reps": a.reps, "results": out, "fill_sweep": sweep}))


if __name__ == "__main__":
    main()
