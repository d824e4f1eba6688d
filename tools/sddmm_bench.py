#!/usr/bin/env python3
"""Times bmsp_sddmm_values in place (c = d + 0.5 * s: the values stay bounded over the repeats) on
  rmat20   R-MAT 2^20 x 2 + I (the webbase-1M stand-in, hyper-sparse tiles)
  banded   2^17 rows, half-bandwidth 32 (full and near-full tiles)
  fem27    fem_like 27pt (47^3 rows; 3.7 values per tile)
  rmat16   R-MAT 2^16 x 8 (hub block-rows of thousands of tiles)
in fp16 and fp32 at k = 32 and 128, under BMSP_SDDMM_KERNEL = value / tile and the launcher's default.  Per case:
  us         HIP events around --batch launches after warm-up, the kernels interleaved sample by sample; the median of --reps samples
  hbm_frac   bmsp_sddmm_launch_info's compulsory_bytes / time as a fraction of the 8 TB/s HBM peak (operand rows are counted once per
             tile that touches them, so a kernel served by the caches can exceed what HBM alone would allow)
  route_us   the route a caller had before: to_coo_device, a torch gather-multiply-sum of the X and Y rows on the device, the builder
  default_is_fastest   whether the launcher's own choice is the faster of the two kernels (the rule the threshold is set by)
fill_sweep: both kernels on a half-bandwidth-32 band thinned at random to 3 .. 58 values per tile -- where the default should change.
Prints one JSON line."""
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

DT = {B.F32: "fp32", B.F16: "fp16"}
HBM_PEAK = 8.0e12  # bytes/s, MI355X spec
KERNELS = ("value", "tile", "default")


class _Raw:
    """a DeviceArray seen through __cuda_array_interface__ (no copy)"""

    def __init__(self, d):
        self.d = d
        self.__cuda_array_interface__ = {"shape": (d.n,), "typestr": d.dtype.str, "data": (d.ptr, False), "version": 2}


def as_tensor(d):
    return torch.as_tensor(_Raw(d), device="cuda")


def force(kernel):
    if kernel == "default":
        os.environ.pop("BMSP_SDDMM_KERNEL", None)
    else:
        os.environ["BMSP_SDDMM_KERNEL"] = kernel


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


def route(S, Xt, Yt, k):
    """the pre-existing way: device COO, gather both operand rows per stored coordinate, multiply, reduce in fp32, add 0.5 * s, the
    builder"""
    r, c, v = S.to_coo_device()
    rows, cols, vals = as_tensor(r).long(), as_tensor(c).long(), as_tensor(v)
    d = (Xt[rows].float() * Yt[cols].float()).sum(dim=1)
    v2 = (d.double() + 0.5 * vals).contiguous()
    i = S.info()
    h = C.c_void_p()
    B.check(B.lib().bmsp_matrix_from_coo_device(i["num_rows"], i["num_cols"], rows.numel(), r.ptr, c.ptr, v2.data_ptr(), i["transposed"],
                                                i["dtype"], None, C.byref(h)))
    return B.BmSpMatrix(h.value)


def operands(nr, nc, k, dtype):
    rng = np.random.default_rng(7)
    draw = lambda n: (rng.uniform(0.5, 2.0, (n, k)) * rng.choice([-1.0, 1.0], (n, k)) / np.sqrt(k)).astype(B.NP_DTYPE[dtype])
    return B.DeviceArray.from_host(draw(nr).ravel()), B.DeviceArray.from_host(draw(nc).ravel())


def bench_kernels(S, X, Y, k, a):
    """{kernel: us} of the in-place value pass under each switch, and the launcher's description of each"""
    fns, infos = {}, {}
    for kern in KERNELS:
        force(kern)
        infos[kern] = B.sddmm_launch_info(S, k)

        def run(kern=kern):
            force(kern)
            B.sddmm_values(S, S, X, Y, k, 1.0, 0.5)
        fns[kern] = run
    us = steady_us(fns, a.batch, a.reps, a.warmup)
    force("default")
    return us, infos


def bench_case(name, coo, dtype, k, a, with_route=True):
    nr, nc, r, c, vals = coo
    S = B.BmSpMatrix.from_coo(nr, nc, r, c, vals, dtype=dtype)
    i = S.info()
    X, Y = operands(nr, nc, k, dtype)
    us, infos = bench_kernels(S, X, Y, k, a)
    res = {"matrix": name, "dtype": DT[dtype], "k": k, "rows": nr, "nnz": i["nnz"], "tiles": i["block_num"],
           "values_per_tile": round(i["nnz"] / max(1, i["block_num"]), 2), "us": us,
           "kernel": {kern: infos[kern]["kernel"] for kern in KERNELS},
           "compulsory_bytes": {kern: infos[kern]["compulsory_bytes"] for kern in KERNELS},
           "hbm_frac": {kern: round(infos[kern]["compulsory_bytes"] / (us[kern] * 1e-6) / HBM_PEAK, 3) for kern in KERNELS}}
    faster = "tile" if us["tile"] < us["value"] else "value"
    res["faster"] = faster
    res["default_is_fastest"] = infos["default"]["kernel"] == infos[faster]["kernel"]
    if with_route:
        Xt, Yt = as_tensor(X).view(nr, k), as_tensor(Y).view(nc, k)
        rt = steady_us({"route": lambda: route(S, Xt, Yt, k)}, 1, max(3, a.reps // 3), 1)["route"]
        res["route_us"] = rt
        res["speedup_vs_route"] = round(rt / us["default"], 1)
    return res


def thinned_band(n, hb, keep, seed=3):
    nr, nc, r, c, v = gen.banded(n, hb)
    m = np.random.default_rng(seed).random(r.size) < keep
    return nr, nc, r[m], c[m], v[m]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--batch", type=int, default=10, help="launches per timed sample")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="small matrices (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--no-route", action="store_true", help="skip the torch route")
    a = ap.parse_args()
    B.set_device(0)
    if a.quick:
        mats = [("rmat12", lambda: gen.rmat(12, 2)), ("banded_s", lambda: gen.banded(1 << 10, 32))]
        ks, keeps, band_n = (32,), (0.1, 1.0), 1 << 10
    else:
        mats = [("rmat20 (webbase-1M-like)", lambda: gen.rmat(20, 2)), ("banded_hb32", lambda: gen.banded(1 << 17, 32)),
                ("fem27", lambda: gen.fem_like(47, "27pt")), ("rmat16x8", lambda: gen.rmat(16, 8))]
        ks, keeps, band_n = (32, 128), (0.05, 0.1, 0.15, 0.2, 0.3, 0.5, 1.0), 1 << 16
    out = []
    for name, make in mats:
        coo = make()
        for dtype in (B.F16, B.F32):
            for k in ks:
                out.append(bench_case(name, coo, dtype, k, a, with_route=not a.no_route))
    sweep = []
    for keep in keeps:
        coo = thinned_band(band_n, 32, keep)
        for dtype in (B.F16, B.F32):
            for k in ks:
                row = bench_case("band thinned to %g" % keep, coo, dtype, k, a, with_route=False)
                sweep.append({key: row[key] for key in ("matrix", "dtype", "k", "values_per_tile", "us", "faster", "default_is_fastest")})
    print(json.dumps({"tool": "sddmm_bench", "reps": a.reps, "batch": a.batch, "results": out, "fill_sweep": sweep}))


if __name__ == "__main__":
    main()
