"""bmsp_spmv, bmsp_spmm, bmsp_spmv_op and bmsp_spmv_sharded on Inf, NaN, subnormals and overflowing sums INSIDE stored tiles, on every kernel.

The contract (bmsp.h, bmsp_spmv): u_i is the sum over the STORED entries of row i of a * v.  An element of v at a column where row i
stores nothing never reaches u_i, whatever it holds -- inside a stored tile too; a stored value is always multiplied (stored 0 against Inf
gives NaN, a stored Inf / NaN propagates); fp32 arithmetic (double for F64), F16 widened exactly, subnormals kept; a row without stored
entries is +0.  The CPU oracle multiplies whole tiles (0 * Inf = NaN at every position a tile does not store), so it is no reference here;
the reference of this file is `reference` below: per output, the np.longdouble sum of the stored products, with the IEEE class rules
written out.

There is no tolerance in this file.  Finite data are small integers times a power of two, so that every finite partial sum is exactly
representable in the accumulator type in ANY order, fused or not (test_inputs_are_exact_and_hit_their_classes proves it on the CPU: per
output, the products are multiples of one power of two q and the sum of their magnitudes stays below 2^24 q, 2^53 q for F64).  A special
value then only decides the class of an output -- finite, +Inf, -Inf or NaN -- and the class does not depend on the order either: products
that overflow share one sign per row, meet no Inf or NaN there, and every other finite product of such a row is below 2^60.  NaNs are compared by position, everything
else as numbers (-0 == +0); bit for bit only where two launches of the same kernel are compared with each other.

Matrices (about a thousand rows: the smallest at which every kernel is still chosen): `dense` banded(1003, 21), `mid` random 777 x 1234
with every nibble pattern, `sparse` random 1237 x 911; from each every entry is removed whose column is in D_c = {c : c % 8 in (2, 5)} or
whose row is in D_r = {r : r % 8 in (1, 6)}: every surviving tile has holes at fixed positions next to stored values (the dense kind turns
into nibbles 1101 and 1011 -- the partly filled branch of spmv_rowgroup_kernel) and the rows of D_r are empty rows inside stored tiles.
One kernel cannot be launched on such a matrix: spmv_sweep_kernel<FULL> needs a quarter of the tiles FULL.  Its launch runs on `full`, the
dense kind with the holes in every fourth block-column and block-row only, and so does a launch of spmv_rowgroup_kernel (full nibbles
beside absent and partly filled ones: its fast branch); every test runs on that kind as on the others, the planted values inside its
full tiles.

Test A: x = +Inf, -Inf, NaN in rotation at every index of D_c (D_r for op T): no output may see them.
Test B: stored NaN / Inf / zeros, Inf and NaN in x at stored columns, sums that overflow: the IEEE class and the value of every output.
Test C: subnormal values or a subnormal x: kept exactly.
Test D: v and u one element into their allocations: the same bits, the neighbours of u untouched.
"""
import numpy as np
import pytest

import util
from util import SPMV_LAUNCHES, SPMV_LAUNCH_DTYPES, SPMV_CHUNK_LAYOUT, SPMM_LAUNCHES

NPDT = {0: np.float32, 1: np.float16, 2: np.float64}
OUTDT = {0: np.float32, 1: np.float32, 2: np.float64}
UINT = {4: np.uint32, 8: np.uint64}
DT = ("f32", "f16", "f64")
LD = np.longdouble
INF, NAN = float("inf"), float("nan")
HOLE_C, HOLE_R = (2, 5), (1, 6)
KINDS = ("dense", "mid", "sparse")

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------
# 0. the matrices
# ---------------------------------------------------------------------------------------------------------
def hole_cols(kind, nc):
    i = np.arange(nc)
    m = np.isin(i % 8, HOLE_C)
    return i[m & ((i // 8) % 4 == 1)] if kind == "full" else i[m]


def hole_rows(kind, nr):
    i = np.arange(nr)
    m = np.isin(i % 8, HOLE_R)
    return i[m & ((i // 8) % 4 == 2)] if kind == "full" else i[m]


def structure(kind):
    """(nr, nc, r, c): coordinates sorted by (r, c), without the entries of D_c and D_r"""
    def make():
        from pybmsp import gen
        if kind in ("dense", "full"):
            nr = nc = 1003
            _, _, r, c, _ = gen.banded(1003, 21)
        elif kind == "mid":
            nr, nc, r, c, _ = gen.random_coo(777, 1234, 120000, seed=11)
        else:
            nr, nc = 1237, 911
            g = np.random.default_rng(77)
            r, c = g.integers(0, nr, 14000), g.integers(0, nc, 14000)
        key = np.unique(np.asarray(r, np.int64) * nc + np.asarray(c, np.int64))
        r, c = key // nc, key % nc
        keep = ~(np.isin(c, hole_cols(kind, nc)) | np.isin(r, hole_rows(kind, nr)))
        return nr, nc, r[keep], c[keep]
    return cached(("structure", kind), make)


def operand(kind, op):
    """op(A) as (n_out, n_in, o, i, D_in, D_out): output and input index of every stored entry, the input indices no entry has, the
    outputs without entries inside stored tiles"""
    nr, nc, r, c = structure(kind)
    if op == "T":
        return nc, nr, c, r, hole_rows(kind, nr), hole_cols(kind, nc)
    return nr, nc, r, c, hole_cols(kind, nc), hole_rows(kind, nr)


def ints(o, i):
    """-2, -1, 1, 2 by position"""
    v = ((o * 3 + i * 7) % 5 - 2).astype(np.float64)
    v[v == 0] = 1.0
    return v


def xints(n):
    """-10 .. 10 without 0"""
    x = ((np.arange(n) % 21) - 10).astype(np.float64)
    x[x == 0] = 3.0
    return x


def u0_for(n_out):
    """the finite u of the beta != 0 launches: even integers (beta = 0.5 keeps them integers)"""
    return 2.0 * ((np.arange(n_out) % 7) - 3)


def poisoned_x(kind, op):
    """(x, x0): x holds +Inf, -Inf, NaN in rotation at every index no entry has, x0 zeros there"""
    n_in, D_in = operand(kind, op)[1], operand(kind, op)[4]
    x0 = xints(n_in)
    x0[D_in] = 0.0
    x = x0.copy()
    x[D_in] = np.array([INF, -INF, NAN])[np.arange(D_in.size) % 3]
    return x, x0


# ---------------------------------------------------------------------------------------------------------
# 1. the reference
# ---------------------------------------------------------------------------------------------------------
def rounded(v, dtype):
    with np.errstate(over="ignore"):
        return np.asarray(v, np.float64).astype(NPDT[dtype]).astype(np.float64)


def reference(n_out, o, i, a, x, dtype):
    """t = op(A) x by the contract, and why: per output, over its stored entries, in np.longdouble from the operands as stored.  Any NaN
    product (a NaN operand, 0 * Inf) -> NaN; products of both infinite signs -> NaN; of one infinite sign -> that Inf, where a product is
    infinite from a magnitude of 2^128 on (2^1024 for F64); otherwise the exact finite sum.  Returns (t, flags), flags a dict of per-output
    masks naming the causes."""
    assert np.finfo(LD).nmant >= 63 and np.finfo(LD).maxexp > 1100
    a, xi = rounded(a, dtype), rounded(x, dtype)[i]
    lim = np.ldexp(LD(1), 1024 if dtype == 2 else 128)
    with np.errstate(invalid="ignore"):
        p = a.astype(LD) * xi.astype(LD)
    nanp = np.isnan(p)
    big = ~nanp & np.isfinite(a) & np.isfinite(xi) & (np.abs(p) >= lim)          # finite operands, the product overflows
    infp = ~nanp & (np.isinf(a) | np.isinf(xi))
    pos, neg = (big | infp) & (p > 0), (big | infp) & (p < 0)
    fin = ~(nanp | big | infp)
    has = lambda m: np.bincount(o[m], minlength=n_out) > 0
    s = np.zeros(n_out, LD)
    np.add.at(s, o[fin], p[fin])
    t = s.copy()
    t[has(pos)] = LD(INF)
    t[has(neg)] = -LD(INF)
    t[has(nanp) | (has(pos) & has(neg))] = LD(NAN)
    flags = {"nan_operand": has(nanp & (np.isnan(a) | np.isnan(xi))), "stored_nan": has(np.isnan(a)), "zero_inf": has(nanp & ~np.isnan(a) & ~np.isnan(xi)),
             "nan_product": has(nanp), "inf_pos": has(infp & (p > 0)), "inf_neg": has(infp & (p < 0)), "big_pos": has(big & (p > 0)), "big_neg": has(big & (p < 0)),
             "other_below_2_60": ~has(fin & (np.abs(p) >= np.ldexp(LD(1), 60))), "finite_sum": s, "products": (p, fin)}
    return t, flags


def expected(t, alpha, beta, u0, dtype):
    """the epilogue on the reference's t, in the output type (every finite value is exact there)"""
    with np.errstate(invalid="ignore", over="ignore"):
        e = LD(alpha) * t
        if beta != 0:
            e = e + LD(beta) * u0.astype(LD)
        return e.astype(OUTDT[dtype])


def assert_class_and_value(got, want, what=""):
    """NaN by position; everything else, +-Inf included, as numbers (-0 == +0)"""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.argwhere(gn != wn)
    assert bad.size == 0, "%s: NaN mask differs at %d outputs, first %s: got %r, want %r" % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    bad = np.argwhere(~gn & (got != want))
    assert bad.size == 0, "%s: %d outputs differ, first %s: got %r, want %r" % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def bits(a):
    return np.ascontiguousarray(a).view(UINT[a.dtype.itemsize])


def check_a(out, out0, want0, zero_rows):
    """test A's comparison: out = the launch on the poisoned x, out0 = on x0, want0 = the exact product of x0, zero_rows = the outputs that
    must be +0 (None when beta != 0)"""
    assert np.isfinite(out).all(), "Inf / NaN at outputs %s" % np.argwhere(~np.isfinite(out))[:8].tolist()
    np.testing.assert_array_equal(bits(out), bits(out0))
    np.testing.assert_array_equal(out0.astype(np.float64), want0)
    if zero_rows is not None:
        assert not bits(out)[zero_rows].any(), "an output without stored entries is not +0"


# ---------------------------------------------------------------------------------------------------------
# 2. the inputs of tests B and C
# ---------------------------------------------------------------------------------------------------------
BIG = {0: (120, 8), 1: None, 2: (1000, 30)}   # overflow: entries m 2^120 against x = 2^8 (F64: 2^1000, 2^30); F16: 65504 against 65504, exact in fp32
NEED = {"pinf": 48, "ninf": 32, "nan": 32, "big": 128}   # outputs that must store a column of each kind of special x


def planted(kind, op, dtype):
    """(a, x, zeros): test B's values and vector on operand(kind, op), and the number of stored zeros among a.
    x: +Inf / -Inf / NaN / the large value at a few input indices that ARE stored, taken from a fixed pseudo-random order of the candidates
    of one residue mod 8 each until NEED outputs store them.  Outputs that store a +Inf column: every second one holds a stored ZERO there
    (0 * Inf).  Outputs that store a large-x column and no Inf / NaN column: three of four hold m 2^120, m in {1, 2}, of ONE sign per output,
    at all such columns (F16: 65504 there and stored zeros elsewhere: k 65504^2, k <= 4, is exact in fp32 -- there is no overflow class for
    F16).  An overflowing product never shares an output with an Inf or NaN: a fused multiply-add does not round the product, so
    fma(2^120, 2^8, -Inf) is -Inf where the separate multiply gives +Inf - Inf = NaN -- the class would depend on the kernel.  Of the
    outputs no special x reaches, by rank mod 8: a stored NaN, a stored +Inf, a stored -Inf (each at the middle entry of the output: inside
    the band, where the full kind's full tiles are), +Inf and -Inf products together (the two middle entries); four stay finite."""
    def make():
        n_out, n_in, o, i, D_in, _ = operand(kind, op)
        a, x = ints(o, i), xints(n_in)
        touched = np.zeros(n_out, bool)
        cols = {}
        for name, residue in (("pinf", 0), ("ninf", 3), ("nan", 4), ("big", 7)):
            cand = np.arange(residue, n_in, 8)
            cand = cand[np.argsort((cand * 2654435761 + 12345) % 1000003, kind="stable")]
            whole = cand[~np.isin(cand // 8, D_in // 8)]      # the full kind: block-columns without holes first, where the full tiles are
            cand = np.concatenate((whole, cand[np.isin(cand // 8, D_in // 8)]))
            seen, take = np.zeros(n_out, bool), []
            for c in cand:
                if seen.sum() >= NEED[name]:
                    break
                rows = o[i == c]
                if rows.size:
                    take.append(c)
                    seen[rows] = True
            assert seen.sum() >= NEED[name], (kind, op, name, seen.sum())
            cols[name] = np.array(take)
            if name == "big":
                special = touched.copy()      # outputs that an Inf or NaN of x reaches
            touched |= seen
        x[cols["pinf"]], x[cols["ninf"]], x[cols["nan"]] = INF, -INF, NAN
        # stored zeros against +Inf
        at = np.flatnonzero(np.isin(i, cols["pinf"]))
        rank = {r: k for k, r in enumerate(np.unique(o[at]))}
        z = at[[rank[r] % 2 == 0 for r in o[at]]]
        a[z] = 0.0
        # sums that overflow
        at = np.flatnonzero(np.isin(i, cols["big"]))
        rank = {r: k for k, r in enumerate(np.unique(o[at]))}
        sel = at[[rank[r] % 4 != 3 and not special[r] for r in o[at]]]
        sign = np.array([1.0 if rank[r] % 8 < 4 else -1.0 for r in o[sel]])
        if dtype == 1:
            x[cols["big"]] = 65504.0
            rows_big = np.unique(o[sel])
            a[np.isin(o, rows_big) & np.isfinite(a)] = 0.0
            a[sel] = sign * 65504.0
        else:
            x[cols["big"]] = np.ldexp(1.0, BIG[dtype][1])
            a[sel] = sign * (1 + (i[sel] // 8) % 2) * np.ldexp(1.0, BIG[dtype][0])
        # stored special values in outputs no special x reaches
        cnt = np.bincount(o, minlength=n_out)
        first = np.concatenate(([0], np.cumsum(cnt)[:-1]))      # (o is sorted for op N only: work on a sorted view)
        order = np.lexsort((i, o))
        free = np.flatnonzero(~touched & (cnt >= 2))
        for k, r in enumerate(free):
            e = order[first[r]:first[r] + cnt[r]]
            if k % 8 == 0:
                a[e[cnt[r] // 2]] = NAN
            elif k % 8 == 1:
                a[e[cnt[r] // 2]] = INF
            elif k % 8 == 2:
                a[e[cnt[r] // 2]] = -INF
            elif k % 8 == 3:
                e0, e1 = e[cnt[r] // 2 - 1], e[cnt[r] // 2]
                a[e0] = INF * np.sign(x[i[e0]])
                a[e1] = -INF * np.sign(x[i[e1]])
        return a, x, int((a == 0).sum())
    return cached(("planted", kind, op, dtype), make)


TINY = {0: -149, 1: -24, 2: -1074}   # the smallest subnormal of the storage type


def subnormal(kind, op, dtype, which):
    """(a, x, exact t): which = "values": a = small integers * the smallest subnormal, x small integers; which = "x": the other way round.
    t = (integer product) * 2^TINY, formed in np.longdouble"""
    def make():
        n_out, n_in, o, i, _, _ = operand(kind, op)
        a, x = ints(o, i), xints(n_in)
        s = np.zeros(n_out)
        np.add.at(s, o, a * x[i])
        t = np.ldexp(s.astype(LD), TINY[dtype])
        tiny = np.ldexp(1.0, TINY[dtype])
        return (a * tiny, x, t) if which == "values" else (a, x * tiny, t)
    return cached(("subnormal", kind, op, dtype, which), make)


# ---------------------------------------------------------------------------------------------------------
# 3. the launches
# ---------------------------------------------------------------------------------------------------------
class Launch:
    def __init__(self, name, api, kind, kernel, env=None, dtypes=(0, 1, 2), variant=0, op="N", layout=False, k=0, alpha=1.0, beta=0.0, slots=None, split=None):
        self.name, self.api, self.kind, self.kernel, self.env, self.dtypes, self.variant = name, api, kind, kernel, dict(env or {}), dtypes, variant
        self.op, self.layout, self.k, self.alpha, self.beta, self.slots, self.split = op, layout, k, alpha, beta, slots, split
        if slots:
            self.env["BMSP_SPMV_OP_SLOTS"] = str(slots)
        if split:
            self.env["BMSP_SPMV_OP_SPLIT"] = str(split)


# what bmsp_spmv's default variant launches on each kind (bmsp_spmv_op (N, row-major) is that call)
DEFAULT_KERNEL = {"dense": "spmv_rowgroup_kernel", "mid": "spmv_vstream_kernel<kCached, kSorted>", "sparse": "spmv_vstream_kernel<kCached, kAtomic>"}


def _launches():
    out = []
    for name, (kind, env, variant, kernel) in SPMV_LAUNCHES.items():
        kind = "full" if kernel.endswith("<FULL>") else kind
        out.append(Launch(name, "spmv", kind, kernel, env, SPMV_LAUNCH_DTYPES.get(name, (0, 1, 2)), variant))
    # the mid kind (every nibble pattern) on the kernels that take it, and the dense kind with the row-group kernel switched off
    out += [Launch("mid_default", "spmv", "mid", DEFAULT_KERNEL["mid"]), Launch("mid_rowgroup", "spmv", "mid", "spmv_rowgroup_kernel", variant=3),
            Launch("mid_blockrow_batched", "spmv", "mid", "spmv_blockrow_kernel<64", variant=1), Launch("mid_blockrow_8", "spmv", "mid", "spmv_blockrow_kernel<8", variant=2),
            Launch("dense_no_rowgroup", "spmv", "dense", "spmv_vstream_kernel<", {"BMSP_SPMV_NO_ROWGROUP": "1"}),
            # full tiles beside holed ones: the row-group kernel's fast branch (every nibble of a trip 0xF or 0) next to its partly filled one
            Launch("full_rowgroup", "spmv", "full", "spmv_rowgroup_kernel", variant=3)]
    for name, (kind, novs, k, kernel) in SPMM_LAUNCHES.items():
        out.append(Launch("spmm_" + name, "spmm", kind, kernel, {"BMSP_SPMM_NO_VSTREAM": "1"} if novs else {}, k=k))
    out.append(Launch("spmm_k1_dense", "spmm", "dense", "spmv: spmv_rowgroup_kernel", k=1))
    for kind in KINDS:
        for op in "NT":
            for layout in (False, True):
                tag = "op_%s_%s_%s" % (kind, op, "col" if layout else "row")
                out.append(Launch(tag + "_slots1", "op", kind, None, op=op, layout=layout, slots=1))
                out.append(Launch(tag + "_slots8_ab", "op", kind, None, op=op, layout=layout, slots=8, alpha=2.0, beta=0.5))
                if kind == "dense":
                    out.append(Launch(tag + "_split4", "op", kind, None, op=op, layout=layout, slots=8, split=4))
    out.append(Launch("sharded_dense", "sharded", "dense", "spmv_rowgroup_kernel"))
    out.append(Launch("sharded_sparse", "sharded", "sparse", "spmv_vstream_kernel<", {"BMSP_SPMV_NOCHUNK": "1"}))
    return out


LAUNCHES = {L.name: L for L in _launches()}
PARAMS = [pytest.param(L.name, d, id="%s-%s" % (L.name, DT[d])) for L in LAUNCHES.values() for d in L.dtypes]
SPMV_PARAMS = [pytest.param(L.name, d, id="%s-%s" % (L.name, DT[d])) for L in LAUNCHES.values() if L.api == "spmv" for d in L.dtypes]

def make_matrix(bmsp, monkeypatch, L, dtype, a):
    """the environment of the launch, the matrix of values `a` on operand(L.kind, L.op), and the assertion that the launcher picks the kernel"""
    for key, val in L.env.items():
        monkeypatch.setenv(key, val)
    nr, nc, r, c = structure(L.kind)
    A = bmsp.BmSpMatrix.from_coo(nr, nc, r, c, a, transposed=L.layout, dtype=dtype)
    assert A.nnz == r.size, (A.nnz, r.size)   # stored zeros, NaN and subnormals are all stored
    if L.api == "spmv":
        info = bmsp.spmv_launch_info(A, L.variant)
        assert info["kernel"].startswith(L.kernel), info
        if L.name in SPMV_CHUNK_LAYOUT:
            assert bmsp.spmv_chunk_layout(A) == SPMV_CHUNK_LAYOUT[L.name]
    elif L.api == "spmm":
        info = bmsp.spmm_launch_info(A, L.k)
        assert info.startswith(L.kernel) if L.k == 1 else info == L.kernel, info
    elif L.api == "op":
        info = bmsp.spmv_op_launch_info(A, L.op)
        if L.op == "N" and not L.layout:
            assert info["kernel"] == "bmsp_spmv: " + DEFAULT_KERNEL[L.kind], info
        else:
            minor = "MINOR" if (L.op == "T") != L.layout else "MAJOR"
            assert info["kernel"] == "spmv_op_sweep_kernel<%s, %d>" % (minor, L.slots), info
            assert not L.split or info["split_blocks"] > 0, info
    else:   # the sharded sweep: the whole matrix and three row panels of it
        nbr = (nr + 7) // 8
        for lo, hi in ((0, nbr), (0, nbr // 3), (nbr // 3, 2 * nbr // 3), (2 * nbr // 3, nbr)):
            M = A if (lo, hi) == (0, nbr) else A.row_panel(lo, hi)
            info = bmsp.spmv_launch_info(M, L.variant)
            assert info["kernel"].startswith(L.kernel), (lo, hi, info)
    return A


def x_of(L, x):
    """the launch's input from the vector x: SpMM's X holds x and -x in alternating columns"""
    return x if not L.k else x[:, None] * np.where(np.arange(L.k) % 2 == 0, 1.0, -1.0)[None, :]


def per_column(L, f):
    """f(sign) per column of the launch's output, stacked as the launch returns it"""
    if not L.k:
        return f(1.0)
    cols = {s: f(s) for s in (1.0, -1.0)}
    return np.stack([cols[1.0 if j % 2 == 0 else -1.0] for j in range(L.k)], axis=1)


def poison(bmsp, n, dtype):
    u = bmsp.DeviceArray(n, dtype)
    bmsp.check(bmsp.lib().bmsp_memset(u.ptr, 0xFF, n * u.dtype.itemsize))
    return u


def run(bmsp, L, A, dtype, x, u0=None):
    """the launch on x (host, float64), into a NaN-poisoned u -- or, when beta != 0, over u0; the result on the host"""
    n_out = operand(L.kind, L.op)[0]
    with np.errstate(over="ignore"):
        xd = bmsp.DeviceArray.from_host(np.ascontiguousarray(x_of(L, x), NPDT[dtype]).ravel())
    u = poison(bmsp, n_out * max(1, L.k), OUTDT[dtype])
    if L.api == "spmv":
        bmsp.check(bmsp.lib().bmsp_spmv(A.h, xd.ptr, u.ptr, L.variant, None))
    elif L.api == "spmm":
        bmsp.spmm(A, xd, L.k, u)
    elif L.api == "op":
        if L.beta != 0:
            u = bmsp.DeviceArray.from_host(u0.astype(OUTDT[dtype]))
        bmsp.spmv_op(A, xd, L.op, L.alpha, L.beta, u)
    else:
        comm = bmsp.Comm.loopback(3)
        _, sh = bmsp.spmv_sharded(comm, A, xd, u, variant=L.variant)
        comm.free()
        assert sh["world"] == 3, sh
    out = u.to_host()
    return out.reshape(n_out, L.k) if L.k else out


# ---------------------------------------------------------------------------------------------------------
# 4. CPU self-checks: the reference alone meets the conditions the GPU tests rely on
# ---------------------------------------------------------------------------------------------------------
def _exact_in_any_order(p, o, n_out, dtype):
    """per output: every product is a multiple of one power of two q, and sum |p| < 2^24 q (2^53 q for F64); returns max sum |p| / q"""
    nz = p != 0
    m, e = np.frexp(p[nz].astype(np.float64))          # (products of two stored values hold at most 48 bits: exact in float64)
    assert np.array_equal(np.ldexp(m, e).astype(LD), p[nz])
    M = np.abs(np.ldexp(m, 53)).astype(np.int64)
    low = e - 53 + np.frexp((M & -M).astype(np.float64))[1] - 1   # exponent of the lowest set bit
    q = np.full(n_out, 10 ** 6)
    np.minimum.at(q, o[nz], low)
    mag = np.zeros(n_out, LD)
    np.add.at(mag, o[nz], np.abs(p[nz]))
    rows = np.flatnonzero(q < 10 ** 6)
    ratio = mag[rows] / np.ldexp(LD(1), q[rows])
    assert ratio.max() < 2.0 ** (53 if dtype == 2 else 24), ratio.max()
    return float(ratio.max())


@pytest.mark.parametrize("kind", KINDS + ("full",))
def test_structures_have_their_holes(oracle, kind):
    """D_c and D_r hold no stored entry; every surviving tile of the dense kind has a nibble that is neither 0 nor 0xF; the full kind keeps
    a quarter of its tiles full (what spmv_sweep_kernel<FULL> is chosen by)"""
    nr, nc, r, c = structure(kind)
    assert not np.isin(c, hole_cols(kind, nc)).any() and not np.isin(r, hole_rows(kind, nr)).any()
    assert np.unique(r * nc + c).size == r.size and nr in (1003, 777, 1237)
    M = oracle.bmsp_from_coo(oracle.Coo(nr, nc, r, c, np.ones(r.size)), 0, False)
    bm = M.bmps.astype(np.uint64)
    nib = np.stack([(bm >> np.uint64(4 * q)) & np.uint64(15) for q in range(16)], axis=1)
    partly = ((nib != 0) & (nib != 15)).any(axis=1)
    if kind == "dense":
        assert partly.all() and M.nnz >= 16 * M.block_num
        assert {13, 11} <= set(np.unique(nib).tolist())      # 1101 and 1011
    if kind == "mid":
        assert set(np.unique(nib).tolist()) == {n for n in range(16) if not n & 0b0010 or not n & 0b0100}   # every pattern the holes leave
    if kind == "full":
        assert 4 * int((bm == np.uint64(0xFFFFFFFFFFFFFFFF)).sum()) >= M.block_num and partly.any()
    assert partly.any()


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("kind", KINDS + ("full",))
def test_inputs_are_exact_and_hit_their_classes(kind, op, dtype):
    """Test A's, B's and C's inputs.  With the special values taken out every finite partial sum is exact in any order; test B's outputs fall
    into every class by every cause in at least 16 outputs each and a quarter of them stay finite; in an output with an overflowing product
    every other finite product is below 2^60 and all overflowing products share one sign."""
    n_out, n_in, o, i, D_in, D_out = operand(kind, op)
    assert not np.isin(i, D_in).any() and not np.isin(o, D_out).any()
    x, x0 = poisoned_x(kind, op)
    t, f = reference(n_out, o, i, ints(o, i), x0, dtype)
    assert np.isfinite(t).all()
    _exact_in_any_order(f["products"][0], o, n_out, dtype)
    assert np.array_equal(reference(n_out, o, i, ints(o, i), x, dtype)[0], t)      # the reference itself never sees D_in
    for which in ("values", "x"):
        a, xs, want = subnormal(kind, op, dtype, which)
        assert np.array_equal(rounded(a, dtype), a) and np.array_equal(rounded(xs, dtype), xs)
        small = np.abs(a if which == "values" else xs)
        assert small.max() < np.finfo(NPDT[dtype]).tiny and small.min() > 0      # subnormal in the storage type, not zero
        ts, fs = reference(n_out, o, i, a, xs, dtype)
        assert np.array_equal(ts, want) and np.array_equal(want.astype(OUTDT[dtype]).astype(LD), want)
        _exact_in_any_order(fs["products"][0], o, n_out, dtype)
        if dtype != 1:
            nzw = want[want != 0]
            assert nzw.size and np.abs(nzw).max() < np.finfo(OUTDT[dtype]).tiny     # the results are subnormal too
    a, xb, zeros = planted(kind, op, dtype)
    assert zeros >= 16
    if kind == "full":   # what spmv_sweep_kernel<FULL> and the row-group kernel's fast branch multiply: every kind of special value inside FULL tiles
        nr, nc, r, c = structure(kind)
        _, inv, per_tile = np.unique((r // 8) * nc + c // 8, return_inverse=True, return_counts=True)
        in_full, xi = per_tile[inv] == 64, xb[i]
        large = np.isfinite(a) & (np.abs(a) >= 65504.0)
        for name, m in (("stored NaN", np.isnan(a)), ("stored +Inf", a == INF), ("stored -Inf", a == -INF), ("stored 0 against Inf", (a == 0) & np.isinf(xi)),
                        ("overflowing / 65504^2 product", large), ("+Inf in x", xi == INF), ("-Inf in x", xi == -INF), ("NaN in x", np.isnan(xi))):
            assert int((m & in_full).sum()) >= 16, (op, dtype, name, int((m & in_full).sum()))
    t, f = reference(n_out, o, i, a, xb, dtype)
    p, fin = f["products"]
    _exact_in_any_order(np.where(fin, p, 0), o, n_out, dtype)
    assert np.array_equal(expected(t, 1.0, 0.0, None, dtype).astype(LD)[~np.isnan(t)], t[~np.isnan(t)])   # every value is one of the output type
    count = lambda m: int(np.asarray(m).sum())
    nan, finite = np.isnan(t), np.isfinite(t)
    assert count(finite) * 4 >= n_out, count(finite)
    classes = {"finite, non-zero": finite & (t != 0),
               "NaN from a stored NaN": f["stored_nan"] & ~f["zero_inf"],
               "NaN from a NaN in x": f["nan_operand"] & ~f["stored_nan"],
               "NaN from 0 * Inf": f["zero_inf"] & ~f["nan_operand"],
               "NaN from +Inf and -Inf": nan & ~f["nan_product"],
               "+Inf": t == INF, "-Inf": t == -INF,
               "+Inf from a stored Inf or an Inf in x": (t == INF) & ~f["big_pos"], "-Inf from a stored Inf or an Inf in x": (t == -INF) & ~f["big_neg"]}
    if dtype != 1:
        classes["overflow to +Inf"] = (t == INF) & f["big_pos"] & ~f["inf_pos"]
        classes["overflow to -Inf"] = (t == -INF) & f["big_neg"] & ~f["inf_neg"]
        assert not (f["big_pos"] & f["big_neg"]).any()
        assert f["other_below_2_60"][f["big_pos"] | f["big_neg"]].all()
        assert not ((f["big_pos"] | f["big_neg"]) & (f["inf_pos"] | f["inf_neg"] | f["nan_product"])).any()   # (fused or not: the same class)
    else:
        assert not (f["big_pos"] | f["big_neg"]).any()
        classes["65504^2 and more, positive"] = finite & (t >= 65504.0 ** 2)
        classes["65504^2 and more, negative"] = finite & (t <= -65504.0 ** 2)
    for name, m in classes.items():
        assert count(m) >= 16, (kind, op, dtype, name, count(m))


def _padded_product(kind, x, granule):
    """an emulation that multiplies MORE than the stored values: every position of each stored tile ("tile": the reference project's
    sweep) or of each nibble that holds a stored value ("nibble": spmv_rowgroup_kernel before this file existed), unstored ones as 0"""
    nr, nc, r, c = structure(kind)
    if granule == "tile":
        g = np.unique((r // 8) * nc + c // 8)
        pr = np.repeat((g // nc) * 8, 64) + np.tile(np.repeat(np.arange(8), 8), g.size)
        pc = np.repeat((g % nc) * 8, 64) + np.tile(np.tile(np.arange(8), 8), g.size)
    else:
        g = np.unique(r * nc + (c // 4))
        pr = np.repeat(g // nc, 4)
        pc = np.repeat((g % nc) * 4, 4) + np.tile(np.arange(4), g.size)
    ok = (pr < nr) & (pc < nc)
    key = np.unique(pr[ok] * nc + pc[ok])
    pr, pc = key // nc, key % nc
    vals = np.zeros(key.size)
    vals[np.searchsorted(key, r * nc + c)] = ints(r, c)
    out = np.zeros(nr)
    with np.errstate(invalid="ignore"):
        np.add.at(out, pr, vals * x[pc])
    return out


@pytest.mark.parametrize("granule", ["tile", "nibble"])
@pytest.mark.parametrize("kind", ["dense", "mid"])
def test_padded_multiplies_fail_test_a(oracle, kind, granule):
    """Test A sees a kernel that multiplies unstored positions, without taking the code under test as the measure: a whole-tile multiply
    (for fp32 the oracle's own sweep) and a per-nibble multiply give NaN in at least 16 rows and fail check_a; the same emulations of the
    zeroed x pass it."""
    nr, nc, r, c = structure(kind)
    x, x0 = poisoned_x(kind, "N")
    want0 = util.scipy_csr(nr, nc, r, c, ints(r, c)) @ x0
    zero_rows = np.flatnonzero(np.bincount(r, minlength=nr) == 0)
    out0 = _padded_product(kind, x0, granule).astype(np.float32)
    check_a(out0, out0, want0, zero_rows)
    outs = [_padded_product(kind, x, granule).astype(np.float32)]
    if granule == "tile":
        ref = oracle.bmsp_from_coo(oracle.Coo(nr, nc, r, c, ints(r, c)), 0, False)
        outs.append(np.asarray(oracle.spmv_f32(ref, x.astype(np.float32)), np.float32))
        np.testing.assert_array_equal(np.isnan(outs[0]), np.isnan(outs[1]))
    for out in outs:
        assert np.isnan(out).sum() >= 16
        with pytest.raises(AssertionError):
            check_a(out, out0, want0, zero_rows)


# ---------------------------------------------------------------------------------------------------------
# 5. the GPU tests
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("launch,dtype", PARAMS)
def test_a_unstored_positions_add_nothing(bmsp, monkeypatch, launch, dtype):
    """x = +Inf, -Inf, NaN at every input index no entry has, next to stored columns inside every tile: no output is Inf or NaN, the result
    equals the same launch on x with zeros there bit for bit, that one equals the exact product, and the outputs without stored entries
    are +0 over a NaN-poisoned u."""
    L = LAUNCHES[launch]
    n_out, n_in, o, i, _, _ = operand(L.kind, L.op)
    a = ints(o, i)
    A = make_matrix(bmsp, monkeypatch, L, dtype, a)
    x, x0 = poisoned_x(L.kind, L.op)
    u0 = u0_for(n_out)
    out, out0 = (run(bmsp, L, A, dtype, xs, u0) for xs in (x, x0))
    t0 = cached(("a_ref", L.kind, L.op, dtype), lambda: reference(n_out, o, i, a, x0, dtype)[0])
    want0 = per_column(L, lambda s: expected(s * t0, L.alpha, L.beta, u0, dtype).astype(np.float64))
    check_a(out, out0, want0, np.flatnonzero(np.bincount(o, minlength=n_out) == 0) if L.beta == 0 else None)


@pytest.mark.gpu
@pytest.mark.parametrize("launch,dtype", PARAMS)
def test_b_stored_special_values_give_the_ieee_class(bmsp, monkeypatch, launch, dtype):
    """stored NaN, +-Inf and zeros, +-Inf and NaN in x at stored columns, products that overflow: the class and the value of every output
    against `reference`."""
    L = LAUNCHES[launch]
    n_out, n_in, o, i, _, _ = operand(L.kind, L.op)
    a, x, zeros = planted(L.kind, L.op, dtype)
    A = make_matrix(bmsp, monkeypatch, L, dtype, a)
    stored = A.host_arrays()[3]
    assert int((stored == 0).sum()) == zeros and int(np.isnan(stored).sum()) == int(np.isnan(a).sum())    # the zeros and NaNs ARE stored
    u0 = u0_for(n_out)
    out = run(bmsp, L, A, dtype, x, u0)
    ref = cached(("b_ref", L.kind, L.op, dtype), lambda: {s: reference(n_out, o, i, a, s * x, dtype)[0] for s in (1.0, -1.0)})
    assert_class_and_value(out, per_column(L, lambda s: expected(ref[s], L.alpha, L.beta, u0, dtype)), launch)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["values", "x"])
@pytest.mark.parametrize("launch,dtype", PARAMS)
def test_c_subnormals_are_kept(bmsp, monkeypatch, launch, dtype, which):
    """subnormal stored values against small integers, and small integers against a subnormal x (F16: subnormal in fp16 -- the widening
    must not flush them): every sum is an exact multiple of the smallest subnormal in any order.  (beta != 0 launches run over u = 0.)"""
    L = LAUNCHES[launch]
    n_out = operand(L.kind, L.op)[0]
    a, x, t = subnormal(L.kind, L.op, dtype, which)
    A = make_matrix(bmsp, monkeypatch, L, dtype, a)
    assert np.count_nonzero(A.host_arrays()[3]) == a.size      # the builder kept them
    u0 = np.zeros(n_out)
    out = run(bmsp, L, A, dtype, x, u0)
    want = per_column(L, lambda s: expected(s * t, L.alpha, L.beta, u0, dtype))
    assert_class_and_value(out, want, launch)


@pytest.mark.gpu
@pytest.mark.parametrize("launch,dtype", SPMV_PARAMS)
def test_d_element_alignment_suffices(bmsp, monkeypatch, launch, dtype):
    """bmsp.h asks for device pointers and nothing more: v one element into a NaN-filled allocation (NaN behind its end too), u one element
    into a 0xFF-filled one, test A's inputs: the same bits as the aligned run, the elements before and after u untouched."""
    L = LAUNCHES[launch]
    n_out, n_in, o, i, _, _ = operand(L.kind, L.op)
    A = make_matrix(bmsp, monkeypatch, L, dtype, ints(o, i))
    x, _ = poisoned_x(L.kind, L.op)
    aligned = run(bmsp, L, A, dtype, x)
    assert np.isfinite(aligned).all()
    host = np.full(n_in + 2, NAN, NPDT[dtype])
    host[1:n_in + 1] = x.astype(NPDT[dtype])
    xd = bmsp.DeviceArray.from_host(host)
    u = poison(bmsp, n_out + 2, OUTDT[dtype])
    es, os_ = xd.dtype.itemsize, u.dtype.itemsize
    bmsp.check(bmsp.lib().bmsp_spmv(A.h, xd.ptr + es, u.ptr + os_, L.variant, None))
    got = u.to_host()
    np.testing.assert_array_equal(bits(got[1:-1]), bits(aligned))
    guard = got.view(np.uint8)
    assert (guard[:os_] == 0xFF).all() and (guard[-os_:] == 0xFF).all(), "the neighbours of u were written"
