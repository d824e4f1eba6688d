"""GPU tests of bmsp_sddmm / bmsp_sddmm_values / bmsp_sddmm_launch_info: C = alpha * (X . Y^T) on the pattern of S + beta * S, or * S.

Expected values come from numpy on the host.

1. Integer operands (X, Y in [-3, 3], s in [-4, 4]): every partial sum and every result is exactly representable (the host self-check
   in test_sddmm_api.py asserts it for the very arrays used here), so any summation order, the matrix cores' included, is exact: the
   four arrays equal those of from_coo of the numpy result, and the two kernels agree in every bit.
2. Real operands with magnitudes in [0.5, 2): let d64 be the dot product of the (storage-rounded) operands in float64 and
   A = sum_t |x_t * y_t|.  A sum of k exactly formed products added in ANY order with round-to-nearest additions obeys
   |d - d64| <= gamma_(k-1) * A < k * u * A, u = 2^-24 (2^-53 for F64) (Higham, Accuracy and Stability, (3.5): each product takes part in
   at most k - 1 additions; the fused multiply-adds of the vector kernel round once per term, which the same bound covers, fp16 products
   being exact in fp32).  The bound used is 2 * k * u * A: doubled, because the rounding of the matrix core's internal group additions is
   not documented as round-to-nearest.  The epilogue c = fl(fl(alpha * d) + fl(beta * s)) then adds one rounding per operation:
       |c - (alpha * d64 + beta * s)| <= |alpha| * E + 3 * u * (|alpha| * (|d64| + E) + |beta * s|),   E = 2 * k * u * A
   (u for the product, u for beta * s, u for the sum, each of a quantity bounded by the bracket; second-order terms are covered by the
   third u of the product term).  An fp16 output is rounded once more: + max(2^-11 * |c32|, 2^-25), the second term being half the
   spacing of the fp16 subnormals (|c32| is bounded by the reference plus the fp32 bound).
3. The epilogue bit for bit: integer X and Y make d exact, alpha, beta and s are real; c equals numpy arithmetic in the arithmetic type,
   operation by operation, for both forms; with beta = 0 a NaN stored in S does not propagate; an fp16 result beyond 65504 is Inf.
4. Life cycle: in place, into a with_layout copy, a scale output and an earlier sddmm output; refusals; S unchanged; value caches
   dropped; a stream; determinism.
5. launch_info: kernel name and lanes follow the switches and the default rule, compulsory_bytes equals a numpy restatement."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from stream_gate import _hip
from test_transpose import snapshot, assert_unchanged, assert_same_arrays, entries

pytestmark = pytest.mark.gpu

NPDT = {0: np.float32, 1: np.float16, 2: np.float64}
ARITH = {0: np.float32, 1: np.float32, 2: np.float64}
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
EPS = {0: 2.0 ** -24, 1: 2.0 ** -24, 2: 2.0 ** -53}
DNAME = ("f32", "f16", "f64")
NAMES = ("banded", "random", "rmat", "dense", "1x1", "5x3", "3x70", "nnz0", "rows0")
KS = (1, 3, 8, 31, 32, 33, 64, 100)
KMAX = max(KS)
LDKINDS = ("k", "k+3", "pad")
KERNELS = (None, "value", "tile")
LANES = (None, "1", "8")
# (alpha, beta, mul_s) of test 1
EPILOGUES = ((1.0, 0.0, False), (-2.0, 1.0, False), (0.5, -1.0, False), (1.0, 0.0, True), (-0.5, 0.0, True))
FILL_THRESHOLD = 6  # values per tile from which the tile kernel is the default (sddmm.hip, DESIGN section 4 "SDDMM")
RUN = 8             # consecutive tiles one wave of the tile kernel takes

_CACHE = {}


def patterns():
    """{name: (num_rows, num_cols, rows, cols)}: the coordinates only, generated once"""
    if "coo" not in _CACHE:
        from pybmsp import gen
        e = np.zeros(0, np.int32)
        dr, dc = np.divmod(np.arange(16 * 24), 24)
        m = {"banded": gen.banded(133, 12), "random": gen.random_coo(203, 157, 203 * 26, seed=3), "rmat": gen.rmat(10, 8),
             "dense": (16, 24, dr, dc, None), "1x1": (1, 1, np.array([0]), np.array([0]), None), "5x3": gen.random_coo(5, 3, 9, seed=6),
             "3x70": gen.random_coo(3, 70, 60, seed=7), "nnz0": (37, 11, e, e, None), "rows0": (0, 13, e, e, None)}
        _CACHE["coo"] = {k: (x[0], x[1], np.asarray(x[2], np.int64), np.asarray(x[3], np.int64)) for k, x in m.items()}
    return _CACHE["coo"]


def ld_of(k, kind):
    return {"k": k, "k+3": k + 3, "pad": 8 * ((k + 7) // 8) + 8}[kind]


def int_operands(name):
    """integer X (num_rows x KMAX) and Y (num_cols x KMAX) in [-3, 3] and s in [-4, 4] per stored coordinate, fixed per pattern; a case
    of k columns uses the first k"""
    key = ("int", name)
    if key not in _CACHE:
        nr, nc, r, c = patterns()[name]
        rng = np.random.default_rng(300 + NAMES.index(name))
        _CACHE[key] = (rng.integers(-3, 4, (nr, KMAX)), rng.integers(-3, 4, (nc, KMAX)), rng.integers(-4, 5, r.size))
    return _CACHE[key]


def int_dots(name, k):
    """(d, sum |x y|) per stored coordinate in int64"""
    key = ("int_dot", name, k)
    if key not in _CACHE:
        nr, nc, r, c = patterns()[name]
        X, Y, _ = int_operands(name)
        p = X[r, :k] * Y[c, :k]
        _CACHE[key] = (p.sum(axis=1), np.abs(p).sum(axis=1))
    return _CACHE[key]


def int_result(name, k, alpha, beta, mul_s):
    """the result of test 1 per stored coordinate in float64 (exact: see the self-check)"""
    d = int_dots(name, k)[0].astype(np.float64)
    s = int_operands(name)[2].astype(np.float64)
    return alpha * d * s if mul_s else alpha * d + beta * s


def int_cases():
    """test 1: every pattern x dtype x k twice; layouts, leading dimension, switches and epilogue drawn per case from a fixed stream
    (test_sddmm_api.py asserts that every value of every parameter, and every kernel switch with every dtype and leading dimension,
    occurs)"""
    if "int_cases" not in _CACHE:
        rng = np.random.default_rng(20240)
        out = []
        for name in NAMES:
            for dtype in (0, 1, 2):
                for k in KS:
                    for rep in range(2):
                        out.append((name, dtype, k, int(rng.integers(2)), int(rng.integers(2)), LDKINDS[rng.integers(3)],
                                    LDKINDS[rng.integers(3)], KERNELS[rng.integers(3)], LANES[rng.integers(3)], int(rng.integers(len(EPILOGUES)))))
        _CACHE["int_cases"] = out
    return _CACHE["int_cases"]


def case_id(c):
    return "%s-%s-k%d-s%d-o%d-ldx_%s-ldy_%s-%s-lanes%s-e%d" % (c[0], DNAME[c[1]], c[2], c[3], c[4], c[5], c[6], c[7] or "dflt", c[8] or "dflt", c[9])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def assert_exact(got, want, msg=""):
    """equal as values everywhere, bit for bit wherever the result is not zero: the sign of a zero result is the summation order's
    (x + (-x) = +0, a lone product 0 * (-3) is -0) even when every operation is exact"""
    assert got.dtype == want.dtype and got.shape == want.shape, msg
    np.testing.assert_array_equal(got, want, err_msg=msg)
    nz = want != 0
    np.testing.assert_array_equal(bits(got)[nz], bits(want)[nz], err_msg=msg)


def set_switches(monkeypatch, kernel, lanes):
    for var, val in (("BMSP_SDDMM_KERNEL", kernel), ("BMSP_SDDMM_LANES", lanes)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)


def build(bmsp, name, vals, lay, dtype):
    nr, nc, r, c = patterns()[name]
    return bmsp.BmSpMatrix.from_coo(nr, nc, r, c, vals, transposed=lay, dtype=dtype)


def source(bmsp, name, dtype, lay):
    """S of test 1 (integer values), built once per (pattern, dtype, layout): the out-of-place calls never modify it"""
    key = ("S", name, dtype, lay)
    if key not in _CACHE:
        _CACHE[key] = build(bmsp, name, int_operands(name)[2].astype(np.float64), lay, dtype)
    return _CACHE[key]


def padded(bmsp, M, k, ld, dtype):
    """rows of M[:, :k] at leading dimension ld on the device, the padding columns filled with NaN"""
    h = np.full((M.shape[0], ld), np.nan, NPDT[dtype])
    h[:, :k] = M[:, :k]
    return bmsp.DeviceArray.from_host(h.ravel(), NPDT[dtype])


def expected_info(S, k, ldx, ldy, kernel, lanes):
    """numpy restatement of the launcher's rule and of the counting rule of compulsory_bytes"""
    i = S.info()
    nnz, nb, es = i["nnz"], i["block_num"], np.dtype(NPDT[i["dtype"]]).itemsize
    if nb == 0 or nnz == 0:
        return {"kernel": "none (empty matrix)", "lanes": 0, "compulsory_bytes": 0}
    can_tile = i["dtype"] != 2 and (ldx * es) % 16 == 0 and (ldy * es) % 16 == 0
    tile = can_tile and nnz >= FILL_THRESHOLD * nb
    if kernel == "value":
        tile = False
    elif kernel == "tile":
        tile = can_tile
    keys, bmps, offs, _ = S.host_arrays()
    if tile:
        g, name = 0, "sddmm_tile_kernel"
        brow, bcol = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
        xr = np.minimum(8, i["num_rows"] - 8 * brow).sum()
        yr = np.minimum(8, i["num_cols"] - 8 * bcol).sum()
    else:
        g = int(lanes) if lanes else (1 if nnz < 6 * nb else 8)
        name = "sddmm_value_kernel<%d>" % g
        r, c, _ = entries(keys, bmps, offs, i["transposed"])
        tile_of = np.repeat(np.arange(nb), np.diff(offs.astype(np.int64)))
        xr = np.unique(tile_of * (1 << 32) + r).size  # (tile, row) pairs that hold a value
        yr = np.unique(tile_of * (1 << 32) + c).size
    return {"kernel": name, "lanes": g, "compulsory_bytes": int(24 * nb + 2 * nnz * es + (xr + yr) * k * es)}


# ---------------------------------------------------------------------------------------------------------
# 0. the patterns reach the branches they are there for (host only, but the cases below depend on it)
# ---------------------------------------------------------------------------------------------------------
def test_the_patterns_are_what_the_cases_need():
    m = patterns()
    per_row = {}
    for name in ("banded", "rmat", "random"):
        nr, nc, r, c = m[name]
        tiles = np.unique((r // 8) << 32 | (c // 8))
        per_row[name] = np.bincount(tiles >> 32)
        fill = r.size / tiles.size
        assert (fill >= FILL_THRESHOLD) == (name != "rmat"), (name, fill)  # dense tiles / hyper-sparse tiles
    assert per_row["rmat"].max() > RUN, per_row["rmat"].max()  # a hub block-row longer than one wave's run of tiles
    nr, nc, r, c = m["banded"]
    assert nr % 8 and nc % 8  # ragged last block-row and block-column
    starts = np.concatenate([[0], np.cumsum(per_row["banded"])])
    assert np.any(starts[1:-1] % 2 == 1)  # a pair of tiles straddles two block-rows
    assert any(np.unique((x[2] // 8) << 32 | (x[3] // 8)).size % 2 for x in m.values() if x[2].size)  # an odd last tile


# ---------------------------------------------------------------------------------------------------------
# 1. integer operands, bit for bit
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", int_cases(), ids=case_id)
def test_integer_operands_exact(bmsp, monkeypatch, case):
    name, dtype, k, s_lay, o_lay, ldxk, ldyk, kernel, lanes, e = case
    alpha, beta, mul_s = EPILOGUES[e]
    nr, nc, r, c = patterns()[name]
    Xi, Yi, _ = int_operands(name)
    ldx, ldy = ld_of(k, ldxk), ld_of(k, ldyk)
    S = source(bmsp, name, dtype, s_lay)
    snap = snapshot(S)
    X, Y = padded(bmsp, Xi, k, ldx, dtype), padded(bmsp, Yi, k, ldy, dtype)
    want = bmsp.BmSpMatrix.from_coo(nr, nc, r, c, int_result(name, k, alpha, beta, mul_s), transposed=o_lay, dtype=dtype)
    wk, wb, wo, wv = want.host_arrays()

    set_switches(monkeypatch, kernel, lanes)
    info = bmsp.sddmm_launch_info(S, k, ldx, ldy, o_lay)
    assert info == expected_info(S, k, ldx, ldy, kernel, lanes), (info, expected_info(S, k, ldx, ldy, kernel, lanes))
    es = np.dtype(NPDT[dtype]).itemsize
    if (dtype == 2 or (ldx * es) % 16 or (ldy * es) % 16) and r.size:
        assert info["kernel"].startswith("sddmm_value_kernel"), info  # the fallback, also when `tile` is forced
    Cm = bmsp.sddmm(S, X, Y, k, alpha, beta, mul_s, transposed=o_lay, ldx=ldx, ldy=ldy)
    assert Cm.info() == want.info()
    gk, gb, go, gv = Cm.host_arrays()
    for g, w in ((gk, wk), (gb, wb), (go, wo)):
        np.testing.assert_array_equal(g, w)
    assert_exact(gv, wv, case_id(case))
    np.testing.assert_array_equal(Cm.block_row_ptr(), want.block_row_ptr())
    assert_unchanged(S, snap)

    # the two kernels agree in every bit, with each other and with the call above (where the tile kernel cannot run, all three are
    # the value kernel)
    for kern in ("value", "tile"):
        set_switches(monkeypatch, kern, lanes)
        other = bmsp.sddmm(S, X, Y, k, alpha, beta, mul_s, transposed=o_lay, ldx=ldx, ldy=ldy).host_arrays()[3]
        np.testing.assert_array_equal(bits(other), bits(gv), err_msg=kern)


# ---------------------------------------------------------------------------------------------------------
# 2. real operands, derived bound
# ---------------------------------------------------------------------------------------------------------
REAL_NAMES = ("banded", "random", "rmat", "dense", "5x3")


def real_operands(name, dtype):
    """X, Y, s with magnitudes in [0.5, 2) and mixed signs, rounded to the storage type (so the float64 reference sees what the
    device sees)"""
    key = ("real", name, dtype)
    if key not in _CACHE:
        nr, nc, r, c = patterns()[name]
        rng = np.random.default_rng(500 + 10 * NAMES.index(name) + dtype)
        draw = lambda shape: (rng.uniform(0.5, 2.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(NPDT[dtype]).astype(np.float64)
        _CACHE[key] = (draw((nr, KMAX)), draw((nc, KMAX)), draw(r.size))
    return _CACHE[key]


def real_cases():
    rng = np.random.default_rng(777)
    return [(name, dtype, k, int(rng.integers(2)), int(rng.integers(2)), ("k", "pad")[rng.integers(2)], LANES[rng.integers(3)])
            for name in REAL_NAMES for dtype in (0, 1, 2) for k in KS]


@pytest.mark.parametrize("case", real_cases(), ids=lambda c: "%s-%s-k%d-s%d-o%d-ld_%s-lanes%s" % (c[0], DNAME[c[1]], c[2], c[3], c[4], c[5], c[6] or "dflt"))
def test_real_operands_within_the_derived_bound(bmsp, monkeypatch, case):
    name, dtype, k, s_lay, o_lay, ldk, lanes = case
    alpha, beta = 1.25, -0.75
    nr, nc, r, c = patterns()[name]
    Xr, Yr, s = real_operands(name, dtype)
    ld = ld_of(k, ldk)
    S = build(bmsp, name, s, s_lay, dtype)
    X, Y = padded(bmsp, Xr, k, ld, dtype), padded(bmsp, Yr, k, ld, dtype)
    p = Xr[r, :k] * Yr[c, :k]
    d64, A = p.sum(axis=1), np.abs(p).sum(axis=1)
    u = EPS[dtype]
    E = 2 * k * u * A
    ref = alpha * d64 + beta * s
    bound = abs(alpha) * E + 3 * u * (abs(alpha) * (np.abs(d64) + E) + np.abs(beta * s))
    if dtype == 1:
        bound = bound + np.maximum(2.0 ** -11 * (np.abs(ref) + bound), 2.0 ** -25)
    order = np.lexsort((c, r))  # to_coo's order
    for kern in ("value", "tile"):
        set_switches(monkeypatch, kern, lanes)
        Cm = bmsp.sddmm(S, X, Y, k, alpha, beta, transposed=o_lay, ldx=ld, ldy=ld)
        gr, gc, gv = Cm.to_coo()
        np.testing.assert_array_equal(gr, r[order])
        np.testing.assert_array_equal(gc, c[order])
        err = np.abs(np.asarray(gv, np.float64) - ref[order])
        worst = float(np.max(err / bound[order])) if err.size else 0.0
        print("sddmm real %s %s k=%d %s: worst error / bound = %.3g" % (name, DNAME[dtype], k, kern, worst))
        assert np.all(err <= bound[order]), (kern, worst)


# ---------------------------------------------------------------------------------------------------------
# 3. the epilogue, bit for bit
# ---------------------------------------------------------------------------------------------------------
def epilogue_ref(d, s, alpha, beta, mul_s, dtype):
    """numpy arithmetic in the arithmetic type, one rounding per operation, then one rounding to fp16 for F16"""
    F = ARITH[dtype]
    with np.errstate(all="ignore"):
        t = F(alpha) * d.astype(F)
        if mul_s:
            out = t * s.astype(F)
        elif F(beta) == 0:
            out = t
        else:
            out = t + F(beta) * s.astype(F)
        return out.astype(NPDT[dtype])


@pytest.mark.parametrize("kernel", ["value", "tile"])
@pytest.mark.parametrize("form", ["add", "mul", "alpha_only"])
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", ["random", "banded"])
def test_epilogue_bit_for_bit(bmsp, monkeypatch, name, dtype, form, kernel):
    k = 33
    nr, nc, r, c = patterns()[name]
    Xi, Yi, _ = int_operands(name)
    rng = np.random.default_rng(900 + dtype)
    s = (rng.uniform(0.5, 2.0, r.size) * rng.choice([-1.0, 1.0], r.size)).astype(NPDT[dtype])
    alpha, beta, mul_s = {"add": (0.7, -1.3, False), "mul": (-1.1, 0.0, True), "alpha_only": (1.0 / 3.0, 0.0, False)}[form]
    d = int_dots(name, k)[0]
    set_switches(monkeypatch, kernel, None)
    for s_lay, o_lay in ((0, 0), (1, 0), (0, 1)):
        sv = s.astype(np.float64).copy()
        if form == "alpha_only":
            sv[::3] = np.nan  # beta == 0: s is not read
        S = build(bmsp, name, sv, s_lay, dtype)
        X, Y = padded(bmsp, Xi, k, 40, dtype), padded(bmsp, Yi, k, 40, dtype)
        Cm = bmsp.sddmm(S, X, Y, k, alpha, beta, mul_s, transposed=o_lay, ldx=40, ldy=40)
        gr, gc, gv = Cm.to_coo()  # sorted by (row, col); the storage values widened exactly
        order = np.lexsort((c, r))
        np.testing.assert_array_equal(gr, r[order])
        np.testing.assert_array_equal(gc, c[order])
        exp = epilogue_ref(d[order], s[order], alpha, beta, mul_s, dtype)
        assert not np.any(np.isnan(gv))
        np.testing.assert_array_equal(bits(np.asarray(gv).astype(NPDT[dtype])), bits(exp))


@pytest.mark.parametrize("kernel", ["value", "tile"])
def test_fp16_overflow_is_inf(bmsp, monkeypatch, kernel):
    name, k = "dense", 64
    nr, nc, r, c = patterns()[name]
    Xi, Yi, sv = int_operands(name)
    d = int_dots(name, k)[0]
    set_switches(monkeypatch, kernel, None)
    S = build(bmsp, name, sv.astype(np.float64), 0, 1)
    Cm = bmsp.sddmm(S, padded(bmsp, Xi, k, k, 1), padded(bmsp, Yi, k, k, 1), k, 3000.0, 1.0)
    exp = epilogue_ref(d, sv, 3000.0, 1.0, False, 1)
    assert np.isinf(exp).sum() > 10 and np.isfinite(exp).sum() > 10
    kk, bb, oo, gv = Cm.host_arrays()
    er, ec, idx = entries(kk, bb, oo, 0)
    np.testing.assert_array_equal(bits(gv[idx]), bits(exp[er * nc + ec]))  # (dense: coordinate (r, c) is entry r * nc + c)


# ---------------------------------------------------------------------------------------------------------
# 4. life cycle
# ---------------------------------------------------------------------------------------------------------
def refused(bmsp, fn, word):
    with pytest.raises(bmsp.BmspError) as e:
        fn()
    assert e.value.status == -1 and word in str(e.value), str(e.value)


@pytest.mark.parametrize("kernel", [None, "value", "tile"])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_values_into_existing_matrices(bmsp, monkeypatch, dtype, kernel):
    name, k = "random", 32
    nr, nc, r, c = patterns()[name]
    Xi, Yi, sv = int_operands(name)
    X, Y = padded(bmsp, Xi, k, k, dtype), padded(bmsp, Yi, k, k, dtype)
    set_switches(monkeypatch, kernel, None)
    for lay in (0, 1):
        S = build(bmsp, name, sv.astype(np.float64), lay, dtype)
        snap = snapshot(S)
        ref = {(e, lo): bmsp.BmSpMatrix.from_coo(nr, nc, r, c, int_result(name, k, *EPILOGUES[e]), transposed=lo, dtype=dtype)
               for e in (1, 2, 4) for lo in (0, 1)}

        def same(M, e):
            a, b = M.host_arrays(), ref[(e, M.info()["transposed"])].host_arrays()
            for x, y in zip(a[:3], b[:3]):
                np.testing.assert_array_equal(x, y)
            assert_exact(a[3], b[3])

        first = bmsp.sddmm(S, X, Y, k, *EPILOGUES[1], transposed=1 - lay)
        same(first, 1)
        outs = [S.with_layout(1 - lay), S.with_layout(lay), bmsp.scale(S, transposed=1 - lay), first]
        for M in outs:
            for e in (2, 4):
                assert bmsp.sddmm_values(M, S, X, Y, k, *EPILOGUES[e]) is M
                same(M, e)
        assert_unchanged(S, snap)
        # what sddmm made is accepted by its siblings
        bmsp.scale_values(first, S)
        first.copy_values_from(S)
        assert_same_arrays(first, S.with_layout(1 - lay))
        # refusals: an unrelated handle, a transpose output
        other = build(bmsp, name, sv.astype(np.float64), lay, dtype)
        refused(bmsp, lambda: bmsp.sddmm_values(other, S, X, Y, k), "out")
        if nr != nc:
            refused(bmsp, lambda: bmsp.sddmm_values(S.transpose(lay), S, X, Y, k), "out")
        assert_unchanged(S, snap)
        # in place
        assert S.sddmm_(X, Y, k, *EPILOGUES[2]) is S
        same(S, 2)
        # after invalidate(S, 1) every earlier output is refused; in place needs no history
        S.invalidate(True)
        for M in outs:
            refused(bmsp, lambda: bmsp.sddmm_values(M, S, X, Y, k), "out")
        S.sddmm_(X, Y, k, 1.0, 0.0)
        np.testing.assert_array_equal(S.to_coo()[2], int_dots(name, k)[0][np.lexsort((c, r))].astype(np.float64))


def test_square_transpose_output_is_refused(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(8, 4)
    S = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    X = bmsp.DeviceArray.from_host(np.ones(n * 8, np.float32))
    refused(bmsp, lambda: bmsp.sddmm_values(S.transpose(0), S, X, X, 8), "out")
    refused(bmsp, lambda: bmsp.sddmm_values(S.transpose(1), S, X, X, 8), "out")


@pytest.mark.parametrize("dtype", [0, 1])
def test_in_place_drops_the_value_caches(bmsp, dtype):
    """after prepare(SPGEMM) and an in-place sddmm_, the next product equals that of a freshly built matrix with the same values"""
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(10, 8)
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    k = 8
    rng = np.random.default_rng(31)
    Xi, Yi = rng.integers(-3, 4, (n, k)), rng.integers(-3, 4, (n, k))
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, dtype=dtype)
    B = A.with_layout(1)
    A.prepare(3)
    bmsp.spgemm(A, B, tc_version=5)
    A.sddmm_(bmsp.DeviceArray.from_host(Xi.ravel(), NPDT[dtype]), bmsp.DeviceArray.from_host(Yi.ravel(), NPDT[dtype]), k, 0.5)
    fresh = bmsp.BmSpMatrix.from_coo(n, n, r, c, 0.5 * (Xi[r] * Yi[c]).sum(axis=1), dtype=dtype)
    assert_same_arrays(A, fresh)
    P, _ = bmsp.spgemm(A, B, tc_version=5)
    Pf, _ = bmsp.spgemm(fresh, B, tc_version=5)
    assert_same_arrays(P, Pf)


@pytest.mark.parametrize("kernel", ["value", "tile"])
def test_non_default_stream_and_determinism(bmsp, monkeypatch, kernel):
    name, k, dtype = "banded", 100, 0
    Xr, Yr, s = real_operands(name, dtype)
    S = build(bmsp, name, s, 0, dtype)
    X, Y = padded(bmsp, Xr, k, 104, dtype), padded(bmsp, Yr, k, 104, dtype)
    set_switches(monkeypatch, kernel, None)
    H = _hip()
    st = C.c_void_p()
    assert H.hipStreamCreate(C.byref(st)) == 0
    try:
        C0 = bmsp.sddmm(S, X, Y, k, 1.5, 0.25, transposed=1, ldx=104, ldy=104, stream=st.value)
        W = S.with_layout(0)
        bmsp.sddmm_values(W, S, X, Y, k, 1.5, 0.25, ldx=104, ldy=104, stream=st.value)
        assert H.hipStreamSynchronize(st) == 0
    finally:
        H.hipStreamDestroy(st)
    C1 = bmsp.sddmm(S, X, Y, k, 1.5, 0.25, transposed=1, ldx=104, ldy=104)
    assert_same_arrays(C0, C1)  # two identical calls, identical bits
    assert_same_arrays(W, bmsp.sddmm(S, X, Y, k, 1.5, 0.25, transposed=0, ldx=104, ldy=104))


def test_refusals_with_a_real_handle(bmsp):
    S = build(bmsp, "5x3", np.ones(patterns()["5x3"][2].size), 0, 0)
    X = bmsp.DeviceArray.from_host(np.ones(5 * 4, np.float32))
    Y = bmsp.DeviceArray.from_host(np.ones(3 * 4, np.float32))
    L = bmsp.lib()
    msg = lambda: L.bmsp_last_error().decode()
    h = C.c_void_p()
    info = bmsp.SddmmInfo()
    assert L.bmsp_sddmm(S.h, None, 4, Y.ptr, 4, 4, 1.0, 0.0, 0, 0, None, C.byref(h)) == -1 and "d_X" in msg() and "null" in msg()
    assert L.bmsp_sddmm(S.h, X.ptr, 4, None, 4, 4, 1.0, 0.0, 0, 0, None, C.byref(h)) == -1 and "d_Y" in msg() and "null" in msg()
    assert L.bmsp_sddmm(S.h, X.ptr, 4, Y.ptr, 4, 4, 1.0, 0.0, 0, 0, None, None) == -1 and "out" in msg() and "null" in msg()
    assert L.bmsp_sddmm_values(S.h, X.ptr, 4, Y.ptr, 4, 4, 1.0, 0.0, 0, None, None) == -1 and "out" in msg() and "null" in msg()
    assert L.bmsp_sddmm_launch_info(S.h, 4, 4, 4, 0, None) == -1 and "info" in msg() and "null" in msg()
    assert L.bmsp_sddmm(S.h, X.ptr, 3, Y.ptr, 4, 4, 1.0, 0.0, 0, 0, None, C.byref(h)) == -1 and "ldx" in msg()
    assert L.bmsp_sddmm_values(S.h, X.ptr, 4, Y.ptr, 4, 4, 1.0, 1.0, 1, S.h, None) == -1 and "beta" in msg()
    assert L.bmsp_sddmm_launch_info(S.h, 0, 4, 4, 0, C.byref(info)) == -1 and "k" in msg()
    panel = S.row_panel(0, 1)
    assert L.bmsp_sddmm_values(panel.h, X.ptr, 4, Y.ptr, 4, 4, 1.0, 0.0, 0, panel.h, None) == -1 and "view" in msg()
    for bad in (bmsp.DeviceArray.from_host(np.ones(5 * 4, np.float64)), bmsp.DeviceArray.from_host(np.ones(5 * 4 - 1, np.float32))):
        with pytest.raises(ValueError):
            bmsp.sddmm(S, bad, Y, 4)
    with pytest.raises(ValueError):
        bmsp.sddmm(S, X, bmsp.DeviceArray.from_host(np.ones(2 * 4, np.float32)), 4)


# ---------------------------------------------------------------------------------------------------------
# 5. launch_info on every pattern under the default rule and the switches
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_launch_info_follows_the_rule(bmsp, monkeypatch, name, dtype):
    S = source(bmsp, name, dtype, 0)
    St = source(bmsp, name, dtype, 1)
    for kernel in KERNELS:
        for lanes in LANES:
            set_switches(monkeypatch, kernel, lanes)
            for M in (S, St):
                for k, ld in ((32, 32), (8, 24), (33, 36), (5, 5)):
                    assert bmsp.sddmm_launch_info(M, k, ld, ld) == expected_info(M, k, ld, ld, kernel, lanes), (name, kernel, lanes, k, ld)
    set_switches(monkeypatch, None, None)
    i = S.info()
    if i["nnz"]:
        dflt = bmsp.sddmm_launch_info(S, 32)
        dense_tiles = i["nnz"] >= FILL_THRESHOLD * i["block_num"]
        assert (dflt["kernel"] == "sddmm_tile_kernel") == (dense_tiles and dtype != 2), dflt
        assert dflt["lanes"] == (0 if dflt["kernel"] == "sddmm_tile_kernel" else (8 if dense_tiles else 1))


def test_cpp_wrapper_runs(tmp_path):
    """tests/cpp_sddmm_check.cpp: bmSparse_sddmm / bmSparse_sddmm_values for float, half and double on the data/real fixture"""
    from conftest import MTX
    from test_sddmm_api import build_cpp_sddmm_check
    exe = str(tmp_path / "cpp_sddmm_check")
    build_cpp_sddmm_check(exe)
    out = subprocess.run([exe, os.path.join(MTX, "real", "A_matrix.mtx")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("OK") == 3 and "FAIL" not in out.stdout, out.stdout
