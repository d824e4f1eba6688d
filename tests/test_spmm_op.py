"""GPU tests of bmsp_spmm_op: Y = alpha * op(A) * X + beta * Y for k vectors, op in {N, T} and both tile layouts.

The matrices are those of tests/test_spmv_op.py (imported: that file asserts they have a hub block-row and a hub block-column, empty
blocks, ragged edges and zero sizes); k is taken from {1, 3, 8, 17, 70}: below, at and across every lane group W and across a 64-column
chunk with a ragged last chunk.  Expected values come from numpy on the host and are cached: integer operands make every summation order
exact (test 1), real operands are held to the any-order bound of test_spmv_op.py's test 2, per element (test 2), the epilogue is checked
bit for bit against numpy arithmetic in the vector type (test 3).  Tests 4 - 8: strides and padding, stored entries only, the life cycle
of the shared view and the scratch, streams, refusals and the C++ wrapper."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from stream_gate import Gate, new_stream, destroy_stream, stream_sync
from test_transpose import snapshot, assert_unchanged, _write_values
from test_add import stored
from test_spmv_op import matrices, NAMES, NPDT, OUTDT, EPS, ALPHA_BETA, SPLIT_NAMES, bits, assert_exact, build

pytestmark = pytest.mark.gpu

KS_ALL = (1, 3, 8, 17, 70)
KS = {"random": KS_ALL, "banded": KS_ALL, "5x3": KS_ALL, "3x70": KS_ALL, "rmat": (3, 17), "sparse_rect": (1, 17), "1x1": (1, 17),
      "nnz0": (1, 17), "rows0": (1, 17)}
KMAX = {n: max(k) for n, k in KS.items()}
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def lengths(name, op):
    nr, nc, _, _ = matrices()[name]
    return (nr, nc) if op else (nc, nr)  # (in_len, out_len)


def int_values(name):
    """integer values in [-4, 4] per stored coordinate and integer X in [-3, 3] (in_len x KMAX) for both ops, fixed per matrix: every
    partial sum is an integer below 2^24 (test_the_matrices_are_what_the_cases_need of test_spmv_op.py)"""
    def make():
        nr, nc, r, c = matrices()[name]
        rng = np.random.default_rng(300 + NAMES.index(name))
        return (rng.integers(-4, 5, r.size).astype(np.float64), rng.integers(-3, 4, (nc, KMAX[name])), rng.integers(-3, 4, (nr, KMAX[name])))
    return cached(("int", name), make)


def real_values(name):
    """values and X with magnitudes in [0.5, 2) and mixed signs, Y0 likewise, fixed per matrix"""
    def make():
        nr, nc, r, c = matrices()[name]
        rng = np.random.default_rng(400 + NAMES.index(name))
        draw = lambda *n: rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
        km = KMAX[name]
        return (draw(r.size), draw(nc, km), draw(nr, km), draw(nc, km), draw(nr, km))  # values, X for N, X for T, Y0 for T, Y0 for N
    return cached(("real", name), make)


def product(n_out, out, inn, vals, X):
    """sum over the entries of vals * X[inn] into rows `out`, in X's dtype"""
    res = np.zeros((n_out, X.shape[1]), X.dtype)
    if vals.size:
        np.add.at(res, out, vals[:, None] * X[inn])
    return res


def int_ref(name, op):
    """the integer result of op(A) * X on the host COO, in int64 (out_len x KMAX)"""
    def make():
        nr, nc, r, c = matrices()[name]
        vals, xn, xt = int_values(name)
        return product(nc if op else nr, c if op else r, r if op else c, vals.astype(np.int64), (xt if op else xn).astype(np.int64))
    return cached(("int_ref", name, op), make)


def dev(bmsp, a):
    return bmsp.DeviceArray.from_host(np.ascontiguousarray(a))


def run(bmsp, A, Xh, op, alpha=1.0, beta=0.0, Y0=None, stream=None):
    """unit strides: X (in_len x k) on the host in A's dtype, returns Y (out_len x k) on the host"""
    k = Xh.shape[1]
    Y = bmsp.spmm_op(A, dev(bmsp, Xh), k, op, alpha, beta, None if Y0 is None else dev(bmsp, Y0), stream=stream)
    n_out = A.num_cols if op else A.num_rows
    return Y.to_host()[:n_out * k].reshape(n_out, k)


def set_switches(monkeypatch, lanes, split):
    for var, val in (("BMSP_SPMM_OP_LANES", lanes), ("BMSP_SPMV_OP_SPLIT", split)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)


def default_lanes(k):
    return next(w for w in (8, 16, 32, 64) if w >= min(k, 64))


def scratch_slots(bmsp, name, op, split):
    """the scratch slots of the view of (name, op), from the host planner on the tiles' coordinates"""
    nr, nc, r, c = matrices()[name]
    blocks = ((nc if op else nr) + 7) // 8
    tiles = np.unique((r // 8) << 32 | (c // 8))
    ptr = np.concatenate([[0], np.cumsum(np.bincount((tiles & 0xFFFFFFFF) if op else (tiles >> 32), minlength=blocks))])
    return bmsp.spmv_op_plan_items(ptr, split)[2]


def check_launch_info(bmsp, A, name, op, lay, k, lanes, split):
    info = bmsp.spmm_op_launch_info(A, op, k)
    i = A.info()
    if op == 0 and lay == 0:
        assert info["kernel"] == "bmsp_spmm: " + bmsp.spmm_launch_info(A, k), info
        assert (info["lanes"], info["col_chunks"], info["items"], info["split_blocks"]) == (0, 0, 0, 0), info
        return info
    blocks = ((i["num_cols"] if op else i["num_rows"]) + 7) // 8
    if not blocks:
        assert info["kernel"] == "none (no output)" and info["items"] == 0, info
        return info
    W = int(lanes) if lanes else default_lanes(k)
    minor = "MINOR" if (op == 1) != (lay == 1) else "MAJOR"
    assert info["kernel"] == "spmm_op_sweep_kernel<%s, %d>" % (minor, W), info
    assert info["lanes"] == W and info["col_chunks"] == -(-k // W), info
    assert info["items"] >= blocks and info["view_bytes"] >= 16 * i["block_num"], info
    slots = scratch_slots(bmsp, name, op, int(split) if split else 64)
    assert info["scratch_bytes"] >= 8 * k * slots * np.dtype(OUTDT[i["dtype"]]).itemsize, (info, slots)
    if split == "4" and name in SPLIT_NAMES:
        assert info["split_blocks"] > 0 and slots > 0 and info["items"] > blocks, info
    if split is None and name != "rmat":
        assert info["split_blocks"] == 0 and info["items"] == blocks and info["scratch_bytes"] == 0, info
    assert info["compulsory_bytes"] >= np.dtype(OUTDT[i["dtype"]]).itemsize * (i["num_cols"] if op else i["num_rows"]) * k, info
    return info


PARAMS = [(d, lay, op, ln, sp) for d in (0, 1, 2) for lay in (0, 1) for op in (0, 1) for ln in (None, "8", "64") for sp in (None, "4")]
IDS = ["%s-lay%d-%s-lanes%s-split%s" % ("f32 f16 f64".split()[d], lay, "NT"[op], ln or "dflt", sp or "dflt") for d, lay, op, ln, sp in PARAMS]


# ---------------------------------------------------------------------------------------------------------
# 1. exact on integers
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,lay,op,lanes,split", PARAMS, ids=IDS)
def test_exact_on_integers(bmsp, monkeypatch, dtype, lay, op, lanes, split):
    set_switches(monkeypatch, lanes, split)
    for name in NAMES:
        vals, xn, xt = int_values(name)
        A = build(bmsp, name, vals, lay, dtype)  # a fresh matrix: SPLIT is read when the view is built
        snap = snapshot(A)
        other = None if (op, lay) == (0, 0) else (A.transpose(0) if op else A.with_layout(0))  # the materialised route
        n_out = lengths(name, op)[1]
        for k in KS[name]:
            Xh = np.ascontiguousarray((xt if op else xn)[:, :k].astype(NPDT[dtype]))
            X = dev(bmsp, Xh)
            Y = run(bmsp, A, Xh, op)
            assert_exact(Y, int_ref(name, op)[:, :k].astype(OUTDT[dtype]), "%s k=%d" % (name, k))
            check_launch_info(bmsp, A, name, op, lay, k, lanes, split)
            ref = bmsp.spmm(A if other is None else other, X, k).to_host()[:n_out * k].reshape(n_out, k)
            if other is None:  # bmsp_spmm's own case: the call IS bmsp_spmm
                np.testing.assert_array_equal(bits(Y), bits(ref), err_msg=name)
            else:
                assert_exact(ref, Y, name)
            for col in range(k):  # bmsp_spmv_op on the columns
                u = bmsp.spmv_op(A, dev(bmsp, Xh[:, col]), op).to_host()
                assert_exact(u, np.ascontiguousarray(Y[:, col]), "%s k=%d column %d" % (name, k, col))
        assert_unchanged(A, snap)


# ---------------------------------------------------------------------------------------------------------
# 2. rounding bound on real values
# ---------------------------------------------------------------------------------------------------------
def exact_sums(bmsp, name, dtype, op):
    """per output element: the extended-precision sum of a * x over the values STORED in a handle of this dtype, the sum of |a||x| and,
    per output row, the entry count (the stored values do not depend on the tile layout)"""
    def make():
        LD = np.longdouble
        assert np.finfo(LD).nmant >= 63
        vals, xn, xt = real_values(name)[:3]
        r, c, a = stored(build(bmsp, name, vals, 0, dtype))
        out, inn = (c, r) if op else (r, c)
        n_out = lengths(name, op)[1]
        X = (xt if op else xn).astype(NPDT[dtype]).astype(LD)
        return product(n_out, out, inn, a.astype(LD), X), product(n_out, out, inn, np.abs(a.astype(LD)), np.abs(X)), \
            np.bincount(out, minlength=n_out)
    return cached(("exact", name, dtype, op), make)


@pytest.mark.parametrize("dtype,lay,op,lanes,split", PARAMS, ids=IDS)
def test_rounding_bound_on_real_values(bmsp, monkeypatch, dtype, lay, op, lanes, split):
    """|Y - ref| <= gamma_n (|alpha| sum|a||x| + |beta||y0|) per element, gamma_n = n eps / (1 - n eps), n = entries of the row + 6: the
    bound of test_spmv_op.py's test 2.  Derived, not measured."""
    set_switches(monkeypatch, lanes, split)
    LD, R, eps = np.longdouble, OUTDT[dtype], EPS[dtype]
    for name in NAMES:
        vals, xn, xt, y0t, y0n = real_values(name)
        A = build(bmsp, name, vals, lay, dtype)
        t, mag, cnt = exact_sums(bmsp, name, dtype, op)
        n = (cnt + 6).astype(LD)[:, None]
        gamma = n * LD(eps) / (1 - n * LD(eps))
        for k in KS[name]:
            Xh = np.ascontiguousarray((xt if op else xn)[:, :k].astype(NPDT[dtype]))
            Y0 = np.ascontiguousarray((y0t if op else y0n)[:, :k].astype(R))
            for alpha, beta in ALPHA_BETA:
                ar, br = LD(R(alpha)), LD(R(beta))
                Y = run(bmsp, A, Xh, op, alpha, beta, Y0)
                ref = ar * t[:, :k] + br * Y0.astype(LD)
                bound = gamma * (abs(ar) * mag[:, :k] + abs(br) * np.abs(Y0.astype(LD)))
                err = np.abs(Y.astype(LD) - ref)
                assert np.all(err <= bound), (name, k, alpha, beta, float(np.max(err - bound)))


# ---------------------------------------------------------------------------------------------------------
# 3. the epilogue bit for bit, determinism, +0 rows
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("lay,op", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("split", [None, "4"])
def test_epilogue_bit_for_bit(bmsp, monkeypatch, dtype, lay, op, split):
    set_switches(monkeypatch, None, split)
    R = OUTDT[dtype]
    for name in NAMES:
        nr, nc, r, c = matrices()[name]
        vals, xn, xt, y0t, y0n = real_values(name)
        A = build(bmsp, name, vals, lay, dtype)
        k = 17
        Xh = np.ascontiguousarray((xt if op else xn)[:, :k].astype(NPDT[dtype]))
        Y0 = np.ascontiguousarray((y0t if op else y0n)[:, :k].astype(R))
        t = run(bmsp, A, Xh, op, 1.0, 0.0)
        empty = np.bincount(c if op else r, minlength=Y0.shape[0]) == 0
        assert np.all(bits(t)[empty] == 0), name  # a row without stored entries: +0
        if (lay, op) == (0, 0):
            ref = bmsp.spmm(A, dev(bmsp, Xh), k).to_host()[:t.size].reshape(t.shape)
            np.testing.assert_array_equal(bits(t), bits(ref), err_msg=name)
        for alpha, beta in ALPHA_BETA + [(-2.0, 0.0), (1.0, 1.0), (1e-3, 1e3), (-0.3, 0.7)]:
            a, b = R(alpha), R(beta)
            with np.errstate(all="ignore"):
                want = a * t if beta == 0 else a * t + b * Y0
            assert want.dtype == np.dtype(R)
            start = np.full(Y0.shape, np.nan, R) if beta == 0 else Y0  # beta == 0: Y is not read, a NaN in it does not propagate
            got = [run(bmsp, A, Xh, op, alpha, beta, start) for _ in range(2)]
            np.testing.assert_array_equal(bits(got[0]), bits(want), err_msg="%s %r" % (name, (alpha, beta)))
            np.testing.assert_array_equal(bits(got[0]), bits(got[1]))  # two identical calls, identical bits
            if beta == 0:
                assert not np.isnan(got[0]).any()
                assert np.all(bits(got[0])[empty] == bits(np.array([a * R(0.0)], R))[0])  # fl(alpha * (+0)): -0 for a negative alpha


# ---------------------------------------------------------------------------------------------------------
# 4. strides and padding
# ---------------------------------------------------------------------------------------------------------
SENTINEL = -77.0


@pytest.mark.parametrize("dtype,lay,op,lanes,split", PARAMS, ids=IDS)
def test_strides_and_padding(bmsp, monkeypatch, dtype, lay, op, lanes, split):
    """ldx = k + 3, ldy = k + 5, X and Y one element into larger buffers (element-aligned only); NaN in X's padding columns and behind
    its last row, a sentinel in Y's padding and 64 elements before and behind it: the bits of the unit-stride run, every sentinel intact,
    no NaN"""
    set_switches(monkeypatch, lanes, split)
    R, T = OUTDT[dtype], NPDT[dtype]
    for name in ("random", "5x3", "3x70"):
        vals, xn, xt, y0t, y0n = real_values(name)
        A = build(bmsp, name, vals, lay, dtype)
        n_in, n_out = lengths(name, op)
        for k in (3, 17, 70):
            ldx, ldy = k + 3, k + 5
            Xh = np.ascontiguousarray((xt if op else xn)[:, :k].astype(T))
            Y0 = np.ascontiguousarray((y0t if op else y0n)[:, :k].astype(R))
            xbuf = np.full(1 + (n_in + 9) * ldx, np.nan, T)  # nine rows of NaN behind row in_len - 1
            xbuf[1:1 + n_in * ldx].reshape(n_in, ldx)[:, :k] = Xh
            dX = dev(bmsp, xbuf)
            Xv = bmsp.DeviceArray(xbuf.size - 1, T, ptr=dX.ptr + np.dtype(T).itemsize, owner=dX)
            for alpha, beta in ((1.0, 0.0), (0.75, -2.25)):
                unit = run(bmsp, A, Xh, op, alpha, beta, Y0)
                ybuf = np.full(64 + 1 + n_out * ldy + 64, SENTINEL, R)
                ybuf[65:65 + n_out * ldy].reshape(n_out, ldy)[:, :k] = Y0
                dY = dev(bmsp, ybuf)
                Yv = bmsp.DeviceArray(ybuf.size - 65, R, ptr=dY.ptr + 65 * np.dtype(R).itemsize, owner=dY)
                bmsp.spmm_op(A, Xv, k, op, alpha, beta, Yv, ldx=ldx, ldy=ldy)
                out = dY.to_host()
                body = out[65:65 + n_out * ldy].reshape(n_out, ldy)
                np.testing.assert_array_equal(bits(np.ascontiguousarray(body[:, :k])), bits(unit), err_msg="%s k=%d" % (name, k))
                assert not np.isnan(out).any()
                assert np.all(body[:, k:] == SENTINEL) and np.all(out[:65] == SENTINEL) and np.all(out[65 + n_out * ldy:] == SENTINEL)


# ---------------------------------------------------------------------------------------------------------
# 5. stored entries only
# ---------------------------------------------------------------------------------------------------------
TILE = (np.array([0, 0, 2, 3, 3, 5, 7, 7]), np.array([1, 5, 2, 0, 7, 5, 1, 6]))  # one 8 x 8 tile with a few stored positions


def special_matrix(name):
    if name == "tile":
        return 8, 8, TILE[0].astype(np.int64), TILE[1].astype(np.int64)
    return matrices()[name]


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("lay,op", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("lanes", [None, "8", "64"])
@pytest.mark.parametrize("k", [3, 17])
def test_stored_entries_only(bmsp, monkeypatch, dtype, lay, op, lanes, k):
    """X holds Inf or NaN in every row that output row i does not store, inside stored tiles too: row i is finite and exact"""
    set_switches(monkeypatch, lanes, None)
    T, R = NPDT[dtype], OUTDT[dtype]
    rng = np.random.default_rng(77)
    for name in ("tile", "random"):
        nr, nc, r, c = special_matrix(name)
        vals = rng.integers(-4, 5, r.size).astype(np.float64)
        A = bmsp.BmSpMatrix.from_coo(nr, nc, r, c, vals, transposed=lay, dtype=dtype)
        out, inn = (c, r) if op else (r, c)
        n_in, n_out = (nr, nc) if op else (nc, nr)
        Xi = rng.integers(-3, 4, (n_in, k))
        rows = range(n_out) if name == "tile" else (0, 7, 8, 100, n_out - 1)
        for i in rows:
            mine = out == i
            Xh = np.repeat(np.where(np.arange(n_in) % 2 == 0, np.inf, np.nan).astype(T)[:, None], k, axis=1)
            Xh[inn[mine]] = Xi[inn[mine]].astype(T)
            want = (vals[mine].astype(np.int64)[:, None] * Xi[inn[mine]]).sum(axis=0).astype(R)
            with np.errstate(all="ignore"):
                Y = run(bmsp, A, Xh, op)
            assert np.all(np.isfinite(Y[i])), (name, i, Y[i])
            assert_exact(np.ascontiguousarray(Y[i]), want, "%s row %d" % (name, i))


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("lay,op", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("k", [3, 17])
def test_stored_zero_inf_and_subnormals(bmsp, dtype, lay, op, k):
    """a stored 0 against Inf is NaN, a stored Inf propagates, subnormal fp32 products survive: no tolerance"""
    T, R = NPDT[dtype], OUTDT[dtype]
    nr, nc, r, c = special_matrix("tile")
    out, inn = (c, r) if op else (r, c)
    sub = float(np.float32(2.0 ** -140))  # subnormal in fp32 (fp16 cannot hold it: the F16 case carries it in Y's arithmetic through X = 1)
    # (2, 2) is alone in its row and its column: the subnormal product is the whole sum under both ops
    vals = np.array([0.0, 2.0, sub if dtype == 0 else 2.0 ** -24, 3.0, -1.0, np.inf, 1.0, -2.0])
    A = bmsp.BmSpMatrix.from_coo(nr, nc, r, c, vals, transposed=lay, dtype=dtype)
    sr, sc, sv = stored(A)
    so, si = (sc, sr) if op else (sr, sc)
    Xh = np.ones((8, k), T)
    e0 = np.flatnonzero(sv == 0)[0]  # the stored zero meets Inf
    Xh[si[e0]] = np.inf
    with np.errstate(all="ignore"):
        Y = run(bmsp, A, Xh, op)
        want = np.zeros((8, k), R)
        for e in range(sv.size):  # at most two entries per output: the order of the two does not change the sum
            want[so[e]] += R(sv[e]) * Xh[si[e]].astype(R)
    np.testing.assert_array_equal(Y, want)  # (NaN equals NaN: its sign and payload are not part of the contract)
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(bits(Y)[ok], bits(want)[ok])
    assert np.isnan(Y[so[e0]]).all()
    einf = np.flatnonzero(np.isinf(sv))[0]
    assert np.all(np.isinf(Y[so[einf]]) | np.isnan(Y[so[einf]]))
    if dtype == 0:
        es = np.flatnonzero(sv == np.float32(sub))[0]
        alone = np.flatnonzero(so == so[es])
        assert alone.size == 1 and np.all(Y[so[es]] == np.float32(sub)) and np.float32(sub) != 0


# ---------------------------------------------------------------------------------------------------------
# 6. life cycle
# ---------------------------------------------------------------------------------------------------------
def _int_result(nr, nc, r, c, vals, X, op, R):
    return product(nc if op else nr, c if op else r, r if op else c, vals.astype(np.int64), X.astype(np.int64)).astype(R)


@pytest.mark.parametrize("lay", [0, 1])
def test_new_values_in_place_need_no_invalidate(bmsp, lay):
    name, k = "random", 17
    nr, nc, r, c = matrices()[name]
    vals, xn, xt = int_values(name)
    vals2 = np.random.default_rng(9).integers(-4, 5, vals.size).astype(np.float64)
    for dtype in (0, 1, 2):
        A = build(bmsp, name, vals, lay, dtype)
        new = build(bmsp, name, vals2, lay, dtype).host_arrays()[3]
        for op in (0, 1):
            Xh = (xt if op else xn)[:, :k].astype(NPDT[dtype])
            assert_exact(run(bmsp, A, Xh, op), int_ref(name, op)[:, :k].astype(OUTDT[dtype]))
        items = [bmsp.spmm_op_launch_info(A, op, k)["items"] for op in (0, 1)]
        _write_values(bmsp, A, new)  # no invalidate: values are read from the handle's array at every call
        snap = snapshot(A)
        for op in (0, 1):
            Xi = (xt if op else xn)[:, :k]
            Xh = Xi.astype(NPDT[dtype])
            want = _int_result(nr, nc, r, c, vals2, Xi, op, OUTDT[dtype])
            first = run(bmsp, A, Xh, op)
            assert_exact(first, want)
            A.invalidate(False)  # a value-only invalidation keeps the view
            assert bmsp.spmm_op_launch_info(A, op, k)["items"] == items[op]
            np.testing.assert_array_equal(bits(run(bmsp, A, Xh, op)), bits(first))
        assert_unchanged(A, snap)


@pytest.mark.parametrize("lay", [0, 1])
def test_structure_change_with_invalidate(bmsp, lay, monkeypatch):
    """the arrays of the second matrix of test_spmv_op.py's test of this name written over A's: after invalidate(True) the results follow"""
    from pybmsp import gen
    monkeypatch.setenv("BMSP_SPMV_OP_SPLIT", "4")
    n, k = 96, 17
    _, _, r, c, _ = gen.random_coo(n, n, 900, seed=4)
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    c2 = (c + 40) % n  # every tile moves five block-columns on: same tile count, same nnz, another order
    rng = np.random.default_rng(12)
    vals, Xi = rng.integers(-4, 5, r.size).astype(np.float64), rng.integers(-3, 4, (n, k))
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, vals, transposed=lay, dtype=0)
    B = bmsp.BmSpMatrix.from_coo(n, n, r, c2, vals, transposed=lay, dtype=0)
    assert (A.block_num, A.nnz) == (B.block_num, B.nnz)
    Xh = Xi.astype(np.float32)
    for op in (0, 1):
        assert_exact(run(bmsp, A, Xh, op), _int_result(n, n, r, c, vals, Xi, op, np.float32))
    for dst, src in zip(A.device_arrays(), B.host_arrays()):
        bmsp.check(bmsp.lib().bmsp_memcpy_h2d(dst.ptr, src.ctypes.data, src.nbytes))
    A.invalidate(True)
    for op in (0, 1):
        assert_exact(run(bmsp, A, Xh, op), _int_result(n, n, r, c2, vals, Xi, op, np.float32))
        ia, ib = bmsp.spmm_op_launch_info(A, op, k), bmsp.spmm_op_launch_info(B, op, k)
        if (op, lay) == (0, 0):  # no view: view_bytes / scratch_bytes report the temporary, which only a call with an epilogue makes
            ia = dict(ia, view_bytes=0, scratch_bytes=0)
            ib = dict(ib, view_bytes=0, scratch_bytes=0)
        assert ia == ib


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("lay,op", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_scratch_grows_and_is_reused(bmsp, monkeypatch, dtype, lay, op):
    """k = 3, 70, 3 on one handle under SPLIT = 4 (and with an epilogue, for the temporary of (N, row-major)): each result bit-equal to
    the same call on a fresh handle"""
    monkeypatch.setenv("BMSP_SPMV_OP_SPLIT", "4")
    name = "random"
    vals, xn, xt, y0t, y0n = real_values(name)
    A = build(bmsp, name, vals, lay, dtype)
    for k in (3, 70, 3):
        Xh = np.ascontiguousarray((xt if op else xn)[:, :k].astype(NPDT[dtype]))
        Y0 = np.ascontiguousarray((y0t if op else y0n)[:, :k].astype(OUTDT[dtype]))
        for alpha, beta in ((1.0, 0.0), (0.75, -2.25)):
            fresh = run(bmsp, build(bmsp, name, vals, lay, dtype), Xh, op, alpha, beta, Y0)
            np.testing.assert_array_equal(bits(run(bmsp, A, Xh, op, alpha, beta, Y0)), bits(fresh), err_msg="k=%d" % k)


def test_interleaving_on_one_handle(bmsp):
    """bmsp_spmv, bmsp_spmm, bmsp_spmv_op and bmsp_spmm_op with both ops on one row-major handle: every result as it was alone"""
    name, k = "rmat", 17
    vals, xn, xt, y0t, y0n = real_values(name)
    A = build(bmsp, name, vals, 0, 0)
    snap = snapshot(A)
    f32 = lambda a: np.ascontiguousarray(a.astype(np.float32))
    Xn, Xt, Yn, Yt = f32(xn[:, :k]), f32(xt[:, :k]), f32(y0n[:, :k]), f32(y0t[:, :k])
    dn, dt, dXn = dev(bmsp, f32(xn[:, 0])), dev(bmsp, f32(xt[:, 0])), dev(bmsp, Xn)
    calls = {"spmv": lambda: bmsp.spmv(A, dn).to_host(), "spmm": lambda: bmsp.spmm(A, dXn, k).to_host(),
             "vN": lambda: bmsp.spmv_op(A, dn, "N").to_host(), "vT": lambda: bmsp.spmv_op(A, dt, "T").to_host(),
             "vT+": lambda: A.rmatvec(dt, 0.75, -2.25, dev(bmsp, f32(y0t[:, 0]))).to_host(),
             "N": lambda: run(bmsp, A, Xn, 0), "T": lambda: run(bmsp, A, Xt, 1),
             "N+": lambda: A.matmat(dXn, k, 0.75, -2.25, dev(bmsp, Yn)).to_host(),
             "T+": lambda: A.rmatmat(dev(bmsp, Xt), k, 0.75, -2.25, dev(bmsp, Yt)).to_host()}
    alone = {key: f() for key, f in calls.items()}
    for order in (("T", "spmv", "N+", "vT", "T+", "spmm", "N", "vT+"), ("N+", "T", "vT+", "T", "spmm", "T+", "vN", "N", "spmv", "vT")):
        for key in order:
            np.testing.assert_array_equal(bits(calls[key]()), bits(alone[key]), err_msg=key)
    np.testing.assert_array_equal(bits(alone["spmm"]), bits(alone["N"].ravel()))
    assert_unchanged(A, snap)


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_column_major_outputs_of_add_and_prune_multiply(bmsp, dtype):
    name, k = "random", 17
    nr, nc, r, c = matrices()[name]
    vals, xn, xt = int_values(name)
    A = build(bmsp, name, vals, 0, dtype)
    B = build(bmsp, name, np.roll(vals, 7), 1, dtype)
    made = {"add": bmsp.add(A, B, 1.0, -1.0, transposed=1), "prune": A.prune(1.5, transposed=1)[0]}
    for what, M in made.items():
        assert M.info()["transposed"] == 1
        mr, mc, mv = M.to_coo()
        assert what != "prune" or (0 < mv.size < vals.size and np.all(np.abs(mv) > 1.5))
        for op in (0, 1):
            Xi = (xt if op else xn)[:, :k]
            want = _int_result(nr, nc, mr.astype(np.int64), mc.astype(np.int64), mv, Xi, op, OUTDT[dtype])
            assert_exact(run(bmsp, M, Xi.astype(NPDT[dtype]), op), want, what)


# ---------------------------------------------------------------------------------------------------------
# 7. streams
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [0, 1])
def test_on_a_gated_stream(bmsp, monkeypatch, op):
    """a column-major matrix (both ops sweep a view), fp32, k = 17, SPLIT = 4 so that the call needs scratch.  With the view and the
    scratch in place the call returns while the gate is SEEN closed; a first call on a handle builds the view and returns only after
    the gate's timeout.  Both results equal the null-stream result bit for bit."""
    monkeypatch.setenv("BMSP_SPMV_OP_SPLIT", "4")
    name, k = "random", 17
    vals, xn, xt, y0t, y0n = real_values(name)
    Xh = np.ascontiguousarray((xt if op else xn)[:, :k].astype(np.float32))
    Y0 = np.ascontiguousarray((y0t if op else y0n)[:, :k].astype(np.float32))
    A = build(bmsp, name, vals, 1, 0)
    want = run(bmsp, A, Xh, op, 0.75, -2.25, Y0)  # the null stream; builds the view and the scratch
    assert bmsp.spmm_op_launch_info(A, op, k)["scratch_bytes"] > 0
    s = new_stream()
    try:
        X, Y = dev(bmsp, Xh), dev(bmsp, Y0)
        bmsp.synchronize()
        gate = Gate().close(s)
        try:
            bmsp.spmm_op(A, X, k, op, 0.75, -2.25, Y, stream=s.value)
            seen_closed = gate.is_closed()
        finally:
            gate.finish()
        assert seen_closed, "the call did not return while the gate was closed"
        np.testing.assert_array_equal(bits(Y.to_host().reshape(want.shape)), bits(want))
        # a first call on a fresh handle: the view build synchronises the stream
        B = build(bmsp, name, vals, 1, 0)
        Y = dev(bmsp, Y0)
        bmsp.synchronize()
        gate = Gate().close(s)
        try:
            bmsp.spmm_op(B, X, k, op, 0.75, -2.25, Y, stream=s.value)
            by_timeout = gate.opened_by_timeout()
        finally:
            gate.finish()
        assert by_timeout, "the first call returned before the gate's timeout"
        np.testing.assert_array_equal(bits(Y.to_host().reshape(want.shape)), bits(want))
    finally:
        destroy_stream(s)


# ---------------------------------------------------------------------------------------------------------
# 8. refusals on real handles, and the C++ wrapper
# ---------------------------------------------------------------------------------------------------------
def test_row_panel_view_and_null_operands_are_refused(bmsp):
    vals, xn, xt = int_values("random")
    A = build(bmsp, "random", vals, 0, 0)
    k = 3
    n = max(A.num_rows, A.num_cols)
    X, Y = dev(bmsp, np.ones(n * k, np.float32)), bmsp.DeviceArray(n * k, np.float32)
    P = A.row_panel(1, 3)
    for op in (0, 1):
        with pytest.raises(bmsp.BmspError) as e:
            bmsp.spmm_op(P, X, k, op, Y=Y)
        assert e.value.status == -1 and "view" in str(e.value)
        with pytest.raises(bmsp.BmspError) as e:
            bmsp.spmm_op_launch_info(P, op, k)
        assert e.value.status == -1 and "view" in str(e.value)
    L = bmsp.lib()
    msg = lambda: L.bmsp_last_error().decode()
    assert L.bmsp_spmm_op(A.h, 1, 1.0, None, k, 0.0, Y.ptr, k, k, None) == -1 and "d_X" in msg() and "null" in msg()
    assert L.bmsp_spmm_op(A.h, 1, 1.0, X.ptr, k, 0.0, None, k, k, None) == -1 and "d_Y" in msg() and "null" in msg()
    assert L.bmsp_spmm_op_launch_info(A.h, 1, k, k, k, None) == -1 and "info" in msg() and "null" in msg()
    assert L.bmsp_spmm_op(A.h, 3, 1.0, X.ptr, k, 0.0, Y.ptr, k, k, None) == -1 and "op" in msg()
    assert L.bmsp_spmm_op(A.h, 1, 1.0, X.ptr, k, 0.0, Y.ptr, k, 0, None) == -1 and "k" in msg()
    assert L.bmsp_spmm_op(A.h, 1, 1.0, X.ptr, k - 1, 0.0, Y.ptr, k, k, None) == -1 and "ldx" in msg()
    assert L.bmsp_spmm_op(A.h, 1, 1.0, X.ptr, k, 0.0, Y.ptr, k - 1, k, None) == -1 and "ldy" in msg()


def test_cpp_wrapper_runs(tmp_path):
    """tests/cpp_spmm_op_check.cpp: bmSparse_SpMM_op for float, half and double on the data/real fixture, both layouts and both ops"""
    from conftest import MTX
    from test_spmm_op_api import build_cpp_spmm_op_check
    exe = str(tmp_path / "cpp_spmm_op_check")
    build_cpp_spmm_op_check(exe)
    out = subprocess.run([exe, os.path.join(MTX, "real", "A_matrix.mtx")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("OK") == 3 and "FAIL" not in out.stdout, out.stdout
