"""GPU tests of bmsp_spmv_op: u = alpha * op(A) * v + beta * u for op in {N, T} and both tile layouts.

Expected values come from numpy on the host: integer operands make every summation order exact (test 1: bit for bit against the integer
result, against bmsp_spmv on the materialised transpose / layout conversion, and across the switch settings -- a zero sum compares as a
value where another kernel's order may sign it, see assert_exact); real operands are held to
the any-order summation bound derived below (test 2); the epilogue is checked bit for bit against numpy arithmetic in the vector type
(test 3).  Tests 4 - 6 cover the cached views' life cycle, streams, operands made by the other device operations and refusals."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from stream_gate import _hip
from test_transpose import snapshot, assert_unchanged, _write_values
from test_add import stored

pytestmark = pytest.mark.gpu

NPDT = {0: np.float32, 1: np.float16, 2: np.float64}
OUTDT = {0: np.float32, 1: np.float32, 2: np.float64}
UINT = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}
EPS = {0: 2.0 ** -24, 1: 2.0 ** -24, 2: 2.0 ** -53}
ALPHA_BETA = [(1.0, 0.0), (-1.5, 0.0), (0.75, -2.25), (0.0, 1.0)]
SPLIT_NAMES = ("random", "banded", "rmat")  # under BMSP_SPMV_OP_SPLIT=4 these have output blocks of more than 4 tiles in both directions

_CACHE = {}


def matrices():
    """{name: (num_rows, num_cols, rows, cols)}: the coordinates only, generated once"""
    if "coo" not in _CACHE:
        from pybmsp import gen
        e = np.zeros(0, np.int32)
        m = {"random": gen.random_coo(203, 157, 203 * 26, seed=3), "banded": gen.banded(400, 12), "rmat": gen.rmat(14, 8),
             "sparse_rect": gen.random_coo(300, 500, 150, seed=5), "1x1": (1, 1, np.array([0]), np.array([0]), None),
             "5x3": gen.random_coo(5, 3, 9, seed=6), "3x70": gen.random_coo(3, 70, 60, seed=7), "nnz0": (37, 11, e, e, None),
             "rows0": (0, 13, e, e, None)}
        _CACHE["coo"] = {k: (x[0], x[1], np.asarray(x[2], np.int64), np.asarray(x[3], np.int64)) for k, x in m.items()}
    return _CACHE["coo"]


NAMES = ("random", "banded", "rmat", "sparse_rect", "1x1", "5x3", "3x70", "nnz0", "rows0")


def int_values(name):
    """integer values in [-4, 4] per stored coordinate and integer vectors in [-3, 3] for both ops, fixed per matrix"""
    key = ("int", name)
    if key not in _CACHE:
        nr, nc, r, c = matrices()[name]
        rng = np.random.default_rng(100 + NAMES.index(name))
        _CACHE[key] = (rng.integers(-4, 5, r.size).astype(np.float64), rng.integers(-3, 4, nc), rng.integers(-3, 4, nr))
    return _CACHE[key]


def real_values(name):
    """values and vectors with magnitudes in [0.5, 2) and mixed signs (no underflow anywhere), u0 likewise, fixed per matrix"""
    key = ("real", name)
    if key not in _CACHE:
        nr, nc, r, c = matrices()[name]
        rng = np.random.default_rng(200 + NAMES.index(name))
        draw = lambda n: rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
        _CACHE[key] = (draw(r.size), draw(nc), draw(nr), draw(nc), draw(nr))  # values, v for N, v for T, u0 for T, u0 for N
    return _CACHE[key]


def int_ref(name, op):
    """the integer result of op(A) * v on the host COO, in int64"""
    key = ("int_ref", name, op)
    if key not in _CACHE:
        nr, nc, r, c = matrices()[name]
        vals, vn, vt = int_values(name)
        out = np.zeros(nc if op else nr, np.int64)
        np.add.at(out, c if op else r, vals.astype(np.int64) * (vt[r] if op else vn[c]))
        _CACHE[key] = out
    return _CACHE[key]


def build(bmsp, name, vals, lay, dtype):
    nr, nc, r, c = matrices()[name]
    return bmsp.BmSpMatrix.from_coo(nr, nc, r, c, vals, transposed=lay, dtype=dtype)


def bits(a):
    return np.ascontiguousarray(a).view(UINT[a.dtype])


def assert_exact(got, want, msg=""):
    """equal as values everywhere, bit for bit wherever the result is not zero.  The sign of a zero SUM of stored entries is the
    summation order's even when every operation is exact ((-0) + (-0) = -0, x + (-x) = +0; a lone product 0 * (-3) is -0), and
    bmsp_spmv's sweeps, which (N, row-major) must reproduce, do not all start from +0: such zeros compare as values.  (Rows WITHOUT
    stored entries are +0 by contract: test 3.)"""
    assert got.dtype == want.dtype and got.shape == want.shape, msg
    np.testing.assert_array_equal(got, want, err_msg=msg)
    nz = want != 0
    np.testing.assert_array_equal(bits(got)[nz], bits(want)[nz], err_msg=msg)


def set_switches(monkeypatch, slots, split):
    for var, val in (("BMSP_SPMV_OP_SLOTS", slots), ("BMSP_SPMV_OP_SPLIT", split)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)


def check_launch_info(bmsp, A, name, op, lay, slots, split):
    """the launcher's decisions: the slots asked for (or the default from the mean number of tiles per output block), split blocks
    under a small SPLIT; (N, row-major) is bmsp_spmv and has no view"""
    info = bmsp.spmv_op_launch_info(A, op)
    i = A.info()
    if op == 0 and lay == 0:
        assert info["kernel"].startswith("bmsp_spmv: ") and (info["slots"], info["items"], info["split_blocks"]) == (0, 0, 0), info
        return info
    blocks = ((i["num_cols"] if op else i["num_rows"]) + 7) // 8
    want = int(slots) if slots else (8 if i["block_num"] >= 6 * blocks else 1)  # the measured threshold: 6 tiles per output block
    assert info["slots"] == want, (info, want)
    assert info["items"] >= blocks and info["view_bytes"] >= 16 * i["block_num"]
    if blocks:
        minor = "MINOR" if (op == 1) != (lay == 1) else "MAJOR"
        assert info["kernel"] == "spmv_op_sweep_kernel<%s, %d>" % (minor, want), info
    if split == "4" and name in SPLIT_NAMES:
        assert info["split_blocks"] > 0 and info["items"] > blocks, info
    if split is None and name != "rmat":
        assert info["split_blocks"] == 0 and info["items"] == blocks, info  # nothing here has more than 64 tiles in one block
    return info


def test_the_matrices_are_what_the_cases_need():
    m = matrices()
    nr, nc, r, c = m["rmat"]
    tiles = np.unique((r // 8) << 32 | (c // 8))
    by_row, by_col = np.bincount(tiles >> 32), np.bincount(tiles & 0xFFFFFFFF)
    assert by_row.max() > 1000 and by_col.max() > 1000, (by_row.max(), by_col.max())  # hub block-row and hub block-column
    nr, nc, r, c = m["sparse_rect"]
    assert np.unique(r // 8).size < (nr + 7) // 8 and np.unique(c // 8).size < (nc + 7) // 8  # empty block-rows and block-columns
    longest = max(max(np.bincount(x[2]).max(), np.bincount(x[3]).max()) for x in m.values() if x[2].size)
    assert longest * 4 * 3 < 2 ** 24, longest  # every partial sum of test 1 is an integer below 2^24: exact in fp32 in any order


PARAMS = [(d, lay, op, sl, sp) for d in (0, 1, 2) for lay in (0, 1) for op in (0, 1) for sl in (None, "1", "8") for sp in (None, "4")]
IDS = ["%s-lay%d-%s-slots%s-split%s" % ("f32 f16 f64".split()[d], lay, "NT"[op], sl or "dflt", sp or "dflt") for d, lay, op, sl, sp in PARAMS]


# ---------------------------------------------------------------------------------------------------------
# 1. exact on integers
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,lay,op,slots,split", PARAMS, ids=IDS)
def test_exact_on_integers(bmsp, monkeypatch, dtype, lay, op, slots, split):
    set_switches(monkeypatch, slots, split)
    for name in NAMES:
        vals, vn, vt = int_values(name)
        A = build(bmsp, name, vals, lay, dtype)  # a fresh matrix: SPLIT is read when the view is built
        snap = snapshot(A)
        v = bmsp.DeviceArray.from_host((vt if op else vn).astype(NPDT[dtype]))
        u = bmsp.spmv_op(A, v, op).to_host()
        assert_exact(u, int_ref(name, op).astype(OUTDT[dtype]), name)
        first = _CACHE.setdefault(("seen", dtype, lay, op, name), u)  # every switch setting gives the same bits
        np.testing.assert_array_equal(bits(u), bits(first), err_msg=name)
        check_launch_info(bmsp, A, name, op, lay, slots, split)
        if op == 1:  # the materialised transpose through the tuned sweep
            assert_exact(bmsp.spmv(A.transpose(0), v).to_host(), u, name)
        elif lay == 1:
            assert_exact(bmsp.spmv(A.with_layout(0), v).to_host(), u, name)
        else:  # bmsp_spmv's own case: the same bits
            np.testing.assert_array_equal(bits(bmsp.spmv(A, v).to_host()), bits(u), err_msg=name)
        assert_unchanged(A, snap)


# ---------------------------------------------------------------------------------------------------------
# 2. rounding bound on real values
# ---------------------------------------------------------------------------------------------------------
def exact_sums(A, v_host, op, n_out):
    """per output: the extended-precision sum of a * v over the values STORED in the handle, the sum of |a||v| and the entry count"""
    LD = np.longdouble
    assert np.finfo(LD).nmant >= 63
    r, c, a = stored(A)
    out, inn = (c, r) if op else (r, c)
    prod = a.astype(LD) * v_host.astype(LD)[inn]
    t, mag = np.zeros(n_out, LD), np.zeros(n_out, LD)
    np.add.at(t, out, prod)
    np.add.at(mag, out, np.abs(prod))
    return t, mag, np.bincount(out, minlength=n_out)


@pytest.mark.parametrize("dtype,lay,op,slots,split", PARAMS, ids=IDS)
def test_rounding_bound_on_real_values(bmsp, monkeypatch, dtype, lay, op, slots, split):
    """|u_j - ref_j| <= gamma_k (|alpha| sum|a||v| + |beta||u0_j|), gamma_k = k eps / (1 - k eps), k = n_j + 6: n_j roundings of the
    products (none when fused) and n_j - 1 of the sums in any order, plus the epilogue's; eps = 2^-24 (2^-53 for F64).  Derived, not
    measured: it holds for every legal implementation."""
    set_switches(monkeypatch, slots, split)
    LD, R, eps = np.longdouble, OUTDT[dtype], EPS[dtype]
    for name in NAMES:
        vals, vn, vt, u0t, u0n = real_values(name)
        A = build(bmsp, name, vals, lay, dtype)
        vh = (vt if op else vn).astype(NPDT[dtype])
        u0 = (u0t if op else u0n).astype(R)
        v = bmsp.DeviceArray.from_host(vh)
        t, mag, cnt = exact_sums(A, vh, op, u0.size)
        k = (cnt + 6).astype(LD)
        gamma = k * LD(eps) / (1 - k * LD(eps))
        for alpha, beta in ALPHA_BETA:
            ar, br = LD(R(alpha)), LD(R(beta))
            u = bmsp.spmv_op(A, v, op, alpha, beta, bmsp.DeviceArray.from_host(u0)).to_host()
            ref = ar * t + br * u0.astype(LD)
            bound = gamma * (abs(ar) * mag + abs(br) * np.abs(u0.astype(LD)))
            err = np.abs(u.astype(LD) - ref)
            assert np.all(err <= bound), (name, alpha, beta, float(np.max(err - bound)))


# ---------------------------------------------------------------------------------------------------------
# 3. the epilogue, bit for bit
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("lay,op", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_epilogue_bit_for_bit(bmsp, dtype, lay, op):
    R = OUTDT[dtype]
    for name in NAMES:
        nr, nc, r, c = matrices()[name]
        vals, vn, vt, u0t, u0n = real_values(name)
        A = build(bmsp, name, vals, lay, dtype)
        v = bmsp.DeviceArray.from_host((vt if op else vn).astype(NPDT[dtype]))
        u0 = (u0t if op else u0n).astype(R)
        t = bmsp.spmv_op(A, v, op, 1.0, 0.0).to_host()
        empty = np.bincount(c if op else r, minlength=u0.size) == 0
        assert np.all(bits(t)[empty] == 0), name  # a row without stored entries: +0
        if (lay, op) == (0, 0):
            np.testing.assert_array_equal(bits(t), bits(bmsp.spmv(A, v).to_host()), err_msg=name)
        for alpha, beta in ALPHA_BETA + [(-2.0, 0.0), (1.0, 1.0), (1e-3, 1e3), (-0.3, 0.7)]:
            a, b = R(alpha), R(beta)
            with np.errstate(all="ignore"):
                want = a * t if beta == 0 else a * t + b * u0
            assert want.dtype == np.dtype(R)
            start = np.full(u0.size, np.nan, R) if beta == 0 else u0  # beta == 0: u is not read, a NaN in it does not propagate
            got = [bmsp.spmv_op(A, v, op, alpha, beta, bmsp.DeviceArray.from_host(start)).to_host() for _ in range(2)]
            np.testing.assert_array_equal(bits(got[0]), bits(want), err_msg="%s %r" % (name, (alpha, beta)))
            np.testing.assert_array_equal(bits(got[0]), bits(got[1]))  # two identical calls, identical bits
            if beta == 0:
                assert not np.isnan(got[0]).any()
                assert np.all(bits(got[0])[empty] == bits(np.array([a * R(0.0)], R))[0])  # fl(alpha * (+0)): -0 for a negative alpha


# ---------------------------------------------------------------------------------------------------------
# 4. caches and values
# ---------------------------------------------------------------------------------------------------------
def _int_result(nr, nc, r, c, vals, vec, op, R):
    out = np.zeros(nc if op else nr, np.int64)
    np.add.at(out, c if op else r, vals.astype(np.int64) * (vec[r] if op else vec[c]))
    return out.astype(R)


@pytest.mark.parametrize("lay", [0, 1])
def test_new_values_in_place_need_no_invalidate(bmsp, lay):
    name = "random"
    nr, nc, r, c = matrices()[name]
    vals, vn, vt = int_values(name)
    vals2 = np.random.default_rng(9).integers(-4, 5, vals.size).astype(np.float64)
    for dtype in (0, 1, 2):
        A = build(bmsp, name, vals, lay, dtype)
        new = build(bmsp, name, vals2, lay, dtype).host_arrays()[3]
        for op in (0, 1):
            v = bmsp.DeviceArray.from_host((vt if op else vn).astype(NPDT[dtype]))
            before = bmsp.spmv_op(A, v, op).to_host()
            assert_exact(before, int_ref(name, op).astype(OUTDT[dtype]))
        items = [bmsp.spmv_op_launch_info(A, op)["items"] for op in (0, 1)]
        _write_values(bmsp, A, new)  # no invalidate: values are read from the handle's array at every call
        snap = snapshot(A)
        for op in (0, 1):
            vec = vt if op else vn
            v = bmsp.DeviceArray.from_host(vec.astype(NPDT[dtype]))
            want = _int_result(nr, nc, r, c, vals2, vec, op, OUTDT[dtype])
            assert_exact(bmsp.spmv_op(A, v, op).to_host(), want)
            A.invalidate(False)  # a value-only invalidation keeps the views
            assert bmsp.spmv_op_launch_info(A, op)["items"] == items[op]
            assert_exact(bmsp.spmv_op(A, v, op).to_host(), want)
        assert_unchanged(A, snap)


@pytest.mark.parametrize("lay", [0, 1])
def test_structure_change_with_invalidate(bmsp, lay, monkeypatch):
    """the arrays of a second matrix with the same tile and value counts written over A's: after invalidate(True) the results follow"""
    from pybmsp import gen
    monkeypatch.setenv("BMSP_SPMV_OP_SPLIT", "4")
    n = 96
    _, _, r, c, _ = gen.random_coo(n, n, 900, seed=4)
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    c2 = (c + 40) % n  # every tile moves five block-columns on: same tile count, same nnz, another order
    rng = np.random.default_rng(12)
    vals, vec = rng.integers(-4, 5, r.size).astype(np.float64), rng.integers(-3, 4, n)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, vals, transposed=lay, dtype=0)
    B = bmsp.BmSpMatrix.from_coo(n, n, r, c2, vals, transposed=lay, dtype=0)
    assert (A.block_num, A.nnz) == (B.block_num, B.nnz)
    v = bmsp.DeviceArray.from_host(vec.astype(np.float32))
    for op in (0, 1):
        assert_exact(bmsp.spmv_op(A, v, op).to_host(), _int_result(n, n, r, c, vals, vec, op, np.float32))
    for dst, src in zip(A.device_arrays(), B.host_arrays()):
        bmsp.check(bmsp.lib().bmsp_memcpy_h2d(dst.ptr, src.ctypes.data, src.nbytes))
    A.invalidate(True)
    for op in (0, 1):
        assert_exact(bmsp.spmv_op(A, v, op).to_host(), _int_result(n, n, r, c2, vals, vec, op, np.float32))
        assert bmsp.spmv_op_launch_info(A, op) == bmsp.spmv_op_launch_info(B, op)


def test_interleaving_on_one_handle(bmsp):
    """bmsp_spmv, op N and op T on one row-major handle, with and without an epilogue: every result as it was alone"""
    name = "rmat"
    vals, vn, vt, u0t, u0n = real_values(name)
    A = build(bmsp, name, vals, 0, 0)
    snap = snapshot(A)
    dn, dt = bmsp.DeviceArray.from_host(vn.astype(np.float32)), bmsp.DeviceArray.from_host(vt.astype(np.float32))
    un, ut = u0n.astype(np.float32), u0t.astype(np.float32)
    calls = {"spmv": lambda: bmsp.spmv(A, dn), "N": lambda: bmsp.spmv_op(A, dn, "N"), "T": lambda: bmsp.spmv_op(A, dt, "T"),
             "N+": lambda: A.matvec(dn, 0.75, -2.25, bmsp.DeviceArray.from_host(un)),
             "T+": lambda: A.rmatvec(dt, 0.75, -2.25, bmsp.DeviceArray.from_host(ut))}
    alone = {k: f().to_host() for k, f in calls.items()}
    for order in (("T", "spmv", "N+", "T+", "N"), ("N+", "T", "T", "spmv", "T+", "N", "spmv")):
        for k in order:
            np.testing.assert_array_equal(bits(calls[k]().to_host()), bits(alone[k]), err_msg=k)
    np.testing.assert_array_equal(bits(alone["spmv"]), bits(alone["N"]))
    assert_unchanged(A, snap)


# ---------------------------------------------------------------------------------------------------------
# 5. streams, and the outputs of the other operations
# ---------------------------------------------------------------------------------------------------------
def test_on_a_stream(bmsp):
    H = _hip()
    s = C.c_void_p()
    assert H.hipStreamCreate(C.byref(s)) == 0
    try:
        for name, lay in (("rmat", 0), ("random", 1)):
            vals, vn, vt = int_values(name)
            A = build(bmsp, name, vals, lay, 0)
            for op in (0, 1):
                v = bmsp.DeviceArray.from_host((vt if op else vn).astype(np.float32))
                u0 = np.ones(int_ref(name, op).size, np.float32)
                u = bmsp.spmv_op(A, v, op, 2.0, -1.0, bmsp.DeviceArray.from_host(u0), stream=s.value)
                assert H.hipStreamSynchronize(s) == 0
                assert_exact(u.to_host(), (2 * int_ref(name, op) - 1).astype(np.float32))
    finally:
        H.hipStreamDestroy(s)


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_column_major_outputs_of_add_and_prune_multiply(bmsp, dtype):
    name = "random"
    nr, nc, r, c = matrices()[name]
    vals, vn, vt = int_values(name)
    A = build(bmsp, name, vals, 0, dtype)
    B = build(bmsp, name, np.roll(vals, 7), 1, dtype)
    made = {"add": bmsp.add(A, B, 1.0, -1.0, transposed=1), "prune": A.prune(1.5, transposed=1)[0]}
    for what, M in made.items():
        assert M.info()["transposed"] == 1
        mr, mc, mv = M.to_coo()
        assert what != "prune" or (0 < mv.size < vals.size and np.all(np.abs(mv) > 1.5))
        for op in (0, 1):
            vec = vt if op else vn
            v = bmsp.DeviceArray.from_host(vec.astype(NPDT[dtype]))
            want = _int_result(nr, nc, mr.astype(np.int64), mc.astype(np.int64), mv, vec, op, OUTDT[dtype])
            assert_exact(bmsp.spmv_op(M, v, op).to_host(), want, what)


# ---------------------------------------------------------------------------------------------------------
# 6. refusals on real handles, and the C++ wrapper
# ---------------------------------------------------------------------------------------------------------
def test_row_panel_view_and_null_vectors_are_refused(bmsp):
    vals, vn, vt = int_values("random")
    A = build(bmsp, "random", vals, 0, 0)
    v, u = bmsp.DeviceArray.from_host(vt.astype(np.float32)), bmsp.DeviceArray(A.num_cols, np.float32)
    P = A.row_panel(1, 3)
    for op in (0, 1):
        with pytest.raises(bmsp.BmspError) as e:
            bmsp.spmv_op(P, bmsp.DeviceArray.from_host(np.ones(max(A.num_rows, A.num_cols), np.float32)), op,
                         u=bmsp.DeviceArray(max(A.num_rows, A.num_cols), np.float32))
        assert e.value.status == -1 and "view" in str(e.value)
        with pytest.raises(bmsp.BmspError) as e:
            bmsp.spmv_op_launch_info(P, op)
        assert e.value.status == -1 and "view" in str(e.value)
    L = bmsp.lib()
    msg = lambda: L.bmsp_last_error().decode()
    assert L.bmsp_spmv_op(A.h, 1, 1.0, None, 0.0, u.ptr, None) == -1 and "d_v" in msg() and "null" in msg()
    assert L.bmsp_spmv_op(A.h, 1, 1.0, v.ptr, 0.0, None, None) == -1 and "d_u" in msg() and "null" in msg()
    assert L.bmsp_spmv_op_launch_info(A.h, 1, None) == -1 and "info" in msg() and "null" in msg()
    assert L.bmsp_spmv_op(A.h, 3, 1.0, v.ptr, 0.0, u.ptr, None) == -1 and "op" in msg()


def test_cpp_wrapper_runs(tmp_path):
    """tests/cpp_spmv_op_check.cpp: bmSparse_SpMV_op for float, half and double on the data/real fixture, both layouts and both ops"""
    from conftest import MTX
    from test_spmv_op_api import build_cpp_spmv_op_check
    exe = str(tmp_path / "cpp_spmv_op_check")
    build_cpp_spmv_op_check(exe)
    out = subprocess.run([exe, os.path.join(MTX, "real", "A_matrix.mtx")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("OK") == 3 and "FAIL" not in out.stdout, out.stdout
