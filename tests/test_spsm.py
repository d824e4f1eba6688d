"""GPU tests of bmsp_spsm: op(tri(A)) X = alpha B for k right-hand sides.  The contract is one sentence -- column c of X holds, bit for
bit, what bmsp_spsv writes for column c of B -- so the reference for a column is tests/spsv_ref.c on that column (through
test_spsv_api.reference) and there is no tolerance anywhere.  The matrices, their values and the reference live in tests/test_spsv_api.py.
B's padding columns hold NaN in every test: they are never read."""
import subprocess
import numpy as np
import pytest
from test_spsv_api import MATRICES, SMALL, SHAPES, VEC, values, rhs, reference, assert_same_bits
from test_spsv import OPS, FILLS, CHAINS, COMBOS, set_chain, build, case, refused
from test_spsm_api import build_cpp_spsm_check

pytestmark = pytest.mark.gpu

SENTINEL = {np.dtype(np.float32): np.uint32(0xDEADBEEF), np.dtype(np.float64): np.uint64(0xDEADBEEFDEADBEEF)}


def sentinel(shape, R):
    """an array of R filled with a bit pattern no solve produces (a large negative number, not a NaN)"""
    R = np.dtype(R)
    return np.full(shape, SENTINEL[R], SENTINEL[R].dtype).view(R)


def make_B(n, k, ldb, dtype):
    """n x ldb: column c is the right-hand side of seed 5 + c (the first k columns do not depend on k), the padding NaN"""
    B = np.full((n, ldb), np.nan, VEC[dtype])
    for c in range(k):
        B[:, c] = rhs(n, dtype, seed=5 + c)
    return B


def wanted(n, r, c, v, dtype, op, fill, unit, alpha, B, k):
    """n x k: the helper's solve of every column"""
    return np.stack([reference(n, r, c, v, dtype, op, fill, unit, alpha, np.ascontiguousarray(B[:, j])) for j in range(k)], axis=1)


def solve(bmsp, A, B, k, ldx, op, fill, unit, alpha=1.0, dtype=0, rows=None):
    """X as rows x ldx on the host: made of the sentinel, solved into"""
    n = B.shape[0]
    R = VEC[dtype]
    X = bmsp.DeviceArray.from_host(sentinel((n if rows is None else rows, ldx), R), R)
    out = bmsp.spsm(A, bmsp.DeviceArray.from_host(B, R), k, op, fill, unit, alpha, X, B.shape[1], ldx)
    assert out is X
    return X.to_host().reshape(-1, ldx)


def assert_padding_untouched(X, k):
    R = X.dtype
    assert (X[:, k:].view(SENTINEL[R].dtype) == SENTINEL[R]).all(), "the padding columns of X were written"


def set_lanes(monkeypatch, w):
    if w is None:
        monkeypatch.delenv("BMSP_SPSM_LANES", raising=False)
    else:
        monkeypatch.setenv("BMSP_SPSM_LANES", str(w))


def default_lanes(k):
    return 8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64


# ---------------------------------------------------------------------------------------------------------
# 1. bits against the helper, under every chain setting
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", MATRICES + SMALL)
def test_bits_match_the_helper_under_every_chain_setting(bmsp, monkeypatch, name, dtype, lay):
    k, ldb, ldx = 5, 7, 6
    for op, fill, unit in COMBOS:
        n, r, c, v, A = case(bmsp, name, dtype, lay, op, fill, unit)
        B = make_B(n, k, ldb, dtype)
        want = wanted(n, r, c, v, dtype, op, fill, unit, 1.0, B, k)
        assert np.isfinite(want).all()
        for chain in CHAINS:
            set_chain(monkeypatch, chain)
            A.invalidate(True)      # the switch is read when a plan is built
            X = solve(bmsp, A, B, k, ldx, op, fill, unit, 1.0, dtype)
            assert_same_bits(X[:, :k], want, "%s op %s %s unit %s chain %s" % (name, op, fill, unit, chain))
            assert_padding_untouched(X, k)


# ---------------------------------------------------------------------------------------------------------
# 2. every width, chunked and ragged columns; launch info
# ---------------------------------------------------------------------------------------------------------
KS = ((1, 2), (9, 9), (33, 33), (70, 70))       # (k, leading dimension of both): k = 1 with ld 2 is not the hand-off


@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 2])
@pytest.mark.parametrize("name", ["ragged203", "rmat10", "dense9"])
def test_every_width_with_chunked_and_ragged_columns(bmsp, monkeypatch, name, dtype, lay):
    kmax = max(k for k, _ in KS)
    for op, fill, unit in COMBOS:
        n, r, c, v, A = case(bmsp, name, dtype, lay, op, fill, unit)
        want = wanted(n, r, c, v, dtype, op, fill, unit, -1.5, make_B(n, kmax, kmax, dtype), kmax)
        plan = bmsp.spsv_analyse(A, op, fill, unit)
        for w in (8, 16, 32, 64, None):
            set_lanes(monkeypatch, w)
            for k, ld in KS:
                X = solve(bmsp, A, make_B(n, k, ld, dtype), k, ld, op, fill, unit, -1.5, dtype)
                assert_same_bits(X[:, :k], want[:, :k], "%s op %s %s unit %s W %s k %d" % (name, op, fill, unit, w, k))
                assert_padding_untouched(X, k)
                info = bmsp.spsm_launch_info(A, op, fill, k, unit, ld, ld)
                lanes = w or default_lanes(k)
                assert info["lanes"] == lanes and info["col_chunks"] == -(-k // lanes), (info, w, k)
                assert info["kernel"] == plan["kernel"].replace("spsv_level_kernel", "spsm_level_kernel").replace(">", ", %d>" % lanes), info
                for key in ("levels", "launches", "chain_launches", "chained_levels", "plan_bytes"):
                    assert info[key] == plan[key], (key, info, plan)
    set_lanes(monkeypatch, 64)
    assert bmsp.spsm_launch_info(A, op, fill, 70)["col_chunks"] == 2          # a last chunk of 6 columns
    set_lanes(monkeypatch, 8)
    assert bmsp.spsm_launch_info(A, op, fill, 70)["col_chunks"] == 9
    set_lanes(monkeypatch, 7)                                                 # not a width: the default rule
    assert bmsp.spsm_launch_info(A, op, fill, 70)["lanes"] == 64


# ---------------------------------------------------------------------------------------------------------
# 3. differential against bmsp_spsv on the device; columns do not mix
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_every_column_is_the_single_vector_solve_and_columns_do_not_mix(bmsp, dtype, lay):
    R = VEC[dtype]
    k = 33
    for name in ("rmat10", "ragged203"):
        for op, fill, unit in COMBOS:
            n, r, c, v, A = case(bmsp, name, dtype, lay, op, fill, unit)
            clean = make_B(n, k, k, dtype)
            B = clean.copy()
            B[:, 3] = np.nan
            B[0, 17] = np.inf
            B[:, 32] = (B[:, 32] * R(np.finfo(R).tiny) * R(0.25)).astype(R)       # a subnormal right-hand side
            assert (np.abs(B[:, 32]) < np.finfo(R).tiny).all() and (B[:, 32] != 0).all()
            X = solve(bmsp, A, B, k, k, op, fill, unit, 1.0, dtype)
            Xc = solve(bmsp, A, clean, k, k, op, fill, unit, 1.0, dtype)
            for j in range(k):
                x = bmsp.spsv(A, bmsp.DeviceArray.from_host(np.ascontiguousarray(B[:, j]), R), op, fill, unit).to_host()
                assert_same_bits(X[:, j], x, "%s op %s %s unit %s column %d" % (name, op, fill, unit, j))
                if j not in (3, 17, 32):
                    assert np.isfinite(X[:, j]).all()
                    assert_same_bits(X[:, j], Xc[:, j], "column %d is not its clean solve" % j)
            assert np.isnan(X[:, 3]).all()
            assert not np.isfinite(X[0, 17])
            assert (X[:, 32] != 0).any()


# ---------------------------------------------------------------------------------------------------------
# 4. what is not read
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", ["ragged203", "rmat10", "dense9"])
def test_the_other_triangle_a_unit_diagonal_and_the_padding_of_b_are_never_read(bmsp, name, dtype, lay):
    k, ldb, ldx = 5, 8, 5
    for op, fill, unit in COMBOS:
        n, r, c, v = values(name, dtype, op, fill, unit)
        read = (r > c) if fill == "lower" else (r < c)
        if not unit:
            read = read | (r == c)
        poisoned = np.where(read, v, np.nan)
        B = make_B(n, k, ldb, dtype)                         # (its padding is NaN)
        got = solve(bmsp, build(bmsp, n, r, c, poisoned, lay, dtype), B, k, ldx, op, fill, unit, 1.0, dtype)
        assert not np.isnan(got).any()
        assert_same_bits(got, wanted(n, r, c, v, dtype, op, fill, unit, 1.0, B, k), "%s op %s %s unit %s" % (name, op, fill, unit))


# ---------------------------------------------------------------------------------------------------------
# 5. what is not written; in place
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("k", [5, 19])
def test_nothing_else_is_written_and_in_place(bmsp, dtype, lay, k):
    R = np.dtype(VEC[dtype])
    U = SENTINEL[R].dtype
    name = "ragged203"                                        # n = 203: the last block-row has three rows that do not exist
    ldx, guard, extra = k + 3, 64, 8
    for op, fill, unit in COMBOS:
        n, r, c, v, A = case(bmsp, name, dtype, lay, op, fill, unit)
        B = make_B(n, k, k + 1, dtype)
        want = wanted(n, r, c, v, dtype, op, fill, unit, 1.0, B, k)
        dB = bmsp.DeviceArray.from_host(B, R)
        total = guard + (n + extra) * ldx + guard
        whole = bmsp.DeviceArray.from_host(sentinel(total, R), R)
        X = bmsp.DeviceArray((n + extra) * ldx, R, ptr=whole.ptr + guard * R.itemsize, owner=whole)
        assert bmsp.spsm(A, dB, k, op, fill, unit, 1.0, X, k + 1, ldx) is X
        out = whole.to_host()
        assert (out[:guard].view(U) == SENTINEL[R]).all() and (out[-guard:].view(U) == SENTINEL[R]).all()
        body = out[guard:-guard].reshape(n + extra, ldx)
        assert (body[n:].view(U) == SENTINEL[R]).all(), "a row at or beyond n was written"
        assert (body[:n, k:].view(U) == SENTINEL[R]).all(), "the padding columns of X were written"
        assert_same_bits(body[:n, :k], want, "op %s %s unit %s" % (op, fill, unit))
        assert_same_bits(dB.to_host().reshape(n, k + 1)[:, :k], B[:, :k])        # B is only read
        # in place: X is B, same stride; B's NaN padding stays what it was
        assert bmsp.spsm(A, dB, k, op, fill, unit, 1.0, dB, k + 1, k + 1) is dB
        inp = dB.to_host().reshape(n, k + 1)
        assert_same_bits(inp[:, :k], want)
        assert np.isnan(inp[:, k:]).all()
        # in place with different strides is refused, by the wrapper and by the library
        with pytest.raises(ValueError, match="in place"):
            bmsp.spsm(A, dB, k, op, fill, unit, 1.0, dB, k + 1, k)
        L = bmsp.lib()
        assert L.bmsp_spsm(A.h, 0, 0, int(unit), 1.0, dB.ptr, k + 1, dB.ptr, k, k, None) == -1
        assert "ldx" in L.bmsp_last_error().decode() and "in place" in L.bmsp_last_error().decode()


# ---------------------------------------------------------------------------------------------------------
# 6. edges
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_no_entries_no_rows_and_the_hand_off(bmsp, dtype):
    R = VEC[dtype]
    e = np.zeros(0, np.int64)
    k = 5
    for lay in (0, 1):
        A = build(bmsp, 13, e, e, np.zeros(0), lay, dtype)      # nnz = 0: under a unit diagonal X = fl(alpha B), every row written
        B = make_B(13, k, 7, dtype)
        for op in OPS:
            for fill in FILLS:
                X = solve(bmsp, A, B, k, 6, op, fill, True, -1.5, dtype)
                assert_same_bits(X[:, :k], (R(-1.5) * B[:, :k]).astype(R))
                assert_padding_untouched(X, k)
                info = bmsp.spsm_launch_info(A, op, fill, k, True, 7, 6)
                assert info["levels"] == 1 and info["launches"] == 1 and info["lanes"] == 8 and info["col_chunks"] == 1, info
        Z = build(bmsp, 0, e, e, np.zeros(0), lay, dtype)
        for op in OPS:
            for unit in (False, True):
                X = bmsp.spsm(Z, bmsp.DeviceArray(0, R), k, op, "lower", unit)
                assert X.n == 0
                info = bmsp.spsm_launch_info(Z, op, "lower", k, unit)
                assert info["levels"] == 0 and info["launches"] == 0 and info["kernel"] == "none (empty matrix)", info
        # k = 1 with unit strides IS bmsp_spsv
        for op, fill, unit in COMBOS:
            n, r, c, v, A = case(bmsp, "rmat10", dtype, lay, op, fill, unit)
            b = rhs(n, dtype)
            info = bmsp.spsm_launch_info(A, op, fill, 1, unit)
            assert info["kernel"] == "bmsp_spsv: " + bmsp.spsv_analyse(A, op, fill, unit)["kernel"], info
            assert info["lanes"] == 8 and info["col_chunks"] == 1, info
            x = bmsp.spsm(A, bmsp.DeviceArray.from_host(b, R), 1, op, fill, unit).to_host()
            assert_same_bits(x, bmsp.spsv(A, bmsp.DeviceArray.from_host(b, R), op, fill, unit).to_host())
            assert_same_bits(x, reference(n, r, c, v, dtype, op, fill, unit, 1.0, b))
            assert bmsp.spsm_launch_info(A, op, fill, 1, unit, 2, 1)["kernel"].startswith("spsm_level_kernel<")


# ---------------------------------------------------------------------------------------------------------
# 7. plan sharing and updates
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 2])
def test_the_plan_is_shared_with_spsv_and_follows_its_life_cycle(bmsp, monkeypatch, dtype, lay):
    op, fill = ("T", "upper") if lay else ("N", "lower")
    k = 9
    set_chain(monkeypatch, None)
    n, r, c, v, A = case(bmsp, "rmat10", dtype, lay, op, fill, False)
    B = make_B(n, k, k, dtype)
    want = wanted(n, r, c, v, dtype, op, fill, False, 1.0, B, k)
    # the solve builds the plan; the analysis then finds it
    assert_same_bits(solve(bmsp, A, B, k, k, op, fill, False, 1.0, dtype), want)
    plan = bmsp.spsv_analyse(A, op, fill)
    assert plan["levels"] > 1 and plan["plan_bytes"] == 4 * SHAPES["rmat10"][0] + 4 * (plan["levels"] + 1)
    assert bmsp.spsm_launch_info(A, op, fill, k)["plan_bytes"] == plan["plan_bytes"]
    # a value-only update in place is seen by the next call, without an invalidate, on the plan that was there
    set_chain(monkeypatch, "0")                                 # (a rebuilt plan would show: it would not chain)
    A.scale_(left=bmsp.DeviceArray.from_host(np.full(n, 2.0, VEC[dtype])))
    want2 = wanted(n, r, c, 2.0 * v, dtype, op, fill, False, 1.0, B, k)
    assert_same_bits(solve(bmsp, A, B, k, k, op, fill, False, 1.0, dtype), want2)
    assert bmsp.spsv_analyse(A, op, fill) == plan
    # invalidate(True) under the new switch: another plan, the same bits
    A.invalidate(True)
    assert_same_bits(solve(bmsp, A, B, k, k, op, fill, False, 1.0, dtype), want2)
    rebuilt = bmsp.spsv_analyse(A, op, fill)
    assert rebuilt["chain_launches"] == 0 and rebuilt["launches"] == rebuilt["levels"] == plan["levels"]
    assert bmsp.spsm_launch_info(A, op, fill, k)["launches"] == rebuilt["launches"]


# ---------------------------------------------------------------------------------------------------------
# 8. streams
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,lay", [("N", 0), ("T", 0), ("N", 1)])
def test_on_a_gated_stream(bmsp, op, lay):
    import stream_gate as G
    k = 9
    n, r, c, v, A = case(bmsp, "rmat10", 0, lay, op, "lower", False)
    hB = make_B(n, k, k, 0)
    want = wanted(n, r, c, v, 0, op, "lower", False, 1.0, hB, k)
    B = bmsp.DeviceArray.from_host(hB)
    bmsp.spsv_analyse(A, op, "lower")                  # the plan exists from here on: spsm builds nothing
    X = bmsp.DeviceArray.from_host(np.zeros(n * k, np.float32))
    bmsp.synchronize()
    st, side = G.new_stream(), G.Side()
    gate = G.Gate()
    try:
        gate.close(st)
        bmsp.spsm(A, B, k, op, "lower", X=X, stream=st.value)
        closed = gate.is_closed()                      # the call came back while the gate held the stream
        held = side.read(X.ptr, n * k, np.float32)
        still = gate.is_closed()
        gate.finish()
        assert closed, "bmsp_spsm did not return while the gate was closed"
        if still:
            assert not held.any()                      # nothing ran ahead of the gate
        assert_same_bits(X.to_host().reshape(n, k), want)
        # on a fresh handle the call builds the plan, which synchronises the stream: it returns only after the gate's timeout
        F = build(bmsp, n, r, c, v, lay, 0)
        bmsp.synchronize()
        gate2 = G.Gate()
        gate2.close(st)
        bmsp.spsm(F, B, k, op, "lower", X=X, stream=st.value)
        assert gate2.opened_by_timeout(), "bmsp_spsm returned before the stream was drained"
        gate2.finish()
        assert_same_bits(X.to_host().reshape(n, k), want)
    finally:
        gate.finish()
        side.close()
        G.destroy_stream(st)


# ---------------------------------------------------------------------------------------------------------
# 9. refusals on real handles; the C++ wrappers
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
def test_refusals_on_real_handles(bmsp, lay):
    k = 4
    n, r, c, v = values("ragged203", 0, "N", "lower", False)
    B = bmsp.DeviceArray.from_host(make_B(n, k, k, 0))
    L = bmsp.lib()
    info = bmsp.SpsmInfo()
    import ctypes as C
    gone = 202                     # in the ragged last block, whose rows 203 .. 207 do not exist and must not count
    keep = ~((r == gone) & (c == gone))
    A = build(bmsp, n, r[keep], c[keep], v[keep], lay, 0)
    for op in OPS:
        for fill in FILLS:
            refused(bmsp, lambda: bmsp.spsm(A, B, k, op, fill), "diag", "row %d " % gone)
            refused(bmsp, lambda: bmsp.spsm_launch_info(A, op, fill, k), "diag", "row %d " % gone)
            with pytest.raises(bmsp.BmspError) as e1:
                bmsp.spsv(A, B, op, fill)
            with pytest.raises(bmsp.BmspError) as e2:
                bmsp.spsm(A, B, k, op, fill)
            assert str(e1.value) == str(e2.value)              # the same message as bmsp_spsv's
            assert bmsp.spsm_launch_info(A, op, fill, k, True)["levels"] == 26      # the unit solve of the same handle works
    full = build(bmsp, n, r, c, v, lay, 0)
    assert L.bmsp_spsm(full.h, 0, 0, 0, 1.0, None, k, B.ptr, k, k, None) == -1 and "d_B" in L.bmsp_last_error().decode()
    assert L.bmsp_spsm(full.h, 0, 0, 0, 1.0, B.ptr, k, None, k, k, None) == -1 and "d_X" in L.bmsp_last_error().decode()
    assert L.bmsp_spsm_launch_info(full.h, 0, 0, 0, k, k, k, None, None) == -1 and "info" in L.bmsp_last_error().decode()
    assert L.bmsp_spsm(full.h, 0, 0, 0, 1.0, None, k - 1, None, k, k, None) == -1 and L.bmsp_last_error().decode().startswith("ldb")
    # not square
    e = np.arange(8)
    W = bmsp.BmSpMatrix.from_coo(8, 16, e, e, np.ones(8), transposed=bool(lay))
    refused(bmsp, lambda: bmsp.spsm_launch_info(W, "N", "lower", k), "square")
    assert L.bmsp_spsm(W.h, 0, 0, 1, 1.0, B.ptr, k, B.ptr, k, k, None) == -1 and "square" in L.bmsp_last_error().decode()
    # a row-panel view
    if not lay:
        P = full.row_panel(1, 13)
        refused(bmsp, lambda: bmsp.spsm_launch_info(P, "N", "lower", k, True), "row-panel view")
        assert L.bmsp_spsm(P.h, 0, 0, 1, 1.0, B.ptr, k, B.ptr, k, k, None) == -1 and "row-panel view" in L.bmsp_last_error().decode()
        assert L.bmsp_spsm_launch_info(P.h, 0, 0, 1, k, k, k, None, C.byref(info)) == -1 and "row-panel view" in L.bmsp_last_error().decode()


def test_cpp_wrapper_runs(bmsp, tmp_path):
    """tests/cpp_spsm_check.cpp: bmSparse_SpSM and bmSparse_SpSM_launch_info for float, half and double on a fixture written here"""
    n, r, c, v = values("ragged203", 1, "N", "lower", False)
    v = np.where(r == c, np.sign(v) * 64.0, v)          # (one diagonal for every triangle and op: larger than any row or column sum)
    mtx = tmp_path / "tri.mtx"
    with open(mtx, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n, r.size))
        for i, j, a in zip(r, c, v):
            f.write("%d %d %.17g\n" % (i + 1, j + 1, a))
    exe = str(tmp_path / "cpp_spsm_check")
    build_cpp_spsm_check(exe)
    out = subprocess.run([exe, str(mtx)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("OK") == 3 and "FAIL" not in out.stdout, out.stdout
