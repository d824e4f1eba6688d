"""GPU tests of bmsp_matrix_ilu0 / bmsp_matrix_ilu0_values: the incomplete factorisation ILU(0) by fixed-point sweeps, for both tile layouts
of A and of F, F32 / F16 / F64, one and eight lanes per tile, bit for bit against tests/ilu0_ref.c (the sweep and the sequential
factorisation as row loops with fmaf / fma, one division below the diagonal, fp16 storage rounding by its own routine).  There is no
tolerance anywhere: the call fixes its arithmetic, its statistics are order-independent, and the stop rule is evaluated in the arithmetic
type.  The matrices, their values and the reference live in tests/test_ilu0_api.py, where the CPU tests establish what these cases rely
on: the reference reaches the sequential factor within 2n sweeps with every iterate finite.

The file is named to be collected last: every GPU test that was there before it keeps its place in the order of the suite."""
import subprocess
import numpy as np
import pytest
from test_spsv_api import NP, VEC, rhs, reference, assert_same_bits
from test_ilu0_api import NAMES, NO_CHECK, ilu_values, csr_of, ref_sweeps, fixed_point, build_cpp_ilu0_check
from test_spsv import build, refused
from test_transpose import snapshot, assert_unchanged

pytestmark = pytest.mark.gpu

TOLS = (2.0 ** -10, 2.0 ** -20)
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]           # (layout of A, layout of F)
DT = ("F32", "F16", "F64")


def set_env(monkeypatch, var, value):
    if value is None:
        monkeypatch.delenv(var, raising=False)
    else:
        monkeypatch.setenv(var, value)


def stored(F, dtype):
    """F's values on the host in (row, col) order -- the reference's CSR order -- in the arithmetic type (fp16 widened exactly)"""
    r, c, v = F.to_coo()
    n = max(F.num_rows, 1)
    o = np.argsort(r.astype(np.int64) * n + c, kind="stable")
    return np.ascontiguousarray(v[o].astype(NP[dtype]).astype(VEC[dtype]))


def same_history(got, want, dtype):
    assert got.dtype == np.float64 and got.shape == want.shape, (got.shape, want.shape)
    assert_same_bits(got.astype(VEC[dtype]), want)
    assert np.array_equal(got, want.astype(np.float64))       # widened exactly


def same_structure(F, G):
    for x, y in zip(F.host_arrays()[:3], G.host_arrays()[:3]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(F.block_row_ptr(), G.block_row_ptr())


# ---------------------------------------------------------------------------------------------------------
# 1. until nothing changes: the sequential factor
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_until_nothing_changes_gives_the_sequential_factor(bmsp, monkeypatch, name, dtype):
    set_env(monkeypatch, "BMSP_ILU0_CHECK", None)
    n, r, c, v = ilu_values(name, dtype)
    seq, (_, ws, wc, wd, wf, _, _) = fixed_point(name, dtype)
    mats = {lay: build(bmsp, n, r, c, v, lay, dtype) for lay in (0, 1)}
    for la, lf in LAYOUTS:
        for lanes in (None, "1", "8"):
            set_env(monkeypatch, "BMSP_ILU0_LANES", lanes)
            F, info, hist = bmsp.ilu0(mats[la], out_transposed=lf, history=True)
            msg = "%s A %d F %d lanes %s" % (name, la, lf, lanes)
            assert_same_bits(stored(F, dtype), seq, msg)
            assert (info["sweeps"], info["converged"], info["max_sweeps"]) == (ws, wc, 2 * n), (info, ws, msg)
            same_history(hist, wd, dtype)
            assert info["delta"] == 0.0 and info["fmax"] == float(wf[-1]), (info, msg)
            g = int(lanes or 8)
            assert info["lanes"] == g and info["kernel"] == "ilu0_sweep_kernel<%s, %d, STATS>" % (DT[dtype], g), info
            assert F.info()["transposed"] == lf and info["view_bytes"] > 0


# ---------------------------------------------------------------------------------------------------------
# 2. a fixed number of sweeps without a check
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_no_check_runs_exactly_m_sweeps_of_the_reference(bmsp, name, dtype):
    n, r, c, v = ilu_values(name, dtype)
    S = csr_of(name)
    seq, _ = fixed_point(name, dtype)
    mats = {lay: build(bmsp, n, r, c, v, lay, dtype) for lay in (0, 1)}
    for k, m in enumerate((1, 2, 3, 5)):
        want, ws, *_ = ref_sweeps(S, v, dtype, m, NO_CHECK)
        assert ws == m
        for la, lf in (LAYOUTS[k], LAYOUTS[3 - k]):
            F, info = bmsp.ilu0(mats[la], max_iter=m, tol=NO_CHECK, out_transposed=lf)
            assert_same_bits(stored(F, dtype), want, "%s A %d F %d m %d" % (name, la, lf, m))
            assert (info["sweeps"], info["max_sweeps"], info["converged"], info["delta"], info["fmax"]) == (m, m, 0, -1.0, -1.0), info
            assert info["kernel"] == "ilu0_sweep_kernel<%s, 8, NO_STATS>" % DT[dtype], info
            # the same sweeps into the existing F: from A's values again, and an odd and an even number of them end in F's array
            G, info = bmsp.ilu0_values(mats[la], F, max_iter=m, tol=NO_CHECK)
            assert G is F and info["sweeps"] == m
            assert_same_bits(stored(F, dtype), want)
    # max_iter = 0 means 2n: the fixed point, unchecked
    F, info = bmsp.ilu0(mats[dtype % 2], max_iter=0, tol=NO_CHECK, out_transposed=(dtype + 1) % 2)
    assert (info["sweeps"], info["max_sweeps"], info["converged"]) == (2 * n, 2 * n, 0), info
    assert_same_bits(stored(F, dtype), seq, name)


# ---------------------------------------------------------------------------------------------------------
# 3. the tolerance, and max_iter below the stopping point
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_tolerance_stops_where_the_reference_stops(bmsp, monkeypatch, name, dtype):
    set_env(monkeypatch, "BMSP_ILU0_CHECK", None)
    n, r, c, v = ilu_values(name, dtype)
    S = csr_of(name)
    mats = {lay: build(bmsp, n, r, c, v, lay, dtype) for lay in (0, 1)}
    for k, tol in enumerate(TOLS):
        want, ws, wc, wd, wf, wch, _ = ref_sweeps(S, v, dtype, 2 * n, tol)
        assert wc == 1
        for la, lf in (LAYOUTS[k], LAYOUTS[3 - k]):
            msg = "%s A %d F %d tol %g" % (name, la, lf, tol)
            F, info, hist = bmsp.ilu0(mats[la], tol=tol, out_transposed=lf, history=True)
            assert (info["sweeps"], info["converged"]) == (ws, wc), (info, ws, msg)
            assert_same_bits(stored(F, dtype), want, msg)
            same_history(hist, wd, dtype)
            assert info["delta"] == float(wd[-1]) and info["fmax"] == float(wf[-1]), (info, msg)
            # one sweep fewer than the reference needs: not converged, and the reference's iterate after that many
            if ws >= 2:
                want1, ws1, wc1, wd1, *_ = ref_sweeps(S, v, dtype, ws - 1, tol)
                assert (ws1, wc1) == (ws - 1, 0)
                F, info, hist = bmsp.ilu0(mats[la], max_iter=ws - 1, tol=tol, out_transposed=lf, history=True)
                assert (info["sweeps"], info["converged"], info["max_sweeps"]) == (ws - 1, 0, ws - 1), (info, msg)
                assert_same_bits(stored(F, dtype), want1, msg)
                same_history(hist, wd1, dtype)


# ---------------------------------------------------------------------------------------------------------
# 4. the read-back interval decides nothing
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", ["ragged203", "rmat10", "dense17"])
def test_check_interval_changes_nothing(bmsp, monkeypatch, name, dtype):
    n, r, c, v = ilu_values(name, dtype)
    A = build(bmsp, n, r, c, v, dtype % 2, dtype)
    for tol, max_iter in ((0.0, 0), (TOLS[0], 0), (TOLS[1], 4), (0.0, 3)):
        runs = []
        for check in (None, "1", "3", "8", str(1 << 31)):
            set_env(monkeypatch, "BMSP_ILU0_CHECK", check)
            F, info, hist = bmsp.ilu0(A, max_iter=max_iter, tol=tol, out_transposed=1, history=True)
            runs.append((stored(F, dtype), info, hist))
        for f, info, hist in runs[1:]:
            assert_same_bits(f, runs[0][0], "%s tol %g max_iter %d" % (name, tol, max_iter))
            assert info == runs[0][1], (info, runs[0][1])
            assert np.array_equal(hist, runs[0][2])
    # a value that does not parse, or below 1, is the default
    for check in ("x", "0", "-3"):
        set_env(monkeypatch, "BMSP_ILU0_CHECK", check)
        F, info, hist = bmsp.ilu0(A, max_iter=max_iter, tol=tol, out_transposed=1, history=True)
        assert_same_bits(stored(F, dtype), runs[0][0])
        assert info == runs[0][1]


# ---------------------------------------------------------------------------------------------------------
# 5. the initial iterate
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", ["ragged203", "fem8", "dense9"])
def test_initial_iterate_and_warm_start(bmsp, name, dtype):
    R = VEC[dtype]
    n, r, c, v = ilu_values(name, dtype)
    S = csr_of(name)
    seq, _ = fixed_point(name, dtype)
    left = np.array([0.5, 1.0, 2.0])[np.arange(n) % 3]                 # powers of two: F^0 = diag(left) * A exactly, in every dtype
    for la, lf in LAYOUTS:
        A = build(bmsp, n, r, c, v, la, dtype)
        msg = "%s A %d F %d" % (name, la, lf)
        # a given F^0: the reference started from it, checked and unchecked
        f0 = v * left[r]
        for tol, m in ((0.0, 0), (TOLS[0], 0), (NO_CHECK, 1), (NO_CHECK, 2), (NO_CHECK, 3)):
            F = A.scale(left=bmsp.DeviceArray.from_host(left, R), transposed=lf)
            assert_same_bits(stored(F, dtype), f0.astype(R))
            want, ws, wc, wd, *_ = ref_sweeps(S, v, dtype, m or 2 * n, tol, f0=f0)
            if tol == NO_CHECK:
                _, info = bmsp.ilu0_values(A, F, max_iter=m, tol=tol, f0_given=True)
            else:
                _, info, hist = bmsp.ilu0_values(A, F, max_iter=m, tol=tol, history=True, f0_given=True)
                same_history(hist, wd, dtype)
            assert (info["sweeps"], info["converged"]) == (ws, wc), (info, ws, wc, msg)
            assert_same_bits(stored(F, dtype), want, "%s tol %g m %d" % (msg, tol, m))
        # from the fixed point: one sweep, nothing changes
        F, _ = bmsp.ilu0(A, out_transposed=lf)
        _, info, hist = bmsp.ilu0_values(A, F, history=True, f0_given=True)
        assert (info["sweeps"], info["converged"], info["delta"]) == (1, 1, 0.0) and hist.tolist() == [0.0], info
        assert_same_bits(stored(F, dtype), seq)
        # without the flag a NaN-filled F is not read: F^0 = A's values
        for tol, m in ((NO_CHECK, 1), (NO_CHECK, 2), (TOLS[0], 0), (0.0, 0)):
            N = A.scale(left=bmsp.DeviceArray.from_host(np.full(n, np.nan), R), transposed=lf)
            assert np.isnan(stored(N, dtype)).all()
            _, info = bmsp.ilu0_values(A, N, max_iter=m, tol=tol)
            want, ws, *_ = ref_sweeps(S, v, dtype, m or 2 * n, tol)
            got = stored(N, dtype)
            assert not np.isnan(got).any() and info["sweeps"] == ws, (info, msg)
            assert_same_bits(got, want, msg)
        # a value-only update of A in place: the warm start from the old factor needs no invalidate
        A.scale_(left=bmsp.DeviceArray.from_host(np.full(n, 2.0), R))
        v2 = 2.0 * v
        want, ws, wc, wd, *_ = ref_sweeps(S, v2, dtype, 2 * n, 0.0, f0=seq)
        _, info, hist = bmsp.ilu0_values(A, F, history=True, f0_given=True)
        assert (info["sweeps"], info["converged"]) == (ws, wc), (info, ws, msg)
        same_history(hist, wd, dtype)
        assert_same_bits(stored(F, dtype), want, msg)
        assert ws > 1                                                    # (the new values do move the factor)


# ---------------------------------------------------------------------------------------------------------
# 6. nothing else is written; F's structure is a layout conversion's
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_a_is_unchanged_and_f_has_the_structure_of_a_layout_conversion(bmsp, dtype):
    for name in ("ragged203", "random2000"):
        n, r, c, v = ilu_values(name, dtype)
        for la, lf in LAYOUTS:
            A = build(bmsp, n, r, c, v, la, dtype)
            snap, rowptr = snapshot(A), A.block_row_ptr().copy()
            G = A.with_layout(lf)
            F, _ = bmsp.ilu0(A, out_transposed=lf)
            same_structure(F, G)
            for tol, m, given in ((NO_CHECK, 2, False), (TOLS[0], 0, True), (NO_CHECK, 3, True), (0.0, 0, False)):
                bmsp.ilu0_values(A, F, max_iter=m, tol=tol, f0_given=given)
                bmsp.ilu0_values(A, G, max_iter=m, tol=tol, f0_given=given)       # an F made by the layout conversion itself
            same_structure(F, G)
            assert_same_bits(stored(F, dtype), stored(G, dtype))
            assert_unchanged(A, snap)
            np.testing.assert_array_equal(A.block_row_ptr(), rowptr)


# ---------------------------------------------------------------------------------------------------------
# 7. special values
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", ["rmat10", "dense17"])
def test_nan_and_a_zero_pivot_follow_the_dependencies_only(bmsp, name, dtype):
    n, r, c, v = ilu_values(name, dtype)
    S = csr_of(name)
    off = np.flatnonzero(r != c)
    below = np.flatnonzero(r > c)
    k = int(c[below[below.size // 2]])                                # a pivot that some entry below it is divided by
    cases = []
    vn = v.copy()
    vn[off[off.size // 2]] = np.nan                                   # a stored NaN at one off-diagonal entry
    cases.append(vn)
    vz = v.copy()
    vz[(r == k) & (c == k)] = 0.0                                      # a stored zero pivot
    cases.append(vz)
    for vals in cases:
        for la, lf in LAYOUTS:
            A = build(bmsp, n, r, c, vals, la, dtype)
            for m in (1, 3, 6):
                F, info = bmsp.ilu0(A, max_iter=m, tol=NO_CHECK, out_transposed=lf)
                want, *_ = ref_sweeps(S, vals, dtype, m, NO_CHECK)
                got = stored(F, dtype)
                assert_same_bits(got, want, "%s A %d F %d m %d" % (name, la, lf, m))
                assert np.array_equal(np.isfinite(got), np.isfinite(want))
            assert not np.isfinite(want).all() and np.isfinite(want).any()      # (the special value spread, and not everywhere)


# ---------------------------------------------------------------------------------------------------------
# 8. empty cases
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_no_rows_the_diagonal_only_and_one_row(bmsp, dtype):
    e = np.zeros(0, np.int64)
    for la, lf in LAYOUTS:
        Z = build(bmsp, 0, e, e, np.zeros(0), la, dtype)
        for tol in (0.0, NO_CHECK):
            F, info = bmsp.ilu0(Z, tol=tol, out_transposed=lf)
            assert F.num_rows == 0 and F.nnz == 0 and F.block_num == 0 and F.info()["transposed"] == lf
            assert info["sweeps"] == 0 and info["kernel"] == "none (empty matrix)", info
            _, info = bmsp.ilu0_values(Z, F, tol=tol)
            assert info["sweeps"] == 0 and info["kernel"] == "none (empty matrix)", info
        for name in ("diag3001", "dense1"):
            n, r, c, v = ilu_values(name, dtype)
            A = build(bmsp, n, r, c, v, la, dtype)
            F, info, hist = bmsp.ilu0(A, out_transposed=lf, history=True)
            assert (info["sweeps"], info["converged"], info["delta"]) == (1, 1, 0.0) and hist.tolist() == [0.0], info
            assert_same_bits(stored(F, dtype), v.astype(VEC[dtype]))          # F == A
            F, info = bmsp.ilu0(A, max_iter=3, tol=NO_CHECK, out_transposed=lf)
            assert_same_bits(stored(F, dtype), v.astype(VEC[dtype]))


# ---------------------------------------------------------------------------------------------------------
# 9. end to end: the factor in the triangular solves
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", ["ragged203", "banded400", "rmat10", "dense9", "dense17"])
def test_the_factor_applied_by_the_triangular_solves(bmsp, name, dtype):
    R = VEC[dtype]
    n, r, c, v = ilu_values(name, dtype)
    seq, _ = fixed_point(name, dtype)
    b = rhs(n, dtype)
    fv = seq.astype(np.float64)
    y_ref = reference(n, r, c, fv, dtype, "N", "lower", True, 1.0, b)
    x_ref = reference(n, r, c, fv, dtype, "N", "upper", False, 1.0, y_ref)
    assert np.isfinite(x_ref).all()
    for la, lf in LAYOUTS:
        A = build(bmsp, n, r, c, v, la, dtype)
        F, _ = bmsp.ilu0(A, out_transposed=lf)
        y = bmsp.spsv(F, bmsp.DeviceArray.from_host(b, R), "N", "lower", True)
        x = bmsp.spsv(F, y, "N", "upper", False)
        assert_same_bits(y.to_host(), y_ref, name)
        assert_same_bits(x.to_host(), x_ref, name)
        # the iterative solve runs on F too and reaches the substitution's bits
        yi, info = bmsp.spitsv(F, bmsp.DeviceArray.from_host(b, R), "N", "lower", True)
        xi, info2 = bmsp.spitsv(F, yi, "N", "upper", False)
        assert info["converged"] == 1 and info2["converged"] == 1
        assert_same_bits(xi.to_host(), x_ref, name)
    # (on the dense patterns ILU(0) is LU: there these are the bits of a direct solve of A x = b without pivoting)


# ---------------------------------------------------------------------------------------------------------
# 10. streams
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("la,lf,m,given", [(0, 0, 3, False), (0, 0, 4, False), (0, 1, 3, False), (1, 0, 2, False), (1, 1, 3, True), (0, 0, 2, True)])
def test_no_check_on_a_gated_stream(bmsp, la, lf, m, given):
    """the last iterate in F's array or in the temporary (one device copy behind the sweeps); F^0 read from A, gathered from A, or given"""
    import stream_gate as G
    n, r, c, v = ilu_values("rmat10", 0)
    S = csr_of("rmat10")
    A = build(bmsp, n, r, c, v, la, 0)
    F, _ = bmsp.ilu0(A, max_iter=m, tol=NO_CHECK, out_transposed=lf)             # the view, the index and the temporary exist from here on
    null = stored(F, 0)
    assert_same_bits(null, ref_sweeps(S, v, 0, m, NO_CHECK)[0])
    vals = F.device_arrays()[3]
    if given:
        F.copy_values_from(A)                                                    # F^0 = A's values, given
    else:
        vals.zero()
    want = null
    start = vals.to_host().copy()
    bmsp.synchronize()
    st, side = G.new_stream(), G.Side()
    gate = G.Gate()
    try:
        gate.close(st)
        bmsp.ilu0_values(A, F, max_iter=m, tol=NO_CHECK, stream=st.value, f0_given=given)
        closed = gate.is_closed()                      # the call came back while the gate held the stream
        held = side.read(vals.ptr, vals.n, np.float32)
        still = gate.is_closed()
        gate.finish()
        assert closed, "bmsp_matrix_ilu0_values (BMSP_ILU_NO_CHECK) did not return while the gate was closed"
        if still:
            assert_same_bits(held, start)              # nothing ran ahead of the gate
        assert_same_bits(stored(F, 0), want)
    finally:
        gate.finish()
        side.close()
        G.destroy_stream(st)


# ---------------------------------------------------------------------------------------------------------
# 11. refusals on real handles; the C++ wrapper
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
def test_refusals_on_real_handles(bmsp, lay):
    n, r, c, v = ilu_values("ragged203", 0)
    L = bmsp.lib()
    full = build(bmsp, n, r, c, v, lay, 0)
    good, _ = bmsp.ilu0(full, out_transposed=1 - lay)
    before = stored(good, 0)

    def into(A, F, max_iter=0, tol=0.0, flags=0):
        return L.bmsp_matrix_ilu0_values(A.h, F.h, max_iter, tol, flags, None, None, None)

    # a missing diagonal, the first such row named: by both entry points, and nothing of F is written
    for gone in ((77,), (202,), (150, 77)):
        keep = ~np.isin(r, gone) | (r != c)
        A = build(bmsp, n, r[keep], c[keep], v[keep], lay, 0)
        for lf in (0, 1):
            refused(bmsp, lambda: bmsp.ilu0(A, out_transposed=lf), "matrix A", "row %d " % min(gone), "diagonal")
            refused(bmsp, lambda: bmsp.ilu0(A, max_iter=2, tol=NO_CHECK, out_transposed=lf), "row %d " % min(gone))
            G = A.with_layout(lf)
            held = stored(G, 0)
            refused(bmsp, lambda: bmsp.ilu0_values(A, G), "row %d " % min(gone))
            refused(bmsp, lambda: bmsp.ilu0_values(A, G, f0_given=True), "row %d " % min(gone))       # (the answer is cached on G)
            assert_same_bits(stored(G, 0), held)
    # a non-square A
    e = np.arange(8)
    W = bmsp.BmSpMatrix.from_coo(8, 16, e, e, np.ones(8), transposed=bool(lay))
    refused(bmsp, lambda: bmsp.ilu0(W), "square")
    refused(bmsp, lambda: bmsp.ilu0_values(W, W.with_layout(0)), "square")
    # a row-panel view
    if not lay:
        refused(bmsp, lambda: bmsp.ilu0(full.row_panel(1, 13)), "row-panel view")
    # F == A; an unrelated F of the same structure; an F made by transpose; an F of another dtype; A's structure changed since
    assert into(full, full) == -1 and "F is A" in L.bmsp_last_error().decode()
    with pytest.raises(ValueError):
        bmsp.ilu0_values(full, full)
    refused(bmsp, lambda: bmsp.ilu0_values(full, build(bmsp, n, r, c, v, lay, 0)), "matrix F", "not made from A")
    refused(bmsp, lambda: bmsp.ilu0_values(full, full.transpose(lay)), "matrix F", "not made from A")
    assert into(full, good, max_iter=-1) == -1 and L.bmsp_last_error().decode().startswith("max_iter")
    assert into(full, good, flags=6) == -1 and L.bmsp_last_error().decode().startswith("flags")
    assert_same_bits(stored(good, 0), before)                     # nothing was done on the device
    bmsp.ilu0_values(full, good)
    full.invalidate(True)
    refused(bmsp, lambda: bmsp.ilu0_values(full, good), "matrix F", "structure changed")
    assert_same_bits(stored(good, 0), before)


def test_cpp_wrapper_runs(bmsp, tmp_path):
    """tests/cpp_ilu0_check.cpp: bmSparse_ILU0 / bmSparse_ILU0_values for float, half and double on a fixture written here"""
    n, r, c, v = ilu_values("ragged203", 1)
    mtx = tmp_path / "ilu.mtx"
    with open(mtx, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n, r.size))
        for i, j, a in zip(r, c, v):
            f.write("%d %d %.17g\n" % (i + 1, j + 1, a))
    exe = str(tmp_path / "cpp_ilu0_check")
    build_cpp_ilu0_check(exe)
    out = subprocess.run([exe, str(mtx)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("OK") == 3 and "FAIL" not in out.stdout, out.stdout


# ---------------------------------------------------------------------------------------------------------
# 12. F's value-derived caches
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("lay", [0, 1])
def test_a_product_with_f_after_new_values_reads_no_stale_cache(bmsp, dtype, lay):
    """in the style of tests/test_value_cache_coherence.py: F is prepared as a SpGEMM operand and multiplied (its value-derived caches
    exist), bmsp_matrix_ilu0_values rewrites its values, and a product with F must equal that of a handle adopted from copies of F's four
    arrays, which has no cache -- in all four arrays"""
    n, r, c, v = ilu_values("banded400", dtype)
    A = build(bmsp, n, r, c, v, lay, dtype)
    P = build(bmsp, n, r, c, np.abs(v), 1, dtype)                     # the right operand, column-major
    F = A.with_layout(0)                                              # F^0 = A's values: the product below caches what it derives from them
    F.prepare(3)
    P.prepare(3)
    old, _ = bmsp.spgemm(F, P)
    old = [x.copy() for x in old.host_arrays()]
    bmsp.ilu0_values(A, F)
    got, _ = bmsp.spgemm(F, P)
    fresh = F.clone()
    want, _ = bmsp.spgemm(fresh, P)
    for x, y in zip(got.host_arrays(), want.host_arrays()):
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))
    assert not np.array_equal(got.host_arrays()[3].view(np.uint8), old[3].view(np.uint8))      # (stale values would have shown)
