"""GPU tests of bmsp_spitsv: block-Jacobi sweeps towards the x of op(tri(A)) x = alpha b, for both tile layouts, both ops, both triangles
and both kinds of diagonal, F32 / F16 / F64, bit for bit against tests/spitsv_ref.c (a row loop of sweeps with fmaf / fma whose x comes from
the new vector inside the row's block of eight) and, at the fixed point, against bmsp_spsv and tests/spsv_ref.c.  There is no tolerance
anywhere: the call fixes its arithmetic, its statistics are order-independent, and the stop rule is evaluated in the vector type.  The
matrices and their values are those of tests/test_spsv_api.py; the reference lives in tests/test_spitsv_api.py.

The file is named to be collected last: every GPU test that was there before it keeps its place in the order of the suite."""
import subprocess
import numpy as np
import pytest
from test_spsv_api import MATRICES, SMALL, NP, VEC, values, rhs, reference, assert_same_bits
from test_spitsv_api import COMBOS, NO_CHECK, ref_sweeps, plan_levels, build_cpp_spitsv_check
from test_spsv import build, case, solve, dependants, refused
from test_transpose import snapshot, assert_unchanged

pytestmark = pytest.mark.gpu

TOLS = (2.0 ** -10, 2.0 ** -20)
STOP_EARLY = ("ragged203", "banded400", "fem8", "rmat10")     # the reference stops before `levels` on these, at both tolerances


def set_check(monkeypatch, check):
    if check is None:
        monkeypatch.delenv("BMSP_SPITSV_CHECK", raising=False)
    else:
        monkeypatch.setenv("BMSP_SPITSV_CHECK", check)


def sweep(bmsp, A, b, op, fill, unit, dtype, alpha=1.0, max_iter=0, tol=0.0, x0=None, history=False, stream=None):
    """(x on the host, info[, history]) of one bmsp_spitsv call; x0 = the initial iterate (BMSP_ITSV_X0_GIVEN) or None"""
    R = VEC[dtype]
    dx = None if x0 is None else bmsp.DeviceArray.from_host(x0, R)
    out = bmsp.spitsv(A, bmsp.DeviceArray.from_host(b, R), op, fill, unit, alpha, max_iter, tol, dx, x0 is not None, history, stream)
    return (out[0].to_host(),) + tuple(out[1:])


def same_history(got, want, dtype):
    assert got.dtype == np.float64 and got.shape == want.shape, (got.shape, want.shape)
    assert_same_bits(got.astype(VEC[dtype]), want)
    assert np.array_equal(got, want.astype(np.float64))       # widened exactly


# ---------------------------------------------------------------------------------------------------------
# 1. the fixed point is bmsp_spsv's x
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", MATRICES + SMALL)
def test_until_nothing_changes_gives_the_bits_of_spsv(bmsp, monkeypatch, name, dtype, lay):
    set_check(monkeypatch, None)
    for op, fill, unit in COMBOS:
        n, r, c, v, A = case(bmsp, name, dtype, lay, op, fill, unit)
        b = rhs(n, dtype)
        levels = plan_levels(bmsp, n, r, c, op, fill)
        x, info, hist = sweep(bmsp, A, b, op, fill, unit, dtype, history=True)
        msg = "%s op %s %s unit %s" % (name, op, fill, unit)
        assert_same_bits(x, solve(bmsp, A, b, op, fill, unit, 1.0, dtype), msg)
        assert_same_bits(x, reference(n, r, c, v, dtype, op, fill, unit, 1.0, b), msg)
        assert info["converged"] == 1 and 1 <= info["sweeps"] <= levels + 1 and info["levels"] == levels, (info, msg)
        assert info["delta"] == 0.0 and hist.size == info["sweeps"] and hist[-1] == 0.0, (info, hist)
        _, ws, wc, wd, wx, _ = ref_sweeps(n, r, c, v, dtype, op, fill, unit, 1.0, b, levels + 1, 0.0)
        assert (info["sweeps"], info["converged"]) == (ws, wc), (info, ws, msg)
        same_history(hist, wd, dtype)
        assert info["xmax"] == float(wx[-1])
        minor = (op == "T") != bool(lay)
        assert info["kernel"] == "spitsv_sweep_kernel<%s, %s, %s, %s, STATS>" % (
            ("F32", "F16", "F64")[dtype], "MINOR" if minor else "MAJOR", "LOWER" if (fill == "lower") != (op == "T") else "UPPER",
            "UNIT" if unit else "NON_UNIT"), info


# ---------------------------------------------------------------------------------------------------------
# 2. a fixed number of sweeps without a check
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", MATRICES + SMALL)
def test_no_check_runs_exactly_m_sweeps_of_the_reference(bmsp, name, dtype, lay):
    for op, fill, unit in COMBOS:
        n, r, c, v, A = case(bmsp, name, dtype, lay, op, fill, unit)
        b = rhs(n, dtype)
        levels = plan_levels(bmsp, n, r, c, op, fill)
        for m in sorted({1, 2, 3, max(1, levels // 2)}):
            x, info = sweep(bmsp, A, b, op, fill, unit, dtype, max_iter=m, tol=NO_CHECK)
            want, ws, *_ = ref_sweeps(n, r, c, v, dtype, op, fill, unit, 1.0, b, m, NO_CHECK)
            assert ws == m
            assert_same_bits(x, want, "%s op %s %s unit %s m %d" % (name, op, fill, unit, m))
            assert (info["sweeps"], info["converged"], info["delta"], info["xmax"], info["levels"]) == (m, 0, -1.0, -1.0, levels), info
            assert info["kernel"].endswith(", NO_STATS>"), info
    # max_iter = 0 means levels + 1: the substitution's bits, unchecked
    x, info = sweep(bmsp, A, b, op, fill, unit, dtype, max_iter=0, tol=NO_CHECK)
    assert info["sweeps"] == levels + 1 and info["converged"] == 0
    assert_same_bits(x, reference(n, r, c, v, dtype, op, fill, unit, 1.0, b))


# ---------------------------------------------------------------------------------------------------------
# 3. / 4. the tolerance, and max_iter below the stopping point
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", MATRICES + SMALL)
def test_tolerance_stops_where_the_reference_stops(bmsp, monkeypatch, name, dtype, lay):
    set_check(monkeypatch, None)
    for op, fill, unit in COMBOS:
        n, r, c, v, A = case(bmsp, name, dtype, lay, op, fill, unit)
        b = rhs(n, dtype)
        levels = plan_levels(bmsp, n, r, c, op, fill)
        for tol in TOLS:
            want, ws, wc, wd, wx, wch = ref_sweeps(n, r, c, v, dtype, op, fill, unit, 1.0, b, levels + 1, tol)
            msg = "%s op %s %s unit %s tol %g" % (name, op, fill, unit, tol)
            if name in STOP_EARLY:      # the tolerance is what stops these, not finite termination
                assert wc == 1 and ws < levels and wch[-1] == 1, (ws, levels, msg)
            x, info, hist = sweep(bmsp, A, b, op, fill, unit, dtype, tol=tol, history=True)
            assert (info["sweeps"], info["converged"]) == (ws, wc), (info, ws, wc, msg)
            assert_same_bits(x, want, msg)
            same_history(hist, wd, dtype)
            assert info["delta"] == float(wd[-1]) and info["xmax"] == float(wx[-1]), (info, msg)
            # one sweep fewer than the reference needs: not converged, and the reference's x after that many
            if ws >= 2:
                want1, ws1, wc1, wd1, *_ = ref_sweeps(n, r, c, v, dtype, op, fill, unit, 1.0, b, ws - 1, tol)
                assert (ws1, wc1) == (ws - 1, 0)
                x, info, hist = sweep(bmsp, A, b, op, fill, unit, dtype, max_iter=ws - 1, tol=tol, history=True)
                assert (info["sweeps"], info["converged"]) == (ws - 1, 0), (info, msg)
                assert_same_bits(x, want1, msg)
                same_history(hist, wd1, dtype)


# ---------------------------------------------------------------------------------------------------------
# 5. the read-back interval decides nothing
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", ["ragged203", "rmat10", "random2000", "dense9"])
def test_check_interval_changes_nothing(bmsp, monkeypatch, name, dtype, lay):
    for op, fill, unit in COMBOS:
        n, r, c, v, A = case(bmsp, name, dtype, lay, op, fill, unit)
        b = rhs(n, dtype)
        for tol, max_iter in ((0.0, 0), (TOLS[0], 0), (TOLS[1], 7), (0.0, 3)):
            runs = []
            for check in ("1", None, str(1 << 31)):
                set_check(monkeypatch, check)
                runs.append(sweep(bmsp, A, b, op, fill, unit, dtype, max_iter=max_iter, tol=tol, history=True))
            for x, info, hist in runs[1:]:
                assert_same_bits(x, runs[0][0], "%s op %s %s unit %s tol %g" % (name, op, fill, unit, tol))
                assert info == runs[0][1], (info, runs[0][1])
                assert np.array_equal(hist, runs[0][2])
    # a value that does not parse, or below 1, is the default
    for check in ("x", "0", "-3"):
        set_check(monkeypatch, check)
        x, info, hist = sweep(bmsp, A, b, op, fill, unit, dtype, max_iter=max_iter, tol=tol, history=True)
        assert_same_bits(x, runs[0][0])
        assert info == runs[0][1]


# ---------------------------------------------------------------------------------------------------------
# 6. the initial iterate
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", ["ragged203", "fem8", "dense5"])
def test_initial_iterate(bmsp, name, dtype, lay):
    R = VEC[dtype]
    rng = np.random.default_rng(17)
    for op, fill, unit in COMBOS:
        n, r, c, v, A = case(bmsp, name, dtype, lay, op, fill, unit)
        b = rhs(n, dtype)
        levels = plan_levels(bmsp, n, r, c, op, fill)
        exact = reference(n, r, c, v, dtype, op, fill, unit, 1.0, b)
        # from the exact solution: one sweep, nothing changes
        x, info, hist = sweep(bmsp, A, b, op, fill, unit, dtype, x0=exact, history=True)
        assert (info["sweeps"], info["converged"], info["delta"]) == (1, 1, 0.0) and hist.tolist() == [0.0], info
        assert_same_bits(x, exact)
        # from a random iterate: the reference, with and without a tolerance, and for a fixed number of sweeps
        x0 = (rng.uniform(-4.0, 4.0, n)).astype(R)
        for tol, m in ((0.0, 0), (TOLS[0], 0), (NO_CHECK, 1), (NO_CHECK, 2), (NO_CHECK, 3)):
            want, ws, wc, wd, *_ = ref_sweeps(n, r, c, v, dtype, op, fill, unit, 1.0, b, m or levels + 1, tol, x0=x0)
            if tol == NO_CHECK:
                x, info = sweep(bmsp, A, b, op, fill, unit, dtype, max_iter=m, tol=tol, x0=x0)
            else:
                x, info, hist = sweep(bmsp, A, b, op, fill, unit, dtype, max_iter=m, tol=tol, x0=x0, history=True)
                same_history(hist, wd, dtype)
            assert (info["sweeps"], info["converged"]) == (ws, wc), (info, ws, wc)
            assert_same_bits(x, want, "%s op %s %s unit %s tol %g m %d" % (name, op, fill, unit, tol, m))
        # without the flag a NaN-filled d_x is not read: x^0 = +0
        db = bmsp.DeviceArray.from_host(b, R)
        for tol, m in ((NO_CHECK, 1), (NO_CHECK, 2), (TOLS[0], 0)):
            dx = bmsp.DeviceArray.from_host(np.full(n, np.nan, R), R)
            _, info = bmsp.spitsv(A, db, op, fill, unit, 1.0, m, tol, dx)
            want, ws, *_ = ref_sweeps(n, r, c, v, dtype, op, fill, unit, 1.0, b, m or levels + 1, tol)
            got = dx.to_host()
            assert not np.isnan(got).any() and info["sweeps"] == ws
            assert_same_bits(got, want)


# ---------------------------------------------------------------------------------------------------------
# 7. what is not read
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", ["ragged203", "rmat10", "dense9"])
def test_the_other_triangle_and_a_unit_diagonal_are_never_read(bmsp, name, dtype, lay):
    for op, fill, unit in COMBOS:
        n, r, c, v = values(name, dtype, op, fill, unit)
        read = (r > c) if fill == "lower" else (r < c)
        if not unit:
            read = read | (r == c)
        poisoned = build(bmsp, n, r, c, np.where(read, v, np.nan), lay, dtype)
        b = rhs(n, dtype)
        for tol, m in ((0.0, 0), (NO_CHECK, 2), (TOLS[0], 0)):
            x, info = sweep(bmsp, poisoned, b, op, fill, unit, dtype, max_iter=m, tol=tol)
            want, ws, wc, *_ = ref_sweeps(n, r, c, v, dtype, op, fill, unit, 1.0, b, m or plan_levels(bmsp, n, r, c, op, fill) + 1, tol)
            assert not np.isnan(x).any()
            assert_same_bits(x, want, "%s op %s %s unit %s" % (name, op, fill, unit))
            assert (info["sweeps"], info["converged"]) == (ws, wc)


# ---------------------------------------------------------------------------------------------------------
# 8. nothing else is written
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_nothing_else_is_written(bmsp, dtype, lay):
    R = VEC[dtype]
    pad = 24
    for name in ("ragged203", "random2000"):
        for op, fill, unit in COMBOS:
            n, r, c, v, A = case(bmsp, name, dtype, lay, op, fill, unit)
            snap = snapshot(A)
            b = rhs(n, dtype)
            db = bmsp.DeviceArray.from_host(b, R)
            for tol, m, x0 in ((0.0, 0, False), (NO_CHECK, 1, False), (NO_CHECK, 2, False), (TOLS[0], 0, True), (NO_CHECK, 3, True)):
                whole = bmsp.DeviceArray.from_host(np.full(n + 2 * pad, -7.0, R), R)      # guard elements round x, ragged n included
                dx = bmsp.DeviceArray(n, R, ptr=whole.ptr + pad * np.dtype(R).itemsize, owner=whole)
                bmsp.spitsv(A, db, op, fill, unit, 1.0, m, tol, dx, x0)
                out = whole.to_host()
                assert (out[:pad] == R(-7.0)).all() and (out[n + pad:] == R(-7.0)).all()
                want, *_ = ref_sweeps(n, r, c, v, dtype, op, fill, unit, 1.0, b, m or 10 ** 4, tol, x0=np.full(n, -7.0, R) if x0 else None)
                assert_same_bits(out[pad:n + pad], want)
                assert_same_bits(db.to_host(), b)
            assert_unchanged(A, snap)


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_no_entries_and_no_rows(bmsp, dtype):
    R = VEC[dtype]
    e = np.zeros(0, np.int64)
    for lay in (0, 1):
        A = build(bmsp, 13, e, e, np.zeros(0), lay, dtype)      # nnz = 0: under a unit diagonal x = alpha b after one sweep, every row written
        b = rhs(13, dtype)
        for op in "NT":
            for fill in ("lower", "upper"):
                x, info, hist = sweep(bmsp, A, b, op, fill, True, dtype, alpha=-1.5, history=True)
                assert_same_bits(x, (R(-1.5) * b).astype(R))
                assert (info["sweeps"], info["converged"], info["levels"]) == (2, 1, 1) and hist[1] == 0.0, info
                x, info = sweep(bmsp, A, b, op, fill, True, dtype, alpha=-1.5, max_iter=1, tol=NO_CHECK)
                assert_same_bits(x, (R(-1.5) * b).astype(R))
                refused(bmsp, lambda: bmsp.spitsv(A, bmsp.DeviceArray.from_host(b, R), op, fill), "diag", "row 0 ")
        Z = build(bmsp, 0, e, e, np.zeros(0), lay, dtype)
        for op in "NT":
            for unit in (False, True):
                for tol in (0.0, NO_CHECK):
                    x, info = bmsp.spitsv(Z, bmsp.DeviceArray(0, R), op, "lower", unit, tol=tol)
                    assert x.n == 0 and info["sweeps"] == 0 and info["levels"] == 0 and info["kernel"].startswith("none"), info


# ---------------------------------------------------------------------------------------------------------
# 9. special values
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_inf_and_nan_follow_the_dependencies_only(bmsp, dtype, lay):
    name = "rmat10"
    for op in "NT":
        for fill in ("lower", "upper"):
            n, r, c, v = values(name, dtype, op, fill, False)
            levels = plan_levels(bmsp, n, r, c, op, fill)
            k, hit = next((k, h) for k in (n // 2, n // 3, n // 4, 2 * n // 3, 9, n - 10) for h in [dependants(n, r, c, op, fill, k)]
                          if 1 < h.sum() < n)
            b = rhs(n, dtype)
            cases = []
            vz = v.copy()
            vz[(r == k) & (c == k)] = 0.0                      # a stored zero on one diagonal: Inf there, Inf / NaN downstream
            cases.append((vz, b, False))
            vn = v.copy()
            vn[(r == k) & (c == k)] = np.nan                   # a stored NaN
            cases.append((vn, b, False))
            bi = b.copy()
            bi[k] = np.inf                                     # an Inf in b
            cases.append((v, bi, False))
            cases.append((values(name, dtype, op, fill, True)[3], bi, True))
            for vals, bb, unit in cases:
                A = build(bmsp, n, r, c, vals, lay, dtype)
                exact = solve(bmsp, A, bb, op, fill, unit, 1.0, dtype)
                x, info, hist = sweep(bmsp, A, bb, op, fill, unit, dtype, history=True)
                assert np.array_equal(~np.isfinite(x), hit)
                assert_same_bits(x, exact)
                assert_same_bits(x, reference(n, r, c, vals, dtype, op, fill, unit, 1.0, bb))
                # (whether a NaN "changed" depends on its payload, which is the hardware's: the sweep count is not compared with the
                # helper's, the statistics of the sweeps both ran are -- NaN differences skipped, an infinite one kept)
                want, ws, wc, wd, wx, _ = ref_sweeps(n, r, c, vals, dtype, op, fill, unit, 1.0, bb, levels + 1, 0.0)
                assert wc == 1 and info["converged"] == 1 and 1 <= info["sweeps"] <= levels + 1, (info, ws)
                both = min(ws, info["sweeps"])
                same_history(hist[:both], wd[:both], dtype)
                # a few sweeps: the special values have travelled exactly as far as in the reference
                x, _ = sweep(bmsp, A, bb, op, fill, unit, dtype, max_iter=3, tol=NO_CHECK)
                assert_same_bits(x, ref_sweeps(n, r, c, vals, dtype, op, fill, unit, 1.0, bb, 3, NO_CHECK)[0])


# ---------------------------------------------------------------------------------------------------------
# 10. life cycle
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 2])
def test_a_value_update_in_place_needs_no_invalidate(bmsp, dtype, lay):
    op, fill = ("T", "upper") if lay else ("N", "lower")
    n, r, c, v, A = case(bmsp, "rmat10", dtype, lay, op, fill, False)
    b = rhs(n, dtype)
    for tol, m in ((TOLS[0], 0), (NO_CHECK, 2)):
        x, _ = sweep(bmsp, A, b, op, fill, False, dtype, max_iter=m, tol=tol)
        assert_same_bits(x, ref_sweeps(n, r, c, v, dtype, op, fill, False, 1.0, b, m or 100, tol)[0])
    A.scale_(left=bmsp.DeviceArray.from_host(np.full(n, 2.0, VEC[dtype])))
    vs = 2.0 * v
    for tol, m in ((TOLS[0], 0), (NO_CHECK, 2), (0.0, 0)):
        x, _ = sweep(bmsp, A, b, op, fill, False, dtype, max_iter=m, tol=tol)
        assert_same_bits(x, ref_sweeps(n, r, c, vs, dtype, op, fill, False, 1.0, b, m or 100, tol)[0])


@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_spsv_and_spsm_are_untouched_by_an_interleaved_call(bmsp, dtype, lay):
    """the plan is shared, the temporary is the iteration's own: the substitutions give the same bits before and after"""
    R = VEC[dtype]
    k = 5
    for op, fill, unit in COMBOS:
        n, r, c, v, A = case(bmsp, "rmat10", dtype, lay, op, fill, unit)
        b = rhs(n, dtype)
        B = np.stack([np.roll(b, j) for j in range(k)], axis=1).astype(R)
        plan = bmsp.spsv_analyse(A, op, fill, unit)
        x1 = solve(bmsp, A, b, op, fill, unit, 1.0, dtype)
        X1 = bmsp.spsm(A, bmsp.DeviceArray.from_host(B.ravel(), R), k, op, fill, unit).to_host()
        xi, info = sweep(bmsp, A, b, op, fill, unit, dtype, max_iter=3, tol=NO_CHECK)
        x2 = solve(bmsp, A, b, op, fill, unit, 1.0, dtype)
        xj, info = sweep(bmsp, A, b, op, fill, unit, dtype)
        X2 = bmsp.spsm(A, bmsp.DeviceArray.from_host(B.ravel(), R), k, op, fill, unit).to_host()
        assert bmsp.spsv_analyse(A, op, fill, unit) == plan and info["levels"] == plan["levels"]
        assert_same_bits(x2, x1)
        assert_same_bits(X2, X1)
        assert_same_bits(xj, x1)
        assert_same_bits(X1.reshape(n, k)[:, 0], x1)
        # a fresh handle that only ever iterated builds the plan the substitution then finds
        F = build(bmsp, n, r, c, v, lay, dtype)
        assert_same_bits(sweep(bmsp, F, b, op, fill, unit, dtype, max_iter=3, tol=NO_CHECK)[0], xi)
        assert bmsp.spsv_analyse(F, op, fill, unit) == plan


# ---------------------------------------------------------------------------------------------------------
# 11. streams
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [3, 4])        # the last iterate in d_x, and in the temporary (one device copy behind the sweeps)
@pytest.mark.parametrize("op,lay", [("N", 0), ("T", 0), ("N", 1)])
def test_no_check_on_a_gated_stream(bmsp, op, lay, m):
    import stream_gate as G
    n, r, c, v, A = case(bmsp, "rmat10", 0, lay, op, "lower", False)
    hb = rhs(n, 0)
    b = bmsp.DeviceArray.from_host(hb)
    null = bmsp.spitsv(A, b, op, "lower", max_iter=m, tol=NO_CHECK)[0].to_host()     # the plan and the temporary exist from here on
    assert_same_bits(null, ref_sweeps(n, r, c, v, 0, op, "lower", False, 1.0, hb, m, NO_CHECK)[0])
    x = bmsp.DeviceArray.from_host(np.zeros(n, np.float32))
    bmsp.synchronize()
    st, side = G.new_stream(), G.Side()
    gate = G.Gate()
    try:
        gate.close(st)
        bmsp.spitsv(A, b, op, "lower", max_iter=m, tol=NO_CHECK, x=x, stream=st.value)
        closed = gate.is_closed()                      # the call came back while the gate held the stream
        held = side.read(x.ptr, n, np.float32)
        still = gate.is_closed()
        gate.finish()
        assert closed, "bmsp_spitsv (BMSP_ITSV_NO_CHECK) did not return while the gate was closed"
        if still:
            assert not held.any()                      # nothing ran ahead of the gate
        assert_same_bits(x.to_host(), null)
    finally:
        gate.finish()
        side.close()
        G.destroy_stream(st)


# ---------------------------------------------------------------------------------------------------------
# 12. refusals on real handles; the C++ wrapper
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
def test_refusals_on_real_handles(bmsp, lay):
    n, r, c, v = values("ragged203", 0, "N", "lower", False)
    b = bmsp.DeviceArray.from_host(rhs(n, 0))
    x = bmsp.DeviceArray.from_host(np.full(n, -7.0, np.float32))
    full = build(bmsp, n, r, c, v, lay, 0)
    L = bmsp.lib()

    def call(A, db, dx, max_iter=0, tol=0.0, flags=0, op=0, fill=0, diag=0):
        return L.bmsp_spitsv(A.h, op, fill, diag, 1.0, db, dx, max_iter, tol, flags, None, None, None)

    assert call(full, None, x.ptr) == -1 and "d_b" in L.bmsp_last_error().decode()
    assert call(full, b.ptr, None) == -1 and "d_x" in L.bmsp_last_error().decode()
    assert call(full, b.ptr, b.ptr) == -1 and "d_x must not be d_b" in L.bmsp_last_error().decode()
    assert call(full, b.ptr, b.ptr, max_iter=-1) == -1 and L.bmsp_last_error().decode().startswith("max_iter")
    assert call(full, b.ptr, x.ptr, fill=3) == -1 and L.bmsp_last_error().decode().startswith("fill")
    for gone in (77, 202):
        keep = ~((r == gone) & (c == gone))
        A = build(bmsp, n, r[keep], c[keep], v[keep], lay, 0)
        for op in "NT":
            for fill in ("lower", "upper"):
                refused(bmsp, lambda: bmsp.spitsv(A, b, op, fill, x=x), "diag", "row %d " % gone)
                refused(bmsp, lambda: bmsp.spitsv(A, b, op, fill, tol=NO_CHECK, max_iter=2, x=x), "diag", "row %d " % gone)
    e = np.arange(8)
    W = bmsp.BmSpMatrix.from_coo(8, 16, e, e, np.ones(8), transposed=bool(lay))
    refused(bmsp, lambda: bmsp.spitsv(W, b, x=x), "square")
    if not lay:
        refused(bmsp, lambda: bmsp.spitsv(full.row_panel(1, 13), b, unit_diag=True, x=x), "row-panel view")
    assert (x.to_host() == np.float32(-7.0)).all()          # nothing was done on the device
    with pytest.raises(ValueError):
        bmsp.spitsv(full, b, x0_given=True)


def test_cpp_wrapper_runs(bmsp, tmp_path):
    """tests/cpp_spitsv_check.cpp: bmSparse_SpITSV for float, half and double on a fixture written here"""
    n, r, c, v = values("ragged203", 1, "N", "lower", False)
    v = np.where(r == c, np.sign(v) * 64.0, v)          # (one diagonal for every triangle and op: larger than any row or column sum)
    mtx = tmp_path / "tri.mtx"
    with open(mtx, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n, r.size))
        for i, j, a in zip(r, c, v):
            f.write("%d %d %.17g\n" % (i + 1, j + 1, a))
    exe = str(tmp_path / "cpp_spitsv_check")
    build_cpp_spitsv_check(exe)
    out = subprocess.run([exe, str(mtx)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("OK") == 3 and "FAIL" not in out.stdout, out.stdout
