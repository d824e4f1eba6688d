"""GPU tests of bmsp_spsv: op(tri(A)) x = alpha b for both tile layouts, both ops, both triangles and both kinds of diagonal, F32 / F16 /
F64, bit for bit against tests/spsv_ref.c (a row loop with fmaf / fma and one division, run on the triangle's COO in chain order).  There
is no tolerance anywhere: the call fixes its arithmetic.  The matrices, their values and the reference live in tests/test_spsv_api.py."""
import subprocess
import numpy as np
import pytest
from test_spsv_api import (MATRICES, SMALL, SHAPES, NP, VEC, pattern, values, rhs, reference, assert_same_bits, block_records, py_plan,
                           effective_lower, build_cpp_spsv_check)
from test_transpose import snapshot, assert_unchanged, _write_values

pytestmark = pytest.mark.gpu

OPS, FILLS = ("N", "T"), ("lower", "upper")
CHAINS = ("0", None, str(1 << 31))      # never chain, the default, chain every run of levels
COMBOS = [(op, fill, unit) for op in OPS for fill in FILLS for unit in (False, True)]


def set_chain(monkeypatch, chain):
    if chain is None:
        monkeypatch.delenv("BMSP_SPSV_CHAIN", raising=False)
    else:
        monkeypatch.setenv("BMSP_SPSV_CHAIN", chain)


def build(bmsp, n, r, c, v, lay, dtype):
    return bmsp.BmSpMatrix.from_coo(n, n, r, c, v, transposed=bool(lay), dtype=dtype)


def solve(bmsp, A, b, op, fill, unit, alpha=1.0, dtype=0):
    return bmsp.spsv(A, bmsp.DeviceArray.from_host(b, VEC[dtype]), op, fill, unit, alpha).to_host()


def case(bmsp, name, dtype, lay, op, fill, unit):
    n, r, c, v = values(name, dtype, op, fill, unit)
    return n, r, c, v, build(bmsp, n, r, c, v, lay, dtype)


# ---------------------------------------------------------------------------------------------------------
# 1. bits against the helper, under every chain setting
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", MATRICES + SMALL)
def test_bits_match_the_helper_under_every_chain_setting(bmsp, monkeypatch, name, dtype, lay):
    for op, fill, unit in COMBOS:
        n, r, c, v, A = case(bmsp, name, dtype, lay, op, fill, unit)
        b = rhs(n, dtype)
        want = reference(n, r, c, v, dtype, op, fill, unit, 1.0, b)
        assert np.isfinite(want).all()
        for chain in CHAINS:
            set_chain(monkeypatch, chain)
            A.invalidate(True)      # the switch is read when a plan is built
            got = solve(bmsp, A, b, op, fill, unit, 1.0, dtype)
            assert_same_bits(got, want, "%s op %s %s unit %s chain %s" % (name, op, fill, unit, chain))


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_no_entries_and_no_rows(bmsp, dtype):
    e = np.zeros(0, np.int64)
    for lay in (0, 1):
        A = build(bmsp, 13, e, e, np.zeros(0), lay, dtype)      # nnz = 0: under a unit diagonal x = alpha b, every row written
        b = rhs(13, dtype)
        for op in OPS:
            for fill in FILLS:
                got = solve(bmsp, A, b, op, fill, True, -1.5, dtype)
                assert_same_bits(got, (VEC[dtype](-1.5) * b).astype(VEC[dtype]))
                info = bmsp.spsv_analyse(A, op, fill, True)
                assert info["levels"] == 1 and info["max_level_width"] == 2 and info["launches"] == 1, info
        Z = build(bmsp, 0, e, e, np.zeros(0), lay, dtype)
        for op in OPS:
            for unit in (False, True):
                x = bmsp.spsv(Z, bmsp.DeviceArray(0, VEC[dtype]), op, "lower", unit)
                assert x.n == 0
                info = bmsp.spsv_analyse(Z, op, "lower", unit)
                assert info["levels"] == 0 and info["launches"] == 0 and info["kernel"].startswith("none"), info


# ---------------------------------------------------------------------------------------------------------
# 2. launch info
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MATRICES)
def test_analyse_reports_the_planners_schedule(bmsp, monkeypatch, name):
    n, r, c = pattern(name)
    blocks, levels, widths = SHAPES[name]
    for lay in (0, 1):
        for op in OPS:
            for fill in FILLS:
                _, _, _, v = values(name, 0, op, fill, False)
                ptr, other = block_records(n, r, c, op)
                lower = effective_lower(op, fill)
                for chain in CHAINS:
                    set_chain(monkeypatch, chain)
                    A = build(bmsp, n, r, c, v, lay, 0)
                    info = bmsp.spsv_analyse(A, op, fill)
                    _, _, lp, segs = py_plan(ptr, other, lower, 32 if chain is None else int(chain))
                    assert info["levels"] == lp.size - 1 and info["max_level_width"] == int(np.diff(lp).max()), (info, chain)
                    assert info["launches"] == len(segs) and info["chain_launches"] == int(segs[:, 2].sum()), (info, chain)
                    assert info["chained_levels"] == int(((segs[:, 1] - segs[:, 0]) * segs[:, 2]).sum()), (info, chain)
                    assert info["plan_bytes"] == 4 * blocks + 4 * (info["levels"] + 1), info
                    if chain == "0":
                        assert info["launches"] == info["levels"] and info["chain_launches"] == 0, info
                    if op == "N" and fill == "lower":
                        assert info["levels"] == levels[0] and info["max_level_width"] == widths[0], info
                    minor = (op == "T") != bool(lay)
                    assert info["kernel"] == "spsv_level_kernel<F32, %s, %s, NON_UNIT>" % ("MINOR" if minor else "MAJOR", "LOWER" if lower else "UPPER")
                    assert bmsp.spsv_analyse(A, op, fill, True)["kernel"].endswith(", UNIT>")
    set_chain(monkeypatch, None)
    n, r, c, v, A = case(bmsp, "banded400", 0, 0, "N", "lower", False)
    info = bmsp.spsv_analyse(A, "N", "lower")
    assert info["chain_launches"] > 0 and info["launches"] < info["levels"], info


# ---------------------------------------------------------------------------------------------------------
# 3. what is not read
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
        poisoned = np.where(read, v, np.nan)
        b = rhs(n, dtype)
        tri = build(bmsp, n, r[read], c[read], v[read], lay, dtype)
        want = solve(bmsp, tri, b, op, fill, unit, 1.0, dtype)
        got = solve(bmsp, build(bmsp, n, r, c, poisoned, lay, dtype), b, op, fill, unit, 1.0, dtype)
        assert not np.isnan(got).any()
        assert_same_bits(got, want, "%s op %s %s unit %s" % (name, op, fill, unit))
        assert_same_bits(got, reference(n, r, c, v, dtype, op, fill, unit, 1.0, b))


# ---------------------------------------------------------------------------------------------------------
# 4. in place; nothing else is written
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_in_place_and_nothing_else_is_written(bmsp, dtype, lay):
    R = VEC[dtype]
    for name in ("ragged203", "random2000"):
        for op, fill, unit in COMBOS:
            n, r, c, v, A = case(bmsp, name, dtype, lay, op, fill, unit)
            snap = snapshot(A)
            b = rhs(n, dtype)
            pad = 24
            db = bmsp.DeviceArray.from_host(b, R)
            dx = bmsp.DeviceArray.from_host(np.full(n + pad, -7.0, R), R)   # (room behind n: nothing at or beyond n is written)
            bmsp.spsv(A, db, op, fill, unit, 1.0, dx)
            out = dx.to_host()
            assert_same_bits(db.to_host(), b)
            assert (out[n:] == R(-7.0)).all()
            assert_same_bits(out[:n], reference(n, r, c, v, dtype, op, fill, unit, 1.0, b))
            assert bmsp.spsv(A, db, op, fill, unit, 1.0, db) is db
            assert_same_bits(db.to_host(), out[:n])
            assert_unchanged(A, snap)


# ---------------------------------------------------------------------------------------------------------
# 5. alpha
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_alpha_is_rounded_once_and_multiplied_first(bmsp, dtype, lay):
    for op, fill, unit in COMBOS:
        n, r, c, v, A = case(bmsp, "fem8", dtype, lay, op, fill, unit)
        b = rhs(n, dtype)
        for alpha in (1.0, -1.5, 0.0, float(np.float32(1.0) / np.float32(3.0)), 1.0 / 3.0):
            got = solve(bmsp, A, b, op, fill, unit, alpha, dtype)
            assert_same_bits(got, reference(n, r, c, v, dtype, op, fill, unit, VEC[dtype](alpha), b), "alpha %r" % alpha)


# ---------------------------------------------------------------------------------------------------------
# 6. special values
# ---------------------------------------------------------------------------------------------------------
def dependants(n, r, c, op, fill, k):
    """the rows whose solution depends on row k (k included): reachability in the effective strict triangle"""
    keep = (r > c) if fill == "lower" else (r < c)
    er, ec = (c[keep], r[keep]) if op == "T" else (r[keep], c[keep])
    hit = np.zeros(n, bool)
    hit[k] = True
    lower = effective_lower(op, fill)
    o = np.lexsort((ec, er)) if lower else np.lexsort((ec, -er))
    for i, j in zip(er[o], ec[o]):
        if hit[j]:
            hit[i] = True
    return hit


@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_zero_diagonal_and_infinite_rhs(bmsp, monkeypatch, dtype, lay):
    name = "rmat10"
    for chain in ("0", None):
        set_chain(monkeypatch, chain)
        for op in OPS:
            for fill in FILLS:
                n, r, c, v = values(name, dtype, op, fill, False)
                k, hit = next((k, h) for k in (n // 2, n // 3, n // 4, 2 * n // 3, 9, n - 10) for h in [dependants(n, r, c, op, fill, k)]
                              if 1 < h.sum() < n)
                # a stored zero on one diagonal: Inf / NaN exactly where the helper has them, finite bits elsewhere
                vz = v.copy()
                vz[(r == k) & (c == k)] = 0.0
                b = rhs(n, dtype)
                want = reference(n, r, c, vz, dtype, op, fill, False, 1.0, b)
                got = solve(bmsp, build(bmsp, n, r, c, vz, lay, dtype), b, op, fill, False, 1.0, dtype)
                assert np.isinf(want[k]) and np.array_equal(~np.isfinite(want), hit)
                assert np.array_equal(np.isinf(got), np.isinf(want))
                assert_same_bits(got, want)
                # an Inf in b_k reaches exactly the dependent rows (and only as far as the helper says)
                bi = b.copy()
                bi[k] = np.inf
                for unit in (False, True):
                    n, r, c, vu = values(name, dtype, op, fill, unit)
                    want = reference(n, r, c, vu, dtype, op, fill, unit, 1.0, bi)
                    got = solve(bmsp, build(bmsp, n, r, c, vu, lay, dtype), bi, op, fill, unit, 1.0, dtype)
                    assert np.array_equal(~np.isfinite(want), hit)
                    assert np.array_equal(np.isinf(got), np.isinf(want))
                    assert_same_bits(got, want)


@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_subnormals_are_kept(bmsp, dtype, lay):
    S, R = NP[dtype], VEC[dtype]
    tiny_s = float(np.finfo(S).smallest_subnormal)
    n, r, c = pattern("dense9")
    rng = np.random.default_rng(3)
    for op in OPS:
        for fill in FILLS:
            # subnormal off-diagonals (stored subnormal in S) against ordinary x; and subnormal results: b at the bottom of R's normal
            # range, halved by the diagonal
            v = np.where(r == c, 2.0, tiny_s * rng.integers(1, 900, r.size) * rng.choice([-1.0, 1.0], r.size))
            v = v.astype(S).astype(np.float64)
            for scale in (1.0, float(np.finfo(R).tiny)):
                b = (rhs(n, dtype) * R(scale)).astype(R)
                for unit in (False, True):
                    want = reference(n, r, c, v, dtype, op, fill, unit, 1.0, b)
                    got = solve(bmsp, build(bmsp, n, r, c, v, lay, dtype), b, op, fill, unit, 1.0, dtype)
                    assert_same_bits(got, want)
                    if scale != 1.0 and not unit:
                        assert (np.abs(want) < np.finfo(R).tiny).any() and (want != 0).all()
            # ordinary off-diagonals against a subnormal right-hand side: every sum and every result is subnormal and none is flushed
            v2 = np.where(r == c, 1.0, rng.uniform(0.5, 2.0, r.size) / 16 * rng.choice([-1.0, 1.0], r.size)).astype(S).astype(np.float64)
            b = (rhs(n, dtype) * R(np.finfo(R).tiny) * R(0.25)).astype(R)
            want = reference(n, r, c, v2, dtype, op, fill, False, 1.0, b)
            got = solve(bmsp, build(bmsp, n, r, c, v2, lay, dtype), b, op, fill, False, 1.0, dtype)
            assert (want != 0).all() and (np.abs(want) < np.finfo(R).tiny).all()
            assert_same_bits(got, want)


# ---------------------------------------------------------------------------------------------------------
# 7. life cycle
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("dtype", [0, 2])
def test_new_values_need_no_invalidate_and_value_updates_keep_the_plan(bmsp, monkeypatch, dtype, lay):
    op, fill = ("T", "upper") if lay else ("N", "lower")
    set_chain(monkeypatch, "0")     # plans built here never chain; the switch changes below, so a rebuilt plan would show
    n, r, c, v, A = case(bmsp, "rmat10", dtype, lay, op, fill, False)
    b = rhs(n, dtype)
    assert_same_bits(solve(bmsp, A, b, op, fill, False, 1.0, dtype), reference(n, r, c, v, dtype, op, fill, False, 1.0, b))
    plan = bmsp.spsv_analyse(A, op, fill)
    assert plan["chain_launches"] == 0 and plan["launches"] == plan["levels"] > 1
    # overwritten in place: the next solve reads the new values, without invalidate
    _, _, _, v2 = values("rmat10", dtype, op, fill, False, seed=12)
    assert not np.array_equal(v, v2)
    _write_values(bmsp, A, build(bmsp, n, r, c, v2, lay, dtype).host_arrays()[3])
    assert_same_bits(solve(bmsp, A, b, op, fill, False, 1.0, dtype), reference(n, r, c, v2, dtype, op, fill, False, 1.0, b))
    # invalidate(A, 0), scale_, copy_values and add_values into A keep the plan
    A.invalidate(False)
    A.scale_(left=bmsp.DeviceArray.from_host(np.full(n, 2.0, VEC[dtype])))
    src = build(bmsp, n, r, c, v, 1 - lay, dtype)
    B = src.with_layout(lay)
    B.copy_values_from(src)
    S = bmsp.add(B, B, 0.5, 0.5, transposed=lay)
    plan_s = bmsp.spsv_analyse(S, op, fill)
    set_chain(monkeypatch, None)
    bmsp.add_values(S, B, B, 2.0, -1.0)
    B.copy_values_from(src)
    assert bmsp.spsv_analyse(S, op, fill) == plan_s == plan
    assert bmsp.spsv_analyse(A, op, fill) == plan
    vs = 2.0 * v2
    assert_same_bits(solve(bmsp, A, b, op, fill, False, 1.0, dtype), reference(n, r, c, vs, dtype, op, fill, False, 1.0, b))
    assert_same_bits(solve(bmsp, S, b, op, fill, False, 1.0, dtype), reference(n, r, c, v, dtype, op, fill, False, 1.0, b))


def test_plan_survives_value_updates_without_a_rebuild(bmsp, monkeypatch):
    """the chain switch is read only when a plan is built: a plan that reports the old setting after the switch changed was not rebuilt"""
    n, r, c, v, A = case(bmsp, "banded400", 0, 0, "N", "lower", False)
    set_chain(monkeypatch, "0")
    before = bmsp.spsv_analyse(A, "N", "lower")
    assert before["chain_launches"] == 0
    set_chain(monkeypatch, None)
    A.invalidate(False)
    A.scale_(left=bmsp.DeviceArray.from_host(np.ones(n, np.float32)))
    assert bmsp.spsv_analyse(A, "N", "lower") == before
    A.invalidate(True)
    assert bmsp.spsv_analyse(A, "N", "lower")["chain_launches"] > 0


@pytest.mark.parametrize("lay", [0, 1])
def test_structure_change_with_invalidate(bmsp, lay):
    """A's four arrays are overwritten with those of its transpose (as many tiles and values, other keys): invalidate(A, 1), a new plan"""
    n, r, c, v = values("rmat10", 0, "N", "lower", False)
    A = build(bmsp, n, r, c, v, lay, 0)
    b = rhs(n, 0)
    assert_same_bits(solve(bmsp, A, b, "N", "lower", False), reference(n, r, c, v, 0, "N", "lower", False, 1.0, b))
    one = bmsp.spsv_analyse(A, "N", "lower")
    _, _, _, vt = values("rmat10", 0, "T", "upper", False)       # (dominant for the lower triangle of the transpose)
    T = build(bmsp, n, c, r, vt, lay, 0)
    for d, h in zip(A.device_arrays(), T.host_arrays()):
        assert d.n == h.size
        bmsp.check(bmsp.lib().bmsp_memcpy_h2d(d.ptr, h.ctypes.data, h.nbytes))
    A.invalidate(True)
    assert_same_bits(solve(bmsp, A, b, "N", "lower", False), reference(n, c, r, vt, 0, "N", "lower", False, 1.0, b))
    two = bmsp.spsv_analyse(A, "N", "lower")
    assert (one["levels"], two["levels"]) == SHAPES["rmat10"][1]


@pytest.mark.parametrize("lay", [0, 1])
def test_op_t_shares_the_view_of_spmv_op(bmsp, lay):
    n, r, c, v, A = case(bmsp, "rmat10", 0, lay, "T", "lower", False)
    view = bmsp.spmv_op_launch_info(A, "T")["view_bytes"]
    assert view > 0
    b = rhs(n, 0)
    assert_same_bits(solve(bmsp, A, b, "T", "lower", False), reference(n, r, c, v, 0, "T", "lower", False, 1.0, b))
    assert bmsp.spmv_op_launch_info(A, "T")["view_bytes"] == view
    # and the other way round: the solve builds the view the product then finds
    n, r, c, v, A = case(bmsp, "rmat10", 0, lay, "T", "upper", True)
    solve(bmsp, A, b, "T", "upper", True)
    assert bmsp.spmv_op_launch_info(A, "T")["view_bytes"] == view


# ---------------------------------------------------------------------------------------------------------
# 8. refusals on real handles
# ---------------------------------------------------------------------------------------------------------
def refused(bmsp, fn, *words):
    with pytest.raises(bmsp.BmspError) as e:
        fn()
    assert e.value.status == -1, e.value
    for w in words:
        assert w in str(e.value), (w, str(e.value))


@pytest.mark.parametrize("lay", [0, 1])
def test_refusals_on_real_handles(bmsp, lay):
    n, r, c, v = values("ragged203", 0, "N", "lower", False)
    b = bmsp.DeviceArray.from_host(rhs(n, 0))
    hb = b.to_host()
    for gone in (77, 202):         # 202: the ragged last block, whose rows 203 .. 207 do not exist and must not count
        keep = ~((r == gone) & (c == gone))
        A = build(bmsp, n, r[keep], c[keep], v[keep], lay, 0)
        for op in OPS:
            for fill in FILLS:
                refused(bmsp, lambda: bmsp.spsv_analyse(A, op, fill), "diag", "row %d " % gone)
                refused(bmsp, lambda: bmsp.spsv(A, b, op, fill), "diag", "row %d " % gone)
                # the refused analysis leaves nothing a later non-unit call would trust, and the unit solve of the same handle works
                _, _, _, vu = values("ragged203", 0, op, fill, True)
                U = build(bmsp, n, r[keep], c[keep], vu[keep], lay, 0)
                refused(bmsp, lambda: bmsp.spsv(U, b, op, fill), "row %d " % gone)
                assert_same_bits(bmsp.spsv(U, b, op, fill, True).to_host(), reference(n, r[keep], c[keep], vu[keep], 0, op, fill, True, 1.0, hb))
                refused(bmsp, lambda: bmsp.spsv(U, b, op, fill), "row %d " % gone)
    full = build(bmsp, n, r, c, v, lay, 0)
    assert bmsp.spsv_analyse(full, "N", "lower")["levels"] == 26     # every diagonal entry stored: rows >= n did not count
    L = bmsp.lib()
    assert L.bmsp_spsv(full.h, 0, 0, 0, 1.0, None, b.ptr, None) == -1 and "d_b" in L.bmsp_last_error().decode()
    assert L.bmsp_spsv(full.h, 0, 0, 0, 1.0, b.ptr, None, None) == -1 and "d_x" in L.bmsp_last_error().decode()
    assert L.bmsp_spsv(full.h, 0, 3, 0, 1.0, None, None, None) == -1 and L.bmsp_last_error().decode().startswith("fill")
    # not square
    e = np.arange(8)
    W = bmsp.BmSpMatrix.from_coo(8, 16, e, e, np.ones(8), transposed=bool(lay))
    refused(bmsp, lambda: bmsp.spsv_analyse(W, "N", "lower"), "square")
    assert L.bmsp_spsv(W.h, 0, 0, 1, 1.0, b.ptr, b.ptr, None) == -1 and "square" in L.bmsp_last_error().decode()
    # a row-panel view
    if not lay:
        P = full.row_panel(1, 13)
        refused(bmsp, lambda: bmsp.spsv_analyse(P, "N", "lower", True), "row-panel view")
        assert L.bmsp_spsv(P.h, 0, 0, 1, 1.0, b.ptr, b.ptr, None) == -1 and "row-panel view" in L.bmsp_last_error().decode()


# ---------------------------------------------------------------------------------------------------------
# 9. streams
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,lay", [("N", 0), ("T", 0), ("N", 1)])
def test_on_a_gated_stream(bmsp, op, lay):
    import stream_gate as G
    n, r, c, v, A = case(bmsp, "rmat10", 0, lay, op, "lower", False)
    hb = rhs(n, 0)
    b = bmsp.DeviceArray.from_host(hb)
    null = bmsp.spsv(A, b, op, "lower").to_host()     # the plan exists from here on
    assert_same_bits(null, reference(n, r, c, v, 0, op, "lower", False, 1.0, hb))
    x = bmsp.DeviceArray.from_host(np.zeros(n, np.float32))
    bmsp.synchronize()
    st, side = G.new_stream(), G.Side()
    gate = G.Gate()
    try:
        gate.close(st)
        bmsp.spsv(A, b, op, "lower", x=x, stream=st.value)
        closed = gate.is_closed()                      # the call came back while the gate held the stream
        held = side.read(x.ptr, n, np.float32)
        still = gate.is_closed()
        gate.finish()
        assert closed, "bmsp_spsv did not return while the gate was closed"
        if still:
            assert not held.any()                      # nothing ran ahead of the gate
        assert_same_bits(x.to_host(), null)
        # the analysis of a fresh handle synchronises the stream: it returns only after the gate's timeout
        F = build(bmsp, n, r, c, v, lay, 0)
        bmsp.synchronize()
        gate2 = G.Gate()
        gate2.close(st)
        info = bmsp.spsv_analyse(F, op, "lower", stream=st.value)
        assert gate2.opened_by_timeout(), "bmsp_spsv_analyse returned before the stream was drained"
        gate2.finish()
        assert info["levels"] == SHAPES["rmat10"][1][0]
    finally:
        gate.finish()
        side.close()
        G.destroy_stream(st)


def test_cpp_wrapper_runs(bmsp, tmp_path):
    """tests/cpp_spsv_check.cpp: bmSparse_SpSV and bmSparse_SpSV_analyse for float, half and double on a fixture written here"""
    n, r, c, v = values("ragged203", 1, "N", "lower", False)
    v = np.where(r == c, np.sign(v) * 64.0, v)          # (one diagonal for every triangle and op: larger than any row or column sum)
    mtx = tmp_path / "tri.mtx"
    with open(mtx, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n, r.size))
        for i, j, a in zip(r, c, v):
            f.write("%d %d %.17g\n" % (i + 1, j + 1, a))
    exe = str(tmp_path / "cpp_spsv_check")
    build_cpp_spsv_check(exe)
    out = subprocess.run([exe, str(mtx)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("OK") == 3 and "FAIL" not in out.stdout, out.stdout
