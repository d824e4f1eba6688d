"""GPU tests of bmsp_matrix_color_blocks / bmsp_matrix_permute_blocks / bmsp_vec_permute_blocks.  Everything is integers or raw bits, so
there is no tolerance anywhere.  The colouring is compared with the sequential reference of tests/test_reorder_api.py (whose self-checks
run without a GPU); a permuted matrix with the host route it replaces (to_coo, the indices mapped through the inverse permutations,
from_coo in the output layout), all four arrays and the block-row pointer; the vectors with numpy indexing; the whole chain -- reorder,
permute b, bmsp_spsv, permute x back -- with the reference of tests/test_spsv_api.py applied to the host-permuted triples."""
import ctypes as C
import subprocess
import numpy as np
import pytest
import stream_gate as sg
from test_reorder_api import NAMES, SEEDS, pattern, generic_values, reference, inverse, permuted, plan_levels, build_cpp_reorder_check
from test_spsv_api import reference as spsv_reference, assert_same_bits, effective_lower, NP, VEC
from test_transpose import assert_same_arrays, snapshot, assert_unchanged, _write_values
from test_streams import Case, Ops, run_gated, dev, SYNC, ASYNC

pytestmark = pytest.mark.gpu

LAYOUTS = [(lin, lout) for lin in (0, 1) for lout in (0, 1)]
SQUARE = tuple(n for n in NAMES if n != "empty")


def build(bmsp, name, lay, dtype, v=None):
    n, r, c = pattern(name)
    return bmsp.BmSpMatrix.from_coo(n, n, r, c, generic_values(name, dtype) if v is None else v, transposed=bool(lay), dtype=dtype)


def dperm(bmsp, p):
    return bmsp.DeviceArray.from_host(np.asarray(p), np.uint32)


def host_route(bmsp, A, rp, cp, lay_out):
    """what permute_blocks replaces: the stored entries, their indices through the inverse permutations, the builder"""
    i = A.info()
    r, c, v = A.to_coo()
    r2, c2 = permuted(r, c, rp, cp)
    return bmsp.BmSpMatrix.from_coo(i["num_rows"], i["num_cols"], r2, c2, v, transposed=bool(lay_out), dtype=i["dtype"])


def assert_same_matrix(got, want):
    assert_same_arrays(got, want)
    np.testing.assert_array_equal(got.block_row_ptr(), want.block_row_ptr())


# ---------------------------------------------------------------------------------------------------------
# 1. the colouring
# ---------------------------------------------------------------------------------------------------------
def check_colouring(name, seed, got):
    colors, perm, info = got
    rc, _, rp, n_colors, n_rounds = reference(name, seed)
    np.testing.assert_array_equal(colors.to_host(), rc)
    if perm is not None:
        np.testing.assert_array_equal(perm.to_host(), rp)
    assert (info["blocks"], info["colors"], info["rounds"]) == (rc.size, n_colors, n_rounds), (info, n_colors, n_rounds)
    assert info["kernel"] == ("color_round_kernel<8 lanes>" if rc.size else "none (empty matrix)")
    assert (info["view_bytes"] > 0) == (rc.size > 0)


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_colouring_equals_the_reference(bmsp, name, lay, seed, dtype):
    A = build(bmsp, name, lay, dtype)
    snap = snapshot(A)
    check_colouring(name, seed, A.color_blocks(seed))
    check_colouring(name, seed, A.color_blocks(seed))                           # the view is cached now
    check_colouring(name, seed, bmsp.color_blocks(A, seed, want_perm=False))    # d_perm = NULL
    assert_unchanged(A, snap)


@pytest.mark.parametrize("check", ["1", "3", "1000"])
@pytest.mark.parametrize("name", ["dense528", "hub", "band203"])
def test_rounds_enqueued_ahead_do_not_change_the_result(bmsp, monkeypatch, name, check):
    monkeypatch.setenv("BMSP_COLOR_CHECK", check)
    for seed in SEEDS:
        check_colouring(name, seed, build(bmsp, name, 0, 0).color_blocks(seed))


@pytest.mark.parametrize("lay", [0, 1])
def test_a_triangle_colours_like_its_symmetrisation(bmsp, lay):
    for seed in SEEDS:
        lo, _, li = build(bmsp, "lowerband", lay, 0).color_blocks(seed)
        fu, _, fi = build(bmsp, "band200", lay, 0).color_blocks(seed)
        np.testing.assert_array_equal(lo.to_host(), fu.to_host())
        assert (li["colors"], li["rounds"]) == (fi["colors"], fi["rounds"])


def test_colouring_refusals(bmsp):
    from pybmsp import gen
    A = build(bmsp, "band200", 0, 0)
    with pytest.raises(bmsp.BmspError) as e:
        A.row_panel(2, 9).color_blocks()
    assert e.value.status == -1 and ("view" in str(e.value) or "square" in str(e.value))
    n, m, r, c, v = gen.random_coo(203, 96, 1500, seed=6)
    with pytest.raises(bmsp.BmspError) as e:
        bmsp.BmSpMatrix.from_coo(n, m, r, c, v).color_blocks()
    assert e.value.status == -1 and "square" in str(e.value)
    info = bmsp.ColorInfo()
    assert bmsp.lib().bmsp_matrix_color_blocks(A.h, 0, None, None, None, C.byref(info)) == -1
    assert "d_colors" in bmsp.lib().bmsp_last_error().decode()
    check_colouring("band200", 0, A.color_blocks(0))


# ---------------------------------------------------------------------------------------------------------
# 2. the permutation
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("lin,lout", LAYOUTS)
@pytest.mark.parametrize("name", NAMES)
def test_symmetric_permutation_by_the_colouring_equals_the_host_route(bmsp, name, lin, lout, dtype):
    A = build(bmsp, name, lin, dtype)
    snap = snapshot(A)
    p = reference(name, 0)[2]
    d = dperm(bmsp, p)
    B = A.permute_blocks(d, d, lout)
    assert_same_matrix(B, host_route(bmsp, A, p, p, lout))
    assert_unchanged(A, snap)
    # back through the inverse, and the identity in both spellings
    dinv = dperm(bmsp, inverse(p))
    assert_same_matrix(B.permute_blocks(dinv, dinv, lin), A)
    ident = dperm(bmsp, np.arange(p.size))
    assert_same_matrix(A.permute_blocks(ident, ident, lin), A)
    assert_same_matrix(A.permute_blocks(None, None, lout), A.with_layout(lout))
    assert_same_matrix(A.permute_blocks(transposed=None), A)


def rectangle():
    from pybmsp import gen
    n, m, r, c, _ = gen.random_coo(203, 96, 1500, seed=6)
    rng = np.random.default_rng(4)
    rp = np.r_[rng.permutation(25), 25].astype(np.uint32)       # 203 % 8 != 0: the last block-row stays
    cp = rng.permutation(12).astype(np.uint32)                  # 96 % 8 == 0: any permutation
    return n, m, np.asarray(r, np.int64), np.asarray(c, np.int64), rp, cp


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("lin,lout", LAYOUTS)
@pytest.mark.parametrize("which", ["rows", "cols", "both"])
def test_rectangle_rows_columns_and_both(bmsp, which, lin, lout, dtype):
    n, m, r, c, rp, cp = rectangle()
    v = np.random.default_rng(9).uniform(0.5, 2.0, r.size).astype(NP[dtype]).astype(np.float64)
    A = bmsp.BmSpMatrix.from_coo(n, m, r, c, v, transposed=bool(lin), dtype=dtype)
    snap = snapshot(A)
    rp = rp if which != "cols" else None
    cp = cp if which != "rows" else None
    B = A.permute_blocks(None if rp is None else dperm(bmsp, rp), None if cp is None else dperm(bmsp, cp), lout)
    assert_same_matrix(B, host_route(bmsp, A, rp, cp, lout))
    assert B.info()["num_rows"] == n and B.info()["num_cols"] == m
    assert_unchanged(A, snap)


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("lin,lout", LAYOUTS)
def test_copy_values_replays_a_value_update(bmsp, lin, lout, dtype):
    name = "band203"
    A = build(bmsp, name, lin, dtype)
    p = reference(name, 12345)[2]
    d = dperm(bmsp, p)
    B = A.permute_blocks(d, None, lout)
    v2 = generic_values(name, dtype, seed=21)
    A2 = build(bmsp, name, lin, dtype, v2)
    _write_values(bmsp, A, A2.host_arrays()[3])
    A.invalidate(False)
    B.copy_values_from(A)
    assert_same_matrix(B, A2.permute_blocks(d, None, lout))
    assert_same_matrix(B, host_route(bmsp, A2, p, None, lout))


def test_permutation_refusals_return_nothing_and_leave_the_handles_usable(bmsp):
    L = bmsp.lib()
    A = build(bmsp, "band203", 0, 0)
    snap = snapshot(A)
    good = reference("band203", 0)[2]
    nb = good.size
    dup, far, huge, moved = good.copy(), good.copy(), good.copy(), good.copy()
    dup[1] = dup[0]
    far[2] = nb
    huge[nb // 2] = 0xFFFFFFFF
    moved[[0, nb - 1]] = moved[[nb - 1, 0]]
    dgood = dperm(bmsp, good)
    for bad in (dup, far, huge, moved):
        for args, word in (((dperm(bmsp, bad).ptr, None), "d_row_perm"), ((None, dperm(bmsp, bad).ptr), "d_col_perm"),
                           ((dgood.ptr, dperm(bmsp, bad).ptr), "d_col_perm")):
            out = C.c_void_p()
            assert L.bmsp_matrix_permute_blocks(A.h, args[0], args[1], 1, None, C.byref(out)) == -1
            assert word in L.bmsp_last_error().decode() and out.value is None
        assert_same_matrix(A.permute_blocks(dgood, dgood, 1), host_route(bmsp, A, good, good, 1))
    out = C.c_void_p()
    for lay in (2, -1):
        assert L.bmsp_matrix_permute_blocks(A.h, dgood.ptr, dgood.ptr, lay, None, C.byref(out)) == -1
        assert "out_transposed" in L.bmsp_last_error().decode() and out.value is None
    assert L.bmsp_matrix_permute_blocks(A.h, dgood.ptr, dgood.ptr, 0, None, None) == -1 and "out" in L.bmsp_last_error().decode()
    with pytest.raises(bmsp.BmspError) as e:
        A.row_panel(1, 7).permute_blocks(None, dgood, 0)
    assert e.value.status == -1 and "view" in str(e.value)
    assert_same_matrix(A.permute_blocks(dgood, None, 0), host_route(bmsp, A, good, None, 0))
    assert_unchanged(A, snap)


# ---------------------------------------------------------------------------------------------------------
# 3. the vectors
# ---------------------------------------------------------------------------------------------------------
def block_index(p, n):
    i = np.arange(n)
    return np.asarray(p, np.int64)[i // 8] * 8 + i % 8


@pytest.mark.parametrize("f64", [0, 1])
@pytest.mark.parametrize("n", [200, 203])
def test_vectors_gather_scatter_and_round_trip(bmsp, n, f64):
    R = np.float64 if f64 else np.float32
    p = reference("band%d" % n, 0)[2]
    idx = block_index(p, n)
    x = np.random.default_rng(n + f64).uniform(-2, 2, n).astype(R)
    pad = 13                                                     # entries at and beyond n: never written
    dp, dx = dperm(bmsp, p), bmsp.DeviceArray.from_host(x)

    def poisoned():
        return bmsp.DeviceArray.from_host(np.full(n + pad, np.nan, R))

    y = bmsp.vec_permute_blocks(dp, dx, False, poisoned(), n).to_host()
    assert_same_bits(y[:n], x[idx])
    assert np.isnan(y[n:]).all()
    z = bmsp.vec_permute_blocks(dp, dx, True, poisoned(), n).to_host()
    want = np.empty(n, R)
    want[idx] = x
    assert_same_bits(z[:n], want)
    assert np.isnan(z[n:]).all()
    back = bmsp.vec_permute_blocks(dp, bmsp.DeviceArray.from_host(y[:n].copy()), True, poisoned(), n).to_host()
    assert_same_bits(back[:n], x)
    assert np.isnan(back[n:]).all()
    assert_same_bits(bmsp.vec_permute_blocks(dp, dx).to_host(), x[idx])          # y made by the wrapper


@pytest.mark.parametrize("entry", [26, 0xFFFFFFFF])
@pytest.mark.parametrize("inv", [False, True])
def test_an_entry_out_of_range_moves_nothing_for_its_block(bmsp, inv, entry):
    """the contract of the header: such an entry is skipped and no access outside [0, n) is made (nothing here provokes a fault)"""
    n = 203
    p = reference("band203", 0)[2].copy()
    idx = block_index(p, n)
    p[3] = entry                                                 # (a perm used for this call only)
    x = np.random.default_rng(8).uniform(-2, 2, n).astype(np.float32)
    y = bmsp.vec_permute_blocks(dperm(bmsp, p), bmsp.DeviceArray.from_host(x), inv,
                                bmsp.DeviceArray.from_host(np.full(n + 5, np.nan, np.float32)), n).to_host()
    want = np.full(n + 5, np.nan, np.float32)
    keep = np.arange(n) // 8 != 3
    if inv:
        want[idx[keep]] = x[:n][keep]
    else:
        want[:n][keep] = x[idx[keep]]
    assert_same_bits(y, want)


# ---------------------------------------------------------------------------------------------------------
# 4. end to end: reorder, solve, permute back
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("name", ["band200", "poisson5", "hub"])
def test_reordered_solve_has_colours_many_levels_and_the_reference_bits(bmsp, name, lay, dtype):
    n, r, c = pattern(name)
    rng = np.random.default_rng(11)
    v = (rng.uniform(0.5, 2.0, r.size) * rng.choice([-1.0, 1.0], r.size)).astype(NP[dtype]).astype(np.float64)
    off = r != c
    s = np.maximum(np.bincount(r[off], weights=np.abs(v[off]), minlength=n), np.bincount(c[off], weights=np.abs(v[off]), minlength=n))
    v[~off] = ((1.0 + s) * rng.choice([-1.0, 1.0], n))[r[~off]]             # dominant in its row and in its column
    v = v.astype(NP[dtype]).astype(np.float64)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, transposed=bool(lay), dtype=dtype)
    B, perm, info = A.reorder_multicolor()
    p = perm.to_host()
    np.testing.assert_array_equal(p, reference(name, 0)[2])
    assert info["colors"] == reference(name, 0)[3]
    idx = block_index(p, n)
    r2, c2 = permuted(r, c, p, p)
    b = (rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(VEC[dtype])
    for op in ("N", "T"):
        for fill in ("lower", "upper"):
            natural = plan_levels(bmsp, n, r, c, int(effective_lower(op, fill)))
            assert name != "band200" or natural == 25
            assert bmsp.spsv_analyse(A, op, fill)["levels"] == natural
            assert bmsp.spsv_analyse(B, op, fill)["levels"] == info["colors"]
            bp = bmsp.vec_permute_blocks(perm, bmsp.DeviceArray.from_host(b))
            xp = bmsp.spsv(B, bp, op, fill)
            x = bmsp.vec_permute_blocks(perm, xp, inverse=True).to_host()
            want = np.empty(n, VEC[dtype])
            want[idx] = spsv_reference(n, r2, c2, v, dtype, op, fill, False, 1.0, b[idx])
            assert_same_bits(x, want, (name, op, fill))


# ---------------------------------------------------------------------------------------------------------
# 5. streams
# ---------------------------------------------------------------------------------------------------------
def test_color_blocks_runs_on_its_stream_and_synchronises_it(bmsp):
    """structure arrays of a handle are never gated (tests/test_streams.py): the call is made behind a closed gate, must return only
    after the gate has opened by its timeout, and gives the null-stream result -- with the view missing and with it cached"""
    A = build(bmsp, "band203", 1, 0)
    for _ in range(2):
        s, gate = sg.new_stream(), sg.Gate()
        try:
            gate.close(s)
            got = A.color_blocks(12345, stream=s.value)
            assert gate.opened_by_timeout(), "color_blocks returned while the gate on its stream was closed"
        finally:
            gate.finish()
            sg.destroy_stream(s)
        check_colouring("band203", 12345, got)


def _alt_perm(p):
    return np.r_[p[:-1][::-1], p[-1:]].astype(np.uint32)        # another permutation that keeps the last block


def permute_case():
    n, r, c = pattern("band203")
    p = reference("band203", 0)[2]

    def make(bmsp, alt):
        v = (1 + (3 * r + 7 * c) % 3 + (1 if alt else 0)).astype(np.float64)
        A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, dtype=0)
        rp, cp = dev(bmsp, _alt_perm(p) if alt else p), dev(bmsp, _alt_perm(p) if alt else p)
        return Ops([A.device_arrays()[3], rp, cp], [], A=A, rp=rp, cp=cp)

    return Case("permute_blocks", SYNC, make, lambda bmsp, o, s: o.A.permute_blocks(o.rp, o.cp, 1, stream=s),
                lambda bmsp, o, res: list(res.host_arrays()) + [res.block_row_ptr()])


def vec_case(inv):
    n = 203
    p = reference("band203", 0)[2]

    def make(bmsp, alt):
        x = (1 + np.arange(n) % 4 + (1 if alt else 0)).astype(np.float32)
        dp, dx, dy = dev(bmsp, _alt_perm(p) if alt else p), dev(bmsp, x), bmsp.DeviceArray(n, np.float32)
        return Ops([dp, dx], [dy], p=dp, x=dx, y=dy)

    return Case("vec_permute_blocks_inverse" if inv else "vec_permute_blocks", ASYNC, make,
                lambda bmsp, o, s: bmsp.vec_permute_blocks(o.p, o.x, inv, o.y, n, s), lambda bmsp, o, res: [o.y.to_host()])


@pytest.mark.parametrize("case", [permute_case(), vec_case(False), vec_case(True)], ids=repr)
def test_on_a_gated_non_blocking_stream(bmsp, monkeypatch, case):
    assert run_gated(bmsp, monkeypatch, case) == case.sync


# ---------------------------------------------------------------------------------------------------------
# 6. the C++ surface
# ---------------------------------------------------------------------------------------------------------
def test_cpp_wrappers_run(bmsp, tmp_path):
    """tests/cpp_reorder_check.cpp on band200: its own checks for float, half and double, and the colouring it prints against the reference"""
    n, r, c = pattern("band200")
    v = generic_values("band200", 1)
    mtx = tmp_path / "band200.mtx"
    with open(mtx, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n, r.size))
        for i, j, a in zip(r, c, v):
            f.write("%d %d %.17g\n" % (i + 1, j + 1, a))
    exe = str(tmp_path / "cpp_reorder_check")
    build_cpp_reorder_check(exe)
    out = subprocess.run([exe, str(mtx)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("OK") == 3 and "FAIL" not in out.stdout, out.stdout
    lines = {l.split()[0]: [int(w) for w in l.split()[1:]] for l in out.stdout.splitlines() if l.split()[0] in ("COLORS", "PERM", "INFO")}
    rc, _, rp, n_colors, n_rounds = reference("band200", 0)
    assert lines["COLORS"] == rc.tolist() and lines["PERM"] == rp.tolist() and lines["INFO"] == [rc.size, n_colors, n_rounds]
