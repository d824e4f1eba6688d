"""GPU tests of bmsp_matrix_aggregate / bmsp_matrix_from_aggregates and of pybmsp.amg on top of them.  Everything compared is integers or
raw bits, so there is no tolerance except in the last case.  The aggregation is compared with the plain-Python reference of
tests/test_aggregate_api.py (whose self-checks run without a GPU); a prolongator with bmsp_matrix_from_coo on the same triples, all four
arrays and the block-row pointer; the Galerkin product of integer-valued operands with the sums in int64; the whole chain -- hierarchy,
V-cycle, CG -- with the library's own unpreconditioned solver run in the same test."""
import ctypes as C
import subprocess
import numpy as np
import pytest
import stream_gate as sg
from test_aggregate_api import NAMES, SEEDS, SKIP, pattern, values, reference, kernel_name, build_cpp_aggregate_check
from test_transpose import assert_same_arrays, snapshot, assert_unchanged
from test_streams import Case, Ops, run_gated, dev, SYNC

pytestmark = pytest.mark.gpu

NP = {0: np.float32, 1: np.float16, 2: np.float64}
VEC = {0: np.float32, 1: np.float32, 2: np.float64}


def build(bmsp, name, lay, dtype):
    n, r, c = pattern(name)
    return bmsp.BmSpMatrix.from_coo(n, n, r, c, values(name, dtype), transposed=bool(lay), dtype=dtype)


def assert_same_matrix(got, want):
    assert_same_arrays(got, want)
    np.testing.assert_array_equal(got.block_row_ptr(), want.block_row_ptr())


# ---------------------------------------------------------------------------------------------------------
# 1. the aggregation
# ---------------------------------------------------------------------------------------------------------
def check_aggregation(name, seed, lay, got):
    agg, num, info = got
    ra, rnum, rounds, _ = reference(name, seed)
    np.testing.assert_array_equal(agg.to_host(), ra)
    assert (num, info["nodes"], info["aggregates"], info["rounds"]) == (rnum, ra.size, rnum, rounds), (num, info, rnum, rounds)
    assert info["kernel"] == kernel_name(ra.size, lay)
    assert (info["view_bytes"] > 0) == (ra.size > 0)
    assert info["launches"] == (2 * rounds + 4 if ra.size else 0)


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_aggregation_equals_the_reference(bmsp, name, lay, seed, dtype):
    S = build(bmsp, name, lay, dtype)
    snap = snapshot(S)
    check_aggregation(name, seed, lay, S.aggregate(seed))
    check_aggregation(name, seed, lay, bmsp.aggregate(S, seed))                 # the view is cached now
    assert_unchanged(S, snap)


@pytest.mark.parametrize("check", ["1", "3", "1000"])
@pytest.mark.parametrize("name", ["path203", "rand1000", "star530"])
def test_rounds_enqueued_ahead_do_not_change_the_result(bmsp, monkeypatch, name, check):
    monkeypatch.setenv("BMSP_AGG_CHECK", check)
    for seed in SEEDS:
        check_aggregation(name, seed, 0, build(bmsp, name, 0, 0).aggregate(seed))


@pytest.mark.parametrize("name", ["path203", "rand1000", "grid13x11"])
def test_the_other_schedule_gives_the_same_aggregates(bmsp, monkeypatch, name):
    monkeypatch.setenv("BMSP_AGG_SCHEDULE", "separate")
    for seed in SEEDS:
        agg, num, info = build(bmsp, name, 1, 0).aggregate(seed)
        np.testing.assert_array_equal(agg.to_host(), reference(name, seed)[0])
        assert num == reference(name, seed)[1]


@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("one,other", [("lowerpath", "path203"), ("zeros", "grid13x11")])
def test_one_sided_patterns_and_stored_zeros_aggregate_alike(bmsp, one, other, lay):
    for seed in SEEDS:
        a, na, ia = build(bmsp, one, lay, 0).aggregate(seed)
        b, nb_, ib = build(bmsp, other, lay, 0).aggregate(seed)
        np.testing.assert_array_equal(a.to_host(), b.to_host())
        assert (na, ia["rounds"]) == (nb_, ib["rounds"])


def test_aggregation_refusals(bmsp):
    from pybmsp import gen
    L = bmsp.lib()
    S = build(bmsp, "grid13x11", 0, 0)
    with pytest.raises(bmsp.BmspError) as e:
        S.row_panel(2, 9).aggregate()
    assert e.value.status == -1 and ("view" in str(e.value) or "square" in str(e.value))
    n, m, r, c, v = gen.random_coo(203, 96, 1500, seed=6)
    with pytest.raises(bmsp.BmspError) as e:
        bmsp.BmSpMatrix.from_coo(n, m, r, c, v).aggregate()
    assert e.value.status == -1 and "square" in str(e.value)
    agg, count, info = bmsp.DeviceArray(143, np.uint32), C.c_int64(-5), bmsp.AggregateInfo()
    assert L.bmsp_matrix_aggregate(S.h, 0, None, C.byref(count), None, C.byref(info)) == -1 and "d_agg" in L.bmsp_last_error().decode()
    assert L.bmsp_matrix_aggregate(S.h, 0, agg.ptr, None, None, C.byref(info)) == -1 and "num_aggregates" in L.bmsp_last_error().decode()
    assert count.value == -5
    check_aggregation("grid13x11", 0, 0, S.aggregate(0))


# ---------------------------------------------------------------------------------------------------------
# 2. the prolongator
# ---------------------------------------------------------------------------------------------------------
def maps():
    """name -> (num_rows, num_aggregates, agg): the reference maps, and one with skipped rows; sizes that are no multiples of 8"""
    out = {}
    for name in ("grid13x11", "rand1000", "star530"):
        agg, num, _, _ = reference(name, 0)
        out[name] = (agg.size, num, agg)
    rng = np.random.default_rng(5)
    agg = rng.integers(0, 45, 203).astype(np.uint32)
    agg[rng.random(203) < 0.3] = SKIP
    agg[8:16] = SKIP                                                # a whole block-row without entries
    agg[200:] = SKIP                                                # the partial last block-row too
    out["skipped"] = (203, 45, agg)
    return out


MAPS = maps()


def coo_route(bmsp, num_rows, num_agg, agg, w, lay, dtype):
    keep = agg != SKIP
    rows = np.flatnonzero(keep)
    vals = np.ones(rows.size) if w is None else w[keep].astype(np.float64)
    return bmsp.BmSpMatrix.from_coo(num_rows, num_agg, rows, agg[keep].astype(np.int64), vals, transposed=bool(lay), dtype=dtype)


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("lay", [0, 1])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", sorted(MAPS))
def test_prolongator_equals_the_builder_bit_for_bit(bmsp, name, weighted, lay, dtype):
    num_rows, num_agg, agg = MAPS[name]
    if name in ("skipped", "grid13x11"):
        assert num_rows % 8 and num_agg % 8, (num_rows, num_agg)
    w = np.random.default_rng(3).uniform(-2.0, 2.0, num_rows).astype(VEC[dtype]) if weighted else None
    P = bmsp.from_aggregates(dev(bmsp, agg), num_agg, None if w is None else dev(bmsp, w), None, dtype, bool(lay))
    assert_same_matrix(P, coo_route(bmsp, num_rows, num_agg, agg, w, lay, dtype))
    i = P.info()
    assert (i["num_rows"], i["num_cols"], i["nnz"]) == (num_rows, num_agg, int(np.count_nonzero(agg != SKIP)))


def test_prolongator_of_nothing(bmsp):
    for lay in (0, 1):
        P = bmsp.from_aggregates(bmsp.DeviceArray(0, np.uint32), 0, transposed=bool(lay))
        assert_same_matrix(P, bmsp.BmSpMatrix.from_coo(0, 0, [], [], [], transposed=bool(lay)))
        agg = np.full(13, SKIP, np.uint32)
        assert_same_matrix(bmsp.from_aggregates(dev(bmsp, agg), 5, transposed=bool(lay)), coo_route(bmsp, 13, 5, agg, None, lay, 0))


def test_an_entry_out_of_range_is_refused_and_out_is_untouched(bmsp):
    L = bmsp.lib()
    num_rows, num_agg, good = MAPS["skipped"]
    for where, entry in ((0, num_agg), (100, 0xFFFFFFFE), (202, num_agg + 7)):
        bad = good.copy()
        bad[where] = entry
        d = dev(bmsp, bad)
        for lay in (0, 1):
            out = C.c_void_p()
            assert L.bmsp_matrix_from_aggregates(num_rows, num_agg, d.ptr, None, 0, lay, None, C.byref(out)) == -1
            assert "d_agg" in L.bmsp_last_error().decode() and out.value is None
    assert_same_matrix(bmsp.from_aggregates(dev(bmsp, good), num_agg), coo_route(bmsp, num_rows, num_agg, good, None, 0, 0))


# ---------------------------------------------------------------------------------------------------------
# 3. streams
# ---------------------------------------------------------------------------------------------------------
def test_aggregate_runs_on_its_stream_and_synchronises_it(bmsp):
    """structure arrays of a handle are never gated (tests/test_streams.py): the call is made behind a closed gate, must return only
    after the gate has opened by its timeout, and gives the null-stream result -- with the view missing and with it cached"""
    S = build(bmsp, "path203", 1, 0)
    for _ in range(2):
        s, gate = sg.new_stream(), sg.Gate()
        try:
            gate.close(s)
            got = S.aggregate(12345, stream=s.value)
            assert gate.opened_by_timeout(), "aggregate returned while the gate on its stream was closed"
        finally:
            gate.finish()
            sg.destroy_stream(s)
        check_aggregation("path203", 12345, 1, got)


def from_aggregates_case(weighted):
    num_rows, num_agg, agg = MAPS["skipped"]

    def make(bmsp, alt):
        a = np.where(agg == SKIP, agg, (agg + 1) % num_agg).astype(np.uint32) if alt else agg
        ins = [dev(bmsp, a)]
        if weighted:
            ins.append(dev(bmsp, (1 + np.arange(num_rows) % 5 + (1 if alt else 0)).astype(np.float32)))
        return Ops(ins, [], agg=ins[0], w=ins[1] if weighted else None)

    return Case("from_aggregates_weighted" if weighted else "from_aggregates", SYNC, make,
                lambda bmsp, o, s: bmsp.from_aggregates(o.agg, num_agg, o.w, num_rows, 0, True, stream=s),
                lambda bmsp, o, res: list(res.host_arrays()) + [res.block_row_ptr()])


@pytest.mark.parametrize("case", [from_aggregates_case(False), from_aggregates_case(True)], ids=repr)
def test_on_a_gated_non_blocking_stream(bmsp, monkeypatch, case):
    assert run_gated(bmsp, monkeypatch, case) == case.sync


# ---------------------------------------------------------------------------------------------------------
# 4. the set-up on top: Galerkin product, hierarchy, cycle
# ---------------------------------------------------------------------------------------------------------
def test_galerkin_product_of_integer_operands_is_exact(bmsp):
    """A = grid13x11 with 4 / -1, P = the unit-weight prolongator of its reference aggregates, F32: every partial sum of P^T A P is a small
    integer, hence exact in fp32, and equals the sum of A_ij over i in a, j in b computed in int64"""
    from pybmsp import amg
    n, r, c = pattern("grid13x11")
    v = np.where(r == c, 4.0, -1.0)
    agg, num, _, _ = reference("grid13x11", 0)
    want = np.zeros((num, num), np.int64)
    np.add.at(want, (agg[r], agg[c]), v.astype(np.int64))
    for lay_a in (0, 1):
        for lay_p in (0, 1):
            A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, transposed=bool(lay_a), dtype=0)
            P = bmsp.from_aggregates(dev(bmsp, agg), num, transposed=bool(lay_p))
            Ac, R = amg.galerkin(A, P)
            gr, gc, gv = Ac.to_coo()
            got = np.zeros((num, num))
            got[gr, gc] = gv
            np.testing.assert_array_equal(got, want.astype(np.float64))
            assert_same_matrix(R, P.transpose(False))


def test_vcycle_preconditioned_cg_converges_in_fewer_iterations_than_plain_cg(bmsp):
    """F64, Poisson 5pt 32 x 32, a fixed right-hand side, tol 1e-8: amg.build_hierarchy then amg.pcg must return CONVERGED in fewer
    iterations than the library's own unpreconditioned CG run here (the yardstick is the existing solver; no absolute count is asserted).
    The one tolerance of this file: the true residual of the returned x against the tolerance asked for, with a factor 10 for the
    difference between the recurrence's residual and b - A x in float64."""
    from pybmsp import amg, gen
    n, _, r, c, v = gen.poisson("5pt", 32, 32)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, dtype=2)
    b = (1.0 + np.arange(n) % 7).astype(np.float64)
    db = bmsp.DeviceArray.from_host(b)
    _, plain = A.solve(db, "cg", None, tol=1e-8)
    assert plain["status"] == bmsp.KRYLOV_CONVERGED
    levels = amg.build_hierarchy(A)
    sizes = [lv.n for lv in levels]
    assert len(levels) >= 2 and sizes[0] == n and all(a > b_ for a, b_ in zip(sizes, sizes[1:])) and sizes[-1] <= 40, sizes
    x, info = amg.pcg(A, db, levels, tol=1e-8, max_iter=plain["iterations"])
    print("levels", sizes, "V-cycle CG", info, "plain CG", plain["iterations"])
    assert info["status"] == bmsp.KRYLOV_CONVERGED, info
    assert info["iterations"] < plain["iterations"], (info, plain)
    dense = np.zeros((n, n))
    dense[r, c] = v
    assert np.linalg.norm(b - dense @ x.to_host()) <= 10 * 1e-8 * np.linalg.norm(b)


# ---------------------------------------------------------------------------------------------------------
# 5. the C++ surface
# ---------------------------------------------------------------------------------------------------------
def test_cpp_wrappers_run(bmsp, tmp_path):
    """tests/cpp_aggregate_check.cpp on grid13x11: its own checks for float, half and double, and the map it prints against the reference"""
    n, r, c = pattern("grid13x11")
    v = values("grid13x11", 1)
    mtx = tmp_path / "grid13x11.mtx"
    with open(mtx, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n, r.size))
        for i, j, a in zip(r, c, v):
            f.write("%d %d %.17g\n" % (i + 1, j + 1, a))
    exe = str(tmp_path / "cpp_aggregate_check")
    build_cpp_aggregate_check(exe)
    out = subprocess.run([exe, str(mtx)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("OK") == 3 and "FAIL" not in out.stdout, out.stdout
    lines = {l.split()[0]: [int(w) for w in l.split()[1:]] for l in out.stdout.splitlines() if l.split()[0] in ("AGG", "INFO")}
    agg, num, rounds, _ = reference("grid13x11", 0)
    assert lines["AGG"] == agg.tolist() and lines["INFO"] == [n, num, rounds]
