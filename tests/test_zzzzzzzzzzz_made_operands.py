"""GPU cases of the made-operand tests: tests/test_made_operands.py holds the generators, the table of chain cases, the numpy models
(check_container, the modelled decisions, the expected routes) and the CPU self-checks these cases rest on, and describes them.

Every matrix a maker returns goes through check_container and gets a twin (M.clone(): the same four arrays on a handle with no cached
fact); every consumer f is applied to both and f(M), f(twin(M)) must agree in every output bit, in the counters of a product's
statistics (everything but t_us) and in the launch reports.  Half of the cases (by the checksum of the case id) take M's outputs first,
the other half the twin's.  Products are also compared with the oracle, chains with the oracle's chain, on keys, bitmaps, offsets,
values and the four stage counters, and every case asserts the route it names from sort_path, sort_long, mac_variant and stage timer 2.
There is no tolerance anywhere.

One route is not what its name says, by the code: F64 has no kernel that works from C's structure alone (mac_choice.h, structure():
neither v15() nor the fp16 strip kernel), so under strip mode's switches an F64 product takes task-list mode; the case asserts that.

The file is named to be collected last: every GPU test that was there before it keeps its place in the order of the suite."""
import zlib
import numpy as np
import pytest

from test_made_operands import (CHAIN, C1_MAKERS, MAKER_W, check_container, expected_route, first_product, second_operand, oracle_chain, square_operand,
                                row_counts)
from test_zzzzzzzz_structure_invalidate import SPGEMM_SWITCHES, switches, same_bits, same_matrix, counters

pytestmark = pytest.mark.gpu

NPDT = {0: np.float32, 1: np.float16, 2: np.float64}
NO_CHECK = -1.0
STAGE_COUNTERS = ("task_list_size", "bmp_reduction", "surviving_tasks", "c_blocks", "c_nnz")


# ---------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------
def twin(M):
    return M.clone()


def m_first(request):
    return zlib.crc32(request.node.callspec.id.encode()) & 1 == 0


def build(bmsp, coo, dtype=0, layout=False):
    return bmsp.BmSpMatrix.from_coo(*coo, transposed=bool(layout), dtype=dtype)


def dev(bmsp, a, dtype):
    return bmsp.DeviceArray.from_host(np.ascontiguousarray(a, dtype=dtype))


def vec(n, k=None, salt=0):
    """multiples of 1/8 between -1.25 and 1.25 that differ from one entry to the next"""
    j = np.arange(n * (k or 1)) + salt
    x = ((j % 21) - 10) / 8.0
    return x if k is None else x.reshape(n, k)


def random_coo(nr, nc, nnz, seed):
    from pybmsp import gen
    _, _, r, c, v = gen.random_coo(nr, nc, nnz, seed=seed)
    return (nr, nc, r, c, v)


def agree(x, y, what):
    """two outputs of one consumer, bit for bit: matrices (with info and block-row pointer; each also passes check_container), device and
    host arrays, statistics and launch reports (dicts, t_us left out), tuples of those"""
    if isinstance(x, (tuple, list)):
        assert len(x) == len(y), what
        for i, (p, q) in enumerate(zip(x, y)):
            agree(p, q, "%s[%d]" % (what, i))
    elif hasattr(x, "host_arrays"):
        assert x.info() == y.info(), (what, x.info(), y.info())
        check_container(x, what)
        same_matrix(x, y, what)
        same_bits(x.block_row_ptr(), y.block_row_ptr(), what + " block-row pointer")
    elif hasattr(x, "to_host"):
        same_bits(x.to_host(), y.to_host(), what)
    elif isinstance(x, np.ndarray):
        same_bits(x, y, what)
    elif isinstance(x, dict):
        assert counters(x) == counters(y), (what, x, y)
    else:
        assert x == y, (what, x, y)


def on_both(request, M, T, consumers):
    """every consumer on M and on its twin, in the order of the case"""
    for name, f in consumers:
        if m_first(request):
            a, b = f(M), f(T)
        else:
            b, a = f(T), f(M)
        agree(a, b, name)


def equals_oracle(Cm, ref, what=""):
    k, b, o, v = Cm.host_arrays()
    np.testing.assert_array_equal(k, ref.keys, err_msg=what)
    np.testing.assert_array_equal(b, ref.bmps, err_msg=what)
    np.testing.assert_array_equal(o, ref.offsets, err_msg=what)
    np.testing.assert_array_equal(v.astype(np.float64), ref.values, err_msg=what)
    want = np.searchsorted((ref.keys >> np.uint64(32)).astype(np.int64), np.arange((ref.num_rows + 7) // 8 + 1))
    np.testing.assert_array_equal(Cm.block_row_ptr(), want.astype(np.uint32), err_msg=what)


def same_counters(st, rst, what=""):
    assert {k: st[k] for k in STAGE_COUNTERS[:3]} == {k: rst[k] for k in STAGE_COUNTERS[:3]}, (what, st, rst)


def first_line(bmsp, M):
    """spmv (default variant), spmv_op N and T, spmm with k = 3, to_csr_device -- with their launch reports"""
    i = M.info()
    nr, nc, dt = i["num_rows"], i["num_cols"], NPDT[i["dtype"]]
    x, y, X = dev(bmsp, vec(nc), dt), dev(bmsp, vec(nr, salt=3), dt), dev(bmsp, vec(nc, 3).ravel(), dt)
    return [
        ("spmv", lambda H: (bmsp.spmv(H, x), bmsp.spmv_launch_info(H))),
        ("spmv_op N", lambda H: (bmsp.spmv_op(H, x, "N"), bmsp.spmv_op_launch_info(H, "N"))),
        ("spmv_op T", lambda H: (bmsp.spmv_op(H, y, "T"), bmsp.spmv_op_launch_info(H, "T"))),
        ("spmm k=3", lambda H: (bmsp.spmm(H, X, 3), bmsp.spmm_launch_info(H, 3))),
        ("to_csr_device", lambda H: H.to_csr_device()),
    ]


# ---------------------------------------------------------------------------------------------------------
# bmsp_spgemm by every symbolic route
# ---------------------------------------------------------------------------------------------------------
def _t2(st):
    return st["t_us"][2]


def _route(path, long=None):
    def ran(st, pair):
        assert st["sort_path"] == path and (long is None or st["sort_long"] == long), st
    return ran


def _strip_after_t2(st, pair):
    _route(2, 1)(st, pair)
    assert pair == "square" or _t2(st) > 0, st     # (the square pair's row maxima bound C1 by 256: T_2 never runs there)


def _strip_without_t2(st, pair):
    _route(2, 1)(st, pair)
    assert _t2(st) == 0, st


# name -> (switches, sort mode, A tiles per block-row of the first operand, how the product is made, what the statistics must show)
SPGEMM_ROUTES = {
    "strip_after_t2": ({"BMSP_SPGEMM_ROWMERGE": "1"}, 0, 8, "whole", _strip_after_t2),
    "strip_surely_fits": ({"BMSP_SPGEMM_ROWMERGE": "1"}, 0, 4, "whole", _strip_without_t2),
    "strip_second_product": ({"BMSP_SPGEMM_ROWMERGE": "1"}, 0, 8, "twice", _strip_without_t2),
    "tasklist": ({"BMSP_SPGEMM_ROWMERGE": "2"}, 0, 8, "whole", _route(2, 2)),
    "windows": ({"BMSP_SPGEMM_ROWWINDOW": "1", "BMSP_WIN_THIN": "1"}, 0, 8, "whole", _route(3)),
    "pipeline_segmented": ({"BMSP_SPGEMM_ROWMERGE": "0"}, 1, 8, "whole", _route(1)),
    "pipeline_global": ({"BMSP_SPGEMM_ROWMERGE": "0"}, 2, 8, "whole", _route(0)),
    "symbolic_numeric": ({"BMSP_SPGEMM_ROWMERGE": "1"}, 0, 8, "split", _route(2, 1)),
    "sharded3": ({}, 0, 8, "sharded", None),
}
F32_V15, F16_V15, F64 = (0, 5), (1, 5), (2, 5)
MAKER_CASES = [(r, F32_V15) for r in SPGEMM_ROUTES] + [(r, n) for n in (F16_V15, F64) for r in ("strip_after_t2", "tasklist", "pipeline_segmented")]


def make_product(bmsp, monkeypatch, route, numerics, A_coo, B_coo, pair):
    """(C1, its statistics, the operand handles): one product by the route, on handles of its own, the route asserted"""
    env, mode, _, how, ran = SPGEMM_ROUTES[route]
    dtype, tc = numerics
    if dtype == 2 and route == "strip_after_t2":
        ran = _route(2, 2)          # no kernel works from C's structure alone for F64: task-list mode (the docstring of the file)
    a, b = build(bmsp, A_coo, dtype, False), build(bmsp, B_coo, dtype, True)
    with switches(monkeypatch, SPGEMM_SWITCHES, env):
        if how == "whole":
            C1, st = bmsp.spgemm(a, b, mode=mode, tc_version=tc)
        elif how == "twice":
            _, st0 = bmsp.spgemm(a, b, mode=mode, tc_version=tc)
            _strip_after_t2(st0, pair)
            C1, st = bmsp.spgemm(a, b, mode=mode, tc_version=tc)
        elif how == "split":
            C1, st = bmsp.spgemm_symbolic(a, b, mode=mode, tc_version=tc)
            t = bmsp.spgemm_numeric(a, b, C1, tc_version=tc)["t_us"]
            assert t[3] == 0 and t[4] == 0 and t[5] == 0 and t[7] > 0, t      # the numeric stage alone, from the stamped structure
        else:
            comm = bmsp.Comm.loopback(3)
            C1, st, sh = bmsp.spgemm_sharded(comm, a, b, mode=mode, tc_version=tc, gather=True)
            assert sh["world"] == 3 and sh["gathered"] == 1, sh
            comm.free()
    if ran is not None:
        ran(st, pair)
    return C1, st, a, b


def oracle_product(oracle, A_coo, B_coo, dtype):
    return oracle.spgemm(oracle.bmsp_from_coo(oracle.Coo(*A_coo), dtype, False), oracle.bmsp_from_coo(oracle.Coo(*B_coo), dtype, True))


def consumers_of_product(oracle, bmsp, C1, oC1, a1, b1, B2_coo, square):
    """section 5 of the issue on one C1: everything but the first line (first_line) and the left-operand product (compared with the
    oracle's chain by the caller)"""
    i = C1.info()
    nr, nc, dtype = i["num_rows"], i["num_cols"], i["dtype"]
    dt, nbr = NPDT[dtype], (i["num_rows"] + 7) // 8
    b2 = build(bmsp, B2_coo, dtype, True)
    L_coo, D_coo = random_coo(40, nr, 300, 21), random_coo(nr, nc, 500, 22)
    D = build(bmsp, D_coo, dtype, False)
    X, Y = dev(bmsp, vec(nr, 3).ravel(), dt), dev(bmsp, vec(nc, 3, salt=5).ravel(), dt)
    rhs = dev(bmsp, vec(nr, salt=1), dt)
    keep = []

    def as_right_operand(H):
        Ht = H.with_layout(True)
        P, st = bmsp.spgemm(build(bmsp, L_coo, dtype, False), Ht)
        return Ht, P, st

    def panel_as_left_operand(H):
        V = H.row_panel(1, nbr - 1)
        keep.append(V)
        P, st = bmsp.spgemm(V, b2)
        return P, st

    def factor(H):
        F, info = bmsp.ilu0(H, max_iter=3, tol=NO_CHECK)
        return F, {k: info[k] for k in ("kernel", "lanes", "sweeps", "view_bytes")}

    out = [
        ("with_layout(True) as the right operand", as_right_operand),
        ("row_panel(1, nbr - 1) as the left operand", panel_as_left_operand),
        ("transpose", lambda H: (H.transpose(False), H.transpose(True))),
        ("add", lambda H: bmsp.add(H, D)),
        ("prune", lambda H: bmsp.prune(H, 0.0)),
        ("diagonal", lambda H: bmsp.diagonal(H)),
        ("sddmm", lambda H: (bmsp.sddmm(H, X, Y, 3), bmsp.sddmm_launch_info(H, 3))),
        ("spgemm_masked", lambda H: (bmsp.spgemm_masked(a1, b1, H), bmsp.spgemm_masked_launch_info(a1, b1, H))),
    ]
    if square:
        out += [
            ("spsv lower N", lambda H: (bmsp.spsv(H, rhs, "N", "lower"), bmsp.spsv_analyse(H, "N", "lower"))),
            ("spsv lower T", lambda H: (bmsp.spsv(H, rhs, "T", "lower"), bmsp.spsv_analyse(H, "T", "lower"))),
            ("ilu0", factor),
            ("aggregate", lambda H: H.aggregate(0)),
            ("color_blocks", lambda H: H.color_blocks(0)),
        ]
    return out, b2


@pytest.mark.parametrize("route,numerics", MAKER_CASES, ids=["%s-%s" % (r, {0: "f32", 1: "f16", 2: "f64"}[n[0]]) for r, n in MAKER_CASES])
def test_spgemm_maker(oracle, bmsp, monkeypatch, request, route, numerics):
    """C1 by the route, from the edge-shaped pair (ragged, empty block-rows first, in the middle and last, one widest block-row) and from
    the square pair (a full diagonal): container, oracle, and every consumer of section 5 on C1 and its twin"""
    dtype, tc = numerics
    a_tiles = SPGEMM_ROUTES[route][2]
    S = square_operand()
    for pair, (A_coo, B_coo) in (("edges", first_product(MAKER_W, a_tiles)), ("square", (S, S))):
        oC1, ost = oracle_product(oracle, A_coo, B_coo, dtype)
        C1, st, a1, b1 = make_product(bmsp, monkeypatch, route, numerics, A_coo, B_coo, pair)
        print(route, numerics, pair, {k: st[k] for k in ("sort_path", "sort_long", "mac_variant", "mac_kernel")}, "T_2 %.1f us" % _t2(st))
        check_container(C1, "%s C1" % pair)
        equals_oracle(C1, oC1, "%s C1" % pair)
        if route == "sharded3":
            assert (st["surviving_tasks"], st["c_blocks"], st["c_nnz"]) == (ost["surviving_tasks"], oC1.block_num, oC1.nnz), (st, ost)
        else:
            same_counters(st, ost, "%s C1" % pair)
            assert (st["c_blocks"], st["c_nnz"]) == (oC1.block_num, oC1.nnz)
        T = twin(C1)
        check_container(T, "%s twin" % pair)
        B2_coo = second_operand(oC1.keys, oC1.num_cols, 4, 200) if pair == "edges" else S
        consumers, b2 = consumers_of_product(oracle, bmsp, C1, oC1, a1, b1, B2_coo, pair == "square")
        with switches(monkeypatch, SPGEMM_SWITCHES, {}):
            on_both(request, C1, T, first_line(bmsp, C1) + consumers)
            # as the left operand of the next product: the twin, and the oracle's chain
            first, second = (C1, T) if m_first(request) else (T, C1)
            (P1, s1), (P2, s2) = bmsp.spgemm(first, b2), bmsp.spgemm(second, b2)
        oC2, ost2 = oracle.spgemm(oC1, oracle.bmsp_from_coo(oracle.Coo(*B2_coo), oC1.dtype, True))
        assert counters(s1) == counters(s2), (s1, s2)
        # both pairs are built so that C1's and B2's widest block-rows bound every block-row of C2 by 256 (edges: 64 x 4): strip mode without
        # T_2 -- but for F64, which has no strip kernel and takes task-list mode
        for s in (s1, s2):
            print(route, numerics, pair, "C1 x B2", {k: s[k] for k in ("sort_path", "sort_long", "mac_variant", "mac_kernel")}, "T_2 %.1f us" % _t2(s))
            assert (s["sort_path"], s["sort_long"], _t2(s) == 0) == ((2, 2, False) if dtype == 2 else (2, 1, True)), s
        agree(P1, P2, "%s C1 x B2" % pair)
        equals_oracle(P1, oC2, "%s C1 x B2" % pair)
        same_counters(s1, ost2, "%s C1 x B2" % pair)
        assert (s1["c_blocks"], s1["c_nnz"]) == (oC2.block_num, oC2.nnz)


# ---------------------------------------------------------------------------------------------------------
# chains on the thresholds the second product reads
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maker", sorted(C1_MAKERS))
@pytest.mark.parametrize("name", sorted(CHAIN))
def test_chain_on_the_threshold(oracle, bmsp, monkeypatch, request, name, maker):
    """C2 = C1 x B2 with (w, b) on or one above a threshold, C1 from strip mode (pointer and maximum written by its scans), from task-list
    mode (the same, by other code), from the column-window passes (the pointer alone) and from the pipeline (both left to the lazy path):
    the route of the second product is the one the true w calls for, on C1 and on its twin; both equal the oracle's chain"""
    w, b, u, env2, mode2 = CHAIN[name]
    A_coo, B_coo, B2_coo, oC1, oC2, ost2 = oracle_chain(oracle, name)
    env1, mode1, (path1, long1) = C1_MAKERS[maker]
    a1, b1 = build(bmsp, A_coo, 0, False), build(bmsp, B_coo, 0, True)
    with switches(monkeypatch, SPGEMM_SWITCHES, env1):
        C1, st1 = bmsp.spgemm(a1, b1, mode=mode1)
    assert st1["sort_path"] == path1 and (long1 is None or st1["sort_long"] == long1), st1
    check_container(C1, "C1")
    equals_oracle(C1, oC1, "C1")
    assert int(np.diff(C1.block_row_ptr()).max()) == w == int(row_counts(oC1.keys).max())
    T = twin(C1)
    b2 = build(bmsp, B2_coo, 0, True)
    first, second = (C1, T) if m_first(request) else (T, C1)
    with switches(monkeypatch, SPGEMM_SWITCHES, env2):
        (P1, s1), (P2, s2) = bmsp.spgemm(first, b2, mode=mode2), bmsp.spgemm(second, b2, mode=mode2)
    want = expected_route(name)
    for st in (s1, s2):
        print(name, maker, {k: st[k] for k in ("sort_path", "sort_long", "mac_variant", "mac_kernel")}, "T_2 %.1f us" % _t2(st))
        assert st["sort_path"] == want["sort_path"], (st, want)
        assert want["sort_long"] is None or st["sort_long"] == want["sort_long"], (st, want)
        assert want["mac_variant"] is None or st["mac_variant"] in want["mac_variant"], (st, want)
        assert want["t2_zero"] is None or (_t2(st) == 0) == want["t2_zero"], (st, want)
        same_counters(st, ost2, "C2")
        assert (st["c_blocks"], st["c_nnz"]) == (oC2.block_num, oC2.nnz)
    assert counters(s1) == counters(s2), (s1, s2)
    agree(P1, P2, "C1 x B2")
    equals_oracle(P1, oC2, "C1 x B2")
    equals_oracle(P2, oC2, "twin(C1) x B2")


# ---------------------------------------------------------------------------------------------------------
# the other makers
# ---------------------------------------------------------------------------------------------------------
G_SHAPE = (77, 93)          # ragged both ways; the random pattern leaves block-rows of different widths


def _other_inputs(bmsp):
    G_coo = random_coo(G_SHAPE[0], G_SHAPE[1], 700, 31)
    return G_coo, build(bmsp, G_coo), build(bmsp, square_operand())


def _make_transpose(bmsp, tmp_path):
    return _other_inputs(bmsp)[1].transpose(False)


def _make_with_layout(bmsp, tmp_path):
    return build(bmsp, _other_inputs(bmsp)[0], 0, True).with_layout(False)


def _make_add(bmsp, tmp_path):
    return bmsp.add(_other_inputs(bmsp)[1], build(bmsp, random_coo(G_SHAPE[0], G_SHAPE[1], 400, 32)), 1.0, -0.5)


def _make_prune(bmsp, tmp_path):
    P, st = bmsp.prune(_other_inputs(bmsp)[1], 0.5)
    assert 0 < st["nnz_out"] < st["nnz_in"] and st["blocks_out"] == P.block_num, st
    return P


def _make_scale(bmsp, tmp_path):
    return bmsp.scale(_other_inputs(bmsp)[1], dev(bmsp, 1.0 + vec(G_SHAPE[0]) / 4, np.float32), dev(bmsp, 2.0 + vec(G_SHAPE[1]) / 4, np.float32))


def _make_from_diagonal(bmsp, tmp_path):
    return bmsp.from_diagonal(dev(bmsp, 1.0 + vec(G_SHAPE[0]) / 4, np.float32))


def _make_sddmm(bmsp, tmp_path):
    X, Y = dev(bmsp, vec(G_SHAPE[0], 3).ravel(), np.float32), dev(bmsp, vec(G_SHAPE[1], 3, salt=5).ravel(), np.float32)
    return bmsp.sddmm(_other_inputs(bmsp)[1], X, Y, 3)


def _make_spgemm_masked(bmsp, tmp_path):
    G = _other_inputs(bmsp)[1]
    H = build(bmsp, random_coo(G_SHAPE[1], G_SHAPE[0], 700, 33), 0, True)
    return bmsp.spgemm_masked(G, H, build(bmsp, random_coo(G_SHAPE[0], G_SHAPE[0], 500, 34)))


def _make_ilu0(bmsp, tmp_path):
    return bmsp.ilu0(_other_inputs(bmsp)[2], max_iter=3, tol=NO_CHECK)[0]


def _make_permute_blocks(bmsp, tmp_path):
    S = _other_inputs(bmsp)[2]
    _, perm, _ = S.color_blocks(0)
    return S.permute_blocks(perm, perm)


def _make_from_aggregates(bmsp, tmp_path):
    agg, num, _ = _other_inputs(bmsp)[2].aggregate(0)
    assert 0 < num < agg.n
    return bmsp.from_aggregates(agg, num)


def _make_save_load(bmsp, tmp_path):
    path = str(tmp_path / "g.bmsp")
    _other_inputs(bmsp)[1].save(path)
    return bmsp.BmSpMatrix.load(path)


def _make_from_csr_device(bmsp, tmp_path):
    return bmsp.BmSpMatrix.from_csr_device(G_SHAPE[0], G_SHAPE[1], *_other_inputs(bmsp)[1].to_csr_device())


OTHER_MAKERS = {"transpose": _make_transpose, "with_layout": _make_with_layout, "add": _make_add, "prune": _make_prune, "scale": _make_scale,
                "from_diagonal": _make_from_diagonal, "sddmm": _make_sddmm, "spgemm_masked": _make_spgemm_masked, "ilu0": _make_ilu0,
                "permute_blocks": _make_permute_blocks, "from_aggregates": _make_from_aggregates, "save_load": _make_save_load,
                "from_csr_device": _make_from_csr_device}


@pytest.mark.parametrize("maker", sorted(OTHER_MAKERS))
def test_other_maker(bmsp, request, tmp_path, maker):
    """one small output of every other maker (row-major tiles): container, and the first line of consumers on it and on its twin"""
    M = OTHER_MAKERS[maker](bmsp, tmp_path)
    assert M.info()["transposed"] == 0 and M.block_num > 0
    check_container(M, maker)
    T = twin(M)
    check_container(T, maker + " twin")
    on_both(request, M, T, first_line(bmsp, M))


# ---------------------------------------------------------------------------------------------------------
# the chain multigrid stands on
# ---------------------------------------------------------------------------------------------------------
def test_amg_galerkin_on_twins(bmsp, monkeypatch):
    """pybmsp.amg.galerkin(A, P) -- a transpose, two products and a layout conversion -- on cusp's 5-point Poisson matrix on a 16 x 16
    grid with the tentative prolongator of its MIS(2) aggregates (from_aggregates): the same chain with every intermediate replaced by
    its twin gives the same coarse operator and restriction, bit for bit"""
    from pybmsp import amg, gen
    n, _, r, c, v = gen.poisson("5pt", 16, 16)
    with switches(monkeypatch, SPGEMM_SWITCHES, {}):
        A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
        agg, num, _ = bmsp.aggregate(A, 0)
        assert 0 < num < n
        P = amg.tentative(A, agg, num)
        assert P.info()["transposed"] == 1
        check_container(P, "P")
        Ac, R = amg.galerkin(A, P)
        Rt = twin(twin(P).transpose(False))
        APt = twin(bmsp.spgemm(twin(A), twin(P))[0])
        AP_col = twin(APt.with_layout(True))
        Act, st = bmsp.spgemm(Rt, AP_col)
    for M, what in ((Ac, "Ac"), (R, "R"), (APt, "A P"), (AP_col, "A P, column-major tiles")):
        check_container(M, what)
    agree(Ac, Act, "the coarse operator")
    agree(R, Rt, "the restriction")
    assert Ac.info()["num_rows"] == Ac.info()["num_cols"] == num
