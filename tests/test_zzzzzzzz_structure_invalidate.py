"""GPU cases of the structure-invalidation tests: every family of tests/test_structure_invalidate.py (which holds the inputs, the rewrites,
the hard rule that keeps a stale cache inside its allocations, the table of caches and the CPU self-checks these cases rest on, and
describes them).  One rewrite per case; every case asserts that the kernel or route it pins ran before the rewrite and gave P's result,
and after the rewrite and bmsp_matrix_invalidate(A, 1): bit equality of A's result with that of `fresh` (a handle built from P' by
from_coo), bit equality of both with the reference, and equal launch info / stats.  No case leaves a cache stale on purpose, and there is
no tolerance anywhere.

The file is named to be collected last: every GPU test that was there before it keeps its place in the order of the suite."""
import contextlib
import numpy as np
import pytest

import util
from test_structure_invalidate import (NPDT, OUTDT, CHUNK_VALUES, ITEM_TILES, BACK, READERS, ROUTES, PRODUCT_INPUT, Tiles, pattern, rewrite, mvals, xvec,
                                       spmv_reference, shard_bounds_model, colour_reference, product_operands, oracle_product, params)

pytestmark = pytest.mark.gpu

BMSP_ERR_INVALID = -1
NO_CHECK = -1.0
SPMV_SWITCHES = ("BMSP_SPMV_NOCHUNK", "BMSP_SPMV_RED", "BMSP_SPMV_NO_POSCACHE", "BMSP_SPMV_OLD", "BMSP_SPMV_NO_ROWGROUP", "BMSP_SPMV_CHUNK",
                 "BMSP_SPMV_CHUNK_SORTED", "BMSP_SPMV_GROUP", "BMSP_SPMV_PASSES", "BMSP_SPMV_NT", "BMSP_SPMV_PERSIST", "BMSP_SPMV_OCC",
                 "BMSP_SPMV_POSCACHE_MAX", "BMSP_SPMM_NO_VSTREAM")
SPGEMM_SWITCHES = ("BMSP_MAC_STRIP", "BMSP_MAC_ROWSPARSE", "BMSP_MAC_VALU_DENSE", "BMSP_MAC_F32MFMA", "BMSP_MAC_B_DENSE", "BMSP_MAC_DIRECT", "BMSP_MAC_OLD",
                   "BMSP_MAC_QUOTA", "BMSP_SPGEMM_ROWMERGE", "BMSP_SPGEMM_ROWWINDOW", "BMSP_SEGSORT_WIDE", "BMSP_SEGSORT_READBACK", "BMSP_SEGSORT_RADIX",
                   "BMSP_SEGSORT_NO_MERGE", "BMSP_SEG_AVG_MAX", "BMSP_RM_BUILD_WAVE", "BMSP_RM_DEPTH1", "BMSP_EXPAND_LOOKBACK", "BMSP_STRIP_PROF",
                   "BMSP_WIN_CAND", "BMSP_WIN_CAND_HASH", "BMSP_WIN_THIN")


# ---------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def switches(monkeypatch, known, env):
    """exactly these switches, whatever the caller's environment holds"""
    with monkeypatch.context() as m:
        for k in known:
            m.delenv(k, raising=False)
        for k, v in env.items():
            m.setenv(k, v)
        yield


def build(bmsp, P, dtype=0, layout=False, vals=None):
    nr, nc, r, c = P
    return bmsp.BmSpMatrix.from_coo(nr, nc, r, c, mvals(r, c) if vals is None else vals, transposed=bool(layout), dtype=dtype)


def overwrite(bmsp, A, src):
    """src's four arrays over A's through the public pointers, then bmsp_matrix_invalidate(A, 1): the documented contract.  The hard rule
    is checked on the handles themselves first: same shape, dtype, layout and counts, bit-identical offsets"""
    assert A.info() == src.info(), (A.info(), src.info())
    have, want = A.host_arrays(), src.host_arrays()
    np.testing.assert_array_equal(have[2], want[2])
    assert not np.array_equal(have[0], want[0])
    for dst, s in zip(A.device_arrays(), want):
        assert dst.n == s.size and dst.dtype == s.dtype
        bmsp.check(bmsp.lib().bmsp_memcpy_h2d(dst.ptr, s.ctypes.data, s.nbytes))
    bmsp.synchronize()
    A.invalidate(True)


def dev(bmsp, a, dtype):
    return bmsp.DeviceArray.from_host(np.ascontiguousarray(a, dtype=dtype))


def same_bits(x, y, what=""):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    assert x.dtype == y.dtype and x.shape == y.shape, (what, x.dtype, y.dtype, x.shape, y.shape)
    bad = np.flatnonzero(x.view(np.uint8) != y.view(np.uint8))
    assert bad.size == 0, "%s: %d of %d bytes differ" % (what, bad.size, x.nbytes)


def exactly(got, want, dtype, what=""):
    """a device result against the float64 reference: the output type of the dtype, every element equal (integers: exact)"""
    assert got.dtype == np.dtype(OUTDT[dtype]), (what, got.dtype)
    np.testing.assert_array_equal(got.astype(np.float64).reshape(np.shape(want)), want, err_msg=what)


def same_matrix(Ma, Mb, what=""):
    for name, x, y in zip(("keys", "bmps", "offsets", "values"), Ma.host_arrays(), Mb.host_arrays()):
        same_bits(x, y, "%s %s" % (what, name))


def equals_model(M, t, np_dtype, what=""):
    """a handle's four arrays against the numpy model of the builder on the expected triples"""
    k, b, o, v = M.host_arrays()
    np.testing.assert_array_equal(k, t.keys, err_msg=what)
    np.testing.assert_array_equal(b, t.bmps, err_msg=what)
    np.testing.assert_array_equal(o, t.offsets, err_msg=what)
    same_bits(v, t.values.astype(np_dtype), what + " values")


def counters(st):
    return {k: v for k, v in st.items() if k != "t_us"}


def goes_back(request, family):
    return BACK[family] is not None and request.node.callspec.id == BACK[family]


# ---------------------------------------------------------------------------------------------------------
# SpMV: every launch of util.spmv_launch_params(), rewrites C and Rsplit
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("launch,dtype,rw", params("spmv"))
def test_spmv(bmsp, monkeypatch, request, launch, dtype, rw):
    kind, env, variant, kernel = util.SPMV_LAUNCHES[launch]
    P = pattern(kind)
    Q = rewrite(P, rw)
    nr, nc = P[:2]
    x = xvec(nc)
    dx = dev(bmsp, x, NPDT[dtype])

    def call(M):
        y = bmsp.DeviceArray(nr, OUTDT[dtype])
        bmsp.check(bmsp.lib().bmsp_memset(y.ptr, 0xFF, nr * y.dtype.itemsize))
        bmsp.check(bmsp.lib().bmsp_spmv(M.h, dx.ptr, y.ptr, variant, None))
        return y.to_host()

    def info(M):
        d = bmsp.spmv_launch_info(M, variant)
        assert d["kernel"].startswith(kernel), d
        if launch in util.SPMV_CHUNK_LAYOUT:       # (the two chunk launches share the kernel's name: the layout tells them apart)
            d["chunk_layout"] = bmsp.spmv_chunk_layout(M)
            assert d["chunk_layout"] == util.SPMV_CHUNK_LAYOUT[launch], d
            # the long block-row is folded across chunks: carry slots and counters on top of words, values, records, x and u
            nnz, nch = M.nnz, -(-M.nnz // CHUNK_VALUES)
            assert d["compulsory_bytes"] > 8 * nnz + 32 * nch + 4 * (nr + nc), d
        return d

    with switches(monkeypatch, SPMV_SWITCHES, env):
        A = build(bmsp, P, dtype).prepare(3)
        if kind == "sparse":
            assert int(np.diff(A.block_row_ptr()).max()) > ITEM_TILES
        i0 = info(A)
        exactly(call(A), spmv_reference(P, x), dtype, "before the rewrite")
        fresh = build(bmsp, Q, dtype)
        overwrite(bmsp, A, fresh)
        ya, yf = call(A), call(fresh)
        same_bits(ya, yf, "A against the fresh handle")
        exactly(yf, spmv_reference(Q, x), dtype, "after the rewrite")
        ia, jf = info(A), info(fresh)
        assert ia == jf, (ia, jf)
        same_bits(call(A), yf, "A again")
        if goes_back(request, "spmv"):
            again = build(bmsp, P, dtype)
            overwrite(bmsp, A, again)
            exactly(call(A), spmv_reference(P, x), dtype, "back to P")
            assert info(A) == info(again) == i0


# ---------------------------------------------------------------------------------------------------------
# SpMM: every launch of util.SPMM_LAUNCHES, rewrite C
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("launch,rw", params("spmm"))
def test_spmm(bmsp, monkeypatch, request, launch, rw):
    kind, novs, k, kernel = util.SPMM_LAUNCHES[launch]
    P = pattern(kind)
    Q = rewrite(P, rw)
    nr, nc = P[:2]
    X = xvec(nc, k)
    dX = dev(bmsp, X.ravel(), np.float32)
    call = lambda M: bmsp.spmm(M, dX, k).to_host()
    with switches(monkeypatch, SPMV_SWITCHES, {"BMSP_SPMM_NO_VSTREAM": "1"} if novs else {}):
        A = build(bmsp, P).prepare(3)
        assert bmsp.spmm_launch_info(A, k) == kernel
        exactly(call(A), spmv_reference(P, X), 0, "before the rewrite")
        fresh = build(bmsp, Q)
        overwrite(bmsp, A, fresh)
        ya, yf = call(A), call(fresh)
        same_bits(ya, yf, "A against the fresh handle")
        exactly(yf, spmv_reference(Q, X), 0, "after the rewrite")
        assert bmsp.spmm_launch_info(A, k) == bmsp.spmm_launch_info(fresh, k) == kernel
        assert bmsp.spmv_launch_info(A) == bmsp.spmv_launch_info(fresh)
        if goes_back(request, "spmm"):
            overwrite(bmsp, A, build(bmsp, P))
            exactly(call(A), spmv_reference(P, X), 0, "back to P")
            assert bmsp.spmm_launch_info(A, k) == kernel


# ---------------------------------------------------------------------------------------------------------
# SpGEMM: the block-MAC kernels that read a cache of the operand, and the symbolic routes
# ---------------------------------------------------------------------------------------------------------
def _product_case(oracle, bmsp, monkeypatch, request, family, inp, side, dtype, tc, env, ran):
    """ran(stats): asserts the pinned kernel / route.  The handle under test T is A (side left) or B (right, right_rowptr)"""
    (Pa, va), (Pb, vb) = product_operands(inp, side, False)
    (Qa, wa), (Qb, wb) = product_operands(inp, side, True)
    want0, want1 = oracle_product(oracle, inp, side, False, dtype, tc)[0], oracle_product(oracle, inp, side, True, dtype, tc)[0]
    left = side == "left"
    with switches(monkeypatch, SPGEMM_SWITCHES, env):
        A, B = build(bmsp, Pa, dtype, False, va), build(bmsp, Pb, dtype, True, vb)
        T = A if left else B
        product = (lambda M, L=None: bmsp.spgemm(M, B, tc_version=tc)) if left else (lambda M, L=None: bmsp.spgemm(L or A, M, tc_version=tc))
        T.prepare(3)
        C0, st0 = product(T)
        ran(st0)
        util.assert_bmsp_equal_exact(want0, *C0.host_arrays(), np.float32)
        fresh = build(bmsp, Qa, dtype, False, wa) if left else build(bmsp, Qb, dtype, True, wb)
        overwrite(bmsp, T, fresh)
        # right_rowptr: a fresh left handle per call, its columns relabelled as B's rows were
        La, Lf = (build(bmsp, Qa, dtype, False, wa), build(bmsp, Qa, dtype, False, wa)) if side == "right_rowptr" else (None, None)
        (C1, st1), (Cf, stf) = product(T, La), product(fresh, Lf)
        ran(stf)
        assert counters(st1) == counters(stf), (st1, stf)
        same_matrix(C1, Cf, "the product on T against the fresh handle")
        util.assert_bmsp_equal_exact(want1, *Cf.host_arrays(), np.float32)
        if goes_back(request, family):
            again = build(bmsp, Pa, dtype, False, va) if left else build(bmsp, Pb, dtype, True, vb)
            overwrite(bmsp, T, again)
            (C2, st2), (Cg, stg) = product(T), product(again)
            assert counters(st2) == counters(stg), (st2, stg)
            same_matrix(C2, Cg, "back to P")
            util.assert_bmsp_equal_exact(want0, *C2.host_arrays(), np.float32)


@pytest.mark.parametrize("reader,side", params("spgemm_reader"))
def test_spgemm_reader(oracle, bmsp, monkeypatch, request, reader, side):
    """every entry of test_value_cache_coherence.READERS with its switches: the handle as the left operand under R, as the right one under C"""
    dtype, tc, env, variants, rinp = READERS[reader]

    def ran(st):
        assert st["mac_kernel"] == (tc if dtype == 1 and tc != 5 else 5) and st["mac_variant"] in variants, st
    _product_case(oracle, bmsp, monkeypatch, request, "spgemm_reader", PRODUCT_INPUT[rinp], side, dtype, tc, env, ran)


@pytest.mark.parametrize("route,side", params("spgemm_route"))
def test_spgemm_route(oracle, bmsp, monkeypatch, request, route, side):
    """the four symbolic routes, the handle on either side, and the right operand's block-row pointer under a relabelled left operand"""
    env, (sort_paths, sort_long) = ROUTES[route]

    def ran(st):
        assert st["sort_path"] in sort_paths and (sort_long is None or st["sort_long"] == sort_long), st
    _product_case(oracle, bmsp, monkeypatch, request, "spgemm_route", "square", side, 0, 5, env, ran)


def _numeric_stage_alone(st):
    """the stamps matched: T_7 alone ran, no symbolic stage (as test_value_cache_coherence.py reads the stage timers)"""
    t = st["t_us"]
    return t[3] == 0 and t[4] == 0 and t[5] == 0 and t[7] > 0


@pytest.mark.parametrize("maker,side", params("numeric_stamp"))
def test_numeric_stamp(oracle, bmsp, monkeypatch, maker, side):
    """C from bmsp_spgemm and from bmsp_spgemm_symbolic; an operand is rewritten and invalidated: bmsp_spgemm_numeric refuses the C stamped
    for the other structure with BMSP_ERR_INVALID and leaves its arrays alone; a new whole product is right, and takes the numeric stage.
    `product`: C itself is invalidated and loses its stamps"""
    inp, dtype, tc = "square", 0, 5
    op_side = "left" if side == "product" else side
    (Pa, va), (Pb, vb) = product_operands(inp, op_side, False)
    (Qa, wa), (Qb, wb) = product_operands(inp, op_side, True)
    want0, want1 = oracle_product(oracle, inp, op_side, False, dtype, tc)[0], oracle_product(oracle, inp, op_side, True, dtype, tc)[0]
    with switches(monkeypatch, SPGEMM_SWITCHES, {}):
        A, B = build(bmsp, Pa, dtype, False, va), build(bmsp, Pb, dtype, True, vb)
        C, _ = bmsp.spgemm(A, B, tc_version=tc) if maker == "spgemm" else bmsp.spgemm_symbolic(A, B, tc_version=tc)
        st = bmsp.spgemm_numeric(A, B, C, tc_version=tc)
        assert _numeric_stage_alone(st), st
        util.assert_bmsp_equal_exact(want0, *C.host_arrays(), np.float32)
        if side == "product":
            # C's own structure is declared changed (its arrays stay): stamps and the kept task list are gone, so the call takes the checked
            # path -- the whole product, compared with C's structure -- exactly as for a C adopted from copies of the arrays, never stamped
            i = C.info()
            fresh = bmsp.BmSpMatrix.from_arrays(i["num_rows"], i["num_cols"], *C.host_arrays(), dtype=i["dtype"], transposed=i["transposed"])
            C.invalidate(True)
            st1, stf = bmsp.spgemm_numeric(A, B, C, tc_version=tc), bmsp.spgemm_numeric(A, B, fresh, tc_version=tc)
            assert not _numeric_stage_alone(st1) and sum(st1["t_us"][1:7]) > 0, st1
            assert counters(st1) == counters(stf), (st1, stf)
            same_matrix(C, fresh, "C against the adopted copy")
            util.assert_bmsp_equal_exact(want0, *C.host_arrays(), np.float32)
            return
        T, fresh = (A, build(bmsp, Qa, dtype, False, wa)) if side == "left" else (B, build(bmsp, Qb, dtype, True, wb))
        overwrite(bmsp, T, fresh)
        held = C.host_arrays()
        with pytest.raises(bmsp.BmspError) as e:
            bmsp.spgemm_numeric(A, B, C, tc_version=tc)
        assert e.value.status == BMSP_ERR_INVALID and "stamp" in str(e.value), str(e.value)
        for x, y in zip(held, C.host_arrays()):
            same_bits(x, y, "C after the refused call")
        (C1, st1), (Cf, stf) = bmsp.spgemm(A, B, tc_version=tc), (bmsp.spgemm(fresh, B, tc_version=tc) if side == "left" else bmsp.spgemm(A, fresh, tc_version=tc))
        assert counters(st1) == counters(stf), (st1, stf)
        same_matrix(C1, Cf, "the new product against the fresh handle")
        util.assert_bmsp_equal_exact(want1, *C1.host_arrays(), np.float32)
        st = bmsp.spgemm_numeric(A, B, C1, tc_version=tc)
        assert _numeric_stage_alone(st), st
        util.assert_bmsp_equal_exact(want1, *C1.host_arrays(), np.float32)


# ---------------------------------------------------------------------------------------------------------
# the sharded SpMV's cached panel view and bounds
# ---------------------------------------------------------------------------------------------------------
SHARD_FIELDS = ("world", "rank", "panel_block_row_begin", "panel_block_row_end", "panel_tasks", "exchange_bytes")


@pytest.mark.parametrize("world,rw", params("sharded_spmv"))
def test_sharded_spmv(bmsp, monkeypatch, request, world, rw):
    P = pattern("sparse")
    Q = rewrite(P, rw)
    nr, nc = P[:2]
    x = xvec(nc)
    dx = dev(bmsp, x, np.float32)
    comm = bmsp.Comm.loopback(world)

    def call(M, T):
        out = []
        for _ in range(2):      # the second call reuses the cached panel view and bounds
            y = bmsp.DeviceArray.from_host(np.full(nr, np.nan, np.float32))
            _, sh = bmsp.spmv_sharded(comm, M, dx, y)
            out.append((y.to_host(), {k: sh[k] for k in SHARD_FIELDS}))
            assert sh["world"] == world and sh["panel_block_row_end"] == shard_bounds_model(Tiles(T, 0), world)[1], sh
        same_bits(out[0][0], out[1][0], "the second call")
        assert out[0][1] == out[1][1]
        return out[0]

    with switches(monkeypatch, SPMV_SWITCHES, {}):
        A = build(bmsp, P).prepare(3)
        y0, _ = call(A, P)
        exactly(y0, spmv_reference(P, x), 0, "before the rewrite")
        fresh = build(bmsp, Q)
        overwrite(bmsp, A, fresh)
        (ya, sa), (yf, sf) = call(A, Q), call(fresh, Q)
        same_bits(ya, yf, "A against the fresh handle")
        exactly(yf, spmv_reference(Q, x), 0, "after the rewrite")
        assert sa == sf, (sa, sf)
        if goes_back(request, "sharded_spmv"):
            overwrite(bmsp, A, build(bmsp, P))
            exactly(call(A, P)[0], spmv_reference(P, x), 0, "back to P")
    comm.free()


# ---------------------------------------------------------------------------------------------------------
# the readers of the block-row pointer: to_csr_device, prune (ROW_REL), row_absmax, diagonal
# ---------------------------------------------------------------------------------------------------------
def _rowptr_call(bmsp, reader, M):
    if reader == "to_csr_device":
        return [a.to_host() for a in M.to_csr_device()], None
    if reader == "prune_row_rel":
        out, st = bmsp.prune(M, 0.5, "row_rel")
        return list(out.host_arrays()) + [out.block_row_ptr()], st
    if reader == "row_absmax":
        return [bmsp.row_absmax(M).to_host()], None
    return [bmsp.diagonal(M).to_host()], None


def _rowptr_reference(reader, T):
    nr, nc, r, c = T
    v = mvals(r, c)
    o = np.lexsort((c, r))
    rowmax = np.zeros(nr)
    np.maximum.at(rowmax, r, v)
    if reader == "to_csr_device":
        return [np.searchsorted(r[o], np.arange(nr + 1)).astype(np.int32), c[o].astype(np.int32), v[o]], None
    if reader == "prune_row_rel":        # |v| <= 0.5 * rowmax(row) goes: 1 beside a 2 or a 3 (0.5 * 2 and 0.5 * 3 are exact)
        keep = ~(v <= 0.5 * rowmax[r])
        t = Tiles((nr, nc, r[keep], c[keep]), 0, v[keep])
        st = {"nnz_in": r.size, "nnz_out": int(keep.sum()), "blocks_in": Tiles(T, 0).keys.size, "blocks_out": t.keys.size}
        assert 0 < st["nnz_out"] < st["nnz_in"]
        return [t.keys, t.bmps, t.offsets, t.values.astype(np.float32), t.rowptr.astype(np.uint32)], st
    if reader == "row_absmax":
        return [rowmax.astype(np.float32)], None
    d = np.zeros(min(nr, nc), np.float32)
    d[r[r == c]] = v[r == c]
    return [d], None


@pytest.mark.parametrize("reader,rw", params("rowptr_reader"))
def test_rowptr_reader(bmsp, request, reader, rw):
    P = pattern("square" if reader == "diagonal" else "sparse")
    Q = rewrite(P, rw)

    def check(M, T, what):
        got, st = _rowptr_call(bmsp, reader, M)
        want, wst = _rowptr_reference(reader, T)
        assert st == wst, (what, st, wst)
        for g, w in zip(got, want):
            same_bits(g, w, what)
        np.testing.assert_array_equal(M.block_row_ptr(), Tiles(T, 0).rowptr, err_msg=what)
        return got

    A = build(bmsp, P).prepare(3)
    np.testing.assert_array_equal(A.block_row_ptr(), Tiles(P, 0).rowptr)       # the cache exists and is P's
    check(A, P, "before the rewrite")
    fresh = build(bmsp, Q)
    overwrite(bmsp, A, fresh)
    ga, gf = check(A, Q, "after the rewrite"), check(fresh, Q, "the fresh handle")
    for x, y in zip(ga, gf):
        same_bits(x, y, "A against the fresh handle")
    if goes_back(request, "rowptr_reader"):
        overwrite(bmsp, A, build(bmsp, P))
        check(A, P, "back to P")


# ---------------------------------------------------------------------------------------------------------
# the sweeps: spitsv (plans, second iterate, op view) and ilu0_values (diagonal index, second iterate, op-T view of F)
# ---------------------------------------------------------------------------------------------------------
def _dominant(T):
    """(n, r, c, v) sorted by (row, col): off-diagonal values 1..3, the diagonal 1 + the row's off-diagonal sum (exact in fp32)"""
    n, _, r, c = T
    o = np.lexsort((c, r))
    r, c = r[o], c[o]
    v = mvals(r, c)
    off = r != c
    s = np.bincount(r[off], weights=v[off], minlength=n)
    v[~off] = 1.0 + s[r[~off]]
    return n, r, c, v


def _dominant_matrix(bmsp, T):
    n, r, c, v = _dominant(T)
    return bmsp.BmSpMatrix.from_coo(n, n, r, c, v)


@pytest.mark.parametrize("sweeps,rw", params("spitsv"))
def test_spitsv(bmsp, request, sweeps, rw):
    """bmsp_spitsv, BMSP_ITSV_NO_CHECK, three sweeps, on the square pattern with a stored diagonal: bit for bit the C reference of
    tests/test_spitsv_api.py on the triples"""
    from test_spitsv_api import ref_sweeps
    P = pattern("diag")
    Q = rewrite(P, rw)
    b = xvec(P[0]).astype(np.float32)
    db = dev(bmsp, b, np.float32)

    def call(M):
        x, info = bmsp.spitsv(M, db, "N", "lower", False, 1.0, max_iter=sweeps, tol=NO_CHECK)
        assert info["kernel"].startswith("spitsv_sweep_kernel<F32") and info["sweeps"] == sweeps, info
        return x.to_host(), info

    def reference(T):
        n, r, c, v = _dominant(T)
        want, ws, *_ = ref_sweeps(n, r, c, v, 0, "N", "lower", False, 1.0, b, sweeps, NO_CHECK)
        assert ws == sweeps
        return want

    mk = lambda T: _dominant_matrix(bmsp, T)
    A = mk(P).prepare(3)
    x0, i0 = call(A)
    same_bits(x0, reference(P), "before the rewrite")
    fresh = mk(Q)
    overwrite(bmsp, A, fresh)
    (xa, ia), (xf, jf) = call(A), call(fresh)
    same_bits(xa, xf, "A against the fresh handle")
    same_bits(xf, reference(Q), "after the rewrite")
    assert ia == jf, (ia, jf)
    assert not np.array_equal(x0, xf)
    if goes_back(request, "spitsv"):
        overwrite(bmsp, A, mk(P))
        xb, ib = call(A)
        same_bits(xb, x0, "back to P")
        assert ib == i0


@pytest.mark.parametrize("sweeps,rw", params("ilu0_values"))
def test_ilu0_values(bmsp, sweeps, rw):
    """bmsp_matrix_ilu0_values, BMSP_ILU_NO_CHECK, three sweeps.  The caches of the sweeps live on F, and an F whose source's structure was
    declared changed is refused (bmsp.h): after the rewrite of A the old F is refused with BMSP_ERR_INVALID and keeps its values, and the
    sweeps into an F made from the rewritten A give the bits of the fresh handle's and of the C reference of tests/test_ilu0_api.py"""
    from test_ilu0_api import Csr, ref_sweeps
    P = pattern("diag")
    Q = rewrite(P, rw)

    def stored(F):
        r, c, v = F.to_coo()
        o = np.lexsort((c, r))
        return np.ascontiguousarray(v[o].astype(np.float32))

    def reference(T):
        n, r, c, v = _dominant(T)
        want, ws, *_ = ref_sweeps(Csr(n, r, c), v, 0, sweeps, NO_CHECK)
        assert ws == sweeps
        return want

    def call(M, F):
        _, info = bmsp.ilu0_values(M, F, max_iter=sweeps, tol=NO_CHECK)
        assert info["kernel"].startswith("ilu0_sweep_kernel<F32") and info["sweeps"] == sweeps, info
        return stored(F), info

    mk = lambda T: _dominant_matrix(bmsp, T)
    A = mk(P).prepare(3)
    F = A.with_layout(0)
    f0, i0 = call(A, F)
    same_bits(f0, reference(P), "before the rewrite")
    fresh = mk(Q)
    overwrite(bmsp, A, fresh)
    with pytest.raises(bmsp.BmspError) as e:
        bmsp.ilu0_values(A, F, max_iter=sweeps, tol=NO_CHECK)
    assert e.value.status == BMSP_ERR_INVALID and "structure changed" in str(e.value), str(e.value)
    same_bits(stored(F), f0, "F after the refused call")
    (fa, ia), (ff, jf) = call(A, A.with_layout(0)), call(fresh, fresh.with_layout(0))
    same_bits(fa, ff, "A against the fresh handle")
    same_bits(ff, reference(Q), "after the rewrite")
    assert ia == jf, (ia, jf)
    G, ig = bmsp.ilu0(A, max_iter=sweeps, tol=NO_CHECK)
    same_bits(stored(G), ff, "bmsp_matrix_ilu0 on the rewritten A")


# ---------------------------------------------------------------------------------------------------------
# colouring and block permutation
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,rw", params("color_permute"))
def test_color_permute(bmsp, request, seed, rw):
    from test_reorder_api import permuted
    P = pattern("square")
    Q = rewrite(P, rw)

    def check(M, T, what):
        colors, perm, info = M.color_blocks(seed)
        wc, wp, n_colors, n_rounds = colour_reference(T, seed)
        np.testing.assert_array_equal(colors.to_host(), wc, err_msg=what)
        np.testing.assert_array_equal(perm.to_host(), wp, err_msg=what)
        assert (info["blocks"], info["colors"], info["rounds"]) == (wc.size, n_colors, n_rounds) and info["kernel"].startswith("color_round_kernel"), info
        B = M.permute_blocks(perm, perm)
        n, _, r, c = T
        r2, c2 = permuted(r, c, wp, wp)
        t = Tiles((n, n, r2, c2), 0, mvals(r, c))
        equals_model(B, t, np.float32, what)
        np.testing.assert_array_equal(B.block_row_ptr(), t.rowptr, err_msg=what)
        return colors.to_host(), info, B

    A = build(bmsp, P).prepare(3)
    c0, _, _ = check(A, P, "before the rewrite")
    fresh = build(bmsp, Q)
    overwrite(bmsp, A, fresh)
    (ca, ia, Ba), (cf, jf, Bf) = check(A, Q, "after the rewrite"), check(fresh, Q, "the fresh handle")
    same_bits(ca, cf, "colours of A against the fresh handle")
    same_matrix(Ba, Bf, "the permuted matrix of A against the fresh handle")
    assert ia == jf, (ia, jf)
    assert not np.array_equal(c0, cf)
    if goes_back(request, "color_permute"):
        overwrite(bmsp, A, build(bmsp, P))
        check(A, P, "back to P")
