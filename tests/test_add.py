"""GPU tests of the sparse addition C = alpha*A + beta*B (bmsp_matrix_add / bmsp_matrix_add_values): structure against the oracle's
build of the concatenated COO [fl(alpha*a); fl(beta*b)] in C's layout, values against that build bit for bit (F32 / F64) and against a
numpy emulation of the semantics (all dtypes: fp32 / fp64 products and sum, fp16 rounded once from fp32); at full size against the
library's own builder of the concatenated device COO."""
import ctypes as C
import itertools
import os
import numpy as np
import pytest
import util
from stream_gate import _hip
from test_transpose import entries, assert_same_arrays, snapshot, assert_unchanged, _write_values

pytestmark = pytest.mark.gpu

NPDT = {0: np.float32, 1: np.float16, 2: np.float64}
UINT = {0: np.uint32, 1: np.uint16, 2: np.uint64}
ARITH = {0: np.float32, 1: np.float32, 2: np.float64}
LAYOUTS3 = list(itertools.product((0, 1), repeat=3))  # (A layout, B layout, C layout)


def stored(M):
    """(rows, cols, values) of every stored entry of a device matrix, values in its storage dtype"""
    k, b, o, v = M.host_arrays()
    r, c, idx = entries(k, b, o, M.info()["transposed"])
    return r, c, v[idx]


def scaled(s, v, dtype):
    F = ARITH[dtype]
    with np.errstate(all="ignore"):
        return F(s) * v.astype(F)


def emulate(A, B, alpha, beta, dtype):
    """the semantics in numpy: (sorted linear coordinates of C, values in the storage dtype), plus the concatenated scaled COO"""
    nc = A.num_cols
    ra, ca, va = stored(A)
    rb, cb, vb = stored(B)
    sa, sb = scaled(alpha, va, dtype), scaled(beta, vb, dtype)
    ka, kb = ra * nc + ca, rb * nc + cb
    oa, ob = np.argsort(ka), np.argsort(kb)
    ka, kb, sa_s, sb_s = ka[oa], kb[ob], sa[oa], sb[ob]
    keys = np.union1d(ka, kb)
    pa = np.minimum(np.searchsorted(ka, keys), max(ka.size - 1, 0))
    pb = np.minimum(np.searchsorted(kb, keys), max(kb.size - 1, 0))
    ha = (ka[pa] == keys) if ka.size else np.zeros(keys.size, bool)
    hb = (kb[pb] == keys) if kb.size else np.zeros(keys.size, bool)
    out = np.zeros(keys.size, ARITH[dtype])
    with np.errstate(all="ignore"):
        out[ha & ~hb] = sa_s[pa[ha & ~hb]]
        out[hb & ~ha] = sb_s[pb[hb & ~ha]]
        out[ha & hb] = sa_s[pa[ha & hb]] + sb_s[pb[ha & hb]]
        want = out.astype(NPDT[dtype])
    coo = (np.concatenate([ra, rb]), np.concatenate([ca, cb]), np.concatenate([sa, sb]).astype(np.float64))
    return keys, want, coo


def assert_same_values(got, want, dtype):
    """bit for bit, except that a NaN only has to be a NaN"""
    assert got.shape == want.shape
    gn, wn = np.isnan(got.astype(np.float64)), np.isnan(want.astype(np.float64))
    np.testing.assert_array_equal(gn, wn)
    np.testing.assert_array_equal(got[~gn].view(UINT[dtype]), want[~wn].view(UINT[dtype]))


def check_structure(C_, ref):
    i = C_.info()
    assert (i["num_rows"], i["num_cols"], i["nnz"], i["block_num"], i["transposed"]) == \
        (ref.num_rows, ref.num_cols, ref.nnz, ref.block_num, ref.transposed)
    k, b, o, _ = C_.host_arrays()
    np.testing.assert_array_equal(k, ref.keys)
    np.testing.assert_array_equal(b, ref.bmps)
    np.testing.assert_array_equal(o, ref.offsets)
    nbr = (ref.num_rows + 7) // 8
    exp = np.searchsorted((ref.keys >> np.uint64(32)).astype(np.int64), np.arange(nbr + 1), side="left")
    np.testing.assert_array_equal(C_.block_row_ptr(), exp.astype(np.uint32))


def check_add(oracle, bmsp, A, B, alpha, beta, lay, oracle_values=True):
    """C = add(A, B) against the oracle's build and the emulation; A and B unchanged.  Returns (C, the oracle's build)."""
    dtype = A.dtype
    snaps = (snapshot(A), snapshot(B))
    C_ = bmsp.add(A, B, alpha, beta, transposed=lay)
    assert_unchanged(A, snaps[0])
    assert_unchanged(B, snaps[1])
    keys, want, (r, c, v) = emulate(A, B, alpha, beta, dtype)
    ref = oracle.bmsp_from_coo(oracle.Coo(A.num_rows, A.num_cols, r, c, v), dtype, lay)
    check_structure(C_, ref)
    k, b, o, cv = C_.host_arrays()
    if oracle_values and dtype != bmsp.F16:
        util.assert_bmsp_equal_exact(ref, k, b, o, cv, NPDT[dtype])
    rr, cc, idx = entries(k, b, o, lay)
    lin = rr * A.num_cols + cc
    order = np.argsort(lin)
    np.testing.assert_array_equal(lin[order], keys)
    assert_same_values(cv[idx][order], want, dtype)
    return C_, ref


def build(bmsp, nr, nc, r, c, v, lay, dtype):
    return bmsp.BmSpMatrix.from_coo(nr, nc, r, c, v, transposed=lay, dtype=dtype)


# ---------------------------------------------------------------------------------------------------------
# 1. layouts x dtypes
# ---------------------------------------------------------------------------------------------------------
def _overlapping_pair(nr, nc, seed):
    from pybmsp import gen
    _, _, r1, c1, v1 = gen.random_coo(nr, nc, nr * nc // 6, seed=seed)
    _, _, r2, c2, v2 = gen.random_coo(nr, nc, nr * nc // 6, seed=seed + 100)
    # a shared part: half of A's entries also stored in B (with other values)
    r2, c2 = np.concatenate([r2, r1[::2]]), np.concatenate([c2, c1[::2]])
    v2 = np.concatenate([v2, -0.5 * v1[::2] + 0.25])
    return (r1, c1, v1), (r2, c2, v2)


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_all_layout_combinations(oracle, bmsp, dtype):
    nr, nc = 203, 157
    (r1, c1, v1), (r2, c2, v2) = _overlapping_pair(nr, nc, 3)
    for la, lb, lc in LAYOUTS3:
        A, B = build(bmsp, nr, nc, r1, c1, v1, la, dtype), build(bmsp, nr, nc, r2, c2, v2, lb, dtype)
        check_add(oracle, bmsp, A, B, 1.5, -0.75, lc)
        check_add(oracle, bmsp, A, B, 1.0, 1.0, lc)


def test_default_output_layout_is_as(oracle, bmsp):
    (r1, c1, v1), (r2, c2, v2) = _overlapping_pair(40, 50, 5)
    for la in (0, 1):
        A, B = build(bmsp, 40, 50, r1, c1, v1, la, 0), build(bmsp, 40, 50, r2, c2, v2, 1 - la, 0)
        assert bmsp.add(A, B).info()["transposed"] == la


# ---------------------------------------------------------------------------------------------------------
# 2. fixtures
# ---------------------------------------------------------------------------------------------------------
def _mtx_shape(path):
    with open(path) as f:
        for ln in f:
            if not ln.startswith("%") and ln.strip():
                return tuple(int(x) for x in ln.split()[:2])


def _fixture_pairs():
    by_shape = {}
    for p in util.all_fixture_mtx():
        by_shape.setdefault(_mtx_shape(p), []).append(p)
    pairs = []
    for paths in by_shape.values():
        pairs += list(itertools.combinations(paths, 2)) + [(p, p) for p in paths[:1]]
    return pairs


def _short(p):
    return os.path.relpath(p, util.MTX)


@pytest.mark.parametrize("pa,pb", _fixture_pairs(), ids=lambda p: _short(p))
def test_fixture_pairs(oracle, bmsp, pa, pb):
    for dtype in (0, 1, 2):
        for la, lb, lc in ((0, 0, 0), (0, 1, 1), (1, 0, 0), (1, 1, 1)):
            A = bmsp.BmSpMatrix.from_mtx(pa, transposed=la, dtype=dtype)
            B = bmsp.BmSpMatrix.from_mtx(pb, transposed=lb, dtype=dtype)
            check_add(oracle, bmsp, A, B, 2.0, -0.5, lc)


def test_real_fixture_pair_present():
    names = {(_short(a), _short(b)) for a, b in _fixture_pairs()}
    assert (os.path.join("real", "A_matrix.mtx"), os.path.join("real", "B_matrix.mtx")) in names
    assert any(a.endswith("000_nonzeros.mtx") or b.endswith("000_nonzeros.mtx") for a, b in names)


# ---------------------------------------------------------------------------------------------------------
# 3. edge shapes and pattern relations
# ---------------------------------------------------------------------------------------------------------
def _edge_cases():
    from pybmsp import gen
    rng = np.random.default_rng(11)
    e = np.zeros(0, np.int64)
    cases = {
        "1x1": (1, 1, ([0], [0], [2.5]), ([0], [0], [-1.25])),
        "1x1_one_empty": (1, 1, ([0], [0], [2.5]), (e, e, np.zeros(0))),
        "both_empty": (37, 11, (e, e, np.zeros(0)), (e, e, np.zeros(0))),
    }
    for nr, nc in ((1, 300), (300, 1), (13, 29), (29, 13), (61, 61)):
        _, _, r1, c1, v1 = gen.random_coo(nr, nc, max(1, nr * nc // 4), seed=nr)
        _, _, r2, c2, v2 = gen.random_coo(nr, nc, max(1, nr * nc // 5), seed=nc + 7)
        cases["%dx%d" % (nr, nc)] = (nr, nc, (r1, c1, v1), (r2, c2, v2))
    cases["61x61_b_empty"] = (61, 61, cases["61x61"][2], (e, e, np.zeros(0)))
    cases["61x61_a_empty"] = (61, 61, (e, e, np.zeros(0)), cases["61x61"][3])
    # disjoint tiles: A in even block columns, B in odd ones
    n = 80
    rr, cc = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    rr, cc = rr.ravel(), cc.ravel()
    sel = rng.random(rr.size) < 0.2
    even = (cc // 8) % 2 == 0
    cases["disjoint_tiles"] = (n, n, (rr[sel & even], cc[sel & even], rng.uniform(-1, 1, (sel & even).sum())),
                               (rr[sel & ~even], cc[sel & ~even], rng.uniform(-1, 1, (sel & ~even).sum())))
    # same tiles, disjoint bits: A on even columns, B on odd columns, both in every tile
    evc = cc % 2 == 0
    cases["same_tiles_disjoint_bits"] = (n, n, (rr[sel & evc], cc[sel & evc], rng.uniform(-1, 1, (sel & evc).sum())),
                                         (rr[sel & ~evc], cc[sel & ~evc], rng.uniform(-1, 1, (sel & ~evc).sum())))
    # identical patterns, other values
    cases["identical"] = (n, n, (rr[sel], cc[sel], rng.uniform(-1, 1, sel.sum())), (rr[sel], cc[sel], rng.uniform(-1, 1, sel.sum())))
    # nested: B's pattern inside A's (and the reverse)
    sub = sel & (rng.random(rr.size) < 0.5)
    cases["nested_b_in_a"] = (n, n, (rr[sel], cc[sel], rng.uniform(-1, 1, sel.sum())), (rr[sub], cc[sub], rng.uniform(-1, 1, sub.sum())))
    cases["nested_a_in_b"] = (n, n, cases["nested_b_in_a"][3], cases["nested_b_in_a"][2])
    # full tiles plus a diagonal (A - 0.5 I on a banded matrix)
    nb, _, r, c, v = gen.banded(300, 12)
    d = np.arange(nb)
    cases["banded_minus_identity"] = (nb, nb, (r, c, v), (d, d, np.ones(nb)))
    return cases


_EDGES = _edge_cases()


@pytest.mark.parametrize("name", sorted(_EDGES))
def test_edge_shapes_and_patterns(oracle, bmsp, name):
    nr, nc, (r1, c1, v1), (r2, c2, v2) = _EDGES[name]
    for dtype in (0, 1, 2):
        for la, lb, lc in ((0, 0, 0), (1, 0, 1), (0, 1, 0), (1, 1, 0)):
            A, B = build(bmsp, nr, nc, r1, c1, v1, la, dtype), build(bmsp, nr, nc, r2, c2, v2, lb, dtype)
            check_add(oracle, bmsp, A, B, 1.0, -0.5, lc)


def test_cancellation_keeps_structure(oracle, bmsp):
    """A + (-A): every entry of A stored, every value zero"""
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(11, 4)
    for dtype in (0, 1, 2):
        for la, lb, lc in LAYOUTS3:
            A, B = build(bmsp, n, n, r, c, v, la, dtype), build(bmsp, n, n, r, c, v, lb, dtype)
            C_, _ = check_add(oracle, bmsp, A, B, 1.0, -1.0, lc)
            assert C_.nnz == A.nnz and C_.block_num == A.block_num
            assert not np.any(C_.host_arrays()[3])


def test_same_handle_twice(oracle, bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.fem_like(6, "27pt")
    for dtype in (0, 1, 2):
        for la in (0, 1):
            A = build(bmsp, n, n, r, c, v, la, dtype)
            for lc in (0, 1):
                C_, _ = check_add(oracle, bmsp, A, A, 0.75, 2.5, lc)
                assert C_.block_num == A.block_num and C_.nnz == A.nnz


# ---------------------------------------------------------------------------------------------------------
# 4. special values
# ---------------------------------------------------------------------------------------------------------
def _specials(dtype, n, rng):
    """n raw values: ordinary numbers with -0, +0, +-Inf, NaNs, subnormals and values near the top of the range mixed in"""
    T = NPDT[dtype]
    fi = np.finfo(T)
    pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, float(fi.tiny) / 4, -float(fi.tiny) / 8, float(fi.tiny), float(fi.max),
                     -float(fi.max) * 0.75, float(fi.smallest_subnormal)], dtype=T)
    vals = rng.standard_normal(n).astype(T)
    pick = rng.random(n) < 0.5
    vals[pick] = pool[rng.integers(0, pool.size, pick.sum())]
    return vals


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_special_values(oracle, bmsp, dtype):
    rng = np.random.default_rng(20 + dtype)
    (r1, c1, v1), (r2, c2, v2) = _overlapping_pair(64, 72, 9)
    coefs = [(1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (-0.0, 0.0), (0.5, -2.0), (3.0e-5, 7.0), (1.0e30, 1.0e30), (-1.0, 1.0e-30),
             (np.inf, 1.0), (np.nan, 1.0)]
    for la, lb, lc in ((0, 0, 0), (0, 1, 1), (1, 0, 1)):
        A, B = build(bmsp, 64, 72, r1, c1, v1, la, dtype), build(bmsp, 64, 72, r2, c2, v2, lb, dtype)
        for M in (A, B):
            _write_values(bmsp, M, _specials(dtype, M.nnz, rng))
            M.invalidate(False)
        for alpha, beta in coefs:
            check_add(oracle, bmsp, A, B, alpha, beta, lc, oracle_values=False)


def test_fp16_overflow_and_subnormal_results(oracle, bmsp):
    """fp16: 60000 + 60000 -> +Inf after the fp32 sum; 2^-24 * 0.5 products rounded once (ties to even) from fp32"""
    n = 16
    r, c = np.arange(n), (np.arange(n) * 3) % n
    A = build(bmsp, n, n, r, c, np.full(n, 60000.0), 0, 1)
    B = build(bmsp, n, n, r, c, np.linspace(2.0 ** -24, 6e4, n), 1, 1)
    C_, _ = check_add(oracle, bmsp, A, B, 1.0, 1.0, 0)
    assert np.isinf(C_.host_arrays()[3]).sum() >= n // 2
    S = build(bmsp, n, n, r, c, np.full(n, 2.0 ** -24) * np.arange(1, n + 1), 0, 1)
    C_, _ = check_add(oracle, bmsp, S, S, 0.5, 0.25, 1)
    # alpha = beta = 1: what the builder's duplicate summation gives on the concatenated COO (rounded fp16 values)
    for M1, M2 in ((A, B), (S, B)):
        C_, ref = check_add(oracle, bmsp, M1, M2, 1.0, 1.0, 0)
        util.assert_bmsp_equal_exact(ref, *C_.host_arrays(), np.float16)


# ---------------------------------------------------------------------------------------------------------
# 5. size: hub block-rows and the headline R-MAT
# ---------------------------------------------------------------------------------------------------------
def test_hub_block_rows_rmat16(oracle, bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(16, 8)
    A = build(bmsp, n, n, r, c, v, 0, 0)
    for lt, lc in ((1, 0), (0, 1)):
        At = A.transpose(lt)
        check_add(oracle, bmsp, A, At, 1.0, 1.0, lc)
    H = build(bmsp, n, n, r, c, v, 0, 1)
    check_add(oracle, bmsp, H, H.transpose(1), 1.0, -3.0, 0)


def _device_concat(bmsp, parts, dtype):
    n = sum(p.n for p in parts)
    out = bmsp.DeviceArray(n, dtype)
    off = 0
    for p in parts:
        if p.n:
            bmsp.check(bmsp.lib().bmsp_memcpy_d2d(out.ptr + off, p.ptr, p.n * p.dtype.itemsize))
        off += p.n * p.dtype.itemsize
    return out


def coo_route(bmsp, A, B, lay):
    """the pre-existing way to A + B: both operands to device COO, concatenated on the device, built again"""
    ra, ca, va = A.to_coo_device()
    rb, cb, vb = B.to_coo_device()
    r, c, v = (_device_concat(bmsp, [x, y], t) for x, y, t in ((ra, rb, np.int32), (ca, cb, np.int32), (va, vb, np.float64)))
    i = A.info()
    return bmsp.BmSpMatrix.from_coo_device(i["num_rows"], i["num_cols"], r, c, v, transposed=lay, dtype=i["dtype"])


def test_headline_rmat20_a_plus_at_matches_coo_route(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(20, 2)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    At = A.transpose(1)  # the layout-flipping transpose: A^T in the other layout
    snap_a, snap_t = snapshot(A), snapshot(At)
    for lc in (0, 1):
        C_ = bmsp.add(A, At, transposed=lc)
        assert_same_arrays(C_, coo_route(bmsp, A, At, lc))
    assert_unchanged(A, snap_a)
    assert_unchanged(At, snap_t)


# ---------------------------------------------------------------------------------------------------------
# 6. lanes, streams
# ---------------------------------------------------------------------------------------------------------
def test_both_lane_groups_agree(oracle, bmsp, monkeypatch):
    from pybmsp import gen
    cases = [gen.banded(400, 12), gen.rmat(12, 4)]
    for nr, nc, r, c, v in cases:
        for dtype in (0, 1, 2):
            A = build(bmsp, nr, nc, r, c, v, 0, dtype)
            B = A.transpose(1)
            outs = {}
            for g in ("1", "8"):
                monkeypatch.setenv("BMSP_ADD_LANES", g)
                outs[g] = [bmsp.add(A, B, 1.25, -0.5, transposed=lc) for lc in (0, 1)]
                check_add(oracle, bmsp, A, B, 1.25, -0.5, 1)
            for x, y in zip(outs["1"], outs["8"]):
                assert_same_arrays(x, y)
    monkeypatch.delenv("BMSP_ADD_LANES")


def test_non_default_stream(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(13, 6)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, dtype=2)
    B = A.transpose(1)
    H = _hip()
    s = C.c_void_p()
    assert H.hipStreamCreate(C.byref(s)) == 0
    try:
        C0 = bmsp.add(A, B, 2.0, 3.0, transposed=0, stream=s.value)
        assert H.hipStreamSynchronize(s) == 0
        assert_same_arrays(C0, bmsp.add(A, B, 2.0, 3.0, transposed=0))
        v2 = np.random.default_rng(5).uniform(-1, 1, v.size)
        _write_values(bmsp, A, bmsp.BmSpMatrix.from_coo(n, n, r, c, v2, dtype=2).host_arrays()[3])
        A.invalidate(False)
        bmsp.add_values(C0, A, B, -1.0, 0.5, stream=s.value)
        assert H.hipStreamSynchronize(s) == 0
        assert_same_arrays(C0, bmsp.add(A, B, -1.0, 0.5, transposed=0))
    finally:
        H.hipStreamDestroy(s)


# ---------------------------------------------------------------------------------------------------------
# 7. downstream use of C
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rmat", "fem"])
def test_sum_works_downstream(oracle, bmsp, kind):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(12, 6) if kind == "rmat" else gen.fem_like(10, "27pt")
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    B = A.transpose(1)
    C_, ref = check_add(oracle, bmsp, A, B, 1.0, 0.5, 0)
    x = gen.spmv_x(n, "cusp")
    y = bmsp.spmv(C_, bmsp.DeviceArray.from_host(x)).to_host()
    yr = oracle.spmv_f32(ref, x)
    assert np.allclose(y, yr, rtol=1e-5, atol=1e-5), float(np.max(np.abs(y - yr)))
    C1, ref1 = check_add(oracle, bmsp, A, B, 1.0, 0.5, 1)
    P, st = bmsp.spgemm(C_, C1, tc_version=5)
    oc, ost = oracle.spgemm(ref, ref1)
    pk, pb, po, pv = P.host_arrays()
    np.testing.assert_array_equal(pk, oc.keys)
    np.testing.assert_array_equal(pb, oc.bmps)
    np.testing.assert_array_equal(po, oc.offsets)
    assert st["c_nnz"] == ost["c_nnz"]
    assert np.allclose(pv, oc.values, rtol=1e-5, atol=1e-6), float(np.max(np.abs(pv - oc.values)))


# ---------------------------------------------------------------------------------------------------------
# 8. add_values
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_add_values_follows_new_values(oracle, bmsp, dtype):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(12, 6) if dtype != 1 else gen.fem_like(10, "27pt")
    v2 = np.random.default_rng(3).uniform(-2.0, 2.0, v.size)
    for la, lb, lc in ((0, 1, 0), (0, 1, 1), (1, 1, 0), (0, 0, 1)):
        A = build(bmsp, n, n, r, c, v, la, dtype)
        B = build(bmsp, n, n, c, r, v * 0.5, lb, dtype)
        Cm = bmsp.add(A, B, 1.0, 1.0, transposed=lc)
        if dtype != 2:
            Cm.prepare(3)  # holds derived caches: add_values drops the value-derived ones
        _write_values(bmsp, A, build(bmsp, n, n, r, c, v2, la, dtype).host_arrays()[3])
        A.invalidate(False)
        bmsp.add_values(Cm, A, B, -0.25, 3.0)
        assert_same_arrays(Cm, bmsp.add(A, B, -0.25, 3.0, transposed=lc))
        check_add(oracle, bmsp, A, B, -0.25, 3.0, lc)
        # the SpMV of C sees the new values
        if dtype == 0 and lc == 0:  # (the SpMV takes row-major tiles)
            x = gen.spmv_x(n, "cusp")
            y = bmsp.spmv(Cm, bmsp.DeviceArray.from_host(x)).to_host()
            y2 = bmsp.spmv(bmsp.add(A, B, -0.25, 3.0, transposed=lc), bmsp.DeviceArray.from_host(x)).to_host()
            np.testing.assert_array_equal(y, y2)
    # the same handle as both operands
    A = build(bmsp, n, n, r, c, v, 0, dtype)
    Cm = bmsp.add(A, A, 2.0, 1.0)
    bmsp.add_values(Cm, A, A, 0.5, 0.5)
    assert_same_arrays(Cm, bmsp.add(A, A, 0.5, 0.5))


def test_add_values_refusals(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(10, 4)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    B = bmsp.BmSpMatrix.from_coo(n, n, c, r, v, transposed=1)
    Cm = bmsp.add(A, B)
    bmsp.add_values(Cm, A, B)  # paired: fine

    def refused(fn, word):
        with pytest.raises(bmsp.BmspError) as e:
            fn()
        assert e.value.status == -1 and word in str(e.value), str(e.value)

    refused(lambda: bmsp.add_values(Cm, B, A), "swapped")
    other = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)
    refused(lambda: bmsp.add_values(Cm, other, B), "add_values")
    P, _ = bmsp.spgemm(A, B)
    refused(lambda: bmsp.add_values(P, A, B), "bmsp_matrix_add")
    refused(lambda: bmsp.add_values(A.transpose(0), A, B), "bmsp_matrix_add")
    A.invalidate(True)  # A's structure is declared changed
    refused(lambda: bmsp.add_values(Cm, A, B), "structure")
    C2 = bmsp.add(A, B)
    C2.invalidate(True)  # C's own structure declared changed: it forgets its operands
    refused(lambda: bmsp.add_values(C2, A, B), "bmsp_matrix_add")


def test_add_refusals(bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(10, 4)
    A = bmsp.BmSpMatrix.from_coo(n, n, r, c, v)

    def refused(fn, word):
        with pytest.raises(bmsp.BmspError) as e:
            fn()
        assert e.value.status == -1 and word in str(e.value), str(e.value)

    wide = bmsp.BmSpMatrix.from_coo(n, n + 1, r, c, v)
    refused(lambda: bmsp.add(A, wide), "shapes")
    refused(lambda: bmsp.add(wide, A), "shapes")
    refused(lambda: bmsp.add(A, bmsp.BmSpMatrix.from_coo(n, n, r, c, v, dtype=1)), "dtypes")
    refused(lambda: bmsp.add(A, bmsp.BmSpMatrix.from_coo(n, n, r, c, v, dtype=2)), "dtypes")
    V = A.row_panel(3, 9)
    refused(lambda: bmsp.add(V, V), "view")
    refused(lambda: bmsp.add(A, V), "view")
    Cm = bmsp.add(A, A)
    refused(lambda: bmsp.add_values(Cm, A, wide), "shapes")


def test_cpp_wrappers_run(bmsp, tmp_path):
    """tests/cpp_add_check.cpp: bmSparse_add / bmSparse_add_values on the data/real fixture"""
    import subprocess
    from conftest import MTX
    from test_add_api import build_cpp_add_check
    exe = str(tmp_path / "cpp_add_check")
    build_cpp_add_check(exe)
    out = subprocess.run([exe, os.path.join(MTX, "real", "A_matrix.mtx")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    for word in ("CHECK add OK", "CHECK add_values OK", "CHECK half OK"):
        assert word in out.stdout, out.stdout
