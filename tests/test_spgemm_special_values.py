"""SpGEMM on operands that hold Inf, NaN, subnormals or values whose products overflow, against the CPU oracle on every block-MAC path.

The library decides between kernels by the VALUES of its operands in one place: a per-handle cache (values_finite, f32_exp_min,
f32_exp_max) filled by ensure_finite_flag and read by the strip block-MAC, the row-sparse block-MAC and the fp32 MFMA task-list kernel.
Those three skip candidate pairs or multiply stored values only, which is right for finite operands alone: the reference (restated in
oracle/bmsp_oracle.c) multiplies whole 8x8 tiles of every surviving pair, so an Inf at A(i, k) meets the implicit zeros of B's tile and
gives NaN along that tile row of C.  The tests here plant such values, force every path as the neighbouring tests force it, assert on a
finite twin (the special values replaced by ordinary ones) that the forced kernel really runs, then assert which kernel ran on the
special operands and compare every array of C with the oracle.

There is no tolerance in this file.  Finite values are small integers, or small integers times a power of two, chosen so that every
partial sum of the FINITE values is exactly representable in fp32 in ANY order (test_family_is_exact_and_hits_its_classes proves that on
the CPU for every input family, with the special values taken out); a stored Inf / NaN or an fp16 product that overflows then only
decides the class of a result -- finite, +Inf, -Inf or NaN -- and that class does not depend on the order either.  One family is
different: in f32_overflow the first product that overflows in the fmaf chain decides +Inf or -Inf and the sum stays there whatever
follows (the product is never rounded, so no NaN arises), which DOES depend on the order.  The comparison is valid all the same: every
fp32 kernel that may run on those operands claims the oracle's order (ascending k, tasks in list order) and is compared bit for bit;
the matrix-core kernels, which do not, must be refused by the exponent guard, and the test asserts that they are.  NaNs are compared by
position, never by payload or sign: the host's default NaN and the GPU's differ in the sign bit.

SpMV / SpMM (the last section): x holds Inf and NaN at every column of the block-columns in which the matrix stores NO tile, and no kernel
may read them.  Special values of x INSIDE a block-column that holds a tile, stored Inf / NaN, subnormals and overflowing sums are the
subject of test_spmv_special_values.py: the oracle multiplies whole tiles there (0 * Inf = NaN for the positions a tile does not store),
the kernels multiply stored values only (bmsp.h, bmsp_spmv), so that file compares with a reference of its own.
"""
import numpy as np
import pytest

import util
from util import SPMV_LAUNCHES, SPMV_CHUNK_LAYOUT, SPMM_LAUNCHES, spmv_launch_params

NPDT = {0: np.float32, 1: np.float16, 2: np.float64}
INF, NAN = float("inf"), float("nan")


# ---------------------------------------------------------------------------------------------------------
# 0. comparison rule
# ---------------------------------------------------------------------------------------------------------
STAGE_COUNTERS = ("task_list_size", "bmp_reduction", "surviving_tasks", "c_blocks", "c_nnz")


def compare_values(got, ref, exact_bits):
    """NaN masks equal (position only); every other value, +-Inf included, equal -- bit for bit (sign of zero too) with exact_bits,
    as numbers (-0 == +0) without."""
    got = np.asarray(got)
    ref = np.asarray(ref, dtype=np.float64).astype(got.dtype)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    bad = np.flatnonzero(gn != rn)
    assert bad.size == 0, "NaN mask differs at %d of %d values, first %d: got %r, oracle %r" % (bad.size, got.size, bad[0], got[bad[0]], ref[bad[0]])
    g, r = got[~gn], ref[~rn]
    if exact_bits:
        ut = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        g, r = g.view(ut), r.view(ut)
    bad = np.flatnonzero(g != r)
    assert bad.size == 0, "%d of %d values differ, first: got %r, oracle %r" % (bad.size, got.size, got[~gn][bad[0]], ref[~rn][bad[0]])


def compare_with_oracle(Cm, refC, exact_bits, st=None, rst=None):
    """keys, bitmaps, offsets (and the stage counters, given both stats) bit for bit as check_spgemm does; values by compare_values."""
    if st is not None and rst is not None:
        for key in STAGE_COUNTERS:
            assert st[key] == rst[key], (key, st[key], rst[key])
    k, b, o, v = Cm.host_arrays()
    np.testing.assert_array_equal(k, refC.keys)
    np.testing.assert_array_equal(b, refC.bmps)
    np.testing.assert_array_equal(o, refC.offsets)
    compare_values(v, refC.values, exact_bits)


def exact_bits_for(dtype, tc):
    """V15 numerics (fp32 / fp64 operands, fp16 under tc_version 5): the oracle's operation order, bit for bit; fp16 on the matrix cores:
    the hardware's accumulation order, equal as numbers."""
    return not (dtype == 1 and tc != 5)


# ---------------------------------------------------------------------------------------------------------
# 1. input families
# ---------------------------------------------------------------------------------------------------------
def _ints(r, c, salt):
    """-2, -1, 1, 2 by position"""
    v = ((np.asarray(r, np.int64) * 3 + np.asarray(c, np.int64) * 7 + salt) % 5 - 2).astype(np.float64)
    v[v == 0] = 1.0
    return v


def _structure(name):
    """(A, B) as (rows, cols, r, c) of a structure of test_gpu_parity's kernels tests: _strip_case's banded64 (full tiles, ragged last
    block-row), fem (nearly empty tiles), rect_ragged (rectangular, ragged on every side), filtered_run; `rmat`: the R-MAT of
    test_spgemm_rowwindow_path[rmat11_narrow] (hub block-rows, small enough for the window passes)."""
    from pybmsp import gen
    from test_gpu_parity import _strip_case
    if name == "rmat":
        n, _, r, c, _ = gen.rmat(11, 8)
        A = (n, n, r, c)
        return A, A
    A, B, _ = _strip_case(gen, None, name)
    if B is None:
        B = A
    return A[:4], B[:4]


def _find(coo, row, col=None):
    """index of the stored entry of `row` whose column is nearest to `col` (the middle one of the row when None)"""
    r, c = np.asarray(coo[2]), np.asarray(coo[3])
    idx = np.flatnonzero(r == row)
    assert idx.size, "row %d holds nothing" % row
    if col is None:
        return int(idx[idx.size // 2])
    return int(idx[np.argmin(np.abs(c[idx].astype(np.int64) - col))])


class Family:
    """A, B: COO tuples (rows, cols, r, c, v) with the special values; At, Bt: the finite twin on the same structure; expect: which
    classes the oracle's C must hold; finite: the operands themselves are finite (the cached flag says so and the fast kernels DO run)."""

    def __init__(self, name, A, B, At, Bt, dtypes, tcs16, expect, finite=False, no_nan=False):
        self.name, self.A, self.B, self.At, self.Bt = name, A, B, At, Bt
        self.dtypes, self.tcs16, self.expect, self.finite, self.no_nan = dtypes, tcs16, expect, finite, no_nan
        self._sparse = None

    def sparse_tiles(self, oracle):
        """the fill rule of mac_rowsparse_applies: at most 16 stored values per tile on both sides"""
        if self._sparse is None:
            a = oracle.bmsp_from_coo(oracle.Coo(*self.At), 0, False)
            b = oracle.bmsp_from_coo(oracle.Coo(*self.Bt), 0, True)
            self._sparse = a.nnz <= 16 * a.block_num and b.nnz <= 16 * b.block_num
        return self._sparse


def _twin(coo):
    v = np.array(coo[4], dtype=np.float64)
    v[~np.isfinite(v)] = 1.0
    return coo[:4] + (v,)


def _planted(structure, plant):
    """integer values on `structure`, then plant(A, B, va, vb) writes the special values"""
    A, B = _structure(structure)
    va, vb = _ints(A[2], A[3], 0), _ints(B[2], B[3], 1)
    plant(A, B, va, vb)
    return A + (va,), B + (vb,)


_FAMILIES = {}


def family(name):
    if name not in _FAMILIES:
        _FAMILIES[name] = _build_family(name)
    return _FAMILIES[name]


def _build_family(name):
    both, all16 = (0, 1), (5, 4, 1)
    if name == "inf_a":            # one stored +Inf in A only; full tiles: Inf meets stored finite values (+-Inf, Inf - Inf) and, at the band's edge, implicit zeros
        def plant(A, B, va, vb):
            va[_find(A, 517, 500)] = INF
        A, B = _planted("banded64", plant)
        return Family(name, A, B, _twin(A), _twin(B), both, all16, {"nan", "pinf", "ninf"})
    if name == "inf_b":            # one stored +Inf in B only, nearly empty tiles
        def plant(A, B, va, vb):
            vb[_find(B, 803)] = INF
        A, B = _planted("fem", plant)
        return Family(name, A, B, _twin(A), _twin(B), both, all16, {"nan"})
    if name == "nan_a":            # one stored NaN in A; rectangular A x B
        def plant(A, B, va, vb):
            va[_find(A, 117)] = NAN
        A, B = _planted("rect_ragged", plant)
        return Family(name, A, B, _twin(A), _twin(B), both, all16, {"nan"})
    if name == "neg_inf_pair":     # +Inf and -Inf in one row of A against equal entries of B: Inf - Inf from the STORED products alone
        def plant(A, B, va, vb):
            i = 900
            ks = np.asarray(A[3])[np.asarray(A[2]) == i]
            brow = {int(k): set(np.asarray(B[3])[np.asarray(B[2]) == k].tolist()) for k in ks}
            for k1 in ks:
                for k2 in ks:
                    common = brow[int(k1)] & brow[int(k2)] if k1 < k2 else ()
                    if common:
                        j = min(common)
                        r, c = np.asarray(A[2]), np.asarray(A[3])
                        va[np.flatnonzero((r == i) & (c == k1))[0]] = INF
                        va[np.flatnonzero((r == i) & (c == k2))[0]] = -INF
                        rb, cb = np.asarray(B[2]), np.asarray(B[3])
                        vb[np.flatnonzero((rb == k1) & (cb == j))[0]] = 1.0
                        vb[np.flatnonzero((rb == k2) & (cb == j))[0]] = 1.0
                        return
            raise AssertionError("no pair of columns with a common column of B")
        A, B = _planted("fem", plant)
        return Family(name, A, B, _twin(A), _twin(B), both, all16, {"nan"})
    if name == "inf_times_stored_zero":  # an explicit 0.0 in B opposite the Inf of A: NaN even by "stored values only" arithmetic
        def plant(A, B, va, vb):
            ia = _find(A, 60)
            k = int(np.asarray(A[3])[ia])
            va[ia] = INF
            vb[_find(B, k)] = 0.0
        A, B = _planted("rect_ragged", plant)
        return Family(name, A, B, _twin(A), _twin(B), both, all16, {"nan"})
    if name == "inf_in_filtered_pair":   # the Inf sits in A's tile (0, 0), all of whose candidate pairs die in the bitmap filter: C holds no NaN at all
        def plant(A, B, va, vb):
            r, c = np.asarray(A[2]), np.asarray(A[3])
            va[np.flatnonzero((r == 3) & (c == 0))[0]] = INF
        A, B = _planted("filtered_run", plant)
        return Family(name, A, B, _twin(A), _twin(B), both, all16, set(), no_nan=True)
    if name == "rmat_inf":         # the Inf in an R-MAT with hub block-rows (the column-window passes)
        def plant(A, B, va, vb):
            r = np.asarray(A[2])
            cnt = np.bincount(r[r >= 1024], minlength=2048)
            va[_find(A, int(np.argmax(cnt)))] = INF   # a row of several entries: their products meet the implicit zeros opposite the Inf
        A, B = _planted("rmat", plant)
        return Family(name, A, B, _twin(A), _twin(B), both, (5, 4), {"nan"})
    if name in ("f16_product_overflow", "f32_overflow"):
        # columns K of A and rows K of B hold large powers of two of both signs, everything else small integers: a product is small x small
        # or large x large, never mixed -- the large products overflow (fp16 under V15: each product is rounded to fp16; fp32: in the fmaf
        # chain) to +-Inf, sums of both signs to NaN; under tc_version 4 the fp16 products are exact and the sums stay below 2^21
        A, B = _structure("banded64")
        va, vb = _ints(A[2], A[3], 0), _ints(B[2], B[3], 1)
        ka, kb = (np.asarray(A[3]) >= 400) & (np.asarray(A[3]) < 404), (np.asarray(B[2]) >= 400) & (np.asarray(B[2]) < 404)
        if name == "f16_product_overflow":
            ea, eb = 8 + (np.asarray(A[2]) + np.asarray(A[3])) % 2, 8 + (np.asarray(B[2]) * 3 + np.asarray(B[3])) % 2
        else:
            ea, eb = 64 + (np.asarray(A[2]) * 5 + np.asarray(A[3])) % 37, 64 + (np.asarray(B[2]) * 3 + np.asarray(B[3]) * 7) % 37
        # the sign by column of A and row of B only: the row (i, :) x column (:, j) products then have the signs s(k) -- both signs for every (i, j)
        # that all of K reaches -- while (i, j) reached by one k alone give +-Inf
        sa = np.where(np.asarray(A[3]) % 2 == 0, 1.0, -1.0)
        wa, wb = va.copy(), vb.copy()
        wa[ka] = (sa * np.ldexp(1.0, ea))[ka]
        wb[kb] = np.ldexp(1.0, eb)[kb]
        if name == "f16_product_overflow":
            return Family(name, A + (wa,), B + (wb,), A + (va,), B + (vb,), (1,), (5, 4), {"nan", "pinf", "ninf"}, finite=True)
        return Family(name, A + (wa,), B + (wb,), A + (va,), B + (vb,), (0,), (), {"pinf", "ninf"}, finite=True)
    if name == "f16_subnormal":    # 2^-24 .. 2^-15 (fp16 subnormals and the smallest normals) against 2^0 .. 2^10, both signs
        A, B = _structure("fem")
        ra, ca, rb, cb = (np.asarray(x, np.int64) for x in (A[2], A[3], B[2], B[3]))
        wa = np.where((ra + ca) % 3 == 0, -1.0, 1.0) * np.ldexp(1.0, -24 + (ra + 2 * ca) % 10)
        wb = np.where((rb * 2 + cb) % 5 == 0, -1.0, 1.0) * np.ldexp(1.0, (rb + 3 * cb) % 11)
        return Family(name, A + (wa,), B + (wb,), A + (_ints(ra, ca, 0),), B + (_ints(rb, cb, 1),), (1,), (5, 4, 3, 2, 1), set(), finite=True)
    if name == "f32_subnormal":    # 2^-149 .. 2^-127 (fp32 subnormals) against powers of two up to 2^20; e + f <= 14 except at both ends of A's range
        A, B = _structure("fem")
        ra, ca, rb, cb = (np.asarray(x, np.int64) for x in (A[2], A[3], B[2], B[3]))
        def exp_a(k):                                # by the column of A = the row of B; the upper third of the range at every eighth k only
            e = (k * 7 + 3) % 23
            return np.where((e > 14) & (k % 8 != 0), e - 12, e)
        e = exp_a(ca)
        f = np.where(exp_a(rb) == 0, 20, np.maximum(0, 14 - exp_a(rb)))
        wa = np.where((ra + ca) % 3 == 0, -1.0, 1.0) * np.ldexp(1.0, -149 + e)
        wb = np.where((rb * 2 + cb) % 5 == 0, -1.0, 1.0) * np.ldexp(1.0, f)
        return Family(name, A + (wa,), B + (wb,), A + (_ints(ra, ca, 0),), B + (_ints(rb, cb, 1),), (0,), (), set(), finite=True)
    raise ValueError(name)


FAMILIES = ["inf_a", "inf_b", "nan_a", "neg_inf_pair", "inf_times_stored_zero", "inf_in_filtered_pair", "rmat_inf", "f16_product_overflow",
            "f16_subnormal", "f32_subnormal", "f32_overflow"]

_ORACLE = {}


def oracle_product(oracle, fam, dtype, exact_products, twin=False):
    """the oracle's (C, stats) of a family's operands, computed once per (family, dtype, numerics) and never written to"""
    key = (fam.name, dtype, bool(exact_products), twin)
    if key not in _ORACLE:
        A, B = (fam.At, fam.Bt) if twin else (fam.A, fam.B)
        ra = oracle.bmsp_from_coo(oracle.Coo(*A), dtype, False)
        rb = oracle.bmsp_from_coo(oracle.Coo(*B), dtype, True)
        _ORACLE[key] = oracle.spgemm(ra, rb, exact_products=exact_products)
    return _ORACLE[key]


def _dense64(coo):
    nr, nc, r, c, v = coo
    return util.scipy_csr(nr, nc, r, c, v)


def _tile_classes(C):
    """per C tile: holds a NaN / holds a finite value / holds any special value"""
    v = C.values
    off = C.offsets.astype(np.int64)
    seg = np.repeat(np.arange(C.block_num), np.diff(off))
    has = lambda mask: np.bincount(seg[mask], minlength=C.block_num) > 0
    return has(np.isnan(v)), has(np.isfinite(v)), has(~np.isfinite(v))


@pytest.mark.parametrize("name", FAMILIES)
def test_family_is_exact_and_hits_its_classes(oracle, name):
    """CPU self-check of the input families.  (1) Every partial sum of the finite values is exact in fp32 in any order: with the special
    values taken out (Inf / NaN -> 0; the overflow families: their small-integer twin, not their real operands -- see the file's
    docstring for f32_overflow) the sum of |a| |b| over every C value, in units of the smallest product, stays
    below 2^24, and the oracle's chain equals the float64 product exactly, under both product numerics of fp16.  (2) The family produces
    what it is for: the classes it names, a finite value in a tile that also holds a NaN, a tile no special value reaches."""
    fam = family(name)
    overflow = name in ("f16_product_overflow", "f32_overflow")
    fin = lambda coo: coo[:4] + (np.where(np.isfinite(coo[4]), coo[4], 0.0),)
    legs = [(fam.At, fam.Bt)] if overflow else [(fin(fam.A), fin(fam.B)), (fam.At, fam.Bt)]
    if name == "f16_product_overflow":
        legs.append((fam.A, fam.B))  # exact under tc_version 4
    for dtype in fam.dtypes:
        for li, (A, B) in enumerate(legs):
            da, db = _dense64(A), _dense64(B)
            nza, nzb = np.abs(A[4][A[4] != 0]), np.abs(B[4][B[4] != 0])
            quantum = nza.min() * nzb.min()
            mag = (abs(da) @ abs(db))
            assert mag.max() / quantum < 2.0 ** 24, (name, mag.max() / quantum)
            assert float(NPDT[dtype](nza.min())) == nza.min() and float(NPDT[dtype](nza.max())) == nza.max()   # representable as stored
            ref64 = (da @ db).tocsr()
            ra = oracle.bmsp_from_coo(oracle.Coo(*A), dtype, False)
            rb = oracle.bmsp_from_coo(oracle.Coo(*B), dtype, True)
            for exact_products in ((False, True) if dtype == 1 else (False,)):
                if name == "f16_product_overflow" and li == 1 and not exact_products:
                    continue     # (that leg is the point of the family: it overflows under V15)
                C, _ = oracle.spgemm(ra, rb, exact_products=exact_products)
                got = oracle.bmsp_to_coo(C)
                want = np.asarray(ref64[got.rows, got.cols]).ravel()
                bad = np.flatnonzero(got.vals != want)
                assert bad.size == 0, (name, dtype, exact_products, got.rows[bad[:4]], got.cols[bad[:4]], got.vals[bad[:4]], want[bad[:4]])
    for dtype in fam.dtypes:
        C, _ = oracle_product(oracle, fam, dtype, False)
        v = C.values
        if fam.no_nan:
            assert np.isfinite(v).all() and not np.isfinite(fam.A[4]).all()
            continue
        for cls, mask in (("nan", np.isnan(v)), ("pinf", v == INF), ("ninf", v == -INF)):
            assert cls not in fam.expect or mask.any(), (name, cls)
        nan_t, fin_t, spec_t = _tile_classes(C)
        if "nan" in fam.expect:
            assert (nan_t & fin_t).any(), "no finite value in a tile that holds a NaN"
        elif fam.expect:      # (the fmaf chain never rounds a product: an overflowed sum stays +-Inf whatever is added, NaN cannot arise)
            assert not np.isnan(v).any() and (spec_t & fin_t).any(), "no finite value in a tile that holds an Inf"
        if fam.expect:
            assert (~spec_t).any(), "no tile without a special value"
        else:
            assert np.isfinite(v).all()
        if name == "f16_product_overflow":   # the same inputs with exact products: large finite numbers
            Cx, _ = oracle_product(oracle, fam, dtype, True)
            assert np.isfinite(Cx.values).all() and np.abs(Cx.values).max() >= 2.0 ** 16
        if name in ("f16_subnormal", "f32_subnormal"):
            tiny = 2.0 ** -14 if name == "f16_subnormal" else 2.0 ** -126
            assert ((np.abs(v) < tiny) & (v != 0)).any() and np.abs(fam.A[4]).min() < tiny


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_oracle_takes_inf_and_nan_from_coo(oracle, dtype):
    """golden vector: the oracle's builder stores Inf / NaN as given (fp16: values beyond 65520 become Inf), and its product of a 2 x 2
    tile pair follows IEEE: Inf * stored 0 and Inf * implicit 0 are NaN, Inf * 2 is Inf, Inf - Inf is NaN."""
    A = oracle.bmsp_from_coo(oracle.Coo(8, 8, [0, 0, 1, 2, 2], [0, 1, 0, 0, 1], [INF, 1.0, 3.0, INF, -INF]), dtype, False)
    B = oracle.bmsp_from_coo(oracle.Coo(8, 8, [0, 0, 1, 1], [0, 1, 0, 2], [2.0, 0.0, 2.0, NAN]), dtype, True)
    assert A.values.tolist()[:3] == [INF, 1.0, 3.0] and A.values.tolist()[3:] == [INF, -INF]
    assert np.isnan(B.values[[3]]).all() and B.values.tolist()[:1] == [2.0]
    for exact_products in ((False, True) if dtype == 1 else (False,)):
        C, _ = oracle.spgemm(A, B, exact_products=exact_products)
        d = util.bmsp_host_to_dok(8, 8, C.keys, C.bmps, C.offsets, C.values)
        assert sorted(d) == [(i, j) for i in range(3) for j in range(3) if (i, j) != (1, 2)]   # (row 1 of A stores no k = 1 entry)
        assert d[(0, 0)] == INF and np.isnan(d[(0, 1)]) and np.isnan(d[(0, 2)])      # Inf*2 + 1*2; Inf * stored 0; Inf * implicit 0 + 1 * NaN
        assert d[(1, 0)] == 6.0 and d[(1, 1)] == 0.0                                  # no special value reaches row 1
        assert np.isnan(d[(2, 0)]) and np.isnan(d[(2, 1)]) and np.isnan(d[(2, 2)])   # Inf*2 - Inf*2
    if dtype == 1:
        H = oracle.bmsp_from_coo(oracle.Coo(8, 8, [0, 1], [0, 0], [65519.0, 65520.0]), 1, False)
        assert H.values.tolist() == [65504.0, INF]


# ---------------------------------------------------------------------------------------------------------
# 2. every path, forced as the neighbouring tests force it
# ---------------------------------------------------------------------------------------------------------
FAST = (3, 4, 5)   # BMSP_MAC_STRIP, BMSP_MAC_F32MFMA, BMSP_MAC_ROWSPARSE: right for finite operands only

# name -> (environment, sort mode); the switches of test_valu_block_mac_staging, test_mfma32_block_mac_paths, test_strip_block_mac,
# test_spgemm_rowmerge_path, test_spgemm_rowmerge_task_list, test_spgemm_rowwindow_path, test_f32_mfma_block_mac, test_spgemm_rowsparse_block_mac
PATHS = {
    "default": ({}, 0),
    "pipe_seg_gather": ({"BMSP_MAC_VALU_DENSE": "0"}, 1),
    "pipe_glob_dense": ({"BMSP_MAC_VALU_DENSE": "1"}, 2),
    "pipe_seg_b_compact": ({"BMSP_MAC_STRIP": "0", "BMSP_MAC_B_DENSE": "0", "BMSP_MAC_DIRECT": "0"}, 1),
    "pipe_glob_b_dense": ({"BMSP_MAC_STRIP": "0", "BMSP_MAC_B_DENSE": "1", "BMSP_MAC_DIRECT": "0"}, 2),
    "pipe_seg_direct": ({"BMSP_MAC_STRIP": "0", "BMSP_MAC_B_DENSE": "1", "BMSP_MAC_DIRECT": "1"}, 1),
    "pipe_seg": ({}, 1),
    "pipe_glob": ({}, 2),
    "strip": ({"BMSP_MAC_STRIP": "1"}, 0),
    "rowmerge": ({"BMSP_SPGEMM_ROWMERGE": "1"}, 0),
    "rowsparse": ({"BMSP_MAC_ROWSPARSE": "1"}, 0),
    "f32mfma": ({"BMSP_MAC_F32MFMA": "1"}, 0),
    "tasklist": ({"BMSP_SPGEMM_ROWMERGE": "2", "BMSP_MAC_STRIP": "0"}, 0),
    "rowwindow": ({"BMSP_SPGEMM_ROWWINDOW": "1", "BMSP_WIN_THIN": "1"}, 0),
}


def _paths_for(name, dtype, tc):
    """Which switches run for which numerics.  Left out on purpose, because the switch cannot reach a fast kernel there and the run would
    repeat `default`: BMSP_MAC_STRIP=1 for fp16 under tc_version 5 and 1 (the fp16 strip kernel has tc_version 4's numerics only),
    BMSP_SPGEMM_ROWMERGE=1 and BMSP_MAC_ROWSPARSE=1 under tc_version 1 (no numeric stage works from C's structure alone for the K = 16
    MFMA numerics: row-merge means task-list mode, which `tasklist` forces), BMSP_MAC_F32MFMA=1 for fp16 (fp32 only), the staging
    switches of another tc_version's kernels.  tc_version 2 and 3 share tc_version 1's kernel and run `default` only."""
    if dtype == 0:
        paths = ["default", "pipe_seg_gather", "pipe_glob_dense", "strip", "rowmerge", "rowsparse", "f32mfma", "tasklist", "rowwindow"]
    elif tc == 5:
        paths = ["default", "pipe_seg_gather", "pipe_glob_dense", "rowmerge", "rowsparse", "tasklist", "rowwindow"]
    elif tc == 4:
        paths = ["default", "pipe_seg_b_compact", "pipe_glob_b_dense", "pipe_seg_direct", "strip", "rowmerge", "tasklist", "rowwindow"]
    else:
        paths = ["default", "pipe_seg", "pipe_glob", "tasklist", "rowwindow"]
    if name == "rmat_inf":      # hub block-rows: beyond the strip and row-sparse kernels' tables; what the window passes are for
        paths = [p for p in paths if p in ("default", "pipe_seg_gather", "pipe_seg_direct", "rowmerge", "rowwindow", "f32mfma")]
    elif name in ("inf_a", "neg_inf_pair", "inf_times_stored_zero", "f16_product_overflow", "f32_overflow", "f32_subnormal"):
        paths = [p for p in paths if p != "rowwindow"]   # (the window passes: one structure of every kind is enough)
    if tc in (3, 2):
        paths = ["default"]
    return paths


def _cases():
    out = []
    for name in FAMILIES:
        fam_dtypes, fam_tcs = {"f16_product_overflow": ((1,), (5, 4)), "f16_subnormal": ((1,), (5, 4, 3, 2, 1)), "f32_subnormal": ((0,), ()),
                               "f32_overflow": ((0,), ()), "rmat_inf": ((0, 1), (5, 4))}.get(name, ((0, 1), (5, 4, 1)))
        for dtype in fam_dtypes:
            for tc in ((5,) if dtype == 0 else fam_tcs):
                for path in _paths_for(name, dtype, tc):
                    out.append(pytest.param(name, dtype, tc, path, id="%s-%s-tc%d-%s" % (name, ("f32", "f16")[dtype], tc, path)))
    return out


def _expected_twin(path, dtype, tc, sparse, hub, mode):
    """what the stats of the finite twin must show: (sort paths allowed, mac variants allowed or None)"""
    v15 = dtype == 0 or tc == 5
    if path == "default":
        return None, None
    if path.startswith("pipe"):
        sp = (0,) if mode == 2 else (0, 1)
        if "BMSP_MAC_VALU_DENSE" in PATHS[path][0]:
            return sp, (0,)
        if dtype == 1 and tc == 4:
            return sp, (1, 2)
        return sp, (0,)
    if path == "rowwindow":
        return (3,), None
    if hub:      # hub block-rows: the row-merge task-list mode while its table holds them, the column-window passes beyond
        return (2, 3), ((4,) if path == "f32mfma" else None)
    if path == "strip":
        return (2,), ((3,) if dtype == 1 else ((5,) if sparse else (3,)))
    if path == "rowmerge":
        if dtype == 1 and tc == 4:
            return (2,), (3,)
        if dtype == 0:
            return (2,), ((5,) if sparse else (3,))
        return (2,), ((5,) if sparse else (0,))
    if path == "rowsparse":
        return (2,), ((5,) if v15 else None)
    if path == "f32mfma":
        return (2,), (4,)
    if path == "tasklist":
        return (2,), None
    raise ValueError(path)


def _make(bmsp, A, B, dtype):
    return (bmsp.BmSpMatrix.from_coo(*A, transposed=False, dtype=dtype), bmsp.BmSpMatrix.from_coo(*B, transposed=True, dtype=dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype,tc,path", _cases())
def test_special_values_on_every_path(oracle, bmsp, monkeypatch, name, dtype, tc, path):
    """One family on one forced path.  Finite twin first: the stats must show the forced kernel, and C must equal the oracle's.  Then the
    special operands: non-finite ones must not take the strip (3), fp32 MFMA (4) or row-sparse (5) kernel, finite ones (overflowing
    products, subnormals) must take what the twin took -- unless an fp32 exponent guard sends them to the vector-ALU kernel -- and C must
    equal the oracle's by compare_with_oracle."""
    fam = family(name)
    env, mode = PATHS[path]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    if name == "rmat_inf" and path == "rowwindow":
        monkeypatch.setenv("BMSP_WIN_CAND", "64")
    exact_products = dtype == 1 and tc != 5
    exact_bits = exact_bits_for(dtype, tc)
    sorts, variants = _expected_twin(path, dtype, tc, fam.sparse_tiles(oracle), name == "rmat_inf", mode)
    # the finite twin
    a, b = _make(bmsp, fam.At, fam.Bt, dtype)
    Ct, stt = bmsp.spgemm(a, b, mode=mode, tc_version=tc)
    assert sorts is None or stt["sort_path"] in sorts, stt
    assert variants is None or stt["c_blocks"] == 0 or stt["mac_variant"] in variants, stt
    assert stt["mac_kernel"] == (tc if exact_products else 5), stt
    refT, rstT = oracle_product(oracle, fam, dtype, exact_products, twin=True)
    compare_with_oracle(Ct, refT, exact_bits, stt, rstT)
    # the special values
    a, b = _make(bmsp, fam.A, fam.B, dtype)
    Cs, sts = bmsp.spgemm(a, b, mode=mode, tc_version=tc)
    assert sorts is None or sts["sort_path"] in sorts, sts
    if not fam.finite:
        assert sts["mac_variant"] not in FAST, sts
    elif name == "f32_subnormal":
        assert sts["mac_variant"] == 0, sts                # products below the normal range: V15's vector-ALU kernel
    elif name == "f32_overflow":
        assert sts["mac_variant"] not in (3, 4), sts       # sums overflow: not the matrix cores (the row-sparse chain is the reference's own operations)
        assert path != "rowsparse" or sts["mac_variant"] == 5, sts
    else:
        assert sts["mac_variant"] == stt["mac_variant"], (sts, stt)   # finite operands: the flag says so, the forced kernel runs
    refS, rstS = oracle_product(oracle, fam, dtype, exact_products)
    compare_with_oracle(Cs, refS, exact_bits, sts, rstS)
    if fam.no_nan:
        assert np.isfinite(Cs.host_arrays()[3]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["inf_a", "nan_a"])
@pytest.mark.parametrize("path", ["pipe_seg", "tasklist"])
def test_special_values_fp64(oracle, bmsp, monkeypatch, name, path):
    """fp64 operands hold no cached flag (every kernel multiplies whole tiles): the pipeline and the row-merge task-list mode."""
    fam = family(name)
    env, mode = PATHS[path]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    for A, B, twin in ((fam.At, fam.Bt, True), (fam.A, fam.B, False)):
        a, b = _make(bmsp, A, B, 2)
        Cm, st = bmsp.spgemm(a, b, mode=mode, tc_version=5)
        assert st["sort_path"] == (2 if path == "tasklist" else 1) or (path == "pipe_seg" and st["sort_path"] == 0), st
        assert st["mac_variant"] == 0 and st["mac_kernel"] == 5, st
        ref, rst = oracle_product(oracle, fam, 2, False, twin=twin)
        compare_with_oracle(Cm, ref, True, st, rst)


# ---------------------------------------------------------------------------------------------------------
# 3. the cached flag follows the values
# ---------------------------------------------------------------------------------------------------------
def _flag_coo(salt):
    """203 x 203, band of half width 12: tiles more than a quarter full (the strip kernel, not the row-sparse one), ragged last block-row"""
    from pybmsp import gen
    n, _, r, c, _ = gen.banded(203, 12)
    return (n, n, r, c, _ints(r, c, salt))


def _oracle_of(oracle, M):
    """the oracle's matrix of a handle's CURRENT arrays"""
    i = M.info()
    k, b, o, v = M.host_arrays()
    return oracle.Bmsp(i["num_rows"], i["num_cols"], i["dtype"], i["transposed"], k, b, o, v.astype(np.float64))


def _write_values(bmsp, M, coo, dtype, layout):
    """the values of `coo` (M's structure) into M's value array through the public pointer, then bmsp_matrix_invalidate(M, 0)"""
    src = bmsp.BmSpMatrix.from_coo(*coo, transposed=layout, dtype=dtype)
    d, s = M.device_arrays()[3], src.device_arrays()[3]
    assert d.n == s.n
    bmsp.check(bmsp.lib().bmsp_memcpy_d2d(d.ptr, s.ptr, d.n * d.dtype.itemsize))
    bmsp.synchronize()
    M.invalidate(False)


ROUTES = ["raw", "raw_borrowed", "copy_layout", "copy_transpose", "add_values", "scale_values", "scale_inplace", "sddmm_inplace"]


def _route(bmsp, route, dtype, layout, salt):
    """(M, poison, restore, keep): a matrix in tile layout `layout` with finite integer values, and the two calls that make its values
    non-finite and finite again by `route`"""
    coo = _flag_coo(salt)
    n, _, r, c, v = coo
    p = _find(coo, 101, 99)
    bad = v.copy(); bad[p] = INF
    bad_coo = coo[:4] + (bad,)
    npdt = NPDT[dtype]
    ones = bmsp.DeviceArray.from_host(np.ones(n, np.float32))
    if route in ("raw", "raw_borrowed", "scale_inplace"):
        if route == "scale_inplace":   # one stored zero in the column that is divided by zero: 0 / 0 = NaN next to x / 0 = +-Inf
            v = v.copy(); v[_find(coo, 98, 99)] = 0.0
            coo = coo[:4] + (v,)
        M = bmsp.BmSpMatrix.from_coo(*coo, transposed=layout, dtype=dtype)
        keep = [M]
        if route == "raw_borrowed":
            M = bmsp.BmSpMatrix.from_device_arrays(n, n, *M.device_arrays(), dtype=dtype, transposed=layout)
        restore = lambda: _write_values(bmsp, M, coo, dtype, layout)
        if route == "scale_inplace":   # down column 99 (no way back by the same call -- Inf * x stays Inf: the raw write restores)
            d0 = np.ones(n, np.float32); d0[99] = 0.0
            dz = bmsp.DeviceArray.from_host(d0)
            poison = lambda: M.scale_(right=dz, div_right=True)
        else:
            poison = lambda: _write_values(bmsp, M, bad_coo, dtype, layout)
        return M, poison, restore, keep
    if route in ("copy_layout", "copy_transpose"):
        if route == "copy_layout":
            src = bmsp.BmSpMatrix.from_coo(*coo, transposed=not layout, dtype=dtype)
            M = src.with_layout(layout)
            tr = lambda q: q
        else:
            tr = lambda q: (q[1], q[0], q[3], q[2], q[4])
            src = bmsp.BmSpMatrix.from_coo(*tr(coo), transposed=not layout, dtype=dtype)
            M = src.transpose(layout)
        def poison():
            _write_values(bmsp, src, tr(bad_coo), dtype, not layout)
            M.copy_values_from(src)
        def restore():
            _write_values(bmsp, src, tr(coo), dtype, not layout)
            M.copy_values_from(src)
        return M, poison, restore, [src]
    if route == "add_values":
        # fp16: 60000 + 60000 overflows; fp32: alpha = 1e30 times 1e30 does.  The finite state is 0 * X + Y
        big = 60000.0 if dtype == 1 else 1e30
        y = v.copy()
        if dtype == 1:
            y[p] = big
        X = bmsp.BmSpMatrix.from_coo(n, n, r[[p]], c[[p]], np.array([big]), transposed=layout, dtype=dtype)
        Y = bmsp.BmSpMatrix.from_coo(n, n, r, c, y, transposed=layout, dtype=dtype)
        M = bmsp.add(X, Y, 0.0, 1.0, transposed=layout)
        poison = lambda: bmsp.add_values(M, X, Y, 1.0 if dtype == 1 else 1e30, 1.0)
        restore = lambda: bmsp.add_values(M, X, Y, 0.0, 1.0)
        return M, poison, restore, [X, Y]
    if route == "scale_values":     # into a derived matrix: x / 0 = +-Inf down column 99 and, from a stored zero, 0 / 0 = NaN
        z = v.copy(); z[_find(coo, 98, 99)] = 0.0
        src = bmsp.BmSpMatrix.from_coo(n, n, r, c, z, transposed=layout, dtype=dtype)
        M = bmsp.scale(src, right=ones)
        d0 = np.ones(n, np.float32); d0[99] = 0.0
        dz = bmsp.DeviceArray.from_host(d0)
        poison = lambda: bmsp.scale_values(M, src, right=dz, div_right=True)
        restore = lambda: bmsp.scale_values(M, src, right=ones, div_right=True)
        return M, poison, restore, [src, ones, dz]
    if route == "sddmm_inplace":    # values x_i . y_j, k = 2; one Inf in X
        M = bmsp.BmSpMatrix.from_coo(*coo, transposed=layout, dtype=dtype)
        i = np.arange(n)
        X = np.stack([1.0 + i % 2, np.where(i % 3 == 0, -1.0, 1.0)], axis=1)
        Y = np.stack([np.where(i % 5 == 0, -1.0, 1.0), 1.0 + (i + 1) % 2], axis=1)
        Xb = X.copy(); Xb[101, 0] = INF
        dX, dXb, dY = (bmsp.DeviceArray.from_host(q.astype(npdt).ravel()) for q in (X, Xb, Y))
        restore = lambda: M.sddmm_(dX, dY, 2)
        poison = lambda: M.sddmm_(dXb, dY, 2)
        restore()
        return M, poison, restore, [dX, dXb, dY]
    raise ValueError(route)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("switch", ["BMSP_MAC_STRIP", "BMSP_SPGEMM_ROWMERGE"])
@pytest.mark.parametrize("dtype", [0, 1])
def test_flag_follows_the_values(oracle, bmsp, monkeypatch, dtype, switch, which, route):
    """Finite operands, prepare(3) and a product: the strip kernel runs, the flag is cached as 1 and the dense / lane tile copies exist.
    Then the values of one operand (A, or the column-major B) turn non-finite by `route`: the next product must be the oracle's product of
    the handle's CURRENT arrays and must not come from a fast kernel.  Then finite again by the same route: the oracle's product again,
    and the strip kernel again -- the flag is not stuck at 0."""
    monkeypatch.setenv(switch, "1")
    tc = 4 if dtype == 1 else 5
    layout = which == "B"
    M, poison, restore, keep = _route(bmsp, route, dtype, layout, 0)
    other = bmsp.BmSpMatrix.from_coo(*_flag_coo(1), transposed=not layout, dtype=dtype)
    a, b = (other, M) if layout else (M, other)
    a.prepare(3); b.prepare(3)

    def product(fast):
        Cm, st = bmsp.spgemm(a, b, tc_version=tc)
        ref, rst = oracle.spgemm(_oracle_of(oracle, a), _oracle_of(oracle, b), exact_products=(dtype == 1))
        finite = np.isfinite(M.host_arrays()[3]).all()
        assert finite == fast, "the route left the values %s" % ("finite" if finite else "non-finite")
        assert (st["mac_variant"] == 3) if fast else (st["mac_variant"] not in FAST), st
        compare_with_oracle(Cm, ref, exact_bits_for(dtype, tc), st, rst)
        return ref

    first = product(True)
    poison()
    assert not np.isfinite(product(False).values).all()
    restore()
    again = product(True)
    if route != "scale_inplace":
        np.testing.assert_array_equal(again.values, first.values)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("dtype", [0, 1])
def test_numeric_after_values_turn_non_finite(oracle, bmsp, dtype, which):
    """bmsp_spgemm_symbolic + bmsp_spgemm_numeric on finite operands: the strip kernel alone, and the oracle's values.  Then an operand
    turns non-finite in place (bmsp_matrix_invalidate(m, 0)): bmsp_spgemm_numeric into the SAME stamped C must give the oracle's values,
    and not through the strip kernel alone."""
    tc = 4 if dtype == 1 else 5
    layout = which == "B"
    M, poison, restore, keep = _route(bmsp, "raw", dtype, layout, 0)
    other = bmsp.BmSpMatrix.from_coo(*_flag_coo(1), transposed=not layout, dtype=dtype)
    a, b = (other, M) if layout else (M, other)
    sym, _ = bmsp.spgemm_symbolic(a, b, tc_version=tc)
    for fast in (True, False, True):
        stn = bmsp.spgemm_numeric(a, b, sym, tc_version=tc)
        ref, _ = oracle.spgemm(_oracle_of(oracle, a), _oracle_of(oracle, b), exact_products=(dtype == 1))
        assert (stn["mac_variant"] == 3) if fast else (stn["mac_variant"] not in FAST), stn
        compare_with_oracle(sym, ref, exact_bits_for(dtype, tc))
        assert np.isfinite(ref.values).all() == fast
        poison() if fast else restore()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tc", [(1, 4), (0, 5)])
def test_structural_refusal_keeps_the_pair_hint(bmsp, dtype, tc):
    """The other side of the rule above: a pair that strip mode refuses for its STRUCTURE (finite values, hub block-rows: the R-MAT of
    test_spgemm_rowwindow_path[rmat13]) still remembers what it needed.  The first product tries the task-list pass, gives it up on the
    hub rows and takes the column windows (sort_long 1); every later product goes straight to the window passes (sort_long 0)."""
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(13, 16)
    v = np.round(v * 8) / 8
    a = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, dtype=dtype)
    b = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, transposed=True, dtype=dtype)
    first, st1 = bmsp.spgemm(a, b, tc_version=tc)
    assert st1["sort_path"] == 3 and st1["sort_long"] == 1, st1
    for _ in range(2):
        again, st2 = bmsp.spgemm(a, b, tc_version=tc)
        assert st2["sort_path"] == 3 and st2["sort_long"] == 0, st2
        for x, y in zip(first.host_arrays(), again.host_arrays()):
            np.testing.assert_array_equal(x, y)


# ---------------------------------------------------------------------------------------------------------
# 4. row-panel views and the sharded product: a view computes its flag over its own slice of the values
# ---------------------------------------------------------------------------------------------------------
def _panel_operands(inf_in):
    """483 x 483 bands (ragged last block-row), B's values not A's; one Inf in the last third of A's block-rows, or in B"""
    from pybmsp import gen
    n, _, r, c, _ = gen.banded(483, 12)
    va, vb = _ints(r, c, 0), _ints(r, c, 1)
    coo = (n, n, r, c, va)
    (va if inf_in == "A" else vb)[_find(coo, 451, 449)] = INF
    return (n, n, r, c, va), (n, n, r, c, vb)


@pytest.mark.gpu
@pytest.mark.parametrize("inf_in", ["A", "B"])
@pytest.mark.parametrize("dtype", [0, 1])
def test_views_and_shards_keep_their_own_flag(oracle, bmsp, monkeypatch, dtype, inf_in):
    """Three row-panel views of A times B, concatenated, and the sharded product on a loopback communicator of three (rounds 0 and 1,
    gathered and owner-keeps) equal the oracle's product of the whole.  With the Inf in A's last panel only that panel leaves the strip
    kernel -- the finite panels keep it; with the Inf in B every panel falls back.  (Integer inputs: the kernels agree exactly.)"""
    monkeypatch.setenv("BMSP_MAC_STRIP", "1")
    tc = 4 if dtype == 1 else 5
    Ac, Bc = _panel_operands(inf_in)
    A, B = _make(bmsp, Ac, Bc, dtype)
    ref, rst = oracle.spgemm(oracle.bmsp_from_coo(oracle.Coo(*Ac), dtype, False), oracle.bmsp_from_coo(oracle.Coo(*Bc), dtype, True),
                             exact_products=(dtype == 1))
    assert np.isnan(ref.values).any()
    exact_bits = exact_bits_for(dtype, tc)
    bounds = bmsp.partition_rows(A, B, 3)
    assert np.all(np.diff(bounds) > 0), bounds
    panels, keep, variants = [], [], []
    for p in range(3):
        view = A.row_panel(bounds[p], bounds[p + 1])
        Cp, st = bmsp.spgemm(view, B, tc_version=tc)
        keep.append((view, Cp))
        panels.append(Cp.device_arrays())
        variants.append(st["mac_variant"])
    with_inf = [p for p in range(3) if bounds[p] <= 451 // 8 < bounds[p + 1]] if inf_in == "A" else [0, 1, 2]
    assert with_inf == ([2] if inf_in == "A" else [0, 1, 2]), bounds
    assert all(variants[p] not in FAST for p in with_inf), variants
    if inf_in == "A":
        assert any(variants[p] == 3 for p in range(3) if p not in with_inf), variants
    compare_with_oracle(bmsp.concat_panels(Ac[0], Bc[1], panels), ref, exact_bits)
    comm = bmsp.Comm.loopback(3)
    for rounds, gather in ((0, True), (1, True), (0, False)):
        Cs, st, sh = bmsp.spgemm_sharded(comm, A, B, tc_version=tc, rounds=rounds, gather=gather)
        assert sh["world"] == 3 and st["surviving_tasks"] == rst["surviving_tasks"] and st["c_blocks"] == rst["c_blocks"], (st, sh)
        compare_with_oracle(Cs, ref, exact_bits)
    comm.free()


# ---------------------------------------------------------------------------------------------------------
# 5. SpMV / SpMM: x is never read where the matrix stores no tile
# ---------------------------------------------------------------------------------------------------------
def _gap_matrix(kind):
    """(nr, nc, r, c, v, empty block-columns, empty block-rows): integer values; no tile in block-column 0, in the last, ragged one and
    in every seventh between; the same for the block-rows.  sparse: ~3 values per tile; dense: full tiles in a band"""
    from pybmsp import gen
    if kind == "sparse":
        nr, nc = 1237, 911
        g = np.random.default_rng(77)
        r, c = g.integers(0, nr, 14000), g.integers(0, nc, 14000)
    else:
        nr = nc = 1003
        _, _, r, c, _ = gen.banded(1003, 21)
    key = np.unique(np.asarray(r, np.int64) * nc + np.asarray(c, np.int64))
    r, c = (key // nc).astype(np.int32), (key % nc).astype(np.int32)
    gap = lambda b, last: (b == 0) | (b == last) | (b % 7 == 3)
    keep = ~gap(c // 8, (nc - 1) // 8) & ~gap(r // 8, (nr - 1) // 8)
    r, c = r[keep], c[keep]
    bcols, brows = np.arange((nc + 7) // 8), np.arange((nr + 7) // 8)
    return nr, nc, r, c, _ints(r, c, 2), bcols[gap(bcols, (nc - 1) // 8)], brows[gap(brows, (nr - 1) // 8)]


def _poisoned_x(n, empty_blocks, width=None):
    """(x, x0): small integers; x holds Inf and NaN, alternating, at every index of the empty blocks, x0 zeros there"""
    x0 = ((np.arange(n) % 21) - 10).astype(np.float64)
    if width:
        x0 = x0[:, None] + (np.arange(width) % 3)[None, :]
    x = x0.copy()
    for b in empty_blocks:
        lo, hi = 8 * b, min(n, 8 * b + 8)
        x0[lo:hi] = 0.0
        x[lo:hi:2] = INF
        x[lo + 1:hi:2] = NAN
    return x, x0


@pytest.mark.gpu
@pytest.mark.parametrize("launch,dtype", spmv_launch_params())
def test_spmv_padding_adds_nothing(oracle, bmsp, monkeypatch, launch, dtype):
    """x = Inf / NaN wherever the matrix stores no tile (block-column 0, the last, ragged one, every seventh): the sweep must not read
    them -- no output is Inf or NaN, the result equals the sweep of x with zeros there bit for bit, and (integer inputs: exact in any
    order) the float64 product and, for fp32 (the oracle's SpMV is fp32 only), the oracle's sweep of the zeroed x."""
    kind, env, variant, kernel = SPMV_LAUNCHES[launch]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    nr, nc, r, c, v, ebc, _ = _gap_matrix(kind)
    A = bmsp.BmSpMatrix.from_coo(nr, nc, r, c, v, dtype=dtype)
    assert bmsp.spmv_launch_info(A, variant)["kernel"].startswith(kernel), bmsp.spmv_launch_info(A, variant)
    if launch in SPMV_CHUNK_LAYOUT:   # (the two chunk launches share the kernel's name: the layout tells them apart)
        assert bmsp.spmv_chunk_layout(A) == SPMV_CHUNK_LAYOUT[launch]
    x, x0 = _poisoned_x(nc, ebc)
    out = []
    for xs in (x, x0):
        y = bmsp.DeviceArray(nr, bmsp.OUT_DTYPE[dtype])
        bmsp.check(bmsp.lib().bmsp_memset(y.ptr, 0xFF, nr * y.dtype.itemsize))
        bmsp.check(bmsp.lib().bmsp_spmv(A.h, bmsp.DeviceArray.from_host(xs.astype(NPDT[dtype])).ptr, y.ptr, variant, None))
        out.append(y.to_host())
    assert np.isfinite(out[0]).all(), np.flatnonzero(~np.isfinite(out[0]))[:8]
    np.testing.assert_array_equal(out[0].view(np.uint8), out[1].view(np.uint8))
    np.testing.assert_array_equal(out[1].astype(np.float64), util.scipy_csr(nr, nc, r, c, v) @ x0)
    if dtype == 0:
        ref = oracle.bmsp_from_coo(oracle.Coo(nr, nc, r, c, v), 0, False)
        np.testing.assert_array_equal(out[0], oracle.spmv_f32(ref, x0.astype(np.float32)))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("layout", [False, True])
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_spmv_op_padding_adds_nothing(oracle, bmsp, kind, op, layout, dtype):
    """the same for bmsp_spmv_op, op N and T on both tile layouts; for op T the special values sit at the ROWS of the block-rows that hold
    no tile.  The oracle has no op(A) sweep and no SpMM: the independent reference of this test and the next is the float64 product,
    which integer inputs make exact in any order; the oracle's own sweep is compared where it applies (fp32, op N, row-major tiles)."""
    nr, nc, r, c, v, ebc, ebr = _gap_matrix(kind)
    A = bmsp.BmSpMatrix.from_coo(nr, nc, r, c, v, transposed=layout, dtype=dtype)
    n_in, empty = (nr, ebr) if op == "T" else (nc, ebc)
    x, x0 = _poisoned_x(n_in, empty)
    S = util.scipy_csr(nr, nc, r, c, v)
    out = [bmsp.spmv_op(A, bmsp.DeviceArray.from_host(xs.astype(NPDT[dtype])), op).to_host() for xs in (x, x0)]
    assert np.isfinite(out[0]).all(), np.flatnonzero(~np.isfinite(out[0]))[:8]
    np.testing.assert_array_equal(out[0].view(np.uint8), out[1].view(np.uint8))
    np.testing.assert_array_equal(out[1].astype(np.float64), (S.T if op == "T" else S) @ x0)
    if dtype == 0 and op == "N" and not layout:
        ref = oracle.bmsp_from_coo(oracle.Coo(nr, nc, r, c, v), 0, False)
        np.testing.assert_array_equal(out[0], oracle.spmv_f32(ref, x0.astype(np.float32)))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("launch", list(SPMM_LAUNCHES))
def test_spmm_padding_adds_nothing(bmsp, monkeypatch, launch, dtype):
    """the same for every SpMM kernel test_spmm.py pins (spmm_kernel<64> needs 2^32 values and is out of reach): the rows of X of the
    block-columns that hold no tile are Inf / NaN"""
    kind, novs, k, kernel = SPMM_LAUNCHES[launch]
    if novs:
        monkeypatch.setenv("BMSP_SPMM_NO_VSTREAM", "1")
    nr, nc, r, c, v, ebc, _ = _gap_matrix(kind)
    A = bmsp.BmSpMatrix.from_coo(nr, nc, r, c, v, dtype=dtype)
    assert bmsp.spmm_launch_info(A, k) == kernel
    X, X0 = _poisoned_x(nc, ebc, width=k)
    out = [bmsp.spmm(A, bmsp.DeviceArray.from_host(Xs.astype(NPDT[dtype]).ravel()), k).to_host() for Xs in (X, X0)]
    assert np.isfinite(out[0]).all(), np.flatnonzero(~np.isfinite(out[0]))[:8]
    np.testing.assert_array_equal(out[0].view(np.uint8), out[1].view(np.uint8))
    np.testing.assert_array_equal(out[1].astype(np.float64).reshape(nr, k), util.scipy_csr(nr, nc, r, c, v) @ X0)
