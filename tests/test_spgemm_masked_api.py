"""CPU tests of the surface of bmsp_spgemm_masked: the C entry points refuse bad scalars and null handles with BMSP_ERR_INVALID and name
the argument, scalars before handles, all before any device call; the Python wrappers refuse aliasing, shapes and dtype combinations from
info() alone; the symbols are exported and declared with their exact prototypes; the Python and C++ wrappers exist and link; and the
generated inputs of the GPU file (tests/test_spgemm_masked.py) meet the conditions its bit-for-bit comparisons rest on."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from conftest import REPO

BMSP_ERR_INVALID = -1


def build_cpp_spgemm_masked_check(out_path):
    lib_dir = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp_spgemm_masked_check.cpp"), "-o", out_path, "-L" + lib_dir, "-lbmsp",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def _msg(bmsp):
    return bmsp.lib().bmsp_last_error().decode(errors="replace")


def calls(bmsp, beta=0.0, flags=0, lay=0, out=True, info=True):
    """the three entry points with null A, B and M: [(name, status, message)]"""
    L = bmsp.lib()
    h, inf = C.c_void_p(), bmsp.SpgemmMaskedInfo()
    res = []
    res.append(("bmsp_spgemm_masked", L.bmsp_spgemm_masked(None, None, None, 1.0, beta, flags, lay, None, C.byref(h) if out else None), _msg(bmsp)))
    res.append(("bmsp_spgemm_masked_values", L.bmsp_spgemm_masked_values(None, None, None, 1.0, beta, flags, None, None), _msg(bmsp)))
    if not flags and not beta:
        res.append(("bmsp_spgemm_masked_launch_info", L.bmsp_spgemm_masked_launch_info(None, None, None, lay, C.byref(inf) if info else None),
                    _msg(bmsp)))
    return res


# ---------------------------------------------------------------------------------------------------------
# refusals through the raw C calls, null handles
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,word", [(dict(flags=2), "flags"), (dict(flags=-1), "flags"), (dict(flags=3), "flags"), (dict(flags=1, beta=0.5), "beta"),
                                     (dict(flags=1, beta=-1.0), "beta")])
def test_bad_scalars_are_refused_before_the_handles(bmsp, kw, word):
    for ptrs in (dict(), dict(out=False, info=False)):
        for name, status, msg in calls(bmsp, **kw, **ptrs):
            assert status == BMSP_ERR_INVALID, name
            assert word in msg and "null" not in msg, (name, msg)


@pytest.mark.parametrize("lay", [2, -1, 1 << 16])
def test_bad_out_transposed_is_refused_before_the_handles(bmsp, lay):
    L = bmsp.lib()
    h, inf = C.c_void_p(), bmsp.SpgemmMaskedInfo()
    for hp, ip in ((None, None), (C.byref(h), C.byref(inf))):
        assert L.bmsp_spgemm_masked(None, None, None, 1.0, 0.0, 0, lay, None, hp) == BMSP_ERR_INVALID
        assert "out_transposed" in _msg(bmsp) and "null" not in _msg(bmsp), _msg(bmsp)
        assert L.bmsp_spgemm_masked_launch_info(None, None, None, lay, ip) == BMSP_ERR_INVALID
        assert "out_transposed" in _msg(bmsp) and "null" not in _msg(bmsp), _msg(bmsp)


def test_null_handles_are_refused_after_the_scalars(bmsp):
    for kw in (dict(), dict(out=False, info=False), dict(flags=1), dict(beta=2.0), dict(lay=1)):
        for name, status, msg in calls(bmsp, **kw):
            assert status == BMSP_ERR_INVALID, name
            assert "null" in msg and "A" in msg and "must" not in msg, (name, msg)


class Fake:
    """stands in for a matrix: the wrappers refuse from info() alone, before any C call (h is None: a C call would refuse the null)"""
    h = None

    def __init__(self, nr, nc, dtype=0, lay=0):
        self._i = {"num_rows": nr, "num_cols": nc, "dtype": dtype, "transposed": lay, "nnz": 0, "block_num": 0}

    def info(self):
        return dict(self._i)


def test_python_wrappers_refuse_bad_arguments(bmsp):
    A, B, M = Fake(5, 3), Fake(3, 7), Fake(5, 7)
    bad = [(A, Fake(4, 7), M), (A, B, Fake(5, 6)), (A, B, Fake(6, 7)),          # shapes that do not chain, M not m x p
           (A, Fake(3, 7, 1), M), (Fake(5, 3, 2), B, M),                          # A and B differ in dtype
           (A, B, Fake(5, 7, 1)), (A, B, Fake(5, 7, 2)),                          # F32 operands: M must be F32
           (Fake(5, 3, 1), Fake(3, 7, 1), Fake(5, 7, 2)),                         # F16 operands: M is F16 or F32
           (Fake(5, 3, 2), Fake(3, 7, 2), Fake(5, 7, 0))]                         # F64 operands: M must be F64
    for a, b, m in bad:
        with pytest.raises(ValueError):
            bmsp.spgemm_masked(a, b, m)
        with pytest.raises(ValueError):
            bmsp.spgemm_masked_values(m, a, b, m)
        with pytest.raises(ValueError):
            bmsp.spgemm_masked_launch_info(a, b, m)
    with pytest.raises(ValueError):
        bmsp.spgemm_masked(A, B, M, 1.0, 0.5, mul_m=True)
    with pytest.raises(ValueError):
        bmsp.spgemm_masked_values(M, A, B, M, 1.0, 0.5, mul_m=True)
    # out aliasing A or B (square, so that every shape chains)
    S, T = Fake(8, 8), Fake(8, 8)
    for out, a, b, m in ((S, S, T, S), (T, S, T, T), (S, S, S, S)):
        with pytest.raises(ValueError):
            bmsp.spgemm_masked_values(out, a, b, m)
    # the four dtype combinations pass the wrapper's checks: the C call then refuses the null handle
    for da, dm in ((0, 0), (1, 1), (1, 0), (2, 2)):
        with pytest.raises(bmsp.BmspError) as e:
            bmsp.spgemm_masked(Fake(5, 3, da), Fake(3, 7, da), Fake(5, 7, dm))
        assert e.value.status == BMSP_ERR_INVALID and "null" in str(e.value)


# ---------------------------------------------------------------------------------------------------------
# symbols and wrappers
# ---------------------------------------------------------------------------------------------------------
def test_spgemm_masked_symbols_are_declared(bmsp):
    for name in ("bmsp_spgemm_masked", "bmsp_spgemm_masked_values", "bmsp_spgemm_masked_launch_info"):
        assert name in bmsp.SYMBOLS and hasattr(bmsp.lib(), name)
    with open(os.path.join(REPO, "include", "bmsp.h")) as f:
        text = f.read()
    for line in ("#define BMSP_MASKED_MUL_M 1   /* flags bit 0: c = fl(fl(alpha*d) * m) instead of fl(fl(alpha*d) + fl(beta*m)); beta must be 0 */",
                 "int bmsp_spgemm_masked(bmsp_matrix_t A, bmsp_matrix_t B, bmsp_matrix_t M, double alpha, double beta, int flags,\n"
                 "                       int out_transposed, void *stream, bmsp_matrix_t *out);",
                 "int bmsp_spgemm_masked_values(bmsp_matrix_t A, bmsp_matrix_t B, bmsp_matrix_t M, double alpha, double beta, int flags,\n"
                 "                              bmsp_matrix_t out, void *stream);",
                 "typedef struct { char kernel[64]; int lanes; int64_t pairs, view_bytes; } bmsp_spgemm_masked_info;",
                 "int bmsp_spgemm_masked_launch_info(bmsp_matrix_t A, bmsp_matrix_t B, bmsp_matrix_t M, int out_transposed,\n"
                 "                                   bmsp_spgemm_masked_info *info);"):
        assert line in text, line
    # the ctypes mirror has the C struct's layout: 64 + int (+ padding) + two int64
    I = bmsp.SpgemmMaskedInfo
    assert C.sizeof(I) == 64 + 8 + 16 and I.lanes.offset == 64 and I.pairs.offset == 72 and I.view_bytes.offset == 80
    assert bmsp.MASKED_MUL_M == 1


def test_python_wrappers_exist(bmsp):
    for fn in (bmsp.spgemm_masked, bmsp.spgemm_masked_values, bmsp.spgemm_masked_launch_info, bmsp.BmSpMatrix.mult_masked):
        assert callable(fn)
    with open(os.path.join(REPO, "include", "bmSpMatrix.h")) as f:
        text = f.read()
    assert "inline void bmSparse_mult_masked(" in text and "inline void bmSparse_mult_masked_values(" in text


def test_cpp_spgemm_masked_wrappers_compile_and_link(tmp_path):
    """include/bmSpMatrix.h with bmSparse_mult_masked / bmSparse_mult_masked_values instantiated for float, half (both mask types) and
    double links against libbmsp.so with a plain host compiler."""
    build_cpp_spgemm_masked_check(str(tmp_path / "cpp_spgemm_masked_check"))


# ---------------------------------------------------------------------------------------------------------
# the generated inputs of tests/test_spgemm_masked.py, host only
# ---------------------------------------------------------------------------------------------------------
def test_integer_cases_are_exact_in_every_storage_type(oracle):
    """test 1 of the GPU file compares bit for bit: a, b in [-3, 3] (hub cases {-1, 0, 1}), m in [-4, 4]; every partial sum in any order
    is bounded by sum |a b| < 2^24, an integer exact in fp32 (the arithmetic type of F16 and F32; F16 products are exact there), and
    every result of every epilogue is an exactly representable fp16 number of magnitude at most 2048, hence exact in fp32 and fp64 --
    all in int64 / float64 arithmetic on the very arrays the GPU file uses"""
    import test_spgemm_masked as T
    worst = 0
    for name in T.NAMES:
        a, b, mv = T.int_operands(name)
        lim = 1 if name in T.HUBS else 3
        for x, lo, hi in ((a, -lim, lim), (b, -lim, lim), (mv, -4, 4)):
            assert x.size == 0 or (x.min() >= lo and x.max() <= hi)
        d, s = T.int_dots(name)
        if d.size == 0:
            continue
        assert d.dtype == np.int64 and s.dtype == np.int64
        assert np.all(np.abs(d) <= s) and s.max() < 2 ** 24
        worst = max(worst, int(s.max()))
        for alpha, beta, mul_m in T.EPILOGUES:
            t2 = np.int64(2 * alpha) * d                                          # 2 * alpha * d in int64 (alpha is a multiple of 1/2)
            res2 = t2 * mv if mul_m else t2 + np.int64(2 * beta) * mv             # 2 * c
            assert np.abs(res2).max() <= 2 * 2048, (name, alpha, beta, mul_m, int(np.abs(res2).max()))
            res = res2.astype(np.float64) / 2
            with np.errstate(over="raise"):
                np.testing.assert_array_equal(res.astype(np.float16).astype(np.float64), res, err_msg="%s %s" % (name, (alpha, beta, mul_m)))
                t = t2.astype(np.float64) / 2
                np.testing.assert_array_equal(t.astype(np.float16).astype(np.float64), t)
            for dt in range(len(T.DTYPES)):  # the expectation the GPU file uses (oracle + numpy epilogue) is this very number
                exp = T.int_expected(oracle, name, dt, T.EPILOGUES.index((alpha, beta, mul_m)))
                assert exp.dtype == T.NPDT[T.DTYPES[dt][1]]
                np.testing.assert_array_equal(exp.astype(np.float64), res, err_msg="%s %s %s" % (name, dt, (alpha, beta, mul_m)))
    assert 0 < worst < 2 ** 24


def test_the_oracle_sample_equals_a_dense_product(oracle):
    """the oracle's product sampled on M equals an independent dense numpy product A_dense @ B_dense sampled on M (integer operands:
    both are exact)"""
    import test_spgemm_masked as T
    for name in T.NAMES:
        a, b, _ = T.int_operands(name)
        m, n, p, A, B, M = T.patterns()[name]
        want = (T.dense_of(m, n, A, a) @ T.dense_of(n, p, B, b))[M[0], M[1]]
        for dtype in (0, 1, 2):
            got = T.oracle_dots(oracle, name, a.astype(np.float64), b.astype(np.float64), dtype)
            assert got.dtype == T.ARITH[dtype]
            np.testing.assert_array_equal(got.astype(np.float64), want, err_msg=name)
        np.testing.assert_array_equal(T.int_dots(name)[0], want.astype(np.int64))


def test_real_operands_use_the_whole_mantissa():
    import test_spgemm_masked as T
    for dtype in (0, 1, 2):
        a, b, mv = T.real_operands("random", dtype)
        for x in (a, b):
            # (drawn from [0.5, 2); the rounding to the storage type may land on 2 itself)
            assert np.all((np.abs(x) >= 0.5) & (np.abs(x) <= 2.0)) and (x < 0).any() and (x > 0).any()
            np.testing.assert_array_equal(x.astype(T.NPDT[dtype]).astype(np.float64), x)
            last = T.bits(x.astype(T.NPDT[dtype])) & 1  # the last mantissa bit of the stored value
            assert x.size // 4 < int(last.sum()) < 3 * x.size // 4


def test_case_lists_cover_every_parameter():
    import test_spgemm_masked as T
    cases = T.int_cases()
    assert len(cases) < 300  # the file stays small
    for pos, values in ((0, T.NAMES), (1, range(len(T.DTYPES))), (2, (0, 1)), (3, (0, 1)), (4, (0, 1)), (5, (0, 1)), (6, T.LANES),
                        (7, range(len(T.EPILOGUES)))):
        assert {c[pos] for c in cases} == set(values), pos
    assert {(c[2], c[3], c[4]) for c in cases} == {(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)}  # all 2^3 operand layouts
    big = [c for c in cases if c[0] in ("random", "dense", "rmat", "banded", "13x70x11", "outside") + tuple(T.HUBS)]
    for dt in range(len(T.DTYPES)):
        assert {(c[2], c[3], c[4]) for c in big if c[1] == dt} == {(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)}, dt
        assert {c[5] for c in big if c[1] == dt} == {0, 1} and {c[6] for c in big if c[1] == dt} == set(T.LANES), dt
        assert {c[7] for c in big if c[1] == dt} == set(range(len(T.EPILOGUES))), dt
    order = T.order_cases()
    for pos, values in ((0, T.ORDER_NAMES), (1, range(len(T.DTYPES))), (2, (0, 1)), (3, (0, 1)), (4, (0, 1)), (5, (0, 1)), (6, T.LANES)):
        assert {c[pos] for c in order} == set(values), pos


def test_the_patterns_are_what_the_cases_need():
    import test_spgemm_masked as T
    pats = T.patterns()
    tiles = lambda rc, ncols: np.unique((rc[0] // 8) * ((ncols + 7) // 8) + rc[1] // 8)
    # the hub cases have the list lengths stated, their matches include the first and the last entry of the longer list, one has none
    for name, (la, lb) in T.HUBS.items():
        m, n, p, A, B, M = pats[name]
        ka, kb = np.unique(A[1] // 8), np.unique(B[0] // 8)
        assert m == 8 and p == 8 and ka.size == la == A[0].size and kb.size == lb == B[0].size, name
        assert tiles(M, p).size == 1 and M[0].size == 64
        common = np.intersect1d(ka, kb)
        assert T.expected_pairs(name) == common.size
        if name == "hub_nomatch":
            assert common.size == 0
            continue
        longer = ka if la >= lb else kb
        assert longer[0] in common and longer[-1] in common, name
        shorter = kb if la >= lb else ka
        assert shorter[0] in common and shorter[-1] in common, name
        a, b, _ = T.int_operands(name)
        assert np.count_nonzero(T.int_dots(name)[0]) > 0, name  # the matches carry products
    assert pats["hub300x3"][1] == 2400 and pats["hub3x300"][1] == 2400
    # dense and hyper-sparse mask tiles: both sides of 6 values per tile, the fill at which the tile-wise family changes its lane group
    # (the masked product takes eight lanes at every fill: T.FILL_THRESHOLD)
    for name, full in (("dense", True), ("banded", True), ("rmat", False), ("random", False)):
        m, n, p, A, B, M = pats[name]
        assert (M[0].size >= 6 * tiles(M, p).size) == full, name
    assert T.FILL_THRESHOLD == 0
    m, n, p, A, B, M = pats["dense"]
    assert M[0].size == 64 * tiles(M, p).size  # full tiles
    assert np.unique(pats["13x70x11"][3][1] // 8).size == 9  # nine inner blocks
    # more than one workgroup of tiles at one lane per tile and at eight
    assert tiles(pats["rmat"][5], 1024).size > 256 and 8 * tiles(pats["banded"][5], 133).size > 256
    # "outside": coordinates inside product tiles that the product does not hold, and whole mask tiles without a candidate pair
    m, n, p, A, B, M = pats["outside"]
    a, b, _ = T.int_operands("outside")
    held = (T.dense_of(m, n, A, np.ones(A[0].size)) @ T.dense_of(n, p, B, np.ones(B[0].size))) > 0
    assert (~held[M[0], M[1]]).sum() > 100 and held[M[0], M[1]].sum() > 10
    assert np.any(M[0] >= 8) and np.any(M[1] >= 16) and T.expected_pairs("outside") > 0
    # the empty cases
    assert pats["a0"][3][0].size == 0 and pats["b0"][4][0].size == 0 and pats["m0"][5][0].size == 0 and pats["rows0"][0] == 0
    # ragged everywhere
    for name in ("5x3x7", "13x70x11", "random"):
        assert all(x % 8 for x in pats[name][:3]), name
