"""CPU tests of the surface of bmsp_matrix_fsai / bmsp_fsai_*, and what tests/test_zzzzzzzzzzzzz_fsai.py shares with them: the C reference
(tests/fsai_ref.c through ctypes: include/bmsp.h's arithmetic restated with fmaf / fma, gcc -O2 -ffp-contract=off), the inputs of every
regime and their self-checks.

Inputs (all (n, r, c, v) sorted by (row, col), v float64 holding values of the dtype; patterns (n, r, c)):
    dominant(n, density, seed)   random at the density, the diagonal 1 + 1.1 * the larger of the row's and the column's absolute
                                 off-diagonal sum: every principal sub-matrix of A and of A^T is strictly dominant, LU needs no pivoting
    lane_pattern(n, longest)     rows of length 1, 7, 8, 9, ... up to `longest` (and min(i + 1, .)), columns drawn at random below the diagonal
    far_case / hub_case / mismatch_case / special_case   the walks and the special values the GPU file names
    poisson7 / nonsym7           the two 8^3 stencils of the convergence tests

Checks here: SPD with the full pattern gives inv(cholesky(A)); GENERAL with full patterns gives W^T L A = I; the two scalings; the
regime inputs are what they claim; the header and pybmsp carry the interface."""
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile
import numpy as np
import pytest
from conftest import REPO
from test_spsv_api import VEC, NP

NONE, SQRT, UNIT = 0, 1, 2
LONGEST = (1, 8, 9, 16, 17, 32, 33, 64)
LENGTHS = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)


@functools.lru_cache(maxsize=None)
def ref_lib():
    d = tempfile.mkdtemp(prefix="fsai_ref_")
    so = os.path.join(d, "libfsai_ref.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(REPO, "tests", "fsai_ref.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp = C.c_void_p
    for fn in (L.fsai_ref_f32, L.fsai_ref_f64):
        fn.argtypes = [C.c_int64, vp, vp, vp, vp, vp, C.c_int, vp, vp]
        fn.restype = C.c_int64
    return L


def sort_coo(n, r, c, v=None):
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    o = np.lexsort((c, r))
    return (n, r[o], c[o]) if v is None else (n, r[o], c[o], np.asarray(v, np.float64)[o])


def _csr_ptr(n, r):
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=ptr[1:])
    return ptr


def reference(A, S, dtype, op="N", scale=SQRT):
    """(g, pivot, bad): G's values in S's (row, col) order, the n values y_m and the count of bad rows, by tests/fsai_ref.c"""
    R = VEC[dtype]
    n, ar, ac, av = A
    if op == "T":
        n, ar, ac, av = sort_coo(n, ac, ar, av)
    _, sr, sc = S[:3]
    a_ptr, s_ptr = _csr_ptr(n, ar), _csr_ptr(n, sr)
    a_col, s_col = np.ascontiguousarray(ac, np.int64), np.ascontiguousarray(sc, np.int64)
    a_val = np.ascontiguousarray(np.asarray(av, NP[dtype]).astype(R))
    g, piv = np.zeros(max(s_col.size, 1), R), np.zeros(max(n, 1), R)
    fn = ref_lib().fsai_ref_f64 if R is np.float64 else ref_lib().fsai_ref_f32
    with np.errstate(all="ignore"):
        bad = fn(n, a_ptr.ctypes.data, a_col.ctypes.data, a_val.ctypes.data, s_ptr.ctypes.data, s_col.ctypes.data, scale, g.ctypes.data,
                 piv.ctypes.data)
    assert bad >= 0, "a row of the pattern is longer than 64"
    return g[:s_col.size], piv[:n], int(bad)


def dense_of(M):
    n, r, c, v = M
    D = np.zeros((n, n))
    D[r, c] = v
    return D


# ---------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dominant(n, density, seed, dtype):
    rng = np.random.default_rng(seed)
    mask = rng.random((n, n)) < density
    np.fill_diagonal(mask, True)
    r, c = np.nonzero(mask)
    v = rng.uniform(0.5, 2.0, r.size) * rng.choice([-1.0, 1.0], r.size)
    off = r != c
    rows = np.bincount(r[off], weights=np.abs(v[off]), minlength=n)
    cols = np.bincount(c[off], weights=np.abs(v[off]), minlength=n)
    v[~off] = 1.0 + 1.1 * np.maximum(rows, cols)[r[~off]]
    out = sort_coo(n, r, c, v.astype(NP[dtype]).astype(np.float64))
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def lane_pattern(n, longest, seed=7):
    rng = np.random.default_rng(seed + longest)
    allowed = [l for l in LENGTHS if l <= longest]
    r, c = [], []
    for i in range(n):
        want = longest if i == n - 1 or i == longest - 1 else allowed[rng.integers(len(allowed))]
        m = min(i + 1, want)
        cols = np.sort(rng.choice(i, m - 1, replace=False)) if m > 1 else np.zeros(0, np.int64)
        r += [i] * m
        c += list(cols) + [i]
    return sort_coo(n, r, c)


def lower_of(A):
    n, r, c = A[:3]
    k = c <= r
    return (n, r[k], c[k])


def full_lower(n):
    r, c = np.tril_indices(n)
    return sort_coo(n, r, c)


def row_lengths(S):
    return np.bincount(S[1], minlength=S[0])


def legal(S):
    """every row stores the diagonal and nothing to its right"""
    n, r, c = S[:3]
    return bool((c <= r).all()) and np.array_equal(np.unique(r[r == c]), np.arange(n))


@functools.lru_cache(maxsize=None)
def far_case(dtype):
    """n = 30 013: row i stores i and i - 8 k for scattered k (block columns far apart); A is banded at those offsets plus a few others"""
    n = 30013
    offs = np.array([0, 8, 24, 8 * 37, 8 * 411, 8 * 1999, 8 * 3500])
    i = np.arange(n)
    r = np.concatenate([i[i >= o] for o in offs])
    c = np.concatenate([i[i >= o] - o for o in offs])
    S = sort_coo(n, r, c)
    extra = np.array([1, 5, 8 * 37 + 3])
    ar = np.concatenate([r, c[r != c]] + [i[i >= o] for o in extra])
    ac = np.concatenate([c, r[r != c]] + [i[i >= o] - o for o in extra])
    key = np.unique(ar * n + ac)
    ar, ac = key // n, key % n
    v = -(0.25 + ((ar * 7919 + ac * 104729) % 1000) / 4000.0)
    v[ar == ac] = 9.0
    return sort_coo(n, ar, ac, v.astype(NP[dtype]).astype(np.float64)), S


@functools.lru_cache(maxsize=None)
def hub_case(dtype):
    """n = 4000: row 3999 of A stores 3000 entries, row 3999 of S five (the merge: a long tile list against a short P); every other row of
    S is short too"""
    n = 4000
    rng = np.random.default_rng(3)
    i = np.arange(n)
    hub = np.sort(rng.choice(n - 1, 2999, replace=False))
    ar = np.concatenate([i, i[1:], i[:-1], np.full(hub.size, n - 1)])
    ac = np.concatenate([i, i[:-1], i[1:], hub])
    key = np.unique(ar * n + ac)
    ar, ac = key // n, key % n
    v = -(0.001 + ((ar * 31 + ac * 17) % 100) / 1e5)
    v[ar == ac] = 8.0
    sr = np.concatenate([i, i[1:], np.full(3, n - 1)])
    sc = np.concatenate([i, i[:-1], np.array([5, 1700, 3100])])
    skey = np.unique(sr * n + sc)
    return sort_coo(n, ar, ac, v.astype(NP[dtype]).astype(np.float64)), sort_coo(n, skey // n, skey % n)


@functools.lru_cache(maxsize=None)
def mismatch_case(dtype):
    """n = 70: S holds columns A does not store (+0 entries of B), A entries S does not have, and A stores explicit zeros"""
    A = dominant(70, 0.2, 21, dtype)
    n, r, c, v = A[0], A[1], A[2], A[3].copy()
    off = np.flatnonzero(r != c)
    v[off[::5]] = 0.0                                   # explicit stored zeros
    S = lane_pattern(70, 9, seed=99)
    return (n, r, c, v), S


SPECIALS = ("zero_first_pivot", "zero_last_pivot", "inf", "nan", "negative")


@functools.lru_cache(maxsize=None)
def special_case(kind, dtype):
    """dominant(70) with a few rows' worth of special values: (A, S, the rows of S that reach a special value)"""
    A = dominant(70, 0.3, 5, dtype)
    n, r, c, v = A[0], A[1], A[2], A[3].copy()
    S = lane_pattern(70, 9, seed=4)
    sr, sc = S[1], S[2]
    first_col = {i: int(sc[sr == i].min()) for i in (20, 41, 63)}
    for i in (20, 41, 63):
        d = (r == i) & (c == i)
        if kind == "zero_first_pivot":
            p = first_col[i]
            v[(r == p) & (c == p)] = 0.0
        elif kind == "zero_last_pivot":
            # the last pivot of row i is B_mm after elimination: a row whose pattern is the diagonal alone has B_mm = a_ii
            v[d] = 0.0
        elif kind == "inf":
            v[d] = np.inf
        elif kind == "nan":
            v[d] = np.nan
        else:
            v[d] = -v[d]
    if kind == "zero_last_pivot":                       # rows 20, 41, 63 store the diagonal alone
        keep = ~(np.isin(sr, (20, 41, 63)) & (sr != sc))
        S = (n, sr[keep], sc[keep])
    return (n, r, c, v), S


def stencil7(k, diag, off):
    """the 7-point stencil on k^3 with the six off-diagonals (x-, x+, y-, y+, z-, z+); x is the fastest axis"""
    n = k ** 3
    idx = np.arange(n)
    x, y, z = idx % k, (idx // k) % k, idx // (k * k)
    r, c, v = [idx], [idx], [np.full(n, float(diag))]
    for (ax, step, val, ok) in ((x, -1, off[0], x > 0), (x, 1, off[1], x < k - 1), (y, -k, off[2], y > 0), (y, k, off[3], y < k - 1),
                                (z, -k * k, off[4], z > 0), (z, k * k, off[5], z < k - 1)):
        r.append(idx[ok]); c.append(idx[ok] + step); v.append(np.full(int(ok.sum()), float(val)))
    return sort_coo(n, np.concatenate(r), np.concatenate(c), np.concatenate(v))


def poisson7(k=8):
    return stencil7(k, 6.0, (-1.0,) * 6)


def nonsym7(k=8):
    return stencil7(k, 6.0, (-1.75, -0.25, -1.5, -0.5, -1.0, -1.0))


def solve_rhs(n, dtype, seed=17):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(VEC[dtype])


def dense_factor(S, g):
    G = np.zeros((S[0], S[0]))
    G[S[1], S[2]] = g
    return G


# ---------------------------------------------------------------------------------------------------------
# the reference against linear algebra
# ---------------------------------------------------------------------------------------------------------
def spd24():
    rng = np.random.default_rng(1)
    Q, _ = np.linalg.qr(rng.standard_normal((24, 24)))
    D = Q @ np.diag(np.linspace(1.0, 100.0, 24)) @ Q.T
    D = (D + D.T) / 2
    r, c = np.nonzero(np.ones((24, 24), bool))
    return sort_coo(24, r, c, D[r, c])


def test_spd_full_pattern_is_the_inverse_cholesky_factor():
    A = spd24()
    S = full_lower(24)
    g, piv, bad = reference(A, S, 2, "N", SQRT)
    G = dense_factor(S, g)
    want = np.linalg.inv(np.linalg.cholesky(dense_of(A)))
    err = np.abs(G - want).max()
    print("SPD full pattern: max |G - inv(chol(A))| = %.3e" % err)
    assert bad == 0 and err <= 1e-10
    # scaling: diag(G A G^T) = 1 to 8 u (longest row)
    d = np.diag(G @ dense_of(A) @ G.T)
    assert np.abs(d - 1.0).max() <= 8 * 2.0 ** -53 * 24, np.abs(d - 1.0).max()
    # the pivot is y_m, and under SQRT g_mm = y_m / sqrt(y_m)
    assert np.array_equal(np.diag(G), piv / np.sqrt(piv))


def test_general_full_patterns_invert_exactly():
    rng = np.random.default_rng(2)
    D = rng.uniform(-1.0, 1.0, (12, 12))
    np.fill_diagonal(D, 1.0 + 1.1 * np.maximum(np.abs(D).sum(0), np.abs(D).sum(1)))
    r, c = np.nonzero(np.ones((12, 12), bool))
    A = sort_coo(12, r, c, D[r, c])
    S = full_lower(12)
    gl, _, bl = reference(A, S, 2, "N", NONE)
    gw, _, bw = reference(A, S, 2, "T", UNIT)
    L, W = dense_factor(S, gl), dense_factor(S, gw)
    err = np.abs(W.T @ L @ D - np.eye(12)).max()
    print("GENERAL full patterns: max |W^T L A - I| = %.3e" % err)
    assert bl == 0 and bw == 0 and err <= 1e-10
    assert (np.diag(W) == 1.0).all()                    # a UNIT diagonal is exactly 1


@pytest.mark.parametrize("dtype", [0, 2])
def test_unit_diagonal_is_exactly_one_and_sqrt_scaling_on_sparse_patterns(dtype):
    A = dominant(200, 0.3, 11, dtype)
    for longest in (9, 33):
        S = lane_pattern(200, longest)
        g, piv, bad = reference(A, S, dtype, "T", UNIT)
        assert bad == 0 and np.isfinite(piv).all() and (g[S[1] == S[2]] == 1.0).all()
        gn, pn, _ = reference(A, S, dtype, "N", NONE)
        assert np.array_equal(gn[S[1] == S[2]], pn)     # g = y: the diagonal entry is the pivot


def test_regime_inputs_are_what_they_claim():
    for longest in LONGEST:
        S = lane_pattern(200, longest)
        lens = row_lengths(S)
        assert legal(S) and lens.max() == longest and lens.min() == 1
        assert set(np.unique(lens[longest:])) == {l for l in LENGTHS if l <= longest}, longest
    A = dominant(200, 0.3, 11, 0)
    assert 0.25 < A[1].size / 200 ** 2 < 0.35
    (FA, FS), (HA, HS), (MA, MS) = far_case(0), hub_case(0), mismatch_case(0)
    assert legal(FS) and row_lengths(FS).max() == 7 and (FS[1] - FS[2]).max() == 8 * 3500 and FS[0] % 8 != 0
    assert legal(HS) and np.bincount(HA[1], minlength=4000)[3999] == 3000 and row_lengths(HS)[3999] == 5
    assert reference(FA, FS, 0)[2] == 0 and reference(HA, HS, 2)[2] == 0
    a_keys, s_keys = set(zip(MA[1].tolist(), MA[2].tolist())), set(zip(MS[1].tolist(), MS[2].tolist()))
    assert s_keys - a_keys and a_keys - s_keys and (MA[3] == 0.0).sum() > 10 and legal(MS)
    for kind in SPECIALS:
        for dtype in (0, 2):
            SA, SS = special_case(kind, dtype)
            assert legal(SS)
            g, piv, bad = reference(SA, SS, dtype, "N", SQRT)
            assert 3 <= bad < 70, (kind, bad)           # the rows that reach the special value, and not every row
            rows_bad = np.unique(SS[1][~np.isfinite(g)])
            assert rows_bad.size == bad
    assert reference(special_case("negative", 2)[0], special_case("negative", 2)[1], 2, "N", NONE)[2] == 0   # only SQRT minds the sign
    for M in (poisson7(), nonsym7()):
        assert M[0] == 512 and np.bincount(M[1]).max() == 7
    N = dense_of(nonsym7())
    assert not np.array_equal(N, N.T) and np.array_equal(dense_of(poisson7()), dense_of(poisson7()).T)


def test_prototype_iteration_counts():
    """FSAI on tril(A) against no preconditioner in float64 (dense numpy CG on Poisson 7pt 8^3): the margin the GPU test relies on"""
    A = poisson7()
    D = dense_of(A)
    S = lower_of(A)
    g, _, bad = reference(A, S, 2, "N", SQRT)
    G = dense_factor(S, g)
    assert bad == 0
    b = solve_rhs(512, 2).astype(np.float64)

    def cg(apply):
        x, r = np.zeros(512), b.copy()
        z = apply(r)
        p, rho = z.copy(), r @ z
        for k in range(1, 200):
            q = D @ p
            a = rho / (p @ q)
            x, r = x + a * p, r - a * q
            if np.sqrt(r @ r) <= 1e-6 * np.linalg.norm(b):
                return k
            z = apply(r)
            rho, old = r @ z, rho
            p = z + (rho / old) * p
        return 200
    plain, fsai = cg(lambda r: r / np.diag(D)), cg(lambda r: G.T @ (G @ r))
    print("Poisson 7pt 8^3, float64 CG: jacobi %d iterations, fsai %d" % (plain, fsai))
    assert fsai < plain


# ---------------------------------------------------------------------------------------------------------
# the interface
# ---------------------------------------------------------------------------------------------------------
def test_header_carries_the_interface_and_the_arithmetic():
    text = open(os.path.join(REPO, "include", "bmsp.h")).read()
    flat = re.sub(r"\s+", " ", text.replace(" * ", " "))
    for phrase in ("int bmsp_matrix_fsai(bmsp_matrix_t A, int op, bmsp_matrix_t S, int scale, int out_transposed, void *d_pivot",
                   "int bmsp_matrix_fsai_values(bmsp_matrix_t A, int op, bmsp_matrix_t G, int scale, void *d_pivot, void *stream, bmsp_fsai_info *info);",
                   "L_ak = B_ak / B_kk", "B_ab = fma(-L_ak, B_kb, B_ab)", "y_m = 1 / B_mm", "s = fma(-L_ca, y_c, s)", "q = sqrt(y_m)",
                   "g_a = y_a / y_m", "BMSP_FSAI_LANES=<W>", "tests/fsai_ref.c", "typedef struct bmsp_fsai_s *bmsp_fsai_t;",
                   "#define BMSP_FSAI_SCALE_SQRT 1", "#define BMSP_FSAI_GENERAL 1", "#define BMSP_FSAI_COLMAJOR 2", "\"cg+fsai\"",
                   "more than 64 stored entries"):
        assert re.sub(r"\s+", " ", phrase) in flat, phrase


def test_pybmsp_exposes_every_new_name(bmsp):
    for name in ("fsai", "fsai_values", "fsai_pattern", "Fsai", "FsaiInfo", "FsaiHandleInfo", "FSAI_SCALE_NONE", "FSAI_SCALE_SQRT",
                 "FSAI_SCALE_UNIT", "FSAI_SPD", "FSAI_GENERAL", "FSAI_NO_MATERIALISE", "FSAI_COLMAJOR"):
        assert hasattr(bmsp, name), name
    for name in ("apply", "update", "solve", "solve_gmres", "info", "factors"):
        assert callable(getattr(bmsp.Fsai, name)), name
    assert callable(bmsp.BmSpMatrix.fsai)
    for sym in ("bmsp_matrix_fsai", "bmsp_matrix_fsai_values", "bmsp_fsai_create", "bmsp_fsai_update", "bmsp_fsai_free", "bmsp_fsai_get_info",
                "bmsp_fsai_factors", "bmsp_fsai_apply", "bmsp_fsai_solve", "bmsp_fsai_solve_gmres"):
        assert sym in bmsp.SYMBOLS and hasattr(bmsp.lib(), sym), sym
    assert C.sizeof(bmsp.FsaiInfo) == 64 + 8 + 5 * 8 and C.sizeof(bmsp.FsaiHandleInfo) == 16 + 16 + 2 * C.sizeof(bmsp.FsaiInfo)


def test_scalars_are_refused_before_handles_and_named(bmsp):
    L = bmsp.lib()
    out, info = C.c_void_p(0x5a5a), bmsp.FsaiInfo()
    for args, word in (((None, 2, None, 1, 0), "op"), ((None, 0, None, 3, 0), "scale"), ((None, 0, None, -1, 0), "scale"),
                       ((None, 0, None, 1, 2), "out_transposed")):
        assert L.bmsp_matrix_fsai(args[0], args[1], args[2], args[3], args[4], None, None, C.byref(out), C.byref(info)) == -1
        assert L.bmsp_last_error().decode().startswith(word), (word, L.bmsp_last_error())
    assert L.bmsp_matrix_fsai(None, 0, None, 1, 0, None, None, C.byref(out), C.byref(info)) == -1 and "matrix A" in L.bmsp_last_error().decode()
    assert L.bmsp_matrix_fsai_values(None, 0, None, 5, None, None, C.byref(info)) == -1 and L.bmsp_last_error().decode().startswith("scale")
    assert L.bmsp_matrix_fsai_values(None, 0, None, 1, None, None, C.byref(info)) == -1 and "matrix A" in L.bmsp_last_error().decode()
    h = C.c_void_p(0x5a5a)
    assert L.bmsp_fsai_create(None, None, 2, 0, None, C.byref(h)) == -1 and L.bmsp_last_error().decode().startswith("kind")
    assert L.bmsp_fsai_create(None, None, 0, 4, None, C.byref(h)) == -1 and L.bmsp_last_error().decode().startswith("flags")
    assert L.bmsp_fsai_create(None, None, 0, 0, None, C.byref(h)) == -1 and "matrix A" in L.bmsp_last_error().decode()
    assert L.bmsp_fsai_apply(None, None, None, None) == -1 and L.bmsp_fsai_solve(None, 5, None, None, 0, 1e-6, 0, None, None, None) == -1
    assert L.bmsp_last_error().decode().startswith("method")
    assert L.bmsp_fsai_solve_gmres(None, 300, None, None, 0, 1e-6, 0, None, None, None) == -1 and L.bmsp_last_error().decode().startswith("restart")
    assert L.bmsp_fsai_free(None) == 0
    assert out.value == 0x5a5a and h.value == 0x5a5a


def build_cpp_fsai_check(out_path):
    lib_dir = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp_fsai_check.cpp"), "-o", out_path, "-L" + lib_dir, "-lbmsp",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_fsai_wrapper_compiles_and_links(bmsp, tmp_path):
    """include/bmSpMatrix.h with bmSparse_fsai and bmSpFsai instantiated for float and double links against libbmsp.so with a plain host
    compiler."""
    build_cpp_fsai_check(str(tmp_path / "cpp_fsai_check"))
