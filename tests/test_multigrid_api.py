"""CPU tests of the surface of bmsp_mg_create / _free / _info / _vcycle / _solve, and what tests/test_zzzzzzzzzz_multigrid.py shares with
them: the hierarchies, the C reference of the cycle (tests/multigrid_ref.c through ctypes: include/bmsp.h's arithmetic restated with fmaf /
fma, gcc -O2 -ffp-contract=off) and its self-checks.

The hierarchies are built in numpy from test_aggregate_api.pattern(name): off-diagonal values -(0.5 + h(i, j) / 2) with h a hash of the
unordered pair in [0, 1) (symmetric wherever the pattern is), the diagonal 1 + 1.1 * the row's absolute off-diagonal sum (strictly
dominant), rounded to the dtype.  No aggregation and no SpGEMM is involved: coarse operators are P^T A P formed by scipy in float64 and
rounded, inverses are numpy's of the rounded operator.  A failure therefore points at the cycle.
    j:<pattern>      one level, no inverse: Jacobi steps only.  one, diag7, path203 (ragged n), dense24 (full tiles), intile, star530 (a
                     530-entry row: the long walk), rand1000, and path203_nodiag (row 5 stores no diagonal: d = +0, Inf / NaN rows)
    d:<n>            one level with its inverse, n = 1, 7, 24 (ld_inv = 29 > n), 203
    two              grid13x11 (n = 143), P piecewise constant over i // 3 with weights, R = P^T, A1 = P^T A0 P, exact inverse
    three            rand1000s (rand1000's pattern made symmetric, so that CG applies), two entries per row of P on both levels, the last
                     level without an inverse
    star             star530, P over i // 3 plus a column 0 that every row reaches: row 0 of R = P^T holds 530 entries (the hub row in R)
    nonsym           rand1000 as it is (not symmetric), two levels, R = P^T, exact inverse: what BiCGStab + cycle is solved on
    fat              path203, P piecewise constant over i // 26 (8 columns): R = P^T is one block-row of 26 tiles, beyond the 24 tiles
                     per block-row up to which the default restriction takes the row kernel
    empty            n = 0

Self-checks here: the float entry against the all-double entry and against a permuted summation order (printed; sanity bounds written
down in the test); for `two` the iteration matrix I - M^-1 A0 of the reference in double has spectral radius < 1; test_krylov_api.restate
with the reference cycle as its preconditioner converges on every (case, method, dtype) of SOLVES -- the list the GPU file solves bit
for bit.  Also: the header declares the interface verbatim, struct layouts, scalar refusals before handles and by name, the C++ wrapper
compiles and links."""
import ctypes as C
import functools
import inspect
import os
import subprocess
import tempfile
import numpy as np
import pytest
from conftest import REPO
from test_spsv_api import VEC, NP, _msg, _flat
from test_aggregate_api import pattern
from test_krylov_api import restate, cdot, CONVERGED, NO_CHECK

BMSP_ERR_INVALID = -1
JACOBI = ("one", "diag7", "path203", "dense24", "intile", "star530", "rand1000", "path203_nodiag")
DENSE = (1, 7, 24, 203)
MULTI = ("two", "three", "star", "nonsym", "fat")
CASES = tuple("j:" + p for p in JACOBI) + tuple("d:%d" % n for n in DENSE) + MULTI + ("empty",)
PREPOST = ((1, 0), (1, 1), (2, 3))
OMEGA = 2.0 / 3.0
TOL = {0: 1e-5, 2: 1e-10}
# (case, method) the GPU file solves bit for bit, F32 and F64 each: CG needs a symmetric A and a symmetric cycle (R = P^T, pre == post)
SOLVES = (("two", "cg"), ("two", "bicgstab"), ("three", "cg"), ("three", "bicgstab"), ("nonsym", "bicgstab"))


# ---------------------------------------------------------------------------------------------------------
# the hierarchies
# ---------------------------------------------------------------------------------------------------------
def coo_sorted(shape, r, c, v):
    r, c, v = np.asarray(r, np.int64), np.asarray(c, np.int64), np.asarray(v, np.float64)
    o = np.lexsort((c, r))
    return (int(shape[0]), int(shape[1]), r[o], c[o], v[o])


def dominant(name, dtype):
    """the level-0 operator of pattern `name`: (n, n, r, c, v) sorted by (row, col), v float64 holding values of the dtype"""
    drop = None
    if name == "path203_nodiag":
        name, drop = "path203", 5
    n, r, c = pattern("rand1000" if name == "rand1000s" else name)
    if name == "rand1000s":
        key = np.unique(np.concatenate([r * n + c, c * n + r]))
        r, c = key // n, key % n
    key = np.unique(np.concatenate([r * max(n, 1) + c, np.arange(n) * (max(n, 1) + 1)]))      # every diagonal entry stored
    r, c = key // max(n, 1), key % max(n, 1)
    lo, hi = np.minimum(r, c), np.maximum(r, c)
    v = -(0.5 + ((lo * 7919 + hi * 104729) % 1000) / 2000.0)
    off = r != c
    rowsum = np.bincount(r[off], weights=np.abs(v[off]), minlength=n)
    v[~off] = 1.0 + 1.1 * rowsum[r[~off]]
    if drop is not None:
        keep = ~((r == drop) & (c == drop))
        r, c, v = r[keep], c[keep], v[keep]
    return coo_sorted((n, n), r, c, v.astype(NP[dtype]).astype(np.float64))


def _sp(m):
    import scipy.sparse as sp
    return sp.csr_matrix((m[4], (m[2], m[3])), shape=(m[0], m[1]))


def _coo_of(S, dtype):
    S = S.tocoo()
    return coo_sorted(S.shape, S.row, S.col, np.asarray(S.data, np.float64).astype(NP[dtype]).astype(np.float64))


def transpose(m):
    return coo_sorted((m[1], m[0]), m[3], m[2], m[4])


def prolongator(n, nc, dtype, second=None, hub=False):
    """piecewise constant over i // ceil(n / nc) with weights 0.5 + (i % 5) / 8; second: one more entry per row, in the next column (cyclic),
    weight 0.25; hub: one more entry (i, 0) of weight 2^-6 for the rows outside aggregate 0"""
    i = np.arange(n)
    per = -(-n // nc)
    r, c, v = [i], [i // per], [0.5 + (i % 5) / 8.0]
    if second:
        r.append(i)
        c.append((i // per + 1) % nc)
        v.append(np.full(n, 0.25))
    if hub:
        far = i[i // per != 0]
        r.append(far)
        c.append(np.zeros(far.size, np.int64))
        v.append(np.full(far.size, 2.0 ** -6))
    return coo_sorted((n, nc), np.concatenate(r), np.concatenate(c), np.concatenate(v).astype(NP[dtype]).astype(np.float64))


def _freeze(h):
    for group in (h["A"], h["P"], h["R"]):
        for m in group:
            for a in m[2:]:
                a.setflags(write=False)
    if h["inv"] is not None:
        h["inv"].setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def hierarchy(case, dtype):
    """{"A": [...], "P": [...], "R": [... = P^T], "inv": the dense inverse of A[-1] as an array of the vector type with ld columns or None,
    "ld": its leading dimension}; every operator (rows, cols, r, c, v) sorted by (row, col).  Shared, never written."""
    R = VEC[dtype]
    if case.startswith("j:") or case == "empty":
        return _freeze({"A": [dominant(case[2:] if case != "empty" else "empty", dtype)], "P": [], "R": [], "inv": None, "ld": 0})
    if case.startswith("d:"):
        n = int(case[2:])
        A = dominant({1: "one", 7: "diag7", 24: "dense24", 203: "path203"}[n], dtype)
        ld = 29 if n == 24 else n
        inv = np.zeros((n, ld), R)
        inv[:, :n] = np.linalg.inv(_sp(A).toarray()).astype(R)
        inv[:, n:] = np.nan                                  # (the padding is never read)
        return _freeze({"A": [A], "P": [], "R": [], "inv": inv, "ld": ld})
    name, sizes, second, hub, exact = {"two": ("grid13x11", (48,), False, False, True), "three": ("rand1000s", (250, 63), True, False, False),
                                       "star": ("star530", (177,), False, True, True), "nonsym": ("rand1000", (250,), True, False, True), "fat": ("path203", (8,), False, False, True)}[case]
    As, Ps = [dominant(name, dtype)], []
    for nc in sizes:
        P = prolongator(As[-1][0], nc, dtype, second, hub)
        Ps.append(P)
        As.append(_coo_of(_sp(P).T @ _sp(As[-1]) @ _sp(P), dtype))
    inv = np.ascontiguousarray(np.linalg.inv(_sp(As[-1]).toarray()).astype(R)) if exact else None
    return _freeze({"A": As, "P": Ps, "R": [transpose(P) for P in Ps], "inv": inv, "ld": As[-1][0]})


@functools.lru_cache(maxsize=None)
def rhs(case, dtype):
    n = hierarchy(case, dtype)["A"][0][0]
    rng = np.random.default_rng(n + 29)
    b = (rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(VEC[dtype])
    b.setflags(write=False)
    return b


# ---------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_lib():
    d = tempfile.mkdtemp(prefix="multigrid_ref_")
    so = os.path.join(d, "libmultigrid_ref.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(REPO, "tests", "multigrid_ref.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp = C.c_void_p
    for fn in (L.mg_vcycle_ref_f32, L.mg_vcycle_ref_f64, L.mg_vcycle_ref_wide):
        fn.argtypes = [C.c_int, vp] + [vp] * 9 + [vp, C.c_int64, C.c_double, C.c_int, C.c_int, vp, vp]
        fn.restype = None
    return L


def _csr(m, S, reverse):
    rows, _, r, c, v = m
    ptr = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=rows), out=ptr[1:])
    c, v = np.ascontiguousarray(c), np.ascontiguousarray(v.astype(S))
    if reverse:                                  # every row's entries in descending column order: another summation order
        o = np.lexsort((-c, r))
        c, v = np.ascontiguousarray(c[o]), np.ascontiguousarray(v[o])
    return ptr, c, v


def ref_cycle(case, dtype, r, pre=1, post=1, omega=OMEGA, wide=False, reverse=False):
    """one cycle of the hierarchy for right-hand side r by tests/multigrid_ref.c: the bits of row mode (wide: float operands, all in
    double, returned as float64; dtype 2 has no wide form).  reverse: the same chains walked in descending column order."""
    h = hierarchy(case, dtype)
    S = VEC[dtype]
    W = np.float64 if wide else S
    fn = ref_lib().mg_vcycle_ref_f64 if dtype == 2 else (ref_lib().mg_vcycle_ref_wide if wide else ref_lib().mg_vcycle_ref_f32)
    assert not (wide and dtype == 2)
    levels = len(h["A"])
    n = np.array([A[0] for A in h["A"]], np.int64)
    keep, tables = [], []
    for group in (h["A"], h["P"], h["R"]):
        csr = [_csr(m, S, reverse) for m in group]
        keep.append(csr)
        for k in range(3):
            tables.append((C.c_void_p * max(len(csr), 1))(*[t[k].ctypes.data for t in csr]))
    inv = None if h["inv"] is None else np.ascontiguousarray(h["inv"])
    r = np.ascontiguousarray(r, S)
    z = np.zeros(int(n[0]), W)
    fn(levels, n.ctypes.data, *[C.cast(t, C.c_void_p) for t in tables], None if inv is None else inv.ctypes.data, h["ld"], omega, pre, post,
       r.ctypes.data, z.ctypes.data)
    del keep
    return z


def cpu_solve(case, method, dtype, max_iter=200, tol=None, x0=None):
    """test_krylov_api.restate with a scipy product of the vector type, the C dot and the reference cycle"""
    h = hierarchy(case, dtype)
    A = _sp(h["A"][0]).astype(VEC[dtype]).tocsr()
    matvec = lambda x: (A @ x).astype(VEC[dtype])
    return restate(method, matvec, lambda r: ref_cycle(case, dtype, r), cdot, rhs(case, dtype), x0, max_iter, TOL[dtype] if tol is None else tol)


# ---------------------------------------------------------------------------------------------------------
# self-checks
# ---------------------------------------------------------------------------------------------------------
def test_the_inputs_are_what_they_are_named_for():
    for case in CASES:
        for dtype in (0, 2):
            h = hierarchy(case, dtype)
            for l, A in enumerate(h["A"]):
                assert A[0] == A[1]
                if l + 1 < len(h["A"]):
                    assert (h["P"][l][0], h["P"][l][1]) == (A[0], h["A"][l + 1][0]) and (h["R"][l][0], h["R"][l][1]) == (h["A"][l + 1][0], A[0])
    assert hierarchy("j:path203", 0)["A"][0][0] % 8 != 0 and hierarchy("empty", 0)["A"][0][0] == 0
    A = hierarchy("j:dense24", 0)["A"][0]
    assert A[2].size == 24 * 24
    A = hierarchy("j:star530", 0)["A"][0]
    assert np.bincount(A[2]).max() == 530
    A = hierarchy("j:path203_nodiag", 0)["A"][0]
    assert not ((A[2] == 5) & (A[3] == 5)).any() and ((A[2] == 6) & (A[3] == 6)).any()
    Rm = hierarchy("star", 0)["R"][0]
    assert np.bincount(Rm[2])[0] == 530                       # the hub row is in R
    assert [A[0] for A in hierarchy("three", 0)["A"]] == [1000, 250, 63] and hierarchy("three", 0)["inv"] is None
    assert np.bincount(hierarchy("three", 0)["P"][0][2]).min() == 2
    for case, sym in (("two", True), ("three", True), ("nonsym", False)):
        S = _sp(hierarchy(case, 2)["A"][0])
        assert (abs(S - S.T).nnz == 0) == sym, case
    assert hierarchy("d:24", 0)["ld"] == 29 and hierarchy("d:24", 0)["inv"].shape == (24, 29)


@pytest.mark.parametrize("case", [c for c in CASES if c not in ("empty", "j:path203_nodiag")])
def test_float_entry_against_the_all_double_entry(case):
    """A sanity check, printed: e_row = ||z(float) - z(all double)||inf is float rounding through chains of at most 530 terms of a
    strictly dominant operator, so it stays below 530 * 2^-24 * 8 (the factor 8: levels and steps) relative to ||z||inf; the all-double
    entry under a reversed summation order moves by double rounding only, below 530 * 2^-53 * 8 in the same measure."""
    for pre, post in PREPOST if not case.startswith("d:") else ((1, 1),):
        r = rhs(case, 0)
        z32 = ref_cycle(case, 0, r, pre, post)
        zw = ref_cycle(case, 0, r, pre, post, wide=True)
        zp = ref_cycle(case, 0, r, pre, post, wide=True, reverse=True)
        scale = np.abs(zw).max()
        e_row, e_perm = np.abs(z32.astype(np.float64) - zw).max(), np.abs(zp - zw).max()
        print("%-12s pre %d post %d  |z| %.3e  float vs all-double %.3e  all-double reversed order %.3e" % (case, pre, post, scale, e_row, e_perm))
        assert np.isfinite(zw).all() and scale > 0
        assert e_row <= 530 * 2.0 ** -24 * 8 * scale and e_perm <= 530 * 2.0 ** -53 * 8 * scale


def test_missing_diagonal_gives_inf_and_nan_not_an_error():
    with np.errstate(all="ignore"):
        z = ref_cycle("j:path203_nodiag", 0, rhs("j:path203_nodiag", 0), 2, 3)
    assert not np.isfinite(z[5]) and not np.isfinite(z).all() and np.isfinite(z[100:]).all()
    assert ref_cycle("empty", 0, rhs("empty", 0)).size == 0


def test_two_level_iteration_matrix_contracts():
    """I - M^-1 A0 column by column from the double reference: spectral radius < 1 (the cycle is a convergent iteration on its own)"""
    h = hierarchy("two", 2)
    A = _sp(h["A"][0]).toarray()
    n = A.shape[0]
    M = np.stack([ref_cycle("two", 2, A[:, j].copy()) for j in range(n)], axis=1)            # M^-1 A
    rho = np.abs(np.linalg.eigvals(np.eye(n) - M)).max()
    print("spectral radius of I - M^-1 A on `two`: %.4f" % rho)
    assert rho < 1.0


@pytest.mark.parametrize("case,method", SOLVES)
@pytest.mark.parametrize("dtype", [0, 2])
def test_restatement_with_the_reference_cycle_converges(case, method, dtype):
    x, its, status, hist, bb = cpu_solve(case, method, dtype)
    h = hierarchy(case, dtype)
    res = np.linalg.norm(rhs(case, dtype).astype(np.float64) - _sp(h["A"][0]) @ x.astype(np.float64)) / np.sqrt(bb)
    plain = restate(method, lambda v: (_sp(h["A"][0]).astype(VEC[dtype]) @ v).astype(VEC[dtype]), None, cdot, rhs(case, dtype), None, 400, TOL[dtype])
    print("%-7s %-8s %s  cycle %3d iterations (none: %3d)  true residual %.3e" % (case, method, "F64" if dtype else "F32", its, plain[1], res))
    assert status == CONVERGED and 1 <= its < plain[1], (status, its, plain[1])
    assert res <= 2 * TOL[dtype]


# ---------------------------------------------------------------------------------------------------------
# the entry points
# ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_interface_verbatim(bmsp):
    hdr = _flat(open(os.path.join(REPO, "include", "bmsp.h")).read())
    for line in (
            "typedef struct bmsp_mg_s *bmsp_mg_t;",
            "int bmsp_mg_create(int levels, const bmsp_matrix_t *A /* levels */, const bmsp_matrix_t *P /* levels-1 */, "
            "const bmsp_matrix_t *R /* levels-1; NULL or NULL entries: restrict by P^T */, "
            "const void *d_coarse_inv /* n_c x n_c row-major, vector type; may be NULL */, int64_t ld_inv, "
            "double omega, int pre, int post, void *stream, bmsp_mg_t *out);",
            "int bmsp_mg_free(bmsp_mg_t mg);", "int bmsp_mg_info(bmsp_mg_t mg, bmsp_mg_info_t *info);",
            "int bmsp_mg_vcycle(bmsp_mg_t mg, const void *d_r, void *d_z, void *stream);",
            "int bmsp_mg_solve(bmsp_mg_t mg, int method, const void *d_b, void *d_x, int64_t max_iter, double tol, int flags, "
            "double *relres_history, bmsp_krylov_info *info, void *stream);",
            "#define BMSP_MG_MAX_LEVELS 16", "#define BMSP_MG_RESTRICT_ROW 0", "#define BMSP_MG_RESTRICT_SPMV 1", "#define BMSP_MG_RESTRICT_PT 2",
            "typedef struct { int levels, pre, post, coarse_exact; int64_t n[BMSP_MG_MAX_LEVELS]; int restrict_mode[BMSP_MG_MAX_LEVELS]; "
            "char kernel[64], coarse_kernel[64]; int64_t workspace_bytes, launches_per_cycle; } bmsp_mg_info_t;"):
        assert _flat(line) in hdr, line
    for phrase in ("s = fma(+-m_ij, v_j, s)", "x'_i = fl(x_i + fl(wR * fl(s_i / d_i)))", "x_i = fl(wR * fl(r_i / d_i))", "rc = rowchain(R, +0, +, t)",
                   "x_i = rowchain(P, x, +, e)", "s = fma(inv_ij, r_j, s)", "BMSP_MG_RESTRICT=row|spmv", "no atomic, no flag, no spin and no LDS",
                   "CG needs a symmetric cycle", "tests/multigrid_ref.c", "One stream per handle at a time", "\"cg+mg\" or \"bicgstab+mg\""):
        assert _flat(phrase) in hdr, phrase
    for name in ("bmsp_mg_create", "bmsp_mg_free", "bmsp_mg_info", "bmsp_mg_vcycle", "bmsp_mg_solve"):
        assert name in bmsp.SYMBOLS and hasattr(bmsp.lib(), name)
    # the Krylov interface is as it was: kind 4 is still nobody's
    assert "typedef struct { int kind; bmsp_matrix_t F; int64_t sweeps; } bmsp_precond;" in hdr and "#define BMSP_PC_ILU_SWEEPS 3" in hdr


def test_struct_layout_and_wrappers(bmsp):
    I = bmsp.MgInfo
    assert [f[0] for f in I._fields_] == ["levels", "pre", "post", "coarse_exact", "n", "restrict_mode", "kernel", "coarse_kernel",
                                          "workspace_bytes", "launches_per_cycle"]
    assert C.sizeof(I) == 16 + 128 + 64 + 128 + 16
    assert (I.n.offset, I.restrict_mode.offset, I.kernel.offset, I.coarse_kernel.offset, I.workspace_bytes.offset,
            I.launches_per_cycle.offset) == (16, 144, 208, 272, 336, 344)
    assert (bmsp.MG_MAX_LEVELS, bmsp.MG_RESTRICT_ROW, bmsp.MG_RESTRICT_SPMV, bmsp.MG_RESTRICT_PT) == (16, 0, 1, 2)
    sig = inspect.signature(bmsp.Multigrid.__init__).parameters
    assert list(sig)[1:8] == ["A", "P", "R", "coarse_inv", "omega", "pre", "post"]
    assert (sig["R"].default, sig["coarse_inv"].default, sig["omega"].default, sig["pre"].default, sig["post"].default) == (None, None, 2.0 / 3.0, 1, 1)
    assert list(inspect.signature(bmsp.Multigrid.vcycle).parameters) == ["self", "r", "z", "stream"]
    assert list(inspect.signature(bmsp.Multigrid.solve).parameters)[:3] == ["self", "b", "method"]
    assert inspect.signature(bmsp.Multigrid.solve).parameters["method"].default == "cg"
    from pybmsp import amg
    assert list(inspect.signature(amg.device_cycle).parameters) == ["levels", "omega", "pre", "post"]
    assert callable(amg.vcycle) and callable(amg.pcg)


def test_scalars_are_refused_before_handles_and_named(bmsp):
    L = bmsp.lib()
    out = C.c_void_p(0x5a5a)
    buf = (C.c_float * 16)()
    inv = C.addressof(buf)

    def create(levels=1, A=None, P=None, R=None, inv=None, ld=0, omega=OMEGA, pre=1, post=1, o=out):
        return L.bmsp_mg_create(levels, A, P, R, inv, ld, omega, pre, post, None, C.byref(o) if o is not None else None)

    for kw, word in ((dict(levels=0, omega=float("nan")), "levels"), (dict(levels=17), "levels"), (dict(levels=-1), "levels"),
                     (dict(omega=float("nan"), pre=-1), "omega"), (dict(omega=float("inf")), "omega"), (dict(pre=-1, post=17), "pre"),
                     (dict(pre=17), "pre"), (dict(post=-1), "post"), (dict(post=17), "post"), (dict(pre=0, post=0), "pre + post"),
                     (dict(levels=2, pre=0, post=0, inv=inv), "pre + post")):
        assert create(**kw) == BMSP_ERR_INVALID, kw
        assert _msg(bmsp).startswith(word), (kw, _msg(bmsp))
        assert out.value == 0x5a5a
    # good scalars: the pointers are named, in order
    assert create(o=None) == BMSP_ERR_INVALID and _msg(bmsp).startswith("out")
    assert create() == BMSP_ERR_INVALID and _msg(bmsp).startswith("A ")
    assert create(pre=0, post=0, inv=inv) == BMSP_ERR_INVALID and _msg(bmsp).startswith("A ")        # (one level with its inverse needs no step)
    nulls = (C.c_void_p * 2)(None, None)
    assert create(levels=2, A=nulls) == BMSP_ERR_INVALID and _msg(bmsp).startswith("P ")
    assert create(levels=2, A=nulls, P=nulls) == BMSP_ERR_INVALID and _msg(bmsp).startswith("A[0]")
    assert out.value == 0x5a5a
    info = bmsp.MgInfo()
    assert L.bmsp_mg_info(None, C.byref(info)) == BMSP_ERR_INVALID and _msg(bmsp).startswith("mg")
    assert L.bmsp_mg_vcycle(None, inv, inv, None) == BMSP_ERR_INVALID and _msg(bmsp).startswith("mg")
    assert L.bmsp_mg_free(None) == 0
    kinfo = bmsp.KrylovInfo()
    hist = (C.c_double * 4)()

    def solve(method=0, max_iter=0, tol=1e-6, flags=0, h=None):
        return L.bmsp_mg_solve(None, method, None, None, max_iter, tol, flags, h, C.byref(kinfo), None)

    for kw, word in ((dict(method=2, max_iter=-1), "method"), (dict(max_iter=-1, tol=float("nan")), "max_iter"), (dict(max_iter=(1 << 20) + 1), "max_iter"),
                     (dict(tol=float("nan"), flags=2), "tol"), (dict(tol=-0.5), "tol"), (dict(flags=2, tol=NO_CHECK, h=hist), "flags"),
                     (dict(tol=NO_CHECK, h=hist), "relres_history")):
        assert solve(**kw) == BMSP_ERR_INVALID, kw
        assert _msg(bmsp).startswith(word), (kw, _msg(bmsp))
    assert solve() == BMSP_ERR_INVALID and _msg(bmsp).startswith("mg")
    # bmsp_krylov_solve still refuses kind 4
    P = bmsp.Precond
    assert L.bmsp_krylov_solve(None, 0, 0, C.byref(P(4, None, 0)), None, None, 0, 1e-6, 0, None, None, None) == BMSP_ERR_INVALID
    assert _msg(bmsp).startswith("pc->kind")


def build_cpp_multigrid_check(out_path):
    lib_dir = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp_multigrid_check.cpp"), "-o", out_path, "-L" + lib_dir, "-lbmsp",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_multigrid_wrapper_compiles_and_links(bmsp, tmp_path):
    """include/bmSpMatrix.h with bmSpMultigrid instantiated for float and double links against libbmsp.so with a plain host compiler."""
    build_cpp_multigrid_check(str(tmp_path / "cpp_multigrid_check"))
