"""CPU tests of the surface of bmsp_matrix_ilu0 / bmsp_matrix_ilu0_values, and what tests/test_zz_ilu0.py shares with them: the matrices
and their values, and the reference (tests/ilu0_ref.c through ctypes: the fixed-point sweep and the sequential ILU(0) over CSR + CSC).  The
patterns are those of tests/test_spsv_api.py plus dense16 and dense17: two and three block-rows of full tiles, so that the cut at
K == min(I, J) lies on and off a tile edge.

Checked here without a GPU: the reference's sweeps reach the sequential factor's bits within 2n sweeps on every matrix and dtype with every
iterate finite (the condition the GPU cases rely on), and entry (i, j) is final after sweep 2 min(i, j) + 1 (+ 1 below the diagonal); the
reference's fp16 rounding against numpy's; the prototypes, the defines and the layout of bmsp_ilu0_info in bmsp.h; the refusals of the two
C entry points (scalars before handles, the argument named); the Python and C++ wrappers; the gfx950 assembly of ilu0.hip (every
instantiation, no scratch, subnormals kept, integer atomics in the kernels with statistics and only there, the full division sequence)."""
import ctypes as C
import functools
import inspect
import os
import re
import subprocess
import tempfile
import numpy as np
import pytest
from conftest import REPO
from test_spsv_api import MATRICES, SMALL, NP, VEC, pattern, assert_same_bits, _msg, _flat

BMSP_ERR_INVALID = -1
NO_CHECK = -1.0
NAMES = MATRICES + SMALL + ("dense16", "dense17")


# ---------------------------------------------------------------------------------------------------------
# the matrices
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ilu_values(name, dtype, seed=11):
    """(n, r, c, v) of matrix `name`, sorted by (row, col), the values rounded to the dtype (as float64): off-diagonal magnitudes in
    [0.5, 2) with mixed signs; the diagonal +-(1 + the row's absolute off-diagonal sum)"""
    n, r, c = pattern(name)
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.5, 2.0, r.size) * rng.choice([-1.0, 1.0], r.size)
    v = v.astype(NP[dtype]).astype(np.float64)
    off = r != c
    s = np.bincount(r[off], weights=np.abs(v[off]), minlength=n)
    v[~off] = ((1.0 + s) * rng.choice([-1.0, 1.0], n))[r[~off]]
    v = v.astype(NP[dtype]).astype(np.float64)
    v.setflags(write=False)         # (shared through the cache)
    return n, r, c, v


# ---------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_lib():
    d = tempfile.mkdtemp(prefix="ilu0_ref_")
    so = os.path.join(d, "libilu0_ref.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(REPO, "tests", "ilu0_ref.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp, i64 = C.c_void_p, C.c_int64
    for fn, real in ((L.ilu0_ref_f32, C.c_float), (L.ilu0_ref_f64, C.c_double)):
        fn.argtypes = [i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, real, C.c_int, C.c_int, vp, vp, vp, vp, vp]
        fn.restype = i64
    for fn in (L.ilu0_seq_f32, L.ilu0_seq_f64):
        fn.argtypes = [i64, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int]
        fn.restype = None
    L.ilu0_ref_f32_to_f16.argtypes = [C.c_float]
    L.ilu0_ref_f32_to_f16.restype = C.c_uint16
    L.ilu0_ref_f16_to_f32.argtypes = [C.c_uint16]
    L.ilu0_ref_f16_to_f32.restype = C.c_float
    return L


class Csr:
    """the pattern (n, r, c), sorted by (row, col), as the arrays ilu0_ref.c takes"""

    def __init__(self, n, r, c):
        r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
        assert np.all(np.diff(r * max(n, 1) + c) > 0)
        self.n = n
        self.rowptr = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(r, minlength=n), out=self.rowptr[1:])
        self.col = np.ascontiguousarray(c, np.int32)
        order = np.lexsort((r, c))
        self.colptr = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(c, minlength=n), out=self.colptr[1:])
        self.rowidx = np.ascontiguousarray(r[order], np.int32)
        self.csc2csr = np.ascontiguousarray(order, np.int64)
        self.dpos = np.full(n, -1, np.int64)
        on = np.flatnonzero(r == c)
        self.dpos[r[on]] = on
        assert (self.dpos >= 0).all(), "the reference needs every diagonal entry"

    def args(self):
        return [self.n] + [a.ctypes.data for a in (self.rowptr, self.col, self.colptr, self.rowidx, self.csc2csr, self.dpos)]


@functools.lru_cache(maxsize=None)
def csr_of(name):
    return Csr(*pattern(name))


def ref_sweeps(S, v, dtype, max_iter, tol, f0=None):
    """at most max_iter sweeps by the C helper on pattern S with A's values v, from f0 (default: v); tol = NO_CHECK runs them all.
    Returns (f, sweeps, converged, delta, fmax, changed, nonfinite), f and the per-sweep arrays (cut to `sweeps`) in the arithmetic type."""
    R = VEC[dtype]
    a = np.ascontiguousarray(np.asarray(v, NP[dtype]).astype(R))
    f = a.copy() if f0 is None else np.ascontiguousarray(np.asarray(f0, NP[dtype]).astype(R))
    tmp = np.zeros_like(a)
    m = int(max_iter)
    changed, nonfinite = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.int32)
    delta, fmax = np.zeros(max(m, 1), R), np.zeros(max(m, 1), R)
    conv = C.c_int32(0)
    fn = ref_lib().ilu0_ref_f64 if dtype == 2 else ref_lib().ilu0_ref_f32
    check = tol != NO_CHECK
    sweeps = fn(*S.args(), a.ctypes.data, f.ctypes.data, tmp.ctypes.data, m, R(tol if check else 0.0), int(check), int(dtype == 1),
                changed.ctypes.data, delta.ctypes.data, fmax.ctypes.data, nonfinite.ctypes.data, C.addressof(conv))
    k = int(sweeps)
    return f, k, int(conv.value), delta[:k].copy(), fmax[:k].copy(), changed[:k].copy(), nonfinite[:k].copy()


def ref_sequential(S, v, dtype):
    """the sequential ILU(0): row by row, columns ascending, in place"""
    R = VEC[dtype]
    a = np.ascontiguousarray(np.asarray(v, NP[dtype]).astype(R))
    f = np.zeros_like(a)
    fn = ref_lib().ilu0_seq_f64 if dtype == 2 else ref_lib().ilu0_seq_f32
    fn(*S.args(), a.ctypes.data, f.ctypes.data, int(dtype == 1))
    return f


@functools.lru_cache(maxsize=None)
def fixed_point(name, dtype):
    """(the sequential factor, the reference's run to it with tol = 0): computed once, shared by the tests; nobody writes into them"""
    n, r, c, v = ilu_values(name, dtype)
    S = csr_of(name)
    seq = ref_sequential(S, v, dtype)
    run = ref_sweeps(S, v, dtype, 2 * n, 0.0)
    for a in (seq,) + tuple(x for x in run if isinstance(x, np.ndarray)):
        a.setflags(write=False)
    return seq, run


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_reference_sweeps_reach_the_sequential_bits_within_2n_sweeps(name, dtype):
    n, r, c, v = ilu_values(name, dtype)
    S = csr_of(name)
    seq, (f, sweeps, conv, delta, fmax, changed, nonfinite) = fixed_point(name, dtype)
    assert np.isfinite(seq).all()
    assert conv == 1 and 1 <= sweeps <= 2 * n and changed[-1] == 0 and delta[-1] == 0, (sweeps, n)
    assert not nonfinite.any() and np.isfinite(fmax).all()           # every iterate is finite
    assert_same_bits(f, seq, name)
    # the sequential factor is a fixed point: one sweep from it changes nothing
    g, sw, cv, *_ = ref_sweeps(S, v, dtype, 5, 0.0, f0=seq)
    assert (sw, cv) == (1, 1)
    assert_same_bits(g, seq)
    # finite termination entry by entry: (i, j) is final after sweep 2 min(i, j) + 1, + 1 below the diagonal
    for m in (1, 2, 3, 6):
        g, sw, *_ = ref_sweeps(S, v, dtype, m, NO_CHECK)
        assert sw == m
        due = 2 * np.minimum(r, c) + 1 + (r > c) <= m
        assert_same_bits(g[due], seq[due], "%s after %d sweeps" % (name, m))


def test_dense_patterns_put_the_cut_on_and_off_a_tile_edge():
    assert pattern("dense16")[0] == 16 and pattern("dense17")[0] == 17
    for name, blocks in (("dense16", 2), ("dense17", 3)):
        n, r, c = pattern(name)
        assert r.size == n * n and (n + 7) // 8 == blocks


def test_fp16_rounding_routine_matches_numpy():
    L = ref_lib()
    rng = np.random.default_rng(3)
    x = np.concatenate([
        rng.uniform(-70000.0, 70000.0, 4000), rng.uniform(-2.0, 2.0, 4000), rng.uniform(-1e-4, 1e-4, 4000),      # normals, overflow
        rng.uniform(-2.0 ** -14, 2.0 ** -14, 4000), rng.uniform(-2.0 ** -24, 2.0 ** -24, 2000),                   # subnormals, underflow
        [0.0, -0.0, 65504.0, 65519.9, 65520.0, 65536.0, -65520.0, 1e30, -1e30, np.inf, -np.inf, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001,
         3 * 2.0 ** -25, 2.0 ** -26, 1e-45, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25],
    ]).astype(np.float32)
    # ties: halfway between two neighbouring halves, normal and subnormal, both parities
    h = np.arange(0, 0x7bff, 37, dtype=np.uint16)
    lo, hi = h.view(np.float16).astype(np.float64), (h + 1).astype(np.uint16).view(np.float16).astype(np.float64)
    ties = ((lo + hi) / 2).astype(np.float32)
    assert np.array_equal(ties.astype(np.float64), (lo + hi) / 2)     # (exact in fp32)
    x = np.concatenate([x, ties, -ties, np.nextafter(ties, np.float32(np.inf)), np.nextafter(ties, np.float32(-np.inf))])
    with np.errstate(over="ignore"):
        want = x.astype(np.float16)
    got = np.array([L.ilu0_ref_f32_to_f16(float(a)) for a in x], np.uint16)
    assert np.array_equal(got, want.view(np.uint16)), np.flatnonzero(got != want.view(np.uint16))[:8]
    back = np.array([L.ilu0_ref_f16_to_f32(int(b)) for b in got], np.float32)
    assert np.array_equal(back.view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert np.isnan(np.uint16(L.ilu0_ref_f32_to_f16(float("nan"))).view(np.float16))
    assert np.isnan(L.ilu0_ref_f16_to_f32(0x7e00))


# ---------------------------------------------------------------------------------------------------------
# the entry points
# ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_interface_verbatim(bmsp):
    hdr = _flat(open(os.path.join(REPO, "include", "bmsp.h")).read())
    for line in ("#define BMSP_ILU_F0_GIVEN 1", "#define BMSP_ILU_NO_CHECK (-1.0)",
                 "typedef struct { char kernel[64]; int lanes; int64_t sweeps, max_sweeps; int converged; double delta, fmax; "
                 "int64_t view_bytes; } bmsp_ilu0_info;",
                 "int bmsp_matrix_ilu0(bmsp_matrix_t A, int64_t max_iter, double tol, int out_transposed, void *stream, "
                 "bmsp_matrix_t *F, double *delta_history, bmsp_ilu0_info *info);",
                 "int bmsp_matrix_ilu0_values(bmsp_matrix_t A, bmsp_matrix_t F, int64_t max_iter, double tol, int flags, void *stream, "
                 "double *delta_history, bmsp_ilu0_info *info);"):
        assert _flat(line) in hdr, line
    for phrase in ("s = fma(-f^k_ik, f^k_kj, s)", "never a reciprocal", "after sweep 2m + 1 when i <= j and after sweep 2m + 2",
                   "!changed || (tol > 0 && delta <= fl(tol * fmax))", "BMSP_ILU0_CHECK", "BMSP_ILU0_LANES", "max_iter == 0 means 2n",
                   "must not overlap on different streams", "one lane group's serial chain", "F == A is refused"):
        assert _flat(phrase) in hdr, phrase
    for name in ("bmsp_matrix_ilu0", "bmsp_matrix_ilu0_values"):
        assert name in bmsp.SYMBOLS and hasattr(bmsp.lib(), name)


def test_info_layout_and_wrappers(bmsp):
    I = bmsp.Ilu0Info
    assert [f[0] for f in I._fields_] == ["kernel", "lanes", "sweeps", "max_sweeps", "converged", "delta", "fmax", "view_bytes"]
    assert C.sizeof(I) == 120
    assert (I.lanes.offset, I.sweeps.offset, I.max_sweeps.offset, I.converged.offset, I.delta.offset, I.fmax.offset, I.view_bytes.offset) == \
        (64, 72, 80, 88, 96, 104, 112)
    assert set(I().as_dict()) == {f[0] for f in I._fields_}
    assert (bmsp.ILU_F0_GIVEN, bmsp.ILU_NO_CHECK) == (1, -1.0)
    assert list(inspect.signature(bmsp.ilu0).parameters) == ["A", "max_iter", "tol", "out_transposed", "history", "stream"]
    d = {k: p.default for k, p in inspect.signature(bmsp.ilu0).parameters.items()}
    assert (d["max_iter"], d["tol"], d["out_transposed"], d["history"], d["stream"]) == (0, 0.0, None, False, None)
    pv = inspect.signature(bmsp.ilu0_values).parameters
    assert list(pv)[:2] == ["A", "F"] and pv["f0_given"].default is False and pv["max_iter"].default == 0 and pv["tol"].default == 0.0
    assert list(inspect.signature(bmsp.BmSpMatrix.ilu0).parameters)[1:] == list(inspect.signature(bmsp.ilu0).parameters)[1:]


def test_scalars_are_refused_before_handles_and_named(bmsp):
    L = bmsp.lib()
    hist = (C.c_double * 4)()
    info = bmsp.Ilu0Info()
    out = C.c_void_p()

    def make(max_iter=0, tol=0.0, lay=0, h=None, A=None, F=C.byref(out)):
        return L.bmsp_matrix_ilu0(A, max_iter, tol, lay, None, F, h, C.byref(info))

    def into(max_iter=0, tol=0.0, flags=0, h=None, A=None, F=None):
        return L.bmsp_matrix_ilu0_values(A, F, max_iter, tol, flags, None, h, C.byref(info))

    # every scalar is named although the handles are null too
    for kw, word in ((dict(max_iter=-1, tol=-2.0), "max_iter"), (dict(max_iter=(1 << 20) + 1), "max_iter"), (dict(tol=float("nan"), lay=2), "tol"),
                     (dict(tol=-0.5), "tol"), (dict(tol=-2.0), "tol"), (dict(tol=NO_CHECK, h=hist, lay=3), "delta_history"),
                     (dict(lay=2), "out_transposed"), (dict(lay=-1, tol=NO_CHECK), "out_transposed")):
        assert make(**kw) == BMSP_ERR_INVALID, kw
        assert _msg(bmsp).startswith(word), (kw, _msg(bmsp))
    for kw, word in ((dict(max_iter=-1, flags=2), "max_iter"), (dict(max_iter=(1 << 20) + 1), "max_iter"), (dict(tol=float("nan"), flags=2), "tol"),
                     (dict(tol=-0.5), "tol"), (dict(tol=NO_CHECK, h=hist, flags=4), "delta_history"), (dict(flags=2), "flags"),
                     (dict(flags=-1, tol=NO_CHECK), "flags")):
        assert into(**kw) == BMSP_ERR_INVALID, kw
        assert _msg(bmsp).startswith(word), (kw, _msg(bmsp))
    # good scalars (the largest max_iter, NO_CHECK without a history, the flag, a history with a check): the handle is named
    assert make(max_iter=1 << 20, tol=NO_CHECK, lay=1) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)
    assert make(h=hist) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)
    assert into(max_iter=1 << 20, tol=NO_CHECK, flags=1) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)
    assert into(tol=2.0 ** -10, h=hist) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)
    assert out.value is None


def build_cpp_ilu0_check(out_path):
    lib_dir = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp_ilu0_check.cpp"), "-o", out_path, "-L" + lib_dir, "-lbmsp",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_ilu0_wrappers_compile_and_link(bmsp, tmp_path):
    """include/bmSpMatrix.h with bmSparse_ILU0 / bmSparse_ILU0_values instantiated for float, half and double links against libbmsp.so
    with a plain host compiler."""
    build_cpp_ilu0_check(str(tmp_path / "cpp_ilu0_check"))


# ---------------------------------------------------------------------------------------------------------
# the kernels in the assembly
# ---------------------------------------------------------------------------------------------------------
INT_ATOMIC = re.compile(r"\s*(global|flat)_atomic_(u?max|or)_(x2|u64|b64)\b")
ANY_ATOMIC = re.compile(r"\s*\w*atomic\w*|\s*ds_(add|sub|min|max|inc|dec|cmpst|wrxchg)", re.I)
FLOAT_ATOMIC = re.compile(r"\s*\w*atomic\w*_(f16|f32|f64|pk_\w+)\b", re.I)
FRAG = "17ilu0_sweep_kernel"


@pytest.fixture(scope="module")
def ilu0_asm(tmp_path_factory):
    from test_fold_handoff_asm import to_asm, functions
    path = to_asm("ilu0", str(tmp_path_factory.mktemp("ilu0_asm")))
    return functions(path), open(path).read()


def test_every_instantiation_is_in_the_assembly(ilu0_asm):
    fns, _ = ilu0_asm
    ks = {n: b for n, b in fns.items() if FRAG in n}
    assert len(ks) == 12, sorted(ks)
    for s in "ftd":
        for g in (1, 8):
            for stats in (0, 1):
                assert sum(FRAG + "I%sLi%dELb%dEE" % (s, g, stats) in n for n in ks) == 1, (s, g, stats)


def test_kernels_use_no_scratch_keep_subnormals_and_only_integer_atomics(ilu0_asm):
    fns, text = ilu0_asm
    n = 0
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        if "ilu0_sweep" not in m.group(1):
            continue
        n += 1
        body = m.group(2)
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), m.group(1)
        assert re.search(r"\.amdhsa_float_denorm_mode_32 3\b", body) and re.search(r"\.amdhsa_float_denorm_mode_16_64 3\b", body), m.group(1)
    assert n == 12
    for name, body in fns.items():
        if FRAG not in name:
            continue
        assert not any(re.match(r"\s*scratch_", ln) for ln in body), name
        atomics = [ln for ln in body if ANY_ATOMIC.match(ln)]
        assert not [ln for ln in atomics if FLOAT_ATOMIC.match(ln)], (name, atomics[:3])
        if re.search(r"Li[18]ELb1EE", name):                # <.., STATS = true>
            assert atomics and all(INT_ATOMIC.match(ln) for ln in atomics), (name, atomics[:4])
        else:
            assert not atomics, (name, atomics[:3])         # the preconditioner mode: launches only


def test_division_sequence_and_fused_multiply_adds(ilu0_asm):
    """one fused multiply-add per product; the strict lower triangle ends with the full IEEE division sequence, and a reciprocal only
    ever seeds one"""
    fns, _ = ilu0_asm
    fma = re.compile(r"\s*v_(fma|fmac)_(f32|f64)")
    for name, body in fns.items():
        if FRAG not in name:
            continue
        assert any(fma.match(ln) for ln in body), name
        ops = [ln.split()[0] for ln in body if ln.strip()]
        fixup = sum(o.startswith("v_div_fixup") for o in ops)
        assert fixup >= 1 and sum(o.startswith("v_div_fmas") for o in ops) == fixup and sum(o.startswith("v_rcp") for o in ops) == fixup, name
        assert sum(o.startswith("v_div_scale") for o in ops) == 2 * fixup, name
