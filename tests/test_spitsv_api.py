"""CPU tests of the surface of bmsp_spitsv, and what tests/test_zz_spitsv.py shares with them: the reference (tests/spitsv_ref.c through
ctypes).  The matrices, their values and the helpers are those of tests/test_spsv_api.py.

Checked here without a GPU: the refusals of the C entry point (scalars before handles, the argument named, in order); the prototype, the
defines and the layout of bmsp_spitsv_info in bmsp.h; the Python and C++ wrappers; the reference against spsv_ref.c after `levels` sweeps
(finite termination, on the CPU); the gfx950 assembly of spitsv.hip (every instantiation, no scratch, subnormals kept, integer atomics in
the kernels with statistics and only there, no floating-point atomic anywhere)."""
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
from test_spsv_api import (MATRICES, SMALL, NP, VEC, pattern, values, rhs, reference, assert_same_bits, block_records, effective_lower,
                           _msg, _flat, _targs)

BMSP_ERR_INVALID = -1
NO_CHECK = -1.0
COMBOS = [(op, fill, unit) for op in "NT" for fill in ("lower", "upper") for unit in (False, True)]


# ---------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_lib():
    d = tempfile.mkdtemp(prefix="spitsv_ref_")
    so = os.path.join(d, "libspitsv_ref.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(REPO, "tests", "spitsv_ref.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp = C.c_void_p
    for fn, real in ((L.spitsv_ref_f32, C.c_float), (L.spitsv_ref_f64, C.c_double)):
        fn.argtypes = [C.c_int64, C.c_int, C.c_int, vp, vp, vp, vp, real, vp, vp, vp, C.c_int64, real, C.c_int, vp, vp, vp, vp]
        fn.restype = C.c_int64
    return L


def triangle_csr(n, r, c, v, dtype, op, fill):
    """(lower, rowptr, col, val, diag) of the effective strict triangle in chain order: what test_spsv_api.reference hands its helper"""
    R = VEC[dtype]
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    v = np.asarray(v, NP[dtype]).astype(R)
    keep = (r >= c) if fill == "lower" else (r <= c)
    r, c, v = r[keep], c[keep], v[keep]
    if op == "T":
        r, c = c, r
    lower = effective_lower(op, fill)
    diag = np.ones(n, R)
    on = r == c
    diag[r[on]] = v[on]
    r, c, v = r[~on], c[~on], v[~on]
    o = np.lexsort((c if lower else -c, r))
    r, c, v = r[o], c[o], np.ascontiguousarray(v[o])
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=rowptr[1:])
    return lower, rowptr, np.ascontiguousarray(c, np.int32), v, diag


def ref_sweeps(n, r, c, v, dtype, op, fill, unit, alpha, b, max_iter, tol, x0=None):
    """at most max_iter sweeps by the C helper from x0 (default +0); tol = NO_CHECK runs them all.  Returns (x, sweeps, converged, delta
    per sweep, xmax per sweep, changed per sweep), the per-sweep arrays cut to `sweeps`."""
    R = VEC[dtype]
    lower, rowptr, col, val, diag = triangle_csr(n, r, c, v, dtype, op, fill)
    bb = np.ascontiguousarray(b, R)
    x = np.zeros(n, R) if x0 is None else np.array(x0, R)
    tmp = np.zeros(n, R)
    m = int(max_iter)
    changed, delta, xmax = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), R), np.zeros(max(m, 1), R)
    conv = C.c_int32(0)
    fn = ref_lib().spitsv_ref_f64 if dtype == 2 else ref_lib().spitsv_ref_f32
    check = tol != NO_CHECK
    sweeps = fn(n, int(lower), int(bool(unit)), rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, diag.ctypes.data, R(alpha),
                bb.ctypes.data, x.ctypes.data, tmp.ctypes.data, m, R(tol if check else 0.0), int(check), changed.ctypes.data,
                delta.ctypes.data, xmax.ctypes.data, C.addressof(conv))
    return x, int(sweeps), int(conv.value), delta[:sweeps].copy(), xmax[:sweeps].copy(), changed[:sweeps].copy()


def plan_levels(bmsp, n, r, c, op, fill):
    ptr, other = block_records(n, r, c, op)
    _, _, lp, _ = bmsp.spsv_plan(ptr, other, effective_lower(op, fill), 0)
    return lp.size - 1


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("name", MATRICES + SMALL)
def test_reference_reaches_the_substitution_after_levels_sweeps(bmsp, name, dtype):
    """finite termination on the CPU: after `levels` sweeps the helper holds spsv_ref.c's bits, one more sweep changes nothing, and with
    tol = 0 it stops by itself within levels + 1 sweeps"""
    for op, fill, unit in COMBOS:
        n, r, c, v = values(name, dtype, op, fill, unit)
        b = rhs(n, dtype)
        levels = plan_levels(bmsp, n, r, c, op, fill)
        want = reference(n, r, c, v, dtype, op, fill, unit, 1.0, b)
        x, sweeps, conv, *_ = ref_sweeps(n, r, c, v, dtype, op, fill, unit, 1.0, b, levels, NO_CHECK)
        assert sweeps == levels and conv == 0
        assert_same_bits(x, want, "%s %s %s %s" % (name, op, fill, unit))
        x, sweeps, conv, delta, _, changed = ref_sweeps(n, r, c, v, dtype, op, fill, unit, 1.0, b, levels + 1, 0.0)
        assert conv == 1 and sweeps <= levels + 1 and changed[-1] == 0 and delta[-1] == 0
        assert_same_bits(x, want)
        # started from the solution: one sweep, nothing changes
        x, sweeps, conv, *_ = ref_sweeps(n, r, c, v, dtype, op, fill, unit, 1.0, b, 5, 0.0, x0=want)
        assert (sweeps, conv) == (1, 1)
        assert_same_bits(x, want)


# ---------------------------------------------------------------------------------------------------------
# the entry point
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture()
def vec():
    bufs = (C.c_float * 16)(), (C.c_float * 16)()
    return C.addressof(bufs[0]), C.addressof(bufs[1]), bufs


def test_refusals_in_order_scalars_before_handles(bmsp, vec):
    L = bmsp.lib()
    b, x, _ = vec
    hist = (C.c_double * 4)()
    info = bmsp.SpitsvInfo()

    def call(op=0, fill=0, diag=0, max_iter=0, tol=0.0, flags=0, h=None, A=None, db=b, dx=x):
        return L.bmsp_spitsv(A, op, fill, diag, 1.0, db, dx, max_iter, tol, flags, h, C.byref(info), None)

    # every scalar is named although the handle (and everything behind it) is null too, in the order of the argument list
    for kw, word in ((dict(op=2), "op"), (dict(op=-1, fill=7), "op"), (dict(fill=2, diag=5), "fill"), (dict(diag=2, max_iter=-1), "diag"),
                     (dict(max_iter=-1, tol=-2.0), "max_iter"), (dict(max_iter=(1 << 20) + 1), "max_iter"),
                     (dict(tol=float("nan"), flags=2), "tol"), (dict(tol=-0.5), "tol"), (dict(tol=-2.0), "tol"),
                     (dict(flags=2, tol=NO_CHECK, h=hist), "flags"), (dict(flags=-1), "flags"),
                     (dict(tol=NO_CHECK, h=hist), "delta_history")):
        assert call(**kw) == BMSP_ERR_INVALID, kw
        assert _msg(bmsp).startswith(word), (kw, _msg(bmsp))
    # good scalars (the largest max_iter, NO_CHECK without a history, the flag): the handle is named, then the vectors
    assert call(max_iter=1 << 20, tol=NO_CHECK, flags=1) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)
    assert call(tol=0.0, h=hist) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)
    assert L.bmsp_spitsv(None, 1, 1, 1, 1.0, None, None, 0, 0.0, 0, None, None, None) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)


def test_header_declares_the_interface_verbatim(bmsp):
    hdr = _flat(open(os.path.join(REPO, "include", "bmsp.h")).read())
    for line in ("#define BMSP_ITSV_X0_GIVEN 1", "#define BMSP_ITSV_NO_CHECK (-1.0)",
                 "typedef struct { char kernel[64]; int64_t sweeps, levels; int converged; double delta, xmax; } bmsp_spitsv_info;",
                 "int bmsp_spitsv(bmsp_matrix_t A, int op, int fill, int diag, double alpha, const void *d_b, void *d_x, "
                 "int64_t max_iter, double tol, int flags, double *delta_history /* host, may be NULL */, "
                 "bmsp_spitsv_info *info /* may be NULL */, void *stream);"):
        assert _flat(line) in hdr, line
    for phrase in ("d_x == d_b is refused", "bit for bit bmsp_spsv's x", "!changed || (tol > 0 && delta <= fl(tol * xmax))",
                   "BMSP_SPITSV_CHECK", "must not overlap on different streams", "bounds the sweep"):
        assert _flat(phrase) in hdr, phrase
    assert "bmsp_spitsv" in bmsp.SYMBOLS and hasattr(bmsp.lib(), "bmsp_spitsv")


def test_info_layout_and_wrappers(bmsp):
    I = bmsp.SpitsvInfo
    assert [f[0] for f in I._fields_] == ["kernel", "sweeps", "levels", "converged", "delta", "xmax"]
    assert C.sizeof(I) == 104 and (I.sweeps.offset, I.levels.offset, I.converged.offset, I.delta.offset, I.xmax.offset) == (64, 72, 80, 88, 96)
    assert set(I().as_dict()) == {f[0] for f in I._fields_}
    assert (bmsp.ITSV_X0_GIVEN, bmsp.ITSV_NO_CHECK) == (1, -1.0)
    assert list(inspect.signature(bmsp.spitsv).parameters) == ["A", "b", "op", "fill", "unit_diag", "alpha", "max_iter", "tol", "x", "x0_given",
                                                               "history", "stream"]
    d = {k: p.default for k, p in inspect.signature(bmsp.spitsv).parameters.items()}
    assert (d["op"], d["fill"], d["unit_diag"], d["alpha"], d["max_iter"], d["tol"], d["x"], d["x0_given"], d["history"], d["stream"]) == \
        ("N", "lower", False, 1.0, 0, 0.0, None, False, False, None)
    assert callable(bmsp.BmSpMatrix.solve_triangular_iterative)
    assert list(inspect.signature(bmsp.BmSpMatrix.solve_triangular_iterative).parameters)[1:] == list(inspect.signature(bmsp.spitsv).parameters)[1:]


def build_cpp_spitsv_check(out_path):
    lib_dir = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp_spitsv_check.cpp"), "-o", out_path, "-L" + lib_dir, "-lbmsp",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_spitsv_wrapper_compiles_and_links(bmsp, tmp_path):
    """include/bmSpMatrix.h with bmSparse_SpITSV instantiated for float, half and double links against libbmsp.so with a plain host
    compiler."""
    build_cpp_spitsv_check(str(tmp_path / "cpp_spitsv_check"))


# ---------------------------------------------------------------------------------------------------------
# the kernels in the assembly
# ---------------------------------------------------------------------------------------------------------
INT_ATOMIC = re.compile(r"\s*(global|flat)_atomic_(u?max|or)_(x2|u64|b64)\b")
ANY_ATOMIC = re.compile(r"\s*\w*atomic\w*|\s*ds_(add|sub|min|max|inc|dec|cmpst|wrxchg)", re.I)
FLOAT_ATOMIC = re.compile(r"\s*\w*atomic\w*_(f16|f32|f64|pk_\w+)\b", re.I)
FRAG = "19spitsv_sweep_kernel"


@pytest.fixture(scope="module")
def spitsv_asm(tmp_path_factory):
    from test_fold_handoff_asm import to_asm, functions
    path = to_asm("spitsv", str(tmp_path_factory.mktemp("spitsv_asm")))
    return functions(path), open(path).read()


def _sweep_targs(s, minor, lower, unit, stats):
    return _targs(s, minor, lower, unit)[:-1] + "Lb%dEE" % stats


def test_every_instantiation_is_in_the_assembly(spitsv_asm):
    fns, _ = spitsv_asm
    ks = {n: b for n, b in fns.items() if FRAG in n}
    assert len(ks) == 48, sorted(ks)
    for s in (0, 1, 2):
        for minor in (0, 1):
            for lower in (0, 1):
                for unit in (0, 1):
                    for stats in (0, 1):
                        assert sum(FRAG + _sweep_targs(s, minor, lower, unit, stats) in n for n in ks) == 1, (s, minor, lower, unit, stats)


def test_kernels_use_no_scratch_keep_subnormals_and_only_integer_atomics(spitsv_asm):
    fns, text = spitsv_asm
    n = 0
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        if "spitsv_sweep" not in m.group(1):
            continue
        n += 1
        body = m.group(2)
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), m.group(1)
        assert re.search(r"\.amdhsa_float_denorm_mode_32 3\b", body) and re.search(r"\.amdhsa_float_denorm_mode_16_64 3\b", body), m.group(1)
    assert n == 48
    for name, body in fns.items():
        if FRAG not in name:
            continue
        assert not any(re.match(r"\s*scratch_", ln) for ln in body), name
        atomics = [ln for ln in body if ANY_ATOMIC.match(ln)]
        assert not [ln for ln in atomics if FLOAT_ATOMIC.match(ln)], (name, atomics[:3])
        if re.search(r"Lb[01]ELb[01]ELb[01]ELb1EE", name):     # <.., STATS = true>
            assert atomics and all(INT_ATOMIC.match(ln) for ln in atomics), (name, atomics[:4])
        else:
            assert not atomics, (name, atomics[:3])       # the preconditioner mode: launches only


def test_division_sequence_and_fused_multiply_adds(spitsv_asm):
    """the chain of operations is bmsp_spsv's: fused multiply-adds everywhere, one IEEE division sequence in the non-unit kernels, none
    and no reciprocal in the unit ones"""
    fns, _ = spitsv_asm
    fma = re.compile(r"\s*v_(fma|fmac)_(f32|f64)")
    for name, body in fns.items():
        if FRAG not in name:
            continue
        assert any(fma.match(ln) for ln in body), name
        ops = [ln.split()[0] for ln in body if ln.strip()]
        unit = re.search(r"Lb[01]ELb[01]ELb1ELb[01]EE", name) is not None
        div = [o for o in ops if o.startswith("v_div_") or o.startswith("v_rcp")]
        if unit:
            assert not div, (name, div[:4])
            continue
        fixup = sum(o.startswith("v_div_fixup") for o in ops)
        assert fixup >= 1 and sum(o.startswith("v_div_fmas") for o in ops) == fixup and sum(o.startswith("v_rcp") for o in ops) == fixup, name
