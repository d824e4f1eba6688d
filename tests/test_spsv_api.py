"""CPU tests of the surface of bmsp_spsv, and what tests/test_spsv.py shares with them: the matrices, the reference (tests/spsv_ref.c through
ctypes) and a Python restatement of the planner.

Checked here without a GPU: bmsp_spsv_plan against the restatement and its invariants; the refusals of the three C entry points (scalars
before handles, the argument named); the prototypes and defines in bmsp.h; the layout of bmsp_spsv_info; the Python and C++ wrappers; the
gfx950 assembly of spsv.hip (every instantiation, no scratch, subnormals kept, no atomic, the division sequence in the non-unit kernels,
fused multiply-adds in all of them)."""
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile
import numpy as np
import pytest
from conftest import REPO

BMSP_ERR_INVALID = -1
NP = {0: np.float32, 1: np.float16, 2: np.float64}       # storage type of a dtype (F32, F16, F64)
VEC = {0: np.float32, 1: np.float32, 2: np.float64}      # type of b and x


# ---------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_lib():
    d = tempfile.mkdtemp(prefix="spsv_ref_")
    so = os.path.join(d, "libspsv_ref.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(REPO, "tests", "spsv_ref.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.spsv_ref_f32.argtypes = [C.c_int64, C.c_int, C.c_int, vp, vp, vp, vp, C.c_float, vp, vp]
    L.spsv_ref_f64.argtypes = [C.c_int64, C.c_int, C.c_int, vp, vp, vp, vp, C.c_double, vp, vp]
    L.spsv_ref_f32.restype = L.spsv_ref_f64.restype = None
    return L


def effective_lower(op, fill):
    return (fill == "lower") != (op == "T")


def reference(n, r, c, v, dtype, op, fill, unit, alpha, b):
    """x of op(tri(A)) x = alpha b by the C helper: A = COO (r, c, v) with v already rounded to the dtype; only the triangle `fill` of A is
    handed over, in chain order."""
    R = VEC[dtype]
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    v = np.asarray(v, NP[dtype]).astype(R)                  # (fp16 widens exactly)
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
    col = np.ascontiguousarray(c, np.int32)
    bb = np.ascontiguousarray(b, R)
    x = np.zeros(n, R)
    fn = ref_lib().spsv_ref_f64 if dtype == 2 else ref_lib().spsv_ref_f32
    fn(n, int(lower), int(bool(unit)), rowptr.ctypes.data, col.ctypes.data, v.ctypes.data, diag.ctypes.data, R(alpha), bb.ctypes.data,
       x.ctypes.data)
    return x


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_same_bits(got, want, msg=""):
    """bit for bit; a NaN must be a NaN (its sign and payload are the hardware's)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype, msg)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "NaN at %s, expected at %s %s" % (np.flatnonzero(gn)[:8], np.flatnonzero(wn)[:8], msg)
    bad = np.flatnonzero((bits(got) != bits(want)) & ~wn)
    assert bad.size == 0, "%d of %d differ, first at %d: %r != %r %s" % (bad.size, got.size, bad[0], got[bad[0]], want[bad[0]], msg)


# ---------------------------------------------------------------------------------------------------------
# the matrices
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pattern(name):
    """(n, rows, cols) of a test matrix: the generator's coordinates and the whole diagonal, sorted by (row, col)"""
    from pybmsp import gen
    if name == "ragged203":
        n, _, r, c, _ = gen.random_coo(203, 203, 203 * 26, seed=3)
    elif name == "banded400":
        n, _, r, c, _ = gen.banded(400, 12)
    elif name == "fem8":
        n, _, r, c, _ = gen.fem_like(8, "27pt")
    elif name == "rmat10":
        n, _, r, c, _ = gen.rmat(10, 8)
    elif name == "random2000":
        n, _, r, c, _ = gen.random_coo(2000, 2000, 1500, seed=5)
    elif name == "diag3001":
        n, r, c = 3001, np.zeros(0, np.int64), np.zeros(0, np.int64)
    elif name.startswith("dense"):                      # dense1, dense5, dense9: every coordinate
        n = int(name[5:])
        r, c = [a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij")]
    else:
        raise KeyError(name)
    d = np.arange(n, dtype=np.int64)
    key = np.unique(np.concatenate([np.asarray(r, np.int64) * n + np.asarray(c, np.int64), d * n + d]))
    return int(n), key // n, key % n


MATRICES = ("ragged203", "banded400", "fem8", "rmat10", "random2000", "diag3001")
SMALL = ("dense1", "dense5", "dense9")
# block-rows, levels (lower, upper), widest level (lower, upper) of the six: computed on the CPU when the operation was specified
SHAPES = {"ragged203": (26, (26, 26), (1, 1)), "banded400": (50, (50, 50), (1, 1)), "fem8": (64, (59, 59), (2, 2)),
          "rmat10": (128, (39, 38), (8, 38)), "random2000": (250, (16, 12), (37, 43)), "diag3001": (376, (1, 1), (376, 376))}


def values(name, dtype, op, fill, unit, seed=11):
    """the values of matrix `name` for one solve, rounded to the dtype, as float64: off-diagonal magnitudes in [0.5, 2) with mixed signs;
    the stored diagonal +-(1 + the absolute sum of the entry's row of the effective strict triangle); under a unit diagonal the rows of
    that triangle scaled to an absolute sum of at most 0.5 (the stored diagonal is then never read)."""
    n, r, c = pattern(name)
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.5, 2.0, r.size) * rng.choice([-1.0, 1.0], r.size)
    strict = (r > c) if fill == "lower" else (r < c)
    erow = c if op == "T" else r                        # the row of the effective matrix an entry of the triangle belongs to
    if unit:
        s = np.bincount(erow[strict], weights=np.abs(v[strict]), minlength=n)
        f = np.where(s > 0.5, 0.5 / np.maximum(s, 1e-300), 1.0) * 0.999     # (rounding to the dtype must not lift the sum over 0.5)
        v[strict] *= f[erow[strict]]
    v = v.astype(NP[dtype]).astype(np.float64)
    s = np.bincount(erow[strict], weights=np.abs(v[strict]), minlength=n)
    on = r == c
    v[on] = ((1.0 + s) * rng.choice([-1.0, 1.0], n))[r[on]]
    return n, r, c, v.astype(NP[dtype]).astype(np.float64)


def rhs(n, dtype, seed=5):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(VEC[dtype])


def block_records(n, r, c, op):
    """(ptr, other) of the records of op(A) in the order of its output blocks"""
    br, bc = (c // 8, r // 8) if op == "T" else (r // 8, c // 8)
    blocks = (n + 7) // 8
    key = np.unique(np.asarray(br, np.int64) * blocks + bc)
    ptr = np.zeros(blocks + 1, np.uint32)
    np.cumsum(np.bincount(key // blocks, minlength=blocks), out=ptr[1:])
    return ptr, (key % blocks).astype(np.uint32)


def py_plan(ptr, other, lower, chain):
    """the planner restated: (level_of, order, level_ptr, segments)"""
    ptr, other = np.asarray(ptr, np.int64), np.asarray(other, np.int64)
    blocks = ptr.size - 1 if ptr.size else 0
    lev = np.zeros(blocks, np.int64)
    for I in (range(blocks) if lower else range(blocks - 1, -1, -1)):
        d = other[ptr[I]:ptr[I + 1]]
        d = d[d < I] if lower else d[d > I]
        lev[I] = 1 + lev[d].max() if d.size else 0
    order = np.lexsort((np.arange(blocks), lev))
    nl = int(lev.max()) + 1 if blocks else 0
    level_ptr = np.concatenate([[0], np.cumsum(np.bincount(lev, minlength=nl))]).astype(np.int64)
    w = np.diff(level_ptr)
    segs, l = [], 0
    while l < nl:
        e = l
        while e < nl and w[e] <= chain:
            e += 1
        if e - l >= 2:
            segs.append((l, e, 1))
            l = e
        else:
            segs.append((l, l + 1, 0))
            l += 1
    return lev, order, level_ptr, np.asarray(segs, np.int64).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------------
# the planner
# ---------------------------------------------------------------------------------------------------------
def arrow(blocks):
    """first block-column and last block-row full, and the diagonal"""
    rows = [(I, sorted({0, I})) for I in range(blocks - 1)] + [(blocks - 1, list(range(blocks)))]
    ptr = np.cumsum([0] + [len(o) for _, o in rows]).astype(np.uint32)
    return ptr, np.asarray([j for _, o in rows for j in o], np.uint32)


def gaps(blocks):
    """empty block-rows between full ones"""
    rows = [list(range(blocks)) if I % 3 == 0 else [] for I in range(blocks)]
    ptr = np.cumsum([0] + [len(o) for o in rows]).astype(np.uint32)
    return ptr, np.asarray([j for o in rows for j in o], np.uint32)


def plan_structures():
    out = {}
    for name in MATRICES + SMALL:
        n, r, c = pattern(name)
        for op in "NT":
            out[name + "-" + op] = block_records(n, r, c, op)
    out["arrow"] = arrow(13)
    out["gaps"] = gaps(11)
    out["empty"] = (np.zeros(1, np.uint32), np.zeros(0, np.uint32))
    out["none"] = (np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    return out


CHAINS = (0, 1, 4, 1 << 31)


@pytest.mark.parametrize("lower", [1, 0])
@pytest.mark.parametrize("name", sorted(plan_structures()))
def test_plan_matches_the_restatement_and_its_invariants(bmsp, name, lower):
    ptr, other = plan_structures()[name]
    blocks = max(0, ptr.size - 1)
    for chain in CHAINS:
        lev, order, lp, segs = bmsp.spsv_plan(ptr, other, lower, chain)
        wl, wo, wlp, ws = py_plan(ptr, other, lower, chain)
        np.testing.assert_array_equal(lev, wl)
        np.testing.assert_array_equal(order, wo)
        np.testing.assert_array_equal(lp, wlp)
        np.testing.assert_array_equal(segs.reshape(-1, 3), ws)
        # invariants, on the library's own output
        nl = lp.size - 1
        assert sorted(order.tolist()) == list(range(blocks))
        keys = [(int(lev[I]), int(I)) for I in order]
        assert keys == sorted(keys)
        for I in range(blocks):
            d = other[ptr[I]:ptr[I + 1]].astype(np.int64)
            d = d[d < I] if lower else d[d > I]
            assert (lev[d] < lev[I]).all()
            assert lev[I] == (lev[d].max() + 1 if d.size else 0)
        if blocks:
            assert lp[0] == 0 and lp[-1] == blocks and (np.diff(lp.astype(np.int64)) > 0).all()
        at = 0
        for l0, l1, kind in segs.reshape(-1, 3).astype(np.int64):
            assert l0 == at and l1 > l0 and kind in (0, 1)
            at = l1
            w = np.diff(lp.astype(np.int64))[l0:l1]
            if kind:
                assert l1 - l0 >= 2 and (w <= chain).all()
            else:
                assert l1 - l0 == 1
        assert at == nl
        if chain == 0:
            assert len(segs) == nl and not segs.reshape(-1, 3)[:, 2].any()


@pytest.mark.parametrize("name", MATRICES)
def test_the_matrices_have_the_shapes_the_cases_need(bmsp, name):
    n, r, c = pattern(name)
    blocks, levels, widths = SHAPES[name]
    ptr, other = block_records(n, r, c, "N")
    assert ptr.size - 1 == blocks
    for lower in (1, 0):
        _, _, lp, _ = bmsp.spsv_plan(ptr, other, lower, 0)
        assert lp.size - 1 == levels[1 - lower], (name, lower, lp.size - 1)
        assert int(np.diff(lp.astype(np.int64)).max()) == widths[1 - lower], (name, lower)


def _msg(bmsp):
    return bmsp.lib().bmsp_last_error().decode(errors="replace")


def test_plan_refusals(bmsp):
    L = bmsp.lib()
    ptr = np.array([0, 1, 3], np.uint32)
    other = np.array([0, 0, 1], np.uint32)
    nl, ns = C.c_int64(), C.c_int64()

    def call(p, o, blocks, chain):
        return L.bmsp_spsv_plan(p, o, blocks, 1, chain, None, None, None, None, C.byref(nl), C.byref(ns))

    assert call(ptr.ctypes.data, other.ctypes.data, 2, 4) == 0 and nl.value == 2
    assert call(ptr.ctypes.data, other.ctypes.data, -1, 4) == BMSP_ERR_INVALID and "blocks" in _msg(bmsp)
    assert call(ptr.ctypes.data, other.ctypes.data, 2, -1) == BMSP_ERR_INVALID and "chain" in _msg(bmsp)
    assert call(None, other.ctypes.data, 2, 4) == BMSP_ERR_INVALID and "ptr" in _msg(bmsp)
    assert call(None, None, 0, 4) == 0 and nl.value == 0 and ns.value == 0
    down = np.array([0, 3, 2], np.uint32)
    assert call(down.ctypes.data, other.ctypes.data, 2, 4) == BMSP_ERR_INVALID and "ptr decreases" in _msg(bmsp)
    far = np.array([0, 1, 2], np.uint32)
    assert call(ptr.ctypes.data, far.ctypes.data, 2, 4) == BMSP_ERR_INVALID and "other" in _msg(bmsp)


# ---------------------------------------------------------------------------------------------------------
# the entry points
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture()
def vec():
    """a host buffer standing in for a device vector: the calls under test refuse before they touch it"""
    buf = (C.c_float * 16)()
    return C.addressof(buf)


def test_scalars_are_refused_before_handles_and_named(bmsp, vec):
    L = bmsp.lib()
    info = bmsp.SpsvInfo()
    for args, word in (((2, 0, 0), "op"), ((-1, 0, 0), "op"), ((0, 2, 0), "fill"), ((1, -1, 0), "fill"), ((0, 0, 2), "diag"),
                       ((1, 1, -1), "diag")):
        assert L.bmsp_spsv(None, *args, 1.0, vec, vec, None) == BMSP_ERR_INVALID
        assert _msg(bmsp).startswith(word), (args, _msg(bmsp))
        assert L.bmsp_spsv_analyse(None, *args, None, C.byref(info)) == BMSP_ERR_INVALID
        assert _msg(bmsp).startswith(word), (args, _msg(bmsp))
    # a bad scalar is named although the handle is null too; with good scalars the handle is
    assert L.bmsp_spsv(None, 0, 0, 0, 1.0, vec, vec, None) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)
    assert L.bmsp_spsv(None, 1, 1, 1, 1.0, None, None, None) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)
    assert L.bmsp_spsv_analyse(None, 0, 0, 0, None, None) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)


def _flat(s):
    return re.sub(r"\s+", " ", s)


def test_header_declares_the_interface_verbatim(bmsp):
    hdr = _flat(open(os.path.join(REPO, "include", "bmsp.h")).read())
    for line in ("#define BMSP_FILL_LOWER 0", "#define BMSP_FILL_UPPER 1", "#define BMSP_DIAG_NON_UNIT 0", "#define BMSP_DIAG_UNIT 1",
                 "typedef struct { char kernel[64]; int64_t levels, max_level_width, launches, chain_launches, chained_levels, plan_bytes; } "
                 "bmsp_spsv_info;",
                 "int bmsp_spsv_analyse(bmsp_matrix_t A, int op, int fill, int diag, void *stream, bmsp_spsv_info *info /* may be NULL */);",
                 "int bmsp_spsv(bmsp_matrix_t A, int op, int fill, int diag, double alpha, const void *d_b, void *d_x, void *stream);",
                 "int bmsp_spsv_plan(const uint32_t *ptr, const uint32_t *other, int64_t blocks, int lower, int64_t chain, "
                 "uint32_t *level_of, uint32_t *order, uint32_t *level_ptr, uint32_t *segments, int64_t *n_levels, int64_t *n_segments);"):
        assert _flat(line) in hdr, line
    assert "thousands of tiles" in hdr          # the stated limit: a long block-row is one lane group's serial chain
    for name in ("bmsp_spsv_analyse", "bmsp_spsv", "bmsp_spsv_plan"):
        assert name in bmsp.SYMBOLS and hasattr(bmsp.lib(), name)


def test_info_layout_and_wrappers(bmsp):
    I = bmsp.SpsvInfo
    assert [f[0] for f in I._fields_] == ["kernel", "levels", "max_level_width", "launches", "chain_launches", "chained_levels", "plan_bytes"]
    assert C.sizeof(I) == 64 + 6 * 8 and I.levels.offset == 64 and I.plan_bytes.offset == 104
    assert set(I().as_dict()) == {f[0] for f in I._fields_}
    assert (bmsp.FILL_LOWER, bmsp.FILL_UPPER, bmsp.DIAG_NON_UNIT, bmsp.DIAG_UNIT) == (0, 1, 0, 1)
    for name in ("spsv", "spsv_analyse", "spsv_plan"):
        assert callable(getattr(bmsp, name))
    assert callable(bmsp.BmSpMatrix.solve_triangular)
    import inspect
    assert list(inspect.signature(bmsp.spsv).parameters) == ["A", "b", "op", "fill", "unit_diag", "alpha", "x", "stream"]
    assert list(inspect.signature(bmsp.spsv_analyse).parameters) == ["A", "op", "fill", "unit_diag", "stream"]
    assert list(inspect.signature(bmsp.spsv_plan).parameters) == ["ptr", "other", "lower", "chain"]


def build_cpp_spsv_check(out_path):
    lib_dir = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp_spsv_check.cpp"), "-o", out_path, "-L" + lib_dir, "-lbmsp",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_spsv_wrappers_compile_and_link(bmsp, tmp_path):
    """include/bmSpMatrix.h with bmSparse_SpSV / bmSparse_SpSV_analyse instantiated for float, half and double links against libbmsp.so
    with a plain host compiler."""
    build_cpp_spsv_check(str(tmp_path / "cpp_spsv_check"))


# ---------------------------------------------------------------------------------------------------------
# the kernels in the assembly
# ---------------------------------------------------------------------------------------------------------
FMA = re.compile(r"\s*v_(fma|fmac)_(f32|f64)")
ATOMIC = re.compile(r"\s*\w*atomic\w*|\s*ds_(add|sub|min|max|inc|dec|cmpst|wrxchg)", re.I)


@pytest.fixture(scope="module")
def spsv_asm(tmp_path_factory):
    from test_fold_handoff_asm import to_asm, functions
    path = to_asm("spsv", str(tmp_path_factory.mktemp("spsv_asm")))
    return functions(path), open(path).read()


def _kernels(fns, frag):
    return {n: b for n, b in fns.items() if frag in n}


def _targs(s, minor, lower, unit):
    """the mangled template arguments <S, MINOR, LOWER, UNIT>"""
    return "I%sLb%dELb%dELb%dEE" % ({0: "f", 1: "t", 2: "d"}[s], minor, lower, unit)


def test_every_instantiation_is_in_the_assembly(spsv_asm):
    fns, _ = spsv_asm
    for frag in ("17spsv_level_kernel", "17spsv_chain_kernel"):
        ks = _kernels(fns, frag)
        assert len(ks) == 24, sorted(ks)
        for s in (0, 1, 2):
            for minor in (0, 1):
                for lower in (0, 1):
                    for unit in (0, 1):
                        assert sum(frag + _targs(s, minor, lower, unit) in n for n in ks) == 1, (frag, s, minor, lower, unit)


def test_kernels_use_no_scratch_keep_subnormals_and_hold_no_atomic(spsv_asm):
    fns, text = spsv_asm
    n = 0
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        if "spsv_" not in m.group(1):
            continue
        n += 1
        body = m.group(2)
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), m.group(1)
        assert re.search(r"\.amdhsa_float_denorm_mode_32 3\b", body) and re.search(r"\.amdhsa_float_denorm_mode_16_64 3\b", body), m.group(1)
    assert n == 48
    for name, body in fns.items():
        bad = [ln for ln in body if ATOMIC.match(ln)]
        assert not bad, (name, bad[:3])
        assert not any(re.match(r"\s*scratch_", ln) for ln in body), name


def test_division_sequence_and_fused_multiply_adds(spsv_asm):
    fns, _ = spsv_asm
    for frag in ("17spsv_level_kernel", "17spsv_chain_kernel"):
        for name, body in _kernels(fns, frag).items():
            assert any(FMA.match(ln) for ln in body), name
            ops = [ln.split()[0] for ln in body if ln.strip()]
            unit = re.search(r"Lb[01]ELb[01]ELb1EE", name) is not None
            div = [o for o in ops if o.startswith("v_div_") or o.startswith("v_rcp")]
            if unit:
                assert not div, (name, div[:4])          # x_i = s: nothing divides
                continue
            scale = sum(o.startswith("v_div_scale") for o in ops)
            fmas = sum(o.startswith("v_div_fmas") for o in ops)
            fixup = sum(o.startswith("v_div_fixup") for o in ops)
            rcp = sum(o.startswith("v_rcp") for o in ops)
            assert fixup >= 1 and fmas == fixup and scale == 2 * fixup, (name, scale, fmas, fixup)
            # a reciprocal only ever seeds a division sequence: one per sequence, and each is followed by the sequence's v_div_fmas
            assert rcp == fixup, (name, rcp, fixup)
            for k, o in enumerate(ops):
                if o.startswith("v_rcp"):
                    nxt = [p for p in ops[k + 1:] if p.startswith("v_div_fmas") or p.startswith("v_rcp")]
                    assert nxt and nxt[0].startswith("v_div_fmas"), name
