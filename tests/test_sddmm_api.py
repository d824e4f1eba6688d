"""CPU tests of the surface of bmsp_sddmm: the C entry points refuse bad scalars and null pointers with BMSP_ERR_INVALID and name the
argument, scalars before handles, all before any device call; the symbols are exported and declared with their exact prototypes; the
Python and C++ wrappers exist and link; the gfx950 assembly of sddmm.hip holds every instantiation, the matrix-core instructions of the
two tile kernels, no scratch, keeps subnormals and holds no atomic and no LDS add of any kind; and the generated inputs of the GPU file
(tests/test_sddmm.py) meet the conditions its bit-for-bit comparisons rest on."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from conftest import REPO

BMSP_ERR_INVALID = -1


def build_cpp_sddmm_check(out_path):
    lib_dir = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp_sddmm_check.cpp"), "-o", out_path, "-L" + lib_dir, "-lbmsp",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def _msg(bmsp):
    return bmsp.lib().bmsp_last_error().decode(errors="replace")


@pytest.fixture()
def buf():
    """a host buffer standing in for a device array: the calls under test refuse before they touch it"""
    b = (C.c_float * 64)()
    return C.addressof(b)


def calls(bmsp, buf, k=4, ldx=4, ldy=4, beta=0.0, flags=0, lay=0, X="buf", Y="buf", out=True, info=True):
    """the three entry points with a null S: [(name, status, message)]"""
    L = bmsp.lib()
    x = buf if X == "buf" else None
    y = buf if Y == "buf" else None
    h, inf = C.c_void_p(), bmsp.SddmmInfo()
    res = []
    res.append(("bmsp_sddmm", L.bmsp_sddmm(None, x, ldx, y, ldy, k, 1.0, beta, flags, lay, None, C.byref(h) if out else None), _msg(bmsp)))
    res.append(("bmsp_sddmm_values", L.bmsp_sddmm_values(None, x, ldx, y, ldy, k, 1.0, beta, flags, None, None), _msg(bmsp)))
    if not flags and not beta:
        res.append(("bmsp_sddmm_launch_info", L.bmsp_sddmm_launch_info(None, k, ldx, ldy, lay, C.byref(inf) if info else None), _msg(bmsp)))
    return res


# ---------------------------------------------------------------------------------------------------------
# refusals through the raw C calls, null handles
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,word", [
    (dict(k=0), "k must"), (dict(k=-3), "k must"), (dict(k=8, ldx=7, ldy=8), "ldx"), (dict(k=8, ldx=8, ldy=5), "ldy"),
    (dict(flags=2), "flags"), (dict(flags=-1), "flags"), (dict(flags=1, beta=0.5), "beta"),
])
def test_bad_scalars_are_refused_before_the_handles(bmsp, buf, kw, word):
    for ptrs in (dict(), dict(X=None, Y=None, out=False, info=False)):
        for name, status, msg in calls(bmsp, buf, **kw, **ptrs):
            assert status == BMSP_ERR_INVALID, name
            assert word in msg and "null" not in msg, (name, msg)


@pytest.mark.parametrize("lay", [2, -1, 1 << 16])
def test_bad_out_transposed_is_refused_before_the_handles(bmsp, buf, lay):
    L = bmsp.lib()
    h, inf = C.c_void_p(), bmsp.SddmmInfo()
    for hp, ip in ((None, None), (C.byref(h), C.byref(inf))):
        assert L.bmsp_sddmm(None, buf, 4, buf, 4, 4, 1.0, 0.0, 0, lay, None, hp) == BMSP_ERR_INVALID
        assert "out_transposed" in _msg(bmsp) and "null" not in _msg(bmsp), _msg(bmsp)
        assert L.bmsp_sddmm_launch_info(None, 4, 4, 4, lay, ip) == BMSP_ERR_INVALID
        assert "out_transposed" in _msg(bmsp) and "null" not in _msg(bmsp), _msg(bmsp)


def test_null_handle_is_refused_after_the_scalars(bmsp, buf):
    for kw in (dict(), dict(X=None), dict(Y=None), dict(out=False, info=False), dict(flags=1), dict(beta=2.0), dict(lay=1)):
        for name, status, msg in calls(bmsp, buf, **kw):
            assert status == BMSP_ERR_INVALID, name
            assert "null" in msg and "S" in msg and "must" not in msg, (name, msg)


def test_python_wrappers_refuse_bad_arguments(bmsp):
    class Fake:  # stands in for a matrix: the wrappers refuse from info() alone, before any C call
        h = None

        def info(self):
            return {"num_rows": 5, "num_cols": 3, "dtype": 0, "transposed": 0}

    f32 = lambda n: type("A", (), {"dtype": np.dtype(np.float32), "n": n, "ptr": 0})()
    f64 = lambda n: type("A", (), {"dtype": np.dtype(np.float64), "n": n, "ptr": 0})()
    for args in ((f32(20), f32(12), 0), (f64(20), f32(12), 4), (f32(20), f64(12), 4), (f32(19), f32(12), 4), (f32(20), f32(11), 4),
                 (None, f32(12), 4), (f32(20), None, 4)):
        with pytest.raises(ValueError):
            bmsp.sddmm(Fake(), *args)
        with pytest.raises(ValueError):
            bmsp.sddmm_values(Fake(), Fake(), *args)
    with pytest.raises(ValueError):
        bmsp.sddmm(Fake(), f32(20), f32(12), 4, ldx=3)
    with pytest.raises(ValueError):
        bmsp.sddmm(Fake(), f32(5 * 6 - 3), f32(12), 4, ldx=6)  # too few elements at the leading dimension
    with pytest.raises(ValueError):
        bmsp.sddmm_values(Fake(), Fake(), f32(20), f32(3 * 9 - 6), 4, ldy=9)


# ---------------------------------------------------------------------------------------------------------
# symbols and wrappers
# ---------------------------------------------------------------------------------------------------------
def test_sddmm_symbols_are_declared(bmsp):
    for name in ("bmsp_sddmm", "bmsp_sddmm_values", "bmsp_sddmm_launch_info"):
        assert name in bmsp.SYMBOLS and hasattr(bmsp.lib(), name)
    with open(os.path.join(REPO, "include", "bmsp.h")) as f:
        text = f.read()
    for line in ("#define BMSP_SDDMM_MUL_S 1   /* flags bit 0: c = fl(fl(alpha*d) * s) instead of fl(fl(alpha*d) + fl(beta*s)) */",
                 "int bmsp_sddmm(bmsp_matrix_t S, const void *d_X, int64_t ldx, const void *d_Y, int64_t ldy, int k,\n"
                 "               double alpha, double beta, int flags, int out_transposed, void *stream, bmsp_matrix_t *out);",
                 "int bmsp_sddmm_values(bmsp_matrix_t S, const void *d_X, int64_t ldx, const void *d_Y, int64_t ldy, int k,\n"
                 "                      double alpha, double beta, int flags, bmsp_matrix_t out, void *stream);",
                 "typedef struct { char kernel[64]; int lanes; int64_t compulsory_bytes; } bmsp_sddmm_info;",
                 "int bmsp_sddmm_launch_info(bmsp_matrix_t S, int k, int64_t ldx, int64_t ldy, int out_transposed, bmsp_sddmm_info *info);"):
        assert line in text, line
    # the ctypes mirror has the C struct's layout: 64 + int (+ padding) + one int64
    assert C.sizeof(bmsp.SddmmInfo) == 64 + 8 + 8 and bmsp.SddmmInfo.lanes.offset == 64 and bmsp.SddmmInfo.compulsory_bytes.offset == 72
    assert bmsp.SDDMM_MUL_S == 1


def test_python_wrappers_exist(bmsp):
    for fn in (bmsp.sddmm, bmsp.sddmm_values, bmsp.sddmm_launch_info, bmsp.BmSpMatrix.sddmm, bmsp.BmSpMatrix.sddmm_):
        assert callable(fn)


def test_cpp_sddmm_wrappers_compile_and_link(tmp_path):
    """include/bmSpMatrix.h with bmSparse_sddmm / bmSparse_sddmm_values instantiated for float, half and double links against
    libbmsp.so with a plain host compiler."""
    build_cpp_sddmm_check(str(tmp_path / "cpp_sddmm_check"))


# ---------------------------------------------------------------------------------------------------------
# the kernels in the assembly
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sddmm_asm(tmp_path_factory):
    from test_fold_handoff_asm import to_asm, functions
    d = str(tmp_path_factory.mktemp("sddmm_asm"))
    fns = functions(to_asm("sddmm", d))
    with open(os.path.join(d, "sddmm.s")) as f:
        text = f.read()
    return fns, text


def test_every_instantiation_is_there(sddmm_asm):
    """value kernel: 3 dtypes (t = uint16_t bits of an fp16, f, d) x 1 / 8 lanes per tile; tile kernel: fp16 and fp32"""
    fns, _ = sddmm_asm
    values, tiles = set(), set()
    for name in fns:
        m = re.search(r"18sddmm_value_kernelI([tfd])Li([18])E", name)
        if m:
            values.add((m.group(1), int(m.group(2))))
        m = re.search(r"17sddmm_tile_kernelI([tfd])E", name)
        if m:
            tiles.add(m.group(1))
    assert values == {(d, g) for d in "tfd" for g in (1, 8)}, sorted(values)
    assert tiles == {"t", "f"}, sorted(tiles)


def test_tile_kernels_use_the_matrix_cores(sddmm_asm):
    fns, _ = sddmm_asm
    want = {"t": "v_mfma_f32_16x16x32_f16", "f": "v_mfma_f32_16x16x4_f32"}
    for name, body in fns.items():
        m = re.search(r"17sddmm_tile_kernelI([tf])E", name)
        if m:
            used = set(re.findall(r"^\s*(v_mfma_\w+)", "\n".join(body), re.M))
            assert used == {want[m.group(1)]}, (name, used)
        elif "sddmm_value_kernel" in name:
            assert not any("v_mfma" in ln for ln in body), name


def test_no_scratch_and_subnormals_kept(sddmm_asm):
    _, text = sddmm_asm
    sizes = re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text)
    assert sizes and all(int(s) == 0 for s in sizes), sizes
    assert set(re.findall(r"\.amdhsa_float_denorm_mode_32\s+(\d+)", text)) == {"3"}
    assert set(re.findall(r"\.amdhsa_float_denorm_mode_16_64\s+(\d+)", text)) == {"3"}


def test_no_atomics_no_lds(sddmm_asm):
    """every output value has one writer and every sum a fixed order: no atomic instruction of any kind in the whole file, no LDS
    instruction at all, and no atomic call in the source"""
    _, text = sddmm_asm
    bad = set(re.findall(r"^\s*((?:global|flat|buffer|ds)_\w*atomic\w*|ds_\w+)\s", text, re.M))
    assert not bad, bad
    lds = re.findall(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", text)
    assert lds and all(int(s) == 0 for s in lds), lds
    with open(os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "csrc", "sddmm.hip")) as f:
        src = f.read()
    code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
    assert not re.findall(r"\b(atomic\w*|unsafeAtomic\w+|__hip_atomic\w+|__builtin_amdgcn_\w*atomic\w*)\s*\(", code)
    assert "__shared__" not in code


def test_tile_kernel_loads_are_global(sddmm_asm):
    """the operand fragments come from global loads (16 bytes in the full k steps), never flat ones"""
    fns, _ = sddmm_asm
    for name, body in fns.items():
        if "sddmm_tile_kernel" in name or "sddmm_value_kernel" in name:
            assert not any(re.match(r"\s*flat_", ln) for ln in body), name
            assert any(re.match(r"\s*global_load_dwordx4\s", ln) for ln in body), name


# ---------------------------------------------------------------------------------------------------------
# the generated inputs of tests/test_sddmm.py, host only
# ---------------------------------------------------------------------------------------------------------
def test_integer_cases_are_exact_in_every_storage_type():
    """test 1 of the GPU file compares bit for bit: X, Y in [-3, 3], s in [-4, 4]; every partial sum (bounded by sum |x y|) is an
    integer below 2^24 and every result (all five epilogues, every k) is exactly representable in fp16, hence in fp32 and fp64"""
    import test_sddmm as T
    worst = 0
    for name in T.NAMES:
        X, Y, s = T.int_operands(name)
        for a, lo, hi in ((X, -3, 3), (Y, -3, 3), (s, -4, 4)):
            assert a.size == 0 or (a.min() >= lo and a.max() <= hi)
        for k in T.KS:
            d, absd = T.int_dots(name, k)
            if d.size == 0:
                continue
            assert absd.max() <= 9 * k <= 900 < 2 ** 11  # any partial sum in any order: an integer, exact in fp32 (and as fp16 operands' products)
            worst = max(worst, int(absd.max()))
            for alpha, beta, mul_s in T.EPILOGUES:
                res = T.int_result(name, k, alpha, beta, mul_s)
                t = alpha * d.astype(np.float64)  # the intermediate alpha * d and beta * s: exact in fp32
                for q in (t, beta * s.astype(np.float64), res):
                    np.testing.assert_array_equal(q.astype(np.float32).astype(np.float64), q)
                with np.errstate(over="raise"):
                    np.testing.assert_array_equal(res.astype(np.float16).astype(np.float64), res, err_msg="%s k=%d %s" % (name, k, (alpha, beta, mul_s)))
    assert 0 < worst < 2 ** 24


def test_integer_cases_cover_every_parameter():
    import test_sddmm as T
    cases = T.int_cases()
    assert len(cases) + 400 < 1500  # the file stays small
    for pos, values in ((0, T.NAMES), (1, (0, 1, 2)), (2, T.KS), (3, (0, 1)), (4, (0, 1)), (5, T.LDKINDS), (6, T.LDKINDS), (7, T.KERNELS),
                        (8, T.LANES), (9, tuple(range(len(T.EPILOGUES))))):
        assert {c[pos] for c in cases} == set(values), pos
    # every kernel switch meets every dtype with aligned and with misaligned leading dimensions, and both layout pairs that flip
    big = [c for c in cases if c[0] in ("banded", "random", "rmat", "dense")]
    for dtype in (0, 1, 2):
        es = (4, 2, 8)[dtype]
        for kern in T.KERNELS:
            al = {((T.ld_of(c[2], c[5]) * es) % 16 == 0 and (T.ld_of(c[2], c[6]) * es) % 16 == 0) for c in big if c[1] == dtype and c[7] == kern}
            assert al == {True, False}, (dtype, kern)
            assert {(c[3], c[4]) for c in big if c[1] == dtype and c[7] == kern} == {(0, 0), (0, 1), (1, 0), (1, 1)}, (dtype, kern)
        for lanes in T.LANES:
            assert {c[0] for c in big if c[1] == dtype and c[8] == lanes} == {"banded", "random", "rmat", "dense"}, (dtype, lanes)
    # a k tail, a single step and several steps of both matrix-core kernels
    assert {1, 31, 32, 33, 100} <= {c[2] for c in big if c[1] in (0, 1) and c[7] == "tile"}


def test_the_patterns_reach_their_branches():
    import test_sddmm as T
    T.test_the_patterns_are_what_the_cases_need()
