"""CPU tests of the diagonal operations' surface: the four C entry points refuse bad scalar arguments and null pointers with
BMSP_ERR_INVALID and name the argument, scalars before handles, all before any device call; the symbols are exported and declared; the
Python and C++ wrappers exist and link; and the gfx950 assembly of diag.hip uses no scratch, keeps subnormals, holds no atomic of any
kind, divides with the full IEEE sequence (every reciprocal is followed by its v_div_fixup) and carries no division in the multiply-only
variants."""
import ctypes as C
import os
import re
import subprocess
import pytest
from conftest import REPO

BMSP_ERR_INVALID = -1


def build_cpp_diag_check(out_path):
    lib_dir = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp_diag_check.cpp"), "-o", out_path, "-L" + lib_dir, "-lbmsp",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def _msg(bmsp):
    return bmsp.lib().bmsp_last_error().decode(errors="replace")


def _scale(bmsp, A, l, r, flags, lay, out=True):
    h = C.c_void_p()
    rc = bmsp.lib().bmsp_matrix_scale(A, l, r, flags, lay, None, C.byref(h) if out else None)
    return rc, _msg(bmsp), h


def _from_diagonal(bmsp, nr, nc, d, dtype, lay, out=True):
    h = C.c_void_p()
    rc = bmsp.lib().bmsp_matrix_from_diagonal(nr, nc, d, dtype, lay, None, C.byref(h) if out else None)
    return rc, _msg(bmsp), h


@pytest.fixture()
def vec():
    """a host buffer standing in for a device vector: the calls under test refuse before they touch it"""
    buf = (C.c_float * 16)()
    return C.addressof(buf), buf


# ---------------------------------------------------------------------------------------------------------
# refusals through the raw C calls, null handles
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [4, 8, 7, -1, 1 << 16])
def test_scale_rejects_unknown_flags(bmsp, vec, flags):
    rc, msg, h = _scale(bmsp, None, vec[0], vec[0], flags, 0)
    assert rc == BMSP_ERR_INVALID and "flags" in msg, msg
    assert h.value is None
    rc = bmsp.lib().bmsp_matrix_scale_values(None, vec[0], vec[0], flags, None, None)
    assert rc == BMSP_ERR_INVALID and "flags" in _msg(bmsp), _msg(bmsp)


@pytest.mark.parametrize("lay", [2, -1, 7])
def test_scale_rejects_bad_layout(bmsp, vec, lay):
    rc, msg, _ = _scale(bmsp, None, vec[0], None, 0, lay)
    assert rc == BMSP_ERR_INVALID and "out_transposed" in msg, msg


@pytest.mark.parametrize("flags,l,r,word", [(1, False, True, "d_left"), (2, True, False, "d_right"), (3, True, False, "d_right"),
                                            (3, False, True, "d_left"), (1, False, False, "d_left"), (2, False, False, "d_right")])
def test_div_flag_needs_its_vector(bmsp, vec, flags, l, r, word):
    lp, rp = (vec[0] if l else None), (vec[0] if r else None)
    rc, msg, _ = _scale(bmsp, None, lp, rp, flags, 0)
    assert rc == BMSP_ERR_INVALID and word in msg and "null" in msg, msg
    rc = bmsp.lib().bmsp_matrix_scale_values(None, lp, rp, flags, None, None)
    assert rc == BMSP_ERR_INVALID and word in _msg(bmsp) and "null" in _msg(bmsp), _msg(bmsp)


def test_scale_rejects_null_handles_after_the_scalars(bmsp, vec):
    """legal scalars (every flag with its vector, both sides null without flags): the call gets as far as the handle check"""
    for flags, lp, rp in ((0, None, None), (0, vec[0], None), (1, vec[0], None), (2, None, vec[0]), (3, vec[0], vec[0])):
        for lay in (0, 1):
            rc, msg, h = _scale(bmsp, None, lp, rp, flags, lay)
            assert rc == BMSP_ERR_INVALID and "null" in msg and "A" in msg and "flags" not in msg, msg
            assert h.value is None
        rc = bmsp.lib().bmsp_matrix_scale_values(None, lp, rp, flags, None, None)
        assert rc == BMSP_ERR_INVALID and "null" in _msg(bmsp) and "A" in _msg(bmsp), _msg(bmsp)


def test_diagonal_rejects_null_arguments(bmsp, vec):
    L = bmsp.lib()
    assert L.bmsp_matrix_diagonal(None, None, None) == BMSP_ERR_INVALID
    assert "null" in _msg(bmsp) and "A" in _msg(bmsp), _msg(bmsp)
    assert L.bmsp_matrix_diagonal(None, vec[0], None) == BMSP_ERR_INVALID
    assert "null" in _msg(bmsp) and "A" in _msg(bmsp), _msg(bmsp)


@pytest.mark.parametrize("nr,nc", [(-1, 4), (4, -1), (-3, -3), (-1, 0)])
def test_from_diagonal_rejects_negative_dimensions(bmsp, vec, nr, nc):
    rc, msg, h = _from_diagonal(bmsp, nr, nc, vec[0], 0, 0)
    assert rc == BMSP_ERR_INVALID and "num_rows" in msg and "num_cols" in msg, msg
    assert h.value is None


@pytest.mark.parametrize("dtype", [3, -1, 17])
def test_from_diagonal_rejects_unknown_dtype(bmsp, vec, dtype):
    rc, msg, _ = _from_diagonal(bmsp, 4, 4, vec[0], dtype, 0)
    assert rc == BMSP_ERR_INVALID and "dtype" in msg, msg


@pytest.mark.parametrize("lay", [2, -1, 7])
def test_from_diagonal_rejects_bad_layout(bmsp, vec, lay):
    rc, msg, _ = _from_diagonal(bmsp, 4, 4, vec[0], 0, lay)
    assert rc == BMSP_ERR_INVALID and "transposed" in msg, msg


def test_from_diagonal_rejects_null_vector_and_null_output(bmsp, vec):
    for nr, nc in ((4, 4), (1, 9), (9, 1)):
        rc, msg, _ = _from_diagonal(bmsp, nr, nc, None, 0, 0)
        assert rc == BMSP_ERR_INVALID and "d_diag" in msg and "null" in msg, msg
    # an empty diagonal needs no vector: the call gets as far as the output pointer
    for nr, nc, d in ((0, 5, None), (5, 0, None), (0, 0, None), (4, 4, vec[0])):
        rc, msg, _ = _from_diagonal(bmsp, nr, nc, d, 0, 0, out=False)
        assert rc == BMSP_ERR_INVALID and "out" in msg and "null" in msg and "d_diag" not in msg, msg


# ---------------------------------------------------------------------------------------------------------
# symbols and wrappers
# ---------------------------------------------------------------------------------------------------------
def test_diag_symbols_are_declared(bmsp):
    for name in ("bmsp_matrix_diagonal", "bmsp_matrix_from_diagonal", "bmsp_matrix_scale", "bmsp_matrix_scale_values"):
        assert name in bmsp.SYMBOLS and hasattr(bmsp.lib(), name)
    with open(os.path.join(REPO, "include", "bmsp.h")) as f:
        text = f.read()
    assert "int bmsp_matrix_diagonal(bmsp_matrix_t A, void *d_diag, void *stream);" in text
    assert "int bmsp_matrix_from_diagonal(int num_rows, int num_cols, const void *d_diag, bmsp_dtype dtype, int transposed," in text
    assert "int bmsp_matrix_scale(bmsp_matrix_t A, const void *d_left, const void *d_right, int flags, int out_transposed," in text
    assert "int bmsp_matrix_scale_values(bmsp_matrix_t A, const void *d_left, const void *d_right, int flags, bmsp_matrix_t out," in text
    for word in ("#define BMSP_SCALE_DIV_LEFT  1", "#define BMSP_SCALE_DIV_RIGHT 2"):
        assert word in text, word


def test_python_wrappers_exist(bmsp):
    for fn in (bmsp.diagonal, bmsp.from_diagonal, bmsp.scale, bmsp.scale_values, bmsp.BmSpMatrix.diagonal, bmsp.BmSpMatrix.scale,
               bmsp.BmSpMatrix.scale_, bmsp.BmSpMatrix.from_diagonal):
        assert callable(fn)
    assert (bmsp.SCALE_DIV_LEFT, bmsp.SCALE_DIV_RIGHT) == (1, 2)


def test_cpp_diag_wrappers_compile_and_link(tmp_path):
    """include/bmSpMatrix.h with ::diagonal / ::scale / ::scale_inplace and the bmSparse_* free functions instantiated for float, half
    and double links against libbmsp.so with a plain host compiler."""
    build_cpp_diag_check(str(tmp_path / "cpp_diag_check"))


# ---------------------------------------------------------------------------------------------------------
# the kernels in the assembly
# ---------------------------------------------------------------------------------------------------------
DTYPES = {"f": ("v_rcp_f32", "v_div_fixup_f32"), "t": ("v_rcp_f32", "v_div_fixup_f32"), "d": ("v_rcp_f64", "v_div_fixup_f64")}


@pytest.fixture(scope="module")
def diag_asm(tmp_path_factory):
    from test_fold_handoff_asm import to_asm, functions
    d = str(tmp_path_factory.mktemp("diag_asm"))
    fns = functions(to_asm("diag", d))
    with open(os.path.join(d, "diag.s")) as f:
        text = f.read()
    return fns, text


def _scale_kernels(fns):
    """{(dtype letter, lanes, div left, div right): instruction lines} of scale_values_kernel<S, G, DL, DR>"""
    out = {}
    for name, body in fns.items():
        m = re.search(r"19scale_values_kernelI([ftd])Li([18])ELb([01])ELb([01])E", name)
        if m:
            out[(m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)))] = body
    return out


def _count(body, op):
    return sum(bool(re.match(r"\s*" + op + r"(_e32|_e64|_dpp|_sdwa)?\s", ln)) for ln in body)


def _has(body, op):
    return _count(body, op) > 0


def test_diag_kernels_are_all_there(diag_asm):
    """three dtypes x two lane groups x {multiply, divide} per side of the value pass; three dtypes of the two for_each passes"""
    fns, _ = diag_asm
    ks = _scale_kernels(fns)
    assert sorted(ks) == sorted((d, g, dl, dr) for d in "ftd" for g in (1, 8) for dl in (0, 1) for dr in (0, 1)), sorted(ks)
    for frag in ("12ReadDiagonalI", "12MakeDiagonalI"):
        assert len([n for n in fns if "for_each_kernel" in n and frag in n]) == 3, (frag, sorted(fns))
    assert len([n for n in fns if "for_each_kernel" in n and "13CopyStructure" in n]) == 1, sorted(fns)


def test_diag_kernels_use_no_scratch_and_keep_subnormals(diag_asm):
    _, text = diag_asm
    sizes = re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text)
    assert sizes and all(int(s) == 0 for s in sizes), sizes
    assert set(re.findall(r"\.amdhsa_float_denorm_mode_32\s+(\d+)", text)) == {"3"}
    assert set(re.findall(r"\.amdhsa_float_denorm_mode_16_64\s+(\d+)", text)) == {"3"}


def test_diag_has_no_atomics(diag_asm):
    """every output element has one writer: no atomic instruction of any kind in the assembly, no atomic call in the source"""
    fns, text = diag_asm
    atomics = set(re.findall(r"^\s*(\w*atomic\w*|ds_(?:add|sub|max|min|and|or|xor|inc|dec|cmpst|wrxchg|pk_add)_\w+)\s", text, re.M))
    assert not atomics, atomics
    with open(os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "csrc", "diag.hip")) as f:
        src = f.read()
    code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
    assert not re.findall(r"\b(atomic\w*|unsafeAtomic\w+|__hip_atomic\w+|__builtin_amdgcn_\w*atomic\w*)\s*\(", code)


def test_division_is_the_ieee_sequence_and_only_where_asked(diag_asm):
    fns, _ = diag_asm
    # wherever a reciprocal appears, in any function of the file, the fixup of the same precision closes the sequence
    for name, body in fns.items():
        for rcp, fix in set(DTYPES.values()):
            if _has(body, rcp):
                assert _has(body, fix) and _has(body, fix.replace("fixup", "fmas")) and _has(body, fix.replace("fixup", "scale")), name
    ks = _scale_kernels(fns)
    for (d, g, dl, dr), body in ks.items():
        rcp, fix = DTYPES[d]
        if dl or dr:
            assert _has(body, fix) and _has(body, rcp), (d, g, dl, dr)
            assert _count(body, fix) >= dl + dr, (d, g, dl, dr, _count(body, fix))
        else:  # the multiply-only instantiations hold neither
            assert not any(re.match(r"\s*v_(rcp|div_fixup|div_fmas|div_scale)_", ln) for ln in body), (d, g)
            assert _has(body, "v_mul_f64" if d == "d" else "v_mul_f32"), (d, g)
    for d in "ftd":  # at least one function per precision holds the fixup
        assert any(_has(body, DTYPES[d][1]) for (dd, _, _, _), body in ks.items() if dd == d)


def test_products_are_not_fused(diag_asm):
    """the two factors are applied one after the other, each rounded: nothing to contract, and no fma outside a division sequence"""
    fns, _ = diag_asm
    for (d, g, dl, dr), body in _scale_kernels(fns).items():
        if not (dl or dr):
            assert not any(re.match(r"\s*v_(pk_)?(fma|fmac|mad|mac)_(f16|f32|f64|legacy)", ln) for ln in body), (d, g)
