"""CPU tests of the sparse-addition surface: the two C entry points refuse null handles and bad layout flags with BMSP_ERR_INVALID and
say why, the wrappers exist, the C++ wrappers (bmSparse_add / bmSparse_add_values) compile and link against libbmsp.so, and the value
pass in the gfx950 assembly has no contracted multiply-add and no scratch."""
import ctypes as C
import os
import re
import subprocess
import pytest
from conftest import REPO

BMSP_ERR_INVALID = -1


def build_cpp_add_check(out_path):
    lib_dir = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp_add_check.cpp"), "-o", out_path, "-L" + lib_dir, "-lbmsp",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def _status_and_message(bmsp, status):
    return status, bmsp.lib().bmsp_last_error().decode(errors="replace")


def test_add_rejects_null_handles_and_bad_flags(bmsp):
    L = bmsp.lib()
    out = C.c_void_p()
    st, msg = _status_and_message(bmsp, L.bmsp_matrix_add(1.0, None, 1.0, None, 0, None, C.byref(out)))
    assert st == BMSP_ERR_INVALID and "null" in msg and "A" in msg, msg
    assert out.value is None
    for flag in (2, -1, 7):
        st, msg = _status_and_message(bmsp, L.bmsp_matrix_add(1.0, None, 1.0, None, flag, None, C.byref(out)))
        assert st == BMSP_ERR_INVALID and "out_transposed" in msg, msg
    st, msg = _status_and_message(bmsp, L.bmsp_matrix_add(1.0, None, 1.0, None, 1, None, None))
    assert st == BMSP_ERR_INVALID and "null" in msg, msg


def test_add_values_rejects_null_handles(bmsp):
    L = bmsp.lib()
    st, msg = _status_and_message(bmsp, L.bmsp_matrix_add_values(1.0, None, 1.0, None, None, None))
    assert st == BMSP_ERR_INVALID and "null" in msg, msg


def test_add_symbols_are_declared(bmsp):
    for name in ("bmsp_matrix_add", "bmsp_matrix_add_values"):
        assert name in bmsp.SYMBOLS and hasattr(bmsp.lib(), name)
    with open(os.path.join(REPO, "include", "bmsp.h")) as f:
        text = f.read()
    assert "int bmsp_matrix_add(double alpha" in text and "int bmsp_matrix_add_values(double alpha" in text


def test_python_wrappers_exist(bmsp):
    assert callable(bmsp.add) and callable(bmsp.add_values)


def test_cpp_add_wrappers_compile_and_link(tmp_path):
    """include/bmSpMatrix.h with bmSparse_add / bmSparse_add_values instantiated for float and half links against libbmsp.so with a
    plain host compiler."""
    build_cpp_add_check(str(tmp_path / "cpp_add_check"))


# ---------------------------------------------------------------------------------------------------------
# the value pass in the assembly
# ---------------------------------------------------------------------------------------------------------
FMA = re.compile(r"^\s*v_(pk_)?(fma|fmac|mad|mac)_(f|mix|legacy)\w*\s")  # floating point only: v_mad_u64_u32 is address arithmetic
ARITH = {"It": ("v_mul_f32", "v_add_f32"), "If": ("v_mul_f32", "v_add_f32"), "Id": ("v_mul_f64", "v_add_f64")}


@pytest.fixture(scope="module")
def add_asm(tmp_path_factory):
    from test_fold_handoff_asm import to_asm, functions
    d = str(tmp_path_factory.mktemp("add_asm"))
    fns = functions(to_asm("add", d))
    kernels = {n: body for n, body in fns.items() if "17add_values_kernel" in n}
    with open(os.path.join(d, "add.s")) as f:
        text = f.read()
    return kernels, text


def test_value_pass_is_not_contracted(add_asm):
    """all six instantiations (fp16 / fp32 / fp64 storage x 1 / 8 lanes per tile) multiply and add with separate roundings"""
    kernels, _ = add_asm
    assert len(kernels) == 6, sorted(kernels)
    for name, body in kernels.items():
        fused = [ln.strip() for ln in body if FMA.match(ln)]
        assert not fused, (name, fused)
        mul, add = next(v for k, v in ARITH.items() if "17add_values_kernel" + k in name)
        assert any(ln.strip().startswith(mul) for ln in body), (name, mul)
        assert any(ln.strip().startswith(add) for ln in body), (name, add)


def test_add_kernels_use_no_scratch(add_asm):
    _, text = add_asm
    sizes = re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text)
    assert sizes and all(int(s) == 0 for s in sizes), sizes
    # subnormals are kept: fp32 and fp16 / fp64 denormal modes both "preserve" (3) in every kernel
    assert set(re.findall(r"\.amdhsa_float_denorm_mode_32\s+(\d+)", text)) == {"3"}
    assert set(re.findall(r"\.amdhsa_float_denorm_mode_16_64\s+(\d+)", text)) == {"3"}
