"""CPU tests of the transpose / layout-conversion surface: the three C entry points refuse null handles and bad layout flags with
BMSP_ERR_INVALID and say why, and the C++ wrappers (bmSpMatrix<T>::transpose / with_layout) compile and link against libbmsp.so."""
import ctypes as C
import os
import subprocess
import pytest
from conftest import REPO

BMSP_ERR_INVALID = -1


def build_cpp_transpose_check(out_path):
    lib_dir = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp_transpose_check.cpp"), "-o", out_path, "-L" + lib_dir, "-lbmsp",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def _status_and_message(bmsp, status):
    return status, bmsp.lib().bmsp_last_error().decode(errors="replace")


@pytest.mark.parametrize("fn", ["bmsp_matrix_transpose", "bmsp_matrix_convert_layout"])
def test_transpose_and_convert_reject_null_and_bad_flags(bmsp, fn):
    L = bmsp.lib()
    out = C.c_void_p()
    st, msg = _status_and_message(bmsp, getattr(L, fn)(None, 0, None, C.byref(out)))
    assert st == BMSP_ERR_INVALID and "null" in msg, msg
    assert out.value is None
    for flag in (2, -1, 7):
        st, msg = _status_and_message(bmsp, getattr(L, fn)(None, flag, None, C.byref(out)))
        assert st == BMSP_ERR_INVALID and "out_transposed" in msg, msg
    # a null output pointer
    st, msg = _status_and_message(bmsp, getattr(L, fn)(None, 1, None, None))
    assert st == BMSP_ERR_INVALID and "null" in msg, msg


def test_copy_values_rejects_null_handles(bmsp):
    L = bmsp.lib()
    st, msg = _status_and_message(bmsp, L.bmsp_matrix_copy_values(None, None, None))
    assert st == BMSP_ERR_INVALID and "null" in msg, msg


def test_python_wrappers_exist(bmsp):
    for name in ("transpose", "with_layout", "copy_values_from"):
        assert callable(getattr(bmsp.BmSpMatrix, name))


def test_cpp_transpose_wrappers_compile_and_link(tmp_path):
    """include/bmSpMatrix.h with transpose() / with_layout() instantiated for float and half links against libbmsp.so with a plain
    host compiler."""
    build_cpp_transpose_check(str(tmp_path / "cpp_transpose_check"))
