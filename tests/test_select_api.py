"""CPU tests of the selection surface: the two C entry points refuse bad scalar arguments, null outputs and null handles with
BMSP_ERR_INVALID and name the argument, the scalars before the handles and all before any device call; every pair of int64 band bounds
is legal; the symbols are exported and declared; the Python and C++ wrappers exist and link; the bit helpers of the band (bmsp_bits.h)
agree with brute force on the host; and the gfx950 assembly of select.hip holds both mark kernels and uses no scratch."""
import ctypes as C
import os
import re
import subprocess
import pytest
from conftest import REPO

BMSP_ERR_INVALID = -1
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def build_cpp_select_check(out_path):
    lib_dir = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp_select_check.cpp"), "-o", out_path, "-L" + lib_dir, "-lbmsp",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def _band(bmsp, A, lo, hi, flags, lay, out=True, stats=True):
    """(status, message, out handle) of one raw bmsp_matrix_select_band call"""
    h, st = C.c_void_p(), bmsp.SelectStats()
    rc = bmsp.lib().bmsp_matrix_select_band(A, lo, hi, flags, lay, None, C.byref(h) if out else None, C.byref(st) if stats else None)
    return rc, bmsp.lib().bmsp_last_error().decode(errors="replace"), h


def _mask(bmsp, A, M, flags, lay, out=True, stats=True):
    h, st = C.c_void_p(), bmsp.SelectStats()
    rc = bmsp.lib().bmsp_matrix_select_mask(A, M, flags, lay, None, C.byref(h) if out else None, C.byref(st) if stats else None)
    return rc, bmsp.lib().bmsp_last_error().decode(errors="replace"), h


def _calls(bmsp, flags, lay, out=True, stats=True):
    """both entry points with null handles and these scalars"""
    return [_band(bmsp, None, -1, 1, flags, lay, out, stats), _mask(bmsp, None, None, flags, lay, out, stats)]


def test_select_rejects_null_handles(bmsp):
    for rc, msg, h in _calls(bmsp, 0, 0) + _calls(bmsp, 1, 1, out=False):
        assert rc == BMSP_ERR_INVALID and "null" in msg and "A" in msg, msg
        assert h.value is None
    # a live-looking A with a null M: M is named (the handle is never dereferenced: the check comes first)
    dummy = C.c_void_p(C.addressof(C.create_string_buffer(8)))
    rc, msg, _ = _mask(bmsp, dummy, None, 0, 0)
    assert rc == BMSP_ERR_INVALID and "null" in msg and "M" in msg, msg


@pytest.mark.parametrize("flags", [2, 3, -1, 1 << 16])
def test_select_rejects_unknown_flags(bmsp, flags):
    for rc, msg, _ in _calls(bmsp, flags, 0):
        assert rc == BMSP_ERR_INVALID and "flags" in msg, msg


@pytest.mark.parametrize("lay", [2, -1, 7])
def test_select_rejects_bad_layout(bmsp, lay):
    for rc, msg, _ in _calls(bmsp, 0, lay):
        assert rc == BMSP_ERR_INVALID and "out_transposed" in msg, msg


def test_select_rejects_both_outputs_null(bmsp):
    for rc, msg, _ in _calls(bmsp, 0, 0, out=False, stats=False):
        assert rc == BMSP_ERR_INVALID and "out" in msg and "stats" in msg, msg


@pytest.mark.parametrize("lo", [INT64_MIN, INT64_MAX, 1 << 62, -(1 << 62)])
@pytest.mark.parametrize("hi", [INT64_MIN, INT64_MAX, 1 << 62, -(1 << 62)])
def test_every_band_bound_is_legal(bmsp, lo, hi):
    """with a null handle the call gets as far as the handle check, whatever the bounds"""
    rc, msg, _ = _band(bmsp, None, lo, hi, 0, 0)
    assert rc == BMSP_ERR_INVALID and "null" in msg and "A" in msg, msg


def test_select_symbols_are_declared(bmsp):
    for name in ("bmsp_matrix_select_band", "bmsp_matrix_select_mask"):
        assert name in bmsp.SYMBOLS and hasattr(bmsp.lib(), name)
    with open(os.path.join(REPO, "include", "bmsp.h")) as f:
        text = f.read()
    flat = re.sub(r"\s+", " ", text)
    assert ("int bmsp_matrix_select_band(bmsp_matrix_t A, int64_t lo, int64_t hi, int flags, int out_transposed, void *stream, "
            "bmsp_matrix_t *out, bmsp_select_stats *stats);") in flat
    assert ("int bmsp_matrix_select_mask(bmsp_matrix_t A, bmsp_matrix_t M, int flags, int out_transposed, void *stream, "
            "bmsp_matrix_t *out, bmsp_select_stats *stats);") in flat
    for line in ("#define BMSP_SELECT_COMPLEMENT 1", "#define BMSP_BAND_MIN INT64_MIN", "#define BMSP_BAND_MAX INT64_MAX",
                 "typedef bmsp_prune_stats bmsp_select_stats;"):
        assert line in flat, line


def test_python_wrappers_exist(bmsp):
    for name in ("select_band", "band_count", "tril", "triu", "offdiagonal", "select_mask", "mask_count"):
        assert callable(getattr(bmsp, name)), name
    for name in ("tril", "triu", "band", "mask"):
        assert callable(getattr(bmsp.BmSpMatrix, name)), name
    assert (bmsp.SELECT_COMPLEMENT, bmsp.BAND_MIN, bmsp.BAND_MAX) == (1, INT64_MIN, INT64_MAX)
    assert bmsp.SelectStats is bmsp.PruneStats and C.sizeof(bmsp.SelectStats) == 32
    L = bmsp.lib()
    assert L.bmsp_matrix_select_band.argtypes[1:3] == [C.c_int64, C.c_int64]
    assert len(L.bmsp_matrix_select_band.argtypes) == 8 and len(L.bmsp_matrix_select_mask.argtypes) == 7


def test_cpp_select_wrappers_compile_and_link(tmp_path):
    """include/bmSpMatrix.h with ::tril / ::triu / ::band / ::mask and bmSparse_select_band / _mask instantiated for float and half
    links against libbmsp.so with a plain host compiler."""
    build_cpp_select_check(str(tmp_path / "cpp_select_check"))


def test_band_bit_helpers_on_the_host(tmp_path):
    """tile_band_mask against brute force for all dlo, dhi in [-9, 9], its mirror against tile_transpose, and the whole-tile keep / drop
    conditions against the per-entry predicate for delta in [-3, 3], lo, hi in [-30, 30] and the clamped sentinels (no HIP)."""
    exe = str(tmp_path / "host_select_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "csrc"),
                           os.path.join(REPO, "tests", "host_select_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "CHECK host select OK" in out.stdout, out.stdout[-2000:] + out.stderr


# ---------------------------------------------------------------------------------------------------------
# the kernels in the assembly
# ---------------------------------------------------------------------------------------------------------
def test_select_kernels_are_there_and_use_no_scratch(tmp_path):
    from test_fold_handoff_asm import to_asm, functions
    path = to_asm("select", str(tmp_path))
    fns = functions(path)
    for frag in ("select_band_mark_kernel", "select_mask_mark_kernel"):
        assert len([n for n in fns if frag in n]) == 1, (frag, sorted(fns))
    with open(path) as f:
        text = f.read()
    sizes = re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text)
    assert len(sizes) >= 2 and all(int(s) == 0 for s in sizes), sizes
