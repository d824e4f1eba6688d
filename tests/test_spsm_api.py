"""CPU tests of the surface of bmsp_spsm (the triangular solve for k right-hand sides): the prototypes and the struct in bmsp.h, the
layout of bmsp_spsm_info, the refusals that need no matrix (scalars before handles, the argument named), the argument checks of the
Python wrappers, the C++ wrappers (compile + link), and the gfx950 assembly of spsm.hip: every instantiation of both kernels, no private
memory, fused multiply-adds in all of them, the division sequence in the non-unit ones.  The refusals that need a matrix on the device
are in tests/test_spsm.py."""
import ctypes as C
import inspect
import os
import re
import subprocess
import pytest
from conftest import REPO
from test_spsv_api import _flat, _msg, FMA

BMSP_ERR_INVALID = -1
WIDTHS = (8, 16, 32, 64)


# ---------------------------------------------------------------------------------------------------------
# the header and the bindings
# ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_interface_verbatim(bmsp):
    hdr = _flat(open(os.path.join(REPO, "include", "bmsp.h")).read())
    for line in ("int bmsp_spsm(bmsp_matrix_t A, int op, int fill, int diag, double alpha, const void *d_B, int64_t ldb, void *d_X, int64_t ldx, "
                 "int k, void *stream);",
                 "typedef struct { char kernel[64]; int lanes, col_chunks; int64_t levels, launches, chain_launches, chained_levels, plan_bytes; } "
                 "bmsp_spsm_info;",
                 "int bmsp_spsm_launch_info(bmsp_matrix_t A, int op, int fill, int diag, int k, int64_t ldb, int64_t ldx, void *stream, "
                 "bmsp_spsm_info *info);"):
        assert _flat(line) in hdr, line
    for name in ("bmsp_spsm", "bmsp_spsm_launch_info"):
        assert name in bmsp.SYMBOLS and hasattr(bmsp.lib(), name)


def test_info_layout_and_wrappers(bmsp):
    I = bmsp.SpsmInfo
    assert [f[0] for f in I._fields_] == ["kernel", "lanes", "col_chunks", "levels", "launches", "chain_launches", "chained_levels", "plan_bytes"]
    assert C.sizeof(I) == 64 + 2 * 4 + 5 * 8
    assert (I.lanes.offset, I.col_chunks.offset, I.levels.offset, I.plan_bytes.offset) == (64, 68, 72, 104)
    assert set(I().as_dict()) == {f[0] for f in I._fields_}
    assert list(inspect.signature(bmsp.spsm).parameters) == ["A", "B", "k", "op", "fill", "unit_diag", "alpha", "X", "ldb", "ldx", "stream"]
    assert list(inspect.signature(bmsp.spsm_launch_info).parameters) == ["A", "op", "fill", "k", "unit_diag", "ldb", "ldx", "stream"]
    assert list(inspect.signature(bmsp.BmSpMatrix.solve_triangular_multi).parameters)[:3] == ["self", "B", "k"]
    assert callable(bmsp.BmSpMatrix.solve_triangular)        # the single-vector solve stays


# ---------------------------------------------------------------------------------------------------------
# refusals that need no matrix
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture()
def buf():
    """a host buffer standing in for a device array: the calls under test refuse before they touch it"""
    b = (C.c_float * 64)()
    return C.addressof(b)


def test_scalars_are_refused_before_handles_and_named(bmsp, buf):
    L = bmsp.lib()
    info = bmsp.SpsmInfo()

    def both(op, fill, diag, k, ldb, ldx, word):
        assert L.bmsp_spsm(None, op, fill, diag, 1.0, buf, ldb, buf, ldx, k, None) == BMSP_ERR_INVALID
        assert _msg(bmsp).startswith(word), ((op, fill, diag, k, ldb, ldx), _msg(bmsp))
        assert L.bmsp_spsm(None, op, fill, diag, 1.0, None, ldb, None, ldx, k, None) == BMSP_ERR_INVALID
        assert _msg(bmsp).startswith(word), ((op, fill, diag, k, ldb, ldx), _msg(bmsp))
        assert L.bmsp_spsm_launch_info(None, op, fill, diag, k, ldb, ldx, None, C.byref(info)) == BMSP_ERR_INVALID
        assert _msg(bmsp).startswith(word), ((op, fill, diag, k, ldb, ldx), _msg(bmsp))
        assert L.bmsp_spsm_launch_info(None, op, fill, diag, k, ldb, ldx, None, None) == BMSP_ERR_INVALID
        assert _msg(bmsp).startswith(word), ((op, fill, diag, k, ldb, ldx), _msg(bmsp))

    for args, word in (((2, 0, 0), "op"), ((-1, 0, 0), "op"), ((0, 2, 0), "fill"), ((1, -1, 0), "fill"), ((0, 0, 2), "diag"),
                       ((1, 1, -1), "diag")):
        both(*args, 4, 4, 4, word)
    both(0, 0, 0, 0, 4, 4, "k")
    both(1, 1, 1, -3, 4, 4, "k")
    both(0, 0, 0, 5, 4, 5, "ldb")
    both(0, 0, 0, 5, 5, 4, "ldx")
    both(0, 0, 0, 5, 4, 4, "ldb")          # both too small: the first in the argument list is named
    both(2, 0, 0, 0, 0, 0, "op")           # and op before k
    # a bad scalar is named although the handle is null too; with good scalars the handle is
    assert L.bmsp_spsm(None, 0, 0, 0, 1.0, buf, 7, buf, 6, 5, None) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)
    assert L.bmsp_spsm(None, 1, 1, 1, 1.0, None, 1, None, 1, 1, None) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)
    assert L.bmsp_spsm_launch_info(None, 0, 0, 0, 5, 7, 6, None, C.byref(info)) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)
    assert L.bmsp_spsm_launch_info(None, 0, 0, 0, 5, 7, 6, None, None) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)


def test_python_wrappers_check_their_arguments(bmsp):
    """what the wrappers refuse before they look at the matrix (None stands in for it)"""
    for fn in (lambda **kw: bmsp.spsm(None, None, **kw), lambda **kw: bmsp.spsm_launch_info(None, kw.pop("op", "N"), kw.pop("fill", "lower"), **kw)):
        with pytest.raises(ValueError, match="op must be"):
            fn(k=4, op="X")
        with pytest.raises(ValueError, match="fill must be"):
            fn(k=4, fill="diagonal")
        with pytest.raises(ValueError, match="k must be >= 1"):
            fn(k=0)
        with pytest.raises(ValueError, match="ldb and ldx must be >= k"):
            fn(k=4, ldb=3)
        with pytest.raises(ValueError, match="ldb and ldx must be >= k"):
            fn(k=4, ldx=2)


# ---------------------------------------------------------------------------------------------------------
# the C++ wrappers
# ---------------------------------------------------------------------------------------------------------
def build_cpp_spsm_check(out_path):
    lib_dir = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp_spsm_check.cpp"), "-o", out_path, "-L" + lib_dir, "-lbmsp",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_spsm_wrappers_compile_and_link(bmsp, tmp_path):
    """include/bmSpMatrix.h with bmSparse_SpSM / bmSparse_SpSM_launch_info instantiated for float, half and double links against
    libbmsp.so with a plain host compiler."""
    build_cpp_spsm_check(str(tmp_path / "cpp_spsm_check"))


# ---------------------------------------------------------------------------------------------------------
# the kernels in the assembly
# ---------------------------------------------------------------------------------------------------------
FRAGS = ("17spsm_level_kernel", "17spsm_chain_kernel")
FMA_F16 = re.compile(r"\s*v_(fma|fmac|fma_mix)_f32")


@pytest.fixture(scope="module")
def spsm_asm(tmp_path_factory):
    from test_fold_handoff_asm import to_asm, functions
    path = to_asm("spsm", str(tmp_path_factory.mktemp("spsm_asm")))
    return functions(path), open(path).read()


def _targs(s, minor, lower, unit, w):
    """the mangled template arguments <S, MINOR, LOWER, UNIT, W>"""
    return "I%sLb%dELb%dELb%dELi%dEE" % ({0: "f", 1: "t", 2: "d"}[s], minor, lower, unit, w)


def test_every_instantiation_is_in_the_assembly(spsm_asm):
    fns, _ = spsm_asm
    for frag in FRAGS:
        ks = {n: b for n, b in fns.items() if frag in n}
        assert len(ks) == 3 * 2 * 2 * 2 * len(WIDTHS), sorted(ks)
        for s in (0, 1, 2):
            for minor in (0, 1):
                for lower in (0, 1):
                    for unit in (0, 1):
                        for w in WIDTHS:
                            assert sum(frag + _targs(s, minor, lower, unit, w) in n for n in ks) == 1, (frag, s, minor, lower, unit, w)


def test_no_kernel_uses_private_memory(spsm_asm):
    _, text = spsm_asm
    meta = text[text.index("amdhsa.kernels:"):]
    # (a kernel's keys are listed in alphabetical order: .name stands right before .private_segment_fixed_size)
    seen = {n: int(v) for n, v in re.findall(r"^    \.name:\s+(\S+)\n    \.private_segment_fixed_size:\s+(\d+)$", meta, re.M)}
    assert len(seen) == meta.count(".private_segment_fixed_size:")
    ours = {n: v for n, v in seen.items() if "spsm_" in n}
    assert len(ours) == 2 * 3 * 2 * 2 * 2 * len(WIDTHS), len(ours)      # both kernels; `seen` holds the plan's passes and the warm-up too
    assert all(v == 0 for v in seen.values()), {n: v for n, v in seen.items() if v}


def test_division_sequence_and_fused_multiply_adds(spsm_asm):
    fns, _ = spsm_asm
    for frag in FRAGS:
        for name, body in fns.items():
            if frag not in name:
                continue
            # F16 kernels: the compiler folds the exact widening of a stored half into the multiply-add itself, v_fma_mix_f32 -- the same
            # fp32 fused multiply-add with the conversion inside the instruction; under a unit diagonal it is the only kind they hold
            fma = FMA_F16 if "kernelIt" in name else FMA
            assert any(fma.match(ln) for ln in body), name
            ops = [ln.split()[0] for ln in body if ln.strip()]
            unit = re.search(r"Lb[01]ELb[01]ELb1ELi\d+EE", name) is not None
            div = [o for o in ops if o.startswith("v_div_") or o.startswith("v_rcp")]
            if unit:
                assert not div, (name, div[:4])          # x_i = s: nothing divides
                continue
            scale = sum(o.startswith("v_div_scale") for o in ops)
            fmas = sum(o.startswith("v_div_fmas") for o in ops)
            fixup = sum(o.startswith("v_div_fixup") for o in ops)
            rcp = sum(o.startswith("v_rcp") for o in ops)
            assert fixup >= 1 and fmas == fixup and scale == 2 * fixup, (name, scale, fmas, fixup)
            # a reciprocal only ever seeds a division sequence: one per sequence
            assert rcp == fixup, (name, rcp, fixup)
