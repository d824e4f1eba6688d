"""CPU tests of the surface of bmsp_spmv_op: the C entry points refuse a bad `op` and null pointers with BMSP_ERR_INVALID and name the
argument, scalars before handles, all before any device call; the symbols are exported and declared with their exact prototypes; the
Python and C++ wrappers exist and link; the gfx950 assembly of spmv_op.hip holds every instantiation, uses no scratch, keeps subnormals,
holds no atomic and no LDS add of any kind and no fused multiply-add in the kernels that only fold and scale; and the host part of the
item planner agrees with a numpy restatement."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from conftest import REPO

BMSP_ERR_INVALID = -1


def build_cpp_spmv_op_check(out_path):
    lib_dir = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp_spmv_op_check.cpp"), "-o", out_path, "-L" + lib_dir, "-lbmsp",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def _msg(bmsp):
    return bmsp.lib().bmsp_last_error().decode(errors="replace")


@pytest.fixture()
def vec():
    """a host buffer standing in for a device vector: the calls under test refuse before they touch it"""
    buf = (C.c_float * 16)()
    return C.addressof(buf)


# ---------------------------------------------------------------------------------------------------------
# refusals through the raw C calls, null handles
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [2, -1, 7, 1 << 16])
def test_bad_op_is_refused_before_the_handles(bmsp, vec, op):
    L = bmsp.lib()
    for a in ((None, None, None), (None, vec, vec)):
        assert L.bmsp_spmv_op(a[0], op, 1.0, a[1], 0.0, a[2], None) == BMSP_ERR_INVALID
        assert "op" in _msg(bmsp) and "null" not in _msg(bmsp), _msg(bmsp)
    info = bmsp.SpmvOpInfo()
    for ip in (None, C.byref(info)):
        assert L.bmsp_spmv_op_launch_info(None, op, ip) == BMSP_ERR_INVALID
        assert "op" in _msg(bmsp) and "null" not in _msg(bmsp), _msg(bmsp)


@pytest.mark.parametrize("op", [0, 1])
def test_null_handle_is_refused_after_the_scalars(bmsp, vec, op):
    L = bmsp.lib()
    for v, u in ((None, None), (vec, None), (None, vec), (vec, vec)):
        assert L.bmsp_spmv_op(None, op, 1.0, v, 0.0, u, None) == BMSP_ERR_INVALID
        assert "null" in _msg(bmsp) and "A" in _msg(bmsp) and "op must" not in _msg(bmsp), _msg(bmsp)
    info = bmsp.SpmvOpInfo()
    for ip in (None, C.byref(info)):
        assert L.bmsp_spmv_op_launch_info(None, op, ip) == BMSP_ERR_INVALID
        assert "null" in _msg(bmsp) and "A" in _msg(bmsp), _msg(bmsp)


def test_python_wrapper_refuses_a_bad_op(bmsp):
    for op in ("X", 2, None):
        with pytest.raises(ValueError):
            bmsp.spmv_op(None, None, op)
        with pytest.raises(ValueError):
            bmsp.spmv_op_launch_info(None, op)


# ---------------------------------------------------------------------------------------------------------
# symbols and wrappers
# ---------------------------------------------------------------------------------------------------------
def test_spmv_op_symbols_are_declared(bmsp):
    for name in ("bmsp_spmv_op", "bmsp_spmv_op_launch_info", "bmsp_spmv_op_plan_items"):
        assert name in bmsp.SYMBOLS and hasattr(bmsp.lib(), name)
    with open(os.path.join(REPO, "include", "bmsp.h")) as f:
        text = f.read()
    for line in ("#define BMSP_OP_N 0", "#define BMSP_OP_T 1",
                 "int bmsp_spmv_op(bmsp_matrix_t A, int op, double alpha, const void *d_v, double beta, void *d_u, void *stream);",
                 "typedef struct { char kernel[64]; int slots; int64_t items, split_blocks, view_bytes, compulsory_bytes; } bmsp_spmv_op_info;",
                 "int bmsp_spmv_op_launch_info(bmsp_matrix_t A, int op, bmsp_spmv_op_info *info);",
                 "int bmsp_spmv_op_plan_items(const uint32_t *ptr, int64_t blocks, int64_t split, uint32_t *items, uint32_t *folds, "
                 "int64_t *n_items,"):
        assert line in text, line
    # the ctypes mirror has the C struct's layout: 64 + int (+ padding) + four int64
    assert C.sizeof(bmsp.SpmvOpInfo) == 64 + 8 + 4 * 8 and bmsp.SpmvOpInfo.items.offset == 72


def test_python_wrappers_exist(bmsp):
    for fn in (bmsp.spmv_op, bmsp.spmv_op_launch_info, bmsp.spmv_op_plan_items, bmsp.BmSpMatrix.matvec, bmsp.BmSpMatrix.rmatvec):
        assert callable(fn)
    assert (bmsp.OP_N, bmsp.OP_T) == (0, 1)


def test_cpp_spmv_op_wrappers_compile_and_link(tmp_path):
    """include/bmSpMatrix.h with bmSparse_SpMV_op instantiated for float, half and double links against libbmsp.so with a plain host
    compiler."""
    build_cpp_spmv_op_check(str(tmp_path / "cpp_spmv_op_check"))


# ---------------------------------------------------------------------------------------------------------
# the kernels in the assembly
# ---------------------------------------------------------------------------------------------------------
FLOAT_FMA = re.compile(r"\s*v_(pk_)?(fma|fmac|mad|mac)_(f16|f32|f64|legacy)")
FLOAT_FMA_MIX = re.compile(r"\s*v_(fma|mad)_mix")


@pytest.fixture(scope="module")
def op_asm(tmp_path_factory):
    from test_fold_handoff_asm import to_asm, functions
    d = str(tmp_path_factory.mktemp("spmv_op_asm"))
    fns = functions(to_asm("spmv_op", d))
    with open(os.path.join(d, "spmv_op.s")) as f:
        text = f.read()
    return fns, text


def test_every_instantiation_is_there(op_asm):
    """sweep: 3 dtypes (t = uint16_t bits of an fp16, f, d) x MINOR x SLOTS; fold and epilogue: one per vector type"""
    fns, _ = op_asm
    sweeps = set()
    for name in fns:
        m = re.search(r"20spmv_op_sweep_kernelI([tfd])Lb([01])ELi([18])E", name)
        if m:
            sweeps.add((m.group(1), int(m.group(2)), int(m.group(3))))
    assert sweeps == {(d, mi, s) for d in "tfd" for mi in (0, 1) for s in (1, 8)}, sorted(sweeps)
    for frag in ("19spmv_op_fold_kernelI", "23spmv_op_epilogue_kernelI"):
        assert sorted(re.search(frag + r"([fd])E", n).group(1) for n in fns if frag in n) == ["d", "f"], (frag, sorted(fns))


def test_no_scratch_and_subnormals_kept(op_asm):
    _, text = op_asm
    sizes = re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text)
    assert sizes and all(int(s) == 0 for s in sizes), sizes
    assert set(re.findall(r"\.amdhsa_float_denorm_mode_32\s+(\d+)", text)) == {"3"}
    assert set(re.findall(r"\.amdhsa_float_denorm_mode_16_64\s+(\d+)", text)) == {"3"}


def test_no_atomics_and_no_lds_adds(op_asm):
    """every output has one writer and every sum a fixed order: no atomic instruction of any kind in the whole file, no LDS add, and no
    atomic call in the source"""
    _, text = op_asm
    bad = set(re.findall(r"^\s*((?:global|flat|buffer|ds)_\w*atomic\w*|ds_(?:pk_)?add_\w+)\s", text, re.M))
    assert not bad, bad
    with open(os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "csrc", "spmv_op.hip")) as f:
        src = f.read()
    code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
    assert not re.findall(r"\b(atomic\w*|unsafeAtomic\w+|__hip_atomic\w+|__builtin_amdgcn_\w*atomic\w*)\s*\(", code)


def test_fold_and_epilogue_are_not_fused(op_asm):
    """the kernels that only add partial sums and apply the epilogue hold separate multiplies and adds: nothing there may contract"""
    fns, _ = op_asm
    seen = 0
    for name, body in fns.items():
        m = re.search(r"(?:19spmv_op_fold_kernel|23spmv_op_epilogue_kernel)I([fd])E", name)
        if not m:
            continue
        seen += 1
        assert not [ln for ln in body if FLOAT_FMA.match(ln) or FLOAT_FMA_MIX.match(ln)], name
        for op in (("v_mul_f64", "v_add_f64") if m.group(1) == "d" else ("v_mul_f32", "v_add_f32")):
            assert any(re.match(r"\s*" + op + r"(_e32|_e64)?\s", ln) for ln in body), (name, op)
    assert seen == 4


# ---------------------------------------------------------------------------------------------------------
# the item planner, host only
# ---------------------------------------------------------------------------------------------------------
def plan_ref(ptr, split):
    """numpy restatement: a block of n <= split tiles is one item with slot ~0; a longer one gets ceil(n / split) items with consecutive
    slots and one fold {block, first slot, parts}"""
    items, folds, slot = [], [], 0
    for b in range(len(ptr) - 1):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        if hi - lo <= split:
            items.append((b, lo, hi, 0xFFFFFFFF))
            continue
        parts = -(-(hi - lo) // split)
        folds.append((b, slot, parts))
        for k in range(parts):
            items.append((b, lo + k * split, min(lo + (k + 1) * split, hi), slot))
            slot += 1
    return (np.array(items, np.uint32).reshape(-1, 4), np.array(folds, np.uint32).reshape(-1, 3), slot)


PLANS = {
    "no_blocks": ([0], 4),
    "all_empty": ([0, 0, 0, 0], 4),
    "empty_between": ([0, 0, 3, 3, 3, 7, 7], 4),
    "exactly_split": ([0, 4, 8], 4),
    "split_plus_one": ([0, 5, 10, 11], 4),
    "one_giant": ([0, 100003], 256),
    "giant_among_small": ([0, 1, 1, 2000, 2001, 2001, 2300], 256),
    "split_one": ([0, 3, 3, 4], 1),
    "random": (np.concatenate([[0], np.cumsum(np.random.default_rng(5).integers(0, 40, 300))]), 7),
}


@pytest.mark.parametrize("name", sorted(PLANS))
def test_item_planner_matches_numpy(bmsp, name):
    ptr, split = PLANS[name]
    items, folds, slots = bmsp.spmv_op_plan_items(ptr, split)
    ri, rf, rs = plan_ref(ptr, split)
    np.testing.assert_array_equal(items, ri)
    np.testing.assert_array_equal(folds, rf)
    assert slots == rs
    # every tile is in exactly one item, in order; no item is longer than split
    if len(ptr) > 1 and ptr[-1] > 0:
        ne = items[items[:, 2] > items[:, 1]]
        assert ne[0, 1] == 0 and ne[-1, 2] == ptr[-1] and np.array_equal(ne[1:, 1], ne[:-1, 2])
    assert np.all(items[:, 2] - items[:, 1] <= split)


def test_item_planner_refuses_bad_arguments(bmsp):
    L = bmsp.lib()
    ptr = np.array([0, 3, 2], np.uint32)
    n = C.c_int64()
    for args, word in (((ptr.ctypes.data, -1, 4), "blocks"), ((ptr.ctypes.data, 2, 0), "split"), ((None, 2, 4), "ptr"),
                       ((ptr.ctypes.data, 2, 4), "decreases")):
        assert L.bmsp_spmv_op_plan_items(args[0], args[1], args[2], None, None, C.byref(n), None, None) == BMSP_ERR_INVALID
        assert word in _msg(bmsp), _msg(bmsp)
    assert L.bmsp_spmv_op_plan_items(None, 0, 4, None, None, C.byref(n), None, None) == 0 and n.value == 0
