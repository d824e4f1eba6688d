"""CPU tests of the surface of bmsp_matrix_color_blocks / bmsp_matrix_permute_blocks / bmsp_vec_permute_blocks, and what
tests/test_zzzzzz_reorder.py shares with them: the named inputs and the numpy reference of the colouring -- the rule of include/bmsp.h as a
sequential loop over the block-rows in descending key order, returning colours, rounds and the ordering.

Checked here without a GPU, per input and for the seeds 0 and 12345: the reference's colouring is proper and uses at most 1 + the largest
degree colours; its ordering is a permutation with a trailing partial block-row last; the host planner of bmsp_spsv (pybmsp.spsv_plan) on
the block pattern permuted by it reports as many levels as there are colours for both triangles when n % 8 == 0 and no more otherwise, 25
levels on band200 in the natural order against its 4 colours.  Also: the prototypes and the layout of bmsp_color_info in bmsp.h, the
refusals of the three C entry points that need no device (scalars and null pointers, the argument named), the Python wrappers and the C++
ones (compile + link)."""
import ctypes as C
import functools
import inspect
import os
import subprocess
import numpy as np
import pytest
from conftest import REPO
from test_spsv_api import block_records, _msg, _flat

BMSP_ERR_INVALID = -1
NAMES = ("band200", "band203", "lowerband", "poisson5", "dense528", "hub", "gaps", "empty")
SEEDS = (0, 12345)
GAP_TILES = ((0, 0), (0, 5), (3, 3), (3, 7), (4, 0), (9, 9), (9, 15), (15, 2), (15, 9), (18, 18))   # of 20 block-rows, 14 hold no tile


# ---------------------------------------------------------------------------------------------------------
# the inputs
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pattern(name):
    """(n, rows, cols) of a named input, sorted by (row, col), int64"""
    from pybmsp import gen
    if name == "band200":
        n, _, r, c, _ = gen.banded(200, 9)
    elif name == "band203":
        n, _, r, c, _ = gen.banded(203, 9)
    elif name == "lowerband":                   # the tiles of band200 on and below the block diagonal
        n, r, c = pattern("band200")
        keep = r // 8 >= c // 8
        r, c = r[keep], c[keep]
    elif name == "poisson5":
        n, _, r, c, _ = gen.poisson("5pt", 12, 10)
    elif name == "dense528":                    # 66 mutually adjacent block-rows
        n = 528
        r, c = [a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij")]
    elif name == "hub":                         # a diagonal, block-row 3 and block-column 3 full
        n = 640
        d, a, h = np.arange(n), np.repeat(np.arange(24, 32), n), np.tile(np.arange(n), 8)
        r, c = np.concatenate([d, a, h]), np.concatenate([d, h, a])
    elif name == "gaps":
        n = 160
        r = np.array([8 * i + (i + 3 * j) % 8 for i, j in GAP_TILES] + [8 * i + (i + j + 4) % 8 for i, j in GAP_TILES])
        c = np.array([8 * j + (2 * i + j) % 8 for i, j in GAP_TILES] + [8 * j + (i + j + 1) % 8 for i, j in GAP_TILES])
    elif name == "empty":
        n, r, c = 0, np.zeros(0, np.int64), np.zeros(0, np.int64)
    else:
        raise KeyError(name)
    n = int(n)
    key = np.unique(np.asarray(r, np.int64) * max(n, 1) + np.asarray(c, np.int64))
    r, c = key // max(n, 1), key % max(n, 1)
    r.setflags(write=False)
    c.setflags(write=False)
    return n, r, c


def generic_values(name, dtype, seed=7):
    """one value per stored entry of input `name`, generic (no two alike in bits beyond chance, none zero), rounded to the dtype"""
    n, r, c = pattern(name)
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.5, 2.0, r.size) * rng.choice([-1.0, 1.0], r.size)
    return v.astype({0: np.float32, 1: np.float16, 2: np.float64}[dtype]).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------
def neighbours(n, r, c):
    """adj[I] = the sorted block-rows J != I with a tile (I, J) or (J, I)"""
    nb = (n + 7) // 8
    br, bc = r // 8, c // 8
    off = br != bc
    e = np.unique(np.concatenate([br[off] * max(nb, 1) + bc[off], bc[off] * max(nb, 1) + br[off]]))
    ptr = np.searchsorted(e // max(nb, 1), np.arange(nb + 1))
    other = e % max(nb, 1)
    return [other[ptr[i]:ptr[i + 1]] for i in range(nb)]


@functools.lru_cache(maxsize=None)
def reference(name, seed):
    """(colors, rounds, perm, n_colors, n_rounds) of input `name`: the rule of include/bmsp.h, sequentially"""
    from pybmsp import gen
    n, r, c = pattern(name)
    nb = (n + 7) // 8
    adj = neighbours(n, r, c)
    ids = np.arange(nb, dtype=np.uint64)
    h = gen.splitmix64(np.uint64(seed) ^ ids)
    order = np.lexsort((ids, h))[::-1]          # descending (hash, index)
    colors, rounds = np.full(nb, -1, np.int64), np.zeros(nb, np.int64)
    for i in order:
        done = [j for j in adj[i] if colors[j] >= 0]        # exactly the neighbours with a greater key
        used = {int(colors[j]) for j in done}
        k = 0
        while k in used:
            k += 1
        colors[i] = k
        rounds[i] = 1 + max([int(rounds[j]) for j in done], default=0)
    n_colors = int(colors.max()) + 1 if nb else 0
    cls = colors.copy()
    if n % 8:                                   # the class of the trailing partial block-row goes last
        last = colors[nb - 1]
        cls = np.where(colors < last, colors, np.where(colors == last, n_colors - 1, colors - 1))
    perm = np.lexsort((np.arange(nb), cls)).astype(np.uint32)
    for a in (colors, rounds, perm):
        a.setflags(write=False)
    return colors.astype(np.uint32), rounds, perm, n_colors, int(rounds.max()) if nb else 0


def inverse(perm):
    inv = np.empty(perm.size, np.int64)
    inv[np.asarray(perm, np.int64)] = np.arange(perm.size)
    return inv


def permuted(r, c, row_perm=None, col_perm=None):
    """the coordinates of P A Q^T, block (I', J') = block (row_perm[I'], col_perm[J']) of A, in A's entry order"""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    r2 = r if row_perm is None else inverse(row_perm)[r // 8] * 8 + r % 8
    c2 = c if col_perm is None else inverse(col_perm)[c // 8] * 8 + c % 8
    return r2, c2


def plan_levels(bmsp, n, r, c, lower):
    ptr, other = block_records(n, r, c, "N")
    return bmsp.spsv_plan(ptr, other, lower, 0)[2].size - 1


# ---------------------------------------------------------------------------------------------------------
# the reference's self-checks
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", NAMES)
def test_reference_colouring_is_proper_and_orders_into_levels(bmsp, name, seed):
    n, r, c = pattern(name)
    nb = (n + 7) // 8
    colors, rounds, perm, n_colors, n_rounds = reference(name, seed)
    adj = neighbours(n, r, c)
    for i in range(nb):
        assert not np.any(colors[adj[i]] == colors[i]), (name, i)
        if adj[i].size == 0:
            assert colors[i] == 0 and rounds[i] == 1
    assert n_colors <= 1 + max([a.size for a in adj], default=-1)
    assert np.array_equal(np.sort(perm), np.arange(nb))
    if n % 8:
        assert perm[-1] == nb - 1
    if nb:
        assert 1 <= n_rounds <= nb and n_colors >= 1
    r2, c2 = permuted(r, c, perm, perm)
    assert r2.size == 0 or (r2.max() < n and c2.max() < n)
    # A block-row of colour c > 0 has a neighbour of every smaller colour, in front of it in the ordering: with a tile on BOTH sides of
    # the diagonal for every neighbour pair (a symmetric block pattern) that is a dependency in either triangle, so each has exactly
    # n_colors levels.  lowerband stores one side only: each of its triangles has at most n_colors levels (5 colours, 4 levels under
    # seed 12345), and the equality holds for its symmetrised pattern, the graph that was coloured.
    symmetric = np.array_equal(np.unique(r // 8 * max(nb, 1) + c // 8), np.unique(c // 8 * max(nb, 1) + r // 8))
    assert symmetric == (name not in ("lowerband", "gaps"))     # (gaps: most of its tiles have no mirror image either)
    for lower in (1, 0):
        levels = plan_levels(bmsp, n, r2, c2, lower)
        both = plan_levels(bmsp, n, np.concatenate([r2, c2]), np.concatenate([c2, r2]), lower)
        if n % 8 == 0:
            assert both == n_colors, (name, seed, lower, both, n_colors)
            assert levels == n_colors if symmetric else levels <= n_colors, (name, seed, lower, levels, n_colors)
        else:
            assert levels <= both <= n_colors, (name, seed, lower, levels, both, n_colors)


def test_the_inputs_cover_what_they_are_named_for(bmsp):
    n, r, c = pattern("band200")
    assert reference("band200", 0)[3] == 4
    assert plan_levels(bmsp, n, r, c, 1) == 25 and plan_levels(bmsp, n, r, c, 0) == 25
    for seed in SEEDS:
        assert np.array_equal(reference("lowerband", seed)[0], reference("band200", seed)[0])       # symmetrisation
        assert reference("dense528", seed)[3] == 66                                                 # the second colour window
        assert np.array_equal(np.sort(reference("dense528", seed)[0]), np.arange(66))
    assert pattern("band203")[0] % 8 == 3
    hub = neighbours(*pattern("hub"))
    assert hub[3].size == 79 and all(a.size == 1 for i, a in enumerate(hub) if i != 3)
    gaps = pattern("gaps")
    assert np.setdiff1d(np.arange(20), gaps[1] // 8).size == 14
    assert pattern("poisson5")[0] == 120 and pattern("empty")[0] == 0


# ---------------------------------------------------------------------------------------------------------
# the entry points
# ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_interface_verbatim(bmsp):
    hdr = _flat(open(os.path.join(REPO, "include", "bmsp.h")).read())
    for line in ("typedef struct { char kernel[64]; int64_t blocks, colors, rounds, view_bytes; } bmsp_color_info;",
                 "int bmsp_matrix_color_blocks(bmsp_matrix_t A, uint64_t seed, uint32_t *d_colors, uint32_t *d_perm /* may be NULL */, "
                 "void *stream, bmsp_color_info *info /* may be NULL */);",
                 "int bmsp_matrix_permute_blocks(bmsp_matrix_t A, const uint32_t *d_row_perm /* NULL = identity */, "
                 "const uint32_t *d_col_perm /* NULL = identity */, int out_transposed, void *stream, bmsp_matrix_t *out);",
                 "int bmsp_vec_permute_blocks(int64_t n, int vec_f64, const uint32_t *d_perm, int inverse, const void *d_x, void *d_y, "
                 "void *stream);",
                 "BMSP_ERR_INTERNAL = -7"):
        assert _flat(line) in hdr, line
    assert "no access outside [0, n)" in hdr
    for name in ("bmsp_matrix_color_blocks", "bmsp_matrix_permute_blocks", "bmsp_vec_permute_blocks"):
        assert name in bmsp.SYMBOLS and hasattr(bmsp.lib(), name)


def test_info_layout_and_wrappers(bmsp):
    I = bmsp.ColorInfo
    assert [f[0] for f in I._fields_] == ["kernel", "blocks", "colors", "rounds", "view_bytes"]
    assert C.sizeof(I) == 64 + 4 * 8 and I.blocks.offset == 64 and I.view_bytes.offset == 88
    assert set(I().as_dict()) == {f[0] for f in I._fields_}
    assert list(inspect.signature(bmsp.color_blocks).parameters)[:3] == ["A", "seed", "stream"]
    assert list(inspect.signature(bmsp.permute_blocks).parameters) == ["A", "row_perm", "col_perm", "transposed", "stream"]
    assert list(inspect.signature(bmsp.vec_permute_blocks).parameters) == ["perm", "x", "inverse", "y", "n", "stream"]
    for name in ("color_blocks", "permute_blocks", "reorder_multicolor"):
        assert callable(getattr(bmsp.BmSpMatrix, name))


@pytest.fixture()
def vec():
    """host buffers standing in for device vectors: the calls under test refuse before they touch them"""
    buf = (C.c_float * 32)()
    return C.addressof(buf), C.addressof(buf) + 64


def test_scalars_and_null_pointers_are_refused_and_named(bmsp, vec):
    L = bmsp.lib()
    x, y = vec
    out = C.c_void_p()
    info = bmsp.ColorInfo()
    assert L.bmsp_matrix_color_blocks(None, 0, x, y, None, C.byref(info)) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)
    assert L.bmsp_matrix_color_blocks(None, 0, None, None, None, None) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)
    for lay in (2, -1):
        assert L.bmsp_matrix_permute_blocks(None, None, None, lay, None, C.byref(out)) == BMSP_ERR_INVALID
        assert "out_transposed" in _msg(bmsp) and out.value is None
    assert L.bmsp_matrix_permute_blocks(None, None, None, 0, None, C.byref(out)) == BMSP_ERR_INVALID and "matrix A" in _msg(bmsp)
    assert out.value is None
    V = L.bmsp_vec_permute_blocks
    for args, word in (((-1, 0, x, 0, x, y), "n "), ((8, 2, x, 0, x, y), "vec_f64"), ((8, -1, x, 0, x, y), "vec_f64"),
                       ((8, 0, x, 2, x, y), "inverse"), ((8, 1, x, -1, x, y), "inverse"), ((8, 0, None, 0, x, y), "d_perm"),
                       ((8, 0, x, 0, None, y), "d_x"), ((8, 0, x, 1, x, None), "d_y"), ((8, 0, x, 0, y, y), "d_y must not be d_x")):
        assert V(*args, None) == BMSP_ERR_INVALID, args
        assert word in _msg(bmsp), (args, _msg(bmsp))
    assert V(0, 0, None, 0, None, None, None) == 0          # nothing to move: nothing is touched


def build_cpp_reorder_check(out_path):
    lib_dir = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp_reorder_check.cpp"), "-o", out_path, "-L" + lib_dir, "-lbmsp",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_reorder_wrappers_compile_and_link(bmsp, tmp_path):
    """include/bmSpMatrix.h with bmSparse_color_blocks / bmSparse_permute_blocks / bmSparse_vec_permute_blocks and
    bmSpMatrix<T>::permute_blocks instantiated for float, half and double links against libbmsp.so with a plain host compiler."""
    build_cpp_reorder_check(str(tmp_path / "cpp_reorder_check"))
