"""bmsp_matrix_invalidate(m, 1) against every structure-derived cache of a handle.

include/bmsp.h lets a caller rewrite `keys`, `bmps` and `offsets` of a handle in place and call bmsp_matrix_invalidate(m, 1); from then
on every operator must see the new structure.  The promise rests on csrc/matrix.h: every structure-derived cache is a member of
bmsp_structure_caches, which owns its allocations and which invalidate_matrix (csrc/builder.hip) replaces by a fresh one.  A cache kept
anywhere else produces no error: the next call succeeds with the numbers of the old structure (section 5 and tests/host_handle_check.cpp
guard the rule, the GPU cases its effect).  One GPU case (tests/test_zzzzzzzz_structure_invalidate.py) is: build A from a pattern P, prepare(3), make ONE call pinned to
one kernel or route and assert from launch info / stats that it ran (the cache exists) and gave P's result; write P' over A's four arrays
(from a second handle built from P' by from_coo, through bmsp_memcpy_h2d), A.invalidate(True); the same call on A and on `fresh`, a handle
built from P', must agree bit for bit with each other and with the reference (numpy float64 on P''s COO; the oracle for products; the
bit-exact C references of test_spitsv_api.py / test_ilu0_api.py for the sweeps), and report the same launch info / stats -- a cache that is
merely gone and never rebuilt (a *_tried flag left set) fails the last check.  This file holds the inputs, the rewrites, the numpy model,
the table of cases and the CPU self-checks.  There is no tolerance anywhere: matrix values are 1..3, vector entries small positive
integers, every sum is exact in fp16 / fp32 / fp64 in any order (test_every_sum_is_exact).

HARD RULE (as in test_streams.py): a stale cache must give a WRONG ANSWER, never an out-of-range access.  Every rewrite takes P to a P'
of the same shape (both dimensions multiples of 8), the same block_num and nnz, a BIT-IDENTICAL offsets array and the same global tile
order; only where a tile sits and where its entries sit inside it change.  P occupies even block-rows and even block-columns only; a tile
is relabelled monotonically into a slot P leaves empty (2k -> 2k + 1) and reflected inside (i -> 7 - i):

  C        every tile moves from block-column 2c to 2c + 1, columns reflected
  R        every tile of every other occupied block-row moves from 2I to 2I + 1; rows reflected in every tile (the block-row pointer changes)
  RC       both
  Rsplit   the trailing half of the tiles of every other occupied block-row moves to the empty block-row behind it, rows reflected in the
           tiles that move (block-row lengths and max_row_blocks change); only for readers that allocate nothing from the structure
  D        (input `diag` only) off-diagonal tiles move from (2I, 2J) to (2I + 1, 2J + 1), both reflections; see below

Tiles are ordered by (block-row, block-column) in BOTH tile layouts (only the order inside a tile differs), so the same rewrites keep the
tile order of a column-major handle too: nothing has to be exchanged for layout 1 (test_rewrite_invariants runs both layouts).

Why every mix of stale and fresh quantities stays in bounds, per cache:
  rowptr, max_row_blocks        tile indices <= block_num; block-row lengths of P are those of a matrix of the same block_num
  SpMV plan (spmv_chunks)       items hold block-rows < nbr, tile ranges inside [0, block_num], value offsets taken from `offsets` (unchanged);
                                carry slots and counters are sized by the plan that indexes them
  position cache (spmv_pos)     per stored value {tile slot in its batch, position < 64}; tinfo {block column inside the shape, block-row
                                inside the item's window}; eoff from `offsets`: x is read inside num_cols, u written inside the window
  chunk words (spmv_cw)         per stored value {row relative to the chunk's first block-row, column < num_cols}, records hold block-rows
                                of P: rows < num_rows; the value index is the word's own position (nnz unchanged)
  block_meta, sym_recs          per tile {bitmap, value offset from `offsets` (unchanged), block column inside the shape}: a stale bitmap has
                                the popcount of the fresh one (reflection), so offset + popcount stays inside the values
  col_index / col_index_row     tile indices inside P's block-rows, i.e. <= block_num; col_mass: prefix sums up to block_num
  dense_tiles, lane_tiles       block_num x 64 values in position order, indexed by tile; csr_rowptr / csr_ent: num_rows + 1 offsets into
                                nnz entries with columns inside the shape
  sp_tasks / task_begin / c_of_wave   only read for a C whose stamps match; C's own counts never change (below)
  op views, spsv plans, ilu0_diag, krylov_ws   tile records {bitmap, value offset, other block index inside the shape}, pointers of
                                blocks + 1 entries, value indices < nnz; level lists hold block indices < blocks
  shard_view, shard_bounds      block-row bounds <= nbr; the panel's tile range is taken from the fresh block-row pointer
SpGEMM allocates C from the structure, so C's counts must not change: the handle under test is rewritten by R as the left operand and by
C as the right operand (C's block-rows / block-columns are relabelled with it: test_product_counts_do_not_change).  For the right
operand's block-row pointer, R is applied to B and the call is made with a FRESH left handle whose columns carry the same relabelling:
the correct product is then the product of before, and a stale block-row pointer of B loses contributions.

Input `diag` (spitsv, ilu0) needs every diagonal entry stored, in the odd block-rows too, so it cannot leave them empty: every block (b, b)
holds its eight diagonal entries and stays where it is (both reflections map the diagonal onto itself), the off-diagonal tiles sit at
(2I, 2J) and move to (2I + 1, 2J + 1).  The tile ORDER changes here (a diagonal tile and its block-row's off-diagonal tiles swap places);
the offsets stay bit-identical because EVERY tile of this input holds exactly eight values, which is all the argument above uses.

Never run, on the GPU, a library or a test variant that leaves a cache stale on purpose.  That the cases would notice a stale cache is
shown here on the CPU: a numpy model of SpMV on (keys, in-tile positions, block-row pointer) with each of the three stale in turn
(test_stale_hybrids_give_other_results), and the oracle's products of the old and the new operand (test_old_and_new_products_differ)."""
import functools
import os
import re
import numpy as np
import pytest

import util
from test_value_cache_coherence import READERS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "csrc")
NPDT = {0: np.float32, 1: np.float16, 2: np.float64}
OUTDT = {0: np.float32, 1: np.float32, 2: np.float64}
DT = {0: "f32", 1: "f16", 2: "f64"}
MASK32 = np.uint64(0xFFFFFFFF)

# csrc/spmv_plan.h kItemTiles, csrc/spmv.hip BMSP_CH_V, csrc/matrix.h kIdxMinLen (test_constants_match_sources)
ITEM_TILES, CHUNK_VALUES, IDX_MIN_LEN = 256, 512, 16
LONG_K = 9     # the occupied block-row (block-row 2 * LONG_K) of `sparse` that holds a tile in every even block column


# ---------------------------------------------------------------------------------------------------------
# 1. inputs: patterns on even block-rows and block-columns, values, vectors
# ---------------------------------------------------------------------------------------------------------
def _uniq(nr, nc, r, c):
    key = np.unique(np.asarray(r, np.int64) * nc + np.asarray(c, np.int64))
    r, c = key // nc, key % nc
    r.setflags(write=False)
    c.setflags(write=False)
    return int(nr), int(nc), r, c


def _scattered(rng, tiles_br, tiles_bc, per_tile=3):
    """`per_tile` distinct positions in each of the given tiles"""
    pos = np.argsort(rng.random((tiles_br.size, 64)), axis=1)[:, :per_tile]
    r = (8 * tiles_br[:, None] + pos // 8).ravel()
    c = (8 * tiles_bc[:, None] + pos % 8).ravel()
    return r, c


@functools.lru_cache(maxsize=None)
def pattern(name):
    """(nr, nc, r, c), sorted by (row, col), no duplicates; tiles on even block-rows and even block-columns only (`diag`: see the docstring)

    sparse  640 x 8320, ~3 values per tile, 3445 tiles: 75 tiles in every occupied block-row, all 520 even block columns in block-row 18
            (longer than kItemTiles on both sides of Rsplit: the plan marks it long; 1560 values: the chunked sweep folds it across chunks)
    dense   640 x 640, a band of three tiles per occupied block-row: the diagonal tile full, the others 24 to 28 values (row-group, sweep<FULL>,
            the strip / K = 32 MFMA / fp32 MFMA block-MACs)
    fem     640 x 640, the same band with nearly empty tiles (15 and 9 values): the row-sparse kernel
    square  640 x 640, ~24 of 40 tiles per occupied block-row, ~3 values per tile, some on the diagonal and the anti-diagonal of the
            diagonal tiles: block-rows of B longer than kIdxMinLen for col_index; diagonal(); colouring
    diag    320 x 320, every diagonal entry stored, exactly eight values in every tile"""
    rng = np.random.default_rng({"sparse": 5, "dense": 6, "fem": 7, "square": 8, "diag": 9}[name])
    if name == "sparse":
        nr, nc, slots = 640, 8320, 520
        br, bc = [], []
        for k in range(nr // 16):
            cols = np.arange(slots) if k == LONG_K else np.sort(rng.choice(slots, 75, replace=False))
            br.append(np.full(cols.size, 2 * k)); bc.append(2 * cols)
        return _uniq(nr, nc, *_scattered(rng, np.concatenate(br), np.concatenate(bc)))
    if name in ("dense", "fem"):
        n, r, c = 640, [], []
        i, j = np.divmod(np.arange(64), 8)
        for k in range(n // 16):
            for q in (k - 1, k, k + 1):
                if not 0 <= q < n // 16:
                    continue
                if name == "dense":
                    keep = np.ones(64, bool) if q == k else (((3 * i + 5 * j + k) % 8 < 3) | ((i == 1) & (j < 4)))
                else:
                    keep = ((i == j) | (j == i + 1)) if q == k else ((i == j) | ((i == 0) & (j == 5)))
                r.append(16 * k + i[keep]); c.append(16 * q + j[keep])
        return _uniq(n, n, np.concatenate(r), np.concatenate(c))
    if name == "square":
        n, slots = 640, 40
        br, bc = [], []
        for k in range(slots):
            cols = np.union1d(rng.choice(slots, 24, replace=False), [k])
            br.append(np.full(cols.size, 2 * k)); bc.append(2 * cols)
        r, c = _scattered(rng, np.concatenate(br), np.concatenate(bc))
        d = 16 * np.arange(slots)
        extra_r = np.concatenate([d + q for q in (0, 1, 2, 0, 3)])
        extra_c = np.concatenate([d + q for q in (0, 1, 2, 7, 4)])
        return _uniq(n, n, np.concatenate([r, extra_r]), np.concatenate([c, extra_c]))
    if name == "diag":
        n, slots = 320, 20
        r, c = [np.arange(n)], [np.arange(n)]
        for k in range(slots):
            for q in rng.choice(np.delete(np.arange(slots), k), 5, replace=False):
                pos = rng.choice(64, 8, replace=False)
                r.append(16 * k + pos // 8); c.append(16 * q + pos % 8)
        return _uniq(n, n, np.concatenate(r), np.concatenate(c))
    raise ValueError(name)


def mvals(r, c, salt=0):
    """stored values 1..3 by coordinate"""
    return (1 + (3 * np.asarray(r, np.int64) + 7 * np.asarray(c, np.int64) + salt) % 3).astype(np.float64)


def xvec(n, width=None):
    """small positive integers that increase strictly inside every block of 8 and are larger on odd blocks than on even ones: a tile that
    moves to the next block column, or whose columns are reflected, meets other entries of x everywhere"""
    j = np.arange(n)
    x = (1 + j % 8 + 8 * ((j // 8) % 2)).astype(np.float64)
    return x if width is None else x[:, None] + np.arange(width, dtype=np.float64)[None, :]


def _tile_rank(br, bc):
    """per entry: rank of its tile inside the tile's block-row, and the number of tiles of that block-row"""
    key = br * (1 << 32) + bc
    tiles = np.unique(key)
    trow = tiles >> 32
    first = np.searchsorted(trow, trow)
    rank = np.arange(tiles.size) - first
    count = (np.searchsorted(trow, trow, side="right") - first)
    t = np.searchsorted(tiles, key)
    return rank[t], count[t]


def rewrite(P, kind):
    """P' as (nr, nc, r', c') with entry i of P' the image of entry i of P (not sorted again)"""
    nr, nc, r, c = P
    br, ir, bc, ic = r // 8, r % 8, c // 8, c % 8
    if kind in ("C", "RC"):
        bc, ic = bc + 1, 7 - ic
    if kind in ("R", "RC"):
        br, ir = br + (br // 2) % 2, 7 - ir
    if kind == "Rsplit":
        rank, count = _tile_rank(br, bc)
        moved = ((br // 2) % 2 == 1) & (rank >= (count + 1) // 2)
        br, ir = br + moved, np.where(moved, 7 - ir, ir)
    if kind == "D":
        off = br != bc
        br, bc, ir, ic = br + off, bc + off, np.where(off, 7 - ir, ir), np.where(off, 7 - ic, ic)
    if kind not in ("C", "R", "RC", "Rsplit", "D"):
        raise ValueError(kind)
    return nr, nc, 8 * br + ir, 8 * bc + ic


def transposed(P):
    return P[1], P[0], P[3], P[2]


def relabelled_left(P):
    """the left operand whose COLUMNS carry rewrite R: against R applied to the right operand's rows the product does not change"""
    return transposed(rewrite(transposed(P), "R"))


REWRITE_OF = {"sparse": ("C", "R", "RC", "Rsplit"), "dense": ("C", "R", "RC", "Rsplit"), "fem": ("C", "R", "RC"), "square": ("C", "R", "RC"),
              "diag": ("D",)}


# ---------------------------------------------------------------------------------------------------------
# 2. the numpy model of the format and of SpMV
# ---------------------------------------------------------------------------------------------------------
class Tiles:
    """the four arrays of a handle built from COO triples, straight from the format's definition, plus what the caches derive from them:
    the tile and the in-tile position of every stored value, and the block-row pointer"""

    def __init__(self, P, layout, vals=None):
        nr, nc, r, c = P
        vals = mvals(r, c) if vals is None else np.asarray(vals, np.float64)
        pos = (c % 8) * 8 + r % 8 if layout else (r % 8) * 8 + c % 8
        key = (r // 8) * (1 << 32) + c // 8
        o = np.lexsort((pos, key))
        key, pos = key[o], pos[o]
        tiles, first, counts = np.unique(key, return_index=True, return_counts=True)
        self.nr, self.nc, self.layout = nr, nc, layout
        self.keys = tiles.astype(np.uint64)
        self.tile = np.searchsorted(tiles, key)
        self.pos = pos
        self.bmps = np.zeros(tiles.size, np.uint64)
        np.bitwise_or.at(self.bmps, self.tile, np.uint64(1) << (63 - pos).astype(np.uint64))
        self.offsets = np.concatenate([first, [key.size]]).astype(np.uint64)
        self.values = vals[o]
        self.rowptr = np.searchsorted(tiles >> 32, np.arange((nr + 7) // 8 + 1)).astype(np.int64)
        self.popcounts = counts


def model_spmv(t, x, keys=None, pos=None, rowptr=None, rows_from="keys"):
    """u = A x for a row-major handle from (keys, positions, block-row pointer), any of them replaced by a stale one.  rows_from: where
    the kernel takes a tile's block-row from -- its key (the caches built from the keys) or the block-row pointer (the kernels that walk it)"""
    keys = t.keys if keys is None else keys
    pos = t.pos if pos is None else pos
    rowptr = t.rowptr if rowptr is None else rowptr
    brow = (keys >> np.uint64(32)).astype(np.int64)[t.tile] if rows_from == "keys" else np.searchsorted(rowptr, t.tile, side="right") - 1
    bcol = (keys & MASK32).astype(np.int64)[t.tile]
    return np.bincount(8 * brow + pos // 8, weights=t.values * x[8 * bcol + pos % 8], minlength=t.nr)


def spmv_reference(P, x):
    """numpy float64 on the COO triples: u (x a vector) or U (x of several columns)"""
    nr, nc, r, c = P
    S = util.scipy_csr(nr, nc, r, c, mvals(r, c))
    return S @ x


def shard_bounds_model(t, parts):
    """comm.hip spmv_bounds: block-row bounds balanced by stored values"""
    off = t.offsets.astype(np.int64)
    total = int(off[t.rowptr[-1]])
    nbr = t.rowptr.size - 1
    bounds, r = [0], 0
    for p in range(1, parts):
        target = total * p // parts
        while r < nbr and off[t.rowptr[r]] < target:
            r += 1
        bounds.append(r)
    return bounds + [nbr]


def colour_reference(P, seed):
    """(colors, perm, n_colors, n_rounds): the sequential rule of test_reorder_api.reference on these triples (n a multiple of 8)"""
    from pybmsp import gen
    from test_reorder_api import neighbours
    n, _, r, c = P
    nb = n // 8
    adj = neighbours(n, r, c)
    ids = np.arange(nb, dtype=np.uint64)
    order = np.lexsort((ids, gen.splitmix64(np.uint64(seed) ^ ids)))[::-1]
    colors, rounds = np.full(nb, -1, np.int64), np.zeros(nb, np.int64)
    for i in order:
        done = [j for j in adj[i] if colors[j] >= 0]
        used = {int(colors[j]) for j in done}
        k = 0
        while k in used:
            k += 1
        colors[i] = k
        rounds[i] = 1 + max([int(rounds[j]) for j in done], default=0)
    perm = np.lexsort((np.arange(nb), colors)).astype(np.uint32)
    return colors.astype(np.uint32), perm, int(colors.max()) + 1, int(rounds.max())


# ---------------------------------------------------------------------------------------------------------
# 3. the oracle's side of the products (computed once, never written to)
# ---------------------------------------------------------------------------------------------------------
_MEMO = {}


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


PRODUCT_INPUT = {"band9": "dense", "band64": "dense", "fem": "fem"}     # the input of a reader of test_value_cache_coherence.READERS, here
SIDES = ("left", "right", "right_rowptr")


def product_operands(inp, side, new):
    """(A, B) as (triples, values): the handle under test with values mvals(.., 0), the partner with mvals(.., 1).  left: the handle is A,
    rewritten by R; right: the handle is B, rewritten by C; right_rowptr: the handle is B, rewritten by R, and -- after the rewrite -- the
    partner is the left operand whose columns carry the same relabelling"""
    P = pattern(inp)
    if side == "left":
        T = rewrite(P, "R") if new else P
        return (T, mvals(T[2], T[3])), (P, mvals(P[2], P[3], 1))
    T = rewrite(P, "C" if side == "right" else "R") if new else P
    if side == "right_rowptr":      # every entry of both operands keeps its value where it goes (entry i is the image of entry i): the same product
        return (relabelled_left(P) if new else P, mvals(P[2], P[3], 1)), (T, mvals(P[2], P[3]))
    return (P, mvals(P[2], P[3], 1)), (T, mvals(T[2], T[3]))


def oracle_product(oracle, inp, side, new, dtype, tc, stale_b=False):
    """the oracle's C (and stats); stale_b: the relabelled left operand against the OLD right operand -- what a stale view of B gives"""
    def make():
        (Pa, va), (Pb, vb) = product_operands(inp, side, new)
        if stale_b:
            Pb, vb = product_operands(inp, side, False)[1]
        A = oracle.bmsp_from_coo(oracle.Coo(Pa[0], Pa[1], Pa[2], Pa[3], va), dtype, False)
        B = oracle.bmsp_from_coo(oracle.Coo(Pb[0], Pb[1], Pb[2], Pb[3], vb), dtype, True)
        return oracle.spgemm(A, B, exact_products=(dtype == 1 and tc != 5))
    return _memo(("product", inp, side, new, dtype, tc, stale_b), make)


# ---------------------------------------------------------------------------------------------------------
# 4. the GPU cases, by family: (id, parameters).  tests/test_zzzzzzzz_structure_invalidate.py runs test_<family> over them
# ---------------------------------------------------------------------------------------------------------
ROUTES = {
    # name -> (switches as test_spgemm_regimes.py / test_spgemm_special_values.py pin them, (sort_path values, sort_long or None))
    "pipeline": ({"BMSP_SPGEMM_ROWMERGE": "0"}, ((0, 1), None)),
    "strip_mode": ({"BMSP_SPGEMM_ROWMERGE": "1"}, ((2,), 1)),
    "tasklist_mode": ({"BMSP_SPGEMM_ROWMERGE": "2", "BMSP_MAC_STRIP": "0"}, ((2,), 2)),
    "windows": ({"BMSP_SPGEMM_ROWWINDOW": "1", "BMSP_WIN_THIN": "1"}, ((3,), None)),
}
BACK = {"spmv": "chunk_row_sorted-f32-C", "spmm": "vstream4-C", "spgemm_reader": "f32_strip-left", "spgemm_route": "windows-right",
        "numeric_stamp": None, "sharded_spmv": "loopback3-Rsplit", "rowptr_reader": "to_csr_device-R", "spitsv": "no_check3-D",
        "ilu0_values": None, "color_permute": "seed5-RC"}     # one case per family also goes back to P


def family_cases(family):
    if family == "spmv":
        return [("%s-%s-%s" % (l, DT[d], rw), (l, d, rw)) for l, d in util.spmv_launch_params() for rw in ("C", "Rsplit")]
    if family == "spmm":
        return [("%s-C" % l, (l, "C")) for l in util.SPMM_LAUNCHES]
    if family == "spgemm_reader":
        return [("%s-%s" % (rd, side), (rd, side)) for rd in READERS for side in ("left", "right")]
    if family == "spgemm_route":
        return [("%s-%s" % (rt, side), (rt, side)) for rt in ROUTES for side in SIDES]
    if family == "numeric_stamp":
        return [("%s-%s" % (maker, side), (maker, side)) for maker in ("spgemm", "symbolic") for side in ("left", "right", "product")]
    if family == "sharded_spmv":
        return [("loopback3-Rsplit", (3, "Rsplit"))]
    if family == "rowptr_reader":
        return [("%s-R" % rd, (rd, "R")) for rd in ("to_csr_device", "prune_row_rel", "row_absmax", "diagonal")]
    if family == "spitsv":
        return [("no_check3-D", (3, "D"))]
    if family == "ilu0_values":
        return [("no_check3-D", (3, "D"))]
    if family == "color_permute":
        return [("seed5-RC", (5, "RC"))]
    raise ValueError(family)


FAMILIES = tuple(BACK)


def params(family):
    return [pytest.param(*p, id=i) for i, p in family_cases(family)]


def all_case_ids():
    return {"%s[%s]" % (f, i) for f in FAMILIES for i, _ in family_cases(f)}


def _ids(family, pred=lambda p: True):
    return ["%s[%s]" % (family, i) for i, p in family_cases(family) if pred(p)]


def _reader_ids(names):
    return _ids("spgemm_reader", lambda p: p[0] in names)


def _spmv_ids(prefix):
    return _ids("spmv", lambda p: util.SPMV_LAUNCHES[p[0]][3].startswith(prefix))


OTHER_FILES = "tests/"      # a case id that starts with this names a test of another file: "tests/<file>::<test function>"
# every owning member of the handle's two cache groups (bmsp_matrix_invalidate(m, 1) releases them all) -> the GPU cases that read it after a rewrite
CACHES = {
    "rowptr": _ids("rowptr_reader") + _spmv_ids("spmv_blockrow_kernel") + _spmv_ids("spmv_rowgroup_kernel") + _ids("spgemm_route", lambda p: p[1] == "right_rowptr"),
    "spmv_chunks": _spmv_ids("spmv_vstream_kernel") + _spmv_ids("spmv_sweep_kernel") + _ids("spmm") + _ids("sharded_spmv"),
    "spmv_pos": _spmv_ids("spmv_vstream_kernel<kCached") + _ids("spmm", lambda p: p[0].startswith("vstream")),
    "spmv_cw": _spmv_ids("spmv_chunk_kernel"),
    "block_meta": _reader_ids(("f16_mfma", "f16_valu", "f32_valu", "f32_mfma")) + _ids("spgemm_route", lambda p: p[0] in ("pipeline", "tasklist_mode")),
    "sym_recs": _ids("spgemm_route", lambda p: p[0] == "windows" and p[1] != "left"),
    "col_index": _ids("spgemm_route", lambda p: p[0] == "windows" and p[1] != "left"),
    "col_index_row": _ids("spgemm_route", lambda p: p[0] == "windows" and p[1] != "left"),
    "col_mass": _ids("spgemm_route", lambda p: p[0] == "windows" and p[1] != "left"),
    "dense_tiles": _reader_ids(("f16_mfma", "f16_strip", "f16_valu", "f32_valu")),
    "lane_tiles": _reader_ids(("f32_strip", "f32_mfma")),
    "csr_rowptr": _reader_ids(("f16_rowsparse", "f32_rowsparse")),
    "csr_ent": _reader_ids(("f16_rowsparse", "f32_rowsparse")),
    "sp_tasks": _ids("numeric_stamp", lambda p: p[0] == "symbolic"),
    "sp_task_begin": _ids("numeric_stamp", lambda p: p[0] == "symbolic"),
    "sp_c_of_wave": _ids("numeric_stamp", lambda p: p[0] == "symbolic"),
    "tp_map": ["tests/test_transpose.py::test_copy_values_refuses_foreign_or_stale_sources"],
    "add_map": ["tests/test_add.py::test_add_values_refusals"],
    "spmv_op_views": _ids("spitsv") + _ids("color_permute") + ["tests/test_spmv_op.py::test_structure_change_with_invalidate"],
    "spmv_op_tmp": ["tests/test_spmv_op.py::test_structure_change_with_invalidate"],
    "spmm_op_scratch": ["tests/test_spmm_op.py::test_structure_change_with_invalidate"],
    "spmm_op_tmp": ["tests/test_spmm_op.py::test_structure_change_with_invalidate"],
    # (bmsp_matrix_ilu0_values refuses an F whose structure was declared changed, so no call can read these two on an invalidated handle:
    # the case asserts the refusal and runs the sweeps on an F made from the rewritten A)
    "ilu0_diag": _ids("ilu0_values"),
    "ilu0_tmp": _ids("ilu0_values"),
    "krylov_ws": ["tests/test_zzzzz_krylov.py::test_operands_and_workspace"],
    "spsv_plans": _ids("spitsv") + ["tests/test_spsv.py::test_structure_change_with_invalidate"],
    "spitsv_tmp": _ids("spitsv"),
    "shard_view": _ids("sharded_spmv"),
}
PUBLIC = ("keys", "bmps", "offsets", "values")
ALIASES = ("spmv_tinfo", "spmv_eoff")      # pointers into the allocation of spmv_pos: never freed on their own, reset with it


# ---------------------------------------------------------------------------------------------------------
# 5. completeness: what execution cannot show, by source scan (the rest is executed: tests/host_handle_check.cpp)
# ---------------------------------------------------------------------------------------------------------
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def function_body(text, signature):
    """the text between the braces of the function (or struct) whose definition starts with `signature`"""
    at = text.index(signature)
    depth, start = 0, text.index("{", at)
    for i in range(start, len(text)):
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return text[start + 1:i]
    raise AssertionError("unbalanced braces after " + signature)


GROUPS = ("bmsp_value_caches", "bmsp_structure_caches")
NESTED = ("bmsp_spmv_op_view", "bmsp_spsv_plan_s")      # member arrays of the structure group; each element owns one allocation (`mem`)


def _declarations(struct_text):
    for line in struct_text.splitlines():
        line = line.split("//")[0]
        if "(" not in line:     # (methods)
            yield line


def raw_pointers(struct_text):
    """the members of a struct that are plain pointers"""
    out = set()
    for line in _declarations(struct_text):
        if re.match(r"\s*(?:const\s+)?[\w:]+\s*\*", line):
            out |= set(re.findall(r"\*\s*(\w+)", line))
    return out


def owning_members(struct_text):
    """the members of a struct that own memory: a DevBuf, an array of views / plans, a matrix pointer"""
    out = set()
    for line in _declarations(struct_text):
        m = re.match(r"\s*bmsp::DevBuf<[\w ]+>\s+([^;]+);", line)
        if m:
            out |= {n.strip() for n in m.group(1).split(",")}
        m = re.match(r"\s*(?:%s)\s+(\w+)\[" % "|".join(NESTED), line) or re.match(r"\s*bmsp::MatrixPtr\s+(\w+);", line)
        if m:
            out.add(m.group(1))
    return out


def member_names(struct_text):
    out = set()
    for line in _declarations(struct_text):
        m = re.match(r"\s*(?:const\s+)?[\w:]+(?:<[\w:, ]+>)?\s*\*?\s*(\w[^;]*);", line)
        if m:
            out |= {re.match(r"\*?\s*(\w+)", n.strip()).group(1) for n in m.group(1).split(",")}
    return out


@functools.lru_cache(maxsize=None)
def scan_handle():
    """(owning members of the two groups, {struct: its text} for the groups, the handle and the nested structs, bodies of the functions
    that drop caches)"""
    header, builder = _source("matrix.h"), _source("builder.hip")
    texts = {g: function_body(header, "struct %s {" % g) for g in GROUPS + NESTED}
    texts["bmsp_matrix_s"] = function_body(header, "struct bmsp_matrix_s :")
    bodies = {"free_matrix": function_body(builder, "void free_matrix(bmsp_matrix_s *m)"),
              "invalidate_matrix": function_body(builder, "void invalidate_matrix(bmsp_matrix_s *m, int structure_changed)"),
              "drop_value_caches": function_body(builder, "void drop_value_caches(bmsp_matrix_s *m)")}
    owning = set().union(*(owning_members(texts[g]) for g in GROUPS))
    return owning, texts, bodies


def test_invalidate_releases_every_pooled_field():
    """Every allocation a handle caches has an owner, and the owners live in the two groups that bmsp_matrix_invalidate assigns afresh:
    no pointer member of the handle, of a group or of a view / plan is raw but the four public arrays and the two aliases into spmv_pos,
    the handle itself declares no owner beside the groups, and the functions that drop caches return nothing to the pool by hand.  What
    the resets then do to a filled handle -- every release, every default, the new uid -- is executed by tests/host_handle_check.cpp
    (test_abi.py), which must name every member of the groups.  This fails the moment a cache is added as a plain pointer"""
    owning, texts, bodies = scan_handle()
    assert len(owning) >= 28, sorted(owning)
    raw = {name: raw_pointers(text) for name, text in texts.items()}
    assert raw["bmsp_matrix_s"] == set(PUBLIC), raw["bmsp_matrix_s"]
    assert raw["bmsp_structure_caches"] == set(ALIASES) and raw["bmsp_value_caches"] == set(), raw
    for n in NESTED:
        assert raw[n] == set() and owning_members(texts[n]) == {"mem"}, (n, raw[n])
    assert owning_members(texts["bmsp_matrix_s"]) == set(), "an owner outside the groups is not reset by bmsp_matrix_invalidate"
    assert re.search(r"struct bmsp_matrix_s : bmsp_value_caches, bmsp_structure_caches \{", _source("matrix.h"))
    for fn, body in bodies.items():
        assert "pool_free(" not in body and "= nullptr" not in body, fn
    inv = bodies["invalidate_matrix"]
    assert inv.index("hipDeviceSynchronize()") < inv.index("m->reset_value_caches();") < inv.index("if (structure_changed) m->reset_structure_caches();")
    handle = texts["bmsp_matrix_s"]
    assert "static_cast<bmsp_value_caches &>(*this) = bmsp_value_caches();" in function_body(handle, "void reset_value_caches()")
    reset = function_body(handle, "void reset_structure_caches()")
    assert "static_cast<bmsp_structure_caches &>(*this) = bmsp_structure_caches();" in reset and "uid = bmsp::next_matrix_uid();" in reset
    assert "bmsp::pool_free(keys); bmsp::pool_free(bmps); bmsp::pool_free(offsets); bmsp::pool_free(values);" in function_body(handle, "void release_arrays()")
    assert "holds_memory()" in bodies["drop_value_caches"] and "m->values_finite = -1" in bodies["drop_value_caches"]
    for g in GROUPS:        # the value group's question: every owner of the group, and nothing else
        if g == "bmsp_value_caches":
            asked = set(re.findall(r"\w+", function_body(texts[g], "bool holds_memory() const")))
            assert asked - {"return"} == owning_members(texts[g]), asked
    with open(os.path.join(REPO, "tests", "host_handle_check.cpp")) as f:
        check = f.read()
    for g in GROUPS:
        missing = {n for n in member_names(texts[g]) if not re.search(r"\b%s\b" % n, check)}
        assert missing == set(), "tests/host_handle_check.cpp does not name: %s" % sorted(missing)
    for name in os.listdir(CSRC):       # the sub-lists are gone, not moved
        assert not re.search(r"\bdrop_spmv_op_views\b|\bdrop_spsv_plans\b", _source(name)), name


@pytest.mark.parametrize("group,line,lost", [("bmsp_structure_caches", "    uint32_t *x = nullptr;", {"x"}),
                                             ("bmsp_value_caches", "    void *x = nullptr;   // a new operand form", {"x"}),
                                             ("bmsp_structure_caches", "    const uint64_t *x = nullptr, *y = nullptr;", {"x", "y"}),
                                             ("bmsp_structure_caches", "    bmsp::DevBuf<uint32_t> x;", set())],
                         ids=["structure-uint32", "value-void", "structure-two", "structure-owned"])
def test_the_scan_notices_a_forgotten_line(group, line, lost):
    """the scan itself, on the text: with a plain pointer member added to a group exactly that member is reported (and an owned one is not)"""
    _, texts, _ = scan_handle()
    before = raw_pointers(texts[group])
    mutated = texts[group] + "\n" + line + "\n"
    assert raw_pointers(mutated) - before == lost
    assert member_names(mutated) - member_names(texts[group]) == (lost or {"x"})


def test_caches_table_covers_the_scanned_set():
    """CACHES names exactly the owning members of the two groups (csrc/matrix.h), and every case id in it exists: a new cache without a
    case fails here"""
    owning, _, _ = scan_handle()
    assert len(owning) >= 28, sorted(owning)
    assert set(CACHES) == owning, (sorted(set(CACHES) - owning), sorted(owning - set(CACHES)))
    ids = all_case_ids()
    import test_zzzzzzzz_structure_invalidate as gpu_cases
    for f in FAMILIES:
        assert callable(getattr(gpu_cases, "test_" + f)), f
        assert BACK[f] is None or BACK[f] in dict(family_cases(f)), (f, BACK[f])
    for field, cases in CACHES.items():
        assert cases, field
        for c in cases:
            if c.startswith(OTHER_FILES):
                path, name = c.split("::")
                with open(os.path.join(REPO, path)) as fh:
                    text = fh.read()
                assert re.search(r"^def %s\(" % re.escape(name), text, re.M) and ("invalidate(True)" in text or "bmsp_matrix_invalidate(" in text), c
            else:
                assert c in ids, (field, c)
    own = {c for cases in CACHES.values() for c in cases if not c.startswith(OTHER_FILES)}
    assert {c.split("[")[0] for c in own} == set(FAMILIES)        # and no family runs beside the table


def test_constants_match_sources():
    assert re.search(r"constexpr uint32_t kItemTiles = %d;" % ITEM_TILES, _source("spmv_plan.h"))
    assert re.search(r"#define BMSP_CH_V %d\b" % CHUNK_VALUES, _source("spmv.hip"))
    assert re.search(r"constexpr uint32_t kIdxMinLen = %d;" % IDX_MIN_LEN, _source("matrix.h"))
    assert re.search(r"rowptr\[r \+ 1\] - rowptr\[r\] > kItemTiles", _source("spmv.hip"))      # "long" = more than kItemTiles tiles


# ---------------------------------------------------------------------------------------------------------
# 6. the rewrites keep what the hard rule needs, and change what the caches hold
# ---------------------------------------------------------------------------------------------------------
def _entry_tiles(P):
    """per entry, in the order given: the index of its tile in the global tile order"""
    key = (P[2] // 8) * (1 << 32) + P[3] // 8
    return np.searchsorted(np.unique(key), key)


def _pairs():
    return [(inp, rw, lay) for inp in REWRITE_OF for rw in REWRITE_OF[inp] for lay in (0, 1)]


@pytest.mark.parametrize("inp,rw,lay", _pairs())
def test_rewrite_invariants(oracle, inp, rw, lay):
    P = pattern(inp)
    Q = rewrite(P, rw)
    nr, nc, r, c = P
    assert nr % 8 == 0 and nc % 8 == 0 and Q[:2] == P[:2]
    assert r.size == Q[2].size and Q[2].min() >= 0 and Q[2].max() < nr and Q[3].min() >= 0 and Q[3].max() < nc
    if inp != "diag":
        assert np.all((r // 8) % 2 == 0) and np.all((c // 8) % 2 == 0)
    a, b = Tiles(P, lay), Tiles(Q, lay)
    # the model is the builder: the oracle's arrays of both patterns
    for t, T in ((a, P), (b, Q)):
        o = oracle.bmsp_from_coo(oracle.Coo(T[0], T[1], T[2], T[3], mvals(T[2], T[3])), 0, bool(lay))
        np.testing.assert_array_equal(o.keys, t.keys)
        np.testing.assert_array_equal(o.bmps, t.bmps)
        np.testing.assert_array_equal(o.offsets, t.offsets)
        np.testing.assert_array_equal(o.values, t.values)
    assert a.keys.size == b.keys.size and a.values.size == b.values.size
    np.testing.assert_array_equal(a.offsets, b.offsets)
    np.testing.assert_array_equal(a.popcounts, b.popcounts)
    assert np.all(np.diff(b.keys.astype(np.int64)) > 0)
    changed = np.count_nonzero(a.keys != b.keys)
    # C, RC and D move every tile (D: every off-diagonal one), R every other occupied block-row, Rsplit the trailing half of those
    assert changed >= {"C": 1.0, "RC": 1.0, "R": 0.45, "D": 0.45, "Rsplit": 0.125}[rw] * a.keys.size, (changed, a.keys.size)
    assert np.count_nonzero(a.bmps != b.bmps) >= changed // 2, "the reflection leaves most bitmaps as they were"
    if inp == "diag":
        assert np.all(a.popcounts == 8)       # what keeps the offsets although the tile order changes (see the docstring)
        for T in (P, Q):
            on = T[2] == T[3]
            assert np.array_equal(np.sort(T[2][on]), np.arange(nr))     # every diagonal entry stored, before and after
    else:
        # the same global tile order: tile t of P' is the image of tile t of P (entry i of P' is the image of entry i of P)
        np.testing.assert_array_equal(_entry_tiles(P), _entry_tiles(Q))
    # what each rewrite changes besides: the block-row pointer, the longest block-row
    if rw in ("C",):
        np.testing.assert_array_equal(a.rowptr, b.rowptr)
    else:
        assert not np.array_equal(a.rowptr, b.rowptr)
    if rw == "Rsplit":
        assert np.diff(a.rowptr).max() != np.diff(b.rowptr).max() or inp == "dense"
        assert not np.array_equal(np.sort(np.diff(a.rowptr)), np.sort(np.diff(b.rowptr)))


def test_inputs_reach_what_they_are_built_for():
    s, d, f, q = (Tiles(pattern(n), 0) for n in ("sparse", "dense", "fem", "square"))
    # sparse: ~3 values per tile, a few thousand tiles, one block-row long for the plan before and after Rsplit, folded by the chunked sweep
    assert 2000 <= s.keys.size <= 5000 and 2.5 < s.values.size / s.keys.size <= 3.0
    for t in (s, Tiles(rewrite(pattern("sparse"), "Rsplit"), 0), Tiles(rewrite(pattern("sparse"), "C"), 0)):
        lens = np.diff(t.rowptr)
        assert lens.max() > ITEM_TILES and np.count_nonzero(lens > ITEM_TILES) in (1, 2)
        k = int(np.argmax(lens))
        v0, v1 = int(t.offsets[t.rowptr[k]]), int(t.offsets[t.rowptr[k + 1]])
        assert v0 // CHUNK_VALUES != (v1 - 1) // CHUNK_VALUES          # its values lie in more than one chunk: a fold
        assert not np.any(t.bmps == ~np.uint64(0)) and t.values.size < 16 * t.keys.size      # value-stream eligible, not row-group by default
    # dense: at least 16 values per tile, a quarter of the tiles full, some partial; no long block-row (the row-group kernel's condition)
    full = d.bmps == ~np.uint64(0)
    assert d.popcounts.min() >= 16 and 4 * np.count_nonzero(full) >= d.keys.size and np.count_nonzero(~full) > d.keys.size // 2
    assert np.diff(d.rowptr).max() <= ITEM_TILES and d.values.size >= 16 * d.keys.size
    # fem: nearly empty tiles (the row-sparse kernel takes operands of at most 16 values per tile on average)
    assert f.values.size <= 16 * f.keys.size and f.popcounts.max() <= 16
    # square: block-rows of the right operand longer than kIdxMinLen (col_index), stored diagonal entries before and after R
    assert np.diff(q.rowptr).max() > IDX_MIN_LEN
    for T in (pattern("square"), rewrite(pattern("square"), "R")):
        assert np.count_nonzero(T[2] == T[3]) >= 40
    P, Q = pattern("square"), rewrite(pattern("square"), "R")
    assert not np.array_equal(np.sort(P[2][P[2] == P[3]]), np.sort(Q[2][Q[2] == Q[3]]))


def test_every_sum_is_exact():
    """values 1..3 and vector entries up to 16 (+ the column index of an SpMM, up to 32): every partial sum is an integer below 2^24, and
    every stored value, vector entry and scalar product fits fp16 exactly; products of the SpGEMM cases are sums of at most 3 x 8 terms of
    at most 9"""
    for inp in ("sparse", "dense", "square"):
        for rw in (None,) + REWRITE_OF[inp]:
            P = pattern(inp) if rw is None else rewrite(pattern(inp), rw)
            nr, nc, r, c = P
            assert set(np.unique(mvals(r, c))) <= {1.0, 2.0, 3.0}
            X = xvec(nc, 33)
            assert X.max() <= 48 and np.array_equal(X.astype(np.float16).astype(np.float64), X)
            assert np.bincount(r, weights=mvals(r, c) * X.max(), minlength=nr).max() < 2.0 ** 24
    x = xvec(64)
    assert np.all(np.diff(x.reshape(-1, 8), axis=1) > 0) and x.reshape(-1, 8)[1].min() > x.reshape(-1, 8)[0].max()
    for inp in ("dense", "fem", "square"):
        t = Tiles(pattern(inp), 0)
        assert np.diff(t.rowptr).max() * 8 * 9 < 2 ** 11


# ---------------------------------------------------------------------------------------------------------
# 7. sensitivity: a stale cache gives another result
# ---------------------------------------------------------------------------------------------------------
STALE = {"C": ("keys", "pos"), "R": ("keys", "pos", "rowptr"), "Rsplit": ("keys", "pos", "rowptr")}
# the share of the rows that hold anything in either result in which a hybrid must differ from the right one.  C moves every tile one block
# column on: every row.  R moves every other occupied block-row: those rows differ where they were and where they are now, two thirds of the
# rows that hold anything (stale positions: every row, all are reflected).  Rsplit moves a quarter of the tiles, out of half of the
# block-rows and into as many
MIN_SHARE = {"C": 0.75, "R": 0.5, "Rsplit": 0.125}


@pytest.mark.parametrize("inp,rw", [(i, rw) for i in ("sparse", "dense") for rw in ("C", "R", "Rsplit")])
def test_stale_hybrids_give_other_results(inp, rw):
    """the model of SpMV on P' with the keys, the in-tile positions or the block-row pointer of P in turn, the others fresh: each hybrid
    differs from the right result in at least MIN_SHARE of the rows that hold anything in either"""
    P, Q = pattern(inp), rewrite(pattern(inp), rw)
    old, new = Tiles(P, 0), Tiles(Q, 0)
    x = xvec(P[1])
    right = model_spmv(new, x)
    np.testing.assert_array_equal(right, spmv_reference(Q, x))
    np.testing.assert_array_equal(model_spmv(new, x, rows_from="rowptr"), right)
    assert not np.array_equal(model_spmv(old, x), right)
    for what in ("keys", "pos", "rowptr"):
        stale = {what: getattr(old, what)}
        rows_from = "rowptr" if what == "rowptr" else "keys"
        got = model_spmv(new, x, rows_from=rows_from, **stale)
        if what not in STALE[rw]:
            np.testing.assert_array_equal(getattr(old, what), getattr(new, what))
            continue
        live = np.count_nonzero((got != 0) | (right != 0))
        diff = np.count_nonzero(got != right)
        print(inp, rw, "stale", what, ":", diff, "of", live, "non-empty rows differ")
        assert diff >= MIN_SHARE[rw] * live, (inp, rw, what, diff, live)


def test_shard_bounds_move_with_rsplit():
    """the sharded SpMV caches its block-row bounds with the panel view: Rsplit moves the first bound of three panels, so the statistics
    of a call on stale bounds differ from the fresh handle's"""
    P = pattern("sparse")
    a, b = shard_bounds_model(Tiles(P, 0), 3), shard_bounds_model(Tiles(rewrite(P, "Rsplit"), 0), 3)
    assert a[0] == b[0] == 0 and a[-1] == b[-1] == P[0] // 8 and a[1] != b[1], (a, b)


def _structure_or_every_value_differs(X, Y):
    if not (np.array_equal(X.keys, Y.keys) and np.array_equal(X.bmps, Y.bmps)):
        return True
    return X.nnz > 0 and not np.any(X.values == Y.values)


def _product_numerics():
    out = {(PRODUCT_INPUT[READERS[rd][4]], READERS[rd][0], READERS[rd][1]) for rd in READERS}
    return sorted(out | {("square", 0, 5)})


@pytest.mark.parametrize("inp,dtype,tc", _product_numerics())
def test_product_counts_do_not_change(oracle, inp, dtype, tc):
    """SpGEMM allocates C from the structure: on the oracle's products alone, C before and after the rewrite of the handle has the same
    tile count, nnz, offsets and stage counters, for the handle on either side; with the relabelled left operand C does not change at all"""
    for side in SIDES:
        (C0, s0), (C1, s1) = oracle_product(oracle, inp, side, False, dtype, tc), oracle_product(oracle, inp, side, True, dtype, tc)
        assert C0.block_num == C1.block_num > 0 and C0.nnz == C1.nnz > 0
        np.testing.assert_array_equal(C0.offsets, C1.offsets)
        assert s0 == s1, (s0, s1)
        if side == "right_rowptr":
            np.testing.assert_array_equal(C0.keys, C1.keys)
            np.testing.assert_array_equal(C0.bmps, C1.bmps)
            np.testing.assert_array_equal(C0.values, C1.values)
        assert C1.values.max() < 2 ** 11 and np.array_equal(C1.values, np.round(C1.values))


@pytest.mark.parametrize("inp,dtype,tc", _product_numerics())
def test_old_and_new_products_differ(oracle, inp, dtype, tc):
    """the product of the old operand differs from that of the new one in structure or in every value; for the relabelled left operand:
    the product with the OLD right operand -- what a stale block-row pointer or view of B multiplies -- differs from the right one"""
    for side in ("left", "right"):
        assert _structure_or_every_value_differs(oracle_product(oracle, inp, side, False, dtype, tc)[0], oracle_product(oracle, inp, side, True, dtype, tc)[0])
    stale = oracle_product(oracle, inp, "right_rowptr", True, dtype, tc, stale_b=True)[0]
    assert _structure_or_every_value_differs(stale, oracle_product(oracle, inp, "right_rowptr", True, dtype, tc)[0])


def test_square_and_diag_rewrites_change_what_their_readers_return():
    """rowptr readers (R on sparse / square), colouring (RC on square), the sweeps (D on diag): the reference result of P' is not P's"""
    P, Q = pattern("sparse"), rewrite(pattern("sparse"), "R")
    assert not np.array_equal(np.bincount(P[2], minlength=P[0]), np.bincount(Q[2], minlength=Q[0]))      # CSR row lengths
    S, T = pattern("square"), rewrite(pattern("square"), "RC")
    assert not np.array_equal(colour_reference(S, 5)[0], colour_reference(T, 5)[0])
    D, E = pattern("diag"), rewrite(pattern("diag"), "D")
    assert not np.array_equal(np.sort(D[2] * 320 + D[3]), np.sort(E[2] * 320 + E[3]))
