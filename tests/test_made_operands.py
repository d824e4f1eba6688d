"""Matrices the library makes itself -- products by every symbolic route, and the outputs of the other makers -- as operands downstream.

Almost every differential suite runs on operands from the COO builder, whose block-row pointer and widest block-row (max_row_blocks) are
derived lazily (ensure_rowptr, ensure_row_stats).  The library's own makers write those facts by hand -- strip mode and task-list mode
write the pointer and the maximum from their scans, the column-window passes the pointer alone, from_diagonal / from_aggregates / load
seed the pointer -- and every later call trusts them: the next product reads the left operand's maximum for surely_fits (strip mode
without T_2), seg_bound (the read-back-free sort), 2 w > kKCap (the strip kernel's merged A list) and the row-sparse kernel's table size;
every operator that walks block-rows reads the pointer.  The rule tested here: what a maker leaves on a handle changes time and nothing
else.

check_container(M)    the format's invariants on a handle, in numpy: keys strictly increasing, block indices inside the grid, no bit
    outside the ragged last block-row / block-column, offsets the exclusive prefix sum of the popcounts, offsets[block_num] == nnz, the
    block-row pointer the searchsorted of the block-row index, no tile with an empty bitmap (include/bmsp.h lets no maker leave one).
twin(M)               M.clone(): the same four arrays on a fresh handle with no cached fact.  For every consumer f, f(M) and f(twin(M))
    must agree in every output bit, in the counters of a product's statistics and in the launch reports.
first_product(w, a)   built on cap_product of test_spgemm_regimes.py: C1 = A1 x B1 has ragged dimensions (77 x 1069), an empty first
    block-row, a run of three empty block-rows in the middle, an empty last one, exactly one widest block-row of w tiles at position 6 and
    a second-widest of 40 at position 2; every tile of C1 holds one value, at a column that is a function of its block column.
second_operand(...)   B2 whose block-row k holds its one value per tile in the row C1's tiles of block column k hold theirs in (every
    candidate pair survives): the block-rows the widest block-row of C1 meets hold exactly b tiles (so that segment has w * b tasks) on
    columns (index * b + 0 .. b - 1) mod u of a pool of u (so the widest block-row of C2 has min(u, w * b) tiles), every other block-row
    fewer than b.  CHAIN puts (w, b) on and one above each threshold the second product reads.

Who leaves what (csrc), and which GPU cases make it:
    pointer and maximum    bmsp_spgemm in strip mode and in task-list mode (rowmerge.hip), bmsp_spgemm_symbolic on those routes
    pointer alone          the column-window passes (rowwindow.hip, maximum left at -1); from_diagonal and from_aggregates (kernels of
                           their own); load, from_csr_device, add, prune, scale, sddmm, spgemm_masked, ilu0, transpose, with_layout,
                           permute_blocks (they call ensure_rowptr on what they return)
    neither                the sort pipeline (segmented and global sort), concat_panels (sharded and paneled products)
Who reads them: the maximum -- surely_fits, seg_bound and the BMSP_SEG_AVG_MAX clause (spgemm.hip), 2 w > kKCap and the row-sparse rule
(mac_choice.h), the row-sparse kernel's table size (blockmac_rowsparse.hip, from C's own maximum); the pointer -- spmv, spmv_op, spmm,
to_csr_device, the next product on either side, row_panel, transpose, add, prune, diagonal, sddmm, spgemm_masked, spsv, ilu0,
aggregate, color_blocks: each is a consumer of the GPU cases.

There is no tolerance in this file or in the GPU cases (tests/test_zzzzzzzzzzz_made_operands.py, collected last): every comparison is
bit for bit.  The CPU self-checks below assert, from the oracle's C1 alone, that every chain case sits where w decides: w is attained by
one block-row, the modelled decision at w differs from the one at the second-widest 40 in every `above` case (an understated or stale
maximum would change the route or the counters), and C2 holds values whose fp32 bits change under the reversed task order."""
import functools
import os
import re
import numpy as np
import pytest

from test_spgemm_regimes import (CSRC, STRIP_ROW_CAP, K_CAP, NARROW_CAP, BLOCK_SEG_MAX, TASK_BLOCK_IDX_BITS, RS_TABLE, cap_product, product_terms,
                                 order_sensitive, _col_in_tile)
from test_structure_invalidate import Tiles

MASK32 = np.uint64(0xffffffff)
SEG_BOUND_MAX = 16384         # spgemm.hip: seg_bound <= 16384 keeps the segmented sort under BMSP_SEG_AVG_MAX
RS_SMALL = STRIP_ROW_CAP      # mac_choice.h rs_row_cap(9): beyond it the row-sparse kernel takes its larger table (RS_TABLE)


def test_constants_match_sources():
    spgemm = open(os.path.join(CSRC, "spgemm.hip")).read()
    assert re.search(r"seg_bound > 0 && seg_bound <= (\d+)\)", spgemm).group(1) == str(SEG_BOUND_MAX)
    assert re.search(r"A->max_row_blocks \* \(uint64_t\)B->max_row_blocks <= \(uint64_t\)mac_strip_row_cap\(\)", spgemm)
    assert re.search(r"2 \* f\.a\.max_row_blocks > kKCap", open(os.path.join(CSRC, "mac_choice.h")).read())
    assert re.search(r"C->max_row_blocks > rs_row_cap\(9\)", open(os.path.join(CSRC, "blockmac_rowsparse.hip")).read())
    assert RS_SMALL < RS_TABLE


# ---- the container check -----------------------------------------------------------------------------------------------------------------
def popcounts(bmps):
    return np.unpackbits(np.ascontiguousarray(bmps, dtype=np.uint64).view(np.uint8)).reshape(-1, 64).sum(axis=1).astype(np.int64)


def edge_mask(valid_rows, valid_cols, layout):
    """the bits of a tile whose row inside the tile is >= valid_rows or whose column is >= valid_cols (bit 63 - position, position =
    8 * row + column in the row-major layout, 8 * column + row in the column-major one)"""
    m = 0
    for r in range(8):
        for c in range(8):
            if r >= valid_rows or c >= valid_cols:
                m |= 1 << (63 - ((8 * c + r) if layout else (8 * r + c)))
    return m


def check_container(M, what=""):
    """the invariants of the format on a handle (host_arrays, info, block_row_ptr); see the docstring of the file.  No maker is exempt
    from the empty-bitmap rule: include/bmsp.h documents none that may leave an empty tile."""
    k, b, o, v = M.host_arrays()
    i = M.info()
    rp = np.asarray(M.block_row_ptr()).astype(np.int64)
    nr, nc, layout = i["num_rows"], i["num_cols"], i["transposed"]
    nbr, nbc = -(-nr // 8), -(-nc // 8)
    assert k.dtype == b.dtype == o.dtype == np.uint64, (what, k.dtype, b.dtype, o.dtype)
    assert k.size == b.size == i["block_num"] and o.size == k.size + 1 and v.size == i["nnz"], (what, k.size, b.size, o.size, v.size, i)
    brow, bcol = (k >> np.uint64(32)).astype(np.int64), (k & MASK32).astype(np.int64)
    assert np.all(k[1:] > k[:-1]), "%s: keys not strictly increasing" % what
    assert k.size == 0 or (brow.max() < nbr and bcol.max() < nbc), "%s: a block index outside %d x %d" % (what, nbr, nbc)
    outside = np.zeros(k.size, np.uint64)
    row_edge, col_edge = (brow == nbr - 1) & (nr % 8 != 0), (bcol == nbc - 1) & (nc % 8 != 0)
    outside[row_edge] |= np.uint64(edge_mask(nr % 8, 8, layout))
    outside[col_edge] |= np.uint64(edge_mask(8, nc % 8, layout))
    assert not np.any(b & outside), "%s: a bitmap bit outside the ragged edge" % what
    pc = popcounts(b)
    assert np.all(pc > 0), "%s: a tile with an empty bitmap" % what
    assert np.array_equal(o.astype(np.int64), np.concatenate([[0], np.cumsum(pc)])), "%s: offsets are not the prefix sum of the popcounts" % what
    assert int(o[-1]) == i["nnz"], "%s: offsets[block_num] != nnz" % what
    assert rp.size == nbr + 1 and np.array_equal(rp, np.searchsorted(brow, np.arange(nbr + 1))), "%s: block-row pointer" % what


class HostMatrix:
    """a handle's read-only face over host arrays (the CPU self-checks, and the oracle's matrices)"""

    def __init__(self, nr, nc, keys, bmps, offsets, values, layout=0, rowptr=None, nnz=None):
        self.nr, self.nc, self.layout = int(nr), int(nc), int(layout)
        self.arrays = (np.asarray(keys, np.uint64), np.asarray(bmps, np.uint64), np.asarray(offsets, np.uint64), np.asarray(values))
        self.nnz = self.arrays[3].size if nnz is None else nnz
        brow = (self.arrays[0] >> np.uint64(32)).astype(np.int64)
        self.rowptr = np.searchsorted(brow, np.arange(-(-self.nr // 8) + 1)).astype(np.uint32) if rowptr is None else np.asarray(rowptr, np.uint32)

    def host_arrays(self):
        return self.arrays

    def info(self):
        return dict(num_rows=self.nr, num_cols=self.nc, nnz=self.nnz, block_num=self.arrays[0].size, dtype=0, transposed=self.layout)

    def block_row_ptr(self):
        return self.rowptr


def of_oracle(m):
    return HostMatrix(m.num_rows, m.num_cols, m.keys, m.bmps, m.offsets, m.values, m.transposed)


def _good(layout):
    """21 x 27, ragged both ways, with tiles in the last block-row and the last block column and an empty block-row in between"""
    r = np.array([0, 3, 7, 2, 5, 16, 19, 20, 20, 18])
    c = np.array([1, 9, 26, 25, 0, 3, 24, 26, 8, 17])
    return Tiles((21, 27, r, c), layout)


@pytest.mark.parametrize("layout", [0, 1])
def test_check_container_accepts_and_rejects(layout):
    """a good handle passes; a hand-made bad array of each kind is rejected with the message of its own rule"""
    t = _good(layout)

    def make(keys=t.keys, bmps=t.bmps, offsets=t.offsets, values=t.values, **kw):
        return HostMatrix(21, 27, np.array(keys), np.array(bmps), np.array(offsets), values, layout, **kw)
    check_container(make())
    assert t.keys.size >= 6 and t.rowptr[2] == t.rowptr[1]         # the empty block-row 1

    def rejected(M, message):
        with pytest.raises(AssertionError, match=message):
            check_container(M)
    swapped = t.keys.copy()
    swapped[[1, 2]] = swapped[[2, 1]]
    rejected(make(keys=swapped), "strictly increasing")
    doubled = t.keys.copy()
    doubled[1] = doubled[0]
    rejected(make(keys=doubled), "strictly increasing")
    wide = t.keys.copy()
    wide[-1] = (np.uint64(2) << np.uint64(32)) | np.uint64(4)       # block column 4 of 4
    rejected(make(keys=wide), "block index outside")
    tall = t.keys.copy()
    tall[-1] = (np.uint64(3) << np.uint64(32)) | np.uint64(0)       # block-row 3 of 3
    rejected(make(keys=tall), "block index outside")
    last_row = int(np.flatnonzero((t.keys >> np.uint64(32)) == 2)[0])
    last_col = int(np.flatnonzero((t.keys & MASK32) == 3)[0])
    for tile, (row, col) in ((last_row, (5, 0)), (last_col, (0, 3))):   # row 21 of 21; column 27 of 27
        bad = t.bmps.copy()
        bad[tile] |= np.uint64(1) << np.uint64(63 - ((8 * col + row) if layout else (8 * row + col)))
        offs = np.concatenate([[0], np.cumsum(popcounts(bad))]).astype(np.uint64)
        rejected(make(bmps=bad, offsets=offs, values=np.append(t.values, 1.0)), "outside the ragged edge")
    inside = t.bmps.copy()                                          # (a bit more inside the edge only breaks the offsets)
    inside[last_row] |= np.uint64(1) << np.uint64(63 - ((8 * 7 + 4) if layout else (8 * 4 + 7)))
    assert popcounts(inside)[last_row] == popcounts(t.bmps)[last_row] + 1
    rejected(make(bmps=inside), "prefix sum")
    shifted = t.offsets.copy()
    shifted[2] += np.uint64(1)
    rejected(make(offsets=shifted), "prefix sum")
    rejected(make(nnz=int(t.offsets[-1]) + 1), "block_num")         # the value array's length against info()
    long_offsets = t.offsets.copy()
    long_offsets[-1] += np.uint64(1)
    rejected(make(offsets=long_offsets), "prefix sum")
    for at, step in ((1, 1), (2, -1), (3, 1), (0, 1)):              # off by one at a block-row, after the empty one, at the end, at the start
        ptr = t.rowptr.copy()
        ptr[at] += step
        rejected(make(rowptr=ptr), "block-row pointer")
    rejected(make(rowptr=t.rowptr[:-1]), "block-row pointer")
    empty = t.bmps.copy()
    empty[1] = 0
    offs = np.concatenate([[0], np.cumsum(popcounts(empty))]).astype(np.uint64)
    rejected(HostMatrix(21, 27, t.keys, empty, offs, t.values[:int(offs[-1])], layout), "empty bitmap")


def test_offsets_end_is_checked_against_nnz():
    """offsets[block_num] == nnz is a rule of its own: a handle whose info() reports another nnz than its offsets end in"""
    t = _good(0)
    M = HostMatrix(21, 27, t.keys, t.bmps, t.offsets, np.zeros(int(t.offsets[-1]) + 2), 0, nnz=int(t.offsets[-1]) + 2)
    with pytest.raises(AssertionError, match="offsets\\[block_num\\] != nnz"):
        check_container(M)


# ---- operand shapes -----------------------------------------------------------------------------------------------------------------------
N_BLOCK_ROWS, POS_W, POS_W2, W2 = 10, 6, 2, 40
EMPTY_ROWS = (0, 3, 4, 5, 9)
NBC1 = 134                    # block columns of C1: the last one holds its values in column 4 of the tile, the last column 8 * 134 - 3 keeps


def ragged_count(n):
    """the smallest number of block columns >= n whose last one holds its value (_col_in_tile) in a column that 8 * n - 3 columns keep"""
    while _col_in_tile(n - 1) > 4:
        n += 1
    return n


@functools.lru_cache(maxsize=None)
def first_product(w, a=4, seed=11):
    """(A1, B1) as COO; see the docstring of the file.  a: A tiles per block-row (B1's block-rows grow as a shrinks)"""
    assert W2 < w <= NBC1 and ragged_count(NBC1) == NBC1
    rng = np.random.default_rng(seed)

    def row(c, must=()):
        others = np.setdiff1d(np.arange(NBC1), must)
        S = rng.permutation(np.concatenate([np.asarray(must, np.int64), rng.choice(others, c - len(must), replace=False)]))
        n = min(a, c)
        return ("tiles", [np.concatenate([S[t::n], rng.choice(S, c // 2, replace=False)]) for t in range(n)])
    empty = ("tiles", [])
    rows = [empty, row(17), row(W2, (0,)), empty, empty, empty, row(w, (0, NBC1 - 1)), row(20), row(9), empty]
    assert len(rows) == N_BLOCK_ROWS and all((rows[i] == empty) == (i in EMPTY_ROWS) for i in range(N_BLOCK_ROWS))
    A, B, want = cap_product(rows, NBC1)
    assert want == {1: 17, POS_W2: W2, POS_W: w, 7: 20, 8: 9}
    A, B = (A[0] - 3,) + A[1:], (B[0], B[1] - 3) + B[2:]
    assert A[2].max() < A[0] and B[3].max() == B[1] - 1            # nothing is cut off, and the last column is in use
    return A, B


def second_operand(c1_keys, c1_cols, b, u, seed=5):
    """B2 as COO for a C1 with these keys and this many columns; see the docstring of the file"""
    rng = np.random.default_rng(seed)
    nbc1, nbc2 = -(-c1_cols // 8), ragged_count(u + u // 2)
    pool = np.concatenate([[0], 1 + np.sort(rng.choice(nbc2 - 2, u - 2, replace=False)), [nbc2 - 1]]).astype(np.int64)
    kcol = (c1_keys & MASK32).astype(np.int64)[(c1_keys >> np.uint64(32)).astype(np.int64) == POS_W]
    index = {int(k): i for i, k in enumerate(kcol)}
    few = 1 if b <= 2 else 2
    assert few < b <= u
    bk, bm = [], []
    for k in range(nbc1):
        m = np.unique((index[k] * b + np.arange(b)) % u if k in index else (7 * k + 3 * np.arange(few)) % u)
        bk.append(np.full(m.size, k, np.int64)); bm.append(pool[m])
    bk, bm = np.concatenate(bk), np.concatenate(bm)
    r, c = 8 * bk + _col_in_tile(bk), 8 * bm + _col_in_tile(bm)
    assert r.max() < c1_cols and c.max() < 8 * nbc2 - 3 and c.max() // 8 == nbc2 - 1     # nothing is cut off, and the last block column is in use
    return (c1_cols, 8 * nbc2 - 3, r, c, 1.0 + 0.5 * np.cos(0.9 * r + 0.31 * c))


PIPELINE = {"BMSP_SPGEMM_ROWMERGE": "0", "BMSP_MAC_ROWSPARSE": "0"}     # expand - sort - compress, a block-MAC kernel that reads the task list
CHAIN = {
    # name: (w, b, u, switches of the second product, its sort mode)
    "strip_on": (64, 4, 200, {}, 0),                                    # w * b = 256 = STRIP_ROW_CAP: surely_fits, strip mode without T_2
    "strip_above": (65, 4, 200, {}, 0),                                 # 260: T_2 first
    "kcap_on": (96, 2, 150, {"BMSP_MAC_ROWSPARSE": "0"}, 0),            # 2 w = 192 = K_CAP: the fp32 strip kernel
    "kcap_above": (97, 2, 150, {"BMSP_MAC_ROWSPARSE": "0"}, 0),         # 194: no strip kernel, so no strip mode: task-list mode
    "narrow_on": (64, 64, 128, PIPELINE, 1),                            # w * b = 4096 = NARROW_CAP: T_5 without a read-back
    "narrow_above": (65, 64, 128, PIPELINE, 1),                         # 4160, and a segment of 4160 tasks: the list kernels
    "seg_on": (128, 128, 256, dict(PIPELINE, BMSP_SEG_AVG_MAX="0"), 0),     # w * b = 16384: the clause keeps the segmented sort
    "seg_above": (129, 128, 256, dict(PIPELINE, BMSP_SEG_AVG_MAX="0"), 0),  # 16512: the global sort
    "rs_on": (70, 4, 256, {}, 0),                                       # C2's widest block-row 256 = rs_row_cap(9): strip mode, the small table
    "rs_above": (70, 4, 257, {}, 0),                                    # 257: task-list mode, the row-sparse kernel's larger table
}
C1_MAKERS = {
    # name: (switches of the first product, its sort mode, (sort_path, sort_long or None)): what leaves pointer + maximum, and what leaves neither
    "strip": ({"BMSP_SPGEMM_ROWMERGE": "1"}, 0, (2, 1)),
    "tasklist": ({"BMSP_SPGEMM_ROWMERGE": "2"}, 0, (2, 2)),
    "lazy": ({"BMSP_SPGEMM_ROWMERGE": "0"}, 1, (1, None)),
    "windows": ({"BMSP_SPGEMM_ROWWINDOW": "1", "BMSP_WIN_THIN": "1"}, 0, (3, None)),      # the pointer alone, the maximum left at -1
}


def kind_of(name):
    return name.split("_")[0]


def decision(name, w, b, c2_widest):
    """the one comparison of the second product that the case is about, as the sources make it, on a claimed widest block-row"""
    return {"strip": w * b <= STRIP_ROW_CAP, "kcap": 2 * w <= K_CAP, "narrow": 0 < w * b <= NARROW_CAP, "seg": 0 < w * b <= SEG_BOUND_MAX,
            "rs": c2_widest > RS_SMALL}[kind_of(name)]


def expected_route(name):
    """what the statistics of the second product must show: sort_path, sort_long (None: not stated), the mac_variants allowed (None: the
    case does not pin the kernel) and whether stage timer 2 is zero (None: T_2 always runs on that path)"""
    w, b, u, env, mode = CHAIN[name]
    kind, longest, widest = kind_of(name), w * b, min(u, w * b)
    if kind in ("strip", "rs"):
        strip = widest <= STRIP_ROW_CAP
        return dict(sort_path=2, sort_long=1 if strip else 2, mac_variant=(5,), t2_zero=w * b <= STRIP_ROW_CAP and strip)
    if kind == "kcap":
        return dict(sort_path=2, sort_long=1, mac_variant=(3,), t2_zero=True) if 2 * w <= K_CAP else dict(sort_path=2, sort_long=2, mac_variant=(0,), t2_zero=False)
    if kind == "seg" and w * b > SEG_BOUND_MAX:
        return dict(sort_path=0, sort_long=None, mac_variant=None, t2_zero=None)
    # test_zzz_spgemm_regimes.pipeline_path: no long segment up to the wave's (and the workgroup kernel's) 4096, pieces + merge passes up to four pieces
    assert longest <= 4 * NARROW_CAP
    return dict(sort_path=1, sort_long=0 if longest <= max(NARROW_CAP, BLOCK_SEG_MAX) else 1, mac_variant=None, t2_zero=None)


_MEMO = {}


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def oracle_first(oracle, w, a=4, dtype=0):
    """(A1, B1, the oracle's C1 and its statistics)"""
    def make():
        A, B = first_product(w, a)
        C, st = oracle.spgemm(oracle.bmsp_from_coo(oracle.Coo(*A), dtype, False), oracle.bmsp_from_coo(oracle.Coo(*B), dtype, True))
        return A, B, C, st
    return _memo(("first", w, a, dtype), make)


def oracle_chain(oracle, name):
    """(A1, B1, B2 as COO, the oracle's C1, C2 and the statistics of C2 = C1 x B2) of a chain case"""
    def make():
        w, b, u, _, _ = CHAIN[name]
        A, B, C1, _ = oracle_first(oracle, w)
        B2 = second_operand(C1.keys, C1.num_cols, b, u)
        C2, st = oracle.spgemm(C1, oracle.bmsp_from_coo(oracle.Coo(*B2), 0, True))
        return A, B, B2, C1, C2, st
    return _memo(("chain", name), make)


def row_counts(keys, nbr=N_BLOCK_ROWS):
    return np.bincount((keys >> np.uint64(32)).astype(np.int64), minlength=nbr)


def chain_terms(C1, B2):
    """every task of C1 x B2 in the expansion's order (C1's tiles in key order, the tiles of B2's block-row in column order), as
    product_terms of test_spgemm_regimes.py gives them for its own operands: segment, position, block column of C2, the two fp32 factors"""
    assert np.array_equal(C1.offsets, np.arange(C1.keys.size + 1))                     # one value per tile of C1
    a_bi, a_k = (C1.keys >> np.uint64(32)).astype(np.int64), (C1.keys & MASK32).astype(np.int64)
    _, _, r2, c2, v2 = B2
    o = np.lexsort((c2 // 8, r2 // 8))
    r2, c2, v2 = r2[o], c2[o], v2[o]
    assert np.all(np.diff(r2 // 8 * (1 << 32) + c2 // 8) > 0)                           # one value per tile of B2
    assert np.array_equal(r2 % 8, _col_in_tile(r2 // 8))                                # ... in the row C1's tiles hold theirs in
    assert np.all(popcounts(C1.bmps) == 1)
    pos = 63 - np.log2(C1.bmps.astype(np.float64)).astype(np.int64)
    assert np.array_equal(pos % 8, _col_in_tile(a_k))                                   # every candidate pair survives
    bptr = np.searchsorted(r2 // 8, np.arange(int(a_k.max()) + 2))
    cnt = bptr[a_k + 1] - bptr[a_k]
    ta = np.repeat(np.arange(a_k.size), cnt)
    tb = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(bptr[a_k], cnt)
    seg = a_bi[ta]
    return {"seg": seg, "pos": np.arange(seg.size) - np.searchsorted(seg, seg), "j": c2[tb] // 8, "a": C1.values[ta].astype(np.float32),
            "b": v2[tb].astype(np.float32), "max_b": int(np.diff(bptr).max())}


# ---- CPU self-checks ---------------------------------------------------------------------------------------------------------------------
def _check_first(C1, w):
    counts = row_counts(C1.keys)
    assert (C1.num_rows % 8, C1.num_cols % 8) == (5, 5) and -(-C1.num_rows // 8) == N_BLOCK_ROWS
    assert all(counts[i] == 0 for i in EMPTY_ROWS) and counts[0] == 0 and counts[-1] == 0 and np.all(counts[3:6] == 0)
    assert counts[POS_W] == w and np.sum(counts == w) == 1 and POS_W not in (0, N_BLOCK_ROWS - 1)
    assert counts[POS_W2] == W2 and np.sort(counts)[-2] == W2 < w
    assert int((C1.keys & MASK32).max()) == NBC1 - 1                                    # a tile in the ragged last block column
    check_container(of_oracle(C1), "the oracle's C1")


@pytest.mark.parametrize("name", sorted(CHAIN))
def test_chain_case_sits_where_w_decides(oracle, name):
    w, b, u, env, mode = CHAIN[name]
    A, B, B2, C1, C2, st = oracle_chain(oracle, name)
    _check_first(C1, w)
    t = chain_terms(C1, B2)
    assert t["max_b"] == b and st["task_list_size"] == st["surviving_tasks"] == t["seg"].size
    per_row = np.bincount(t["seg"], minlength=N_BLOCK_ROWS)
    assert per_row[POS_W] == w * b == per_row.max() and np.sum(per_row == w * b) == 1   # the widest block-row's segment is the bound itself
    c2 = row_counts(C2.keys)
    assert c2[POS_W] == min(u, w * b) == c2.max() and (np.sum(c2 == c2.max()) == 1 or kind_of(name) != "rs")
    check_container(of_oracle(C2), "the oracle's C2")
    assert (C2.num_cols % 8, int((C2.keys & MASK32).max())) == (5, -(-C2.num_cols // 8) - 1)
    # on / above: the decision at the true widest block-row, and at what an understated or stale maximum would claim
    above = name.endswith("_above")
    widest, second = int(c2.max()), int(np.sort(c2)[-2])
    if kind_of(name) == "rs":
        assert widest == RS_SMALL + above and decision(name, w, b, widest) == above
        assert not decision(name, w, b, second)
    else:
        bound = {"strip": STRIP_ROW_CAP, "kcap": K_CAP, "narrow": NARROW_CAP, "seg": SEG_BOUND_MAX}[kind_of(name)]
        assert (2 * w if kind_of(name) == "kcap" else w * b) - bound == (0 if not above else (2 if kind_of(name) == "kcap" else b))
        assert decision(name, w, b, widest) == (not above)
        assert decision(name, W2, b, widest)
    if above:
        assert decision(name, w, b, widest) != decision(name, W2, b, second)
    assert jbits(B2) + TASK_BLOCK_IDX_BITS <= 32                                        # narrow sort words: the wave's capacity is NARROW_CAP
    route = expected_route(name)
    if route["t2_zero"] is not None:
        assert route["t2_zero"] == (w * b <= STRIP_ROW_CAP and route["sort_long"] == 1)
    if kind_of(name) in ("strip", "kcap"):
        assert c2.max() <= STRIP_ROW_CAP                                                # strip mode, where it is allowed, fits
    # the order of the tasks inside a C2 tile shows in its bits
    s = order_sensitive(t)
    assert s["differs"].any(), name
    if kind_of(name) in ("narrow", "seg"):
        assert (s["differs"] & (s["seg"] == POS_W)).any()


def jbits(B):
    return max(1, int(-(-B[1] // 8) - 1).bit_length())


MAKER_W = 64


@pytest.mark.parametrize("a,surely", [(4, True), (8, False)])
def test_maker_pairs_sit_on_either_side_of_surely_fits(oracle, a, surely):
    """the first products of the maker cases: with four A tiles per block-row the row maxima bound every block-row of C1 by strip mode's
    256 (strip mode without T_2 on the first product), with eight they do not (T_2 runs, strip mode fits all the same)"""
    A, B, C1, st = oracle_first(oracle, MAKER_W, a)
    _check_first(C1, MAKER_W)
    t = product_terms(A, B)
    assert (t["max_a"], t["max_a"] * t["max_b"] <= STRIP_ROW_CAP) == (a, surely), (t["max_a"], t["max_b"])
    assert row_counts(C1.keys).max() <= STRIP_ROW_CAP and 2 * a <= K_CAP


def square_operand():
    """cusp's 5-point Poisson matrix on a 13 x 15 grid, 195 rows (ragged): its square has a full, positive diagonal"""
    from pybmsp import gen
    n, _, r, c, v = gen.poisson("5pt", 13, 15)
    return (n, n, np.asarray(r, np.int64), np.asarray(c, np.int64), np.asarray(v, np.float64))


def test_square_product_has_a_full_diagonal(oracle):
    S = square_operand()
    C, _ = oracle.spgemm(oracle.bmsp_from_coo(oracle.Coo(*S), 0, False), oracle.bmsp_from_coo(oracle.Coo(*S), 0, True))
    coo = oracle.bmsp_to_coo(C)
    d = np.zeros(S[0])
    on = coo.rows == coo.cols
    d[coo.rows[on]] = coo.vals[on]
    assert S[0] % 8 == 3 and np.all(d >= 17) and np.count_nonzero(on) == S[0]
    check_container(of_oracle(C), "the oracle's square product")
