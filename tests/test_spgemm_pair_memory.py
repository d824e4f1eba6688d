"""bmsp_spgemm's memory of what a pair of operands needs, against every call history: inputs, the table of histories, CPU self-checks.

bmsp_spgemm keeps on A's handle what the pair (A, B) turned out to need (csrc/matrix.h, rm_partner_*: whether strip mode fits, and which
path forms the task list otherwise), keyed by B's uid; the next product of the pair goes there directly, and the sharded and paneled
products copy the memory into every row-panel view and merge it back into the parent.  So the route a product takes -- and with it the
numeric kernel that computes its values -- depends on the calls made on the handles before it.  The GPU cases of
tests/test_zzzz_spgemm_pair_memory.py apply every history of HISTORIES to fresh handles of every pair below and then probe the pair.

Pairs (the smallest that show their mode; every property is asserted below, from the operands alone, against the caps that
test_spgemm_regimes.py reads out of the sources):

S  strip fit: gen.banded(203, 9) on both sides -- tiles more than a quarter full (the row-sparse kernel does not apply: strip mode means
   the strip kernel), every block-row of C within STRIP_ROW_CAP, 2 x the widest block-row of A within K_CAP.
R  row-sparse fit: gen.fem_like(10, "27pt") on both sides -- at most 16 stored values per tile on average, every block-row of C within
   STRIP_ROW_CAP: strip mode with the row-sparse kernel where V15's numerics are asked for.
T  task-list mode: three block-rows of C of 257 tiles between ordinary ones (cap_product of test_spgemm_regimes.py, smaller than its
   b_257 / c_* products and with three heavy block-rows, so that three row panels all hold work): the largest block-row of C lies in
   (STRIP_ROW_CAP, TL_CAP].
W  column windows: gen.rmat(13, 6), the R-MAT of test_structural_refusal_keeps_the_pair_hint with the smallest edge factor out of 4, 6,
   8, 12, 16 that still has a block-row of C beyond TL_CAP (909 tiles; with 4 the widest holds 873) -- a third of the candidate pairs,
   and of the oracle's time, of edge factor 16.  A block-row of B lies beyond STRIP_ROW_CAP (the strip pass refuses it unseen), the
   task-list pass runs and overflows.  That its fresh first product reports sort_path 3 is asserted on the GPU.
V  the whole fits, a view does not: three block-rows of A of 100 tiles (100 > K_CAP / 2 = 96: the strip kernel's k list refuses them)
   whose tiles hold 8 values, B tiles one value (nnz <= 16 block_num on both sides: the row-sparse kernel takes the whole product), every
   block-row of C of at most 200 <= STRIP_ROW_CAP tiles.  mac_rowsparse_applies refuses row-panel views, so a view of such an A has no
   structure-only numeric stage and leaves strip mode.  Such inputs exist under the caps: 100 A tiles of 8 values and ~101 one-value B
   tiles per block-row of B keep both fills at 8 and 1, and C's block-row is bounded by the 200-column pool whatever the 100 x 101
   candidate pairs are.

Values: multiples of 1/4 in [1/4, 1], both signs (the `exact` values of test_spgemm_regimes.py): fp16 holds every operand, every product
is a multiple of 1/16 and every C value's sum of magnitudes stays below 2^24 / 16 -- exact in fp32 in any order, so EVERY kernel that may
run gives the oracle's bits and a change of kernel cannot hide behind a tolerance.  There is no tolerance in these two files.

Partners: b2 is a right operand of another structure with the same number of rows that needs ANOTHER mode (for S, R, V: block-rows of
300 tiles -- beyond STRIP_ROW_CAP; for T, W: one tile per block-row on 64 block columns -- no block-row of C beyond 64 tiles); b3 is a
second handle built from b's own triples.  The CPU checks assert that A b and A b2 differ, so a product answered from the other
partner's C could not pass.
"""
import functools
import numpy as np
import pytest
import scipy.sparse as sp

from test_spgemm_regimes import STRIP_ROW_CAP, TL_CAP, K_CAP, TL_B_ROW_MAX, cap_product

SORT_AUTO, SORT_SEGMENTED, SORT_GLOBAL = 0, 1, 2
F32, F16 = 0, 1
ROWSPARSE_FILL = 16        # mac_rowsparse_applies: stored values per tile, on average, on both sides

PAIRS = ("S", "R", "T", "W", "V")
# (dtype, tc_version) under mode = BMSP_SORT_AUTO: tc_version 5 for fp32, both 4 and 5 for fp16
CONFIGS = ((F32, 5), (F16, 4), (F16, 5))

# history -> what the FIRST probe must report: "fresh" = what the first product of fresh handles reports, "steady" = what their second does
HISTORIES = {
    "none": "fresh",                 # nothing: a second set of fresh handles behaves as the first
    "other_tc": "steady",            # two products under the other tc_version
    "explicit_mode": "steady",       # one product under BMSP_SORT_SEGMENTED, one under BMSP_SORT_GLOBAL
    "symbolic_numeric": "steady",    # bmsp_spgemm_symbolic, then bmsp_spgemm_numeric twice
    "other_partner": "fresh",        # spgemm(a, b2): the memory is keyed by the partner
    "twin_partner": "fresh",         # spgemm(a, b3), b3 a second handle of b's structure: keyed by the handle's uid, not by the structure
    "writer_on_b": "steady",         # b's values doubled in place (bmsp_matrix_scale_values into b itself)
    "invalidate_b": "fresh",         # bmsp_matrix_invalidate(b, 1), nothing changed
    "invalidate_a": "fresh",
    "prepared": "fresh",             # a.prepare(3), b.prepare(3) before the first product: nothing is known about the pair yet
    "sharded": "steady",             # bmsp_spgemm_sharded on a loopback communicator of three: gathered, then owner-keeps
    "forced_panels": "steady",       # one product under BMSP_SPGEMM_FORCE_PANELS=1
    "user_views": "steady",          # the products of three a.row_panel(...) views with b
    "switch_off_strip": "steady",    # one product under BMSP_MAC_STRIP=0, one under BMSP_SPGEMM_ROWMERGE=2
}
# the histories that multiply (a, b) as a whole before the probe; after the others the first probe is the pair's first whole product
SUBSET = ("none", "other_tc", "other_partner", "sharded", "forced_panels", "invalidate_b")


def cases():
    """(pair, dtype, tc_version, history): the full cross on S and R, SUBSET on T, W and V"""
    out = []
    for pair in PAIRS:
        for dtype, tc in CONFIGS:
            for h in (HISTORIES if pair in ("S", "R") else SUBSET):
                out.append((pair, dtype, tc, h))
    return out


def exact_values(r, c, right):
    """multiples of 1/4 in [1/4, 1], both signs, by position (the rule of test_spgemm_regimes._assemble)"""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    if right:
        return ((r + c * 3) % 4 + 1) / 4.0 * np.where((r // 2 + c) % 2 == 0, 1.0, -1.0)
    return ((r * 3 + c) % 4 + 1) / 4.0 * np.where((r + c // 3) % 2 == 0, 1.0, -1.0)


def _wide_partner(n_rows):
    """block-row k holds 300 one-value tiles on distinct block columns out of 512: no block-row of C within STRIP_ROW_CAP"""
    k = np.repeat(np.arange((n_rows + 7) // 8), 300)
    j = (7 * k + 3 * np.tile(np.arange(300), (n_rows + 7) // 8)) % 512
    r = np.minimum(8 * k + (k + j) % 8, n_rows - 1)
    c = 8 * j + (5 * j + 3) % 8
    return n_rows, 8 * 512, r, c, exact_values(r, c, True)


def _narrow_partner(n_rows):
    """block-row k holds one one-value tile at block column k % 64: no block-row of C beyond 64 tiles"""
    k = np.arange((n_rows + 7) // 8)
    r = np.minimum(8 * k + k % 8, n_rows - 1)
    c = 8 * (k % 64) + (5 * k + 3) % 8
    return n_rows, 8 * 64, r, c, exact_values(r, c, True)


@functools.lru_cache(maxsize=None)
def operands(pair):
    """(A, B, B2): COO tuples (rows, cols, r, c, v); A in row-major tiles, B and B2 right operands"""
    from pybmsp import gen
    if pair in ("S", "R", "W"):
        n, _, r, c, _ = {"S": lambda: gen.banded(203, 9), "R": lambda: gen.fem_like(10, "27pt"), "W": lambda: gen.rmat(13, 6)}[pair]()
        A = (n, n, r, c, exact_values(r, c, False))
        B = (n, n, r, c, exact_values(r, c, True))
    else:
        heavy = (4, 257, "all") if pair == "T" else (100, 200, "all")
        A, B, _ = cap_product([heavy, (3, 40, "all"), heavy, (2, 17, "all"), heavy, (5, 200, "all")], 1 << 12, exact=True, seed=5)
    B2 = _narrow_partner(A[1]) if pair in ("T", "W") else _wide_partner(A[1])
    return A, B, B2


def scaled(coo, factor):
    return coo[:4] + (np.asarray(coo[4]) * factor,)


_ORACLE = {}


def oracle_product(oracle, pair, dtype, tc, partner="b", b_scale=1.0):
    """(C, counters) of the oracle for A x (b_scale * B or B2), computed once per session and left unchanged"""
    mfma = tc != 5 and dtype == F16
    key = (pair, dtype, mfma, partner, b_scale)
    if key not in _ORACLE:
        A, B, B2 = operands(pair)
        right = scaled(B if partner == "b" else B2, b_scale)
        _ORACLE[key] = oracle.spgemm(oracle.bmsp_from_coo(oracle.Coo(*A), dtype, False), oracle.bmsp_from_coo(oracle.Coo(*right), dtype, True), exact_products=mfma)
    return _ORACLE[key]


# ---- CPU self-checks ---------------------------------------------------------------------------------------------------------------------
def _csr(coo, absolute=False):
    v = np.abs(coo[4]) if absolute else coo[4]
    return sp.csr_matrix((v, (coo[2], coo[3])), shape=coo[:2])


def _tiles(coo):
    """(tiles, stored values, tiles per block-row)"""
    key = np.unique(np.asarray(coo[2], np.int64) // 8 * (1 << 32) + np.asarray(coo[3], np.int64) // 8)
    nnz = np.unique(np.asarray(coo[2], np.int64) * (1 << 32) + np.asarray(coo[3], np.int64)).size
    return key.size, nnz, np.bincount(key >> 32, minlength=(coo[0] + 7) // 8)


def _c_block_rows(A, B):
    """C tiles per block-row of A x B: the tiles that hold a structural non-zero (magnitudes: nothing cancels)"""
    C = (_csr(A, True) @ _csr(B, True)).tocoo()
    key = np.unique(C.row.astype(np.int64) // 8 * (1 << 32) + C.col.astype(np.int64) // 8)
    return np.bincount(key >> 32, minlength=(A[0] + 7) // 8)


def _sparse_tiles(coo):
    tiles, nnz, _ = _tiles(coo)
    return nnz <= ROWSPARSE_FILL * tiles


@pytest.mark.parametrize("pair", PAIRS)
def test_pair_is_what_it_claims(pair):
    """the structural properties the docstring of the file states, from the operands and the caps of the sources"""
    A, B, B2 = operands(pair)
    assert A[1] == B[0] == B2[0]
    (ta, na, rows_a), (tb, nb, rows_b) = _tiles(A), _tiles(B)
    c_rows = _c_block_rows(A, B)
    if pair == "S":
        assert na > ROWSPARSE_FILL * ta and nb > ROWSPARSE_FILL * tb                   # more than a quarter full: not the row-sparse kernel
        assert c_rows.max() <= STRIP_ROW_CAP and 2 * rows_a.max() <= K_CAP
        assert rows_a.max() * rows_b.max() <= STRIP_ROW_CAP                             # (the row maxima alone bound C: the pass runs without T_2)
    if pair == "R":
        assert _sparse_tiles(A) and _sparse_tiles(B)
        assert c_rows.max() <= STRIP_ROW_CAP and 2 * rows_a.max() <= K_CAP              # (under tc_version 4 the fp16 strip kernel takes it)
    if pair == "T":
        assert STRIP_ROW_CAP < c_rows.max() <= TL_CAP and rows_b.max() <= STRIP_ROW_CAP  # the strip pass runs and overflows
        assert sorted(c_rows.tolist()) == [17, 40, 200, 257, 257, 257]
    if pair == "W":
        # the strip pass refuses B's widest block-row unseen, the task-list pass runs and a block-row of C overflows it; the windows' column range
        assert STRIP_ROW_CAP < rows_b.max() <= TL_B_ROW_MAX and c_rows.max() > TL_CAP and A[1] // 8 < (1 << 20)
    if pair == "V":
        assert _sparse_tiles(A) and _sparse_tiles(B)
        assert 2 * rows_a.max() > K_CAP and np.sum(2 * rows_a > K_CAP) == 3 and c_rows.max() <= STRIP_ROW_CAP
        # fp32: every product of stored values a normal number (biased exponents summing to >= 128): both operands within [1/4, 1]
        assert np.abs(A[4]).min() >= 0.25 and np.abs(B[4]).min() >= 0.25
    if pair in ("T", "V"):   # three row panels balanced by candidate pairs all hold a heavy block-row
        cand = np.asarray((_pattern(A) @ _pattern(B)).sum(axis=1)).ravel()
        third = np.searchsorted(np.cumsum(cand), [cand.sum() / 3.0, 2 * cand.sum() / 3.0])
        assert 0 < third[0] < third[1] < cand.size - 1, (cand, third)
    # the other partner needs another mode
    c2 = _c_block_rows(A, B2)
    if pair in ("S", "R", "V"):
        assert _tiles(B2)[2].max() > STRIP_ROW_CAP and c2.max() <= TL_CAP
    else:
        assert c2.max() <= 64 <= STRIP_ROW_CAP and _sparse_tiles(B2)


def _pattern(coo):
    """tile pattern as a 0 / 1 matrix of block-rows x block columns"""
    key = np.unique(np.asarray(coo[2], np.int64) // 8 * (1 << 32) + np.asarray(coo[3], np.int64) // 8)
    return sp.csr_matrix((np.ones(key.size), (key >> 32, key & 0xffffffff)), shape=((coo[0] + 7) // 8, (coo[1] + 7) // 8))


@pytest.mark.parametrize("pair", PAIRS)
def test_values_are_exact(pair):
    """multiples of 1/4 up to 1 that fp16 holds; the largest sum of magnitudes of a C value, counted in units of 1/16, stays below 2^24:
    every partial sum is representable in fp32 in any order -- also after the writer's doubling of B"""
    A, B, B2 = operands(pair)
    for right in (B, B2, scaled(B, 2.0)):
        for v in (A[4], right[4]):
            assert np.array_equal(v * 4, np.round(v * 4)) and 0.25 <= np.abs(v).min() and np.abs(v).max() <= 2
            assert np.array_equal(np.asarray(v).astype(np.float16).astype(np.float64), v)
        mag = (_csr(A, True) @ _csr(right, True)).max()
        assert mag * 16 < 2 ** 24, mag


@pytest.mark.parametrize("pair", PAIRS)
def test_partners_give_other_products(pair):
    """A b, A b2 and A (2 b) differ in at least one C value: a product answered from the other partner's (or the unscaled) C cannot pass"""
    A, B, B2 = operands(pair)
    C, C2 = _csr(A) @ _csr(B), _csr(A) @ _csr(B2)
    n = max(C.shape[1], C2.shape[1])
    C.resize((C.shape[0], n)); C2.resize((C2.shape[0], n))
    assert abs(C - C2).max() > 0 and abs(C).max() > 0
    assert not np.array_equal(np.unique(B[2].astype(np.int64) // 8 * (1 << 32) + B[3] // 8), np.unique(B2[2].astype(np.int64) // 8 * (1 << 32) + B2[3] // 8))


def test_case_table():
    """the full cross on S and R, the subset elsewhere; every history has its rule"""
    cs = cases()
    assert len(cs) == len(set(cs)) == 2 * 3 * len(HISTORIES) + 3 * 3 * len(SUBSET)
    assert set(SUBSET) <= set(HISTORIES) and set(HISTORIES.values()) == {"fresh", "steady"}
    assert [h for h, rule in HISTORIES.items() if rule == "fresh"] == ["none", "other_partner", "twin_partner", "invalidate_b", "invalidate_a", "prepared"]


def test_oracle_agrees_with_the_structure(oracle):
    """the oracle's C of the smallest pair holds the block-rows counted above (the count is the structure the caps are compared with)"""
    for dtype, tc in CONFIGS:
        C, st = oracle_product(oracle, "S", dtype, tc)
        A, B, _ = operands("S")
        assert np.array_equal(np.bincount((C.keys >> np.uint64(32)).astype(np.int64), minlength=(A[0] + 7) // 8), _c_block_rows(A, B))
        assert np.array_equal(np.asarray(C.values, np.float64), np.asarray(C.values, np.float64).astype(np.float32))
