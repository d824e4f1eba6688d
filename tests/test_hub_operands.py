"""Operands with a hub block-row at the row-sparse kernel's limit, and sharded products whose later rounds outgrow the first allocation:
the generators, the table of cases and the CPU self-checks.  The GPU cases that run them live in tests/test_zzzzzzz_hub_operands.py.

A.  The row-sparse block-MAC (blockmac_rowsparse.hip) multiplies from a CSR copy that rs_count_kernel / rs_fill_kernel build straight from
the tiles: one wave per block-row, 64 tiles per step, the eight row counts of a step in 16-bit fields (four to a 64-bit word), a carry
from step to step.  A block-row of 8192 tiles or more could overflow a field, so such a matrix has no copy (mac_choice.h kRsRowBlocksEnd)
and the rule's per-operand half (mac_rowsparse_operand, asked for a product and by prepare_spgemm_operand) says so before ensure_csr32 is reached.

steps             A: 11 block-rows of 0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193 tiles -- both sides of every 64-tile step and of every
                  carry; B: 193 block-rows whose lengths cycle through the same list inside 256 block columns (layout 1: the copy goes
                  through tile_transpose).  Tiles hold 1 .. 5 values at positions drawn per tile, generic values (multiples of 1/64): a
                  value placed one slot off, or a row whose entries are out of column order, changes the bits of C.  Rows and columns
                  are no multiples of 8.
hub_a(L)          A: a block-row of L tiles of 1 or 2 values and one of 3 tiles; B: 8 L rows x 64 columns, one tile per block-row.
hub_b_untouched(L) B: one block-row (k0) of L tiles, every other one short; A stores nothing in block column k0.
hub_b_filtered(L) the same B; A has one tile in block column k0 with values in tile column 0 only, B's hub tiles have values in tile row
                  1 only: all L candidate pairs die in the bitmap filter.
full_rows         hub_a(8191) with every tile of the hub block-row holding all 8 values of tile rows 2, 3 (two adjacent 16-bit fields
                  reach 65528 = 8 x 8191 each) and 7 (the last field of the second word); above 16 values per tile: BMSP_MAC_ROWSPARSE=1.
The hub cases hold small positive integers by position (A 1 .. 7, B 1 .. 3): every product is exact in fp16, every sum stays below 2^24
and is exact in fp32 in any order -- a mismatch is never summation order, and every lost, duplicated or misplaced entry changes a sum.

B.  spgemm_sharded (comm.hip) allocates the whole C after round 0 as base + the round's size x rounds left x 1.25 + 1024 and grows by
copy when a later round does not fit.  partition_rows balances CANDIDATE pairs, so:
grow_tiles        64 block-rows with 64 candidates and 8 C tiles each, then 512 block-rows with 8 candidates and 8 C tiles each: the
                  first half of the work holds 512 of C's 4608 tiles, round 0 sizes the tile arrays far too small.
grow_values       64 block-rows whose pairs give one value per C tile, then 64 whose pairs give 64: the tiles fit, the values do not.
growth_events() restates the rule (its two constants read from comm.hip) and EXPECTED_GROWTH states, per (P, rounds), in which round
which resource outgrows its allocation -- the GPU cases must find the same from the library's own partition and C."""
import functools
import os
import re
import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "csrc")

RS_ROW_BLOCKS_END = 8192        # mac_choice.h kRsRowBlocksEnd: the first block-row length without a CSR copy
RS_FILL_MAX = 16                # mac_choice.h kRsFillMax: stored values per tile on average, per operand
RS_C_ROW_MAX = 256              # strip mode's bound on a block-row of C (mac_choice.h rs_row_cap(9))
GROW_FACTOR, GROW_SLACK = 1.25, 1024    # comm.hip spgemm_sharded: nb_cap / nz_cap
STEP_LENS = [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193]
HUB_LS = (8191, 8192, 8193)
HUB_K0 = 17                     # the hub block-row of B in the hub_b cases


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_constants_match_sources():
    """the limit is named once (mac_choice.h) and used by the rule's per-operand half -- which the gate and prepare both ask -- and by the
    guard; the fill rule; the sharded product's rule"""
    rule = _src("mac_choice.h")
    m = re.findall(r"constexpr int64_t kRsRowBlocksEnd = 1 << (\d+);", rule)
    assert len(m) == 1 and 1 << int(m[0]) == RS_ROW_BLOCKS_END
    rs, bld = _src("blockmac_rowsparse.hip"), _src("builder.hip")
    assert len(re.findall(r"if \(m\.max_row_blocks >= kRsRowBlocksEnd\) return 0;", rule)) == 1
    assert re.search(r"if \(m->max_row_blocks >= kRsRowBlocksEnd\) fail\(BMSP_ERR_LIMIT", rs)
    # the gate (mac_choose, through Eval::rowsparse) and prepare ask that half and spell no rule of their own
    assert len(re.findall(r"mac_rowsparse_operand\(f\.a, f\.sw\) != 1 \|\| mac_rowsparse_operand\(f\.b, f\.sw\) != 1", rule)) == 1
    assert re.search(r"const int rs = mac_rowsparse_operand\(m, sw\);", rule) and re.search(r"mac_prepare_forms\(mac_operand_facts\(m\)", bld)
    assert "max_row_blocks" not in bld.split("void prepare_spgemm_operand")[1].split("\n}\n")[0]
    assert "1 << 13" not in rs and "1 << 13" not in bld and rule.count("1 << 13") == 1
    # (a lane of rs_count_kernel, a step of rs_fill_kernel: 8 values per tile and row, fields of 16 bits)
    assert 8 * (RS_ROW_BLOCKS_END - 1) < 1 << 16 <= 8 * RS_ROW_BLOCKS_END
    assert re.search(r"constexpr int64_t kRsFillMax = %d;" % RS_FILL_MAX, rule) and re.search(r"m\.nnz <= kRsFillMax \* m\.block_num", rule)
    assert re.search(r"rs_row_cap\(int hb\) \{ return hb == 9 \? %du" % RS_C_ROW_MAX, rule)
    comm = _src("comm.hip")
    for res in ("b", "z"):
        m = re.search(r"n%s_cap = std::max<int64_t>\(need_%s, base_%s \+ \(int64_t\)\(\(double\)%s0\[\(size_t\)P\] \* left \* ([0-9.]+)\) \+ (\d+)\);" % (res, res, res, res), comm)
        assert m and float(m.group(1)) == GROW_FACTOR and int(m.group(2)) == GROW_SLACK
    assert re.search(r"if \(need_b > cap_b \|\| need_z > cap_z \|\| !C->keys\)", comm)


# ---- from the operands alone (numpy) -------------------------------------------------------------------------------------------------------
def tiles_of(M):
    """the tiles of a COO operand (rows, cols, r, c, v), in key order: block-row, block column, 8 x 8 pattern, stored values"""
    _, _, r, c, _ = M
    key = (r // 8).astype(np.int64) * (1 << 32) + c // 8
    u, inv = np.unique(key, return_inverse=True)
    pat = np.zeros((u.size, 8, 8), bool)
    pat[inv, r % 8, c % 8] = True
    assert int(pat.sum()) == r.size      # no coordinate twice
    return {"bi": u >> 32, "bj": u & 0xffffffff, "pat": pat, "nnz": pat.sum((1, 2))}


def row_lengths(M):
    """tiles per block-row, for every block-row of the matrix"""
    t = tiles_of(M)
    return np.bincount(t["bi"], minlength=(M[0] + 7) // 8)


def mean_fill(M):
    t = tiles_of(M)
    return M[2].size / t["bi"].size


def pairs_of(A, B):
    """every candidate pair of A x B in the expansion's order: block-row and block column of its C tile, whether it survives the bitmap
    filter (a tile column of A with a value whose tile row of B holds one), and the pattern it contributes"""
    ta, tb = tiles_of(A), tiles_of(B)
    n_k = max((A[1] + 7) // 8, (B[0] + 7) // 8)
    bptr = np.searchsorted(tb["bi"], np.arange(n_k + 1))
    cnt = bptr[ta["bj"] + 1] - bptr[ta["bj"]]
    ia = np.repeat(np.arange(ta["bi"].size), cnt)
    ib = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(bptr[ta["bj"]], cnt)
    alive = np.any(ta["pat"].any(1)[ia] & tb["pat"].any(2)[ib], axis=1)
    return {"i": ta["bi"][ia], "j": tb["bj"][ib], "alive": alive, "ia": ia, "ib": ib, "ta": ta, "tb": tb,
            "per_row": np.bincount(ta["bi"], weights=cnt, minlength=(A[0] + 7) // 8).astype(np.int64)}


def c_structure(A, B):
    """C = A x B as the library stores it, from the patterns: per block-row of A the C tiles and the stored C values"""
    p = pairs_of(A, B)
    a = p["alive"]
    key = p["i"][a] * (1 << 32) + p["j"][a]
    u, inv = np.unique(key, return_inverse=True)
    prod = np.einsum("nik,nkj->nij", p["ta"]["pat"][p["ia"][a]].astype(np.uint8), p["tb"]["pat"][p["ib"][a]].astype(np.uint8)) > 0
    pat = np.zeros((u.size, 8, 8), bool)
    np.logical_or.at(pat, inv, prod)
    nbr = (A[0] + 7) // 8
    return {"tiles": np.bincount(u >> 32, minlength=nbr), "values": np.bincount(u >> 32, weights=pat.sum((1, 2)), minlength=nbr).astype(np.int64),
            "candidates": p["per_row"], "filtered": int((~a).sum())}


def candidate_bounds(per_row, parts):
    """partition_rows (shard.hip): the first block-row at which the candidate pairs in front reach p / parts of all of them"""
    cum = np.concatenate([[0], np.cumsum(per_row)]).astype(object)
    total, nbr = int(cum[-1]), len(per_row)
    assert total > 0
    bounds, r = [0], 0
    for p in range(1, parts):
        target = total * p // parts
        while r < nbr and cum[r] < target:
            r += 1
        bounds.append(r)
    bounds.append(nbr)
    return np.maximum.accumulate(np.asarray(bounds, dtype=np.int64))


def growth_events(panel_tiles, panel_values, P, rounds):
    """spgemm_sharded's allocation rule on the sizes of the rounds * P panels: [(round, tiles outgrown, values outgrown)] for every round
    after the first that takes the grow-by-copy branch"""
    cap_b = cap_z = base_b = base_z = 0
    events = []
    for k in range(rounds):
        size_b, size_z = int(np.sum(panel_tiles[k * P:(k + 1) * P])), int(np.sum(panel_values[k * P:(k + 1) * P]))
        need_b, need_z = base_b + size_b, base_z + size_z
        if need_b > cap_b or need_z > cap_z or k == 0:
            if k:
                events.append((k, need_b > cap_b, need_z > cap_z))
            left = rounds - k
            cap_b = max(need_b, base_b + int(size_b * left * GROW_FACTOR) + GROW_SLACK)
            cap_z = max(need_z, base_z + int(size_z * left * GROW_FACTOR) + GROW_SLACK)
        base_b, base_z = need_b, need_z
    return events


def panel_sums(per_row, bounds):
    c = np.concatenate([[0], np.cumsum(per_row)])
    return c[bounds[1:]] - c[bounds[:-1]]


# ---- generators ----------------------------------------------------------------------------------------------------------------------------
def _coo(rows, cols, r, c, v):
    r, c, v = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64), np.asarray(v, dtype=np.float64)
    assert r.size and 0 <= r.min() and r.max() < rows and 0 <= c.min() and c.max() < cols
    return (int(rows), int(cols), r, c, v)


def _int_values(r, c, top):
    return 1.0 + (3 * r + 5 * c + r // 8) % top


def _from_tiles(bi, bj, rr, cc, rows, cols, top):
    """one value per (tile, slot): block-row, block column, row and column inside the tile; integer values 1 .. top by position"""
    r, c = 8 * np.asarray(bi, dtype=np.int64) + rr, 8 * np.asarray(bj, dtype=np.int64) + cc
    key = np.unique(r * (1 << 32) + c)
    r, c = key >> 32, key & 0xffffffff
    return _coo(rows, cols, r, c, _int_values(r, c, top))


def _sparse_tiles(rng, bi, bj, rows, cols, lo=1, hi=5):
    """lo .. hi values per tile at positions drawn per tile; generic values, multiples of 1/64, none zero.  A coordinate beyond a ragged
    edge moves four rows / columns back: it stays in its tile (an edge cuts at most three)"""
    n = bi.size
    count = rng.integers(lo, hi + 1, n)
    slot = np.argsort(rng.random((n, 64)), axis=1)[:, :hi]
    keep = np.arange(hi)[None, :] < count[:, None]
    t = np.repeat(np.arange(n), hi).reshape(n, hi)[keep]
    s = slot[keep]
    r, c = 8 * bi[t] + s // 8, 8 * bj[t] + s % 8
    r, c = np.where(r >= rows, r - 4, r), np.where(c >= cols, c - 4, c)
    key = np.unique(r * (1 << 32) + c)
    v = np.round(rng.standard_normal(key.size) * 64) / 64
    v[v == 0] = 1 / 64
    return _coo(rows, cols, key >> 32, key & 0xffffffff, v)


def steps_product():
    rng = np.random.default_rng(11)
    n_k, nbc = STEP_LENS[-1], 256
    a_bi = np.repeat(np.arange(len(STEP_LENS)), STEP_LENS)
    a_bj = np.concatenate([np.sort(rng.choice(n_k, n, replace=False)) for n in STEP_LENS])
    b_len = [STEP_LENS[k % len(STEP_LENS)] for k in range(n_k)]
    b_bi = np.repeat(np.arange(n_k), b_len)
    b_bj = np.concatenate([np.sort(rng.choice(nbc, n, replace=False)) for n in b_len])
    A = _sparse_tiles(rng, a_bi, a_bj, 8 * len(STEP_LENS) - 3, 8 * n_k - 2)
    B = _sparse_tiles(rng, b_bi, b_bj, 8 * n_k - 2, 8 * nbc - 3)
    return A, B


def _narrow_b(L, per_row=1):
    """8 L rows x 64 columns, `per_row` tiles per block-row of 1 or 2 values; tile k holds a value in the tile row that A's tile k has its
    first value's column in (_hub_row_a): the pair survives"""
    k = np.repeat(np.arange(L), per_row)
    j = (5 * k + k // 8 + 3 * np.tile(np.arange(per_row), L)) % 8
    first = (k, j, (3 * k + 1) % 8, (k // 3 + j) % 8)
    odd = k % 3 == 0
    second = (k[odd], j[odd], (3 * k[odd] + 5) % 8, (k[odd] + 1) % 8)
    return _from_tiles(*(np.concatenate(x) for x in zip(first, second)), 8 * L, 64, 3)


def _hub_row_a(L, full):
    """block-row 0: L tiles (every block column); block-row 1: 3 tiles.  Sparse: 1 or 2 values per tile; full: tile rows 2, 3 and 7 whole"""
    k = np.arange(L)
    if full:
        bi, bj = np.zeros(24 * L, np.int64), np.repeat(k, 24)
        rr, cc = np.tile(np.repeat([2, 3, 7], 8), L), np.tile(np.arange(8), 3 * L)
    else:
        odd = k % 2 == 1
        bi, bj = np.zeros(L + int(odd.sum()), np.int64), np.concatenate([k, k[odd]])
        rr, cc = np.concatenate([k % 8, (k[odd] + 3) % 8]), np.concatenate([(3 * k + 1) % 8, (5 * k[odd] + 2) % 8])
    k1 = np.array([1, L // 2, L - 2])
    bi, bj = np.concatenate([bi, np.ones(6, np.int64)]), np.concatenate([bj, k1, k1])
    rr, cc = np.concatenate([rr, (k1 + 1) % 8, (k1 + 4) % 8]), np.concatenate([cc, (3 * k1 + 1) % 8, (3 * k1 + 5) % 8])
    return _from_tiles(bi, bj, rr, cc, 16, 8 * L, 7)


def hub_a_product(L, full=False):
    return _hub_row_a(L, full), _narrow_b(L)


def hub_b_product(L, filtered):
    n_i, n_k = 24, 40
    k_short = np.array([k for k in range(n_k) if k != HUB_K0])
    # B: the hub block-row, values in tile row 1 only; two tiles in every other block-row
    j = np.arange(L)
    odd = j % 2 == 1
    hub = (np.full(L + int(odd.sum()), HUB_K0), np.concatenate([j, j[odd]]), np.ones(L + int(odd.sum()), np.int64), np.concatenate([j % 8, (j[odd] + 3) % 8]))
    sk = np.repeat(k_short, 2)
    sj = (sk * 211 + np.tile([0, 4099], k_short.size)) % L
    short = (np.concatenate([sk, sk[::2]]), np.concatenate([sj, sj[::2]]), np.concatenate([(3 * sk) % 8, (3 * sk[::2] + 2) % 8]),
             np.concatenate([(sj + sk) % 8, (sj[::2] + 3) % 8]))
    B = _from_tiles(*(np.concatenate(x) for x in zip(hub, short)), 8 * n_k, 8 * L, 3)
    # A: three tiles per block-row at short block-rows of B, one value in tile column 3 k % 8 (B's short tiles have one in that row)
    i = np.repeat(np.arange(n_i), 3)
    k = k_short[(7 * i + 13 * np.tile(np.arange(3), n_i)) % k_short.size]
    a = (np.concatenate([i, i[::2]]), np.concatenate([k, k[::2]]), np.concatenate([(i + k) % 8, (i[::2] + 2 * k[::2] + 1) % 8]),
         np.concatenate([(3 * k) % 8, (3 * k[::2] + 2) % 8]))
    if filtered:    # one tile in block column k0, values in tile column 0 only
        a = tuple(np.concatenate([x, y]) for x, y in zip(a, ([5, 5], [HUB_K0, HUB_K0], [2, 5], [0, 0])))
    A = _from_tiles(*a, 8 * n_i, 8 * n_k, 7)
    return A, B


def second_partner(L):
    """a right operand for hub_a's A with two tiles per block-row: with a short-rowed A the product takes the row-sparse kernel"""
    return _narrow_b(L, per_row=2)


def short_a(L):
    """block-row 1 of hub_a's A alone (its 3 tiles), same dimensions"""
    rows, cols, r, c, v = _hub_row_a(L, False)
    m = r >= 8
    return (rows, cols, r[m], c[m], v[m])


def _generic(rng, n):
    """multiples of 1/64 in [1/4, 5/4]: fp16 holds them, products are multiples of 2^-12 below 2^-12 * 6400"""
    return np.round(rng.uniform(0.25, 1.25, n) * 64) / 64


def grow_tiles_product():
    rng = np.random.default_rng(5)
    m_top, n_bot, nbc = 64, 512, 32
    a_bi = np.concatenate([np.repeat(np.arange(m_top), 8), m_top + np.arange(n_bot)])
    a_bj = np.concatenate([np.tile(np.arange(8), m_top), 8 + np.arange(n_bot)])
    # A tiles: two values; B tiles: one value in every tile row (whatever column of A holds a value, the pair survives)
    ar = np.concatenate([8 * a_bi + (a_bi + a_bj) % 8, 8 * a_bi + (a_bi + 3 * a_bj + 1) % 8])
    ac = np.concatenate([8 * a_bj + (3 * a_bj + a_bi) % 8, 8 * a_bj + (3 * a_bj + a_bi + 4) % 8])
    b_bi = np.concatenate([np.repeat(np.arange(8), 8), np.repeat(8 + np.arange(n_bot), 8)])
    b_bj = np.concatenate([np.tile(3 + 2 * np.arange(8), 8), (np.repeat(np.arange(n_bot), 8) + 4 * np.tile(np.arange(8), n_bot)) % nbc])
    br = np.repeat(8 * b_bi, 8) + np.tile(np.arange(8), b_bi.size)
    bc = np.repeat(8 * b_bj, 8) + (np.tile(np.arange(8), b_bi.size) + np.repeat(b_bi + b_bj, 8)) % 8
    return (_coo(8 * (m_top + n_bot), 8 * (8 + n_bot), ar, ac, _generic(rng, ar.size)), _coo(8 * (8 + n_bot), 8 * nbc, br, bc, _generic(rng, br.size)))


def grow_values_product():
    rng = np.random.default_rng(6)
    half, nbc = 64, 32
    i = np.arange(2 * half)
    b_bi, b_bj = np.repeat(i, 8), (np.repeat(i, 8) + 4 * np.tile(np.arange(8), i.size)) % nbc
    top_a, top_b = i < half, b_bi < half
    full = np.arange(64)
    ar = np.concatenate([8 * i[top_a] + i[top_a] % 8, np.repeat(8 * i[~top_a], 64) + np.tile(full // 8, half)])
    ac = np.concatenate([8 * i[top_a] + (3 * i[top_a]) % 8, np.repeat(8 * i[~top_a], 64) + np.tile(full % 8, half)])
    nb = int((~top_b).sum())
    br = np.concatenate([8 * b_bi[top_b] + (3 * b_bi[top_b]) % 8, np.repeat(8 * b_bi[~top_b], 64) + np.tile(full // 8, nb)])
    bc = np.concatenate([8 * b_bj[top_b] + (b_bj[top_b] + b_bi[top_b]) % 8, np.repeat(8 * b_bj[~top_b], 64) + np.tile(full % 8, nb)])
    return (_coo(16 * half, 16 * half, ar, ac, _generic(rng, ar.size)), _coo(16 * half, 8 * nbc, br, bc, _generic(rng, br.size)))


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
HUB_CASES = [(kind, L) for kind in ("hub_a", "hub_b_untouched", "hub_b_filtered") for L in HUB_LS]
SHARD_RUNS = [(2, 2), (2, 4), (3, 3)]
# (P, rounds) -> [(round, tiles outgrown, values outgrown)], worked out by hand from the rule in the docstrings of the tests below
EXPECTED_GROWTH = {
    "grow_tiles": {(2, 2): [(1, True, True)], (2, 4): [(2, True, False)], (3, 3): [(2, True, True)], (8, 4): [(2, True, False)]},
    "grow_values": {(2, 2): [(1, False, True)], (2, 4): [(2, False, True)], (3, 3): [(1, False, True), (2, False, True)]},
}


@functools.lru_cache(maxsize=None)
def case(kind, L=0):
    """(A, B) as COO tuples (rows, cols, r, c, v); B is built in layout 1 by the tests"""
    if kind == "steps":
        return steps_product()
    if kind == "hub_a":
        return hub_a_product(L)
    if kind == "full_rows":
        return hub_a_product(L, full=True)
    if kind in ("hub_b_untouched", "hub_b_filtered"):
        return hub_b_product(L, kind == "hub_b_filtered")
    return {"grow_tiles": grow_tiles_product, "grow_values": grow_values_product}[kind]()


def hub_side(kind):
    return 0 if kind in ("hub_a", "full_rows") else 1


# ---- CPU self-checks -----------------------------------------------------------------------------------------------------------------------
def test_steps_is_what_it_claims(oracle):
    A, B = case("steps")
    assert row_lengths(A).tolist() == STEP_LENS
    assert row_lengths(B).tolist() == [STEP_LENS[k % len(STEP_LENS)] for k in range(STEP_LENS[-1])]
    assert A[0] % 8 and A[1] % 8 and B[1] % 8 and A[1] == B[0] and (B[1] + 7) // 8 == RS_C_ROW_MAX
    for M in (A, B):
        n = tiles_of(M)["nnz"]
        assert n.min() >= 1 and n.max() <= 5 and set(range(1, 6)) <= set(n.tolist())
        assert np.array_equal(M[4] * 64, np.round(M[4] * 64)) and np.all(M[4] != 0) and np.abs(M[4]).max() < 8
        assert np.array_equal(M[4].astype(np.float16).astype(np.float64), M[4])
    c = c_structure(A, B)
    assert c["tiles"].max() <= RS_C_ROW_MAX and c["tiles"][0] == 0 and c["tiles"][1:].min() > 0
    # ... and the oracle counts what numpy counts
    oc, st = oracle.spgemm(oracle.bmsp_from_coo(oracle.Coo(*A), 0, False), oracle.bmsp_from_coo(oracle.Coo(*B), 0, True))
    assert st["task_list_size"] == int(c["candidates"].sum()) and st["bmp_reduction"] == c["filtered"]
    assert (oc.block_num, oc.nnz) == (int(c["tiles"].sum()), int(c["values"].sum()))


@pytest.mark.parametrize("kind,L", HUB_CASES + [("full_rows", 8191)])
def test_hub_case_is_what_it_claims(oracle, kind, L):
    """the longest block-row of the hub operand is exactly L (the other operand's is short), the fill is at most 16 per tile where no
    switch is set, C's block-rows hold at most 256 tiles, integer values whose sums are exact, and the filtered case filters L pairs"""
    A, B = case(kind, L)
    side = hub_side(kind)
    la, lb = row_lengths(A), row_lengths(B)
    assert int((la, lb)[side].max()) == L and int((la, lb)[1 - side].max()) <= 4
    assert np.sort((la, lb)[side])[-2] <= 4     # one hub
    if kind == "full_rows":
        assert mean_fill(A) > RS_FILL_MAX and mean_fill(B) <= RS_FILL_MAX
        rows = np.bincount(A[2], minlength=16)
        assert rows[2] == rows[3] == rows[7] == 8 * L == 65528 and rows[:8].sum() == 24 * L
    else:
        assert mean_fill(A) <= 2 and mean_fill(B) <= 2
        for M in (A, B):
            assert set(tiles_of(M)["nnz"].tolist()) == {1, 2}
    c = c_structure(A, B)
    assert c["tiles"].max() <= (8 if side == 0 else RS_C_ROW_MAX) and c["tiles"].sum() > 0
    if kind == "hub_a" or kind == "full_rows":
        assert int(c["candidates"][0]) == L and c["filtered"] < L // 2
    if kind == "hub_b_untouched":
        assert not np.any(A[3] // 8 == HUB_K0) and c["candidates"].max() <= 6
    if kind == "hub_b_filtered":
        hub = (pairs_of(A, B)["ta"]["bj"] == HUB_K0)
        assert hub.sum() == 1 and c["candidates"][5] == L + 6 and c["filtered"] >= L
        p = pairs_of(A, B)
        assert not np.any(p["alive"][p["ta"]["bj"][p["ia"]] == HUB_K0])
    # exactness: integers 1 .. 7 and 1 .. 3, at most (values in a row of A) terms of at most 21 per sum
    assert set(np.unique(A[4]).tolist()) <= set(range(1, 8)) and set(np.unique(B[4]).tolist()) <= {1.0, 2.0, 3.0}
    assert A[4].max() == 7 and B[4].max() == 3 and A[4].max() * B[4].max() == 21 < 2048
    assert 21 * int(np.bincount(A[2]).max()) < 2 ** 24
    oc, st = oracle.spgemm(oracle.bmsp_from_coo(oracle.Coo(*A), 0, False), oracle.bmsp_from_coo(oracle.Coo(*B), 0, True))
    assert st["task_list_size"] == int(c["candidates"].sum()) and st["bmp_reduction"] == c["filtered"]
    assert (oc.block_num, oc.nnz) == (int(c["tiles"].sum()), int(c["values"].sum())) and oc.values.max() < 2 ** 24
    assert np.array_equal(oc.values, np.round(oc.values)) and oc.values.min() >= 1


def test_second_partner():
    """the hub A's second right operand: short block-rows, nearly empty tiles, pairs that survive with the hub and with the short A"""
    for L in (8193,):
        A, B2, As = case("hub_a", L)[0], second_partner(L), short_a(L)
        assert B2[0] == A[1] and row_lengths(B2).max() == 2 and mean_fill(B2) <= 2 and row_lengths(As).max() == 3
        assert c_structure(A, B2)["tiles"].max() <= 8 and c_structure(As, B2)["tiles"].sum() > 0
        assert set(np.unique(B2[4]).tolist()) <= {1.0, 2.0, 3.0}


@pytest.mark.parametrize("kind", ["grow_tiles", "grow_values"])
def test_growth_is_what_it_claims(oracle, kind):
    """grow_tiles, (P, rounds) = (2, 2): 8192 candidates, the four panels end at block-rows 32, 64, 320, 576; round 0 = the 64 top block-rows
    = 512 tiles, allocation int(512 * 2 * 1.25) + 1024 = 2304; round 1 needs 512 + 4096.  (2, 4): round 0 = 32 block-rows = 256 tiles,
    allocation int(256 * 4 * 1.25) + 1024 = 2304, round 1 needs 512, round 2 (block-rows 64 .. 320) 512 + 2048: two earlier rounds' slices
    move.  (3, 3): the panels end at 15, 29, 43, 57, 121, 235, 349, 463; round 0 = 43 block-rows = 344 tiles, allocation 1290 + 1024 = 2314,
    round 1 (block-rows 43 .. 235) needs 344 + 1536, round 2 1880 + 2728.  (8, 4): rounds 0 and 1 are 32 of the top block-rows each, as
    for (2, 4).  A top block-row of C holds 64 values, a bottom one 16: the values outgrow their allocation too under (2, 2) (4096 in
    round 0, 11264 allocated, 12288 needed) and (3, 3), not under (2, 4) and (8, 4) -- the table says which.
    grow_values: every block-row has 8 candidates and 8 C tiles; the top 64 give 8 values,
    the bottom 64 give 512.  (2, 2): round 0 = 512 tiles and values, allocation 2304 each; round 1 needs 1024 tiles and 512 + 32768 values.
    (2, 4): rounds of 32 block-rows; round 2 is the first of the bottom half: 256 + 256 + 16384 values against 2304.  (3, 3): the panels end
    at 15, 29, 43, 57, 71, 86, 100, 114; round 0 = 344 values, allocation 2314; round 1 (block-rows 43 .. 86: 21 top, 22 bottom) needs
    344 + 168 + 11264 and grows to max(need, 344 + int(11432 * 2 * 1.25) + 1024 = 29948); round 2 needs 33280: it grows twice."""
    A, B = case(kind)
    c = c_structure(A, B)
    if kind == "grow_tiles":
        assert c["candidates"].tolist() == [64] * 64 + [8] * 512 and c["tiles"].tolist() == [8] * 576 and c["filtered"] == 0
        assert int(c["tiles"][:64].sum()) == 512 and int(c["tiles"].sum()) == 4608
        assert candidate_bounds(c["candidates"], 4).tolist() == [0, 32, 64, 320, 576]
        assert candidate_bounds(c["candidates"], 8).tolist() == [0, 16, 32, 48, 64, 192, 320, 448, 576]
        assert candidate_bounds(c["candidates"], 9).tolist() == [0, 15, 29, 43, 57, 121, 235, 349, 463, 576]
        assert c["values"].tolist() == [64] * 64 + [16] * 512
    else:
        assert c["candidates"].tolist() == [8] * 128 and c["tiles"].tolist() == [8] * 128 and c["filtered"] == 0
        assert c["values"].tolist() == [8] * 64 + [512] * 64
        assert candidate_bounds(c["candidates"], 9).tolist() == [0, 15, 29, 43, 57, 71, 86, 100, 114, 128]
    for (P, rounds), want in EXPECTED_GROWTH[kind].items():
        bounds = candidate_bounds(c["candidates"], P * rounds)
        got = growth_events(panel_sums(c["tiles"], bounds), panel_sums(c["values"], bounds), P, rounds)
        assert got == want, (kind, P, rounds, got)
        assert got and all(k >= 1 for k, _, _ in got)
    # values whose sums are exact in fp32 in any order (the sharded and the whole product may take different kernels), fp16 operands
    for M in (A, B):
        assert np.array_equal(M[4] * 64, np.round(M[4] * 64)) and M[4].min() >= 0.25 and M[4].max() <= 1.25
        assert np.array_equal(M[4].astype(np.float16).astype(np.float64), M[4])
    assert (80 * 80) * int(np.bincount(A[2]).max()) < 2 ** 24      # (units of 2^-12; a value of A gives one term to a value of C at most)
    oc, st = oracle.spgemm(oracle.bmsp_from_coo(oracle.Coo(*A), 0, False), oracle.bmsp_from_coo(oracle.Coo(*B), 0, True))
    assert st["task_list_size"] == int(c["candidates"].sum()) and (oc.block_num, oc.nnz) == (int(c["tiles"].sum()), int(c["values"].sum()))
    rows = (oc.keys >> np.uint64(32)).astype(np.int64)
    assert np.array_equal(np.bincount(rows, minlength=c["tiles"].size), c["tiles"])
    assert np.array_equal(np.bincount(rows, weights=np.diff(oc.offsets.astype(np.int64)), minlength=c["tiles"].size).astype(np.int64), c["values"])
