"""bmsp_spgemm's symbolic stages at every segment-length and capacity edge: exactly on, one below and one above each threshold.

The product switches kernels on the length of a block-row's task segment (segsort.hip: register networks of 128 .. 4096 words, the
wave's capacity, the workgroup kernel, pieces + merge passes, counting passes, the read-back-free kernel), on the C tiles per
block-row (rowmerge.hip: strip mode up to 256 in a 512-slot table, task-list mode up to 896 in a 1024-slot table, 16-bit task offsets,
early refusals by B's widest block-row), on the strip kernel's lists (192 merged A tiles, 512 merged C tiles), on the row-sparse
kernel's table (768 tiles) and on the number of candidate pairs (2 << 20 picks the expansion tile).  The thresholds are mirrored below
as named constants and read back from the sources by test_constants_match_sources: a later change of one fails that test instead of
leaving these cases beside the edge.

Two generators build the operands, pure numpy:

edge_product(lengths, a_tiles)   one block-row of A per wanted segment length L (empty block-rows in between), `a` tiles each holding the
    SAME full row; every A tile meets a block-row of B of its own that holds its share of L one-value tiles at sorted random block
    columns out of ~1.5 x share, the column inside the tile a function of the block column alone.  Every candidate pair survives the
    bitmap filter, the segment has exactly L tasks, the expansion emits it as `a` ascending runs (unsorted), and the C values that
    receive a term from two A tiles change their fp32 bits in about a third of the cases when the terms are added in the other order.
cap_product(rows)                block-row i of A holds `a` full-row tiles; the B block-row of tile t holds the columns S[t::a] of a
    c-element set S plus a random half of S: block-row i of C has exactly c tiles.  S comes from all block columns, from a range, or
    from the columns whose home slot (j * 0x9E3779B1) >> (32 - bits) lies in the last 8 slots of the table: every probe sequence of
    such a row runs into the end of the table and wraps.

There is no tolerance in this file: keys, bitmaps, offsets, values and the four stage counters are compared bit for bit with the oracle
(check_spgemm).  fp32 / tc_version 5 and fp16 / tc_version 5 follow the oracle's operation order -- the values depend on the order of
the tasks inside every C tile, i.e. on the sort being right AND stable; the CPU self-checks assert, from the operands alone with an
emulated fmaf chain, that every segment holds C values whose bits differ between the two orders (and, for segments cut into pieces or
tiles, one whose tasks lie in different pieces and different 4096-tiles).  fp16 / tc_version 4 (matrix cores) runs on values that are
multiples of 1/4 up to 1, whose sums are exact in fp32 in any order (asserted on the CPU).  The block-MAC kernel that reads the task
list is pinned (BMSP_MAC_ROWSPARSE=0) wherever the task order is what the case is about: the row-sparse kernel never reads the list.

This file holds the constants, the generators, the table of products and the CPU self-checks; the GPU cases that run the products live
in tests/test_zzz_spgemm_regimes.py, named to be collected last so that every earlier GPU test keeps its place in the suite's order."""
import functools
import os
import re
import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "csrc")

# ---- the thresholds, as the sources state them (test_constants_match_sources) ---------------------------------------------------------
TASK_WAVE_MAX = 2048          # segsort.hip kTaskWaveMax: words a wave sorts in registers with 64-bit sort words (32-bit: twice that)
BLOCK_SEG_MAX = 4096          # kBlockSegMax: the workgroup kernel
TASK_BLOCK_IDX_BITS = 12      # kTaskBlockIdxBits: position bits of a sort word; narrow words while jbits + 12 <= 32
MERGE_TILE = 1024             # kMergeTile
SEG_RADIX_TILE = 4096         # kSegRadixTile
SEG_RADIX_BITS = 7            # kSegRadixBits: column bits per counting pass
ROW_CAP = 384                 # rowmerge.hip kRowCap (strip mode is called with kJCap / 2 = 256, the smaller of the two)
HASH_BITS = 9                 # kHashBits: strip mode's table
TL_CAP = 896                  # kTlCap
TL_BITS = 10                  # kTlBits: task-list mode's table
K_CAP = 192                   # mac_choice.h kKCap: merged A tiles of a strip (blockmac_strip.hip)
J_CAP = 512                   # kJCap: merged C tiles of a strip
RS_TABLE = 768                # mac_choice.h rs_row_cap(10): the row-sparse kernel's larger table
SMALL_PRODUCT = 2 << 20       # spgemm.hip small_product
NARROW_CAP, WIDE_CAP = 2 * TASK_WAVE_MAX, TASK_WAVE_MAX   # a wave's capacity in sort words
STRIP_ROW_CAP = J_CAP // 2
TL_B_ROW_MAX = TL_CAP + 63    # rowmerge_tasklist's early refusal
TL_TASKS_MAX = 65535 - 64     # 16-bit task offsets: ns + 64 > 65535 voids the pass


def test_constants_match_sources():
    """the named constants above against the constexpr lines (and the two literals) of the sources"""
    def src(name):
        return open(os.path.join(CSRC, name)).read()

    def cx(text, name):
        m = [re.search(r"\b%s\s*=\s*(\d+)" % name, ln) for ln in text.splitlines() if "constexpr" in ln]
        m = [x for x in m if x]
        assert len(m) == 1, (name, len(m))
        return int(m[0].group(1))
    seg, rm, rule = src("segsort.hip"), src("rowmerge.hip"), src("mac_choice.h")    # (the capacities the block-MAC rule reads sit beside it)
    assert cx(seg, "kTaskWaveMax") == TASK_WAVE_MAX and cx(seg, "kBlockSegMax") == BLOCK_SEG_MAX
    assert cx(seg, "kTaskBlockIdxBits") == TASK_BLOCK_IDX_BITS and cx(seg, "kMergeTile") == MERGE_TILE
    assert cx(seg, "kSegRadixTile") == SEG_RADIX_TILE and cx(seg, "kSegRadixBits") == SEG_RADIX_BITS
    assert cx(rm, "kRowCap") == ROW_CAP and cx(rm, "kHashBits") == HASH_BITS and cx(rm, "kTlCap") == TL_CAP and cx(rm, "kTlBits") == TL_BITS
    assert cx(rule, "kKCap") == K_CAP and cx(rule, "kJCap") == J_CAP
    m = re.search(r"constexpr uint32_t rs_row_cap\(int hb\) \{ return hb == 9 \? (\d+)u : (\d+)u; \}", rule)
    assert m and int(m.group(1)) == STRIP_ROW_CAP and int(m.group(2)) == RS_TABLE
    m = re.search(r"small_product = total <= \((\d+)u << (\d+)\)", src("spgemm.hip"))
    assert m and int(m.group(1)) << int(m.group(2)) == SMALL_PRODUCT
    # what the cases below derive from them
    assert STRIP_ROW_CAP <= ROW_CAP and STRIP_ROW_CAP + 63 < (1 << HASH_BITS) and TL_CAP + 63 < (1 << TL_BITS)
    assert re.search(r"B->max_row_blocks > \(int64_t\)\(kTlCap \+ 63\)", rm) and re.search(r"B->max_row_blocks > \(int64_t\)row_cap", rm)
    assert len(re.findall(r"ns(?:_all)? \+ 64u > 65535u", rm)) == 4     # in both build forms: inside the walk and after it
    assert re.search(r"max_len > 4u \* cap", seg) and re.search(r"sizeof\(W\) == 4 \? 2 \* kTaskWaveMax : kTaskWaveMax", seg)


# ---- generators -------------------------------------------------------------------------------------------------------------------------
def _col_in_tile(j):
    return (5 * j + 3) % 8


def _assemble(tiles_a, tiles_b, n_block_rows, n_k, nbc, exact, salts):
    """tiles_a: (block-row, k, row inside the tile, segment); tiles_b: (k, block column); the COO operands.  A tiles hold one full row,
    B tiles one value at (row (k + j) % 8, column _col_in_tile(j))."""
    bi, k, r, sg = (np.asarray(x, dtype=np.int64) for x in zip(*tiles_a))
    ra = np.repeat(8 * bi + r, 8)
    ca = (np.repeat(8 * k, 8) + np.tile(np.arange(8), bi.size))
    bk, bj = tiles_b
    rb = 8 * bk + (bk + bj) % 8
    cb = 8 * bj + _col_in_tile(bj)
    if exact:   # multiples of 1/4 up to 1, both signs: every sum of products is exact in fp32 (and fp16 holds every operand)
        va = ((ra * 3 + ca) % 4 + 1) / 4.0 * np.where((ra + ca // 3) % 2 == 0, 1.0, -1.0)
        vb = ((rb + cb * 3) % 4 + 1) / 4.0 * np.where((rb // 2 + cb) % 2 == 0, 1.0, -1.0)
    else:
        sa = np.repeat(np.asarray(salts, dtype=np.float64)[sg], 8)
        sb = np.zeros(n_k)
        sb[k] = np.asarray(salts, dtype=np.float64)[sg]
        va = np.sin(1.3 * ra + 0.7 * ca + sa)
        vb = np.cos(0.9 * rb + 0.31 * cb + 2.0 * sb[bk])
    A = (8 * n_block_rows, 8 * n_k, ra.astype(np.int64), ca.astype(np.int64), va)
    B = (8 * n_k, 8 * nbc, rb.astype(np.int64), cb.astype(np.int64), vb)
    return A, B


def product_terms(A, B):
    """Every task of A x B, from the operands alone, in the expansion's order (A tiles in key order, the tiles of B's block-row k in column
    order): block-row of A (= segment), position inside the segment, block column of C, and the two fp32 operands of the one scalar product
    the task holds (A tiles hold one full row, B tiles one value: asserted)."""
    (_, _, r1, c1, v1), (_, _, r2, c2, v2) = A, B
    o = np.lexsort((c1, r1 // 8 * (1 << 32) + c1 // 8))
    r1, c1, v1 = r1[o], c1[o], np.asarray(v1)[o]
    tkey = r1 // 8 * (1 << 32) + c1 // 8
    assert r1.size % 8 == 0 and np.array_equal(tkey.reshape(-1, 8)[:, 0:1].repeat(8, 1), tkey.reshape(-1, 8))
    assert np.array_equal(r1.reshape(-1, 8)[:, 0:1].repeat(8, 1), r1.reshape(-1, 8)) and np.array_equal(c1.reshape(-1, 8) % 8, np.tile(np.arange(8), (r1.size // 8, 1)))
    a_bi, a_k = tkey[::8] >> 32, tkey[::8] & 0xffffffff
    a_vals = v1.reshape(-1, 8).astype(np.float32)
    assert np.all(np.diff(tkey[::8]) > 0)
    o = np.lexsort((c2 // 8, r2 // 8))
    r2, c2, v2 = r2[o], c2[o], np.asarray(v2)[o]
    bkey = r2 // 8 * (1 << 32) + c2 // 8
    assert np.all(np.diff(bkey) > 0)    # one value per B tile
    n_k = int(max(a_k.max(), (r2 // 8).max())) + 2
    bptr = np.searchsorted(r2 // 8, np.arange(n_k + 1))
    cnt = bptr[a_k + 1] - bptr[a_k]
    ta = np.repeat(np.arange(a_k.size), cnt)
    first = np.cumsum(cnt) - cnt
    tb = np.arange(cnt.sum()) - np.repeat(first, cnt) + np.repeat(bptr[a_k], cnt)
    seg = a_bi[ta]
    seg_first = np.searchsorted(seg, seg)   # tasks arrive grouped by block-row of A
    return {"seg": seg, "pos": np.arange(seg.size) - seg_first, "j": c2[tb] // 8, "a": a_vals[ta, r2[tb] % 8], "b": v2[tb].astype(np.float32),
            "a_tile": ta, "max_a": int(np.bincount(a_bi).max()), "max_b": int(np.diff(bptr).max())}


def order_sensitive(t):
    """per C value (segment, block column) with at least two terms: whether V15's fmaf chain (acc = fl32(a * b + acc), tasks ascending) ends
    in other bits when the tasks are taken in the opposite order; and the positions of its first and last task.  Emulated in float64
    (the product of two fp32 numbers is exact there; the double rounding of the sum does not matter for a count)."""
    o = np.lexsort((t["pos"], t["j"], t["seg"]))
    seg, j, pos = t["seg"][o], t["j"][o], t["pos"][o]
    p = t["a"][o].astype(np.float64) * t["b"][o].astype(np.float64)
    head = np.ones(seg.size, bool)
    head[1:] = (seg[1:] != seg[:-1]) | (j[1:] != j[:-1])
    g = np.cumsum(head) - 1
    start = np.flatnonzero(head)
    size = np.diff(np.append(start, seg.size))
    idx = np.arange(seg.size) - start[g]
    m = int(size.max())
    out = []
    for place in (idx, size[g] - 1 - idx):
        P = np.zeros((start.size, m))
        M = np.zeros((start.size, m), bool)
        P[g, place] = p
        M[g, place] = True
        acc = np.zeros(start.size, np.float32)
        for c in range(m):
            acc = np.where(M[:, c], (P[:, c] + acc.astype(np.float64)).astype(np.float32), acc)
        out.append(acc)
    multi = size >= 2
    return {"seg": seg[start][multi], "differs": (out[0] != out[1])[multi], "first": pos[start][multi], "last": pos[start + size - 1][multi]}


def vacuity_failures(t, lengths_by_row, cap):
    """the segments that could not tell a wrong or unstable sort from a right one (none is wanted): see the docstring of the file"""
    s = order_sensitive(t)
    bad = []
    for row, L in lengths_by_row.items():
        mine = s["seg"] == row
        d = mine & s["differs"]
        cols = t["j"][t["seg"] == row]
        n_values = int(np.unique(cols).size)
        if n_values == L:   # a single A tile: one ascending run, one term per C value -- nothing for a sort to get wrong but the copy
            assert np.all(np.diff(cols) > 0)
            continue
        # L / 32 where two A tiles share ~L / 3 of ~3 L / 4 C values (a third of them differ); a quarter of the C values where many A
        # tiles leave the segment fewer C values than that (every value then has several terms, and more of them differ)
        need = 0 if L < 2 else (1 if L <= 62 else min(-(-L // 32), -(-n_values // 4)))
        if int(d.sum()) < need:
            bad.append((row, L, "sensitive values", int(d.sum()), need))
        if L > cap and not np.any(d & (s["first"] // cap != s["last"] // cap)):
            bad.append((row, L, "none across pieces of", cap))
        if L > SEG_RADIX_TILE and not np.any(d & (s["first"] // SEG_RADIX_TILE != s["last"] // SEG_RADIX_TILE)):
            bad.append((row, L, "none across tiles"))
    return bad


def _block_row_of(i):
    return i + i // 2      # every third block-row of A is empty


def edge_product(lengths, a_tiles=2, nbc=None, top=False, exact=False, seed=1):
    """see the docstring of the file.  lengths: L or (L, a) per segment; nbc: block columns of B (default: what the widest pool needs);
    top: every pool sits at the END of the column range (the last task of the last run is at block column nbc - 1).  The last column
    of the pool is put into the first and the last run by hand (a C value with two terms whose tasks are as far apart as the segment
    allows), and the values of a segment are re-drawn until the vacuity conditions hold for it."""
    rng = np.random.default_rng(seed)
    plan = []
    for L in lengths:
        L, a = (int(L), a_tiles) if np.isscalar(L) else (int(L[0]), int(L[1]))
        a = max(1, min(a, L))
        if nbc is not None:
            a = max(a, -(-L // max(1, 2 * nbc // 3)))
        plan.append((L, a))
    if nbc is None:
        nbc = max(max(2, -(-3 * -(-L // a) // 2)) for L, a in plan)
    segments, k0 = [], 0
    for i, (L, a) in enumerate(plan):
        shares = [L // a + (1 if t < L % a else 0) for t in range(a)]
        pool = min(nbc, max(shares[0], -(-3 * shares[0] // 2)))
        assert shares[0] <= pool
        base = nbc - pool if top else int(rng.integers(0, nbc - pool + 1))
        runs = []
        for t, s in enumerate(shares):
            c = np.sort(rng.choice(pool, s, replace=False))
            if a >= 2 and t in (0, a - 1):
                c[-1] = pool - 1
            runs.append(c + base)
        segments.append((_block_row_of(i), (3 * i + 1) % 8, k0, runs))
        k0 += a
    n_rows = _block_row_of(len(plan) - 1) + 1

    def build(which, salts):
        ta, bk, bj = [], [], []
        for s in which:
            row, r, k_first, runs = segments[s]
            for t, c in enumerate(runs):
                ta.append((row, k_first + t, r, s))
                bk.append(np.full(c.size, k_first + t)); bj.append(c)
        return _assemble(ta, (np.concatenate(bk), np.concatenate(bj)), n_rows, k0, nbc, exact, salts)
    salts = [0.0] * len(plan)
    if not exact:
        for s, (L, a) in enumerate(plan):
            if L < 2:
                continue
            for attempt in range(40):
                salts[s] = float(attempt)
                A, B = build([s], salts)
                t = product_terms(A, B)
                assert t["seg"].size == L
                if not vacuity_failures(t, {segments[s][0]: L}, WIDE_CAP) and not vacuity_failures(t, {segments[s][0]: L}, NARROW_CAP):
                    break
            else:
                raise AssertionError("no values found for segment %d of length %d" % (s, L))
    A, B = build(range(len(plan)), salts)
    return A, B, {segments[s][0]: plan[s][0] for s in range(len(plan))}


def home_slot(j, bits):
    return ((np.asarray(j, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xffffffff)) >> np.uint64(32 - bits)


def cap_product(rows, nbc, exact=False, seed=2, extra_b_row=0):
    """see the docstring of the file.  rows: (a, c, pool) per block-row of A -- pool "all", ("range", lo, hi) or ("wrap", bits) -- or
    ("tiles", [columns of tile 0, columns of tile 1, ...]) for a walk laid out by hand.  extra_b_row: a block-row of B of that many
    tiles that no tile of A meets (it counts for max_row_blocks(B) and for nothing else)."""
    rng = np.random.default_rng(seed)
    ta, bk, bj, k0, want = [], [], [], 0, {}
    for i, row in enumerate(rows):
        if row[0] == "tiles":
            runs = [np.unique(np.asarray(c, dtype=np.int64)) for c in row[1]]
        else:
            a, c, pool = row
            if pool == "all":
                cand = np.arange(nbc)
            elif pool[0] == "range":
                cand = np.arange(pool[1], pool[2])
            else:
                cand = np.flatnonzero(home_slot(np.arange(nbc), pool[1]) >= (1 << pool[1]) - 8)
            S = rng.choice(cand, c, replace=False)
            runs = [np.unique(np.concatenate([S[t::a], rng.choice(S, c // 2, replace=False)])) for t in range(a)]
        if runs:
            want[i] = int(np.unique(np.concatenate(runs)).size)
        for t, c in enumerate(runs):
            ta.append((i, k0 + t, (3 * i + 1) % 8, 0))
            bk.append(np.full(c.size, k0 + t)); bj.append(c)
        k0 += len(runs)
    if extra_b_row:
        bk.append(np.full(extra_b_row, k0)); bj.append(np.arange(extra_b_row) * (nbc // extra_b_row))
        k0 += 1
    A, B = _assemble(ta, (np.concatenate(bk), np.concatenate(bj)), len(rows), k0, nbc, exact, [0.0])
    if not exact:   # away from zero: strip mode's numeric kernels want every product a normal number
        A, B = A[:4] + (1.0 + 0.5 * A[4],), B[:4] + (1.0 + 0.5 * B[4],)
    return A, B, want


def pairs_product(extra):
    """1024 block-rows of A with two tiles each, all meeting the same two block-rows of B of 1024 tiles (on the same columns, which keeps
    C at 2^20 one-value tiles): exactly 2 << 20 candidate pairs; `extra` further block-rows of A with one tile meeting one tile."""
    n, w = 1024, 1024
    ta = [(i, t, (3 * i + 1) % 8, 0) for i in range(n) for t in range(2)] + [(n + e, 2 + e, 5, 0) for e in range(extra)]
    bk = np.concatenate([np.repeat(np.arange(2), w), 2 + np.arange(extra)])
    bj = np.concatenate([np.tile(np.arange(w), 2), 7 * np.arange(extra)])
    A, B = _assemble(ta, (bk, bj), n + extra, 2 + extra, w, False, [0.0])
    return A, B, n * 2 * w + extra


# ---- the products ------------------------------------------------------------------------------------------------------------------------
A1_LENGTHS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048]
A1_UPPER = [2049, 4095, 4096]
A2_LONG = [4097, 8191, 8192, 8193, 12288, 12289, 16384]
A2_SHORT = [1, 2, 5, 700]


def _around(long, short):
    out = []
    for i, L in enumerate(long):
        out += [short[i % len(short)], L]
    return out + list(short)


EDGE = {
    # name: (lengths, keywords of edge_product)
    "a1": (A1_LENGTHS, {}),
    "a1_upper": (A1_LENGTHS[::3] + A1_UPPER, {}),
    "a1_sentinel": ([5, 700] + A1_UPPER, {"nbc": 1 << 20, "top": True}),      # jbits + 12 == 32; the 4096-task segment ends at column 2^20 - 1
    "a1_real_wide": ([5, 700] + A1_UPPER, {"nbc": (1 << 20) + 1, "top": True}),  # 21 column bits: 64-bit sort words without the switch
    "a1_refusal": ([(17, 17), (241, 1), 700, 4096, 3], {}),               # bound 17 x 2048 > 4096 while no segment exceeds 4096
    "a1_bound_4097": ([(17, 17), (241, 1), 200, 3], {}),                  # bound 17 x 241 = 4097, every segment <= 241
    "a2": (_around(A2_LONG, A2_SHORT), {}),
    "a2_half": (_around([L // 2 + (L & 1) for L in A2_LONG], A2_SHORT), {}),  # 2049, 4096, 4096, 4097, 6144, 6145, 8192
    "a2_all_long_odd": ([4097, 8192, 6000], {}),
    # (64-bit words: 2049 .. 4096 tasks are the workgroup kernel's, pieces of 2048 begin at 4097 -- one pass is out of reach, three are odd)
    "a2_all_long_odd_half": ([8193, 16384, 12000], {}),
    "a2_mixed_odd": ([4097, 700, 8192, 1, 2], {}),
    "a2_mixed_odd_half": ([8193, 700, 16384, 1, 2], {}),
    "a2_mixed_even": ([5, 16384, 8193, 700], {}),
    "a2_mixed_even_half": ([5, 8192, 4097, 700], {}),
    "a3_16384": ([700, 16384, 2, 4097], {}),
    "a3_16385": ([700, 16385, 2, 4097], {}),
    "a3_8192": ([700, 8192, 2, 2049], {}),
    "a3_8193": ([700, 8193, 2, 2049], {}),
    "a3_pass1": (_around(A2_LONG, A2_SHORT), {"nbc": 128}),       # jbits 7: one counting pass
    "a3_pass2_lo": (_around(A2_LONG, A2_SHORT), {"nbc": 129}),    # jbits 8
    "a3_pass2_hi": (_around(A2_LONG, A2_SHORT), {"nbc": 1 << 14}),  # jbits 14
    "a3_pass3_lo": (_around(A2_LONG, A2_SHORT), {"nbc": (1 << 14) + 1}),  # jbits 15
    "a3_pass3_hi": (_around(A2_LONG, A2_SHORT), {"nbc": 1 << 20}),  # jbits 20: the last width of the narrow words
    "a3_pass3_top": (_around(A2_LONG, A2_SHORT), {"nbc": (1 << 20) + 1}),  # jbits 21: the last width of three passes, 64-bit words without the switch
}
WRAP9, WRAP10 = ("wrap", HASH_BITS), ("wrap", TL_BITS)
_ORD = [(3, 40, "all"), (2, 17, "all"), (5, 200, "all")]


def _beside(row):
    return [_ORD[0], row, _ORD[1], _ORD[2]]


CAP = {
    # name: (rows, block columns of B, keywords of cap_product)
    **{"b_%d_%s" % (c, p): (_beside((4, c, "all" if p == "all" else WRAP9)), 1 << 15, {}) for c in (255, 256, 257) for p in ("all", "wrap")},
    # two A tiles walk side by side, sixteen B tiles each per step: 128 + 122 = 250 columns after eight steps, the ninth brings seven more
    "b_last_step": (_beside(("tiles", [np.arange(135), 1000 + np.arange(122)])), 1 << 11, {}),
    # 256 columns from the first A tile; the others (three beside it, one in the next group of four) bring only columns already there
    "b_duplicates": (_beside(("tiles", [3 * np.arange(256), 3 * np.arange(5), 3 * np.arange(40, 45), 3 * np.arange(90, 95), 3 * np.arange(200)])), 1 << 10, {}),
    "b_brow_256": ([(1, 40, "all"), (1, 200, "all"), (1, 17, "all")], 1 << 10, {"extra_b_row": 256}),
    "b_brow_257": ([(1, 40, "all"), (1, 200, "all"), (1, 17, "all")], 1 << 10, {"extra_b_row": 257}),
    "b_jcap_512": ([(2, 256, ("range", 0, 600)), (2, 256, ("range", 600, 1200)), (2, 17, "all")], 1200, {}),
    "b_jcap_513": ([(2, 256, ("range", 0, 600)), (2, 257, ("range", 600, 1200)), (2, 17, "all")], 1200, {}),
    "b_kcap_192": ([(96, 200, ("range", 0, 300)), (96, 200, ("range", 300, 600)), (2, 17, "all")], 600, {}),
    "b_kcap_193": ([(96, 200, ("range", 0, 300)), (97, 200, ("range", 300, 600)), (2, 17, "all")], 600, {}),
    **{"b_rs_%d" % c: (_beside((4, c, "all")), 1 << 12, {}) for c in (767, 768, 769)},
    **{"c_%d_%s" % (c, p): (_beside((4, c, "all" if p == "all" else WRAP10)), 1 << 17, {}) for c in (895, 896, 897) for p in ("all", "wrap")},
    "c_brow_959": (_beside((4, 300, "all")), 1 << 12, {"extra_b_row": TL_B_ROW_MAX}),
    "c_brow_960": (_beside((4, 300, "all")), 1 << 12, {"extra_b_row": TL_B_ROW_MAX + 1}),
    # 128 A tiles over 512 shared block columns, the last one trimmed: 65 471 and 65 472 surviving pairs in one block-row
    "c_tasks_65471": ([_ORD[0], ("tiles", [7 * np.arange(512)] * 127 + [7 * np.arange(512 - 65)])], 7 * 512, {}),
    "c_tasks_65472": ([_ORD[0], ("tiles", [7 * np.arange(512)] * 127 + [7 * np.arange(512 - 64)])], 7 * 512, {}),
}


@functools.lru_cache(maxsize=None)
def product(name, exact=False):
    """(A, B, expectation): the expectation is {block-row: segment length} for the edge products, {block-row: C tiles} for the capacity
    products, the number of candidate pairs for the expansion products"""
    if name in EDGE:
        return edge_product(EDGE[name][0], exact=exact, **EDGE[name][1])
    if name in CAP:
        return cap_product(CAP[name][0], CAP[name][1], exact=exact, **CAP[name][2])
    return pairs_product({"d_exact": 0, "d_plus_one": 1}[name])


def jbits_of(B):
    return max(1, int(B[1] // 8 - 1).bit_length())


def tiny_product(kind):
    """64 x 64 operands (8 x 8 tiles, every tile stored) for the cases that only ask WHICH block-MAC kernel runs: `sparse` -- two values per
    tile, placed so that every candidate pair survives (A tile (i, k) holds a value in tile column k % 8, B tile (k, j) one in tile row
    k % 8); `full` -- all 64 values; `tiny` -- `sparse` with the first stored value of either operand replaced by 2^-70 (their product is
    no normal number).  Values are multiples of 1/4 up to 1 of both signs: fp16 holds them and every sum is exact in fp32 in any order."""
    t = np.arange(64)
    bi, bk = t // 8, t % 8
    if kind == "full":
        r = c = None
        ra = rb = np.repeat(np.arange(64), 64)
        ca = cb = np.tile(np.arange(64), 64)
    else:
        ra = np.concatenate([8 * bi + (bi + bk) % 8, 8 * bi + (bi + 2 * bk + 3) % 8])
        ca = np.concatenate([8 * bk + bk % 8, 8 * bk + (bk + 4) % 8])
        rb = np.concatenate([8 * bi + bi % 8, 8 * bi + (bi + 4) % 8])            # (B's tile (k, j) = (bi, bk) here)
        cb = np.concatenate([8 * bk + (bi + bk) % 8, 8 * bk + (3 * bk + bi + 1) % 8])
    va = ((ra * 3 + ca) % 4 + 1) / 4.0 * np.where((ra + ca // 3) % 2 == 0, 1.0, -1.0)
    vb = ((rb + cb * 3) % 4 + 1) / 4.0 * np.where((rb // 2 + cb) % 2 == 0, 1.0, -1.0)
    if kind == "tiny":
        va[0] = vb[0] = 2.0 ** -70
    return (64, 64, ra.astype(np.int64), ca.astype(np.int64), va), (64, 64, rb.astype(np.int64), cb.astype(np.int64), vb)


def test_tiny_products_are_what_they_claim(oracle):
    for kind, per_tile in (("sparse", 2), ("tiny", 2), ("full", 64)):
        A, B = tiny_product(kind)
        for M in (A, B):
            key = (M[2] // 8) * 8 + M[3] // 8
            assert np.unique(M[2] * 64 + M[3]).size == M[2].size and np.array_equal(np.bincount(key, minlength=64), np.full(64, per_tile))
        _, st = oracle.spgemm(oracle.bmsp_from_coo(oracle.Coo(*A), 0, False), oracle.bmsp_from_coo(oracle.Coo(*B), 0, True))
        assert st["task_list_size"] == st["surviving_tasks"] == 512 and st["c_blocks"] == 64     # every pair survives
        assert 8 * 8 <= STRIP_ROW_CAP                                                            # ... and strip mode runs without T_2
        mags = np.abs(np.concatenate([A[4], B[4]]))
        assert np.array_equal(mags.astype(np.float16).astype(np.float64), mags) or kind == "tiny"
        assert (mags.min() == 2.0 ** -70) == (kind == "tiny") and np.sort(mags)[2] >= 0.25 and mags.max() == 1.0


def _oracle_product(oracle, name, dtype=0, exact=False):
    A, B, want = product(name, exact)
    refA = oracle.bmsp_from_coo(oracle.Coo(*A), dtype, False)
    refB = oracle.bmsp_from_coo(oracle.Coo(*B), dtype, True)
    C, st = oracle.spgemm(refA, refB)
    return A, B, want, refA, refB, C, st


# ---- CPU self-checks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_product_is_what_it_claims(oracle, name):
    """exact segment lengths (from the operands, and from the oracle's counters and C), every candidate pair survives, the runs are
    unsorted, and the vacuity conditions hold for both word widths"""
    A, B, want, refA, refB, C, st = _oracle_product(oracle, name)
    t = product_terms(A, B)
    rows, counts = np.unique(t["seg"], return_counts=True)
    assert dict(zip(rows.tolist(), counts.tolist())) == want
    total = sum(want.values())
    assert st["task_list_size"] == total and st["surviving_tasks"] == total and st["bmp_reduction"] == 0
    # every C tile holds one value per task-carrying column; block-rows of C = the segments' block-rows
    assert set((C.keys >> np.uint64(32)).tolist()) == set(want)
    for row, L in want.items():
        mine = t["seg"] == row
        assert int(np.unique(t["j"][mine]).size) == int(np.sum((C.keys >> np.uint64(32)) == row))
        if L >= 63 and np.unique(t["a_tile"][mine]).size > 1:     # the expansion's order is not the sorted one
            assert np.any(np.diff(t["j"][mine]) < 0)
    assert (refA.block_num, refB.block_num) == (int(np.unique(t["a_tile"]).size), total)
    for cap in (NARROW_CAP, WIDE_CAP):
        assert vacuity_failures(t, want, cap) == []


def test_edge_two_term_values_change_with_the_order(oracle):
    """what the vacuity conditions rest on, measured on the A1 product: between a quarter and a half of the C values with two terms end
    in other fp32 bits when the terms are added in the other order (sin / cos values, two A tiles per block-row)"""
    A, B, want = product("a1")
    s = order_sensitive(product_terms(A, B))
    frac = s["differs"].mean()
    assert s["differs"].size > sum(want.values()) // 4 and 0.25 < frac < 0.5, (s["differs"].size, frac)


def test_edge_dispatch_bounds():
    """max_row_blocks(A) x max_row_blocks(B), the dispatcher's condition for the read-back-free kernel, for the products that are meant to
    sit on either side of a wave's capacity; the sort-word widths; the sentinel word"""
    def bound(name):
        t = product_terms(*product(name)[:2])
        return t["max_a"] * t["max_b"]
    assert bound("a1") == WIDE_CAP and bound("a1_upper") == NARROW_CAP and bound("a1_sentinel") == NARROW_CAP
    assert bound("a1_bound_4097") == NARROW_CAP + 1 and max(product("a1_bound_4097")[2].values()) <= 241
    assert bound("a1_refusal") > NARROW_CAP and max(product("a1_refusal")[2].values()) == NARROW_CAP
    A, B, want = product("a1_sentinel")
    assert jbits_of(B) + TASK_BLOCK_IDX_BITS == 32 and B[1] // 8 == 1 << 20
    t = product_terms(A, B)
    last = (t["seg"] == max(want)) & (t["pos"] == NARROW_CAP - 1)
    assert want[max(want)] == NARROW_CAP and int(t["j"][last][0]) == (1 << 20) - 1
    assert ((int(t["j"][last][0]) << TASK_BLOCK_IDX_BITS) | (NARROW_CAP - 1)) == 0xffffffff    # the padding value of the 32-bit network
    assert jbits_of(product("a1_real_wide")[1]) + TASK_BLOCK_IDX_BITS == 33
    for name, jb in (("a3_pass1", 7), ("a3_pass2_lo", 8), ("a3_pass2_hi", 14), ("a3_pass3_lo", 15), ("a3_pass3_hi", 20), ("a3_pass3_top", 21)):
        assert jbits_of(product(name)[1]) == jb and -(-jb // SEG_RADIX_BITS) == int(name[7])
    assert -(-22 // SEG_RADIX_BITS) == 4 and 20 + TASK_BLOCK_IDX_BITS == 32     # 21 bits: the last three-pass width, the first of the wide words


@pytest.mark.parametrize("name", sorted(CAP))
def test_cap_product_is_what_it_claims(oracle, name):
    """C tiles per block-row exactly as wanted (from the oracle's C), max_row_blocks(B), and -- for the wrapping pools -- a probe that leaves
    the table's last slot in every such block-row"""
    A, B, want, refA, refB, C, st = _oracle_product(oracle, name)
    rows, counts = np.unique(C.keys >> np.uint64(32), return_counts=True)
    assert dict(zip(rows.tolist(), counts.tolist())) == want
    assert st["surviving_tasks"] == st["task_list_size"]
    t = product_terms(A, B)
    assert st["surviving_tasks"] == t["seg"].size
    extra = CAP[name][2].get("extra_b_row", 0)
    if extra:
        assert t["max_b"] == extra
    for i, row in enumerate(CAP[name][0]):
        if row[0] != "tiles" and row[2] in (WRAP9, WRAP10):
            bits = row[2][1]
            cols = (C.keys[(C.keys >> np.uint64(32)) == i] & np.uint64(0xffffffff)).astype(np.int64)
            h = home_slot(cols, bits).astype(np.int64)
            assert h.min() >= (1 << bits) - 8 and cols.size > 8    # more columns than slots up to the end: linear probing must wrap
    if name.startswith("c_tasks_"):
        per_row = np.bincount(t["seg"])
        assert int(per_row.max()) == int(name[8:]) and (TL_TASKS_MAX == 65471) and want[1] == 512 <= TL_CAP
    if name.startswith("b_kcap_"):
        a_rows = np.bincount(np.unique(A[2] // 8 * (1 << 32) + A[3] // 8) >> 32)
        assert int(a_rows[0] + a_rows[1]) == int(name[7:]) and want[0] <= STRIP_ROW_CAP and want[1] <= STRIP_ROW_CAP
    if name.startswith("b_jcap_"):
        assert want[0] + want[1] == int(name[7:])


def test_cap_walk_cases_step_by_step():
    """the two hand-made walks of strip mode (four A tiles side by side, sixteen B tiles of each per step): the count of distinct columns
    after every step"""
    def steps(tiles):
        seen, out = set(), []
        for g0 in range(0, len(tiles), 4):
            group = tiles[g0:g0 + 4]
            for s in range(max(-(-len(c) // 16) for c in group)):
                for c in group:
                    seen.update(np.unique(c)[16 * s:16 * s + 16].tolist())
                out.append(len(seen))
        return out
    a = steps(CAP["b_last_step"][0][1][1])
    assert a[-2] < STRIP_ROW_CAP < a[-1] and a[-2] == 250 and a[-1] == 257
    d = steps(CAP["b_duplicates"][0][1][1])
    first = d.index(STRIP_ROW_CAP)
    assert d[-1] == STRIP_ROW_CAP and len(d) - first > 10      # the cap is reached, and a dozen steps follow that bring nothing new


@pytest.mark.parametrize("name", ["a1", "a2_half", "a3_pass1", "b_256_all", "b_kcap_192", "c_896_wrap", "c_tasks_65471"])
def test_exact_values_are_exact(name):
    """the operands of the matrix-core runs: multiples of 1/4 up to 1 (fp16 holds them), so every product is a multiple of 1/16 and every
    C value's sum of magnitudes stays far below 2^24 / 16: exact in fp32 in any order"""
    A, B, _ = product(name, True)
    for v in (A[4], B[4]):
        assert np.array_equal(v * 4, np.round(v * 4)) and np.abs(v).max() <= 1 and np.abs(v).min() >= 0.25
        assert np.array_equal(v.astype(np.float16).astype(np.float64), v)
    t = product_terms(A, B)
    o = np.lexsort((t["j"], t["seg"]))
    key = t["seg"][o] * (1 << 32) + t["j"][o]
    _, inv = np.unique(key, return_inverse=True)
    mag = np.bincount(inv, weights=np.abs(t["a"][o].astype(np.float64) * t["b"][o]))
    assert mag.max() * 16 < 2 ** 24


def test_expansion_products(oracle):
    """exactly 2 << 20 candidate pairs, and one more (the oracle's counter), in segments a wave sorts"""
    for name, total in (("d_exact", SMALL_PRODUCT), ("d_plus_one", SMALL_PRODUCT + 1)):
        A, B, want = product(name)
        assert want == total
        t = product_terms(A, B)
        assert t["seg"].size == total and t["max_a"] * t["max_b"] == WIDE_CAP
    assert _oracle_product(oracle, "d_exact")[6]["task_list_size"] == SMALL_PRODUCT
