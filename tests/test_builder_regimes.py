"""The builder and the COO / CSR conversions at every regime of the two device-wide primitives they are made of.

device_exclusive_scan switches by length (a lone workgroup up to 8192 elements, 1024-element tiles up to 2^20 and 4096 above, the
tile sums added up by each workgroup up to 1024 tiles and scanned recursively beyond), device_radix_sort_pairs by length (1024- or
4096-key tiles) and by key width (digit width ceil(bits / ceil(bits / 9)), two digits per thread above 256 bins, a histogram scan
of bins * tiles elements).  Every case here feeds UNSORTED input whose duplicate groups sum differently in a different order, and
compares bit for bit with the C oracle (stable comparison sort, duplicates summed in input order, rounded to the matrix type
after every add) or with numpy on the same triples.  The only tolerance is that of the device comparison's atomic double sum.
"""
import functools
import numpy as np
import pytest
import util
from pybmsp import gen

gpu = pytest.mark.gpu

NPDT = {0: np.float32, 1: np.float16, 2: np.float64}
BMSP_ERR_INVALID = -1
DUP_GAP = 8192  # a duplicate sits at least this far behind the entry it repeats: different sort tiles at both tile sizes (1024, 4096)
HUB = 10000     # entries of the one heavily repeated coordinate

# builder sizes: nnz (the builder scans nnz + 1 elements) -> what it crosses
SMALL_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 8191, 8192]
MID_SIZES = [(1 << 20) - 1, 1 << 20, (1 << 20) + 1]
SMALL_SHAPE = (5003, 3001)      # 25 key bits: 9 + 9 + 7, 512 bins
MID_SHAPE = (160000, 150001)    # 36 key bits: 4 x 9, 512 bins at both tile sizes
RECURSIVE = (4194304, (50001, 40007), False)   # scan of 4 194 305 elements = 1025 tiles of 4096; 32 key bits: 4 x 8, 256 bins
HIST_LONG = (8392705, MID_SHAPE, True)         # 2050 sort tiles x 512 bins > 2^20: the histogram scan on 4096-element tiles

# key widths: shape -> key bits = ceil_log2(block rows) + ceil_log2(block cols) + 6, and the passes the sort makes of them
WIDTH_SHAPES = [
    ((8, 8), 6, [6]),
    ((5, 7), 6, [6]),                      # num_rows < 8 and num_cols < 8: rbits = cbits = 0
    ((60, 5), 9, [9]),                     # one 512-bin pass
    ((60, 12), 10, [5, 5]),
    ((500, 500), 18, [9, 9]),
    ((1000, 500), 19, [7, 7, 5]),          # narrower last pass
    ((10000, 8000), 27, [9, 9, 9]),
    ((20000, 8000), 28, [7, 7, 7, 7]),
    ((40000001, 2 ** 31 - 1), 57, [9, 9, 9, 9, 9, 9, 3]),
    ((2 ** 27 + 5, 9), 32, [8, 8, 8, 8]),  # the tall mirror
]
WIDTH_NNZ = 20000


def ceil_log2(x):
    return 0 if x <= 1 else int(x - 1).bit_length()


def key_bits(shape):
    return ceil_log2((shape[0] + 7) // 8) + ceil_log2((shape[1] + 7) // 8) + 6


def sort_passes(bits):
    """the digit widths device_radix_sort_pairs uses for `bits` key bits"""
    passes = -(-bits // 9)
    width = -(-bits // passes)
    return [min(width, bits - s) for s in range(0, bits, width)]


# ---------------------------------------------------------------------------------------------------------
# input generator
# ---------------------------------------------------------------------------------------------------------
def _h(n, seed, salt):
    return gen.splitmix64(np.arange(n, dtype=np.uint64) + np.uint64(((seed * 64 + salt) << 34) & 0xFFFFFFFFFFFFFFFF))


@functools.lru_cache(maxsize=3)
def regime_input(nr, nc, n, seed=1):
    """n unsorted COO triples, uniform over nr x nc.  About one entry in eight repeats the coordinate of a root entry at least DUP_GAP
    positions before it (any earlier root when the case is shorter than that); roots are one entry in 32, so a group holds about
    five.  min(HUB, n // 8) further entries, spread evenly over the input, all sit on one coordinate.  Values are +-2^e (1 + k/8),
    e in [-12, 12]: a group's fp32 / fp16 sum depends on its order.  The hub's signs keep its running sum inside the largest
    magnitude, so no fp16 sum overflows into an inf whose NaN offspring would compare by payload.
    Returns (rows int32, cols int32, vals float64, group int64): group[i] is the root position of a repeated entry, -1 for the hub,
    -2 for the witness of per-add rounding (below), i for everything else."""
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64), np.zeros(0, np.int64)
    rows = (_h(n, seed, 0) % np.uint64(nr)).astype(np.int32)
    cols = (_h(n, seed, 1) % np.uint64(nc)).astype(np.int32)
    hv = _h(n, seed, 2)
    e = (hv % np.uint64(25)).astype(np.int64) - 12
    k = ((hv >> np.uint64(8)) % np.uint64(8)).astype(np.float64)
    sign = np.where((hv >> np.uint64(16)) & np.uint64(1), -1.0, 1.0)
    vals = sign * np.ldexp(1.0 + k / 8.0, e)
    hd = _h(n, seed, 3)
    idx = np.arange(n, dtype=np.int64)
    root_pos = np.flatnonzero(hd % np.uint64(32) == np.uint64(1))
    is_dup = hd % np.uint64(8) == np.uint64(0)
    # roots a repeated entry may pick: those at least DUP_GAP before it; in a short case (or near the start) any earlier one
    far = np.searchsorted(root_pos, idx - DUP_GAP, side="right")
    near = np.searchsorted(root_pos, idx - 1, side="right")
    avail = np.where(far > 0, far, near)
    is_dup &= avail > 0
    pick = ((hd >> np.uint64(8)) % np.maximum(avail, 1).astype(np.uint64)).astype(np.int64)
    group = idx.copy()
    if root_pos.size:
        group[is_dup] = root_pos[pick[is_dup]]
    rows, cols = rows[group], cols[group]
    hubs = min(HUB, n // 8)
    if hubs:
        at = (np.arange(hubs, dtype=np.int64) * n) // hubs + (n // hubs) // 2
        at = at[(group[at] == at) & ~np.isin(at, root_pos)]  # leave the groups alone
        hr, hc = int(_h(1, seed, 4)[0] % np.uint64(nr)), int(_h(1, seed, 5)[0] % np.uint64(nc))
        rows[at], cols[at] = hr, hc
        group[at] = -1
        run = 0.0
        mag = np.abs(vals[at])
        out = np.empty(at.size)
        for j in range(at.size):  # sign against the running sum: |run| never exceeds the largest magnitude
            out[j] = -mag[j] if run > 0 else mag[j]
            run += out[j]
        vals[at] = out
    # the witness: three entries of one coordinate, 2^12 + 2^-12 (1 + 1/8) - 2^12.  Rounded after every add this is 2^-11 in fp32 (the
    # small term is just over half an ulp of 4096) and 0 in fp16; summed exactly and rounded once it is the small term itself.  So every
    # input that holds it tells a builder that accumulates in a wider type from one that rounds as the matrix type does.
    free = np.flatnonzero((group == idx) & ~np.isin(idx, root_pos))
    if free.size >= 3:
        at = free[[free.size // 4, free.size // 2, (3 * free.size) // 4]]
        rows[at], cols[at] = int(_h(1, seed, 6)[0] % np.uint64(nr)), int(_h(1, seed, 7)[0] % np.uint64(nc))
        vals[at] = [4096.0, 1.125 * 2.0 ** -12, -4096.0]
        group[at] = -2
    for a in (rows, cols, vals, group):
        a.setflags(write=False)
    return rows, cols, vals, group


def reversed_groups(r, c, v, group):
    """the same triples with the members of every duplicate group (and of the hub) in reverse input order"""
    idx = np.arange(group.size)
    order = np.lexsort((idx, group))    # by group, then by position
    rev = np.lexsort((-idx, group))     # by group, then by position descending
    perm = np.empty(group.size, np.int64)
    perm[order] = rev                   # the k-th member of a group gives way to its k-th last
    return r[perm], c[perm], v[perm]


# ---------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------
def dev_triples(bmsp, r, c, v):
    return (bmsp.DeviceArray.from_host(r, np.int32), bmsp.DeviceArray.from_host(c, np.int32), bmsp.DeviceArray.from_host(v, np.float64))


def check_arrays(bmsp, ref, got, nr, nc, dtype, row_ptr=True):
    """the check_builder pattern of test_gpu_parity: counts, keys, bitmaps, offsets, values and the dense block-row pointer"""
    assert np.isfinite(ref.values).all()  # bit comparison of NaNs would compare payloads
    info = got.info()
    assert (info["num_rows"], info["num_cols"], info["nnz"], info["block_num"]) == (nr, nc, ref.nnz, ref.block_num)
    k, b, o, v = got.host_arrays()
    util.assert_bmsp_equal_exact(ref, k, b, o, v, NPDT[dtype])
    if row_ptr:
        rp = got.block_row_ptr()
        nbr = (nr + 7) // 8
        exp = np.searchsorted((ref.keys >> np.uint64(32)).astype(np.int64), np.arange(nbr + 1), side="left")
        np.testing.assert_array_equal(rp, exp.astype(np.uint32))


def check_regime(oracle, bmsp, shape, n, dtype, transposed, seed=1, row_ptr=True):
    nr, nc = shape
    r, c, v, _ = regime_input(nr, nc, n, seed)
    ref = oracle.bmsp_from_coo(oracle.Coo(nr, nc, r, c, v), dtype, transposed)
    got = bmsp.BmSpMatrix.from_coo_device(nr, nc, *dev_triples(bmsp, r, c, v), transposed=transposed, dtype=dtype)
    check_arrays(bmsp, ref, got, nr, nc, dtype, row_ptr)
    return ref, got


# ---------------------------------------------------------------------------------------------------------
# input self-checks (CPU, oracle only)
# ---------------------------------------------------------------------------------------------------------
def _order_sensitive_fraction(oracle, shape, n, dtype):
    nr, nc = shape
    r, c, v, g = regime_input(nr, nc, n)
    a = oracle.bmsp_from_coo(oracle.Coo(nr, nc, r, c, v), dtype, False)
    b = oracle.bmsp_from_coo(oracle.Coo(nr, nc, *reversed_groups(r, c, v, g)), dtype, False)
    np.testing.assert_array_equal(a.keys, b.keys); np.testing.assert_array_equal(a.bmps, b.bmps)
    assert np.isfinite(a.values).all() and np.isfinite(b.values).all()
    # both in (row, col) order, which is also the order of the sorted unique coordinates
    va, vb = oracle.bmsp_to_coo(a).vals, oracle.bmsp_to_coo(b).vals
    _, cnt = np.unique(r.astype(np.int64) * nc + c, return_counts=True)
    dup = cnt > 1
    return int((va != vb)[dup].sum()), int(dup.sum())


@pytest.mark.parametrize("dtype", [0, 1])
def test_input_is_order_sensitive(oracle, dtype):
    """an unstable sort can only show where a duplicate group's sum depends on its order: at least 1 % of the duplicated coordinates
    of the 1 048 577-entry input change value when every group is fed in reverse"""
    differ, dups = _order_sensitive_fraction(oracle, MID_SHAPE, (1 << 20) + 1, dtype)
    assert dups > 20000 and differ >= 0.01 * dups, (differ, dups)


@pytest.mark.parametrize("n", [s for s in SMALL_SIZES if s >= 63])
def test_small_inputs_are_order_sensitive(oracle, n):
    """... and every smaller case with duplicates holds at least one such coordinate in fp32 and in fp16"""
    for dtype in (0, 1):
        differ, dups = _order_sensitive_fraction(oracle, SMALL_SHAPE, n, dtype)
        assert dups >= 1 and differ >= 1, (dtype, differ, dups)


@pytest.mark.parametrize("shape,n", [(SMALL_SHAPE, s) for s in SMALL_SIZES if s >= 63] + [(MID_SHAPE, (1 << 20) + 1)])
def test_inputs_tell_per_add_rounding_from_one_final_rounding(oracle, shape, n):
    """a builder that sums duplicates in a wider type and rounds once would pass on input whose sums are all exact: every case with
    duplicates holds at least one coordinate whose fp32 and fp16 value, rounded after every add, differs from the exact sum rounded
    once.  (The fp64 sums are exact: all values are multiples of 2^-15 below 2^13, a coordinate holds at most some 10^4 of them.)"""
    nr, nc = shape
    r, c, v, g = regime_input(nr, nc, n)
    assert (g == -2).sum() == 3
    exact = oracle.bmsp_from_coo(oracle.Coo(nr, nc, r, c, v), 2, False).values
    for dtype in (0, 1):
        per_add = oracle.bmsp_from_coo(oracle.Coo(nr, nc, r, c, v), dtype, False).values
        assert (per_add != exact.astype(NPDT[dtype]).astype(np.float64)).sum() >= 1, dtype


def test_input_duplicates_span_sort_tiles():
    """the members of at least half of the duplicate groups lie in different 4096-entry input tiles; one entry in eight is a repeat,
    none closer than DUP_GAP to its root once the input is long enough; the hub is spread over the whole input"""
    n = (1 << 20) + 1
    r, c, v, g = regime_input(*MID_SHAPE, n)
    idx = np.arange(n)
    rep = (g != idx) & (g >= 0)
    assert 0.10 * n < rep.sum() < 0.15 * n
    late = rep & (idx >= 4 * DUP_GAP)
    assert (idx[late] - g[late]).min() >= DUP_GAP
    assert np.array_equal(r[rep], r[g[rep]]) and np.array_equal(c[rep], c[g[rep]])
    lo, hi = idx // 4096, idx // 4096  # first and last input tile of every group, kept at its root
    lo, hi = lo.copy(), hi.copy()
    np.minimum.at(lo, g[rep], idx[rep] // 4096); np.maximum.at(hi, g[rep], idx[rep] // 4096)
    roots = np.unique(g[rep])
    assert (lo[roots] != hi[roots]).sum() >= 0.5 * roots.size
    hub = np.flatnonzero(g == -1)
    assert 0.8 * HUB <= hub.size <= HUB and hub[0] < n // 100 and hub[-1] > n - n // 100  # its sorted run crosses 4096-key tiles
    assert np.unique(r[hub]).size == 1 and np.unique(c[hub]).size == 1
    assert not np.all(np.diff(r.astype(np.int64) * MID_SHAPE[1] + c) >= 0)  # unsorted
    assert np.all(np.abs(v) * 2.0 ** 15 == np.round(np.abs(v) * 2.0 ** 15)) and np.unique(np.frexp(v)[1]).size == 25


def test_width_table():
    """the shapes of the key-width cases give the widths and passes their table claims"""
    for shape, bits, passes in WIDTH_SHAPES:
        assert key_bits(shape) == bits, shape
        assert sort_passes(bits) == passes, shape
    assert sorted({b for _, b, _ in WIDTH_SHAPES}) == [6, 9, 10, 18, 19, 27, 28, 32, 57]
    assert key_bits(SMALL_SHAPE) == 25 and sort_passes(25) == [9, 9, 7]
    assert key_bits(MID_SHAPE) == 36 and sort_passes(36) == [9, 9, 9, 9]
    assert key_bits(RECURSIVE[1]) == 32
    # the regime edges of the builder sizes, from the constants of prims.hip.h
    assert -(-(RECURSIVE[0] + 1) // 4096) == 1025 and -(-RECURSIVE[0] // 4096) == 1024
    assert -(-HIST_LONG[0] // 4096) == 2050 and 2050 * 512 > 1 << 20


# ---------------------------------------------------------------------------------------------------------
# builder against the oracle at the regime edges
# ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("n", SMALL_SIZES)
def test_builder_small_regimes(oracle, bmsp, n, dtype, transposed):
    """empty input, one wave round, one wave's slice, one sort tile, and the scan of 8192 / 8193 elements (lone workgroup / tile sums)"""
    check_regime(oracle, bmsp, SMALL_SHAPE, n, dtype, transposed)


@gpu
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("n", MID_SIZES)
def test_builder_around_2_20(oracle, bmsp, n, dtype, transposed):
    """2^20 - 1: everything on 1024 tiles; 2^20: the scan of nnz + 1 moves to 4096 tiles one entry before the sort; 2^20 + 1: both"""
    check_regime(oracle, bmsp, MID_SHAPE, n, dtype, transposed)


@gpu
@pytest.mark.parametrize("case", [RECURSIVE, HIST_LONG], ids=["scan_1025_tiles", "hist_scan_4096_tiles"])
def test_builder_large_regimes(oracle, bmsp, case):
    """the recursive scan (1025 tiles of 4096) and a histogram scan long enough for 4096-element tiles"""
    n, shape, transposed = case
    check_regime(oracle, bmsp, shape, n, 0, transposed)


# ---------------------------------------------------------------------------------------------------------
# key widths
# ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("shape,bits,passes", WIDTH_SHAPES, ids=["%dx%d" % s for s, _, _ in WIDTH_SHAPES])
def test_builder_key_widths(oracle, bmsp, shape, bits, passes, transposed):
    """one to seven passes, even and narrower last digits, one and two digits per thread; the arrays are the check (no x fits)"""
    assert key_bits(shape) == bits and sort_passes(bits) == passes
    check_regime(oracle, bmsp, shape, WIDTH_NNZ, 0, transposed, row_ptr=shape[0] < 2 ** 27)  # 2^24 block rows: pointer not fetched, for size


# ---------------------------------------------------------------------------------------------------------
# conversions at the same edges
# ---------------------------------------------------------------------------------------------------------
def input_with_stored(shape, stored, seed=2):
    """the shortest prefix of the generator's input that holds exactly `stored` distinct coordinates"""
    nr, nc = shape
    if stored == 0:
        return regime_input(nr, nc, 0, seed)[:3]
    n = stored + stored // 2 + 16
    r, c, v, _ = regime_input(nr, nc, n, seed)
    _, first = np.unique(r.astype(np.int64) * nc + c, return_index=True)
    first.sort()
    assert first.size > stored
    cut = first[stored]  # position of the first entry with a (stored + 1)-th coordinate
    return r[:cut], c[:cut], v[:cut]


def check_conversions(oracle, bmsp, shape, r, c, v, dtype, transposed, csr=True):
    nr, nc = shape
    ref = oracle.bmsp_from_coo(oracle.Coo(nr, nc, r, c, v), dtype, transposed)
    assert np.isfinite(ref.values).all()
    back = oracle.bmsp_to_coo(ref)  # sorted by (row, col), values exact in the matrix type
    M = bmsp.BmSpMatrix.from_coo_device(nr, nc, *dev_triples(bmsp, r, c, v), transposed=transposed, dtype=dtype)
    assert M.nnz == ref.nnz
    hr, hc, hv = M.to_coo()
    np.testing.assert_array_equal(hr, back.rows); np.testing.assert_array_equal(hc, back.cols); np.testing.assert_array_equal(hv, back.vals)
    dr, dc, dv = (a.to_host() for a in M.to_coo_device())
    np.testing.assert_array_equal(dr, back.rows); np.testing.assert_array_equal(dc, back.cols); np.testing.assert_array_equal(dv, back.vals)
    if not csr:
        return M, ref
    csr_dev = M.to_csr_device()
    ro, cc, vv = (a.to_host() for a in csr_dev)
    want = np.zeros(nr + 1, np.int64)
    np.cumsum(np.bincount(back.rows, minlength=nr), out=want[1:])
    np.testing.assert_array_equal(ro, want.astype(np.int32))
    np.testing.assert_array_equal(cc, back.cols); np.testing.assert_array_equal(vv, back.vals)
    M2 = bmsp.BmSpMatrix.from_csr_device(nr, nc, *csr_dev, transposed=transposed, dtype=dtype)
    for x, y in zip(M2.host_arrays(), M.host_arrays()):
        np.testing.assert_array_equal(x, y)
    util.assert_bmsp_equal_exact(ref, *M2.host_arrays(), NPDT[dtype])
    return M, ref


@gpu
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("stored", [0, 1, 8192, 8193])
def test_conversions_small_counts(oracle, bmsp, stored, dtype, transposed):
    r, c, v = input_with_stored(SMALL_SHAPE, stored)
    M, _ = check_conversions(oracle, bmsp, SMALL_SHAPE, r, c, v, dtype, transposed)
    assert M.nnz == stored


@gpu
@pytest.mark.parametrize("stored,transposed", [(1 << 20, False), (1 << 20, True), ((1 << 20) + 1, False), ((1 << 20) + 1, True),
                                               (4200000, False), (4200000, True)])
def test_conversions_large_counts(oracle, bmsp, stored, transposed):
    """2^20 stored values: the two partial sorts on 1024-key tiles; one more: on 4096-key tiles; 4.2 M: 1026 tiles of 4096"""
    r, c, v = input_with_stored(MID_SHAPE, stored)
    M, _ = check_conversions(oracle, bmsp, MID_SHAPE, r, c, v, 0, transposed)
    assert M.nnz == stored


# cb = ceil_log2(num_cols) and rb = ceil_log2(num_rows) are the widths of the two partial sorts of the expansion
CONV_SHAPES = [(20000, 1), (20000, 8), (20000, 9), (20000, 512), (20000, 513), (3001, 2 ** 31 - 1), (1, 20000), (8, 20000), (9, 20000)]


@gpu
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=["%dx%d" % s for s in CONV_SHAPES])
def test_conversions_sort_widths(oracle, bmsp, shape, dtype):
    """num_cols = 1 / num_rows = 1 leave one of the sorts with no bits at all; 8 | 9 and 512 | 513 step cb; 2^31 - 1 is 31 bits, 4 x 8"""
    # a shape of few cells holds hundreds of entries per coordinate: fp16 sums of +-2^12 would overflow there
    n = 20000 if dtype != 1 or shape[0] * shape[1] > 10 ** 6 else min(20000, shape[0] * shape[1] // 8)
    r, c, v, _ = regime_input(shape[0], shape[1], n, 3)
    for transposed in (False, True):
        check_conversions(oracle, bmsp, shape, r, c, v, dtype, transposed)


@gpu
def test_conversions_tall(oracle, bmsp):
    """num_rows = 2^27 + 5: rb = 28, four passes of 7.  COO only: the CSR offsets alone would be half a gigabyte"""
    shape = (2 ** 27 + 5, 9)
    r, c, v, _ = regime_input(shape[0], shape[1], 20000, 3)
    for transposed in (False, True):
        check_conversions(oracle, bmsp, shape, r, c, v, 0, transposed, csr=False)


@gpu
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_conversions_row_gaps(oracle, bmsp, dtype):
    """non-empty rows more than 100 000 empty rows apart, and empty rows at both ends: the fill loop of the CSR offsets"""
    at = np.array([3, 150000, 150001, 300007, 450012], np.int32)
    shape = (600000, 50)
    r, c, v, _ = regime_input(at.size, shape[1], 600, 4)
    for transposed in (False, True):
        check_conversions(oracle, bmsp, shape, at[r], c, v, dtype, transposed)


@gpu
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("num_rows", [0, 1, 5])
def test_conversions_empty(oracle, bmsp, num_rows, dtype):
    none = regime_input(7, 7, 0)[:3]
    for transposed in (False, True):
        M, _ = check_conversions(oracle, bmsp, (num_rows, 7), *none, dtype, transposed)
        assert (M.nnz, M.block_num) == (0, 0)
        np.testing.assert_array_equal(M.to_csr_device()[0].to_host(), np.zeros(num_rows + 1, np.int32))


@gpu
@pytest.mark.parametrize("stored", [(1 << 20) + 1, 2100000])
def test_compare_large(oracle, bmsp, stored):
    """bmSpMatrix::compare, host and device, against the formula of bmsp.h in numpy float64: a permuted comparand that lacks every
    11th entry, holds entries the matrix lacks and, for about 1000 coordinates, two entries of different value (the first in input
    order counts, as with the stable host sort)"""
    nr, nc = MID_SHAPE
    r, c, v = input_with_stored(MID_SHAPE, stored)
    M, ref = check_conversions(oracle, bmsp, MID_SHAPE, r, c, v, 0, False, csr=False)
    back = oracle.bmsp_to_coo(ref)
    mr, mc, mv = back.rows, back.cols, back.vals
    n = mr.size
    assert n == stored
    mkey = (mr.astype(np.uint64) << np.uint64(32)) | mc.astype(np.uint64)
    cv = mv.copy()
    cv[::7] *= 1.0 + 1e-3                      # relative error 1e-3 on every 7th entry
    keep = np.ones(n, bool); keep[5::11] = False
    twice = np.flatnonzero(keep)[::max(1, int(keep.sum()) // 1000)]  # coordinates the comparand holds twice
    h = gen.splitmix64(np.arange(3000, dtype=np.uint64) + np.uint64(77 << 40))
    er, ec = (h % np.uint64(nr)).astype(np.int32), ((h >> np.uint64(32)) % np.uint64(nc)).astype(np.int32)
    fresh = ~np.isin((er.astype(np.uint64) << np.uint64(32)) | ec.astype(np.uint64), mkey)  # entries only the comparand has
    r3 = np.concatenate([mr[keep], mr[twice], er[fresh]])
    c3 = np.concatenate([mc[keep], mc[twice], ec[fresh]])
    v3 = np.concatenate([cv[keep], cv[twice] * 1.5 + 1.0, np.full(int(fresh.sum()), 9.0)])
    perm = gen.splitmix64(np.arange(r3.size, dtype=np.uint64) + np.uint64(78 << 40)).argsort(kind="stable")
    r3, c3, v3 = r3[perm], c3[perm], v3[perm]
    # expectation: the first comparand entry, in input order, of every coordinate the matrix holds
    ckey = (r3.astype(np.uint64) << np.uint64(32)) | c3.astype(np.uint64)
    order = np.argsort(ckey, kind="stable")
    at = np.searchsorted(ckey[order], mkey, side="left")
    hit = at < ckey.size
    hit[hit] = ckey[order][at[hit]] == mkey[hit]
    missing = int((~hit).sum())
    assert missing == int((~keep).sum()) and 900 <= twice.size <= 1100 and fresh.sum() > 2900
    e = v3[order[at[hit]]]
    assert (e != cv[hit]).sum() > 300  # the permutation put the second entry first for a good part of the coordinates held twice
    eps = 1e-8
    e = np.where(np.abs(e) < eps, 0.0, e); m = np.where(np.abs(mv[hit]) < eps, 0.0, mv[hit])
    want = float(np.sum(np.abs(e - m) / np.maximum(np.abs(e), eps)) / n)
    host_err, host_miss = M.compare(r3, c3, v3)
    dev_err, dev_miss = M.compare_device(*dev_triples(bmsp, r3, c3, v3))
    print("compare at %d stored values: expected %.17g, host %.17g, device %.17g, missing %d" % (n, want, host_err, dev_err, missing))
    assert dev_miss == host_miss == missing
    tol = 1e-12 * max(1.0, want)
    assert abs(host_err - want) <= tol and abs(dev_err - want) <= tol and abs(dev_err - host_err) <= tol and want > 0


# ---------------------------------------------------------------------------------------------------------
# the device entry points reject bad input.  These tests only ever call the builder: its kernels index by entry number, so a
# malformed call is memory-safe whether or not it is refused, and no refused or malformed matrix is handed to an operator.
# ---------------------------------------------------------------------------------------------------------
GOOD = 5000


def _good(bmsp):
    nr, nc = SMALL_SHAPE
    r, c, v, _ = regime_input(nr, nc, GOOD, 5)
    return nr, nc, r.copy(), c.copy(), v.copy()


def _expect_invalid(bmsp, call):
    with pytest.raises(bmsp.BmspError) as ei:
        m = call()
        del m
    assert ei.value.status == BMSP_ERR_INVALID, ei.value


def _well_formed_after(oracle, bmsp):
    """a well-formed call straight after a refused one gives oracle-exact arrays: nothing was left half-built in the pool"""
    nr, nc, r, c, v = _good(bmsp)
    ref = oracle.bmsp_from_coo(oracle.Coo(nr, nc, r, c, v), 0, False)
    got = bmsp.BmSpMatrix.from_coo_device(nr, nc, *dev_triples(bmsp, r, c, v))
    check_arrays(bmsp, ref, got, nr, nc, 0)
    ro = np.searchsorted(oracle.bmsp_to_coo(ref).rows, np.arange(nr + 1), side="left").astype(np.int32)
    M2 = bmsp.BmSpMatrix.from_csr_device(nr, nc, *got.to_csr_device())
    np.testing.assert_array_equal(got.to_csr_device()[0].to_host(), ro)
    util.assert_bmsp_equal_exact(ref, *M2.host_arrays(), np.float32)


@gpu
@pytest.mark.parametrize("where", [0, GOOD // 2, GOOD - 1], ids=["first", "middle", "last"])
@pytest.mark.parametrize("what", ["row_eq_num_rows", "col_eq_num_cols", "negative_row", "negative_col"])
def test_from_coo_device_rejects_index_outside_shape(oracle, bmsp, what, where):
    nr, nc, r, c, v = _good(bmsp)
    if what == "row_eq_num_rows": r[where] = nr
    elif what == "col_eq_num_cols": c[where] = nc
    elif what == "negative_row": r[where] = -1
    else: c[where] = -1
    for transposed in (False, True):
        _expect_invalid(bmsp, lambda: bmsp.BmSpMatrix.from_coo_device(nr, nc, *dev_triples(bmsp, r, c, v), transposed=transposed))
    _well_formed_after(oracle, bmsp)


@gpu
@pytest.mark.parametrize("what", ["col_out_of_range", "negative_col", "first_offset_not_0", "last_offset_not_nnz", "decreasing_offsets",
                                  "decreasing_offsets_of_empty_rows"])
def test_from_csr_device_rejects_malformed_input(oracle, bmsp, what):
    nr, nc, r, c, v = _good(bmsp)
    order = np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    ro = np.searchsorted(r, np.arange(nr + 1), side="left").astype(np.int32)
    assert ro[0] == 0 and ro[-1] == GOOD
    if what == "col_out_of_range": c[GOOD // 3] = nc
    elif what == "negative_col": c[GOOD - 1] = -5
    elif what == "first_offset_not_0": ro[0] = 1
    elif what == "last_offset_not_nnz": ro[-1] = GOOD - 1
    elif what == "decreasing_offsets":
        k = int(np.flatnonzero(np.diff(ro) > 0)[nr // 3])  # a row that holds entries: its end moves before its start
        ro[k + 1] = ro[k] - 1
    else:
        k = int(np.flatnonzero((np.diff(ro)[:-1] == 0) & (np.diff(ro)[1:] == 0))[7])  # rows k, k + 1 empty: no entry sees the dip
        ro[k + 1] -= 1
        assert ro[k] > ro[k + 1] < ro[k + 2]
    dev = lambda: (bmsp.DeviceArray.from_host(ro, np.int32), bmsp.DeviceArray.from_host(c, np.int32), bmsp.DeviceArray.from_host(v, np.float64))
    _expect_invalid(bmsp, lambda: bmsp.BmSpMatrix.from_csr_device(nr, nc, *dev()))
    _well_formed_after(oracle, bmsp)


@gpu
def test_device_entry_points_reject_unknown_dtype(oracle, bmsp):
    nr, nc, r, c, v = _good(bmsp)
    _expect_invalid(bmsp, lambda: bmsp.BmSpMatrix.from_coo_device(nr, nc, *dev_triples(bmsp, r, c, v), dtype=7))
    order = np.lexsort((c, r))
    ro = np.searchsorted(r[order], np.arange(nr + 1), side="left").astype(np.int32)
    _expect_invalid(bmsp, lambda: bmsp.BmSpMatrix.from_csr_device(nr, nc, bmsp.DeviceArray.from_host(ro, np.int32),
                                                                  bmsp.DeviceArray.from_host(c[order], np.int32),
                                                                  bmsp.DeviceArray.from_host(v[order], np.float64), dtype=7))
    _well_formed_after(oracle, bmsp)
