"""bmsp_spmm (csrc/spmm.hip): every launch path, stride, dtype and edge against a plain high-precision reference.

bmsp_spmm picks one of six launch paths.  On matrices that carry the SpMV position cache: spmm_vstream_kernel<4> (k <= 4) and
spmm_vstream_kernel<8> (k <= 8), each with a 16-byte x_vec branch; otherwise spmm_kernel<4> (k <= 4), spmm_kernel<16> (k <= 16) and
spmm_wide_kernel (larger k); k = 1 with unit strides is handed to the SpMV.  spmm_kernel<64> only runs once the value array reaches
2^32 elements: it cannot be reached at test sizes and is not tried here.  The kernel of every launch is asserted through
bmsp_spmm_launch_info before the launch.

Per launch:
  1. poison: Y is num_rows * ldy + 64 elements of 0xFF bytes (NaN); afterwards no NaN is left in Y[:, :k], the padding columns
     Y[:, k:ldy] and the 64-element tail are still 0xFF byte for byte, and the NaNs in the padding columns X[:, k:ldx] reach no output.
  2. exact family: A holds integers of {-4..4} \\ {0}, X integers of {-8..8}; every product and partial sum is an integer below 2^24, so
     any correct kernel returns the int64 result exactly, in any order and dtype: array_equal, no slack for a dropped, duplicated or
     misplaced element.
  3. rounding family: A ~ N(0, 1), X ~ U(-1, 1), both rounded to the input dtype; reference accumulated in np.longdouble from the
     rounded inputs.  Bound per output element (BOUND below):

         (2 n_i + 2) u (|A||X|)_ij + n_i * (smallest subnormal of the accumulator type)

     n_i = stored values of row i, u = 2^-24 for F32 and F16 (float accumulators), 2^-53 for F64.  Derivation: a sum of n products in
     any order, fused or not, folds included, is off by at most gamma_n ~ n u relative to |A||X| (each of the n - 1 additions and each
     product rounds once; a fused product does not round at all); adding an exact zero partial rounds nothing, so slots and items that
     hold nothing of the row cost nothing; the factor 2 covers the second-order terms of gamma_n and the non-fused product of the
     value-stream walk (product and add round separately: 2 n roundings).  The subnormal floor is the absolute error of n roundings
     that underflow.  The CPU tests below show that the bound passes float / double emulations of a correct kernel in three orders and
     fails fp16 accumulation (F16) and float accumulation (F64), without taking the code under test as the measure.
  4. at k = 3, columns 0 and k - 1 agree with bmsp_spmv of that column within the same bound.
  5. spmm_kernel<*> and spmm_wide_kernel: a second call gives identical bytes (the value-stream walk is exempt: its LDS adds come in
     hardware order).
  6. A's four arrays are byte-identical before and after.
  7. row-panel views: the panel's rows meet 1 to 3; the rows outside the panel are rows without stored values of the view (it keeps the
     parent's num_rows and its plan covers every block-row), so they are written as exact 0 -- asserted uniformly by the same
     comparisons, since the reference of a view holds the panel's entries only.
  8. the three argument errors return BMSP_ERR_INVALID and leave a poisoned Y untouched.
"""
import ctypes
import functools
import numpy as np
import pytest

LD = np.longdouble
KMAX_FULL, KMAX_SHORT = 100, 65
U = {0: 2.0 ** -24, 1: 2.0 ** -24, 2: 2.0 ** -53}       # unit roundoff of the accumulator type
ACC = {0: np.float32, 1: np.float32, 2: np.float64}
NP_IN = {0: np.float32, 1: np.float16, 2: np.float64}
DT_NAME = {0: "f32", 1: "f16", 2: "f64"}


# ---- the matrices (structure only; the values come with the family) ------------------------------------------------------------------
def _unique(nr, nc, r, c):
    key = np.unique(np.asarray(r, np.int64) * nc + np.asarray(c, np.int64))
    return nr, nc, (key // nc).astype(np.int32), (key % nc).astype(np.int32)


def _sparse_gaps():
    nr, nc = 1237, 911
    g = np.random.default_rng(101)
    r, c = g.integers(0, nr, 13000), g.integers(0, nc, 13000)
    hub = 701  # block-row 87 (87 % 3 == 0): one row with every column stored
    r, c = np.concatenate([r, np.full(nc, hub)]), np.concatenate([c, np.arange(nc)])
    br, last = r // 8, (nr + 7) // 8 - 1
    keep = (br % 3 != 1) & (br != 0) & (br != last)
    return _unique(nr, nc, r[keep], c[keep])


def _mid_density():
    nr, nc = 301, 403
    r, c = np.nonzero(np.random.default_rng(102).random((nr, nc)) < 6.0 / 64.0)
    return _unique(nr, nc, r, c)


def _tiles(g, brow, bcols, nr, nc, per_tile):
    """per_tile(n) random cells in each tile (brow, bc), clipped to the matrix"""
    rows, cols = [], []
    cnt = per_tile(len(bcols))
    for bc, n in zip(bcols.tolist(), cnt.tolist()):
        h, w = min(8, nr - 8 * brow), min(8, nc - 8 * bc)
        cell = g.choice(h * w, size=min(n, h * w), replace=False)
        rows.append(8 * brow + cell // w)
        cols.append(8 * bc + cell % w)
    return np.concatenate(rows), np.concatenate(cols)


def _long_rows():
    nr, nc = 29, 60011
    nbc = (nc + 7) // 8  # 7502, the last one three columns wide
    g = np.random.default_rng(103)
    some = lambda n: g.integers(1, 4, n)
    parts = [_tiles(g, 0, np.setdiff1d(np.arange(nbc), [5, 4000]), nr, nc, some),       # 7500 tiles: 30 items
             _tiles(g, 2, np.sort(g.choice(nbc, 257, replace=False)), nr, nc, some),     # 257 tiles: two items, the second of one tile
             _tiles(g, 3, np.sort(g.choice(nbc, 40, replace=False)), nr, nc, some)]      # short, rows 24..28
    return _unique(nr, nc, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))


def _full_tiles():
    nr, nc = 67, 1027
    r, c = np.divmod(np.arange(nr * nc), nc)
    return _unique(nr, nc, r, c)


def _gen(which, *a):
    from pybmsp import gen
    n, m, r, c, _ = getattr(gen, which)(*a)
    return _unique(n, m, r, c)


# name -> (structure, carries the position cache, full k list, row panel in block-rows or None)
CASES = {
    "sparse_gaps": (_sparse_gaps, True, True, None),
    "mid_density": (_mid_density, True, False, None),
    "long_rows": (_long_rows, True, True, None),
    "full_tiles": (_full_tiles, False, True, None),
    "dense_rowgroup": (lambda: _gen("banded", 1003, 12), False, False, None),
    "hub_rmat": (lambda: _gen("rmat", 11, 8), True, False, None),
    "panel_view": (lambda: _gen("rmat", 12, 4), True, False, (100, 390)),
    "empty": (lambda: (37, 21, np.zeros(0, np.int32), np.zeros(0, np.int32)), False, False, None),
    "one": (lambda: (1, 1, np.zeros(1, np.int32), np.zeros(1, np.int32)), True, False, None),
}
NONEMPTY = [c for c in CASES if c != "empty"]


@functools.lru_cache(maxsize=None)
def structure(case):
    """(nr, nc, r, c) sorted by (row, col), with the entries outside a view's panel kept (the parent's structure)"""
    return CASES[case][0]()


def panel_mask(case):
    nr, nc, r, c = structure(case)
    panel = CASES[case][3]
    return np.ones(r.size, bool) if panel is None else (r // 8 >= panel[0]) & (r // 8 < panel[1])


def kmax(case):
    return KMAX_FULL if CASES[case][2] else KMAX_SHORT


# ---- the two families and their references ----------------------------------------------------------------------------------------
def case_seed(case, salt):
    return [sorted(CASES).index(case), salt]


@functools.lru_cache(maxsize=2)
def exact_inputs(case):
    """(values, X, want): integer values / X as float64 and the int64 product (of the panel, for a view)"""
    nr, nc, r, c = structure(case)
    g = np.random.default_rng(case_seed(case, 1))
    v = g.integers(1, 5, r.size) * g.choice([-1, 1], r.size)
    X = g.integers(-8, 9, (nc, kmax(case)))
    import scipy.sparse as sp
    m = panel_mask(case)
    want = sp.coo_matrix((v[m].astype(np.int64), (r[m], c[m])), shape=(nr, nc)).tocsr() @ X.astype(np.int64)
    assert np.max(np.abs(want), initial=0) < 2 ** 24
    return v.astype(np.float64), X.astype(np.float64), np.asarray(want)


def row_sums_ld(nr, r, prod_of_cols, k):
    """sum over each row's entries (r sorted) of prod_of_cols(j0, j1) (nnz x (j1 - j0), longdouble), in column chunks"""
    out = np.zeros((nr, k), LD)
    if r.size == 0:
        return out
    starts = np.flatnonzero(np.r_[True, r[1:] != r[:-1]])
    for j0 in range(0, k, 16):
        j1 = min(k, j0 + 16)
        out[r[starts], j0:j1] = np.add.reduceat(prod_of_cols(j0, j1), starts, axis=0)
    return out


@functools.lru_cache(maxsize=2)
def rounding_inputs(case, dtype):
    """(values, X, ref, bound): values / X rounded to the input dtype, the longdouble product of the rounded inputs (of the panel, for
    a view) and the bound of check 3 per output element"""
    nr, nc, r, c = structure(case)
    g = np.random.default_rng(case_seed(case, 2))
    v = g.standard_normal(r.size).astype(NP_IN[dtype])
    X = g.uniform(-1.0, 1.0, (nc, kmax(case))).astype(NP_IN[dtype])
    m = panel_mask(case)
    rm, cm, vm = r[m], c[m], v[m].astype(LD)
    ref = row_sums_ld(nr, rm, lambda j0, j1: vm[:, None] * X[cm, j0:j1].astype(LD), X.shape[1])
    mag = row_sums_ld(nr, rm, lambda j0, j1: np.abs(vm)[:, None] * np.abs(X[cm, j0:j1].astype(LD)), X.shape[1])
    n_i = np.bincount(rm, minlength=nr).astype(LD)[:, None]
    bound = (2 * n_i + 2) * LD(U[dtype]) * mag + n_i * LD(np.finfo(ACC[dtype]).smallest_subnormal)
    return v, X, ref, bound


BOUND = "(2 n_i + 2) u |A||X| + n_i * smallest subnormal"


def longdouble_is_wide():
    return np.finfo(LD).nmant >= 63


def need_wide_longdouble(dtype):
    if dtype == 2 and not longdouble_is_wide():
        pytest.skip("np.longdouble has %d mantissa bits here, no wider than the double accumulators: the F64 rounding cases have no "
                    "higher-precision reference (every other case runs)" % np.finfo(LD).nmant)


# ---- CPU: each case has the property its row of the table names -----------------------------------------------------------------
def tile_stats(case):
    """(values per tile sorted by key, tiles per block-row, full tiles) of what the library is given (the panel, for a view)"""
    nr, nc, r, c = structure(case)
    m = panel_mask(case)
    r, c = r[m].astype(np.int64), c[m].astype(np.int64)
    nbc = (nc + 7) // 8
    key, per_tile = np.unique((r // 8) * nbc + c // 8, return_counts=True)
    per_row = np.bincount(key // nbc, minlength=(nr + 7) // 8)
    return per_tile, per_row, int(np.count_nonzero(per_tile == 64))


def plan_items(per_row, group):
    """the sweep plan's items as (first block-row, last + 1, tiles, part of a long block-row): block-rows of more than 256 tiles are cut
    into 256-tile items; the others are grouped until the running tile count crosses a multiple of `group`, a 16-block-row window
    ends or a long block-row intervenes"""
    rowptr = np.r_[0, np.cumsum(per_row)]
    items = []
    for b in range(len(per_row)):
        n = int(per_row[b])
        if n > 256:
            items += [(b, b + 1, min(256, n - t), True) for t in range(0, n, 256)]
        elif b == 0 or b % 16 == 0 or rowptr[b] // group != rowptr[b - 1] // group or per_row[b - 1] > 256 or items[-1][3]:
            items.append((b, b + 1, n, False))
        else:
            f, _, t, _ = items[-1]
            items[-1] = (f, b + 1, t + n, False)
    return items


@pytest.mark.parametrize("case", list(CASES))
def test_case_structure(case):
    nr, nc, r, c = structure(case)
    cache = CASES[case][1]
    per_tile, per_row, full = tile_stats(case)
    nnz, nb = int(per_tile.sum()), per_tile.size
    assert np.all(np.diff(r.astype(np.int64) * nc + c) > 0) and (r.size == 0 or (r.min() >= 0 and r.max() < nr and c.min() >= 0 and c.max() < nc))
    if case in ("sparse_gaps", "mid_density", "long_rows", "full_tiles"):
        assert nr % 8 and nc % 8
    if case == "empty":
        assert nb == 0 and nr % 8 and nc % 8
        return
    # the position cache is built for sparse tiles (under 16 values per tile, under a quarter of the tiles full); dense tiles without a
    # long block-row take the SpMV's row-group path, full tiles the FULL sweep: neither builds it
    if cache:
        assert nnz < 16 * nb and 4 * full < nb
    else:
        assert nnz >= 16 * nb and per_row.max() <= 256
    group = 256 if 4 * full >= nb else 96
    items = plan_items(per_row, group)
    assert sum(t for _, _, t, _ in items) == nb and items[0][0] == 0 and items[-1][1] == per_row.size
    if case == "sparse_gaps":
        last = per_row.size - 1
        empty = np.flatnonzero(per_row == 0)
        assert last == 154 and set(empty) == {b for b in range(last + 1) if b % 3 == 1 or b in (0, last)}
        assert 8000 <= nnz <= 10000 and np.bincount(r, minlength=nr).max() == nc  # the hub row
        # items that begin and items that end on an empty block-row, and more than one block-row per item
        assert any(per_row[f] == 0 for f, _, _, _ in items) and any(per_row[e - 1] == 0 for _, e, _, _ in items)
        assert per_row.max() <= 256
    if case == "mid_density":
        assert 5.0 <= nnz / nb <= 7.0
        # the first item holds more than one batch, and its first batch is cut by the 512 values before it reaches 128 tiles
        assert items[0][2] > 64 and np.cumsum(per_tile)[min(items[0][2], 128) - 1] > 512
        assert 64 < np.searchsorted(np.cumsum(per_tile), 512, side="right") < min(items[0][2], 128)
    if case == "long_rows":
        assert per_row.tolist() == [7500, 0, 257, 40]
        cnt = [sum(1 for f, _, _, lg in items if f == b and lg) for b in range(4)]
        assert cnt == [30, 0, 2, 0] and cnt[0] >= 17               # more than S = 16 / 4 / 1 items to fold
        assert [t for f, _, t, _ in items if f == 2] == [256, 1]    # a one-tile tail item
        assert set(np.unique(r[r >= 24])) <= set(range(24, 29)) and r.max() == 28 and c.max() >= nc - 3
    if case == "full_tiles":
        assert r.size == nr * nc and 4 * full >= nb and group == 256
        assert full == (nr // 8) * (nc // 8) and nb > full           # partial edge tiles on both sides
        assert any(t >= 64 for _, _, t, _ in items)                  # a 64-tile batch of full tiles: eight passes of kStreamCap values
    if case == "dense_rowgroup":
        assert nnz >= 16 * nb and per_row.max() <= 256
    if case == "hub_rmat":
        assert per_row.max() <= 256 and per_row.min() >= 1
    if case == "panel_view":
        lo, hi = CASES[case][3]
        assert per_row[:lo].sum() == 0 and per_row[hi:].sum() == 0 and per_row[lo:hi].min() >= 1
        assert np.count_nonzero(~panel_mask(case)[: np.argmax(panel_mask(case))]) > 0  # values before the panel: pos_base != 0
    if case == "one":
        assert (nr, nc, nnz) == (1, 1, 1)


# ---- CPU: the bound is attainable and discriminating ------------------------------------------------------------------------------
def emulate(r, prod, nr, acc_t, order):
    """row sums of prod (nnz x k, already rounded to the product type) accumulated in acc_t; r sorted.  order: "seq" a row's entries in
    key order, "rev" the reverse, "pair" adjacent pairs level by level (np.add.reduceat over two-element segments)"""
    k = prod.shape[1]
    out = np.zeros((nr, k), acc_t)
    if r.size == 0:
        return out
    starts = np.flatnonzero(np.r_[True, r[1:] != r[:-1]])
    lens = np.diff(np.r_[starts, r.size])
    rows = r[starts]
    if order == "pair":
        p, ln = prod.astype(acc_t), lens.copy()
        while ln.max() > 1:
            st = np.r_[0, np.cumsum(ln)[:-1]]
            half = (ln + 1) // 2
            # the start of every pair of every row: st[row] + 2 * (index inside the row's pairs)
            pair_row = np.repeat(np.arange(ln.size), half)
            idx = st[pair_row] + 2 * (np.arange(half.sum()) - np.repeat(np.r_[0, np.cumsum(half)[:-1]], half))
            p = np.add.reduceat(p, idx, axis=0).astype(acc_t)
            ln = half
        out[rows] = p
        return out
    acc = np.zeros((rows.size, k), acc_t)
    for t in range(int(lens.max())):
        on = lens > t
        idx = starts[on] + (t if order == "seq" else lens[on] - 1 - t)
        acc[on] = (acc[on].astype(prod.dtype) + prod[idx]).astype(acc_t)
    out[rows] = acc
    return out


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("case", list(CASES))
def test_bound_passes_correct_orders_and_fails_narrow_accumulators(case, dtype):
    need_wide_longdouble(dtype)
    k = 3
    nr, nc, r, c = structure(case)
    v, X, ref, bound = rounding_inputs(case, dtype)
    m = panel_mask(case)
    rm, cm, vm = r[m], c[m], v[m]
    ref, bound = ref[:, :k], bound[:, :k]
    acc_t = ACC[dtype]
    prod = vm.astype(acc_t)[:, None] * X[cm, :k].astype(acc_t)  # the separately rounded product
    assert prod.dtype == acc_t
    for order in ("seq", "rev", "pair"):
        got = emulate(rm, prod, nr, acc_t, order)
        over = np.abs(got.astype(LD) - ref) > bound
        assert not over.any(), (order, int(over.sum()), np.argwhere(over)[0].tolist())
    if case == "empty" or dtype == 0:
        return
    # the two wrong kernels the bound must catch: fp16 accumulators on F16 input, float accumulators on F64 input
    narrow = np.float16 if dtype == 1 else np.float32
    wide = np.float32 if dtype == 1 else np.float64
    got = emulate(rm, prod.astype(wide), nr, narrow, "seq")
    assert np.any(np.abs(got.astype(LD) - ref) > bound)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
# (k, ldx, ldy, BMSP_SPMM_NO_VSTREAM, X one element into its allocation)
FULL = [(1, 3, 3, 0, 0), (3, 3, 3, 0, 0), (4, 4, 4, 0, 0), (5, 5, 7, 0, 0), (8, 8, 8, 0, 0), (8, 11, 9, 0, 0), (8, 8, 8, 0, 1), (9, 9, 9, 0, 0),
        (16, 16, 19, 0, 0), (17, 17, 17, 0, 0), (64, 64, 64, 0, 0), (65, 67, 65, 0, 0), (100, 100, 101, 0, 0),
        (1, 2, 2, 1, 0), (3, 3, 5, 1, 0), (4, 4, 4, 1, 0), (5, 5, 5, 1, 0), (8, 8, 8, 1, 0), (1, 1, 1, 0, 0)]
SHORT = [(3, 3, 3, 0, 0), (8, 8, 8, 0, 0), (12, 13, 12, 0, 0), (65, 67, 65, 0, 0), (3, 3, 5, 1, 0), (1, 1, 1, 0, 0)]
LAUNCHES = [(case, dtype, cfg) for case in CASES for dtype in (0, 1, 2) for cfg in (FULL if CASES[case][2] else SHORT)]


def launch_id(p):
    case, dtype, (k, ldx, ldy, novs, unal) = p
    return "%s-%s-k%d_ldx%d_ldy%d%s%s" % (case, DT_NAME[dtype], k, ldx, ldy, "-novs" if novs else "", "-unaligned" if unal else "")


def expected_kernel(cache, k, ldx, ldy, novs):
    if k == 1 and ldx == 1 and ldy == 1:
        return "spmv: "
    if cache and k <= 8 and not novs:
        return "spmm_vstream_kernel<4>" if k <= 4 else "spmm_vstream_kernel<8>"
    return "spmm_kernel<4>" if k <= 4 else "spmm_kernel<16>" if k <= 16 else "spmm_wide_kernel"


def poisoned(bmsp, n, dtype):
    y = bmsp.DeviceArray(n, dtype)
    bmsp.check(bmsp.lib().bmsp_memset(y.ptr, 0xFF, y.n * y.dtype.itemsize))
    return y


@pytest.fixture(scope="module")
def matrices():
    """the device matrices of the (case, dtype) pair under test, by family; released when the pair changes and at the end of the module"""
    held = {}
    yield held
    held.clear()


def matrix(bmsp, held, case, dtype, family):
    """(the matrix the launches run on, its four host arrays at creation, the parent of a view and its arrays)"""
    key = (case, dtype, family)
    if key not in held:
        for old in [o for o in held if o[:2] != (case, dtype)]:
            del held[old]
        nr, nc, r, c = structure(case)
        v = exact_inputs(case)[0] if family == "exact" else rounding_inputs(case, dtype)[0]
        P = bmsp.BmSpMatrix.from_coo(nr, nc, r, c, v.astype(np.float64), dtype=dtype)
        A = P if CASES[case][3] is None else P.row_panel(*CASES[case][3])
        held[key] = (A, A.host_arrays(), P, P.host_arrays())
    return held[key]


def run(bmsp, monkeypatch, case, dtype, cfg, family, A, X):
    """one poisoned launch of cfg: asserts the kernel name and check 1; returns (Y[:, :k] on the host, kernel, a relaunch function)"""
    k, ldx, ldy, novs, unal = cfg
    nr, nc = structure(case)[:2]
    if novs:
        monkeypatch.setenv("BMSP_SPMM_NO_VSTREAM", "1")
    else:
        monkeypatch.delenv("BMSP_SPMM_NO_VSTREAM", raising=False)
    np_in, np_out = bmsp.NP_DTYPE[dtype], bmsp.OUT_DTYPE[dtype]
    Xs = np.full(unal + nc * ldx, np.nan, np_in)
    Xs[unal:].reshape(nc, ldx)[:, :k] = X[:, :k]
    dX = bmsp.DeviceArray.from_host(Xs)
    assert dX.ptr % 16 == 0 and (not unal or (dX.ptr + Xs.itemsize) % 16 != 0)
    kernel = bmsp.spmm_launch_info(A, k, ldx, ldy)
    want = expected_kernel(CASES[case][1], k, ldx, ldy, novs)
    if want == "spmv: ":
        assert kernel == "spmv: " + bmsp.spmv_launch_info(A)["kernel"]
    else:
        assert kernel == want

    def go():
        Y = poisoned(bmsp, nr * ldy + 64, np_out)
        bmsp.check(bmsp.lib().bmsp_spmm(A.h, dX.ptr + unal * Xs.itemsize, ldx, Y.ptr, ldy, k, None))
        return Y.to_host()

    h = go()
    Yv = h[:nr * ldy].reshape(nr, ldy)
    assert not np.isnan(Yv[:, :k]).any(), (kernel, "rows never stored or NaN read from padding", np.argwhere(np.isnan(Yv[:, :k]))[:4].tolist())
    assert np.all(np.ascontiguousarray(Yv[:, k:]).view(np.uint8) == 0xFF), (kernel, "padding columns of Y written")
    assert np.all(h[nr * ldy:].view(np.uint8) == 0xFF), (kernel, "tail of Y written")
    return Yv[:, :k], kernel, go


def assert_read_only(bmsp, held, case, dtype, family):
    A, a0, P, p0 = matrix(bmsp, held, case, dtype, family)
    for now, then in zip(A.host_arrays() + P.host_arrays(), a0 + p0):
        assert np.array_equal(now.view(np.uint8), then.view(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("launch", LAUNCHES, ids=launch_id)
def test_exact_family(bmsp, monkeypatch, matrices, launch):
    """checks 1, 2, 6, 7: small-integer inputs, the result equals the int64 product exactly"""
    case, dtype, cfg = launch
    _, X, want = exact_inputs(case)
    A = matrix(bmsp, matrices, case, dtype, "exact")[0]
    Y, kernel, _ = run(bmsp, monkeypatch, case, dtype, cfg, "exact", A, X)
    bad = Y != want[:, :cfg[0]].astype(Y.dtype)
    assert not bad.any(), (kernel, int(bad.sum()), "first (row, col)", np.argwhere(bad)[0].tolist())
    assert_read_only(bmsp, matrices, case, dtype, "exact")


@pytest.mark.gpu
@pytest.mark.parametrize("launch", LAUNCHES, ids=launch_id)
def test_rounding_family(bmsp, monkeypatch, matrices, launch):
    """checks 1, 3, 4, 5, 6, 7: random inputs against the longdouble reference within BOUND"""
    case, dtype, cfg = launch
    need_wide_longdouble(dtype)
    k = cfg[0]
    _, X, ref, bound = rounding_inputs(case, dtype)
    A = matrix(bmsp, matrices, case, dtype, "rounding")[0]
    Y, kernel, go = run(bmsp, monkeypatch, case, dtype, cfg, "rounding", A, X)
    err = np.abs(Y.astype(LD) - ref[:, :k])
    over = err > bound[:, :k]
    print("%s %s: max err / bound = %.3g" % (launch_id(launch), kernel, float(np.max(err / np.maximum(bound[:, :k], np.finfo(LD).tiny), initial=0))))
    assert not over.any(), (kernel, BOUND, int(over.sum()), "first (row, col)", np.argwhere(over)[0].tolist())
    if kernel.startswith("spmm_kernel") or kernel == "spmm_wide_kernel":
        nr, ldy = structure(case)[0], cfg[2]
        again = go()[:nr * ldy].reshape(nr, ldy)[:, :k]
        assert np.array_equal(np.ascontiguousarray(again).view(np.uint8), np.ascontiguousarray(Y).view(np.uint8)), (kernel, "second call differs")
    if cfg == (3, 3, 3, 0, 0):
        nr = structure(case)[0]
        lo, hi = (0, nr) if CASES[case][3] is None else (8 * CASES[case][3][0], 8 * CASES[case][3][1])
        for j in (0, k - 1):
            y = poisoned(bmsp, nr, bmsp.OUT_DTYPE[dtype])
            dx = bmsp.DeviceArray.from_host(np.ascontiguousarray(X[:, j]))
            bmsp.check(bmsp.lib().bmsp_spmv(A.h, dx.ptr, y.ptr, 0, None))
            y = y.to_host()[lo:hi]
            assert np.all(np.abs(y.astype(LD) - ref[lo:hi, j]) <= bound[lo:hi, j]), ("spmv", j)
            assert np.all(np.abs(y.astype(LD) - Y[lo:hi, j].astype(LD)) <= bound[lo:hi, j]), ("spmv against spmm", j)
    assert_read_only(bmsp, matrices, case, dtype, "rounding")


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_plan_items_match_the_library(bmsp, monkeypatch, case):
    """plan_items() above restates the plan's rules for the structure tests; this ties it to the plan the library builds.  With the
    chunked sweep and the row-group kernel switched off, bmsp_spmv_launch_info counts its compulsory bytes from the plan's items: 32 B
    per item, and for the cached value-stream kernel 64 B per item of a long block-row and 2 B per tile of every item that is not a
    single batch (short, <= 128 tiles, <= 512 values).  The same figures from plan_items() must give the same bytes."""
    monkeypatch.setenv("BMSP_SPMV_NOCHUNK", "1")
    monkeypatch.setenv("BMSP_SPMV_NO_ROWGROUP", "1")
    nr, nc, r, c = structure(case)
    P = bmsp.BmSpMatrix.from_coo(nr, nc, r, c, exact_inputs(case)[0], dtype=0)
    A = P if CASES[case][3] is None else P.row_panel(*CASES[case][3])
    per_tile, per_row, full = tile_stats(case)
    nv, nb = int(per_tile.sum()), per_tile.size
    items = plan_items(per_row, 256 if 4 * full >= nb else 96)
    li = bmsp.spmv_launch_info(A)
    xy = 4 * nc + 4 * nr
    if li["kernel"].startswith("spmv_vstream_kernel<kCached"):
        ends = np.cumsum([t for _, _, t, _ in items])
        vals = np.diff(np.r_[0, np.r_[0, np.cumsum(per_tile)][ends]])
        multi = sum(t for (_, _, t, lg), n in zip(items, vals.tolist()) if lg or t > 128 or n > 512)
        want = 32 * len(items) + xy + 64 * sum(1 for it in items if it[3]) + 4 * nv + 4 * nb + 2 * multi + 2 * nv
    else:
        assert li["kernel"].startswith("spmv_sweep_kernel"), li
        want = 32 * len(items) + 24 * nb + 4 * nv + xy
    assert li["compulsory_bytes"] == want, (li, len(items))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_zero_row_matrix_launches_nothing(bmsp, dtype):
    A = bmsp.BmSpMatrix.from_coo(0, 5, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), dtype=dtype)
    assert bmsp.spmm_launch_info(A, 3) == "none (empty matrix)" and bmsp.spmm_launch_info(A, 1) == "none (empty matrix)"
    X = bmsp.DeviceArray.from_host(np.ones(15, bmsp.NP_DTYPE[dtype]))
    Y = poisoned(bmsp, 64, bmsp.OUT_DTYPE[dtype])
    bmsp.check(bmsp.lib().bmsp_spmm(A.h, X.ptr, 3, Y.ptr, 3, 3, None))
    assert np.all(Y.to_host().view(np.uint8) == 0xFF)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_argument_errors(bmsp, dtype):
    """check 8: BMSP_ERR_INVALID through pybmsp.check, from bmsp_spmm and bmsp_spmm_launch_info alike, and Y stays as it was"""
    nr, nc, r, c = structure("mid_density")
    v = exact_inputs("mid_density")[0]
    A = bmsp.BmSpMatrix.from_coo(nr, nc, r, c, v, dtype=dtype)
    At = bmsp.BmSpMatrix.from_coo(nr, nc, r, c, v, transposed=True, dtype=dtype)
    X = bmsp.DeviceArray.from_host(np.ones(nc * 8, bmsp.NP_DTYPE[dtype]))
    Y = poisoned(bmsp, nr * 8 + 64, bmsp.OUT_DTYPE[dtype])
    name = ctypes.create_string_buffer(64)
    for M, k, ldx, ldy in ((At, 3, 3, 3), (A, 0, 3, 3), (A, 4, 3, 4), (A, 4, 4, 3)):
        with pytest.raises(bmsp.BmspError) as e:
            bmsp.check(bmsp.lib().bmsp_spmm(M.h, X.ptr, ldx, Y.ptr, ldy, k, None))
        assert e.value.status == -1  # BMSP_ERR_INVALID
        with pytest.raises(bmsp.BmspError) as e:
            bmsp.check(bmsp.lib().bmsp_spmm_launch_info(M.h, k, ldx, ldy, name, 64))
        assert e.value.status == -1
    bmsp.synchronize()
    assert np.all(Y.to_host().view(np.uint8) == 0xFF)
