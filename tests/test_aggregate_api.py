"""CPU tests of the surface of bmsp_matrix_aggregate / bmsp_matrix_from_aggregates, and what tests/test_zzzzzzzzz_aggregate.py shares with
them: the named inputs and the plain-Python reference of the aggregation -- the rule of include/bmsp.h: the greedy distance-2 independent
set in descending key order, the assignment rule, and a simulation of the documented round schedule (two launches a round, elimination
lagging one round) for `rounds`.

Checked here without a GPU, per input and for the seeds 0 and 12345: the Luby simulation and the greedy agree on the roots; roots are
pairwise further than 2 apart; every node is within 2 of its own root; every aggregate is connected; ids are dense and ascend with the
root index; each input has the property it is named for.  Also: the prototypes and the layout of bmsp_aggregate_info in bmsp.h, the
Python wrappers, the refusals of the C entry points that need no device (the argument named), and the C++ wrappers (compile + link)."""
import ctypes as C
import functools
import inspect
import os
import subprocess
import numpy as np
import pytest
from conftest import REPO
from test_spsv_api import _msg, _flat

BMSP_ERR_INVALID = -1
NAMES = ("empty", "one", "diag7", "path203", "grid13x11", "dense24", "star530", "lowerpath", "intile", "zeros", "rand1000")
SEEDS = (0, 12345)
ROOT = 1 << 64          # above every key: what a root reads as in the first-level pass
SKIP = 0xFFFFFFFF
# intile: 5 diagonal tiles with off-diagonal bits inside them (one-sided, so both directions are decoded), node 38 linked to the rest by
# ONE bit of the off-diagonal tile (0, 4)
INTILE_IN = ((1, 4), (2, 7), (5, 3), (6, 0), (7, 5))
INTILE_LINK = (6, 38)


# ---------------------------------------------------------------------------------------------------------
# the inputs
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pattern(name):
    """(n, rows, cols) of a named input, sorted by (row, col), int64"""
    from pybmsp import gen
    if name == "empty":
        n, r, c = 0, [], []
    elif name == "one":
        n, r, c = 1, [0], [0]
    elif name == "diag7":
        n, r, c = 7, np.arange(7), np.arange(7)
    elif name == "path203":
        n, i = 203, np.arange(202)
        r, c = np.concatenate([np.arange(203), i, i + 1]), np.concatenate([np.arange(203), i + 1, i])
    elif name == "lowerpath":                   # the strict lower triangle of path203
        n, r, c = pattern("path203")
        keep = r > c
        r, c = r[keep], c[keep]
    elif name in ("grid13x11", "zeros"):
        n, _, r, c, _ = gen.poisson("5pt", 13, 11)
    elif name == "dense24":
        n = 24
        r, c = [a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij")]
    elif name == "star530":                     # node 0 adjacent to all: block-row 0 holds 67 tiles
        n, i = 530, np.arange(530)
        r, c = np.concatenate([i, np.zeros(530, np.int64), i]), np.concatenate([i, i, np.zeros(530, np.int64)])
    elif name == "intile":
        n = 40
        pairs = [(8 * b + i, 8 * b + j) for b in range(5) for i, j in INTILE_IN if 38 not in (8 * b + i, 8 * b + j)] + [INTILE_LINK]
        r, c = [p[0] for p in pairs], [p[1] for p in pairs]
    elif name == "rand1000":
        n, _, r, c, _ = gen.random_coo(1000, 1000, 4000, seed=3)
    else:
        raise KeyError(name)
    n = int(n)
    key = np.unique(np.asarray(r, np.int64) * max(n, 1) + np.asarray(c, np.int64))
    r, c = key // max(n, 1), key % max(n, 1)
    r.setflags(write=False)
    c.setflags(write=False)
    return n, r, c


def values(name, dtype, seed=7):
    """one value per stored entry of input `name`, rounded to the dtype: generic and non-zero, except `zeros`, whose off-diagonal values
    are stored zeros"""
    n, r, c = pattern(name)
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.5, 2.0, r.size) * rng.choice([-1.0, 1.0], r.size)
    if name == "zeros":
        v[r != c] = 0.0
    return v.astype({0: np.float32, 1: np.float16, 2: np.float64}[dtype]).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def neighbours(name):
    """adj[i] = the sorted nodes j != i with (i, j) or (j, i) stored"""
    n, r, c = pattern(name)
    off = r != c
    m = max(n, 1)
    e = np.unique(np.concatenate([r[off] * m + c[off], c[off] * m + r[off]]))
    ptr = np.searchsorted(e // m, np.arange(n + 1))
    other = e % m
    return [other[ptr[i]:ptr[i + 1]].tolist() for i in range(n)]


def node_keys(n, seed):
    """K(i) = (splitmix64(seed ^ i) >> 32) << 32 | i, + 1 (0 = none), as Python integers: the order of (hash32, i)"""
    from pybmsp import gen
    ids = np.arange(n, dtype=np.uint64)
    h = gen.splitmix64(np.uint64(seed) ^ ids) >> np.uint64(32)
    return [((int(a) << 32) | i) + 1 for i, a in enumerate(h)]


def within2(adj, i):
    out = {i}
    for j in adj[i]:
        out.add(j)
        out.update(adj[j])
    return out


def greedy_roots(adj, K):
    """i becomes a root iff no node already chosen lies within distance <= 2: sequentially, in descending key order"""
    root = [False] * len(adj)
    for i in sorted(range(len(adj)), key=lambda i: -K[i]):
        if not any(root[j] for j in within2(adj, i)):
            root[i] = True
    return root


def luby_roots(adj, K):
    """(root flags, rounds) of the schedule of csrc/aggregate.hip: per round, first m1[i] = max w over N[i] for EVERY node (w = K while
    undecided, ROOT for a root, 0 once eliminated), then for every undecided i the maximum m2 of m1 over N[i]: ROOT eliminates i, its
    own key makes it a root.  The roots of a round eliminate in the next one; every round decides at least one node."""
    n = len(adj)
    w = list(K)
    rounds = 0
    while any(0 < x < ROOT for x in w):
        m1 = [max([w[i]] + [w[j] for j in adj[i]]) for i in range(n)]
        nw = list(w)
        for i in range(n):
            if 0 < w[i] < ROOT:
                m2 = max([m1[i]] + [m1[j] for j in adj[i]])
                nw[i] = 0 if m2 == ROOT else (ROOT if m2 == K[i] else w[i])
        assert nw != w, "a round decided no node"
        w = nw
        rounds += 1
    return [x == ROOT for x in w], rounds


def assign(adj, K, root):
    """ids by rank among the roots; a non-root joins the neighbouring root of greatest key, else the greatest root its neighbours touch"""
    n = len(adj)
    rank = np.cumsum([0] + [int(f) for f in root])
    p1 = [max([K[i] if root[i] else 0] + [K[j] for j in adj[i] if root[j]]) for i in range(n)]
    agg = np.zeros(n, np.uint32)
    for i in range(n):
        t = K[i] if root[i] else (p1[i] or max([0] + [p1[j] for j in adj[i]]))
        assert t, "the independent set is not maximal"
        agg[i] = rank[(t - 1) & 0xFFFFFFFF]
    return agg


@functools.lru_cache(maxsize=None)
def reference(name, seed):
    """(agg uint32, num_aggregates, rounds, root flags) of input `name`"""
    n = pattern(name)[0]
    adj, K = neighbours(name), node_keys(n, seed)
    root, rounds = luby_roots(adj, K)
    agg = assign(adj, K, root)
    agg.setflags(write=False)
    return agg, int(sum(root)), rounds, tuple(root)


def kernel_name(n, lay):
    return "agg_pass_kernel<layout %d>" % lay if n else "none (empty matrix)"


# ---------------------------------------------------------------------------------------------------------
# the reference's self-checks
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", NAMES)
def test_reference_is_a_greedy_mis2_with_connected_aggregates(name, seed):
    n = pattern(name)[0]
    adj, K = neighbours(name), node_keys(n, seed)
    agg, num, rounds, root = reference(name, seed)
    assert list(root) == greedy_roots(adj, K)                       # the Luby rounds give the sequential greedy set
    roots = [i for i in range(n) if root[i]]
    assert num == len(roots) and (rounds >= 1) == (n > 0)
    for i in roots:                                                 # pairwise further than 2 apart
        assert within2(adj, i) & set(roots) == {i}, (name, i)
    assert [int(agg[i]) for i in roots] == list(range(num))         # dense, ascending with the root index
    assert n == 0 or (agg.max() == num - 1 and np.unique(agg).size == num)
    for i in range(n):                                              # every node within 2 of its own root
        assert roots[agg[i]] in within2(adj, i), (name, i)
        if not adj[i]:
            assert root[i] and np.count_nonzero(agg == agg[i]) == 1  # a node without neighbours: a root and a singleton
    for a, s in enumerate(roots):                                   # connected: everything is reached from the root inside the aggregate
        members = set(np.flatnonzero(agg == a).tolist())
        seen, todo = {s}, [s]
        while todo:
            for j in adj[todo.pop()]:
                if j in members and j not in seen:
                    seen.add(j)
                    todo.append(j)
        assert seen == members, (name, a)


def test_the_inputs_cover_what_they_are_named_for():
    assert pattern("empty")[0] == 0 and pattern("one")[0] == 1
    assert pattern("diag7")[0] % 8 == 7 and all(not a for a in neighbours("diag7"))
    assert pattern("path203")[0] % 8 == 3
    n, r, c = pattern("path203")
    assert np.any((r // 8 != c // 8) & (r != c))                                    # neighbours across tile borders
    n, r, c = pattern("lowerpath")
    assert np.all(r > c) and neighbours("lowerpath") == neighbours("path203")
    assert pattern("grid13x11")[0] == 143
    assert all(len(a) == 23 for a in neighbours("dense24"))
    n, r, c = pattern("star530")
    assert np.unique(c[r < 8] // 8).size == 67 and len(neighbours("star530")[0]) == 529
    n, r, c = pattern("intile")
    off = r != c
    assert np.count_nonzero(off & (r // 8 != c // 8)) == 1 and neighbours("intile")[38] == [6]
    assert not np.any(np.isin(r[off] * n + c[off], c[off] * n + r[off]))             # one-sided: each link is in one direction only
    assert np.all(values("zeros", 0)[pattern("zeros")[1] != pattern("zeros")[2]] == 0.0)
    n, r, c = pattern("rand1000")
    assert n == 1000 and not np.array_equal(np.unique(r * n + c), np.unique(c * n + r))
    for seed in SEEDS:
        assert reference("dense24", seed)[1] == 1                                   # one aggregate
        assert reference("diag7", seed)[1] == 7 and reference("diag7", seed)[2] == 1
        assert np.array_equal(reference("lowerpath", seed)[0], reference("path203", seed)[0])
        assert np.array_equal(reference("zeros", seed)[0], reference("grid13x11", seed)[0])
        assert reference("rand1000", seed)[2] > 2                                   # several rounds, lagging eliminations among them


# ---------------------------------------------------------------------------------------------------------
# the entry points
# ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_interface_verbatim(bmsp):
    hdr = _flat(open(os.path.join(REPO, "include", "bmsp.h")).read())
    for line in ("typedef struct { char kernel[64]; int64_t nodes, aggregates, rounds, launches, view_bytes; } bmsp_aggregate_info;",
                 "int bmsp_matrix_aggregate(bmsp_matrix_t S, uint64_t seed, uint32_t *d_agg /* n entries, device */, "
                 "int64_t *num_aggregates /* host */, void *stream, bmsp_aggregate_info *info /* may be NULL */);",
                 "int bmsp_matrix_from_aggregates(int num_rows, int num_aggregates, const uint32_t *d_agg, "
                 "const void *d_weights /* NULL = ones */, bmsp_dtype dtype, int transposed, void *stream, bmsp_matrix_t *out);"):
        assert _flat(line) in hdr, line
    for name in ("bmsp_matrix_aggregate", "bmsp_matrix_from_aggregates"):
        assert name in bmsp.SYMBOLS and hasattr(bmsp.lib(), name)


def test_info_layout_and_wrappers(bmsp):
    I = bmsp.AggregateInfo
    assert [f[0] for f in I._fields_] == ["kernel", "nodes", "aggregates", "rounds", "launches", "view_bytes"]
    assert C.sizeof(I) == 64 + 5 * 8 and I.nodes.offset == 64 and I.view_bytes.offset == 96
    assert set(I().as_dict()) == {f[0] for f in I._fields_}
    assert list(inspect.signature(bmsp.aggregate).parameters) == ["S", "seed", "stream"]
    assert list(inspect.signature(bmsp.from_aggregates).parameters) == ["agg", "num_aggregates", "weights", "num_rows", "dtype",
                                                                       "transposed", "stream"]
    for name in ("aggregate", "from_aggregates"):
        assert callable(getattr(bmsp.BmSpMatrix, name))
    src = open(os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "pybmsp", "amg.py")).read()
    for name in ("strength", "tentative", "smooth", "galerkin", "build_hierarchy", "vcycle", "pcg"):
        assert "\ndef %s(" % name in src, name


def test_scalars_and_null_pointers_are_refused_and_named(bmsp):
    L = bmsp.lib()
    buf = (C.c_uint32 * 16)()
    x = C.addressof(buf)
    count = C.c_int64(-5)
    info = bmsp.AggregateInfo()
    assert L.bmsp_matrix_aggregate(None, 0, x, C.byref(count), None, C.byref(info)) == BMSP_ERR_INVALID and "matrix S" in _msg(bmsp)
    assert L.bmsp_matrix_aggregate(None, 0, None, None, None, None) == BMSP_ERR_INVALID and "matrix S" in _msg(bmsp)
    assert count.value == -5
    out = C.c_void_p()
    F = L.bmsp_matrix_from_aggregates
    for args, word in (((-1, 4, x, None, 0, 0), "num_rows"), ((8, -1, x, None, 0, 0), "num_aggregates"), ((8, 4, None, None, 0, 0), "d_agg"),
                       ((8, 4, x, None, 7, 0), "dtype"), ((8, 4, x, None, -1, 0), "dtype"), ((8, 4, x, None, 0, 2), "transposed"),
                       ((8, 4, x, None, 2, -1), "transposed")):
        assert F(*args, None, C.byref(out)) == BMSP_ERR_INVALID, args
        assert word in _msg(bmsp) and out.value is None, (args, _msg(bmsp))
    assert F(8, 4, x, None, 0, 0, None, None) == BMSP_ERR_INVALID and "out" in _msg(bmsp)
    assert F(0, 4, None, None, 0, 0, None, None) == BMSP_ERR_INVALID and "out" in _msg(bmsp)


def build_cpp_aggregate_check(out_path):
    lib_dir = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp_aggregate_check.cpp"), "-o", out_path, "-L" + lib_dir, "-lbmsp",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_aggregate_wrappers_compile_and_link(bmsp, tmp_path):
    """include/bmSpMatrix.h with bmSparse_aggregate and bmSpMatrix<T>::from_aggregates instantiated for float, half and double links
    against libbmsp.so with a plain host compiler."""
    build_cpp_aggregate_check(str(tmp_path / "cpp_aggregate_check"))
