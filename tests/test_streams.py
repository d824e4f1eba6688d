"""Every stream-taking operator on a gated, non-blocking stream (tests/stream_gate.py).

run_gated(case) builds the operands of one call on the null stream with every INPUT buffer holding an alternative input, computes
`expected` by the same operator on the null stream from separate buffers that hold the real input, poisons the outputs, closes a
timed gate on a non-blocking stream s, enqueues on s the device copies that replace the alternative input with the real one, makes
the call on s and compares every output with `expected` bit for bit.  A pass launched on another stream, a memset or a
synchronisation on the null stream where s was meant, or a host read of a device value before its producer ran, reads the
alternative input (or writes before the gate opens) and gives other bits.  On the blocking streams of the older
test_non_default_stream tests all of these are ordered by the runtime and stay invisible.

HARD RULE: the alternative input is WELL-FORMED.  A mis-ordered read must give a wrong answer, never an out-of-range access: indices
stay inside the shape, CSR offsets run from 0 to nnz without decreasing, counts and shapes equal the real input's, values are finite.
No case may gate an input whose early read could index outside an allocation (structure arrays of a matrix handle, segment starts of
the segmented sort and the like are never gated).

Values are small positive integers: real values 1..3 (vectors 1..4), the alternative is the real input plus one.  Every sum is exact in
any order, so bit equality holds for the kernels whose LDS float adds have no fixed order and for fp16 on the matrix cores; and, all
values being positive, every output element with a stored entry behind it differs between the real and the alternative input
(test_input_pairs_are_exact_and_discriminate proves both on the CPU, in float64, for every structure and operator used below).

Which calls are asynchronous, from include/bmsp.h (the sentence of the header each row comes from):

  call                                  contract   header sentence
  bmsp_spmv, plan cached                ASYNC      "Asynchronous on `stream` once the cached sweep plan of A exists"
  bmsp_spmv, after bmsp_matrix_prepare  ASYNC      the same sentence: prepare builds the plan and every cache the default launch reads
  bmsp_spmv, first call                 SYNC       "the call that builds the plan, the position cache or the chunk cache ... synchronises"
  bmsp_spmv, first call, variants 1, 2  ASYNC      the same sentence: the block-row kernels need none of the three
  bmsp_spmm, first call                 SYNC       "the first product of a handle builds bmsp_spmv's plan and synchronises as that call does"
  bmsp_spmm, short block-rows           ASYNC      "After that the call is asynchronous on `stream` unless A has block-rows long enough ..."
  bmsp_spmm, long block-rows            SYNC       "... the call synchronises `stream` before they go back to the pool"
  bmsp_spmv_op, view cached             ASYNC      "Asynchronous on `stream`, except for the one-time build of the view (it synchronises)"
  bmsp_spmv_op, first call              SYNC       the same sentence
  bmsp_spgemm, _symbolic, _numeric      SYNC       "Runs on `stream`; synchronous with respect to the host on return ... The same holds for"
  bmsp_spgemm_sharded_ex                SYNC       the same sentence ("and the sharded products below")
  bmsp_spmv_sharded                     SYNC       "Runs on `stream` and synchronises it before it returns (the exchange; ...)"
  bmsp_matrix_from_coo_device / _csr    SYNC       "Runs on `stream` and synchronises it before it returns (the tile count is read back, ...)"
  bmsp_matrix_to_coo_device / _csr      SYNC       "Both run on `stream` and synchronise it before they return"
  bmsp_matrix_compare_device            SYNC       "runs on `stream` and synchronises it before it returns (the two results are host values)"
  bmsp_matrix_prepare                   SYNC       "Runs on `stream` and synchronises it whenever it builds something"
  bmsp_segsort_u64                      SYNC       "Runs on `stream` and synchronises it before it returns"
  bmsp_matrix_transpose / _convert      SYNC       "Work runs on `stream`; the calls synchronise it before they return"
  bmsp_matrix_copy_values               ASYNC      "asynchronous on `stream` unless out holds such caches"
  bmsp_matrix_add                       SYNC       "runs on `stream` and synchronises it before it returns"
  bmsp_matrix_add_values                ASYNC      "asynchronous on `stream` unless C holds such caches"
  bmsp_matrix_prune                     SYNC       "runs on `stream` and synchronises it before it returns"
  bmsp_matrix_row_absmax                ASYNC      "asynchronous on `stream`"
  bmsp_matrix_diagonal / _from_diagonal ASYNC      "Asynchronous on `stream`"
  bmsp_matrix_scale / _scale_values     ASYNC      "Asynchronous on `stream`"
  bmsp_sddmm / _sddmm_values            ASYNC      "Asynchronous on `stream`: nothing is read back"

ASYNC: the call must return while the gate is still closed and every output must still hold its bytes from before the call; the
same operator then runs to completion on the null stream on a second set of handles of the same sizes (the pool-reuse interference),
eight blocks of the pool's smallest size class are drawn and filled (canaries: a write that the pending call enqueued on a temporary
it has already released lands in one of them), and only then the gate opens.  SYNC: the call must return only after the gate has
opened by its timeout -- everything it enqueued before it blocked was behind the gate.  A case that can show neither fails as
inconclusive; it never passes."""
import functools
import numpy as np
import pytest

import stream_gate as sg
import util
from util import SPMV_LAUNCHES

NPDT = {0: np.float32, 1: np.float16, 2: np.float64}
OUTDT = {0: np.float32, 1: np.float32, 2: np.float64}
DT = {0: "f32", 1: "f16", 2: "f64"}
ASYNC, SYNC = "async", "sync"
OBSERVED = {}


class OrderingError(AssertionError):
    """an output of the gated call differs from the null-stream result of the real input"""


# ---------------------------------------------------------------------------------------------------------
# 0. inputs: structures, values, and the CPU proof that they are exact and discriminate
# ---------------------------------------------------------------------------------------------------------
def _uniq(nr, nc, r, c):
    key = np.unique(np.asarray(r, np.int64) * nc + np.asarray(c, np.int64))
    return int(nr), int(nc), (key // nc).astype(np.int32), (key % nc).astype(np.int32)


@functools.lru_cache(maxsize=None)
def structure(name):
    """(nr, nc, r, c), sorted by (row, col), duplicates removed"""
    from pybmsp import gen
    if name in ("sparse", "dense"):           # the gap matrices of the SpMV launch table
        from test_spgemm_special_values import _gap_matrix
        nr, nc, r, c = _gap_matrix(name)[:4]
    elif name == "hub":                       # 24 x 60011, ~7500 tiles per block-row: carry slots and arrival counters
        from test_fold_history import long_row
        nr, nc, r, c = long_row()[:4]
    elif name == "folds":                     # every head / tail / fold case of the chunked sweep
        from test_spmv_chunk_folds import LAYOUT, layout
        cells = np.unique(layout(LAYOUT, 11), axis=0)
        nr, nc, r, c = 256, 4096 * 8, cells[:, 0], cells[:, 1]
    elif name == "spmm_long":                 # block-rows of 7500 and 257 tiles: SpMM carry buffers from the pool
        from test_spmm import _long_rows
        nr, nc, r, c = _long_rows()
    elif name == "rmat10":
        nr, nc, r, c = gen.rmat(10, 8)[:4]
    elif name == "rmat11":                    # hub block-rows: the column-window passes
        nr, nc, r, c = gen.rmat(11, 8)[:4]
    elif name == "banded":
        nr, nc, r, c = gen.banded(1003, 12)[:4]
    elif name == "rect":
        nr, nc, r, c = gen.random_coo(203, 331, 3000, seed=6)[:4]
    elif name in ("banded64", "fem"):
        from test_gpu_parity import _strip_case
        nr, nc, r, c = _strip_case(gen, None, name)[0][:4]
    else:
        raise ValueError(name)
    return _uniq(nr, nc, r, c)


def mvals(S, alt, salt=0):
    """matrix values 1..3 by position; the alternative is one more"""
    r, c = S[2].astype(np.int64), S[3].astype(np.int64)
    return (1 + (3 * r + 7 * c + salt) % 3 + (1 if alt else 0)).astype(np.float64)


def vec(n, alt, salt=0, width=None):
    """vector entries 1..4 by index; the alternative is one more"""
    x = 1 + (np.arange(n) + salt) % 4
    if width:
        x = 1 + (np.arange(n)[:, None] + 2 * np.arange(width)[None, :] + salt) % 4
    return (x + (1 if alt else 0)).astype(np.float64)


def mirrored(S):
    """the well-formed alternative of a COO / CSR STRUCTURE input: every coordinate mirrored inside the shape, sorted again"""
    nr, nc, r, c = S
    return _uniq(nr, nc, nr - 1 - r, nc - 1 - c)


USES = set()    # (structure, operator): what the GPU cases below run; the CPU test proves its claims for each


def use(struct, op):
    USES.add((struct, op))
    return struct


def _csr(S, v):
    return util.scipy_csr(S[0], S[1], S[2], S[3], v)


def host_results(struct, op):
    """(real result, alternative result, magnitude of the real sum, storage bits of the widest rounding) as dense float64 arrays over
    the output elements that have a stored entry behind them"""
    S = structure(struct)
    nr, nc = S[:2]
    Ar, Aa, P = _csr(S, mvals(S, 0)), _csr(S, mvals(S, 1)), _csr(S, np.ones(S[2].size))
    rows = np.asarray(P.sum(axis=1)).ravel() > 0
    cols = np.asarray(P.sum(axis=0)).ravel() > 0
    if op == "spmv_x":
        return (Ar @ vec(nc, 0))[rows], (Ar @ vec(nc, 1))[rows], (Ar @ vec(nc, 0))[rows], 24
    if op == "spmv_vals":
        return (Ar @ vec(nc, 0))[rows], (Aa @ vec(nc, 0))[rows], (Ar @ vec(nc, 0))[rows], 24
    if op == "spmm_x":
        X0, X1 = vec(nc, 0, width=33), vec(nc, 1, width=33)
        return (Ar @ X0)[rows], (Ar @ X1)[rows], (Ar @ X0)[rows], 24
    if op in ("spmv_op_N", "spmv_op_T"):     # u = 2 * op(A) v - u, v and u gated
        M, n_in, n_out, m = (Ar, nc, nr, rows) if op == "spmv_op_N" else (Ar.T, nr, nc, cols)
        f = lambda alt: 2 * (M @ vec(n_in, alt)) - vec(n_out, alt, 1)
        return f(0)[m], f(1)[m], (2 * (M @ vec(n_in, 0)) + vec(n_out, 0, 1))[m], 24
    if op == "spgemm":                       # A x B, B the same structure with other values (A must be square) -- both gated
        Br, Ba = _csr(S, mvals(S, 0, 1)), _csr(S, mvals(S, 1, 1))
        pat = (P @ P).tocoo()
        Cr, Ca = (Ar @ Br).tocsr(), (Aa @ Ba).tocsr()
        g = lambda M: np.asarray(M[pat.row, pat.col]).ravel()
        return g(Cr), g(Ca), g(Cr), 24      # (fp16 under V15 rounds every PRODUCT to fp16: products <= 16, exact; sums are fp32)
    if op == "values":                       # operators that move or combine stored values one by one: the worst is sddmm / scale / add
        a0, a1 = mvals(S, 0), mvals(S, 1)
        k = 8
        X0, X1, Y = vec(nr, 0, width=k), vec(nr, 1, width=k), vec(nc, 0, 3, width=k)
        d0 = np.einsum("ij,ij->i", X0[S[2]], Y[S[3]])
        d1 = np.einsum("ij,ij->i", X1[S[2]], Y[S[3]])
        l0, l1, rr = vec(nr, 0, 1), vec(nr, 1, 1), vec(nc, 0, 2)
        real = np.concatenate([a0, d0 + a0, l0[S[2]] * a0 * rr[S[3]], 2 * a0 + 3 * mvals(S, 0, 1)])
        alt = np.concatenate([a1, d1 + a1, l1[S[2]] * a1 * rr[S[3]], 2 * a1 + 3 * mvals(S, 1, 1)])
        return real, alt, real, 11
    raise ValueError(op)


def test_input_pairs_are_exact_and_discriminate():
    """CPU, float64: for every (structure, operator) the GPU cases use, the real result is exactly representable with every partial sum
    (positive integers whose total stays below 2^24, below 2^11 where a result or a product is stored as fp16), and the real and the
    alternative result differ in EVERY output element that has a stored entry behind it -- a stale read of any part is visible."""
    assert USES
    for struct, op in sorted(USES):
        real, alt, mag, bits = host_results(struct, op)
        assert real.size and np.all(real == np.round(real)) and np.all(alt == np.round(alt)), (struct, op)
        assert np.max(np.abs(mag)) < 2.0 ** bits and np.max(np.abs(alt)) < 2.0 ** 24, (struct, op, float(np.max(np.abs(mag))))
        same = np.flatnonzero(real == alt)
        assert same.size == 0, (struct, op, same[:4])
    for struct in sorted({s for s, _ in USES}):     # every stored value 1..4: exact in fp16, fp32 and fp64
        S = structure(struct)
        for alt in (0, 1):
            v = mvals(S, alt)
            assert v.min() >= 1 and v.max() <= 4 and np.all(v.astype(np.float16).astype(np.float64) == v)
    for S in (structure("rect"), structure("rmat10")):   # the mirrored COO / CSR input is well-formed and another structure
        M = mirrored(S)
        assert M[2].size == S[2].size and M[2].min() >= 0 and M[2].max() < S[0] and M[3].min() >= 0 and M[3].max() < S[1]
        assert not (np.array_equal(M[2], S[2]) and np.array_equal(M[3], S[3]))
        ro = np.searchsorted(M[2], np.arange(S[0] + 1))
        assert ro[0] == 0 and ro[-1] == M[2].size and np.all(np.diff(ro) >= 0)


# ---------------------------------------------------------------------------------------------------------
# 1. the harness
# ---------------------------------------------------------------------------------------------------------
class Ops:
    """one operand set of a call: inputs = the gated device buffers, outputs = the device buffers the call writes"""

    def __init__(self, inputs, outputs=(), **kw):
        self.inputs, self.outputs = list(inputs), list(outputs)
        self.__dict__.update(kw)


class Case:
    """make(bmsp, alt) -> Ops; prepare(bmsp, ops): host-side preparation that may synchronise (before the gate closes);
    call(bmsp, ops, stream) -> result; read(bmsp, ops, result) -> list of host arrays (after the stream is synchronised; asserts the
    path); late(bmsp, ops, result) -> device buffers the call allocated itself, poisoned while the gate is still closed"""

    def __init__(self, name, sync, make, call, read, prepare=None, late=None, env=None):
        self.name, self.sync, self.make, self.call, self.read = name, sync, make, call, read
        self.prepare = prepare or (lambda bmsp, ops: None)
        self.late = late or (lambda bmsp, ops, res: [])
        self.env = env or {}

    def __repr__(self):
        return self.name


def nbytes(d):
    return d.n * d.dtype.itemsize


def dev(bmsp, a, dtype=None):
    return bmsp.DeviceArray.from_host(np.ascontiguousarray(a, dtype=dtype))


def clone(bmsp, d):
    e = bmsp.DeviceArray(d.n, d.dtype)
    if nbytes(d):
        bmsp.check(bmsp.lib().bmsp_memcpy_d2d(e.ptr, d.ptr, nbytes(d)))
    return e


def mat(bmsp, S, alt, dtype, lay=False, salt=0):
    return bmsp.BmSpMatrix.from_coo(S[0], S[1], S[2], S[3], mvals(S, alt, salt), transposed=lay, dtype=dtype)


def vals_of(M):
    return M.device_arrays()[3]


def u8(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def compare(expected, got, what):
    assert len(expected) == len(got), (what, len(expected), len(got))
    for i, (e, g) in enumerate(zip(expected, got)):
        e, g = np.asarray(e), np.asarray(g)
        if e.shape != g.shape or e.dtype != g.dtype or not np.array_equal(u8(e), u8(g)):
            n = int(np.count_nonzero(u8(e) != u8(g))) if e.shape == g.shape and e.dtype == g.dtype else -1
            raise OrderingError("%s: output %d differs from the null-stream result of the real input in %d of %d elements" %
                                (what, i, n, e.size))


def run_gated(bmsp, monkeypatch, case, misorder=False, interference=None):
    """the steps of the file's docstring; misorder: the call itself goes to the null stream (the caller-level mistake the harness must
    flag); interference: another case whose real call runs on the null stream while the gate is closed and must stay right too."""
    H = sg._hip()
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    # 1, 2: the reference on the null stream, from buffers of its own; copies of the real input for the gated copies
    ref = case.make(bmsp, 0)
    srcs = [clone(bmsp, d) for d in ref.inputs]
    case.prepare(bmsp, ref)
    expected = case.read(bmsp, ref, case.call(bmsp, ref, None))
    bmsp.synchronize()
    ops = case.make(bmsp, 1)
    assert len(ops.inputs) == len(srcs) and ops.inputs
    for s_, d in zip(srcs, ops.inputs):
        assert (d.n, d.dtype) == (s_.n, s_.dtype) and not np.array_equal(u8(d.to_host()), u8(s_.to_host())), "alternative input equals the real one"
    second = case.make(bmsp, 1) if case.sync == ASYNC and not misorder else None
    other = other_ref = other_expected = None
    if interference is not None:
        other_ref = interference.make(bmsp, 0)
        interference.prepare(bmsp, other_ref)
        other_expected = interference.read(bmsp, other_ref, interference.call(bmsp, other_ref, None))
        other = interference.make(bmsp, 0)
        interference.prepare(bmsp, other)
    # 3, 4: preparation that may synchronise, then the poison
    case.prepare(bmsp, ops)
    if second is not None:
        case.prepare(bmsp, second)
    bmsp.synchronize()
    in_ptrs = {d.ptr for d in ops.inputs}
    for d in ops.outputs:
        if d.ptr not in in_ptrs and nbytes(d):
            bmsp.check(bmsp.lib().bmsp_memset(d.ptr, 0xFF, nbytes(d)))
    before = [u8(d.to_host()).copy() for d in ops.outputs]
    bmsp.synchronize()
    s, side, gate = sg.new_stream(), sg.Side(), sg.Gate()
    canaries = []
    try:
        gate.close(s)                                                       # 5
        for s_, d in zip(srcs, ops.inputs):                                 # 6
            sg.memcpy_d2d_async(d.ptr, s_.ptr, nbytes(d), s)
        res = case.call(bmsp, ops, None if misorder else s.value)           # 7
        closed = gate.is_closed()
        if misorder:
            assert closed, "inconclusive: the gate opened before the mis-ordered call returned"
            gate.open()
        elif closed:                                                        # 8
            assert case.sync != SYNC, "%s is documented as synchronising, but returned while the gate was closed" % case.name
            OBSERVED[case.name] = ASYNC
            for i, (d, b) in enumerate(zip(ops.outputs, before)):
                now = u8(side.read(d.ptr, d.n, d.dtype))
                assert np.array_equal(now, b), "%s: output %d was written while the gate was closed" % (case.name, i)
            for d in case.late(bmsp, ops, res):
                side.fill(d.ptr, 0xFF, nbytes(d))
            if second is not None:
                keep = case.call(bmsp, second, None)
                sg.hip_check(H.hipStreamSynchronize(None), "hipStreamSynchronize(null)")
            if other is not None:
                other_res = interference.call(bmsp, other, None)
                sg.hip_check(H.hipStreamSynchronize(None), "hipStreamSynchronize(null)")
            # canaries: the small pool blocks the pending call has released, drawn again and filled while it is still pending
            canaries = [bmsp.DeviceArray(CANARY_BYTES, np.uint8) for _ in range(CANARIES)]
            for d in canaries:
                side.fill(d.ptr, 0xFF, CANARY_BYTES)
            assert gate.is_closed(), "inconclusive: the gate opened (G = %g s) before the interference had finished" % gate.timeout
            gate.open()
        else:
            assert case.sync != ASYNC, "%s is documented as asynchronous, but returned after the gate had opened" % case.name
            assert gate.opened_by_timeout(), "inconclusive: the call returned after the gate, but the gate was not opened by its timeout"
            OBSERVED[case.name] = SYNC
        sg.stream_sync(s)                                                   # 9
    finally:
        gate.finish()
        sg.destroy_stream(s)
        side.close()
    bmsp.synchronize()
    for d in canaries:
        assert np.all(d.to_host() == 0xFF), "%s wrote to a temporary after it had gone back to the pool" % case.name
    compare(expected, case.read(bmsp, ops, res), case.name)                 # 10
    if other is not None:
        compare(other_expected, interference.read(bmsp, other, other_res), "interference " + interference.name)
    return OBSERVED.get(case.name)


CANARIES, CANARY_BYTES = 8, 64    # eight blocks of the pool's smallest size class (512 bytes)


def ids(cases):
    return [c.name for c in cases]


# ---------------------------------------------------------------------------------------------------------
# 2. the cases
# ---------------------------------------------------------------------------------------------------------
ALL_SPMV = dict(SPMV_LAUNCHES)
ALL_SPMV.update({
    "chunk_storage_order": ("folds", {"BMSP_SPMV_CHUNK": "1", "BMSP_SPMV_CHUNK_SORTED": "0"}, 0, "spmv_chunk_kernel"),
    "chunk_row_sorted": ("folds", {"BMSP_SPMV_CHUNK": "1", "BMSP_SPMV_CHUNK_SORTED": "1"}, 0, "spmv_chunk_kernel"),
    "hub_chunk": ("hub", {"BMSP_SPMV_CHUNK": "1"}, 0, "spmv_chunk_kernel"),
    "hub_vstream_sorted": ("hub", {"BMSP_SPMV_NOCHUNK": "1", "BMSP_SPMV_RED": "1"}, 0, "spmv_vstream_kernel<kCached, kSorted>"),
})


def spmv_case(launch, gated, phase, dtype):
    kind, env, variant, kernel = ALL_SPMV[launch]
    S = structure(use(kind, "spmv_" + gated))
    nr, nc = S[:2]

    def make(bmsp, alt):
        A = mat(bmsp, S, alt and gated == "vals", dtype)
        x = dev(bmsp, vec(nc, alt and gated == "x"), NPDT[dtype])
        y = bmsp.DeviceArray(nr, OUTDT[dtype])
        return Ops([x] if gated == "x" else [vals_of(A)], [y], A=A, x=x, y=y)

    def call(bmsp, o, st):
        bmsp.check(bmsp.lib().bmsp_spmv(o.A.h, o.x.ptr, o.y.ptr, variant, st))

    def prepare(bmsp, o):
        if phase == "steady":
            assert bmsp.spmv_launch_info(o.A, variant)["kernel"].startswith(kernel), bmsp.spmv_launch_info(o.A, variant)
            call(bmsp, o, None)
            if "chunk" in launch:
                assert bmsp.spmv_chunk_layout(o.A) == (1 if env.get("BMSP_SPMV_CHUNK_SORTED") == "0" else 2)
        if phase == "prepared":
            # bmsp_matrix_prepare instead of a first call: it must build all the launcher then reads.  The kernel is pinned on a twin of the
            # same structure -- the query on o.A itself would build whatever prepare had left out -- and on o.A by read(), after the call
            twin = mat(bmsp, S, 0, dtype)
            assert bmsp.spmv_launch_info(twin, variant)["kernel"].startswith(kernel), bmsp.spmv_launch_info(twin, variant)
            o.A.prepare(1)
        if gated == "vals":
            o.A.invalidate(False)

    def read(bmsp, o, res):
        assert bmsp.spmv_launch_info(o.A, variant)["kernel"].startswith(kernel), bmsp.spmv_launch_info(o.A, variant)
        return [o.y.to_host()]

    sync = ASYNC if phase in ("steady", "prepared") or kernel.startswith("spmv_blockrow_kernel") else SYNC
    return Case("spmv-%s-%s-%s-%s" % (launch, gated, phase, DT[dtype]), sync, make, call, read, prepare, env=env)


# (the chunked sweep is an fp32 kernel)
SPMV_CASES = [spmv_case(l, "x", ph, dt) for l in ALL_SPMV for ph in ("first", "steady") for dt in (0, 1, 2) if dt == 0 or "chunk" not in l] + \
             [spmv_case(l, "vals", ph, 0) for l in ALL_SPMV for ph in ("first", "steady")]
# after bmsp_matrix_prepare instead of a first call: every default-variant launch, in every dtype it exists for
SPMV_PREPARED = {dt: [spmv_case(l, "x", "prepared", dt) for l in ALL_SPMV if ALL_SPMV[l][2] == 0 and (dt == 0 or "chunk" not in l)] for dt in (0, 1, 2)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", SPMV_CASES, ids=ids(SPMV_CASES))
def test_spmv(bmsp, monkeypatch, case):
    run_gated(bmsp, monkeypatch, case)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1, 2], ids=[DT[d] for d in (0, 1, 2)])
def test_spmv_on_prepared_handles(bmsp, monkeypatch, dtype):
    """bmsp_matrix_prepare builds exactly what the launcher then reads, on every path: the first bmsp_spmv of a prepared handle is
    asynchronous.  One gated run per launch (the case's name is in every message), each under its own environment."""
    assert SPMV_PREPARED[dtype]
    for case in SPMV_PREPARED[dtype]:
        with monkeypatch.context() as m:
            assert run_gated(bmsp, m, case) == ASYNC, case.name


# name -> (structure, BMSP_SPMM_NO_VSTREAM, k, kernel): the six launch paths as test_spmm.py pins them, on short and on long block-rows
SPMM_PATHS = {
    "spmv_handoff": ("sparse", False, 1, "spmv: "),
    "vstream4": ("sparse", False, 3, "spmm_vstream_kernel<4>"),
    "vstream8": ("sparse", False, 7, "spmm_vstream_kernel<8>"),
    "kernel4": ("sparse", True, 3, "spmm_kernel<4>"),
    "kernel16": ("sparse", True, 13, "spmm_kernel<16>"),
    "wide": ("sparse", True, 21, "spmm_wide_kernel"),
    "kernel16_dense": ("dense", False, 9, "spmm_kernel<16>"),
    "vstream4_long": ("spmm_long", False, 3, "spmm_vstream_kernel<4>"),
    "vstream8_long": ("spmm_long", False, 8, "spmm_vstream_kernel<8>"),
    "kernel16_long": ("spmm_long", True, 13, "spmm_kernel<16>"),
    "wide_long": ("spmm_long", True, 33, "spmm_wide_kernel"),
}


def spmm_case(path, phase, dtype):
    kind, novs, k, kernel = SPMM_PATHS[path]
    S = structure(use(kind, "spmm_x"))
    nr, nc = S[:2]

    def make(bmsp, alt):
        A = mat(bmsp, S, 0, dtype)
        X = dev(bmsp, vec(nc, alt, width=k).ravel(), NPDT[dtype])
        Y = bmsp.DeviceArray(nr * k, OUTDT[dtype])
        return Ops([X], [Y], A=A, X=X, Y=Y)

    def call(bmsp, o, st):
        bmsp.check(bmsp.lib().bmsp_spmm(o.A.h, o.X.ptr, k, o.Y.ptr, k, k, st))

    def pinned(bmsp, o):
        name = bmsp.spmm_launch_info(o.A, k)
        assert name.startswith(kernel) if kernel == "spmv: " else name == kernel, name

    def prepare(bmsp, o):
        if phase == "steady":
            pinned(bmsp, o)
            call(bmsp, o, None)

    def read(bmsp, o, res):
        pinned(bmsp, o)
        return [o.Y.to_host()]

    sync = ASYNC if phase == "steady" and kind != "spmm_long" else SYNC
    return Case("spmm-%s-%s-%s" % (path, phase, DT[dtype]), sync, make, call, read, prepare, env={"BMSP_SPMM_NO_VSTREAM": "1"} if novs else {})


SPMM_CASES = [spmm_case(p, ph, dt) for p in SPMM_PATHS for ph, dt in (("first", 0), ("steady", 0), ("steady", 1), ("steady", 2))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SPMM_CASES, ids=ids(SPMM_CASES))
def test_spmm(bmsp, monkeypatch, case):
    run_gated(bmsp, monkeypatch, case)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["vstream4", "kernel16"])
def test_spmm_without_long_rows_leaves_the_pool_buffers_alone(bmsp, monkeypatch, path):
    """A steady bmsp_spmm on a matrix WITHOUT long block-rows releases its carry and counter buffers when the call returns, without
    synchronising.  While it is still pending behind the gate, a product on a matrix WITH long block-rows draws carry and counter
    buffers from the same pool and runs to completion, and the harness draws the smallest pool blocks again as canaries.  Both results
    must be right and the canaries untouched: neither the short-row kernel nor a memset in front of it writes to the released buffers."""
    assert run_gated(bmsp, monkeypatch, spmm_case(path, "steady", 0), interference=spmm_case(path + "_long", "steady", 0)) == ASYNC


def spmv_op_case(op, lay, phase, slots, struct, split, dtype=0):
    S = structure(use(struct, "spmv_op_" + op))
    nr, nc = S[:2]
    n_in, n_out = (nr, nc) if op == "T" else (nc, nr)
    env = {"BMSP_SPMV_OP_SLOTS": slots}
    if split:
        env["BMSP_SPMV_OP_SPLIT"] = "4"

    def make(bmsp, alt):
        A = mat(bmsp, S, 0, dtype, lay=lay)
        v = dev(bmsp, vec(n_in, alt), NPDT[dtype])
        u0 = dev(bmsp, vec(n_out, alt, 1), OUTDT[dtype])
        u = clone(bmsp, u0)
        return Ops([v, u], [u], A=A, v=v, u0=u0)

    def call(bmsp, o, st):
        bmsp.spmv_op(o.A, o.v, op, 2.0, -1.0, o.inputs[1], stream=st)

    def pinned(bmsp, o):
        info = bmsp.spmv_op_launch_info(o.A, op)
        assert info["kernel"].startswith("spmv_op_sweep_kernel<") and info["slots"] == int(slots), info
        assert (info["split_blocks"] > 0) == bool(split), info

    def prepare(bmsp, o):
        if phase == "steady":
            pinned(bmsp, o)
            call(bmsp, o, None)     # (u is input and output: the warm call consumed it)
            bmsp.synchronize()
            bmsp.check(bmsp.lib().bmsp_memcpy_d2d(o.inputs[1].ptr, o.u0.ptr, nbytes(o.u0)))

    def read(bmsp, o, res):
        pinned(bmsp, o)
        return [o.inputs[1].to_host()]

    return Case("spmv_op-%s-%s-%s-slots%s-%s%s" % (op, "colmajor" if lay else "rowmajor", phase, slots, struct, "-split" if split else ""),
                ASYNC if phase == "steady" else SYNC, make, call, read, prepare, env=env)


SPMV_OP_CASES = [spmv_op_case(op, lay, ph, sl, st, sp) for op, lay in (("N", 1), ("T", 0), ("T", 1)) for ph in ("first", "steady")
                 for sl, st, sp in (("8", "rect", False), ("1", "rmat10", True), ("8", "rmat10", True))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SPMV_OP_CASES, ids=ids(SPMV_OP_CASES))
def test_spmv_op(bmsp, monkeypatch, case):
    run_gated(bmsp, monkeypatch, case)


# ---- SpGEMM ---------------------------------------------------------------------------------------------
STAT_KEYS = ("task_list_size", "bmp_reduction", "surviving_tasks", "c_blocks", "c_nnz", "sort_path", "mac_kernel", "mac_variant")


def _sparse_tiles(S):
    blocks = np.unique((S[2].astype(np.int64) // 8) * (1 << 32) + S[3] // 8).size
    return S[2].size <= 16 * blocks


def spgemm_operands(bmsp, S, alt, dtype):
    A = mat(bmsp, S, alt, dtype)
    B = mat(bmsp, S, alt, dtype, lay=True, salt=1)
    return A, B


def matrix_out(M):
    return list(M.host_arrays()) + [np.array([v for _, v in sorted(M.info().items())], np.int64)]


def stats_out(st):
    return np.array([st[k] for k in STAT_KEYS], np.int64)


def spgemm_case(path, struct, dtype, tc, what="spgemm", extra_env=None):
    """path: a key of test_spgemm_special_values.PATHS, forced and asserted as that file's neighbours force and assert it"""
    from test_spgemm_special_values import PATHS, _expected_twin
    S = structure(use(struct, "spgemm"))
    env, mode = PATHS[path]
    env = dict(env, **(extra_env or {}))
    sorts, variants = _expected_twin(path, dtype, tc, _sparse_tiles(S), struct == "rmat11", mode)

    def make(bmsp, alt):
        A, B = spgemm_operands(bmsp, S, alt, dtype)
        o = Ops([vals_of(A), vals_of(B)], [], A=A, B=B)
        if what == "numeric":
            o.C, _ = bmsp.spgemm_symbolic(A, B, mode=mode, tc_version=tc)
            o.outputs = [vals_of(o.C)]
        return o

    def prepare(bmsp, o):
        if what == "spgemm":
            bmsp.spgemm(o.A, o.B, mode=mode, tc_version=tc)    # a steady pair: records, hints and caches exist ...
        o.A.invalidate(False)                                  # ... and the value-derived ones are rebuilt inside the gated call
        o.B.invalidate(False)

    def call(bmsp, o, st):
        if what == "spgemm":
            return bmsp.spgemm(o.A, o.B, mode=mode, tc_version=tc, stream=st)
        if what == "symbolic":
            return bmsp.spgemm_symbolic(o.A, o.B, mode=mode, tc_version=tc, stream=st)
        return o.C, bmsp.spgemm_numeric(o.A, o.B, o.C, tc_version=tc, stream=st)

    def read(bmsp, o, res):
        Cm, st = res
        if what != "numeric":
            assert sorts is None or st["sort_path"] in sorts, st
        if what == "spgemm":
            assert variants is None or st["mac_variant"] in variants, st
            assert extra_env or st["mac_kernel"] == (tc if dtype == 1 and tc != 5 else 5), st
        return matrix_out(Cm) + ([stats_out(st)] if what == "spgemm" else [])

    return Case("%s-%s-%s-%s-tc%d" % (what, path, struct, DT[dtype], tc), SYNC, make, call, read, prepare, env=env)


SPGEMM_CASES = [spgemm_case(p, s, 0, 5) for p, s in (("default", "banded64"), ("pipe_seg_gather", "banded64"), ("pipe_glob_dense", "banded64"),
                                                      ("pipe_seg_gather", "fem"), ("strip", "banded64"), ("rowmerge", "banded64"),
                                                      ("rowmerge", "fem"), ("rowsparse", "fem"), ("f32mfma", "banded64"),
                                                      ("tasklist", "banded64"), ("tasklist", "fem"))] + \
               [spgemm_case(p, s, 1, 4) for p, s in (("default", "banded64"), ("pipe_seg_b_compact", "banded64"), ("pipe_glob_b_dense", "banded64"),
                                                      ("pipe_seg_direct", "banded64"), ("strip", "banded64"), ("rowmerge", "fem"),
                                                      ("tasklist", "banded64"))] + \
               [spgemm_case("pipe_glob_dense", "fem", 1, 5), spgemm_case("rowsparse", "fem", 1, 5), spgemm_case("pipe_seg", "fem", 2, 5),
                spgemm_case("rowwindow", "rmat11", 0, 5, extra_env={"BMSP_WIN_CAND": "64"}),
                spgemm_case("rowwindow", "rmat11", 1, 4, extra_env={"BMSP_WIN_CAND": "64"}),
                spgemm_case("default", "rmat10", 0, 5, extra_env={"BMSP_SPGEMM_FORCE_PANELS": "1"}),
                spgemm_case("default", "rmat10", 1, 4, extra_env={"BMSP_SPGEMM_FORCE_PANELS": "1"})] + \
               [spgemm_case(p, s, dt, tc, what=w) for w in ("symbolic", "numeric")
                for p, s, dt, tc in (("strip", "banded64", 0, 5), ("strip", "banded64", 1, 4), ("tasklist", "fem", 0, 5), ("pipe_seg_gather", "fem", 0, 5))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SPGEMM_CASES, ids=ids(SPGEMM_CASES))
def test_spgemm(bmsp, monkeypatch, case):
    run_gated(bmsp, monkeypatch, case)


def sharded_spgemm_case(P, rounds, gather, dtype, tc):
    S = structure(use("banded64", "spgemm"))

    def make(bmsp, alt):
        A, B = spgemm_operands(bmsp, S, alt, dtype)
        return Ops([vals_of(A), vals_of(B)], [], A=A, B=B, comm=bmsp.Comm.loopback(P))

    def prepare(bmsp, o):
        o.A.invalidate(False)
        o.B.invalidate(False)

    def call(bmsp, o, st):
        return bmsp.spgemm_sharded(o.comm, o.A, o.B, tc_version=tc, stream=st, gather=gather, rounds=rounds)

    def read(bmsp, o, res):
        Cm, st, sh = res
        assert sh["world"] == P and sh["gathered"] == int(gather), sh
        return matrix_out(Cm) + [np.array([st[k] for k in STAT_KEYS[:5]], np.int64)]

    return Case("spgemm_sharded-P%d-rounds%d-%s-%s" % (P, rounds, "gather" if gather else "owner_keeps", DT[dtype]), SYNC, make, call, read, prepare)


def sharded_spmv_case(phase):
    S = structure(use("rmat10", "spmv_x"))

    def make(bmsp, alt):
        A = mat(bmsp, S, 0, 0)
        x = dev(bmsp, vec(S[1], alt), np.float32)
        y = bmsp.DeviceArray(S[0], np.float32)
        return Ops([x], [y], A=A, x=x, y=y, comm=bmsp.Comm.loopback(2))

    def call(bmsp, o, st):
        return bmsp.spmv_sharded(o.comm, o.A, o.x, o.y, stream=st)

    def prepare(bmsp, o):
        if phase == "steady":
            call(bmsp, o, None)

    def read(bmsp, o, res):
        assert res[1]["world"] == 2
        return [o.y.to_host()]

    return Case("spmv_sharded-P2-%s" % phase, SYNC, make, call, read, prepare)


SHARDED_CASES = [sharded_spgemm_case(P, rounds, gather, dt, tc) for P in (2, 3) for rounds, gather in ((0, True), (1, True), (0, False))
                 for dt, tc in ((0, 5),)] + [sharded_spgemm_case(3, 0, True, 1, 4), sharded_spmv_case("first"), sharded_spmv_case("steady")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SHARDED_CASES, ids=ids(SHARDED_CASES))
def test_sharded(bmsp, monkeypatch, case):
    run_gated(bmsp, monkeypatch, case)


# ---- builders, conversions, comparison, prepare, segmented sort ---------------------------------------------
def builder_case(form, struct, dtype, lay):
    S0 = structure(use(struct, "values"))

    def make(bmsp, alt):
        S = mirrored(S0) if alt else S0
        r, c, v = dev(bmsp, S[2], np.int32), dev(bmsp, S[3], np.int32), dev(bmsp, mvals(S, alt), np.float64)
        if form == "coo":
            return Ops([r, c, v], [], r=r, c=c, v=v)
        ro = dev(bmsp, np.searchsorted(S[2], np.arange(S[0] + 1)), np.int32)
        return Ops([ro, c, v], [], ro=ro, c=c, v=v)

    def call(bmsp, o, st):
        if form == "coo":
            return bmsp.BmSpMatrix.from_coo_device(S0[0], S0[1], o.r, o.c, o.v, transposed=lay, dtype=dtype, stream=st)
        return bmsp.BmSpMatrix.from_csr_device(S0[0], S0[1], o.ro, o.c, o.v, transposed=lay, dtype=dtype, stream=st)

    return Case("from_%s_device-%s-%s-%s" % (form, struct, DT[dtype], "colmajor" if lay else "rowmajor"), SYNC, make, call,
                lambda bmsp, o, res: matrix_out(res))


def export_case(form, struct, dtype, lay):
    S = structure(use(struct, "values"))

    def make(bmsp, alt):
        A = mat(bmsp, S, alt, dtype, lay=lay)
        n = S[2].size
        first = bmsp.DeviceArray(n if form == "coo" else S[0] + 1, np.int32)
        c, v = bmsp.DeviceArray(n, np.int32), bmsp.DeviceArray(n, np.float64)
        return Ops([vals_of(A)], [first, c, v], A=A)

    def call(bmsp, o, st):
        f = bmsp.lib().bmsp_matrix_to_coo_device if form == "coo" else bmsp.lib().bmsp_matrix_to_csr_device
        bmsp.check(f(o.A.h, o.outputs[0].ptr, o.outputs[1].ptr, o.outputs[2].ptr, st))

    return Case("to_%s_device-%s-%s-%s" % (form, struct, DT[dtype], "colmajor" if lay else "rowmajor"), SYNC, make, call,
                lambda bmsp, o, res: [d.to_host() for d in o.outputs])


def compare_case(struct, dtype):
    S0 = structure(use(struct, "values"))

    def make(bmsp, alt):
        A = mat(bmsp, S0, 0, dtype)
        S = mirrored(S0) if alt else S0
        r, c, v = dev(bmsp, S[2], np.int32), dev(bmsp, S[3], np.int32), dev(bmsp, mvals(S, alt), np.float64)
        return Ops([r, c, v], [], A=A, r=r, c=c, v=v)

    def read(bmsp, o, res):
        return [np.array([res[0]], np.float64), np.array([res[1]], np.int64)]

    def call(bmsp, o, st):
        return o.A.compare_device(o.r, o.c, o.v, stream=st)

    return Case("compare_device-%s-%s" % (struct, DT[dtype]), SYNC, make, call, read)


def prepare_case(what, dtype, tc):
    S = structure(use(use("banded64", "spgemm"), "spmv_vals"))

    def make(bmsp, alt):
        A, B = spgemm_operands(bmsp, S, alt, dtype)
        x = dev(bmsp, vec(S[1], 0), NPDT[dtype])
        return Ops([vals_of(A), vals_of(B)], [], A=A, B=B, x=x)

    def prepare(bmsp, o):
        o.A.invalidate(False)
        o.B.invalidate(False)

    def call(bmsp, o, st):
        o.A.prepare(what, stream=st)
        o.B.prepare(what, stream=st)

    def read(bmsp, o, res):
        """the ungated products that follow the prepared handles"""
        out = [bmsp.spmv(o.A, o.x).to_host()]
        Cm, st = bmsp.spgemm(o.A, o.B, tc_version=tc)
        return out + matrix_out(Cm) + [stats_out(st)]

    return Case("prepare-what%d-%s" % (what, DT[dtype]), SYNC, make, call, read, prepare, env={"BMSP_MAC_STRIP": "1"})


def segsort_case(shape, val_bytes):
    from test_gpu_parity import _segsort_cuts
    n = 200000
    rng = np.random.default_rng(val_bytes)
    cuts = np.unique(_segsort_cuts(shape, rng, n)).astype(np.int64)
    cuts = cuts[cuts < n]

    def make(bmsp, alt):
        g = np.random.default_rng(100 + alt)
        keys = g.integers(0, 1 << 40, n).astype(np.uint64)
        keys[: n // 2] &= np.uint64(0xFF)
        pay = np.stack([np.arange(n, dtype=np.uint64) + np.uint64(alt * n), keys ^ np.uint64(0xABCDEF)], axis=1)
        dk = dev(bmsp, keys)
        if val_bytes == 0:
            dv = None
        elif val_bytes == 4:
            dv = dev(bmsp, pay[:, 0].astype(np.uint32))
        elif val_bytes == 8:
            dv = dev(bmsp, pay[:, 0].copy())
        else:
            dv = dev(bmsp, pay.reshape(-1))
            dv.dtype = np.dtype([("a", np.uint64), ("b", np.uint64)])
            dv.n = n
        bufs = [dk] + ([dv] if dv is not None else [])
        return Ops(bufs, bufs, dk=dk, dv=dv, segs=dev(bmsp, cuts, np.int32))

    def call(bmsp, o, st):
        bmsp.segsort(o.dk, o.dv, o.segs, stream=st)

    return Case("segsort-%s-val%d" % (shape, val_bytes), SYNC, make, call, lambda bmsp, o, res: [d.to_host() for d in o.outputs])


PLUMBING_CASES = [builder_case(f, s, dt, lay) for f in ("coo", "csr") for s, dt, lay in (("rect", 0, False), ("rmat10", 1, True), ("rmat10", 2, False))] + \
                 [export_case(f, s, dt, lay) for f in ("coo", "csr") for s, dt, lay in (("rect", 0, True), ("rmat10", 1, False), ("rmat10", 2, False))] + \
                 [compare_case("rect", 0), compare_case("rmat10", 2)] + \
                 [prepare_case(w, dt, tc) for w in (1, 2, 3) for dt, tc in ((0, 5), (1, 4))] + \
                 [segsort_case(sh, vb) for sh, vb in (("mixed", 16), ("tiny", 8), ("block", 4), ("long", 16), ("long", 0))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PLUMBING_CASES, ids=ids(PLUMBING_CASES))
def test_builders_conversions_prepare_segsort(bmsp, monkeypatch, case):
    run_gated(bmsp, monkeypatch, case)


# ---- the operators the blocking-stream tests of their own files exercise --------------------------------------
def derived_case(name, sync, struct, dtype, env, fresh, update=None, operands=None, lay_in=False, pin=None):
    """fresh(bmsp, o, stream) -> a new handle from o.A (and o's operands); update(bmsp, o, stream): the *_values / copy_values form into
    o.out, a handle made by fresh() at make time.  Gated: A's values and the operand buffers named by `operands`."""
    S = structure(use(struct, "values"))

    def make(bmsp, alt):
        A = mat(bmsp, S, alt, dtype, lay=lay_in)
        o = Ops([vals_of(A)], [], A=A, alt=alt)
        if operands:
            operands(bmsp, o, S, alt, dtype)
        if update:
            o.out = fresh(bmsp, o, None)
            o.outputs = [vals_of(o.out)]
        return o

    def call(bmsp, o, st):
        if update:
            update(bmsp, o, st)
            return o.out
        return fresh(bmsp, o, st)

    def late(bmsp, o, res):
        return [] if update else [vals_of(res)]

    return Case(name + "-" + DT[dtype], sync, make, call, lambda bmsp, o, res: matrix_out(res), pin, late=late, env=env)


def _b_operand(bmsp, o, S, alt, dtype):
    o.B = mat(bmsp, S, alt, dtype, lay=True, salt=1)
    o.inputs.append(vals_of(o.B))


def _scale_operands(bmsp, o, S, alt, dtype):
    o.l, o.r = dev(bmsp, vec(S[0], alt, 1), OUTDT[dtype]), dev(bmsp, vec(S[1], 0, 2), OUTDT[dtype])
    o.inputs.append(o.l)


def _sddmm_operands(bmsp, o, S, alt, dtype):
    o.X, o.Y = dev(bmsp, vec(S[0], alt, width=8).ravel(), NPDT[dtype]), dev(bmsp, vec(S[1], 0, 3, width=8).ravel(), NPDT[dtype])
    o.inputs.append(o.X)


def vector_case(name, struct, dtype, env, n_out, run, operands=None):
    """an operator that writes a vector of n_out(S) entries from A's values"""
    S = structure(use(struct, "values"))

    def make(bmsp, alt):
        A = mat(bmsp, S, alt, dtype)
        return Ops([vals_of(A)], [bmsp.DeviceArray(n_out(S), OUTDT[dtype])], A=A)

    def call(bmsp, o, st):
        bmsp.check(run(bmsp)(o.A.h, o.outputs[0].ptr, st))

    return Case(name + "-" + DT[dtype], ASYNC, make, call, lambda bmsp, o, res: [o.outputs[0].to_host()], env=env)


def from_diagonal_case(dtype, lay):
    n = 1003
    use("banded", "values")

    def make(bmsp, alt):
        d = dev(bmsp, vec(n, alt), OUTDT[dtype])
        return Ops([d], [], d=d)

    def call(bmsp, o, st):
        return bmsp.from_diagonal(o.d, n, n + 5, dtype=dtype, transposed=lay, stream=st)

    return Case("from_diagonal-%s-%s" % (DT[dtype], "colmajor" if lay else "rowmajor"), ASYNC, make, call, lambda bmsp, o, res: matrix_out(res),
                late=lambda bmsp, o, res: [vals_of(res)])


def _sddmm_pin(kernel):
    def pin(bmsp, o):     # (the query reads S's structure back: before the gate closes)
        assert bmsp.sddmm_launch_info(o.A, 8)["kernel"] == kernel, bmsp.sddmm_launch_info(o.A, 8)
    return pin


DERIVED_CASES = []
for lanes in ("1", "8"):
    e = {"BMSP_TRANSPOSE_LANES": lanes}
    DERIVED_CASES += [
        derived_case("transpose-lanes" + lanes, SYNC, "rmat10", 2, e, lambda bmsp, o, st: o.A.transpose(1, stream=st)),
        derived_case("transpose_same_layout-lanes" + lanes, SYNC, "banded", 1, e, lambda bmsp, o, st: o.A.transpose(0, stream=st)),
        derived_case("convert_layout-lanes" + lanes, SYNC, "rmat10", 0, e, lambda bmsp, o, st: o.A.with_layout(1, stream=st)),
        derived_case("copy_values-lanes" + lanes, ASYNC, "rmat10", 0, e, lambda bmsp, o, st: o.A.transpose(1, stream=st),
                     update=lambda bmsp, o, st: o.out.copy_values_from(o.A, stream=st)),
    ]
    e = {"BMSP_ADD_LANES": lanes}
    DERIVED_CASES += [
        derived_case("add-lanes" + lanes, SYNC, "rmat10", 0, e, lambda bmsp, o, st: bmsp.add(o.A, o.B, 2.0, 3.0, stream=st), operands=_b_operand),
        derived_case("add_values-lanes" + lanes, ASYNC, "banded", 1, e, lambda bmsp, o, st: bmsp.add(o.A, o.B, 2.0, 3.0, stream=st),
                     update=lambda bmsp, o, st: bmsp.add_values(o.out, o.A, o.B, 2.0, 3.0, stream=st), operands=_b_operand),
    ]
    e = {"BMSP_PRUNE_LANES": lanes}
    DERIVED_CASES += [
        derived_case("prune-lanes" + lanes, SYNC, "rmat10", 0, e, lambda bmsp, o, st: bmsp.prune(o.A, 2.5, stream=st)[0]),
        derived_case("prune_row_rel-lanes" + lanes, SYNC, "banded", 2, e, lambda bmsp, o, st: bmsp.prune(o.A, 0.5, "row_rel", stream=st)[0]),
        vector_case("row_absmax-lanes" + lanes, "rmat10", 0, e, lambda S: S[0], lambda bmsp: bmsp.lib().bmsp_matrix_row_absmax),
    ]
    e = {"BMSP_SCALE_LANES": lanes}
    DERIVED_CASES += [
        derived_case("scale-lanes" + lanes, ASYNC, "rmat10", 0, e, lambda bmsp, o, st: bmsp.scale(o.A, o.l, o.r, transposed=1, stream=st),
                     operands=_scale_operands),
        derived_case("scale_values-lanes" + lanes, ASYNC, "banded", 1, e, lambda bmsp, o, st: bmsp.scale(o.A, o.l, o.r, stream=st),
                     update=lambda bmsp, o, st: bmsp.scale_values(o.out, o.A, o.l, o.r, stream=st), operands=_scale_operands),
    ]
for kernel, lanes, name in (("value", "1", "sddmm_value_kernel<1>"), ("value", "8", "sddmm_value_kernel<8>"), ("tile", None, "sddmm_tile_kernel")):
    e = {"BMSP_SDDMM_KERNEL": kernel}
    if lanes:
        e["BMSP_SDDMM_LANES"] = lanes
    tag = kernel + (lanes or "")
    DERIVED_CASES += [
        derived_case("sddmm-" + tag, ASYNC, "rmat10", 0, e,
                     lambda bmsp, o, st: bmsp.sddmm(o.A, o.X, o.Y, 8, 1.0, 1.0, stream=st), operands=_sddmm_operands, pin=_sddmm_pin(name)),
        derived_case("sddmm_values-" + tag, ASYNC, "banded", 1 if kernel == "tile" else 0, e,
                     lambda bmsp, o, st: bmsp.sddmm(o.A, o.X, o.Y, 8, 1.0, 1.0, stream=st),
                     update=lambda bmsp, o, st: bmsp.sddmm_values(o.out, o.A, o.X, o.Y, 8, 1.0, 1.0, stream=st),
                     operands=_sddmm_operands, pin=_sddmm_pin(name)),
    ]
DERIVED_CASES += [vector_case("diagonal", "banded", dt, {}, lambda S: min(S[0], S[1]), lambda bmsp: bmsp.lib().bmsp_matrix_diagonal) for dt in (0, 1, 2)]
DERIVED_CASES += [from_diagonal_case(0, False), from_diagonal_case(1, True), from_diagonal_case(2, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", DERIVED_CASES, ids=ids(DERIVED_CASES))
def test_derived_matrix_operators(bmsp, monkeypatch, case):
    run_gated(bmsp, monkeypatch, case)


# ---------------------------------------------------------------------------------------------------------
# 3. self-checks of the gate
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gate_holds_one_stream_only(bmsp):
    """While the gate is closed on s: work on another stream completes (a blocked host function does not stall the runtime), a buffer
    that an async copy on s is about to overwrite still holds its old bytes, and the library's own bmsp_memset + bmsp_memcpy_d2h
    complete with the right bytes (they synchronise the device, so they return once the gate has opened by its timeout).  open() then
    lets the copy through; a gate nobody opens opens by itself after G."""
    n = 4096
    old, new = np.arange(n, dtype=np.float32), -np.arange(n, dtype=np.float32) - 1
    d_old, d_new, d_other = dev(bmsp, old), dev(bmsp, new), bmsp.DeviceArray(n, np.float32)
    bmsp.synchronize()
    s, side, gate = sg.new_stream(), sg.Side(), sg.Gate()
    try:
        gate.close(s)
        sg.memcpy_d2d_async(d_old.ptr, d_new.ptr, 4 * n, s)
        side.fill(d_other.ptr, 0x3C, 4 * n)
        assert np.all(u8(side.read(d_other.ptr, n, np.float32)) == 0x3C)
        sg.hip_check(sg._hip().hipStreamSynchronize(None), "null stream")
        assert np.array_equal(side.read(d_old.ptr, n, np.float32), old)
        assert gate.is_closed(), "work on other streams took longer than G or waited for the gate"
        gate.open()
        sg.stream_sync(s)
        assert not gate.is_closed() and not gate.opened_by_timeout()
        assert np.array_equal(d_old.to_host(), new)
        gate.finish()
        # the library's synchronous plumbing against a gate nobody opens
        gate = sg.Gate()
        gate.close(s)
        sg.memcpy_d2d_async(d_old.ptr, d_other.ptr, 4 * n, s)
        assert gate.is_closed()
        bmsp.check(bmsp.lib().bmsp_memset(d_new.ptr, 0x11, 4 * n))
        assert np.all(u8(d_new.to_host()) == 0x11)
        assert sg.wait_until(lambda: not gate.is_closed(), 20 * sg.G), "the gate did not open by itself"
        assert gate.opened_by_timeout()
        sg.stream_sync(s)
        assert np.all(u8(d_old.to_host()) == 0x3C)
    finally:
        gate.finish()
        sg.destroy_stream(s)
        side.close()


@pytest.mark.gpu
def test_harness_flags_a_caller_level_misordering(bmsp, monkeypatch):
    """The method discriminates on this runtime: the gate closed on s, the copy of the real x enqueued on s, bmsp_spmv called with
    stream = NULL.  The sweep reads the alternative x, and the harness's comparison raises."""
    case = spmv_case("vstream_cached_sorted", "x", "steady", 0)
    with pytest.raises(OrderingError):
        run_gated(bmsp, monkeypatch, case, misorder=True)
    assert run_gated(bmsp, monkeypatch, case) == ASYNC


# ---------------------------------------------------------------------------------------------------------
# 4. two handles, two streams
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("launch", ["hub_chunk", "hub_vstream_sorted"])
def test_two_handles_two_streams_spmv(bmsp, monkeypatch, launch):
    """"different handles may": 16 alternating launches of two hub matrices of equal size (the same pool buckets) on two non-blocking
    streams, no gate; every result bit-equal to the handle's serial result."""
    kind, env, variant, kernel = ALL_SPMV[launch]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    S = structure(use(kind, "spmv_x"))
    As = [mat(bmsp, S, 0, 0), mat(bmsp, S, 0, 0, salt=1)]
    xs = [dev(bmsp, vec(S[1], 0, i), np.float32) for i in range(4)]
    for A in As:
        assert bmsp.spmv_launch_info(A, variant)["kernel"].startswith(kernel)
    serial = [[bmsp.spmv(A, x).to_host() for x in xs] for A in As]
    outs = [[bmsp.DeviceArray(S[0], np.float32) for _ in range(8)] for _ in As]
    for h in outs:
        for y in h:
            bmsp.check(bmsp.lib().bmsp_memset(y.ptr, 0xFF, nbytes(y)))
    bmsp.synchronize()
    streams = [sg.new_stream(), sg.new_stream()]
    try:
        for i in range(16):
            h, j = i % 2, i // 2
            bmsp.check(bmsp.lib().bmsp_spmv(As[h].h, xs[j % 4].ptr, outs[h][j].ptr, variant, streams[h].value))
        for s in streams:
            sg.stream_sync(s)
    finally:
        for s in streams:
            sg.destroy_stream(s)
    for h in range(2):
        for j in range(8):
            compare([serial[h][j % 4]], [outs[h][j].to_host()], "handle %d launch %d" % (h, j))


@pytest.mark.gpu
@pytest.mark.parametrize("path,struct", [("rowmerge", "banded64"), ("pipe_seg_gather", "fem")])
def test_two_handles_two_streams_spgemm(bmsp, monkeypatch, path, struct):
    """4 alternating bmsp_spgemm calls of two pairs of equal size on two non-blocking streams (row-merge strip mode; the pipeline)"""
    from test_spgemm_special_values import PATHS
    env, mode = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    S = structure(use(struct, "spgemm"))
    pairs = [spgemm_operands(bmsp, S, alt, 0) for alt in (0, 1)]
    serial = []
    for A, B in pairs:
        Cm, st = bmsp.spgemm(A, B, mode=mode, tc_version=5)
        assert st["sort_path"] == (2 if path == "rowmerge" else st["sort_path"]) and (path != "rowmerge" or st["sort_long"] == 1), st
        serial.append(matrix_out(Cm) + [stats_out(st)])
    streams = [sg.new_stream(), sg.new_stream()]
    got = []
    try:
        for i in range(4):
            A, B = pairs[i % 2]
            Cm, st = bmsp.spgemm(A, B, mode=mode, tc_version=5, stream=streams[i % 2].value)
            got.append((i % 2, Cm, st))
        for s in streams:
            sg.stream_sync(s)
    finally:
        for s in streams:
            sg.destroy_stream(s)
    for h, Cm, st in got:
        compare(serial[h], matrix_out(Cm) + [stats_out(st)], "pair %d" % h)
