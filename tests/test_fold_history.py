"""Results must not depend on launch history: the carry-slot folds across back-to-back launches with changing inputs.

Six kernels hand partial sums of long / split block-rows between workgroups through carry slots that persist from launch to launch
(the SpMV plan's and the chunk cache's) or come back from the pool (SpMM).  Equal inputs from launch to launch hide a fold that reads a
slot left over from the previous launch, so every case here runs four inputs:
  x0 -- gen.spmv_x(n, "cusp");  x1 -- x0 permuted, sign-flipped, times a power of two (2^12; 2^8 in fp16), so that a stale partial
  from the other input breaks even the tolerance check;  z -- zeros (y must be exactly 0);  x3 -- uniform in [-1, 1).
Three phases per case:
  solo    -- synchronize, one launch into a NaN-poisoned y, read back; against scipy float64 with check_spmv's bound (and the oracle
             for fp32);
  queued  -- 24 poisoned outputs, then a seeded launch sequence in which every input follows every other at least once, with no host
             call between the launches; one synchronize, then every output against its reference -- and, where the kernel's reduction
             order is fixed (chunked sweep, sorted value-stream reduction, sweep kernel, slot-walk SpMM kernels), bitwise equal to the
             solo result of the same input;
  values  -- (chunked sweep, value-stream kernel) new values copied into A's value array, invalidate(), another queued sequence
             against the new reference.
The LDS float adds of the value-stream kernel's atomic reduction and of the SpMM value-stream walk give an order that the hardware
picks, so those cases are held to the bound, which the contrast of x0 and x1 makes tight enough to catch a stale slot."""
import numpy as np
import pytest
import util
from test_spmv_chunk_folds import LAYOUT, layout

pytestmark = pytest.mark.gpu

Z = 2             # index of the zero input
QUEUE = 24        # launches per queued phase
# a circuit through all 12 ordered pairs of the 4 inputs (each input follows each other one once)
CIRCUIT = [0, 1, 2, 3, 0, 2, 1, 3, 2, 0, 3, 1, 0]


def sequence(seed):
    g = np.random.default_rng(seed)
    relabel = g.permutation(4)
    seq = [int(relabel[i]) for i in CIRCUIT] + [int(i) for i in g.integers(0, 4, QUEUE - len(CIRCUIT))]
    pairs = {(a, b) for a, b in zip(seq, seq[1:]) if a != b}
    assert len(pairs) == 12 and Z in seq
    return seq


def inputs(n, np_in, seed):
    from pybmsp import gen
    g = np.random.default_rng(seed)
    x0 = gen.spmv_x(n, "cusp").astype(np.float64)
    x1 = -x0[g.permutation(n)] * (2.0 ** 8 if np_in == np.float16 else 2.0 ** 12)
    x3 = g.uniform(-1.0, 1.0, n)
    return [x.astype(np_in) for x in (x0, x1, np.zeros(n), x3)]


def long_block_rows(A):
    return int(np.count_nonzero(np.diff(A.block_row_ptr().astype(np.int64)) > 256))


class Case:
    """one matrix and its four inputs; kind: "spmv", "spmm" (k vectors, row-major) or "sharded" (comm)"""

    def __init__(self, bmsp, oracle, nr, nc, r, c, v, dtype=0, seed=0, kind="spmv", k=1, comm=None):
        self.bmsp, self.lib = bmsp, bmsp.lib()
        self.nr, self.nc, self.r, self.c, self.dtype = nr, nc, np.asarray(r), np.asarray(c), dtype
        self.kind, self.k, self.comm = kind, k, comm
        self.np_in, self.np_out = bmsp.NP_DTYPE[dtype], bmsp.OUT_DTYPE[dtype]
        self.tol = 1e-13 if dtype == 2 else 1e-5
        self.A = bmsp.BmSpMatrix.from_coo(nr, nc, r, c, v, dtype=dtype)
        self.xs = inputs(nc * k, self.np_in, seed)
        self.dx = [bmsp.DeviceArray.from_host(x) for x in self.xs]
        self.set_values(v)
        self.oracle_y = None
        if dtype == 0 and kind == "spmv":
            om = oracle.bmsp_from_coo(oracle.Coo(nr, nc, self.r, self.c, np.asarray(v, np.float64)), 0, False)
            self.oracle_y = [oracle.spmv_f32(om, x) for x in self.xs]

    def set_values(self, v):
        self.v = np.asarray(v, np.float64)
        S = util.scipy_csr(self.nr, self.nc, self.r, self.c, self.v.astype(self.np_in).astype(np.float64))
        X = [x.astype(np.float64).reshape(self.nc, self.k) for x in self.xs]
        self.want = [(S @ x).reshape(-1) for x in X]
        self.mag = [(abs(S) @ np.abs(x)).reshape(-1) for x in X]

    def output(self):
        n = self.nr * self.k
        y = self.bmsp.DeviceArray(n, self.np_out)
        assert self.lib.bmsp_memset(y.ptr, 0xFF, n * y.dtype.itemsize) == 0  # NaN poison: every row must be written
        return y

    def launch(self, i, y):
        if self.kind == "spmv":
            self.bmsp.check(self.lib.bmsp_spmv(self.A.h, self.dx[i].ptr, y.ptr, 0, None))
        elif self.kind == "spmm":
            self.bmsp.check(self.lib.bmsp_spmm(self.A.h, self.dx[i].ptr, self.k, y.ptr, self.k, self.k, None))
        else:
            self.bmsp.spmv_sharded(self.comm, self.A, self.dx[i], y)

    def check(self, i, y, what):
        assert np.all(np.isfinite(y)), (what, i, int(np.count_nonzero(~np.isfinite(y))))
        if i == Z:
            assert np.all(y == 0), (what, int(np.count_nonzero(y)))
        err = np.abs(y.astype(np.float64) - self.want[i])
        lim = 2 * (self.tol * self.mag[i] + 1e-30) + self.tol * np.abs(self.want[i])
        bad = err > lim
        assert not np.any(bad), (what, "input", i, "rows off", int(bad.sum()), "first", int(np.argmax(bad)), float(np.max(err - lim)))

    def solo(self):
        ys = []
        for i in range(4):
            y = self.output()
            self.bmsp.synchronize()
            self.launch(i, y)
            h = y.to_host()
            self.check(i, h, "solo")
            if self.oracle_y is not None:
                yr = self.oracle_y[i]
                bound = self.tol * self.mag[i] + 1e-30
                assert np.all(np.abs(h - yr) <= bound + 1e-5 * np.abs(yr)), ("oracle", i, float(np.max(np.abs(h - yr))))
            ys.append(h)
        return ys

    def queued(self, seq, what):
        outs = [self.output() for _ in seq]
        self.bmsp.synchronize()
        for i, y in zip(seq, outs):  # back to back: no host call but the launches themselves
            self.launch(i, y)
        self.bmsp.synchronize()
        got = [y.to_host() for y in outs]
        for n, (i, h) in enumerate(zip(seq, got)):
            self.check(i, h, "%s launch %d" % (what, n))
        return got

    def new_values(self):
        """values 1.5 - v written into A's own value array in place, then invalidate()"""
        v2 = 1.5 - self.v
        A2 = self.bmsp.BmSpMatrix.from_coo(self.nr, self.nc, self.r, self.c, v2, dtype=self.dtype)
        d, s = self.A.device_arrays()[3], A2.device_arrays()[3]
        self.bmsp.check(self.lib.bmsp_memcpy_d2d(d.ptr, s.ptr, d.n * d.dtype.itemsize))
        self.A.invalidate()
        self.set_values(v2)


def assert_bitwise(seq, got, ref, what):
    for n, (i, h) in enumerate(zip(seq, got)):
        assert np.array_equal(h.view(np.uint8), ref[i].view(np.uint8)), (what, "launch", n, "input", i,
                                                                         int(np.count_nonzero(h != ref[i])), "rows differ")


def run_history(case, seed, bitwise, values=False, kernel=None):
    """the three phases; kernel: spmv_launch_info's name, asserted again after the value change"""
    seq = sequence(seed)
    solo = case.solo()
    got = case.queued(seq, "queued")
    if bitwise:
        assert_bitwise(seq, got, solo, "queued vs solo")
    if values:
        case.new_values()
        seq2 = sequence(seed + 1000)
        got = case.queued(seq2, "after new values")
        if bitwise:  # the same input gives the same bits everywhere in the sequence
            first = {}
            for n, i in enumerate(seq2):
                first.setdefault(i, n)
            assert_bitwise(seq2, got, {i: got[n] for i, n in first.items()}, "after new values")
        if kernel is not None:
            assert case.bmsp.spmv_launch_info(case.A)["kernel"] == kernel


@pytest.fixture(scope="module")
def headline():
    from pybmsp import gen
    return gen.rmat(20, 2)  # the matrix bench.py times


def long_row():
    from pybmsp import gen
    nr, nc = 24, 60011
    _, _, r, c, v = gen.random_coo(nr, nc, 90000, seed=22)  # ~7500 tiles per block-row: long items + folds
    return nr, nc, r, c, v


def test_chunk_kernel_headline(oracle, bmsp, headline):
    # the default SpMV on the headline matrix: ~6 K chunks, hub chunks beside window chunks (uneven load); also the row-by-row check of
    # this kernel on this matrix with a general x
    n, _, r, c, v = headline
    case = Case(bmsp, oracle, n, n, r, c, v, seed=1)
    assert bmsp.spmv_launch_info(case.A)["kernel"] == "spmv_chunk_kernel"
    run_history(case, 1, bitwise=True, values=True, kernel="spmv_chunk_kernel")


def test_chunk_kernel_fold_layout(oracle, bmsp, monkeypatch):
    # head, tail, both and neither slot; two- to four-way folds (test_spmv_chunk_folds.LAYOUT)
    monkeypatch.setenv("BMSP_SPMV_CHUNK", "1")
    cells = np.unique(layout(LAYOUT, 11), axis=0)
    r, c = cells[:, 0].astype(np.int32), cells[:, 1].astype(np.int32)
    v = np.random.default_rng(11).uniform(0.1, 1.0, len(cells))
    case = Case(bmsp, oracle, 256, 4096 * 8, r, c, v, seed=2)
    assert bmsp.spmv_launch_info(case.A)["kernel"] == "spmv_chunk_kernel"
    run_history(case, 2, bitwise=True, values=True, kernel="spmv_chunk_kernel")


# (matrix, dtype, entry source, reduction): every <MODE, RED> and every dtype once with long items
VSTREAM = [("headline", 0, "cached", "atomic"), ("long_row", 0, "decode", "sorted"), ("long_row", 1, "cached", "sorted"),
           ("long_row", 1, "decode", "atomic"), ("long_row", 2, "cached", "atomic"), ("long_row", 2, "decode", "sorted")]


@pytest.mark.parametrize("matrix,dtype,src,red", VSTREAM)
def test_value_stream_kernel(oracle, bmsp, monkeypatch, headline, matrix, dtype, src, red):
    monkeypatch.setenv("BMSP_SPMV_NOCHUNK", "1")
    monkeypatch.setenv("BMSP_SPMV_RED", "0" if red == "atomic" else "1")
    if src == "decode":
        monkeypatch.setenv("BMSP_SPMV_NO_POSCACHE", "1")
    if matrix == "headline":
        nr, _, r, c, v = headline
        nc = nr
    else:
        nr, nc, r, c, v = long_row()
    seed = 10 + VSTREAM.index((matrix, dtype, src, red))
    case = Case(bmsp, oracle, nr, nc, r, c, v, dtype=dtype, seed=seed)
    name = "spmv_vstream_kernel<k%s, k%s>" % (src.capitalize(), red.capitalize())
    assert bmsp.spmv_launch_info(case.A)["kernel"] == name
    assert long_block_rows(case.A) > 0
    run_history(case, seed, bitwise=red == "sorted", values=True, kernel=name)


def test_sweep_kernel_sparse(oracle, bmsp, monkeypatch):
    monkeypatch.setenv("BMSP_SPMV_OLD", "1")
    nr, nc, r, c, v = long_row()
    case = Case(bmsp, oracle, nr, nc, r, c, v, seed=20)
    assert bmsp.spmv_launch_info(case.A)["kernel"] == "spmv_sweep_kernel"
    assert long_block_rows(case.A) > 0
    run_history(case, 20, bitwise=True)


def test_sweep_kernel_full_tiles(oracle, bmsp):
    # every tile full: block-rows 0 and 1 hold 600 tiles each (long items), block-rows 2 .. 4 hold 8
    g = np.random.default_rng(21)
    rr, cc = np.meshgrid(np.arange(16), np.arange(4800), indexing="ij")
    r2, c2 = np.meshgrid(np.arange(16, 40), np.arange(64), indexing="ij")
    r = np.concatenate([rr.ravel(), r2.ravel()]).astype(np.int32)
    c = np.concatenate([cc.ravel(), c2.ravel()]).astype(np.int32)
    v = g.uniform(-1.0, 1.0, r.size)
    case = Case(bmsp, oracle, 40, 4800, r, c, v, seed=21)
    assert bmsp.spmv_launch_info(case.A)["kernel"] == "spmv_sweep_kernel<FULL>"
    assert long_block_rows(case.A) == 2
    run_history(case, 21, bitwise=True)


# k -> the kernel spmm.hip's launch() picks on a matrix with the position cache (sparse tiles): k <= 8 the value-stream walk
# (KK = 4 / 8) unless BMSP_SPMM_NO_VSTREAM; otherwise k <= 4 spmm_kernel<4>, k <= 16 spmm_kernel<16>, larger k spmm_wide_kernel
SPMM = [(3, False, "spmm_vstream_kernel<4>"), (6, False, "spmm_vstream_kernel<8>"), (3, True, "spmm_kernel<4>"), (12, False, "spmm_kernel<16>"),
        (40, False, "spmm_wide_kernel")]


@pytest.mark.parametrize("k,no_vstream,kernel", SPMM)
def test_spmm(oracle, bmsp, monkeypatch, k, no_vstream, kernel):
    if no_vstream:
        monkeypatch.setenv("BMSP_SPMM_NO_VSTREAM", "1")
    nr, nc, r, c, v = long_row()
    case = Case(bmsp, oracle, nr, nc, r, c, v, seed=30 + k, kind="spmm", k=k)
    # launch()'s condition for the value-stream walk is the position cache, which the cached value-stream SpMV reads
    assert bmsp.spmv_launch_info(case.A)["kernel"].startswith("spmv_vstream_kernel<kCached")
    assert long_block_rows(case.A) > 0
    # each call synchronizes itself (long items: its carry slots go back to the pool): "queued" is consecutive calls; the value-stream
    # walk adds into LDS in an order the hardware picks, the slot walks reduce in a fixed order
    run_history(case, 30 + k, bitwise=not kernel.startswith("spmm_vstream"))


def test_sharded_spmv_loopback(oracle, bmsp):
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(16, 8)
    comm = bmsp.Comm.loopback(3)
    try:
        case = Case(bmsp, oracle, n, n, r, c, v, seed=40, kind="sharded", comm=comm)
        assert long_block_rows(case.A) > 0
        nbr = (n + 7) // 8
        assert bmsp.spmv_launch_info(case.A.row_panel(0, nbr // 3))["kernel"].startswith("spmv_vstream_kernel")  # row slices
        # the loopback sweeps its panels one after another and synchronizes after each: "queued" is consecutive calls; a row slice
        # takes the value-stream kernel's atomic reduction (sparse tiles), so the bound holds it
        run_history(case, 40, bitwise=False)
    finally:
        comm.free()
