"""Every library call that rewrites a handle's values in place, crossed with every block-MAC kernel that reads a value-derived cache.

A handle caches data derived from its values, which the block-MAC kernels read in place of `values`: dense_tiles (the fp16 tile copies of
the K = 32 MFMA and strip kernels, the dense staging of the vector-ALU kernel), lane_tiles (the fp32 strip kernel, the fp32 MFMA task-list
kernel), csr_rowptr / csr_ent (the row-sparse kernel) and values_finite with the fp32 exponent range (which decide the kernel a product
may take).  A writer that forgets drop_value_caches leaves them stale, and the next product returns, successfully, the numbers of the old
values.  One case here is: build T and a partner, prepare(3), run a product pinned to ONE kernel and assert from the stats that it ran (the
cache exists); apply ONE writer to T; run the product again on T and on `fresh`, a handle adopted from copies of T's four arrays, which has
no cache.  The two products must be bit-identical in all four arrays and report the same kernel, and fresh's product must be the oracle's
product of the new values, bit for bit.

There is no tolerance in this file.  Operand values are positive multiples of 1/16 up to 4, so products are multiples of 1/256 and every
partial sum of the matrix-core kernels (at most 129 terms of at most 4) is exact in fp32 in any order; the fp32 kernels and the fp16
kernels of tc_version 5 follow the oracle's operation order and are compared with it bit for bit whatever the values.  Every writer makes
every value of T strictly larger (old values lie in [1/16, 1]; new ones are old + 1, 4 - 2 old, 2 or 3 times old, or a dot product of at
least 2), and all operands are positive: every stored value of the product grows, so a product computed from a stale cache differs from
the right one in EVERY value.  That condition is asserted on the oracle's products alone, here and in the CPU checks at the end.

Checked by mutation when the file was written: against a library whose drop_value_caches does nothing, every case of the two device
tests fails by assertion except the sixteen `raw` ones (the raw write goes through bmsp_matrix_invalidate, the baseline); against the
library before bmsp_spgemm_numeric dropped C's caches, exactly the numeric_* cases fail.
"""
import contextlib
import os
import subprocess
import numpy as np
import pytest

import util
from conftest import MTX, REPO
from test_spgemm_special_values import compare_with_oracle

INF = float("inf")
FAST = (3, 4, 5)           # strip, fp32 MFMA, row-sparse: right for finite, normal products only
STRIP_K_CAP = 192          # blockmac_strip.hip: merged A tiles of a strip (two block-rows of A)
ROWSPARSE_FILL = 16        # mac_rowsparse_applies / launch_mac_valu: stored values per tile, on average, that separate the two
SWITCHES = ("BMSP_MAC_STRIP", "BMSP_MAC_ROWSPARSE", "BMSP_MAC_VALU_DENSE", "BMSP_MAC_F32MFMA", "BMSP_MAC_B_DENSE", "BMSP_MAC_DIRECT",
            "BMSP_MAC_OLD", "BMSP_MAC_QUOTA", "BMSP_SPGEMM_ROWMERGE", "BMSP_SPGEMM_ROWWINDOW")


# ---------------------------------------------------------------------------------------------------------
# 1. inputs, values, readers, writers
# ---------------------------------------------------------------------------------------------------------
_MEMO = {}


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def _structure(name):
    """(n, rows, cols) of a square pattern: band9 / band64 tiles more than a quarter full (203 and 259 rows: ragged last block-row, several
    block-rows per strip), fem nearly empty tiles, hub an R-MAT whose first block-row of A exceeds the strip kernel's k list"""
    def make():
        from pybmsp import gen
        n, _, r, c, _ = {"band9": lambda: gen.banded(203, 9), "band64": lambda: gen.banded(259, 64), "fem": lambda: gen.fem_like(10, "27pt"),
                         "hub": lambda: gen.rmat(10, 8)}[name]()
        return n, np.asarray(r, np.int64), np.asarray(c, np.int64)
    return _memo(("structure", name), make)


def _old(r, c):
    return (1 + (3 * r + 7 * c) % 16) / 16.0


VALUES = {
    "old": _old,                                                   # [1/16, 1]
    "partner": lambda r, c: (1 + (5 * r + 11 * c + 3) % 16) / 16.0,
    "partner2": lambda r, c: (1 + (7 * r + 13 * c + 5) % 16) / 16.0,
    "partner4": lambda r, c: (1 + (7 * r + 13 * c + 5) % 16) / 4.0,   # [1/4, 4]: against 2^127 a product overflows
    "ones": lambda r, c: np.ones(r.shape),
    # what the writers leave; each strictly above `old`
    "plus1": lambda r, c: _old(r, c) + 1.0,
    "affine": lambda r, c: 4.0 - 2.0 * _old(r, c),                 # add_values with alpha = -2 on `old`, beta = 4 on ones
    "rowscale": lambda r, c: _old(r, c) * (2 + r % 2),            # diag(2, 3, 2, ...) * old
    "dots": lambda r, c: (1.0 + r % 2) + (1.0 + c % 2),           # x_i . y_j with x_i = (1 + i % 2, 1), y_j = (1, 1 + j % 2)
}

# name -> (dtype, tc_version, switches, variants allowed, input): one kernel each, and the cache it reads
READERS = {
    "f16_mfma": (1, 4, {"BMSP_MAC_STRIP": "0", "BMSP_MAC_B_DENSE": "1"}, (1, 2), "band64"),                             # dense_tiles of A and of B
    "f16_strip": (1, 4, {"BMSP_MAC_STRIP": "1"}, (3,), "band9"),                                                        # dense_tiles
    "f16_valu": (1, 5, {"BMSP_MAC_VALU_DENSE": "1", "BMSP_MAC_ROWSPARSE": "0"}, (0,), "band9"),                         # dense_tiles
    "f16_rowsparse": (1, 5, {"BMSP_MAC_ROWSPARSE": "1"}, (5,), "fem"),                                                  # csr_ent
    "f32_rowsparse": (0, 5, {}, (5,), "fem"),                                                                           # csr_ent
    "f32_strip": (0, 5, {"BMSP_MAC_ROWSPARSE": "0", "BMSP_MAC_STRIP": "1"}, (3,), "band9"),                             # lane_tiles
    "f32_valu": (0, 5, {"BMSP_MAC_VALU_DENSE": "1", "BMSP_MAC_STRIP": "0", "BMSP_MAC_ROWSPARSE": "0"}, (0,), "band64"),  # fp32 dense_tiles
    "f32_mfma": (0, 5, {"BMSP_MAC_F32MFMA": "1"}, (4,), "band9"),                                                       # lane_tiles
}
F32_READERS = [k for k in READERS if READERS[k][0] == 0]

# ordinary writers: name -> the values they leave in T.  Each acts on T in tile layout 0 (T is the left operand) and 1 (the right one).
WRITERS = {"raw": "plus1", "copy_layout": "plus1", "copy_transpose": "plus1", "add_values": "affine", "scale_inplace": "rowscale",
           "scale_values": "rowscale", "sddmm_inplace": "dots", "sddmm_values": "dots", "masked_inplace": "rowscale", "masked_values": "rowscale"}
# bmsp_spgemm_numeric, T = C (fp32, layout 0: left operand of fp32 readers only): name -> (operand dtype, tc_version, switches of the call)
NUMERIC = {
    "numeric_strip": (0, 5, {}),                                                       # a structure-only kernel alone (strip or row-sparse)
    "numeric_tasklist": (0, 5, {"BMSP_MAC_STRIP": "0", "BMSP_MAC_ROWSPARSE": "0"}),   # T_7 from the task list bmsp_spgemm_symbolic kept
    "numeric_whole": (1, 4, {}),                                                       # hub block-row: the whole product, checked, copied
}
# the hub C (a block-row of 123 tiles, more than the strip kernel's k list takes from a left operand) meets the kernels without that limit
WHOLE_READERS = ["f32_rowsparse", "f32_valu", "f32_mfma"]


def _input(writer, reader):
    return "hub" if writer == "numeric_whole" else READERS[reader][4]


def _cases():
    out = [(w, r, s) for w in WRITERS for r in READERS for s in ("left", "right")]
    out += [(w, r, "left") for w in NUMERIC for r in (WHOLE_READERS if w == "numeric_whole" else F32_READERS)]
    return out


def _ids(cases):
    return [pytest.param(*c, id="-".join(c)) for c in cases]


# ---------------------------------------------------------------------------------------------------------
# 2. the oracle's side: T before and after the writer, and the product with the partner (computed once, never written to)
# ---------------------------------------------------------------------------------------------------------
def _omat(oracle, inp, values, dtype, layout):
    def make():
        n, r, c = _structure(inp)
        return oracle.bmsp_from_coo(oracle.Coo(n, n, r, c, VALUES[values](r, c)), dtype, bool(layout))
    return _memo(("omat", inp, values, dtype, bool(layout)), make)


def _oracle_T(oracle, writer, inp, dtype, side, new):
    if writer in NUMERIC:
        od, otc, _ = NUMERIC[writer]
        A, P = _omat(oracle, inp, "plus1" if new else "old", od, False), _omat(oracle, inp, "partner2", od, True)
        return _memo(("oC", inp, od, otc, new), lambda: oracle.spgemm(A, P, exact_products=(otc != 5))[0])
    return _omat(oracle, inp, WRITERS[writer] if new else "old", dtype, side == "right")


def _oracle_D(oracle, writer, reader, side, new):
    dtype, tc, _, _, _ = READERS[reader]
    inp = _input(writer, reader)
    what = (writer if writer in NUMERIC else WRITERS[writer]) if new else ("old", writer in NUMERIC and NUMERIC[writer][:2])
    def make():
        T = _oracle_T(oracle, writer, inp, dtype, side, new)
        P = _omat(oracle, inp, "partner", dtype, side == "left")
        a, b = (T, P) if side == "left" else (P, T)
        return oracle.spgemm(a, b, exact_products=(tc != 5))[0]
    return _memo(("oD", inp, dtype, tc, side, what), make)


def _assert_every_value_differs(old, new):
    np.testing.assert_array_equal(old.keys, new.keys)
    np.testing.assert_array_equal(old.bmps, new.bmps)
    assert old.nnz == new.nnz and old.nnz > 0
    assert np.isfinite(old.values).all() and np.isfinite(new.values).all()
    same = np.flatnonzero(old.values == new.values)
    assert same.size == 0, "%d of %d product values do not change: a stale cache would go unnoticed there" % (same.size, old.nnz)


# ---------------------------------------------------------------------------------------------------------
# 3. the device's side
# ---------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _env(monkeypatch, env):
    """exactly these block-MAC switches, whatever the caller's environment holds"""
    with monkeypatch.context() as m:
        for k in SWITCHES:
            m.delenv(k, raising=False)
        for k, v in env.items():
            m.setenv(k, v)
        yield


def _raw_write(bmsp, M, n, r, c, v, dtype, layout):
    """new values through the public pointer, then bmsp_matrix_invalidate(M, 0): the documented contract"""
    src = bmsp.BmSpMatrix.from_coo(n, n, r, c, v, transposed=layout, dtype=dtype)
    d, s = M.device_arrays()[3], src.device_arrays()[3]
    assert d.n == s.n
    bmsp.check(bmsp.lib().bmsp_memcpy_d2d(d.ptr, s.ptr, d.n * d.dtype.itemsize))
    bmsp.synchronize()
    M.invalidate(False)


def _vectors(bmsp, n, dtype):
    """(diag(2, 3, 2, ...) as a float32 vector, X, Y of the `dots` values in T's dtype)"""
    i = np.arange(n)
    dl = bmsp.DeviceArray.from_host((2 + i % 2).astype(np.float32))
    X = np.stack([1.0 + i % 2, np.ones(n)], axis=1)
    Y = np.stack([np.ones(n), 1.0 + i % 2], axis=1)
    return dl, bmsp.DeviceArray.from_host(X.ravel(), bmsp.NP_DTYPE[dtype]), bmsp.DeviceArray.from_host(Y.ravel(), bmsp.NP_DTYPE[dtype])


def _build(bmsp, monkeypatch, writer, inp, dtype, side):
    """(T, write, keep): T holds the `old` values (or, for bmsp_spgemm_numeric, the product of `old` and `partner2`); write() applies the
    writer; keep holds what must outlive both"""
    n, r, c = _structure(inp)
    L = side == "right"
    mk = lambda values, layout, dt=dtype: bmsp.BmSpMatrix.from_coo(n, n, r, c, VALUES[values](r, c), transposed=layout, dtype=dt)
    if writer in NUMERIC:
        od, otc, wenv = NUMERIC[writer]
        A0, A1, P = mk("old", False, od), mk("plus1", False, od), mk("partner2", True, od)
        with _env(monkeypatch, wenv):
            if writer == "numeric_tasklist":
                T, _ = bmsp.spgemm_symbolic(A0, P, tc_version=otc)
                bmsp.spgemm_numeric(A0, P, T, tc_version=otc)
            else:
                T, _ = bmsp.spgemm(A0, P, tc_version=otc)

        def write():
            with _env(monkeypatch, wenv):
                st = bmsp.spgemm_numeric(A1, P, T, tc_version=otc)
            t = st["t_us"]
            if writer == "numeric_strip":       # the strip or the row-sparse kernel alone: no symbolic stage, no task list
                assert t[3] == 0 and t[4] == 0 and t[5] == 0 and t[7] > 0 and st["mac_variant"] in (3, 5) and st["surviving_tasks"] == 0, st
            elif writer == "numeric_tasklist":  # T_7 alone from the kept list, by a task-list kernel
                assert t[3] == 0 and t[4] == 0 and t[5] == 0 and t[7] > 0 and st["mac_variant"] not in (3, 5) and st["surviving_tasks"] > 0, st
            else:                               # the whole product ran behind the call (its symbolic stages were timed)
                assert sum(t[1:7]) > 0 and st["surviving_tasks"] > 0, st
        return T, write, [A0, A1, P]
    new = WRITERS[writer]
    dl, dX, dY = _vectors(bmsp, n, dtype)
    if writer == "raw":
        T = mk("old", L)
        return T, lambda: _raw_write(bmsp, T, n, r, c, VALUES[new](r, c), dtype, L), []
    if writer in ("copy_layout", "copy_transpose"):
        if writer == "copy_layout":
            sr, sc = r, c
            src = mk("old", not L)
            T = src.with_layout(L)
        else:
            sr, sc = c, r     # src = T^T: entry (j, i) holds the value of T's (i, j)
            src = bmsp.BmSpMatrix.from_coo(n, n, sr, sc, VALUES["old"](r, c), transposed=not L, dtype=dtype)
            T = src.transpose(L)

        def write():
            _raw_write(bmsp, src, n, sr, sc, VALUES[new](r, c), dtype, not L)
            T.copy_values_from(src)
        return T, write, [src]
    if writer == "add_values":
        X, Y = mk("old", L), mk("ones", L)
        T = bmsp.add(X, Y, 1.0, 0.0, transposed=L)
        return T, lambda: bmsp.add_values(T, X, Y, -2.0, 4.0), [X, Y]
    if writer == "scale_inplace":
        T = mk("old", L)
        return T, lambda: T.scale_(left=dl), [dl]
    if writer == "sddmm_inplace":
        T = mk("old", L)
        return T, lambda: T.sddmm_(dX, dY, 2), [dX, dY]
    if writer == "masked_inplace":
        T, D, B = mk("old", L), bmsp.from_diagonal(dl, dtype=dtype), mk("old", True)
        return T, lambda: bmsp.spgemm_masked_values(T, D, B, T, 1.0, 0.0), [dl, D, B]
    # into a copy in the other layout's handle: src keeps the old values, T = src.with_layout(L) receives the new ones
    src = mk("old", not L)
    T = src.with_layout(L)
    if writer == "scale_values":
        return T, lambda: bmsp.scale_values(T, src, left=dl), [src, dl]
    if writer == "sddmm_values":
        return T, lambda: bmsp.sddmm_values(T, src, dX, dY, 2), [src, dX, dY]
    if writer == "masked_values":
        D, B = bmsp.from_diagonal(dl, dtype=dtype), mk("old", True)
        return T, lambda: bmsp.spgemm_masked_values(T, D, B, src, 1.0, 0.0), [src, dl, D, B]
    raise ValueError(writer)


def _fresh(bmsp, M):
    """a handle adopted from copies of M's four arrays: no cache, no flag"""
    i = M.info()
    k, b, o, v = M.host_arrays()
    return bmsp.BmSpMatrix.from_arrays(i["num_rows"], i["num_cols"], k, b, o, v, dtype=i["dtype"], transposed=i["transposed"])


def _assert_same_product(Ca, Cb):
    for name, x, y in zip(("keys", "bmps", "offsets", "values"), Ca.host_arrays(), Cb.host_arrays()):
        assert x.shape == y.shape, name
        bad = np.flatnonzero(x.view(np.uint8) != y.view(np.uint8))
        assert bad.size == 0, "%s: %d of %d bytes differ between the product on T and on the cache-free handle" % (name, bad.size, x.nbytes)


@pytest.mark.gpu
@pytest.mark.parametrize("writer,reader,side", _ids(_cases()))
def test_writer_drops_what_the_reader_reads(oracle, bmsp, monkeypatch, writer, reader, side):
    """One writer, one pinned kernel, T on one side (see the file's docstring).  Step a asserts from the stats that the pinned kernel ran
    on the old values and gave the oracle's product, so that the cache under test exists and holds the old values; step c that the
    product on T after the write is that of a cache-free handle and the oracle's product of the new values."""
    dtype, tc, env, variants, _ = READERS[reader]
    inp = _input(writer, reader)
    t_dtype = 0 if writer in NUMERIC else dtype
    n, r, c = _structure(inp)
    T, write, keep = _build(bmsp, monkeypatch, writer, inp, dtype, side)
    partner = bmsp.BmSpMatrix.from_coo(n, n, r, c, VALUES["partner"](r, c), transposed=(side == "left"), dtype=dtype)

    def product(M):
        a, b = (M, partner) if side == "left" else (partner, M)
        with _env(monkeypatch, env):
            return bmsp.spgemm(a, b, tc_version=tc)

    D_old, D_new = _oracle_D(oracle, writer, reader, side, False), _oracle_D(oracle, writer, reader, side, True)
    _assert_every_value_differs(D_old, D_new)
    # a. the cache exists
    T.prepare(3)
    C0, st0 = product(T)
    assert st0["mac_kernel"] == (tc if dtype == 1 and tc != 5 else 5) and st0["mac_variant"] in variants, st0
    util.assert_bmsp_equal_exact(D_old, *C0.host_arrays(), np.float32)
    # b. the writer; T now holds what the writer is meant to leave
    write()
    util.assert_bmsp_equal_exact(_oracle_T(oracle, writer, inp, dtype, side, True), *T.host_arrays(), bmsp.NP_DTYPE[t_dtype])
    # c. T against a handle without caches, and that against the oracle
    fresh = _fresh(bmsp, T)
    C1, st1 = product(T)
    Cf, stf = product(fresh)
    assert stf["mac_variant"] in variants, stf
    assert st1["mac_variant"] == stf["mac_variant"] and st1["mac_kernel"] == stf["mac_kernel"], (st1, stf)
    _assert_same_product(C1, Cf)
    util.assert_bmsp_equal_exact(D_new, *Cf.host_arrays(), np.float32)


# ---------------------------------------------------------------------------------------------------------
# 4. the finite flag and the exponent range follow the writer
# ---------------------------------------------------------------------------------------------------------
FLAG_READERS = ["f32_strip", "f32_rowsparse", "f32_mfma"]
FLAG_WRITERS = ["scale_inf", "scale_tiny", "add_huge", "sddmm_inf", "numeric_overflow"]


def _flag_cases():
    return [(w, r, s) for w in FLAG_WRITERS for r in FLAG_READERS for s in (("left",) if w == "numeric_overflow" else ("left", "right"))]


def _mid(inp):
    """(row, column, index) of the middle stored entry of the middle row"""
    n, r, c = _structure(inp)
    idx = np.flatnonzero(r == n // 2)
    assert idx.size
    p = int(idx[idx.size // 2])
    return int(r[p]), int(c[p]), p


def _poisoned(inp, writer):
    """what the poisoning call of a flag writer leaves in T, as float32 values in the order of _structure (the CPU's model of it)"""
    n, r, c = _structure(inp)
    i0, _, p = _mid(inp)
    old = _old(r, c).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        if writer == "scale_inf":
            d = np.ones(n, np.float32); d[i0] = INF
            return old * d[r]
        if writer == "scale_tiny":
            return old * np.float32(2.0 ** -70) * np.float32(2.0 ** -70)
        if writer == "add_huge":
            x = np.zeros(r.shape, np.float32); x[p] = np.float32(1e30)
            return np.float32(1e30) * x + old
        if writer == "sddmm_inf":
            x0 = (1.0 + np.arange(n) % 2).astype(np.float32); x0[i0] = INF
            return x0[r] * np.float32(1.0) + np.float32(1.0) * (1.0 + c % 2).astype(np.float32)
    raise ValueError(writer)


def _overflow_operand(inp):
    n, r, c = _structure(inp)
    v = _old(r, c)
    v[_mid(inp)[2]] = 2.0 ** 127
    return v


def _flag_build(bmsp, monkeypatch, writer, inp, side):
    """(T, poison, restore, keep) for fp32: T finite, the call that makes its values non-finite (or its products subnormal), and the call
    that makes them ordinary again"""
    n, r, c = _structure(inp)
    L = side == "right"
    i0, _, p = _mid(inp)
    mk = lambda values, layout: bmsp.BmSpMatrix.from_coo(n, n, r, c, VALUES[values](r, c), transposed=layout, dtype=0)
    dev = lambda a: bmsp.DeviceArray.from_host(np.asarray(a, np.float32))
    if writer == "scale_inf":       # Inf * x stays Inf: the way back is the raw write
        T = mk("old", L)
        d = np.ones(n, np.float32); d[i0] = INF
        dv = dev(d)
        return T, lambda: T.scale_(left=dv), lambda: _raw_write(bmsp, T, n, r, c, _old(r, c), 0, L), [dv]
    if writer == "scale_tiny":      # 2^-70 twice over: values around 2^-142, subnormal and exact; 2^70 twice over brings them back
        T = mk("old", L)
        lo, hi = dev(np.full(n, 2.0 ** -70)), dev(np.full(n, 2.0 ** 70))
        return T, lambda: (T.scale_(left=lo), T.scale_(left=lo)), lambda: (T.scale_(left=hi), T.scale_(left=hi)), [lo, hi]
    if writer == "add_huge":        # alpha = 1e30 on an X that holds 1e30 at one entry of Y's pattern
        X = bmsp.BmSpMatrix.from_coo(n, n, r[[p]], c[[p]], np.array([1e30]), transposed=L, dtype=0)
        Y = mk("old", L)
        T = bmsp.add(X, Y, 0.0, 1.0, transposed=L)
        return T, lambda: bmsp.add_values(T, X, Y, 1e30, 1.0), lambda: bmsp.add_values(T, X, Y, 0.0, 1.0), [X, Y]
    if writer == "sddmm_inf":
        _, dX, dY = _vectors(bmsp, n, 0)
        x = np.stack([1.0 + np.arange(n) % 2, np.ones(n)], axis=1); x[i0, 0] = INF
        dXb = dev(x.ravel())
        T = mk("old", L)
        T.sddmm_(dX, dY, 2)
        return T, lambda: T.sddmm_(dXb, dY, 2), lambda: T.sddmm_(dX, dY, 2), [dX, dY, dXb]
    if writer == "numeric_overflow":  # one entry of A at 2^127 against values of P up to 4: entries of C overflow in the fmaf chain
        A0, P = mk("old", False), mk("partner4", True)
        Ab = bmsp.BmSpMatrix.from_coo(n, n, r, c, _overflow_operand(inp), dtype=0)
        with _env(monkeypatch, {}):
            T, _ = bmsp.spgemm(A0, P, tc_version=5)

        def numeric(A):
            with _env(monkeypatch, {}):
                bmsp.spgemm_numeric(A, P, T, tc_version=5)
        return T, lambda: numeric(Ab), lambda: numeric(A0), [A0, Ab, P]
    raise ValueError(writer)


def _oracle_of(oracle, M):
    """the oracle's matrix of a handle's CURRENT arrays"""
    i = M.info()
    k, b, o, v = M.host_arrays()
    return oracle.Bmsp(i["num_rows"], i["num_cols"], i["dtype"], i["transposed"], k, b, o, v.astype(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("writer,reader,side", _ids(_flag_cases()))
def test_writer_resets_the_value_flags(oracle, bmsp, monkeypatch, writer, reader, side):
    """Finite T, prepare(3) and a product: the pinned fast kernel (fp32 strip, row-sparse or fp32 MFMA) runs, so values_finite is cached as
    1 with the exponent range.  The writer then leaves an Inf / NaN in T, or values whose products fall below the normal range: the
    product on T must be, bit for bit, that of a cache-free handle with T's arrays, by the same kernel -- not a fast one -- and that must
    be the oracle's product (NaN by position, everything else by its bits).  Then the way back: ordinary values again, and T takes the
    fast kernel again, as the cache-free handle does."""
    dtype, tc, env, variants, inp = READERS[reader]
    n, r, c = _structure(inp)
    T, poison, restore, keep = _flag_build(bmsp, monkeypatch, writer, inp, side)
    partner = bmsp.BmSpMatrix.from_coo(n, n, r, c, VALUES["partner"](r, c), transposed=(side == "left"), dtype=0)

    def product(M):
        a, b = (M, partner) if side == "left" else (partner, M)
        with _env(monkeypatch, env):
            return bmsp.spgemm(a, b, tc_version=tc)

    def check(fast):
        fresh = _fresh(bmsp, T)
        (C1, st1), (Cf, stf) = product(T), product(fresh)
        assert (stf["mac_variant"] in variants) if fast else (stf["mac_variant"] not in FAST), stf
        assert st1["mac_variant"] == stf["mac_variant"], (st1, stf)
        _assert_same_product(C1, Cf)
        ot, op = _oracle_of(oracle, fresh), _oracle_of(oracle, partner)
        ref, _ = oracle.spgemm(*((ot, op) if side == "left" else (op, ot)))
        compare_with_oracle(Cf, ref, True)
        return ref

    T.prepare(3)
    first = check(True)
    assert np.isfinite(first.values).all()
    poison()
    v = T.host_arrays()[3]
    if writer == "scale_tiny":
        assert np.isfinite(v).all() and float(np.abs(v).min()) * float(VALUES["partner"](r, c).min()) < 2.0 ** -126
    else:
        assert not np.isfinite(v).all()
    bad = check(False)
    assert writer == "scale_tiny" or not np.isfinite(bad.values).all()
    restore()
    again = check(True)
    np.testing.assert_array_equal(again.values, first.values)


# ---------------------------------------------------------------------------------------------------------
# 5. the same sequence through the C++ surface
# ---------------------------------------------------------------------------------------------------------
def build_cpp_numeric_refresh_check(out_path):
    lib_dir = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp_numeric_refresh_check.cpp"), "-o", out_path, "-L" + lib_dir, "-lbmsp",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_numeric_refresh_check_compiles_and_links(tmp_path):
    """include/bmSpMatrix.h with bmSparse_mult / bmSparse_mult_numeric on a product as the left operand links with a plain host compiler"""
    build_cpp_numeric_refresh_check(str(tmp_path / "cpp_numeric_refresh_check"))


@pytest.mark.gpu
def test_cpp_numeric_refresh(tmp_path, bmsp):
    """tests/cpp_numeric_refresh_check.cpp: C = A P, D1 = C R, new values in A, bmSparse_mult_numeric, D2 = C R on the 7-point Laplacian:
    D2 equals the product on a C adopted afresh and is twice D1"""
    exe = str(tmp_path / "cpp_numeric_refresh_check")
    build_cpp_numeric_refresh_check(exe)
    out = subprocess.run([exe, os.path.join(MTX, "laplacian", "7pt_10x10x10.mtx")], capture_output=True, text=True)
    checks = [l.split() for l in out.stdout.splitlines() if l.startswith("CHECK")]
    assert out.returncode == 0 and len(checks) == 1, (out.stdout[-400:], out.stderr[-400:])
    f = checks[0]
    assert f[1] == "numeric_refresh" and f[-2:] == ["FRESH_OK", "DOUBLED_OK"] and int(f[8]) > 0, f
    assert int(f[3]) in FAST and int(f[4]) in FAST, f   # the products with C on the left ran a kernel that reads a cache of C


# ---------------------------------------------------------------------------------------------------------
# 6. CPU checks of what the device tests rest on (oracle and numpy only)
# ---------------------------------------------------------------------------------------------------------
def _mean_fill(m):
    return m.nnz / max(1, m.block_num)


def _max_row_blocks(m):
    return int(np.bincount((m.keys >> np.uint64(32)).astype(np.int64)).max())


def test_every_case_is_named_once():
    cases = _cases() + _flag_cases()
    assert len(set(cases)) == len(cases)
    assert {w for w, _, _ in _cases()} == set(WRITERS) | set(NUMERIC) and {r for _, r, _ in _cases()} == set(READERS)


@pytest.mark.parametrize("writer,reader,side", _ids(_cases()))
def test_old_and_new_products_differ_in_every_value(oracle, writer, reader, side):
    """the condition against vacuity, on the oracle alone: same structure, no value of the product survives the writer; and the values
    are what the file's docstring says -- positive multiples of 1/16 up to 4, representable as stored, the new ones above the old"""
    dtype, tc, _, _, _ = READERS[reader]
    inp = _input(writer, reader)
    _assert_every_value_differs(_oracle_D(oracle, writer, reader, side, False), _oracle_D(oracle, writer, reader, side, True))
    old, new = _oracle_T(oracle, writer, inp, dtype, side, False), _oracle_T(oracle, writer, inp, dtype, side, True)
    np.testing.assert_array_equal(old.keys, new.keys)
    np.testing.assert_array_equal(old.bmps, new.bmps)
    assert (new.values > old.values).all() and (old.values > 0).all()
    if writer not in NUMERIC:
        for m in (old, new):
            assert (m.values * 16 == np.round(m.values * 16)).all() and m.values.max() <= 4.0
            np.testing.assert_array_equal(m.values_as_dtype().astype(np.float64), m.values)
    else:   # C: sums of products of multiples of 1/16, exact in fp32 whatever the order (the matrix-core product of numeric_whole)
        terms = _max_row_blocks(_omat(oracle, inp, "old", 0, False)) * 8
        assert terms * 2.0 * 1.0 * 256 < 2.0 ** 24
        assert (new.values * 256 == np.round(new.values * 256)).all()
        np.testing.assert_array_equal(new.values.astype(np.float32).astype(np.float64), new.values)


@pytest.mark.parametrize("reader", list(READERS))
def test_inputs_lie_on_the_intended_side_of_the_fill_threshold(oracle, reader):
    """the row-sparse kernel takes operands of at most 16 stored values per tile on average, the fp32 dense staging and the readers that
    must not be the row-sparse kernel by default those above; the matrix-core readers' sums stay exact (at most 129 terms of at most 4)"""
    dtype, tc, env, variants, inp = READERS[reader]
    for side in ("left", "right"):
        T, P = _omat(oracle, inp, "old", dtype, side == "right"), _omat(oracle, inp, "partner", dtype, side == "left")
        if inp == "fem":
            assert _mean_fill(T) <= ROWSPARSE_FILL and _mean_fill(P) <= ROWSPARSE_FILL
        else:
            assert _mean_fill(T) >= ROWSPARSE_FILL and _mean_fill(P) >= ROWSPARSE_FILL
    if dtype == 1 and tc != 5:
        n, r, c = _structure(inp)
        assert int(np.bincount(r).max()) * 4.0 * 1.0 * 256 < 2.0 ** 24
    if dtype == 0:   # T = C of bmsp_spgemm_numeric on this reader's input
        C = _oracle_T(oracle, "numeric_strip", inp, 0, "left", True)
        assert (_mean_fill(C) <= ROWSPARSE_FILL) == (inp == "fem"), _mean_fill(C)
        assert 2 * _max_row_blocks(C) <= STRIP_K_CAP      # C is within the strip kernel's reach as a left operand
        assert 2 * _max_row_blocks(_omat(oracle, inp, "old", 0, False)) <= STRIP_K_CAP


def test_hub_case_is_beyond_the_strip_kernel(oracle):
    """numeric_whole: two block-rows of the fp16 operand A merge to more tiles than the strip kernel's k list holds, so no structure-only
    kernel applies to A x P and a C stamped by bmsp_spgemm (no kept task list) takes the checked whole-product path; C itself, as the
    left operand of the readers, has nearly empty tiles (the row-sparse reader applies by default) and a hub block-row too"""
    A = _omat(oracle, "hub", "old", 1, False)
    assert 2 * _max_row_blocks(A) > STRIP_K_CAP, _max_row_blocks(A)
    C = _oracle_T(oracle, "numeric_whole", "hub", 0, "left", True)
    assert 2 * _max_row_blocks(C) > STRIP_K_CAP and _max_row_blocks(C) <= 768, _max_row_blocks(C)
    assert _mean_fill(C) <= ROWSPARSE_FILL and _mean_fill(_omat(oracle, "hub", "partner", 0, True)) <= ROWSPARSE_FILL


@pytest.mark.parametrize("writer", FLAG_WRITERS)
@pytest.mark.parametrize("inp", sorted({READERS[r][4] for r in FLAG_READERS}))
def test_flag_cases_leave_the_values_they_claim(oracle, writer, inp):
    """the poisoned T holds an Inf / NaN -- or, for scale_tiny, exact subnormal values whose products with the partner lie below 2^-126 --
    and the ordinary T does not"""
    n, r, c = _structure(inp)
    partner = VALUES["partner"](r, c)
    assert np.isfinite(_old(r, c)).all() and _old(r, c).min() * partner.min() >= 2.0 ** -126
    if writer == "numeric_overflow":
        A = oracle.bmsp_from_coo(oracle.Coo(n, n, r, c, _overflow_operand(inp)), 0, False)
        assert np.isfinite(A.values).all()
        C, _ = oracle.spgemm(A, _omat(oracle, inp, "partner4", 0, True))
        assert np.isinf(C.values).any() and np.isfinite(C.values).any()
        C0, _ = oracle.spgemm(_omat(oracle, inp, "old", 0, False), _omat(oracle, inp, "partner4", 0, True))
        assert np.isfinite(C0.values).all()
        return
    v = _poisoned(inp, writer)
    if writer == "scale_tiny":
        exact = _old(r, c) * 2.0 ** -140
        np.testing.assert_array_equal(v.astype(np.float64), exact)      # representable: 2^70 twice over restores the old values
        assert np.abs(exact).max() < 2.0 ** -126 and exact.min() * partner.min() < 2.0 ** -126
    else:
        assert not np.isfinite(v).all() and np.isfinite(v).any()
