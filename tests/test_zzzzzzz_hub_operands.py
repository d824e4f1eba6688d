"""GPU cases of tests/test_hub_operands.py (which holds the generators, the table of cases and the CPU self-checks these cases rest on):
the row-sparse block-MAC's CSR copies at every edge of their 64-tile steps and on both sides of the 8192-tile limit, bit for bit
against the oracle (check_spgemm: keys, bitmaps, offsets, values, the four counters), and the sharded product's grow-by-copy branch
against the unsharded product.

Mutation record A -- this file against the library as it was before mac_rowsparse_applies and prepare_spgemm_operand asked about
kRsRowBlocksEnd (the parent commit, built once, run once):
    19 of the 31 cases fail, every one with status BMSP_ERR_LIMIT (-6, "row-sparse block-MAC: a block-row of 8192 or more tiles"), a
    host-side error return before any launch: test_hub_without_a_switch, test_hub_forced and test_hub_prepare for hub_a,
    hub_b_untouched and hub_b_filtered at L = 8192 and 8193 (3 x 6), and test_hub_handle_two_partners.  Every L = 8191 case, full_rows
    and both test_steps_through_the_kernel cases pass: exactly the L >= 8192 cases fail, as read from the code.
Mutation record B -- spgemm_sharded's grow-by-copy branch (comm.hip) with one copy dropped, test_sharded_growth only:
    (i)   without the copy of the earlier rounds' values (nv <- C->values): all six cases fail on the values (grow_tiles 4096, 4096 and
          6832 of 12288 values differ under (2, 2), (2, 4), (3, 3); grow_values 512, 512 and 11776 of 33280) -- also (2, 4) of
          grow_tiles, where only the tiles outgrow their allocation: the branch moves all four arrays;
    (ii)  without the copy of the earlier rounds' offsets: all six cases fail on the offsets (511 .. 1879 entries);
    (iii) nb_cap without the max(need_b, ...): not tried, it is the same program -- with left >= 1 the second argument,
          base + int(size * left * 1.25) + 1024, is never below need = base + size.
    Both gave wrong answers only: host comparisons of arrays the library had finished writing.

The file is named to be collected last: every GPU test that was there before it keeps its place in the order of the suite."""
import numpy as np
import pytest
from test_gpu_parity import check_spgemm
from test_zzz_spgemm_regimes import _SWITCHES
from test_hub_operands import (RS_ROW_BLOCKS_END, HUB_CASES, SHARD_RUNS, EXPECTED_GROWTH, case, second_partner, short_a, growth_events)

pytestmark = pytest.mark.gpu
ROWSPARSE = 5       # BMSP_MAC_ROWSPARSE (bmsp.h)
F32_V15, F16_V15 = (0, 5), (1, 5)


def run(oracle, bmsp, monkeypatch, kind, L, env, numerics):
    """one product under exactly these switches, bit for bit against the oracle; returns the statistics"""
    dtype, tc = numerics
    with monkeypatch.context() as m:
        for k in _SWITCHES + ("BMSP_RS_LANES",):
            m.delenv(k, raising=False)
        for k, v in env.items():
            m.setenv(k, v)
        A, B = case(kind, L)
        st = check_spgemm(oracle, bmsp, A, B, dtype, 0, tc, exact_expected=True)
    print(kind, L, env, numerics, {k: st[k] for k in ("sort_path", "sort_long", "mac_variant", "mac_kernel", "bmp_reduction")})
    return st


@pytest.mark.parametrize("lanes", [None, "8"])
def test_steps_through_the_kernel(oracle, bmsp, monkeypatch, lanes):
    """block-rows of 0 .. 193 tiles on both sides (layout 0 and, through tile_transpose, layout 1), ragged edges: the CSR copies' steps
    and carries, read by the kernel with the lane width it picks and with 8"""
    env = {"BMSP_SPGEMM_ROWMERGE": "1", "BMSP_MAC_ROWSPARSE": "1"}
    if lanes:
        env["BMSP_RS_LANES"] = lanes
    for numerics in (F32_V15, F16_V15):
        st = run(oracle, bmsp, monkeypatch, "steps", 0, env, numerics)
        assert st["mac_variant"] == ROWSPARSE, st


@pytest.mark.parametrize("kind,L", HUB_CASES)
def test_hub_without_a_switch(oracle, bmsp, monkeypatch, kind, L):
    """a hub block-row of 8191 tiles is multiplied by the row-sparse kernel; one of 8192 or 8193 -- in A, in a block-row of B that A
    never touches, in one whose pairs all die in the filter -- by a kernel that reads tiles, and the call succeeds"""
    for numerics in (F32_V15, F16_V15):
        st = run(oracle, bmsp, monkeypatch, kind, L, {}, numerics)
        assert (st["mac_variant"] == ROWSPARSE) == (L < RS_ROW_BLOCKS_END), st
        if kind == "hub_b_filtered":
            assert st["bmp_reduction"] >= L


@pytest.mark.parametrize("kind,L", HUB_CASES + [("full_rows", 8191)])
def test_hub_forced(oracle, bmsp, monkeypatch, kind, L):
    """BMSP_MAC_ROWSPARSE=1 lifts the fill rule, never the limit; full_rows: row counts of 65528 in adjacent 16-bit fields"""
    for numerics in (F32_V15, F16_V15):
        st = run(oracle, bmsp, monkeypatch, kind, L, {"BMSP_MAC_ROWSPARSE": "1"}, numerics)
        assert (st["mac_variant"] == ROWSPARSE) == (L < RS_ROW_BLOCKS_END), st


def _clear(m):
    for k in _SWITCHES + ("BMSP_RS_LANES", "BMSP_SHARD_ROUNDS"):
        m.delenv(k, raising=False)


def _handles(bmsp, A, B, dtype):
    return (bmsp.BmSpMatrix.from_coo(*A, transposed=False, dtype=dtype), bmsp.BmSpMatrix.from_coo(*B, transposed=True, dtype=dtype))


@pytest.mark.parametrize("kind,L", HUB_CASES)
def test_hub_prepare(bmsp, monkeypatch, kind, L):
    """bmsp_matrix_prepare(SPGEMM) of both operands succeeds whatever the hub's length (fp32: the CSR copy below the limit, lane tiles
    from it on); the product of prepared handles is the product of unprepared ones, from the same kernel"""
    with monkeypatch.context() as m:
        _clear(m)
        A, B = case(kind, L)
        for dtype in (0, 1):
            a1, b1 = _handles(bmsp, A, B, dtype)
            a1.prepare(2)
            b1.prepare(2)
            c1, st1 = bmsp.spgemm(a1, b1, tc_version=5)
            a0, b0 = _handles(bmsp, A, B, dtype)
            c0, st0 = bmsp.spgemm(a0, b0, tc_version=5)
            for x, y in zip(c1.host_arrays(), c0.host_arrays()):
                np.testing.assert_array_equal(x, y)
            assert st1["mac_variant"] == st0["mac_variant"] and (st1["mac_variant"] == ROWSPARSE) == (L < RS_ROW_BLOCKS_END), (st0, st1)


def _against_oracle(oracle, A, B, dtype, Cm, st):
    oc, ost = oracle.spgemm(oracle.bmsp_from_coo(oracle.Coo(*A), dtype, False), oracle.bmsp_from_coo(oracle.Coo(*B), dtype, True))
    for k in ("task_list_size", "bmp_reduction", "surviving_tasks", "c_blocks", "c_nnz"):
        assert st[k] == ost[k], (k, st, ost)
    k, b, o, v = Cm.host_arrays()
    np.testing.assert_array_equal(k, oc.keys)
    np.testing.assert_array_equal(b, oc.bmps)
    np.testing.assert_array_equal(o, oc.offsets)
    np.testing.assert_array_equal(v.astype(np.float64), oc.values)


def test_hub_handle_two_partners(oracle, bmsp, monkeypatch):
    """the hub A (8193 tiles) times its narrow B, then times a second B with which a short-rowed A takes the row-sparse kernel (shown on
    the hub A's short block-row alone): nothing the handle remembers from the first product sends the second to the kernel"""
    L = 8193
    with monkeypatch.context() as m:
        _clear(m)
        A, B = case("hub_a", L)
        B2, As = second_partner(L), short_a(L)
        for dtype in (0, 1):
            a, b = _handles(bmsp, A, B, dtype)
            a_short, b2 = _handles(bmsp, As, B2, dtype)
            for partner, coo in ((b, B), (b2, B2), (b, B)):
                Cm, st = bmsp.spgemm(a, partner, tc_version=5)
                assert st["mac_variant"] != ROWSPARSE, st
                _against_oracle(oracle, A, coo, dtype, Cm, st)
            Cm, st = bmsp.spgemm(a_short, b2, tc_version=5)
            assert st["mac_variant"] == ROWSPARSE, st
            _against_oracle(oracle, As, B2, dtype, Cm, st)


@pytest.mark.parametrize("P,rounds", SHARD_RUNS)
@pytest.mark.parametrize("kind", ["grow_tiles", "grow_values"])
def test_sharded_growth(bmsp, monkeypatch, kind, P, rounds):
    """a later round outgrows the allocation made after round 0: the earlier rounds' slices are copied into new arrays.  All four arrays
    equal the unsharded product's; that the branch ran is read off the library's own partition and the whole C through the restated
    rule, in the round and on the resource the CPU check worked out.  Twice per communicator (the second call reuses its stream)."""
    with monkeypatch.context() as m:
        _clear(m)
        A_coo, B_coo = case(kind)
        comm = bmsp.Comm.loopback(P)
        for dtype, tc in ((0, 5), (1, 4)):
            A, Bt = _handles(bmsp, A_coo, B_coo, dtype)
            whole, st0 = bmsp.spgemm(A, Bt, tc_version=tc)
            ref = whole.host_arrays()
            bounds = bmsp.partition_rows(A, Bt, rounds * P)
            first = np.searchsorted((ref[0] >> np.uint64(32)).astype(np.int64), bounds)      # the first tile of every panel
            tiles, values = np.diff(first), np.diff(ref[2].astype(np.int64)[first])
            assert growth_events(tiles, values, P, rounds) == EXPECTED_GROWTH[kind][(P, rounds)], (bounds, tiles, values)
            for _ in range(2):
                Cs, st, sh = bmsp.spgemm_sharded(comm, A, Bt, tc_version=tc, rounds=rounds, gather=True)
                for x, y in zip(Cs.host_arrays(), ref):
                    np.testing.assert_array_equal(x, y)
                assert sh["world"] == P and st["surviving_tasks"] == st0["surviving_tasks"] and st["c_blocks"] == st0["c_blocks"] == whole.block_num
                assert sh["exchange_bytes"] == 24 * whole.block_num + 4 * whole.nnz and sh["gathered"] == 1 and sh["rounds"] == rounds
                assert 0.0 <= sh["exchange_hidden_frac"] <= 1.0 and sh["exchange_exposed_us"] <= sh["exchange_us"] + 1e-6
        comm.free()
