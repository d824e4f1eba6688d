"""GPU cases of the pair-memory tests: every history of tests/test_spgemm_pair_memory.py (which holds the pairs, the table of histories
and the CPU self-checks these cases rest on, and describes them) applied to fresh handles of a pair, then the probe: the product under
X = (BMSP_SORT_AUTO, tc_version) twice.

    fresh_first(X) / steady(X)   sort_path, sort_long, mac_kernel and mac_variant of the first / second X on fresh handles of the pair, taken
                                 in the same run on handles of their own (base()), never from a table.
    1.  every product -- of the probe, of the history, sharded and paneled ones included -- is the oracle's, as check_spgemm(...,
        exact_expected=True) compares it: keys, bitmaps, offsets, the stage counters, and the values (bit for bit where the kernels
        claim the oracle's order; as numbers, which the exact inputs make the same thing, on the fp16 matrix cores).
    2.  the second X after the history reports steady(X).
    3.  the first X after the history reports fresh_first(X) where the history leaves nothing known about the pair (none, prepared,
        other_partner, twin_partner, invalidate_a, invalidate_b) and steady(X) after every other history.  (The issue's table reads
        "everything else steady"; `none` and `prepared` multiply nothing, so their first probe IS a pair's first product.)
    4.  steady(X) itself where the pair is built for it: S strip mode and the strip kernel; R strip mode and the row-sparse kernel
        under V15's numerics; T task-list mode; W column windows without the task-list attempt; V as R.
There is no tolerance in this file.  The four path fields are printed per product, so a failing log shows the sequence.

The name sorts after test_zzz_spgemm_regimes.py: every GPU test that was there before keeps its place in the order of the suite.

Cells left out: none.  (W under `sharded` takes under two seconds on MI355X.)

Mutation record (MI355X, each library built from a scratch copy of the tree; case ids as pytest prints them):
  * the library before this change (one field rm_partner_mode, 1 strip / 2 task list / 3 pipeline / 4 windows): 13 of the 138 cases of
    test_pair_memory fail, all on the path assertions (rule 2 / 3), none on a value --
      S-f16-tc4-other_tc, S-f16-tc4-switch_off_strip, S-f32-tc5-switch_off_strip, R-f32-tc5-switch_off_strip,
      R-f16-tc4-switch_off_strip, R-f16-tc5-switch_off_strip           (arguments or switches excluded strip mode; task-list mode stuck)
      V-f16-tc5-other_tc               (under tc_version 4 the strip kernel's k list refuses A: a predicate's refusal was remembered)
      V-f32-tc5-sharded, V-f32-tc5-forced_panels, V-f16-tc5-sharded, V-f16-tc5-forced_panels,
      R-f16-tc5-sharded, R-f16-tc5-forced_panels                      (a view's refusal handed to the parent)
    Both predicted defects showed.  test_views_inherit_and_hand_back passes there.
  * a refusal by the predicate written as "strip mode does not fit" (what the value rule of spgemm.hip forbade before, now for every
    refusal without a pass): V-f32-tc5-sharded, V-f32-tc5-forced_panels, V-f16-tc5-other_tc fail here, and 48 cases of
    test_flag_follows_the_values in test_spgemm_special_values.py (every fp32 case, every fp16 case under BMSP_SPGEMM_ROWMERGE);
    test_views_and_shards_keep_their_own_flag, test_numeric_after_values_turn_non_finite and
    test_structural_refusal_keeps_the_pair_hint do not notice.
  * rm_hint_inherit emptied: none of the 138 cases notices (rule 3 accepts the extra pass of a first probe, and nothing else shows
    it); both cases of test_views_inherit_and_hand_back fail.
"""
import numpy as np
import pytest
from test_spgemm_special_values import compare_with_oracle, exact_bits_for
from test_zzz_spgemm_regimes import _SWITCHES
from test_spgemm_pair_memory import (F32, F16, SORT_AUTO, SORT_SEGMENTED, SORT_GLOBAL, HISTORIES, cases, operands, oracle_product)

FIELDS = ("sort_path", "sort_long", "mac_kernel", "mac_variant")
PATH_ROWMERGE, PATH_ROWWINDOW, RM_STRIP, RM_TASKLIST, MAC_STRIP, MAC_ROWSPARSE = 2, 3, 1, 2, 3, 5
ALL_SWITCHES = tuple(_SWITCHES) + ("BMSP_SPGEMM_FORCE_PANELS",)


class Pair:
    """fresh handles of a pair and the products on them, each compared with the oracle"""

    def __init__(self, oracle, bmsp, pair, dtype):
        self.oracle, self.bmsp, self.pair, self.dtype, self.b_scale = oracle, bmsp, pair, dtype, 1.0
        A, B, _ = operands(pair)
        self.a = bmsp.BmSpMatrix.from_coo(*A, dtype=dtype)
        self.b = self.right(B)

    def right(self, coo):
        return self.bmsp.BmSpMatrix.from_coo(*coo, transposed=True, dtype=self.dtype)

    def reference(self, tc, partner="b"):
        return oracle_product(self.oracle, self.pair, self.dtype, tc, partner, self.b_scale if partner == "b" else 1.0)

    def check(self, what, Cm, st, tc, partner="b", structure_only=False):
        ref, rst = self.reference(tc, partner)
        print(self.pair, self.dtype, what, "tc", tc, {k: st[k] for k in FIELDS if k in st})
        if structure_only:
            for key in ("task_list_size", "bmp_reduction", "surviving_tasks", "c_blocks", "c_nnz"):
                assert st[key] == rst[key], (key, st[key], rst[key])
            k, b, o, v = Cm.host_arrays()
            assert np.array_equal(k, ref.keys) and np.array_equal(b, ref.bmps) and np.array_equal(o, ref.offsets) and not v.any()
        else:
            compare_with_oracle(Cm, ref, exact_bits_for(self.dtype, tc), st, rst)
        return tuple(st[k] for k in FIELDS)

    def multiply(self, what, tc, mode=SORT_AUTO, a=None, b=None, partner="b"):
        Cm, st = self.bmsp.spgemm(self.a if a is None else a, self.b if b is None else b, mode=mode, tc_version=tc)
        return self.check(what, Cm, st, tc, partner)


_BASE = {}


def base(oracle, bmsp, pair, dtype, tc):
    """(fresh_first(X), steady(X)) on handles of their own, once per session"""
    if (pair, dtype, tc) not in _BASE:
        p = Pair(oracle, bmsp, pair, dtype)
        _BASE[(pair, dtype, tc)] = (p.multiply("fresh first", tc), p.multiply("fresh second", tc))
    return _BASE[(pair, dtype, tc)]


def apply_history(p, history, tc, monkeypatch):
    bmsp = p.bmsp
    A, B, B2 = operands(p.pair)
    if history == "other_tc":
        for _ in range(2):
            p.multiply(history, 4 if tc == 5 else 5)
    elif history == "explicit_mode":
        p.multiply(history + " segmented", tc, mode=SORT_SEGMENTED)
        p.multiply(history + " global", tc, mode=SORT_GLOBAL)
    elif history == "symbolic_numeric":
        Cm, st = bmsp.spgemm_symbolic(p.a, p.b, tc_version=tc)
        p.check(history + " symbolic", Cm, st, tc, structure_only=True)
        for _ in range(2):
            stn = bmsp.spgemm_numeric(p.a, p.b, Cm, tc_version=tc)
            print(p.pair, p.dtype, history + " numeric", {k: stn[k] for k in FIELDS})
            compare_with_oracle(Cm, p.reference(tc)[0], exact_bits_for(p.dtype, tc))
    elif history == "other_partner":
        p.multiply(history + " before", tc)        # (the pair is known; the other partner's product then takes the memory over)
        other = p.multiply(history, tc, b=p.right(B2), partner="b2")
        if built_for(p.pair, p.dtype, tc):
            assert other[:2] != built_for(p.pair, p.dtype, tc)[0], "the other partner was meant to need another mode"
    elif history == "twin_partner":
        p.multiply(history + " before", tc)
        p.multiply(history, tc, b=p.right(B))
    elif history == "writer_on_b":
        p.multiply(history + " before", tc)
        p.b.scale_(left=bmsp.DeviceArray.from_host(np.full(B[0], 2.0, np.float32)))
        p.b_scale = 2.0
    elif history in ("invalidate_a", "invalidate_b"):
        p.multiply(history + " before", tc)
        (p.a if history == "invalidate_a" else p.b).invalidate(True)
    elif history == "prepared":
        p.a.prepare(3)
        p.b.prepare(3)
    elif history == "sharded":
        comm = bmsp.Comm.loopback(3)
        for gather in (True, False):
            Cs, st, sh = bmsp.spgemm_sharded(comm, p.a, p.b, tc_version=tc, rounds=0, gather=gather)
            assert sh["world"] == 3, sh
            p.check(history + (" gathered" if gather else " owner-keeps"), Cs, st, tc)
        comm.free()
    elif history == "forced_panels":
        with monkeypatch.context() as m:
            m.setenv("BMSP_SPGEMM_FORCE_PANELS", "1")
            p.multiply(history, tc)
    elif history == "user_views":
        bounds = bmsp.partition_rows(p.a, p.b, 3)
        assert np.all(np.diff(bounds) > 0), bounds
        keep, panels, total = [], [], {}
        for i in range(3):
            view = p.a.row_panel(bounds[i], bounds[i + 1])
            Cp, st = bmsp.spgemm(view, p.b, tc_version=tc)
            print(p.pair, p.dtype, history, i, {k: st[k] for k in FIELDS})
            keep.append((view, Cp))
            panels.append(Cp.device_arrays())
            for key in ("task_list_size", "bmp_reduction", "surviving_tasks", "c_blocks", "c_nnz"):
                total[key] = total.get(key, 0) + st[key]
        ref, rst = p.reference(tc)
        compare_with_oracle(bmsp.concat_panels(A[0], B[1], panels), ref, exact_bits_for(p.dtype, tc), total, rst)
    elif history == "switch_off_strip":
        p.multiply(history + " before", tc)        # (a fit is remembered: the switched products must not replace it; other_tc has none to replace)
        for switch, value in (("BMSP_MAC_STRIP", "0"), ("BMSP_SPGEMM_ROWMERGE", "2")):
            with monkeypatch.context() as m:
                m.setenv(switch, value)
                st = p.multiply("%s %s=%s" % (history, switch, value), tc)
                assert st[:2] != (PATH_ROWMERGE, RM_STRIP), st
    else:
        assert history == "none"


def built_for(pair, dtype, tc):
    """rule 4: ((sort_path, sort_long), mac_variant or None) of steady(X) where the pair is built for X, else None"""
    v15 = dtype == F32 or tc == 5          # V15's numerics: fp32 operands, fp16 under tc_version 5
    if pair == "S":                        # (fp16 under tc_version 5 has no structure-only kernel for tiles this full: not built for it)
        return ((PATH_ROWMERGE, RM_STRIP), MAC_STRIP) if dtype == F32 or tc == 4 else None
    if pair == "R":                        # (on the matrix cores the fp16 strip kernel takes the nearly empty tiles)
        return ((PATH_ROWMERGE, RM_STRIP), MAC_ROWSPARSE if v15 else MAC_STRIP)
    if pair == "V":                        # (on the matrix cores the strip kernel's k list refuses A and no structure-only kernel is left)
        return ((PATH_ROWMERGE, RM_STRIP), MAC_ROWSPARSE) if v15 else None
    return ((PATH_ROWMERGE, RM_TASKLIST), None) if pair == "T" else ((PATH_ROWWINDOW, 0), None)


def assert_steady(pair, dtype, tc, steady):
    want = built_for(pair, dtype, tc)
    if want:
        assert steady[:2] == want[0] and want[1] in (None, steady[3]), (steady, want)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tc", [(F32, 5), (F16, 4)])
def test_views_inherit_and_hand_back(oracle, bmsp, monkeypatch, dtype, tc):
    """What test_pair_memory cannot see (rule 3 accepts a first probe that pays for a pass, and the statistics of a sharded product of
    several panels mix the panels'): the sharded product of W on a loopback communicator of ONE, one round -- a single panel, a view of
    the whole A, whose statistics are the call's.  The first call tries the task-list pass and takes the column windows, as a fresh whole
    product does; the second goes straight to the windows only if the view's memory was handed back to the parent (rm_hint_merge) AND
    the next view inherited it (rm_hint_inherit); the parent's own product then needs no attempt either."""
    for k in ALL_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    fresh, steady = base(oracle, bmsp, "W", dtype, tc)
    assert (fresh[:2], steady[:2]) == ((PATH_ROWWINDOW, 1), (PATH_ROWWINDOW, 0)), (fresh, steady)
    p = Pair(oracle, bmsp, "W", dtype)
    comm = bmsp.Comm.loopback(1)
    seen = []
    for i in range(2):
        Cs, st, sh = bmsp.spgemm_sharded(comm, p.a, p.b, tc_version=tc, rounds=1, gather=True)
        assert sh["world"] == 1, sh
        seen.append(p.check("one panel, call %d" % i, Cs, st, tc)[:2])
    comm.free()
    assert seen == [fresh[:2], steady[:2]], seen
    assert p.multiply("whole", tc) == steady


@pytest.mark.gpu
@pytest.mark.parametrize("pair,dtype,tc,history",[pytest.param(*c, id="%s-%s-tc%d-%s" % (c[0], "f16" if c[1] == F16 else "f32", c[2], c[3])) for c in cases()])
def test_pair_memory(oracle, bmsp, monkeypatch, pair, dtype, tc, history):
    """Predicted to fail before the memory kept "does strip mode fit" apart from the list path, and observed to (see the mutation record):
    a product whose arguments or switches exclude strip mode (S-f16-tc4 x other_tc, x switch_off_strip; S-f32-tc5 x switch_off_strip)
    overwrote a remembered strip fit with the task-list mode that ran; a row-panel view that the predicates refuse for being a view
    handed its task-list mode to the parent (V x sharded, x forced_panels under V15's numerics; R-f16-tc5 the same way)."""
    for k in ALL_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    fresh, steady = base(oracle, bmsp, pair, dtype, tc)
    if pair == "W":
        assert fresh[0] == PATH_ROWWINDOW, "inconclusive: the fresh first product of W did not take the column windows: %r" % (fresh,)
    assert_steady(pair, dtype, tc, steady)
    p = Pair(oracle, bmsp, pair, dtype)
    apply_history(p, history, tc, monkeypatch)
    first = p.multiply("probe 1", tc)
    second = p.multiply("probe 2", tc)
    print("fresh_first", fresh, "steady", steady, "first", first, "second", second)
    assert second == steady, (second, steady)
    want = fresh if HISTORIES[history] == "fresh" else steady
    assert first == want, (first, want, HISTORIES[history])
