"""GPU cases of the SpGEMM regime tests: every product of tests/test_spgemm_regimes.py (which holds the thresholds, the generators, the
table of products and the CPU self-checks these cases rest on, and describes them) through bmsp_spgemm under the switches that pin the
path the product is built for, bit for bit against the oracle -- keys, bitmaps, offsets, values and the four stage counters, no tolerance
anywhere -- and every case asserts the path it is meant to run from sort_path, sort_long and mac_variant.

The file is named to be collected last: every GPU test that was there before it keeps its place in the order of the suite."""
import numpy as np
import pytest
from test_gpu_parity import check_spgemm
from test_spgemm_regimes import (NARROW_CAP, WIDE_CAP, BLOCK_SEG_MAX, TASK_BLOCK_IDX_BITS, STRIP_ROW_CAP, RS_TABLE, TL_CAP, product, product_terms, jbits_of,
                                 tiny_product)

_SWITCHES = ("BMSP_SPGEMM_ROWMERGE", "BMSP_SPGEMM_ROWWINDOW", "BMSP_SEGSORT_WIDE", "BMSP_SEGSORT_READBACK", "BMSP_SEGSORT_RADIX", "BMSP_SEGSORT_NO_MERGE",
             "BMSP_SEG_AVG_MAX", "BMSP_MAC_ROWSPARSE", "BMSP_MAC_STRIP", "BMSP_MAC_OLD", "BMSP_MAC_VALU_DENSE", "BMSP_MAC_F32MFMA", "BMSP_RM_BUILD_WAVE",
             "BMSP_RM_DEPTH1", "BMSP_EXPAND_LOOKBACK", "BMSP_STRIP_PROF", "BMSP_WIN_CAND", "BMSP_WIN_CAND_HASH", "BMSP_WIN_THIN")
F32_V15, F16_V15, F16_MFMA = (0, 5), (1, 5), (1, 4)


def run(oracle, bmsp, monkeypatch, name, env, numerics=F32_V15, mode=0):
    """one product under exactly these switches, bit for bit against the oracle; returns the statistics"""
    dtype, tc = numerics
    with monkeypatch.context() as m:
        for k in _SWITCHES:
            m.delenv(k, raising=False)
        for k, v in env.items():
            m.setenv(k, v)
        A, B, _ = product(name, numerics == F16_MFMA)
        st = check_spgemm(oracle, bmsp, A, B, dtype, mode, tc, exact_expected=True)
    print(name, env, numerics, {k: st[k] for k in ("sort_path", "sort_long", "mac_variant", "mac_kernel")})
    return st


def sort_env(wide=False, readback=False, radix=None):
    env = {"BMSP_SPGEMM_ROWMERGE": "0", "BMSP_MAC_ROWSPARSE": "0"}    # T_5 of the pipeline; a block-MAC kernel that reads the task list
    if wide:
        env["BMSP_SEGSORT_WIDE"] = "1"
    if readback:
        env["BMSP_SEGSORT_READBACK"] = "1"
    if radix is not None:
        env["BMSP_SEGSORT_RADIX"] = str(radix)
    return env


def takes_direct_kernel(name, wide):
    """the dispatcher's own condition (segsort_tasks_by_column), from the operands"""
    A, B, _ = product(name)
    t = product_terms(A, B)
    narrow = jbits_of(B) + TASK_BLOCK_IDX_BITS <= 32 and not wide
    return 0 < t["max_a"] * t["max_b"] <= (NARROW_CAP if narrow else WIDE_CAP)


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("route", ["direct", "readback"])
def test_a1_every_register_network(oracle, bmsp, monkeypatch, route, wide):
    """A1: segments of 1 .. 2048 tasks at both sides of every network size (128 .. 2048 words), 32- and 64-bit sort words, the
    read-back-free kernel and the list kernels"""
    assert takes_direct_kernel("a1", wide)          # ... unless it is pinned to the other side:
    env = sort_env(wide, route == "readback")
    for numerics in (F32_V15, F16_V15, F16_MFMA) if not wide else (F32_V15,):
        st = run(oracle, bmsp, monkeypatch, "a1", env, numerics, mode=1)
        assert st["sort_path"] == 1 and st["sort_long"] == 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["direct", "readback"])
@pytest.mark.parametrize("name", ["a1_upper", "a1_sentinel"])
def test_a1_wave_capacity_narrow(oracle, bmsp, monkeypatch, name, route):
    """A1: 2049, 4095 and 4096 tasks in 32-bit words (64 words per lane), the bound exactly 4096; `a1_sentinel`: B of exactly 2^20 block
    columns -- the word of the 4096th task, at block column 2^20 - 1, equals the network's padding value"""
    assert takes_direct_kernel(name, False)
    st = run(oracle, bmsp, monkeypatch, name, sort_env(False, route == "readback"), mode=1)
    assert st["sort_path"] == 1 and st["sort_long"] == 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("name,wide", [("a1_upper", True), ("a1_real_wide", False)])
def test_a1_workgroup_kernel_wide(oracle, bmsp, monkeypatch, name, wide):
    """A1: 2049 .. 4096 tasks in 64-bit words -- the only way into segsort_tasks_block_kernel -- forced, and with 2^20 + 1 block columns,
    where the width is real"""
    assert not takes_direct_kernel(name, wide)      # the bound 4096 exceeds the wide capacity: the list kernels without a switch
    for env in (sort_env(wide, True), sort_env(wide, False)):
        st = run(oracle, bmsp, monkeypatch, name, env, mode=1)
        assert st["sort_path"] == 1 and st["sort_long"] == 0, st
    st = run(oracle, bmsp, monkeypatch, name, sort_env(wide, True), F16_V15, mode=1)
    assert st["sort_path"] == 1 and st["sort_long"] == 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a1_bound_4097", "a1_refusal"])
def test_a1_bound_beyond_the_wave(oracle, bmsp, monkeypatch, name):
    """A1, refusal edge: the bound from the operands is 4097 (and far more) while no segment exceeds 4096 -- the read-back-free kernel must not
    be taken (nothing tells it from the list kernels in the statistics: the condition is asserted from the operands), the result is right"""
    assert not takes_direct_kernel(name, False)
    st = run(oracle, bmsp, monkeypatch, name, sort_env(), mode=1)
    assert st["sort_path"] == 1 and st["sort_long"] == 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a2", "a2_all_long_odd", "a2_mixed_odd", "a2_mixed_even"])
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_a2_pieces_and_merge_passes(oracle, bmsp, monkeypatch, wide, name):
    """A2 (BMSP_SEGSORT_RADIX=0): segments of 4097 .. 16384 tasks (wide: half of that) -- two, three and four pieces at both sides of every
    piece count, short segments around them; every segment long and one pass (the scratch pair is handed back); a mixed list with one
    pass (the copy-back launch) and with two"""
    name = name + ("_half" if wide else "")
    env = sort_env(wide, radix=0)
    for numerics in (F32_V15, F16_V15, F16_MFMA) if name == "a2" else (F32_V15,):
        st = run(oracle, bmsp, monkeypatch, name, env, numerics, mode=1)
        assert st["sort_path"] == 1 and st["sort_long"] == 1, st


@pytest.mark.gpu
@pytest.mark.parametrize("name,wide,long_mode", [("a3_16384", False, 1), ("a3_16385", False, 2), ("a3_8192", True, 1), ("a3_8193", True, 2)])
def test_a3_merge_or_counting_by_default(oracle, bmsp, monkeypatch, name, wide, long_mode):
    """A3: without a switch, a longest segment of four pieces stays with the merge passes, one task more takes the counting passes"""
    st = run(oracle, bmsp, monkeypatch, name, sort_env(wide), mode=1)
    assert st["sort_path"] == 1 and st["sort_long"] == long_mode, st


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a3_pass1", "a3_pass2_lo", "a3_pass2_hi", "a3_pass3_lo", "a3_pass3_hi", "a3_pass3_top"])
def test_a3_counting_passes(oracle, bmsp, monkeypatch, name):
    """A3 (BMSP_SEGSORT_RADIX=1): the A2 lengths on tiles of 4096 (4097 = a full tile and one element) with one, two and three counting
    passes, at both ends of each pass count's range of column bits; with an odd number the sorted keys end in the other array and the
    segments of one task are carried over by CopyLoneKeys"""
    for numerics in (F32_V15, F16_V15, F16_MFMA) if name == "a3_pass1" else (F32_V15,):
        st = run(oracle, bmsp, monkeypatch, name, sort_env(radix=1), numerics, mode=1)
        assert st["sort_path"] == 1 and st["sort_long"] == 2, st


_STRIP_RUNS = [({}, F32_V15, 5), ({"BMSP_MAC_ROWSPARSE": "0"}, F32_V15, 3), ({}, F16_MFMA, 3)]   # (switches, numerics, mac_variant in strip mode)


@pytest.mark.gpu
@pytest.mark.parametrize("pool", ["all", "wrap"])
@pytest.mark.parametrize("c", [255, 256, 257])
def test_b_strip_mode_row_cap(oracle, bmsp, monkeypatch, c, pool):
    """B: a block-row of C of 255, 256 and 257 tiles next to ordinary ones, from any columns and from columns whose probes wrap around the
    512-slot table: strip mode up to 256, task-list mode beyond"""
    for env, numerics, variant in _STRIP_RUNS:
        st = run(oracle, bmsp, monkeypatch, "b_%d_%s" % (c, pool), dict(env, BMSP_SPGEMM_ROWMERGE="1"), numerics)
        if c <= STRIP_ROW_CAP:
            assert (st["sort_path"], st["sort_long"], st["mac_variant"]) == (2, 1, variant), st
        else:
            assert (st["sort_path"], st["sort_long"]) == (2, 2), st


@pytest.mark.gpu
@pytest.mark.parametrize("name,strip", [("b_last_step", False), ("b_duplicates", True), ("b_brow_256", True), ("b_brow_257", False)])
def test_b_strip_mode_walks_and_refusal(oracle, bmsp, monkeypatch, name, strip):
    """B: the last step of the walk carries the count from 250 to 257; 256 columns and then a dozen steps of duplicates; a block-row of B of
    256 and of 257 tiles that no A tile meets (the early refusal; with 256 the pass runs without T_2)"""
    for env, numerics, variant in _STRIP_RUNS:
        st = run(oracle, bmsp, monkeypatch, name, dict(env, BMSP_SPGEMM_ROWMERGE="1"), numerics)
        if strip:
            assert (st["sort_path"], st["sort_long"], st["mac_variant"]) == (2, 1, variant), st
        else:
            assert (st["sort_path"], st["sort_long"]) == (2, 2), st


@pytest.mark.gpu
def test_b_strip_kernel_lists(oracle, bmsp, monkeypatch):
    """B: kJCap -- two neighbouring block-rows of 256 C tiles on disjoint columns (512 merged: fits), and 256 + 257 reached through an explicit
    mode (the strip kernel refuses C); kKCap -- 96 + 96 A tiles in a strip (the strip kernel), 96 + 97 (not)"""
    for env, numerics, variant in _STRIP_RUNS[1:]:
        st = run(oracle, bmsp, monkeypatch, "b_jcap_512", dict(env, BMSP_SPGEMM_ROWMERGE="1"), numerics)
        assert (st["sort_path"], st["sort_long"], st["mac_variant"]) == (2, 1, 3), st
        st = run(oracle, bmsp, monkeypatch, "b_kcap_192", dict(env, BMSP_SPGEMM_ROWMERGE="1"), numerics)
        assert (st["sort_path"], st["sort_long"], st["mac_variant"]) == (2, 1, 3), st
        st = run(oracle, bmsp, monkeypatch, "b_kcap_193", dict(env, BMSP_SPGEMM_ROWMERGE="1"), numerics)
        assert (st["sort_path"], st["sort_long"]) == (2, 2) and st["mac_variant"] != 3, st
    pipeline = {"BMSP_SPGEMM_ROWMERGE": "0", "BMSP_MAC_STRIP": "1"}
    st = run(oracle, bmsp, monkeypatch, "b_jcap_512", pipeline, F16_MFMA, mode=1)
    assert st["sort_path"] == 1 and st["mac_variant"] == 3, st
    st = run(oracle, bmsp, monkeypatch, "b_jcap_513", pipeline, F16_MFMA, mode=1)
    assert st["sort_path"] == 1 and st["mac_variant"] in (1, 2), st


@pytest.mark.gpu
@pytest.mark.parametrize("c", [767, 768, 769])
def test_b_rowsparse_table(oracle, bmsp, monkeypatch, c):
    """B: block-rows of C of 767, 768 and 769 tiles through task-list mode (no switch): the row-sparse kernel up to its table's 768"""
    for numerics in (F32_V15, F16_V15):
        st = run(oracle, bmsp, monkeypatch, "b_rs_%d" % c, {}, numerics)
        assert (st["sort_path"], st["sort_long"]) == (2, 2) and (st["mac_variant"] == 5) == (c <= RS_TABLE), st


def _tasklist_env(form):
    env = {"BMSP_SPGEMM_ROWMERGE": "2", "BMSP_MAC_STRIP": "0", "BMSP_MAC_ROWSPARSE": "0"}
    if form == "wave":
        env["BMSP_RM_BUILD_WAVE"] = "1"
    return env


def pipeline_path(name):
    """(sort_path, sort_long) of the expand - sort - compress pipeline under BMSP_SORT_AUTO, from the operands: the segmented sort from an
    average of four tasks per block-row of A on; no long segment, pieces + merge passes up to four pieces, counting passes beyond"""
    A, B, _ = product(name)
    t = product_terms(A, B)
    cap = NARROW_CAP if jbits_of(B) + TASK_BLOCK_IDX_BITS <= 32 else WIDE_CAP
    longest = int(np.bincount(t["seg"]).max())
    assert t["seg"].size // (A[0] // 8) >= 4
    return 1, (0 if longest <= max(cap, BLOCK_SEG_MAX) else (1 if longest <= 4 * cap else 2))


def _tasklist_case(oracle, bmsp, monkeypatch, name, form, fits):
    """task-list mode when the block-rows fit.  Otherwise three products in a row (the workgroup build's overflow is a matter of timing
    between four waves) that leave it for the window passes, taken after the task-list pass was tried (sort_path 3, sort_long 1): B has
    fewer than 2^20 block columns, and a block-row that overflows the task-list pass brings hundreds of candidate pairs per window, far
    above the sixteen per table entry below which rowmerge_windowed declines.  With the window passes switched off: the pipeline's
    segmented sort, with the long-segment form the longest block-row calls for (pipeline_path)"""
    env = _tasklist_env(form)
    for numerics in (F32_V15, F16_V15, F16_MFMA):
        if fits:
            st = run(oracle, bmsp, monkeypatch, name, env, numerics)
            assert (st["sort_path"], st["sort_long"]) == (2, 2), st
            continue
        for _ in range(3):
            st = run(oracle, bmsp, monkeypatch, name, env, numerics)
            assert (st["sort_path"], st["sort_long"]) == (3, 1), st
        st = run(oracle, bmsp, monkeypatch, name, dict(env, BMSP_SPGEMM_ROWWINDOW="0"), numerics)
        assert (st["sort_path"], st["sort_long"]) == pipeline_path(name), st


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["workgroup", "wave"])
@pytest.mark.parametrize("pool", ["all", "wrap"])
@pytest.mark.parametrize("c", [895, 896, 897])
def test_c_task_list_row_cap(oracle, bmsp, monkeypatch, c, pool, form):
    """C: a block-row of C of 895, 896 and 897 tiles, from any columns and from columns whose probes wrap around the 1024-slot table"""
    _tasklist_case(oracle, bmsp, monkeypatch, "c_%d_%s" % (c, pool), form, c <= TL_CAP)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["workgroup", "wave"])
@pytest.mark.parametrize("name,fits", [("c_tasks_65471", True), ("c_tasks_65472", False), ("c_brow_959", True), ("c_brow_960", False)])
def test_c_task_list_offsets_and_refusal(oracle, bmsp, monkeypatch, name, fits, form):
    """C: 16-bit task offsets -- a block-row of 512 C tiles with 65 471 surviving pairs stays in task-list mode, with 65 472 it does not
    (before this case existed the bound was looked at only when a further step of the walk followed: the one-wave form accepted up to
    65 535 pairs depending on where the steps fell, the workgroup form always; the C was right either way); the early refusal -- a
    block-row of B of 959 and of 960 tiles that no A tile meets"""
    _tasklist_case(oracle, bmsp, monkeypatch, name, form, fits)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["d_exact", "d_plus_one"])
def test_d_expansion_tile(oracle, bmsp, monkeypatch, name):
    """D: exactly 2 << 20 candidate pairs (the small expansion tile) and one more (the large one)"""
    st = run(oracle, bmsp, monkeypatch, name, sort_env(), mode=1)
    assert st["sort_path"] == 1 and st["task_list_size"] == product(name)[2], st


# name -> (operands of tiny_product, (dtype, tc_version), switches, B adopted with ownership 2, (mac_kernel, mac_variants allowed))
_ONE_ANSWER = {
    "f32_rowsparse": ("sparse", F32_V15, {}, False, (5, (5,))),
    "f32_strip": ("sparse", F32_V15, {"BMSP_MAC_ROWSPARSE": "0"}, False, (5, (3,))),
    "f32_tiny_values": ("tiny", F32_V15, {}, False, (5, (0,))),                      # products below 2^-126: the vector-ALU kernel
    "f16_strip": ("full", F16_MFMA, {}, False, (4, (3,))),
    "f16_k32_tasklist": ("full", F16_MFMA, {"BMSP_SPGEMM_ROWMERGE": "0"}, False, (4, (1, 2))),
    "f16_k16": ("full", (1, 1), {}, False, (1, (0,))),
    "f16_v15_rowsparse": ("sparse", F16_V15, {}, False, (5, (5,))),
    "f64_valu": ("sparse", (2, 5), {}, False, (5, (0,))),
    "f32_mfma_tasklist": ("full", F32_V15, {"BMSP_MAC_F32MFMA": "1"}, False, (5, (4,))),
    "f32_adopted_b": ("sparse", F32_V15, {}, True, (5, (3,))),                       # no CSR copy of adopted arrays: never the row-sparse kernel
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(_ONE_ANSWER))
def test_three_callers_one_answer(oracle, bmsp, monkeypatch, case):
    """the block-MAC kernel is decided in one place (csrc/mac_choice.h): bmsp_spgemm, bmsp_spgemm_symbolic + bmsp_spgemm_numeric, and
    bmsp_spgemm after bmsp_matrix_prepare(SPGEMM) on both operands -- each on handles of its own -- report the same mac_kernel and
    mac_variant, the expected one, and store the oracle's values bit for bit (every sum of these operands is exact in fp32 in any order,
    so the matrix cores' numerics have one answer too).  What prepare builds for an adopted operand is pinned by the host check of the
    rule (tests/host_mac_choice_check.cpp): the handle does not show its cached forms."""
    kind, (dtype, tc), env, adopt_b, (kernel, variants) = _ONE_ANSWER[case]
    A, B = tiny_product(kind)
    ref, rst = oracle.spgemm(oracle.bmsp_from_coo(oracle.Coo(*A), dtype, False), oracle.bmsp_from_coo(oracle.Coo(*B), dtype, True), exact_products=(dtype == 1 and tc != 5))
    keep = []

    def operands():
        a, b = bmsp.BmSpMatrix.from_coo(*A, transposed=False, dtype=dtype), bmsp.BmSpMatrix.from_coo(*B, transposed=True, dtype=dtype)
        if adopt_b:
            keep.append(b)
            b = bmsp.BmSpMatrix.from_device_arrays(B[0], B[1], *b.device_arrays(), dtype=dtype, transposed=True)
        return a, b

    with monkeypatch.context() as m:
        for k in _SWITCHES + ("BMSP_MAC_B_DENSE", "BMSP_MAC_DIRECT"):
            m.delenv(k, raising=False)
        for k, v in env.items():
            m.setenv(k, v)
        a, b = operands()
        whole = bmsp.spgemm(a, b, tc_version=tc)
        a, b = operands()
        split, _ = bmsp.spgemm_symbolic(a, b, tc_version=tc)
        split = (split, bmsp.spgemm_numeric(a, b, split, tc_version=tc))
        a, b = operands()
        a.prepare(2)
        b.prepare(2)
        prepared = bmsp.spgemm(a, b, tc_version=tc)
    answers = []
    for what, (Cm, st) in (("bmsp_spgemm", whole), ("symbolic + numeric", split), ("prepare + bmsp_spgemm", prepared)):
        print(case, what, {k: st[k] for k in ("sort_path", "sort_long", "mac_variant", "mac_kernel")})
        k, bm, o, v = Cm.host_arrays()
        np.testing.assert_array_equal(k, ref.keys)
        np.testing.assert_array_equal(bm, ref.bmps)
        np.testing.assert_array_equal(o, ref.offsets)
        np.testing.assert_array_equal(v.astype(np.float64), ref.values, err_msg=what)
        answers.append((st["mac_kernel"], st["mac_variant"]))
    assert answers[0] == answers[1] == answers[2], answers
    assert answers[0][0] == kernel and answers[0][1] in variants, answers
    assert rst["surviving_tasks"] == 512 and whole[1]["surviving_tasks"] == 512 and whole[1]["c_nnz"] == ref.nnz
