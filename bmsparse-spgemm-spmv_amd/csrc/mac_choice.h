// mac_choice.h -- which block multiply-accumulate kernel (T_7) a product takes: the whole rule, as a pure function of plain facts.
//
// No HIP and no handle types: the gatherer (mac_choice.hip: mac_decide; builder.hip: prepare_spgemm_operand) copies what the rule reads out of the handles
// into MacFacts, and tests/host_mac_choice_check.cpp builds MacFacts by hand.  A new kernel's rule goes into mac_choose (and, where it
// reads another cached operand form, into mac_prepare_forms) and nowhere else.
//
// Laziness.  Three kinds of fact cost a kernel and a read-back the first time they are asked for: a matrix's row maxima, its value
// figures ("every stored value is finite", the fp32 exponent range: two reductions) and the two process-wide self-tests of the fp32 MFMA.
// They enter MacFacts as "not known yet" (-1), the rule reads its facts in a fixed order -- free tests first -- and when it reaches one
// that is not known it stops and names it (MacChoice::need).  The gatherer fetches exactly that fact and asks again, so a product pays
// for a figure only while a kernel that needs it is still a candidate.
#ifndef BMSP_MAC_CHOICE_H_
#define BMSP_MAC_CHOICE_H_

#include <cstdint>

namespace bmsp {

// ---- kernel capacities the rule reads -------------------------------------------------------------------------------------------------
constexpr int kKCap = 192;  // strip kernels (blockmac_strip.hip): merged A tiles of a strip (two block-rows)
constexpr int kJCap = 512;  // ... and merged C tiles of a strip
// strip mode's bound on a block-row of C: two block-rows of at most this many tiles always fit a strip's column list
constexpr uint32_t mac_strip_row_cap() { return (uint32_t)kJCap / 2u; }
// row-sparse kernel (blockmac_rowsparse.hip): the table of a block-row's C columns has 2^hb slots.  hb = 9 for at most 256 tiles (strip
// mode's bound) or 10 for at most 768 (products that come with a task list)
constexpr uint32_t rs_row_cap(int hb) { return hb == 9 ? 256u : 768u; }
static_assert(mac_strip_row_cap() <= rs_row_cap(10), "a block-row of C that strip mode accepts must fit the row-sparse kernel's larger table");
// the row-sparse kernel's CSR copy counts a block-row's values per matrix row in 16-bit fields (8 values per tile and row): a block-row of
// this many tiles or more has no such copy -- the rule asks first, ensure_csr32 refuses
constexpr int64_t kRsRowBlocksEnd = 1 << 13;
constexpr int64_t kRsFillMax = 16;       // row-sparse: stored values per tile, on average, per operand
constexpr int kF32ExpSumMax = 254 + 100;  // fp32 matrix pipe: largest sum of the operands' largest biased exponents (every sum far from overflow)
constexpr int kRsExpSumMin = 128;        // row-sparse, fp32: every product of stored values a normal number (2^(ea + eb - 254) >= 2^-126)

// value types and bmsp_spgemm_stats::mac_variant values, as include/bmsp.h numbers them (asserted where both are visible: mac_choice.hip)
enum : int { kMacF32 = 0, kMacF16 = 1, kMacF64 = 2 };
enum : int { kMacVariantDefault = 0, kMacVariantStaged = 1, kMacVariantDirect = 2, kMacVariantStrip = 3, kMacVariantF32Mfma = 4, kMacVariantRowSparse = 5 };

// cached operand forms a launch reads (MacChoice::a_forms / b_forms, mac_prepare_forms)
enum : unsigned { kMacFormCsr = 1u, kMacFormDenseTiles = 2u, kMacFormLaneTiles = 4u, kMacFormBlockMeta = 8u };

struct MacOperand {
    int dtype = kMacF32;
    int64_t nnz = 0, block_num = 0, values_extent = 0, num_block_rows = 0;
    int64_t max_row_blocks = -1;  // most tiles in a block-row; -1: not computed yet
    bool pool_owned = true;       // the value array comes from the library's allocator (read slack behind the last value)
    bool borrowed = false;        // ownership 2: adopted arrays, row-panel views
    bool view = false;            // a row-panel view (values addressed inside the parent's array)
    int values_finite = -1;       // 1 no inf / NaN stored, 0 some, -1 not looked yet; with it, for fp32, the biased exponent range of the
    int f32_exp_min = 255, f32_exp_max = 0;  // non-zero stored values
};

// The switches that steer the choice, read once per call (mac_switch: -1 unset, 0 "0", 1 "1", 2 anything else).  BMSP_MAC_STRIP 0 / 1:
// never a strip-mode kernel / the strip kernel whatever the task counts say (the capacities hold); _ROWSPARSE 0 / 1: never / whatever
// the fill; _VALU_DENSE set: the vector-ALU kernel for V15 numerics, 1 = staged from dense copies, else element gathers; _F32MFMA set
// (fp32 operands): no structure-only kernel, 1 = the fp32 MFMA task-list kernel, else the vector-ALU one; _OLD set: the K = 16 kernels
// under tc_version 4; _B_DENSE / _DIRECT 0 / 1: the K = 32 kernel's B form and staging; BMSP_STRIP_PROF set: the strip kernels' timing
// build, so not the row-sparse kernel in strip mode.
struct MacSwitches {
    int8_t strip = -1, rowsparse = -1, valu_dense = -1, f32mfma = -1, old = -1, b_dense = -1, direct = -1, strip_prof = -1;
};
inline int8_t mac_switch(const char *v) { return !v ? -1 : (v[0] == '0' ? 0 : (v[0] == '1' ? 1 : 2)); }

struct MacFacts {
    MacOperand a, b;
    int tc_version = 5;
    bool has_c = false;  // C's structure exists (otherwise the question is strip mode's: is there a kernel that will need C's structure only?)
    int64_t c_block_num = 0, c_max_row_blocks = -1;
    bool has_tasks = false;  // a sorted task list exists (the caller prefers it: bmsp_spgemm past strip mode, or strip mode switched off)
    uint64_t n_tasks = 0, candidates = 0;
    int f32_chain_ok = -1;   // process: v_mfma_f32_16x16x4_f32 is the k-ascending fmaf chain on this device (-1: self-test not run yet)
    int f32_exp_floor = -1;  // process: smallest sum of the operands' smallest biased exponents the fp32 matrix pipe takes (-1: not run yet)
    MacSwitches sw;
};

enum class MacPath {
    None,          // no structure-only kernel: the caller forms a task list (or, with one, never returned)
    RowSparse,     // blockmac_rowsparse.hip: CSR copies, C's structure
    StripF16,      // blockmac_strip.hip: dense tiles, C's structure
    StripF32,      // ... lane tiles
    Mfma32Staged,  // blockmac32.hip: A dense tiles, B dense tiles or block records, task list
    Mfma32Direct,  // ... both dense
    Mfma16Group,   // spgemm.hip: block records, task list
    Mfma16,        // ... the four arrays
    F32Mfma,       // blockmac_f32.hip: lane tiles, task list
    ValuDense,     // spgemm.hip launch_mac_valu: block records + dense tiles
    ValuGather,    // ... block records
    ValuPointer,   // ... the four arrays (values beyond 4 GiB)
};
enum class MacNeed { None, RowStatsA, RowStatsB, RowStatsC, Finite, F32Chain, F32ExpFloor };

struct MacChoice {
    MacPath path = MacPath::None;
    MacNeed need = MacNeed::None;  // not None: `path` is not decided yet -- fetch this fact and ask again
    int mac_kernel = 0, mac_variant = 0;  // as bmsp_spgemm_stats reports them
    const char *name = "none";
    unsigned a_forms = 0, b_forms = 0;  // kMacForm*: what the launch reads of A and of B beside the four arrays
};

// ---- the per-operand halves, written once ---------------------------------------------------------------------------------------------
// addressing: tiles, records and values behind the 32-bit byte offsets of a buffer descriptor
inline bool mac_dense_f16_addressable(const MacOperand &m) { return m.block_num < (1ll << 25); }   // 128-byte tiles
inline bool mac_lane_tiles_addressable(const MacOperand &m) { return m.block_num < (1ll << 24); }  // 256-byte tiles
inline bool mac_records_addressable(const MacOperand &m) { return m.block_num < (1ll << 28); }     // 16-byte records
inline bool mac_values_addressable(const MacOperand &m, int elem_bytes, int slack) { return (uint64_t)m.values_extent * (uint64_t)elem_bytes + (uint64_t)slack < (1ull << 32); }
inline bool mac_copy_within_4g(const MacOperand &m, int tile_bytes) { return (uint64_t)m.block_num * (uint64_t)tile_bytes <= (4ull << 30); }

// Row-sparse kernel, per operand: at most kRsFillMax stored values per tile on average (BMSP_MAC_ROWSPARSE=1: whatever the fill), 8-byte
// entries behind 32-bit byte offsets, a CSR copy of its own (no view, no adopted arrays), every block-row below kRsRowBlocksEnd tiles.
// 1 yes, 0 no, -1 the row maxima are needed first (asked once the tests before them have passed).
inline bool mac_rowsparse_operand_before_rows(const MacOperand &m, const MacSwitches &sw)
{
    return sw.rowsparse != 0 && m.nnz < (1ll << 29) && !m.view && !m.borrowed;
}
inline int mac_rowsparse_operand(const MacOperand &m, const MacSwitches &sw)
{
    if (!mac_rowsparse_operand_before_rows(m, sw)) return 0;
    if (m.max_row_blocks < 0) return -1;
    if (m.max_row_blocks >= kRsRowBlocksEnd) return 0;
    return (sw.rowsparse == 1 || m.nnz <= kRsFillMax * m.block_num) ? 1 : 0;
}
// fp32 exponent window of a pair (value figures known): every product of stored values at least 2^(floor - 254), every sum far from overflow
inline bool mac_f32_exp_min_ok(const MacOperand &a, const MacOperand &b, int floor) { return a.f32_exp_min + b.f32_exp_min >= floor; }
inline bool mac_f32_window_ok(const MacOperand &a, const MacOperand &b, int floor)
{
    return mac_f32_exp_min_ok(a, b, floor) && a.f32_exp_max + b.f32_exp_max <= kF32ExpSumMax;
}
// Vector-ALU kernel, per operand: staged from a dense copy when the tiles are at least a quarter full (fp32: the copy is then <= 4x the
// values; FEM-like 3.7 values per tile: 17x the memory for -10 % of T_7, not taken; fp16 copies exist anyway) and the copy stays within 4 GiB
inline bool mac_valu_dense_operand(const MacOperand &m)
{
    if (m.dtype == kMacF16) return mac_copy_within_4g(m, 128);
    return m.dtype == kMacF32 && m.nnz >= 16 * m.block_num && mac_copy_within_4g(m, 256);
}
// K = 32 MFMA kernel: which form B takes.  Measured (block-MAC log): the dense copy wins on every generator case -- the kernel
// is bound by instruction issue and LDS traffic, not by bytes, and the dense line needs no block record and no nibble decode (cage-like
// 421 vs 468 us, R-MAT 2^16 2.58 vs 2.91 ms, full tiles 72 vs 84 us) -- at 128 B per block of extra memory and ~2x the L2 miss traffic.
// So: dense unless the copy would be large (> 4 GiB) and the tiles are sparse, or BMSP_MAC_B_DENSE says otherwise; always dense when the
// value array is borrowed without the read slack the 12-byte nibble loads need.
inline bool mac_mfma32_b_dense(const MacOperand &b, const MacSwitches &sw)
{
    if (sw.b_dense >= 0) return sw.b_dense == 1;
    if (!b.pool_owned) return true;
    const bool full_tiles = b.block_num && (double)b.nnz / (double)b.block_num >= 32.0;
    return full_tiles || mac_copy_within_4g(b, 128);
}

// ---- the rule ---------------------------------------------------------------------------------------------------------------------------
namespace mac_detail {
struct Eval {
    const MacFacts &f;
    MacNeed need = MacNeed::None;
    // a fact that costs a launch the first time: false (and the first such fact recorded) while it is not known
    bool known(bool have, MacNeed n)
    {
        if (!have && need == MacNeed::None) need = n;
        return have && need == MacNeed::None;
    }
    bool rows_a() { return known(f.a.max_row_blocks >= 0, MacNeed::RowStatsA); }
    bool rows_c() { return known(f.c_max_row_blocks >= 0, MacNeed::RowStatsC); }
    bool figures() { return known(f.a.values_finite >= 0 && f.b.values_finite >= 0, MacNeed::Finite); }
    bool finite() { return figures() && f.a.values_finite == 1 && f.b.values_finite == 1; }
    bool f32_chain() { return known(f.f32_chain_ok >= 0, MacNeed::F32Chain) && f.f32_chain_ok == 1; }
    // the fp32 matrix pipe reproduces the fmaf chain bit for bit only while no product underflows and no sum overflows: the figures of both
    // operands, then the floor the device's self-test sets
    bool f32_window() { return figures() && known(f.f32_exp_floor >= 0, MacNeed::F32ExpFloor) && mac_f32_window_ok(f.a, f.b, f.f32_exp_floor); }
    bool v15() const { return f.a.dtype == kMacF32 || (f.a.dtype == kMacF16 && f.tc_version == 5); }
    // the switches that send V15 numerics to a task-list kernel
    bool v15_forced_to_tasks() const { return f.sw.valu_dense >= 0 || (f.a.dtype == kMacF32 && f.sw.f32mfma >= 0); }

    // operands of nearly empty tiles whose product takes V15's numerics: the scalar products that exist are a few per cent of what a
    // tile-by-tile kernel multiplies.  Finite values and, for fp32, every product of stored values a normal number
    bool rowsparse()
    {
        if (f.a.dtype != f.b.dtype || !v15()) return false;
        if (!mac_rowsparse_operand_before_rows(f.a, f.sw) || !mac_rowsparse_operand_before_rows(f.b, f.sw)) return false;
        if (!rows_a() || !known(f.b.max_row_blocks >= 0, MacNeed::RowStatsB)) return false;
        if (mac_rowsparse_operand(f.a, f.sw) != 1 || mac_rowsparse_operand(f.b, f.sw) != 1 || !finite()) return false;
        return f.a.dtype != kMacF32 || mac_f32_exp_min_ok(f.a, f.b, kRsExpSumMin);
    }
    bool mfma32_supported() const
    {
        return f.a.dtype == kMacF16 && mac_dense_f16_addressable(f.a) && mac_dense_f16_addressable(f.b) && mac_values_addressable(f.b, 2, 16);
    }
    // what the strip kernels need of the operands alone: tiles they address, a strip's merged A tiles within the k list, finite values
    // (a skipped candidate pair must contribute an exact zero)
    bool strip_operands()
    {
        if (f.a.dtype == kMacF16) {
            if (!mfma32_supported()) return false;
        } else if (f.a.dtype == kMacF32) {
            if (f.b.dtype != kMacF32 || !mac_lane_tiles_addressable(f.a) || !mac_lane_tiles_addressable(f.b) || !f32_chain()) return false;
            if (!f32_window()) return false;
        } else {
            return false;
        }
        if (f.a.num_block_rows >= (1ll << 31) || !rows_a() || 2 * f.a.max_row_blocks > kKCap) return false;
        return finite();
    }
    bool fits_c(int64_t row_cap) { return f.c_block_num < (1ll << 31) && f.c_block_num != 0 && rows_c() && f.c_max_row_blocks <= row_cap; }

    // strip mode: the kernels that work from C's structure alone.  fp16 under tc_version 4: the K = 32 strip kernel (the matrix cores'
    // numerics); V15 numerics (fp32, or fp16 under tc_version 5): the row-sparse kernel, else for fp32 the fp32 strip kernel (V15's
    // summation order on v_mfma_f32_16x16x4_f32)
    MacPath structure()
    {
        if (f.sw.strip == 0) return MacPath::None;
        if (f.a.dtype == kMacF16 && f.tc_version == 4) return f.sw.old < 0 && strip_operands() ? MacPath::StripF16 : MacPath::None;
        if (!v15() || v15_forced_to_tasks()) return MacPath::None;
        if (f.sw.strip_prof < 0 && rowsparse()) return MacPath::RowSparse;
        return f.a.dtype == kMacF32 && strip_operands() ? MacPath::StripF32 : MacPath::None;
    }
    // The strip kernel against the task-list kernels.  Its walk visits every candidate pair and pays a fixed price per (window, k-group)
    // item: it wins where items are fat -- C tiles that collect many tasks from candidate pairs that nearly all survive (dense-tile
    // ceiling: 32.8 tasks per C tile, 840 us against 1430 us for the direct kernel).  On the FEM-like product (14 tasks per C tile, 61 %
    // of the pairs survive, 3 MFMAs per item) the direct kernel stays ahead (530 vs 640 us), so the bar sits between the two.
    bool strip_beats_tasks()
    {
        if (f.sw.strip == 0) return false;
        if (f.sw.strip < 0 && (f.n_tasks < 20 * (uint64_t)f.c_block_num || 10 * f.n_tasks < 9 * f.candidates)) return false;
        return fits_c(kJCap / 2) && strip_operands();
    }
    MacPath with_tasks()
    {
        if (f.a.dtype == kMacF16 && f.tc_version != 5) {
            if (f.tc_version == 4 && f.sw.old < 0 && mfma32_supported()) {
                if (strip_beats_tasks()) return MacPath::StripF16;
                // >= 4.6 tasks per C tile: the direct kernel (no LDS); sparser task lists keep the staged one
                const bool direct = mac_mfma32_b_dense(f.b, f.sw) && (f.sw.direct >= 0 ? f.sw.direct == 1 : 10 * f.n_tasks >= 46 * (uint64_t)f.c_block_num);
                return direct ? MacPath::Mfma32Direct : MacPath::Mfma32Staged;
            }
            // the group kernel's 12-byte value loads may run past the last stored value: arrays from the library's allocator carry that slack
            const bool group = f.tc_version == 4 && f.a.pool_owned && f.b.pool_owned && mac_records_addressable(f.a) && mac_records_addressable(f.b);
            return group ? MacPath::Mfma16Group : MacPath::Mfma16;
        }
        if (f.a.dtype != kMacF64 && !v15_forced_to_tasks() && rowsparse() && fits_c(rs_row_cap(10))) return MacPath::RowSparse;
        // Opt-in (BMSP_MAC_F32MFMA=1).  Measured on MI355X the kernel is bound by the 256 bytes it reads per operand tile and beats neither
        // vector-ALU kernel (block-MAC log round 3); kept, with its parity tests, as the measured answer to "does the fp32 MFMA
        // help V15"
        if (f.a.dtype == kMacF32 && f.sw.f32mfma == 1 && f.n_tasks < (1ull << 29) && mac_lane_tiles_addressable(f.a) && mac_lane_tiles_addressable(f.b) &&
            f32_chain() && finite() && f32_window())
            return MacPath::F32Mfma;
        if (!(mac_values_addressable(f.a, elem_bytes(), 0) && mac_values_addressable(f.b, elem_bytes(), 0) && mac_records_addressable(f.a) && mac_records_addressable(f.b)))
            return MacPath::ValuPointer;  // value arrays beyond the 4 GiB a buffer descriptor addresses
        if (f.a.dtype == kMacF64) return MacPath::ValuGather;
        const bool dense = f.sw.valu_dense >= 0 ? f.sw.valu_dense == 1 : (mac_valu_dense_operand(f.a) && mac_valu_dense_operand(f.b));
        return dense ? MacPath::ValuDense : MacPath::ValuGather;
    }
    int elem_bytes() const { return f.a.dtype == kMacF16 ? 2 : (f.a.dtype == kMacF32 ? 4 : 8); }
};

inline MacChoice describe(MacPath p, const MacFacts &f)
{
    MacChoice c;
    c.path = p;
    const int mfma_kernel = f.tc_version;  // the fp16 matrix-core kernels report the tc_version they stand for, V15 numerics report 5
    const unsigned b32 = mac_mfma32_b_dense(f.b, f.sw) ? kMacFormDenseTiles : kMacFormBlockMeta;
    switch (p) {
    case MacPath::None: break;
    case MacPath::RowSparse: c = {p, MacNeed::None, 5, kMacVariantRowSparse, "block_mac_rowsparse_kernel", kMacFormCsr, kMacFormCsr}; break;
    case MacPath::StripF16: c = {p, MacNeed::None, mfma_kernel, kMacVariantStrip, "block_mac_strip_kernel (fp16)", kMacFormDenseTiles, kMacFormDenseTiles}; break;
    case MacPath::StripF32: c = {p, MacNeed::None, 5, kMacVariantStrip, "block_mac_strip_kernel (fp32)", kMacFormLaneTiles, kMacFormLaneTiles}; break;
    case MacPath::Mfma32Staged: c = {p, MacNeed::None, mfma_kernel, kMacVariantStaged, "block_mac_mfma32_kernel", kMacFormDenseTiles, b32}; break;
    case MacPath::Mfma32Direct: c = {p, MacNeed::None, mfma_kernel, kMacVariantDirect, "block_mac_direct_kernel", kMacFormDenseTiles, kMacFormDenseTiles}; break;
    case MacPath::Mfma16Group: c = {p, MacNeed::None, mfma_kernel, kMacVariantDefault, "block_mac_mfma_f16_group_kernel", kMacFormBlockMeta, kMacFormBlockMeta}; break;
    case MacPath::Mfma16: c = {p, MacNeed::None, mfma_kernel, kMacVariantDefault, "block_mac_mfma_f16_kernel", 0u, 0u}; break;
    case MacPath::F32Mfma: c = {p, MacNeed::None, 5, kMacVariantF32Mfma, "block_mac_f32_mfma_kernel", kMacFormLaneTiles, kMacFormLaneTiles}; break;
    case MacPath::ValuDense: c = {p, MacNeed::None, 5, kMacVariantDefault, "block_mac_valu_group_kernel (dense-staged)", kMacFormBlockMeta | kMacFormDenseTiles, kMacFormBlockMeta | kMacFormDenseTiles}; break;
    case MacPath::ValuGather: c = {p, MacNeed::None, 5, kMacVariantDefault, "block_mac_valu_group_kernel", kMacFormBlockMeta, kMacFormBlockMeta}; break;
    case MacPath::ValuPointer: c = {p, MacNeed::None, 5, kMacVariantDefault, "block_mac_valu_kernel", 0u, 0u}; break;
    }
    return c;
}
}  // namespace mac_detail

// The kernel of a product.  Without C (has_c false): strip mode's question -- is there a numeric stage that will need C's structure
// only, and which; MacPath::None = form a task list.  With C and no task list (bmsp_spgemm_numeric on a stamped C): the same kernels, and C
// must fit them.  With a task list: the kernel of the tc_version and value type that T_7 runs from it.
inline MacChoice mac_choose(const MacFacts &f)
{
    mac_detail::Eval e{f};
    MacPath p;
    if (f.has_tasks) {
        p = e.with_tasks();
    } else {
        p = e.structure();
        if (p != MacPath::None && f.has_c && !e.fits_c(kJCap / 2)) p = MacPath::None;
    }
    if (e.need != MacNeed::None) {
        MacChoice c;
        c.need = e.need;
        return c;
    }
    return mac_detail::describe(p, f);
}

// Which cached forms bmsp_matrix_prepare(m, SPGEMM) builds for one operand (kMacForm*), from the per-operand halves of the rule.
// `transposed`: the right operand's tile layout.  need = RowStatsA / F32Chain: that fact of m / of the process first.
struct MacPrepare {
    unsigned forms = 0;
    MacNeed need = MacNeed::None;
};
inline MacPrepare mac_prepare_forms(const MacOperand &m, bool transposed, int f32_chain_ok, const MacSwitches &sw)
{
    MacPrepare r;
    if (m.values_extent >= (1ll << 32) || !mac_records_addressable(m)) return r;  // pointer-based block-MAC: no records
    r.forms = kMacFormBlockMeta;
    // K = 32 MFMA block-MAC: A (normal layout) is always read from its dense copy, B from the dense copy or from the records
    if (m.dtype == kMacF16 && mac_dense_f16_addressable(m) && (!transposed || mac_mfma32_b_dense(m, sw))) r.forms |= kMacFormDenseTiles;
    if (m.dtype != kMacF32) return r;
    if (mac_valu_dense_operand(m)) r.forms |= kMacFormDenseTiles;
    // fp32 operands of nearly empty tiles: the row-sparse kernel's CSR copy (8 B per value) -- what such a matrix is multiplied from;
    // otherwise the tiles in MFMA lane order (256 B per block) of the fp32 strip kernel and the opt-in fp32 MFMA task-list kernel.  (fp16
    // operands take the row-sparse kernel only under tc_version 5: their copy is made by the first such product)
    const int rs = mac_rowsparse_operand(m, sw);
    if (rs < 0) { r.need = MacNeed::RowStatsA; return r; }
    if (rs == 1) { r.forms |= kMacFormCsr; return r; }
    if (!mac_lane_tiles_addressable(m)) return r;
    if (f32_chain_ok < 0) { r.need = MacNeed::F32Chain; return r; }
    if (f32_chain_ok == 1) r.forms |= kMacFormLaneTiles;
    return r;
}

}  // namespace bmsp
#endif
