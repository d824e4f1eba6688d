// host_mac_choice_check.cpp -- the block-MAC rule (csrc/mac_choice.h) on both sides of every boundary, from facts built by hand.
// The expected kernels were worked out from the rule as the predicates spelt it before they were gathered into mac_choose
// (mac_rowsparse_applies, mac_strip_operands_ok, mac_strip_eligible, launch_block_mac, launch_mac_valu, prepare_spgemm_operand), not
// from mac_choose.  Prints OK and exits 0, or one line per mismatch.
#include "../bmsparse-spgemm-spmv_amd/csrc/mac_choice.h"
#include <cstdio>
#include <initializer_list>

using namespace bmsp;

static int g_bad = 0;
#define CHECK(cond) \
    do { \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); g_bad++; } \
    } while (0)

// an operand every kernel accepts: 100 tiles in 10 block-rows of 10, `fill` values per tile, all values 1.0 (biased exponent 127)
static MacOperand operand(int dtype, int64_t fill)
{
    MacOperand m;
    m.dtype = dtype; m.block_num = 100; m.nnz = fill * m.block_num; m.values_extent = m.nnz; m.num_block_rows = 10; m.max_row_blocks = 10;
    m.values_finite = 1; m.f32_exp_min = 127; m.f32_exp_max = 127;
    return m;
}
// strip mode's question for a pair of such operands; the process facts known and good
static MacFacts facts(int dtype, int tc, int64_t fill)
{
    MacFacts f;
    f.a = operand(dtype, fill); f.b = operand(dtype, fill); f.tc_version = tc; f.f32_chain_ok = 1; f.f32_exp_floor = 128;
    return f;
}
static MacFacts with_c(MacFacts f, int64_t c_rows)
{
    f.has_c = true; f.c_block_num = 1000; f.c_max_row_blocks = c_rows;
    return f;
}
static MacFacts with_tasks(MacFacts f, int64_t c_rows, uint64_t n_tasks, uint64_t candidates)
{
    f = with_c(f, c_rows); f.has_tasks = true; f.n_tasks = n_tasks; f.candidates = candidates;
    return f;
}
static MacPath path(const MacFacts &f)
{
    const MacChoice c = mac_choose(f);
    CHECK(c.need == MacNeed::None);
    return c.path;
}
static bool valu(MacPath p) { return p == MacPath::ValuDense || p == MacPath::ValuGather || p == MacPath::ValuPointer; }

int main()
{
    const int F32 = kMacF32, F16 = kMacF16, F64 = kMacF64;
    {  // what the statistics report, and the forms a launch reads
        MacChoice c = mac_choose(facts(F32, 5, 2));
        CHECK(c.path == MacPath::RowSparse && c.mac_kernel == 5 && c.mac_variant == 5 && c.a_forms == kMacFormCsr && c.b_forms == kMacFormCsr);
        c = mac_choose(facts(F32, 5, 64));
        CHECK(c.path == MacPath::StripF32 && c.mac_kernel == 5 && c.mac_variant == 3 && c.a_forms == kMacFormLaneTiles);
        c = mac_choose(facts(F16, 4, 64));
        CHECK(c.path == MacPath::StripF16 && c.mac_kernel == 4 && c.mac_variant == 3 && c.b_forms == kMacFormDenseTiles);
        c = mac_choose(facts(F64, 5, 2));
        CHECK(c.path == MacPath::None && c.mac_kernel == 0 && c.mac_variant == 0);
    }
    for (int side = 0; side < 2; side++) {  // the row-sparse operand rule, each operand separately; the other kernel is the fp32 strip kernel
        MacFacts f = facts(F32, 5, 16);
        CHECK(path(f) == MacPath::RowSparse);  // mean fill exactly 16
        MacOperand &m = side ? f.b : f.a;
        m.nnz += 1; m.values_extent += 1;      // 16 + 1 / block_num
        CHECK(path(f) == MacPath::StripF32);
        f.sw.rowsparse = 1;                    // whatever the fill
        CHECK(path(f) == MacPath::RowSparse);
        f.sw.rowsparse = 2;                    // (neither 0 nor 1: as unset)
        CHECK(path(f) == MacPath::StripF32);

        f = facts(F32, 5, 2);
        (side ? f.b : f.a).max_row_blocks = 8191;
        CHECK(path(f) == MacPath::RowSparse);
        (side ? f.b : f.a).max_row_blocks = 8192;  // no CSR copy of such a block-row; A's 8192 tiles are beyond the strip kernel's k list too
        CHECK(path(f) == (side ? MacPath::StripF32 : MacPath::None));
        f.sw.rowsparse = 1;                        // the switch lifts the fill rule only
        CHECK(path(f) == (side ? MacPath::StripF32 : MacPath::None));

        f = facts(F32, 5, 2);
        MacOperand &n = side ? f.b : f.a;
        n.block_num = 1ll << 26; n.nnz = (1ll << 29) - 1; n.values_extent = n.nnz;
        CHECK(path(f) == MacPath::RowSparse);
        n.nnz = 1ll << 29; n.values_extent = n.nnz;  // 8-byte entries beyond 32-bit byte offsets; 2^26 lane tiles are beyond them as well
        CHECK(path(f) == MacPath::None);

        for (int kind = 0; kind < 2; kind++) {  // a row-panel view, adopted arrays: no CSR copy of their own
            f = facts(F32, 5, 2);
            MacOperand &v = side ? f.b : f.a;
            if (kind) v.view = true; else v.borrowed = true;
            CHECK(path(f) == MacPath::StripF32);
            CHECK(path(with_tasks(f, 10, 100, 100)) == MacPath::ValuGather);
            f.a.dtype = f.b.dtype = F16;
            CHECK(path(f) == MacPath::None && valu(path(with_tasks(f, 10, 100, 100))));
        }
        f = facts(F32, 5, 2);
        (side ? f.b : f.a).values_finite = 0;  // a skipped pair must contribute an exact zero: no structure-only kernel at all
        CHECK(path(f) == MacPath::None && path(with_tasks(f, 10, 100, 100)) == MacPath::ValuGather);
        f.sw.f32mfma = 1;
        CHECK(path(with_tasks(f, 10, 100, 100)) == MacPath::ValuGather);
    }
    {  // fp32 exponents.  Row-sparse: every product a normal number (sums of the smallest biased exponents >= 128)
        MacFacts f = facts(F32, 5, 2);
        f.a.f32_exp_min = 64; f.b.f32_exp_min = 64;
        CHECK(path(f) == MacPath::RowSparse);
        f.a.f32_exp_min = 63;  // 127: neither the row-sparse kernel nor (floor 128) the matrix pipe
        CHECK(path(f) == MacPath::None && path(with_tasks(f, 10, 100, 100)) == MacPath::ValuGather);
        f.a.f32_exp_min = 64; f.f32_exp_floor = 174;  // a device whose pipe needs more room: the row-sparse kernel does not care
        CHECK(path(f) == MacPath::RowSparse);
        // the matrix pipe: the floor the self-test set, and sums of the largest exponents up to 354
        for (int floor : {128, 174}) {
            f = facts(F32, 5, 64);
            f.f32_exp_floor = floor;
            f.a.f32_exp_min = floor - 100; f.b.f32_exp_min = 100;
            CHECK(path(f) == MacPath::StripF32);
            f.b.f32_exp_min = 99;
            CHECK(path(f) == MacPath::None);
        }
        f = facts(F32, 5, 64);
        f.a.f32_exp_max = 200; f.b.f32_exp_max = 154;
        MacFacts t = with_tasks(f, 10, 100, 100);
        t.sw.f32mfma = 1;
        CHECK(path(f) == MacPath::StripF32 && path(t) == MacPath::F32Mfma);
        f.b.f32_exp_max = 155; t.b.f32_exp_max = 155;
        CHECK(path(f) == MacPath::None && path(t) == MacPath::ValuDense);
        t = with_tasks(facts(F32, 5, 64), 10, 100, 100);  // the task-list kernel asks the same floor
        t.sw.f32mfma = 1; t.a.f32_exp_min = 28; t.b.f32_exp_min = 100;
        CHECK(path(t) == MacPath::F32Mfma);
        t.b.f32_exp_min = 99;
        CHECK(path(t) == MacPath::ValuDense);
    }
    {  // the strip kernels' lists: 2 x (A's longest block-row) <= 192 merged A tiles; a block-row of C of at most 256 tiles
        for (int dt : {F32, F16}) {
            MacFacts f = facts(dt, dt == F16 ? 4 : 5, 64);
            const MacPath strip = dt == F16 ? MacPath::StripF16 : MacPath::StripF32;
            f.a.max_row_blocks = 96;
            CHECK(path(f) == strip);
            f.a.max_row_blocks = 97;
            CHECK(path(f) == MacPath::None);
            f.a.max_row_blocks = 10; f.b.max_row_blocks = 5000;  // (B's block-rows are walked, not held)
            CHECK(path(f) == strip);
            CHECK(path(with_c(f, 256)) == strip && path(with_c(f, 257)) == MacPath::None);
            MacFacts e = with_c(f, 1);
            e.c_block_num = 0;
            CHECK(path(e) == MacPath::None);
        }
        MacFacts f = facts(F32, 5, 2);  // strip mode's bound holds for the row-sparse kernel too; with a task list its larger table counts
        CHECK(path(with_c(f, 256)) == MacPath::RowSparse && path(with_c(f, 257)) == MacPath::None);
        CHECK(path(with_tasks(f, 257, 100, 100)) == MacPath::RowSparse && path(with_tasks(f, 768, 100, 100)) == MacPath::RowSparse);
        CHECK(path(with_tasks(f, 769, 100, 100)) == MacPath::ValuGather);
        f.a.dtype = f.b.dtype = F16;
        CHECK(path(with_tasks(f, 768, 100, 100)) == MacPath::RowSparse && valu(path(with_tasks(f, 769, 100, 100))));
    }
    {  // fp16 under every tc_version
        for (int tc : {1, 2, 3}) {
            CHECK(path(facts(F16, tc, 64)) == MacPath::None && path(facts(F16, tc, 2)) == MacPath::None);
            const MacChoice c = mac_choose(with_tasks(facts(F16, tc, 64), 10, 1000, 1000));
            CHECK(c.path == MacPath::Mfma16 && c.mac_kernel == tc && c.mac_variant == 0);
        }
        CHECK(path(facts(F16, 4, 2)) == MacPath::StripF16);  // the matrix cores' numerics: never the row-sparse kernel
        CHECK(path(facts(F16, 5, 2)) == MacPath::RowSparse && path(facts(F16, 5, 64)) == MacPath::None);
        MacFacts f = facts(F16, 5, 2);
        f.a.f32_exp_min = f.b.f32_exp_min = 1;  // (fp32 figures: not read for fp16)
        CHECK(path(f) == MacPath::RowSparse);
        CHECK(path(with_tasks(facts(F16, 5, 64), 10, 100, 100)) == MacPath::ValuDense && path(with_tasks(facts(F16, 5, 17), 10, 100, 100)) == MacPath::ValuDense);
        // tc_version 4 with a task list: strip against task-list at 20 tasks per C tile and 90 % survivors (C: 1000 tiles)
        f = facts(F16, 4, 64);
        CHECK(path(with_tasks(f, 10, 20000, 22222)) == MacPath::StripF16);
        CHECK(path(with_tasks(f, 10, 19999, 19999)) == MacPath::Mfma32Direct);
        CHECK(path(with_tasks(f, 10, 20000, 22223)) == MacPath::Mfma32Direct);
        CHECK(path(with_tasks(f, 257, 20000, 20000)) == MacPath::Mfma32Direct);
        f.sw.strip = 1;  // whatever the task counts say; the capacities hold
        CHECK(path(with_tasks(f, 10, 1000, 9000)) == MacPath::StripF16 && path(with_tasks(f, 257, 20000, 20000)) == MacPath::Mfma32Direct);
        f.sw.strip = 0;
        CHECK(path(with_tasks(f, 10, 20000, 20000)) == MacPath::Mfma32Direct && path(f) == MacPath::None);
        // direct against staged at 4.6 tasks per C tile
        f = facts(F16, 4, 64);
        MacChoice c = mac_choose(with_tasks(f, 10, 4600, 4600));
        CHECK(c.path == MacPath::Mfma32Direct && c.mac_kernel == 4 && c.mac_variant == 2 && c.a_forms == kMacFormDenseTiles && c.b_forms == kMacFormDenseTiles);
        c = mac_choose(with_tasks(f, 10, 4599, 4599));
        CHECK(c.path == MacPath::Mfma32Staged && c.mac_variant == 1 && c.b_forms == kMacFormDenseTiles);
        f.sw.direct = 0;
        CHECK(path(with_tasks(f, 10, 4600, 4600)) == MacPath::Mfma32Staged);
        f.sw.direct = 1;
        CHECK(path(with_tasks(f, 10, 10, 10)) == MacPath::Mfma32Direct);
        f.sw.b_dense = 0;  // the direct kernel reads B's dense copy
        c = mac_choose(with_tasks(f, 10, 4600, 4600));
        CHECK(c.path == MacPath::Mfma32Staged && c.b_forms == kMacFormBlockMeta);
        f.sw.b_dense = 1; f.sw.direct = -1;
        CHECK(path(with_tasks(f, 10, 4600, 4600)) == MacPath::Mfma32Direct);
        f = facts(F16, 4, 8);  // B's form without a switch: dense while the copy stays within 4 GiB or the tiles are half full; always for borrowed values
        f.b.block_num = (1ll << 25) - 1; f.b.nnz = 8 * f.b.block_num; f.b.values_extent = f.b.nnz;
        CHECK(mac_choose(with_tasks(f, 10, 10, 10)).b_forms == kMacFormDenseTiles);
        CHECK(mac_mfma32_b_dense(f.b, f.sw));
        f.b.block_num = (1ll << 25) + 1;
        CHECK(!mac_mfma32_b_dense(f.b, f.sw));
        f.b.nnz = 32 * f.b.block_num;
        CHECK(mac_mfma32_b_dense(f.b, f.sw));
        f.b.nnz = 8 * f.b.block_num; f.b.pool_owned = false;
        CHECK(mac_mfma32_b_dense(f.b, f.sw));
        // BMSP_MAC_OLD, or operands the K = 32 kernel does not address: the K = 16 kernels; the group kernel needs the allocator's read slack
        f = facts(F16, 4, 64);
        f.sw.old = 1;
        c = mac_choose(with_tasks(f, 10, 20000, 20000));
        CHECK(path(f) == MacPath::None && c.path == MacPath::Mfma16Group && c.mac_kernel == 4 && c.mac_variant == 0 && c.a_forms == kMacFormBlockMeta);
        f.sw.old = 0;  // (set at all)
        CHECK(path(f) == MacPath::None && path(with_tasks(f, 10, 20000, 20000)) == MacPath::Mfma16Group);
        f.b.pool_owned = false;
        CHECK(path(with_tasks(f, 10, 20000, 20000)) == MacPath::Mfma16);
        f = facts(F16, 4, 64);
        f.a.block_num = 1ll << 25;  // 128-byte tiles beyond 32-bit byte offsets
        CHECK(path(f) == MacPath::None && path(with_tasks(f, 10, 20000, 20000)) == MacPath::Mfma16Group);
        f.a.block_num = 1ll << 28;
        CHECK(path(with_tasks(f, 10, 20000, 20000)) == MacPath::Mfma16);
    }
    {  // fp64, and the vector-ALU forms
        MacFacts f = facts(F64, 5, 64);
        CHECK(path(f) == MacPath::None && path(with_c(f, 10)) == MacPath::None && path(with_tasks(f, 10, 100, 100)) == MacPath::ValuGather);
        f.sw.valu_dense = 1;
        CHECK(path(with_tasks(f, 10, 100, 100)) == MacPath::ValuGather);
        f.a.values_extent = 1ll << 29;  // 4 GiB of doubles
        CHECK(path(with_tasks(f, 10, 100, 100)) == MacPath::ValuPointer);
        f = facts(F32, 5, 17);  // fp32 above the row-sparse fill: dense-staged from a quarter full on, on both sides
        f.sw.strip = 0;
        CHECK(path(with_tasks(f, 10, 100, 100)) == MacPath::ValuDense);
        f.b.nnz = 16 * f.b.block_num - 1;
        CHECK(path(with_tasks(f, 10, 100, 100)) == MacPath::ValuGather);
        f.b.nnz = 17 * f.b.block_num; f.a.block_num = (1ll << 24) + 1; f.a.nnz = 17 * f.a.block_num; f.a.values_extent = f.a.nnz;  // a copy above 4 GiB
        CHECK(path(with_tasks(f, 10, 100, 100)) == MacPath::ValuGather);
        f.a.block_num = 1ll << 28; f.a.values_extent = 100;
        CHECK(path(with_tasks(f, 10, 100, 100)) == MacPath::ValuPointer);
    }
    {  // the switches of V15 numerics: unset / 0 / 1
        for (int fill : {2, 64}) {
            MacFacts f = facts(F32, 5, fill);
            const MacPath quiet = fill == 2 ? MacPath::RowSparse : MacPath::StripF32;
            CHECK(path(f) == quiet && path(with_c(f, 10)) == quiet);
            for (int v : {0, 1}) {
                f = facts(F32, 5, fill);
                f.sw.valu_dense = (int8_t)v;  // set at all: the vector-ALU kernel, from dense copies under 1
                CHECK(path(f) == MacPath::None && path(with_c(f, 10)) == MacPath::None);
                CHECK(path(with_tasks(f, 10, 100, 100)) == (v ? MacPath::ValuDense : MacPath::ValuGather));
                f = facts(F32, 5, fill);
                f.sw.f32mfma = (int8_t)v;     // set at all: a task-list kernel, the fp32 MFMA one under 1
                CHECK(path(f) == MacPath::None && path(with_c(f, 10)) == MacPath::None);
                const MacChoice c = mac_choose(with_tasks(f, 10, 100, 100));
                if (v) CHECK(c.path == MacPath::F32Mfma && c.mac_kernel == 5 && c.mac_variant == 4 && c.a_forms == kMacFormLaneTiles);
                else CHECK(c.path == (fill == 2 ? MacPath::ValuGather : MacPath::ValuDense) && c.mac_variant == 0);
            }
            f = facts(F32, 5, fill);
            f.sw.rowsparse = 0;
            CHECK(path(f) == MacPath::StripF32 && path(with_tasks(f, 10, 100, 100)) == (fill == 2 ? MacPath::ValuGather : MacPath::ValuDense));
            f = facts(F32, 5, fill);
            f.sw.strip = 0;  // strip mode's kernels off, the row-sparse one with them; a task list still takes it
            CHECK(path(f) == MacPath::None && path(with_tasks(f, 10, 100, 100)) == (fill == 2 ? MacPath::RowSparse : MacPath::ValuDense));
            f.sw.strip = 1;  // (fp32 with a task list never takes the strip kernel)
            CHECK(path(f) == quiet && path(with_tasks(f, 10, 100000, 100000)) == (fill == 2 ? MacPath::RowSparse : MacPath::ValuDense));
            f = facts(F32, 5, fill);
            f.sw.strip_prof = 1;  // the strip kernels' timing build: not the row-sparse kernel in strip mode
            CHECK(path(f) == MacPath::StripF32 && path(with_tasks(f, 10, 100, 100)) == (fill == 2 ? MacPath::RowSparse : MacPath::ValuDense));
        }
        MacFacts f = facts(F32, 5, 2);
        f.sw.f32mfma = 1; f.n_tasks = 0;
        MacFacts t = with_tasks(f, 10, 1ull << 29, 1ull << 29);  // 2^29 tasks: beyond the fp32 MFMA kernel's task index
        CHECK(path(t) == MacPath::ValuGather);
        t = with_tasks(f, 10, 100, 100);
        t.a.block_num = 1ll << 24; t.a.nnz = 2 * t.a.block_num; t.a.values_extent = t.a.nnz;
        CHECK(path(t) == MacPath::ValuGather);
        f = facts(F16, 5, 2);  // fp16 under tc_version 5: _VALU_DENSE counts, _F32MFMA is an fp32 switch, the fp16 strip kernel has other numerics
        f.sw.f32mfma = 1;
        CHECK(path(f) == MacPath::RowSparse && path(with_tasks(f, 10, 100, 100)) == MacPath::RowSparse);
        f = facts(F16, 5, 2);
        f.sw.valu_dense = 0;
        CHECK(path(f) == MacPath::None && path(with_tasks(f, 10, 100, 100)) == MacPath::ValuGather);
        f = facts(F16, 5, 2);
        f.sw.strip_prof = 1;
        CHECK(path(f) == MacPath::None);
    }
    {  // the fp32 MFMA's self-test failed on this device: the kernels that do not use the instruction remain
        MacFacts f = facts(F32, 5, 64);
        f.f32_chain_ok = 0;
        CHECK(path(f) == MacPath::None);
        f.sw.f32mfma = 1;
        CHECK(path(with_tasks(f, 10, 100, 100)) == MacPath::ValuDense);
        f = facts(F32, 5, 2);
        f.f32_chain_ok = 0;
        CHECK(path(f) == MacPath::RowSparse);
    }
    {  // laziness: the facts that cost a launch are asked for one at a time, in the order the old predicates paid for them, and only
       // while a kernel that needs them is a candidate
        auto unknown = [](MacFacts f) {
            f.a.max_row_blocks = f.b.max_row_blocks = -1; f.a.values_finite = f.b.values_finite = -1; f.f32_chain_ok = -1; f.f32_exp_floor = -1;
            f.c_max_row_blocks = -1;
            return f;
        };
        MacFacts f = unknown(facts(F32, 5, 2));  // nearly empty tiles: row maxima, figures, the row-sparse kernel -- never a self-test
        CHECK(mac_choose(f).need == MacNeed::RowStatsA);
        f.a.max_row_blocks = 10;
        CHECK(mac_choose(f).need == MacNeed::RowStatsB);
        f.b.max_row_blocks = 10;
        CHECK(mac_choose(f).need == MacNeed::Finite);
        f.a.values_finite = f.b.values_finite = 1;
        CHECK(mac_choose(f).need == MacNeed::None && mac_choose(f).path == MacPath::RowSparse);
        f = unknown(facts(F32, 5, 64));          // fuller tiles: the fill is looked at once the row maxima are there (refused without a value
        CHECK(mac_choose(f).need == MacNeed::RowStatsA);  // figure); the strip kernel: self-test, figures, floor
        f.a.max_row_blocks = 10;
        CHECK(mac_choose(f).need == MacNeed::RowStatsB);
        f.b.max_row_blocks = 10;
        CHECK(mac_choose(f).need == MacNeed::F32Chain);
        f.f32_chain_ok = 1;
        CHECK(mac_choose(f).need == MacNeed::Finite);
        f.a.values_finite = f.b.values_finite = 1;
        CHECK(mac_choose(f).need == MacNeed::F32ExpFloor);
        f.f32_exp_floor = 128;
        CHECK(mac_choose(f).need == MacNeed::None && mac_choose(f).path == MacPath::StripF32);
        f = unknown(facts(F16, 4, 64));          // fp16 under tc_version 4: A's row maxima (the k list), then "finite"
        CHECK(mac_choose(f).need == MacNeed::RowStatsA);
        f.a.max_row_blocks = 10;
        CHECK(mac_choose(f).need == MacNeed::Finite);
        f = facts(F32, 5, 64);
        f = with_c(f, 10);
        f.c_max_row_blocks = -1;
        CHECK(mac_choose(f).need == MacNeed::RowStatsC);
        f = unknown(facts(F32, 5, 64));          // the self-test failed: no value figure is fetched
        f.f32_chain_ok = 0; f.a.max_row_blocks = f.b.max_row_blocks = 10;
        CHECK(mac_choose(f).need == MacNeed::None && mac_choose(f).path == MacPath::None);
        // nothing fetched at all: fp64; fp16 under the K = 16 numerics; a switch that sends V15 to the vector-ALU kernel; an adopted operand
        CHECK(mac_choose(unknown(facts(F64, 5, 2))).need == MacNeed::None && mac_choose(unknown(with_tasks(facts(F64, 5, 2), 10, 100, 100))).need == MacNeed::None);
        CHECK(mac_choose(unknown(facts(F16, 1, 2))).need == MacNeed::None && mac_choose(unknown(with_tasks(facts(F16, 1, 2), 10, 100, 100))).need == MacNeed::None);
        f = unknown(with_tasks(facts(F32, 5, 2), 10, 100, 100));
        f.sw.valu_dense = 1;
        CHECK(mac_choose(f).need == MacNeed::None && mac_choose(f).path == MacPath::ValuDense);
        f = unknown(with_tasks(facts(F32, 5, 64), 10, 100, 100));
        f.b.borrowed = true;
        CHECK(mac_choose(f).need == MacNeed::None && mac_choose(f).path == MacPath::ValuDense);
        f = unknown(with_tasks(facts(F32, 5, 64), 10, 100, 100));  // fuller fp32 tiles from a task list: row maxima, no value figure
        CHECK(mac_choose(f).need == MacNeed::RowStatsA);
        f.a.max_row_blocks = f.b.max_row_blocks = 10;
        CHECK(mac_choose(f).need == MacNeed::None && mac_choose(f).path == MacPath::ValuDense);
        f = unknown(with_tasks(facts(F16, 4, 64), 10, 100, 100));  // few tasks per C tile: the K = 32 task-list kernel without a figure
        CHECK(mac_choose(f).need == MacNeed::None && mac_choose(f).path == MacPath::Mfma32Staged);
        f = unknown(with_tasks(facts(F16, 4, 64), 10, 20000, 20000));  // the strip kernel is a candidate: C's row maxima first
        CHECK(mac_choose(f).need == MacNeed::RowStatsC);
        f = unknown(with_tasks(facts(F32, 5, 2), 10, 100, 100));       // non-finite values under BMSP_MAC_F32MFMA=1: the floor is not asked for
        f.sw.f32mfma = 1; f.f32_chain_ok = 1; f.a.values_finite = 0; f.b.values_finite = 1;
        CHECK(mac_choose(f).need == MacNeed::None && mac_choose(f).path == MacPath::ValuGather);
    }
    {  // bmsp_matrix_prepare(m, SPGEMM): the forms per operand
        const MacSwitches none;
        auto forms = [&](const MacOperand &m, bool transposed, int chain, const MacSwitches &sw) {
            const MacPrepare p = mac_prepare_forms(m, transposed, chain, sw);
            CHECK(p.need == MacNeed::None);
            return p.forms;
        };
        CHECK(forms(operand(F32, 2), false, 1, none) == (kMacFormBlockMeta | kMacFormCsr));
        CHECK(forms(operand(F32, 16), true, 1, none) == (kMacFormBlockMeta | kMacFormCsr | kMacFormDenseTiles));
        CHECK(forms(operand(F32, 17), false, 1, none) == (kMacFormBlockMeta | kMacFormDenseTiles | kMacFormLaneTiles));
        CHECK(forms(operand(F32, 17), false, 0, none) == (kMacFormBlockMeta | kMacFormDenseTiles));
        MacOperand m = operand(F32, 2);
        m.borrowed = true;
        CHECK(forms(m, true, 1, none) == (kMacFormBlockMeta | kMacFormLaneTiles));
        m = operand(F32, 2);
        m.view = true;
        CHECK(forms(m, false, 1, none) == (kMacFormBlockMeta | kMacFormLaneTiles));
        m = operand(F32, 2);
        m.max_row_blocks = 8191;
        CHECK(forms(m, false, 1, none) == (kMacFormBlockMeta | kMacFormCsr));
        m.max_row_blocks = 8192;
        CHECK(forms(m, false, 1, none) == (kMacFormBlockMeta | kMacFormLaneTiles));
        m.max_row_blocks = -1;
        CHECK(mac_prepare_forms(m, false, 1, none).need == MacNeed::RowStatsA);
        CHECK(mac_prepare_forms(operand(F32, 2), false, -1, none).need == MacNeed::None);     // the self-test is not run for a CSR copy
        CHECK(mac_prepare_forms(operand(F32, 17), false, -1, none).need == MacNeed::F32Chain);
        MacSwitches sw;
        sw.rowsparse = 0;
        CHECK(forms(operand(F32, 2), false, 1, sw) == (kMacFormBlockMeta | kMacFormLaneTiles));
        m = operand(F32, 2);
        m.block_num = 1ll << 24; m.nnz = 1ll << 29; m.values_extent = m.nnz;
        CHECK(forms(m, false, 1, none) == (kMacFormBlockMeta | kMacFormDenseTiles));          // 32 values per tile; no CSR copy, no lane tiles
        CHECK(forms(operand(F16, 2), false, -1, none) == (kMacFormBlockMeta | kMacFormDenseTiles));
        CHECK(forms(operand(F16, 2), true, -1, none) == (kMacFormBlockMeta | kMacFormDenseTiles));
        sw = MacSwitches();
        sw.b_dense = 0;
        CHECK(forms(operand(F16, 2), true, -1, sw) == kMacFormBlockMeta && forms(operand(F16, 2), false, -1, sw) == (kMacFormBlockMeta | kMacFormDenseTiles));
        CHECK(forms(operand(F64, 2), false, -1, none) == kMacFormBlockMeta);
        m = operand(F32, 2);
        m.block_num = 1ll << 28;
        CHECK(forms(m, false, 1, none) == 0u);
        m = operand(F64, 2);
        m.values_extent = 1ll << 32;
        CHECK(forms(m, false, 1, none) == 0u);
    }
    CHECK(mac_switch(nullptr) == -1 && mac_switch("0") == 0 && mac_switch("1") == 1 && mac_switch("") == 2 && mac_switch("2") == 2);
    if (g_bad) { printf("%d checks failed\n", g_bad); return 1; }
    printf("OK\n");
    return 0;
}
