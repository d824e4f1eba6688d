// mac_choice.hip -- the gatherer of the block-MAC decision: copies what the rule of mac_choice.h reads out of the handles, asks it, and
// fetches the facts it names.  bmsp_spgemm, bmsp_spgemm_numeric (spgemm.hip) and bmsp_matrix_prepare(m, SPGEMM) (builder.hip) decide
// through this file and nowhere else.  No kernels here.
#include "matrix.h"
#include <cstdlib>

namespace bmsp {

static_assert(kMacF32 == BMSP_F32 && kMacF16 == BMSP_F16 && kMacF64 == BMSP_F64, "mac_choice.h numbers the value types as bmsp.h does");
static_assert(kMacVariantDefault == BMSP_MAC_DEFAULT && kMacVariantStaged == BMSP_MAC_STAGED && kMacVariantDirect == BMSP_MAC_DIRECT &&
              kMacVariantStrip == BMSP_MAC_STRIP && kMacVariantF32Mfma == BMSP_MAC_F32MFMA && kMacVariantRowSparse == BMSP_MAC_ROWSPARSE, "... and the variants");

MacSwitches mac_read_switches()
{
    MacSwitches sw;
    sw.strip = mac_switch(getenv("BMSP_MAC_STRIP")); sw.rowsparse = mac_switch(getenv("BMSP_MAC_ROWSPARSE"));
    sw.valu_dense = mac_switch(getenv("BMSP_MAC_VALU_DENSE")); sw.f32mfma = mac_switch(getenv("BMSP_MAC_F32MFMA"));
    sw.old = mac_switch(getenv("BMSP_MAC_OLD")); sw.b_dense = mac_switch(getenv("BMSP_MAC_B_DENSE"));
    sw.direct = mac_switch(getenv("BMSP_MAC_DIRECT")); sw.strip_prof = mac_switch(getenv("BMSP_STRIP_PROF"));
    return sw;
}

MacOperand mac_operand_facts(const bmsp_matrix_s *m)
{
    MacOperand o;
    o.dtype = (int)m->dtype; o.nnz = m->nnz; o.block_num = m->block_num; o.values_extent = m->values_extent(); o.num_block_rows = m->num_block_rows();
    o.max_row_blocks = m->max_row_blocks;
    o.pool_owned = pool_owns(m->values); o.borrowed = m->ownership == 2; o.view = m->view_values_end != 0;
    o.values_finite = m->values_finite; o.f32_exp_min = m->f32_exp_min; o.f32_exp_max = m->f32_exp_max;
    return o;
}

// The block-MAC kernel of A x B (mac_choice.h): without C, strip mode's question; with C, and with C's task list where `tasks` is given.
// Copies what the rule reads out of the handles, asks it, and fetches the facts it names -- row maxima, value figures, the fp32 MFMA's
// self-tests -- one at a time, in the order it names them: a figure is paid for only while a kernel that needs it is a candidate.
MacChoice mac_decide(bmsp_matrix_s *A, bmsp_matrix_s *B, bmsp_matrix_s *C, const MacTasks *tasks, int tc_version, const MacSwitches &sw, hipStream_t st)
{
    MacFacts f;
    f.tc_version = tc_version; f.sw = sw; f.has_c = C != nullptr; f.has_tasks = tasks != nullptr;
    if (tasks) { f.n_tasks = tasks->n; f.candidates = tasks->candidates; }
    for (;;) {
        f.a = mac_operand_facts(A); f.b = mac_operand_facts(B);
        if (C) { f.c_block_num = C->block_num; f.c_max_row_blocks = C->max_row_blocks; }
        const MacChoice ch = mac_choose(f);
        switch (ch.need) {
        case MacNeed::None: return ch;
        case MacNeed::RowStatsA: ensure_row_stats(A, st); break;
        case MacNeed::RowStatsB: ensure_row_stats(B, st); break;
        case MacNeed::RowStatsC: ensure_row_stats(C, st); break;
        case MacNeed::Finite: ensure_finite_flag(A, st); ensure_finite_flag(B, st); break;
        case MacNeed::F32Chain: f.f32_chain_ok = mac_f32_mfma_usable(st) ? 1 : 0; break;
        case MacNeed::F32ExpFloor: f.f32_exp_floor = mac_f32_exp_floor(st); break;
        }
    }
}

}  // namespace bmsp
