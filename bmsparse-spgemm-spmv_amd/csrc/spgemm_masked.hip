// spgemm_masked.hip -- the masked sparse product on the pattern of a third matrix (bmsp_spgemm_masked / bmsp_spgemm_masked_values): for every
// stored coordinate (i, j) of M, d_ij = the sum over the inner indices k at which A stores (i, k) and B stores (k, j) of a_ik * b_kj, k
// ascending over the whole inner dimension, one fused multiply-add per product starting from +0; then c = alpha * d + beta * m or
// alpha * d * m (sddmm.hip's epilogue).
//
// The output has M's keys, offsets and (possibly transposed) bitmaps, as an SDDMM or a scaled matrix has: no symbolic pass, no sort, no
// scan, no read-back.  Every output value has exactly one writer: no sum across lanes, no atomic, no LDS, no hand-off.  The one structure
// the pass needs besides the operands' own arrays is B's tiles in (block-column, block-row) order with a block-column pointer: the cached
// op-T view of bmsp_spmv_op / bmsp_spmm_op (spmv_op_ensure_view), structure only.
//
// Kernels:
//   spgemm_masked_kernel<SA, SM, G>  vector ALU, operands of storage type SA, mask and output of SM.  G lanes per M tile (lane_group,
//                  tile_pass.hip.h).  The unit of work is one byte of the output bitmap (a row of a row-major output tile, a column of a
//                  column-major one): G = 8 gives lane t byte t, G = 1 lets the lane visit its tile's non-empty bytes one after another.
//                  Per unit a lane walks the intersection of A's block-row I with B's block-column J (walk_pairs, walk_pairs.hip.h) in ascending K and keeps
//                  the byte's eight accumulators in registers; the loop over the eight positions is fully unrolled and predicated by the
//                  bitmap.  The eight lanes of a group issue the same list and record loads; they diverge only on their byte's positions.
//   spgemm_masked_count_kernel       the same walk, counting the matches of every M tile (bmsp_spgemm_masked_launch_info's `pairs`).
#include "walk_pairs.hip.h"
#include <cstring>
#include <vector>

namespace bmsp {
namespace {

// Mean values per M tile from which eight lanes per tile are the default.  Measured (DESIGN section 4 "Masked SpGEMM"): eight lanes won on
// every class and at every fill timed, down to 1.5 values per tile -- the eight lanes of a group share every list and record load of the
// walk, a lone lane repeats the walk for each of its bytes next to 63 lanes on other tiles' walks -- so the family's 6 is not used here.
constexpr int64_t kFillThreshold = 0;

__device__ __forceinline__ float fma_f(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_f(double a, double b, double c) { return __builtin_fma(a, b, c); }

// what the kernels read of the three matrices (device pointers; the view's records and block-column pointer for B)
template <typename SA>
struct Operands {
    const uint64_t *a_keys, *a_bmps, *a_offsets;
    const SA *a_vals;
    const uint32_t *a_rowptr;  // null: A or B holds no tile, every list is empty
    const uint4 *b_recs;
    const uint32_t *b_ptr;
    const SA *b_vals;
    int a_lay, b_lay;
};

// Byte t of output tile (I, J): positions u = 0 .. 7 with (r, c) = (t, u) for a row-major output, (u, t) for a column-major one; `byte`
// holds the stored ones (bit 7 - u).  acc[u] = d of position u.  `acc` is indexed by unrolled loop counters only: it lives in registers.
template <typename SA, typename F>
__device__ __forceinline__ void dot_byte(const Operands<SA> &op, uint32_t a_lo, uint32_t a_hi, uint32_t b_lo, uint32_t b_hi, int olay, int t,
                                         uint32_t byte, F (&acc)[8])
{
    using DA = TileValue<SA>;
    const ListA<true> la{op.a_keys, op.a_bmps, op.a_offsets};
    const ListB lb{op.b_recs};
    walk_pairs(la, a_lo, a_hi, lb, b_lo, b_hi, [&](const ListA<true>::Entry &ea, const ListB::Entry &eb) {
        const uint64_t ab = ea.bmp, bb = eb.bmp;
        const uint64_t arm = op.a_lay ? tile_transpose(ab) : ab;  // row-major: byte r = row r of A, bit 7 - k = inner index k
        const uint64_t bcm = op.b_lay ? bb : tile_transpose(bb);  // column-major: byte c = column c of B, bit 7 - k = inner index k
        if ((tile_or_bytes(arm) & tile_or_bytes(bcm)) == 0) return;  // no common inner index
        const SA *av = op.a_vals + ea.off;
        const SA *bv = op.b_vals + eb.off;
        const uint32_t fixed = olay ? tile_byte(bcm, t) : tile_byte(arm, t);
        if (fixed == 0) return;
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (!((byte >> (7 - u)) & 1u)) continue;
            const int r = olay ? u : t, c = olay ? t : u;
            uint32_t common = fixed & (olay ? tile_byte(arm, u) : tile_byte(bcm, u));
            F d = acc[u];
            while (common) {  // (at most 8 bits)
                const int k = __builtin_clz(common) - 24;
                common &= ~(0x80u >> k);
                const F a = DA::load(av[tile_rank(ab, op.a_lay ? 8 * k + r : 8 * r + k)]);
                const F b = DA::load(bv[tile_rank(bb, op.b_lay ? 8 * c + k : 8 * k + c)]);
                d = fma_f(a, b, d);
            }
            acc[u] = d;
        }
    });
}

// Value pass over M's tiles [0, nb): m_vals and o_vals may be the same array (in place: flip == 0, a value is read and written by one
// lane).
template <typename SA, typename SM, int G>
__global__ __launch_bounds__(kThreads) void spgemm_masked_kernel(Operands<SA> op, const uint64_t *__restrict__ m_keys,
                                                                 const uint64_t *__restrict__ m_bmps, const uint64_t *__restrict__ m_offsets,
                                                                 const SM *m_vals, SM *o_vals, uint64_t nb, int flip, int olay,
                                                                 typename TileValue<SA>::F alpha, typename TileValue<SA>::F beta, int mode)
{
    using DM = TileValue<SM>;
    using F = typename TileValue<SA>::F;
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t j = gid / G;
    if (j >= nb) return;
    const uint64_t key = m_keys[j], ib = m_bmps[j], off = m_offsets[j];
    const uint64_t ob = flip ? tile_transpose(ib) : ib;
    uint32_t a_lo = 0, a_hi = 0, b_lo = 0, b_hi = 0;
    if (op.a_rowptr) {
        a_lo = op.a_rowptr[key_row(key)]; a_hi = op.a_rowptr[key_row(key) + 1];
        b_lo = op.b_ptr[key_col(key)]; b_hi = op.b_ptr[key_col(key) + 1];
    }
    const SM *src = m_vals + off;
    SM *dst = o_vals + off;
#pragma unroll 1
    for (int s = 0; s < 8 / G; s++) {  // G = 8: lane t takes byte t; G = 1: the non-empty bytes one after another
        const int t = G == 8 ? (int)(gid % G) : s;
        const uint32_t byte = tile_byte(ob, t);
        if (byte == 0) continue;
        F acc[8];
#pragma unroll
        for (int u = 0; u < 8; u++) acc[u] = 0;
        dot_byte<SA, F>(op, a_lo, a_hi, b_lo, b_hi, olay, t, byte, acc);
        const int base = tile_rank(ob, 8 * t);
        F sv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {  // (every load of m before the first store: in place they are the same array)
            sv[u] = 0;
            if (mode != kModeAlpha && ((byte >> (7 - u)) & 1u)) sv[u] = DM::load(src[tile_rank(ib, flip ? tile_transposed_pos(8 * t + u) : 8 * t + u)]);
        }
        int w = base;
#pragma unroll
        for (int u = 0; u < 8; u++)
            if ((byte >> (7 - u)) & 1u) dst[w++] = DM::store(epilogue<F>(acc[u], alpha, beta, sv[u], mode));
    }
}

// the matches of every M tile: the value kernel's walk with a counter in place of the products
__global__ __launch_bounds__(kThreads) void spgemm_masked_count_kernel(const uint64_t *__restrict__ a_keys, const uint32_t *__restrict__ a_rowptr,
                                                                       const uint4 *__restrict__ b_recs, const uint32_t *__restrict__ b_ptr,
                                                                       const uint64_t *__restrict__ m_keys, uint64_t nb, uint32_t *__restrict__ counts)
{
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= nb) return;
    const uint64_t key = m_keys[j];
    uint32_t n = 0;
    const ListA<false> la{a_keys, nullptr, nullptr};
    const ListB lb{b_recs};
    walk_pairs(la, a_rowptr[key_row(key)], a_rowptr[key_row(key) + 1], lb, b_ptr[key_col(key)], b_ptr[key_col(key) + 1],
               [&](const ListA<false>::Entry &, const ListB::Entry &) { n++; });
    counts[j] = n;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
void check_operand(const bmsp_matrix_s *m, const char *what)
{
    refuse_view(m, what);
    if (m->block_num >= (1ll << 32) || m->nnz >= (1ll << 32)) fail(BMSP_ERR_LIMIT, "%s: 2^32 tiles or values or more", what);
}

bool no_pairs(const bmsp_matrix_s *A, const bmsp_matrix_s *B) { return A->block_num == 0 || B->block_num == 0; }

template <typename SA, typename SM>
void launch_masked(int lanes, bmsp_matrix_s *A, bmsp_matrix_s *B, const bmsp_spmv_op_view *w, const bmsp_matrix_s *M, bmsp_matrix_s *out,
                   double alpha, double beta, int mode, hipStream_t st)
{
    using F = typename TileValue<SA>::F;
    Operands<SA> op;
    op.a_keys = A->keys; op.a_bmps = A->bmps; op.a_offsets = A->offsets; op.a_vals = (const SA *)A->values;
    op.a_rowptr = w ? A->rowptr : nullptr;
    op.b_recs = w ? (const uint4 *)w->mem : nullptr;
    op.b_ptr = w ? (const uint32_t *)((const char *)w->mem + w->off_ptr) : nullptr;
    op.b_vals = (const SA *)B->values;
    op.a_lay = A->transposed; op.b_lay = B->transposed;
    const uint64_t nb = (uint64_t)out->block_num;
    const int flip = M->transposed != out->transposed;
    launch_lane_group(lanes, nb, [&](auto g, dim3 grid) {
        hipLaunchKernelGGL((spgemm_masked_kernel<SA, SM, decltype(g)::value>), grid, dim3(kThreads), 0, st, op, M->keys, M->bmps, M->offsets,
                           (const SM *)M->values, (SM *)out->values, nb, flip, out->transposed, (F)alpha, (F)beta, mode);
    });
}

// out's values from A, B and M through out's layout; out has M's tile order (out == M: in place)
void masked_pass(bmsp_matrix_s *A, bmsp_matrix_s *B, const bmsp_matrix_s *M, bmsp_matrix_s *out, double alpha, double beta, int flags,
                 hipStream_t st)
{
    if (out->block_num == 0 || out->nnz == 0) return;
    const bmsp_spmv_op_view *w = nullptr;
    if (!no_pairs(A, B)) {
        ensure_rowptr(A, st);
        w = &spmv_op_ensure_view(B, BMSP_OP_T, st);
    }
    const int lanes = lane_group(M->nnz, M->block_num, "BMSP_MASKED_LANES", kFillThreshold);
    const int mode = epilogue_mode(A->dtype, beta, (flags & BMSP_MASKED_MUL_M) != 0);
    if (A->dtype == BMSP_F16 && M->dtype == BMSP_F32) {
        launch_masked<uint16_t, float>(lanes, A, B, w, M, out, alpha, beta, mode, st);
        return;
    }
    dispatch_dtype(A->dtype, [&](auto s) { launch_masked<decltype(s), decltype(s)>(lanes, A, B, w, M, out, alpha, beta, mode, st); });
}

// M's keys and offsets, its bitmaps transposed when the layout flips: the structure of a layout conversion, tile order kept
struct CopyMaskPattern {
    const uint64_t *s_keys, *s_bmps, *s_off;
    uint64_t nb;
    int flip;
    uint64_t *keys, *bmps, *offsets;
    __device__ void operator()(uint64_t i) const
    {
        offsets[i] = s_off[i];
        if (i == nb) return;
        keys[i] = s_keys[i];
        const uint64_t b = s_bmps[i];
        bmps[i] = flip ? tile_transpose(b) : b;
    }
};

}  // namespace

// the refusals that need the handles, before any device call; out: null for the calls that make their own output
void spgemm_masked_check_matrices(const bmsp_matrix_s *A, const bmsp_matrix_s *B, const bmsp_matrix_s *M, const bmsp_matrix_s *out)
{
    if (A->num_cols != B->num_rows)
        fail(BMSP_ERR_INVALID, "spgemm_masked: A.num_cols (%d) != B.num_rows (%d)", A->num_cols, B->num_rows);
    if (M->num_rows != A->num_rows || M->num_cols != B->num_cols)
        fail(BMSP_ERR_INVALID, "spgemm_masked: M is %d x %d, A * B is %d x %d", M->num_rows, M->num_cols, A->num_rows, B->num_cols);
    if (A->dtype != B->dtype) fail(BMSP_ERR_INVALID, "spgemm_masked: A and B differ in dtype (%d, %d)", (int)A->dtype, (int)B->dtype);
    if (M->dtype != A->dtype && !(A->dtype == BMSP_F16 && M->dtype == BMSP_F32))
        fail(BMSP_ERR_INVALID, "spgemm_masked: M's dtype (%d) must be A's (%d), or F32 for F16 operands", (int)M->dtype, (int)A->dtype);
    check_operand(A, "spgemm_masked: A");
    check_operand(B, "spgemm_masked: B");
    check_operand(M, "spgemm_masked: M");
    if (!out) return;
    if (out == A || out == B) fail(BMSP_ERR_INVALID, "spgemm_masked_values: out is %s: the pass would read what it writes", out == A ? "A" : "B");
    if (out != M) {
        // a transpose's output has the source's uid too, but its own tile order (tp_map)
        if (!out->tp_src_uid || out->tp_src_uid != M->uid || out->tp_map)
            fail(BMSP_ERR_INVALID, "spgemm_masked_values: out is neither M nor made from M by bmsp_spgemm_masked, bmsp_sddmm, bmsp_matrix_scale or "
                                   "a layout conversion, or M's structure changed since");
        if (M->block_num != out->block_num || M->nnz != out->nnz || M->dtype != out->dtype || M->num_rows != out->num_rows ||
            M->num_cols != out->num_cols)
            fail(BMSP_ERR_INVALID, "spgemm_masked_values: M's and out's sizes or dtypes differ");
        refuse_view(out, "spgemm_masked_values: out");
    }
}

void spgemm_masked_check_args(double beta, int flags, int out_transposed)
{
    if (flags & ~BMSP_MASKED_MUL_M) fail(BMSP_ERR_INVALID, "flags has unknown bits (got 0x%x)", (unsigned)flags);
    if ((flags & BMSP_MASKED_MUL_M) && beta != 0.0) fail(BMSP_ERR_INVALID, "beta must be 0 under BMSP_MASKED_MUL_M (got %g)", beta);
    check_layout_flag(out_transposed, "out_transposed");
}

// a new matrix of M's structure in layout out_transposed with the masked product as values; what a layout conversion records is
// recorded too, so that spgemm_masked_values_into, sddmm_values_into, scale_values_into and copy_values_from accept the output
bmsp_matrix_s *spgemm_masked_matrix(bmsp_matrix_s *A, bmsp_matrix_s *B, bmsp_matrix_s *M, double alpha, double beta, int flags,
                                    int out_transposed, hipStream_t st)
{
    spgemm_masked_check_args(beta, flags, out_transposed);
    spgemm_masked_check_matrices(A, B, M, nullptr);
    auto m = make_matrix();
    m->num_rows = M->num_rows; m->num_cols = M->num_cols; m->dtype = M->dtype; m->transposed = out_transposed;
    m->nnz = M->nnz; m->block_num = M->block_num;
    m->tp_src_uid = M->uid;
    m->tp_permute = out_transposed != M->transposed ? 1 : 0;
    const uint64_t nb = (uint64_t)M->block_num;
    alloc_tile_arrays(m.get(), nb);
    alloc_values(m.get(), m->nnz);
    device_for_each(CopyMaskPattern{M->keys, M->bmps, M->offsets, nb, m->tp_permute, m->keys, m->bmps, m->offsets}, nb + 1, st);
    masked_pass(A, B, M, m.get(), alpha, beta, flags, st);
    ensure_rowptr(m.get(), st);
    return m.release();
}

void spgemm_masked_values_into(bmsp_matrix_s *A, bmsp_matrix_s *B, bmsp_matrix_s *M, double alpha, double beta, int flags, bmsp_matrix_s *out,
                               hipStream_t st)
{
    spgemm_masked_check_args(beta, flags, 0);
    spgemm_masked_check_matrices(A, B, M, out);
    drop_value_caches(out);
    masked_pass(A, B, M, out, alpha, beta, flags, st);
}

// The launcher's own decision for (A, B, M) and the matches its walk finds: builds A's block-row pointer and B's view if they are missing,
// counts on the device with the value kernel's walker and reads the per-tile counts back (it synchronises).
void spgemm_masked_launch_info(bmsp_matrix_s *A, bmsp_matrix_s *B, bmsp_matrix_s *M, int out_transposed, bmsp_spgemm_masked_info *info)
{
    spgemm_masked_check_args(0.0, 0, out_transposed);
    spgemm_masked_check_matrices(A, B, M, nullptr);
    memset(info, 0, sizeof(*info));
    const bmsp_spmv_op_view *w = nullptr;
    if (!no_pairs(A, B)) {
        ensure_rowptr(A, nullptr);
        w = &spmv_op_ensure_view(B, BMSP_OP_T, nullptr);
        info->view_bytes = (int64_t)w->bytes;
    }
    if (M->block_num == 0 || M->nnz == 0) {
        snprintf(info->kernel, sizeof(info->kernel), "none (empty mask)");
        return;
    }
    info->lanes = lane_group(M->nnz, M->block_num, "BMSP_MASKED_LANES", kFillThreshold);
    snprintf(info->kernel, sizeof(info->kernel), "spgemm_masked_kernel<%d>", info->lanes);
    if (!w) return;
    const uint64_t nb = (uint64_t)M->block_num;
    DevBuf<uint32_t> counts((size_t)nb);
    hipLaunchKernelGGL(spgemm_masked_count_kernel, grid_for(nb), dim3(kThreads), 0, nullptr, A->keys, A->rowptr, (const uint4 *)w->mem,
                       (const uint32_t *)((const char *)w->mem + w->off_ptr), M->keys, nb, counts.p);
    BMSP_CHECK_LAUNCH();
    BMSP_HIP(hipDeviceSynchronize());
    std::vector<uint32_t> h((size_t)nb);
    copy_d2h_staged(h.data(), counts.p, 4 * (size_t)nb);
    int64_t pairs = 0;
    for (uint32_t c : h) pairs += c;
    info->pairs = pairs;
}

}  // namespace bmsp

BMSP_DEFINE_WARM(spgemm_masked)
