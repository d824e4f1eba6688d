// spsv.hip -- the sparse triangular solve op(tri(A)) * x = alpha * b (bmsp_spsv) for op in {N, T}, the lower or the upper triangle of a
// square A in either tile layout and a unit or a stored diagonal, without a transpose, a conversion or a second copy of A.
//
// What is reused (spmv_op.hip): the tiles as 16-byte records in the order of the OUTPUT blocks with a pointer per output block and the
// tile's other block index in every record -- the access pattern of a substitution -- and the lane mapping per (op, layout): MINOR = false,
// the output index inside the block is the byte index of the bitmap; MINOR = true, it is the bit index inside each byte.  (N, row-major A)
// has no view: it reads A's own arrays and the block-row pointer.
//
// What is new: the dependency schedule and the substitution inside the diagonal tile.
//   plan     per (op, fill), structure only, cached on the handle: the level of an output block is 1 + the largest level of the blocks it
//            depends on (every tile of the strict block triangle counts, whatever its bitmap), found in one pass on the host
//            (spsv_plan) over the block pointer and the 4-byte other-index column; the blocks ordered by (level, index), the level
//            pointer and the launch schedule.
//   kernels  eight lanes per block-row, lane i owns row i of the block.  A group walks its block-row's records in chain order (ascending
//            other index for a lower system, descending for an upper one) up to the diagonal tile, s = fma(-a_ij, x_j, s) per stored entry,
//            then substitutes inside the diagonal tile in eight steps: the lane whose turn it is divides (the IEEE division sequence),
//            x_c goes round the group by a wave shuffle, the lanes that store (i, c) take it into their sums.
//            spsv_level_kernel: one launch per level, 32 block-rows per workgroup.
//            spsv_chain_kernel: ONE workgroup walks a run of consecutive narrow levels, a workgroup barrier between two levels; x is
//            stored and loaded again inside the workgroup, so x is never __restrict__ and never read through a read-only path.
// Ordering comes from kernel boundaries and the workgroup barrier alone: no flag, no spin, no atomic, no cooperative launch.  Every x_i
// has one writer and one fixed chain of operations: x is a pure function of A's arrays, b and alpha.
#include "spsv_plan.hip.h"

namespace bmsp {
namespace {

constexpr int kGroups = kThreads / 8;  // block-rows per workgroup and pass

// block-rows order[first .. first + width) of one level
template <typename S, bool MINOR, bool LOWER, bool UNIT>
__global__ __launch_bounds__(kThreads) void spsv_level_kernel(SpsvTiles T, const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ order,
                                                              uint32_t first, uint32_t width, const S *__restrict__ vals,
                                                              typename TileValue<S>::R alpha, const typename TileValue<S>::R *b,
                                                              typename TileValue<S>::R *x, int64_t n)
{
    const uint64_t g = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) >> 3;
    if (g >= width) return;  // (whole groups leave: a shuffle stays inside its group)
    spsv_block_row<S, MINOR, LOWER, UNIT>(T, ptr, vals, alpha, b, x, x, n, order[first + g], (int)(threadIdx.x & 7));
}

// levels [l0, l1) by one workgroup; the level loop is uniform, the barrier orders the stores to x of a level before the loads of the next
template <typename S, bool MINOR, bool LOWER, bool UNIT>
__global__ __launch_bounds__(kThreads) void spsv_chain_kernel(SpsvTiles T, const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ order,
                                                              const uint32_t *__restrict__ level_ptr, uint32_t l0, uint32_t l1,
                                                              const S *__restrict__ vals, typename TileValue<S>::R alpha,
                                                              const typename TileValue<S>::R *b, typename TileValue<S>::R *x, int64_t n)
{
    const uint32_t g = threadIdx.x >> 3;
    const int i = (int)(threadIdx.x & 7);
    for (uint32_t l = l0; l < l1; l++) {
        const uint64_t hi = level_ptr[l + 1];
        for (uint64_t k = (uint64_t)level_ptr[l] + g; k < hi; k += kGroups)
            spsv_block_row<S, MINOR, LOWER, UNIT>(T, ptr, vals, alpha, b, x, x, n, order[k], i);
        __syncthreads();
    }
}

template <typename S, bool MINOR, bool LOWER, bool UNIT>
void launch_plan(const bmsp_matrix_s *A, const SpsvTiles &T, const uint32_t *ptr, const bmsp_spsv_plan_s &pl, double alpha, const void *b, void *x,
                 hipStream_t st)
{
    using R = typename TileValue<S>::R;
    const uint32_t *order = pl.mem, *level_ptr = (const uint32_t *)((const char *)pl.mem + pl.off_level_ptr);
    for (size_t s = 0; s < pl.segments.size(); s += 3) {
        const uint32_t l0 = pl.segments[s], l1 = pl.segments[s + 1];
        if (pl.segments[s + 2]) {
            hipLaunchKernelGGL((spsv_chain_kernel<S, MINOR, LOWER, UNIT>), dim3(1), dim3(kThreads), 0, st, T, ptr, order, level_ptr, l0, l1,
                               (const S *)A->values, (R)alpha, (const R *)b, (R *)x, (int64_t)A->num_rows);
        } else {
            const uint32_t first = pl.level_ptr[l0], width = pl.level_ptr[l0 + 1] - first;
            hipLaunchKernelGGL((spsv_level_kernel<S, MINOR, LOWER, UNIT>), grid_for((uint64_t)width * 8), dim3(kThreads), 0, st, T, ptr, order,
                               first, width, (const S *)A->values, (R)alpha, (const R *)b, (R *)x, (int64_t)A->num_rows);
        }
        BMSP_CHECK_LAUNCH();
    }
}

template <typename S, bool MINOR, bool LOWER, typename... Args>
void launch_diag(bool unit, Args &&...args)
{
    if (unit) launch_plan<S, MINOR, LOWER, true>(args...);
    else launch_plan<S, MINOR, LOWER, false>(args...);
}

template <typename S, typename... Args>
void launch_variant(bool minor, bool lower, bool unit, Args &&...args)
{
    if (minor) {
        if (lower) launch_diag<S, true, true>(unit, args...);
        else launch_diag<S, true, false>(unit, args...);
    } else {
        if (lower) launch_diag<S, false, true>(unit, args...);
        else launch_diag<S, false, false>(unit, args...);
    }
}

}  // namespace

void spsv_check_args(int op, int fill, int diag)
{
    spmv_op_check_op(op);
    if (fill != BMSP_FILL_LOWER && fill != BMSP_FILL_UPPER)
        fail(BMSP_ERR_INVALID, "fill must be BMSP_FILL_LOWER (0) or BMSP_FILL_UPPER (1) (got %d)", fill);
    if (diag != BMSP_DIAG_NON_UNIT && diag != BMSP_DIAG_UNIT)
        fail(BMSP_ERR_INVALID, "diag must be BMSP_DIAG_NON_UNIT (0) or BMSP_DIAG_UNIT (1) (got %d)", diag);
}

void spsv_check_matrix(const bmsp_matrix_s *A)
{
    if (A->num_rows != A->num_cols) fail(BMSP_ERR_INVALID, "spsv: matrix A must be square (it is %d x %d)", A->num_rows, A->num_cols);
    spmv_op_check_matrix(A, "spsv");
}

// Levels and launch schedule of a substitution over `blocks` output blocks whose records [ptr[I], ptr[I + 1]) carry the other block
// index other[t]: block I depends on every other[t] < I (lower) or > I (upper).  Host only.
void spsv_plan(const uint32_t *ptr, const uint32_t *other, int64_t blocks, int lower, int64_t chain, uint32_t *level_of, uint32_t *order,
               uint32_t *level_ptr, uint32_t *segments, int64_t *n_levels, int64_t *n_segments)
{
    if (blocks < 0) fail(BMSP_ERR_INVALID, "blocks must be >= 0 (got %lld)", (long long)blocks);
    if (chain < 0) fail(BMSP_ERR_INVALID, "chain must be >= 0 (got %lld)", (long long)chain);
    if (blocks && !ptr) fail(BMSP_ERR_INVALID, "ptr is null");
    if (blocks >= (1ll << 32)) fail(BMSP_ERR_LIMIT, "spsv: 2^32 blocks or more");
    for (int64_t I = 0; I < blocks; I++)
        if (ptr[I + 1] < ptr[I]) fail(BMSP_ERR_INVALID, "ptr decreases at block %lld", (long long)I);
    if (blocks && ptr[blocks] > ptr[0] && !other) fail(BMSP_ERR_INVALID, "other is null");
    for (uint64_t t = blocks ? ptr[0] : 0; blocks && t < ptr[blocks]; t++)
        if ((int64_t)other[t] >= blocks) fail(BMSP_ERR_INVALID, "other[%llu] = %u is not below blocks (%lld)", (unsigned long long)t, other[t], (long long)blocks);
    std::vector<uint32_t> lev((size_t)blocks, 0u);
    int64_t levels = 0;
    for (int64_t k = 0; k < blocks; k++) {
        const int64_t I = lower ? k : blocks - 1 - k;
        uint32_t l = 0;
        for (uint64_t t = ptr[I]; t < ptr[I + 1]; t++) {
            const int64_t J = other[t];
            if ((lower ? J < I : J > I) && lev[(size_t)J] + 1 > l) l = lev[(size_t)J] + 1;
        }
        lev[(size_t)I] = l;
        if ((int64_t)l + 1 > levels) levels = (int64_t)l + 1;
    }
    std::vector<uint32_t> lp((size_t)levels + 1, 0u);
    for (int64_t I = 0; I < blocks; I++) lp[(size_t)lev[(size_t)I] + 1]++;
    for (int64_t l = 0; l < levels; l++) lp[(size_t)l + 1] += lp[(size_t)l];
    if (order) {
        std::vector<uint32_t> at(lp.begin(), lp.end() - 1);
        for (int64_t I = 0; I < blocks; I++) order[at[lev[(size_t)I]]++] = (uint32_t)I;
    }
    if (level_of) memcpy(level_of, lev.data(), 4 * (size_t)blocks);
    if (level_ptr) memcpy(level_ptr, lp.data(), 4 * ((size_t)levels + 1));
    // a maximal run of at least two consecutive levels of at most `chain` block-rows each is one chain launch; every other level its own
    int64_t ns = 0;
    const auto emit = [&](int64_t l0, int64_t l1, uint32_t kind) {
        if (segments) { uint32_t *s = segments + 3 * ns; s[0] = (uint32_t)l0; s[1] = (uint32_t)l1; s[2] = kind; }
        ns++;
    };
    for (int64_t l = 0; l < levels;) {
        int64_t e = l;
        while (e < levels && (int64_t)(lp[(size_t)e + 1] - lp[(size_t)e]) <= chain) e++;
        if (e - l >= 2) { emit(l, e, 1u); l = e; continue; }
        emit(l, l + 1, 0u);
        l++;
    }
    if (n_levels) *n_levels = levels;
    if (n_segments) *n_segments = ns;
}

void spsv_analyse(bmsp_matrix_s *A, int op, int fill, int diag, hipStream_t st, bmsp_spsv_info *info)
{
    spsv_check_args(op, fill, diag);
    spsv_check_matrix(A);
    const bmsp_spsv_plan_s &pl = ensure_plan(A, op, fill, st);
    refuse_missing_diagonal(pl, diag);
    if (!info) return;
    memset(info, 0, sizeof *info);
    info->levels = pl.levels;
    info->max_level_width = pl.max_level_width;
    info->launches = (int64_t)(pl.segments.size() / 3);
    info->chain_launches = pl.chain_launches;
    info->chained_levels = pl.chained_levels;
    info->plan_bytes = (int64_t)pl.bytes;
    if (pl.blocks == 0) {
        snprintf(info->kernel, sizeof info->kernel, "none (empty matrix)");
        return;
    }
    const bool minor = (op == BMSP_OP_T) != (A->transposed != 0);
    snprintf(info->kernel, sizeof info->kernel, "spsv_level_kernel<%s, %s, %s, %s>",
             A->dtype == BMSP_F16 ? "F16" : (A->dtype == BMSP_F32 ? "F32" : "F64"), minor ? "MINOR" : "MAJOR",
             effective_lower(op, fill) ? "LOWER" : "UPPER", diag == BMSP_DIAG_UNIT ? "UNIT" : "NON_UNIT");
}

void spsv(bmsp_matrix_s *A, int op, int fill, int diag, double alpha, const void *b, void *x, hipStream_t st)
{
    spsv_check_args(op, fill, diag);
    spsv_check_matrix(A);
    const bmsp_spsv_plan_s &pl = ensure_plan(A, op, fill, st);
    refuse_missing_diagonal(pl, diag);
    if (pl.blocks == 0) return;
    const uint32_t *ptr = nullptr;
    const bmsp_spmv_op_view *w = view_of(A, op, st, &ptr);  // (both exist: the plan was made from them)
    const SpsvTiles T = tiles_of(A, w);
    const bool minor = (op == BMSP_OP_T) != (A->transposed != 0);
    dispatch_dtype(A->dtype, [&](auto s) {
        using S = decltype(s);
        launch_variant<S>(minor, effective_lower(op, fill), diag == BMSP_DIAG_UNIT, A, T, ptr, pl, alpha, b, x, st);
    });
}

}  // namespace bmsp

BMSP_DEFINE_WARM(spsv)
