// spitsv.hip -- the iterative sparse triangular solve (bmsp_spitsv): block-Jacobi sweeps towards the x of op(tri(A)) * x = alpha * b,
//       x_I^{k+1} = T_II^{-1} * (alpha * b_I - sum_{J != I, triangle} T_IJ * x_J^k),
// exact inside every 8 x 8 diagonal tile and Jacobi between block-rows: a sweep is ONE launch over all block-rows with no levels, where
// bmsp_spsv walks a dependency chain.  Operands, triangles, diagonals and the refusals are bmsp_spsv's.
//
// What is reused (spsv_plan.hip.h): the tile records of (A, op), the cached plan of (A, op, fill) -- for `levels` and the missing-diagonal
// row only; a sweep has no schedule -- and spsv_block_row itself, with the previous iterate as its input and the next one as its output.
// Every row therefore runs bmsp_spsv's chain of operations, and a block-row of plan level l holds bmsp_spsv's bits after sweep l + 1.
//
// What is new:
//   spitsv_sweep_kernel   eight lanes per block-row, 32 block-rows per workgroup, block-rows in natural order.  <STATS>: every lane
//       compares its row with the previous iterate (bits changed; |x_new - x_old|; |x_new|; NaNs skipped), the three are reduced across
//       the wave in registers and across the workgroup's four waves through LDS, and ONE lane issues at most one integer atomic per
//       statistic into this sweep's own record: the bits of a non-negative float order like an unsigned integer, so there is no
//       floating-point atomic and the record does not depend on arrival order.
//   termination on the device   sweep k + 1 begins by evaluating the stop rule on record k (uniformly: one record, every lane) and
//       returns without writing when it holds; its own record stays zero, "nothing changed", so every later sweep returns too.  The host
//       enqueues BMSP_SPITSV_CHECK sweeps, reads their records back and evaluates the same predicate: the switch decides how much is
//       enqueued ahead, never the result.
//   The record, the stop rule and the reduction live in sweep_stats.hip.h: ilu0.hip's sweeps end the same way.
// The iterates ping-pong between d_x and one temporary kept on the handle; whichever holds the last one, it ends in d_x.
#include "spsv_plan.hip.h"
#include "sweep_stats.hip.h"
#include <cmath>

namespace bmsp {
namespace {

constexpr int64_t kMaxIter = 1ll << 20;
// Sweeps enqueued between two read-backs (BMSP_SPITSV_CHECK; measured in DESIGN §4 "Iterative triangular solve")
constexpr int64_t kCheckDefault = 8;

// One sweep over block-rows [0, blocks).  prev: the record of the sweep before (null for the first), mine: this sweep's.
template <typename S, bool MINOR, bool LOWER, bool UNIT, bool STATS>
__global__ __launch_bounds__(kThreads) void spitsv_sweep_kernel(SpsvTiles T, const uint32_t *__restrict__ ptr, uint32_t blocks,
                                                                const S *__restrict__ vals, typename TileValue<S>::R alpha,
                                                                const typename TileValue<S>::R *b, const typename TileValue<S>::R *x_in,
                                                                typename TileValue<S>::R *x_out, int64_t n, typename TileValue<S>::R tol,
                                                                const SweepRecord *prev, SweepRecord *mine)
{
    using R = typename TileValue<S>::R;
    if (STATS && prev && stop_rule<R>(*prev, tol)) return;  // (every lane of the grid reads the same record: all leave or none)
    const uint64_t g = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) >> 3;
    const int i = (int)(threadIdx.x & 7);
    const bool live = g < blocks;  // (whole groups: a shuffle of the substitution stays inside its group)
    R xi = R(0);
    if (live) xi = spsv_block_row<S, MINOR, LOWER, UNIT>(T, ptr, vals, alpha, b, x_in, x_out, n, (uint32_t)g, i);
    if (!STATS) return;
    using V = TileValue<R>;
    unsigned long long changed = 0, delta = 0, xmax = 0;
    const int64_t o = (int64_t)g * 8 + i;
    if (live && o < n) {
        const R old = x_in[o];
        changed = __builtin_bit_cast(typename V::U, xi) != __builtin_bit_cast(typename V::U, old);
        const typename V::U d = V::abs_bits(xi - old), m = V::abs_bits(xi);
        if (d <= V::kInf) delta = d;  // (NaN bits lie above kInf: skipped)
        if (m <= V::kInf) xmax = m;
    }
    sweep_publish(changed, delta, xmax, mine);
}

struct SweepArgs {
    const bmsp_matrix_s *A;
    SpsvTiles T;
    const uint32_t *ptr;
    int64_t blocks;
    double alpha, tol;
    const void *b;
};

template <typename S, bool MINOR, bool LOWER, bool UNIT, bool STATS>
void launch_sweep(const SweepArgs &a, const void *x_in, void *x_out, const SweepRecord *prev, SweepRecord *mine, hipStream_t st)
{
    using R = typename TileValue<S>::R;
    hipLaunchKernelGGL((spitsv_sweep_kernel<S, MINOR, LOWER, UNIT, STATS>), grid_for((uint64_t)a.blocks * 8), dim3(kThreads), 0, st, a.T, a.ptr,
                       (uint32_t)a.blocks, (const S *)a.A->values, (R)a.alpha, (const R *)a.b, (const R *)x_in, (R *)x_out,
                       (int64_t)a.A->num_rows, (R)a.tol, prev, mine);
    BMSP_CHECK_LAUNCH();
}

template <typename S, bool MINOR, bool LOWER, typename... Args>
void launch_stats(bool unit, bool stats, Args &&...args)
{
    if (unit) {
        if (stats) launch_sweep<S, MINOR, LOWER, true, true>(args...);
        else launch_sweep<S, MINOR, LOWER, true, false>(args...);
    } else {
        if (stats) launch_sweep<S, MINOR, LOWER, false, true>(args...);
        else launch_sweep<S, MINOR, LOWER, false, false>(args...);
    }
}

template <typename S, typename... Args>
void launch_variant(bool minor, bool lower, bool unit, bool stats, Args &&...args)
{
    if (minor) {
        if (lower) launch_stats<S, true, true>(unit, stats, args...);
        else launch_stats<S, true, false>(unit, stats, args...);
    } else {
        if (lower) launch_stats<S, false, true>(unit, stats, args...);
        else launch_stats<S, false, false>(unit, stats, args...);
    }
}

bool no_check(double tol) { return tol == BMSP_ITSV_NO_CHECK; }

}  // namespace

void spitsv_check_args(int op, int fill, int diag, int64_t max_iter, double tol, int flags, const double *delta_history)
{
    spsv_check_args(op, fill, diag);
    if (max_iter < 0 || max_iter > kMaxIter)
        fail(BMSP_ERR_INVALID, "max_iter must be 0 (levels + 1 of the plan) or 1 .. 2^20 (got %lld)", (long long)max_iter);
    if (std::isnan(tol) || (tol < 0.0 && !no_check(tol)))
        fail(BMSP_ERR_INVALID, "tol must be >= 0 or BMSP_ITSV_NO_CHECK (-1.0) (got %g)", tol);
    if (flags & ~BMSP_ITSV_X0_GIVEN) fail(BMSP_ERR_INVALID, "flags: unknown bits (got %d; BMSP_ITSV_X0_GIVEN = 1 is the only one)", flags);
    if (no_check(tol) && delta_history) fail(BMSP_ERR_INVALID, "delta_history must be NULL under BMSP_ITSV_NO_CHECK: nothing is read back");
}

void spitsv_check_vectors(const void *b, const void *x)
{
    if (b == x) fail(BMSP_ERR_INVALID, "d_x must not be d_b: b is read in every sweep");
}

void spitsv(bmsp_matrix_s *A, int op, int fill, int diag, double alpha, const void *b, void *x, int64_t max_iter, double tol, int flags,
            double *delta_history, bmsp_spitsv_info *info, hipStream_t st)
{
    spitsv_check_args(op, fill, diag, max_iter, tol, flags, delta_history);
    spsv_check_matrix(A);
    spitsv_check_vectors(b, x);
    const bmsp_spsv_plan_s &pl = ensure_plan(A, op, fill, st);
    refuse_missing_diagonal(pl, diag);
    const bool stats = !no_check(tol), f64 = A->dtype == BMSP_F64;
    if (info) {
        memset(info, 0, sizeof *info);
        info->levels = pl.levels;
        info->converged = stats ? 1 : 0;
        info->delta = info->xmax = stats ? 0.0 : -1.0;
        snprintf(info->kernel, sizeof info->kernel, "none (empty matrix)");
    }
    if (pl.blocks == 0) return;
    const bool minor = (op == BMSP_OP_T) != (A->transposed != 0), lower = effective_lower(op, fill), unit = diag == BMSP_DIAG_UNIT;
    if (info)
        snprintf(info->kernel, sizeof info->kernel, "spitsv_sweep_kernel<%s, %s, %s, %s, %s>",
                 A->dtype == BMSP_F16 ? "F16" : (A->dtype == BMSP_F32 ? "F32" : "F64"), minor ? "MINOR" : "MAJOR", lower ? "LOWER" : "UPPER",
                 unit ? "UNIT" : "NON_UNIT", stats ? "STATS" : "NO_STATS");
    const uint32_t *ptr = nullptr;
    const bmsp_spmv_op_view *w = view_of(A, op, st, &ptr);  // (both exist: the plan was made from them)
    const SweepArgs args{A, tiles_of(A, w), ptr, pl.blocks, alpha, stats ? tol : 0.0, b};
    const size_t bytes = spmv_op_vector_size(A) * (size_t)A->num_rows;
    if (!A->spitsv_tmp) A->spitsv_tmp.alloc(bytes);
    // x^j lives in even(j) ? first : second.  A given x^0 is d_x's content; otherwise x^0 = +0 is written into the temporary, d_x is not
    // read and the first sweep overwrites it.
    void *first = x, *second = A->spitsv_tmp;
    if (!(flags & BMSP_ITSV_X0_GIVEN)) {
        first = A->spitsv_tmp;
        second = x;
        BMSP_HIP(hipMemsetAsync(first, 0, bytes, st));
    }
    const auto iterate = [&](int64_t j) { return j & 1 ? second : first; };
    const auto sweep = [&](int64_t k, const SweepRecord *prev, SweepRecord *mine) {
        dispatch_dtype(A->dtype, [&](auto s) {
            using S = decltype(s);
            launch_variant<S>(minor, lower, unit, stats, args, (const void *)iterate(k), iterate(k + 1), prev, mine, st);
        });
    };
    const int64_t m = max_iter ? max_iter : pl.levels + 1;
    int64_t sweeps = m;
    if (!stats) {
        for (int64_t k = 0; k < m; k++) sweep(k, nullptr, nullptr);
    } else {
        const int64_t check = sweep_check_from_env("BMSP_SPITSV_CHECK", kCheckDefault);
        DevBuf<SweepRecord> recs((size_t)m);
        std::vector<SweepRecord> host((size_t)m);
        BMSP_HIP(hipMemsetAsync(recs.p, 0, sizeof(SweepRecord) * (size_t)m, st));
        bool converged = false;
        for (int64_t done = 0; done < m && !converged;) {
            const int64_t batch = check < m - done ? check : m - done;
            for (int64_t k = done; k < done + batch; k++) sweep(k, k ? recs.p + k - 1 : nullptr, recs.p + k);
            BMSP_HIP(hipStreamSynchronize(st));
            copy_d2h_staged(host.data() + done, recs.p + done, sizeof(SweepRecord) * (size_t)batch);
            for (int64_t k = done; k < done + batch && !converged; k++) {
                const SweepRecord &r = host[(size_t)k];
                if (f64 ? stop_rule<double>(r, tol) : stop_rule<float>(r, (float)tol)) {
                    converged = true;
                    sweeps = k + 1;  // (the sweeps enqueued behind it returned at once and wrote nothing)
                }
            }
            done += batch;
        }
        const auto widen = [&](unsigned long long u) { return f64 ? VecBits<double>::from(u) : (double)VecBits<float>::from(u); };
        if (delta_history)
            for (int64_t k = 0; k < sweeps; k++) delta_history[k] = widen(host[(size_t)k].delta);
        if (info) {
            info->converged = converged ? 1 : 0;
            info->delta = widen(host[(size_t)sweeps - 1].delta);
            info->xmax = widen(host[(size_t)sweeps - 1].xmax);
        }
    }
    if (info) info->sweeps = sweeps;
    if (iterate(sweeps) != x) BMSP_HIP(hipMemcpyAsync(x, iterate(sweeps), bytes, hipMemcpyDeviceToDevice, st));
}

}  // namespace bmsp

BMSP_DEFINE_WARM(spitsv)
