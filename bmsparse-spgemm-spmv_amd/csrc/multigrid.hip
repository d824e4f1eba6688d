// multigrid.hip -- the V-cycle of a caller-supplied hierarchy, enqueued on a stream (bmsp_mg_create / _free / _info / _vcycle), and CG and
// BiCGStab preconditioned by it (bmsp_mg_solve binds the cycle to krylov.hip's preconditioner hook).  include/bmsp.h writes the
// arithmetic out operation by operation; tests/multigrid_ref.c restates it.
//
// What is reused (spsv_plan.hip.h): the tile records read from a matrix's own arrays with the dense block-row pointer (SpsvTiles,
// spsv_rec: tiles are in (block-row, block-column) order in both layouts, so neither needs a view), the fused multiply-add and the walk
// of one tile's row (tile_row_chain, here in its two halves tile_row_gather / tile_row_fold), MINOR for column-major tiles.  bmsp_matrix_diagonal gives the diagonals at create.
//
// What is new:
//   mg_row_kernel<S, MINOR, NEG, INIT, JACOBI>   eight lanes per block-row, lane i owns row i, the walk of spsv_block_row over ALL tiles
//       of the block-row, four tiles in flight and their records loaded one batch ahead: s = init_i (or +0), s = fma(+-m_ij, v_j, s) per stored entry in
//       column order.  Four instantiations per (S, MINOR): the residual (NEG, INIT, store), the Jacobi step (NEG, INIT, x' = x + wR *
//       (s / d)), the restriction (+, +0, store) and the prolongation (+, INIT = x, store: the add is the chain's start).
//   mg_first_step_kernel    x = wR * (r / d), the Jacobi step from x = 0: no walk.
//   mg_dense_kernel         the coarsest level by its dense inverse, one lane per row; the handle keeps the inverse column by column so
//       that consecutive lanes load consecutive addresses.
// Every kernel takes `stopped` (null, or the status word of the solve that drives the cycle) and returns without writing once it is set.
// Every output has one writer and one fixed chain: no atomic, no flag, no spin, no LDS.  Ordering comes from kernel boundaries alone.
#include "spsv_plan.hip.h"
#include <cmath>
#include <string>

// The handle: the operators are borrowed, everything on the device that it allocates is an owner below.
struct bmsp_mg_s {
    int levels = 0, pre = 0, post = 0;
    bmsp_dtype dtype = BMSP_F32;
    double omega = 0.0;
    bool exact = false;  // the coarsest level has its inverse
    std::vector<bmsp_matrix_s *> A, P, R;  // levels, levels - 1, levels - 1 (null entries: restrict by P^T)
    std::vector<int64_t> n;
    // diagonals of every level | per level l > 0 its right-hand side | per level two iterates (level 0: one, the other is d_z) and the
    // residual: offsets in bytes into `work`
    bmsp::DevBuf<void> diag, inv, work;
    std::vector<size_t> off_diag, off_rhs, off_x0, off_x1, off_t;
    size_t work_bytes = 0;
};

namespace bmsp {
namespace {

constexpr int64_t kMaxCoarse = 4096;
// How a block-row is walked (WALK), chosen per operator by a pure function of its structure (walk_of below; BMSP_MG_WALK=group1|group4|wave
// forces one, read per call).  The chain of a row is the same in all three, term by term: they differ in who loads what and when.
//   1, 4   eight lanes per block-row; the values and v of 1 or 4 tiles are gathered together, their records loaded one batch ahead
//   wave   a wave per block-row: lane group g gathers tile t + g of every eight, then the chain goes through the eight groups in tile
//          order -- every lane folds its own tile's row onto the running s and the wave takes the result of the group whose turn it is
//          (one shuffle per tile) -- so eight tiles' loads are in flight for sixteen loads per lane; group 0 stores.  For the block-rows of
//          a coarse operator (a hundred tiles), where a lane group's serial walk leaves the device idle.
// Measured per level on the bench hierarchies, fp32, us per Jacobi step at group1 / group4 / wave (DESIGN §4 "Multigrid cycle"): below 32
// tiles per block-row in the mean group1 is level with group4 or faster (7 tiles 39 / 47 / 103, 9 tiles 12.7 / 12.8 / 21.5, 24 tiles 23.4 /
// 22.3 / 36.8); from there a long block-row wants its loads in flight together, and the wave walk wins where the groups alone would
// leave the device idle (294 - 724 block-rows of 41 - 91 tiles: 28 - 59 / 28 - 57 / 7 - 15) and loses where they fill it (12 978
// block-rows of 55 tiles 37 / 30 / 33, 23 574 of 94 tiles 73 / 60 / 84).  Nothing was measured between 724 and 12 978 block-rows: 8 192
// is one wave per SIMD slot of the device.
constexpr int kWalkWave = 8;
constexpr int64_t kLongTiles = 32, kWaveBlockRows = 8192;
// Restriction by the row kernel up to this many tiles per block-row of R in the mean, by bmsp_spmv_op beyond (BMSP_MG_RESTRICT=row|spmv
// forces one, read per call): a lane group walks its block-row alone, and bmsp_spmv_op splits long block-rows over several.  Measured
// per level in DESIGN §4 "Multigrid cycle", and on synthetic operators of exactly 12 / 24 / 48 / 96 tiles per block-row (the sub-cycle
// around the restriction, row / spmv, us: 23.8 / 26.9, 37.2 / 36.0, 63.2 / 53.5, 120.5 / 88.2): the two cross at 24.
constexpr int64_t kRestrictRowTiles = 24;

template <typename S, bool MINOR, bool NEG, bool INIT, bool JACOBI, int WALK>
__global__ __launch_bounds__(kThreads) void mg_row_kernel(const int *stopped, SpsvTiles T, const uint32_t *__restrict__ ptr, uint32_t blocks,
                                                          const S *__restrict__ vals, const typename TileValue<S>::R *init,
                                                          const typename TileValue<S>::R *v, const typename TileValue<S>::R *d,
                                                          typename TileValue<S>::R wR, typename TileValue<S>::R *out, int64_t n)
{
#pragma clang fp contract(off)
    using F = typename TileValue<S>::F;
    constexpr bool WAVE = WALK == kWalkWave;
    if (stopped && *stopped) return;  // (every lane of the grid reads the same word, written by an earlier launch: all leave or none)
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t I64 = WAVE ? gid >> 6 : gid >> 3;
    if (I64 >= blocks) return;  // (whole groups, whole waves under WAVE: a shuffle stays among lanes that are all here)
    const uint32_t I = (uint32_t)I64;
    const int i = (int)(threadIdx.x & 7);
    const int64_t o = (int64_t)I * 8 + i;
    const bool row = o < n;  // (the ragged last block: its rows beyond n hold no entry, read nothing and are not written)
    F s = INIT && row ? init[o] : F(0);
    int64_t t = (int64_t)ptr[I];
    const int64_t end = (int64_t)ptr[I + 1];
    const uint4 none = make_uint4(0u, 0u, 0u, 0u);  // (an empty bitmap: nothing is gathered for a slot beyond the block-row)
    if constexpr (!WAVE) {
        constexpr int kBatch = WALK;
        uint4 next[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; b++) next[b] = t + b < end ? spsv_rec(T, (uint64_t)(t + b)) : none;
        for (; t < end; t += kBatch) {
            F a[kBatch][8], x[kBatch][8];
            int cnt[kBatch];
#pragma unroll
            for (int b = 0; b < kBatch; b++) {
                const uint4 r = next[b];
                cnt[b] = tile_row_gather<S, MINOR>((uint64_t)r.y << 32 | r.x, vals + r.z, v + (uint64_t)r.w * 8, i, a[b], x[b]);  // only stored entries index v
            }
#pragma unroll
            for (int b = 0; b < kBatch; b++) next[b] = t + kBatch + b < end ? spsv_rec(T, (uint64_t)(t + kBatch + b)) : none;
#pragma unroll
            for (int b = 0; b < kBatch; b++) s = tile_row_fold<F, NEG>(a[b], x[b], cnt[b], s);
        }
    } else {
        const int g = lane_id() >> 3;
        uint4 next = t + g < end ? spsv_rec(T, (uint64_t)(t + g)) : none;
        for (; t < end; t += 8) {  // (t and end are the wave's: the loop and the shuffles in it are uniform)
            F a[8], x[8];
            const uint4 r = next;
            const int cnt = tile_row_gather<S, MINOR>((uint64_t)r.y << 32 | r.x, vals + r.z, v + (uint64_t)r.w * 8, i, a, x);
            next = t + 8 + g < end ? spsv_rec(T, (uint64_t)(t + 8 + g)) : none;
#pragma unroll
            for (int gp = 0; gp < 8; gp++) {
                if (t + gp >= end) break;
                const F s2 = tile_row_fold<F, NEG>(a, x, cnt, s);  // (meaningful in group gp: its tile is the chain's next)
                s = __shfl(s2, 8 * gp + i, kWave);
            }
        }
        if (g != 0) return;
    }
    if (!row) return;
    if (JACOBI) {
        const F q = s / d[o];
        const F wq = wR * q;
        out[o] = v[o] + wq;
    } else {
        out[o] = s;
    }
}

// x = +0, the iterate of a level that has no pre-smoothing step
template <typename R>
__global__ __launch_bounds__(kThreads) void mg_zero_kernel(const int *stopped, R *x, int64_t n)
{
    if (stopped && *stopped) return;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) x[i] = R(0);
}

template <typename R>
__global__ __launch_bounds__(kThreads) void mg_first_step_kernel(const int *stopped, const R *r, const R *d, R wR, R *x, int64_t n)
{
#pragma clang fp contract(off)
    if (stopped && *stopped) return;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const R q = r[i] / d[i];
    x[i] = wR * q;
}

// invT[j * n + i] = inv_ij
template <typename R>
__global__ __launch_bounds__(kThreads) void mg_dense_kernel(const int *stopped, const R *__restrict__ invT, const R *__restrict__ r, R *x, int64_t n)
{
    if (stopped && *stopped) return;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    R s = R(0);
    for (int64_t j = 0; j < n; j++) s = fused(invT[j * n + i], r[j], s);
    x[i] = s;
}

// the caller's row-major inverse (leading dimension ld) into the handle's column-by-column copy
template <typename R>
struct TransposeInverse {
    const R *inv;
    R *invT;
    uint64_t n, ld;
    __device__ void operator()(uint64_t k) const
    {
        const uint64_t j = k / n, i = k % n;
        invT[k] = inv[i * ld + j];
    }
};

struct RowCall {
    const int *stopped;
    bmsp_matrix_s *M;
    const void *init, *v, *d;
    double w;
    void *out;
};

// WALK of an operator: a function of its mean tiles per block-row alone, unless BMSP_MG_WALK says
int walk_of(const bmsp_matrix_s *M)
{
    if (const char *e = getenv("BMSP_MG_WALK")) {
        if (!strcmp(e, "group1")) return 1;
        if (!strcmp(e, "group4")) return 4;
        if (!strcmp(e, "wave")) return kWalkWave;
    }
    const int64_t rows = M->num_block_rows();
    if (M->block_num < kLongTiles * rows) return 1;
    return rows <= kWaveBlockRows ? kWalkWave : 4;
}

template <typename S, bool MINOR, bool NEG, bool INIT, bool JACOBI, int WALK>
void launch_walk(const RowCall &c, int64_t blocks, hipStream_t st)
{
    using R = typename TileValue<S>::R;
    const bmsp_matrix_s *M = c.M;
    hipLaunchKernelGGL((mg_row_kernel<S, MINOR, NEG, INIT, JACOBI, WALK>), grid_for((uint64_t)blocks * (WALK == kWalkWave ? 64 : 8)), dim3(kThreads), 0,
                       st, c.stopped, SpsvTiles{nullptr, M->keys, M->bmps, M->offsets}, (const uint32_t *)M->rowptr, (uint32_t)blocks,
                       (const S *)M->values, (const R *)c.init, (const R *)c.v, (const R *)c.d, (R)c.w, (R *)c.out, (int64_t)M->num_rows);
    BMSP_CHECK_LAUNCH();
}

template <typename S, bool MINOR, bool NEG, bool INIT, bool JACOBI>
void launch_row(const RowCall &c, hipStream_t st)
{
    bmsp_matrix_s *M = c.M;
    const int64_t blocks = M->num_block_rows();
    if (blocks == 0) return;
    ensure_rowptr(M, st);  // (made at create; a bmsp_matrix_invalidate(M, 1) since then has dropped it)
    const int walk = walk_of(M);
    if (walk == kWalkWave) launch_walk<S, MINOR, NEG, INIT, JACOBI, kWalkWave>(c, blocks, st);
    else if (walk == 4) launch_walk<S, MINOR, NEG, INIT, JACOBI, 4>(c, blocks, st);
    else launch_walk<S, MINOR, NEG, INIT, JACOBI, 1>(c, blocks, st);
}

enum RowKind { kResidual, kJacobi, kRestrict, kProlong };

template <typename S>
void launch_kind(int kind, const RowCall &c, hipStream_t st)
{
    const bool minor = c.M->transposed != 0;
    if (minor) {
        if (kind == kResidual) launch_row<S, true, true, true, false>(c, st);
        else if (kind == kJacobi) launch_row<S, true, true, true, true>(c, st);
        else if (kind == kRestrict) launch_row<S, true, false, false, false>(c, st);
        else launch_row<S, true, false, true, false>(c, st);
    } else {
        if (kind == kResidual) launch_row<S, false, true, true, false>(c, st);
        else if (kind == kJacobi) launch_row<S, false, true, true, true>(c, st);
        else if (kind == kRestrict) launch_row<S, false, false, false, false>(c, st);
        else launch_row<S, false, false, true, false>(c, st);
    }
}

void row_call(const bmsp_mg_s *mg, int kind, const RowCall &c, hipStream_t st)
{
    if (mg->dtype == BMSP_F64) launch_kind<double>(kind, c, st);
    else launch_kind<float>(kind, c, st);
}

size_t vec_size(const bmsp_mg_s *mg) { return mg->dtype == BMSP_F64 ? 8 : 4; }
size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

// BMSP_MG_RESTRICT_* of level l (to level l + 1), decided per call
int restrict_mode(const bmsp_mg_s *mg, int l)
{
    const bmsp_matrix_s *R = mg->R[(size_t)l];
    if (!R) return BMSP_MG_RESTRICT_PT;
    if (const char *e = getenv("BMSP_MG_RESTRICT")) {
        if (!strcmp(e, "row")) return BMSP_MG_RESTRICT_ROW;
        if (!strcmp(e, "spmv")) return BMSP_MG_RESTRICT_SPMV;
    }
    return R->block_num <= kRestrictRowTiles * R->num_block_rows() ? BMSP_MG_RESTRICT_ROW : BMSP_MG_RESTRICT_SPMV;
}

struct Cycle {
    const bmsp_mg_s *mg;
    const int *stopped;
    hipStream_t st;
    int64_t launches = 0;
    bool dry = false;  // count the launches, enqueue nothing (bmsp_mg_info)

    char *work(size_t off) const { return (char *)mg->work.p + off; }
    const void *diag(int l) const { return (const char *)mg->diag.p + mg->off_diag[(size_t)l]; }

    // `steps` damped-Jacobi steps on level l for right-hand side r.  x: the current iterate, or null for x = 0; buf: the two buffers;
    // *at: the buffer x lives in (the first step from zero writes buf[*at]).  Returns the new iterate.
    void *smooth(int l, int steps, const void *r, void *x, void *const buf[2], int *at)
    {
        const int64_t n = mg->n[(size_t)l];
        for (int k = 0; k < steps; k++) {
            launches++;
            if (!x) {
                x = buf[*at];
                if (dry) continue;
                if (mg->dtype == BMSP_F64)
                    hipLaunchKernelGGL(mg_first_step_kernel<double>, grid_for((uint64_t)n), dim3(kThreads), 0, st, stopped, (const double *)r,
                                       (const double *)diag(l), mg->omega, (double *)x, n);
                else
                    hipLaunchKernelGGL(mg_first_step_kernel<float>, grid_for((uint64_t)n), dim3(kThreads), 0, st, stopped, (const float *)r,
                                       (const float *)diag(l), (float)mg->omega, (float *)x, n);
                BMSP_CHECK_LAUNCH();
                continue;
            }
            *at ^= 1;
            void *y = buf[*at];
            if (!dry) row_call(mg, kJacobi, RowCall{stopped, mg->A[(size_t)l], r, x, diag(l), mg->omega, y}, st);
            x = y;
        }
        return x;
    }

    // the cycle of level l for right-hand side r; the result ends in `out` when it is given (level 0: d_z), else where it returns
    void *run(int l, const void *r, void *out)
    {
        const int64_t n = mg->n[(size_t)l];
        const bool last = l == mg->levels - 1;
        void *buf[2] = {out ? out : (void *)work(mg->off_x0[(size_t)l]), work(mg->off_x1[(size_t)l])};
        if (last && mg->exact) {
            launches++;
            if (!dry) {
                if (mg->dtype == BMSP_F64)
                    hipLaunchKernelGGL(mg_dense_kernel<double>, grid_for((uint64_t)n), dim3(kThreads), 0, st, stopped, (const double *)mg->inv.p,
                                       (const double *)r, (double *)buf[0], n);
                else
                    hipLaunchKernelGGL(mg_dense_kernel<float>, grid_for((uint64_t)n), dim3(kThreads), 0, st, stopped, (const float *)mg->inv.p,
                                       (const float *)r, (float *)buf[0], n);
                BMSP_CHECK_LAUNCH();
            }
            return buf[0];
        }
        const int pre = last ? mg->pre + mg->post : mg->pre, post = last ? 0 : mg->post;
        // the iterate changes buffers with every step but the first from zero: start where the last one lands in buf[0]
        const int flips = pre > 0 ? pre + post - 1 : post;
        int at = flips & 1;
        void *x = smooth(l, pre, r, nullptr, buf, &at);
        if (last) return x;
        const void *t = r;
        if (!x) {  // pre == 0: x = 0 and the residual is r
            x = buf[at];
            launches++;
            if (!dry) {  // (a kernel, not a memset: it reads `stopped` like the rest)
                if (mg->dtype == BMSP_F64) hipLaunchKernelGGL(mg_zero_kernel<double>, grid_for((uint64_t)n), dim3(kThreads), 0, st, stopped, (double *)x, n);
                else hipLaunchKernelGGL(mg_zero_kernel<float>, grid_for((uint64_t)n), dim3(kThreads), 0, st, stopped, (float *)x, n);
                BMSP_CHECK_LAUNCH();
            }
        } else {
            void *tt = work(mg->off_t[(size_t)l]);
            launches++;
            if (!dry) row_call(mg, kResidual, RowCall{stopped, mg->A[(size_t)l], r, x, nullptr, 0.0, tt}, st);
            t = tt;
        }
        void *rc = work(mg->off_rhs[(size_t)l + 1]);
        const int mode = restrict_mode(mg, l);
        launches++;
        if (!dry) {
            if (mode == BMSP_MG_RESTRICT_ROW) row_call(mg, kRestrict, RowCall{stopped, mg->R[(size_t)l], nullptr, t, nullptr, 0.0, rc}, st);
            else if (mode == BMSP_MG_RESTRICT_SPMV) spmv_op(mg->R[(size_t)l], BMSP_OP_N, 1.0, t, 0.0, rc, st);
            else spmv_op(mg->P[(size_t)l], BMSP_OP_T, 1.0, t, 0.0, rc, st);
        }
        const void *e = run(l + 1, rc, nullptr);
        launches++;
        if (!dry) row_call(mg, kProlong, RowCall{stopped, mg->P[(size_t)l], x, e, nullptr, 0.0, x}, st);  // (in place: a lane reads its own x_i only)
        return smooth(l, post, r, x, buf, &at);
    }
};

void check_operator(const bmsp_matrix_s *M, const char *name, int l, int64_t rows, int64_t cols, bmsp_dtype dtype)
{
    char what[48];
    snprintf(what, sizeof what, "mg_create (%s[%d])", name, l);
    spmv_op_check_matrix(M, what);  // (row-panel views first: their shape is the panel's)
    if (M->dtype == BMSP_F16) fail(BMSP_ERR_UNSUPPORTED, "%s[%d]: an F16 operator is not supported (the vectors of the cycle would be fp16)", name, l);
    if (M->dtype != dtype) fail(BMSP_ERR_INVALID, "%s[%d]: dtype differs from A[0]'s (every operator of a hierarchy has one dtype)", name, l);
    if (M->num_rows != rows || M->num_cols != cols)
        fail(BMSP_ERR_INVALID, "%s[%d]: shape %d x %d does not chain (expected %lld x %lld)", name, l, M->num_rows, M->num_cols, (long long)rows,
             (long long)cols);
}

}  // namespace

void mg_check_args(int levels, double omega, int pre, int post, const void *d_coarse_inv)
{
    if (levels < 1 || levels > BMSP_MG_MAX_LEVELS) fail(BMSP_ERR_INVALID, "levels must be 1 .. %d (got %d)", BMSP_MG_MAX_LEVELS, levels);
    if (!std::isfinite(omega)) fail(BMSP_ERR_INVALID, "omega must be finite (got %g)", omega);
    if (pre < 0 || pre > 16) fail(BMSP_ERR_INVALID, "pre must be 0 .. 16 (got %d)", pre);
    if (post < 0 || post > 16) fail(BMSP_ERR_INVALID, "post must be 0 .. 16 (got %d)", post);
    if (pre + post == 0 && !(levels == 1 && d_coarse_inv))
        fail(BMSP_ERR_INVALID, "pre + post must be >= 1: a level without an exact solve needs a smoothing step");
}

// the refusals that read the handles: host only, nothing is done on the device
void mg_check_operands(int levels, bmsp_matrix_s *const *A, bmsp_matrix_s *const *P, bmsp_matrix_s *const *R, const void *d_coarse_inv,
                       int64_t ld_inv)
{
    const bmsp_dtype dtype = A[0]->dtype;
    for (int l = 0; l < levels; l++) {
        check_operator(A[l], "A", l, A[l]->num_rows, A[l]->num_cols, dtype);
        if (A[l]->num_rows != A[l]->num_cols) fail(BMSP_ERR_INVALID, "A[%d]: must be square (it is %d x %d)", l, A[l]->num_rows, A[l]->num_cols);
    }
    for (int l = 0; l + 1 < levels; l++) {  // (the level operators first: the shapes of P and R are named against them)
        check_operator(P[l], "P", l, A[l]->num_rows, A[l + 1]->num_rows, dtype);
        if (R && R[l]) check_operator(R[l], "R", l, A[l + 1]->num_rows, A[l]->num_rows, dtype);
    }
    const int64_t nc = A[levels - 1]->num_rows;
    if (d_coarse_inv && nc > kMaxCoarse) fail(BMSP_ERR_INVALID, "d_coarse_inv: the coarsest level has %lld rows, at most %lld with an inverse", (long long)nc, (long long)kMaxCoarse);
    if (d_coarse_inv && ld_inv < nc) fail(BMSP_ERR_INVALID, "ld_inv must be >= the rows of the coarsest level (%lld; got %lld)", (long long)nc, (long long)ld_inv);
}

// (the arguments were checked at the C boundary: mg_check_args, mg_check_operands)
bmsp_mg_s *mg_create(int levels, bmsp_matrix_s *const *A, bmsp_matrix_s *const *P, bmsp_matrix_s *const *R, const void *d_coarse_inv,
                     int64_t ld_inv, double omega, int pre, int post, hipStream_t st)
{
    const bmsp_dtype dtype = A[0]->dtype;
    const int64_t nc = A[levels - 1]->num_rows;
    std::unique_ptr<bmsp_mg_s> mg(new bmsp_mg_s());
    mg->levels = levels; mg->pre = pre; mg->post = post; mg->omega = omega; mg->dtype = dtype; mg->exact = d_coarse_inv != nullptr;
    const size_t es = vec_size(mg.get());
    size_t dbytes = 0, wbytes = 0;
    for (int l = 0; l < levels; l++) {
        mg->A.push_back(A[l]);
        mg->P.push_back(l + 1 < levels ? P[l] : nullptr);
        mg->R.push_back(l + 1 < levels && R ? R[l] : nullptr);
        const int64_t n = A[l]->num_rows;
        mg->n.push_back(n);
        const size_t vb = round256(es * (size_t)n);
        mg->off_diag.push_back(dbytes);
        dbytes += vb;
        mg->off_rhs.push_back(wbytes);
        if (l > 0) wbytes += vb;
        mg->off_x0.push_back(wbytes);
        if (l > 0) wbytes += vb;
        mg->off_x1.push_back(wbytes);
        wbytes += vb;
        mg->off_t.push_back(wbytes);
        wbytes += vb;
    }
    mg->diag.alloc(dbytes);
    mg->work.alloc(wbytes);
    mg->work_bytes = dbytes + wbytes;
    for (int l = 0; l < levels; l++) {
        ensure_rowptr(A[l], st);
        if (mg->n[(size_t)l]) matrix_diagonal(A[l], (char *)mg->diag.p + mg->off_diag[(size_t)l], st);
        if (l + 1 < levels) {
            ensure_rowptr(P[l], st);
            if (mg->R[(size_t)l]) ensure_rowptr(mg->R[(size_t)l], st);
        }
    }
    if (mg->exact) {
        mg->inv.alloc(es * (size_t)nc * (size_t)nc);
        mg->work_bytes += es * (size_t)nc * (size_t)nc;
        const uint64_t un = (uint64_t)nc;
        if (dtype == BMSP_F64) device_for_each(TransposeInverse<double>{(const double *)d_coarse_inv, (double *)mg->inv.p, un, (uint64_t)ld_inv}, un * un, st);
        else device_for_each(TransposeInverse<float>{(const float *)d_coarse_inv, (float *)mg->inv.p, un, (uint64_t)ld_inv}, un * un, st);
    }
    BMSP_HIP(hipStreamSynchronize(st));  // (the caller's inverse has been read: it may go)
    return mg.release();
}

void mg_free(bmsp_mg_s *mg)
{
    if (!mg) return;
    delete mg;  // (as bmsp_matrix_free: no synchronisation here; the caller lets what it enqueued on the handle finish first)
}

void mg_vcycle(bmsp_mg_s *mg, const void *r, void *z, const int *stopped, hipStream_t st)
{
    if (mg->n[0] == 0) return;
    Cycle c{mg, stopped, st};
    c.run(0, r, z);
}

void mg_info(bmsp_mg_s *mg, bmsp_mg_info_t *info)
{
    memset(info, 0, sizeof *info);
    info->levels = mg->levels; info->pre = mg->pre; info->post = mg->post; info->coarse_exact = mg->exact ? 1 : 0;
    for (int l = 0; l < mg->levels; l++) {
        info->n[l] = mg->n[(size_t)l];
        info->restrict_mode[l] = l + 1 < mg->levels ? restrict_mode(mg, l) : -1;
    }
    info->workspace_bytes = (int64_t)mg->work_bytes;
    const char *dt = mg->dtype == BMSP_F64 ? "F64" : "F32";
    if (mg->n[0] == 0) {
        snprintf(info->kernel, sizeof info->kernel, "none (empty matrix)");
        snprintf(info->coarse_kernel, sizeof info->coarse_kernel, "none (empty matrix)");
        return;
    }
    const int walk = walk_of(mg->A[0]);
    snprintf(info->kernel, sizeof info->kernel, "mg_row_kernel<%s, %s, %s>", dt, mg->A[0]->transposed ? "MINOR" : "MAJOR",
             walk == kWalkWave ? "wave" : (walk == 4 ? "group4" : "group1"));
    if (mg->exact) snprintf(info->coarse_kernel, sizeof info->coarse_kernel, "mg_dense_kernel<%s>", dt);
    else snprintf(info->coarse_kernel, sizeof info->coarse_kernel, "mg_row_kernel<%s, %s> (%d Jacobi steps)", dt, mg->A[(size_t)mg->levels - 1]->transposed ? "MINOR" : "MAJOR", mg->pre + mg->post);
    Cycle c{mg, nullptr, nullptr};
    c.dry = true;
    c.run(0, nullptr, nullptr);
    info->launches_per_cycle = c.launches;
}

// a first call that restricts by a view of bmsp_spmv_op -- (P, T), or (R, N) of a column-major R -- builds it before the iteration is
// enqueued, not in the middle of it (a row-major R under op N is bmsp_spmv's, whose own first call builds its plan)
static void ensure_restriction_views(bmsp_mg_s *mg, hipStream_t st)
{
    for (int l = 0; l + 1 < mg->levels && mg->n[0]; l++) {
        const int mode = restrict_mode(mg, l);
        if (mode == BMSP_MG_RESTRICT_PT) spmv_op_ensure_view(mg->P[(size_t)l], BMSP_OP_T, st);
        else if (mode == BMSP_MG_RESTRICT_SPMV && mg->R[(size_t)l]->transposed) spmv_op_ensure_view(mg->R[(size_t)l], BMSP_OP_N, st);
    }
}

SolvePc mg_solve_pc(bmsp_mg_s *mg, hipStream_t st, bmsp_matrix_s **A)
{
    ensure_restriction_views(mg, st);
    *A = mg->A[0];
    SolvePc pc;
    pc.hook = [](void *h, const void *in, void *out, const int *stopped, hipStream_t s) { mg_vcycle((bmsp_mg_s *)h, in, out, stopped, s); };
    pc.handle = mg;
    pc.name = "mg";
    return pc;
}

}  // namespace bmsp

BMSP_DEFINE_WARM(multigrid)
