// spmm_op.hip -- Y = alpha * op(A) * X + beta * Y for k vectors, op in {N, T} and either tile layout (bmsp_spmm_op), without
// materialising A^T or a second layout: the multi-vector form of spmv_op.hip, on the SAME cached view (records in the order of the output
// blocks, work items of at most SPLIT tiles, fold list; spmv_op_ensure_view).
//
// What k vectors change: the single-vector sweep spends its time on the per-tile decode and a chain of dependent loads for 1.5 values per
// tile; here a lane owns a COLUMN of X and Y, so one decode of a tile feeds up to W multiply-adds per stored value and the X row of a stored
// value is one coalesced request of its lane group.
//
// Kernels:
//   sweep<S, MINOR, W>  a wave takes one work item; its 64 lanes are 64 / W tile slots x W columns.  Slot g walks tiles g, g + 64 / W, ... of
//                       the item; every lane keeps eight accumulators, one per output of the block, statically indexed (the loop over the
//                       outputs is unrolled: byte j of the bitmap for MAJOR, the positions 8i + j for MINOR, as in the single-vector sweep).
//                       Per stored value: one value load (uniform in the group), one load of X[8 * other + idx][c], one multiply-add; an
//                       unstored position loads nothing.  The slot sums meet in a fixed xor tree of wave shuffles.  W = 64: one slot, the
//                       record, the bit walk and the value are wave-uniform and kept scalar.  Columns beyond W are further column chunks
//                       (grid dimension y).  A whole-block item applies the epilogue and stores Y; an item of a split block stores its
//                       8 x chunk partial sums to its scratch slot.
//   fold<R>             a lane per (split block, output, column): the parts added in item order, epilogue, store.
//   epilogue<R>         (N, layout 0) with alpha != 1 or beta != 0: bmsp_spmm's sum from the temporary, scaled into the strided Y.
// Every output has one writer and every sum a fixed order: no atomic anywhere.
#include "tile_pass.hip.h"
#include <cstring>
#include <vector>

namespace bmsp {
namespace {

constexpr uint32_t kWhole = ~0u;  // an item's scratch slot when it is a whole output block (spmv_op.hip)
constexpr unsigned kMaxGridY = 65535;

template <typename S, bool MINOR, int W>
__global__ __launch_bounds__(kThreads) void spmm_op_sweep_kernel(const uint4 *__restrict__ recs, const uint4 *__restrict__ items,
                                                                 uint32_t n_items, const S *__restrict__ vals, const S *__restrict__ X,
                                                                 uint64_t ldx, typename TileValue<S>::R alpha, typename TileValue<S>::R beta,
                                                                 typename TileValue<S>::R *Y, uint64_t ldy,
                                                                 typename TileValue<S>::R *__restrict__ scratch, int64_t out_len, uint32_t k,
                                                                 uint32_t n_chunks)
{
    using D = TileValue<S>;
    using F = typename D::F;
    constexpr int G = 64 / W;  // tile slots of a wave
    const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kThreads / kWave) + (uint32_t)wave_id()));
    if (item >= n_items) return;  // (the whole wave)
    uint4 it = items[item];       // {output block, first tile, end tile, scratch slot}
    it.x = (uint32_t)__builtin_amdgcn_readfirstlane((int)it.x);
    it.y = (uint32_t)__builtin_amdgcn_readfirstlane((int)it.y);
    it.z = (uint32_t)__builtin_amdgcn_readfirstlane((int)it.z);
    it.w = (uint32_t)__builtin_amdgcn_readfirstlane((int)it.w);
    const uint32_t c0 = (uint32_t)lane_id() % W, g = (uint32_t)lane_id() / W;
    for (uint32_t chunk = blockIdx.y; chunk < n_chunks; chunk += gridDim.y) {
        const uint32_t c = chunk * W + c0;
        const bool cok = c < k;
        F acc[8];
#pragma unroll
        for (int j = 0; j < 8; j++) acc[j] = F(0);
        for (uint32_t t = it.y + g; t < it.z; t += G) {
            uint4 r = recs[t];
            if (G == 1) {  // one slot: the record is the wave's
                r.x = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.x);
                r.y = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.y);
                r.z = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.z);
                r.w = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.w);
            }
            const uint64_t bmp = (uint64_t)r.y << 32 | r.x;
            const S *tv = vals + r.z;
            const S *tx = X + (uint64_t)r.w * 8 * ldx + c;  // only stored entries index its rows: never beyond the matrix
            if (!MINOR) {
                int n = 0;  // values are stored in position order: byte after byte
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    uint32_t byte = tile_byte(bmp, j);
                    while (byte) {
                        const int i = __builtin_clz(byte) - 24;
                        byte &= ~(0x80u >> i);
                        const F a = D::load(tv[n++]);
                        const F x = cok ? D::load(tx[(uint64_t)i * ldx]) : F(0);
                        acc[j] += a * x;
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    uint64_t m = bmp & (0x8080808080808080ull >> j);  // positions 8i + j
                    while (m) {
                        const int p = tile_pop_first(m);
                        const F a = D::load(tv[tile_rank(bmp, p)]);
                        const F x = cok ? D::load(tx[(uint64_t)(p >> 3) * ldx]) : F(0);
                        acc[j] += a * x;
                    }
                }
            }
        }
        if (G > 1) {  // (every lane of the wave arrives: the loop's trip counts differ, the shuffles follow it)
#pragma unroll
            for (int j = 0; j < 8; j++) {
#pragma unroll
                for (int d = W; d < 64; d <<= 1) acc[j] += __shfl_xor(acc[j], d, kWave);
            }
        }
        if (g != 0 || !cok) continue;
        if (it.w != kWhole) {
            F *s = scratch + (uint64_t)it.w * 8 * k + c;
#pragma unroll
            for (int j = 0; j < 8; j++) s[(uint64_t)j * k] = acc[j];
            continue;
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int64_t o = (int64_t)it.x * 8 + j;
            if (o < out_len) {  // (the ragged last block)
                const int64_t e = o * (int64_t)ldy + c;
                Y[e] = spmv_op_epilogue<F>(alpha, acc[j], beta, Y, e);
            }
        }
    }
}

// folds: {output block, first scratch slot, parts} per split block; a slot holds 8 x k sums; the parts are added in item order
template <typename R>
__global__ __launch_bounds__(kThreads) void spmm_op_fold_kernel(const uint32_t *__restrict__ folds, uint64_t n, const R *__restrict__ scratch,
                                                                R alpha, R beta, R *Y, uint64_t ldy, int64_t out_len, uint32_t k)
{
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;  // (split block, output, column)
    if (gid >= n) return;
    const uint32_t c = (uint32_t)(gid % k);
    const uint64_t fj = gid / k, f = fj >> 3;
    const int j = (int)(fj & 7);
    const uint32_t block = folds[3 * f], first = folds[3 * f + 1], parts = folds[3 * f + 2];
    const R *s = scratch + ((uint64_t)first * 8 + j) * k + c;
    R acc = s[0];
    for (uint32_t p = 1; p < parts; p++) acc += s[(uint64_t)p * 8 * k];
    const int64_t o = (int64_t)block * 8 + j;
    if (o < out_len) {
        const int64_t e = o * (int64_t)ldy + c;
        Y[e] = spmv_op_epilogue<R>(alpha, acc, beta, Y, e);
    }
}

// t: out_len x k, unit stride
template <typename R>
__global__ __launch_bounds__(kThreads) void spmm_op_epilogue_kernel(const R *__restrict__ t, R alpha, R beta, R *Y, uint64_t ldy, uint64_t n,
                                                                    uint32_t k)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t e = (int64_t)((i / k) * ldy + i % k);
    Y[e] = spmv_op_epilogue<R>(alpha, t[i], beta, Y, e);
}

// W: the smallest lane group that min(k, 64) columns fill, or what BMSP_SPMM_OP_LANES forces
int lanes_for(int k)
{
    if (const char *e = getenv("BMSP_SPMM_OP_LANES")) {
        const int w = atoi(e);
        if (w == 8 || w == 16 || w == 32 || w == 64) return w;
    }
    return k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64;
}

int64_t scratch_elems(const bmsp_spmv_op_view &w, int k)
{
    if ((uint64_t)w.slots * 8 * (uint64_t)k > 0xffffffffull)
        fail(BMSP_ERR_LIMIT, "spmm_op: %lld scratch slots of 8 x %d sums exceed 2^32 - 1 elements", (long long)w.slots, k);
    return w.slots * 8 * (int64_t)k;
}

// a buffer on the handle that only grows; growing waits for the work enqueued on the old one
void grow(DevBuf<void> &buf, int64_t &have, int64_t need, size_t elem, hipStream_t st)
{
    if (need <= have && buf) return;
    if (buf) BMSP_HIP(hipStreamSynchronize(st));
    buf.release(); have = 0;
    buf.alloc(elem * (size_t)(need ? need : 1));
    have = need;
}

template <typename S, bool MINOR, int W>
void launch_sweep_w(const bmsp_matrix_s *A, const bmsp_spmv_op_view &w, int64_t out_len, double alpha, const void *X, int64_t ldx, double beta,
                    void *Y, int64_t ldy, int k, hipStream_t st)
{
    using R = typename TileValue<S>::R;
    const char *mem = (const char *)w.mem;
    const uint32_t chunks = (uint32_t)ceil_div(k, W);
    dim3 grid = grid_for((uint64_t)w.items * kWave);
    grid.y = chunks < kMaxGridY ? chunks : kMaxGridY;
    hipLaunchKernelGGL((spmm_op_sweep_kernel<S, MINOR, W>), grid, dim3(kThreads), 0, st, (const uint4 *)mem, (const uint4 *)(mem + w.off_items),
                       (uint32_t)w.items, (const S *)A->values, (const S *)X, (uint64_t)ldx, (R)alpha, (R)beta, (R *)Y, (uint64_t)ldy,
                       (R *)A->spmm_op_scratch, out_len, (uint32_t)k, chunks);
    BMSP_CHECK_LAUNCH();
}

template <typename S, bool MINOR>
void launch_sweep(const bmsp_matrix_s *A, const bmsp_spmv_op_view &w, int lanes, int64_t out_len, double alpha, const void *X, int64_t ldx,
                  double beta, void *Y, int64_t ldy, int k, hipStream_t st)
{
    using R = typename TileValue<S>::R;
    switch (lanes) {
    case 8: launch_sweep_w<S, MINOR, 8>(A, w, out_len, alpha, X, ldx, beta, Y, ldy, k, st); break;
    case 16: launch_sweep_w<S, MINOR, 16>(A, w, out_len, alpha, X, ldx, beta, Y, ldy, k, st); break;
    case 32: launch_sweep_w<S, MINOR, 32>(A, w, out_len, alpha, X, ldx, beta, Y, ldy, k, st); break;
    default: launch_sweep_w<S, MINOR, 64>(A, w, out_len, alpha, X, ldx, beta, Y, ldy, k, st); break;
    }
    if (w.split_blocks) {
        const uint64_t n = (uint64_t)w.split_blocks * 8 * (uint64_t)k;
        hipLaunchKernelGGL((spmm_op_fold_kernel<R>), grid_for(n), dim3(kThreads), 0, st, (const uint32_t *)((const char *)w.mem + w.off_folds), n,
                           (const R *)A->spmm_op_scratch, (R)alpha, (R)beta, (R *)Y, (uint64_t)ldy, out_len, (uint32_t)k);
        BMSP_CHECK_LAUNCH();
    }
}

template <typename R>
void launch_epilogue(const void *t, double alpha, double beta, void *Y, int64_t ldy, int64_t out_len, int k, hipStream_t st)
{
    const uint64_t n = (uint64_t)out_len * (uint64_t)k;
    if (n == 0) return;
    hipLaunchKernelGGL((spmm_op_epilogue_kernel<R>), grid_for(n), dim3(kThreads), 0, st, (const R *)t, (R)alpha, (R)beta, (R *)Y, (uint64_t)ldy, n,
                       (uint32_t)k);
    BMSP_CHECK_LAUNCH();
}

// bmsp_spmm's own case: its sum, then the epilogue (the call itself when the epilogue is the identity)
void spmm_plain(bmsp_matrix_s *A, double alpha, const void *X, int64_t ldx, double beta, void *Y, int64_t ldy, int k, hipStream_t st)
{
    const bool f64 = A->dtype == BMSP_F64;
    const bool identity = f64 ? (alpha == 1.0 && beta == 0.0) : ((float)alpha == 1.0f && (float)beta == 0.0f);
    if (identity) {
        spmm(A, X, ldx, Y, ldy, k, st);
        return;
    }
    grow(A->spmm_op_tmp, A->spmm_op_tmp_elems, (int64_t)A->num_rows * k, spmv_op_vector_size(A), st);
    spmm(A, X, ldx, A->spmm_op_tmp, k, k, st);
    if (f64) launch_epilogue<double>(A->spmm_op_tmp, alpha, beta, Y, ldy, A->num_rows, k, st);
    else launch_epilogue<float>(A->spmm_op_tmp, alpha, beta, Y, ldy, A->num_rows, k, st);
}

// X rows the tiles read, each counted once per tile: the input side of a tile is the bit index (MAJOR) or the byte index (MINOR)
int64_t count_x_rows(const bmsp_matrix_s *A, bool minor)
{
    std::vector<uint64_t> bmps((size_t)A->block_num);
    if (A->block_num) {
        BMSP_HIP(hipDeviceSynchronize());
        copy_d2h_staged(bmps.data(), A->bmps, 8 * bmps.size());
    }
    int64_t rows = 0;
    for (uint64_t b : bmps) {
        if (!minor) { rows += __builtin_popcount(tile_or_bytes(b)); continue; }
        for (int i = 0; i < 8; i++) rows += tile_byte(b, i) != 0;
    }
    return rows;
}

}  // namespace

void spmm_op_check_args(int op, int k, int64_t ldx, int64_t ldy)
{
    spmv_op_check_op(op);
    if (k < 1) fail(BMSP_ERR_INVALID, "k must be >= 1 (got %d)", k);
    if (ldx < k) fail(BMSP_ERR_INVALID, "ldx must be >= k (got %lld, k = %d)", (long long)ldx, k);
    if (ldy < k) fail(BMSP_ERR_INVALID, "ldy must be >= k (got %lld, k = %d)", (long long)ldy, k);
}

void spmm_op(bmsp_matrix_s *A, int op, double alpha, const void *X, int64_t ldx, double beta, void *Y, int64_t ldy, int k, hipStream_t st)
{
    spmm_op_check_args(op, k, ldx, ldy);
    spmv_op_check_matrix(A, "spmm_op");
    if (op == BMSP_OP_N && !A->transposed) {
        spmm_plain(A, alpha, X, ldx, beta, Y, ldy, k, st);
        return;
    }
    const bmsp_spmv_op_view &w = spmv_op_ensure_view(A, op, st);
    if (w.items == 0) return;  // no output
    const int lanes = lanes_for(k);
    if (w.slots) grow(A->spmm_op_scratch, A->spmm_op_scratch_elems, scratch_elems(w, k), spmv_op_vector_size(A), st);
    const int64_t out_len = spmv_op_out_length(A, op);
    const bool minor = (op == BMSP_OP_T) != (A->transposed != 0);
    dispatch_dtype(A->dtype, [&](auto s) {
        using S = decltype(s);
        if (minor) launch_sweep<S, true>(A, w, lanes, out_len, alpha, X, ldx, beta, Y, ldy, k, st);
        else launch_sweep<S, false>(A, w, lanes, out_len, alpha, X, ldx, beta, Y, ldy, k, st);
    });
}

// The launcher's own decisions for (A, op, k) -- lanes_for and the view are what spmm_op itself uses -- and the bytes the launch moves
// (the counting rule is in bmsp.h).  (N, layout 0) is bmsp_spmm: its name behind "bmsp_spmm: ", no view.
void spmm_op_launch_info(bmsp_matrix_s *A, int op, int k, int64_t ldx, int64_t ldy, hipStream_t st, bmsp_spmm_op_info *info)
{
    spmm_op_check_args(op, k, ldx, ldy);
    spmv_op_check_matrix(A, "spmm_op");
    memset(info, 0, sizeof *info);
    const int64_t as = (int64_t)spmv_op_vector_size(A);
    if (op == BMSP_OP_N && !A->transposed) {
        char name[48];
        spmm_launch_info(A, k, ldx, ldy, st, name, sizeof name);  // the alpha == 1, beta == 0 call: bmsp_spmm into Y
        snprintf(info->kernel, sizeof info->kernel, "bmsp_spmm: %s", name);
        info->view_bytes = info->scratch_bytes = A->spmm_op_tmp ? as * A->spmm_op_tmp_elems : 0;
        return;
    }
    const bmsp_spmv_op_view &w = spmv_op_ensure_view(A, op, st);
    const bool minor = (op == BMSP_OP_T) != (A->transposed != 0);
    info->items = w.items;
    info->split_blocks = w.split_blocks;
    info->view_bytes = (int64_t)w.bytes;
    if (w.items == 0) {
        snprintf(info->kernel, sizeof info->kernel, "none (no output)");
        return;
    }
    info->lanes = lanes_for(k);
    info->col_chunks = (int)ceil_div(k, info->lanes);
    info->scratch_bytes = as * scratch_elems(w, k);
    snprintf(info->kernel, sizeof info->kernel, "spmm_op_sweep_kernel<%s, %d>", minor ? "MINOR" : "MAJOR", info->lanes);
    const int64_t es = (int64_t)dtype_size(A->dtype);
    info->compulsory_bytes = info->col_chunks * (16 * A->block_num + 16 * w.items + es * A->nnz) + es * k * count_x_rows(A, minor) +
                             as * spmv_op_out_length(A, op) * k + 2 * info->scratch_bytes + 12 * w.split_blocks;
}

}  // namespace bmsp

BMSP_DEFINE_WARM(spmm_op)
