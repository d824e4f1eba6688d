// spsm.hip -- the sparse triangular solve for k right-hand sides, op(tri(A)) * X = alpha * B (bmsp_spsm): column c of X holds, bit for
// bit, what bmsp_spsv writes for column c of B.  B and X are n x k, row-major with a leading dimension (bmsp_spmm's convention).
//
// What is reused (spsv_plan.hip.h): the tile records of (A, op) and the cached plan of (A, op, fill) -- the same levels, the same order,
// the same launch schedule, BMSP_SPSV_CHAIN with its meaning.  There is no second plan: one built by bmsp_spsv serves here and the other
// way round.
//
// What is new: the lane mapping.  The cost of a level is a chain of dependent loads whatever the lanes do, and the columns of B are
// independent, so one walk of the chain carries W columns.  A lane owns ONE column of X for one block-row, all eight rows of it, as eight
// sums in registers; the W lanes of a slot walk the same records, read the same bitmaps and values of A, and load the rows of X they
// depend on side by side (coalesced).  Columns beyond W go to further column chunks, independent of each other: the grid's second
// dimension.  Inside the diagonal tile a lane substitutes on its own (it holds the whole column of the block): no shuffle.
//   spsm_level_kernel  one launch per level, kThreads / W block-rows per workgroup, grid (ceil(width / slots), column chunks)
//   spsm_chain_kernel  one workgroup per column chunk walks a run of consecutive narrow levels, a workgroup barrier between two levels;
//                      X is stored and loaded again inside the workgroup, so X is never __restrict__ and never read through a read-only
//                      path
// Per row the chain of operations is that of spsv_block_row: s = fl(alpha * b), one fma(-a_ij, x_j, s) per stored entry of the effective
// strict triangle in the order of a sequential substitution, one IEEE division (or none).  Ordering comes from kernel boundaries and the
// workgroup barrier alone: no flag, no spin, no atomic, no cooperative launch.
#include "spsv_plan.hip.h"

namespace bmsp {
namespace {

constexpr int kDenseTile = 8;          // a tile of more stored values than this takes the four-rows-at-a-time path
constexpr unsigned kMaxGrid = 65535;  // column chunks per launch (grid y of the level kernel, grid x of the chain kernel); more are looped over

// positions of column c of a diagonal tile's strict triangle: the rows after c in chain order (the other side is never read)
template <bool MINOR, bool LOWER>
__host__ __device__ constexpr uint64_t strict_column_mask(int c)
{
    uint64_t m = 0;
    for (int i = 0; i < 8; i++)
        if (LOWER ? i > c : i < c) m |= 1ull << (63 - (MINOR ? 8 * c + i : 8 * i + c));
    return m;
}

// positions of a diagonal tile's strict triangle on the side that is read
template <bool MINOR, bool LOWER>
__host__ __device__ constexpr uint64_t strict_triangle_mask()
{
    uint64_t m = 0;
    for (int c = 0; c < 8; c++) m |= strict_column_mask<MINOR, LOWER>(c);
    return m;
}

// The W lanes of a slot solve block-row I for the columns [col0, col0 + W) of X, lane `col` its own column (col < k; the lanes of a
// ragged last chunk beyond k do not come here).  Every x the block-row depends on outside the block is final (an earlier launch, or an
// earlier level of this workgroup behind a barrier).  B may be X (in place, same stride): a lane reads its own eight elements of B before
// it writes them.
//
// A tile's bitmap and values are the same for every lane of the slot; what differs is the column of X.  The eight sums are unrolled so
// that they stay in registers; a row's values are fetched together (the address of an entry that is not stored falls back on the row's
// first value, which exists, and its product is discarded), so a row costs one round of loads, not one per entry -- four rows of a tile
// of more than kDenseTile values, and the whole triangle of the diagonal tile (measured: DESIGN §4 "Triangular solve, several
// right-hand sides").
template <typename S, bool MINOR, bool LOWER, bool UNIT>
__device__ __forceinline__ void spsm_block_row(const SpsvTiles &T, const uint32_t *__restrict__ ptr, const S *__restrict__ vals,
                                               typename TileValue<S>::R alpha, const typename TileValue<S>::R *B, uint64_t ldb,
                                               typename TileValue<S>::R *X, uint64_t ldx, int64_t n, uint32_t I, uint32_t col)
{
#pragma clang fp contract(off)
    using D = TileValue<S>;
    using F = typename D::F;
    const int64_t o = (int64_t)I * 8;
    F s[8];
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = o + i < n ? alpha * B[(uint64_t)(o + i) * ldb + col] : F(0);  // (rows beyond n: nothing stored, not written)
    int64_t t = LOWER ? (int64_t)ptr[I] : (int64_t)ptr[I + 1] - 1;
    const int64_t end = LOWER ? (int64_t)ptr[I + 1] : (int64_t)ptr[I] - 1;
    uint4 r = make_uint4(0u, 0u, 0u, 0u), next = r;
    bool diag = false;
    if (t != end) next = spsv_rec(T, (uint64_t)t);
    for (; t != end; t += LOWER ? 1 : -1) {
        r = next;
        if (LOWER ? r.w >= I : r.w <= I) {  // the diagonal tile, or the first tile of the triangle that is not read
            diag = r.w == I;
            break;
        }
        // the next record of the block-row is on its way while this tile's values and X arrive (records do not depend on X)
        const int64_t tn = t + (LOWER ? 1 : -1);
        if (tn != end) next = spsv_rec(T, (uint64_t)tn);
        const uint64_t bmp = (uint64_t)r.y << 32 | r.x;
        const S *tv = vals + r.z;
        // the rows of X the tile's stored entries index (never beyond the matrix: a stored entry has a column below n)
        F xr[8];
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const bool used = MINOR ? tile_byte(bmp, c) != 0 : ((tile_or_bytes(bmp) >> (7 - c)) & 1u) != 0;
            xr[c] = used ? X[((uint64_t)r.w * 8 + c) * ldx + col] : F(0);
        }
        if (popc64(bmp) > kDenseTile) {
            // a dense tile, four rows at a time: their 32 value loads are in flight together (one round of latency, not one per row)
#pragma unroll
            for (int h = 0; h < 8; h += 4) {
                uint64_t half = 0;
#pragma unroll
                for (int i = h; i < h + 4; i++) half |= MINOR ? bmp & (0x8080808080808080ull >> i) : bmp & tile_byte_mask(i);
                if (!half) continue;
                const int first = tile_rank(bmp, __builtin_clzll(half));
                F a[4][8];
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int c = 0; c < 8; c++) {
                        const int p = MINOR ? 8 * c + h + i : 8 * (h + i) + c;
                        a[i][c] = D::load(tv[tile_has(bmp, p) ? tile_rank(bmp, p) : first]);
                    }
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int k = 0; k < 8; k++) {
                        const int c = LOWER ? k : 7 - k;
                        const F u = fused(-a[i][c], xr[c], s[h + i]);
                        if (tile_has(bmp, MINOR ? 8 * c + h + i : 8 * (h + i) + c)) s[h + i] = u;
                    }
            }
            continue;
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
            // row i of the tile: byte i (MAJOR), or bit i of every byte (MINOR)
            const uint64_t row = MINOR ? bmp & (0x8080808080808080ull >> i) : bmp & tile_byte_mask(i);
            if (!row) continue;
            const int first = tile_rank(bmp, __builtin_clzll(row));  // the row's first stored value
            F a[8];
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const int p = MINOR ? 8 * c + i : 8 * i + c;
                a[c] = D::load(tv[tile_has(bmp, p) ? tile_rank(bmp, p) : first]);
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int c = LOWER ? k : 7 - k;  // ascending for a lower system, descending for an upper one
                const F u = fused(-a[c], xr[c], s[i]);
                if (tile_has(bmp, MINOR ? 8 * c + i : 8 * i + c)) s[i] = u;
            }
        }
    }
    if (diag) {
        // every value the substitution reads is fetched before its first step (the address of an entry that is not stored, or not read,
        // falls back on a value that is read): the eight steps then wait for arithmetic only
        const uint64_t bmp = (uint64_t)r.y << 32 | r.x;
        const S *tv = vals + r.z;
        constexpr uint64_t kRead = strict_triangle_mask<MINOR, LOWER>() | (UNIT ? 0ull : 0x8040201008040201ull);  // (tile_diagonal_mask())
        const uint64_t read = bmp & kRead;
        if (read) {
            const int first = tile_rank(bmp, __builtin_clzll(read));
            F a[8][8];
#pragma unroll
            for (int i = 0; i < 8; i++)
#pragma unroll
                for (int c = 0; c < 8; c++) {
                    const int p = MINOR ? 8 * c + i : 8 * i + c;
                    if ((kRead >> (63 - p)) & 1ull) a[i][c] = D::load(tv[tile_has(bmp, p) ? tile_rank(bmp, p) : first]);
                }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int c = LOWER ? k : 7 - k;
                // x_c: every entry of row c inside the block has been taken in
                if (!UNIT) {
                    const F q = s[c] / a[c][c];
                    if (tile_has(bmp, 9 * c)) s[c] = q;
                }
                // column c of the strict triangle: the rows after c in chain order that store (i, c)
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    if (LOWER ? i <= c : i >= c) continue;
                    const F u = fused(-a[i][c], s[c], s[i]);
                    if (tile_has(bmp, MINOR ? 8 * c + i : 8 * i + c)) s[i] = u;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (o + i < n) X[(uint64_t)(o + i) * ldx + col] = s[i];
}

// block-rows order[first .. first + width) of one level, the column chunks along grid y
template <typename S, bool MINOR, bool LOWER, bool UNIT, int W>
__global__ __launch_bounds__(kThreads) void spsm_level_kernel(SpsvTiles T, const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ order,
                                                              uint32_t first, uint32_t width, const S *__restrict__ vals,
                                                              typename TileValue<S>::R alpha, const typename TileValue<S>::R *B, uint64_t ldb,
                                                              typename TileValue<S>::R *X, uint64_t ldx, int64_t n, uint32_t k, uint32_t chunks)
{
    constexpr uint32_t kSlots = kThreads / W;
    const uint64_t g = (uint64_t)blockIdx.x * kSlots + threadIdx.x / W;
    if (g >= width) return;
    const uint32_t I = order[first + g];
    for (uint32_t ch = blockIdx.y; ch < chunks; ch += gridDim.y) {
        const uint32_t col = ch * W + threadIdx.x % W;
        if (col < k) spsm_block_row<S, MINOR, LOWER, UNIT>(T, ptr, vals, alpha, B, ldb, X, ldx, n, I, col);
    }
}

// levels [l0, l1) by one workgroup per column chunk; the loops are uniform, the barrier orders the stores to X of a level before the
// loads of the next (the chunks of one workgroup touch different columns: they need nothing of each other)
template <typename S, bool MINOR, bool LOWER, bool UNIT, int W>
__global__ __launch_bounds__(kThreads) void spsm_chain_kernel(SpsvTiles T, const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ order,
                                                              const uint32_t *__restrict__ level_ptr, uint32_t l0, uint32_t l1,
                                                              const S *__restrict__ vals, typename TileValue<S>::R alpha,
                                                              const typename TileValue<S>::R *B, uint64_t ldb, typename TileValue<S>::R *X,
                                                              uint64_t ldx, int64_t n, uint32_t k, uint32_t chunks)
{
    constexpr uint32_t kSlots = kThreads / W;
    const uint32_t g = threadIdx.x / W;
    for (uint32_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const uint32_t col = ch * W + threadIdx.x % W;
        for (uint32_t l = l0; l < l1; l++) {
            const uint64_t hi = level_ptr[l + 1];
            if (col < k)
                for (uint64_t j = (uint64_t)level_ptr[l] + g; j < hi; j += kSlots)
                    spsm_block_row<S, MINOR, LOWER, UNIT>(T, ptr, vals, alpha, B, ldb, X, ldx, n, order[j], col);
            __syncthreads();
        }
    }
}

// Measured (tools/spsm_bench.py; DESIGN §4 "Triangular solve, several right-hand sides"): the smallest lane group that min(k, 64)
// columns fill, or what BMSP_SPSM_LANES forces
int lanes_for(int k)
{
    if (const char *e = getenv("BMSP_SPSM_LANES")) {
        const int w = atoi(e);
        if (w == 8 || w == 16 || w == 32 || w == 64) return w;
    }
    return k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64;
}

template <typename S, bool MINOR, bool LOWER, bool UNIT, int W>
void launch_plan(const bmsp_matrix_s *A, const SpsvTiles &T, const uint32_t *ptr, const bmsp_spsv_plan_s &pl, double alpha, const void *B,
                 int64_t ldb, void *X, int64_t ldx, int k, hipStream_t st)
{
    using R = typename TileValue<S>::R;
    constexpr uint32_t kSlots = kThreads / W;
    const uint32_t *order = pl.mem, *level_ptr = (const uint32_t *)((const char *)pl.mem + pl.off_level_ptr);
    const uint32_t chunks = (uint32_t)ceil_div(k, W);
    const unsigned gc = chunks < kMaxGrid ? chunks : kMaxGrid;
    for (size_t s = 0; s < pl.segments.size(); s += 3) {
        const uint32_t l0 = pl.segments[s], l1 = pl.segments[s + 1];
        if (pl.segments[s + 2]) {
            hipLaunchKernelGGL((spsm_chain_kernel<S, MINOR, LOWER, UNIT, W>), dim3(gc), dim3(kThreads), 0, st, T, ptr, order, level_ptr, l0, l1,
                               (const S *)A->values, (R)alpha, (const R *)B, (uint64_t)ldb, (R *)X, (uint64_t)ldx, (int64_t)A->num_rows,
                               (uint32_t)k, chunks);
        } else {
            const uint32_t first = pl.level_ptr[l0], width = pl.level_ptr[l0 + 1] - first;
            dim3 grid = grid_for(width, kSlots);
            grid.y = gc;
            hipLaunchKernelGGL((spsm_level_kernel<S, MINOR, LOWER, UNIT, W>), grid, dim3(kThreads), 0, st, T, ptr, order, first, width,
                               (const S *)A->values, (R)alpha, (const R *)B, (uint64_t)ldb, (R *)X, (uint64_t)ldx, (int64_t)A->num_rows,
                               (uint32_t)k, chunks);
        }
        BMSP_CHECK_LAUNCH();
    }
}

template <typename S, bool MINOR, bool LOWER, bool UNIT, typename... Args>
void launch_lanes(int lanes, Args &&...args)
{
    switch (lanes) {
    case 8: launch_plan<S, MINOR, LOWER, UNIT, 8>(args...); break;
    case 16: launch_plan<S, MINOR, LOWER, UNIT, 16>(args...); break;
    case 32: launch_plan<S, MINOR, LOWER, UNIT, 32>(args...); break;
    default: launch_plan<S, MINOR, LOWER, UNIT, 64>(args...); break;
    }
}

template <typename S, bool MINOR, bool LOWER, typename... Args>
void launch_diag(bool unit, Args &&...args)
{
    if (unit) launch_lanes<S, MINOR, LOWER, true>(args...);
    else launch_lanes<S, MINOR, LOWER, false>(args...);
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

// k = 1 with unit strides IS bmsp_spsv
bool is_spsv(int k, int64_t ldb, int64_t ldx) { return k == 1 && ldb == 1 && ldx == 1; }

}  // namespace

void spsm_check_args(int op, int fill, int diag, int k, int64_t ldb, int64_t ldx)
{
    spsv_check_args(op, fill, diag);
    if (k < 1) fail(BMSP_ERR_INVALID, "k must be >= 1 (got %d)", k);
    if (ldb < k) fail(BMSP_ERR_INVALID, "ldb must be >= k (got %lld, k = %d)", (long long)ldb, k);
    if (ldx < k) fail(BMSP_ERR_INVALID, "ldx must be >= k (got %lld, k = %d)", (long long)ldx, k);
}

void spsm_check_in_place(const void *B, int64_t ldb, const void *X, int64_t ldx)
{
    if (B == X && ldb != ldx)
        fail(BMSP_ERR_INVALID, "ldx must equal ldb when d_X == d_B (in place) (got ldb = %lld, ldx = %lld)", (long long)ldb, (long long)ldx);
}

void spsm(bmsp_matrix_s *A, int op, int fill, int diag, double alpha, const void *B, int64_t ldb, void *X, int64_t ldx, int k, hipStream_t st)
{
    spsm_check_args(op, fill, diag, k, ldb, ldx);
    spsv_check_matrix(A);
    spsm_check_in_place(B, ldb, X, ldx);
    if (A->num_rows == 0) return;
    if (is_spsv(k, ldb, ldx)) {
        spsv(A, op, fill, diag, alpha, B, X, st);
        return;
    }
    const bmsp_spsv_plan_s &pl = ensure_plan(A, op, fill, st);
    refuse_missing_diagonal(pl, diag);
    const uint32_t *ptr = nullptr;
    const bmsp_spmv_op_view *w = view_of(A, op, st, &ptr);  // (both exist: the plan was made from them)
    const SpsvTiles T = tiles_of(A, w);
    const bool minor = (op == BMSP_OP_T) != (A->transposed != 0);
    const int lanes = lanes_for(k);
    dispatch_dtype(A->dtype, [&](auto s) {
        using S = decltype(s);
        launch_variant<S>(minor, effective_lower(op, fill), diag == BMSP_DIAG_UNIT, lanes, A, T, ptr, pl, alpha, B, ldb, X, ldx, k, st);
    });
}

// The launcher's own decisions for (A, op, fill, diag, k, strides): lanes_for, is_spsv and the plan are what spsm itself uses.
void spsm_launch_info(bmsp_matrix_s *A, int op, int fill, int diag, int k, int64_t ldb, int64_t ldx, hipStream_t st, bmsp_spsm_info *info)
{
    spsm_check_args(op, fill, diag, k, ldb, ldx);
    spsv_check_matrix(A);
    bmsp_spsv_info si;
    spsv_analyse(A, op, fill, diag, st, &si);  // builds the plan if it is missing; refuses a missing diagonal
    memset(info, 0, sizeof *info);
    info->levels = si.levels;
    info->launches = si.launches;
    info->chain_launches = si.chain_launches;
    info->chained_levels = si.chained_levels;
    info->plan_bytes = si.plan_bytes;
    if (A->num_rows == 0) {
        snprintf(info->kernel, sizeof info->kernel, "none (empty matrix)");
        return;
    }
    if (is_spsv(k, ldb, ldx)) {
        snprintf(info->kernel, sizeof info->kernel, "bmsp_spsv: %s", si.kernel);
        info->lanes = 8;
        info->col_chunks = 1;
        return;
    }
    const bool minor = (op == BMSP_OP_T) != (A->transposed != 0);
    info->lanes = lanes_for(k);
    info->col_chunks = (int)ceil_div(k, info->lanes);
    snprintf(info->kernel, sizeof info->kernel, "spsm_level_kernel<%s, %s, %s, %s, %d>",
             A->dtype == BMSP_F16 ? "F16" : (A->dtype == BMSP_F32 ? "F32" : "F64"), minor ? "MINOR" : "MAJOR",
             effective_lower(op, fill) ? "LOWER" : "UPPER", diag == BMSP_DIAG_UNIT ? "UNIT" : "NON_UNIT", info->lanes);
}

}  // namespace bmsp

BMSP_DEFINE_WARM(spsm)
