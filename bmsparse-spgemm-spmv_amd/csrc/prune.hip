// prune.hip -- drops stored entries of a matrix already on the device (bmsp_matrix_prune / bmsp_matrix_row_absmax), without going back
// through scalar COO entries.
//
// An entry goes iff |v| <= tol (BMSP_PRUNE_ABS) or |v| <= tol * rowmax(its row) (BMSP_PRUNE_ROW_REL), compared in double on the exactly
// widened stored value; NaN is never dropped (the comparison is false).  Tiles keep their order and their keys in both layouts, so the
// output is a COMPACTION of A's tile list: nothing is sorted, nothing is searched.
//
// Passes:
//   rowmax  (ROW_REL, row_absmax) G lanes per tile: a lane takes the maximum of |v| over the rows of its tile (all eight, or row t of
//           eight lanes), as the BITS of the non-negative value (they order as unsigned integers; NaN bits lie above +Inf and are
//           skipped).  The tiles of a block-row are neighbours in the tile list, so the lanes of a wave that hold the same block-row
//           combine with a segmented shuffle scan and only the last of them issues an integer atomic max per row: a hub block-row of
//           n tiles costs n / 64 (G = 1) or n / 8 (G = 8) atomics per row, not n.  Max is exact and order-independent.
//   mark    G lanes per tile: the kept bitmap in A's layout (G = 8: a lane per bitmap byte, OR'd across the eight lanes).  The diagonal
//           of a tile with block_row == block_col is the positions 0, 9, .., 63 in either layout.
//   scan, place   the compaction selection shares (tile_compact.hip.h): slot and value offset of every kept tile in one scan, whose total
//           is read back (count-only calls end there), then the move of the kept tiles and values as raw bits.
#include "tile_compact.hip.h"
#include <cmath>

namespace bmsp {
namespace {

__device__ __forceinline__ void atomic_max_bits(uint32_t *p, uint32_t v) { atomicMax(p, v); }
__device__ __forceinline__ void atomic_max_bits(uint64_t *p, uint64_t v) { atomicMax((unsigned long long *)p, (unsigned long long)v); }

// rowmax[row] = max(rowmax[row], max |v| over the non-NaN stored entries of the row), as bits; the caller zeroes rowmax (num_rows entries).
// Every lane stays to the end: the shuffles need the whole wave.
template <typename S, int G>
__global__ __launch_bounds__(kThreads) void row_absmax_kernel(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ bmps,
                                                              const uint64_t *__restrict__ offsets, const S *__restrict__ vals, uint64_t nb,
                                                              int flip, int64_t num_rows, typename TileValue<S>::U *__restrict__ rowmax)
{
    using P = TileValue<S>;
    using U = typename P::U;
    constexpr int R = 8 / G;  // rows of the tile a lane takes
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t j = gid / G;
    const int t = (int)(gid % G);
    const bool live = j < nb;
    uint32_t brow = ~0u;
    U m[R];
#pragma unroll
    for (int i = 0; i < R; i++) m[i] = 0;
    if (live) {
        brow = key_row(keys[j]);
        const uint64_t ib = bmps[j];
        const uint64_t rb = flip ? tile_transpose(ib) : ib;  // row-major form: byte r = row r
        const S *src = vals + offsets[j];
#pragma unroll
        for (int i = 0; i < R; i++) {
            const int row = G == 1 ? i : t;
            uint32_t byte = tile_byte(rb, row);
            while (byte) {
                const int c = __builtin_clz(byte) - 24;
                byte &= ~(0x80u >> c);
                const int p = 8 * row + c;
                const U b = P::abs_bits(src[tile_rank(ib, flip ? tile_transposed_pos(p) : p)]);
                if (b <= P::kInf && b > m[i]) m[i] = b;
            }
        }
    }
    // segmented inclusive max over the lanes of one block-row (and, G = 8, of one tile row): they are G apart and contiguous
    const int lane = lane_id();
#pragma unroll
    for (int d = G; d < kWave; d <<= 1) {
        const uint32_t ob = __shfl_up(brow, d, kWave);
        const bool same = lane >= d && ob == brow;
#pragma unroll
        for (int i = 0; i < R; i++) {
            const U om = __shfl_up(m[i], d, kWave);
            if (same && om > m[i]) m[i] = om;
        }
    }
    const uint32_t nxt = __shfl_down(brow, G, kWave);
    if (!live || (lane + G < kWave && nxt == brow)) return;  // a later lane of the wave carries this block-row on
#pragma unroll
    for (int i = 0; i < R; i++) {
        const int64_t row = (int64_t)brow * 8 + (G == 1 ? i : t);
        if (m[i] && row < num_rows) atomic_max_bits(rowmax + row, m[i]);
    }
}

// kept[j]: the bits of tile j's bitmap (A's layout) whose entries stay
template <typename S, int G>
__global__ __launch_bounds__(kThreads) void prune_mark_kernel(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ bmps,
                                                              const uint64_t *__restrict__ offsets, const S *__restrict__ vals, uint64_t nb,
                                                              int transposed, int rule, double tol, int keep_diagonal,
                                                              const typename TileValue<S>::R *__restrict__ rowmax, uint64_t *__restrict__ kept)
{
    using P = TileValue<S>;
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t j = gid / G;
    const int t = (int)(gid % G);
    const bool live = j < nb;
    uint64_t keep = 0;
    if (live) {
        const uint64_t key = keys[j], ib = bmps[j];
        const uint64_t mine = G == 1 ? ib : ib & tile_byte_mask(t);
        const S *src = vals + offsets[j] + (G == 1 ? 0 : tile_rank(ib, 8 * t));
        const uint64_t row0 = (uint64_t)key_row(key) * 8;
        uint64_t m = mine;
        while (m) {
            const int p = tile_pop_first(m);
            const uint64_t bit = 1ull << (63 - p);
            const double a = fabs(P::widen(*src++));
            double thr = tol;
            if (rule == BMSP_PRUNE_ROW_REL) thr = tol * (double)rowmax[row0 + (transposed ? (p & 7) : (p >> 3))];  // one IEEE multiply
            if (!(a <= thr)) keep |= bit;  // NaN stays
        }
        if (keep_diagonal && key_row(key) == key_col(key)) keep |= mine & tile_diagonal_mask();
    }
    if (G == 8) {
        keep |= __shfl_xor(keep, 1, kWave);
        keep |= __shfl_xor(keep, 2, kWave);
        keep |= __shfl_xor(keep, 4, kWave);
    }
    if (live && t == 0) kept[j] = keep;
}

template <typename S>
void launch_row_absmax(int g, const bmsp_matrix_s *A, int64_t num_rows, void *rowmax, hipStream_t st)
{
    using U = typename TileValue<S>::U;
    const uint64_t nb = (uint64_t)A->block_num;
    launch_lane_group(g, nb, [&](auto lanes, dim3 grid) {
        hipLaunchKernelGGL((row_absmax_kernel<S, decltype(lanes)::value>), grid, dim3(kThreads), 0, st, A->keys, A->bmps, A->offsets,
                           (const S *)A->values, nb, A->transposed, num_rows, (U *)rowmax);
    });
}

template <typename S>
void launch_mark(int g, const bmsp_matrix_s *A, int rule, double tol, int flags, const void *rowmax, uint64_t *kept, hipStream_t st)
{
    using R = typename TileValue<S>::R;
    const uint64_t nb = (uint64_t)A->block_num;
    const int kd = flags & BMSP_PRUNE_KEEP_DIAGONAL;
    launch_lane_group(g, nb, [&](auto lanes, dim3 grid) {
        hipLaunchKernelGGL((prune_mark_kernel<S, decltype(lanes)::value>), grid, dim3(kThreads), 0, st, A->keys, A->bmps, A->offsets,
                           (const S *)A->values, nb, A->transposed, rule, tol, kd, (const R *)rowmax, kept);
    });
}

// zeroes `rowmax` (`entries` of A's row-maximum type) and fills its first num_rows entries
void compute_row_absmax(const bmsp_matrix_s *A, void *rowmax, int64_t entries, hipStream_t st)
{
    const size_t es = A->dtype == BMSP_F64 ? 8 : 4;
    if (entries == 0) return;
    BMSP_HIP(hipMemsetAsync(rowmax, 0, es * (size_t)entries, st));
    if (A->block_num == 0 || A->nnz == 0) return;
    const int g = lane_group(A->nnz, A->block_num, "BMSP_PRUNE_LANES");
    dispatch_dtype(A->dtype, [&](auto s) { launch_row_absmax<decltype(s)>(g, A, (int64_t)A->num_rows, rowmax, st); });
}

}  // namespace

void prune_check_args(int rule, double tol, int flags, int out_transposed)
{
    if (rule != BMSP_PRUNE_ABS && rule != BMSP_PRUNE_ROW_REL)
        fail(BMSP_ERR_INVALID, "rule must be BMSP_PRUNE_ABS (0) or BMSP_PRUNE_ROW_REL (1) (got %d)", rule);
    if (!(tol >= 0.0)) fail(BMSP_ERR_INVALID, "tol must be >= 0 and not NaN (got %g)", tol);
    if (rule == BMSP_PRUNE_ROW_REL && std::isinf(tol)) fail(BMSP_ERR_INVALID, "tol must be finite under BMSP_PRUNE_ROW_REL (Inf * 0 is NaN for an empty row)");
    if (flags & ~BMSP_PRUNE_KEEP_DIAGONAL) fail(BMSP_ERR_INVALID, "flags has unknown bits (got 0x%x)", (unsigned)flags);
    check_layout_flag(out_transposed, "out_transposed");
}

void row_absmax(bmsp_matrix_s *A, void *d_rowmax, hipStream_t st)
{
    check_compact_source(A, "row_absmax");
    compute_row_absmax(A, d_rowmax, A->num_rows, st);
}

// *out (when out is not null) = A without the entries the rule drops, tiles in layout out_transposed; *stats (when not null) the counts
void prune_matrix(bmsp_matrix_s *A, int rule, double tol, int flags, int out_transposed, hipStream_t st, bmsp_matrix_s **out,
                  bmsp_prune_stats *stats)
{
    prune_check_args(rule, tol, flags, out_transposed);
    if (!out && !stats) fail(BMSP_ERR_INVALID, "prune: out and stats are both null");
    check_compact_source(A, "prune");
    const uint64_t nb = (uint64_t)A->block_num;
    const int g = lane_group(A->nnz, A->block_num, "BMSP_PRUNE_LANES");
    DevBuf<uint64_t> kept(nb);  // temporaries: back to the pool after the synchronisation at the end of compact_tiles
    DevBuf<uint64_t> rowmax;    // (holds floats for F32 / F16)
    if (rule == BMSP_PRUNE_ROW_REL) {
        const int64_t padded = A->num_block_rows() * 8;  // every row a key can name
        rowmax.alloc((size_t)padded);
        compute_row_absmax(A, rowmax.p, padded, st);
    }
    if (nb) dispatch_dtype(A->dtype, [&](auto s) { launch_mark<decltype(s)>(g, A, rule, tol, flags, rowmax.p, kept.p, st); });
    compact_tiles(A, kept.p, out_transposed, "BMSP_PRUNE_LANES", st, out, stats);
}

}  // namespace bmsp

BMSP_DEFINE_WARM(prune)
