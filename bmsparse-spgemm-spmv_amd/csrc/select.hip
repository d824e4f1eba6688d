// select.hip -- keeps the stored entries of a matrix already on the device by POSITION (bmsp_matrix_select_band / bmsp_matrix_select_mask),
// without going back through scalar COO entries: a band lo <= col - row <= hi (tril, triu, the diagonal part, the off-diagonal part) or
// the pattern of another matrix M of the same shape, either one complemented on request.
//
// Tiles keep their order and their keys in both layouts, so the output is a COMPACTION of A's tile list, as for pruning: nothing is
// sorted, nothing is re-tiled.  No pass reads a value of A before the move, and M's values are never read.
//
// Passes:
//   mark    one lane per tile of A: the kept bitmap in A's layout, pure integer work.
//           band: with delta = block_col - block_row the tile holds the matrix diagonals 8 delta - 7 .. 8 delta + 7; it goes, stays
//                 whole, or keeps bmp & tile_band_mask(lo - 8 delta, hi - 8 delta) (bmsp_bits.h; a column-major tile takes the mirrored
//                 band).  16 bytes read per tile.
//           mask: binary search of the tile's key among M's tiles of the same block-row (bounded by M's block-row pointer, so a hub
//                 block-row costs log2 probes, as in add.hip); m = M's bitmap there, through tile_transpose when the layouts differ, 0 when
//                 M has no such tile; kept = bmp & m.
//           BMSP_SELECT_COMPLEMENT keeps bmp & ~(what the predicate keeps).
//   scan, place   the compaction pruning shares (tile_compact.hip.h).
#include "tile_compact.hip.h"

namespace bmsp {
namespace {

// the band bounds are clamped to +-2^36 before anything is subtracted from them: coordinates are below 2^35, so no diagonal of a matrix
// lies outside, and lo - 8 delta (|8 delta| < 2^35) cannot overflow
constexpr int64_t kBandClamp = 1ll << 36;
inline int64_t clamp_band(int64_t v) { return v < -kBandClamp ? -kBandClamp : v > kBandClamp ? kBandClamp : v; }

// kept[j]: the bits of tile j's bitmap (A's layout) whose entries lie in the band (complement: outside it)
__global__ __launch_bounds__(kThreads) void select_band_mark_kernel(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ bmps,
                                                                    uint64_t nb, int transposed, int64_t lo, int64_t hi, int complement,
                                                                    uint64_t *__restrict__ kept)
{
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= nb) return;
    const uint64_t key = keys[j], bmp = bmps[j];
    const int64_t delta = (int64_t)key_col(key) - (int64_t)key_row(key);
    const uint64_t in = tile_band_select(bmp, delta, lo, hi, transposed);
    kept[j] = complement ? bmp & ~in : in;
}

// kept[j]: the bits of A tile j's bitmap (A's layout) whose coordinates M stores (complement: does not store)
__global__ __launch_bounds__(kThreads) void select_mask_mark_kernel(const uint64_t *__restrict__ a_keys, const uint64_t *__restrict__ a_bmps,
                                                                    uint64_t nb, const uint64_t *__restrict__ m_keys,
                                                                    const uint64_t *__restrict__ m_bmps, const uint32_t *__restrict__ m_rowptr,
                                                                    int flip, int complement, uint64_t *__restrict__ kept)
{
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= nb) return;
    const uint64_t key = a_keys[j], bmp = a_bmps[j];
    const uint32_t r = key_row(key), end = m_rowptr[r + 1];
    const uint32_t lb = lower_bound_key(m_keys, m_rowptr[r], end, key);
    uint64_t m = 0;
    if (lb < end && m_keys[lb] == key) m = flip ? tile_transpose(m_bmps[lb]) : m_bmps[lb];
    kept[j] = complement ? bmp & ~m : bmp & m;
}

}  // namespace

void select_check_args(int flags, int out_transposed, const void *out, const void *stats)
{
    if (flags & ~BMSP_SELECT_COMPLEMENT) fail(BMSP_ERR_INVALID, "flags has unknown bits (got 0x%x)", (unsigned)flags);
    check_layout_flag(out_transposed, "out_transposed");
    if (!out && !stats) fail(BMSP_ERR_INVALID, "out and stats are both null");
}

// *out (when out is not null) = A's entries with lo <= col - row <= hi (or the others), tiles in layout out_transposed; *stats the counts
void select_band(bmsp_matrix_s *A, int64_t lo, int64_t hi, int flags, int out_transposed, hipStream_t st, bmsp_matrix_s **out,
                 bmsp_select_stats *stats)
{
    select_check_args(flags, out_transposed, out, stats);
    check_compact_source(A, "select_band");
    lo = clamp_band(lo);
    hi = clamp_band(hi);
    const uint64_t nb = (uint64_t)A->block_num;
    DevBuf<uint64_t> kept(nb);  // temporary: back to the pool after the synchronisation at the end of compact_tiles
    if (nb) {
        hipLaunchKernelGGL(select_band_mark_kernel, grid_for(nb), dim3(kThreads), 0, st, A->keys, A->bmps, nb, A->transposed, lo, hi,
                           flags & BMSP_SELECT_COMPLEMENT, kept.p);
        BMSP_CHECK_LAUNCH();
    }
    compact_tiles(A, kept.p, out_transposed, "BMSP_SELECT_LANES", st, out, stats);
}

// *out (when out is not null) = A's entries at the coordinates M stores (or the others), tiles in layout out_transposed; *stats the counts
void select_mask(bmsp_matrix_s *A, bmsp_matrix_s *M, int flags, int out_transposed, hipStream_t st, bmsp_matrix_s **out,
                 bmsp_select_stats *stats)
{
    select_check_args(flags, out_transposed, out, stats);
    check_compact_source(A, "select_mask");
    refuse_view(M, "select_mask");
    if (A->num_rows != M->num_rows || A->num_cols != M->num_cols)
        fail(BMSP_ERR_INVALID, "select_mask: the shapes of A and M differ (%dx%d and %dx%d)", A->num_rows, A->num_cols, M->num_rows, M->num_cols);
    const uint64_t nb = (uint64_t)A->block_num;
    DevBuf<uint64_t> kept(nb);  // temporary: back to the pool after the synchronisation at the end of compact_tiles
    if (nb) {
        ensure_rowptr(M, st);
        hipLaunchKernelGGL(select_mask_mark_kernel, grid_for(nb), dim3(kThreads), 0, st, A->keys, A->bmps, nb, M->keys, M->bmps, M->rowptr.p,
                           (int)(A->transposed != M->transposed), flags & BMSP_SELECT_COMPLEMENT, kept.p);
        BMSP_CHECK_LAUNCH();
    }
    compact_tiles(A, kept.p, out_transposed, "BMSP_SELECT_LANES", st, out, stats);
}

}  // namespace bmsp

BMSP_DEFINE_WARM(select)
