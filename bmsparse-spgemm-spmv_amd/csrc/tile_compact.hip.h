// tile_compact.hip.h -- the compaction of a matrix's tile list that pruning (prune.hip) and selection (select.hip) end in.  A mark pass
// of the caller leaves kept[j], the bits of tile j's bitmap (A's layout) whose entries stay; tiles keep their keys and their order in both
// layouts, so nothing is sorted and nothing is searched:
//   scan    one exclusive scan of {tile kept ? 1 : 0 (low 32 bits), kept values (high 32 bits)}: slot and value offset of every kept
//           tile at once (a transposed bitmap has the same popcount, so the offsets need no second scan).  The total is read back: the one
//           synchronisation in the middle; count-only calls end here.
//   place   G lanes per tile of A: a kept tile writes its key, kept bitmap (transposed when the layout flips) and offset at its slot and
//           compacts its kept values there; values move as raw bits.
#ifndef BMSP_TILE_COMPACT_HIP_H_
#define BMSP_TILE_COMPACT_HIP_H_

#include "tile_pass.hip.h"

namespace bmsp {
namespace {

// {tile kept (low 32 bits), kept values (high 32 bits)} of tile j; 0 at j == nb
struct KeptIn {
    const uint64_t *kept;
    uint64_t nb;
    __device__ uint64_t operator()(uint64_t j) const
    {
        if (j >= nb) return 0;
        const uint64_t b = kept[j];
        return (uint64_t)(b != 0) | (uint64_t)popc64(b) << 32;
    }
};

struct KeptOut {
    uint64_t *pos;  // nb + 1: {output slot, output value offset} of tile j; the totals at nb
    uint64_t nb;
    uint64_t *total;  // host scalar
    __device__ void operator()(uint64_t j, uint64_t ex) const
    {
        pos[j] = ex;
        if (j == nb) *total = ex;
    }
};

// A's tiles [0, nb): a kept tile goes to its slot with its kept values; index nb writes the terminal offset
template <typename T, int G>
__global__ __launch_bounds__(kThreads) void prune_place_kernel(const uint64_t *__restrict__ a_keys, const uint64_t *__restrict__ a_bmps,
                                                               const uint64_t *__restrict__ a_off, const T *__restrict__ a_vals,
                                                               const uint64_t *__restrict__ kept, const uint64_t *__restrict__ pos, uint64_t nb,
                                                               int flip, uint64_t *__restrict__ o_keys, uint64_t *__restrict__ o_bmps,
                                                               uint64_t *__restrict__ o_off, T *__restrict__ o_vals)
{
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t j = gid / G;
    const int t = (int)(gid % G);
    if (j > nb) return;
    const uint64_t w = pos[j];
    const uint64_t c = (uint32_t)w, off = w >> 32;
    if (j == nb) {
        if (t == 0) o_off[c] = off;
        return;
    }
    const uint64_t kb = kept[j];
    if (!kb) return;
    const uint64_t ib = a_bmps[j];
    const uint64_t ob = flip ? tile_transpose(kb) : kb;
    if (t == 0) {
        o_keys[c] = a_keys[j];
        o_bmps[c] = ob;
        o_off[c] = off;
    }
    uint64_t m = G == 1 ? ob : ob & tile_byte_mask(t);
    T *dst = o_vals + off + (G == 1 ? 0 : tile_rank(ob, 8 * t));
    const T *src = a_vals + a_off[j];
    while (m) {
        const int p = tile_pop_first(m);
        *dst++ = src[tile_rank(ib, flip ? tile_transposed_pos(p) : p)];
    }
}

template <typename T>
void launch_place(int g, const bmsp_matrix_s *A, const uint64_t *kept, const uint64_t *pos, bmsp_matrix_s *out, hipStream_t st)
{
    const uint64_t nb = (uint64_t)A->block_num;
    const int flip = A->transposed != out->transposed;
    launch_lane_group(g, nb + 1, [&](auto lanes, dim3 grid) {  // (index nb: the terminal offset)
        hipLaunchKernelGGL((prune_place_kernel<T, decltype(lanes)::value>), grid, dim3(kThreads), 0, st, A->keys, A->bmps, A->offsets,
                           (const T *)A->values, kept, pos, nb, flip, out->keys, out->bmps, out->offsets, (T *)out->values);
    });
}

// what a compaction refuses about its source: slots and kept values are counted in the two 32-bit halves of one scan word
void check_compact_source(const bmsp_matrix_s *A, const char *what)
{
    refuse_view(A, what);
    if (A->block_num >= 0xffffffffll) fail(BMSP_ERR_LIMIT, "%s: %lld tiles exceed the 32-bit slot count", what, (long long)A->block_num);
    if (A->nnz >= (1ll << 32)) fail(BMSP_ERR_LIMIT, "%s: nnz %lld exceeds the 32-bit value count", what, (long long)A->nnz);
}

// *out (when out is not null) = A's entries at the bits of kept[0 .. block_num), tiles in layout out_transposed; *stats (when not null)
// the counts.  `override_var`: the environment switch of the place pass's lanes per tile.  Synchronises `st` before it returns, so the
// caller's kept array may go back to the pool then.
void compact_tiles(const bmsp_matrix_s *A, const uint64_t *kept, int out_transposed, const char *override_var, hipStream_t st,
                   bmsp_matrix_s **out, bmsp_prune_stats *stats)
{
    const uint64_t nb = (uint64_t)A->block_num;
    DevBuf<uint64_t> pos(nb + 1);  // temporary: back to the pool after the synchronisation at the end
    HostScalar<uint64_t> total;
    device_exclusive_scan<uint64_t>(KeptIn{kept, nb}, KeptOut{pos.p, nb, total.dev()}, nb + 1, st);
    const uint64_t t = total.wait(st);
    const uint64_t nc = (uint32_t)t, nnz_out = t >> 32;
    if (stats) {
        stats->nnz_in = A->nnz; stats->blocks_in = A->block_num;
        stats->nnz_out = (int64_t)nnz_out; stats->blocks_out = (int64_t)nc;
    }
    if (!out) {
        BMSP_HIP(hipStreamSynchronize(st));  // the temporaries go back to the pool
        return;
    }
    auto m = make_matrix();
    m->num_rows = A->num_rows; m->num_cols = A->num_cols; m->dtype = A->dtype; m->transposed = out_transposed;
    m->block_num = (int64_t)nc;
    m->nnz = (int64_t)nnz_out;
    alloc_tile_arrays(m.get(), nc);
    alloc_values(m.get(), nnz_out);
    // the lane group of the move follows what is left of the tiles
    const int gp = lane_group(m->nnz, m->block_num, override_var);
    dispatch_width(m->dtype, [&](auto width) { launch_place<decltype(width)>(gp, A, kept, pos.p, m.get(), st); });
    ensure_rowptr(m.get(), st);
    BMSP_HIP(hipStreamSynchronize(st));
    *out = m.release();
}

}  // namespace
}  // namespace bmsp
#endif
