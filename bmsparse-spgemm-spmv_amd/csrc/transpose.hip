// transpose.hip -- transpose and tile-layout conversion of a matrix already on the device (bmsp_matrix_transpose /
// bmsp_matrix_convert_layout / bmsp_matrix_copy_values), without going back through scalar COO entries.
//
// What the format gives (builder.hip, MakeSortKey): A stored in layout L and A^T stored in the OTHER layout have the same bitmap and the
// same value segment for every tile -- bit (63 - pos) with pos = 8*r + c (L = 0) names the same entry as pos = 8*c' + r' of the swapped
// tile (L = 1).  Only the keys swap, (brow, bcol) -> (bcol, brow), and the tiles re-order by the new key.  The other two operations (A^T in
// the SAME layout, A in the other layout) transpose every bitmap (tile_transpose) and permute the values inside each tile: output value k
// of a tile is the source value whose rank is the popcount of the source bitmap in front of the transposed position.
//
// Passes:  sort keys (swapped key, tile index) -> stable LSD radix sort on the block-column bits only (the input is sorted by (brow, bcol),
// so sorting (bcol, brow) keys on bcol alone gives (bcol, brow) order; the sorted keys ARE the output keys, the payload is the tile map)
// -> one exclusive scan of the output popcounts that also writes bitmaps (and keys for a conversion) -> the value move.  A conversion
// needs no sort: the tile order and keys stay.  Values are moved as raw bits (unsigned integers of the element width).
#include "tile_pass.hip.h"

namespace bmsp {
namespace {

struct SwappedKey {
    const uint64_t *keys;
    uint64_t *sk;
    uint32_t *idx;
    __device__ void operator()(uint64_t i) const
    {
        const uint64_t k = keys[i];
        sk[i] = key_make(key_col(k), key_row(k));
        idx[i] = (uint32_t)i;
    }
};

// popcount of output tile i (a transposed bitmap has the same popcount), 0 at i == nb (the terminal offset)
struct OutCount {
    const uint32_t *map;  // null: tile i comes from source tile i
    const uint64_t *a_bmps;
    uint64_t nb;
    __device__ uint64_t operator()(uint64_t i) const { return i < nb ? (uint64_t)popc64(a_bmps[map ? map[i] : (uint32_t)i]) : 0; }
};

struct OutTiles {
    const uint32_t *map;
    const uint64_t *a_bmps;
    uint64_t nb;
    int permute;
    uint64_t *bmps, *offsets;
    __device__ void operator()(uint64_t i, uint64_t ex) const
    {
        offsets[i] = ex;
        if (i == nb) return;
        const uint64_t b = a_bmps[map ? map[i] : (uint32_t)i];
        bmps[i] = permute ? tile_transpose(b) : b;
    }
};

// Value move for output tiles [0, nb): G lanes per tile (lane_group, tile_pass.hip.h).  PERMUTE = false: the tile's segment is copied as
// is (layout-flipping transpose).  PERMUTE = true: the output tile is the transpose of the source tile; output position p = 8i + j holds
// the source entry at q = 8j + i.
template <typename T, int G, bool PERMUTE>
__global__ __launch_bounds__(kThreads) void move_values_kernel(const uint32_t *__restrict__ map, const uint64_t *__restrict__ a_bmps,
                                                               const uint64_t *__restrict__ a_off, const T *__restrict__ a_vals,
                                                               const uint64_t *__restrict__ o_off, T *__restrict__ o_vals, uint64_t nb)
{
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t j = gid / G;
    const int t = (int)(gid % G);
    if (j >= nb) return;
    const uint32_t s = map ? map[j] : (uint32_t)j;
    const T *src = a_vals + a_off[s];
    T *dst = o_vals + o_off[j];
    if (!PERMUTE) {
        const int n = (int)(o_off[j + 1] - o_off[j]);
        for (int k = t; k < n; k += G) dst[k] = src[k];
        return;
    }
    const uint64_t ib = a_bmps[s];
    const uint64_t ob = tile_transpose(ib);
    if (G == 8) {  // lane = output row
        uint32_t row = tile_byte(ob, t);
        int k = tile_rank(ob, 8 * t);
        while (row) {
            const int c = __builtin_clz(row) - 24;  // first stored column of the row
            row &= ~(0x80u >> c);
            dst[k++] = src[tile_rank(ib, 8 * c + t)];  // output (row t, column c) = source (row c, column t)
        }
    } else {  // one lane walks the stored positions in order
        uint64_t m = ob;
        int k = 0;
        while (m) {
            const int p = tile_pop_first(m);
            dst[k++] = src[tile_rank(ib, tile_transposed_pos(p))];
        }
    }
}

template <typename T, bool PERMUTE>
void launch_move(int g, const bmsp_matrix_s *A, bmsp_matrix_s *out, hipStream_t st)
{
    const uint64_t nb = (uint64_t)out->block_num;
    launch_lane_group(g, nb, [&](auto lanes, dim3 grid) {
        hipLaunchKernelGGL((move_values_kernel<T, decltype(lanes)::value, PERMUTE>), grid, dim3(kThreads), 0, st, out->tp_map, A->bmps,
                           A->offsets, (const T *)A->values, out->offsets, (T *)out->values, nb);
    });
}

}  // namespace

// moves the values of `out` from those of A through out's tile map (tp_map; null = same tile order) and permutation flag
void move_values(const bmsp_matrix_s *A, bmsp_matrix_s *out, hipStream_t st)
{
    if (out->block_num == 0 || out->nnz == 0) return;
    const int g = lane_group(out->nnz, out->block_num, "BMSP_TRANSPOSE_LANES");
    dispatch_width(out->dtype, [&](auto width) {
        using T = decltype(width);
        if (out->tp_permute) launch_move<T, true>(g, A, out, st);
        else launch_move<T, false>(g, A, out, st);
    });
}

namespace {

void check_source(const bmsp_matrix_s *A, int out_transposed, const char *what)
{
    check_layout_flag(out_transposed, "out_transposed");
    refuse_view(A, what);
    if (A->nnz >= (1ll << 32)) fail(BMSP_ERR_LIMIT, "nnz %lld exceeds the 32-bit element range", (long long)A->nnz);
    if (A->block_num >= (1ll << 32)) fail(BMSP_ERR_LIMIT, "more than 2^32 blocks");
}

}  // namespace

// Every tile of A as (swapped key (bcol, brow), tile index), stably sorted on the block-column bits only: the input is sorted by
// (brow, bcol), so equal block columns keep their block-row order and the result is in (bcol, brow) order.
void sort_tiles_by_block_column(const bmsp_matrix_s *A, TileSort &ts, hipStream_t st)
{
    const uint64_t nb = (uint64_t)A->block_num;
    ts.k0.alloc(nb); ts.k1.alloc(nb); ts.p0.alloc(nb); ts.p1.alloc(nb);
    device_for_each(SwappedKey{A->keys, ts.k0.p, ts.p0.p}, nb, st);
    PingPong<uint64_t> kk{ts.k0.p, ts.k1.p};
    PingPong<uint32_t> pp{ts.p0.p, ts.p1.p};
    const int cbits = ceil_log2_u64((uint64_t)A->num_block_cols());
    device_radix_sort_pairs<uint32_t>(kk, pp, nb, 32, 32 + cbits, st);
    ts.keys = kk.cur; ts.map = pp.cur;
}

// The tail that a transpose and a block permutation (reorder.hip) share.  m holds its dimensions, counts, dtype, layout and tp_*
// fields and, when its tiles were re-ordered, its keys and tile map (m->keys null: A's tile order and keys).  Makes the other arrays,
// writes bitmaps and offsets in one scan, moves the values and synchronises `st` (the sort temporaries go back to the pool).
void finish_moved_tiles(bmsp_matrix_s *A, bmsp_matrix_s *m, hipStream_t st)
{
    const uint64_t nb = (uint64_t)A->block_num;
    const bool keeps_keys = m->keys == nullptr;
    alloc_tile_arrays(m, nb);  // (re-ordered tiles hold their keys already)
    alloc_values(m, (uint64_t)m->nnz);
    if (keeps_keys && nb) BMSP_HIP(hipMemcpyAsync(m->keys, A->keys, 8 * nb, hipMemcpyDeviceToDevice, st));
    device_exclusive_scan<uint64_t>(OutCount{m->tp_map, A->bmps, nb}, OutTiles{m->tp_map, A->bmps, nb, m->tp_permute, m->bmps, m->offsets},
                                    nb + 1, st);
    move_values(A, m, st);
    ensure_rowptr(m, st);
    BMSP_HIP(hipStreamSynchronize(st));
}

// out = A^T (swap = true) or A (swap = false) with its tiles in layout out_transposed
bmsp_matrix_s *transpose_matrix(bmsp_matrix_s *A, int out_transposed, bool swap, hipStream_t st)
{
    check_source(A, out_transposed, swap ? "transpose" : "convert_layout");
    auto m = make_matrix();
    m->num_rows = swap ? A->num_cols : A->num_rows;
    m->num_cols = swap ? A->num_rows : A->num_cols;
    m->nnz = A->nnz; m->block_num = A->block_num; m->dtype = A->dtype; m->transposed = out_transposed;
    m->tp_src_uid = A->uid;
    // a transpose into the other layout, or a conversion into the same one, keeps every tile as it is
    m->tp_permute = (out_transposed != A->transposed) != swap ? 1 : 0;
    TileSort ts;  // sort temporaries: go back to the pool after the synchronisation at the end
    if (swap) {
        sort_tiles_by_block_column(A, ts, st);
        m->keys = ts.take_keys();
        m->tp_map = ts.take_map();
    }
    finish_moved_tiles(A, m.get(), st);
    return m.release();
}

void copy_values_from(bmsp_matrix_s *A, bmsp_matrix_s *out, hipStream_t st)
{
    if (!out->tp_src_uid || out->tp_src_uid != A->uid)
        fail(BMSP_ERR_INVALID, "copy_values: the target was not made from this matrix by a transpose or a layout conversion, or the source's "
                               "structure changed since");
    if (A->block_num != out->block_num || A->nnz != out->nnz || A->dtype != out->dtype)
        fail(BMSP_ERR_INVALID, "copy_values: source and target sizes or dtypes differ");
    drop_value_caches(out);
    move_values(A, out, st);
}

}  // namespace bmsp

BMSP_DEFINE_WARM(transpose)
