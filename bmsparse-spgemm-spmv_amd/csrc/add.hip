// add.hip -- sparse addition C = alpha*A + beta*B of two matrices already on the device (bmsp_matrix_add / bmsp_matrix_add_values),
// without going back through scalar COO entries.
//
// Keys are (block_row << 32 | block_col) in both tile layouts and every matrix holds them sorted, so C's tiles are the MERGE of two sorted
// tile lists and each C bitmap is the OR of the operands' bitmaps, both in C's layout.  Nothing is sorted.
//
// Passes:
//   rank    one lane per tile of A and of B: binary search of the tile's key among the OTHER operand's tiles of the same block-row (bounded
//           by the cached block-row pointers, so a hub block-row costs log2 probes).  A tile i: lbB = B tiles with a smaller key, hit = B
//           holds the key.  B tile j: lbA and hit likewise, and the values it adds to C (the bits of its bitmap that A's tile lacks).
//   scan    one exclusive scan over B's tiles of {unmatched, added values} packed in 64 bits; U[j] = unmatched B tiles before j.  Its total
//           is read back (C's tile count and nnz: the one synchronisation in the middle).
//   place   A tile i lands at i + U[lbB]; an unmatched B tile j at U[j] + lbA.  Writes C's keys, OR'd bitmaps and the two source maps
//           (A tile or ~0u, B tile or ~0u) that bmsp_matrix_add_values replays.
//   offsets exclusive scan of C's popcounts.
//   values  G lanes per C tile (lane_group, tile_pass.hip.h): for every stored position of C the operands' ranks come from tile_rank, at
//           the transposed position for an operand stored in the other layout.
#include "tile_pass.hip.h"

namespace bmsp {
namespace {

constexpr uint32_t kNone = ~0u;

// rank words: bits 0-31 the lower bound in the other operand, bit 32 "the other operand holds this key", bits 33-39 (B tiles only) the
// values the tile adds to C
struct RankTiles {
    const uint64_t *a_keys, *b_keys, *a_bmps, *b_bmps;
    const uint32_t *a_rowptr, *b_rowptr;
    uint64_t na;
    int a_flip, b_flip;  // the operand's layout differs from C's
    uint64_t *a_rank, *b_rank;
    __device__ void operator()(uint64_t i) const
    {
        if (i < na) {
            const uint64_t k = a_keys[i];
            const uint32_t r = key_row(k), hi = b_rowptr[r + 1];
            const uint32_t lb = lower_bound_key(b_keys, b_rowptr[r], hi, k);
            a_rank[i] = (uint64_t)lb | (uint64_t)(lb < hi && b_keys[lb] == k) << 32;
            return;
        }
        const uint64_t j = i - na;
        const uint64_t k = b_keys[j];
        const uint32_t r = key_row(k), hi = a_rowptr[r + 1];
        const uint32_t lb = lower_bound_key(a_keys, a_rowptr[r], hi, k);
        const bool hit = lb < hi && a_keys[lb] == k;
        const uint64_t bb = b_flip ? tile_transpose(b_bmps[j]) : b_bmps[j];
        uint64_t added = bb;
        if (hit) added &= ~(a_flip ? tile_transpose(a_bmps[lb]) : a_bmps[lb]);
        b_rank[j] = (uint64_t)lb | (uint64_t)hit << 32 | (uint64_t)popc64(added) << 33;
    }
};

// {unmatched (low 32 bits), values added to C (high 32 bits)} of B tile j; 0 at j == nb
struct UnmatchedIn {
    const uint64_t *b_rank;
    uint64_t nb;
    __device__ uint64_t operator()(uint64_t j) const
    {
        if (j >= nb) return 0;
        const uint64_t w = b_rank[j];
        return (uint64_t)(1u - (uint32_t)((w >> 32) & 1u)) | (w >> 33) << 32;
    }
};

struct UnmatchedOut {
    uint32_t *u;
    uint64_t nb;
    uint64_t *total;  // host scalar
    __device__ void operator()(uint64_t j, uint64_t ex) const
    {
        u[j] = (uint32_t)ex;
        if (j == nb) *total = ex;
    }
};

struct PlaceTiles {
    const uint64_t *a_keys, *b_keys, *a_bmps, *b_bmps, *a_rank, *b_rank;
    const uint32_t *u;
    uint64_t na, nc;
    int a_flip, b_flip;
    uint64_t *keys, *bmps;
    uint32_t *map;  // map[c]: A tile of C tile c, map[nc + c]: its B tile (kNone: none)
    __device__ void operator()(uint64_t i) const
    {
        if (i < na) {
            const uint64_t w = a_rank[i];
            const uint32_t lb = (uint32_t)w;
            const bool hit = (w >> 32) & 1u;
            const uint64_t c = i + u[lb];
            uint64_t b = a_flip ? tile_transpose(a_bmps[i]) : a_bmps[i];
            if (hit) b |= b_flip ? tile_transpose(b_bmps[lb]) : b_bmps[lb];
            keys[c] = a_keys[i];
            bmps[c] = b;
            map[c] = (uint32_t)i;
            map[nc + c] = hit ? lb : kNone;
            return;
        }
        const uint64_t j = i - na;
        const uint64_t w = b_rank[j];
        if ((w >> 32) & 1u) return;  // placed with its A tile
        const uint64_t c = (uint64_t)u[j] + (uint32_t)w;
        keys[c] = b_keys[j];
        bmps[c] = b_flip ? tile_transpose(b_bmps[j]) : b_bmps[j];
        map[c] = kNone;
        map[nc + c] = (uint32_t)j;
    }
};

struct CountIn {
    const uint64_t *bmps;
    uint64_t nc;
    __device__ uint64_t operator()(uint64_t c) const { return c < nc ? (uint64_t)popc64(bmps[c]) : 0; }
};

// fl(fl(alpha*a) + fl(beta*b)), never contracted into an FMA (a fused multiply-add rounds once and changes bits)
template <typename F>
__device__ __forceinline__ F scaled_sum(F alpha, F a, F beta, F b)
{
#pragma clang fp contract(off)
    const F x = alpha * a;
    const F y = beta * b;
    return x + y;
}
template <typename F>
__device__ __forceinline__ F scaled(F alpha, F a)
{
#pragma clang fp contract(off)
    return alpha * a;
}

template <typename S>
struct Operand {
    const uint64_t *bmps, *offsets;
    const S *vals;
    const uint32_t *map;  // C tile -> this operand's tile (kNone: none)
    int flip;
};

// Value pass over C tiles [0, nc): G lanes per tile.  G = 1: a lane walks all stored positions of its tile; G = 8: lane t takes row t of
// C's layout (byte t of the bitmap).  A position present in one operand only is that operand's scaled value.
template <typename S, int G>
__global__ __launch_bounds__(kThreads) void add_values_kernel(Operand<S> a, Operand<S> b, typename TileValue<S>::F alpha,
                                                              typename TileValue<S>::F beta, const uint64_t *__restrict__ c_bmps,
                                                              const uint64_t *__restrict__ c_off, S *__restrict__ c_vals, uint64_t nc)
{
    using A = TileValue<S>;  // fp16: fp32 products and sum, one RNE rounding at the end
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t j = gid / G;
    const int t = (int)(gid % G);
    if (j >= nc) return;
    const uint64_t bc = c_bmps[j];
    uint64_t m = G == 1 ? bc : bc & tile_byte_mask(t);
    if (!m) return;
    const uint32_t sa = a.map[j], sb = b.map[j];
    uint64_t ba = 0, bb = 0;  // operand bitmaps in their own layouts
    const S *va = nullptr, *vb = nullptr;
    if (sa != kNone) { ba = a.bmps[sa]; va = a.vals + a.offsets[sa]; }
    if (sb != kNone) { bb = b.bmps[sb]; vb = b.vals + b.offsets[sb]; }
    const uint64_t ba_c = a.flip ? tile_transpose(ba) : ba, bb_c = b.flip ? tile_transpose(bb) : bb;
    S *dst = c_vals + c_off[j] + (G == 1 ? 0 : tile_rank(bc, 8 * t));
    while (m) {
        const int p = tile_pop_first(m);
        const bool in_a = tile_has(ba_c, p), in_b = tile_has(bb_c, p);
        typename A::F x{}, y{};
        if (in_a) x = A::load(va[tile_rank(ba, a.flip ? tile_transposed_pos(p) : p)]);
        if (in_b) y = A::load(vb[tile_rank(bb, b.flip ? tile_transposed_pos(p) : p)]);
        *dst++ = A::store(in_a && in_b ? scaled_sum(alpha, x, beta, y) : in_a ? scaled(alpha, x) : scaled(beta, y));
    }
}

template <typename S>
void launch_values(int group, const bmsp_matrix_s *A, const bmsp_matrix_s *B, bmsp_matrix_s *C, double alpha, double beta, hipStream_t st)
{
    using F = typename TileValue<S>::F;
    const uint64_t nc = (uint64_t)C->block_num;
    const Operand<S> a{A->bmps, A->offsets, (const S *)A->values, C->add_map, A->transposed != C->transposed};
    const Operand<S> b{B->bmps, B->offsets, (const S *)B->values, C->add_map + nc, B->transposed != C->transposed};
    // alpha and beta are rounded once to the arithmetic type (fp32 for F32 and F16)
    launch_lane_group(group, nc, [&](auto lanes, dim3 grid) {
        hipLaunchKernelGGL((add_values_kernel<S, decltype(lanes)::value>), grid, dim3(kThreads), 0, st, a, b, (F)alpha, (F)beta, C->bmps,
                           C->offsets, (S *)C->values, nc);
    });
}

void compute_values(const bmsp_matrix_s *A, const bmsp_matrix_s *B, bmsp_matrix_s *C, double alpha, double beta, hipStream_t st)
{
    if (C->block_num == 0 || C->nnz == 0) return;
    const int g = lane_group(C->nnz, C->block_num, "BMSP_ADD_LANES");
    dispatch_dtype(C->dtype, [&](auto s) { launch_values<decltype(s)>(g, A, B, C, alpha, beta, st); });
}

void check_operands(const bmsp_matrix_s *A, const bmsp_matrix_s *B, const char *what)
{
    refuse_view(A, what);
    refuse_view(B, what);
    if (A->num_rows != B->num_rows || A->num_cols != B->num_cols)
        fail(BMSP_ERR_INVALID, "%s: shapes differ (%dx%d and %dx%d)", what, A->num_rows, A->num_cols, B->num_rows, B->num_cols);
    if (A->dtype != B->dtype) fail(BMSP_ERR_INVALID, "%s: dtypes differ (%d and %d)", what, (int)A->dtype, (int)B->dtype);
}

}  // namespace

// C = alpha*A + beta*B with C's tiles in layout out_transposed
bmsp_matrix_s *add_matrices(double alpha, bmsp_matrix_s *A, double beta, bmsp_matrix_s *B, int out_transposed, hipStream_t st)
{
    check_layout_flag(out_transposed, "out_transposed");
    check_operands(A, B, "add");
    const uint64_t na = (uint64_t)A->block_num, nb = (uint64_t)B->block_num;
    // C's tiles (at most na + nb) are indexed by the 32-bit source maps, with ~0u as "none"; B's added values are counted in 32 bits
    if (na + nb >= 0xffffffffull) fail(BMSP_ERR_LIMIT, "add: the operands hold %llu tiles together; C's 32-bit tile maps hold fewer than 2^32 - 1",
                                        (unsigned long long)(na + nb));
    if (B->nnz >= (1ll << 32)) fail(BMSP_ERR_LIMIT, "add: B's nnz %lld exceeds the 32-bit count of the merge", (long long)B->nnz);
    const int a_flip = A->transposed != out_transposed, b_flip = B->transposed != out_transposed;
    auto m = make_matrix();
    m->num_rows = A->num_rows; m->num_cols = A->num_cols; m->dtype = A->dtype; m->transposed = out_transposed;
    m->add_a_uid = A->uid; m->add_b_uid = B->uid;
    ensure_rowptr(A, st);
    ensure_rowptr(B, st);
    DevBuf<uint64_t> a_rank(na), b_rank(nb);  // temporaries: back to the pool after the synchronisation at the end
    DevBuf<uint32_t> u(nb + 1);
    device_for_each(RankTiles{A->keys, B->keys, A->bmps, B->bmps, A->rowptr, B->rowptr, na, a_flip, b_flip, a_rank.p, b_rank.p}, na + nb, st);
    HostScalar<uint64_t> total;
    device_exclusive_scan<uint64_t>(UnmatchedIn{b_rank.p, nb}, UnmatchedOut{u.p, nb, total.dev()}, nb + 1, st);
    const uint64_t t = total.wait(st);
    const uint64_t nc = na + (uint32_t)t;
    m->block_num = (int64_t)nc;
    m->nnz = A->nnz + (int64_t)(t >> 32);
    alloc_tile_arrays(m.get(), nc);
    alloc_values(m.get(), m->nnz);
    m->add_map.alloc(2 * (size_t)(nc ? nc : 1));
    device_for_each(PlaceTiles{A->keys, B->keys, A->bmps, B->bmps, a_rank.p, b_rank.p, u.p, na, nc, a_flip, b_flip, m->keys, m->bmps, m->add_map},
                    na + nb, st);
    device_exclusive_scan<uint64_t>(CountIn{m->bmps, nc}, PtrOut<uint64_t>{m->offsets}, nc + 1, st);
    compute_values(A, B, m.get(), alpha, beta, st);
    ensure_rowptr(m.get(), st);
    BMSP_HIP(hipStreamSynchronize(st));
    return m.release();
}

void add_values(double alpha, bmsp_matrix_s *A, double beta, bmsp_matrix_s *B, bmsp_matrix_s *C, hipStream_t st)
{
    if (!C->add_a_uid) fail(BMSP_ERR_INVALID, "add_values: C was not made by bmsp_matrix_add (or its structure changed since)");
    check_operands(A, B, "add_values");
    if (A->uid != B->uid && A->uid == C->add_b_uid && B->uid == C->add_a_uid)
        fail(BMSP_ERR_INVALID, "add_values: the operands are swapped (C was made as A + B with the other order)");
    if (A->uid != C->add_a_uid || B->uid != C->add_b_uid)
        fail(BMSP_ERR_INVALID, "add_values: the operands are not those C was made from, or their structure changed since");
    if (A->dtype != C->dtype || A->num_rows != C->num_rows || A->num_cols != C->num_cols)
        fail(BMSP_ERR_INVALID, "add_values: C's shape or dtype differs from the operands'");
    drop_value_caches(C);
    compute_values(A, B, C, alpha, beta, st);
}

}  // namespace bmsp

BMSP_DEFINE_WARM(add)
