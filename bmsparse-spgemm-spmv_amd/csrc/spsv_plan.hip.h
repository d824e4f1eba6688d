// spsv_plan.hip.h -- what the triangular solves share (spsv.hip: one right-hand side; spsm.hip: k of them; spitsv.hip: block-Jacobi
// sweeps): where the tile records of (A, op) come from and how one is read, the fused multiply-add of the substitution, the cached plan
// of (A, op, fill) -- its build and the refusal it carries -- and the walk of one block-row by eight lanes (spsv_block_row: spsv.hip
// with one vector, spitsv.hip with the previous and the next iterate).  The kernels stay in their files: they differ in what a lane
// owns (a row there, a column of X in spsm.hip) and in what orders them (levels there, nothing in a sweep).  multigrid.hip's row kernel
// takes the record read, the fused multiply-add and the chain over one tile's row from here as well.
#ifndef BMSP_SPSV_PLAN_HIP_H_
#define BMSP_SPSV_PLAN_HIP_H_

#include "tile_pass.hip.h"
#include <cstring>
#include <vector>

namespace bmsp {

// Measured (tools/spsv_bench.py; DESIGN §4 "Triangular solve"): levels of at most this many block-rows are chained in one workgroup
constexpr int64_t kChainDefault = 32;  // BMSP_SPSV_CHAIN

// where the tile records come from: the view of (A, op), or (recs == null) A's own arrays
struct SpsvTiles {
    const uint4 *recs;
    const uint64_t *keys, *bmps, *offsets;
};

// {bitmap lo, hi, value offset, the tile's other block index}
__device__ __forceinline__ uint4 spsv_rec(const SpsvTiles &T, uint64_t t)
{
    if (T.recs) return T.recs[t];
    const uint64_t b = T.bmps[t];
    return make_uint4((uint32_t)b, (uint32_t)(b >> 32), (uint32_t)T.offsets[t], key_col(T.keys[t]));
}

__device__ __forceinline__ float fused(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fused(double a, double b, double c) { return __builtin_fma(a, b, c); }

// Row i of one tile into the chain s: s = fma(+-a_ic, x_c, s) per stored entry (i, c) of the tile, c ascending (ASCENDING) or descending,
// one fused multiply-add each.  tx: the eight x of the tile's block column; tv: the tile's values.  The triangular solves subtract
// (NEG); multigrid.hip's row kernel walks whole block-rows with either sign.
template <typename S, bool MINOR, bool ASCENDING, bool NEG>
__device__ __forceinline__ typename TileValue<S>::F tile_row_chain(uint64_t bmp, const S *tv, const typename TileValue<S>::F *tx, int i,
                                                                   typename TileValue<S>::F s)
{
#pragma clang fp contract(off)
    using D = TileValue<S>;
    using F = typename D::F;
    const auto term = [](S v) -> F { return NEG ? -D::load(v) : D::load(v); };
    if (!MINOR) {
        uint32_t byte = tile_byte(bmp, i);
        if (ASCENDING) {
            int k = tile_rank(bmp, 8 * i);
            while (byte) {
                const int c = __builtin_clz(byte) - 24;
                byte &= ~(0x80u >> c);
                s = fused(term(tv[k++]), tx[c], s);
            }
        } else {
            int k = tile_rank(bmp, 8 * i) + __builtin_popcount(byte);
            while (byte) {
                const int c = 7 - __builtin_ctz(byte);
                byte &= byte - 1;
                s = fused(term(tv[--k]), tx[c], s);
            }
        }
    } else {
        uint64_t m = bmp & (0x8080808080808080ull >> i);  // positions 8j + i
        while (m) {
            int p;
            if (ASCENDING) p = tile_pop_first(m);
            else { p = 63 - __builtin_ctzll(m); m &= m - 1; }
            s = fused(term(tv[tile_rank(bmp, p)]), tx[p >> 3], s);
        }
    }
    return s;
}

// The same chain in two halves, for walks that keep several tiles in flight (multigrid.hip): tile_row_gather loads row i's stored values
// of one tile and the x they meet into registers, in column order, and returns their number; tile_row_fold takes them into the chain.
// Between the two the loads of further tiles can be issued: the chain itself is tile_row_chain's, term by term.
template <typename S, bool MINOR>
__device__ __forceinline__ int tile_row_gather(uint64_t bmp, const S *tv, const typename TileValue<S>::F *tx, int i,
                                               typename TileValue<S>::F (&a)[8], typename TileValue<S>::F (&x)[8])
{
    using D = TileValue<S>;
    int cnt = 0;
    if (!MINOR) {
        uint32_t byte = tile_byte(bmp, i);
        const int k0 = tile_rank(bmp, 8 * i);
#pragma unroll
        for (int q = 0; q < 8; q++)
            if (byte) {
                const int c = __builtin_clz(byte) - 24;
                byte &= ~(0x80u >> c);
                a[q] = D::load(tv[k0 + q]);
                x[q] = tx[c];
                cnt = q + 1;
            }
    } else {
        uint64_t m = bmp & (0x8080808080808080ull >> i);  // positions 8j + i
#pragma unroll
        for (int q = 0; q < 8; q++)
            if (m) {
                const int p = tile_pop_first(m);
                a[q] = D::load(tv[tile_rank(bmp, p)]);
                x[q] = tx[p >> 3];
                cnt = q + 1;
            }
    }
    return cnt;
}
template <typename F, bool NEG>
__device__ __forceinline__ F tile_row_fold(const F (&a)[8], const F (&x)[8], int cnt, F s)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int q = 0; q < 8; q++)
        if (q < cnt) s = fused(NEG ? -a[q] : a[q], x[q], s);
    return s;
}

// Lane i of a group of eight computes row i of output block I and returns it (stored too when the row exists).  The x of the tiles off
// the block diagonal is read from x_in, the row is written to x_out, inside the diagonal tile the group's new values go round by shuffle.
//   substitution (spsv.hip): x_in == x_out; every x the row depends on outside the block is final (an earlier launch, or an earlier
//       level of this workgroup behind a barrier).  b may be x (in place): a row's b is read by its own lane before that lane writes.
//   sweep (spitsv.hip): x_in is the previous iterate, x_out the next one, two buffers -- exact inside the block, Jacobi between blocks.
template <typename S, bool MINOR, bool LOWER, bool UNIT>
__device__ __forceinline__ typename TileValue<S>::F spsv_block_row(const SpsvTiles &T, const uint32_t *__restrict__ ptr,
                                                                   const S *__restrict__ vals, typename TileValue<S>::R alpha,
                                                                   const typename TileValue<S>::R *b, const typename TileValue<S>::R *x_in,
                                                                   typename TileValue<S>::R *x_out, int64_t n, uint32_t I, int i)
{
#pragma clang fp contract(off)
    using D = TileValue<S>;
    using F = typename D::F;
    const int64_t o = (int64_t)I * 8 + i;
    const bool row = o < n;  // (the ragged last block: its rows beyond n store nothing and are not written)
    F s = row ? alpha * b[o] : F(0);
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
        // the next record of the block-row is on its way while this tile's values and x arrive (records do not depend on x)
        const int64_t tn = t + (LOWER ? 1 : -1);
        if (tn != end) next = spsv_rec(T, (uint64_t)tn);
        const uint64_t bmp = (uint64_t)r.y << 32 | r.x;
        const S *tv = vals + r.z;
        const F *tx = x_in + (uint64_t)r.w * 8;  // only stored entries index it: never beyond the matrix
        s = tile_row_chain<S, MINOR, LOWER, true>(bmp, tv, tx, i, s);
    }
    F xi = s;  // no diagonal tile (unit diagonal): nothing inside the block
    if (diag) {
        const uint64_t bmp = (uint64_t)r.y << 32 | r.x;
        const S *tv = vals + r.z;
        F a[8], d = F(1);
        uint32_t stored = 0;  // bit c: (i, c) lies in the strict triangle and is stored
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const int p = MINOR ? 8 * c + i : 8 * i + c;
            a[c] = F(0);
            if ((LOWER ? c < i : c > i) && tile_has(bmp, p)) {
                a[c] = D::load(tv[tile_rank(bmp, p)]);
                stored |= 1u << c;
            }
        }
        if (!UNIT && tile_has(bmp, 9 * i)) d = D::load(tv[tile_rank(bmp, 9 * i)]);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int c = LOWER ? k : 7 - k;
            if (i == c) xi = UNIT ? s : s / d;
            const F xc = __shfl(xi, c, 8);  // (the whole group is here: the walk above is the same for its eight lanes)
            if ((stored >> c) & 1u) s = fused(-a[c], xc, s);
        }
    }
    if (row) x_out[o] = xi;
    return xi;
}

// other[t] = the other block index of record t
struct OtherColumn {
    SpsvTiles T;
    uint32_t *other;
    __device__ void operator()(uint64_t t) const { other[t] = spsv_rec(T, t).w; }
};

// first[I] = the first row of output block I below n whose diagonal entry is not stored, ~0u if there is none
struct MissingDiagonal {
    SpsvTiles T;
    const uint32_t *ptr;
    int64_t n;
    uint32_t *first;
    __device__ void operator()(uint64_t I) const
    {
        uint32_t lo = ptr[I], hi = ptr[I + 1];
        const uint32_t e = hi;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (spsv_rec(T, mid).w < (uint32_t)I) lo = mid + 1;
            else hi = mid;
        }
        uint64_t bmp = 0;
        if (lo < e) {
            const uint4 r = spsv_rec(T, lo);
            if (r.w == (uint32_t)I) bmp = (uint64_t)r.y << 32 | r.x;
        }
        uint32_t miss = ~0u;
        for (int k = 7; k >= 0; k--)
            if ((int64_t)I * 8 + k < n && !tile_has(bmp, 9 * k)) miss = (uint32_t)(I * 8 + k);
        first[I] = miss;
    }
};

inline int64_t chain_from_env()
{
    if (const char *e = getenv("BMSP_SPSV_CHAIN")) {
        char *end = nullptr;
        const long long c = strtoll(e, &end, 10);
        if (end != e && c >= 0) return (int64_t)c;
    }
    return kChainDefault;
}

inline SpsvTiles tiles_of(const bmsp_matrix_s *A, const bmsp_spmv_op_view *w)
{
    if (w) return SpsvTiles{(const uint4 *)w->mem, nullptr, nullptr, nullptr};
    return SpsvTiles{nullptr, A->keys, A->bmps, A->offsets};
}

// the view of (A, op), or null for (N, row-major A); *ptr = the pointer per output block
inline const bmsp_spmv_op_view *view_of(bmsp_matrix_s *A, int op, hipStream_t st, const uint32_t **ptr)
{
    if (op == BMSP_OP_N && !A->transposed) {
        ensure_rowptr(A, st);
        *ptr = A->rowptr;
        return nullptr;
    }
    const bmsp_spmv_op_view &w = spmv_op_ensure_view(A, op, st);
    *ptr = op == BMSP_OP_T ? (const uint32_t *)((const char *)w.mem + w.off_ptr) : A->rowptr;
    return &w;
}

inline bool effective_lower(int op, int fill) { return (fill == BMSP_FILL_LOWER) != (op == BMSP_OP_T); }

// builds the plan of (A, op, fill) if it is missing: synchronises `st`
inline bmsp_spsv_plan_s &ensure_plan(bmsp_matrix_s *A, int op, int fill, hipStream_t st)
{
    bmsp_spsv_plan_s &pl = A->spsv_plans[op][fill];
    if (pl.mem) return pl;
    const uint32_t *ptr = nullptr;
    const bmsp_spmv_op_view *w = view_of(A, op, st, &ptr);
    const SpsvTiles T = tiles_of(A, w);
    const int64_t blocks = A->num_block_rows();
    const uint64_t nb = (uint64_t)A->block_num;
    DevBuf<uint32_t> d_other((size_t)nb), d_miss((size_t)blocks);
    device_for_each(OtherColumn{T, d_other.p}, nb, st);
    device_for_each(MissingDiagonal{T, ptr, (int64_t)A->num_rows, d_miss.p}, (uint64_t)blocks, st);
    std::vector<uint32_t> hptr((size_t)blocks + 1, 0u), other((size_t)nb), miss((size_t)blocks);
    BMSP_HIP(hipStreamSynchronize(st));
    copy_d2h_staged(hptr.data(), ptr, 4 * ((size_t)blocks + 1));
    if (nb) copy_d2h_staged(other.data(), d_other.p, 4 * (size_t)nb);
    if (blocks) copy_d2h_staged(miss.data(), d_miss.p, 4 * (size_t)blocks);

    bmsp_spsv_plan_s np;
    np.blocks = blocks;
    np.chain = chain_from_env();
    for (int64_t I = 0; I < blocks && np.missing_diag_row < 0; I++)
        if (miss[(size_t)I] != ~0u) np.missing_diag_row = (int64_t)miss[(size_t)I];
    std::vector<uint32_t> order((size_t)blocks);
    np.level_ptr.assign((size_t)blocks + 1, 0u);
    np.segments.assign(3 * (size_t)blocks, 0u);
    int64_t n_levels = 0, n_segments = 0;
    spsv_plan(hptr.data(), other.data(), blocks, effective_lower(op, fill) ? 1 : 0, np.chain, nullptr, order.data(), np.level_ptr.data(),
              np.segments.data(), &n_levels, &n_segments);
    np.levels = n_levels;
    np.level_ptr.resize((size_t)n_levels + 1);
    np.segments.resize(3 * (size_t)n_segments);
    for (int64_t l = 0; l < n_levels; l++) {
        const int64_t wd = (int64_t)np.level_ptr[(size_t)l + 1] - (int64_t)np.level_ptr[(size_t)l];
        if (wd > np.max_level_width) np.max_level_width = wd;
    }
    for (int64_t s = 0; s < n_segments; s++)
        if (np.segments[3 * (size_t)s + 2]) {
            np.chain_launches++;
            np.chained_levels += (int64_t)np.segments[3 * (size_t)s + 1] - (int64_t)np.segments[3 * (size_t)s];
        }
    np.off_level_ptr = 4 * (size_t)blocks;
    np.bytes = np.off_level_ptr + 4 * ((size_t)n_levels + 1);
    DevBuf<char> mem(np.bytes);
    if (blocks) copy_h2d_staged(mem.p, order.data(), 4 * (size_t)blocks);
    copy_h2d_staged(mem.p + np.off_level_ptr, np.level_ptr.data(), 4 * ((size_t)n_levels + 1));
    np.mem.adopt((uint32_t *)mem.take());
    pl = std::move(np);
    return pl;
}

inline void refuse_missing_diagonal(const bmsp_spsv_plan_s &pl, int diag)
{
    if (diag == BMSP_DIAG_NON_UNIT && pl.missing_diag_row >= 0)
        fail(BMSP_ERR_INVALID, "diag: BMSP_DIAG_NON_UNIT, but row %lld of A has no stored diagonal entry", (long long)pl.missing_diag_row);
}

}  // namespace bmsp
#endif
