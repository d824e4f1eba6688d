// sddmm.hip -- the sampled dense-dense product on the pattern of a matrix already on the device (bmsp_sddmm / bmsp_sddmm_values): for every
// stored coordinate (i, j) of S, d_ij = row i of X . row j of Y (both row-major, k long), then c = alpha * d + beta * s or alpha * d * s.
//
// Nothing changes or searches a structure: the output has S's keys, offsets and (possibly transposed) bitmaps, as a scaled matrix has.
// Every output value has exactly one writer: no sum across waves, no atomic, no LDS, no hand-off.
//
// Kernels:
//   sddmm_value_kernel<S, G>  vector ALU, all three dtypes.  G lanes per tile (lane_group, tile_pass.hip.h): G = 1 walks the stored
//                  positions of the output bitmap, G = 8 gives lane t byte t of it.  A lane forms each of its dot products alone, with
//                  16-byte loads of both rows where bases and leading dimensions allow and element loads otherwise; both forms add
//                  element t into partial sum t mod NV (NV elements per 16 bytes) and add the partial sums in index order, so they give
//                  the same bits.
//   sddmm_tile_kernel<S>      matrix cores, F16 (v_mfma_f32_16x16x32_f16) and F32 (v_mfma_f32_16x16x4_f32).  One MFMA serves two tiles
//                  p, q: A = 8 X rows of p's block-row over 8 of q's, B = 8 Y rows of p's block-column beside 8 of q's; D[0:8][0:8] is
//                  tile p, D[8:16][8:16] tile q, the off-diagonal blocks are dropped.  Lane l loads 16 bytes of operand row l & 15 at
//                  k-offset NV * (l >> 4) of each step of 4 * NV k-values -- the operand map of both instructions (F32: element j of
//                  the load feeds the j-th of four MFMAs; A and B use the same assignment, which is all a dot product needs).  A wave
//                  takes kRun consecutive tiles and keeps their accumulators in registers over one pass through k; per k step it
//                  issues all of its operand loads, none under a branch, then the MFMAs.  The k tail is loaded by elements and masked
//                  to zero; rows past the matrix edge and the missing partner of an odd last tile are zero fragments (row 0 is read
//                  in their place, never a row that does not exist).
// Epilogue (both): each operation rounded on its own, never contracted; with beta == 0 the stored s is not read.
#include "tile_pass.hip.h"
#include <cstring>

namespace bmsp {
namespace {

constexpr int kRun = 8;            // tiles per wave of the tile kernel
constexpr int kPairs = kRun / 2;   // MFMA accumulators per wave
constexpr int kFillThreshold = 6;  // mean values per tile from which the tile kernel is the default (measured: DESIGN section 4 "SDDMM")

typedef _Float16 half8_d __attribute__((ext_vector_type(8)));
typedef float float4_d __attribute__((ext_vector_type(4)));
typedef double double2_d __attribute__((ext_vector_type(2)));

// the element type of X and Y as loaded, NV of them per 16 bytes
template <typename S>
struct Operand;
template <>
struct Operand<uint16_t> {
    using E = _Float16;
    using V = half8_d;
    static constexpr int NV = 8;
};
template <>
struct Operand<float> {
    using E = float;
    using V = float4_d;
    static constexpr int NV = 4;
};
template <>
struct Operand<double> {
    using E = double;
    using V = double2_d;
    static constexpr int NV = 2;
};

__device__ __forceinline__ float fma_f(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_f(double a, double b, double c) { return __builtin_fma(a, b, c); }

// x . y over k elements: element t goes into partial sum t mod NV, the partial sums are added in index order (vec: 16-byte loads)
template <typename S>
__device__ __forceinline__ typename TileValue<S>::F dot_rows(const typename Operand<S>::E *__restrict__ x,
                                                             const typename Operand<S>::E *__restrict__ y, int k, bool vec)
{
    using F = typename TileValue<S>::F;
    using V = typename Operand<S>::V;
    constexpr int NV = Operand<S>::NV;
    F acc[NV];
#pragma unroll
    for (int j = 0; j < NV; j++) acc[j] = 0;
    int t = 0;
    if (vec) {
        for (; t + NV <= k; t += NV) {
            const V xv = *(const V *)(x + t), yv = *(const V *)(y + t);
#pragma unroll
            for (int j = 0; j < NV; j++) acc[j] = fma_f((F)xv[j], (F)yv[j], acc[j]);
        }
    } else {
        for (; t + NV <= k; t += NV) {
#pragma unroll
            for (int j = 0; j < NV; j++) acc[j] = fma_f((F)x[t + j], (F)y[t + j], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < NV - 1; j++)  // (the tail: fewer than NV elements)
        if (t + j < k) acc[j] = fma_f((F)x[t + j], (F)y[t + j], acc[j]);
    F sum = acc[0];
#pragma unroll
    for (int j = 1; j < NV; j++) sum += acc[j];
    return sum;
}

// Value pass over tiles [0, nb): the value at position p of output tile j = epilogue(X row . Y row, s read through S's bitmap -- the
// transposed position when the layout flips).  s_vals and o_vals may be the same array (in place: flip == 0, a value is read and
// written by one lane).
template <typename S, int G>
__global__ __launch_bounds__(kThreads) void sddmm_value_kernel(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ s_bmps,
                                                               const uint64_t *__restrict__ offsets, const S *s_vals, S *o_vals, uint64_t nb,
                                                               int flip, int olay, const void *__restrict__ Xv, int64_t ldx,
                                                               const void *__restrict__ Yv, int64_t ldy, int k, int vec,
                                                               typename TileValue<S>::F alpha, typename TileValue<S>::F beta, int mode)
{
    using D = TileValue<S>;
    using F = typename D::F;
    using E = typename Operand<S>::E;
    const E *X = (const E *)Xv, *Y = (const E *)Yv;
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t j = gid / G;
    const int t = (int)(gid % G);
    if (j >= nb) return;
    const uint64_t key = keys[j], ib = s_bmps[j], off = offsets[j];
    const int64_t row0 = (int64_t)key_row(key) * 8, col0 = (int64_t)key_col(key) * 8;
    const uint64_t ob = flip ? tile_transpose(ib) : ib;
    const S *src = s_vals + off;
    // G = 8: lane t takes byte t of the output bitmap (a row of a row-major tile, a column of a column-major one); G = 1: all of it
    uint64_t m = G == 8 ? ob & tile_byte_mask(t) : ob;
    S *dst = o_vals + off + (G == 8 ? tile_rank(ob, 8 * t) : 0);
    while (m) {
        const int p = tile_pop_first(m);
        const int row = olay ? (p & 7) : (p >> 3), col = olay ? (p >> 3) : (p & 7);
        const F d = dot_rows<S>(X + (row0 + row) * ldx, Y + (col0 + col) * ldy, k, vec != 0);
        F s = 0;
        if (mode != kModeAlpha) s = D::load(src[tile_rank(ib, flip ? tile_transposed_pos(p) : p)]);
        *dst++ = D::store(epilogue<F>(d, alpha, beta, s, mode));
    }
}

// ---- tile kernel ----------------------------------------------------------------------------------------------------------------------
// This lane's 16 bytes of an operand row at k-offset t0, without a branch (a load under a branch waits for its data before the next
// one is issued; a wave has sixteen of these per k step and wants them all in flight): a row that does not exist is read as row 0 --
// `off` is 0 then, and row 0 exists in a matrix that has a tile -- and replaced by zeros; in the k tail (FULL = false) the elements
// are loaded one by one at indices clamped to k - 1 and those at or past k replaced by zeros.
template <typename S, bool FULL>
__device__ __forceinline__ typename Operand<S>::V load_fragment(const typename Operand<S>::E *__restrict__ base, int64_t off, bool ok, int t0, int k)
{
    using V = typename Operand<S>::V;
    using E = typename Operand<S>::E;
    constexpr int NV = Operand<S>::NV;
    V f;
    if (FULL) {
        f = *(const V *)(base + off + t0);
#pragma unroll
        for (int j = 0; j < NV; j++) f[j] = ok ? f[j] : (E)0;
    } else {
#pragma unroll
        for (int j = 0; j < NV; j++) {
            const int t = t0 + j;
            const E e = base[off + (t < k ? t : k - 1)];
            f[j] = ok && t < k ? e : (E)0;
        }
    }
    return f;
}

__device__ __forceinline__ float4_d mma_step(half8_d a, half8_d b, float4_d c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float4_d mma_step(float4_d a, float4_d b, float4_d c)
{
#pragma unroll
    for (int j = 0; j < 4; j++) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], c, 0, 0, 0);
    return c;
}

// one step of 4 * NV k-values for all pairs: every load first, then the MFMAs
template <typename S, bool FULL>
__device__ __forceinline__ void tile_step(float4_d (&acc)[kPairs], const typename Operand<S>::E *__restrict__ X,
                                          const typename Operand<S>::E *__restrict__ Y, const int64_t (&xoff)[kPairs],
                                          const int64_t (&yoff)[kPairs], uint32_t okx, uint32_t oky, int t0, int k)
{
    using V = typename Operand<S>::V;
    V fa[kPairs], fb[kPairs];
#pragma unroll
    for (int i = 0; i < kPairs; i++) {
        fa[i] = load_fragment<S, FULL>(X, xoff[i], (okx >> i) & 1u, t0, k);
        fb[i] = load_fragment<S, FULL>(Y, yoff[i], (oky >> i) & 1u, t0, k);
    }
#pragma unroll
    for (int i = 0; i < kPairs; i++) acc[i] = mma_step(fa[i], fb[i], acc[i]);
}

// Wave w takes tiles [kRun * w, kRun * w + kRun) as kPairs pairs (p, q = p + 1).  Operand lane l serves row (l & 7) of tile p (l & 8 == 0)
// or q; result lane l holds rows 4 * ((l >> 4) & 1) .. + 3 of column l & 7 of tile p (l < 32 and (l & 15) < 8) or q (l >= 32 and
// (l & 15) >= 8); the other result lanes hold the off-diagonal blocks and store nothing.  A tile past the end (the odd last tile's
// partner, the pairs a short last wave lacks) has zero fragments and stores nothing.
template <typename S>
__global__ __launch_bounds__(kThreads) void sddmm_tile_kernel(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ s_bmps,
                                                              const uint64_t *__restrict__ offsets, const S *s_vals, S *o_vals, uint64_t nb,
                                                              int flip, int olay, const void *__restrict__ Xv, int64_t ldx,
                                                              const void *__restrict__ Yv, int64_t ldy, int k, int64_t num_rows,
                                                              int64_t num_cols, float alpha, float beta, int mode)
{
    using D = TileValue<S>;
    using E = typename Operand<S>::E;
    constexpr int NV = Operand<S>::NV, STEP = 4 * NV;
    const int lane = lane_id(), g = lane >> 4;
    const uint64_t wave = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
    const uint64_t tile0 = wave * kRun;
    if (tile0 >= nb) return;  // (the whole wave)

    const E *X = (const E *)Xv, *Y = (const E *)Yv;
    int64_t xoff[kPairs], yoff[kPairs];  // (offsets, not pointers: the loads stay global loads)
    uint32_t okx = 0, oky = 0;
#pragma unroll
    for (int i = 0; i < kPairs; i++) {
        const uint64_t ti = tile0 + 2 * i + ((lane >> 3) & 1);
        const bool there = ti < nb;
        const uint64_t key = keys[there ? ti : tile0];
        const int64_t r = (int64_t)key_row(key) * 8 + (lane & 7), c = (int64_t)key_col(key) * 8 + (lane & 7);
        const bool rx = there && r < num_rows, cy = there && c < num_cols;
        okx |= (rx ? 1u : 0u) << i;
        oky |= (cy ? 1u : 0u) << i;
        xoff[i] = rx ? r * ldx : 0;
        yoff[i] = cy ? c * ldy : 0;
    }

    float4_d acc[kPairs];
#pragma unroll
    for (int i = 0; i < kPairs; i++) acc[i] = float4_d{0.f, 0.f, 0.f, 0.f};
    int kk = 0;
    for (; kk + STEP <= k; kk += STEP) tile_step<S, true>(acc, X, Y, xoff, yoff, okx, oky, kk + NV * g, k);
    if (kk < k) tile_step<S, false>(acc, X, Y, xoff, yoff, okx, oky, kk + NV * g, k);  // (wave-uniform)

    // result lanes: the diagonal blocks of D.  Every load of s before the first store (in place they are the same array; a lane reads
    // only what it writes), and no load under a branch: a position that is not stored reads value 0 of the array and stores nothing.
    const bool second = g >= 2;
    if (second != ((lane & 15) >= 8)) return;
    const int c = lane & 7, r0 = 4 * (g & 1);
    uint32_t dst[kPairs][4], src[kPairs][4];  // value indices of the store (~0: none) and of s (fewer than 2^32 values: checked by the host)
    uint64_t ibs[kPairs];
    uint32_t offs[kPairs];
#pragma unroll
    for (int i = 0; i < kPairs; i++) {  // (the structure words of every pair in flight before the first is used)
        const uint64_t tr = tile0 + 2 * i + (second ? 1 : 0);
        ibs[i] = s_bmps[tr < nb ? tr : tile0];
        offs[i] = (uint32_t)offsets[tr < nb ? tr : tile0];
    }
#pragma unroll
    for (int i = 0; i < kPairs; i++) {
        const bool there = tile0 + 2 * i + (second ? 1 : 0) < nb;
        const uint64_t ib = ibs[i];
        const uint32_t off = offs[i];
        const uint64_t ob = flip ? tile_transpose(ib) : ib;
#pragma unroll
        for (int jr = 0; jr < 4; jr++) {
            const int r = r0 + jr;
            const int p = olay ? 8 * c + r : 8 * r + c;
            const bool has = there && tile_has(ob, p);
            dst[i][jr] = has ? off + (uint32_t)tile_rank(ob, p) : ~0u;
            src[i][jr] = has ? off + (uint32_t)tile_rank(ib, flip ? tile_transposed_pos(p) : p) : 0u;
        }
    }
    float sv[kPairs][4];
#pragma unroll
    for (int i = 0; i < kPairs; i++) {
#pragma unroll
        for (int jr = 0; jr < 4; jr++) sv[i][jr] = 0.f;
    }
    if (mode != kModeAlpha) {  // (wave-uniform; one block of loads)
#pragma unroll
        for (int i = 0; i < kPairs; i++) {
#pragma unroll
            for (int jr = 0; jr < 4; jr++) sv[i][jr] = D::load(s_vals[src[i][jr]]);
        }
    }
#pragma unroll
    for (int i = 0; i < kPairs; i++) {
#pragma unroll
        for (int jr = 0; jr < 4; jr++)
            if (dst[i][jr] != ~0u) o_vals[dst[i][jr]] = D::store(epilogue<float>(acc[i][jr], alpha, beta, sv[i][jr], mode));
    }
}

// ---- selection ------------------------------------------------------------------------------------------------------------------------
struct Choice {
    bool tile;  // sddmm_tile_kernel, else sddmm_value_kernel
    int lanes;  // lanes per tile of the value kernel (0 for the tile kernel)
    bool vec;   // 16-byte loads (value kernel; the tile kernel requires them)
};

bool aligned16(const void *p, int64_t ld, size_t es) { return ((uintptr_t)p % 16) == 0 && ((uint64_t)ld * es) % 16 == 0; }

// The one place the kernel is decided: the launcher and bmsp_sddmm_launch_info both call it.  The tile kernel needs F16 / F32 and 16-byte
// aligned operands; by default it runs from a mean fill of kFillThreshold values per tile.  BMSP_SDDMM_KERNEL=value|tile forces a side
// where the case can take it (read per call).
Choice choose_kernel(const bmsp_matrix_s *S, const void *X, int64_t ldx, const void *Y, int64_t ldy)
{
    const size_t es = dtype_size(S->dtype);
    const bool vec = aligned16(X, ldx, es) && aligned16(Y, ldy, es);
    const bool can_tile = vec && S->dtype != BMSP_F64;
    bool tile = can_tile && S->nnz >= (int64_t)kFillThreshold * S->block_num;
    if (const char *e = getenv("BMSP_SDDMM_KERNEL")) {
        if (!strcmp(e, "value")) tile = false;
        else if (!strcmp(e, "tile")) tile = can_tile;
    }
    return Choice{tile, tile ? 0 : lane_group(S->nnz, S->block_num, "BMSP_SDDMM_LANES"), vec};
}

template <typename S>
void launch_value(const Choice &ch, const bmsp_matrix_s *Sm, bmsp_matrix_s *out, const void *X, int64_t ldx, const void *Y, int64_t ldy, int k,
                  double alpha, double beta, int mode, hipStream_t st)
{
    using F = typename TileValue<S>::F;
    const uint64_t nb = (uint64_t)out->block_num;
    const int flip = Sm->transposed != out->transposed;
    launch_lane_group(ch.lanes, nb, [&](auto lanes, dim3 grid) {
        hipLaunchKernelGGL((sddmm_value_kernel<S, decltype(lanes)::value>), grid, dim3(kThreads), 0, st, Sm->keys, Sm->bmps, Sm->offsets,
                           (const S *)Sm->values, (S *)out->values, nb, flip, out->transposed, X, ldx, Y, ldy, k, ch.vec ? 1 : 0, (F)alpha,
                           (F)beta, mode);
    });
}

template <typename S>
void launch_tile(const bmsp_matrix_s *Sm, bmsp_matrix_s *out, const void *X, int64_t ldx, const void *Y, int64_t ldy, int k, double alpha,
                 double beta, int mode, hipStream_t st)
{
    const uint64_t nb = (uint64_t)out->block_num;
    const int flip = Sm->transposed != out->transposed;
    const uint64_t waves = (nb + kRun - 1) / kRun;
    hipLaunchKernelGGL((sddmm_tile_kernel<S>), grid_for(waves * kWave), dim3(kThreads), 0, st, Sm->keys, Sm->bmps, Sm->offsets,
                       (const S *)Sm->values, (S *)out->values, nb, flip, out->transposed, X, ldx, Y, ldy, k, (int64_t)Sm->num_rows,
                       (int64_t)Sm->num_cols, (float)alpha, (float)beta, mode);
    BMSP_CHECK_LAUNCH();
}

// out's values from S, X and Y through out's layout; out has S's tile order (out == S: in place)
void sddmm_pass(const bmsp_matrix_s *S, bmsp_matrix_s *out, const void *X, int64_t ldx, const void *Y, int64_t ldy, int k, double alpha,
                double beta, int flags, hipStream_t st)
{
    if (out->block_num == 0 || out->nnz == 0) return;
    const Choice ch = choose_kernel(S, X, ldx, Y, ldy);
    const int mode = epilogue_mode(S->dtype, beta, (flags & BMSP_SDDMM_MUL_S) != 0);
    if (ch.tile) {
        if (S->dtype == BMSP_F16) launch_tile<uint16_t>(S, out, X, ldx, Y, ldy, k, alpha, beta, mode, st);
        else launch_tile<float>(S, out, X, ldx, Y, ldy, k, alpha, beta, mode, st);
        return;
    }
    dispatch_dtype(S->dtype, [&](auto s) { launch_value<decltype(s)>(ch, S, out, X, ldx, Y, ldy, k, alpha, beta, mode, st); });
}

// S's keys and offsets, its bitmaps transposed when the layout flips: the structure of a layout conversion, tile order kept
struct CopyPattern {
    const uint64_t *s_keys, *s_bmps, *s_off;
    uint64_t nb;
    int flip;
    uint64_t *keys, *bmps, *offsets;
    __device__ void operator()(uint64_t i) const
    {
        offsets[i] = s_off[i];
        if (i == nb) return;
        keys[i] = s_keys[i];
        const uint64_t b = s_bmps[i];
        bmps[i] = flip ? tile_transpose(b) : b;
    }
};

void check_source(const bmsp_matrix_s *S, const char *what)
{
    refuse_view(S, what);
    if (S->block_num >= (1ll << 32) || S->nnz >= (1ll << 32)) fail(BMSP_ERR_LIMIT, "%s: 2^32 tiles or values or more", what);
}

}  // namespace

void sddmm_check_args(int k, int64_t ldx, int64_t ldy, double beta, int flags, int out_transposed)
{
    if (k < 1) fail(BMSP_ERR_INVALID, "k must be >= 1 (got %d)", k);
    if (ldx < k) fail(BMSP_ERR_INVALID, "ldx must be >= k (got %lld, k = %d)", (long long)ldx, k);
    if (ldy < k) fail(BMSP_ERR_INVALID, "ldy must be >= k (got %lld, k = %d)", (long long)ldy, k);
    if (flags & ~BMSP_SDDMM_MUL_S) fail(BMSP_ERR_INVALID, "flags has unknown bits (got 0x%x)", (unsigned)flags);
    if ((flags & BMSP_SDDMM_MUL_S) && beta != 0.0) fail(BMSP_ERR_INVALID, "beta must be 0 under BMSP_SDDMM_MUL_S (got %g)", beta);
    check_layout_flag(out_transposed, "out_transposed");
}

// a new matrix of S's structure in layout out_transposed with the sampled product as values; what a layout conversion records is recorded
// too, so that sddmm_values_into, scale_values_into and copy_values_from accept the output
bmsp_matrix_s *sddmm_matrix(bmsp_matrix_s *S, const void *X, int64_t ldx, const void *Y, int64_t ldy, int k, double alpha, double beta,
                            int flags, int out_transposed, hipStream_t st)
{
    sddmm_check_args(k, ldx, ldy, beta, flags, out_transposed);
    check_source(S, "sddmm");
    auto m = make_matrix();
    m->num_rows = S->num_rows; m->num_cols = S->num_cols; m->dtype = S->dtype; m->transposed = out_transposed;
    m->nnz = S->nnz; m->block_num = S->block_num;
    m->tp_src_uid = S->uid;
    m->tp_permute = out_transposed != S->transposed ? 1 : 0;
    const uint64_t nb = (uint64_t)S->block_num;
    alloc_tile_arrays(m.get(), nb);
    alloc_values(m.get(), m->nnz);
    device_for_each(CopyPattern{S->keys, S->bmps, S->offsets, nb, m->tp_permute, m->keys, m->bmps, m->offsets}, nb + 1, st);
    sddmm_pass(S, m.get(), X, ldx, Y, ldy, k, alpha, beta, flags, st);
    ensure_rowptr(m.get(), st);
    return m.release();
}

void sddmm_values_into(bmsp_matrix_s *S, const void *X, int64_t ldx, const void *Y, int64_t ldy, int k, double alpha, double beta, int flags,
                       bmsp_matrix_s *out, hipStream_t st)
{
    sddmm_check_args(k, ldx, ldy, beta, flags, 0);
    check_source(S, "sddmm_values");
    if (out != S) {
        // a transpose's output has the source's uid too, but its own tile order (tp_map)
        if (!out->tp_src_uid || out->tp_src_uid != S->uid || out->tp_map)
            fail(BMSP_ERR_INVALID, "sddmm_values: out is neither S nor made from S by bmsp_sddmm, bmsp_matrix_scale or a layout conversion, "
                                   "or S's structure changed since");
        if (S->block_num != out->block_num || S->nnz != out->nnz || S->dtype != out->dtype || S->num_rows != out->num_rows ||
            S->num_cols != out->num_cols)
            fail(BMSP_ERR_INVALID, "sddmm_values: S's and out's sizes or dtypes differ");
    }
    drop_value_caches(out);
    sddmm_pass(S, out, X, ldx, Y, ldy, k, alpha, beta, flags, st);
}

// The launcher's decision for (S, k, ldx, ldy) with 16-byte aligned X and Y, and the bytes that launch moves: 24 B of structure per tile
// (key, bitmap, offset), S's values when the epilogue reads them (counted: launch_info has no beta), the values written, and k elements
// for every X row and Y row a tile touches, once per tile -- the tile kernel touches the min(8, rows left) X rows and min(8, columns left)
// Y rows of its tile, the value kernel the rows and columns that hold a stored value.
void sddmm_launch_info(bmsp_matrix_s *S, int k, int64_t ldx, int64_t ldy, int out_transposed, bmsp_sddmm_info *info)
{
    sddmm_check_args(k, ldx, ldy, 0.0, 0, out_transposed);
    check_source(S, "sddmm_launch_info");
    memset(info, 0, sizeof(*info));
    if (S->block_num == 0 || S->nnz == 0) {
        snprintf(info->kernel, sizeof(info->kernel), "none (empty matrix)");
        return;
    }
    const Choice ch = choose_kernel(S, nullptr, ldx, nullptr, ldy);
    if (ch.tile) snprintf(info->kernel, sizeof(info->kernel), "sddmm_tile_kernel");
    else snprintf(info->kernel, sizeof(info->kernel), "sddmm_value_kernel<%d>", ch.lanes);
    info->lanes = ch.lanes;
    const size_t nb = (size_t)S->block_num;
    std::vector<uint64_t> keys(nb), bmps(nb);
    BMSP_HIP(hipDeviceSynchronize());
    copy_d2h_staged(keys.data(), S->keys, nb * sizeof(uint64_t));
    copy_d2h_staged(bmps.data(), S->bmps, nb * sizeof(uint64_t));
    int64_t x_rows = 0, y_rows = 0;
    for (size_t t = 0; t < nb; t++) {
        if (ch.tile) {
            const int64_t r = (int64_t)S->num_rows - 8 * (int64_t)key_row(keys[t]), c = (int64_t)S->num_cols - 8 * (int64_t)key_col(keys[t]);
            x_rows += r < 8 ? r : 8;
            y_rows += c < 8 ? c : 8;
        } else {
            // bytes of the bitmap that hold a value / bit columns in use: rows and columns of a row-major tile, swapped for a column-major one
            int bytes = 0;
            for (int i = 0; i < 8; i++) bytes += tile_byte(bmps[t], i) != 0;
            const int bits = popc64((uint64_t)tile_or_bytes(bmps[t]));
            x_rows += S->transposed ? bits : bytes;
            y_rows += S->transposed ? bytes : bits;
        }
    }
    const int64_t es = (int64_t)dtype_size(S->dtype);
    info->compulsory_bytes = 24 * (int64_t)nb + 2 * S->nnz * es + (x_rows + y_rows) * (int64_t)k * es;
}

}  // namespace bmsp

BMSP_DEFINE_WARM(sddmm)
