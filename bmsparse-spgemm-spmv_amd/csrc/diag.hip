// diag.hip -- what connects a device VECTOR to a matrix already on the device, besides the SpMV: reading the diagonal
// (bmsp_matrix_diagonal), making a diagonal matrix (bmsp_matrix_from_diagonal) and scaling rows and columns, out = diag(l) * A * diag(r)
// (bmsp_matrix_scale / bmsp_matrix_scale_values), without going back through scalar COO entries.
//
// None of the three changes or searches a structure.  A scaled matrix has A's keys, offsets and (possibly transposed) bitmaps; a diagonal
// matrix has tile t = {key (t, t), positions 0, 9, .., 63, offset 8t}; the diagonal of A lives in the tiles with block_row == block_col at
// those same positions in either layout.  Nothing is sorted, scanned or read back, no pass needs an atomic: every output element has
// exactly one writer.
//
// Passes:
//   diagonal       a lane per diagonal entry i: binary search of key (i/8, i/8) inside block-row i/8 (the cached block-row pointer), then
//                  one bitmap test and at most one value load.  The eight lanes of a block-row search the same addresses (one request) and
//                  store eight neighbouring outputs; an absent entry stores +0, so the output needs no clearing pass.
//   from_diagonal  one for_each over max(entries, tiles + 1, block-rows + 1) indices writes values, keys, bitmaps, offsets and the
//                  block-row pointer from the closed form.
//   scale          a for_each copies keys and offsets and writes the bitmaps (transposed when the layout flips), then the value pass;
//                  scale_values is the value pass alone.
//   value pass     G lanes per tile (lane_group, tile_pass.hip.h).  G = 8: lane t takes byte t of the OUTPUT bitmap (a
//                  row of a row-major tile, a column of a column-major one), loads l[8*brow + t] and r[8*bcol + t] -- the two 32-byte
//                  segments of the tile, one load per lane group -- keeps the factor its byte shares and fetches the other per position
//                  with a wave shuffle inside the group.  G = 1 (tiles of 1 - 5 values): a lane walks its tile and loads the two factors of
//                  each value; preloading sixteen to use two or three costs more than the cached loads it would save.
//                  Multiply and divide are compile-time variants per side: x / d is the IEEE division sequence, never a reciprocal.
#include "tile_pass.hip.h"

namespace bmsp {
namespace {

// one side of the scaling: an IEEE multiply or an IEEE divide, each rounded on its own
template <bool DIV, typename F>
__device__ __forceinline__ F apply_factor(F x, F d)
{
#pragma clang fp contract(off)
    if (DIV) return x / d;
    return x * d;
}

// ---- diagonal -------------------------------------------------------------------------------------------------------------------------
template <typename S>
struct ReadDiagonal {
    using D = TileValue<S>;
    const uint64_t *keys, *bmps, *offsets;
    const S *vals;
    const uint32_t *rowptr;
    typename D::R *diag;
    __device__ void operator()(uint64_t i) const
    {
        const uint32_t br = (uint32_t)(i >> 3);
        const int p = 9 * (int)(i & 7);
        const uint64_t want = key_make(br, br);
        const uint32_t begin = rowptr[br], end = rowptr[br + 1];
        const uint32_t lo = lower_bound_key(keys, begin, end, want);
        typename D::R out = 0;
        if (lo < end && keys[lo] == want) {
            const uint64_t b = bmps[lo];
            if (tile_has(b, p)) out = D::load(vals[offsets[lo] + tile_rank(b, p)]);  // (exact: R is F)
        }
        diag[i] = out;
    }
};

// ---- from_diagonal --------------------------------------------------------------------------------------------------------------------
template <typename S>
struct MakeDiagonal {
    using D = TileValue<S>;
    const typename D::R *diag;
    uint64_t n, nt, nbr;  // entries, tiles, block-rows of the matrix
    uint64_t *keys, *bmps, *offsets;
    S *vals;
    uint32_t *rowptr;
    __device__ void operator()(uint64_t i) const
    {
        if (i < n) vals[i] = D::store(diag[i]);
        if (i < nt) {
            const uint64_t cnt = n - 8 * i < 8 ? n - 8 * i : 8;  // entries of the last tile
            keys[i] = key_make((uint32_t)i, (uint32_t)i);
            bmps[i] = tile_diagonal_mask() & (~0ull << (63 - 9 * (cnt - 1)));
        }
        if (i <= nt) offsets[i] = i < nt ? 8 * i : n;
        if (i <= nbr) rowptr[i] = (uint32_t)(i < nt ? i : nt);  // block-rows below the diagonal's end are empty
    }
};

// ---- scale ----------------------------------------------------------------------------------------------------------------------------
struct CopyStructure {
    const uint64_t *a_keys, *a_bmps, *a_off;
    uint64_t nb;
    int flip;
    uint64_t *keys, *bmps, *offsets;
    __device__ void operator()(uint64_t i) const
    {
        offsets[i] = a_off[i];
        if (i == nb) return;
        keys[i] = a_keys[i];
        const uint64_t b = a_bmps[i];
        bmps[i] = flip ? tile_transpose(b) : b;
    }
};

// Value pass over tiles [0, nb): out tile j = l (rows) * A tile j * r (columns), read through A's bitmap (the transposed position when
// the layout flips).  a_vals and o_vals may be the same array (in place: flip == 0, value k of a tile is read and written by one lane).
// A null l or r skips that side; with both null the values move unchanged.  Every lane stays to the end of the G = 8 form: the
// shuffles need the whole lane group.
template <typename S, int G, bool DL, bool DR>
__global__ __launch_bounds__(kThreads) void scale_values_kernel(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ a_bmps,
                                                                const uint64_t *__restrict__ offsets, const S *a_vals, S *o_vals,
                                                                uint64_t nb, int flip, int olay,
                                                                const typename TileValue<S>::R *__restrict__ l,
                                                                const typename TileValue<S>::R *__restrict__ r, int64_t num_rows,
                                                                int64_t num_cols)
{
    using D = TileValue<S>;
    using F = typename D::F;
    using R = typename D::R;
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t j = gid / G;
    const int t = (int)(gid % G);
    const bool live = j < nb;
    const bool has_l = l != nullptr, has_r = r != nullptr;
    uint64_t ib = 0, off = 0;
    int64_t row0 = 0, col0 = 0;
    if (live) {
        const uint64_t key = keys[j];
        ib = a_bmps[j];
        off = offsets[j];
        row0 = (int64_t)key_row(key) * 8;
        col0 = (int64_t)key_col(key) * 8;
    }
    const uint64_t ob = flip ? tile_transpose(ib) : ib;
    const S *src = a_vals + off;
    if (G == 8) {
        // lane t: byte t of the output bitmap = row t (olay 0) or column t (olay 1) of the tile; its own factor stays in a register,
        // the factor of the other side comes from the lane of the group that loaded it
        R lt = 0, rt = 0;
        if (live && has_l && row0 + t < num_rows) lt = l[row0 + t];  // (the ragged last block-row / block-column)
        if (live && has_r && col0 + t < num_cols) rt = r[col0 + t];
        const R own = olay ? rt : lt, others = olay ? lt : rt;
        const bool need_others = olay ? has_l : has_r;
        const int base = lane_id() & ~7;
        R oth_c[8];  // (all eight shuffles before the lanes diverge on their bitmap bytes)
#pragma unroll
        for (int c = 0; c < 8; c++) oth_c[c] = need_others ? __shfl(others, base + c, kWave) : R(0);
        const uint32_t byte = tile_byte(ob, t);
        S *dst = o_vals + off + tile_rank(ob, 8 * t);
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const R oth = oth_c[c];
            if (!(byte & (0x80u >> c))) continue;
            const int p = 8 * t + c;
            const S v = src[tile_rank(ib, flip ? tile_transposed_pos(p) : p)];
            if (!has_l && !has_r) {
                *dst++ = v;
                continue;
            }
            F x = D::load(v);
            if (has_l) x = apply_factor<DL, F>(x, (F)(olay ? oth : own));
            if (has_r) x = apply_factor<DR, F>(x, (F)(olay ? own : oth));
            *dst++ = D::store(x);
        }
    } else {  // one lane walks the stored positions of the output tile in order
        if (!live) return;
        S *dst = o_vals + off;
        uint64_t m = ob;
        while (m) {
            const int p = tile_pop_first(m);
            const S v = src[tile_rank(ib, flip ? tile_transposed_pos(p) : p)];
            if (!has_l && !has_r) {
                *dst++ = v;
                continue;
            }
            const int row = olay ? (p & 7) : (p >> 3), col = olay ? (p >> 3) : (p & 7);
            F x = D::load(v);
            if (has_l) x = apply_factor<DL, F>(x, (F)l[row0 + row]);
            if (has_r) x = apply_factor<DR, F>(x, (F)r[col0 + col]);
            *dst++ = D::store(x);
        }
    }
}

template <typename S, bool DL, bool DR>
void launch_scale(int g, const bmsp_matrix_s *A, bmsp_matrix_s *out, const void *l, const void *r, hipStream_t st)
{
    using R = typename TileValue<S>::R;
    const uint64_t nb = (uint64_t)out->block_num;
    const int flip = A->transposed != out->transposed;
    launch_lane_group(g, nb, [&](auto lanes, dim3 grid) {
        hipLaunchKernelGGL((scale_values_kernel<S, decltype(lanes)::value, DL, DR>), grid, dim3(kThreads), 0, st, A->keys, A->bmps,
                           A->offsets, (const S *)A->values, (S *)out->values, nb, flip, out->transposed, (const R *)l, (const R *)r,
                           (int64_t)out->num_rows, (int64_t)out->num_cols);
    });
}

template <typename S>
void launch_scale_flags(int g, const bmsp_matrix_s *A, bmsp_matrix_s *out, const void *l, const void *r, int flags, hipStream_t st)
{
    // a null side never divides: its flag was refused, the multiply-only variant serves
    const bool dl = l && (flags & BMSP_SCALE_DIV_LEFT), dr = r && (flags & BMSP_SCALE_DIV_RIGHT);
    if (dl && dr) launch_scale<S, true, true>(g, A, out, l, r, st);
    else if (dl) launch_scale<S, true, false>(g, A, out, l, r, st);
    else if (dr) launch_scale<S, false, true>(g, A, out, l, r, st);
    else launch_scale<S, false, false>(g, A, out, l, r, st);
}

// out's values = diag(l) * A * diag(r) through out's layout; out has A's tile order (out == A: in place)
void scale_pass(const bmsp_matrix_s *A, bmsp_matrix_s *out, const void *l, const void *r, int flags, hipStream_t st)
{
    if (out->block_num == 0 || out->nnz == 0) return;
    const int g = lane_group(out->nnz, out->block_num, "BMSP_SCALE_LANES");
    dispatch_dtype(out->dtype, [&](auto s) { launch_scale_flags<decltype(s)>(g, A, out, l, r, flags, st); });
}

void check_source(const bmsp_matrix_s *A, const char *what)
{
    refuse_view(A, what);
    if (A->block_num >= (1ll << 32)) fail(BMSP_ERR_LIMIT, "%s: more than 2^32 blocks", what);
}

}  // namespace

void scale_check_args(const void *d_left, const void *d_right, int flags, int out_transposed)
{
    if (flags & ~(BMSP_SCALE_DIV_LEFT | BMSP_SCALE_DIV_RIGHT)) fail(BMSP_ERR_INVALID, "flags has unknown bits (got 0x%x)", (unsigned)flags);
    check_layout_flag(out_transposed, "out_transposed");
    if ((flags & BMSP_SCALE_DIV_LEFT) && !d_left) fail(BMSP_ERR_INVALID, "flags has BMSP_SCALE_DIV_LEFT but d_left is null");
    if ((flags & BMSP_SCALE_DIV_RIGHT) && !d_right) fail(BMSP_ERR_INVALID, "flags has BMSP_SCALE_DIV_RIGHT but d_right is null");
}

void from_diagonal_check_args(int num_rows, int num_cols, const void *d_diag, bmsp_dtype dtype, int transposed)
{
    if (num_rows < 0 || num_cols < 0) fail(BMSP_ERR_INVALID, "num_rows and num_cols must be >= 0 (got %d x %d)", num_rows, num_cols);
    if (dtype != BMSP_F32 && dtype != BMSP_F16 && dtype != BMSP_F64) fail(BMSP_ERR_INVALID, "unknown dtype %d", (int)dtype);
    check_layout_flag(transposed, "transposed");
    if (!d_diag && num_rows > 0 && num_cols > 0) fail(BMSP_ERR_INVALID, "d_diag is null");
}

// d_diag[i] = the stored value at (i, i), +0 where none is stored; min(num_rows, num_cols) entries
void matrix_diagonal(bmsp_matrix_s *A, void *d_diag, hipStream_t st)
{
    check_source(A, "diagonal");
    const uint64_t n = (uint64_t)(A->num_rows < A->num_cols ? A->num_rows : A->num_cols);
    if (n == 0) return;
    ensure_rowptr(A, st);
    dispatch_dtype(A->dtype, [&](auto s) {
        using S = decltype(s);
        using R = typename TileValue<S>::R;
        device_for_each(ReadDiagonal<S>{A->keys, A->bmps, A->offsets, (const S *)A->values, A->rowptr, (R *)d_diag}, n, st);
    });
}

// the num_rows x num_cols matrix with d_diag[i] stored at every (i, i), tiles in layout `transposed`
bmsp_matrix_s *matrix_from_diagonal(int num_rows, int num_cols, const void *d_diag, bmsp_dtype dtype, int transposed, hipStream_t st)
{
    from_diagonal_check_args(num_rows, num_cols, d_diag, dtype, transposed);
    auto m = make_matrix();
    const uint64_t n = (uint64_t)(num_rows < num_cols ? num_rows : num_cols), nt = (n + 7) / 8;
    m->num_rows = num_rows; m->num_cols = num_cols; m->dtype = dtype; m->transposed = transposed;
    m->nnz = (int64_t)n; m->block_num = (int64_t)nt;
    const uint64_t nbr = (uint64_t)m->num_block_rows();
    alloc_tile_arrays(m.get(), nt);
    alloc_values(m.get(), n);
    m->rowptr.alloc((size_t)(nbr + 1));
    m->rowptr_rows = (int64_t)nbr;
    const uint64_t work = n > nbr + 1 ? n : nbr + 1;  // (nt <= nbr)
    dispatch_dtype(dtype, [&](auto s) {
        using S = decltype(s);
        using R = typename TileValue<S>::R;
        device_for_each(MakeDiagonal<S>{(const R *)d_diag, n, nt, nbr, m->keys, m->bmps, m->offsets, (S *)m->values, m->rowptr}, work, st);
    });
    return m.release();
}

// out = diag(l) * A * diag(r) as a new matrix with tiles in layout out_transposed; what a layout conversion records is recorded too, so
// that scale_values_into and copy_values_from accept the output
bmsp_matrix_s *scale_matrix(bmsp_matrix_s *A, const void *d_left, const void *d_right, int flags, int out_transposed, hipStream_t st)
{
    scale_check_args(d_left, d_right, flags, out_transposed);
    check_source(A, "scale");
    auto m = make_matrix();
    m->num_rows = A->num_rows; m->num_cols = A->num_cols; m->dtype = A->dtype; m->transposed = out_transposed;
    m->nnz = A->nnz; m->block_num = A->block_num;
    m->tp_src_uid = A->uid;
    m->tp_permute = out_transposed != A->transposed ? 1 : 0;
    const uint64_t nb = (uint64_t)A->block_num;
    alloc_tile_arrays(m.get(), nb);
    alloc_values(m.get(), m->nnz);
    device_for_each(CopyStructure{A->keys, A->bmps, A->offsets, nb, m->tp_permute, m->keys, m->bmps, m->offsets}, nb + 1, st);
    scale_pass(A, m.get(), d_left, d_right, flags, st);
    ensure_rowptr(m.get(), st);
    return m.release();
}

void scale_values_into(bmsp_matrix_s *A, const void *d_left, const void *d_right, int flags, bmsp_matrix_s *out, hipStream_t st)
{
    scale_check_args(d_left, d_right, flags, 0);
    check_source(A, "scale_values");
    if (out != A) {
        // a transpose's output has the source's uid too, but its own tile order (tp_map)
        if (!out->tp_src_uid || out->tp_src_uid != A->uid || out->tp_map)
            fail(BMSP_ERR_INVALID, "scale_values: out is neither A nor made from A by bmsp_matrix_scale or a layout conversion, or A's "
                                   "structure changed since");
        if (A->block_num != out->block_num || A->nnz != out->nnz || A->dtype != out->dtype || A->num_rows != out->num_rows ||
            A->num_cols != out->num_cols)
            fail(BMSP_ERR_INVALID, "scale_values: A's and out's sizes or dtypes differ");
    }
    drop_value_caches(out);
    scale_pass(A, out, d_left, d_right, flags, st);
}

}  // namespace bmsp

BMSP_DEFINE_WARM(diag)
