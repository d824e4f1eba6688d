// fsai.hip -- the factorised sparse approximate inverse on a prescribed lower-triangular pattern (bmsp_matrix_fsai / _values) and the
// preconditioner handle that applies it by two sparse products (bmsp_fsai_create / _update / _apply / _solve / _solve_gmres).
// include/bmsp.h writes the arithmetic out operation by operation; tests/fsai_ref.c restates it.
//
// Row i of G needs the m x m matrix B = op(A)[P, P] on the stored columns P = (p_1 < .. < p_m = i) of row i of the pattern, its LU
// factorisation without pivoting and the solve y^T B = e_m^T.  Rows are independent: no levels, no sweeps, no hand-off between rows.
//
// Kernels:
//   fsai_pattern_row    one lane per row of the pattern: its length, and the first rows that miss the diagonal, store a column to
//                  its right or hold more than 64 entries (integer atomicMin, taken only by the rows that have something to report).
//                  The host bounds m with it before the row kernel is launched.
//   fsai_row_kernel<S, W>   W lanes per row, 64 / W rows per wave, one wave per workgroup.  Lane a finds p_a by walking the row's tiles,
//                  gathers row p_a of op(A) on P -- one binary search in A's block-row per distinct block column of P, the lower bound
//                  moving forward, so a hub row of A under a short P and a P that spans far-apart block columns cost the same few
//                  probes -- and owns row a of B in LDS (pitch W + 1: the lanes of a group hit W different banks).  LU: at step k every
//                  lane a > k reads row k (one address per group: a broadcast) and updates its own row; one barrier per step.  The
//                  solve for y runs a = m - 1 .. 1 in lane a, each y_a one chain over c ascending.  Every B_ab is one chain in k order
//                  and every y_a one chain in c order, whoever computes them: the bits are the text's for every W.
//                  LDS is sized from W alone; the host refuses a row longer than 64 before anything is launched.
// No flag, no spin, no floating-point atomic: the only atomic of the row kernel is the integer count of rows that hold a non-finite value.
// op T runs on a temporary bmsp_matrix_transpose(A), freed before the call returns.
#include "spsv_plan.hip.h"
#include <cmath>
#include <string>

// The handle: A is borrowed; the factors, the materialised transpose and the work vector are owned.
struct bmsp_fsai_s {
    bmsp_matrix_s *A = nullptr;
    int kind = 0, flags = 0;
    bmsp::MatrixPtr G1, G2own, G2t;  // G2own: the second factor of the GENERAL kind (SPD: G2 is G1)
    bmsp_fsai_info info1{}, info2{};
    bmsp::DevBuf<void> work;         // t = G1 r
    bmsp_matrix_s *G2() const { return G2own ? G2own.get() : G1.get(); }
};

namespace bmsp {
namespace {

constexpr int kMaxRow = 64;

// the stored columns of row r of a tile as a byte, bit (7 - c) = column c, for either tile layout
__device__ __forceinline__ uint32_t row_bits(uint64_t bmp, int r, int lay)
{
    if (!lay) return tile_byte(bmp, r);
    const uint64_t x = (bmp >> (7 - r)) & 0x0101010101010101ull;  // byte c (0 = most significant) holds (r, c)
    return (uint32_t)((x * 0x0102040810204080ull) >> 56);
}

// facts[0]: first row without a stored diagonal; facts[1]: first row that stores a column right of the diagonal; facts[2]: (row << 32 |
// length) of the first row longer than kMaxRow -- all ~0 when there is none
struct PatternRow {
    const uint64_t *keys, *bmps;
    const uint32_t *ptr;
    int lay;
    uint32_t *len;
    unsigned long long *facts;
    __device__ void operator()(uint64_t i) const
    {
        const uint32_t I = (uint32_t)(i >> 3);
        const int r = (int)(i & 7);
        uint32_t cnt = 0;
        bool diag = false, right = false;
        for (uint32_t t = ptr[I]; t < ptr[I + 1]; t++) {
            const uint32_t bits = row_bits(bmps[t], r, lay), bc = key_col(keys[t]);
            cnt += (uint32_t)__builtin_popcount(bits);
            if (bc == I) {
                diag = diag || (bits & (0x80u >> r));
                right = right || (bits & ((0x80u >> r) - 1u));
            } else if (bc > I && bits) {
                right = true;
            }
        }
        len[i] = cnt;
        if (!diag) atomicMin(facts + 0, (unsigned long long)i);
        if (right) atomicMin(facts + 1, (unsigned long long)i);
        if (cnt > (uint32_t)kMaxRow) atomicMin(facts + 2, (unsigned long long)i << 32 | cnt);
    }
};

struct SquaredLength {
    const uint32_t *len;
    __device__ uint64_t operator()(uint64_t i) const { return (uint64_t)len[i] * len[i]; }
};

template <typename S>
struct RowArgs {
    const uint64_t *a_keys, *a_bmps, *a_off;
    const uint32_t *a_ptr;
    const S *a_vals;
    const uint64_t *g_keys, *g_bmps, *g_off;
    const uint32_t *g_ptr;
    S *g_vals;
    S *pivot;
    uint32_t *bad;
    int64_t n;
    int alay, glay, scale;
};

template <typename S, int W>
__global__ __launch_bounds__(kWave) void fsai_row_kernel(RowArgs<S> p)
{
#pragma clang fp contract(off)
    using D = TileValue<S>;
    constexpr int kRows = kWave / W, kPitch = W + 1;
    __shared__ S Bs[kRows * W * kPitch];
    __shared__ S Ys[kWave];
    __shared__ uint32_t Ps[kWave];
    // (no lane leaves before the end: every barrier and shuffle below is reached by the whole wave)
    const int lane = (int)threadIdx.x, g = lane / W, a = lane % W;
    const int64_t i = (int64_t)blockIdx.x * kRows + g;
    const int r = (int)(i & 7);

    // P: lane a takes the a-th stored column of row i and the place of (i, p_a) in G's values
    int m = 0;
    uint32_t mycol = 0, myidx = 0;
    if (i < p.n) {
        const uint32_t I = (uint32_t)(i >> 3);
        for (uint32_t t = p.g_ptr[I]; t < p.g_ptr[I + 1]; t++) {
            const uint64_t bmp = p.g_bmps[t];
            uint32_t bits = row_bits(bmp, r, p.glay);
            const int cnt = __builtin_popcount(bits);
            if (a >= m && a < m + cnt) {
                int c = 0;
                for (int q = a - m;; q--) {
                    c = __builtin_clz(bits) - 24;
                    if (q == 0) break;
                    bits &= ~(0x80u >> c);
                }
                mycol = key_col(p.g_keys[t]) * 8 + (uint32_t)c;
                myidx = (uint32_t)p.g_off[t] + (uint32_t)tile_rank(bmp, p.glay ? 8 * c + r : 8 * r + c);
            }
            m += cnt;
        }
        if (m > W) m = W;  // (the host bounded the longest row by W; never taken)
    }
    Ps[lane] = mycol;
    __syncthreads();

    // B: lane a gathers row p_a of op(A) on the columns P
    S *row = Bs + (g * W + a) * kPitch;
    const uint32_t *P = Ps + g * W;
    if (a < m) {
        const uint32_t IA = mycol >> 3;
        const int ra = (int)(mycol & 7);
        uint32_t lo = p.a_ptr[IA];
        const uint32_t hi = p.a_ptr[IA + 1];
        uint32_t have = ~0u, off = 0;
        uint64_t bmp = 0;
        for (int b = 0; b < m; b++) {
            const uint32_t col = P[b], bc = col >> 3;
            if (bc != have) {
                have = bc;
                const uint64_t key = key_make(IA, bc);
                lo = lower_bound_key(p.a_keys, lo, hi, key);
                const bool found = lo < hi && p.a_keys[lo] == key;
                bmp = found ? p.a_bmps[lo] : 0ull;
                off = found ? (uint32_t)p.a_off[lo] : 0u;
            }
            const int c = (int)(col & 7), pos = p.alay ? 8 * c + ra : 8 * ra + c;
            row[b] = tile_has(bmp, pos) ? p.a_vals[off + (uint32_t)tile_rank(bmp, pos)] : S(0);
        }
    }
    int mmax = m;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int o = __shfl_xor(mmax, d, kWave);
        mmax = o > mmax ? o : mmax;
    }
    __syncthreads();

    // LU without pivoting: row k is final when step k starts, and only its owner has written it
    for (int k = 0; k + 1 < mmax; k++) {
        if (a > k && a < m) {
            const S *rk = Bs + (g * W + k) * kPitch;
            const S l = row[k] / rk[k];
            row[k] = l;
            const S nl = -l;
            for (int b = k + 1; b < m; b++) row[b] = fused(nl, rk[b], row[b]);
        }
        __syncthreads();
    }

    // y^T B = e_m^T: y_m = 1 / B_mm, then y_a = -sum_{c > a} L_ca y_c, one chain per a in c order
    S *Y = Ys + g * W;
    if (m > 0 && a == m - 1) Y[a] = S(1) / row[a];
    __syncthreads();
    for (int k = mmax - 2; k >= 0; k--) {
        if (a == k && k + 1 < m) {
            S s = S(0);
            for (int c = k + 1; c < m; c++) s = fused(-Bs[(g * W + c) * kPitch + k], Y[c], s);
            Y[k] = s;
        }
        __syncthreads();
    }

    bool bad = false;
    if (a < m) {
        const S ym = Y[m - 1], ya = Y[a];
        S gv = ya;
        if (p.scale == BMSP_FSAI_SCALE_SQRT) {
            const S q = (S)__builtin_sqrt((double)ym);  // (for a float the double root rounded once more is the correctly rounded root)
            gv = ya / q;
        } else if (p.scale == BMSP_FSAI_SCALE_UNIT) {
            gv = ya / ym;
        }
        p.g_vals[myidx] = gv;
        bad = D::abs_bits(gv) >= D::kInf;
        if (a == m - 1 && p.pivot) p.pivot[i] = ym;
    }
    const uint64_t group = W == kWave ? ~0ull : ((1ull << (W & 63)) - 1ull) << (g * W);
    if ((__ballot(bad) & group) && a == 0) atomicAdd(p.bad, 1u);
}

struct Pattern {
    int64_t max_row = 0, pairs = 0;
};

// the pattern's facts, and its refusals: synchronises `st`
Pattern check_pattern(bmsp_matrix_s *S, const char *name, hipStream_t st)
{
    Pattern pt;
    const uint64_t n = (uint64_t)S->num_rows;
    if (n == 0) return pt;
    ensure_rowptr(S, st);
    DevBuf<uint32_t> len((size_t)n);
    DevBuf<unsigned long long> facts(5);
    BMSP_HIP(hipMemsetAsync(facts.p, 0xff, 3 * sizeof(unsigned long long), st));
    BMSP_HIP(hipMemsetAsync(facts.p + 3, 0, 2 * sizeof(unsigned long long), st));
    device_for_each(PatternRow{S->keys, S->bmps, S->rowptr, S->transposed, len.p, facts.p}, n, st);
    device_max_sum(SquaredLength{len.p}, n, facts.p + 3, facts.p + 4, st);
    unsigned long long h[5];
    read_back_bytes(h, facts.p, sizeof h, st);
    if (h[0] != ~0ull) fail(BMSP_ERR_INVALID, "matrix %s: row %lld of %s has no stored diagonal entry", name, (long long)h[0], name);
    if (h[1] != ~0ull)
        fail(BMSP_ERR_INVALID, "matrix %s: row %lld of %s stores a column to the right of the diagonal", name, (long long)h[1], name);
    if (h[2] != ~0ull)
        fail(BMSP_ERR_LIMIT, "matrix %s: row %lld of %s has %lld stored entries, at most %d (thin the pattern first, bmsp_matrix_prune)", name,
             (long long)(h[2] >> 32), name, (long long)(h[2] & 0xffffffffull), kMaxRow);
    pt.max_row = (int64_t)std::llround(std::sqrt((double)h[3]));
    pt.pairs = (int64_t)h[4];
    return pt;
}

// W: the smallest of 8, 16, 32, 64 that holds the longest row; BMSP_FSAI_LANES=<W> (read per call) forces a larger one
int lanes_for(int64_t max_row)
{
    int w = 8;
    while (w < max_row) w *= 2;
    if (const char *e = getenv("BMSP_FSAI_LANES")) {
        const int f = atoi(e);
        if ((f == 8 || f == 16 || f == 32 || f == 64) && f > w) w = f;
    }
    return w;
}

const char *dtype_label(bmsp_dtype t) { return t == BMSP_F64 ? "F64" : "F32"; }

template <typename S, int W>
void launch_rows(const RowArgs<S> &p, hipStream_t st)
{
    const uint64_t rows_per = (uint64_t)(kWave / W);
    const uint64_t blocks = ((uint64_t)p.n + rows_per - 1) / rows_per;
    if (blocks > 0x7fffffffull) fail(BMSP_ERR_LIMIT, "fsai: grid too large");
    hipLaunchKernelGGL((fsai_row_kernel<S, W>), dim3((unsigned)blocks), dim3(kWave), 0, st, p);
    BMSP_CHECK_LAUNCH();
}

// G's values from op(A) on G's own pattern (checked: pt); synchronises `st` for the count of bad rows
void fill_factor(bmsp_matrix_s *A, int op, bmsp_matrix_s *G, int scale, void *d_pivot, const Pattern &pt, hipStream_t st, bmsp_fsai_info *info)
{
    memset(info, 0, sizeof *info);
    info->rows = G->num_rows;
    info->max_row = pt.max_row;
    info->pairs = pt.pairs;
    if (G->num_rows == 0) {
        snprintf(info->kernel, sizeof info->kernel, "none (empty matrix)");
        return;
    }
    const int W = lanes_for(pt.max_row);
    const int64_t es = (int64_t)dtype_size(G->dtype);
    info->lanes = W;
    info->lds_bytes = es * kWave * (W + 1) + es * kWave + 4 * kWave;
    snprintf(info->kernel, sizeof info->kernel, "fsai_row_kernel<%s, %d>", dtype_label(G->dtype), W);
    MatrixPtr At;
    bmsp_matrix_s *M = A;
    if (op == BMSP_OP_T) {
        At = own_matrix(transpose_matrix(A, A->transposed, true, st));
        M = At.get();
    }
    ensure_rowptr(M, st);
    ensure_rowptr(G, st);
    DevBuf<uint32_t> bad(1);
    BMSP_HIP(hipMemsetAsync(bad.p, 0, 4, st));
    dispatch_dtype(G->dtype, [&](auto s) {
        using S = decltype(s);
        if constexpr (!std::is_same<S, uint16_t>::value) {
            RowArgs<S> p;
            p.a_keys = M->keys; p.a_bmps = M->bmps; p.a_off = M->offsets; p.a_ptr = M->rowptr; p.a_vals = (const S *)M->values;
            p.g_keys = G->keys; p.g_bmps = G->bmps; p.g_off = G->offsets; p.g_ptr = G->rowptr; p.g_vals = (S *)G->values;
            p.pivot = (S *)d_pivot; p.bad = bad.p; p.n = G->num_rows;
            p.alay = M->transposed; p.glay = G->transposed; p.scale = scale;
            if (W == 8) launch_rows<S, 8>(p, st);
            else if (W == 16) launch_rows<S, 16>(p, st);
            else if (W == 32) launch_rows<S, 32>(p, st);
            else launch_rows<S, 64>(p, st);
        }
    });
    info->bad_rows = (int64_t)read_back(bad.p, st);  // (the temporary transpose and the counter go back to the pool behind this)
}

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

void check_one(const bmsp_matrix_s *M, const char *name)
{
    char what[32];
    snprintf(what, sizeof what, "fsai: matrix %s", name);
    refuse_view(M, what);
    if (M->block_num >= (1ll << 32) || M->nnz >= (1ll << 32)) fail(BMSP_ERR_LIMIT, "fsai: matrix %s: 2^32 tiles or values or more", name);
}

// a view bmsp_spmv_op needs for (M, op), or bmsp_spmv's own plan
void ensure_product(bmsp_matrix_s *M, int op, hipStream_t st)
{
    if (M->num_rows == 0) return;
    if (op == BMSP_OP_N && !M->transposed) prepare_spmv(M, st);
    else spmv_op_ensure_view(M, op, st);
}

}  // namespace

void fsai_check_args(int op, int scale, int out_transposed)
{
    spmv_op_check_op(op);
    if (scale < BMSP_FSAI_SCALE_NONE || scale > BMSP_FSAI_SCALE_UNIT)
        fail(BMSP_ERR_INVALID, "scale must be BMSP_FSAI_SCALE_NONE (0), _SQRT (1) or _UNIT (2) (got %d)", scale);
    check_layout_flag(out_transposed, "out_transposed");
}

// the refusals that read the handles, host only; `name` is "S" (bmsp_matrix_fsai) or "G" (bmsp_matrix_fsai_values)
void fsai_check_matrices(const bmsp_matrix_s *A, const bmsp_matrix_s *P, const char *name)
{
    if (A->dtype == BMSP_F16) fail(BMSP_ERR_UNSUPPORTED, "fsai: an F16 matrix A is not supported (the factor would be fp16)");
    if (A->num_rows != A->num_cols) fail(BMSP_ERR_INVALID, "fsai: matrix A must be square (it is %d x %d)", A->num_rows, A->num_cols);
    check_one(A, "A");
    if (P->num_rows != A->num_rows || P->num_cols != A->num_cols)
        fail(BMSP_ERR_INVALID, "fsai: matrix %s must have A's shape (%s is %d x %d, A is %d x %d)", name, name, P->num_rows, P->num_cols,
             A->num_rows, A->num_cols);
    check_one(P, name);
    if (name[0] == 'G') {
        if (P == A) fail(BMSP_ERR_INVALID, "fsai_values: matrix G is A: A is read while G is written");
        if (P->dtype != A->dtype) fail(BMSP_ERR_INVALID, "fsai_values: matrix G: dtype differs from A's");
    }
}

bmsp_matrix_s *fsai_matrix(bmsp_matrix_s *A, int op, bmsp_matrix_s *S, int scale, int out_transposed, void *d_pivot, hipStream_t st,
                           bmsp_fsai_info *info)
{
    fsai_check_args(op, scale, out_transposed);
    fsai_check_matrices(A, S, "S");
    const Pattern pt = check_pattern(S, "S", st);
    auto G = make_matrix();
    G->num_rows = S->num_rows; G->num_cols = S->num_cols; G->dtype = A->dtype; G->transposed = out_transposed;
    G->nnz = S->nnz; G->block_num = S->block_num;
    const uint64_t nb = (uint64_t)S->block_num;
    alloc_tile_arrays(G.get(), nb);
    alloc_values(G.get(), (uint64_t)G->nnz);
    device_for_each(CopyPattern{S->keys, S->bmps, S->offsets, nb, out_transposed != S->transposed ? 1 : 0, G->keys, G->bmps, G->offsets}, nb + 1, st);
    fill_factor(A, op, G.get(), scale, d_pivot, pt, st, info);
    if (G->num_rows == 0) BMSP_HIP(hipStreamSynchronize(st));
    return G.release();
}

void fsai_values_into(bmsp_matrix_s *A, int op, bmsp_matrix_s *G, int scale, void *d_pivot, hipStream_t st, bmsp_fsai_info *info)
{
    fsai_check_args(op, scale, 0);
    fsai_check_matrices(A, G, "G");
    const Pattern pt = check_pattern(G, "G", st);
    drop_value_caches(G);
    fill_factor(A, op, G, scale, d_pivot, pt, st, info);
}

// ---- the handle -----------------------------------------------------------------------------------------------------------------------
void fsai_create_check_args(int kind, int flags)
{
    if (kind != BMSP_FSAI_SPD && kind != BMSP_FSAI_GENERAL)
        fail(BMSP_ERR_INVALID, "kind must be BMSP_FSAI_SPD (0) or BMSP_FSAI_GENERAL (1) (got %d)", kind);
    if (flags & ~(BMSP_FSAI_NO_MATERIALISE | BMSP_FSAI_COLMAJOR))
        fail(BMSP_ERR_INVALID, "flags: unknown bits (got %d; BMSP_FSAI_NO_MATERIALISE = 1 and BMSP_FSAI_COLMAJOR = 2 are the only ones)", flags);
}

static void build_views(bmsp_fsai_s *f, hipStream_t st)
{
    ensure_product(f->G1.get(), BMSP_OP_N, st);
    if (f->G2t) ensure_product(f->G2t.get(), BMSP_OP_N, st);
    else ensure_product(f->G2(), BMSP_OP_T, st);
}

bmsp_fsai_s *fsai_create(bmsp_matrix_s *A, bmsp_matrix_s *S, int kind, int flags, hipStream_t st)
{
    fsai_create_check_args(kind, flags);
    fsai_check_matrices(A, S, "S");
    std::unique_ptr<bmsp_fsai_s> f(new bmsp_fsai_s());
    f->A = A; f->kind = kind; f->flags = flags;
    const int lay = flags & BMSP_FSAI_COLMAJOR ? 1 : 0;
    if (kind == BMSP_FSAI_SPD) {
        f->G1 = own_matrix(fsai_matrix(A, BMSP_OP_N, S, BMSP_FSAI_SCALE_SQRT, lay, nullptr, st, &f->info1));
        f->info2 = f->info1;
    } else {
        f->G1 = own_matrix(fsai_matrix(A, BMSP_OP_N, S, BMSP_FSAI_SCALE_NONE, lay, nullptr, st, &f->info1));
        f->G2own = own_matrix(fsai_matrix(A, BMSP_OP_T, S, BMSP_FSAI_SCALE_UNIT, lay, nullptr, st, &f->info2));
    }
    if (!(flags & BMSP_FSAI_NO_MATERIALISE)) f->G2t = own_matrix(transpose_matrix(f->G2(), lay, true, st));
    f->work.alloc(dtype_size(A->dtype) * (size_t)(A->num_rows ? A->num_rows : 1));
    build_views(f.get(), st);
    BMSP_HIP(hipStreamSynchronize(st));
    return f.release();
}

void fsai_update(bmsp_fsai_s *f, hipStream_t st)
{
    if (f->kind == BMSP_FSAI_SPD) {
        fsai_values_into(f->A, BMSP_OP_N, f->G1.get(), BMSP_FSAI_SCALE_SQRT, nullptr, st, &f->info1);
        f->info2 = f->info1;
    } else {
        fsai_values_into(f->A, BMSP_OP_N, f->G1.get(), BMSP_FSAI_SCALE_NONE, nullptr, st, &f->info1);
        fsai_values_into(f->A, BMSP_OP_T, f->G2own.get(), BMSP_FSAI_SCALE_UNIT, nullptr, st, &f->info2);
    }
    if (f->G2t) copy_values_from(f->G2(), f->G2t.get(), st);
    build_views(f, st);
    BMSP_HIP(hipStreamSynchronize(st));
}

void fsai_free(bmsp_fsai_s *f)
{
    if (!f) return;
    delete f;  // (as bmsp_mg_free: no synchronisation; the caller lets what it enqueued on the handle finish first)
}

void fsai_get_info(bmsp_fsai_s *f, bmsp_fsai_handle_info *info)
{
    memset(info, 0, sizeof *info);
    info->kind = f->kind; info->flags = f->flags; info->n = f->A->num_rows;
    info->materialised = f->G2t ? 1 : 0;
    info->factor[0] = f->info1; info->factor[1] = f->info2;
    const int64_t es = (int64_t)dtype_size(f->A->dtype);
    int64_t bytes = es * f->A->num_rows;
    for (const bmsp_matrix_s *M : {(const bmsp_matrix_s *)f->G1.get(), (const bmsp_matrix_s *)f->G2own.get(), (const bmsp_matrix_s *)f->G2t.get()})
        if (M) bytes += 8 * (3 * M->block_num + 1) + es * M->nnz;
    info->owned_bytes = bytes;
}

void fsai_factors(bmsp_fsai_s *f, bmsp_matrix_s **G1, bmsp_matrix_s **G2)
{
    if (G1) *G1 = f->G1.get();
    if (G2) *G2 = f->G2();
}

// z = G2^T (G1 r): exactly two public products
void fsai_apply(bmsp_fsai_s *f, const void *r, void *z, hipStream_t st)
{
    if (f->A->num_rows == 0) return;
    spmv_op(f->G1.get(), BMSP_OP_N, 1.0, r, 0.0, f->work, st);
    if (f->G2t) spmv_op(f->G2t.get(), BMSP_OP_N, 1.0, f->work, 0.0, z, st);
    else spmv_op(f->G2(), BMSP_OP_T, 1.0, f->work, 0.0, z, st);
}

SolvePc fsai_solve_pc(bmsp_fsai_s *f, hipStream_t st, bmsp_matrix_s **A)
{
    build_views(f, st);  // (made at create; a bmsp_matrix_invalidate on a lent factor since then has dropped them)
    *A = f->A;
    SolvePc pc;
    pc.hook = [](void *h, const void *in, void *out, const int *, hipStream_t s) { fsai_apply((bmsp_fsai_s *)h, in, out, s); };
    pc.handle = f;
    pc.name = "fsai";
    return pc;
}

}  // namespace bmsp

BMSP_DEFINE_WARM(fsai)
