// ilu0.hip -- the incomplete factorisation ILU(0) by fixed-point sweeps (bmsp_matrix_ilu0 / bmsp_matrix_ilu0_values; Chow and Patel 2015):
// for every stored coordinate (i, j) of A,
//       f_ij^{k+1} = (a_ij - sum over k < min(i, j) with (i, k) and (k, j) stored of f_ik^k * f_kj^k) [ / f_jj^k when i > j ],
// one fused multiply-add per product in ascending k starting from a_ij, one IEEE division in the strict lower triangle, one rounding to
// the storage type.  A sweep is ONE launch over all tiles with no levels: every entry is recomputed from the previous iterate and has
// exactly one writer.  Entry (i, j) holds its final bits after sweep 2 min(i, j) + 1 (+ 1 below the diagonal), so the iteration ends in
// the sequential ILU(0), bit for bit -- what bmsp_spitsv is to bmsp_spsv, this is to a level-scheduled factorisation.
//
// What is reused: the intersection walk of the masked product (walk_pairs.hip.h) with F as both operands -- block-row I of F through its
// block-row pointer, block-column J of F through the cached op-T view of bmsp_spmv_op -- and A as the "mask" whose values start the
// accumulators; the statistics, the stop rule and the read-back protocol of bmsp_spitsv (sweep_stats.hip.h).
//
// What is new:
//   ilu0_sweep_kernel<S, G, STATS>  G lanes per tile (lane_group), a lane owns one byte of the output bitmap at a time, eight accumulators
//       in registers.  Both lists are cut behind K = min(I, J) before the walk (two binary searches), and in the pair with K == min(I, J)
//       the common-index mask is cut to k < min(i, j) for each output position.  The divisor f_jj is read through the diagonal index.
//   DiagIndex   the value index of every (j, j) of F, n entries, and the first row without one: built once per structure of F.
// The iterates ping-pong between F's value array and one temporary kept on F's handle; whichever holds the last one, it ends in F.
#include "walk_pairs.hip.h"
#include "sweep_stats.hip.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace bmsp {
namespace {

constexpr int64_t kMaxIter = 1ll << 20;
// sweeps enqueued between two read-backs (BMSP_ILU0_CHECK): bmsp_spitsv's measured choice
constexpr int64_t kCheckDefault = 8;
// Mean values per tile from which eight lanes are the default: 0, the measured choice of the masked product, whose walk this is.
constexpr int64_t kFillThreshold = 0;

__device__ __forceinline__ float fnma_f(float a, float b, float c) { return __builtin_fmaf(-a, b, c); }
__device__ __forceinline__ double fnma_f(double a, double b, double c) { return __builtin_fma(-a, b, c); }

__device__ __forceinline__ bool same_bits(float a, float b) { return __builtin_bit_cast(uint32_t, a) == __builtin_bit_cast(uint32_t, b); }
__device__ __forceinline__ bool same_bits(double a, double b) { return __builtin_bit_cast(uint64_t, a) == __builtin_bit_cast(uint64_t, b); }
__device__ __forceinline__ bool same_bits(uint16_t a, uint16_t b) { return a == b; }

// what a sweep reads and writes (device pointers).  F's tiles in layout `lay`; A has F's keys and offsets and, when `flip`, the
// transposed bitmaps: a's value of an F position is found through the transposed position.
template <typename S>
struct SweepArgs {
    const uint64_t *keys, *bmps, *offsets;  // F's
    const uint32_t *rowptr;                 // F's block-row pointer
    const uint4 *recs;                      // F's op-T view: records in (block-column, block-row) order
    const uint32_t *colptr;                 //   and its block-column pointer
    const uint32_t *diag;                   // value index of (j, j) in F
    const S *a_vals;
    const S *f_in;
    S *f_out;
    uint64_t nb, n;  // tiles; rows
    int lay, flip;
};

// first record of [lo, hi) whose block-row is above m (the records of a block-column ascend in block-row)
__device__ __forceinline__ uint32_t cut_records(const uint4 *__restrict__ recs, uint32_t lo, uint32_t hi, uint32_t m)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (recs[mid].w <= m) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Byte t of output tile (I, J) of F: positions u = 0 .. 7 with (r, c) = (t, u) for a row-major F, (u, t) for a column-major one; `byte`
// holds the stored ones (bit 7 - u).  acc[u] -= the products of position u over the inner indices k < min(i, j), ascending.  `acc` is
// indexed by unrolled loop counters only: it lives in registers.
template <typename S, typename F>
__device__ __forceinline__ void sweep_byte(const SweepArgs<S> &p, uint32_t I, uint32_t J, uint32_t a_lo, uint32_t a_hi, uint32_t b_lo,
                                           uint32_t b_hi, int t, uint32_t byte, F (&acc)[8])
{
    using D = TileValue<S>;
    const ListA<true> la{p.keys, p.bmps, p.offsets};
    const ListB lb{p.recs};
    const int lay = p.lay;
    const S *__restrict__ fv = p.f_in;
    walk_pairs(la, a_lo, a_hi, lb, b_lo, b_hi, [&](const ListA<true>::Entry &ea, const ListB::Entry &eb) {
        const uint64_t ab = ea.bmp, bb = eb.bmp;
        const uint64_t arm = lay ? tile_transpose(ab) : ab;  // row-major: byte r = row r of F(I, K), bit 7 - k = inner index k
        const uint64_t bcm = lay ? bb : tile_transpose(bb);  // column-major: byte c = column c of F(K, J), bit 7 - k = inner index k
        if ((tile_or_bytes(arm) & tile_or_bytes(bcm)) == 0) return;  // no common inner index
        const S *av = fv + ea.off;
        const S *bv = fv + eb.off;
        const uint32_t fixed = lay ? tile_byte(bcm, t) : tile_byte(arm, t);
        if (fixed == 0) return;
        // inner indices of this pair are 8 K + k: all below min(i, j) when K < min(I, J), else those with k < min(i, j) - 8 K
        const int64_t base = 8 * (int64_t)ea.k;
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (!((byte >> (7 - u)) & 1u)) continue;
            const int r = lay ? u : t, c = lay ? t : u;
            const int64_t i = 8 * (int64_t)I + r, j = 8 * (int64_t)J + c;
            const int64_t room = (i < j ? i : j) - base;  // (>= 0: the lists end at K = min(I, J))
            const uint32_t below = room >= 8 ? 0xffu : (0xff00u >> (int)room) & 0xffu;
            uint32_t common = fixed & (lay ? tile_byte(arm, u) : tile_byte(bcm, u)) & below;
            F d = acc[u];
            while (common) {  // (at most 8 bits)
                const int k = __builtin_clz(common) - 24;
                common &= ~(0x80u >> k);
                const F a = D::load(av[tile_rank(ab, lay ? 8 * k + r : 8 * r + k)]);
                const F b = D::load(bv[tile_rank(bb, lay ? 8 * c + k : 8 * k + c)]);
                d = fnma_f(a, b, d);
            }
            acc[u] = d;
        }
    });
}

// One sweep over F's tiles [0, nb).  prev: the record of the sweep before (null for the first), mine: this sweep's.
template <typename S, int G, bool STATS>
__global__ __launch_bounds__(kThreads) void ilu0_sweep_kernel(SweepArgs<S> p, typename TileValue<S>::F tol, const SweepRecord *prev,
                                                               SweepRecord *mine)
{
#pragma clang fp contract(off)
    using D = TileValue<S>;
    using F = typename D::F;
    using V = TileValue<F>;
    if (STATS && prev && stop_rule<F>(*prev, tol)) return;  // (every lane of the grid reads the same record: all leave or none)
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t tile = gid / G;
    unsigned long long changed = 0, delta = 0, fmax = 0;
    if (tile < p.nb) {
        const uint64_t key = p.keys[tile], fb = p.bmps[tile], off = p.offsets[tile];
        const uint64_t ab = p.flip ? tile_transpose(fb) : fb;  // A's bitmap of the tile
        const uint32_t I = key_row(key), J = key_col(key), m = I < J ? I : J;
        const uint32_t a_lo = p.rowptr[I], a_hi = lower_bound_key(p.keys, a_lo, p.rowptr[I + 1], key_make(I, m) + 1);
        const uint32_t b_lo = p.colptr[J], b_hi = cut_records(p.recs, b_lo, p.colptr[J + 1], m);
        const S *src = p.a_vals + off;
        const S *old = p.f_in + off;
        S *dst = p.f_out + off;
#pragma unroll 1
        for (int s = 0; s < 8 / G; s++) {  // G = 8: lane t takes byte t; G = 1: the non-empty bytes one after another
            const int t = G == 8 ? (int)(gid % G) : s;
            const uint32_t byte = tile_byte(fb, t);
            if (byte == 0) continue;
            F acc[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                acc[u] = 0;
                if ((byte >> (7 - u)) & 1u) acc[u] = D::load(src[tile_rank(ab, p.flip ? tile_transposed_pos(8 * t + u) : 8 * t + u)]);
            }
            sweep_byte<S, F>(p, I, J, a_lo, a_hi, b_lo, b_hi, t, byte, acc);
            int w = tile_rank(fb, 8 * t);
#pragma unroll
            for (int u = 0; u < 8; u++) {
                if (!((byte >> (7 - u)) & 1u)) continue;
                const int r = p.lay ? u : t, c = p.lay ? t : u;
                F v = acc[u];
                const uint64_t col = 8 * (uint64_t)J + c;
                if ((I > J || (I == J && r > c)) && col < p.n) v = v / D::load(p.f_in[p.diag[col]]);
                const S out = D::store(v);
                if (STATS) {
                    const S was = old[w];
                    const F nv = D::load(out), ov = D::load(was);
                    if (!same_bits(out, was)) changed = 1;
                    const unsigned long long d = V::abs_bits(nv - ov), a = V::abs_bits(nv);
                    if (d <= V::kInf && d > delta) delta = d;  // (NaN bits lie above kInf: skipped)
                    if (a <= V::kInf && a > fmax) fmax = a;
                }
                dst[w++] = out;
            }
        }
    }
    if (!STATS) return;
    sweep_publish(changed, delta, fmax, mine);
}

// diag[j] = the value index of (j, j) in F; *missing = the first row whose diagonal entry is not stored (min; ~0: none)
struct DiagIndex {
    const uint64_t *keys, *bmps, *offsets;
    const uint32_t *rowptr;
    uint32_t *diag, *missing;
    __device__ void operator()(uint64_t j) const
    {
        const uint32_t I = (uint32_t)(j >> 3);
        const int pos = 9 * (int)(j & 7);  // (row and column j & 7: the same position in either layout)
        const uint32_t hi = rowptr[I + 1];
        const uint32_t t = lower_bound_key(keys, rowptr[I], hi, key_make(I, I));
        if (t < hi && keys[t] == key_make(I, I) && tile_has(bmps[t], pos)) {
            diag[j] = (uint32_t)(offsets[t] + (uint64_t)tile_rank(bmps[t], pos));
        } else {
            diag[j] = 0;
            atomicMin(missing, (uint32_t)j);
        }
    }
};

// ---- host ------------------------------------------------------------------------------------------------------------------------------
bool no_check(double tol) { return tol == BMSP_ILU_NO_CHECK; }

const char *dtype_name(bmsp_dtype t) { return t == BMSP_F16 ? "F16" : (t == BMSP_F32 ? "F32" : "F64"); }

// F's block-row pointer, op-T view, diagonal index and second iterate buffer, made on first use (the view and the index synchronise
// `st`); refuses a matrix with a row whose diagonal entry is not stored
const bmsp_spmv_op_view &ensure_buffers(bmsp_matrix_s *F, hipStream_t st)
{
    ensure_rowptr(F, st);
    const bmsp_spmv_op_view &w = spmv_op_ensure_view(F, BMSP_OP_T, st);
    if (F->ilu0_missing_row == -2) {
        const uint64_t n = (uint64_t)F->num_rows;
        DevBuf<uint32_t> diag((size_t)n), missing(1);
        BMSP_HIP(hipMemsetAsync(missing.p, 0xff, 4, st));
        device_for_each(DiagIndex{F->keys, F->bmps, F->offsets, F->rowptr, diag.p, missing.p}, n, st);
        BMSP_HIP(hipStreamSynchronize(st));
        uint32_t first = ~0u;
        copy_d2h_staged(&first, missing.p, 4);
        F->ilu0_diag = std::move(diag);
        F->ilu0_missing_row = first == ~0u ? -1 : (int64_t)first;
    }
    if (F->ilu0_missing_row >= 0)
        fail(BMSP_ERR_INVALID, "matrix A: row %lld of A has no stored diagonal entry", (long long)F->ilu0_missing_row);
    if (!F->ilu0_tmp) F->ilu0_tmp.alloc(dtype_size(F->dtype) * (size_t)F->nnz);
    return w;
}

template <typename S, bool STATS>
void launch_sweep(int lanes, const SweepArgs<S> &p, double tol, const SweepRecord *prev, SweepRecord *mine, hipStream_t st)
{
    using F = typename TileValue<S>::F;
    launch_lane_group(lanes, p.nb, [&](auto g, dim3 grid) {
        hipLaunchKernelGGL((ilu0_sweep_kernel<S, decltype(g)::value, STATS>), grid, dim3(kThreads), 0, st, p, (F)tol, prev, mine);
    });
}

void empty_info(bmsp_ilu0_info *info, bool stats, int64_t cap)
{
    if (!info) return;
    memset(info, 0, sizeof *info);
    info->max_sweeps = cap;
    info->converged = stats ? 1 : 0;
    info->delta = info->fmax = stats ? 0.0 : -1.0;
    snprintf(info->kernel, sizeof info->kernel, "none (empty matrix)");
}

// The sweeps on F from the iterate `f0` (F's own value array, or A's when the layouts agree): checks done, F's value caches dropped.
void run_sweeps(const bmsp_matrix_s *A, bmsp_matrix_s *F, const void *f0, int64_t max_iter, double tol, double *delta_history,
                bmsp_ilu0_info *info, hipStream_t st)
{
    const bool stats = !no_check(tol), f64 = F->dtype == BMSP_F64;
    const int64_t m = max_iter ? max_iter : 2 * (int64_t)F->num_rows;
    const bmsp_spmv_op_view &w = ensure_buffers(F, st);
    const int lanes = lane_group(F->nnz, F->block_num, "BMSP_ILU0_LANES", kFillThreshold);
    if (info) {
        empty_info(info, stats, m);
        info->lanes = lanes;
        info->view_bytes = (int64_t)w.bytes + 4 * (int64_t)F->num_rows;
        snprintf(info->kernel, sizeof info->kernel, "ilu0_sweep_kernel<%s, %d, %s>", dtype_name(F->dtype), lanes, stats ? "STATS" : "NO_STATS");
    }
    const size_t bytes = dtype_size(F->dtype) * (size_t)F->nnz;
    // f^0 = f0; f^j, j >= 1, lives in odd(j) ? odd : even.  A given f^0 in F's array fixes even = F's array; otherwise the pair is chosen
    // so that a known number of sweeps ends in F's array, and a checked call's first sweep does.
    void *odd = F->values, *even = F->ilu0_tmp;
    if (f0 == F->values || (!stats && !(m & 1))) {
        odd = F->ilu0_tmp;
        even = F->values;
    }
    const auto iterate = [&](int64_t j) -> const void * { return j == 0 ? f0 : (j & 1 ? odd : even); };
    const auto sweep = [&](int64_t k, const SweepRecord *prev, SweepRecord *mine) {
        dispatch_dtype(F->dtype, [&](auto s) {
            using S = decltype(s);
            SweepArgs<S> p;
            p.keys = F->keys; p.bmps = F->bmps; p.offsets = F->offsets; p.rowptr = F->rowptr;
            p.recs = (const uint4 *)w.mem;
            p.colptr = (const uint32_t *)((const char *)w.mem + w.off_ptr);
            p.diag = F->ilu0_diag;
            p.a_vals = (const S *)A->values;
            p.f_in = (const S *)iterate(k);
            p.f_out = (S *)(k & 1 ? even : odd);
            p.nb = (uint64_t)F->block_num; p.n = (uint64_t)F->num_rows;
            p.lay = F->transposed; p.flip = A->transposed != F->transposed;
            if (stats) launch_sweep<S, true>(lanes, p, tol, prev, mine, st);
            else launch_sweep<S, false>(lanes, p, tol, prev, mine, st);
        });
    };
    int64_t sweeps = m;
    if (!stats) {
        for (int64_t k = 0; k < m; k++) sweep(k, nullptr, nullptr);
    } else {
        const int64_t check = sweep_check_from_env("BMSP_ILU0_CHECK", kCheckDefault);
        // (m may be 2 n: the records live per batch, not per call.)  Slot 0 holds the last record of the batch before, slot 1 + q the
        // record of the batch's sweep q.
        const int64_t cap = check < m ? check : m;
        DevBuf<SweepRecord> recs((size_t)cap + 1);
        std::vector<SweepRecord> host;
        bool converged = false;
        for (int64_t done = 0, last = 0; done < m && !converged; last = cap) {
            const int64_t batch = check < m - done ? check : m - done;
            if (done) BMSP_HIP(hipMemcpyAsync(recs.p, recs.p + last, sizeof(SweepRecord), hipMemcpyDeviceToDevice, st));
            BMSP_HIP(hipMemsetAsync(recs.p + 1, 0, sizeof(SweepRecord) * (size_t)batch, st));
            for (int64_t q = 0; q < batch; q++) sweep(done + q, done + q ? recs.p + q : nullptr, recs.p + q + 1);
            BMSP_HIP(hipStreamSynchronize(st));
            host.resize((size_t)(done + batch));
            copy_d2h_staged(host.data() + done, recs.p + 1, sizeof(SweepRecord) * (size_t)batch);
            for (int64_t k = done; k < done + batch && !converged; k++) {
                const SweepRecord &r = host[(size_t)k];
                if (f64 ? stop_rule<double>(r, tol) : stop_rule<float>(r, (float)tol)) {
                    converged = true;
                    sweeps = k + 1;  // (the sweeps enqueued behind it returned at once and wrote nothing)
                }
            }
            done += batch;
        }
        const auto widen = [&](unsigned long long u) { return f64 ? VecBits<double>::from(u) : (double)VecBits<float>::from(u); };
        if (delta_history)
            for (int64_t k = 0; k < sweeps; k++) delta_history[k] = widen(host[(size_t)k].delta);
        if (info) {
            info->converged = converged ? 1 : 0;
            info->delta = widen(host[(size_t)sweeps - 1].delta);
            info->fmax = widen(host[(size_t)sweeps - 1].xmax);
        }
    }
    if (info) info->sweeps = sweeps;
    if (iterate(sweeps) != F->values) BMSP_HIP(hipMemcpyAsync(F->values, iterate(sweeps), bytes, hipMemcpyDeviceToDevice, st));
}

bool is_empty(const bmsp_matrix_s *A) { return A->num_rows == 0 || A->block_num == 0 || A->nnz == 0; }

}  // namespace

void ilu0_check_args(int64_t max_iter, double tol, const double *delta_history)
{
    if (max_iter < 0 || max_iter > kMaxIter) fail(BMSP_ERR_INVALID, "max_iter must be 0 (2 n) or 1 .. 2^20 (got %lld)", (long long)max_iter);
    if (std::isnan(tol) || (tol < 0.0 && !no_check(tol)))
        fail(BMSP_ERR_INVALID, "tol must be >= 0 or BMSP_ILU_NO_CHECK (-1.0) (got %g)", tol);
    if (no_check(tol) && delta_history) fail(BMSP_ERR_INVALID, "delta_history must be NULL under BMSP_ILU_NO_CHECK: nothing is read back");
}

void ilu0_check_flags(int flags)
{
    if (flags & ~BMSP_ILU_F0_GIVEN) fail(BMSP_ERR_INVALID, "flags: unknown bits (got %d; BMSP_ILU_F0_GIVEN = 1 is the only one)", flags);
}

// the refusals that need the handles, before any device call; F: null for the call that makes its own
void ilu0_check_matrices(const bmsp_matrix_s *A, const bmsp_matrix_s *F)
{
    if (A->num_rows != A->num_cols) fail(BMSP_ERR_INVALID, "ilu0: matrix A must be square (it is %d x %d)", A->num_rows, A->num_cols);
    refuse_view(A, "ilu0: matrix A");
    if (A->block_num >= (1ll << 32) || A->nnz >= (1ll << 32)) fail(BMSP_ERR_LIMIT, "ilu0: matrix A: 2^32 tiles or values or more");
    if (!F) return;
    if (F == A) fail(BMSP_ERR_INVALID, "ilu0_values: matrix F is A: a is read in every sweep");
    // a transpose's output has the source's uid too, but its own tile order (tp_map)
    if (!F->tp_src_uid || F->tp_src_uid != A->uid || F->tp_map)
        fail(BMSP_ERR_INVALID, "ilu0_values: matrix F was not made from A by bmsp_matrix_ilu0, bmsp_matrix_convert_layout, bmsp_matrix_scale, "
                               "bmsp_sddmm or bmsp_spgemm_masked, or A's structure changed since");
    if (A->block_num != F->block_num || A->nnz != F->nnz || A->dtype != F->dtype || A->num_rows != F->num_rows || A->num_cols != F->num_cols)
        fail(BMSP_ERR_INVALID, "ilu0_values: matrix F: A's and F's sizes or dtypes differ");
    refuse_view(F, "ilu0_values: matrix F");
}

bmsp_matrix_s *ilu0_matrix(bmsp_matrix_s *A, int64_t max_iter, double tol, int out_transposed, hipStream_t st, double *delta_history,
                           bmsp_ilu0_info *info)
{
    ilu0_check_args(max_iter, tol, delta_history);
    check_layout_flag(out_transposed, "out_transposed");
    ilu0_check_matrices(A, nullptr);
    // A's structure and values in the layout asked for: the structure of a layout conversion, and f^0
    MatrixPtr F = own_matrix(transpose_matrix(A, out_transposed, false, st));
    if (is_empty(A)) empty_info(info, !no_check(tol), max_iter ? max_iter : 2 * (int64_t)A->num_rows);
    else run_sweeps(A, F.get(), F->values, max_iter, tol, delta_history, info, st);
    return F.release();
}

void ilu0_values_into(bmsp_matrix_s *A, bmsp_matrix_s *F, int64_t max_iter, double tol, int flags, hipStream_t st, double *delta_history,
                      bmsp_ilu0_info *info)
{
    ilu0_check_args(max_iter, tol, delta_history);
    ilu0_check_flags(flags);
    ilu0_check_matrices(A, F);
    if (is_empty(A)) {
        empty_info(info, !no_check(tol), max_iter ? max_iter : 2 * (int64_t)A->num_rows);
        return;
    }
    ensure_buffers(F, st);  // (a missing diagonal is refused before anything of F is written)
    drop_value_caches(F);
    const void *f0 = F->values;
    if (!(flags & BMSP_ILU_F0_GIVEN)) {
        // f^0 = A's values: read in place when the layouts agree, else gathered into F's array (bmsp_matrix_copy_values' pass)
        if (A->transposed == F->transposed) f0 = A->values;
        else copy_values_from(A, F, st);
    }
    run_sweeps(A, F, f0, max_iter, tol, delta_history, info, st);
}

}  // namespace bmsp

BMSP_DEFINE_WARM(ilu0)
