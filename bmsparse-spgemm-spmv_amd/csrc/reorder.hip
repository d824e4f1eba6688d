// reorder.hip -- a block multi-colour ordering and the block permutations that apply it (bmsp_matrix_color_blocks /
// bmsp_matrix_permute_blocks / bmsp_vec_permute_blocks), without going back through scalar COO entries.
//
// What the format gives: the level rule of bmsp_spsv counts tiles and ignores bitmaps, so a proper colouring of the block-row graph with
// every colour class made contiguous is a matrix whose triangles have as many levels as there are colours.  A permutation of block-rows
// and block-columns moves whole tiles: bitmaps and value segments stay, only the keys change -- transpose.hip's passes (rewrite keys, stable
// radix sort with the source tile as payload, one scan for bitmaps and offsets, move_values through the tile map) with another key.
//
// Colouring (Jones-Plassmann on hashed priorities): key(I) = (splitmix64(seed ^ I), I); color(I) = the smallest colour no neighbour of a
// greater key holds -- the sequential greedy colouring in descending key order, a pure function of structure and seed.  The neighbours
// of I are the block columns of block-row I (A's keys and block-row pointer) and the block-rows of block-column I (the cached op-T view of
// bmsp_spmv_op: its pointer and the other-index word of its records); A + A^T is never formed.
//   color_round_kernel   ONE launch per round, eight lanes per block-row.  A block-row is coloured in round k iff every neighbour of a
//       greater key carries a round stamp in [1, k): a stamp written in this launch reads as 0 or k, both "uncoloured", and a colour is
//       read only next to a stamp of an earlier launch.  Nothing waits between workgroups: no flag, no spin, no cooperative launch.  The
//       smallest free colour is found in windows of 64: the lanes OR a 64-bit mask of the colours in [base, base + 64) over the
//       neighbours, the first zero bit wins, a full mask moves the window.
//   termination   every round leaves a record {block-rows still uncoloured, 1 + the largest colour it gave}, built by integer atomics
//       (one add and at most one max per workgroup).  Round k + 1 begins by reading record k and returns when nothing is left; the host
//       enqueues BMSP_COLOR_CHECK rounds, reads their records back and stops at the first zero (bmsp_spitsv's protocol).  Every round
//       colours at least the greatest remaining key, so there are at most `blocks` rounds.
// Ordering: block-rows sorted by (class, index) by the stable radix sort on the class bits alone.
#include "tile_pass.hip.h"
#include "sweep_stats.hip.h"
#include <cstring>
#include <vector>

namespace bmsp {
namespace {

constexpr int64_t kColorCheckDefault = 16;  // rounds enqueued between two read-backs (BMSP_COLOR_CHECK)
constexpr uint32_t kNone = ~0u;

// the finaliser of pybmsp/gen.py
__device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// {block-rows still uncoloured after the round, 1 + the largest colour the round gave}; all zero = the round did not run
struct RoundRecord {
    uint32_t pending, top;
};

struct FirstRecord {
    RoundRecord *rec;
    uint32_t blocks;
    __device__ void operator()(uint64_t) const { rec[0] = RoundRecord{blocks, 0u}; }
};

// Round k over block-rows [0, nb).  stamp[I]: the round that coloured I, 0 = uncoloured; neither stamp nor colors is read through a
// read-only path: both are written in this launch.
__global__ __launch_bounds__(kThreads) void color_round_kernel(const uint32_t *__restrict__ rowptr, const uint64_t *__restrict__ keys,
                                                               const uint32_t *__restrict__ colptr, const uint4 *__restrict__ crecs,
                                                               uint32_t nb, uint64_t seed, uint32_t k, uint32_t *stamp, uint32_t *colors,
                                                               const RoundRecord *prev, RoundRecord *mine)
{
    if (prev->pending == 0) return;  // (every lane of the grid reads the same record of an earlier launch: all leave or none)
    const uint64_t g = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) >> 3;
    const uint32_t t = threadIdx.x & 7u;
    uint32_t pending = 0, top = 0;
    if (g < nb && stamp[g] == 0) {  // (whole groups: only the group itself writes its stamp, at its end)
        const uint32_t I = (uint32_t)g;
        const uint64_t hI = splitmix64(seed ^ (uint64_t)I);
        const uint32_t r0 = rowptr[I], nr = rowptr[I + 1] - r0, c0 = colptr[I], total = nr + (colptr[I + 1] - c0);
        for (uint32_t base = 0;; base += 64) {
            uint64_t mask = 0;
            uint32_t blocked = 0;
            for (uint32_t e = t; e < total; e += 8) {
                const uint32_t J = e < nr ? key_col(keys[r0 + e]) : crecs[c0 + (e - nr)].w;
                if (J == I || J >= nb) continue;
                const uint64_t hJ = splitmix64(seed ^ (uint64_t)J);
                if (hJ < hI || (hJ == hI && J < I)) continue;  // a smaller key: I does not wait for it
                const uint32_t s = stamp[J];
                if (s == 0 || s >= k) {
                    blocked = 1;
                    break;
                }
                const uint32_t c = colors[J] - base;  // (below the window: wraps beyond 64)
                if (c < 64) mask |= 1ull << c;
            }
#pragma unroll
            for (int d = 1; d < 8; d <<= 1) {  // (the group is here as a whole: the loop above ends for every lane)
                mask |= __shfl_xor(mask, d, 8);
                blocked |= __shfl_xor(blocked, d, 8);
            }
            if (blocked) {
                pending = t == 0 ? 1u : 0u;
                break;
            }
            if (~mask) {
                const uint32_t c = base + (uint32_t)__builtin_ctzll(~mask);
                if (t == 0) {
                    colors[I] = c;
                    stamp[I] = k;
                }
                top = c + 1;
                break;
            }
        }
    }
    // the workgroup's count and maximum: registers across the wave, LDS across the four waves, then ONE lane issues the atomics
    pending = wave_sum(pending);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = __shfl_xor(top, d, kWave);
        top = o > top ? o : top;
    }
    __shared__ uint32_t part[2][kThreads / kWave];
    if (lane_id() == 0) {
        part[0][wave_id()] = pending;
        part[1][wave_id()] = top;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t p = 0, m = 0;
#pragma unroll
        for (int w = 0; w < kThreads / kWave; w++) {
            p += part[0][w];
            m = part[1][w] > m ? part[1][w] : m;
        }
        if (p) atomicAdd(&mine->pending, p);
        if (m > __hip_atomic_load(&mine->top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&mine->top, m);
    }
}

// sort key of block-row I: its class's place in the ordering.  Classes ascend by colour; with a trailing partial block-row (last != kNone)
// that block-row's class goes last, and being the largest index it is last within it.
struct ClassKey {
    const uint32_t *colors;
    uint32_t last, n_colors;
    uint64_t *key;
    uint32_t *idx;
    __device__ void operator()(uint64_t I) const
    {
        uint32_t c = colors[I];
        if (last != kNone) {
            const uint32_t cl = colors[last];
            c = c < cl ? c : (c == cl ? n_colors - 1 : c - 1);
        }
        key[I] = c;
        idx[I] = (uint32_t)I;
    }
};

// ---- permutation -----------------------------------------------------------------------------------------------------------------------
// inv[perm[i]] = i for the entries in range (inv starts as all kNone: what stays kNone was hit by no entry)
struct ScatterInverse {
    const uint32_t *perm;
    uint32_t m;
    uint32_t *inv;
    __device__ void operator()(uint64_t i) const
    {
        const uint32_t p = perm[i];
        if (p < m) inv[p] = (uint32_t)i;
    }
};

// *bad += the indices of [0, m) no entry of perm hit (an entry out of range or a duplicate leaves one), + 1 when the last block must map to
// itself (partial) and does not
__global__ __launch_bounds__(kThreads) void perm_check_kernel(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ inv, uint32_t m,
                                                              int partial, uint32_t *bad)
{
    const uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    uint32_t b = 0;
    if (p < m) {
        b = inv[p] == kNone ? 1u : 0u;
        if (partial && p == m - 1 && perm[p] != m - 1) b++;
    }
    b = wave_sum(b);
    if (lane_id() == 0 && b) atomicAdd(bad, b);
}

// tile i under its new key (row' with row_perm[row'] = row, col' likewise; null = unchanged) and its index as the payload
struct PermutedKey {
    const uint64_t *keys;
    const uint32_t *inv_r, *inv_c;
    uint64_t *sk;
    uint32_t *idx;
    __device__ void operator()(uint64_t i) const
    {
        const uint64_t k = keys[i];
        const uint32_t r = key_row(k), c = key_col(k);
        sk[i] = key_make(inv_r ? inv_r[r] : r, inv_c ? inv_c[c] : c);
        idx[i] = (uint32_t)i;
    }
};

// the inverse of a permutation of [0, m) into inv, and its check into *bad
void invert_and_check(const uint32_t *perm, uint32_t m, bool partial, uint32_t *inv, uint32_t *bad, hipStream_t st)
{
    if (m == 0) return;
    BMSP_HIP(hipMemsetAsync(inv, 0xff, 4 * (size_t)m, st));
    device_for_each(ScatterInverse{perm, m, inv}, m, st);
    hipLaunchKernelGGL(perm_check_kernel, grid_for(m), dim3(kThreads), 0, st, perm, (const uint32_t *)inv, m, partial ? 1 : 0, bad);
    BMSP_CHECK_LAUNCH();
}

// element e = 8 i + r of the permuted side and element 8 perm[i] + r of the other, both below n
template <typename R>
__global__ __launch_bounds__(kThreads) void vec_permute_kernel(const uint32_t *__restrict__ perm, const R *__restrict__ x, R *__restrict__ y,
                                                               int64_t n, uint32_t blocks, int inverse)
{
    const uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t i = e >> 3;
    if (i >= blocks) return;
    const uint32_t p = perm[i];
    if (p >= blocks) return;  // (an entry out of range moves nothing)
    const int64_t a = (int64_t)e, b = (int64_t)p * 8 + (int64_t)(e & 7);
    if (a >= n || b >= n) return;
    if (inverse) y[b] = x[a];
    else y[a] = x[b];
}

}  // namespace

void color_check_matrix(const bmsp_matrix_s *A)
{
    if (A->num_rows != A->num_cols) fail(BMSP_ERR_INVALID, "color_blocks: matrix A must be square (it is %d x %d)", A->num_rows, A->num_cols);
    spmv_op_check_matrix(A, "color_blocks");
}

void color_blocks(bmsp_matrix_s *A, uint64_t seed, uint32_t *d_colors, uint32_t *d_perm, hipStream_t st, bmsp_color_info *info)
{
    color_check_matrix(A);
    const int64_t nb = A->num_block_rows();
    if (info) {
        memset(info, 0, sizeof *info);
        info->blocks = nb;
        snprintf(info->kernel, sizeof info->kernel, "none (empty matrix)");
    }
    if (nb == 0) return;
    ensure_rowptr(A, st);
    const bmsp_spmv_op_view &w = spmv_op_ensure_view(A, BMSP_OP_T, st);
    const uint4 *crecs = (const uint4 *)w.mem;
    const uint32_t *colptr = (const uint32_t *)((const char *)w.mem + w.off_ptr);
    DevBuf<uint32_t> stamp((size_t)nb);
    DevBuf<RoundRecord> recs((size_t)nb + 1);
    std::vector<RoundRecord> host((size_t)nb + 1);
    BMSP_HIP(hipMemsetAsync(stamp.p, 0, 4 * (size_t)nb, st));
    BMSP_HIP(hipMemsetAsync(recs.p, 0, sizeof(RoundRecord) * ((size_t)nb + 1), st));
    device_for_each(FirstRecord{recs.p, (uint32_t)nb}, 1, st);
    const int64_t check = sweep_check_from_env("BMSP_COLOR_CHECK", kColorCheckDefault);
    int64_t rounds = 0, colors = 0;
    // at most nb rounds: each colours at least the greatest remaining key
    for (int64_t done = 0; done < nb && !rounds;) {
        const int64_t batch = check < nb - done ? check : nb - done;
        for (int64_t k = done + 1; k <= done + batch; k++) {
            hipLaunchKernelGGL(color_round_kernel, grid_for((uint64_t)nb * 8), dim3(kThreads), 0, st, (const uint32_t *)A->rowptr,
                               (const uint64_t *)A->keys, colptr, crecs, (uint32_t)nb, seed, (uint32_t)k, stamp.p, d_colors,
                               (const RoundRecord *)(recs.p + k - 1), recs.p + k);
            BMSP_CHECK_LAUNCH();
        }
        BMSP_HIP(hipStreamSynchronize(st));
        copy_d2h_staged(host.data() + done + 1, recs.p + done + 1, sizeof(RoundRecord) * (size_t)batch);
        for (int64_t k = done + 1; k <= done + batch; k++) {
            if ((int64_t)host[(size_t)k].top > colors) colors = (int64_t)host[(size_t)k].top;
            if (host[(size_t)k].pending == 0) {  // (the rounds enqueued behind it returned at once and wrote nothing)
                rounds = k;
                break;
            }
        }
        done += batch;
    }
    if (!rounds) fail(BMSP_ERR_INTERNAL, "color_blocks: %lld rounds left block-rows uncoloured", (long long)nb);
    if (info) {
        info->colors = colors;
        info->rounds = rounds;
        info->view_bytes = (int64_t)w.bytes;
        snprintf(info->kernel, sizeof info->kernel, "color_round_kernel<8 lanes>");
    }
    if (!d_perm) return;
    const bool partial = (A->num_rows & 7) != 0;
    DevBuf<uint64_t> k0((size_t)nb), k1((size_t)nb);
    DevBuf<uint32_t> p0((size_t)nb), p1((size_t)nb);
    device_for_each(ClassKey{d_colors, partial ? (uint32_t)(nb - 1) : kNone, (uint32_t)colors, k0.p, p0.p}, (uint64_t)nb, st);
    PingPong<uint64_t> kk{k0.p, k1.p};
    PingPong<uint32_t> pp{p0.p, p1.p};
    device_radix_sort_pairs<uint32_t>(kk, pp, (uint64_t)nb, 0, ceil_log2_u64((uint64_t)colors), st);
    BMSP_HIP(hipMemcpyAsync(d_perm, pp.cur, 4 * (size_t)nb, hipMemcpyDeviceToDevice, st));
    BMSP_HIP(hipStreamSynchronize(st));  // the sort temporaries go back to the pool
}

void permute_check_matrix(const bmsp_matrix_s *A)
{
    refuse_view(A, "permute_blocks");
    if (A->nnz >= (1ll << 32)) fail(BMSP_ERR_LIMIT, "nnz %lld exceeds the 32-bit element range", (long long)A->nnz);
    if (A->block_num >= (1ll << 32)) fail(BMSP_ERR_LIMIT, "more than 2^32 blocks");
}

// out = P * A * Q^T at tile granularity: block (I', J') of out is block (row_perm[I'], col_perm[J']) of A
bmsp_matrix_s *permute_blocks(bmsp_matrix_s *A, const uint32_t *d_row_perm, const uint32_t *d_col_perm, int out_transposed, hipStream_t st)
{
    check_layout_flag(out_transposed, "out_transposed");
    permute_check_matrix(A);
    const uint64_t nb = (uint64_t)A->block_num;
    const uint32_t nbr = (uint32_t)A->num_block_rows(), nbc = (uint32_t)A->num_block_cols();
    // 1. the inverses, and with them the check: nothing below indexes by an entry that was not checked
    DevBuf<uint32_t> inv_r, inv_c, bad(2);
    if (d_row_perm || d_col_perm) {
        BMSP_HIP(hipMemsetAsync(bad.p, 0, 8, st));
        if (d_row_perm) {
            inv_r.alloc(nbr);
            invert_and_check(d_row_perm, nbr, (A->num_rows & 7) != 0, inv_r.p, bad.p, st);
        }
        if (d_col_perm) {
            inv_c.alloc(nbc);
            invert_and_check(d_col_perm, nbc, (A->num_cols & 7) != 0, inv_c.p, bad.p + 1, st);
        }
        uint32_t h[2] = {0u, 0u};
        read_back_bytes(h, bad.p, 8, st);
        if (h[0])
            fail(BMSP_ERR_INVALID, "d_row_perm is not a permutation of [0, %u) that keeps a trailing partial block in place", nbr);
        if (h[1])
            fail(BMSP_ERR_INVALID, "d_col_perm is not a permutation of [0, %u) that keeps a trailing partial block in place", nbc);
    }
    auto m = make_matrix();
    m->num_rows = A->num_rows; m->num_cols = A->num_cols;
    m->nnz = A->nnz; m->block_num = A->block_num; m->dtype = A->dtype; m->transposed = out_transposed;
    m->tp_src_uid = A->uid;
    m->tp_permute = out_transposed != A->transposed ? 1 : 0;  // the other layout: every tile transposed in place
    TileSort ts;  // sort temporaries: go back to the pool after the synchronisation at the end
    if (d_row_perm || d_col_perm) {
        // 2. / 3. the new keys, sorted.  The input is in (row, col) order: new rows alone need the row bits only (a stable sort keeps the
        // columns of a row ascending); new columns need both halves
        ts.k0.alloc(nb); ts.k1.alloc(nb); ts.p0.alloc(nb); ts.p1.alloc(nb);
        device_for_each(PermutedKey{A->keys, d_row_perm ? inv_r.p : nullptr, d_col_perm ? inv_c.p : nullptr, ts.k0.p, ts.p0.p}, nb, st);
        PingPong<uint64_t> kk{ts.k0.p, ts.k1.p};
        PingPong<uint32_t> pp{ts.p0.p, ts.p1.p};
        if (d_col_perm) device_radix_sort_pairs<uint32_t>(kk, pp, nb, 0, ceil_log2_u64((uint64_t)nbc), st);
        device_radix_sort_pairs<uint32_t>(kk, pp, nb, 32, 32 + ceil_log2_u64((uint64_t)nbr), st);
        ts.keys = kk.cur; ts.map = pp.cur;
        m->keys = ts.take_keys();
        m->tp_map = ts.take_map();
    }
    // 4. / 5. bitmaps and offsets in one scan, the values through the tile map
    finish_moved_tiles(A, m.get(), st);
    return m.release();
}

void vec_permute_check_args(int64_t n, int vec_f64, const void *d_perm, int inverse, const void *d_x, const void *d_y)
{
    vec_check_args(n, vec_f64);
    if (inverse != 0 && inverse != 1) fail(BMSP_ERR_INVALID, "inverse must be 0 or 1 (got %d)", inverse);
    if (n == 0) return;
    if (!d_perm) fail(BMSP_ERR_INVALID, "d_perm is null");
    if (!d_x) fail(BMSP_ERR_INVALID, "d_x is null");
    if (!d_y) fail(BMSP_ERR_INVALID, "d_y is null");
    if (d_x == d_y) fail(BMSP_ERR_INVALID, "d_y must not be d_x: a block permutation is not done in place");
}

void vec_permute_blocks(int64_t n, int vec_f64, const uint32_t *d_perm, int inverse, const void *d_x, void *d_y, hipStream_t st)
{
    vec_permute_check_args(n, vec_f64, d_perm, inverse, d_x, d_y);
    if (n == 0) return;
    const int64_t blocks = ceil_div(n, 8);
    if (blocks >= (1ll << 32)) fail(BMSP_ERR_LIMIT, "vec_permute_blocks: 2^32 blocks or more");
    if (vec_f64)
        hipLaunchKernelGGL(vec_permute_kernel<double>, grid_for((uint64_t)blocks * 8), dim3(kThreads), 0, st, d_perm, (const double *)d_x,
                           (double *)d_y, n, (uint32_t)blocks, inverse);
    else
        hipLaunchKernelGGL(vec_permute_kernel<float>, grid_for((uint64_t)blocks * 8), dim3(kThreads), 0, st, d_perm, (const float *)d_x,
                           (float *)d_y, n, (uint32_t)blocks, inverse);
    BMSP_CHECK_LAUNCH();
}

}  // namespace bmsp

BMSP_DEFINE_WARM(reorder)
