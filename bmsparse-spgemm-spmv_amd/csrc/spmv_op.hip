// spmv_op.hip -- u = alpha * op(A) * v + beta * u for op in {N, T} and either tile layout (bmsp_spmv_op), without materialising A^T or a
// second layout.
//
// What the format gives (transpose.hip): a tile stored in layout L is, bit for bit, the tile of A^T in the other layout.  So a product
// with op(A) needs no new tiles, only (a) the tiles in the order of the OUTPUT blocks -- A's own order for N, (block-column, block-row)
// order for T, from transpose_matrix's stable radix sort on the block-column bits (sort_tiles_by_block_column) -- and (b) a lane
// mapping per (op, layout):
//   MINOR = false  the output index inside the block is the BYTE index of the bitmap: (T, layout 1) (and (N, layout 0), which is
//                  bmsp_spmv's case and goes to bmsp_spmv).  Lane j takes byte j: its values are contiguous from tile_rank(bmp, 8j).
//   MINOR = true   the output index is the BIT index inside each byte: (T, layout 0) and (N, layout 1).  Lane j takes positions 8i + j.
//
// The view (bmsp_spmv_op_view, matrix.h; one per op, structure only) holds the tiles as 16-byte records in sweep order and the work items:
// an output block, or a range of at most SPLIT tiles of one (a hub block-column of a power-law matrix would otherwise be one walker's).
// Every output has ONE writer and every sum a fixed order, so there is no atomic anywhere: a whole-block item applies the epilogue and
// stores u; the items of a split block store their 8 partial sums to their own scratch slot and the fold kernel adds a block's slots in
// item order.  The result is a pure function of A's arrays, v and the two switches.
//
// Kernels:
//   sweep<S, MINOR, SLOTS>  SLOTS = 1: eight lanes walk an item's tiles one after another (32 items per workgroup).  SLOTS = 8: a wave
//                           takes an item, eight tiles per step, one per lane group (the 16-byte record loads of a step are one 128-byte
//                           request); the eight slot sums meet in a fixed xor tree of wave shuffles.
//   fold<R>                 eight lanes per split block.
//   epilogue<R>             (N, layout 0) with alpha != 1 or beta != 0: bmsp_spmv's sum, scaled into u.
#include "tile_pass.hip.h"
#include <cstring>
#include <vector>

namespace bmsp {
namespace {

constexpr uint32_t kWhole = ~0u;  // an item's scratch slot when it is a whole output block
// Both measured (tools/spmv_op_bench.py; DESIGN §4 "SpMV with op(A)"): 64 tiles per item is the fastest or within 10 % of it on every
// matrix timed (a hub block's item is a chain of dependent loads: 256 took 1.7x on R-MAT 2^16 x 8, no split 16x; 16 took 1.3 - 1.9x: more
// items, and a fold of more parts); banded fp32 matrices of 3 / 5 tiles per output block run faster with SLOTS = 1, of 7 / 9 with SLOTS = 8
constexpr int64_t kSplitDefault = 64;  // tiles per item (BMSP_SPMV_OP_SPLIT)
constexpr int64_t kSlotsTiles = 6;     // SLOTS = 8 from this mean number of tiles per output block (BMSP_SPMV_OP_SLOTS)

template <typename S, bool MINOR, int SLOTS>
__global__ __launch_bounds__(kThreads) void spmv_op_sweep_kernel(const uint4 *__restrict__ recs, const uint4 *__restrict__ items,
                                                                 uint64_t n_items, const S *__restrict__ vals, const S *__restrict__ v,
                                                                 typename TileValue<S>::R alpha, typename TileValue<S>::R beta,
                                                                 typename TileValue<S>::R *u, typename TileValue<S>::R *__restrict__ scratch,
                                                                 int64_t out_len)
{
    using D = TileValue<S>;
    using F = typename D::F;
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t item = SLOTS == 8 ? gid >> 6 : gid >> 3;
    const int j = (int)(threadIdx.x & 7);
    const int g = SLOTS == 8 ? lane_id() >> 3 : 0;
    const bool live = item < n_items;
    uint4 it = make_uint4(0u, 0u, 0u, kWhole);  // {output block, first tile, end tile, scratch slot}
    if (live) it = items[item];
    F acc = 0;
    for (uint64_t t = (uint64_t)it.y + g; t < it.z; t += SLOTS) {
        const uint4 r = recs[t];
        const uint64_t bmp = (uint64_t)r.y << 32 | r.x;
        const S *tv = vals + r.z;
        const S *tx = v + (uint64_t)r.w * 8;  // only stored entries index it: never beyond the matrix
        if (!MINOR) {
            uint32_t byte = tile_byte(bmp, j);
            int k = tile_rank(bmp, 8 * j);
            while (byte) {
                const int c = __builtin_clz(byte) - 24;
                byte &= ~(0x80u >> c);
                acc += D::load(tv[k++]) * D::load(tx[c]);
            }
        } else {
            uint64_t m = bmp & (0x8080808080808080ull >> j);  // positions 8i + j
            while (m) {
                const int p = tile_pop_first(m);
                acc += D::load(tv[tile_rank(bmp, p)]) * D::load(tx[p >> 3]);
            }
        }
    }
    if (SLOTS == 8) {  // (every lane of the wave arrives: the loop's trip counts differ, the shuffles follow it)
        acc += __shfl_xor(acc, 8, kWave);
        acc += __shfl_xor(acc, 16, kWave);
        acc += __shfl_xor(acc, 32, kWave);
    }
    if (!live || g != 0) return;
    if (it.w != kWhole) {
        scratch[(uint64_t)it.w * 8 + j] = acc;
        return;
    }
    const int64_t o = (int64_t)it.x * 8 + j;
    if (o < out_len) u[o] = spmv_op_epilogue<F>(alpha, acc, beta, u, o);  // (the ragged last block)
}

// folds: {output block, first scratch slot, parts} per split block; the parts are added in item order
template <typename R>
__global__ __launch_bounds__(kThreads) void spmv_op_fold_kernel(const uint32_t *__restrict__ folds, uint64_t n_folds,
                                                                const R *__restrict__ scratch, R alpha, R beta, R *u, int64_t out_len)
{
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t f = gid >> 3;
    const int j = (int)(gid & 7);
    if (f >= n_folds) return;
    const uint32_t block = folds[3 * f], first = folds[3 * f + 1], parts = folds[3 * f + 2];
    const R *s = scratch + (uint64_t)first * 8 + j;
    R acc = s[0];
    for (uint32_t p = 1; p < parts; p++) acc += s[(uint64_t)p * 8];
    const int64_t o = (int64_t)block * 8 + j;
    if (o < out_len) u[o] = spmv_op_epilogue<R>(alpha, acc, beta, u, o);
}

template <typename R>
__global__ __launch_bounds__(kThreads) void spmv_op_epilogue_kernel(const R *__restrict__ t, R alpha, R beta, R *u, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) u[i] = spmv_op_epilogue<R>(alpha, t[i], beta, u, i);
}

// ---- the view --------------------------------------------------------------------------------------------------------------------------
// ptr[b] = first tile whose sorted key's high half is >= b
struct BlockPtrSearch {
    const uint64_t *keys;
    uint32_t n;
    uint32_t *ptr;
    __device__ void operator()(uint64_t b) const
    {
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if ((keys[mid] >> 32) < b) lo = mid + 1;
            else hi = mid;
        }
        ptr[b] = lo;
    }
};

// record i of the view: tile map[i] of A (null: tile i); `other` = the low half of sorted[i] (op T: the block-row) or A's block column
struct PackRecords {
    const uint32_t *map;
    const uint64_t *sorted, *keys, *bmps, *offsets;
    uint4 *recs;
    __device__ void operator()(uint64_t i) const
    {
        const uint32_t s = map ? map[i] : (uint32_t)i;
        const uint64_t b = bmps[s];
        recs[i] = make_uint4((uint32_t)b, (uint32_t)(b >> 32), (uint32_t)offsets[s], key_col(map ? sorted[i] : keys[s]));
    }
};

int64_t split_from_env()
{
    if (const char *e = getenv("BMSP_SPMV_OP_SPLIT")) {
        const long long s = atoll(e);
        if (s >= 1 && s < (1ll << 32)) return (int64_t)s;
    }
    return kSplitDefault;
}

size_t round16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

int64_t spmv_op_out_blocks(const bmsp_matrix_s *A, int op) { return op == BMSP_OP_T ? A->num_block_cols() : A->num_block_rows(); }
int64_t spmv_op_out_length(const bmsp_matrix_s *A, int op) { return op == BMSP_OP_T ? A->num_cols : A->num_rows; }
int64_t spmv_op_in_length(const bmsp_matrix_s *A, int op) { return op == BMSP_OP_T ? A->num_rows : A->num_cols; }
size_t spmv_op_vector_size(const bmsp_matrix_s *A) { return A->dtype == BMSP_F64 ? 8 : 4; }

void spmv_op_check_matrix(const bmsp_matrix_s *A, const char *what)
{
    refuse_view(A, what);
    if (A->block_num >= (1ll << 32)) fail(BMSP_ERR_LIMIT, "%s: more than 2^32 tiles", what);
    if (A->nnz >= (1ll << 32)) fail(BMSP_ERR_LIMIT, "%s: nnz %lld exceeds the 32-bit value offsets of the tile records", what, (long long)A->nnz);
}

// builds the view of (A, op) if it is missing: synchronises `st` (the block pointer is read back for the item planner)
bmsp_spmv_op_view &spmv_op_ensure_view(bmsp_matrix_s *A, int op, hipStream_t st)
{
    bmsp_spmv_op_view &w = A->spmv_op_views[op];
    if (w.mem) return w;
    const uint64_t nb = (uint64_t)A->block_num;
    const int64_t blocks = spmv_op_out_blocks(A, op);
    TileSort ts;  // sort temporaries (op T): transpose_matrix's sort
    DevBuf<uint32_t> tptr;
    const uint64_t *sorted = nullptr;
    const uint32_t *map = nullptr, *ptr = nullptr;
    if (op == BMSP_OP_T) {
        sort_tiles_by_block_column(A, ts, st);
        sorted = ts.keys; map = ts.map;
        tptr.alloc((size_t)blocks + 1);
        device_for_each(BlockPtrSearch{sorted, (uint32_t)nb, tptr.p}, (uint64_t)blocks + 1, st);
        ptr = tptr.p;
    } else {
        ensure_rowptr(A, st);
        ptr = A->rowptr;
    }
    std::vector<uint32_t> hptr((size_t)blocks + 1, 0u);
    BMSP_HIP(hipStreamSynchronize(st));
    copy_d2h_staged(hptr.data(), ptr, 4 * ((size_t)blocks + 1));
    const int64_t split = split_from_env();
    int64_t n_items = 0, split_blocks = 0, slots = 0;
    spmv_op_plan_items(hptr.data(), blocks, split, nullptr, nullptr, &n_items, &split_blocks, &slots);
    std::vector<uint32_t> items(4 * (size_t)n_items), folds(3 * (size_t)split_blocks);
    spmv_op_plan_items(hptr.data(), blocks, split, items.data(), folds.data(), &n_items, &split_blocks, &slots);

    bmsp_spmv_op_view nw;
    nw.blocks = blocks; nw.items = n_items; nw.split_blocks = split_blocks; nw.slots = slots;
    nw.off_ptr = round16(16 * (size_t)nb);
    nw.off_items = nw.off_ptr + (op == BMSP_OP_T ? round16(4 * ((size_t)blocks + 1)) : 0);
    nw.off_folds = nw.off_items + 16 * (size_t)n_items;
    nw.off_scratch = round16(nw.off_folds + 12 * (size_t)split_blocks);
    nw.bytes = nw.off_scratch + 8 * spmv_op_vector_size(A) * (size_t)slots;
    DevBuf<char> mem(nw.bytes);
    device_for_each(PackRecords{map, sorted, A->keys, A->bmps, A->offsets, (uint4 *)mem.p}, nb, st);
    if (op == BMSP_OP_T) BMSP_HIP(hipMemcpyAsync(mem.p + nw.off_ptr, ptr, 4 * ((size_t)blocks + 1), hipMemcpyDeviceToDevice, st));
    BMSP_HIP(hipStreamSynchronize(st));  // the sort temporaries go back to the pool
    copy_h2d_staged(mem.p + nw.off_items, items.data(), 4 * items.size());
    copy_h2d_staged(mem.p + nw.off_folds, folds.data(), 4 * folds.size());
    nw.mem.adopt((uint32_t *)mem.take());
    w = std::move(nw);
    return w;
}

namespace {

int slots_for(const bmsp_matrix_s *A, const bmsp_spmv_op_view &w)
{
    if (const char *e = getenv("BMSP_SPMV_OP_SLOTS")) {
        const int s = atoi(e);
        if (s == 1 || s == 8) return s;
    }
    return A->block_num >= kSlotsTiles * w.blocks ? 8 : 1;
}

template <typename S, bool MINOR>
void launch_sweep(const bmsp_matrix_s *A, const bmsp_spmv_op_view &w, int slots, int64_t out_len, double alpha, const void *v, double beta,
                  void *u, hipStream_t st)
{
    using R = typename TileValue<S>::R;
    const char *mem = (const char *)w.mem;
    const uint4 *recs = (const uint4 *)mem, *items = (const uint4 *)(mem + w.off_items);
    R *scratch = (R *)(mem + w.off_scratch);
    const uint64_t n = (uint64_t)w.items;
    if (slots == 8)
        hipLaunchKernelGGL((spmv_op_sweep_kernel<S, MINOR, 8>), grid_for(n * 64), dim3(kThreads), 0, st, recs, items, n, (const S *)A->values,
                           (const S *)v, (R)alpha, (R)beta, (R *)u, scratch, out_len);
    else
        hipLaunchKernelGGL((spmv_op_sweep_kernel<S, MINOR, 1>), grid_for(n * 8), dim3(kThreads), 0, st, recs, items, n, (const S *)A->values,
                           (const S *)v, (R)alpha, (R)beta, (R *)u, scratch, out_len);
    BMSP_CHECK_LAUNCH();
    if (w.split_blocks) {
        hipLaunchKernelGGL((spmv_op_fold_kernel<R>), grid_for((uint64_t)w.split_blocks * 8), dim3(kThreads), 0, st,
                           (const uint32_t *)(mem + w.off_folds), (uint64_t)w.split_blocks, (const R *)scratch, (R)alpha, (R)beta, (R *)u, out_len);
        BMSP_CHECK_LAUNCH();
    }
}

template <typename R>
void launch_epilogue(const void *t, double alpha, double beta, void *u, int64_t n, hipStream_t st)
{
    if (n == 0) return;
    hipLaunchKernelGGL((spmv_op_epilogue_kernel<R>), grid_for((uint64_t)n), dim3(kThreads), 0, st, (const R *)t, (R)alpha, (R)beta, (R *)u, n);
    BMSP_CHECK_LAUNCH();
}

// bmsp_spmv's own case: its sum, then the epilogue (the call itself when the epilogue is the identity)
void spmv_plain(bmsp_matrix_s *A, double alpha, const void *v, double beta, void *u, hipStream_t st)
{
    const bool f64 = A->dtype == BMSP_F64;
    const bool identity = f64 ? (alpha == 1.0 && beta == 0.0) : ((float)alpha == 1.0f && (float)beta == 0.0f);
    if (identity) {
        spmv(A, v, u, BMSP_SPMV_DEFAULT, st);
        return;
    }
    if (!A->spmv_op_tmp) A->spmv_op_tmp.alloc(spmv_op_vector_size(A) * (size_t)(A->num_rows ? A->num_rows : 1));
    spmv(A, v, A->spmv_op_tmp, BMSP_SPMV_DEFAULT, st);
    if (f64) launch_epilogue<double>(A->spmv_op_tmp, alpha, beta, u, A->num_rows, st);
    else launch_epilogue<float>(A->spmv_op_tmp, alpha, beta, u, A->num_rows, st);
}

}  // namespace

void spmv_op_check_op(int op)
{
    if (op != BMSP_OP_N && op != BMSP_OP_T) fail(BMSP_ERR_INVALID, "op must be BMSP_OP_N (0) or BMSP_OP_T (1) (got %d)", op);
}

// Work items of a sweep over `blocks` output blocks with tiles [ptr[b], ptr[b + 1]): a block of at most `split` tiles is one item
// {b, begin, end, ~0u}; a longer one gets ceil(n / split) items of at most `split` tiles with consecutive scratch slots and one fold
// {b, first slot, parts}.  Host only.  items / folds may be null (the counts alone).
void spmv_op_plan_items(const uint32_t *ptr, int64_t blocks, int64_t split, uint32_t *items, uint32_t *folds, int64_t *n_items,
                        int64_t *split_blocks, int64_t *slots)
{
    if (blocks < 0) fail(BMSP_ERR_INVALID, "blocks must be >= 0 (got %lld)", (long long)blocks);
    if (split < 1) fail(BMSP_ERR_INVALID, "split must be >= 1 (got %lld)", (long long)split);
    if (blocks && !ptr) fail(BMSP_ERR_INVALID, "ptr is null");
    int64_t ni = 0, nf = 0, ns = 0;
    for (int64_t b = 0; b < blocks; b++) {
        if (ptr[b + 1] < ptr[b]) fail(BMSP_ERR_INVALID, "ptr decreases at block %lld", (long long)b);
        const int64_t lo = ptr[b], hi = ptr[b + 1], n = hi - lo;
        if (n <= split) {
            if (items) { uint32_t *it = items + 4 * ni; it[0] = (uint32_t)b; it[1] = (uint32_t)lo; it[2] = (uint32_t)hi; it[3] = kWhole; }
            ni++;
            continue;
        }
        const int64_t parts = ceil_div(n, split);
        if (folds) { uint32_t *f = folds + 3 * nf; f[0] = (uint32_t)b; f[1] = (uint32_t)ns; f[2] = (uint32_t)parts; }
        nf++;
        for (int64_t k = 0; k < parts; k++, ni++, ns++) {
            if (!items) continue;
            uint32_t *it = items + 4 * ni;
            const int64_t e = lo + (k + 1) * split;
            it[0] = (uint32_t)b; it[1] = (uint32_t)(lo + k * split); it[2] = (uint32_t)(e < hi ? e : hi); it[3] = (uint32_t)ns;
        }
    }
    if (ns >= (int64_t)kWhole) fail(BMSP_ERR_LIMIT, "spmv_op: more than 2^32 - 1 scratch slots");
    if (n_items) *n_items = ni;
    if (split_blocks) *split_blocks = nf;
    if (slots) *slots = ns;
}

void spmv_op(bmsp_matrix_s *A, int op, double alpha, const void *v, double beta, void *u, hipStream_t st)
{
    spmv_op_check_op(op);
    spmv_op_check_matrix(A, "spmv_op");
    if (op == BMSP_OP_N && !A->transposed) {
        spmv_plain(A, alpha, v, beta, u, st);
        return;
    }
    const bmsp_spmv_op_view &w = spmv_op_ensure_view(A, op, st);
    if (w.items == 0) return;  // no output
    const int slots = slots_for(A, w);
    const int64_t out_len = spmv_op_out_length(A, op);
    const bool minor = (op == BMSP_OP_T) != (A->transposed != 0);
    dispatch_dtype(A->dtype, [&](auto s) {
        using S = decltype(s);
        if (minor) launch_sweep<S, true>(A, w, slots, out_len, alpha, v, beta, u, st);
        else launch_sweep<S, false>(A, w, slots, out_len, alpha, v, beta, u, st);
    });
}

// The launcher's own decisions for (A, op), and the bytes the launch moves: records (16 B per tile) + values + items (16 B each) + v + u +
// per scratch slot its 8 accumulators stored and read back + the fold list (12 B per split block).  (N, layout 0) is bmsp_spmv: its name
// behind "bmsp_spmv: ", its compulsory bytes, no view (slots, items and split_blocks 0; view_bytes = the temporary once it exists).
void spmv_op_launch_info(bmsp_matrix_s *A, int op, hipStream_t st, bmsp_spmv_op_info *info)
{
    spmv_op_check_op(op);
    spmv_op_check_matrix(A, "spmv_op");
    memset(info, 0, sizeof *info);
    if (op == BMSP_OP_N && !A->transposed) {
        char name[48];
        spmv_launch_info(A, BMSP_SPMV_DEFAULT, st, name, sizeof name, &info->compulsory_bytes, nullptr);
        snprintf(info->kernel, sizeof info->kernel, "bmsp_spmv: %s", name);
        info->view_bytes = A->spmv_op_tmp ? (int64_t)spmv_op_vector_size(A) * A->num_rows : 0;
        return;
    }
    const bmsp_spmv_op_view &w = spmv_op_ensure_view(A, op, st);
    const bool minor = (op == BMSP_OP_T) != (A->transposed != 0);
    info->slots = slots_for(A, w);
    info->items = w.items;
    info->split_blocks = w.split_blocks;
    info->view_bytes = (int64_t)w.bytes;
    if (w.items == 0) {
        snprintf(info->kernel, sizeof info->kernel, "none (no output)");
        return;
    }
    snprintf(info->kernel, sizeof info->kernel, "spmv_op_sweep_kernel<%s, %d>", minor ? "MINOR" : "MAJOR", info->slots);
    const int64_t es = (int64_t)dtype_size(A->dtype), as = (int64_t)spmv_op_vector_size(A);
    info->compulsory_bytes = 16 * A->block_num + es * A->nnz + 16 * w.items + es * spmv_op_in_length(A, op) + as * spmv_op_out_length(A, op) +
                             2 * 8 * as * w.slots + 12 * w.split_blocks;
}

}  // namespace bmsp

BMSP_DEFINE_WARM(spmv_op)
