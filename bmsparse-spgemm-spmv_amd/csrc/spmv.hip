// spmv.hip -- u = A * v on the bmSparse format, gfx950 / wave64.
//
// Reference: bmSparse_SpMV<VI,VO>, src/bmSparse_SPMV.cu:191-230 with spmv_kernel (:153-189, one 64-thread block per
// block-row, one lane per tile ELEMENT, serial loop over the row's tiles) and spmv_kernel_new (:84-150, the "batched"
// path: several tiles per step, wide lane reduction).  Both rebuild a block-row pointer on every call (:199-206).
//
// MI355X design: five kernel families -- spmv_blockrow_kernel (variants 1, 2 and matrices beyond the buffer descriptors' 4 GiB),
// spmv_rowgroup_kernel (16 lanes per block-row, 16-byte value loads), spmv_chunk_kernel (one wave per 512 stored values over its own
// structure cache), spmv_vstream_kernel (lane per stored value) and spmv_sweep_kernel (lane per tile).  Each has its header below; which
// one runs for a matrix is decided in ONE place, choose() near the end of this file, where the table of path, condition and caches is.
// All but the block-row kernels walk the cached sweep plan; spmv_sweep_kernel, described here, is the plan's first user:
//   * A per-matrix SWEEP PLAN (built once, cached like the block-row pointer) cuts the block array into wave-sized
//     work items.  Short block-rows are grouped into items aligned to block-row boundaries (<= 16 block-rows inside
//     one aligned 16-row window, < 512 tiles; ~96 tiles for the value-stream kernel), so an item owns a contiguous slice of u outright.
//     A block-row with more than 256 tiles (hub rows of web / R-MAT graphs) is cut into 256-tile items of its own.
//   * One wave per item.  Lane l loads key / bitmap / offset of tiles l and l+64 of a 128-tile batch: three fully
//     coalesced streams, no dependent pointer chase.  Work per lane is one tile whatever the row lengths are, so
//     skewed graphs stay balanced.
//       sparse tiles (<= 8 stored values): the lane peels the first two elements off the top of the bitmap and issues
//         their value / x gathers back to back (buffer loads against wave-uniform descriptors; an absent element points
//         out of range and reads 0, so there is no branch and no 64-bit address arithmetic), then adds the products into
//         the item's u tile in LDS (16 block-rows x 8 rows per wave); tiles with more values wait in an LDS queue that
//         is drained 64 tiles at a time, so every lane of a drain has work.
//       dense tiles: queued in LDS and swept by the whole wave, lane p = tile position p (contiguous value loads),
//         8-lane DPP row sums, one LDS add per tile row.
//   * Short items store their u slice with coalesced stores (empty block-rows come out as zeros for free).
//     Long-row items park their 8 partial sums in a carry slot and bump a per-row arrival counter; the last wave to
//     arrive folds all slots in a fixed order and writes the row (write-through stores + agent-scope counter,
//     self-resetting), so the whole product is ONE launch.
//   Measured alternatives (DESIGN.md "SpMV design log"): ds_add_f32 costs ~3 cycles per ACTIVE lane on gfx950 while
//   integer LDS atomics run at full rate (experiments/lds_atomic_rate.hip); an atomic-free pull formulation and an
//   integer-atomic counting-sort exchange were both built and were slower (2-3x the instructions per tile, lower
//   occupancy).  This kernel needs ~2.8 wave instructions per tile, inside the budget of an HBM-bound sweep.
// variant 1 ("batched"): a whole wave sweeps one block-row, 8 tiles x 8 tile rows per step, and folds the eight partial
//     rows with xor-shuffles (wavefront reduction): contiguous value loads per tile, for matrices with dense tiles.
// variant 2: 8-lane group per block-row (kept for comparison).
#include "spmv_plan.h"
#include "prims.hip.h"
#include <cstdlib>
#include <cstdio>
#include <algorithm>
#include <vector>
#include <type_traits>

namespace bmsp {
namespace {

constexpr uint32_t kVsGroup = 96;  // plan granularity for the value-stream kernel: most items are one 128-tile batch
// the value-stream kernel takes matrices whose tiles are mostly sparse (full tiles go to the FULL sweep / the row-group kernel)
bool vstream_eligible(const bmsp_matrix_s *A)
{
    return !(A->spmv_full_tiles * 4 >= A->block_num) && !getenv("BMSP_SPMV_OLD") && A->num_block_cols() < (1ll << 28);
}

// ---------------------------------------------------------------------------------------------------------
// plan construction (once per matrix)
// ---------------------------------------------------------------------------------------------------------
struct RowClass {
    const uint32_t *rowptr;
    const uint64_t *offsets;
    uint32_t nbr;
    uint32_t group;  // short block-rows are grouped up to the next multiple of `group` tiles
    __device__ bool is_long(uint32_t r) const { return rowptr[r + 1] - rowptr[r] > kItemTiles; }
    __device__ bool starts(uint32_t r) const
    {
        if (r == 0 || (r % kItemRows) == 0) return true;
        if (rowptr[r] / group != rowptr[r - 1] / group) return true;
        return is_long(r) || is_long(r - 1);
    }
    // packed counts: low 36 bits = items contributed by row r, high bits = 1 if long
    __device__ uint64_t operator()(uint64_t r64) const
    {
        if (r64 >= nbr) return 0;
        uint32_t r = (uint32_t)r64;
        if (is_long(r)) {
            uint32_t len = rowptr[r + 1] - rowptr[r];
            return (uint64_t)((len + kItemTiles - 1) / kItemTiles) | (1ull << 36);
        }
        return starts(r) ? 1ull : 0ull;
    }
};
struct PlanTotals {
    uint64_t n;
    uint64_t *out;
    __device__ void operator()(uint64_t i, uint64_t ex) const
    {
        if (i == n) *out = ex;
    }
};
struct FullTileIn {
    const uint64_t *bmps;
    uint64_t n;
    __device__ uint64_t operator()(uint64_t b) const { return (b < n && bmps[b] == ~0ull) ? 1ull : 0ull; }
};
struct PlanFill {
    RowClass rc;
    uint32_t nb;
    SweepItem *items;
    __device__ void operator()(uint64_t r64, uint64_t ex) const
    {
        const uint32_t base = (uint32_t)(ex & ((1ull << 36) - 1)), lbase = (uint32_t)(ex >> 36);
        const uint32_t r = (uint32_t)r64;
        if (r == rc.nbr) {
            if (rc.nbr && !rc.is_long(rc.nbr - 1)) { items[base - 1].row_end = rc.nbr; items[base - 1].blk_end = nb; items[base - 1].first_item = (uint32_t)rc.offsets[nb]; }
            return;
        }
        const bool lg = rc.is_long(r), st = lg || rc.starts(r);
        if (!st) return;
        const uint32_t s = rc.rowptr[r], e = rc.rowptr[r + 1];
        if (r > 0 && !rc.is_long(r - 1)) { items[base - 1].row_end = r; items[base - 1].blk_end = s; items[base - 1].first_item = (uint32_t)rc.offsets[s]; }
        if (lg) {
            const uint32_t cnt = (e - s + kItemTiles - 1) / kItemTiles;
            for (uint32_t c = 0; c < cnt; c++) {
                SweepItem it;
                it.row_begin = r; it.row_end = r + 1;
                it.blk_begin = s + c * kItemTiles;
                it.blk_end = min(e, s + (c + 1) * kItemTiles);
                it.first_item = base; it.num_items = cnt; it.long_idx = lbase; it.val_begin = (uint32_t)rc.offsets[it.blk_begin];
                items[base + c] = it;
            }
        } else {
            items[base].row_begin = r; items[base].blk_begin = s;
            items[base].num_items = 0; items[base].long_idx = 0xffffffffu; items[base].val_begin = (uint32_t)rc.offsets[s];
        }
    }
};

}  // namespace

void build_plan(bmsp_matrix_s *A, hipStream_t st)
{
    if (A->spmv_chunks) return;
    ensure_rowptr(A, st);
    const uint32_t nbr = (uint32_t)A->num_block_rows(), nb = (uint32_t)A->block_num;
    HostScalar<uint64_t> full_h;
    device_exclusive_scan<uint64_t>(FullTileIn{A->bmps, nb}, PlanTotals{nb, full_h.dev()}, (uint64_t)nb + 1, st);
    A->spmv_full_tiles = (int64_t)full_h.wait(st);
    // short block-rows are grouped up to the next multiple of `group` tiles: one 128-tile batch for the value-stream kernel
    const char *ge = getenv("BMSP_SPMV_GROUP");
    RowClass rc{A->rowptr, A->offsets, nbr, ge ? (uint32_t)std::max(16, atoi(ge)) : (vstream_eligible(A) ? kVsGroup : kItemTiles)};
    DevBuf<uint64_t> tot(1);
    device_exclusive_scan<uint64_t>(rc, PlanTotals{nbr, tot.p}, (uint64_t)nbr + 1, st);
    const uint64_t packed = read_back(tot.p, st);
    const uint32_t n_items = (uint32_t)(packed & ((1ull << 36) - 1)), n_long = (uint32_t)(packed >> 36);
    // one allocation: header | items | counters | carry
    const size_t acc_sz = A->dtype == BMSP_F64 ? 8 : 4;
    const size_t off_items = 64, off_cnt = off_items + sizeof(SweepItem) * (size_t)n_items;
    const size_t off_carry = (off_cnt + 4 * (size_t)n_long + 63) & ~size_t(63);
    const size_t total = off_carry + acc_sz * 8 * (size_t)n_items + 64;
    char *mem = (char *)pool_alloc(total);
    BMSP_HIP(hipMemsetAsync(mem, 0, total, st));
    uint32_t hdr[4] = {n_items, n_long, (uint32_t)off_cnt, (uint32_t)off_carry};
    BMSP_HIP(hipMemcpyAsync(mem, hdr, sizeof hdr, hipMemcpyHostToDevice, st));
    if (nbr) device_exclusive_scan<uint64_t>(rc, PlanFill{rc, nb, (SweepItem *)(mem + off_items)}, (uint64_t)nbr + 1, st);
    A->spmv_chunks.adopt((uint32_t *)mem);
    A->spmv_num_chunks = n_items;
    A->spmv_plan_long = n_long;
    A->spmv_plan_off_cnt = off_cnt;
    A->spmv_plan_off_carry = off_carry;
}

namespace {

// ---------------------------------------------------------------------------------------------------------
// the sweep kernel
// ---------------------------------------------------------------------------------------------------------
// Buffer (SRSRC) loads: 32-bit byte offsets against a wave-uniform descriptor, and an out-of-range offset returns 0.
// That removes the 64-bit address arithmetic and -- by steering absent elements to offset ~0 -- every exec-mask branch
// of the predicated gathers; x's descriptor ends at num_cols, so the ragged last block column reads as 0 by itself.
using rsrc_t = __amdgpu_buffer_rsrc_t;
constexpr uint32_t kOob = 0xffffffffu;
__device__ __forceinline__ rsrc_t make_rsrc(const void *p, uint32_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, bytes, 0x00020000);
}
template <typename T>
struct Buf;
template <>
struct Buf<float> {
    static __device__ __forceinline__ float ld(rsrc_t r, uint32_t off) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0)); }
};
template <>
struct Buf<_Float16> {
    static __device__ __forceinline__ float ld(rsrc_t r, uint32_t off) { return (float)__builtin_bit_cast(_Float16, __builtin_amdgcn_raw_buffer_load_b16(r, off, 0, 0)); }
};
template <>
struct Buf<double> {
    static __device__ __forceinline__ double ld(rsrc_t r, uint32_t off) { return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0)); }
};

// four consecutive elements with one buffer load (16 bytes for float): the full-tile path below
template <typename T>
struct Buf4;
template <>
struct Buf4<float> {
    typedef float v4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ void ld(rsrc_t r, uint32_t off, float (&o)[4])
    {
        const v4 v = __builtin_bit_cast(v4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
    }
};
template <>
struct Buf4<_Float16> {
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ void ld(rsrc_t r, uint32_t off, float (&o)[4])
    {
        const h4 v = __builtin_bit_cast(h4, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0));
        o[0] = (float)v[0]; o[1] = (float)v[1]; o[2] = (float)v[2]; o[3] = (float)v[3];
    }
};
template <>
struct Buf4<double> {
    typedef double d2 __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ void ld(rsrc_t r, uint32_t off, double (&o)[4])
    {
        const d2 a = __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
        const d2 b = __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(r, off + 16u, 0, 0));
        o[0] = a[0]; o[1] = a[1]; o[2] = b[0]; o[3] = b[1];
    }
};

__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, uint32_t l)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
}

constexpr int kSparseMax = 8;   // tiles with more stored values than this go to the wave-wide dense pass (6 would fit 7 waves per SIMD -- 71 VGPRs instead of 83 -- but sends more tiles to the dense pass: 44 vs 35.7 us on the webbase-like matrix)
constexpr int kInlineSlots = 2; // stored values of a tile handled in the streaming loop; the rest of a tile waits in a queue
                                // (1, 2 and 3 measure the same within 2 %)
constexpr int kDenseTrip = 8;   // dense tiles per trip of the wave-wide pass
constexpr uint32_t kLeftCap = 128;  // leftover queue: flushed 64 tiles at a time, so every lane has work
constexpr uint32_t kDenseCap = 64;  // dense queue, swept after each half batch
constexpr int kFullTrip = 4;        // FULL tiles (all 64 values stored): 4 tiles per wave step x kFullTrip steps in flight

template <typename A>
__device__ __forceinline__ void lds_add(A *p, A v)
{
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);  // ds_add_f32 / ds_add_f64
}

// sum over the 8 lanes of a tile row (aligned groups of 8 lanes) with DPP adds -- no LDS traffic
__device__ __forceinline__ float row8_sum(float v)
{
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));   // quad_perm 1,0,3,2
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false));   // quad_perm 2,3,0,1
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, false));  // row_half_mirror
    return v;
}
__device__ __forceinline__ double row8_sum(double v)
{
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) v += __shfl_xor(v, d, kWave);
    return v;
}

// up to N stored elements of one tile, handled by ONE lane: positions peeled off the top of the bitmap, all value / x
// loads issued back to back (absent ones point out of range and read 0), then the LDS adds (exec-masked).  Returns the
// bitmap of the elements that are left.
template <typename T, typename A, int N>
__device__ __forceinline__ uint64_t peel_tile(uint64_t bm, uint32_t voff, uint32_t xbase, A *__restrict__ trow, rsrc_t rv, rsrc_t rx)
{
    A a[N], xv[N];
    uint32_t pr[N];
    bool has[N];
#pragma unroll
    for (int j = 0; j < N; j++) {
        has[j] = bm != 0;
        const uint32_t p = (uint32_t)__clzll((long long)bm) & 63u;
        bm &= ~(0x8000000000000000ull >> p);
        pr[j] = p >> 3;
        a[j] = Buf<T>::ld(rv, has[j] ? voff + (uint32_t)(j * sizeof(T)) : kOob);
        xv[j] = Buf<T>::ld(rx, has[j] ? xbase + (p & 7u) * (uint32_t)sizeof(T) : kOob);
    }
#pragma unroll
    for (int j = 0; j < N; j++)
        if (has[j]) lds_add(trow + pr[j], a[j] * xv[j]);
    return bm;
}

// the same in two steps, so that the requests of BOTH tiles of a lane can be in flight before the first LDS add
template <typename T, typename A, int N>
struct Peeled {
    A a[N], xv[N];
    uint32_t pr[N];
    bool has[N];
    uint64_t rest;
};
template <typename T, typename A, int N>
__device__ __forceinline__ Peeled<T, A, N> peel_issue(uint64_t bm, uint32_t voff, uint32_t xbase, rsrc_t rv, rsrc_t rx)
{
    Peeled<T, A, N> q;
#pragma unroll
    for (int j = 0; j < N; j++) {
        q.has[j] = bm != 0;
        const uint32_t p = (uint32_t)__clzll((long long)bm) & 63u;
        bm &= ~(0x8000000000000000ull >> p);
        q.pr[j] = p >> 3;
        q.a[j] = Buf<T>::ld(rv, q.has[j] ? voff + (uint32_t)(j * sizeof(T)) : kOob);
        q.xv[j] = Buf<T>::ld(rx, q.has[j] ? xbase + (p & 7u) * (uint32_t)sizeof(T) : kOob);
    }
    q.rest = bm;
    return q;
}
template <typename T, typename A, int N>
__device__ __forceinline__ void peel_commit(const Peeled<T, A, N> &q, A *__restrict__ trow)
{
#pragma unroll
    for (int j = 0; j < N; j++)
        if (q.has[j]) lds_add(trow + q.pr[j], q.a[j] * q.xv[j]);
}

// FULL: matrices whose plan counted many full tiles (FEM-like) get the variant with the 16-byte-per-lane full-tile pass; the
// graph-like default keeps the leaner code (the extra pass costs the webbase-like case 7 % even when it never runs)
template <typename T, bool FULL, bool NT, bool PERSIST = false, int OCC = 1>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(OCC, 8))) void spmv_sweep_kernel(const SweepItem *__restrict__ items, uint32_t num_items,
                                                              const uint64_t *__restrict__ keys, const uint64_t *__restrict__ bmps,
                                                              const uint64_t *__restrict__ offsets, const T *__restrict__ values,
                                                              const T *__restrict__ x, typename Acc<T>::type *__restrict__ y,
                                                              typename Acc<T>::type *__restrict__ carry, uint32_t *__restrict__ counters,
                                                              uint32_t num_rows, uint32_t num_cols, uint32_t values_bytes, uint32_t row_lo)
{
    using A = typename Acc<T>::type;
    __shared__ A tile_all[4][kItemRows * 8];
    // queues of tiles waiting for a full-wave pass: (bitmap, value byte offset, x byte offset, u-tile row base)
    __shared__ uint64_t l_bmp_all[4][kLeftCap], d_bmp_all[4][kDenseCap];
    __shared__ uint32_t l_off_all[4][kLeftCap], l_xb_all[4][kLeftCap], l_tb_all[4][kLeftCap];
    __shared__ uint32_t d_off_all[4][kDenseCap], d_xb_all[4][kDenseCap], d_tb_all[4][kDenseCap];
    __shared__ uint32_t f_off_all[4][kDenseCap], f_xb_all[4][kDenseCap], f_tb_all[4][kDenseCap];
    const int w = wave_id(), lane = lane_id();
    A *tile = tile_all[w];
    uint64_t *l_bmp = l_bmp_all[w], *d_bmp = d_bmp_all[w];
    uint32_t *l_off = l_off_all[w], *l_xb = l_xb_all[w], *l_tb = l_tb_all[w];
    uint32_t *d_off = d_off_all[w], *d_xb = d_xb_all[w], *d_tb = d_tb_all[w];
    uint32_t *f_off = f_off_all[w], *f_xb = f_xb_all[w], *f_tb = f_tb_all[w];
    const rsrc_t rv = make_rsrc(values, values_bytes), rx = make_rsrc(x, num_cols * (uint32_t)sizeof(T));
    const uint64_t lt = lanemask_lt();
    // PERSIST: the grid is sized to the chip and every wave walks items with the grid stride (no relaunch gaps)
    for (uint32_t item_id = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + w); item_id < num_items; item_id += PERSIST ? gridDim.x * 4 : num_items) {
    const SweepItem it = items[item_id];
    tile[lane] = A(0);
    tile[64 + lane] = A(0);
    uint32_t n_left = 0;  // wave-uniform fill of the leftover queue
    __builtin_amdgcn_wave_barrier();

    for (uint32_t base = it.blk_begin; base < it.blk_end; base += kBatch) {
        // lane-per-tile: three coalesced streams, two tiles per lane
        const uint32_t b0 = base + lane, b1 = base + 64 + lane;
        uint64_t bm0 = 0, bm1 = 0, k0 = (uint64_t)it.row_begin << 32, k1 = k0, o0 = 0, o1 = 0;
        if (NT) {  // streamed once: non-temporal, so that the tile words do not push x out of the L2
            if (b0 < it.blk_end) { bm0 = __builtin_nontemporal_load(bmps + b0); k0 = __builtin_nontemporal_load(keys + b0); o0 = __builtin_nontemporal_load(offsets + b0); }
            if (b1 < it.blk_end) { bm1 = __builtin_nontemporal_load(bmps + b1); k1 = __builtin_nontemporal_load(keys + b1); o1 = __builtin_nontemporal_load(offsets + b1); }
        } else {
            if (b0 < it.blk_end) { bm0 = bmps[b0]; k0 = keys[b0]; o0 = offsets[b0]; }
            if (b1 < it.blk_end) { bm1 = bmps[b1]; k1 = keys[b1]; o1 = offsets[b1]; }
        }
        const uint32_t x0 = key_col(k0) * 8u * (uint32_t)sizeof(T), x1 = key_col(k1) * 8u * (uint32_t)sizeof(T);
        const uint32_t tb0 = (key_row(k0) - it.row_begin) * 8u, tb1 = (key_row(k1) - it.row_begin) * 8u;
        const uint32_t vo0 = (uint32_t)o0 * (uint32_t)sizeof(T), vo1 = (uint32_t)o1 * (uint32_t)sizeof(T);
        // the inline element requests of both tiles go out together (one memory round trip for the pair, not two)
        const bool sp0 = !(FULL && bm0 == ~0ull) && __popcll(bm0) <= kSparseMax, sp1 = !(FULL && bm1 == ~0ull) && __popcll(bm1) <= kSparseMax;
        const Peeled<T, A, kInlineSlots> pe0 = peel_issue<T, A, kInlineSlots>(sp0 ? bm0 : 0ull, vo0, x0, rv, rx);
        const Peeled<T, A, kInlineSlots> pe1 = peel_issue<T, A, kInlineSlots>(sp1 ? bm1 : 0ull, vo1, x1, rv, rx);
        // the two tiles of a lane are queued one after the other so that the queues never hold more than 64 new entries
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint64_t bm = h ? bm1 : bm0;
            const uint32_t vo = h ? vo1 : vo0, xb = h ? x1 : x0, tb = h ? tb1 : tb0;
            // full tiles have their own queue: no bitmap, values at fixed places
            const bool full = FULL && bm == ~0ull && (sizeof(T) >= 4 || (vo & 3u) == 0u);  // multi-dword loads want dword-aligned values
            const uint64_t fm = __ballot(full);
            const int fn = __popcll(fm);
            if (full) {
                const int s = __popcll(fm & lt);
                f_off[s] = vo; f_xb[s] = xb; f_tb[s] = tb;
            }
            // other dense tiles are queued for the wave-wide pass
            const bool dense = !full && __popcll(bm) > kSparseMax;
            const uint64_t dm = __ballot(dense);
            const int qn = __popcll(dm);
            if (dense) {
                const int s = __popcll(dm & lt);
                d_bmp[s] = bm; d_off[s] = vo; d_xb[s] = xb; d_tb[s] = tb;
            }
            // every sparse tile: its first kInlineSlots stored values right here (covers most tiles of a graph matrix entirely)
            peel_commit<T, A, kInlineSlots>(h ? pe1 : pe0, tile + tb);
            const uint64_t rest = h ? pe1.rest : pe0.rest;
            // tiles with more values wait in the leftover queue until 64 of them make a full wave
            const uint64_t lm = __ballot(rest != 0);
            if (rest) {
                const uint32_t s = n_left + (uint32_t)__popcll(lm & lt);
                l_bmp[s] = rest; l_off[s] = vo + kInlineSlots * (uint32_t)sizeof(T); l_xb[s] = xb; l_tb[s] = tb;
            }
            n_left += (uint32_t)__popcll(lm);
            __builtin_amdgcn_wave_barrier();
            if (n_left >= 64u) {
                n_left -= 64u;
                const uint32_t s = n_left + (uint32_t)lane;
                peel_tile<T, A, kSparseMax - kInlineSlots>(l_bmp[s], l_off[s], l_xb[s], tile + l_tb[s], rv, rx);
            }
            // full tiles: 16 lanes per tile, each lane four consecutive values of one tile row (one 16-byte load) against the
            // matching four x entries; the two half-rows meet in one DPP add; four tiles per step, kFullTrip steps in flight
            for (int q = 0; FULL && q < fn; q += 4 * kFullTrip) {
                const int ts = lane >> 4, rr = (lane >> 1) & 7, hf = lane & 1;
                A part[kFullTrip];
#pragma unroll
                for (int t = 0; t < kFullTrip; t++) {
                    const int e = q + 4 * t + ts;
                    const bool on = e < fn;
                    const int ee = on ? e : 0;
                    A a4[4], x4[4];
                    Buf4<T>::ld(rv, on ? f_off[ee] + (uint32_t)((rr * 8 + hf * 4) * sizeof(T)) : kOob, a4);
                    Buf4<T>::ld(rx, on ? f_xb[ee] + (uint32_t)(hf * 4 * sizeof(T)) : kOob, x4);
                    part[t] = a4[0] * x4[0] + a4[1] * x4[1] + a4[2] * x4[2] + a4[3] * x4[3];
                }
#pragma unroll
                for (int t = 0; t < kFullTrip; t++) {
                    const int e = q + 4 * t + ts;
                    const A other = __shfl_xor(part[t], 1, kWave);
                    if (e < fn && hf == 0) lds_add(tile + f_tb[e] + rr, part[t] + other);
                }
            }
            // dense tiles: the whole wave per tile, lane p owns tile position p (coalesced value loads), kDenseTrip tiles per trip
            for (int q = 0; q < qn; q += kDenseTrip) {
                A pa[kDenseTrip];
#pragma unroll
                for (int t = 0; t < kDenseTrip; t++) {
                    const int e = min(q + t, qn - 1);
                    const uint64_t bb = q + t < qn ? d_bmp[e] : 0ull;
                    const bool has = tile_has(bb, lane);
                    const A av = Buf<T>::ld(rv, has ? d_off[e] + (uint32_t)tile_rank(bb, lane) * (uint32_t)sizeof(T) : kOob);
                    const A xx = Buf<T>::ld(rx, has ? d_xb[e] + ((uint32_t)lane & 7u) * (uint32_t)sizeof(T) : kOob);
                    pa[t] = av * xx;
                }
#pragma unroll
                for (int t = 0; t < kDenseTrip; t++) {
                    const int e = min(q + t, qn - 1);
                    const A sum = row8_sum(pa[t]);
                    if (q + t < qn && (lane & 7) == 0 && tile_byte(d_bmp[e], lane >> 3)) lds_add(tile + d_tb[e] + (lane >> 3), sum);
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    // the leftover tiles that never filled a wave
    if (n_left) {
        const bool on = (uint32_t)lane < n_left;
        peel_tile<T, A, kSparseMax - kInlineSlots>(on ? l_bmp[lane] : 0ull, on ? l_off[lane] : 0u, on ? l_xb[lane] : 0u, tile + (on ? l_tb[lane] : 0u), rv, rx);
    }
    __builtin_amdgcn_wave_barrier();

    if (it.num_items == 0) {
        // short item: the wave owns u[row_begin*8, row_end*8)
        const uint32_t n_out = (it.row_end - it.row_begin) * 8u, out0 = it.row_begin * 8u;
        for (uint32_t e = lane; e < n_out; e += 64)
            if (out0 + e >= row_lo && out0 + e < num_rows) y[out0 + e] = tile[e];
        __builtin_amdgcn_wave_barrier();
        continue;
    }
    // long row: park the partial sums, the last arriver folds them.  Write-through (sc1) stores + drained vmcnt +
    // agent-scope counter add; the wave whose add comes last reads every slot with sc1 loads (MI355X_MICROARCH.md
    // "Valid forms": every store and load of the handed-off bytes sc1, no cache-wide fence -- a release fence per item
    // writes back the whole L2 thousands of times per launch: measured 10x slower).
    if (lane < 8) __hip_atomic_store(&carry[(size_t)item_id * 8 + lane], tile[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    uint32_t ticket = 0;
    if (lane == 0) ticket = __hip_atomic_fetch_add(&counters[it.long_idx], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ticket = __builtin_amdgcn_readfirstlane(ticket);
    if (ticket != it.num_items - 1) continue;
    // lanes 0..7 own tile row `r`; lane group g = lane/8 walks items g, g+8, ...; fixed order
    const int r = lane & 7, g = lane >> 3;
    A sum = 0;
    for (uint32_t c = g; c < it.num_items; c += 8)
        sum += __hip_atomic_load(&carry[(size_t)(it.first_item + c) * 8 + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int d = 8; d < 64; d <<= 1) sum += __shfl_xor(sum, d, kWave);
    const uint32_t row = it.row_begin * 8u + (uint32_t)r;
    if (g == 0 && row >= row_lo && row < num_rows) y[row] = sum;
    if (lane == 0) __hip_atomic_store(&counters[it.long_idx], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---------------------------------------------------------------------------------------------------------
// value-stream sweep (round 2; the default for matrices whose tiles are mostly sparse)
// ---------------------------------------------------------------------------------------------------------
// Same plan, same items, same epilogue as the sweep above, but the elements are walked LANE PER STORED VALUE instead of lane per tile:
//   1. lane-per-tile: the tile words of up to 128 tiles (two per lane, coalesced); the batch is the longest run of those tiles that holds
//      at most 512 stored values;
//   2. every stored value has a 16-bit ENTRY {tile slot in the batch, position in the tile} at its index inside the batch.  kDecode
//      builds the entries in LDS from the bitmaps (a loop of max-popcount trips over the tile lanes: 36 % of the kernel's VALU work on
//      the webbase-like matrix, 52 % on the cage-like one).  kCached reads them from the POSITION CACHE -- the same entries, written
//      once per matrix by kBuild into a 2-byte-per-value array that sits beside the values (part of the cached SpMV plan, like the
//      block-row pointer and the items; bmsp_matrix_prepare builds it, BMSP_SPMV_NO_POSCACHE=1 or a cache above BMSP_SPMV_POSCACHE_MAX
//      bytes keeps the decode in the kernel).  With the cache the bitmaps are not read at all: keys + next offsets + entries + values.
//   3. lane-per-value: value v is ONE coalesced load of the value array (no value gather), its x entry one gather with every lane busy.
//   4. reduction into the item's u tile in LDS.  kAtomic: ds_add_f32 -- 3 cycles per active lane on gfx950
//      (experiments/lds_atomic_rate.hip), affordable at < 2 values per tile.  kSorted: the products are counting-sorted by row with
//      INTEGER LDS atomics (full rate), run sums are taken with DPP steps, the last lane of a run adds to the tile with a plain
//      read-modify-write.
#ifndef BMSP_VS_TILES
#define BMSP_VS_TILES 128
#endif
#ifndef BMSP_VS_PRE
#define BMSP_VS_PRE 4
#endif
constexpr uint32_t kVsTiles = BMSP_VS_TILES;  // tiles per batch at most
constexpr int kVsTpl = (int)kVsTiles / 64;    // ... = tiles per lane
constexpr uint32_t kVsVals = 512;   // values per batch at most
constexpr int kVsChunks = kVsVals / 64;
enum { kDecode = 0, kCached = 1, kBuild = 2 };
enum { kAtomic = 0, kSorted = 1 };

// lane i receives `src` of the lane the DPP control names; lanes without a source (or outside ROW_MASK) keep `old`
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t old, uint32_t src)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)src, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp_val(float old, float src)
{
    return __builtin_bit_cast(float, dpp_u32<CTRL, ROW_MASK>(__builtin_bit_cast(uint32_t, old), __builtin_bit_cast(uint32_t, src)));
}
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ double dpp_val(double old, double src)
{
    const uint64_t o = __builtin_bit_cast(uint64_t, old), v = __builtin_bit_cast(uint64_t, src);
    const uint32_t lo = dpp_u32<CTRL, ROW_MASK>((uint32_t)o, (uint32_t)v), hi = dpp_u32<CTRL, ROW_MASK>((uint32_t)(o >> 32), (uint32_t)(v >> 32));
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
// inclusive sums over runs of equal `key` in lane order (keys are sorted, so equal keys d lanes apart mean one run)
template <typename A>
__device__ __forceinline__ A wave_run_sum(A v, uint32_t key)
{
#define BMSP_RUN_STEP(CTRL, RM)                                   \
    {                                                             \
        const A pv = dpp_val<CTRL, RM>(A(0), v);                  \
        const uint32_t pk = dpp_u32<CTRL, RM>(0xffffffffu, key);  \
        v += pk == key ? pv : A(0);                               \
    }
    BMSP_RUN_STEP(0x111, 0xf)  // row_shr:1
    BMSP_RUN_STEP(0x112, 0xf)  // row_shr:2
    BMSP_RUN_STEP(0x114, 0xf)  // row_shr:4
    BMSP_RUN_STEP(0x118, 0xf)  // row_shr:8
    BMSP_RUN_STEP(0x142, 0xa)  // row_bcast:15 -> rows 1 and 3
    BMSP_RUN_STEP(0x143, 0xc)  // row_bcast:31 -> rows 2 and 3
#undef BMSP_RUN_STEP
    return v;
}
__device__ __forceinline__ uint32_t wave_inclusive_sum_dpp(uint32_t v)
{
    v += dpp_u32<0x111>(0, v);
    v += dpp_u32<0x112>(0, v);
    v += dpp_u32<0x114>(0, v);
    v += dpp_u32<0x118>(0, v);
    v += dpp_u32<0x142, 0xa>(0, v);
    v += dpp_u32<0x143, 0xc>(0, v);
    return v;
}

template <typename A, int MODE, int RED>
struct VsLds {
    // u tile (16 block-rows x 8) | tile slots | [row counters, then row starts] | [entries, then the products in row order] | [their rows]
    static constexpr uint32_t tile = 0, tinfo = tile + kItemRows * 8 * sizeof(A), cnt = tinfo + kVsTiles * 4;
    static constexpr uint32_t region = cnt + (RED == kSorted ? kItemRows * 8 * 4 : 0);
    static constexpr uint32_t region_bytes = (RED == kSorted ? kVsVals * sizeof(A) : (MODE == kCached ? 0 : kVsVals * 2));
    static constexpr uint32_t srow = region + region_bytes;
    static constexpr uint32_t bytes = srow + (RED == kSorted ? kVsVals : 0);
};

// what a wave requests for an item before it works on it (kCached): the keys of its first 128 tiles, their end offsets unless the item is
// a single batch, and entries + values of its first 256 values
constexpr int kPre = BMSP_VS_PRE;
template <typename A>
struct VsPre {
    uint32_t ti[kVsTpl];  // the tile's slot word {block column, block-row inside the item's window}, from the tile cache
    uint32_t oe[kVsTpl];  // end of the tile's values relative to the item's first value (multi-batch items only)
    uint32_t e[kPre];
    A a[kPre];
};
// values of the item (short items carry their value range; a long-row item holds 256 tiles, its count is not in the plan)
__host__ __device__ __forceinline__ uint32_t vs_item_values(const SweepItem &it) { return it.num_items == 0 ? it.first_item - it.val_begin : 64u * kPre; }
// the common case: the whole item is one batch, and the item says how many values that is -- no offset is read
__host__ __device__ __forceinline__ bool vs_single(const SweepItem &it)
{
    return it.num_items == 0 && it.blk_end - it.blk_begin <= kVsTiles && vs_item_values(it) <= kVsVals;
}
template <typename T>
__device__ __forceinline__ void vs_request(const SweepItem &it, int lane, const uint32_t *__restrict__ tcache, const uint16_t *__restrict__ eoff,
                                           rsrc_t rv, rsrc_t rp, uint32_t pos_base, VsPre<typename Acc<T>::type> &pre)
{
    const uint32_t bend = min(it.blk_begin + kVsTiles, it.blk_end);
    const bool single = vs_single(it);
#pragma unroll
    for (int t = 0; t < kVsTpl; t++) {
        const uint32_t b = it.blk_begin + 64u * (uint32_t)t + (uint32_t)lane;
        pre.ti[t] = 0;
        pre.oe[t] = 0;
        if (b < bend) pre.ti[t] = tcache[b];
        if (!single && b < bend) pre.oe[t] = (uint32_t)eoff[b];
    }
    const uint32_t n_item = vs_item_values(it);
#pragma unroll
    for (int u = 0; u < kPre; u++) {
        const uint32_t idx = 64u * (uint32_t)u + (uint32_t)lane;
        const bool on = idx < n_item;
        pre.e[u] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(rp, on ? (it.val_begin - pos_base + idx) * 2u : kOob, 0, 0);
        pre.a[u] = Buf<T>::ld(rv, on ? (it.val_begin + idx) * (uint32_t)sizeof(T) : kOob);
    }
}

// One wave per workgroup (a finished wave frees its slot and its LDS at once), one item per wave.  (A resident grid whose waves walk items
// id, id + grid, ... with the next item's requests in flight behind the current item's x gathers was built and measured: 33.9 us instead
// of 28.3 on the webbase-like matrix -- 79 / 114 VGPRs for the two request sets, and the hardware's wave dispatcher balances one-item
// waves better than a static walk does.)
template <typename T, int MODE, int RED>
__global__ __launch_bounds__(64, sizeof(typename Acc<T>::type) == 4 ? 8 : 1) void spmv_vstream_kernel(const SweepItem *__restrict__ items, uint32_t num_items,
                                                          const uint64_t *__restrict__ keys, const uint64_t *__restrict__ bmps,
                                                          const uint64_t *__restrict__ offsets, const T *__restrict__ values,
                                                          const T *__restrict__ x, typename Acc<T>::type *__restrict__ y,
                                                          typename Acc<T>::type *__restrict__ carry, uint32_t *__restrict__ counters,
                                                          uint32_t num_rows, uint32_t num_cols, uint32_t values_bytes,
                                                          uint16_t *__restrict__ pos, uint32_t pos_base, uint32_t pos_count, uint32_t row_lo,
                                                          uint32_t *__restrict__ tcache, uint16_t *__restrict__ eoff)
{
    using A = typename Acc<T>::type;
    using L = VsLds<A, MODE, RED>;
    __shared__ __attribute__((aligned(16))) unsigned char lds[L::bytes];
    A *const tile = (A *)(lds + L::tile);
    uint32_t *const tinfo = (uint32_t *)(lds + L::tinfo);
    uint32_t *const cnt = (uint32_t *)(lds + L::cnt);
    uint16_t *const ent = (uint16_t *)(lds + L::region);
    A *const sorted = (A *)(lds + L::region);
    uint8_t *const srow = lds + L::srow;
    const int lane = lane_id();
    const rsrc_t rv = make_rsrc(values, values_bytes), rx = make_rsrc(x, num_cols * (uint32_t)sizeof(T));
    const rsrc_t rp = make_rsrc(pos, pos_count * 2u);
    const uint32_t item_id = blockIdx.x;
    const SweepItem it = items[item_id];
    VsPre<A> pre;
    if (MODE == kCached) vs_request<T>(it, lane, tcache, eoff, rv, rp, pos_base, pre);
    {
        tile[lane] = A(0);
        tile[64 + lane] = A(0);
        const uint32_t n_item = vs_item_values(it);
        const bool single = MODE == kCached && vs_single(it);
        const bool long_item = RED == kAtomic && it.num_items != 0;  // (in the kSorted kernels the eight sums cost registers the sort needs: 64 -> spills)
        A acc8[8] = {A(0), A(0), A(0), A(0), A(0), A(0), A(0), A(0)};

        for (uint32_t base = it.blk_begin; base < it.blk_end;) {
            const bool first = MODE == kCached && base == it.blk_begin;
            const uint32_t bend = min(base + kVsTiles, it.blk_end);
            uint64_t bm[kVsTpl], kk[kVsTpl];
            uint32_t ti[kVsTpl];              // kCached: the tile's slot word straight from the tile cache
            uint32_t ob[kVsTpl], eb[kVsTpl];  // start / end of the tile's values, relative to the batch's first value
            uint32_t v_first = first ? it.val_begin : 0u;
            uint32_t v_rel = 0;               // kCached, later batches: the batch's first value relative to the item's
            if (MODE == kCached && !first) { v_rel = (uint32_t)eoff[base - 1]; v_first = it.val_begin + v_rel; }
#pragma unroll
            for (int t = 0; t < kVsTpl; t++) {
                const uint32_t b = base + 64u * (uint32_t)t + (uint32_t)lane;
                bm[t] = 0; kk[t] = (uint64_t)it.row_begin << 32; ob[t] = 0; eb[t] = kOob; ti[t] = 0;
                if (first) {
                    ti[t] = pre.ti[t];
                    if (b < bend) eb[t] = single ? 0u : pre.oe[t];
                } else if (MODE == kCached) {
                    if (b < bend) { ti[t] = tcache[b]; eb[t] = (uint32_t)eoff[b] - v_rel; }
                } else {
                    if (b < bend) { bm[t] = bmps[b]; kk[t] = keys[b]; ob[t] = (uint32_t)offsets[b]; }
                }
            }
            if (MODE != kCached) {
                v_first = __builtin_amdgcn_readfirstlane(ob[0]);
#pragma unroll
                for (int t = 0; t < kVsTpl; t++) {
                    ob[t] -= v_first;
                    eb[t] = ob[t] + (uint32_t)__popcll(bm[t]);  // lanes past the batch: 0 - v_first, far above the cut
                }
            }
            // the batch: tiles whose values end inside the first kVsVals values (a prefix: offsets ascend; >= 8 tiles, a tile holds <= 64)
            bool ok[kVsTpl];
            uint32_t nb = 0;
#pragma unroll
            for (int t = 0; t < kVsTpl; t++) {
                ok[t] = base + 64u * (uint32_t)t + (uint32_t)lane < bend && eb[t] <= kVsVals;
                nb += (uint32_t)__popcll(__ballot(ok[t]));
            }
            uint32_t nvals = n_item;
            if (!single) {
                uint32_t el = eb[0];
#pragma unroll
                for (int t = 1; t < kVsTpl; t++) el = (nb - 1u) >> 6 == (uint32_t)t ? eb[t] : el;
                nvals = (uint32_t)__builtin_amdgcn_readlane((int)el, (int)((nb - 1u) & 63u));
            }
            // tile slots: column and row-in-window of every tile of the batch
#pragma unroll
            for (int t = 0; t < kVsTpl; t++) tinfo[64 * t + lane] = MODE == kCached ? ti[t] : (key_col(kk[t]) | ((key_row(kk[t]) - it.row_begin) << 28));
            if (RED == kSorted) {
                cnt[lane] = 0;
                cnt[64 + lane] = 0;
            }
            if (MODE != kCached) {
                // entries from the bitmaps: {slot, position} of every stored value, at the value's index inside the batch
                uint64_t any = 0;
#pragma unroll
                for (int t = 0; t < kVsTpl; t++) {
                    bm[t] = ok[t] ? bm[t] : 0;
                    any |= bm[t];
                }
                while (__any(any != 0)) {
                    any = 0;
#pragma unroll
                    for (int t = 0; t < kVsTpl; t++) {
                        if (bm[t]) {
                            const uint32_t p = (uint32_t)__clzll((long long)bm[t]);
                            bm[t] &= ~(0x8000000000000000ull >> p);
                            ent[ob[t]++] = (uint16_t)(((64u * (uint32_t)t + (uint32_t)lane) << 6) | p);
                        }
                        any |= bm[t];
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            if (MODE == kBuild) {
                // the tile cache: slot word and end of the tile's values relative to the item's first value (every tile of the batch)
#pragma unroll
                for (int t = 0; t < kVsTpl; t++) {
                    const uint32_t b = base + 64u * (uint32_t)t + (uint32_t)lane;
                    if (ok[t]) {
                        tcache[b] = key_col(kk[t]) | ((key_row(kk[t]) - it.row_begin) << 28);
                        eoff[b] = (uint16_t)(v_first + eb[t] - it.val_begin);
                    }
                }
                for (uint32_t idx = (uint32_t)lane; idx < nvals; idx += 64u) pos[v_first - pos_base + idx] = ent[idx];
                __builtin_amdgcn_wave_barrier();
                base += nb;
                continue;
            }
            const uint32_t pos_first = (v_first - pos_base) * 2u;

            if (RED == kAtomic || long_item) {
                for (uint32_t c0 = 0; c0 < nvals; c0 += 256u) {
                    A av[4], xv[4];
                    uint32_t rowl[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const uint32_t idx = c0 + 64u * (uint32_t)u + (uint32_t)lane;
                        const bool on = idx < nvals;
                        uint32_t e;
                        if (first && c0 == 0) {
                            e = pre.e[u];
                            av[u] = pre.a[u];
                        } else {
                            e = MODE == kCached ? (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(rp, on ? pos_first + idx * 2u : kOob, 0, 0) : (on ? (uint32_t)ent[idx] : 0u);
                            av[u] = Buf<T>::ld(rv, on ? (v_first + idx) * (uint32_t)sizeof(T) : kOob);
                        }
                        const uint32_t ti = tinfo[e >> 6], p = e & 63u;
                        rowl[u] = (ti >> 28) * 8u + (p >> 3);
                        xv[u] = Buf<T>::ld(rx, on ? ((ti & 0x0fffffffu) * 8u + (p & 7u)) * (uint32_t)sizeof(T) : kOob);
                    }
                    if (long_item) {
                        // a long block-row: every product belongs to one of EIGHT rows -- eight register sums per lane, folded once
                        // per item, instead of 64 LDS float adds on eight addresses per instruction
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            const A pr = c0 + 64u * (uint32_t)u + (uint32_t)lane < nvals ? av[u] * xv[u] : A(0);
#pragma unroll
                            for (int k = 0; k < 8; k++) acc8[k] += rowl[u] == (uint32_t)k ? pr : A(0);
                        }
                    } else {
#pragma unroll
                        for (int u = 0; u < 4; u++)
                            if (c0 + 64u * (uint32_t)u + (uint32_t)lane < nvals) lds_add(tile + rowl[u], av[u] * xv[u]);
                    }
                }
            } else {
                // the value's rank among the values of its row: integer LDS counter
                A prod[kVsChunks];
                A xg[kVsChunks];
                uint32_t rr[kVsChunks];  // row | rank << 8
#pragma unroll
                for (int u = 0; u < kVsChunks; u++) {
                    if (64u * (uint32_t)u < nvals) {
                        const uint32_t idx = 64u * (uint32_t)u + (uint32_t)lane;
                        const bool on = idx < nvals;
                        uint32_t e;
                        A av;
                        if (first && u < kPre) {
                            e = pre.e[u];
                            av = pre.a[u];
                        } else {
                            e = MODE == kCached ? (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(rp, on ? pos_first + idx * 2u : kOob, 0, 0) : (on ? (uint32_t)ent[idx] : 0u);
                            av = Buf<T>::ld(rv, on ? (v_first + idx) * (uint32_t)sizeof(T) : kOob);
                        }
                        const uint32_t ti = tinfo[e >> 6], p = e & 63u;
                        const uint32_t rowl = (ti >> 28) * 8u + (p >> 3);
                        xg[u] = Buf<T>::ld(rx, on ? ((ti & 0x0fffffffu) * 8u + (p & 7u)) * (uint32_t)sizeof(T) : kOob);
                        uint32_t rank = 0;
                        if (on) rank = __hip_atomic_fetch_add(&cnt[rowl], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                        rr[u] = rowl | (rank << 8);
                        prod[u] = av;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                // row counters -> row starts (exclusive sums; lane l owns rows 2l and 2l+1)
                {
                    const uint32_t c0 = cnt[2 * lane], c1 = cnt[2 * lane + 1];
                    const uint32_t ex = wave_inclusive_sum_dpp(c0 + c1) - (c0 + c1);
                    cnt[2 * lane] = ex;
                    cnt[2 * lane + 1] = ex + c0;
                }
                __builtin_amdgcn_wave_barrier();
                // products into row order (the entries of kDecode live in the same bytes: all of them were read above)
#pragma unroll
                for (int u = 0; u < kVsChunks; u++) {
                    if (64u * (uint32_t)u < nvals) {
                        if (64u * (uint32_t)u + (uint32_t)lane < nvals) {
                            const uint32_t rowl = rr[u] & 0xffu, at = cnt[rowl] + (rr[u] >> 8);
                            sorted[at] = prod[u] * xg[u];
                            srow[at] = (uint8_t)rowl;
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();
                // run sums; the last lane of every run adds its sum to the u tile (one lane per row and chunk: no atomic)
#pragma unroll
                for (int u = 0; u < kVsChunks; u++) {
                    if (64u * (uint32_t)u < nvals) {
                        const uint32_t idx = 64u * (uint32_t)u + (uint32_t)lane;
                        const bool on = idx < nvals;
                        const A sv = on ? sorted[idx] : A(0);
                        const uint32_t row = on ? (uint32_t)srow[idx] : 0xfeu;
                        const uint32_t nxt = (lane < 63 && idx + 1u < nvals) ? (uint32_t)srow[idx + 1u] : 0xffu;
                        const A run = wave_run_sum(sv, row);
                        if (on && nxt != row) tile[row] += run;
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            base += nb;
        }

        if (MODE != kBuild) {
            if (it.num_items == 0) {
                // short item: the wave owns u[row_begin*8, row_end*8)
                const uint32_t n_out = (it.row_end - it.row_begin) * 8u, out0 = it.row_begin * 8u;
                for (uint32_t e = lane; e < n_out; e += 64)
                    if (out0 + e >= row_lo && out0 + e < num_rows) y[out0 + e] = tile[e];
            } else {
                // long row: park the partial sums, the last arriver folds them (same protocol as spmv_sweep_kernel)
                A mine = lane < 8 ? tile[lane & 7] : A(0);
                if (long_item) {
#pragma unroll
                    for (int k = 0; k < 8; k++) {
                        const A sk = wave_sum(acc8[k]);
                        mine = lane == k ? sk : mine;
                    }
                }
                if (lane < 8) __hip_atomic_store(&carry[(size_t)item_id * 8 + lane], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                uint32_t ticket = 0;
                if (lane == 0) ticket = __hip_atomic_fetch_add(&counters[it.long_idx], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ticket = __builtin_amdgcn_readfirstlane(ticket);
                if (ticket == it.num_items - 1) {
                    const int r = lane & 7, g = lane >> 3;
                    A sum = 0;
                    for (uint32_t c = g; c < it.num_items; c += 8)
                        sum += __hip_atomic_load(&carry[(size_t)(it.first_item + c) * 8 + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                    for (int d = 8; d < 64; d <<= 1) sum += __shfl_xor(sum, d, kWave);
                    const uint32_t row = it.row_begin * 8u + (uint32_t)r;
                    if (g == 0 && row >= row_lo && row < num_rows) y[row] = sum;
                    if (lane == 0) __hip_atomic_store(&counters[it.long_idx], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
}

// the position cache: kBuild pass over the plan's items, once per matrix
void build_pos_cache(bmsp_matrix_s *A, hipStream_t st)
{
    if (A->spmv_pos || A->spmv_pos_tried) return;
    A->spmv_pos_tried = 1;
    const char *cap_e = getenv("BMSP_SPMV_POSCACHE_MAX");
    const size_t cap = cap_e ? (size_t)strtoull(cap_e, nullptr, 10) : (size_t)4 << 30;
    if (getenv("BMSP_SPMV_NO_POSCACHE") || A->block_num == 0) return;
    const uint64_t base = A->view_values_end ? read_back(A->offsets, st) : 0;  // a row-panel view keeps the parent's absolute offsets
    const uint64_t count = (uint64_t)A->values_extent() - base;
    if (count == 0 || count * 2 > cap || count >= (1ull << 31)) return;
    // one allocation: entries (2 B per stored value) | tile slot words (4 B per tile) | tile value ends relative to the item (2 B per tile)
    const size_t nb = (size_t)A->block_num;
    const size_t off_ti = (count * 2 + 63) & ~size_t(63), off_eo = off_ti + ((nb * 4 + 63) & ~size_t(63));
    char *blk = (char *)pool_alloc(off_eo + nb * 2 + 64);
    uint16_t *pos = (uint16_t *)blk;
    A->spmv_tinfo = (uint32_t *)(blk + off_ti);
    A->spmv_eoff = (uint16_t *)(blk + off_eo);
    const char *mem = (const char *)A->spmv_chunks;
    const uint32_t n_items = (uint32_t)A->spmv_num_chunks;
    hipLaunchKernelGGL((spmv_vstream_kernel<float, kBuild, kAtomic>), dim3(n_items), dim3(64), 0, st, (const SweepItem *)(mem + 64), n_items, A->keys,
                       A->bmps, A->offsets, (const float *)nullptr, (const float *)nullptr, (float *)nullptr, (float *)nullptr, (uint32_t *)nullptr,
                       (uint32_t)A->num_rows, (uint32_t)A->num_cols, 0u, pos, (uint32_t)base, (uint32_t)count, 0u, A->spmv_tinfo, A->spmv_eoff);
    BMSP_CHECK_LAUNCH();
    A->spmv_pos.adopt(pos);
    A->spmv_pos_base = (int64_t)base;
    A->spmv_pos_count = (int64_t)count;
}

// ---------------------------------------------------------------------------------------------------------
// block-row kernels (variants 1 and 2)
// ---------------------------------------------------------------------------------------------------------
// one tile row: byte = bits of row r (MSB = column 0), vals points at the first stored value of that row
template <typename T, typename A>
__device__ __forceinline__ A tile_row_dot(uint32_t byte, const T *__restrict__ vals, const T *__restrict__ x, uint32_t xbase,
                                          uint32_t num_cols, A acc)
{
    while (byte) {
        int c = __clz((int)byte) - 24;  // leading set bit of an 8-bit value -> column
        byte &= ~(0x80u >> c);
        uint32_t col = xbase + (uint32_t)c;
        A a = (A)(*vals++);
        A xv = col < num_cols ? (A)x[col] : A(0);
        acc = __builtin_fma(a, xv, acc);
    }
    return acc;
}

template <typename T, int LANES_PER_ROW>
__global__ __launch_bounds__(kThreads) void spmv_blockrow_kernel(const uint32_t *__restrict__ rowptr, const uint64_t *__restrict__ keys,
                                                                 const uint64_t *__restrict__ bmps, const uint64_t *__restrict__ offsets,
                                                                 const T *__restrict__ values, const T *__restrict__ x,
                                                                 typename Acc<T>::type *__restrict__ y, uint32_t num_rows,
                                                                 uint32_t num_cols, uint32_t num_block_rows, uint32_t row_lo)
{
    using A = typename Acc<T>::type;
    constexpr int GROUPS = LANES_PER_ROW / 8;  // tiles in flight per block-row per step
    const uint32_t gid = blockIdx.x * (kThreads / LANES_PER_ROW) + threadIdx.x / LANES_PER_ROW;
    if (gid >= num_block_rows) return;  // uniform per LANES_PER_ROW-lane group
    const int sub = threadIdx.x % LANES_PER_ROW;
    const int g = sub >> 3, r = sub & 7;
    const uint32_t b0 = rowptr[gid], b1 = rowptr[gid + 1];
    A acc = 0;
    for (uint32_t b = b0 + g; b < b1; b += GROUPS) {
        uint64_t bmp = bmps[b];
        uint32_t byte = tile_byte(bmp, r);
        if (byte) {
            uint32_t before = r ? (uint32_t)__popcll(bmp >> (64 - 8 * r)) : 0u;  // values stored in rows above
            acc = tile_row_dot<T, A>(byte, values + offsets[b] + before, x, key_col(keys[b]) * 8u, num_cols, acc);
        }
    }
    if (GROUPS > 1) {
#pragma unroll
        for (int d = 8; d < LANES_PER_ROW; d <<= 1) acc += __shfl_xor(acc, d, kWave);
    }
    uint32_t row = gid * 8u + (uint32_t)r;
    if (g == 0 && row >= row_lo && row < num_rows) y[row] = acc;
}

// ---------------------------------------------------------------------------------------------------------
// row-group kernel (variant 3): matrices whose tiles are mostly dense (FEM / banded)
// ---------------------------------------------------------------------------------------------------------
// The sweep above is built for hyper-sparse tiles (a lane per TILE).  When a tile holds tens of values the bytes are in the value
// array, and the job is to stream it with 16-byte loads: here 16 lanes own one block-row (4 block-rows per wave) and walk its
// tiles; lane j of the group takes tile positions 4j .. 4j+3 (half a tile row): ONE 16-byte load of the <= 4 consecutive stored
// values behind rank(4j) -- the whole wave moves 1 KB of values per instruction when tiles are full -- against one 16-byte load
// of the four x entries (block column cached in L1/L2: neighbouring block-rows of a banded matrix read the same x lines).
// Partly filled nibbles are expanded with three selects, and the x entries of their unstored positions are selected to zero with four
// more (the sum is over the STORED entries: an Inf or NaN of x beside a stored column must not meet the expansion's 0); sums stay in
// registers for the whole block-row (no LDS, no atomics: y is bit-reproducible), the two half-rows meet in one DPP add, 8 lanes store
// the 8 rows.
template <typename T, int U>
__global__ __launch_bounds__(kThreads) void spmv_rowgroup_kernel(const uint32_t *__restrict__ rowptr, const uint64_t *__restrict__ keys,
                                                                 const uint64_t *__restrict__ bmps, const uint64_t *__restrict__ offsets,
                                                                 const T *__restrict__ values, const T *__restrict__ x,
                                                                 typename Acc<T>::type *__restrict__ y, uint32_t num_rows, uint32_t num_cols,
                                                                 uint32_t nbr, uint32_t values_bytes, uint32_t passes, uint32_t row_lo)
{
    using A = typename Acc<T>::type;
    const int lane = lane_id(), j = lane & 15, g = lane >> 4;
    const uint32_t wv = blockIdx.x * 4 + wave_id();
    const rsrc_t rv = make_rsrc(values, values_bytes), rx = make_rsrc(x, num_cols * (uint32_t)sizeof(T));
    const uint32_t xlane = (uint32_t)((j & 1) * 4);        // first of this lane's four tile columns
    const uint32_t bshift = (uint32_t)(60 - 4 * j) & 31u;   // nibble of positions 4j .. 4j+3 inside its bitmap word
    const bool in_hi = j < 8;
    const uint32_t hi_mask = j >= 8 ? 0xffffffffu : (j == 0 ? 0u : 0xffffffffu << (32 - 4 * j));  // bitmap bits of positions < 4j
    const uint32_t lo_mask = j > 8 ? 0xffffffffu << (64 - 4 * j) : 0u;
    const bool ragged_x = (num_cols & 3u) != 0u;
    for (uint32_t p = 0; p < passes; p++) {
        const uint32_t br = (wv * passes + p) * 4u + (uint32_t)g;
        if ((wv * passes + p) * 4u >= nbr) break;  // wave-uniform
        const bool valid = br < nbr;
        uint32_t t = valid ? rowptr[br] : 0u;
        const uint32_t t1 = valid ? rowptr[br + 1] : 0u;
        A acc = 0;
        // tile words of the first trip; inside the loop the NEXT trip's words are requested behind the current trip's value / x
        // loads, so a trip waits for one round trip (its values), not two
        uint32_t blo[U], bhi[U], col[U], off[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const bool on = t + u < t1;
            const uint64_t bm = on ? bmps[t + u] : 0ull;
            blo[u] = (uint32_t)bm; bhi[u] = (uint32_t)(bm >> 32);
            col[u] = on ? (uint32_t)keys[t + u] : 0u;
            off[u] = on ? (uint32_t)offsets[t + u] : 0u;
        }
        while (__any(t < t1)) {
            A av[U][4], xv[U][4];
            uint32_t nib[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                nib[u] = ((in_hi ? bhi[u] : blo[u]) >> bshift) & 0xfu;
                const uint32_t rank = (uint32_t)__builtin_popcount(bhi[u] & hi_mask) + (uint32_t)__builtin_popcount(blo[u] & lo_mask);
                const uint32_t vaddr = (off[u] + rank) * (uint32_t)sizeof(T);
                if (sizeof(T) == 2) {
                    // halves start at any even byte: fetch the enclosing dwords and funnel-shift the odd leading half away
                    typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
                    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
                    const u32x3 d = __builtin_amdgcn_raw_buffer_load_b96(rv, nib[u] ? (vaddr & ~3u) : kOob, 0, 0);
                    const uint32_t sh = (vaddr & 2u) * 8u;
                    const h2 p0 = __builtin_bit_cast(h2, __builtin_amdgcn_alignbit(d[1], d[0], sh)), p1 = __builtin_bit_cast(h2, __builtin_amdgcn_alignbit(d[2], d[1], sh));
                    av[u][0] = (A)p0[0]; av[u][1] = (A)p0[1]; av[u][2] = (A)p1[0]; av[u][3] = (A)p1[1];
                } else {
                    Buf4<T>::ld(rv, nib[u] ? vaddr : kOob, av[u]);
                }
                const uint32_t xc = col[u] * 8u + xlane;
                if (ragged_x && xc + 4u > num_cols) {  // a 16-byte load that leaves x reads as zero altogether: last block column only
#pragma unroll
                    for (int q = 0; q < 4; q++) xv[u][q] = (A)Buf<T>::ld(rx, nib[u] && xc + q < num_cols ? (xc + q) * (uint32_t)sizeof(T) : kOob);
                } else {
                    Buf4<T>::ld(rx, nib[u] ? xc * (uint32_t)sizeof(T) : kOob, xv[u]);
                }
            }
            uint32_t nlo[U], nhi[U], ncol[U], noff[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const bool on = t + U + u < t1;
                const uint64_t bm = on ? bmps[t + U + u] : 0ull;
                nlo[u] = (uint32_t)bm; nhi[u] = (uint32_t)(bm >> 32);
                ncol[u] = on ? (uint32_t)keys[t + U + u] : 0u;
                noff[u] = on ? (uint32_t)offsets[t + U + u] : 0u;
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint32_t n = nib[u];
                A e0, e1, e2, e3, x0 = xv[u][0], x1 = xv[u][1], x2 = xv[u][2], x3 = xv[u][3];
                if (__all(n == 0xfu || n == 0u)) {  // full (or absent) nibbles everywhere: values already sit at their positions
                    e0 = av[u][0]; e1 = av[u][1]; e2 = av[u][2]; e3 = av[u][3];
                    if (n == 0u) { e0 = e1 = e2 = e3 = A(0); }  // (its x was not loaded either: the out-of-range offset reads 0)
                } else {
                    // stored values of the nibble are consecutive: position q holds value number popc(bits before q).  An unstored
                    // position contributes nothing, whatever x holds there (bmsp.h: the sum is over the STORED entries): its x is
                    // selected to zero by the same bit as its value, so an Inf or NaN of x next to a stored column never meets a 0
                    const bool b0 = n & 8u, b1 = n & 4u, b2 = n & 2u, b3 = n & 1u;
                    const uint32_t i2 = (uint32_t)b0 + (uint32_t)b1, i3 = i2 + (uint32_t)b2;
                    e0 = b0 ? av[u][0] : A(0);
                    e1 = b1 ? (b0 ? av[u][1] : av[u][0]) : A(0);
                    e2 = b2 ? (i2 == 0 ? av[u][0] : (i2 == 1 ? av[u][1] : av[u][2])) : A(0);
                    e3 = b3 ? (i3 == 0 ? av[u][0] : (i3 == 1 ? av[u][1] : (i3 == 2 ? av[u][2] : av[u][3]))) : A(0);
                    x0 = b0 ? x0 : A(0); x1 = b1 ? x1 : A(0); x2 = b2 ? x2 : A(0); x3 = b3 ? x3 : A(0);
                }
                acc += e0 * x0 + e1 * x1 + e2 * x2 + e3 * x3;
            }
            t += U;
#pragma unroll
            for (int u = 0; u < U; u++) { blo[u] = nlo[u]; bhi[u] = nhi[u]; col[u] = ncol[u]; off[u] = noff[u]; }
        }
        // lanes 2r and 2r+1 hold the two halves of tile row r
        if (sizeof(A) == 4) acc += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (float)acc), 0xB1, 0xf, 0xf, false));  // quad_perm 1,0,3,2
        else acc += __shfl_xor(acc, 1, kWave);
        const uint32_t row = br * 8u + (uint32_t)(j >> 1);
        if (valid && !(j & 1) && row >= row_lo && row < num_rows) y[row] = acc;
    }
}

// ---------------------------------------------------------------------------------------------------------
// chunked sweep (round 5; the default for the value-stream matrices that fit its encoding, fp32)
// ---------------------------------------------------------------------------------------------------------
// The value-stream kernel spends most of a wave's life waiting on a chain of dependent round trips (item -> slot words / entries / values ->
// LDS slot table -> x gather).  Here the work is cut by STORED VALUES instead: chunk c is values [c*V, (c+1)*V) in storage order, cut
// anywhere (inside a tile, inside a block-row), one wave per chunk.  A per-matrix structure cache holds ONE 32-bit word per stored value,
// {row relative to the chunk's first block-row (high bits), column (low `colbits` bits)}, so that everything a wave loads first depends on
// blockIdx alone: its 32-byte record (scalar), its V words and its V values (lane l: values 8l .. 8l+7 of the chunk, two 16-byte loads of
// each).  The x gathers follow back to back -- one round trip, then the gathers, then the reduction:
//   * a chunk inside ONE block-row (hub block-rows: most of a graph's values) keeps eight register sums per lane, reduced by a halving
//     exchange (10 shuffles) into the eight row sums;
//   * any other chunk reduces by block-row in registers (chunk_seg_reduce: per-lane block-row sums, a DPP segmented scan across lanes) and
//     writes each block-row's 8 sums once, with plain stores, into an LDS window over the chunk's block-rows (kChWin rows at most).
// Every row is written once.  Chunk c owns the block-rows from its first one (exclusive when that block-row began in an earlier chunk) up to
// chunk c+1's first block-row -- empty block-rows included, written as zeros.  A block-row whose values lie in several chunks (ca .. cb) is
// folded through carry slots: chunk ca parks its 8 partial sums in its TAIL slot, chunks ca+1 .. cb in their HEAD slots; write-through (sc1)
// stores, drained vmcnt, one agent-scope arrival counter per folded block-row (indexed by ca); the last to arrive sums the slots in chunk
// order with sc1 loads, writes the 8 rows and resets the counter -- the protocol of the long items above, deterministic, no float atomics.
// Round 6 combined each lane's values by row before one ds_add_f32 per distinct row; since round 7 no LDS float add is left: ds_add_f32
// is paid per active lane and was the largest part of the time after the gathers (rounds 6 and 7).
#ifndef BMSP_CH_V
#define BMSP_CH_V 512
#endif
constexpr uint32_t kChV = BMSP_CH_V;        // stored values per chunk
constexpr int kChPer = (int)kChV / 64;      // ... per lane (consecutive)
static_assert(kChPer % 4 == 0, "a lane loads its values four at a time");
constexpr uint32_t kChWin = 1024;           // LDS row window of a chunk (4 KB): chunks whose block-rows span more rows take the old kernel
constexpr int64_t kChMinChunks = 128;       // fewer chunks than this: the value-stream kernel (a bound set by a pinned test, not by the timings)
enum { kChHead = 1, kChTail = 2 };

struct ChunkRec {             // 32 bytes, one scalar load
    uint32_t fb;              // block-row of the chunk's first value (base of the relative rows)
    uint32_t own_b, own_e;    // block-rows [own_b, own_e) are written by this chunk alone
    uint32_t flags;           // kChHead: block-row fb continues from earlier chunks; kChTail: the last block-row continues into later ones
    uint32_t head_ca, head_cb;  // chunks of the head block-row
    uint32_t tail_cb;           // last chunk of the tail block-row (its first is this chunk)
    uint32_t nwin;              // rows of the window: 8 x (block-rows from the first to the last value)
};

// the halving exchange: lane l ends with the wave sum of s[k], k = 4*bit5 + 2*bit4 + bit3 of l
__device__ __forceinline__ float chunk_sum8(const float (&s)[8], int lane)
{
    const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
    float t[4], u[2];
#pragma unroll
    for (int i = 0; i < 4; i++) t[i] = (h5 ? s[i + 4] : s[i]) + __shfl_xor(h5 ? s[i] : s[i + 4], 32, kWave);
#pragma unroll
    for (int i = 0; i < 2; i++) u[i] = (h4 ? t[i + 2] : t[i]) + __shfl_xor(h4 ? t[i] : t[i + 2], 16, kWave);
    float v = (h3 ? u[1] : u[0]) + __shfl_xor(h3 ? u[0] : u[1], 8, kWave);
    v += __shfl_xor(v, 4, kWave);
    v += __shfl_xor(v, 2, kWave);
    v += __shfl_xor(v, 1, kWave);
    return v;
}

__device__ __forceinline__ void chunk_put8(float *p, const float (&v)[8])
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    *(f4 *)p = f4{v[0], v[1], v[2], v[3]};
    *(f4 *)(p + 4) = f4{v[4], v[5], v[6], v[7]};
}

// one step of wave_run_sum over eight sums at once: a lane whose DPP source lane holds the same key adds that lane's sums; false (and
// nothing done) when no lane of the wave does -- keys are non-decreasing, so no later in-row step would either
template <int CTRL, int ROWS>
__device__ __forceinline__ bool chunk_scan_step(float (&t)[8], uint32_t key)
{
    const bool m = dpp_u32<CTRL, ROWS>(~0u, key) == key;
    if (!__builtin_amdgcn_ballot_w64(m)) return false;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const float n = t[k] + dpp_val<CTRL, ROWS>(0.f, t[k]);
        t[k] = m ? n : t[k];
    }
    return true;
}

// the reduction of a chunk over several block-rows (round 7): rk[] are rows relative to the chunk's first block-row, their block-rows
// (rk >> 3) non-decreasing across a lane's values and across lanes; win is zero-filled (empty block-rows).  Every block-row present is
// written once, as its 8 row sums, with plain LDS stores by the lane where it ends: no LDS float atomics.
//   in-lane: 8 register sums for the current block-row; where the block-row changes they become the lane's head (its first block-row)
//     or, for a block-row that begins and ends in the lane, go straight to the window; what is left is the lane's tail (last block-row);
//   cross-lane: an inclusive segmented scan of the tail sums keyed by the tail block-row (row_shr inside rows of 16, then row_bcast), and
//     a head that continues the left lane's tail block-row adds that lane's scanned sums.
// The sums run in a fixed order (storage order inside a lane, then the scan's fixed tree), so y is reproducible bit for bit.
__device__ __forceinline__ void chunk_seg_reduce(float *win, const uint32_t (&rk)[kChPer], const float (&pr)[kChPer])
{
    const uint32_t bf = rk[0] >> 3, bl = rk[kChPer - 1] >> 3;
    float h[8], t[8];
#pragma unroll
    for (int k = 0; k < 8; k++) h[k] = t[k] = 0.f;
#pragma unroll
    for (int j = 0; j < kChPer; j++) {
        if (j > 0 && (rk[j] >> 3) != (rk[j - 1] >> 3)) {
            const uint32_t bp = rk[j - 1] >> 3;
            if (bp == bf) {
#pragma unroll
                for (int k = 0; k < 8; k++) h[k] = t[k];
            } else {
                chunk_put8(win + 8u * bp, t);
            }
#pragma unroll
            for (int k = 0; k < 8; k++) t[k] = 0.f;
        }
        const uint32_t r = rk[j] & 7u;
#pragma unroll
        for (int k = 0; k < 8; k++) t[k] += r == (uint32_t)k ? pr[j] : 0.f;
    }
    if (chunk_scan_step<0x111, 0xf>(t, bl) && chunk_scan_step<0x112, 0xf>(t, bl) && chunk_scan_step<0x114, 0xf>(t, bl)) chunk_scan_step<0x118, 0xf>(t, bl);
    chunk_scan_step<0x142, 0xa>(t, bl);  // row_bcast:15 into rows 1 and 3
    chunk_scan_step<0x143, 0xc>(t, bl);  // row_bcast:31 into rows 2 and 3
    const uint32_t bl_left = dpp_u32<0x138>(~0u, bl), bf_right = dpp_u32<0x130>(~0u, bf);  // wave_shr:1, wave_shl:1
    float tl[8];
#pragma unroll
    for (int k = 0; k < 8; k++) tl[k] = dpp_val<0x138>(0.f, t[k]);
    if (bf != bl) {
        const bool cont = bl_left == bf;
#pragma unroll
        for (int k = 0; k < 8; k++) h[k] = cont ? h[k] + tl[k] : h[k];
        chunk_put8(win + 8u * bf, h);
    }
    if (bf_right != bl) chunk_put8(win + 8u * bl, t);
}

// U slots per lane of the fold, chunks kb + g, kb + g + 8, ... (those past cb load slot cb again and add 0): every load issued before the
// first wait (a load under a per-element condition would be branched around and waited for one by one)
template <int U>
__device__ __forceinline__ float chunk_fold_batch(const float *__restrict__ carry, uint32_t ca, uint32_t kb, uint32_t cb, uint32_t r, uint32_t g)
{
    float v[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t k = min(kb + g + 8u * (uint32_t)u, cb);
        v[u] = __hip_atomic_load(&carry[((size_t)k * 2 + (k == ca ? 1 : 0)) * 8 + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < U; u++) s += kb + g + 8u * (uint32_t)u <= cb ? v[u] : 0.f;
    return s;
}

// the last of chunks ca .. cb to arrive: slot (ca, tail) + slots (ca+1 .. cb, head).  Lane (row r = lane / 8, group g = lane % 8) sums
// the slots of chunks ca + g + 8i, up to 32 chunks per batch of loads in flight (round 8: the old loop waited for each load), then the
// 8 groups of a row combine by DPP (row_shr 1, 2, 4: lane 8r + 7 ends with the row sum).  The order is fixed by ca and cb alone, so
// repeated sweeps are bitwise equal.
__device__ __forceinline__ void chunk_fold(const float *__restrict__ carry, float *__restrict__ y, uint32_t *__restrict__ counters, uint32_t ca,
                                           uint32_t cb, uint32_t br, uint32_t num_rows, int lane)
{
    const uint32_t r = (uint32_t)lane >> 3, g = (uint32_t)lane & 7u, n = cb - ca + 1u;
    float sum;
    if (n <= 8u) {
        sum = chunk_fold_batch<1>(carry, ca, ca, cb, r, g);
    } else if (n <= 16u) {
        sum = chunk_fold_batch<2>(carry, ca, ca, cb, r, g);
    } else {
        sum = 0.f;
        for (uint32_t kb = ca; kb <= cb; kb += 32u) sum += chunk_fold_batch<4>(carry, ca, kb, cb, r, g);
    }
    sum += dpp_val<0x111>(0.f, sum);  // row_shr:1
    sum += dpp_val<0x112>(0.f, sum);  // row_shr:2
    sum += dpp_val<0x114>(0.f, sum);  // row_shr:4
    const uint32_t row = br * 8u + r;
    if (g == 7u && row < num_rows) y[row] = sum;
    if (lane == 0) __hip_atomic_store(&counters[ca], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the row-sorted form (round 9, layout 2; colbits <= kChSortedColbits) ----
// Which values of a chunk share a row is fixed per matrix, so the cache build (chunk_sort_kernel) groups them once: the chunk's 512 words
// are stored in ROW order (positions sorted by row, ties in storage order), and word p holds
//   bits 0 .. colbits-1  the column of the value at position p
//   next 9               its storage index inside the chunk (values[512 c + idx])
//   next 1               start: position p begins a new row (p = 0: always)
//   next 2               bits 2p and 2p+1 of the chunk's window bitmap (bit e: row 8 fb + e has a value in this chunk; 1024 bits)
// -- the same 4 bytes per stored value.  Positions past nnz (last chunk) are 0 apart from their bitmap bits: they continue the last run and
// add an exact +0 (no x read).  The sweep is left with ONE sum per lane: products in row order, a sequential segmented sum in the lane, the
// wave_run_sum steps on one float across lanes, and every run's last position stores the run total to T[run rank].  Row e of the window is
// T[number of bitmap bits below e] when bit e is set, else 0: no zero-filled window, no per-block-row sums.
constexpr int kChSortedColbits = 20;           // 20 + 9 + 1 + 2 = 32 bits
constexpr uint32_t kChT = kChV + 64;           // run totals, then one dump slot per lane (positions that end no run store there)
constexpr uint32_t kChSortedLds = kChT + 64;   // ... | 32 bitmap words | 32 counts of bits below each word
static_assert(kChSortedLds * 4 <= 6144, "the row-sorted form keeps to 6 KB of LDS per wave");

__device__ __forceinline__ float chunk_row_value(const float *T, const uint32_t *bmw, const uint32_t *pre, uint32_t e)
{
    const uint32_t wd = bmw[e >> 5], sh = e & 31u;
    const float v = T[pre[e >> 5] + (uint32_t)__popc(wd & ((1u << sh) - 1u))];  // <= kChV (the first dump slot) when bit e is clear
    return (wd >> sh) & 1u ? v : 0.f;
}

// one chunk of the row-sorted form, up to the row sums: on return T, the bitmap words and their prefix counts are in lds.  WHOLE: the chunk
// holds kChV values (every chunk but the last) -- 16-byte value loads and no bound on the positions; the two cases are separate code so
// that the gathers of the common one wait for the words alone.  lds: first the values in storage order, then (the same floats) T.
template <bool WHOLE>
__device__ __forceinline__ void chunk_sorted_reduce(float *lds, const uint32_t *__restrict__ words, const float *__restrict__ values,
                                                    const float *__restrict__ x, uint32_t c, uint32_t nnz, uint32_t num_cols, uint32_t colbits, int lane)
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const uint32_t first = c * kChV + (uint32_t)(kChPer * lane), nval = WHOLE ? kChV : nnz - c * kChV;
    // the words are padded to whole chunks (the padding carries bitmap bits): always 16-byte loads, both requested before the values
    const rsrc_t rw = make_rsrc(words, (uint32_t)min((uint64_t)gridDim.x * kChV * 4u, (uint64_t)0xfffffffcu));
    const rsrc_t rv = make_rsrc(values, nnz * 4u), rx = make_rsrc(x, num_cols * 4u);
    uint32_t w[kChPer];
    float a[kChPer], xv[kChPer];
#pragma unroll
    for (int q = 0; q < kChPer; q += 4) {
        const u4 wq = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(rw, (first + q) * 4u, 0, 0));
#pragma unroll
        for (int i = 0; i < 4; i++) w[q + i] = wq[i];
    }
    if constexpr (WHOLE) {
#pragma unroll
        for (int q = 0; q < kChPer; q += 4) {
            const f4 aq = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rv, (first + q) * 4u, 0, 0));
#pragma unroll
            for (int i = 0; i < 4; i++) a[q + i] = aq[i];
        }
    } else {  // element loads, values past nnz read 0
#pragma unroll
        for (int j = 0; j < kChPer; j++) a[j] = Buf<float>::ld(rv, first + j < nnz ? (first + j) * 4u : kOob);
    }
    const uint32_t cmask = (1u << colbits) - 1u;
#pragma unroll
    for (int j = 0; j < kChPer; j++) xv[j] = Buf<float>::ld(rx, WHOLE || (uint32_t)(kChPer * lane + j) < nval ? (w[j] & cmask) * 4u : kOob);
    float *T = lds;
    uint32_t *bmw = (uint32_t *)(lds + kChT), *pre = bmw + 32;
    chunk_put8(T + kChPer * lane, a);
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < kChPer; j++) bits |= (w[j] >> (colbits + 10u)) << (2 * j);
    ((uint16_t *)bmw)[lane] = (uint16_t)bits;
    __builtin_amdgcn_wave_barrier();
    float pr[kChPer];
#pragma unroll
    for (int j = 0; j < kChPer; j++) pr[j] = T[(w[j] >> colbits) & (kChV - 1u)];
    {
        const uint32_t wd = lane < 32 ? bmw[lane] : 0u, pc = (uint32_t)__popc(wd);
        const uint32_t below = wave_inclusive_sum_dpp(pc) - pc;
        if (lane < 32) pre[lane] = below;
    }
    // run rank of every position: starts up to and including it, minus one
    uint32_t st[kChPer], k[kChPer], tot = 0;
#pragma unroll
    for (int j = 0; j < kChPer; j++) {
        st[j] = (w[j] >> (colbits + 9u)) & 1u;
        tot += st[j];
        k[j] = tot;
    }
    const uint32_t base = wave_inclusive_sum_dpp(tot) - tot - 1u;
#pragma unroll
    for (int j = 0; j < kChPer; j++) {
        k[j] += base;
        pr[j] = WHOLE || (uint32_t)(kChPer * lane + j) < nval ? pr[j] * xv[j] : 0.f;
    }
    // the lane's last run, summed across the lanes it covers (lanes with the same last run: its first lane, then lanes without a start)
    float t = pr[0];
#pragma unroll
    for (int j = 1; j < kChPer; j++) t = st[j] ? pr[j] : t + pr[j];
    const float run = wave_run_sum(t, k[kChPer - 1]);
    const float left = dpp_val<0x138>(0.f, run);                // wave_shr:1
    const uint32_t st_right = dpp_u32<0x130>(1u, st[0]);        // wave_shl:1; the last position of the chunk ends its run
    __builtin_amdgcn_wave_barrier();                            // every lane has read its values: the staging area becomes T
    const uint32_t dump = kChV + (uint32_t)lane;
    float acc = st[0] ? pr[0] : left + pr[0];                   // positions before the lane's first start continue the left lane's run
#pragma unroll
    for (int j = 1; j < kChPer; j++) {
        T[st[j] ? (k[j - 1] & (kChV - 1u)) : dump] = acc;
        acc = st[j] ? pr[j] : acc + pr[j];
    }
    T[st_right ? (k[kChPer - 1] & (kChV - 1u)) : dump] = acc;
}

template <bool SORTED>
__global__ __launch_bounds__(64, 8) void spmv_chunk_kernel(const ChunkRec *__restrict__ recs, const uint32_t *__restrict__ words,
                                                            const float *__restrict__ values, const float *__restrict__ x, float *__restrict__ y,
                                                            float *__restrict__ carry, uint32_t *__restrict__ counters, uint32_t nnz,
                                                            uint32_t num_rows, uint32_t num_cols, uint32_t colbits)
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) float win[SORTED ? kChSortedLds : kChWin];
    const int lane = lane_id();
    const uint32_t c = blockIdx.x;
    const ChunkRec rc = recs[c];
    if constexpr (SORTED) {
        if (c * kChV + kChV <= nnz) chunk_sorted_reduce<true>(win, words, values, x, c, nnz, num_cols, colbits, lane);
        else chunk_sorted_reduce<false>(win, words, values, x, c, nnz, num_cols, colbits, lane);
    } else {
        const uint32_t first = c * kChV + (uint32_t)(kChPer * lane);
        const rsrc_t rw = make_rsrc(words, nnz * 4u), rv = make_rsrc(values, nnz * 4u), rx = make_rsrc(x, num_cols * 4u);
        uint32_t w[kChPer];
        float a[kChPer], xv[kChPer];
        if (c * kChV + kChV <= nnz) {  // a whole chunk: 16-byte loads
#pragma unroll
            for (int q = 0; q < kChPer; q += 4) {
                const u4 wq = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(rw, (first + q) * 4u, 0, 0));
                const f4 aq = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rv, (first + q) * 4u, 0, 0));
#pragma unroll
                for (int i = 0; i < 4; i++) { w[q + i] = wq[i]; a[q + i] = aq[i]; }
            }
        } else {  // the last chunk: element loads, values past nnz read 0
#pragma unroll
            for (int j = 0; j < kChPer; j++) {
                const uint32_t off = first + j < nnz ? (first + j) * 4u : kOob;
                w[j] = __builtin_amdgcn_raw_buffer_load_b32(rw, off, 0, 0);
                a[j] = Buf<float>::ld(rv, off);
            }
        }
        const uint32_t cmask = (1u << colbits) - 1u;
#pragma unroll
        for (int j = 0; j < kChPer; j++) xv[j] = Buf<float>::ld(rx, first + j < nnz ? (w[j] & cmask) * 4u : kOob);

        float pr[kChPer];
        uint32_t rr[kChPer];
#pragma unroll
        for (int j = 0; j < kChPer; j++) {
            rr[j] = first + j < nnz ? w[j] >> colbits : rc.nwin - 8u;  // past nnz (last chunk only): the last block-row, adding 0
            pr[j] = first + j < nnz ? a[j] * xv[j] : 0.f;
        }
        if (rc.nwin == 8) {
            // one block-row: eight register sums per lane
            float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < kChPer; j++) {
#pragma unroll
                for (int k = 0; k < 8; k++) s[k] += rr[j] == (uint32_t)k ? pr[j] : 0.f;
            }
            const float v = chunk_sum8(s, lane);
            if ((lane & 7) == 0) win[((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1)] = v;
        } else {
            for (uint32_t e = (uint32_t)lane; e < rc.nwin; e += 64) win[e] = 0.f;
            __builtin_amdgcn_wave_barrier();
            chunk_seg_reduce(win, rr, pr);
        }
    }
    __builtin_amdgcn_wave_barrier();
    // the sum of row `rel` of the window (rel < nwin)
    const auto row_sum = [&](uint32_t rel) -> float {
        if constexpr (SORTED) return chunk_row_value(win, (const uint32_t *)(win + kChT), (const uint32_t *)(win + kChT) + 32, rel);
        else return win[rel];
    };
    // folded block-rows: park the 8 partial sums, drain them, then take both tickets with ONE returning atomic -- lanes 0 (head) and 1
    // (tail) at lane-dependent addresses; two uniform-address atomics were each rewritten into a wave-reduced atomic and waited for in
    // turn (round 8).  The own-row y stores go out behind the ticket and overlap its round trip.
    uint32_t ticket = 0;
    if (rc.flags) {
        if ((rc.flags & kChHead) && lane < 8) __hip_atomic_store(&carry[((size_t)c * 2) * 8 + lane], row_sum((uint32_t)lane), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((rc.flags & kChTail) && lane < 8)
            __hip_atomic_store(&carry[((size_t)c * 2 + 1) * 8 + lane], row_sum(rc.nwin - 8u + (uint32_t)lane), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0 ? (rc.flags & kChHead) != 0u : lane == 1 && (rc.flags & kChTail) != 0u)
            ticket = __hip_atomic_fetch_add(&counters[lane == 0 ? rc.head_ca : c], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // the block-rows this chunk owns (rows before the first value -- chunk 0 -- and after the last are zeros)
    const int32_t base = (int32_t)(rc.fb * 8u);
    const uint32_t row_end = min(rc.own_e * 8u, num_rows);
    for (uint32_t row = rc.own_b * 8u + (uint32_t)lane; row < row_end; row += 64) {
        const int32_t rel = (int32_t)row - base;
        const bool in = rel >= 0 && rel < (int32_t)rc.nwin;
        if constexpr (SORTED) {
            const float v = row_sum(in ? (uint32_t)rel : 0u);
            y[row] = in ? v : 0.f;
        } else {
            y[row] = in ? win[rel] : 0.f;
        }
    }
    if (!rc.flags) return;
    const uint32_t th = (uint32_t)__builtin_amdgcn_readlane((int)ticket, 0), tt = (uint32_t)__builtin_amdgcn_readlane((int)ticket, 1);
    if ((rc.flags & kChHead) && th == rc.head_cb - rc.head_ca) chunk_fold(carry, y, counters, rc.head_ca, rc.head_cb, rc.fb, num_rows, lane);
    if ((rc.flags & kChTail) && tt == rc.tail_cb - c) chunk_fold(carry, y, counters, c, rc.tail_cb, rc.fb + rc.nwin / 8u - 1u, num_rows, lane);
}

// cache build, pass 1: block-row of every chunk's first and last value
__global__ void chunk_bounds_kernel(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ bmps, const uint64_t *__restrict__ offsets,
                                    uint32_t nb, uint32_t nnz, uint32_t *__restrict__ fbr, uint32_t *__restrict__ lbr)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const uint32_t o = (uint32_t)offsets[b], n = (uint32_t)__popcll(bmps[b]);
    if (n == 0) return;
    const uint32_t br = key_row(keys[b]);
    for (uint32_t c = (o + kChV - 1) / kChV; c * kChV < o + n; c++) fbr[c] = br;
    for (uint32_t c = o / kChV; c <= (o + n - 1) / kChV; c++) {
        const uint32_t e = min((c + 1) * kChV, nnz) - 1u;
        if (e >= o && e < o + n) lbr[c] = br;
    }
}

// pass 2: the value words
__global__ void chunk_words_kernel(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ bmps, const uint64_t *__restrict__ offsets,
                                   uint32_t nb, const uint32_t *__restrict__ fbr, uint32_t colbits, uint32_t *__restrict__ words)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    uint64_t bm = bmps[b];
    const uint64_t k = keys[b];
    const uint32_t br = key_row(k), bc = key_col(k);
    uint32_t idx = (uint32_t)offsets[b];
    while (bm) {
        const uint32_t p = (uint32_t)__clzll((long long)bm);
        bm &= ~(0x8000000000000000ull >> p);
        const uint32_t rel = (br - fbr[idx / kChV]) * 8u + (p >> 3);
        words[idx] = (rel << colbits) | (bc * 8u + (p & 7u));
        idx++;
    }
}

// pass 3 (row-sorted form only), one workgroup per chunk, in place: the round-7 words {relative row, column} in storage order become the
// row-ordered words of layout 2.  A value's position is the number of the chunk's values with a smaller (row, storage index) -- counted,
// not ranked by atomics, so the same structure always gives the same words (the bitmap is an OR: order-free).
__global__ __launch_bounds__(kChV) void chunk_sort_kernel(uint32_t *__restrict__ words, uint32_t nnz, uint32_t colbits)
{
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) uint32_t keys[kChV];
    __shared__ uint32_t out[kChV], srow[kChV], bm[kChWin / 32];
    const uint32_t c = blockIdx.x, i = threadIdx.x, n = min(nnz - c * kChV, kChV);
    const uint32_t w = words[(size_t)c * kChV + i];
    const uint32_t r = w >> colbits, key = i < n ? (r << 9) | i : ~0u;  // r < kChWin: 19 bits; the padding sorts last
    keys[i] = key;
    out[i] = 0;
    srow[i] = ~0u;
    if (i < kChWin / 32) bm[i] = 0;
    __syncthreads();
    if (i < n) {
        uint32_t pos = 0;
        for (uint32_t j = 0; j < kChV / 4; j++) {
            const u4 q = ((const u4 *)keys)[j];
            pos += (q[0] < key ? 1u : 0u) + (q[1] < key ? 1u : 0u) + (q[2] < key ? 1u : 0u) + (q[3] < key ? 1u : 0u);
        }
        out[pos] = (w & ((1u << colbits) - 1u)) | (i << colbits);
        srow[pos] = r;
        atomicOr(&bm[(r >> 5) & (kChWin / 32 - 1)], 1u << (r & 31u));
    }
    __syncthreads();
    const uint32_t start = i < n && (i == 0 || srow[i] != srow[i - 1]) ? 1u : 0u;
    words[(size_t)c * kChV + i] = out[i] | (start << (colbits + 9u)) | (((bm[i >> 4] >> ((2u * i) & 31u)) & 3u) << (colbits + 10u));
}

// the chunked sweep's cache: built once per matrix (bmsp_matrix_prepare or the first sweep); nothing is kept for a matrix it does not fit
void build_chunk_cache(bmsp_matrix_s *A, hipStream_t st)
{
    if (A->spmv_cw || A->spmv_cw_tried) return;
    A->spmv_cw_tried = 1;
    if (A->dtype != BMSP_F32 || A->view_values_end || A->view_block_begin || A->nnz == 0 || A->nnz >= (1ll << 30) || A->block_num == 0) return;
    if ((uintptr_t)A->values & 15u) return;  // 16-byte value loads
    const uint32_t nnz = (uint32_t)A->nnz, nb = (uint32_t)A->block_num;
    const uint32_t nch = (nnz + kChV - 1) / kChV;
    const int colbits = A->num_cols <= 1 ? 1 : 32 - __builtin_clz((uint32_t)A->num_cols - 1u);
    if (colbits > 28) return;
    // the row-sorted words need 9 bits of storage index, the start bit and 2 bitmap bits above the column (BMSP_SPMV_CHUNK_SORTED=0: round 7)
    const char *se = getenv("BMSP_SPMV_CHUNK_SORTED");
    const bool sorted = kChV == 512 && kChWin == 1024 && colbits <= kChSortedColbits && !(se && atoi(se) == 0);
    std::vector<uint32_t> fb(nch), lb(nch);
    {
        DevBuf<uint32_t> d(2 * (size_t)nch);
        hipLaunchKernelGGL(chunk_bounds_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, A->keys, A->bmps, A->offsets, nb, nnz, d.p, d.p + nch);
        BMSP_CHECK_LAUNCH();
        BMSP_HIP(hipStreamSynchronize(st));
        copy_d2h_staged(fb.data(), d.p, 4 * (size_t)nch);
        copy_d2h_staged(lb.data(), d.p + nch, 4 * (size_t)nch);
    }
    // records; a chunk whose block-rows do not fit the window (or the row field) sends the whole matrix to the old kernel
    const uint64_t row_cap = std::min<uint64_t>(kChWin, 1ull << (32 - colbits));
    std::vector<ChunkRec> rec(nch);
    const uint32_t nbr = (uint32_t)A->num_block_rows();
    int64_t split = 0;
    for (uint32_t c = 0; c < nch; c++) {
        ChunkRec &r = rec[c];
        r.fb = fb[c];
        r.nwin = (lb[c] - fb[c] + 1u) * 8u;
        if (lb[c] < fb[c] || r.nwin > row_cap) return;
        const bool head = c > 0 && lb[c - 1] == fb[c], tail = c + 1 < nch && fb[c + 1] == lb[c];
        r.own_b = c == 0 ? 0u : fb[c] + (head ? 1u : 0u);
        r.own_e = c + 1 < nch ? fb[c + 1] : nbr;
        r.flags = (head ? kChHead : 0) | (tail && !(head && fb[c] == lb[c]) ? kChTail : 0);
        r.head_ca = r.head_cb = r.tail_cb = c;
    }
    // chunk ranges of the folded block-rows
    for (uint32_t c = 0; c < nch; c++) {
        if (!(rec[c].flags & kChTail)) continue;
        split++;
        uint32_t e = c + 1;
        while (e + 1 < nch && fb[e + 1] == lb[c]) e++;
        rec[c].tail_cb = e;
        for (uint32_t k = c + 1; k <= e; k++) { rec[k].head_ca = c; rec[k].head_cb = e; }
    }
    // one allocation: words (whole chunks) | records | counters | carry (2 slots x 8 rows per chunk)
    const size_t off_rec = (size_t)nch * kChV * 4, off_cnt = off_rec + sizeof(ChunkRec) * (size_t)nch;
    const size_t off_carry = (off_cnt + 4 * (size_t)nch + 63) & ~size_t(63), total = off_carry + 64 * (size_t)nch;
    char *mem = (char *)pool_alloc(total);
    BMSP_HIP(hipMemsetAsync(mem, 0, total, st));
    BMSP_HIP(hipMemcpyAsync(mem + off_rec, rec.data(), sizeof(ChunkRec) * (size_t)nch, hipMemcpyHostToDevice, st));
    {
        DevBuf<uint32_t> d(nch);
        BMSP_HIP(hipMemcpyAsync(d.p, fb.data(), 4 * (size_t)nch, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(chunk_words_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, A->keys, A->bmps, A->offsets, nb, d.p, (uint32_t)colbits, (uint32_t *)mem);
        BMSP_CHECK_LAUNCH();
        if (sorted) {
            hipLaunchKernelGGL(chunk_sort_kernel, dim3(nch), dim3(kChV), 0, st, (uint32_t *)mem, nnz, (uint32_t)colbits);
            BMSP_CHECK_LAUNCH();
        }
        BMSP_HIP(hipStreamSynchronize(st));  // the host records and the staging buffer go away with this scope
    }
    A->spmv_cw.adopt((uint32_t *)mem);
    A->spmv_cw_layout = sorted ? 2 : 1;
    A->spmv_cw_chunks = nch;
    A->spmv_cw_split = split;
    A->spmv_cw_off_rec = off_rec; A->spmv_cw_off_cnt = off_cnt; A->spmv_cw_off_carry = off_carry;
    A->spmv_cw_colbits = colbits;
}

// ---------------------------------------------------------------------------------------------------------
// which kernel runs: decided in ONE place, for the launcher, bmsp_spmv_launch_info, bmsp_spmv_chunk_layout and bmsp_matrix_prepare
// ---------------------------------------------------------------------------------------------------------
// choose() walks this table from the top and takes the first row whose condition holds; it builds the caches of that row:
//   path            condition                                                                              caches read
//   none            no block-row                                                                           -
//   block-row 64    variant 1 ("batched")                                                                  block-row pointer
//   block-row 8     variant 2                                                                              block-row pointer
//   block-row 64    values or x beyond the 4 GiB a buffer descriptor addresses                             block-row pointer
//   row-group       variant 3; or variant 0 with >= 16 values per tile, no hub block-row and the kernel    block-row pointer (the plan is built
//                   not switched off -- either way only on values from this library's allocator            for its count of hub block-rows)
//   chunk           vstream_eligible, chunk_wanted, and the chunk cache fits the matrix                     chunk cache
//   value-stream    vstream_eligible (mostly sparse tiles; red: kAtomic below 2 values per tile)            plan, position cache (kCached;
//                                                                                                          kDecode where it was not built)
//   sweep           the rest: <FULL> with a quarter of the tiles full, else the round-1 kernel             plan
// The environment switches that steer the choice are read here (and in vstream_eligible / chunk_wanted, which only choose() and the plan
// builder call), each at most once per call.
enum class SpmvPath { kNone, kBlockRow64, kBlockRow8, kRowGroup, kChunk, kVstream, kSweep };
enum class SweepKind { kFull, kPlain, kNT, kPersist };

struct SpmvChoice {  // the path, the name bmsp_spmv_launch_info reports for it, and what its launch needs beyond the handle
    SpmvPath path = SpmvPath::kNone;
    const char *name = "none (empty matrix)";
    bool cached = false; int red = kAtomic;  // value-stream: entries from the position cache (kCached) or decoded in the kernel; kAtomic / kSorted
    int layout = 0;                          // chunk: 1 = words in storage order (round 7), 2 = row-sorted words
    uint32_t passes = 1;                     // row-group: block-row groups per wave
    SweepKind sweep = SweepKind::kPlain; int occ = 0; uint32_t grid = 0;  // sweep: the instantiation, which BMSP_SPMV_OCC=6 / 8 replaces by the one
                                                                          // bound to that occupancy; workgroups (BMSP_SPMV_PERSIST caps them)
};
const char *path_name(const SpmvChoice &c) { return c.name; }

// buffer descriptors address 4 GiB; a matrix whose values or x reach beyond goes to the pointer-based block-row kernel
bool beyond_descriptors(const bmsp_matrix_s *A)
{
    const size_t es = dtype_size(A->dtype);
    return (size_t)A->values_extent() * es >= (1ull << 32) || (size_t)A->num_cols * es >= (1ull << 32);
}

// the chunked sweep takes (A, rows): variant 0, fp32, the whole matrix (no row range, no view), the value-stream kernel not asked for
// (red_forced: BMSP_SPMV_RED is set), and (unless BMSP_SPMV_CHUNK=1 asks for it) fewer than 2 values per tile -- the run adds into LDS lose
// to the value-stream kernel's counting sort on denser tiles (FEM-like 3.7 / tile 42.1 vs 28.6 us, cage-like 3.2 / tile 58.4 vs 56.6) --
// and at least kChMinChunks chunks.  The cache must also fit (build_chunk_cache).
bool chunk_wanted(const bmsp_matrix_s *A, uint32_t row_lo, uint32_t row_hi, bool red_forced)
{
    if (A->dtype != BMSP_F32 || row_lo != 0 || row_hi != (uint32_t)A->num_rows || A->view_values_end || A->view_block_begin) return false;
    if (getenv("BMSP_SPMV_NOCHUNK") || getenv("BMSP_SPMV_NO_POSCACHE") || red_forced) return false;
    if (getenv("BMSP_SPMV_CHUNK")) return true;
    return A->nnz < 2 * A->block_num && (A->nnz + kChV - 1) / kChV >= kChMinChunks;
}

SpmvChoice choose(bmsp_matrix_s *A, int variant, uint32_t row_lo, uint32_t row_hi, hipStream_t st)
{
    SpmvChoice c;
    const auto take = [&c](SpmvPath path, const char *name) { c.path = path; c.name = name; return c; };
    const uint32_t nbr = (uint32_t)A->num_block_rows();
    if (nbr == 0) return c;
    if (variant == BMSP_SPMV_BATCHED) return take(SpmvPath::kBlockRow64, "spmv_blockrow_kernel<64 lanes per block-row>");
    if (variant == 2) return take(SpmvPath::kBlockRow8, "spmv_blockrow_kernel<8 lanes per block-row>");
    if (beyond_descriptors(A)) return take(SpmvPath::kBlockRow64, "spmv_blockrow_kernel<64 lanes per block-row>");
    build_plan(A, st);
    // dense tiles and no hub block-row: the row-group kernel streams the value array with 16-byte loads (variant 3); the 16-byte
    // value loads may run 12 bytes past the last stored value: arrays from this library's allocator carry that slack
    const bool dense_tiles = A->block_num > 0 && A->nnz >= 16 * A->block_num;
    if ((variant == 3 || (variant == BMSP_SPMV_DEFAULT && dense_tiles && A->spmv_plan_long == 0 && !getenv("BMSP_SPMV_NO_ROWGROUP"))) && pool_owns(A->values)) {
        const char *pe = getenv("BMSP_SPMV_PASSES");
        c.passes = pe ? (uint32_t)std::max(1, atoi(pe)) : ((nbr + 3) / 4 > 32768 ? 2u : 1u);
        return take(SpmvPath::kRowGroup, "spmv_rowgroup_kernel");
    }
    if (vstream_eligible(A)) {
        const char *re = getenv("BMSP_SPMV_RED");
        if (chunk_wanted(A, row_lo, row_hi, re != nullptr)) {
            build_chunk_cache(A, st);
            if (A->spmv_cw) { c.layout = A->spmv_cw_layout; return take(SpmvPath::kChunk, "spmv_chunk_kernel"); }
        }
        build_pos_cache(A, st);
        c.cached = A->spmv_pos != nullptr;
        c.red = re ? atoi(re) : (A->nnz < 2 * A->block_num ? kAtomic : kSorted);
        return take(SpmvPath::kVstream, c.cached ? (c.red == kAtomic ? "spmv_vstream_kernel<kCached, kAtomic>" : "spmv_vstream_kernel<kCached, kSorted>")
                                                 : (c.red == kAtomic ? "spmv_vstream_kernel<kDecode, kAtomic>" : "spmv_vstream_kernel<kDecode, kSorted>"));
    }
    const char *nt = getenv("BMSP_SPMV_NT"), *pers = getenv("BMSP_SPMV_PERSIST"), *occ = getenv("BMSP_SPMV_OCC");
    const uint32_t n_items = (uint32_t)A->spmv_num_chunks;
    c.sweep = A->spmv_full_tiles * 4 >= A->block_num ? SweepKind::kFull : (nt ? SweepKind::kNT : (pers ? SweepKind::kPersist : SweepKind::kPlain));
    c.occ = occ ? atoi(occ) : 0;
    c.grid = pers ? std::min<uint32_t>((n_items + 3) / 4, (uint32_t)atoi(pers)) : (n_items + 3) / 4;
    return take(SpmvPath::kSweep, c.sweep == SweepKind::kFull ? "spmv_sweep_kernel<FULL>" : "spmv_sweep_kernel");  // (NT / PERSIST / OCC: the plain name)
}

// ---------------------------------------------------------------------------------------------------------
// the launcher: casts and launches what choose() picked
// ---------------------------------------------------------------------------------------------------------
template <typename T>
void launch(bmsp_matrix_s *A, const void *v, void *u, int variant, hipStream_t st, uint32_t row_lo, uint32_t row_hi)
{
    using Ac = typename Acc<T>::type;
    const SpmvChoice c = choose(A, variant, row_lo, row_hi, st);
    const uint32_t nbr = (uint32_t)A->num_block_rows(), n_items = (uint32_t)A->spmv_num_chunks;
    char *mem = (char *)A->spmv_chunks;
    switch (c.path) {
    case SpmvPath::kNone: return;
    case SpmvPath::kBlockRow64:
    case SpmvPath::kBlockRow8: {
        const bool wave = c.path == SpmvPath::kBlockRow64;  // a wave per block-row: 4 per workgroup; 8 lanes per block-row: 32
        hipLaunchKernelGGL((wave ? spmv_blockrow_kernel<T, 64> : spmv_blockrow_kernel<T, 8>), dim3(wave ? (nbr + 3) / 4 : (nbr + 31) / 32), dim3(kThreads), 0, st,
                           A->rowptr, A->keys, A->bmps, A->offsets, (const T *)A->values, (const T *)v, (Ac *)u, row_hi, (uint32_t)A->num_cols, nbr, row_lo);
        break;
    }
    case SpmvPath::kRowGroup: {
        const uint32_t groups = (nbr + 3) / 4, waves = (groups + c.passes - 1) / c.passes;
        hipLaunchKernelGGL((spmv_rowgroup_kernel<T, /* U = */ 3>), dim3((waves + 3) / 4), dim3(kThreads), 0, st, A->rowptr, A->keys, A->bmps, A->offsets,
                           (const T *)A->values, (const T *)v, (Ac *)u, row_hi, (uint32_t)A->num_cols, nbr,
                           (uint32_t)((size_t)A->values_extent() * sizeof(T)) + 16u, c.passes, row_lo);
        break;
    }
    case SpmvPath::kChunk: {  // (fp32 only: chunk_wanted)
        const char *cm = (const char *)A->spmv_cw;
        hipLaunchKernelGGL(c.layout == 2 ? spmv_chunk_kernel<true> : spmv_chunk_kernel<false>, dim3((uint32_t)A->spmv_cw_chunks), dim3(64), 0, st, (const ChunkRec *)(cm + A->spmv_cw_off_rec),
                           (const uint32_t *)cm, (const float *)A->values, (const float *)v, (float *)u, (float *)(cm + A->spmv_cw_off_carry),
                           (uint32_t *)(cm + A->spmv_cw_off_cnt), (uint32_t)A->nnz, (uint32_t)A->num_rows, (uint32_t)A->num_cols,
                           (uint32_t)A->spmv_cw_colbits);
        break;
    }
    case SpmvPath::kVstream: {
        const auto kern = c.cached ? (c.red == kAtomic ? spmv_vstream_kernel<T, kCached, kAtomic> : spmv_vstream_kernel<T, kCached, kSorted>)
                                   : (c.red == kAtomic ? spmv_vstream_kernel<T, kDecode, kAtomic> : spmv_vstream_kernel<T, kDecode, kSorted>);
        hipLaunchKernelGGL(kern, dim3(n_items), dim3(64), 0, st, (const SweepItem *)(mem + 64), n_items, A->keys, A->bmps,
                           A->offsets, (const T *)A->values, (const T *)v, (Ac *)u, (Ac *)(mem + A->spmv_plan_off_carry),
                           (uint32_t *)(mem + A->spmv_plan_off_cnt), row_hi, (uint32_t)A->num_cols,
                           (uint32_t)((size_t)A->values_extent() * sizeof(T)), A->spmv_pos, (uint32_t)A->spmv_pos_base, (uint32_t)A->spmv_pos_count, row_lo,
                           A->spmv_tinfo, A->spmv_eoff);
        break;
    }
    case SpmvPath::kSweep: {
        auto kern = c.sweep == SweepKind::kFull ? spmv_sweep_kernel<T, true, false> : (c.sweep == SweepKind::kNT ? spmv_sweep_kernel<T, false, true> : (c.sweep == SweepKind::kPersist ? spmv_sweep_kernel<T, false, false, true> : spmv_sweep_kernel<T, false, false>));
        if (c.occ == 6) kern = spmv_sweep_kernel<T, false, false, false, 6>;
        if (c.occ == 8) kern = spmv_sweep_kernel<T, false, false, false, 8>;
        hipLaunchKernelGGL(kern, dim3(c.grid), dim3(kThreads), 0, st, (const SweepItem *)(mem + 64), n_items,
                           A->keys, A->bmps, A->offsets, (const T *)A->values, (const T *)v, (Ac *)u,
                           (Ac *)(mem + A->spmv_plan_off_carry), (uint32_t *)(mem + A->spmv_plan_off_cnt), row_hi,
                           (uint32_t)A->num_cols, (uint32_t)((size_t)A->values_extent() * sizeof(T)), row_lo);
        break;
    }
    }
    BMSP_CHECK_LAUNCH();
}

}  // namespace

// Which kernel bmsp_spmv launches for (A, variant) -- choose(), the launcher's own decision -- and the bytes that kernel's layout
// must move per launch ("compulsory": every array it reads or writes, once; counted from the plan, not estimated):
//   chunked sweep: value word + value per stored value (8 B) + chunk records (32 B) + x + y + per carry slot its 8 accumulators stored and
//     read back + per folded block-row its counter (add + reset);
//   value-stream, position + tile cache: items (32 B) + slot word (4 B per tile) + for items that are NOT a single batch the 2-byte value
//     end of every tile + entries (2 B) and values per stored value + x + y + carry slots;
//   value-stream, in-kernel decode: items + keys, bitmaps, offsets (24 B per tile) + values + x + y;
//   row-group / block-row kernels: block-row pointer + 24 B per tile + values + x + y;   sweep: items + 24 B per tile + values + x + y.
// format_bytes is SURVEY 8(d)'s figure for the bmSparse layout whatever the kernel reads: 24 B per tile + values + row pointer + x + y.
// The read-backs of chunk records and plan items below belong to the reporting; choose() makes none.
void spmv_launch_info(bmsp_matrix_s *A, int variant, hipStream_t st, char *kernel, size_t kernel_cap, int64_t *compulsory, int64_t *format_bytes)
{
    if (A->transposed) fail(BMSP_ERR_INVALID, "SpMV needs a matrix built with transposed=0");
    ensure_rowptr(A, st);
    const int64_t es = (int64_t)dtype_size(A->dtype), as = A->dtype == BMSP_F64 ? 8 : 4;
    const int64_t nbr = A->num_block_rows(), nb = A->block_num, nv = A->nnz;
    const int64_t xy = es * A->num_cols + as * A->num_rows;
    const int64_t fmt = 24 * nb + es * nv + 4 * (nbr + 1) + xy;
    if (format_bytes) *format_bytes = fmt;
    const SpmvChoice c = choose(A, variant, 0, (uint32_t)A->num_rows, st);
    const int64_t n_items = A->spmv_num_chunks;
    int64_t bytes = fmt;
    switch (c.path) {
    case SpmvPath::kNone: bytes = 0; break;
    case SpmvPath::kBlockRow64: case SpmvPath::kBlockRow8: case SpmvPath::kRowGroup: break;
    case SpmvPath::kChunk: {
        // chunked sweep: value words + values (4 B each per stored value) + records + x + y + the carry slots of the folded
        // block-rows (8 accumulators stored and read back per chunk that holds a part) and their counters (add + reset)
        const int64_t nch = A->spmv_cw_chunks;
        std::vector<ChunkRec> rec((size_t)nch);
        BMSP_HIP(hipStreamSynchronize(st));
        copy_d2h_staged(rec.data(), (const char *)A->spmv_cw + A->spmv_cw_off_rec, sizeof(ChunkRec) * (size_t)nch);
        int64_t slots = 0;
        for (const ChunkRec &r : rec) slots += ((r.flags & kChHead) ? 1 : 0) + ((r.flags & kChTail) ? 1 : 0);
        bytes = 8 * nv + (int64_t)sizeof(ChunkRec) * nch + xy + 2 * 8 * as * slots + 8 * A->spmv_cw_split;
        break;
    }
    case SpmvPath::kVstream: {
        std::vector<SweepItem> items((size_t)n_items);
        BMSP_HIP(hipStreamSynchronize(st));
        if (n_items) copy_d2h_staged(items.data(), plan_items(A), sizeof(SweepItem) * (size_t)n_items);
        int64_t multi_tiles = 0, long_items = 0;
        for (const SweepItem &it : items) {
            if (!vs_single(it)) multi_tiles += (int64_t)(it.blk_end - it.blk_begin);
            if (it.num_items) long_items++;
        }
        bytes = 32 * n_items + xy + 64 * long_items + es * nv;
        bytes += c.cached ? 4 * nb + 2 * multi_tiles + 2 * nv : 24 * nb;
        break;
    }
    case SpmvPath::kSweep: bytes = 32 * n_items + 24 * nb + es * nv + xy; break;
    }
    if (kernel && kernel_cap) snprintf(kernel, kernel_cap, "%s", path_name(c));
    if (compulsory) *compulsory = bytes;
}

// the layout of the chunk cache the default sweep of A reads (choose() builds it): 0 = no chunk cache (another kernel takes A), 1 = words
// in storage order (round 7), 2 = row-sorted words
int spmv_chunk_layout(bmsp_matrix_s *A, hipStream_t st)
{
    if (A->transposed) fail(BMSP_ERR_INVALID, "SpMV needs a matrix built with transposed=0");
    const SpmvChoice c = choose(A, BMSP_SPMV_DEFAULT, 0, (uint32_t)A->num_rows, st);
    return c.path == SpmvPath::kChunk ? c.layout : 0;
}

// bmsp_matrix_prepare(BMSP_PREPARE_SPMV): everything the default sweep of the whole matrix reads -- choose() builds it.  Second purpose:
// spmm.hip's choose_path() keys its value-stream kernels on A->spmv_pos, so a matrix whose SpMV takes the chunked sweep gets the position
// cache as well (on the value-stream path choose() has built it; the row-group, sweep and block-row paths get none, SpMM's other kernels run)
void prepare_spmv(bmsp_matrix_s *A, hipStream_t st)
{
    if (A->transposed) return;
    if (choose(A, BMSP_SPMV_DEFAULT, 0, (uint32_t)A->num_rows, st).path == SpmvPath::kChunk) build_pos_cache(A, st);
}

// row_lo / row_hi: only rows [row_lo, row_hi) of u are written (the sharded sweep: a rank writes its own slice and nothing else);
// the default is every row
void spmv(bmsp_matrix_s *A, const void *v, void *u, int variant, hipStream_t st, int64_t row_lo, int64_t row_hi)
{
    if (A->transposed) fail(BMSP_ERR_INVALID, "SpMV needs a matrix built with transposed=0");
    if (!v || !u) fail(BMSP_ERR_INVALID, "null vector");
    if (variant < 0 || variant > 3) fail(BMSP_ERR_INVALID, "unknown SpMV variant %d", variant);
    ensure_rowptr(A, st);
    const uint32_t lo = (uint32_t)std::max<int64_t>(0, row_lo);
    const uint32_t hi = (uint32_t)(row_hi < 0 ? (int64_t)A->num_rows : std::min<int64_t>(row_hi, A->num_rows));
    switch (A->dtype) {
    case BMSP_F32: launch<float>(A, v, u, variant, st, lo, hi); break;
    case BMSP_F16: launch<_Float16>(A, v, u, variant, st, lo, hi); break;
    case BMSP_F64: launch<double>(A, v, u, variant, st, lo, hi); break;
    }
}

}  // namespace bmsp

BMSP_DEFINE_WARM(spmv)
