// aggregate.hip -- the two stages of an algebraic-multigrid set-up that the library lacked: partitioning the nodes of a strength graph
// into aggregates (bmsp_matrix_aggregate) and building the tentative prolongator from an aggregate map (bmsp_matrix_from_aggregates),
// without going back through scalar COO entries.
//
// Aggregation (MIS(2) by fixed-priority Luby rounds).  The graph: nodes = the scalar rows 0 .. n-1 of a square S; i != j are neighbours
// iff (i, j) or (j, i) is stored (a stored zero counts, values are never loaded).  The row direction is read from S's keys, bitmaps and
// block-row pointer, the column direction from the cached op-T view of bmsp_spmv_op (its records carry the bitmap and the block-row);
// S + S^T is never formed.  key(i) = (splitmix64(seed ^ i) >> 32, i), on the device one word K(i) = (hash32 << 32 | i) + 1 (0 = none;
// all ones cannot occur because i < 2^31).  The roots are the greedy distance-2 independent set in descending key order, a pure function
// of structure and seed.
//   per-node word w   K(i) while i is undecided, all ones once it is a root, 0 once it is eliminated
//   agg_pass_kernel<LAYOUT, MODE>   ONE template: eight lanes per block-row, a lane per scalar row; the lanes walk the block-row's tiles
//       together (layout 0: a lane takes its byte of every bitmap; layout 1: its bit of every byte) and then the view's records of the
//       block-column (the other way round: spmv_op.hip's MINOR / non-MINOR), every set bit a gather of the neighbour's 8-byte word; the
//       result is the maximum over the closed neighbourhood.  MODE says what is gathered and what is done with the maximum:
//         FIRST    m1[i] = max w over N[i], for every node whatever its state (distance is taken in the whole graph)
//         SECOND   undecided i only: m2 = max m1 over N[i].  All ones: a root lies within distance 2, i is eliminated.  Else m2 == K(i):
//                  i holds the greatest undecided key within distance 2, it becomes a root.  Else it stays, and is counted.
//         ROOTS    p1[i] = max over N[i] of (root ? K : 0): the neighbouring root of greatest key
//         ASSIGN   a root takes its rank among the roots; a node with p1 != 0 joins that root; every other node joins the greatest root
//                  its neighbours are adjacent to, max p1 over N[i] (one exists: the set is maximal)
//   schedule   a round is TWO launches, FIRST then SECOND, and elimination lags one round: the roots of round k are all ones in round
//       k + 1's FIRST pass and eliminate their distance-2 neighbourhood in its SECOND pass, next to that round's selection.  A node a
//       pending root has yet to eliminate is still "undecided" for its neighbours, which delays a selection but never changes it: a key
//       that is the greatest of a superset is the greatest of the set.  Every round decides at least the greatest undecided key, and
//       `rounds` counts them, the last one (eliminations only) included.  The other schedule (select, then eliminate, four launches a
//       round: BMSP_AGG_SCHEDULE=separate, a measurement switch) gives the same roots, and on all six bench matrices in exactly as many
//       launches (34 / 28 / 30 / 20 / 34 / 32: a round that selects right after a selection finds next to nothing, since new local
//       maxima appear only once the eliminations have been made) and in the same time within 3 % (DESIGN §4 "Aggregation").  The lagged
//       form is kept because it has one kind of round; under the other `rounds` counts rounds of four.
//   termination   bmsp_spitsv's protocol: every SECOND pass leaves a record of the nodes still undecided, built by integer atomics (one
//       add per workgroup); the launches of the next round read it and return at once when it is 0.  The host enqueues BMSP_AGG_CHECK
//       rounds, reads their records back and stops at the first zero.  Nothing waits between workgroups.
//
// Prolongator.  P[i, agg[i]] = w_i, one stored entry per row (agg[i] == 0xFFFFFFFF: none).  The builder orders tiles by (block-row,
// block-column) in BOTH layouts (only the position inside a tile differs), so a block-row's tiles are known from its own eight entries:
// eight lanes order their agg >> 3 inside the group by shuffles and mark the distinct ones, one scan of the packed (tiles, entries)
// counts gives tile and value offsets, one pass writes keys, bitmaps, offsets, values and the block-row pointer.  Neither layout pays
// for a sort.  The first pass also validates every entry; its flag comes back with the scan's totals in one 16-byte read-back before
// anything is allocated.
#include "tile_pass.hip.h"
#include "sweep_stats.hip.h"
#include <cstring>
#include <vector>

namespace bmsp {
namespace {

// rounds enqueued between two read-backs (BMSP_AGG_CHECK).  Measured (tools/amg_bench.py, the call with the view cached, wall ms at
// 1 / 2 / 4 / 8): Poisson 7pt 128^3 (15 rounds) 2.507 / 2.336 / 2.270 / 2.181; Poisson 27pt 64^3 (12) 1.735 / 1.576 / 1.507 / 1.491;
// fem_like 27pt (13) 2.759 / 2.606 / 2.562 / 2.486; banded half-bandwidth 32 (8) 0.745 / 0.646 / 0.592 / 0.561 -- 8 is the fastest on
// all four (a call takes 8 - 15 rounds: one or two read-backs); the two R-MAT matrices do not care (204 / 60 ms, the hub rows' walks)
constexpr int64_t kAggCheckDefault = 8;
constexpr int64_t kAggCheckMax = 1024;  // records of one batch
constexpr uint64_t kRoot = ~0ull;
constexpr uint32_t kSkip = ~0u;

enum { kFirst = 0, kSecond = 1, kRoots = 2, kAssign = 3 };
enum { kBoth = 0, kSelectOnly = 1, kEliminateOnly = 2 };

// the finaliser of pybmsp/gen.py (reorder.hip)
__device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t node_key(uint64_t seed, uint32_t i) { return ((splitmix64(seed ^ (uint64_t)i) >> 32 << 32) | i) + 1ull; }

// nodes still undecided after the step; all zero = the step did not run
struct AggRecord {
    uint32_t pending, pad;
};

struct InitKeys {
    uint64_t *w;
    uint64_t seed;
    uint32_t n;
    AggRecord *rec;
    __device__ void operator()(uint64_t i) const
    {
        w[i] = node_key(seed, (uint32_t)i);
        if (i == 0) rec[0] = AggRecord{n, 0u};
    }
};

// what a pass gathers for neighbour j
template <int MODE>
__device__ __forceinline__ uint64_t agg_load(const uint64_t *in, uint32_t j, uint64_t seed)
{
    const uint64_t v = in[j];
    if (MODE == kRoots) return v == kRoot ? node_key(seed, j) : 0ull;
    return v;
}

// the stored positions of lane t's line of a tile as offsets 0 .. 7 along the other axis: its byte (MINOR = false) or its bit of every
// byte (MINOR = true); best = max(best, what the pass gathers at base + offset)
template <int MODE, bool MINOR>
__device__ __forceinline__ void agg_tile(uint64_t bmp, int t, uint64_t base, uint32_t n, const uint64_t *in, uint64_t seed, uint64_t &best)
{
    if (!MINOR) {
        uint32_t byte = tile_byte(bmp, t);
        while (byte) {
            const int c = __builtin_clz(byte) - 24;
            byte &= ~(0x80u >> c);
            const uint64_t j = base + (uint64_t)c;
            if (j < n) {  // (stored entries lie inside the matrix; the test keeps a malformed bitmap from reading beyond the words)
                const uint64_t v = agg_load<MODE>(in, (uint32_t)j, seed);
                best = v > best ? v : best;
            }
        }
    } else {
        uint64_t m = bmp & (0x8080808080808080ull >> t);
        while (m) {
            const int p = tile_pop_first(m);
            const uint64_t j = base + (uint64_t)(p >> 3);
            if (j < n) {
                const uint64_t v = agg_load<MODE>(in, (uint32_t)j, seed);
                best = v > best ? v : best;
            }
        }
    }
}

// One pass over the scalar graph of n nodes in nb block-rows (header comment).  in: what is gathered (w, m1, w, p1 by MODE); w: the
// per-node words (SECOND rewrites its own node's, ASSIGN reads it); out: m1 / p1 (FIRST / ROOTS); p1, rank, agg: ASSIGN.  prev: the
// record of the step before (FIRST, SECOND: every lane of the grid reads the same record of an earlier launch, all leave or none).
template <bool LAY1, int MODE>
__global__ __launch_bounds__(kThreads) void agg_pass_kernel(const uint32_t *__restrict__ rowptr, const uint64_t *__restrict__ keys,
                                                            const uint64_t *__restrict__ bmps, const uint32_t *__restrict__ colptr,
                                                            const uint4 *__restrict__ crecs, uint32_t n, uint32_t nb, uint64_t seed, int sub,
                                                            const uint64_t *in, uint64_t *w, uint64_t *out, const uint32_t *__restrict__ rank,
                                                            uint32_t *agg, const AggRecord *prev, AggRecord *mine)
{
    if (prev && prev->pending == 0) return;
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t g = gid >> 3;
    const int t = (int)(threadIdx.x & 7u);
    const uint64_t i64 = g * 8 + (uint64_t)t;
    bool live = g < nb && i64 < n;
    const uint32_t i = (uint32_t)i64;
    uint64_t own = 0;
    if (live && (MODE == kSecond || MODE == kAssign)) own = w[i];
    if (MODE == kSecond) live = live && own != 0 && own != kRoot;
    uint32_t pending = 0;
    if (live) {
        uint64_t best = agg_load<MODE>(in, i, seed);
        const bool walk = MODE != kAssign || (own != kRoot && best == 0);  // (ASSIGN: only the nodes without a neighbouring root)
        if (walk) {
            const uint32_t r1 = rowptr[g + 1];
            for (uint32_t e = rowptr[g]; e < r1; e++)
                agg_tile<MODE, LAY1>(bmps[e], t, (uint64_t)key_col(keys[e]) * 8, n, in, seed, best);
            const uint32_t c1 = colptr[g + 1];
            for (uint32_t e = colptr[g]; e < c1; e++) {
                const uint4 r = crecs[e];
                agg_tile<MODE, !LAY1>((uint64_t)r.y << 32 | r.x, t, (uint64_t)r.w * 8, n, in, seed, best);
            }
        }
        if (MODE == kFirst || MODE == kRoots) out[i] = best;
        if (MODE == kSecond) {
            if (best == kRoot && sub != kSelectOnly) w[i] = 0;
            else if (best == own && sub != kEliminateOnly) w[i] = kRoot;
            else pending = 1;
        }
        if (MODE == kAssign) {
            const uint64_t target = own == kRoot ? node_key(seed, i) : best;
            agg[i] = target ? rank[(uint32_t)(target - 1)] : kSkip;  // (the low half of K - 1 is the node; 0 cannot occur: maximality)
        }
    }
    if (MODE != kSecond) return;
    // the workgroup's count: registers across the wave, LDS across the four waves, then ONE lane issues the atomic
    pending = wave_sum(pending);
    __shared__ uint32_t part[kThreads / kWave];
    if (lane_id() == 0) part[wave_id()] = pending;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t p = 0;
#pragma unroll
        for (int k = 0; k < kThreads / kWave; k++) p += part[k];
        if (p) atomicAdd(&mine->pending, p);
    }
}

struct RootFlag {
    const uint64_t *w;
    uint64_t n;
    __device__ uint32_t operator()(uint64_t i) const { return i < n && w[i] == kRoot ? 1u : 0u; }
};

struct Passes {
    const uint32_t *rowptr, *colptr;
    const uint64_t *keys, *bmps;
    const uint4 *crecs;
    uint32_t n, nb;
    uint64_t seed;
    int lay1;
    hipStream_t st;
    template <int MODE>
    void run(int sub, const uint64_t *in, uint64_t *w, uint64_t *out, const uint32_t *rank, uint32_t *agg, const AggRecord *prev,
             AggRecord *mine) const
    {
        if (lay1)
            hipLaunchKernelGGL((agg_pass_kernel<true, MODE>), grid_for((uint64_t)nb * 8), dim3(kThreads), 0, st, rowptr, keys, bmps, colptr,
                               crecs, n, nb, seed, sub, in, w, out, rank, agg, prev, mine);
        else
            hipLaunchKernelGGL((agg_pass_kernel<false, MODE>), grid_for((uint64_t)nb * 8), dim3(kThreads), 0, st, rowptr, keys, bmps, colptr,
                               crecs, n, nb, seed, sub, in, w, out, rank, agg, prev, mine);
        BMSP_CHECK_LAUNCH();
    }
};

bool schedule_separate()
{
    const char *e = getenv("BMSP_AGG_SCHEDULE");
    return e && !strcmp(e, "separate");
}

// ---- from_aggregates -------------------------------------------------------------------------------------------------------------------
// What lane t of a block-row's group learns about the group's tiles from the eight entries: whether it is the first lane of its tile,
// its tile's place among the block-row's tiles, bitmap and first value (relative to the block-row), its own value's place in the tile,
// and the group's totals.  Every lane of the group calls it (shuffles).
struct GroupTiles {
    bool first;
    uint32_t tile, tiles, entries, before, in_tile;
    uint64_t bmp;
};

template <bool LAY1>
__device__ __forceinline__ GroupTiles group_tiles(uint32_t a, bool valid, int t)
{
    GroupTiles r{valid, 0u, 0u, 0u, 0u, 0u, 0ull};
    const uint32_t bc = a >> 3, c = a & 7u;
    // my position inside the tile orders the tile's values: 8 row + column (layout 0), 8 column + row (layout 1)
    const uint32_t mypos = LAY1 ? (c << 3 | (uint32_t)t) : ((uint32_t)t << 3 | c);
    uint32_t au[8], vu[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
        au[u] = __shfl(a, u, 8);
        vu[u] = __shfl(valid ? 1u : 0u, u, 8);
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
        if (!vu[u]) continue;
        r.entries++;
        const uint32_t bu = au[u] >> 3, cu = au[u] & 7u;
        if (bu < bc) r.before++;
        if (bu != bc) continue;
        if (u < t) r.first = false;
        const uint32_t pos = LAY1 ? (cu << 3 | (uint32_t)u) : ((uint32_t)u << 3 | cu);
        r.bmp |= 1ull << (63 - pos);
        if (pos < mypos) r.in_tile++;
    }
    const uint32_t f = r.first ? 1u : 0u;
#pragma unroll
    for (int u = 0; u < 8; u++) {
        const uint32_t fu = __shfl(f, u, 8);
        r.tiles += fu;
        if (fu && (au[u] >> 3) < bc) r.tile++;
    }
    return r;
}

// counts[I] = tiles << 32 | entries of block-row I; *bad = 1 when an entry is neither below num_agg nor the skip value
__global__ __launch_bounds__(kThreads) void prolong_count_kernel(const uint32_t *__restrict__ agg, uint32_t num_rows, uint32_t nbr,
                                                                 uint32_t num_agg, uint64_t *counts, uint64_t *bad)
{
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t g = gid >> 3;
    const int t = (int)(threadIdx.x & 7u);
    if (g >= nbr) return;  // (whole groups)
    const uint64_t i = g * 8 + (uint64_t)t;
    uint32_t a = kSkip;
    if (i < num_rows) a = agg[i];
    const bool valid = a != kSkip;
    if (valid && a >= num_agg) *bad = 1ull;
    const GroupTiles r = group_tiles<false>(a, valid, t);  // (the counts do not depend on the layout)
    if (t == 0) counts[g] = (uint64_t)r.tiles << 32 | r.entries;
}

// base[I] = tiles << 32 | entries in front of block-row I (base[nbr]: the totals)
template <typename S, bool LAY1>
__global__ __launch_bounds__(kThreads) void prolong_write_kernel(const uint32_t *__restrict__ agg,
                                                                 const typename TileValue<S>::R *__restrict__ weights, uint32_t num_rows,
                                                                 uint32_t nbr, const uint64_t *__restrict__ base, uint64_t *keys,
                                                                 uint64_t *bmps, uint64_t *offsets, S *vals, uint32_t *rowptr)
{
    using D = TileValue<S>;
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t g = gid >> 3;
    const int t = (int)(threadIdx.x & 7u);
    if (g >= nbr) return;
    const uint64_t i = g * 8 + (uint64_t)t;
    uint32_t a = kSkip;
    if (i < num_rows) a = agg[i];
    const bool valid = a != kSkip;
    const GroupTiles r = group_tiles<LAY1>(a, valid, t);
    const uint64_t b = base[g];
    const uint64_t tile0 = b >> 32, val0 = b & 0xffffffffull;
    if (t == 0) {
        rowptr[g] = (uint32_t)tile0;
        if (g == nbr - 1) {
            rowptr[nbr] = (uint32_t)(tile0 + r.tiles);
            offsets[tile0 + r.tiles] = val0 + r.entries;
        }
    }
    if (!valid) return;
    const uint64_t tile = tile0 + r.tile, off = val0 + r.before;
    if (r.first) {
        keys[tile] = key_make((uint32_t)g, a >> 3);
        bmps[tile] = r.bmp;
        offsets[tile] = off;
    }
    vals[off + r.in_tile] = D::store(weights ? weights[i] : typename D::R(1));
}

}  // namespace

void aggregate_check_matrix(const bmsp_matrix_s *S)
{
    if (S->num_rows != S->num_cols) fail(BMSP_ERR_INVALID, "aggregate: matrix S must be square (it is %d x %d)", S->num_rows, S->num_cols);
    spmv_op_check_matrix(S, "aggregate");
    // K(i) = (hash32 << 32 | i) + 1 must stay below all ones, and 0xFFFFFFFF is no aggregate id
    if ((int64_t)S->num_rows >= (1ll << 32) - 1) fail(BMSP_ERR_LIMIT, "aggregate: %d nodes exceed the 2^32 - 2 the node words hold", S->num_rows);
}

void aggregate(bmsp_matrix_s *S, uint64_t seed, uint32_t *d_agg, int64_t *num_aggregates, hipStream_t st, bmsp_aggregate_info *info)
{
    aggregate_check_matrix(S);
    const int64_t n = S->num_rows, nb = S->num_block_rows();
    if (info) {
        memset(info, 0, sizeof *info);
        info->nodes = n;
        snprintf(info->kernel, sizeof info->kernel, "none (empty matrix)");
    }
    *num_aggregates = 0;
    if (n == 0) {
        BMSP_HIP(hipStreamSynchronize(st));
        return;
    }
    ensure_rowptr(S, st);
    const bmsp_spmv_op_view &v = spmv_op_ensure_view(S, BMSP_OP_T, st);
    const bool separate = schedule_separate();
    int64_t check = sweep_check_from_env("BMSP_AGG_CHECK", kAggCheckDefault);
    if (check > kAggCheckMax) check = kAggCheckMax;
    const int64_t per_round = separate ? 2 : 1;  // steps (a FIRST and a SECOND launch each) per round
    const int64_t batch = check * per_round;
    DevBuf<uint64_t> w((size_t)n), m((size_t)n);
    DevBuf<uint32_t> rank((size_t)n + 1);
    DevBuf<AggRecord> recs((size_t)batch + 1);
    std::vector<AggRecord> host((size_t)batch + 1);
    const Passes P{S->rowptr, (const uint32_t *)((const char *)v.mem + v.off_ptr), S->keys, S->bmps, (const uint4 *)v.mem, (uint32_t)n,
                   (uint32_t)nb, seed, S->transposed ? 1 : 0, st};
    device_for_each(InitKeys{w.p, seed, (uint32_t)n, recs.p}, (uint64_t)n, st);
    // every step decides at least one node while any is left (the greatest undecided key: selected, or eliminated by a root)
    const int64_t cap = 2 * n + 2;
    int64_t steps = 0;
    for (int64_t done = 0; done < cap && !steps; done += batch) {
        BMSP_HIP(hipMemsetAsync(recs.p + 1, 0, sizeof(AggRecord) * (size_t)batch, st));
        for (int64_t k = 1; k <= batch; k++) {
            const int sub = !separate ? kBoth : ((done + k) & 1 ? kSelectOnly : kEliminateOnly);
            P.run<kFirst>(sub, w.p, w.p, m.p, nullptr, nullptr, recs.p + k - 1, nullptr);
            P.run<kSecond>(sub, m.p, w.p, nullptr, nullptr, nullptr, recs.p + k - 1, recs.p + k);
        }
        BMSP_HIP(hipStreamSynchronize(st));
        copy_d2h_staged(host.data() + 1, recs.p + 1, sizeof(AggRecord) * (size_t)batch);
        for (int64_t k = 1; k <= batch; k++)
            if (host[(size_t)k].pending == 0) {  // (the steps enqueued behind it returned at once and wrote nothing)
                steps = done + k;
                break;
            }
        if (!steps) BMSP_HIP(hipMemcpyAsync(recs.p, recs.p + batch, sizeof(AggRecord), hipMemcpyDeviceToDevice, st));
    }
    if (!steps) fail(BMSP_ERR_INTERNAL, "aggregate: %lld steps left nodes undecided", (long long)cap);
    // ids: the rank among the roots in ascending node index; then the two propagation passes
    device_exclusive_scan<uint32_t>(RootFlag{w.p, (uint64_t)n}, PtrOut<uint32_t>{rank.p}, (uint64_t)n + 1, st);
    P.run<kRoots>(kBoth, w.p, w.p, m.p, nullptr, nullptr, nullptr, nullptr);
    P.run<kAssign>(kBoth, m.p, w.p, nullptr, rank.p, d_agg, nullptr, nullptr);
    *num_aggregates = (int64_t)read_back(rank.p + n, st);  // synchronises: the scratch goes back to the pool
    if (info) {
        info->aggregates = *num_aggregates;
        info->rounds = (steps + per_round - 1) / per_round;
        info->launches = 1 + 2 * steps + 3;  // the words, FIRST and SECOND per step, the scan (counted once), ROOTS, ASSIGN
        info->view_bytes = (int64_t)v.bytes;
        snprintf(info->kernel, sizeof info->kernel, "agg_pass_kernel<layout %d>", S->transposed ? 1 : 0);
    }
}

void from_aggregates_check_args(int num_rows, int num_aggregates, const uint32_t *d_agg, bmsp_dtype dtype, int transposed)
{
    if (num_rows < 0 || num_aggregates < 0)
        fail(BMSP_ERR_INVALID, "num_rows and num_aggregates must be >= 0 (got %d, %d)", num_rows, num_aggregates);
    if (dtype != BMSP_F32 && dtype != BMSP_F16 && dtype != BMSP_F64) fail(BMSP_ERR_INVALID, "unknown dtype %d", (int)dtype);
    check_layout_flag(transposed, "transposed");
    if (!d_agg && num_rows > 0) fail(BMSP_ERR_INVALID, "d_agg is null");
}

// the num_rows x num_aggregates matrix with weights[i] (null: 1) stored at (i, d_agg[i]), tiles in layout `transposed`
bmsp_matrix_s *matrix_from_aggregates(int num_rows, int num_aggregates, const uint32_t *d_agg, const void *d_weights, bmsp_dtype dtype,
                                      int transposed, hipStream_t st)
{
    from_aggregates_check_args(num_rows, num_aggregates, d_agg, dtype, transposed);
    auto m = make_matrix();
    m->num_rows = num_rows; m->num_cols = num_aggregates; m->dtype = dtype; m->transposed = transposed;
    const uint64_t nbr = (uint64_t)m->num_block_rows();
    DevBuf<uint64_t> base((size_t)nbr + 2);  // counts, then their scan; [nbr]: the totals; [nbr + 1]: the check's flag
    uint64_t h[2] = {0ull, 0ull};
    if (nbr) {
        BMSP_HIP(hipMemsetAsync(base.p + nbr, 0, 16, st));
        hipLaunchKernelGGL(prolong_count_kernel, grid_for(nbr * 8), dim3(kThreads), 0, st, d_agg, (uint32_t)num_rows, (uint32_t)nbr,
                           (uint32_t)num_aggregates, base.p, base.p + nbr + 1);
        BMSP_CHECK_LAUNCH();
        device_exclusive_scan<uint64_t>(PtrIn<uint64_t>{base.p}, PtrOut<uint64_t>{base.p}, nbr + 1, st);
        read_back_bytes(h, base.p + nbr, 16, st);
        if (h[1])
            fail(BMSP_ERR_INVALID, "d_agg holds an entry that is neither below num_aggregates (%d) nor 0xFFFFFFFF", num_aggregates);
    }
    m->block_num = (int64_t)(h[0] >> 32);
    m->nnz = (int64_t)(h[0] & 0xffffffffull);
    alloc_tile_arrays(m.get(), (uint64_t)m->block_num);
    alloc_values(m.get(), (uint64_t)m->nnz);
    m->rowptr.alloc((size_t)(nbr + 1));
    m->rowptr_rows = (int64_t)nbr;
    if (nbr == 0) {
        BMSP_HIP(hipMemsetAsync(m->offsets, 0, 8, st));
        BMSP_HIP(hipMemsetAsync(m->rowptr, 0, 4, st));
    } else {
        dispatch_dtype(dtype, [&](auto s) {
            using S = decltype(s);
            using R = typename TileValue<S>::R;
            if (transposed)
                hipLaunchKernelGGL((prolong_write_kernel<S, true>), grid_for(nbr * 8), dim3(kThreads), 0, st, d_agg, (const R *)d_weights,
                                   (uint32_t)num_rows, (uint32_t)nbr, (const uint64_t *)base.p, m->keys, m->bmps, m->offsets, (S *)m->values,
                                   m->rowptr);
            else
                hipLaunchKernelGGL((prolong_write_kernel<S, false>), grid_for(nbr * 8), dim3(kThreads), 0, st, d_agg, (const R *)d_weights,
                                   (uint32_t)num_rows, (uint32_t)nbr, (const uint64_t *)base.p, m->keys, m->bmps, m->offsets, (S *)m->values,
                                   m->rowptr);
        });
        BMSP_CHECK_LAUNCH();
    }
    BMSP_HIP(hipStreamSynchronize(st));  // the scan's array goes back to the pool
    return m.release();
}

}  // namespace bmsp

BMSP_DEFINE_WARM(aggregate)
