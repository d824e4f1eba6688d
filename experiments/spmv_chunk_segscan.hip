// Go / no-go of the round-7 reduction of the chunked SpMV sweep (spmv_chunk_kernel): the non-hub chunks' LDS float adds replaced by a
// segmented reduction keyed by block-row, in registers (DPP), on the ladder's matrix and harness (experiments/spmv_chunk_ladder.hip:
// webbase-1M stand-in, R-MAT 2^20 x 2 + I, storage order, nine rotated copies).  DESIGN.md, SpMV round 7.
//   j  the round-6 kernel (the ladder's rung j): a lane's values combined by row, then one ds_add_f32 per distinct row into the window
//   k  j with the window adds replaced: per lane, 8-wide sums per block-row (head, middle block-rows written to the window, tail), an
//      inclusive segmented scan of the tail sums across lanes (row_shr / row_bcast DPP), heads continued from the left lane, every
//      block-row written once with plain LDS stores by the lane where it ends
// A third rung, k with the hub chunks' halving exchange on __builtin_amdgcn_permlane32_swap / permlane16_swap and DPP, ran 0.03 us
// faster than k in the first call and was wrong: the compiler added the builtin's first result to itself (v_add_f32 v4, v4, v4 after
// v_permlane32_swap_b32 v4, v8), so it is not kept.
// Each is checked against a host reference (double) on a NaN-poisoned y, and k against j; then both interleaved for the spread.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

constexpr uint32_t kV = 512, kPer = kV / 64, kWin = 1024, kOob = 0xffffffffu;
enum { kHead = 1, kTail = 2 };
struct Rec { uint32_t fb, own_b, own_e, flags, head_ca, head_cb, tail_cb, nwin; };
typedef __amdgpu_buffer_rsrc_t rsrc_t;
typedef float f4 __attribute__((ext_vector_type(4)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ rsrc_t rsrc(const void *p, uint32_t bytes) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, bytes, 0x00020000); }
__device__ __forceinline__ float ldf(rsrc_t r, uint32_t off) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0)); }

__device__ __forceinline__ float sum8(const float (&s)[8], int lane)
{
    const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
    float t[4], u[2];
#pragma unroll
    for (int i = 0; i < 4; i++) t[i] = (h5 ? s[i + 4] : s[i]) + __shfl_xor(h5 ? s[i] : s[i + 4], 32, 64);
#pragma unroll
    for (int i = 0; i < 2; i++) u[i] = (h4 ? t[i + 2] : t[i]) + __shfl_xor(h4 ? t[i] : t[i + 2], 16, 64);
    float v = (h3 ? u[1] : u[0]) + __shfl_xor(h3 ? u[0] : u[1], 8, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    return v;
}

__device__ __forceinline__ void fold(const float *carry, float *y, uint32_t *counters, uint32_t ca, uint32_t cb, uint32_t br, uint32_t num_rows, int lane)
{
    const int r = lane & 7, g = lane >> 3;
    float sum = 0.f;
    for (uint32_t k = ca + (uint32_t)g; k <= cb; k += 8)
        sum += __hip_atomic_load(&carry[((size_t)k * 2 + (k == ca ? 1 : 0)) * 8 + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int d = 8; d < 64; d <<= 1) sum += __shfl_xor(sum, d, 64);
    const uint32_t row = br * 8u + (uint32_t)r;
    if (g == 0 && row < num_rows) y[row] = sum;
    if (lane == 0) __hip_atomic_store(&counters[ca], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the loads and gathers every rung shares (whole chunks and the partial last one, as in the product)
__device__ __forceinline__ void load_chunk(uint32_t c, int lane, const uint32_t *words, const float *values, const float *x, uint32_t nnz,
                                           uint32_t num_cols, uint32_t (&w)[kPer], float (&a)[kPer], float (&xv)[kPer])
{
    const uint32_t first = c * kV + kPer * (uint32_t)lane;
    const rsrc_t rw = rsrc(words, nnz * 4u), rv = rsrc(values, nnz * 4u), rx = rsrc(x, num_cols * 4u);
    if (c * kV + kV <= nnz) {
#pragma unroll
        for (uint32_t q = 0; q < kPer; q += 4) {
            const u4 wq = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(rw, (first + q) * 4u, 0, 0));
            const f4 aq = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rv, (first + q) * 4u, 0, 0));
#pragma unroll
            for (int i = 0; i < 4; i++) { w[q + i] = wq[i]; a[q + i] = aq[i]; }
        }
    } else {
#pragma unroll
        for (uint32_t j = 0; j < kPer; j++) {
            const uint32_t off = first + j < nnz ? (first + j) * 4u : kOob;
            w[j] = __builtin_amdgcn_raw_buffer_load_b32(rw, off, 0, 0);
            a[j] = ldf(rv, off);
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) xv[j] = ldf(rx, first + j < nnz ? (w[j] & 0xfffffu) * 4u : kOob);
}

// rungs b .. f: the round-5 body, cut after rung R (2 = b .. 6 = f); CMB: its reduction with a lane's values combined by row in registers
// first, one LDS add per distinct row of the lane (j: the round-6 kernel)
template <int R, bool CMB = false>
__global__ __launch_bounds__(64, 8) void r5_kernel(const Rec *recs, const uint32_t *words, const float *values, const float *x, float *y, float *out,
                                                   float *carry, uint32_t *counters, uint32_t nnz, uint32_t num_rows, uint32_t num_cols)
{
    __shared__ float win[kWin];
    const int lane = threadIdx.x & 63;
    const uint32_t c = blockIdx.x;
    const Rec rc = recs[c];
    const uint32_t first = c * kV + kPer * (uint32_t)lane;
    uint32_t w[kPer];
    float a[kPer], xv[kPer];
    load_chunk(c, lane, words, values, x, nnz, num_cols, w, a, xv);
    if (rc.nwin == 8) {
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (uint32_t j = 0; j < kPer; j++) {
            const uint32_t rr = w[j] >> 20;
            const float p = first + j < nnz ? a[j] * xv[j] : 0.f;
#pragma unroll
            for (int k = 0; k < 8; k++) s[k] += rr == (uint32_t)k ? p : 0.f;
        }
        const float v = sum8(s, lane);
        if ((lane & 7) == 0) win[((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1)] = v;
    } else {
        for (uint32_t e = (uint32_t)lane; e < rc.nwin; e += 64) win[e] = 0.f;
        __builtin_amdgcn_wave_barrier();
        if constexpr (CMB) {
            float acc[kPer];
            bool lead[kPer];
#pragma unroll
            for (uint32_t j = 0; j < kPer; j++) acc[j] = first + j < nnz ? a[j] * xv[j] : 0.f;
#pragma unroll
            for (uint32_t j = 0; j < kPer; j++) {
                bool taken = false;
#pragma unroll
                for (uint32_t i = 0; i < j; i++) {
                    const bool hit = !taken && (w[i] >> 20) == (w[j] >> 20);
                    acc[i] += hit ? acc[j] : 0.f;
                    taken |= hit;
                }
                lead[j] = !taken;
            }
#pragma unroll
            for (uint32_t j = 0; j < kPer; j++)
                if (lead[j] && first + j < nnz) __hip_atomic_fetch_add(win + (w[j] >> 20), acc[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
        float run = 0.f;
#pragma unroll
        for (uint32_t j = 0; j < kPer && !CMB; j++) {
            const uint32_t rr = w[j] >> 20;
            const bool on = first + j < nnz;
            const bool flush = j == kPer - 1 || first + j + 1 >= nnz || (w[j + (j < kPer - 1 ? 1 : 0)] >> 20) != rr;
            run += on ? a[j] * xv[j] : 0.f;
            if (flush) {
                if (on) __hip_atomic_fetch_add(win + rr, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                run = 0.f;
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    if constexpr (R == 2) {
        out[c * 64 + lane] = win[lane & 7];
        return;
    }
    const int32_t base = (int32_t)(rc.fb * 8u);
    const uint32_t row_end = min(rc.own_e * 8u, num_rows);
    for (uint32_t row = rc.own_b * 8u + (uint32_t)lane; row < row_end; row += 64) {
        const int32_t rel = (int32_t)row - base;
        y[row] = rel >= 0 && rel < (int32_t)rc.nwin ? win[rel] : 0.f;
    }
    if (R == 3 || !rc.flags) return;
    if ((rc.flags & kHead) && lane < 8) __hip_atomic_store(&carry[((size_t)c * 2) * 8 + lane], win[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((rc.flags & kTail) && lane < 8)
        __hip_atomic_store(&carry[((size_t)c * 2 + 1) * 8 + lane], win[rc.nwin - 8u + (uint32_t)lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (R == 4) return;
    uint32_t ticket = 0;
    if (lane == 0 && (rc.flags & kHead)) ticket = __hip_atomic_fetch_add(&counters[rc.head_ca], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == 1 && (rc.flags & kTail)) ticket = __hip_atomic_fetch_add(&counters[c], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t th = (uint32_t)__builtin_amdgcn_readlane((int)ticket, 0), tt = (uint32_t)__builtin_amdgcn_readlane((int)ticket, 1);
    if constexpr (R == 5) {
        if (th == kOob && tt == kOob) out[c * 64 + lane] = 0.f;  // never true: keeps the tickets used
        return;
    }
    if ((rc.flags & kHead) && th == rc.head_cb - rc.head_ca) fold(carry, y, counters, rc.head_ca, rc.head_cb, rc.fb, num_rows, lane);
    if ((rc.flags & kTail) && tt == rc.tail_cb - c) fold(carry, y, counters, c, rc.tail_cb, rc.fb + rc.nwin / 8u - 1u, num_rows, lane);
}

// ---- round 7: the segmented reduction keyed by block-row (no ds_add_f32) ----------------------------------------------------------------
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ float dppf(float old, float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), CTRL, ROWS, 0xf, false));
}
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ uint32_t dppu(uint32_t old, uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROWS, 0xf, false); }

__device__ __forceinline__ void put8(float *p, const float (&v)[8])
{
    *(f4 *)p = f4{v[0], v[1], v[2], v[3]};
    *(f4 *)(p + 4) = f4{v[4], v[5], v[6], v[7]};
}

// one step of the inclusive segmented scan: lanes whose source lane (DPP CTRL) holds the same key add its sums; false when no lane does
template <int CTRL, int ROWS>
__device__ __forceinline__ bool seg_step(float (&t)[8], uint32_t key)
{
    const bool m = dppu<CTRL, ROWS>(~0u, key) == key;
    if (!__builtin_amdgcn_ballot_w64(m)) return false;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const float n = t[k] + dppf<CTRL, ROWS>(0.f, t[k]);
        t[k] = m ? n : t[k];
    }
    return true;
}

// rk[]: rows relative to the chunk's first block-row, non-decreasing block-rows (rk >> 3) across values and lanes; win zero-filled
__device__ __forceinline__ void seg_reduce(float *win, const uint32_t (&rk)[kPer], const float (&pr)[kPer])
{
    const uint32_t bf = rk[0] >> 3, bl = rk[kPer - 1] >> 3;
    float h[8], t[8];
#pragma unroll
    for (int k = 0; k < 8; k++) h[k] = t[k] = 0.f;
    // in-lane pass: t sums the current block-row; at a block-row change the sums become the head (first block-row) or go to the window
    // (a block-row that begins and ends in this lane)
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) {
        if (j > 0 && (rk[j] >> 3) != (rk[j - 1] >> 3)) {
            const uint32_t bp = rk[j - 1] >> 3;
            if (bp == bf) {
#pragma unroll
                for (int k = 0; k < 8; k++) h[k] = t[k];
            } else {
                put8(win + 8u * bp, t);
            }
#pragma unroll
            for (int k = 0; k < 8; k++) t[k] = 0.f;
        }
        const uint32_t r = rk[j] & 7u;
#pragma unroll
        for (int k = 0; k < 8; k++) t[k] += r == (uint32_t)k ? pr[j] : 0.f;
    }
    // cross-lane pass: inclusive segmented scan of the tail sums keyed by the tail block-row (rows of 16 by row_shr, then row_bcast)
    if (seg_step<0x111, 0xf>(t, bl) && seg_step<0x112, 0xf>(t, bl) && seg_step<0x114, 0xf>(t, bl)) seg_step<0x118, 0xf>(t, bl);
    seg_step<0x142, 0xa>(t, bl);
    seg_step<0x143, 0xc>(t, bl);
    // the left lane's scanned tail continues this lane's head; a block-row is written by the lane where it ends
    const uint32_t bl_left = dppu<0x138>(~0u, bl), bf_right = dppu<0x130>(~0u, bf);
    float tl[8];
#pragma unroll
    for (int k = 0; k < 8; k++) tl[k] = dppf<0x138>(0.f, t[k]);
    if (bf != bl) {
        const bool cont = bl_left == bf;
#pragma unroll
        for (int k = 0; k < 8; k++) h[k] = cont ? h[k] + tl[k] : h[k];
        put8(win + 8u * bf, h);
    }
    if (bf_right != bl) put8(win + 8u * bl, t);
}

// rung k: rung j with the window adds replaced by the segmented reduction.  The tail (own-row y stores, carries, tickets, fold) is rung f's.
__global__ __launch_bounds__(64, 8) void r7_kernel(const Rec *recs, const uint32_t *words, const float *values, const float *x, float *y,
                                                   float *carry, uint32_t *counters, uint32_t nnz, uint32_t num_rows, uint32_t num_cols)
{
    __shared__ __attribute__((aligned(16))) float win[kWin];
    const int lane = threadIdx.x & 63;
    const uint32_t c = blockIdx.x;
    const Rec rc = recs[c];
    const uint32_t first = c * kV + kPer * (uint32_t)lane;
    uint32_t w[kPer];
    float a[kPer], xv[kPer];
    load_chunk(c, lane, words, values, x, nnz, num_cols, w, a, xv);
    float pr[kPer];
    uint32_t rr[kPer];
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) {
        rr[j] = first + j < nnz ? w[j] >> 20 : rc.nwin - 8u;  // past nnz (last chunk): the last block-row, adding 0
        pr[j] = first + j < nnz ? a[j] * xv[j] : 0.f;
    }
    if (rc.nwin == 8) {
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (uint32_t j = 0; j < kPer; j++)
#pragma unroll
            for (int k = 0; k < 8; k++) s[k] += rr[j] == (uint32_t)k ? pr[j] : 0.f;
        const float v = sum8(s, lane);
        if ((lane & 7) == 0) win[((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1)] = v;
    } else {
        for (uint32_t e = (uint32_t)lane; e < rc.nwin; e += 64) win[e] = 0.f;
        __builtin_amdgcn_wave_barrier();
        seg_reduce(win, rr, pr);
    }
    __builtin_amdgcn_wave_barrier();
    const int32_t base = (int32_t)(rc.fb * 8u);
    const uint32_t row_end = min(rc.own_e * 8u, num_rows);
    for (uint32_t row = rc.own_b * 8u + (uint32_t)lane; row < row_end; row += 64) {
        const int32_t rel = (int32_t)row - base;
        y[row] = rel >= 0 && rel < (int32_t)rc.nwin ? win[rel] : 0.f;
    }
    if (!rc.flags) return;
    if ((rc.flags & kHead) && lane < 8) __hip_atomic_store(&carry[((size_t)c * 2) * 8 + lane], win[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((rc.flags & kTail) && lane < 8)
        __hip_atomic_store(&carry[((size_t)c * 2 + 1) * 8 + lane], win[rc.nwin - 8u + (uint32_t)lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    uint32_t ticket = 0;
    if (lane == 0 && (rc.flags & kHead)) ticket = __hip_atomic_fetch_add(&counters[rc.head_ca], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == 1 && (rc.flags & kTail)) ticket = __hip_atomic_fetch_add(&counters[c], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t th = (uint32_t)__builtin_amdgcn_readlane((int)ticket, 0), tt = (uint32_t)__builtin_amdgcn_readlane((int)ticket, 1);
    if ((rc.flags & kHead) && th == rc.head_cb - rc.head_ca) fold(carry, y, counters, rc.head_ca, rc.head_cb, rc.fb, num_rows, lane);
    if ((rc.flags & kTail) && tt == rc.tail_cb - c) fold(carry, y, counters, c, rc.tail_cb, rc.fb + rc.nwin / 8u - 1u, num_rows, lane);
}

#define CK(x)                                                                                 \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } \
    } while (0)

int main()
{
    const uint32_t scale = 20, n = 1u << scale, m = 2u << scale, copies = 9;
    uint64_t z = 12345;
    auto next = [&z]() { z = z * 6364136223846793005ull + 1442695040888963407ull; return (double)(z >> 11) * (1.0 / 9007199254740992.0); };
    std::vector<uint64_t> cells;
    for (uint32_t e = 0; e < m + n; e++) {
        uint32_t r = 0, c = 0;
        if (e < m) {
            for (uint32_t l = 0; l < scale; l++) {
                const double u = next();
                r = (r << 1) | (u >= 0.76 ? 1u : 0u);
                c = (c << 1) | (((u >= 0.57 && u < 0.76) || u >= 0.95) ? 1u : 0u);
            }
        } else {
            r = c = e - m;
        }
        cells.push_back(((uint64_t)(r >> 3) << 43) | ((uint64_t)(c >> 3) << 26) | ((uint64_t)(((r & 7u) << 3) | (c & 7u)) << 20) | c);
    }
    std::sort(cells.begin(), cells.end());
    cells.erase(std::unique(cells.begin(), cells.end()), cells.end());
    const uint32_t nnz = (uint32_t)cells.size(), nch = (nnz + kV - 1) / kV, nbr = n / 8;
    auto brow = [&](uint32_t i) { return (uint32_t)(cells[i] >> 43); };
    // chunk records, as build_chunk_cache makes them
    std::vector<uint32_t> fb(nch), lb(nch);
    for (uint32_t c = 0; c < nch; c++) { fb[c] = brow(c * kV); lb[c] = brow(std::min((c + 1) * kV, nnz) - 1); }
    std::vector<Rec> rec(nch);
    uint32_t hub = 0, folded = 0;
    for (uint32_t c = 0; c < nch; c++) {
        Rec &r = rec[c];
        r.fb = fb[c];
        r.nwin = (lb[c] - fb[c] + 1u) * 8u;
        if (r.nwin > kWin) { printf("chunk %u spans %u rows: beyond the window\n", c, r.nwin); return 1; }
        const bool head = c > 0 && lb[c - 1] == fb[c], tail = c + 1 < nch && fb[c + 1] == lb[c];
        r.own_b = c == 0 ? 0u : fb[c] + (head ? 1u : 0u);
        r.own_e = c + 1 < nch ? fb[c + 1] : nbr;
        r.flags = (head ? kHead : 0) | (tail && !(head && fb[c] == lb[c]) ? kTail : 0);
        r.head_ca = r.head_cb = r.tail_cb = c;
        hub += r.nwin == 8;
        folded += r.flags != 0;
    }
    for (uint32_t c = 0; c < nch; c++) {
        if (!(rec[c].flags & kTail)) continue;
        uint32_t e = c + 1;
        while (e + 1 < nch && fb[e + 1] == lb[c]) e++;
        rec[c].tail_cb = e;
        for (uint32_t k = c + 1; k <= e; k++) { rec[k].head_ca = c; rec[k].head_cb = e; }
    }
    std::vector<uint32_t> hw((size_t)nch * kV, 0);
    std::vector<float> hv((size_t)nch * kV, 0.f), hx(n);
    for (uint32_t i = 0; i < nnz; i++) {
        const uint32_t rel = (brow(i) - fb[i / kV]) * 8u + (uint32_t)((cells[i] >> 23) & 7u);
        hw[i] = (rel << 20) | (uint32_t)(cells[i] & 0xfffffu);
        hv[i] = (float)(0.25 + 0.5 * next());
    }
    for (uint32_t i = 0; i < n; i++) hx[i] = (float)(0.5 + next());
    std::vector<double> yref(n, 0.0);
    for (uint32_t i = 0; i < nnz; i++) yref[brow(i) * 8u + ((cells[i] >> 23) & 7u)] += (double)hv[i] * hx[cells[i] & 0xfffffu];
    printf("nnz %u, chunks %u, hub chunks %u, chunks that fold %u\n", nnz, nch, hub, folded);

    uint32_t *dw[copies], *dcnt;
    float *dv[copies], *dx, *dy, *dout, *dcarry;
    Rec *drec;
    for (uint32_t c = 0; c < copies; c++) {
        CK(hipMalloc((void **)&dw[c], 4ull * hw.size())); CK(hipMemcpy(dw[c], hw.data(), 4ull * hw.size(), hipMemcpyHostToDevice));
        CK(hipMalloc((void **)&dv[c], 4ull * hv.size())); CK(hipMemcpy(dv[c], hv.data(), 4ull * hv.size(), hipMemcpyHostToDevice));
    }
    CK(hipMalloc((void **)&dx, 4ull * n)); CK(hipMemcpy(dx, hx.data(), 4ull * n, hipMemcpyHostToDevice));
    CK(hipMalloc((void **)&dy, 4ull * n));
    CK(hipMalloc((void **)&dout, 4ull * nch * 64));
    CK(hipMalloc((void **)&dcarry, 64ull * nch));
    CK(hipMalloc((void **)&dcnt, 4ull * nch));
    CK(hipMalloc((void **)&drec, sizeof(Rec) * nch)); CK(hipMemcpy(drec, rec.data(), sizeof(Rec) * nch, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int warm = 20, reps = 200;
    auto timed = [&](const char *name, auto launch) -> int {
        CK(hipMemset(dcnt, 0, 4ull * nch));
        for (int it = 0; it < warm; it++) launch(it % copies);
        CK(hipEventRecord(e0, 0));
        for (int it = 0; it < reps; it++) launch(it % copies);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        CK(hipGetLastError());
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        printf("%-44s %7.2f us per launch\n", name, ms * 1e3 / reps);
        return 0;
    };
#define L(...) [&](int k) { hipLaunchKernelGGL(__VA_ARGS__); }
    const char *names[2] = {"j  round-6 kernel (window adds)", "k  j + segmented reduction"};
    auto variant = [&](int v, const char *name) -> int {
        switch (v) {
        case 0: return timed(name, L((r5_kernel<6, true>), dim3(nch), dim3(64), 0, 0, drec, dw[k], dv[k], dx, dy, dout, dcarry, dcnt, nnz, n, n));
        default: return timed(name, L(r7_kernel, dim3(nch), dim3(64), 0, 0, drec, dw[k], dv[k], dx, dy, dcarry, dcnt, nnz, n, n));
        }
    };
    std::vector<std::vector<float>> ys;
    for (int v = 0; v < 2; v++) {
        CK(hipMemset(dy, 0xff, 4ull * n));  // NaN poison: every row must be written
        if (variant(v, names[v])) return 1;
        std::vector<float> h(n);
        CK(hipMemcpy(h.data(), dy, 4ull * n, hipMemcpyDeviceToHost));
        double worst = 0;
        uint32_t bad = 0;
        for (uint32_t i = 0; i < n; i++) {
            if (!std::isfinite(h[i])) bad++;
            worst = std::max(worst, std::fabs(h[i] - yref[i]) / std::max(1e-30, std::fabs(yref[i])));
        }
        uint32_t differ = 0;
        double wf = 0;
        for (uint32_t i = 0; v > 0 && i < n; i++) {
            if (h[i] != ys[0][i]) differ++;
            wf = std::max(wf, (double)std::fabs(h[i] - ys[0][i]) / std::max(1e-30, std::fabs((double)ys[0][i])));
        }
        printf("   non-finite rows %u; largest relative error against the host sum %.3g; against j: %u rows differ, largest relative difference %.3g\n",
               bad, worst, differ, wf);
        if (bad || worst > 1e-5) { printf("   WRONG\n"); return 2; }
        ys.push_back(h);
    }
    for (int rep = 0; rep < 4; rep++)  // again, interleaved, for the spread
        for (int v = 0; v < 2; v++)
            if (variant(v, names[v])) return 1;
    return 0;
}
