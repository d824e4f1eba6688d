// dot_tree.hip.h -- what the solvers share (krylov.hip: bmsp_vec_dot, CG, BiCGStab; gmres.hip: GMRES(m)): the fixed two-level tree of
// the dot product, the hand-off that lets the last workgroup finish it, and the host-side rules of a solve (chunks, the ticket
// threshold, the check ramp, the record).  include/bmsp.h writes the tree out; tests/krylov_ref.c restates it.
#pragma once
#include "sweep_stats.hip.h"
#include <cstring>

namespace bmsp {
namespace {

constexpr int64_t kMaxIter = 1ll << 20;
// Iterations enqueued between two read-backs when BMSP_KRYLOV_CHECK does not say: 1, 2, 4, 8, then 16 per batch.  What is enqueued behind
// a stop is wasted products and preconditioner applications, so a solve of one or two iterations wants 1 and a long one 8 - 16 (measured
// in DESIGN §4 "Krylov solvers"): the ramp reads back after iterations 1, 3, 7, 15, 31, 47, ...
constexpr int64_t kCheckRampMax = 16;
constexpr int kChunk = 4 * kThreads;  // elements per workgroup: lane t takes base + 256 q + t, q = 0..3
// The second level of a dot runs in the last arriver up to this many chunks and as a launch of its own beyond: the tickets are
// same-address atomics and serialise at the memory side, about 11 ns each.  Measured, us per dot, ticket / launch: 64 chunks 5.5 / 8.6,
// 128 chunks 5.3 / 8.2, 256 chunks 6.4 / 9.1, 2048 chunks 28.9 / 8.1 (DESIGN §4 "Krylov solvers").  Nothing was measured between 256
// and 2048 chunks: 384 is interpolated from those points (2.7 us saved by the launch, 11 ns per ticket beyond 128 chunks).
// BMSP_VEC_DOT_FINISH=ticket|launch forces one (read per call); the bits are the same.
constexpr int64_t kTicketMaxChunks = 384;

// one per iteration: the residual dot it recorded; written = 1 once it has
struct KrylovRecord {
    double rr;
    long long written;
};

// ---- the dot tree ----
__device__ __forceinline__ double wave_butterfly(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, kWave);
    return v;
}

// The 256 accumulators of a workgroup: the butterfly inside every wave, then the four wave sums in ascending order.  Every lane returns
// the sum.  Every lane of the workgroup must call it (two barriers).
__device__ __forceinline__ double group_sum(double acc, double *lds4)
{
    acc = wave_butterfly(acc);
    __syncthreads();  // (a previous use of lds4 has been read)
    if (lane_id() == 0) lds4[wave_id()] = acc;
    __syncthreads();
    return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}

// second level: lane t adds P[t], P[t + 256], ... in ascending order, then the same tree
__device__ __forceinline__ double finish_sum(const double *P, uint32_t chunks, double *lds4)
{
    double acc = 0.0;
    for (uint32_t c = threadIdx.x; c < chunks; c += kThreads) acc = acc + __hip_atomic_load(&P[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return group_sum(acc, lds4);
}

// Leaves this workgroup's NACC partials in P[a * chunks + blockIdx.x] and draws a ticket.  True in every lane of the workgroup that
// arrived last, with acc[] replaced by the finished sums; it has reset the ticket.  gridDim.x == chunks.
template <int NACC>
__device__ __forceinline__ bool publish_and_finish(double (&acc)[NACC], double *P, uint32_t chunks, uint32_t *ticket, double *lds4)
{
    __shared__ uint32_t last;
#pragma unroll
    for (int a = 0; a < NACC; a++) acc[a] = group_sum(acc[a], lds4);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < NACC; a++) __hip_atomic_store(&P[(size_t)a * chunks + blockIdx.x], acc[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == chunks - 1u;
    }
    __syncthreads();
    if (!last) return false;
#pragma unroll
    for (int a = 0; a < NACC; a++) acc[a] = finish_sum(P + (size_t)a * chunks, chunks, lds4);
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

template <typename R>
__device__ __forceinline__ double dot_term(R x, R y, double acc)
{
    return __builtin_fma((double)x, (double)y, acc);
}

__device__ __forceinline__ bool bad_denominator(double v) { return v == 0.0 || !__builtin_isfinite(v); }

// whether the last arriver finishes a dot of `chunks` chunks (else a launch of its own does)
bool finish_by_ticket(int64_t chunks)
{
    if (const char *e = getenv("BMSP_VEC_DOT_FINISH")) {
        if (!strcmp(e, "launch")) return false;
        if (!strcmp(e, "ticket")) return true;
    }
    return chunks <= kTicketMaxChunks;
}

bool no_check(double tol) { return tol == BMSP_KRYLOV_NO_CHECK; }
size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }
int64_t chunks_of(int64_t n) { return (n + kChunk - 1) / kChunk; }

}  // namespace
}  // namespace bmsp
