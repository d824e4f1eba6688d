// dot_tree.hip.h -- what the solvers share on the device (krylov.hip: bmsp_vec_dot, CG, BiCGStab; gmres.hip: GMRES(m)): the fixed two-level
// tree of the dot product, the hand-off that lets the last workgroup finish it, the stop rule and the bb / thr step of a solve, and the
// record; with them the host-side rules of the tree (chunks, the ticket threshold).  The host side of a solve is solve_driver.hip.h.
// include/bmsp.h writes the tree out; tests/krylov_ref.c restates it.
#pragma once
#include "solve_schedule.h"
#include "sweep_stats.hip.h"
#include <cstring>

namespace bmsp {
namespace {

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

// ---- the scalars of a solve: State is KrylovState or GmresState, whose kernels read `stopped` first ----
template <typename State>
__device__ __forceinline__ void stop(State *S, int status)
{
    S->status = status;
    S->stopped = 1;
}

// The stop rule on a residual dot, three ways; before_breakdown() runs first on the two breakdown branches.  True if the solve goes on.
// (rr == 0 above thr: NO_CHECK, thr < 0)
struct NothingBefore {
    __device__ __forceinline__ void operator()() const {}
};
template <typename State, typename Before = NothingBefore>
__device__ __forceinline__ bool residual_verdict(State *S, double rr, Before before_breakdown = Before())
{
    if (!__builtin_isfinite(rr)) {
        before_breakdown();
        stop(S, BMSP_KRYLOV_BREAKDOWN);
    } else if (rr <= S->thr) {
        stop(S, BMSP_KRYLOV_CONVERGED);
    } else if (rr == 0.0) {
        before_breakdown();
        stop(S, BMSP_KRYLOV_BREAKDOWN);
    } else {
        return true;
    }
    return false;
}

// bb = dot(b, b) has been formed: thr = fl(tol2 * bb), or -1 under NO_CHECK (tol2 < 0); the zero and the non-finite stops, in that order;
// go_on() where neither fell.
template <typename State, typename GoOn>
__device__ __forceinline__ void bb_step(State *S, double bb, double tol2, GoOn go_on)
{
#pragma clang fp contract(off)
    S->bb = bb;
    const double thr = tol2 * bb;
    S->thr = tol2 < 0.0 ? -1.0 : thr;
    if (bb == 0.0) return stop(S, BMSP_KRYLOV_CONVERGED);
    if (!__builtin_isfinite(bb)) return stop(S, BMSP_KRYLOV_BREAKDOWN);
    go_on();
}

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
