// sweep_stats.hip.h -- the per-sweep statistics and the stop protocol that the fixed-point iterations share (spitsv.hip: block-Jacobi
// sweeps of a triangular solve; ilu0.hip: sweeps towards the incomplete factor).  A sweep is one launch; it leaves one record: whether any
// entry changed in bits, the largest |new - old| and the largest |new|, the latter two as the bits of a non-negative floating-point
// number, which order like an unsigned integer -- so the record is built by integer atomics, does not depend on arrival order, and
// there is no floating-point atomic.  Sweep k + 1 begins by evaluating the stop rule on record k and returns without writing when it
// holds; the host evaluates the same predicate on the records it reads back.
#ifndef BMSP_SWEEP_STATS_HIP_H_
#define BMSP_SWEEP_STATS_HIP_H_

#include "tile_pass.hip.h"

namespace bmsp {

// One sweep's statistics: the bits of max |x_new - x_old| and of max |x_new| in the vector type (widened to 64 bits), and whether any
// x_i changed in bits.  All zero = the sweep did not run.
struct SweepRecord {
    unsigned long long delta, xmax, changed, pad;
};

template <typename R>
struct VecBits;
template <>
struct VecBits<float> {
    static __host__ __device__ float from(unsigned long long u) { return __builtin_bit_cast(float, (uint32_t)u); }
};
template <>
struct VecBits<double> {
    static __host__ __device__ double from(unsigned long long u) { return __builtin_bit_cast(double, (uint64_t)u); }
};

// stop after the sweep of record r iff nothing changed, or (tol > 0 and) delta <= fl(tol * xmax): in the vector type, tol rounded once
template <typename R>
__host__ __device__ __forceinline__ bool stop_rule(const SweepRecord &r, R tol)
{
#pragma clang fp contract(off)
    if (!r.changed) return true;
    if (!(tol > R(0))) return false;
    const R bound = tol * VecBits<R>::from(r.xmax);
    return VecBits<R>::from(r.delta) <= bound;
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, kWave);
        v = o > v ? o : v;
    }
    return v;
}

// The three statistics of every lane of a workgroup into the sweep's record: reduced across the wave in registers and across the
// workgroup's four waves through LDS, then ONE lane issues at most one integer atomic per statistic.  Every lane of the workgroup must
// call it (it holds a barrier).
__device__ __forceinline__ void sweep_publish(unsigned long long changed, unsigned long long delta, unsigned long long xmax, SweepRecord *mine)
{
    changed = wave_max(changed);
    delta = wave_max(delta);
    xmax = wave_max(xmax);
    __shared__ unsigned long long part[3][kThreads / kWave];
    if (lane_id() == 0) {
        part[0][wave_id()] = changed;
        part[1][wave_id()] = delta;
        part[2][wave_id()] = xmax;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long v = part[threadIdx.x][0];
#pragma unroll
        for (int w = 1; w < kThreads / kWave; w++) v = part[threadIdx.x][w] > v ? part[threadIdx.x][w] : v;
        // a maximum only grows: a workgroup whose value the record already covers has nothing to add, and same-address atomics serialise
        // at the memory side.  The look is a relaxed device-scope load; a value older than the record's is smaller, never larger.
        unsigned long long *slot = threadIdx.x == 0 ? &mine->changed : (threadIdx.x == 1 ? &mine->delta : &mine->xmax);
        if (v > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            if (threadIdx.x == 0) atomicOr(slot, 1ull);
            else atomicMax(slot, v);
        }
    }
}

// sweeps enqueued between two read-backs: the value of `var` when it parses and is >= 1, else `fallback` (read per call)
inline int64_t sweep_check_from_env(const char *var, int64_t fallback)
{
    if (const char *e = getenv(var)) {
        char *end = nullptr;
        const long long c = strtoll(e, &end, 10);
        if (end != e && c >= 1) return (int64_t)c;
    }
    return fallback;
}

}  // namespace bmsp
#endif
