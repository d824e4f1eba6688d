// solve_schedule.h -- the two pure rules of an enqueued solve (solve_driver.hip.h applies them): the iteration cap and how many iterations
// go on the stream between two read-backs.  No HIP here: tests/host_solve_schedule_check.cpp runs them on the host.
#pragma once
#include <cstdint>

namespace bmsp {

constexpr int64_t kMaxIter = 1ll << 20;
// Iterations enqueued between two read-backs when BMSP_KRYLOV_CHECK does not say: 1, 2, 4, 8, then 16 per batch.  What is enqueued behind
// a stop is wasted products and preconditioner applications, so a solve of one or two iterations wants 1 and a long one 8 - 16 (measured
// in DESIGN §4 "Krylov solvers"): the ramp reads back after iterations 1, 3, 7, 15, 31, 47, ...
constexpr int64_t kCheckRampMax = 16;

// max_iter == 0 means min(n, 2^20)
inline int64_t cap_of(int64_t n, int64_t max_iter) { return max_iter ? max_iter : (n < kMaxIter ? n : kMaxIter); }

// How many iterations are enqueued next when `done` of `cap` are: `fixed` of them (BMSP_KRYLOV_CHECK; the cap itself under NO_CHECK), or
// under the ramp (fixed == 0) done + 1 up to 16 -- the batches double from 1, so done is 0, 1, 3, 7, 15 when they do -- cut at the cap.
inline int64_t next_batch(int64_t cap, int64_t fixed, int64_t done)
{
    const int64_t check = fixed ? fixed : (done + 1 < kCheckRampMax ? done + 1 : kCheckRampMax);
    return check < cap - done ? check : cap - done;
}

}  // namespace bmsp
