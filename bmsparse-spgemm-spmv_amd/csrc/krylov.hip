// krylov.hip -- the vector side of a Krylov iteration and the two solvers built on it (bmsp_vec_dot, bmsp_vec_axpby, bmsp_krylov_solve).
// Products and preconditioners are the library's own calls (bmsp_spmv_op, bmsp_matrix_diagonal, bmsp_spsv, bmsp_spitsv); what is new:
//   the dot product   a fixed two-level tree (include/bmsp.h writes it out, tests/krylov_ref.c restates it): a workgroup per chunk of
//       1024 elements leaves one partial; the workgroup that draws the last ticket sums the partials in the same tree.  The hand-off is
//       spmv_chunk_kernel's fold hand-off: the partial goes out as an agent-scope store, the store is drained, the ticket is an
//       agent-scope integer add; the last arriver reads every partial with agent-scope loads and resets the ticket.  Nothing waits.
//       Beyond kTicketMaxChunks chunks the second level (and the scalar step behind it) is a launch of its own: same tree, same bits.
//   krylov_step_kernel<R, STEP>   every vector operation of CG and BiCGStab as one instantiation: the element-wise updates of a step,
//       the partial sums of the dots that follow them (same chunks, same lanes, so the bits are bmsp_vec_dot's on the updated vectors)
//       and -- in the last arriver's thread 0 -- the scalar step: alpha, beta, omega by one IEEE division each, the stop rule, the
//       breakdown tests, the record.  A launch per step; the scalars never leave the device.
//   termination on the device   every instantiation begins by reading `stopped` and returns without writing once it is set.  The host
//       enqueues BMSP_KRYLOV_CHECK iterations, reads the state back and goes on or stops; what it enqueued behind a stop did nothing
//       to x.
//   the host side   solve_driver.hip.h, shared with gmres.hip: the preconditioner, the workspace, the start, the batches, the info.
//       run_solve keeps the workspace layout, StepArgs, the start tail (r^ = r, or the first z and p) and the launches of one iteration.
#include "solve_driver.hip.h"
#include <map>
#include <mutex>
#include <utility>

namespace bmsp {
namespace {

// The scalars of one solve, device-resident.  `stopped` is what every kernel reads first; `status` is a BMSP_KRYLOV_* value.
struct KrylovState {
    double bb, thr, rho, alpha, beta, omega, rr;
    long long iterations, products, applies;
    int status, stopped;
    uint32_t ticket, pad;
};
// (the dot tree, the ticket hand-off, stop, residual_verdict, bb_step and KrylovRecord: dot_tree.hip.h)

// bmsp_vec_dot, first level (and the second under TICKET)
template <typename R, bool TICKET>
__global__ __launch_bounds__(kThreads) void vec_dot_kernel(const R *__restrict__ x, const R *__restrict__ y, int64_t n, double *P, uint32_t chunks,
                                                           uint32_t *ticket, double *result)
{
    __shared__ double lds4[4];
    double acc[1] = {0.0};
    const int64_t base = (int64_t)blockIdx.x * kChunk;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int64_t i = base + q * kThreads + (int64_t)threadIdx.x;
        if (i < n) acc[0] = dot_term(x[i], y[i], acc[0]);
    }
    if (TICKET) {
        if (publish_and_finish<1>(acc, P, chunks, ticket, lds4) && threadIdx.x == 0) *result = acc[0];
    } else {
        const double s = group_sum(acc[0], lds4);
        if (threadIdx.x == 0) P[blockIdx.x] = s;
    }
}

// the second level as a launch of its own (BMSP_VEC_DOT_FINISH=launch); chunks == 0 writes +0
__global__ __launch_bounds__(kThreads) void vec_dot_finish_kernel(const double *P, uint32_t chunks, double *result)
{
    __shared__ double lds4[4];
    const double s = finish_sum(P, chunks, lds4);
    if (threadIdx.x == 0) *result = s;
}

template <typename R>
__global__ __launch_bounds__(kThreads) void vec_axpby_kernel(R a, const R *x, R b, R *y, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + (int64_t)threadIdx.x;
    if (i < n) y[i] = spmv_op_epilogue<R>(a, x[i], b, y, i);
}

// ---- the steps of the two methods ----
// Vector slots of the workspace.  CG: r, z, p, q.  BiCGStab: r, rh, p, v, s, t, ph, sh.  The product of the start (op(A) x0) lands in
// slot 3 for both.  With BMSP_PC_NONE z is r, ph is p and sh is s (the pointers alias; nothing is copied).
enum { kR = 0, kZ = 1, kP = 2, kQ = 3, kRh = 1, kV = 3, kS = 4, kT = 5, kPh = 6, kSh = 7 };
enum Step {
    kStepBB,     // bb = dot(b, b); thr; without x0: the start's residual test and rho (r = b)
    kStepR0,     // r = b - slot3; rr0 = dot(r, r): the start's residual test and rho
    kStepZeroX,  // x = 0 if the solve stopped on bb == 0 (the one kernel that writes after a stop)
    kStepJacobi, // z = r / d; rho' = dot(r, z)
    kStepDotRZ,  // rho' = dot(r, z)
    kStepDotPQ,  // alpha = rho / dot(p, q)
    kStepCgXR,   // x += aR p; r -= aR q; rr = dot(r, r): record, stop?
    kStepCgP,    // p = z (first) or z + bR p
    kStepBiP,    // p = r (k = 1) or r + bR (p - wR v); under Jacobi ph = p / d
    kStepDotRhV, // alpha = rho / dot(rh, v)
    kStepBiSX,   // s = r - aR v; x += aR ph; dot(s, s) <= thr: record, converged; under Jacobi sh = s / d
    kStepDotTT,  // omega = dot(t, s) / dot(t, t)
    kStepBiXR    // x += wR sh; r = s - wR t; rr = dot(r, r): record, stop?; rho' = dot(rh, r)
};
constexpr int step_dots(int step)
{
    return step == kStepZeroX || step == kStepCgP || step == kStepBiP ? 0 : (step == kStepDotTT || step == kStepBiXR ? 2 : 1);
}

template <typename R>
struct StepArgs {
    KrylovState *S;
    KrylovRecord *rec;  // null under NO_CHECK
    double *P;          // 2 * chunks partials
    const R *b, *d;     // d: the diagonal (Jacobi)
    R *x;
    R *v[8];
    int64_t n, k;       // k: the iteration, 1-based; 0 = the start
    uint32_t chunks;
    int pc, bicg;
    int ticket;         // 1: the last arriver finishes the dots and takes the scalar step; 0: krylov_finish_kernel does
    double tol2;        // fl(tol * tol), or negative under NO_CHECK
};

// The residual dot of iteration k (0: of the start, which leaves no record).  True if the iteration goes on.
template <typename R>
__device__ __forceinline__ bool residual_step(const StepArgs<R> &a, double rr)
{
    KrylovState *S = a.S;
    S->rr = rr;
    if (a.k > 0) {
        S->iterations = a.k;
        if (a.rec) {
            a.rec[a.k - 1].rr = rr;
            a.rec[a.k - 1].written = 1;
        }
    }
    residual_verdict(S, rr);
    return !S->stopped;
}

// rho' has been formed: beta from it and the old rho (not at the start), then rho = rho'
template <typename R>
__device__ __forceinline__ void rho_step(const StepArgs<R> &a, double rho_new)
{
#pragma clang fp contract(off)
    KrylovState *S = a.S;
    if (bad_denominator(rho_new)) return stop(S, BMSP_KRYLOV_BREAKDOWN);
    if (a.k > 0) {
        double beta = rho_new / S->rho;
        if (a.bicg) {
            const double aw = S->alpha / S->omega;
            beta = beta * aw;
        }
        S->beta = beta;
    }
    S->rho = rho_new;
}

template <typename R, int STEP>
__device__ __forceinline__ void scalar_step(const StepArgs<R> &a, double s0, double s1)
{
#pragma clang fp contract(off)
    KrylovState *S = a.S;
    const bool none = a.pc == BMSP_PC_NONE;
    if (STEP == kStepBB) {
        bb_step(S, s0, a.tol2, [&]() {
            if (a.x) return;  // (x0 given: kStepR0 follows)
            if (residual_step(a, s0) && (none || a.bicg)) rho_step(a, s0);
        });
    } else if (STEP == kStepR0) {
        S->products++;
        if (residual_step(a, s0) && (none || a.bicg)) rho_step(a, s0);
    } else if (STEP == kStepJacobi || STEP == kStepDotRZ) {
        S->applies++;
        rho_step(a, s0);
    } else if (STEP == kStepDotPQ || STEP == kStepDotRhV) {
        S->products++;
        if (STEP == kStepDotRhV && !none) S->applies++;
        if (bad_denominator(s0)) return stop(S, BMSP_KRYLOV_BREAKDOWN);
        S->alpha = S->rho / s0;
    } else if (STEP == kStepCgXR) {
        if (residual_step(a, s0) && none) rho_step(a, s0);
    } else if (STEP == kStepBiSX) {  // (S->rr stays the last recorded residual unless the half step converges)
        if (!__builtin_isfinite(s0)) return stop(S, BMSP_KRYLOV_BREAKDOWN);
        if (s0 <= S->thr) {
            residual_step(a, s0);
        } else if (s0 == 0.0) {
            stop(S, BMSP_KRYLOV_BREAKDOWN);
        }
    } else if (STEP == kStepDotTT) {
        S->products++;
        if (!none) S->applies++;
        if (bad_denominator(s1)) return stop(S, BMSP_KRYLOV_BREAKDOWN);
        const double omega = s0 / s1;
        S->omega = omega;
        if (bad_denominator(omega)) stop(S, BMSP_KRYLOV_BREAKDOWN);
    } else if (STEP == kStepBiXR) {
        if (residual_step(a, s0)) rho_step(a, s1);
    }
}

// element i of a step: each operation rounded on its own
template <typename R, int STEP>
__device__ __forceinline__ void element_step(const StepArgs<R> &a, int64_t i, R aR, R bR, R wR, double (&acc)[2])
{
#pragma clang fp contract(off)
    R *const *v = a.v;
    const bool jacobi = a.pc == BMSP_PC_JACOBI;
    if (STEP == kStepBB) {
        acc[0] = dot_term(a.b[i], a.b[i], acc[0]);
    } else if (STEP == kStepR0) {
        const R r = a.b[i] - v[3][i];
        v[kR][i] = r;
        acc[0] = dot_term(r, r, acc[0]);
    } else if (STEP == kStepZeroX) {
        a.x[i] = R(0);
    } else if (STEP == kStepJacobi) {
        const R r = v[kR][i], z = r / a.d[i];
        v[kZ][i] = z;
        acc[0] = dot_term(r, z, acc[0]);
    } else if (STEP == kStepDotRZ) {
        acc[0] = dot_term(v[kR][i], v[kZ][i], acc[0]);
    } else if (STEP == kStepDotPQ) {
        acc[0] = dot_term(v[kP][i], v[kQ][i], acc[0]);
    } else if (STEP == kStepCgXR) {
        const R ap = aR * v[kP][i], aq = aR * v[kQ][i];
        a.x[i] = a.x[i] + ap;
        const R r = v[kR][i] - aq;
        v[kR][i] = r;
        acc[0] = dot_term(r, r, acc[0]);
    } else if (STEP == kStepCgP) {
        R p = v[kZ][i];
        if (a.k > 0) {
            const R bp = bR * v[kP][i];
            p = p + bp;
        }
        v[kP][i] = p;
    } else if (STEP == kStepBiP) {
        R p = v[kR][i];
        if (a.k > 1) {
            const R wv = wR * v[kV][i];
            const R t = v[kP][i] - wv;
            const R bt = bR * t;
            p = p + bt;
        }
        v[kP][i] = p;
        if (jacobi) v[kPh][i] = p / a.d[i];
    } else if (STEP == kStepDotRhV) {
        acc[0] = dot_term(v[kRh][i], v[kV][i], acc[0]);
    } else if (STEP == kStepBiSX) {
        const R av = aR * v[kV][i], ap = aR * v[kPh][i];
        const R s = v[kR][i] - av;
        v[kS][i] = s;
        a.x[i] = a.x[i] + ap;
        if (jacobi) v[kSh][i] = s / a.d[i];
        acc[0] = dot_term(s, s, acc[0]);
    } else if (STEP == kStepDotTT) {
        const R t = v[kT][i];
        acc[0] = dot_term(t, v[kS][i], acc[0]);
        acc[1] = dot_term(t, t, acc[1]);
    } else if (STEP == kStepBiXR) {
        const R ws = wR * v[kSh][i], wt = wR * v[kT][i];
        a.x[i] = a.x[i] + ws;
        const R r = v[kS][i] - wt;
        v[kR][i] = r;
        acc[0] = dot_term(r, r, acc[0]);
        acc[1] = dot_term(v[kRh][i], r, acc[1]);
    }
}

// One step over chunk blockIdx.x of the vectors; gridDim.x == a.chunks.
template <typename R, int STEP>
__global__ __launch_bounds__(kThreads) void krylov_step_kernel(StepArgs<R> a)
{
    KrylovState *S = a.S;
    if (STEP == kStepZeroX) {
        if (!(S->stopped && S->bb == 0.0)) return;
    } else if (STEP != kStepBB && S->stopped) {
        return;  // (every lane of the grid reads the same word, written by an earlier launch: all leave or none)
    }
    __shared__ double lds4[4];
    double acc[2] = {0.0, 0.0};
    const R aR = (R)S->alpha, bR = (R)S->beta, wR = (R)S->omega;  // rounded once
    const int64_t base = (int64_t)blockIdx.x * kChunk;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int64_t i = base + q * kThreads + (int64_t)threadIdx.x;
        if (i < a.n) element_step<R, STEP>(a, i, aR, bR, wR, acc);
    }
    constexpr int NACC = step_dots(STEP);
    if (NACC == 0) return;
    double part[NACC ? NACC : 1];
#pragma unroll
    for (int j = 0; j < NACC; j++) part[j] = acc[j];
    if (!a.ticket) {
#pragma unroll
        for (int j = 0; j < NACC; j++) {
            const double s = group_sum(part[j], lds4);
            if (threadIdx.x == 0) a.P[(size_t)j * a.chunks + blockIdx.x] = s;
        }
        return;
    }
    if (!publish_and_finish<(NACC ? NACC : 1)>(part, a.P, a.chunks, &S->ticket, lds4)) return;
    if (threadIdx.x == 0) scalar_step<R, STEP>(a, part[0], NACC > 1 ? part[NACC > 1 ? 1 : 0] : 0.0);
}

// The second level of a step's dots and its scalar step as a launch of its own (one workgroup), for vectors of many chunks.
template <typename R, int STEP>
__global__ __launch_bounds__(kThreads) void krylov_finish_kernel(StepArgs<R> a)
{
    KrylovState *S = a.S;
    if (STEP != kStepBB && S->stopped) return;  // (what the step's own launch saw: it does not write the state)
    __shared__ double lds4[4];
    constexpr int NACC = step_dots(STEP);
    double sum[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < NACC; j++) sum[j] = finish_sum(a.P + (size_t)j * a.chunks, a.chunks, lds4);
    if (threadIdx.x == 0) scalar_step<R, STEP>(a, sum[0], sum[1]);
}

template <typename R, int STEP>
void launch_step(const StepArgs<R> &a, hipStream_t st)
{
    hipLaunchKernelGGL((krylov_step_kernel<R, STEP>), dim3(a.chunks), dim3(kThreads), 0, st, a);
    BMSP_CHECK_LAUNCH();
    if constexpr (step_dots(STEP) > 0) {
        if (!a.ticket) {
            hipLaunchKernelGGL((krylov_finish_kernel<R, STEP>), dim3(1), dim3(kThreads), 0, st, a);
            BMSP_CHECK_LAUNCH();
        }
    }
}

// The scratch of bmsp_vec_dot: ticket | partials, one per (device, stream), grown to the largest n seen there and kept for the life of
// the process.  Calls on one stream are ordered by the stream; calls on different streams share nothing; the mutex serialises the
// enqueueing, so calls from several threads do not interleave on one scratch.
struct DotScratch {
    void *mem = nullptr;
    int64_t chunks = 0;
};
std::mutex g_dot_mu;
std::map<std::pair<int, hipStream_t>, DotScratch> g_dot_scratch;

template <typename R>
void run_solve(const SolveCall &c, int method)
{
    bmsp_matrix_s *A = c.A;
    const hipStream_t st = c.st;
    const int64_t n = A->num_rows, m = c.cap;
    const int kind = c.kind();
    const bool bicg = method == BMSP_KRYLOV_BICGSTAB, checked = c.checked(), applied = c.applied();
    const int nvec = bicg ? 8 : 4;
    const int64_t chunks = chunks_of(n);
    // workspace: state | partials | diagonal | vectors | records
    const size_t vbytes = round256(sizeof(R) * (size_t)n);
    const size_t off_P = round256(sizeof(KrylovState)), off_d = off_P + round256(sizeof(double) * 2 * (size_t)chunks);
    const size_t off_v = off_d + vbytes, off_rec = off_v + vbytes * (size_t)nvec;
    char *ws = grow_workspace(A, off_rec + (checked ? sizeof(KrylovRecord) * (size_t)m : 0), st);
    StepArgs<R> a{};
    a.S = (KrylovState *)ws;
    a.rec = checked ? (KrylovRecord *)(ws + off_rec) : nullptr;
    a.P = (double *)(ws + off_P);
    a.b = (const R *)c.b;
    a.d = (const R *)(ws + off_d);
    a.x = (R *)c.x;
    for (int j = 0; j < nvec; j++) a.v[j] = (R *)(ws + off_v + vbytes * (size_t)j);
    if (kind == BMSP_PC_NONE) {
        if (bicg) { a.v[kPh] = a.v[kP]; a.v[kSh] = a.v[kS]; }
        else a.v[kZ] = a.v[kR];
    }
    a.n = n; a.k = 0; a.chunks = (uint32_t)chunks; a.pc = kind; a.bicg = bicg ? 1 : 0;
    a.tol2 = c.tol2();
    a.ticket = finish_by_ticket(chunks) ? 1 : 0;
    begin_info(c, bicg ? "bicgstab" : "cg");
    const auto apply = [&](const R *in, R *tmp, R *out) { pc_apply(c, in, tmp, out, &a.S->stopped); };
    // z = M^-1 r and rho' = dot(r, z), then the next p (CG; with BMSP_PC_NONE z is r and rho' came with the residual)
    const auto next_p = [&]() {
        if (kind == BMSP_PC_JACOBI) launch_step<R, kStepJacobi>(a, st);
        else if (applied) {
            apply(a.v[kR], a.v[kQ], a.v[kZ]);
            launch_step<R, kStepDotRZ>(a, st);
        }
        launch_step<R, kStepCgP>(a, st);
    };
    KrylovState hs{};
    const bool finished = solve_start(
        c, a.S, a.rec, a.d, a.v[kR], hs,
        [&]() {
            StepArgs<R> s = a;
            if (!c.x0()) s.x = nullptr;  // (kStepBB: the start's residual is b's)
            launch_step<R, kStepBB>(s, st);
        },
        [&]() { launch_step<R, kStepZeroX>(a, st); },
        [&]() {
            product(c, a.x, a.v[3]);
            launch_step<R, kStepR0>(a, st);
        });
    if (!finished) {
        if (bicg) BMSP_HIP(hipMemcpyAsync(a.v[kRh], a.v[kR], sizeof(R) * (size_t)n, hipMemcpyDeviceToDevice, st));
        else next_p();
        solve_iterations(c, a.S, hs, [&](int64_t k) {
            a.k = k;
            if (!bicg) {
                product(c, a.v[kP], a.v[kQ]);
                launch_step<R, kStepDotPQ>(a, st);
                launch_step<R, kStepCgXR>(a, st);
                if (k < m) next_p();  // (prepares the next iteration)
            } else {
                launch_step<R, kStepBiP>(a, st);
                if (applied) apply(a.v[kP], a.v[kSh], a.v[kPh]);
                product(c, a.v[kPh], a.v[kV]);
                launch_step<R, kStepDotRhV>(a, st);
                launch_step<R, kStepBiSX>(a, st);
                if (applied) apply(a.v[kS], a.v[kT], a.v[kSh]);
                product(c, a.v[kSh], a.v[kT]);
                launch_step<R, kStepDotTT>(a, st);
                launch_step<R, kStepBiXR>(a, st);
            }
        });
    }
    if (!checked) return no_check_info(c, bicg ? 2 * m : m, bicg ? 2 * m : m);
    checked_info(c, a.rec, hs);
}

}  // namespace

void vec_check_args(int64_t n, int vec_f64)
{
    if (n < 0) fail(BMSP_ERR_INVALID, "n must be >= 0 (got %lld)", (long long)n);
    if (vec_f64 != 0 && vec_f64 != 1) fail(BMSP_ERR_INVALID, "vec_f64 must be 0 (float) or 1 (double) (got %d)", vec_f64);
}

void vec_dot(int64_t n, int vec_f64, const void *x, const void *y, double *result, hipStream_t st)
{
    if (!result) fail(BMSP_ERR_INVALID, "d_result is null");
    if (n > 0 && (!x || !y)) fail(BMSP_ERR_INVALID, "%s is null", !x ? "d_x" : "d_y");
    const int64_t chunks = chunks_of(n);
    if (chunks >= (1ll << 31)) fail(BMSP_ERR_LIMIT, "vec_dot: n %lld needs more than 2^31 chunks", (long long)n);
    if (chunks == 0) {
        BMSP_HIP(hipMemsetAsync(result, 0, sizeof(double), st));
        return;
    }
    int dev = 0;
    BMSP_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_dot_mu);
    DotScratch &sc = g_dot_scratch[std::make_pair(dev, st)];
    if (chunks > sc.chunks) {
        if (sc.mem) BMSP_HIP(hipStreamSynchronize(st));  // (a dot enqueued on the old scratch has finished before it goes back to the pool)
        pool_free(sc.mem);
        sc.mem = nullptr;
        sc.chunks = 0;
        sc.mem = pool_alloc(256 + sizeof(double) * (size_t)chunks);
        BMSP_HIP(hipMemsetAsync(sc.mem, 0, 256, st));  // (the ticket; ordered before the dot by the stream)
        sc.chunks = chunks;
    }
    uint32_t *ticket = (uint32_t *)sc.mem;
    double *P = (double *)((char *)sc.mem + 256);
    const bool by_launch = !finish_by_ticket(chunks);
    const auto go = [&](auto r) {
        using R = decltype(r);
        if (by_launch) {
            hipLaunchKernelGGL((vec_dot_kernel<R, false>), dim3((uint32_t)chunks), dim3(kThreads), 0, st, (const R *)x, (const R *)y, n, P, (uint32_t)chunks, ticket, result);
            BMSP_CHECK_LAUNCH();
            hipLaunchKernelGGL(vec_dot_finish_kernel, dim3(1), dim3(kThreads), 0, st, (const double *)P, (uint32_t)chunks, result);
        } else {
            hipLaunchKernelGGL((vec_dot_kernel<R, true>), dim3((uint32_t)chunks), dim3(kThreads), 0, st, (const R *)x, (const R *)y, n, P, (uint32_t)chunks, ticket, result);
        }
        BMSP_CHECK_LAUNCH();
    };
    if (vec_f64) go(double{});
    else go(float{});
}

void vec_axpby(int64_t n, int vec_f64, double a, const void *x, double b, void *y, hipStream_t st)
{
    if (n == 0) return;
    if (!x || !y) fail(BMSP_ERR_INVALID, "%s is null", !x ? "d_x" : "d_y");
    if (n >= (1ll << 39)) fail(BMSP_ERR_LIMIT, "vec_axpby: n %lld", (long long)n);
    const dim3 grid((uint32_t)((n + kThreads - 1) / kThreads));
    if (vec_f64) hipLaunchKernelGGL(vec_axpby_kernel<double>, grid, dim3(kThreads), 0, st, a, (const double *)x, b, (double *)y, n);
    else hipLaunchKernelGGL(vec_axpby_kernel<float>, grid, dim3(kThreads), 0, st, (float)a, (const float *)x, (float)b, (float *)y, n);
    BMSP_CHECK_LAUNCH();
}

void krylov_check_args(int op, int method, const bmsp_precond *pc, int64_t max_iter, double tol, int flags, const double *relres_history)
{
    spmv_op_check_op(op);
    if (method != BMSP_KRYLOV_CG && method != BMSP_KRYLOV_BICGSTAB)
        fail(BMSP_ERR_INVALID, "method must be BMSP_KRYLOV_CG (0) or BMSP_KRYLOV_BICGSTAB (1) (got %d)", method);
    if (pc && (pc->kind < BMSP_PC_NONE || pc->kind > BMSP_PC_ILU_SWEEPS))
        fail(BMSP_ERR_INVALID, "pc->kind must be BMSP_PC_NONE (0), _JACOBI (1), _ILU_EXACT (2) or _ILU_SWEEPS (3) (got %d)", pc->kind);
    if (pc && pc->kind == BMSP_PC_ILU_SWEEPS && (pc->sweeps < 1 || pc->sweeps > kMaxIter))
        fail(BMSP_ERR_INVALID, "pc->sweeps must be 1 .. 2^20 under BMSP_PC_ILU_SWEEPS (got %lld)", (long long)pc->sweeps);
    if (max_iter < 0 || max_iter > kMaxIter) fail(BMSP_ERR_INVALID, "max_iter must be 0 (min(n, 2^20)) or 1 .. 2^20 (got %lld)", (long long)max_iter);
    if (std::isnan(tol) || (tol < 0.0 && !no_check(tol))) fail(BMSP_ERR_INVALID, "tol must be >= 0 or BMSP_KRYLOV_NO_CHECK (-1.0) (got %g)", tol);
    if (flags & ~BMSP_KRYLOV_X0_GIVEN) fail(BMSP_ERR_INVALID, "flags: unknown bits (got %d; BMSP_KRYLOV_X0_GIVEN = 1 is the only one)", flags);
    if (no_check(tol) && relres_history) fail(BMSP_ERR_INVALID, "relres_history must be NULL under BMSP_KRYLOV_NO_CHECK: nothing is read back");
}

void krylov_check_operands(const bmsp_matrix_s *A, const bmsp_precond *pc)
{
    if (A->num_rows != A->num_cols) fail(BMSP_ERR_INVALID, "krylov_solve: matrix A must be square (it is %d x %d)", A->num_rows, A->num_cols);
    spmv_op_check_matrix(A, "krylov_solve");
    if (pc && (pc->kind == BMSP_PC_ILU_EXACT || pc->kind == BMSP_PC_ILU_SWEEPS)) {
        const bmsp_matrix_s *F = pc->F;
        if (!F) fail(BMSP_ERR_INVALID, "pc->F is null under an ILU preconditioner");
        if (F->num_rows != A->num_rows || F->num_cols != A->num_cols)
            fail(BMSP_ERR_INVALID, "pc->F must have A's shape (F is %d x %d, A is %d x %d)", F->num_rows, F->num_cols, A->num_rows, A->num_cols);
        spmv_op_check_matrix(F, "krylov_solve (pc->F)");
        const bool ok = A->dtype == BMSP_F64 ? F->dtype == BMSP_F64 : (F->dtype == BMSP_F32 || F->dtype == BMSP_F16);
        if (A->dtype != BMSP_F16 && !ok) fail(BMSP_ERR_INVALID, "pc->F: dtype must be F64 for an F64 A, F32 or F16 for an F32 A");
    }
    if (A->dtype == BMSP_F16) fail(BMSP_ERR_UNSUPPORTED, "krylov_solve: an F16 matrix A is not supported (the Krylov vectors would be fp16)");
}

// (the arguments were checked at the C boundary: krylov_check_args, krylov_check_operands)
void krylov_solve(bmsp_matrix_s *A, int op, int method, const SolvePc &pc, const void *b, void *x, int64_t max_iter, double tol, int flags,
                  double *relres_history, bmsp_krylov_info *info, hipStream_t st)
{
    const int64_t n = A->num_rows;
    if (empty_solve(n, info)) return;
    const SolveCall c{A, op, pc, b, x, cap_of(n, max_iter), tol, flags, relres_history, info, st};
    if (A->dtype == BMSP_F64) run_solve<double>(c, method);
    else run_solve<float>(c, method);
}

}  // namespace bmsp

BMSP_DEFINE_WARM(krylov)
