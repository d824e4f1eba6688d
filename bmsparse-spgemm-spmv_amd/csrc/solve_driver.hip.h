// solve_driver.hip.h -- the host side of an enqueued solve, once (krylov.hip: CG, BiCGStab; gmres.hip: GMRES(m)): the call and its
// preconditioner, the workspace on the handle, the start, the batches between two read-backs, and what goes into bmsp_krylov_info.
// A method supplies its workspace layout, its kernels' argument struct, a state struct with the fields named below, and three
// callables: the launch that forms bb, the residual of a given x0, and "enqueue iteration k".  Nothing here is a kernel: the device
// side the methods share is dot_tree.hip.h.  The state is a template parameter throughout -- KrylovState and GmresState have no common
// prefix, their offsets are immediates in the kernels -- and the driver touches only the fields both have by name: stopped, status,
// bb, thr, rr, iterations, products, applies.
#pragma once
#include "dot_tree.hip.h"
#include <cmath>
#include <vector>

namespace bmsp {
namespace {

// The preconditioner kind of a hooked solve (SolvePc::hook: the V-cycle, FSAI), internal: the public kinds end at BMSP_PC_ILU_SWEEPS and
// the C boundary refuses everything beyond.
constexpr int kPcHook = BMSP_PC_ILU_SWEEPS + 1;

// One call of a solve: what the entry point was given (checked at the C boundary), the cap, and what follows from the preconditioner.
struct SolveCall {
    bmsp_matrix_s *A;
    int op;
    SolvePc pc;
    const void *b;
    void *x;
    int64_t cap;  // cap_of(n, max_iter)
    double tol;
    int flags;
    double *relres_history;
    bmsp_krylov_info *info;
    hipStream_t st;

    bool checked() const { return !no_check(tol); }
    bool x0() const { return (flags & BMSP_KRYLOV_X0_GIVEN) != 0; }
    double tol2() const { return checked() ? tol * tol : -1.0; }  // fl(tol * tol), or negative under NO_CHECK
    int kind() const { return pc.hook ? kPcHook : (pc.pc ? pc.pc->kind : BMSP_PC_NONE); }
    // the factor of the two ILU kinds, null otherwise (never under a hook, whose pc.pc is null)
    bmsp_matrix_s *F() const { return kind() == BMSP_PC_ILU_EXACT || kind() == BMSP_PC_ILU_SWEEPS ? pc.pc->F : nullptr; }
    // whether M^-1 v is a vector of its own written by pc_apply: the ILU kinds and the hook.  (Jacobi is fused into the methods' kernels.)
    bool applied() const { return F() || pc.hook; }
    const char *pc_name() const
    {
        static const char *const names[4] = {"none", "jacobi", "ilu", "ilu_sweeps"};
        return pc.hook ? pc.name : names[kind()];
    }
};

template <typename R>
void product(const SolveCall &c, const R *in, R *out)
{
    spmv_op(c.A, c.op, 1.0, in, 0.0, out, c.st);
}

// out = M^-1 in where c.applied().  The ILU kinds through tmp: L then U; under op T the transposed factors, U^T then L^T.  A hooked
// solve: the hook, which gets the status word every kernel of the solver reads first.
template <typename R>
void pc_apply(const SolveCall &c, const R *in, R *tmp, R *out, const int *stopped)
{
    if (c.pc.hook) return c.pc.hook(c.pc.handle, in, out, stopped, c.st);
    const int first = c.op == BMSP_OP_T ? BMSP_FILL_UPPER : BMSP_FILL_LOWER;
    for (int half = 0; half < 2; half++) {
        const int fill = half == 0 ? first : 1 - first;
        const int diag = fill == BMSP_FILL_LOWER ? BMSP_DIAG_UNIT : BMSP_DIAG_NON_UNIT;
        const R *src = half == 0 ? in : tmp;
        R *dst = half == 0 ? tmp : out;
        if (c.kind() == BMSP_PC_ILU_EXACT) spsv(c.F(), c.op, fill, diag, 1.0, src, dst, c.st);
        else spitsv(c.F(), c.op, fill, diag, 1.0, src, dst, c.pc.pc->sweeps, BMSP_ITSV_NO_CHECK, 0, nullptr, nullptr, c.st);
    }
}

// The workspace of a solve lives on A and grows to the largest need seen there.
char *grow_workspace(bmsp_matrix_s *A, size_t need, hipStream_t st)
{
    if (need > A->krylov_ws_bytes) {
        if (A->krylov_ws) BMSP_HIP(hipStreamSynchronize(st));  // (work enqueued on the old one has finished before it goes back to the pool)
        A->krylov_ws.release();
        A->krylov_ws_bytes = 0;
        A->krylov_ws.alloc(need);
        A->krylov_ws_bytes = need;
    }
    return (char *)A->krylov_ws;
}

// info->method is "<method>+<preconditioner>"; call after grow_workspace
void begin_info(const SolveCall &c, const char *method)
{
    if (!c.info) return;
    memset(c.info, 0, sizeof *c.info);
    snprintf(c.info->method, sizeof c.info->method, "%s+%s", method, c.pc_name());
    c.info->max_iterations = c.cap;
    c.info->workspace_bytes = (int64_t)c.A->krylov_ws_bytes;
}

bool empty_solve(int64_t n, bmsp_krylov_info *info)
{
    if (n != 0) return false;
    if (info) {
        memset(info, 0, sizeof *info);
        snprintf(info->method, sizeof info->method, "none (empty matrix)");
        info->status = BMSP_KRYLOV_CONVERGED;
    }
    return true;
}

template <typename State>
void read_state(const SolveCall &c, const State *S, State &hs)
{
    BMSP_HIP(hipStreamSynchronize(c.st));
    copy_d2h_staged(&hs, S, sizeof hs);
}

// The start: the state and the records zeroed, bb (form_bb: the launch that leaves bb, thr and -- without x0 -- the start's residual
// test in S), under a check the first read-back, then x and the start's residual: r = b into `r` with x = 0, or residual() of the x0
// given (the product and the launch that forms r, rr and the residual test), behind zero_x() where nothing is read back (x = 0 if
// bb == 0).  d: where the diagonal goes under Jacobi.  True if the solve has finished; hs is the state read back.
template <typename R, typename State, typename FormBB, typename ZeroX, typename Residual>
bool solve_start(const SolveCall &c, State *S, KrylovRecord *rec, const R *d, R *r, State &hs, FormBB form_bb, ZeroX zero_x, Residual residual)
{
    const size_t xbytes = sizeof(R) * (size_t)c.A->num_rows;
    BMSP_HIP(hipMemsetAsync(S, 0, sizeof(State), c.st));
    if (c.checked() && c.cap > 0) BMSP_HIP(hipMemsetAsync(rec, 0, sizeof(KrylovRecord) * (size_t)c.cap, c.st));
    form_bb();
    if (c.checked()) {
        read_state(c, S, hs);
        if (hs.stopped) {
            if (hs.bb == 0.0 || !c.x0()) BMSP_HIP(hipMemsetAsync(c.x, 0, xbytes, c.st));
            return true;
        }
    }
    if (c.kind() == BMSP_PC_JACOBI) matrix_diagonal(c.A, (void *)d, c.st);
    if (c.x0()) {
        if (!c.checked()) zero_x();
        residual();
    } else {
        BMSP_HIP(hipMemsetAsync(c.x, 0, xbytes, c.st));
        BMSP_HIP(hipMemcpyAsync(r, c.b, xbytes, hipMemcpyDeviceToDevice, c.st));
    }
    return false;
}

// The iterations: enqueue(k) for k = 1 .. cap, next_batch of them between two read-backs (BMSP_KRYLOV_CHECK, else the ramp; all of them
// under NO_CHECK), until the state read back says stopped.  What was enqueued behind a stop did nothing.  True if the solve stopped.
template <typename State, typename Enqueue>
bool solve_iterations(const SolveCall &c, const State *S, State &hs, Enqueue enqueue)
{
    const int64_t fixed = c.checked() ? sweep_check_from_env("BMSP_KRYLOV_CHECK", 0) : c.cap;  // (0: the ramp)
    for (int64_t done = 0; done < c.cap;) {
        const int64_t batch = next_batch(c.cap, fixed, done);
        for (int64_t k = done + 1; k <= done + batch; k++) enqueue(k);
        done += batch;
        if (c.checked()) {
            read_state(c, S, hs);
            if (hs.stopped) return true;
        }
    }
    return false;
}

// NO_CHECK: nothing was read back; the method says how many products and applications cap iterations are
void no_check_info(const SolveCall &c, int64_t products, int64_t applies)
{
    if (!c.info) return;
    c.info->iterations = c.cap;
    c.info->status = BMSP_KRYLOV_MAXITER;
    c.info->relres = c.info->bnorm = -1.0;
    c.info->products = products + (c.x0() ? 1 : 0);
    c.info->precond_applies = c.kind() == BMSP_PC_NONE ? 0 : applies;
}

// A checked solve: the records become the history, the state read back last becomes info.  The device's verdict stands: a kernel that
// records an iteration writes rr into the state, into the record and takes the stop rule in the same thread, so hs.rr is the last
// record's unless a residual was formed since without one (the start, a GMRES restart), and hs.status says what the stop rule said of it.
template <typename State>
void checked_info(const SolveCall &c, const KrylovRecord *rec, const State &hs)
{
    const int64_t its = hs.iterations;
    if (c.relres_history && its > 0) {
        std::vector<KrylovRecord> recs((size_t)its);
        copy_d2h_staged(recs.data(), rec, sizeof(KrylovRecord) * (size_t)its);
        for (int64_t k = 0; k < its; k++) c.relres_history[k] = std::sqrt(recs[(size_t)k].rr / hs.bb);
    }
    if (!c.info) return;
    c.info->iterations = its;
    c.info->status = hs.stopped ? hs.status : BMSP_KRYLOV_MAXITER;
    c.info->bnorm = std::sqrt(hs.bb);
    c.info->relres = hs.bb == 0.0 ? 0.0 : std::sqrt(hs.rr / hs.bb);
    c.info->products = hs.products;
    c.info->precond_applies = hs.applies;
}

}  // namespace
}  // namespace bmsp
