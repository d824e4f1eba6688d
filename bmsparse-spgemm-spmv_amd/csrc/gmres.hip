// gmres.hip -- restarted GMRES on the device (bmsp_gmres_solve, bmsp_mg_solve_gmres): right-preconditioned GMRES(m) for op(A) x = b with
// the whole iteration enqueued on the stream, as krylov.hip's CG and BiCGStab are.  include/bmsp.h fixes the arithmetic operation by
// operation.  Products and preconditioners are the library's own calls; what is new is the orthogonalisation, classical Gram-Schmidt
// applied twice:
//   gmres_dots_kernel    t_i = dot(v_i, w) for up to 16 basis vectors per launch, all of one read of w.  Every t_i has bmsp_vec_dot's tree
//       (dot_tree.hip.h): the same chunks, the same lanes, the same hand-off to the workgroup that arrives last, and beyond
//       kTicketMaxChunks chunks a second-level launch with a workgroup per dot.
//   gmres_update_kernel  w = fl(w - fl(tR_i * v_i)) for i ascending, element by element, in one launch for the whole basis; after the
//       second pass it carries the partial sums of dot(w, w).
//   gmres_scalar_kernel  one workgroup: the second level of dot(w, w), then in thread 0 the column of the Hessenberg matrix, the Givens
//       rotations, the record and the stop rule.
//   gmres_scale_kernel (the normalisation), gmres_y_kernel (the back substitution, one thread) and gmres_xform_kernel (x += Z y).
// The host side is krylov.hip's too (solve_driver.hip.h): run_gmres keeps the workspace layout, GmresArgs, the launches of one iteration
// and the x-formation after a stop inside a cycle.
// Termination is krylov.hip's protocol: every kernel reads `stopped` first and returns without writing once it is set.  The exception
// is the pair that forms x: the scalar kernel leaves in `J` the columns the cycle has completed (0 after a breakdown), gmres_y_kernel
// takes them over and clears J, so the x-formation enqueued behind a stop still applies the cycle the stop fell into, exactly once.
#include "solve_driver.hip.h"

namespace bmsp {
namespace {

constexpr int kDefaultRestart = 30, kMaxRestart = 256;
// Basis vectors per launch of gmres_dots_kernel; BMSP_GMRES_GROUP=1..16 (read per call) sets another.  The bits do not depend on it.
constexpr int kMaxGroup = 16, kDefaultGroup = 8;

// The scalars of one solve, device-resident.  `stopped` is what every kernel reads first; `status` is a BMSP_KRYLOV_* value.
struct GmresState {
    double bb, thr, rr;  // rr: the residual dot last formed or recorded: what info->relres reports
    double scale;        // 1 / beta or 1 / h_{j+1}: what the next normalisation multiplies by
    long long iterations, products, applies;
    int status, stopped;
    uint32_t ticket;
    int J, Jx;           // columns completed by the current cycle and not yet in x; the columns gmres_xform_kernel applies
};

template <typename R>
struct GmresArgs {
    GmresState *S;
    KrylovRecord *rec;  // null under NO_CHECK
    double *P;          // kMaxGroup * chunks partials
    double *U;          // column l of the rotated Hessenberg matrix at U + l * m: entries 0 .. l
    double *cs, *sn;    // the rotations
    double *g, *y;      // m + 1 and m
    double *t;          // the dots of the two passes: t[p * (m + 1) + i]
    const R *b, *d;     // d: the diagonal (Jacobi)
    R *x;
    R *V, *Z;           // basis vector i at V + i * stride, z_i at Z + i * stride (Z == V without a preconditioner)
    int64_t n, stride;
    uint32_t chunks;
    int m, pc, x0;
    double tol2;        // fl(tol * tol), or negative under NO_CHECK
};

// The residual dot at the start of a cycle: the stop rule, then beta, g_0 and the scale of v_0.
template <typename R>
__device__ __forceinline__ void begin_cycle(const GmresArgs<R> &a, double rr)
{
    GmresState *S = a.S;
    S->rr = rr;
    if (!residual_verdict(S, rr)) return;
    const double beta = __builtin_sqrt(rr);
    S->scale = 1.0 / beta;
    a.g[0] = beta;
}

// ---- the start and the restart: bb = dot(b, b), or r = b - (op(A) x) with rr = dot(r, r) ----
enum { kStartBB = 0, kStartR0 = 1 };

template <typename R, int STEP>
__global__ __launch_bounds__(kThreads) void gmres_start_kernel(GmresArgs<R> a)
{
#pragma clang fp contract(off)
    if (STEP == kStartR0 && a.S->stopped) return;
    __shared__ double lds4[4];
    double acc = 0.0;
    const int64_t base = (int64_t)blockIdx.x * kChunk;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int64_t i = base + q * kThreads + (int64_t)threadIdx.x;
        if (i >= a.n) continue;
        if (STEP == kStartBB) {
            acc = dot_term(a.b[i], a.b[i], acc);
        } else {
            const R r = a.b[i] - a.V[a.stride + i];  // (the product landed in slot 1)
            a.V[i] = r;
            acc = dot_term(r, r, acc);
        }
    }
    const double s = group_sum(acc, lds4);
    if (threadIdx.x == 0) a.P[blockIdx.x] = s;
}

template <typename R, int STEP>
__global__ __launch_bounds__(kThreads) void gmres_start_finish_kernel(GmresArgs<R> a)
{
#pragma clang fp contract(off)
    GmresState *S = a.S;
    if (STEP == kStartR0 && S->stopped) return;
    __shared__ double lds4[4];
    const double s = finish_sum(a.P, a.chunks, lds4);
    if (threadIdx.x != 0) return;
    if (STEP == kStartBB) {
        bb_step(S, s, a.tol2, [&]() {
            if (!a.x0) begin_cycle(a, s);  // (r = b)
        });
    } else {
        S->products++;
        begin_cycle(a, s);
    }
}

// x = 0 if the solve stopped on bb == 0 (NO_CHECK with x0 given: nothing is read back)
template <typename R>
__global__ __launch_bounds__(kThreads) void gmres_zero_x_kernel(GmresArgs<R> a)
{
    if (!(a.S->stopped && a.S->bb == 0.0)) return;
    const int64_t i = (int64_t)blockIdx.x * kThreads + (int64_t)threadIdx.x;
    if (i < a.n) a.x[i] = R(0);
}

// v_slot = fl(sR * v_slot): the normalisation of r (slot 0) or of w (slot j + 1), in place
template <typename R>
__global__ __launch_bounds__(kThreads) void gmres_scale_kernel(GmresArgs<R> a, int slot)
{
    if (a.S->stopped) return;
    const R sR = (R)a.S->scale;
    R *v = a.V + (int64_t)slot * a.stride;
    const int64_t i = (int64_t)blockIdx.x * kThreads + (int64_t)threadIdx.x;
    if (i < a.n) v[i] = sR * v[i];
}

// z_j = v_j / d
template <typename R>
__global__ __launch_bounds__(kThreads) void gmres_jacobi_kernel(GmresArgs<R> a, int j)
{
    if (a.S->stopped) return;
    const int64_t i = (int64_t)blockIdx.x * kThreads + (int64_t)threadIdx.x;
    if (i < a.n) a.Z[(int64_t)j * a.stride + i] = a.V[(int64_t)j * a.stride + i] / a.d[i];
}

// ---- the orthogonalisation ----
// group_sum for NV accumulators with one pair of barriers: the same tree per accumulator
template <int NV>
__device__ __forceinline__ void group_sum_many(double (&acc)[NV], double (*lds)[4])
{
#pragma unroll
    for (int g = 0; g < NV; g++) acc[g] = wave_butterfly(acc[g]);
    __syncthreads();  // (a previous use of lds has been read)
    if (lane_id() == 0) {
#pragma unroll
        for (int g = 0; g < NV; g++) lds[g][wave_id()] = acc[g];
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < NV; g++) acc[g] = ((lds[g][0] + lds[g][1]) + lds[g][2]) + lds[g][3];
}

// t[first + g] = dot(v_{first + g}, w) for g < count <= NV, w = slot j + 1; gridDim.x == chunks.  Under TICKET the workgroup that
// arrives last finishes them (publish_and_finish's hand-off); otherwise the partials stay in P for gmres_dots_finish_kernel.
template <typename R, int NV, bool TICKET>
__global__ __launch_bounds__(kThreads) void gmres_dots_kernel(GmresArgs<R> a, int j, int first, int count, double *t)
{
    GmresState *S = a.S;
    if (S->stopped) return;  // (every lane of the grid reads the same word, written by an earlier launch: all leave or none)
    __shared__ double lds[NV][4];
    __shared__ uint32_t last;
    const R *w = a.V + (int64_t)(j + 1) * a.stride;
    const R *v0 = a.V + (int64_t)first * a.stride;
    const int64_t base = (int64_t)blockIdx.x * kChunk + (int64_t)threadIdx.x;
    R wq[4];
#pragma unroll
    for (int q = 0; q < 4; q++) wq[q] = base + q * kThreads < a.n ? w[base + q * kThreads] : R(0);
    double acc[NV];
#pragma unroll
    for (int g = 0; g < NV; g++) {
        acc[g] = 0.0;
        if (g < count) {
            const R *v = v0 + (int64_t)g * a.stride;
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (base + q * kThreads < a.n) acc[g] = dot_term(v[base + q * kThreads], wq[q], acc[g]);
        }
    }
    group_sum_many<NV>(acc, lds);
    const uint32_t chunks = a.chunks;
    if (!TICKET) {
        if (threadIdx.x == 0) {
#pragma unroll
            for (int g = 0; g < NV; g++)
                if (g < count) a.P[(size_t)g * chunks + blockIdx.x] = acc[g];
        }
        return;
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int g = 0; g < NV; g++)
            if (g < count) __hip_atomic_store(&a.P[(size_t)g * chunks + blockIdx.x], acc[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        last = __hip_atomic_fetch_add(&S->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == chunks - 1u;
    }
    __syncthreads();
    if (!last) return;
    // second level: lane t adds P[t], P[t + 256], ... in ascending order, then the same tree (finish_sum, for all of them at once)
#pragma unroll
    for (int g = 0; g < NV; g++) acc[g] = 0.0;
    for (uint32_t c = threadIdx.x; c < chunks; c += kThreads) {
#pragma unroll
        for (int g = 0; g < NV; g++)
            if (g < count) acc[g] = acc[g] + __hip_atomic_load(&a.P[(size_t)g * chunks + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    group_sum_many<NV>(acc, lds);
    if (threadIdx.x == 0) {
        __hip_atomic_store(&S->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int g = 0; g < NV; g++)
            if (g < count) t[first + g] = acc[g];
    }
}

// the second level as a launch of its own: workgroup g finishes t[first + g]
template <typename R>
__global__ __launch_bounds__(kThreads) void gmres_dots_finish_kernel(GmresArgs<R> a, int first, double *t)
{
    if (a.S->stopped) return;
    __shared__ double lds4[4];
    const double s = finish_sum(a.P + (size_t)blockIdx.x * a.chunks, a.chunks, lds4);
    if (threadIdx.x == 0) t[first + (int)blockIdx.x] = s;
}

// w = fl(w - fl(tR_i * v_i)), i = 0 .. j ascending, per element; WW: the partial sums of dot(w, w) of the result go to P
template <typename R, bool WW>
__global__ __launch_bounds__(kThreads) void gmres_update_kernel(GmresArgs<R> a, int j, const double *t)
{
#pragma clang fp contract(off)
    if (a.S->stopped) return;
    __shared__ double lds4[4];
    R *w = a.V + (int64_t)(j + 1) * a.stride;
    const int64_t base = (int64_t)blockIdx.x * kChunk + (int64_t)threadIdx.x;
    R wq[4];
#pragma unroll
    for (int q = 0; q < 4; q++) wq[q] = base + q * kThreads < a.n ? w[base + q * kThreads] : R(0);
    for (int i = 0; i <= j; i++) {
        const R tR = (R)t[i];  // rounded once
        const R *v = a.V + (int64_t)i * a.stride;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (base + q * kThreads < a.n) {
                const R tv = tR * v[base + q * kThreads];
                wq[q] = wq[q] - tv;
            }
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if (base + q * kThreads < a.n) {
            w[base + q * kThreads] = wq[q];
            if (WW) acc = dot_term(wq[q], wq[q], acc);
        }
    }
    if (WW) {
        const double s = group_sum(acc, lds4);
        if (threadIdx.x == 0) a.P[blockIdx.x] = s;
    }
}

// Column j of iteration k: the second level of dot(w, w), then steps 4 - 9 of include/bmsp.h in thread 0.  One workgroup.
template <typename R>
__global__ __launch_bounds__(kThreads) void gmres_scalar_kernel(GmresArgs<R> a, int j, int64_t k)
{
#pragma clang fp contract(off)
    GmresState *S = a.S;
    if (S->stopped) return;
    __shared__ double lds4[4];
    const double ww = finish_sum(a.P, a.chunks, lds4);
    if (threadIdx.x != 0) return;
    double *h = a.U + (size_t)j * (size_t)a.m;
    const double *t1 = a.t, *t2 = a.t + (a.m + 1);
    const double hn = __builtin_sqrt(ww);
    bool ok = __builtin_isfinite(hn);
    for (int i = 0; i <= j; i++) {
        const double hi = t1[i] + t2[i];
        ok = ok && __builtin_isfinite(t1[i]) && __builtin_isfinite(t2[i]) && __builtin_isfinite(hi);
        h[i] = hi;
    }
    if (!ok) {
        S->J = 0;  // (x keeps the iterate of the last completed cycle)
        return stop(S, BMSP_KRYLOV_BREAKDOWN);
    }
    for (int i = 0; i < j; i++) {
        const double c = a.cs[i], s = a.sn[i], p = h[i], q = h[i + 1];
        const double cp = c * p, sq = s * q, cq = c * q, sp = s * p;
        h[i] = cp + sq;
        h[i + 1] = cq - sp;
    }
    const double hh = h[j] * h[j], nn = hn * hn;
    const double d = __builtin_sqrt(hh + nn);
    if (bad_denominator(d)) {
        S->J = 0;
        return stop(S, BMSP_KRYLOV_BREAKDOWN);
    }
    const double c = h[j] / d, s = hn / d;
    h[j] = d;
    a.cs[j] = c;
    a.sn[j] = s;
    const double gj = a.g[j];
    const double gn = -(s * gj);
    a.g[j + 1] = gn;
    a.g[j] = c * gj;
    const double rr = gn * gn;
    S->rr = rr;
    S->iterations = k;
    S->products++;
    if (a.pc != BMSP_PC_NONE) S->applies++;
    S->J = j + 1;
    S->scale = 1.0 / hn;
    if (a.rec) {
        a.rec[k - 1].rr = rr;
        a.rec[k - 1].written = 1;
    }
    residual_verdict(S, rr, [S]() { S->J = 0; });
}

// The back substitution for the J columns the cycle completed, in thread 0; takes J over (Jx) and clears it.  Runs after a stop too.
template <typename R>
__global__ void gmres_y_kernel(GmresArgs<R> a)
{
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    GmresState *S = a.S;
    const int J = S->J;
    S->Jx = J;
    S->J = 0;
    for (int i = J - 1; i >= 0; i--) {
        double s = a.g[i];
        for (int l = i + 1; l < J; l++) {
            const double uy = a.U[(size_t)l * (size_t)a.m + i] * a.y[l];
            s = s - uy;
        }
        a.y[i] = s / a.U[(size_t)i * (size_t)a.m + i];
    }
}

// x = fl(x + fl(yR_i * z_i)), i = 0 .. Jx - 1 ascending, per element.  Runs after a stop too: Jx says whether there is anything to apply.
template <typename R>
__global__ __launch_bounds__(kThreads) void gmres_xform_kernel(GmresArgs<R> a)
{
#pragma clang fp contract(off)
    const int J = a.S->Jx;
    if (J == 0) return;
    const int64_t base = (int64_t)blockIdx.x * kChunk + (int64_t)threadIdx.x;
    R xq[4];
#pragma unroll
    for (int q = 0; q < 4; q++) xq[q] = base + q * kThreads < a.n ? a.x[base + q * kThreads] : R(0);
    for (int i = 0; i < J; i++) {
        const R yR = (R)a.y[i];  // rounded once
        const R *z = a.Z + (int64_t)i * a.stride;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (base + q * kThreads < a.n) {
                const R yz = yR * z[base + q * kThreads];
                xq[q] = xq[q] + yz;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (base + q * kThreads < a.n) a.x[base + q * kThreads] = xq[q];
}

int group_from_env()
{
    if (const char *e = getenv("BMSP_GMRES_GROUP")) {
        const int g = atoi(e);
        if (g >= 1 && g <= kMaxGroup) return g;
    }
    return kDefaultGroup;
}

template <typename R>
void launch_dots(const GmresArgs<R> &a, int j, int first, int count, double *t, bool ticket, hipStream_t st)
{
    const dim3 grid(a.chunks), block(kThreads);
    const auto go = [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        if (ticket) hipLaunchKernelGGL((gmres_dots_kernel<R, NV, true>), grid, block, 0, st, a, j, first, count, t);
        else hipLaunchKernelGGL((gmres_dots_kernel<R, NV, false>), grid, block, 0, st, a, j, first, count, t);
    };
    if (count <= 1) go(std::integral_constant<int, 1>{});
    else if (count <= 2) go(std::integral_constant<int, 2>{});
    else if (count <= 4) go(std::integral_constant<int, 4>{});
    else if (count <= 8) go(std::integral_constant<int, 8>{});
    else go(std::integral_constant<int, 16>{});
    BMSP_CHECK_LAUNCH();
    if (!ticket) {
        hipLaunchKernelGGL(gmres_dots_finish_kernel<R>, dim3((uint32_t)count), block, 0, st, a, first, t);
        BMSP_CHECK_LAUNCH();
    }
}

template <typename R>
void run_gmres(const SolveCall &c, int restart)
{
    bmsp_matrix_s *A = c.A;
    const hipStream_t st = c.st;
    const int64_t n = A->num_rows, max_it = c.cap;
    const int kind = c.kind();
    const bool checked = c.checked();
    const int m = (int)(restart < max_it ? restart : max_it);  // (a basis beyond the cap would never be filled)
    const int group = group_from_env();
    const int64_t chunks = chunks_of(n);
    // workspace: state | partials | Hessenberg columns, rotations, g, y, dots | diagonal | the ILU kinds' intermediate | basis | z | records
    const size_t vbytes = round256(sizeof(R) * (size_t)n);
    const size_t small = sizeof(double) * ((size_t)m * (size_t)m + 4 * (size_t)m + 1 + 2 * ((size_t)m + 1));
    const size_t off_P = round256(sizeof(GmresState)), off_small = off_P + round256(sizeof(double) * kMaxGroup * (size_t)chunks);
    const size_t off_d = off_small + round256(small), off_tmp = off_d + vbytes, off_V = off_tmp + vbytes;
    const size_t off_Z = off_V + vbytes * ((size_t)m + 1), off_rec = off_Z + (kind == BMSP_PC_NONE ? 0 : vbytes * (size_t)m);
    char *ws = grow_workspace(A, off_rec + (checked ? sizeof(KrylovRecord) * (size_t)max_it : 0), st);  // (records: by the cap, not the restart)
    GmresArgs<R> a{};
    a.S = (GmresState *)ws;
    a.rec = checked ? (KrylovRecord *)(ws + off_rec) : nullptr;
    a.P = (double *)(ws + off_P);
    a.U = (double *)(ws + off_small);
    a.cs = a.U + (size_t)m * (size_t)m;
    a.sn = a.cs + m;
    a.g = a.sn + m;
    a.y = a.g + (m + 1);
    a.t = a.y + m;
    a.b = (const R *)c.b;
    a.d = (const R *)(ws + off_d);
    a.x = (R *)c.x;
    a.V = (R *)(ws + off_V);
    a.Z = kind == BMSP_PC_NONE ? a.V : (R *)(ws + off_Z);
    R *tmp = (R *)(ws + off_tmp);
    a.n = n; a.stride = (int64_t)(vbytes / sizeof(R)); a.chunks = (uint32_t)chunks; a.m = m; a.pc = kind; a.x0 = c.x0() ? 1 : 0;
    a.tol2 = c.tol2();
    const bool ticket = finish_by_ticket(chunks);
    char method[24];
    snprintf(method, sizeof method, "gmres(%d)", restart);  // (the restart asked for, not min(restart, cap))
    begin_info(c, method);
    const dim3 cgrid((uint32_t)chunks), egrid((uint32_t)((n + kThreads - 1) / kThreads)), block(kThreads);
    const auto vec = [&](R *base, int i) { return base + (int64_t)i * a.stride; };
    // z_j = M^-1 v_j
    const auto apply = [&](int j) {
        if (kind == BMSP_PC_JACOBI) {
            hipLaunchKernelGGL(gmres_jacobi_kernel<R>, egrid, block, 0, st, a, j);
            BMSP_CHECK_LAUNCH();
        } else if (kind != BMSP_PC_NONE) {
            pc_apply(c, vec(a.V, j), tmp, vec(a.Z, j), &a.S->stopped);
        }
    };
    const auto scale = [&](int slot) {
        hipLaunchKernelGGL(gmres_scale_kernel<R>, egrid, block, 0, st, a, slot);
        BMSP_CHECK_LAUNCH();
    };
    // r = b - op(A) x into slot 0, rr, the stop rule, beta
    const auto residual = [&]() {
        product(c, a.x, vec(a.V, 1));
        hipLaunchKernelGGL((gmres_start_kernel<R, kStartR0>), cgrid, block, 0, st, a);
        BMSP_CHECK_LAUNCH();
        hipLaunchKernelGGL((gmres_start_finish_kernel<R, kStartR0>), dim3(1), block, 0, st, a);
        BMSP_CHECK_LAUNCH();
    };
    // x += Z y for the columns the cycle completed; does nothing where there are none (after a breakdown; a second time)
    const auto form_x = [&]() {
        hipLaunchKernelGGL(gmres_y_kernel<R>, dim3(1), dim3(kWave), 0, st, a);
        BMSP_CHECK_LAUNCH();
        hipLaunchKernelGGL(gmres_xform_kernel<R>, cgrid, block, 0, st, a);
        BMSP_CHECK_LAUNCH();
    };
    GmresState hs{};
    bool finished = solve_start(
        c, a.S, a.rec, a.d, a.V, hs,
        [&]() {
            hipLaunchKernelGGL((gmres_start_kernel<R, kStartBB>), cgrid, block, 0, st, a);
            BMSP_CHECK_LAUNCH();
            hipLaunchKernelGGL((gmres_start_finish_kernel<R, kStartBB>), dim3(1), block, 0, st, a);
            BMSP_CHECK_LAUNCH();
        },
        [&]() {
            hipLaunchKernelGGL(gmres_zero_x_kernel<R>, egrid, block, 0, st, a);
            BMSP_CHECK_LAUNCH();
        },
        residual);
    if (!finished) {
        finished = solve_iterations(c, a.S, hs, [&](int64_t k) {
            const int j = (int)((k - 1) % m);
            if (j == 0) scale(0);  // v_0 = fl(sR * r)
            apply(j);
            product(c, vec(a.Z, j), vec(a.V, j + 1));
            for (int pass = 0; pass < 2; pass++) {
                double *t = a.t + pass * (m + 1);
                for (int first = 0; first <= j; first += group)
                    launch_dots(a, j, first, j + 1 - first < group ? j + 1 - first : group, t, ticket, st);
                if (pass == 0) hipLaunchKernelGGL((gmres_update_kernel<R, false>), cgrid, block, 0, st, a, j, (const double *)t);
                else hipLaunchKernelGGL((gmres_update_kernel<R, true>), cgrid, block, 0, st, a, j, (const double *)t);
                BMSP_CHECK_LAUNCH();
            }
            hipLaunchKernelGGL(gmres_scalar_kernel<R>, dim3(1), block, 0, st, a, j, k);
            BMSP_CHECK_LAUNCH();
            if (j == m - 1 || k == max_it) {
                form_x();
                if (k < max_it) residual();
            } else {
                scale(j + 1);  // v_{j+1} = fl(sR * w)
            }
        });
    }
    if (!checked) return no_check_info(c, max_it + (max_it > 0 ? (max_it - 1) / m : 0), max_it);
    if (finished && hs.J > 0) {  // the stop fell into a cycle whose end is not enqueued: its columns still go into x
        form_x();
        BMSP_HIP(hipStreamSynchronize(st));
    }
    checked_info(c, a.rec, hs);
}

}  // namespace

void gmres_check_args(int op, int restart, const bmsp_precond *pc, int64_t max_iter, double tol, int flags, const double *relres_history)
{
    spmv_op_check_op(op);
    if (restart < 0 || restart > kMaxRestart) fail(BMSP_ERR_INVALID, "restart must be 0 (30) or 1 .. 256 (got %d)", restart);
    krylov_check_args(op, BMSP_KRYLOV_CG, pc, max_iter, tol, flags, relres_history);
}

// (the arguments were checked at the C boundary: gmres_check_args, krylov_check_operands)
void gmres_solve(bmsp_matrix_s *A, int op, const SolvePc &pc, int restart, const void *b, void *x, int64_t max_iter, double tol, int flags,
                 double *relres_history, bmsp_krylov_info *info, hipStream_t st)
{
    const int64_t n = A->num_rows;
    if (empty_solve(n, info)) return;
    const SolveCall c{A, op, pc, b, x, cap_of(n, max_iter), tol, flags, relres_history, info, st};
    if (A->dtype == BMSP_F64) run_gmres<double>(c, restart ? restart : kDefaultRestart);
    else run_gmres<float>(c, restart ? restart : kDefaultRestart);
}

}  // namespace bmsp

BMSP_DEFINE_WARM(gmres)
