/* multigrid_ref.c -- the V-cycle of bmsp_mg_vcycle in row mode as include/bmsp.h fixes it, operation by operation, on CSR operands sorted
 * by (row, column).  Built with gcc -O2 -ffp-contract=off: nothing is contracted but the named fma / fmaf.
 *   mg_vcycle_ref_f32   float operands, float arithmetic (fmaf)       -- the bits of an F32 hierarchy
 *   mg_vcycle_ref_f64   double operands, double arithmetic (fma)      -- the bits of an F64 hierarchy
 *   mg_vcycle_ref_wide  float operands, everything in double          -- the same linear operator without the float roundings
 * Operators per level l: A[l] (n[l] x n[l]), P[l] (n[l] x n[l+1]) and R[l] (n[l+1] x n[l]) as (row pointer, columns, values); inv: the
 * dense inverse of A[levels-1], row-major with leading dimension ld_inv, or NULL.  r: n[0] entries; z: n[0] entries of the work type. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define DEFINE_CYCLE(NAME, ST, W, FMA)                                                                                                  \
    typedef struct {                                                                                                                    \
        int levels, pre, post;                                                                                                          \
        const int64_t *n;                                                                                                               \
        const int64_t *const *Ap, *const *Ac, *const *Pp, *const *Pc, *const *Rp, *const *Rc;                                           \
        const ST *const *Av, *const *Pv, *const *Rv;                                                                                    \
        const ST *inv;                                                                                                                  \
        int64_t ld;                                                                                                                     \
        W wR;                                                                                                                           \
    } NAME##_args;                                                                                                                      \
    /* out_i = rowchain(M, init (NULL: +0), sign, v)_i */                                                                               \
    static void NAME##_chain(int64_t rows, const int64_t *ptr, const int64_t *col, const ST *val, const W *init, int neg, const W *v,   \
                             W *out)                                                                                                    \
    {                                                                                                                                   \
        for (int64_t i = 0; i < rows; i++) {                                                                                            \
            W s = init ? init[i] : (W)0;                                                                                                \
            for (int64_t k = ptr[i]; k < ptr[i + 1]; k++) s = FMA(neg ? -(W)val[k] : (W)val[k], v[col[k]], s);                          \
            out[i] = s;                                                                                                                 \
        }                                                                                                                               \
    }                                                                                                                                   \
    /* `steps` Jacobi steps for A[l] x = r; *x: the iterate (NULL: zero), replaced */                                                   \
    static void NAME##_smooth(const NAME##_args *a, int l, int steps, const W *r, const W *d, W **x)                                    \
    {                                                                                                                                   \
        const int64_t n = a->n[l];                                                                                                      \
        for (int k = 0; k < steps; k++) {                                                                                               \
            W *y = (W *)malloc(sizeof(W) * (size_t)(n + 1));                                                                            \
            if (!*x) {                                                                                                                  \
                for (int64_t i = 0; i < n; i++) {                                                                                       \
                    const W q = r[i] / d[i];                                                                                            \
                    y[i] = a->wR * q;                                                                                                   \
                }                                                                                                                       \
            } else {                                                                                                                    \
                NAME##_chain(n, a->Ap[l], a->Ac[l], a->Av[l], r, 1, *x, y);                                                             \
                for (int64_t i = 0; i < n; i++) {                                                                                       \
                    const W q = y[i] / d[i];                                                                                            \
                    const W wq = a->wR * q;                                                                                             \
                    y[i] = (*x)[i] + wq;                                                                                                \
                }                                                                                                                       \
                free(*x);                                                                                                               \
            }                                                                                                                           \
            *x = y;                                                                                                                     \
        }                                                                                                                               \
    }                                                                                                                                   \
    /* returns the cycle of level l for right-hand side r (malloc'ed, n[l] entries) */                                                  \
    static W *NAME##_level(const NAME##_args *a, int l, const W *r)                                                                     \
    {                                                                                                                                   \
        const int64_t n = a->n[l];                                                                                                      \
        const int last = l == a->levels - 1;                                                                                            \
        W *x = NULL;                                                                                                                    \
        if (last && a->inv) {                                                                                                           \
            x = (W *)malloc(sizeof(W) * (size_t)(n + 1));                                                                               \
            for (int64_t i = 0; i < n; i++) {                                                                                           \
                W s = (W)0;                                                                                                             \
                for (int64_t j = 0; j < n; j++) s = FMA((W)a->inv[i * a->ld + j], r[j], s);                                             \
                x[i] = s;                                                                                                               \
            }                                                                                                                           \
            return x;                                                                                                                   \
        }                                                                                                                               \
        W *d = (W *)malloc(sizeof(W) * (size_t)(n + 1));                                                                                \
        for (int64_t i = 0; i < n; i++) {                                                                                               \
            d[i] = (W)0;                                                                                                                \
            for (int64_t k = a->Ap[l][i]; k < a->Ap[l][i + 1]; k++)                                                                     \
                if (a->Ac[l][k] == i) d[i] = (W)a->Av[l][k];                                                                            \
        }                                                                                                                               \
        if (last) {                                                                                                                     \
            NAME##_smooth(a, l, a->pre + a->post, r, d, &x);                                                                            \
            free(d);                                                                                                                    \
            return x;                                                                                                                   \
        }                                                                                                                               \
        NAME##_smooth(a, l, a->pre, r, d, &x);                                                                                          \
        const int64_t nc = a->n[l + 1];                                                                                                 \
        W *t = (W *)malloc(sizeof(W) * (size_t)(n + 1)), *rc = (W *)malloc(sizeof(W) * (size_t)(nc + 1));                               \
        if (!x) {                                                                                                                       \
            x = (W *)calloc((size_t)(n + 1), sizeof(W));                                                                                \
            memcpy(t, r, sizeof(W) * (size_t)n);                                                                                        \
        } else {                                                                                                                        \
            NAME##_chain(n, a->Ap[l], a->Ac[l], a->Av[l], r, 1, x, t);                                                                  \
        }                                                                                                                               \
        NAME##_chain(nc, a->Rp[l], a->Rc[l], a->Rv[l], NULL, 0, t, rc);                                                                 \
        W *e = NAME##_level(a, l + 1, rc);                                                                                              \
        NAME##_chain(n, a->Pp[l], a->Pc[l], a->Pv[l], x, 0, e, x);                                                                      \
        NAME##_smooth(a, l, a->post, r, d, &x);                                                                                         \
        free(e);                                                                                                                        \
        free(rc);                                                                                                                       \
        free(t);                                                                                                                        \
        free(d);                                                                                                                        \
        return x;                                                                                                                       \
    }                                                                                                                                   \
    void NAME(int levels, const int64_t *n, const int64_t *const *Ap, const int64_t *const *Ac, const ST *const *Av,                    \
              const int64_t *const *Pp, const int64_t *const *Pc, const ST *const *Pv, const int64_t *const *Rp,                        \
              const int64_t *const *Rc, const ST *const *Rv, const ST *inv, int64_t ld_inv, double omega, int pre, int post,            \
              const ST *r, W *z)                                                                                                        \
    {                                                                                                                                   \
        NAME##_args a = {levels, pre, post, n, Ap, Ac, Pp, Pc, Rp, Rc, Av, Pv, Rv, inv, ld_inv, (W)omega};                              \
        if (n[0] == 0) return;                                                                                                          \
        W *rw = (W *)malloc(sizeof(W) * (size_t)(n[0] + 1));                                                                            \
        for (int64_t i = 0; i < n[0]; i++) rw[i] = (W)r[i];                                                                             \
        W *x = NAME##_level(&a, 0, rw);                                                                                                 \
        memcpy(z, x, sizeof(W) * (size_t)n[0]);                                                                                         \
        free(x);                                                                                                                        \
        free(rw);                                                                                                                       \
    }

DEFINE_CYCLE(mg_vcycle_ref_f32, float, float, fmaf)
DEFINE_CYCLE(mg_vcycle_ref_f64, double, double, fma)
DEFINE_CYCLE(mg_vcycle_ref_wide, float, double, fma)
