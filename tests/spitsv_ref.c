/* spitsv_ref.c -- the reference of the iterative-triangular-solve tests: at most max_iter block-Jacobi sweeps as a row loop, one fused
 * multiply-add per stored entry of the strict triangle and one division per row, exactly the chain of spsv_ref.c -- but an entry's x comes
 * from the NEW vector iff its column lies in the row's own block of eight rows, and from the previous iterate otherwise.  Built by the
 * tests with `gcc -O2 -ffp-contract=off -shared -fPIC` and called through ctypes.
 *   rowptr / col / val / diag / lower / unit / alpha / b: as in spsv_ref.c (the strict triangle of the effective matrix as CSR, every row's
 *   entries in CHAIN order; rows run ascending for a lower system and descending for an upper one, so the in-block entries a row reads are
 *   already new).
 *   x: the initial iterate on entry, the last iterate on return; tmp: n elements of scratch.
 *   Per sweep k: changed[k] (some x_i differs in bits), delta[k] = max |fl(x_new - x_old)|, xmax[k] = max |x_new|, NaNs skipped, all in the
 *   vector type.  check != 0: stop after sweep k iff !changed || (tol > 0 && delta <= fl(tol * xmax)); check == 0: run max_iter sweeps.
 *   Returns the number of sweeps that ran; *converged = the stop rule held at the last one. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define SPITSV_REF(NAME, R, FMA, FABS)                                                                                                    \
    int64_t NAME(int64_t n, int lower, int unit, const int64_t *rowptr, const int32_t *col, const R *val, const R *diag, R alpha,          \
                 const R *b, R *x, R *tmp, int64_t max_iter, R tol, int check, int32_t *changed, R *delta, R *xmax, int32_t *converged)   \
    {                                                                                                                                     \
        R *old = x, *new = tmp;                                                                                                           \
        int64_t sweeps = 0;                                                                                                               \
        *converged = 0;                                                                                                                   \
        for (int64_t k = 0; k < max_iter; k++) {                                                                                          \
            int32_t ch = 0;                                                                                                               \
            R dl = 0, mx = 0;                                                                                                             \
            for (int64_t q = 0; q < n; q++) {                                                                                             \
                const int64_t i = lower ? q : n - 1 - q;                                                                                  \
                R s = alpha * b[i];                                                                                                       \
                for (int64_t e = rowptr[i]; e < rowptr[i + 1]; e++)                                                                       \
                    s = FMA(-val[e], (col[e] >> 3) == (i >> 3) ? new[col[e]] : old[col[e]], s);                                            \
                new[i] = unit ? s : s / diag[i];                                                                                          \
                if (memcmp(&new[i], &old[i], sizeof(R))) ch = 1;                                                                          \
                const R d = FABS(new[i] - old[i]), m = FABS(new[i]);                                                                      \
                if (d > dl) dl = d; /* (a NaN compares false: skipped) */                                                                  \
                if (m > mx) mx = m;                                                                                                       \
            }                                                                                                                             \
            changed[k] = ch;                                                                                                              \
            delta[k] = dl;                                                                                                                \
            xmax[k] = mx;                                                                                                                 \
            sweeps = k + 1;                                                                                                               \
            R *t = old;                                                                                                                   \
            old = new;                                                                                                                    \
            new = t;                                                                                                                      \
            if (check) {                                                                                                                  \
                const R bound = tol * mx;                                                                                                 \
                if (!ch || (tol > 0 && dl <= bound)) {                                                                                    \
                    *converged = 1;                                                                                                       \
                    break;                                                                                                                \
                }                                                                                                                         \
            }                                                                                                                             \
        }                                                                                                                                 \
        if (old != x) memcpy(x, old, sizeof(R) * (size_t)n);                                                                              \
        return sweeps;                                                                                                                    \
    }

SPITSV_REF(spitsv_ref_f32, float, fmaf, fabsf)
SPITSV_REF(spitsv_ref_f64, double, fma, fabs)
