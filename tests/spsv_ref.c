/* spsv_ref.c -- the reference of the triangular-solve tests: a sequential substitution, one row after another, with one fused
 * multiply-add per stored entry of the strict triangle and one division per row.  Built by the tests with
 * `gcc -O2 -ffp-contract=off -shared -fPIC` and called through ctypes.
 *   rowptr / col / val: the strict triangle of the effective matrix as CSR, every row's entries in CHAIN order (ascending column for a
 *   lower system, descending for an upper one); diag: the stored diagonal (not read when unit != 0); rows are solved ascending for a
 *   lower system and descending for an upper one.  x may be b. */
#include <math.h>
#include <stdint.h>

void spsv_ref_f32(int64_t n, int lower, int unit, const int64_t *rowptr, const int32_t *col, const float *val, const float *diag, float alpha,
                  const float *b, float *x)
{
    for (int64_t k = 0; k < n; k++) {
        const int64_t i = lower ? k : n - 1 - k;
        float s = alpha * b[i];
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; e++) s = fmaf(-val[e], x[col[e]], s);
        x[i] = unit ? s : s / diag[i];
    }
}

void spsv_ref_f64(int64_t n, int lower, int unit, const int64_t *rowptr, const int32_t *col, const double *val, const double *diag, double alpha,
                  const double *b, double *x)
{
    for (int64_t k = 0; k < n; k++) {
        const int64_t i = lower ? k : n - 1 - k;
        double s = alpha * b[i];
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; e++) s = fma(-val[e], x[col[e]], s);
        x[i] = unit ? s : s / diag[i];
    }
}
