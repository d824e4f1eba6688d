/* fsai_ref.c -- the arithmetic of bmsp_matrix_fsai as include/bmsp.h fixes it, restated on CSR inputs for the tests (built by
 * tests/test_fsai_api.py with gcc -O2 -ffp-contract=off and called through ctypes).  op(A) comes as CSR (the caller hands over the
 * transposed matrix for op T), S as CSR with ascending columns in every row, the diagonal last.  Nothing is contracted except the named
 * fma.  Returns the number of rows of G that hold a non-finite value; -1 if a row of S is longer than 64. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#define FSAI_REF(NAME, R, FMA, SQRT)                                                                                                   \
    int64_t NAME(int64_t n, const int64_t *a_ptr, const int64_t *a_col, const R *a_val, const int64_t *s_ptr, const int64_t *s_col,    \
                 int scale, R *g_val, R *pivot)                                                                                        \
    {                                                                                                                                  \
        static R B[64][64], y[64];                                                                                                     \
        int64_t bad = 0;                                                                                                               \
        int *pos = (int *)malloc(sizeof(int) * (size_t)(n > 0 ? n : 1));                                                               \
        for (int64_t j = 0; j < n; j++) pos[j] = -1;                                                                                   \
        for (int64_t i = 0; i < n; i++) {                                                                                              \
            const int64_t *P = s_col + s_ptr[i];                                                                                       \
            const int m = (int)(s_ptr[i + 1] - s_ptr[i]);                                                                              \
            if (m > 64) { free(pos); return -1; }                                                                                      \
            if (m == 0) continue;                                                                                                      \
            for (int a = 0; a < m; a++) pos[P[a]] = a;                                                                                 \
            for (int a = 0; a < m; a++) {                                                                                              \
                for (int b = 0; b < m; b++) B[a][b] = (R)0;                                                                            \
                for (int64_t k = a_ptr[P[a]]; k < a_ptr[P[a] + 1]; k++)                                                                \
                    if (pos[a_col[k]] >= 0) B[a][pos[a_col[k]]] = a_val[k];                                                            \
            }                                                                                                                          \
            for (int a = 0; a < m; a++) pos[P[a]] = -1;                                                                                \
            for (int k = 0; k + 1 < m; k++)                                                                                            \
                for (int a = k + 1; a < m; a++) {                                                                                      \
                    const R l = B[a][k] / B[k][k];                                                                                     \
                    B[a][k] = l;                                                                                                       \
                    for (int b = k + 1; b < m; b++) B[a][b] = FMA(-l, B[k][b], B[a][b]);                                               \
                }                                                                                                                      \
            y[m - 1] = (R)1 / B[m - 1][m - 1];                                                                                         \
            for (int a = m - 2; a >= 0; a--) {                                                                                         \
                R s = (R)0;                                                                                                            \
                for (int c = a + 1; c < m; c++) s = FMA(-B[c][a], y[c], s);                                                            \
                y[a] = s;                                                                                                              \
            }                                                                                                                          \
            const R ym = y[m - 1];                                                                                                     \
            int row_bad = 0;                                                                                                           \
            for (int a = 0; a < m; a++) {                                                                                              \
                R g = y[a];                                                                                                            \
                if (scale == 1) { const R q = SQRT(ym); g = y[a] / q; }                                                                \
                else if (scale == 2) g = y[a] / ym;                                                                                    \
                g_val[s_ptr[i] + a] = g;                                                                                               \
                if (!isfinite(g)) row_bad = 1;                                                                                         \
            }                                                                                                                          \
            if (pivot) pivot[i] = ym;                                                                                                  \
            bad += row_bad;                                                                                                            \
        }                                                                                                                              \
        free(pos);                                                                                                                     \
        return bad;                                                                                                                    \
    }

FSAI_REF(fsai_ref_f32, float, fmaf, sqrtf)
FSAI_REF(fsai_ref_f64, double, fma, sqrt)
