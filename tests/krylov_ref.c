/* krylov_ref.c -- the reference of the vector primitives behind the Krylov solvers (bmsp_vec_dot, bmsp_vec_axpby), restated from the
 * text of include/bmsp.h: the dot product's fixed two-level tree written with fma(), and the scaled sum with every operation rounded on
 * its own.  Compiled by the tests with `gcc -O2 -ffp-contract=off -shared -fPIC` and called through ctypes.  Plain C, no GPU. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

/* 256 accumulators -> one value: in each wave of 64 lanes the xor butterfly d = 32 .. 1 (every lane adds its partner's value, so all 64
 * end alike), then the four wave sums in ascending order */
static double tree256(double *acc)
{
    double tmp[64];
    double w[4];
    for (int wave = 0; wave < 4; wave++) {
        double *a = acc + 64 * wave;
        for (int d = 32; d >= 1; d >>= 1) {
            for (int t = 0; t < 64; t++) tmp[t] = a[t] + a[t ^ d];
            for (int t = 0; t < 64; t++) a[t] = tmp[t];
        }
        w[wave] = a[0];
    }
    return ((w[0] + w[1]) + w[2]) + w[3];
}

#define KRYLOV_REF(SUFFIX, R)                                                                                          \
    double vec_dot_ref_##SUFFIX(int64_t n, const R *x, const R *y)                                                     \
    {                                                                                                                  \
        const int64_t chunks = (n + 1023) / 1024;                                                                      \
        double *P = (double *)malloc(sizeof(double) * (size_t)(chunks ? chunks : 1));                                  \
        double acc[256];                                                                                               \
        for (int64_t c = 0; c < chunks; c++) {                                                                         \
            for (int t = 0; t < 256; t++) {                                                                            \
                acc[t] = 0.0;                                                                                          \
                for (int q = 0; q < 4; q++) {                                                                          \
                    const int64_t i = 1024 * c + 256 * q + t;                                                          \
                    if (i < n) acc[t] = fma((double)x[i], (double)y[i], acc[t]);                                       \
                }                                                                                                      \
            }                                                                                                          \
            P[c] = tree256(acc);                                                                                       \
        }                                                                                                              \
        double result = 0.0;                                                                                           \
        if (chunks > 0) {                                                                                              \
            for (int t = 0; t < 256; t++) {                                                                            \
                acc[t] = 0.0;                                                                                          \
                for (int64_t c = t; c < chunks; c += 256) acc[t] = acc[t] + P[c];                                      \
            }                                                                                                          \
            result = tree256(acc);                                                                                     \
        }                                                                                                              \
        free(P);                                                                                                       \
        return result;                                                                                                 \
    }                                                                                                                  \
    /* y = fl(fl(a * x) + fl(b * y)); with b == 0 y is not read */                                                     \
    void vec_axpby_ref_##SUFFIX(int64_t n, R a, const R *x, R b, R *y)                                                 \
    {                                                                                                                  \
        for (int64_t i = 0; i < n; i++) {                                                                              \
            const R ax = a * x[i];                                                                                     \
            if (b == (R)0) {                                                                                           \
                y[i] = ax;                                                                                             \
            } else {                                                                                                   \
                const R by = b * y[i];                                                                                 \
                y[i] = ax + by;                                                                                        \
            }                                                                                                          \
        }                                                                                                              \
    }

KRYLOV_REF(f32, float)
KRYLOV_REF(f64, double)
