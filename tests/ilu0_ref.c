/* ilu0_ref.c -- the reference of the ILU(0) tests: the fixed-point sweep of bmsp_matrix_ilu0 and the sequential factorisation it ends in,
 * over the pattern as CSR (entries of a row in ascending column order) and CSC (entries of a column in ascending row order).  Built by the
 * tests with `gcc -O2 -ffp-contract=off -shared -fPIC` and called through ctypes.
 *   rowptr / col: the CSR pattern, n + 1 and nnz entries; values are indexed by CSR position e.
 *   colptr / rowidx / csc2csr: the CSC pattern and, per CSC position, the CSR position of the same entry.
 *   dpos[j]: the CSR position of (j, j).
 *   a: A's values.  half != 0: the storage type is fp16 -- every result is rounded to fp16 (round to nearest even, overflow to Inf) by
 *   the routine below and kept widened; the arithmetic type R is then float.
 *   One entry:  s = a_ij;  s = fma(-f_ik, f_kj, s) for k ascending over k < min(i, j) with (i, k) and (k, j) stored;  s = s / f_jj if
 *   i > j;  one rounding to the storage type.
 *   ilu0_ref_*: at most max_iter sweeps, every read from the previous iterate.  f: the initial iterate on entry, the last one on return;
 *   tmp: nnz elements of scratch.  Per sweep k: changed[k] (some entry differs in bits), delta[k] = max |fl(f_new - f_old)|, fmax[k] =
 *   max |f_new|, NaNs skipped, nonfinite[k] = entries that are Inf or NaN.  check != 0: stop after sweep k iff !changed || (tol > 0 &&
 *   delta <= fl(tol * fmax)); check == 0: run max_iter sweeps.  Returns the sweeps that ran; *converged = the rule held at the last one.
 *   ilu0_seq_*: the sequential ILU(0): the same chain row by row, columns ascending, in place, f = a on entry. */
#include <math.h>
#include <stdint.h>
#include <string.h>

/* float -> IEEE binary16 bits, round to nearest even in one step */
uint16_t ilu0_ref_f32_to_f16(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t e = (u >> 23) & 0xffu, man = u & 0x7fffffu;
    if (e == 0xffu) return (uint16_t)(sign | 0x7c00u | (man ? (0x200u | (man >> 13)) : 0u));
    if (e == 0) return sign; /* (an fp32 subnormal lies far below half of the smallest fp16 one) */
    const int E = (int)e - 127;
    if (E > 15) return (uint16_t)(sign | 0x7c00u);
    const uint32_t full = man | 0x800000u;
    int shift = 13;
    uint32_t hexp = 0;
    if (E >= -14) hexp = (uint32_t)(E + 15);
    else {
        shift = 13 + (-14 - E);
        if (shift > 25) return sign;
    }
    uint32_t kept = full >> shift;
    const uint32_t rem = full & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
    if (rem > halfway || (rem == halfway && (kept & 1u))) kept++;
    uint32_t bits = hexp ? ((hexp - 1u) << 10) + kept : kept;
    if (bits >= 0x7c00u) bits = 0x7c00u;
    return (uint16_t)(sign | bits);
}

/* IEEE binary16 bits -> float, exactly */
float ilu0_ref_f16_to_f32(uint16_t h)
{
    const uint32_t e = (h >> 10) & 31u, m = h & 0x3ffu;
    float v;
    if (e == 31u) v = m ? NAN : INFINITY;
    else if (e == 0) v = ldexpf((float)m, -24);
    else v = ldexpf((float)(m | 0x400u), (int)e - 25);
    return (h & 0x8000u) ? -v : v;
}

static float store_f32(float s, int half) { return half ? ilu0_ref_f16_to_f32(ilu0_ref_f32_to_f16(s)) : s; }
static double store_f64(double s, int half) { (void)half; return s; }

#define ILU0_ENTRY(R, FMA, STORE)                                                                                                         \
    static R entry_##R(int64_t i, int64_t e, const int64_t *rowptr, const int32_t *col, const int64_t *colptr, const int32_t *rowidx,     \
                       const int64_t *csc2csr, const int64_t *dpos, const R *a, const R *f, int half)                                     \
    {                                                                                                                                     \
        const int64_t j = col[e], m = i < j ? i : j;                                                                                      \
        R s = a[e];                                                                                                                       \
        int64_t p = rowptr[i], q = colptr[j];                                                                                             \
        while (p < rowptr[i + 1] && q < colptr[j + 1] && col[p] < m && rowidx[q] < m) {                                                   \
            if (col[p] < rowidx[q]) p++;                                                                                                  \
            else if (rowidx[q] < col[p]) q++;                                                                                             \
            else {                                                                                                                        \
                s = FMA(-f[p], f[csc2csr[q]], s);                                                                                         \
                p++;                                                                                                                      \
                q++;                                                                                                                      \
            }                                                                                                                             \
        }                                                                                                                                 \
        if (i > j) s = s / f[dpos[j]];                                                                                                    \
        return STORE(s, half);                                                                                                            \
    }

ILU0_ENTRY(float, fmaf, store_f32)
ILU0_ENTRY(double, fma, store_f64)

#define ILU0_REF(NAME, SEQ, R, FABS, ISFINITE)                                                                                            \
    int64_t NAME(int64_t n, const int64_t *rowptr, const int32_t *col, const int64_t *colptr, const int32_t *rowidx,                      \
                 const int64_t *csc2csr, const int64_t *dpos, const R *a, R *f, R *tmp, int64_t max_iter, R tol, int check, int half,      \
                 int32_t *changed, R *delta, R *fmax, int32_t *nonfinite, int32_t *converged)                                             \
    {                                                                                                                                     \
        const int64_t nnz = rowptr[n];                                                                                                    \
        R *old = f, *new = tmp;                                                                                                           \
        int64_t sweeps = 0;                                                                                                               \
        *converged = 0;                                                                                                                   \
        for (int64_t k = 0; k < max_iter; k++) {                                                                                          \
            int32_t ch = 0, nf = 0;                                                                                                       \
            R dl = 0, mx = 0;                                                                                                             \
            for (int64_t i = 0; i < n; i++)                                                                                               \
                for (int64_t e = rowptr[i]; e < rowptr[i + 1]; e++) {                                                                     \
                    new[e] = entry_##R(i, e, rowptr, col, colptr, rowidx, csc2csr, dpos, a, old, half);                                   \
                    if (memcmp(&new[e], &old[e], sizeof(R))) ch = 1;                                                                      \
                    const R d = FABS(new[e] - old[e]), m = FABS(new[e]);                                                                  \
                    if (d > dl) dl = d; /* (a NaN compares false: skipped) */                                                              \
                    if (m > mx) mx = m;                                                                                                   \
                    if (!ISFINITE(new[e])) nf++;                                                                                          \
                }                                                                                                                         \
            changed[k] = ch;                                                                                                              \
            delta[k] = dl;                                                                                                                \
            fmax[k] = mx;                                                                                                                 \
            nonfinite[k] = nf;                                                                                                            \
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
        if (old != f) memcpy(f, old, sizeof(R) * (size_t)nnz);                                                                            \
        return sweeps;                                                                                                                    \
    }                                                                                                                                     \
    void SEQ(int64_t n, const int64_t *rowptr, const int32_t *col, const int64_t *colptr, const int32_t *rowidx, const int64_t *csc2csr,  \
             const int64_t *dpos, const R *a, R *f, int half)                                                                             \
    {                                                                                                                                     \
        memcpy(f, a, sizeof(R) * (size_t)rowptr[n]);                                                                                      \
        for (int64_t i = 0; i < n; i++)                                                                                                   \
            for (int64_t e = rowptr[i]; e < rowptr[i + 1]; e++)                                                                           \
                f[e] = entry_##R(i, e, rowptr, col, colptr, rowidx, csc2csr, dpos, a, f, half);                                           \
    }

ILU0_REF(ilu0_ref_f32, ilu0_seq_f32, float, fabsf, isfinite)
ILU0_REF(ilu0_ref_f64, ilu0_seq_f64, double, fabs, isfinite)
