// cpp_spmm_op_check.cpp -- bmSparse_SpMM_op from include/bmSpMatrix.h for float, half and double, used as the reference's user would:
// Y = alpha op(A) X + beta Y for k = 5 vectors with padded leading dimensions, on a row-major and a column-major build of one
// MatrixMarket file and both ops, against the host COO.  The fixture's values and the operands are small integers, so every sum is exact
// and the comparison is for equality; the padding of Y must come back untouched.  Built by tests/test_spmm_op_api.py (compile + link, no
// GPU needed) and run by tests/test_spmm_op.py on the data/real fixture.
#include "bmSpMatrix.h"
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

static half to_half(int x)
{
    // small integers |x| < 2048 are exact in binary16
    half h;
    uint16_t sign = x < 0 ? 0x8000u : 0u;
    unsigned a = (unsigned)(x < 0 ? -x : x);
    if (a == 0) { h.bits = sign; return h; }
    int e = 0;
    while ((a >> (e + 1)) != 0) e++;
    h.bits = (uint16_t)(sign | ((unsigned)(e + 15) << 10) | ((a << (10 - e)) & 0x3ffu));
    return h;
}
template <class T> static T make(int x) { return (T)x; }
template <> half make<half>(int x) { return to_half(x); }

template <class T> static bool check(const std::string &path, const char *name)
{
    typedef typename bmsp::vector_of<T>::type R;
    const int k = 5;
    const size_t ldx = 7, ldy = 6;
    bool ok = true;
    for (int lay = 0; lay < 2; lay++) {
        bmSpMatrix<T> A(path, lay != 0);
        const bmsp::coo_matrix<double> &coo = A.host_coo();
        const size_t nr = (size_t)A.num_rows, nc = (size_t)A.num_cols;
        for (int op = 0; op < 2; op++) {
            const size_t n_in = op == BMSP_OP_T ? nr : nc, n_out = op == BMSP_OP_T ? nc : nr;
            std::vector<T> hx(n_in * ldx);
            std::vector<double> dx(n_in * ldx), want(n_out * k, 0.0);
            for (size_t i = 0; i < n_in * ldx; i++) { dx[i] = (double)((int)(i % 7) - 3); hx[i] = make<T>((int)(i % 7) - 3); }
            std::vector<R> hy(n_out * ldy);
            for (size_t i = 0; i < n_out * ldy; i++) hy[i] = (R)((int)(i % 5) - 2);
            for (size_t e = 0; e < coo.num_entries; e++) {
                const size_t r = (size_t)coo.row_indices[e], c = (size_t)coo.column_indices[e];
                const size_t o = op == BMSP_OP_T ? c : r, in = op == BMSP_OP_T ? r : c;
                for (int j = 0; j < k; j++) want[o * k + j] += coo.values[e] * dx[in * ldx + j];
            }
            bmsp::device_vector<T> X(hx);
            bmsp::device_vector<R> Y(hy);
            bmSparse_SpMM_op(A, op, 2.0, X.data(), (int64_t)ldx, -3.0, Y.data(), (int64_t)ldy, k);
            const std::vector<R> got = Y.to_host();
            for (size_t i = 0; i < n_out; i++) {
                for (size_t j = 0; j < ldy; j++) {
                    const double w = j < (size_t)k ? 2.0 * want[i * k + j] - 3.0 * (double)hy[i * ldy + j] : (double)hy[i * ldy + j];
                    ok = ok && (double)got[i * ldy + j] == w;
                }
            }
        }
    }
    std::printf("CHECK spmm_op %s %s\n", name, ok ? "OK" : "FAIL");
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s A.mtx\n", argv[0]); return 2; }
    try {
        const std::string path = argv[1];
        const bool f = check<float>(path, "float"), h = check<half>(path, "half"), d = check<double>(path, "double");
        return f && h && d ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
