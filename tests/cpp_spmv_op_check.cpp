// cpp_spmv_op_check.cpp -- bmSparse_SpMV_op from include/bmSpMatrix.h for float, half and double, used as the reference's user would:
// u = A^T v and u = alpha A v + beta u on a row-major and a column-major build of one MatrixMarket file, against the host COO.  The
// fixture's values and the vectors are small integers, so every sum is exact and the comparison is for equality.  Built by
// tests/test_spmv_op_api.py (compile + link, no GPU needed) and run by tests/test_spmv_op.py on the data/real fixture.
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
    bool ok = true;
    for (int lay = 0; lay < 2; lay++) {
        bmSpMatrix<T> A(path, lay != 0);
        const bmsp::coo_matrix<double> &coo = A.host_coo();
        const size_t nr = (size_t)A.num_rows, nc = (size_t)A.num_cols;
        for (int op = 0; op < 2; op++) {
            const size_t n_in = op == BMSP_OP_T ? nr : nc, n_out = op == BMSP_OP_T ? nc : nr;
            std::vector<T> hv(n_in);
            std::vector<double> dv(n_in), want(n_out, 0.0);
            for (size_t i = 0; i < n_in; i++) { dv[i] = (double)((int)(i % 7) - 3); hv[i] = make<T>((int)(i % 7) - 3); }
            std::vector<R> hu(n_out);
            for (size_t i = 0; i < n_out; i++) hu[i] = (R)((int)(i % 5) - 2);
            for (size_t k = 0; k < coo.num_entries; k++) {
                const size_t r = (size_t)coo.row_indices[k], c = (size_t)coo.column_indices[k];
                if (op == BMSP_OP_T) want[c] += coo.values[k] * dv[r];
                else want[r] += coo.values[k] * dv[c];
            }
            bmsp::device_vector<T> v(hv);
            bmsp::device_vector<R> u(hu);
            bmSparse_SpMV_op(A, op, 2.0, v.data(), -3.0, u.data());
            const std::vector<R> got = u.to_host();
            for (size_t i = 0; i < n_out; i++) ok = ok && (double)got[i] == 2.0 * want[i] - 3.0 * (double)hu[i];
        }
    }
    std::printf("CHECK spmv_op %s %s\n", name, ok ? "OK" : "FAIL");
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
