// cpp_spgemm_masked_check.cpp -- bmSparse_mult_masked / bmSparse_mult_masked_values from include/bmSpMatrix.h for float, half (with a half
// and with a float mask) and double, used as the reference's user would: on a square MatrixMarket file of small integers every product
// and sum is exact, so C = 2 * (A * A) on A's own pattern (the triangle-counting call, M == A) is compared for equality with a dense host
// product, out of place in both layouts, into an earlier output and in place on a second copy of the mask.  Built by
// tests/test_spgemm_masked_api.py (compile + link, no GPU needed) and run by tests/test_spgemm_masked.py on a Laplacian fixture.
#include "bmSpMatrix.h"
#include <cstdio>
#include <string>
#include <vector>

template <class T> static bool same(bmSpMatrix<T> &C, const std::vector<double> &want, const bmsp::coo_matrix<double> &coo)
{
    C.generate_coo();  // (a matrix written in place: its host copy is from before the call)
    const bmsp::coo_matrix<double> &got = C.host_coo();
    bool ok = got.num_entries == coo.num_entries;
    for (size_t e = 0; ok && e < coo.num_entries; e++)
        ok = got.row_indices[e] == coo.row_indices[e] && got.column_indices[e] == coo.column_indices[e] && got.values[e] == want[e];
    return ok;
}

template <class TI, class TO> static bool check(const std::string &path, const char *name)
{
    bool ok = true;
    for (int lay = 0; lay < 2; lay++) {
        bmSpMatrix<TI> A(path, lay != 0), B(path, lay == 0);
        bmSpMatrix<TO> M(path, lay != 0), M2(path, lay == 0);
        const bmsp::coo_matrix<double> coo = M.host_coo();
        const size_t n = (size_t)A.num_rows;
        if ((size_t)A.num_cols != n) { std::fprintf(stderr, "the fixture must be square\n"); return false; }
        std::vector<double> dense(n * n, 0.0), want(coo.num_entries);
        for (size_t e = 0; e < coo.num_entries; e++) dense[(size_t)coo.row_indices[e] * n + (size_t)coo.column_indices[e]] = coo.values[e];
        for (size_t e = 0; e < coo.num_entries; e++) {
            double d = 0.0;
            for (size_t k = 0; k < n; k++) d += dense[(size_t)coo.row_indices[e] * n + k] * dense[k * n + (size_t)coo.column_indices[e]];
            want[e] = 2.0 * d;
        }
        bmSpMatrix<TO> C, Ct;
        bmSparse_mult_masked(A, B, M, C, 2.0);
        bmSparse_mult_masked(A, B, M, Ct, 1.0, 0.0, 0, lay == 0);
        bmSparse_mult_masked_values(A, B, M, Ct, 2.0);    // into the other layout's output
        bmSparse_mult_masked_values(A, B, M2, M2, 2.0);   // in place on a mask of its own
        ok = ok && same(C, want, coo) && same(Ct, want, coo) && same(M2, want, coo);
    }
    std::printf("CHECK spgemm_masked %s %s\n", name, ok ? "OK" : "FAIL");
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s A.mtx\n", argv[0]); return 2; }
    try {
        const std::string path = argv[1];
        const bool f = check<float, float>(path, "float"), h = check<half, half>(path, "half"), hf = check<half, float>(path, "half->float"),
                   d = check<double, double>(path, "double");
        return f && h && hf && d ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
