// cpp_spsm_check.cpp -- bmSparse_SpSM / bmSparse_SpSM_launch_info from include/bmSpMatrix.h for float, half and double, used as the
// reference's user would: on a row-major and a column-major build of one square MatrixMarket file with a full diagonal, both triangles,
// both ops and both kinds of diagonal are solved for k = 5 right-hand sides at leading dimensions 7 and 6, and every column is compared
// for equality with bmSparse_SpSV on that column -- the contract of the call.  Built by tests/test_spsm_api.py (compile + link, no GPU
// needed) and run by tests/test_spsm.py on a fixture it writes.
#include "bmSpMatrix.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

template <class T> static bool check(const std::string &path, const char *name)
{
    typedef typename bmsp::vector_of<T>::type R;
    const int k = 5;
    const int64_t ldb = 7, ldx = 6;
    bool ok = true;
    for (int lay = 0; lay < 2; lay++) {
        bmSpMatrix<T> A(path, lay != 0);
        const size_t n = (size_t)A.num_rows;
        if ((size_t)A.num_cols != n) { std::fprintf(stderr, "the fixture must be square\n"); return false; }
        std::vector<R> hB(n * (size_t)ldb, (R)0);
        for (size_t i = 0; i < n; i++)
            for (int c = 0; c < k; c++) hB[i * (size_t)ldb + c] = (R)(0.5 + (double)((i * 7 + (size_t)c * 3) % 11) / 8.0) * ((i + c) % 3 ? (R)1 : (R)-1);
        for (int op = 0; op < 2; op++)
            for (int fill = 0; fill < 2; fill++)
                for (int diag = 0; diag < 2; diag++) {
                    bmsp_spsm_info info;
                    bmSparse_SpSM_launch_info(A, op, fill, diag, k, ldb, ldx, &info);
                    ok = ok && info.lanes == 8 && info.col_chunks == 1 && info.levels >= 1 && info.launches >= 1 &&
                         std::strncmp(info.kernel, "spsm_level_kernel<", 18) == 0;
                    bmsp::device_vector<R> B(hB), X(n * (size_t)ldx);
                    bmSparse_SpSM(A, B.data(), ldb, X.data(), ldx, k, op, fill, diag, -1.5);
                    const std::vector<R> hX = X.to_host();
                    for (int c = 0; c < k; c++) {
                        std::vector<R> hb(n), col(n);
                        for (size_t i = 0; i < n; i++) { hb[i] = hB[i * (size_t)ldb + c]; col[i] = hX[i * (size_t)ldx + c]; }
                        bmsp::device_vector<R> b(hb), x(n);
                        bmSparse_SpSV(A, op, fill, diag, -1.5, b.data(), x.data());
                        const std::vector<R> want = x.to_host();
                        ok = ok && std::memcmp(want.data(), col.data(), n * sizeof(R)) == 0;
                    }
                    bmSparse_SpSM(A, B.data(), ldb, B.data(), ldb, k, op, fill, diag, -1.5);  // in place
                    const std::vector<R> hI = B.to_host();
                    for (size_t i = 0; i < n; i++)
                        for (int c = 0; c < k; c++) ok = ok && std::memcmp(&hI[i * (size_t)ldb + c], &hX[i * (size_t)ldx + c], sizeof(R)) == 0;
                }
    }
    std::printf("CHECK spsm %s %s\n", name, ok ? "OK" : "FAIL");
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
