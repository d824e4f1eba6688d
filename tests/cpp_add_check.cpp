// cpp_add_check.cpp -- bmSparse_add / bmSparse_add_values from include/bmSpMatrix.h, used as the reference's user would: A + A^T of a
// MatrixMarket file, then the sum again with other coefficients.  Built by tests/test_add_api.py (compile + link, no GPU needed) and run
// by tests/test_add.py on the data/real fixture.
#include "bmSpMatrix.h"
#include <cstdio>
#include <string>
#include <vector>

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s A.mtx\n", argv[0]); return 2; }
    try {
        const std::string path = argv[1];
        bmSpMatrix<float> A(path, false);
        bmSpMatrix<float> At = A.transpose(true);
        bmSpMatrix<float> S, S2;
        bmSparse_add(1.0, A, 1.0, At, S);
        // A + A^T is symmetric: its transpose in the same layout has the same arrays
        bmSpMatrix<float> St = S.transpose(false);
        const bool sym = St.keys.to_host() == S.keys.to_host() && St.bmps.to_host() == S.bmps.to_host() &&
                         St.values.to_host() == S.values.to_host() && S.nnz >= A.nnz;
        std::printf("CHECK add %s\n", sym ? "OK" : "FAIL");
        // the same sum with other coefficients: add_values on a sum made with 1, 1 against a fresh add (S3.values views C's array)
        bmSparse_add(2.0, A, -0.5, At, S2, true);
        bmSpMatrix<float> S3;
        bmSparse_add(1.0, A, 1.0, At, S3, true);
        bmSparse_add_values(2.0, A, -0.5, At, S3);
        std::printf("CHECK add_values %s\n", S3.values.to_host() == S2.values.to_host() ? "OK" : "FAIL");
        bmSpMatrix<half> H(path, false);
        bmSpMatrix<half> Ht = H.transpose(true), HS;
        bmSparse_add(1.0, H, 1.0, Ht, HS);
        std::printf("CHECK half %s\n", HS.nnz == S.nnz && HS.block_num == S.block_num ? "OK" : "FAIL");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
