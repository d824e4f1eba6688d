// cpp_prune_check.cpp -- bmSpMatrix<T>::prune / bmSparse_prune from include/bmSpMatrix.h, used as the reference's user would: the stored
// zeros of A - A go at tol = 0, pruning at a tolerance shrinks A and keeps its diagonal when asked.  Built by tests/test_prune_api.py
// (compile + link, no GPU needed) and run by tests/test_prune.py on the data/real fixture.
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
        bmSpMatrix<float> D, Z;
        bmSparse_add(1.0, A, -1.0, A, D);
        bmsp_prune_stats st;
        bmSparse_prune(D, Z, 0.0, BMSP_PRUNE_ABS, false, false, &st);
        const bool zeros = D.nnz == A.nnz && Z.nnz == 0 && Z.block_num == 0 && st.nnz_in == A.nnz && st.nnz_out == 0 && st.blocks_out == 0;
        std::printf("CHECK prune zeros %s\n", zeros ? "OK" : "FAIL");
        // nothing stored in A is zero: prune(A, 0) is A, in either layout
        bmSpMatrix<float> P = A.prune(0.0);
        bmSpMatrix<float> Pt = A.prune(0.0, BMSP_PRUNE_ABS, false, true), At = A.with_layout(true);
        const bool same = P.keys.to_host() == A.keys.to_host() && P.bmps.to_host() == A.bmps.to_host() &&
                          P.values.to_host() == A.values.to_host() && Pt.bmps.to_host() == At.bmps.to_host() &&
                          Pt.values.to_host() == At.values.to_host();
        std::printf("CHECK prune identity %s\n", same ? "OK" : "FAIL");
        bmSpMatrix<float> R = A.prune(0.5, BMSP_PRUNE_ROW_REL, true);
        std::printf("CHECK prune row_rel %s\n", R.nnz > 0 && R.nnz <= A.nnz ? "OK" : "FAIL");
        bmSpMatrix<half> H(path, false);
        bmSpMatrix<half> HP = H.prune(0.0), HR;
        bmSparse_prune(H, HR, 0.5, BMSP_PRUNE_ROW_REL, true);
        std::printf("CHECK half %s\n", HP.nnz == H.nnz && HP.block_num == H.block_num && HR.nnz == R.nnz ? "OK" : "FAIL");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
