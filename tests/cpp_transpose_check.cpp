// cpp_transpose_check.cpp -- bmSpMatrix<T>::transpose / with_layout from include/bmSpMatrix.h, used as the reference's user would
// once the second parse of the file goes away: `B = A.with_layout(true)` for the right operand of bmSparse_mult.  Built by
// tests/test_transpose_api.py (compile + link, no GPU needed) and run by tests/test_transpose.py on the data/real fixture.
#include "bmSpMatrix.h"
#include <cstdio>
#include <string>
#include <vector>

template <class T> static bool same(const bmSpMatrix<T> &a, const bmSpMatrix<T> &b)
{
    return a.num_rows == b.num_rows && a.num_cols == b.num_cols && a.nnz == b.nnz && a.block_num == b.block_num &&
           a.keys.to_host() == b.keys.to_host() && a.bmps.to_host() == b.bmps.to_host() && a.offsets.to_host() == b.offsets.to_host();
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s A.mtx\n", argv[0]); return 2; }
    try {
        const std::string path = argv[1];
        bmSpMatrix<float> A(path, false), Bt(path, true);
        // the right operand from the left one instead of a second parse
        bmSpMatrix<float> B = A.with_layout(true);
        std::printf("CHECK with_layout %s\n", same(B, Bt) && B.values.to_host() == Bt.values.to_host() ? "OK" : "FAIL");
        // (A^T)^T in the right-operand layout is the same matrix again
        bmSpMatrix<float> At = A.transpose(false);
        bmSpMatrix<float> Att = At.transpose(true);
        const bool dims = At.num_rows == A.num_cols && At.num_cols == A.num_rows && At.nnz == A.nnz;
        std::printf("CHECK transpose %s\n", dims && same(Att, Bt) && Att.values.to_host() == Bt.values.to_host() ? "OK" : "FAIL");
        bmSpMatrix<half> H(path, false);
        bmSpMatrix<half> Ht = H.with_layout(true);
        std::printf("CHECK half %d %d\n", Ht.nnz, Ht.block_num);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
