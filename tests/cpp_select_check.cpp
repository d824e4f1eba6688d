// cpp_select_check.cpp -- bmSpMatrix<T>::tril / ::triu / ::band / ::mask and bmSparse_select_band / _mask from include/bmSpMatrix.h, used
// as the reference's user would: the two triangles of A split its entries, the band and its complement do, A masked by itself is A and by
// its complement nothing.  Built by tests/test_select_api.py (compile + link, no GPU needed) and run by the GPU test of selection on the
// data/real fixture.
#include "bmSpMatrix.h"
#include <cstdio>
#include <string>

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s A.mtx\n", argv[0]); return 2; }
    try {
        const std::string path = argv[1];
        bmSpMatrix<float> A(path, false);
        bmSpMatrix<float> L = A.tril(-1), U = A.triu(0), S;
        bmSparse_add(1.0, L, 1.0, U, S);
        const bool split = L.nnz + U.nnz == A.nnz && S.keys.to_host() == A.keys.to_host() && S.bmps.to_host() == A.bmps.to_host() &&
                           S.values.to_host() == A.values.to_host();
        std::printf("CHECK select triangles %s\n", split ? "OK" : "FAIL");
        bmSpMatrix<float> B, Bc;
        bmsp_select_stats sb, sc;
        bmSparse_select_band(A, B, -3, 5, false, false, &sb);
        bmSparse_select_band(A, Bc, -3, 5, true, true, &sc);
        const bool band = sb.nnz_in == A.nnz && sb.nnz_out == B.nnz && sb.nnz_out + sc.nnz_out == A.nnz && sb.blocks_out == B.block_num &&
                          A.band(BMSP_BAND_MIN, BMSP_BAND_MAX).values.to_host() == A.values.to_host() && A.band(5, 4).block_num == 0;
        std::printf("CHECK select band %s\n", band ? "OK" : "FAIL");
        bmSpMatrix<half> H(path, true);
        bmSpMatrix<float> M = A.mask(H), Mc = A.mask(H, true), ML;
        bmSparse_select_mask(A, L, ML, false, false, &sb);
        const bool mask = M.bmps.to_host() == A.bmps.to_host() && M.values.to_host() == A.values.to_host() && Mc.block_num == 0 &&
                          Mc.nnz == 0 && ML.bmps.to_host() == L.bmps.to_host() && ML.values.to_host() == L.values.to_host() && sb.nnz_out == L.nnz;
        std::printf("CHECK select mask %s\n", mask ? "OK" : "FAIL");
        bmSpMatrix<half> HL = H.tril(), HU = H.triu(1), HM = H.mask(A), HB;
        bmSparse_select_band(H, HB, 0, 0);
        std::printf("CHECK half %s\n", HL.nnz + HU.nnz == H.nnz && HM.nnz == H.nnz && HB.nnz <= HL.nnz ? "OK" : "FAIL");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
