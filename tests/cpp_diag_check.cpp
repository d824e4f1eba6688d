// cpp_diag_check.cpp -- bmSpMatrix<T>::diagonal / ::scale / ::scale_inplace and bmSparse_diagonal / _from_diagonal / _scale from
// include/bmSpMatrix.h, used as the reference's user would: D^-1 A has a unit diagonal wherever A's is stored, scaling by ones changes no
// bit, A - diag(A) has a zero diagonal.  Built by tests/test_diag_api.py (compile + link, no GPU needed) and run by tests/test_diag.py on
// the data/real fixture.
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
        bmsp::device_vector<float> d;
        bmSparse_diagonal(A, d);
        const std::vector<float> hd = d.to_host();
        const size_t n = (size_t)(A.num_rows < A.num_cols ? A.num_rows : A.num_cols);
        std::printf("CHECK diagonal %s\n", hd.size() == n ? "OK" : "FAIL");
        // rows with a stored non-zero diagonal entry are divided by it, the others by 1
        std::vector<float> piv((size_t)A.num_rows, 1.0f);
        size_t stored = 0;
        for (size_t i = 0; i < n; i++)
            if (hd[i] != 0.0f) { piv[i] = hd[i]; stored++; }
        bmsp::device_vector<float> dp(piv);
        bmSpMatrix<float> J = A.scale(dp.data(), nullptr, BMSP_SCALE_DIV_LEFT);
        const std::vector<float> jd = J.diagonal().to_host();
        bool unit = J.nnz == A.nnz && J.block_num == A.block_num && J.keys.to_host() == A.keys.to_host() && J.bmps.to_host() == A.bmps.to_host();
        for (size_t i = 0; i < n; i++) unit = unit && jd[i] == (hd[i] != 0.0f ? 1.0f : 0.0f);
        std::printf("CHECK scale unit diagonal %s (%zu stored)\n", unit ? "OK" : "FAIL", stored);
        // multiplying by ones changes no bit, in either layout; in place too
        bmsp::device_vector<float> ones_r(std::vector<float>((size_t)A.num_rows, 1.0f)), ones_c(std::vector<float>((size_t)A.num_cols, 1.0f));
        bmSpMatrix<float> S, St, At = A.with_layout(true), B = A.with_layout(false);
        bmSparse_scale(A, ones_r.data(), ones_c.data(), S);
        bmSparse_scale(A, (const float *)nullptr, ones_c.data(), St, BMSP_SCALE_DIV_RIGHT, true);
        B.scale_inplace(ones_r.data(), nullptr, BMSP_SCALE_DIV_LEFT);
        const bool same = S.values.to_host() == A.values.to_host() && S.bmps.to_host() == A.bmps.to_host() &&
                          St.values.to_host() == At.values.to_host() && St.bmps.to_host() == At.bmps.to_host() &&
                          B.values.to_host() == A.values.to_host();
        std::printf("CHECK scale identity %s\n", same ? "OK" : "FAIL");
        // A - diag(A): A's structure plus the diagonal, zeros on it
        bmSpMatrix<float> Dm, R;
        bmSparse_from_diagonal(d, Dm, A.num_rows, A.num_cols);
        bmSparse_add(1.0, A, -1.0, Dm, R);
        const std::vector<float> rd = R.diagonal().to_host();
        bool zero = Dm.nnz == (int)n && R.nnz >= A.nnz;
        for (size_t i = 0; i < n; i++) zero = zero && rd[i] == 0.0f;
        std::printf("CHECK from_diagonal %s\n", zero ? "OK" : "FAIL");
        bmSpMatrix<half> H(path, false);
        bmSpMatrix<half> HS = H.scale(ones_r.data(), ones_c.data());
        bmsp::device_vector<float> hdiag;
        bmSparse_diagonal(H, hdiag);
        bmSpMatrix<half> HD;
        bmSparse_from_diagonal(hdiag, HD, H.num_rows, H.num_cols, true);
        bmSpMatrix<double> G(path, false);
        bmsp::device_vector<double> gd = G.diagonal();
        G.scale_inplace(nullptr, nullptr);
        std::printf("CHECK half %s\n", HS.nnz == H.nnz && HS.block_num == H.block_num && hdiag.size() == n && HD.nnz == (int)n && gd.size() == n ? "OK" : "FAIL");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
