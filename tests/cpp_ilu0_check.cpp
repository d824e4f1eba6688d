// cpp_ilu0_check.cpp -- bmSparse_ILU0 / bmSparse_ILU0_values from include/bmSpMatrix.h for float, half and double, used as the reference's
// user would: on a row-major and a column-major build of one square MatrixMarket file with a full, dominant diagonal, (a) run to the fixed
// point (max_iter = 0, tol = 0) the call converges within 2 n sweeps with a last delta of 0, and for float and double F holds the bits of
// the sequential ILU(0) evaluated on the host COO -- one std::fma per product in ascending k, one division below the diagonal (this file is
// compiled with -ffp-contract=off); (b) restarted from that F with BMSP_ILU_F0_GIVEN one sweep changes nothing; (c) two unchecked sweeps
// into the same F report sweeps = 2, converged = 0, delta = -1.  Built by tests/test_ilu0_api.py (compile + link, no GPU needed) and run
// by tests/test_zz_ilu0.py on a fixture it writes.
#include "bmSpMatrix.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

template <class R> static std::vector<R> sequential(size_t n, const bmsp::coo_matrix<double> &coo)
{
    std::map<std::pair<size_t, size_t>, R> f;  // (row, col) -> value, walked in (row, col) order
    for (size_t k = 0; k < coo.num_entries; k++) f[{(size_t)coo.row_indices[k], (size_t)coo.column_indices[k]}] = (R)coo.values[k];
    for (auto &e : f) {
        const size_t i = e.first.first, j = e.first.second, m = std::min(i, j);
        R s = e.second;
        for (auto it = f.lower_bound({i, 0}); it != f.end() && it->first.first == i && it->first.second < m; ++it) {
            const auto other = f.find({it->first.second, j});
            if (other != f.end()) s = std::fma(-it->second, other->second, s);
        }
        if (i > j) s = s / f.at({j, j});
        e.second = s;
    }
    std::vector<R> out;
    for (auto &e : f) out.push_back(e.second);
    (void)n;
    return out;
}

template <class T> static bool check(const std::string &path, const char *name)
{
    typedef typename bmsp::vector_of<T>::type R;
    bool ok = true;
    for (int lay = 0; lay < 2; lay++)
        for (int out_lay = 0; out_lay < 2; out_lay++) {
            bmSpMatrix<T> A(path, lay != 0), F;
            const size_t n = (size_t)A.num_rows;
            if ((size_t)A.num_cols != n) { std::fprintf(stderr, "the fixture must be square\n"); return false; }
            std::vector<double> hist(2 * n + 1, -1.0);
            bmsp_ilu0_info info;
            bmSparse_ILU0(A, F, 0, 0.0, out_lay != 0, hist.data(), &info);
            ok = ok && info.converged == 1 && info.sweeps >= 1 && info.sweeps <= 2 * (int64_t)n && info.max_sweeps == 2 * (int64_t)n;
            ok = ok && info.delta == 0.0 && hist[(size_t)info.sweeps - 1] == 0.0 && hist[(size_t)info.sweeps] == -1.0;
            ok = ok && F.nnz == A.nnz && F.block_num == A.block_num;
            if (!std::is_same<T, half>::value) {
                const std::vector<R> want = sequential<R>(n, A.host_coo());
                const bmsp::coo_matrix<double> &got = F.host_coo();
                std::map<std::pair<size_t, size_t>, R> g;
                for (size_t k = 0; k < got.num_entries; k++) g[{(size_t)got.row_indices[k], (size_t)got.column_indices[k]}] = (R)got.values[k];
                std::vector<R> have;
                for (auto &e : g) have.push_back(e.second);
                ok = ok && have.size() == want.size() && std::memcmp(have.data(), want.data(), want.size() * sizeof(R)) == 0;
            }
            bmSparse_ILU0_values(A, F, 5, 0.0, BMSP_ILU_F0_GIVEN, nullptr, &info);
            ok = ok && info.sweeps == 1 && info.converged == 1 && info.delta == 0.0;
            bmSparse_ILU0_values(A, F, 2, BMSP_ILU_NO_CHECK, 0, nullptr, &info);
            ok = ok && info.sweeps == 2 && info.converged == 0 && info.delta == -1.0 && info.fmax == -1.0;
        }
    std::printf("CHECK ilu0 %s %s\n", name, ok ? "OK" : "FAIL");
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
