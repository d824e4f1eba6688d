// cpp_krylov_check.cpp -- bmSparse_solve and bmSparse_vec_dot from include/bmSpMatrix.h for float and double, used as the reference's user
// would: on a row-major and a column-major build of one symmetric positive definite MatrixMarket file, CG with the Jacobi preconditioner
// and BiCGStab without one, under both ops, must report convergence and leave a true residual (a row loop over the host COO in double)
// of at most twice the tolerance; the dot product of two vectors of small integers is exact.  Built by tests/test_krylov_api.py (compile +
// link, no GPU needed) and run by tests/test_zzzzz_krylov.py on a fixture it writes.
#include "bmSpMatrix.h"
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

template <class T> static bool check(const std::string &path, const char *name, double tol)
{
    typedef typename bmsp::vector_of<T>::type R;
    bool ok = true;
    for (int lay = 0; lay < 2; lay++) {
        bmSpMatrix<T> A(path, lay != 0);
        const bmsp::coo_matrix<double> &coo = A.host_coo();
        const size_t n = (size_t)A.num_rows;
        if ((size_t)A.num_cols != n) { std::fprintf(stderr, "the fixture must be square\n"); return false; }
        std::vector<R> hb(n), ones(n, (R)1);
        for (size_t i = 0; i < n; i++) hb[i] = (R)(0.5 + (double)((i * 7) % 11) / 8.0) * (i % 3 ? (R)1 : (R)-1);
        bmsp::device_vector<R> b(hb), x(n), one(ones);
        ok = ok && bmSparse_vec_dot<R>((int64_t)n, one.data(), one.data()) == (double)n;
        for (int op = 0; op < 2; op++)
            for (int method = 0; method < 2; method++) {
                bmsp_precond pc = {method == BMSP_KRYLOV_CG ? BMSP_PC_JACOBI : BMSP_PC_NONE, nullptr, 0};
                bmsp_krylov_info info;
                std::vector<double> hist(n, -1.0);
                bmSparse_solve(A, op, method, &pc, b.data(), x.data(), 0, tol, 0, hist.data(), &info);
                const std::vector<R> hx = x.to_host();
                std::vector<double> res(hb.begin(), hb.end());
                for (size_t k = 0; k < coo.num_entries; k++) {
                    const size_t r = (size_t)(op ? coo.column_indices[k] : coo.row_indices[k]), c = (size_t)(op ? coo.row_indices[k] : coo.column_indices[k]);
                    res[r] -= coo.values[k] * (double)hx[c];
                }
                double rr = 0.0, bb = 0.0;
                for (size_t i = 0; i < n; i++) { rr += res[i] * res[i]; bb += (double)hb[i] * (double)hb[i]; }
                ok = ok && info.status == BMSP_KRYLOV_CONVERGED && info.iterations >= 1 && info.relres <= tol && std::sqrt(rr / bb) <= 2.0 * tol;
                ok = ok && hist[(size_t)info.iterations - 1] == info.relres && hist[(size_t)info.iterations] == -1.0;
            }
    }
    std::printf("CHECK krylov %s %s\n", name, ok ? "OK" : "FAIL");
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s A.mtx\n", argv[0]); return 2; }
    try {
        const std::string path = argv[1];
        const bool f = check<float>(path, "float", 1e-5), d = check<double>(path, "double", 1e-10);
        return f && d ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
