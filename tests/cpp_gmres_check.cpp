// cpp_gmres_check.cpp -- bmSparse_solve_gmres and bmSpMultigrid::solve_gmres from include/bmSpMatrix.h for float and double, used as the
// reference's user would: on a row-major and a column-major build of one MatrixMarket file, GMRES(8) with the Jacobi preconditioner and
// GMRES(30) without one, under both ops, and GMRES(8) preconditioned by a one-level cycle (two damped Jacobi steps) must report convergence
// and leave a true residual (a row loop over the host COO in double) of at most twice the tolerance.  Built by tests/test_gmres_api.py
// (compile + link, no GPU needed) and run by tests/test_zzzzzzzzzzzz_gmres.py on a fixture it writes.
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
        std::vector<R> hb(n);
        for (size_t i = 0; i < n; i++) hb[i] = (R)(0.5 + (double)((i * 7) % 11) / 8.0) * (i % 3 ? (R)1 : (R)-1);
        bmsp::device_vector<R> b(hb), x(n);
        const auto residual = [&](int op) {
            const std::vector<R> hx = x.to_host();
            std::vector<double> res(hb.begin(), hb.end());
            for (size_t k = 0; k < coo.num_entries; k++) {
                const size_t r = (size_t)(op ? coo.column_indices[k] : coo.row_indices[k]), c = (size_t)(op ? coo.row_indices[k] : coo.column_indices[k]);
                res[r] -= coo.values[k] * (double)hx[c];
            }
            double rr = 0.0, bb = 0.0;
            for (size_t i = 0; i < n; i++) { rr += res[i] * res[i]; bb += (double)hb[i] * (double)hb[i]; }
            return std::sqrt(rr / bb);
        };
        for (int op = 0; op < 2; op++)
            for (int with = 0; with < 2; with++) {
                bmsp_precond pc = {with ? BMSP_PC_JACOBI : BMSP_PC_NONE, nullptr, 0};
                bmsp_krylov_info info;
                std::vector<double> hist(400, -1.0);
                bmSparse_solve_gmres(A, op, &pc, with ? 8 : 0, b.data(), x.data(), 400, tol, 0, hist.data(), &info);
                ok = ok && info.status == BMSP_KRYLOV_CONVERGED && info.iterations >= 1 && info.iterations < 400 && info.relres <= tol;
                ok = ok && residual(op) <= 2.0 * tol && hist[(size_t)info.iterations] == -1.0 && hist[(size_t)info.iterations - 1] > 0.0;
                ok = ok && std::string(info.method) == (with ? "gmres(8)+jacobi" : "gmres(30)+none");
            }
        std::vector<bmSpMatrix<T> *> levels(1, &A), none;
        bmSpMultigrid<T> mg(levels, none);
        bmsp_krylov_info info;
        mg.solve_gmres(8, b.data(), x.data(), 400, tol, 0, nullptr, &info);
        ok = ok && info.status == BMSP_KRYLOV_CONVERGED && std::string(info.method) == "gmres(8)+mg" && residual(0) <= 2.0 * tol;
        ok = ok && info.precond_applies == info.iterations;
    }
    std::printf("CHECK gmres %s %s\n", name, ok ? "OK" : "FAIL");
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
