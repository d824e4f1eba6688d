// cpp_multigrid_check.cpp -- bmSpMultigrid<T> from include/bmSpMatrix.h for float and double, used as the reference's user would: a
// two-level hierarchy read from three MatrixMarket files (A0 symmetric positive definite, P, A1 = P^T A0 P), R = P^T by default, the
// inverse of A1 formed here by Gauss-Jordan elimination in double.  For both layouts of A0: one cycle must reduce the residual
// (||r - A0 z|| < ||r||, a row loop over the host COO in double), CG and BiCGStab preconditioned by the cycle must report convergence as
// "cg+mg" / "bicgstab+mg" in fewer iterations than rows and leave a true residual of at most twice the tolerance.  Built by
// tests/test_multigrid_api.py (compile + link, no GPU needed) and run by tests/test_zzzzzzzzzz_multigrid.py on fixtures it writes.
#include "bmSpMatrix.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static std::vector<double> inverse(const bmsp::coo_matrix<double> &coo, size_t n)
{
    std::vector<double> a(n * n, 0.0), inv(n * n, 0.0);
    for (size_t k = 0; k < coo.num_entries; k++) a[(size_t)coo.row_indices[k] * n + (size_t)coo.column_indices[k]] = coo.values[k];
    for (size_t i = 0; i < n; i++) inv[i * n + i] = 1.0;
    for (size_t c = 0; c < n; c++) {
        size_t piv = c;
        for (size_t r = c + 1; r < n; r++)
            if (std::fabs(a[r * n + c]) > std::fabs(a[piv * n + c])) piv = r;
        for (size_t j = 0; j < n; j++) { std::swap(a[c * n + j], a[piv * n + j]); std::swap(inv[c * n + j], inv[piv * n + j]); }
        const double d = a[c * n + c];
        for (size_t j = 0; j < n; j++) { a[c * n + j] /= d; inv[c * n + j] /= d; }
        for (size_t r = 0; r < n; r++) {
            const double f = a[r * n + c];
            if (r == c || f == 0.0) continue;
            for (size_t j = 0; j < n; j++) { a[r * n + j] -= f * a[c * n + j]; inv[r * n + j] -= f * inv[c * n + j]; }
        }
    }
    return inv;
}

template <class T> static bool check(const std::string &a0, const std::string &p, const std::string &a1, const char *name, double tol)
{
    typedef typename bmsp::vector_of<T>::type R;
    bool ok = true;
    for (int lay = 0; lay < 2; lay++) {
        bmSpMatrix<T> A0(a0, lay != 0), P(p, lay == 0), A1(a1, false);
        const bmsp::coo_matrix<double> &coo = A0.host_coo();
        const size_t n = (size_t)A0.num_rows, nc = (size_t)A1.num_rows;
        const std::vector<double> inv64 = inverse(A1.host_coo(), nc);
        bmsp::device_vector<R> inv(std::vector<R>(inv64.begin(), inv64.end()));
        std::vector<bmSpMatrix<T> *> As, Ps;
        As.push_back(&A0); As.push_back(&A1); Ps.push_back(&P);
        bmSpMultigrid<T> mg(As, Ps, std::vector<bmSpMatrix<T> *>(), inv.data());
        bmsp_mg_info_t mi;
        mg.info(&mi);
        ok = ok && mi.levels == 2 && mi.n[0] == (int64_t)n && mi.n[1] == (int64_t)nc && mi.restrict_mode[0] == BMSP_MG_RESTRICT_PT && mi.coarse_exact == 1;
        std::vector<R> hb(n);
        for (size_t i = 0; i < n; i++) hb[i] = (R)(0.5 + (double)((i * 7) % 11) / 8.0) * (i % 3 ? (R)1 : (R)-1);
        bmsp::device_vector<R> b(hb), x(n);
        const auto residual = [&](const std::vector<R> &hx) {
            std::vector<double> res(hb.begin(), hb.end());
            for (size_t k = 0; k < coo.num_entries; k++) res[(size_t)coo.row_indices[k]] -= coo.values[k] * (double)hx[(size_t)coo.column_indices[k]];
            double rr = 0.0, bb = 0.0;
            for (size_t i = 0; i < n; i++) { rr += res[i] * res[i]; bb += (double)hb[i] * (double)hb[i]; }
            return std::sqrt(rr / bb);
        };
        mg.vcycle(b.data(), x.data());
        ok = ok && residual(x.to_host()) < 1.0;
        for (int method = 0; method < 2; method++) {
            bmsp_krylov_info info;
            std::vector<double> hist(n, -1.0);
            mg.solve(method, b.data(), x.data(), 0, tol, 0, hist.data(), &info);
            ok = ok && info.status == BMSP_KRYLOV_CONVERGED && info.iterations >= 1 && info.iterations < (int64_t)n && info.relres <= tol;
            ok = ok && residual(x.to_host()) <= 2.0 * tol && hist[(size_t)info.iterations - 1] == info.relres;
            ok = ok && !std::strcmp(info.method, method ? "bicgstab+mg" : "cg+mg") && info.precond_applies >= info.iterations;
        }
    }
    std::printf("CHECK multigrid %s %s\n", name, ok ? "OK" : "FAIL");
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: %s A0.mtx P.mtx A1.mtx\n", argv[0]); return 2; }
    try {
        const bool f = check<float>(argv[1], argv[2], argv[3], "float", 1e-5), d = check<double>(argv[1], argv[2], argv[3], "double", 1e-10);
        return f && d ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
