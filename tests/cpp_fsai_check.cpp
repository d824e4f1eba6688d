// cpp_fsai_check.cpp -- bmSparse_fsai and bmSpFsai<T> from include/bmSpMatrix.h for float and double, used as the reference's user would:
// A (symmetric positive definite) and the pattern S read from two MatrixMarket files, both column-major, the SPD kind with column-major
// factors.  One application and one CG solve; for float the two vectors are written to `out` (z then x, raw floats) so that the caller
// can compare them with the same calls made through ctypes.  Also checked here: the solve converges as "cg+fsai" with a true residual of
// at most twice the tolerance, the factor from bmSparse_fsai has S's size, and GENERAL + BiCGStab / GMRES converge.  Built by
// tests/test_fsai_api.py (compile + link, no GPU needed) and run by tests/test_zzzzzzzzzzzzz_fsai.py on fixtures it writes.
#include "bmSpMatrix.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

template <class T> static bool check(const std::string &a, const std::string &s, const char *name, double tol, const char *out)
{
    typedef typename bmsp::vector_of<T>::type R;
    bmSpMatrix<T> A(a, true), S(s, true), G;
    const bmsp::coo_matrix<double> &coo = A.host_coo();
    const size_t n = (size_t)A.num_rows;
    bool ok = true;
    bmsp_fsai_info gi;
    bmSparse_fsai(A, BMSP_OP_N, S, G, BMSP_FSAI_SCALE_SQRT, true, (R *)nullptr, &gi);
    ok = ok && G.num_rows == S.num_rows && gi.rows == (int64_t)n && gi.bad_rows == 0 && gi.lanes >= gi.max_row;
    std::vector<R> hb(n);
    for (size_t i = 0; i < n; i++) hb[i] = (R)(0.5 + (double)((i * 7) % 11) / 8.0) * (i % 3 ? (R)1 : (R)-1);
    bmsp::device_vector<R> b(hb), x(n), z(n);
    const auto residual = [&](const std::vector<R> &hx) {
        std::vector<double> res(hb.begin(), hb.end());
        for (size_t k = 0; k < coo.num_entries; k++) res[(size_t)coo.row_indices[k]] -= coo.values[k] * (double)hx[(size_t)coo.column_indices[k]];
        double rr = 0.0, bb = 0.0;
        for (size_t i = 0; i < n; i++) { rr += res[i] * res[i]; bb += (double)hb[i] * (double)hb[i]; }
        return std::sqrt(rr / bb);
    };
    {
        bmSpFsai<T> f(A, S, BMSP_FSAI_SPD, BMSP_FSAI_COLMAJOR);
        bmsp_fsai_handle_info hi;
        f.info(&hi);
        ok = ok && hi.kind == BMSP_FSAI_SPD && hi.n == (int64_t)n && hi.materialised == 1 && hi.factor[0].bad_rows == 0;
        f.apply(b.data(), z.data());
        bmsp_krylov_info info;
        f.solve(BMSP_KRYLOV_CG, b.data(), x.data(), 0, tol, 0, nullptr, &info);
        ok = ok && info.status == BMSP_KRYLOV_CONVERGED && info.iterations >= 1 && info.relres <= tol && !std::strcmp(info.method, "cg+fsai");
        ok = ok && info.precond_applies == info.iterations && residual(x.to_host()) <= 2.0 * tol;
        if (out) {
            FILE *fp = std::fopen(out, "wb");
            if (!fp) return false;
            const std::vector<R> hz = z.to_host(), hx = x.to_host();
            std::fwrite(hz.data(), sizeof(R), n, fp);
            std::fwrite(hx.data(), sizeof(R), n, fp);
            std::fclose(fp);
        }
        f.update();
        bmsp::device_vector<R> z2(n);
        f.apply(b.data(), z2.data());
        ok = ok && !std::memcmp(z2.to_host().data(), z.to_host().data(), n * sizeof(R));
    }
    {
        bmSpFsai<T> f(A, S, BMSP_FSAI_GENERAL, BMSP_FSAI_NO_MATERIALISE);
        bmsp_krylov_info info;
        f.solve(BMSP_KRYLOV_BICGSTAB, b.data(), x.data(), 0, tol, 0, nullptr, &info);
        ok = ok && info.status == BMSP_KRYLOV_CONVERGED && !std::strcmp(info.method, "bicgstab+fsai") && residual(x.to_host()) <= 2.0 * tol;
        f.solve_gmres(30, b.data(), x.data(), 0, tol, 0, nullptr, &info);
        ok = ok && info.status == BMSP_KRYLOV_CONVERGED && !std::strcmp(info.method, "gmres(30)+fsai") && residual(x.to_host()) <= 2.0 * tol;
    }
    std::printf("CHECK fsai %s %s\n", name, ok ? "OK" : "FAIL");
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: %s A.mtx S.mtx out.bin\n", argv[0]); return 2; }
    try {
        const bool f = check<float>(argv[1], argv[2], "float", 1e-5, argv[3]), d = check<double>(argv[1], argv[2], "double", 1e-10, nullptr);
        return f && d ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
