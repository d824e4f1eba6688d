// cpp_spitsv_check.cpp -- bmSparse_SpITSV from include/bmSpMatrix.h for float, half and double, used as the reference's user would: on a
// row-major and a column-major build of one square MatrixMarket file with a full diagonal, for both triangles, both ops and both kinds of
// diagonal, (a) run to the fixed point (max_iter = 0, tol = 0) it gives the bits of bmSparse_SpSV and reports convergence within
// levels + 1 sweeps; (b) two sweeps without a check equal two sweeps of a row loop on the host COO -- one std::fma per stored entry in
// chain order, x from the new vector inside the row's block of eight and from the previous iterate outside, one division per row (this file
// is compiled with -ffp-contract=off).  Built by tests/test_spitsv_api.py (compile + link, no GPU needed) and run by tests/test_zz_spitsv.py
// on a fixture it writes.
#include "bmSpMatrix.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

template <class R> static bool same_bits(const std::vector<R> &a, const std::vector<R> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(R)) == 0);
}

template <class T> static bool check(const std::string &path, const char *name)
{
    typedef typename bmsp::vector_of<T>::type R;
    bool ok = true;
    for (int lay = 0; lay < 2; lay++) {
        bmSpMatrix<T> A(path, lay != 0);
        const bmsp::coo_matrix<double> &coo = A.host_coo();  // the stored values, exactly
        const size_t n = (size_t)A.num_rows;
        if ((size_t)A.num_cols != n) { std::fprintf(stderr, "the fixture must be square\n"); return false; }
        std::vector<R> hb(n);
        for (size_t i = 0; i < n; i++) hb[i] = (R)(0.5 + (double)((i * 7) % 11) / 8.0) * (i % 3 ? (R)1 : (R)-1);
        for (int op = 0; op < 2; op++)
            for (int fill = 0; fill < 2; fill++)
                for (int diag = 0; diag < 2; diag++) {
                    const bool lower = (fill == BMSP_FILL_LOWER) != (op == BMSP_OP_T);
                    struct E { size_t r, c; R v; };
                    std::vector<E> es;
                    std::vector<R> d(n, (R)1);
                    for (size_t k = 0; k < coo.num_entries; k++) {
                        size_t r = (size_t)coo.row_indices[k], c = (size_t)coo.column_indices[k];
                        if (fill == BMSP_FILL_LOWER ? r < c : r > c) continue;
                        if (op == BMSP_OP_T) std::swap(r, c);
                        if (r == c) d[r] = (R)coo.values[k];
                        else es.push_back(E{r, c, (R)coo.values[k]});
                    }
                    std::sort(es.begin(), es.end(), [lower](const E &a, const E &b) {
                        if (a.r != b.r) return lower ? a.r < b.r : a.r > b.r;
                        return lower ? a.c < b.c : a.c > b.c;
                    });
                    const R alpha = (R)-1.5;
                    std::vector<R> prev(n, (R)0), next(n, (R)0);
                    for (int sweep = 0; sweep < 2; sweep++) {
                        size_t e = 0;
                        for (size_t k = 0; k < n; k++) {
                            const size_t i = lower ? k : n - 1 - k;
                            R s = alpha * hb[i];
                            for (; e < es.size() && es[e].r == i; e++)
                                s = std::fma(-es[e].v, es[e].c / 8 == i / 8 ? next[es[e].c] : prev[es[e].c], s);
                            next[i] = diag == BMSP_DIAG_UNIT ? s : s / d[i];
                        }
                        prev.swap(next);
                    }
                    bmsp::device_vector<R> b(hb), x(n), exact(n);
                    bmsp_spitsv_info info;
                    bmSparse_SpITSV(A, op, fill, diag, -1.5, b.data(), x.data(), 2, BMSP_ITSV_NO_CHECK, 0, nullptr, &info);
                    ok = ok && same_bits(x.to_host(), prev) && info.sweeps == 2 && info.converged == 0 && info.delta == -1.0;
                    bmSparse_SpSV(A, op, fill, diag, -1.5, b.data(), exact.data());
                    std::vector<double> hist(4096, -1.0);
                    bmSparse_SpITSV(A, op, fill, diag, -1.5, b.data(), x.data(), 0, 0.0, 0, hist.data(), &info);
                    ok = ok && same_bits(x.to_host(), exact.to_host()) && same_bits(b.to_host(), hb);
                    ok = ok && info.converged == 1 && info.sweeps >= 1 && info.sweeps <= info.levels + 1 && info.delta == 0.0;
                    ok = ok && hist[(size_t)info.sweeps - 1] == 0.0 && hist[(size_t)info.sweeps] == -1.0;
                }
    }
    std::printf("CHECK spitsv %s %s\n", name, ok ? "OK" : "FAIL");
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
