// cpp_spsv_check.cpp -- bmSparse_SpSV / bmSparse_SpSV_analyse from include/bmSpMatrix.h for float, half and double, used as the reference's
// user would: on a row-major and a column-major build of one square MatrixMarket file with a full diagonal, both triangles, both ops and
// both kinds of diagonal are solved and compared for equality with a sequential substitution on the host COO -- one std::fma per stored
// entry in chain order, one division per row, the arithmetic the call fixes (this file is compiled with -ffp-contract=off).  Built by
// tests/test_spsv_api.py (compile + link, no GPU needed) and run by tests/test_spsv.py on a fixture it writes.
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
                    // the effective triangle as (row, col, value), rows in solve order, columns in chain order
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
                    std::vector<R> want(n);
                    size_t e = 0;
                    for (size_t k = 0; k < n; k++) {
                        const size_t i = lower ? k : n - 1 - k;
                        R s = alpha * hb[i];
                        for (; e < es.size() && es[e].r == i; e++) s = std::fma(-es[e].v, want[es[e].c], s);
                        want[i] = diag == BMSP_DIAG_UNIT ? s : s / d[i];
                    }
                    bmsp_spsv_info info;
                    bmSparse_SpSV_analyse(A, op, fill, diag, &info);
                    ok = ok && info.levels >= 1 && info.launches >= 1;
                    bmsp::device_vector<R> b(hb), x(n);
                    bmSparse_SpSV(A, op, fill, diag, -1.5, b.data(), x.data());
                    ok = ok && same_bits(x.to_host(), want) && same_bits(b.to_host(), hb);
                    bmSparse_SpSV(A, op, fill, diag, -1.5, b.data(), b.data());  // in place
                    ok = ok && same_bits(b.to_host(), want);
                }
    }
    std::printf("CHECK spsv %s %s\n", name, ok ? "OK" : "FAIL");
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
