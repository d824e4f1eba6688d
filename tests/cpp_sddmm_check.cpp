// cpp_sddmm_check.cpp -- bmSparse_sddmm / bmSparse_sddmm_values from include/bmSpMatrix.h for float, half and double, used as the
// reference's user would: with X and Y of small integers every dot product is exact, so C = 2 * (X . Y^T) on the pattern of one
// MatrixMarket file is compared for equality with the host COO, out of place in both layouts and in place.  Built by
// tests/test_sddmm_api.py (compile + link, no GPU needed) and run by tests/test_sddmm.py on the data/real fixture.
#include "bmSpMatrix.h"
#include <cstdio>
#include <string>
#include <vector>

static half to_half(int x)
{
    // small integers |x| < 2048 are exact in binary16
    half h;
    uint16_t sign = x < 0 ? 0x8000u : 0u;
    unsigned a = (unsigned)(x < 0 ? -x : x);
    if (a == 0) { h.bits = sign; return h; }
    int e = 0;
    while ((a >> (e + 1)) != 0) e++;
    h.bits = (uint16_t)(sign | ((unsigned)(e + 15) << 10) | ((a << (10 - e)) & 0x3ffu));
    return h;
}
template <class T> static T make(int x) { return (T)x; }
template <> half make<half>(int x) { return to_half(x); }

template <class T> static bool same(bmSpMatrix<T> &C, const std::vector<double> &want, const bmsp::coo_matrix<double> &coo)
{
    C.generate_coo();  // (S in place: its host copy is from before the call)
    const bmsp::coo_matrix<double> &got = C.host_coo();
    bool ok = got.num_entries == coo.num_entries;
    for (size_t e = 0; ok && e < coo.num_entries; e++)
        ok = got.row_indices[e] == coo.row_indices[e] && got.column_indices[e] == coo.column_indices[e] && got.values[e] == want[e];
    return ok;
}

template <class T> static bool check(const std::string &path, const char *name)
{
    const int k = 5;
    bool ok = true;
    for (int lay = 0; lay < 2; lay++) {
        bmSpMatrix<T> S(path, lay != 0);
        const bmsp::coo_matrix<double> coo = S.host_coo();
        const size_t nr = (size_t)S.num_rows, nc = (size_t)S.num_cols;
        std::vector<T> hx(nr * k), hy(nc * k);
        std::vector<int> ix(nr * k), iy(nc * k);
        for (size_t i = 0; i < ix.size(); i++) { ix[i] = (int)(i % 7) - 3; hx[i] = make<T>(ix[i]); }
        for (size_t i = 0; i < iy.size(); i++) { iy[i] = (int)(i % 5) - 2; hy[i] = make<T>(iy[i]); }
        std::vector<double> want(coo.num_entries);
        for (size_t e = 0; e < coo.num_entries; e++) {
            int d = 0;
            for (int t = 0; t < k; t++) d += ix[(size_t)coo.row_indices[e] * k + t] * iy[(size_t)coo.column_indices[e] * k + t];
            want[e] = 2.0 * d;
        }
        bmsp::device_vector<T> X(hx), Y(hy);
        bmSpMatrix<T> C, Ct;
        bmSparse_sddmm(S, X.data(), Y.data(), k, C, 2.0);
        bmSparse_sddmm(S, X.data(), Y.data(), k, Ct, 1.0, 0.0, 0, lay == 0);
        bmSparse_sddmm_values(S, X.data(), Y.data(), k, Ct, 2.0);  // into the other layout's output
        bmSparse_sddmm_values(S, X.data(), Y.data(), k, S, 2.0);   // in place
        ok = ok && same(C, want, coo) && same(Ct, want, coo) && same(S, want, coo);
    }
    std::printf("CHECK sddmm %s %s\n", name, ok ? "OK" : "FAIL");
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
