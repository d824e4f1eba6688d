// cpp_numeric_refresh_check.cpp -- the sequence bmSparse_mult_symbolic / bmSparse_mult_numeric exist for, through include/bmSpMatrix.h as
// the reference's user would write it: C = A * P once, D1 = C * R (C is a left operand: the product builds C's value-derived caches), new
// values in A on the same structure (written through the public values pointer, then bmsp_matrix_invalidate(A, 0) as bmsp.h asks),
// bmSparse_mult_numeric(A, P, C) and D2 = C * R.  D2 must be, bit for bit, the product of a C made afresh from C's four arrays (a handle
// without caches), and must be exactly twice D1 (the new values are twice the old ones; a stale cache returns D1 itself).  Built and run by
// tests/test_value_cache_coherence.py on a Laplacian fixture.
#include "bmSpMatrix.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

template <class T> static bool same_bits(const std::vector<T> &x, const std::vector<T> &y)
{
    return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), x.size() * sizeof(T)) == 0);
}

static bool same_matrix(bmSpMatrix<float> &X, bmSpMatrix<float> &Y)
{
    return X.num_rows == Y.num_rows && X.num_cols == Y.num_cols && same_bits(X.keys.to_host(), Y.keys.to_host()) &&
           same_bits(X.bmps.to_host(), Y.bmps.to_host()) && same_bits(X.offsets.to_host(), Y.offsets.to_host()) &&
           same_bits(X.values.to_host(), Y.values.to_host());
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s A.mtx\n", argv[0]); return 2; }
    try {
        const std::string path = argv[1];
        bmSpMatrix<float> A(path, false), P(path, true), R(path, true);
        bmSpMatrix<float> C, D1, D2, Df;
        bmsp_spgemm_stats st;
        bmSparse_mult(A, P, C, false, false, 5);
        bmSparse_mult(C, R, D1, false, false, 5, &st);  // builds C's caches
        const int variant1 = st.mac_variant;
        // new values in A: twice the old ones (exact), same structure
        std::vector<float> v = A.values.to_host();
        for (float &x : v) x *= 2.0f;
        if (!v.empty()) bmsp::check(bmsp_memcpy_h2d(A.values.data(), v.data(), v.size() * sizeof(float)));
        bmsp::check(bmsp_matrix_invalidate(A.handle(), 0));
        bmSparse_mult_numeric(A, P, C, 5);
        bmSparse_mult(C, R, D2, false, false, 5, &st);
        const int variant2 = st.mac_variant;
        // a C without caches: the adopting constructor on copies of C's arrays
        bmsp::device_vector<uint64_t> k(C.keys.to_host()), b(C.bmps.to_host()), o(C.offsets.to_host());
        bmsp::device_vector<float> cv(C.values.to_host());
        bmSpMatrix<float> Cf(C.num_rows, C.num_cols, C.block_num, k, b, o, cv);
        bmSparse_mult(Cf, R, Df, false, false, 5, &st);
        const bool fresh = same_matrix(D2, Df) && st.mac_variant == variant2;
        // not vacuous: doubling A doubles C and D exactly (a power of two), so D2 == 2 * D1 value by value and D2 != D1 wherever D1 != 0
        const std::vector<float> d1 = D1.values.to_host(), d2 = D2.values.to_host();
        bool doubled = d1.size() == d2.size() && !d1.empty();
        size_t changed = 0;
        for (size_t i = 0; doubled && i < d1.size(); i++) {
            doubled = d2[i] == 2.0f * d1[i];
            changed += d2[i] != d1[i];
        }
        std::printf("CHECK numeric_refresh variants %d %d values %zu changed %zu %s %s\n", variant1, variant2, d1.size(), changed, fresh ? "FRESH_OK" : "FRESH_FAIL",
                    doubled ? "DOUBLED_OK" : "DOUBLED_FAIL");
        return fresh && doubled && changed > 0 ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
