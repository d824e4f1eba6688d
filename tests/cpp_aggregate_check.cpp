// cpp_aggregate_check.cpp -- bmSparse_aggregate and bmSpMatrix<T>::from_aggregates from include/bmSpMatrix.h for float, half and double,
// used as the reference's user would, on a row-major and a column-major build of one square MatrixMarket file.  Printed for the caller to
// compare with its own reference: the aggregate map and the counts ("AGG", "INFO" lines, float and row-major only: they depend on
// structure alone).  Checked here: the prolongator of the map holds exactly one entry (i, agg[i], 1) per row.
// Built by tests/test_aggregate_api.py (compile + link, no GPU needed) and run by tests/test_zzzzzzzzz_aggregate.py on a fixture it writes.
#include "bmSpMatrix.h"
#include <cstdio>
#include <string>
#include <vector>

template <class T> static bool check(const std::string &path, const char *name, bool print)
{
    bool ok = true;
    for (int lay = 0; lay < 2; lay++) {
        bmSpMatrix<T> S(path, lay != 0);
        const size_t n = (size_t)S.num_rows;
        if ((size_t)S.num_cols != n) { std::fprintf(stderr, "the fixture must be square\n"); return false; }
        bmsp::device_vector<uint32_t> agg;
        bmsp_aggregate_info info;
        const int64_t count = bmSparse_aggregate(S, agg, 0, &info);
        const std::vector<uint32_t> ha = agg.to_host();
        ok = ok && ha.size() == n && info.nodes == (int64_t)n && info.aggregates == count;
        if (print && lay == 0) {
            std::printf("AGG");
            for (uint32_t a : ha) std::printf(" %u", a);
            std::printf("\nINFO %lld %lld %lld\n", (long long)info.nodes, (long long)info.aggregates, (long long)info.rounds);
        }
        for (int out_lay = 0; out_lay < 2; out_lay++) {
            bmSpMatrix<T> P = bmSpMatrix<T>::from_aggregates((int)n, (int)count, agg.data(), nullptr, out_lay != 0);
            ok = ok && (size_t)P.num_rows == n && P.num_cols == (int)count && P.nnz == (int64_t)n;
            const bmsp::coo_matrix<double> coo = P.host_coo();
            std::vector<int> seen(n, 0);
            for (size_t k = 0; k < coo.num_entries; k++) {
                const size_t r = (size_t)coo.row_indices[k];
                ok = ok && r < n && (uint32_t)coo.column_indices[k] == ha[r] && coo.values[k] == 1.0 && !seen[r];
                if (r < n) seen[r] = 1;
            }
        }
    }
    std::printf("CHECK aggregate %s %s\n", name, ok ? "OK" : "FAIL");
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s S.mtx\n", argv[0]); return 2; }
    try {
        const std::string path = argv[1];
        const bool f = check<float>(path, "float", true), h = check<half>(path, "half", false), d = check<double>(path, "double", false);
        return f && h && d ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
