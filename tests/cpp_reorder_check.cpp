// cpp_reorder_check.cpp -- bmSparse_color_blocks / bmSparse_permute_blocks / bmSparse_vec_permute_blocks and bmSpMatrix<T>::permute_blocks
// from include/bmSpMatrix.h for float, half and double, used as the reference's user would, on a row-major and a column-major build of one
// square MatrixMarket file.  Printed for the caller to compare with its own reference: the colours, the ordering and the counts ("COLORS",
// "PERM", "INFO" lines, float and row-major only: they depend on structure alone).  Checked here: the permuted matrix holds exactly the
// entries of A with both indices mapped through the inverse of the ordering, the levels of its triangles, and the vectors' round trip.
// Built by tests/test_reorder_api.py (compile + link, no GPU needed) and run by tests/test_zzzzzz_reorder.py on a fixture it writes.
#include "bmSpMatrix.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

typedef std::tuple<int, int, double> Entry;

static std::vector<Entry> entries(const bmsp::coo_matrix<double> &coo, const std::vector<uint32_t> *inv)
{
    std::vector<Entry> es;
    for (size_t k = 0; k < coo.num_entries; k++) {
        int r = coo.row_indices[k], c = coo.column_indices[k];
        if (inv) {
            r = (int)(*inv)[(size_t)r / 8] * 8 + r % 8;
            c = (int)(*inv)[(size_t)c / 8] * 8 + c % 8;
        }
        es.push_back(Entry(r, c, coo.values[k]));
    }
    std::sort(es.begin(), es.end());
    return es;
}

template <class T> static bool check(const std::string &path, const char *name, bool print)
{
    typedef typename bmsp::vector_of<T>::type R;
    bool ok = true;
    for (int lay = 0; lay < 2; lay++) {
        bmSpMatrix<T> A(path, lay != 0);
        const size_t n = (size_t)A.num_rows, nb = (n + 7) / 8;
        if ((size_t)A.num_cols != n) { std::fprintf(stderr, "the fixture must be square\n"); return false; }
        bmsp::device_vector<uint32_t> colors, perm;
        bmsp_color_info info;
        bmSparse_color_blocks(A, colors, perm, 0, &info);
        const std::vector<uint32_t> hc = colors.to_host(), hp = perm.to_host();
        ok = ok && hc.size() == nb && hp.size() == nb && info.blocks == (int64_t)nb;
        if (print && lay == 0) {
            std::printf("COLORS");
            for (uint32_t c : hc) std::printf(" %u", c);
            std::printf("\nPERM");
            for (uint32_t p : hp) std::printf(" %u", p);
            std::printf("\nINFO %lld %lld %lld\n", (long long)info.blocks, (long long)info.colors, (long long)info.rounds);
        }
        std::vector<uint32_t> inv(nb, 0u);
        for (size_t i = 0; i < nb; i++) {
            if (hp[i] >= nb) return false;
            inv[hp[i]] = (uint32_t)i;
        }
        for (int out_lay = 0; out_lay < 2; out_lay++) {
            bmSpMatrix<T> B;
            bmSparse_permute_blocks(A, perm.data(), perm.data(), B, out_lay != 0);
            bmSpMatrix<T> B2 = A.permute_blocks(perm.data(), perm.data(), out_lay != 0);
            ok = ok && (size_t)B.num_rows == n && B.nnz == A.nnz && B.block_num == A.block_num;
            ok = ok && entries(B.host_coo(), nullptr) == entries(A.host_coo(), &inv);
            ok = ok && entries(B2.host_coo(), nullptr) == entries(B.host_coo(), nullptr);
            for (int fill = 0; fill < 2; fill++) {
                bmsp_spsv_info si;
                bmSparse_SpSV_analyse(B, BMSP_OP_N, fill, BMSP_DIAG_UNIT, &si);
                ok = ok && (n % 8 ? si.levels <= info.colors : si.levels == info.colors);
            }
        }
        std::vector<R> hx(n);
        for (size_t i = 0; i < n; i++) hx[i] = (R)(1.0 + (double)i);
        bmsp::device_vector<R> x(hx), y(n), z(n);
        bmSparse_vec_permute_blocks((int64_t)n, perm.data(), x.data(), y.data());
        bmSparse_vec_permute_blocks((int64_t)n, perm.data(), y.data(), z.data(), true);
        const std::vector<R> hy = y.to_host(), hz = z.to_host();
        for (size_t i = 0; i < n; i++) ok = ok && hy[i] == hx[(size_t)hp[i / 8] * 8 + i % 8] && hz[i] == hx[i];
    }
    std::printf("CHECK reorder %s %s\n", name, ok ? "OK" : "FAIL");
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s A.mtx\n", argv[0]); return 2; }
    try {
        const std::string path = argv[1];
        const bool f = check<float>(path, "float", true), h = check<half>(path, "half", false), d = check<double>(path, "double", false);
        return f && h && d ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
