// capi.hip -- the extern "C" surface declared in include/bmsp.h.  Translates exceptions to status codes;
// no other logic lives here.
#include "matrix.h"
#include "prims.hip.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <omp.h>
#include <vector>

namespace bmsp {
const std::string &last_error();
void partition_rows(bmsp_matrix_s *A, bmsp_matrix_s *B, int parts, int64_t *bounds, hipStream_t st, uint64_t *total_out = nullptr);
void spgemm_paneled(bmsp_matrix_s *A, bmsp_matrix_s *B, bmsp_matrix_s **C, int mode, int tc_version, int verbose, hipStream_t st,
                    bmsp_spgemm_stats *stats);
bmsp_matrix_s *row_panel(bmsp_matrix_s *m, int64_t rb, int64_t re, hipStream_t st);
bmsp_matrix_s *concat_panels(int num_rows, int num_cols, int parts, const int64_t *block_nums, const int64_t *nnzs,
                             uint64_t *const *d_keys, uint64_t *const *d_bmps, uint64_t *const *d_offsets, void *const *d_values,
                             bmsp_dtype dtype, hipStream_t st);
}  // namespace bmsp

using namespace bmsp;

// host CSR container (class CSRMatrix, include/CSRMatrix.h:13-21)
struct bmsp_csr_s {
    int num_rows = 0, num_cols = 0;
    std::vector<int> row_offsets, cols;
    std::vector<float> vals;
    // device forms, built on first use and cached
    bmsp_matrix_s *dev_normal = nullptr, *dev_transposed = nullptr;
    ~bmsp_csr_s()
    {
        free_matrix(dev_normal);
        free_matrix(dev_transposed);
    }
};

#define BMSP_API_BEGIN try {
#define BMSP_API_END                                         \
    return BMSP_OK;                                          \
    }                                                        \
    catch (const bmsp::Error &e)                             \
    {                                                        \
        bmsp::set_last_error(e.what());                      \
        return e.status;                                     \
    }                                                        \
    catch (const std::bad_alloc &)                           \
    {                                                        \
        bmsp::set_last_error("host allocation failed");      \
        return BMSP_ERR_NOMEM;                               \
    }                                                        \
    catch (const std::exception &e)                          \
    {                                                        \
        bmsp::set_last_error(e.what());                      \
        return BMSP_ERR_INVALID;                             \
    }

static void need(const void *p, const char *what)
{
    if (!p) fail(BMSP_ERR_INVALID, "%s is null", what);
}

// what every solve entry refuses about its handle and its vectors, between the argument checks and the operand checks
static void need_solve_operands(const void *handle, const char *what, const void *d_b, const void *d_x)
{
    need(handle, what); need(d_b, "d_b"); need(d_x, "d_x");
    if (d_b == d_x) fail(BMSP_ERR_INVALID, "d_x must not be d_b: b is read after x has been written");
}

static bmsp_matrix_s *build_from_host_coo(int num_rows, int num_cols, int64_t nnz, const int *rows, const int *cols, const double *vals,
                                          int transposed, bmsp_dtype dtype)
{
    if (dtype != BMSP_F32 && dtype != BMSP_F16 && dtype != BMSP_F64) fail(BMSP_ERR_INVALID, "unknown dtype %d", (int)dtype);
    for (int64_t i = 0; i < nnz; i++)
        if (rows[i] < 0 || rows[i] >= num_rows || cols[i] < 0 || cols[i] >= num_cols)
            fail(BMSP_ERR_INVALID, "entry %lld has index (%d,%d) outside %dx%d", (long long)i, rows[i], cols[i], num_rows, num_cols);
    size_t n = (size_t)nnz;
    DevBuf<int> dr(n), dc(n);
    DevBuf<double> dv(n);
    if (n) {
        copy_h2d_staged(dr.p, rows, sizeof(int) * n);
        copy_h2d_staged(dc.p, cols, sizeof(int) * n);
        copy_h2d_staged(dv.p, vals, sizeof(double) * n);
    }
    return build_from_device_coo(num_rows, num_cols, nnz, dr.p, dc.p, dv.p, transposed, dtype, nullptr);
}

extern "C" {

const char *bmsp_last_error(void) { return bmsp::last_error().c_str(); }
const char *bmsp_version(void) { return "bmsparse-mi355x 0.1 (gfx950)"; }

int bmsp_device_count(int *count)
{
    BMSP_API_BEGIN
    need(count, "count");
    BMSP_HIP(hipGetDeviceCount(count));
    BMSP_API_END
}
int bmsp_set_device(int device)
{
    BMSP_API_BEGIN
    BMSP_HIP(hipSetDevice(device));
    BMSP_API_END
}
int bmsp_malloc(void **dptr, size_t bytes)
{
    BMSP_API_BEGIN
    need(dptr, "dptr");
    *dptr = pool_alloc(bytes);
    BMSP_API_END
}
int bmsp_free(void *dptr)
{
    BMSP_API_BEGIN
    pool_free(dptr);
    BMSP_API_END
}
int bmsp_memcpy_h2d(void *dst, const void *src, size_t bytes)
{
    BMSP_API_BEGIN
    copy_h2d_staged(dst, src, bytes);
    BMSP_API_END
}
int bmsp_memcpy_d2h(void *dst, const void *src, size_t bytes)
{
    BMSP_API_BEGIN
    copy_d2h_staged(dst, src, bytes);
    BMSP_API_END
}
int bmsp_memcpy_d2d(void *dst, const void *src, size_t bytes)
{
    BMSP_API_BEGIN
    if (bytes) BMSP_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice));
    BMSP_API_END
}
int bmsp_memset(void *dptr, int value, size_t bytes)
{
    BMSP_API_BEGIN
    if (bytes) BMSP_HIP(hipMemset(dptr, value, bytes));
    BMSP_API_END
}
int bmsp_synchronize(void)
{
    BMSP_API_BEGIN
    BMSP_HIP(hipDeviceSynchronize());
    BMSP_API_END
}
int bmsp_trim_pool(void)
{
    BMSP_API_BEGIN
    pool_trim();
    BMSP_API_END
}

int bmsp_event_create(void **event)
{
    BMSP_API_BEGIN
    need(event, "event");
    hipEvent_t e;
    BMSP_HIP(hipEventCreate(&e));
    *event = (void *)e;
    BMSP_API_END
}
int bmsp_event_record(void *event, void *stream)
{
    BMSP_API_BEGIN
    BMSP_HIP(hipEventRecord((hipEvent_t)event, as_stream(stream)));
    BMSP_API_END
}
int bmsp_event_elapsed_ms(void *start, void *stop, float *ms)
{
    BMSP_API_BEGIN
    need(ms, "ms");
    BMSP_HIP(hipEventSynchronize((hipEvent_t)stop));
    BMSP_HIP(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    BMSP_API_END
}
int bmsp_event_destroy(void *event)
{
    BMSP_API_BEGIN
    if (event) BMSP_HIP(hipEventDestroy((hipEvent_t)event));
    BMSP_API_END
}

int bmsp_matrix_from_mtx(const char *path, int transposed, bmsp_dtype dtype, bmsp_matrix_t *out)
{
    BMSP_API_BEGIN
    load_kernels();
    need(path, "path");
    need(out, "out");
    HostCoo coo;
    read_matrix_market(path, coo);
    *out = build_from_host_coo(coo.num_rows, coo.num_cols, (int64_t)coo.rows.size(), coo.rows.data(), coo.cols.data(), coo.vals.data(),
                               transposed, dtype);
    BMSP_API_END
}

int bmsp_matrix_from_coo(int num_rows, int num_cols, int64_t nnz, const int *rows, const int *cols, const double *vals, int transposed,
                         bmsp_dtype dtype, bmsp_matrix_t *out)
{
    BMSP_API_BEGIN
    load_kernels();
    need(out, "out");
    if (nnz > 0) { need(rows, "rows"); need(cols, "cols"); need(vals, "vals"); }
    *out = build_from_host_coo(num_rows, num_cols, nnz, rows, cols, vals, transposed, dtype);
    BMSP_API_END
}

int bmsp_matrix_from_coo_device(int num_rows, int num_cols, int64_t nnz, const int *d_rows, const int *d_cols, const double *d_vals,
                                int transposed, bmsp_dtype dtype, void *stream, bmsp_matrix_t *out)
{
    BMSP_API_BEGIN
    load_kernels();
    need(out, "out");
    *out = build_from_device_coo(num_rows, num_cols, nnz, d_rows, d_cols, d_vals, transposed, dtype, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_from_arrays(int num_rows, int num_cols, int64_t block_num, int64_t nnz, uint64_t *d_keys, uint64_t *d_bmps,
                            uint64_t *d_offsets, void *d_values, bmsp_dtype dtype, int transposed, int ownership, bmsp_matrix_t *out)
{
    BMSP_API_BEGIN
    load_kernels();
    need(out, "out");
    if (block_num < 0 || nnz < 0 || num_rows < 0 || num_cols < 0) fail(BMSP_ERR_INVALID, "negative size");
    if (block_num > 0) { need(d_keys, "keys"); need(d_bmps, "bmps"); need(d_offsets, "offsets"); }
    if (nnz > 0) need(d_values, "values");
    if (ownership < 0 || ownership > 2) fail(BMSP_ERR_INVALID, "ownership must be 0, 1 or 2");
    auto m = make_matrix();
    m->num_rows = num_rows; m->num_cols = num_cols; m->block_num = block_num; m->nnz = nnz;
    m->dtype = dtype; m->transposed = transposed ? 1 : 0;
    const size_t nb = (size_t)block_num, es = dtype_size(dtype);
    // offsets always carry block_num+1 entries internally; the caller's array may hold only block_num
    // (the reference builder's, src/bmSpMatrix.cu:194), so the terminal entry is written here.
    uint64_t term = (uint64_t)nnz;
    if (ownership == 0 || ownership == 1) {
        m->ownership = 1;
        m->offsets = (uint64_t *)pool_alloc(8 * (nb + 1));
        if (nb) BMSP_HIP(hipMemcpy(m->offsets, d_offsets, 8 * nb, hipMemcpyDeviceToDevice));
        BMSP_HIP(hipMemcpy(m->offsets + nb, &term, 8, hipMemcpyHostToDevice));
        if (ownership == 1) {
            if ((nb && (!pool_owns(d_keys) || !pool_owns(d_bmps))) || (nnz && !pool_owns(d_values)))
                fail(BMSP_ERR_INVALID, "ownership=1 needs arrays allocated with bmsp_malloc");
            m->keys = d_keys; m->bmps = d_bmps; m->values = d_values;
            pool_free(d_offsets);  // adopted and replaced by the block_num+1 copy
        } else {
            alloc_tile_arrays(m.get(), nb);  // (the offsets are there)
            alloc_values(m.get(), (uint64_t)nnz);
            if (nb) {
                BMSP_HIP(hipMemcpy(m->keys, d_keys, 8 * nb, hipMemcpyDeviceToDevice));
                BMSP_HIP(hipMemcpy(m->bmps, d_bmps, 8 * nb, hipMemcpyDeviceToDevice));
            }
            if (nnz) BMSP_HIP(hipMemcpy(m->values, d_values, es * (size_t)nnz, hipMemcpyDeviceToDevice));
        }
    } else {
        // borrowed: the caller's offsets must already hold block_num+1 entries
        m->ownership = 2;
        m->keys = d_keys; m->bmps = d_bmps; m->offsets = d_offsets; m->values = d_values;
    }
    *out = m.release();
    BMSP_API_END
}

namespace {
struct CacheHeader {
    char magic[8];
    int32_t num_rows, num_cols, dtype, transposed;
    int64_t block_num, nnz;
};
const char kCacheMagic[8] = {'B', 'M', 'S', 'P', 'v', '1', 0, 0};
}  // namespace

int bmsp_matrix_save(bmsp_matrix_t m, const char *path)
{
    BMSP_API_BEGIN
    need(m, "matrix"); need(path, "path");
    if (m->ownership == 2 && m->view_block_begin) fail(BMSP_ERR_UNSUPPORTED, "row-panel views cannot be saved; save the parent");
    FILE *f = fopen(path, "wb");
    if (!f) fail(BMSP_ERR_IO, "cannot create '%s'", path);
    std::unique_ptr<FILE, int (*)(FILE *)> guard(f, fclose);
    CacheHeader h;
    memcpy(h.magic, kCacheMagic, 8);
    h.num_rows = m->num_rows; h.num_cols = m->num_cols; h.dtype = (int32_t)m->dtype; h.transposed = m->transposed;
    h.block_num = m->block_num; h.nnz = m->nnz;
    const size_t nb = (size_t)m->block_num, es = dtype_size(m->dtype);
    std::vector<char> buf;
    auto dump = [&](const void *dptr, size_t bytes) {
        buf.resize(bytes);
        copy_d2h_staged(buf.data(), dptr, bytes);
        if (bytes && fwrite(buf.data(), 1, bytes, f) != bytes) fail(BMSP_ERR_IO, "short write to '%s'", path);
    };
    if (fwrite(&h, sizeof h, 1, f) != 1) fail(BMSP_ERR_IO, "short write to '%s'", path);
    dump(m->keys, 8 * nb); dump(m->bmps, 8 * nb); dump(m->offsets, 8 * (nb + 1)); dump(m->values, es * (size_t)m->nnz);
    BMSP_API_END
}

int bmsp_matrix_load(const char *path, bmsp_matrix_t *out)
{
    BMSP_API_BEGIN
    load_kernels();
    need(path, "path"); need(out, "out");
    FILE *f = fopen(path, "rb");
    if (!f) fail(BMSP_ERR_IO, "cannot open '%s'", path);
    std::unique_ptr<FILE, int (*)(FILE *)> guard(f, fclose);
    CacheHeader h;
    if (fread(&h, sizeof h, 1, f) != 1 || memcmp(h.magic, kCacheMagic, 8) != 0) fail(BMSP_ERR_IO, "'%s' is not a bmSparse cache file", path);
    if (h.block_num < 0 || h.nnz < 0 || h.num_rows < 0 || h.num_cols < 0 || h.dtype < 0 || h.dtype > 2) fail(BMSP_ERR_IO, "'%s': corrupt header", path);
    auto m = make_matrix();
    m->num_rows = h.num_rows; m->num_cols = h.num_cols; m->dtype = (bmsp_dtype)h.dtype; m->transposed = h.transposed ? 1 : 0;
    m->block_num = h.block_num; m->nnz = h.nnz;
    const size_t nb = (size_t)h.block_num, es = dtype_size(m->dtype);
    std::vector<char> buf;
    auto slurp = [&](void **dptr, size_t bytes) {
        *dptr = pool_alloc(bytes ? bytes : 8);
        buf.resize(bytes);
        if (bytes && fread(buf.data(), 1, bytes, f) != bytes) fail(BMSP_ERR_IO, "'%s' is truncated", path);
        copy_h2d_staged(*dptr, buf.data(), bytes);
    };
    slurp((void **)&m->keys, 8 * nb); slurp((void **)&m->bmps, 8 * nb); slurp((void **)&m->offsets, 8 * (nb + 1));
    slurp(&m->values, es * (size_t)h.nnz);
    ensure_rowptr(m.get(), nullptr);
    BMSP_HIP(hipStreamSynchronize(nullptr));
    *out = m.release();
    BMSP_API_END
}

int bmsp_matrix_free(bmsp_matrix_t m)
{
    BMSP_API_BEGIN
    free_matrix(m);
    BMSP_API_END
}

int bmsp_matrix_invalidate(bmsp_matrix_t m, int structure_changed)
{
    BMSP_API_BEGIN
    need(m, "matrix");
    invalidate_matrix(m, structure_changed);
    BMSP_API_END
}

int bmsp_matrix_transpose(bmsp_matrix_t A, int out_transposed, void *stream, bmsp_matrix_t *out)
{
    BMSP_API_BEGIN
    check_layout_flag(out_transposed, "out_transposed");
    need(A, "matrix"); need(out, "out");
    load_kernels();
    *out = transpose_matrix(A, out_transposed, true, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_convert_layout(bmsp_matrix_t A, int out_transposed, void *stream, bmsp_matrix_t *out)
{
    BMSP_API_BEGIN
    check_layout_flag(out_transposed, "out_transposed");
    need(A, "matrix"); need(out, "out");
    load_kernels();
    *out = transpose_matrix(A, out_transposed, false, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_copy_values(bmsp_matrix_t A, bmsp_matrix_t out, void *stream)
{
    BMSP_API_BEGIN
    need(A, "matrix"); need(out, "out");
    copy_values_from(A, out, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_add(double alpha, bmsp_matrix_t A, double beta, bmsp_matrix_t B, int out_transposed, void *stream, bmsp_matrix_t *C)
{
    BMSP_API_BEGIN
    check_layout_flag(out_transposed, "out_transposed");
    need(A, "matrix A"); need(B, "matrix B"); need(C, "output C");
    load_kernels();
    *C = add_matrices(alpha, A, beta, B, out_transposed, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_add_values(double alpha, bmsp_matrix_t A, double beta, bmsp_matrix_t B, bmsp_matrix_t C, void *stream)
{
    BMSP_API_BEGIN
    need(A, "matrix A"); need(B, "matrix B"); need(C, "matrix C");
    add_values(alpha, A, beta, B, C, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_prune(bmsp_matrix_t A, int rule, double tol, int flags, int out_transposed, void *stream, bmsp_matrix_t *out,
                      bmsp_prune_stats *stats)
{
    BMSP_API_BEGIN
    prune_check_args(rule, tol, flags, out_transposed);
    if (!out && !stats) fail(BMSP_ERR_INVALID, "out and stats are both null");
    need(A, "matrix A");
    load_kernels();
    prune_matrix(A, rule, tol, flags, out_transposed, as_stream(stream), out, stats);
    BMSP_API_END
}

int bmsp_matrix_row_absmax(bmsp_matrix_t A, void *d_rowmax, void *stream)
{
    BMSP_API_BEGIN
    need(A, "matrix A"); need(d_rowmax, "d_rowmax");
    load_kernels();
    row_absmax(A, d_rowmax, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_select_band(bmsp_matrix_t A, int64_t lo, int64_t hi, int flags, int out_transposed, void *stream, bmsp_matrix_t *out,
                            bmsp_select_stats *stats)
{
    BMSP_API_BEGIN
    select_check_args(flags, out_transposed, out, stats);
    need(A, "matrix A");
    load_kernels();
    select_band(A, lo, hi, flags, out_transposed, as_stream(stream), out, stats);
    BMSP_API_END
}

int bmsp_matrix_select_mask(bmsp_matrix_t A, bmsp_matrix_t M, int flags, int out_transposed, void *stream, bmsp_matrix_t *out,
                            bmsp_select_stats *stats)
{
    BMSP_API_BEGIN
    select_check_args(flags, out_transposed, out, stats);
    need(A, "matrix A"); need(M, "matrix M");
    load_kernels();
    select_mask(A, M, flags, out_transposed, as_stream(stream), out, stats);
    BMSP_API_END
}

int bmsp_matrix_diagonal(bmsp_matrix_t A, void *d_diag, void *stream)
{
    BMSP_API_BEGIN
    need(A, "matrix A"); need(d_diag, "d_diag");
    load_kernels();
    matrix_diagonal(A, d_diag, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_from_diagonal(int num_rows, int num_cols, const void *d_diag, bmsp_dtype dtype, int transposed, void *stream,
                              bmsp_matrix_t *out)
{
    BMSP_API_BEGIN
    from_diagonal_check_args(num_rows, num_cols, d_diag, dtype, transposed);
    need(out, "out");
    load_kernels();
    *out = matrix_from_diagonal(num_rows, num_cols, d_diag, dtype, transposed, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_scale(bmsp_matrix_t A, const void *d_left, const void *d_right, int flags, int out_transposed, void *stream,
                      bmsp_matrix_t *out)
{
    BMSP_API_BEGIN
    scale_check_args(d_left, d_right, flags, out_transposed);
    need(A, "matrix A"); need(out, "out");
    load_kernels();
    *out = scale_matrix(A, d_left, d_right, flags, out_transposed, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_scale_values(bmsp_matrix_t A, const void *d_left, const void *d_right, int flags, bmsp_matrix_t out, void *stream)
{
    BMSP_API_BEGIN
    scale_check_args(d_left, d_right, flags, 0);
    need(A, "matrix A"); need(out, "matrix out");
    scale_values_into(A, d_left, d_right, flags, out, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_info(bmsp_matrix_t m, int *num_rows, int *num_cols, int64_t *nnz, int64_t *block_num, bmsp_dtype *dtype, int *transposed)
{
    BMSP_API_BEGIN
    need(m, "matrix");
    if (num_rows) *num_rows = m->num_rows;
    if (num_cols) *num_cols = m->num_cols;
    if (nnz) *nnz = m->nnz;
    if (block_num) *block_num = m->block_num;
    if (dtype) *dtype = m->dtype;
    if (transposed) *transposed = m->transposed;
    BMSP_API_END
}

int bmsp_matrix_arrays(bmsp_matrix_t m, uint64_t **d_keys, uint64_t **d_bmps, uint64_t **d_offsets, void **d_values)
{
    BMSP_API_BEGIN
    need(m, "matrix");
    if (d_keys) *d_keys = m->keys;
    if (d_bmps) *d_bmps = m->bmps;
    if (d_offsets) *d_offsets = m->offsets;
    if (d_values) *d_values = m->values;
    BMSP_API_END
}

int bmsp_matrix_block_row_ptr(bmsp_matrix_t m, const uint32_t **d_rowptr, int64_t *num_block_rows)
{
    BMSP_API_BEGIN
    need(m, "matrix");
    ensure_rowptr(m, nullptr);
    BMSP_HIP(hipStreamSynchronize(nullptr));
    if (d_rowptr) *d_rowptr = m->rowptr;
    if (num_block_rows) *num_block_rows = m->num_block_rows();
    BMSP_API_END
}

int bmsp_matrix_prepare(bmsp_matrix_t m, int what, void *stream)
{
    BMSP_API_BEGIN
    need(m, "matrix");
    if (what & ~(BMSP_PREPARE_SPMV | BMSP_PREPARE_SPGEMM)) fail(BMSP_ERR_INVALID, "unknown prepare flags %d", what);
    ensure_rowptr(m, as_stream(stream));
    if (what & BMSP_PREPARE_SPMV) prepare_spmv(m, as_stream(stream));
    if (what & BMSP_PREPARE_SPGEMM) prepare_spgemm_operand(m, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_to_coo_host(bmsp_matrix_t m, int *rows, int *cols, double *vals)
{
    BMSP_API_BEGIN
    need(m, "matrix");
    if (m->nnz) { need(rows, "rows"); need(cols, "cols"); need(vals, "vals"); }
    matrix_to_coo_host(m, rows, cols, vals, nullptr);
    BMSP_API_END
}

int bmsp_matrix_to_coo_device(bmsp_matrix_t m, int *d_rows, int *d_cols, double *d_vals, void *stream)
{
    BMSP_API_BEGIN
    need(m, "matrix");
    if (m->nnz) { need(d_rows, "rows"); need(d_cols, "cols"); need(d_vals, "vals"); }
    matrix_to_coo_device_split(m, d_rows, d_cols, d_vals, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_to_csr_device(bmsp_matrix_t m, int *d_row_offsets, int *d_cols, double *d_vals, void *stream)
{
    BMSP_API_BEGIN
    need(m, "matrix"); need(d_row_offsets, "row_offsets");
    if (m->nnz) { need(d_cols, "cols"); need(d_vals, "vals"); }
    matrix_to_csr_device(m, d_row_offsets, d_cols, d_vals, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_from_csr_device(int num_rows, int num_cols, int64_t nnz, const int *d_row_offsets, const int *d_cols, const double *d_vals,
                                int transposed, bmsp_dtype dtype, void *stream, bmsp_matrix_t *out)
{
    BMSP_API_BEGIN
    load_kernels();
    need(out, "out"); need(d_row_offsets, "row_offsets");
    if (num_rows < 0 || num_cols < 0 || nnz < 0) fail(BMSP_ERR_INVALID, "negative size");
    if (nnz) { need(d_cols, "cols"); need(d_vals, "vals"); }
    *out = build_from_device_csr(num_rows, num_cols, nnz, d_row_offsets, d_cols, d_vals, transposed, dtype, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_compare_device(bmsp_matrix_t m, int64_t nnz, const int *d_rows, const int *d_cols, const double *d_vals, double *mean_rel_err,
                               int64_t *missing, void *stream)
{
    BMSP_API_BEGIN
    need(m, "matrix"); need(mean_rel_err, "mean_rel_err");
    if (nnz < 0) fail(BMSP_ERR_INVALID, "negative size");
    if (nnz) { need(d_rows, "rows"); need(d_cols, "cols"); need(d_vals, "vals"); }
    matrix_compare_device(m, nnz, d_rows, d_cols, d_vals, mean_rel_err, missing, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_compare(bmsp_matrix_t m, int64_t nnz, const int *rows, const int *cols, const double *vals, double *mean_rel_err,
                        int64_t *missing)
{
    BMSP_API_BEGIN
    need(m, "matrix");
    need(mean_rel_err, "mean_rel_err");
    size_t n = (size_t)m->nnz;
    std::vector<int> mr(n), mc(n);
    std::vector<double> mv(n);
    matrix_to_coo_host(m, mr.data(), mc.data(), mv.data(), nullptr);
    // comparand sorted by (row, col) (src/bmSpMatrix.cu:394)
    std::vector<int64_t> perm((size_t)nnz);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) {
        return rows[a] != rows[b] ? rows[a] < rows[b] : cols[a] < cols[b];
    });
    const double eps = 1e-8;  // :403
    double count = 0;
    int64_t miss = 0;
    size_t j = 0;
    for (size_t i = 0; i < n; i++) {
        // skip comparand entries that m does not hold (:405-408)
        while (j < (size_t)nnz && (rows[perm[j]] < mr[i] || (rows[perm[j]] == mr[i] && cols[perm[j]] < mc[i]))) j++;
        if (j >= (size_t)nnz || rows[perm[j]] != mr[i] || cols[perm[j]] != mc[i]) { miss++; continue; }
        double e = std::fabs(vals[perm[j]]) < eps ? 0.0 : vals[perm[j]];
        double r = std::fabs(mv[i]) < eps ? 0.0 : mv[i];
        count += std::fabs(e - r) / std::max(std::fabs(e), eps);  // :418
        j++;
    }
    *mean_rel_err = n ? count / (double)n : 0.0;  // "Final:" (:429)
    if (missing) *missing = miss;
    BMSP_API_END
}

int bmsp_spmv(bmsp_matrix_t A, const void *d_v, void *d_u, int variant, void *stream)
{
    BMSP_API_BEGIN
    need(A, "A");
    spmv(A, d_v, d_u, variant, as_stream(stream));
    BMSP_API_END
}

int bmsp_spmv_launch_info(bmsp_matrix_t A, int variant, char *kernel_name, size_t kernel_name_cap, int64_t *compulsory_bytes, int64_t *format_bytes)
{
    BMSP_API_BEGIN
    need(A, "A");
    spmv_launch_info(A, variant, nullptr, kernel_name, kernel_name_cap, compulsory_bytes, format_bytes);
    BMSP_API_END
}

int bmsp_spmv_chunk_layout(bmsp_matrix_t A, int *layout)
{
    BMSP_API_BEGIN
    need(A, "A"); need(layout, "layout");
    *layout = spmv_chunk_layout(A, nullptr);
    BMSP_API_END
}

int bmsp_spmv_op(bmsp_matrix_t A, int op, double alpha, const void *d_v, double beta, void *d_u, void *stream)
{
    BMSP_API_BEGIN
    spmv_op_check_op(op);
    need(A, "matrix A"); need(d_v, "d_v"); need(d_u, "d_u");
    load_kernels();
    spmv_op(A, op, alpha, d_v, beta, d_u, as_stream(stream));
    BMSP_API_END
}

int bmsp_spmv_op_launch_info(bmsp_matrix_t A, int op, bmsp_spmv_op_info *info)
{
    BMSP_API_BEGIN
    spmv_op_check_op(op);
    need(A, "matrix A"); need(info, "info");
    load_kernels();
    spmv_op_launch_info(A, op, nullptr, info);
    BMSP_API_END
}

int bmsp_spmv_op_plan_items(const uint32_t *ptr, int64_t blocks, int64_t split, uint32_t *items, uint32_t *folds, int64_t *n_items,
                            int64_t *split_blocks, int64_t *slots)
{
    BMSP_API_BEGIN
    spmv_op_plan_items(ptr, blocks, split, items, folds, n_items, split_blocks, slots);
    BMSP_API_END
}

int bmsp_spmm_op(bmsp_matrix_t A, int op, double alpha, const void *d_X, int64_t ldx, double beta, void *d_Y, int64_t ldy, int k, void *stream)
{
    BMSP_API_BEGIN
    spmm_op_check_args(op, k, ldx, ldy);
    need(A, "matrix A"); need(d_X, "d_X"); need(d_Y, "d_Y");
    load_kernels();
    spmm_op(A, op, alpha, d_X, ldx, beta, d_Y, ldy, k, as_stream(stream));
    BMSP_API_END
}

int bmsp_spmm_op_launch_info(bmsp_matrix_t A, int op, int k, int64_t ldx, int64_t ldy, bmsp_spmm_op_info *info)
{
    BMSP_API_BEGIN
    spmm_op_check_args(op, k, ldx, ldy);
    need(A, "matrix A"); need(info, "info");
    load_kernels();
    spmm_op_launch_info(A, op, k, ldx, ldy, nullptr, info);
    BMSP_API_END
}

int bmsp_sddmm(bmsp_matrix_t S, const void *d_X, int64_t ldx, const void *d_Y, int64_t ldy, int k, double alpha, double beta, int flags,
               int out_transposed, void *stream, bmsp_matrix_t *out)
{
    BMSP_API_BEGIN
    sddmm_check_args(k, ldx, ldy, beta, flags, out_transposed);
    need(S, "matrix S"); need(d_X, "d_X"); need(d_Y, "d_Y"); need(out, "out");
    load_kernels();
    *out = sddmm_matrix(S, d_X, ldx, d_Y, ldy, k, alpha, beta, flags, out_transposed, as_stream(stream));
    BMSP_API_END
}

int bmsp_sddmm_values(bmsp_matrix_t S, const void *d_X, int64_t ldx, const void *d_Y, int64_t ldy, int k, double alpha, double beta, int flags,
                      bmsp_matrix_t out, void *stream)
{
    BMSP_API_BEGIN
    sddmm_check_args(k, ldx, ldy, beta, flags, 0);
    need(S, "matrix S"); need(d_X, "d_X"); need(d_Y, "d_Y"); need(out, "matrix out");
    load_kernels();
    sddmm_values_into(S, d_X, ldx, d_Y, ldy, k, alpha, beta, flags, out, as_stream(stream));
    BMSP_API_END
}

int bmsp_sddmm_launch_info(bmsp_matrix_t S, int k, int64_t ldx, int64_t ldy, int out_transposed, bmsp_sddmm_info *info)
{
    BMSP_API_BEGIN
    sddmm_check_args(k, ldx, ldy, 0.0, 0, out_transposed);
    need(S, "matrix S"); need(info, "info");
    sddmm_launch_info(S, k, ldx, ldy, out_transposed, info);
    BMSP_API_END
}

int bmsp_spgemm_masked(bmsp_matrix_t A, bmsp_matrix_t B, bmsp_matrix_t M, double alpha, double beta, int flags, int out_transposed, void *stream,
                       bmsp_matrix_t *out)
{
    BMSP_API_BEGIN
    spgemm_masked_check_args(beta, flags, out_transposed);
    need(A, "matrix A"); need(B, "matrix B"); need(M, "matrix M"); need(out, "out");
    spgemm_masked_check_matrices(A, B, M, nullptr);
    load_kernels();
    *out = spgemm_masked_matrix(A, B, M, alpha, beta, flags, out_transposed, as_stream(stream));
    BMSP_API_END
}

int bmsp_spgemm_masked_values(bmsp_matrix_t A, bmsp_matrix_t B, bmsp_matrix_t M, double alpha, double beta, int flags, bmsp_matrix_t out,
                              void *stream)
{
    BMSP_API_BEGIN
    spgemm_masked_check_args(beta, flags, 0);
    need(A, "matrix A"); need(B, "matrix B"); need(M, "matrix M"); need(out, "matrix out");
    spgemm_masked_check_matrices(A, B, M, out);
    load_kernels();
    spgemm_masked_values_into(A, B, M, alpha, beta, flags, out, as_stream(stream));
    BMSP_API_END
}

int bmsp_spgemm_masked_launch_info(bmsp_matrix_t A, bmsp_matrix_t B, bmsp_matrix_t M, int out_transposed, bmsp_spgemm_masked_info *info)
{
    BMSP_API_BEGIN
    spgemm_masked_check_args(0.0, 0, out_transposed);
    need(A, "matrix A"); need(B, "matrix B"); need(M, "matrix M"); need(info, "info");
    spgemm_masked_check_matrices(A, B, M, nullptr);
    load_kernels();
    spgemm_masked_launch_info(A, B, M, out_transposed, info);
    BMSP_API_END
}

int bmsp_spsv_analyse(bmsp_matrix_t A, int op, int fill, int diag, void *stream, bmsp_spsv_info *info)
{
    BMSP_API_BEGIN
    spsv_check_args(op, fill, diag);
    need(A, "matrix A");
    spsv_check_matrix(A);
    load_kernels();
    spsv_analyse(A, op, fill, diag, as_stream(stream), info);
    BMSP_API_END
}

int bmsp_spsv(bmsp_matrix_t A, int op, int fill, int diag, double alpha, const void *d_b, void *d_x, void *stream)
{
    BMSP_API_BEGIN
    spsv_check_args(op, fill, diag);
    need(A, "matrix A"); need(d_b, "d_b"); need(d_x, "d_x");
    spsv_check_matrix(A);
    load_kernels();
    spsv(A, op, fill, diag, alpha, d_b, d_x, as_stream(stream));
    BMSP_API_END
}

int bmsp_spitsv(bmsp_matrix_t A, int op, int fill, int diag, double alpha, const void *d_b, void *d_x, int64_t max_iter, double tol, int flags,
                double *delta_history, bmsp_spitsv_info *info, void *stream)
{
    BMSP_API_BEGIN
    spitsv_check_args(op, fill, diag, max_iter, tol, flags, delta_history);
    need(A, "matrix A"); need(d_b, "d_b"); need(d_x, "d_x");
    spsv_check_matrix(A);
    spitsv_check_vectors(d_b, d_x);
    load_kernels();
    spitsv(A, op, fill, diag, alpha, d_b, d_x, max_iter, tol, flags, delta_history, info, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_ilu0(bmsp_matrix_t A, int64_t max_iter, double tol, int out_transposed, void *stream, bmsp_matrix_t *F, double *delta_history,
                     bmsp_ilu0_info *info)
{
    BMSP_API_BEGIN
    ilu0_check_args(max_iter, tol, delta_history);
    check_layout_flag(out_transposed, "out_transposed");
    need(A, "matrix A"); need(F, "F");
    ilu0_check_matrices(A, nullptr);
    load_kernels();
    *F = ilu0_matrix(A, max_iter, tol, out_transposed, as_stream(stream), delta_history, info);
    BMSP_API_END
}

int bmsp_matrix_ilu0_values(bmsp_matrix_t A, bmsp_matrix_t F, int64_t max_iter, double tol, int flags, void *stream, double *delta_history,
                            bmsp_ilu0_info *info)
{
    BMSP_API_BEGIN
    ilu0_check_args(max_iter, tol, delta_history);
    ilu0_check_flags(flags);
    need(A, "matrix A"); need(F, "matrix F");
    ilu0_check_matrices(A, F);
    load_kernels();
    ilu0_values_into(A, F, max_iter, tol, flags, as_stream(stream), delta_history, info);
    BMSP_API_END
}

int bmsp_vec_dot(int64_t n, int vec_f64, const void *d_x, const void *d_y, double *d_result, void *stream)
{
    BMSP_API_BEGIN
    vec_check_args(n, vec_f64);
    need(d_result, "d_result");
    load_kernels();
    vec_dot(n, vec_f64, d_x, d_y, d_result, as_stream(stream));
    BMSP_API_END
}

int bmsp_vec_axpby(int64_t n, int vec_f64, double a, const void *d_x, double b, void *d_y, void *stream)
{
    BMSP_API_BEGIN
    vec_check_args(n, vec_f64);
    load_kernels();
    vec_axpby(n, vec_f64, a, d_x, b, d_y, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_color_blocks(bmsp_matrix_t A, uint64_t seed, uint32_t *d_colors, uint32_t *d_perm, void *stream, bmsp_color_info *info)
{
    BMSP_API_BEGIN
    need(A, "matrix A"); need(d_colors, "d_colors");
    color_check_matrix(A);
    load_kernels();
    color_blocks(A, seed, d_colors, d_perm, as_stream(stream), info);
    BMSP_API_END
}

int bmsp_matrix_permute_blocks(bmsp_matrix_t A, const uint32_t *d_row_perm, const uint32_t *d_col_perm, int out_transposed, void *stream,
                               bmsp_matrix_t *out)
{
    BMSP_API_BEGIN
    check_layout_flag(out_transposed, "out_transposed");
    need(A, "matrix A"); need(out, "out");
    permute_check_matrix(A);
    load_kernels();
    *out = permute_blocks(A, d_row_perm, d_col_perm, out_transposed, as_stream(stream));
    BMSP_API_END
}

int bmsp_vec_permute_blocks(int64_t n, int vec_f64, const uint32_t *d_perm, int inverse, const void *d_x, void *d_y, void *stream)
{
    BMSP_API_BEGIN
    vec_permute_check_args(n, vec_f64, d_perm, inverse, d_x, d_y);
    load_kernels();
    vec_permute_blocks(n, vec_f64, d_perm, inverse, d_x, d_y, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_aggregate(bmsp_matrix_t S, uint64_t seed, uint32_t *d_agg, int64_t *num_aggregates, void *stream, bmsp_aggregate_info *info)
{
    BMSP_API_BEGIN
    need(S, "matrix S"); need(d_agg, "d_agg"); need(num_aggregates, "num_aggregates");
    aggregate_check_matrix(S);
    load_kernels();
    aggregate(S, seed, d_agg, num_aggregates, as_stream(stream), info);
    BMSP_API_END
}

int bmsp_matrix_from_aggregates(int num_rows, int num_aggregates, const uint32_t *d_agg, const void *d_weights, bmsp_dtype dtype,
                                int transposed, void *stream, bmsp_matrix_t *out)
{
    BMSP_API_BEGIN
    from_aggregates_check_args(num_rows, num_aggregates, d_agg, dtype, transposed);
    need(out, "out");
    load_kernels();
    *out = matrix_from_aggregates(num_rows, num_aggregates, d_agg, d_weights, dtype, transposed, as_stream(stream));
    BMSP_API_END
}

int bmsp_krylov_solve(bmsp_matrix_t A, int op, int method, const bmsp_precond *pc, const void *d_b, void *d_x, int64_t max_iter, double tol,
                      int flags, double *relres_history, bmsp_krylov_info *info, void *stream)
{
    BMSP_API_BEGIN
    krylov_check_args(op, method, pc, max_iter, tol, flags, relres_history);
    need_solve_operands(A, "matrix A", d_b, d_x);
    krylov_check_operands(A, pc);
    load_kernels();
    krylov_solve(A, op, method, SolvePc{pc}, d_b, d_x, max_iter, tol, flags, relres_history, info, as_stream(stream));
    BMSP_API_END
}

int bmsp_gmres_solve(bmsp_matrix_t A, int op, const bmsp_precond *pc, int restart, const void *d_b, void *d_x, int64_t max_iter, double tol,
                     int flags, double *relres_history, bmsp_krylov_info *info, void *stream)
{
    BMSP_API_BEGIN
    gmres_check_args(op, restart, pc, max_iter, tol, flags, relres_history);
    need_solve_operands(A, "matrix A", d_b, d_x);
    krylov_check_operands(A, pc);
    load_kernels();
    gmres_solve(A, op, SolvePc{pc}, restart, d_b, d_x, max_iter, tol, flags, relres_history, info, as_stream(stream));
    BMSP_API_END
}

int bmsp_mg_create(int levels, const bmsp_matrix_t *A, const bmsp_matrix_t *P, const bmsp_matrix_t *R, const void *d_coarse_inv, int64_t ld_inv,
                   double omega, int pre, int post, void *stream, bmsp_mg_t *out)
{
    BMSP_API_BEGIN
    mg_check_args(levels, omega, pre, post, d_coarse_inv);
    need(out, "out"); need(A, "A");
    if (levels > 1) need(P, "P");
    for (int l = 0; l < levels; l++) {
        if (!A[l]) fail(BMSP_ERR_INVALID, "A[%d] is null", l);
        if (l + 1 < levels && !P[l]) fail(BMSP_ERR_INVALID, "P[%d] is null", l);
    }
    mg_check_operands(levels, A, P, R, d_coarse_inv, ld_inv);
    load_kernels();
    *out = mg_create(levels, A, P, R, d_coarse_inv, ld_inv, omega, pre, post, as_stream(stream));
    BMSP_API_END
}

int bmsp_mg_free(bmsp_mg_t mg)
{
    BMSP_API_BEGIN
    mg_free(mg);
    BMSP_API_END
}

int bmsp_mg_info(bmsp_mg_t mg, bmsp_mg_info_t *info)
{
    BMSP_API_BEGIN
    need(mg, "mg"); need(info, "info");
    mg_info(mg, info);
    BMSP_API_END
}

int bmsp_mg_vcycle(bmsp_mg_t mg, const void *d_r, void *d_z, void *stream)
{
    BMSP_API_BEGIN
    need(mg, "mg"); need(d_r, "d_r"); need(d_z, "d_z");
    if (d_r == d_z) fail(BMSP_ERR_INVALID, "d_z must not be d_r: r is read after z has been written");
    load_kernels();
    mg_vcycle(mg, d_r, d_z, nullptr, as_stream(stream));
    BMSP_API_END
}

int bmsp_mg_solve(bmsp_mg_t mg, int method, const void *d_b, void *d_x, int64_t max_iter, double tol, int flags, double *relres_history,
                  bmsp_krylov_info *info, void *stream)
{
    BMSP_API_BEGIN
    krylov_check_args(BMSP_OP_N, method, nullptr, max_iter, tol, flags, relres_history);
    need_solve_operands(mg, "mg", d_b, d_x);
    load_kernels();
    bmsp_matrix_s *A = nullptr;
    const SolvePc pc = mg_solve_pc(mg, as_stream(stream), &A);
    krylov_solve(A, BMSP_OP_N, method, pc, d_b, d_x, max_iter, tol, flags, relres_history, info, as_stream(stream));
    BMSP_API_END
}

int bmsp_mg_solve_gmres(bmsp_mg_t mg, int restart, const void *d_b, void *d_x, int64_t max_iter, double tol, int flags,
                        double *relres_history, bmsp_krylov_info *info, void *stream)
{
    BMSP_API_BEGIN
    gmres_check_args(BMSP_OP_N, restart, nullptr, max_iter, tol, flags, relres_history);
    need_solve_operands(mg, "mg", d_b, d_x);
    load_kernels();
    bmsp_matrix_s *A = nullptr;
    const SolvePc pc = mg_solve_pc(mg, as_stream(stream), &A);
    gmres_solve(A, BMSP_OP_N, pc, restart, d_b, d_x, max_iter, tol, flags, relres_history, info, as_stream(stream));
    BMSP_API_END
}

int bmsp_matrix_fsai(bmsp_matrix_t A, int op, bmsp_matrix_t S, int scale, int out_transposed, void *d_pivot, void *stream, bmsp_matrix_t *out,
                     bmsp_fsai_info *info)
{
    BMSP_API_BEGIN
    fsai_check_args(op, scale, out_transposed);
    need(A, "matrix A"); need(S, "matrix S"); need(out, "out"); need(info, "info");
    fsai_check_matrices(A, S, "S");
    load_kernels();
    bmsp_matrix_s *G = fsai_matrix(A, op, S, scale, out_transposed, d_pivot, as_stream(stream), info);
    *out = G;
    BMSP_API_END
}

int bmsp_matrix_fsai_values(bmsp_matrix_t A, int op, bmsp_matrix_t G, int scale, void *d_pivot, void *stream, bmsp_fsai_info *info)
{
    BMSP_API_BEGIN
    fsai_check_args(op, scale, 0);
    need(A, "matrix A"); need(G, "matrix G"); need(info, "info");
    fsai_check_matrices(A, G, "G");
    load_kernels();
    fsai_values_into(A, op, G, scale, d_pivot, as_stream(stream), info);
    BMSP_API_END
}

int bmsp_fsai_create(bmsp_matrix_t A, bmsp_matrix_t S, int kind, int flags, void *stream, bmsp_fsai_t *out)
{
    BMSP_API_BEGIN
    fsai_create_check_args(kind, flags);
    need(A, "matrix A"); need(S, "matrix S"); need(out, "out");
    fsai_check_matrices(A, S, "S");
    load_kernels();
    bmsp_fsai_s *f = fsai_create(A, S, kind, flags, as_stream(stream));
    *out = f;
    BMSP_API_END
}

int bmsp_fsai_update(bmsp_fsai_t f, void *stream)
{
    BMSP_API_BEGIN
    need(f, "f");
    load_kernels();
    fsai_update(f, as_stream(stream));
    BMSP_API_END
}

int bmsp_fsai_free(bmsp_fsai_t f)
{
    BMSP_API_BEGIN
    fsai_free(f);
    BMSP_API_END
}

int bmsp_fsai_get_info(bmsp_fsai_t f, bmsp_fsai_handle_info *info)
{
    BMSP_API_BEGIN
    need(f, "f"); need(info, "info");
    fsai_get_info(f, info);
    BMSP_API_END
}

int bmsp_fsai_factors(bmsp_fsai_t f, bmsp_matrix_t *G1, bmsp_matrix_t *G2)
{
    BMSP_API_BEGIN
    need(f, "f");
    fsai_factors(f, G1, G2);
    BMSP_API_END
}

int bmsp_fsai_apply(bmsp_fsai_t f, const void *d_r, void *d_z, void *stream)
{
    BMSP_API_BEGIN
    need(f, "f"); need(d_r, "d_r"); need(d_z, "d_z");
    if (d_r == d_z) fail(BMSP_ERR_INVALID, "d_z must not be d_r");
    load_kernels();
    fsai_apply(f, d_r, d_z, as_stream(stream));
    BMSP_API_END
}

int bmsp_fsai_solve(bmsp_fsai_t f, int method, const void *d_b, void *d_x, int64_t max_iter, double tol, int flags, double *relres_history,
                    bmsp_krylov_info *info, void *stream)
{
    BMSP_API_BEGIN
    krylov_check_args(BMSP_OP_N, method, nullptr, max_iter, tol, flags, relres_history);
    need_solve_operands(f, "f", d_b, d_x);
    load_kernels();
    bmsp_matrix_s *A = nullptr;
    const SolvePc pc = fsai_solve_pc(f, as_stream(stream), &A);
    krylov_solve(A, BMSP_OP_N, method, pc, d_b, d_x, max_iter, tol, flags, relres_history, info, as_stream(stream));
    BMSP_API_END
}

int bmsp_fsai_solve_gmres(bmsp_fsai_t f, int restart, const void *d_b, void *d_x, int64_t max_iter, double tol, int flags,
                          double *relres_history, bmsp_krylov_info *info, void *stream)
{
    BMSP_API_BEGIN
    gmres_check_args(BMSP_OP_N, restart, nullptr, max_iter, tol, flags, relres_history);
    need_solve_operands(f, "f", d_b, d_x);
    load_kernels();
    bmsp_matrix_s *A = nullptr;
    const SolvePc pc = fsai_solve_pc(f, as_stream(stream), &A);
    gmres_solve(A, BMSP_OP_N, pc, restart, d_b, d_x, max_iter, tol, flags, relres_history, info, as_stream(stream));
    BMSP_API_END
}

int bmsp_spsv_plan(const uint32_t *ptr, const uint32_t *other, int64_t blocks, int lower, int64_t chain, uint32_t *level_of, uint32_t *order,
                   uint32_t *level_ptr, uint32_t *segments, int64_t *n_levels, int64_t *n_segments)
{
    BMSP_API_BEGIN
    spsv_plan(ptr, other, blocks, lower, chain, level_of, order, level_ptr, segments, n_levels, n_segments);
    BMSP_API_END
}

int bmsp_spsm(bmsp_matrix_t A, int op, int fill, int diag, double alpha, const void *d_B, int64_t ldb, void *d_X, int64_t ldx, int k, void *stream)
{
    BMSP_API_BEGIN
    spsm_check_args(op, fill, diag, k, ldb, ldx);
    need(A, "matrix A"); need(d_B, "d_B"); need(d_X, "d_X");
    spsv_check_matrix(A);
    spsm_check_in_place(d_B, ldb, d_X, ldx);
    load_kernels();
    spsm(A, op, fill, diag, alpha, d_B, ldb, d_X, ldx, k, as_stream(stream));
    BMSP_API_END
}

int bmsp_spsm_launch_info(bmsp_matrix_t A, int op, int fill, int diag, int k, int64_t ldb, int64_t ldx, void *stream, bmsp_spsm_info *info)
{
    BMSP_API_BEGIN
    spsm_check_args(op, fill, diag, k, ldb, ldx);
    need(A, "matrix A"); need(info, "info");
    spsv_check_matrix(A);
    load_kernels();
    spsm_launch_info(A, op, fill, diag, k, ldb, ldx, as_stream(stream), info);
    BMSP_API_END
}

int bmsp_comm_unique_id(void *id_bytes)
{
    BMSP_API_BEGIN
    need(id_bytes, "id_bytes");
    comm_unique_id(id_bytes);
    BMSP_API_END
}

int bmsp_comm_init(const void *id_bytes, int world, int rank, bmsp_comm_t *out)
{
    BMSP_API_BEGIN
    need(id_bytes, "id_bytes"); need(out, "out");
    *out = comm_init(id_bytes, world, rank);
    BMSP_API_END
}

int bmsp_comm_init_loopback(int world, bmsp_comm_t *out)
{
    BMSP_API_BEGIN
    need(out, "out");
    *out = comm_init_loopback(world);
    BMSP_API_END
}

int bmsp_shard_layout(int parts, const int64_t *block_nums, const int64_t *nnzs, int64_t *block_start, int64_t *value_start)
{
    BMSP_API_BEGIN
    need(block_nums, "block_nums"); need(nnzs, "nnzs"); need(block_start, "block_start"); need(value_start, "value_start");
    shard_layout(parts, block_nums, nnzs, block_start, value_start);
    BMSP_API_END
}

int bmsp_shard_row_slices(int num_rows, int parts, const int64_t *bounds, int64_t *row_start, int64_t *row_count)
{
    BMSP_API_BEGIN
    need(bounds, "bounds"); need(row_start, "row_start"); need(row_count, "row_count");
    shard_row_slices(num_rows, parts, bounds, row_start, row_count);
    BMSP_API_END
}

int bmsp_comm_init_from_env(bmsp_comm_t *out)
{
    BMSP_API_BEGIN
    need(out, "out");
    *out = comm_init_from_env();
    BMSP_API_END
}

int bmsp_comm_info(bmsp_comm_t c, int *rank, int *world)
{
    BMSP_API_BEGIN
    need(c, "comm");
    if (rank) *rank = c->rank;
    if (world) *world = c->world;
    BMSP_API_END
}

int bmsp_comm_free(bmsp_comm_t c)
{
    BMSP_API_BEGIN
    comm_free(c);
    BMSP_API_END
}

int bmsp_spgemm_sharded(bmsp_comm_t c, bmsp_matrix_t A, bmsp_matrix_t B, bmsp_matrix_t *C, int mode, int tc_version, int verbose, void *stream,
                        bmsp_spgemm_stats *stats, bmsp_shard_stats *shard)
{
    BMSP_API_BEGIN
    need(c, "comm"); need(A, "A"); need(B, "B"); need(C, "C");
    spgemm_sharded(c, A, B, C, mode, tc_version, verbose, as_stream(stream), stats, shard);
    BMSP_API_END
}

int bmsp_spgemm_sharded_ex(bmsp_comm_t c, bmsp_matrix_t A, bmsp_matrix_t B, bmsp_matrix_t *C, int mode, int tc_version, int verbose, void *stream,
                           bmsp_spgemm_stats *stats, bmsp_shard_stats *shard, int gather, int rounds)
{
    BMSP_API_BEGIN
    need(c, "comm"); need(A, "A"); need(B, "B"); need(C, "C");
    spgemm_sharded(c, A, B, C, mode, tc_version, verbose, as_stream(stream), stats, shard, gather ? 1 : 0, rounds);
    BMSP_API_END
}

int bmsp_spmv_sharded(bmsp_comm_t c, bmsp_matrix_t A, const void *d_v, void *d_u, int variant, void *stream, bmsp_shard_stats *shard)
{
    BMSP_API_BEGIN
    need(c, "comm"); need(A, "A");
    spmv_sharded(c, A, d_v, d_u, variant, as_stream(stream), shard);
    BMSP_API_END
}

int bmsp_selftest_mfma_layout(int *mismatches)
{
    BMSP_API_BEGIN
    need(mismatches, "mismatches");
    *mismatches = mfma32_selftest(nullptr);
    BMSP_API_END
}

int bmsp_selftest_mfma_f32_cancel(int *mismatches, int *exp_floor)
{
    BMSP_API_BEGIN
    need(mismatches, "mismatches");
    *mismatches = mfma_f32_selftest(nullptr, true);
    if (exp_floor) *exp_floor = mac_f32_exp_floor(nullptr);
    BMSP_API_END
}

int bmsp_selftest_tile_product(int *mismatches)
{
    BMSP_API_BEGIN
    need(mismatches, "mismatches");
    *mismatches = tile_product_selftest(nullptr);
    BMSP_API_END
}

int bmsp_selftest_mfma_f32_chain(int *mismatches)
{
    BMSP_API_BEGIN
    need(mismatches, "mismatches");
    *mismatches = mfma_f32_selftest(nullptr);
    BMSP_API_END
}

int bmsp_spmm(bmsp_matrix_t A, const void *d_X, int64_t ldx, void *d_Y, int64_t ldy, int k, void *stream)
{
    BMSP_API_BEGIN
    need(A, "A");
    if (A->num_cols) need(d_X, "X");
    if (A->num_rows) need(d_Y, "Y");
    spmm(A, d_X, ldx, d_Y, ldy, k, as_stream(stream));
    BMSP_API_END
}

int bmsp_spmm_launch_info(bmsp_matrix_t A, int k, int64_t ldx, int64_t ldy, char *kernel_name, size_t kernel_name_cap)
{
    BMSP_API_BEGIN
    need(A, "A");
    spmm_launch_info(A, k, ldx, ldy, nullptr, kernel_name, kernel_name_cap);
    BMSP_API_END
}

int bmsp_spgemm(bmsp_matrix_t A, bmsp_matrix_t B, bmsp_matrix_t *C, int mode, int tc_version, int verbose, void *stream,
                bmsp_spgemm_stats *stats)
{
    BMSP_API_BEGIN
    try {
        if (getenv("BMSP_SPGEMM_FORCE_PANELS")) throw TaskRangeExceeded(BMSP_ERR_LIMIT, "forced (test hook for the paneled path)");
        spgemm(A, B, C, mode, tc_version, verbose, as_stream(stream), stats);
    } catch (const TaskRangeExceeded &) {
        // more candidate block pairs than one task list can index: the same product, block-row panel after panel
        spgemm_paneled(A, B, C, mode, tc_version, verbose, as_stream(stream), stats);
    }
    BMSP_API_END
}

int bmsp_spgemm_symbolic(bmsp_matrix_t A, bmsp_matrix_t B, bmsp_matrix_t *C, int mode, int tc_version, void *stream, bmsp_spgemm_stats *stats)
{
    BMSP_API_BEGIN
    spgemm(A, B, C, mode, tc_version, 0, as_stream(stream), stats, true);
    BMSP_API_END
}

int bmsp_spgemm_numeric(bmsp_matrix_t A, bmsp_matrix_t B, bmsp_matrix_t C, int tc_version, void *stream, bmsp_spgemm_stats *stats)
{
    BMSP_API_BEGIN
    spgemm_numeric(A, B, C, tc_version, as_stream(stream), stats);
    BMSP_API_END
}

int bmsp_segsort_u64(uint64_t *d_keys, void *d_vals, int val_bytes, int64_t n, const int *d_segs, int64_t num_segs, void *stream)
{
    BMSP_API_BEGIN
    segsort_u64(d_keys, d_vals, val_bytes, n, d_segs, num_segs, as_stream(stream));
    BMSP_API_END
}

int bmsp_partition_rows(bmsp_matrix_t A, bmsp_matrix_t B, int parts, int64_t *bounds)
{
    BMSP_API_BEGIN
    need(A, "A"); need(B, "B"); need(bounds, "bounds");
    partition_rows(A, B, parts, bounds, nullptr);
    BMSP_API_END
}

int bmsp_matrix_row_panel(bmsp_matrix_t m, int64_t brow_begin, int64_t brow_end, bmsp_matrix_t *view)
{
    BMSP_API_BEGIN
    need(m, "matrix"); need(view, "view");
    *view = row_panel(m, brow_begin, brow_end, nullptr);
    BMSP_API_END
}

int bmsp_matrix_concat_panels(int num_rows, int num_cols, int parts, const int64_t *block_nums, const int64_t *nnzs,
                              uint64_t *const *d_keys, uint64_t *const *d_bmps, uint64_t *const *d_offsets, void *const *d_values,
                              bmsp_dtype dtype, bmsp_matrix_t *out)
{
    BMSP_API_BEGIN
    need(out, "out");
    if (parts < 1) fail(BMSP_ERR_INVALID, "parts must be >= 1");
    *out = concat_panels(num_rows, num_cols, parts, block_nums, nnzs, d_keys, d_bmps, d_offsets, d_values, dtype, nullptr);
    BMSP_API_END
}

// ---- host CSR --------------------------------------------------------------------------------------------
// CSRMatrix is a host container in the reference (cusp::csr_matrix<int,float,host_memory>) whose multiply is
// cusp::multiply.  Here the container stays on the host and multiply / spmv run on the GPU through the bmSparse
// operators (CSR -> bmSparse build, product, expansion back to CSR with columns ascending and numeric zeros
// dropped as cusp's host SpGEMM does, csr_spgemm.h:135).

static bmsp_matrix_s *csr_device_form(bmsp_csr_s *m, int transposed)
{
    bmsp_matrix_s *&slot = transposed ? m->dev_transposed : m->dev_normal;
    if (slot) return slot;
    size_t n = m->cols.size();
    std::vector<int> rows(n);
    std::vector<double> vals(n);
    for (int r = 0; r < m->num_rows; r++)
        for (int k = m->row_offsets[r]; k < m->row_offsets[r + 1]; k++) rows[(size_t)k] = r;
    for (size_t i = 0; i < n; i++) vals[i] = (double)m->vals[i];
    slot = build_from_host_coo(m->num_rows, m->num_cols, (int64_t)n, rows.data(), m->cols.data(), vals.data(), transposed, BMSP_F32);
    return slot;
}

int bmsp_csr_from_mtx(const char *path, bmsp_csr_t *out)
{
    BMSP_API_BEGIN
    need(path, "path"); need(out, "out");
    HostCoo coo;
    read_matrix_market(path, coo);
    size_t n = coo.rows.size();
    std::unique_ptr<bmsp_csr_s> m(new bmsp_csr_s());
    m->num_rows = coo.num_rows; m->num_cols = coo.num_cols;
    m->row_offsets.assign((size_t)coo.num_rows + 1, 0);
    m->cols.resize(n); m->vals.resize(n);
    // CUSP's reader sorts by (row, column) (cusp/io/detail/matrix_market.inl:295): stable counting sort by row, then a
    // stable sort by column inside each row
    for (size_t i = 0; i < n; i++) m->row_offsets[(size_t)coo.rows[i] + 1]++;
    for (int r = 0; r < coo.num_rows; r++) m->row_offsets[(size_t)r + 1] += m->row_offsets[(size_t)r];
    {
        std::vector<int> fill(m->row_offsets.begin(), m->row_offsets.end() - 1);
        std::vector<std::pair<int, float>> tmp(n);
        for (size_t i = 0; i < n; i++) tmp[(size_t)fill[(size_t)coo.rows[i]]++] = std::make_pair(coo.cols[i], (float)coo.vals[i]);
        for (int r = 0; r < coo.num_rows; r++)
            std::stable_sort(tmp.begin() + m->row_offsets[(size_t)r], tmp.begin() + m->row_offsets[(size_t)r + 1],
                             [](const std::pair<int, float> &a, const std::pair<int, float> &b) { return a.first < b.first; });
        for (size_t i = 0; i < n; i++) { m->cols[i] = tmp[i].first; m->vals[i] = tmp[i].second; }
    }
    *out = m.release();
    BMSP_API_END
}

int bmsp_csr_from_arrays(int num_rows, int num_cols, int64_t nnz, const int *row_offsets, const int *cols, const float *vals,
                         bmsp_csr_t *out)
{
    BMSP_API_BEGIN
    need(out, "out"); need(row_offsets, "row_offsets");
    if (num_rows < 0 || num_cols < 0 || nnz < 0) fail(BMSP_ERR_INVALID, "negative size");
    if (row_offsets[0] != 0 || row_offsets[num_rows] != nnz) fail(BMSP_ERR_INVALID, "row_offsets do not span [0,nnz]");
    std::unique_ptr<bmsp_csr_s> m(new bmsp_csr_s());
    m->num_rows = num_rows; m->num_cols = num_cols;
    m->row_offsets.assign(row_offsets, row_offsets + num_rows + 1);
    m->cols.assign(cols, cols + nnz);
    m->vals.assign(vals, vals + nnz);
    for (int64_t i = 0; i < nnz; i++)
        if (cols[i] < 0 || cols[i] >= num_cols) fail(BMSP_ERR_INVALID, "column index %d outside [0,%d)", cols[i], num_cols);
    *out = m.release();
    BMSP_API_END
}

int bmsp_csr_info(bmsp_csr_t m, int *num_rows, int *num_cols, int64_t *nnz)
{
    BMSP_API_BEGIN
    need(m, "csr");
    if (num_rows) *num_rows = m->num_rows;
    if (num_cols) *num_cols = m->num_cols;
    if (nnz) *nnz = (int64_t)m->cols.size();
    BMSP_API_END
}

int bmsp_csr_arrays(bmsp_csr_t m, const int **row_offsets, const int **cols, const float **vals)
{
    BMSP_API_BEGIN
    need(m, "csr");
    if (row_offsets) *row_offsets = m->row_offsets.data();
    if (cols) *cols = m->cols.data();
    if (vals) *vals = m->vals.data();
    BMSP_API_END
}

int bmsp_csr_multiply(bmsp_csr_t A, bmsp_csr_t B, bmsp_csr_t *C)
{
    BMSP_API_BEGIN
    need(A, "A"); need(B, "B"); need(C, "C");
    if (A->num_cols != B->num_rows) fail(BMSP_ERR_INVALID, "shape mismatch");
    bmsp_matrix_s *dA = csr_device_form(A, 0), *dB = csr_device_form(B, 1), *dC = nullptr;
    spgemm(dA, dB, &dC, BMSP_SORT_AUTO, 5, 0, nullptr, nullptr);
    auto guard = own_matrix(dC);
    size_t n = (size_t)dC->nnz;
    std::vector<int> r(n), c(n);
    std::vector<double> v(n);
    matrix_to_coo_host(dC, r.data(), c.data(), v.data(), nullptr);
    std::unique_ptr<bmsp_csr_s> m(new bmsp_csr_s());
    m->num_rows = A->num_rows; m->num_cols = B->num_cols;
    m->row_offsets.assign((size_t)A->num_rows + 1, 0);
    for (size_t i = 0; i < n; i++) {
        if ((float)v[i] == 0.0f) continue;  // cusp drops numeric zeros (csr_spgemm.h:135)
        m->row_offsets[(size_t)r[i] + 1]++;
        m->cols.push_back(c[i]);
        m->vals.push_back((float)v[i]);
    }
    for (int i = 0; i < A->num_rows; i++) m->row_offsets[(size_t)i + 1] += m->row_offsets[(size_t)i];
    *C = m.release();
    BMSP_API_END
}

int bmsp_csr_spmv(bmsp_csr_t A, const float *x, float *y)
{
    BMSP_API_BEGIN
    need(A, "A"); need(x, "x"); need(y, "y");
    bmsp_matrix_s *dA = csr_device_form(A, 0);
    DevBuf<float> dx((size_t)A->num_cols), dy((size_t)A->num_rows);
    copy_h2d_staged(dx.p, x, 4 * (size_t)A->num_cols);
    spmv(dA, dx.p, dy.p, BMSP_SPMV_DEFAULT, nullptr);
    copy_d2h_staged(y, dy.p, 4 * (size_t)A->num_rows);
    BMSP_API_END
}

// ---- the host path of class CSRMatrix (configs[0]: "cusp::multiply ..., host CPU path"): the reference's CSRMatrix wraps a
// cusp::csr_matrix<int,float,host_memory> (include/CSRMatrix.h:20), i.e. cusp::multiply runs on the host.  These two follow the
// host algorithms' contracts -- y[i] = sum over the row in column order, accumulator initialised to 0
// (cusp/system/detail/sequential/multiply/csr_spmv.h:56-73; rows in parallel: omp/detail/multiply/csr_spmv.h:67-85); row-wise
// Gustavson product in two passes, numeric zeros dropped by the sequential form (sequential/multiply/csr_spgemm.h:39-157) -- with
// `threads` host threads (0 = all).  No GPU call is made.
int bmsp_csr_spmv_host(bmsp_csr_t A, const float *x, float *y, int threads)
{
    BMSP_API_BEGIN
    need(A, "A"); need(x, "x"); need(y, "y");
    const int nr = A->num_rows;
    const int *ro = A->row_offsets.data(), *ci = A->cols.data();
    const float *va = A->vals.data();
    const int nt = threads > 0 ? threads : omp_get_max_threads();
    (void)nt;
    // rows in parallel, each row summed in column order (omp/detail/multiply/csr_spmv.h:67-85)
#pragma omp parallel for num_threads(nt) schedule(static, 512) if (nt > 1 && nr >= 4096)
    for (int i = 0; i < nr; i++) {
        float sum = 0.0f;
        for (int jj = ro[i]; jj < ro[i + 1]; jj++) sum += va[jj] * x[ci[jj]];
        y[i] = sum;
    }
    BMSP_API_END
}

int bmsp_csr_multiply_host(bmsp_csr_t A, bmsp_csr_t B, bmsp_csr_t *C, int threads)
{
    BMSP_API_BEGIN
    need(A, "A"); need(B, "B"); need(C, "C");
    if (A->num_cols != B->num_rows) fail(BMSP_ERR_INVALID, "shape mismatch");
    const int nr = A->num_rows, nc = B->num_cols;
    const int nt = std::max(1, std::min(threads > 0 ? threads : omp_get_max_threads(), std::max(1, nr / 256)));
    std::unique_ptr<bmsp_csr_s> m(new bmsp_csr_s());
    m->num_rows = nr; m->num_cols = nc;
    m->row_offsets.assign((size_t)nr + 1, 0);
    std::vector<std::vector<int>> t_cols((size_t)nt);
    std::vector<std::vector<float>> t_vals((size_t)nt);
    std::vector<int> bounds((size_t)nt + 1, nr);
    bounds[0] = 0;
    {
        const int64_t nnz = A->row_offsets[(size_t)nr];
        for (int t = 1; t < nt; t++)
            bounds[(size_t)t] = std::max(bounds[(size_t)t - 1], (int)(std::upper_bound(A->row_offsets.begin(), A->row_offsets.end(), (int)(nnz * t / nt)) - A->row_offsets.begin()));
        for (int t = 1; t < nt; t++) bounds[(size_t)t] = std::min(bounds[(size_t)t], nr);
    }
    auto work = [&](int t) {
        // Gustavson with a linked list of touched columns (spmm_csr_pass2, csr_spgemm.h:79-157); numeric zeros are not stored (:135)
        std::vector<int> next((size_t)nc, -1);
        std::vector<float> sums((size_t)nc, 0.0f);
        std::vector<int> &oc = t_cols[(size_t)t];
        std::vector<float> &ov = t_vals[(size_t)t];
        for (int i = bounds[(size_t)t]; i < bounds[(size_t)t + 1]; i++) {
            int head = -2, length = 0;
            for (int jj = A->row_offsets[(size_t)i]; jj < A->row_offsets[(size_t)i + 1]; jj++) {
                const int j = A->cols[(size_t)jj];
                const float v = A->vals[(size_t)jj];
                for (int kk = B->row_offsets[(size_t)j]; kk < B->row_offsets[(size_t)j + 1]; kk++) {
                    const int k = B->cols[(size_t)kk];
                    sums[(size_t)k] += v * B->vals[(size_t)kk];
                    if (next[(size_t)k] == -1) { next[(size_t)k] = head; head = k; length++; }
                }
            }
            int kept = 0;
            for (int q = 0; q < length; q++) {
                if (sums[(size_t)head] != 0.0f) { oc.push_back(head); ov.push_back(sums[(size_t)head]); kept++; }
                const int tmp = head;
                head = next[(size_t)head];
                next[(size_t)tmp] = -1;
                sums[(size_t)tmp] = 0.0f;
            }
            m->row_offsets[(size_t)i + 1] = kept;
        }
    };
#pragma omp parallel for num_threads(nt) schedule(static, 1)
    for (int t = 0; t < nt; t++) work(t);
    for (int i = 0; i < nr; i++) m->row_offsets[(size_t)i + 1] += m->row_offsets[(size_t)i];
    m->cols.reserve((size_t)m->row_offsets[(size_t)nr]);
    m->vals.reserve((size_t)m->row_offsets[(size_t)nr]);
    for (int t = 0; t < nt; t++) {
        m->cols.insert(m->cols.end(), t_cols[(size_t)t].begin(), t_cols[(size_t)t].end());
        m->vals.insert(m->vals.end(), t_vals[(size_t)t].begin(), t_vals[(size_t)t].end());
    }
    *C = m.release();
    BMSP_API_END
}

int bmsp_csr_free(bmsp_csr_t m)
{
    BMSP_API_BEGIN
    delete m;
    BMSP_API_END
}

}  // extern "C"
