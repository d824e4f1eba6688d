/*
 * bmsp.h -- C ABI of the MI355X-native bmSparse engine (libbmsp.so).
 *
 * This is the drop-in boundary.  The reference (GonzaBerger/bmSparse-SPGEMM-SPMV) has no FFI: its
 * operators are C++ templates compiled into the two executables.  Every entry point below names the
 * reference interface it replaces (paths relative to the reference repository root).  The C++ headers
 * include/bmSpMatrix.h and include/CSRMatrix.h keep the reference's class / function names on top of
 * this ABI, so a maintainer swaps the reference's nvcc translation units for `-lbmsp`.
 *
 * Conventions
 *   - plain pointers and sizes only; `void *stream` is a hipStream_t (NULL = the null stream);
 *   - "device pointer" means memory visible to the current HIP device (bmsp_malloc, hipMalloc, or a
 *     PyTorch-ROCm tensor's data_ptr());
 *   - every call returns BMSP_OK (0) or a negative bmsp_status; bmsp_last_error() gives the text for
 *     the calling thread.  Nothing calls exit() (the reference exits on CUDA errors,
 *     src/bmSparse_SPMV.cu:62-70);
 *   - a missing / unreadable file is an error (the reference silently builds an empty matrix,
 *     src/bmSpMatrix.cu:114-127);
 *   - not thread-safe per matrix handle; distinct handles may be used from distinct threads.
 */
#ifndef BMSP_H_
#define BMSP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BMSP_BLOCK_WIDTH 8   /* include/bmSpMatrix.h:15 */
#define BMSP_BLOCK_HEIGHT 8  /* include/bmSpMatrix.h:16 */

typedef enum {
    BMSP_OK = 0,
    BMSP_ERR_INVALID = -1,   /* bad argument / shape mismatch */
    BMSP_ERR_IO = -2,        /* file missing or malformed */
    BMSP_ERR_HIP = -3,       /* a HIP runtime call failed */
    BMSP_ERR_NOMEM = -4,
    BMSP_ERR_UNSUPPORTED = -5,
    BMSP_ERR_LIMIT = -6,     /* a 32-bit internal limit would overflow */
    BMSP_ERR_INTERNAL = -7   /* a bound the library proves for itself did not hold (bmsp_matrix_color_blocks: more rounds than blocks) */
} bmsp_status;

typedef enum { BMSP_F32 = 0, BMSP_F16 = 1, BMSP_F64 = 2 } bmsp_dtype;

typedef struct bmsp_matrix_s *bmsp_matrix_t; /* replaces class bmSpMatrix<T>, include/bmSpMatrix.h:20-40 */
typedef struct bmsp_csr_s *bmsp_csr_t;       /* replaces class CSRMatrix,     include/CSRMatrix.h:13-21 */

const char *bmsp_last_error(void);
const char *bmsp_version(void);

/* ---- device plumbing (lets a plain-C/C++ host manage v and u the way the reference's main does
 *      with cudaMalloc/cudaMemcpy, src/bmSparse_SPMV.cu:276-285,309) ---- */
int bmsp_device_count(int *count);
int bmsp_set_device(int device);
int bmsp_malloc(void **dptr, size_t bytes);
int bmsp_free(void *dptr);
int bmsp_memcpy_h2d(void *dst, const void *src, size_t bytes);
int bmsp_memcpy_d2h(void *dst, const void *src, size_t bytes);
int bmsp_memcpy_d2d(void *dst, const void *src, size_t bytes);
int bmsp_memset(void *dptr, int value, size_t bytes);
int bmsp_synchronize(void);
int bmsp_trim_pool(void); /* return cached device memory to the driver */
/* device-side timing (hipEvent) on the stream the operators are launched on */
int bmsp_event_create(void **event);
int bmsp_event_record(void *event, void *stream);
int bmsp_event_elapsed_ms(void *start, void *stop, float *ms); /* synchronises on `stop` */
int bmsp_event_destroy(void *event);

/* ---- container / builder ------------------------------------------------------------------- */

/* bmSpMatrix<T>::bmSpMatrix(std::string path, bool transpose)  -- src/bmSpMatrix.cu:111-219.
 * Parses a MatrixMarket coordinate file (real / integer / pattern; general / symmetric) on the host and
 * builds keys/bmps/offsets/values on the device.  `transposed` lays tiles out column-major (the B operand
 * of bmsp_spgemm, src/bmSparse_SPGEMM.cu:1262).  Accepts `path` with or without the ".mtx" suffix
 * (the reference's two mains disagree, src/bmSparse_SPMV.cu:257,270). */
int bmsp_matrix_from_mtx(const char *path, int transposed, bmsp_dtype dtype, bmsp_matrix_t *out);

/* Same builder from host COO triples (0-based).  Values are double, cast to dtype with round-to-nearest-even
 * exactly like the reference's `(valueType)data` (src/bmSpMatrix.cu:141).  Duplicate coordinates are summed
 * (the reference corrupts its popcount addressing on duplicates, src/bmSpMatrix.cu:183-216). */
int bmsp_matrix_from_coo(int num_rows, int num_cols, int64_t nnz, const int *rows, const int *cols,
                         const double *vals, int transposed, bmsp_dtype dtype, bmsp_matrix_t *out);

/* Same builder from COO triples already resident on the device (rows/cols int32, vals float64).  The contract is that of
 * bmsp_matrix_from_coo: every index lies in [0, num_rows) x [0, num_cols) and dtype is one of the three bmsp_dtype values.
 * The builder's own kernels check it on the device (no extra launch or synchronisation); a violation returns
 * BMSP_ERR_INVALID, leaves *out untouched and nothing allocated.  Runs on `stream` and synchronises it before it returns (the tile
 * count is read back, the temporaries go back to the pool). */
int bmsp_matrix_from_coo_device(int num_rows, int num_cols, int64_t nnz, const int *d_rows, const int *d_cols,
                                const double *d_vals, int transposed, bmsp_dtype dtype, void *stream,
                                bmsp_matrix_t *out);

/* bmSpMatrix<T>::bmSpMatrix(int,int,int, keys&, bmps&, offsets&, values&)  -- src/bmSpMatrix.cu:30-43.
 * ownership: 0 = copy the four device arrays; 1 = adopt them (they must come from bmsp_malloc; this is the
 * reference's swap semantics); 2 = borrow (caller keeps them alive and frees them). */
int bmsp_matrix_from_arrays(int num_rows, int num_cols, int64_t block_num, int64_t nnz, uint64_t *d_keys,
                            uint64_t *d_bmps, uint64_t *d_offsets, void *d_values, bmsp_dtype dtype,
                            int transposed, int ownership, bmsp_matrix_t *out);

/* Binary cache of the built matrix (the reference only hints at "Dumping bmSparse matrices to disk",
 * src/bmSparse_SPGEMM.cu:21,27): header + keys + bmps + offsets + values, so a SuiteSparse file is parsed and
 * sorted once.  bmsp_matrix_load restores exactly what bmsp_matrix_save wrote (bit-identical arrays). */
int bmsp_matrix_save(bmsp_matrix_t m, const char *path);
int bmsp_matrix_load(const char *path, bmsp_matrix_t *out);

int bmsp_matrix_free(bmsp_matrix_t m);

/* public members of bmSpMatrix<T>: num_rows, num_cols, nnz, block_num (include/bmSpMatrix.h:32) */
int bmsp_matrix_info(bmsp_matrix_t m, int *num_rows, int *num_cols, int64_t *nnz, int64_t *block_num,
                     bmsp_dtype *dtype, int *transposed);
/* public members keys, bmps, offsets, values (include/bmSpMatrix.h:28-31) as device pointers.
 * offsets carries block_num+1 entries (the last equals nnz); the reference holds block_num from the builder
 * (src/bmSpMatrix.cu:194) and block_num+1 after a product (src/bmSparse_SPGEMM.cu:1087,1179). */
int bmsp_matrix_arrays(bmsp_matrix_t m, uint64_t **d_keys, uint64_t **d_bmps, uint64_t **d_offsets,
                       void **d_values);
/* The arrays above are writable (bmSpMatrix<T>::values.data() is public in the reference, include/bmSpMatrix.h:31, and the reference
 * keeps no derived state, so it always sees current values).  This engine caches derived structures on the handle: after writing
 * VALUES in place call bmsp_matrix_invalidate(m, 0) before the next product (drops the dense tile copies the block-MAC kernels read);
 * after changing keys / bitmaps / offsets call it with structure_changed = 1 (drops the block-row pointer, SpMV plan and position
 * cache, block records too).  Synchronises the device.  SpMV reads values directly: a value-only update needs no call for it.
 * The library's own in-place writers need no call on their target: bmsp_matrix_copy_values, bmsp_matrix_add_values,
 * bmsp_matrix_scale_values, bmsp_sddmm_values, bmsp_spgemm_masked_values and bmsp_spgemm_numeric (whose target is C) drop the target's
 * value-derived caches themselves before they write.  Limitation: a row-panel view (bmsp_matrix_row_panel) holds caches of its own over
 * its slice of the parent's values; a write to the parent, by the caller or by one of these calls, does not reach them -- make the
 * views anew (or call bmsp_matrix_invalidate(view, 0)) after the parent's values changed. */
int bmsp_matrix_invalidate(bmsp_matrix_t m, int structure_changed);
/* Transpose and tile-layout conversion of a matrix already on the device (no COO round trip).  `out_transposed` is the layout of
 * the output's tiles, as the builders' flag: 0 row-major, 1 column-major (the right operand of bmsp_spgemm).  The output is a fresh
 * pool-owned handle whose four arrays equal, bit for bit, what the builders make from the swapped COO (transpose) or the same COO
 * (convert_layout) in that layout; offsets hold block_num+1 entries.  Values move as raw bits (-0, Inf, NaN payloads and subnormals
 * survive), every stored entry is kept, A and its caches are untouched.  Row-panel views are refused.  Work runs on `stream`; the
 * calls synchronise it before they return.
 *   bmsp_matrix_transpose:      out = A^T (num_cols x num_rows).  Into the other layout it only re-orders whole tiles.
 *   bmsp_matrix_convert_layout: out = A with tiles in layout out_transposed (a copy when A already has that layout).
 *   bmsp_matrix_copy_values:    `out` was made from A by one of the two calls above and A's STRUCTURE has not changed since (its
 *       uid, renewed by bmsp_matrix_invalidate(A, 1)): re-gathers out's values from A's current values in one pass, no sort; otherwise
 *       BMSP_ERR_INVALID.  Drops out's value-derived caches as bmsp_matrix_invalidate(out, 0) would; asynchronous on `stream` unless
 *       out holds such caches (dropping them synchronises the device). */
int bmsp_matrix_transpose(bmsp_matrix_t A, int out_transposed, void *stream, bmsp_matrix_t *out);
int bmsp_matrix_convert_layout(bmsp_matrix_t A, int out_transposed, void *stream, bmsp_matrix_t *out);
int bmsp_matrix_copy_values(bmsp_matrix_t A, bmsp_matrix_t out, void *stream);
/* Sparse addition C = alpha*A + beta*B of two matrices on the device (no COO round trip).  A and B have the same shape and dtype (F32,
 * F16 or F64); either may use either tile layout; `out_transposed` is C's layout (0 row-major, 1 column-major).
 *   Structure: C's tiles are the union of A's and B's tile keys; each C bitmap is the OR of the operands' bitmaps in C's layout.  Every
 *       coordinate stored in A or B is stored in C, numeric cancellation included (A + (-A) has A's structure with stored zeros).  The
 *       four arrays equal, bit for bit, what the builders make from the concatenated COO [A's entries; B's entries] in that layout;
 *       offsets hold block_num+1 entries.
 *   Values (never a fused multiply-add): F32 c = fl32(fl32(alpha*a) + fl32(beta*b)) with alpha, beta rounded once to fp32; an entry of
 *       one operand only is fl32(alpha*a) or fl32(beta*b).  F64 the same in double.  F16: products and sum in fp32 as for F32, then one
 *       round-to-nearest-even to fp16 (it may overflow to +-Inf).  Subnormals are kept.
 *   An operand in the other layout is read through its transposed bitmap inside the value pass (no conversion, no copy).  A and B are
 *   never modified (they may be the same handle); their block-row pointers are built if missing.  Refused with BMSP_ERR_INVALID: null
 *   handles / output pointer, out_transposed not 0 / 1, shapes or dtypes that differ, row-panel views.  BMSP_ERR_LIMIT: A and B hold
 *   2^32 - 1 tiles or more together (C's 32-bit tile maps), or B holds 2^32 values or more.
 *   bmsp_matrix_add:        a fresh pool-owned C; runs on `stream` and synchronises it before it returns (C's tile count is read back).
 *   bmsp_matrix_add_values: C was made by bmsp_matrix_add from these two operands, in this order, and neither operand's STRUCTURE changed
 *       since (their uids, renewed by bmsp_matrix_invalidate(X, 1)): re-computes C's values from A's and B's current values with this
 *       alpha and beta in one pass, no merge; otherwise BMSP_ERR_INVALID.  Drops C's value-derived caches as bmsp_matrix_copy_values
 *       does; asynchronous on `stream` unless C holds such caches (dropping them synchronises the device). */
int bmsp_matrix_add(double alpha, bmsp_matrix_t A, double beta, bmsp_matrix_t B, int out_transposed, void *stream, bmsp_matrix_t *C);
int bmsp_matrix_add_values(double alpha, bmsp_matrix_t A, double beta, bmsp_matrix_t B, bmsp_matrix_t C, void *stream);
/* Pruning: out = A without the stored entries a rule drops, on the device (no COO round trip).  The library otherwise keeps every
 * coordinate it has stored (a product's structure is symbolic, A + (-A) keeps A's structure); this is the call that shrinks a matrix.
 *   Rules: BMSP_PRUNE_ABS drops an entry iff |v| <= tol; BMSP_PRUNE_ROW_REL iff |v| <= tol * rowmax(row of the entry).  With
 *       BMSP_PRUNE_KEEP_DIAGONAL in `flags` an entry with row == col is never dropped.
 *   Comparison: exact, in double.  The stored value (F16 / F32 / F64) is widened exactly and `tol` is used as given (not rounded to the
 *       storage type); ROW_REL forms tol * rowmax as one IEEE double multiply, then compares.  There is no other arithmetic, so the result
 *       is a pure function of the bits of A and of tol.  tol = 0 under ABS drops exactly the entries equal to +0 or -0: subnormals are
 *       not zero and are kept.  NaN is never dropped by either rule (the comparison is false); +-Inf only by ABS with tol = +Inf.
 *   rowmax(i) = max of |v| over the stored, non-NaN entries of matrix row i (matrix coordinates, whatever the tile layout); 0 for a row
 *       with none.  bmsp_matrix_row_absmax writes exactly this to d_rowmax: num_rows entries, float for F32 / F16 and double for F64
 *       (the convention of bmsp_spmv's u); asynchronous on `stream`; A is not modified.
 *   Output: a fresh pool-owned handle of A's shape and dtype, tiles in layout `out_transposed` (0 row-major, 1 column-major; A may have
 *       either).  Its four arrays equal, bit for bit, what the builders make from the COO of A's kept entries in that layout: tiles that
 *       lose every entry disappear, offsets hold block_num+1 entries, kept values move as raw bits (-0 under a rule that keeps it, NaN
 *       payloads and subnormals survive).  An output with 0 tiles is a valid matrix.
 *   Count only: out == NULL with stats != NULL runs the marking passes alone and fills *stats (what a caller uses to pick a tolerance).
 *       With out != NULL, stats may be NULL.
 *   A and its caches are never modified.  bmsp_matrix_prune runs on `stream` and synchronises it before it returns (the kept counts are
 *   read back).  Refused with BMSP_ERR_INVALID, the message naming the argument: rule not 0 / 1; tol negative or NaN; ROW_REL with
 *   tol = +Inf (Inf * 0 is NaN for an empty or all-zero row); flags with unknown bits; out_transposed not 0 / 1; out and stats both NULL;
 *   null A; null d_rowmax; row-panel views.  The scalar arguments are checked before the handles.  BMSP_ERR_LIMIT: A holds 2^32 - 1
 *   tiles or more, or 2^32 values or more (kept tiles and kept values are counted in the two 32-bit halves of one scan word). */
#define BMSP_PRUNE_ABS      0   /* drop an entry iff |v| <= tol                                  */
#define BMSP_PRUNE_ROW_REL  1   /* drop an entry iff |v| <= tol * rowmax(row of the entry)       */
#define BMSP_PRUNE_KEEP_DIAGONAL 1  /* flags bit 0: an entry with row == col is never dropped    */
typedef struct { int64_t nnz_in, nnz_out, blocks_in, blocks_out; } bmsp_prune_stats;
int bmsp_matrix_prune(bmsp_matrix_t A, int rule, double tol, int flags, int out_transposed, void *stream, bmsp_matrix_t *out,
                      bmsp_prune_stats *stats);
int bmsp_matrix_row_absmax(bmsp_matrix_t A, void *d_rowmax, void *stream);
/* Selection: out = the stored entries of A a POSITION predicate keeps, on the device (no COO round trip).  Pruning shrinks a matrix by
 * value; this shrinks it by coordinate: the triangle the solves, ILU(0) and FSAI are specified on, the band of a preconditioner, the
 * off-diagonal part of a splitting, A restricted to another matrix's pattern (a Galerkin product kept on A's pattern) or to its
 * complement (the fill-in of a product, A*A without spy(A)).  No predicate reads a value.
 *   bmsp_matrix_select_band keeps a stored entry (i, j) iff lo <= j - i <= hi, in matrix coordinates whatever the tile layout.  Every
 *       pair of int64 values is legal: lo > hi is the empty band, BMSP_BAND_MIN / BMSP_BAND_MAX mean unbounded (both bounds are clamped
 *       to +-2^36; coordinates are below 2^35).  tril(A, k) = band(MIN, k), triu(A, k) = band(k, MAX), the diagonal part = band(0, 0),
 *       the off-diagonal part = band(0, 0) with BMSP_SELECT_COMPLEMENT.
 *   bmsp_matrix_select_mask keeps a stored entry of A iff M stores the same coordinate.  M has A's shape, any dtype and either layout;
 *       its values are never read (a stored zero of M counts as stored); M may be A; its block-row pointer is built if missing.
 *   BMSP_SELECT_COMPLEMENT in `flags` keeps exactly the entries the predicate rejects.
 *   Output, count-only calls, stream and side effects are bmsp_matrix_prune's: a fresh pool-owned handle of A's shape and dtype, tiles in
 *       layout `out_transposed`, whose four arrays and block-row pointer equal, bit for bit, what the builders make from the COO of the
 *       kept entries in that layout (values move as raw bits, emptied tiles disappear, 0 tiles is a valid matrix, offsets hold
 *       block_num+1 entries); out == NULL with stats != NULL counts only; A, M and their caches are never modified; the call runs on
 *       `stream` and synchronises it before it returns.  Tiles keep their keys and their order: nothing is sorted or re-tiled.
 *   Refused with BMSP_ERR_INVALID, the message naming the argument, scalars before handles: flags with unknown bits; out_transposed not
 *   0 / 1; out and stats both NULL; null A or M; shapes that differ; row-panel views.  BMSP_ERR_LIMIT: as for bmsp_matrix_prune, on A. */
#define BMSP_SELECT_COMPLEMENT 1            /* flags bit 0: keep what the predicate rejects */
#define BMSP_BAND_MIN INT64_MIN             /* lo: unbounded below */
#define BMSP_BAND_MAX INT64_MAX             /* hi: unbounded above */
typedef bmsp_prune_stats bmsp_select_stats; /* nnz_in, nnz_out, blocks_in, blocks_out */
int bmsp_matrix_select_band(bmsp_matrix_t A, int64_t lo, int64_t hi, int flags, int out_transposed, void *stream,
                            bmsp_matrix_t *out, bmsp_select_stats *stats);
int bmsp_matrix_select_mask(bmsp_matrix_t A, bmsp_matrix_t M, int flags, int out_transposed, void *stream,
                            bmsp_matrix_t *out, bmsp_select_stats *stats);
/* Diagonal operations: what connects a device VECTOR to a matrix besides bmsp_spmv, on the device (no COO round trip).  Nothing in the
 * reference is replaced: it has no diagonal, scaling or addition entry point (include/bmSpMatrix.h:20-40 declares the builders,
 * generate_coo and compare only).  Vectors are float for F32 / F16 matrices and double for F64 (the convention of bmsp_spmv's u and of
 * bmsp_matrix_row_absmax), indexed by MATRIX row / column whatever the tile layout.  No pass sorts, scans, reads back or uses an atomic.
 *   bmsp_matrix_diagonal: d_diag receives min(num_rows, num_cols) entries; entry i is the stored value at (i, i) widened exactly (F32 /
 *       F64 as raw bits: -0, NaN payloads and subnormals survive; F16 widened to float), +0 where (i, i) is not stored -- the call writes
 *       every entry itself, the buffer needs no clearing.  Either tile layout.  A is not modified (its block-row pointer is built if
 *       missing).  Asynchronous on `stream`.
 *   bmsp_matrix_from_diagonal: a fresh pool-owned num_rows x num_cols matrix with d_diag[i] stored at every (i, i), i < min(num_rows,
 *       num_cols), zeros included (the library keeps what it is given; bmsp_matrix_prune is the call that drops).  Its four arrays and
 *       block-row pointer equal, bit for bit, what bmsp_matrix_from_coo makes from the triples (i, i, d_diag[i]) in layout `transposed`:
 *       tile t has key (t << 32) | t, the positions 0, 9, .., 63 (cut to the count of the last tile) and offset 8t.  F16 values are rounded
 *       from the float input by the builder's round-to-nearest-even conversion.  min(num_rows, num_cols) == 0 gives a valid matrix of 0
 *       tiles with offsets = [0] (d_diag may then be NULL).  Asynchronous on `stream`.
 *   bmsp_matrix_scale: out = diag(l) * A * diag(r), l = d_left (num_rows entries), r = d_right (num_cols entries).  Either pointer may be
 *       NULL: that side is skipped, not multiplied by 1; with both NULL the call is bmsp_matrix_convert_layout, bit for bit.  `out` is a
 *       fresh pool-owned handle of A's shape and dtype with tiles in layout out_transposed (A may have either); its keys, bitmaps,
 *       offsets and block-row pointer equal bmsp_matrix_convert_layout(A, out_transposed)'s: every coordinate is kept, results that are
 *       0, Inf or NaN included.  Values: the left factor first, then the right, each operation rounded on its own.  F32:
 *       c = fl32(fl32(l o a) o r), each o an IEEE multiply, or an IEEE divide x / d under BMSP_SCALE_DIV_LEFT / _RIGHT for that side
 *       (the full division sequence, never a reciprocal).  F64 the same in double.  F16: a is widened exactly, the F32 formula is
 *       evaluated in fp32 and the result rounded once to fp16, round-to-nearest-even (it may overflow to +-Inf).  Subnormal inputs and
 *       results are kept; x / 0, 0 / 0, 0 * Inf give what IEEE gives.  A and its caches are not modified.  The output remembers A as a
 *       layout conversion does, so bmsp_matrix_scale_values and bmsp_matrix_copy_values accept it.  Asynchronous on `stream`: unlike its
 *       siblings the call does NOT synchronise (nothing is read back, no temporary is allocated); synchronise the stream before reading
 *       the arrays from another stream or the host.
 *   bmsp_matrix_scale_values: the same value pass into an existing matrix.  out == A scales A in place.  Otherwise `out` must have been
 *       made from A by bmsp_matrix_scale or bmsp_matrix_convert_layout while A's STRUCTURE has not changed since (its uid, renewed by
 *       bmsp_matrix_invalidate(A, 1)); anything else -- an unrelated handle, a bmsp_matrix_transpose output -- is BMSP_ERR_INVALID.
 *       Drops out's value-derived caches as bmsp_matrix_copy_values does (dense tiles, lane tiles, CSR copy, finite flags), an in-place
 *       A's included; its SpMV plan and position cache stay.  Asynchronous on `stream` unless out holds such caches (dropping them
 *       synchronises the device).
 *   Refused with BMSP_ERR_INVALID, the message naming the argument, scalar arguments before handles: flags with unknown bits;
 *   out_transposed / transposed not 0 / 1; a dtype that is none of the three; negative num_rows / num_cols; a DIV flag whose vector is
 *   NULL; null A, out, d_diag (bmsp_matrix_from_diagonal: only while min(num_rows, num_cols) > 0); row-panel views. */
int bmsp_matrix_diagonal(bmsp_matrix_t A, void *d_diag, void *stream);
int bmsp_matrix_from_diagonal(int num_rows, int num_cols, const void *d_diag, bmsp_dtype dtype, int transposed, void *stream,
                              bmsp_matrix_t *out);
#define BMSP_SCALE_DIV_LEFT  1   /* divide by d_left[row] instead of multiplying  */
#define BMSP_SCALE_DIV_RIGHT 2   /* divide by d_right[col] instead of multiplying */
int bmsp_matrix_scale(bmsp_matrix_t A, const void *d_left, const void *d_right, int flags, int out_transposed, void *stream,
                      bmsp_matrix_t *out);
int bmsp_matrix_scale_values(bmsp_matrix_t A, const void *d_left, const void *d_right, int flags, bmsp_matrix_t out,
                             void *stream);
/* dense block-row pointer (num_block_rows+1 uint32 entries) the operators use; built once and cached
 * (the reference rebuilds a compressed one on every call, src/bmSparse_SPMV.cu:199-206). */
int bmsp_matrix_block_row_ptr(bmsp_matrix_t m, const uint32_t **d_rowptr, int64_t *num_block_rows);

/* Builds, ahead of the first product, the per-matrix structures the operators derive lazily and cache (none of them is part of
 * the reference's public state): `what` bit 0 = the SpMV sweep plan (the reference rebuilds its block-row pointer inside every
 * timed SpMV, src/bmSparse_SPMV.cu:199-206) and, for matrices of sparse tiles, its position cache: one 16-bit {tile slot, position}
 * entry per stored value (2 * nnz bytes of device memory; BMSP_SPMV_NO_POSCACHE=1 or a size above BMSP_SPMV_POSCACHE_MAX bytes,
 * default 4 GiB, keeps the bitmap decode inside the kernel instead); bit 1 = the packed operand records of the SpGEMM block-MAC (both
 * operand roles, incl. the dense fp16 tile copies of the MFMA kernels: 128 bytes per block).
 * Idempotent.  Runs on `stream` and synchronises it whenever it builds something (the scalar read-backs of the plan, the finite /
 * exponent flags of the operand records, temporaries that go back to the pool); a call that finds everything built returns at once. */
#define BMSP_PREPARE_SPMV 1
#define BMSP_PREPARE_SPGEMM 2
int bmsp_matrix_prepare(bmsp_matrix_t m, int what, void *stream);

/* bmSpMatrix<T>::generate_coo()  -- src/bmSpMatrix.cu:320-363.  Expands to host COO sorted by (row,col);
 * rows/cols/vals must hold nnz entries.  Unlike the reference it honours the transposed layout. */
int bmsp_matrix_to_coo_host(bmsp_matrix_t m, int *rows, int *cols, double *vals);

/* SURVEY 8(f)2 -- the same expansion with the result left on the device, as COO or CSR sorted by (row, col), so a product can
 * feed CSR consumers without a host round trip.  d_rows/d_cols/d_vals hold nnz entries, d_row_offsets num_rows+1.  Both run on
 * `stream` and synchronise it before they return (their temporaries go back to the pool). */
int bmsp_matrix_to_coo_device(bmsp_matrix_t m, int *d_rows, int *d_cols, double *d_vals, void *stream);
int bmsp_matrix_to_csr_device(bmsp_matrix_t m, int *d_row_offsets, int *d_cols, double *d_vals, void *stream);
/* ... and the builder from a device-resident CSR (int32 offsets/columns, float64 values; duplicates summed as in from_coo).
 * Contract, checked on the device like bmsp_matrix_from_coo_device's (for nnz == 0 at the price of one small launch and a
 * synchronise, which an empty matrix did not have): d_row_offsets[0] == 0, d_row_offsets[num_rows] == nnz, no
 * offset larger than the next, every column in [0, num_cols), a known dtype; otherwise BMSP_ERR_INVALID and no matrix.  Runs on
 * `stream` and synchronises it before it returns, as bmsp_matrix_from_coo_device. */
int bmsp_matrix_from_csr_device(int num_rows, int num_cols, int64_t nnz, const int *d_row_offsets, const int *d_cols,
                                const double *d_vals, int transposed, bmsp_dtype dtype, void *stream, bmsp_matrix_t *out);

/* bmSpMatrix<T>::compare(coo)  -- src/bmSpMatrix.cu:381-432.  Mean relative error against a host COO
 * comparand (entries of the comparand that are absent from m are skipped).  *missing counts entries of m
 * that the comparand lacks (the reference would walk out of bounds). */
int bmsp_matrix_compare(bmsp_matrix_t m, int64_t nnz, const int *rows, const int *cols, const double *vals,
                        double *mean_rel_err, int64_t *missing);
/* the same comparison with a device-resident comparand, entirely on the device (large products); runs on `stream` and
 * synchronises it before it returns (the two results are host values) */
int bmsp_matrix_compare_device(bmsp_matrix_t m, int64_t nnz, const int *d_rows, const int *d_cols, const double *d_vals,
                               double *mean_rel_err, int64_t *missing, void *stream);

/* ---- operators ------------------------------------------------------------------------------ */

/* variants of the SpMV sweep.  0 = reference's default path (`batched`=false, spmv_kernel
 * src/bmSparse_SPMV.cu:153-189), 1 = the wavefront-reduce path `batched`=true was meant to select
 * (spmv_kernel_new :84-150).  Both give the same u; they differ in the lane mapping. */
#define BMSP_SPMV_DEFAULT 0
#define BMSP_SPMV_BATCHED 1

/* bmSparse_SpMV<VI,VO>(A, v, u, batched)  -- src/bmSparse_SPMV.cu:191-230.   u = A * v
 * v: device, num_cols entries of A's dtype; u: device, num_rows entries (float for F32/F16, double for F64).
 * Asynchronous on `stream` once the cached sweep plan of A exists; the call that builds the plan, the position cache or the chunk
 * cache (the first sweep of a handle that takes a kernel which needs them, or bmsp_matrix_prepare) synchronises `stream` for their
 * scalar read-backs.  A is not modified.
 *   Sum: u_i = the sum over the STORED entries of row i of a * v -- the rule of every kernel the launcher may pick, whatever the variant:
 *       an element of v at a column where row i stores nothing never reaches u_i, whatever it holds (Inf, NaN), inside a stored tile too
 *       (the reference multiplies whole tiles: there 0 * Inf = NaN along a tile row).  A stored value is always
 *       multiplied: a stored 0 against an Inf in v gives NaN, a stored Inf or NaN propagates as IEEE 754 says.  Products and sums are in
 *       fp32 (double for F64), in the implementation's order, contraction into fused multiply-adds allowed; F16 operands are widened
 *       exactly; subnormal operands and results are kept (no kernel flushes them, the LDS float adds of spmv_vstream_kernel<., kAtomic>
 *       included: tests/test_spmv_special_values.py).  A row without stored entries is +0 (rows of empty block-rows too).  The sign of a
 *       zero sum and the sign or payload of a NaN are not specified.
 *   Pointers: d_v and d_u need the alignment of their element type and no more (a view one element into an allocation is a legal
 *       argument); nothing before d_u[0] or behind d_u[num_rows - 1] is written.
 * One stream per handle at a time: the cached sweep plan holds the hub rows' carry slots and arrival counters, so two sweeps of the
 * SAME handle must not be in flight on different streams (different handles may). */
int bmsp_spmv(bmsp_matrix_t A, const void *d_v, void *d_u, int variant, void *stream);

/* What bmsp_spmv(A, ..., variant, ...) launches and what that launch must move (the measurement contract of SURVEY 8(d): "if the build
 * stores a more compact internal layout, use that layout's compulsory bytes"): kernel_name receives the name of the kernel the launcher
 * picks for this matrix -- it shares the launcher's decision: one function makes it for both, and for bmsp_spmv_chunk_layout and
 * bmsp_matrix_prepare -- (the cached plan and position cache are built if they are not yet), *compulsory_bytes the bytes of every array
 * that kernel reads or writes, each once, counted from the plan; *format_bytes the layout-independent figure 24 B per block + values +
 * block-row pointer + x + y.  Reporting only: no reference line to replace (the reference prints a time, src/bmSparse_SPMV.cu:306). */
int bmsp_spmv_launch_info(bmsp_matrix_t A, int variant, char *kernel_name, size_t kernel_name_cap, int64_t *compulsory_bytes, int64_t *format_bytes);

/* The layout of the chunked sweep's structure cache for A (spmv_chunk_kernel; the cache is built if it is not yet, as
 * bmsp_spmv_launch_info builds it): *layout = 0 when the default sweep of A does not take the chunked kernel, 1 = one word {row, column}
 * per stored value in storage order, 2 = the row-sorted words (up to 2^20 columns; BMSP_SPMV_CHUNK_SORTED=0 keeps layout 1).  Both move
 * the same bytes.  Reporting only. */
int bmsp_spmv_chunk_layout(bmsp_matrix_t A, int *layout);

/* u = alpha * op(A) * v + beta * u, op(A) = A (BMSP_OP_N) or A^T (BMSP_OP_T), for a matrix in EITHER tile layout -- without
 * bmsp_matrix_transpose / bmsp_matrix_convert_layout, a second copy of the matrix or a second set of SpMV caches.  Nothing in the reference
 * is replaced: its one product is u = A * v on a row-major A (src/bmSparse_SPMV.cu:191-230; bmsp_spmv above).
 *   Vectors: v has the input length of op(A) (num_cols for N, num_rows for T), elements of A's dtype (fp16 for F16), as bmsp_spmv's v;
 *       u has the output length, float for F32 / F16 and double for F64.  Matrix coordinates, whatever the tile layout.
 *   Sum: t_j = the sum over the stored entries of row j of op(A) of a * v, products and sums in fp32 (double for F64), F16 operands widened
 *       exactly; +0 for a row without stored entries.  The order of summation is the implementation's, but t is a pure function of A's
 *       arrays, v and the two switches below: no floating-point atomic anywhere, no dependence on scheduling, two calls with the same
 *       inputs give the same bits.
 *   Epilogue: alpha and beta are rounded once to the vector type.  beta == 0 (after that rounding): u_j = fl(alpha * t_j); u is not read,
 *       a NaN in it does not propagate.  Otherwise u_j = fl(fl(alpha * t_j) + fl(beta * u_j)), each operation rounded on its own, never
 *       contracted (as bmsp_matrix_add).  alpha == 0 is not special-cased.  Every entry of u is written.
 *   (N, row-major A) is bmsp_spmv's case: t is exactly what bmsp_spmv(A, v, ., BMSP_SPMV_DEFAULT) writes; with alpha == 1 and beta == 0
 *       the call IS that call, otherwise bmsp_spmv runs into a temporary kept on the handle and one epilogue kernel follows.
 *   The other three cases sweep a cached view, one per op, built on first use (structure only: 16 B per tile -- bitmap, value offset, the
 *       tile's other block index -- in the order of the output blocks, A's own for N, (block-column, block-row) for T; 16 B per work
 *       item; 8 accumulators of scratch per item of an output block of more than SPLIT tiles).  Values are read from A's value array at
 *       every call, so a value-only update in place needs no bmsp_matrix_invalidate (as for bmsp_spmv).  The view is dropped by
 *       bmsp_matrix_invalidate(A, 1) and bmsp_matrix_free; bmsp_matrix_invalidate(A, 0), bmsp_matrix_copy_values, _scale_values and
 *       _add_values into A keep it.  bmsp_matrix_prepare does not build it.
 *   Asynchronous on `stream`, except for the one-time build of the view (it synchronises).  A's four arrays are not modified.  One stream
 *       per handle at a time (the scratch and the temporary live on the handle).
 *   Switches: BMSP_SPMV_OP_SLOTS=1/8, read per call (lane groups of a wave that walk one work item; default 8 from a mean of 6 tiles per
 *       output block); BMSP_SPMV_OP_SPLIT=<tiles>, read when a view is built (default 64).
 *   Refused with BMSP_ERR_INVALID, the message naming the argument, scalars before handles: op not 0 / 1; null A, d_v, d_u, info;
 *   row-panel views.  BMSP_ERR_LIMIT: 2^32 tiles or values or more. */
#define BMSP_OP_N 0
#define BMSP_OP_T 1
int bmsp_spmv_op(bmsp_matrix_t A, int op, double alpha, const void *d_v, double beta, void *d_u, void *stream);
/* What bmsp_spmv_op(A, op, ...) launches -- the launcher's own decisions, for tests to pin: the sweep kernel by name
 * ("spmv_op_sweep_kernel<MINOR, 8>": MAJOR / MINOR = the output index is the byte / the bit index of the bitmap; "bmsp_spmv: <kernel>" for
 * (N, row-major A), which has no view: slots, items, split_blocks 0), the lane groups per item (1 / 8), the work items, the output blocks
 * split into several items, the bytes the view holds and the bytes the launch moves (records, values, items, v, u, scratch stored and read
 * back, fold list; bmsp_spmv_launch_info's figure for bmsp_spmv).  Builds the view if it is missing.  Reporting only. */
typedef struct { char kernel[64]; int slots; int64_t items, split_blocks, view_bytes, compulsory_bytes; } bmsp_spmv_op_info;
int bmsp_spmv_op_launch_info(bmsp_matrix_t A, int op, bmsp_spmv_op_info *info);
/* The item planner of the view, host only (no GPU call): over `blocks` output blocks with tiles [ptr[b], ptr[b + 1]), a block of at most
 * `split` tiles is one item {b, first tile, end tile, ~0u}; a longer one gets ceil(n / split) items of at most `split` tiles, their fourth
 * word consecutive scratch slots, and one fold entry {b, first slot, parts}.  items (4 words each) and folds (3 words each) may be NULL
 * (the counts alone: call twice); *n_items, *split_blocks, *slots (each may be NULL) receive the counts. */
int bmsp_spmv_op_plan_items(const uint32_t *ptr, int64_t blocks, int64_t split, uint32_t *items, uint32_t *folds, int64_t *n_items,
                            int64_t *split_blocks, int64_t *slots);

/* SpSV, the sparse triangular solve on the device: op(tri(A)) * x = alpha * b, tri(A) the lower or the upper triangle of a square A in
 * EITHER tile layout, op(.) = BMSP_OP_N / BMSP_OP_T, the diagonal stored or taken as 1 -- a Gauss-Seidel sweep, the application of an
 * incomplete factor, the substitution after a factorisation, without bmsp_matrix_to_csr_device and another library.  No conversion, no
 * transpose, no second copy of A.  Nothing in the reference is replaced (it has no solve).
 *   Operands: A is n x n, F32, F16 or F64.  b and x hold n entries of the vector type (float for F32 / F16, double for F64: the convention
 *       of bmsp_matrix_diagonal and _scale).  d_x == d_b (in place) is legal; any other overlap is the caller's error.  `fill` names the
 *       triangle of A that is read, BEFORE op: the effective system is lower iff (fill == BMSP_FILL_LOWER) != (op == BMSP_OP_T).  Tiles on
 *       the other side of the block diagonal are never read, nor the other-side entries of a diagonal tile, nor -- under BMSP_DIAG_UNIT --
 *       the stored diagonal: a NaN stored there does not reach x.  A's four arrays are not modified.
 *   Numerics, fixed bit for bit: alpha is rounded once to the vector type and s = fl(alpha * b_i); then one fused multiply-add per STORED
 *       entry of row i of the effective strict triangle, s = fma(-a_ij, x_j, s), in the order a sequential substitution meets them
 *       (ascending j for a lower system, descending j for an upper one); then x_i = s / a_ii as one IEEE division (the full division
 *       sequence, never a reciprocal), or x_i = s under BMSP_DIAG_UNIT.  fp32 arithmetic (double for F64), F16 values widened exactly,
 *       subnormals kept.  A stored zero on the diagonal gives what IEEE gives; Inf / NaN propagate along dependencies only.  x is a pure
 *       function of A's arrays, b and alpha: it does not depend on scheduling, on BMSP_SPSV_CHAIN or on the stream.  Every x_i, i < n, is
 *       written (rows of block-rows without tiles too, under BMSP_DIAG_UNIT); nothing at or beyond n is.
 *   Plan: cached on the handle per (op, fill), structure only.  The level of a block-row (of op(A)) is 1 + the largest level of the
 *       block-rows it depends on, every tile of the strict block triangle counting as a dependency whatever its bitmap; the plan holds the
 *       block-rows ordered by (level, index), the level pointer and the launch schedule.  It is built by bmsp_spsv_analyse or by the first
 *       bmsp_spsv that finds none: the build copies the block pointer and the 4-byte other-index column to the host, levels them there in
 *       one pass (bmsp_spsv_plan), uploads the result and synchronises `stream`.  Op T and column-major matrices reuse the cached view of
 *       bmsp_spmv_op (built if missing); (N, row-major A) reads A's own arrays.  Values are read from A at every call: a value-only update
 *       needs no bmsp_matrix_invalidate.  bmsp_matrix_invalidate(A, 1) and bmsp_matrix_free drop the plan; bmsp_matrix_invalidate(A, 0),
 *       bmsp_matrix_copy_values, _scale_values and _add_values into A keep it.  Once the plan exists bmsp_spsv is asynchronous on
 *       `stream`: launches only, no temporary, nothing read back; solves of one handle may run on different streams.
 *   Kernels (vector ALU): eight lanes per block-row, a lane per row.  spsv_level_kernel: one launch per level, 32 block-rows per
 *       workgroup.  spsv_chain_kernel: ONE workgroup walks a maximal run of at least two consecutive levels of at most CHAIN block-rows
 *       each, a workgroup barrier between levels.  There is no waiting between workgroups anywhere: no flag, no spin, no atomic, no
 *       cooperative launch.  BMSP_SPSV_CHAIN=<block-rows> is read when a plan is built; 0 = never chain, one launch per level (default 32,
 *       one pass of a workgroup: see README).  A block-row of thousands of tiles is one lane group's serial chain, and a matrix of
 *       thousands of levels is thousands of dependent steps: the fixed order is kept, long block-rows are not split.
 *   bmsp_spsv_analyse: builds the plan if it is missing and reports it (info may be NULL): the level kernel's instantiation by name
 *       ("spsv_level_kernel<F32, MAJOR, LOWER, NON_UNIT>": dtype; MAJOR / MINOR as for bmsp_spmv_op; the EFFECTIVE triangle; the diagonal;
 *       "none (empty matrix)" for n = 0), the levels, the widest level in block-rows, the launches of one solve, how many of them are chain
 *       launches and how many levels those cover, and the device bytes of the plan.
 *   Refused with BMSP_ERR_INVALID, the message naming the argument, scalars before handles: op, fill or diag not 0 / 1; null A, d_b, d_x;
 *   num_rows != num_cols; row-panel views; BMSP_DIAG_NON_UNIT with a row i < n whose (i, i) is not stored (found during the analysis; the
 *   message names the first such row; a BMSP_DIAG_UNIT call of the same handle still works).  BMSP_ERR_LIMIT: 2^32 tiles or values or more. */
#define BMSP_FILL_LOWER 0
#define BMSP_FILL_UPPER 1
#define BMSP_DIAG_NON_UNIT 0
#define BMSP_DIAG_UNIT 1
typedef struct { char kernel[64]; int64_t levels, max_level_width, launches, chain_launches, chained_levels, plan_bytes; } bmsp_spsv_info;
int bmsp_spsv_analyse(bmsp_matrix_t A, int op, int fill, int diag, void *stream, bmsp_spsv_info *info /* may be NULL */);
int bmsp_spsv(bmsp_matrix_t A, int op, int fill, int diag, double alpha, const void *d_b, void *d_x, void *stream);
/* The planner, host only, no GPU call: over `blocks` output blocks whose records [ptr[I], ptr[I + 1]) carry the other block index
 * other[t], block I depends on every other[t] < I (lower != 0) or > I (lower == 0).  level_of[I] (blocks entries) = 0 without
 * dependencies, else 1 + the largest level depended on; order (blocks entries) = the blocks sorted by (level, index); level_ptr
 * (*n_levels + 1 entries; at most blocks + 1) = where each level begins in order; segments (3 words per launch; at most 3 * blocks) =
 * {first level, end level, kind}: kind 1 = one chain launch over a maximal run of at least two consecutive levels of at most `chain`
 * blocks each, kind 0 = one level launch.  Every output pointer may be NULL.  Refused with BMSP_ERR_INVALID: negative blocks or chain, null
 * ptr while blocks > 0, a ptr that decreases, an `other` index >= blocks. */
int bmsp_spsv_plan(const uint32_t *ptr, const uint32_t *other, int64_t blocks, int lower, int64_t chain,
                   uint32_t *level_of, uint32_t *order, uint32_t *level_ptr, uint32_t *segments,
                   int64_t *n_levels, int64_t *n_segments);

/* SpSM, the sparse triangular solve for k right-hand sides: op(tri(A)) * X = alpha * B, everything else as bmsp_spsv -- block Krylov
 * methods, several Gauss-Seidel sweeps at once, the multi-vector application of an incomplete factor next to bmsp_spmm / bmsp_spmm_op.  A
 * solve is a chain of dependent steps, not a stream of bytes, and k calls of bmsp_spsv pay the whole chain k times; the columns of B are
 * independent, so one walk of the chain carries them all.  Nothing in the reference is replaced (it has no solve).
 *   Operands: B and X are n x k, row-major, leading dimensions ldb >= k and ldx >= k (the convention of bmsp_spmm / bmsp_spmm_op),
 *       elements of bmsp_spsv's vector type (float for F32 / F16, double for F64), aligned to their element type and no more.  op, fill and
 *       diag mean exactly what they mean for bmsp_spsv; A may be in either tile layout.
 *   Numerics, one sentence: column c of X holds, bit for bit, what bmsp_spsv(A, op, fill, diag, alpha, column c of B) writes -- s =
 *       fl(alpha * b), one fma(-a_ij, x_j, s) per stored entry of the effective strict triangle in the order of a sequential substitution,
 *       one IEEE division per row (the full sequence, never a reciprocal) or none under BMSP_DIAG_UNIT.  X is a pure function of A's
 *       arrays, B and alpha: it does not depend on BMSP_SPSM_LANES, on BMSP_SPSV_CHAIN, on k, on the strides or on the stream.  Columns do
 *       not mix: an Inf or NaN in one column of B never reaches another column of X.
 *   Read and written: every X[i][c], i < n, c < k, is written (rows of block-rows without tiles too, under BMSP_DIAG_UNIT).  The padding
 *       columns k <= c < ld of B are never read, those of X never written, no row at or beyond n of either is touched.  As in bmsp_spsv the
 *       other triangle, the other-side entries of a diagonal tile and -- under BMSP_DIAG_UNIT -- the stored diagonal never reach X.  d_X ==
 *       d_B with ldx == ldb is legal (in place); d_X == d_B with different strides is refused; any other overlap is the caller's error.
 *   Plan: none of its own.  The call uses the cached bmsp_spsv plan of (op, fill) -- the same levels, order and launch schedule;
 *       BMSP_SPSV_CHAIN keeps its meaning -- and builds it if it is missing, by the code bmsp_spsv uses (that build synchronises `stream`);
 *       op T and column-major matrices use the cached view of bmsp_spmv_op, as bmsp_spsv does.  A plan built by bmsp_spsv / _spsv_analyse
 *       serves bmsp_spsm and the other way round; it is dropped by the same events, and a value-only update needs no
 *       bmsp_matrix_invalidate.  Once the plan exists the call is asynchronous on `stream`: launches only, no temporary, nothing read back.
 *   Kernels (vector ALU): a lane owns ONE column of X for one block-row, all eight rows of it, as eight sums in registers; W lanes (W
 *       columns) form a slot, a workgroup holds 256 / W slots (block-rows); the columns beyond W go to further column chunks, independent
 *       of each other.  spsm_level_kernel: one launch per level, grid (ceil(width / slots), column chunks).  spsm_chain_kernel: one
 *       workgroup per column chunk walks the levels of a chain launch, a workgroup barrier between levels.  No waiting between workgroups:
 *       no flag, no spin, no atomic, no cooperative launch.  A slot's lanes read the same bitmap and values of a tile and load the rows of
 *       X side by side; inside the diagonal tile a lane substitutes on its own.  W in {8, 16, 32, 64}: the smallest W >= min(k, 64), or
 *       what BMSP_SPSM_LANES=8/16/32/64 forces (read per call; measured in DESIGN 4 "Triangular solve, several right-hand sides").
 *   k == 1 with ldb == ldx == 1 IS bmsp_spsv: the call is handed over (as bmsp_spmm hands k = 1 to the SpMV).  n == 0 returns BMSP_OK
 *       without a launch.
 *   bmsp_spsm_launch_info: reporting only, from the function the launcher itself calls; builds the plan if it is missing, like the call.
 *       kernel = the instantiation by name ("spsm_level_kernel<F32, MAJOR, LOWER, NON_UNIT, 32>": the first four as in bmsp_spsv_analyse,
 *       then W; "bmsp_spsv: <bmsp_spsv_analyse's kernel name>" with lanes 8 and col_chunks 1 for the hand-off; "none (empty matrix)" for
 *       n = 0), lanes = W, col_chunks = ceil(k / W); levels, launches, chain_launches, chained_levels and plan_bytes are those of the
 *       shared plan (a launch covers all column chunks through the grid, so launches equals bmsp_spsv_analyse's).
 *   Refused with BMSP_ERR_INVALID, the message naming the argument, scalars before handles, nothing done on the device: op, fill or diag
 *   not 0 / 1; k < 1, ldb < k, ldx < k; null A, d_B, d_X, info; num_rows != num_cols; row-panel views; d_X == d_B with ldb != ldx;
 *   BMSP_DIAG_NON_UNIT with a row whose diagonal entry is not stored (bmsp_spsv's message).  BMSP_ERR_LIMIT: as for bmsp_spsv. */
int bmsp_spsm(bmsp_matrix_t A, int op, int fill, int diag, double alpha, const void *d_B, int64_t ldb, void *d_X, int64_t ldx, int k,
              void *stream);
typedef struct { char kernel[64]; int lanes, col_chunks; int64_t levels, launches, chain_launches, chained_levels, plan_bytes; } bmsp_spsm_info;
int bmsp_spsm_launch_info(bmsp_matrix_t A, int op, int fill, int diag, int k, int64_t ldb, int64_t ldx, void *stream, bmsp_spsm_info *info);

/* SpITSV, the iterative sparse triangular solve: block-Jacobi sweeps towards the x of op(tri(A)) * x = alpha * b -- the application of an
 * incomplete factor or a Gauss-Seidel sweep inside a Krylov iteration, which needs the preconditioner's accuracy and not the exact
 * substitution.  bmsp_spsv walks a dependency chain, `levels` dependent steps; a sweep is ONE launch over all block-rows with full
 * parallelism, and a handful of sweeps reaches a useful accuracy.  Nothing in the reference is replaced (it has no solve).
 *       x_I^{k+1} = T_II^{-1} * (alpha * b_I - sum over the tiles T_IJ, J != I, of the effective triangle of T_IJ * x_J^k)
 * for every block-row I of eight rows: exact inside the 8 x 8 diagonal tile, Jacobi between block-rows.
 *   Operands: A, op, fill, diag, alpha and the vector type of b and x are exactly bmsp_spsv's, both tile layouts, F32 / F16 / F64.  What
 *       is never read is bmsp_spsv's too: the other triangle, the other-side entries of a diagonal tile and -- under BMSP_DIAG_UNIT -- the
 *       stored diagonal.  A's four arrays and b are not modified.  d_x == d_b is refused: b is read in every sweep.
 *   A sweep: every row runs bmsp_spsv's chain of operations -- s = fl(alpha * b_i); one s = fma(-a_ij, x_j, s) per stored entry of row i of
 *       the effective strict triangle in chain order (ascending j for a lower system, descending for an upper one), x_j taken from the
 *       PREVIOUS iterate when column j lies outside row i's own block of eight and from the NEW values inside it (those entries come last
 *       in chain order); one IEEE division, or none under BMSP_DIAG_UNIT.  Every x_i, i < n, is written by every sweep, nothing at or
 *       beyond n is.  The initial iterate is +0 and d_x is not read -- whatever it held, NaN included, never reaches x -- unless
 *       BMSP_ITSV_X0_GIVEN is set in `flags`: then d_x holds x^0.
 *   Finite termination: a block-row of plan level l (bmsp_spsv_analyse) holds bmsp_spsv's bits after sweep l + 1 and keeps them, so
 *       after `levels` sweeps x is bit for bit bmsp_spsv's x, the only bitwise fixed point of the sweep.
 *   Per-sweep statistics, order-independent and therefore deterministic: changed = some x_i differs in bits from the previous iterate;
 *       delta = max_i |fl(x_i^{k+1} - x_i^k)| and xmax = max_i |x_i^{k+1}|, both in the vector type, NaNs skipped.
 *   Stop rule, in the vector type with tol rounded once: stop after sweep k iff !changed || (tol > 0 && delta <= fl(tol * xmax)).
 *       tol == 0 means "until nothing changes": with max_iter >= levels + 1 the call returns bmsp_spsv's bits.  max_iter == 0 means
 *       levels + 1 of the cached plan.  x, sweeps and converged are a pure function of A's arrays, b, alpha, x^0, tol and max_iter: they do
 *       not depend on the stream, on scheduling or on BMSP_SPITSV_CHECK.
 *   Results: x in d_x.  delta_history (host, may be NULL): delta_history[k], k < sweeps, = sweep k's delta, widened exactly.  info (may be
 *       NULL): the kernel instantiation by name ("spitsv_sweep_kernel<F32, MAJOR, LOWER, NON_UNIT, STATS>", the first four as in
 *       bmsp_spsv_analyse, then STATS / NO_STATS; "none (empty matrix)" for n = 0), sweeps = the sweeps that ran, levels of the plan,
 *       converged = the stop rule held at sweep `sweeps` (0: max_iter sweeps ran without it), and the last sweep's delta and xmax.
 *   tol == BMSP_ITSV_NO_CHECK, the preconditioner mode: exactly max_iter sweeps (levels + 1 for 0) by a kernel instantiation without
 *       statistics.  Once the plan and the handle's temporary exist the call is fully asynchronous on `stream`: launches and at most one
 *       device copy, nothing read back, no pool temporary.  delta_history must be NULL; info gets sweeps = max_iter, converged = 0 and
 *       delta = xmax = -1.
 *   Plan and buffers: the cached plan of (A, op, fill) is bmsp_spsv's own -- built if missing (that synchronises `stream`), shared with
 *       bmsp_spsv / bmsp_spsm, dropped by the same events; only its `levels` and its missing-diagonal row are used, a sweep has no
 *       schedule.  Values are read at every call: a value-only update needs no bmsp_matrix_invalidate.  The iterates ping-pong between d_x
 *       and ONE temporary of n vector elements kept on the handle (made by the first call, freed with the plans and with the handle); if
 *       the last iterate sits in the temporary one asynchronous device copy moves it to d_x.  Because of that temporary, calls of ONE
 *       handle must not overlap on different streams.
 *   Kernel (vector ALU): spitsv_sweep_kernel, one launch per sweep, eight lanes per block-row, 32 block-rows per workgroup, block-rows
 *       in natural order, tile records read one ahead, bmsp_spsv's lane mapping and in-tile substitution.  With statistics: reduced
 *       across the wave in registers and across the workgroup in LDS, then at most one integer atomic max / or per workgroup and statistic
 *       into the sweep's own record (the bits of a non-negative float order like an unsigned integer: no floating-point atomic).  Sweep
 *       k + 1 begins by evaluating the stop rule on record k and returns without writing if it holds; the host enqueues
 *       BMSP_SPITSV_CHECK=<sweeps> sweeps (read per call, default 8), reads the records back and decides by the same predicate.  A checked
 *       call therefore synchronises `stream` once per BMSP_SPITSV_CHECK sweeps.  Long block-rows are not split (the chain order is the
 *       contract): a hub block-row of thousands of tiles is one lane group's serial chain and bounds the sweep -- see README.
 *   Measured (one MI355X, fp32, L = tril(A) + dominant diagonal, (N, lower); tools/spitsv_bench.py, DESIGN 4 "Iterative triangular solve"):
 *       banded half-bandwidth 32, 2^17 rows, 16 384 levels: a sweep 8.8 us (bmsp_spmv on the triangle 7.7 us, bmsp_spsv 92.3 ms); the call
 *       to 2^-10 5 sweeps / 124 us, to 2^-20 9 sweeps / 217 us, to the bitwise fixed point 66 sweeps / 1.19 ms.  fem_like 27pt, 12 380
 *       levels: a sweep 17.6 us, 2^-10 9 sweeps / 259 us, 2^-20 17 sweeps / 432 us (bmsp_spsv 129.0 ms).  Hub block-rows: webbase-1M-like
 *       (R-MAT 2^20 x 2, 376 levels) a sweep 1.17 ms against 16.6 us of bmsp_spmv, 2^-10 12 sweeps / 14.3 ms, 2^-20 18 sweeps / 21.5 ms
 *       (bmsp_spsv 43.7 ms: 3.0x / 2.0x, a gain and no more); R-MAT 2^16 x 8 (254 levels) a sweep 0.39 ms, 4.3 / 6.1 ms against 16.5 ms.
 *       BMSP_SPITSV_CHECK on the band at 2^-10: 199.5 / 134.7 / 120.6 / 138.3 / 255.9 us for 1 / 4 / 8 / 16 / everything at once.
 *   n == 0 returns BMSP_OK without a launch (info: sweeps 0).
 *   Refused with BMSP_ERR_INVALID, the message naming the argument, scalars before handles, nothing done on the device: op, fill or diag
 *   not 0 / 1; max_iter < 0 or > 2^20; tol NaN, or negative and not BMSP_ITSV_NO_CHECK; flags with a bit other than BMSP_ITSV_X0_GIVEN;
 *   delta_history given under BMSP_ITSV_NO_CHECK; null A, d_b, d_x; num_rows != num_cols; row-panel views; d_x == d_b;
 *   BMSP_DIAG_NON_UNIT with a row whose diagonal entry is not stored (bmsp_spsv's message).  BMSP_ERR_LIMIT: as for bmsp_spsv. */
#define BMSP_ITSV_X0_GIVEN 1        /* flags bit 0: d_x holds the initial iterate (default: x^0 = +0, d_x is not read) */
#define BMSP_ITSV_NO_CHECK (-1.0)   /* tol: run exactly max_iter sweeps, nothing read back */
typedef struct { char kernel[64]; int64_t sweeps, levels; int converged; double delta, xmax; } bmsp_spitsv_info;
int bmsp_spitsv(bmsp_matrix_t A, int op, int fill, int diag, double alpha, const void *d_b, void *d_x,
                int64_t max_iter, double tol, int flags, double *delta_history /* host, may be NULL */,
                bmsp_spitsv_info *info /* may be NULL */, void *stream);

/* ILU(0), the incomplete factorisation on A's own pattern, by the fixed-point sweeps of Chow and Patel (SIAM J. Sci. Comput. 37, 2015):
 * the factor that bmsp_spsv / bmsp_spsm / bmsp_spitsv apply, made on the device without a host round trip.  It is to a level-scheduled
 * exact factorisation what bmsp_spitsv is to bmsp_spsv: a sweep is ONE launch in which every stored entry is recomputed independently from
 * the previous iterate -- no level schedule, no dependency chain, nothing waits between workgroups, every value has exactly one writer.
 * Nothing in the reference is replaced (it has no factorisation).
 *   Operands: A is n x n with every diagonal entry (i, i), i < n, stored; F32, F16 or F64; either tile layout.  S = the set of A's stored
 *       coordinates.  F has A's shape, dtype and structure and holds both factors: L (unit diagonal, not stored) in the strict lower
 *       triangle, U in the upper triangle including the diagonal -- exactly what bmsp_spsv(F, N, LOWER, UNIT) followed by bmsp_spsv(F, N,
 *       UPPER, NON_UNIT) applies.  Arithmetic is fp32 for F32 and F16 (F16 values are widened exactly), double for F64.
 *   A sweep computes F^{k+1} from F^k for EVERY (i, j) of S:
 *           s = a_ij
 *           for k ascending over k < min(i, j) with (i, k) in S and (k, j) in S:   s = fma(-f^k_ik, f^k_kj, s)
 *           if i > j:  s = s / f^k_jj          (one IEEE division, the full sequence, never a reciprocal)
 *           f^{k+1}_ij = s rounded once to the storage type (F16: round-to-nearest-even, may overflow)
 *       All reads come from the previous iterate; F^0 = A's values, or F's current values under BMSP_ILU_F0_GIVEN.  Unstored positions
 *       never contribute, a stored 0 does.  Subnormals are kept.  A zero pivot gives what IEEE gives; Inf and NaN travel along
 *       dependencies only.  The arithmetic of a sweep is fixed bit for bit.
 *   Finite termination: entry (i, j) with m = min(i, j) holds its final bits after sweep 2m + 1 when i <= j and after sweep 2m + 2 when
 *       i > j (induction over m: its operands are entries with a smaller min, the diagonal (j, j) included).  So after 2n - 1 sweeps F is
 *       bit for bit the sequential ILU(0) that evaluates the same chain row by row, columns ascending, in place -- the only bitwise fixed
 *       point of the sweep.  max_iter == 0 means 2n.
 *   Per-sweep statistics, order-independent and therefore deterministic (as bmsp_spitsv's): changed = some entry differs in bits from the
 *       previous iterate; delta = max |fl(f^{k+1} - f^k)| and fmax = max |f^{k+1}|, both in the arithmetic type, NaNs skipped.
 *   Stop rule, in the arithmetic type with tol rounded once: stop after sweep k iff !changed || (tol > 0 && delta <= fl(tol * fmax)).
 *       tol == 0 means "until nothing changes".  F, sweeps and converged are a pure function of A's arrays, F^0, tol and max_iter: they
 *       do not depend on the stream, on BMSP_ILU0_LANES or on BMSP_ILU0_CHECK.  An iterate that holds an Inf has delta = fmax = Inf,
 *       which meets the rule under any tol > 0: a caller who stops by tolerance checks that info->delta is finite (where the iteration
 *       does not contract, iterates may grow before finite termination brings the factor back; the call does not detect it).
 *   tol == BMSP_ILU_NO_CHECK, the preconditioner mode (three to five sweeps): exactly max_iter sweeps (2n for 0) by a kernel instantiation
 *       without statistics; nothing is read back and, once F's buffers exist, the call is asynchronous on `stream`.  delta_history must
 *       be NULL; info gets sweeps = max_iter, converged = 0 and delta = fmax = -1.
 *   bmsp_matrix_ilu0: *F is a fresh pool-owned matrix of A's structure with tiles in layout out_transposed; its keys, bitmaps, offsets
 *       and block-row pointer equal bmsp_matrix_convert_layout(A, out_transposed)'s, and it remembers A the way a bmsp_matrix_scale or
 *       bmsp_spgemm_masked output does.  Making it synchronises `stream`.
 *   bmsp_matrix_ilu0_values: the same sweeps into an existing F, which must have been made from A by bmsp_matrix_ilu0 or by one of the
 *       layout-keeping makers (bmsp_matrix_convert_layout, bmsp_matrix_scale, bmsp_sddmm, bmsp_spgemm_masked) while A's STRUCTURE has not
 *       changed since (the rule of bmsp_spgemm_masked_values); F == A is refused, a is read in every sweep.  With BMSP_ILU_F0_GIVEN the
 *       sweeps start from F's current values: the warm start after a value-only update of A, which needs no bmsp_matrix_invalidate.
 *       Without the flag F's values are not read -- whatever they held, NaN included, never reaches the result.  Drops F's value-derived
 *       caches before writing, as bmsp_spgemm_masked_values does.
 *   A, its four arrays and its caches are never modified.
 *   Results: delta_history (host, may be NULL): delta_history[k], k < sweeps, = sweep k's delta, widened exactly.  info (may be NULL):
 *       the kernel instantiation by name ("ilu0_sweep_kernel<F32, 8, STATS>": dtype, lanes per tile, STATS / NO_STATS; "none (empty
 *       matrix)"), the lanes per tile, sweeps = the sweeps that ran, max_sweeps = the cap that applied, converged = the stop rule held at
 *       sweep `sweeps`, the last sweep's delta and fmax, and view_bytes = the bytes of F's op-T view plus its diagonal index.
 *   Kernel (vector ALU): ilu0_sweep_kernel, modelled on spgemm_masked_kernel.  1 or 8 lanes per tile (BMSP_ILU0_LANES=1/8, read per call;
 *       default eight at every fill, the measured choice of the masked product).  A lane owns one byte of the output bitmap with eight
 *       accumulators in registers, started from a_ij.  It walks block-row I of F through F's block-row pointer and block-column J of F
 *       through the cached op-T view of bmsp_spmv_op(F, BMSP_OP_T) (structure only, keyed to F, dropped by the usual events) in ascending
 *       K, stops at K > min(I, J), and in a pair with K == min(I, J) cuts the common-index mask to k < min(i, j) per output position.
 *       Either layout of A and of F is read through the transposed bitmap; the tile order is the same in both.  f^k_jj is read through
 *       a per-structure array of the value index of every (j, j): n 32-bit entries, built once on the device when F's buffers are made
 *       -- that is where a missing diagonal is found --, kept on F's handle, freed and invalidated with the view.  A hub x hub tile
 *       (both lists long, a power-law matrix) is one lane group's serial chain, as in the masked product; it is not split.
 *   Buffers: the iterates ping-pong between F's value array and ONE temporary of nnz storage elements kept on F's handle; the last
 *       iterate ends in F's value array, with at most one asynchronous device copy.  Because of that temporary, calls on one F must not
 *       overlap on different streams.
 *   Statistics and stopping are bmsp_spitsv's protocol: wave and LDS reduction, at most one integer atomic max / or per workgroup and
 *       statistic into the sweep's own record (no floating-point atomic); sweep k + 1 evaluates the stop rule on record k and returns
 *       without writing if it holds; the host enqueues BMSP_ILU0_CHECK=<sweeps> sweeps (read per call, default 8) between read-backs.
 *   n == 0 or a matrix without tiles: a valid empty F, sweeps = 0, kernel "none (empty matrix)".
 *   Refused with BMSP_ERR_INVALID, the message naming the argument, scalars before handles, nothing done on the device: max_iter < 0 or
 *   > 2^20; tol NaN, or negative and not BMSP_ILU_NO_CHECK; out_transposed not 0 / 1; flags with unknown bits; delta_history given under
 *   BMSP_ILU_NO_CHECK; null A, F or out pointer; a non-square A; row-panel views; F not made from A, or F == A; a row whose diagonal
 *   entry is not stored (the message names the first such row, as bmsp_spsv's does).  BMSP_ERR_LIMIT: 2^32 tiles or values or more. */
#define BMSP_ILU_F0_GIVEN 1
#define BMSP_ILU_NO_CHECK (-1.0)
typedef struct { char kernel[64]; int lanes; int64_t sweeps, max_sweeps; int converged; double delta, fmax; int64_t view_bytes; } bmsp_ilu0_info;
int bmsp_matrix_ilu0(bmsp_matrix_t A, int64_t max_iter, double tol, int out_transposed, void *stream,
                     bmsp_matrix_t *F, double *delta_history, bmsp_ilu0_info *info);
int bmsp_matrix_ilu0_values(bmsp_matrix_t A, bmsp_matrix_t F, int64_t max_iter, double tol, int flags, void *stream,
                            double *delta_history, bmsp_ilu0_info *info);

/* Vector primitives of the Krylov solvers below, public because a caller's own iteration needs the same two: a deterministic dot product
 * and a scaled sum.  Vectors are of the library's vector type R: float (vec_f64 == 0) or double (vec_f64 == 1); pointers need the
 * alignment of an element and no more.  Both calls are asynchronous on `stream`; nothing in the reference is replaced.
 *   bmsp_vec_dot: *d_result (a double in DEVICE memory) = sum_i x_i * y_i.  The result is a pure function of x, y and n: it does not
 *       depend on the grid, on scheduling or on the stream, and there is no floating-point atomic.  The order, in full:
 *         - accumulation in double for both vector types (the product of two floats is exact in double);
 *         - the vector is cut into chunks of 1024 consecutive elements; chunk c starts at base = 1024 c;
 *         - in a chunk, lane t of 256 starts with acc = +0 and for q = 0, 1, 2, 3 takes element i = base + 256 q + t: if i < n,
 *           acc = fma((double)x_i, (double)y_i, acc);
 *         - the 64 lanes of a wave (lanes 64 w .. 64 w + 63) are combined by the xor butterfly d = 32, 16, 8, 4, 2, 1 with
 *           acc = acc + acc of lane (t xor d): addition commutes bit for bit, so every lane of the wave ends with the same value W[w];
 *         - the chunk partial is P[c] = ((W[0] + W[1]) + W[2]) + W[3];
 *         - the ceil(n / 1024) partials are combined by ONE workgroup the same way: lane t starts with acc = +0 and adds P[t], P[t + 256],
 *           ... in ascending order with plain additions, then the same butterfly, then the same four-wave sum;
 *         - n == 0 gives +0.
 *       tests/krylov_ref.c restates this order in C.  Up to 384 chunks the second level is run by the workgroup that arrives last at an
 *       integer ticket (its own partial goes out at agent scope and is drained, then the ticket; the last arriver reads every partial at
 *       agent scope; it resets the ticket, so calls follow each other without a memset; nothing waits between workgroups: no flag, no
 *       spin, no cooperative launch).  Beyond 384 chunks it is a launch of its own: the tickets are same-address atomics, about 11 ns each,
 *       and cost more than a launch from about there (interpolated between measurements at 256 and 2048 chunks; DESIGN 4 "Krylov solvers").  BMSP_VEC_DOT_FINISH=ticket|launch (read per call, by
 *       bmsp_krylov_solve too) forces one: the same bits, a measurement switch.  The partials and the ticket live in a scratch per device and stream that grows to
 *       the largest n seen on that stream (growing it synchronises that stream) and is kept for the life of the process: calls on one
 *       stream are ordered by it, calls on different streams share nothing, and the library serialises the enqueueing, so calls from
 *       several threads are safe.
 *   bmsp_vec_axpby: y_i = fl(fl(a * x_i) + fl(b * y_i)), the rule of the epilogues above: a and b are rounded once to R, each
 *       operation is rounded on its own and never contracted; with b == 0 after that rounding y is not read (y_i = fl(a * x_i), a NaN in y
 *       does not propagate).  x == y is legal.
 *   Refused with BMSP_ERR_INVALID: n < 0; vec_f64 not 0 / 1; a null pointer while n > 0 (d_result always). */
int bmsp_vec_dot(int64_t n, int vec_f64, const void *d_x, const void *d_y, double *d_result, void *stream);
int bmsp_vec_axpby(int64_t n, int vec_f64, double a, const void *d_x, double b, void *d_y, void *stream);

/* Block multi-colour ordering and block permutation on the device: what a solver that reorders needs, without the round trip through
 * bmsp_matrix_to_coo_device and a builder.  The level rule of bmsp_spsv counts tiles and ignores bitmaps, so a proper colouring of the
 * block-row graph with every colour class made contiguous gives a matrix whose triangular solves have as many levels as there are
 * colours; bmsp_spsv, bmsp_spsm, bmsp_spitsv, bmsp_matrix_ilu0 and the preconditioners of bmsp_krylov_solve work on it unchanged.  Nothing
 * in the reference is replaced.
 *
 *   bmsp_matrix_color_blocks: the greedy colouring of the block-row graph of a square A (any dtype, either layout; structure only) by
 *       hashed priorities, and the ordering by colour class.  d_colors and d_perm hold nb = ceil(n / 8) entries of DEVICE memory.
 *       Graph: block-rows I != J are neighbours iff a tile (I, J) or a tile (J, I) is stored, whatever its bitmap -- the dependency rule
 *           of bmsp_spsv, symmetrised (a lower-triangular A colours like A + A^T).  The neighbours come from A's own keys and block-row
 *           pointer and from the cached op-T view of bmsp_spmv_op (built if missing, which synchronises `stream`); A + A^T is not formed.
 *       Colours, a pure function of structure and seed: key(I) = (splitmix64(seed ^ I), I) compared lexicographically as unsigned
 *           (splitmix64: z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *           z ^ z >> 31).  color(I) is the smallest c >= 0 that no neighbour with a greater key holds (the sequential greedy colouring in
 *           descending key order); round(I) is 1 without a greater-key neighbour, else 1 + the largest round among them.  A block-row
 *           without tiles or neighbours gets colour 0.  Nothing depends on scheduling, lane counts or the stream.
 *       info (may be NULL): kernel = "color_round_kernel<8 lanes>" ("none (empty matrix)" for n = 0); blocks = nb; colors = 1 + the
 *           largest colour (0 for n = 0); rounds = the largest round; view_bytes = the op-T view's size.
 *       d_perm (may be NULL), new -> old: the block-rows sorted by (class, index), classes in ascending colour order.  When n % 8 != 0
 *           the class of the trailing partial block-row goes last (that block-row is then last within it), which keeps the permuted matrix
 *           n x n.  The triangles of bmsp_matrix_permute_blocks(A, d_perm, d_perm) then have at most `colors` levels, exactly `colors`
 *           when n % 8 == 0 and A's block pattern is symmetric (a tile (J, I) for every tile (I, J): a block-row of colour c has a
 *           neighbour of every smaller colour in front of it, which is a dependency only where the tile lies in that triangle).
 *       Kernel (Jones-Plassmann; vector ALU): one launch per round, eight lanes per block-row.  A block-row is coloured in round k iff
 *           every greater-key neighbour carries the stamp of a round before k; a colour written in the current launch reads as
 *           "uncoloured".  No waiting between workgroups: no flag, no spin, no cooperative launch.  The smallest free colour is found in
 *           windows of 64 colours (a 64-bit mask ORed over the neighbours; first zero bit; a full mask moves the window).  The block-rows
 *           left uncoloured are counted per round by integer atomics (one per workgroup); a launch that finds the count of the round before
 *           at 0 returns at once.  The host enqueues BMSP_COLOR_CHECK rounds (default 16, read per call), reads the counts back and stops
 *           at the first 0: the switch decides how much is enqueued ahead, never the result.  At most nb rounds are run, since every
 *           round colours the greatest remaining key; passing that bound returns BMSP_ERR_INTERNAL.  Synchronises `stream`.
 *       Refused with BMSP_ERR_INVALID, the message naming the argument: null A or d_colors; a non-square A; a row-panel view.
 *       BMSP_ERR_LIMIT: as for bmsp_spsv.
 *
 *   bmsp_matrix_permute_blocks: out = P * A * Q^T at tile granularity, a fresh pool-owned handle with its tiles in layout out_transposed:
 *       block (I', J') of out is block (d_row_perm[I'], d_col_perm[J']) of A -- the gather convention A[p][:, q], the one d_perm above
 *       follows; NULL = the identity.  Any dtype, rectangular A, either input and either output layout; dimensions, nnz and the tile
 *       count are A's; the four arrays equal, bit for bit, what the builders make from the permuted COO.  Values move as raw bits; A and
 *       its caches are untouched.  Passes: the inverses of the permutations; the new key per tile; a stable radix sort over the new
 *       key's bits with the source tile as payload (new rows alone: the row bits only -- the input is in (row, column) order; new
 *       columns need both halves; neither: no sort); one scan that writes bitmaps and offsets; the value move of bmsp_matrix_transpose
 *       (bitmaps transposed and values permuted inside tiles exactly when out_transposed differs from A's layout).  No COO round
 *       trip, no atomics outside the check.  bmsp_matrix_copy_values(A, out) replays a value-only update of A.
 *       Checked on the device before anything is built (scatter marks and a count, one 8-byte read-back; no index is used unchecked):
 *       each given array is a permutation of [0, block count), and when the dimension is not a multiple of 8 the last block maps to
 *       itself; otherwise BMSP_ERR_INVALID naming the argument, and *out is left untouched.  Also refused: null A or out;
 *       out_transposed not 0 / 1; row-panel views.  BMSP_ERR_LIMIT: as for bmsp_matrix_transpose.  Runs on `stream` and synchronises
 *       it: at the read-back of the check and before it returns (the sort temporaries go back to the pool).
 *
 *   bmsp_vec_permute_blocks: the vectors that go with it, float (vec_f64 == 0) or double (1), d_perm of ceil(n / 8) entries.
 *       inverse == 0: y[8 i + r] = x[8 perm[i] + r] (b' = P b); inverse == 1: y[8 perm[i] + r] = x[8 i + r] (x = P^T x'); both for
 *       8 i + r < n and 8 perm[i] + r < n, other entries of y are not written.  Asynchronous on `stream`, nothing is read back.  The
 *       permutation is not validated: an entry perm[i] >= ceil(n / 8) is skipped, and no access outside [0, n) of x or y is ever made.
 *       Refused with BMSP_ERR_INVALID: n < 0; vec_f64 or inverse not 0 / 1; while n > 0, a null pointer or d_x == d_y. */
typedef struct { char kernel[64]; int64_t blocks, colors, rounds, view_bytes; } bmsp_color_info;
int bmsp_matrix_color_blocks(bmsp_matrix_t A, uint64_t seed, uint32_t *d_colors, uint32_t *d_perm /* may be NULL */,
                             void *stream, bmsp_color_info *info /* may be NULL */);
int bmsp_matrix_permute_blocks(bmsp_matrix_t A, const uint32_t *d_row_perm /* NULL = identity */,
                               const uint32_t *d_col_perm /* NULL = identity */, int out_transposed, void *stream, bmsp_matrix_t *out);
int bmsp_vec_permute_blocks(int64_t n, int vec_f64, const uint32_t *d_perm, int inverse, const void *d_x, void *d_y, void *stream);

/* Aggregation for algebraic multigrid on the device: the two stages of a smoothed-aggregation set-up that are neither a product, a sum,
 * a scaling, a pruning nor a transpose -- partitioning the nodes of a strength graph into aggregates, and building the tentative
 * prolongator from an aggregate map.  Nothing in the reference is replaced.
 *
 *   bmsp_matrix_aggregate: MIS(2) aggregates of the graph of a square S (any dtype, either layout).  Only S's structure is read: a stored
 *       zero counts, values are never loaded; S and its caches are otherwise untouched.  d_agg holds n = num_rows entries of DEVICE memory.
 *       Graph: the nodes are the scalar rows 0 .. n - 1 (not block-rows); i != j are neighbours iff (i, j) or (j, i) is stored.  The row
 *           direction comes from S's keys, bitmaps and block-row pointer, the column direction from the cached op-T view of bmsp_spmv_op
 *           (built if missing, which synchronises `stream`); S + S^T is not formed, so a strictly lower-triangular pattern aggregates
 *           exactly like its symmetrisation.  Nothing is cached on the handle: the scratch is per call, from the pool.
 *       Keys: key(i) = (splitmix64(seed ^ i) >> 32, i), compared lexicographically as unsigned (splitmix64 as for
 *           bmsp_matrix_color_blocks above); the index half makes keys unique.
 *       Roots: the maximal distance-2 independent set that the sequential greedy gives in descending key order -- i becomes a root iff
 *           no node already chosen lies within distance <= 2 of it.  Distance is taken in the whole graph: a path through a decided node
 *           counts.  The roots depend on nothing but structure and seed.
 *       Aggregates: a root's id is its rank among the roots in ascending node index (one exclusive scan).  A non-root with a root among
 *           its neighbours joins the neighbouring root of greatest key; every other node joins the root of greatest key among the roots
 *           its neighbours are adjacent to (one exists, by maximality).  A node without neighbours is a root and a singleton.
 *           *num_aggregates (host) is the number of roots; every d_agg[i] is below it.
 *       Kernels (vector ALU; no floating-point atomic, no flag, no spin, no cooperative launch): one template, agg_pass_kernel, takes the
 *           maximum of a per-node 8-byte word over the closed neighbourhood -- eight lanes per block-row, a lane per scalar row; the lanes
 *           walk the block-row's tiles together, each taking its byte of every bitmap (layout 0) or its bit of every byte (layout 1),
 *           then the view's records for the column direction the other way round; every set bit is one gather.  It serves the first- and
 *           second-level passes of a round, the root-propagation pass and the final assignment, which propagates the greatest root key
 *           instead of a flag.
 *       Schedule: fixed-priority Luby rounds of TWO launches.  The first takes, for every node whatever its state, the greatest
 *           undecided key in its closed neighbourhood, a root reading as "all ones".  The second, for every undecided node, takes the
 *           maximum of those: all ones eliminates the node (a root within distance 2), its own key makes it a root, anything else leaves
 *           it undecided.  Elimination therefore lags one round behind selection; this delays selections and never changes them.
 *           `rounds` is the number of rounds that decided at least one node, which is every round run, the last one (eliminations
 *           only) included.  BMSP_AGG_SCHEDULE=separate (a measurement switch, read per call) selects and eliminates in rounds of four
 *           launches instead: the same roots and aggregates, another `rounds`; measured, it takes as many launches and as long.
 *       Termination (bmsp_spitsv's protocol): every round records the nodes left undecided by integer atomics, one per workgroup; the
 *           launches of the next round return at once when that is 0.  The host enqueues BMSP_AGG_CHECK rounds (default 8, at most 1024,
 *           read per call) between read-backs; the switch never changes d_agg, *num_aggregates or `rounds`.
 *       info (may be NULL): kernel = "agg_pass_kernel<layout 0>" / "<layout 1>" ("none (empty matrix)" for n = 0); nodes = n;
 *           aggregates; rounds; launches = the kernels that did work (1 for the keys, 2 per round, the scan counted once, 2 for the
 *           assignment); view_bytes = the op-T view's size.
 *       Refused with BMSP_ERR_INVALID, the message naming the argument, nothing done on the device: null S, d_agg or num_aggregates; a
 *       non-square S; a row-panel view.  BMSP_ERR_LIMIT: as for bmsp_spsv, and n beyond 2^32 - 2 (the node words).  Runs on `stream`
 *       and synchronises it.
 *
 *   bmsp_matrix_from_aggregates: a fresh pool-owned num_rows x num_aggregates matrix P with P[i, d_agg[i]] = w_i, one stored entry per
 *       row, tiles in layout `transposed`.  d_agg[i] == 0xFFFFFFFF leaves row i empty (how a caller drops nodes).  d_weights (NULL = ones)
 *       has the vector type: float for BMSP_F16 / BMSP_F32, double for BMSP_F64, converted as the builder converts.  The four arrays and
 *       the block-row pointer equal, bit for bit, what bmsp_matrix_from_coo_device builds from (i, d_agg[i], w_i) in that layout.
 *       Construction, direct (no sort, no COO builder): per block-row eight lanes order their eight d_agg >> 3 inside the group and mark
 *           the distinct ones; one scan of the packed (tiles, entries) counts gives the tile and value offsets; one pass writes keys,
 *           bitmaps, offsets, values and the block-row pointer.  The builder orders tiles by (block-row, block-column) in both layouts
 *           -- only the positions inside a tile differ -- so neither layout pays for a sort.
 *       Checked on the device before anything is built (the flag comes back with the scan's totals in one 16-byte read-back): every entry
 *       is below num_aggregates or the skip value; otherwise BMSP_ERR_INVALID naming d_agg, and *out is left untouched.  Also refused:
 *       negative sizes; a null d_agg while num_rows > 0; a null out; `transposed` not 0 / 1; an unknown dtype.  Synchronises `stream`. */
typedef struct { char kernel[64]; int64_t nodes, aggregates, rounds, launches, view_bytes; } bmsp_aggregate_info;
int bmsp_matrix_aggregate(bmsp_matrix_t S, uint64_t seed, uint32_t *d_agg /* n entries, device */,
                          int64_t *num_aggregates /* host */, void *stream, bmsp_aggregate_info *info /* may be NULL */);
int bmsp_matrix_from_aggregates(int num_rows, int num_aggregates, const uint32_t *d_agg, const void *d_weights /* NULL = ones */,
                                bmsp_dtype dtype, int transposed, void *stream, bmsp_matrix_t *out);

/* Krylov solvers on the device: op(A) x = b for a square A in EITHER tile layout by preconditioned conjugate gradients (A symmetric
 * positive definite) or BiCGStab (van der Vorst's preconditioned form), with the whole iteration enqueued on `stream` -- products,
 * preconditioner, dot products, vector updates and the scalars alpha, beta, omega, which never leave the device.  Nothing in the reference
 * is replaced (it has no solver).
 *   Operands: A is F32 or F64 (an F16 A is BMSP_ERR_UNSUPPORTED: the product's input vector would be fp16, and a Krylov basis in fp16 is
 *       not this call); b and x are n vector elements of type R (float for F32, double for F64).  Every product is bmsp_spmv_op(A, op, 1, .,
 *       0, .): no conversion, no second matrix.  A, b and the factor are not modified (their caches are built if missing).
 *   Preconditioner z = M^-1 r (pc == NULL is BMSP_PC_NONE): BMSP_PC_JACOBI divides by the diagonal, one IEEE division per row, the diagonal
 *       taken with bmsp_matrix_diagonal per call (a zero or unstored diagonal is not refused: IEEE gives Inf or NaN and the solve ends in
 *       BMSP_KRYLOV_BREAKDOWN).  BMSP_PC_ILU_EXACT applies pc->F, a factor as bmsp_matrix_ilu0 makes it (L unit lower, U upper, either
 *       layout), by two bmsp_spsv: (LOWER, UNIT) then (UPPER, NON_UNIT) under op N; under op T the transposed factors in the other order,
 *       bmsp_spsv(F, T, UPPER, NON_UNIT) then (F, T, LOWER, UNIT).  BMSP_PC_ILU_SWEEPS: the same two solves by bmsp_spitsv with exactly
 *       pc->sweeps sweeps each under BMSP_ITSV_NO_CHECK.  F is F64 for an F64 A and F32 or F16 for an F32 A (an F16 factor takes float
 *       vectors in the solves).
 *   Arithmetic, fixed operation by operation, so that x, iterations, status and the history are a pure function of the inputs wherever
 *       the product is one (bmsp_spmv_op's view cases: op T, column-major A): dots are bmsp_vec_dot's; alpha, beta and omega are doubles
 *       formed by one IEEE division each and rounded once to R (aR, bR, wR) before they touch a vector; every vector update is a separately
 *       rounded multiply and a separately rounded add or subtract, never contracted.  bb = dot(b, b); thr = fl(fl(tol * tol) * bb) in double; a
 *       residual with rr = dot(r, r) stops the iteration iff rr <= thr.  relres = sqrt(rr / bb) is formed on the host.  bb == 0: x = 0,
 *       BMSP_KRYLOV_CONVERGED after 0 iterations.  x0 = +0 and d_x is not read, unless BMSP_KRYLOV_X0_GIVEN is set: then r = fl(b - op(A) x0),
 *       one product more.  The initial residual is held to the same rule (rr0 = bb without x0): a start that already meets it returns
 *       CONVERGED with 0 iterations.
 *   CG: z = M^-1 r; p = z; rho = dot(r, z).  Iteration: q = op(A) p; alpha = rho / dot(p, q); x = fl(x + fl(aR * p)); r = fl(r - fl(aR * q));
 *       rr = dot(r, r): record, stop?; z = M^-1 r; rho' = dot(r, z); beta = rho' / rho; rho = rho'; p = fl(z + fl(bR * p)).
 *   BiCGStab: rh = r; rho' = dot(rh, r).  Iteration k: if k = 1 p = r, else beta = fl(fl(rho' / rho) * fl(alpha / omega)) and p = fl(r +
 *       fl(bR * fl(p - fl(wR * v)))); rho = rho'; ph = M^-1 p; v = op(A) ph; alpha = rho / dot(rh, v); s = fl(r - fl(aR * v)); x = fl(x +
 *       fl(aR * ph)); if dot(s, s) <= thr: record it, converged.  sh = M^-1 s; t = op(A) sh; omega = dot(t, s) / dot(t, t); x = fl(x + fl(wR *
 *       sh)); r = fl(s - fl(wR * t)); rr = dot(r, r): record, stop?; rho' = dot(rh, r).
 *       What the definitions allow is fused: the x and r updates with the partial sums of the dots that follow them, under Jacobi the
 *       division too, and with BMSP_PC_NONE rho' IS rr (the same function of the same vector).  The bits are those of the unfused text.
 *   Breakdown: a denominator (dot(p, q); dot(rh, v); dot(t, t); rho, checked when it is formed; omega, checked when it is formed) that is 0
 *       or not finite, or a residual dot that is not finite -- or 0 where that is not convergence, under BMSP_KRYLOV_NO_CHECK -- ends the
 *       solve with status BMSP_KRYLOV_BREAKDOWN.  It is a result, not an error: the call returns BMSP_OK.  x keeps the last iterate
 *       WRITTEN, which is not always the last completed one: dot(p, q), dot(rh, v) and rho are checked before the update they would
 *       scale, so x is then the iterate of the iteration before; BiCGStab's dot(t, t) and omega are checked after the half step x = fl(x +
 *       fl(aR * ph)) has been applied, so x then holds that half step; a residual dot is checked after the update that produced it, so a
 *       non-finite rr or dot(s, s) leaves the x it belongs to, which may itself hold non-finite values.  (Keeping the last completed
 *       iterate instead would cost a second copy of x or one more launch per iteration; a caller who needs it keeps its own copy.)
 *   Limits and modes: max_iter == 0 means min(n, 2^20).  tol == BMSP_KRYLOV_NO_CHECK, the inner-solver mode: exactly max_iter iterations
 *       unless a breakdown stops them on the device; nothing is read back, relres_history must be NULL, info gets iterations = max_iter,
 *       status = BMSP_KRYLOV_MAXITER, relres = bnorm = -1 and the products and applications of a full run.
 *   Device-resident protocol, bmsp_spitsv's adapted: the scalars, the status and one record per iteration live in device memory; every
 *       kernel of the solver begins by reading the status and returns without writing once the solve has stopped.  The host enqueues
 *       BMSP_KRYLOV_CHECK=<iterations> iterations (read per call) between two read-backs of the records and decides by the same
 *       predicate; without the variable the batches are 1, 2, 4, 8, then 16 iterations each.  The library calls in between (bmsp_spmv_op, bmsp_spsv, bmsp_spitsv) cannot return early: after a stop up to CHECK - 1
 *       iterations of them run on unchanged vectors of the workspace and are wasted -- the trade the default is measured for: a solve
 *       of one or two iterations with a costly preconditioner wants 1, a solve of hundreds 8 - 16, and the ramp serves both.  x,
 *       iterations, status and the history never depend on BMSP_KRYLOV_CHECK or on the stream.
 *   Results: x in d_x.  relres_history (host, may be NULL, max_iter entries or min(n, 2^20)): [k] = sqrt(rr_k / bb) of iteration k + 1, k <
 *       iterations.  info (may be NULL): method by name ("cg" / "bicgstab" + "+none" / "+jacobi" / "+ilu" / "+ilu_sweeps"), the
 *       iterations completed (each left a record), the cap that applied, the status, relres of the last record (of the initial
 *       residual after 0 iterations), bnorm = sqrt(bb), the products and preconditioner applications whose results the solve consumed,
 *       and the bytes of the workspace.
 *   Workspace, kept on A's handle: 4 vectors for CG, 8 for BiCGStab, the diagonal, the dot partials, the scalars and the records,
 *       sized for the largest need seen (growing it synchronises `stream`), freed with the handle and by bmsp_matrix_invalidate(A, 1).  One
 *       stream per handle at a time, as for bmsp_spitsv (A's and F's).  Plans and views are built on first use by the calls that own them;
 *       those builds synchronise.  After that a NO_CHECK call is fully asynchronous, and a checked call synchronises once for bb and
 *       once per batch.
 *   Refused with BMSP_ERR_INVALID, the message naming the argument, scalars before handles, nothing done on the device: op or method not
 *   0 / 1; an unknown pc->kind; sweeps < 1 under BMSP_PC_ILU_SWEEPS; max_iter < 0 or > 2^20; tol NaN, or negative and not
 *   BMSP_KRYLOV_NO_CHECK; flags with unknown bits; relres_history given under BMSP_KRYLOV_NO_CHECK; null A, d_b or d_x; d_x == d_b; a
 *   non-square A; row-panel views; an ILU kind with a null F, with F's shape different from A's, or with an F dtype outside the rule
 *   above.  A missing diagonal of F is refused by bmsp_spsv's own message.  BMSP_ERR_UNSUPPORTED: an F16 A. */
#define BMSP_KRYLOV_CG 0
#define BMSP_KRYLOV_BICGSTAB 1
#define BMSP_PC_NONE 0
#define BMSP_PC_JACOBI 1        /* z = r / diag(A), one IEEE division per row; the diagonal is taken with bmsp_matrix_diagonal per call */
#define BMSP_PC_ILU_EXACT 2     /* z = U^-1 L^-1 r by two bmsp_spsv on F (F from bmsp_matrix_ilu0: L unit lower, U upper) */
#define BMSP_PC_ILU_SWEEPS 3    /* the same two solves by bmsp_spitsv, exactly `sweeps` sweeps each, BMSP_ITSV_NO_CHECK */
typedef struct { int kind; bmsp_matrix_t F; int64_t sweeps; } bmsp_precond;
#define BMSP_KRYLOV_X0_GIVEN 1
#define BMSP_KRYLOV_NO_CHECK (-1.0)
#define BMSP_KRYLOV_MAXITER 0
#define BMSP_KRYLOV_CONVERGED 1
#define BMSP_KRYLOV_BREAKDOWN 2
typedef struct { char method[32]; int64_t iterations, max_iterations; int status; double relres, bnorm;
                 int64_t products, precond_applies, workspace_bytes; } bmsp_krylov_info;
int bmsp_krylov_solve(bmsp_matrix_t A, int op, int method, const bmsp_precond *pc /* NULL = none */, const void *d_b, void *d_x,
                      int64_t max_iter, double tol, int flags, double *relres_history /* host, may be NULL */,
                      bmsp_krylov_info *info /* may be NULL */, void *stream);

/* Restarted GMRES on the device: op(A) x = b for a square A in either tile layout by right-preconditioned GMRES(m), m = restart (0 means
 * 30, at most 256), with the whole iteration enqueued on `stream` as in bmsp_krylov_solve.  One product and one preconditioner application
 * per iteration (plus one product per restart), a residual that never grows, and no rho / omega recurrence to break down: the method for
 * matrices that are not symmetric.  Nothing in the reference is replaced (it has no solver).
 *   Carried over from bmsp_krylov_solve, word for word: the operands, the preconditioner kinds and their op-T order, max_iter == 0,
 *       BMSP_KRYLOV_NO_CHECK, BMSP_KRYLOV_X0_GIVEN, the BMSP_KRYLOV_CHECK ramp, the refusals (scalars before handles, the message naming
 *       the argument), bmsp_precond, bmsp_krylov_info and every define.  New: restart < 0 or restart > 256 is refused, the message
 *       naming restart.
 *   Arithmetic, fixed operation by operation.  R is the vector type; scalars are doubles on the device; a scalar is rounded once to R
 *       (suffix R) before it touches a vector; nothing is contracted; dots are bmsp_vec_dot's.
 *       Start: exactly bmsp_krylov_solve's -- bb, thr, bb == 0, x0, r = fl(b - op(A) x0) and the rule for the initial residual.
 *       Cycle start: the residual is r and rr = dot(r, r).  From the second cycle on rr is tested: not finite: BMSP_KRYLOV_BREAKDOWN; rr <=
 *           thr: BMSP_KRYLOV_CONVERGED, with no record added and info->relres reporting this rr; under BMSP_KRYLOV_NO_CHECK rr == 0:
 *           BMSP_KRYLOV_BREAKDOWN.  Then beta = sqrt(rr), s = 1.0 / beta, v_0 = fl(sR * r), g_0 = beta.
 *       Step j = 0 .. m - 1 (iteration k): z_j = M^-1 v_j (z_j is v_j without a preconditioner); w = op(A) z_j.  Two passes p = 1, 2 of
 *           classical Gram-Schmidt: t_i = dot(v_i, w) for i = 0 .. j, all taken of the same w; then per element, for i ascending,
 *           w = fl(w - fl(tR_i * v_i)).  h_i = the first pass's t_i + the second pass's t_i, one add; h_{j+1} = sqrt(dot(w, w)).  A t or h that is not
 *           finite: BMSP_KRYLOV_BREAKDOWN.  The earlier rotations i < j in ascending order, on (a, b) = (h_i, h_{i+1}): h_i = fl(fl(c_i a) +
 *           fl(s_i b)), h_{i+1} = fl(fl(c_i b) - fl(s_i a)).  The new rotation: d = sqrt(fl(fl(h_j h_j) + fl(h_{j+1} h_{j+1}))) (not hypot); d
 *           zero or not finite: BMSP_KRYLOV_BREAKDOWN; c_j = h_j / d, s_j = h_{j+1} / d, h_j = d; g_{j+1} = -fl(s_j g_j), g_j = fl(c_j g_j).
 *           rr_k = fl(g_{j+1} g_{j+1}) is recorded; then not finite: BMSP_KRYLOV_BREAKDOWN; rr_k <= thr: BMSP_KRYLOV_CONVERGED; under
 *           BMSP_KRYLOV_NO_CHECK rr_k == 0: BMSP_KRYLOV_BREAKDOWN; k == max_iter ends the solve with BMSP_KRYLOV_MAXITER.  Otherwise, for j < m
 *           - 1, v_{j+1} = fl(sR * w) with s = 1.0 / h_{j+1}.
 *       End of a cycle with J columns completed (m, or fewer when the rule or the cap stopped it): the back substitution in double, for i =
 *           J - 1 .. 0: s = g_i; for l = i + 1 .. J - 1 ascending s = fl(s - fl(U_il y_l)); y_i = s / U_ii (U the rotated columns).  Then per
 *           element, for i ascending, x = fl(x + fl(yR_i * z_i)).  On BMSP_KRYLOV_BREAKDOWN x is NOT updated from the partial cycle: it keeps
 *           the iterate of the last completed cycle, which is the last iterate written.  If the solve goes on: r = fl(b - op(A) x), rr =
 *           dot(r, r).
 *       What the definitions allow is fused (the update of the second pass carries the partial sums of dot(w, w)); the bits are those
 *       of the text.  x, iterations, status and the history are a pure function of the inputs wherever the product is one.
 *   Kernels: one launch forms up to BMSP_GMRES_GROUP=<vectors> (1 .. 16, read per call; default 8) of the dots t_i from one read of w, each
 *       with bmsp_vec_dot's tree, second level by ticket up to 384 chunks and by a launch beyond (BMSP_VEC_DOT_FINISH is honoured); one
 *       launch applies all of them.  The group never changes the bits.
 *   Device-resident protocol: bmsp_krylov_solve's.  Every kernel reads the status first and returns without writing once the solve has
 *       stopped, except the formation of x for the cycle the stop fell into, which still happens, once.  x, iterations, status and the
 *       history never depend on BMSP_KRYLOV_CHECK, on BMSP_GMRES_GROUP or on the stream.  A BMSP_KRYLOV_NO_CHECK call reads nothing back.
 *   Results: as bmsp_krylov_solve.  relres_history[k] = sqrt(rr_{k+1} / bb).  info->method is "gmres(<m>)+none" / "+jacobi" / "+ilu" /
 *       "+ilu_sweeps"; products = the iterations plus the restarts performed (plus one with x0); precond_applies = the iterations (0 for
 *       none).
 *   Workspace: the one bmsp_krylov_solve keeps on A's handle, grown by the same rule: m' + 1 basis vectors with m' = min(m, max_iter), m' vectors
 *       z_j when there is a preconditioner, one vector between the two solves of the ILU kinds, the diagonal, the rotated Hessenberg columns, the
 *       rotations, g, y, the dots, the dot partials and the records. */
int bmsp_gmres_solve(bmsp_matrix_t A, int op, const bmsp_precond *pc /* NULL = none */, int restart /* 0 = 30 */,
                     const void *d_b, void *d_x, int64_t max_iter, double tol, int flags, double *relres_history,
                     bmsp_krylov_info *info, void *stream);

/* Multigrid on the device: the V-cycle of a hierarchy the caller supplies (pybmsp/amg.py's smoothed aggregation, a geometric one, any),
 * enqueued on a stream like the rest of bmsp_krylov_solve, and CG / BiCGStab for A[0] * x = b preconditioned by one cycle.  The cycle is
 * not a `kind` of bmsp_krylov_solve (bmsp_precond is fixed): it has its own handle and its own solve.  Nothing in the reference is
 * replaced (it has no solver).
 *   Operands: A[l] is square, n_l x n_l, F32 or F64, all of one dtype (F16: BMSP_ERR_UNSUPPORTED, as in bmsp_krylov_solve); P[l] is n_l x
 *       n_{l+1}; R[l] is n_{l+1} x n_l, and R == NULL or R[l] == NULL restricts by P[l]^T.  Every operator may be in either tile layout,
 *       independently of the others: tiles are in (block-row, block-column) order in both, so no view and no conversion is made.
 *       d_coarse_inv (may be NULL) is the dense inverse of A[levels - 1], n_c x n_c row-major with leading dimension ld_inv >= n_c, of
 *       the vector type R (float for F32, double for F64), n_c <= 4096.
 *   The handle borrows the matrices (the caller keeps them alive; their values are read at every cycle) and owns a copy of every level's
 *       diagonal, taken with bmsp_matrix_diagonal at create (a value update of A means a new handle), a copy of the coarse inverse stored
 *       column by column (one lane per row: the lanes' loads coalesce) and the per-level work vectors.  bmsp_mg_create synchronises
 *       `stream`; d_coarse_inv may go when it returns.
 *   Arithmetic, fixed operation by operation (tests/multigrid_ref.c restates it).  Nothing is contracted except the named fma.  wR is
 *       omega rounded once to R; d_i is the stored diagonal entry of the level's A, or +0 if none is stored.
 *       rowchain(M, init, +-, v)_i: s = init_i, then for the stored entries (i, j) of row i in ascending j s = fma(+-m_ij, v_j, s) -- one
 *           fused multiply-add per stored entry in column order, the convention of bmsp_spsv.
 *       residual:     t = rowchain(A, r, -, x).
 *       Jacobi step:  x'_i = fl(x_i + fl(wR * fl(s_i / d_i))) with s the residual chain, out of place (two buffers).  The first step from
 *           x = 0 is x_i = fl(wR * fl(r_i / d_i)), an element-wise launch with no walk.  With pre == 0, x = 0 and t = r.
 *       restriction:  rc = rowchain(R, +0, +, t) in row mode; bmsp_spmv_op(R, N, 1, t, 0, rc) in spmv mode; bmsp_spmv_op(P, T, 1, t, 0, rc)
 *           where R is NULL.
 *       prolongation: x_i = rowchain(P, x, +, e): the add is the start of the chain.
 *       coarsest level with the inverse: s = +0, then for j = 0 .. n_c - 1 s = fma(inv_ij, r_j, s).  Without it: pre + post Jacobi steps
 *           from zero.
 *       recursion:    level l runs `pre` steps, the residual, the restriction, the cycle of level l + 1 for rc, the prolongation of its
 *           result e, `post` steps.  Rows at or beyond n_l are never read or written.
 *       How a block-row is walked is the library's choice per operator, a function of its structure alone (eight lanes per block-row
 *       with one or four tiles in flight, or a wave per block-row whose eight lane groups gather eight tiles and pass the running sum
 *       from group to group in tile order; BMSP_MG_WALK=group1|group4|wave forces one, read per call): the chain of a row is the same in
 *       all of them, term by term, and so are the bits.
 *       In row mode the cycle is therefore a pure function of its inputs: it does not depend on the grid, on scheduling or on the
 *       stream, and uses no atomic, no flag, no spin and no LDS.  A zero or unstored diagonal is not refused: IEEE gives Inf or NaN
 *       (BMSP_PC_JACOBI's rule) and a solve ends in BMSP_KRYLOV_BREAKDOWN.
 *   Restriction mode per level: BMSP_MG_RESTRICT=row|spmv (read per call) forces one; the default is a function of R[l]'s structure
 *       alone -- row mode up to 24 tiles per block-row of R[l] in the mean, spmv mode beyond (bmsp_spmv_op splits long block-rows and
 *       sums in another order; the two were measured to cross there) -- and bmsp_mg_info reports it.  row gives the fixed bits above, spmv gives bmsp_spmv_op's.
 *       Prolongation always takes the row kernel.
 *   bmsp_mg_vcycle: z = one cycle for right-hand side r from z = 0 (d_z must not be d_r), asynchronous on `stream`, nothing read back.
 *       One stream per handle at a time.  A first call that has to build a view for bmsp_spmv_op synchronises, as everywhere else.
 *       n_0 == 0 is legal: the cycle does nothing.  bmsp_mg_free does not synchronise (bmsp_matrix_free does not either): the caller lets
 *       what it enqueued on the handle finish first.
 *   bmsp_mg_solve: bmsp_krylov_solve(A[0], BMSP_OP_N, method, ...) with z = M^-1 r one cycle -- its arithmetic, stop rule, breakdown
 *       rules, BMSP_KRYLOV_CHECK ramp, BMSP_KRYLOV_NO_CHECK mode, BMSP_KRYLOV_X0_GIVEN, history, info and refusals; in CG the cycle is
 *       followed by rho' = dot(r, z), in BiCGStab it stands where the ILU kinds stand.  info->method is "cg+mg" or "bicgstab+mg",
 *       precond_applies counts cycles.  The workspace lives on A[0]'s handle.  The kernels of the cycle read the solver's status word
 *       first and return without writing once the solve has stopped; only the bmsp_spmv_op calls of an iteration enqueued behind a stop
 *       still run (the iterate of a level without a pre-smoothing step is zeroed by such a kernel too, not by a memset).  The views
 *       bmsp_spmv_op needs for the restriction -- (P, T), or (R, N) of a column-major R in spmv mode -- are built before the first
 *       iteration is enqueued.  CG needs a symmetric cycle: R = P^T (R NULL, or the transposes given) and pre == post; BiCGStab takes any.  n_0 == 0
 *       returns BMSP_KRYLOV_CONVERGED after 0 iterations.
 *   bmsp_mg_info: the levels, n per level, the restriction mode per level (BMSP_MG_RESTRICT_*; -1 on the coarsest), the kernel names,
 *       the bytes the handle owns and the launches of one cycle (a bmsp_spmv_op call counts as one).
 *   Refused with BMSP_ERR_INVALID, the message naming the argument, scalars before handles, nothing done on the device: levels outside
 *   1 .. 16; omega not finite; pre or post outside 0 .. 16; pre + post == 0 on a level that has no exact solve; a null out, A, P (levels >
 *   1) or entry of them; shapes that do not chain; mixed dtypes; row-panel views; n_c > 4096 with an inverse; ld_inv < n_c; for the
 *   cycle a null handle or vector, d_z == d_r; for the solve what bmsp_krylov_solve refuses. */
#define BMSP_MG_MAX_LEVELS 16
#define BMSP_MG_RESTRICT_ROW 0
#define BMSP_MG_RESTRICT_SPMV 1
#define BMSP_MG_RESTRICT_PT 2   /* R[l] is NULL: bmsp_spmv_op(P[l], T) */
typedef struct bmsp_mg_s *bmsp_mg_t;
typedef struct { int levels, pre, post, coarse_exact; int64_t n[BMSP_MG_MAX_LEVELS]; int restrict_mode[BMSP_MG_MAX_LEVELS];
                 char kernel[64], coarse_kernel[64]; int64_t workspace_bytes, launches_per_cycle; } bmsp_mg_info_t;
int bmsp_mg_create(int levels, const bmsp_matrix_t *A /* levels */, const bmsp_matrix_t *P /* levels-1 */,
                   const bmsp_matrix_t *R /* levels-1; NULL or NULL entries: restrict by P^T */,
                   const void *d_coarse_inv /* n_c x n_c row-major, vector type; may be NULL */, int64_t ld_inv,
                   double omega, int pre, int post, void *stream, bmsp_mg_t *out);
int bmsp_mg_free(bmsp_mg_t mg);
int bmsp_mg_info(bmsp_mg_t mg, bmsp_mg_info_t *info);
int bmsp_mg_vcycle(bmsp_mg_t mg, const void *d_r, void *d_z, void *stream);
int bmsp_mg_solve(bmsp_mg_t mg, int method, const void *d_b, void *d_x, int64_t max_iter, double tol, int flags,
                  double *relres_history, bmsp_krylov_info *info, void *stream);
/* bmsp_gmres_solve(A[0], BMSP_OP_N, ., restart, ...) with z_j = M^-1 v_j one cycle: its arithmetic, rules, modes, results and refusals;
 * info->method is "gmres(<m>)+mg".  Takes any cycle, symmetric or not.  The views for the restriction are built before the first
 * iteration is enqueued, and the cycle's kernels read the solver's status word first, as in bmsp_mg_solve. */
int bmsp_mg_solve_gmres(bmsp_mg_t mg, int restart, const void *d_b, void *d_x, int64_t max_iter, double tol, int flags,
                        double *relres_history, bmsp_krylov_info *info, void *stream);

/* FSAI on the device: the factorised sparse approximate inverse (Kolotilina-Yeremin) on a prescribed lower-triangular pattern, the
 * preconditioner that is applied by sparse products alone, z = G^T (G r): no levels, no sweeps, nothing that can fail to contract.
 * Nothing in the reference is replaced (it has no solver).
 *   bmsp_matrix_fsai: *out = G, a new matrix with S's structure -- copied as bmsp_sddmm copies S's: no sort, scan, atomic or COO round
 *       trip -- A's dtype and its tiles in layout out_transposed.  A is square, n x n, F32 or F64 (F16: BMSP_ERR_UNSUPPORTED, as in
 *       bmsp_krylov_solve), in either tile layout.  S gives the pattern only (values and dtype ignored), n x n, either layout; every row
 *       i of S stores the diagonal and nothing to its right.  d_pivot (may be NULL) takes n elements of the vector type R (float for F32,
 *       double for F64).  A and S are never modified.  n == 0 is legal.  The call synchronises `stream` (the pattern check, bad_rows).
 *   bmsp_matrix_fsai_values: refills a G made by the first call -- or any matrix of A's shape and dtype with a legal pattern, never A
 *       itself -- after A's values changed, and drops G's value-derived caches as bmsp_matrix_copy_values does.  It synchronises `stream`
 *       too: G's pattern is checked on every call (the handle keeps no record of it), and bad_rows is read back.
 *   Arithmetic, fixed operation by operation, row by row (tests/fsai_ref.c restates it).  Nothing is contracted except the named fma.
 *       1. P = (p_1 < .. < p_m = i) are the stored columns of row i of S.
 *       2. B is m x m in R: B_ab is the stored entry of op(A) at (p_a, p_b), or +0 if none is stored.
 *       3. LU without pivoting: for k = 1 .. m-1, with pivot B_kk, for a = k+1 .. m: L_ak = B_ak / B_kk (one IEEE division), then for
 *          b = k+1 .. m: B_ab = fma(-L_ak, B_kb, B_ab).
 *       4. y_m = 1 / B_mm.
 *       5. For a = m-1 down to 1: s = +0; for c = a+1 .. m ascending s = fma(-L_ca, y_c, s); y_a = s.  This is y^T B = e_m^T.
 *       6. BMSP_FSAI_SCALE_NONE: g = y.  BMSP_FSAI_SCALE_SQRT: q = sqrt(y_m), g_a = y_a / q for every a.  BMSP_FSAI_SCALE_UNIT:
 *          g_a = y_a / y_m for every a.
 *       7. G[i, p_a] = g_a, d_pivot[i] = y_m.
 *       Every B_ab is one chain in k order and every y_a one chain in c order, so the bits do not depend on how a row is computed: W
 *       lanes per row, W the smallest of 8, 16, 32, 64 that holds the longest row of S (a pure function of S's structure), a lane per
 *       row of B, B in LDS sized from W alone.  BMSP_FSAI_LANES=<W> (read per call) forces a larger W and never changes the bits.  No
 *       flag, no spin, no floating-point atomic: only the integer count of bad rows.  op T runs on a temporary bmsp_matrix_transpose(A),
 *       freed before the call returns.
 *   Breakdown: a zero or non-finite pivot, or a negative y_m under SQRT, is not refused: IEEE gives Inf / NaN in that row and only in
 *       that row (BMSP_PC_JACOBI's rule).  info->bad_rows counts the rows of G that hold a non-finite value.
 *   bmsp_fsai_info: the kernel instantiation by name, W (lanes), rows, the longest row, the sum of m^2 over the rows (pairs), bad_rows
 *       and the LDS bytes per workgroup.
 *   BMSP_ERR_LIMIT: the first row of S with more than 64 stored entries, the message naming the row and its length (thin the pattern
 *       first, bmsp_matrix_prune); 2^32 tiles or values or more.
 *   BMSP_ERR_INVALID, the message naming the argument, scalars before handles, nothing left allocated: op, scale or out_transposed out
 *       of range; a null A, S, G, out or info; a non-square A; shapes that differ; row-panel views; the first row of S whose diagonal is
 *       not stored; the first row of S that stores a column to the right of the diagonal.  *out is untouched by a refused call. */
#define BMSP_FSAI_SCALE_NONE 0
#define BMSP_FSAI_SCALE_SQRT 1
#define BMSP_FSAI_SCALE_UNIT 2
typedef struct { char kernel[64]; int lanes; int64_t rows, max_row, pairs, bad_rows, lds_bytes; } bmsp_fsai_info;
int bmsp_matrix_fsai(bmsp_matrix_t A, int op, bmsp_matrix_t S, int scale, int out_transposed, void *d_pivot /* n of R, may be NULL */,
                     void *stream, bmsp_matrix_t *out, bmsp_fsai_info *info);
int bmsp_matrix_fsai_values(bmsp_matrix_t A, int op, bmsp_matrix_t G, int scale, void *d_pivot, void *stream, bmsp_fsai_info *info);

/* The FSAI preconditioner handle.  bmsp_precond is fixed and kind 4 stays refused: like bmsp_mg_t this has its own handle and its own
 * solves, bound to the preconditioner hook of bmsp_krylov_solve / bmsp_gmres_solve.
 *   Kinds: BMSP_FSAI_SPD: G = fsai(A, N, S, SQRT) and z = G^T (G r); G A G^T has a unit diagonal and the preconditioner is symmetric
 *       positive definite, so CG may use it.  BMSP_FSAI_GENERAL: L^ = fsai(A, N, S, NONE), W = fsai(A, T, S, UNIT), z = W^T (L^ r); with
 *       full patterns this is U^-1 D^-1 L^-1 exactly, and for a symmetric A it equals the SPD kind in exact arithmetic.
 *   Application: exactly two public products, and its bits are theirs: t = bmsp_spmv_op(G1, N, 1, r, 0, t), then by default z =
 *       bmsp_spmv_op(G2t, N, 1, t, 0, z) on a transpose the handle materialises with bmsp_matrix_transpose, or under
 *       BMSP_FSAI_NO_MATERIALISE z = bmsp_spmv_op(G2, T, 1, t, 0, z).  BMSP_FSAI_COLMAJOR puts every factor (and transpose) in the
 *       column-major layout, bmsp_spmv_op's pure view case.  (SPD: G1 = G2 = G.  GENERAL: G1 = L^, G2 = W.)
 *   The handle borrows A and owns its factors, its transpose and one work vector; S may be freed after create.  bmsp_fsai_create and
 *       bmsp_fsai_update (new factor values after a value update of A) synchronise `stream`.  bmsp_fsai_factors lends the two factor
 *       handles (either pointer may be NULL).  bmsp_fsai_apply (d_z must not be d_r) is asynchronous: the views the products
 *       need are built at create.  One stream per handle at a time.  bmsp_fsai_free does not synchronise.  bmsp_fsai_get_info reports the
 *       kind, the flags, n, whether the transpose is materialised, the bmsp_fsai_info of both factors and the bytes the handle owns.
 *   bmsp_fsai_solve / bmsp_fsai_solve_gmres: bmsp_krylov_solve(A, BMSP_OP_N, method, ...) / bmsp_gmres_solve(A, BMSP_OP_N, ., restart,
 *       ...) with that application as z = M^-1 r: their arithmetic, stop and breakdown rules, modes, history, info and refusals.
 *       info->method is "cg+fsai", "bicgstab+fsai" or "gmres(<m>)+fsai"; precond_applies counts applications.  The views are built
 *       before the first iteration is enqueued.  As with the ILU kinds, the two library products of an iteration enqueued behind a stop
 *       still run on work vectors: the only wasted work.  bad_rows > 0 is not refused: the solve ends in BMSP_KRYLOV_BREAKDOWN.  n == 0
 *       returns BMSP_KRYLOV_CONVERGED after 0 iterations.
 *   Refused with BMSP_ERR_INVALID: an unknown kind; flags with unknown bits; a null A, S, out, handle or vector; what bmsp_matrix_fsai
 *       refuses; for the solves what bmsp_krylov_solve / bmsp_gmres_solve refuse. */
#define BMSP_FSAI_SPD 0
#define BMSP_FSAI_GENERAL 1
#define BMSP_FSAI_NO_MATERIALISE 1
#define BMSP_FSAI_COLMAJOR 2
typedef struct bmsp_fsai_s *bmsp_fsai_t;
typedef struct { int kind, flags, materialised; int64_t n, owned_bytes; bmsp_fsai_info factor[2]; } bmsp_fsai_handle_info;
int bmsp_fsai_create(bmsp_matrix_t A, bmsp_matrix_t S, int kind, int flags, void *stream, bmsp_fsai_t *out);
int bmsp_fsai_update(bmsp_fsai_t f, void *stream);
int bmsp_fsai_free(bmsp_fsai_t f);
int bmsp_fsai_get_info(bmsp_fsai_t f, bmsp_fsai_handle_info *info);
int bmsp_fsai_factors(bmsp_fsai_t f, bmsp_matrix_t *G1, bmsp_matrix_t *G2);
int bmsp_fsai_apply(bmsp_fsai_t f, const void *d_r, void *d_z, void *stream);
int bmsp_fsai_solve(bmsp_fsai_t f, int method, const void *d_b, void *d_x, int64_t max_iter, double tol, int flags,
                    double *relres_history, bmsp_krylov_info *info, void *stream);
int bmsp_fsai_solve_gmres(bmsp_fsai_t f, int restart, const void *d_b, void *d_x, int64_t max_iter, double tol, int flags,
                          double *relres_history, bmsp_krylov_info *info, void *stream);

/* SDDMM, the sampled dense-dense product on the pattern of S: for every stored coordinate (i, j) of S
 *       c_ij = alpha * d_ij + beta * s_ij      or, under BMSP_SDDMM_MUL_S,      c_ij = alpha * d_ij * s_ij,      d_ij = sum_{t<k} X[i][t] * Y[j][t]
 * on the device, without a COO round trip (the gradient of bmsp_spmm with respect to A's values, the edge scores of graph attention, the
 * residual of a sparse factorisation on its pattern).  Nothing in the reference is replaced: it has no such entry point.
 *   Operands: X is num_rows x k, row-major, leading dimension ldx >= k; Y is num_cols x k, row-major, leading dimension ldy >= k; elements
 *       of S's dtype (fp16 for F16), bmsp_spmm's convention for its X.  Matrix coordinates, whatever S's tile layout.  The padding columns
 *       k <= t < ld are never read into a result, rows at or beyond num_rows / num_cols are never read (the ragged last block-row and
 *       block-column).
 *   Dot product: products and sums in fp32 (double for F64); F16 operands are widened exactly, so their products are exact in fp32.  The
 *       order of summation is the implementation's and contraction into fused multiply-adds is allowed, but d is a pure function of the
 *       inputs and the two switches below: no atomic, no dependence on scheduling, two calls with the same inputs give the same bits.
 *   Epilogue: alpha and beta are rounded once to the arithmetic type (fp32; double for F64); each operation is rounded on its own, never
 *       contracted (as bmsp_matrix_add).  Default form c = fl(fl(alpha * d) + fl(beta * s)); with beta == 0 after that rounding s is not
 *       read: c = fl(alpha * d), a NaN stored in S does not propagate.  BMSP_SDDMM_MUL_S: c = fl(fl(alpha * d) * s); beta must be 0.  F16
 *       outputs are rounded once more to fp16, round-to-nearest-even (the result may overflow to +-Inf).  Subnormals are kept.
 *   bmsp_sddmm: `out` is a fresh pool-owned matrix of S's shape and dtype with tiles in layout out_transposed (S may have either); its
 *       keys, bitmaps, offsets and block-row pointer equal bmsp_matrix_convert_layout(S, out_transposed)'s bit for bit: every coordinate is
 *       kept, results equal to 0 included.  The output remembers S as a bmsp_matrix_scale output does, so bmsp_sddmm_values,
 *       bmsp_matrix_scale_values and bmsp_matrix_copy_values accept it later.  S and its caches are not modified.  Asynchronous on
 *       `stream`: nothing is read back, the call does not synchronise.
 *   bmsp_sddmm_values: the same value pass into an existing matrix.  out == S works in place.  Any other `out` must have been made from S
 *       by bmsp_sddmm, bmsp_matrix_scale or bmsp_matrix_convert_layout while S's STRUCTURE has not changed since (the uid rule of
 *       bmsp_matrix_scale_values); anything else -- an unrelated handle, a bmsp_matrix_transpose output -- is BMSP_ERR_INVALID.  Drops
 *       out's value-derived caches as bmsp_matrix_scale_values does (an in-place S's included; dropping existing ones synchronises the
 *       device).  S is never modified unless it is `out`.
 *   Kernels: sddmm_value_kernel (vector ALU, 1 or 8 lanes per tile, every dtype) and sddmm_tile_kernel (matrix cores, F16 and F32: a
 *       tile's 64 candidates as one 8 x k by k x 8 product, two tiles per MFMA).  The tile kernel needs X, Y, ldx and ldy 16-byte aligned;
 *       see README for when it is the default.  Switches, read per call: BMSP_SDDMM_KERNEL=value|tile forces a side (a forced `tile` on
 *       F64 or misaligned operands runs the value kernel), BMSP_SDDMM_LANES=1/8 the lanes per tile of the value kernel.
 *   bmsp_sddmm_launch_info: the launcher's own decision for (S, k, ldx, ldy) with 16-byte aligned X and Y, made by the function the
 *       launcher itself calls: the kernel by name ("sddmm_value_kernel<1>" / "<8>", "sddmm_tile_kernel", "none (empty matrix)"), the lanes
 *       per tile of the value kernel (0 for the tile kernel) and the bytes the launch must move.  Counting rule: 24 B of structure per
 *       tile (key, bitmap, offset); S's values as read (the info call has no beta: a beta == 0 launch moves nnz elements fewer); the
 *       values written; k elements for every X row and every Y row a tile touches, counted once per tile that touches it -- the tile
 *       kernel touches the min(8, rows left) X rows and min(8, columns left) Y rows of each tile, the value kernel the rows and columns
 *       of the tile that hold a stored value.  Reads S's keys and bitmaps back (it synchronises).  Reporting only.
 *   Refused with BMSP_ERR_INVALID, the message naming the argument, scalars before handles: k < 1; ldx < k or ldy < k; flags with unknown
 *   bits; BMSP_SDDMM_MUL_S with beta != 0; out_transposed not 0 / 1; null S, d_X, d_Y, out, info; row-panel views.  BMSP_ERR_LIMIT: 2^32
 *   tiles or values or more. */
#define BMSP_SDDMM_MUL_S 1   /* flags bit 0: c = fl(fl(alpha*d) * s) instead of fl(fl(alpha*d) + fl(beta*s)) */
int bmsp_sddmm(bmsp_matrix_t S, const void *d_X, int64_t ldx, const void *d_Y, int64_t ldy, int k,
               double alpha, double beta, int flags, int out_transposed, void *stream, bmsp_matrix_t *out);
int bmsp_sddmm_values(bmsp_matrix_t S, const void *d_X, int64_t ldx, const void *d_Y, int64_t ldy, int k,
                      double alpha, double beta, int flags, bmsp_matrix_t out, void *stream);
typedef struct { char kernel[64]; int lanes; int64_t compulsory_bytes; } bmsp_sddmm_info;
int bmsp_sddmm_launch_info(bmsp_matrix_t S, int k, int64_t ldx, int64_t ldy, int out_transposed, bmsp_sddmm_info *info);

/* Masked SpGEMM, the product of two sparse matrices evaluated only on the pattern of a third (GraphBLAS mxm with a mask): for every stored
 * coordinate (i, j) of M
 *       c_ij = alpha * d_ij + beta * m_ij      or, under BMSP_MASKED_MUL_M,      c_ij = alpha * d_ij * m_ij,
 *       d_ij = the sum over the inner indices k at which A stores (i, k) AND B stores (k, j) of a_ik * b_kj
 * on the device (triangle counting (A * A) o A, a Galerkin product kept on a prescribed pattern instead of bmsp_spgemm followed by
 * bmsp_matrix_prune, the residual of an incomplete factorisation on its pattern, masked attention with sparse factors).  Nothing in the
 * reference is replaced: it has no such entry point.
 *   Shapes and layouts: A is m x n, B is n x p, M is m x p, in matrix coordinates.  Each of the three may have either tile layout: an
 *       operand in the "wrong" layout is read through the transposed bitmap, no conversion and no copy is made.  A, B and M may be the
 *       same handle.
 *   Dtypes: A and B share a dtype; M has that dtype, or F32 when A and B are F16 (what bmsp_spgemm returns for F16 operands); the output
 *       has M's dtype.
 *   Dot product: bmsp_spmv's stored-entries-only rule -- an unstored position never contributes (an Inf stored in A opposite a position B
 *       does not store does not reach the result), a stored 0 does (0 * Inf = NaN).  The order is fixed: k ascending over the whole inner
 *       dimension, one fused multiply-add per product, d = fma(a_ik, b_kj, d) starting from +0, in fp32 (double for F64).  F16 operands
 *       are widened exactly, so their products are exact in fp32: these are the numerics of bmsp_spgemm's tc_version 1..4, NOT those of
 *       tc_version 5 (V15) on F16, which rounds every product to fp16.  For finite F32 / F64 operands, alpha = 1 and beta = 0 the call
 *       returns the values bmsp_spgemm(A, B, tc_version 5) stores at M's coordinates (the same chain of fused multiply-adds) and +0 at
 *       coordinates the product does not hold; the sign of a zero result is not specified.  d is a pure function of the three matrices:
 *       nothing in it depends on scheduling or on the lane switch below, two calls with the same inputs give the same bits.
 *   Epilogue: bmsp_sddmm's, operation by operation.  alpha and beta are rounded once to the arithmetic type (fp32; double for F64); each
 *       operation is rounded on its own, never contracted.  Default form c = fl(fl(alpha * d) + fl(beta * m)); with beta == 0 after that
 *       rounding m is not read: c = fl(alpha * d), a NaN stored in M does not propagate.  BMSP_MASKED_MUL_M: c = fl(fl(alpha * d) * m);
 *       beta must be 0.  An F16 output is rounded once more, round-to-nearest-even (it may overflow to +-Inf).  Subnormals are kept.
 *   bmsp_spgemm_masked: `out` is a fresh pool-owned matrix of M's shape and dtype with tiles in layout out_transposed; its keys, bitmaps,
 *       offsets and block-row pointer equal bmsp_matrix_convert_layout(M, out_transposed)'s bit for bit: every coordinate is kept, zeros
 *       included.  The output remembers M as a bmsp_matrix_scale / bmsp_sddmm output does.
 *   bmsp_spgemm_masked_values: the same value pass into an existing matrix.  out == M works in place.  Any other `out` must have been made
 *       from M by this call, bmsp_sddmm, bmsp_matrix_scale or bmsp_matrix_convert_layout while M's STRUCTURE has not changed since;
 *       anything else is BMSP_ERR_INVALID.  out == A or out == B is refused (the pass would read what it writes); M == A with a separate
 *       `out` is the triangle-counting call.  Drops out's value-derived caches as bmsp_sddmm_values does.
 *   A, B and M and their caches are not modified, except that A's block-row pointer and B's op-T view (the cached view of bmsp_spmv_op(B,
 *       BMSP_OP_T): B's tiles in (block-column, block-row) order with a block-column pointer, structure only) are built if missing.
 *   Synchronisation: the first call on a B without its op-T view builds the view and synchronises `stream`.  After that both calls are
 *       asynchronous on `stream`: nothing is read back, no temporary is allocated.  The pass reads A's and B's value arrays at every call,
 *       so value-only updates need no bmsp_matrix_invalidate; bmsp_matrix_invalidate(B, 1) drops the view.
 *   Kernel: spgemm_masked_kernel (vector ALU), 1 or 8 lanes per M tile; a lane owns one byte of the output bitmap at a time and walks the
 *       intersection of A's block-row with B's block-column in ascending inner index.  BMSP_MASKED_LANES=1/8 forces the lanes per tile
 *       (read per call; default: eight at every fill, the measured choice -- see README).  An M tile whose two lists are both long
 *       (hub x hub on a power-law matrix) is one lane group's serial chain.
 *   bmsp_spgemm_masked_launch_info: the kernel by name ("spgemm_masked_kernel<1>" / "<8>", "none (empty mask)"), the lanes per M tile, the
 *       bytes of B's view and `pairs`, the number of triples (M tile (I, J), K) for which A holds tile (I, K) and B holds tile (K, J) --
 *       counted on the device by the walk the value kernel uses.  Builds the view if it is missing and synchronises.  Reporting only.
 *   Refused with BMSP_ERR_INVALID, the message naming the argument, scalars before handles, all before any device call: flags with unknown
 *   bits; BMSP_MASKED_MUL_M with beta != 0; out_transposed not 0 / 1; null A, B, M, out, info; A.num_cols != B.num_rows or M not m x p;
 *   dtype combinations other than the four above; row-panel views; out aliasing A or B.  BMSP_ERR_LIMIT: 2^32 tiles or values or more in
 *   any operand. */
#define BMSP_MASKED_MUL_M 1   /* flags bit 0: c = fl(fl(alpha*d) * m) instead of fl(fl(alpha*d) + fl(beta*m)); beta must be 0 */
int bmsp_spgemm_masked(bmsp_matrix_t A, bmsp_matrix_t B, bmsp_matrix_t M, double alpha, double beta, int flags,
                       int out_transposed, void *stream, bmsp_matrix_t *out);
int bmsp_spgemm_masked_values(bmsp_matrix_t A, bmsp_matrix_t B, bmsp_matrix_t M, double alpha, double beta, int flags,
                              bmsp_matrix_t out, void *stream);
typedef struct { char kernel[64]; int lanes; int64_t pairs, view_bytes; } bmsp_spgemm_masked_info;
int bmsp_spgemm_masked_launch_info(bmsp_matrix_t A, bmsp_matrix_t B, bmsp_matrix_t M, int out_transposed,
                                   bmsp_spgemm_masked_info *info);

/* SURVEY 8(f)3 -- Y = A * X for k vectors at once (what the reference's unfinished `batched` path points at,
 * src/bmSparse_SPMV.cu:84-150,191).  X is row-major num_cols x k with leading dimension ldx (elements of A's dtype),
 * Y row-major num_rows x k with leading dimension ldy (float, double for F64): one pass over A's tiles for all k.
 * Every Y[i][j], i < num_rows, j < k, is written (0 for a row without stored values); the padding columns j >= k of a strided Y
 * and of X are neither written nor read into the result.  Each column of Y is the sum bmsp_spmv defines (stored entries only, IEEE
 * propagation of stored Inf / NaN, fp32 / double arithmetic, subnormals kept -- the LDS float adds of spmm_vstream_kernel included --,
 * +0 for a row without stored entries), on every kernel this call may launch.  On a row-panel view (bmsp_matrix_row_panel) the view keeps the parent's
 * num_rows, so the rows outside the panel are rows without stored values: they are written as exact 0, not left untouched.
 * Runs on `stream`; the first product of a handle builds bmsp_spmv's plan and synchronises as that call does.  After that the call is
 * asynchronous on `stream` unless A has block-rows long enough to be split over several work items: their k-wide carry slots and
 * arrival counters are temporaries, and the call synchronises `stream` before they go back to the pool.  Without such block-rows
 * nothing is enqueued on a temporary.  One stream per handle at a time, as for bmsp_spmv. */
int bmsp_spmm(bmsp_matrix_t A, const void *d_X, int64_t ldx, void *d_Y, int64_t ldy, int k, void *stream);

/* The kernel bmsp_spmm(A, X, ldx, Y, ldy, k) launches, by name: "spmm_vstream_kernel<4>" / "<8>", "spmm_kernel<4>" / "<16>" / "<64>",
 * "spmm_wide_kernel", "spmv: <bmsp_spmv_launch_info's name>" when the call is handed to the SpMV (k = 1, unit strides), or
 * "none (empty matrix)" for a matrix of zero rows (a matrix with rows but no stored value launches a kernel: it writes the zeros).
 * Same argument checks and the same preparation as bmsp_spmm (block-row pointer, plan, position cache); the choice is made by the
 * function the launcher itself calls.  Reporting only (tests pin kernels with it). */
int bmsp_spmm_launch_info(bmsp_matrix_t A, int k, int64_t ldx, int64_t ldy, char *kernel_name, size_t kernel_name_cap);

/* Y = alpha * op(A) * X + beta * Y for k vectors at once, op(A) = A (BMSP_OP_N) or A^T (BMSP_OP_T), for a matrix in EITHER tile layout
 * -- the multi-vector form of bmsp_spmv_op: the gradient of bmsp_spmm with respect to X (A^T * G) without bmsp_matrix_transpose and a
 * second copy of the matrix, the multi-vector product of a column-major matrix (bmsp_spmm refuses those), and a scaled accumulate.
 * Nothing in the reference is replaced: its one product is u = A * v on a row-major A (src/bmSparse_SPMV.cu:191-230; bmsp_spmv above).
 *   Operands: X is in_len x k, row-major, leading dimension ldx >= k, elements of A's dtype (fp16 for F16); in_len = num_cols for N,
 *       num_rows for T.  Y is out_len x k, row-major, leading dimension ldy >= k, float for F32 / F16 and double for F64.  Matrix
 *       coordinates, whatever the tile layout.  Pointers need the alignment of their element type and no more.
 *   Read and written: every Y[i][c], i < out_len, c < k, is written.  The padding columns k <= c < ld of X are never read into a result,
 *       those of Y never written.  No row of X at or beyond in_len is read (the ragged last block).
 *   Sum: t[i][c] = the sum over the stored entries of row i of op(A) of a * X[col][c] -- bmsp_spmv's rule, stored entries only: an X
 *       element at an input index where output row i stores nothing never reaches t[i][c], inside a stored tile too, and a stored value
 *       is always multiplied (a stored 0 against Inf is NaN; Inf and NaN propagate as IEEE says).  Products and sums in fp32 (double for
 *       F64), F16 operands widened exactly, subnormals kept; +0 for a row without stored entries.  Contraction into fused multiply-adds
 *       is allowed and the order of summation is the implementation's, but t is a pure function of A's arrays, X, k, the strides and the
 *       switches below: no floating-point atomic anywhere, no dependence on scheduling, two calls with the same inputs give the same bits.
 *   Epilogue: bmsp_spmv_op's, element by element.  alpha and beta are rounded once to the vector type.  beta == 0 (after that rounding):
 *       Y = fl(alpha * t); Y is not read, a NaN in it does not propagate.  Otherwise Y = fl(fl(alpha * t) + fl(beta * Y)), each operation
 *       rounded on its own, never contracted.  alpha == 0 is not special-cased.
 *   (N, row-major A) is bmsp_spmm's case: t is exactly what bmsp_spmm(A, X, ldx, ., ., k) writes; with alpha == 1 and beta == 0 the call
 *       IS that call into Y, otherwise bmsp_spmm runs into a temporary kept on the handle (out_len x k, unit stride, sized for the largest
 *       out_len * k seen on the handle) and one strided epilogue kernel follows.  bmsp_spmm's synchronisation rules apply to this case.
 *   The other three cases sweep the cached view of (A, op) that bmsp_spmv_op builds: the same records, items and fold list, ONE view per
 *       op shared by both calls, dropped by the same events (bmsp_matrix_invalidate(A, 1), bmsp_matrix_free; value-only updates keep it).
 *       The items of an output block of more than SPLIT tiles need 8 * k accumulators per scratch slot: a buffer on the handle that grows
 *       when slots * k exceeds what any earlier call needed and is freed with the views.  Values are read from A's value array at every
 *       call.
 *   Asynchronous on `stream` with two exceptions, both of which synchronise it: the one-time build of the view, and a call that has to
 *       grow the scratch or the temporary (the old buffer goes back to the pool only after the work enqueued on it has finished).  One
 *       stream per handle at a time.  A's four arrays are not modified.
 *   Switches, read per call: BMSP_SPMM_OP_LANES=8/16/32/64 forces W, the lanes (= columns of X and Y) of one tile slot of a wave; by default
 *       the smallest of them that is >= min(k, 64).  Columns beyond W go to further column chunks.  BMSP_SPMV_OP_SPLIT belongs to the
 *       shared view and keeps its meaning (read when a view is built).
 *   Refused with BMSP_ERR_INVALID, the message naming the argument, scalars before handles: op not 0 / 1; k < 1; ldx < k or ldy < k; null
 *   A, d_X, d_Y, info; row-panel views.  BMSP_ERR_LIMIT: 2^32 tiles or values or more; slots * 8 * k scratch elements beyond 2^32 - 1. */
int bmsp_spmm_op(bmsp_matrix_t A, int op, double alpha, const void *d_X, int64_t ldx, double beta, void *d_Y, int64_t ldy, int k, void *stream);
/* What bmsp_spmm_op(A, op, ., X, ldx, ., Y, ldy, k) launches -- the launcher's own decisions, made by the function the launcher calls:
 * the kernel by name ("spmm_op_sweep_kernel<MINOR, 16>": MAJOR / MINOR as for bmsp_spmv_op, then W; "bmsp_spmm: <bmsp_spmm_launch_info's
 * name>" for (N, row-major A) -- bmsp_spmm into Y at ldy, the alpha == 1, beta == 0 call --, which has no view: lanes, col_chunks, items, split_blocks 0, view_bytes = scratch_bytes = the temporary
 * once it exists; "none (no output)"), W (`lanes`), the column chunks ceil(k / W), the work items, the split output blocks, the bytes
 * the view holds, the bytes of the scratch this call needs (8 * k * slots accumulators) and the bytes the launch must move.
 *   Counting rule for compulsory_bytes (the view cases; 0 for (N, row-major A), whose kernels bmsp_spmm_launch_info names): per column
 *       chunk the 16 B record of every tile and the 16 B of every work item; per column chunk every stored value once (element size of
 *       A's dtype); k elements of X for every X row a tile reads, counted once per tile that reads it (the rows of the tile's input side
 *       that hold a stored value, not once per matrix); Y written: out_len * k accumulator elements; Y read: NOT counted -- the info call
 *       has no beta and reports the beta == 0 launch, a beta != 0 launch moves out_len * k accumulator elements more; per scratch slot
 *       its 8 * k accumulators stored and read back; the fold list, 12 B per split block.  Builds the view if it is missing (it synchronises) and reads A's bitmaps back for the X rows.  Reporting only. */
typedef struct { char kernel[64]; int lanes, col_chunks; int64_t items, split_blocks, view_bytes, scratch_bytes, compulsory_bytes; } bmsp_spmm_op_info;
int bmsp_spmm_op_launch_info(bmsp_matrix_t A, int op, int k, int64_t ldx, int64_t ldy, bmsp_spmm_op_info *info);

/* per-stage figures of one product: the lines the reference prints when VERBOSE
 * (src/bmSparse_SPGEMM.cu:849-1220) plus what the roofline needs. */
typedef struct {
    int64_t task_list_size;  /* candidate block pairs ("Task list size") */
    int64_t bmp_reduction;   /* pairs dropped by the bitmap filter ("Bmp reduction") */
    int64_t surviving_tasks;
    int64_t c_blocks;        /* "C blocks" */
    int64_t c_nnz;           /* "C nnz" (symbolic) */
    double t_us[10];         /* device time per stage, microseconds: [1]=T_1 [2]=T_2 [3]=T_3 [4]=T_4 [5]=T_5
                                [6]=T_6 [7]=T_7 [9]=T_9 ; [0]=whole call ("Toda F"); [8]=segmented sort only */
    int sort_path;           /* 0 = global radix sort (reference: thrust::sort), 1 = segmented sort, 2 = none: C's structure formed
                              * block-row by block-row in LDS (BMSP_SORT_PATH_ROWMERGE; T_3 then holds the whole symbolic pass) */
    int mac_kernel;          /* which block-MAC kernel ran (see tc_version) */
    int mac_variant;         /* which implementation of it: BMSP_MAC_* below */
    int sort_long;           /* detail of sort_path.  sort_path 1: how block-rows of more tasks than one wave sorts in registers were ordered -- 0 =
                              * there were none, 1 = pieces + merge passes, 2 = stable counting passes on the column bits (BMSP_SORT_LONG_*).
                              * sort_path 2 (row-merge): 1 = strip mode (C's structure only, no task list), 2 = task-list mode (BMSP_ROWMERGE_*).
                              * sort_path 3 (column windows): 1 = this call first tried the task-list pass and gave it up (the first product of a
                              * pair), 0 = it went straight to the window passes (BMSP_ROWWINDOW_AFTER_TASKLIST) */
} bmsp_spgemm_stats;
/* implementations behind one tc_version (the launcher picks by the product's shape; all give the tc_version's numerics) */
#define BMSP_SORT_PATH_ROWMERGE 2
#define BMSP_ROWMERGE_STRIP 1
#define BMSP_ROWMERGE_TASKLIST 2
#define BMSP_ROWWINDOW_AFTER_TASKLIST 1
#define BMSP_SORT_LONG_MERGE 1
#define BMSP_SORT_LONG_RADIX 2
#define BMSP_SORT_PATH_ROWWINDOW 3 /* none either: block-rows of C formed window by window of block columns in dense LDS tables (operands with hub block-rows) */
#define BMSP_MAC_DEFAULT 0 /* the only kernel of that tc_version (V15 vector-ALU kernels, K = 16 MFMA kernels) */
#define BMSP_MAC_STAGED 1  /* tc 4: K = 32 MFMA, operands staged through LDS per task (sparse task lists) */
#define BMSP_MAC_DIRECT 2  /* tc 4: K = 32 MFMA, operand lines loaded per task straight into the MFMA lanes */
#define BMSP_MAC_STRIP 3   /* tc 4: K = 32 MFMA, two block-rows of C per wave, A tiles register-resident, B tiles loaded once per strip */
#define BMSP_MAC_ROWSPARSE 5 /* V15 numerics (fp32 operands; fp16 operands under tc 5) on operands of nearly empty tiles (row-merge strip mode): the
                             * reference's chain over the products of STORED values only, row-wise over CSR copies, accumulators per C value in LDS */
#define BMSP_MAC_F32MFMA 4 /* tc 5, fp32, opt-in (BMSP_MAC_F32MFMA=1): V15's fmaf chain on v_mfma_f32_16x16x4_f32, operands from lane-ordered tile copies */

/* sort modes = the reference's `segmented` argument (src/bmSparse_SPGEMM.cu:963-1016):
 * 0 = global sort below BMSP_SORT_BORDER surviving tasks, segmented sort above; 1 = always segmented;
 * 2 = always global. */
#define BMSP_SORT_AUTO 0
#define BMSP_SORT_SEGMENTED 1
#define BMSP_SORT_GLOBAL 2
#define BMSP_SORT_BORDER 2730000 /* src/bmSparse_SPGEMM.cu:53 */

/* bmSparse_mult<VI,VO>(A, B, C, mode, VERBOSE, tc_version)  -- src/bmSparse_SPGEMM.cu:827-1223.   C = A * B
 * A: normal layout; B: built with transposed=1; same dtype.  *C receives a new fp32 (fp64 for F64 inputs)
 * matrix in normal layout.  tc_version selects the block multiply-accumulate kernel like the reference's
 * switch (:1132-1155): 5 = vector-ALU kernel with the reference's V15 numerics (each product rounded to the
 * input type, fp32 accumulate); 1..4 = matrix-core (MFMA) kernel: exact products, fp32 accumulate.
 * verbose != 0 prints the reference's stage lines to stdout.  stats may be NULL.
 * Runs on `stream`; synchronous with respect to the host on return (the reference ends with cudaDeviceSynchronize, :1158): `stream`
 * is synchronised, every temporary is back in the pool.  The same holds for bmsp_spgemm_symbolic, bmsp_spgemm_numeric and the sharded
 * products below.
 * A product with 2^32 or more candidate block pairs (more than one task list can index) is run block-row panel after panel
 * and concatenated; stats then hold the sums over the panels (stage lines are printed per panel). */
int bmsp_spgemm(bmsp_matrix_t A, bmsp_matrix_t B, bmsp_matrix_t *C, int mode, int tc_version, int verbose,
                void *stream, bmsp_spgemm_stats *stats);

/* The two halves of bmsp_spgemm for callers that multiply the same sparsity pattern again and again (new values in A / B, same
 * structure: time stepping, AMG set-ups).  The reference has one entry point, bmSparse_mult, whose stages T_1 ... T_9 are the symbolic half
 * (src/bmSparse_SPGEMM.cu:849-1107: C's keys, bitmaps, offsets, nnz) and T_7 the numeric half (:1109-1158).
 *   bmsp_spgemm_symbolic: C's structure only; *C's values are allocated and zero; where the product was formed through a task list, C
 *                         keeps that list (8 bytes per surviving pair + 4 per C tile, freed with C).  Same arguments as bmsp_spgemm otherwise.
 *   bmsp_spgemm_numeric : C must hold the structure of A x B (from bmsp_spgemm / _symbolic on operands of the SAME structure); its values
 *                         are overwritten with those of A x B under tc_version's numerics: for the V15 numerics (tc_version 5, and fp32 /
 *                         fp64 operands under any tc_version) exactly what bmsp_spgemm would store, bit for bit; for the matrix-core
 *                         kernels (fp16 operands, tc_version 1..4: exact products, fp32 accumulation in the order of whichever kernel
 *                         runs) within the tolerance stated for them.  Every product is stamped with a fingerprint of its operands'
 *                         structures (dimensions, keys, bitmaps): a C stamped for other operands is refused (BMSP_ERR_INVALID).  For a
 *                         matching stamp: where a strip block-MAC applies (fp16 operands with tc_version 4, fp32 operands; block-rows of
 *                         C of at most 256 tiles) only that kernel runs; a C from bmsp_spgemm_symbolic that kept its task list runs the
 *                         tc_version's block-MAC kernel from it (any value type).  Otherwise -- no kept list, or a C without a stamp
 *                         (adopted arrays) -- the whole product runs, its structure is checked against C's (BMSP_ERR_INVALID on a
 *                         mismatch) and its values are copied.  After changing an operand's values in place call
 *                         bmsp_matrix_invalidate(m, 0) first (cached tile copies); after changing its structure, (m, 1).  C itself
 *                         needs no such call: bmsp_spgemm_numeric is one of the library's in-place writers and drops C's own
 *                         value-derived caches (C is a valid left operand of a further product) before it writes C's values. */
int bmsp_spgemm_symbolic(bmsp_matrix_t A, bmsp_matrix_t B, bmsp_matrix_t *C, int mode, int tc_version, void *stream,
                         bmsp_spgemm_stats *stats);
int bmsp_spgemm_numeric(bmsp_matrix_t A, bmsp_matrix_t B, bmsp_matrix_t C, int tc_version, void *stream, bmsp_spgemm_stats *stats);

/* Hardware self test of the operand / result lane layout the K = 32 block-MAC relies on (v_mfma_f32_16x16x32_f16: lane l holds
 * A[l&15][8*(l>>4)+j], B[8*(l>>4)+j][l&15], D[4*(l>>4)+i][l&15]): one 16x16x32 product of asymmetric small integers against a host
 * loop.  *mismatches = number of wrong elements (0 on gfx950).  The reference's analogue is the fragment-layout assumption of
 * multiplyV12..V14 (src/bmSparse_SPGEMM.cu:548-552), which it never checks. */
int bmsp_selftest_mfma_layout(int *mismatches);
/* Hardware self test of the ACCUMULATION ORDER of v_mfma_f32_16x16x4_f32: D = C + A * B on random fp32 operands against the host chain
 * fmaf(a_k, b_k, sum) for k ascending -- the order of multiplyV15<float, float> (src/bmSparse_SPGEMM.cu:269-273 as nvcc contracts it).
 * *mismatches = number of result elements that differ in any bit (0 on gfx950).  With 0 the fp32 product (tc_version 5) CAN run its
 * block-MAC on the matrix cores with values bit-identical to the vector-ALU kernel (BMSP_MAC_F32MFMA=1 selects that kernel; it is not the
 * default: measured on MI355X it is bound by the 256-byte operand tiles it reads and no faster than the vector-ALU kernels). */
int bmsp_selftest_mfma_f32_chain(int *mismatches);
/* The same on the corner the exponent guard of the fp32 matrix-core kernels must know about: every product a normal number (~2^-123), signs
 * alternating, so that the partial sums cancel into the subnormal range.  *mismatches = result elements that differ from the host's fmaf
 * chain; *exp_floor (may be NULL) = the smallest sum of the two operands' smallest biased exponents those kernels then accept: 128 when
 * the instruction is the chain there too, 174 otherwise (products can then not cancel below 2^-126) -- below the floor V15's vector-ALU
 * kernel computes the product. */
int bmsp_selftest_mfma_f32_cancel(int *mismatches, int *exp_floor);
/* Hardware self test of the byte-permute form of bmp_calculator (src/bmSparse_SPGEMM.cu:787-810) the row-merge passes use: 2^20 pairs of
 * bitmaps of every density, the v_perm_b32 sign-replication product on the row-major copy of B's tile against the multiply form on the
 * tile as stored.  *mismatches = pairs whose products differ (0 on gfx950). */
int bmsp_selftest_tile_product(int *mismatches);

/* bb_segsort<K,T>(keys, vals, n, segs, length)  -- include/bb_segsort-master/bb_segsort.h:35-192,
 * instantiated by the reference with K = uint64_t, T = 16-byte task_list_elem (src/bmSparse_SPGEMM.cu:1010).
 * Sorts every segment [segs[i], segs[i+1]) (last ends at n) ascending by key, in place, STABLY
 * (bb_segsort is unstable).  d_vals may be NULL (keys only). val_bytes in {4, 8, 16}.  Runs on `stream` and synchronises it before
 * it returns (work lists and the second key / value arrays are temporaries). */
int bmsp_segsort_u64(uint64_t *d_keys, void *d_vals, int val_bytes, int64_t n, const int *d_segs,
                     int64_t num_segs, void *stream);

/* ---- row-panel sharding (new; the reference is single-GPU).  One process per GPU: each rank calls these
 *      with its own rank id.  These three are the building blocks; bmsp_spgemm_sharded below runs the whole thing. ---- */

/* Splits A's block-rows into `parts` contiguous panels balanced by candidate-task count
 * (sum over the panel's A blocks of B's blocks in the matching block-row).  bounds receives parts+1
 * block-row indices. */
int bmsp_partition_rows(bmsp_matrix_t A, bmsp_matrix_t B, int parts, int64_t *bounds);
/* The sub-matrix of block-rows [brow_begin, brow_end) as a matrix that borrows m's arrays (no copy);
 * num_rows stays global so keys stay global.  Free the view before m. */
int bmsp_matrix_row_panel(bmsp_matrix_t m, int64_t brow_begin, int64_t brow_end, bmsp_matrix_t *view);
/* Concatenates `parts` row panels (each a product of bmsp_spgemm on a panel, given by its four device arrays)
 * into one matrix, re-basing offsets.  Arrays of pointers/sizes are host arrays of length parts. */
int bmsp_matrix_concat_panels(int num_rows, int num_cols, int parts, const int64_t *block_nums,
                              const int64_t *nnzs, uint64_t *const *d_keys, uint64_t *const *d_bmps,
                              uint64_t *const *d_offsets, void *const *d_values, bmsp_dtype dtype,
                              bmsp_matrix_t *out);

/* ---- the sharded operators themselves: one process per GPU, RCCL over xGMI (nothing in the reference to
 *      replace -- it is single-GPU: src/bmSparse_SPGEMM.cu:1226-1288 runs one product on device 0).  librccl is opened on the first
 *      bmsp_comm_* call, not at load time. -------------------------------------------------------------------------------- */
typedef struct bmsp_comm_s *bmsp_comm_t;
#define BMSP_COMM_ID_BYTES 128
/* rank 0 creates the 128-byte rendezvous id (ncclUniqueId) and hands it to the other ranks by any means (file, MPI, torch.distributed) */
int bmsp_comm_unique_id(void *id_bytes);
/* collective: every rank calls it with the same id, after bmsp_set_device(its GPU) */
int bmsp_comm_init(const void *id_bytes, int world, int rank, bmsp_comm_t *out);
/* the same from the environment, for the drop-in executables: BMSP_WORLD, BMSP_RANK and, when BMSP_WORLD > 1, BMSP_COMM_FILE (a path
 * every rank can reach: rank 0 writes the id there, the others wait for it) */
int bmsp_comm_init_from_env(bmsp_comm_t *out);
/* BMSP_COMM_NONCE (optional, a number the launcher gives every rank of one run) is written into / required from the rendezvous file;
 * rank 0 removes a pre-existing file first, readers refuse files without this run's nonce (and, when no nonce is set, files older than
 * 120 s), so a file left by a crashed run is never joined. */
/* An in-process "communicator" of `world` panels on the CURRENT device, no RCCL: bmsp_spgemm_sharded / bmsp_spmv_sharded then compute
 * the `world` panels one after another and move every panel into its slice with a device copy.  It shares the size gather -> slice
 * layout -> offset re-basing -> terminal offset code with the RCCL transport (only the byte movement differs): the way to run the
 * sharded operators' P > 1 logic on one GPU.  Nothing in the reference to replace (single-GPU). */
int bmsp_comm_init_loopback(int world, bmsp_comm_t *out);
int bmsp_comm_info(bmsp_comm_t c, int *rank, int *world);
/* The slice-layout arithmetic of the two exchanges, host only (no GPU call): where panel r of the sharded product lands in the whole C
 * (block_start / value_start: parts+1 entries, exclusive sums of the panels' block / value counts; offsets of panel r are re-based by
 * value_start[r]), and which rows of u panel r = block-rows [bounds[r], bounds[r+1]) delivers. */
int bmsp_shard_layout(int parts, const int64_t *block_nums, const int64_t *nnzs, int64_t *block_start, int64_t *value_start);
int bmsp_shard_row_slices(int num_rows, int parts, const int64_t *bounds, int64_t *row_start, int64_t *row_count);
int bmsp_comm_free(bmsp_comm_t c);

typedef struct {
    int world, rank;
    int64_t panel_block_row_begin, panel_block_row_end; /* this rank's block-rows of A */
    int64_t panel_tasks;                                /* surviving tasks of this rank's panel (SpGEMM) */
    int64_t exchange_bytes;                             /* bytes every rank holds after the exchange (whole C / whole y) */
    double exchange_us;                                 /* device time of the exchange on this rank (all rounds) */
    double exchange_exposed_us;                         /* ... of it, the part after this rank's last panel product had finished (not hidden behind compute) */
    double exchange_hidden_frac;                        /* 1 - exposed / total: share of the exchange that ran while panels were being multiplied */
    int rounds, gathered;                               /* rounds of panels per rank; 0 = owner keeps (no exchange: C is this rank's panel) */
} bmsp_shard_stats;

/* C = A * B with A cut into `world` block-row panels balanced by candidate-task count, B replicated (every rank passes the same A
 * and B), every rank multiplies its panel and ALL ranks return the whole C: the panels are broadcast straight into their final
 * slices (an allgatherv without padding or staging copies), offsets re-based in place.  stats = this rank's panel product. */
int bmsp_spgemm_sharded(bmsp_comm_t c, bmsp_matrix_t A, bmsp_matrix_t B, bmsp_matrix_t *C, int mode, int tc_version, int verbose,
                        void *stream, bmsp_spgemm_stats *stats, bmsp_shard_stats *shard);
/* The same with its two knobs.  gather = 1: as above, in `rounds` rounds per rank (0: the library's choice, 4 when world > 1; BMSP_SHARD_ROUNDS):
 * A is cut into rounds x world panels, rank r multiplies panels r, world + r, ...; after every round the panel sizes are gathered and the
 * round's panels are broadcast into their final slices on a second stream while the next round multiplies (shard->exchange_hidden_frac).
 * gather = 0, "owner keeps" ("If only the owner needs C, skip the gather and report it separately"): world panels, no
 * exchange; *C is this rank's panel of C (block-rows [panel_block_row_begin, panel_block_row_end), global keys) -- the loopback
 * communicator owns every panel and returns them concatenated. */
int bmsp_spgemm_sharded_ex(bmsp_comm_t c, bmsp_matrix_t A, bmsp_matrix_t B, bmsp_matrix_t *C, int mode, int tc_version, int verbose,
                           void *stream, bmsp_spgemm_stats *stats, bmsp_shard_stats *shard, int gather, int rounds);
/* u = A * v with A cut into block-row panels balanced by stored values, v replicated; every rank sweeps its panel (writing only its
 * own rows of u), the row slices are exchanged in place and all ranks return the whole u (num_rows entries).  The panel view and its sweep plan are cached on A across calls.
 * Every u_i is the sum bmsp_spmv defines (stored entries only; its special-value and subnormal rules hold panel by panel).
 * Runs on `stream` and synchronises it before it returns (the exchange; the loopback communicator's scratch vectors). */
int bmsp_spmv_sharded(bmsp_comm_t c, bmsp_matrix_t A, const void *d_v, void *d_u, int variant, void *stream, bmsp_shard_stats *shard);

/* ---- host CSR (class CSRMatrix, include/CSRMatrix.h:13-21; declared only in the reference; backed by
 *      cusp::csr_matrix<int,float,host_memory> and cusp::multiply) ---------------------------------- */
int bmsp_csr_from_mtx(const char *path, bmsp_csr_t *out);                    /* CSRMatrix(std::string) */
int bmsp_csr_from_arrays(int num_rows, int num_cols, int64_t nnz, const int *row_offsets, const int *cols,
                         const float *vals, bmsp_csr_t *out);                /* CSRMatrix(csr_matrix*) */
int bmsp_csr_info(bmsp_csr_t m, int *num_rows, int *num_cols, int64_t *nnz);
int bmsp_csr_arrays(bmsp_csr_t m, const int **row_offsets, const int **cols, const float **vals);
int bmsp_csr_multiply(bmsp_csr_t A, bmsp_csr_t B, bmsp_csr_t *C);            /* CSRMatrix::multiply */
int bmsp_csr_spmv(bmsp_csr_t A, const float *x, float *y);
/* The HOST forms of the two (the reference's CSRMatrix holds a cusp host matrix, so its multiply is cusp's host path --
 * cusp/system/detail/sequential/multiply/csr_spmv.h:56-73, csr_spgemm.h:39-157 and the omp variants): no GPU call is made; `threads`
 * host threads (0 = all).  The product's columns come out in the list order of the Gustavson accumulator (unsorted within a row,
 * csr_spgemm.h:153), numeric zeros dropped. */
int bmsp_csr_multiply_host(bmsp_csr_t A, bmsp_csr_t B, bmsp_csr_t *C, int threads);
int bmsp_csr_spmv_host(bmsp_csr_t A, const float *x, float *y, int threads);
int bmsp_csr_free(bmsp_csr_t m);

#ifdef __cplusplus
}
#endif
#endif /* BMSP_H_ */
