/*
 * bmSpMatrix.h -- the reference's container and operator names on top of the MI355X C ABI (bmsp.h).
 *
 * Keeps the public surface of the reference header include/bmSpMatrix.h:20-40 (class bmSpMatrix<T> with public
 * keys / bmps / offsets / values / num_rows / num_cols / nnz / block_num, the three constructors, compare, print,
 * generate_coo) and of the two operator templates bmSparse_SpMV (src/bmSparse_SPMV.cu:191-192) and bmSparse_mult
 * (src/bmSparse_SPGEMM.cu:827-828), so the reference's mains compile against it after swapping
 * thrust::device_vector / cusp::coo_matrix for the two small types below.  Everything is a call into libbmsp.so;
 * this header contains no compute.
 */
#ifndef BMSPMATRIX_H_
#define BMSPMATRIX_H_

#include "bmsp.h"
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#define BLOCK_WIDTH 8
#define BLOCK_HEIGHT 8
#define BMSP_BLOCK_SIZE (BLOCK_WIDTH * BLOCK_HEIGHT)

#ifndef BMSP_NO_HALF_TYPE
/* 16-bit storage type for bmSpMatrix<half> (the reference uses CUDA's __half, src/bmSpMatrix.cu:20,436). */
struct half {
    uint16_t bits;
};
#endif

namespace bmsp {

inline void check(int status)
{
    if (status != BMSP_OK) throw std::runtime_error(std::string("bmsp: ") + bmsp_last_error());
}

template <class T> struct dtype_of;
template <> struct dtype_of<float> { static const bmsp_dtype value = BMSP_F32; };
template <> struct dtype_of<double> { static const bmsp_dtype value = BMSP_F64; };
#ifndef BMSP_NO_HALF_TYPE
template <> struct dtype_of<half> { static const bmsp_dtype value = BMSP_F16; };
#endif
/* element type of the vectors that go with a matrix (SpMV results, row maxima, diagonals, scaling factors): float, double for double */
template <class T> struct vector_of { typedef float type; };
template <> struct vector_of<double> { typedef double type; };

/* The subset of thrust::device_vector the reference's code uses: size/data/begin/end/swap/clear/shrink_to_fit,
 * construction from a host vector, copy back to the host.  Owns pool memory unless it is a view. */
template <class T> class device_vector {
    T *p_ = nullptr;
    size_t n_ = 0;
    bool own_ = true;

public:
    typedef T value_type;
    device_vector() {}
    explicit device_vector(size_t n) { resize(n); }
    explicit device_vector(const std::vector<T> &h)
    {
        resize(h.size());
        if (n_) check(bmsp_memcpy_h2d(p_, h.data(), n_ * sizeof(T)));
    }
    device_vector(const device_vector &) = delete;
    device_vector &operator=(const device_vector &) = delete;
    device_vector(device_vector &&o) noexcept { swap(o); }
    device_vector &operator=(device_vector &&o) noexcept
    {
        if (this != &o) { clear(); swap(o); }
        return *this;
    }
    ~device_vector() { clear(); }
    static device_vector view(T *p, size_t n)
    {
        device_vector v;
        v.p_ = p; v.n_ = n; v.own_ = false;
        return v;
    }
    void resize(size_t n)
    {
        clear();
        void *q = nullptr;
        check(bmsp_malloc(&q, (n ? n : 1) * sizeof(T)));
        p_ = static_cast<T *>(q); n_ = n; own_ = true;
    }
    size_t size() const { return n_; }
    bool empty() const { return n_ == 0; }
    T *data() { return p_; }
    const T *data() const { return p_; }
    T *begin() { return p_; }
    T *end() { return p_ + n_; }
    void swap(device_vector &o)
    {
        std::swap(p_, o.p_); std::swap(n_, o.n_); std::swap(own_, o.own_);
    }
    void clear()
    {
        if (p_ && own_) bmsp_free(p_);
        p_ = nullptr; n_ = 0; own_ = true;
    }
    void shrink_to_fit() {}
    T *release()
    {
        T *q = p_;
        p_ = nullptr; n_ = 0;
        return q;
    }
    std::vector<T> to_host() const
    {
        std::vector<T> h(n_);
        if (n_) check(bmsp_memcpy_d2h(h.data(), p_, n_ * sizeof(T)));
        return h;
    }
};

/* host COO with the member names of cusp::coo_matrix (cusp/coo_matrix.h:155-163, detail/matrix_base.h:38-40) */
template <class T> struct coo_matrix {
    size_t num_rows = 0, num_cols = 0, num_entries = 0;
    std::vector<int> row_indices, column_indices;
    std::vector<T> values;
};

}  // namespace bmsp

template <class valueType> class bmSpMatrix {
private:
    bmsp_matrix_t h_ = nullptr;
    bmsp::coo_matrix<double> coo;  // filled by generate_coo()
    void refresh()
    {
        int64_t nz = 0, nb = 0;
        bmsp::check(bmsp_matrix_info(h_, &num_rows, &num_cols, &nz, &nb, nullptr, nullptr));
        nnz = (int)nz; block_num = (int)nb;
        uint64_t *k, *b, *o; void *v;
        bmsp::check(bmsp_matrix_arrays(h_, &k, &b, &o, &v));
        keys = bmsp::device_vector<uint64_t>::view(k, (size_t)nb);
        bmps = bmsp::device_vector<uint64_t>::view(b, (size_t)nb);
        offsets = bmsp::device_vector<uint64_t>::view(o, (size_t)nb + 1);
        values = bmsp::device_vector<valueType>::view(static_cast<valueType *>(v), (size_t)nz);
    }

public:
    bmsp::device_vector<uint64_t> keys;
    bmsp::device_vector<uint64_t> bmps;
    bmsp::device_vector<uint64_t> offsets;
    bmsp::device_vector<valueType> values;
    int num_rows = 0, num_cols = 0, nnz = 0, block_num = 0;

    bmSpMatrix() {}
    /* src/bmSpMatrix.cu:111-219 */
    bmSpMatrix(std::string path, bool transpose)
    {
        bmsp::check(bmsp_matrix_from_mtx(path.c_str(), transpose ? 1 : 0, bmsp::dtype_of<valueType>::value, &h_));
        refresh();
    }
    /* src/bmSpMatrix.cu:30-43: adopts the four device vectors (the reference swaps them in) */
    bmSpMatrix(int num_rows_, int num_cols_, int block_num_, bmsp::device_vector<uint64_t> &keys_,
               bmsp::device_vector<uint64_t> &bmps_, bmsp::device_vector<uint64_t> &offsets_,
               bmsp::device_vector<valueType> &values_)
    {
        size_t nz = values_.size();
        bmsp::check(bmsp_matrix_from_arrays(num_rows_, num_cols_, block_num_, (int64_t)nz, keys_.data(), bmps_.data(), offsets_.data(),
                                            values_.data(), bmsp::dtype_of<valueType>::value, 0, 1, &h_));
        keys_.release(); bmps_.release(); offsets_.release(); values_.release();
        refresh();
    }
    bmSpMatrix(const bmSpMatrix &) = delete;
    bmSpMatrix &operator=(const bmSpMatrix &) = delete;
    bmSpMatrix(bmSpMatrix &&o) noexcept { *this = std::move(o); }
    bmSpMatrix &operator=(bmSpMatrix &&o) noexcept
    {
        if (this != &o) {
            reset(nullptr);
            h_ = o.h_; o.h_ = nullptr;
            if (h_) refresh();
            o.reset(nullptr);
        }
        return *this;
    }
    ~bmSpMatrix() { reset(nullptr); }

    /* takes ownership of a C-ABI handle (used by bmSparse_mult for C) */
    void reset(bmsp_matrix_t h)
    {
        keys.clear(); bmps.clear(); offsets.clear(); values.clear();
        if (h_) bmsp_matrix_free(h_);
        h_ = h;
        num_rows = num_cols = nnz = block_num = 0;
        coo = bmsp::coo_matrix<double>();
        if (h_) refresh();
    }
    bmsp_matrix_t handle() const { return h_; }

    /* A^T (num_cols x num_rows) with its tiles column-major when transposed_layout (bmsp_matrix_transpose) */
    bmSpMatrix<valueType> transpose(bool transposed_layout) const
    {
        bmsp_matrix_t t = nullptr;
        bmsp::check(bmsp_matrix_transpose(h_, transposed_layout ? 1 : 0, nullptr, &t));
        bmSpMatrix<valueType> out;
        out.reset(t);
        return out;
    }
    /* the same matrix with its tiles column-major when transposed_layout (bmsp_matrix_convert_layout): the right operand of
     * bmSparse_mult from a left one, `bmSpMatrix<half> B = A.with_layout(true);` instead of parsing the file twice */
    bmSpMatrix<valueType> with_layout(bool transposed_layout) const
    {
        bmsp_matrix_t t = nullptr;
        bmsp::check(bmsp_matrix_convert_layout(h_, transposed_layout ? 1 : 0, nullptr, &t));
        bmSpMatrix<valueType> out;
        out.reset(t);
        return out;
    }
    /* the num_rows x num_aggregates matrix with weights[i] (null: 1) stored at (i, agg[i]), one entry per row, agg[i] == 0xFFFFFFFF
     * leaving row i empty (bmsp_matrix_from_aggregates): the tentative prolongator of an aggregate map; agg and weights are device
     * arrays of num_rows entries, the weights float (double for double) */
    static bmSpMatrix<valueType> from_aggregates(int num_rows, int num_aggregates, const uint32_t *agg,
                                                 const typename bmsp::vector_of<valueType>::type *weights = nullptr,
                                                 bool transposed_layout = false)
    {
        bmsp_matrix_t t = nullptr;
        bmsp::check(bmsp_matrix_from_aggregates(num_rows, num_aggregates, agg, weights, bmsp::dtype_of<valueType>::value,
                                                transposed_layout ? 1 : 0, nullptr, &t));
        bmSpMatrix<valueType> out;
        out.reset(t);
        return out;
    }
    /* P * A * Q^T at tile granularity (bmsp_matrix_permute_blocks): block (I', J') of the result is block (row_perm[I'], col_perm[J'])
     * of this matrix; the permutations are device arrays of ceil(num_rows / 8) / ceil(num_cols / 8) entries, null = the identity */
    bmSpMatrix<valueType> permute_blocks(const uint32_t *row_perm, const uint32_t *col_perm, bool transposed_layout) const
    {
        bmsp_matrix_t t = nullptr;
        bmsp::check(bmsp_matrix_permute_blocks(h_, row_perm, col_perm, transposed_layout ? 1 : 0, nullptr, &t));
        bmSpMatrix<valueType> out;
        out.reset(t);
        return out;
    }

    /* this matrix without the stored entries the rule drops (bmsp_matrix_prune): |v| <= tol under BMSP_PRUNE_ABS, |v| <= tol * rowmax
     * under BMSP_PRUNE_ROW_REL; tol = 0 drops the stored zeros a product or a sum leaves behind */
    bmSpMatrix<valueType> prune(double tol, int rule = BMSP_PRUNE_ABS, bool keep_diagonal = false, bool transposed_layout = false) const
    {
        bmsp_matrix_t t = nullptr;
        bmsp::check(bmsp_matrix_prune(h_, rule, tol, keep_diagonal ? BMSP_PRUNE_KEEP_DIAGONAL : 0, transposed_layout ? 1 : 0, nullptr, &t, nullptr));
        bmSpMatrix<valueType> out;
        out.reset(t);
        return out;
    }

    /* the stored entries with lo <= col - row <= hi (complement: the others) as a new matrix (bmsp_matrix_select_band); BMSP_BAND_MIN /
     * BMSP_BAND_MAX leave a side unbounded.  tril(k) = band(MIN, k), triu(k) = band(k, MAX); no value is read */
    bmSpMatrix<valueType> band(int64_t lo, int64_t hi, bool complement = false, bool transposed_layout = false) const
    {
        bmsp_matrix_t t = nullptr;
        bmsp::check(bmsp_matrix_select_band(h_, lo, hi, complement ? BMSP_SELECT_COMPLEMENT : 0, transposed_layout ? 1 : 0, nullptr, &t, nullptr));
        bmSpMatrix<valueType> out;
        out.reset(t);
        return out;
    }
    bmSpMatrix<valueType> tril(int64_t k = 0, bool transposed_layout = false) const { return band(BMSP_BAND_MIN, k, false, transposed_layout); }
    bmSpMatrix<valueType> triu(int64_t k = 0, bool transposed_layout = false) const { return band(k, BMSP_BAND_MAX, false, transposed_layout); }
    /* the stored entries at the coordinates M stores (complement: does not store) as a new matrix (bmsp_matrix_select_mask); M has this
     * matrix's shape, any value type and either layout, its values are never read */
    template <class maskType>
    bmSpMatrix<valueType> mask(const bmSpMatrix<maskType> &M, bool complement = false, bool transposed_layout = false) const
    {
        bmsp_matrix_t t = nullptr;
        bmsp::check(bmsp_matrix_select_mask(h_, M.handle(), complement ? BMSP_SELECT_COMPLEMENT : 0, transposed_layout ? 1 : 0, nullptr, &t, nullptr));
        bmSpMatrix<valueType> out;
        out.reset(t);
        return out;
    }

    /* the diagonal as a device vector of min(num_rows, num_cols) entries, +0 where (i, i) is not stored (bmsp_matrix_diagonal) */
    bmsp::device_vector<typename bmsp::vector_of<valueType>::type> diagonal() const
    {
        bmsp::device_vector<typename bmsp::vector_of<valueType>::type> d((size_t)(num_rows < num_cols ? num_rows : num_cols));
        bmsp::check(bmsp_matrix_diagonal(h_, d.data(), nullptr));
        bmsp::check(bmsp_synchronize());
        return d;
    }
    /* diag(left) * this * diag(right) as a new matrix (bmsp_matrix_scale): device vectors of num_rows / num_cols entries, a null one
     * skips its side; flags = BMSP_SCALE_DIV_LEFT | BMSP_SCALE_DIV_RIGHT divides by that side instead */
    bmSpMatrix<valueType> scale(const typename bmsp::vector_of<valueType>::type *left, const typename bmsp::vector_of<valueType>::type *right,
                                int flags = 0, bool transposed_layout = false) const
    {
        bmsp_matrix_t t = nullptr;
        bmsp::check(bmsp_matrix_scale(h_, left, right, flags, transposed_layout ? 1 : 0, nullptr, &t));
        bmsp::check(bmsp_synchronize());
        bmSpMatrix<valueType> out;
        out.reset(t);
        return out;
    }
    /* the same into this matrix's own values (bmsp_matrix_scale_values with out == A) */
    void scale_inplace(const typename bmsp::vector_of<valueType>::type *left, const typename bmsp::vector_of<valueType>::type *right, int flags = 0)
    {
        bmsp::check(bmsp_matrix_scale_values(h_, left, right, flags, h_, nullptr));
        bmsp::check(bmsp_synchronize());
    }

    /* src/bmSpMatrix.cu:320-363 */
    void generate_coo()
    {
        coo.num_rows = (size_t)num_rows; coo.num_cols = (size_t)num_cols; coo.num_entries = (size_t)nnz;
        coo.row_indices.resize((size_t)nnz); coo.column_indices.resize((size_t)nnz); coo.values.resize((size_t)nnz);
        if (h_) bmsp::check(bmsp_matrix_to_coo_host(h_, coo.row_indices.data(), coo.column_indices.data(), coo.values.data()));
    }
    const bmsp::coo_matrix<double> &host_coo()
    {
        if (coo.num_entries == 0) generate_coo();
        return coo;
    }
    /* src/bmSpMatrix.cu:381-432: prints "Final: <mean relative error>" and returns true */
    template <class T> bool compare(const bmsp::coo_matrix<T> &other)
    {
        std::vector<double> v(other.values.begin(), other.values.end());
        double err = 0; int64_t missing = 0;
        bmsp::check(bmsp_matrix_compare(h_, (int64_t)other.num_entries, other.row_indices.data(), other.column_indices.data(), v.data(),
                                        &err, &missing));
        std::printf("Final: %g", err);
        return true;
    }
    void print()
    {
        const bmsp::coo_matrix<double> &c = host_coo();
        std::printf("sparse matrix <%d, %d> with %d entries\n", num_rows, num_cols, nnz);
        for (size_t i = 0; i < c.num_entries; i++) std::printf(" %d %d %g\n", c.row_indices[i], c.column_indices[i], c.values[i]);
    }
};

/* src/bmSparse_SPMV.cu:191-230.  v, u are device pointers; synchronous like the reference (cudaDeviceSynchronize, :223). */
template <class ValueIn, class ValueOut> inline void bmSparse_SpMV(bmSpMatrix<ValueIn> &A, ValueIn *v, ValueOut *u, bool batched)
{
    static_assert(std::is_same<ValueOut, float>::value || std::is_same<ValueOut, double>::value, "u is float (double for double input)");
    bmsp::check(bmsp_spmv(A.handle(), v, u, batched ? BMSP_SPMV_BATCHED : BMSP_SPMV_DEFAULT, nullptr));
    bmsp::check(bmsp_synchronize());
}

/* u = alpha * op(A) * v + beta * u (bmsp_spmv_op), op = BMSP_OP_N or BMSP_OP_T, A in either tile layout: the transposed product without a
 * transposed copy.  v (the input length of op(A), A's value type) and u (the output length; float, double for double) are device pointers;
 * synchronous like bmSparse_SpMV. */
template <class ValueIn>
inline void bmSparse_SpMV_op(bmSpMatrix<ValueIn> &A, int op, double alpha, const ValueIn *v, double beta, typename bmsp::vector_of<ValueIn>::type *u)
{
    bmsp::check(bmsp_spmv_op(A.handle(), op, alpha, v, beta, u, nullptr));
    bmsp::check(bmsp_synchronize());
}

/* Triangular solve (bmsp_spsv): op(tri(A)) * x = alpha * b, tri(A) the BMSP_FILL_LOWER / BMSP_FILL_UPPER triangle of the square A (named
 * before op), diag = BMSP_DIAG_NON_UNIT / BMSP_DIAG_UNIT, A in either tile layout.  b and x are device pointers to num_rows entries (float,
 * double for double) and may be the same; synchronous like bmSparse_SpMV.  bmSparse_SpSV_analyse builds the cached plan of (A, op, fill)
 * ahead of the first solve and reports it (info may be null). */
template <class ValueIn>
inline void bmSparse_SpSV(bmSpMatrix<ValueIn> &A, int op, int fill, int diag, double alpha, const typename bmsp::vector_of<ValueIn>::type *b,
                          typename bmsp::vector_of<ValueIn>::type *x)
{
    bmsp::check(bmsp_spsv(A.handle(), op, fill, diag, alpha, b, x, nullptr));
    bmsp::check(bmsp_synchronize());
}
template <class ValueIn>
inline void bmSparse_SpSV_analyse(bmSpMatrix<ValueIn> &A, int op, int fill, int diag, bmsp_spsv_info *info = nullptr)
{
    bmsp::check(bmsp_spsv_analyse(A.handle(), op, fill, diag, nullptr, info));
}

/* Iterative triangular solve (bmsp_spitsv): block-Jacobi sweeps towards the x of bmSparse_SpSV's system; op, fill, diag, alpha, b and x as
 * there, but x must not be b.  max_iter == 0 means levels + 1 of the plan (then tol == 0 returns bmSparse_SpSV's bits); tol > 0 stops at
 * max |x_new - x_old| <= tol * max |x_new|; tol == BMSP_ITSV_NO_CHECK runs exactly max_iter sweeps with nothing read back.  flags:
 * BMSP_ITSV_X0_GIVEN = x holds the initial iterate (default +0).  delta_history (host) and info may be null; synchronous like bmSparse_SpMV. */
template <class ValueIn>
inline void bmSparse_SpITSV(bmSpMatrix<ValueIn> &A, int op, int fill, int diag, double alpha, const typename bmsp::vector_of<ValueIn>::type *b,
                            typename bmsp::vector_of<ValueIn>::type *x, int64_t max_iter = 0, double tol = 0.0, int flags = 0,
                            double *delta_history = nullptr, bmsp_spitsv_info *info = nullptr)
{
    bmsp::check(bmsp_spitsv(A.handle(), op, fill, diag, alpha, b, x, max_iter, tol, flags, delta_history, info, nullptr));
    bmsp::check(bmsp_synchronize());
}

/* Incomplete factorisation ILU(0) by fixed-point sweeps (bmsp_matrix_ilu0 / bmsp_matrix_ilu0_values): F receives A's structure in the
 * layout asked for and holds L (unit diagonal, not stored) below the diagonal and U on and above it -- what bmSparse_SpSV(F, N, LOWER,
 * UNIT) followed by bmSparse_SpSV(F, N, UPPER, NON_UNIT) applies.  A must be square with every diagonal entry stored.  max_iter == 0
 * means 2 n (then tol == 0 returns the sequential ILU(0)'s bits); tol > 0 stops at max |f_new - f_old| <= tol * max |f_new|; tol ==
 * BMSP_ILU_NO_CHECK runs exactly max_iter sweeps with nothing read back.  The _values form writes into an F made from A by bmSparse_ILU0
 * or a layout-keeping maker, never into A; flags: BMSP_ILU_F0_GIVEN = start from F's current values (default: from A's).  delta_history
 * (host) and info may be null; synchronous like bmSparse_SpMV. */
template <class ValueIn>
inline void bmSparse_ILU0(bmSpMatrix<ValueIn> &A, bmSpMatrix<ValueIn> &F, int64_t max_iter = 0, double tol = 0.0, bool transposed_layout = false,
                          double *delta_history = nullptr, bmsp_ilu0_info *info = nullptr)
{
    bmsp_matrix_t f = nullptr;
    bmsp::check(bmsp_matrix_ilu0(A.handle(), max_iter, tol, transposed_layout ? 1 : 0, nullptr, &f, delta_history, info));
    bmsp::check(bmsp_synchronize());
    F.reset(f);
}
template <class ValueIn>
inline void bmSparse_ILU0_values(bmSpMatrix<ValueIn> &A, bmSpMatrix<ValueIn> &F, int64_t max_iter = 0, double tol = 0.0, int flags = 0,
                                 double *delta_history = nullptr, bmsp_ilu0_info *info = nullptr)
{
    bmsp::check(bmsp_matrix_ilu0_values(A.handle(), F.handle(), max_iter, tol, flags, nullptr, delta_history, info));
    bmsp::check(bmsp_synchronize());
}

/* Krylov solvers (bmsp_krylov_solve): op(A) * x = b for a square float or double A in either tile layout by preconditioned CG
 * (BMSP_KRYLOV_CG) or BiCGStab (BMSP_KRYLOV_BICGSTAB), the whole iteration enqueued on the device.  pc (may be null: none) names the
 * preconditioner: BMSP_PC_JACOBI, or BMSP_PC_ILU_EXACT / BMSP_PC_ILU_SWEEPS with pc->F = F.handle() of a factor from bmSparse_ILU0.  Stops at
 * dot(r, r) <= tol^2 * dot(b, b), after max_iter iterations (0: min(n, 2^20)) or on a breakdown (info->status); tol == BMSP_KRYLOV_NO_CHECK
 * runs exactly max_iter iterations with nothing read back.  flags: BMSP_KRYLOV_X0_GIVEN = x holds the initial iterate (default +0).
 * relres_history (host) and info may be null; synchronous like bmSparse_SpMV.  bmSparse_vec_dot is the solver's deterministic dot product
 * of two device vectors (bmsp_vec_dot), returned to the host. */
template <class ValueIn>
inline void bmSparse_solve(bmSpMatrix<ValueIn> &A, int op, int method, const bmsp_precond *pc, const typename bmsp::vector_of<ValueIn>::type *b,
                           typename bmsp::vector_of<ValueIn>::type *x, int64_t max_iter = 0, double tol = 1e-6, int flags = 0,
                           double *relres_history = nullptr, bmsp_krylov_info *info = nullptr)
{
    bmsp::check(bmsp_krylov_solve(A.handle(), op, method, pc, b, x, max_iter, tol, flags, relres_history, info, nullptr));
    bmsp::check(bmsp_synchronize());
}
/* Restarted GMRES (bmsp_gmres_solve): bmSparse_solve's arguments with the restart length (0: 30, at most 256) where the method stood; one
 * product and one preconditioner application per iteration, no recurrence to break down, for matrices that are not symmetric. */
template <class ValueIn>
inline void bmSparse_solve_gmres(bmSpMatrix<ValueIn> &A, int op, const bmsp_precond *pc, int restart,
                                 const typename bmsp::vector_of<ValueIn>::type *b, typename bmsp::vector_of<ValueIn>::type *x,
                                 int64_t max_iter = 0, double tol = 1e-6, int flags = 0, double *relres_history = nullptr,
                                 bmsp_krylov_info *info = nullptr)
{
    bmsp::check(bmsp_gmres_solve(A.handle(), op, pc, restart, b, x, max_iter, tol, flags, relres_history, info, nullptr));
    bmsp::check(bmsp_synchronize());
}
template <class R>
inline double bmSparse_vec_dot(int64_t n, const R *x, const R *y)
{
    static_assert(sizeof(R) == 4 || sizeof(R) == 8, "float or double vectors");
    bmsp::device_vector<double> out(1);
    bmsp::check(bmsp_vec_dot(n, sizeof(R) == 8 ? 1 : 0, x, y, out.data(), nullptr));
    bmsp::check(bmsp_synchronize());
    return out.to_host()[0];
}

/* Multigrid on the device (bmsp_mg_create / bmsp_mg_vcycle / bmsp_mg_solve): the V-cycle of a hierarchy of float or double matrices, and CG
 * / BiCGStab for A[0] * x = b preconditioned by one cycle.  A holds the level operators, P the prolongators (one fewer), R the restrictions
 * (empty, or null entries: restrict by P^T), coarse_inv (may be null) the dense inverse of the coarsest operator on the device, n_c x n_c
 * row-major at leading dimension ld_inv (0: n_c), of the vector type.  The matrices are borrowed: they must outlive the object.  vcycle: z =
 * one cycle for r from z = 0 (device pointers, z != r); solve: bmSparse_solve's arguments; both synchronous like bmSparse_SpMV. */
template <class valueType> class bmSpMultigrid {
    bmsp_mg_t h_ = nullptr;

public:
    typedef typename bmsp::vector_of<valueType>::type vectorType;
    bmSpMultigrid(const std::vector<bmSpMatrix<valueType> *> &A, const std::vector<bmSpMatrix<valueType> *> &P,
                  const std::vector<bmSpMatrix<valueType> *> &R = std::vector<bmSpMatrix<valueType> *>(), const vectorType *coarse_inv = nullptr,
                  int64_t ld_inv = 0, double omega = 2.0 / 3.0, int pre = 1, int post = 1)
    {
        std::vector<bmsp_matrix_t> a, p, r;
        for (size_t l = 0; l < A.size(); l++) a.push_back(A[l] ? A[l]->handle() : nullptr);
        for (size_t l = 0; l < P.size(); l++) p.push_back(P[l] ? P[l]->handle() : nullptr);
        for (size_t l = 0; l < R.size(); l++) r.push_back(R[l] ? R[l]->handle() : nullptr);
        if (P.size() + 1 != A.size() || (!R.empty() && R.size() != P.size())) throw std::runtime_error("bmSpMultigrid: P (and R) hold one operator fewer than A");
        if (ld_inv == 0 && !A.empty() && A.back()) ld_inv = A.back()->num_rows;
        bmsp::check(bmsp_mg_create((int)a.size(), a.data(), p.empty() ? nullptr : p.data(), r.empty() ? nullptr : r.data(), coarse_inv, ld_inv,
                                   omega, pre, post, nullptr, &h_));
    }
    bmSpMultigrid(const bmSpMultigrid &) = delete;
    bmSpMultigrid &operator=(const bmSpMultigrid &) = delete;
    ~bmSpMultigrid() { if (h_) bmsp_mg_free(h_); }
    bmsp_mg_t handle() const { return h_; }
    void info(bmsp_mg_info_t *out) const { bmsp::check(bmsp_mg_info(h_, out)); }
    void vcycle(const vectorType *r, vectorType *z)
    {
        bmsp::check(bmsp_mg_vcycle(h_, r, z, nullptr));
        bmsp::check(bmsp_synchronize());
    }
    void solve(int method, const vectorType *b, vectorType *x, int64_t max_iter = 0, double tol = 1e-6, int flags = 0,
               double *relres_history = nullptr, bmsp_krylov_info *info = nullptr)
    {
        bmsp::check(bmsp_mg_solve(h_, method, b, x, max_iter, tol, flags, relres_history, info, nullptr));
        bmsp::check(bmsp_synchronize());
    }
    // GMRES(restart) preconditioned by one cycle (bmsp_mg_solve_gmres): any cycle, symmetric or not
    void solve_gmres(int restart, const vectorType *b, vectorType *x, int64_t max_iter = 0, double tol = 1e-6, int flags = 0,
                     double *relres_history = nullptr, bmsp_krylov_info *info = nullptr)
    {
        bmsp::check(bmsp_mg_solve_gmres(h_, restart, b, x, max_iter, tol, flags, relres_history, info, nullptr));
        bmsp::check(bmsp_synchronize());
    }
};

/* FSAI (bmsp_matrix_fsai / bmsp_fsai_*): bmSparse_fsai makes G, the factorised sparse approximate inverse of op(A) on the lower-triangular
 * pattern of S (every row stores its diagonal, nothing to its right and at most 64 entries), scaled by BMSP_FSAI_SCALE_NONE / _SQRT /
 * _UNIT; pivot (may be null) takes the n values y_m on the device.  bmSpFsai is the preconditioner z = G2^T (G1 r) by two sparse products:
 * kind BMSP_FSAI_SPD (CG may use it) or BMSP_FSAI_GENERAL, flags BMSP_FSAI_NO_MATERIALISE | BMSP_FSAI_COLMAJOR.  A is borrowed and must
 * outlive the object; S may go after construction.  apply: z != r, device pointers; solve / solve_gmres: bmSparse_solve's and
 * bmSparse_solve_gmres's arguments; update: new factor values after a value update of A.  Synchronous like bmSparse_SpMV. */
template <class ValueIn, class ValueS>
inline void bmSparse_fsai(bmSpMatrix<ValueIn> &A, int op, bmSpMatrix<ValueS> &S, bmSpMatrix<ValueIn> &G, int scale = BMSP_FSAI_SCALE_SQRT,
                          bool transposed_layout = false, typename bmsp::vector_of<ValueIn>::type *pivot = nullptr, bmsp_fsai_info *info = nullptr)
{
    bmsp_matrix_t g = nullptr;
    bmsp_fsai_info local;
    bmsp::check(bmsp_matrix_fsai(A.handle(), op, S.handle(), scale, transposed_layout ? 1 : 0, pivot, nullptr, &g, info ? info : &local));
    G.reset(g);
}
template <class valueType> class bmSpFsai {
    bmsp_fsai_t h_ = nullptr;

public:
    typedef typename bmsp::vector_of<valueType>::type vectorType;
    template <class ValueS>
    bmSpFsai(bmSpMatrix<valueType> &A, bmSpMatrix<ValueS> &S, int kind = BMSP_FSAI_SPD, int flags = 0)
    {
        bmsp::check(bmsp_fsai_create(A.handle(), S.handle(), kind, flags, nullptr, &h_));
    }
    bmSpFsai(const bmSpFsai &) = delete;
    bmSpFsai &operator=(const bmSpFsai &) = delete;
    ~bmSpFsai() { if (h_) bmsp_fsai_free(h_); }
    bmsp_fsai_t handle() const { return h_; }
    void info(bmsp_fsai_handle_info *out) const { bmsp::check(bmsp_fsai_get_info(h_, out)); }
    void update() { bmsp::check(bmsp_fsai_update(h_, nullptr)); }
    void apply(const vectorType *r, vectorType *z)
    {
        bmsp::check(bmsp_fsai_apply(h_, r, z, nullptr));
        bmsp::check(bmsp_synchronize());
    }
    void solve(int method, const vectorType *b, vectorType *x, int64_t max_iter = 0, double tol = 1e-6, int flags = 0,
               double *relres_history = nullptr, bmsp_krylov_info *info = nullptr)
    {
        bmsp::check(bmsp_fsai_solve(h_, method, b, x, max_iter, tol, flags, relres_history, info, nullptr));
        bmsp::check(bmsp_synchronize());
    }
    void solve_gmres(int restart, const vectorType *b, vectorType *x, int64_t max_iter = 0, double tol = 1e-6, int flags = 0,
                     double *relres_history = nullptr, bmsp_krylov_info *info = nullptr)
    {
        bmsp::check(bmsp_fsai_solve_gmres(h_, restart, b, x, max_iter, tol, flags, relres_history, info, nullptr));
        bmsp::check(bmsp_synchronize());
    }
};

/* Block multi-colour ordering and block permutation (bmsp_matrix_color_blocks / bmsp_matrix_permute_blocks / bmsp_vec_permute_blocks).
 * bmSparse_color_blocks: the greedy colouring of the block-row graph of a square A by hashed priorities into colors and the ordering by
 * colour class into perm (new -> old), both resized to ceil(num_rows / 8); the triangles of bmSparse_permute_blocks(A, perm, perm, B)
 * have at most info->colors levels.  bmSparse_permute_blocks: B = P * A * Q^T at tile granularity, null = the identity.
 * bmSparse_vec_permute_blocks: y[8 i + r] = x[8 perm[i] + r], or with inverse y[8 perm[i] + r] = x[8 i + r], on device vectors of n
 * entries; y must not be x.  Synchronous like bmSparse_SpMV. */
template <class ValueIn>
inline void bmSparse_color_blocks(bmSpMatrix<ValueIn> &A, bmsp::device_vector<uint32_t> &colors, bmsp::device_vector<uint32_t> &perm,
                                  uint64_t seed = 0, bmsp_color_info *info = nullptr)
{
    const size_t nb = ((size_t)A.num_rows + 7) / 8;
    colors = bmsp::device_vector<uint32_t>(nb);
    perm = bmsp::device_vector<uint32_t>(nb);
    bmsp::check(bmsp_matrix_color_blocks(A.handle(), seed, colors.data(), perm.data(), nullptr, info));
    bmsp::check(bmsp_synchronize());
}
template <class valueType>
inline void bmSparse_permute_blocks(bmSpMatrix<valueType> &A, const uint32_t *row_perm, const uint32_t *col_perm, bmSpMatrix<valueType> &B,
                                    bool transposed_layout = false)
{
    bmsp_matrix_t b = nullptr;
    bmsp::check(bmsp_matrix_permute_blocks(A.handle(), row_perm, col_perm, transposed_layout ? 1 : 0, nullptr, &b));
    B.reset(b);
}
template <class R>
inline void bmSparse_vec_permute_blocks(int64_t n, const uint32_t *perm, const R *x, R *y, bool inverse = false)
{
    static_assert(sizeof(R) == 4 || sizeof(R) == 8, "float or double vectors");
    bmsp::check(bmsp_vec_permute_blocks(n, sizeof(R) == 8 ? 1 : 0, perm, inverse ? 1 : 0, x, y, nullptr));
    bmsp::check(bmsp_synchronize());
}

/* MIS(2) aggregation of the scalar graph of a square S by hashed priorities (bmsp_matrix_aggregate): agg is resized to num_rows and holds
 * every row's aggregate; returns the number of aggregates.  Structure only: a pure function of S's pattern and the seed.  Synchronous. */
template <class ValueIn>
inline int64_t bmSparse_aggregate(bmSpMatrix<ValueIn> &S, bmsp::device_vector<uint32_t> &agg, uint64_t seed = 0,
                                  bmsp_aggregate_info *info = nullptr)
{
    int64_t count = 0;
    agg = bmsp::device_vector<uint32_t>((size_t)S.num_rows);
    bmsp::check(bmsp_matrix_aggregate(S.handle(), seed, agg.data(), &count, nullptr, info));
    return count;
}

/* Triangular solve for k right-hand sides (bmsp_spsm): op(tri(A)) * X = alpha * B; op, fill and diag as for bmSparse_SpSV.  B and X are
 * device pointers to num_rows x k row-major arrays at leading dimensions ldb, ldx >= k (float, double for double); they may be the same
 * when ldb == ldx.  Column c of X holds the bits bmSparse_SpSV writes for column c of B, for one walk of the dependency chain instead of
 * k; synchronous like bmSparse_SpMV.  bmSparse_SpSM_launch_info reports what that call launches (it builds the shared plan if missing). */
template <class ValueIn>
inline void bmSparse_SpSM(bmSpMatrix<ValueIn> &A, const typename bmsp::vector_of<ValueIn>::type *B, int64_t ldb,
                          typename bmsp::vector_of<ValueIn>::type *X, int64_t ldx, int k, int op, int fill, int diag, double alpha)
{
    bmsp::check(bmsp_spsm(A.handle(), op, fill, diag, alpha, B, ldb, X, ldx, k, nullptr));
    bmsp::check(bmsp_synchronize());
}
template <class ValueIn>
inline void bmSparse_SpSM_launch_info(bmSpMatrix<ValueIn> &A, int op, int fill, int diag, int k, int64_t ldb, int64_t ldx, bmsp_spsm_info *info)
{
    bmsp::check(bmsp_spsm_launch_info(A.handle(), op, fill, diag, k, ldb, ldx, nullptr, info));
}

/* Multi-vector form: U = A * V for k vectors, V row-major num_cols x k, U row-major num_rows x k. */
template <class ValueIn, class ValueOut> inline void bmSparse_SpMM(bmSpMatrix<ValueIn> &A, ValueIn *V, ValueOut *U, int k)
{
    static_assert(std::is_same<ValueOut, float>::value || std::is_same<ValueOut, double>::value, "U is float (double for double input)");
    bmsp::check(bmsp_spmm(A.handle(), V, k, U, k, k, nullptr));
    bmsp::check(bmsp_synchronize());
}

/* Y = alpha * op(A) * X + beta * Y for k vectors (bmsp_spmm_op), op = BMSP_OP_N or BMSP_OP_T, A in either tile layout: the transposed
 * multi-vector product without a transposed copy.  X (input length of op(A) x k, A's value type, leading dimension ldx) and Y (output
 * length x k; float, double for double; leading dimension ldy) are row-major device pointers; synchronous like bmSparse_SpMV. */
template <class ValueIn>
inline void bmSparse_SpMM_op(bmSpMatrix<ValueIn> &A, int op, double alpha, const ValueIn *X, int64_t ldx, double beta,
                             typename bmsp::vector_of<ValueIn>::type *Y, int64_t ldy, int k)
{
    bmsp::check(bmsp_spmm_op(A.handle(), op, alpha, X, ldx, beta, Y, ldy, k, nullptr));
    bmsp::check(bmsp_synchronize());
}

/* src/bmSparse_SPGEMM.cu:827-1223.  `mode` is the reference's `segmented` flag (declared bool there). */
template <class valueIn, class valueOut>
inline void bmSparse_mult(bmSpMatrix<valueIn> &A, bmSpMatrix<valueIn> &B, bmSpMatrix<valueOut> &C, bool mode, bool VERBOSE, long tc_version,
                          bmsp_spgemm_stats *stats = nullptr)
{
    bmsp_matrix_t c = nullptr;
    bmsp_spgemm_stats st;
    bmsp::check(bmsp_spgemm(A.handle(), B.handle(), &c, mode ? BMSP_SORT_SEGMENTED : BMSP_SORT_AUTO, (int)tc_version, VERBOSE ? 1 : 0, nullptr, &st));
    C.reset(c);
    if (stats) *stats = st;
    std::printf("Toda F: %lld \xce\xbcs \n", (long long)(st.t_us[0] + 0.5)); /* :1220 */
}

/* The two halves of bmSparse_mult for repeated products on one sparsity pattern (bmsp_spgemm_symbolic / bmsp_spgemm_numeric; the reference
 * runs both halves in every call, src/bmSparse_SPGEMM.cu:849-1158): _symbolic leaves C with the product's structure and zero values,
 * _numeric overwrites the values of a C of that structure with those of A x B. */
template <class valueIn, class valueOut>
inline void bmSparse_mult_symbolic(bmSpMatrix<valueIn> &A, bmSpMatrix<valueIn> &B, bmSpMatrix<valueOut> &C, bool mode, long tc_version,
                                   bmsp_spgemm_stats *stats = nullptr)
{
    bmsp_matrix_t c = nullptr;
    bmsp::check(bmsp_spgemm_symbolic(A.handle(), B.handle(), &c, mode ? BMSP_SORT_SEGMENTED : BMSP_SORT_AUTO, (int)tc_version, nullptr, stats));
    C.reset(c);
}
template <class valueIn, class valueOut>
inline void bmSparse_mult_numeric(bmSpMatrix<valueIn> &A, bmSpMatrix<valueIn> &B, bmSpMatrix<valueOut> &C, long tc_version, bmsp_spgemm_stats *stats = nullptr)
{
    bmsp::check(bmsp_spgemm_numeric(A.handle(), B.handle(), C.handle(), (int)tc_version, nullptr, stats));
}

/* C = alpha*A + beta*B (bmsp_matrix_add): C's tiles column-major when transposed_layout.  A and B share shape and value type; either
 * layout.  _values re-computes C's values after A's or B's values changed in place (same structures, same order; bmsp_matrix_add_values). */
template <class valueType>
inline void bmSparse_add(double alpha, bmSpMatrix<valueType> &A, double beta, bmSpMatrix<valueType> &B, bmSpMatrix<valueType> &C,
                         bool transposed_layout = false)
{
    bmsp_matrix_t c = nullptr;
    bmsp::check(bmsp_matrix_add(alpha, A.handle(), beta, B.handle(), transposed_layout ? 1 : 0, nullptr, &c));
    C.reset(c);
}
template <class valueType>
inline void bmSparse_add_values(double alpha, bmSpMatrix<valueType> &A, double beta, bmSpMatrix<valueType> &B, bmSpMatrix<valueType> &C)
{
    bmsp::check(bmsp_matrix_add_values(alpha, A.handle(), beta, B.handle(), C.handle(), nullptr));
}

/* C = A without the stored entries the rule drops (bmsp_matrix_prune), C's tiles column-major when transposed_layout; stats (optional)
 * receives the entry and tile counts before and after. */
template <class valueType>
inline void bmSparse_prune(bmSpMatrix<valueType> &A, bmSpMatrix<valueType> &C, double tol, int rule = BMSP_PRUNE_ABS, bool keep_diagonal = false,
                           bool transposed_layout = false, bmsp_prune_stats *stats = nullptr)
{
    bmsp_matrix_t c = nullptr;
    bmsp::check(bmsp_matrix_prune(A.handle(), rule, tol, keep_diagonal ? BMSP_PRUNE_KEEP_DIAGONAL : 0, transposed_layout ? 1 : 0, nullptr, &c, stats));
    C.reset(c);
}

/* C = the stored entries of A with lo <= col - row <= hi (bmsp_matrix_select_band) / at the coordinates M stores (bmsp_matrix_select_mask),
 * or with `complement` the others; C's tiles column-major when transposed_layout; stats (optional) receives the entry and tile counts
 * before and after. */
template <class valueType>
inline void bmSparse_select_band(bmSpMatrix<valueType> &A, bmSpMatrix<valueType> &C, int64_t lo, int64_t hi, bool complement = false,
                                 bool transposed_layout = false, bmsp_select_stats *stats = nullptr)
{
    bmsp_matrix_t c = nullptr;
    bmsp::check(bmsp_matrix_select_band(A.handle(), lo, hi, complement ? BMSP_SELECT_COMPLEMENT : 0, transposed_layout ? 1 : 0, nullptr, &c, stats));
    C.reset(c);
}
template <class valueType, class maskType>
inline void bmSparse_select_mask(bmSpMatrix<valueType> &A, bmSpMatrix<maskType> &M, bmSpMatrix<valueType> &C, bool complement = false,
                                 bool transposed_layout = false, bmsp_select_stats *stats = nullptr)
{
    bmsp_matrix_t c = nullptr;
    bmsp::check(bmsp_matrix_select_mask(A.handle(), M.handle(), complement ? BMSP_SELECT_COMPLEMENT : 0, transposed_layout ? 1 : 0, nullptr, &c, stats));
    C.reset(c);
}

/* Diagonal operations (bmsp_matrix_diagonal / _from_diagonal / _scale): d = diag(A) as a device vector (resized to min(num_rows,
 * num_cols)); C = the num_rows x num_cols matrix with d[i] at every (i, i); C = diag(left) * A * diag(right), a null side skipped. */
template <class valueType>
inline void bmSparse_diagonal(bmSpMatrix<valueType> &A, bmsp::device_vector<typename bmsp::vector_of<valueType>::type> &d)
{
    d = A.diagonal();
}
template <class valueType>
inline void bmSparse_from_diagonal(const bmsp::device_vector<typename bmsp::vector_of<valueType>::type> &d, bmSpMatrix<valueType> &C, int num_rows = -1,
                                   int num_cols = -1, bool transposed_layout = false)
{
    bmsp_matrix_t c = nullptr;
    bmsp::check(bmsp_matrix_from_diagonal(num_rows < 0 ? (int)d.size() : num_rows, num_cols < 0 ? (int)d.size() : num_cols, d.data(),
                                          bmsp::dtype_of<valueType>::value, transposed_layout ? 1 : 0, nullptr, &c));
    bmsp::check(bmsp_synchronize());
    C.reset(c);
}
template <class valueType>
inline void bmSparse_scale(bmSpMatrix<valueType> &A, const typename bmsp::vector_of<valueType>::type *left,
                           const typename bmsp::vector_of<valueType>::type *right, bmSpMatrix<valueType> &C, int flags = 0,
                           bool transposed_layout = false)
{
    C = A.scale(left, right, flags, transposed_layout);
}
/* SDDMM (bmsp_sddmm / bmsp_sddmm_values): C = alpha * (X . Y^T) on S's pattern + beta * S, or alpha * (X . Y^T) * S under flags =
 * BMSP_SDDMM_MUL_S (beta must then be 0).  X (num_rows x k) and Y (num_cols x k) are row-major device pointers of S's value type at
 * leading dimensions ldx / ldy (<= 0: k).  C receives S's structure in the layout asked for; the _values form writes into S itself (C is
 * S) or into a C made from S by bmSparse_sddmm, bmSparse_scale or with_layout.  Synchronous like bmSparse_scale. */
template <class valueType>
inline void bmSparse_sddmm(bmSpMatrix<valueType> &S, const valueType *X, const valueType *Y, int k, bmSpMatrix<valueType> &C, double alpha = 1.0,
                           double beta = 0.0, int flags = 0, bool transposed_layout = false, int64_t ldx = 0, int64_t ldy = 0)
{
    bmsp_matrix_t c = nullptr;
    bmsp::check(bmsp_sddmm(S.handle(), X, ldx > 0 ? ldx : k, Y, ldy > 0 ? ldy : k, k, alpha, beta, flags, transposed_layout ? 1 : 0, nullptr, &c));
    bmsp::check(bmsp_synchronize());
    C.reset(c);
}
template <class valueType>
inline void bmSparse_sddmm_values(bmSpMatrix<valueType> &S, const valueType *X, const valueType *Y, int k, bmSpMatrix<valueType> &C,
                                  double alpha = 1.0, double beta = 0.0, int flags = 0, int64_t ldx = 0, int64_t ldy = 0)
{
    bmsp::check(bmsp_sddmm_values(S.handle(), X, ldx > 0 ? ldx : k, Y, ldy > 0 ? ldy : k, k, alpha, beta, flags, C.handle(), nullptr));
    bmsp::check(bmsp_synchronize());
}

/* Masked SpGEMM (bmsp_spgemm_masked / bmsp_spgemm_masked_values): C = alpha * (A * B) on M's pattern + beta * M, or alpha * (A * B) * M
 * under flags = BMSP_MASKED_MUL_M (beta must then be 0).  A, B and M may have either tile layout and may be the same matrix; M and C have
 * A's value type, or float for half operands.  C receives M's structure in the layout asked for; the _values form writes into M itself (C
 * is M) or into a C made from M by bmSparse_mult_masked, bmSparse_sddmm, bmSparse_scale or with_layout, never into A or B.  Synchronous
 * like bmSparse_sddmm. */
template <class valueIn, class valueOut>
inline void bmSparse_mult_masked(bmSpMatrix<valueIn> &A, bmSpMatrix<valueIn> &B, bmSpMatrix<valueOut> &M, bmSpMatrix<valueOut> &C,
                                 double alpha = 1.0, double beta = 0.0, int flags = 0, bool transposed_layout = false)
{
    bmsp_matrix_t c = nullptr;
    bmsp::check(bmsp_spgemm_masked(A.handle(), B.handle(), M.handle(), alpha, beta, flags, transposed_layout ? 1 : 0, nullptr, &c));
    bmsp::check(bmsp_synchronize());
    C.reset(c);
}
template <class valueIn, class valueOut>
inline void bmSparse_mult_masked_values(bmSpMatrix<valueIn> &A, bmSpMatrix<valueIn> &B, bmSpMatrix<valueOut> &M, bmSpMatrix<valueOut> &C,
                                        double alpha = 1.0, double beta = 0.0, int flags = 0)
{
    bmsp::check(bmsp_spgemm_masked_values(A.handle(), B.handle(), M.handle(), alpha, beta, flags, C.handle(), nullptr));
    bmsp::check(bmsp_synchronize());
}

/* The same product sharded over one process per GPU (bmsp_spgemm_sharded): every rank passes the same A and B, multiplies
 * its block-row panel of A and returns the whole C. */
template <class valueIn, class valueOut>
inline void bmSparse_mult_sharded(bmsp_comm_t comm, bmSpMatrix<valueIn> &A, bmSpMatrix<valueIn> &B, bmSpMatrix<valueOut> &C, bool mode, bool VERBOSE,
                                  long tc_version, bmsp_spgemm_stats *stats = nullptr, bmsp_shard_stats *shard = nullptr)
{
    bmsp_matrix_t c = nullptr;
    bmsp_spgemm_stats st;
    bmsp::check(bmsp_spgemm_sharded(comm, A.handle(), B.handle(), &c, mode ? BMSP_SORT_SEGMENTED : BMSP_SORT_AUTO, (int)tc_version, VERBOSE ? 1 : 0,
                                    nullptr, &st, shard));
    C.reset(c);
    if (stats) *stats = st;
    std::printf("Toda F: %lld \xce\xbcs \n", (long long)(st.t_us[0] + 0.5));
}

#endif /* BMSPMATRIX_H_ */
