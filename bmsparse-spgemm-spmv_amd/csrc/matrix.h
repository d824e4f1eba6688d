// matrix.h -- the device-resident bmSparse container behind bmsp_matrix_t
// (class bmSpMatrix<T>, reference include/bmSpMatrix.h:20-40).
#ifndef BMSP_MATRIX_H_
#define BMSP_MATRIX_H_

#include "mac_choice.h"
#include "runtime.h"
#include <memory>
#include <utility>
#include <vector>

struct bmsp_matrix_s;
namespace bmsp {
uint64_t next_matrix_uid();
// a matrix under construction, a view made per call, or one kept by another handle: freed with everything it holds unless released
using MatrixPtr = std::unique_ptr<bmsp_matrix_s>;
}  // namespace bmsp

// The cached view of bmsp_spmv_op for one op (spmv_op.hip): the tiles as 16-byte records {bitmap lo, hi, value offset, the tile's OTHER
// block index} in the order the sweep walks them, the pointer of blocks + 1 entries per output block (op T; op N uses rowptr), the work
// items {output block, first tile, end tile, scratch slot or ~0u}, the fold list {output block, first slot, parts} of the split blocks and
// 8 accumulators of scratch per slot -- one allocation, structure only (kept across value-only invalidation).
struct bmsp_spmv_op_view {
    bmsp::DevBuf<uint32_t> mem;
    size_t off_ptr = 0, off_items = 0, off_folds = 0, off_scratch = 0, bytes = 0;
    int64_t blocks = 0, items = 0, split_blocks = 0, slots = 0;
};

// The cached plan of bmsp_spsv for one (op, fill) (spsv.hip), structure only: on the device the output blocks ordered by (level, index)
// and the level pointer (one allocation); on the host the level pointer again and the launch schedule {first level, end level, kind (0 one
// level kernel, 1 one chain kernel)}, three words per launch.  missing_diag_row: the first row below n whose diagonal entry A does not
// store (-1: none) -- what a BMSP_DIAG_NON_UNIT call is refused for.
struct bmsp_spsv_plan_s {
    bmsp::DevBuf<uint32_t> mem;
    size_t off_level_ptr = 0, bytes = 0;
    int64_t blocks = 0, levels = 0, max_level_width = 0, chain_launches = 0, chained_levels = 0, chain = 0, missing_diag_row = -1;
    std::vector<uint32_t> level_ptr, segments;
};

// What the operators derive from a handle's four arrays and cache on it is built lazily, is never part of the reference's public state, and
// lives in two groups.  Every member's initialiser is its "not built" value and every allocation has an owner, so a group is dropped by
// assigning a fresh one (bmsp_matrix_s::reset_*): a new cache needs its line here and nowhere else.

// Derived from the VALUES (and the structure): dropped by bmsp_matrix_invalidate(m, 0) and before an operation rewrites the values in place.
struct bmsp_value_caches {
    // fp16 matrices: every tile expanded to 64 halves in position order (128 B per block), for the K = 32 MFMA block-MAC: built lazily
    bmsp::DevBuf<void> dense_tiles;
    bmsp::DevBuf<uint32_t> csr_rowptr, csr_ent;  // fp32 operands of the row-sparse block-MAC: a row-major CSR copy (row pointer of num_rows + 1 entries; {column, value bits} per stored value)
    bmsp::DevBuf<void> lane_tiles;   // fp32 matrices: tiles in the lane order of the fp32 MFMA block-MAC (256 B per block): built lazily
    int values_finite = -1;          // fp16 operands of the strip block-MAC: 1 = no inf / NaN stored (-1 = not looked yet)
    int f32_exp_min = 255, f32_exp_max = 0;  // fp32: biased exponent range of the non-zero stored values (with values_finite)
    bool holds_memory() const { return dense_tiles || lane_tiles || csr_rowptr || csr_ent; }
};

// Derived from the STRUCTURE alone (keys, bitmaps, offsets): kept across value-only invalidation, dropped by bmsp_matrix_invalidate(m, 1).
struct bmsp_structure_caches {
    bmsp::DevBuf<uint32_t> rowptr;  // dense block-row pointer, num_block_rows()+1 entries
    int64_t rowptr_rows = 0;
    int64_t max_row_blocks = -1;  // most blocks in one block-row (ensure_row_stats; bounds the SpGEMM's task segments without a read-back)
    // sweep plan of the SpMV (see spmv.hip): chunk descriptors
    bmsp::DevBuf<uint32_t> spmv_chunks;
    int64_t spmv_num_chunks = 0;
    int64_t spmv_plan_long = 0;
    int64_t spmv_full_tiles = 0;  // tiles with all 64 values stored (decides the sweep variant)
    size_t spmv_plan_off_cnt = 0, spmv_plan_off_carry = 0;
    // position cache of the value-stream SpMV: one 16-bit {tile slot in its batch, position in the tile} entry per stored value
    bmsp::DevBuf<uint16_t> spmv_pos;
    uint32_t *spmv_tinfo = nullptr;  // same allocation: per tile {block column, block-row inside its item's window} (the value-stream kernel's slot word)
    uint16_t *spmv_eoff = nullptr;   // same allocation: per tile, end of its values relative to its item's first value
    int64_t spmv_pos_base = 0, spmv_pos_count = 0;
    int spmv_pos_tried = 0;
    // chunked sweep (spmv_chunk_kernel): one 32-bit word {row relative to the chunk's first block-row, column} per stored value, padded to
    // whole chunks | chunk records | arrival counters | carry slots -- one allocation, structure only (kept across value-only invalidation).
    // spmv_cw_layout: 1 = the words in storage order (round 7), 2 = row-sorted words {column, storage index, run start, window bitmap bits}
    bmsp::DevBuf<uint32_t> spmv_cw;
    int64_t spmv_cw_chunks = 0, spmv_cw_split = 0;  // chunks; block-rows folded across chunks
    size_t spmv_cw_off_rec = 0, spmv_cw_off_cnt = 0, spmv_cw_off_carry = 0;
    int spmv_cw_colbits = 0, spmv_cw_tried = 0, spmv_cw_layout = 0;
    // (bitmap, value offset) of every block as one 16-byte record, for kernels that gather both (block-MAC): built lazily
    bmsp::DevBuf<uint32_t> block_meta;  // block_num x {bmp lo, bmp hi, offset in elements, 0}
    bmsp::DevBuf<uint32_t> sym_recs;    // right operands: block_num x {bitmap ROW-major (lo, hi), block column, rows the tile uses}: all the column-window passes (rowwindow.hip) read per candidate pair
    // column index of the long block-rows (right operands of the column-window passes): col_index[col_index_row[k] + c / col_index_gran] = first
    // tile of block-row k whose block column is >= c; col_index_row[k] = ~0 for block-rows of at most kIdxMinLen tiles
    bmsp::DevBuf<uint32_t> col_mass;  // prefix sums of this matrix's tiles per granule of col_index_gran block columns (ceil(cols / gran) + 1 entries): where the column-window passes cut
    bmsp::DevBuf<uint32_t> col_index, col_index_row;
    uint32_t col_index_gran = 0;
    int col_index_tried = 0;
    // SpGEMM row-merge paths: what the product of this matrix with the right operand whose uid is rm_partner_uid (B's uid: the key of the
    // three fields below) turned out to need, so that the next product of the pair goes there directly.  The memory holds only what the
    // pair's STRUCTURE needs, two facts kept apart: whether strip mode fits (rm_partner_strip: 0 unknown, 1 a strip pass ran and fitted,
    // 2 a strip pass ran and a block-row of C did not fit) and which path forms the task list otherwise (rm_partner_mode: 0 unknown,
    // 2 task-list mode, 3 the pipeline, 4 column windows).  A call whose arguments, switches or operand values keep strip mode out, or
    // whose left operand is refused for being a row-panel view, runs no strip pass and writes nothing about strip mode.
    uint64_t rm_partner_uid = 0;
    int rm_partner_strip = 0;
    int rm_partner_mode = 0;
    int64_t rm_partner_cw_hash = 0;  // column-window passes: candidate pairs per hashed window that worked for the pair (0: the default)
    // a product made by bmsp_spgemm_symbolic keeps its sorted task list for bmsp_spgemm_numeric (T_7 alone on new operand values)
    bmsp::DevBuf<uint64_t> sp_tasks;
    bmsp::DevBuf<uint32_t> sp_task_begin, sp_c_of_wave;
    uint64_t sp_n_tasks = 0, sp_candidates = 0;
    int64_t sp_a_blocks = 0, sp_b_blocks = 0;
    // a product remembers which operand STRUCTURES it was formed from (struct_hash of A and B; 0 = not stamped: a view, adopted arrays): the
    // fast paths of bmsp_spgemm_numeric trust C only when the stamps match the operands it is given
    uint64_t sp_a_hash = 0, sp_b_hash = 0;
    // made by bmsp_matrix_transpose / bmsp_matrix_convert_layout / bmsp_matrix_scale: the source's uid (0 = neither), the source tile of every tile (the sort's
    // payload; null = the source's tile order) and whether values are permuted inside each tile -- what bmsp_matrix_copy_values replays
    uint64_t tp_src_uid = 0;
    bmsp::DevBuf<uint32_t> tp_map;
    int tp_permute = 0;
    // made by bmsp_matrix_add: the operands' uids (0 = not a sum) and, per tile, its A tile (add_map[c]) and its B tile (add_map[block_num + c];
    // ~0u = none) -- what bmsp_matrix_add_values replays
    uint64_t add_a_uid = 0, add_b_uid = 0;
    bmsp::DevBuf<uint32_t> add_map;
    uint64_t struct_hash = 0;  // this matrix: sum over its blocks of mix(key, bitmap), + dimensions; 0 = not computed (ensure_struct_hash)
    // bmsp_spmv_op: the view per op (0 = N, 1 = T), built on first use; the sum of a layout-0 matrix under op N before its epilogue
    bmsp_spmv_op_view spmv_op_views[2];
    bmsp::DevBuf<void> spmv_op_tmp;
    // bmsp_spmm_op (spmm_op.hip): 8 * k accumulators per scratch slot of the views' split blocks, and the sum of a layout-0 matrix under
    // op N before its epilogue; both grow to the largest call seen
    bmsp::DevBuf<void> spmm_op_scratch, spmm_op_tmp;
    int64_t spmm_op_scratch_elems = 0, spmm_op_tmp_elems = 0;
    // bmsp_spsv: the plan per [op][fill], built by bmsp_spsv_analyse or the first solve
    bmsp_spsv_plan_s spsv_plans[2][2];
    // bmsp_spitsv: the second iterate buffer, num_rows vector elements, made by the first call (one stream per handle at a time: two calls
    // on two streams would share it)
    bmsp::DevBuf<void> spitsv_tmp;
    // bmsp_matrix_ilu0 (ilu0.hip), on the factor F: the value index of every (j, j), num_rows entries; the first row whose diagonal entry
    // is not stored (-1: none; -2: not looked yet); the second iterate buffer, nnz storage elements.  One stream per handle at a time, as
    // for spitsv_tmp.
    bmsp::DevBuf<uint32_t> ilu0_diag;
    int64_t ilu0_missing_row = -2;
    bmsp::DevBuf<void> ilu0_tmp;
    // bmsp_krylov_solve (krylov.hip), on A: one allocation -- scalars and ticket | dot partials | diagonal | vectors | records -- sized
    // for the largest need seen; one stream per handle at a time
    bmsp::DevBuf<void> krylov_ws;
    size_t krylov_ws_bytes = 0;
    // sharded SpMV (comm.hip): this rank's panel view, kept for its cached sweep plan
    bmsp::MatrixPtr shard_view;
    int shard_world = 0, shard_rank = 0;
    std::vector<int64_t> shard_bounds;
};

struct bmsp_matrix_s : bmsp_value_caches, bmsp_structure_caches {
    // identity of this matrix's STRUCTURE: a fresh number at construction and after bmsp_matrix_invalidate(m, 1).  What one matrix remembers
    // about another (the row-merge hint above) is keyed by it -- not by a device pointer, which the pool hands out again
    uint64_t uid = bmsp::next_matrix_uid();
    int num_rows = 0, num_cols = 0;
    int64_t nnz = 0, block_num = 0;
    bmsp_dtype dtype = BMSP_F32;
    int transposed = 0;
    // the four public arrays of the reference container (device memory): raw, because the ABI hands them out and `ownership` decides them
    uint64_t *keys = nullptr;     // block_num
    uint64_t *bmps = nullptr;     // block_num
    uint64_t *offsets = nullptr;  // block_num + 1 (last = nnz)
    void *values = nullptr;       // nnz elements of dtype
    int ownership = 1;            // 1: arrays belong to the pool / this handle, 2: borrowed
    // a row-panel view points into its parent
    int64_t view_block_begin = 0;
    int64_t view_values_end = 0;  // row-panel views: end (in elements) of the panel's values inside the parent's array

    // the four arrays go back to the pool if they are this handle's (ownership 1), and are forgotten either way
    void release_arrays()
    {
        if (ownership == 1) { bmsp::pool_free(keys); bmsp::pool_free(bmps); bmsp::pool_free(offsets); bmsp::pool_free(values); }
        keys = bmps = offsets = nullptr; values = nullptr;
    }
    ~bmsp_matrix_s() { release_arrays(); }
    // what invalidate_matrix does to the handle once the device is idle (no HIP call here: tests/host_handle_check.cpp runs these)
    void reset_value_caches() { static_cast<bmsp_value_caches &>(*this) = bmsp_value_caches(); }
    void reset_structure_caches()
    {
        static_cast<bmsp_structure_caches &>(*this) = bmsp_structure_caches();
        uid = bmsp::next_matrix_uid();  // what other matrices remembered about this one's old structure no longer applies
    }
    // elements addressable from `values`: offsets of a view stay absolute into the parent's value array
    int64_t values_extent() const { return view_values_end ? view_values_end : nnz; }
    int64_t num_block_rows() const { return ((int64_t)num_rows + 7) / 8; }
    int64_t num_block_cols() const { return ((int64_t)num_cols + 7) / 8; }
};

// one RCCL communicator (bmsp_comm_t); `comm` is an ncclComm_t
struct bmsp_comm_s {
    void *comm = nullptr;
    int rank = 0, world = 1, device = 0;
    void *xstream = nullptr;  // the exchange stream of the sharded SpGEMM (a round's broadcasts run on it while the next round multiplies)
    int loopback = 0;  // 1: no RCCL -- every panel is computed by this process on this device, "broadcast" = device copy (comm.hip)
};

namespace bmsp {

// What `m` remembers is about the right operand of uid `partner` from here on: a memory kept for another partner is not this pair's.
inline void rm_hint_key(bmsp_matrix_s *m, uint64_t partner)
{
    if (m->rm_partner_uid == partner) return;
    m->rm_partner_uid = partner; m->rm_partner_strip = 0; m->rm_partner_mode = 0; m->rm_partner_cw_hash = 0;
}
// A row-panel view inherits what its parent learned about a right operand and hands back what it learned itself: views are made per call,
// and without this every panel product would pay for a pass that does not fit (hub block-rows).  What comes back holds for the parent:
// a strip pass that overflowed on a panel overflows on every matrix that holds the panel's block-rows (2 stays), a panel that fitted
// says so until another panel or the parent's own pass says otherwise, and of the list paths the one that corrects itself wins (a pair
// sent to the column windows that does not need them ends in the pipeline and remembers that; the reverse never happens).  A view that
// ran no strip pass -- the rule refuses views where it accepts the parent (mac_rowsparse_operand) -- has written nothing about
// strip mode, so nothing of the kind reaches the parent.
inline void rm_hint_inherit(bmsp_matrix_s *view, const bmsp_matrix_s *parent)
{
    view->rm_partner_uid = parent->rm_partner_uid; view->rm_partner_strip = parent->rm_partner_strip; view->rm_partner_mode = parent->rm_partner_mode;
    view->rm_partner_cw_hash = parent->rm_partner_cw_hash;
}
inline void rm_hint_merge(bmsp_matrix_s *parent, const bmsp_matrix_s *view)
{
    if (!view->rm_partner_uid) return;
    rm_hint_key(parent, view->rm_partner_uid);
    if (view->rm_partner_strip == 2 || (view->rm_partner_strip == 1 && parent->rm_partner_strip == 0)) parent->rm_partner_strip = view->rm_partner_strip;
    if (view->rm_partner_mode > parent->rm_partner_mode) parent->rm_partner_mode = view->rm_partner_mode;
    if (view->rm_partner_cw_hash) parent->rm_partner_cw_hash = view->rm_partner_cw_hash;
}

inline size_t dtype_size(bmsp_dtype t) { return t == BMSP_F16 ? 2 : (t == BMSP_F32 ? 4 : 8); }

// host COO triples produced by the MatrixMarket parser
struct HostCoo {
    int num_rows = 0, num_cols = 0;
    std::vector<int> rows, cols;
    std::vector<double> vals;
};

// MatrixMarket coordinate reader (reference: src/bmSpMatrix.cu:111-161 ; CUSP reader semantics for
// pattern / symmetric, cusp/io/detail/matrix_market.inl:171-196,245-292).
void read_matrix_market(const std::string &path, HostCoo &out);

// builder (reference: src/bmSpMatrix.cu:163-216) from COO triples resident on the device
bmsp_matrix_s *build_from_device_coo(int num_rows, int num_cols, int64_t nnz, const int *d_rows, const int *d_cols,
                                     const double *d_vals, int transposed, bmsp_dtype dtype, hipStream_t st);

void ensure_rowptr(bmsp_matrix_s *m, hipStream_t st);
void ensure_row_stats(bmsp_matrix_s *m, hipStream_t st);
uint64_t ensure_struct_hash(bmsp_matrix_s *m, hipStream_t st);
void ensure_block_meta(bmsp_matrix_s *m, hipStream_t st);
void ensure_sym_recs(bmsp_matrix_s *m, hipStream_t st);
void ensure_col_index(bmsp_matrix_s *m, uint32_t gran, hipStream_t st);
void ensure_col_mass(bmsp_matrix_s *m, uint32_t gran, hipStream_t st);
constexpr uint32_t kIdxMinLen = 16;
int tile_product_selftest(hipStream_t st);
void ensure_dense_tiles(bmsp_matrix_s *m, hipStream_t st);
void ensure_lane_tiles(bmsp_matrix_s *m, hipStream_t st);
void ensure_finite_flag(bmsp_matrix_s *m, hipStream_t st);
bool mac_f32_mfma_usable(hipStream_t st);
int mfma32_selftest(hipStream_t st);
int mfma_f32_selftest(hipStream_t st, bool cancel = false);
int mac_f32_exp_floor(hipStream_t st);
void ensure_csr32(bmsp_matrix_s *m, hipStream_t st);
// Which block-MAC kernel a product takes is decided in ONE place: the pure rule of mac_choice.h, asked through mac_decide (mac_choice.hip),
// which copies the facts out of the handles and fetches the costly ones only when the rule names them.  bmsp_spgemm, bmsp_spgemm_numeric
// and bmsp_matrix_prepare(SPGEMM) ask it and nothing else; the launchers below launch what they are told and keep only their tuning.
struct MacTasks {  // a product's sorted task list
    const uint64_t *sorted;
    uint64_t n, candidates;
    const uint32_t *begin, *c_of_wave;
};
MacSwitches mac_read_switches();
MacOperand mac_operand_facts(const bmsp_matrix_s *m);
MacChoice mac_decide(bmsp_matrix_s *A, bmsp_matrix_s *B, bmsp_matrix_s *C, const MacTasks *tasks, int tc_version, const MacSwitches &sw, hipStream_t st);
void launch_mac_mfma32(const uint64_t *tasks, uint64_t n_tasks, const uint32_t *task_begin, const uint32_t *c_of_wave, bmsp_matrix_s *A,
                       bmsp_matrix_s *B, bmsp_matrix_s *C, bool b_dense, bool direct, hipStream_t st);
void launch_mac_f32_mfma(const uint64_t *tasks, uint64_t n_tasks, const uint32_t *task_begin, const uint32_t *c_of_wave, bmsp_matrix_s *A,
                         bmsp_matrix_s *B, bmsp_matrix_s *C, hipStream_t st);
void launch_mac_strip(bmsp_matrix_s *A, bmsp_matrix_s *B, bmsp_matrix_s *C, bool prof, hipStream_t st);  // prof: the timing build (BMSP_STRIP_PROF)
void launch_mac_rowsparse(bmsp_matrix_s *A, bmsp_matrix_s *B, bmsp_matrix_s *C, hipStream_t st);
bool rowmerge_symbolic(bmsp_matrix_s *A, bmsp_matrix_s *B, bmsp_matrix_s *C, const uint64_t *first_pos, uint64_t total, uint32_t row_cap,
                       uint64_t *surviving, uint64_t *candidates, hipStream_t st);
bool rowmerge_tasklist(bmsp_matrix_s *A, bmsp_matrix_s *B, bmsp_matrix_s *C, const uint64_t *first_pos, uint64_t total, DevBuf<uint64_t> &tasks,
                       DevBuf<uint32_t> &task_begin, DevBuf<uint32_t> &c_of_wave, uint64_t *n_tasks, hipStream_t st);
bool rowmerge_windowed(bmsp_matrix_s *A, bmsp_matrix_s *B, bmsp_matrix_s *C, const uint64_t *first_pos, uint64_t total, DevBuf<uint64_t> &tasks,
                       DevBuf<uint32_t> &task_begin, DevBuf<uint32_t> &c_of_wave, uint64_t *n_tasks, hipStream_t st);
void matrix_to_coo_host(bmsp_matrix_s *m, int *rows, int *cols, double *vals, hipStream_t st);
void matrix_to_coo_device(bmsp_matrix_s *m, uint64_t *d_rc, double *d_vals, hipStream_t st);  // every stored value as ((row << 32) | col, value), sorted by (row, col)
void matrix_to_coo_device_split(bmsp_matrix_s *m, int *d_rows, int *d_cols, double *d_vals, hipStream_t st);
void matrix_to_csr_device(bmsp_matrix_s *m, int *d_row_offsets, int *d_cols, double *d_vals, hipStream_t st);
void matrix_compare_device(bmsp_matrix_s *m, int64_t nnz, const int *d_rows, const int *d_cols, const double *d_vals, double *mean_rel_err,
                           int64_t *missing, hipStream_t st);
bmsp_matrix_s *build_from_device_csr(int num_rows, int num_cols, int64_t nnz, const int *d_row_offsets, const int *d_cols, const double *d_vals,
                                     int transposed, bmsp_dtype dtype, hipStream_t st);
void free_matrix(bmsp_matrix_s *m);
inline MatrixPtr own_matrix(bmsp_matrix_s *m) { return MatrixPtr(m); }
inline MatrixPtr make_matrix() { return own_matrix(new bmsp_matrix_s()); }
// pooled arrays of a matrix of nb tiles / nnz elements of m->dtype, never empty allocations (at least one element each).
// alloc_tile_arrays makes whichever of keys, bmps (nb) and offsets (nb + 1) the matrix does not hold yet; the values are a call of
// their own for the builders that learn nnz after they have filled the tile arrays.
void alloc_tile_arrays(bmsp_matrix_s *m, uint64_t nb);
void alloc_values(bmsp_matrix_s *m, uint64_t nnz);
// argument checks shared by the operations: a tile-layout flag (`name` = the argument's name) is 0 or 1; `op` does not take a row-panel view
void check_layout_flag(int value, const char *name);
void refuse_view(const bmsp_matrix_s *m, const char *op);
// before m's values are rewritten in place: drops what invalidate_matrix(m, 0) drops
void drop_value_caches(bmsp_matrix_s *m);
// transpose.hip: the tiles of a matrix in (block-column, block-row) order -- the sorted swapped keys and, as payload, the source tile of
// each.  The four buffers live as long as the struct (the pool is not stream-aware); take_* hands the two results to a matrix (the keys raw: a public array).
struct TileSort {
    DevBuf<uint64_t> k0, k1;
    DevBuf<uint32_t> p0, p1;
    const uint64_t *keys = nullptr;
    const uint32_t *map = nullptr;
    uint64_t *take_keys() { return keys == k0.p ? k0.take() : k1.take(); }
    DevBuf<uint32_t> take_map() { return std::move(map == p0.p ? p0 : p1); }
};
void sort_tiles_by_block_column(const bmsp_matrix_s *A, TileSort &ts, hipStream_t st);
// transpose.hip: out = A^T (swap) or A (!swap) with tiles in layout out_transposed; re-gather such an out's values from A
bmsp_matrix_s *transpose_matrix(bmsp_matrix_s *A, int out_transposed, bool swap, hipStream_t st);
void copy_values_from(bmsp_matrix_s *A, bmsp_matrix_s *out, hipStream_t st);
// transpose.hip, for the makers that re-order whole tiles (reorder.hip): the value move through out's tile map and permutation flag, and
// the tail of such a maker -- arrays, bitmaps and offsets in one scan, values, block-row pointer; synchronises `st`
void move_values(const bmsp_matrix_s *A, bmsp_matrix_s *out, hipStream_t st);
void finish_moved_tiles(bmsp_matrix_s *A, bmsp_matrix_s *m, hipStream_t st);
// reorder.hip: the greedy colouring of the block-row graph by hashed priorities and the ordering by colour class; out = P * A * Q^T at
// tile granularity (tiles in layout out_transposed; bmsp_matrix_copy_values replays it); the block permutation of a vector
void color_check_matrix(const bmsp_matrix_s *A);
void color_blocks(bmsp_matrix_s *A, uint64_t seed, uint32_t *d_colors, uint32_t *d_perm, hipStream_t st, bmsp_color_info *info);
void permute_check_matrix(const bmsp_matrix_s *A);
bmsp_matrix_s *permute_blocks(bmsp_matrix_s *A, const uint32_t *d_row_perm, const uint32_t *d_col_perm, int out_transposed, hipStream_t st);
void vec_permute_check_args(int64_t n, int vec_f64, const void *d_perm, int inverse, const void *d_x, const void *d_y);
void vec_permute_blocks(int64_t n, int vec_f64, const uint32_t *d_perm, int inverse, const void *d_x, void *d_y, hipStream_t st);
// aggregate.hip: the MIS(2) aggregates of the scalar graph of a square S by hashed priorities (builds S's block-row pointer and op-T view
// if they are missing; synchronises `st`); the num_rows x num_aggregates matrix with one entry (i, d_agg[i]) per row
void aggregate_check_matrix(const bmsp_matrix_s *S);
void aggregate(bmsp_matrix_s *S, uint64_t seed, uint32_t *d_agg, int64_t *num_aggregates, hipStream_t st, bmsp_aggregate_info *info);
void from_aggregates_check_args(int num_rows, int num_aggregates, const uint32_t *d_agg, bmsp_dtype dtype, int transposed);
bmsp_matrix_s *matrix_from_aggregates(int num_rows, int num_aggregates, const uint32_t *d_agg, const void *d_weights, bmsp_dtype dtype,
                                      int transposed, hipStream_t st);
// add.hip: C = alpha*A + beta*B with tiles in layout out_transposed; re-compute such a C's values from the same two structures
bmsp_matrix_s *add_matrices(double alpha, bmsp_matrix_s *A, double beta, bmsp_matrix_s *B, int out_transposed, hipStream_t st);
void add_values(double alpha, bmsp_matrix_s *A, double beta, bmsp_matrix_s *B, bmsp_matrix_s *C, hipStream_t st);
// prune.hip: *out = A without the entries the rule drops (tiles in layout out_transposed) and / or the counts; the row maxima of |v|
void prune_check_args(int rule, double tol, int flags, int out_transposed);
void prune_matrix(bmsp_matrix_s *A, int rule, double tol, int flags, int out_transposed, hipStream_t st, bmsp_matrix_s **out,
                  bmsp_prune_stats *stats);
void row_absmax(bmsp_matrix_s *A, void *d_rowmax, hipStream_t st);
// select.hip: *out = A's entries in the band lo <= col - row <= hi / at the coordinates M stores (or, under BMSP_SELECT_COMPLEMENT, the
// others), tiles in layout out_transposed, and / or the counts
void select_check_args(int flags, int out_transposed, const void *out, const void *stats);
void select_band(bmsp_matrix_s *A, int64_t lo, int64_t hi, int flags, int out_transposed, hipStream_t st, bmsp_matrix_s **out,
                 bmsp_select_stats *stats);
void select_mask(bmsp_matrix_s *A, bmsp_matrix_s *M, int flags, int out_transposed, hipStream_t st, bmsp_matrix_s **out,
                 bmsp_select_stats *stats);
// diag.hip: the diagonal as a vector, a diagonal matrix from a vector, out = diag(l) * A * diag(r) as a new matrix (tiles in layout
// out_transposed) or into A itself / a matrix made from A by scale_matrix or a layout conversion
void scale_check_args(const void *d_left, const void *d_right, int flags, int out_transposed);
void from_diagonal_check_args(int num_rows, int num_cols, const void *d_diag, bmsp_dtype dtype, int transposed);
void matrix_diagonal(bmsp_matrix_s *A, void *d_diag, hipStream_t st);
bmsp_matrix_s *matrix_from_diagonal(int num_rows, int num_cols, const void *d_diag, bmsp_dtype dtype, int transposed, hipStream_t st);
bmsp_matrix_s *scale_matrix(bmsp_matrix_s *A, const void *d_left, const void *d_right, int flags, int out_transposed, hipStream_t st);
void scale_values_into(bmsp_matrix_s *A, const void *d_left, const void *d_right, int flags, bmsp_matrix_s *out, hipStream_t st);
// sddmm.hip: the sampled dense-dense product alpha * (X . Y^T) on S's pattern (+ beta * S, or * S) as a new matrix (tiles in layout
// out_transposed) or into S itself / a matrix made from S by sddmm_matrix, scale_matrix or a layout conversion; what that call launches
void sddmm_check_args(int k, int64_t ldx, int64_t ldy, double beta, int flags, int out_transposed);
bmsp_matrix_s *sddmm_matrix(bmsp_matrix_s *S, const void *X, int64_t ldx, const void *Y, int64_t ldy, int k, double alpha, double beta,
                            int flags, int out_transposed, hipStream_t st);
void sddmm_values_into(bmsp_matrix_s *S, const void *X, int64_t ldx, const void *Y, int64_t ldy, int k, double alpha, double beta, int flags,
                       bmsp_matrix_s *out, hipStream_t st);
void sddmm_launch_info(bmsp_matrix_s *S, int k, int64_t ldx, int64_t ldy, int out_transposed, bmsp_sddmm_info *info);
// spgemm_masked.hip: the masked sparse product alpha * (A * B) on M's pattern (+ beta * M, or * M) as a new matrix (tiles in layout
// out_transposed) or into M itself / a matrix made from M by spgemm_masked_matrix, sddmm_matrix, scale_matrix or a layout conversion; what
// that call launches.  Builds A's block-row pointer and B's op-T view if they are missing (the latter synchronises `st`).
void spgemm_masked_check_args(double beta, int flags, int out_transposed);
void spgemm_masked_check_matrices(const bmsp_matrix_s *A, const bmsp_matrix_s *B, const bmsp_matrix_s *M, const bmsp_matrix_s *out);
bmsp_matrix_s *spgemm_masked_matrix(bmsp_matrix_s *A, bmsp_matrix_s *B, bmsp_matrix_s *M, double alpha, double beta, int flags,
                                    int out_transposed, hipStream_t st);
void spgemm_masked_values_into(bmsp_matrix_s *A, bmsp_matrix_s *B, bmsp_matrix_s *M, double alpha, double beta, int flags, bmsp_matrix_s *out,
                               hipStream_t st);
void spgemm_masked_launch_info(bmsp_matrix_s *A, bmsp_matrix_s *B, bmsp_matrix_s *M, int out_transposed, bmsp_spgemm_masked_info *info);
// spsv.hip: the triangular solve op(tri(A)) * x = alpha * b for either tile layout; its plan (levels, launch schedule) as a report; the
// host part of the planner.  Both build the plan of (A, op, fill) if it is missing, which synchronises `st`.
void spsv_check_args(int op, int fill, int diag);
void spsv_check_matrix(const bmsp_matrix_s *A);
void spsv(bmsp_matrix_s *A, int op, int fill, int diag, double alpha, const void *b, void *x, hipStream_t st);
void spsv_analyse(bmsp_matrix_s *A, int op, int fill, int diag, hipStream_t st, bmsp_spsv_info *info);
void spsv_plan(const uint32_t *ptr, const uint32_t *other, int64_t blocks, int lower, int64_t chain, uint32_t *level_of, uint32_t *order,
               uint32_t *level_ptr, uint32_t *segments, int64_t *n_levels, int64_t *n_segments);
// spsm.hip: the triangular solve for k right-hand sides, op(tri(A)) * X = alpha * B, on the plan of spsv.hip (built if it is missing,
// which synchronises `st`); what that call launches
void spsm_check_args(int op, int fill, int diag, int k, int64_t ldb, int64_t ldx);
void spsm_check_in_place(const void *B, int64_t ldb, const void *X, int64_t ldx);
void spsm(bmsp_matrix_s *A, int op, int fill, int diag, double alpha, const void *B, int64_t ldb, void *X, int64_t ldx, int k, hipStream_t st);
void spsm_launch_info(bmsp_matrix_s *A, int op, int fill, int diag, int k, int64_t ldb, int64_t ldx, hipStream_t st, bmsp_spsm_info *info);
// spitsv.hip: block-Jacobi sweeps towards the solution of op(tri(A)) * x = alpha * b on the plan of spsv.hip (built if it is missing, which
// synchronises `st`), until the stop rule holds or max_iter sweeps have run
void spitsv_check_args(int op, int fill, int diag, int64_t max_iter, double tol, int flags, const double *delta_history);
void spitsv_check_vectors(const void *b, const void *x);
void spitsv(bmsp_matrix_s *A, int op, int fill, int diag, double alpha, const void *b, void *x, int64_t max_iter, double tol, int flags,
            double *delta_history, bmsp_spitsv_info *info, hipStream_t st);
// ilu0.hip: the incomplete factorisation ILU(0) of A by fixed-point sweeps, as a new matrix of A's structure (tiles in layout
// out_transposed) or into a matrix made from A by ilu0_matrix or a layout-keeping maker.  Both build F's op-T view and diagonal index if
// they are missing, which synchronises `st`.
void ilu0_check_args(int64_t max_iter, double tol, const double *delta_history);
void ilu0_check_flags(int flags);
void ilu0_check_matrices(const bmsp_matrix_s *A, const bmsp_matrix_s *F);
bmsp_matrix_s *ilu0_matrix(bmsp_matrix_s *A, int64_t max_iter, double tol, int out_transposed, hipStream_t st, double *delta_history,
                           bmsp_ilu0_info *info);
void ilu0_values_into(bmsp_matrix_s *A, bmsp_matrix_s *F, int64_t max_iter, double tol, int flags, hipStream_t st, double *delta_history,
                      bmsp_ilu0_info *info);
// krylov.hip: the deterministic dot product and the scaled sum of device vectors; CG and BiCGStab for op(A) x = b with the iteration
// enqueued on `st` (scalars, status and records device-resident)
void vec_check_args(int64_t n, int vec_f64);
void vec_dot(int64_t n, int vec_f64, const void *x, const void *y, double *result, hipStream_t st);
void vec_axpby(int64_t n, int vec_f64, double a, const void *x, double b, void *y, hipStream_t st);
void krylov_check_args(int op, int method, const bmsp_precond *pc, int64_t max_iter, double tol, int flags, const double *relres_history);
void krylov_check_operands(const bmsp_matrix_s *A, const bmsp_precond *pc);
// The preconditioner of a solve: a public bmsp_precond (null: none) or, where `hook` is set, a handle's: out = M^-1 in enqueued on the
// stream by hook(handle, ...), printed as `name` in info->method, op N only.  `stopped` is the solve's status word on the device, which
// the hook's kernels read first.
struct SolvePc {
    const bmsp_precond *pc = nullptr;
    void (*hook)(void *handle, const void *in, void *out, const int *stopped, hipStream_t st) = nullptr;
    void *handle = nullptr;
    const char *name = nullptr;
};
void krylov_solve(bmsp_matrix_s *A, int op, int method, const SolvePc &pc, const void *b, void *x, int64_t max_iter, double tol, int flags,
                  double *relres_history, bmsp_krylov_info *info, hipStream_t st);
// gmres.hip: restarted GMRES for op(A) x = b, enqueued on `st` like the two solvers above; restart 0 means 30
void gmres_check_args(int op, int restart, const bmsp_precond *pc, int64_t max_iter, double tol, int flags, const double *relres_history);
void gmres_solve(bmsp_matrix_s *A, int op, const SolvePc &pc, int restart, const void *b, void *x, int64_t max_iter, double tol, int flags,
                 double *relres_history, bmsp_krylov_info *info, hipStream_t st);
// multigrid.hip: the V-cycle of a caller-supplied hierarchy (the operators borrowed; diagonals, the coarse inverse and the work vectors
// owned by the handle), enqueued on `st`, and the cycle as the preconditioner of a solve.  mg_create synchronises `st`.
void mg_check_args(int levels, double omega, int pre, int post, const void *d_coarse_inv);
void mg_check_operands(int levels, bmsp_matrix_s *const *A, bmsp_matrix_s *const *P, bmsp_matrix_s *const *R, const void *d_coarse_inv,
                       int64_t ld_inv);
bmsp_mg_s *mg_create(int levels, bmsp_matrix_s *const *A, bmsp_matrix_s *const *P, bmsp_matrix_s *const *R, const void *d_coarse_inv,
                     int64_t ld_inv, double omega, int pre, int post, hipStream_t st);
void mg_free(bmsp_mg_s *mg);
void mg_info(bmsp_mg_s *mg, bmsp_mg_info_t *info);
void mg_vcycle(bmsp_mg_s *mg, const void *r, void *z, const int *stopped, hipStream_t st);
// the cycle as the preconditioner of a solve of A[0] x = b (*A: A[0]); builds the restriction views a first cycle would
SolvePc mg_solve_pc(bmsp_mg_s *mg, hipStream_t st, bmsp_matrix_s **A);
// fsai.hip: the factorised sparse approximate inverse of op(A) on S's lower-triangular pattern as a new matrix (tiles in layout
// out_transposed) or into a matrix G with a legal pattern (both synchronise `st`), and the preconditioner handle z = G2^T (G1 r) by two
// bmsp_spmv_op, with CG / BiCGStab / GMRES for A x = b on top.  fsai_create and fsai_update synchronise `st`.
void fsai_check_args(int op, int scale, int out_transposed);
void fsai_check_matrices(const bmsp_matrix_s *A, const bmsp_matrix_s *P, const char *name);
bmsp_matrix_s *fsai_matrix(bmsp_matrix_s *A, int op, bmsp_matrix_s *S, int scale, int out_transposed, void *d_pivot, hipStream_t st,
                           bmsp_fsai_info *info);
void fsai_values_into(bmsp_matrix_s *A, int op, bmsp_matrix_s *G, int scale, void *d_pivot, hipStream_t st, bmsp_fsai_info *info);
void fsai_create_check_args(int kind, int flags);
bmsp_fsai_s *fsai_create(bmsp_matrix_s *A, bmsp_matrix_s *S, int kind, int flags, hipStream_t st);
void fsai_update(bmsp_fsai_s *f, hipStream_t st);
void fsai_free(bmsp_fsai_s *f);
void fsai_get_info(bmsp_fsai_s *f, bmsp_fsai_handle_info *info);
void fsai_factors(bmsp_fsai_s *f, bmsp_matrix_s **G1, bmsp_matrix_s **G2);
void fsai_apply(bmsp_fsai_s *f, const void *r, void *z, hipStream_t st);
// the handle as the preconditioner of a solve of A x = b (*A: its A); rebuilds the views of the factors if they were dropped
SolvePc fsai_solve_pc(bmsp_fsai_s *f, hipStream_t st, bmsp_matrix_s **A);
// eager construction of the cached derived structures (bmsp_matrix_prepare)
void prepare_spmv(bmsp_matrix_s *m, hipStream_t st);
void prepare_spgemm_operand(bmsp_matrix_s *m, hipStream_t st);

void spmv(bmsp_matrix_s *A, const void *v, void *u, int variant, hipStream_t st, int64_t row_lo = 0, int64_t row_hi = -1);
void spmv_launch_info(bmsp_matrix_s *A, int variant, hipStream_t st, char *kernel, size_t kernel_cap, int64_t *compulsory, int64_t *format_bytes);
int spmv_chunk_layout(bmsp_matrix_s *A, hipStream_t st);
// spmv_op.hip: u = alpha * op(A) * v + beta * u for either tile layout; what that call launches; the host part of its item planner
void spmv_op_check_op(int op);
void spmv_op(bmsp_matrix_s *A, int op, double alpha, const void *v, double beta, void *u, hipStream_t st);
void spmv_op_launch_info(bmsp_matrix_s *A, int op, hipStream_t st, bmsp_spmv_op_info *info);
void spmv_op_plan_items(const uint32_t *ptr, int64_t blocks, int64_t split, uint32_t *items, uint32_t *folds, int64_t *n_items,
                        int64_t *split_blocks, int64_t *slots);
// what bmsp_spmm_op shares with bmsp_spmv_op: the argument checks (`what` names the call in the messages), the lengths of op(A)'s input and
// output, the element size of the vectors that go with A, the cached view of (A, op) -- built if it is missing, which synchronises `st`
// -- and the epilogue
void spmv_op_check_matrix(const bmsp_matrix_s *A, const char *what);
int64_t spmv_op_out_blocks(const bmsp_matrix_s *A, int op);
int64_t spmv_op_out_length(const bmsp_matrix_s *A, int op);
int64_t spmv_op_in_length(const bmsp_matrix_s *A, int op);
size_t spmv_op_vector_size(const bmsp_matrix_s *A);
bmsp_spmv_op_view &spmv_op_ensure_view(bmsp_matrix_s *A, int op, hipStream_t st);
#ifdef __HIPCC__
// u_j = fl(alpha * t) when beta == 0 (u is not read), else fl(fl(alpha * t) + fl(beta * u_j)): never contracted (add.hip's scaled_sum)
template <typename R>
__device__ __forceinline__ R spmv_op_epilogue(R alpha, R t, R beta, const R *u, int64_t j)
{
#pragma clang fp contract(off)
    const R x = alpha * t;
    if (beta == R(0)) return x;
    const R y = beta * u[j];
    return x + y;
}
#endif
// spmm_op.hip: Y = alpha * op(A) * X + beta * Y for k vectors and either tile layout; what that call launches
void spmm_op_check_args(int op, int k, int64_t ldx, int64_t ldy);
void spmm_op(bmsp_matrix_s *A, int op, double alpha, const void *X, int64_t ldx, double beta, void *Y, int64_t ldy, int k, hipStream_t st);
void spmm_op_launch_info(bmsp_matrix_s *A, int op, int k, int64_t ldx, int64_t ldy, hipStream_t st, bmsp_spmm_op_info *info);
void spmm(bmsp_matrix_s *A, const void *X, int64_t ldx, void *Y, int64_t ldy, int k, hipStream_t st);
void spmm_launch_info(bmsp_matrix_s *A, int k, int64_t ldx, int64_t ldy, hipStream_t st, char *kernel, size_t kernel_cap);
void spgemm(bmsp_matrix_s *A, bmsp_matrix_s *B, bmsp_matrix_s **C, int mode, int tc_version, int verbose, hipStream_t st,
            bmsp_spgemm_stats *stats, bool structure_only = false);
void spgemm_numeric(bmsp_matrix_s *A, bmsp_matrix_s *B, bmsp_matrix_s *C, int tc_version, hipStream_t st, bmsp_spgemm_stats *stats);
template <typename T>
struct PingPong;
// stable sort of (key, task) pairs inside the runs of equal (key >> jbits): the SpGEMM's segmented path
// false = some block-row has more tasks than the LDS paths hold; nothing was modified and the caller sorts globally
bool segsort_tasks_by_column(PingPong<uint64_t> &keys, PingPong<uint64_t> &vals, uint64_t n, int jbits, hipStream_t st, uint64_t max_seg_bound = 0,
                             uint64_t seg_count_bound = 0, int *long_mode = nullptr);  // *long_mode: BMSP_SORT_LONG_* (0: no long segment)
void segsort_check_violation();
void segsort_u64(uint64_t *d_keys, void *d_vals, int val_bytes, int64_t n, const int *d_segs, int64_t num_segs,
                 hipStream_t st);

// multi-GPU (comm.hip)
void comm_unique_id(void *id128);
bmsp_comm_s *comm_init(const void *id128, int world, int rank);
bmsp_comm_s *comm_init_from_env();
bmsp_comm_s *comm_init_loopback(int world);
void shard_layout(int parts, const int64_t *block_nums, const int64_t *nnzs, int64_t *block_start, int64_t *value_start);
void shard_row_slices(int num_rows, int parts, const int64_t *bounds, int64_t *row_start, int64_t *row_count);
void invalidate_matrix(bmsp_matrix_s *m, int structure_changed);
void comm_free(bmsp_comm_s *c);
void spgemm_sharded(bmsp_comm_s *c, bmsp_matrix_s *A, bmsp_matrix_s *B, bmsp_matrix_s **C, int mode, int tc_version, int verbose, hipStream_t st,
                    bmsp_spgemm_stats *stats, bmsp_shard_stats *sh, int gather = 1, int rounds = 0);
void spmv_sharded(bmsp_comm_s *c, bmsp_matrix_s *A, const void *x, void *y, int variant, hipStream_t st, bmsp_shard_stats *sh);

}  // namespace bmsp
#endif
