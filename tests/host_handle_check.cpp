// host_handle_check.cpp -- the lifetime of what a matrix handle caches (csrc/matrix.h), executed on the host with a counting pool.
// A handle is filled: every owner of the two cache groups holds an allocation of its own, every flag and counter a value that is not its
// default, both op views and all four spsv plans are built, and shard_view is a handle that holds caches itself.  Then, by the number of
// live allocations and by value: what bmsp_matrix_invalidate(m, 1) and (m, 0) do to it (invalidate_matrix is the device synchronisation
// and these two resets), re-assigning an owner, deleting the handle with either ownership, and moving a buffer out.  No HIP is linked:
// pool_alloc, pool_free and next_matrix_uid are the stand-ins below, and a pool_free of anything that is not live (a second release, a
// pointer the pool never made) is an error.  Prints "OK owners=<allocations the caches of one filled handle hold>" and exits 0, or one
// line per mismatch.  tests/test_structure_invalidate.py checks that the lists below name every member of the groups.
#include "../bmsparse-spgemm-spmv_amd/csrc/matrix.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <set>

static int g_bad = 0;
#define CHECK(cond) \
    do { \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); g_bad++; } \
    } while (0)

static std::set<void *> g_live;
static long g_frees = 0;
static uint64_t g_uid = 0;
namespace bmsp {
void *pool_alloc(size_t bytes)
{
    void *p = malloc(bytes ? bytes : 1);
    g_live.insert(p);
    return p;
}
void pool_free(void *p)
{
    if (!p) return;
    if (!g_live.erase(p)) { printf("pool_free of %p, which is not live\n", p); g_bad++; return; }
    g_frees++;
    free(p);
}
uint64_t next_matrix_uid() { return ++g_uid; }
}  // namespace bmsp
using namespace bmsp;

// every member of the two groups, once: X(name, default) for flags and counters, X(name) for owners of one allocation
#define VALUE_SCALARS(X) X(values_finite, -1) X(f32_exp_min, 255) X(f32_exp_max, 0)
#define VALUE_OWNERS(X) X(dense_tiles) X(lane_tiles) X(csr_rowptr) X(csr_ent)
#define STRUCTURE_SCALARS(X) \
    X(rowptr_rows, 0) X(max_row_blocks, -1) X(spmv_num_chunks, 0) X(spmv_plan_long, 0) X(spmv_full_tiles, 0) X(spmv_plan_off_cnt, 0) \
    X(spmv_plan_off_carry, 0) X(spmv_pos_base, 0) X(spmv_pos_count, 0) X(spmv_pos_tried, 0) X(spmv_cw_chunks, 0) X(spmv_cw_split, 0) \
    X(spmv_cw_off_rec, 0) X(spmv_cw_off_cnt, 0) X(spmv_cw_off_carry, 0) X(spmv_cw_colbits, 0) X(spmv_cw_tried, 0) X(spmv_cw_layout, 0) \
    X(col_index_gran, 0) X(col_index_tried, 0) X(rm_partner_uid, 0) X(rm_partner_strip, 0) X(rm_partner_mode, 0) X(rm_partner_cw_hash, 0) \
    X(sp_n_tasks, 0) X(sp_candidates, 0) X(sp_a_blocks, 0) X(sp_b_blocks, 0) X(sp_a_hash, 0) X(sp_b_hash, 0) X(tp_src_uid, 0) X(tp_permute, 0) \
    X(add_a_uid, 0) X(add_b_uid, 0) X(struct_hash, 0) X(spmm_op_scratch_elems, 0) X(spmm_op_tmp_elems, 0) X(ilu0_missing_row, -2) \
    X(krylov_ws_bytes, 0) X(shard_world, 0) X(shard_rank, 0)
#define STRUCTURE_OWNERS(X) \
    X(rowptr) X(spmv_chunks) X(spmv_pos) X(spmv_cw) X(block_meta) X(sym_recs) X(col_mass) X(col_index) X(col_index_row) X(sp_tasks) \
    X(sp_task_begin) X(sp_c_of_wave) X(tp_map) X(add_map) X(spmv_op_tmp) X(spmm_op_scratch) X(spmm_op_tmp) X(spitsv_tmp) X(ilu0_diag) \
    X(ilu0_tmp) X(krylov_ws)
// (the members that are neither: spmv_tinfo and spmv_eoff, aliases into spmv_pos; spmv_op_views, spsv_plans, shard_view and
// shard_bounds, handled by name below)

#define FILL_SCALAR(name, dflt) m.name = (decltype(m.name))77;
#define FILL_OWNER(name) m.name.alloc(3);
#define IS_DEFAULT_SCALAR(name, dflt) CHECK(m.name == (decltype(m.name))(dflt));
#define IS_NULL(name) CHECK(!m.name);
#define IS_HELD(name) CHECK(m.name && g_live.count((void *)m.name));
#define IS_FILLED_SCALAR(name, dflt) CHECK(m.name == (decltype(m.name))77);

static void fill_caches(bmsp_matrix_s &m)
{
    VALUE_SCALARS(FILL_SCALAR) VALUE_OWNERS(FILL_OWNER) STRUCTURE_SCALARS(FILL_SCALAR) STRUCTURE_OWNERS(FILL_OWNER)
    m.spmv_tinfo = (uint32_t *)m.spmv_pos.p;
    m.spmv_eoff = m.spmv_pos.p + 1;
    for (bmsp_spmv_op_view &w : m.spmv_op_views) {
        w.mem.alloc(3);
        w.off_ptr = w.off_items = w.off_folds = w.off_scratch = w.bytes = 77;
        w.blocks = w.items = w.split_blocks = w.slots = 77;
    }
    for (auto &per_op : m.spsv_plans)
        for (bmsp_spsv_plan_s &pl : per_op) {
            pl.mem.alloc(3);
            pl.off_level_ptr = pl.bytes = 77;
            pl.blocks = pl.levels = pl.max_level_width = pl.chain_launches = pl.chained_levels = pl.chain = pl.missing_diag_row = 77;
            pl.level_ptr.assign(5, 7u); pl.segments.assign(3, 7u);
        }
    m.shard_bounds.assign(4, 77);
}

// a handle of ownership 1 with every cache filled; shard_view is a view into its arrays (ownership 2) with every cache filled but a view
static bmsp_matrix_s *full_handle(size_t *owners)
{
    auto m = make_matrix();
    m->keys = (uint64_t *)pool_alloc(8); m->bmps = (uint64_t *)pool_alloc(8); m->offsets = (uint64_t *)pool_alloc(16); m->values = pool_alloc(4);
    const size_t before = g_live.size();
    fill_caches(*m);
    *owners = g_live.size() - before;
    m->shard_view = make_matrix();
    bmsp_matrix_s &v = *m->shard_view;
    v.keys = m->keys; v.bmps = m->bmps; v.offsets = m->offsets; v.values = m->values; v.ownership = 2;
    fill_caches(v);
    return m.release();
}

static void check_value_group_default(const bmsp_matrix_s &m) { VALUE_SCALARS(IS_DEFAULT_SCALAR) VALUE_OWNERS(IS_NULL) CHECK(!m.holds_memory()); }

static void check_structure_group_default(const bmsp_matrix_s &m)
{
    STRUCTURE_SCALARS(IS_DEFAULT_SCALAR) STRUCTURE_OWNERS(IS_NULL)
    CHECK(!m.spmv_tinfo); CHECK(!m.spmv_eoff);
    for (const bmsp_spmv_op_view &w : m.spmv_op_views)
        CHECK(!w.mem && !w.off_ptr && !w.off_items && !w.off_folds && !w.off_scratch && !w.bytes && !w.blocks && !w.items && !w.split_blocks && !w.slots);
    for (const auto &per_op : m.spsv_plans)
        for (const bmsp_spsv_plan_s &pl : per_op)
            CHECK(!pl.mem && !pl.off_level_ptr && !pl.bytes && !pl.blocks && !pl.levels && !pl.max_level_width && !pl.chain_launches && !pl.chained_levels &&
                  !pl.chain && pl.missing_diag_row == -1 && pl.level_ptr.empty() && pl.segments.empty());
    CHECK(!m.shard_view); CHECK(m.shard_bounds.empty());
}

static void check_structure_group_filled(const bmsp_matrix_s &m, bool has_view)
{
    STRUCTURE_SCALARS(IS_FILLED_SCALAR) STRUCTURE_OWNERS(IS_HELD)
    CHECK((void *)m.spmv_tinfo == (void *)m.spmv_pos.p && m.spmv_eoff == m.spmv_pos.p + 1);
    for (const bmsp_spmv_op_view &w : m.spmv_op_views) CHECK(w.mem && g_live.count(w.mem.p) && w.bytes == 77 && w.slots == 77);
    for (const auto &per_op : m.spsv_plans)
        for (const bmsp_spsv_plan_s &pl : per_op) CHECK(pl.mem && g_live.count(pl.mem.p) && pl.missing_diag_row == 77 && pl.level_ptr.size() == 5 && pl.segments.size() == 3);
    CHECK((m.shard_view != nullptr) == has_view); CHECK(m.shard_bounds.size() == 4);
}

// the bytes of a handle's structure group (the storage was zeroed before the handle was made in it, and nothing writes padding)
static const unsigned char *structure_bytes(const bmsp_matrix_s *m) { return (const unsigned char *)static_cast<const bmsp_structure_caches *>(m); }

static void public_arrays_live(const bmsp_matrix_s &m, const void *const arr[4])
{
    CHECK(m.keys == arr[0] && m.bmps == arr[1] && m.offsets == arr[2] && m.values == arr[3]);
    for (int i = 0; i < 4; i++) CHECK(g_live.count((void *)arr[i]));
}

int main()
{
    size_t owners = 0;
    {  // bmsp_matrix_invalidate(m, 1): everything but the four arrays released once, every member its default, a new uid
        bmsp_matrix_s *m = full_handle(&owners);
        CHECK(owners == 4 + 21 + 2 + 4);
        CHECK(g_live.size() == 4 + 2 * owners);
        check_structure_group_filled(*m, true);
        check_structure_group_filled(*m->shard_view, false);
        const void *arr[4] = {m->keys, m->bmps, m->offsets, m->values};
        const uint64_t uid = m->uid;
        const long frees = g_frees;
        m->reset_value_caches();
        m->reset_structure_caches();
        CHECK(g_frees - frees == (long)(2 * owners));
        CHECK(g_live.size() == 4);
        public_arrays_live(*m, arr);
        CHECK(m->uid != uid && m->ownership == 1);
        check_value_group_default(*m);
        check_structure_group_default(*m);
        // ... and as a whole: the group of the reset handle against the group of a handle nobody touched, byte for byte
        alignas(bmsp_matrix_s) static unsigned char s0[sizeof(bmsp_matrix_s)], s1[sizeof(bmsp_matrix_s)];
        memset(s0, 0, sizeof s0); memset(s1, 0, sizeof s1);
        bmsp_matrix_s *a = new (s0) bmsp_matrix_s(), *b = new (s1) bmsp_matrix_s();
        fill_caches(*a);
        CHECK(memcmp(structure_bytes(a), structure_bytes(b), sizeof(bmsp_structure_caches)) != 0);
        a->reset_value_caches();
        a->reset_structure_caches();
        CHECK(memcmp(structure_bytes(a), structure_bytes(b), sizeof(bmsp_structure_caches)) == 0);
        a->~bmsp_matrix_s(); b->~bmsp_matrix_s();
        delete m;
        CHECK(g_live.empty());
    }
    {  // bmsp_matrix_invalidate(m, 0): the value group's four allocations and nothing else; the structure group bit for bit as it was
        alignas(bmsp_matrix_s) static unsigned char s0[sizeof(bmsp_matrix_s)], snap[sizeof(bmsp_structure_caches)];
        memset(s0, 0, sizeof s0);
        bmsp_matrix_s *m = new (s0) bmsp_matrix_s();
        m->keys = (uint64_t *)pool_alloc(8); m->bmps = (uint64_t *)pool_alloc(8); m->offsets = (uint64_t *)pool_alloc(16); m->values = pool_alloc(4);
        fill_caches(*m);
        m->shard_view = make_matrix();
        fill_caches(*m->shard_view);
        const void *arr[4] = {m->keys, m->bmps, m->offsets, m->values};
        const uint64_t uid = m->uid;
        const size_t live = g_live.size();
        const long frees = g_frees;
        CHECK(m->holds_memory());
        memcpy(snap, structure_bytes(m), sizeof snap);
        m->reset_value_caches();
        CHECK(g_frees - frees == 4 && g_live.size() == live - 4);
        CHECK(memcmp(snap, structure_bytes(m), sizeof snap) == 0);
        check_value_group_default(*m);
        check_structure_group_filled(*m, true);
        check_structure_group_filled(*m->shard_view, false);
        CHECK(m->shard_view->holds_memory() && m->shard_view->values_finite == 77);  // (the view's values are the parent's, its caches its own call's)
        public_arrays_live(*m, arr);
        CHECK(m->uid == uid);
        m->~bmsp_matrix_s();
        CHECK(g_live.empty());
    }
    {  // re-assigning an owner releases what it held, once: regrow (krylov_ws), rebuild from a temporary (col_index_row), adopt (rowptr)
        size_t n = 0;
        bmsp_matrix_s *m = full_handle(&n);
        const size_t live = g_live.size();
        long frees = g_frees;
        void *old = m->krylov_ws;
        m->krylov_ws.release();
        CHECK(!m->krylov_ws && g_frees - frees == 1 && !g_live.count(old));
        m->krylov_ws.alloc(64);
        CHECK(m->krylov_ws && g_frees - frees == 1 && g_live.size() == live);
        frees = g_frees;
        old = m->col_index_row;
        DevBuf<uint32_t> fresh(5);
        uint32_t *fp = fresh.p;
        m->col_index_row = std::move(fresh);
        CHECK(m->col_index_row == fp && !fresh.p && g_frees - frees == 1 && !g_live.count(old) && g_live.size() == live);
        frees = g_frees;
        old = m->rowptr;
        uint32_t *raw = (uint32_t *)pool_alloc(12);
        m->rowptr.adopt(raw);
        CHECK(m->rowptr == raw && g_frees - frees == 1 && !g_live.count(old) && g_live.size() == live);
        frees = g_frees;
        m->shard_view = make_matrix();  // (comm.hip: another communicator shape) the old view goes with its caches
        CHECK(g_frees - frees == (long)n && g_live.size() == live - n);
        delete m;
        CHECK(g_live.empty());
    }
    {  // delete with ownership 2: the caches go, the four arrays are the caller's
        size_t n = 0;
        bmsp_matrix_s *m = full_handle(&n);
        const void *arr[4] = {m->keys, m->bmps, m->offsets, m->values};
        m->ownership = 2;
        delete m;
        CHECK(g_live.size() == 4);
        for (int i = 0; i < 4; i++) { CHECK(g_live.count((void *)arr[i])); pool_free((void *)arr[i]); }
        CHECK(g_live.empty());
    }
    {  // a buffer moved out of the handle is no longer the handle's to free
        size_t n = 0;
        bmsp_matrix_s *m = full_handle(&n);
        uint32_t *map = m->tp_map.take();
        DevBuf<uint32_t> tasks_begin = std::move(m->sp_task_begin);
        void *tb = tasks_begin.p;
        CHECK(!m->tp_map && !m->sp_task_begin);
        delete m;
        CHECK(g_live.size() == 2 && g_live.count(map) && g_live.count(tb));
        pool_free(map);
    }
    CHECK(g_live.empty());
    if (g_bad) return 1;
    printf("OK owners=%zu\n", owners);
    return 0;
}
