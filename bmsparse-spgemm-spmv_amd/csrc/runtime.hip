// runtime.hip -- error state, pooled device memory.
#include "runtime.h"
#include <atomic>
#include <map>
#include <mutex>
#include <unordered_map>
#include <vector>
#include <algorithm>
#include <cstring>

namespace bmsp {

uint64_t next_matrix_uid()
{
    static std::atomic<uint64_t> next{1};
    return next.fetch_add(1);
}

static thread_local std::string g_last_error;

void set_last_error(const std::string &msg) { g_last_error = msg; }
const std::string &last_error() { return g_last_error; }

[[noreturn]] void fail(int status, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw Error(status, buf);
}

namespace {
// Blocks of at most kSlabMax bytes are carved out of 64 MiB slabs (one hipMalloc per slab): the first product on a fresh matrix needs
// a dozen small temporaries and cached arrays, and a hipMalloc of its own for each cost 0.1 - 0.3 ms apiece (SpMV prepare: 1.9 ms of host
// time for 0.13 ms of kernels).  Carved blocks go back to the size-class lists like any other and are never returned to the driver.
constexpr size_t kSlabBytes = 64u << 20, kSlabMax = 8u << 20;
struct Slab {
    char *base;
    size_t used;
};
struct Pool {
    std::mutex mu;
    std::map<std::pair<int, size_t>, std::vector<void *>> free_blocks;  // (device, rounded size) -> blocks
    std::unordered_map<void *, std::pair<int, size_t>> live;            // every block we ever allocated -> (device, rounded size)
    std::unordered_map<void *, bool> carved;                            // blocks that are part of a slab (never hipFree'd on their own)
    std::map<int, Slab> slab;                                           // device -> the slab being carved
    ~Pool() {}                                          // leave memory to process teardown (runtime may be gone)
};
Pool &pool()
{
    static Pool *p = new Pool();
    return *p;
}
size_t round_size(size_t b)
{
    if (b < 512) return 512;
    if (b <= (1u << 20)) return (b + 511) & ~size_t(511);
    // above 1 MiB: round up to 1/8 of the leading power of two, so a block is reusable for similar sizes
    size_t p2 = size_t(1) << (63 - __builtin_clzll((unsigned long long)b));
    size_t step = p2 >> 3;
    return (b + step - 1) / step * step;
}
}  // namespace

void *pool_alloc(size_t bytes)
{
    // every block carries kPoolSlack readable bytes past the requested size: kernels that fetch a tile's values with one wide
    // load may touch (and discard) up to 12 bytes beyond the last stored value
    size_t r = round_size(bytes + kPoolSlack);
    int dev = 0;
    (void)hipGetDevice(&dev);  // a block is only ever handed out on the device it was allocated on (bmsp_set_device may change it)
    Pool &P = pool();
    {
        std::lock_guard<std::mutex> lk(P.mu);
        auto it = P.free_blocks.find(std::make_pair(dev, r));
        if (it != P.free_blocks.end() && !it->second.empty()) {
            void *p = it->second.back();
            it->second.pop_back();
            return p;
        }
    }
    void *p = nullptr;
    if (r <= kSlabMax && !getenv("BMSP_POOL_NO_SLAB")) {
        std::lock_guard<std::mutex> lk(P.mu);
        Slab &sl = P.slab[dev];
        const size_t need = (r + 255) & ~size_t(255);
        if (!sl.base || sl.used + need > kSlabBytes) {
            char *nb = nullptr;
            if (hipMalloc((void **)&nb, kSlabBytes) == hipSuccess) { sl.base = nb; sl.used = 0; }
            else { (void)hipGetLastError(); sl.base = nullptr; }
        }
        if (sl.base) {
            p = sl.base + sl.used;
            sl.used += need;
            P.live[p] = std::make_pair(dev, r);
            P.carved[p] = true;
            return p;
        }
    }
    hipError_t e = hipMalloc(&p, r);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        pool_trim();
        e = hipMalloc(&p, r);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            fail(BMSP_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", r, hipGetErrorString(e));
        }
    }
    std::lock_guard<std::mutex> lk(P.mu);
    P.live[p] = std::make_pair(dev, r);
    return p;
}

void pool_free(void *p)
{
    if (!p) return;
    Pool &P = pool();
    std::lock_guard<std::mutex> lk(P.mu);
    auto it = P.live.find(p);
    if (it == P.live.end()) return;  // not ours (borrowed pointer): leave it alone
    P.free_blocks[it->second].push_back(p);
}

// ---- pinned host scalars (prims.hip.h: HostScalar) ----------------------------------------------------------
namespace {
struct SlotPool {
    std::mutex mu;
    std::vector<void *> free_slots;
};
SlotPool &slots()
{
    static SlotPool *p = new SlotPool();
    return *p;
}
}  // namespace

void *host_slot_acquire()
{
    SlotPool &S = slots();
    {
        std::lock_guard<std::mutex> lk(S.mu);
        if (!S.free_slots.empty()) {
            void *p = S.free_slots.back();
            S.free_slots.pop_back();
            return p;
        }
    }
    // one page of 64-byte slots per refill; never returned to the driver (a handful of pages per process)
    char *page = nullptr;
    BMSP_HIP(hipHostMalloc((void **)&page, 4096, hipHostMallocDefault));
    std::lock_guard<std::mutex> lk(S.mu);
    for (int i = 1; i < 64; i++) S.free_slots.push_back(page + 64 * i);
    return page;
}

void host_slot_release(void *p)
{
    if (!p) return;
    SlotPool &S = slots();
    std::lock_guard<std::mutex> lk(S.mu);
    S.free_slots.push_back(p);
}

bool pool_owns(void *p)
{
    Pool &P = pool();
    std::lock_guard<std::mutex> lk(P.mu);
    return P.live.find(p) != P.live.end();
}

void warm_blockmac32(hipStream_t st);
void warm_blockmac_f32(hipStream_t st);
void warm_blockmac_strip(hipStream_t st);
void warm_blockmac_rowsparse(hipStream_t st);
void warm_builder(hipStream_t st);
void warm_rowmerge(hipStream_t st);
void warm_rowwindow(hipStream_t st);
void warm_segsort(hipStream_t st);
void warm_spgemm(hipStream_t st);
void warm_spmm(hipStream_t st);
void warm_spmv(hipStream_t st);
void warm_shard(hipStream_t st);
void warm_comm(hipStream_t st);
void warm_transpose(hipStream_t st);
void warm_add(hipStream_t st);
void warm_prune(hipStream_t st);
void warm_select(hipStream_t st);
void warm_diag(hipStream_t st);
void warm_spmv_op(hipStream_t st);
void warm_sddmm(hipStream_t st);
void warm_spgemm_masked(hipStream_t st);
void warm_spmm_op(hipStream_t st);
void warm_spsv(hipStream_t st);
void warm_spsm(hipStream_t st);
void warm_spitsv(hipStream_t st);
void warm_ilu0(hipStream_t st);
void warm_krylov(hipStream_t st);
void warm_gmres(hipStream_t st);
void warm_reorder(hipStream_t st);
void warm_aggregate(hipStream_t st);
void warm_multigrid(hipStream_t st);
void warm_fsai(hipStream_t st);

void *host_slot_acquire();
void host_slot_release(void *p);

void load_kernels()
{
    static std::mutex mu;
    static std::vector<int> done;  // devices whose code objects are resident
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return; }
    std::lock_guard<std::mutex> lk(mu);
    for (int d : done)
        if (d == dev) return;
    done.push_back(dev);
    if (getenv("BMSP_LAZY_KERNELS")) return;
    warm_blockmac32(nullptr);
    warm_blockmac_f32(nullptr);
    warm_blockmac_strip(nullptr);
    warm_blockmac_rowsparse(nullptr);
    warm_builder(nullptr);
    warm_rowmerge(nullptr);
    warm_rowwindow(nullptr);
    warm_segsort(nullptr);
    warm_spgemm(nullptr);
    warm_spmm(nullptr);
    warm_spmv(nullptr);
    warm_shard(nullptr);
    warm_comm(nullptr);
    warm_transpose(nullptr);
    warm_add(nullptr);
    warm_prune(nullptr);
    warm_select(nullptr);
    warm_diag(nullptr);
    warm_spmv_op(nullptr);
    warm_sddmm(nullptr);
    warm_spgemm_masked(nullptr);
    warm_spmm_op(nullptr);
    warm_spsv(nullptr);
    warm_spsm(nullptr);
    warm_spitsv(nullptr);
    warm_ilu0(nullptr);
    warm_krylov(nullptr);
    warm_gmres(nullptr);
    warm_reorder(nullptr);
    warm_aggregate(nullptr);
    warm_multigrid(nullptr);
    warm_fsai(nullptr);
    // the first pinned host page and the first device-to-host copy of a process cost ~15 ms (measured inside the first product's T_1):
    // taken here too, with a copy through the slot
    // ... and so does the first timed event of a process (the stage timers' events; the queue is switched to profiling)
    {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
            (void)hipEventRecord(e0, nullptr);
            warm_builder(nullptr);
            (void)hipEventRecord(e1, nullptr);
            (void)hipEventSynchronize(e1);
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, e0, e1);
        }
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    void *slot = host_slot_acquire();
    void *d = pool_alloc(64);
    (void)hipMemsetAsync(d, 0, 64, nullptr);
    (void)hipMemcpyAsync(slot, d, 64, hipMemcpyDeviceToHost, nullptr);
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    pool_free(d);
    host_slot_release(slot);
}

namespace {
constexpr size_t kStageBytes = 8u << 20;
struct Stage {
    std::mutex mu;
    char *buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipStream_t st = nullptr;
};
Stage &stage()
{
    static Stage *s = new Stage();
    return *s;
}
void stage_init(Stage &S)
{
    if (S.buf[0]) return;
    for (int i = 0; i < 2; i++) {
        BMSP_HIP(hipHostMalloc((void **)&S.buf[i], kStageBytes, hipHostMallocDefault));
        BMSP_HIP(hipEventCreateWithFlags(&S.ev[i], hipEventDisableTiming));
    }
    BMSP_HIP(hipStreamCreateWithFlags(&S.st, hipStreamNonBlocking));
}
}  // namespace

void copy_h2d_staged(void *dst, const void *src, size_t bytes)
{
    if (!bytes) return;
    Stage &S = stage();
    std::lock_guard<std::mutex> lk(S.mu);
    stage_init(S);
    BMSP_HIP(hipDeviceSynchronize());  // (a synchronous copy: earlier work on dst is done, as hipMemcpy would have it)
    int cur = 0;
    for (size_t off = 0; off < bytes; off += kStageBytes, cur ^= 1) {
        const size_t n = std::min(kStageBytes, bytes - off);
        if (off >= 2 * kStageBytes) BMSP_HIP(hipEventSynchronize(S.ev[cur]));  // the copy that last used this half has left it
        memcpy(S.buf[cur], (const char *)src + off, n);
        BMSP_HIP(hipMemcpyAsync((char *)dst + off, S.buf[cur], n, hipMemcpyHostToDevice, S.st));
        BMSP_HIP(hipEventRecord(S.ev[cur], S.st));
    }
    BMSP_HIP(hipStreamSynchronize(S.st));
}

void copy_d2h_staged(void *dst, const void *src, size_t bytes)
{
    if (!bytes) return;
    Stage &S = stage();
    std::lock_guard<std::mutex> lk(S.mu);
    stage_init(S);
    BMSP_HIP(hipDeviceSynchronize());
    // chunk k travels while chunk k - 1 is copied out of its half
    size_t prev_off = 0, prev_n = 0;
    int cur = 0;
    for (size_t off = 0; off < bytes; off += kStageBytes, cur ^= 1) {
        const size_t n = std::min(kStageBytes, bytes - off);
        BMSP_HIP(hipMemcpyAsync(S.buf[cur], (const char *)src + off, n, hipMemcpyDeviceToHost, S.st));
        BMSP_HIP(hipEventRecord(S.ev[cur], S.st));
        if (prev_n) {
            BMSP_HIP(hipEventSynchronize(S.ev[cur ^ 1]));
            memcpy((char *)dst + prev_off, S.buf[cur ^ 1], prev_n);
        }
        prev_off = off; prev_n = n;
    }
    BMSP_HIP(hipEventSynchronize(S.ev[cur ^ 1]));
    memcpy((char *)dst + prev_off, S.buf[cur ^ 1], prev_n);
}

void pool_trim()
{
    Pool &P = pool();
    std::vector<void *> victims;
    {
        std::lock_guard<std::mutex> lk(P.mu);
        for (auto &kv : P.free_blocks) {
            std::vector<void *> keep;
            for (void *p : kv.second) {
                if (P.carved.count(p)) { keep.push_back(p); continue; }  // part of a slab: stays in its list
                victims.push_back(p);
                P.live.erase(p);
            }
            kv.second.swap(keep);
        }
    }
    if (!victims.empty()) (void)hipDeviceSynchronize();
    for (void *p : victims) (void)hipFree(p);
}

}  // namespace bmsp
