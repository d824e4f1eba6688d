// The floor of the chunked SpMV sweep (spmv_chunk_kernel) with everything but its memory pattern stripped: one wave per V stored values,
// lane l loads values 8l .. 8l+7 of its chunk (two 16-byte loads of the value words, two of the values), issues the eight x gathers back to
// back and stores ONE sum per lane -- no record, no reduction, no fold.  Shape of the webbase-1M stand-in: 3.13 M values over 2^20 rows and
// columns, R-MAT column skew (a = 0.57, b = 0.19, c = 0.19), values in bmSparse storage order (block-row, block column, position), nine
// copies rotated so that the streams come from HBM.  Go / no-go of DESIGN.md round 5: the full kernel cannot beat this number.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

template <int V>
__global__ __launch_bounds__(64) void chunk_floor_kernel(const uint32_t *__restrict__ words, const float *__restrict__ vals, const float *__restrict__ x,
                                                         float *__restrict__ y, uint32_t nnz, uint32_t ncols)
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    constexpr int P = V / 64;
    const uint32_t first = blockIdx.x * V + (threadIdx.x & 63) * P;
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(words), 0, nnz * 4u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(vals), 0, nnz * 4u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(x), 0, ncols * 4u, 0x00020000);
    uint32_t w[P];
    float a[P];
#pragma unroll
    for (int q = 0; q < P; q += 4) {
        const u4 wq = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(rw, (first + q) * 4u, 0, 0));
        const f4 aq = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rv, (first + q) * 4u, 0, 0));
#pragma unroll
        for (int i = 0; i < 4; i++) { w[q + i] = wq[i]; a[q + i] = aq[i]; }
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < P; j++) s += a[j] * __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, (w[j] & 0xfffffu) * 4u, 0, 0));
    y[blockIdx.x * 64 + (threadIdx.x & 63)] = s;
}

int main()
{
    const uint32_t scale = 20, n = 1u << scale, m = 2u << scale, copies = 9;
    uint64_t z = 12345;
    auto next = [&z]() { z = z * 6364136223846793005ull + 1442695040888963407ull; return (double)(z >> 11) * (1.0 / 9007199254740992.0); };
    std::vector<uint64_t> cells;
    for (uint32_t e = 0; e < m + n; e++) {
        uint32_t r = 0, c = 0;
        if (e < m) {
            for (uint32_t l = 0; l < scale; l++) {
                const double u = next();
                r = (r << 1) | (u >= 0.76 ? 1u : 0u);
                c = (c << 1) | (((u >= 0.57 && u < 0.76) || u >= 0.95) ? 1u : 0u);
            }
        } else {
            r = c = e - m;  // the identity
        }
        cells.push_back(((uint64_t)(r >> 3) << 43) | ((uint64_t)(c >> 3) << 26) | ((uint64_t)(((r & 7u) << 3) | (c & 7u)) << 20) | c);
    }
    std::sort(cells.begin(), cells.end());
    cells.erase(std::unique(cells.begin(), cells.end()), cells.end());
    const uint32_t nnz = (uint32_t)cells.size();
    std::vector<uint32_t> hw(nnz + 1024, 0);
    for (uint32_t i = 0; i < nnz; i++) hw[i] = (uint32_t)(cells[i] & 0xfffffu);
    printf("nnz %u\n", nnz);
    uint32_t *dw[copies];
    float *dv[copies], *dx, *dy;
    for (uint32_t c = 0; c < copies; c++) {
        hipMalloc((void **)&dw[c], 4ull * hw.size()); hipMemcpy(dw[c], hw.data(), 4ull * hw.size(), hipMemcpyHostToDevice);
        hipMalloc((void **)&dv[c], 4ull * hw.size()); hipMemset(dv[c], 0, 4ull * hw.size());
    }
    hipMalloc((void **)&dx, 4ull * n); hipMemset(dx, 0, 4ull * n);
    hipMalloc((void **)&dy, 4ull * (nnz / 4 + 1024));  // one float per lane: full / V * 64 <= nnz / 4
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    const uint32_t full = nnz / 1024 * 1024;  // whole chunks of every V below (no bounds checks in the kernel)
#define RUN(V)                                                                                                                              \
    {                                                                                                                                       \
        const uint32_t g = full / V;                                                                                                        \
        for (int it = 0; it < 20; it++) hipLaunchKernelGGL(chunk_floor_kernel<V>, dim3(g), dim3(64), 0, 0, dw[it % copies], dv[it % copies], dx, dy, full, n); \
        hipEventRecord(e0, 0);                                                                                                              \
        const int reps = 200;                                                                                                               \
        for (int it = 0; it < reps; it++) hipLaunchKernelGGL(chunk_floor_kernel<V>, dim3(g), dim3(64), 0, 0, dw[it % copies], dv[it % copies], dx, dy, full, n); \
        hipEventRecord(e1, 0); hipEventSynchronize(e1);                                                                                     \
        float ms = 0; hipEventElapsedTime(&ms, e0, e1);                                                                                     \
        printf("V %4d: %u waves, %.2f us per sweep over %u values\n", V, g, ms * 1e3 / reps, full);                                       \
    }
    RUN(256) RUN(512) RUN(1024)
    return 0;
}
