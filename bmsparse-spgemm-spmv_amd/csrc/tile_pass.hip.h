// tile_pass.hip.h -- what the tile-wise passes over a matrix already on the device share (transpose.hip, add.hip, prune.hip, diag.hip):
// how many lanes a tile gets and how a pass is launched at that width, the dispatch on dtype / element width, the value types of a
// dtype, and the key search inside a block-row.  The kernels themselves stay in their files: they differ where it matters (shuffles,
// atomics, contraction).  The bit-level facts of the tile format are in bmsp_bits.h.
#ifndef BMSP_TILE_PASS_HIP_H_
#define BMSP_TILE_PASS_HIP_H_

#include "matrix.h"
#include "prims.hip.h"
#include <cstdlib>
#include <type_traits>

namespace bmsp {

// Lanes per tile of a value pass, from the mean tile fill: a lane per tile below 6 values (the headline R-MAT: 1.5; fem_like 27pt: 3.7),
// eight lanes from there (banded: 58).  G = 1: a lane walks its tile's few values; G = 8: lane t takes byte t of the bitmap, consecutive
// lanes on consecutive values of one segment (a wave per tile measured slower even on full tiles, DESIGN §4 "Transpose", where the
// threshold was measured).  The environment variable `override_var` = 1 / 8 forces one (measurement and test switch, read per call).
// `threshold`: the mean fill from which eight lanes are the default, for a pass that measured another one than the family's 6.
inline int lane_group(int64_t nnz, int64_t nb, const char *override_var, int64_t threshold = 6)
{
    if (const char *e = getenv(override_var)) {
        const int g = atoi(e);
        if (g == 1 || g == 8) return g;
    }
    return nb == 0 || nnz < threshold * nb ? 1 : 8;
}

// Launches a pass over `tiles` tiles at g = 1 or 8 lanes per tile: launch(std::integral_constant<int, G>, grid) names the kernel
// instantiated for G and passes its arguments; the grid holds tiles * G lanes.
template <typename Launch>
void launch_lane_group(int g, uint64_t tiles, Launch &&launch)
{
    if (g == 8) launch(std::integral_constant<int, 8>{}, grid_for(tiles * 8));
    else launch(std::integral_constant<int, 1>{}, grid_for(tiles));
    BMSP_CHECK_LAUNCH();
}

// fn(S{}) with the storage type S of a dtype: uint16_t (the bits of an fp16), float, double
template <typename Fn>
void dispatch_dtype(bmsp_dtype dtype, Fn &&fn)
{
    if (dtype == BMSP_F16) fn(uint16_t{});
    else if (dtype == BMSP_F32) fn(float{});
    else fn(double{});
}

// fn(T{}) with the unsigned integer T of a dtype's element width, for passes that move values as raw bits
template <typename Fn>
void dispatch_width(bmsp_dtype dtype, Fn &&fn)
{
    const size_t es = dtype_size(dtype);
    if (es == 2) fn(uint16_t{});
    else if (es == 4) fn(uint32_t{});
    else fn(uint64_t{});
}

// Storage type S of a dtype: F the type its arithmetic runs in (fp16: fp32, one RNE rounding at the end), R the type of the vectors
// that go with the matrix (bmsp_spmv's convention for u: row maxima, diagonals, scaling factors), U the bits of an R.
//   load / store  exact widening to F; back with one rounding to nearest even (fp16: through f64_to_f16_bits, the builder's rounding)
//   abs_bits      the bits of |s| as an R: non-negative values order as unsigned integers, NaN bits lie above kInf
//   widen         the stored value as a double, exactly
template <typename S>
struct TileValue;
template <>
struct TileValue<float> {
    using F = float;
    using R = float;
    using U = uint32_t;
    static constexpr U kInf = 0x7f800000u;
    static __device__ __forceinline__ F load(float s) { return s; }
    static __device__ __forceinline__ float store(F f) { return f; }
    static __device__ __forceinline__ U abs_bits(float s) { return __builtin_bit_cast(uint32_t, s) & 0x7fffffffu; }
    static __device__ __forceinline__ double widen(float s) { return (double)s; }
};
template <>
struct TileValue<uint16_t> {
    using F = float;
    using R = float;
    using U = uint32_t;
    static constexpr U kInf = 0x7f800000u;
    static __device__ __forceinline__ F load(uint16_t s) { return (float)__builtin_bit_cast(_Float16, s); }
    static __device__ __forceinline__ uint16_t store(F f) { return f64_to_f16_bits((double)f); }  // exact widening, then one rounding
    static __device__ __forceinline__ U abs_bits(uint16_t s)
    {
        return __builtin_bit_cast(uint32_t, (float)__builtin_bit_cast(_Float16, (uint16_t)(s & 0x7fffu)));
    }
    static __device__ __forceinline__ double widen(uint16_t s) { return (double)__builtin_bit_cast(_Float16, s); }
};
template <>
struct TileValue<double> {
    using F = double;
    using R = double;
    using U = uint64_t;
    static constexpr U kInf = 0x7ff0000000000000ull;
    static __device__ __forceinline__ F load(double s) { return s; }
    static __device__ __forceinline__ double store(F f) { return f; }
    static __device__ __forceinline__ U abs_bits(double s) { return __builtin_bit_cast(uint64_t, s) & 0x7fffffffffffffffull; }
    static __device__ __forceinline__ double widen(double s) { return s; }
};

// The epilogue of the sampled products (sddmm.hip, spgemm_masked.hip): c from the dot product d and the stored value s of the pattern.
enum { kModeAlpha = 0, kModeAdd = 1, kModeMul = 2 };  // c = alpha*d | alpha*d + beta*s | alpha*d * s

// alpha and beta rounded once to the arithmetic type decide the form: beta == 0 there means s is not read
inline int epilogue_mode(bmsp_dtype dtype, double beta, bool mul)
{
    if (mul) return kModeMul;
    const bool zero = dtype == BMSP_F64 ? beta == 0.0 : (float)beta == 0.0f;
    return zero ? kModeAlpha : kModeAdd;
}

// c from the dot product d and the stored s (read only when mode says so): each operation rounded on its own, never contracted
template <typename F>
__device__ __forceinline__ F epilogue(F d, F alpha, F beta, F s, int mode)
{
#pragma clang fp contract(off)
    const F t = alpha * d;
    if (mode == kModeMul) return t * s;
    if (mode == kModeAdd) {
        const F u = beta * s;
        return t + u;
    }
    return t;
}

// first index in [lo, hi) whose key is >= k; [lo, hi) is a block-row's range of the cached block-row pointer
__device__ __forceinline__ uint32_t lower_bound_key(const uint64_t *keys, uint32_t lo, uint32_t hi, uint64_t k)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

}  // namespace bmsp
#endif
