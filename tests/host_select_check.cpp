// host_select_check.cpp -- the bit helpers of band selection (csrc/bmsp_bits.h) on the host, no HIP: tile_band_mask against a brute-force
// loop over the 64 positions, its mirror for column-major tiles against tile_transpose, and the whole-tile keep / drop conditions with
// tile_band_select against the per-entry predicate lo <= col - row <= hi.  Built and run by tests/test_select_api.py; prints the failures
// and exits 1 when there are any.
#include "bmsp_bits.h"
#include <cstdio>
#include <vector>

using namespace bmsp;

static uint64_t brute_mask(int64_t dlo, int64_t dhi)
{
    uint64_t m = 0;
    for (int r = 0; r < 8; r++)
        for (int c = 0; c < 8; c++)
            if (dlo <= c - r && c - r <= dhi) m |= 1ull << (63 - (8 * r + c));
    return m;
}

int main()
{
    int bad = 0;
    for (int dlo = -9; dlo <= 9; dlo++)
        for (int dhi = -9; dhi <= 9; dhi++) {
            const uint64_t m = tile_band_mask(dlo, dhi);
            if (m != brute_mask(dlo, dhi)) { std::printf("FAIL mask(%d, %d) = %016llx\n", dlo, dhi, (unsigned long long)m); bad++; }
            if (tile_band_mask(-dhi, -dlo) != tile_transpose(m)) { std::printf("FAIL mirror(%d, %d)\n", dlo, dhi); bad++; }
        }
    // a tile at block distance delta: entry (r, c) lies on the matrix diagonal 8 delta + c - r
    const int64_t clamp = 1ll << 36;
    std::vector<int64_t> bounds;
    for (int64_t v = -30; v <= 30; v++) bounds.push_back(v);
    bounds.push_back(-clamp);
    bounds.push_back(clamp);
    const uint64_t patterns[] = {~0ull, 0x8040201008040201ull, 0x0123456789abcdefull, 0xf0e1d2c3b4a59687ull};
    for (int64_t delta = -3; delta <= 3; delta++)
        for (int64_t lo : bounds)
            for (int64_t hi : bounds) {
                uint64_t in = 0;  // row-major positions inside the band
                for (int r = 0; r < 8; r++)
                    for (int c = 0; c < 8; c++)
                        if (lo <= 8 * delta + c - r && 8 * delta + c - r <= hi) in |= 1ull << (63 - (8 * r + c));
                if (tile_band_misses(delta, lo, hi) != (in == 0) && lo <= hi) {
                    std::printf("FAIL misses(%lld, %lld, %lld)\n", (long long)delta, (long long)lo, (long long)hi); bad++;
                }
                if (tile_band_misses(delta, lo, hi) && in != 0) { std::printf("FAIL misses drops entries (%lld, %lld, %lld)\n", (long long)delta, (long long)lo, (long long)hi); bad++; }
                if (tile_band_covers(delta, lo, hi) != (in == ~0ull)) {
                    std::printf("FAIL covers(%lld, %lld, %lld)\n", (long long)delta, (long long)lo, (long long)hi); bad++;
                }
                for (uint64_t bmp : patterns) {
                    if (tile_band_select(bmp, delta, lo, hi, 0) != (bmp & in)) { std::printf("FAIL select row-major (%lld, %lld, %lld)\n", (long long)delta, (long long)lo, (long long)hi); bad++; }
                    if (tile_band_select(bmp, delta, lo, hi, 1) != (bmp & tile_transpose(in))) { std::printf("FAIL select column-major (%lld, %lld, %lld)\n", (long long)delta, (long long)lo, (long long)hi); bad++; }
                }
            }
    std::printf("%s\n", bad ? "FAILED" : "CHECK host select OK");
    return bad ? 1 : 0;
}
