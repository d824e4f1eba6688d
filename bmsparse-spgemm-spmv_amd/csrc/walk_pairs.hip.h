// walk_pairs.hip.h -- the intersection walk that spgemm_masked.hip and ilu0.hip share: for an output tile (I, J), the pairs of a tile of
// block-row I of one operand and a tile of block-column J of another with the same inner block index, in ascending order of that index.
// The block-row is a range of the operand's own arrays (block-row pointer), the block-column a range of the records of the cached op-T
// view of bmsp_spmv_op (spmv_op_ensure_view).  The kernels stay in their files: they differ in what a pair contributes.
#ifndef BMSP_WALK_PAIRS_HIP_H_
#define BMSP_WALK_PAIRS_HIP_H_

#include "tile_pass.hip.h"

namespace bmsp {

// The two candidate lists of an M tile, as sequences of entries with an inner block index `k` and whatever a match needs of the tile --
// loaded with the index in one go, so that nothing is fetched after a match is known.
//   A's block-row: tiles [lo, hi) of A, block columns ascending.  FULL = false (the counting walk) loads the key alone.
template <bool FULL>
struct ListA {
    struct Entry {
        uint32_t k;
        uint64_t bmp, off;
    };
    const uint64_t *__restrict__ keys, *__restrict__ bmps, *__restrict__ offsets;
    __device__ __forceinline__ Entry load(uint32_t i) const
    {
        Entry e;
        e.k = key_col(keys[i]);
        e.bmp = FULL ? bmps[i] : 0;
        e.off = FULL ? offsets[i] : 0;
        return e;
    }
};
//   B's block-column: records [lo, hi) of B's op-T view {bitmap lo, hi, value offset, block-row}, block-rows ascending
struct ListB {
    struct Entry {
        uint32_t k;
        uint64_t bmp, off;
    };
    const uint4 *__restrict__ recs;
    __device__ __forceinline__ Entry load(uint32_t i) const
    {
        const uint4 r = recs[i];
        Entry e;
        e.k = r.w;
        e.bmp = (uint64_t)r.y << 32 | r.x;
        e.off = r.z;
        return e;
    }
};

// Lower bound of k in list[left, hi), searched from the left end: probes at distance 1, 2, 4, .. until an entry is not below k, then
// halvings inside the last step -- 2 * log2(distance) loads, one load when the next match is the next entry (lists of like length).
// Returns the index; found = list[index].k == k, and then `hit` is that entry (the last probe that was not below k).  Both loops are
// bounded by 32.
template <typename L>
__device__ __forceinline__ uint32_t lower_bound_from(const L &list, uint32_t left, uint32_t hi, uint32_t k, typename L::Entry &hit, bool &found)
{
    uint32_t lo = left, end = hi, step = 1;
    bool have = false;
    for (int s = 0; s < 32 && lo < end; s++) {
        const uint32_t room = end - lo;
        const uint32_t p = lo + (step < room ? step : room) - 1;
        const typename L::Entry e = list.load(p);
        if (e.k < k) {
            lo = p + 1;
            step <<= 1;
        } else {
            end = p;
            hit = e;
            have = true;
            break;
        }
    }
    for (int s = 0; s < 32 && lo < end; s++) {
        const uint32_t mid = lo + ((end - lo) >> 1);
        const typename L::Entry e = list.load(mid);
        if (e.k < k) lo = mid + 1;
        else {
            end = mid;
            hit = e;
        }
    }
    found = have && hit.k == k;
    return lo;
}

// fn(a, b) for every pair of an entry of A's block-row [a_lo, a_hi) and an entry of B's block-column [b_lo, b_hi) with the same inner
// block index, in ascending order of that index.  The shorter list is walked, its next entry loaded one step ahead; each entry is found
// in the longer list by lower_bound_from, whose left end carries forward from the previous hit: min * log(max / min) loads and not a walk
// of both lists.  Every loop is bounded by a list length (the searches by 32).
template <typename LA, typename Fn>
__device__ __forceinline__ void walk_pairs(const LA &la, uint32_t a_lo, uint32_t a_hi, const ListB &lb, uint32_t b_lo, uint32_t b_hi, Fn &&fn)
{
    if (a_lo >= a_hi || b_lo >= b_hi) return;
    if (a_hi - a_lo <= b_hi - b_lo) {
        uint32_t left = b_lo;
        typename LA::Entry next = la.load(a_lo);
        for (uint32_t a = a_lo; a < a_hi; a++) {
            const typename LA::Entry cur = next;
            next = la.load(a + 1 < a_hi ? a + 1 : a);
            if (left >= b_hi) break;
            ListB::Entry hit;
            bool found;
            left = lower_bound_from(lb, left, b_hi, cur.k, hit, found);
            if (found) {
                fn(cur, hit);
                left++;
            }
        }
    } else {
        uint32_t left = a_lo;
        ListB::Entry next = lb.load(b_lo);
        for (uint32_t b = b_lo; b < b_hi; b++) {
            const ListB::Entry cur = next;
            next = lb.load(b + 1 < b_hi ? b + 1 : b);
            if (left >= a_hi) break;
            typename LA::Entry hit;
            bool found;
            left = lower_bound_from(la, left, a_hi, cur.k, hit, found);
            if (found) {
                fn(hit, cur);
                left++;
            }
        }
    }
}

}  // namespace bmsp
#endif
