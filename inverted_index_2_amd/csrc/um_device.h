// um_device.h — device helpers shared by the block-wise paths (union_many.hip, count_ranges.hip): the segmented OR that
// leaves one atomic per touched bitmap word, and the search of the range that owns a query block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dv1_device.h"

namespace ii2 {

// inclusive scan by `op` over the lanes of each run of equal keys (runs are contiguous): the run's last lane holds the run's total
template <class Op>
__device__ __forceinline__ uint32_t seg_scan(uint32_t key, uint32_t v, Op op) {
    const int l = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ok = (uint32_t)__shfl_up((int)key, d, 64);
        const uint32_t ov = (uint32_t)__shfl_up((int)v, d, 64);
        if (l >= d && ok == key) v = op(v, ov);
    }
    return v;
}
// ... the run's OR
__device__ __forceinline__ uint32_t seg_or(uint32_t key, uint32_t bits) {
    return seg_scan(key, bits, [](uint32_t a, uint32_t b) { return a | b; });
}
// ... the run's sum (histogram.hip)
__device__ __forceinline__ uint32_t seg_add(uint32_t key, uint32_t n) {
    return seg_scan(key, n, [](uint32_t a, uint32_t b) { return a + b; });
}

// the range that holds query block g: the last r with pre[r] <= g
__device__ __forceinline__ uint32_t um_range_of(const uint32_t *pre, uint32_t n_ranges, uint32_t g) {
    uint32_t lo = 0, hi = n_ranges;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pre[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace ii2
