// hist_device.h — the bucket arithmetic of the histograms (ii2_histogram_ranges, ii2_histogram_ids), shared by their kernels
// (histogram.hip) and the host-only entry points ii2_hist_bucket / ii2_hist_block (setop.cpp).  The axis is `first`, the first id
// of every bucket, strictly ascending, plus `last`, the inclusive last id of the last bucket: the host passes its 64-bit edges, the
// device a uint32 copy of edges[0 .. n_buckets) - edges[n_buckets] - 1 fits 32 bits where the edge itself, 2^32, does not.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ii2 {

constexpr int HIST_SKIP = 0, HIST_WHOLE = 1, HIST_SPLIT = 2, HIST_WIDE = 3;      // II2_HIST_* of ii2.h
constexpr uint32_t HIST_STRIP = 64;      // buckets a SPLIT block meets at most: one counter per lane of a wave

// the bucket of id among the buckets lo .. hi: the last b with first[b] <= id, and lo where there is none (the caller has clipped
// id to the axis, or tests it against the axis itself)
template <class E>
__host__ __device__ inline uint32_t hist_find(const E *first, uint32_t lo, uint32_t hi, uint32_t id) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
        if (first[mid] <= (E)id) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

// the bucket of id on the whole axis, -1 outside it
template <class E>
__host__ __device__ inline int64_t hist_bucket(const E *first, uint32_t n_buckets, uint32_t last, uint32_t id) {
    if ((E)id < first[0] || id > last) return -1;
    return (int64_t)hist_find(first, 0u, n_buckets - 1u, id);
}

// What a block with the doc bounds [first_doc, up] is to the axis: SKIP - the bounds miss it; else b_lo .. b_hi are the buckets the
// bounds, clipped to the axis, meet, and the block is WHOLE - both bounds inside one bucket -, SPLIT - 2 .. HIST_STRIP buckets, or
// one bucket with a bound outside the axis - or WIDE - more.  first0 = first[0], which the kernels hold in a register: most
// blocks of a coarse axis are then placed without reading the edges at all.
template <class E>
__host__ __device__ inline int hist_block(const E *first, uint32_t n_buckets, E first0, uint32_t last, uint32_t first_doc, uint32_t up,
                                          uint32_t *b_lo, uint32_t *b_hi) {
    if (up < first_doc || first_doc > last || (E)up < first0) return HIST_SKIP;
    const bool below = (E)first_doc < first0, above = up > last;
    const uint32_t lo = below ? 0u : hist_find(first, 0u, n_buckets - 1u, first_doc);
    const uint32_t hi = above ? n_buckets - 1u : hist_find(first, lo, n_buckets - 1u, up);
    *b_lo = lo;
    *b_hi = hi;
    if (lo == hi && !below && !above) return HIST_WHOLE;
    return hi - lo < HIST_STRIP ? HIST_SPLIT : HIST_WIDE;
}

}  // namespace ii2
