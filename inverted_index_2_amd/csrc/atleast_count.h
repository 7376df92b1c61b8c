// atleast_count.h — the counter arithmetic of the threshold query's counting form (ii2_atleast_ranges: atleast.hip, setop.cpp).
// A doc's counter is bit-sliced: bit b of the counter of the doc at bit i of a bitmap word is bit i of plane word pl[b], plane 0
// the least significant.  The device kernels and the host-only exports (ii2_atleast_plan, ii2_atleast_word) run the same code.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define II2_HD __host__ __device__ inline
#else
#define II2_HD inline
#endif

namespace ii2 {

constexpr uint32_t THR_MAX_PLANES = 8;                      // counters of at most 8 bits: min_match <= 255
constexpr uint64_t THR_PLANE_DOCS = 1ull << 30;             // docs x planes of one window: 128 MiB of planes

// bits of v: the planes a counter needs to reach min_match = v (0 for 0)
II2_HD uint32_t thr_bit_width(uint64_t v) {
    uint32_t w = 0;
    while (v) { w++; v >>= 1; }
    return w;
}

// docs per window with n_planes planes: the union's window (2^window_log2, 11 .. 30), at most 2^30 / n_planes rounded down to a
// power of two
II2_HD uint64_t thr_window_docs(uint32_t n_planes, int64_t window_log2) {
    const int64_t lg = window_log2 < 11 ? 11 : window_log2 > 30 ? 30 : window_log2;
    uint64_t w = THR_PLANE_DOCS;
    while (w * (n_planes ? n_planes : 1u) > THR_PLANE_DOCS) w >>= 1;
    return (1ull << lg) < w ? (1ull << lg) : w;
}

// add the docs of word g to their counters (ripple carry); a counter that would pass 2^B - 1 stays there
template <uint32_t B> II2_HD void thr_add_word(uint32_t (&pl)[B], uint32_t g) {
    uint32_t carry = g;
#pragma unroll
    for (uint32_t b = 0; b < B; b++) {
        const uint32_t t = pl[b] & carry;
        pl[b] ^= carry;
        carry = t;
    }
#pragma unroll
    for (uint32_t b = 0; b < B; b++) pl[b] |= carry;        // the carry left the top plane: all ones
}

// the docs whose counter is >= m (m < 2^B), compared from the most significant plane down
template <uint32_t B> II2_HD uint32_t thr_ge_word(const uint32_t (&pl)[B], uint32_t m) {
    uint32_t gt = 0u, eq = 0xFFFFFFFFu;
#pragma unroll
    for (uint32_t k = 0; k < B; k++) {
        const uint32_t b = B - 1u - k;
        const uint32_t mb = ((m >> b) & 1u) ? 0xFFFFFFFFu : 0u;
        gt |= eq & pl[b] & ~mb;
        eq &= ~(pl[b] ^ mb);
    }
    return gt | eq;
}

}  // namespace ii2
