// cr_walk.h — the walk of a wave over its run of query blocks, as the counting kernels share it (histogram.hip; k_cr_count and
// k_ex_match still carry their own copies: DESIGN §7).  The query's blocks are the ranges' blocks back to back (CountParams: pre[r]
// = blocks of the ranges before r); the walk steps from range to range, drops the blocks that no list of the range owns, and hands
// every other block to the sink - unless, with BOUNDED, the block's doc bounds miss [doc_lo, doc_hi] or, with SUMMARY, they
// cover at most 64 chunks of the marked bitmap's summary none of which is set.  Such a block is never read.
#pragma once
#include <hip/hip_runtime.h>

#include "internal.h"
#include "um_device.h"

namespace ii2 {

// sink(R, ofirst, j, e0, e1, up): block of list j of range R, whose first list's counter is ofirst; skip entries e0 (its own) and
// e1 (the next); up = a bound of its last doc - the next block's first doc inside a list, the list's last doc at its end.
// Everything the sink receives is wave-uniform.
template <bool BOUNDED, bool SUMMARY, class Sink>
__device__ __forceinline__ void cr_walk(const CountParams &p, uint32_t g0, uint32_t g1, uint32_t l, Sink sink) {
    static_assert(BOUNDED || !SUMMARY, "the summary test clips the block's bounds to [doc_lo, doc_hi]: they must overlap");
    uint32_t r = um_range_of(p.pre, p.n_ranges, g0);
    UmRange R = p.ranges[r];
    uint32_t rbeg = p.pre[r], rend = p.pre[r + 1u], ofirst = p.out_first[r];
    for (uint32_t g = g0; g < g1; g++) {
        while (g >= rend) {
            r++;
            R = p.ranges[r];
            rbeg = rend;
            rend = p.pre[r + 1u];
            ofirst = p.out_first[r];
        }
        const uint32_t b = R.b0 + (g - rbeg);
        const uint32_t j = R.blk_list[b];
        if (j < R.l0 || j >= R.l1) continue;                              // no list of the range owns it: no counter
        const ii2_skip e0 = R.skip[b], e1 = R.skip[b + 1u];
        const uint32_t up = (b + 1u < R.b1 && R.blk_list[b + 1u] == j) ? e1.first_doc : R.last_doc[j];
        if (BOUNDED && (e0.first_doc > p.doc_hi || up < p.doc_lo)) continue;
        if (SUMMARY && p.summary_skip) {
            const uint32_t ca = ((e0.first_doc > p.doc_lo ? e0.first_doc : p.doc_lo) - p.win_lo) >> 11;
            const uint32_t cc = ((up < p.doc_hi ? up : p.doc_hi) - p.win_lo) >> 11;          // (<= (doc_hi - win_lo) >> 11 < 32 n_sum)
            if (cc - ca < 64u) {                                          // one summary bit per lane
                const uint32_t ch = ca + l;
                const bool hit = ch <= cc && ((p.summary[ch >> 5] >> (ch & 31u)) & 1u) != 0u;
                if (__ballot(hit) == 0ull) continue;
            }
        }
        sink(R, ofirst, j, e0, e1, up);
    }
}

}  // namespace ii2
