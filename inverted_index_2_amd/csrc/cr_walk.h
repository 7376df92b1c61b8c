// cr_walk.h — the walk of a wave over its run of query blocks, as every reader of a marked doc set shares it (k_cr_count,
// k_ex_match, k_hs_count), with the pieces around it: the wave's run, the launch grid, the test of an id and the ids of a block.
// The query's blocks are the ranges' blocks back to back (CountParams: pre[r] = blocks of the ranges before r); a workgroup is
// four waves, a wave takes per_wave consecutive query blocks.  The walk steps from range to range, drops the blocks that no list
// of the range owns, and hands every other block to the sink - unless, with BOUNDED, the block's doc bounds miss [doc_lo, doc_hi]
// or, with SUMMARY, they cover at most 64 chunks of the marked bitmap's summary none of which is set.  Such a block is never read.
#pragma once
#include <hip/hip_runtime.h>

#include "dv1_device.h"
#include "internal.h"
#include "um_device.h"

namespace ii2 {

// the grid of a walk over p's blocks
inline dim3 cr_grid(const CountParams &p) {
    const uint64_t waves = (p.n_blocks + (uint64_t)p.per_wave - 1u) / p.per_wave;
    return dim3((unsigned)((waves + 3u) / 4u));
}

// a wave's lane, its number in the workgroup (a scalar) and its run of query blocks [g0, g1); g0 == g1: no work (wave-uniform)
struct CrWave {
    uint32_t l, wv, g0, g1;
};
__device__ __forceinline__ CrWave cr_wave(const CountParams &p) {
    const uint32_t l = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t g0 = ((uint64_t)blockIdx.x * 4u + wv) * p.per_wave;
    if (g0 >= p.n_blocks) return CrWave{l, wv, 0u, 0u};
    return CrWave{l, wv, (uint32_t)g0, (uint32_t)(g0 + p.per_wave < p.n_blocks ? g0 + p.per_wave : p.n_blocks)};
}

// 1 when the id is valid and a hit: its bit of the marked bitmap, inside the window - or, for the set "every doc", not removed
template <bool EVERY_DOC>
__device__ __forceinline__ uint32_t cr_hit(const CountParams &p, uint32_t id, bool v) {
    if (EVERY_DOC) return v && !tomb_has(p.tomb, p.tomb_nwords, id) ? 1u : 0u;
    const uint32_t rel = id - p.win_lo;
    const bool in = v && id >= p.win_lo && rel < p.win_docs;
    const uint32_t w = in ? p.bitmap[rel >> 5] : 0u;
    return (w >> (rel & 31u)) & 1u;
}

// The ids of the block between the skip entries e0 and e1 of R, decoded in registers, four per lane and step: f(id, valid) for
// each.  Nothing is staged and the four calls of a step do not depend on one another.
template <class F>
__device__ __forceinline__ void cr_block_ids(const UmRange &R, const ii2_skip &e0, const ii2_skip &e1, F f) {
    decode_block_wave4(GlobalBytes{R.payload}, e0.byte_off, e1.byte_off, e0.first_doc,
                       [&](uint32_t ix, uint32_t id0, uint32_t id1, uint32_t id2, uint32_t id3, uint32_t mask) {
                           const uint32_t i1 = ix + (mask & 1u), i2 = i1 + ((mask >> 1) & 1u), i3 = i2 + ((mask >> 2) & 1u);
                           f(id0, (mask & 1u) && ix < II2_DV1_BLOCK);
                           f(id1, (mask & 2u) && i1 < II2_DV1_BLOCK);
                           f(id2, (mask & 4u) && i2 < II2_DV1_BLOCK);
                           f(id3, (mask & 8u) && i3 < II2_DV1_BLOCK);
                       });
}

// sink(R, ofirst, j, e0, e1, up): block of list j of range R, whose first list's counter is ofirst; skip entries e0 (its own) and
// e1 (the next); up = a bound of its last doc - the next block's first doc inside a list, the list's last doc at its end.
// Everything the sink receives is wave-uniform.  Without BOUNDED nothing reads doc_lo / doc_hi (the "every doc" count leaves them
// unset), and a sink that ignores `up` costs no load for it.
template <bool BOUNDED, bool SUMMARY, class Sink>
__device__ __forceinline__ void cr_walk(const CountParams &p, const CrWave &w, Sink sink) {
    static_assert(BOUNDED || !SUMMARY, "the summary test clips the block's bounds to [doc_lo, doc_hi]: they must overlap");
    uint32_t r = um_range_of(p.pre, p.n_ranges, w.g0);
    UmRange R = p.ranges[r];
    uint32_t rbeg = p.pre[r], rend = p.pre[r + 1u], ofirst = p.out_first[r];
    for (uint32_t g = w.g0; g < w.g1; g++) {
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
                const uint32_t ch = ca + w.l;
                const bool hit = ch <= cc && ((p.summary[ch >> 5] >> (ch & 31u)) & 1u) != 0u;
                if (__ballot(hit) == 0ull) continue;
            }
        }
        sink(R, ofirst, j, e0, e1, up);
    }
}

}  // namespace ii2
