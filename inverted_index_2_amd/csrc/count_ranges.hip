// count_ranges.hip — hits per posting list against a doc set (ii2_count_ranges: facet counts, document frequencies).  The lists
// come as the ranges of ii2_union_ranges and are walked the same way, by DV1 block: range r owns the blocks [b0, b1) of its
// segment, the query's blocks are the ranges' blocks back to back (pre[r] = blocks of the ranges before r), and out_first[r] is
// the counter of the range's first list.  Per window of at most 2^30 docs of the span that the set and the lists share:
//   1. k_cr_mark: one wave per 64 consecutive ids of the set - lanes whose ids share a bitmap word are adjacent, a segmented OR
//      leaves the word's bits in the run's last lane, which takes the tombstones off them and issues the only atomicOr for that
//      word (and, the same way, for the word's bit in the summary: one bit per 64 words = 2048 docs);
//   2. k_cr_count: one wave per run of query blocks.  A block whose doc bounds miss the window's docs is skipped unread, and so
//      is one whose bounds cover at most 64 summary bits none of which is set: against a small set most blocks of a long list
//      have no set doc anywhere near them.  The others are decoded in registers, four ids per lane, every id tests its bit and
//      the hits stay in a register until the owning list changes or the run ends: one wave sum and one atomicAdd per (wave,
//      list), which keeps a list that owns many blocks off the ~90 atomics / us one address takes;
//   3. k_ir_clear (intersect_ranges.hip): the words and summary words that were set are zeroed again.  The scratch is all-zero
//      between calls.
// The second instantiation of k_cr_count serves the set "every doc" with tombstones: it tests each id against the tombstones
// instead and needs no mark, no window and no scratch.
// No kernel waits for another workgroup.
#include <hip/hip_runtime.h>

#include "dv1_device.h"
#include "internal.h"
#include "um_device.h"

namespace ii2 {

// the set's first and last id, side by side for one copy to the host
__global__ void k_cr_edges(CountParams p) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        p.edges[0] = p.set[0];
        p.edges[1] = p.set[p.n_set - 1u];
    }
}

__global__ __launch_bounds__(256) void k_cr_mark(CountParams p) {
    const uint32_t l = threadIdx.x & 63u;
    const uint64_t i0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u;
    if (i0 >= p.n_set) return;                                            // (wave-uniform; no workgroup barrier below)
    const uint64_t i = i0 + l;
    const uint32_t id = i < p.n_set ? p.set[i] : 0u;
    const uint32_t rel = id - p.win_lo;
    // bounded against the window before it indexes the bitmap (a set that is not ascending costs atomics, never an access outside);
    // ids outside the docs that can hit are not marked at all
    const bool v = i < p.n_set && id >= p.win_lo && rel < p.win_docs && id >= p.doc_lo && id <= p.doc_hi;
    if (__ballot(v) == 0ull) return;
    const uint32_t key = v ? rel >> 5 : 0xFFFFFFFFu;
    uint32_t bits = seg_or(key, v ? 1u << (rel & 31u) : 0u);
    const uint32_t next = (uint32_t)__shfl_down((int)key, 1, 64);
    const bool last = v && (l == 63u || next != key);                     // the lane that holds the word's bits
    if (last && p.tomb) {                                                 // removed docs never reach the bitmap
        const uint32_t tw = p.win_lo / 32u + key;
        if (tw < p.tomb_nwords) bits &= ~p.tomb[tw];
    }
    const bool live = last && bits != 0u;
    const uint32_t skey = v ? key >> 11 : 0xFFFFFFFFu;                    // summary word of the bitmap word
    const uint32_t sbits = seg_or(skey, live ? 1u << ((key >> 6) & 31u) : 0u);
    const uint32_t snext = (uint32_t)__shfl_down((int)skey, 1, 64);
    if (live) atomicOr(&p.bitmap[key], bits);
    if (v && (l == 63u || snext != skey) && sbits) atomicOr(&p.summary[skey], sbits);
}

template <bool EVERY_DOC>
__global__ __launch_bounds__(256) void k_cr_count(CountParams p) {
    const uint32_t l = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t g0 = ((uint64_t)blockIdx.x * 4u + wv) * p.per_wave;
    if (g0 >= p.n_blocks) return;                                         // (wave-uniform; no workgroup barrier below)
    const uint32_t g1 = (uint32_t)(g0 + p.per_wave < p.n_blocks ? g0 + p.per_wave : p.n_blocks);
    uint32_t r = um_range_of(p.pre, p.n_ranges, (uint32_t)g0);
    UmRange R = p.ranges[r];
    uint32_t rbeg = p.pre[r], rend = p.pre[r + 1u], ofirst = p.out_first[r];
    uint32_t cur = 0xFFFFFFFFu;                                           // the counter the hits in `acc` belong to (none yet)
    uint32_t acc = 0, n_dec = 0;
    auto flush = [&]() {
        if (cur != 0xFFFFFFFFu) {
            const uint32_t s = wave_sum(acc);
            if (l == 0 && s) atomicAdd(&p.counts[cur], s);
        }
        acc = 0;
    };
    auto test = [&](uint32_t id, bool v) -> uint32_t {
        if (EVERY_DOC) return v && !tomb_has(p.tomb, p.tomb_nwords, id) ? 1u : 0u;
        const uint32_t rel = id - p.win_lo;
        const bool in = v && id >= p.win_lo && rel < p.win_docs;
        const uint32_t w = in ? p.bitmap[rel >> 5] : 0u;
        return (w >> (rel & 31u)) & 1u;
    };
    for (uint32_t g = (uint32_t)g0; g < g1; g++) {
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
        if (!EVERY_DOC) {
            // a bound of the block's last doc: the next block's first doc, or the list's last doc
            const uint32_t up = (b + 1u < R.b1 && R.blk_list[b + 1u] == j) ? e1.first_doc : R.last_doc[j];
            if (e0.first_doc > p.doc_hi || up < p.doc_lo) continue;
            if (p.summary_skip) {
                const uint32_t ca = ((e0.first_doc > p.doc_lo ? e0.first_doc : p.doc_lo) - p.win_lo) >> 11;
                const uint32_t cc = ((up < p.doc_hi ? up : p.doc_hi) - p.win_lo) >> 11;      // (<= (doc_hi - win_lo) >> 11 < 32 n_sum)
                if (cc - ca < 64u) {                                      // one summary bit per lane
                    const uint32_t ch = ca + l;
                    const bool hit = ch <= cc && ((p.summary[ch >> 5] >> (ch & 31u)) & 1u) != 0u;
                    if (__ballot(hit) == 0ull) continue;
                }
            }
        }
        const uint32_t idx = ofirst + (j - R.l0);
        if (idx != cur) {
            flush();
            cur = idx;
        }
        n_dec++;
        decode_block_wave4(GlobalBytes{R.payload}, e0.byte_off, e1.byte_off, e0.first_doc,
                           [&](uint32_t ix, uint32_t id0, uint32_t id1, uint32_t id2, uint32_t id3, uint32_t mask) {
                               const uint32_t i1 = ix + (mask & 1u), i2 = i1 + ((mask >> 1) & 1u), i3 = i2 + ((mask >> 2) & 1u);
                               // four independent tests (gathers): the order does not matter, nothing is staged
                               const uint32_t h0 = test(id0, (mask & 1u) && ix < II2_DV1_BLOCK);
                               const uint32_t h1 = test(id1, (mask & 2u) && i1 < II2_DV1_BLOCK);
                               const uint32_t h2 = test(id2, (mask & 4u) && i2 < II2_DV1_BLOCK);
                               const uint32_t h3 = test(id3, (mask & 8u) && i3 < II2_DV1_BLOCK);
                               acc += (h0 + h1) + (h2 + h3);
                           });
    }
    flush();
    if (l == 0 && n_dec) atomicAdd(&p.decoded[blockIdx.x % CR_DECODED_SLOTS], n_dec);
}

hipError_t launch_cr_edges(const CountParams &p, hipStream_t s) {
    hipLaunchKernelGGL(k_cr_edges, dim3(1), dim3(64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_cr_mark(const CountParams &p, hipStream_t s) {
    const uint64_t waves = (p.n_set + 63u) / 64u;
    hipLaunchKernelGGL(k_cr_mark, dim3((unsigned)((waves + 3u) / 4u)), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_cr_count(const CountParams &p, bool every_doc, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    const uint64_t waves = (p.n_blocks + (uint64_t)p.per_wave - 1u) / p.per_wave;
    const dim3 grid((unsigned)((waves + 3u) / 4u));
    if (ev0) (void)hipEventRecord(ev0, s);
    if (every_doc) hipLaunchKernelGGL(k_cr_count<true>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_cr_count<false>, grid, dim3(256), 0, s, p);
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

}  // namespace ii2
