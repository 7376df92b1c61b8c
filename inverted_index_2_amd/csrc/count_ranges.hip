// count_ranges.hip — hits per posting list against a doc set (ii2_count_ranges: facet counts, document frequencies).  The lists
// come as the ranges of ii2_union_ranges; out_first[r] is the counter of range r's first list.  Per window of at most 2^30 docs of
// the span that the set and the lists share:
//   1. k_cr_mark: one wave per 64 consecutive ids of the set - lanes whose ids share a bitmap word are adjacent, a segmented OR
//      leaves the word's bits in the run's last lane, which takes the tombstones off them and issues the only atomicOr for that
//      word (and, the same way, for the word's bit in the summary: one bit per 64 words = 2048 docs);
//   2. k_cr_count: the walk of cr_walk.h, bounded and with the summary skip - against a small set most blocks of a long list have
//      no set doc anywhere near them and are never read.  Every id of the others tests its bit and the hits stay in a register
//      until the owning list changes or the run ends: one wave sum and one atomicAdd per (wave, list), which keeps a list that owns
//      many blocks off the ~90 atomics / us one address takes;
//   3. k_ir_clear (intersect_ranges.hip): the words and summary words that were set are zeroed again.  The scratch is all-zero
//      between calls.
// The second instantiation of k_cr_count serves the set "every doc" with tombstones: it tests each id against the tombstones
// instead and needs no mark, no bounds, no window and no scratch.
// No kernel waits for another workgroup.
#include <hip/hip_runtime.h>

#include "cr_walk.h"
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
    const CrWave w = cr_wave(p);
    if (w.g0 == w.g1) return;                                             // (wave-uniform; no workgroup barrier below)
    uint32_t cur = 0xFFFFFFFFu;                                           // the counter the hits in `acc` belong to (none yet)
    uint32_t acc = 0, n_dec = 0;
    auto flush = [&]() {
        if (cur != 0xFFFFFFFFu) {
            const uint32_t s = wave_sum(acc);
            if (w.l == 0 && s) atomicAdd(&p.counts[cur], s);
        }
        acc = 0;
    };
    // "every doc": no bound test (the host sets no doc_lo / doc_hi), no summary
    cr_walk<!EVERY_DOC, !EVERY_DOC>(p, w, [&](const UmRange &R, uint32_t ofirst, uint32_t j, const ii2_skip &e0, const ii2_skip &e1, uint32_t) {
        const uint32_t idx = ofirst + (j - R.l0);
        if (idx != cur) {
            flush();
            cur = idx;
        }
        n_dec++;
        cr_block_ids(R, e0, e1, [&](uint32_t id, bool v) { acc += cr_hit<EVERY_DOC>(p, id, v); });
    });
    flush();
    if (w.l == 0 && n_dec) atomicAdd(&p.decoded[blockIdx.x % CR_DECODED_SLOTS], n_dec);
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
    const dim3 grid = cr_grid(p);
    if (ev0) (void)hipEventRecord(ev0, s);
    if (every_doc) hipLaunchKernelGGL(k_cr_count<true>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_cr_count<false>, grid, dim3(256), 0, s, p);
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

}  // namespace ii2
