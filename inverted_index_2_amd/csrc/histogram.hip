// histogram.hip — hits per (posting list, value bucket) against a doc set (ii2_histogram_ranges: date histograms, terms over
// time) and the bucket counts of a doc set itself (ii2_histogram_ids).  The value axis is n_buckets buckets of ids, first[b] the
// first id of bucket b and `last` the last id of the last one (hist_device.h); ids outside it are counted nowhere.
//   k_hs_count is the walk of k_cr_count (cr_walk.h) with a two-dimensional counter index.  The set is marked by k_cr_mark and
//   cleared by k_ir_clear exactly as for ii2_count_ranges; the host has clipped doc_lo / doc_hi to the axis, so blocks outside it
//   are never read.  A block's doc bounds say, before it is read, which buckets it can meet (hist_block), and that picks its sink:
//     WHOLE  one bucket: the hits stay in a register until the (list, bucket) pair changes or the run ends - one wave sum and one
//            atomicAdd per pair, as k_cr_count has per list;
//     SPLIT  2 .. 64 buckets: each hit bisects first[b_lo .. b_hi] and adds 1 to its wave's strip of 64 counters in LDS; after the
//            block lane i moves strip[i] to the global counter - at most one global atomic per touched bucket;
//     WIDE   more: one global atomicAdd per hit - the buckets are narrower than 1/64 of the block's span, the addresses spread.
//   The second instantiation serves the set "every doc": ids are tested against the tombstones, no mark, no window, no scratch.
//   The edges are read from global memory: the bucket search of a block's bounds is wave-uniform (scalar addresses), the per-id
//   search of a SPLIT block touches at most 64 consecutive edges (256 bytes) - see DESIGN 4.9d.
//   k_hs_ids_edges: one thread per bucket bisects the ascending set for the bucket's two edges; no atomics.
//   k_hs_ids_tomb: one wave per 64 consecutive ids - each lane finds its bucket and tests the tombstones, a segmented sum over the
//   runs of equal buckets leaves one atomicAdd per (wave, bucket) run.
// No kernel waits for another workgroup.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "cr_walk.h"
#include "dv1_device.h"
#include "hist_device.h"
#include "internal.h"
#include "um_device.h"

namespace ii2 {

// Orders the LDS traffic of ONE wave: the lanes' adds into the wave's strip before the flush reads of other lanes of the same
// wave, and the flush's clearing stores before the next block's adds.  A wave's LDS operations are issued and executed in program
// order, so at wavefront scope the fence costs no wait; it keeps the compiler from moving the accesses across it.
__device__ __forceinline__ void strip_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <bool EVERY_DOC>
__global__ __launch_bounds__(256) void k_hs_count(HistParams hp) {
    __shared__ uint32_t strips[4][HIST_STRIP];
    const CountParams &p = hp.c;
    const CrWave w = cr_wave(p);
    if (w.g0 == w.g1) return;                                             // (wave-uniform; no workgroup barrier below)
    const uint32_t l = w.l, wv = w.wv;
    strips[wv][l] = 0u;                                                   // this wave's own strip: all-zero whenever it leaves a block
    strip_fence();
    const uint32_t nb = hp.n_buckets, first0 = hp.first0, last = hp.last;
    uint32_t cur = 0xFFFFFFFFu;                                           // the (list, bucket) counter the hits in `acc` belong to (none yet)
    uint32_t acc = 0, n_whole = 0, n_split = 0, n_wide = 0;
    auto flush = [&]() {
        if (cur != 0xFFFFFFFFu) {
            const uint32_t s = wave_sum(acc);
            if (l == 0 && s) atomicAdd(&p.counts[cur], s);
        }
        acc = 0;
    };
    cr_walk<true, !EVERY_DOC>(p, w, [&](const UmRange &R, uint32_t ofirst, uint32_t j, const ii2_skip &e0, const ii2_skip &e1, uint32_t up) {
        // the walk's values are wave-uniform but come out of vector loads: as scalars, the bucket search of the bounds below runs
        // on the scalar unit
        const uint32_t fd = (uint32_t)__builtin_amdgcn_readfirstlane((int)e0.first_doc), ub = (uint32_t)__builtin_amdgcn_readfirstlane((int)up);
        uint32_t b_lo = 0, b_hi = 0;
        int kind = hist_block(hp.first, nb, first0, last, fd, ub, &b_lo, &b_hi);
        if (kind == HIST_SKIP) return;
        if (kind == HIST_WHOLE && !hp.whole) kind = HIST_SPLIT;
        // the list's first counter (< lists named x n_buckets <= II2_HIST_MAX_CELLS)
        const uint32_t row = (uint32_t)__builtin_amdgcn_readfirstlane((int)((ofirst + (j - R.l0)) * nb));
        if (kind == HIST_WHOLE) {
            if (row + b_lo != cur) {
                flush();
                cur = row + b_lo;
            }
            n_whole++;
            cr_block_ids(R, e0, e1, [&](uint32_t id, bool v) { acc += cr_hit<EVERY_DOC>(p, id, v); });
            return;
        }
        flush();
        cur = 0xFFFFFFFFu;
        const bool split = kind == HIST_SPLIT;                            // (b_hi - b_lo < HIST_STRIP)
        if (split) n_split++;
        else n_wide++;
        // a hit inside the axis finds its bucket among b_lo .. b_hi (hist_find stays inside them whatever the id) and adds 1 to the
        // wave's strip in LDS (SPLIT) or to the global counter (WIDE): two instances, so that neither atomic goes through a
        // generic pointer
        auto searched = [&](auto to_strip) {
            cr_block_ids(R, e0, e1, [&](uint32_t id, bool v) {
                if (!cr_hit<EVERY_DOC>(p, id, v) || id < first0 || id > last) return;
                const uint32_t b = hist_find(hp.first, b_lo, b_hi, id);
                if (decltype(to_strip)::value) atomicAdd(&strips[wv][b - b_lo], 1u);
                else atomicAdd(&p.counts[row + b], 1u);
            });
        };
        if (split) searched(std::true_type{});
        else searched(std::false_type{});
        if (split) {
            strip_fence();                                                // every lane's adds before any lane's read below
            const uint32_t v = strips[wv][l];
            if (v) {                                                      // (only lanes l <= b_hi - b_lo can hold a count)
                strips[wv][l] = 0u;
                atomicAdd(&p.counts[row + b_lo + l], v);
            }
            strip_fence();                                                // the clearing stores before the next block's adds
        }
    });
    flush();
    const uint32_t slot = blockIdx.x % CR_DECODED_SLOTS;
    if (l == 0 && n_whole) atomicAdd(&p.decoded[slot], n_whole);
    if (l == 0 && n_split) atomicAdd(&p.decoded[CR_DECODED_SLOTS + slot], n_split);
    if (l == 0 && n_wide) atomicAdd(&p.decoded[2u * CR_DECODED_SLOTS + slot], n_wide);
}

// first i in [0, n) with set[i] >= v (UPPER: > v)
template <bool UPPER>
__device__ __forceinline__ uint64_t set_bound(const uint32_t *set, uint64_t n, uint32_t v) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const uint32_t x = set[mid];
        if (UPPER ? x <= v : x < v) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_hs_ids_edges(HistParams hp) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= hp.n_buckets) return;
    const uint64_t lo = set_bound<false>(hp.c.set, hp.c.n_set, hp.first[b]);
    const uint64_t hi = b + 1u < hp.n_buckets ? set_bound<false>(hp.c.set, hp.c.n_set, hp.first[b + 1u]) : set_bound<true>(hp.c.set, hp.c.n_set, hp.last);
    hp.c.counts[b] = (uint32_t)(hi - lo);                                 // (a set that is not ascending: any value)
}

__global__ __launch_bounds__(256) void k_hs_ids_tomb(HistParams hp) {
    const CountParams &p = hp.c;
    const uint32_t l = threadIdx.x & 63u;
    const uint64_t i0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u;
    if (i0 >= p.n_set) return;                                            // (wave-uniform; no workgroup barrier below)
    const uint64_t i = i0 + l;
    const uint32_t id = i < p.n_set ? p.set[i] : 0u;
    const int64_t b = i < p.n_set ? hist_bucket(hp.first, hp.n_buckets, hp.last, id) : -1;
    const uint32_t key = b < 0 ? 0xFFFFFFFFu : (uint32_t)b;               // (< n_buckets)
    const uint32_t n = seg_add(key, b >= 0 && !tomb_has(p.tomb, p.tomb_nwords, id) ? 1u : 0u);
    const uint32_t next = (uint32_t)__shfl_down((int)key, 1, 64);
    if (b >= 0 && (l == 63u || next != key) && n) atomicAdd(&p.counts[key], n);
}

hipError_t launch_hs_count(const HistParams &p, bool every_doc, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    const dim3 grid = cr_grid(p.c);
    if (ev0) (void)hipEventRecord(ev0, s);
    if (every_doc) hipLaunchKernelGGL(k_hs_count<true>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_hs_count<false>, grid, dim3(256), 0, s, p);
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

hipError_t launch_hs_ids(const HistParams &p, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (ev0) (void)hipEventRecord(ev0, s);
    if (p.c.tomb) {
        const uint64_t waves = (p.c.n_set + 63u) / 64u;
        hipLaunchKernelGGL(k_hs_ids_tomb, dim3((unsigned)((waves + 3u) / 4u)), dim3(256), 0, s, p);
    } else {
        hipLaunchKernelGGL(k_hs_ids_edges, dim3((p.n_buckets + 255u) / 256u), dim3(256), 0, s, p);
    }
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

}  // namespace ii2
