// explain_ranges.hip — which groups each doc of an id array lies in (ii2_explain_ranges: highlighting, "matched queries", the
// tiers of a fuzzy hit).  The transpose of count_ranges.hip: the ids are marked into the per-context doc bitmap by k_cr_mark and
// the groups' blocks are walked once, by the walk k_cr_count<false> runs (cr_walk.h, out_first[r] = the group of range r); a hit
// does not add 1 to its list's counter, it ORs bit g of its group into the row of its doc.  The ids come in any order (a ranked
// page is score-descending), so a hit finds its row through a table:
//   1. k_ex_prepare: one thread per row inserts (id << 32 | row) into an open-addressing table of 64-bit entries, linear probing
//      from ex_slot(id), wrapping at the end; an empty slot (all-ones) is claimed by a compare-and-swap, a slot that holds the same
//      id takes the smaller entry by atomicMin: a repeated id keeps its FIRST row, whatever order the threads arrive in.  The table
//      has at least twice as many slots as rows, so every probe ends.  The same kernel reduces the ids' minimum and maximum
//      (k_cr_edges would read set[0] and set[n - 1] of an ascending set);
//   2. k_cr_mark (count_ranges.hip), per window;
//   3. k_ex_match, per window: the walk of cr_walk.h, bounded and with the summary skip; every decoded id whose bit is set probes
//      the table until it meets its id or an empty slot and issues one 64-bit atomicOr into its row.  The bits that were clear
//      before (the call's n_hits) stay in a register: one wave sum and one atomicAdd per wave, spread over CR_DECODED_SLOTS words
//      as the decoded blocks are;
//   4. k_ir_clear (intersect_ranges.hip), per window.
// No kernel waits for another workgroup.
#include <hip/hip_runtime.h>

#include "cr_walk.h"
#include "dv1_device.h"
#include "internal.h"
#include "um_device.h"

namespace ii2 {

__device__ __forceinline__ uint32_t wave_min(uint32_t x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t y = (uint32_t)__shfl_xor((int)x, d, 64);
        x = y < x ? y : x;
    }
    return x;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t y = (uint32_t)__shfl_xor((int)x, d, 64);
        x = y > x ? y : x;
    }
    return x;
}

__global__ __launch_bounds__(256) void k_ex_prepare(ExplainParams p) {
    const uint64_t row = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool v = row < p.c.n_set;
    const uint32_t id = v ? p.c.set[row] : 0u;
    if (v) {
        const unsigned long long e = ((unsigned long long)id << 32) | row;      // (never EX_EMPTY: row < 2^32 - 1)
        const uint32_t mask = (1u << p.log2_slots) - 1u;
        uint32_t s = ex_slot(id, p.log2_slots);
        for (uint32_t probe = 0; probe <= mask; probe++, s = (s + 1u) & mask) {  // (ends at an empty slot: the table is at most half full)
            const unsigned long long old = atomicCAS(&p.table[s], (unsigned long long)EX_EMPTY, e);
            if (old == EX_EMPTY) break;
            if ((uint32_t)(old >> 32) == id) {                                   // the id again: its first row stays
                atomicMin(&p.table[s], e);
                break;
            }
        }
    }
    // the ids' span: one atomic per wave and bound, and none where the word already says as much
    const uint32_t mn = wave_min(v ? id : 0xFFFFFFFFu), mx = wave_max(v ? id : 0u);
    if ((threadIdx.x & 63u) == 0u && v) {
        if (mn < __hip_atomic_load(&p.span[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&p.span[0], mn);
        if (mx > __hip_atomic_load(&p.span[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&p.span[1], mx);
    }
}

// the row of id, 0xFFFFFFFF when the table does not hold it
__device__ __forceinline__ uint32_t ex_row_of(const ExplainParams &p, uint32_t id) {
    const uint32_t mask = (1u << p.log2_slots) - 1u;
    uint32_t s = ex_slot(id, p.log2_slots);
    for (uint32_t probe = 0; probe <= mask; probe++, s = (s + 1u) & mask) {
        const unsigned long long e = p.table[s];
        if (e == EX_EMPTY) break;
        if ((uint32_t)(e >> 32) == id) return (uint32_t)e;
    }
    return 0xFFFFFFFFu;
}

__global__ __launch_bounds__(256) void k_ex_match(ExplainParams q) {
    const CountParams &p = q.c;
    const CrWave w = cr_wave(p);
    if (w.g0 == w.g1) return;                                             // (wave-uniform; no workgroup barrier below)
    uint32_t fresh = 0, n_dec = 0;                                        // mask bits this lane set first; blocks decoded
    cr_walk<true, true>(p, w, [&](const UmRange &R, uint32_t grp, uint32_t, const ii2_skip &e0, const ii2_skip &e1, uint32_t) {
        n_dec++;
        // a hit: the doc's row gets the group's bit (a repeated id's later rows are not in the table and stay 0)
        cr_block_ids(R, e0, e1, [&](uint32_t id, bool v) {
            if (!cr_hit<false>(p, id, v)) return;
            const uint32_t row = ex_row_of(q, id);
            if (row >= p.n_set) return;                                   // (not among the ids: cannot be, its bit was marked)
            const unsigned long long bit = 1ull << (grp & 63u);
            const unsigned long long old = atomicOr(&q.masks[(uint64_t)row * q.n_words + (grp >> 6)], bit);
            fresh += (old & bit) ? 0u : 1u;
        });
    });
    const uint32_t s = wave_sum(fresh);
    if (w.l == 0 && s) atomicAdd(&q.hits[blockIdx.x % CR_DECODED_SLOTS], (unsigned long long)s);
    if (w.l == 0 && n_dec) atomicAdd(&p.decoded[blockIdx.x % CR_DECODED_SLOTS], n_dec);
}

hipError_t launch_ex_prepare(const ExplainParams &p, hipStream_t s) {
    hipLaunchKernelGGL(k_ex_prepare, dim3((unsigned)((p.c.n_set + 255u) / 256u)), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_ex_match(const ExplainParams &p, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (ev0) (void)hipEventRecord(ev0, s);
    hipLaunchKernelGGL(k_ex_match, cr_grid(p.c), dim3(256), 0, s, p);
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

}  // namespace ii2
