// setop_small.hip — AND / OR of posting lists that together hold at most 8192 postings (in at most 128 DV1 blocks): one launch.
// The general paths cut a query into tiles over four (intersection) or some forty (union through the merge passes)
// launches; below a few thousand postings that is all launch and dependency latency — 14-20 us per AND, 110-150 us
// per OR — and short lists are what most terms of a real dictionary have (PrefixSearch, inverted_index.go:274-292,
// unions the lists of every matching term).
//
// The decode, rank and block-scan stages are those of small_set_device.h; particular to this kernel:
//   - the lists come in the by-value parameter block;
//   - one workgroup stores every id at its rank in LDS; when the bisections are too many for one CU (many lists) the ids
//     are shared out over up to 32 workgroups, which all decode every block, store into a small global array, and the
//     workgroup that finishes last (a device-wide ticket) goes on;
//   - over the ascending ids the first id of every run of equal ids survives — for an AND only when the run is n_lists
//     long (each list holds an id once, so id[i + n_lists - 1] == id[i] says it all) — unless the tombstone bitmap has it;
//   - what fits out_cap is written, the count is the whole result's.
#include <hip/hip_runtime.h>

#include "internal.h"
#include "small_set_device.h"

namespace ii2 {

constexpr uint32_t SS_THREADS = 1024;
constexpr uint32_t SS_WAVES = SS_THREADS / 64u;

__global__ __launch_bounds__(SS_THREADS) void k_setop_small(SmallSetParams p) {
    __shared__ uint32_t raw[SMALL_SET_POSTINGS];                    // list j decoded at raw[lpre[j] ...], ascending
    __shared__ uint32_t lcnt[MAX_LISTS], lpre[MAX_LISTS + 1];       // postings of every list (the host knows them), their prefix
    __shared__ uint32_t lbase[MAX_LISTS + 1];                       // first block of every list in the concatenated block list
    __shared__ uint32_t wsum[SS_WAVES];
    __shared__ uint32_t last_s;
    __shared__ uint8_t blist[SMALL_SET_BLOCKS];                     // the list every block belongs to
    const uint32_t tid = threadIdx.x;
    if (tid <= p.n_lists) {
        lpre[tid] = p.lpre[tid];
        lbase[tid] = p.blk_base[tid];
        if (tid < p.n_lists) {
            lcnt[tid] = p.lpre[tid + 1u] - p.lpre[tid];
            for (uint32_t b = p.blk_base[tid]; b < p.blk_base[tid + 1u]; b++) blist[b] = (uint8_t)tid;
        }
    }
    __syncthreads();
    // 1. decode (redundant across workgroups, but cheaper than a second launch)
    ss_decode<SS_WAVES, SMALL_SET_BLOCKS / SS_WAVES>(p.n_blocks, blist, lbase, lpre, raw, [&](uint32_t j) { return p.lists[j].skip; },
                                                     [&](uint32_t j) { return p.lists[j].payload; });
    __syncthreads();
    const uint32_t n_total = lpre[p.n_lists];
    // 2. ranks: this workgroup's share of the ids, at most eight per thread
    const uint32_t per_wg = (n_total + gridDim.x - 1u) / gridDim.x;
    const uint32_t e_end = (blockIdx.x + 1u) * per_wg < n_total ? (blockIdx.x + 1u) * per_wg : n_total;
    uint32_t rk[8], xv[8];
#pragma unroll
    for (uint32_t q = 0; q < 8u; q++) { rk[q] = 0xFFFFFFFFu; xv[q] = 0; }
    ss_rank<SS_THREADS, 8u>(p.n_lists, lcnt, lpre, raw, blockIdx.x * per_wg, e_end,
                            [&](uint32_t q, uint32_t r, uint32_t x, uint32_t) { rk[q] = r; xv[q] = x; });
    const bool solo = gridDim.x == 1u;               // one workgroup: the ascending ids replace the decoded blocks in LDS
    if (solo) {
        __syncthreads();                             // (every rank is computed: raw may be overwritten)
#pragma unroll
        for (uint32_t q = 0; q < 8u; q++) if (rk[q] != 0xFFFFFFFFu) raw[rk[q]] = xv[q];
        __syncthreads();
    } else {
        // 3. several workgroups: the ids go to a small global array; the last workgroup to get here (a device-wide
        // ticket) filters them
#pragma unroll
        for (uint32_t q = 0; q < 8u; q++) if (rk[q] != 0xFFFFFFFFu) p.sorted[rk[q]] = xv[q];
        __threadfence();
        __syncthreads();
        if (tid == 0) {
            const uint32_t t = atomicAdd(p.ticket, 1u);
            last_s = t == gridDim.x - 1u ? 1u : 0u;
            if (last_s) *p.ticket = 0u;                                   // ready for the next launch (stream order)
        }
        __syncthreads();
        if (!last_s) return;
        __threadfence();
    }
    // written by other CUs: read at device scope (past this CU's L1), relaxed, so the loads still overlap
    auto key = [&](uint32_t i) -> uint32_t {
        return solo ? raw[i] : __hip_atomic_load(p.sorted + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    const uint32_t a0 = 8u * tid;
    uint32_t kept[8];
    uint32_t keepmask = 0, cnt = 0;
    if (a0 < n_total) {
        uint32_t prev = a0 ? key(a0 - 1u) : 0u;
#pragma unroll
        for (uint32_t q = 0; q < 8u; q++) {
            const uint32_t i = a0 + q;
            kept[q] = 0;
            if (i >= n_total) continue;
            const uint32_t v = key(i);
            kept[q] = v;
            bool keep = i == 0u || prev != v;                             // first of its run
            prev = v;
            if (keep && !p.is_union) keep = i + p.n_lists - 1u < n_total && key(i + p.n_lists - 1u) == v;
            if (keep && tomb_has(p.tomb, p.tomb_nwords, v)) keep = false;
            if (keep) { keepmask |= 1u << q; cnt++; }
        }
    }
    uint32_t total;
    uint32_t pos = ss_block_scan<SS_WAVES>(cnt, wsum, &total);
#pragma unroll
    for (uint32_t q = 0; q < 8u; q++)
        if ((keepmask >> q) & 1u) { if (pos < p.out_cap) p.out[pos] = kept[q]; pos++; }
    if (tid == 0) *p.d_count = total;
}

hipError_t launch_setop_small(const SmallSetParams &p, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (ev0) (void)hipEventRecord(ev0, s);
    // one workgroup ranks everything in LDS (no global round trips: ~6 us) unless the bisections — one per id and other
    // list — are too many for one CU; then the ids are shared out (at most 8 K ids per workgroup: eight per thread)
    const uint64_t work = (uint64_t)p.lpre[p.n_lists] * (p.n_lists > 1u ? p.n_lists - 1u : 1u);
    uint32_t grid = (uint32_t)((work + 16383u) / 16384u);
    grid = grid < 1u ? 1u : grid > 32u ? 32u : grid;
    hipLaunchKernelGGL(k_setop_small, dim3(grid), dim3(SS_THREADS), 0, s, p);
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

}  // namespace ii2
