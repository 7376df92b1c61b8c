// setop_batch.hip — many small AND / OR queries in one launch (ii2_query_batch): one workgroup per query.
// A single small query is one workgroup of k_setop_small (setop_small.hip) and a launch of its own: one of the card's 256
// CUs busy, the others idle, a launch (and for a synchronous call a stream wait) per query.  A search front end has
// thousands of such queries (PrefixSearch takes MANY prefixes, inverted_index.go:192); here they share one launch.
//
//   k_setop_batch   query blockIdx.x of its size class, in one workgroup: the decode, rank and block-scan stages of
//                   small_set_device.h around k_setop_small's filter (first of its run, for an AND a run of n_lists, not
//                   deleted), with the query read from a device table (BatchQuery / BatchList) instead of a by-value
//                   parameter block, and in two sizes: 256 threads and a 2048-posting stage for the common tiny query (up
//                   to eight workgroups per CU), 1024 threads and 8192 postings for the rest.  The host bins the queries by
//                   size, so every launch has one workgroup shape.  The result goes to the query's slot of the batch's
//                   staging buffer (its size is the host-known bound of the result), the count to the query's word of the
//                   counts array.
//   k_batch_pack    after the scan of the counts: staging -> the caller's buffer, results back to back in query order.  It
//                   tests the total against the capacity itself and writes nothing when it does not fit, so it is enqueued
//                   before the call's one stream wait.
// No workgroup waits for another one anywhere: the order of the results comes from the scan between the two kernels.
#include <hip/hip_runtime.h>

#include "internal.h"
#include "small_set_device.h"

namespace ii2 {

template <uint32_t THREADS, uint32_t CAP, uint32_t BLOCKS>
__global__ __launch_bounds__(THREADS) void k_setop_batch(BatchParams p, uint32_t q_base) {
    constexpr uint32_t WAVES = THREADS / 64u;
    constexpr uint32_t PER_WAVE = BLOCKS / WAVES;                   // blocks a wave decodes
    constexpr uint32_t PER_THREAD = CAP / THREADS;                  // ids a thread ranks
    static_assert(PER_WAVE * WAVES == BLOCKS && PER_THREAD == 8u, "a wave takes 8 blocks, a thread 8 ids");
    __shared__ uint32_t raw[CAP];                                   // list j decoded at raw[lpre[j] ...], ascending
    __shared__ uint32_t lcnt[MAX_LISTS], lpre[MAX_LISTS + 1];       // postings of every list (the host knows them), their prefix
    __shared__ uint32_t lbase[MAX_LISTS + 1];                       // first block of every list in the concatenated block list
    __shared__ const ii2_skip *lskip[MAX_LISTS];
    __shared__ const uint8_t *lpay[MAX_LISTS];
    __shared__ uint32_t wsum[WAVES];
    __shared__ uint8_t blist[BLOCKS];                               // the list every block belongs to
    const uint32_t tid = threadIdx.x, l = tid & 63u, wv = tid >> 6;
    const BatchQuery bq = p.queries[q_base + blockIdx.x];
    const uint32_t n_lists = bq.n_lists < MAX_LISTS ? bq.n_lists : MAX_LISTS;
    if (wv == 0) {                                                  // the query's lists: counts and blocks, prefixed by one wave
        BatchList bl{nullptr, nullptr, 0u, 0u};
        if (l < n_lists) bl = p.lists[bq.first_list + l];
        const uint32_t ci = wave_incl_scan(bl.cnt), bi = wave_incl_scan(bl.nblk);
        if (l == 0) { lpre[0] = 0; lbase[0] = 0; }
        if (l < n_lists) {
            lcnt[l] = bl.cnt;
            lpre[l + 1u] = ci;
            lbase[l + 1u] = bi;
            lskip[l] = bl.skip;
            lpay[l] = bl.payload;
            for (uint32_t b = bi - bl.nblk; b < bi && b < BLOCKS; b++) blist[b] = (uint8_t)l;
        }
    }
    __syncthreads();
    const uint32_t n_blocks = lbase[n_lists], n_total = lpre[n_lists];
    if (n_blocks > BLOCKS || n_total > CAP) {                       // not this size class (the host bins the queries: never taken)
        if (tid == 0) p.cnt[bq.slot] = 0;
        return;
    }
    // 1. decode, 2. ranks: at most eight ids per thread
    ss_decode<WAVES, PER_WAVE>(n_blocks, blist, lbase, lpre, raw, [&](uint32_t j) { return lskip[j]; }, [&](uint32_t j) { return lpay[j]; });
    __syncthreads();
    uint32_t rk[PER_THREAD], xv[PER_THREAD];
#pragma unroll
    for (uint32_t q = 0; q < PER_THREAD; q++) { rk[q] = 0xFFFFFFFFu; xv[q] = 0; }
    ss_rank<THREADS, PER_THREAD>(n_lists, lcnt, lpre, raw, 0u, n_total, [&](uint32_t q, uint32_t r, uint32_t x, uint32_t) { rk[q] = r; xv[q] = x; });
    __syncthreads();                                 // (every rank is computed: the ascending ids replace the decoded blocks)
#pragma unroll
    for (uint32_t q = 0; q < PER_THREAD; q++) if (rk[q] < CAP) raw[rk[q]] = xv[q];
    __syncthreads();
    // 3. over the ascending ids: the first id of every run survives - for an AND only when the run is n_lists long - unless
    // the tombstone bitmap has it; block scan, write-out into the query's staging slot, count
    const uint32_t a0 = PER_THREAD * tid;
    uint32_t kept[PER_THREAD];
    uint32_t keepmask = 0, cnt = 0;
    if (a0 < n_total) {
        uint32_t prev = a0 ? raw[a0 - 1u] : 0u;
#pragma unroll
        for (uint32_t q = 0; q < PER_THREAD; q++) {
            const uint32_t i = a0 + q;
            kept[q] = 0;
            if (i >= n_total) continue;
            const uint32_t v = raw[i];
            kept[q] = v;
            bool keep = i == 0u || prev != v;                             // first of its run
            prev = v;
            if (keep && !bq.is_union) keep = i + n_lists - 1u < n_total && raw[i + n_lists - 1u] == v;
            if (keep && tomb_has(p.tomb, p.tomb_nwords, v)) keep = false;
            if (keep) { keepmask |= 1u << q; cnt++; }
        }
    }
    uint32_t total;
    uint32_t pos = ss_block_scan<WAVES>(cnt, wsum, &total);
    uint32_t *out = p.stage + bq.stage_off;
#pragma unroll
    for (uint32_t q = 0; q < PER_THREAD; q++)
        if ((keepmask >> q) & 1u) { if (pos < bq.bound) out[pos] = kept[q]; pos++; }
    if (tid == 0) p.cnt[bq.slot] = total < bq.bound ? total : bq.bound;
}

constexpr uint32_t PACK_THREADS = 256;

// result q: off[q + 1] - off[q] ids from its staging slot to out + off[q]; workgroups (x, y): queries x, x + gridDim.x, ...,
// every gridDim.y-th run of 256 ids of each
__global__ __launch_bounds__(PACK_THREADS) void k_batch_pack(BatchPackParams p) {
    if (p.off[p.n_queries] > p.cap) return;          // all or nothing: the host reports II2_ECAPACITY from the same word
    for (uint32_t q = blockIdx.x; q < p.n_queries; q += gridDim.x) {
        const uint64_t o0 = p.off[q], n = p.off[q + 1u] - o0;
        const uint32_t *src = p.stage + p.stage_off[q];
        for (uint64_t i = (uint64_t)blockIdx.y * PACK_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.y * PACK_THREADS)
            p.out[o0 + i] = src[i];
    }
}

// one launch per size class that holds a query
uint32_t setop_batch_forms(const BatchParams &p) { return (p.n_tiny ? BATCH_FORM_TINY : 0u) | (p.n_small ? BATCH_FORM_SMALL : 0u); }

hipError_t launch_setop_batch(const BatchParams &p, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (ev0) (void)hipEventRecord(ev0, s);
    const uint32_t forms = setop_batch_forms(p);
    if (forms & BATCH_FORM_TINY)
        hipLaunchKernelGGL((k_setop_batch<256u, BATCH_TINY_POSTINGS, BATCH_TINY_BLOCKS>), dim3(p.n_tiny), dim3(256), 0, s, p, 0u);
    if (forms & BATCH_FORM_SMALL)
        hipLaunchKernelGGL((k_setop_batch<1024u, SMALL_SET_POSTINGS, SMALL_SET_BLOCKS>), dim3(p.n_small), dim3(1024), 0, s, p, p.n_tiny);
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

hipError_t launch_batch_pack(const BatchPackParams &p, uint64_t max_bound, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (ev0) (void)hipEventRecord(ev0, s);
    if (p.n_queries) {
        // one workgroup per query while the results are short; a long result (a large query of the batch) is shared out
        const uint32_t gx = p.n_queries < 65536u ? p.n_queries : 65536u;
        uint64_t gy = (max_bound + 8u * PACK_THREADS - 1u) / (8u * PACK_THREADS);
        gy = gy < 1u ? 1u : gy > 256u ? 256u : gy;
        while (gy > 1u && gx * gy > (1u << 20)) gy >>= 1;
        hipLaunchKernelGGL(k_batch_pack, dim3(gx, (uint32_t)gy), dim3(PACK_THREADS), 0, s, p);
    }
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

}  // namespace ii2
