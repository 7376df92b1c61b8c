// setop_groups_batch.hip — many short AND-of-ORs / NOT queries in one launch (ii2_query_batch_groups): one workgroup per query.
// A single short grouped query is one workgroup of k_setop_groups (setop_groups.hip) and a launch and a host wait of its own:
// one of the card's 256 CUs busy for ~17 us inside a 44 - 60 us call.  An unmerged shard makes every term a group - one short
// list per Put segment - so a front end's AND / NOT queries are all of that shape; here they share one launch and one wait.
//
//   k_setop_groups_batch   query blockIdx.x of its size class, in one workgroup: the decode, rank and block-scan stages of
//                          small_set_device.h around k_setop_groups' survive rule (ss_group_run_kept: every required tag in the
//                          run of equal ids, the excluded tag not its last; then not deleted).  The query comes from the batch's
//                          device table as in k_setop_batch (BatchQuery / BatchList), which gains n_req per query and one tag
//                          byte per list; the lists of a query are in tag order, the required groups first, the lists of all
//                          its excluded groups last under tag n_req.  Two sizes, binned by the host: 256 threads and a
//                          2048-posting stage, 1024 threads and 8192 postings.  The result goes to the query's slot of the
//                          staging buffer - bounded by the slot's size, the postings of its smallest required group - the count
//                          to the query's word of the counts array.
// The scan of the counts and the pack into the caller's buffer are the flat batch's (scan.hip, k_batch_pack in setop_batch.hip).
// No workgroup waits for another one anywhere.
#include <hip/hip_runtime.h>

#include "internal.h"
#include "small_set_device.h"

namespace ii2 {

template <uint32_t THREADS, uint32_t CAP, uint32_t BLOCKS>
__global__ __launch_bounds__(THREADS) void k_setop_groups_batch(GroupBatchParams gp, uint32_t q_base) {
    constexpr uint32_t WAVES = THREADS / 64u;
    constexpr uint32_t PER_WAVE = BLOCKS / WAVES;                   // blocks a wave decodes
    constexpr uint32_t PER_THREAD = CAP / THREADS;                  // ids a thread ranks
    static_assert(PER_WAVE * WAVES == BLOCKS && PER_THREAD == 8u, "a wave takes 8 blocks, a thread 8 ids");
    __shared__ uint32_t raw[CAP];                                   // list j decoded at raw[lpre[j] ...]; then every id at its rank
    __shared__ uint8_t tags[CAP];                                   // the group tag of the id at that rank
    __shared__ uint32_t lcnt[MAX_LISTS], lpre[MAX_LISTS + 1];       // postings of every list (the host knows them), their prefix
    __shared__ uint32_t lbase[MAX_LISTS + 1];                       // first block of every list in the concatenated block list
    __shared__ const ii2_skip *lskip[MAX_LISTS];
    __shared__ const uint8_t *lpay[MAX_LISTS];
    __shared__ uint32_t wsum[WAVES];
    __shared__ uint8_t blist[BLOCKS];                               // the list every block belongs to
    __shared__ uint8_t ltag[MAX_LISTS];
    const BatchParams &p = gp.b;
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
            ltag[l] = gp.tag[bq.first_list + l];
            for (uint32_t b = bi - bl.nblk; b < bi && b < BLOCKS; b++) blist[b] = (uint8_t)l;
        }
    }
    __syncthreads();
    const uint32_t n_blocks = lbase[n_lists], n_total = lpre[n_lists];
    if (n_blocks > BLOCKS || n_total > CAP) {                       // not this size class (the host bins the queries: never taken)
        if (tid == 0) p.cnt[bq.slot] = 0;
        return;
    }
    // 1. decode, 2. ranks: at most eight ids per thread, each with its list's tag
    ss_decode<WAVES, PER_WAVE>(n_blocks, blist, lbase, lpre, raw, [&](uint32_t j) { return lskip[j]; }, [&](uint32_t j) { return lpay[j]; });
    __syncthreads();
    uint32_t rk[PER_THREAD], xv[PER_THREAD], tg[PER_THREAD];
#pragma unroll
    for (uint32_t q = 0; q < PER_THREAD; q++) { rk[q] = 0xFFFFFFFFu; xv[q] = 0; tg[q] = 0; }
    ss_rank<THREADS, PER_THREAD>(n_lists, lcnt, lpre, raw, 0u, n_total,
                                 [&](uint32_t q, uint32_t r, uint32_t x, uint32_t j) { rk[q] = r; xv[q] = x; tg[q] = ltag[j]; });
    __syncthreads();                                 // (every rank is computed: the ascending ids replace the decoded blocks)
#pragma unroll
    for (uint32_t q = 0; q < PER_THREAD; q++)
        if (rk[q] < CAP) { raw[rk[q]] = xv[q]; tags[rk[q]] = (uint8_t)tg[q]; }
    __syncthreads();
    // 3. over the ascending ids: the head of every run walks it - every required tag present, the excluded one absent - then
    // the tombstone test; block scan, write-out into the query's staging slot, count
    const uint32_t a0 = PER_THREAD * tid, n_req = bq.n_req;
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
            if (keep) keep = ss_group_run_kept(raw, tags, i, n_total, n_req);
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

// one launch per size class that holds a query
uint32_t setop_groups_batch_forms(const GroupBatchParams &p) { return (p.b.n_tiny ? BATCH_FORM_TINY : 0u) | (p.b.n_small ? BATCH_FORM_SMALL : 0u); }

hipError_t launch_setop_groups_batch(const GroupBatchParams &p, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (ev0) (void)hipEventRecord(ev0, s);
    const uint32_t forms = setop_groups_batch_forms(p);
    if (forms & BATCH_FORM_TINY)
        hipLaunchKernelGGL((k_setop_groups_batch<256u, BATCH_TINY_POSTINGS, BATCH_TINY_BLOCKS>), dim3(p.b.n_tiny), dim3(256), 0, s, p, 0u);
    if (forms & BATCH_FORM_SMALL)
        hipLaunchKernelGGL((k_setop_groups_batch<1024u, SMALL_SET_POSTINGS, SMALL_SET_BLOCKS>), dim3(p.b.n_small), dim3(1024), 0, s, p, p.b.n_tiny);
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

}  // namespace ii2
