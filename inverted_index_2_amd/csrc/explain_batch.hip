// explain_batch.hip — which groups each doc of many short result pages lies in, in one launch (ii2_explain_batch): one workgroup
// per query.  A single explain (ii2_explain_ranges) is the windowed bitmap form of explain_ranges.hip: per call an (id, row) table
// in workspace, a mark, a walk and a clear per window and up to two waits - also for a page of ten ids over a few dozen
// one-posting lists of an unmerged shard.  Here such queries share one launch and one wait.
//
//   k_explain_batch   query blockIdx.x of its size class, in one workgroup.  The query comes from the batch calls' device table
//                     (BatchQuery / BatchList: stage_off = the first word of its rows, bound = its ids) plus the 32-bit group
//                     number of every list and, per query, the start of its id slice and the words of a row.
//                     1. ss_decode (small_set_device.h): every list one ascending stretch of raw[];
//                     2. meanwhile the page's ids go to LDS and into an LDS table of (id << 32 | row) entries as k_ex_prepare
//                        builds it in workspace: a compare-and-swap claims an empty slot, a slot that holds the same id takes the
//                        smaller entry by atomicMin - a repeated id keeps its FIRST row; the table has at least twice as many
//                        slots as ids.  A row that does not find itself in the table is a later copy and stays zero;
//                     3. NO ranking.  Pair (row r, list j) = p mod n_ids, p div n_ids, thread t the pairs t, t + THREADS, ...: one
//                        branch-free bisection of list j's stretch for the row's id; a hit ORs bit g & 63 of the list's group g
//                        into word g >> 6 of the row (a 64-bit vector atomic: the lists of a word's groups are different
//                        threads' pairs).  The bits that were clear before are the query's hits: several lists of one group that
//                        hold the id count once.
// The host zeroes all rows of a call with one memset in front of the launch, so the kernel stores nothing but its hits and one
// hit count per query.  No workgroup waits for another one and the kernel uses no per-context scratch: the doc bitmap, its
// summary and the workspace table of the single form stay as they were.
// Static LDS of the 1024-thread form: 32 KB decoded ids, 16 KB table, 4 KB page ids, 1 KB later-copy flags, ~2.6 KB list tables:
// 55.6 KB.  II2_EXPLAIN_BATCH_IDS = 1024 is what keeps it below 64 KB: 2048 ids would want a 32 KB table and 8 KB of ids.
#include <hip/hip_runtime.h>

#include "internal.h"
#include "small_set_device.h"

namespace ii2 {

template <uint32_t THREADS, uint32_t CAP, uint32_t BLOCKS>
__global__ __launch_bounds__(THREADS) void k_explain_batch(ExplainBatchParams ep, uint32_t q_base) {
    constexpr uint32_t WAVES = THREADS / 64u;
    constexpr uint32_t PER_WAVE = BLOCKS / WAVES;                   // blocks a wave decodes
    constexpr uint32_t IDS = II2_EXPLAIN_BATCH_IDS, SLOTS = 2u * IDS;
    static_assert(PER_WAVE * WAVES == BLOCKS && (SLOTS & (SLOTS - 1u)) == 0u, "a wave takes 8 blocks; the table is a power of two");
    __shared__ uint32_t raw[CAP];                                   // list j decoded at raw[lpre[j] ...]
    __shared__ unsigned long long table[SLOTS];                     // (id << 32 | first row), EX_EMPTY where free
    __shared__ uint32_t ids[IDS];                                   // the page
    __shared__ uint8_t later[IDS];                                  // 1: the row repeats an earlier row's id
    __shared__ uint32_t lcnt[MAX_LISTS], lpre[MAX_LISTS + 1];       // postings of every list (the host knows them), their prefix
    __shared__ uint32_t lbase[MAX_LISTS + 1];                       // first block of every list in the concatenated block list
    __shared__ const ii2_skip *lskip[MAX_LISTS];
    __shared__ const uint8_t *lpay[MAX_LISTS];
    __shared__ uint32_t lgrp[MAX_LISTS];                            // the group of every list: a number, not a tag byte
    __shared__ uint8_t blist[BLOCKS];                               // the list every block belongs to
    __shared__ uint32_t n_fresh;
    const BatchParams &p = ep.b;
    const uint32_t tid = threadIdx.x, l = tid & 63u, wv = tid >> 6;
    const BatchQuery bq = p.queries[q_base + blockIdx.x];
    const ExplainBatchQuery xq = ep.pages[q_base + blockIdx.x];
    const uint32_t n_lists = bq.n_lists < MAX_LISTS ? bq.n_lists : MAX_LISTS;
    const uint32_t n_ids = bq.bound < IDS ? bq.bound : IDS;
    uint32_t log2_slots = 6;
    while ((1u << log2_slots) < 2u * n_ids) log2_slots++;           // (<= SLOTS: n_ids <= IDS)
    const uint32_t n_slots = 1u << log2_slots, smask = n_slots - 1u;
    if (wv == 0) {                                                  // the query's lists: counts and blocks, prefixed by one wave
        BatchList bl{nullptr, nullptr, 0u, 0u};
        if (l < n_lists) bl = p.lists[bq.first_list + l];
        const uint32_t ci = wave_incl_scan(bl.cnt), bi = wave_incl_scan(bl.nblk);
        if (l == 0) { lpre[0] = 0; lbase[0] = 0; n_fresh = 0; }
        if (l < n_lists) {
            lcnt[l] = bl.cnt;
            lpre[l + 1u] = ci;
            lbase[l + 1u] = bi;
            lskip[l] = bl.skip;
            lpay[l] = bl.payload;
            lgrp[l] = ep.grp[bq.first_list + l];
            for (uint32_t b = bi - bl.nblk; b < bi && b < BLOCKS; b++) blist[b] = (uint8_t)l;
        }
    }
    const uint32_t *page = ep.ids + xq.ids_first;                   // read at [0, n_ids) only
    for (uint32_t r = tid; r < n_ids; r += THREADS) ids[r] = page[r];
    for (uint32_t s = tid; s < n_slots; s += THREADS) table[s] = EX_EMPTY;
    __syncthreads();
    const uint32_t n_blocks = lbase[n_lists], n_total = lpre[n_lists];
    if (n_blocks > BLOCKS || n_total > CAP) {                       // not this size class (the host bins the queries: never taken)
        if (tid == 0) p.cnt[bq.slot] = 0;
        return;
    }
    // 2. every row into the table (never EX_EMPTY: row < IDS); the probe ends at an empty slot, the table is at most half full
    for (uint32_t r = tid; r < n_ids; r += THREADS) {
        const uint32_t id = ids[r];
        const unsigned long long e = ((unsigned long long)id << 32) | r;
        uint32_t s = ex_slot(id, log2_slots);
        for (uint32_t probe = 0; probe <= smask; probe++, s = (s + 1u) & smask) {
            const unsigned long long old = atomicCAS(&table[s], (unsigned long long)EX_EMPTY, e);
            if (old == EX_EMPTY) break;
            if ((uint32_t)(old >> 32) == id) {                      // the id again: its first row stays
                atomicMin(&table[s], e);
                break;
            }
        }
    }
    // 1. decode
    ss_decode<WAVES, PER_WAVE>(n_blocks, blist, lbase, lpre, raw, [&](uint32_t j) { return lskip[j]; }, [&](uint32_t j) { return lpay[j]; });
    __syncthreads();
    for (uint32_t r = tid; r < n_ids; r += THREADS) {               // the table is complete: is this row its id's first?
        const uint32_t id = ids[r];
        uint32_t s = ex_slot(id, log2_slots), first = r;
        for (uint32_t probe = 0; probe <= smask; probe++, s = (s + 1u) & smask) {
            const unsigned long long e = table[s];
            if (e == EX_EMPTY) break;
            if ((uint32_t)(e >> 32) == id) { first = (uint32_t)e; break; }
        }
        later[r] = first != r ? 1u : 0u;
    }
    __syncthreads();
    // 3. a bisection per (row, list) pair; neighbouring threads take neighbouring rows of one list
    unsigned long long *rows = ep.masks + bq.stage_off;
    const uint32_t n_pairs = n_ids * n_lists, n_words = xq.n_words;
    uint32_t fresh = 0;
    for (uint32_t pr = tid; pr < n_pairs; pr += THREADS) {
        const uint32_t j = pr / n_ids, r = pr - j * n_ids;
        const uint32_t x = ids[r], n = lcnt[j];
        if (later[r] || n == 0u) continue;                          // (no list of the table is empty)
        const uint32_t *B = raw + lpre[j];
        uint32_t pos = 0;                                           // the ids of the list below x
        for (uint32_t st = 1u << (31u - (uint32_t)__clz((int)n)); st > 0u; st >>= 1) {
            const uint32_t cand = pos + st;
            if (cand <= n && B[cand - 1u] < x) pos = cand;
        }
        if (pos >= n || B[pos] != x) continue;
        const uint32_t g = lgrp[j];
        if ((g >> 6) >= n_words) continue;                          // (the host numbers the groups below 64 n_words: never taken)
        const unsigned long long bit = 1ull << (g & 63u);
        const unsigned long long old = atomicOr(&rows[(uint64_t)r * n_words + (g >> 6)], bit);
        fresh += (old & bit) ? 0u : 1u;
    }
    const uint32_t s = wave_sum(fresh);
    if (l == 0 && s) atomicAdd(&n_fresh, s);
    __syncthreads();
    if (tid == 0) p.cnt[bq.slot] = n_fresh;
}

// one launch per size class that holds a query
hipError_t launch_explain_batch(const ExplainBatchParams &p, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (ev0) (void)hipEventRecord(ev0, s);
    const BatchParams &b = p.b;
    if (b.n_tiny) hipLaunchKernelGGL((k_explain_batch<256u, BATCH_TINY_POSTINGS, BATCH_TINY_BLOCKS>), dim3(b.n_tiny), dim3(256), 0, s, p, 0u);
    if (b.n_small) hipLaunchKernelGGL((k_explain_batch<1024u, SMALL_SET_POSTINGS, SMALL_SET_BLOCKS>), dim3(b.n_small), dim3(1024), 0, s, p, b.n_tiny);
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

}  // namespace ii2
