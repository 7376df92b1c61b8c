// topk_batch.hip — many short ranked queries in one launch (ii2_topk_batch): one workgroup per query.
// A single ranked query (ii2_topk_weighted_ranges) is the windowed bitmap form of topk.hip: per call the doc bitmap and the counter
// planes, a mark and an add per group, a histogram, a wait, a count, a scan, an emit and a second wait - also when the whole
// query is a few dozen one-posting lists of an unmerged shard.  Here such queries share one launch and one wait.
//
//   k_topk_batch   query blockIdx.x of its size class, in one workgroup.  Stages 1 and 2 are k_setop_groups_batch's
//                  (setop_groups_batch.hip): ss_decode, ss_rank, every id and its group tag stored at its rank; the query comes
//                  from the same device table (BatchQuery / BatchList, a tag byte per list) plus a weight byte per list and
//                  min_score per query.
//                  3. the head of every run of equal ids sums the weights of the run's distinct required tags (tb_run_score,
//                     topk_batch_run.h); the doc is eligible when that score reaches min_score, the run's last tag is not the
//                     excluded one and the tombstones do not have it;
//                  4. the eligible (id, score) pairs are compacted in ascending id order (ss_block_scan), ids into raw[], scores
//                     into the tag bytes; their number E is the query's `eligible` word;
//                  5. a stable counting sort of the E pairs on the digit 255 - score, ranked as k_sb_scatter (seg_build.hip)
//                     ranks a tile: wave w owns the pairs [w CAP / WAVES, ...), item j of lane l at 64 j + l; the lanes with the
//                     same digit find each other by eight ballots, the match mask gives the rank among them and a per-wave LDS
//                     counter the rank among the wave's earlier items; thread d then scans the digit totals and turns the
//                     counters into starts.  digit start + wave start + rank is the pair's place in (score descending, id
//                     ascending): it goes to that slot of the query's staging area when it is below the bound, min(k, postings
//                     of the required groups).  No histogram cut, no second pass.
// The scan of the counts and the pack into the caller's buffers are the flat batch's (scan.hip, k_batch_pack in setop_batch.hip).
// No workgroup waits for another one and the kernel uses no per-context scratch: the doc bitmap and the counter planes of the
// single-query form stay zero.
// Static LDS of the 1024-thread form: 32 KB ids, 8 KB tags / scores, 8 KB counters, ~2.5 KB list tables - two workgroups per CU,
// which is the thread limit too.
#include <hip/hip_runtime.h>

#include "internal.h"
#include "small_set_device.h"
#include "topk_batch_run.h"

namespace ii2 {

constexpr uint32_t TB_DIGITS = 256;                                 // digit = 255 - score: the best score first

template <uint32_t THREADS, uint32_t CAP, uint32_t BLOCKS>
__global__ __launch_bounds__(THREADS) void k_topk_batch(TopkBatchParams tp, uint32_t q_base) {
    constexpr uint32_t WAVES = THREADS / 64u;
    constexpr uint32_t PER_WAVE = BLOCKS / WAVES;                   // blocks a wave decodes
    constexpr uint32_t PER_THREAD = CAP / THREADS;                  // ids a thread ranks
    constexpr uint32_t WAVE_ITEMS = CAP / WAVES;                    // compacted pairs a wave places in stage 5
    static_assert(PER_WAVE * WAVES == BLOCKS && PER_THREAD == 8u, "a wave takes 8 blocks, a thread 8 ids");
    static_assert(WAVE_ITEMS == 64u * PER_THREAD && WAVES >= TB_DIGITS / 64u && CAP <= 65536u, "stage 5: eight items a lane, u16 counters");
    __shared__ uint32_t raw[CAP];                                   // list j decoded at raw[lpre[j] ...]; every id at its rank; the eligible ids
    __shared__ uint8_t tags[CAP];                                   // the group tag of the id at that rank; the eligible ids' scores
    __shared__ uint16_t wcnt[WAVES][TB_DIGITS];                     // per wave and digit: pairs so far, then the wave's first place of the digit
    __shared__ uint32_t lcnt[MAX_LISTS], lpre[MAX_LISTS + 1];       // postings of every list (the host knows them), their prefix
    __shared__ uint32_t lbase[MAX_LISTS + 1];                       // first block of every list in the concatenated block list
    __shared__ const ii2_skip *lskip[MAX_LISTS];
    __shared__ const uint8_t *lpay[MAX_LISTS];
    __shared__ uint32_t wsum[WAVES];
    __shared__ uint8_t blist[BLOCKS];                               // the list every block belongs to
    __shared__ uint8_t ltag[MAX_LISTS];
    __shared__ uint8_t tw[MAX_LISTS + 1];                           // the weight of every tag (the excluded tag's is never read)
    const BatchParams &p = tp.g.b;
    const uint32_t tid = threadIdx.x, l = tid & 63u, wv = tid >> 6;
    const BatchQuery bq = p.queries[q_base + blockIdx.x];
    const uint32_t n_lists = bq.n_lists < MAX_LISTS ? bq.n_lists : MAX_LISTS;
    if (wv == 0) {                                                  // the query's lists: counts and blocks, prefixed by one wave
        BatchList bl{nullptr, nullptr, 0u, 0u};
        if (l < n_lists) bl = p.lists[bq.first_list + l];
        const uint32_t ci = wave_incl_scan(bl.cnt), bi = wave_incl_scan(bl.nblk);
        if (l == 0) { lpre[0] = 0; lbase[0] = 0; }
        if (l < n_lists) {
            const uint32_t t = tp.g.tag[bq.first_list + l];
            lcnt[l] = bl.cnt;
            lpre[l + 1u] = ci;
            lbase[l + 1u] = bi;
            lskip[l] = bl.skip;
            lpay[l] = bl.payload;
            ltag[l] = (uint8_t)t;
            if (t <= MAX_LISTS) tw[t] = tp.weight[bq.first_list + l];     // (the lists of a group carry the same weight)
            for (uint32_t b = bi - bl.nblk; b < bi && b < BLOCKS; b++) blist[b] = (uint8_t)l;
        }
    }
    for (uint32_t i = tid; i < WAVES * TB_DIGITS; i += THREADS) (&wcnt[0][0])[i] = 0;
    __syncthreads();
    const uint32_t n_blocks = lbase[n_lists], n_total = lpre[n_lists];
    if (n_blocks > BLOCKS || n_total > CAP) {                       // not this size class (the host bins the queries: never taken)
        if (tid == 0) { p.cnt[bq.slot] = 0; tp.eligible[bq.slot] = 0; }
        return;
    }
    // 1. decode, 2. ranks: at most eight ids per thread, each with its list's tag
    ss_decode<WAVES, PER_WAVE>(n_blocks, blist, lbase, lpre, raw, [&](uint32_t j) { return lskip[j]; }, [&](uint32_t j) { return lpay[j]; });
    __syncthreads();
    {
        uint32_t rk[PER_THREAD], xv[PER_THREAD], tg[PER_THREAD];
#pragma unroll
        for (uint32_t q = 0; q < PER_THREAD; q++) { rk[q] = 0xFFFFFFFFu; xv[q] = 0; tg[q] = 0; }
        ss_rank<THREADS, PER_THREAD>(n_lists, lcnt, lpre, raw, 0u, n_total,
                                     [&](uint32_t q, uint32_t r, uint32_t x, uint32_t j) { rk[q] = r; xv[q] = x; tg[q] = ltag[j]; });
        __syncthreads();                             // (every rank is computed: the ascending ids replace the decoded blocks)
#pragma unroll
        for (uint32_t q = 0; q < PER_THREAD; q++)
            if (rk[q] < CAP) { raw[rk[q]] = xv[q]; tags[rk[q]] = (uint8_t)tg[q]; }
    }
    __syncthreads();
    // 3. over the ascending ids: the head of every run scores it; eligible: score >= min_score, not excluded, not deleted
    const uint32_t a0 = PER_THREAD * tid, n_req = bq.n_req, min_score = tp.min_score[q_base + blockIdx.x];
    uint32_t kept[PER_THREAD], ksc[PER_THREAD];
    uint32_t keepmask = 0, cnt = 0;
    if (a0 < n_total) {
        uint32_t prev = a0 ? raw[a0 - 1u] : 0u;
#pragma unroll
        for (uint32_t q = 0; q < PER_THREAD; q++) {
            const uint32_t i = a0 + q;
            kept[q] = 0;
            ksc[q] = 0;
            if (i >= n_total) continue;
            const uint32_t v = raw[i];
            kept[q] = v;
            const bool head = i == 0u || prev != v;                       // first of its run
            prev = v;
            if (!head) continue;
            bool excluded;
            const uint32_t score = tb_run_score([&](uint32_t k) { return i + k < n_total && raw[i + k] == v ? (uint32_t)tags[i + k] : TB_RUN_END; },
                                                [&](uint32_t t) { return (uint32_t)tw[t]; }, n_req, &excluded);
            ksc[q] = score;
            if (tb_run_eligible(score, excluded, min_score) && !tomb_has(p.tomb, p.tomb_nwords, v)) { keepmask |= 1u << q; cnt++; }
        }
    }
    // 4. the eligible pairs, compacted in id order: the ids to move are in registers, so the scan's barrier separates the walk's
    // reads from the overwrite
    uint32_t n_elig;
    {
        uint32_t pos = ss_block_scan<WAVES>(cnt, wsum, &n_elig);
#pragma unroll
        for (uint32_t q = 0; q < PER_THREAD; q++)
            if ((keepmask >> q) & 1u) { raw[pos] = kept[q]; tags[pos] = (uint8_t)ksc[q]; pos++; }
    }
    __syncthreads();
    // 5. every pair's place in (score descending, id ascending): a stable counting sort on 255 - score
    uint32_t id[PER_THREAD], dg[PER_THREAD], rank[PER_THREAD];
    volatile uint16_t *my_cnt = wcnt[wv];
    const uint64_t lt = (1ull << l) - 1ull;
#pragma unroll
    for (uint32_t j = 0; j < PER_THREAD; j++) {
        const uint32_t loc = wv * WAVE_ITEMS + j * 64u + l;
        const bool valid = loc < n_elig;
        id[j] = valid ? raw[loc] : 0u;
        dg[j] = valid ? (TB_DIGITS - 1u) - tags[loc] : 0u;
        rank[j] = 0;
        uint64_t m = __ballot(valid);
        if (m == 0) continue;                                             // (wave-uniform: the wave's pairs end before this item)
        const uint32_t d = dg[j];
#pragma unroll
        for (uint32_t b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const uint64_t bal = __ballot(bit);
            m &= bit ? bal : ~bal;
        }
        // m: the valid lanes whose pair has this lane's digit; the lowest of them keeps the wave's counter
        const int leader = m ? __ffsll((unsigned long long)m) - 1 : 0;
        uint32_t old = 0;
        if (valid && (int)l == leader) {
            old = my_cnt[d];
            my_cnt[d] = (uint16_t)(old + (uint32_t)__popcll(m));
        }
        old = (uint32_t)__shfl((int)old, leader, 64);
        rank[j] = old + (uint32_t)__popcll(m & lt);
        __builtin_amdgcn_wave_barrier();      // (the next item's leaders read what this item's leaders stored)
    }
    __syncthreads();
    {   // thread d: where digit d starts (exclusive scan of the digit totals) and, from it, every wave's first place
        uint32_t tot = 0;
        if (tid < TB_DIGITS)
            for (uint32_t k = 0; k < WAVES; k++) tot += wcnt[k][tid];
        const uint32_t incl = wave_incl_scan(tot);
        if (l == 63u && wv < TB_DIGITS / 64u) wsum[wv] = incl;
        __syncthreads();
        if (tid < TB_DIGITS) {
            uint32_t at = incl - tot;
            for (uint32_t w = 0; w < TB_DIGITS / 64u; w++) if (w < wv) at += wsum[w];
            for (uint32_t k = 0; k < WAVES; k++) { const uint32_t c = wcnt[k][tid]; wcnt[k][tid] = (uint16_t)at; at += c; }
        }
    }
    __syncthreads();
    uint32_t *out_ids = p.stage + bq.stage_off, *out_scores = tp.stage_scores + bq.stage_off;
#pragma unroll
    for (uint32_t j = 0; j < PER_THREAD; j++) {
        if (wv * WAVE_ITEMS + j * 64u + l >= n_elig) continue;
        const uint32_t at = wcnt[wv][dg[j]] + rank[j];
        if (at < bq.bound) { out_ids[at] = id[j]; out_scores[at] = (TB_DIGITS - 1u) - dg[j]; }
    }
    if (tid == 0) {
        p.cnt[bq.slot] = n_elig < bq.bound ? n_elig : bq.bound;
        tp.eligible[bq.slot] = n_elig;
    }
}

// one launch per size class that holds a query
hipError_t launch_topk_batch(const TopkBatchParams &p, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (ev0) (void)hipEventRecord(ev0, s);
    const BatchParams &b = p.g.b;
    if (b.n_tiny) hipLaunchKernelGGL((k_topk_batch<256u, BATCH_TINY_POSTINGS, BATCH_TINY_BLOCKS>), dim3(b.n_tiny), dim3(256), 0, s, p, 0u);
    if (b.n_small) hipLaunchKernelGGL((k_topk_batch<1024u, SMALL_SET_POSTINGS, SMALL_SET_BLOCKS>), dim3(b.n_small), dim3(1024), 0, s, p, b.n_tiny);
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

}  // namespace ii2
