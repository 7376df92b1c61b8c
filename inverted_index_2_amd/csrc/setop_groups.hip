// setop_groups.hip — a short AND of ORs over list ranges, with or without excluded (NOT) groups, in one launch
// (ii2_andnot_ranges).  The group path (intersect_ranges.hip) costs the driver's union and, per further group, a descriptor
// copy, a filter, three scan kernels, a compaction and a host wait; short lists spread over many Put segments - one posting
// per term and segment - are the normal state of an unmerged shard, and for them all of that is latency.  Here the whole
// query is one workgroup, one launch and one host wait.  The decode, rank and block-scan stages are those of
// small_set_device.h; particular to this kernel:
//
//   - the host lays the lists out group by group, the required groups first (tags 0 .. n_req - 1), the lists of ALL excluded
//     groups last under one tag, n_req (NOT g1 AND NOT g2 = NOT (g1 OR g2));
//   - the id AND its list's tag are stored at the rank.  Lists are in tag order, so the tags inside a run of equal ids ascend;
//   - the thread that holds the head of a run (a run is at most n_lists <= 64 long: a list holds an id once) walks it and
//     counts the tag changes among the required tags (ss_group_run_kept, shared with setop_groups_batch.hip): the id survives
//     when every required tag occurs and the run's last tag is not the excluded one.  The same id in two lists of one group -
//     or the same list twice - repeats a tag and is counted once.  Then the tombstone test, the block scan, the write-out -
//     only when the whole result fits out_cap - and the count.
//   - the threshold query (ii2_atleast_ranges) is the same kernel with "at least min_match required tags" as the rule of the run
//     walk: a second instantiation, launched by that entry point only.
// The kernel waits for no other workgroup.
#include <hip/hip_runtime.h>

#include "internal.h"
#include "small_set_device.h"

namespace ii2 {

constexpr uint32_t GS_THREADS = 1024;
constexpr uint32_t GS_WAVES = GS_THREADS / 64u;
constexpr uint32_t GS_PER_WAVE = SMALL_SET_BLOCKS / GS_WAVES;          // blocks a wave decodes
constexpr uint32_t GS_PER_THREAD = SMALL_SET_POSTINGS / GS_THREADS;    // ids a thread ranks
static_assert(GS_PER_WAVE * GS_WAVES == SMALL_SET_BLOCKS && GS_PER_THREAD == 8u, "a wave takes 8 blocks, a thread 8 ids");

template <bool AT_LEAST> __global__ __launch_bounds__(GS_THREADS) void k_setop_groups(GroupSetParams p) {
    __shared__ uint32_t raw[SMALL_SET_POSTINGS];                    // list j decoded at raw[lpre[j] ...]; then every id at its rank
    __shared__ uint8_t tags[SMALL_SET_POSTINGS];                    // the group tag of the id at that rank
    __shared__ uint32_t lcnt[MAX_LISTS], lpre[MAX_LISTS + 1];       // postings of every list (the host knows them), their prefix
    __shared__ uint32_t lbase[MAX_LISTS + 1];                       // first block of every list in the concatenated block list
    __shared__ uint32_t wsum[GS_WAVES];
    __shared__ uint8_t blist[SMALL_SET_BLOCKS];                     // the list every block belongs to
    __shared__ uint8_t ltag[MAX_LISTS];
    const uint32_t tid = threadIdx.x;
    const uint32_t n_lists = p.n_lists < MAX_LISTS ? p.n_lists : MAX_LISTS;
    if (tid <= n_lists) {
        lpre[tid] = p.lpre[tid];
        lbase[tid] = p.blk_base[tid];
        if (tid < n_lists) {
            lcnt[tid] = p.lpre[tid + 1u] - p.lpre[tid];
            ltag[tid] = p.tag[tid];
            for (uint32_t b = p.blk_base[tid]; b < p.blk_base[tid + 1u] && b < SMALL_SET_BLOCKS; b++) blist[b] = (uint8_t)tid;
        }
    }
    __syncthreads();
    const uint32_t n_blocks = lbase[n_lists], n_total = lpre[n_lists];
    if (n_blocks > SMALL_SET_BLOCKS || n_total > SMALL_SET_POSTINGS) {      // (the host sizes the query: never taken)
        if (tid == 0) *p.d_count = 0;
        return;
    }
    // 1. decode, 2. ranks: at most eight ids per thread, each with its list's tag
    ss_decode<GS_WAVES, GS_PER_WAVE>(n_blocks, blist, lbase, lpre, raw, [&](uint32_t j) { return p.lists[j].skip; },
                                     [&](uint32_t j) { return p.lists[j].payload; });
    __syncthreads();
    uint32_t rk[GS_PER_THREAD], xv[GS_PER_THREAD], tg[GS_PER_THREAD];
#pragma unroll
    for (uint32_t q = 0; q < GS_PER_THREAD; q++) { rk[q] = 0xFFFFFFFFu; xv[q] = 0; tg[q] = 0; }
    ss_rank<GS_THREADS, GS_PER_THREAD>(n_lists, lcnt, lpre, raw, 0u, n_total,
                                       [&](uint32_t q, uint32_t r, uint32_t x, uint32_t j) { rk[q] = r; xv[q] = x; tg[q] = ltag[j]; });
    __syncthreads();                                 // (every rank is computed: the ascending ids replace the decoded blocks)
#pragma unroll
    for (uint32_t q = 0; q < GS_PER_THREAD; q++)
        if (rk[q] < SMALL_SET_POSTINGS) { raw[rk[q]] = xv[q]; tags[rk[q]] = (uint8_t)tg[q]; }
    __syncthreads();
    // 3. over the ascending ids: the head of every run walks it - every required tag present, the excluded one absent - then
    // the tombstone test; block scan, write-out when the whole result fits, count
    const uint32_t a0 = GS_PER_THREAD * tid, n_req = p.n_req;
    uint32_t kept[GS_PER_THREAD];
    uint32_t keepmask = 0, cnt = 0;
    if (a0 < n_total) {
        uint32_t prev = a0 ? raw[a0 - 1u] : 0u;
#pragma unroll
        for (uint32_t q = 0; q < GS_PER_THREAD; q++) {
            const uint32_t i = a0 + q;
            kept[q] = 0;
            if (i >= n_total) continue;
            const uint32_t v = raw[i];
            kept[q] = v;
            bool keep = i == 0u || prev != v;                             // first of its run
            prev = v;
            if constexpr (AT_LEAST) {
                if (keep) keep = ss_group_run_reaches(raw, tags, i, n_total, n_req, p.min_match);
            } else {
                if (keep) keep = ss_group_run_kept(raw, tags, i, n_total, n_req);
            }
            if (keep && tomb_has(p.tomb, p.tomb_nwords, v)) keep = false;
            if (keep) { keepmask |= 1u << q; cnt++; }
        }
    }
    uint32_t total;
    uint32_t pos = ss_block_scan<GS_WAVES>(cnt, wsum, &total);
    if (total <= p.out_cap) {                        // all or nothing: the host reports II2_ECAPACITY from the count
#pragma unroll
        for (uint32_t q = 0; q < GS_PER_THREAD; q++)
            if ((keepmask >> q) & 1u) p.out[pos++] = kept[q];
    }
    if (tid == 0) *p.d_count = total;
}

hipError_t launch_setop_groups(const GroupSetParams &p, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (ev0) (void)hipEventRecord(ev0, s);
    hipLaunchKernelGGL(k_setop_groups<false>, dim3(1), dim3(GS_THREADS), 0, s, p);
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

hipError_t launch_setop_groups_atleast(const GroupSetParams &p, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (ev0) (void)hipEventRecord(ev0, s);
    hipLaunchKernelGGL(k_setop_groups<true>, dim3(1), dim3(GS_THREADS), 0, s, p);
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

}  // namespace ii2
