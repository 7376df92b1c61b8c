// setop_groups.hip — a short AND of ORs over list ranges, with or without excluded (NOT) groups, in one launch
// (ii2_andnot_ranges).  The group path (intersect_ranges.hip) costs the driver's union and, per further group, a descriptor
// copy, a filter, three scan kernels, a compaction and a host wait; short lists spread over many Put segments - one posting
// per term and segment - are the normal state of an unmerged shard, and for them all of that is latency.  Here the whole
// query is one workgroup, one launch and one host wait, in the manner of k_setop_batch's 1024-thread form:
//
//   1. every block of every list is decoded into LDS, one wave per block.  The host lays the lists out group by group, the
//      required groups first (tags 0 .. n_req - 1), the lists of ALL excluded groups last under one tag, n_req
//      (NOT g1 AND NOT g2 = NOT (g1 OR g2));
//   2. an id's rank among all ids = its position in its own list + one bisection per other list, ties broken by the list
//      number (the ranks are a permutation); the id AND its list's tag are stored at the rank.  Lists are in tag order, so
//      the tags inside a run of equal ids ascend;
//   3. the thread that holds the head of a run (a run is at most n_lists <= 64 long: a list holds an id once) walks it and
//      counts the tag changes among the required tags: the id survives when every required tag occurs and the run's last
//      tag is not the excluded one.  The same id in two lists of one group - or the same list twice - repeats a tag and is
//      counted once.  Then the tombstone test, a block scan, the write-out - only when the whole result fits out_cap - and
//      the count.
// The kernel waits for no other workgroup.
#include <hip/hip_runtime.h>

#include "dv1_device.h"
#include "internal.h"

namespace ii2 {

constexpr uint32_t GS_THREADS = 1024;
constexpr uint32_t GS_WAVES = GS_THREADS / 64u;
constexpr uint32_t GS_PER_WAVE = SMALL_SET_BLOCKS / GS_WAVES;          // blocks a wave decodes
constexpr uint32_t GS_PER_THREAD = SMALL_SET_POSTINGS / GS_THREADS;    // ids a thread ranks
static_assert(GS_PER_WAVE * GS_WAVES == SMALL_SET_BLOCKS && GS_PER_THREAD == 8u, "a wave takes 8 blocks, a thread 8 ids");

__global__ __launch_bounds__(GS_THREADS) void k_setop_groups(GroupSetParams p) {
    __shared__ uint32_t raw[SMALL_SET_POSTINGS];                    // list j decoded at raw[lpre[j] ...]; then every id at its rank
    __shared__ uint8_t tags[SMALL_SET_POSTINGS];                    // the group tag of the id at that rank
    __shared__ uint32_t lcnt[MAX_LISTS], lpre[MAX_LISTS + 1];       // postings of every list (the host knows them), their prefix
    __shared__ uint32_t lbase[MAX_LISTS + 1];                       // first block of every list in the concatenated block list
    __shared__ uint32_t wsum[GS_WAVES];
    __shared__ uint8_t blist[SMALL_SET_BLOCKS];                     // the list every block belongs to
    __shared__ uint8_t ltag[MAX_LISTS];
    const uint32_t tid = threadIdx.x, l = tid & 63u, wv = tid >> 6;
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
    // 1. decode: block b of the concatenated block list, one wave each (wave w: blocks w, w + 16, ...); every block of a list
    // but its last is full, so block bi of list j starts at raw[lpre[j] + 256 bi].  The skip entries of all the wave's
    // blocks are requested first, then the first 256 payload bytes of all of them, then they are decoded.
    uint32_t bj[GS_PER_WAVE], q0[GS_PER_WAVE], q1[GS_PER_WAVE], f0[GS_PER_WAVE], pw[GS_PER_WAVE];
#pragma unroll
    for (uint32_t t = 0; t < GS_PER_WAVE; t++) {
        const uint32_t b = wv + t * GS_WAVES;
        bj[t] = 0xFFFFFFFFu; q0[t] = 0; q1[t] = 0; f0[t] = 0;
        if (b < n_blocks) {
            const uint32_t j = blist[b];                                  // (wave-uniform)
            const ii2_skip *sk = p.lists[j].skip + (b - lbase[j]);
            const ii2_skip e0 = sk[0], e1 = sk[1];
            bj[t] = j; q0[t] = e0.byte_off; q1[t] = e1.byte_off; f0[t] = e0.first_doc;
        }
    }
#pragma unroll
    for (uint32_t t = 0; t < GS_PER_WAVE; t++) {
        pw[t] = 0;
        if (bj[t] != 0xFFFFFFFFu && q0[t] + 4u * l < q1[t]) pw[t] = load_u32_unaligned(p.lists[bj[t]].payload + q0[t] + 4u * l);
    }
#pragma unroll
    for (uint32_t t = 0; t < GS_PER_WAVE; t++) {
        if (bj[t] == 0xFFFFFFFFu) continue;                               // (wave-uniform)
        const uint32_t b = wv + t * GS_WAVES, j = bj[t];
        const uint32_t at = lpre[j] + (b - lbase[j]) * II2_DV1_BLOCK, end = lpre[j + 1u];
        const uint8_t *pl = p.lists[j].payload;
        const uint32_t first_q = q0[t], pre = pw[t];
        decode_block_wave([&](uint32_t myq) -> uint32_t { return myq == first_q + 4u * l ? pre : load_u32_unaligned(pl + myq); },
                          q0[t], q1[t], f0[t], [&](uint32_t ix, uint32_t id) { if (at + ix < end) raw[at + ix] = id; });
    }
    __syncthreads();
    // 2. ranks: at most eight ids per thread (list-major numbering e = 0 .. n_total)
    uint32_t top = 1;                                // the largest power of two <= the longest list
    for (uint32_t c = l; c < n_lists; c += 64u) top = lcnt[c] > top ? lcnt[c] : top;
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)top, d, 64); top = o > top ? o : top; }
    top = 1u << (31u - (uint32_t)__clz((int)top));
    uint32_t rk[GS_PER_THREAD], xv[GS_PER_THREAD], tg[GS_PER_THREAD];
#pragma unroll 4
    for (uint32_t q = 0; q < GS_PER_THREAD; q++) {
        const uint32_t e = tid + q * GS_THREADS;
        rk[q] = 0xFFFFFFFFu;
        xv[q] = 0;
        tg[q] = 0;
        if (e >= n_total) continue;
        uint32_t j = 0;                                                   // my list: the last j with lpre[j] <= e
        for (uint32_t st = 32u; st > 0u; st >>= 1) if (j + st < n_lists && lpre[j + st] <= e) j += st;
        const uint32_t x = raw[e];
        uint32_t r = e - lpre[j];
        if (n_lists <= 8u) {
            for (uint32_t c = 0; c < n_lists; c++) {
                if (c == j) continue;
                const uint32_t *B = raw + lpre[c];
                uint32_t lo = 0, hi = lcnt[c];                            // first index with B[i] > x (c < j) or >= x (c > j)
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    const uint32_t y = B[mid];
                    if (y < x || (c < j && y == x)) lo = mid + 1u; else hi = mid;
                }
                r += lo;
            }
        } else {
            // many lists: branch-free bisections with the same steps for every list, eight lists (eight independent
            // chains of LDS reads) at a time
            for (uint32_t c0 = 0; c0 < n_lists; c0 += 8u) {
                uint32_t pos[8], n[8], base[8];
#pragma unroll
                for (uint32_t u = 0; u < 8u; u++) {
                    const uint32_t c = c0 + u;
                    const bool on = c < n_lists && c != j;
                    n[u] = on ? lcnt[c] : 0u;
                    base[u] = on ? lpre[c] : 0u;
                    pos[u] = 0;
                }
                for (uint32_t st = top; st > 0u; st >>= 1) {
#pragma unroll
                    for (uint32_t u = 0; u < 8u; u++) {
                        const uint32_t cand = pos[u] + st;
                        if (cand <= n[u]) {
                            const uint32_t y = raw[base[u] + cand - 1u];
                            if (y < x || (c0 + u < j && y == x)) pos[u] = cand;     // ties: lists before mine go first
                        }
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < 8u; u++) r += pos[u];
            }
        }
        rk[q] = r;
        xv[q] = x;
        tg[q] = ltag[j];
    }
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
            if (keep) {
                uint32_t seen = 0, last = 0xFFFFFFFFu;
                for (uint32_t k = i; k < n_total && raw[k] == v; k++) {
                    const uint32_t t = tags[k];
                    seen += (t != last && t < n_req) ? 1u : 0u;
                    last = t;
                }
                keep = seen == n_req && last < n_req;
            }
            if (keep && p.tomb && (v >> 5) < p.tomb_nwords) keep = ((p.tomb[v >> 5] >> (v & 31u)) & 1u) == 0u;
            if (keep) { keepmask |= 1u << q; cnt++; }
        }
    }
    const uint32_t incl = wave_incl_scan(cnt);
    if (l == 63u) wsum[wv] = incl;
    __syncthreads();
    uint32_t pos = incl - cnt, total = 0;
    for (uint32_t w = 0; w < GS_WAVES; w++) { if (w < wv) pos += wsum[w]; total += wsum[w]; }
    if (total <= p.out_cap) {                        // all or nothing: the host reports II2_ECAPACITY from the count
#pragma unroll
        for (uint32_t q = 0; q < GS_PER_THREAD; q++)
            if ((keepmask >> q) & 1u) p.out[pos++] = kept[q];
    }
    if (tid == 0) *p.d_count = total;
}

hipError_t launch_setop_groups(const GroupSetParams &p, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (ev0) (void)hipEventRecord(ev0, s);
    hipLaunchKernelGGL(k_setop_groups, dim3(1), dim3(GS_THREADS), 0, s, p);
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

}  // namespace ii2
