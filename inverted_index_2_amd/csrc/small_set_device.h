// small_set_device.h — the three stages that the short-list set-op kernels share: k_setop_small (setop_small.hip),
// k_setop_batch in both sizes (setop_batch.hip), k_setop_groups (setop_groups.hip) and k_setop_groups_batch in both sizes
// (setop_groups_batch.hip) - and the survive rule of the two group kernels, ss_group_run_kept.
//
// A short query - at most MAX_LISTS lists that hold at most PER_THREAD x THREADS postings in PER_WAVE x WAVES DV1 blocks -
// is decoded, ordered and filtered in the LDS of one workgroup:
//   1. ss_decode      every block of the concatenated block list into raw[], list j as one ascending stretch raw[lpre[j] ...];
//   2. ss_rank        an id's rank among all ids = its index in its own list + one bisection per other list, ties broken by
//                     the list number, so the ranks are a permutation: storing every id at its rank sorts them - no sort
//                     network;
//   3. ss_block_scan  the output positions of what the kernel's filter over the ascending ids keeps.
// The kernels differ in where their list table comes from (by-value parameters or a device table), in how many workgroups
// share the ranking, in what survives a run of equal ids and in the write-out rule: all of that stays in the kernel files.
// All pointers but the functors' are LDS; the calls are workgroup-uniform.
#pragma once
#include "dv1_device.h"

namespace ii2 {

// Stage 1.  Block b of the concatenated block list belongs to list blist[b], whose first block is lbase[j]; wave w of WAVES
// decodes blocks w, w + WAVES, ... (PER_WAVE at most, b < n_blocks).  Every block of a list but its last is full, so block bi
// of list j starts at raw[lpre[j] + 256 bi]; ids past the list's end (lpre[j + 1]) are dropped.  The skip entries of all the
// wave's blocks are requested first, then the first 256 payload bytes of all of them, then they are decoded: two memory
// round trips per wave instead of two per block.  skip_of(j) / pay_of(j): the skip entry of list j's first block (the entry
// after its last block is readable) and the payload its byte offsets refer to.  The caller's barrier follows.
template <uint32_t WAVES, uint32_t PER_WAVE, class SkipOf, class PayOf>
__device__ __forceinline__ void ss_decode(uint32_t n_blocks, const uint8_t *blist, const uint32_t *lbase, const uint32_t *lpre,
                                          uint32_t *raw, SkipOf skip_of, PayOf pay_of) {
    const uint32_t l = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t bj[PER_WAVE], q0[PER_WAVE], q1[PER_WAVE], f0[PER_WAVE], pw[PER_WAVE];
#pragma unroll
    for (uint32_t t = 0; t < PER_WAVE; t++) {
        const uint32_t b = wv + t * WAVES;
        bj[t] = 0xFFFFFFFFu; q0[t] = 0; q1[t] = 0; f0[t] = 0;
        if (b < n_blocks) {
            const uint32_t j = blist[b];                                  // (wave-uniform)
            const ii2_skip *sk = skip_of(j) + (b - lbase[j]);
            const ii2_skip e0 = sk[0], e1 = sk[1];
            bj[t] = j; q0[t] = e0.byte_off; q1[t] = e1.byte_off; f0[t] = e0.first_doc;
        }
    }
#pragma unroll
    for (uint32_t t = 0; t < PER_WAVE; t++) {
        pw[t] = 0;
        if (bj[t] != 0xFFFFFFFFu && q0[t] + 4u * l < q1[t]) pw[t] = load_u32_unaligned(pay_of(bj[t]) + q0[t] + 4u * l);
    }
#pragma unroll
    for (uint32_t t = 0; t < PER_WAVE; t++) {
        if (bj[t] == 0xFFFFFFFFu) continue;                               // (wave-uniform)
        const uint32_t b = wv + t * WAVES, j = bj[t];
        const uint32_t at = lpre[j] + (b - lbase[j]) * II2_DV1_BLOCK, end = lpre[j + 1u];
        const uint8_t *pl = pay_of(j);
        const uint32_t first_q = q0[t], pre = pw[t];
        decode_block_wave([&](uint32_t myq) -> uint32_t { return myq == first_q + 4u * l ? pre : load_u32_unaligned(pl + myq); },
                          q0[t], q1[t], f0[t], [&](uint32_t ix, uint32_t id) { if (at + ix < end) raw[at + ix] = id; });
    }
}

// Stage 2.  The ids are numbered list by list, e = 0 .. lpre[n_lists]; the workgroup ranks e_first <= e < e_end (at most
// PER_THREAD x THREADS of them), thread t the ids e_first + t + q THREADS, and calls done(q, rank, id, list) for each.  List
// c holds lcnt[c] ids at raw[lpre[c] ...].  Ranks only read raw[]: a caller that stores the ids back into it puts a barrier
// in between.
template <uint32_t THREADS, uint32_t PER_THREAD, class Done>
__device__ __forceinline__ void ss_rank(uint32_t n_lists, const uint32_t *lcnt, const uint32_t *lpre, const uint32_t *raw, uint32_t e_first,
                                        uint32_t e_end, Done done) {
    const uint32_t l = threadIdx.x & 63u;
    uint32_t top = 1;                                // the largest power of two <= the longest list
    for (uint32_t c = l; c < n_lists; c += 64u) top = lcnt[c] > top ? lcnt[c] : top;
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)top, d, 64); top = o > top ? o : top; }
    top = 1u << (31u - (uint32_t)__clz((int)top));
#pragma unroll 4
    for (uint32_t q = 0; q < PER_THREAD; q++) {
        const uint32_t e = e_first + threadIdx.x + q * THREADS;
        if (e >= e_end) continue;
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
            // many lists: a bisection per list is a chain of dependent LDS reads, and the chains of 63 lists one after the
            // other were most of the kernel's time — branch-free bisections with the same steps for every list, eight
            // lists (eight independent chains) at a time
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
        done(q, r, x, j);
    }
}

// Stage 3.  Exclusive scan of cnt over the workgroup's WAVES x 64 threads, in thread order: returns the sum over the threads
// before this one, *total = the sum over all.  wsum: WAVES words of LDS; one barrier.  All threads must call.
template <uint32_t WAVES>
__device__ __forceinline__ uint32_t ss_block_scan(uint32_t cnt, uint32_t *wsum, uint32_t *total) {
    const uint32_t l = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan(cnt);
    if (l == 63u) wsum[wv] = incl;
    __syncthreads();
    uint32_t pos = incl - cnt, sum = 0;
    for (uint32_t w = 0; w < WAVES; w++) { if (w < wv) pos += wsum[w]; sum += wsum[w]; }
    *total = sum;
    return pos;
}

// The survive rule of the group kernels.  raw[0, n_total): every id at its rank; tags[]: the group tag of the id at that rank -
// the required groups are tags 0 .. n_req - 1, the excluded lists tag n_req; lists are in tag order, so the tags inside a run of
// equal ids ascend.  i is the head of a run (at most MAX_LISTS long: a list holds an id once): the id survives when every
// required tag occurs in the run (AT_LEAST: at least min_match of them) and its last tag is not the excluded one.  A repeated tag
// is counted once.
template <bool AT_LEAST>
__device__ __forceinline__ bool ss_group_run(const uint32_t *raw, const uint8_t *tags, uint32_t i, uint32_t n_total, uint32_t n_req, uint32_t min_match) {
    const uint32_t v = raw[i];
    uint32_t seen = 0, last = 0xFFFFFFFFu;
    for (uint32_t k = i; k < n_total && raw[k] == v; k++) {
        const uint32_t t = tags[k];
        seen += (t != last && t < n_req) ? 1u : 0u;
        last = t;
    }
    return (AT_LEAST ? seen >= min_match : seen == n_req) && last < n_req;
}
// in every required group (ii2_andnot_ranges, ii2_query_batch_groups) ...
__device__ __forceinline__ bool ss_group_run_kept(const uint32_t *raw, const uint8_t *tags, uint32_t i, uint32_t n_total, uint32_t n_req) {
    return ss_group_run<false>(raw, tags, i, n_total, n_req, 0u);
}
// ... or in at least min_match of them (ii2_atleast_ranges)
__device__ __forceinline__ bool ss_group_run_reaches(const uint32_t *raw, const uint8_t *tags, uint32_t i, uint32_t n_total, uint32_t n_req,
                                                     uint32_t min_match) {
    return ss_group_run<true>(raw, tags, i, n_total, n_req, min_match);
}

}  // namespace ii2
