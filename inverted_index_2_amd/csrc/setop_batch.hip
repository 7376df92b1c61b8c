// setop_batch.hip — many small AND / OR queries in one launch (ii2_query_batch): one workgroup per query.
// A single small query is one workgroup of k_setop_small (setop_small.hip) and a launch of its own: one of the card's 256
// CUs busy, the others idle, a launch (and for a synchronous call a stream wait) per query.  A search front end has
// thousands of such queries (PrefixSearch takes MANY prefixes, inverted_index.go:192); here they share one launch.
//
//   k_setop_batch   query blockIdx.x of its size class.  The algorithm is k_setop_small's single-workgroup form - decode
//                   every block into LDS one wave per block, rank every id by its position in its own list plus one
//                   bisection per other list, first-of-run / run-of-n_lists filter, tombstone test, block scan - with the
//                   query read from a device table (BatchQuery / BatchList) instead of a by-value parameter block, and in
//                   two sizes: 256 threads and a 2048-posting stage for the common tiny query (up to eight workgroups per
//                   CU), 1024 threads and 8192 postings for the rest.  The host bins the queries by size, so every launch
//                   has one workgroup shape.  The result goes to the query's slot of the batch's staging buffer (its size is
//                   the host-known bound of the result), the count to the query's word of the counts array.
//   k_batch_pack    after the scan of the counts: staging -> the caller's buffer, results back to back in query order.  It
//                   tests the total against the capacity itself and writes nothing when it does not fit, so it is enqueued
//                   before the call's one stream wait.
// No workgroup waits for another one anywhere: the order of the results comes from the scan between the two kernels.
#include <hip/hip_runtime.h>

#include "dv1_device.h"
#include "internal.h"

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
    // 1. decode: block b of the concatenated block list, one wave each (wave w: blocks w, w + WAVES, ...); every block of
    // a list but its last is full, so block bi of list j starts at raw[lpre[j] + 256 bi].  The skip entries of all the
    // wave's blocks are requested first, then the first 256 payload bytes of all of them, then they are decoded.
    uint32_t bj[PER_WAVE], q0[PER_WAVE], q1[PER_WAVE], f0[PER_WAVE], pw[PER_WAVE];
#pragma unroll
    for (uint32_t t = 0; t < PER_WAVE; t++) {
        const uint32_t b = wv + t * WAVES;
        bj[t] = 0xFFFFFFFFu; q0[t] = 0; q1[t] = 0; f0[t] = 0;
        if (b < n_blocks) {
            const uint32_t j = blist[b];                                  // (wave-uniform)
            const ii2_skip *sk = lskip[j] + (b - lbase[j]);
            const ii2_skip e0 = sk[0], e1 = sk[1];
            bj[t] = j; q0[t] = e0.byte_off; q1[t] = e1.byte_off; f0[t] = e0.first_doc;
        }
    }
#pragma unroll
    for (uint32_t t = 0; t < PER_WAVE; t++) {
        pw[t] = 0;
        if (bj[t] != 0xFFFFFFFFu && q0[t] + 4u * l < q1[t]) pw[t] = load_u32_unaligned(lpay[bj[t]] + q0[t] + 4u * l);
    }
#pragma unroll
    for (uint32_t t = 0; t < PER_WAVE; t++) {
        if (bj[t] == 0xFFFFFFFFu) continue;                               // (wave-uniform)
        const uint32_t b = wv + t * WAVES, j = bj[t];
        const uint32_t at = lpre[j] + (b - lbase[j]) * II2_DV1_BLOCK, end = lpre[j + 1u];
        const uint8_t *pl = lpay[j];
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
    uint32_t rk[PER_THREAD], xv[PER_THREAD];
#pragma unroll 4
    for (uint32_t q = 0; q < PER_THREAD; q++) {
        const uint32_t e = tid + q * THREADS;
        rk[q] = 0xFFFFFFFFu;
        xv[q] = 0;
        if (e >= n_total) continue;
        uint32_t j = 0;                                                   // my list: the last j with lpre[j] <= e
        for (uint32_t st = 32u; st > 0u; st >>= 1) if (j + st < n_lists && lpre[j + st] <= e) j += st;
        const uint32_t i = e - lpre[j];
        const uint32_t x = raw[lpre[j] + i];
        uint32_t r = i;
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
    }
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
            if (keep && p.tomb && (v >> 5) < p.tomb_nwords) keep = ((p.tomb[v >> 5] >> (v & 31u)) & 1u) == 0u;
            if (keep) { keepmask |= 1u << q; cnt++; }
        }
    }
    const uint32_t incl = wave_incl_scan(cnt);
    if (l == 63u) wsum[wv] = incl;
    __syncthreads();
    uint32_t pos = incl - cnt, total = 0;
    for (uint32_t w = 0; w < WAVES; w++) { if (w < wv) pos += wsum[w]; total += wsum[w]; }
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

hipError_t launch_setop_batch(const BatchParams &p, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (ev0) (void)hipEventRecord(ev0, s);
    if (p.n_tiny)
        hipLaunchKernelGGL((k_setop_batch<256u, BATCH_TINY_POSTINGS, BATCH_TINY_BLOCKS>), dim3(p.n_tiny), dim3(256), 0, s, p, 0u);
    if (p.n_small)
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
