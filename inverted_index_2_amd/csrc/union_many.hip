// union_many.hip — OR of any number of posting lists (ii2_union_ranges): the unit of work is the DV1 block, not the list,
// so the number of lists does not matter.  The lists come as ranges of consecutive lists of segments (a prefix is one run
// of terms in every sorted dictionary); range r owns the blocks [b0, b1) of its segment and the query's blocks are the
// ranges' blocks back to back (pre[r] = blocks of the ranges before r).  Per window of at most 2^30 docs:
//   1. k_um_mark: one wave per run of query blocks - every block decoded in registers, its ids staged in LDS and read
//      back 64 at a time in ascending order; lanes whose ids share a bitmap word are adjacent, a segmented OR leaves the
//      word's bits in the run's last lane, which issues the only atomicOr for that word (and, the same way, for the
//      word's bit in the summary: one bit per 64 words);
//   2. k_um_count: one wave per summary word (2048 bitmap words): popcount of words & ~tombstones over its set chunks;
//   3. scan.hip: exclusive scan of those counts (the last entry is the window's total);
//   4. k_um_compact: one wave per summary word again - the ids in ascending order at their offsets when the whole result
//      fits the caller's buffer, and in every case the words and summary words it read are zeroed.  The scratch is
//      all-zero between calls: no call clears its doc range.
// No kernel waits for another workgroup.
#include <hip/hip_runtime.h>

#include "dv1_device.h"
#include "internal.h"
#include "um_device.h"

namespace ii2 {

__device__ __forceinline__ uint32_t um_tomb(const UnionManyParams &p, uint32_t word) {
    return (p.tomb && word < p.tomb_nwords) ? p.tomb[word] : 0u;
}

__global__ __launch_bounds__(256) void k_um_mark(UnionManyParams p) {
    __shared__ uint32_t stage[4][II2_DV1_BLOCK];
    const uint32_t l = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t g0 = ((uint64_t)blockIdx.x * 4u + wv) * p.per_wave;
    if (g0 >= p.n_blocks) return;                                         // (wave-uniform; no workgroup barrier below)
    const uint32_t g1 = (uint32_t)(g0 + p.per_wave < p.n_blocks ? g0 + p.per_wave : p.n_blocks);
    uint32_t *s = stage[wv];
    uint32_t r = um_range_of(p.pre, p.n_ranges, (uint32_t)g0);
    UmRange R = p.ranges[r];
    uint32_t rbeg = p.pre[r], rend = p.pre[r + 1u];
    const uint64_t win_end = (uint64_t)p.win_lo + p.win_docs;            // one past the window's last doc
    uint32_t sink = 0;
    for (uint32_t g = (uint32_t)g0; g < g1; g++) {
        while (g >= rend) {
            r++;
            R = p.ranges[r];
            rbeg = rend;
            rend = p.pre[r + 1u];
        }
        const uint32_t b = R.b0 + (g - rbeg);
        const ii2_skip e0 = R.skip[b], e1 = R.skip[b + 1u];
        if (p.check_window) {        // several windows: a block whose docs miss this one is not decoded
            if ((uint64_t)e0.first_doc >= win_end) continue;
            const uint32_t j = R.blk_list[b];
            uint32_t up = 0xFFFFFFFFu;                                    // a bound of the block's last doc
            if (b + 1u < R.b1 && R.blk_list[b + 1u] == j) up = e1.first_doc;
            else if (j >= R.l0 && j < R.l1) up = R.last_doc[j];
            if (up < p.win_lo) continue;
        }
        const uint32_t n = decode_block_wave4(GlobalBytes{R.payload}, e0.byte_off, e1.byte_off, e0.first_doc,
                                              [&](uint32_t ix, uint32_t id0, uint32_t id1, uint32_t id2, uint32_t id3, uint32_t mask) {
                                                  if ((mask & 1u) && ix < II2_DV1_BLOCK) s[ix] = id0;
                                                  ix += mask & 1u;
                                                  if ((mask & 2u) && ix < II2_DV1_BLOCK) s[ix] = id1;
                                                  ix += (mask >> 1) & 1u;
                                                  if ((mask & 4u) && ix < II2_DV1_BLOCK) s[ix] = id2;
                                                  ix += (mask >> 2) & 1u;
                                                  if ((mask & 8u) && ix < II2_DV1_BLOCK) s[ix] = id3;
                                              });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");               // the wave's LDS writes before its reads of other lanes' ids
        const uint32_t m = n < II2_DV1_BLOCK ? n : II2_DV1_BLOCK;
        for (uint32_t k = 0; k < m; k += 64u) {                           // 64 consecutive postings per pass, ascending along the lanes
            const uint32_t i = k + l;
            const uint32_t id = i < m ? s[i] : 0u;
            const uint32_t rel = id - p.win_lo;
            const bool v = i < m && id >= p.win_lo && rel < p.win_docs;
            const uint32_t key = v ? rel >> 5 : 0xFFFFFFFFu;
            const uint32_t bits = seg_or(key, v ? 1u << (rel & 31u) : 0u);
            const uint32_t next = (uint32_t)__shfl_down((int)key, 1, 64);
            const uint32_t skey = v ? key >> 11 : 0xFFFFFFFFu;           // summary word of the bitmap word
            const uint32_t sbits = seg_or(skey, v ? 1u << ((key >> 6) & 31u) : 0u);
            const uint32_t snext = (uint32_t)__shfl_down((int)skey, 1, 64);
            if (p.no_atomics) {                                           // timing experiment: everything but the atomics
                sink ^= bits ^ sbits;
                continue;
            }
            if (v && (l == 63u || next != key)) atomicOr(&p.bitmap[key], bits);
            if (v && (l == 63u || snext != skey)) atomicOr(&p.summary[skey], sbits);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");               // reads done before the next block's writes
    }
    if (p.no_atomics && sink == 0x9E3779B9u) p.bounds[0] = sink;          // (keeps the experiment's work alive)
}

__global__ __launch_bounds__(256) void k_um_count(UnionManyParams p) {
    const uint32_t l = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * 4u;
    for (uint32_t sw = blockIdx.x * 4u + (threadIdx.x >> 6); sw <= p.n_sum; sw += n_waves) {
        if (sw == p.n_sum) {                                              // the scan's closing entry
            if (l == 0) p.cnt[sw] = 0;
            continue;
        }
        uint32_t bits = p.summary[sw], c = 0;
        while (bits) {
            const uint32_t chunk = (uint32_t)__builtin_ctz(bits);
            bits &= bits - 1u;
            const uint32_t wi = (sw * 32u + chunk) * 64u + l;
            c += (uint32_t)__popc(p.bitmap[wi] & ~um_tomb(p, p.win_lo / 32u + wi));
        }
        c = wave_sum(c);
        if (l == 0) p.cnt[sw] = c;
    }
}

__global__ __launch_bounds__(256) void k_um_compact(UnionManyParams p) {
    const uint32_t l = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * 4u;
    const uint64_t base = p.window ? p.run[p.window & 1u] : 0ull;        // ids of the windows before this one
    const uint64_t total = base + p.off[p.n_sum];
    const bool write = p.write && total <= p.out_cap;                     // all or nothing
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        p.run[(p.window + 1u) & 1u] = total;
        *p.d_count = total;
    }
    for (uint32_t sw = blockIdx.x * 4u + (threadIdx.x >> 6); sw < p.n_sum; sw += n_waves) {
        uint32_t bits = p.summary[sw];
        if (!bits) continue;
        uint64_t pos = base + p.off[sw];
        while (bits) {
            const uint32_t chunk = (uint32_t)__builtin_ctz(bits);
            bits &= bits - 1u;
            const uint32_t wi = (sw * 32u + chunk) * 64u + l;
            const uint32_t w = p.bitmap[wi];
            if (w) p.bitmap[wi] = 0u;
            uint32_t v = w & ~um_tomb(p, p.win_lo / 32u + wi);
            const uint32_t c = (uint32_t)__popc(v);
            const uint32_t incl = wave_incl_scan(c);
            if (write) {
                uint64_t at = pos + incl - c;
                const uint32_t doc0 = p.win_lo + wi * 32u;
                while (v) {
                    const uint32_t bit = (uint32_t)__builtin_ctz(v);
                    v &= v - 1u;
                    if (at < p.out_cap) p.out[at] = doc0 + bit;
                    at++;
                }
            }
            pos += wave_bcast(incl, 63);
        }
        if (l == 0) p.summary[sw] = 0u;
    }
}

// smallest first doc and largest last doc over the query's blocks (segments whose list spans are not mirrored on the host)
__global__ __launch_bounds__(256) void k_um_bounds(UnionManyParams p) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    if (g < p.n_blocks) {
        const uint32_t r = um_range_of(p.pre, p.n_ranges, g);
        const UmRange &R = p.ranges[r];
        const uint32_t b = R.b0 + (g - p.pre[r]);
        lo = R.skip[b].first_doc;
        const uint32_t j = R.blk_list[b];
        hi = (j >= R.l0 && j < R.l1) ? R.last_doc[j] : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, d, 64));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, d, 64));
    }
    if ((threadIdx.x & 63u) == 0) {
        atomicMin(&p.bounds[0], lo);
        atomicMax(&p.bounds[1], hi);
    }
}

hipError_t launch_union_many_bounds(const UnionManyParams &p, hipStream_t s) {
    hipLaunchKernelGGL(k_um_bounds, dim3((p.n_blocks + 255u) / 256u), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_union_many_mark(const UnionManyParams &p, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    const uint64_t waves = (p.n_blocks + (uint64_t)p.per_wave - 1u) / p.per_wave;
    if (ev0) (void)hipEventRecord(ev0, s);
    hipLaunchKernelGGL(k_um_mark, dim3((unsigned)((waves + 3u) / 4u)), dim3(256), 0, s, p);
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

hipError_t launch_union_many_count(const UnionManyParams &p, uint32_t grid, hipStream_t s) {
    hipLaunchKernelGGL(k_um_count, dim3(grid), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_union_many_compact(const UnionManyParams &p, uint32_t grid, hipStream_t s) {
    hipLaunchKernelGGL(k_um_compact, dim3(grid), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace ii2
