// seg_build.hip — ii2_seg_build: one segment from unordered (list, value) pairs (gfx950, wave64).
//
// The bulk form of Shard.Put (reference shard.go:33-67) followed by the merges that fold the Puts' direct segments
// (shard.go:163-212): every pair becomes the 64-bit key list_id << 32 | value, the keys are sorted by a hand-written
// least-significant-digit radix sort (8-bit digits, only the digits that can differ), equal neighbours are dropped, the
// list offsets are looked up and the two-pass DV1 encoder of api.cpp writes the segment.  No library (scan.hip is the
// precedent), and NO WORKGROUP EVER WAITS FOR ANOTHER: each radix pass is the classic three steps on the context's
// stream, ordered by the stream alone.  The parts of a pass that ii2_dict_build's sort of (key, index) pairs runs as well - the
// digit counting, the wave's ballot ranking, the digit scan of the tile, the staging slot - live in radix_device.h.
//
//   k_sb_hist      one workgroup per tile of SB_TILE keys: per-wave digit counts in LDS, the tile's 256 counts stored
//                  digit-major (count[digit * n_tiles + tile]), so ONE exclusive scan of the table (scan_excl_u32) gives
//                  every (tile, digit) its global base.  The first pass also forms the keys from the caller's two arrays
//                  and notes a list_id >= n_lists (k_sb_pack fused into it: the pairs are read once).
//   k_sb_scatter   the workgroup ranks its tile's keys STABLY by digit and moves them: keys in registers, wave w owning
//                  keys [1024 w, 1024 (w + 1)) of the tile with item j of lane l at 1024 w + 64 j + l, so that loads are
//                  coalesced and "item, then lane" is the tile's order inside a wave.  Per item the lanes with the same
//                  digit find each other by eight ballots over the digit's bits; the match mask gives the rank among
//                  them, a per-wave LDS counter the rank among the wave's earlier items.  Wave bases come from the LDS
//                  table, tile bases from the scanned count table.  The keys go through LDS in digit order: a wave's
//                  global stores are then runs of consecutive addresses per digit, not 64 scattered 8-byte stores.
//   k_sb_heads     head flag = key[i] != key[i - 1] (a tile's first key reads its predecessor from global memory); run
//                  once to count the heads per tile, and - after a scan of those counts - again to compact the unique
//                  keys: low words into d_values, high words into d_ulist.
//   k_sb_offsets   one thread per list t: post_off[t] = lower_bound(d_ulist, t) - no walk over the gaps between non-empty
//                  lists - and the count of non-empty lists.
// One readback (unique keys, non-empty lists, the bad-id word) and with it one wait, then the encoder.
#include <algorithm>

#include "radix_device.h"

namespace ii2 {

// control words of one call in the context's mailbox (u64 each)
constexpr uint32_t SB_CTL_UNIQUE = 0, SB_CTL_NONEMPTY = 1, SB_CTL_BAD = 2, SB_CTL_WORDS = 3;

// PACK (first pass): key[i] = list_id[i] << 32 | values[i] is formed, stored and counted; a list_id >= n_lists leaves
// n - i in ctl[SB_CTL_BAD] (the largest wins: the first bad pair).  Otherwise the keys are read.
template <bool PACK>
__global__ __launch_bounds__(SB_THREADS) void k_sb_hist(const uint32_t *__restrict__ list_id, const uint32_t *__restrict__ values, uint64_t *keys,
                                                        uint64_t n, uint32_t n_tiles, uint32_t shift, uint32_t n_lists, uint32_t *__restrict__ count,
                                                        unsigned long long *ctl) {
    __shared__ uint32_t wcnt[SB_WAVES][SB_DIGITS];
    const uint32_t tid = threadIdx.x, w = tid >> 6;
    for (uint32_t k = 0; k < SB_WAVES; k++) wcnt[k][tid] = 0;
    __syncthreads();
    const uint64_t tile0 = (uint64_t)blockIdx.x * SB_TILE;
#pragma unroll 4
    for (uint32_t j = 0; j < SB_ITEMS; j++) {
        const uint64_t i = tile0 + (uint64_t)j * SB_THREADS + tid;
        const bool valid = i < n;
        uint64_t key = 0;
        if (valid) {
            if (PACK) {
                const uint32_t t = list_id[i];
                key = (uint64_t)t << 32 | values[i];
                keys[i] = key;
                if (t >= n_lists) atomicMax(&ctl[SB_CTL_BAD], (unsigned long long)(n - i));
            } else {
                key = keys[i];
            }
        }
        sb_hist_count(wcnt[w], sb_digit(key, shift), valid);
    }
    __syncthreads();
    sb_hist_store(wcnt, n_tiles, count);
}

__global__ __launch_bounds__(SB_THREADS) void k_sb_scatter(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, uint64_t n, uint32_t n_tiles,
                                                           uint32_t shift, const uint32_t *__restrict__ base) {
    __shared__ uint64_t stage[SB_TILE];
    __shared__ uint32_t wcnt[SB_WAVES][SB_DIGITS];      // per wave and digit: keys so far, then the wave's first slot of the digit in `stage`
    __shared__ uint32_t goff[SB_DIGITS];                // global index of stage slot s of digit d = goff[d] + s
    __shared__ uint32_t wsum[SB_WAVES];
    const uint32_t tid = threadIdx.x, w = tid >> 6, l = tid & 63u;
    const uint64_t tile0 = (uint64_t)blockIdx.x * SB_TILE;
    const uint32_t nv = n - tile0 < SB_TILE ? (uint32_t)(n - tile0) : SB_TILE;      // keys of this tile
    for (uint32_t k = 0; k < SB_WAVES; k++) wcnt[k][tid] = 0;
    uint64_t key[SB_ITEMS];
    uint32_t rank[SB_ITEMS];
#pragma unroll
    for (uint32_t j = 0; j < SB_ITEMS; j++) {
        const uint32_t loc = w * SB_WAVE_KEYS + j * 64u + l;
        key[j] = loc < nv ? in[tile0 + loc] : 0ull;
    }
    __syncthreads();
    const uint64_t lt = (1ull << l) - 1ull;
#pragma unroll
    for (uint32_t j = 0; j < SB_ITEMS; j++) rank[j] = sb_wave_rank(sb_digit(key[j], shift), w * SB_WAVE_KEYS + j * 64u + l < nv, wcnt[w], l, lt);
    __syncthreads();
    sb_tile_bases(wcnt, goff, wsum, base, n_tiles);
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < SB_ITEMS; j++) {
        const bool valid = w * SB_WAVE_KEYS + j * 64u + l < nv;
        if (valid) stage[sb_stage_slot(wcnt, w, sb_digit(key[j], shift), rank[j])] = key[j];
    }
    __syncthreads();
    for (uint32_t s = tid; s < nv; s += SB_THREADS) {
        const uint64_t k = stage[s];
        out[goff[sb_digit(k, shift)] + s] = k;
    }
}

// WRITE == false: cnt[tile] = unique keys that start in the tile.  WRITE == true: cnt holds the exclusive scan of those counts and
// unique key r goes to ulist[r] (its list) / values[r] (its value).
template <bool WRITE>
__global__ __launch_bounds__(SB_THREADS) void k_sb_heads(const uint64_t *__restrict__ keys, uint64_t n, uint32_t *cnt, uint32_t *__restrict__ ulist,
                                                         uint32_t *__restrict__ values) {
    __shared__ uint32_t wsum[SB_WAVES];
    const uint32_t tid = threadIdx.x, w = tid >> 6, l = tid & 63u;
    const uint64_t wave0 = (uint64_t)blockIdx.x * SB_TILE + (uint64_t)w * SB_WAVE_KEYS;
    const uint64_t lt = (1ull << l) - 1ull;
    uint64_t key[WRITE ? SB_ITEMS : 1];
    uint32_t pos[WRITE ? SB_ITEMS : 1];
    uint32_t run = 0;      // heads of this wave so far (wave-uniform)
#pragma unroll
    for (uint32_t j = 0; j < SB_ITEMS; j++) {
        const uint64_t i = wave0 + j * 64u + l;
        const bool valid = i < n;
        const uint64_t k = valid ? keys[i] : 0ull;
        uint64_t prev = (uint64_t)__shfl_up((unsigned long long)k, 1, 64);
        if (l == 0 && valid && i > 0) prev = keys[i - 1];
        const bool head = valid && (i == 0 || k != prev);
        const uint64_t m = __ballot(head);
        if (WRITE) {
            key[j] = k;
            pos[j] = head ? run + (uint32_t)__popcll(m & lt) : 0xFFFFFFFFu;
        }
        run += (uint32_t)__popcll(m);
    }
    if (l == 0) wsum[w] = run;
    __syncthreads();
    if (!WRITE) {
        if (tid == 0) {
            uint32_t t = 0;
            for (uint32_t k = 0; k < SB_WAVES; k++) t += wsum[k];
            cnt[blockIdx.x] = t;
        }
        return;
    }
    uint32_t at = cnt[blockIdx.x];
    for (uint32_t k = 0; k < SB_WAVES; k++)
        if (k < w) at += wsum[k];
#pragma unroll
    for (uint32_t j = 0; j < (WRITE ? SB_ITEMS : 1); j++) {
        if (pos[j] != 0xFFFFFFFFu) {
            ulist[at + pos[j]] = (uint32_t)(key[j] >> 32);
            values[at + pos[j]] = (uint32_t)key[j];
        }
    }
}

// thread t <= n_lists: post_off[t] = unique keys of lists < t.  ctl: the unique count for the host, the non-empty lists.
__global__ __launch_bounds__(SB_THREADS) void k_sb_offsets(const uint32_t *__restrict__ ulist, const uint32_t *__restrict__ n_unique, uint64_t n_lists,
                                                           uint64_t *__restrict__ post_off, unsigned long long *ctl) {
    const uint64_t t = (uint64_t)blockIdx.x * SB_THREADS + threadIdx.x;
    const uint32_t nu = *n_unique;
    bool nonempty = false;
    if (t <= n_lists) {
        uint32_t lo = 0, hi = nu;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if ((uint64_t)ulist[mid] < t) lo = mid + 1; else hi = mid;
        }
        post_off[t] = lo;
        nonempty = t < n_lists && lo < nu && (uint64_t)ulist[lo] == t;
    }
    const uint64_t m = __ballot(nonempty);
    if (lane_id() == 0 && m) atomicAdd(&ctl[SB_CTL_NONEMPTY], (unsigned long long)__popcll(m));
    if (t == 0) ctl[SB_CTL_UNIQUE] = nu;
}

}  // namespace ii2

using namespace ii2;

namespace {
uint32_t bit_width64(uint64_t x) { return x ? 64u - (uint32_t)__builtin_clzll((unsigned long long)x) : 0u; }
}  // namespace

extern "C" int ii2_seg_build(ii2_ctx *ctx, uint64_t n_lists, uint64_t n_pairs, const uint32_t *list_id, const uint32_t *values, int where,
                             ii2_seg **out, ii2_build_stats *stats) {
    if (!ctx || !out || (where != II2_HOST && where != II2_DEVICE)) return fail(ctx, II2_EINVAL, "ii2_seg_build: bad argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *out = nullptr;
    if (n_pairs >= (1ull << 32)) return fail(ctx, II2_ERANGE, "ii2_seg_build: 2^32 pairs or more; split the input");
    if (n_lists >= (1ull << 31)) return fail(ctx, II2_ERANGE, "ii2_seg_build: 2^31 lists or more");
    if (n_pairs && n_lists == 0) return fail(ctx, II2_EINVAL, "ii2_seg_build: pairs but no list");
    if (n_pairs && (!list_id || !values)) return fail(ctx, II2_EINVAL, "ii2_seg_build: list_id or values is NULL");
    hipStream_t st = ctx->stream;
    const uint64_t n = n_pairs;
    const size_t n_tiles = (size_t)((n + SB_TILE - 1) / SB_TILE);
    const uint32_t n_passes = n ? (32u + bit_width64(n_lists - 1) + 7u) / 8u : 0u;

    // The encoder reserves the context's workspace, which moves when it grows: the sort's arrays, d_post_off and d_values
    // live in a block of their own (size-class cache: a stream of calls allocates once), carved like the workspace.
    const size_t key_words = align_up((size_t)n, 64);           // (keeps the halves of a key buffer 256-byte aligned)
    const size_t tmpb = scan_temp_bytes(std::max<size_t>(SB_DIGITS * n_tiles, n_tiles + 1));
    const size_t sz_keys = align_up(key_words * sizeof(uint64_t)), sz_count = align_up(SB_DIGITS * n_tiles * sizeof(uint32_t)),
                 sz_tcnt = align_up((n_tiles + 1) * sizeof(uint32_t)), sz_off = align_up((size_t)(n_lists + 1) * sizeof(uint64_t));
    BuildBlock blk(st);
    if (dm_alloc(&blk.p, 2 * sz_keys + sz_count + align_up(tmpb) + sz_tcnt + sz_off) != hipSuccess)
        return fail(ctx, II2_ENOMEM, "ii2_seg_build: device allocation failed");
    uint8_t *at = (uint8_t *)blk.p;
    uint64_t *d_a = (uint64_t *)at; at += sz_keys;
    uint64_t *d_b = (uint64_t *)at; at += sz_keys;
    uint32_t *d_count = (uint32_t *)at; at += sz_count;
    void *d_tmp = at; at += align_up(tmpb);
    uint32_t *d_tcnt = (uint32_t *)at; at += sz_tcnt;
    uint64_t *d_post_off = (uint64_t *)at;

    uint64_t n_unique = 0, n_nonempty = 0;
    const uint32_t *d_values = (const uint32_t *)d_a;
    if (n == 0) {
        HIP_TRY(ctx, hipMemsetAsync(d_post_off, 0, (size_t)(n_lists + 1) * sizeof(uint64_t), st));
    } else {
        unsigned long long *d_ctl = (unsigned long long *)(ctx->d_mail + II2_MAIL_BUILD);
        HIP_TRY(ctx, hipMemsetAsync(d_ctl, 0, SB_CTL_WORDS * sizeof(uint64_t), st));
        const uint32_t *d_lid = list_id, *d_val = values;
        if (where == II2_HOST) {      // staged in the second key buffer: the first pass reads it before any key is stored there
            uint32_t *stage = (uint32_t *)d_b;
            HIP_TRY(ctx, hipMemcpyAsync(stage, list_id, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemcpyAsync(stage + key_words, values, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            d_lid = stage;
            d_val = stage + key_words;
        }
        const dim3 grid((unsigned)n_tiles), block(SB_THREADS);
        uint64_t *src = d_a, *dst = d_b;
        for (uint32_t p = 0; p < n_passes; p++) {
            const uint32_t shift = 8u * p;
            if (p == 0)
                hipLaunchKernelGGL(k_sb_hist<true>, grid, block, 0, st, d_lid, d_val, src, n, (uint32_t)n_tiles, shift, (uint32_t)n_lists, d_count, d_ctl);
            else
                hipLaunchKernelGGL(k_sb_hist<false>, grid, block, 0, st, (const uint32_t *)nullptr, (const uint32_t *)nullptr, src, n, (uint32_t)n_tiles,
                                   shift, (uint32_t)n_lists, d_count, d_ctl);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, scan_excl_u32(d_tmp, tmpb, d_count, d_count, SB_DIGITS * n_tiles, st));
            hipLaunchKernelGGL(k_sb_scatter, grid, block, 0, st, (const uint64_t *)src, dst, n, (uint32_t)n_tiles, shift, (const uint32_t *)d_count);
            HIP_TRY(ctx, hipGetLastError());
            std::swap(src, dst);
        }
        // src: the sorted keys.  dst is free: its halves take the unique keys' lists and values
        uint32_t *d_ulist = (uint32_t *)dst, *d_uval = (uint32_t *)dst + key_words;
        HIP_TRY(ctx, hipMemsetAsync(d_tcnt + n_tiles, 0, sizeof(uint32_t), st));
        hipLaunchKernelGGL(k_sb_heads<false>, grid, block, 0, st, (const uint64_t *)src, n, d_tcnt, (uint32_t *)nullptr, (uint32_t *)nullptr);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, scan_excl_u32(d_tmp, tmpb, d_tcnt, d_tcnt, n_tiles + 1, st));
        hipLaunchKernelGGL(k_sb_heads<true>, grid, block, 0, st, (const uint64_t *)src, n, d_tcnt, d_ulist, d_uval);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_sb_offsets, dim3((unsigned)((n_lists + 1 + SB_THREADS - 1) / SB_THREADS)), block, 0, st, (const uint32_t *)d_ulist,
                           (const uint32_t *)(d_tcnt + n_tiles), n_lists, d_post_off, d_ctl);
        HIP_TRY(ctx, hipGetLastError());
        uint64_t *h_ctl = ctx->h_mail + II2_MAIL_BUILD;
        HIP_TRY(ctx, hipMemcpyAsync(h_ctl, d_ctl, SB_CTL_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (h_ctl[SB_CTL_BAD]) {
            ctx->err = "ii2_seg_build: list_id[" + std::to_string(n - h_ctl[SB_CTL_BAD]) + "] is >= n_lists (" + std::to_string(n_lists) + ")";
            return II2_EINVAL;
        }
        n_unique = h_ctl[SB_CTL_UNIQUE];
        n_nonempty = h_ctl[SB_CTL_NONEMPTY];
        d_values = d_uval;
    }
    ii2_seg *seg = nullptr;
    if (int rc = ii2_seg_encode_dev_unlocked(ctx, n_lists, d_post_off, d_values, n_unique, &seg)) return rc;
    *out = seg;
    if (stats) {
        stats->n_pairs = n_pairs;
        stats->n_postings = n_unique;
        stats->n_nonempty = n_nonempty;
        stats->n_passes = n_passes;
    }
    return II2_OK;
}
