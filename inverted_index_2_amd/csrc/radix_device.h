// radix_device.h — the parts of one least-significant-digit radix pass (8-bit digits, 64-bit keys) that both device sorts
// run: ii2_seg_build's keys alone (seg_build.hip) and ii2_dict_build's (key, index) pairs (dict_build.hip).  A pass is three
// steps on one stream and NO WORKGROUP EVER WAITS FOR ANOTHER:
//   hist     one workgroup per tile of SB_TILE keys: per-wave digit counts in LDS, the tile's 256 counts stored digit-major
//            (count[digit * n_tiles + tile]), so ONE exclusive scan of the table (scan_excl_u32) gives every (tile, digit)
//            its global base (sb_hist_count / sb_hist_store);
//   scatter  the workgroup ranks its tile's keys STABLY by digit and moves them: wave w owns keys [1024 w, 1024 (w + 1)) of
//            the tile with item j of lane l at 1024 w + 64 j + l, so that loads are coalesced and "item, then lane" is the
//            tile's order inside a wave.  Per item the lanes with the same digit find each other by eight ballots over the
//            digit's bits; the match mask gives the rank among them, a per-wave LDS counter the rank among the wave's earlier
//            items (sb_wave_rank).  Wave bases come from the LDS table, tile bases from the scanned count table
//            (sb_tile_bases).  The keys go through LDS in digit order (slot sb_stage_slot): a wave's global stores are then
//            runs of consecutive addresses per digit, not 64 scattered stores.
// Also the host's block of device memory for one sort (BuildBlock).
#pragma once
#include "dv1_device.h"
#include "internal.h"

namespace ii2 {

constexpr uint32_t SB_THREADS = 256;
constexpr uint32_t SB_WAVES = SB_THREADS / 64;
constexpr uint32_t SB_ITEMS = 16;                           // keys per thread
constexpr uint32_t SB_TILE = SB_THREADS * SB_ITEMS;         // 4096 keys per workgroup
constexpr uint32_t SB_WAVE_KEYS = 64 * SB_ITEMS;            // consecutive keys of the tile one wave owns
constexpr uint32_t SB_DIGITS = 256;
static_assert(SB_DIGITS == SB_THREADS, "one thread per digit where the tile's counts are combined");

__device__ __forceinline__ uint32_t sb_digit(uint64_t key, uint32_t shift) { return (uint32_t)(key >> shift) & (SB_DIGITS - 1u); }

// exclusive scan of one u32 per thread over the 256 threads of a workgroup (wsum: SB_WAVES words of LDS)
__device__ __forceinline__ uint32_t sb_wg_excl_scan(uint32_t v, uint32_t *wsum) {
    const int l = lane_id(), w = (int)threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan(v);
    if (l == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t pre = 0;
    for (int k = 0; k < (int)SB_WAVES; k++)
        if (k < w) pre += wsum[k];
    return pre + incl - v;
}

// hist, one item of every lane: digit d counted in the wave's row of LDS counters.  The valid lanes are a prefix of the wave;
// a wave whose keys share the digit (high digits mostly do) adds once.
__device__ __forceinline__ void sb_hist_count(uint32_t *wave_cnt, uint32_t d, bool valid) {
    const uint64_t vm = __ballot(valid);
    if (vm == 0) return;
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
    if (__ballot(valid && d != d0) == 0) {
        if (lane_id() == 0) atomicAdd(&wave_cnt[d0], (uint32_t)__popcll(vm));
    } else if (valid) {
        atomicAdd(&wave_cnt[d], 1u);
    }
}

// hist, the end (after a barrier): thread d adds the waves' counts of digit d and stores the tile's, digit-major
__device__ __forceinline__ void sb_hist_store(const uint32_t (*wcnt)[SB_DIGITS], uint32_t n_tiles, uint32_t *__restrict__ count) {
    const uint32_t tid = threadIdx.x;
    uint32_t c = 0;
    for (uint32_t k = 0; k < SB_WAVES; k++) c += wcnt[k][tid];
    count[(size_t)tid * n_tiles + blockIdx.x] = c;
}

// scatter, the wave's ballot ranking of one item of every lane: the rank of this lane's key among the keys of its wave with
// the same digit d, this item's and the earlier items'.  my_cnt: the wave's row of LDS counters (zero before the first item),
// lt: the lanes below this one.
__device__ __forceinline__ uint32_t sb_wave_rank(uint32_t d, bool valid, volatile uint32_t *my_cnt, uint32_t l, uint64_t lt) {
    uint64_t m = __ballot(valid);
#pragma unroll
    for (uint32_t b = 0; b < 8; b++) {
        const bool bit = (d >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    // m: the valid lanes whose key has this lane's digit; the lowest of them keeps the wave's counter
    const int leader = m ? __ffsll((unsigned long long)m) - 1 : 0;
    uint32_t old = 0;
    if (valid && (int)l == leader) {
        old = my_cnt[d];
        my_cnt[d] = old + (uint32_t)__popcll(m);
    }
    old = (uint32_t)__shfl((int)old, leader, 64);
    const uint32_t rank = old + (uint32_t)__popcll(m & lt);
    __builtin_amdgcn_wave_barrier();      // (the next item's leaders read what this item's leaders stored)
    return rank;
}

// scatter, the digit scan of the tile (between two barriers): thread d finds where digit d starts in the tile (exclusive scan
// of the digit totals) and, from it, every wave's first slot of the digit in the staging array (left in wcnt) and the global
// index of the digit's slot s: goff[d] + s.
__device__ __forceinline__ void sb_tile_bases(uint32_t (*wcnt)[SB_DIGITS], uint32_t *goff, uint32_t *wsum, const uint32_t *__restrict__ base,
                                              uint32_t n_tiles) {
    const uint32_t tid = threadIdx.x;
    uint32_t c[SB_WAVES], tot = 0;
    for (uint32_t k = 0; k < SB_WAVES; k++) { c[k] = wcnt[k][tid]; tot += c[k]; }
    uint32_t at = sb_wg_excl_scan(tot, wsum);
    goff[tid] = base[(size_t)tid * n_tiles + blockIdx.x] - at;      // (u32 arithmetic: every index below is < n < 2^32)
    for (uint32_t k = 0; k < SB_WAVES; k++) { wcnt[k][tid] = at; at += c[k]; }
}

// scatter, the staging: where the key of digit d and rank `rank` of wave w goes in the tile's staging array
__device__ __forceinline__ uint32_t sb_stage_slot(const uint32_t (*wcnt)[SB_DIGITS], uint32_t w, uint32_t d, uint32_t rank) { return wcnt[w][d] + rank; }

// the device block of one sort call: handed back on every exit path, after the stream has passed whatever still reads or writes it
struct BuildBlock {
    hipStream_t stream;
    void *p = nullptr;
    explicit BuildBlock(hipStream_t s) : stream(s) {}
    ~BuildBlock() {
        if (!p) return;
        (void)hipStreamSynchronize(stream);
        dm_free(p);
    }
    BuildBlock(const BuildBlock &) = delete;
};

}  // namespace ii2
