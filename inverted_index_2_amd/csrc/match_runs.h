// match_runs.h — what ii2_dict_match (dict_match.hip) and ii2_dict_fuzzy (dict_fuzzy.hip) share: a workgroup of 256 threads takes
// 256 consecutive terms of ONE dictionary and every thread ends up with a 64-bit match word (bit p = pattern p).  From there on
// the two calls are one: the run starts and ends per workgroup (match_runs_tail, below), the two scans, k_match_offsets,
// k_match_place and the copies (match_runs_drive, defined once in dict_match.hip).  How a term is matched is the caller's part:
// the kernels differ in it and in nothing else.
#pragma once
#include <cstdint>
#include <functional>

#include "dv1_device.h"
#include "internal.h"

namespace ii2 {

constexpr uint32_t DM_THREADS = 256;
constexpr uint32_t DM_WAVES = DM_THREADS / 64;
// LDS stage of a workgroup's term bytes: 64 bytes per term on average
constexpr uint32_t MATCH_STAGE = 16384;
// the counters a call carries through the scans, one row of the two tables each: row 0 = {matched (pattern, term) pairs, workgroups
// that matched out of LDS}, row 1 (ii2_dict_fuzzy) = {pairs that ran the recurrence, -}
constexpr uint32_t MATCH_MAX_ROWS = 2;

struct MatchDicts {
    const uint64_t *off[MAX_LISTS];
    const uint8_t *bytes[MAX_LISTS];
    uint32_t n[MAX_LISTS];
    uint32_t wg_first[MAX_LISTS + 1];     // workgroups of the dictionaries before s: ceil(n / 256) each
    uint64_t term_first[MAX_LISTS + 1];   // terms of the dictionaries before s: where its match words start
    uint32_t k;
    uint32_t n_patterns;
};

// the dictionary of workgroup wg: the last s with wg_first[s] <= wg (dictionaries without terms have no workgroup)
__device__ __forceinline__ uint32_t match_dict_of(const MatchDicts &d, uint32_t wg) {
    uint32_t lo = 0, hi = d.k;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (d.wg_first[mid] <= wg) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint64_t wave_or64(uint64_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x |= (uint64_t)__shfl_xor((unsigned long long)x, o, 64);
    return x;
}

// Per pattern the run starts and run ends among this wave's lanes: lane p of the wave keeps pattern p's two counts.  The loop
// runs over the patterns that have a start or an end in the wave at all (wave-uniform).
__device__ __forceinline__ void wave_run_counts(uint64_t st, uint64_t en, uint32_t *n_st, uint32_t *n_en) {
    const uint32_t l = (uint32_t)lane_id();
    uint32_t cs = 0, ce = 0;
    for (uint64_t live = wave_or64(st | en); live; live &= live - 1ull) {
        const uint32_t p = (uint32_t)__builtin_ctzll(live);
        const uint32_t a = (uint32_t)__popcll(__ballot((st >> p) & 1ull)), b = (uint32_t)__popcll(__ballot((en >> p) & 1ull));
        if (l == p) { cs = a; ce = b; }
    }
    *n_st = cs;
    *n_en = ce;
}

// The part of a matching kernel behind "the match word is known": thread tid of workgroup wg holds m, the match word of its term
// (0 behind the dictionary's last term).  tab_st / tab_en[p * n_wg + wg] = the workgroup's run starts (m[i] && !m[i - 1]) / run
// ends (m[i] && !m[i + 1]) of pattern p, counted with one ballot per wave and only for the patterns some lane of the wave has a
// start or an end of.  The neighbours across the workgroup's edges are matched again here, not fetched from their workgroups:
// wave 0 takes the term before the workgroup's first (have_left), wave 1 the term behind its last (have_right), lane p pattern
// p - neighbour(right ? 1 : 0, p) says whether pattern p matches that term - and the wave's ballot is the neighbour's match
// word: one pattern per lane instead of all of them for the thread at the edge.
// Rows P .. P + ROWS - 1 of the two tables carry the call's counters through the same scans, so that no workgroup touches a
// shared word (3907 atomics on one word took longer than the matching of one pattern): tab_st[P * n_wg + wg] = its matched
// (pattern, term) pairs, tab_en[P * n_wg + wg] = 1 when it matched out of LDS, and with ROWS == 2 tab_st[(P + 1) * n_wg + wg] =
// the sum of the threads' `extra` (tab_en of that row: 0).
template <uint32_t ROWS, class Neighbour>
__device__ __forceinline__ void match_runs_tail(uint32_t P, uint32_t wg, uint32_t n_wg, bool have_left, bool have_right, uint64_t m, uint32_t extra,
                                                bool staged, Neighbour neighbour, uint32_t *__restrict__ tab_st, uint32_t *__restrict__ tab_en) {
    static_assert(ROWS >= 1 && ROWS <= MATCH_MAX_ROWS, "one or two counter rows");
    __shared__ uint64_t lw[DM_THREADS + 2];                 // lw[1 + i] = word of the workgroup's term i; lw[0] / lw[257] the neighbours outside
    __shared__ uint32_t wcnt[DM_WAVES][2][64];
    __shared__ uint32_t wsum[ROWS][DM_WAVES];
    const uint32_t tid = threadIdx.x, l = (uint32_t)lane_id(), wv = tid >> 6;
    lw[1 + tid] = m;
    if (wv < 2u) {
        const bool have = wv == 0 ? have_left : have_right;
        bool hit = false;
        if (have && l < P) hit = neighbour(wv, l);
        const uint64_t w = __ballot(hit);
        if (l == 0) lw[wv == 0 ? 0 : DM_THREADS + 1] = w;
    }
    __syncthreads();
    const uint64_t st = m & ~lw[tid], en = m & ~lw[tid + 2];      // (a thread behind the last term has m = 0; the one at the last term sees 0 after it)
    uint32_t cs, ce;
    wave_run_counts(st, en, &cs, &ce);
    wcnt[wv][0][l] = cs;
    wcnt[wv][1][l] = ce;
    uint32_t mine = (uint32_t)__popcll(m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
    if (l == 0) wsum[0][wv] = mine;
    if (ROWS > 1) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) extra += __shfl_down(extra, o, 64);
        if (l == 0) wsum[ROWS - 1][wv] = extra;
    }
    __syncthreads();
    if (tid < 2u * 64u) {
        const uint32_t which = tid >> 6, p = tid & 63u;
        if (p < P) {
            uint32_t c = 0;
            for (uint32_t w = 0; w < DM_WAVES; w++) c += wcnt[w][which][p];
            (which ? tab_en : tab_st)[(uint64_t)p * n_wg + wg] = c;
        }
    }
    if (tid == DM_THREADS - 1) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < DM_WAVES; w++) all += wsum[0][w];
        tab_st[(uint64_t)P * n_wg + wg] = all;
        tab_en[(uint64_t)P * n_wg + wg] = staged ? 1u : 0u;
        if (ROWS > 1) {
            uint32_t ex = 0;
            for (uint32_t w = 0; w < DM_WAVES; w++) ex += wsum[ROWS - 1][w];
            tab_st[(uint64_t)(P + 1) * n_wg + wg] = ex;
            tab_en[(uint64_t)(P + 1) * n_wg + wg] = 0;
        }
    }
}

// The host driver's tail, for both calls (dict_match.hip).  ctx->mu is held, md is filled and holds at least one pattern and one
// workgroup.  It reserves the workspace - head_bytes for the caller's parsed patterns in front - and calls launch(head, words,
// tab_st, tab_en), which uploads the patterns and starts the matching kernel (its return code ends the call when non-zero).  Then
// the two scans, the offsets, the first wait; k_match_place and the second wait when the runs fit cap; and only then the caller's
// arrays are written.  counters[2 * r] / [2 * r + 1] = the totals of row r of tab_st / tab_en, r < n_rows.  Returns II2_OK, or
// II2_ECAPACITY with run_off and the counters filled and the run arrays untouched; `name` starts the error texts.
struct MatchRunsOut {
    uint64_t *run_off, *run_first, *run_end;
    uint32_t *run_dict;
    uint64_t cap;
};
using MatchLaunch = std::function<int(void *head, uint64_t *words, uint32_t *tab_st, uint32_t *tab_en)>;
int match_runs_drive(ii2_ctx *ctx, const char *name, const MatchDicts &md, uint32_t n_rows, size_t head_bytes, const MatchLaunch &launch,
                     const MatchRunsOut &out, uint64_t *n_runs, uint64_t *counters /* 2 * n_rows */);

}  // namespace ii2
