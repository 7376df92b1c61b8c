// match_runs.h — what ii2_dict_match (dict_match.hip), ii2_dict_fuzzy (dict_fuzzy.hip) and ii2_dict_regex (dict_regex.hip) share: a workgroup of 256 threads takes
// 256 consecutive terms of ONE dictionary and every thread ends up with a 64-bit match word (bit p = pattern p).  From there on
// the two calls are one: the run starts and ends per workgroup (match_runs_tail, below), the two scans, k_match_offsets,
// k_match_place and the copies (match_runs_drive, defined once in dict_match.hip).  In front of the match word they are one as
// well: match_patterns_to_lds copies the parsed patterns, TermStage computes where the workgroup's terms lie, fills the LDS stage
// and reads a term - the thread's own or a neighbour across the workgroup's edge - for the caller's matcher; on the host
// match_call is the entry point but its parser, its launch and its stats.  How a term is matched is the caller's part: the
// kernels differ in it and in nothing else.
#pragma once
#include <cstdint>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "dv1_device.h"
#include "internal.h"

namespace ii2 {

constexpr uint32_t DM_THREADS = 256;
constexpr uint32_t DM_WAVES = DM_THREADS / 64;
// LDS stage of a workgroup's term bytes: 64 bytes per term on average
constexpr uint32_t MATCH_STAGE = 16384;
// the counters a call carries through the scans, one row of the two tables each: row 0 = {matched (pattern, term) pairs, workgroups
// that matched out of LDS}, row 1 (ii2_dict_fuzzy, ii2_dict_regex) = {pairs that passed the filters in front of the matcher, -}
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

// P parsed patterns of either call into the workgroup's LDS, word by word (no barrier: the caller's)
template <class Pattern> __device__ __forceinline__ void match_patterns_to_lds(Pattern *lp, const Pattern *__restrict__ pats, uint32_t P) {
    static_assert(sizeof(Pattern) % 4 == 0, "a parsed pattern is copied into LDS word by word");
    const uint32_t *src = (const uint32_t *)pats;
    uint32_t *dst = (uint32_t *)lp;
    for (uint32_t i = threadIdx.x; i < P * (uint32_t)(sizeof(Pattern) / 4); i += DM_THREADS) dst[i] = src[i];
}

// the same for patterns whose size is a multiple of 16 (ii2_dict_regex: 2.6 KB each), in 16-byte loads; lp and pats are 16-byte aligned
template <class Pattern> __device__ __forceinline__ void match_patterns_to_lds16(Pattern *lp, const Pattern *__restrict__ pats, uint32_t P) {
    static_assert(sizeof(Pattern) % 16 == 0, "a parsed pattern is copied into LDS in 16-byte loads");
    const uint4 *src = (const uint4 *)pats;
    uint4 *dst = (uint4 *)lp;
    for (uint32_t i = threadIdx.x; i < P * (uint32_t)(sizeof(Pattern) / 16); i += DM_THREADS) dst[i] = src[i];
}

// The term bytes of workgroup wg, which takes terms [t0, t1) of dictionary s: where they are and how a matcher reads them.  The
// stage (MATCH_STAGE bytes of the kernel's LDS) holds the workgroup's own terms when they fit (`staged`) - and the two neighbours
// across its edges as well when those fit too (`wide`).  The dictionary's bytes are 256-byte aligned and padded by 16: every
// 16-byte load from a multiple of 16 up to the one that covers the span's last byte stays inside.  All of this is
// workgroup-uniform.  The constructor fills the stage and holds no barrier: the caller's comes before the first own() or
// neighbour().  Both hand f(bytes, length) the term, f called on the stage's copy or on global memory - two calls, so that each
// keeps its address space.
struct TermStage {
    const uint64_t *__restrict__ off;
    const uint8_t *__restrict__ bytes;
    const uint8_t *stage;
    uint32_t t0, t1, tl;            // tl: the term before t0 (t0 itself at the dictionary's front)
    uint64_t a0;                    // the stage's first byte is bytes[a0]
    bool staged, wide, have_left, have_right;       // (no neighbour before a dictionary's first term or behind its last)

    __device__ __forceinline__ TermStage(const MatchDicts &d, uint32_t s, uint32_t wg, uint32_t stage_on, uint8_t *stage_lds)
        : off(d.off[s]), bytes(d.bytes[s]), stage(stage_lds) {
        const uint32_t n = d.n[s];
        t0 = (wg - d.wg_first[s]) * DM_THREADS;                 // t0 < n
        t1 = min(t0 + DM_THREADS, n);
        have_left = t0 > 0;
        have_right = t1 < n;
        tl = have_left ? t0 - 1u : t0;
        const uint32_t tr = have_right ? t1 + 1u : t1;
        const uint64_t b0 = off[t0], b1 = off[t1], bl = off[tl], br = off[tr];
        staged = stage_on && b1 - (b0 & ~15ull) <= MATCH_STAGE;
        wide = staged && br - (bl & ~15ull) <= MATCH_STAGE;
        a0 = (wide ? bl : b0) & ~15ull;
        const uint64_t a1 = wide ? br : b1;
        if (staged)
            for (uint64_t i = (uint64_t)threadIdx.x * 16u; a0 + i < a1; i += DM_THREADS * 16u)
                *(uint4 *)(stage_lds + i) = *(const uint4 *)(bytes + a0 + i);
    }
    template <class F> __device__ __forceinline__ auto read(uint32_t t, bool from_stage, F f) const {
        const uint64_t b = off[t], len = off[t + 1] - b;
        return from_stage ? f(stage + (b - a0), len) : f(bytes + b, len);
    }
    // the thread's own term t, t0 <= t < t1
    template <class F> __device__ __forceinline__ auto own(uint32_t t, F f) const { return read(t, staged, f); }
    // the term before t0 (right == 0) or at t1 (right != 0), where there is one
    template <class F> __device__ __forceinline__ auto neighbour(uint32_t right, F f) const { return read(right ? t1 : tl, wide, f); }
};

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

// The whole of an entry point but its matcher, for both calls.  `in` is what the ABI hands over (pat_arg: the call's own
// per-pattern array that must not be NULL); `t` the call's name, its pattern limit and its three texts of its own.  In the order
// of the ABI's contract: the argument checks, ctx->mu, the dictionaries into MatchDicts, pat_off, parse(p, bytes, len, &pattern)
// for every pattern (II2_ERANGE: t.too_long, any other error: t.unparsed); with no pattern or no term run_off and *stats are
// zeroed, stats->n_terms is set and sums->n_wg stays 0; else match_runs_drive with n_rows counter rows, the parsed patterns
// uploaded and launch(md, device patterns, n_wg, words, tab_st, tab_en) starting the kernel on ctx->stream.  Returns what
// match_runs_drive returns; on II2_OK and II2_ECAPACITY *sums is filled, and the caller's stats are the caller's to fill.
struct MatchCallIn {
    uint32_t k;
    const ii2_dict *const *dicts;
    uint32_t n_patterns;
    const uint8_t *pat_bytes;
    const uint64_t *pat_off;
    const void *pat_arg;
};
struct MatchCallTexts {
    const char *name;
    uint32_t max_patterns;
    const char *too_many, *too_long, *unparsed;
};
struct MatchSums {
    uint64_t n_terms = 0, n_runs = 0, counters[2 * MATCH_MAX_ROWS] = {};
    uint32_t n_wg = 0;              // the workgroups launched: 0 when there was nothing to scan
};
template <class Pattern, class Stats, class Parse, class Launch>
int match_call(ii2_ctx *ctx, const MatchCallTexts &t, const MatchCallIn &in, const MatchRunsOut &out, Stats *stats, uint32_t n_rows, Parse parse,
               Launch launch, MatchSums *sums) {
    const auto bad = [&](int code, const char *what) {
        if (ctx) ctx->err = std::string(t.name) + ": " + what;
        return code;
    };
    const uint32_t k = in.k, n_patterns = in.n_patterns;
    if (!ctx || !in.dicts || k == 0 || k > II2_MAX_LISTS) return bad(II2_EINVAL, "bad argument");
    if (n_patterns > t.max_patterns) return fail(ctx, II2_ERANGE, t.too_many);
    if (n_patterns && (!in.pat_bytes || !in.pat_off || !in.pat_arg || !out.run_off || (out.cap && (!out.run_first || !out.run_end))))
        return bad(II2_EINVAL, "an array is NULL");
    std::lock_guard<std::mutex> g(ctx->mu);
    MatchDicts md;
    std::memset(&md, 0, sizeof md);
    md.k = k;
    md.n_patterns = n_patterns;
    for (uint32_t s = 0; s < k; s++) {
        const ii2_dict *dict = in.dicts[s];
        if (!dict || dict->device != ctx->device) return bad(II2_EINVAL, "a dictionary is NULL or lives on another device");
        if (dict->n >= (1ull << 31)) return bad(II2_ERANGE, "a dictionary of 2^31 or more terms");
        md.off[s] = dict->d_off; md.bytes[s] = dict->d_bytes;
        md.n[s] = (uint32_t)dict->n;
        md.wg_first[s + 1] = md.wg_first[s] + (md.n[s] + DM_THREADS - 1) / DM_THREADS;
        md.term_first[s + 1] = md.term_first[s] + md.n[s];
    }
    std::vector<Pattern> pats(n_patterns);
    for (uint32_t p = 0; p < n_patterns; p++) {
        if (in.pat_off[0] != 0 || in.pat_off[p + 1] < in.pat_off[p]) return bad(II2_EINVAL, "pat_off must start at 0 and be non-decreasing");
        const int rc = parse(p, in.pat_bytes + in.pat_off[p], in.pat_off[p + 1] - in.pat_off[p], &pats[p]);
        if (rc) return fail(ctx, rc, rc == II2_ERANGE ? t.too_long : t.unparsed);
    }
    const uint32_t n_wg = md.wg_first[k];
    sums->n_terms = md.term_first[k];
    if (n_patterns == 0 || n_wg == 0) {        // nothing to scan: no pattern, or no term in any dictionary
        for (uint64_t i = 0; out.run_off && i <= (uint64_t)n_patterns * k; i++) out.run_off[i] = 0;
        if (stats) { std::memset(stats, 0, sizeof *stats); stats->n_terms = n_patterns ? sums->n_terms : 0; }
        return II2_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = match_runs_drive(ctx, t.name, md, n_rows, n_patterns * sizeof(Pattern),
                                    [&](void *head, uint64_t *d_words, uint32_t *d_tab_st, uint32_t *d_tab_en) -> int {
        HIP_TRY(ctx, hipMemcpyAsync(head, pats.data(), n_patterns * sizeof(Pattern), hipMemcpyHostToDevice, ctx->stream));
        launch(md, (const Pattern *)head, n_wg, d_words, d_tab_st, d_tab_en);
        HIP_TRY(ctx, hipGetLastError());
        return II2_OK;
    }, out, &sums->n_runs, sums->counters);
    if (rc == II2_OK || rc == II2_ECAPACITY) sums->n_wg = n_wg;
    return rc;
}

}  // namespace ii2
