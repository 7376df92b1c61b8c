// dict_fuzzy.hip — typo-tolerant term search in resident dictionaries, hand-written: patterns and distances in, list ranges out,
// for every range entry point.
//
// The third way to resolve a term, beside ii2_dict_find (exact, prefix) and ii2_dict_match (substring, suffix, glob): every term
// within edit distance d of a pattern, what Lucene's FuzzyQuery and the reference's dictionary library (a Levenshtein automaton
// over the FST) answer.  As in dict_match.hip the dictionaries are read whole; the answer of pattern p in dictionary s (entry
// p * k + s) is the maximal runs of consecutive matching terms.
//
// k_dict_fuzzy<W> has k_dict_match's shape: a workgroup of 256 threads takes 256 consecutive terms of ONE dictionary, a thread per
// term, the terms' bytes staged into LDS in 16-byte loads where they fit MATCH_STAGE.  What differs is the matcher
// (fuzzy_device.h): a pattern holds at most 64 bytes, so a DP column is one word W and a term byte costs one LDS load of the
// pattern's table Peq[byte] and some 15 integer instructions.  The tables live in DYNAMIC LDS sized by the call, n_patterns * 256
// words, and are built by the workgroup from the parsed patterns - zeroed, then one bit ORed in per pattern position - instead of
// uploading up to 32 KB per call.  W is uint32_t when every pattern of the call holds at most 32 bytes (1 KB of table per
// pattern, half the VALU work: a 64-bit add is an add and an add-with-carry here, a 64-bit logic op two instructions), uint64_t
// otherwise or with option fuzzy.wide.  Behind the match word everything is ii2_dict_match's, shared through match_runs.h: the
// run starts and ends, the two scans, k_match_offsets, k_match_place; a second counter row carries n_tested.
#include <algorithm>
#include <cstring>
#include <vector>

#include "dv1_device.h"
#include "fuzzy_device.h"
#include "internal.h"
#include "match_runs.h"

namespace ii2 {

static_assert(II2_FUZZY_MAX_PATTERNS <= 64, "a match word is 64 bits, a wave's lane p counts pattern p");
static_assert(II2_FUZZY_MAX_PATTERN == 64, "a DP column is at most one 64-bit word");

__device__ __forceinline__ void lds_or(uint32_t *p, uint32_t v) { atomicOr(p, v); }
__device__ __forceinline__ void lds_or(uint64_t *p, uint64_t v) { atomicOr((unsigned long long *)p, (unsigned long long)v); }

// workgroup wg: terms [t0, t0 + 256) of its dictionary.  words[term_first[s] + t] = the match word of term t; the two tables and
// their two counter rows are match_runs_tail's (the second one: the pairs this workgroup's threads ran the recurrence for).
// Dynamic LDS: n_patterns * 256 * sizeof(W) bytes.
template <class W>
__global__ __launch_bounds__(DM_THREADS) void k_dict_fuzzy(MatchDicts d, const FuzzyPattern *__restrict__ pats, uint32_t stage_on, uint32_t n_wg,
                                                           uint64_t *__restrict__ words, uint32_t *__restrict__ tab_st, uint32_t *__restrict__ tab_en) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[MATCH_STAGE];
    __shared__ __attribute__((aligned(16))) FuzzyPattern lp[II2_FUZZY_MAX_PATTERNS];
    extern __shared__ __attribute__((aligned(16))) uint8_t fuzzy_peq_lds[];
    W *peq = (W *)fuzzy_peq_lds;                            // peq[p * 256 + c]: bit i <=> byte i of pattern p is c
    const uint32_t tid = threadIdx.x, wg = blockIdx.x;
    const uint32_t s = match_dict_of(d, wg), n = d.n[s], P = d.n_patterns;
    const uint64_t *__restrict__ off = d.off[s];
    const uint8_t *__restrict__ bytes = d.bytes[s];
    const uint32_t t0 = (wg - d.wg_first[s]) * DM_THREADS, t1 = min(t0 + DM_THREADS, n);      // t0 < n
    {       // the patterns: 72 bytes each, word by word; the tables: all zero first
        const uint32_t *src = (const uint32_t *)pats;
        uint32_t *dst = (uint32_t *)lp;
        for (uint32_t i = tid; i < P * (uint32_t)(sizeof(FuzzyPattern) / 4); i += DM_THREADS) dst[i] = src[i];
        for (uint32_t i = tid; i < P * 256u; i += DM_THREADS) peq[i] = 0;
    }
    // the stage, as in k_dict_match: the workgroup's own terms when they fit, the two neighbours across its edges as well when
    // those fit too (`wide`); 16-byte loads stay inside the dictionary's 16 bytes of padding
    const uint32_t tl = t0 > 0 ? t0 - 1u : t0, tr = t1 < n ? t1 + 1u : t1;
    const uint64_t b0 = off[t0], b1 = off[t1], bl = off[tl], br = off[tr];
    const bool staged = stage_on && b1 - (b0 & ~15ull) <= MATCH_STAGE;
    const bool wide = staged && br - (bl & ~15ull) <= MATCH_STAGE;
    const uint64_t a0 = (wide ? bl : b0) & ~15ull, a1 = wide ? br : b1;
    if (staged)
        for (uint64_t i = (uint64_t)tid * 16u; a0 + i < a1; i += DM_THREADS * 16u)
            *(uint4 *)(stage + i) = *(const uint4 *)(bytes + a0 + i);
    __syncthreads();
    // one bit per pattern position: thread i takes position i & 63 of pattern i >> 6
    for (uint32_t i = tid; i < P * II2_FUZZY_MAX_PATTERN; i += DM_THREADS) {
        const uint32_t p = i >> 6, j = i & 63u;
        if (j < lp[p].len) lds_or(&peq[p * 256u + lp[p].lit[j]], (W)1 << j);
    }
    __syncthreads();
    const uint32_t t = t0 + tid;
    uint64_t m = 0;
    uint32_t n_tested = 0;
    if (t < t1) {
        const uint64_t b = off[t], len = off[t + 1] - b;
        for (uint32_t p = 0; p < P; p++) {
            bool tested;
            const bool hit = staged ? fuzzy_term<W>(lp[p], peq + p * 256u, stage + (b - a0), len, &tested)
                                    : fuzzy_term<W>(lp[p], peq + p * 256u, bytes + b, len, &tested);
            if (hit) m |= 1ull << p;
            n_tested += tested ? 1u : 0u;
        }
        words[d.term_first[s] + t] = m;
    }
    // (no neighbour before a dictionary's first term or behind its last; the neighbours' pairs are not counted as tested)
    match_runs_tail<2>(P, wg, n_wg, t0 > 0, t1 < n, m, n_tested, staged, [&](uint32_t right, uint32_t p) {
        const uint32_t tn = right ? t1 : tl;
        const uint64_t b = off[tn], len = off[tn + 1] - b;
        bool tested;
        return wide ? fuzzy_term<W>(lp[p], peq + p * 256u, stage + (b - a0), len, &tested)
                    : fuzzy_term<W>(lp[p], peq + p * 256u, bytes + b, len, &tested);
    }, tab_st, tab_en);
}

}  // namespace ii2

using namespace ii2;

extern "C" {

int ii2_dict_fuzzy(ii2_ctx *ctx, uint32_t k, const ii2_dict *const *dicts, uint32_t n_patterns, const uint8_t *pat_bytes, const uint64_t *pat_off,
                   const uint8_t *pat_dist, const uint8_t *pat_prefix, const uint8_t *pat_flags, uint64_t *run_off, uint64_t *run_first,
                   uint64_t *run_end, uint32_t *run_dict, uint64_t cap, ii2_fuzzy_stats *stats) {
    if (!ctx || !dicts || k == 0 || k > II2_MAX_LISTS) return fail(ctx, II2_EINVAL, "ii2_dict_fuzzy: bad argument");
    if (n_patterns > II2_FUZZY_MAX_PATTERNS) return fail(ctx, II2_ERANGE, "ii2_dict_fuzzy: more than 16 patterns in one call");
    if (n_patterns && (!pat_bytes || !pat_off || !pat_dist || !run_off || (cap && (!run_first || !run_end))))
        return fail(ctx, II2_EINVAL, "ii2_dict_fuzzy: an array is NULL");
    std::lock_guard<std::mutex> g(ctx->mu);
    MatchDicts md;
    std::memset(&md, 0, sizeof md);
    md.k = k;
    md.n_patterns = n_patterns;
    for (uint32_t s = 0; s < k; s++) {
        if (!dicts[s] || dicts[s]->device != ctx->device) return fail(ctx, II2_EINVAL, "ii2_dict_fuzzy: a dictionary is NULL or lives on another device");
        if (dicts[s]->n >= (1ull << 31)) return fail(ctx, II2_ERANGE, "ii2_dict_fuzzy: a dictionary of 2^31 or more terms");
        md.off[s] = dicts[s]->d_off; md.bytes[s] = dicts[s]->d_bytes;
        md.n[s] = (uint32_t)dicts[s]->n;
        md.wg_first[s + 1] = md.wg_first[s] + (md.n[s] + DM_THREADS - 1) / DM_THREADS;
        md.term_first[s + 1] = md.term_first[s] + md.n[s];
    }
    std::vector<FuzzyPattern> pats(n_patterns);
    uint32_t longest = 0;
    if (n_patterns && pat_off[0] != 0) return fail(ctx, II2_EINVAL, "ii2_dict_fuzzy: pat_off must start at 0 and be non-decreasing");
    for (uint32_t p = 0; p < n_patterns; p++) {
        if (pat_off[p + 1] < pat_off[p]) return fail(ctx, II2_EINVAL, "ii2_dict_fuzzy: pat_off must start at 0 and be non-decreasing");
        const int rc = fuzzy_parse(pat_flags ? pat_flags[p] : 0u, pat_bytes + pat_off[p], pat_off[p + 1] - pat_off[p], pat_prefix ? pat_prefix[p] : 0u,
                                   pat_dist[p], &pats[p]);
        if (rc == II2_ERANGE) return fail(ctx, rc, "ii2_dict_fuzzy: a pattern of more than 64 bytes");
        if (rc) return fail(ctx, rc, "ii2_dict_fuzzy: an unknown flag, or a prefix longer than its pattern");
        longest = std::max<uint32_t>(longest, pats[p].len);
    }
    const uint64_t n_pairs = (uint64_t)n_patterns * k, n_terms = md.term_first[k];
    const uint32_t n_wg = md.wg_first[k];
    if (n_patterns == 0 || n_wg == 0) {        // nothing to scan: no pattern, or no term in any dictionary
        for (uint64_t i = 0; run_off && i <= n_pairs; i++) run_off[i] = 0;
        if (stats) { std::memset(stats, 0, sizeof *stats); stats->n_terms = n_patterns ? n_terms : 0; }
        return II2_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool narrow = longest <= 32u && !ctx->opt_fuzzy_wide;
    uint64_t n_runs = 0, counters[4] = {0, 0, 0, 0};    // {matched pairs, staged workgroups, tested pairs, -}
    const int rc = match_runs_drive(ctx, "ii2_dict_fuzzy", md, 2, n_patterns * sizeof(FuzzyPattern),
                                    [&](void *head, uint64_t *d_words, uint32_t *d_tab_st, uint32_t *d_tab_en) -> int {
        HIP_TRY(ctx, hipMemcpyAsync(head, pats.data(), n_patterns * sizeof(FuzzyPattern), hipMemcpyHostToDevice, st));
        const uint32_t stage_on = ctx->opt_fuzzy_stage ? 1u : 0u;
        if (narrow)
            hipLaunchKernelGGL(k_dict_fuzzy<uint32_t>, dim3(n_wg), dim3(DM_THREADS), n_patterns * 256u * sizeof(uint32_t), st, md, (const FuzzyPattern *)head,
                               stage_on, n_wg, d_words, d_tab_st, d_tab_en);
        else
            hipLaunchKernelGGL(k_dict_fuzzy<uint64_t>, dim3(n_wg), dim3(DM_THREADS), n_patterns * 256u * sizeof(uint64_t), st, md, (const FuzzyPattern *)head,
                               stage_on, n_wg, d_words, d_tab_st, d_tab_en);
        HIP_TRY(ctx, hipGetLastError());
        return II2_OK;
    }, MatchRunsOut{run_off, run_first, run_end, run_dict, cap}, &n_runs, counters);
    if (rc && rc != II2_ECAPACITY) return rc;
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->n_terms = n_terms;
        stats->n_matched = counters[0];
        stats->n_runs = n_runs;
        stats->n_tested = counters[2];
        stats->n_staged = (uint32_t)counters[1];
        stats->n_global = n_wg - stats->n_staged;
        stats->word_bits = narrow ? 32u : 64u;
    }
    return rc;
}

// host only: one pattern against one term, by the parse, the filters and the recurrence k_dict_fuzzy runs
int ii2_term_fuzzy(uint32_t flags, const uint8_t *pat, uint64_t pat_len, uint32_t prefix, uint32_t max_dist, const uint8_t *term, uint64_t term_len,
                   int *match, uint32_t *dist) {
    if (!match || (pat_len && !pat) || (term_len && !term)) return II2_EINVAL;
    FuzzyPattern m;
    const int rc = fuzzy_parse(flags, pat, pat_len, prefix, max_dist, &m);
    if (rc) return rc;
    bool tested, hit;
    uint64_t exact;
    if (m.len <= 32u) {          // the instance the kernel takes for a call of such patterns
        uint32_t peq[256];
        fuzzy_peq_build(m, peq);
        hit = fuzzy_term<uint32_t>(m, peq, term, term_len, &tested);
        exact = m.len ? fuzzy_distance<uint32_t>(peq, m.len, m.transpose != 0, m.nocase != 0, term, term_len) : term_len;
    } else {
        uint64_t peq[256];
        fuzzy_peq_build(m, peq);
        hit = fuzzy_term<uint64_t>(m, peq, term, term_len, &tested);
        exact = fuzzy_distance<uint64_t>(peq, m.len, m.transpose != 0, m.nocase != 0, term, term_len);
    }
    *match = hit ? 1 : 0;
    if (dist) *dist = (uint32_t)std::min<uint64_t>(exact, 0xFFFFFFFFull);
    return II2_OK;
}

}  // extern "C"
