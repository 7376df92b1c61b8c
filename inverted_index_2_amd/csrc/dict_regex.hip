// dict_regex.hip — regular-expression term search in resident dictionaries, hand-written: patterns in, list ranges out, for every
// range entry point.
//
// The fourth way to resolve a term, beside ii2_dict_find (exact, prefix), ii2_dict_match (substring, suffix, glob) and
// ii2_dict_fuzzy (edit distance): every term a regular expression matches as a whole, what Lucene's RegexpQuery and the
// reference's dictionary library (a regex automaton walked over the FST) answer.  As in dict_match.hip the dictionaries are read
// whole; the answer of pattern p in dictionary s (entry p * k + s) is the maximal runs of consecutive matching terms.
//
// k_dict_regex has k_dict_fuzzy's data flow (TermStage, match_runs.h): a workgroup of 256 threads takes 256 consecutive terms of
// ONE dictionary, a thread per term, the terms' bytes staged into LDS in 16-byte loads where they fit MATCH_STAGE.  Its own is the
// matcher (regex_device.h): a pattern is a Glushkov automaton of at most 64 positions, parsed on the host, so a thread's set of
// states is one 64-bit register and a term byte costs one LDS load of b[byte], a shift for the positions that only advance and
// one more LDS load per other live position.  The parsed patterns - 2608 bytes each - live in DYNAMIC LDS sized by the call and are
// copied there in 16-byte loads.  Behind the match word everything is ii2_dict_match's, shared through match_runs.h: the run
// starts and ends, the two scans, k_match_offsets, k_match_place; a second counter row carries n_tested.
#include <algorithm>
#include <cstring>
#include <vector>

#include "dv1_device.h"
#include "internal.h"
#include "match_runs.h"
#include "regex_device.h"

namespace ii2 {

static_assert(II2_REGEX_MAX_PATTERNS <= 64, "a match word is 64 bits, a wave's lane p counts pattern p");
static_assert(II2_REGEX_MAX_POSITIONS == 64, "a set of states is one 64-bit word");
// the stage, the patterns and match_runs_tail's 4.1 KB stay below the 64 KB a workgroup gets without a function attribute
static_assert(MATCH_STAGE + II2_REGEX_MAX_PATTERNS * sizeof(RegexPattern) + 4608 <= 65536, "k_dict_regex's LDS at the largest call");

// workgroup wg: terms [t0, t0 + 256) of its dictionary.  words[term_first[s] + t] = the match word of term t; the two tables and
// their two counter rows are match_runs_tail's (the second one: the pairs of this workgroup's threads that passed the length
// filter).  Dynamic LDS: n_patterns * sizeof(RegexPattern) bytes.
__global__ __launch_bounds__(DM_THREADS) void k_dict_regex(MatchDicts d, const RegexPattern *__restrict__ pats, uint32_t stage_on, uint32_t n_wg,
                                                           uint64_t *__restrict__ words, uint32_t *__restrict__ tab_st, uint32_t *__restrict__ tab_en) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[MATCH_STAGE];
    extern __shared__ __attribute__((aligned(16))) uint8_t regex_pat_lds[];
    RegexPattern *lp = (RegexPattern *)regex_pat_lds;
    const uint32_t tid = threadIdx.x, wg = blockIdx.x, s = match_dict_of(d, wg), P = d.n_patterns;
    match_patterns_to_lds16(lp, pats, P);
    const TermStage ts(d, s, wg, stage_on, stage);
    __syncthreads();
    const uint32_t t = ts.t0 + tid;
    uint64_t m = 0;
    uint32_t n_tested = 0;
    bool tested;
    const auto one = [&](uint32_t p) { return [&, p](const uint8_t *term, uint64_t len) { return regex_term(lp[p], term, len, &tested); }; };
    if (t < ts.t1) {
        for (uint32_t p = 0; p < P; p++) {
            if (ts.own(t, one(p))) m |= 1ull << p;
            n_tested += tested ? 1u : 0u;
        }
        words[d.term_first[s] + t] = m;
    }
    // (the neighbours' pairs are not counted as tested)
    match_runs_tail<2>(P, wg, n_wg, ts.have_left, ts.have_right, m, n_tested, ts.staged,
                       [&](uint32_t right, uint32_t p) { return ts.neighbour(right, one(p)); }, tab_st, tab_en);
}

}  // namespace ii2

using namespace ii2;

extern "C" {

int ii2_dict_regex(ii2_ctx *ctx, uint32_t k, const ii2_dict *const *dicts, uint32_t n_patterns, const uint8_t *pat_bytes, const uint64_t *pat_off,
                   const uint8_t *pat_flags, uint64_t *run_off, uint64_t *run_first, uint64_t *run_end, uint32_t *run_dict, uint64_t cap,
                   ii2_regex_stats *stats) {
    static const MatchCallTexts texts = {"ii2_dict_regex", II2_REGEX_MAX_PATTERNS, "ii2_dict_regex: more than 8 patterns in one call",
                                         "ii2_dict_regex: a pattern of more than 256 bytes or more than 64 positions",
                                         "ii2_dict_regex: an unknown flag, or a pattern outside the syntax"};
    uint32_t most = 0;
    MatchSums sums;                                     // two counter rows: {matched pairs, staged workgroups, tested pairs, -}
    // (pat_flags may be NULL: the array that must not be is pat_off)
    const int rc = match_call<RegexPattern>(ctx, texts, MatchCallIn{k, dicts, n_patterns, pat_bytes, pat_off, pat_off},
                                            MatchRunsOut{run_off, run_first, run_end, run_dict, cap}, stats, 2,
        [&](uint32_t p, const uint8_t *bytes, uint64_t len, RegexPattern *out) {
            const int rc = regex_parse(pat_flags ? pat_flags[p] : 0u, bytes, len, out);
            if (!rc) most = std::max<uint32_t>(most, out->n_pos);
            return rc;
        },
        [&](const MatchDicts &md, const RegexPattern *d_pats, uint32_t n_wg, uint64_t *d_words, uint32_t *d_tab_st, uint32_t *d_tab_en) {
            hipLaunchKernelGGL(k_dict_regex, dim3(n_wg), dim3(DM_THREADS), n_patterns * sizeof(RegexPattern), ctx->stream, md, d_pats,
                               ctx->opt_regex_stage ? 1u : 0u, n_wg, d_words, d_tab_st, d_tab_en);
        }, &sums);
    if ((rc && rc != II2_ECAPACITY) || !sums.n_wg || !stats) return rc;
    std::memset(stats, 0, sizeof *stats);               // (it has a pad word)
    stats->n_terms = sums.n_terms;
    stats->n_matched = sums.counters[0];
    stats->n_runs = sums.n_runs;
    stats->n_tested = sums.counters[2];
    stats->n_staged = (uint32_t)sums.counters[1];
    stats->n_global = sums.n_wg - stats->n_staged;
    stats->max_positions = most;
    return rc;
}

// host only: one pattern against one term, by the parse, the filter and the step k_dict_regex runs
int ii2_term_regex(uint32_t flags, const uint8_t *pat, uint64_t pat_len, const uint8_t *term, uint64_t term_len, int *match, uint32_t *n_pos) {
    if (!match || (pat_len && !pat) || (term_len && !term)) return II2_EINVAL;
    RegexPattern m;
    const int rc = regex_parse(flags, pat, pat_len, &m, n_pos);
    if (rc) return rc;
    bool tested;
    *match = regex_term(m, term, term_len, &tested) ? 1 : 0;
    return II2_OK;
}

}  // extern "C"
