// dict_fuzzy.hip — typo-tolerant term search in resident dictionaries, hand-written: patterns and distances in, list ranges out,
// for every range entry point.
//
// The third way to resolve a term, beside ii2_dict_find (exact, prefix) and ii2_dict_match (substring, suffix, glob): every term
// within edit distance d of a pattern, what Lucene's FuzzyQuery and the reference's dictionary library (a Levenshtein automaton
// over the FST) answer.  As in dict_match.hip the dictionaries are read whole; the answer of pattern p in dictionary s (entry
// p * k + s) is the maximal runs of consecutive matching terms.
//
// k_dict_fuzzy<W, UTF8> has k_dict_match's front (TermStage, match_runs.h): a workgroup of 256 threads takes 256 consecutive terms of
// ONE dictionary, a thread per term, the terms' bytes staged into LDS in 16-byte loads where they fit MATCH_STAGE.  Its own is the matcher
// (fuzzy_device.h): a pattern holds at most 64 bytes, so a DP column is one word W and a term byte costs one LDS load of the
// pattern's table Peq[byte] and some 15 integer instructions.  The tables live in DYNAMIC LDS sized by the call, n_patterns * 256
// words, and are built by the workgroup from the parsed patterns - zeroed, then one bit ORed in per pattern position - instead of
// uploading up to 32 KB per call.  W is uint32_t when every pattern of the call holds at most 32 positions (1 KB of table per
// pattern, half the VALU work: a 64-bit add is an add and an add-with-carry here, a 64-bit logic op two instructions), uint64_t
// otherwise or with option fuzzy.wide.  Behind the match word everything is ii2_dict_match's, shared through match_runs.h: the
// run starts and ends, the two scans, k_match_offsets, k_match_place; a second counter row carries n_tested.
//
// k_dict_fuzzy<W, true> runs when a pattern of the call carries II2_MATCH_UTF8 (utf8_bits: bit p = pattern p does).  Such a
// pattern's positions are symbols (utf8_device.h): its table has the hashed layout of fuzzy_device.h, built by the workgroup with
// LDS atomics - a wave takes the 64 bytes of one pattern, a ballot of the bytes that start a sequence numbers the symbols -, the
// thread counts its term's symbols once for all the patterns, and the recurrence decodes the term as it reads it.  The pattern loop
// is wave-uniform, so which reader a pattern takes is a uniform branch; an unflagged pattern in such a call reads bytes as ever.
// The two instances with UTF8 = false are the kernels of every call without the flag.
#include <algorithm>
#include <cstring>
#include <type_traits>
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
template <class W, bool UTF8>
__global__ __launch_bounds__(DM_THREADS) void k_dict_fuzzy(MatchDicts d, const FuzzyPattern *__restrict__ pats, uint32_t stage_on, uint32_t n_wg,
                                                           uint64_t *__restrict__ words, uint32_t *__restrict__ tab_st, uint32_t *__restrict__ tab_en,
                                                           uint32_t utf8_bits) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[MATCH_STAGE];
    __shared__ __attribute__((aligned(16))) FuzzyPattern lp[II2_FUZZY_MAX_PATTERNS];
    extern __shared__ __attribute__((aligned(16))) uint8_t fuzzy_peq_lds[];
    W *peq = (W *)fuzzy_peq_lds;                            // peq[p * 256 + c]: bit i <=> byte i of pattern p is c
    const uint32_t tid = threadIdx.x, wg = blockIdx.x, s = match_dict_of(d, wg), P = d.n_patterns;
    match_patterns_to_lds(lp, pats, P);                 // 72 bytes each
    for (uint32_t i = tid; i < P * 256u; i += DM_THREADS) peq[i] = 0;      // the tables: all zero first, before the stage's barrier
    const TermStage ts(d, s, wg, stage_on, stage);
    __syncthreads();
    // one bit per pattern position: thread i takes position i & 63 of pattern i >> 6
    for (uint32_t i = tid; i < P * II2_FUZZY_MAX_PATTERN; i += DM_THREADS) {
        const uint32_t p = i >> 6, j = i & 63u;             // (a wave holds the 64 positions of ONE pattern: p is wave-uniform)
        if (UTF8 && ((utf8_bits >> p) & 1u)) {
            // byte j starts a sequence unless it is a continuation byte (the pattern is well-formed); the symbol's position is the
            // number of starts before it, and the zero bytes behind the pattern's last count as starts at positions >= len
            const bool start = (lp[p].lit[j] & 0xC0u) != 0x80u;
            const uint32_t pos = (uint32_t)__popcll(__ballot(start) & ((1ull << j) - 1ull));
            if (start && pos < lp[p].len) {
                uint32_t c;
                utf8_at(lp[p].lit, j, II2_FUZZY_MAX_PATTERN, &c);
                W *tab = peq + p * 256u;
                if (c < 0x80u) {
                    lds_or(&tab[c], (W)1 << pos);
                } else {        // claim the first slot that is empty or already this symbol's: at most 32 keys in 64 slots
                    uint32_t *keys = (uint32_t *)(tab + FUZZY_SYM_KEYS);
                    for (uint32_t h = fuzzy_sym_hash(c);; h = (h + 1u) & (FUZZY_SYM_SLOTS - 1u)) {
                        const uint32_t old = atomicCAS(&keys[h], 0u, c);
                        if (old == 0u || old == c) {
                            lds_or(&tab[FUZZY_SYM_MASKS + h], (W)1 << pos);
                            break;
                        }
                    }
                }
            }
        } else if (j < lp[p].len) {
            lds_or(&peq[p * 256u + lp[p].lit[j]], (W)1 << j);
        }
    }
    __syncthreads();
    const uint32_t t = ts.t0 + tid;
    uint64_t m = 0;
    uint32_t n_tested = 0;
    bool tested;
    const auto one = [&](uint32_t p, uint64_t tsym) {
        return [&, p, tsym](const uint8_t *term, uint64_t len) {
            return fuzzy_term<W, UTF8>(lp[p], UTF8 && ((utf8_bits >> p) & 1u), peq + p * 256u, term, len, tsym, &tested);
        };
    };
    const auto count = [](const uint8_t *term, uint64_t len) { return utf8_count(term, len); };
    if (t < ts.t1) {
        const uint64_t tsym = UTF8 ? ts.own(t, count) : 0;      // once per term, for every flagged pattern
        for (uint32_t p = 0; p < P; p++) {
            if (ts.own(t, one(p, tsym))) m |= 1ull << p;
            n_tested += tested ? 1u : 0u;
        }
        words[d.term_first[s] + t] = m;
    }
    // (the neighbours' pairs are not counted as tested)
    match_runs_tail<2>(P, wg, n_wg, ts.have_left, ts.have_right, m, n_tested, ts.staged, [&](uint32_t right, uint32_t p) {
        const uint64_t tsym = UTF8 && ((utf8_bits >> p) & 1u) ? ts.neighbour(right, count) : 0;
        return ts.neighbour(right, one(p, tsym));
    }, tab_st, tab_en);
}

}  // namespace ii2

using namespace ii2;

extern "C" {

int ii2_dict_fuzzy(ii2_ctx *ctx, uint32_t k, const ii2_dict *const *dicts, uint32_t n_patterns, const uint8_t *pat_bytes, const uint64_t *pat_off,
                   const uint8_t *pat_dist, const uint8_t *pat_prefix, const uint8_t *pat_flags, uint64_t *run_off, uint64_t *run_first,
                   uint64_t *run_end, uint32_t *run_dict, uint64_t cap, ii2_fuzzy_stats *stats) {
    static const MatchCallTexts texts = {"ii2_dict_fuzzy", II2_FUZZY_MAX_PATTERNS, "ii2_dict_fuzzy: more than 16 patterns in one call",
                                         "ii2_dict_fuzzy: a pattern of more than 64 bytes",
                                         "ii2_dict_fuzzy: an unknown flag, or a prefix longer than its pattern"};
    uint32_t longest = 0, utf8_bits = 0, n_utf8 = 0;     // longest: in positions - symbols for a flagged pattern, bytes otherwise
    bool narrow = false;
    MatchSums sums;                                     // two counter rows: {matched pairs, staged workgroups, tested pairs, -}
    const int rc = match_call<FuzzyPattern>(ctx, texts, MatchCallIn{k, dicts, n_patterns, pat_bytes, pat_off, pat_dist},
                                            MatchRunsOut{run_off, run_first, run_end, run_dict, cap}, stats, 2,
        [&](uint32_t p, const uint8_t *bytes, uint64_t len, FuzzyPattern *out) {
            bool utf8 = false;
            const int rc = fuzzy_parse(pat_flags ? pat_flags[p] : 0u, bytes, len, pat_prefix ? pat_prefix[p] : 0u, pat_dist[p], out, &utf8);
            if (!rc) longest = std::max<uint32_t>(longest, out->len);
            if (!rc && utf8) { utf8_bits |= 1u << p; n_utf8++; }
            return rc;
        },
        [&](const MatchDicts &md, const FuzzyPattern *d_pats, uint32_t n_wg, uint64_t *d_words, uint32_t *d_tab_st, uint32_t *d_tab_en) {
            const uint32_t stage_on = ctx->opt_fuzzy_stage ? 1u : 0u;
            narrow = longest <= 32u && !ctx->opt_fuzzy_wide;
            const auto kernel = narrow ? (utf8_bits ? k_dict_fuzzy<uint32_t, true> : k_dict_fuzzy<uint32_t, false>)
                                       : (utf8_bits ? k_dict_fuzzy<uint64_t, true> : k_dict_fuzzy<uint64_t, false>);
            hipLaunchKernelGGL(kernel, dim3(n_wg), dim3(DM_THREADS), n_patterns * 256u * (narrow ? sizeof(uint32_t) : sizeof(uint64_t)), ctx->stream, md,
                               d_pats, stage_on, n_wg, d_words, d_tab_st, d_tab_en, utf8_bits);
        }, &sums);
    if ((rc && rc != II2_ECAPACITY) || !sums.n_wg || !stats) return rc;
    std::memset(stats, 0, sizeof *stats);
    stats->n_terms = sums.n_terms;
    stats->n_matched = sums.counters[0];
    stats->n_runs = sums.n_runs;
    stats->n_tested = sums.counters[2];
    stats->n_staged = (uint32_t)sums.counters[1];
    stats->n_global = sums.n_wg - stats->n_staged;
    stats->word_bits = narrow ? 32u : 64u;
    stats->n_utf8 = n_utf8;
    return rc;
}

// host only: one pattern against one term, by the parse, the filters and the recurrence k_dict_fuzzy runs
int ii2_term_fuzzy(uint32_t flags, const uint8_t *pat, uint64_t pat_len, uint32_t prefix, uint32_t max_dist, const uint8_t *term, uint64_t term_len,
                   int *match, uint32_t *dist) {
    if (!match || (pat_len && !pat) || (term_len && !term)) return II2_EINVAL;
    FuzzyPattern m;
    bool utf8;
    const int rc = fuzzy_parse(flags, pat, pat_len, prefix, max_dist, &m, &utf8);
    if (rc) return rc;
    bool tested, hit;
    uint64_t exact;
    const uint64_t tpos = utf8 ? utf8_count(term, term_len) : term_len;     // the term's positions
    const auto run = [&](auto *peq) {
        using W = std::remove_pointer_t<decltype(peq)>;
        fuzzy_peq_build(m, utf8, peq);
        hit = fuzzy_term<W, true>(m, utf8, peq, term, term_len, tpos, &tested);
        if (!m.len) exact = tpos;
        else if (utf8) exact = fuzzy_distance<W>(FuzzySymbols<W>{peq, term, m.nocase != 0}, m.len, m.transpose != 0, term_len);
        else exact = fuzzy_distance<W>(FuzzyBytes<W>{peq, term, m.nocase != 0}, m.len, m.transpose != 0, term_len);
    };
    if (m.len <= 32u) {          // the instance the kernel takes for a call of such patterns
        uint32_t peq[256];
        run(peq);
    } else {
        uint64_t peq[256];
        run(peq);
    }
    *match = hit ? 1 : 0;
    if (dist) *dist = (uint32_t)std::min<uint64_t>(exact, 0xFFFFFFFFull);
    return II2_OK;
}

}  // extern "C"
