// dict_match.hip — substring, suffix and wildcard term search in resident dictionaries, hand-written: patterns in, list ranges
// out, for every range entry point.
//
// Neither the term lookup (dict_find.hip) nor the reference's FST can answer "which terms hold `timeout`": both walk a term from
// its front.  A dictionary that lies in HBM as flat bytes can be read whole instead - a million terms are some 15 MB.  The
// answer of pattern p in dictionary s (entry p * k + s, as in ii2_dict_find) is the maximal runs of consecutive matching terms.
//
// Method, two kernels around one scan, no workgroup waits for another:
//   k_dict_match   a workgroup of 256 threads takes 256 consecutive terms of ONE dictionary, a thread per term.  The parsed
//                  patterns (match_device.h) and - where they fit MATCH_STAGE bytes - the terms' bytes are copied into LDS
//                  first, 16 bytes per lane; a span that does not fit (one very long term) is matched from global memory, by
//                  that workgroup alone.  Every thread leaves a 64-bit match word (bit p = pattern p) in workspace; the
//                  workgroup counts per pattern its run starts (m[i] && !m[i - 1]) and run ends (m[i] && !m[i + 1]) with one
//                  ballot per wave, and only for the patterns some lane of the wave has a start or an end of.  The neighbour
//                  across a workgroup's edge is matched again by that workgroup, a lane per pattern, never fetched from the
//                  other one.  The call's counters ride through the scans as one more row of the tables: no atomics.
//   scan           of the two tables [pattern][workgroup] (the workgroups dictionary by dictionary, so a pair's entries are
//                  adjacent): the entry of a pair's first workgroup is its run_off, every entry is its workgroup's place.
//   k_match_place  reads the match words, not the terms: the j-th start of a pair writes run_first / run_dict at j, the j-th
//                  end writes run_end at j - they belong to one run.  Launched only when the total fits the caller's cap.
// Everything behind the match word - the counting of run starts and ends (match_runs_tail), the scans, the two kernels under them
// and the copies (match_runs_drive) - is shared with ii2_dict_fuzzy (dict_fuzzy.hip) through match_runs.h and defined here; so is
// everything in front of it but the matcher: the patterns' copy, the stage (TermStage) and the entry point's frame (match_call).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "dv1_device.h"
#include "internal.h"
#include "match_device.h"
#include "match_runs.h"

namespace ii2 {

// With the patterns (5.5 KB) and the small arrays a workgroup holds 25.5 KB of the CU's 160 KB beside its stage (match_runs.h):
// six workgroups per CU.
static_assert(II2_MATCH_MAX_PATTERNS == 64, "a match word is 64 bits, a wave's lane p counts pattern p");

// workgroup wg: terms [t0, t0 + 256) of its dictionary.  words[term_first[s] + t] = the match word of term t; the two tables and
// their counter row are match_runs_tail's.  UTF8 = false is the kernel of every call without II2_MATCH_UTF8; the other instance
// runs when a pattern of the call carries the flag, and its glob steps over the term by symbols for those patterns (match_device.h).
template <bool UTF8>
__global__ __launch_bounds__(DM_THREADS) void k_dict_match(MatchDicts d, const MatchPattern *__restrict__ pats, uint32_t stage_on, uint32_t n_wg,
                                                           uint64_t *__restrict__ words, uint32_t *__restrict__ tab_st, uint32_t *__restrict__ tab_en) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[MATCH_STAGE];
    __shared__ __attribute__((aligned(16))) MatchPattern lp[II2_MATCH_MAX_PATTERNS];
    const uint32_t wg = blockIdx.x, s = match_dict_of(d, wg), P = d.n_patterns;
    match_patterns_to_lds(lp, pats, P);                 // 88 bytes each
    const TermStage ts(d, s, wg, stage_on, stage);
    __syncthreads();
    const uint32_t t = ts.t0 + threadIdx.x;
    uint64_t m = 0;
    if (t < ts.t1) {
        m = ts.own(t, [&](const uint8_t *term, uint64_t len) { return match_word<UTF8>(lp, P, term, len); });
        words[d.term_first[s] + t] = m;
    }
    match_runs_tail<1>(P, wg, n_wg, ts.have_left, ts.have_right, m, 0u, ts.staged, [&](uint32_t right, uint32_t p) {
        return ts.neighbour(right, [&](const uint8_t *term, uint64_t len) { return match_term<UTF8>(lp[p], term, len); });
    }, tab_st, tab_en);
}

// run_off[p * k + s] = the runs before pair (p, s) = the scanned start table at the pair's first workgroup; run_off[P * k] = all
// of them; behind it the counters the tables' rows P .. P + n_rows - 1 carried, two per row: [P * k + 1 + 2 r] = the total of row
// r of the start table (row 0: matched pairs), [P * k + 2 + 2 r] = of the end table (row 0: staged workgroups)
__global__ void k_match_offsets(MatchDicts d, uint32_t n_wg, uint32_t n_rows, const uint64_t *__restrict__ pre_st, const uint64_t *__restrict__ pre_en,
                                uint64_t *__restrict__ run_off) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, n = d.n_patterns * d.k;
    const uint64_t row_p = (uint64_t)d.n_patterns * n_wg;
    if (i > n + 2u * n_rows) return;
    if (i > n) {
        const uint32_t c = i - n - 1u;
        const uint64_t row = row_p + (uint64_t)(c >> 1) * n_wg;
        const uint64_t *__restrict__ pre = (c & 1u) ? pre_en : pre_st;
        run_off[i] = pre[row + n_wg] - pre[row];
        return;
    }
    const uint32_t p = i / d.k, s = i - p * d.k;
    run_off[i] = i == n ? pre_st[row_p] : pre_st[(uint64_t)p * n_wg + d.wg_first[s]];
}

// the same workgroups again, over the match words: every run start and every run end goes to its rank
__global__ __launch_bounds__(DM_THREADS) void k_match_place(MatchDicts d, uint32_t n_wg, const uint64_t *__restrict__ words, const uint64_t *__restrict__ pre_st,
                                                            const uint64_t *__restrict__ pre_en, uint64_t n_runs, uint64_t *__restrict__ run_first,
                                                            uint64_t *__restrict__ run_end, uint32_t *__restrict__ run_dict) {
    __shared__ uint32_t wcnt[DM_WAVES][2][64];
    const uint32_t tid = threadIdx.x, wg = blockIdx.x;
    const uint32_t s = match_dict_of(d, wg), n = d.n[s];
    const uint32_t t = (wg - d.wg_first[s]) * DM_THREADS + tid;
    const uint64_t *__restrict__ w = words + d.term_first[s];
    uint64_t st = 0, en = 0;
    if (t < n) {
        const uint64_t m = w[t];
        st = m & ~(t > 0 ? w[t - 1] : 0ull);
        en = m & ~(t + 1u < n ? w[t + 1] : 0ull);
    }
    uint32_t cs, ce;
    wave_run_counts(st, en, &cs, &ce);
    const uint32_t l = (uint32_t)lane_id(), wv = tid >> 6;
    wcnt[wv][0][l] = cs;
    wcnt[wv][1][l] = ce;
    __syncthreads();
    const uint64_t below = (1ull << l) - 1ull;
    for (uint64_t live = wave_or64(st | en); live; live &= live - 1ull) {
        const uint32_t p = (uint32_t)__builtin_ctzll(live);
        const uint64_t bs = __ballot((st >> p) & 1ull), be = __ballot((en >> p) & 1ull);
        uint32_t before_s = 0, before_e = 0;
        for (uint32_t v = 0; v < wv; v++) { before_s += wcnt[v][0][p]; before_e += wcnt[v][1][p]; }
        const uint64_t at = (uint64_t)p * n_wg + wg;
        if ((st >> p) & 1ull) {
            const uint64_t j = pre_st[at] + before_s + (uint32_t)__popcll(bs & below);
            if (j < n_runs) {       // (always: the scan's total is n_runs)
                run_first[j] = t;
                run_dict[j] = s;
            }
        }
        if ((en >> p) & 1ull) {
            const uint64_t j = pre_en[at] + before_e + (uint32_t)__popcll(be & below);
            if (j < n_runs) run_end[j] = (uint64_t)t + 1u;
        }
    }
}

int match_runs_drive(ii2_ctx *ctx, const char *name, const MatchDicts &md, uint32_t n_rows, size_t head_bytes, const MatchLaunch &launch,
                     const MatchRunsOut &out, uint64_t *n_runs_out, uint64_t *counters) {
    const uint32_t k = md.k, n_patterns = md.n_patterns, n_wg = md.wg_first[k];
    const uint64_t n_pairs = (uint64_t)n_patterns * k, n_terms = md.term_first[k], cap = out.cap;
    const uint64_t n_off = n_pairs + 1 + 2ull * n_rows;              // run_off, then two counters per row
    hipStream_t st = ctx->stream;
    // a pair's runs are at most every other term of its dictionary; the caller's cap bounds what is ever written
    uint64_t most = 0;
    for (uint32_t s = 0; s < k; s++) most += (uint64_t)n_patterns * ((md.n[s] + 1u) / 2u);
    const uint64_t n_place = std::min(cap, most);
    const uint64_t n_tab = ((uint64_t)n_patterns + n_rows) * n_wg + 1;   // the patterns' rows, the counters' rows, + 1: the scan's total
    const size_t tmp_bytes = scan_temp_bytes(n_tab);
    int rc = ii2_ws_reserve(ctx, align_up(head_bytes) + align_up(n_terms * sizeof(uint64_t)) + 2 * align_up(n_tab * sizeof(uint32_t)) +
                                     2 * align_up(n_tab * sizeof(uint64_t)) + tmp_bytes + align_up(n_off * sizeof(uint64_t)) +
                                     2 * align_up(n_place * sizeof(uint64_t)) + align_up(n_place * sizeof(uint32_t)));
    if (rc) return rc;
    void *d_head = ws_take<uint8_t>(ctx, head_bytes);
    uint64_t *d_words = ws_take<uint64_t>(ctx, n_terms);
    uint32_t *d_tab_st = ws_take<uint32_t>(ctx, n_tab), *d_tab_en = ws_take<uint32_t>(ctx, n_tab);
    uint64_t *d_pre_st = ws_take<uint64_t>(ctx, n_tab), *d_pre_en = ws_take<uint64_t>(ctx, n_tab);
    void *d_tmp = ws_take<uint8_t>(ctx, tmp_bytes);
    uint64_t *d_run_off = ws_take<uint64_t>(ctx, n_off);
    uint64_t *d_first = ws_take<uint64_t>(ctx, n_place), *d_end = ws_take<uint64_t>(ctx, n_place);
    uint32_t *d_dict = ws_take<uint32_t>(ctx, n_place);
    HIP_TRY(ctx, hipMemsetAsync(d_tab_st + (n_tab - 1), 0, sizeof(uint32_t), st));
    HIP_TRY(ctx, hipMemsetAsync(d_tab_en + (n_tab - 1), 0, sizeof(uint32_t), st));
    rc = launch(d_head, d_words, d_tab_st, d_tab_en);
    if (rc) return rc;
    HIP_TRY(ctx, scan_excl_u32_to_u64(d_tmp, tmp_bytes, d_tab_st, d_pre_st, n_tab, st));
    HIP_TRY(ctx, scan_excl_u32_to_u64(d_tmp, tmp_bytes, d_tab_en, d_pre_en, n_tab, st));
    hipLaunchKernelGGL(k_match_offsets, dim3((unsigned)((n_off + 255) / 256)), dim3(256), 0, st, md, n_wg, n_rows, (const uint64_t *)d_pre_st,
                       (const uint64_t *)d_pre_en, d_run_off);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<uint64_t> h_off(n_off), h_first, h_end;             // the caller's arrays are written only once nothing can fail any more:
    std::vector<uint32_t> h_dict;                                   // an error return leaves all of them untouched
    HIP_TRY(ctx, hipMemcpyAsync(h_off.data(), d_run_off, n_off * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                       // the first wait: the sizes
    const uint64_t n_runs = h_off[n_pairs];
    if (n_runs <= cap && n_runs) {
        hipLaunchKernelGGL(k_match_place, dim3(n_wg), dim3(DM_THREADS), 0, st, md, n_wg, (const uint64_t *)d_words, (const uint64_t *)d_pre_st,
                           (const uint64_t *)d_pre_en, n_runs, d_first, d_end, d_dict);
        HIP_TRY(ctx, hipGetLastError());
        h_first.resize(n_runs); h_end.resize(n_runs); h_dict.resize(out.run_dict ? n_runs : 0);
        HIP_TRY(ctx, hipMemcpyAsync(h_first.data(), d_first, n_runs * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(h_end.data(), d_end, n_runs * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        if (out.run_dict) HIP_TRY(ctx, hipMemcpyAsync(h_dict.data(), d_dict, n_runs * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));                   // the second wait: the runs
        std::memcpy(out.run_first, h_first.data(), n_runs * sizeof(uint64_t));
        std::memcpy(out.run_end, h_end.data(), n_runs * sizeof(uint64_t));
        if (out.run_dict) std::memcpy(out.run_dict, h_dict.data(), n_runs * sizeof(uint32_t));
    }
    std::memcpy(out.run_off, h_off.data(), (n_pairs + 1) * sizeof(uint64_t));
    *n_runs_out = n_runs;
    for (uint32_t c = 0; c < 2u * n_rows; c++) counters[c] = h_off[n_pairs + 1 + c];
    if (n_runs > cap) {
        ctx->err = std::string(name) + ": more runs than cap (run_off is filled: allocate run_off[n_patterns * k] and call again)";
        return II2_ECAPACITY;
    }
    return II2_OK;
}

}  // namespace ii2

using namespace ii2;

extern "C" {

int ii2_dict_match(ii2_ctx *ctx, uint32_t k, const ii2_dict *const *dicts, uint32_t n_patterns, const uint8_t *pat_bytes, const uint64_t *pat_off,
                   const uint8_t *pat_kind, uint64_t *run_off, uint64_t *run_first, uint64_t *run_end, uint32_t *run_dict, uint64_t cap,
                   ii2_match_stats *stats) {
    static const MatchCallTexts texts = {"ii2_dict_match", II2_MATCH_MAX_PATTERNS, "ii2_dict_match: more than 64 patterns in one call",
                                         "ii2_dict_match: a pattern of more than 64 bytes",
                                         "ii2_dict_match: an unknown kind, a glob that ends in a lone backslash, or an ill-formed pattern under II2_MATCH_UTF8"};
    MatchSums sums;                                     // one counter row: {matched pairs, staged workgroups}
    bool utf8 = false;                                  // a pattern carries II2_MATCH_UTF8
    const int rc = match_call<MatchPattern>(ctx, texts, MatchCallIn{k, dicts, n_patterns, pat_bytes, pat_off, pat_kind},
                                            MatchRunsOut{run_off, run_first, run_end, run_dict, cap}, stats, 1,
        [&](uint32_t p, const uint8_t *bytes, uint64_t len, MatchPattern *out) {
            const int rc = match_parse(pat_kind[p], bytes, len, out);
            if (!rc && out->utf8) utf8 = true;
            return rc;
        },
        [&](const MatchDicts &md, const MatchPattern *d_pats, uint32_t n_wg, uint64_t *d_words, uint32_t *d_tab_st, uint32_t *d_tab_en) {
            hipLaunchKernelGGL(utf8 ? k_dict_match<true> : k_dict_match<false>, dim3(n_wg), dim3(DM_THREADS), 0, ctx->stream, md, d_pats,
                               ctx->opt_match_stage ? 1u : 0u, n_wg, d_words, d_tab_st, d_tab_en);
        }, &sums);
    if ((rc && rc != II2_ECAPACITY) || !sums.n_wg || !stats) return rc;
    stats->n_terms = sums.n_terms;
    stats->n_matched = sums.counters[0];
    stats->n_runs = sums.n_runs;
    stats->n_staged = (uint32_t)sums.counters[1];
    stats->n_global = sums.n_wg - stats->n_staged;
    return rc;
}

// host only: one pattern against one term, by the parse and the matchers k_dict_match runs
int ii2_term_match(uint32_t kind, const uint8_t *pat, uint64_t pat_len, const uint8_t *term, uint64_t term_len, int *match) {
    if (!match || (pat_len && !pat) || (term_len && !term)) return II2_EINVAL;
    MatchPattern m;
    const int rc = match_parse(kind, pat, pat_len, &m);
    if (rc) return rc;
    *match = match_term<true>(m, term, term_len) ? 1 : 0;
    return II2_OK;
}

// host only: a byte string's symbols by the decoder the kernels run under II2_MATCH_UTF8 (utf8_device.h)
int ii2_utf8_decode(const uint8_t *bytes, uint64_t len, uint32_t *symbols, uint64_t cap, uint64_t *n_symbols, int *well_formed) {
    if (!n_symbols || (len && !bytes) || (cap && !symbols)) return II2_EINVAL;
    uint64_t n = 0;
    bool fine = true;
    for (uint64_t i = 0; i < len; n++) {
        uint32_t sym;
        const uint32_t w = utf8_at(bytes, i, len, &sym);
        if (bytes[i] >= 0x80u && w == 1u) fine = false;
        if (n < cap) symbols[n] = sym;
        i += w;
    }
    *n_symbols = n;
    if (well_formed) *well_formed = fine ? 1 : 0;
    return II2_OK;
}

}  // extern "C"
