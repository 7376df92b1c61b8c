// topk_count.h — the score arithmetic of the ranked query (ii2_topk_ranges: topk.hip, setop.cpp).  A doc's score is the bit-sliced
// counter of atleast_count.h (B = bit_width(n') planes, so it never saturates); here are the three things the ranking adds: a
// doc's score read back from the planes, the docs of a word whose score equals / exceeds a value, and the cut of a score
// histogram for k.  The device kernels and the host-only exports (ii2_topk_word, ii2_topk_cut) run the same code.
#pragma once
#include <stdint.h>

#include "atleast_count.h"

namespace ii2 {

constexpr uint32_t TOPK_SCORES = 256;                      // histogram entries: scores 0 .. 255

// the score of the doc at bit `bit` of a bitmap word: its B counter bits gathered, plane 0 the least significant
template <uint32_t B> II2_HD uint32_t top_score(const uint32_t (&pl)[B], uint32_t bit) {
    uint32_t s = 0u;
#pragma unroll
    for (uint32_t b = 0; b < B; b++) s |= ((pl[b] >> bit) & 1u) << b;
    return s;
}

// the docs whose counter equals s (eq) and those whose counter exceeds it (gt), s < 2^B, compared from the most significant
// plane down like thr_ge_word
template <uint32_t B> II2_HD void top_cmp_word(const uint32_t (&pl)[B], uint32_t s, uint32_t *eq_out, uint32_t *gt_out) {
    uint32_t gt = 0u, eq = 0xFFFFFFFFu;
#pragma unroll
    for (uint32_t k = 0; k < B; k++) {
        const uint32_t b = B - 1u - k;
        const uint32_t sb = ((s >> b) & 1u) ? 0xFFFFFFFFu : 0u;
        gt |= eq & pl[b] & ~sb;
        eq &= ~(pl[b] ^ sb);
    }
    *eq_out = eq;
    *gt_out = gt;
}
template <uint32_t B> II2_HD uint32_t top_eq_word(const uint32_t (&pl)[B], uint32_t s) {
    uint32_t eq, gt;
    top_cmp_word<B>(pl, s, &eq, &gt);
    return eq;
}

// The cut of a score histogram (hist[s] = docs of score s, TOPK_SCORES entries) for the k best docs: *cut_score = the largest s
// with sum(hist[t], t >= s) >= k - the smallest s with hist[s] > 0 when fewer than k docs are there; *n_above = the docs of a
// higher score, all of them taken; *n_cut = the docs of score cut_score taken, min(hist[cut_score], k - n_above);
// *max_score = the highest s with hist[s] > 0.  k == 0 or an all-zero histogram: all four are 0.
II2_HD void top_cut(const uint64_t *hist, uint64_t k, uint32_t *max_score, uint32_t *cut_score, uint64_t *n_above, uint64_t *n_cut) {
    *max_score = *cut_score = 0u;
    *n_above = *n_cut = 0ull;
    if (!k) return;
    uint64_t above = 0;
    bool seen = false;
    for (uint32_t s = TOPK_SCORES; s-- > 0u;) {
        const uint64_t h = hist[s];
        if (!h) continue;
        if (!seen) *max_score = s;
        seen = true;
        *cut_score = s;
        *n_above = above;
        *n_cut = h < k - above ? h : k - above;
        above += h;
        if (above >= k) return;
    }
}

}  // namespace ii2
