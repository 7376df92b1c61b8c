// topk_count.h — the score arithmetic of the ranked query (ii2_topk_ranges: topk.hip, setop.cpp).  A doc's score is the bit-sliced
// counter of atleast_count.h (B = bit_width(n') planes, so it never saturates); here are the three things the ranking adds: a
// doc's score read back from the planes, the docs of a word whose score equals / exceeds a value, and the cut of a score
// histogram for k.  The device kernels and the host-only exports (ii2_topk_word, ii2_topk_cut) run the same code.
// The weighted form (ii2_topk_weighted_ranges) adds two: a constant added to the counters of a word's docs, and the choice of the
// groups that may be added in late mode (ii2_topkw_word, ii2_topkw_plan).
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

// add the constant w (0 < w < 2^B) to the counters of the docs in word g: a full-adder ripple per plane from plane ctz(w) up - a
// multiple of 2^ctz(w) leaves the planes below alone.  A carry out of the top plane saturates as thr_add_word does.
template <uint32_t B> II2_HD void top_add_weighted(uint32_t (&pl)[B], uint32_t g, uint32_t w) {
    const uint32_t z = w ? (uint32_t)__builtin_ctz(w) : B;
    uint32_t carry = 0u;
#pragma unroll
    for (uint32_t b = 0; b < B; b++) {
        if (b < z) continue;
        const uint32_t a = ((w >> b) & 1u) ? g : 0u;
        const uint32_t x = pl[b];
        pl[b] = x ^ a ^ carry;
        carry = (x & a) | (carry & (x ^ a));
    }
    carry |= (w >> B) ? g : 0u;                            // (a weight the planes cannot hold: saturate)
#pragma unroll
    for (uint32_t b = 0; b < B; b++) pl[b] |= carry;       // the carry left the top plane: all ones
}

// The late set of a weighted query.  The counted groups in descending order of postings, ties by index; the late groups are the
// longest prefix of that order whose weights sum to at most min_score - 1: a doc that lies in late groups only scores below
// min_score, so a late group's add may skip every 2048-doc chunk that no early group touched.  late[g] = 1 for those groups;
// returns their number.  min_score > the sum of all weights: nothing is late (nothing runs).
II2_HD uint32_t top_late_set(uint64_t n, const uint32_t *weights, const uint64_t *postings, uint32_t min_score, uint8_t *late) {
    uint64_t total = 0;
    for (uint64_t g = 0; g < n; g++) { late[g] = 0; total += weights[g]; }
    if (min_score > total) return 0u;
    uint64_t sum = 0;
    uint32_t n_late = 0;
    for (;;) {
        uint64_t best = n;                                 // the largest group not yet taken, the lowest index among equals
        for (uint64_t g = 0; g < n; g++)
            if (!late[g] && (best == n || postings[g] > postings[best])) best = g;
        if (best == n || sum + weights[best] + 1u > min_score) return n_late;
        sum += weights[best];
        late[best] = 1;
        n_late++;
    }
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
