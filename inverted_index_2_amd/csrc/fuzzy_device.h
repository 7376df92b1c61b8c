// fuzzy_device.h — the edit-distance matcher behind ii2_dict_fuzzy, for the device and for the host alike: k_dict_fuzzy
// (dict_fuzzy.hip) and the host-only ii2_term_fuzzy run these functions and no others.
//
// A pattern is parsed ONCE, on the host (fuzzy_parse): with II2_MATCH_NOCASE its bytes are folded there; the matcher folds the
// TERM's bytes as it reads them.  Everything compares bytes: no UTF-8, and only ASCII A-Z folds.
//
// The distance is the bit-parallel recurrence of Myers (1999) in Hyyro's (2003) form: a pattern holds at most
// II2_FUZZY_MAX_PATTERN = 64 bytes, so one column of the DP is one machine word W - bit i is pattern position i - and a term byte
// costs a handful of integer instructions with no loop over the pattern.  Peq[c] has bit i set when pattern byte i is c (256
// words per pattern: fuzzy_peq_build on the host, the kernel builds them in LDS); with II2_FUZZY_TRANSPOSE one more term (Hyyro's
// optimal string alignment) lets an adjacent swap cost 1.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "../../include/ii2.h"
#include "match_device.h"

namespace ii2 {

// one parsed pattern: 72 bytes, 16 of them fill 1.1 KB of LDS
struct FuzzyPattern {
    uint8_t lit[II2_FUZZY_MAX_PATTERN];   // the bytes (folded with nocase)
    uint32_t max_dist;                    // the largest distance that matches
    uint8_t len;                          // bytes, <= II2_FUZZY_MAX_PATTERN
    uint8_t prefix;                       // leading bytes a term must share, <= len
    uint8_t transpose;                    // 1: an adjacent transposition costs 1
    uint8_t nocase;                       // 1: the term's A-Z compare as a-z
};
static_assert(sizeof(FuzzyPattern) == 72, "FuzzyPattern is copied into LDS word by word");

// host: raw pattern bytes -> FuzzyPattern.  II2_EINVAL for a flag bit other than II2_FUZZY_TRANSPOSE / II2_MATCH_NOCASE or a
// prefix above the pattern's length, II2_ERANGE above 64 bytes.
inline int fuzzy_parse(uint32_t flags, const uint8_t *pat, uint64_t pat_len, uint32_t prefix, uint32_t max_dist, FuzzyPattern *out) {
    if (flags & ~(uint32_t)(II2_FUZZY_TRANSPOSE | II2_MATCH_NOCASE)) return II2_EINVAL;
    if (pat_len > II2_FUZZY_MAX_PATTERN) return II2_ERANGE;
    if (prefix > pat_len) return II2_EINVAL;
    FuzzyPattern m = {};
    m.max_dist = max_dist;
    m.len = (uint8_t)pat_len;
    m.prefix = (uint8_t)prefix;
    m.transpose = (flags & II2_FUZZY_TRANSPOSE) ? 1 : 0;
    m.nocase = (flags & II2_MATCH_NOCASE) ? 1 : 0;
    for (uint64_t i = 0; i < pat_len; i++) m.lit[i] = match_fold(pat[i], m.nocase != 0);
    *out = m;
    return II2_OK;
}

// host: the pattern's table, peq[256]
template <class W> inline void fuzzy_peq_build(const FuzzyPattern &m, W *peq) {
    for (uint32_t c = 0; c < 256u; c++) peq[c] = 0;
    for (uint32_t i = 0; i < m.len; i++) peq[m.lit[i]] |= (W)1 << i;
}

// The exact distance between the pattern behind peq (m = its length, 1 .. bits of W) and the term: Levenshtein, or optimal
// string alignment with `transpose`.  The word starts all ones above bit m - 1 as well: those bits never reach bit m - 1, which
// alone moves the score.
template <class W>
__host__ __device__ __forceinline__ uint32_t fuzzy_distance(const W *peq, uint32_t m, bool transpose, bool nocase, const uint8_t *t, uint64_t tlen) {
    const W top = (W)1 << (m - 1u);
    W Pv = ~(W)0, Mv = 0, D0prev = 0, Eqprev = 0;
    uint32_t score = m;
    for (uint64_t j = 0; j < tlen; j++) {
        const W Eq = peq[match_fold(t[j], nocase)];
        W D0 = (((Eq & Pv) + Pv) ^ Pv) | Eq | Mv;
        if (transpose) D0 |= ((~D0prev & Eq) << 1) & Eqprev;
        const W Hp = Mv | ~(D0 | Pv), Hn = D0 & Pv;
        score += (Hp & top) != 0;
        score -= (Hn & top) != 0;
        const W X = (W)(Hp << 1) | (W)1;
        Pv = (W)(Hn << 1) | ~(D0 | X);
        Mv = X & D0;
        D0prev = D0;
        Eqprev = Eq;
    }
    return score;
}

// the filters in front of the recurrence: a distance is at least the difference of the lengths, and the first `prefix` bytes
// must be the pattern's
__host__ __device__ __forceinline__ bool fuzzy_passes(const FuzzyPattern &m, const uint8_t *t, uint64_t tlen) {
    const uint64_t diff = tlen > m.len ? tlen - m.len : m.len - tlen;
    if (diff > m.max_dist || tlen < m.prefix) return false;
    return match_at(m.lit, m.prefix, t, m.nocase != 0);
}

// pattern m (peq: its table) against one term.  *tested = the pair passed the filters (and ran the recurrence, which the empty
// pattern does not need: its distance is the term's length, and the length filter has decided).
template <class W> __host__ __device__ __forceinline__ bool fuzzy_term(const FuzzyPattern &m, const W *peq, const uint8_t *t, uint64_t tlen, bool *tested) {
    *tested = fuzzy_passes(m, t, tlen);
    if (!*tested) return false;
    if (m.len == 0) return true;
    return fuzzy_distance<W>(peq, m.len, m.transpose != 0, m.nocase != 0, t, tlen) <= m.max_dist;
}

}  // namespace ii2
