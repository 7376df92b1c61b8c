// fuzzy_device.h — the edit-distance matcher behind ii2_dict_fuzzy, for the device and for the host alike: k_dict_fuzzy
// (dict_fuzzy.hip) and the host-only ii2_term_fuzzy run these functions and no others.
//
// A pattern is parsed ONCE, on the host (fuzzy_parse): with II2_MATCH_NOCASE its bytes are folded there; the matcher folds the
// TERM's bytes as it reads them.  Without II2_MATCH_UTF8 everything compares bytes; only ASCII A-Z folds.
//
// The distance is the bit-parallel recurrence of Myers (1999) in Hyyro's (2003) form: a pattern holds at most
// II2_FUZZY_MAX_PATTERN = 64 bytes, so one column of the DP is one machine word W - bit i is pattern position i - and a term byte
// costs a handful of integer instructions with no loop over the pattern.  Peq[c] has bit i set when pattern byte i is c (256
// words per pattern: fuzzy_peq_build on the host, the kernel builds them in LDS); with II2_FUZZY_TRANSPOSE one more term (Hyyro's
// optimal string alignment) lets an adjacent swap cost 1.
//
// Under II2_MATCH_UTF8 a pattern position is a SYMBOL (utf8_device.h: a code point, or one ill-formed byte of a term): len counts
// symbols, the term is decoded as it is read, and the table keeps its 256 words in another layout (FUZZY_SYM_*, below).  The
// recurrence is written once: fuzzy_distance takes the reader that fetches the next Eq.  The prefix stays a byte compare -
// fuzzy_parse turns the symbol prefix into bytes, and a well-formed pattern's first s symbols equal a term's first s symbols
// exactly when the bytes do.
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
    uint8_t len;                          // positions: bytes, <= II2_FUZZY_MAX_PATTERN; symbols under II2_MATCH_UTF8
    uint8_t prefix;                       // leading BYTES a term must share (II2_MATCH_UTF8: the bytes of the prefix symbols)
    uint8_t transpose;                    // 1: an adjacent transposition costs 1
    uint8_t nocase;                       // 1: the term's A-Z compare as a-z
};
static_assert(sizeof(FuzzyPattern) == 72, "FuzzyPattern is copied into LDS word by word");

// The table of a II2_MATCH_UTF8 pattern, in the same 256 words W: entries 0 .. 127 are the ASCII symbols' masks; a larger symbol
// goes through an open-addressing hash of FUZZY_SYM_SLOTS slots - a non-ASCII symbol takes at least 2 of at most 64 bytes, so a
// pattern holds at most 32 distinct ones and the load stays at or below one half: slot h's mask is entry FUZZY_SYM_MASKS + h, its
// key (the symbol; 0 = empty, which no such symbol is) is 32-bit word h of the bytes from entry FUZZY_SYM_KEYS on (256 bytes: all
// of entries 192 .. 255 at W = uint32_t).  A term's ill-formed byte is a symbol no pattern holds: its probe ends at an empty slot.
constexpr uint32_t FUZZY_SYM_SLOTS = 64, FUZZY_SYM_MASKS = 128, FUZZY_SYM_KEYS = 192;

__host__ __device__ __forceinline__ uint32_t fuzzy_sym_hash(uint32_t c) { return (c * 0x9E3779B1u) >> 26; }      // 0 .. 63

// Eq of symbol c >= 0x80: the probe k_dict_fuzzy and ii2_term_fuzzy run
template <class W> __host__ __device__ __forceinline__ W fuzzy_sym_eq(const W *peq, uint32_t c) {
    const uint32_t *keys = (const uint32_t *)(peq + FUZZY_SYM_KEYS);
    for (uint32_t h = fuzzy_sym_hash(c);; h = (h + 1u) & (FUZZY_SYM_SLOTS - 1u)) {
        const uint32_t k = keys[h];
        if (k == c) return peq[FUZZY_SYM_MASKS + h];
        if (k == 0) return 0;
    }
}

// host: raw pattern bytes -> FuzzyPattern, *utf8 = the pattern carries II2_MATCH_UTF8 (a parsed pattern has no room for the bit:
// the kernel gets the call's bits as one word).  II2_EINVAL for a flag bit other than II2_FUZZY_TRANSPOSE / II2_MATCH_NOCASE /
// II2_MATCH_UTF8, a prefix above the pattern's length (in symbols under II2_MATCH_UTF8) or, under that flag, a pattern that is not
// well-formed UTF-8; II2_ERANGE above 64 bytes.
inline int fuzzy_parse(uint32_t flags, const uint8_t *pat, uint64_t pat_len, uint32_t prefix, uint32_t max_dist, FuzzyPattern *out, bool *utf8) {
    if (flags & ~(uint32_t)(II2_FUZZY_TRANSPOSE | II2_MATCH_NOCASE | II2_MATCH_UTF8)) return II2_EINVAL;
    if (pat_len > II2_FUZZY_MAX_PATTERN) return II2_ERANGE;
    *utf8 = (flags & II2_MATCH_UTF8) != 0;
    uint64_t len = pat_len;
    if (*utf8) {
        if (!utf8_well_formed(pat, pat_len)) return II2_EINVAL;
        len = utf8_count(pat, pat_len);
        if (prefix > len) return II2_EINVAL;
        uint64_t bytes = 0;
        for (uint32_t s = 0; s < prefix; s++) bytes += utf8_width(pat, bytes, pat_len);
        prefix = (uint32_t)bytes;
    }
    if (prefix > pat_len) return II2_EINVAL;
    FuzzyPattern m = {};
    m.max_dist = max_dist;
    m.len = (uint8_t)len;
    m.prefix = (uint8_t)prefix;
    m.transpose = (flags & II2_FUZZY_TRANSPOSE) ? 1 : 0;
    m.nocase = (flags & II2_MATCH_NOCASE) ? 1 : 0;
    for (uint64_t i = 0; i < pat_len; i++) m.lit[i] = match_fold(pat[i], m.nocase != 0);
    *out = m;
    return II2_OK;
}

// host: the pattern's table, peq[256], in the layout its flag asks for
template <class W> inline void fuzzy_peq_build(const FuzzyPattern &m, bool utf8, W *peq) {
    for (uint32_t c = 0; c < 256u; c++) peq[c] = 0;
    if (!utf8) {
        for (uint32_t i = 0; i < m.len; i++) peq[m.lit[i]] |= (W)1 << i;
        return;
    }
    uint32_t *keys = (uint32_t *)(peq + FUZZY_SYM_KEYS);
    for (uint32_t i = 0, at = 0; i < m.len; i++) {
        uint32_t c;
        at += utf8_at(m.lit, at, II2_FUZZY_MAX_PATTERN, &c);
        if (c < 0x80u) {
            peq[c] |= (W)1 << i;
            continue;
        }
        uint32_t h = fuzzy_sym_hash(c);
        while (keys[h] != 0 && keys[h] != c) h = (h + 1u) & (FUZZY_SYM_SLOTS - 1u);
        keys[h] = c;
        peq[FUZZY_SYM_MASKS + h] |= (W)1 << i;
    }
}

// How the recurrence reads a term: a reader hands it the Eq of the symbol at t[*j] and moves *j behind that symbol.  Bytes against
// the 256-entry table ...
template <class W> struct FuzzyBytes {
    const W *peq;
    const uint8_t *t;
    bool nocase;
    __host__ __device__ __forceinline__ W operator()(uint64_t *j, uint64_t) const { return peq[match_fold(t[(*j)++], nocase)]; }
};
// ... or symbols: ASCII directly, anything larger through the hash
template <class W> struct FuzzySymbols {
    const W *peq;
    const uint8_t *t;
    bool nocase;
    __host__ __device__ __forceinline__ W operator()(uint64_t *j, uint64_t tlen) const {
        uint32_t c;
        *j += utf8_at(t, *j, tlen, &c);
        return c < 0x80u ? peq[match_fold((uint8_t)c, nocase)] : fuzzy_sym_eq<W>(peq, c);
    }
};

// The exact distance between the pattern behind peq (m = its length, 1 .. bits of W) and the term: Levenshtein, or optimal
// string alignment with `transpose`.  The word starts all ones above bit m - 1 as well: those bits never reach bit m - 1, which
// alone moves the score.
template <class W, class Reader>
__host__ __device__ __forceinline__ uint32_t fuzzy_distance(const Reader &next_eq, uint32_t m, bool transpose, uint64_t tlen) {
    const W top = (W)1 << (m - 1u);
    W Pv = ~(W)0, Mv = 0, D0prev = 0, Eqprev = 0;
    uint32_t score = m;
    for (uint64_t j = 0; j < tlen;) {
        const W Eq = next_eq(&j, tlen);
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

// the filters in front of the recurrence: a distance is at least the difference of the lengths - tpos = the term's positions: tlen,
// or its symbols for a II2_MATCH_UTF8 pattern -, and the first `prefix` bytes must be the pattern's
__host__ __device__ __forceinline__ bool fuzzy_passes(const FuzzyPattern &m, const uint8_t *t, uint64_t tlen, uint64_t tpos) {
    const uint64_t diff = tpos > m.len ? tpos - m.len : m.len - tpos;
    if (diff > m.max_dist || tlen < m.prefix) return false;
    return match_at(m.lit, m.prefix, t, m.nocase != 0);
}

// pattern m (peq: its table) against one term.  *tested = the pair passed the filters (and ran the recurrence, which the empty
// pattern does not need: its distance is the term's length, and the length filter has decided).  UTF8: the instance that knows
// II2_MATCH_UTF8 patterns; `utf8` says that m is one, and then tsym is the term's symbol count (utf8_count).
template <class W, bool UTF8>
__host__ __device__ __forceinline__ bool fuzzy_term(const FuzzyPattern &m, bool utf8, const W *peq, const uint8_t *t, uint64_t tlen, uint64_t tsym, bool *tested) {
    const bool sym = UTF8 && utf8;
    *tested = fuzzy_passes(m, t, tlen, sym ? tsym : tlen);
    if (!*tested) return false;
    if (m.len == 0) return true;
    if (sym) return fuzzy_distance<W>(FuzzySymbols<W>{peq, t, m.nocase != 0}, m.len, m.transpose != 0, tlen) <= m.max_dist;
    return fuzzy_distance<W>(FuzzyBytes<W>{peq, t, m.nocase != 0}, m.len, m.transpose != 0, tlen) <= m.max_dist;
}

}  // namespace ii2
