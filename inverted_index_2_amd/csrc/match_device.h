// match_device.h — the three term matchers behind ii2_dict_match (substring, suffix, glob), for the device and for the host
// alike: k_dict_match (dict_match.hip) and the host-only ii2_term_match run these functions and no others.
//
// A pattern is parsed ONCE, on the host (match_parse): escapes are resolved into literal bytes plus two 64-bit masks that say
// which positions are `*` and which are `?` (a pattern holds at most II2_MATCH_MAX_PATTERN = 64 bytes, one bit each); with
// II2_MATCH_NOCASE its literal bytes are folded there.  The matchers never look at `\`; they fold the TERM's bytes as they read
// them.  Everything compares bytes and only ASCII A-Z folds; under II2_MATCH_UTF8 the glob's `?` and `*` take whole symbols of
// the term (utf8_device.h) - the literals still compare bytes, which for a well-formed pattern is the same thing: an occurrence
// of its bytes in a term starts and ends on symbol boundaries of the term.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "../../include/ii2.h"
#include "utf8_device.h"

namespace ii2 {

// one parsed pattern: 88 bytes, 64 of them fill 5.5 KB of LDS
struct MatchPattern {
    uint8_t lit[II2_MATCH_MAX_PATTERN];   // the bytes after escape resolution (folded with nocase); a wildcard's byte is unused
    uint64_t star, any1;                  // bit i: position i is `*` / `?` (GLOB only)
    uint32_t len;                         // positions, <= II2_MATCH_MAX_PATTERN
    uint8_t kind;                         // II2_MATCH_CONTAINS / SUFFIX / GLOB
    uint8_t nocase;                       // 1: the term's A-Z compare as a-z
    uint8_t utf8;                         // 1: II2_MATCH_UTF8 - `?` is one symbol of the term, `*` a run of whole symbols
    uint8_t pad;
};
static_assert(sizeof(MatchPattern) == 88, "MatchPattern is copied into LDS word by word");

__host__ __device__ __forceinline__ uint8_t match_fold(uint8_t c, bool nocase) { return nocase && c >= 'A' && c <= 'Z' ? (uint8_t)(c + 32u) : c; }

// host: raw pattern bytes -> MatchPattern.  II2_ERANGE above 64 bytes, II2_EINVAL for an unknown kind, a lone `\` at the end of a
// glob or, under II2_MATCH_UTF8, a pattern that is not well-formed UTF-8.
inline int match_parse(uint32_t kind_flags, const uint8_t *pat, uint64_t pat_len, MatchPattern *out) {
    const uint32_t kind = kind_flags & ~(uint32_t)(II2_MATCH_NOCASE | II2_MATCH_UTF8);
    if (kind > II2_MATCH_GLOB) return II2_EINVAL;
    if (pat_len > II2_MATCH_MAX_PATTERN) return II2_ERANGE;
    MatchPattern m = {};
    m.kind = (uint8_t)kind;
    m.nocase = (kind_flags & II2_MATCH_NOCASE) ? 1 : 0;
    m.utf8 = (kind_flags & II2_MATCH_UTF8) ? 1 : 0;
    if (m.utf8 && !utf8_well_formed(pat, pat_len)) return II2_EINVAL;      // (`\`, `*` and `?` are ASCII: the literals are well-formed too)
    for (uint64_t i = 0; i < pat_len; i++) {
        uint8_t c = pat[i];
        if (kind == II2_MATCH_GLOB) {
            if (c == '\\') {
                if (++i == pat_len) return II2_EINVAL;
                c = pat[i];
            } else if (c == '*') {
                m.star |= 1ull << m.len++;
                continue;
            } else if (c == '?') {
                m.any1 |= 1ull << m.len++;
                continue;
            }
        }
        m.lit[m.len++] = match_fold(c, m.nocase != 0);
    }
    *out = m;
    return II2_OK;
}

// the literal p[0 .. n) at t[0 .. n)
__host__ __device__ __forceinline__ bool match_at(const uint8_t *p, uint32_t n, const uint8_t *t, bool nocase) {
    for (uint32_t j = 0; j < n; j++)
        if (match_fold(t[j], nocase) != p[j]) return false;
    return true;
}

__host__ __device__ __forceinline__ bool match_suffix(const MatchPattern &m, const uint8_t *t, uint64_t tlen) {
    return tlen >= m.len && match_at(m.lit, m.len, t + (tlen - m.len), m.nocase != 0);
}

__host__ __device__ __forceinline__ bool match_contains(const MatchPattern &m, const uint8_t *t, uint64_t tlen) {
    if (tlen < m.len) return false;
    for (uint64_t i = 0; i + m.len <= tlen; i++)
        if (match_at(m.lit, m.len, t + i, m.nocase != 0)) return true;
    return false;
}

// whole-term glob, iterative with two pointers: on a mismatch go back to the last `*` and let it take one byte more.  Constant
// state, no recursion; O(len(pattern) * len(term)) at worst.  UTF8: the instance that honours m.utf8 - there `?` and a `*` that
// takes one more step by the width of the term's symbol, so ti stands on a symbol boundary wherever the pattern does.
template <bool UTF8> __host__ __device__ __forceinline__ bool match_glob(const MatchPattern &m, const uint8_t *t, uint64_t tlen) {
    const bool sym = UTF8 && m.utf8 != 0;
    const uint32_t none = 0xFFFFFFFFu;
    uint32_t pi = 0, star_pi = none;
    uint64_t ti = 0, star_ti = 0;
    while (ti < tlen) {
        if (pi < m.len && ((m.star >> pi) & 1ull)) {
            star_pi = pi++;
            star_ti = ti;
        } else if (pi < m.len && (((m.any1 >> pi) & 1ull) || m.lit[pi] == match_fold(t[ti], m.nocase != 0))) {
            ti += sym && ((m.any1 >> pi) & 1ull) ? utf8_width(t, ti, tlen) : 1u;
            pi++;
        } else if (star_pi != none) {
            pi = star_pi + 1u;
            star_ti += sym ? utf8_width(t, star_ti, tlen) : 1u;
            ti = star_ti;
        } else {
            return false;
        }
    }
    while (pi < m.len && ((m.star >> pi) & 1ull)) pi++;
    return pi == m.len;
}

template <bool UTF8> __host__ __device__ __forceinline__ bool match_term(const MatchPattern &m, const uint8_t *t, uint64_t tlen) {
    if (m.kind == II2_MATCH_CONTAINS) return match_contains(m, t, tlen);
    if (m.kind == II2_MATCH_SUFFIX) return match_suffix(m, t, tlen);
    return match_glob<UTF8>(m, t, tlen);
}

// bit p of the answer: pattern p of pats[0 .. n) matches the term
template <bool UTF8> __host__ __device__ __forceinline__ uint64_t match_word(const MatchPattern *pats, uint32_t n, const uint8_t *t, uint64_t tlen) {
    uint64_t w = 0;
    for (uint32_t p = 0; p < n; p++)
        if (match_term<UTF8>(pats[p], t, tlen)) w |= 1ull << p;
    return w;
}

}  // namespace ii2
