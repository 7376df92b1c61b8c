// utf8_device.h — the one UTF-8 decoder behind II2_MATCH_UTF8, for the device and for the host alike: k_dict_fuzzy, k_dict_match,
// ii2_term_fuzzy, ii2_term_match and ii2_utf8_decode read a term's symbols through utf8_at and nothing else.
//
// A byte string is read left to right as symbols.  Where a well-formed sequence starts at byte i (RFC 3629, Unicode table 3-7: no
// overlong form, no U+D800..DFFF, nothing above U+10FFFF, the whole sequence inside the string) it is one symbol, its code point.
// Otherwise byte i alone is one symbol, 0xDC00 + byte, and reading goes on at i + 1 - Python's
// bytes.decode("utf-8", "surrogateescape").  Total on arbitrary bytes, and injective: no code point lies in 0xDC80..0xDCFF.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace ii2 {

constexpr uint32_t UTF8_ESCAPE = 0xDC00u;         // an ill-formed byte b is the symbol UTF8_ESCAPE + b

// The symbol at t[i], i < tlen: *sym = the symbol, returns its width in bytes (1 .. 4).  Never reads t[j] for j >= tlen: a
// sequence cut off by the string's end is ill-formed, whatever lies behind it (in the LDS stage: the next term).
__host__ __device__ __forceinline__ uint32_t utf8_at(const uint8_t *t, uint64_t i, uint64_t tlen, uint32_t *sym) {
    const uint32_t b0 = t[i];
    *sym = b0;
    if (b0 < 0x80u) return 1u;
    *sym = UTF8_ESCAPE + b0;
    if (b0 < 0xC2u || b0 > 0xF4u) return 1u;        // a continuation byte, C0 / C1 (overlong), F5 .. FF
    const uint32_t n = b0 < 0xE0u ? 2u : b0 < 0xF0u ? 3u : 4u;
    if (tlen - i < n) return 1u;
    // the second byte's range keeps out the overlong forms (E0, F0), the surrogates (ED) and what lies above U+10FFFF (F4)
    const uint32_t lo = b0 == 0xE0u ? 0xA0u : b0 == 0xF0u ? 0x90u : 0x80u, hi = b0 == 0xEDu ? 0x9Fu : b0 == 0xF4u ? 0x8Fu : 0xBFu;
    const uint32_t b1 = t[i + 1];
    if (b1 < lo || b1 > hi) return 1u;
    uint32_t c = ((b0 & (0x7Fu >> n)) << 6) | (b1 & 0x3Fu);
    if (n > 2u) {
        const uint32_t b2 = t[i + 2];
        if ((b2 & 0xC0u) != 0x80u) return 1u;
        c = (c << 6) | (b2 & 0x3Fu);
    }
    if (n > 3u) {
        const uint32_t b3 = t[i + 3];
        if ((b3 & 0xC0u) != 0x80u) return 1u;
        c = (c << 6) | (b3 & 0x3Fu);
    }
    *sym = c;
    return n;
}

// the width alone
__host__ __device__ __forceinline__ uint32_t utf8_width(const uint8_t *t, uint64_t i, uint64_t tlen) {
    uint32_t sym;
    return utf8_at(t, i, tlen, &sym);
}

// the symbols of t[0 .. tlen)
__host__ __device__ __forceinline__ uint64_t utf8_count(const uint8_t *t, uint64_t tlen) {
    uint64_t n = 0;
    for (uint64_t i = 0; i < tlen; n++) i += utf8_width(t, i, tlen);
    return n;
}

// every byte of t[0 .. tlen) belongs to a well-formed sequence (what a pattern must be under II2_MATCH_UTF8)
__host__ __device__ __forceinline__ bool utf8_well_formed(const uint8_t *t, uint64_t tlen) {
    for (uint64_t i = 0; i < tlen;) {
        uint32_t sym;
        const uint32_t w = utf8_at(t, i, tlen, &sym);
        if (t[i] >= 0x80u && w == 1u) return false;
        i += w;
    }
    return true;
}

}  // namespace ii2
