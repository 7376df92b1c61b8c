// term_device.h — the order of terms (file.CompareTermValues = bytes.Compare, file/types.go:24-26) and the bisections built on
// it, for the device and for the host alike: the alignment (align.hip), the lookup (dict_find.hip) and the host-only
// ii2_term_bounds run these functions and no others.
//
// A dictionary keeps, next to its bytes, every term's first 8 bytes as a big-endian integer, zero padded (the key): most
// comparisons end there; ties go on through the bytes and end with the lengths.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace ii2 {

// a sorted, duplicate-free dictionary: key[n], off[n + 1] byte offsets into bytes
struct TermDict {
    const uint64_t *key;
    const uint64_t *off;
    const uint8_t *bytes;
};

struct TermRef { uint64_t key; const uint8_t *p; uint64_t len; };

// the key of the term p[0 .. len)
__host__ __device__ __forceinline__ uint64_t term_key(const uint8_t *__restrict__ p, uint64_t len) {
    uint64_t kk = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        kk <<= 8;
        if ((uint64_t)j < len) kk |= p[j];
    }
    return kk;
}

// the key of chunk c of the term: bytes [8c, 8c + 8) big-endian, zero padded (chunk 0 is term_key).  bytes.Compare order is the
// order of the tuple (chunk 0, chunk 1, ..., length): a zero byte past a term's end ties with a real one, the length decides.
__host__ __device__ __forceinline__ uint64_t term_chunk(const uint8_t *__restrict__ p, uint64_t len, uint32_t c) {
    const uint64_t at = 8ull * c;
    return at < len ? term_key(p + at, len - at) : 0ull;
}

// bytes.Compare of term (ka, bytes a[0 .. la)) with term (kb, b[0 .. lb)): -1 / 0 / 1.  The keys decide unless they tie.
__host__ __device__ __forceinline__ int term_cmp(uint64_t ka, const uint8_t *__restrict__ a, uint64_t la, uint64_t kb, const uint8_t *__restrict__ b, uint64_t lb, bool long_terms) {
    if (ka != kb) return ka < kb ? -1 : 1;
    if (long_terms) {
        const uint64_t m = la < lb ? la : lb;
        for (uint64_t j = 8; j < m; j++) {
            const uint8_t x = a[j], y = b[j];
            if (x != y) return x < y ? -1 : 1;
        }
    }
    return la == lb ? 0 : (la < lb ? -1 : 1);      // (equal keys, one a prefix of the other — also decides the zero padding)
}

__host__ __device__ __forceinline__ TermRef term_at(const TermDict &d, uint32_t i) {
    const uint64_t b = d.off[i];
    return TermRef{d.key[i], d.bytes + b, d.off[i + 1] - b};
}

// first index in [lo, hi) of the dictionary whose term is > x (upper = true) or >= x (upper = false)
__host__ __device__ __forceinline__ uint32_t term_bound(const TermDict &d, uint32_t lo, uint32_t hi, const TermRef &x, bool upper, bool long_terms) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const TermRef y = term_at(d, mid);
        const int c = term_cmp(y.key, y.p, y.len, x.key, x.p, x.len, long_terms);
        if (c < 0 || (upper && c == 0)) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// the key bits that a prefix of len bytes covers
__host__ __device__ __forceinline__ uint64_t prefix_mask(uint64_t len) { return len >= 8 ? ~0ull : ~(~0ull >> (8 * len)); }

// Is term t before or inside the run of the terms that start with p: t < p, or len(t) >= len(p) and t[0 .. len(p)) == p?  (True
// for a stretch at the front of a sorted dictionary, false behind it: the run ends where this turns false.)  The keys decide
// under the prefix's mask unless they tie there.  The length test is part of it: key "a" zero padded equals the masked key of
// "a\0", yet "a" does not start with "a\0" - it is before it.
__host__ __device__ __forceinline__ bool term_in_prefix_run(const TermRef &t, const TermRef &p) {
    const uint64_t mk = t.key & prefix_mask(p.len);
    if (mk != p.key) return mk < p.key;
    if (t.len < p.len) return term_cmp(t.key, t.p, t.len, p.key, p.p, p.len, true) < 0;      // too short to start with p
    for (uint64_t j = 8; j < p.len; j++) {
        const uint8_t x = t.p[j], y = p.p[j];
        if (x != y) return x < y;
    }
    return true;
}

// first index in [lo, hi) whose term is behind the run of p
__host__ __device__ __forceinline__ uint32_t prefix_run_end(const TermDict &d, uint32_t lo, uint32_t hi, const TermRef &p) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (term_in_prefix_run(term_at(d, mid), p)) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// The answer of one probe in dictionary d of n terms: exact - [j, j + 1) when term j is the probe, else [j, j) at the insertion
// point; prefix - [lower bound, end of the prefix's run).
__host__ __device__ __forceinline__ void term_find(const TermDict &d, uint32_t n, const TermRef &x, bool prefix, uint32_t *first, uint32_t *end) {
    const uint32_t j = term_bound(d, 0u, n, x, false, true);
    *first = j;
    if (prefix) { *end = prefix_run_end(d, j, n, x); return; }
    bool found = false;
    if (j < n) {
        const TermRef y = term_at(d, j);
        found = term_cmp(y.key, y.p, y.len, x.key, x.p, x.len, true) == 0;
    }
    *end = j + (found ? 1u : 0u);
}

}  // namespace ii2
