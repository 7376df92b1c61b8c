// regex_device.h — the regular-expression matcher behind ii2_dict_regex, for the device and for the host alike: k_dict_regex
// (dict_regex.hip) and the host-only ii2_term_regex run these functions and no others.
//
// A pattern is parsed ONCE, on the host (regex_parse), into its Glushkov position automaton: every byte, `.`, class or escape of
// the pattern is one position, numbered in pattern order, and a pattern holds at most II2_REGEX_MAX_POSITIONS = 64 of them after
// its counted repetitions are expanded - so a set of states is one 64-bit word and a term byte costs one load of b[byte] and a
// few integer instructions (regex_step), with no loop over the pattern.  A pattern matches the WHOLE term.  Everything compares
// bytes: no UTF-8; II2_MATCH_NOCASE is resolved in the tables here (only ASCII letters fold) and the term is never folded.
// The syntax is the subset of Python's `re` that include/ii2.h lists; where a pattern is accepted it means what
// re.fullmatch(pattern, term, re.DOTALL) means on bytes.
#pragma once
#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/ii2.h"

namespace ii2 {

constexpr uint32_t REGEX_UNBOUNDED = 0xFFFFFFFFu;

// one parsed pattern: 2608 bytes, 8 of them fill 20.4 KB of LDS
struct RegexPattern {
    uint64_t b[256];                              // bit i: position i accepts the byte
    uint64_t follow[II2_REGEX_MAX_POSITIONS];     // the positions that may come after position i
    uint64_t first, last;                         // the positions a match may start at / end at
    uint64_t lin;                                 // the positions whose follow set is exactly {i + 1}: they advance by a shift
    uint32_t n_pos;                               // positions, <= II2_REGEX_MAX_POSITIONS
    uint32_t nullable;                            // 1: the empty term matches
    uint32_t min_len, max_len;                    // the shortest and the longest term of the language (REGEX_UNBOUNDED: no longest)
    uint32_t pad[2];
};
static_assert(sizeof(RegexPattern) == 2608 && sizeof(RegexPattern) % 16 == 0, "RegexPattern is copied into LDS in 16-byte loads");

// ---- host: the parser ---------------------------------------------------------------------------------------------------------

// a set of bytes
struct RegexSet {
    uint64_t w[4] = {0, 0, 0, 0};
    void add(uint32_t c) { w[c >> 6] |= 1ull << (c & 63u); }
    void add(uint32_t lo, uint32_t hi) { for (uint32_t c = lo; c <= hi; c++) add(c); }
    bool has(uint32_t c) const { return (w[c >> 6] >> (c & 63u)) & 1ull; }
    void merge(const RegexSet &o) { for (int i = 0; i < 4; i++) w[i] |= o.w[i]; }
    void invert() { for (int i = 0; i < 4; i++) w[i] = ~w[i]; }
};

// what Glushkov's construction keeps of a sub-expression
struct RegexFrag {
    uint64_t first = 0, last = 0;
    uint32_t min_len = 0, max_len = 0;
    bool nullable = true;                         // (the default is the empty expression)
};

struct RegexParser {
    const uint8_t *s;
    uint64_t n, i = 0;
    bool nocase;
    RegexPattern *m;
    uint64_t n_pos = 0;                           // counts on above the limit (nothing is stored for such a position)
    int err = 0;                                  // the first II2_EINVAL; the position limit is judged at the end
    uint32_t depth = 0;

    static uint32_t sat_add(uint32_t a, uint32_t b) { return a == REGEX_UNBOUNDED || b == REGEX_UNBOUNDED ? REGEX_UNBOUNDED : a + b; }
    bool more() const { return i < n && !err; }
    bool fail() { if (!err) err = II2_EINVAL; return false; }

    // one position that accepts `set` (as listed: case folding and negation happen here)
    RegexFrag position(RegexSet set, bool negate) {
        if (nocase)
            for (uint32_t c = 'a'; c <= 'z'; c++)
                if (set.has(c) || set.has(c - 32u)) { set.add(c); set.add(c - 32u); }
        if (negate) set.invert();
        RegexFrag f;
        f.nullable = false;
        f.min_len = f.max_len = 1;
        if (n_pos < II2_REGEX_MAX_POSITIONS) {
            const uint64_t bit = 1ull << n_pos;
            for (uint32_t c = 0; c < 256u; c++) if (set.has(c)) m->b[c] |= bit;
            f.first = f.last = bit;
        }
        n_pos++;
        return f;
    }
    void link(uint64_t from, uint64_t to) {
        for (; from; from &= from - 1ull) m->follow[__builtin_ctzll(from)] |= to;
    }
    RegexFrag concat(const RegexFrag &a, const RegexFrag &b) {
        link(a.last, b.first);
        RegexFrag f;
        f.first = a.first | (a.nullable ? b.first : 0);
        f.last = b.last | (b.nullable ? a.last : 0);
        f.nullable = a.nullable && b.nullable;
        f.min_len = a.min_len + b.min_len;
        f.max_len = sat_add(a.max_len, b.max_len);
        return f;
    }
    static RegexFrag either(const RegexFrag &a, const RegexFrag &b) {
        RegexFrag f;
        f.first = a.first | b.first;
        f.last = a.last | b.last;
        f.nullable = a.nullable || b.nullable;
        f.min_len = a.min_len < b.min_len ? a.min_len : b.min_len;
        f.max_len = a.max_len > b.max_len ? a.max_len : b.max_len;
        return f;
    }
    static RegexFrag optional(RegexFrag a) {
        a.nullable = true;
        a.min_len = 0;
        return a;
    }
    RegexFrag repeat(RegexFrag a, bool star) {        // a+ or a*
        link(a.last, a.first);
        if (a.max_len) a.max_len = REGEX_UNBOUNDED;
        return star ? optional(a) : a;
    }

    static int hex(uint8_t c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }
    static bool punct(uint8_t c) { return (c >= 0x21 && c <= 0x2f) || (c >= 0x3a && c <= 0x40) || (c >= 0x5b && c <= 0x60) || (c >= 0x7b && c <= 0x7e); }
    // behind a `\`: the set it names; *single = it is one byte (which may end a range)
    bool escape(RegexSet *set, bool *single) {
        if (i >= n) return fail();
        const uint8_t c = s[i++];
        RegexSet r;
        *single = false;
        switch (c) {
        case 'd': case 'D': r.add('0', '9'); break;
        case 'w': case 'W': r.add('0', '9'); r.add('A', 'Z'); r.add('a', 'z'); r.add('_'); break;
        case 's': case 'S': r.add(' '); r.add('\t', '\r'); break;
        default:
            *single = true;
            if (c == 'n') r.add('\n');
            else if (c == 'r') r.add('\r');
            else if (c == 't') r.add('\t');
            else if (c == 'f') r.add('\f');
            else if (c == 'v') r.add('\v');
            else if (c == 'x') {
                if (i + 2 > n || hex(s[i]) < 0 || hex(s[i + 1]) < 0) return fail();
                r.add((uint32_t)(hex(s[i]) * 16 + hex(s[i + 1])));
                i += 2;
            } else if (punct(c)) r.add(c);
            else return fail();
        }
        if (c == 'D' || c == 'W' || c == 'S') r.invert();
        *set = r;
        return true;
    }
    static uint32_t only(const RegexSet &r) {
        for (uint32_t c = 0; c < 256u; c++) if (r.has(c)) return c;
        return 0;
    }
    // behind a `[`
    RegexFrag bracket() {
        RegexSet set;
        bool negate = false;
        if (i < n && s[i] == '^') { negate = true; i++; }
        for (bool at_front = true;; at_front = false) {
            if (i >= n) { fail(); return {}; }
            uint8_t c = s[i++];
            if (c == ']' && !at_front) break;
            RegexSet lo;
            bool single = true;
            if (c == '\\') { if (!escape(&lo, &single)) return {}; }
            else lo.add(c);
            if (i + 1 < n && s[i] == '-' && s[i + 1] != ']') {        // a range (a `-` in front of the `]` is literal)
                i++;
                RegexSet hi;
                bool hi_single = true;
                c = s[i++];
                if (c == '\\') { if (!escape(&hi, &hi_single)) return {}; }
                else hi.add(c);
                if (!single || !hi_single || only(hi) < only(lo)) { fail(); return {}; }
                set.add(only(lo), only(hi));
            } else set.merge(lo);
        }
        return position(set, negate);
    }

    // a decimal number; false when there is no digit
    bool number(uint64_t *v) {
        if (i >= n || s[i] < '0' || s[i] > '9') return false;
        uint64_t x = 0;
        for (; i < n && s[i] >= '0' && s[i] <= '9'; i++) x = x < (1ull << 24) ? x * 10u + (s[i] - '0') : x;     // (saturates: far above any count that fits)
        *v = x;
        return true;
    }

    RegexFrag atom() {
        const uint8_t c = s[i++];
        if (c == '(') {
            if (i < n && s[i] == '?') {
                if (i + 1 >= n || s[i + 1] != ':') { fail(); return {}; }
                i += 2;
            }
            depth++;
            const RegexFrag f = alternation();
            depth--;
            if (err) return {};
            if (i >= n || s[i] != ')') { fail(); return {}; }
            i++;
            return f;
        }
        if (c == '[') return bracket();
        RegexSet set;
        if (c == '.') { set.invert(); return position(set, false); }
        if (c == '\\') {
            bool single;
            if (!escape(&set, &single)) return {};
            return position(set, false);
        }
        if (c == '*' || c == '+' || c == '?' || c == '{' || c == '^' || c == '$' || c == ')') { fail(); return {}; }
        set.add(c);
        return position(set, false);
    }

    // forget the positions from `keep` on (x{0}: the atom was parsed to find its end)
    void forget(uint64_t keep) {
        if (keep < II2_REGEX_MAX_POSITIONS) {
            const uint64_t below = (1ull << keep) - 1ull;
            for (uint32_t c = 0; c < 256u; c++) m->b[c] &= below;
            for (uint32_t p = 0; p < II2_REGEX_MAX_POSITIONS; p++) m->follow[p] = p < keep ? m->follow[p] & below : 0;
        }
        n_pos = keep;
    }

    RegexFrag quantified() {
        const uint64_t at = i, pos0 = n_pos;
        RegexFrag f = atom();
        if (err) return {};
        const uint64_t per = n_pos - pos0;
        if (i >= n) return f;
        const uint8_t q = s[i];
        if (q != '*' && q != '+' && q != '?' && q != '{') return f;
        i++;
        if (q == '*' || q == '+') f = repeat(f, q == '*');
        else if (q == '?') f = optional(f);
        else {
            uint64_t lo, hi;
            bool open = false;
            if (!number(&lo)) { fail(); return {}; }
            hi = lo;
            if (i < n && s[i] == ',') {
                i++;
                if (!number(&hi)) open = true;
            }
            if (i >= n || s[i] != '}' || (!open && hi < lo)) { fail(); return {}; }
            i++;
            const uint64_t after = i;
            // x{m,n}: m copies and n - m nested optionals (x(x(...)?)?)?; x{m,}: m copies and x*.  An atom without a position
            // holds the empty string alone, whatever its count.
            const uint64_t copies = open ? lo + 1 : hi;
            if (per == 0) {
            } else if (copies == 0) {
                forget(pos0);
                f = RegexFrag();
            } else if (pos0 + per * copies > II2_REGEX_MAX_POSITIONS) {
                n_pos = pos0 + per * copies;            // too many: counted, not built
                if (n_pos > (1ull << 24)) n_pos = 1ull << 24;
                f = RegexFrag();
            } else {
                std::vector<RegexFrag> c(copies);       // (on the heap: the parser recurses once per nested group)
                c[0] = f;
                for (uint64_t j = 1; j < copies; j++) { i = at; c[j] = atom(); }
                RegexFrag tail;
                if (open) tail = repeat(c[copies - 1], true);
                else for (uint64_t j = hi; j > lo; j--) tail = optional(concat(c[j - 1], tail));
                for (uint64_t j = lo; j > 0; j--) tail = concat(c[j - 1], tail);
                f = tail;
                i = after;
            }
        }
        if (i < n && s[i] == '?') i++;                  // lazy: the same whole-term matches
        if (i < n && (s[i] == '*' || s[i] == '+' || s[i] == '?' || s[i] == '{')) { fail(); return {}; }
        return f;
    }

    RegexFrag sequence() {
        RegexFrag f;
        while (more() && s[i] != '|' && !(s[i] == ')' && depth)) f = concat(f, quantified());
        return f;
    }
    RegexFrag alternation() {
        RegexFrag f = sequence();
        while (more() && s[i] == '|') {
            i++;
            f = either(f, sequence());
        }
        return f;
    }
};

// host: raw pattern bytes -> RegexPattern.  II2_EINVAL for a flag bit other than II2_MATCH_NOCASE or a pattern outside the
// syntax, II2_ERANGE above II2_REGEX_MAX_PATTERN bytes or II2_REGEX_MAX_POSITIONS positions.  *n_pos (may be NULL) = the
// pattern's positions whenever the syntax holds, also when they are too many.
inline int regex_parse(uint32_t flags, const uint8_t *pat, uint64_t pat_len, RegexPattern *out, uint32_t *n_pos = nullptr) {
    if (flags & ~(uint32_t)II2_MATCH_NOCASE) return II2_EINVAL;
    if (pat_len > II2_REGEX_MAX_PATTERN) return II2_ERANGE;
    RegexPattern m = {};
    RegexParser ps{pat, pat_len, 0, (flags & II2_MATCH_NOCASE) != 0, &m};
    const RegexFrag f = ps.alternation();
    if (ps.err) return ps.err;
    if (ps.i != pat_len) return II2_EINVAL;
    if (n_pos) *n_pos = (uint32_t)(ps.n_pos < REGEX_UNBOUNDED ? ps.n_pos : REGEX_UNBOUNDED);
    if (ps.n_pos > II2_REGEX_MAX_POSITIONS) return II2_ERANGE;
    m.first = f.first;
    m.last = f.last;
    m.n_pos = (uint32_t)ps.n_pos;
    m.nullable = f.nullable ? 1 : 0;
    m.min_len = f.min_len;
    m.max_len = f.max_len;
    for (uint32_t p = 0; p + 1 < m.n_pos; p++)
        if (m.follow[p] == 1ull << (p + 1)) m.lin |= 1ull << p;
    *out = m;
    return II2_OK;
}

// ---- host and device: the matcher -----------------------------------------------------------------------------------------------

// the filter in front of the automaton: the term's length lies between the language's shortest and longest
__host__ __device__ __forceinline__ bool regex_passes(const RegexPattern &m, uint64_t tlen) {
    return tlen >= m.min_len && (m.max_len == REGEX_UNBOUNDED || tlen <= m.max_len);
}

// the states after byte c, from the states D: the positions of `lin` advance by a shift, the others OR their follow sets in
__host__ __device__ __forceinline__ uint64_t regex_step(const RegexPattern &m, uint64_t D, uint8_t c) {
    uint64_t next = (D & m.lin) << 1;
    for (uint64_t rest = D & ~m.lin; rest; rest &= rest - 1ull) next |= m.follow[__builtin_ctzll(rest)];
    return next & m.b[c];
}

// pattern m against one term.  *tested = the pair passed the length filter.
__host__ __device__ __forceinline__ bool regex_term(const RegexPattern &m, const uint8_t *t, uint64_t tlen, bool *tested) {
    *tested = regex_passes(m, tlen);
    if (!*tested) return false;
    if (tlen == 0) return m.nullable != 0;
    uint64_t D = m.first & m.b[t[0]];
    for (uint64_t j = 1; j < tlen && D; j++) D = regex_step(m, D, t[j]);
    return (D & m.last) != 0;
}

}  // namespace ii2
