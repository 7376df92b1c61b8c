// host_index.cpp — host-side mirror of the reference's Shard / InvertedIndex operations above
// the C ABI (include/ii2.h).  The reference is Go; this image has no Go toolchain, so the host
// layer is C++ with the reference's names, argument meaning and error behaviour, and the posting
// work of every operation goes to the GPU through the same entry points a cgo binding would
// use.  Segments live in HBM (DV1); term dictionaries are plain sorted byte strings here (the
// reference's vellum FST, locks and pools are out of scope — SURVEY.md §8).  A shard opened on a
// directory keeps its segments and its removed list on disk as well (segment_file.h: the `file`
// package's Writer / Reader / RemoveSegment and the removed.list persistence).
//
//   Shard.Put / Read / Remove / Merge / MinMax      shard.go:33-298
//   Shard.PutBatch / InvertedIndex.PutBatch          additive: many Puts as ONE merged-quality segment per shard (ii2_seg_build)
//   NewShard (load existing files, removed.list)     shard.go:300-358
//   file.Writer / Reader / RemoveSegment             file/writer.go, file/reader.go
//   Segments.add ordering                            segments.go:56-64
//   RemovedLists.Put / Values / Sync                 removed_list.go:36-71
//   InvertedIndex.Put / Read / Merge / PutRemoved / PrefixSearch   inverted_index.go:41-340
//   shardKey                                         shard.go:362-378
//   Intersect(terms)                                 additive
//   IntersectExcept(terms, except)                   additive: Intersect minus the ids under any excluded term
//   IntersectAtLeast(terms, min_match, except)       additive: the ids under at least min_match of the terms, minus the excluded terms
//   IntersectTop(terms, k, min_match, except)        additive: the k ids under the most of the terms, with their scores, in rank order
//   IntersectTopWeighted(terms, weights, k, min_score, except)   additive: the same with a weight per term, the score their sum
//   IntersectTopBatch(queries)                       additive: many IntersectTopWeighted queries in one device call
//   IntersectMany(queries)                           additive: many IntersectExcept queries in one device call
//   TermCounts(prefix, terms, except)                additive: per term under a prefix, the docs of IntersectExcept under it (facets)
//   Histogram(terms, except, edges)                  additive: the docs of IntersectExcept per value bucket (ii2_histogram_ids)
//   TermHistogram(prefix, terms, except, edges)      additive: TermCounts per value bucket (ii2_histogram_ranges)
//   MatchedTerms(ids, terms)                         additive: per id, which of the terms it lies under (ii2_explain_ranges)
//   MatchedTermsBatch(pages)                         additive: MatchedTerms for many (ids, terms) pages in one device call (ii2_explain_batch)
//   MatchSearch(patterns, kind) / MatchTerms(pattern, kind, limit)   additive: substring, suffix and wildcard search (ii2_dict_match)
//   FuzzySearch(terms, max_dist, prefix, flags) / FuzzyTerms(pattern, max_dist, prefix, flags, limit)   additive: typo-tolerant search (ii2_dict_fuzzy)
//   RegexSearch(patterns, flags) / RegexTerms(pattern, flags, limit)   additive: regular-expression search (ii2_dict_regex)
//   SetResolve(mode)                                 additive: the two bulk calls look their terms up on the host or on the device (ii2_dict_find)
//   SetFirstCap(ids) / SecondCalls()                 additive, for the tests: the first buffer of the calls that may need a second one (two_call)
//   SetBuild(mode)                                   additive: PutBatch sorts and looks up its terms on the host or on the device (ii2_dict_build)
//
// Built as its own library (libii2_host.so) that only sees include/ii2.h and links libii2_hip.so:
// the product library exports the C ABI and nothing else.  A small C facade (ii2h_*) at the bottom
// lets the Python tests replay the reference's test scripts against this layer.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/ii2.h"
#include "segment_file.h"

namespace ii2h {

using Term = std::string;      // raw bytes; std::string compares like bytes.Compare (unsigned char order)

struct TermValues {            // file/types.go:9-12
    Term term;
    std::vector<uint32_t> values;
};

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

static void ck(ii2_ctx *ctx, int rc, const char *what) {
    if (rc) throw Error(std::string(what) + ": " + ii2_last_error(ctx));     // fmt.Errorf("…: %w", err)
}

static bool term_less(const Term &a, const Term &b) {
    const size_t m = std::min(a.size(), b.size());
    const int c = m ? std::memcmp(a.data(), b.data(), m) : 0;
    return c ? c < 0 : a.size() < b.size();
}

struct SegHandle {
    ii2_seg *h = nullptr;
    explicit SegHandle(ii2_seg *s) : h(s) {}
    ~SegHandle() { ii2_seg_free(h); }
    SegHandle(const SegHandle &) = delete;
};

struct DevMem {                // device buffer freed at scope exit
    ii2_ctx *ctx;
    void *p = nullptr;
    explicit DevMem(ii2_ctx *c) : ctx(c) {}
    ~DevMem() { if (p) ii2_dev_free(ctx, p); }
    DevMem(DevMem &&o) : ctx(o.ctx), p(o.p) { o.p = nullptr; }
    DevMem &operator=(DevMem &&o) { std::swap(ctx, o.ctx); std::swap(p, o.p); return *this; }
};
struct TombHandle {
    ii2_tomb *h = nullptr;
    ~TombHandle() { ii2_tomb_free(h); }
};

struct DictHandle {
    ii2_dict *h = nullptr;
    ~DictHandle() { ii2_dict_free(h); }
};

struct Segment {               // segments.go:16-24
    int64_t key;               // unix-ns key
    std::vector<Term> terms;   // sorted
    std::shared_ptr<SegHandle> seg;   // terms.size() lists
    bool merging = false;
    // `terms` resident in HBM for ii2_dict_find: made on the first device lookup of this segment, once, and freed with it (a
    // segment that is never looked up in bulk has none)
    mutable std::unique_ptr<DictHandle> dict;
    const ii2_dict *resident_dict(ii2_ctx *ctx) const {
        static std::mutex mu;  // (first lookups are rare: one lock for all segments keeps Segment movable)
        std::lock_guard<std::mutex> g(mu);
        if (!dict) {
            std::vector<uint8_t> bytes;
            std::vector<uint64_t> off(terms.size() + 1, 0);
            for (size_t i = 0; i < terms.size(); i++) {
                bytes.insert(bytes.end(), terms[i].begin(), terms[i].end());
                off[i + 1] = bytes.size();
            }
            auto d = std::make_unique<DictHandle>();
            ck(ctx, ii2_dict_create(ctx, bytes.data(), off.data(), terms.size(), II2_HOST, &d->h), "resolve: dictionary");
            dict = std::move(d);
        }
        return dict->h;
    }
};

static int64_t now_ns() {      // strictly increasing across threads (segment keys order the tombstone batches)
    static std::mutex mu;
    static int64_t last = 0;
    std::lock_guard<std::mutex> g(mu);
    int64_t t = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::system_clock::now().time_since_epoch()).count();
    if (t <= last) t = last + 1;
    last = t;
    return t;
}

// ---- the two-call output protocol (InvertedIndex::two_call; Shard::MatchSearch) ----
// No call allocates more than first_cap ids at first: a result that does not fit is written by a second call with the size the
// first one reported (II2_ECAPACITY writes nothing; the batch calls fill their offsets under it).  Either call passes one entry
// more than it needs.  `arrays`: the uint32 arrays of `cap` entries the output holds, back to back.  call(d_out, cap, &n) makes
// the library call and returns its rc, n = the size it reported.  *second_calls (may be null) counts the retries.
constexpr uint64_t FIRST_CAP_IDS = 1ull << 22;
struct DevOutput {
    DevMem mem;
    uint64_t cap, n;           // entries per array, entries written
};
template <class Call> static DevOutput two_call_dev(ii2_ctx *ctx, uint64_t first_cap, std::atomic<uint64_t> *second_calls, uint64_t bound, unsigned arrays,
                                                    const char *what, Call call) {
    DevOutput o{DevMem(ctx), std::min(bound, first_cap) + 1, 0};
    for (int attempt = 0;; attempt++) {
        ck(ctx, ii2_dev_alloc(ctx, arrays * o.cap * sizeof(uint32_t), &o.mem.p), what);
        const int rc = call((uint32_t *)o.mem.p, o.cap, &o.n);
        if (rc != II2_ECAPACITY || attempt) {
            ck(ctx, rc, what);
            return o;
        }
        if (second_calls) (*second_calls)++;
        ck(ctx, ii2_dev_free(ctx, o.mem.p), what);
        o.mem.p = nullptr;
        o.cap = o.n + 1;
    }
}

// ---- one union per name over list ranges (MatchSearch; InvertedIndex::PrefixSearch keeps its own copy of this loop, which
// tests/test_query_batch_cpu.py pins inside its body, and shares the bound) ----
struct NamedRanges {
    std::vector<const ii2_seg *> segs;
    std::vector<uint64_t> first, end;
};
// The ids a union over ranges in `segs` (the segment of each range) can give at most: the postings of every DISTINCT segment,
// once.  A prefix has one range per segment, a substring search any number of runs in one, and however many they are they hold
// no more postings than the segment does.  postings(seg): that segment's count.
template <class Seg, class Postings> static uint64_t union_bound(std::vector<Seg> segs, Postings postings) {
    std::sort(segs.begin(), segs.end(), std::less<Seg>());
    segs.erase(std::unique(segs.begin(), segs.end()), segs.end());
    uint64_t b = 0;
    for (const Seg &s : segs) b += postings(s);
    return b;
}
static uint64_t seg_postings(const ii2_seg *h) {
    ii2_seg_info info;
    ii2_seg_get_info(h, &info);
    return info.n_postings;
}
// ONE ii2_query_batch call, one wait and one download for all the names (an OR query each), through two_call(bound, call).  The
// output's size: the C ABI gives no per-list counts, so a name is bounded by the postings of the segments its ranges lie in
// (union_bound).  Names whose bounds add up to the call's limit of 2^32 ids go in several calls; one that reaches it alone goes
// through ii2_union_ranges.
template <class TwoCall> static std::map<Term, std::vector<uint32_t>> or_per_name(ii2_ctx *ctx, const std::map<Term, NamedRanges> &found, const char *what,
                                                                                  TwoCall two_call) {
    std::map<Term, std::vector<uint32_t>> out;
    auto download = [&](const DevMem &d, uint64_t n) {
        std::vector<uint32_t> v(n);
        if (n) ck(ctx, ii2_copy_d2h(ctx, v.data(), d.p, n * sizeof(uint32_t)), what);
        return v;
    };
    constexpr uint64_t CALL_IDS = 0xFFFFFFFFull;
    auto it = found.begin();
    while (it != found.end()) {
        std::vector<const Term *> names;
        std::vector<uint8_t> op;
        std::vector<uint64_t> query_first{0}, first, end;
        std::vector<const ii2_seg *> segs;
        uint64_t bound = 0;
        for (; it != found.end(); ++it) {
            const NamedRanges &r = it->second;
            const uint64_t b = union_bound(r.segs, seg_postings);
            if (!names.empty() && bound + b >= CALL_IDS) break;
            bound += b;
            names.push_back(&it->first);
            op.push_back(II2_OP_OR);
            segs.insert(segs.end(), r.segs.begin(), r.segs.end());
            first.insert(first.end(), r.first.begin(), r.first.end());
            end.insert(end.end(), r.end.begin(), r.end.end());
            query_first.push_back(segs.size());
        }
        if (bound >= CALL_IDS) {                                          // (one name, alone in its call)
            DevMem d_out(ctx);
            uint64_t n = 0;
            ck(ctx, ii2_dev_alloc(ctx, (bound + 1) * sizeof(uint32_t), &d_out.p), what);
            ck(ctx, ii2_union_ranges(ctx, segs.size(), segs.data(), first.data(), end.data(), nullptr, (uint32_t *)d_out.p, bound + 1, &n), what);
            out[*names[0]] = download(d_out, n);
            continue;
        }
        std::vector<uint64_t> off(names.size() + 1, 0);
        const DevOutput o = two_call(bound, [&](uint32_t *d_ids, uint64_t cap, uint64_t *n) {
            const int rc = ii2_query_batch(ctx, names.size(), op.data(), query_first.data(), segs.data(), first.data(), end.data(), nullptr, d_ids, cap,
                                           off.data());
            *n = off.back();
            return rc;
        });
        const std::vector<uint32_t> all = download(o.mem, o.n);          // sort + compact, on the GPU
        for (size_t q = 0; q < names.size(); q++) out[*names[q]] = std::vector<uint32_t>(all.begin() + off[q], all.begin() + off[q + 1]);
    }
    return out;
}

// ---- term search over the resident dictionaries: what substring and typo-tolerant search share ----
// fn(pattern index, segment, j0, j1) for every run [j0, j1) of consecutive terms of every segment that `patterns[p]` matches,
// with no host pass over the terms: the segments' resident dictionaries in chunks of at most II2_MAX_LISTS, the patterns in
// chunks of at most max_patterns.  call(p0, np, k, dicts, bytes, off, run_off, first, end, which, cap) makes the ABI call for
// patterns [p0, p0 + np) - its per-pattern arrays are its own - and returns its code; a result above the first buffer takes the
// second call that II2_ECAPACITY asks for.  Per pattern the runs come segment by segment, ascending inside one.
template <class Call, class Fn> static void term_runs(ii2_ctx *ctx, const std::vector<std::shared_ptr<Segment>> &segs, const std::vector<Term> &patterns,
                                                      size_t max_patterns, const char *what, Call call, Fn fn) {
    for (size_t p0 = 0; p0 < patterns.size(); p0 += max_patterns) {
        const size_t np = std::min(max_patterns, patterns.size() - p0);
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> off(np + 1, 0);
        for (size_t p = 0; p < np; p++) {
            bytes.insert(bytes.end(), patterns[p0 + p].begin(), patterns[p0 + p].end());
            off[p + 1] = bytes.size();
        }
        bytes.push_back(0);                                               // (never empty)
        for (size_t s0 = 0; s0 < segs.size(); s0 += II2_MAX_LISTS) {
            const size_t k = std::min<size_t>(II2_MAX_LISTS, segs.size() - s0);
            std::vector<const ii2_dict *> dicts;
            for (size_t s = 0; s < k; s++) dicts.push_back(segs[s0 + s]->resident_dict(ctx));
            std::vector<uint64_t> run_off(np * k + 1, 0), first, end;
            std::vector<uint32_t> which;
            uint64_t cap = 4096;
            for (int attempt = 0;; attempt++) {
                first.resize(cap);
                end.resize(cap);
                which.resize(cap);
                const int rc = call(p0, np, (uint32_t)k, dicts.data(), bytes.data(), off.data(), run_off.data(), first.data(), end.data(), which.data(), cap);
                if (rc != II2_ECAPACITY || attempt) {
                    ck(ctx, rc, what);
                    break;
                }
                cap = run_off.back();
            }
            for (size_t p = 0; p < np; p++)
                for (uint64_t j = run_off[p * k]; j < run_off[(p + 1) * k]; j++) fn(p0 + p, segs[s0 + which[j]], (size_t)first[j], (size_t)end[j]);
        }
    }
}
// map<pattern, ids>: the distinct patterns' runs - runs(patterns, fn) is match_runs or fuzzy_runs with its own arguments bound -
// then ONE batch of OR queries, one per pattern (or_per_name).  A pattern that matches no term has no entry.  No tombstone
// filter, as in Read.
template <class Runs, class TwoCall> static std::map<Term, std::vector<uint32_t>> runs_search(ii2_ctx *ctx, std::vector<Term> patterns, const char *what,
                                                                                              Runs runs, TwoCall two_call) {
    std::sort(patterns.begin(), patterns.end(), term_less);
    patterns.erase(std::unique(patterns.begin(), patterns.end()), patterns.end());
    std::map<Term, NamedRanges> found;
    runs(patterns, [&](size_t p, const std::shared_ptr<Segment> &sg, size_t j0, size_t j1) {
        NamedRanges &r = found[patterns[p]];
        r.segs.push_back(sg->seg->h);
        r.first.push_back(j0);
        r.end.push_back(j1);
    });
    return or_per_name(ctx, found, what, two_call);
}

// ---- substring, suffix and wildcard search (additive: the reference's FST walks a term from its front only) ----
// term_runs for the patterns of `kind` (II2_MATCH_*, | II2_MATCH_NOCASE, | II2_MATCH_UTF8: passed through): ii2_dict_match
template <class Fn> static void match_runs(ii2_ctx *ctx, const std::vector<std::shared_ptr<Segment>> &segs, const std::vector<Term> &patterns, uint32_t kind,
                                           Fn fn) {
    term_runs(ctx, segs, patterns, II2_MATCH_MAX_PATTERNS, "match search",
              [&](size_t, size_t np, uint32_t k, const ii2_dict *const *dicts, const uint8_t *bytes, const uint64_t *off, uint64_t *run_off, uint64_t *first,
                  uint64_t *end, uint32_t *which, uint64_t cap) {
                  const std::vector<uint8_t> kinds(np, (uint8_t)kind);
                  return ii2_dict_match(ctx, k, dicts, (uint32_t)np, bytes, off, kinds.data(), run_off, first, end, which, cap, nullptr);
              }, fn);
}
template <class TwoCall> static std::map<Term, std::vector<uint32_t>> match_search(ii2_ctx *ctx, const std::vector<std::shared_ptr<Segment>> &segs,
                                                                                   std::vector<Term> patterns, uint32_t kind, TwoCall two_call) {
    return runs_search(ctx, std::move(patterns), "match search", [&](const std::vector<Term> &distinct, auto fn) { match_runs(ctx, segs, distinct, kind, fn); },
                       two_call);
}
// the distinct terms of `segs` that the pattern matches, in bytes.Compare order, at most `limit`: read from the runs
static std::vector<Term> match_terms(ii2_ctx *ctx, const std::vector<std::shared_ptr<Segment>> &segs, const Term &pattern, uint32_t kind, uint64_t limit) {
    std::vector<Term> out;
    match_runs(ctx, segs, {pattern}, kind, [&](size_t, const std::shared_ptr<Segment> &sg, size_t j0, size_t j1) {
        out.insert(out.end(), sg->terms.begin() + j0, sg->terms.begin() + j1);
    });
    std::sort(out.begin(), out.end(), term_less);
    out.erase(std::unique(out.begin(), out.end()), out.end());
    if (out.size() > limit) out.resize(limit);
    return out;
}

// ---- typo-tolerant search (additive: what the reference's dictionary library answers with a Levenshtein automaton) ----
// term_runs for the terms within `max_dist` edits of a pattern that share its first `prefix` bytes (flags: II2_FUZZY_TRANSPOSE,
// II2_MATCH_NOCASE, II2_MATCH_UTF8 - then edits and prefix count UTF-8 symbols): ii2_dict_fuzzy.  A pattern shorter than the prefix,
// in bytes or under II2_MATCH_UTF8 in symbols, is compared as a whole.
template <class Fn> static void fuzzy_runs(ii2_ctx *ctx, const std::vector<std::shared_ptr<Segment>> &segs, const std::vector<Term> &patterns, uint32_t max_dist,
                                           uint32_t prefix, uint32_t flags, Fn fn) {
    if (max_dist > 255 || flags > 255) throw Error("fuzzy search: max_dist and flags are at most 255");
    term_runs(ctx, segs, patterns, II2_FUZZY_MAX_PATTERNS, "fuzzy search",
              [&](size_t p0, size_t np, uint32_t k, const ii2_dict *const *dicts, const uint8_t *bytes, const uint64_t *off, uint64_t *run_off, uint64_t *first,
                  uint64_t *end, uint32_t *which, uint64_t cap) {
                  const std::vector<uint8_t> dist(np, (uint8_t)max_dist), fl(np, (uint8_t)flags);
                  std::vector<uint8_t> pre(np);
                  for (size_t p = 0; p < np; p++) {
                      const Term &pat = patterns[p0 + p];
                      uint64_t positions = pat.size();
                      if (flags & II2_MATCH_UTF8)
                          ck(ctx, ii2_utf8_decode((const uint8_t *)pat.data(), pat.size(), nullptr, 0, &positions, nullptr), "fuzzy search");
                      pre[p] = (uint8_t)std::min<uint64_t>(prefix, positions);
                  }
                  return ii2_dict_fuzzy(ctx, k, dicts, (uint32_t)np, bytes, off, dist.data(), pre.data(), fl.data(), run_off, first, end, which, cap, nullptr);
              }, fn);
}
// (the names are query terms here: ids under any term within distance)
template <class TwoCall> static std::map<Term, std::vector<uint32_t>> fuzzy_search(ii2_ctx *ctx, const std::vector<std::shared_ptr<Segment>> &segs,
                                                                                   std::vector<Term> terms, uint32_t max_dist, uint32_t prefix, uint32_t flags,
                                                                                   TwoCall two_call) {
    return runs_search(ctx, std::move(terms), "fuzzy search",
                       [&](const std::vector<Term> &distinct, auto fn) { fuzzy_runs(ctx, segs, distinct, max_dist, prefix, flags, fn); }, two_call);
}
// the distinct terms of `segs` within distance of the pattern with their distances, distance ascending, then bytes ascending, at
// most `limit`: the terms are read from the runs, and only those get their distance, from ii2_term_fuzzy on the host
static std::vector<std::pair<Term, uint32_t>> fuzzy_terms(ii2_ctx *ctx, const std::vector<std::shared_ptr<Segment>> &segs, const Term &pattern,
                                                          uint32_t max_dist, uint32_t prefix, uint32_t flags, uint64_t limit) {
    std::vector<Term> hit;
    fuzzy_runs(ctx, segs, {pattern}, max_dist, prefix, flags, [&](size_t, const std::shared_ptr<Segment> &sg, size_t j0, size_t j1) {
        hit.insert(hit.end(), sg->terms.begin() + j0, sg->terms.begin() + j1);
    });
    std::sort(hit.begin(), hit.end(), term_less);
    hit.erase(std::unique(hit.begin(), hit.end()), hit.end());
    std::vector<std::pair<Term, uint32_t>> out;
    for (const Term &t : hit) {
        int match = 0;
        uint32_t dist = 0;
        ck(ctx, ii2_term_fuzzy(flags, (const uint8_t *)pattern.data(), pattern.size(), 0, max_dist, (const uint8_t *)t.data(), t.size(), &match, &dist),
           "fuzzy terms");
        out.emplace_back(t, dist);
    }
    std::stable_sort(out.begin(), out.end(), [](const std::pair<Term, uint32_t> &a, const std::pair<Term, uint32_t> &b) { return a.second < b.second; });
    if (out.size() > limit) out.resize(limit);
    return out;
}

// ---- regular-expression search (additive: what the reference's dictionary library answers with a regex automaton over the FST) ----
// term_runs for the terms a pattern matches as a whole (flags: 0 or II2_MATCH_NOCASE; the syntax is include/ii2.h's): ii2_dict_regex
// in chunks of II2_REGEX_MAX_PATTERNS patterns.  Every pattern is parsed on the host first (ii2_term_regex), so that one that
// does not parse fails the whole call, with the library's return code, before any search runs.
template <class Fn> static void regex_runs(ii2_ctx *ctx, const std::vector<std::shared_ptr<Segment>> &segs, const std::vector<Term> &patterns, uint32_t flags,
                                           Fn fn) {
    if (flags > 255) throw Error("regex search: flags are at most 255");      // (they travel as one byte per pattern below)
    for (const Term &p : patterns) {
        int match = 0;
        uint32_t n_pos = 0;
        const int rc = ii2_term_regex(flags, (const uint8_t *)p.data(), p.size(), nullptr, 0, &match, &n_pos);
        if (rc)             // (ii2_term_regex has no context to leave a text in: the code it returned, and the count behind II2_ERANGE)
            throw Error("regex search: ii2_term_regex returned " + std::to_string(rc) + (rc == II2_ERANGE ? " (II2_ERANGE: " + std::to_string(p.size()) +
                        " bytes, " + std::to_string(n_pos) + " positions)" : rc == II2_EINVAL ? " (II2_EINVAL)" : "") + " for the pattern " + p);
    }
    term_runs(ctx, segs, patterns, II2_REGEX_MAX_PATTERNS, "regex search",
              [&](size_t, size_t np, uint32_t k, const ii2_dict *const *dicts, const uint8_t *bytes, const uint64_t *off, uint64_t *run_off, uint64_t *first,
                  uint64_t *end, uint32_t *which, uint64_t cap) {
                  const std::vector<uint8_t> fl(np, (uint8_t)flags);
                  return ii2_dict_regex(ctx, k, dicts, (uint32_t)np, bytes, off, fl.data(), run_off, first, end, which, cap, nullptr);
              }, fn);
}
template <class TwoCall> static std::map<Term, std::vector<uint32_t>> regex_search(ii2_ctx *ctx, const std::vector<std::shared_ptr<Segment>> &segs,
                                                                                   std::vector<Term> patterns, uint32_t flags, TwoCall two_call) {
    return runs_search(ctx, std::move(patterns), "regex search", [&](const std::vector<Term> &distinct, auto fn) { regex_runs(ctx, segs, distinct, flags, fn); },
                       two_call);
}
// the distinct terms of `segs` that the pattern matches, in bytes.Compare order, at most `limit`: read from the runs
static std::vector<Term> regex_terms(ii2_ctx *ctx, const std::vector<std::shared_ptr<Segment>> &segs, const Term &pattern, uint32_t flags, uint64_t limit) {
    std::vector<Term> out;
    regex_runs(ctx, segs, {pattern}, flags, [&](size_t, const std::shared_ptr<Segment> &sg, size_t j0, size_t j1) {
        out.insert(out.end(), sg->terms.begin() + j0, sg->terms.begin() + j1);
    });
    std::sort(out.begin(), out.end(), term_less);
    out.erase(std::unique(out.begin(), out.end()), out.end());
    if (out.size() > limit) out.resize(limit);
    return out;
}

// ---- file.Writer / file.Reader over segment_file.h (file/writer.go, file/reader.go) -----------------------------
// The encode and decode steps run on the device through the C ABI (ii2_seg_encode / ii2_seg_import + ii2_seg_decode):
// there is no host codec in the product.
class Writer {
   public:
    // file/writer.go:122-136 (NewWriter) and :95-120 (NewDirectWriter)
    Writer(ii2_ctx *ctx, std::string dir, bool direct) : ctx_(ctx), dir_(std::move(dir)), direct_(direct), key_(std::to_string(now_ns())) {}
    // terms must ascend (file/writer.go:30); direct mode keeps Values[0] only (:34-40)
    void Append(const TermValues &tv) {
        if (closed_) throw Error("writer: append after close");
        if (direct_ && tv.values.empty()) throw Error("writer: fst insert: direct mode needs one value per term");
        terms_.push_back(tv.term);
        if (direct_) vals_.push_back(tv.values[0]);
        else vals_.insert(vals_.end(), tv.values.begin(), tv.values.end());
        off_.push_back(vals_.size());
    }
    // file/writer.go:61-90: both files appear under their final names only here
    void Close() {
        if (closed_) return;
        closed_ = true;
        file::TermFile tf;
        tf.terms = std::move(terms_);
        tf.direct = direct_;
        if (direct_) tf.direct_vals = vals_;
        file::write_terms(dir_, key_, tf);
        const uint64_t n_terms = tf.terms.size();
        if (!direct_) {
            ii2_seg *s = nullptr;
            ck(ctx_, ii2_seg_encode(ctx_, n_terms, off_.data(), vals_.data(), II2_HOST, &s), "writer: encode");
            SegHandle seg(s);
            file::write_dv1(dir_, key_, export_dv1(ctx_, s));
            file::commit(file::dv1_path(dir_, key_));
        }
        file::commit(file::tdx_path(dir_, key_));
    }
    const std::string &GetKey() const { return key_; }

    static file::Dv1File export_dv1(ii2_ctx *ctx, const ii2_seg *s) {
        ii2_seg_info info;
        ii2_seg_get_info(s, &info);
        file::Dv1File d;
        d.n_lists = info.n_lists;
        d.n_postings = info.n_postings;
        d.blk_off.resize(info.n_lists + 1);
        d.skip.resize(info.n_blocks + 1);
        d.payload.resize(info.n_bytes);
        ck(ctx, ii2_seg_export(ctx, s, d.blk_off.data(), d.skip.data(), d.payload.empty() ? nullptr : d.payload.data()), "writer: export");
        return d;
    }

   private:
    ii2_ctx *ctx_;
    std::string dir_;
    bool direct_;
    std::string key_;
    bool closed_ = false;
    std::vector<Term> terms_;
    std::vector<uint32_t> vals_;
    std::vector<uint64_t> off_{0};
};

// a segment file pair brought to the device: the term dictionary on the host, the lists as an ii2_seg
struct LoadedSegment {
    std::vector<Term> terms;
    ii2_seg *seg = nullptr;        // caller owns
};
static LoadedSegment load_segment(ii2_ctx *ctx, const std::string &dir, const std::string &key) {
    LoadedSegment out;
    file::TermFile tf = file::read_terms(dir, key);
    const uint64_t n = tf.terms.size();
    if (tf.direct) {
        std::vector<uint64_t> off(n + 1);
        for (uint64_t i = 0; i <= n; i++) off[i] = i;
        ck(ctx, ii2_seg_encode(ctx, n, off.data(), tf.direct_vals.data(), II2_HOST, &out.seg), "reader: encode");
    } else {
        file::Dv1File d = file::read_dv1(dir, key);
        if (d.n_lists != n) throw Error("reader: " + key + ": term file and value file disagree on the term count");
        ck(ctx, ii2_seg_import(ctx, d.n_lists, d.n_postings, d.skip.size() - 1, d.payload.size(), d.blk_off.data(), d.skip.data(),
                               d.payload.empty() ? nullptr : d.payload.data(), II2_HOST, &out.seg), "reader: values file");
    }
    out.terms = std::move(tf.terms);
    return out;
}

class Reader {
   public:
    struct NothingInRange {};      // vellum.ErrIteratorDone from NewReader: the shard skips the segment (shard.go:257-261)
    // file/reader.go:136-199: min / max inclusive, nullptr = open
    Reader(ii2_ctx *ctx, const std::string &dir, const std::string &key, const Term *min, const Term *max) {
        LoadedSegment ls = load_segment(ctx, dir, key);
        SegHandle seg(ls.seg);
        terms_ = std::move(ls.terms);
        at_ = min ? std::lower_bound(terms_.begin(), terms_.end(), *min, term_less) - terms_.begin() : 0;
        end_ = max ? std::upper_bound(terms_.begin(), terms_.end(), *max, term_less) - terms_.begin() : terms_.size();
        if (at_ >= end_) throw NothingInRange{};
        ii2_seg_info info;
        ii2_seg_get_info(seg.h, &info);
        off_.resize(terms_.size() + 1);
        vals_.resize(info.n_postings);
        ck(ctx, ii2_seg_decode(ctx, seg.h, off_.data(), vals_.empty() ? nullptr : vals_.data(), II2_HOST), "reader: values file: decompress");
    }
    // false = go_iterators.EmptyIterator
    bool Next(TermValues *tv) {
        if (closed_ || at_ >= end_) return false;
        tv->term = terms_[at_];
        tv->values.assign(vals_.begin() + off_[at_], vals_.begin() + off_[at_ + 1]);
        at_++;
        return true;
    }
    void Close() { closed_ = true; }

   private:
    std::vector<Term> terms_;
    std::vector<uint64_t> off_;
    std::vector<uint32_t> vals_;
    size_t at_ = 0, end_ = 0;
    bool closed_ = false;
};

class Shard {
   public:
    // basedir empty: segments live in HBM only (the replayed reference scripts); else shard.go:300-358 — load every
    // segment file pair and removed.list found there, and keep the directory in step with every later operation
    explicit Shard(ii2_ctx *ctx, std::string basedir = "") : ctx_(ctx), basedir_(std::move(basedir)) {
        if (basedir_.empty()) return;
        std::error_code ec;
        if (!file::fs::is_directory(basedir_, ec)) throw Error("load inverted index shard: " + basedir_ + " is not a directory");
        std::vector<std::string> keys;
        for (auto &e : file::fs::directory_iterator(basedir_)) {
            if (e.is_directory()) continue;
            const std::string name = e.path().filename().string();
            if (name.size() <= 4 || name.compare(name.size() - 4, 4, "_tdx") != 0) continue;      // (*_tmp files are not segments)
            keys.push_back(name.substr(0, name.size() - 4));
        }
        std::sort(keys.begin(), keys.end());
        for (auto &key : keys) {
            char *endp = nullptr;
            errno = 0;
            const long long k = std::strtoll(key.c_str(), &endp, 10);
            if (errno || !endp || *endp || key.empty()) throw Error("load inverted index: key to int conversion: " + key);
            LoadedSegment ls = load_segment(ctx_, basedir_, key);
            add(Segment{(int64_t)k, std::move(ls.terms), std::make_shared<SegHandle>(ls.seg)});
        }
        try { file::read_removed(basedir_, &removed_); }
        catch (const std::exception &e) { throw Error(std::string("rem list: ") + e.what()); }
    }
    const std::string &basedir() const { return basedir_; }
    void Close() {}                // shard.go:247-249

    // shard.go:33-67 — one direct segment, every term -> [val]
    void Put(std::vector<Term> terms, uint32_t val) {
        std::sort(terms.begin(), terms.end(), term_less);
        terms.erase(std::unique(terms.begin(), terms.end()), terms.end());
        std::vector<uint64_t> off(terms.size() + 1);
        for (size_t i = 0; i <= terms.size(); i++) off[i] = i;
        std::vector<uint32_t> vals(terms.size(), val);
        ii2_seg *s = nullptr;
        ck(ctx_, ii2_seg_encode(ctx_, terms.size(), off.data(), vals.data(), II2_HOST, &s), "s: put");
        Segment seg{now_ns(), std::move(terms), std::make_shared<SegHandle>(s)};
        if (!basedir_.empty()) {   // file.NewDirectWriter: term file only, the value rides in it (file/writer.go:95-120)
            file::TermFile tf;
            tf.terms = seg.terms;
            tf.direct = true;
            tf.direct_vals = vals;
            const std::string key = std::to_string(seg.key);
            try { file::write_terms(basedir_, key, tf); file::commit(file::tdx_path(basedir_, key)); }
            catch (const std::exception &e) { throw Error(std::string("index put: ") + e.what()); }
        }
        std::lock_guard<std::mutex> g(mu_);
        add(std::move(seg));       // make the new segment visible (shard.go:64)
    }

    // additive: many Puts at once.  What N calls of Put (shard.go:33-67) and the merges that fold their N direct segments
    // (shard.go:163-212) leave behind, made directly: the dictionary is the sorted, duplicate-free terms of all docs, every
    // (doc, term) is one (index of the term, val) pair, and ONE ii2_seg_build call sorts and encodes them into one ordinary
    // (non-direct) segment.  No tombstone filter, as in Put.  No docs or no terms: no segment.
    void PutBatch(const std::vector<std::pair<std::vector<Term>, uint32_t>> &docs) {
        if (build_on_device(docs)) { put_batch_device(docs); return; }
        std::vector<Term> terms;
        for (auto &d : docs) terms.insert(terms.end(), d.first.begin(), d.first.end());
        std::sort(terms.begin(), terms.end(), term_less);
        terms.erase(std::unique(terms.begin(), terms.end()), terms.end());
        if (terms.empty()) return;
        std::vector<uint32_t> list_id, vals;
        for (auto &d : docs)
            for (auto &t : d.first) {
                list_id.push_back((uint32_t)(std::lower_bound(terms.begin(), terms.end(), t, term_less) - terms.begin()));
                vals.push_back(d.second);
            }
        ii2_seg *s = nullptr;
        ck(ctx_, ii2_seg_build(ctx_, terms.size(), list_id.size(), list_id.data(), vals.data(), II2_HOST, &s, nullptr), "s: put batch");
        Segment seg{now_ns(), std::move(terms), std::make_shared<SegHandle>(s)};
        if (!basedir_.empty()) {   // written like a merged segment: term file + value file
            try { write_segment(ctx_, seg); }
            catch (const std::exception &e) { throw Error(std::string("index put batch: ") + e.what()); }
        }
        std::lock_guard<std::mutex> g(mu_);
        add(std::move(seg));
    }

    // additive: where PutBatch sorts, deduplicates and looks up its terms - 0: on the host (std::sort, std::unique and one
    // bisection per occurrence), 1: on the device (ii2_dict_build; the occurrences' indices never leave it), -1 (the default):
    // the device from BUILD_MIN_TERMS term occurrences per batch - the smallest probed size from which the device route's
    // [min - max] lies wholly below the host route's (scripts/dict_build_probe.py case r).  A batch with a term
    // above II2_DICT_BUILD_MAX_TERM takes the host route under every mode.  The segment, its files and every later answer are
    // the same on both routes.
    static constexpr uint64_t BUILD_MIN_TERMS = 8192;
    void SetBuild(int mode) {
        if (mode < -1 || mode > 1) throw Error("set build: mode is -1, 0 or 1");
        build_mode_.store(mode);
    }

    // shard.go:72-75 + makeIterator :253-278 — merged view of all segments, [min,max] inclusive, no tombstones
    // The snapshot of shared pointers plays the part of the reference's per-segment read locks (segments.go:32-46):
    // a merge may detach and unlink these segments meanwhile, their device arrays live until the last reader lets go.
    std::vector<TermValues> Read(const Term *min, const Term *max) const {
        const std::vector<std::shared_ptr<Segment>> snap = snapshot();
        std::vector<const Segment *> segs;
        for (auto &s : snap) segs.push_back(s.get());
        return merged(segs, min, max, nullptr);
    }

    // additive: substring, suffix and wildcard search over this shard's segments (InvertedIndex::MatchSearch / MatchTerms say what
    // they return); no tombstone filter, as in Read
    std::map<Term, std::vector<uint32_t>> MatchSearch(const std::vector<Term> &patterns, uint32_t kind) const {
        const std::vector<std::shared_ptr<Segment>> segs = snapshot();
        return match_search(ctx_, segs, patterns, kind, [&](uint64_t bound, auto call) {
            return two_call_dev(ctx_, FIRST_CAP_IDS, nullptr, bound, 1, "match search", call);
        });
    }
    std::vector<Term> MatchTerms(const Term &pattern, uint32_t kind, uint64_t limit) const { return match_terms(ctx_, snapshot(), pattern, kind, limit); }
    // additive: typo-tolerant search over this shard's segments (InvertedIndex::FuzzySearch / FuzzyTerms say what they return); no
    // tombstone filter, as in Read
    std::map<Term, std::vector<uint32_t>> FuzzySearch(const std::vector<Term> &terms, uint32_t max_dist, uint32_t prefix, uint32_t flags) const {
        const std::vector<std::shared_ptr<Segment>> segs = snapshot();
        return fuzzy_search(ctx_, segs, terms, max_dist, prefix, flags, [&](uint64_t bound, auto call) {
            return two_call_dev(ctx_, FIRST_CAP_IDS, nullptr, bound, 1, "fuzzy search", call);
        });
    }
    std::vector<std::pair<Term, uint32_t>> FuzzyTerms(const Term &pattern, uint32_t max_dist, uint32_t prefix, uint32_t flags, uint64_t limit) const {
        return fuzzy_terms(ctx_, snapshot(), pattern, max_dist, prefix, flags, limit);
    }
    // additive: regular-expression search over this shard's segments (InvertedIndex::RegexSearch / RegexTerms say what they return);
    // no tombstone filter, as in Read
    std::map<Term, std::vector<uint32_t>> RegexSearch(const std::vector<Term> &patterns, uint32_t flags) const {
        const std::vector<std::shared_ptr<Segment>> segs = snapshot();
        return regex_search(ctx_, segs, patterns, flags, [&](uint64_t bound, auto call) {
            return two_call_dev(ctx_, FIRST_CAP_IDS, nullptr, bound, 1, "regex search", call);
        });
    }
    std::vector<Term> RegexTerms(const Term &pattern, uint32_t flags, uint64_t limit) const { return regex_terms(ctx_, snapshot(), pattern, flags, limit); }

    // shard.go:78-105
    void Remove(const std::vector<uint32_t> &values) {
        if (values.empty()) return;
        std::lock_guard<std::mutex> g(mu_);
        std::vector<int64_t> ts{now_ns()};
        for (auto &s : segments_) ts.push_back(s->key);
        removed_sync(ts);
        removed_[now_ns()] = values;
        WriteRemovedList();
    }

    // shard.go:107-120 (called with mu_ held)
    void WriteRemovedList() const {
        if (basedir_.empty()) return;
        try { file::write_removed(basedir_, removed_); }
        catch (const std::exception &e) { throw Error(std::string("write rem list: ") + e.what()); }
    }

    // removed_list.go:44-54
    std::vector<uint32_t> RemovedValues() const {
        std::lock_guard<std::mutex> g(mu_);
        std::vector<uint32_t> r;
        for (auto &kv : removed_) r.insert(r.end(), kv.second.begin(), kv.second.end());
        std::sort(r.begin(), r.end());
        return r;
    }

    // shard.go:127-245.  `worker`: the context (= HIP stream) of the calling worker thread; segments are shared
    // between contexts of one device, so InvertedIndex.Merge's workers each bring their own (inverted_index.go:83-103)
    int Merge(int reqCount, int mCount, ii2_ctx *worker = nullptr) {
        ii2_ctx *ctx = worker ? worker : ctx_;
        std::vector<std::shared_ptr<Segment>> picked;
        {   // pick under the list lock; the `merging` flag keeps concurrent merges off the same segments (shard.go:134-146)
            std::lock_guard<std::mutex> g(mu_);
            if ((int)segments_.size() < reqCount) return 0;
            for (auto &s : segments_) {
                if ((int)picked.size() == mCount) break;
                if (!s->merging) { s->merging = true; picked.push_back(s); }
            }
        }
        if (picked.size() < 2) return 0;           // NB: a lone picked flag stays set (shard.go:149-151)
        std::vector<const Segment *> segs;
        for (auto &s : picked) segs.push_back(s.get());
        const std::vector<uint32_t> removed = RemovedValues();
        Segment out;
        const bool any = merged_segment(ctx, segs, removed, &out);
        if (any && !basedir_.empty()) {            // file.NewWriter + Close: both files, renamed when complete
            try { write_segment(ctx, out); }
            catch (const std::exception &e) { throw Error(std::string("s: merge: writer close: ") + e.what()); }
        }
        {
            std::lock_guard<std::mutex> g(mu_);
            if (any) add(std::move(out));          // lazy writer: nothing survives -> no segment (shard.go:219-225)
            segments_.erase(std::remove_if(segments_.begin(), segments_.end(),
                                           [&](const std::shared_ptr<Segment> &s) {
                                               return std::find(picked.begin(), picked.end(), s) != picked.end();
                                           }),
                            segments_.end());      // Segments.detach: invisible for new reads (shard.go:228-230)
        }
        if (!basedir_.empty()) {                   // file.RemoveSegment for every merged segment; the last error is reported (shard.go:232-242)
            std::string err;
            for (auto &sg : picked) {
                try { file::remove_segment(basedir_, std::to_string(sg->key)); }
                catch (const std::exception &e) { err = e.what(); }
            }
            if (!err.empty()) throw Error(err);
        }
        return (int)picked.size();
    }

    // shard.go:280-298
    bool MinMax(Term *mn, Term *mx) const {
        std::lock_guard<std::mutex> g(mu_);
        bool any = false;
        for (auto &s : segments_) {
            if (s->terms.empty()) continue;
            if (!any || term_less(s->terms.front(), *mn)) *mn = s->terms.front();
            if (!any || term_less(*mx, s->terms.back())) *mx = s->terms.back();
            any = true;
        }
        return any;
    }

    size_t SegmentCount() const { std::lock_guard<std::mutex> g(mu_); return segments_.size(); }
    // the segments as they are now (a reader's hold on them, as Read takes it)
    std::vector<std::shared_ptr<Segment>> snapshot() const { std::lock_guard<std::mutex> g(mu_); return segments_; }

   private:

    // file.NewWriter + Close for a device-resident segment: both files, under their final names only when complete
    bool build_on_device(const std::vector<std::pair<std::vector<Term>, uint32_t>> &docs) const {
        const int mode = build_mode_.load();
        if (mode == 0) return false;
        uint64_t n = 0;
        for (auto &d : docs)
            for (auto &t : d.first) {
                if (t.size() > II2_DICT_BUILD_MAX_TERM) return false;
                n++;
            }
        return n > 0 && (mode == 1 || n >= BUILD_MIN_TERMS);
    }
    // PutBatch's device route: every term occurrence flat -> ii2_dict_build (the arrays staged in device buffers, so that the
    // occurrences' indices stay there) -> ii2_seg_build on those indices -> ii2_dict_export for Segment::terms and the term
    // file.  The built dictionary becomes the segment's resident one: its first device lookup uploads nothing.
    void put_batch_device(const std::vector<std::pair<std::vector<Term>, uint32_t>> &docs) {
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> off{0};
        std::vector<uint32_t> vals;
        for (auto &d : docs)
            for (auto &t : d.first) {
                bytes.insert(bytes.end(), t.begin(), t.end());
                off.push_back(bytes.size());
                vals.push_back(d.second);
            }
        const uint64_t n = vals.size();
        DevMem d_bytes(ctx_), d_off(ctx_), d_ids(ctx_), d_vals(ctx_);
        ck(ctx_, ii2_dev_alloc(ctx_, bytes.size() + 16, &d_bytes.p), "s: put batch");
        ck(ctx_, ii2_dev_alloc(ctx_, off.size() * sizeof(uint64_t), &d_off.p), "s: put batch");
        ck(ctx_, ii2_dev_alloc(ctx_, n * sizeof(uint32_t), &d_ids.p), "s: put batch");
        ck(ctx_, ii2_dev_alloc(ctx_, n * sizeof(uint32_t), &d_vals.p), "s: put batch");
        if (!bytes.empty()) ck(ctx_, ii2_copy_h2d(ctx_, d_bytes.p, bytes.data(), bytes.size()), "s: put batch");
        ck(ctx_, ii2_copy_h2d(ctx_, d_off.p, off.data(), off.size() * sizeof(uint64_t)), "s: put batch");
        ck(ctx_, ii2_copy_h2d(ctx_, d_vals.p, vals.data(), n * sizeof(uint32_t)), "s: put batch");
        auto dict = std::make_unique<DictHandle>();
        ck(ctx_, ii2_dict_build(ctx_, n, (const uint8_t *)d_bytes.p, (const uint64_t *)d_off.p, II2_DEVICE, &dict->h, (uint32_t *)d_ids.p, nullptr), "s: put batch: dictionary");
        uint64_t n_unique = 0, n_bytes = 0;
        ii2_dict_info(dict->h, &n_unique, &n_bytes);
        ii2_seg *s = nullptr;
        ck(ctx_, ii2_seg_build(ctx_, n_unique, n, (const uint32_t *)d_ids.p, (const uint32_t *)d_vals.p, II2_DEVICE, &s, nullptr), "s: put batch");
        auto handle = std::make_shared<SegHandle>(s);
        std::vector<uint8_t> tb(n_bytes + 1);
        std::vector<uint64_t> to(n_unique + 1);
        ck(ctx_, ii2_dict_export(ctx_, dict->h, tb.data(), to.data()), "s: put batch: dictionary");
        std::vector<Term> terms(n_unique);
        for (uint64_t i = 0; i < n_unique; i++) terms[i].assign((const char *)tb.data() + to[i], to[i + 1] - to[i]);
        Segment seg{now_ns(), std::move(terms), std::move(handle)};
        seg.dict = std::move(dict);
        if (!basedir_.empty()) {   // written like a merged segment: term file + value file
            try { write_segment(ctx_, seg); }
            catch (const std::exception &e) { throw Error(std::string("index put batch: ") + e.what()); }
        }
        std::lock_guard<std::mutex> g(mu_);
        add(std::move(seg));
    }
    void write_segment(ii2_ctx *ctx, const Segment &s) const {
        const std::string key = std::to_string(s.key);
        file::TermFile tf;
        tf.terms = s.terms;
        file::write_terms(basedir_, key, tf);
        file::write_dv1(basedir_, key, Writer::export_dv1(ctx, s.seg->h));
        file::commit(file::dv1_path(basedir_, key));
        file::commit(file::tdx_path(basedir_, key));
    }

    // segments.go:56-64 — insert before the first segment with terms >= new.terms (mu_ held, or the constructor)
    void add(Segment s) {
        auto sp = std::make_shared<Segment>(std::move(s));
        size_t pos = 0;
        while (pos < segments_.size() && segments_[pos]->terms.size() < sp->terms.size()) pos++;
        segments_.insert(segments_.begin() + pos, sp);
    }

    void removed_sync(const std::vector<int64_t> &ts) {   // removed_list.go:57-71
        if (ts.empty()) return;
        const int64_t oldest = *std::min_element(ts.begin(), ts.end());
        for (auto it = removed_.begin(); it != removed_.end();) it = it->first < oldest ? removed_.erase(it) : ++it;
    }

    // Term alignment (host; file.CompareTermValues order): union of the segments' terms inside [min,max]
    // and, per segment, an aligned view with one slot per union term.
    struct Aligned {
        std::vector<Term> terms;
        std::vector<std::shared_ptr<SegHandle>> views;
    };
    Aligned align(ii2_ctx *ctx, const std::vector<const Segment *> &segs, const Term *min, const Term *max) const {
        // every segment's dictionary restricted to [min, max] is a run of consecutive terms (the dictionaries are sorted);
        // the k-way dictionary merge itself runs on the device (ii2_align_terms) and so does the construction of the
        // aligned views (ii2_seg_select_aligned): the host only flattens the byte strings
        Aligned a;
        struct Part { const Segment *seg; size_t j0, j1; };
        std::vector<Part> parts;
        for (auto *s : segs) {
            size_t j0 = 0, j1 = s->terms.size();
            if (min) j0 = std::lower_bound(s->terms.begin(), s->terms.end(), *min, term_less) - s->terms.begin();
            if (max) j1 = std::upper_bound(s->terms.begin(), s->terms.end(), *max, term_less) - s->terms.begin();
            if (j0 >= j1) continue;                // segment has nothing in range: skipped (shard.go:257-261)
            parts.push_back(Part{s, j0, j1});
        }
        if (parts.empty()) return a;
        std::vector<std::shared_ptr<SegHandle>> views;
        // the library aligns at most II2_MAX_LISTS dictionaries per call: more segments are aligned in groups against the
        // union of the previous groups (kept as an extra dictionary)... the host mirror keeps it simple and aligns in one
        // call when it can, else falls back to groups of II2_MAX_LISTS merged pairwise by fold_to_limit's rounds
        const size_t kmax = II2_MAX_LISTS;
        if (parts.size() <= kmax) {
            std::string bytes;
            std::vector<uint64_t> off{0}, first{0};
            for (auto &pt : parts) {
                for (size_t j = pt.j0; j < pt.j1; j++) { bytes += pt.seg->terms[j]; off.push_back(bytes.size()); }
                first.push_back(off.size() - 1);
            }
            ii2_align *al = nullptr;
            ck(ctx, ii2_align_terms(ctx, (uint32_t)parts.size(), (const uint8_t *)bytes.data(), off.data(), first.data(), &al), "index read");
            struct AlignGuard { ii2_align *h; ~AlignGuard() { ii2_align_free(h); } } guard{al};
            uint64_t nu = 0;
            ii2_align_info(al, &nu, nullptr);
            std::vector<uint64_t> rep(nu);
            ck(ctx, ii2_align_export(ctx, al, rep.data(), nullptr), "index read");
            a.terms.reserve(nu);
            for (uint64_t u = 0; u < nu; u++) a.terms.emplace_back(bytes.data() + off[rep[u]], off[rep[u] + 1] - off[rep[u]]);
            std::vector<const ii2_seg *> srcs;
            std::vector<uint64_t> fl;
            for (auto &pt : parts) { srcs.push_back(pt.seg->seg->h); fl.push_back(pt.j0); }
            std::vector<ii2_seg *> vs(parts.size(), nullptr);
            ck(ctx, ii2_seg_select_aligned_all(ctx, srcs.data(), al, fl.data(), vs.data()), "index read");     // (one wait for all the views)
            for (ii2_seg *v : vs) a.views.push_back(std::make_shared<SegHandle>(v));
            return a;
        }
        // more than II2_MAX_LISTS segments: union dictionary on the host, views through ii2_seg_select
        for (auto &pt : parts) a.terms.insert(a.terms.end(), pt.seg->terms.begin() + pt.j0, pt.seg->terms.begin() + pt.j1);
        std::sort(a.terms.begin(), a.terms.end(), term_less);
        a.terms.erase(std::unique(a.terms.begin(), a.terms.end()), a.terms.end());
        for (auto &pt : parts) {
            std::vector<int64_t> src(a.terms.size(), -1);
            size_t j = pt.j0;
            for (size_t i = 0; i < a.terms.size(); i++) {
                while (j < pt.j1 && term_less(pt.seg->terms[j], a.terms[i])) j++;
                if (j < pt.j1 && pt.seg->terms[j] == a.terms[i]) src[i] = (int64_t)j;
            }
            ii2_seg *v = nullptr;
            ck(ctx, ii2_seg_select(ctx, pt.seg->seg->h, a.terms.size(), src.data(), &v), "index read");
            a.views.push_back(std::make_shared<SegHandle>(v));
        }
        return a;
    }

    // The library merges at most II2_MAX_LISTS segments per call; the reference has no such bound (mCount is the
    // caller's), so more are folded in rounds: the union is associative, and the tombstone filter and the empty-term
    // drop only have to happen in the last round.
    void fold_to_limit(ii2_ctx *ctx, std::vector<std::shared_ptr<SegHandle>> &views) const {
        while (views.size() > II2_MAX_LISTS) {
            std::vector<const ii2_seg *> hs;
            for (size_t i = 0; i < II2_MAX_LISTS; i++) hs.push_back(views[i]->h);
            ii2_seg *m = nullptr;
            ii2_merge_stats st;
            std::memset(&st, 0, sizeof st);
            ck(ctx, ii2_merge_segments_to_seg(ctx, II2_MAX_LISTS, hs.data(), nullptr, &m, &st), "s: merge");
            views.erase(views.begin(), views.begin() + II2_MAX_LISTS);
            if (m) views.insert(views.begin(), std::make_shared<SegHandle>(m));
        }
    }

    // The small read in one launch (ii2_read_small): a few small segments, the slice of each one's terms that lies in
    // [min, max].  false: over the limits, take the general path.
    bool read_small(const std::vector<const Segment *> &segs, const Term *min, const Term *max, std::vector<TermValues> *out) const {
        if (segs.empty() || segs.size() > II2_MAX_LISTS) return false;
        std::string bytes;
        std::vector<uint64_t> off{0}, first{0}, lfirst;
        std::vector<const ii2_seg *> hs;
        uint64_t n_post = 0;
        for (auto *sg : segs) {
            size_t j0 = 0, j1 = sg->terms.size();
            if (min) j0 = std::lower_bound(sg->terms.begin(), sg->terms.end(), *min, term_less) - sg->terms.begin();
            if (max) j1 = std::upper_bound(sg->terms.begin(), sg->terms.end(), *max, term_less) - sg->terms.begin();
            if (j0 >= j1) continue;                // segment has nothing in range: skipped (shard.go:257-261)
            ii2_seg_info info;
            ii2_seg_get_info(sg->seg->h, &info);
            n_post += info.n_postings;
            if (off.size() - 1 + (j1 - j0) > II2_SMALL_MERGE_TERMS || n_post > II2_SMALL_MERGE_POSTINGS) return false;
            for (size_t j = j0; j < j1; j++) { bytes += sg->terms[j]; off.push_back(bytes.size()); }
            if (bytes.size() > 16384) return false;
            first.push_back(off.size() - 1);
            lfirst.push_back(j0);
            hs.push_back(sg->seg->h);
        }
        if (hs.empty()) return true;                // nothing in range: an empty read
        const uint64_t n = off.size() - 1;
        std::vector<uint64_t> rep(n), po(n + 1);
        std::vector<uint32_t> vals(n_post + 1);
        uint64_t nu = 0;
        const int rc = ii2_read_small(ctx_, (uint32_t)hs.size(), hs.data(), (const uint8_t *)bytes.data(), off.data(), first.data(), lfirst.data(),
                                      rep.data(), po.data(), vals.data(), n_post, &nu);
        if (rc == II2_ERANGE) return false;
        ck(ctx_, rc, "index read");
        out->reserve(nu);
        for (uint64_t u = 0; u < nu; u++)
            out->push_back(TermValues{Term(bytes.data() + off[rep[u]], off[rep[u] + 1] - off[rep[u]]),
                                      std::vector<uint32_t>(vals.begin() + po[u], vals.begin() + po[u + 1])});
        return true;
    }

    std::vector<TermValues> merged(const std::vector<const Segment *> &segs, const Term *min, const Term *max,
                                   const std::vector<uint32_t> *removed) const {
        std::vector<TermValues> out;
        if (!removed && read_small(segs, min, max, &out)) return out;
        Aligned a = align(ctx_, segs, min, max);
        if (a.views.empty()) return out;
        fold_to_limit(ctx_, a.views);
        TombHandle tomb;
        if (removed && !removed->empty()) ck(ctx_, ii2_tomb_create(ctx_, removed->data(), removed->size(), II2_HOST, &tomb.h), "s: merge");
        std::vector<const ii2_seg *> hs;
        uint64_t cap = 0;
        for (auto &v : a.views) {
            hs.push_back(v->h);
            ii2_seg_info info;
            ii2_seg_get_info(v->h, &info);
            cap += info.n_postings;
        }
        const uint64_t T = a.terms.size();
        DevMem d_off(ctx_), d_vals(ctx_);
        ck(ctx_, ii2_dev_alloc(ctx_, (T + 1) * 8, &d_off.p), "s: merge");
        ck(ctx_, ii2_dev_alloc(ctx_, (cap + 1) * 4, &d_vals.p), "s: merge");
        ii2_merge_stats st;
        std::memset(&st, 0, sizeof st);
        ck(ctx_, ii2_merge_segments(ctx_, (uint32_t)hs.size(), hs.data(), tomb.h, (uint64_t *)d_off.p, (uint32_t *)d_vals.p, cap + 1, &st), "s: merge");
        std::vector<uint64_t> off(T + 1);
        std::vector<uint32_t> vals(st.n_out);
        ck(ctx_, ii2_copy_d2h(ctx_, off.data(), d_off.p, (T + 1) * 8), "s: merge");
        if (st.n_out) ck(ctx_, ii2_copy_d2h(ctx_, vals.data(), d_vals.p, st.n_out * 4), "s: merge");
        for (uint64_t t = 0; t < T; t++) {
            TermValues tv{a.terms[t], std::vector<uint32_t>(vals.begin() + off[t], vals.begin() + off[t + 1])};
            if (removed && tv.values.empty()) continue;      // merge drops emptied terms (shard.go:192-194)
            out.push_back(std::move(tv));
        }
        return out;
    }

    // Merge into a new device-resident segment; false when no term survives.
    bool merged_segment(ii2_ctx *ctx, const std::vector<const Segment *> &segs, const std::vector<uint32_t> &removed, Segment *out) const {
        // The common case — a few small segments (every Put writes a direct segment of one posting per term, shard.go:33-67,
        // and the smallest segments are picked first, shard.go:135-146) — is one launch: alignment, union, removed-list
        // filter, empty-term drop and encode in ii2_merge_small.  Anything larger takes the general path below.
        {
            size_t n_terms = 0, n_bytes = 0;
            uint64_t n_post = 0;
            for (auto *sg : segs) {
                n_terms += sg->terms.size();
                for (auto &t : sg->terms) n_bytes += t.size();
                ii2_seg_info inf;
                if (ii2_seg_get_info(sg->seg->h, &inf) == II2_OK) n_post += inf.n_postings;
            }
            if (!segs.empty() && segs.size() <= II2_MAX_LISTS && n_terms <= II2_SMALL_MERGE_TERMS && n_post <= II2_SMALL_MERGE_POSTINGS &&
                removed.size() <= II2_SMALL_MERGE_REMOVED && n_bytes <= 16384) {
                std::string bytes;
                std::vector<uint64_t> off{0}, first{0};
                std::vector<const ii2_seg *> hs;
                for (auto *sg : segs) {
                    for (auto &t : sg->terms) { bytes += t; off.push_back(bytes.size()); }
                    first.push_back(off.size() - 1);
                    hs.push_back(sg->seg->h);
                }
                std::vector<uint64_t> kept(n_terms + 1);
                uint64_t n_kept = 0;
                ii2_seg *m = nullptr;
                ii2_merge_stats st;
                std::memset(&st, 0, sizeof st);
                const int rc = ii2_merge_small(ctx, (uint32_t)hs.size(), hs.data(), (const uint8_t *)bytes.data(), off.data(), first.data(),
                                               removed.empty() ? nullptr : removed.data(), removed.size(), &m, kept.data(), &n_kept, &st);
                if (rc == II2_OK) {
                    if (!m) return false;
                    out->terms.clear();
                    for (uint64_t j = 0; j < n_kept; j++) out->terms.emplace_back(bytes.data() + off[kept[j]], off[kept[j] + 1] - off[kept[j]]);
                    out->seg = std::make_shared<SegHandle>(m);
                    out->key = now_ns();
                    return true;
                }
                if (rc != II2_ERANGE) ck(ctx, rc, "s: merge");      // (a view's posting count is an upper bound: the kernel may still refuse)
            }
        }
        Aligned a = align(ctx, segs, nullptr, nullptr);
        if (a.views.empty()) return false;
        fold_to_limit(ctx, a.views);
        TombHandle tomb;
        if (!removed.empty()) ck(ctx, ii2_tomb_create(ctx, removed.data(), removed.size(), II2_HOST, &tomb.h), "s: merge");
        std::vector<const ii2_seg *> hs;
        for (auto &v : a.views) hs.push_back(v->h);
        ii2_seg *m = nullptr;
        ii2_merge_stats st;
        std::memset(&st, 0, sizeof st);
        ck(ctx, ii2_merge_segments_to_seg(ctx, (uint32_t)hs.size(), hs.data(), tomb.h, &m, &st), "s: merge");
        if (!m) return false;
        SegHandle full(m);
        // drop the terms that lost every posting: compacted view over the merged segment
        const uint64_t T = a.terms.size();
        std::vector<uint64_t> off(T + 1);
        ck(ctx, ii2_seg_decode(ctx, m, off.data(), nullptr, II2_HOST), "s: merge");
        std::vector<int64_t> src;
        for (uint64_t t = 0; t < T; t++)
            if (off[t + 1] > off[t]) { src.push_back((int64_t)t); out->terms.push_back(a.terms[t]); }
        ii2_seg *c = nullptr;
        ck(ctx, ii2_seg_select(ctx, m, src.size(), src.data(), &c), "s: merge");
        out->seg = std::make_shared<SegHandle>(c);
        out->key = now_ns();
        return true;
    }

    ii2_ctx *ctx_;
    std::atomic<int> build_mode_{-1};                      // SetBuild
    std::string basedir_;                                  // empty: no files
    mutable std::mutex mu_;                                // Segments.m and RemovedLists.m in one: guards the two members below
    std::vector<std::shared_ptr<Segment>> segments_;       // sorted by term count
    std::map<int64_t, std::vector<uint32_t>> removed_;     // RemovedLists.lists
};

// shard.go:362-378
static uint32_t shard_key(const Term &t) {
    uint8_t a = 0, b = 0;
    if (t.size() >= 2) { a = (uint8_t)t[0]; b = (uint8_t)t[1]; }
    return (uint32_t)((uint16_t)((uint16_t)(a << 8) + b) >> 6);
}

class InvertedIndex {
   public:
    // inverted_index.go:342-403: every sub-directory of basedir is a shard named by its key ("%04d")
    explicit InvertedIndex(ii2_ctx *ctx, std::string basedir = "") : ctx_(ctx), basedir_(std::move(basedir)) {
        if (basedir_.empty()) return;
        std::error_code ec;
        if (!file::fs::is_directory(basedir_, ec)) throw Error("shards read: " + basedir_ + " is not a directory");
        for (auto &e : file::fs::directory_iterator(basedir_)) {
            if (!e.is_directory()) continue;
            const std::string name = e.path().filename().string();
            char *endp = nullptr;
            const unsigned long k = std::strtoul(name.c_str(), &endp, 10);
            if (name.empty() || !endp || *endp || k >= 1024) continue;          // not a shard directory
            try { shards_.emplace((uint32_t)k, std::make_unique<Shard>(ctx_, e.path().string())); }
            catch (const std::exception &ex) { throw Error(std::string("shard init: ") + ex.what()); }
        }
    }

    void Put(const std::vector<Term> &terms, uint32_t val) {                  // inverted_index.go:113-145
        std::map<uint32_t, std::vector<Term>> groups;
        for (auto &t : terms) groups[shard_key(t)].push_back(t);
        for (auto &g : groups) shard(g.first).Put(g.second, val);
    }
    // additive: every doc's terms grouped by shard as Put groups them, one Shard.PutBatch per shard that receives something
    void PutBatch(const std::vector<std::pair<std::vector<Term>, uint32_t>> &docs) {
        std::map<uint32_t, std::vector<std::pair<std::vector<Term>, uint32_t>>> groups;
        for (auto &d : docs) {
            std::map<uint32_t, std::vector<Term>> mine;
            for (auto &t : d.first) mine[shard_key(t)].push_back(t);
            for (auto &m : mine) groups[m.first].emplace_back(std::move(m.second), d.second);
        }
        for (auto &g : groups) shard(g.first).PutBatch(g.second);
    }
    void PutRemoved(const std::vector<uint32_t> &values) {                    // inverted_index.go:41-55
        for (auto &s : shard_list()) s.second->Remove(values);
    }
    // inverted_index.go:62-109: `concurrency` workers pull shards off one queue; every worker owns a context (a HIP
    // stream with its scratch) on the index's device, the segments are shared.  A worker that fails records the
    // error and stops pulling, the others drain the queue (the reference's goroutines do the same); concurrency <= 0
    // starts no worker and merges nothing.
    int64_t Merge(int reqCount, int mCount, int concurrency) {
        std::vector<Shard *> shards;
        for (auto &s : shard_list()) shards.push_back(s.second);
        if (concurrency <= 0 || shards.empty()) return 0;
        const size_t nw = std::min<size_t>((size_t)concurrency, shards.size());
        std::vector<ii2_ctx *> workers;                          // worker 0 uses the index's own context
        {
            std::lock_guard<std::mutex> g(mu_);
            while (workers_.size() + 1 < nw) {
                ii2_ctx *c = nullptr;
                if (ii2_ctx_create(ii2_ctx_device(ctx_), 0, &c)) throw Error(std::string("merge: worker context: ") + ii2_last_error(nullptr));
                workers_.push_back(c);
            }
            workers.assign(workers_.begin(), workers_.begin() + (nw - 1));
        }
        std::atomic<size_t> next{0};
        std::atomic<int64_t> merged{0};
        std::mutex err_mu;
        std::string err;
        auto work = [&](ii2_ctx *c) {
            for (;;) {
                const size_t i = next.fetch_add(1);
                if (i >= shards.size()) return;
                try { merged += shards[i]->Merge(reqCount, mCount, c); }
                catch (const std::exception &e) { std::lock_guard<std::mutex> g(err_mu); err = e.what(); return; }
            }
        };
        std::vector<std::thread> pool;
        for (size_t w = 1; w < nw; w++) pool.emplace_back(work, workers[w - 1]);
        work(ctx_);
        for (auto &t : pool) t.join();
        if (!err.empty()) throw Error(err);
        return merged.load();
    }
    ~InvertedIndex() { for (ii2_ctx *c : workers_) ii2_ctx_destroy(c); }
    std::vector<TermValues> Read(const Term *min, const Term *max) const {    // inverted_index.go:300-340
        std::vector<TermValues> out;
        for (auto &s : shard_list()) {                                        // ascending shard key
            Term mn, mx;
            if (!s.second->MinMax(&mn, &mx)) continue;
            if (min && term_less(mx, *min)) continue;
            if (max && term_less(*max, mn)) continue;
            auto part = s.second->Read(min, max);
            out.insert(out.end(), std::make_move_iterator(part.begin()), std::make_move_iterator(part.end()));
        }
        return out;
    }
    // The reference reads each selected shard from its smallest prefix on (the merged terms of all its segments), keeps the
    // terms that start with a prefix, stops at the first term past the greatest prefix, then sorts and compacts the collected
    // lists.  Here no list leaves the device: in every segment the lists of a prefix are one run of consecutive terms
    // (prefix_runs), and ONE ii2_query_batch call - an OR query per prefix - unions the runs of every segment of every shard.
    std::map<Term, std::vector<uint32_t>> PrefixSearch(std::vector<Term> prefixes) const {   // inverted_index.go:192-295
        std::sort(prefixes.begin(), prefixes.end(), term_less);
        prefixes.erase(std::unique(prefixes.begin(), prefixes.end()), prefixes.end());
        struct Ranges {
            std::vector<const ii2_seg *> segs;
            std::vector<uint64_t> first, end;
        };
        std::map<Term, Ranges> found;
        std::vector<std::shared_ptr<Segment>> held;          // the segments read, alive until the unions are done
        prefix_runs(prefixes, [&](const Term &p, const std::shared_ptr<Segment> &sg, size_t j0, size_t j1) {
            Ranges &r = found[p];
            r.segs.push_back(sg->seg->h);
            r.first.push_back(j0);
            r.end.push_back(j1);
            held.push_back(sg);
        });
        std::map<Term, std::vector<uint32_t>> out;
        // ONE ii2_query_batch call, one wait and one download for all the prefixes (an OR query each), through two_call.  The
        // output's size: the C ABI gives no per-list counts, so a prefix is bounded by the postings of the segments its runs lie
        // in.  Prefixes whose bounds add up to the call's limit of 2^32 ids go in several calls; one that reaches it alone goes
        // through ii2_union_ranges.
        constexpr uint64_t CALL_IDS = 0xFFFFFFFFull;
        auto it = found.begin();
        while (it != found.end()) {
            std::vector<const Term *> names;
            std::vector<uint8_t> op;
            std::vector<uint64_t> query_first{0}, first, end;
            std::vector<const ii2_seg *> segs;
            uint64_t bound = 0;
            for (; it != found.end(); ++it) {
                const Ranges &r = it->second;
                const uint64_t b = union_bound(r.segs, seg_postings);
                if (!names.empty() && bound + b >= CALL_IDS) break;
                bound += b;
                names.push_back(&it->first);
                op.push_back(II2_OP_OR);
                segs.insert(segs.end(), r.segs.begin(), r.segs.end());
                first.insert(first.end(), r.first.begin(), r.first.end());
                end.insert(end.end(), r.end.begin(), r.end.end());
                query_first.push_back(segs.size());
            }
            if (bound >= CALL_IDS) {                                          // (one prefix, alone in its call)
                DevMem d_out(ctx_);
                uint64_t n = 0;
                ck(ctx_, ii2_dev_alloc(ctx_, (bound + 1) * sizeof(uint32_t), &d_out.p), "prefix search");
                ck(ctx_, ii2_union_ranges(ctx_, segs.size(), segs.data(), first.data(), end.data(), nullptr, (uint32_t *)d_out.p, bound + 1, &n),
                   "prefix search");
                out[*names[0]] = download(d_out, n, "prefix search");
                continue;
            }
            std::vector<uint64_t> off(names.size() + 1, 0);
            const Output o = two_call(bound, 1, "prefix search", [&](uint32_t *d_ids, uint64_t cap, uint64_t *n) {
                const int rc = ii2_query_batch(ctx_, names.size(), op.data(), query_first.data(), segs.data(), first.data(), end.data(), nullptr, d_ids,
                                               cap, off.data());
                *n = off.back();
                return rc;
            });
            const std::vector<uint32_t> all = download(o.mem, o.n, "prefix search");      // :288-292 sort + compact, on the GPU
            for (size_t q = 0; q < names.size(); q++) out[*names[q]] = std::vector<uint32_t>(all.begin() + off[q], all.begin() + off[q + 1]);
        }
        return out;
    }
    // additive: substring, suffix and wildcard search - map<pattern, ids> of every pattern of `kind` (II2_MATCH_CONTAINS / SUFFIX /
    // GLOB, | II2_MATCH_NOCASE, | II2_MATCH_UTF8).  It visits every segment of every shard (a pattern selects no shard): ii2_dict_match over the
    // segments' resident dictionaries (match_runs), then one OR query per pattern over all its runs in ONE ii2_query_batch call,
    // through two_call, as PrefixSearch does.  A pattern that matches no term has no entry.  Like Read, no tombstone filter.
    std::map<Term, std::vector<uint32_t>> MatchSearch(const std::vector<Term> &patterns, uint32_t kind) const {
        const std::vector<std::shared_ptr<Segment>> segs = all_segments();      // alive until the unions are done
        return match_search(ctx_, segs, patterns, kind, [&](uint64_t bound, auto call) { return two_call(bound, 1, "match search", call); });
    }
    // additive: the distinct terms the pattern matches, over every segment of every shard, in bytes.Compare order, at most `limit`
    std::vector<Term> MatchTerms(const Term &pattern, uint32_t kind, uint64_t limit) const { return match_terms(ctx_, all_segments(), pattern, kind, limit); }
    // additive: typo-tolerant search - map<query term, ids under any term within `max_dist` edits of it> (flags: II2_FUZZY_TRANSPOSE,
    // II2_MATCH_NOCASE, II2_MATCH_UTF8 - symbols instead of bytes; `prefix` leading bytes must be equal, Lucene's prefix_length).  It visits every segment of every shard:
    // ii2_dict_fuzzy over the segments' resident dictionaries (fuzzy_runs), then one OR query per query term over all its runs in
    // ONE ii2_query_batch call, through two_call, as MatchSearch does.  A term that matches nothing has no entry.  Like Read, no
    // tombstone filter.
    std::map<Term, std::vector<uint32_t>> FuzzySearch(const std::vector<Term> &terms, uint32_t max_dist, uint32_t prefix, uint32_t flags) const {
        const std::vector<std::shared_ptr<Segment>> segs = all_segments();      // alive until the unions are done
        return fuzzy_search(ctx_, segs, terms, max_dist, prefix, flags, [&](uint64_t bound, auto call) { return two_call(bound, 1, "fuzzy search", call); });
    }
    // additive: the distinct terms within distance of the pattern and their distances, over every segment of every shard, distance
    // ascending, then in bytes.Compare order, at most `limit`
    std::vector<std::pair<Term, uint32_t>> FuzzyTerms(const Term &pattern, uint32_t max_dist, uint32_t prefix, uint32_t flags, uint64_t limit) const {
        return fuzzy_terms(ctx_, all_segments(), pattern, max_dist, prefix, flags, limit);
    }
    // additive: regular-expression search - map<pattern, ids under any term the pattern matches as a whole> (flags: 0 or
    // II2_MATCH_NOCASE; the syntax is include/ii2.h's).  It visits every segment of every shard: ii2_dict_regex over the segments'
    // resident dictionaries (regex_runs, chunks of 8 patterns), then one OR query per pattern over all its runs in ONE
    // ii2_query_batch call, through two_call, as MatchSearch does.  A pattern that matches nothing has no entry; one that does not
    // parse fails the whole call before any search runs.  Like Read, no tombstone filter.
    std::map<Term, std::vector<uint32_t>> RegexSearch(const std::vector<Term> &patterns, uint32_t flags) const {
        const std::vector<std::shared_ptr<Segment>> segs = all_segments();      // alive until the unions are done
        return regex_search(ctx_, segs, patterns, flags, [&](uint64_t bound, auto call) { return two_call(bound, 1, "regex search", call); });
    }
    // additive: the distinct terms the pattern matches, over every segment of every shard, in bytes.Compare order, at most `limit`
    std::vector<Term> RegexTerms(const Term &pattern, uint32_t flags, uint64_t limit) const { return regex_terms(ctx_, all_segments(), pattern, flags, limit); }
    // additive: ids present under every term.  A term's postings are spread over the segments of its shard (every Put writes
    // one): one group per term, one one-list range per segment that holds it (Plan::add), and ONE ii2_intersect_ranges call - no
    // list is merged, downloaded or uploaded again.  The output's size: the smallest term's bound.  Like Read, no tombstone filter.
    std::vector<uint32_t> Intersect(const std::vector<Term> &terms) const {
        Resolver where(*this);
        Plan plan;
        const uint64_t bound = smallest(plan.add(where, terms, {}, Absent::EmptyQuery));
        if (!bound) return {};                               // no term, or a term in no segment: nothing is under every term
        const Output o = two_call(bound, 1, "intersect", [&](uint32_t *d_ids, uint64_t cap, uint64_t *n) {
            return ii2_intersect_ranges(ctx_, plan.n_groups(), plan.group_first.data(), plan.segs.data(), plan.first.data(), plan.end.data(), nullptr,
                                        d_ids, cap, n);
        });
        return download(o.mem, o.n, "intersect");
    }
    // additive: ids present under every term of `terms` and under none of `except` ("error AND db NOT healthcheck").  One group
    // per term as Intersect builds them, the excluded terms' groups flagged, and ONE ii2_andnot_ranges call: no second query, no
    // second download, no set difference on the host.  An excluded term found in no segment is dropped; a required one gives the
    // empty result.  The output's size: the smallest REQUIRED term's bound (an exclusion only removes ids).  Like Intersect and
    // Read, no tombstone filter.
    std::vector<uint32_t> IntersectExcept(const std::vector<Term> &terms, const std::vector<Term> &except) const {
        Resolver where(*this);
        Plan plan;
        const uint64_t bound = smallest(plan.add(where, terms, except, Absent::EmptyQuery));
        if (!bound) return {};
        const Output o = filter_run(plan, bound, "intersect except");
        return download(o.mem, o.n, "intersect except");
    }
    // additive: ids present under AT LEAST min_match of `terms` and under none of `except` (minimum-should-match, "any two of
    // these tags").  One group per term as IntersectExcept builds them - but a required term found in no segment is an empty group,
    // not an empty result - and ONE ii2_atleast_ranges call and one download.  Like Intersect and Read, no tombstone filter.
    std::vector<uint32_t> IntersectAtLeast(const std::vector<Term> &terms, uint32_t min_match, const std::vector<Term> &except) const {
        if (!min_match) throw std::runtime_error("intersect at least: min_match is 0");
        Resolver where(*this);
        Plan plan;
        std::vector<uint64_t> posts = plan.add(where, terms, except, Absent::EmptyGroup);
        if (posts.size() < min_match) return {};
        // the output's size: a result id lies in at least one of any n' - min_match + 1 terms, so those with the smallest bounds
        std::sort(posts.begin(), posts.end());
        uint64_t bound = 0;
        for (size_t k = 0; k + min_match <= posts.size(); k++) bound += posts[k];
        const Output o = filter_run(plan, bound, "intersect at least", min_match);
        return download(o.mem, o.n, "intersect at least");
    }
    // additive: the k ids under the MOST of `terms` - at least min_match of them, under none of `except` - with the number of terms each
    // lies under, ordered by that score descending, then id ascending (a ranked page of a search).  One group per term as
    // IntersectAtLeast builds them (a term found in no segment is an empty group), ONE ii2_topk_ranges call and one download of the k
    // (id, score) pairs.  Like IntersectAtLeast, no tombstone filter.
    std::vector<std::pair<uint32_t, uint32_t>> IntersectTop(const std::vector<Term> &terms, uint64_t k, uint32_t min_match, const std::vector<Term> &except) const {
        if (!min_match) throw std::runtime_error("intersect top: min_match is 0");
        if (k > II2_TOPK_MAX) throw std::runtime_error("intersect top: k above II2_TOPK_MAX");
        Resolver where(*this);
        Plan plan;
        if (plan.add(where, terms, except, Absent::EmptyGroup).size() < min_match || !k) return {};
        return ranked(k, "intersect top", [&](uint32_t *d_ids, uint32_t *d_scores, uint64_t *n) {
            return ii2_topk_ranges(ctx_, plan.n_groups(), plan.group_first.data(), plan.group_not.data(), min_match, k, plan.segs.data(),
                                   plan.first.data(), plan.end.data(), nullptr, d_ids, d_scores, n, nullptr, nullptr);
        });
    }
    // additive: which of `terms` each of `ids` lies under (highlighting, "matched queries": which 3 of 5 terms gave a score of 3).
    // ids in any order - an ascending result or IntersectTop's ranked page.  One group per term as IntersectTop builds them (a term
    // found in no segment is an empty group: its bit is never set), one upload of the ids, ONE ii2_explain_ranges call and one
    // download.  Returns ids.size() rows of ceil(terms.size() / 64) words: bit j & 63 of word i * n_words + (j >> 6) says ids[i]
    // lies under terms[j]; an id given twice has its bits in its first row and zeros after.  Like Intersect, no tombstone filter.
    std::vector<uint64_t> MatchedTerms(const std::vector<uint32_t> &ids, const std::vector<Term> &terms) const {
        if (ids.size() > II2_EXPLAIN_MAX_IDS) throw std::runtime_error("matched terms: more than II2_EXPLAIN_MAX_IDS ids");
        const uint64_t n_words = (terms.size() + 63) / 64, n_out = ids.size() * n_words;
        std::vector<uint64_t> masks(n_out, 0);
        Resolver where(*this);
        Plan plan;
        if (plan.add(where, terms, {}, Absent::EmptyGroup).empty() || !n_out) return masks;      // no term in any segment: every row is 0
        DevMem d_ids(ctx_), d_masks(ctx_);
        ck(ctx_, ii2_dev_alloc(ctx_, ids.size() * sizeof(uint32_t), &d_ids.p), "matched terms");
        ck(ctx_, ii2_dev_alloc(ctx_, n_out * sizeof(uint64_t), &d_masks.p), "matched terms");
        ck(ctx_, ii2_copy_h2d(ctx_, d_ids.p, ids.data(), ids.size() * sizeof(uint32_t)), "matched terms");
        ck(ctx_, ii2_explain_ranges(ctx_, plan.n_groups(), plan.group_first.data(), plan.segs.data(), plan.first.data(), plan.end.data(),
                                    (const uint32_t *)d_ids.p, ids.size(), (uint64_t *)d_masks.p, n_out, nullptr), "matched terms");
        ck(ctx_, ii2_copy_d2h(ctx_, masks.data(), d_masks.p, n_out * sizeof(uint64_t)), "matched terms");
        return masks;
    }
    // additive: MatchedTerms for MANY pages - the screenful of ranked pages IntersectTopBatch returns, each against its own terms -
    // in one device call; result p is that of MatchedTerms(pages[p].ids, pages[p].terms).  Per page the groups are built exactly as
    // MatchedTerms builds them (a term found in no segment keeps its bit and never sets it; a page none of whose terms is in a
    // segment keeps its place without a group: its rows are 0), the terms resolved through Resolver::prepare like
    // IntersectTopBatch's; one upload of all ids, ONE ii2_explain_batch call and one download.
    struct TermsPage {
        std::vector<uint32_t> ids;
        std::vector<Term> terms;
    };
    std::vector<std::vector<uint64_t>> MatchedTermsBatch(const std::vector<TermsPage> &pages) const {
        std::vector<std::vector<uint64_t>> out(pages.size());
        if (pages.empty()) return out;
        const std::vector<Term> none;
        Resolver where(*this);
        where.prepare(pages.size(), [&](size_t p, bool ex) -> const std::vector<Term> & { return ex ? none : pages[p].terms; });
        Plan plan;
        std::vector<uint32_t> ids;
        std::vector<uint64_t> ids_off(1, 0), mask_off(pages.size() + 1, 0);
        uint64_t n_out = 0;
        for (size_t p = 0; p < pages.size(); p++) {
            const TermsPage &P = pages[p];
            if (P.ids.size() > II2_EXPLAIN_MAX_IDS) throw std::runtime_error("matched terms batch: page " + std::to_string(p) + ": more than II2_EXPLAIN_MAX_IDS ids");
            out[p].assign(P.ids.size() * ((P.terms.size() + 63) / 64), 0);
            if (!plan.add(where, P.terms, none, Absent::EmptyGroup).empty()) n_out += out[p].size();      // (else: no group, no row on the device)
            ids.insert(ids.end(), P.ids.begin(), P.ids.end());
            ids_off.push_back(ids.size());
        }
        if (!n_out) return out;
        DevMem d_ids(ctx_), d_masks(ctx_);
        ck(ctx_, ii2_dev_alloc(ctx_, ids.size() * sizeof(uint32_t), &d_ids.p), "matched terms batch");
        ck(ctx_, ii2_dev_alloc(ctx_, n_out * sizeof(uint64_t), &d_masks.p), "matched terms batch");
        ck(ctx_, ii2_copy_h2d(ctx_, d_ids.p, ids.data(), ids.size() * sizeof(uint32_t)), "matched terms batch");
        ck(ctx_, ii2_explain_batch(ctx_, pages.size(), plan.query_first.data(), plan.group_first.data(), plan.segs.data(), plan.first.data(), plan.end.data(),
                                   (const uint32_t *)d_ids.p, ids_off.data(), (uint64_t *)d_masks.p, n_out, mask_off.data(), nullptr), "matched terms batch");
        std::vector<uint64_t> words(n_out);
        ck(ctx_, ii2_copy_d2h(ctx_, words.data(), d_masks.p, n_out * sizeof(uint64_t)), "matched terms batch");
        for (size_t p = 0; p < pages.size(); p++)
            if (mask_off[p + 1] > mask_off[p]) std::copy(words.begin() + mask_off[p], words.begin() + mask_off[p + 1], out[p].begin());
        return out;
    }
    // additive: IntersectTop with a weight per term (an idf tier, a field boost): a doc's score is the sum of the weights of the terms it
    // lies under, 1 .. 255 each and at most 255 together; at least min_score.  The groups are IntersectTop's - a term found in no
    // segment keeps its slot, and its weight, and matches nothing - and the call is ONE ii2_topk_weighted_ranges.
    std::vector<std::pair<uint32_t, uint32_t>> IntersectTopWeighted(const std::vector<Term> &terms, const std::vector<uint32_t> &weights, uint64_t k,
                                                                    uint32_t min_score, const std::vector<Term> &except) const {
        if (!min_score) throw std::runtime_error("intersect top weighted: min_score is 0");
        if (weights.size() != terms.size()) throw std::runtime_error("intersect top weighted: one weight per term");
        if (k > II2_TOPK_MAX) throw std::runtime_error("intersect top weighted: k above II2_TOPK_MAX");
        Resolver where(*this);
        Plan plan;
        if (plan.add(where, terms, except, Absent::EmptyGroup, &weights).empty() || !k) return {};
        return ranked(k, "intersect top weighted", [&](uint32_t *d_ids, uint32_t *d_scores, uint64_t *n) {
            return ii2_topk_weighted_ranges(ctx_, plan.n_groups(), plan.group_first.data(), plan.group_not.data(), plan.group_weight.data(), min_score,
                                            k, plan.segs.data(), plan.first.data(), plan.end.data(), nullptr, d_ids, d_scores, n, nullptr, nullptr);
        });
    }
    // additive: MANY IntersectTopWeighted queries in one ii2_topk_batch call (through two_call) and one download; result q is that
    // of IntersectTopWeighted(queries[q]...).  Per query the groups are built exactly as IntersectTopWeighted builds them; a query
    // none of whose terms is in a segment keeps its place without a group - its result is empty, the call goes on.  The output's
    // size: per query min(k, the postings bounds of its terms).  The library takes result bounds below 2^32 ids per call
    // (II2_ERANGE beyond).
    struct TopQuery {
        std::vector<Term> terms;
        std::vector<uint32_t> weights;
        uint64_t k;
        uint32_t min_score;
        std::vector<Term> except;
    };
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> IntersectTopBatch(const std::vector<TopQuery> &queries) const {
        std::vector<std::vector<std::pair<uint32_t, uint32_t>>> out(queries.size());
        if (queries.empty()) return out;
        Resolver where(*this);
        where.prepare(queries.size(), [&](size_t q, bool ex) -> const std::vector<Term> & { return ex ? queries[q].except : queries[q].terms; });
        Plan plan;
        std::vector<uint32_t> min_score, ks;
        uint64_t total = 0;
        const std::vector<Term> none;
        for (size_t q = 0; q < queries.size(); q++) {
            const TopQuery &Q = queries[q];
            const std::string who = "intersect top batch: query " + std::to_string(q);
            if (!Q.min_score) throw std::runtime_error(who + ": min_score is 0");
            if (Q.weights.size() != Q.terms.size()) throw std::runtime_error(who + ": one weight per term");
            if (Q.k > II2_TOPK_MAX) throw std::runtime_error(who + ": k above II2_TOPK_MAX");
            min_score.push_back(Q.min_score);
            ks.push_back((uint32_t)Q.k);
            uint64_t post = 0;                                   // (k = 0 asks for nothing: a query without terms)
            for (uint64_t p : plan.add(where, Q.k ? Q.terms : none, Q.except, Absent::EmptyGroup, &Q.weights)) post += p;
            total += std::min(Q.k, post);
        }
        std::vector<uint64_t> off(queries.size() + 1, 0);
        const Output o = two_call(total, 2, "intersect top batch", [&](uint32_t *d_ids, uint64_t cap, uint64_t *n) {      // ids [0, cap), then scores [cap, 2 cap)
            const int rc = ii2_topk_batch(ctx_, queries.size(), plan.query_first.data(), plan.group_first.data(), plan.group_not.data(),
                                          plan.group_weight.data(), min_score.data(), ks.data(), plan.segs.data(), plan.first.data(), plan.end.data(),
                                          nullptr, d_ids, d_ids + cap, cap, off.data(), nullptr, nullptr);
            *n = off.back();
            return rc;
        });
        const std::vector<uint32_t> raw = download(o.mem, o.n ? o.cap + o.n : 0, "intersect top batch");
        for (size_t q = 0; q < queries.size(); q++)
            for (uint64_t i = off[q]; i < off[q + 1]; i++) out[q].push_back({raw[i], raw[o.cap + i]});
        return out;
    }
   private:
    // ---- terms -> lists: where the terms of a query live ----
    // One (segment, list) per segment of the term's shard that holds the term, in the order of the shard's snapshot.
    using TermHits = std::vector<std::pair<std::shared_ptr<Segment>, uint64_t>>;
    // (term, segment) pairs - the call's distinct terms times the segments of their shards - from which a bulk call looks its terms
    // up on the device in mode -1: the smallest measured count at which that beat the host bisection (8 segments of 100 000
    // terms, MI355X: 159 against 182 us at 768 pairs, 129 against 82 us at 384)
    static constexpr uint64_t RESOLVE_MIN_PAIRS = 768;
    // The lookup of a query's terms.  As made it bisects the host dictionaries, one std::lower_bound per (term, segment) and call.
    // prepare() - the bulk calls - may move the whole call's lookups to the device instead (ii2h_set_resolve): per shard the
    // call's distinct terms that hash to it are probed against all segments of ONE snapshot by ii2_dict_find, at most
    // II2_MAX_LISTS dictionaries per call, and append() then only reads the answers.  The ranges are the same either way.
    // `remember`: the host bisection keeps its answers too, so a term asked for again gets the same lists without a second
    // lookup (TermCounts lays its filter out once more per re-counted term).
    class Resolver {
       public:
        explicit Resolver(const InvertedIndex &ix, bool remember = false) : ix_(ix), remember_(remember) {}
        // terms_of(q, false / true): the required / excluded terms of query q
        template <class TermsOf> void prepare(size_t n_queries, TermsOf terms_of) {
            const int mode = ix_.resolve_mode_.load();
            if (mode == 0) return;
            std::map<uint32_t, std::vector<const Term *>> by_shard;      // the call's distinct terms
            for (size_t q = 0; q < n_queries; q++)
                for (int ex = 0; ex < 2; ex++)
                    for (const Term &t : terms_of(q, ex != 0))
                        if (found_.emplace(t, TermHits()).second) by_shard[shard_key(t)].push_back(&t);
            std::vector<std::pair<std::vector<std::shared_ptr<Segment>>, const std::vector<const Term *> *>> work;
            uint64_t pairs = 0;
            for (auto &st : by_shard)
                if (Shard *sh = ix_.find_shard(st.first)) {
                    work.emplace_back(sh->snapshot(), &st.second);
                    pairs += (uint64_t)work.back().first.size() * st.second.size();
                }
            if (mode < 0 && pairs < RESOLVE_MIN_PAIRS) { found_.clear(); return; }
            device_ = true;
            std::vector<uint8_t> bytes;
            std::vector<uint64_t> off, lo, hi;
            std::vector<const ii2_dict *> dicts;
            for (auto &w : work) {
                const std::vector<std::shared_ptr<Segment>> &snap = w.first;
                const std::vector<const Term *> &probes = *w.second;
                bytes.assign(1, 0);                                      // (never an empty array)
                off.assign(1, 0);
                for (const Term *t : probes) {
                    bytes.insert(bytes.end() - 1, t->begin(), t->end());
                    off.push_back(bytes.size() - 1);
                }
                for (size_t s0 = 0; s0 < snap.size(); s0 += II2_MAX_LISTS) {
                    const size_t k = std::min<size_t>(II2_MAX_LISTS, snap.size() - s0);
                    dicts.clear();
                    for (size_t s = 0; s < k; s++) dicts.push_back(snap[s0 + s]->resident_dict(ix_.ctx_));
                    lo.assign(probes.size() * k, 0);
                    hi.assign(probes.size() * k, 0);
                    ck(ix_.ctx_, ii2_dict_find(ix_.ctx_, (uint32_t)k, dicts.data(), probes.size(), bytes.data(), off.data(), nullptr, II2_HOST, lo.data(),
                                               hi.data(), nullptr), "resolve");
                    for (size_t p = 0; p < probes.size(); p++) {
                        TermHits &hits = found_[*probes[p]];
                        for (size_t s = 0; s < k; s++)
                            if (hi[p * k + s] > lo[p * k + s]) hits.emplace_back(snap[s0 + s], lo[p * k + s]);
                    }
                }
            }
        }
        // One one-list range per segment that holds the term; returns the term's postings bound, 0: in no segment.  The bound:
        // the C ABI gives no per-list counts, so a term is bounded by its segments - a list of a segment holds at most its
        // postings minus one per other list (every list a shard's segment holds is non-empty: a Put writes one posting per term,
        // a merge drops empty terms), exact for Put segments, loose for merged ones.
        uint64_t append(const Term &t, std::vector<std::shared_ptr<Segment>> &held, std::vector<const ii2_seg *> &segs, std::vector<uint64_t> &first,
                        std::vector<uint64_t> &end) {
            uint64_t post = 0;
            auto take = [&](const std::shared_ptr<Segment> &sg, uint64_t j) {
                ii2_seg_info info;
                ii2_seg_get_info(sg->seg->h, &info);
                held.push_back(sg);
                segs.push_back(sg->seg->h);
                first.push_back(j);
                end.push_back(j + 1);
                post += info.n_postings > info.n_lists ? info.n_postings - (info.n_lists - 1) : 1;
            };
            if (remember_ && !found_.count(t)) bisect(t, [&, &hits = found_[t]](const std::shared_ptr<Segment> &sg, uint64_t j) { hits.emplace_back(sg, j); });
            if (device_ || remember_) {
                for (auto &hit : found_.at(t)) take(hit.first, hit.second);
            } else {
                bisect(t, take);
            }
            return post;
        }

       private:
        // the host lookup: fn(segment, list) for every segment of the term's shard that holds it, in the order of the shard's snapshot
        template <class Fn> void bisect(const Term &t, Fn fn) const {
            if (Shard *sh = ix_.find_shard(shard_key(t))) {
                for (auto &sg : sh->snapshot()) {
                    const std::vector<Term> &T = sg->terms;
                    const size_t j = std::lower_bound(T.begin(), T.end(), t, term_less) - T.begin();
                    if (j != T.size() && T[j] == t) fn(sg, j);
                }
            }
        }
        const InvertedIndex &ix_;
        const bool remember_;
        bool device_ = false;
        std::unordered_map<Term, TermHits> found_;
    };
    // ---- the query plan: what the range and batch entry points take ----
    // What a required term found in no segment does to its query: the AND forms have nothing under every term, the at-least and
    // ranked forms keep the term as a group without ranges (it matches no doc and keeps its slot and weight).
    enum class Absent { EmptyQuery, EmptyGroup };
    using Lists = std::vector<std::pair<const ii2_seg *, uint64_t>>;      // (segment, list)
    // Queries as flat arrays: query q owns the groups query_first[q] .. query_first[q + 1] - 1, group g the ranges group_first[g] ..
    // group_first[g + 1] - 1 - one one-list range per segment of the term's shard that holds the term.  A single query is a plan of
    // one query (the range entry points take group_first on and ignore query_first).
    struct Plan {
        std::vector<std::shared_ptr<Segment>> held;          // the segments read, alive until the call is done
        std::vector<uint64_t> query_first{0}, group_first{0}, first, end;
        std::vector<uint8_t> group_not;
        std::vector<uint32_t> group_weight;                  // filled for the queries added with weights
        std::vector<const ii2_seg *> segs;
        size_t n_groups() const { return group_not.size(); }
        // Appends one query: a group per required term, then `extra` - lists given directly - as one more required group, then a
        // flagged group per excluded term (the packers lay a query out that way: the required groups first, the excluded ones
        // last; an excluded group's weight is 0 and ignored).  An excluded term found in no segment removes nothing and is dropped.
        // A query that turns out empty - `rule` says what an absent required term means; no required term and no `extra`, or under
        // EmptyGroup no required term found - is undone: it keeps its place, without a group.  Returns the postings bounds of the
        // required terms found, in their order (none for an empty query), valid until the next add: each caller derives its
        // output bound from them.
        const std::vector<uint64_t> &add(Resolver &where, const std::vector<Term> &terms, const std::vector<Term> &except, Absent rule,
                                         const std::vector<uint32_t> *weights = nullptr, const Lists *extra = nullptr) {
            const size_t g_mark = group_not.size(), r_mark = segs.size();
            auto close_group = [&](uint8_t flag, uint32_t weight) {
                group_first.push_back(segs.size());
                group_not.push_back(flag);
                if (weights) group_weight.push_back(weight);
            };
            posts_.clear();
            bool nothing = false;                                // under EmptyQuery: a required term in no segment, the others are not looked up
            for (size_t i = 0; i < terms.size() && !nothing; i++) {
                const uint64_t post = where.append(terms[i], held, segs, first, end);
                if (post) posts_.push_back(post);
                nothing = !post && rule == Absent::EmptyQuery;
                close_group(0, weights ? (*weights)[i] : 0u);
            }
            if (extra) {
                for (auto &sl : *extra) {
                    segs.push_back(sl.first);
                    first.push_back(sl.second);
                    end.push_back(sl.second + 1);
                }
                close_group(0, 0u);
            }
            if (nothing || (posts_.empty() && !extra)) {
                posts_.clear();
                group_first.resize(g_mark + 1);
                group_not.resize(g_mark);
                if (weights) group_weight.resize(g_mark);
                segs.resize(r_mark);
                first.resize(r_mark);
                end.resize(r_mark);
            } else {
                for (auto &t : except)
                    if (where.append(t, held, segs, first, end)) close_group(1, 0u);
            }
            query_first.push_back(group_not.size());
            return posts_;
        }

       private:
        std::vector<uint64_t> posts_;
    };
    // the output bound of an AND query: its smallest term's (0: the query is empty)
    static uint64_t smallest(const std::vector<uint64_t> &posts) { return posts.empty() ? 0 : *std::min_element(posts.begin(), posts.end()); }

    // ---- the two-call output protocol ----
    // The bounds above may be a whole merged segment, so no call allocates more than FIRST_CAP ids at first: a result that does not
    // fit is written by a second call with the size the first one reported (II2_ECAPACITY writes nothing; the batch calls fill
    // their offsets under it).  Either call passes one entry more than it needs.  `arrays`: the uint32 arrays of `cap` entries the output holds, back to back (1: ids, 2: ids then
    // scores).  call(d_out, cap, &n) makes the library call and returns its rc, n = the size it reported.
    static constexpr uint64_t FIRST_CAP = FIRST_CAP_IDS;
    using Output = DevOutput;
    template <class Call> Output two_call(uint64_t bound, unsigned arrays, const char *what, Call call) const {
        return two_call_dev(ctx_, first_cap_.load(), &second_calls_, bound, arrays, what, call);
    }
    std::vector<uint32_t> download(const DevMem &d, uint64_t n, const char *what) const {
        std::vector<uint32_t> v(n);
        if (n) ck(ctx_, ii2_copy_d2h(ctx_, v.data(), d.p, n * sizeof(uint32_t)), what);
        return v;
    }
    // ONE ii2_andnot_ranges call - min_match > 0: ONE ii2_atleast_ranges call - over a plan of one query; the result stays on the device
    Output filter_run(const Plan &f, uint64_t bound, const char *what, uint32_t min_match = 0) const {
        return two_call(bound, 1, what, [&](uint32_t *d_ids, uint64_t cap, uint64_t *n) {
            return min_match ? ii2_atleast_ranges(ctx_, f.n_groups(), f.group_first.data(), f.group_not.data(), min_match, f.segs.data(), f.first.data(),
                                                  f.end.data(), nullptr, d_ids, cap, n, nullptr)
                             : ii2_andnot_ranges(ctx_, f.n_groups(), f.group_first.data(), f.group_not.data(), f.segs.data(), f.first.data(),
                                                 f.end.data(), nullptr, d_ids, cap, n);
        });
    }
    // the tail of the two single ranked methods: exactly 2k entries - ids [0, k), then scores [k, 2k); a ranked result never
    // exceeds k, so there is no second call - one call, one download, the (id, score) pairs
    template <class Call> std::vector<std::pair<uint32_t, uint32_t>> ranked(uint64_t k, const char *what, Call call) const {
        DevMem d_out(ctx_);
        ck(ctx_, ii2_dev_alloc(ctx_, 2 * k * sizeof(uint32_t), &d_out.p), what);
        uint64_t n = 0;
        ck(ctx_, call((uint32_t *)d_out.p, (uint32_t *)d_out.p + k, &n), what);
        const std::vector<uint32_t> raw = download(d_out, n ? k + n : 0, what);
        std::vector<std::pair<uint32_t, uint32_t>> out(n);
        for (uint64_t i = 0; i < n; i++) out[i] = {raw[i], raw[k + i]};
        return out;
    }
    // ---- a prefix's lists ----
    // fn(prefix, segment, j0, j1) for every non-empty run of lists of every prefix (sorted, distinct) in every segment of every
    // shard, shard by shard in key order.  A shard whose MinMax excludes a prefix is not read for it.  In a segment the terms that
    // start with a prefix are one run, [lower_bound(prefix), the first term after it that does not start with it), and every run is
    // cut at the end of the GREATEST prefix's run: the reference stops reading a shard at the first term past the greatest prefix
    // (its first len(greatest) bytes compare greater; inverted_index.go:192-295), so with prefixes a and ab the run of a ends
    // where the run of ab ends.
    template <class Fn> void prefix_runs(const std::vector<Term> &prefixes, Fn fn) const {
        for (auto &s : shard_list()) {
            Term mn, mx;
            if (!s.second->MinMax(&mn, &mx)) continue;
            std::vector<const Term *> mine;
            for (auto &p : prefixes) {
                size_t l = std::min(p.size(), mn.size());
                if (p.compare(0, l, mn, 0, l) < 0) continue;
                l = std::min(p.size(), mx.size());
                if (p.compare(0, l, mx, 0, l) > 0) continue;
                mine.push_back(&p);
            }
            if (mine.empty()) continue;
            for (auto &sg : s.second->snapshot()) {
                const std::vector<Term> &T = sg->terms;
                const size_t stop = prefix_end(T, *mine.back());
                for (const Term *p : mine) {
                    const size_t j0 = std::lower_bound(T.begin(), T.end(), *p, term_less) - T.begin();
                    const size_t j1 = std::min(prefix_end(T, *p), stop);
                    if (j0 < j1) fn(*p, sg, j0, j1);
                }
            }
        }
    }

   public:
    // additive: facet counts - for every term that starts with `prefix` the number of distinct docs under it that
    // IntersectExcept(terms, except) returns; terms with count 0 are omitted.  With `terms` empty the doc set is "every doc" and
    // the result is the document frequency of each term under the prefix (`except` must then be empty too: there is no doc
    // universe to take it from).  The filter result stays on the device, and ONE ii2_count_ranges call counts the prefix's run
    // of every segment of every shard against it - the runs are found as PrefixSearch finds them.  Per term the per-segment
    // counts are summed.  Nothing stops a (term, doc) pair from being Put again, so a term whose hits come from two or more
    // segments may hold the same doc twice: those terms alone are counted again exactly, all of them in ONE
    // ii2_query_batch_groups call - the query's groups plus the term's group, no output buffer, the sizes read from the offsets it
    // fills under II2_ECAPACITY.  Like Read and Intersect, no tombstone filter.
    std::map<Term, uint64_t> TermCounts(const Term &prefix, const std::vector<Term> &terms, const std::vector<Term> &except) const {
        std::map<Term, uint64_t> out;
        if (terms.empty() && !except.empty()) throw Error("term counts: an exclusion needs a required term");
        Resolver where(*this, true);                             // (the re-count lays the filter's terms out again: the same lists)
        Output set{DevMem(ctx_), 0, 0};
        if (!terms.empty()) {
            Plan filter;
            const uint64_t bound = smallest(filter.add(where, terms, except, Absent::EmptyQuery));
            if (!bound) return out;
            set = filter_run(filter, bound, "term counts");
            if (!set.n) return out;
        }
        // the prefix's run in every segment of every shard
        std::vector<std::shared_ptr<Segment>> held;
        std::vector<const ii2_seg *> segs;
        std::vector<uint64_t> first, end;
        uint64_t n_named = 0;
        prefix_runs({prefix}, [&](const Term &, const std::shared_ptr<Segment> &sg, size_t j0, size_t j1) {
            held.push_back(sg);
            segs.push_back(sg->seg->h);
            first.push_back(j0);
            end.push_back(j1);
            n_named += j1 - j0;
        });
        if (segs.empty()) return out;
        std::vector<uint64_t> counts(n_named);
        ck(ctx_, ii2_count_ranges(ctx_, segs.size(), segs.data(), first.data(), end.data(), terms.empty() ? nullptr : (const uint32_t *)set.mem.p, set.n,
                                  nullptr, counts.data(), counts.size(), nullptr),
           "term counts");
        // per term: the sum over its segments, and the lists that hit
        struct Hit {
            uint64_t sum = 0;
            Lists lists;                                         // (segment, list) of every segment with a hit
        };
        std::map<Term, Hit> hits;
        size_t k = 0;
        for (size_t r = 0; r < segs.size(); r++)
            for (uint64_t j = first[r]; j < end[r]; j++, k++) {
                if (!counts[k]) continue;
                Hit &h = hits[held[r]->terms[j]];
                h.sum += counts[k];
                h.lists.emplace_back(segs[r], j);
            }
        std::vector<const Term *> again;
        for (auto &kv : hits) {
            out[kv.first] = kv.second.sum;
            if (kv.second.lists.size() > 1) again.push_back(&kv.first);
        }
        // the exact re-count: per term one query of the filter's groups plus the term's own (for "every doc" that group alone),
        // in calls of at most 2^20 queries whose result bounds stay below 2^32 ids
        constexpr size_t CALL_QUERIES = 1u << 20;
        constexpr uint64_t CALL_IDS = 0xFFFFFFFFull;
        size_t at = 0;
        while (at < again.size()) {
            Plan plan;
            uint64_t bound = 0;
            const size_t q0 = at;
            for (; at < again.size() && at - q0 < CALL_QUERIES; at++) {
                const Hit &h = hits[*again[at]];
                if (at > q0 && bound + h.sum >= CALL_IDS) break;
                bound += h.sum;                                  // (the term's group holds at least its hits; the result is no longer)
                plan.add(where, terms, except, Absent::EmptyQuery, nullptr, &h.lists);
            }
            const size_t nq = at - q0;
            std::vector<uint64_t> off(nq + 1, 0);
            const int rc = ii2_query_batch_groups(ctx_, nq, plan.query_first.data(), plan.group_first.data(), plan.group_not.data(), plan.segs.data(),
                                                  plan.first.data(), plan.end.data(), nullptr, nullptr, 0, off.data());
            if (rc != II2_ECAPACITY) ck(ctx_, rc, "term counts");
            for (size_t q = 0; q < nq; q++) {
                const uint64_t c = off[q + 1] - off[q];
                if (c) out[*again[q0 + q]] = c;
                else out.erase(*again[q0 + q]);
            }
        }
        return out;
    }
    // the buckets of a histogram's axis, its edges checked as the library checks them - by ii2_hist_bucket, which needs no device - so
    // that bad edges are an error even where nothing is left to count
    static uint32_t hist_buckets(const std::vector<uint64_t> &edges, const char *what) {
        if (edges.size() < 2) throw Error(std::string(what) + ": fewer than two edges");
        int64_t b = 0;
        const int rc = ii2_hist_bucket(edges.data(), (uint32_t)std::min<size_t>(edges.size() - 1, 0xFFFFFFFFu), 0, &b);
        if (rc == II2_ERANGE) throw Error(std::string(what) + ": more than II2_HIST_MAX_BUCKETS buckets");
        if (rc) throw Error(std::string(what) + ": the edges are not strictly ascending values <= 2^32");
        return (uint32_t)(edges.size() - 1);
    }
    // additive: the date histogram of a query - how many of the ids that IntersectExcept(terms, except) returns fall into each bucket
    // of the value axis: edges = n_buckets + 1 strictly ascending values <= 2^32, bucket b = the ids edges[b] <= id < edges[b + 1]
    // (2^32 as the last edge includes id 0xFFFFFFFF); ids outside the axis are counted nowhere.  IntersectExcept's body up to the
    // download: the result stays on the device and ONE ii2_histogram_ids call counts it.  Like Intersect, no tombstone filter.
    std::vector<uint64_t> Histogram(const std::vector<Term> &terms, const std::vector<Term> &except, const std::vector<uint64_t> &edges) const {
        std::vector<uint64_t> out(hist_buckets(edges, "histogram"), 0);
        Resolver where(*this);
        Plan plan;
        const uint64_t bound = smallest(plan.add(where, terms, except, Absent::EmptyQuery));
        if (!bound) return out;
        const Output set = filter_run(plan, bound, "histogram");
        ck(ctx_, ii2_histogram_ids(ctx_, (const uint32_t *)set.mem.p, set.n, nullptr, (uint32_t)out.size(), edges.data(), out.data(), out.size()), "histogram");
        return out;
    }
    // additive: terms over time - TermCounts over the value axis of Histogram: for every term that starts with `prefix`, per bucket
    // the number of distinct docs under it that IntersectExcept(terms, except) returns; terms with an all-zero row are omitted.
    // With `terms` empty the doc set is "every doc": each term's frequency over time (`except` must then be empty too).  TermCounts'
    // plan with ONE ii2_histogram_ranges call over the prefix's runs; per term the per-segment rows are summed.  A term that hits
    // in two or more segments may hold a doc twice, so those terms alone are counted again exactly: ONE ii2_query_batch_groups
    // call per 2^20 of them - the filter's groups plus the term's own, the results kept on the device - and one ii2_histogram_ids
    // call per such term on its slice of the output.  Like Read and Intersect, no tombstone filter.
    std::map<Term, std::vector<uint64_t>> TermHistogram(const Term &prefix, const std::vector<Term> &terms, const std::vector<Term> &except,
                                                        const std::vector<uint64_t> &edges) const {
        std::map<Term, std::vector<uint64_t>> out;
        if (terms.empty() && !except.empty()) throw Error("term histogram: an exclusion needs a required term");
        const uint32_t nb = hist_buckets(edges, "term histogram");
        Resolver where(*this, true);                             // (the re-count lays the filter's terms out again: the same lists)
        Output set{DevMem(ctx_), 0, 0};
        if (!terms.empty()) {
            Plan filter;
            const uint64_t bound = smallest(filter.add(where, terms, except, Absent::EmptyQuery));
            if (!bound) return out;
            set = filter_run(filter, bound, "term histogram");
            if (!set.n) return out;
        }
        // the prefix's run in every segment of every shard, in calls of at most II2_HIST_MAX_CELLS counters
        std::vector<std::shared_ptr<Segment>> held;
        std::vector<const ii2_seg *> segs;
        std::vector<uint64_t> first, end;
        const uint64_t call_lists = std::max<uint64_t>(1, II2_HIST_MAX_CELLS / nb);
        prefix_runs({prefix}, [&](const Term &, const std::shared_ptr<Segment> &sg, size_t j0, size_t j1) {
            for (uint64_t j = j0; j < j1; j += call_lists) {         // (a run longer than a call's lists is cut)
                held.push_back(sg);
                segs.push_back(sg->seg->h);
                first.push_back(j);
                end.push_back(std::min<uint64_t>(j + call_lists, j1));
            }
        });
        struct Hit {
            std::vector<uint64_t> row;
            Lists lists;                                         // (segment, list) of every segment with a hit
        };
        std::map<Term, Hit> hits;
        std::vector<uint64_t> counts;
        for (size_t r0 = 0; r0 < segs.size();) {
            size_t r1 = r0;
            uint64_t n_named = 0;
            for (; r1 < segs.size() && (r1 == r0 || n_named + (end[r1] - first[r1]) <= call_lists); r1++) n_named += end[r1] - first[r1];
            counts.assign(n_named * nb, 0);
            ck(ctx_, ii2_histogram_ranges(ctx_, r1 - r0, segs.data() + r0, first.data() + r0, end.data() + r0, terms.empty() ? nullptr : (const uint32_t *)set.mem.p,
                                          set.n, nullptr, nb, edges.data(), counts.data(), counts.size(), nullptr),
               "term histogram");
            size_t k = 0;
            for (size_t r = r0; r < r1; r++)
                for (uint64_t j = first[r]; j < end[r]; j++, k++) {
                    const uint64_t *row = counts.data() + k * nb;
                    if (std::all_of(row, row + nb, [](uint64_t c) { return c == 0; })) continue;
                    Hit &h = hits[held[r]->terms[j]];
                    h.row.resize(nb, 0);
                    for (uint32_t b = 0; b < nb; b++) h.row[b] += row[b];
                    h.lists.emplace_back(segs[r], j);
                }
            r0 = r1;
        }
        std::vector<const Term *> again;
        for (auto &kv : hits) {
            out[kv.first] = kv.second.row;
            if (kv.second.lists.size() > 1) again.push_back(&kv.first);
        }
        // the exact re-count, as TermCounts lays it out - but the results are written: each term's slice is counted per bucket
        constexpr size_t CALL_QUERIES = 1u << 20;
        constexpr uint64_t CALL_IDS = 0xFFFFFFFFull;
        size_t at = 0;
        while (at < again.size()) {
            Plan plan;
            uint64_t bound = 0;
            const size_t q0 = at;
            for (; at < again.size() && at - q0 < CALL_QUERIES; at++) {
                const Hit &h = hits[*again[at]];
                uint64_t sum = 0;
                for (uint64_t c : h.row) sum += c;
                if (at > q0 && bound + sum >= CALL_IDS) break;
                bound += sum;                                    // (the term's group holds at least its hits; the result is no longer)
                plan.add(where, terms, except, Absent::EmptyQuery, nullptr, &h.lists);
            }
            const size_t nq = at - q0;
            std::vector<uint64_t> off(nq + 1, 0);
            const Output o = two_call(bound, 1, "term histogram", [&](uint32_t *d_ids, uint64_t cap, uint64_t *n) {
                const int rc = ii2_query_batch_groups(ctx_, nq, plan.query_first.data(), plan.group_first.data(), plan.group_not.data(), plan.segs.data(),
                                                      plan.first.data(), plan.end.data(), nullptr, d_ids, cap, off.data());
                *n = off.back();
                return rc;
            });
            for (size_t q = 0; q < nq; q++) {
                std::vector<uint64_t> &row = out[*again[q0 + q]];
                ck(ctx_, ii2_histogram_ids(ctx_, (const uint32_t *)o.mem.p + off[q], off[q + 1] - off[q], nullptr, nb, edges.data(), row.data(), row.size()),
                   "term histogram");
                if (std::all_of(row.begin(), row.end(), [](uint64_t c) { return c == 0; })) out.erase(*again[q0 + q]);
            }
        }
        return out;
    }
    // additive: MANY IntersectExcept queries, queries[q] = (terms, except), in one ii2_query_batch_groups call (through two_call),
    // one wait and one download.  Per term the groups are built exactly as IntersectExcept builds them.  A required term found in
    // no segment (or no term at all) makes that query one without groups - its result is empty, the call goes on.  The output's
    // size: per query the smallest REQUIRED term's bound.  The library takes result bounds below 2^32 ids per call (II2_ERANGE
    // beyond: send such a bulk in parts).  Like Intersect and Read, no tombstone filter.
    std::vector<std::vector<uint32_t>> IntersectMany(const std::vector<std::pair<std::vector<Term>, std::vector<Term>>> &queries) const {
        std::vector<std::vector<uint32_t>> out(queries.size());
        if (queries.empty()) return out;
        Resolver where(*this);
        where.prepare(queries.size(), [&](size_t q, bool ex) -> const std::vector<Term> & { return ex ? queries[q].second : queries[q].first; });
        Plan plan;
        uint64_t total = 0;
        for (auto &qe : queries) total += smallest(plan.add(where, qe.first, qe.second, Absent::EmptyQuery));
        std::vector<uint64_t> off(queries.size() + 1, 0);
        const Output o = two_call(total, 1, "intersect batch", [&](uint32_t *d_ids, uint64_t cap, uint64_t *n) {
            const int rc = ii2_query_batch_groups(ctx_, queries.size(), plan.query_first.data(), plan.group_first.data(), plan.group_not.data(),
                                                  plan.segs.data(), plan.first.data(), plan.end.data(), nullptr, d_ids, cap, off.data());
            *n = off.back();
            return rc;
        });
        std::vector<uint32_t> all(o.n);
        if (o.n) ck(ctx_, ii2_copy_d2h(ctx_, all.data(), o.mem.p, o.n * sizeof(uint32_t)), "intersect batch");
        for (size_t q = 0; q < queries.size(); q++) out[q].assign(all.begin() + off[q], all.begin() + off[q + 1]);
        return out;
    }
    // tests: the first call of two_call allocates at most `ids` ids (1 .. FIRST_CAP, the default), so that a small index reaches the
    // second call; SecondCalls counts those
    void SetFirstCap(uint64_t ids) {
        if (ids < 1 || ids > FIRST_CAP) throw Error("set first cap: 1 to 2^22 ids");
        first_cap_.store(ids);
    }
    uint64_t SecondCalls() const { return second_calls_.load(); }
    // additive: how IntersectMany and IntersectTopBatch turn their terms into lists - 0: bisections of the host dictionaries, 1:
    // ii2_dict_find on resident dictionaries, -1 (the default): the device from RESOLVE_MIN_PAIRS (term, segment) pairs per call.
    // The results are the same in every mode.
    void SetResolve(int mode) {
        if (mode < -1 || mode > 1) throw Error("set resolve: mode is -1, 0 or 1");
        resolve_mode_.store(mode);
    }
    // additive: where every shard's PutBatch sorts and looks up its terms (Shard::SetBuild), for the shards there are and the ones to come
    void SetBuild(int mode) {
        if (mode < -1 || mode > 1) throw Error("set build: mode is -1, 0 or 1");
        std::lock_guard<std::mutex> g(mu_);
        build_mode_ = mode;
        for (auto &s : shards_) s.second->SetBuild(mode);
    }
    size_t ShardCount() const { std::lock_guard<std::mutex> g(mu_); return shards_.size(); }
    size_t SegmentCount() const { size_t n = 0; for (auto &s : shard_list()) n += s.second->SegmentCount(); return n; }      // over all shards
    Shard *OnlyShard() { std::lock_guard<std::mutex> g(mu_); return shards_.empty() ? nullptr : shards_.begin()->second.get(); }

   private:
    // the first term at or after `p` in the sorted dictionary T that does not start with p (the terms that do are one run)
    static size_t prefix_end(const std::vector<Term> &T, const Term &p) {
        return std::partition_point(T.begin(), T.end(), [&](const Term &t) { return term_less(t, p) || t.compare(0, p.size(), p) == 0; }) - T.begin();
    }
    // shards are never removed: a snapshot of (key, pointer) pairs in key order is all a reader needs (ii.shardsM)
    std::vector<std::pair<uint32_t, Shard *>> shard_list() const {
        std::lock_guard<std::mutex> g(mu_);
        std::vector<std::pair<uint32_t, Shard *>> v;
        for (auto &s : shards_) v.emplace_back(s.first, s.second.get());
        return v;
    }
    std::vector<std::shared_ptr<Segment>> all_segments() const {          // of every shard, shard by shard in key order
        std::vector<std::shared_ptr<Segment>> v;
        for (auto &s : shard_list()) {
            const auto snap = s.second->snapshot();
            v.insert(v.end(), snap.begin(), snap.end());
        }
        return v;
    }
    Shard *find_shard(uint32_t key) const {
        std::lock_guard<std::mutex> g(mu_);
        auto it = shards_.find(key);
        return it == shards_.end() ? nullptr : it->second.get();
    }
    Shard &shard(uint32_t key) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = shards_.find(key);
        if (it == shards_.end()) {                 // inverted_index.go:163-190 newShard: mkdir <basedir>/<key>
            std::string dir;
            if (!basedir_.empty()) {
                char name[8];
                std::snprintf(name, sizeof name, "%04u", key);
                dir = (file::fs::path(basedir_) / name).string();
                std::error_code ec;
                if (!file::fs::create_directory(dir, ec) && ec) throw Error("new shard: " + dir + ": " + ec.message());
            }
            it = shards_.emplace(key, std::make_unique<Shard>(ctx_, dir)).first;
            it->second->SetBuild(build_mode_);
        }
        return *it->second;
    }
    ii2_ctx *ctx_;
    std::atomic<int> resolve_mode_{-1};                    // SetResolve
    std::atomic<uint64_t> first_cap_{FIRST_CAP};           // SetFirstCap
    mutable std::atomic<uint64_t> second_calls_{0};        // two_call's retries
    int build_mode_ = -1;                                  // SetBuild (guarded by mu_)
    std::string basedir_;
    mutable std::mutex mu_;                                // guards shards_ (the map, not the shards) and workers_
    std::vector<ii2_ctx *> workers_;                       // contexts of Merge's workers 1..n-1 (created on demand)
    std::map<uint32_t, std::unique_ptr<Shard>> shards_;    // sorted by key, like ii.shards
};

}  // namespace ii2h

// ---- C facade for the Python tests ----------------------------------------------------------
using namespace ii2h;

struct ii2h_target {
    std::shared_ptr<Shard> shard;          // shared by every session attached to the same shard / index:
    std::shared_ptr<InvertedIndex> index;  // the error text and the last results below are per session
    std::string err;
    std::vector<TermValues> result;     // last Read / PrefixSearch result
    std::vector<uint32_t> ids;          // last Intersect / RemovedValues result
    std::vector<uint32_t> scores;       // last IntersectTop result: the score of each of ids
    std::vector<std::pair<Term, uint64_t>> counts;      // last TermCounts result
    std::vector<uint64_t> hist;                         // last Histogram result
    std::vector<std::pair<Term, std::vector<uint64_t>>> term_hist;      // last TermHistogram result
    std::vector<uint64_t> masks;        // last MatchedTerms / MatchedTermsBatch result (the pages' rows back to back)
};

static std::vector<Term> unpack_terms(const uint8_t *bytes, const uint64_t *off, uint64_t n) {
    std::vector<Term> t(n);
    for (uint64_t i = 0; i < n; i++) t[i].assign((const char *)bytes + off[i], off[i + 1] - off[i]);
    return t;
}

// (id, score) pairs into ids / scores, after what these hold
static void split_pairs(const std::vector<std::pair<uint32_t, uint32_t>> &top, std::vector<uint32_t> &ids, std::vector<uint32_t> &scores) {
    for (auto &p : top) { ids.push_back(p.first); scores.push_back(p.second); }
}
// The queries of a bulk call: n_q queries over the terms (bytes, off), query q owns terms q_first[q] .. q_first[q + 1] - 1, the first
// q_req[q] of them required, the others excluded.  fn(q, a, m, e) per query, in order: its required terms are [a, m), its excluded ones [m, e).
template <class Fn> static void split_queries(const uint8_t *bytes, const uint64_t *off, const uint64_t *q_first, const uint64_t *q_req, uint64_t n_q, Fn fn) {
    const std::vector<Term> terms = unpack_terms(bytes, off, n_q ? q_first[n_q] : 0);
    for (uint64_t q = 0; q < n_q; q++) {
        const uint64_t a = q_first[q], m = std::min(a + q_req[q], q_first[q + 1]);
        fn(q, terms.begin() + a, terms.begin() + m, terms.begin() + q_first[q + 1]);
    }
}

#define H_TRY(t, ...)                                   \
    try { __VA_ARGS__; return 0; }                      \
    catch (const std::exception &e) { (t)->err = e.what(); return -1; }

extern "C" {

ii2h_target *ii2h_create(ii2_ctx *ctx, int is_index) {
    auto *t = new ii2h_target();
    if (is_index) t->index = std::make_shared<InvertedIndex>(ctx);
    else t->shard = std::make_shared<Shard>(ctx);
    return t;
}
// another handle on the same Shard / InvertedIndex with its own result and error slots: one per calling thread
// (the operations themselves are thread-safe like the reference's; a handle's result buffers are not shared state)
ii2h_target *ii2h_attach(const ii2h_target *owner) {
    auto *t = new ii2h_target();
    t->shard = owner->shard;
    t->index = owner->index;
    return t;
}
// NewShard(basedir) / NewInvertedIndex(basedir): loads what the directory holds.  NULL + message in err[] on failure.
ii2h_target *ii2h_open(ii2_ctx *ctx, int is_index, const char *basedir, char *err, uint64_t err_cap) {
    auto t = std::make_unique<ii2h_target>();
    try {
        if (is_index) t->index = std::make_shared<InvertedIndex>(ctx, basedir);
        else t->shard = std::make_shared<Shard>(ctx, basedir);
    } catch (const std::exception &e) {
        if (err && err_cap) { std::strncpy(err, e.what(), err_cap - 1); err[err_cap - 1] = 0; }
        return nullptr;
    }
    return t.release();
}
// file.NewWriter / NewDirectWriter + Append* + Close in one call; key_out receives GetKey() (NUL-terminated, <= 31 chars)
int ii2h_file_write(ii2h_target *t, ii2_ctx *ctx, const char *dir, int direct, const uint8_t *term_bytes, const uint64_t *term_off, uint64_t n_terms,
                    const uint64_t *post_off, const uint32_t *values, char *key_out) {
    H_TRY(t, {
        Writer w(ctx, dir, direct != 0);
        auto terms = unpack_terms(term_bytes, term_off, n_terms);
        for (uint64_t i = 0; i < n_terms; i++)
            w.Append(TermValues{terms[i], std::vector<uint32_t>(values + post_off[i], values + post_off[i + 1])});
        w.Close();
        std::strncpy(key_out, w.GetKey().c_str(), 31);
        key_out[31] = 0;
    })
}
// file.NewReader(dir, key, min, max) drained with Next() into the target's result; *n_terms = 0 and rc 1 when the
// segment has nothing in range (vellum.ErrIteratorDone)
int ii2h_file_read(ii2h_target *t, ii2_ctx *ctx, const char *dir, const char *key, const uint8_t *mn, uint64_t mnl, int has_min,
                   const uint8_t *mx, uint64_t mxl, int has_max, uint64_t *n_terms) {
    try {
        Term a((const char *)mn, has_min ? mnl : 0), b((const char *)mx, has_max ? mxl : 0);
        t->result.clear();
        *n_terms = 0;
        Reader r(ctx, dir, key, has_min ? &a : nullptr, has_max ? &b : nullptr);
        TermValues tv;
        while (r.Next(&tv)) t->result.push_back(tv);
        r.Close();
        *n_terms = t->result.size();
        return 0;
    } catch (const Reader::NothingInRange &) {
        return 1;
    } catch (const std::exception &e) {
        t->err = e.what();
        return -1;
    }
}
int ii2h_remove_segment(ii2h_target *t, const char *dir, const char *key) {
    H_TRY(t, { file::remove_segment(dir, key); })
}
// the term dictionary file alone (no device involved): terms into the target's result, a direct segment's value as each
// term's one-element list; *direct = the file's mode
int ii2h_terms_read(ii2h_target *t, const char *dir, const char *key, int *direct, uint64_t *n_terms) {
    H_TRY(t, {
        file::TermFile tf = file::read_terms(dir, key);
        t->result.clear();
        for (size_t i = 0; i < tf.terms.size(); i++)
            t->result.push_back(TermValues{tf.terms[i], tf.direct ? std::vector<uint32_t>{tf.direct_vals[i]} : std::vector<uint32_t>{}});
        *direct = tf.direct ? 1 : 0;
        *n_terms = t->result.size();
    })
}
// removed.list alone: write batches (timestamp i, values vals[off[i] .. off[i+1])); read them back as RemovedLists.Values()
int ii2h_removed_write(ii2h_target *t, const char *dir, uint64_t n, const int64_t *ts, const uint64_t *off, const uint32_t *vals) {
    H_TRY(t, {
        file::RemovedBatches b;
        for (uint64_t i = 0; i < n; i++) b[ts[i]] = std::vector<uint32_t>(vals + off[i], vals + off[i + 1]);
        file::write_removed(dir, b);
    })
}
int ii2h_removed_read(ii2h_target *t, const char *dir, uint64_t *n_batches, uint64_t *n_ids) {
    H_TRY(t, {
        file::RemovedBatches b;
        t->ids.clear();
        *n_batches = 0;
        if (file::read_removed(dir, &b)) {
            *n_batches = b.size();
            for (auto &kv : b) t->ids.insert(t->ids.end(), kv.second.begin(), kv.second.end());
            std::sort(t->ids.begin(), t->ids.end());
        }
        *n_ids = t->ids.size();
    })
}
void ii2h_destroy(ii2h_target *t) { delete t; }
const char *ii2h_last_error(const ii2h_target *t) { return t->err.c_str(); }

int ii2h_put(ii2h_target *t, const uint8_t *bytes, const uint64_t *off, uint64_t n, uint32_t val) {
    H_TRY(t, { auto terms = unpack_terms(bytes, off, n); if (t->index) t->index->Put(terms, val); else t->shard->Put(terms, val); })
}
// n_docs docs, flat: doc d owns the terms doc_first[d] .. doc_first[d + 1] - 1 of (bytes, off) and the value vals[d]
int ii2h_put_batch(ii2h_target *t, const uint8_t *bytes, const uint64_t *off, const uint64_t *doc_first, const uint32_t *vals, uint64_t n_docs) {
    H_TRY(t, {
        const std::vector<Term> terms = unpack_terms(bytes, off, n_docs ? doc_first[n_docs] : 0);
        std::vector<std::pair<std::vector<Term>, uint32_t>> docs(n_docs);
        for (uint64_t d = 0; d < n_docs; d++) {
            docs[d].first.assign(terms.begin() + doc_first[d], terms.begin() + doc_first[d + 1]);
            docs[d].second = vals[d];
        }
        if (t->index) t->index->PutBatch(docs); else t->shard->PutBatch(docs);
    })
}
int ii2h_remove(ii2h_target *t, const uint32_t *vals, uint64_t n) {
    H_TRY(t, { std::vector<uint32_t> v(vals, vals + n); if (t->index) t->index->PutRemoved(v); else t->shard->Remove(v); })
}
int ii2h_merge(ii2h_target *t, int req, int m, int concurrency, int64_t *merged) {
    H_TRY(t, { *merged = t->index ? t->index->Merge(req, m, concurrency) : t->shard->Merge(req, m); })
}
// min/max: NULL pointer = nil
int ii2h_read(ii2h_target *t, const uint8_t *mn, uint64_t mnl, int has_min, const uint8_t *mx, uint64_t mxl, int has_max, uint64_t *n_terms) {
    H_TRY(t, {
        Term a((const char *)mn, has_min ? mnl : 0), b((const char *)mx, has_max ? mxl : 0);
        t->result = t->index ? t->index->Read(has_min ? &a : nullptr, has_max ? &b : nullptr)
                             : t->shard->Read(has_min ? &a : nullptr, has_max ? &b : nullptr);
        *n_terms = t->result.size();
    })
}
int ii2h_prefix_search(ii2h_target *t, const uint8_t *bytes, const uint64_t *off, uint64_t n, uint64_t *n_found) {
    H_TRY(t, {
        t->result.clear();
        for (auto &kv : t->index->PrefixSearch(unpack_terms(bytes, off, n))) t->result.push_back(TermValues{kv.first, kv.second});
        *n_found = t->result.size();
    })
}
// map<pattern, ids> of the patterns (packed like terms) into the result slots, one per pattern that matched, in pattern order
int ii2h_match_search(ii2h_target *t, const uint8_t *bytes, const uint64_t *off, uint64_t n, uint32_t kind, uint64_t *n_found) {
    H_TRY(t, {
        t->result.clear();
        const std::vector<Term> patterns = unpack_terms(bytes, off, n);
        for (auto &kv : t->index ? t->index->MatchSearch(patterns, kind) : t->shard->MatchSearch(patterns, kind))
            t->result.push_back(TermValues{kv.first, kv.second});
        *n_found = t->result.size();
    });
}
// the distinct terms one pattern matches, at most `limit`, into the result slots (terms only)
int ii2h_match_terms(ii2h_target *t, const uint8_t *pattern, uint64_t pattern_len, uint32_t kind, uint64_t limit, uint64_t *n_found) {
    H_TRY(t, {
        t->result.clear();
        const Term p((const char *)pattern, pattern_len);
        for (auto &term : t->index ? t->index->MatchTerms(p, kind, limit) : t->shard->MatchTerms(p, kind, limit)) t->result.push_back(TermValues{term, {}});
        *n_found = t->result.size();
    });
}
// map<query term, ids> of the query terms (packed like terms) into the result slots, one per term that matched, in term order
int ii2h_fuzzy_search(ii2h_target *t, const uint8_t *bytes, const uint64_t *off, uint64_t n, uint32_t max_dist, uint32_t prefix, uint32_t flags,
                      uint64_t *n_found) {
    H_TRY(t, {
        t->result.clear();
        const std::vector<Term> terms = unpack_terms(bytes, off, n);
        for (auto &kv : t->index ? t->index->FuzzySearch(terms, max_dist, prefix, flags) : t->shard->FuzzySearch(terms, max_dist, prefix, flags))
            t->result.push_back(TermValues{kv.first, kv.second});
        *n_found = t->result.size();
    });
}
// the distinct terms within distance of one pattern, at most `limit`, into the result slots: a term's single value is its distance
int ii2h_fuzzy_terms(ii2h_target *t, const uint8_t *pattern, uint64_t pattern_len, uint32_t max_dist, uint32_t prefix, uint32_t flags, uint64_t limit,
                     uint64_t *n_found) {
    H_TRY(t, {
        t->result.clear();
        const Term p((const char *)pattern, pattern_len);
        for (auto &td : t->index ? t->index->FuzzyTerms(p, max_dist, prefix, flags, limit) : t->shard->FuzzyTerms(p, max_dist, prefix, flags, limit))
            t->result.push_back(TermValues{td.first, {td.second}});
        *n_found = t->result.size();
    });
}
// map<pattern, ids> of the regular expressions (packed like terms) into the result slots, one per pattern that matched, in pattern order
int ii2h_regex_search(ii2h_target *t, const uint8_t *bytes, const uint64_t *off, uint64_t n, uint32_t flags, uint64_t *n_found) {
    H_TRY(t, {
        t->result.clear();
        const std::vector<Term> patterns = unpack_terms(bytes, off, n);
        for (auto &kv : t->index ? t->index->RegexSearch(patterns, flags) : t->shard->RegexSearch(patterns, flags))
            t->result.push_back(TermValues{kv.first, kv.second});
        *n_found = t->result.size();
    });
}
// the distinct terms one regular expression matches, at most `limit`, into the result slots (terms only)
int ii2h_regex_terms(ii2h_target *t, const uint8_t *pattern, uint64_t pattern_len, uint32_t flags, uint64_t limit, uint64_t *n_found) {
    H_TRY(t, {
        t->result.clear();
        const Term p((const char *)pattern, pattern_len);
        for (auto &term : t->index ? t->index->RegexTerms(p, flags, limit) : t->shard->RegexTerms(p, flags, limit)) t->result.push_back(TermValues{term, {}});
        *n_found = t->result.size();
    });
}
int ii2h_intersect(ii2h_target *t, const uint8_t *bytes, const uint64_t *off, uint64_t n, uint64_t *n_ids) {
    H_TRY(t, { t->ids = t->index->Intersect(unpack_terms(bytes, off, n)); *n_ids = t->ids.size(); })
}
int ii2h_intersect_at_least(ii2h_target *t, const uint8_t *bytes, const uint64_t *off, uint64_t n, uint32_t min_match, const uint8_t *x_bytes,
                            const uint64_t *x_off, uint64_t n_x, uint64_t *n_ids) {
    H_TRY(t, { t->ids = t->index->IntersectAtLeast(unpack_terms(bytes, off, n), min_match, unpack_terms(x_bytes, x_off, n_x)); *n_ids = t->ids.size(); })
}
int ii2h_intersect_top(ii2h_target *t, const uint8_t *bytes, const uint64_t *off, uint64_t n, uint64_t k, uint32_t min_match, const uint8_t *x_bytes,
                       const uint64_t *x_off, uint64_t n_x, uint64_t *n_ids) {
    H_TRY(t, {
        t->ids.clear();
        t->scores.clear();
        split_pairs(t->index->IntersectTop(unpack_terms(bytes, off, n), k, min_match, unpack_terms(x_bytes, x_off, n_x)), t->ids, t->scores);
        *n_ids = t->ids.size();
    })
}
int ii2h_intersect_top_weighted(ii2h_target *t, const uint8_t *bytes, const uint64_t *off, uint64_t n, const uint32_t *weights, uint64_t k,
                                uint32_t min_score, const uint8_t *x_bytes, const uint64_t *x_off, uint64_t n_x, uint64_t *n_ids) {
    H_TRY(t, {
        t->ids.clear();
        t->scores.clear();
        split_pairs(t->index->IntersectTopWeighted(unpack_terms(bytes, off, n), std::vector<uint32_t>(weights, weights + n), k, min_score,
                                                   unpack_terms(x_bytes, x_off, n_x)), t->ids, t->scores);
        *n_ids = t->ids.size();
    })
}
// which of the n terms each of the n_ids ids lies under: n_ids rows of *n_words words (bit j of a row: term j), fetched by ii2h_masks_copy
int ii2h_matched_terms(ii2h_target *t, const uint32_t *ids, uint64_t n_ids, const uint8_t *bytes, const uint64_t *off, uint64_t n, uint64_t *n_words) {
    H_TRY(t, {
        t->masks = t->index->MatchedTerms(std::vector<uint32_t>(ids, ids + n_ids), unpack_terms(bytes, off, n));
        *n_words = (n + 63) / 64;
    })
}
void ii2h_masks_copy(const ii2h_target *t, uint64_t *out) {
    if (!t->masks.empty()) std::memcpy(out, t->masks.data(), t->masks.size() * 8);
}
// the same for n_pages pages in one device call: page p holds the ids ids[ids_off[p] .. ids_off[p + 1]) and the terms term_first[p] ..
// term_first[p + 1] - 1 of (bytes, off).  words_off[p] (n_pages + 1 entries): where page p's rows - ids x ceil(terms / 64) words -
// start in the target's masks, fetched by ii2h_masks_batch_copy
int ii2h_matched_terms_batch(ii2h_target *t, const uint32_t *ids, const uint64_t *ids_off, const uint8_t *bytes, const uint64_t *off,
                             const uint64_t *term_first, uint64_t n_pages, uint64_t *words_off) {
    H_TRY(t, {
        std::vector<InvertedIndex::TermsPage> pages(n_pages);
        for (uint64_t p = 0; p < n_pages; p++) {
            pages[p].ids.assign(ids + ids_off[p], ids + ids_off[p + 1]);
            pages[p].terms = unpack_terms(bytes, off + term_first[p], term_first[p + 1] - term_first[p]);
        }
        t->masks.clear();
        words_off[0] = 0;
        uint64_t p = 0;
        for (auto &rows : t->index->MatchedTermsBatch(pages)) {
            t->masks.insert(t->masks.end(), rows.begin(), rows.end());
            words_off[++p] = t->masks.size();
        }
    })
}
void ii2h_masks_batch_copy(const ii2h_target *t, uint64_t *out) { ii2h_masks_copy(t, out); }
int ii2h_intersect_except(ii2h_target *t, const uint8_t *bytes, const uint64_t *off, uint64_t n, const uint8_t *x_bytes, const uint64_t *x_off,
                          uint64_t n_x, uint64_t *n_ids) {
    H_TRY(t, { t->ids = t->index->IntersectExcept(unpack_terms(bytes, off, n), unpack_terms(x_bytes, x_off, n_x)); *n_ids = t->ids.size(); })
}
int ii2h_set_resolve(ii2h_target *t, int mode) {
    H_TRY(t, {
        if (!t->index) throw Error("set resolve: not an index");
        t->index->SetResolve(mode);
    });
}
int ii2h_set_build(ii2h_target *t, int mode) {
    H_TRY(t, { if (t->index) t->index->SetBuild(mode); else t->shard->SetBuild(mode); });
}
// tests: the first buffer of the calls that may need a second one, and how many second calls there were (InvertedIndex::SetFirstCap)
int ii2h_set_first_cap(ii2h_target *t, uint64_t ids) {
    H_TRY(t, {
        if (!t->index) throw Error("set first cap: not an index");
        t->index->SetFirstCap(ids);
    });
}
uint64_t ii2h_second_calls(const ii2h_target *t) { return t->index ? t->index->SecondCalls() : 0; }
// tests, no device: the output bound or_per_name gives one name (union_bound) whose range i lies in segment range_seg[i], segment
// s holding postings[s] postings
uint64_t ii2h_union_bound(const uint64_t *range_seg, uint64_t n_ranges, const uint64_t *postings) {
    return union_bound(std::vector<uint64_t>(range_seg, range_seg + n_ranges), [&](uint64_t s) { return postings[s]; });
}
// n_q queries laid out as split_queries takes them.  Result q: the values of the target's result q (its term is empty)
int ii2h_intersect_batch(ii2h_target *t, const uint8_t *bytes, const uint64_t *off, const uint64_t *q_first, const uint64_t *q_req, uint64_t n_q,
                         uint64_t *n_results) {
    H_TRY(t, {
        std::vector<std::pair<std::vector<Term>, std::vector<Term>>> queries(n_q);
        split_queries(bytes, off, q_first, q_req, n_q, [&](uint64_t q, auto a, auto m, auto e) {
            queries[q].first.assign(a, m);
            queries[q].second.assign(m, e);
        });
        t->result.clear();
        for (auto &ids : t->index->IntersectMany(queries)) t->result.push_back(TermValues{Term(), std::move(ids)});
        *n_results = t->result.size();
    })
}
// n_q ranked queries over the terms (bytes, off), owned and split as ii2h_intersect_batch's; weights: one per REQUIRED term, query after
// query; k and min_score: one per query.  Result q: the ids in the values of the target's result q (its term is empty), the scores of
// all results back to back in the target's scores
int ii2h_intersect_top_batch(ii2h_target *t, const uint8_t *bytes, const uint64_t *off, const uint64_t *q_first, const uint64_t *q_req,
                             const uint32_t *weights, const uint64_t *k, const uint32_t *min_score, uint64_t n_q, uint64_t *n_results) {
    H_TRY(t, {
        std::vector<InvertedIndex::TopQuery> queries(n_q);
        uint64_t w0 = 0;                                         // (one weight per required term, query after query)
        split_queries(bytes, off, q_first, q_req, n_q, [&](uint64_t q, auto a, auto m, auto e) {
            queries[q].terms.assign(a, m);
            queries[q].except.assign(m, e);
            queries[q].weights.assign(weights + w0, weights + w0 + (m - a));
            w0 += m - a;
            queries[q].k = k[q];
            queries[q].min_score = min_score[q];
        });
        t->result.clear();
        t->scores.clear();
        for (auto &top : t->index->IntersectTopBatch(queries)) {
            t->result.push_back(TermValues{Term(), {}});
            split_pairs(top, t->result.back().values, t->scores);
        }
        *n_results = t->result.size();
    })
}
int ii2h_term_counts(ii2h_target *t, const uint8_t *prefix, uint64_t prefix_len, const uint8_t *bytes, const uint64_t *off, uint64_t n,
                     const uint8_t *x_bytes, const uint64_t *x_off, uint64_t n_x, uint64_t *n_found) {
    H_TRY(t, {
        auto m = t->index->TermCounts(Term((const char *)prefix, prefix_len), unpack_terms(bytes, off, n), unpack_terms(x_bytes, x_off, n_x));
        t->counts.assign(m.begin(), m.end());
        *n_found = t->counts.size();
    })
}
uint64_t ii2h_count_term_len(const ii2h_target *t, uint64_t i) { return t->counts[i].first.size(); }
void ii2h_count_copy(const ii2h_target *t, uint64_t i, uint8_t *term, uint64_t *count) {
    std::memcpy(term, t->counts[i].first.data(), t->counts[i].first.size());
    *count = t->counts[i].second;
}
int ii2h_histogram(ii2h_target *t, const uint8_t *bytes, const uint64_t *off, uint64_t n, const uint8_t *x_bytes, const uint64_t *x_off, uint64_t n_x,
                   const uint64_t *edges, uint64_t n_edges, uint64_t *n_buckets) {
    H_TRY(t, {
        t->hist = t->index->Histogram(unpack_terms(bytes, off, n), unpack_terms(x_bytes, x_off, n_x), std::vector<uint64_t>(edges, edges + n_edges));
        *n_buckets = t->hist.size();
    })
}
void ii2h_hist_copy(const ii2h_target *t, uint64_t *counts) {
    if (!t->hist.empty()) std::memcpy(counts, t->hist.data(), t->hist.size() * sizeof(uint64_t));
}
int ii2h_term_histogram(ii2h_target *t, const uint8_t *prefix, uint64_t prefix_len, const uint8_t *bytes, const uint64_t *off, uint64_t n,
                        const uint8_t *x_bytes, const uint64_t *x_off, uint64_t n_x, const uint64_t *edges, uint64_t n_edges, uint64_t *n_found) {
    H_TRY(t, {
        auto m = t->index->TermHistogram(Term((const char *)prefix, prefix_len), unpack_terms(bytes, off, n), unpack_terms(x_bytes, x_off, n_x),
                                         std::vector<uint64_t>(edges, edges + n_edges));
        t->term_hist.assign(m.begin(), m.end());
        *n_found = t->term_hist.size();
    })
}
uint64_t ii2h_term_hist_term_len(const ii2h_target *t, uint64_t i) { return t->term_hist[i].first.size(); }
void ii2h_term_hist_copy(const ii2h_target *t, uint64_t i, uint8_t *term, uint64_t *counts) {
    std::memcpy(term, t->term_hist[i].first.data(), t->term_hist[i].first.size());
    std::memcpy(counts, t->term_hist[i].second.data(), t->term_hist[i].second.size() * sizeof(uint64_t));
}
int ii2h_removed_values(ii2h_target *t, uint64_t *n_ids) {
    H_TRY(t, { Shard *s = t->shard ? t->shard.get() : t->index->OnlyShard(); t->ids = s ? s->RemovedValues() : std::vector<uint32_t>(); *n_ids = t->ids.size(); })
}
uint64_t ii2h_result_term_len(const ii2h_target *t, uint64_t i) { return t->result[i].term.size(); }
uint64_t ii2h_result_values_len(const ii2h_target *t, uint64_t i) { return t->result[i].values.size(); }
void ii2h_result_copy(const ii2h_target *t, uint64_t i, uint8_t *term, uint32_t *values) {
    std::memcpy(term, t->result[i].term.data(), t->result[i].term.size());
    if (!t->result[i].values.empty()) std::memcpy(values, t->result[i].values.data(), t->result[i].values.size() * 4);
}
void ii2h_ids_copy(const ii2h_target *t, uint32_t *out) {
    if (!t->ids.empty()) std::memcpy(out, t->ids.data(), t->ids.size() * 4);
}
void ii2h_scores_copy(const ii2h_target *t, uint32_t *out) {
    if (!t->scores.empty()) std::memcpy(out, t->scores.data(), t->scores.size() * 4);
}
uint64_t ii2h_segment_count(const ii2h_target *t) { return t->shard ? t->shard->SegmentCount() : 0; }
uint64_t ii2h_index_segment_count(const ii2h_target *t) { return t->index ? t->index->SegmentCount() : 0; }      // the segments of all its shards
uint64_t ii2h_shard_count(const ii2h_target *t) { return t->index ? t->index->ShardCount() : 1; }

}  // extern "C"
