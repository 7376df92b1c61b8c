/*
 * ii2.h — C ABI of the MI355X posting-list engine (libii2_hip.so).
 *
 * Drop-in boundary for the posting-list hot path of lezhnev74/inverted_index_2.  The
 * reference is a plain Go library with no FFI seam (SURVEY.md §8 b), so the boundary is
 * drawn *beneath* its exported Go API: the Go methods keep their signatures and bind
 * these entry points through cgo (stub in INTEGRATION.md).  Each entry point names the
 * reference code it replaces (file:line into the reference tree).
 *
 * Conventions
 *   - every call returns 0 on success or a negative II2_E* code; ii2_last_error(ctx)
 *     gives the message (the Go side wraps it with fmt.Errorf("…: %w"), cf. shard.go:160).
 *   - plain pointers and sizes only.  `where` says whether a caller buffer lives in host
 *     memory (II2_HOST — what cgo passes) or in this device's HBM (II2_DEVICE).
 *   - inputs are read-only and never retained after return; outputs are written only on
 *     success (all-or-nothing per call).  One exception, stated where it applies: an intersect /
 *     union whose result does not fit `cap` returns II2_ECAPACITY with the buffer's content
 *     unspecified (the merge entry points write nothing in that case).
 *   - per-call limits (II2_ERANGE beyond them): a merge takes < 2^32 input postings, < 2^31 input
 *     blocks and < 2^30 term slots; ii2_align_terms takes < 2^31 terms; one segment holds < 2^31
 *     lists, < 2^31 blocks and < 4 GiB of payload (split larger inputs into several segments / calls);
 *     ii2_seg_build takes < 2^32 pairs for < 2^31 lists (the encoder's limits on the segment it makes apply unchanged);
 *     ii2_dict_build takes < 2^31 terms of at most II2_DICT_BUILD_MAX_TERM = 256 bytes each (longer terms: sort on the host, ii2_dict_create);
 *     ii2_query_batch takes <= 2^20 queries whose result bounds (AND: the shortest operand, OR: the postings of
 *     its ranges) add up to < 2^32 ids; ii2_query_batch_groups takes <= 2^20 queries whose result bounds (the postings of each query's
 *     smallest required group) add up to < 2^32 ids, a query of at most II2_MAX_LISTS non-empty lists - required and excluded -
 *     that hold at most 8192 postings in at most 128 blocks shares the batch's launch (larger ones run one by one: no error).
 *     The one-launch form of ii2_andnot_ranges takes queries whose non-empty lists - required
 *     and excluded - are at most II2_MAX_LISTS and hold at most 8192 postings in at most 128 blocks, by default only while
 *     postings x lists <= 32768 (what the form costs; beyond it, or beyond the kernel, a query takes the general form: no error).
 *     ii2_topk_ranges takes at most 255 required groups that have postings and k <= II2_TOPK_MAX = 2^20.
 *     ii2_topk_weighted_ranges takes group weights 1 .. 255 whose sum over those groups is at most 255.
 *     ii2_topk_batch takes <= 2^20 such queries whose result bounds (min(k, the postings of the query's required groups)) add up
 *     to < 2^32 ids; a query of at most II2_MAX_LISTS counted lists that hold at most 8192 postings in at most 128 blocks shares
 *     the batch's launch (larger ones run one by one: no error).
 *   - a ctx is bound to one GPU and one HIP stream; calls on one ctx are serialised by an
 *     internal mutex, so a ctx may be shared by goroutines / threads (InvertedIndex.Merge
 *     fans Shard.Merge over `concurrency` goroutines, inverted_index.go:83-103); use one
 *     ctx per worker to overlap.
 *   - segments and tombstone bitmaps belong to a DEVICE, not to the ctx that made them: they
 *     are read-only once created and any ctx of that device may use them, from any thread,
 *     concurrently (the reference's readers share segments, segments.go:32-46).  The caller
 *     must not free one while a call that reads it is still running.
 *   - doc ids ("values") are uint32 everywhere, as in the reference (file/types.go:11).
 *   - there is NO CPU fallback: without a usable gfx950 device ii2_ctx_create fails.
 */
#ifndef II2_H
#define II2_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define II2_ABI_VERSION 1

enum { II2_HOST = 0, II2_DEVICE = 1 };

enum {
    II2_OK = 0,
    II2_EINVAL = -1,     /* bad argument (NULL, unsorted sizes, too many lists …) */
    II2_ENOMEM = -2,     /* device or host allocation failed */
    II2_EHIP = -3,       /* a HIP runtime call failed (message has the HIP error string) */
    II2_ECAPACITY = -4,  /* caller's output buffer is too small (merge: nothing written; intersect / union: content unspecified) */
    II2_ERANGE = -5,     /* beyond a per-call or per-segment limit (see the conventions above) */
    II2_ECOMM = -6,      /* RCCL failure / communicator not initialised */
    II2_ENODEVICE = -7   /* no usable gfx950 GPU — the library has no CPU path */
};

#define II2_MAX_LISTS 64u   /* lists per intersect / union call, segments per merge */
#define II2_DV1_BLOCK 256u  /* postings per DV1 block */

typedef struct ii2_ctx ii2_ctx;
typedef struct ii2_seg ii2_seg;    /* device-resident DV1 segment: n_lists posting lists */
typedef struct ii2_tomb ii2_tomb;  /* device-resident tombstone bitmap */

/* One entry per DV1 block (+ one sentinel): first doc id of the block and the byte offset
 * of its payload (the varint gaps of the block's remaining postings). */
typedef struct { uint32_t first_doc; uint32_t byte_off; } ii2_skip;

typedef struct {
    uint64_t n_lists;      /* aligned term slots */
    uint64_t n_postings;
    uint64_t n_blocks;
    uint64_t n_bytes;      /* payload bytes */
} ii2_seg_info;

typedef struct {
    uint64_t n_in;         /* postings read (sum of input list lengths) */
    uint64_t n_out;        /* postings written */
    uint64_t n_terms_out;  /* terms with >= 1 surviving posting (0 => write no segment, shard.go:219-225) */
    uint64_t n_tiles;      /* workgroup tiles the merge was cut into */
} ii2_merge_stats;

/* ---- context -------------------------------------------------------------------------- */
int ii2_abi_version(void);
/* Binds a context to GPU `device` (hipSetDevice ordinal).  Fails with II2_ENODEVICE when
 * there is no gfx950 device. */
int ii2_ctx_create(int device, uint32_t flags, ii2_ctx **out);
void ii2_ctx_destroy(ii2_ctx *ctx);
const char *ii2_last_error(const ii2_ctx *ctx);     /* ctx may be NULL: last create error */
int ii2_ctx_sync(ii2_ctx *ctx);                     /* waits for the ctx stream; fails once when an ii2_intersect_async
                                                     * since the previous sync gave up (see ii2_ctx_counters) */
void *ii2_ctx_stream(ii2_ctx *ctx);                 /* the hipStream_t, for event timing */
int ii2_ctx_device(const ii2_ctx *ctx);             /* the device ordinal the context is bound to (-1 for NULL) */

/* raw device buffers for II2_DEVICE arguments */
int ii2_dev_alloc(ii2_ctx *ctx, size_t bytes, void **dptr);
int ii2_dev_free(ii2_ctx *ctx, void *dptr);
int ii2_copy_h2d(ii2_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int ii2_copy_d2h(ii2_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);

/* ---- segments: the encode / decode steps ----------------------------------------------- */
/* Encode step.  Replaces Writer.Append -> intcomp.CompressUint32 (file/writer.go:32-59):
 * builds a device-resident DV1 segment from n_lists lists given CSR-style
 * (post_off[n_lists+1] into values).  Lists are stored verbatim (any u32 sequence
 * round-trips, cf. file/writer_test.go:14), but merge / intersect / union require each
 * list ascending and duplicate-free — what the index itself always produces. */
int ii2_seg_encode(ii2_ctx *ctx, uint64_t n_lists, const uint64_t *post_off, const uint32_t *values,
                   int where, ii2_seg **out);
/* Build step (bulk Put).  Replaces N calls of Shard.Put (shard.go:33-67), each of which writes its own direct segment, followed
 * by the merges that fold those segments (shard.go:163-212): ONE segment from n_pairs (list, value) pairs in any order, repeats
 * allowed.  *out is the DV1 segment of n_lists lists in which list t holds, ascending and duplicate-free, every v for which
 * (t, v) occurs among the pairs - bit for bit what ii2_seg_encode returns for the same lists given in CSR form, and a segment
 * like any other (merge, union, select, export, ii2_seg_allgather).  No tombstone filter: a Put applies none.
 * list_id[n_pairs] and values[n_pairs] both live where `where` says.  n_pairs == 0: the segment of n_lists empty lists (the arrays
 * may be NULL); n_lists == 0 with n_pairs > 0: II2_EINVAL.  A list_id >= n_lists is II2_EINVAL (found on the device while the
 * keys are formed; the message names the first such pair), *out stays NULL and nothing stays allocated.
 * On the device: a least-significant-digit radix sort of the keys list_id << 32 | value (8-bit digits, only the digits that can
 * differ: stats->n_passes = ceil((32 + bit_width(n_lists - 1)) / 8), 0 without pairs), a pass that drops equal neighbours, a
 * lookup of every list's offset, one readback and the two-pass encoder.  No workgroup of it waits for another (seg_build.hip). */
typedef struct {
    uint64_t n_pairs;      /* pairs read */
    uint64_t n_postings;   /* distinct (list, value) pairs = postings of the segment */
    uint64_t n_nonempty;   /* lists with >= 1 posting */
    uint32_t n_passes;     /* radix passes run */
} ii2_build_stats;
int ii2_seg_build(ii2_ctx *ctx, uint64_t n_lists, uint64_t n_pairs, const uint32_t *list_id,
                  const uint32_t *values, int where, ii2_seg **out, ii2_build_stats *stats /* may be NULL */);
/* Adopt an already DV1-encoded segment (blk_off[n_lists+1], skip[n_blocks+1], payload[n_bytes]).
 * The caller states the lengths of its arrays; blk_off[n_lists] must equal n_blocks and
 * skip[n_blocks].byte_off must equal n_bytes, else II2_EINVAL — the library never reads past the
 * stated lengths, whatever the arrays contain. */
int ii2_seg_import(ii2_ctx *ctx, uint64_t n_lists, uint64_t n_postings, uint64_t n_blocks, uint64_t n_bytes,
                   const uint32_t *blk_off, const ii2_skip *skip, const uint8_t *payload, int where, ii2_seg **out);
/* Decode step.  Replaces Reader.Next -> intcomp.UncompressUint32 (file/reader.go:79-100):
 * post_off[n_lists+1] and values[n_postings] are written to caller buffers. */
int ii2_seg_decode(ii2_ctx *ctx, const ii2_seg *seg, uint64_t *post_off, uint32_t *values, int where);
/* Copy the DV1 arrays out (any of the three may be NULL). */
int ii2_seg_export(ii2_ctx *ctx, const ii2_seg *seg, uint32_t *blk_off, ii2_skip *skip, uint8_t *payload);
/* A view of `src` with n_out term slots that shares src's skip table and payload: slot i holds list
 * src_list[i] of src, or is empty when src_list[i] < 0.  This is how the host aligns the term ids of
 * k segments before a merge (terms a segment lacks become empty slots) and drops emptied terms after
 * one.  Selected indices must ascend and may only skip empty lists between two selected ones. */
int ii2_seg_select(ii2_ctx *ctx, const ii2_seg *src, uint64_t n_out, const int64_t *src_list, ii2_seg **out);
/* ---- term alignment on the device -------------------------------------------------------- */
/* Replaces the k-way walk over the segments' term dictionaries that feeds the merging iterator
 * (shard.go:253-278, file/reader.go:33-71; order = file.CompareTermValues = bytes.Compare,
 * file/types.go:24-26).  Input, host memory: k sorted, duplicate-free dictionaries, flat —
 * term_bytes, term_off[n_all + 1] (byte offsets of the terms), seg_first[k + 1] (index in term_off
 * of each dictionary's first term; seg_first[0] = 0, seg_first[k] = n_all).  The result stays on
 * the device: the union dictionary (n_union terms, ascending) and, per dictionary, which of its
 * terms is which union term. */
typedef struct ii2_align ii2_align;
/* A segment's term dictionary resident in HBM (sorted, duplicate-free terms: term_off[n_terms + 1] byte offsets into
 * term_bytes, term_off[0] = 0; `where` says where the two arrays live).  Made once, when the segment is created or
 * loaded; alignments then read it in place.  II2_EINVAL, with nothing left allocated and *out NULL: term_off that does not
 * start at 0, descends or ends past the bytes, and terms that do not ascend strictly in bytes.Compare order - term i > 0 must
 * be greater than term i - 1 (an equal or a smaller neighbour is refused; checked on the device, next to the keys).  The
 * alignment ranks by bisection and relies on that order: ii2_align_terms makes its dictionaries by this call and refuses alike. */
typedef struct ii2_dict ii2_dict;
int ii2_dict_create(ii2_ctx *ctx, const uint8_t *term_bytes, const uint64_t *term_off, uint64_t n_terms, int where, ii2_dict **out);
void ii2_dict_free(ii2_dict *dict);
/* Term and prefix lookup in k resident dictionaries: the step in front of every range entry point, which take list indices where
 * callers have terms (replaces one dictionary bisection per (term, segment): the FST lookups of Intersect and PrefixSearch,
 * inverted_index.go:274-292; order = bytes.Compare, file/types.go:24-26).  Probe p is probe_bytes[probe_off[p] ..
 * probe_off[p + 1]); entry p * k + s of list_first / list_end answers it in dicts[s]:
 *   - exact probe (probe_prefix == NULL or probe_prefix[p] == 0): with j the index of the first term >= the probe, [j, j + 1)
 *     when term j is the probe and [j, j) - empty, at the insertion point - when it is not;
 *   - prefix probe (probe_prefix[p] == 1): [j, the first term at or after j that does not start with the probe) - the run
 *     PrefixSearch reads.  The empty prefix is the whole dictionary.
 * The k ranges of one probe are adjacent: they are one group of ii2_intersect_ranges / ii2_andnot_ranges / ii2_atleast_ranges /
 * the ranked calls / ii2_query_batch_groups / ii2_topk_batch with group_first[g] = g * k and the k segments repeated per group
 * (every range entry point takes empty ranges).  An empty dictionary gives [0, 0).
 * `where` says where probe_bytes, probe_off[n_probes + 1], probe_prefix[n_probes], list_first and list_end [n_probes * k each]
 * live, all five together.  *n_found (host, may be NULL) = the number of non-empty ranges.
 * All-or-nothing, every check before anything is launched: II2_EINVAL for a NULL array with n_probes > 0 (probe_prefix
 * excepted), k == 0 or k > II2_MAX_LISTS, a dictionary that is NULL or of another device, probe_off that does not start at 0 or
 * descends, a flag other than 0 / 1 (arrays on the device are checked there, in front of the lookup, which then writes nothing);
 * II2_ERANGE for n_probes * k >= 2^32.  n_probes == 0 writes nothing and sets *n_found = 0.
 * One wait per call.  Not a set operation: it takes no kernel path of ii2_ctx_paths.  One thread per (probe, dictionary), a
 * workgroup per 256 consecutive probes of one dictionary; the bisection compares 8-byte keys and goes to the bytes on ties
 * (dict_find.hip). */
int ii2_dict_find(ii2_ctx *ctx, uint32_t k, const ii2_dict *const *dicts, uint64_t n_probes, const uint8_t *probe_bytes,
                  const uint64_t *probe_off /* n_probes + 1 */, const uint8_t *probe_prefix /* n_probes; NULL: all exact */, int where,
                  uint64_t *list_first, uint64_t *list_end /* n_probes * k each */, uint64_t *n_found /* host, may be NULL */);
/* The lookup's arithmetic, host only (no GPU needed): one probe against one host dictionary (term_off[n_terms + 1] from 0, as
 * ii2_dict_create takes it) by the functions the kernel runs - the 8-byte keys, the comparison, the bisection, the prefix rule.  [*first, *end) as above.  II2_EINVAL: a NULL output, NULL term_off with n_terms > 0, NULL probe with probe_len > 0,
 * term_off not ascending from 0, prefix other than 0 / 1.  II2_ERANGE: 2^31 or more terms. */
int ii2_term_bounds(const uint8_t *term_bytes, const uint64_t *term_off, uint64_t n_terms, const uint8_t *probe, uint64_t probe_len,
                    int prefix, uint64_t *first, uint64_t *end);
/* Substring, suffix and wildcard term search in k resident dictionaries: the terms a pattern selects, as list ranges for the
 * range entry points - what neither ii2_dict_find nor the reference's FST can answer, because both walk a term from the front.
 * The dictionaries are scanned whole, at memory speed; all arrays are host memory.
 * Pattern p is pat_bytes[pat_off[p] .. pat_off[p + 1]) of kind pat_kind[p], one of II2_MATCH_CONTAINS / SUFFIX / GLOB, optionally
 * OR-ed with II2_MATCH_NOCASE (ASCII A-Z and a-z compare equal; no other byte folds) and / or II2_MATCH_UTF8 (below).  Without
 * II2_MATCH_UTF8 everything compares bytes:
 *   CONTAINS  the pattern is literal and matches a term that holds it anywhere; the empty pattern matches every term;
 *   SUFFIX    the pattern is literal and matches a term that ends with it; the empty pattern matches every term;
 *   GLOB      matches the WHOLE term: `*` any run of bytes (the empty one included), `?` exactly one byte, `\x` the byte x
 *             literally; no bracket classes; a lone `\` at the end is II2_EINVAL; the empty pattern matches only the empty term.
 * II2_MATCH_UTF8 reads the term as a sequence of SYMBOLS, left to right: where a well-formed UTF-8 sequence starts at byte i (RFC
 * 3629, Unicode table 3-7: no overlong form, no U+D800..DFFF, nothing above U+10FFFF, the whole sequence inside the term) it is
 * one symbol, its code point; otherwise byte i alone is one symbol, 0xDC00 + byte, and reading goes on at i + 1 - exactly Python's
 * bytes.decode("utf-8", "surrogateescape"), total on arbitrary bytes and injective.  The pattern must be well-formed UTF-8, else
 * II2_EINVAL: so an ill-formed byte of a term equals no pattern symbol.  Under the flag
 *   GLOB      matches the pattern against the term's symbols: `?` is exactly one symbol (one code point, or one ill-formed
 *             byte), `*` any run of whole symbols - it never ends inside a sequence, `*??` does not match a term of one 3-byte
 *             symbol -, `\x` the symbol x literally;
 *   CONTAINS, SUFFIX   accept the flag and answer as without it: a well-formed pattern starts with a non-continuation byte, so an
 *             occurrence of its bytes in a term always starts and ends on symbol boundaries of the term.  Only the pattern check
 *             is new.
 * II2_MATCH_NOCASE still folds ASCII A-Z only; the limit stays II2_MATCH_MAX_PATTERN bytes.  Flagged and unflagged patterns may be
 * mixed in one call.  A call without a flagged pattern launches the kernel it always did.
 * Pair (p, s) - pattern p in dicts[s] - is entry p * k + s, ii2_dict_find's layout.  Its answer is the maximal runs of
 * consecutive matching term indices, ascending: run j of the call is [run_first[j], run_end[j]) in dictionary run_dict[j], and
 * pair (p, s) owns the runs run_off[p * k + s] .. run_off[p * k + s + 1] - 1.  So pattern p is ONE group of the range entry
 * points: group_first[p] = run_off[p * k], segs[j] = the segment of dictionary run_dict[j], list_first / list_end = run_first /
 * run_end (plus first_list where a dictionary names lists from there on).  An empty dictionary gives no run.
 * Every check runs before anything is launched or written: II2_EINVAL for a NULL array with n_patterns > 0 (run_dict and stats
 * excepted; the three run arrays may be NULL with cap == 0), k == 0 or k > II2_MAX_LISTS, a dictionary that is NULL or of
 * another device, pat_off that does not start at 0 or descends, an unknown kind, a trailing `\`, an ill-formed pattern under
 * II2_MATCH_UTF8; II2_ERANGE for a pattern above
 * II2_MATCH_MAX_PATTERN bytes or more than II2_MATCH_MAX_PATTERNS patterns (callers chunk).  n_patterns == 0 sets run_off[0] = 0
 * and launches nothing.  More runs than cap: II2_ECAPACITY with run_off and *stats completely filled and the three run arrays
 * untouched - allocate run_off[n_patterns * k] entries and call again.
 * At most two waits per call.  Not a set operation: it takes no kernel path of ii2_ctx_paths.  No workgroup waits for another.
 * Never reads past the 16 bytes of padding behind a dictionary's bytes.  Option "match.stage" (default 1): a workgroup copies
 * the bytes of its 256 terms into LDS first when they fit; 0: every thread reads global memory.  Results are identical
 * (dict_match.hip). */
#define II2_MATCH_MAX_PATTERN  64u   /* bytes per pattern; longer: II2_ERANGE */
#define II2_MATCH_MAX_PATTERNS 64u   /* patterns per call; more: II2_ERANGE (callers chunk) */
enum { II2_MATCH_CONTAINS = 0, II2_MATCH_SUFFIX = 1, II2_MATCH_GLOB = 2 };
#define II2_MATCH_NOCASE 0x80u       /* OR-ed into a kind: ASCII A-Z and a-z compare equal, no other byte folds */
#define II2_MATCH_UTF8 0x08u         /* OR-ed into a kind or into ii2_dict_fuzzy's flags: positions are UTF-8 symbols, not bytes */
typedef struct {
    uint64_t n_terms;     /* terms tested, summed over the k dictionaries */
    uint64_t n_matched;   /* (pattern, term) pairs that matched */
    uint64_t n_runs;      /* runs = run_off[n_patterns * k] */
    uint32_t n_staged;    /* workgroups that matched out of the LDS stage */
    uint32_t n_global;    /* workgroups that matched from global memory */
} ii2_match_stats;        /* 32 bytes */
int ii2_dict_match(ii2_ctx *ctx, uint32_t k, const ii2_dict *const *dicts, uint32_t n_patterns, const uint8_t *pat_bytes,
                   const uint64_t *pat_off /* n_patterns + 1, from 0 */, const uint8_t *pat_kind /* n_patterns */,
                   uint64_t *run_off /* n_patterns * k + 1 */, uint64_t *run_first, uint64_t *run_end,
                   uint32_t *run_dict /* may be NULL */, uint64_t cap, ii2_match_stats *stats /* may be NULL */);
/* The matchers' arithmetic, host only (no GPU needed): one pattern of `kind` (as above, II2_MATCH_NOCASE included) against one
 * term by the functions the kernel runs - the same parse, the same three matchers.  *match = 0 / 1.  II2_EINVAL: a NULL output,
 * NULL pat with pat_len > 0, NULL term with term_len > 0, an unknown kind, a trailing `\`, an ill-formed pattern under
 * II2_MATCH_UTF8.  II2_ERANGE: pat_len above II2_MATCH_MAX_PATTERN. */
int ii2_term_match(uint32_t kind, const uint8_t *pat, uint64_t pat_len, const uint8_t *term, uint64_t term_len, int *match);
/* The decoder's arithmetic, host only (no GPU needed): the symbols of bytes[0 .. len) by the one decoder the kernels run under
 * II2_MATCH_UTF8 (the rule above).  *n_symbols is always the full count; symbols (may be NULL with cap == 0) receives the first
 * min(cap, *n_symbols) of them; *well_formed (may be NULL) = 1 when every byte belongs to a well-formed sequence - what a pattern
 * must be.  II2_EINVAL: a NULL n_symbols, NULL bytes with len > 0, NULL symbols with cap > 0. */
int ii2_utf8_decode(const uint8_t *bytes, uint64_t len, uint32_t *symbols /* may be NULL */, uint64_t cap, uint64_t *n_symbols,
                    int *well_formed /* may be NULL */);
/* Typo-tolerant term search in k resident dictionaries: every term within an edit distance of a pattern, as list ranges for the
 * range entry points - the third mode of a search front end beside ii2_dict_find and ii2_dict_match (Lucene's FuzzyQuery; the
 * reference's dictionary library answers it with a Levenshtein automaton over the FST).  The dictionaries are scanned whole; all
 * arrays are host memory.  Everything compares bytes, as ii2_dict_match does, unless a pattern carries II2_MATCH_UTF8.
 * Pattern p is pat_bytes[pat_off[p] .. pat_off[p + 1]) and matches a term when BOTH hold: the term's first pat_prefix[p] bytes
 * equal the pattern's first pat_prefix[p] bytes (Lucene's prefix_length: stripping a common prefix changes no distance; a term
 * shorter than the prefix does not match), and the edit distance between the whole pattern and the whole term is at most
 * pat_dist[p].  pat_flags[p] is 0 or an OR of
 *   II2_FUZZY_TRANSPOSE  the distance is optimal string alignment: beside insert, delete and substitute (1 each: plain
 *                        Levenshtein, the default) swapping two adjacent bytes costs 1, and no substring is edited twice -
 *                        `ca` to `abc` is 3, not 2;
 *   II2_MATCH_NOCASE     ASCII A-Z and a-z compare equal, in the prefix test and in the distance; no other byte folds.
 *   II2_MATCH_UTF8       pattern and term are read as sequences of symbols (ii2_dict_match's rule above: a code point per
 *                        well-formed sequence, one symbol per ill-formed byte of a term) and every "byte" of this contract is a
 *                        symbol: the distance, Levenshtein or optimal string alignment, is taken between the two symbol
 *                        sequences (`cafe` is 1 edit from the 5 bytes of cafe with an acute e, not 2), pat_prefix[p] counts
 *                        symbols (above the pattern's symbol count: II2_EINVAL), the length filter compares symbol counts and
 *                        n_tested counts the pairs that pass the filters so defined.  The pattern must be well-formed UTF-8,
 *                        else II2_EINVAL.  II2_MATCH_NOCASE still folds ASCII A-Z only, and the limit stays
 *                        II2_FUZZY_MAX_PATTERN BYTES.  Flagged and unflagged patterns may be mixed in one call, each with its
 *                        own rule.
 * The empty pattern has distance term_len (symbols under II2_MATCH_UTF8) to every term.
 * The answer's layout is exactly ii2_dict_match's: pair (p, s) is entry p * k + s, its runs are the maximal stretches of
 * consecutive matching term indices, in run_off / run_first / run_end / run_dict - so pattern p is ONE group of every range entry
 * point.  The runs carry no distance, on purpose: a caller that wants tiers sends the same pattern with distances 0, 1 and 2; the
 * three groups nest, so in ii2_topk_weighted_ranges their weights add up for the closer terms.
 * Every check runs before anything is launched or written: II2_EINVAL for a NULL array with n_patterns > 0 (pat_prefix,
 * pat_flags, run_dict and stats excepted; the three run arrays may be NULL with cap == 0), k == 0 or k > II2_MAX_LISTS, a
 * dictionary that is NULL or of another device, pat_off that does not start at 0 or descends, a flag bit other than the three
 * above, a pat_prefix[p] above the pattern's length, an ill-formed pattern under II2_MATCH_UTF8; II2_ERANGE for a pattern above II2_FUZZY_MAX_PATTERN bytes, more than
 * II2_FUZZY_MAX_PATTERNS patterns (callers chunk) or a dictionary of 2^31 terms or more.  n_patterns == 0, or no term in any
 * dictionary: run_off is all zero and nothing is launched.  More runs than cap: II2_ECAPACITY with run_off and *stats completely
 * filled and the three run arrays untouched - allocate run_off[n_patterns * k] entries and call again.
 * At most two waits per call.  Not a set operation: it takes no kernel path of ii2_ctx_paths.  No workgroup waits for another.
 * Never reads past the 16 bytes of padding behind a dictionary's bytes.  On the device (dict_fuzzy.hip) a thread per term runs
 * the bit-parallel recurrence of Myers / Hyyro with a DP column in one register; terms whose length differs from the pattern's
 * by more than the distance, or whose prefix differs, are skipped before it (stats->n_tested counts the rest).  Options:
 * "fuzzy.stage" (default 1): a workgroup copies the bytes of its 256 terms into LDS first when they fit; 0: every thread reads
 * global memory.  "fuzzy.wide" (default 0): the 32-bit instance of the kernel runs when every pattern of the call holds at most
 * 32 positions (symbols under II2_MATCH_UTF8, bytes otherwise); 1: always the 64-bit one.  Results are identical under all four
 * settings.  A call in which no pattern carries II2_MATCH_UTF8 launches the kernels it always did; with one, the instances that
 * decode the term as they read it run (stats->n_utf8 > 0). */
#define II2_FUZZY_MAX_PATTERN  64u   /* bytes per pattern; longer: II2_ERANGE */
#define II2_FUZZY_MAX_PATTERNS 16u   /* patterns per call; more: II2_ERANGE (callers chunk) */
#define II2_FUZZY_TRANSPOSE    0x01u /* an adjacent transposition costs 1 (optimal string alignment) */
/* II2_MATCH_NOCASE (0x80) and II2_MATCH_UTF8 (0x08) are the only other flags */
typedef struct {
    uint64_t n_terms;    /* terms read, summed over the k dictionaries */
    uint64_t n_matched;  /* (pattern, term) pairs within distance */
    uint64_t n_runs;     /* runs = run_off[n_patterns * k] */
    uint64_t n_tested;   /* pairs that passed the length and prefix filter and ran the recurrence */
    uint32_t n_staged, n_global;   /* workgroups that matched out of LDS / from global memory */
    uint32_t word_bits;  /* 32 or 64: the instance that ran; 0 when nothing was launched */
    uint32_t n_utf8;     /* patterns of the call that carry II2_MATCH_UTF8; 0: the byte instances ran */
} ii2_fuzzy_stats;       /* 48 bytes */
int ii2_dict_fuzzy(ii2_ctx *ctx, uint32_t k, const ii2_dict *const *dicts, uint32_t n_patterns, const uint8_t *pat_bytes,
                   const uint64_t *pat_off /* n_patterns + 1, from 0 */, const uint8_t *pat_dist /* n_patterns: max distance 0 .. 255 */,
                   const uint8_t *pat_prefix /* n_patterns; NULL: all 0 */, const uint8_t *pat_flags /* n_patterns; NULL: all 0 */,
                   uint64_t *run_off /* n_patterns * k + 1 */, uint64_t *run_first, uint64_t *run_end,
                   uint32_t *run_dict /* may be NULL */, uint64_t cap, ii2_fuzzy_stats *stats /* may be NULL */);
/* The matcher's arithmetic, host only (no GPU needed): one pattern against one term by the functions the kernel runs - the same
 * parse, the same filters, the same recurrence.  *match = 0 / 1 as the kernel decides it; *dist (may be NULL) = the exact
 * distance under `flags` (in symbols under II2_MATCH_UTF8), whatever prefix and max_dist are and for any term length.  prefix and
 * max_dist are 32-bit here and any max_dist is accepted.  II2_EINVAL: a NULL match, NULL pat with pat_len > 0, NULL term with
 * term_len > 0, a flag bit other than the three above, prefix above the pattern's length (pat_len, or its symbols), an ill-formed
 * pattern under II2_MATCH_UTF8.  II2_ERANGE: pat_len above II2_FUZZY_MAX_PATTERN. */
int ii2_term_fuzzy(uint32_t flags, const uint8_t *pat, uint64_t pat_len, uint32_t prefix, uint32_t max_dist, const uint8_t *term,
                   uint64_t term_len, int *match, uint32_t *dist /* may be NULL */);
/* Regular-expression term search in k resident dictionaries: every term a pattern matches, as list ranges for the range entry
 * points - the fourth mode of a search front end beside ii2_dict_find, ii2_dict_match and ii2_dict_fuzzy (Lucene's RegexpQuery;
 * the reference's dictionary library answers it with a regex automaton walked over the FST).  It replaces the loop over every term
 * of every segment with a host regex library that a front end would run otherwise.  The dictionaries are scanned whole; all
 * arrays are host memory.  Everything compares bytes (no UTF-8: II2_MATCH_UTF8 is II2_EINVAL here, as any unknown flag bit).
 * Pattern p is pat_bytes[pat_off[p] .. pat_off[p + 1]) and matches a term when it matches the WHOLE term (GLOB's rule, vellum's
 * and Lucene's; write `.*foo.*` for "contains").  Where a pattern is accepted it means what Python's
 * re.fullmatch(pattern, term, re.DOTALL) means on bytes:
 *   literal     any byte other than \ . [ ( ) | * + ? { ^ $; an unescaped `]` outside a class and an unescaped `}` outside a
 *               counted repetition are literal;
 *   .           any byte, `\n` included;
 *   escapes     \d \D \w \W \s \S (ASCII: [0-9], [A-Za-z0-9_], [ \t\n\r\f\v] and their complements), \n \r \t \f \v, \xHH
 *               (two hex digits), `\` and an ASCII punctuation byte: that byte; anything else behind `\` is II2_EINVAL (other
 *               letters, digits, a lone `\` at the end);
 *   [...]       bytes, ranges lo-hi and the escapes above (\D \W \S included); a leading `^` negates; a `]` right after `[` or
 *               `[^` is literal, so is a `-` first or last and a `[`; hi < lo, a range that ends in a class escape or an
 *               unterminated class is II2_EINVAL;
 *   ( ) (?: )   groups, the same thing: there are no captures; any other `(?` is II2_EINVAL; empty groups and empty alternatives
 *               (`(a|)`, `a|`) match the empty string; unbalanced parentheses are II2_EINVAL;
 *   |           alternation;
 *   * + ? {m} {m,} {m,n}   on the preceding byte, `.`, class, escape or group; one `?` directly behind a quantifier is accepted
 *               and ignored (laziness cannot change a whole-term match); II2_EINVAL: any other quantifier behind a quantifier
 *               (`a**`, `a*+`, `a{2}{3}`), a quantifier with nothing in front, `{,n}`, n < m, a `{` that starts none of the three;
 *   ^ $         outside a class II2_EINVAL (there are no zero-width assertions; the literals are \^ and \$);
 *   the empty pattern matches only the empty term.
 * pat_flags[p] is 0 or II2_MATCH_NOCASE: ASCII A-Z and a-z compare equal and no other byte folds - a byte c is in a position's
 * set when fold(c) is in the fold of the listed set, and a negated class is the complement of that (`[^a]` rejects `a` and `A`,
 * `[Z-a]` accepts `z` and `A`).
 * A pattern becomes its Glushkov position automaton on the host: every byte, `.`, class or escape is one position; x{m,n} is m
 * copies of x followed by n - m nested optionals, x{m,} m copies followed by x*, x{0} nothing.  At most II2_REGEX_MAX_POSITIONS
 * positions after that expansion, II2_REGEX_MAX_PATTERN raw bytes and II2_REGEX_MAX_PATTERNS patterns: more is II2_ERANGE.
 * The answer's layout is exactly ii2_dict_match's: pair (p, s) is entry p * k + s, its runs are the maximal stretches of
 * consecutive matching term indices, in run_off / run_first / run_end / run_dict - so pattern p is ONE group of every range entry
 * point.
 * Every check runs before anything is launched or written: II2_EINVAL for a NULL array with n_patterns > 0 (pat_flags, run_dict
 * and stats excepted; the three run arrays may be NULL with cap == 0), k == 0 or k > II2_MAX_LISTS, a dictionary that is NULL or
 * of another device, pat_off that does not start at 0 or descends, a flag bit other than II2_MATCH_NOCASE, a pattern outside the
 * syntax; II2_ERANGE for the three limits or a dictionary of 2^31 terms or more.  n_patterns == 0, or no term in any dictionary:
 * run_off is all zero and nothing is launched.  More runs than cap: II2_ECAPACITY with run_off and *stats completely filled and
 * the three run arrays untouched - allocate run_off[n_patterns * k] entries and call again.
 * At most two waits per call.  Not a set operation: it takes no kernel path of ii2_ctx_paths.  No workgroup waits for another.
 * Never reads past the 16 bytes of padding behind a dictionary's bytes.  On the device (dict_regex.hip) a thread per term keeps
 * the automaton's states in one 64-bit register; terms shorter than the language's shortest or longer than its longest are
 * skipped before it (stats->n_tested counts the rest).  Option "regex.stage" (default 1): a workgroup copies the bytes of its
 * 256 terms into LDS first when they fit; 0: every thread reads global memory.  Results are identical under both settings. */
#define II2_REGEX_MAX_PATTERN   256u  /* raw bytes per pattern; longer: II2_ERANGE */
#define II2_REGEX_MAX_POSITIONS 64u   /* positions after expansion; more: II2_ERANGE */
#define II2_REGEX_MAX_PATTERNS  8u    /* patterns per call; more: II2_ERANGE (callers chunk) */
typedef struct {
    uint64_t n_terms;    /* terms read, summed over the k dictionaries */
    uint64_t n_matched;  /* (pattern, term) pairs that matched */
    uint64_t n_runs;     /* runs = run_off[n_patterns * k] */
    uint64_t n_tested;   /* pairs that passed the length filter and ran the automaton */
    uint32_t n_staged, n_global;   /* workgroups that matched out of LDS / from global memory */
    uint32_t max_positions;   /* the largest position count among the call's patterns; 0 when nothing was launched */
    uint32_t pad;
} ii2_regex_stats;            /* 48 bytes */
int ii2_dict_regex(ii2_ctx *ctx, uint32_t k, const ii2_dict *const *dicts, uint32_t n_patterns, const uint8_t *pat_bytes,
                   const uint64_t *pat_off /* n_patterns + 1, from 0 */, const uint8_t *pat_flags /* n_patterns; NULL: all 0 */,
                   uint64_t *run_off /* n_patterns * k + 1 */, uint64_t *run_first, uint64_t *run_end,
                   uint32_t *run_dict /* may be NULL */, uint64_t cap, ii2_regex_stats *stats /* may be NULL */);
/* The matcher's arithmetic, host only (no GPU needed): one pattern against one term by the functions the kernel runs - the same
 * parse, the same filter, the same step.  *match = 0 / 1.  *n_pos (may be NULL) = the pattern's positions, set whenever the
 * syntax holds: also on II2_ERANGE from the position limit, when it is the count that was too large (a caller sizes patterns by
 * it).  II2_EINVAL: a NULL match, NULL pat with pat_len > 0, NULL term with term_len > 0, a flag bit other than
 * II2_MATCH_NOCASE, a pattern outside the syntax.  II2_ERANGE: the two limits of a pattern. */
int ii2_term_regex(uint32_t flags, const uint8_t *pat, uint64_t pat_len, const uint8_t *term, uint64_t term_len, int *match,
                   uint32_t *n_pos /* may be NULL */);
/* Dictionary build step (bulk Put, in front of ii2_seg_build).  Replaces the std::sort over every term occurrence, the
 * std::unique and the string bisection per occurrence that a bulk Put does on the host before ii2_seg_build (order = bytes.Compare,
 * file/types.go:24-26).  Input: n_terms terms in any order, repeats allowed, any bytes, the empty term included - term i is
 * term_bytes[term_off[i] .. term_off[i + 1]).  *out is a dictionary like the one ii2_dict_create makes from the sorted,
 * duplicate-free terms: the same offsets, bytes, 8-byte keys and long-terms flag, usable by ii2_dict_find, ii2_align_dicts,
 * ii2_seg_select_aligned* and ii2_dict_free.  term_id[i] (may be NULL) is the index of input term i in it.
 * `where` says where term_bytes, term_off and term_id live, all three together; with II2_DEVICE term_id is directly the list_id
 * of ii2_seg_build(ctx, n_unique, n_terms, term_id, values, II2_DEVICE, ...).  n_terms == 0: the empty dictionary and all-zero
 * stats (the arrays may be NULL).
 * Every check happens before anything the caller sees is written, and *out stays NULL on any error: II2_EINVAL for a NULL
 * array with n_terms > 0 or a term_off that does not start at 0 or descends (arrays on the device are checked there, in the
 * first kernel); II2_ERANGE for 2^31 or more terms or a term longer than II2_DICT_BUILD_MAX_TERM.  After an error nothing stays
 * allocated.  The library never reads beyond term_bytes[term_off[n_terms]): the caller's arrays carry no padding.
 * On the device (dict_build.hip): bytes.Compare order is the order of (chunk 0, chunk 1, ..., length) with chunk c = bytes
 * [8c, 8c + 8) big-endian, zero padded, so the terms are sorted by a stable least-significant-digit radix sort of (64-bit key,
 * 32-bit index) pairs, 8-bit digits, the length first and then the chunks from the last to the first.  Only the bytes that can
 * differ get a pass: one kernel reduces OR and AND of every chunk and of the lengths, stats->n_passes is what
 * ii2_dict_build_plan returns for the same terms (terms behind a common prefix skip its passes, identical terms run none).
 * Then equal neighbours are numbered and the dictionary is gathered.  The call waits three times, whatever n_terms and the
 * number of passes: for the plan, for the dictionary's sizes, and at the end.  No workgroup of it waits for another.  Not a
 * set operation: it takes no kernel path of ii2_ctx_paths. */
#define II2_DICT_BUILD_MAX_TERM 256u     /* bytes per term; longer: II2_ERANGE (sort on the host, ii2_dict_create) */
typedef struct {
    uint64_t n_terms;    /* terms read */
    uint64_t n_unique;   /* distinct terms = terms of the dictionary */
    uint64_t n_bytes;    /* bytes of the dictionary */
    uint32_t min_len, max_len;
    uint32_t n_passes;   /* radix passes run */
    uint32_t pad;
} ii2_dict_build_stats;  /* 40 bytes */
int ii2_dict_build(ii2_ctx *ctx, uint64_t n_terms, const uint8_t *term_bytes, const uint64_t *term_off /* n_terms + 1, from 0 */,
                   int where, ii2_dict **out, uint32_t *term_id /* n_terms, may be NULL */, ii2_dict_build_stats *stats /* may be NULL */);
/* The sizes of a dictionary (either output may be NULL) and its arrays copied to the host: term_bytes[n_bytes], term_off[n_terms + 1]
 * (either may be NULL). */
int ii2_dict_info(const ii2_dict *dict, uint64_t *n_terms, uint64_t *n_bytes);
int ii2_dict_export(ii2_ctx *ctx, const ii2_dict *dict, uint8_t *term_bytes, uint64_t *term_off);
/* The build's arithmetic, host only (no GPU needed), by the very functions the driver and the kernels use.
 * ii2_term_chunk: the key of chunk c of a term - bytes [8c, 8c + 8) big-endian, zero padded (chunk 0 is the dictionary's key).
 * ii2_dict_build_plan: the passes ii2_dict_build would run for these terms (host arrays) - pos_pass[p] = 1 when byte position p
 * (0 .. 255) gets a radix pass, len_pass[b] = 1 when byte b (0, 1) of the lengths gets one, *n_passes their number, the least and
 * the greatest length.  Same errors as the call (and II2_EINVAL for a NULL output). */
int ii2_term_chunk(const uint8_t *term, uint64_t len, uint32_t c, uint64_t *key);
int ii2_dict_build_plan(const uint8_t *term_bytes, const uint64_t *term_off, uint64_t n_terms, uint8_t *pos_pass /* 256 */,
                        uint8_t *len_pass /* 2 */, uint32_t *n_passes, uint32_t *min_len, uint32_t *max_len);
/* The alignment of k resident dictionaries: no upload, no host pass over the terms, no sort — every term finds its place
 * in the k-way merge by bounded bisections in the other dictionaries (align.hip). */
int ii2_align_dicts(ii2_ctx *ctx, uint32_t k, const ii2_dict *const *dicts, ii2_align **out);
/* The same from flat host arrays (k temporary dictionaries are made and freed inside the call): */
int ii2_align_terms(ii2_ctx *ctx, uint32_t k, const uint8_t *term_bytes, const uint64_t *term_off,
                    const uint64_t *seg_first, ii2_align **out);
/* The alignment's arithmetic, host only (no GPU needed): what the ranking kernel of ii2_align_terms / ii2_align_dicts would do
 * for these dictionaries (host arrays as ii2_align_terms takes them), by the constants and functions the kernel uses.  A
 * workgroup takes terms_per_workgroup consecutive terms of one dictionary (n_workgroups in all); for every other dictionary it
 * finds the bracket of terms its stretch can meet, and bisects there - in LDS when the bracket has at most staged_cap entries
 * (brackets_staged), in global memory when it has more (brackets_global), not at all when it is empty (brackets_empty).
 * max_bracket is the largest bracket; long_terms is 1 when some term of any dictionary is longer than 8 bytes (a tie of the
 * 8-byte keys is then decided by the bytes, else by the lengths alone).  Same checks and codes as ii2_align_terms - II2_EINVAL:
 * k == 0 or k > II2_MAX_LISTS, a NULL array, seg_first that does not start at 0 or descends, term_off that descends, terms of a
 * dictionary that do not ascend strictly; II2_ERANGE: 2^31 or more terms - and II2_EINVAL for a NULL plan.  *plan is written
 * only on success. */
typedef struct {
    uint64_t n_terms, n_workgroups;
    uint64_t brackets_staged;   /* 0 < size <= staged_cap: bisected in LDS        */
    uint64_t brackets_global;   /* size > staged_cap: bisected in global memory   */
    uint64_t brackets_empty;    /* size == 0                                      */
    uint64_t max_bracket;
    uint32_t long_terms;        /* some term is longer than 8 bytes               */
    uint32_t terms_per_workgroup, staged_cap;
    uint32_t pad;
} ii2_align_plan_info;          /* 64 bytes */
int ii2_align_plan(uint32_t k, const uint8_t *term_bytes, const uint64_t *term_off, const uint64_t *seg_first,
                   ii2_align_plan_info *plan);
int ii2_align_info(const ii2_align *a, uint64_t *n_union, uint32_t *k);
/* rep[n_union]: index (into term_off) of one input term equal to union term u, in union order;
 * src_list[k * n_union]: row s = for every union term the term of dictionary s equal to it (index
 * inside that dictionary) or -1.  Either may be NULL. */
int ii2_align_export(ii2_ctx *ctx, const ii2_align *a, uint64_t *rep, int64_t *src_list);
/* The term-aligned view of `src` for dictionary s of the alignment, built on the device: n_union
 * slots, slot u = list first_list + (index of union term u in dictionary s), or empty.  The
 * dictionary must describe the consecutive lists [first_list, first_list + its size) of src.
 * Same result as ii2_seg_select with row s of src_list, without the mapping ever visiting the host. */
int ii2_seg_select_aligned(ii2_ctx *ctx, const ii2_seg *src, const ii2_align *a, uint32_t s,
                           uint64_t first_list, ii2_seg **out);
/* The views of ALL k dictionaries of the alignment in one call: srcs[s] / first_list[s] (NULL: 0 for every one) as above,
 * outs[k].  The same kernels with one wait at the end instead of one per view; all-or-nothing (outs are NULL on error). */
int ii2_seg_select_aligned_all(ii2_ctx *ctx, const ii2_seg *const *srcs, const ii2_align *a, const uint64_t *first_list,
                               ii2_seg **outs);
void ii2_align_free(ii2_align *a);

int ii2_seg_get_info(const ii2_seg *seg, ii2_seg_info *info);
/* Introspection: the arrays the library DERIVES when a segment is made and every query and merge kernel reads next to the DV1
 * bytes, copied to host buffers (any output may be NULL).  With n_lists / n_blocks as ii2_seg_get_info reports them (a view's
 * n_blocks is its store's):
 *   cnt[n_lists]            postings per list;
 *   last_doc[n_lists]       last doc per list, 0 for an empty list;
 *   blk_list[n_blocks + 1]  the list that owns each block, in the segment's own numbering; 0xFFFFFFFF for a block that none of a
 *                           view's lists owns and, for every segment, in the entry past the last block;
 *   spans[3 * n_lists]      {first doc, first doc of the last block, last doc} per list, zeros for an empty list: the host mirror
 *                           exactly as the path choice reads it.  Written only when the segment has the mirror
 *                           (info->spans_mirrored; segments of more than 65536 lists and the views of ii2_seg_select_aligned*
 *                           have none: their spans are fetched when a query first asks);
 *   info                    is_view: made by ii2_seg_select*; merge_blocks / merge_bytes: what a merge of the segment can at
 *                           most read - the totals, or for a view of ii2_seg_select the blocks and payload bytes of its window of
 *                           the store; n_postings: exact for whole segments and the views of ii2_seg_select, for the views of
 *                           ii2_seg_select_aligned* the store's total (an upper bound).
 * II2_EINVAL for a NULL ctx or seg and for a segment of another device.  One wait, no kernel.  Not a set operation: it takes no
 * kernel path of ii2_ctx_paths. */
typedef struct {
    uint64_t n_postings;
    uint64_t merge_blocks;
    uint64_t merge_bytes;
    uint32_t is_view;
    uint32_t spans_mirrored;
} ii2_seg_meta_info;    /* 32 bytes */
int ii2_seg_export_meta(ii2_ctx *ctx, const ii2_seg *seg, uint32_t *cnt, uint32_t *last_doc, uint32_t *blk_list, uint32_t *spans,
                        ii2_seg_meta_info *info /* may be NULL */);
/* The dense form of list list_idx, if a query has cached one: an array of 32-bit words in which bit d - origin is set when doc d is
 * in the list (origin = the list's first doc & ~31, n_words = ((last doc - origin) >> 5) + 1).  The one-launch two-list AND makes
 * it the first time it is about to mark the list - its longer one - and option intersect.dense_form allows it; later calls on
 * that list read the words instead of marking.  The forms belong to the segment's store: a view made by ii2_seg_select* and its
 * parent share them, they are counted by ii2_devmem_stats and freed with the segment.
 *   info = {present (0 / 1), origin, n_words, bytes held by this store's forms in all};
 *   words (may be NULL): the n_words words; II2_ECAPACITY when cap < n_words.
 * Builds nothing.  Not a set operation: it takes no kernel path of ii2_ctx_paths. */
int ii2_seg_dense_form(ii2_ctx *ctx, const ii2_seg *seg, uint64_t list_idx, uint64_t info[4], uint32_t *words /* may be NULL */, uint64_t cap);
/* Frees a segment.  As with any free, no call that reads the segment may still be running (the library's calls are
 * synchronous: that is "after they returned"; a query started with ii2_intersect_async is waited for first).  The
 * segment's device arrays go back to a size-class cache and are handed out again by the next segment that is made — a
 * stream of Shard.Merge calls allocates nothing and no free waits for the device.  The cache keeps at most
 * II2_DEVMEM_CACHE_MB megabytes (environment, default 16384; 0: every free goes to the driver) and is emptied when the
 * process's last context is destroyed. */
void ii2_seg_free(ii2_seg *seg);
/* Bytes of segment arrays handed out / waiting in the cache for reuse (either pointer may be NULL). */
void ii2_devmem_stats(uint64_t *live_bytes, uint64_t *idle_bytes);

/* ---- tombstones ------------------------------------------------------------------------ */
/* Replaces RemovedLists.Values() + slices.BinarySearch per value (removed_list.go:44-54,
 * shard.go:165,183): a dense bitmap over [0, max(removed)] built on the device; duplicates
 * in `removed` are harmless, order is irrelevant. */
int ii2_tomb_create(ii2_ctx *ctx, const uint32_t *removed, uint64_t n_removed, int where, ii2_tomb **out);
void ii2_tomb_free(ii2_tomb *tomb);

/* ---- the hot path ---------------------------------------------------------------------- */
/* Segment merge.  Replaces the body of Shard.Merge's loop (shard.go:163-212) together with
 * the k-way merging iterator it drains (shard.go:253-278, go-iterators NewMergingIterator
 * folding equal terms with file.MergeTermValues, file/types.go:14-22): for every aligned
 * term slot t the union of the k segments' lists, sorted, duplicate-free, minus the
 * tombstones.  All k segments must have the same n_lists (the host aligns term ids; the
 * bytes.Compare term ordering of file/types.go:24-26 stays on the host).
 * Output, device-resident: out_off[n_lists+1] (u64) and out_values (u32, capacity
 * out_cap >= sum of the inputs' n_postings is always enough).  A term whose
 * out_off[t+1]==out_off[t] has no survivors and is dropped by the caller (shard.go:192-194).
 * All-or-nothing: when the merged postings do not fit out_cap the call returns II2_ECAPACITY and
 * neither out_off nor out_values has been written (the fit is decided on the device before the
 * packing pass and the offset scan write anything). */
int ii2_merge_segments(ii2_ctx *ctx, uint32_t k, const ii2_seg *const *segs, const ii2_tomb *tomb,
                       uint64_t *d_out_off, uint32_t *d_out_values, uint64_t out_cap,
                       ii2_merge_stats *stats);
/* Same, then the encode step on the merged lists: returns a new DV1 segment (what
 * w.Append writes, shard.go:207).  *out is NULL when no term survives. */
int ii2_merge_segments_to_seg(ii2_ctx *ctx, uint32_t k, const ii2_seg *const *segs, const ii2_tomb *tomb,
                              ii2_seg **out, ii2_merge_stats *stats);

/* The common Shard.Merge in ONE launch.  Every Shard.Put writes a direct segment with one posting per term (shard.go:33-67)
 * and Shard.Merge picks the smallest segments first (shard.go:135-146): the usual merge is a handful of tiny segments.  This
 * entry point does, in one kernel and one host round trip, what otherwise takes ii2_align_terms + k x ii2_seg_select_aligned +
 * ii2_tomb_create + ii2_merge_segments_to_seg + the empty-term compaction: term alignment of the k dictionaries
 * (bytes.Compare order), same-term union, tombstone filter, empty-term drop (shard.go:192-194) and the encode step.
 * Input: k segments, segs[s] holding exactly one list per term of dictionary s, the dictionaries flat in host memory as for
 * ii2_align_terms, and RemovedLists.Values() (host, any order, duplicates allowed) or NULL.  Output: *out = the merged
 * segment, one list per SURVIVING term (NULL when none survives, shard.go:219-225); kept[j] (capacity seg_first[k]) = index
 * into term_off of an input term equal to the term of output list j; *n_kept = number of output lists.
 * Limits (II2_ERANGE beyond them: use the general entry points): */
#define II2_SMALL_MERGE_TERMS 512u       /* input terms in all */
#define II2_SMALL_MERGE_POSTINGS 8192u   /* input postings in all */
#define II2_SMALL_MERGE_REMOVED 4096u    /* removed ids */
int ii2_merge_small(ii2_ctx *ctx, uint32_t k, const ii2_seg *const *segs, const uint8_t *term_bytes, const uint64_t *term_off,
                    const uint64_t *seg_first, const uint32_t *removed, uint64_t n_removed, ii2_seg **out, uint64_t *kept,
                    uint64_t *n_kept, ii2_merge_stats *stats);

/* The small Shard.Read in ONE launch (reference shard.go:72-75 -> makeIterator shard.go:253-278: the k-way merging iterator
 * without the tombstone filter): the merged lists of k small segments straight to host memory — what otherwise takes
 * ii2_align_terms + k x ii2_seg_select_aligned + ii2_merge_segments + two downloads (1.5 ms for a few hundred bytes).
 * Dictionary s (flat, as for ii2_merge_small) names the lists list_first[s] .. of segs[s] (a range-restricted read passes
 * the slice of each segment's terms that lies in [min, max]; list_first == NULL: every dictionary starts at list 0).
 * Output: *n_union merged terms in bytes.Compare order, EVERY one of them (a read drops nothing); rep[j] (capacity
 * seg_first[k]) = index into term_off of an input term equal to term j; post_off[j] .. post_off[j + 1] (capacity
 * seg_first[k] + 1) = its ids in values (capacity cap; II2_ECAPACITY and nothing written when they do not fit).
 * Limits: II2_SMALL_MERGE_TERMS / II2_SMALL_MERGE_POSTINGS (postings of the whole segments), II2_ERANGE beyond them. */
int ii2_read_small(ii2_ctx *ctx, uint32_t k, const ii2_seg *const *segs, const uint8_t *term_bytes, const uint64_t *term_off,
                   const uint64_t *seg_first, const uint64_t *list_first, uint64_t *rep, uint64_t *post_off, uint32_t *values,
                   uint64_t cap, uint64_t *n_union);

/* Multi-term intersection (build-defined operator, absent in the reference — SURVEY §0 D1):
 * ascending ids present in every list segs[i]/list_idx[i], minus the tombstones when
 * tomb != NULL (tomb == NULL is the reference's Read behaviour).
 * d_out: device buffer, capacity cap >= the shortest list is always enough. */
int ii2_intersect(ii2_ctx *ctx, uint32_t n, const ii2_seg *const *segs, const uint64_t *list_idx,
                  const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap, uint64_t *count);
/* Enqueue only: the count lands in the device word d_count; no host synchronisation.  (What the path choice needs
 * to know about a list — its first and last doc — is mirrored on the host when its segment is created, for segments
 * of up to 65536 lists; a list of a larger segment costs one small fetch + sync the first time it is queried.) */
int ii2_intersect_async(ii2_ctx *ctx, uint32_t n, const ii2_seg *const *segs, const uint64_t *list_idx,
                        const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap, uint64_t *d_count);

/* Multi-term union.  Replaces PrefixSearch's append + slices.Sort + slices.Compact
 * (inverted_index.go:274-292).  cap >= sum of the list lengths is always enough. */
int ii2_union(ii2_ctx *ctx, uint32_t n, const ii2_seg *const *segs, const uint64_t *list_idx,
              const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap, uint64_t *count);
/* Union of every list in n list ranges: lists [list_first[i], list_end[i]) of segs[i], for any number of lists
 * (PrefixSearch: a prefix is one run of consecutive terms in each sorted dictionary).  Ascending, deduplicated ids,
 * minus the tombstones when tomb != NULL.  cap >= the postings of all the lists is always enough; on II2_ECAPACITY
 * nothing is written to d_out and *count holds the size needed.  Empty ranges and empty lists are allowed; n == 0 or
 * no postings: *count = 0, d_out untouched (may be NULL).  Segments and views (ii2_seg_select*, merged segments) alike;
 * a segment may appear in several ranges and ranges may overlap.  Up to II2_MAX_LISTS non-empty lists take the paths of
 * ii2_union; more are unioned block by block through a per-context doc bitmap (at most 128 MiB + 64 KiB, kept until
 * ii2_ctx_destroy; a doc range wider than 2^30 docs is done window by window). */
int ii2_union_ranges(ii2_ctx *ctx, uint64_t n, const ii2_seg *const *segs, const uint64_t *list_first,
                     const uint64_t *list_end, const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap, uint64_t *count);
/* AND of ORs over list ranges: the ascending, duplicate-free ids that lie in at least one list of EVERY group, minus the
 * tombstones when tomb != NULL.  Group g is the ranges group_first[g] .. group_first[g + 1] - 1 of the range arrays, each range
 * being lists [list_first[i], list_end[i]) of segs[i] exactly as ii2_union_ranges takes them (segments and views alike; a
 * segment may appear in several ranges and groups; ranges may overlap).  A term of an unmerged shard is one group holding one
 * one-list range per segment that has the term; a prefix is one run per segment.
 * n_groups == 0, or any group without postings: *count = 0, d_out untouched (may be NULL).  n_groups == 1 is the union of
 * that group.  cap >= the postings of the group with the fewest postings is always enough; on II2_ECAPACITY nothing is written
 * and *count holds the size needed.  Up to II2_MAX_LISTS groups of one non-empty list each take the paths of ii2_intersect
 * when the result surely fits; otherwise the union of the group with the fewest postings is filtered by every other group in
 * ascending order of postings (a probe of its lists per run of candidates, or a mark of its blocks into the doc bitmap that
 * ii2_union_ranges uses; see option intersect.ranges_mark).  Any number of groups. */
int ii2_intersect_ranges(ii2_ctx *ctx, uint64_t n_groups, const uint64_t *group_first, const ii2_seg *const *segs,
                         const uint64_t *list_first, const uint64_t *list_end, const ii2_tomb *tomb,
                         uint32_t *d_out, uint64_t cap, uint64_t *count);

/* AND of ORs over list ranges MINUS excluded groups - boolean queries with NOT ("docs with `error` and `db` but not
 * `healthcheck`"): the ascending, duplicate-free ids that lie in at least one list of EVERY required group and in NO list of ANY
 * excluded group, minus the tombstones when tomb != NULL.  Groups and ranges are exactly those of ii2_intersect_ranges (segments
 * and views alike; a list may appear in any number of ranges and groups; ranges may overlap; any number of groups and lists).
 * group_not (host memory, n_groups bytes): 0 = group g is required, 1 = it is excluded.
 *   - group_not == NULL: the call IS ii2_intersect_ranges (same code path, same results, same errors).  An all-zero array gives
 *     the same result (the path may differ).
 *   - n_groups == 0: *count = 0.  n_groups > 0 and no required group: II2_EINVAL - the library has no doc universe to complement.
 *     A flag other than 0 / 1: II2_EINVAL.  Bad ranges are rejected as ii2_intersect_ranges rejects them, under this entry point's
 *     name.  Every check happens before anything is launched or written.
 *   - a required group without postings, or required groups whose doc spans do not overlap: *count = 0, nothing launched, d_out
 *     may be NULL.  An excluded group without postings is ignored, and so is any excluded list whose doc span misses the required
 *     groups' common span; the excluded groups never narrow that span.
 *   - one required group is allowed: (a OR b) NOT c.  A list that is both required and excluded removes its ids.
 *   - cap >= the postings of the required group with the fewest postings is always enough.  All-or-nothing on EVERY path: on
 *     II2_ECAPACITY nothing is written to d_out and *count holds the size needed (the required part, which may go through the paths
 *     of ii2_intersect, is computed into a per-context array that always holds it, kept until ii2_ctx_destroy).
 *   - the tombstones are applied once, to the required part.
 * Short queries (see the conventions above; option andnot.small) are ONE launch and one wait: every list decoded into LDS group by
 * group, every id ranked together with its group's tag, a run of equal ids kept when it holds every required tag and not the
 * excluded one.  The general form runs the required groups through the paths of ii2_intersect_ranges, then one exclusion pass over
 * the survivors - all excluded ranges as one group, the probe / mark filter with the flag turned round (intersect.ranges_mark). */
int ii2_andnot_ranges(ii2_ctx *ctx, uint64_t n_groups, const uint64_t *group_first, const uint8_t *group_not,
                      const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end,
                      const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap, uint64_t *count);

/* MANY AND / OR queries in one call: what a search front end sends in bulk.  Replaces the per-prefix loop of PrefixSearch
 * (PrefixSearch(prefixes [][]byte), inverted_index.go:192: inverted_index.go:274-292 once per prefix) and a loop over the
 * build-defined Intersect (ii2_intersect) - a launch, and for the synchronous calls a stream wait, per query - by a number of
 * launches and ONE wait that do not depend on the number of queries.
 * Query q owns the ranges query_first[q] .. query_first[q + 1] - 1 of the range arrays (query_first[0] = 0), a range being lists
 * [list_first[i], list_end[i]) of segs[i] exactly as ii2_union_ranges takes them (segments and views alike; a segment or list
 * may appear in any number of ranges and queries; ranges may overlap).  All five arrays live in host memory.
 *   op[q] == II2_OP_OR    the union of every list in the query's ranges: the result of ii2_union_ranges on them (no range or
 *                         no postings: an empty result);
 *   op[q] == II2_OP_AND   every list in the query's ranges is one operand: the result of ii2_intersect on them (1 ..
 *                         II2_MAX_LISTS lists; an empty operand gives an empty result).
 * tomb (may be NULL) applies to every query.  The results are packed back to back in d_out (device) in query order and
 * out_off[n_queries + 1] (host) receives their offsets, out_off[0] = 0; each result is bit-identical to what the single-query
 * entry point returns for that query.  cap >= the sum over the queries of their bounds (AND: the shortest operand, OR: the
 * postings of the ranges) is always enough.
 * All-or-nothing.  Every query is checked before anything is launched: an AND without a list or with more than II2_MAX_LISTS
 * lists, a bad range, a segment of another device or an unknown op is II2_EINVAL, the message names the query's index, nothing
 * is launched and nothing written.  When the packed results exceed cap the call returns II2_ECAPACITY, d_out is untouched and
 * out_off is completely filled (allocate out_off[n_queries] ids and call again; d_out may be NULL when cap is 0).
 * n_queries == 0: out_off[0] = 0, d_out may be NULL.
 * Queries that fit one workgroup (at most 8192 postings in at most 128 blocks and II2_MAX_LISTS non-empty lists) are answered
 * together, one workgroup each, in one launch per size class; the others go one after the other through the paths of
 * ii2_intersect / ii2_union_ranges (and may cost a wait each) and are packed with the rest.  The staged results live in a
 * per-context buffer that grows to the largest batch seen and is kept until ii2_ctx_destroy. */
enum { II2_OP_AND = 0, II2_OP_OR = 1 };
int ii2_query_batch(ii2_ctx *ctx, uint64_t n_queries, const uint8_t *op, const uint64_t *query_first,
                    const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end,
                    const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap, uint64_t *out_off);

/* MANY AND-of-ORs / NOT queries in one call: ii2_query_batch for an index that is not fully merged.  There a term is not one
 * list but a group - one short list per Put segment of its shard that holds it (shard.go:33-67, :135-146) - so a front end's
 * "a AND b NOT c" is an ii2_andnot_ranges query, which ii2_query_batch's AND (every list an operand, no NOT) cannot express.
 * Replaces a loop over the build-defined Intersect / IntersectExcept (ii2_intersect_ranges / ii2_andnot_ranges: a launch and a
 * stream wait per query) and, with one required group per prefix, many prefixes ANDed (PrefixSearch(prefixes [][]byte),
 * inverted_index.go:192, followed by an intersection on the host) by a number of launches and ONE wait that do not depend on
 * the number of queries.
 * Query q owns the groups query_first[q] .. query_first[q + 1] - 1 (query_first[0] = 0); group_first[G + 1], group_not[G] and
 * the range arrays are exactly those of ii2_andnot_ranges over all G = query_first[n_queries] groups of the batch
 * (group_first[0] = 0; group_not == NULL: every group is required; segments and views alike; a list may appear in any number
 * of ranges, groups and queries).  All six arrays live in host memory.  The result of query q is bit-identical to what
 * ii2_andnot_ranges - ii2_intersect_ranges when group_not == NULL - returns for its groups:
 *   - one required group and nothing excluded is that group's union: OR, AND, AND of ORs and NOT are all one shape;
 *   - a query without a group, a required group without postings or required groups whose doc spans do not overlap: an empty
 *     result; an excluded group without postings is ignored; a list both required and excluded removes its ids;
 *   - tomb (may be NULL) applies to every query, once per query.
 * The results are packed back to back in d_out (device) in query order and out_off[n_queries + 1] (host) receives their
 * offsets, out_off[0] = 0.  cap >= the sum over the queries of the postings of their smallest required group is always enough.
 * All-or-nothing.  Every query is checked before anything is launched: a query that has groups but no required one, a flag
 * other than 0 / 1, a bad range, query_first / group_first not ascending from 0, or a segment of another device is
 * II2_EINVAL, the message names the query's index ("... query 17: ..."), nothing is launched and nothing written (tombstones
 * of another device: II2_EINVAL as well).  More than 2^20 queries, or result bounds that add up to 2^32 ids or more:
 * II2_ERANGE.  When the packed results exceed cap the call returns II2_ECAPACITY, d_out is untouched and out_off is completely
 * filled (allocate out_off[n_queries] ids and call again; d_out may be NULL when cap is 0).  n_queries == 0: out_off[0] = 0.
 * Queries that fit one workgroup (see the conventions above; option batch.groups) are answered together, one workgroup each, in
 * one launch per size class (option batch.tiny): every list decoded into LDS group by group, every id ranked with its group's
 * tag, a run of equal ids kept when it holds every required tag and not the excluded one.  The others go one after the other
 * through the paths of ii2_andnot_ranges (and cost its waits each) and are packed with the rest.  The staged results live in
 * the per-context buffer of ii2_query_batch. */
int ii2_query_batch_groups(ii2_ctx *ctx, uint64_t n_queries, const uint64_t *query_first, const uint64_t *group_first,
                           const uint8_t *group_not, const ii2_seg *const *segs, const uint64_t *list_first,
                           const uint64_t *list_end, const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap, uint64_t *out_off);

/* Hits per list against a doc set - facet counts ("of the docs matching the query, how many per level=*, per host=*?") and,
 * with the set "every doc", the document frequency of every term under a prefix.  The lists are named by n ranges exactly as
 * ii2_union_ranges takes them (segments and views alike; a list may appear in several ranges; empty ranges and empty lists are
 * allowed).  counts (host memory) receives one entry per list named, in range order - the lists list_first[0] .. list_end[0] - 1
 * of range 0, then those of range 1, and so on: counts[k] = the ids of that list that lie in the set and are not in tomb (tomb
 * may be NULL).  An empty list gets 0; a list named twice is counted twice.
 *   - the set: d_set[n_set], a device array of this context's device, ascending and duplicate-free - what every query entry
 *     point writes to d_out.  n_set == 0 with d_set != NULL: all counts are 0, nothing is launched.  d_set == NULL means "every
 *     doc": the counts are the lists' lengths minus their removed ids (tomb == NULL: from the segments' host mirrors, without a
 *     launch).  A set that is not ascending gives unspecified counts, never an access outside the call's buffers.
 *   - counts_cap smaller than the number of lists named (the sum of list_end[i] - list_first[i]): II2_ECAPACITY, nothing is
 *     launched and nothing written.  Bad ranges are rejected as ii2_union_ranges rejects them, under this entry point's name;
 *     counts == NULL with lists named, or more than 2^32 set ids: II2_EINVAL.  II2_ERANGE at 2^32 - 2 blocks or ranges, or
 *     2^31 lists named.
 *   - all-or-nothing: every argument is checked before anything is launched; counts and stats are written only on success.
 * One pass over the encoded lists, whatever their number: the set is marked once into the per-context doc bitmap of
 * ii2_union_ranges (window by window over the doc span that the set and the lists share: option union.many_window_log2), then
 * every block of the lists that can hold a set doc is decoded and each of its ids tested.  Blocks outside that span are not
 * read, and neither are those that meet no marked 2048-doc chunk of the bitmap's summary (option count.summary_skip).  The call
 * waits at most twice.  It is not a set operation: it takes no kernel path (ii2_ctx_paths). */
typedef struct {
    uint64_t n_lists;    /* lists named by the ranges = counts written */
    uint64_t n_blocks;   /* DV1 blocks those lists own */
    uint64_t n_decoded;  /* blocks decoded, summed over the windows (the others were skipped unread) */
    uint64_t n_hits;     /* sum of the counts */
    uint32_t n_windows;  /* doc windows processed (0: nothing was marked) */
} ii2_count_stats;       /* 40 bytes */
int ii2_count_ranges(ii2_ctx *ctx, uint64_t n, const ii2_seg *const *segs, const uint64_t *list_first,
                     const uint64_t *list_end, const uint32_t *d_set, uint64_t n_set, const ii2_tomb *tomb,
                     uint64_t *counts, uint64_t counts_cap, ii2_count_stats *stats /* may be NULL */);

/* Hits per list AND value bucket - the counts of ii2_count_ranges over the value axis: "matches per hour" for a query (a date
 * histogram), "matches per hour, per level=*" (terms over time) and, with the set "every doc", a term's frequency over time.  A
 * posting is a uint32 value - in the reference's use a timestamp or a record id that grows with time - and the axis cuts the
 * values into n_buckets buckets.
 *   - the edges: edges[n_buckets + 1] (host memory), strictly ascending, each <= 2^32; bucket b is the ids edges[b] <= id <
 *     edges[b + 1].  The values are 64-bit only so that edges[n_buckets] = 2^32 can include id 0xFFFFFFFF; on the device the axis
 *     is a uint32 first id per bucket plus one inclusive last id.  Ids below edges[0] or at / above edges[n_buckets] are counted
 *     nowhere - the value-range restriction: blocks wholly outside the axis are not read, the set is not marked outside it.
 *   - ii2_histogram_ranges: ranges, set, tombstones and the order of the lists named are exactly ii2_count_ranges'.
 *     counts[k * n_buckets + b] = the ids of list k in bucket b that lie in the set and are not in tomb.  d_set == NULL means
 *     "every doc", minus tomb when given; unlike ii2_count_ranges that form always runs the walk.  With edges = {0, 2^32} the counts
 *     equal ii2_count_ranges' on the same arguments.
 *   - ii2_histogram_ids: counts[b] = the ids of the ascending, duplicate-free device set d_set[n_set] in bucket b, minus tomb.  A
 *     set that is not ascending gives unspecified counts, never an access outside the call's buffers.  n_set == 0: zeros, no
 *     launch.  Without tomb one thread per bucket bisects the set; with it every id finds its bucket and tests its bit.
 *   - II2_EINVAL: n_buckets == 0, edges NULL, not strictly ascending or above 2^32; counts == NULL with cells to write; the range
 *     errors of ii2_count_ranges under this entry point's name; tombstones of another device; NULL ctx; 2^32 ids or more
 *     (ii2_histogram_ids).  II2_ERANGE: more than II2_HIST_MAX_BUCKETS buckets (chunk the axis), more than II2_HIST_MAX_CELLS
 *     lists named x buckets (chunk the lists), and ii2_count_ranges' block / range / list limits.  II2_ECAPACITY: counts_cap <
 *     lists named x n_buckets (ii2_histogram_ids: < n_buckets); nothing is launched and nothing written.
 *   - all-or-nothing: every argument is checked before anything is launched; counts and stats are written only on success.
 * ii2_histogram_ranges is ii2_count_ranges' pass with a two-dimensional counter index: one pass over the encoded lists whatever the
 * number of buckets, the same marking of the set - over the doc span that the set, the lists AND the axis share -, the same summary
 * skip (option count.summary_skip) and at most two waits (the "every doc" form: one).  A block's doc bounds say, before it is
 * read, which buckets it can meet (ii2_hist_block): a block inside ONE bucket - most blocks - is counted as ii2_count_ranges
 * counts it, one atomic per (wave, list, bucket); a block that meets 2 .. 64 buckets or leaves the axis sends each hit through a
 * bucket search into 64 counters in LDS; a block that meets more adds each hit to its global counter (option hist.whole = 0
 * sends every block through the bucket search).  Neither call is a set operation: they take no kernel path (ii2_ctx_paths). */
#define II2_HIST_MAX_BUCKETS 4096u        /* buckets per call; more: II2_ERANGE (callers chunk the axis) */
#define II2_HIST_MAX_CELLS (1u << 26)     /* lists named x buckets per call; more: II2_ERANGE (callers chunk the lists) */
typedef struct {
    uint64_t n_lists;    /* lists named by the ranges (counts written = n_lists x n_buckets) */
    uint64_t n_blocks;   /* DV1 blocks those lists own */
    uint64_t n_decoded;  /* blocks decoded, summed over the windows = n_whole + n_split + n_wide */
    uint64_t n_hits;     /* sum of the counts */
    uint64_t n_whole;    /* decoded blocks whose bounds lie in ONE bucket: no per-id bucket search */
    uint64_t n_split;    /* decoded blocks whose bounds meet 2 .. 64 buckets or leave the axis (strip form) */
    uint64_t n_wide;     /* decoded blocks whose bounds meet more than 64 buckets */
    uint32_t n_windows;  /* doc windows processed (0: nothing was marked) */
    uint32_t n_buckets;
} ii2_hist_stats;        /* 64 bytes */
int ii2_histogram_ranges(ii2_ctx *ctx, uint64_t n, const ii2_seg *const *segs, const uint64_t *list_first,
                         const uint64_t *list_end, const uint32_t *d_set, uint64_t n_set, const ii2_tomb *tomb,
                         uint32_t n_buckets, const uint64_t *edges /* n_buckets + 1, host */, uint64_t *counts,
                         uint64_t counts_cap, ii2_hist_stats *stats /* may be NULL */);
int ii2_histogram_ids(ii2_ctx *ctx, const uint32_t *d_set, uint64_t n_set, const ii2_tomb *tomb, uint32_t n_buckets,
                      const uint64_t *edges, uint64_t *counts, uint64_t counts_cap);
/* Host only, no GPU: the arithmetic the histogram kernels run (the same functions).  Both check the edges as the calls above do.
 * ii2_hist_bucket: *bucket = the bucket of id, -1 outside the axis.  ii2_hist_block: what a block with the doc bounds
 * [first_doc, up] is to the axis - inside a list `up` is the next block's first doc, at a list's end the list's last doc -: SKIP
 * the bounds miss the axis (b_lo, b_hi = 0); else *b_lo .. *b_hi are the buckets that the bounds, clipped to the axis, meet, and the
 * block is WHOLE (both bounds inside one bucket), SPLIT (2 .. 64 buckets, or one bucket with a bound outside the axis) or WIDE
 * (more than 64 buckets). */
#define II2_HIST_SKIP 0
#define II2_HIST_WHOLE 1
#define II2_HIST_SPLIT 2
#define II2_HIST_WIDE 3
int ii2_hist_bucket(const uint64_t *edges, uint32_t n_buckets, uint32_t id, int64_t *bucket /* -1: outside */);
int ii2_hist_block(const uint64_t *edges, uint32_t n_buckets, uint32_t first_doc, uint32_t up, int *kind, uint32_t *b_lo,
                   uint32_t *b_hi);

/* Which groups each doc of an id array lies in - what ii2_atleast_ranges, the ii2_topk_* calls and a term search's one group of
 * many lists do not say: highlighting, "matched queries", which 3 of 5 groups gave a score of 3, the d = 0 tier of a fuzzy hit
 * against its d = 2 tier.  The transpose of ii2_count_ranges: one pass over the groups' blocks, a hit sets a bit in its doc's row.
 *   - groups and ranges are exactly those of ii2_intersect_ranges (arrays in host memory, group_first[0] = 0; segments and views
 *     alike; a list may appear in any number of ranges and groups; ranges may overlap; empty ranges, empty lists and empty groups
 *     are allowed).  There is no group_not and no tomb: an excluded group is one more group whose bit the caller reads, and the
 *     ids are given, not filtered.
 *   - the ids: d_ids[n_ids], a device array of this context's device, IN ANY ORDER - a boolean query's ascending result or a
 *     ranked page (score-descending) alike.
 *   - the masks: d_masks (device) receives n_ids * n_words 64-bit words, doc-major, n_words = ceil(n_groups / 64): bit g & 63 of
 *     word i * n_words + (g >> 6) is set exactly when d_ids[i] lies in at least one list of group g.  The bits at and above
 *     n_groups in a row's last word are 0.
 *   - an id that is repeated: its FIRST row holds its mask, every later row is all zero (deterministic).  A repeated id never
 *     causes an access outside the call's buffers.
 *   - n_ids == 0 or n_groups == 0: nothing is launched or written, the device pointers may be NULL.  No group owns a block, or the
 *     ids' span misses the lists' span: the masks are zeroed and n_decoded = 0.
 *   - every check runs before anything is launched or written; stats is written only on success.  II2_EINVAL: a NULL array with
 *     something to read or write, bad ranges (rejected as ii2_count_ranges rejects them, under this entry point's name),
 *     group_first not ascending from 0, a segment of another device.  II2_ERANGE: n_ids > II2_EXPLAIN_MAX_IDS (the pointer is
 *     not read), 2^32 - 2 blocks or ranges, 2^32 - 1 groups.  II2_ECAPACITY: masks_cap < n_ids * n_words, nothing is written.
 * The ids are inserted into an open-addressing table of (id, row) entries in workspace - 1 << log2_slots slots, the smallest
 * power of two >= 2 * n_ids and at least 64, linear probing from ii2_explain_slot(id), the smaller row winning a repeated id - and
 * marked into the per-context doc bitmap of ii2_union_ranges, window by window over the doc span that the ids and the lists share
 * (option union.many_window_log2); then every block of the groups that can hold one of them is decoded (blocks that meet no
 * marked 2048-doc chunk are not read: option count.summary_skip), and each id whose bit is marked looks its row up and ORs its
 * group's bit in.  The bitmap and its summary are all zero again when the call returns.  The call waits at most twice (the spans,
 * the stats).  It is not a set operation: it takes no kernel path (ii2_ctx_paths). */
#define II2_EXPLAIN_MAX_IDS (1u << 24)   /* ids per call; more: II2_ERANGE (rows are independent: callers chunk) */
typedef struct {
    uint64_t n_ids;      /* rows */
    uint64_t n_lists;    /* lists named by the ranges */
    uint64_t n_blocks;   /* DV1 blocks those lists own */
    uint64_t n_decoded;  /* blocks decoded, summed over the windows */
    uint64_t n_hits;     /* (doc, group) bits set = popcount of all masks */
    uint32_t n_windows;  /* doc windows processed (0: nothing was marked) */
    uint32_t n_words;    /* mask words per doc = ceil(n_groups / 64) */
    uint32_t log2_slots; /* size of the id -> row table; 0 when nothing was launched */
    uint32_t pad;
} ii2_explain_stats;     /* 56 bytes */
int ii2_explain_ranges(ii2_ctx *ctx, uint64_t n_groups, const uint64_t *group_first, const ii2_seg *const *segs,
                       const uint64_t *list_first, const uint64_t *list_end, const uint32_t *d_ids, uint64_t n_ids,
                       uint64_t *d_masks, uint64_t masks_cap, ii2_explain_stats *stats /* may be NULL */);
/* Host only, no GPU: the slot an id's probe starts at in a table of 1 << log2_slots entries, by the function the kernels run
 * (a multiplicative hash; tests choose colliding ids with it).  log2_slots outside 1 .. 31 or slot == NULL: II2_EINVAL. */
int ii2_explain_slot(uint32_t id, uint32_t log2_slots, uint32_t *slot);

/* MANY explains in one call - the pages that ii2_topk_batch / ii2_query_batch_groups hand back, each explained against its own
 * groups: query q owns the groups query_first[q] .. query_first[q + 1] - 1 of an ii2_explain_ranges call and the ids
 * d_ids[ids_off[q] .. ids_off[q + 1]) - the d_ids / out_off of those calls fit as they are.
 *   - query_first, group_first and the range arrays are exactly those of ii2_query_batch_groups (host memory, ascending from 0).
 *     As in ii2_explain_ranges there is no group_not and no tomb.  d_ids is a device array, the ids of a page in any order;
 *     ids_off (host, n_queries + 1) ascends from 0.
 *   - the masks: with n_words_q = ceil(n_groups_q / 64), query q's rows are the n_ids_q * n_words_q words of d_masks (device) from
 *     word mask_off[q] = the sum over the queries p before it of n_ids_p * n_words_p, and they are bit for bit what
 *     ii2_explain_ranges writes for that query alone: the first-row rule of a repeated id, zero bits at and above n_groups_q,
 *     all-zero rows for ids that lie in no list.  mask_off (host, n_queries + 1, may be NULL) depends on the arguments alone - no
 *     two-call protocol - and is filled on success and on II2_ECAPACITY.
 *   - all or nothing: every check runs before anything is launched or written.  II2_EINVAL ("ii2_explain_batch: query N: ..."):
 *     a NULL array with something to read or write, query_first / group_first / ids_off not ascending from 0, a bad range
 *     (rejected as ii2_explain_ranges rejects it), a segment of another device.  II2_ERANGE: more than 2^20 queries, a query of
 *     more than II2_EXPLAIN_MAX_IDS ids, 2^32 rows or more in all, the per-query block / range / group limits of
 *     ii2_explain_ranges.  II2_ECAPACITY: masks_cap < mask_off[n_queries]; d_masks is untouched and stats is not written.
 *     n_queries == 0: mask_off[0] = 0, the device pointers may be NULL.
 * A query whose non-empty lists are at most II2_MAX_LISTS and hold at most 8192 postings in at most 128 blocks, with at most
 * II2_EXPLAIN_BATCH_IDS ids, is answered by one workgroup of the batch kernel (option batch.explain; option batch.tiny picks the
 * 256- or the 1024-thread form): every list decoded into LDS, the page's ids in an LDS table that keeps a repeated id's first
 * row, one bisection per (row, list) pair, a hit ORed into its row.  No per-context scratch is touched and no workgroup waits for
 * another; the call waits ONCE for all of them.  Every other query with ids and blocks runs through ii2_explain_ranges' form on
 * its own slices, with that form's waits; a query without ids, without groups or whose groups own no block runs nothing (its
 * rows, if any, are zero).  The call takes no kernel path (ii2_ctx_paths). */
#define II2_EXPLAIN_BATCH_IDS 1024u     /* ids of a page the batch kernel takes: table + ids + decoded postings stay below 64 KB of LDS */
typedef struct {
    uint32_t n_tiny, n_small;   /* queries answered by the batch kernel, per size class */
    uint32_t n_single;          /* queries run one by one through ii2_explain_ranges' form */
    uint32_t n_empty;           /* queries for which nothing ran */
    uint64_t n_rows;            /* rows = ids_off[n_queries] */
    uint64_t n_words;           /* mask words written = mask_off[n_queries] */
    uint64_t n_hits;            /* (doc, group) bits set = popcount of all masks */
} ii2_explain_batch_stats;      /* 40 bytes: four 32-bit words, then three 64-bit ones at offsets 16, 24, 32 - no padding anywhere */
int ii2_explain_batch(ii2_ctx *ctx, uint64_t n_queries, const uint64_t *query_first, const uint64_t *group_first,
                      const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end,
                      const uint32_t *d_ids, const uint64_t *ids_off /* host, n_queries + 1, ascending from 0 */,
                      uint64_t *d_masks, uint64_t masks_cap /* words */, uint64_t *mask_off /* host, n_queries + 1, may be NULL */,
                      ii2_explain_batch_stats *stats /* may be NULL */);
/* Host only, no GPU: the form the planner of ii2_explain_batch gives a query whose n_lists non-empty lists hold n_postings
 * postings in n_blocks blocks, with n_ids ids, under the values batch_explain / batch_tiny of the two options - by the function
 * the driver bins its queries with.  EMPTY: no ids or no block.  form == NULL: II2_EINVAL. */
#define II2_EXPLAIN_BATCH_EMPTY 0
#define II2_EXPLAIN_BATCH_TINY 1
#define II2_EXPLAIN_BATCH_SMALL 2
#define II2_EXPLAIN_BATCH_SINGLE 3
int ii2_explain_batch_plan(uint64_t n_lists, uint64_t n_postings, uint64_t n_blocks, uint64_t n_ids, int64_t batch_explain,
                           int64_t batch_tiny, uint32_t *form);

/* THRESHOLD query - "docs that lie in at least min_match of these n groups" (minimum-should-match, n-gram / fuzzy term matching,
 * "any two of these tags"): the ascending, duplicate-free ids that lie in at least one list of AT LEAST min_match required groups
 * and in NO list of ANY excluded group, minus the tombstones when tomb != NULL.  An id that sits in several lists of one group
 * counts once for that group.  Groups, ranges and group_not are exactly those of ii2_andnot_ranges (segments and views alike; a
 * list may appear in any number of ranges and groups; ranges may overlap; group_not == NULL: every group is required).
 * ii2_union_ranges is min_match = 1, ii2_andnot_ranges is min_match = the number of required groups.
 *   - min_match == 0: II2_EINVAL.  n_groups > 0 and no required group: II2_EINVAL, for the reason ii2_andnot_ranges gives.  A
 *     flag other than 0 / 1: II2_EINVAL.  Bad ranges are rejected as ii2_andnot_ranges rejects them, under this entry point's
 *     name.  Every check happens before anything is launched or written.
 *   - a required group without postings does NOT fail the query: it matches no doc.  With n' the number of required groups
 *     that have postings: min_match > n', or n_groups == 0: *count = 0, nothing is launched, d_out may be NULL.  An excluded
 *     group without postings is ignored, and so is any excluded list whose doc span misses the required groups' span.
 *   - a result doc lies in at least one of any n' - min_match + 1 groups, so cap >= the postings of the n' - min_match + 1
 *     required groups with the fewest postings is always enough (ii2_andnot_ranges' bound at min_match = n', ii2_union_ranges'
 *     at 1).  All-or-nothing on EVERY form: on II2_ECAPACITY nothing is written to d_out and *count holds the size needed.
 *   - the counting form holds its counters in at most 8 bit planes: 1 < min_match < n' with min_match > 255 is II2_ERANGE.
 *     II2_ERANGE also at 2^32 - 2 blocks or ranges.
 *   - stats and *count are written only on success and on II2_ECAPACITY.
 * The forms, tried in this order (stats->form tells which one ran; the call counts no kernel path of its own in ii2_ctx_paths -
 * the two hand-offs run existing code and count its paths):
 *   II2_ATLEAST_NONE   nothing to do (count 0, nothing launched).
 *   II2_ATLEAST_AND    min_match = n': the call is ii2_andnot_ranges on the required groups that have postings plus the
 *   II2_ATLEAST_OR     excluded ones; min_match = 1 with no excluded list that counts: the call is ii2_union_ranges on the
 *                      required ranges.  Same results, same errors as those entry points (option atleast.handoff, default 1;
 *                      min_match = n' > 255 is handed off whatever the option says: the counters cannot hold it).
 *   II2_ATLEAST_SMALL  the lists that count fit one workgroup (at most II2_MAX_LISTS non-empty lists, required and excluded
 *                      together, 8192 postings in 128 blocks, by default postings x lists <= 32768): ONE launch and one wait,
 *                      the kernel of ii2_andnot_ranges' one-launch form with "at least min_match required tags" as the rule for a
 *                      run of equal ids (option atleast.small: 1 default, 2 up to the kernel's capacity, 0 never).
 *   II2_ATLEAST_COUNT  any number of groups and lists: per window of the doc span, the groups in ascending order of postings
 *                      are marked one after the other into the per-context doc bitmap of ii2_union_ranges (the union is what
 *                      counts an id once per group) and added into a bit-sliced counter per doc - B = bit_width(min_match)
 *                      bitmaps, saturating, a second grow-only per-context allocation of at most 128 MiB kept until
 *                      ii2_ctx_destroy.  A doc absent from the first n' - min_match + 1 groups cannot reach min_match: the
 *                      groups behind them ("late") only add into 2048-doc chunks that already hold a counter.  Then the
 *                      excluded lists are marked, the counters compared with min_match, and the union's count / scan / compact
 *                      kernels produce the ids (tombstones, several windows, count-first when they may not fit).  The window
 *                      is min(1 << union.many_window_log2, 2^30 / B rounded down to a power of two) docs. */
#define II2_ATLEAST_NONE 0u
#define II2_ATLEAST_SMALL 1u
#define II2_ATLEAST_COUNT 2u
#define II2_ATLEAST_AND 3u
#define II2_ATLEAST_OR 4u
typedef struct {
    uint64_t n_counted;   /* required groups with postings (n') */
    uint64_t bound;       /* the result bound the call used: the postings of the n' - min_match + 1 smallest of them (0: min_match > n') */
    uint32_t form;        /* II2_ATLEAST_NONE / _SMALL / _COUNT / _AND / _OR: what ran */
    uint32_t n_planes;    /* counter bitmaps of the counting form (0 otherwise) */
    uint32_t n_windows;   /* doc windows of the counting form */
    uint32_t n_late;      /* groups added in "late" mode */
} ii2_atleast_stats;      /* 32 bytes */
int ii2_atleast_ranges(ii2_ctx *ctx, uint64_t n_groups, const uint64_t *group_first,
                       const uint8_t *group_not, uint32_t min_match,
                       const ii2_seg *const *segs, const uint64_t *list_first,
                       const uint64_t *list_end, const ii2_tomb *tomb,
                       uint32_t *d_out, uint64_t cap, uint64_t *count,
                       ii2_atleast_stats *stats /* may be NULL */);
/* The counting form's arithmetic, host only (no GPU needed).  For a query of n_counted required groups with postings:
 * *n_planes = bit_width(min_match), *window_docs = the docs per window at option union.many_window_log2 = window_log2 (see above;
 * n_planes x window_docs / 8 <= 128 MiB), *first_late = n_counted - min_match + 1 - the groups from that index on, in ascending
 * order of postings, are added in late mode.  min_match == 0: II2_EINVAL.  1 < min_match < n_counted with min_match > 255:
 * II2_ERANGE.  min_match > n_counted (nothing runs), or min_match = n_counted > 255 (always handed off): all three are 0. */
int ii2_atleast_plan(uint64_t n_counted, uint32_t min_match, uint32_t window_log2,
                     uint32_t *n_planes, uint64_t *window_docs, uint64_t *first_late);
/* *mask = the docs of one bitmap word whose counter is >= min_match after the words adds[0 .. n_adds) have been added into
 * n_planes zero planes, by the functions the kernels run (saturating: a counter never wraps).  n_planes outside 1 .. 8,
 * min_match == 0 or min_match >= 2^n_planes: II2_EINVAL. */
int ii2_atleast_word(uint32_t n_planes, uint32_t min_match, const uint32_t *adds, uint32_t n_adds, uint32_t *mask);

/* RANKED query - "the k docs that match the most of these groups, and how many each matched": what a search front end asks of
 * a posting-list engine most often.  Groups, ranges and group_not are exactly those of ii2_atleast_ranges / ii2_andnot_ranges
 * (segments and views alike; a list may appear in any number of ranges and groups; ranges may overlap; group_not == NULL: every
 * group is required).  score(d) = the number of REQUIRED groups that hold d in at least one list (an id in several lists of one
 * group counts once).  d is eligible when score(d) >= min_match, d lies in no list of any excluded group, and d is not in tomb
 * (when tomb != NULL).  The result is the k eligible docs that come first in the order SCORE DESCENDING, THEN DOC ID ASCENDING -
 * ties at the cut go to the smallest ids - written in that order to d_ids[0 .. *count), d_scores[i] = score(d_ids[i]);
 * *count = min(k, eligible docs).  It replaces a loop of ii2_atleast_ranges calls with min_match = n', n' - 1, ... until k ids
 * have come back (n' marks and adds per round, and no score per doc), or n ii2_union_ranges calls, n downloads and a count on
 * the host.
 *   - a required group without postings matches no doc, as in ii2_atleast_ranges.  With n' the required groups that have
 *     postings: min_match > n', or n_groups == 0: *count = 0, hist all zero, nothing is launched, the device pointers may be
 *     NULL.  An excluded group without postings is ignored, and so is any excluded list whose doc span misses the required
 *     groups' span.
 *   - II2_EINVAL: min_match == 0; n_groups > 0 and no required group; a flag other than 0 / 1; a bad range (rejected as
 *     ii2_andnot_ranges rejects it, under this entry point's name); d_ids == NULL with k > 0 and something to return.
 *     II2_ERANGE: n' > 255 (the scores are exact 8-bit counters and must not saturate); k > II2_TOPK_MAX (a ranked page, not a
 *     dump: whoever wants every doc calls ii2_atleast_ranges); 2^32 - 2 blocks or ranges.  Every check happens before anything is
 *     launched or written.
 *   - k == 0 is allowed: only hist and stats are produced (the score distribution), nothing is emitted, d_ids may be NULL.
 *   - *count <= k always: there is no II2_ECAPACITY.  d_ids and d_scores hold k entries; d_scores may be NULL; the entries
 *     [*count, k) are not written.  All-or-nothing: on any error d_ids, d_scores, hist, stats and *count are untouched.
 *   - hist (host, 256 entries, may be NULL): hist[s] = the eligible docs whose score is exactly s - 0 for s < min_match and for
 *     s > n'.
 * How it runs (the call counts no kernel path in ii2_ctx_paths): per window of the doc span - min(1 << union.many_window_log2,
 * 2^30 / B rounded down to a power of two) docs, B = bit_width(n') - every required group is marked into the per-context doc
 * bitmap and added into B counter bitmaps as ii2_atleast_ranges' counting form does it, the excluded lists are marked, and
 * pass 1 tallies the eligible docs by score.  The host reads the histogram and cuts it for k (ii2_topk_cut).  Pass 2 counts the
 * docs of every score from the cut up per 65536-doc stretch, scans that class-major table once and places every doc directly:
 * rank order without a sort, the cut class filled by its smallest ids up to its quota.  With one window the counters stay
 * between the passes and every group is marked once; with several, pass 2 marks and adds again.  A one-window call waits twice
 * (a third time for the bounds of spans the host does not mirror).  The call leaves the per-context scratch - doc bitmap,
 * counter planes and their summaries - all zero, as every call that uses them does; its temporaries are workspace. */
#define II2_TOPK_MAX (1u << 20)
typedef struct {
    uint64_t n_counted;   /* required groups with postings (n') */
    uint64_t n_eligible;  /* eligible docs = sum of hist */
    uint64_t n_cut;       /* docs of score cut_score returned: the smallest ids of that score */
    uint32_t max_score;   /* highest score of an eligible doc (0: none) */
    uint32_t cut_score;   /* lowest score returned (0: nothing returned) */
    uint32_t n_planes;    /* counter bitmaps: bit_width(n'); 0 when nothing ran */
    uint32_t n_windows;   /* doc windows */
    uint32_t n_marks;     /* mark launches for required groups, over the whole call */
    uint32_t pad;
} ii2_topk_stats;         /* 48 bytes */
int ii2_topk_ranges(ii2_ctx *ctx, uint64_t n_groups, const uint64_t *group_first,
                    const uint8_t *group_not, uint32_t min_match, uint64_t k,
                    const ii2_seg *const *segs, const uint64_t *list_first,
                    const uint64_t *list_end, const ii2_tomb *tomb,
                    uint32_t *d_ids, uint32_t *d_scores /* may be NULL */, uint64_t *count,
                    uint64_t *hist /* host, 256 entries, may be NULL */,
                    ii2_topk_stats *stats /* may be NULL */);
/* The ranked query's arithmetic, host only (no GPU needed).  ii2_topk_cut: for a histogram of 256 entries (hist[s] = docs of
 * score s) and k, *cut_score = the largest s with sum(hist[t], t >= s) >= k - the smallest s with hist[s] > 0 when fewer than k
 * docs are there -, *n_above = sum(hist[t], t > cut_score), *n_cut = min(hist[cut_score], k - n_above), *max_score = the largest s
 * with hist[s] > 0.  k == 0 or an all-zero hist: all four are 0.  A NULL argument: II2_EINVAL. */
int ii2_topk_cut(const uint64_t *hist, uint64_t k, uint32_t *max_score, uint32_t *cut_score,
                 uint64_t *n_above, uint64_t *n_cut);
/* scores[i] = the counter of the doc at bit i of one bitmap word after the words adds[0 .. n_adds) have been added into n_planes
 * zero planes, read back by the function the kernels use to extract a score; docs outside mask get 0.  (The adds saturate at
 * 2^n_planes - 1, which the ranked query never reaches.)  n_planes outside 1 .. 8, a NULL scores, or a NULL adds with
 * n_adds > 0: II2_EINVAL. */
int ii2_topk_word(uint32_t n_planes, const uint32_t *adds, uint32_t n_adds, uint32_t mask, uint32_t *scores /* 32 */);

/* ---- the ranked query with a weight per group ---------------------------------------------- */
/* ii2_topk_ranges ranks by the number of groups a doc lies in; here every required group carries a weight - an idf tier, a field
 * boost (title:error^4 body:error^1 host:db*^2) - and score(d) = the sum of group_weight[g] over the REQUIRED groups g that hold
 * d in at least one list.  d is eligible when score(d) >= min_score, d lies in no list of any excluded group, and d is not in
 * tomb.  Everything not stated here is ii2_topk_ranges' contract word for word: groups, ranges, group_not, the tombstones, the
 * order (score descending, then doc id ascending), *count <= k, k == 0, d_scores == NULL, all-or-nothing on every error, the
 * scratch left all zero, and the message prefix, which is this entry point's name.
 *   - group_weight (host, n_groups entries): the weight of each group; an excluded group's entry is ignored.  NULL: every weight
 *     is 1, and the call returns what ii2_topk_ranges returns for min_match = min_score.
 *   - W' = the weights summed over the n' required groups that have postings.  min_score > W', n_groups == 0, or no required
 *     group with postings: *count = 0, hist all zero, nothing is launched, stats holds only n_counted and total_weight.
 *   - II2_EINVAL: min_score == 0; a required group of weight 0 (drop the group instead); everything ii2_topk_ranges rejects as
 *     II2_EINVAL.  II2_ERANGE: a required group's weight above 255; W' above 255 (the scores are exact 8-bit values that never
 *     saturate, so ii2_topk_ranges' kernels serve unchanged); k > II2_TOPK_MAX; the block and range limits.
 *   - hist[s] = the eligible docs whose score is exactly s.
 * How it runs (no kernel path is counted): as ii2_topk_ranges with B = bit_width(W') counter bitmaps, but behind every mark the
 * group's weight is added to its docs' counters by a ripple-carry add that starts at bit ctz(weight) - the bitmaps below are
 * neither read nor written.  Late mode (option topk.late, default 1): take the counted groups in descending order of postings,
 * ties by index; the longest prefix whose weights sum to at most min_score - 1 is marked after all other groups, and its adds
 * skip every 2048-doc chunk that no earlier group touched - a doc that lies only in those groups scores below min_score.  Every
 * eligible doc's score stays exact; the big low-weight groups (the stop-words) touch only the chunks the rare terms named. */
typedef struct {
    uint64_t n_counted;     /* required groups with postings (n') */
    uint64_t n_eligible;    /* eligible docs = sum of hist */
    uint64_t n_cut;         /* docs of score cut_score returned */
    uint32_t total_weight;  /* W' = sum of the weights of the n' counted groups */
    uint32_t max_score, cut_score;
    uint32_t n_planes;      /* bit_width(W'); 0 when nothing ran */
    uint32_t n_windows, n_marks;
    uint32_t n_late;        /* counted groups added in late mode */
    uint32_t pad;
} ii2_topkw_stats;          /* 56 bytes */
int ii2_topk_weighted_ranges(ii2_ctx *ctx, uint64_t n_groups, const uint64_t *group_first, const uint8_t *group_not,
                             const uint32_t *group_weight /* host, n_groups entries; NULL: every weight 1 */,
                             uint32_t min_score, uint64_t k, const ii2_seg *const *segs, const uint64_t *list_first,
                             const uint64_t *list_end, const ii2_tomb *tomb, uint32_t *d_ids, uint32_t *d_scores,
                             uint64_t *count, uint64_t *hist /* host, 256, may be NULL */, ii2_topkw_stats *stats);
/* The weighted query's arithmetic, host only (no GPU needed).  ii2_topkw_word: ii2_topk_word with a weight per add - scores[i] =
 * the sum of weights[j] over the words adds[j] that hold bit i, as the kernels' add leaves it in n_planes planes (saturating at
 * 2^n_planes - 1, never wrapping); docs outside mask get 0.  n_planes outside 1 .. 8, a weight of 0 or above 255, a NULL scores,
 * or NULL adds / weights with n_adds > 0: II2_EINVAL. */
int ii2_topkw_word(uint32_t n_planes, const uint32_t *adds, const uint32_t *weights, uint32_t n_adds, uint32_t mask, uint32_t *scores /* 32 */);
/* What ii2_topk_weighted_ranges would use for n_counted required groups with postings, of these weights and posting counts:
 * *total_weight = W', *n_planes = bit_width(W'), *window_docs as ii2_atleast_plan gives it for that many planes, late[g] = 1 for
 * the groups added in late mode (option topk.late 1) and *n_late their number.  min_score > W': every output is 0, as
 * ii2_atleast_plan's are when nothing would run.  II2_EINVAL: a NULL output, NULL weights / postings with n_counted > 0, min_score == 0, a weight of 0.
 * II2_ERANGE: a weight above 255, W' above 255. */
int ii2_topkw_plan(uint64_t n_counted, const uint32_t *weights, const uint64_t *postings, uint32_t min_score, uint32_t window_log2,
                   uint32_t *total_weight, uint32_t *n_planes, uint64_t *window_docs, uint8_t *late /* n_counted */, uint32_t *n_late);

/* ---- many ranked queries in one call --------------------------------------------------------- */
/* Query q is an ii2_topk_weighted_ranges call over the groups query_first[q] .. query_first[q + 1] - 1 with min_score[q] and k[q];
 * query_first, group_first, group_not and the range arrays are exactly those of ii2_query_batch_groups.  group_weight (host) covers
 * all G = query_first[n_queries] groups of the batch, an excluded group's entry is ignored, NULL: every weight is 1.  min_score
 * (host, n_queries; NULL: every one is 1) and k (host, n_queries).
 *   - Result q is bit for bit what ii2_topk_weighted_ranges writes for that query: the same ids in the same order (score descending,
 *     then doc id ascending) and the same scores; its *count is out_off[q + 1] - out_off[q], its stats.n_eligible is eligible[q].
 *     The results are packed back to back in query order into d_ids and, when given, into d_scores at the same offsets.
 *   - The per-query rules are that call's, word for word: a required group without postings matches no doc; min_score[q] above W',
 *     a query without groups, or k[q] == 0 gives an empty result (eligible[q] is still exact for k[q] == 0); an excluded group
 *     without postings is ignored; tomb applies to every query.
 *   - All-or-nothing: every query is checked before anything is launched or written, and everything that call rejects is rejected
 *     with the same code - min_score 0, a weight of 0 or above 255 on a required group, W' above 255 (so n' above 255), k above
 *     II2_TOPK_MAX, no required group, a bad flag, a bad range, a segment or tombstones of another device - under the message
 *     "ii2_topk_batch: query N: ...".  More than 2^20 queries, or bounds that add up to 2^32 ids or more: II2_ERANGE.
 *   - The bound of query q is min(k[q], the postings of its required groups that have postings), 0 when nothing runs.  cap (in
 *     entries, for d_ids and d_scores each) >= the sum of the bounds is always enough.  When the packed results exceed cap:
 *     II2_ECAPACITY, d_ids and d_scores untouched, out_off completely filled, eligible and stats written.  n_queries == 0 sets
 *     out_off[0] = 0.
 * How it runs (no kernel path is counted, like the rest of the ranked family; stats tells what ran): a query whose counted lists -
 * the non-empty lists of its required groups and the excluded lists that count - are at most II2_MAX_LISTS and hold at most 8192
 * postings in at most 128 blocks, with at most II2_MAX_LISTS required groups that have postings, is answered by one workgroup of
 * the batch kernel (option batch.topk; option batch.tiny picks the 256- or the 1024-thread form): every list decoded into LDS,
 * every id ranked with its group's tag, the head of every run of equal ids sums the weights of the run's distinct required
 * groups, and the eligible (id, score) pairs are put in rank order by one stable counting sort on 255 - score.  No per-context
 * scratch is touched and the whole batch has one wait.  The other queries run one after the other through
 * ii2_topk_weighted_ranges' form, each with that form's own waits. */
typedef struct {
    uint32_t n_tiny, n_small;   /* queries answered by the batch kernel, per size class */
    uint32_t n_single;          /* queries run one by one through ii2_topk_weighted_ranges' form */
    uint32_t n_empty;           /* queries for which nothing ran */
    uint64_t n_staged;          /* sum of the queries' result bounds */
} ii2_topk_batch_stats;         /* 24 bytes */
int ii2_topk_batch(ii2_ctx *ctx, uint64_t n_queries, const uint64_t *query_first, const uint64_t *group_first,
                   const uint8_t *group_not, const uint32_t *group_weight /* NULL: every weight 1 */,
                   const uint32_t *min_score /* [n_queries]; NULL: every one 1 */, const uint32_t *k /* [n_queries] */,
                   const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end, const ii2_tomb *tomb,
                   uint32_t *d_ids, uint32_t *d_scores /* may be NULL */, uint64_t cap, uint64_t *out_off /* host, n_queries + 1 */,
                   uint64_t *eligible /* host, n_queries, may be NULL */, ii2_topk_batch_stats *stats /* may be NULL */);
/* The batch kernel's rule and the host's choice of form, host only (no GPU needed).  ii2_topk_batch_run: tags[0 .. n_tags) are the
 * group tags of one run of equal ids, ascending (required groups 0 .. n_req - 1, the excluded lists n_req), weights[t] the weight
 * of tag t < n_req; *score = the sum of the weights of the run's distinct required tags, *excluded = 1 when the run's last tag is
 * the excluded one, computed by the function the kernel calls.  A NULL argument, n_tags == 0 or above II2_MAX_LISTS + 1, n_req
 * above II2_MAX_LISTS, or a tag above n_req: II2_EINVAL. */
int ii2_topk_batch_run(const uint8_t *tags, uint32_t n_tags, uint32_t n_req, const uint8_t *weights /* n_req */,
                       uint32_t *score, uint32_t *excluded);
/* ii2_topk_batch_plan: a query whose n_lists counted lists hold n_postings postings in n_blocks blocks, n_counted required
 * groups with postings that hold req_postings of them, and k, under the values batch_topk / batch_tiny of the two options:
 * *form = the II2_TOPK_BATCH_* the host planner picks with the same function, *bound = min(k, req_postings), 0 for an empty one
 * (n_counted == 0).  A NULL output: II2_EINVAL. */
#define II2_TOPK_BATCH_EMPTY 0
#define II2_TOPK_BATCH_TINY 1
#define II2_TOPK_BATCH_SMALL 2
#define II2_TOPK_BATCH_SINGLE 3
int ii2_topk_batch_plan(uint64_t n_lists, uint64_t n_postings, uint64_t n_blocks, uint64_t n_counted, uint64_t req_postings,
                        uint64_t k, int64_t batch_topk, int64_t batch_tiny, uint32_t *form, uint64_t *bound);

/* ---- host-buffer convenience (what the cgo binding calls) ------------------------------- */
/* k term-aligned segments, flat: seg_off[k*(n_terms+1)] (per segment, offsets into that
 * segment's own slice), seg_base[k+1] (where each segment's slice starts in values).
 * removed: RemovedLists.Values() (any order, duplicates allowed) or NULL. */
int ii2_merge_host(ii2_ctx *ctx, uint32_t k, uint64_t n_terms, const uint64_t *seg_off,
                   const uint64_t *seg_base, const uint32_t *values,
                   const uint32_t *removed, uint64_t n_removed,
                   uint64_t *out_off, uint32_t *out_values, uint64_t out_cap, ii2_merge_stats *stats);
/* n lists, flat: list_off[n+1] into values. */
int ii2_intersect_host(ii2_ctx *ctx, uint32_t n, const uint64_t *list_off, const uint32_t *values,
                       const uint32_t *removed, uint64_t n_removed,
                       uint32_t *out, uint64_t cap, uint64_t *count);
int ii2_union_host(ii2_ctx *ctx, uint32_t n, const uint64_t *list_off, const uint32_t *values,
                   const uint32_t *removed, uint64_t n_removed,
                   uint32_t *out, uint64_t cap, uint64_t *count);

/* ---- multi-GPU: concatenate per-shard results in rank order ----------------------------- */
/* Replaces InvertedIndex.Read's shard-order concatenation (inverted_index.go:330-339) when
 * the term space (or the doc-id space) is sharded over the GPUs of one node.  One process
 * per GPU; rank 0 calls ii2_comm_unique_id and hands the 128 bytes to the others. */
#define II2_UNIQUE_ID_BYTES 128
#define II2_MAX_RANKS 64u
int ii2_comm_unique_id(void *id_out);
int ii2_comm_init(ii2_ctx *ctx, int world, int rank, const void *unique_id);
/* Every rank contributes d_local[n_local]; every rank receives all contributions in rank
 * order in d_out (capacity cap, in values) and the per-rank counts in counts_host[world].
 * Whether the concatenation fits is decided on the SMALLEST capacity of all ranks, identically
 * on every rank: either every rank exchanges, or every rank returns II2_ECAPACITY.  d_local may
 * be d_out + (its own offset) for an in-place gather, and must not overlap d_out otherwise. */
int ii2_allgatherv(ii2_ctx *ctx, const uint32_t *d_local, uint64_t n_local,
                   uint32_t *d_out, uint64_t cap, uint64_t *counts_host);

/* The same exchange in bytes (any device array): n_bytes / cap_bytes / counts_host are bytes. */
int ii2_allgatherv_bytes(ii2_ctx *ctx, const void *d_local, uint64_t n_bytes, void *d_out, uint64_t cap_bytes,
                         uint64_t *counts_host);

/* The exchange of MERGED SEGMENTS (what Shard.Merge writes, shard.go:207): every rank contributes the DV1 segment of its
 * term range and receives ONE segment holding all ranks' lists in rank order — the terms' global order when the ranks own
 * contiguous term ranges (shardKey ranges are contiguous, shard.go:362-378).  The postings travel encoded (about one byte
 * per posting for merged lists instead of four): after one all-gather of the ranks' shapes, ONE grouped exchange moves the
 * segment's arrays (list table, skip table, payload and the per-list counts / last docs / block owners) to every peer - a
 * send and a receive per peer and array, every peer on its own xGMI link, no host wait until the segment is complete; block
 * numbers, byte offsets and owners are shifted on arrival.  Every rank takes the same decision: II2_ERANGE on all ranks when
 * the concatenation exceeds one segment's limits.  With no communicator (one rank) *out is a copy of `local`.  `local` must be
 * a whole segment, not a view made by ii2_seg_select* (II2_EINVAL). */
int ii2_seg_allgather(ii2_ctx *ctx, const ii2_seg *local, ii2_seg **out);
/* The same concatenation on ONE device: the lists of segs[0], then those of segs[1], ... as one segment (what a rank holds after
 * the exchange, made from segments it already has - e.g. the term-range chunks of a merge; also the one-GPU check of the
 * exchange's arithmetic: same plan, same shifts).  Whole segments only; II2_ERANGE beyond one segment's limits. */
int ii2_seg_concat(ii2_ctx *ctx, uint32_t n, const ii2_seg *const *segs, ii2_seg **out);
/* Its arithmetic, host only: shape[3 r ..] = {n_lists, n_blocks, n_bytes} of rank r; list_off / block_off / byte_off
 * (world + 1 entries each) = where rank r's lists, blocks and payload bytes start in the concatenated segment.
 * II2_ERANGE when the totals exceed one segment's limits (2^31 lists or blocks, 4 GiB of payload). */
int ii2_seg_gather_plan(const uint64_t *shape, int world, uint64_t *list_off, uint64_t *block_off, uint64_t *byte_off);

/* The exchange's arithmetic, host only (no GPU needed): offsets[r] = where rank r's contribution
 * starts in the concatenation (offsets has world + 1 entries, offsets[world] = total).
 * II2_ECAPACITY when the total exceeds cap (offsets are still filled), II2_EINVAL for
 * world outside 1..II2_MAX_RANKS. */
int ii2_gatherv_offsets(const uint64_t *counts, int world, uint64_t cap, uint64_t *offsets);

/* ---- diagnostics ------------------------------------------------------------------------ */
/* Runs the device self-checks (wave scan, block decode against a scalar decode). 0 = pass. */
int ii2_selftest(ii2_ctx *ctx);
/* Tuning and diagnostic knobs, by name; unknown names are II2_EINVAL.  Path selection (1 = default on):
 *   intersect.dense, intersect.dense_bpw   the wave-streaming kernel for dense queries / its driver blocks per wave
 *   intersect.bitmap, intersect.g, intersect.wgs, intersect.map_docs   the general tile kernel's modes and sizes
 *   union.stream, union.dense, union.sparsity   unions through the streaming kernel / through the OR tiles (the latter up
 *                                           to `sparsity` docs of the lists' common range per posting, default 2048)
 *   setop.small, union.rank                 short-list ANDs / ORs in one launch; ORs of a few medium lists by ranking
 *   batch.small                             ii2_query_batch: 1 (default) the small queries of a batch share the batch kernel, 0 every
 *                                           query of a batch goes through the single-query paths one after the other
 *   batch.tiny                              ... and those of at most 2048 postings in at most 32 blocks run as 256-thread workgroups
 *                                           (1, default: up to seven per CU) or, like the rest, as 1024-thread ones (0)
 *   batch.groups                            ii2_query_batch_groups: 1 (default) the queries that fit one workgroup share the batch kernel
 *                                           (batch.tiny picks its form as above), 0 every query of a batch goes through the paths of
 *                                           ii2_andnot_ranges one after the other
 *   batch.topk                              ii2_topk_batch: 1 (default) the queries that fit one workgroup share the batch kernel
 *                                           (batch.tiny picks its form as above), 0 every query of a batch goes through
 *                                           ii2_topk_weighted_ranges' form one after the other
 *   batch.explain                           ii2_explain_batch: 1 (default) the queries that fit one workgroup share the batch kernel
 *                                           (batch.tiny picks its form as above), 0 every query of a batch that has ids and blocks
 *                                           goes through ii2_explain_ranges' form one after the other
 *   union.many                             ii2_union_ranges: 1 = the block-wise path even for <= 64 lists (default 0: only above)
 *   union.many_window_log2                  tests: docs per window of that path, 1 << N (11 .. 30, default 30)
 *   debug.union_many_no_atomics             timing experiments: that path's mark kernel sets no bit (results wrong)
 *   count.summary_skip                      ii2_count_ranges: 1 (default) a block whose docs meet no marked 2048-doc chunk of the set's
 *                                           bitmap is not decoded; 0 (tests, measuring) every block that meets the window is
 *                                           (ii2_histogram_ranges too)
 *   hist.per_wave                           ii2_histogram_ranges: query blocks per wave of its count kernel; 0 (default) by the rule of
 *                                           the block-wise paths (more than one only above 32 blocks per CU), N > 0 (tests) N
 *   hist.whole                              ii2_histogram_ranges: 1 (default) a block whose doc bounds lie in one bucket is counted
 *                                           without a bucket search per id; 0 (tests, measuring) every decoded block is searched.
 *                                           Same results
 *   intersect.ranges                        ii2_intersect_ranges: 1 = the group path even for single-list groups (default 0: they go to
 *                                           ii2_intersect's paths when the result surely fits)
 *   intersect.ranges_mark                   its filters mark a group into the doc bitmap when the group holds at most N postings per
 *                                           (list x 256 candidates) or the candidates are fewer than 1024 per CU, else probe its lists
 *                                           (default 64; 0: always probe)
 *   andnot.small                            ii2_andnot_ranges: 1 (default) queries of at most II2_MAX_LISTS non-empty lists, 8192 postings and
 *                                           128 blocks with postings x lists <= 32768 whose result surely fits run as one launch; 2 the
 *                                           same up to the kernel's capacity (no postings x lists bound); 0 never (always the general form)
 *   atleast.small                           ii2_atleast_ranges: its one-launch form, with andnot.small's values and limits (default 1)
 *   atleast.handoff                         ii2_atleast_ranges: 1 (default) min_match = n' runs ii2_andnot_ranges' paths and min_match = 1
 *                                           without exclusion ii2_union_ranges'; 0 (tests, measuring) they take the forms of its own
 *   topk.late                               ii2_topk_weighted_ranges: 1 (default) the largest groups whose weights sum to less than
 *                                           min_score are added in late mode; 0 (tests, measuring) no group is.  Same results
 *   merge.bitmap_tiles, merge.large_tile    bitmap tiles for dense terms (1: terms with >= 1 posting per 80 docs; N > 1: per N docs; 0: off)
 *                                           / input postings a doc-range tile of a large term aims at
 *   intersect.and2                          dense 2-list ANDs: 1 one launch (look-back for the output offsets), 2 two kernels, 0 the n-list kernel
 *   intersect.dense_form                    the one-launch 2-list AND reads its longer list as a cached bitmap (ii2_seg_dense_form) instead of
 *                                           marking it: 1 (default) for a list whose bitmap is at most half its payload bytes, made by
 *                                           the first such query on the list, which waits for the build once (ii2_intersect_async
 *                                           too); 0 never (no form is made or used); 2 (tests) for any list
 *   intersect.and2_tiles                    ... with such a bitmap, runs of 16 blocks of the shorter list a wave owns: 1, 2 (half as many
 *                                           workgroups, each paying its waits - skip entries, loads, look-back - once for two runs), or
 *                                           0 (default) 2 exactly when the grid at 1 is larger than the device holds at once
 *   intersect.and2_slots                    ... the workgroups "the device holds at once" of that rule: 0 (default) CUs x the runtime's
 *                                           occupancy answer for the kernel; N > 0 (tests) N
 *   intersect.and2_words                    the one-launch 2-list AND reads BOTH lists as cached bitmaps and ANDs them word by word - no
 *                                           block of either list is read: 1 (default) when intersect.dense_form != 0, each list's bitmap is
 *                                           at most half its payload bytes and the shorter list holds at least intersect.and2_words_min
 *                                           blocks - the shorter list's bitmap is then made by the first such query on the pair, which
 *                                           waits for the build once; 0 never; 2 (tests) for any pair the one-launch AND takes, unless
 *                                           intersect.dense_form = 0.  Same results, same path name (and.and2_fused)
 *   intersect.and2_words_min                ... the fewest blocks of the shorter list: 0 (default) CUs x the runtime's occupancy answer
 *                                           for the present kernel x 16 (16 384 on an MI355X); N > 0 (tests) N
 *   intersect.and2_words_store              ... how that kernel stores the result ids: 1 (default) write-through - the bytes leave the
 *                                           L2 as they are stored, the kernel's end has nothing to write back - as 16-byte stores to
 *                                           16-byte-aligned addresses between single ids; 0 plain 16-byte stores at any 4-byte
 *                                           alignment.  Same results
 *   intersect.and2_words_order              ... and when: 0 (default) both chunks of a wave are extracted before its first store;
 *                                           1 (measurements: slower) the first chunk's stores leave before the second is extracted
 *   encode.stream                           merged segments encoded in one pass over the ids (1) or by the two-pass encoder (0);
 *                                           tests: -1 / -2 force a give-up of the one-pass encoder's look-back (see below)
 *   merge.spin, intersect.and2_spin         polls a bounded inter-workgroup wait may take (tests shorten them; see ii2_ctx_counters).
 *                                           intersect.and2_spin < 0 (tests) forces a give-up: -1 workgroup 1 at once, -2 one
 *                                           workgroup in the middle of the grid only after the last workgroup has stored the count
 *                                           (which then looks valid; the host learns it from the error word alone)
 *   merge.alone                             Mi input postings above which a merge's tile kernel does not share the GPU with another
 *                                           context's (default 64: big ones only get in each other's way, small ones hide each other's tails)
 *   debug.no_chain                          experiments: the kernels that wait between workgroups (one-launch AND, one-pass encoder,
 *                                           direct placement) are NOT ordered per device across contexts (they may
 *                                           then hold each other's slots until their bounded waits run out)
 *   debug.lb_epoch                          tests: waits for the stream and sets the number of the context's last look-back launch to N
 *                                           (0 .. 2^24 - 1), nothing else: the next such launch - one-launch AND, one-pass encoder,
 *                                           ii2_lookback_check - takes N + 1, or, at N = 2^24 - 1, clears the records and starts again at 1.
 *                                           Set it while no ii2_intersect_async launch waits for its ii2_ctx_sync
 *   debug.stamps, profile.events            see ii2_debug_read / ii2_profile_read below
 * Every combination returns the same results; the tests run the kernels with the alternatives switched on and off. */
int ii2_set_option(ii2_ctx *ctx, const char *name, int64_t value);
/* With option "debug.stamps"=1 the intersect kernel sums, per workgroup, the shader cycles spent
 * in each part of its tile loop; this copies those counters (8 words per workgroup) out. */
int ii2_debug_read(ii2_ctx *ctx, uint64_t *out, uint64_t n_words);
/* With option "profile.events"=N (N > 0) every Nth call brackets its pass (intersect: every kernel of the
 * query; merge: every kernel of the call) with HIP events on the ctx stream — a timed event pair idles the stream
 * for ~10 us, so sample (N = 8) when the calls themselves are being timed; this waits for the stream and
 * returns the summed device time and the number of bracketed launches since the previous read. */
int ii2_profile_read(ii2_ctx *ctx, double *total_ms, uint64_t *launches);
/* One event pair around a whole run of calls: begin != 0 records the start event on the ctx stream, begin == 0 the
 * end event; ii2_profile_region_ms waits for the end event and returns the device time between the two — the time
 * the stream spent on everything enqueued in between, without a per-call event pair's idle time. */
/* How often this context took a second path: out[0] = merges repeated through the parking + packing pass, out[1] = two-list ANDs
 * repeated through the two-kernel form / segments encoded again by the two-pass encoder - in both cases because a BOUNDED WAIT
 * between workgroups of one launch ran out.  Those launches (the merge's direct placement, the one-launch AND, the one-pass
 * encoder) order their output by letting a workgroup wait for workgroups with smaller indices; that terminates because the
 * hardware starts a launch's workgroups in index order, which HIP does not promise - hence the bound, and the repeat on a path
 * without such waits (results identical).  A synchronous call (ii2_intersect, ii2_merge_segments_to_seg) notices its own
 * launch's give-up - by the count or byte count, which is all ones, or by the launch's error word when the give-up came after
 * the count was stored - and returns the repeated, exact result; nothing of it is reported later.  A launch of
 * ii2_intersect_async that gave up makes the next ii2_ctx_sync fail (once), whatever calls came in between.
 * out[2] = host waits (stream synchronisations) spent inside ii2_allgatherv* / ii2_seg_allgather / ii2_seg_concat so far.
 * out[3] = stream waits the per-device order of those launches (across contexts) put in front of this context's launches:
 * 0 while one context works alone.  n = number of words `out` holds (up to 4 are written). */
int ii2_ctx_counters(ii2_ctx *ctx, uint64_t *out, uint32_t n);
int ii2_profile_region(ii2_ctx *ctx, int begin);
int ii2_profile_region_ms(ii2_ctx *ctx, double *ms);
/* How often this context took each kernel path since it was created: out[i] = count of path i.  n = words `out` holds
 * (at most that many are written); returns the number of path ids the library knows.  A path is one host decision that selects a
 * kernel, a template instantiation or a kernel sequence (DESIGN.md has the list); a path chosen through another - a batch's
 * single query, the driver union of the group path, the required part of a NOT - is counted as well.  Host words only: the
 * kernels and their arguments are the same with or without a reader. */
int ii2_ctx_paths(ii2_ctx *ctx, uint64_t *out, uint32_t n);
/* Name of path i ("and.small", "or.rank", ...), NULL beyond the last id.  Needs no context and no GPU. */
const char *ii2_path_name(uint32_t i);
/* How often the merge tile kernel left its ordinary path on this context since it was created: out[i] = count of event i.  n = words
 * `out` holds (at most that many are written); returns the number of event ids the library knows.  The events are the kernel's
 * recoveries (DESIGN.md has the list): a batch of small terms redone term by term, a doc range bisected because it held more
 * postings than a tile sorts or because a bucket of its sort overflowed, and the leaves of such a bisection, by the way they were
 * merged.  Every merge counts - ii2_merge_segments*, ii2_merge_host and the merge passes of the unions.  The counters live on the
 * device and are never cleared by a call; the read waits for the context's stream. */
int ii2_merge_events(ii2_ctx *ctx, uint64_t *out, uint32_t n);
/* Name of event i ("batch_redo", "range_overfull", ...), NULL beyond the last id.  Needs no context and no GPU. */
const char *ii2_merge_event_name(uint32_t i);
/* A test and diagnostic facility, no part of any query: runs the protocol that orders the output of the one-launch two-list AND
 * and of the one-pass encoder - a workgroup publishes an amount and asks for the sum of the amounts of the workgroups before it
 * (see ii2_ctx_counters) - WITHOUT a payload, on this context's own records and launch numbers (epochs), which it shares with
 * those kernels; the kernel calls the very functions they call.  A logical grid of n_wg workgroups (1 .. II2_LB_CHECK_MAX_WG)
 * of which g_base .. n_wg - 1 are launched (g_base a multiple of 64, < n_wg); workgroup g publishes amount[g] (amount: n_wg
 * host words, each and their sum below 2^40; those before g_base are checked and not used) after delay[g] units of waiting (delay: NULL or n_wg host words, each at most
 * II2_LB_CHECK_MAX_DELAY; a unit is about half a microsecond).  spin = polls a wait may take, 1 .. II2_LB_CHECK_MAX_SPIN.
 * The records of what is NOT launched - the amounts of workgroups 0 .. g_base - 1, then, for each of the g_base / 64 groups
 * before, its amount and its inclusive prefix - are written before the launch as the caller says: seed_state[i] (II2_LB_SEED_*)
 * and seed_value[i] (< 2^40; any value: it need not be the sum it stands for), g_base + 2 * (g_base / 64) host entries each
 * in that order (NULL when g_base = 0).
 * Outputs, host arrays, one entry per launched workgroup g - g_base: out_prefix = the amounts before g as the protocol found
 * them (0 when it gave up); out_state = 0 or II2_LB_GAVE_UP_* bits; out_walk = the windows of 32 group records the workgroup
 * looked at | (the place 0 .. 31 in the last of them of the prefix record it used, or II2_LB_NO_PREFIX) << 24; out_polls = the
 * rounds of loads it took.  out_agg [n_wg - g_base] and out_grp [2 x the launched groups] receive the raw records
 * {epoch : 24 | value : 40} of the launched workgroups and groups as the kernel left them.  out_info[0] = the epoch of this
 * launch, [1] = the records' error word afterwards (= that epoch exactly when a workgroup gave up), [2] = the workgroups the
 * records hold now.  A give-up is reported here alone, never by ii2_ctx_sync.
 * II2_EINVAL for any argument outside the above, before anything is launched, counted or written. */
#define II2_LB_CHECK_MAX_WG (1u << 24)
#define II2_LB_CHECK_MAX_SPIN 65536u
#define II2_LB_CHECK_MAX_DELAY 256u
#define II2_LB_SEED_MISSING 0u /* all zero */
#define II2_LB_SEED_READY 1u   /* tagged with this launch's epoch */
#define II2_LB_SEED_STALE 2u   /* ... with the epoch before it */
#define II2_LB_SEED_LATER 3u   /* ... with the epoch after it (what a launch before a wrap of the epochs leaves) */
#define II2_LB_GAVE_UP_PREFIX 1u /* the wait for the amounts before it ran out */
#define II2_LB_GAVE_UP_GROUP 2u  /* a group's last workgroup: the wait for its group's amounts ran out */
#define II2_LB_NO_PREFIX 0xFFu
int ii2_lookback_check(ii2_ctx *ctx, uint32_t n_wg, uint32_t g_base, const uint64_t *amount, uint32_t spin, const uint8_t *seed_state,
                       const uint64_t *seed_value, const uint16_t *delay, uint64_t *out_prefix, uint32_t *out_state, uint32_t *out_walk,
                       uint32_t *out_polls, uint64_t *out_agg, uint64_t *out_grp, uint64_t *out_info);

#ifdef __cplusplus
}
#endif
#endif
