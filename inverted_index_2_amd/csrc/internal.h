// internal.h — host-side structures and kernel launcher prototypes of libii2_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <functional>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ii2.h"

// The kernel paths of the set operations (ii2_ctx_paths / ii2_path_name): one id per host decision that selects
// another kernel, template instantiation or kernel sequence.  The names live in api.cpp (PATH_NAMES), in this order.
namespace ii2 {
enum Path : uint32_t {
    P_AND_SMALL, P_AND_AND2_FUSED, P_AND_AND2_SPLIT, P_AND_DENSE2, P_AND_DENSE3, P_AND_DENSE4,
    P_AND_TILES_PAIR, P_AND_TILES, P_AND_TILES_WIDE, P_AND_TILES_SUB, P_AND_TILES_WIDE_SUB,
    P_OR_SMALL, P_OR_RANK, P_OR_STREAM2, P_OR_STREAM3, P_OR_STREAM4, P_OR_TILES, P_OR_TILES_WIDE, P_OR_MERGE,
    P_OR_MANY, P_OR_MANY_WINDOW, P_OR_MANY_COUNT_FIRST,
    P_IR_HANDOFF, P_IR_GROUPS, P_IR_PROBE, P_IR_MARK, P_IR_PROBE_DROP, P_IR_MARK_DROP,
    P_ANDNOT_SMALL, P_ANDNOT_GENERAL,
    P_BATCH_TINY, P_BATCH_SMALL, P_BATCH_SINGLE, P_BATCH_PACK,
    P_GBATCH_TINY, P_GBATCH_SMALL, P_GBATCH_SINGLE, P_GBATCH_PACK,
    P_SPAN_FETCH, P_SPAN_BOUNDS,
    P_COUNT
};
// The events of the merge tile kernel's recovery (ii2_merge_events / ii2_merge_event_name): one id per cold site of
// k_merge_tiles (merge.hip) where a tile leaves the ordinary path.  The names live in api.cpp (MERGE_EVENT_NAMES), in this order.
enum MergeEvent : uint32_t { ME_BATCH_REDO, ME_RANGE_OVERFULL, ME_RANGE_BUCKET_OVERFLOW, ME_LEAF_BITMAP, ME_LEAF_SORTED, ME_COUNT };
}  // namespace ii2

// mailbox layout (u64 words; h_mail and d_mail both hold II2_MAIL_WORDS)
constexpr size_t II2_MAIL_WORDS = 1024;
constexpr size_t II2_MAIL_COUNT = 200;     // word of h_mail that receives the result count of ii2_intersect / ii2_union
constexpr size_t II2_MAIL_LB_OWN = 24;     // the look-back error word behind a synchronous call's own launch ...
constexpr size_t II2_MAIL_LB_PENDING = 25; // ... and in front of it, as the asynchronous launches before it left it
constexpr size_t II2_MAIL_BUILD = 32;      // ii2_seg_build: {unique keys, non-empty lists, bad-id word} (seg_build.hip)
constexpr size_t II2_MAIL_DICT_BUILD = 40; // ii2_dict_build: the plan's reduction words, then the dictionary's byte count (dict_build.hip: 70 words)
constexpr size_t II2_MAIL_COMM = 256;      // all-gatherv: {count, cap} of this rank, then of every rank (2 + 2 * II2_MAX_RANKS words)

struct ii2_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::string err;
    // grow-only device scratch, carved per call (no hipMalloc on the steady-state path)
    uint8_t *ws = nullptr;
    size_t ws_cap = 0;
    size_t ws_used = 0;
    // small pinned host mailbox for counts read back after a call
    uint64_t *h_mail = nullptr;
    uint64_t *d_mail = nullptr;
    // options
    int64_t opt_intersect_g = 0;        // 0 = auto
    int64_t opt_intersect_wgs = 0;      // tile-kernel workgroups per CU (0 = default)
    int64_t opt_merge_large_tile = 0;   // 0 = default (MERGE_CAP / 20 * 19 = 3401 input postings per range tile)
    int64_t opt_merge_direct = 1;       // tiles place their survivors themselves when the output buffer surely fits (0: always park + pack)
    int64_t opt_merge_spin = 0;         // bounded waits of the direct placement: polls (0 = default; tests shorten it)
    uint64_t merge_fallbacks = 0;       // merges repeated through the parking + packing pass after a bounded wait ran out
    int64_t opt_merge_skip = 0;         // timing experiments: phases of the merge tile kernel left out (results wrong)
    int64_t opt_merge_bitmap = 1;       // single-term tiles whose doc range fits the LDS bitmap are merged by marking bits
    uint8_t *aux = nullptr;             // grow-only: merge per-tile arrays + parked survivors
    size_t aux_cap = 0;
    void *h_small_in = nullptr, *h_small_out = nullptr, *d_small_in = nullptr, *d_small_out = nullptr;   // ii2_merge_small: upload / download blocks
    void *h_segs = nullptr;             // pinned staging block of a merge call's segment views ...
    void *d_segs = nullptr;             // ... and its device copy (MergeSegs)
    // grow-only staging buffers of the encode / decode / merge-to-segment paths (no hipMalloc per call)
    uint8_t *pool[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t pool_cap[4] = {0, 0, 0, 0};
    int64_t opt_merge_alone = 0;        // merge: Mi input postings above which the tile kernel does not share the GPU with another one (0: 64)
    int64_t opt_debug_no_chain = 0;     // experiments: kernels that wait between workgroups are NOT ordered per device
    int64_t opt_debug_stamps = 0;       // intersect: collect per-phase cycle counters
    int64_t opt_intersect_map_docs = 0; // 0 = default (8192 docs per driver block)
    int64_t opt_union_rank = 1;         // unions of <= 8 lists / 2^20 postings by ranking (union_rank.hip)
    int64_t opt_union_sparsity = 2048;   // OR tiles are used up to this many docs of the common range per posting
    int64_t opt_small_setop = 1;        // queries of <= 32 blocks in all run as one single-workgroup kernel
    int64_t opt_union_stream = 1;       // ... and, for 2-4 lists paced by a long dense one, through the streaming kernel
    int64_t opt_union_dense = 1;        // unions of lists that are dense together go through the byte-map tiles (OR)
    int64_t opt_intersect_bitmap = 1;   // per-list bitmaps for very dense tiles
    int64_t opt_intersect_subtiles = 0; // tiny sparse drivers: tiles per CU their blocks are split into (0 = default)
    int64_t opt_intersect_submax = 0;   // ... and the most slices one driver block is cut into (0 = default)
    int64_t opt_intersect_dense = 1;    // dense 2..4-list queries go to the wave-streaming kernels (intersect_dense.hip)
    int64_t opt_dense_bpw = 0;          // driver blocks per wave there (0 = default)
    int64_t opt_encode_stream = 1;      // merged segments are encoded in one pass over the ids (encode_stream.hip)
    int64_t opt_and2_spin = 0;          // bounded waits of its look-back: polls (0 = default; 1 forces the fallback in tests)
    int64_t opt_and2_tiles = 0;         // tiles a wave of the one-launch two-list AND owns where the longer list has a dense form: 0 auto, 1, 2
    int64_t opt_and2_slots = 0;         // ... auto: workgroups of the one-tile instance the device holds at once (0 = CUs x the occupancy query; tests inject one)
    int and2_wgs_per_cu = -1;           // the occupancy query's answer, asked once (-1: not yet)
    int64_t opt_and2_words = 1;         // two dense lists: AND the cached dense forms of BOTH word by word (intersect_words.hip): 0 never, 1 by the rule of setop.cpp and2_words_pick, 2 always (tests)
    int64_t opt_and2_words_store = 1;   // ... its id stores: 0 plain, 1 write-through (sc1) to 16-byte-aligned addresses
    int64_t opt_and2_words_order = 0;   // ... 0 both chunks of a wave are staged before the first store, 1 (measurements) chunk 0's stores leave first and chunk 1 is staged behind them
    int64_t opt_and2_words_min = 0;    // ... the rule: blocks the shorter list holds at least (0 = CUs x the occupancy query x 16; tests inject one)
    unsigned long long *d_lb = nullptr; // look-back records of the fused two-list AND: [0] error word, then agg[], grp[]
    size_t lb_cap = 0;                  // workgroups the records hold
    uint32_t lb_epoch = 0;              // launches so far
    uint64_t lb_fallbacks = 0;          // calls repeated through the two-kernel form
    uint32_t lb_pending = 0;            // first epoch of the look-back launches whose error word has not been looked at yet (0: none)
    uint32_t lb_snap_first = 0;         // epochs lb_pending .. lb_epoch as they were when the error word was copied into
    uint32_t lb_snap_last = 0;          //   h_mail[II2_MAIL_LB_PENDING] (0: no such copy waiting to be looked at)
    bool lb_async_failed = false;       // one of those gave up: ii2_ctx_sync reports it
    uint64_t lb_waits = 0;              // stream waits ii2_lookback_launch put in front of this context's launches (per-device order)
    int64_t opt_intersect_and2 = 1;     // dense 2-list ANDs: the shorter list's postings are tested against the longer one's bitmap (intersect_and2.hip)
    int64_t opt_dense_form = 1;         // ... against the longer list's cached dense form instead of marking it: 0 never, 1 where the form is <= half the list's payload, 2 always
    int64_t opt_profile_events = 0;     // N > 0: bracket the dominant kernel of every Nth call with HIP events
    uint64_t prof_calls = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;   // recorded pairs since the last read
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_pool;     // reusable pairs
    hipEvent_t region_ev[2] = {nullptr, nullptr};                 // ii2_profile_region: one pair around a whole run of calls
    unsigned long long *d_debug = nullptr;
    uint64_t *d_mail_mapped = nullptr;  // h_mail as the device sees it (result counts of the synchronous calls go there directly)
    uint32_t *d_small = nullptr;        // small set operations: ascending ids [8192] + the workgroup ticket (setop_small.hip)
    int64_t opt_union_many = 0;         // 1: ii2_union_ranges takes the block-wise path (union_many.hip) even for <= 64 lists
    int64_t opt_union_many_no_atomics = 0;     // timing experiments: its mark kernel decodes and combines but sets no bit
    int64_t opt_union_many_window_log2 = 30;   // docs per window of that path: 1 << this (tests shrink it; 11 .. 30)
    uint32_t *d_um_bits = nullptr;      // its doc bitmap + summary: all-zero between calls (grow-only, <= 128 MiB + 64 KiB)
    size_t um_bits_words = 0;
    bool um_dirty = false;              // a call stopped between mark and compact: scratch and staging are cleared / waited for first
    void *h_um = nullptr;               // pinned staging of its range descriptors (grow-only)
    size_t h_um_cap = 0;
    int64_t opt_count_summary_skip = 1; // ii2_count_ranges: blocks whose docs meet no marked chunk of the bitmap's summary are not decoded (0: tests, measuring)
    int64_t opt_hist_per_wave = 0;      // ii2_histogram_ranges: query blocks per wave of its count kernel (0: um_per_wave's rule; tests inject one)
    int64_t opt_hist_whole = 1;         // ... 0 (tests, measuring): every decoded block goes through the per-id bucket search
    int64_t opt_intersect_ranges = 0;   // 1: ii2_intersect_ranges takes the group path even where ii2_intersect's paths would do
    int64_t opt_ir_mark = 64;           // ... whose filters mark a group with at most this many postings per (list x 256 candidates), or
                                        //     fewer than 4 runs of 256 candidates per CU (0: always probe)
    int64_t opt_match_stage = 1;        // ii2_dict_match: a workgroup matches its 256 terms out of an LDS copy of their bytes where they fit (0: always from global memory)
    int64_t opt_fuzzy_stage = 1;        // ii2_dict_fuzzy: the same stage (0: always from global memory)
    int64_t opt_regex_stage = 1;        // ii2_dict_regex: the same stage (0: always from global memory)
    int64_t opt_fuzzy_wide = 0;         // ... 1: the 64-bit instance of its kernel even where every pattern holds at most 32 bytes
    uint32_t *d_ir = nullptr;           // its two candidate arrays (ping-pong; grow-only: the driver's union reserves the workspace itself)
    size_t ir_words = 0;
    void *h_ir = nullptr;               // pinned staging of its filters' descriptors (grow-only)
    size_t h_ir_cap = 0;
    int64_t opt_andnot_small = 1;       // ii2_andnot_ranges: short queries in one launch (setop_groups.hip); 0: never, 2: up to the kernel's capacity
    uint32_t *d_an = nullptr;           // its required part's result, the candidates of the exclusion pass (grow-only; neither d_ir, which the
    size_t an_words = 0;                //     group path ping-pongs in, nor workspace, which the driver's union reserves itself)
    int64_t opt_atleast_small = 1;      // ii2_atleast_ranges: short queries in one launch (setop_groups.hip), as andnot.small; 0: never, 2: up to the kernel's capacity
    int64_t opt_topk_late = 1;          // ii2_topk_weighted_ranges: 1 the big low-weight groups are added in late mode; 0 none is (tests, measuring)
    int64_t opt_atleast_handoff = 1;    // ... min_match = n' through ii2_andnot_ranges' paths, min_match = 1 without exclusion through the union's (0: tests, measuring)
    uint32_t *d_thr = nullptr;          // its counting form's counter planes + accumulated summary: all-zero between calls like d_um_bits and
    size_t thr_words = 0;               //     cleaned with it (grow-only, <= 128 MiB + 64 KiB)
    int64_t opt_batch_small = 1;        // ii2_query_batch: small queries share the batch kernel (0: every query through the single-query paths)
    int64_t opt_batch_tiny = 1;         // ... of both entry points: those of <= 2048 postings in <= 32 blocks in the 256-thread form (0: all in the 1024-thread one)
    int64_t opt_batch_groups = 1;       // ii2_query_batch_groups: queries that fit share its batch kernel (0: every query through ii2_andnot_ranges' paths)
    int64_t opt_batch_topk = 1;         // ii2_topk_batch: queries that fit share its batch kernel (0: every query through ii2_topk_weighted_ranges' form)
    int64_t opt_batch_explain = 1;      // ii2_explain_batch: queries that fit share its batch kernel (0: every query through ii2_explain_ranges' form)
    uint8_t *d_batch = nullptr;        // its device block: descriptor table, counts, offsets, scan temp, staged results (grow-only)
    size_t batch_cap = 0;
    void *h_batch = nullptr;            // pinned: the descriptor table on its way up, the offsets on their way down (grow-only)
    size_t h_batch_cap = 0;
    void *comm = nullptr;               // ncclComm_t
    int world = 1, rank = 0;
    uint64_t comm_syncs = 0;            // host waits inside the exchange entry points (what a chunked exchange pays per chunk)
    int cu_count = 256;
    unsigned long long *d_merge_events = nullptr;   // [ii2::ME_COUNT] counted by k_merge_tiles on the device (ii2_merge_events): allocated and zeroed with the
                                        //     context, never cleared by a call
    uint64_t paths[ii2::P_COUNT] = {};  // how often each kernel path was taken (ii2_ctx_paths): host words, bumped under mu where the launch is decided
};
static inline void took(ii2_ctx *ctx, ii2::Path p) { ctx->paths[p]++; }

// skip table + payload of one encoded segment; shared by the views made with ii2_seg_select
namespace ii2 {
// device memory of segments: a size-class cache in front of hipMalloc / hipFree (devmem.cpp)
hipError_t dm_alloc(void **p, size_t bytes);
void dm_free(void *p);
hipError_t dm_malloc_retry(void **p, size_t bytes);   // hipMalloc; on failure the cache's idle arrays go back to the driver and it tries once more
void dm_trim(size_t keep_bytes);
void dm_user(int delta);
void dm_stats(uint64_t *live_bytes, uint64_t *idle_bytes);
}  // namespace ii2

struct ii2_seg_store {
    ii2_skip *d_skip = nullptr;
    uint8_t *d_payload = nullptr;
    void *slab = nullptr;            // one allocation that holds ALL arrays of a small segment (ii2_merge_small): freed as a whole
    // The dense form of a list: bit d - origin of `d_words` is set when doc d is in the list (origin = first doc & ~31).  Made by the
    // first one-launch two-list AND that is about to mark the list (setop.cpp: dense_form_get), read by every later one instead of
    // marking.  Keyed by the list's first block number in the store: a view and its parent find the same entry.
    struct DenseForm {
        uint32_t *d_words = nullptr; // nullptr: the list was looked at and has no form (so far)
        uint32_t origin = 0, n_words = 0;
        uint64_t payload_bytes = 0;  // of the list: what criterion (b) compares the form's bytes with
    };
    std::mutex form_mu;              // contexts on different threads share the cache; held while a form is built: nobody reads a half-made one
    std::unordered_map<uint64_t, DenseForm> forms;
    uint64_t form_bytes = 0;         // held by the forms in all
    ~ii2_seg_store() {
        for (auto &f : forms) ii2::dm_free(f.second.d_words);
        ii2::dm_free(d_skip);
        ii2::dm_free(d_payload);
        ii2::dm_free(slab);
    }
};

// A segment is read-only once created and belongs to a DEVICE, not to a context: any context of that device may
// read it, from any thread (the reference's readers share segments, segments.go:32-46).
struct ii2_seg {
    int device = 0;
    bool is_view = false;                    // made by ii2_seg_select*: blocks numbered inside another segment's store (not self-contained)
    bool in_slab = false;                    // every array below lives in store->slab (nothing to free one by one)
    hipStream_t born = nullptr;              // stream of the call that is building the segment (cleared when it is finished): an unfinished segment's arrays may
                                             // still be written by enqueued kernels, so releasing one waits for that stream first
    std::shared_ptr<ii2_seg_store> store;   // owns d_skip / d_payload
    uint64_t n_lists = 0, n_postings = 0, n_blocks = 0, n_bytes = 0;
    // what a merge of this segment can at most read: the segment's own totals, or - for a view of some lists of a store
    // (ii2_seg_select) - the blocks and payload bytes of its window of the store; 0 = the totals above.  (A view's n_blocks and
    // n_bytes stay its STORE's: its block numbers and byte offsets live there.)
    uint64_t win_blocks = 0, win_bytes = 0;
    uint64_t merge_blocks() const { return win_blocks ? win_blocks : n_blocks; }
    uint64_t merge_bytes() const { return win_bytes ? win_bytes : n_bytes; }
    uint32_t *d_blk_off = nullptr;   // [n_lists+1]
    ii2_skip *d_skip = nullptr;      // [n_blocks+1]
    uint8_t *d_payload = nullptr;    // [n_bytes + 16]
    uint32_t *d_last_doc = nullptr;  // [n_lists] last doc id of each list (0 for an empty list)
    uint32_t *d_cnt = nullptr;       // [n_lists] postings of each list
    uint32_t *d_blk_list = nullptr;  // [n_blocks] list owning each block (0xFFFFFFFF: none of this view's lists)
    std::vector<uint32_t> h_blk_off; // host mirror of d_blk_off
    std::vector<uint32_t> h_cnt;     // host mirror of d_cnt (fetched when a small query first needs it)
    // per list: first_doc of its first and of its last block and its last doc (tile-height heuristic), fetched once
    struct ListSpan { uint32_t first_doc, last_block_first_doc, last_doc; };
    mutable std::mutex span_mu;             // contexts on different threads share the cache
    mutable std::unordered_map<uint64_t, ListSpan> span_cache;
    std::vector<uint32_t> h_spans;          // {first doc, first doc of the last block, last doc} per list, mirrored at creation (segments of <= SPAN_MIRROR_MAX lists)
    static constexpr uint64_t SPAN_MIRROR_MAX = 1u << 16;
};

namespace ii2 { constexpr uint32_t TOMB_SUM_SHIFT = 4; }    // docs per bit of a tombstone bitmap's summary: 1 << TOMB_SUM_SHIFT
namespace ii2 { constexpr uint32_t TOMB_PAD_WORDS = 4; }    // zero words every tombstone bitmap carries behind its n_words (ii2_tomb_create): a 16-byte load of its last word is legal

struct ii2_tomb {
    int device = 0;
    uint32_t *d_words = nullptr;
    uint32_t *d_summary = nullptr;   // bit g set <=> some doc of [g << TOMB_SUM_SHIFT, (g + 1) << TOMB_SUM_SHIFT) is removed (same allocation as d_words)
    uint64_t n_words = 0;   // bitmap covers doc ids [0, 32*n_words); TOMB_PAD_WORDS zero words follow
};

// a term dictionary resident in HBM: sorted, duplicate-free terms of one segment (made by align.hip, looked up by dict_find.hip)
struct ii2_dict {
    int device = 0;
    uint64_t n = 0, n_bytes = 0;
    uint8_t *d_bytes = nullptr;           // [n_bytes + 16]
    uint64_t *d_off = nullptr;            // [n + 1] byte offsets
    uint64_t *d_key = nullptr;            // [n] first 8 bytes, big-endian, zero padded
    uint32_t long_terms = 0;              // 1: some term is longer than 8 bytes (a tie of the keys does not decide)
    ~ii2_dict() {
        if (d_bytes) (void)hipFree(d_bytes);
        if (d_off) (void)hipFree(d_off);
        if (d_key) (void)hipFree(d_key);
    }
};

void ii2_comm_destroy_internal(ii2_ctx *ctx);
int ii2_seg_alloc_internal(ii2_ctx *ctx, uint64_t n_lists, uint64_t n_postings, uint64_t n_blocks, uint64_t n_bytes, ii2_seg **out, bool with_meta = false);   // ctx->mu held
int ii2_seg_rebase_internal(ii2_ctx *ctx, ii2_seg *seg, int world, const uint64_t *lo, const uint64_t *bo, const uint64_t *qo);            // ctx->mu held
// host helpers of every entry point
#define HIP_TRY(ctx, expr)                                                                 \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                \
            return II2_EHIP;                                                               \
        }                                                                                  \
    } while (0)

static inline int fail(ii2_ctx *ctx, int code, const char *msg) {
    if (ctx) ctx->err = msg;
    return code;
}
static inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// Workspace: ii2_ws_reserve the total up front (api.cpp; ctx->mu held), then carve it with ws_take
int ii2_ws_reserve(ii2_ctx *ctx, size_t bytes);
template <class T> static inline T *ws_take(ii2_ctx *ctx, size_t count) {
    T *p = (T *)(ctx->ws + ctx->ws_used);
    ctx->ws_used += align_up(count * sizeof(T));
    return p;
}

// temp device allocation freed at scope exit (cold paths only: encode / import / host calls)
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return ii2::dm_malloc_retry(&p, bytes ? bytes : 16); }
    template <class T> T *as() const { return (T *)p; }
};

void *ii2_pool_get(ii2_ctx *ctx, int slot, size_t bytes);      // grow-only ctx buffer `slot`, at least `bytes` (nullptr: out of memory); ctx->mu held
int ensure_debug(ii2_ctx *ctx, bool clear);                    // ctx->d_debug: option debug.stamps' cycle counters, made on first use (clear: zeroed first)
int ii2_seg_host_cnt(ii2_ctx *ctx, const ii2_seg *seg);       // fills seg->h_cnt on first use (thread-safe)
int ii2_seg_host_blk_off(ii2_ctx *ctx, const ii2_seg *seg);   // fills seg->h_blk_off on first use (thread-safe)
bool ii2_profile_pair(ii2_ctx *ctx, hipEvent_t *e0, hipEvent_t *e1);   // false when profiling is off
// a view over src's store whose four per-slot arrays were built on the device (align.hip); takes ownership of them
int ii2_seg_adopt_view(ii2_ctx *ctx, const ii2_seg *src, uint64_t n_out, uint32_t *d_blk_off, uint32_t *d_cnt, uint32_t *d_last_doc,
                       uint32_t *d_blk_list, ii2_seg **out);
int ii2_seg_encode_dev_unlocked(ii2_ctx *ctx, uint64_t n_lists, const uint64_t *d_post_off, const uint32_t *d_values,
                                uint64_t n_postings, ii2_seg **out);
int ii2_seg_decode_dev_unlocked(ii2_ctx *ctx, const ii2_seg *seg, uint64_t *d_post_off, uint32_t *d_values);
int ii2_seg_encode_stream_unlocked(ii2_ctx *ctx, uint64_t n_lists, const uint64_t *d_post_off, const uint32_t *d_values, uint64_t n_postings,
                                   uint64_t n_nonempty, uint64_t payload_bound, ii2_seg **out);

namespace ii2 {

// One posting list as the kernels see it: `skip` points at the list's first block entry;
// skip[nblk] is readable (next list's first block or the sentinel) and bounds the payload.
struct ListView {
    const ii2_skip *skip;
    const uint8_t *payload;
    const uint32_t *last_doc;    // the list's last doc id
    uint32_t nblk;
    uint32_t pad;
};

struct SegView {
    const uint32_t *blk_off;    // [n_terms+1] first block of each aligned term slot
    const ii2_skip *skip;
    const uint8_t *payload;
    const uint32_t *cnt;        // [n_terms] postings of each list (same indexing as blk_off)
    const uint32_t *blk_list;   // [n_blocks of the store] list that owns each block, in the segment's own numbering
    const uint32_t *last_doc;   // [n_terms] last doc id of each list (same indexing as blk_off)
    uint32_t list_base;         // blk_off / cnt point at this list of the segment (blk_list[b] - list_base = term slot)
    uint32_t pad;
};

constexpr uint32_t MAX_LISTS = II2_MAX_LISTS;

struct IntersectParams {
    ListView lists[MAX_LISTS];   // lists[0] is the driver (fewest blocks)
    uint32_t n_lists;
    uint32_t G;                  // driver blocks per tile
    uint32_t sparse_driver;      // host hint: most tiles will gallop (picks the kernel instantiation with the pipelined gallop)
    uint32_t sub;                // tiles per driver block (1; > 1 only with G == 1: tiny drivers are spread over more workgroups)
    uint32_t n_tiles;
    uint32_t tomb_nwords;
    const uint32_t *tomb;        // may be null
    uint32_t *ranges;            // [n_tiles][2 + 4*n_lists] tile doc range + per-list phase descriptors
    uint32_t *out;               // final ids
    uint64_t out_cap;
    uint32_t *tmp;               // per-tile slot of slot_words: result bitmap words or survivor id list
    uint32_t *tile_count;        // [n_tiles] survivors per tile (bit 31: the slot holds an id list)
    uint64_t *d_count;           // result count
    unsigned long long *debug;   // optional per-workgroup phase cycle counters [grid][8] (diagnostics)
    uint32_t *sums;              // [n_sums] partial sums of tile_count: per 64 tiles, then per 4096 tiles
    uint32_t n_sums, n_sums1;    // total entries, entries of the per-64 level
    uint32_t slot_words;
    uint32_t desc_words;         // words per tile in `ranges`
    uint32_t max_grid;           // workgroups of the tile kernel (each walks tiles w, w+grid, ...)
    uint32_t bitmap_mode;        // 1: very dense tiles use per-list bitmaps (option intersect.bitmap)
    uint32_t map_docs_per_block; // tiles with more docs per driver block than this take the gallop path (option intersect.map_docs)
    uint32_t op_union;           // 1: OR instead of AND — fixed doc-range tiles [u_base + t * u_span, ...], every list searched per tile
    uint32_t u_base, u_span, u_max;
};

// small AND / OR in one workgroup (setop_small.hip)
constexpr uint32_t SMALL_SET_POSTINGS = 8192;  // postings the lists may hold together ...
constexpr uint32_t SMALL_SET_BLOCKS = 128;     // ... in at most this many DV1 blocks
struct SmallSetParams {
    ListView lists[MAX_LISTS];   // non-empty lists, any order
    uint32_t blk_base[MAX_LISTS + 1];   // first block of each list in the concatenated block list
    uint32_t lpre[MAX_LISTS + 1];       // exclusive prefix of the lists' posting counts; lpre[n_lists] <= SMALL_SET_POSTINGS
    uint32_t n_lists;
    uint32_t n_blocks;           // <= SMALL_SET_BLOCKS
    uint32_t is_union;
    uint32_t tomb_nwords;
    const uint32_t *tomb;        // may be null
    uint32_t *out;
    uint64_t out_cap;
    uint64_t *d_count;
    uint32_t *sorted;            // [SMALL_SET_POSTINGS] scratch: every id at its rank
    uint32_t *ticket;            // zero between launches (the last workgroup resets it)
};
hipError_t launch_setop_small(const SmallSetParams &p, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);

// many small AND / OR queries in one launch (setop_batch.hip): the queries and their lists come from a device table
constexpr uint32_t BATCH_TINY_POSTINGS = 2048; // the 256-thread form: postings the lists of a query may hold together ...
constexpr uint32_t BATCH_TINY_BLOCKS = 32;     // ... in at most this many blocks (larger ones: SMALL_SET_POSTINGS / SMALL_SET_BLOCKS, 1024 threads)
constexpr uint64_t BATCH_MAX_QUERIES = 1u << 20;
struct BatchList {
    const ii2_skip *skip;        // the list's first block entry (skip[nblk] is readable)
    const uint8_t *payload;
    uint32_t nblk;               // > 0
    uint32_t cnt;                // its postings: 256 (nblk - 1) < cnt <= 256 nblk
};
struct BatchQuery {
    uint64_t stage_off;          // its slot of the staging buffer starts here ...
    uint32_t bound;              // ... and holds this many ids (AND: the shortest list, OR: all postings)
    uint32_t first_list;         // its lists: lists[first_list .. first_list + n_lists), all non-empty
    uint32_t n_lists;            // 1 .. MAX_LISTS
    uint32_t is_union;
    uint32_t slot;               // its word of the counts array (= its index in the caller's batch)
    uint32_t n_req;              // ii2_query_batch_groups: its required groups, 1 .. n_lists (ii2_query_batch: 0)
};
struct BatchParams {
    const BatchQuery *queries;   // [n_tiny + n_small], the tiny ones first
    const BatchList *lists;
    const uint32_t *tomb;        // may be null
    uint32_t tomb_nwords;
    uint32_t n_tiny, n_small;
    uint32_t *stage;
    uint32_t *cnt;               // [queries of the batch + 1]
};
struct BatchPackParams {
    const uint32_t *stage;
    const uint64_t *stage_off;   // [n_queries] every query's staging slot
    const uint64_t *off;         // [n_queries + 1] exclusive prefix of the counts
    uint32_t *out;
    uint64_t cap;
    uint32_t n_queries;
};
hipError_t launch_setop_batch(const BatchParams &p, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
constexpr uint32_t BATCH_FORM_TINY = 1u, BATCH_FORM_SMALL = 2u;
uint32_t setop_batch_forms(const BatchParams &p);      // the forms of the batch kernel that launch runs (BATCH_FORM_*)

// a short AND of ORs minus excluded lists in one workgroup (setop_groups.hip): the lists group by group, the required groups
// first (tags 0 .. n_req - 1), the lists of all excluded groups last (tag n_req)
constexpr uint64_t ANDNOT_SMALL_WORK = 32768;   // postings x lists up to which ii2_andnot_ranges takes it by default (setop.cpp: andnot_small)
struct GroupSetParams {
    ListView lists[MAX_LISTS];   // non-empty lists in tag order
    uint32_t blk_base[MAX_LISTS + 1];   // first block of each list in the concatenated block list
    uint32_t lpre[MAX_LISTS + 1];       // exclusive prefix of the lists' posting counts; lpre[n_lists] <= SMALL_SET_POSTINGS
    uint8_t tag[MAX_LISTS];      // the group of each list, ascending
    uint32_t n_lists;
    uint32_t n_blocks;           // <= SMALL_SET_BLOCKS
    uint32_t n_req;              // required groups, 1 .. n_lists
    uint32_t tomb_nwords;
    const uint32_t *tomb;        // may be null
    uint32_t *out;
    uint64_t out_cap;            // nothing is written when the result is longer
    uint64_t *d_count;
    uint32_t min_match;          // the threshold instantiation (ii2_atleast_ranges): required groups an id must lie in, 1 .. n_req
};
hipError_t launch_setop_groups(const GroupSetParams &p, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// the same kernel with the survive rule "in at least min_match required groups" instead of "in every one"
hipError_t launch_setop_groups_atleast(const GroupSetParams &p, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
hipError_t launch_batch_pack(const BatchPackParams &p, uint64_t max_bound, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);

// many short AND-of-ORs / NOT queries in one launch (setop_groups_batch.hip): the batch kernel's table (is_union unused), every
// query's lists in tag order as k_setop_groups takes them - the required groups first (tags 0 .. n_req - 1), the lists of all
// its excluded groups last (tag n_req) - and one tag byte per list of the table
struct GroupBatchParams {
    BatchParams b;
    const uint8_t *tag;          // [lists of the table]
};
hipError_t launch_setop_groups_batch(const GroupBatchParams &p, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
uint32_t setop_groups_batch_forms(const GroupBatchParams &p);      // the forms of its kernel that launch runs (BATCH_FORM_*)

// many short ranked queries in one launch (topk_batch.hip): the grouped batch's table - n_req the required groups with postings,
// bound = min(k, their postings) - plus, parallel to it, one weight byte per list (its group's; an excluded list's is unused)
// and min_score per query of the table.  The ranked ids go to stage + stage_off, their scores to stage_scores + stage_off, the
// count (at most bound) to cnt[slot] and the number of eligible docs to eligible[slot].
struct TopkBatchParams {
    GroupBatchParams g;
    const uint8_t *weight;       // [lists of the table]
    const uint32_t *min_score;   // [n_tiny + n_small], in the table's order
    uint32_t *stage_scores;
    uint32_t *eligible;          // [queries of the batch]
};
hipError_t launch_topk_batch(const TopkBatchParams &p, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);

// OR of a few medium-size lists by ranking (union_rank.hip)
constexpr uint32_t UNION_RANK_MAXL = 8;
constexpr uint32_t UNION_RANK_MAX_POSTINGS = 1u << 20;
struct UnionRankParams {
    ListView lists[UNION_RANK_MAXL];
    uint32_t blk_base[UNION_RANK_MAXL + 1];   // first block of each list in the concatenated block list
    uint32_t lpre[UNION_RANK_MAXL + 1];       // exclusive prefix of the lists' posting counts
    uint32_t n_lists;
    uint32_t n_blocks;
    uint32_t tomb_nwords;
    const uint32_t *tomb;        // may be null
    uint32_t *raw;               // [n_total] the lists decoded back to back
    uint32_t *sorted;            // [n_total] every id at its rank
    uint32_t *wg_cnt;            // survivors per 2048 ids
    uint32_t *out;
    uint64_t out_cap;
    uint64_t *d_count;
};
hipError_t launch_union_rank(const UnionRankParams &p, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);

// output offsets inside one launch (lookback.h): records {epoch : 24 | value : 40} in a buffer of the context's own
struct LookBack {
    unsigned long long *agg;     // [workgroups]
    unsigned long long *grp;     // [2 * ceil(workgroups / 64)]
    unsigned long long *err;     // = epoch when a bounded wait ran out
    uint32_t epoch;              // this launch's number, 1 .. 2^24 - 1
    uint32_t spin;               // polls a wait may take (0: default; or one of the two test values below)
};
constexpr uint32_t LB_GROUP = 64;                    // workgroups per group record
constexpr uint32_t LB_VALUE_BITS = 40;
constexpr unsigned long long LB_VALUE_MASK = (1ull << LB_VALUE_BITS) - 1ull;
constexpr uint32_t LB_EPOCH_MAX = (1u << (64u - LB_VALUE_BITS)) - 1u;
constexpr uint32_t LB_SPIN_EARLY = 0xFFFFFFFFu;     // tests: workgroup 1 gives up at once
constexpr uint32_t LB_SPIN_LATE = 0xFFFFFFFEu;      // tests: one workgroup gives up after the last one has stored the count (lookback.h)
// the protocol without a payload (lookback_check.hip: ii2_lookback_check).  Arrays indexed by g hold n_wg entries, the outputs one
// per launched workgroup (g - g_base)
constexpr uint32_t LB_CHECK_THREADS = 128;
constexpr uint32_t LB_CHECK_GAVE_UP_PREFIX = II2_LB_GAVE_UP_PREFIX, LB_CHECK_GAVE_UP_GROUP = II2_LB_GAVE_UP_GROUP;      // bits of state[]
constexpr uint32_t LB_CHECK_NO_PREFIX = II2_LB_NO_PREFIX;      // walk[] >> 24 when no prefix record ended the walk
struct LbCheckParams {
    LookBack lb;
    uint32_t n_wg, g_base;
    const unsigned long long *amount;   // [n_wg]
    const uint16_t *delay;              // [n_wg] or nullptr: units of s_sleep(16) before the publish
    unsigned long long *prefix;         // amounts before the workgroup (0 when its wait ran out)
    uint32_t *state;                    // 0, or which of its waits ran out
    uint32_t *walk;                     // windows of group records looked at | place of the prefix record used << 24
    uint32_t *polls;                    // rounds of loads lb_prefix took
};
hipError_t launch_lb_check(const LbCheckParams &p, hipStream_t s);

// dense streaming intersection (intersect_dense.hip)
constexpr uint32_t DENSE_MAXL = 4;             // lists it takes
constexpr uint32_t DENSE_CAPW = 16384;         // docs per LDS window of a wave
struct DenseParams {
    ListView lists[DENSE_MAXL];  // lists[0] is the driver (fewest blocks)
    uint32_t first_doc[DENSE_MAXL], last_doc[DENSE_MAXL];   // of every list (host copies: starting guess of the block search)
    uint32_t n_lists;
    uint32_t is_union;           // 1: OR of the lists (lists[0] = the list with the most blocks paces the rounds)
    uint32_t u_lo, u_hi;         // union: smallest first doc / largest last doc over all lists
    uint32_t bpw;                // driver blocks per wave (a multiple of 16)
    uint32_t n_waves;            // waves with work; the grid is ceil(n_waves / 4) workgroups
    uint32_t n_meta;             // entries of meta (4 per workgroup)
    uint32_t base32;             // first doc of the driver & ~31: origin of the result bitmap
    uint32_t tomb_nwords;
    const uint32_t *tomb;        // may be null
    uint32_t *bitmap;            // result bits; wave w's slot starts at word ((its first doc & ~31) - base32) / 32 + w
    uint4 *meta;                 // per wave {first doc & ~31, words, ids, -}
    uint32_t *wg_sum;            // ids per workgroup
    uint32_t *out;
    uint64_t out_cap;
    uint64_t *d_count;
    unsigned long long *debug;   // optional per-workgroup cycle counters [2048][8] (diagnostics)
    uint32_t debug_expand;       // the counters are the expand kernel's (option debug.stamps = 2), else the tile kernel's
    uint2 *hmask;                // two-list AND (intersect_and2.hip): one answer bit per posting of lists[0], 64 bits per lane of a wave
    LookBack lb;                 // ... in one launch (k_and2_fused): the output offsets come from a look-back; lb.agg == nullptr selects the two-kernel form
    float a_scale;               // blocks of lists[1] per doc and ...
    float b_dpb;                 // ... docs per block of lists[0]: where a wave's first probe of lists[1]'s skip table goes
    const uint32_t *a_bits;      // k_and2_fused: lists[1]'s dense form (bit d - a_origin <=> doc d), or null: the list is marked
    uint32_t a_origin;           // a multiple of 32
    uint32_t a_nwords;
    uint32_t and2_tiles;         // k_and2_fused with a dense form: tiles of sixteen lists[0] blocks a wave owns (2: the grid is half as many workgroups; else 1)
    const uint32_t *b_bits;      // k_and2_words: lists[0]'s dense form as well (null: one of the kernels above) ...
    uint32_t b_origin;           // a multiple of 32
    uint32_t b_nwords;
    uint32_t w_lo, w_n;          // ... and the window both forms cover, by and2_words_plan: its first word (doc >> 5) and its words (0: no common doc)
    uint32_t words_store;        // ... its id stores: 0 plain, 1 write-through at 16-byte alignment
    uint32_t words_early;        // ... chunk 0's stores leave before chunk 1 is staged (else both chunks are staged first)
};
hipError_t launch_intersect_dense(const DenseParams &p, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// AND of exactly two lists: lists[1] is marked, the postings of lists[0] are tested against it (meta = {first doc, last doc, ids, flags})
hipError_t launch_intersect_and2(const DenseParams &p, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// the kernel (sequence) those two launchers run for p: what they switch on and what setop.cpp records
Path intersect_dense_path(const DenseParams &p);
Path intersect_and2_path(const DenseParams &p);
// workgroups of the one-tile dense-form instance of k_and2_fused that a CU holds at once (occupancy query; 0: unknown)
uint32_t and2_fused_wgs_per_cu();
// both lists have a dense form (intersect_words.hip): sets p.w_lo / p.w_n and returns the workgroups of k_and2_words (>= 1: what
// the look-back records are prepared for); launch_intersect_and2 runs that kernel for a p with b_bits set
uint32_t and2_words_plan(DenseParams &p);
hipError_t launch_and2_words(const DenseParams &p, hipStream_t s);
// the dense form of list L: bits[0, n_words) (all zero before) get bit d - origin for every doc d of the list
hipError_t launch_dense_form_build(const ListView &L, uint32_t origin, uint32_t n_words, uint32_t *bits, hipStream_t s);

// OR of any number of lists, block by block (union_many.hip)
struct UmRange {
    const ii2_skip *skip;        // the range's segment
    const uint8_t *payload;
    const uint32_t *blk_list;
    const uint32_t *last_doc;
    uint32_t b0, b1;             // its blocks [b0, b1) ...
    uint32_t l0, l1;             // ... owned by its lists [l0, l1)
};
struct UnionManyParams {
    const UmRange *ranges;       // [n_ranges], none without blocks
    const uint32_t *pre;         // [n_ranges + 1] exclusive prefix of the ranges' blocks
    uint32_t n_ranges;
    uint32_t n_blocks;           // pre[n_ranges]
    uint32_t per_wave;           // query blocks per wave of the mark kernel
    uint32_t check_window;       // 1: several windows - the mark kernel skips blocks whose docs miss this one
    uint32_t win_lo;             // first doc of the window (a multiple of 32: word i <-> tombstone word win_lo / 32 + i)
    uint32_t win_docs;           // docs of the window (<= 2^30)
    uint32_t n_sum;              // summary words (each covers 64 x 32 bitmap words = 65536 docs)
    uint32_t window;             // index of the window: run[window & 1] = ids before it
    uint32_t *bitmap;            // [n_sum * 2048]
    uint32_t *summary;           // [n_sum]: bit c of word s <=> some bit of bitmap words (32 s + c) * 64 .. + 63
    uint32_t *cnt;               // [n_sum + 1] ids per summary word
    uint64_t *off;               // [n_sum + 1] their exclusive prefix
    uint64_t *run;               // [2]
    uint32_t *bounds;            // [2] k_um_bounds: smallest first doc, largest last doc
    const uint32_t *tomb;        // may be null
    uint32_t tomb_nwords;
    uint32_t write;              // 0: count and clear only
    uint32_t no_atomics;         // timing experiments (option debug.union_many_no_atomics): the mark kernel sets no bit (results wrong)
    uint32_t *out;
    uint64_t out_cap;
    uint64_t *d_count;
};
hipError_t launch_union_many_bounds(const UnionManyParams &p, hipStream_t s);
hipError_t launch_union_many_mark(const UnionManyParams &p, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
hipError_t launch_union_many_count(const UnionManyParams &p, uint32_t grid, hipStream_t s);
hipError_t launch_union_many_compact(const UnionManyParams &p, uint32_t grid, hipStream_t s);

// docs in at least m of n groups, counting form (atleast.hip): the bit-sliced counters behind the union's mark kernel
struct ThrParams {
    uint32_t *bitmap;            // the window's doc bitmap G [n_sum * 2048] and ...
    uint32_t *summary;           // ... its summary [n_sum], as UnionManyParams has them
    uint32_t *planes;            // [n_planes][plane_words]: plane b holds bit b of every doc's counter, laid out as the bitmap
    uint32_t *acc;               // [n_sum] the accumulated summary S_acc: the chunks some counter of which may be non-zero
    uint32_t plane_words;        // n_sum * 2048
    uint32_t n_sum;
    uint32_t n_planes;           // 1 .. THR_MAX_PLANES (atleast_count.h)
    uint32_t min_match;          // < 2^n_planes
    uint32_t late;               // k_thr_add: 1 = chunks that S_acc does not name are cleared, not added
};
hipError_t launch_thr_add(const ThrParams &p, uint32_t grid, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
hipError_t launch_thr_select(const ThrParams &p, uint32_t grid, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);

// the k docs in the most groups (topk.hip): the counting form's planes read as scores.  G, its summary, the planes and S_acc are
// ThrParams'; the classes of pass 2 are the scores cut_score .. cut_score + n_cls - 1
struct TopParams {
    uint32_t *bitmap;            // the window's doc bitmap G [n_sum * 2048]: the excluded docs
    uint32_t *summary;           // [n_sum] its summary
    uint32_t *planes;            // [n_planes][plane_words] the counters
    uint32_t *acc;               // [n_sum] S_acc: the chunks that hold a counter
    uint32_t plane_words;        // n_sum * 2048
    uint32_t n_sum;
    uint32_t n_planes;           // 1 .. THR_MAX_PLANES
    uint32_t min_match;          // k_top_hist: the lowest eligible score
    uint32_t clear;              // k_top_hist: 1 = it zeroes what it read (no pass 2 follows on these planes)
    uint32_t win_lo;             // first doc of the window (a multiple of 32: word i <-> tombstone word win_lo / 32 + i)
    uint32_t window;             // index of the window: run[window & 1] = docs per class before it
    uint32_t tomb_nwords;
    const uint32_t *tomb;        // may be null
    uint64_t *hist;              // [256] eligible docs per score, summed over the windows
    uint64_t *base;              // [256] k_top_base: eligible docs of a higher score
    uint32_t cut_score;          // pass 2: the lowest score returned ...
    uint32_t n_cls;              // ... and the number of classes from there up to the highest (0: k_top_emit only cleans up)
    uint64_t n_cut;              // docs of score cut_score returned
    uint64_t k;                  // entries of ids / scores
    uint32_t *cnt;               // [n_cls * n_sum + 1] docs per (class, summary word), class-major
    uint64_t *off;               // [n_cls * n_sum + 1] their exclusive prefix
    uint64_t *run;               // [2][256]
    uint32_t *ids;               // [k] the result, score descending, then id ascending
    uint32_t *scores;            // [k], may be null
};
// the weighted query's add (topk.hip: k_top_add): ThrParams' scratch, and the weight of the group just marked
struct TopAddParams {
    uint32_t *bitmap;            // the window's doc bitmap G [n_sum * 2048] and ...
    uint32_t *summary;           // ... its summary [n_sum]
    uint32_t *planes;            // [n_planes][plane_words] the counters
    uint32_t *acc;               // [n_sum] S_acc
    uint32_t plane_words;        // n_sum * 2048
    uint32_t n_sum;
    uint32_t n_planes;           // 1 .. THR_MAX_PLANES
    uint32_t weight;             // 1 .. 2^n_planes - 1: added to the counter of every doc in G
    uint32_t late;               // 1 = chunks that S_acc does not name are cleared, not added
};
hipError_t launch_top_add(const TopAddParams &p, uint32_t grid, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
hipError_t launch_top_hist(const TopParams &p, uint32_t grid, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
hipError_t launch_top_base(const TopParams &p, hipStream_t s);
hipError_t launch_top_count(const TopParams &p, uint32_t grid, hipStream_t s);
hipError_t launch_top_emit(const TopParams &p, uint32_t grid, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);

// AND of ORs over list ranges: the filters of the group path (intersect_ranges.hip)
constexpr uint32_t IR_PROBE_RUN = 256;          // consecutive candidates per wave of the probe
struct IrList {
    const ii2_skip *skip;        // the list's first block entry (skip[nblk] is readable)
    const uint8_t *payload;
    const uint32_t *last_doc;    // the list's last doc id
    uint32_t nblk;
    uint32_t lo, hi;             // its first and last doc, mirrored on the host; lo > hi: not mirrored (the kernel reads them)
    uint32_t pad;
};
struct IrParams {
    const uint32_t *cand;        // [n_cand] the candidates, ascending
    uint64_t n_cand;
    uint32_t *flag;              // [n_cand + 1] 1 = found in the group (flag[n_cand] = 0), then in place their exclusive scan
    uint32_t drop;               // 1: an exclusion - 1 = NOT found in the group (mark: the flags start at 1 and hits clear them)
    const IrList *lists;         // probe: the group's non-empty lists
    uint32_t n_lists;
    uint32_t win_lo, win_docs;   // mark: the window (win_lo a multiple of 32) ...
    uint32_t n_sum;              // ... its summary words ...
    uint32_t *bitmap;            // ... and the doc bitmap + summary it was marked into (UnionManyParams)
    uint32_t *summary;
    uint32_t *out;               // compact: the survivors, when all of them fit out_cap
    uint64_t out_cap;
    uint64_t *d_count;
};
hipError_t launch_ir_probe(const IrParams &p, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
hipError_t launch_ir_test(const IrParams &p, hipStream_t s);
hipError_t launch_ir_clear(const IrParams &p, uint32_t grid, hipStream_t s);
hipError_t launch_ir_compact(const IrParams &p, hipStream_t s);

// hits per list against a doc set (count_ranges.hip): the ranges' blocks as the block-wise OR walks them, one counter per list named
constexpr uint32_t CR_DECODED_SLOTS = 64;       // words the waves' decoded-block counts are spread over (one word takes ~90 atomics / us)
struct CountParams {
    const UmRange *ranges;       // [n_ranges], none without blocks
    const uint32_t *pre;         // [n_ranges + 1] exclusive prefix of the ranges' blocks
    const uint32_t *out_first;   // [n_ranges] counter of each range's first list
    uint32_t n_ranges;
    uint32_t n_blocks;           // pre[n_ranges]
    uint32_t per_wave;           // query blocks per wave of the count kernel
    uint32_t summary_skip;       // 1: a block whose docs meet no marked 2048-doc chunk is not decoded (option count.summary_skip)
    uint32_t win_lo;             // first doc of the window (a multiple of 32: word i <-> tombstone word win_lo / 32 + i)
    uint32_t win_docs;           // docs of the window (<= 2^30)
    uint32_t doc_lo, doc_hi;     // the docs of the window that can hit: it clipped to the set's and the lists' span (inclusive)
    uint32_t n_sum;              // summary words of the window
    uint32_t *bitmap;            // [n_sum * 2048] the per-context doc bitmap (UnionManyParams) ...
    uint32_t *summary;           // [n_sum] ... and its summary
    const uint32_t *set;         // [n_set] the doc set, ascending
    uint64_t n_set;
    const uint32_t *tomb;        // may be null
    uint32_t tomb_nwords;
    uint32_t pad;
    uint32_t *counts;            // [lists named] hits per list, accumulated over the windows
    uint32_t *decoded;           // [CR_DECODED_SLOTS] blocks decoded
    uint32_t *edges;             // [2] k_cr_edges: the set's first and last id
};
hipError_t launch_cr_edges(const CountParams &p, hipStream_t s);
hipError_t launch_cr_mark(const CountParams &p, hipStream_t s);
hipError_t launch_cr_count(const CountParams &p, bool every_doc, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);

// hits per (list, value bucket) (histogram.hip): the count's walk with a two-dimensional counter index.  The axis on the device:
// first[b] = the first id of bucket b, last = the inclusive last id of the last bucket (hist_device.h)
struct HistParams {
    CountParams c;               // the walk and the mark; counts = [lists named x n_buckets], list-major; decoded = [3 x CR_DECODED_SLOTS]:
                                 //     blocks decoded as WHOLE, as SPLIT, as WIDE; doc_lo / doc_hi clipped to the axis
    const uint32_t *first;       // [n_buckets]
    uint32_t n_buckets;          // 1 .. II2_HIST_MAX_BUCKETS
    uint32_t last;
    uint32_t whole;              // 0: a WHOLE block goes through the SPLIT sink (option hist.whole)
    uint32_t first0;             // first[0]
};
hipError_t launch_hs_count(const HistParams &p, bool every_doc, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// ii2_histogram_ids: c.set / n_set / tomb, counts = [n_buckets]
hipError_t launch_hs_ids(const HistParams &p, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);

// which groups each doc of an id array lies in (explain_ranges.hip): the count's walk with another sink - a hit ORs its group's bit
// into the row of its doc, which an open-addressing table of (id << 32 | row) entries finds (empty slots are all-ones)
constexpr uint64_t EX_EMPTY = ~0ull;
// the slot an id's probe starts at in a table of 1 << log2_slots entries, 1 <= log2_slots <= 31 (ii2_explain_slot)
__host__ __device__ static inline uint32_t ex_slot(uint32_t id, uint32_t log2_slots) { return (id * 0x9E3779B1u) >> (32u - log2_slots); }
struct ExplainParams {
    CountParams c;               // the walk and the mark: set = the ids (any order), out_first = the group of each range; counts, edges unused
    unsigned long long *table;   // [1 << log2_slots]
    unsigned long long *masks;   // [n_set * n_words] doc-major, zeroed by the host
    unsigned long long *hits;    // [CR_DECODED_SLOTS] mask bits that were clear when their hit set them
    uint32_t *span;              // [2] the ids' minimum (starts all-ones) and maximum (starts 0)
    uint32_t log2_slots;
    uint32_t n_words;            // mask words per doc
};
hipError_t launch_ex_prepare(const ExplainParams &p, hipStream_t s);
hipError_t launch_ex_match(const ExplainParams &p, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);

// the same for many short pages in one launch (explain_batch.hip): the batch kernels' table - every query's non-empty lists in
// group order, stage_off = the first word of its rows in masks, bound = its ids (<= II2_EXPLAIN_BATCH_IDS); tomb, stage, is_union
// and n_req unused - plus, parallel to it, the group number of every list and one ExplainBatchQuery per query of the table.  The
// rows are zero before the launch; cnt[slot] receives the query's hits.
struct ExplainBatchQuery {
    uint64_t ids_first;          // its page: ids[ids_first .. ids_first + bound)
    uint32_t n_words;            // mask words per row
    uint32_t pad;
};
struct ExplainBatchParams {
    BatchParams b;
    const uint32_t *grp;         // [lists of the table]
    const ExplainBatchQuery *pages;   // [n_tiny + n_small], in the table's order
    const uint32_t *ids;
    unsigned long long *masks;
};
hipError_t launch_explain_batch(const ExplainBatchParams &p, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);

}  // namespace ii2
int ii2_lookback_prepare(ii2_ctx *ctx, size_t n_wg, ii2::LookBack *lb);      // api.cpp; ctx->mu held
void ii2_lookback_forget(ii2_ctx *ctx);      // api.cpp: the context's stream is about to be destroyed
int ii2_lookback_launch(ii2_ctx *ctx, bool exclusive, const std::function<hipError_t()> &launch);      // api.cpp; ctx->mu held: kernels that wait between workgroups, ordered per device
int lb_note_pending(ii2_ctx *ctx);      // api.cpp: the error word as the asynchronous launches so far left it, copied behind them ...
void lb_fold_pending(ii2_ctx *ctx);     // ... and looked at once the stream has passed the copy (ii2_ctx_sync reports a give-up among them)
namespace ii2 {

constexpr size_t SELFTEST_SCRATCH = 64 * 4 * 1408;
hipError_t launch_selftest(uint32_t *d_fail, uint8_t *d_scratch, hipStream_t s);

// scans (scan.hip) — temp storage comes from the caller
size_t scan_temp_bytes(size_t n);
hipError_t scan_excl_u32(void *tmp, size_t tmp_bytes, const uint32_t *in, uint32_t *out, size_t n, hipStream_t s);
hipError_t scan3_excl(void *tmp, size_t tmp_bytes, const uint32_t *in0, uint64_t *out0, const uint32_t *in1, uint64_t *out1, const uint32_t *in2,
                      uint32_t *out2, size_t n, hipStream_t s);      // three scans of one length in the launches of one; tmp: 3 x scan_temp_bytes(n)
hipError_t scan_excl_u32_to_u64(void *tmp, size_t tmp_bytes, const uint32_t *in, uint64_t *out, size_t n, hipStream_t s);
hipError_t scan_excl_u32_to_u64_guarded(void *tmp, size_t tmp_bytes, const uint32_t *in, uint64_t *out, size_t n, const uint64_t *guard,
                                        uint64_t guard_max, hipStream_t s);
hipError_t scan_excl_u64(void *tmp, size_t tmp_bytes, const uint64_t *in, uint64_t *out, size_t n, hipStream_t s);

// codec
hipError_t launch_enc_list_blocks(const uint64_t *post_off, uint64_t n_lists, uint32_t *nblk, hipStream_t s);
hipError_t launch_enc_block_sizes(const uint64_t *post_off, const uint32_t *blk_off, uint64_t n_lists,
                                  const uint32_t *values, uint64_t n_blocks, uint32_t *sizes, ii2_skip *skip, hipStream_t s);
hipError_t launch_enc_write(const uint64_t *post_off, const uint32_t *blk_off, uint64_t n_lists,
                            const uint32_t *values, uint64_t n_blocks, const uint64_t *byte_off64,
                            ii2_skip *skip, uint8_t *payload, uint64_t n_postings, uint32_t *blk_list, hipStream_t s);
hipError_t launch_enc_stream(const uint64_t *post_off, const uint32_t *values, const uint32_t *blk_off, uint64_t n_lists, uint64_t n,
                             ii2_skip *skip, uint8_t *payload, uint64_t payload_cap, uint32_t *blk_list, uint32_t *part, uint64_t *d_result,
                             const LookBack &lb, unsigned long long *debug, hipStream_t s);      // part: [4 * enc_stream_workgroups(n)] scratch
uint64_t enc_stream_workgroups(uint64_t n);
hipError_t launch_enc_list_meta(const uint64_t *post_off, const uint32_t *values, uint64_t n_lists, uint32_t *cnt, uint32_t *last_doc, hipStream_t s);
hipError_t launch_dec_block_counts(const ii2_skip *skip, const uint8_t *payload, uint64_t n_blocks, uint32_t *counts, hipStream_t s);
hipError_t launch_dec_write(const ii2_skip *skip, const uint8_t *payload, uint64_t n_blocks, const uint64_t *bpo,
                            uint32_t *values, hipStream_t s);
hipError_t launch_gather_post_off(const uint32_t *blk_off, const uint64_t *bpo, uint64_t n_lists, uint64_t *post_off, hipStream_t s);
hipError_t launch_tomb_build(const uint32_t *removed, uint64_t n, uint32_t *words, uint64_t n_words, uint32_t *summary, hipStream_t s);
hipError_t launch_list_last_doc(const uint32_t *blk_off, const ii2_skip *skip, const uint8_t *payload, uint64_t n_lists, uint32_t *cnt, uint32_t *blk_list,
                                uint32_t *last_doc, hipStream_t s);
hipError_t launch_validate_counts(const uint32_t *blk_off, const uint32_t *blk_list, const ii2_skip *skip, const uint8_t *payload,
                                  uint64_t n_blocks, uint32_t *bad, hipStream_t s);
hipError_t launch_validate_seg(const uint32_t *blk_off, uint64_t n_lists, const ii2_skip *skip, uint64_t n_blocks, uint64_t n_bytes,
                               uint32_t *bad, hipStream_t s);
hipError_t launch_list_spans(const uint32_t *blk_off, const ii2_skip *skip, const uint32_t *last_doc, uint64_t n_lists, uint32_t *spans, hipStream_t s);
hipError_t launch_seg_rebase(uint32_t *blk_off, uint64_t n_lists, uint32_t add_blocks, ii2_skip *skip, uint64_t n_blocks, uint32_t add_bytes,
                             uint32_t *blk_list, uint32_t add_lists, hipStream_t s);
hipError_t launch_seg_close(uint32_t *blk_off_end, uint32_t n_blocks, ii2_skip *skip_end, uint32_t n_bytes, uint8_t *payload_end, uint32_t *blk_list_end, hipStream_t s);
hipError_t launch_sum_u32(const uint32_t *v, uint64_t n, uint64_t *out, hipStream_t s);
hipError_t launch_max_u32(const uint32_t *v, uint64_t n, uint32_t *out, hipStream_t s);

// intersect
constexpr uint32_t ISECT_GMAX = 16;         // driver blocks per tile (max)
constexpr uint32_t ISECT_SMAX = 16384;      // doc span a tile's LDS byte map can cover
hipError_t launch_intersect(const IntersectParams &p, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
Path intersect_tiles_path(const IntersectParams &p);      // the k_isect_tiles instantiation that launcher runs for p (what setop.cpp records)

// merge / union (merge.hip)
constexpr uint32_t MERGE_THREADS = 256;     // threads per workgroup of the tile kernel
constexpr uint32_t MERGE_CAP = 3584;        // postings a tile sorts in LDS (14 per thread)
constexpr uint32_t MERGE_NT_MAX = 256;      // terms per batch tile (one thread per term)
constexpr uint32_t MERGE_BM_WORDS = 2 * MERGE_CAP;          // LDS bitmap of a bitmap tile: the sort arrays' 56 KB
constexpr uint32_t MERGE_BM_DOCS = MERGE_BM_WORDS * 32u;    // docs a bitmap tile covers (229376)
// the k term-aligned inputs, by value in the kernel arguments
struct MergeSegs {
    SegView segs[MAX_LISTS];
    uint32_t k;
    uint32_t pad0;
    uint64_t n_terms;
};
static_assert(sizeof(MergeSegs) <= 4096, "MergeSegs travels through one pinned 4 KB block");

// direct placement of the merged postings (merge.hip): tile tickets, an error flag for bounded waits
struct MergeSync { uint32_t ticket, error, pad0, pad1; };

struct MergeParams {
    uint32_t k;
    uint32_t n_tiles_ub;          // host-side upper bound of the tile count (sizes grids and per-tile arrays)
    uint64_t n_terms;
    const uint32_t *tomb;
    const uint32_t *tomb_summary;  // 1 bit per (1 << TOMB_SUM_SHIFT) docs: most bit tests stop at this small, L2-resident array
    uint32_t tomb_nwords;
    uint32_t small_max;           // terms with more input postings get their own tiles (doc ranges)
    uint32_t range_target;        // input postings a range tile of a large term aims at
    uint32_t wmin;                // minimum packing weight of a term (bounds terms per batch)
    uint32_t batch_q;             // batch id = weight prefix / batch_q
    uint32_t bitmap_tiles;        // 1: dense terms are cut into bitmap tiles
    uint32_t bitmap_sparsity;     // ... when they hold at least one posting per this many docs
    uint32_t pad0;                // option debug.merge_skip (experiments / tests): phases left out, bit 6: the scanner never runs
    uint32_t spin_limit;          // polls a wait of the direct placement may take (0: default)
    uint32_t direct;              // 1: tiles go to their final place from inside the tile kernel (ticket order + scanner); 0: parking + packing pass
    MergeSync *sync;              // (zeroed by the host)
    uint64_t *tile_off;           // [n_tiles_ub + 1] output offset of every tile: written by the scanner (direct) or by the scan before the packing pass
    // per term (plan)
    uint32_t *tn;                 // [T+1] input postings
    uint32_t *tmin, *tmax;        // [T+1] smallest / largest doc id over the k lists
    uint32_t *tinfo;              // [T+1] longest list (bits 0-7), bit 8: bitmap tiles, bit 9: splitters uniform in doc space
    uint32_t *weight;             // [T+1] packing weight of a small term (0 for large terms)
    uint32_t *ntl;                // [T+1] tiles of a large term (0 for small terms)
    const uint64_t *npre;         // [T+1] exclusive prefix of tn: where a term's parking region starts
    const uint32_t *term_tile;    // [T+1] first tile of each term; [T] = number of tiles
    const uint32_t *n_tiles_dev;  // = term_tile + T
    // per tile
    uint4 *desc;                  // {t0, t1 | flags, dlo, dhi}
    uint4 *cut0;                  // [k * n_tiles_ub] where list s's part of the tile begins: {block | inside, payload byte, doc before, -} (merge.hip: cut_for)
    uint2 *cut1;                  // [k * n_tiles_ub] ... and where it ends: {block | inside, payload byte}
    uint32_t cut_ss, cut_st;      // entry of (list s, tile): s * cut_ss + tile * cut_st ([tile][s] for few lists, [s][tile] for many: the plan kernel's lanes then run along the tiles)
    uint32_t *term_alloc;         // [T] bump allocator inside a large term's parking region (zeroed by the host)
    uint32_t *tmp;                // parked survivors
    uint32_t *tile_count;         // [n_tiles_ub+1] survivors per tile (zeroed by the host)
    unsigned long long *tile_slot;   // [n_tiles_ub] where in tmp the tile parked them
    uint32_t *out_counts;         // [T] survivors per term (zeroed by the host)
    uint32_t *out_values;
    uint64_t out_cap;
    uint64_t *d_total;            // total survivors
    unsigned long long *debug;    // optional diagnostics words
    unsigned long long *events;   // [ME_COUNT] the context's event counters: every workgroup adds what it met, once, at its end
};
constexpr uint32_t MERGE_DESC_LARGE = 1u << 30;   // desc.y: the tile belongs to a large term (its count goes through tile_count)
constexpr uint32_t MERGE_DESC_BITMAP = 1u << 31;  // desc.y: bitmap tile

hipError_t launch_merge_plan_terms(const MergeSegs *ms, const MergeParams &p, hipStream_t s);
hipError_t launch_merge_init(uint64_t *mail, uint32_t n_mail_words64, uint32_t *cnt, uint64_t n_cnt, void *aux, uint64_t aux_bytes, uint64_t *tile_off,
                             uint64_t n_off, hipStream_t s);      // the call's clears in one launch (aux_bytes: a multiple of 4)
hipError_t launch_merge_heads(const MergeParams &p, const uint64_t *wpre, uint32_t *head, hipStream_t s);
hipError_t launch_merge_term_tile(const MergeParams &p, const uint32_t *head, const uint32_t *hpre, const uint32_t *lpre,
                                  uint32_t *term_tile, hipStream_t s);
hipError_t launch_merge_tile_desc(const MergeSegs *ms, const MergeParams &p, hipStream_t s);
hipError_t launch_merge_tile_runs(const MergeSegs *ms, const MergeParams &p, hipStream_t s);
hipError_t launch_merge_tiles(const MergeSegs *ms, const MergeParams &p, uint32_t grid, hipStream_t s);
hipError_t launch_merge_large_counts(const MergeParams &p, const uint64_t *tile_off, hipStream_t s);
hipError_t launch_merge_pack(const MergeParams &p, const uint64_t *tile_off, hipStream_t s);
hipError_t launch_count_nonzero(const uint32_t *v, uint64_t n, uint64_t *out, hipStream_t s, const uint32_t *err = nullptr, const uint32_t *n_tiles = nullptr,
                                uint64_t *mail = nullptr);      // mail: also mail[3] = *err (0 without), mail[4] = *n_tiles

}  // namespace ii2

// k SegViews over n_terms aligned term slots -> d_out_off (u64[n_terms+1], may be null), d_out_values (ops.cpp; ctx->mu held)
int merge_core(ii2_ctx *ctx, uint32_t k, const ii2::SegView *views, uint64_t n_terms, uint64_t blocks_ub, uint64_t postings_ub,
               const ii2_tomb *tomb, uint64_t *d_out_off, uint32_t *d_out_values, uint64_t out_cap, ii2_merge_stats *stats);
