// setop.cpp — AND / OR of posting lists (include/ii2.h): ii2_intersect(_async), ii2_union and their host-buffer forms.
// A call collects its lists once, then takes the first path of its chooser that fits:
//   AND: a list is empty (count 0), the small kernel (setop_small.hip), the dense forms - and2 in one launch, and2 in two
//        kernels (intersect_and2.hip), n-list dense (intersect_dense.hip) - then the tiles (intersect.hip).
//   OR:  the small kernel, rank (union_rank.hip), stream (intersect_dense.hip), the byte-map tiles (intersect.hip), then
//        the merge passes (ops.cpp: merge_core).
//   OR of list ranges (ii2_union_ranges): up to 64 non-empty lists the OR chooser above, more lists block by block
//        (union_many.hip).
//   AND of ORs over list ranges (ii2_intersect_ranges): no group, a group without blocks or groups whose doc spans do not
//        overlap (count 0, no launch); one group: the OR of list ranges; up to 64 groups of one non-empty list each whose
//        result surely fits: the AND chooser above (ii2_intersect); otherwise the group path - the OR of the group with the
//        fewest postings as candidates, then per further group a probe or mark filter (intersect_ranges.hip).
//   AND of ORs minus excluded groups (ii2_andnot_ranges): group_not == NULL: the call above.  No group (count 0); a required group
//        without blocks or required groups whose doc spans do not overlap (count 0, no launch); up to 64 non-empty lists of 8192
//        postings in 128 blocks, a result that surely fits: one launch (setop_groups.hip); otherwise the required groups through
//        the chooser above into a candidate array, then ONE exclusion pass over the excluded lists that reach the candidates'
//        span - the probe / mark filter with the flag turned round - or, without such a list, a copy.
//   At least m of n groups (ii2_atleast_ranges): no group or m above the n' required groups that have postings (count 0, no launch);
//        m = n': the call above on those groups, m = 1 without exclusion: the OR of list ranges (the hand-offs); the lists that
//        count fit one workgroup: one launch (setop_groups.hip, the threshold rule); otherwise the counting form - per window the
//        groups marked one by one (union_many.hip) and added into bit-sliced counters, compared with m (atleast.hip), then the
//        OR of list ranges' count, scan and compact.
//   Many AND / OR queries in one call (ii2_query_batch): the small ones in one launch per size class (setop_batch.hip), the
//        others one by one through the choosers above; all of them staged, then packed in query order.
//   Many AND-of-ORs / NOT queries in one call (ii2_query_batch_groups): every query an ii2_andnot_ranges call - those that fit
//        one workgroup in one launch per size class (setop_groups_batch.hip), the others one by one through that entry point's
//        paths; staged and packed by the same code as the flat batch.
//   Many ranked queries in one call (ii2_topk_batch): every query an ii2_topk_weighted_ranges call - those that fit one workgroup
//        in one launch per size class (topk_batch.hip), the others one by one through that entry point's form; ids and scores
//        staged and packed by the same code as the flat batch.
// The file is in that order, every section closed by its entry points (those of the AND and the OR chooser together, behind the
// OR section: each of the two is also called by the sections below), the helpers that several sections share in front.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "atleast_count.h"
#include "hist_device.h"
#include "internal.h"
#include "topk_batch_run.h"
#include "topk_count.h"

using namespace ii2;

namespace {
// one input list of a call: the kernels' view of it and where it lives
struct SetList {
    ListView v;
    const ii2_seg *seg;
    uint64_t idx;
};
// where a call's result goes
struct SetOut {
    const ii2_tomb *tomb;        // may be null
    uint32_t *d_out;
    uint64_t cap;
    uint64_t *d_count;
};
}  // namespace

// the kernels' view of list j of seg (its host block table is loaded)
static ListView list_view(const ii2_seg *seg, uint64_t j) {
    const uint32_t b0 = seg->h_blk_off[j], b1 = seg->h_blk_off[j + 1];
    return ListView{seg->d_skip + b0, seg->d_payload, seg->d_last_doc + j, b1 - b0, 0u};
}

// the lists' doc spans were mirrored on the host when the segment was created
static bool spans_mirrored(const ii2_seg *seg) { return seg->h_spans.size() == 3 * seg->n_lists; }

// every block of a list of c postings in nb blocks but its last is full (what the one-workgroup kernels' layout of the decoded
// blocks relies on)
static bool blocks_full(uint32_t nb, uint64_t c) { return c <= (uint64_t)nb * II2_DV1_BLOCK && c + II2_DV1_BLOCK > (uint64_t)nb * II2_DV1_BLOCK; }

// the n lists of a call, checked and viewed once (a union names every rejection "ii2_union: bad list")
static int collect_lists(ii2_ctx *ctx, bool is_union, uint32_t n, const ii2_seg *const *segs, const uint64_t *list_idx, SetList *L) {
    for (uint32_t i = 0; i < n; i++) {
        const ii2_seg *seg = segs[i];
        const uint64_t idx = list_idx ? list_idx[i] : 0;
        if (!seg || idx >= seg->n_lists) return fail(ctx, II2_EINVAL, is_union ? "ii2_union: bad list" : "list index out of range");
        if (seg->device != ctx->device) return fail(ctx, II2_EINVAL, is_union ? "ii2_union: bad list" : "segment lives on another device");
        if (int rc = ii2_seg_host_blk_off(ctx, seg)) return rc;
        L[i] = SetList{list_view(seg, idx), seg, idx};
    }
    return II2_OK;
}

// the tombstone fields, and with them the output fields, of every kernel's parameters
template <class P> static void set_tomb(P &p, const ii2_tomb *tomb) {
    p.tomb = tomb ? tomb->d_words : nullptr;
    p.tomb_nwords = tomb ? (uint32_t)std::min<uint64_t>(tomb->n_words, 0xFFFFFFFFull) : 0;
}
template <class P> static void set_out(P &p, const SetOut &o) {
    set_tomb(p, o.tomb);
    p.out = o.d_out;
    p.out_cap = o.cap;
    p.d_count = o.d_count;
}

// lists, blk_base and lpre of the kernels that decode the lists back to back (small set, rank); *np = their postings, or
// past `limit` as soon as a prefix of the lists is (no further count is fetched then)
template <class P> static int fill_concat(ii2_ctx *ctx, const SetList *L, uint32_t m, uint64_t limit, P &p, uint64_t *np) {
    uint32_t nb = 0;
    uint64_t sum = 0;
    for (uint32_t i = 0; i < m && sum <= limit; i++) {
        if (int rc = ii2_seg_host_cnt(ctx, L[i].seg)) return rc;
        p.lists[i] = L[i].v;
        p.blk_base[i] = nb;
        p.lpre[i] = (uint32_t)sum;
        nb += L[i].v.nblk;
        sum += L[i].seg->h_cnt[L[i].idx];
    }
    p.blk_base[m] = nb;
    p.lpre[m] = (uint32_t)sum;
    p.n_lists = m;
    p.n_blocks = nb;
    *np = sum;
    return II2_OK;
}

// first doc, first doc of the last block and last doc of a non-empty list: fetched once per (segment, list), then cached
static int list_span(ii2_ctx *ctx, const SetList &l, ii2_seg::ListSpan *out) {
    const ii2_seg *seg = l.seg;
    const uint64_t idx = l.idx;
    if (spans_mirrored(seg) && idx < seg->n_lists) {      // mirrored when the segment was created: no fetch, no sync
        *out = ii2_seg::ListSpan{seg->h_spans[3 * idx], seg->h_spans[3 * idx + 1], seg->h_spans[3 * idx + 2]};
        return II2_OK;
    }
    {
        std::lock_guard<std::mutex> sg(seg->span_mu);
        auto hit = seg->span_cache.find(idx);
        if (hit != seg->span_cache.end()) { *out = hit->second; return II2_OK; }
    }
    ii2_skip e[2];
    uint32_t last = 0;
    hipStream_t st = ctx->stream;
    took(ctx, P_SPAN_FETCH);
    HIP_TRY(ctx, hipMemcpyAsync(&e[0], l.v.skip, sizeof(ii2_skip), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(&e[1], l.v.skip + (l.v.nblk - 1), sizeof(ii2_skip), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(&last, l.v.last_doc, sizeof last, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *out = ii2_seg::ListSpan{e[0].first_doc, e[1].first_doc, last};
    std::lock_guard<std::mutex> sg(seg->span_mu);
    seg->span_cache[idx] = *out;
    return II2_OK;
}

// The grow-only per-context blocks.  A device block that holds `have` units and must hold `need`: the stream is waited for, the
// block freed and `want` >= need units of unit_bytes allocated (`err`: the text of II2_ENOMEM) ...
template <class T> static int grow_device(ii2_ctx *ctx, T **block, size_t *have, size_t need, size_t want, size_t unit_bytes, const char *err) {
    if (*have >= need) return II2_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (*block) (void)hipFree(*block);
    *block = nullptr;
    *have = 0;
    if (ii2::dm_malloc_retry((void **)block, want * unit_bytes) != hipSuccess) return fail(ctx, II2_ENOMEM, err);
    *have = want;
    return II2_OK;
}
// ... and a pinned one of `bytes` (a quarter more is taken); sync: the stream may still be copying from the old block
static int grow_pinned(ii2_ctx *ctx, void **block, size_t *cap, size_t bytes, bool sync, const char *err) {
    if (*cap >= bytes) return II2_OK;
    if (sync) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (*block) (void)hipHostFree(*block);
    *block = nullptr;
    *cap = 0;
    const size_t want = align_up(bytes + bytes / 4, 1 << 16);
    if (hipHostMalloc(block, want) != hipSuccess) return fail(ctx, II2_ENOMEM, err);
    *cap = want;
    return II2_OK;
}

// device-side address of a word of the pinned host mailbox (hipHostMalloc memory is mapped), or null if the runtime
// does not give one
static uint64_t *ii2_mapped_mail(ii2_ctx *ctx, uint32_t word) {
    if (!ctx->d_mail_mapped) {
        void *dp = nullptr;
        if (hipHostGetDevicePointer(&dp, ctx->h_mail, 0) != hipSuccess || !dp) { (void)hipGetLastError(); return nullptr; }
        ctx->d_mail_mapped = (uint64_t *)dp;
    }
    return ctx->d_mail_mapped + word;
}

// the count of a synchronous call: its kernels write it into the mapped mailbox word directly, or into d_mail, which is
// copied there (d_count: what the call was given); one stream synchronisation
static int read_count(ii2_ctx *ctx, const uint64_t *d_count, uint64_t *count) {
    if (d_count == ctx->d_mail)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_mail + II2_MAIL_COUNT, ctx->d_mail, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *count = ctx->h_mail[II2_MAIL_COUNT];
    return II2_OK;
}

// AND / OR of non-empty lists that hold <= SMALL_SET_BLOCKS blocks together: one single-workgroup kernel (setop_small.hip).
// *taken = false when the query is too large (or the path is switched off).
static int setop_small(ii2_ctx *ctx, bool is_union, const SetList *L, uint32_t n, const SetOut &o, bool *taken) {
    *taken = false;
    if (!ctx->opt_small_setop) return II2_OK;
    uint32_t nb = 0;
    for (uint32_t i = 0; i < n; i++) {             // by blocks first: no size is fetched for a query that is too large anyway
        if (L[i].v.nblk > SMALL_SET_BLOCKS - nb) return II2_OK;
        nb += L[i].v.nblk;
    }
    // an AND pays off below ~2k postings (the general path is four launches, ~14-20 us whatever the size); an OR up
    // to the kernel's capacity (the merge passes are ~40 launches)
    const uint64_t limit = is_union ? SMALL_SET_POSTINGS : SMALL_SET_POSTINGS / 4u;
    SmallSetParams sp;
    std::memset(&sp, 0, sizeof sp);
    uint64_t np = 0;
    if (int rc = fill_concat(ctx, L, n, limit, sp, &np)) return rc;
    if (np > limit) return II2_OK;
    sp.is_union = is_union ? 1u : 0u;
    set_out(sp, o);
    if (!ctx->d_small) {
        const size_t bytes = ((size_t)SMALL_SET_POSTINGS + 16) * sizeof(uint32_t);
        if (ii2::dm_malloc_retry((void **)&ctx->d_small, bytes) != hipSuccess) return fail(ctx, II2_ENOMEM, "small set-operation scratch allocation failed");
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_small, 0, bytes, ctx->stream));
    }
    sp.sorted = ctx->d_small;
    sp.ticket = ctx->d_small + (size_t)SMALL_SET_POSTINGS;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ii2_profile_pair(ctx, &e0, &e1);
    took(ctx, is_union ? P_OR_SMALL : P_AND_SMALL);
    HIP_TRY(ctx, launch_setop_small(sp, ctx->stream, e0, e1));
    *taken = true;
    return II2_OK;
}

// The streaming kernels' waves and workspace (intersect_dense.hip, intersect_and2.hip): dp.lists[0] paces the waves, bpw of
// its blocks each; the result bitmap covers the driver's docs (AND) or all lists' docs (OR), and2: one bit per posting of
// lists[0] instead.  dp.lists, first_doc / last_doc and the OR's fields are set.
static int dense_setup(ii2_ctx *ctx, DenseParams &dp, uint32_t bpw, bool and2, const SetOut &o) {
    const uint32_t lo = dp.is_union ? dp.u_lo : dp.first_doc[0], hi = dp.is_union ? dp.u_hi : dp.last_doc[0];
    dp.bpw = bpw;
    dp.n_waves = (dp.lists[0].nblk + bpw - 1) / bpw;
    const uint32_t grid = (dp.n_waves + 3u) / 4u;
    dp.n_meta = grid * 4u;
    dp.base32 = lo & ~31u;
    const uint64_t bm_words = and2 ? (uint64_t)dp.n_meta * 128u : (((uint64_t)hi - dp.base32) >> 5) + 1 + dp.n_meta + 8;
    size_t need = align_up(bm_words * sizeof(uint32_t)) + align_up((size_t)dp.n_meta * sizeof(uint4)) + align_up((size_t)grid * sizeof(uint32_t)) + 4096;
    if (int rc = ii2_ws_reserve(ctx, need)) return rc;
    dp.bitmap = ws_take<uint32_t>(ctx, bm_words);
    dp.hmask = and2 ? reinterpret_cast<uint2 *>(dp.bitmap) : nullptr;
    dp.meta = ws_take<uint4>(ctx, dp.n_meta);
    dp.wg_sum = ws_take<uint32_t>(ctx, grid);
    set_out(dp, o);
    return II2_OK;
}

// The tile kernel's descriptors, slots, counts and sums (intersect.hip) for p.n_tiles tiles of G driver blocks over
// p.n_lists lists.
static int tiles_setup(ii2_ctx *ctx, IntersectParams &p, uint32_t G, const SetOut &o) {
    const size_t dstride = 2 + 4 * (size_t)p.n_lists;
    p.desc_words = (uint32_t)dstride;
    p.slot_words = (std::max((ISECT_SMAX + 32u) / 32u, G * 256u) + 3u) & ~3u;
    size_t need = align_up((size_t)p.n_tiles * dstride * sizeof(uint32_t)) + align_up((size_t)p.n_tiles * p.slot_words * sizeof(uint32_t)) +
                  2 * align_up(((size_t)p.n_tiles + 2) * sizeof(uint32_t)) + align_up(((size_t)p.n_tiles / 64 + p.n_tiles / 4096 + 4) * sizeof(uint32_t)) + 4096;
    if (int rc = ii2_ws_reserve(ctx, need)) return rc;
    p.ranges = ws_take<uint32_t>(ctx, (size_t)p.n_tiles * dstride);
    p.tmp = ws_take<uint32_t>(ctx, (size_t)p.n_tiles * p.slot_words);
    p.tile_count = ws_take<uint32_t>(ctx, (size_t)p.n_tiles + 1);
    p.n_sums1 = p.n_tiles / 64 + 1;
    p.n_sums = p.n_sums1;
    p.sums = ws_take<uint32_t>(ctx, p.n_sums);
    const uint32_t wgs_default = 5u;    // LDS per workgroup: ~29 KB
    p.max_grid = (uint32_t)ctx->cu_count * (ctx->opt_intersect_wgs > 0 ? (uint32_t)ctx->opt_intersect_wgs : wgs_default);
    p.bitmap_mode = ctx->opt_intersect_bitmap ? 1u : 0u;
    set_out(p, o);
    return II2_OK;
}

// ---- AND ------------------------------------------------------------------------------------
// The dense form of l - a list of a one-launch two-list AND, whose docs are sp - into *out (bits stays null: the call reads the
// list's blocks as before), and into *meets_b whether criterion (b) holds for the list: the form's bytes are at most half the
// list's payload bytes (it must be clearly smaller than what it replaces).  Found in the store's cache, or made now when the
// policy allows it: FORM_BY_OPTION = as option intersect.dense_form says (1: where (b) holds, 2: whatever it says - tests),
// FORM_IF_B = where (b) holds and only there, not even a form that exists otherwise, FORM_ALWAYS = whatever (b) says.  The
// store's mutex is held from the look-up until the build kernel has FINISHED: a context on another thread that asks for the
// same list waits here and then reads a complete form, whatever its stream.  An allocation failure is not the query's: no form.
struct FormRef { const uint32_t *bits; uint32_t origin, n_words; };
enum FormPolicy { FORM_BY_OPTION, FORM_IF_B, FORM_ALWAYS };
static int dense_form_get(ii2_ctx *ctx, const SetList &l, const ii2_seg::ListSpan &sp, FormPolicy policy, FormRef *out, bool *meets_b) {
    *meets_b = false;
    ii2_seg_store *store = l.seg->store.get();
    if (!store || !ctx->opt_dense_form || sp.last_doc < sp.first_doc) return II2_OK;
    hipStream_t st = ctx->stream;
    std::lock_guard<std::mutex> fg(store->form_mu);
    const uint64_t key = l.seg->h_blk_off[l.idx];
    auto it = store->forms.find(key);
    if (it == store->forms.end()) {
        ii2_skip e[2];                                      // payload bytes: between the skip entries of the first and the one-past-last block
        HIP_TRY(ctx, hipMemcpyAsync(&e[0], l.v.skip, sizeof(ii2_skip), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(&e[1], l.v.skip + l.v.nblk, sizeof(ii2_skip), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        ii2_seg_store::DenseForm f;
        f.origin = sp.first_doc & ~31u;
        f.n_words = ((sp.last_doc - f.origin) >> 5) + 1u;
        f.payload_bytes = (uint64_t)(e[1].byte_off - e[0].byte_off);
        it = store->forms.emplace(key, f).first;
    }
    ii2_seg_store::DenseForm &f = it->second;
    const uint64_t bytes = (uint64_t)f.n_words * sizeof(uint32_t);
    const bool fits = 2 * bytes <= f.payload_bytes;
    *meets_b = fits;
    if (policy == FORM_IF_B && !fits) return II2_OK;
    if (!f.d_words) {
        if (policy == FORM_BY_OPTION && ctx->opt_dense_form != 2 && !fits) return II2_OK;
        uint32_t *w = nullptr;
        if (dm_alloc((void **)&w, bytes + 16) != hipSuccess) { (void)hipGetLastError(); return II2_OK; }      // (16-byte loads of the last words are legal)
        hipError_t e = hipMemsetAsync(w, 0, bytes + 16, st);
        if (e == hipSuccess) e = launch_dense_form_build(l.v, f.origin, f.n_words, w, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            dm_free(w);
            ctx->err = std::string("dense form: ") + hipGetErrorString(e);
            return II2_EHIP;
        }
        f.d_words = w;
        store->form_bytes += bytes + 16;
    }
    out->bits = f.d_words;
    out->origin = f.origin;
    out->n_words = f.n_words;
    return II2_OK;
}

// Both lists of a one-launch two-list AND as dense forms, ANDed word by word (intersect_words.hip; option intersect.and2_words:
// 0 never, 2 always - tests -, 1 = the rule).  That kernel reads two bitmaps where the present ones read one and the shorter
// list's payload: it moves less when the shorter list, too, meets criterion (b) - so (ii) both lists meet it, each on its own
// (whatever intersect.dense_form = 2 forces; the caller learns that from its one dense_form_get per list) - and a second form
// costs memory and a build, which pays on a pair large enough to be asked often: (iii), answered here, the shorter list holds
// at least intersect.and2_words_min blocks.  0 = CUs x workgroups of the one-tile instance per CU, by the occupancy query, x 16
// blocks: 16 384 on an MI355X, a quarter of what the present kernel takes in one round.  The word AND measured 8 - 15 % faster
// than the present kernel at 8 k, 16 k and 32 k blocks and 23 % at 130 k (DESIGN.md 4.1a', profiles/and2_words_threshold.txt);
// below 16 k blocks that is under a microsecond a query for a second form.  (i), the one-launch path and intersect.dense_form
// != 0, is the caller's and dense_form_get's.
static bool and2_words_large_enough(ii2_ctx *ctx, const SetList *L) {
    uint64_t min_blocks = ctx->opt_and2_words_min > 0 ? (uint64_t)ctx->opt_and2_words_min : 0u;
    if (!min_blocks) {
        if (ctx->and2_wgs_per_cu < 0) ctx->and2_wgs_per_cu = (int)and2_fused_wgs_per_cu();
        min_blocks = (uint64_t)ctx->cu_count * (uint64_t)ctx->and2_wgs_per_cu * 16u;
        if (!min_blocks) return false;                      // (the query failed: nothing to judge by)
    }
    return L[0].v.nblk >= min_blocks;
}

// Tiles a wave of the one-launch two-list AND owns when the longer list has a dense form (option intersect.and2_tiles: 1, 2, or
// 0 = this rule).  A workgroup's life there is a chain of waits that a second tile shares (intersect_and2.hip, k_and2_fused_x2):
// two tiles a wave halve the grid, each workgroup 1.7 times as long.  That pays when the one-tile grid - wgs
// workgroups - does not fit the device at once and so runs in rounds; a grid the device holds at once is one round already, and
// pairing its tiles would only halve the waves that hide each other's waits.  The device holds CUs x (workgroups of the one-tile
// instance per CU, by the occupancy query); option intersect.and2_slots puts a number in its place (tests).
static uint32_t and2_tiles_pick(ii2_ctx *ctx, uint32_t wgs) {
    if (ctx->opt_and2_tiles == 1 || ctx->opt_and2_tiles == 2) return (uint32_t)ctx->opt_and2_tiles;
    uint64_t slots = ctx->opt_and2_slots > 0 ? (uint64_t)ctx->opt_and2_slots : 0u;
    if (!slots) {
        if (ctx->and2_wgs_per_cu < 0) ctx->and2_wgs_per_cu = (int)and2_fused_wgs_per_cu();
        slots = (uint64_t)ctx->cu_count * (uint64_t)ctx->and2_wgs_per_cu;
    }
    return slots != 0u && wgs > slots ? 2u : 1u;
}

// Lists that are dense together (the headline 2-term query): every wave streams through its own run of driver blocks, no
// partition pass, no workgroup barriers (intersect_dense.hip).  L is sorted by blocks; per_block: docs per driver block.
static int intersect_dense(ii2_ctx *ctx, const SetList *L, uint32_t n, double per_block, const SetOut &o) {
    DenseParams dp;
    std::memset(&dp, 0, sizeof dp);
    for (uint32_t i = 0; i < n; i++) {
        dp.lists[i] = L[i].v;
        ii2_seg::ListSpan sp;
        if (int rc = list_span(ctx, L[i], &sp)) return rc;
        dp.first_doc[i] = sp.first_doc;
        dp.last_doc[i] = sp.last_doc;
    }
    dp.n_lists = n;
    // a wave's passes take 16 driver blocks each; one round (16 blocks) per wave by default: more, shorter waves balance
    // better than fewer, longer ones (measured on Zipf rank pairs 1/2 ... 2/3/5), and waves never wait for each other
    uint32_t bpw = ctx->opt_dense_bpw > 0 ? (uint32_t)ctx->opt_dense_bpw : 16u;
    bpw = std::min<uint32_t>(std::max<uint32_t>((bpw + 15u) & ~15u, 16u), 1024u);
    // two lists: the longer one is marked, the shorter one's postings are tested where they sit (intersect_and2.hip): the
    // hand-over to the second kernel is one bit per posting of the shorter list instead of a result bitmap
    const bool and2 = n == 2 && ctx->opt_intersect_and2 && bpw == 16u;
    if (int rc = dense_setup(ctx, dp, bpw, and2, o)) return rc;
    if (and2 && ctx->opt_intersect_and2 == 1) {
        const double spanA = (double)dp.last_doc[1] - (double)dp.first_doc[1] + 1.0;
        dp.a_scale = (float)((double)L[1].v.nblk / spanA);
        dp.b_dpb = (float)per_block;
        // the longer list as a cached bitmap where it has (or now gets) one: that instance of the kernel marks nothing; both
        // lists where option intersect.and2_words says so (the rule: and2_words_large_enough): that kernel reads no block at
        // all.  One look-up per list.  A form that cannot be had (an allocation failure): the call goes on with what it has
        const int64_t wmode = ctx->opt_dense_form ? ctx->opt_and2_words : 0;
        FormRef fa{}, fb{};
        bool a_meets_b = false, b_meets_b = false;
        if (int rcf = dense_form_get(ctx, L[1], ii2_seg::ListSpan{dp.first_doc[1], 0u, dp.last_doc[1]}, wmode == 2 ? FORM_ALWAYS : FORM_BY_OPTION, &fa, &a_meets_b))
            return rcf;
        if (fa.bits && (wmode == 2 || (wmode == 1 && a_meets_b && and2_words_large_enough(ctx, L))))
            if (int rcf = dense_form_get(ctx, L[0], ii2_seg::ListSpan{dp.first_doc[0], 0u, dp.last_doc[0]}, wmode == 2 ? FORM_ALWAYS : FORM_IF_B, &fb, &b_meets_b))
                return rcf;
        dp.a_bits = fa.bits; dp.a_origin = fa.origin; dp.a_nwords = fa.n_words;
        dp.b_bits = fb.bits; dp.b_origin = fb.origin; dp.b_nwords = fb.n_words;
        dp.words_store = ctx->opt_and2_words_store != 0 ? 1u : 0u;
        dp.words_early = ctx->opt_and2_words_order == 1 ? 1u : 0u;
        dp.and2_tiles = dp.a_bits ? and2_tiles_pick(ctx, dp.n_meta / 4u) : 1u;
        // one launch: the look-back records - one per workgroup of the kernel that runs - live in a buffer of their own (only
        // these kernels write it, every word tagged with its launch's number: nothing to clear between launches)
        const uint32_t wgs = dp.b_bits ? and2_words_plan(dp) : dp.n_meta / 4u;
        if (int rcl = ii2_lookback_prepare(ctx, wgs, &dp.lb)) return rcl;
        if (ctx->opt_and2_spin)
            dp.lb.spin = ctx->opt_and2_spin > 0 ? (uint32_t)std::min<int64_t>(ctx->opt_and2_spin, 0x7FFFFFFF) : ctx->opt_and2_spin == -2 ? LB_SPIN_LATE : LB_SPIN_EARLY;
    }
    if (ctx->opt_debug_stamps) {
        if (int rcd = ensure_debug(ctx, true)) return rcd;
        dp.debug = ctx->d_debug;
        dp.debug_expand = ctx->opt_debug_stamps == 2 ? 1u : 0u;
    }
    hipStream_t st = ctx->stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ii2_profile_pair(ctx, &e0, &e1);
    took(ctx, and2 ? intersect_and2_path(dp) : intersect_dense_path(dp));
    if (and2 && dp.lb.agg) {           // (the one-launch form waits between workgroups: one such kernel per device at a time)
        if (int rcq = ii2_lookback_launch(ctx, true, [&] { return launch_intersect_and2(dp, st, e0, e1); })) return rcq;
    } else {
        HIP_TRY(ctx, and2 ? launch_intersect_and2(dp, st, e0, e1) : launch_intersect_dense(dp, st, e0, e1));
    }
    return II2_OK;
}

static int intersect_unlocked(ii2_ctx *ctx, uint32_t n, const ii2_seg *const *segs, const uint64_t *list_idx, const SetOut &o) {
    if (n == 0 || n > MAX_LISTS || !segs || !o.d_count) return fail(ctx, II2_EINVAL, "ii2_intersect: bad argument");
    SetList L[MAX_LISTS];
    if (int rc = collect_lists(ctx, false, n, segs, list_idx, L)) return rc;
    for (uint32_t i = 0; i < n; i++) {
        if (L[i].v.nblk == 0) {
            HIP_TRY(ctx, hipMemsetAsync(o.d_count, 0, sizeof(uint64_t), ctx->stream));
            return II2_OK;
        }
    }
    if (!o.d_out) return fail(ctx, II2_EINVAL, "ii2_intersect: output buffer is NULL");
    if (ctx->opt_intersect_g <= 0) {
        bool taken = false;
        if (int rc = setop_small(ctx, false, L, n, o, &taken)) return rc;
        if (taken) return II2_OK;
    }
    std::stable_sort(L, L + n, [](const SetList &a, const SetList &b) { return a.v.nblk < b.v.nblk; });
    const uint32_t nblk0 = L[0].v.nblk;
    // tile height: aim the tile's doc span at the LDS byte map; keep >= ~8 tiles per CU
    uint32_t G = 1;
    double per_block_span = 0;                   // docs per driver block (tile-height heuristics)
    if (ctx->opt_intersect_g > 0) G = (uint32_t)std::min<int64_t>(ctx->opt_intersect_g, ISECT_GMAX);
    else if (nblk0 > 1) {
        ii2_seg::ListSpan ends;
        if (int rc = list_span(ctx, L[0], &ends)) return rc;
        const double per_block = (double)(ends.last_block_first_doc - ends.first_doc) / (double)(nblk0 - 1);
        per_block_span = per_block;
        const double g = per_block > 0 ? 0.85 * ISECT_SMAX / per_block : ISECT_GMAX;
        G = g >= ISECT_GMAX ? ISECT_GMAX : g < 1 ? 1u : (uint32_t)g;
        while (G > 1 && nblk0 / G < 8u * (uint32_t)ctx->cu_count) G >>= 1;
    }
    // the driver must be dense enough for the 1-bit-per-doc result bitmap to stay small next to the payload
    if (ctx->opt_intersect_dense && ctx->opt_intersect_g <= 0 && n >= 2 && n <= DENSE_MAXL && nblk0 >= 1024 &&
        per_block_span > 0 && per_block_span <= 1100.0)
        return intersect_dense(ctx, L, n, per_block_span, o);
    // a tiny sparse driver (a rare term against long lists) would keep only a handful of workgroups busy, each decoding
    // one block of the long list per candidate, one after the other: split its blocks over several tiles
    uint32_t sub = 1;
    if (n >= 2 && G == 1 && (per_block_span >= 8192.0 || (nblk0 == 1 && L[n - 1].v.nblk >= 64)) && ctx->opt_intersect_g <= 0) {
        const uint32_t want_tiles = (ctx->opt_intersect_subtiles > 0 ? (uint32_t)ctx->opt_intersect_subtiles : 4u) * (uint32_t)ctx->cu_count;
        if (nblk0 < want_tiles) sub = std::min<uint32_t>(ctx->opt_intersect_submax > 0 ? (uint32_t)ctx->opt_intersect_submax : 16u, (want_tiles + nblk0 - 1u) / nblk0);
    }
    IntersectParams p;
    std::memset(&p, 0, sizeof p);
    for (uint32_t i = 0; i < n; i++) p.lists[i] = L[i].v;
    p.n_lists = n;
    p.G = G;
    // the pipelined gallop pays when a driver block faces many blocks of a long list (candidates then hit distinct blocks)
    p.sparse_driver = ((per_block_span >= 8192.0 && L[n - 1].v.nblk / 16u >= nblk0) || sub > 1) ? 1u : 0u;
    p.sub = sub;
    p.n_tiles = ((nblk0 + G - 1) / G) * sub;
    if (int rc = tiles_setup(ctx, p, G, o)) return rc;
    // measured on 100M-doc Zipf pairs: the gallop path wins from ~32 docs per driver posting on (ranks 30/60: 80 -> 64 us),
    // the map tiles below that (ranks 10/20: 78 vs 100 us)
    p.map_docs_per_block = ctx->opt_intersect_map_docs > 0 ? (uint32_t)ctx->opt_intersect_map_docs : 8192u;
    if (ctx->opt_debug_stamps) {
        if (int rcd = ensure_debug(ctx, false)) return rcd;
        p.debug = ctx->d_debug;
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ii2_profile_pair(ctx, &e0, &e1);
    took(ctx, intersect_tiles_path(p));
    HIP_TRY(ctx, launch_intersect(p, ctx->stream, e0, e1));
    return II2_OK;
}

// ii2_intersect with ctx->mu held (ii2_intersect_ranges hands single-list groups to it)
static int intersect_sync(ii2_ctx *ctx, uint32_t n, const ii2_seg *const *segs, const uint64_t *list_idx, const ii2_tomb *tomb, uint32_t *d_out,
                          uint64_t cap, uint64_t *count) {
    // the count lands in the pinned host mailbox directly (the kernels write it once, at their end): one stream
    // synchronisation, no copy behind it
    uint64_t *d_cnt = ii2_mapped_mail(ctx, II2_MAIL_COUNT);
    const SetOut o{tomb, d_out, cap, d_cnt ? d_cnt : ctx->d_mail};
    if (int rcn = lb_note_pending(ctx)) return rcn;       // (the give-ups of asynchronous launches before this one stay reported)
    int rc = intersect_unlocked(ctx, n, segs, list_idx, o);
    if (rc) return rc;
    const uint32_t own = ctx->lb_pending;           // epoch of this call's one-launch AND (0: it took another path)
    ctx->lb_pending = 0;
    if (own) HIP_TRY(ctx, hipMemcpyAsync(ctx->h_mail + II2_MAIL_LB_OWN, ctx->d_lb, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = read_count(ctx, o.d_count, count))) return rc;
    lb_fold_pending(ctx);
    if (own && (*count == ~0ull || ctx->h_mail[II2_MAIL_LB_OWN] == own)) {
        // a bounded wait of the one-launch two-list AND ran out (its workgroups did not start in index order; the count is all
        // ones, or looks valid when the workgroup gave up after the last one had stored it): nothing is wrong with the inputs —
        // the same query again through the two-kernel form, which has no inter-workgroup waits
        ctx->lb_fallbacks++;
        const int64_t keep = ctx->opt_intersect_and2;
        ctx->opt_intersect_and2 = 2;
        rc = intersect_unlocked(ctx, n, segs, list_idx, o);
        ctx->opt_intersect_and2 = keep;
        if (rc) return rc;
        if ((rc = read_count(ctx, o.d_count, count))) return rc;
    }
    if (*count > cap) return fail(ctx, II2_ECAPACITY, "ii2_intersect: result does not fit the output buffer (content unspecified)");
    return II2_OK;
}

// ---- OR -------------------------------------------------------------------------------------
// Few long lists, the longest one dense: the streaming kernel of the dense intersection with OR semantics - every wave
// walks its own run of blocks of the longest list (the pacer), the other lists mark into the same bitmap
// (intersect_dense.hip).  The lists' ends are cached per (segment, list): no host sync after the first use.
static int union_stream(ii2_ctx *ctx, const SetList *L, uint32_t m, const SetOut &o, bool *taken) {
    uint32_t pace = 0;
    for (uint32_t i = 1; i < m; i++) if (L[i].v.nblk > L[pace].v.nblk) pace = i;
    if (L[pace].v.nblk < 1024) return II2_OK;
    DenseParams dp;
    std::memset(&dp, 0, sizeof dp);
    uint32_t u_lo = 0xFFFFFFFFu, u_hi = 0;
    ii2_seg::ListSpan psp{};
    for (uint32_t i = 0, at_next = 1; i < m; i++) {
        ii2_seg::ListSpan sp;
        if (int rc = list_span(ctx, L[i], &sp)) return rc;
        const uint32_t at = i == pace ? 0u : at_next++;
        dp.lists[at] = L[i].v;
        dp.first_doc[at] = sp.first_doc;
        dp.last_doc[at] = sp.last_doc;
        if (i == pace) psp = sp;
        u_lo = std::min(u_lo, sp.first_doc);
        u_hi = std::max(u_hi, sp.last_doc);
    }
    const double per_block = (double)(psp.last_block_first_doc - psp.first_doc) / (double)(dp.lists[0].nblk - 1);
    // the stretches before the pacer's first and after its last doc are one wave's work each: keep them short
    const uint64_t own = (uint64_t)psp.last_doc - psp.first_doc + 1, all = (uint64_t)u_hi - u_lo + 1;
    if (!(per_block > 0 && per_block <= 1100.0 && all <= own + own / 4 + 65536)) return II2_OK;
    dp.n_lists = m;
    dp.is_union = 1u;
    dp.u_lo = u_lo;
    dp.u_hi = u_hi;
    if (int rc = dense_setup(ctx, dp, 16u, false, o)) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ii2_profile_pair(ctx, &e0, &e1);
    took(ctx, intersect_dense_path(dp));
    HIP_TRY(ctx, launch_intersect_dense(dp, ctx->stream, e0, e1));
    *taken = true;
    return II2_OK;
}

// OR of the lists through the set-op kernels; *taken = false when none fits (the caller merges instead)
static int union_unlocked(ii2_ctx *ctx, const SetList *all, uint32_t n, const SetOut &o, bool *taken) {
    *taken = false;
    if (!ctx->opt_union_dense) return II2_OK;
    SetList L[MAX_LISTS];        // the non-empty lists
    uint32_t m = 0;
    uint64_t total_blocks = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (all[i].v.nblk == 0) continue;
        L[m++] = all[i];
        total_blocks += all[i].v.nblk;
    }
    if (int rc = setop_small(ctx, true, L, m, o, taken)) return rc;
    if (*taken) return II2_OK;
    // a few lists of medium size: decode, rank every id by bisection in the other lists, filter, write (union_rank.hip)
    if (ctx->opt_union_rank && m <= UNION_RANK_MAXL && total_blocks <= UNION_RANK_MAX_POSTINGS / II2_DV1_BLOCK + m) {
        UnionRankParams up;
        std::memset(&up, 0, sizeof up);
        uint64_t np = 0;
        if (int rc = fill_concat(ctx, L, m, ~0ull, up, &np)) return rc;
        if (np <= UNION_RANK_MAX_POSTINGS) {
            const uint32_t nwg = (uint32_t)((np + 2047) / 2048);
            const size_t need = 2 * align_up(np * sizeof(uint32_t)) + align_up(((size_t)nwg + 1) * sizeof(uint32_t)) + 4096;
            if (int rc = ii2_ws_reserve(ctx, need)) return rc;
            up.raw = ws_take<uint32_t>(ctx, np);
            up.sorted = ws_take<uint32_t>(ctx, np);
            up.wg_cnt = ws_take<uint32_t>(ctx, (size_t)nwg + 1);
            set_out(up, o);
            hipEvent_t e0 = nullptr, e1 = nullptr;
            ii2_profile_pair(ctx, &e0, &e1);
            took(ctx, P_OR_RANK);
            HIP_TRY(ctx, launch_union_rank(up, ctx->stream, e0, e1));
            *taken = true;
            return II2_OK;
        }
    }
    if (total_blocks < 64) return II2_OK;
    if (ctx->opt_union_stream && m >= 2 && m <= DENSE_MAXL) {
        if (int rc = union_stream(ctx, L, m, o, taken)) return rc;
        if (*taken) return II2_OK;
    }
    // Lists dense TOGETHER (>= 1 posting per 16 docs of their common range): the byte-map tiles of the intersection with OR
    // semantics over fixed doc ranges - no decode-to-raw, no fold, ~20x the merge path's rate.  The common doc range comes
    // from the lists' cached ends (one round trip per list the first time it is used, none after).
    uint32_t mm[2] = {0xFFFFFFFFu, 0u};
    for (uint32_t i = 0; i < m; i++) {
        ii2_seg::ListSpan sp;
        if (int rc = list_span(ctx, L[i], &sp)) return rc;
        mm[0] = std::min(mm[0], sp.first_doc);
        mm[1] = std::max(mm[1], sp.last_doc);
    }
    if (mm[1] < mm[0]) return II2_OK;
    constexpr uint32_t S = ISECT_SMAX - 64u;               // tile span: a multiple of 32 below the byte-map size
    const uint32_t base = mm[0] & ~31u;
    const uint64_t span = (uint64_t)mm[1] - base + 1;
    if (total_blocks * II2_DV1_BLOCK * (uint64_t)ctx->opt_union_sparsity < span) return II2_OK;       // too sparse (the tile count grows with the span): the merge passes do better
    const uint64_t n_tiles = (span + S - 1) / S;
    if (n_tiles >= (1ull << 24)) return II2_OK;
    IntersectParams p;
    std::memset(&p, 0, sizeof p);
    for (uint32_t i = 0; i < m; i++) p.lists[i] = L[i].v;
    p.n_lists = m;
    p.op_union = 1u;
    p.sub = 1u;
    p.u_base = base;
    p.u_span = S;
    p.u_max = mm[1];
    p.n_tiles = (uint32_t)n_tiles;
    if (int rc = tiles_setup(ctx, p, 1u, o)) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ii2_profile_pair(ctx, &e0, &e1);
    took(ctx, intersect_tiles_path(p));
    HIP_TRY(ctx, launch_intersect(p, ctx->stream, e0, e1));
    *taken = true;
    return II2_OK;
}

// OR of n collected lists (blocks_ub > 0 blocks in all) through the chooser, else the merge passes; ctx->mu held
static int union_lists(ii2_ctx *ctx, const SetList *L, uint32_t n, uint64_t blocks_ub, const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap,
                       uint64_t *count) {
    uint64_t *d_cnt = ii2_mapped_mail(ctx, II2_MAIL_COUNT);      // the count goes straight into the pinned host mailbox
    const SetOut o{tomb, d_out, cap, d_cnt ? d_cnt : ctx->d_mail};
    bool taken = false;
    if (int rc = union_unlocked(ctx, L, n, o, &taken)) return rc;
    if (taken) {
        if (int rc = read_count(ctx, o.d_count, count)) return rc;
        if (*count > cap) return fail(ctx, II2_ECAPACITY, "ii2_union: result does not fit the output buffer (content unspecified)");
        return II2_OK;
    }
    // the merge passes over one-term views of the segments: blk_off shifted to the list
    SegView views[MAX_LISTS];
    for (uint32_t i = 0; i < n; i++) {
        const ii2_seg *s = L[i].seg;
        const uint64_t li = L[i].idx;
        views[i] = SegView{s->d_blk_off + li, s->d_skip, s->d_payload, s->d_cnt + li, s->d_blk_list, s->d_last_doc + li, (uint32_t)li, 0u};
    }
    ii2_merge_stats st;
    std::memset(&st, 0, sizeof st);
    took(ctx, P_OR_MERGE);
    if (int rc = merge_core(ctx, n, views, 1, blocks_ub, blocks_ub * II2_DV1_BLOCK, tomb, nullptr, d_out, cap, &st)) {
        if (rc == II2_ECAPACITY) *count = ctx->h_mail[0];      // the size needed, as on the chooser's paths (merge_core has just read it)
        return rc;
    }
    *count = st.n_out;
    return II2_OK;
}

// ---- the entry points of the two choosers ------------------------------------------------------
extern "C" {

int ii2_intersect_async(ii2_ctx *ctx, uint32_t n, const ii2_seg *const *segs, const uint64_t *list_idx,
                        const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap, uint64_t *d_count) {
    if (!ctx) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return intersect_unlocked(ctx, n, segs, list_idx, SetOut{tomb, d_out, cap, d_count});
}

int ii2_intersect(ii2_ctx *ctx, uint32_t n, const ii2_seg *const *segs, const uint64_t *list_idx,
                  const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap, uint64_t *count) {
    if (!ctx || !count) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return intersect_sync(ctx, n, segs, list_idx, tomb, d_out, cap, count);
}

int ii2_union(ii2_ctx *ctx, uint32_t n, const ii2_seg *const *segs, const uint64_t *list_idx, const ii2_tomb *tomb,
              uint32_t *d_out, uint64_t cap, uint64_t *count) {
    if (!ctx || !count) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n == 0 || n > MAX_LISTS || !segs) return fail(ctx, II2_EINVAL, "ii2_union: list count must be 1..64");
    SetList L[MAX_LISTS];
    if (int rc = collect_lists(ctx, true, n, segs, list_idx, L)) return rc;
    uint64_t blocks_ub = 0;
    for (uint32_t i = 0; i < n; i++) blocks_ub += L[i].v.nblk;
    if (!blocks_ub) { *count = 0; return II2_OK; }
    if (!d_out) return fail(ctx, II2_EINVAL, "ii2_union: output buffer is NULL");
    return union_lists(ctx, L, n, blocks_ub, tomb, d_out, cap, count);
}

}  // extern "C"

// ---- OR of list ranges ------------------------------------------------------------------------
// one range of a call, checked: lists [l0, l1) of seg own its blocks [b0, b1)
struct RangeIn {
    const ii2_seg *seg;
    uint64_t l0, l1;
    uint32_t b0, b1;
};

// docs per window of the block-wise paths (option union.many_window_log2)
static uint64_t um_window(const ii2_ctx *ctx) {
    return 1ull << std::min<int64_t>(std::max<int64_t>(ctx->opt_union_many_window_log2, 11), 30);
}

// the per-context doc bitmap - and the counter planes of ii2_atleast_ranges - are all-zero between calls: a call that stopped
// half-way (its copy from the staging block may still be pending, its marks are still set) is cleaned up by the next one
static int um_scratch_clean(ii2_ctx *ctx) {
    if (!ctx->um_dirty) return II2_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->d_um_bits) HIP_TRY(ctx, hipMemsetAsync(ctx->d_um_bits, 0, ctx->um_bits_words * sizeof(uint32_t), ctx->stream));
    if (ctx->d_thr) HIP_TRY(ctx, hipMemsetAsync(ctx->d_thr, 0, ctx->thr_words * sizeof(uint32_t), ctx->stream));
    ctx->um_dirty = false;
    return II2_OK;
}

// ... and holds the bitmap + summary of the largest window of a doc span (grow-only, zeroed when it grows)
static int um_scratch_reserve(ii2_ctx *ctx, const char *who, uint64_t span, uint64_t W) {
    const uint64_t n_sum_call = (std::min(span, W) + 65535) / 65536;
    const size_t words = n_sum_call * 2048 + n_sum_call;
    if (ctx->um_bits_words >= words) return II2_OK;
    if (int rc = grow_device(ctx, &ctx->d_um_bits, &ctx->um_bits_words, words, words, sizeof(uint32_t), (std::string(who) + ": scratch allocation failed").c_str()))
        return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_um_bits, 0, words * sizeof(uint32_t), ctx->stream));
    return II2_OK;
}

// The ranges [0, n) of segs / list_first / list_end, checked (`who` names the entry point in the messages); those that own
// blocks are appended to rs.  *n_blocks, *n_nonempty grow by their blocks and non-empty lists.
static int collect_ranges(ii2_ctx *ctx, const char *who, uint64_t n, const ii2_seg *const *segs, const uint64_t *list_first,
                          const uint64_t *list_end, std::vector<RangeIn> &rs, uint64_t *n_blocks, uint64_t *n_nonempty) {
    for (uint64_t i = 0; i < n; i++) {
        const ii2_seg *seg = segs[i];
        const uint64_t l0 = list_first[i], l1 = list_end[i];
        if (!seg || l0 > l1 || l1 > seg->n_lists || seg->device != ctx->device) return fail(ctx, II2_EINVAL, (std::string(who) + ": bad range").c_str());
        if (l0 == l1) continue;
        if (int rc = ii2_seg_host_blk_off(ctx, seg)) return rc;
        // the lists [l0, l1) must own the consecutive blocks blk_off[l0] .. blk_off[l1] (views skip only empty lists between
        // selected ones): checked, not assumed
        const std::vector<uint32_t> &bo = seg->h_blk_off;
        for (uint64_t j = l0; j < l1; j++) {
            if (bo[j + 1] < bo[j]) return fail(ctx, II2_EINVAL, (std::string(who) + ": the segment's list table does not ascend").c_str());
            *n_nonempty += bo[j + 1] > bo[j] ? 1u : 0u;
        }
        if (bo[l1] > seg->n_blocks) return fail(ctx, II2_EINVAL, (std::string(who) + ": the segment's list table does not ascend").c_str());
        if (bo[l1] == bo[l0]) continue;
        rs.push_back(RangeIn{seg, l0, l1, bo[l0], bo[l1]});
        *n_blocks += bo[l1] - bo[l0];
    }
    return II2_OK;
}

// the block-wise descriptors of rs[r0, r1) (union_many.hip): UmRange[r1 - r0], then the exclusive block prefix [r1 - r0 + 1]
static size_t um_desc_bytes(size_t nr) { return align_up(nr * sizeof(UmRange)) + align_up((nr + 1) * sizeof(uint32_t)); }
static void um_desc_fill(const std::vector<RangeIn> &rs, size_t r0, size_t r1, uint8_t *h) {
    const size_t nr = r1 - r0;
    UmRange *hr = (UmRange *)h;
    uint32_t *hpre = (uint32_t *)(h + align_up(nr * sizeof(UmRange)));
    uint32_t acc = 0;
    for (size_t r = 0; r < nr; r++) {
        const RangeIn &q = rs[r0 + r];
        const ii2_seg *s = q.seg;
        hr[r] = UmRange{s->d_skip, s->d_payload, s->d_blk_list, s->d_last_doc, q.b0, q.b1, (uint32_t)q.l0, (uint32_t)q.l1};
        hpre[r] = acc;
        acc += q.b1 - q.b0;
    }
    hpre[nr] = acc;
}

// the window fields of the block-wise paths' parameters: `docs` docs from wlo on, in the per-context bitmap + summary
static void um_set_window(const ii2_ctx *ctx, UnionManyParams &p, uint64_t wlo, uint64_t docs) {
    p.win_lo = (uint32_t)wlo;
    p.win_docs = (uint32_t)docs;
    p.n_sum = (uint32_t)((docs + 65535) / 65536);
    p.bitmap = ctx->d_um_bits;
    p.summary = ctx->d_um_bits + (size_t)p.n_sum * 2048;
}
// query blocks per wave of the mark kernel
static uint32_t um_per_wave(const ii2_ctx *ctx, uint64_t n_blocks) {
    const uint64_t target_waves = (uint64_t)ctx->cu_count * 32u;
    return (uint32_t)std::max<uint64_t>(1, (n_blocks + target_waves - 1) / target_waves);
}

// the doc span of the ranges' non-empty lists from the segments' mirrored spans; false when a segment has none (the caller then
// reduces over the blocks: k_um_bounds)
static bool mirrored_span(const std::vector<RangeIn> &rs, uint32_t *lo, uint32_t *hi) {
    for (const RangeIn &q : rs) {
        const ii2_seg *s = q.seg;
        if (!spans_mirrored(s)) return false;
        for (uint64_t j = q.l0; j < q.l1; j++) {
            if (s->h_blk_off[j + 1] == s->h_blk_off[j]) continue;
            *lo = std::min(*lo, s->h_spans[3 * j]);
            *hi = std::max(*hi, s->h_spans[3 * j + 2]);
        }
    }
    return true;
}

// The block-wise OR (union_many.hip) of the ranges' blocks: per window of the doc range mark, count, scan, compact.
static int union_many(ii2_ctx *ctx, const std::vector<RangeIn> &rs, uint64_t n_blocks, const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap,
                      uint64_t *count) {
    hipStream_t st = ctx->stream;
    const size_t nr = rs.size();
    took(ctx, P_OR_MANY);
    if (int rc = um_scratch_clean(ctx)) return rc;
    // range descriptors + block prefix: thousands of entries, through a grow-only pinned block
    const size_t desc_bytes = align_up(nr * sizeof(UmRange)), stage_bytes = um_desc_bytes(nr);
    if (int rc = grow_pinned(ctx, &ctx->h_um, &ctx->h_um_cap, stage_bytes, false, "ii2_union_ranges: staging allocation failed")) return rc;
    um_desc_fill(rs, 0, nr, (uint8_t *)ctx->h_um);
    // the doc range: from the lists' mirrored spans, else one reduction over the blocks (below, once the descriptors are up)
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    const bool mirrored = mirrored_span(rs, &lo, &hi);
    const uint64_t W = um_window(ctx);                          // docs per window
    // workspace: descriptors, counts, offsets, scan temp, the running offset and the bounds (sized for the largest window possible
    // before the bounds are known: min(W, 2^32) docs)
    const uint64_t n_sum_max = (W + 65535) / 65536;
    UnionManyParams p;
    std::memset(&p, 0, sizeof p);
    const size_t scan_tmp = scan_temp_bytes(n_sum_max + 1);
    if (int rc = ii2_ws_reserve(ctx, stage_bytes + 2 * align_up((n_sum_max + 1) * sizeof(uint64_t)) + scan_tmp + 2 * 256 + 4096)) return rc;
    uint8_t *d_stage = ws_take<uint8_t>(ctx, stage_bytes);
    p.ranges = (const UmRange *)d_stage;
    p.pre = (const uint32_t *)(d_stage + desc_bytes);
    p.cnt = ws_take<uint32_t>(ctx, n_sum_max + 1);
    p.off = ws_take<uint64_t>(ctx, n_sum_max + 1);
    void *d_scan = ws_take<uint8_t>(ctx, scan_tmp);
    p.run = ws_take<uint64_t>(ctx, 2);
    p.bounds = ws_take<uint32_t>(ctx, 2);
    p.n_ranges = (uint32_t)nr;
    p.n_blocks = (uint32_t)n_blocks;
    ctx->um_dirty = true;
    HIP_TRY(ctx, hipMemcpyAsync(d_stage, ctx->h_um, stage_bytes, hipMemcpyHostToDevice, st));
    if (!mirrored) {
        HIP_TRY(ctx, hipMemsetAsync(p.bounds, 0xFF, sizeof(uint32_t), st));
        HIP_TRY(ctx, hipMemsetAsync(p.bounds + 1, 0, sizeof(uint32_t), st));
        took(ctx, P_SPAN_BOUNDS);
        HIP_TRY(ctx, launch_union_many_bounds(p, st));
        uint32_t *hb = (uint32_t *)(ctx->h_mail + II2_MAIL_COUNT + 1);
        HIP_TRY(ctx, hipMemcpyAsync(hb, p.bounds, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        lo = hb[0];
        hi = hb[1];
    }
    if (lo > hi) return fail(ctx, II2_EINVAL, "ii2_union_ranges: inconsistent list bounds");
    const uint32_t base = lo & ~31u;
    const uint64_t span = (uint64_t)hi - base + 1;
    const uint64_t n_win = (span + W - 1) / W;
    // the scratch: bitmap + summary of the largest window, zero
    if (int rc = um_scratch_reserve(ctx, "ii2_union_ranges", span, W)) return rc;
    uint64_t *d_cnt = ii2_mapped_mail(ctx, II2_MAIL_COUNT);
    p.d_count = d_cnt ? d_cnt : ctx->d_mail;
    set_tomb(p, tomb);
    p.out = d_out;
    p.out_cap = cap;
    p.check_window = n_win > 1 ? 1u : 0u;
    p.no_atomics = ctx->opt_union_many_no_atomics ? 1u : 0u;
    p.per_wave = um_per_wave(ctx, n_blocks);
    // several windows whose result may not fit: count first (nothing written), then write
    const bool count_first = n_win > 1 && cap < n_blocks * II2_DV1_BLOCK;
    if (count_first) took(ctx, P_OR_MANY_COUNT_FIRST);
    for (int pass = count_first ? 0 : 1; pass < 2; pass++) {
        p.write = (uint32_t)pass;
        for (uint64_t w = 0; w < n_win; w++) {
            const uint64_t wlo = base + w * W;
            p.window = (uint32_t)w;
            um_set_window(ctx, p, wlo, std::min<uint64_t>(W, (uint64_t)hi - wlo + 1));
            const uint32_t grid = (uint32_t)std::min<uint64_t>((p.n_sum + 1 + 3) / 4, (uint64_t)ctx->cu_count * 8u);
            hipEvent_t e0 = nullptr, e1 = nullptr;
            ii2_profile_pair(ctx, &e0, &e1);
            took(ctx, P_OR_MANY_WINDOW);
            HIP_TRY(ctx, launch_union_many_mark(p, st, e0, e1));
            HIP_TRY(ctx, launch_union_many_count(p, grid, st));
            HIP_TRY(ctx, scan_excl_u32_to_u64(d_scan, scan_tmp, p.cnt, p.off, p.n_sum + 1, st));
            HIP_TRY(ctx, launch_union_many_compact(p, grid, st));
        }
        if (int rc = read_count(ctx, p.d_count, count)) return rc;
        ctx->um_dirty = false;
        if (*count > cap) return fail(ctx, II2_ECAPACITY, "ii2_union_ranges: result does not fit the output buffer (nothing written)");
    }
    return II2_OK;
}

// OR of collected ranges (n_blocks > 0 blocks, n_nonempty non-empty lists) into d_out, all or nothing
static int union_collected(ii2_ctx *ctx, const std::vector<RangeIn> &rs, uint64_t n_blocks, uint64_t n_nonempty, const ii2_tomb *tomb,
                           uint32_t *d_out, uint64_t cap, uint64_t *count) {
    // up to 64 lists: the tuned OR paths - when the result surely fits (they may write part of a result that does not)
    if (!ctx->opt_union_many && n_nonempty <= MAX_LISTS) {
        SetList L[MAX_LISTS];
        uint32_t m = 0;
        uint64_t n_post = 0;
        for (const RangeIn &q : rs) {
            if (cap < n_blocks * II2_DV1_BLOCK)
                if (int rc = ii2_seg_host_cnt(ctx, q.seg)) return rc;
            for (uint64_t j = q.l0; j < q.l1; j++) {
                const uint32_t b0 = q.seg->h_blk_off[j], b1 = q.seg->h_blk_off[j + 1];
                if (b1 == b0) continue;
                L[m++] = SetList{list_view(q.seg, j), q.seg, j};
                n_post += cap < n_blocks * II2_DV1_BLOCK ? q.seg->h_cnt[j] : (uint64_t)(b1 - b0) * II2_DV1_BLOCK;
            }
        }
        if (cap >= n_post) return union_lists(ctx, L, m, n_blocks, tomb, d_out, cap, count);
    }
    return union_many(ctx, rs, n_blocks, tomb, d_out, cap, count);
}

static int union_ranges_unlocked(ii2_ctx *ctx, uint64_t n, const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end,
                                 const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap, uint64_t *count) {
    if (n && (!segs || !list_first || !list_end)) return fail(ctx, II2_EINVAL, "ii2_union_ranges: bad argument");
    std::vector<RangeIn> rs;
    uint64_t n_blocks = 0, n_nonempty = 0;
    if (int rc = collect_ranges(ctx, "ii2_union_ranges", n, segs, list_first, list_end, rs, &n_blocks, &n_nonempty)) return rc;
    if (!n_blocks) { *count = 0; return II2_OK; }
    if (n_blocks >= 0xFFFFFFFFull || rs.size() >= 0xFFFFFFFFull) return fail(ctx, II2_ERANGE, "ii2_union_ranges: more than 2^32 - 2 blocks in one call");
    if (!d_out) return fail(ctx, II2_EINVAL, "ii2_union_ranges: output buffer is NULL");
    return union_collected(ctx, rs, n_blocks, n_nonempty, tomb, d_out, cap, count);
}

extern "C" int ii2_union_ranges(ii2_ctx *ctx, uint64_t n, const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end,
                                const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap, uint64_t *count) {
    if (!ctx || !count) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return union_ranges_unlocked(ctx, n, segs, list_first, list_end, tomb, d_out, cap, count);
}

// ---- hits per list against a doc set ------------------------------------------------------------
// what a call found out before its first launch: the checked ranges that own blocks, the counter of each one's first list, and
// the totals
struct CountIn {
    std::vector<RangeIn> rs;
    std::vector<uint32_t> out_first;
    uint64_t n_named = 0, n_blocks = 0;
};

// counts and stats of a call that succeeded with nothing to count: every count 0
static int count_done(const CountIn &in, uint64_t *counts, ii2_count_stats *stats) {
    if (in.n_named) std::memset(counts, 0, in.n_named * sizeof(uint64_t));
    if (stats) *stats = ii2_count_stats{in.n_named, in.n_blocks, 0, 0, 0};
    return II2_OK;
}

// The windows of a walk that tests ids against a marked doc set (marked_call): the docs [lo, hi] in windows of
// um_window(ctx) docs, per window k_cr_mark of p.set, `walk` - the launch that reads the marks through p's window fields, set here -
// and k_ir_clear.  *n_win grows by the windows run.
template <class Walk>
static int marked_windows(ii2_ctx *ctx, const char *who, CountParams &p, uint32_t lo, uint32_t hi, uint32_t *n_win, Walk walk) {
    hipStream_t st = ctx->stream;
    const uint64_t W = um_window(ctx);
    const uint32_t base = lo & ~2047u;                          // the summary's bits are the docs' 2048-doc chunks: doc >> 11
    const uint64_t span = (uint64_t)hi - base + 1;
    if (int rc = um_scratch_reserve(ctx, who, span, W)) return rc;
    for (uint64_t wlo = base; wlo <= hi; wlo += W, ++*n_win) {
        UnionManyParams wp;
        um_set_window(ctx, wp, wlo, std::min<uint64_t>(W, (uint64_t)hi - wlo + 1));
        p.win_lo = wp.win_lo;
        p.win_docs = wp.win_docs;
        p.n_sum = wp.n_sum;
        p.bitmap = wp.bitmap;
        p.summary = wp.summary;
        p.doc_lo = std::max(lo, p.win_lo);
        p.doc_hi = (uint32_t)std::min<uint64_t>(hi, wlo + p.win_docs - 1);
        IrParams ip;
        std::memset(&ip, 0, sizeof ip);
        ip.n_sum = p.n_sum;
        ip.bitmap = p.bitmap;
        ip.summary = p.summary;
        const uint32_t grid = (uint32_t)std::min<uint64_t>((p.n_sum + 3) / 4, (uint64_t)ctx->cu_count * 8u);
        HIP_TRY(ctx, launch_cr_mark(p, st));
        HIP_TRY(ctx, walk());
        HIP_TRY(ctx, launch_ir_clear(ip, grid, st));
    }
    return II2_OK;
}

// What a reader of a marked doc set hands to marked_call.
struct MarkedIn {
    const char *who;                                            // the entry point in the messages
    const std::vector<RangeIn> &rs;                             // the checked ranges that own blocks
    const uint32_t *range_words;                                // [rs.size()] CountParams::out_first: each range's first counter / its group
    uint64_t n_blocks;
    const void *extra;                                          // the caller's own upload behind them (the histogram's axis) ...
    size_t extra_bytes;
    size_t back_bytes;                                          // ... its counters on the device: zeroed, read back at the end
    size_t ws_bytes;                                            // ... and the workspace it takes in `setup`
    const uint32_t *clip;                                       // {first, last} doc the docs that can hit are clipped to as well, or NULL
    bool every_doc;                                             // no set: no span, no mark, no window - `walk` once, as the caller set p
};

// The host side of a walk of the ranges' blocks against a doc set (cr_walk.h), as ii2_count_ranges, ii2_histogram_ranges and
// ii2_explain_ranges share it.  One staging copy takes up the range descriptors with their block prefix, the ranges' words, the
// caller's extra and the start values of the four span words {lists' first doc, lists' last doc, set's smallest id, set's largest
// id}; `setup(d_extra, d_back, d_span)` completes the caller's parameters around p and enqueues what else it needs.  Then the
// span - the lists' from the segments' mirrors, else by k_um_bounds, the set's by `edges`, one copy, one wait - the windows of its
// overlap (marked_windows around `walk(e0, e1)`, the profile events on the first one) and the caller's counters back behind a
// second wait: *back, or NULL when the set and the lists (and the clip) share no doc - nothing was marked, every counter is 0.
// The caller sets p.per_wave, the set and the tombstones; the walk's other fields are set here.
template <class Setup, class Edges, class Walk>
static int marked_call(ii2_ctx *ctx, const MarkedIn &in, CountParams &p, uint32_t *n_win, const uint8_t **back, Setup setup, Edges edges, Walk walk) {
    hipStream_t st = ctx->stream;
    const size_t nr = in.rs.size();
    const std::string who(in.who);
    *back = nullptr;
    if (int rc = um_scratch_clean(ctx)) return rc;
    const size_t desc_bytes = align_up(nr * sizeof(UmRange)), um_bytes = um_desc_bytes(nr), extra_at = um_bytes + align_up(nr * sizeof(uint32_t));
    const size_t span_at = extra_at + align_up(in.extra_bytes), up_bytes = span_at + 256;
    if (int rc = grow_pinned(ctx, &ctx->h_um, &ctx->h_um_cap, up_bytes + in.back_bytes, false, (who + ": staging allocation failed").c_str())) return rc;
    uint8_t *h = (uint8_t *)ctx->h_um;
    um_desc_fill(in.rs, 0, nr, h);
    std::memcpy(h + um_bytes, in.range_words, nr * sizeof(uint32_t));
    if (in.extra_bytes) std::memcpy(h + extra_at, in.extra, in.extra_bytes);
    const uint32_t span0[4] = {0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u};      // (k_um_bounds and k_ex_prepare reduce into them)
    std::memcpy(h + span_at, span0, sizeof span0);
    // the lists' doc span: from the mirrored spans, else one reduction over the blocks (below, once the descriptors are up)
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    const bool mirrored = in.every_doc || mirrored_span(in.rs, &lo, &hi);
    if (int rc = ii2_ws_reserve(ctx, up_bytes + align_up(in.back_bytes) + in.ws_bytes + 4096)) return rc;
    uint8_t *d_stage = ws_take<uint8_t>(ctx, up_bytes);
    uint8_t *d_back = ws_take<uint8_t>(ctx, in.back_bytes);
    uint32_t *d_span = (uint32_t *)(d_stage + span_at);
    UnionManyParams bp;                                         // (k_um_bounds takes the union's parameters)
    std::memset(&bp, 0, sizeof bp);
    bp.ranges = (const UmRange *)d_stage;
    bp.pre = (const uint32_t *)(d_stage + desc_bytes);
    bp.n_ranges = (uint32_t)nr;
    bp.n_blocks = (uint32_t)in.n_blocks;
    bp.bounds = d_span;
    p.ranges = bp.ranges;
    p.pre = bp.pre;
    p.out_first = (const uint32_t *)(d_stage + um_bytes);
    p.n_ranges = bp.n_ranges;
    p.n_blocks = bp.n_blocks;
    p.summary_skip = ctx->opt_count_summary_skip ? 1u : 0u;
    p.edges = d_span + 2;
    ctx->um_dirty = true;
    HIP_TRY(ctx, hipMemcpyAsync(d_stage, h, up_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(d_back, 0, in.back_bytes, st));
    if (int rc = setup(d_stage + extra_at, d_back, d_span)) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (in.every_doc) {
        ii2_profile_pair(ctx, &e0, &e1);
        HIP_TRY(ctx, walk(e0, e1));
    } else {
        if (!mirrored) HIP_TRY(ctx, launch_union_many_bounds(bp, st));
        HIP_TRY(ctx, edges());
        uint32_t *hb = (uint32_t *)(ctx->h_mail + II2_MAIL_COUNT + 1);
        HIP_TRY(ctx, hipMemcpyAsync(hb, d_span, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (!mirrored) {
            lo = hb[0];
            hi = hb[1];
        }
        if (lo > hi) return fail(ctx, II2_EINVAL, (who + ": inconsistent list bounds").c_str());
        // the docs that can hit: the lists' span clipped to the set's (and to the caller's clip)
        lo = std::max(std::max(lo, hb[2]), in.clip ? in.clip[0] : 0u);
        hi = std::min(std::min(hi, hb[3]), in.clip ? in.clip[1] : 0xFFFFFFFFu);
        if (lo > hi) {                                          // no overlap: nothing was marked, what was enqueued has been waited for
            ctx->um_dirty = false;
            return II2_OK;
        }
        ii2_profile_pair(ctx, &e0, &e1);
        if (int rc = marked_windows(ctx, in.who, p, lo, hi, n_win, [&]() {
                const hipError_t e = walk(e0, e1);
                e0 = e1 = nullptr;
                return e;
            }))
            return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(h + up_bytes, d_back, in.back_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->um_dirty = false;
    *back = h + up_bytes;
    return II2_OK;
}

// The block-wise count (count_ranges.hip) of the ranges' blocks against d_set - per window of the doc span that the set and the
// lists share mark, count, clear - or, with d_set == NULL, against "every doc" minus the tombstones in one launch.  At most two
// waits: the span fetch and the final read.
static int count_many(ii2_ctx *ctx, const CountIn &in, const uint32_t *d_set, uint64_t n_set, const ii2_tomb *tomb, uint64_t *counts,
                      ii2_count_stats *stats) {
    const size_t n_words = (size_t)in.n_named + CR_DECODED_SLOTS;
    CountParams p;
    std::memset(&p, 0, sizeof p);
    p.per_wave = um_per_wave(ctx, in.n_blocks);
    p.set = d_set;
    p.n_set = n_set;
    set_tomb(p, tomb);
    const MarkedIn m{"ii2_count_ranges", in.rs, in.out_first.data(), in.n_blocks, nullptr, 0, n_words * sizeof(uint32_t), 0, nullptr, !d_set};
    uint32_t n_win = 0;
    const uint8_t *back = nullptr;
    if (int rc = marked_call(ctx, m, p, &n_win, &back,
                             [&](uint8_t *, uint8_t *d_back, uint32_t *) {
                                 p.counts = (uint32_t *)d_back;
                                 p.decoded = p.counts + in.n_named;
                                 return II2_OK;
                             },
                             [&]() { return launch_cr_edges(p, ctx->stream); },
                             [&](hipEvent_t e0, hipEvent_t e1) { return launch_cr_count(p, !d_set, ctx->stream, e0, e1); }))
        return rc;
    if (!back) return count_done(in, counts, stats);
    const uint32_t *h_words = (const uint32_t *)back;
    uint64_t hits = 0, decoded = 0;
    for (uint64_t k = 0; k < in.n_named; k++) {
        counts[k] = h_words[k];
        hits += h_words[k];
    }
    for (uint32_t k = 0; k < CR_DECODED_SLOTS; k++) decoded += h_words[in.n_named + k];
    if (stats) *stats = ii2_count_stats{in.n_named, in.n_blocks, decoded, hits, n_win};
    return II2_OK;
}

// The checks that the counting entry points share (`who` names the one in the messages), and what they find out: the ranges one
// by one - those that own blocks keep the index of their first list's count.
static int count_collect(ii2_ctx *ctx, const char *who, uint64_t n, const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end,
                         uint64_t n_set, const ii2_tomb *tomb, CountIn &in) {
    const std::string w(who);
    if (n && (!segs || !list_first || !list_end)) return fail(ctx, II2_EINVAL, (w + ": bad argument").c_str());
    if (tomb && tomb->device != ctx->device) return fail(ctx, II2_EINVAL, (w + ": tombstones live on another device").c_str());
    if (n_set > (1ull << 32)) return fail(ctx, II2_EINVAL, (w + ": more than 2^32 set ids").c_str());
    uint64_t n_nonempty = 0;
    for (uint64_t i = 0; i < n; i++) {
        const size_t before = in.rs.size();
        if (int rc = collect_ranges(ctx, who, 1, segs + i, list_first + i, list_end + i, in.rs, &in.n_blocks, &n_nonempty)) return rc;
        if (in.n_named >= (1ull << 31)) return fail(ctx, II2_ERANGE, (w + ": 2^31 lists or more in one call").c_str());
        if (in.rs.size() > before) in.out_first.push_back((uint32_t)in.n_named);
        in.n_named += list_end[i] - list_first[i];
    }
    if (in.n_named >= (1ull << 31)) return fail(ctx, II2_ERANGE, (w + ": 2^31 lists or more in one call").c_str());
    if (in.n_blocks >= 0xFFFFFFFFull || in.rs.size() >= 0xFFFFFFFFull) return fail(ctx, II2_ERANGE, (w + ": more than 2^32 - 2 blocks in one call").c_str());
    return II2_OK;
}

static int count_ranges_unlocked(ii2_ctx *ctx, uint64_t n, const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end,
                                 const uint32_t *d_set, uint64_t n_set, const ii2_tomb *tomb, uint64_t *counts, uint64_t counts_cap,
                                 ii2_count_stats *stats) {
    CountIn in;
    if (int rc = count_collect(ctx, "ii2_count_ranges", n, segs, list_first, list_end, n_set, tomb, in)) return rc;
    if (in.n_named && !counts) return fail(ctx, II2_EINVAL, "ii2_count_ranges: counts is NULL");
    if (counts_cap < in.n_named) return fail(ctx, II2_ECAPACITY, "ii2_count_ranges: counts holds fewer entries than lists are named (nothing written)");
    if (!in.n_blocks || (d_set && !n_set)) return count_done(in, counts, stats);
    if (!d_set && !tomb) {
        // every doc, nothing removed: the lists' lengths, from the segments' host mirrors
        for (const RangeIn &q : in.rs)
            if (int rc = ii2_seg_host_cnt(ctx, q.seg)) return rc;
        count_done(in, counts, stats);
        uint64_t hits = 0;
        for (size_t r = 0; r < in.rs.size(); r++)
            for (uint64_t j = in.rs[r].l0; j < in.rs[r].l1; j++) hits += counts[in.out_first[r] + (j - in.rs[r].l0)] = in.rs[r].seg->h_cnt[j];
        if (stats) stats->n_hits = hits;
        return II2_OK;
    }
    return count_many(ctx, in, d_set, n_set, tomb, counts, stats);
}

extern "C" int ii2_count_ranges(ii2_ctx *ctx, uint64_t n, const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end,
                                const uint32_t *d_set, uint64_t n_set, const ii2_tomb *tomb, uint64_t *counts, uint64_t counts_cap,
                                ii2_count_stats *stats) {
    if (!ctx) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return count_ranges_unlocked(ctx, n, segs, list_first, list_end, d_set, n_set, tomb, counts, counts_cap, stats);
}

// ---- hits per list and value bucket --------------------------------------------------------------
// the value axis of a histogram call as the device takes it (hist_device.h)
struct HistAxis {
    std::vector<uint32_t> first;                                // [n_buckets] edges[0 .. n_buckets)
    uint32_t last = 0;                                          // edges[n_buckets] - 1
};
// the edge checks of every histogram entry point; *msg says what is wrong
static int hist_check_edges(uint32_t n_buckets, const uint64_t *edges, const char **msg) {
    *msg = "no bucket, or edges is NULL";
    if (!n_buckets || !edges) return II2_EINVAL;
    *msg = "more than II2_HIST_MAX_BUCKETS buckets in one call";
    if (n_buckets > II2_HIST_MAX_BUCKETS) return II2_ERANGE;
    *msg = "the edges are not strictly ascending values <= 2^32";
    for (uint32_t b = 0; b < n_buckets; b++)
        if (edges[b] >= edges[b + 1]) return II2_EINVAL;
    if (edges[n_buckets] > (1ull << 32)) return II2_EINVAL;
    return II2_OK;
}
static int hist_axis(ii2_ctx *ctx, const char *who, uint32_t n_buckets, const uint64_t *edges, HistAxis &ax) {
    const char *msg = nullptr;
    if (int rc = hist_check_edges(n_buckets, edges, &msg)) return fail(ctx, rc, (std::string(who) + ": " + msg).c_str());
    ax.first.resize(n_buckets);
    for (uint32_t b = 0; b < n_buckets; b++) ax.first[b] = (uint32_t)edges[b];
    ax.last = (uint32_t)(edges[n_buckets] - 1u);
    return II2_OK;
}

extern "C" int ii2_hist_bucket(const uint64_t *edges, uint32_t n_buckets, uint32_t id, int64_t *bucket) {
    const char *msg = nullptr;
    if (int rc = hist_check_edges(n_buckets, edges, &msg)) return rc;
    if (!bucket) return II2_EINVAL;
    *bucket = hist_bucket(edges, n_buckets, (uint32_t)(edges[n_buckets] - 1u), id);
    return II2_OK;
}

extern "C" int ii2_hist_block(const uint64_t *edges, uint32_t n_buckets, uint32_t first_doc, uint32_t up, int *kind, uint32_t *b_lo, uint32_t *b_hi) {
    const char *msg = nullptr;
    if (int rc = hist_check_edges(n_buckets, edges, &msg)) return rc;
    if (!kind || !b_lo || !b_hi) return II2_EINVAL;
    uint32_t lo = 0, hi = 0;
    *kind = hist_block(edges, n_buckets, edges[0], (uint32_t)(edges[n_buckets] - 1u), first_doc, up, &lo, &hi);
    *b_lo = lo;
    *b_hi = hi;
    return II2_OK;
}

// counts and stats of a histogram call that succeeded with nothing to count: every cell 0
static int hist_done(const CountIn &in, uint32_t n_buckets, uint64_t *counts, ii2_hist_stats *stats) {
    if (in.n_named) std::memset(counts, 0, in.n_named * n_buckets * sizeof(uint64_t));
    if (stats) *stats = ii2_hist_stats{in.n_named, in.n_blocks, 0, 0, 0, 0, 0, 0, n_buckets};
    return II2_OK;
}

// count_many with a counter per (list, bucket) (histogram.hip): the axis goes up with the descriptors in the one staging copy, the
// docs that can hit are the lists' span clipped to the set's AND to the axis.  At most two waits - the span fetch and the final
// read; the "every doc" form waits once.
static int hist_many(ii2_ctx *ctx, const CountIn &in, const uint32_t *d_set, uint64_t n_set, const ii2_tomb *tomb, const HistAxis &ax, uint64_t *counts,
                     ii2_hist_stats *stats) {
    const uint32_t nb = (uint32_t)ax.first.size();
    const uint32_t axis[2] = {ax.first[0], ax.last};
    HistParams hp;
    std::memset(&hp, 0, sizeof hp);
    CountParams &p = hp.c;
    if (!d_set) {
        // no set to fetch a span of: the lists' mirrored span where there is one, clipped to the axis, before anything goes up
        uint32_t lo = 0xFFFFFFFFu, hi = 0;
        if (!mirrored_span(in.rs, &lo, &hi)) lo = 0, hi = 0xFFFFFFFFu;
        p.doc_lo = std::max(lo, axis[0]);
        p.doc_hi = std::min(hi, axis[1]);
        if (p.doc_lo > p.doc_hi) return hist_done(in, nb, counts, stats);
    }
    const size_t n_cells = (size_t)in.n_named * nb, n_words = n_cells + 3 * CR_DECODED_SLOTS;
    p.per_wave = ctx->opt_hist_per_wave > 0 ? (uint32_t)std::min<int64_t>(ctx->opt_hist_per_wave, 1 << 20) : um_per_wave(ctx, in.n_blocks);
    p.set = d_set;
    p.n_set = n_set;
    set_tomb(p, tomb);
    hp.n_buckets = nb;
    hp.first0 = axis[0];
    hp.last = axis[1];
    hp.whole = ctx->opt_hist_whole ? 1u : 0u;
    const MarkedIn m{"ii2_histogram_ranges", in.rs, in.out_first.data(), in.n_blocks, ax.first.data(), nb * sizeof(uint32_t), n_words * sizeof(uint32_t), 0, axis, !d_set};
    uint32_t n_win = 0;
    const uint8_t *back = nullptr;
    if (int rc = marked_call(ctx, m, p, &n_win, &back,
                             [&](uint8_t *d_axis, uint8_t *d_back, uint32_t *) {
                                 hp.first = (const uint32_t *)d_axis;
                                 p.counts = (uint32_t *)d_back;
                                 p.decoded = p.counts + n_cells;
                                 return II2_OK;
                             },
                             [&]() { return launch_cr_edges(p, ctx->stream); },
                             [&](hipEvent_t e0, hipEvent_t e1) { return launch_hs_count(hp, !d_set, ctx->stream, e0, e1); }))
        return rc;
    if (!back) return hist_done(in, nb, counts, stats);
    const uint32_t *h_words = (const uint32_t *)back;
    uint64_t hits = 0, kinds[3] = {0, 0, 0};
    for (size_t k = 0; k < n_cells; k++) {
        counts[k] = h_words[k];
        hits += h_words[k];
    }
    for (uint32_t k = 0; k < 3 * CR_DECODED_SLOTS; k++) kinds[k / CR_DECODED_SLOTS] += h_words[n_cells + k];
    if (stats) *stats = ii2_hist_stats{in.n_named, in.n_blocks, kinds[0] + kinds[1] + kinds[2], hits, kinds[0], kinds[1], kinds[2], n_win, nb};
    return II2_OK;
}

extern "C" int ii2_histogram_ranges(ii2_ctx *ctx, uint64_t n, const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end,
                                    const uint32_t *d_set, uint64_t n_set, const ii2_tomb *tomb, uint32_t n_buckets, const uint64_t *edges,
                                    uint64_t *counts, uint64_t counts_cap, ii2_hist_stats *stats) {
    if (!ctx) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HistAxis ax;
    if (int rc = hist_axis(ctx, "ii2_histogram_ranges", n_buckets, edges, ax)) return rc;
    CountIn in;
    if (int rc = count_collect(ctx, "ii2_histogram_ranges", n, segs, list_first, list_end, n_set, tomb, in)) return rc;
    if (in.n_named * n_buckets > II2_HIST_MAX_CELLS) return fail(ctx, II2_ERANGE, "ii2_histogram_ranges: more than II2_HIST_MAX_CELLS lists x buckets in one call");
    if (in.n_named && !counts) return fail(ctx, II2_EINVAL, "ii2_histogram_ranges: counts is NULL");
    if (counts_cap < in.n_named * n_buckets)
        return fail(ctx, II2_ECAPACITY, "ii2_histogram_ranges: counts holds fewer entries than lists named x buckets (nothing written)");
    if (!in.n_blocks || (d_set && !n_set)) return hist_done(in, n_buckets, counts, stats);
    return hist_many(ctx, in, d_set, n_set, tomb, ax, counts, stats);
}

// The bucket counts of a device set: without tombstones a bisection of the set per edge, with them one pass over the ids.  One
// wait: the counters' copy.
extern "C" int ii2_histogram_ids(ii2_ctx *ctx, const uint32_t *d_set, uint64_t n_set, const ii2_tomb *tomb, uint32_t n_buckets,
                                 const uint64_t *edges, uint64_t *counts, uint64_t counts_cap) {
    if (!ctx) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HistAxis ax;
    if (int rc = hist_axis(ctx, "ii2_histogram_ids", n_buckets, edges, ax)) return rc;
    if (tomb && tomb->device != ctx->device) return fail(ctx, II2_EINVAL, "ii2_histogram_ids: tombstones live on another device");
    if (n_set >= (1ull << 32)) return fail(ctx, II2_EINVAL, "ii2_histogram_ids: 2^32 set ids or more");
    if (n_set && !d_set) return fail(ctx, II2_EINVAL, "ii2_histogram_ids: the set is NULL");
    if (!counts) return fail(ctx, II2_EINVAL, "ii2_histogram_ids: counts is NULL");
    if (counts_cap < n_buckets) return fail(ctx, II2_ECAPACITY, "ii2_histogram_ids: counts holds fewer entries than buckets (nothing written)");
    if (!n_set) {
        std::memset(counts, 0, n_buckets * sizeof(uint64_t));
        return II2_OK;
    }
    hipStream_t st = ctx->stream;
    if (int rc = um_scratch_clean(ctx)) return rc;               // (a stopped call's copy out of the staging block may be pending)
    const size_t ax_bytes = align_up(n_buckets * sizeof(uint32_t));
    if (int rc = grow_pinned(ctx, &ctx->h_um, &ctx->h_um_cap, 2 * ax_bytes, false, "ii2_histogram_ids: staging allocation failed")) return rc;
    uint8_t *h = (uint8_t *)ctx->h_um;
    std::memcpy(h, ax.first.data(), n_buckets * sizeof(uint32_t));
    uint32_t *h_words = (uint32_t *)(h + ax_bytes);
    if (int rc = ii2_ws_reserve(ctx, 2 * ax_bytes + 4096)) return rc;
    uint32_t *d_first = ws_take<uint32_t>(ctx, n_buckets);
    uint32_t *d_words = ws_take<uint32_t>(ctx, n_buckets);
    HistParams hp;
    std::memset(&hp, 0, sizeof hp);
    hp.c.set = d_set;
    hp.c.n_set = n_set;
    set_tomb(hp.c, tomb);
    hp.c.counts = d_words;
    hp.first = d_first;
    hp.n_buckets = n_buckets;
    hp.last = ax.last;
    ctx->um_dirty = true;
    HIP_TRY(ctx, hipMemcpyAsync(d_first, h, n_buckets * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (tomb) {
        HIP_TRY(ctx, hipMemsetAsync(d_words, 0, n_buckets * sizeof(uint32_t), st));
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ii2_profile_pair(ctx, &e0, &e1);
    HIP_TRY(ctx, launch_hs_ids(hp, st, e0, e1));
    HIP_TRY(ctx, hipMemcpyAsync(h_words, d_words, n_buckets * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->um_dirty = false;
    for (uint32_t b = 0; b < n_buckets; b++) counts[b] = h_words[b];
    return II2_OK;
}

// ---- AND of ORs over list ranges ----------------------------------------------------------------
// one group of a call: its checked ranges rs[r0, r1), their blocks, non-empty lists and postings, and its doc span
struct GroupIn {
    size_t r0, r1;
    uint64_t n_blocks, n_nonempty, n_post;
    uint32_t lo, hi;
    bool span_known;
};

// the pinned staging block of the group path's descriptors: `bytes` of it, once the stream has passed the last copy from it
static int ir_stage(ii2_ctx *ctx, size_t bytes, uint8_t **h) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // (a no-op after the count read that ends every step)
    if (int rc = grow_pinned(ctx, &ctx->h_ir, &ctx->h_ir_cap, bytes, false, "ii2_intersect_ranges: staging allocation failed")) return rc;
    *h = (uint8_t *)ctx->h_ir;
    return II2_OK;
}

// one filter pass of the group path: the group's ranges rs[r0, r1) with their sizes, the doc span the mark's windows cover, and
// whether the candidates found survive (a required group) or those NOT found (the excluded lists of ii2_andnot_ranges)
struct IrPass {
    size_t r0, r1;
    uint64_t n_blocks, n_nonempty, n_post;
    uint32_t lo, hi;
    bool drop;
};

// a non-empty list of a pass that its probe looks at: every one of a required group; of an exclusion those whose mirrored doc
// span meets [lo, hi] (a list elsewhere removes nothing)
static bool ir_list_counts(const IrPass &G, const ii2_seg *s, uint64_t j) {
    if (s->h_blk_off[j + 1] == s->h_blk_off[j]) return false;
    if (!G.drop || !spans_mirrored(s)) return true;
    return s->h_spans[3 * j] <= G.hi && s->h_spans[3 * j + 2] >= G.lo;
}

// The candidates cand[0, nc) (ascending, nc > 0) filtered by one group - probe or mark (intersect_ranges.hip), scan, compact - into
// out, which is written only when all *n_out survivors fit out_cap.  One count read.
static int ir_filter_pass(ii2_ctx *ctx, const char *who, const std::vector<RangeIn> &rs, const IrPass &G, const uint32_t *cand, uint64_t nc,
                          uint32_t *out, uint64_t out_cap, uint64_t *n_out) {
    hipStream_t st = ctx->stream;
    uint64_t *d_cnt = ii2_mapped_mail(ctx, II2_MAIL_COUNT);
    const size_t nr = G.r1 - G.r0;
    // probe: one search per list and run of 256 candidates, the runs' block walks one after the other (latency-bound: it needs
    // enough runs to fill the GPU); mark: every posting of the group once.  Measured: the probe wins on long
    // lists against millions of candidates, the mark on many lists and on few candidates (option intersect.ranges_mark).
    const uint64_t runs = (nc + IR_PROBE_RUN - 1) / IR_PROBE_RUN;
    const bool mark = ctx->opt_ir_mark > 0 &&
                      (runs < 4u * (uint64_t)ctx->cu_count || (double)G.n_post <= (double)ctx->opt_ir_mark * (double)G.n_nonempty * (double)runs);
    took(ctx, mark ? (G.drop ? P_IR_MARK_DROP : P_IR_MARK) : (G.drop ? P_IR_PROBE_DROP : P_IR_PROBE));
    const size_t desc_bytes = mark ? um_desc_bytes(nr) : align_up(G.n_nonempty * sizeof(IrList));
    uint8_t *h = nullptr;
    if (int rc = ir_stage(ctx, desc_bytes, &h)) return rc;
    size_t m = 0;
    if (mark) um_desc_fill(rs, G.r0, G.r1, h);
    else {
        IrList *hl = (IrList *)h;
        for (size_t r = G.r0; r < G.r1; r++) {
            const ii2_seg *s = rs[r].seg;
            const bool mirrored = spans_mirrored(s);
            for (uint64_t j = rs[r].l0; j < rs[r].l1 && m < G.n_nonempty; j++) {
                if (!ir_list_counts(G, s, j)) continue;
                const uint32_t b0 = s->h_blk_off[j], b1 = s->h_blk_off[j + 1];
                hl[m++] = IrList{s->d_skip + b0, s->d_payload, s->d_last_doc + j, b1 - b0, mirrored ? s->h_spans[3 * j] : 1u,
                                 mirrored ? s->h_spans[3 * j + 2] : 0u, 0u};
            }
        }
    }
    const size_t scan_tmp = scan_temp_bytes(nc + 1);
    if (int rc = ii2_ws_reserve(ctx, desc_bytes + align_up((nc + 1) * sizeof(uint32_t)) + scan_tmp + 4096)) return rc;
    uint8_t *d_desc = ws_take<uint8_t>(ctx, desc_bytes);
    IrParams ip;
    std::memset(&ip, 0, sizeof ip);
    ip.cand = cand;
    ip.n_cand = nc;
    ip.drop = G.drop ? 1u : 0u;
    ip.flag = ws_take<uint32_t>(ctx, nc + 1);
    void *d_scan = ws_take<uint8_t>(ctx, scan_tmp);
    HIP_TRY(ctx, hipMemcpyAsync(d_desc, h, desc_bytes, hipMemcpyHostToDevice, st));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ii2_profile_pair(ctx, &e0, &e1);
    if (mark) {
        if (G.drop) {                                   // a candidate outside every window survives: the flags start at one
            HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)ip.flag, 1, nc, st));
            HIP_TRY(ctx, hipMemsetAsync(ip.flag + nc, 0, sizeof(uint32_t), st));
        } else {
            HIP_TRY(ctx, hipMemsetAsync(ip.flag, 0, (nc + 1) * sizeof(uint32_t), st));
        }
        if (int rc = um_scratch_clean(ctx)) return rc;
        const uint64_t W = um_window(ctx);
        const uint32_t base = G.lo & ~31u;
        const uint64_t span = (uint64_t)G.hi - base + 1;
        if (int rc = um_scratch_reserve(ctx, who, span, W)) return rc;
        UnionManyParams p;
        std::memset(&p, 0, sizeof p);
        p.ranges = (const UmRange *)d_desc;
        p.pre = (const uint32_t *)(d_desc + align_up(nr * sizeof(UmRange)));
        p.n_ranges = (uint32_t)nr;
        p.n_blocks = (uint32_t)G.n_blocks;
        p.check_window = 1u;                        // blocks outside the candidates' span are not decoded
        p.per_wave = um_per_wave(ctx, G.n_blocks);
        ctx->um_dirty = true;
        for (uint64_t wlo = base; wlo <= G.hi; wlo += W) {
            um_set_window(ctx, p, wlo, std::min<uint64_t>(W, (uint64_t)G.hi - wlo + 1));
            ip.win_lo = p.win_lo;
            ip.win_docs = p.win_docs;
            ip.n_sum = p.n_sum;
            ip.bitmap = p.bitmap;
            ip.summary = p.summary;
            const uint32_t grid = (uint32_t)std::min<uint64_t>((p.n_sum + 3) / 4, (uint64_t)ctx->cu_count * 8u);
            HIP_TRY(ctx, launch_union_many_mark(p, st, e0, e1));
            HIP_TRY(ctx, launch_ir_test(ip, st));
            HIP_TRY(ctx, launch_ir_clear(ip, grid, st));
            e0 = e1 = nullptr;
        }
    } else {
        ip.lists = (const IrList *)d_desc;
        ip.n_lists = (uint32_t)m;
        HIP_TRY(ctx, hipMemsetAsync(ip.flag + nc, 0, sizeof(uint32_t), st));
        HIP_TRY(ctx, launch_ir_probe(ip, st, e0, e1));
    }
    HIP_TRY(ctx, scan_excl_u32(d_scan, scan_tmp, ip.flag, ip.flag, nc + 1, st));
    ip.out = out;
    ip.out_cap = out_cap;
    ip.d_count = d_cnt ? d_cnt : ctx->d_mail;
    HIP_TRY(ctx, launch_ir_compact(ip, st));
    if (int rc = read_count(ctx, ip.d_count, n_out)) return rc;
    ctx->um_dirty = false;
    return II2_OK;
}

// The group path: the driver's union (the group with the fewest postings, minus the tombstones) is the candidate array, then
// one filter pass per further group in ascending order of postings - probe or mark (intersect_ranges.hip), scan, compact -
// until no candidate is left.  The last pass writes d_out only when the whole result fits.  One count read per group.
static int intersect_groups(ii2_ctx *ctx, const std::vector<RangeIn> &rs, std::vector<GroupIn> &gs, const ii2_tomb *tomb, uint32_t *d_out,
                            uint64_t cap, uint64_t *count) {
    hipStream_t st = ctx->stream;
    // the spans not mirrored on the host: one bounds reduction per such group (k_um_bounds), one wait for all of them
    std::vector<size_t> need;
    for (size_t g = 0; g < gs.size(); g++) if (!gs[g].span_known) need.push_back(g);
    if (!need.empty()) {
        size_t bytes = 0;
        for (size_t g : need) bytes += um_desc_bytes(gs[g].r1 - gs[g].r0);
        const size_t bounds_bytes = align_up(2 * need.size() * sizeof(uint32_t));
        uint8_t *h = nullptr;
        if (int rc = ir_stage(ctx, bytes + bounds_bytes, &h)) return rc;
        if (int rc = ii2_ws_reserve(ctx, bytes + bounds_bytes + 4096)) return rc;
        uint8_t *d = ws_take<uint8_t>(ctx, bytes + bounds_bytes);       // the descriptors, then {smallest first doc, largest last doc} per group
        uint32_t *hb = (uint32_t *)(h + bytes), *d_bounds = (uint32_t *)(d + bytes);
        size_t at = 0;
        for (size_t i = 0; i < need.size(); i++) {
            um_desc_fill(rs, gs[need[i]].r0, gs[need[i]].r1, h + at);
            at += um_desc_bytes(gs[need[i]].r1 - gs[need[i]].r0);
            hb[2 * i] = 0xFFFFFFFFu;
            hb[2 * i + 1] = 0u;
        }
        HIP_TRY(ctx, hipMemcpyAsync(d, h, bytes + bounds_bytes, hipMemcpyHostToDevice, st));
        at = 0;
        for (size_t i = 0; i < need.size(); i++) {
            const GroupIn &G = gs[need[i]];
            const size_t nr = G.r1 - G.r0;
            UnionManyParams p;
            std::memset(&p, 0, sizeof p);
            p.ranges = (const UmRange *)(d + at);
            p.pre = (const uint32_t *)(d + at + align_up(nr * sizeof(UmRange)));
            p.n_ranges = (uint32_t)nr;
            p.n_blocks = (uint32_t)G.n_blocks;
            p.bounds = d_bounds + 2 * i;
            took(ctx, P_SPAN_BOUNDS);
            HIP_TRY(ctx, launch_union_many_bounds(p, st));
            at += um_desc_bytes(nr);
        }
        HIP_TRY(ctx, hipMemcpyAsync(hb, d_bounds, 2 * need.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        for (size_t i = 0; i < need.size(); i++) {
            gs[need[i]].lo = hb[2 * i];
            gs[need[i]].hi = hb[2 * i + 1];
        }
    }
    uint32_t clo = 0, chi = 0xFFFFFFFFu;
    for (const GroupIn &G : gs) {
        if (G.lo > G.hi) return fail(ctx, II2_EINVAL, "ii2_intersect_ranges: inconsistent list bounds");
        clo = std::max(clo, G.lo);
        chi = std::min(chi, G.hi);
    }
    if (clo > chi) { *count = 0; return II2_OK; }
    // the driver's union: the candidates
    took(ctx, P_IR_GROUPS);
    size_t drv = 0;
    for (size_t g = 1; g < gs.size(); g++) if (gs[g].n_post < gs[drv].n_post) drv = g;
    const uint64_t half = (gs[drv].n_post + 64) & ~63ull;
    if (int rc = grow_device(ctx, &ctx->d_ir, &ctx->ir_words, 2 * half, 2 * half + half / 2, sizeof(uint32_t), "ii2_intersect_ranges: candidate allocation failed"))
        return rc;
    uint32_t *buf[2] = {ctx->d_ir, ctx->d_ir + half};
    uint64_t nc = 0;
    {
        const GroupIn &D = gs[drv];
        const std::vector<RangeIn> sub(rs.begin() + D.r0, rs.begin() + D.r1);
        if (int rc = union_collected(ctx, sub, D.n_blocks, D.n_nonempty, tomb, buf[0], D.n_post, &nc)) return rc;
    }
    std::vector<size_t> order;
    for (size_t g = 0; g < gs.size(); g++) if (g != drv) order.push_back(g);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return gs[a].n_post < gs[b].n_post; });
    uint32_t src = 0;
    for (size_t k = 0; k < order.size() && nc; k++) {
        const GroupIn &G = gs[order[k]];
        const bool last = k + 1 == order.size();
        const IrPass pass{G.r0, G.r1, G.n_blocks, G.n_nonempty, G.n_post, clo, chi, false};
        if (int rc = ir_filter_pass(ctx, "ii2_intersect_ranges", rs, pass, buf[src], nc, last ? d_out : buf[src ^ 1u], last ? cap : nc, &nc)) return rc;
        if (last && nc > cap) {
            *count = nc;
            return fail(ctx, II2_ECAPACITY, "ii2_intersect_ranges: result does not fit the output buffer (nothing written)");
        }
        src ^= 1u;
    }
    *count = nc;            // (0 when a pass before the last one left no candidate: nothing written)
    return II2_OK;
}

// The groups of a call, checked (`who` names the entry point in the messages): the ranges of group g that own blocks are
// rs[gs[g].r0, gs[g].r1); *n_blocks = the blocks of all of them.  n_groups > 0.
static int collect_groups(ii2_ctx *ctx, const char *who, uint64_t n_groups, const uint64_t *group_first, const ii2_seg *const *segs,
                          const uint64_t *list_first, const uint64_t *list_end, std::vector<RangeIn> &rs, std::vector<GroupIn> &gs, uint64_t *n_blocks) {
    if (!group_first) return fail(ctx, II2_EINVAL, (std::string(who) + ": bad argument").c_str());
    for (uint64_t g = 0; g < n_groups; g++)
        if (group_first[g + 1] < group_first[g]) return fail(ctx, II2_EINVAL, (std::string(who) + ": group_first does not ascend").c_str());
    if (group_first[n_groups] > group_first[0] && (!segs || !list_first || !list_end)) return fail(ctx, II2_EINVAL, (std::string(who) + ": bad argument").c_str());
    gs.resize(n_groups);
    for (uint64_t g = 0; g < n_groups; g++) {
        const uint64_t a = group_first[g], b = group_first[g + 1];
        GroupIn &G = gs[g];
        std::memset(&G, 0, sizeof G);
        G.r0 = rs.size();
        if (int rc = collect_ranges(ctx, who, b - a, segs + a, list_first + a, list_end + a, rs, &G.n_blocks, &G.n_nonempty)) return rc;
        G.r1 = rs.size();
        *n_blocks += G.n_blocks;
    }
    return II2_OK;
}

// postings (the driver, the order of the filters, the hand-off's capacity) and the doc spans mirrored on the host
static int group_sizes(ii2_ctx *ctx, const std::vector<RangeIn> &rs, std::vector<GroupIn> &gs) {
    for (GroupIn &G : gs) {
        G.lo = 0xFFFFFFFFu;
        G.hi = 0;
        G.span_known = true;
        for (size_t r = G.r0; r < G.r1; r++) {
            const ii2_seg *s = rs[r].seg;
            if (int rc = ii2_seg_host_cnt(ctx, s)) return rc;
            const bool mirrored = spans_mirrored(s);
            G.span_known = G.span_known && mirrored;
            for (uint64_t j = rs[r].l0; j < rs[r].l1; j++) {
                if (s->h_blk_off[j + 1] == s->h_blk_off[j]) continue;
                G.n_post += s->h_cnt[j];
                if (!mirrored) continue;
                G.lo = std::min(G.lo, s->h_spans[3 * j]);
                G.hi = std::max(G.hi, s->h_spans[3 * j + 2]);
            }
        }
    }
    return II2_OK;
}

// the doc span the groups whose spans are known have in common (*clo > *chi: none - nothing lies in every group)
static void common_span(const std::vector<GroupIn> &gs, uint32_t *clo, uint32_t *chi) {
    *clo = 0;
    *chi = 0xFFFFFFFFu;
    for (const GroupIn &G : gs) {
        if (!G.span_known) continue;
        *clo = std::max(*clo, G.lo);
        *chi = std::min(*chi, G.hi);
    }
}

// AND of sized groups that all own blocks and whose known spans overlap, d_out != NULL: the first path of the chooser that fits
static int intersect_sized(ii2_ctx *ctx, const std::vector<RangeIn> &rs, std::vector<GroupIn> &gs, const ii2_tomb *tomb, uint32_t *d_out,
                           uint64_t cap, uint64_t *count) {
    const uint64_t n_groups = gs.size();
    if (n_groups == 1) {
        const GroupIn &G = gs[0];
        if (G.r0 == 0 && G.r1 == rs.size()) return union_collected(ctx, rs, G.n_blocks, G.n_nonempty, tomb, d_out, cap, count);
        const std::vector<RangeIn> sub(rs.begin() + G.r0, rs.begin() + G.r1);
        return union_collected(ctx, sub, G.n_blocks, G.n_nonempty, tomb, d_out, cap, count);
    }
    // one non-empty list per group, up to 64 groups, a result that surely fits: the tuned AND (ii2_intersect, look-back repeat included)
    if (!ctx->opt_intersect_ranges && n_groups <= MAX_LISTS) {
        const ii2_seg *hs[MAX_LISTS];
        uint64_t hl[MAX_LISTS];
        uint64_t shortest = ~0ull;
        bool single = true;
        for (uint64_t g = 0; g < n_groups && single; g++) {
            const GroupIn &G = gs[g];
            single = G.n_nonempty == 1;
            for (size_t r = G.r0; r < G.r1 && single; r++)
                for (uint64_t j = rs[r].l0; j < rs[r].l1; j++)
                    if (rs[r].seg->h_blk_off[j + 1] > rs[r].seg->h_blk_off[j]) { hs[g] = rs[r].seg; hl[g] = j; }
            shortest = std::min(shortest, G.n_post);
        }
        if (single && cap >= shortest) {
            took(ctx, P_IR_HANDOFF);
            return intersect_sync(ctx, (uint32_t)n_groups, hs, hl, tomb, d_out, cap, count);
        }
    }
    return intersect_groups(ctx, rs, gs, tomb, d_out, cap, count);
}

static int intersect_ranges_unlocked(ii2_ctx *ctx, uint64_t n_groups, const uint64_t *group_first, const ii2_seg *const *segs,
                                     const uint64_t *list_first, const uint64_t *list_end, const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap,
                                     uint64_t *count) {
    if (n_groups == 0) { *count = 0; return II2_OK; }
    std::vector<RangeIn> rs;
    std::vector<GroupIn> gs;
    uint64_t n_blocks = 0;
    if (int rc = collect_groups(ctx, "ii2_intersect_ranges", n_groups, group_first, segs, list_first, list_end, rs, gs, &n_blocks)) return rc;
    for (const GroupIn &G : gs) if (!G.n_blocks) { *count = 0; return II2_OK; }
    if (n_blocks >= 0xFFFFFFFFull || rs.size() >= 0xFFFFFFFFull) return fail(ctx, II2_ERANGE, "ii2_intersect_ranges: more than 2^32 - 2 blocks in one call");
    if (!d_out) return fail(ctx, II2_EINVAL, "ii2_intersect_ranges: output buffer is NULL");
    if (int rc = group_sizes(ctx, rs, gs)) return rc;
    uint32_t clo, chi;
    common_span(gs, &clo, &chi);
    if (clo > chi) { *count = 0; return II2_OK; }
    return intersect_sized(ctx, rs, gs, tomb, d_out, cap, count);
}

extern "C" int ii2_intersect_ranges(ii2_ctx *ctx, uint64_t n_groups, const uint64_t *group_first, const ii2_seg *const *segs,
                                    const uint64_t *list_first, const uint64_t *list_end, const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap,
                                    uint64_t *count) {
    if (!ctx || !count) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return intersect_ranges_unlocked(ctx, n_groups, group_first, segs, list_first, list_end, tomb, d_out, cap, count);
}

// ---- which groups each doc of an id array lies in ------------------------------------------------------
// The transpose of count_many (explain_ranges.hip): the ids are the marked set, the groups' blocks are walked once and a hit ORs
// its group's bit into its doc's row of d_masks (zeroed first), found through a table of (id, row) built in workspace.  rs are the
// checked ranges that own blocks, group_of the group of each.  At most two waits: the spans and the final read.
static int explain_many(ii2_ctx *ctx, const std::vector<RangeIn> &rs, const std::vector<uint32_t> &group_of, const uint32_t *d_ids, uint64_t n_ids,
                        uint64_t *d_masks, ii2_explain_stats *res) {
    hipStream_t st = ctx->stream;
    uint32_t log2_slots = 6;
    while ((1ull << log2_slots) < 2 * n_ids) log2_slots++;
    const size_t n_slots = (size_t)1 << log2_slots;
    const size_t cnt_bytes = CR_DECODED_SLOTS * (sizeof(uint64_t) + sizeof(uint32_t));      // hits [CR_DECODED_SLOTS] u64, then decoded [CR_DECODED_SLOTS] u32
    ExplainParams q;
    std::memset(&q, 0, sizeof q);
    CountParams &p = q.c;
    p.per_wave = um_per_wave(ctx, res->n_blocks);
    p.set = d_ids;
    p.n_set = n_ids;
    q.masks = (unsigned long long *)d_masks;
    q.log2_slots = log2_slots;
    q.n_words = res->n_words;
    res->log2_slots = log2_slots;
    const MarkedIn m{"ii2_explain_ranges", rs, group_of.data(), res->n_blocks, nullptr, 0, cnt_bytes, align_up(n_slots * sizeof(uint64_t)), nullptr, false};
    const uint8_t *back = nullptr;
    if (int rc = marked_call(ctx, m, p, &res->n_windows, &back,
                             [&](uint8_t *, uint8_t *d_cnt, uint32_t *d_span) {
                                 q.table = ws_take<unsigned long long>(ctx, n_slots);
                                 q.hits = (unsigned long long *)d_cnt;
                                 p.decoded = (uint32_t *)(d_cnt + CR_DECODED_SLOTS * sizeof(uint64_t));
                                 q.span = d_span + 2;
                                 HIP_TRY(ctx, hipMemsetAsync(d_masks, 0, n_ids * res->n_words * sizeof(uint64_t), st));
                                 HIP_TRY(ctx, hipMemsetAsync(q.table, 0xFF, n_slots * sizeof(uint64_t), st));
                                 return II2_OK;
                             },
                             [&]() { return launch_ex_prepare(q, st); },
                             [&](hipEvent_t e0, hipEvent_t e1) { return launch_ex_match(q, st, e0, e1); }))
        return rc;
    if (!back) return II2_OK;                                    // no overlap: the masks are zero and waited for
    const uint64_t *h_hits = (const uint64_t *)back;
    const uint32_t *h_dec = (const uint32_t *)(back + CR_DECODED_SLOTS * sizeof(uint64_t));
    for (uint32_t k = 0; k < CR_DECODED_SLOTS; k++) {
        res->n_hits += h_hits[k];
        res->n_decoded += h_dec[k];
    }
    return II2_OK;
}

// sliced (ii2_explain_batch): the groups are a query's slice of a batch's, so group_first[0] is where its ranges start, not 0
static int explain_ranges_unlocked(ii2_ctx *ctx, uint64_t n_groups, const uint64_t *group_first, const ii2_seg *const *segs, const uint64_t *list_first,
                                   const uint64_t *list_end, const uint32_t *d_ids, uint64_t n_ids, uint64_t *d_masks, uint64_t masks_cap,
                                   ii2_explain_stats *stats, bool sliced = false) {
    const char *who = "ii2_explain_ranges";
    if (n_ids > II2_EXPLAIN_MAX_IDS) return fail(ctx, II2_ERANGE, "ii2_explain_ranges: more than II2_EXPLAIN_MAX_IDS ids in one call (rows are independent: split them)");
    if (n_groups >= 0xFFFFFFFFull) return fail(ctx, II2_ERANGE, "ii2_explain_ranges: 2^32 - 1 groups or more in one call");
    ii2_explain_stats res;
    std::memset(&res, 0, sizeof res);
    res.n_ids = n_ids;
    res.n_words = (uint32_t)((n_groups + 63) / 64);
    std::vector<RangeIn> rs;
    std::vector<uint32_t> group_of;
    if (n_groups) {
        std::vector<GroupIn> gs;
        if (!sliced && group_first && group_first[0] != 0) return fail(ctx, II2_EINVAL, "ii2_explain_ranges: group_first does not ascend from 0");
        if (int rc = collect_groups(ctx, who, n_groups, group_first, segs, list_first, list_end, rs, gs, &res.n_blocks)) return rc;
        if (res.n_blocks >= 0xFFFFFFFFull || rs.size() >= 0xFFFFFFFFull) return fail(ctx, II2_ERANGE, "ii2_explain_ranges: more than 2^32 - 2 blocks in one call");
        for (uint64_t i = group_first[0]; i < group_first[n_groups]; i++) res.n_lists += list_end[i] - list_first[i];
        group_of.resize(rs.size());
        for (uint64_t g = 0; g < n_groups; g++)
            for (size_t r = gs[g].r0; r < gs[g].r1; r++) group_of[r] = (uint32_t)g;
    }
    const uint64_t n_out = n_ids * res.n_words;
    if (n_out && (!d_ids || !d_masks)) return fail(ctx, II2_EINVAL, "ii2_explain_ranges: ids or masks is NULL");
    if (masks_cap < n_out) return fail(ctx, II2_ECAPACITY, "ii2_explain_ranges: masks holds fewer words than ids x words per id (nothing written)");
    if (n_out) {
        if (res.n_blocks) {
            if (int rc = explain_many(ctx, rs, group_of, d_ids, n_ids, d_masks, &res)) return rc;
        } else {                                                // no group owns a block: every mask is 0
            HIP_TRY(ctx, hipMemsetAsync(d_masks, 0, n_out * sizeof(uint64_t), ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
    }
    if (stats) *stats = res;
    return II2_OK;
}

extern "C" int ii2_explain_ranges(ii2_ctx *ctx, uint64_t n_groups, const uint64_t *group_first, const ii2_seg *const *segs, const uint64_t *list_first,
                                  const uint64_t *list_end, const uint32_t *d_ids, uint64_t n_ids, uint64_t *d_masks, uint64_t masks_cap,
                                  ii2_explain_stats *stats) {
    if (!ctx) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return explain_ranges_unlocked(ctx, n_groups, group_first, segs, list_first, list_end, d_ids, n_ids, d_masks, masks_cap, stats);
}

extern "C" int ii2_explain_slot(uint32_t id, uint32_t log2_slots, uint32_t *slot) {
    if (!slot || log2_slots == 0 || log2_slots > 31) return II2_EINVAL;
    *slot = ex_slot(id, log2_slots);
    return II2_OK;
}

// ---- AND of ORs minus excluded groups -----------------------------------------------------------------
// A grouped query as ii2_andnot_ranges and every query of ii2_query_batch_groups plan it (plan_groups, then size_exclusions): the
// two entry points agree on what is empty and on which excluded lists count because this is the only place that decides it.
struct GroupQuery {
    std::vector<RangeIn> rs, rx;            // the ranges of all groups; those of the excluded groups, back to back: ONE logical group
    std::vector<GroupIn> all, req;          // every group; the required ones, sized (group_sizes)
    IrPass ex;                              // the exclusion over rx
    uint64_t shortest;                      // the postings of the smallest required group: no result is longer
    bool req_known;                         // the host mirrors every required group's doc span
    bool empty;                             // no group, a required group without blocks, or required spans that do not overlap
};

// The opening of every plan (plan_groups, plan_atleast): Q reset, then everything that is checked before anything is launched or
// written, and the groups collected into Q.rs / Q.all.  `who` names the entry point in the messages, `per` what its block limit
// counts over ("call" | "query").  group_not == NULL: every group is required.  Q's vectors keep their storage between calls.
// (Inlined into its callers, and they into theirs, like the walk below: out of line they cost the batch 6 ns per query, 3 % at six
// lists a query.)
__attribute__((always_inline)) static inline int plan_open(ii2_ctx *ctx, const char *who, const char *per, uint64_t n_groups, const uint64_t *group_first, const uint8_t *group_not,
                       const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end, GroupQuery &Q) {
    Q.rs.clear();
    Q.rx.clear();
    Q.all.clear();
    Q.req.clear();
    Q.ex = IrPass{0, 0, 0, 0, 0, 0u, 0xFFFFFFFFu, true};
    Q.shortest = ~0ull;
    Q.req_known = true;
    Q.empty = true;
    if (n_groups == 0) return II2_OK;
    uint64_t n_req = 0;
    for (uint64_t g = 0; g < n_groups; g++) {
        if (group_not && group_not[g] > 1) return fail(ctx, II2_EINVAL, (std::string(who) + ": a group_not flag is neither 0 nor 1").c_str());
        n_req += group_not && group_not[g] ? 0u : 1u;
    }
    if (!n_req) return fail(ctx, II2_EINVAL, (std::string(who) + ": no required group (the library has no doc universe to complement)").c_str());
    uint64_t n_blocks = 0;
    if (int rc = collect_groups(ctx, who, n_groups, group_first, segs, list_first, list_end, Q.rs, Q.all, &n_blocks)) return rc;
    if (n_blocks >= 0xFFFFFFFFull || Q.rs.size() >= 0xFFFFFFFFull)
        return fail(ctx, II2_ERANGE, (std::string(who) + ": more than 2^32 - 2 blocks in one " + per).c_str());
    return II2_OK;
}

// The plan of an AND of ORs minus excluded groups: a required group without postings, or required spans that do not overlap, end
// it (Q.empty); the span the excluded lists must meet is the required groups' common one.
__attribute__((always_inline)) static inline int plan_groups(ii2_ctx *ctx, const char *who, const char *per, uint64_t n_groups, const uint64_t *group_first, const uint8_t *group_not,
                       const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end, GroupQuery &Q) {
    if (int rc = plan_open(ctx, who, per, n_groups, group_first, group_not, segs, list_first, list_end, Q); rc || !n_groups) return rc;
    for (uint64_t g = 0; g < n_groups; g++) {
        const GroupIn &G = Q.all[g];
        if (!group_not || !group_not[g]) {
            if (!G.n_blocks) return II2_OK;                             // a required group without postings
            Q.req.push_back(G);
        } else {                                                        // (an excluded group without postings adds nothing)
            Q.rx.insert(Q.rx.end(), Q.rs.begin() + G.r0, Q.rs.begin() + G.r1);
            Q.ex.n_blocks += G.n_blocks;
        }
    }
    Q.ex.r1 = Q.rx.size();
    if (int rc = group_sizes(ctx, Q.rs, Q.req)) return rc;
    // the common span of the REQUIRED groups only: an excluded group never narrows it
    common_span(Q.req, &Q.ex.lo, &Q.ex.hi);
    if (Q.ex.lo > Q.ex.hi) return II2_OK;
    for (const GroupIn &G : Q.req) { Q.shortest = std::min(Q.shortest, G.n_post); Q.req_known = Q.req_known && G.span_known; }
    Q.empty = false;
    return II2_OK;
}

// The excluded lists of a planned query that count - non-empty, their doc span (where the host mirrors it) meeting the required
// groups' common span - sized for the general form; ex.lo / ex.hi shrink to their span where every one is mirrored.  That
// changes nothing about which lists count: a list that meets the common span lies inside the span of all such lists, so it
// meets the narrowed span too, and no other list does - the walk below may run before or after this.
static int size_exclusions(ii2_ctx *ctx, GroupQuery &Q) {
    IrPass &ex = Q.ex;
    uint32_t elo = 0xFFFFFFFFu, ehi = 0;
    bool ex_known = true;
    for (const RangeIn &q : Q.rx) {
        const ii2_seg *s = q.seg;
        if (int rc = ii2_seg_host_cnt(ctx, s)) return rc;
        const bool mirrored = spans_mirrored(s);
        ex_known = ex_known && mirrored;
        for (uint64_t j = q.l0; j < q.l1; j++) {
            if (!ir_list_counts(ex, s, j)) continue;
            ex.n_nonempty++;
            ex.n_post += s->h_cnt[j];
            if (!mirrored) continue;
            elo = std::min(elo, s->h_spans[3 * j]);
            ehi = std::max(ehi, s->h_spans[3 * j + 2]);
        }
    }
    if (ex.n_nonempty && ex_known) { ex.lo = std::max(ex.lo, elo); ex.hi = std::min(ex.hi, ehi); }   // (lo <= hi: every list that counts meets the common span)
    return II2_OK;
}

// the lists, blocks and postings a walk has taken, whether every list it met fitted, and the error that ended it (rc != II2_OK)
struct Counted { uint32_t m, nb; uint64_t sum; bool fits; int rc; };

// The lists of a planned query that count, in the order the one-workgroup kernels want them (setop_groups.hip,
// setop_groups_batch.hip; `mirror`: the context that mirrors the excluded segments' counts on the way, NULL after size_exclusions): the non-empty lists of the required groups, group by group, tag = the group's number; then the
// excluded lists that count, tag = the number of required groups.  put(segment, list, tag, the totals before it) sees each one
// while they fit one workgroup - at most MAX_LISTS regular lists (blocks_full) of SMALL_SET_POSTINGS postings in SMALL_SET_BLOCKS
// blocks; the walk ends at the first list that does not.
template <class F> __attribute__((always_inline)) static inline Counted for_each_counted_list(ii2_ctx *mirror, const GroupQuery &Q, F &&put) {
    Counted t{0, 0, 0, true, II2_OK};
    auto add = [&](const ii2_seg *s, uint64_t j, uint32_t tag) {
        const uint32_t nb = s->h_blk_off[j + 1] - s->h_blk_off[j], c = s->h_cnt[j];
        if (t.m == MAX_LISTS || nb > SMALL_SET_BLOCKS - t.nb || t.sum + c > SMALL_SET_POSTINGS || !blocks_full(nb, c)) { t.fits = false; return; }
        put(s, j, tag, t);
        t.m++;
        t.nb += nb;
        t.sum += c;
    };
    for (size_t g = 0; g < Q.req.size() && t.fits; g++)
        for (size_t r = Q.req[g].r0; r < Q.req[g].r1 && t.fits; r++)
            for (uint64_t j = Q.rs[r].l0; j < Q.rs[r].l1 && t.fits; j++)
                if (Q.rs[r].seg->h_blk_off[j + 1] > Q.rs[r].seg->h_blk_off[j]) add(Q.rs[r].seg, j, (uint32_t)g);
    // (not skipped on ex.n_nonempty == 0: the batch walks without size_exclusions, which fills it; no list counts then anyway)
    for (size_t r = Q.ex.r0; r < Q.ex.r1 && t.fits; r++) {
        if (mirror && (t.rc = ii2_seg_host_cnt(mirror, Q.rx[r].seg))) return t;
        for (uint64_t j = Q.rx[r].l0; j < Q.rx[r].l1 && t.fits; j++)
            if (ir_list_counts(Q.ex, Q.rx[r].seg, j)) add(Q.rx[r].seg, j, (uint32_t)Q.req.size());
    }
    return t;
}

// The one-launch form (setop_groups.hip) of a planned query: the lists that count, when they fit one workgroup.  opt: the
// entry point's option (1: up to ANDNOT_SMALL_WORK postings x lists, 2: up to the kernel's capacity); min_match == 0: an id
// survives in every required group (ii2_andnot_ranges, counted as its path), else in at least min_match of them
// (ii2_atleast_ranges).  *taken = false when the query is too large.
static int groups_one_launch(ii2_ctx *ctx, const GroupQuery &Q, const SetOut &o, int64_t opt, uint32_t min_match, bool *taken) {
    *taken = false;
    if (Q.req.size() > MAX_LISTS) return II2_OK;
    GroupSetParams gp;
    std::memset(&gp, 0, sizeof gp);
    const Counted t = for_each_counted_list(nullptr, Q, [&](const ii2_seg *s, uint64_t j, uint32_t tag, const Counted &at) {
        gp.lists[at.m] = list_view(s, j);
        gp.blk_base[at.m] = at.nb;
        gp.lpre[at.m] = (uint32_t)at.sum;
        gp.tag[at.m] = (uint8_t)tag;
    });
    if (!t.fits) return II2_OK;
    // The kernel ranks every id by one bisection per other list: its time grows with postings x lists, the general form's with
    // the number of groups.  Measured (scripts/andnot_probe.py): at the kernel's capacity, 64 lists x 8000
    // postings, 410 us against the general form's 165 - 180 (four groups).  Sweep, 2 required + 1 excluded group, 4 - 64 lists:
    // ~60 us + 0.68 ns per posting x list against 133 - 145 us - the one-launch form wins every point up to postings x lists =
    // 65 536 (1.3 - 2.2x), ties at ~130 000 and loses beyond.  The limit is deliberately below that crossover: the general
    // form's wait was half as long on another machine of the same kind (63 - 68 us for three groups).
    // (option value 2 lifts the limit to the kernel's capacity: tests, measurements)
    if (opt == 1 && t.sum * t.m > ANDNOT_SMALL_WORK) return II2_OK;
    gp.blk_base[t.m] = t.nb;
    gp.lpre[t.m] = (uint32_t)t.sum;
    gp.n_lists = t.m;
    gp.n_blocks = t.nb;
    gp.n_req = (uint32_t)Q.req.size();
    gp.min_match = min_match;
    set_out(gp, o);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ii2_profile_pair(ctx, &e0, &e1);
    if (!min_match) took(ctx, P_ANDNOT_SMALL);
    HIP_TRY(ctx, min_match ? launch_setop_groups_atleast(gp, ctx->stream, e0, e1) : launch_setop_groups(gp, ctx->stream, e0, e1));
    *taken = true;
    return II2_OK;
}

// ... of ii2_andnot_ranges: when the result surely fits, too.  *taken = false when the query is too large (or option andnot.small is 0).
static int andnot_small(ii2_ctx *ctx, const GroupQuery &Q, const SetOut &o, bool *taken) {
    *taken = false;
    if (!ctx->opt_andnot_small || o.cap < Q.shortest) return II2_OK;
    return groups_one_launch(ctx, Q, o, ctx->opt_andnot_small, 0u, taken);
}

static int andnot_ranges_unlocked(ii2_ctx *ctx, uint64_t n_groups, const uint64_t *group_first, const uint8_t *group_not,
                                  const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end, const ii2_tomb *tomb,
                                  uint32_t *d_out, uint64_t cap, uint64_t *count) {
    if (!group_not) return intersect_ranges_unlocked(ctx, n_groups, group_first, segs, list_first, list_end, tomb, d_out, cap, count);
    // 1. the plan; 2. the excluded lists that count
    GroupQuery Q;
    if (int rc = plan_groups(ctx, "ii2_andnot_ranges", "call", n_groups, group_first, group_not, segs, list_first, list_end, Q)) return rc;
    if (Q.empty) { *count = 0; return II2_OK; }
    if (!d_out) return fail(ctx, II2_EINVAL, "ii2_andnot_ranges: output buffer is NULL");
    if (int rc = size_exclusions(ctx, Q)) return rc;
    uint64_t *d_cnt = ii2_mapped_mail(ctx, II2_MAIL_COUNT);
    // 3. short lists: one launch
    {
        const SetOut o{tomb, d_out, cap, d_cnt ? d_cnt : ctx->d_mail};
        bool taken = false;
        if (int rc = andnot_small(ctx, Q, o, &taken)) return rc;
        if (taken) {
            if (int rc = read_count(ctx, o.d_count, count)) return rc;
            if (*count > cap) return fail(ctx, II2_ECAPACITY, "ii2_andnot_ranges: result does not fit the output buffer (nothing written)");
            return II2_OK;
        }
    }
    // 4. the required part through the AND chooser - straight into d_out when nothing is excluded and the result surely fits,
    // else into the candidate array, which holds the shortest required group: neither a capacity error nor a partly written
    // result can occur there (tombstones are applied here, once)
    took(ctx, P_ANDNOT_GENERAL);
    if (!Q.ex.n_nonempty && cap >= Q.shortest) return intersect_sized(ctx, Q.rs, Q.req, tomb, d_out, cap, count);
    if (int rc = grow_device(ctx, &ctx->d_an, &ctx->an_words, Q.shortest + 1, (size_t)((Q.shortest + 1 + (Q.shortest + 1) / 4 + 63) & ~63ull), sizeof(uint32_t),
                             "ii2_andnot_ranges: candidate allocation failed"))
        return rc;
    uint64_t nc = 0;
    if (int rc = intersect_sized(ctx, Q.rs, Q.req, tomb, ctx->d_an, Q.shortest, &nc)) return rc;
    // 5. one exclusion pass over the candidates into d_out, written only when all survivors fit
    bool pass = nc && Q.ex.n_nonempty;
    if (pass && !Q.req_known) {
        // the candidates' span is not known from the host mirrors: their first and last id bound the mark's windows
        uint32_t *hb = (uint32_t *)(ctx->h_mail + II2_MAIL_COUNT + 1);
        HIP_TRY(ctx, hipMemcpyAsync(hb, ctx->d_an, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(hb + 1, ctx->d_an + (nc - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        Q.ex.lo = std::max(Q.ex.lo, hb[0]);
        Q.ex.hi = std::min(Q.ex.hi, hb[1]);
        pass = Q.ex.lo <= Q.ex.hi;                      // (else no excluded list reaches a candidate)
    }
    if (pass) {
        if (int rc = ir_filter_pass(ctx, "ii2_andnot_ranges", Q.rx, Q.ex, ctx->d_an, nc, d_out, cap, &nc)) return rc;
        *count = nc;
        if (nc > cap) return fail(ctx, II2_ECAPACITY, "ii2_andnot_ranges: result does not fit the output buffer (nothing written)");
        return II2_OK;
    }
    // no candidate, or no excluded list that reaches one: the candidates are the result
    *count = nc;
    if (nc > cap) return fail(ctx, II2_ECAPACITY, "ii2_andnot_ranges: result does not fit the output buffer (nothing written)");
    if (nc) {
        HIP_TRY(ctx, hipMemcpyAsync(d_out, ctx->d_an, nc * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return II2_OK;
}

extern "C" int ii2_andnot_ranges(ii2_ctx *ctx, uint64_t n_groups, const uint64_t *group_first, const uint8_t *group_not,
                                 const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end, const ii2_tomb *tomb,
                                 uint32_t *d_out, uint64_t cap, uint64_t *count) {
    if (!ctx || !count) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return andnot_ranges_unlocked(ctx, n_groups, group_first, group_not, segs, list_first, list_end, tomb, d_out, cap, count);
}

// ---- at least m of n groups -------------------------------------------------------------------------
// The plan of ii2_atleast_ranges, plan_groups' sibling: the same opening under this entry point's name and the same helpers, but a
// required group without postings is dropped, not fatal (Q.req: the n' required groups that have postings, tags 0 .. n' - 1
// in for_each_counted_list), and the span the excluded lists must meet is the required groups' whole span, not their common
// one - a result doc need not lie in every group.  kept: the groups of the call that are left (the AND hand-off's arguments).
// req_weight (the weighted ranked query): the weight of each group of Q.req, group_weight's entry or 1 without one.
static int plan_atleast(ii2_ctx *ctx, const char *who, uint64_t n_groups, const uint64_t *group_first, const uint8_t *group_not,
                        const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end, GroupQuery &Q, std::vector<uint64_t> &kept,
                        const uint32_t *group_weight = nullptr, std::vector<uint32_t> *req_weight = nullptr) {
    kept.clear();
    if (req_weight) req_weight->clear();
    if (int rc = plan_open(ctx, who, "call", n_groups, group_first, group_not, segs, list_first, list_end, Q); rc || !n_groups) return rc;
    for (uint64_t g = 0; g < n_groups; g++) {
        const GroupIn &G = Q.all[g];
        if (!group_not || !group_not[g]) {
            if (!G.n_blocks) continue;                                  // a required group without postings matches no doc
            Q.req.push_back(G);
            if (req_weight) req_weight->push_back(group_weight ? group_weight[g] : 1u);
        } else {                                                        // (an excluded group without postings adds nothing)
            Q.rx.insert(Q.rx.end(), Q.rs.begin() + G.r0, Q.rs.begin() + G.r1);
            Q.ex.n_blocks += G.n_blocks;
        }
        kept.push_back(g);
    }
    Q.ex.r1 = Q.rx.size();
    if (Q.req.empty()) return II2_OK;
    if (int rc = group_sizes(ctx, Q.rs, Q.req)) return rc;
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    for (const GroupIn &G : Q.req) {
        Q.shortest = std::min(Q.shortest, G.n_post);
        Q.req_known = Q.req_known && G.span_known;
        lo = std::min(lo, G.lo);
        hi = std::max(hi, G.hi);
    }
    if (Q.req_known) { Q.ex.lo = lo; Q.ex.hi = hi; }                   // (else every excluded list counts)
    Q.empty = false;
    return II2_OK;
}

// the counter planes + accumulated summary of the largest window of a doc span (grow-only, zeroed when they grow)
static int thr_scratch_reserve(ii2_ctx *ctx, uint32_t n_planes, uint64_t span, uint64_t W) {
    const uint64_t n_sum_call = (std::min(span, W) + 65535) / 65536;
    const size_t words = (size_t)n_planes * n_sum_call * 2048 + n_sum_call;
    if (ctx->thr_words >= words) return II2_OK;
    if (int rc = grow_device(ctx, &ctx->d_thr, &ctx->thr_words, words, words, sizeof(uint32_t), "ii2_atleast_ranges: counter allocation failed")) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_thr, 0, words * sizeof(uint32_t), ctx->stream));
    return II2_OK;
}

// What the counting form and the ranked form (atleast_count, topk_count) share: the descriptors of every required group and of
// the excluded ranges, staged once by group index; the doc span, its windows and the scratch they need; the marks of one window.
// Each form keeps its workspace, the order of its groups, its adds and its passes.
namespace {
struct CountCore {
    ii2_ctx *const ctx;
    const char *const who;                  // the entry point in the messages
    const GroupQuery &Q;
    const size_t n1;                        // required groups
    const bool excl;
    const uint32_t B;                       // counter planes
    const uint64_t W;                       // docs per window
    std::vector<size_t> at;                 // the descriptor block of required group g in the staging; [n1]: the excluded ranges'
    size_t stage_bytes = 0;
    uint8_t *d_stage = nullptr;
    UnionManyParams p;                      // what every mark shares: bounds, the window (set_window), what the form adds
    uint32_t lo = 0xFFFFFFFFu, hi = 0;      // the doc span: what the host mirrors of it (stage), then all of it (resolve)
    uint32_t base = 0;
    uint64_t span = 0, n_win = 0, wlo = 0, whi = 0;
    uint32_t n_marks = 0;                   // the required groups' marks so far

    CountCore(ii2_ctx *c, const char *w, const GroupQuery &q, uint32_t planes)
        : ctx(c), who(w), Q(q), n1(q.req.size()), excl(q.ex.n_nonempty > 0), B(planes), W(thr_window_docs(planes, c->opt_union_many_window_log2)), at(n1 + 1) {
        std::memset(&p, 0, sizeof p);
    }

    // staging: one descriptor block (ranges + block prefix) per required group, then one for all excluded ranges, in the pinned
    // block with `extra` bytes behind them
    int stage(size_t extra) {
        for (size_t g = 0; g < n1; g++) {
            at[g] = stage_bytes;
            stage_bytes += um_desc_bytes(Q.req[g].r1 - Q.req[g].r0);
            if (Q.req[g].span_known) { lo = std::min(lo, Q.req[g].lo); hi = std::max(hi, Q.req[g].hi); }
        }
        at[n1] = stage_bytes;
        if (excl) stage_bytes += um_desc_bytes(Q.rx.size());
        if (int rc = grow_pinned(ctx, &ctx->h_um, &ctx->h_um_cap, stage_bytes + extra, false, (std::string(who) + ": staging allocation failed").c_str())) return rc;
        uint8_t *h = (uint8_t *)ctx->h_um;
        for (size_t g = 0; g < n1; g++) um_desc_fill(Q.rs, Q.req[g].r0, Q.req[g].r1, h + at[g]);
        if (excl) um_desc_fill(Q.rx, 0, Q.rx.size(), h + at[n1]);
        return II2_OK;
    }
    // ... and up, into the workspace the form has reserved (stage_bytes + 256 of it are the core's)
    int upload() {
        d_stage = ws_take<uint8_t>(ctx, stage_bytes);
        p.bounds = ws_take<uint32_t>(ctx, 2);
        HIP_TRY(ctx, hipMemcpyAsync(d_stage, ctx->h_um, stage_bytes, hipMemcpyHostToDevice, ctx->stream));
        return II2_OK;
    }
    // the descriptors of required group g (n1: the excluded ranges) in a copy of p
    UnionManyParams group_params(size_t g) const {
        const size_t nr = g < n1 ? Q.req[g].r1 - Q.req[g].r0 : Q.rx.size();
        const uint64_t n_blocks = g < n1 ? Q.req[g].n_blocks : Q.ex.n_blocks;
        UnionManyParams q = p;
        q.ranges = (const UmRange *)(d_stage + at[g]);
        q.pre = (const uint32_t *)(d_stage + at[g] + align_up(nr * sizeof(UmRange)));
        q.n_ranges = (uint32_t)nr;
        q.n_blocks = (uint32_t)n_blocks;
        q.per_wave = um_per_wave(ctx, n_blocks);
        return q;
    }
    // The doc span of the required groups: from the mirrored spans, else one reduction over the group's blocks and a wait.  Then
    // its windows and the scratch: bitmap + summary and planes + accumulated summary of the largest window, zero.
    int resolve() {
        hipStream_t st = ctx->stream;
        if (!Q.req_known) {
            HIP_TRY(ctx, hipMemsetAsync(p.bounds, 0xFF, sizeof(uint32_t), st));
            HIP_TRY(ctx, hipMemsetAsync(p.bounds + 1, 0, sizeof(uint32_t), st));
            for (size_t g = 0; g < n1; g++)
                if (!Q.req[g].span_known) HIP_TRY(ctx, launch_union_many_bounds(group_params(g), st));
            uint32_t *hb = (uint32_t *)(ctx->h_mail + II2_MAIL_COUNT + 1);
            HIP_TRY(ctx, hipMemcpyAsync(hb, p.bounds, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
            lo = std::min(lo, hb[0]);
            hi = std::max(hi, hb[1]);
        }
        if (lo > hi) return fail(ctx, II2_EINVAL, (std::string(who) + ": inconsistent list bounds").c_str());
        base = lo & ~31u;
        span = (uint64_t)hi - base + 1;
        n_win = (span + W - 1) / W;
        p.check_window = n_win > 1 ? 1u : 0u;
        if (int rc = um_scratch_reserve(ctx, who, span, W)) return rc;
        return thr_scratch_reserve(ctx, B, span, W);
    }
    // window w of the doc span in p
    void set_window(uint64_t w) {
        wlo = base + w * W;
        const uint64_t docs = std::min<uint64_t>(W, (uint64_t)hi - wlo + 1);
        whi = wlo + docs - 1;
        p.window = (uint32_t)w;
        um_set_window(ctx, p, wlo, docs);
    }
    // ... marked: every required group that can meet it, in the form's order, each followed by add(its place in the order, the
    // group); then the excluded lists, left in the bitmap
    template <class Add> int mark_window(const std::vector<size_t> &order, Add &&add) {
        for (size_t k = 0; k < order.size(); k++) {
            const GroupIn &G = Q.req[order[k]];
            if (G.span_known && (G.hi < wlo || G.lo > whi)) continue;          // none of the group's docs lies in this window
            HIP_TRY(ctx, launch_union_many_mark(group_params(order[k]), ctx->stream));
            if (int rc = add(k, order[k])) return rc;
            n_marks++;
        }
        if (excl) {
            UnionManyParams x = group_params(n1);
            x.check_window = 1u;                                            // blocks outside the required groups' span are not decoded
            HIP_TRY(ctx, launch_union_many_mark(x, ctx->stream));
        }
        return II2_OK;
    }
};
}  // namespace

// the window of p in the params of a counting kernel: G and its summary, the B planes and the accumulated summary behind them
template <class P> static void set_planes(P &t, const UnionManyParams &p, uint32_t *planes, uint32_t B) {
    t.bitmap = p.bitmap;
    t.summary = p.summary;
    t.plane_words = p.n_sum * 2048u;
    t.planes = planes;
    t.acc = planes + (size_t)B * t.plane_words;
    t.n_sum = p.n_sum;
    t.n_planes = B;
}

// The counting form (atleast.hip) of a planned query, order: its required groups in ascending order of postings.  Per window of
// the doc span and group: mark (union_many.hip), add; then the excluded lists' mark, select, and the block-wise OR's count, scan
// and compact.  The descriptors of all groups are staged once.  At most two waits: the bounds of spans the host does not mirror,
// and the count.
static int atleast_count(ii2_ctx *ctx, GroupQuery &Q, const std::vector<size_t> &order, uint32_t min_match, const ii2_tomb *tomb, uint32_t *d_out,
                         uint64_t cap, uint64_t *count, ii2_atleast_stats &stats) {
    hipStream_t st = ctx->stream;
    const size_t n1 = order.size();
    const uint32_t B = thr_bit_width(min_match);
    const size_t first_late = n1 - min_match + 1;
    if (int rc = um_scratch_clean(ctx)) return rc;
    CountCore C(ctx, "ii2_atleast_ranges", Q, B);
    if (int rc = C.stage(0)) return rc;
    const uint64_t n_sum_max = (C.W + 65535) / 65536;
    UnionManyParams &p = C.p;
    const size_t scan_tmp = scan_temp_bytes(n_sum_max + 1);
    if (int rc = ii2_ws_reserve(ctx, C.stage_bytes + 2 * align_up((n_sum_max + 1) * sizeof(uint64_t)) + scan_tmp + 2 * 256 + 4096)) return rc;
    p.cnt = ws_take<uint32_t>(ctx, n_sum_max + 1);
    p.off = ws_take<uint64_t>(ctx, n_sum_max + 1);
    void *d_scan = ws_take<uint8_t>(ctx, scan_tmp);
    p.run = ws_take<uint64_t>(ctx, 2);
    ctx->um_dirty = true;
    if (int rc = C.upload()) return rc;
    if (int rc = C.resolve()) return rc;
    uint64_t *d_cnt = ii2_mapped_mail(ctx, II2_MAIL_COUNT);
    p.d_count = d_cnt ? d_cnt : ctx->d_mail;
    set_tomb(p, tomb);
    p.out = d_out;
    p.out_cap = cap;
    stats.form = II2_ATLEAST_COUNT;
    stats.n_planes = B;
    stats.n_windows = (uint32_t)C.n_win;
    stats.n_late = (uint32_t)(n1 - first_late);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ii2_profile_pair(ctx, &e0, &e1);
    // several windows whose result may not fit: count first (nothing written), then write
    const bool count_first = C.n_win > 1 && cap < stats.bound;
    for (int pass = count_first ? 0 : 1; pass < 2; pass++) {
        p.write = (uint32_t)pass;
        for (uint64_t w = 0; w < C.n_win; w++) {
            C.set_window(w);
            const uint32_t grid = (uint32_t)std::min<uint64_t>((p.n_sum + 1 + 3) / 4, (uint64_t)ctx->cu_count * 8u);
            ThrParams t;
            std::memset(&t, 0, sizeof t);
            set_planes(t, p, ctx->d_thr, B);
            t.min_match = min_match;
            if (int rc = C.mark_window(order, [&](size_t k, size_t) -> int {
                    t.late = k >= first_late ? 1u : 0u;
                    HIP_TRY(ctx, launch_thr_add(t, grid, st, e0, e1));
                    e0 = e1 = nullptr;
                    return II2_OK;
                }))
                return rc;
            HIP_TRY(ctx, launch_thr_select(t, grid, st));
            HIP_TRY(ctx, launch_union_many_count(p, grid, st));
            HIP_TRY(ctx, scan_excl_u32_to_u64(d_scan, scan_tmp, p.cnt, p.off, p.n_sum + 1, st));
            HIP_TRY(ctx, launch_union_many_compact(p, grid, st));
        }
        if (int rc = read_count(ctx, p.d_count, count)) return rc;
        ctx->um_dirty = false;
        if (*count > cap) return fail(ctx, II2_ECAPACITY, "ii2_atleast_ranges: result does not fit the output buffer (nothing written)");
        if (pass == 0) ctx->um_dirty = true;
    }
    return II2_OK;
}

static int atleast_ranges_unlocked(ii2_ctx *ctx, uint64_t n_groups, const uint64_t *group_first, const uint8_t *group_not, uint32_t min_match,
                                   const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end, const ii2_tomb *tomb,
                                   uint32_t *d_out, uint64_t cap, uint64_t *count, ii2_atleast_stats *stats) {
    if (!min_match) return fail(ctx, II2_EINVAL, "ii2_atleast_ranges: min_match is 0");
    // 1. the plan: n' required groups with postings, in ascending order of postings; the bound
    GroupQuery Q;
    std::vector<uint64_t> kept;
    if (int rc = plan_atleast(ctx, "ii2_atleast_ranges", n_groups, group_first, group_not, segs, list_first, list_end, Q, kept)) return rc;
    const size_t n1 = Q.req.size();
    ii2_atleast_stats st{n1, 0, II2_ATLEAST_NONE, 0, 0, 0};
    if (Q.empty || min_match > n1) {
        *count = 0;
        if (stats) *stats = st;
        return II2_OK;
    }
    std::vector<size_t> order(n1);
    for (size_t g = 0; g < n1; g++) order[g] = g;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return Q.req[a].n_post < Q.req[b].n_post; });
    for (size_t k = 0; k + min_match <= n1; k++) st.bound += Q.req[order[k]].n_post;
    const bool is_and = min_match == n1;
    if (!is_and && min_match > 255) return fail(ctx, II2_ERANGE, "ii2_atleast_ranges: min_match above 255 and below the number of required groups with postings");
    if (!d_out) return fail(ctx, II2_EINVAL, "ii2_atleast_ranges: output buffer is NULL");
    // 2. the excluded lists that count
    if (int rc = size_exclusions(ctx, Q)) return rc;
    auto done = [&](int rc) {
        if (stats && (rc == II2_OK || rc == II2_ECAPACITY)) *stats = st;
        return rc;
    };
    // 3. the hand-offs: every group - ii2_andnot_ranges on the groups that are left; any group, nothing excluded - the OR
    if (is_and && (ctx->opt_atleast_handoff || min_match > 255)) {
        st.form = II2_ATLEAST_AND;
        if (kept.size() == n_groups) return done(andnot_ranges_unlocked(ctx, n_groups, group_first, group_not, segs, list_first, list_end, tomb, d_out, cap, count));
        std::vector<uint64_t> gf{0}, lf, le;
        std::vector<uint8_t> gn;
        std::vector<const ii2_seg *> gsegs;
        for (uint64_t g : kept) {
            gsegs.insert(gsegs.end(), segs + group_first[g], segs + group_first[g + 1]);
            lf.insert(lf.end(), list_first + group_first[g], list_first + group_first[g + 1]);
            le.insert(le.end(), list_end + group_first[g], list_end + group_first[g + 1]);
            gf.push_back(gsegs.size());
            gn.push_back(group_not ? group_not[g] : 0);
        }
        return done(andnot_ranges_unlocked(ctx, kept.size(), gf.data(), group_not ? gn.data() : nullptr, gsegs.data(), lf.data(), le.data(), tomb, d_out, cap, count));
    }
    if (min_match == 1 && !Q.ex.n_nonempty && ctx->opt_atleast_handoff) {
        st.form = II2_ATLEAST_OR;
        std::vector<RangeIn> rr;
        uint64_t n_blocks = 0, n_nonempty = 0;
        for (const GroupIn &G : Q.req) {
            rr.insert(rr.end(), Q.rs.begin() + G.r0, Q.rs.begin() + G.r1);
            n_blocks += G.n_blocks;
            n_nonempty += G.n_nonempty;
        }
        return done(union_collected(ctx, rr, n_blocks, n_nonempty, tomb, d_out, cap, count));
    }
    // 4. short lists: one launch
    if (ctx->opt_atleast_small) {
        uint64_t *d_cnt = ii2_mapped_mail(ctx, II2_MAIL_COUNT);
        const SetOut o{tomb, d_out, cap, d_cnt ? d_cnt : ctx->d_mail};
        bool taken = false;
        if (int rc = groups_one_launch(ctx, Q, o, ctx->opt_atleast_small, min_match, &taken)) return rc;
        if (taken) {
            if (int rc = read_count(ctx, o.d_count, count)) return rc;
            st.form = II2_ATLEAST_SMALL;
            if (*count > cap) return done(fail(ctx, II2_ECAPACITY, "ii2_atleast_ranges: result does not fit the output buffer (nothing written)"));
            return done(II2_OK);
        }
    }
    // 5. the counting form
    return done(atleast_count(ctx, Q, order, min_match, tomb, d_out, cap, count, st));
}

// ---- the k docs in the most groups --------------------------------------------------------------------
// The ranked form (topk.hip) of a planned query: atleast_count's marks and adds with B = bit_width(n') planes - an exact counter per
// doc - and then, instead of the select, pass 1 (the score histogram; read back and cut for k on the host) and pass 2 (count
// table, scan, emit in rank order).  One window: the planes stay between the passes and every group is marked once.  Several:
// pass 1 cleans up behind each window and pass 2 marks and adds again.  Waits: the bounds of spans the host does not mirror, the
// histogram, the end of pass 2.  Everything the caller sees is written after the last of them.
// weights == NULL: ii2_topk_ranges - a doc's score is the number of its groups, every add is atleast.hip's.  Else (`who` is
// ii2_topk_weighted_ranges) weights[g] is the weight of Q.req[g] and late[g] whether it is added in late mode: B = bit_width(W'),
// the early groups come first and the late ones after them, every mark is followed by topk.hip's weighted add, and *n_late counts
// the late groups.  min_match is the lowest eligible score in both.
static int topk_count(ii2_ctx *ctx, const char *who, GroupQuery &Q, uint32_t min_match, uint64_t k, const ii2_tomb *tomb, uint32_t *d_ids, uint32_t *d_scores,
                      uint64_t *count, uint64_t *hist, ii2_topk_stats &stats, const uint32_t *weights = nullptr, const uint8_t *late = nullptr,
                      uint32_t *n_late = nullptr) {
    hipStream_t st = ctx->stream;
    const size_t n1 = Q.req.size();
    const std::string name(who);
    uint64_t top = n1;                                                      // the highest score a doc can reach
    std::vector<size_t> order(n1);
    for (size_t g = 0; g < n1; g++) order[g] = g;
    if (weights) {
        top = 0;
        for (size_t g = 0; g < n1; g++) top += weights[g];
        std::stable_partition(order.begin(), order.end(), [&](size_t g) { return !late[g]; });
        *n_late = (uint32_t)std::count(late, late + n1, (uint8_t)1);
    }
    const uint32_t B = thr_bit_width(top);
    if (int rc = um_scratch_clean(ctx)) return rc;
    // staging: the descriptors, then the histogram on its way down
    CountCore C(ctx, who, Q, B);
    if (int rc = C.stage(TOPK_SCORES * sizeof(uint64_t))) return rc;
    uint64_t *h_hist = (uint64_t *)((uint8_t *)ctx->h_um + C.stage_bytes);
    // workspace, sized before the bounds are known: the count table holds a class per score min_match .. n' and a column per
    // summary word of the largest window
    uint64_t n_sum_max = (C.W + 65535) / 65536;
    if (Q.req_known && C.lo <= C.hi) n_sum_max = std::min<uint64_t>(n_sum_max, (std::min<uint64_t>((uint64_t)C.hi - (C.lo & ~31u) + 1, C.W) + 65535) / 65536);
    const size_t table_max = (size_t)(top - min_match + 1) * n_sum_max + 1;
    const size_t scan_tmp = scan_temp_bytes(table_max);
    if (int rc = ii2_ws_reserve(ctx, C.stage_bytes + align_up(table_max * sizeof(uint32_t)) + align_up(table_max * sizeof(uint64_t)) + scan_tmp +
                                         4 * align_up(TOPK_SCORES * sizeof(uint64_t)) + 256 + 4096))
        return rc;
    UnionManyParams &p = C.p;
    TopParams t;
    std::memset(&t, 0, sizeof t);
    t.cnt = ws_take<uint32_t>(ctx, table_max);
    t.off = ws_take<uint64_t>(ctx, table_max);
    void *d_scan = ws_take<uint8_t>(ctx, scan_tmp);
    t.hist = ws_take<uint64_t>(ctx, TOPK_SCORES);
    t.base = ws_take<uint64_t>(ctx, TOPK_SCORES);
    t.run = ws_take<uint64_t>(ctx, 2 * TOPK_SCORES);
    ctx->um_dirty = true;
    if (int rc = C.upload()) return rc;
    HIP_TRY(ctx, hipMemsetAsync(t.hist, 0, TOPK_SCORES * sizeof(uint64_t), st));
    if (int rc = C.resolve()) return rc;
    const uint64_t n_win = C.n_win;
    set_tomb(t, tomb);
    t.min_match = min_match;
    t.k = k;
    t.ids = d_ids;
    t.scores = d_scores;
    hipEvent_t e0 = nullptr, e1 = nullptr, f0 = nullptr, f1 = nullptr;
    ii2_profile_pair(ctx, &e0, &e1);
    // window w of the doc span in p and t; every required group that can meet it marked and added, the excluded lists left in G
    uint32_t grid = 0;
    auto count_window = [&](uint64_t w) -> int {
        C.set_window(w);
        grid = (uint32_t)std::min<uint64_t>((p.n_sum + 3) / 4, (uint64_t)ctx->cu_count * 8u);
        ThrParams a;
        std::memset(&a, 0, sizeof a);
        TopAddParams wa;
        std::memset(&wa, 0, sizeof wa);
        set_planes(a, p, ctx->d_thr, B);
        set_planes(wa, p, ctx->d_thr, B);
        set_planes(t, p, ctx->d_thr, B);
        a.min_match = min_match;
        t.win_lo = p.win_lo;
        t.window = p.window;
        return C.mark_window(order, [&](size_t, size_t g) -> int {
            if (weights) {
                wa.weight = weights[g];
                wa.late = late[g];
                HIP_TRY(ctx, launch_top_add(wa, grid, st));
            } else {
                HIP_TRY(ctx, launch_thr_add(a, grid, st));
            }
            return II2_OK;
        });
    };
    // pass 1: the histogram of the eligible docs' scores
    for (uint64_t w = 0; w < n_win; w++) {
        if (int rc = count_window(w)) return rc;
        t.clear = n_win > 1 || !k ? 1u : 0u;
        HIP_TRY(ctx, launch_top_hist(t, std::min<uint32_t>(grid, (uint32_t)ctx->cu_count * 2u), st, e0, e1));
        e0 = e1 = nullptr;
    }
    if (k) HIP_TRY(ctx, launch_top_base(t, st));
    HIP_TRY(ctx, hipMemcpyAsync(h_hist, t.hist, TOPK_SCORES * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    uint64_t n_eligible = 0, n_above = 0;
    for (uint32_t s = 0; s < TOPK_SCORES; s++) n_eligible += h_hist[s];
    top_cut(h_hist, k, &stats.max_score, &stats.cut_score, &n_above, &stats.n_cut);
    // pass 2: the classes cut_score .. max_score, counted per summary word, scanned and placed
    const bool emit = k && n_eligible;
    t.cut_score = stats.cut_score;
    t.n_cls = emit ? stats.max_score - stats.cut_score + 1u : 0u;
    t.n_cut = stats.n_cut;
    if (emit || (n_win == 1 && k)) {                                        // (nothing eligible behind one window: its planes are still set)
        ii2_profile_pair(ctx, &f0, &f1);
        for (uint64_t w = 0; w < (emit ? n_win : 1); w++) {
            if (n_win > 1) {
                if (int rc = count_window(w)) return rc;
            }
            if (emit) {
                if ((size_t)t.n_cls * p.n_sum + 1 > table_max) return fail(ctx, II2_EINVAL, (name + ": inconsistent count table").c_str());
                HIP_TRY(ctx, launch_top_count(t, grid, st));
                HIP_TRY(ctx, scan_excl_u32_to_u64(d_scan, scan_tmp, t.cnt, t.off, (size_t)t.n_cls * p.n_sum + 1, st));
            }
            HIP_TRY(ctx, launch_top_emit(t, grid, st, f0, f1));
            f0 = f1 = nullptr;
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    ctx->um_dirty = false;
    stats.n_eligible = n_eligible;
    stats.n_planes = B;
    stats.n_windows = (uint32_t)n_win;
    stats.n_marks = C.n_marks;
    if (hist) std::memcpy(hist, h_hist, TOPK_SCORES * sizeof(uint64_t));
    *count = std::min(k, n_eligible);
    return II2_OK;
}

static int topk_ranges_unlocked(ii2_ctx *ctx, uint64_t n_groups, const uint64_t *group_first, const uint8_t *group_not, uint32_t min_match, uint64_t k,
                                const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end, const ii2_tomb *tomb, uint32_t *d_ids,
                                uint32_t *d_scores, uint64_t *count, uint64_t *hist, ii2_topk_stats *stats) {
    if (!min_match) return fail(ctx, II2_EINVAL, "ii2_topk_ranges: min_match is 0");
    if (k > II2_TOPK_MAX) return fail(ctx, II2_ERANGE, "ii2_topk_ranges: k above II2_TOPK_MAX (ii2_atleast_ranges returns every doc)");
    GroupQuery Q;
    std::vector<uint64_t> kept;
    if (int rc = plan_atleast(ctx, "ii2_topk_ranges", n_groups, group_first, group_not, segs, list_first, list_end, Q, kept)) return rc;
    const size_t n1 = Q.req.size();
    if (n1 > 255) return fail(ctx, II2_ERANGE, "ii2_topk_ranges: more than 255 required groups with postings (the scores are exact 8-bit counters)");
    ii2_topk_stats st;
    std::memset(&st, 0, sizeof st);
    st.n_counted = n1;
    if (Q.empty || min_match > n1) {
        *count = 0;
        if (hist) std::memset(hist, 0, TOPK_SCORES * sizeof(uint64_t));
        if (stats) *stats = st;
        return II2_OK;
    }
    if (k && !d_ids) return fail(ctx, II2_EINVAL, "ii2_topk_ranges: output buffer is NULL");
    if (int rc = size_exclusions(ctx, Q)) return rc;
    if (int rc = topk_count(ctx, "ii2_topk_ranges", Q, min_match, k, tomb, d_ids, d_scores, count, hist, st)) return rc;
    if (stats) *stats = st;
    return II2_OK;
}

// The checks and the plan of the weighted ranked query - ii2_topk_ranges' with a weight per counted group - under the name `who`:
// ii2_topk_weighted_ranges and every query of ii2_topk_batch go through here, so the two entry points reject the same things
// with the same codes.  weights: those of Q.req (plan_atleast), *total their sum W'.
static int topkw_plan(ii2_ctx *ctx, const char *who, uint64_t n_groups, const uint64_t *group_first, const uint8_t *group_not, const uint32_t *group_weight,
                      uint32_t min_score, uint64_t k, const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end, GroupQuery &Q,
                      std::vector<uint64_t> &kept, std::vector<uint32_t> &weights, uint64_t *total) {
    const std::string name(who);
    if (!min_score) return fail(ctx, II2_EINVAL, (name + ": min_score is 0").c_str());
    if (k > II2_TOPK_MAX) return fail(ctx, II2_ERANGE, (name + ": k above II2_TOPK_MAX (ii2_atleast_ranges returns every doc)").c_str());
    if (int rc = plan_atleast(ctx, who, n_groups, group_first, group_not, segs, list_first, list_end, Q, kept, group_weight, &weights)) return rc;
    for (uint64_t g = 0; group_weight && g < n_groups; g++) {
        if (group_not && group_not[g]) continue;                            // an excluded group's weight is ignored
        if (!group_weight[g]) return fail(ctx, II2_EINVAL, (name + ": required group " + std::to_string(g) + " has weight 0 (drop the group instead)").c_str());
        if (group_weight[g] > 255) return fail(ctx, II2_ERANGE, (name + ": the weight of required group " + std::to_string(g) + " is above 255").c_str());
    }
    *total = 0;
    for (uint32_t w : weights) *total += w;
    if (*total > 255) return fail(ctx, II2_ERANGE, (name + ": the weights of the required groups with postings sum to more than 255 (the scores are exact 8-bit values)").c_str());
    return II2_OK;
}

// ii2_topk_weighted_ranges: the plan above, then ii2_topk_ranges' ranked form
static int topkw_ranges_unlocked(ii2_ctx *ctx, uint64_t n_groups, const uint64_t *group_first, const uint8_t *group_not, const uint32_t *group_weight,
                                 uint32_t min_score, uint64_t k, const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end,
                                 const ii2_tomb *tomb, uint32_t *d_ids, uint32_t *d_scores, uint64_t *count, uint64_t *hist, ii2_topkw_stats *stats) {
    static const char who[] = "ii2_topk_weighted_ranges";
    const std::string name(who);
    GroupQuery Q;
    std::vector<uint64_t> kept;
    std::vector<uint32_t> weights;
    uint64_t total = 0;
    if (int rc = topkw_plan(ctx, who, n_groups, group_first, group_not, group_weight, min_score, k, segs, list_first, list_end, Q, kept, weights, &total)) return rc;
    const size_t n1 = Q.req.size();
    ii2_topkw_stats st;
    std::memset(&st, 0, sizeof st);
    st.n_counted = n1;
    st.total_weight = (uint32_t)total;
    if (Q.empty || min_score > total) {
        *count = 0;
        if (hist) std::memset(hist, 0, TOPK_SCORES * sizeof(uint64_t));
        if (stats) *stats = st;
        return II2_OK;
    }
    if (k && !d_ids) return fail(ctx, II2_EINVAL, (name + ": output buffer is NULL").c_str());
    if (int rc = size_exclusions(ctx, Q)) return rc;
    std::vector<uint64_t> postings(n1);
    for (size_t g = 0; g < n1; g++) postings[g] = Q.req[g].n_post;
    std::vector<uint8_t> late(n1, 0);
    if (ctx->opt_topk_late) top_late_set(n1, weights.data(), postings.data(), min_score, late.data());
    ii2_topk_stats ts;
    std::memset(&ts, 0, sizeof ts);
    if (int rc = topk_count(ctx, who, Q, min_score, k, tomb, d_ids, d_scores, count, hist, ts, weights.data(), late.data(), &st.n_late)) return rc;
    st.n_eligible = ts.n_eligible;
    st.n_cut = ts.n_cut;
    st.max_score = ts.max_score;
    st.cut_score = ts.cut_score;
    st.n_planes = ts.n_planes;
    st.n_windows = ts.n_windows;
    st.n_marks = ts.n_marks;
    if (stats) *stats = st;
    return II2_OK;
}

// the counters of the 32 docs of a word after adding adds[0, n_adds) into B zero planes, read back as the kernels read a score
template <uint32_t B> static void top_word_scores(const uint32_t *adds, uint32_t n_adds, uint32_t mask, uint32_t *scores) {
    uint32_t pl[B] = {};
    for (uint32_t i = 0; i < n_adds; i++) thr_add_word<B>(pl, adds[i]);
    for (uint32_t bit = 0; bit < 32; bit++) scores[bit] = (mask >> bit) & 1u ? top_score<B>(pl, bit) : 0u;
}

// ... after adding weights[i] to the docs of adds[i], as the weighted form's kernel does (ii2_topkw_word)
template <uint32_t B> static void topw_word_scores(const uint32_t *adds, const uint32_t *weights, uint32_t n_adds, uint32_t mask, uint32_t *scores) {
    uint32_t pl[B] = {};
    for (uint32_t i = 0; i < n_adds; i++) top_add_weighted<B>(pl, adds[i], weights[i]);
    for (uint32_t bit = 0; bit < 32; bit++) scores[bit] = (mask >> bit) & 1u ? top_score<B>(pl, bit) : 0u;
}

// the >= min_match mask after adding adds[0, n_adds) into B zero planes (ii2_atleast_word)
template <uint32_t B> static uint32_t thr_word_mask(uint32_t min_match, const uint32_t *adds, uint32_t n_adds) {
    uint32_t pl[B] = {};
    for (uint32_t i = 0; i < n_adds; i++) thr_add_word<B>(pl, adds[i]);
    return thr_ge_word<B>(pl, min_match);
}

extern "C" {

int ii2_atleast_ranges(ii2_ctx *ctx, uint64_t n_groups, const uint64_t *group_first, const uint8_t *group_not, uint32_t min_match,
                       const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end, const ii2_tomb *tomb, uint32_t *d_out,
                       uint64_t cap, uint64_t *count, ii2_atleast_stats *stats) {
    if (!ctx || !count) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return atleast_ranges_unlocked(ctx, n_groups, group_first, group_not, min_match, segs, list_first, list_end, tomb, d_out, cap, count, stats);
}

// host only: what the counting form would use for a query of n_counted required groups with postings
int ii2_atleast_plan(uint64_t n_counted, uint32_t min_match, uint32_t window_log2, uint32_t *n_planes, uint64_t *window_docs, uint64_t *first_late) {
    if (!n_planes || !window_docs || !first_late || !min_match) return II2_EINVAL;
    *n_planes = 0;
    *window_docs = 0;
    *first_late = 0;
    if (min_match > n_counted) return II2_OK;
    if (min_match > 255) return min_match < n_counted ? II2_ERANGE : II2_OK;
    *n_planes = thr_bit_width(min_match);
    *window_docs = thr_window_docs(*n_planes, window_log2);
    *first_late = n_counted - min_match + 1;
    return II2_OK;
}

// host only: the kernels' word arithmetic
int ii2_atleast_word(uint32_t n_planes, uint32_t min_match, const uint32_t *adds, uint32_t n_adds, uint32_t *mask) {
    if (!mask || (n_adds && !adds) || n_planes < 1 || n_planes > THR_MAX_PLANES || !min_match || (min_match >> n_planes)) return II2_EINVAL;
    switch (n_planes) {
        case 1: *mask = thr_word_mask<1>(min_match, adds, n_adds); break;
        case 2: *mask = thr_word_mask<2>(min_match, adds, n_adds); break;
        case 3: *mask = thr_word_mask<3>(min_match, adds, n_adds); break;
        case 4: *mask = thr_word_mask<4>(min_match, adds, n_adds); break;
        case 5: *mask = thr_word_mask<5>(min_match, adds, n_adds); break;
        case 6: *mask = thr_word_mask<6>(min_match, adds, n_adds); break;
        case 7: *mask = thr_word_mask<7>(min_match, adds, n_adds); break;
        default: *mask = thr_word_mask<8>(min_match, adds, n_adds); break;
    }
    return II2_OK;
}

int ii2_topk_ranges(ii2_ctx *ctx, uint64_t n_groups, const uint64_t *group_first, const uint8_t *group_not, uint32_t min_match, uint64_t k,
                    const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end, const ii2_tomb *tomb, uint32_t *d_ids,
                    uint32_t *d_scores, uint64_t *count, uint64_t *hist, ii2_topk_stats *stats) {
    if (!ctx || !count) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return topk_ranges_unlocked(ctx, n_groups, group_first, group_not, min_match, k, segs, list_first, list_end, tomb, d_ids, d_scores, count, hist, stats);
}

// host only: the cut of a score histogram for k
int ii2_topk_cut(const uint64_t *hist, uint64_t k, uint32_t *max_score, uint32_t *cut_score, uint64_t *n_above, uint64_t *n_cut) {
    if (!hist || !max_score || !cut_score || !n_above || !n_cut) return II2_EINVAL;
    top_cut(hist, k, max_score, cut_score, n_above, n_cut);
    return II2_OK;
}

// host only: the kernels' score extraction
int ii2_topk_word(uint32_t n_planes, const uint32_t *adds, uint32_t n_adds, uint32_t mask, uint32_t *scores) {
    if (!scores || (n_adds && !adds) || n_planes < 1 || n_planes > THR_MAX_PLANES) return II2_EINVAL;
    switch (n_planes) {
        case 1: top_word_scores<1>(adds, n_adds, mask, scores); break;
        case 2: top_word_scores<2>(adds, n_adds, mask, scores); break;
        case 3: top_word_scores<3>(adds, n_adds, mask, scores); break;
        case 4: top_word_scores<4>(adds, n_adds, mask, scores); break;
        case 5: top_word_scores<5>(adds, n_adds, mask, scores); break;
        case 6: top_word_scores<6>(adds, n_adds, mask, scores); break;
        case 7: top_word_scores<7>(adds, n_adds, mask, scores); break;
        default: top_word_scores<8>(adds, n_adds, mask, scores); break;
    }
    return II2_OK;
}

int ii2_topk_weighted_ranges(ii2_ctx *ctx, uint64_t n_groups, const uint64_t *group_first, const uint8_t *group_not, const uint32_t *group_weight,
                             uint32_t min_score, uint64_t k, const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end,
                             const ii2_tomb *tomb, uint32_t *d_ids, uint32_t *d_scores, uint64_t *count, uint64_t *hist, ii2_topkw_stats *stats) {
    if (!ctx || !count) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return topkw_ranges_unlocked(ctx, n_groups, group_first, group_not, group_weight, min_score, k, segs, list_first, list_end, tomb, d_ids, d_scores, count,
                                 hist, stats);
}

// host only: the weighted add and the score extraction of the kernels
int ii2_topkw_word(uint32_t n_planes, const uint32_t *adds, const uint32_t *weights, uint32_t n_adds, uint32_t mask, uint32_t *scores) {
    if (!scores || (n_adds && (!adds || !weights)) || n_planes < 1 || n_planes > THR_MAX_PLANES) return II2_EINVAL;
    for (uint32_t i = 0; i < n_adds; i++)
        if (!weights[i] || weights[i] > 255) return II2_EINVAL;
    switch (n_planes) {
        case 1: topw_word_scores<1>(adds, weights, n_adds, mask, scores); break;
        case 2: topw_word_scores<2>(adds, weights, n_adds, mask, scores); break;
        case 3: topw_word_scores<3>(adds, weights, n_adds, mask, scores); break;
        case 4: topw_word_scores<4>(adds, weights, n_adds, mask, scores); break;
        case 5: topw_word_scores<5>(adds, weights, n_adds, mask, scores); break;
        case 6: topw_word_scores<6>(adds, weights, n_adds, mask, scores); break;
        case 7: topw_word_scores<7>(adds, weights, n_adds, mask, scores); break;
        default: topw_word_scores<8>(adds, weights, n_adds, mask, scores); break;
    }
    return II2_OK;
}

// host only: what the weighted ranked query would use for these counted groups
int ii2_topkw_plan(uint64_t n_counted, const uint32_t *weights, const uint64_t *postings, uint32_t min_score, uint32_t window_log2, uint32_t *total_weight,
                   uint32_t *n_planes, uint64_t *window_docs, uint8_t *late, uint32_t *n_late) {
    if (!total_weight || !n_planes || !window_docs || !n_late || !min_score || (n_counted && (!weights || !postings || !late))) return II2_EINVAL;
    uint64_t total = 0;
    for (uint64_t g = 0; g < n_counted; g++) {
        if (!weights[g]) return II2_EINVAL;
        if (weights[g] > 255 || (total += weights[g]) > 255) return II2_ERANGE;
    }
    *total_weight = *n_planes = *n_late = 0u;
    *window_docs = 0;
    for (uint64_t g = 0; g < n_counted; g++) late[g] = 0;
    if (min_score > total) return II2_OK;
    *total_weight = (uint32_t)total;
    *n_planes = thr_bit_width(total);
    *window_docs = thr_window_docs(*n_planes, window_log2);
    *n_late = top_late_set(n_counted, weights, postings, min_score, late);
    return II2_OK;
}

}  // extern "C"

// ---- many queries in one call ---------------------------------------------------------------------
// one query of a batch as the host plans it
namespace {
struct BatchPlan {
    uint64_t bound;              // ids its staging slot holds: AND the shortest operand, OR every posting of its ranges
    uint64_t stage_off;
    size_t l0;                   // its lists in the call's flat list array: AND every operand, OR the non-empty ones (at most 65 kept)
    uint32_t nl;
    uint32_t n_blocks;
    uint8_t kind;                // BP_*
    uint8_t is_union;
    uint8_t n_req;               // ii2_query_batch_groups: its required groups when it takes the batch kernel (<= MAX_LISTS)
};
enum { BP_EMPTY = 0, BP_TINY = 1, BP_SMALL = 2, BP_LARGE = 3 };
}  // namespace

// grow-only blocks of the batch path: the device block (never the bump workspace: the large queries of a batch reserve from that)
// and the pinned one
static int batch_reserve(ii2_ctx *ctx, size_t dev_bytes, size_t host_bytes) {
    if (int rc = grow_device(ctx, &ctx->d_batch, &ctx->batch_cap, dev_bytes, align_up(dev_bytes + dev_bytes / 4, 1 << 20), 1, "ii2_query_batch: staging allocation failed"))
        return rc;
    return grow_pinned(ctx, &ctx->h_batch, &ctx->h_batch_cap, host_bytes, true, "ii2_query_batch: pinned staging allocation failed");
}

// The blocks of a batch call, nq queries whose staging slots hold stage_ids ids: [the entry point's table, table_bytes | staging
// offsets | counts] are filled in the pinned block h and travel up in one copy; offsets, scan temp and staged ids stay below.
namespace {
struct BatchMem {
    size_t o_soff, o_cnt, up_bytes, o_off, o_scan, scan_tmp, o_stage;
    uint8_t *h, *d;
    uint32_t *d_stage;
    uint64_t *h_soff;            // [nq] every query's staging slot
    uint32_t *h_cnt;             // [nq + 1] the counts of the queries that no batch kernel answers (theirs: 0); [nq] = 0
    // ranked (ii2_topk_batch) only: the eligible words [nq] close the block that travels up, so they sit right in front of the
    // offsets and come down with them in one copy; the scores are staged in a second region of the staging's size
    size_t o_elig;
    uint32_t *d_stage_scores;
    uint32_t *h_elig;            // [nq] filled like h_cnt
};
}  // namespace
static int batch_blocks(ii2_ctx *ctx, size_t table_bytes, uint64_t nq, uint64_t stage_ids, BatchMem *m, bool ranked = false) {
    m->o_soff = table_bytes;
    m->o_cnt = m->o_soff + align_up(nq * sizeof(uint64_t));
    m->o_elig = m->o_cnt + align_up((nq + 1) * sizeof(uint32_t));
    m->up_bytes = m->o_elig + (ranked ? align_up(nq * sizeof(uint32_t)) : 0);
    const size_t off_bytes = align_up((nq + 1) * sizeof(uint64_t));
    m->scan_tmp = scan_temp_bytes(nq + 1);
    m->o_off = m->up_bytes;
    m->o_scan = m->o_off + off_bytes;
    m->o_stage = m->o_scan + m->scan_tmp;
    const size_t stage_bytes = align_up((stage_ids + 4) * sizeof(uint32_t));
    if (int rc = batch_reserve(ctx, m->o_stage + (ranked ? 2 : 1) * stage_bytes, m->up_bytes + off_bytes)) return rc;
    m->h = (uint8_t *)ctx->h_batch;
    m->d = ctx->d_batch;
    m->d_stage = (uint32_t *)(m->d + m->o_stage);
    m->d_stage_scores = ranked ? (uint32_t *)(m->d + m->o_stage + stage_bytes) : nullptr;
    m->h_soff = (uint64_t *)(m->h + m->o_soff);
    m->h_cnt = (uint32_t *)(m->h + m->o_cnt);
    m->h_elig = ranked ? (uint32_t *)(m->h + m->o_elig) : nullptr;
    return II2_OK;
}

// The end of a batch call, behind its batch kernels: counts -> offsets, pack (tests the capacity on the device), offsets down;
// the call's one wait.  `who` names the entry point in the message.
// ranked (ii2_topk_batch; blocks made with batch_blocks' ranked = true, no path counted): a second pack moves the staged scores
// to d_scores (may be NULL) at the same offsets, and the eligible words come down with the offsets into eligible (may be NULL).
namespace {
struct BatchRanked { uint32_t *d_scores; uint64_t *eligible; };
}  // namespace
static int batch_finish(ii2_ctx *ctx, const char *who, Path pack, const BatchMem &m, uint64_t nq, uint64_t max_bound, uint32_t *d_out, uint64_t cap,
                        uint64_t *out_off, const BatchRanked *ranked = nullptr) {
    hipStream_t st = ctx->stream;
    uint8_t *d = m.d;
    HIP_TRY(ctx, scan_excl_u32_to_u64(d + m.o_scan, m.scan_tmp, (const uint32_t *)(d + m.o_cnt), (uint64_t *)(d + m.o_off), nq + 1, st));
    BatchPackParams pp;
    std::memset(&pp, 0, sizeof pp);
    pp.stage = m.d_stage;
    pp.stage_off = (const uint64_t *)(d + m.o_soff);
    pp.off = (const uint64_t *)(d + m.o_off);
    pp.out = d_out;
    pp.cap = cap;
    pp.n_queries = (uint32_t)nq;
    {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ii2_profile_pair(ctx, &e0, &e1);
        if (!ranked) took(ctx, pack);
        HIP_TRY(ctx, launch_batch_pack(pp, max_bound, st, e0, e1));
    }
    if (ranked && ranked->d_scores) {
        pp.stage = m.d_stage_scores;
        pp.out = ranked->d_scores;
        HIP_TRY(ctx, launch_batch_pack(pp, max_bound, st));
    }
    uint64_t *h_off = (uint64_t *)(m.h + m.up_bytes);
    if (ranked) HIP_TRY(ctx, hipMemcpyAsync(m.h + m.o_elig, d + m.o_elig, m.o_off - m.o_elig + (nq + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    else HIP_TRY(ctx, hipMemcpyAsync(h_off, d + m.o_off, (nq + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    std::memcpy(out_off, h_off, (nq + 1) * sizeof(uint64_t));
    if (ranked && ranked->eligible)
        for (uint64_t q = 0; q < nq; q++) ranked->eligible[q] = m.h_elig[q];
    if (out_off[nq] > cap)
        return fail(ctx, II2_ECAPACITY, (std::string(who) + ": the results do not fit the output buffer (nothing written; out_off holds the sizes)").c_str());
    return II2_OK;
}

// The argument checks every batch call makes, under its name w; have: the arrays the entry point cannot do without are there.
static int batch_args(ii2_ctx *ctx, const std::string &w, bool have, uint64_t nq, const uint32_t *d_out, uint64_t cap, const ii2_tomb *tomb) {
    if (!have) return fail(ctx, II2_EINVAL, (w + ": bad argument").c_str());
    if (nq > BATCH_MAX_QUERIES) return fail(ctx, II2_ERANGE, (w + ": more than 2^20 queries in one call").c_str());
    if (!d_out && cap) return fail(ctx, II2_EINVAL, (w + ": output buffer is NULL").c_str());
    if (tomb && tomb->device != ctx->device) return fail(ctx, II2_EINVAL, (w + ": the tombstones live on another device").c_str());
    return II2_OK;
}
static int batch_bad(ii2_ctx *ctx, const std::string &w, uint64_t q, const char *what) {
    return fail(ctx, II2_EINVAL, (w + ": query " + std::to_string(q) + ": " + what).c_str());
}
// a helper's message "<entry point>: ..." gets the query's index behind the name (built on the error path only)
static int batch_named(ii2_ctx *ctx, const std::string &w, uint64_t q, int rc) {
    if (ctx->err.compare(0, w.size() + 2, w + ": ") == 0) ctx->err.insert(w.size(), ": query " + std::to_string(q));
    return rc;
}
// ... and of the grouped ones: query q owns the groups query_first[q] .. query_first[q + 1] - 1
static int batch_group_args(ii2_ctx *ctx, const std::string &w, uint64_t nq, const uint64_t *query_first, const uint64_t *group_first) {
    if (query_first[0] != 0) return batch_bad(ctx, w, 0, "query_first does not ascend from 0");
    for (uint64_t q = 0; q < nq; q++)
        if (query_first[q + 1] < query_first[q]) return batch_bad(ctx, w, q, "query_first does not ascend from 0");
    if (query_first[nq] && !group_first) return fail(ctx, II2_EINVAL, (w + ": bad argument").c_str());
    if (query_first[nq] && group_first[0] != 0) return batch_bad(ctx, w, 0, "group_first does not ascend from 0");
    return II2_OK;
}

// what the planned queries of a batch add up to: the ids their staging slots hold, the largest slot, the queries of each kind
namespace {
struct BatchTally {
    uint64_t stage_ids = 0, max_bound = 0;
    uint32_t n_kind[4] = {0, 0, 0, 0};
    uint32_t n_table() const { return n_kind[BP_TINY] + n_kind[BP_SMALL]; }              // the queries the batch kernel answers ...
    size_t o_lists() const { return align_up((size_t)n_table() * sizeof(BatchQuery)); }   // ... open the table; their lists follow
};
}  // namespace
// a query is planned (kind, bound): its staging slot follows those before it
// (per-query work, inlined like plan_groups: its cold message keeps the compiler from doing it by itself, +1 - 2 ns a query)
__attribute__((always_inline)) static inline int batch_planned(ii2_ctx *ctx, const std::string &w, BatchPlan &pl, BatchTally &T) {
    T.n_kind[pl.kind]++;
    pl.stage_off = T.stage_ids;
    T.stage_ids += pl.bound;
    T.max_bound = std::max(T.max_bound, pl.bound);
    if (T.stage_ids >= (1ull << 32)) return fail(ctx, II2_ERANGE, (w + ": the result bounds of the queries add up to 2^32 ids or more").c_str());
    return II2_OK;
}

// two-list ANDs in the two-kernel form while it lives: nothing of a batch waits between workgroups
namespace {
struct And2Split {
    ii2_ctx *ctx;
    const int64_t keep;
    explicit And2Split(ii2_ctx *c) : ctx(c), keep(c->opt_intersect_and2) { if (keep == 1) ctx->opt_intersect_and2 = 2; }
    ~And2Split() { ctx->opt_intersect_and2 = keep; }
};
}  // namespace

// The pinned block behind the entry point's table, filled and sent up: every query's staging slot and a count of 0 (batch_blocks).
// On the way the large queries run one after the other, run(q, its plan, &count) writing into their staging slots with the waits
// of the single call - an error gets "<entry point>: query <q>: " in front - and each query the batch kernel answers is given its
// row: put(q, its plan, the row), the tiny ones first.
template <class Run, class Put> __attribute__((always_inline)) static inline int batch_fill(ii2_ctx *ctx, const std::string &w, const std::vector<BatchPlan> &plan, const BatchTally &T, const BatchMem &m,
                                                      Run &&run, Put &&put) {
    const uint64_t nq = plan.size();
    uint32_t at_tiny = 0, at_small = T.n_kind[BP_TINY];
    for (uint64_t q = 0; q < nq; q++) {
        const BatchPlan &pl = plan[q];
        m.h_soff[q] = pl.stage_off;
        m.h_cnt[q] = 0;
        if (m.h_elig) m.h_elig[q] = 0;
        if (pl.kind == BP_EMPTY) continue;
        if (pl.kind == BP_LARGE) {
            uint64_t count = 0;
            if (int rc = run(q, pl, &count)) {
                ctx->err = w + ": query " + std::to_string(q) + ": " + ctx->err;
                return rc;
            }
            m.h_cnt[q] = (uint32_t)std::min<uint64_t>(count, pl.bound);
            continue;
        }
        put(q, pl, pl.kind == BP_TINY ? at_tiny++ : at_small++);
    }
    m.h_cnt[nq] = 0;
    HIP_TRY(ctx, hipMemcpyAsync(m.d, m.h, m.up_bytes, hipMemcpyHostToDevice, ctx->stream));
    return II2_OK;
}

// the table's head, the staging and the counts in a batch kernel's params
static void batch_params(BatchParams &b, const BatchMem &m, size_t o_lists, const BatchTally &T, const ii2_tomb *tomb) {
    b.queries = (const BatchQuery *)m.d;
    b.lists = (const BatchList *)(m.d + o_lists);
    set_tomb(b, tomb);
    b.n_tiny = T.n_kind[BP_TINY];
    b.n_small = T.n_kind[BP_SMALL];
    b.stage = m.d_stage;
    b.cnt = (uint32_t *)(m.d + m.o_cnt);
}

static int query_batch_unlocked(ii2_ctx *ctx, uint64_t nq, const uint8_t *op, const uint64_t *query_first, const ii2_seg *const *segs,
                                const uint64_t *list_first, const uint64_t *list_end, const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap,
                                uint64_t *out_off) {
    const std::string w("ii2_query_batch");
    if (nq == 0) { out_off[0] = 0; return II2_OK; }
    if (int rc = batch_args(ctx, w, op && query_first, nq, d_out, cap, tomb)) return rc;
    auto bad = [&](uint64_t q, const char *what) { return batch_bad(ctx, w, q, what); };
    if (query_first[nq] && (!segs || !list_first || !list_end)) return fail(ctx, II2_EINVAL, "ii2_query_batch: bad argument");
    // 1. every query checked and sized before anything is launched
    std::vector<BatchPlan> plan(nq);
    std::vector<SetList> lists;
    lists.reserve(2 * nq);
    BatchTally T;
    size_t n_table_lists = 0;
    const ii2_seg *mirrored = nullptr;     // the segment whose host mirrors were looked at last
    for (uint64_t q = 0; q < nq; q++) {
        if (op[q] != II2_OP_AND && op[q] != II2_OP_OR) return bad(q, "unknown op");
        const uint64_t r0 = query_first[q], r1 = query_first[q + 1];
        if (r0 > r1 || (q == 0 && r0 != 0)) return bad(q, "query_first does not ascend from 0");
        const bool is_union = op[q] == II2_OP_OR;
        BatchPlan &pl = plan[q];
        pl = BatchPlan{0, 0, lists.size(), 0, 0, BP_EMPTY, (uint8_t)is_union};
        uint64_t n_ops = 0, blocks = 0, post = 0, shortest = ~0ull;
        bool regular = true;       // every kept list's count agrees with its blocks (what the batch kernel's staging relies on)
        for (uint64_t r = r0; r < r1; r++) {
            const ii2_seg *seg = segs[r];
            const uint64_t a = list_first[r], b = list_end[r];
            if (!seg || a > b || b > seg->n_lists) return bad(q, "bad range");
            if (seg->device != ctx->device) return bad(q, "segment lives on another device");
            if (a == b) continue;
            if (seg != mirrored) {             // (both take the segment's lock: once per run of ranges of one segment)
                if (int rc = ii2_seg_host_blk_off(ctx, seg)) return rc;
                if (int rc = ii2_seg_host_cnt(ctx, seg)) return rc;
                mirrored = seg;
            }
            const std::vector<uint32_t> &bo = seg->h_blk_off;
            if (bo[b] > seg->n_blocks) return bad(q, "the segment's list table does not ascend");
            if (!is_union && n_ops + (b - a) > MAX_LISTS) return bad(q, "an AND takes 1..64 lists");
            for (uint64_t j = a; j < b; j++) {
                if (bo[j + 1] < bo[j]) return bad(q, "the segment's list table does not ascend");
                const uint32_t nb = bo[j + 1] - bo[j], c = seg->h_cnt[j];
                n_ops++;
                blocks += nb;
                post += c;
                shortest = std::min<uint64_t>(shortest, c);
                if (is_union && nb == 0) continue;
                if (nb == 0 || !blocks_full(nb, c)) regular = false;
                if (pl.nl <= MAX_LISTS) {              // (an OR of more lists is a large query: it goes by its ranges)
                    lists.push_back(SetList{list_view(seg, j), seg, j});
                    pl.nl++;
                }
            }
        }
        if (!is_union && n_ops == 0) return bad(q, "an AND takes 1..64 lists");
        if (blocks >= 0xFFFFFFFFull) return fail(ctx, II2_ERANGE, "ii2_query_batch: more than 2^32 - 2 blocks in one query");
        pl.n_blocks = (uint32_t)blocks;
        pl.bound = is_union ? post : shortest;
        if (pl.bound == 0 || blocks == 0) { pl.bound = 0; pl.kind = BP_EMPTY; }       // an empty operand / no posting: an empty result, no launch
        else if (!ctx->opt_batch_small || !regular || pl.nl > MAX_LISTS || blocks > SMALL_SET_BLOCKS || post > SMALL_SET_POSTINGS) pl.kind = BP_LARGE;
        else pl.kind = ctx->opt_batch_tiny && blocks <= BATCH_TINY_BLOCKS && post <= BATCH_TINY_POSTINGS ? BP_TINY : BP_SMALL;
        if (pl.kind == BP_TINY || pl.kind == BP_SMALL) n_table_lists += pl.nl;
        if (int rc = batch_planned(ctx, w, pl, T)) return rc;
    }
    // 2. the blocks: [queries | lists | staging offsets | counts] travel up in one copy; offsets, scan temp and staged ids stay below
    const size_t o_lists = T.o_lists();
    BatchMem m;
    if (int rc = batch_blocks(ctx, o_lists + align_up(n_table_lists * sizeof(BatchList)), nq, T.stage_ids, &m)) return rc;
    BatchQuery *hq = (BatchQuery *)m.h;
    BatchList *hl = (BatchList *)(m.h + o_lists);
    // 3. the large queries, one after the other through the single-query paths, into their staging slots (each with its own wait);
    // two-list ANDs in the two-kernel form: nothing of a batch waits between workgroups; the table up
    std::vector<const ii2_seg *> one_segs;
    std::vector<uint64_t> one_idx;
    uint32_t at_list = 0;
    if (int rc = batch_fill(ctx, w, plan, T, m,
            [&](uint64_t q, const BatchPlan &pl, uint64_t *count) -> int {
                took(ctx, P_BATCH_SINGLE);
                uint32_t *slot = m.d_stage + pl.stage_off;
                const uint64_t r0 = query_first[q];
                if (pl.is_union) return union_ranges_unlocked(ctx, query_first[q + 1] - r0, segs + r0, list_first + r0, list_end + r0, tomb, slot, pl.bound, count);
                one_segs.clear();
                one_idx.clear();
                for (uint32_t i = 0; i < pl.nl; i++) { one_segs.push_back(lists[pl.l0 + i].seg); one_idx.push_back(lists[pl.l0 + i].idx); }
                const And2Split split(ctx);
                return intersect_sync(ctx, pl.nl, one_segs.data(), one_idx.data(), tomb, slot, pl.bound, count);
            },
            [&](uint64_t q, const BatchPlan &pl, uint32_t at) {
                hq[at] = BatchQuery{pl.stage_off, (uint32_t)pl.bound, at_list, pl.nl, pl.is_union, (uint32_t)q, 0u};
                for (uint32_t i = 0; i < pl.nl; i++) {
                    const SetList &sl = lists[pl.l0 + i];
                    hl[at_list++] = BatchList{sl.v.skip, sl.v.payload, sl.v.nblk, sl.seg->h_cnt[sl.idx]};
                }
            }))
        return rc;
    // 4. the small queries in one launch per size class, counts -> offsets, pack (tests the capacity on the device), offsets down:
    // one wait
    if (T.n_table()) {
        BatchParams bp;
        std::memset(&bp, 0, sizeof bp);
        batch_params(bp, m, o_lists, T, tomb);
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ii2_profile_pair(ctx, &e0, &e1);
        const uint32_t forms = setop_batch_forms(bp);
        if (forms & BATCH_FORM_TINY) took(ctx, P_BATCH_TINY);
        if (forms & BATCH_FORM_SMALL) took(ctx, P_BATCH_SMALL);
        HIP_TRY(ctx, launch_setop_batch(bp, ctx->stream, e0, e1));
    }
    return batch_finish(ctx, "ii2_query_batch", P_BATCH_PACK, m, nq, T.max_bound, d_out, cap, out_off);
}

extern "C" int ii2_query_batch(ii2_ctx *ctx, uint64_t n_queries, const uint8_t *op, const uint64_t *query_first, const ii2_seg *const *segs,
                               const uint64_t *list_first, const uint64_t *list_end, const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap,
                               uint64_t *out_off) {
    if (!ctx || !out_off) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return query_batch_unlocked(ctx, n_queries, op, query_first, segs, list_first, list_end, tomb, d_out, cap, out_off);
}

// ---- many AND-of-ORs / NOT queries in one call ------------------------------------------------------
// Query q owns the groups query_first[q] .. query_first[q + 1] - 1 of an ii2_andnot_ranges call; its result is that call's.
// Every query is planned as that call plans it (plan_groups, size_exclusions, for_each_counted_list); what differs is where a
// short query runs.
static int query_batch_groups_unlocked(ii2_ctx *ctx, uint64_t nq, const uint64_t *query_first, const uint64_t *group_first, const uint8_t *group_not,
                                       const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end, const ii2_tomb *tomb,
                                       uint32_t *d_out, uint64_t cap, uint64_t *out_off) {
    const char *const who = "ii2_query_batch_groups";
    const std::string w(who);
    if (nq == 0) { out_off[0] = 0; return II2_OK; }
    if (int rc = batch_args(ctx, w, query_first, nq, d_out, cap, tomb)) return rc;
    if (int rc = batch_group_args(ctx, w, nq, query_first, group_first)) return rc;
    // 1. every query checked and sized before anything is launched
    std::vector<BatchPlan> plan(nq);
    std::vector<BatchList> tl;             // the table's lists and their tags, the queries in batch order (tiny and small ones alike)
    std::vector<uint8_t> tt;
    GroupQuery gq;                          // (one for the call: its vectors keep their storage from query to query)
    BatchTally T;
    for (uint64_t q = 0; q < nq; q++) {
        const uint64_t g0 = query_first[q], ng = query_first[q + 1] - g0;
        BatchPlan &pl = plan[q];
        pl = BatchPlan{0, 0, tl.size(), 0, 0, BP_EMPTY, 0, 0};
        if (int rc = plan_groups(ctx, who, "query", ng, group_first + g0, group_not ? group_not + g0 : nullptr, segs, list_first, list_end, gq))
            return batch_named(ctx, w, q, rc);
        if (!gq.empty) {
            pl.bound = gq.shortest;
            pl.kind = BP_LARGE;
        }
        // A query fits the batch kernel when the lists that count fit one workgroup (for_each_counted_list).  ANDNOT_SMALL_WORK is
        // NOT applied: that bound prices one workgroup against the general form's waits inside a single call; in a batch the
        // alternative is those waits once per query, one after the other, while the other CUs sit idle (DESIGN.md §4.1i has the
        // case at the kernel's capacity).
        if (pl.kind == BP_LARGE && ctx->opt_batch_groups && gq.req.size() <= MAX_LISTS) {
            // (size_exclusions' totals and narrowed span, a second pass over the excluded lists, are for the general form: the walk
            // mirrors their counts itself, and the lists that count are the same under either span)
            const Counted t = for_each_counted_list(ctx, gq, [&](const ii2_seg *s, uint64_t j, uint32_t tag, const Counted &) {
                const uint32_t b0 = s->h_blk_off[j];
                tl.push_back(BatchList{s->d_skip + b0, s->d_payload, s->h_blk_off[j + 1] - b0, s->h_cnt[j]});
                tt.push_back((uint8_t)tag);
            });
            if (t.rc) return t.rc;
            if (t.fits) {
                pl.nl = t.m;
                pl.n_blocks = t.nb;
                pl.kind = ctx->opt_batch_tiny && t.nb <= BATCH_TINY_BLOCKS && t.sum <= BATCH_TINY_POSTINGS ? BP_TINY : BP_SMALL;
                pl.n_req = (uint8_t)gq.req.size();
            } else {
                tl.resize(pl.l0);
                tt.resize(pl.l0);
            }
        }
        if (int rc = batch_planned(ctx, w, pl, T)) return rc;
    }
    // 2. the blocks: [queries | lists | tags | staging offsets | counts] travel up in one copy (batch_blocks)
    const size_t o_lists = T.o_lists(), o_tags = o_lists + align_up(tl.size() * sizeof(BatchList));
    BatchMem m;
    if (int rc = batch_blocks(ctx, o_tags + align_up(tt.size()), nq, T.stage_ids, &m)) return rc;
    BatchQuery *hq = (BatchQuery *)m.h;
    if (!tl.empty()) {
        std::memcpy(m.h + o_lists, tl.data(), tl.size() * sizeof(BatchList));
        std::memcpy(m.h + o_tags, tt.data(), tt.size());
    }
    // 3. the large queries, one after the other through ii2_andnot_ranges' paths, into their staging slots (each with its own
    // waits); two-list ANDs in the two-kernel form for the duration: nothing of a batch waits between workgroups; the table up
    if (int rc = batch_fill(ctx, w, plan, T, m,
            [&](uint64_t q, const BatchPlan &pl, uint64_t *count) -> int {
                took(ctx, P_GBATCH_SINGLE);
                const uint64_t g0 = query_first[q];
                const And2Split split(ctx);
                return andnot_ranges_unlocked(ctx, query_first[q + 1] - g0, group_first + g0, group_not ? group_not + g0 : nullptr, segs, list_first,
                                              list_end, tomb, m.d_stage + pl.stage_off, pl.bound, count);
            },
            [&](uint64_t q, const BatchPlan &pl, uint32_t at) {
                hq[at] = BatchQuery{pl.stage_off, (uint32_t)pl.bound, (uint32_t)pl.l0, pl.nl, 0u, (uint32_t)q, pl.n_req};
            }))
        return rc;
    // 4. the queries that fit in one launch per size class, then the flat batch's scan, pack and wait (batch_finish)
    if (T.n_table()) {
        GroupBatchParams gp;
        std::memset(&gp, 0, sizeof gp);
        batch_params(gp.b, m, o_lists, T, tomb);
        gp.tag = m.d + o_tags;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ii2_profile_pair(ctx, &e0, &e1);
        const uint32_t forms = setop_groups_batch_forms(gp);
        if (forms & BATCH_FORM_TINY) took(ctx, P_GBATCH_TINY);
        if (forms & BATCH_FORM_SMALL) took(ctx, P_GBATCH_SMALL);
        HIP_TRY(ctx, launch_setop_groups_batch(gp, ctx->stream, e0, e1));
    }
    return batch_finish(ctx, who, P_GBATCH_PACK, m, nq, T.max_bound, d_out, cap, out_off);
}

extern "C" int ii2_query_batch_groups(ii2_ctx *ctx, uint64_t n_queries, const uint64_t *query_first, const uint64_t *group_first,
                                      const uint8_t *group_not, const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end,
                                      const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap, uint64_t *out_off) {
    if (!ctx || !out_off) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return query_batch_groups_unlocked(ctx, n_queries, query_first, group_first, group_not, segs, list_first, list_end, tomb, d_out, cap, out_off);
}

// ---- many ranked queries in one call ------------------------------------------------------------
// The form a planned ranked query takes in a batch: n_lists counted lists (for_each_counted_list; `fits`: the walk saw every one)
// of n_post postings in n_blocks blocks, n_counted required groups with postings.  The host planner and ii2_topk_batch_plan call it.
static_assert(BP_EMPTY == II2_TOPK_BATCH_EMPTY && BP_TINY == II2_TOPK_BATCH_TINY && BP_SMALL == II2_TOPK_BATCH_SMALL && BP_LARGE == II2_TOPK_BATCH_SINGLE,
              "ii2_topk_batch_plan reports the planner's kinds");
static uint8_t topk_batch_form(bool fits, uint64_t n_lists, uint64_t n_post, uint64_t n_blocks, uint64_t n_counted, int64_t opt_topk, int64_t opt_tiny) {
    if (!n_counted) return BP_EMPTY;
    if (!opt_topk || !fits || n_counted > MAX_LISTS || n_lists > MAX_LISTS || n_post > SMALL_SET_POSTINGS || n_blocks > SMALL_SET_BLOCKS) return BP_LARGE;
    return opt_tiny && n_blocks <= BATCH_TINY_BLOCKS && n_post <= BATCH_TINY_POSTINGS ? BP_TINY : BP_SMALL;
}
static uint64_t topk_batch_bound(uint64_t n_counted, uint64_t req_post, uint64_t k) { return n_counted ? std::min(k, req_post) : 0; }

// Query q owns the groups query_first[q] .. query_first[q + 1] - 1 of an ii2_topk_weighted_ranges call; its result is that call's.
// Every query is planned as that call plans it (topkw_plan, for_each_counted_list); what differs is where a short query runs.
static int topk_batch_unlocked(ii2_ctx *ctx, uint64_t nq, const uint64_t *query_first, const uint64_t *group_first, const uint8_t *group_not,
                               const uint32_t *group_weight, const uint32_t *min_score, const uint32_t *k, const ii2_seg *const *segs,
                               const uint64_t *list_first, const uint64_t *list_end, const ii2_tomb *tomb, uint32_t *d_ids, uint32_t *d_scores, uint64_t cap,
                               uint64_t *out_off, uint64_t *eligible, ii2_topk_batch_stats *stats) {
    const char *const who = "ii2_topk_batch";
    const std::string w(who);
    if (nq == 0) {
        out_off[0] = 0;
        if (stats) std::memset(stats, 0, sizeof *stats);
        return II2_OK;
    }
    if (int rc = batch_args(ctx, w, query_first && k, nq, d_ids, cap, tomb)) return rc;
    if (int rc = batch_group_args(ctx, w, nq, query_first, group_first)) return rc;
    // 1. every query checked and sized before anything is launched
    std::vector<BatchPlan> plan(nq);
    std::vector<BatchList> tl;             // the table's lists, their tags and their groups' weights, the queries in batch order
    std::vector<uint8_t> tt, tw;
    GroupQuery gq;
    std::vector<uint64_t> kept;
    std::vector<uint32_t> weights;
    BatchTally T;
    for (uint64_t q = 0; q < nq; q++) {
        const uint64_t g0 = query_first[q], ng = query_first[q + 1] - g0;
        const uint32_t ms = min_score ? min_score[q] : 1u;
        BatchPlan &pl = plan[q];
        pl = BatchPlan{0, 0, tl.size(), 0, 0, BP_EMPTY, 0, 0};
        uint64_t total = 0;
        if (int rc = topkw_plan(ctx, who, ng, group_first + g0, group_not ? group_not + g0 : nullptr, group_weight ? group_weight + g0 : nullptr, ms, k[q],
                                segs, list_first, list_end, gq, kept, weights, &total))
            return batch_named(ctx, w, q, rc);
        if (!gq.empty && ms <= total) {
            uint64_t req_post = 0;
            for (const GroupIn &G : gq.req) req_post += G.n_post;
            pl.bound = topk_batch_bound(gq.req.size(), req_post, k[q]);
            // A query takes the batch kernel when the lists that count fit one workgroup (for_each_counted_list), with at most
            // MAX_LISTS tags for its required groups.  As in ii2_query_batch_groups the walk mirrors the excluded segments' counts
            // itself, and no postings x lists bound applies: the alternative is the single form's waits once per query.
            Counted t{0, 0, 0, false, II2_OK};
            if (ctx->opt_batch_topk && gq.req.size() <= MAX_LISTS) {
                t = for_each_counted_list(ctx, gq, [&](const ii2_seg *s, uint64_t j, uint32_t tag, const Counted &) {
                    const uint32_t b0 = s->h_blk_off[j];
                    tl.push_back(BatchList{s->d_skip + b0, s->d_payload, s->h_blk_off[j + 1] - b0, s->h_cnt[j]});
                    tt.push_back((uint8_t)tag);
                    tw.push_back(tag < weights.size() ? (uint8_t)weights[tag] : (uint8_t)0);
                });
                if (t.rc) return t.rc;
            }
            pl.kind = topk_batch_form(t.fits, t.m, t.sum, t.nb, gq.req.size(), ctx->opt_batch_topk, ctx->opt_batch_tiny);
            if (pl.kind == BP_LARGE) {
                tl.resize(pl.l0);
                tt.resize(pl.l0);
                tw.resize(pl.l0);
            } else {
                pl.nl = t.m;
                pl.n_blocks = t.nb;
                pl.n_req = (uint8_t)gq.req.size();
            }
        }
        if (int rc = batch_planned(ctx, w, pl, T)) return rc;
    }
    const ii2_topk_batch_stats bst{T.n_kind[BP_TINY], T.n_kind[BP_SMALL], T.n_kind[BP_LARGE], T.n_kind[BP_EMPTY], T.stage_ids};
    // 2. the blocks: [queries | lists | tags | weights | min_scores | staging offsets | counts | eligible] travel up in one copy
    const size_t o_lists = T.o_lists(), o_tags = o_lists + align_up(tl.size() * sizeof(BatchList));
    const size_t o_weights = o_tags + align_up(tt.size()), o_ms = o_weights + align_up(tw.size());
    BatchMem m;
    if (int rc = batch_blocks(ctx, o_ms + align_up((size_t)T.n_table() * sizeof(uint32_t)), nq, T.stage_ids, &m, true)) return rc;
    BatchQuery *hq = (BatchQuery *)m.h;
    uint32_t *hms = (uint32_t *)(m.h + o_ms);
    if (!tl.empty()) {
        std::memcpy(m.h + o_lists, tl.data(), tl.size() * sizeof(BatchList));
        std::memcpy(m.h + o_tags, tt.data(), tt.size());
        std::memcpy(m.h + o_weights, tw.data(), tw.size());
    }
    // 3. the queries that do not fit, one after the other through ii2_topk_weighted_ranges' form, ids and scores straight into their
    // staging slots (each with that form's own waits); the table up
    if (int rc = batch_fill(ctx, w, plan, T, m,
            [&](uint64_t q, const BatchPlan &pl, uint64_t *count) -> int {
                const uint64_t g0 = query_first[q];
                ii2_topkw_stats ws;
                if (int rc = topkw_ranges_unlocked(ctx, query_first[q + 1] - g0, group_first + g0, group_not ? group_not + g0 : nullptr,
                                                   group_weight ? group_weight + g0 : nullptr, min_score ? min_score[q] : 1u, k[q], segs, list_first, list_end,
                                                   tomb, m.d_stage + pl.stage_off, m.d_stage_scores + pl.stage_off, count, nullptr, &ws))
                    return rc;
                m.h_elig[q] = (uint32_t)std::min<uint64_t>(ws.n_eligible, 0xFFFFFFFFull);
                return II2_OK;
            },
            [&](uint64_t q, const BatchPlan &pl, uint32_t at) {
                hq[at] = BatchQuery{pl.stage_off, (uint32_t)pl.bound, (uint32_t)pl.l0, pl.nl, 0u, (uint32_t)q, pl.n_req};
                hms[at] = min_score ? min_score[q] : 1u;
            }))
        return rc;
    // 4. the queries that fit in one launch per size class, then the flat batch's scan, pack (ids, then scores) and wait
    if (T.n_table()) {
        TopkBatchParams tp;
        std::memset(&tp, 0, sizeof tp);
        batch_params(tp.g.b, m, o_lists, T, tomb);
        tp.g.tag = m.d + o_tags;
        tp.weight = m.d + o_weights;
        tp.min_score = (const uint32_t *)(m.d + o_ms);
        tp.stage_scores = m.d_stage_scores;
        tp.eligible = (uint32_t *)(m.d + m.o_elig);
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ii2_profile_pair(ctx, &e0, &e1);
        HIP_TRY(ctx, launch_topk_batch(tp, ctx->stream, e0, e1));
    }
    const BatchRanked ranked{d_scores, eligible};
    const int rc = batch_finish(ctx, who, P_COUNT, m, nq, T.max_bound, d_ids, cap, out_off, &ranked);
    if (stats && (rc == II2_OK || rc == II2_ECAPACITY)) *stats = bst;
    return rc;
}

extern "C" int ii2_topk_batch(ii2_ctx *ctx, uint64_t n_queries, const uint64_t *query_first, const uint64_t *group_first, const uint8_t *group_not,
                              const uint32_t *group_weight, const uint32_t *min_score, const uint32_t *k, const ii2_seg *const *segs,
                              const uint64_t *list_first, const uint64_t *list_end, const ii2_tomb *tomb, uint32_t *d_ids, uint32_t *d_scores, uint64_t cap,
                              uint64_t *out_off, uint64_t *eligible, ii2_topk_batch_stats *stats) {
    if (!ctx || !out_off) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return topk_batch_unlocked(ctx, n_queries, query_first, group_first, group_not, group_weight, min_score, k, segs, list_first, list_end, tomb, d_ids,
                               d_scores, cap, out_off, eligible, stats);
}

// host only: the batch kernel's run rule
extern "C" int ii2_topk_batch_run(const uint8_t *tags, uint32_t n_tags, uint32_t n_req, const uint8_t *weights, uint32_t *score, uint32_t *excluded) {
    if (!tags || !weights || !score || !excluded || !n_tags || n_tags > MAX_LISTS + 1 || n_req > MAX_LISTS) return II2_EINVAL;
    for (uint32_t i = 0; i < n_tags; i++)
        if (tags[i] > n_req) return II2_EINVAL;
    bool ex = false;
    *score = tb_run_score([&](uint32_t i) { return i < n_tags ? (uint32_t)tags[i] : TB_RUN_END; }, [&](uint32_t t) { return (uint32_t)weights[t]; }, n_req, &ex);
    *excluded = ex ? 1u : 0u;
    return II2_OK;
}

// host only: the form and the bound the planner above gives a query
extern "C" int ii2_topk_batch_plan(uint64_t n_lists, uint64_t n_postings, uint64_t n_blocks, uint64_t n_counted, uint64_t req_postings, uint64_t k,
                                   int64_t batch_topk, int64_t batch_tiny, uint32_t *form, uint64_t *bound) {
    if (!form || !bound) return II2_EINVAL;
    *form = topk_batch_form(true, n_lists, n_postings, n_blocks, n_counted, batch_topk, batch_tiny);
    *bound = topk_batch_bound(n_counted, req_postings, k);
    return II2_OK;
}

// ---- many explains in one call ------------------------------------------------------------------
// The form a query of ii2_explain_batch takes: n_lists non-empty lists (`fits`: the walk saw every one and each is regular) of
// n_post postings in n_blocks blocks, n_ids ids.  The host planner and ii2_explain_batch_plan call it.
static_assert(BP_EMPTY == II2_EXPLAIN_BATCH_EMPTY && BP_TINY == II2_EXPLAIN_BATCH_TINY && BP_SMALL == II2_EXPLAIN_BATCH_SMALL && BP_LARGE == II2_EXPLAIN_BATCH_SINGLE,
              "ii2_explain_batch_plan reports the planner's kinds");
static uint8_t explain_batch_form(bool fits, uint64_t n_lists, uint64_t n_post, uint64_t n_blocks, uint64_t n_ids, int64_t opt_explain, int64_t opt_tiny) {
    if (!n_ids || !n_blocks) return BP_EMPTY;
    if (!opt_explain || !fits || n_ids > II2_EXPLAIN_BATCH_IDS || n_lists > MAX_LISTS || n_post > SMALL_SET_POSTINGS || n_blocks > SMALL_SET_BLOCKS) return BP_LARGE;
    return opt_tiny && n_blocks <= BATCH_TINY_BLOCKS && n_post <= BATCH_TINY_POSTINGS ? BP_TINY : BP_SMALL;
}

// Query q owns the groups query_first[q] .. query_first[q + 1] - 1 of an ii2_explain_ranges call and the ids d_ids[ids_off[q] ..
// ids_off[q + 1]); its rows are that call's.  Nothing is staged, scanned or packed: every row's place follows from the arguments.
static int explain_batch_unlocked(ii2_ctx *ctx, uint64_t nq, const uint64_t *query_first, const uint64_t *group_first, const ii2_seg *const *segs,
                                  const uint64_t *list_first, const uint64_t *list_end, const uint32_t *d_ids, const uint64_t *ids_off, uint64_t *d_masks,
                                  uint64_t masks_cap, uint64_t *mask_off, ii2_explain_batch_stats *stats) {
    const char *const who = "ii2_explain_batch";
    const std::string w(who);
    if (nq > BATCH_MAX_QUERIES) return fail(ctx, II2_ERANGE, (w + ": more than 2^20 queries in one call").c_str());
    if (nq == 0) {
        if (mask_off) mask_off[0] = 0;
        if (stats) std::memset(stats, 0, sizeof *stats);
        return II2_OK;
    }
    if (!query_first || !ids_off) return fail(ctx, II2_EINVAL, (w + ": bad argument").c_str());
    if (int rc = batch_group_args(ctx, w, nq, query_first, group_first)) return rc;
    if (ids_off[0] != 0) return batch_bad(ctx, w, 0, "ids_off does not ascend from 0");
    for (uint64_t q = 0; q < nq; q++)
        if (ids_off[q + 1] < ids_off[q]) return batch_bad(ctx, w, q, "ids_off does not ascend from 0");
    // 1. every query checked and sized before anything is launched or written
    std::vector<BatchPlan> plan(nq);
    std::vector<uint64_t> moff(nq + 1);
    std::vector<BatchList> tl;             // the table's lists and their groups, the queries in batch order
    std::vector<uint32_t> tg;
    std::vector<RangeIn> rs;
    std::vector<GroupIn> gs;
    BatchTally T;
    moff[0] = 0;
    for (uint64_t q = 0; q < nq; q++) {
        const uint64_t g0 = query_first[q], ng = query_first[q + 1] - g0, n_ids = ids_off[q + 1] - ids_off[q];
        BatchPlan &pl = plan[q];
        pl = BatchPlan{0, 0, tl.size(), 0, 0, BP_EMPTY, 0, 0};
        if (n_ids > II2_EXPLAIN_MAX_IDS) return fail(ctx, II2_ERANGE, (w + ": query " + std::to_string(q) + ": more than II2_EXPLAIN_MAX_IDS ids").c_str());
        if (ng >= 0xFFFFFFFFull) return fail(ctx, II2_ERANGE, (w + ": query " + std::to_string(q) + ": 2^32 - 1 groups or more").c_str());
        const uint64_t n_words = (ng + 63) / 64, n_out = n_ids * n_words;
        moff[q + 1] = moff[q] + n_out;
        uint64_t n_blocks = 0;
        rs.clear();
        if (ng) {
            if (int rc = collect_groups(ctx, who, ng, group_first + g0, segs, list_first, list_end, rs, gs, &n_blocks)) return batch_named(ctx, w, q, rc);
            if (n_blocks >= 0xFFFFFFFFull || rs.size() >= 0xFFFFFFFFull)
                return fail(ctx, II2_ERANGE, (w + ": query " + std::to_string(q) + ": more than 2^32 - 2 blocks").c_str());
        }
        if (n_out && (!d_ids || !d_masks)) return batch_bad(ctx, w, q, "ids or masks is NULL");
        // A query takes the batch kernel when its non-empty lists, group by group, fit one workgroup and its page fits the LDS
        // table.  No postings x lists bound applies: the alternative is the single form's waits once per query.
        Counted t{0, 0, 0, ctx->opt_batch_explain && n_ids && n_ids <= II2_EXPLAIN_BATCH_IDS && n_blocks && n_blocks <= SMALL_SET_BLOCKS, II2_OK};
        for (uint64_t g = 0; t.fits && g < ng; g++)
            for (size_t r = gs[g].r0; t.fits && r < gs[g].r1; r++) {
                const ii2_seg *s = rs[r].seg;
                if (int rc = ii2_seg_host_cnt(ctx, s)) return rc;
                for (uint64_t j = rs[r].l0; j < rs[r].l1; j++) {
                    const uint32_t b0 = s->h_blk_off[j], nb = s->h_blk_off[j + 1] - b0, c = s->h_cnt[j];
                    if (!nb) continue;
                    if (t.m == MAX_LISTS || t.sum + c > SMALL_SET_POSTINGS || !blocks_full(nb, c)) { t.fits = false; break; }
                    tl.push_back(BatchList{s->d_skip + b0, s->d_payload, nb, c});
                    tg.push_back((uint32_t)g);
                    t.m++;
                    t.nb += nb;
                    t.sum += c;
                }
            }
        pl.kind = explain_batch_form(t.fits, t.m, t.sum, t.fits ? t.nb : n_blocks, n_ids, ctx->opt_batch_explain, ctx->opt_batch_tiny);
        if (pl.kind == BP_TINY || pl.kind == BP_SMALL) {
            pl.nl = t.m;
            pl.n_blocks = t.nb;
        } else {
            tl.resize(pl.l0);
            tg.resize(pl.l0);
        }
        if (int rc = batch_planned(ctx, w, pl, T)) return rc;
    }
    if (ids_off[nq] >= (1ull << 32)) return fail(ctx, II2_ERANGE, (w + ": 2^32 rows or more in one call").c_str());
    if (mask_off) std::memcpy(mask_off, moff.data(), (nq + 1) * sizeof(uint64_t));
    if (masks_cap < moff[nq]) return fail(ctx, II2_ECAPACITY, (w + ": masks holds fewer words than the rows of all queries (nothing written; mask_off holds the places)").c_str());
    ii2_explain_batch_stats bst{T.n_kind[BP_TINY], T.n_kind[BP_SMALL], T.n_kind[BP_LARGE], T.n_kind[BP_EMPTY], ids_off[nq], moff[nq], 0};
    // 2. the blocks: [queries | lists | groups | pages | staging offsets (unused) | hit counts] travel up in one copy
    const size_t o_lists = T.o_lists(), o_grp = o_lists + align_up(tl.size() * sizeof(BatchList));
    const size_t o_pages = o_grp + align_up(tg.size() * sizeof(uint32_t));
    BatchMem m;
    if (int rc = batch_blocks(ctx, o_pages + align_up((size_t)T.n_table() * sizeof(ExplainBatchQuery)), nq, 0, &m)) return rc;
    BatchQuery *hq = (BatchQuery *)m.h;
    ExplainBatchQuery *hx = (ExplainBatchQuery *)(m.h + o_pages);
    if (!tl.empty()) {
        std::memcpy(m.h + o_lists, tl.data(), tl.size() * sizeof(BatchList));
        std::memcpy(m.h + o_grp, tg.data(), tg.size() * sizeof(uint32_t));
    }
    // 3. every row zero, in front of everything that sets a bit; then the queries that do not fit, one after the other through
    // ii2_explain_ranges' form on their own slices (each with that form's waits); the table up
    if (moff[nq]) HIP_TRY(ctx, hipMemsetAsync(d_masks, 0, moff[nq] * sizeof(uint64_t), ctx->stream));
    if (int rc = batch_fill(ctx, w, plan, T, m,
            [&](uint64_t q, const BatchPlan &, uint64_t *) -> int {
                const uint64_t g0 = query_first[q];
                ii2_explain_stats es;
                if (int rc = explain_ranges_unlocked(ctx, query_first[q + 1] - g0, group_first + g0, segs, list_first, list_end, d_ids + ids_off[q],
                                                     ids_off[q + 1] - ids_off[q], d_masks + moff[q], moff[q + 1] - moff[q], &es, true))
                    return rc;
                bst.n_hits += es.n_hits;
                return II2_OK;
            },
            [&](uint64_t q, const BatchPlan &pl, uint32_t at) {
                hq[at] = BatchQuery{moff[q], (uint32_t)(ids_off[q + 1] - ids_off[q]), (uint32_t)pl.l0, pl.nl, 0u, (uint32_t)q, 0u};
                hx[at] = ExplainBatchQuery{ids_off[q], (uint32_t)((query_first[q + 1] - query_first[q] + 63) / 64), 0u};
            }))
        return rc;
    // 4. the queries that fit in one launch per size class; their hit counts down: the call's one wait
    if (T.n_table()) {
        ExplainBatchParams xp;
        std::memset(&xp, 0, sizeof xp);
        batch_params(xp.b, m, o_lists, T, nullptr);
        xp.grp = (const uint32_t *)(m.d + o_grp);
        xp.pages = (const ExplainBatchQuery *)(m.d + o_pages);
        xp.ids = d_ids;
        xp.masks = (unsigned long long *)d_masks;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ii2_profile_pair(ctx, &e0, &e1);
        HIP_TRY(ctx, launch_explain_batch(xp, ctx->stream, e0, e1));
        uint32_t *h_hits = (uint32_t *)(m.h + m.up_bytes);
        HIP_TRY(ctx, hipMemcpyAsync(h_hits, m.d + m.o_cnt, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (uint64_t q = 0; q < nq; q++) bst.n_hits += h_hits[q];
    } else if (moff[nq]) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));              // (the zeroed rows of queries for which nothing ran)
    }
    if (stats) *stats = bst;
    return II2_OK;
}

extern "C" int ii2_explain_batch(ii2_ctx *ctx, uint64_t n_queries, const uint64_t *query_first, const uint64_t *group_first, const ii2_seg *const *segs,
                                 const uint64_t *list_first, const uint64_t *list_end, const uint32_t *d_ids, const uint64_t *ids_off, uint64_t *d_masks,
                                 uint64_t masks_cap, uint64_t *mask_off, ii2_explain_batch_stats *stats) {
    if (!ctx) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return explain_batch_unlocked(ctx, n_queries, query_first, group_first, segs, list_first, list_end, d_ids, ids_off, d_masks, masks_cap, mask_off, stats);
}

// host only: the form the planner above gives a query
extern "C" int ii2_explain_batch_plan(uint64_t n_lists, uint64_t n_postings, uint64_t n_blocks, uint64_t n_ids, int64_t batch_explain, int64_t batch_tiny,
                                      uint32_t *form) {
    if (!form) return II2_EINVAL;
    *form = explain_batch_form(true, n_lists, n_postings, n_blocks, n_ids, batch_explain, batch_tiny);
    return II2_OK;
}

extern "C" {

// ---- host-buffer convenience -----------------------------------------------------------------
static int lists_host(ii2_ctx *ctx, bool is_union, uint32_t n, const uint64_t *list_off, const uint32_t *values,
                      const uint32_t *removed, uint64_t n_removed, uint32_t *out, uint64_t cap, uint64_t *count) {
    if (!ctx || !list_off || !count || n == 0 || n > MAX_LISTS) return fail(ctx, II2_EINVAL, "bad argument");
    ii2_seg *seg = nullptr;
    ii2_tomb *tomb = nullptr;
    int rc = ii2_seg_encode(ctx, n, list_off, values, II2_HOST, &seg);
    if (!rc && n_removed) rc = ii2_tomb_create(ctx, removed, n_removed, II2_HOST, &tomb);
    if (!rc) {
        uint64_t bound = 0;
        if (is_union) bound = list_off[n] - list_off[0];
        else {
            bound = ~0ull;
            for (uint32_t i = 0; i < n; i++) bound = std::min<uint64_t>(bound, list_off[i + 1] - list_off[i]);
        }
        DevBuf d_out;
        if (d_out.alloc((bound + 1) * sizeof(uint32_t)) != hipSuccess) rc = fail(ctx, II2_ENOMEM, "result allocation failed");
        std::vector<const ii2_seg *> segs(n, seg);
        std::vector<uint64_t> idx(n);
        for (uint32_t i = 0; i < n; i++) idx[i] = i;
        uint64_t c = 0;
        if (!rc)
            rc = is_union ? ii2_union(ctx, n, segs.data(), idx.data(), tomb, d_out.as<uint32_t>(), bound + 1, &c)
                          : ii2_intersect(ctx, n, segs.data(), idx.data(), tomb, d_out.as<uint32_t>(), bound + 1, &c);
        if (!rc && c > cap) rc = fail(ctx, II2_ECAPACITY, "output buffer too small; nothing was written");
        if (!rc && c) {
            if (!out) rc = fail(ctx, II2_EINVAL, "output buffer is NULL");
            else rc = ii2_copy_d2h(ctx, out, d_out.p, c * sizeof(uint32_t));
        }
        if (!rc) *count = c;
    }
    ii2_seg_free(seg);
    ii2_tomb_free(tomb);
    return rc;
}

int ii2_intersect_host(ii2_ctx *ctx, uint32_t n, const uint64_t *list_off, const uint32_t *values, const uint32_t *removed,
                       uint64_t n_removed, uint32_t *out, uint64_t cap, uint64_t *count) {
    return lists_host(ctx, false, n, list_off, values, removed, n_removed, out, cap, count);
}

int ii2_union_host(ii2_ctx *ctx, uint32_t n, const uint64_t *list_off, const uint32_t *values, const uint32_t *removed,
                   uint64_t n_removed, uint32_t *out, uint64_t cap, uint64_t *count) {
    return lists_host(ctx, true, n, list_off, values, removed, n_removed, out, cap, count);
}

}  // extern "C"
