// setop.cpp — AND / OR of posting lists (include/ii2.h): ii2_intersect(_async), ii2_union and their host-buffer forms.
// A call collects its lists once, then takes the first path of its chooser that fits:
//   AND: a list is empty (count 0), the small kernel (setop_small.hip), the dense forms - and2 in one launch, and2 in two
//        kernels (intersect_and2.hip), n-list dense (intersect_dense.hip) - then the tiles (intersect.hip).
//   OR:  the small kernel, rank (union_rank.hip), stream (intersect_dense.hip), the byte-map tiles (intersect.hip), then
//        the merge passes (ops.cpp: merge_core).
//   OR of list ranges (ii2_union_ranges): up to 64 non-empty lists the OR chooser above, more lists block by block
//        (union_many.hip).
#include <algorithm>
#include <cstring>
#include <vector>

#include "internal.h"

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

// the n lists of a call, checked and viewed once (a union names every rejection "ii2_union: bad list")
static int collect_lists(ii2_ctx *ctx, bool is_union, uint32_t n, const ii2_seg *const *segs, const uint64_t *list_idx, SetList *L) {
    for (uint32_t i = 0; i < n; i++) {
        const ii2_seg *seg = segs[i];
        const uint64_t idx = list_idx ? list_idx[i] : 0;
        if (!seg || idx >= seg->n_lists) return fail(ctx, II2_EINVAL, is_union ? "ii2_union: bad list" : "list index out of range");
        if (seg->device != ctx->device) return fail(ctx, II2_EINVAL, is_union ? "ii2_union: bad list" : "segment lives on another device");
        if (int rc = ii2_seg_host_blk_off(ctx, seg)) return rc;
        const uint32_t b0 = seg->h_blk_off[idx], b1 = seg->h_blk_off[idx + 1];
        L[i] = SetList{ListView{seg->d_skip + b0, seg->d_payload, seg->d_last_doc + idx, b1 - b0, 0u}, seg, idx};
    }
    return II2_OK;
}

// the output and tombstone fields of every kernel's parameters
template <class P> static void set_out(P &p, const SetOut &o) {
    p.tomb = o.tomb ? o.tomb->d_words : nullptr;
    p.tomb_nwords = o.tomb ? (uint32_t)std::min<uint64_t>(o.tomb->n_words, 0xFFFFFFFFull) : 0;
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
    if (seg->h_spans.size() == 3 * seg->n_lists && idx < seg->n_lists) {      // mirrored when the segment was created: no fetch, no sync
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
    HIP_TRY(ctx, hipMemcpyAsync(&e[0], l.v.skip, sizeof(ii2_skip), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(&e[1], l.v.skip + (l.v.nblk - 1), sizeof(ii2_skip), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(&last, l.v.last_doc, sizeof last, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *out = ii2_seg::ListSpan{e[0].first_doc, e[1].first_doc, last};
    std::lock_guard<std::mutex> sg(seg->span_mu);
    seg->span_cache[idx] = *out;
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
        // one launch (k_and2_fused): the look-back records live in a buffer of their own (only these kernels write it, every
        // word tagged with its launch's number: nothing to clear between launches)
        if (int rcl = ii2_lookback_prepare(ctx, dp.n_meta / 4u, &dp.lb)) return rcl;
        if (ctx->opt_and2_spin)
            dp.lb.spin = ctx->opt_and2_spin > 0 ? (uint32_t)std::min<int64_t>(ctx->opt_and2_spin, 0x7FFFFFFF) : ctx->opt_and2_spin == -2 ? LB_SPIN_LATE : LB_SPIN_EARLY;
        const double spanA = (double)dp.last_doc[1] - (double)dp.first_doc[1] + 1.0;
        dp.a_scale = (float)((double)L[1].v.nblk / spanA);
        dp.b_dpb = (float)per_block;
    }
    if (ctx->opt_debug_stamps) {
        if (int rcd = ensure_debug(ctx, true)) return rcd;
        dp.debug = ctx->d_debug;
        dp.debug_expand = ctx->opt_debug_stamps == 2 ? 1u : 0u;
    }
    hipStream_t st = ctx->stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ii2_profile_pair(ctx, &e0, &e1);
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
    HIP_TRY(ctx, launch_intersect(p, ctx->stream, e0, e1));
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
    HIP_TRY(ctx, launch_intersect(p, ctx->stream, e0, e1));
    *taken = true;
    return II2_OK;
}

static int union_lists(ii2_ctx *ctx, const SetList *L, uint32_t n, uint64_t blocks_ub, const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap,
                       uint64_t *count);

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
    if (int rc = merge_core(ctx, n, views, 1, blocks_ub, blocks_ub * II2_DV1_BLOCK, tomb, nullptr, d_out, cap, &st)) return rc;
    *count = st.n_out;
    return II2_OK;
}
// ---- OR of list ranges ------------------------------------------------------------------------
// one range of a call, checked: lists [l0, l1) of seg own its blocks [b0, b1)
struct RangeIn {
    const ii2_seg *seg;
    uint64_t l0, l1;
    uint32_t b0, b1;
};

// The block-wise OR (union_many.hip) of the ranges' blocks: per window of the doc range mark, count, scan, compact.
static int union_many(ii2_ctx *ctx, const std::vector<RangeIn> &rs, uint64_t n_blocks, const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap,
                      uint64_t *count) {
    hipStream_t st = ctx->stream;
    const size_t nr = rs.size();
    if (ctx->um_dirty) {        // the last call stopped half-way: its copy from the staging block may still be pending, its marks are still set
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (ctx->d_um_bits) HIP_TRY(ctx, hipMemsetAsync(ctx->d_um_bits, 0, ctx->um_bits_words * sizeof(uint32_t), st));
        ctx->um_dirty = false;
    }
    // range descriptors + block prefix: thousands of entries, through a grow-only pinned block
    const size_t desc_bytes = align_up(nr * sizeof(UmRange)), stage_bytes = desc_bytes + align_up((nr + 1) * sizeof(uint32_t));
    if (ctx->h_um_cap < stage_bytes) {
        if (ctx->h_um) (void)hipHostFree(ctx->h_um);
        ctx->h_um = nullptr;
        ctx->h_um_cap = 0;
        const size_t want = align_up(stage_bytes + stage_bytes / 4, 1 << 16);
        if (hipHostMalloc(&ctx->h_um, want) != hipSuccess) return fail(ctx, II2_ENOMEM, "ii2_union_ranges: staging allocation failed");
        ctx->h_um_cap = want;
    }
    UmRange *hr = (UmRange *)ctx->h_um;
    uint32_t *hpre = (uint32_t *)((uint8_t *)ctx->h_um + desc_bytes);
    uint32_t acc = 0;
    for (size_t r = 0; r < nr; r++) {
        const ii2_seg *s = rs[r].seg;
        hr[r] = UmRange{s->d_skip, s->d_payload, s->d_blk_list, s->d_last_doc, rs[r].b0, rs[r].b1, (uint32_t)rs[r].l0, (uint32_t)rs[r].l1};
        hpre[r] = acc;
        acc += rs[r].b1 - rs[r].b0;
    }
    hpre[nr] = acc;
    // the doc range: from the lists' mirrored spans, else one reduction over the blocks (below, once the descriptors are up)
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    bool mirrored = true;
    for (const RangeIn &q : rs) {
        const ii2_seg *s = q.seg;
        if (s->h_spans.size() != 3 * s->n_lists) { mirrored = false; break; }
        for (uint64_t j = q.l0; j < q.l1; j++) {
            if (s->h_blk_off[j + 1] == s->h_blk_off[j]) continue;
            lo = std::min(lo, s->h_spans[3 * j]);
            hi = std::max(hi, s->h_spans[3 * j + 2]);
        }
    }
    const int64_t wl = std::min<int64_t>(std::max<int64_t>(ctx->opt_union_many_window_log2, 11), 30);
    const uint64_t W = 1ull << wl;                               // docs per window
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
    const uint64_t n_sum_call = (std::min(span, W) + 65535) / 65536;
    const size_t words = n_sum_call * 2048 + n_sum_call;
    if (ctx->um_bits_words < words) {
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (ctx->d_um_bits) (void)hipFree(ctx->d_um_bits);
        ctx->d_um_bits = nullptr;
        ctx->um_bits_words = 0;
        if (ii2::dm_malloc_retry((void **)&ctx->d_um_bits, words * sizeof(uint32_t)) != hipSuccess)
            return fail(ctx, II2_ENOMEM, "ii2_union_ranges: scratch allocation failed");
        ctx->um_bits_words = words;
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_um_bits, 0, words * sizeof(uint32_t), st));
    }
    uint64_t *d_cnt = ii2_mapped_mail(ctx, II2_MAIL_COUNT);
    p.d_count = d_cnt ? d_cnt : ctx->d_mail;
    p.tomb = tomb ? tomb->d_words : nullptr;
    p.tomb_nwords = tomb ? (uint32_t)std::min<uint64_t>(tomb->n_words, 0xFFFFFFFFull) : 0;
    p.out = d_out;
    p.out_cap = cap;
    p.check_window = n_win > 1 ? 1u : 0u;
    p.no_atomics = ctx->opt_union_many_no_atomics ? 1u : 0u;
    const uint64_t target_waves = (uint64_t)ctx->cu_count * 32u;
    p.per_wave = (uint32_t)std::max<uint64_t>(1, (n_blocks + target_waves - 1) / target_waves);
    // several windows whose result may not fit: count first (nothing written), then write
    const bool count_first = n_win > 1 && cap < n_blocks * II2_DV1_BLOCK;
    for (int pass = count_first ? 0 : 1; pass < 2; pass++) {
        p.write = (uint32_t)pass;
        for (uint64_t w = 0; w < n_win; w++) {
            const uint64_t wlo = base + w * W;
            const uint64_t docs = std::min<uint64_t>(W, (uint64_t)hi - wlo + 1);
            p.window = (uint32_t)w;
            p.win_lo = (uint32_t)wlo;
            p.win_docs = (uint32_t)docs;
            p.n_sum = (uint32_t)((docs + 65535) / 65536);
            p.bitmap = ctx->d_um_bits;
            p.summary = ctx->d_um_bits + (size_t)p.n_sum * 2048;
            const uint32_t grid = (uint32_t)std::min<uint64_t>((p.n_sum + 1 + 3) / 4, (uint64_t)ctx->cu_count * 8u);
            hipEvent_t e0 = nullptr, e1 = nullptr;
            ii2_profile_pair(ctx, &e0, &e1);
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

static int union_ranges_unlocked(ii2_ctx *ctx, uint64_t n, const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end,
                                 const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap, uint64_t *count) {
    if (n && (!segs || !list_first || !list_end)) return fail(ctx, II2_EINVAL, "ii2_union_ranges: bad argument");
    std::vector<RangeIn> rs;
    uint64_t n_blocks = 0, n_nonempty = 0;
    for (uint64_t i = 0; i < n; i++) {
        const ii2_seg *seg = segs[i];
        const uint64_t l0 = list_first[i], l1 = list_end[i];
        if (!seg || l0 > l1 || l1 > seg->n_lists || seg->device != ctx->device) return fail(ctx, II2_EINVAL, "ii2_union_ranges: bad range");
        if (l0 == l1) continue;
        if (int rc = ii2_seg_host_blk_off(ctx, seg)) return rc;
        // the lists [l0, l1) must own the consecutive blocks blk_off[l0] .. blk_off[l1] (views skip only empty lists between
        // selected ones): checked, not assumed
        const std::vector<uint32_t> &bo = seg->h_blk_off;
        for (uint64_t j = l0; j < l1; j++) {
            if (bo[j + 1] < bo[j]) return fail(ctx, II2_EINVAL, "ii2_union_ranges: the segment's list table does not ascend");
            n_nonempty += bo[j + 1] > bo[j] ? 1u : 0u;
        }
        if (bo[l1] > seg->n_blocks) return fail(ctx, II2_EINVAL, "ii2_union_ranges: the segment's list table does not ascend");
        if (bo[l1] == bo[l0]) continue;
        rs.push_back(RangeIn{seg, l0, l1, bo[l0], bo[l1]});
        n_blocks += bo[l1] - bo[l0];
    }
    if (!n_blocks) { *count = 0; return II2_OK; }
    if (n_blocks >= 0xFFFFFFFFull || rs.size() >= 0xFFFFFFFFull) return fail(ctx, II2_ERANGE, "ii2_union_ranges: more than 2^32 - 2 blocks in one call");
    if (!d_out) return fail(ctx, II2_EINVAL, "ii2_union_ranges: output buffer is NULL");
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
                L[m++] = SetList{ListView{q.seg->d_skip + b0, q.seg->d_payload, q.seg->d_last_doc + j, b1 - b0, 0u}, q.seg, j};
                n_post += cap < n_blocks * II2_DV1_BLOCK ? q.seg->h_cnt[j] : (uint64_t)(b1 - b0) * II2_DV1_BLOCK;
            }
        }
        if (cap >= n_post) return union_lists(ctx, L, m, n_blocks, tomb, d_out, cap, count);
    }
    return union_many(ctx, rs, n_blocks, tomb, d_out, cap, count);
}

extern "C" int ii2_union_ranges(ii2_ctx *ctx, uint64_t n, const ii2_seg *const *segs, const uint64_t *list_first, const uint64_t *list_end,
                                const ii2_tomb *tomb, uint32_t *d_out, uint64_t cap, uint64_t *count) {
    if (!ctx || !count) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return union_ranges_unlocked(ctx, n, segs, list_first, list_end, tomb, d_out, cap, count);
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
